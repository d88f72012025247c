"""Timing of the hold-out pass and of a tracking fit (include/pmf_hip_holdout.h).

    python scripts/kbench_holdout.py [--rounds R] [--shape MxNxK] [--frac F] [--epochs E] [--out profiles/holdout_kbench.json]

One context holds synthetic all-normal data of the shape (default 200000x50000x64, f32 store, two batch views of 8 sorted
batches) of which a fraction F (default 0.01: 1e8 entries) is held out: in every column the rows 1/F t + jitter, t = 0, 1, ...
(sorted, unique, scattered over the whole of X).  In ONE run, after three warm-up rounds, R (default 10) rounds alternate
    holdout       pmf_holdout_loss                    one hold-out pass, the N column sums copied back
    fit           pmf_fit, E epochs, tracking off
    fit+track     the same fit with every = 1, patience = 0, restore_best on
on the host clock (each call is synchronous; every fit restarts from the same factors with a reset optimizer); medians are
printed and written as JSON.  The byte floor of the pass is n (4 Kp + 8): an entry's X column, its row index and its value;
the copy rate it is set against is measured here, a device-to-device copy of 4 GiB through torch, counted as bytes read plus
bytes written per second."""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def copy_rate():
    """bytes read + written per second of a device-to-device copy (median of 10 after 3)."""
    import torch
    n = 1 << 30
    a, b = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    ts = []
    for r in range(13):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        if r >= 3:
            ts.append(time.perf_counter() - t0)
    del a, b
    torch.cuda.empty_cache()
    return 2 * 4 * n / float(np.median(ts))


def held_entries(M, N, frac, rng):
    """1-based (rows, cols), sorted by (column, row): per column the rows step t + jitter, step = round(1 / frac)."""
    step = max(1, int(round(1.0 / frac)))
    per = M // step
    rows = (np.arange(per, dtype=np.int64) * step)[None, :] + rng.integers(0, step, (N, per), dtype=np.int64)
    cols = np.repeat(np.arange(1, N + 1, dtype=np.int64), per)
    return (rows + 1).ravel(), cols


def main():
    import pmf_import
    pkg = pmf_import.load()
    rest = sys.argv[1:]
    opt = lambda name, default: rest[rest.index(name) + 1] if name in rest else default    # noqa: E731
    rounds, epochs, frac = int(opt("--rounds", 10)), int(opt("--epochs", 10)), float(opt("--frac", 0.01))
    out = Path(opt("--out", str(ROOT / "profiles" / "holdout_kbench.json")))
    M, N, K = (int(x) for x in opt("--shape", "200000x50000x64").split("x"))
    rate = copy_rate()
    print(f"copy rate {rate / 1e12:.3f} TB/s (read + write)", flush=True)
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0, lib_path=(Path(os.environ["PMF_LIB"]).resolve() if os.environ.get("PMF_LIB") else None))
    ctx.set_data_device(None, M, N, store="f32")
    X0, Y0 = (rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    ctx.set_factors(X0, Y0)
    ctx.set_col_params((rng.standard_normal(N) * 0.1).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    nb, h = 8, N // 2
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=np.sort(rng.integers(0, nb, M)).astype(np.int32),
                              logdelta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                              theta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32))
                         for s, e in ((1, h), (h + 1, N))])
    ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    ctx.synth_data(seed=7, noise=0.1, frac_nan=0.0)
    ctx.set_optimizer("adam", lr=0.01)
    # the fits start away from the factors the data were drawn from (at those the first steps could only raise the loss)
    X1, Y1 = (rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    rows1, cols1 = held_entries(M, N, frac, rng)
    t0 = time.perf_counter()
    n = ctx.set_holdout(rows1, cols1)
    t_set = time.perf_counter() - t0
    del rows1, cols1
    print(f"{M}x{N} K={K}: {n} entries held in {t_set:.1f} s", flush=True)
    Kp = -(-K // 32) * 32
    floor_ms = n * (4 * Kp + 8) / rate * 1e3

    def fit(track):
        ctx.set_factors(X1, Y1)
        ctx.reset_optimizer_state()
        ctx.set_holdout_tracking(every=1 if track else 0, patience=0, restore_best=track)
        t0 = time.perf_counter()
        h = ctx.fit(update_X=True, update_Y=True, max_epochs=epochs, abs_tol=0, rel_tol=0)
        dt = (time.perf_counter() - t0) * 1e3
        assert (h["term_code"], h["epochs"]) == ("max_epochs", epochs), (h["term_code"], h["epochs"])
        assert len(h.get("holdout_loss", [])) == (epochs if track else 0)
        return dt

    def holdout():
        t0 = time.perf_counter()
        ctx.holdout_loss()
        return (time.perf_counter() - t0) * 1e3

    calls = {"holdout": holdout, "fit": lambda: fit(False), "fit+track": lambda: fit(True)}
    ts = {k: [] for k in calls}
    for r in range(rounds + 3):
        for k, f in calls.items():
            dt = f()
            if r >= 3:
                ts[k].append(dt)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    per_epoch = {k: med[k] / epochs for k in ("fit", "fit+track")}
    rec = dict(M=M, N=N, K=K, Kp=Kp, n_held=int(n), frac=frac, rounds=rounds, epochs=epochs, set_holdout_s=t_set,
               copy_rate_tbs=rate / 1e12, floor_ms=floor_ms, holdout_ms=med["holdout"], floor_fraction=floor_ms / med["holdout"],
               epoch_ms=per_epoch["fit"], epoch_tracked_ms=per_epoch["fit+track"],
               tracking_cost_ms=per_epoch["fit+track"] - per_epoch["fit"], geometry=ctx.debug_holdout_pass(),
               min_ms={k: min(v) for k, v in ts.items()}, max_ms={k: max(v) for k, v in ts.items()})
    print(f"hold-out pass {med['holdout']:.3f} ms (floor {floor_ms:.3f} ms: {100 * rec['floor_fraction']:.1f} % of it); epoch "
          f"{per_epoch['fit']:.3f} ms, tracked with restore_best {per_epoch['fit+track']:.3f} ms; {rec['geometry']}", flush=True)
    ctx.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    prev = json.loads(out.read_text()) if out.exists() else {}
    prev["holdout"] = rec
    out.write_text(json.dumps(prev, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
