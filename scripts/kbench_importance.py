"""Timing of pmf_factor_importance against the only route to the same numbers without it: K + 1 calls of pmf_loss.

    python scripts/kbench_importance.py [--rounds R] [--shapes MxNxK,...] [--out profiles/importance_kbench.json]

For every shape (default 20000x10000x32 and 100000x50000x64) and both mixes -- "normal": every column normal; "general": a
fifth Bernoulli, a tenth Poisson, the rest normal, sorted by distribution as the model assembles them -- one context holds
synthetic data (5 % missing, two batch views of 8 sorted batches) and, in ONE run, alternates
    loss          pmf_loss                    one exact-f32 data pass: the yardstick is (K + 1) x its time
    importance    pmf_factor_importance       all four outputs copied back to the host
    sums only     pmf_factor_importance       delta = NULL: the same device work without the K x N copy back
on the host clock (each call is synchronous) after two warm-up rounds; medians are printed and written as JSON.  Per shape and
mix: ratio = (K + 1) loss / importance (above 1: faster than the yardstick), and the share of the device's VALU rate the pass
implies at OPS_PER_EVAL float32 operations per (entry, factor) -- the count of the normal model's evaluation in the kernel
source (two fused multiply-adds, a subtraction, three multiplications, the difference and its addition) -- against
CUS x 64 lanes x CLOCK_GHZ."""
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OPS_PER_EVAL, CUS, CLOCK_GHZ = 8, 256, 2.4
SHAPES = "20000x10000x32,100000x50000x64"


def setup(pkg, M, N, K, mix):
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0, lib_path=(Path(os.environ["PMF_LIB"]).resolve() if os.environ.get("PMF_LIB") else None))
    ctx.set_data_device(None, M, N, store="f32")
    ctx.set_factors((rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32))
    ctx.set_col_params((rng.standard_normal(N) * 0.1).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    nb, h = 8, N // 2
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=np.sort(rng.integers(0, nb, M)).astype(np.int32),
                              logdelta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                              theta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32))
                         for s, e in ((1, h), (h + 1, N))])
    if mix == "normal":
        ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    else:
        nbern, npois = N // 5, N // 10
        ctx.set_noise([(1, nbern), (nbern + 1, N - npois), (N - npois + 1, N)], ["bernoulli", "normal", "poisson"], np.ones(N, np.float32))
    ctx.synth_data(seed=7, noise=0.1, frac_nan=0.05)
    return ctx


def main():
    import pmf_import
    pkg = pmf_import.load()
    rest = sys.argv[1:]
    opt = lambda name, default: rest[rest.index(name) + 1] if name in rest else default    # noqa: E731
    rounds, out = int(opt("--rounds", 5)), Path(opt("--out", str(ROOT / "profiles" / "importance_kbench.json")))
    shapes = [tuple(int(x) for x in s.split("x")) for s in opt("--shapes", SHAPES).split(",")]
    records = []
    for M, N, K in shapes:
        for mix in ("normal", "general"):
            ctx = setup(pkg, M, N, K, mix)
            delta, full, null = np.zeros((N, K)), np.zeros(N), np.zeros(N)
            n_obs = np.zeros(N, np.int64)
            P = lambda a, t: a.ctypes.data_as(t)                                               # noqa: E731
            pd, pi = pkg._abi.pd, pkg._abi.pi64
            calls = {
                "loss": ctx.loss,
                "importance": lambda: ctx._chk(ctx.lib.pmf_factor_importance(ctx._h, P(delta, pd), P(full, pd), P(null, pd), P(n_obs, pi))),
                "sums only": lambda: ctx._chk(ctx.lib.pmf_factor_importance(ctx._h, None, P(full, pd), P(null, pd), P(n_obs, pi))),
            }
            ts = {k: [] for k in calls}
            for r in range(rounds + 2):
                for k, f in calls.items():
                    t0 = time.perf_counter()
                    f()
                    if r >= 2:
                        ts[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            loss_data = ctx.loss()["data"]
            agree = abs(full.sum() - loss_data) / abs(loss_data)                              # the two passes sum the same terms
            yard = (K + 1) * med["loss"]
            evals = float(n_obs.sum()) * K
            share = evals * OPS_PER_EVAL / (med["sums only"] * 1e-3) / (CUS * 64 * CLOCK_GHZ * 1e9)
            rec = dict(M=M, N=N, K=K, mix=mix, rounds=rounds, loss_ms=med["loss"], importance_ms=med["importance"],
                       sums_only_ms=med["sums only"], yardstick_ms=yard, ratio=yard / med["importance"], valu_share=share,
                       full_vs_loss_rel=agree, geometry=ctx.debug_factor_importance(), min_ms={k: min(v) for k, v in ts.items()},
                       max_ms={k: max(v) for k, v in ts.items()})
            records.append(rec)
            print(f"{M}x{N} K={K} {mix:7s}: loss {med['loss']:.3f} ms, importance {med['importance']:.3f} ms (sums only "
                  f"{med['sums only']:.3f}); (K + 1) x loss = {yard:.1f} ms: ratio {rec['ratio']:.2f}; VALU share {share:.3f}; "
                  f"{rec['geometry']}", flush=True)
            ctx.close()
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(ops_per_eval=OPS_PER_EVAL, cus=CUS, clock_ghz=CLOCK_GHZ, records=records), indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
