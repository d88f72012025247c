"""Timing of pmf_remove_batch_effect_device (pmf_debatch_kernel) against the copy floor and against pmf_impute_device.

    python scripts/kbench_debatch.py M N K [--store f32|bf16] [--rounds R] [--hbm TB/s]

Every round times, one after the other on the host clock (each call is synchronous: launch + kernel + wait), one call of
    resident      pmf_remove_batch_effect_device(flags 0, Z = NULL)        reads the resident D, writes M x N f32
    device Z      pmf_remove_batch_effect_device(flags 0, Z = a device matrix, column-major)
    fill          pmf_remove_batch_effect_device(PMF_DEBATCH_FILL_MISSING, Z = NULL): pmf_impute_kernel first, then the above
    impute keep   pmf_impute_device(PMF_IMPUTE_BATCH | PMF_IMPUTE_KEEP_OBSERVED): reads the same D, writes the same bytes and
                  adds an MFMA forward -- the kernel the new one must not be slower than
after three warm-up rounds; the four ALTERNATE in one process and the medians of the rounds are printed.  The copy floor is
the bytes read plus written at --hbm (default: what scripts/hbm_pattern.hip reached when DESIGN section 4.1 was written; pass
the rate it reaches on the same machine in the same session).  Setup as scripts/kbench_impute.py: two batch views of
PMF_NB (default 8) sorted batches, columns sorted by distribution, 5 % missing."""
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
HBM_TBS = 6.5


def main():
    import pmf_import
    import torch
    pkg = pmf_import.load()
    M, N, K = (int(x) for x in sys.argv[1:4])
    rest = sys.argv[4:]
    opt = lambda name, default: rest[rest.index(name) + 1] if name in rest else default    # noqa: E731
    store, rounds, hbm = opt("--store", "f32"), int(opt("--rounds", 10)), float(opt("--hbm", HBM_TBS))
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0, lib_path=(Path(os.environ["PMF_LIB"]).resolve() if os.environ.get("PMF_LIB") else None))
    ctx.set_data_device(None, M, N, store=store)
    ctx.set_factors((rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32))
    ctx.set_col_params((rng.standard_normal(N) * 0.1).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    nb, h = int(os.environ.get("PMF_NB", "8")), N // 2
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=np.sort(rng.integers(0, nb, M)).astype(np.int32),
                              logdelta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                              theta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32))
                         for s, e in ((1, h), (h + 1, N))])
    nbern, npois = N // 5, N // 10       # columns sorted by distribution, as the model assembles them
    ctx.set_noise([(1, nbern), (nbern + 1, N - npois), (N - npois + 1, N)], ["bernoulli", "normal", "poisson"], np.ones(N, np.float32))
    ctx.synth_data(seed=7, noise=0.1, frac_nan=0.05)
    out = torch.empty((N, M), dtype=torch.float32, device="cuda")
    z = torch.empty((N, M), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.impute_device(z.data_ptr(), 1 | 4)           # a device Z with the data's values: the observed entries, predictions elsewhere
    calls = {
        "resident": lambda: ctx.remove_batch_effect_device(out.data_ptr(), 0),
        "device Z": lambda: ctx.remove_batch_effect_device(out.data_ptr(), 0, z_ptr=z.data_ptr()),
        "fill": lambda: ctx.remove_batch_effect_device(out.data_ptr(), 2),
        "impute keep": lambda: ctx.impute_device(out.data_ptr(), 1 | 4),
    }
    ts = {k: [] for k in calls}
    for r in range(rounds + 3):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            if r >= 3:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    esz = 2.0 if store == "bf16" else 4.0
    gb = {"resident": (esz + 4.0) * M * N * 1e-9, "device Z": 8.0 * M * N * 1e-9}
    print(f"{M}x{N} K={K} store={store} nb={nb}: medians of {rounds} alternated rounds; copy floor at {hbm} TB/s")
    med = {k: float(np.median(v)) for k, v in ts.items()}
    for k, v in ts.items():
        line = f"  {k:12s} {med[k]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
        if k in gb:
            floor = gb[k] / hbm
            line += f"  {gb[k] / med[k]:.2f} TB/s moved; floor {floor:.3f} ms, ratio {med[k] / floor:.2f}x"
        print(line)
    print(f"  resident / impute keep = {med['resident'] / med['impute keep']:.3f}")


if __name__ == "__main__":
    main()
