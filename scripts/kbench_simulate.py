"""Timing of pmf_simulate_data_resident / pmf_simulate_data_device (pmf_impute_kernel with the sampling epilogue) against
pmf_impute_device, the store floor and the older pmf_synth_data.

    python scripts/kbench_simulate.py M N K [--store f32|bf16] [--rounds R] [--hbm TB/s] [--noise s] [--frac f] [--kinds mixed|normal]

Every round times, one after the other on the host clock (each call is synchronous: launch + kernel + wait), one call of
    resident      pmf_simulate_data_resident                    writes the tile-major D (f32 or bf16)
    device        pmf_simulate_data_device                      writes M x N f32 column-major
    no draws      pmf_simulate_data_device, noise = 0, frac_missing = 0: normal tiles skip the Philox block altogether
    impute        pmf_impute_device(PMF_IMPUTE_BATCH | PMF_IMPUTE_LINK): the same forward and the same stores, no epilogue
    synth         pmf_synth_data: the scalar forward with its splitmix draws, writes the tile-major D
after three warm-up rounds; the five ALTERNATE in one process and the medians of the rounds are printed.  The store floor is
the bytes written at --hbm (default: what scripts/hbm_pattern.hip reached when DESIGN section 4.1 was written; pass the rate
it reaches on the same machine in the same session).  Setup: one batch view of PMF_NB (default 8) sorted batches over all
columns; --kinds mixed (default): columns sorted by distribution, 20 % bernoulli, 70 % normal, 10 % bernoulli_sq_hinge;
--kinds normal: every column normal (every entry pays logf / cosf)."""
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
    noise, frac, kinds = float(opt("--noise", 0.1)), float(opt("--frac", 0.05)), opt("--kinds", "mixed")
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0, lib_path=(Path(os.environ["PMF_LIB"]).resolve() if os.environ.get("PMF_LIB") else None))
    ctx.set_data_device(None, M, N, store=store)
    ctx.set_factors((rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32))
    ctx.set_col_params((rng.standard_normal(N) * 0.1).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    nb = int(os.environ.get("PMF_NB", "8"))
    ctx.set_batch_views([dict(start1=1, stop1=N, batch_of_row=np.sort(rng.integers(0, nb, M)).astype(np.int32),
                              logdelta=(0.1 * rng.standard_normal((nb, N))).astype(np.float32),
                              theta=(0.1 * rng.standard_normal((nb, N))).astype(np.float32))])
    if kinds == "mixed":
        nbern, nh = N // 5, N // 10
        ctx.set_noise([(1, nbern), (nbern + 1, N - nh), (N - nh + 1, N)], ["bernoulli", "normal", "bernoulli_sq_hinge"], np.ones(N, np.float32))
    else:
        ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    out = torch.empty((N, M), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    calls = {
        "resident": lambda: ctx.simulate_data_resident(seed=7, noise=noise, frac_missing=frac),
        "device": lambda: ctx.simulate_data_device(out.data_ptr(), seed=7, noise=noise, frac_missing=frac),
        "no draws": lambda: ctx.simulate_data_device(out.data_ptr(), seed=7, noise=0.0, frac_missing=0.0),
        "impute": lambda: ctx.impute_device(out.data_ptr(), 1 | 2),
        "synth": lambda: ctx.synth_data(seed=7, noise=noise, frac_nan=frac),
    }
    ts = {k: [] for k in calls}
    for r in range(rounds + 3):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            if r >= 3:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    esz = 2.0 if store == "bf16" else 4.0
    gb = {"resident": esz * M * N * 1e-9, "device": 4.0 * M * N * 1e-9, "no draws": 4.0 * M * N * 1e-9,
          "impute": 4.0 * M * N * 1e-9, "synth": esz * M * N * 1e-9}
    print(f"{M}x{N} K={K} store={store} nb={nb} kinds={kinds} noise={noise} frac={frac}: medians of {rounds} alternated rounds; "
          f"store floor at {hbm} TB/s")
    med = {k: float(np.median(v)) for k, v in ts.items()}
    for k, v in ts.items():
        floor = gb[k] / hbm
        print(f"  {k:9s} {med[k]:8.3f} ms (min {min(v):.3f}, max {max(v):.3f})  {gb[k] / med[k]:.2f} TB/s written; "
              f"floor {floor:.3f} ms, ratio {med[k] / floor:.2f}x")
    print(f"  device / impute = {med['device'] / med['impute']:.3f}   resident / device = {med['resident'] / med['device']:.3f}"
          f"   resident / synth = {med['resident'] / med['synth']:.3f}")


if __name__ == "__main__":
    main()
