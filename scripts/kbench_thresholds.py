"""Timing of the threshold pass (pmf_threshold_grad: pmf_thresh_kernel + its two reduce kernels) beside the fused data pass
of the same context.

    python scripts/kbench_thresholds.py                       the two shapes of DESIGN.md section 6
    python scripts/kbench_thresholds.py M N K N3 [--rounds R] one shape: N3 kind-3 columns (ordinal_sq_hinge3) first, normal after

Both are timed the same way, on the host clock around a call that ends in a device synchronise (pmf_threshold_grad returns the
group sums; pmf_epoch_begin + pmf_epoch_loss returns the loss), after three warm-up calls each, alternating; the fused kernel's
own event time (pmf_kernel_time) is printed beside them.  The data are classes 1..3 on the kind-3 columns."""
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
SHAPES = [(20000, 10000, 32, 2000), (100000, 50000, 64, 10000)]


def mean_se(x):
    x = np.asarray(x, np.float64)
    return float(x.mean()), float(x.std(ddof=1) / np.sqrt(x.size)) if x.size > 1 else 0.0


def run(pkg, M, N, K, N3, rounds):
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0, lib_path=(Path(os.environ["PMF_LIB"]).resolve() if os.environ.get("PMF_LIB") else None))
    ctx.set_data_device(None, M, N)
    ctx.set_factors((rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32))
    ctx.set_col_params(np.zeros(N, np.float32), np.concatenate([np.full(N3, 2.0, np.float32), np.zeros(N - N3, np.float32)]))
    ctx.set_batch_views([])
    ctx.set_noise([(1, N3), (N3 + 1, N)], ["ordinal_sq_hinge3", "normal"], np.ones(N, np.float32))
    ctx.synth_data(seed=7, noise=0.7, frac_nan=0.02)     # z + noise around mu = 2 on the kind-3 columns: classes 1..3 after the clamp
    opts = ctx.make_opts(update_X=True, update_Y=True)
    t_thr, t_fused = [], []
    for r in range(rounds + 3):
        t0 = time.perf_counter()
        ctx.threshold_grad(per_column=False)
        t1 = time.perf_counter()
        ctx.epoch_begin(opts)
        ctx.epoch_loss()
        t2 = time.perf_counter()
        if r == 2:
            ctx.kernel_time(reset=True)
        if r >= 3:
            t_thr.append((t1 - t0) * 1e3)
            t_fused.append((t2 - t1) * 1e3)
    (a, sa), (b, sb) = mean_se(t_thr), mean_se(t_fused)
    kms, kn = ctx.kernel_time()
    d = ctx.debug_threshold_pass()
    print(f"{M}x{N} K={K} kind-3 columns {N3}: threshold pass {a:.3f} +- {sa:.3f} ms, fused pass (both gradients) {b:.3f} +- {sb:.3f} ms "
          f"(its kernel alone {kms:.3f} ms x{kn}); ratio {a / b:.3f}; tiles {d['n_tiles']} units {d['n_units']} grid {d['grid']}")
    ctx.close()


def main():
    import pmf_import
    pkg = pmf_import.load()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 20
    if "--rounds" in sys.argv:
        args.remove(str(rounds))
    shapes = [tuple(int(x) for x in args[:4])] if len(args) >= 4 else SHAPES
    for s in shapes:
        run(pkg, *s, rounds)


if __name__ == "__main__":
    main()
