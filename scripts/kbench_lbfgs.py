"""Timing of the pieces of pmf_fit_lbfgs (csrc/pmf_lbfgs.hip) on synthetic data (pmf_synth_data).

    python scripts/kbench_lbfgs.py M N K [--iters I] [--m m] [--rounds R]
    python scripts/kbench_lbfgs.py --parse DIR M N K [--m m]    condense a rocprofv3 --kernel-trace run of the above

Host clock over synchronous calls, after warm-up, the two alternated: the gradient pass (pmf_epoch_begin + a
synchronize) and pmf_loss.  Then one pmf_fit_lbfgs of I iterations from the random start; from its counters
    own share = 1 - (grad_evals * t_grad + loss_evals * t_loss) / seconds
is what L-BFGS's own kernels (total gradient, recursion, trial points) and its readbacks take of the call, and
trials / iteration and t_loss / t_grad are printed beside it.  The per-kernel figures (one direction at a full queue =
2 m + 1 launches of k_lb_sweep, one trial-point sweep k_lb_trial, k_lb_grad) come from a kernel trace of the same run:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/kbench_lbfgs.py M N K
    python scripts/kbench_lbfgs.py --parse DIR M N K
--parse prints each kernel's mean time and the byte floor of its traffic at the measured copy rate (6.29 TB/s):
a sweep reads p and two vectors and writes p (4 vectors), a trial reads two and writes one or two, k_lb_grad reads the
parameter, the data gradient, the regularizer weights, g_old and s and writes g and y."""
import csv
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
COPY_TBS = 6.29


def arg(rest, name, default):
    return int(rest[rest.index(name) + 1]) if name in rest else default


def vec_bytes(M, N, K):
    return 4.0 * (32 * ((K + 31) // 32)) * (M + N)


def parse(d, M, N, K, m):
    rows = []
    for f in Path(d).rglob("*kernel_trace.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    t = {}
    for r in rows:
        name = r["Kernel_Name"]
        for key in ("k_lb_sweep", "k_lb_trial", "k_lb_grad", "k_lb_finish", "k_lb_sum2", "k_reg_step", "k_loss_reduce", "pmf_fused"):
            if key in name:
                t.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    vb = vec_bytes(M, N, K)
    floor = {"k_lb_sweep": 4 * vb, "k_lb_trial": 3 * vb, "k_lb_grad": 8 * vb}
    for k, v in sorted(t.items()):
        v = np.asarray(v)
        msg = f"{k}: n={v.size} mean {v.mean():.4f} ms  median {np.median(v):.4f}  min {v.min():.4f}  total {v.sum():.2f} ms"
        if k in floor:
            fl = floor[k] / (COPY_TBS * 1e12) * 1e3
            msg += f"  byte floor {fl:.4f} ms ({np.median(v) / fl:.2f}x)"
        print(msg)
    if "k_lb_sweep" in t:
        sw = float(np.median(t["k_lb_sweep"]))
        print(f"one direction at a full queue (m = {m}): {2 * m + 1} sweeps = {(2 * m + 1) * sw:.3f} ms; "
              f"byte floor {(2 * m + 1) * 4 * vb / (COPY_TBS * 1e12) * 1e3:.3f} ms")
    own = sum(float(np.sum(v)) for k, v in t.items() if k.startswith("k_lb_"))
    allk = sum(float(np.sum(v)) for v in t.values())
    print(f"L-BFGS's own kernels: {own:.2f} ms of {allk:.2f} ms traced kernel time = {100 * own / allk:.1f} %")


def main():
    if sys.argv[1] == "--parse":
        M, N, K = (int(x) for x in sys.argv[3:6])
        return parse(sys.argv[2], M, N, K, arg(sys.argv, "--m", 10))
    import pmf_import
    pkg = pmf_import.load()
    M, N, K = (int(x) for x in sys.argv[1:4])
    rest = sys.argv[4:]
    iters, m, rounds = arg(rest, "--iters", 30), arg(rest, "--m", 10), arg(rest, "--rounds", 10)
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0)
    ctx.set_data_device(None, M, N)
    X0 = (rng.standard_normal((K, M)) * 0.3).astype(np.float32)
    Y0 = (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    ctx.set_factors(X0, Y0)
    ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
    ctx.set_batch_views([])
    ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    ctx.synth_data(seed=7, noise=0.1, frac_nan=0.0)
    ctx.set_factors(X0 * 0.5, Y0 * 0.5)                      # start away from the generating factors
    ctx.clear_xreg()
    ctx.clear_yreg()
    ctx.add_reg_l2("X", np.full(K, 0.1, np.float32))       # init_factors!'s 0.05 * sum(x .* x)
    ctx.add_reg_l2("Y", np.full(K, 0.1, np.float32))
    ctx.set_layer_regs()
    ctx.set_optimizer("adagrad", lr=0.05)
    o = ctx.make_opts(update_X=True, update_Y=True)
    for _ in range(3):
        ctx.epoch_begin(o)
        ctx.synchronize()
        ctx.loss()
    tg, tl = [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        ctx.epoch_begin(o)
        ctx.synchronize()
        tg.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctx.loss()
        tl.append((time.perf_counter() - t0) * 1e3)
    tg, tl = float(np.median(tg)), float(np.median(tl))
    print(f"{M}x{N} K={K}: gradient pass {tg:.3f} ms, pmf_loss {tl:.3f} ms, ratio loss / gradient {tl / tg:.3f} "
          f"(medians of {rounds}, host clock, synchronous)")
    r = ctx.fit_lbfgs(m=m, max_iter=iters, rel_tol=0, abs_tol=0)
    sec, it = r["seconds"] * 1e3, max(r["iters"], 1)
    data = r["grad_evals"] * tg + r["loss_evals"] * tl
    print(f"pmf_fit_lbfgs m={m}: {r['iters']} iterations in {sec:.1f} ms = {sec / it:.3f} ms / iteration; "
          f"{r['loss_evals']} loss + {r['grad_evals']} gradient passes, {(r['loss_evals'] - 1) / it:.2f} trials / iteration, "
          f"{r['resets']} resets; loss {r['loss'][0]:.6g} -> {r['final_loss']:.6g} ({r['term_code']})")
    print(f"data passes {data:.1f} ms; L-BFGS's own kernels and readbacks {sec - data:.1f} ms = {100 * (sec - data) / sec:.1f} % "
          f"of the call = {(sec - data) / it:.3f} ms / iteration; trials x loss / gradient = {(r['loss_evals'] - 1) / it * tl / tg:.2f}")
    vb = vec_bytes(M, N, K)
    print(f"byte floors at {COPY_TBS} TB/s: one direction at a full queue ({2 * m + 1} sweeps x 4 vectors of {vb / 1e6:.1f} MB) "
          f"{(2 * m + 1) * 4 * vb / (COPY_TBS * 1e12) * 1e3:.3f} ms; one trial-point sweep (3 vectors) {3 * vb / (COPY_TBS * 1e12) * 1e3:.3f} ms")
    ctx.close()


if __name__ == "__main__":
    main()
