"""Timing of pmf_impute_device (pmf_impute_kernel) against pmf_forward's k_forward, and of the pmf_impute host path.

    python scripts/kbench_impute.py M N K [flags] [--rounds R] [--forward] [--host]
    python scripts/kbench_impute.py --parse DIR         condense a rocprofv3 --kernel-trace --stats run of the above

flags: any of batch, link, keep joined by '+', or 0 (default batch+link: the quantity k_forward produces).
Every round times one pmf_impute_device call on the host clock (the call is synchronous: launch + kernel + wait), after
three warm-up calls.  With --forward every round also runs pmf_forward once (k_forward into an M x N device buffer, then
its copy to the host): the two kernels ALTERNATE in one process, and a `rocprofv3 --kernel-trace --stats -- python
scripts/kbench_impute.py ... --forward` run of its own gives each dispatch's pure kernel time; --parse prints their
means, standard errors and the three-standard-error verdict of the project's A/B rule.  --host times pmf_impute into a
host matrix (the staged path) and prints GB/s."""
import csv
import os
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
HBM_TBS = 6.5   # what scripts/hbm_pattern.hip reaches


def mean_se(x):
    x = np.asarray(x, np.float64)
    return float(x.mean()), float(x.std(ddof=1) / np.sqrt(x.size)) if x.size > 1 else 0.0


def parse(d):
    rows = []
    for f in Path(d).rglob("*kernel_trace.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    t = {}
    for r in rows:
        name = r["Kernel_Name"]
        key = "impute" if "pmf_impute_kernel" in name else "forward" if "k_forward" in name else None
        if key:
            t.setdefault(key, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6))
    out = {}
    for k, v in t.items():
        ms = [x[1] for x in sorted(v)]
        ms = ms[3:] if k == "impute" else ms       # the warm-up calls
        out[k] = mean_se(ms)
        print(f"{k}: n={len(ms)} mean {out[k][0]:.4f} ms  se {out[k][1]:.4f} ms  min {min(ms):.4f}")
    if len(out) == 2:
        d_, se = out["forward"][0] - out["impute"][0], float(np.hypot(out["forward"][1], out["impute"][1]))
        print(f"k_forward - pmf_impute_kernel = {d_:.4f} ms = {d_ / se if se else float('inf'):.1f} standard errors; "
              f"ratio {out['forward'][0] / out['impute'][0]:.2f}x")


def main():
    if sys.argv[1] == "--parse":
        return parse(sys.argv[2])
    import pmf_import
    import torch
    pkg = pmf_import.load()
    M, N, K = (int(x) for x in sys.argv[1:4])
    rest = sys.argv[4:]
    fl = rest[0] if rest and not rest[0].startswith("--") else "batch+link"
    flags = 0 if fl == "0" else sum({"batch": 1, "link": 2, "keep": 4}[w] for w in fl.split("+"))
    rounds = int(rest[rest.index("--rounds") + 1]) if "--rounds" in rest else 10
    rng = np.random.default_rng(3)
    ctx = pkg.Context(0, lib_path=(Path(os.environ["PMF_LIB"]).resolve() if os.environ.get("PMF_LIB") else None))
    ctx.set_data_device(None, M, N)
    ctx.set_factors((rng.standard_normal((K, M)) * 0.3).astype(np.float32), (rng.standard_normal((K, N)) * 0.3).astype(np.float32))
    ctx.set_col_params((rng.standard_normal(N) * 0.1).astype(np.float32), rng.standard_normal(N).astype(np.float32))
    nb, h = int(os.environ.get("PMF_NB", "8")), N // 2
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=np.sort(rng.integers(0, nb, M)).astype(np.int32),
                              logdelta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                              theta=(0.1 * rng.standard_normal((nb, e - s + 1))).astype(np.float32))
                         for s, e in ((1, h), (h + 1, N))])
    nbern, npois = N // 5, N // 10       # columns sorted by distribution, as the model assembles them
    ctx.set_noise([(1, nbern), (nbern + 1, N - npois), (N - npois + 1, N)], ["bernoulli", "normal", "poisson"], np.ones(N, np.float32))
    if flags & 4:
        ctx.synth_data(seed=7, noise=0.1, frac_nan=0.05)
    gb = 4.0 * M * N * 1e-9
    if "--host" in rest:
        out = np.zeros((M, N), np.float32, order="F")
        ctx.impute(flags, out=out)
        ts = []
        for _ in range(max(rounds // 3, 2)):
            t0 = time.perf_counter()
            ctx.impute(flags, out=out)
            ts.append(time.perf_counter() - t0)
        print(f"{M}x{N} K={K} flags={fl} pmf_impute (host path): {min(ts):.3f} s best of {len(ts)} = {gb / min(ts):.2f} GB/s")
        return
    t = torch.empty((N, M), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        ctx.impute_device(t.data_ptr(), flags)
    Z = np.zeros((M, N), np.float32, order="F") if "--forward" in rest else None
    ts = []
    for _ in range(rounds):
        if Z is not None:
            ctx.lib.pmf_forward(ctx._h, Z.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_float)))
        t0 = time.perf_counter()
        ctx.impute_device(t.data_ptr(), flags)
        ts.append((time.perf_counter() - t0) * 1e3)
    m, se = mean_se(ts)
    floor = gb / (HBM_TBS * 1e3) * 1e3
    print(f"{M}x{N} K={K} flags={fl} pmf_impute_device: {m:.3f} ms (se {se:.3f}, min {min(ts):.3f}) per call = "
          f"{gb / (m * 1e-3) * 1e-3:.2f} TB/s written; write floor at {HBM_TBS} TB/s: {floor:.3f} ms ({m / floor:.2f}x)")
    if Z is not None and flags == 3:
        got = t.cpu().numpy().T
        print(f"max |impute - forward| = {float(np.max(np.abs(got - Z))):.3g}")


if __name__ == "__main__":
    main()
