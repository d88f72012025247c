"""Wall time of the factor post-processing stages with postprocess="host" and postprocess="library", and the rates of the
library's kernels against their memory floors.

    python scripts/kbench_postprocess.py [M N K [rounds]]          (default 200000 50000 64, 10 rounds)

Two feature views, synthetic Gaussian data made on the device (pmf_synth_data): the model's host copy of the data is an
8 x N matrix of zeros that is never uploaded.  Every call is synchronous; the host clock is taken around it, the marshalling of the model
and the copy back included -- what fit_ pays per stage.  Medians of `rounds` rounds after one warm-up round, the two paths
alternating within a round, every stage from the same factors.

Per phase of each library call (pmf_debug_postprocess_times: host clock, each phase closed by a stream synchronisation) the
achieved bytes/s against the floor of the phase -- Gram / diagonal passes 4 Kp n bytes read, rotation / scale / permutation
8 Kp n bytes read and written -- and the eigen-solver's time on its own."""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pmf_import  # noqa: E402

pkg = pmf_import.load()
M, N, K = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (200000, 50000, 64)
ROUNDS = int(sys.argv[4]) if len(sys.argv) >= 5 else 10
Kp = 32 * ((K + 31) // 32)
rng = np.random.default_rng(5)
half = N // 2
# the model is built on 8 rows (the column side is what the stages read) and then given M rows of X: no M x N host matrix
model = pkg.make_model(np.zeros((8, N), np.float32), K=K, sample_conditions=["c"] * 8,
                       feature_views=["u"] * half + ["v"] * (N - half), rng=rng)
mf = model.matfac
mf.X = np.zeros((K, M), np.float32, order="F")
model.row_shard = (0, M, M)
X0 = (0.3 * rng.standard_normal(mf.X.shape)).astype(np.float32)
Y0 = (0.3 * rng.standard_normal(mf.Y.shape)).astype(np.float32)
ls0 = np.array(mf.col_transform.unwrapped(1).logsigma, np.float32)
mf.X[...] = X0
mf.Y[...] = Y0

ctx = pkg.Context(0)
ctx.set_data_device(None, M, N)
pkg.matfac.marshal(mf, ctx, with_xreg=False, with_yreg=False)
ctx.synth_data(seed=7, noise=0.5, frac_nan=0.1)
model._ctx, model._ctx_data_id = ctx, (id(model.data), model.data.shape)      # the device copy is the synthetic one

R = pkg.regularizers
STAGES = {
    "whiten": lambda pp: pkg.whiten_(model, postprocess=pp),
    "rotate_by_svd": lambda pp: pkg.rotate_by_svd_(model, postprocess=pp),
    "reorder_by_importance": lambda pp: pkg.reorder_by_importance_(model, postprocess=pp),
    "reweight_eb(L2 on X)": lambda pp: pkg.reweight_eb_(R.L2Regularizer(K, 1.0), mf.X, model=model if pp == "library" else None,
                                                        postprocess=pp),
    "reweight_eb(L2 on Y)": lambda pp: pkg.reweight_eb_(R.L2Regularizer(K, 1.0), mf.Y, model=model if pp == "library" else None,
                                                        postprocess=pp),
}
# bytes of the Gram phase and of the rewriting phase of each library call
FLOOR = {"whiten": (4 * Kp * (M + N), 8 * Kp * (M + 2 * N)), "rotate_by_svd": (4 * Kp * N, 8 * Kp * (M + N)),
         "reorder_by_importance": (4 * Kp * N, 8 * Kp * (M + N)), "reweight_eb(L2 on X)": (4 * Kp * M, 0),
         "reweight_eb(L2 on Y)": (4 * Kp * N, 0)}


def call(name, pp):
    mf.X[...] = X0
    mf.Y[...] = Y0
    mf.col_transform.unwrapped(1).logsigma[...] = ls0
    ctx.synchronize()
    t0 = time.perf_counter()
    STAGES[name](pp)
    dt = time.perf_counter() - t0
    return dt, (ctx.postprocess_times() if pp == "library" else None)


wall = {(s, pp): [] for s in STAGES for pp in ("host", "library")}
phase = {s: [] for s in STAGES}
for r in range(ROUNDS + 1):
    order = ("host", "library") if r % 2 == 0 else ("library", "host")
    for s in STAGES:
        for pp in order:
            dt, ph = call(s, pp)
            if r > 0:
                wall[(s, pp)].append(dt)
                if ph is not None:
                    phase[s].append((ph["gram"], ph["eig"], ph["apply"]))
print(f"{M} x {N}, K = {K} (Kp = {Kp}), medians of {ROUNDS} rounds")
for s in STAGES:
    h, l = (float(np.median(wall[(s, pp)])) * 1e3 for pp in ("host", "library"))
    g, e, a = (float(x) for x in np.median(np.array(phase[s]), axis=0))
    gb, ab = FLOOR[s]
    line = (f"{s:24s} host {h:9.2f} ms  library {l:9.2f} ms  |  Gram phase {g * 1e3:8.3f} ms = {gb / g / 1e12:6.3f} TB/s of "
            f"{gb / 1e6:8.1f} MB   eigen-solver {e * 1e3:8.3f} ms")
    if ab:
        line += f"   rewrite phase {a * 1e3:8.3f} ms = {ab / a / 1e12:6.3f} TB/s of {ab / 1e6:8.1f} MB"
    print(line)
model.release_device()
