"""Wall time of one iteration of the batch-effect EM (theta_delta_em) with stages="host" and stages="library".

    python scripts/kbench_em_stage.py [M N K]          (default 100000 20000 64)

Two views x 8 batches, 10 % missing, synthetic Gaussian data made on the device (pmf_synth_data): the model's host copy of
the data is a matrix of zeros that is never uploaded.  Every call is synchronous; the host clock is taken around it.  A call
with n iterations costs the marshalling, the statistics pass that counts the batches, and n iterations: the time of one
iteration is (call with 6 iterations - call with 1) / 5.  Medians of 10 rounds after one warm-up round, the two paths
alternating within a round."""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pmf_import  # noqa: E402

pkg = pmf_import.load()
M, N, K = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (100000, 20000, 64)
NB, ROUNDS = 8, 10
rng = np.random.default_rng(5)
half = N // 2
batches = {v: [f"{v}{(i * NB) // M}" for i in range(M)] for v in ("u", "v")}
model = pkg.make_model(np.zeros((M, N), np.float32), K=K, sample_conditions=["c"] * M,
                       feature_views=["u"] * half + ["v"] * (N - half), batch_dict=batches, rng=rng)
mf, ct = model.matfac, model.matfac.col_transform
mf.X[...] = 0.3 * rng.standard_normal(mf.X.shape)
mf.Y[...] = 0.3 * rng.standard_normal(mf.Y.shape)
theta0 = [0.5 * rng.standard_normal(v.shape) for v in ct.unwrapped(4).theta.values]
delta20 = [0.5 + rng.random(v.shape) for v in theta0]
sigma2 = 0.5 + rng.random(N)

ctx = pkg.Context(0)
ctx.set_data_device(None, M, N)
pkg.matfac.marshal(mf, ctx, with_xreg=False, with_yreg=False)
ctx.synth_data(seed=7, noise=0.5, frac_nan=0.1)
model._ctx, model._ctx_data_id = ctx, (id(model.data), model.data.shape)      # the device copy is the synthetic one


def call(stages, n_iter):
    for dst, src in zip(ct.unwrapped(4).theta.values, theta0):
        dst[...] = src
    d2 = [d.copy() for d in delta20]
    ctx.synchronize()
    t0 = time.perf_counter()
    theta, d2 = pkg.theta_delta_em(model, d2, sigma2, update_priors=True, batch_em_max_iter=n_iter, batch_em_rtol=0.0,
                                   verbosity=0, stages=stages)
    dt = time.perf_counter() - t0
    return dt, theta, d2


times = {(s, n): [] for s in ("host", "library") for n in (1, 6)}
for r in range(ROUNDS + 1):
    order = ("host", "library") if r % 2 == 0 else ("library", "host")
    outs = {}
    for s in order:
        for n in (1, 6):
            dt, theta, d2 = call(s, n)
            if r > 0:
                times[(s, n)].append(dt)
            outs[(s, n)] = (theta, d2)
    if r == 0:
        err = max(float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(outs[("library", 6)][0], outs[("host", 6)][0]))
        print(f"{M} x {N}, K = {K}, 2 views x {NB} batches: theta after 6 iterations, library against host, rel_err {err:.2e}")
med = {k: float(np.median(v)) * 1e3 for k, v in times.items()}
for s in ("host", "library"):
    print(f"stages={s:8s} call with 1 iteration {med[(s, 1)]:8.2f} ms, with 6 {med[(s, 6)]:8.2f} ms, "
          f"one iteration {(med[(s, 6)] - med[(s, 1)]) / 5:8.2f} ms")
model.release_device()
