"""Cost of the NetworkRegularizer term on Y (csrc/pmf_netreg.hip; development aid): synthetic pathway graphs from a
seeded generator -- N features, K factors, about `nodes` nodes and `edges` edges per pathway of which a third of the nodes
are virtual -- with the regularizer alone (every data entry missing, M = 64) and beside the data pass (M rows of synthetic
data).  Prints ms/epoch with and without the term and the CG iterations of the first and of a warm epoch; the per-kernel
times come from `rocprofv3 --kernel-trace --stats -- python scripts/kbench_netreg.py ...` in a run of its own.
usage: kbench_netreg.py [N [K [M [nodes [edges]]]]]      (defaults 50000 64 200000 2000 20000; M = 0 skips the data pass)"""
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pmf_import  # noqa: E402

pkg = pmf_import.load()
args = [int(x) for x in sys.argv[1:]]
N, K, M, NODES, EDGES = (args + [50000, 64, 200000, 2000, 20000][len(args):])[:5]
EPS = 0.1


def pathway_blocks(rng):
    """AA, AB, BB of one pathway: NODES nodes, a third virtual, EDGES signed edges (built as the package's constructor
    does, vectorised: -w off the diagonal, EPS + sum |w| on it)."""
    v = NODES // 3
    obs = rng.choice(N, NODES - v, replace=False)
    idx = np.concatenate([obs, N + np.arange(v)])                 # global index of every node of the pathway
    a, b = rng.integers(0, NODES, EDGES), rng.integers(0, NODES, EDGES)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    _, first = np.unique(lo * NODES + hi, return_index=True)      # one edge per pair
    i, j = idx[lo[first]], idx[hi[first]]
    w = rng.uniform(0.5, 1.5, i.size) * rng.choice([-1.0, 1.0], i.size)
    T = N + v
    A = sp.coo_matrix((np.concatenate([-w, -w]), (np.concatenate([i, j]), np.concatenate([j, i]))), shape=(T, T)).tocsr()
    diag = EPS + np.asarray(abs(A).sum(axis=1)).ravel()
    A = (A + sp.diags(diag)).tocsr()
    return A[:N, :N], A[:N, N:], A[N:, N:]


def run(ctx, label, with_term, blocks, flags):
    ctx.clear_yreg()
    ctx.add_reg_l2("Y", np.full(K, 0.1, np.float32), 1.0)
    if with_term:
        ctx.add_reg_network("Y", *blocks, p=1.0)
    ctx.set_optimizer("adagrad", lr=0.001)
    r = ctx.fit(max_epochs=1, abs_tol=0, rel_tol=0, **flags)
    first = [ctx.get_reg_network_state("Y", k)[1] for k in range(K)] if with_term else [0]
    ctx.fit(max_epochs=3, epoch=2, abs_tol=0, rel_tol=0, **flags)
    ctx.synchronize()
    t0 = time.time()
    r = ctx.fit(max_epochs=13, epoch=4, abs_tol=0, rel_tol=0, **flags)
    ctx.synchronize()
    ms = (time.time() - t0) / len(r["loss"]) * 1e3               # (a fit that stops on a loss increase ran fewer epochs)
    warm = [ctx.get_reg_network_state("Y", k)[1] for k in range(K)] if with_term else [0]
    print(f"{label}: {ms:.3f} ms/epoch over {len(r['loss'])} epochs ({r['term_code']}); CG iterations first epoch mean {np.mean(first):.1f} max {max(first)}, warm mean "
          f"{np.mean(warm):.1f} max {max(warm)}; loss {r['loss'][0]:.6g} -> {r['loss'][-1]:.6g}", flush=True)
    return ms


rng = np.random.default_rng(11)
t0 = time.time()
parts = [pathway_blocks(rng) for _ in range(K)]
blocks = tuple([p[q] for p in parts] for q in range(3))
print(f"N={N} K={K}: {K} pathways of {NODES} nodes ({NODES // 3} virtual), nnz AA {sum(b.nnz for b in blocks[0])}, AB "
      f"{sum(b.nnz for b in blocks[1])}, BB {sum(b.nnz for b in blocks[2])}; built in {time.time() - t0:.1f} s", flush=True)
ctx = pkg.Context(0)
Y0 = (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
for rows, flags, name in ((64, dict(update_Y=True), "regularizer alone"), (M, dict(update_X=True, update_Y=True), "with the data pass")):
    if rows <= 0:
        continue
    ctx.set_data_device(None, rows, N)
    ctx.set_factors((rng.standard_normal((K, rows)) * 0.3).astype(np.float32), Y0)
    ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
    ctx.set_batch_views([])
    ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    ctx.synth_data(seed=7, noise=0.1, frac_nan=1.0 if rows == 64 else 0.02)
    ctx.clear_xreg()
    ctx.add_reg_l2("X", np.ones(K, np.float32), 1.0)
    ctx.set_layer_regs()
    off = run(ctx, f"{rows}x{N} K={K} {name}, term off", False, blocks, flags)
    ctx.set_Y(Y0)
    on = run(ctx, f"{rows}x{N} K={K} {name}, term on ", True, blocks, flags)
    print(f"  -> the term costs {on - off:.3f} ms/epoch = {100 * (on - off) / off:.1f} % of the epoch without it", flush=True)
ctx.close()
