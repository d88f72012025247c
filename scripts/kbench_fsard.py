"""Cost of one iteration of update_A! on the device, dense entry (pmf_fsard_update_A, csrc/pmf_fsard.hip) against sparse
entry (pmf_fsard_update_A_csr, csrc/pmf_fsard_csr.hip); development aid.  Synthetic S: L feature sets of 15 .. 200 members
drawn without replacement from the view's N_v columns (seeded), weights 1 / sqrt(size); Y = 0.5 N(0, 1).  Every call runs
max_epochs = 200 with term_iter = 201, so all 201 evaluations run and the host looks at the `done` flag once.  A host clock
goes around the synchronous call (uploads of S, the host-side transpose of the sparse entry, allocations and downloads
included) and is divided by the evaluations; reported is the median of 10 rounds after one warm-up round, the entries
alternating within a round.  Also printed: the bytes of S each entry uploads per call.
The per-kernel times come from `rocprofv3 --kernel-trace --stats -- python scripts/kbench_fsard.py 1 <shape>` in a run of
its own.
usage: kbench_fsard.py [rounds [shape]]      (shape: index into SHAPES, default all)"""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import pmf_import  # noqa: E402

pkg = pmf_import.load()
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
MAX_EPOCHS, TERM_ITER = 200, 201
CAPACITY = pkg.featureset_ard.FSARD_DENSE_CAPACITY
SHAPES = [(239, 25, 5000), (256, 64, 5000), (830, 25, 20000), (3090, 25, 20000), (3090, 64, 20000), (3090, 128, 20000)]
if len(sys.argv) > 2:
    SHAPES = [SHAPES[int(sys.argv[2])]]


def synthetic_csr(L, Nv, rng):
    sizes = rng.integers(15, 201, size=L)
    rowptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(Nv, size=s, replace=False)) for s in sizes]).astype(np.int32)
    val = np.repeat(1.0 / np.sqrt(sizes), sizes).astype(np.float32)
    return rowptr, col, val


def dense_of(csr, L, Nv):
    rowptr, col, val = csr
    S = np.zeros((L, Nv), np.float32)
    S[np.repeat(np.arange(L), np.diff(rowptr)), col] = val
    return S


def one_call(entry, S, Nv, K, alpha, lam):
    ssq = np.full((S[0].size - 1 if isinstance(S, tuple) else S.shape[0], K), 1e-8, np.float32)
    t0 = time.perf_counter()
    A, _, best, epochs = entry(1, Nv, S, alpha, lam, 1.01, 0.8, 0.05, ssq, max_epochs=MAX_EPOCHS, term_iter=TERM_ITER, atol=1e-5)
    dt = time.perf_counter() - t0
    assert epochs == MAX_EPOCHS and np.isfinite(best) and np.all(np.isfinite(A)), (epochs, best)
    return dt / (epochs + 1) * 1e6, best


rows = []
ctx = pkg.Context(0)
for L, K, Nv in SHAPES:
    rng = np.random.default_rng(1000 + L + K)
    csr = synthetic_csr(L, Nv, rng)
    nnz = int(csr[0][-1])
    ctx.set_data(np.full((1, Nv), np.nan, np.float32))
    ctx.set_factors(np.zeros((K, 1), np.float32), (0.5 * rng.standard_normal((K, Nv))).astype(np.float32))
    ctx.clear_xreg()
    ctx.clear_yreg()
    alpha = np.full(Nv, 1.01, np.float32)
    lam = np.full(K, 0.01, np.float32)
    entries = {"sparse": (ctx.fsard_update_A_csr, csr)}
    if L * K <= CAPACITY:
        entries["dense"] = (ctx.fsard_update_A, dense_of(csr, L, Nv))
    times = {k: [] for k in entries}
    best = {}
    for r in range(ROUNDS + 1):                                   # round 0 warms up
        for k in (sorted(entries) if r % 2 else sorted(entries, reverse=True)):
            us, best[k] = one_call(*entries[k], Nv, K, alpha, lam)
            if r:
                times[k].append(us)
    # CSR and its transpose, 8 bytes per entry each, and the two pointer arrays; the dense entry uploads L x N_v floats
    up = {"sparse": 16 * nnz + 8 * (L + 1) + 8 * (Nv + 1), "dense": 4 * L * Nv}
    row = dict(L=L, K=K, Nv=Nv, nnz=nnz)
    for k in ("dense", "sparse"):
        if k in entries:
            row[k + "_us_per_iter"] = round(float(np.median(times[k])), 2)
            row[k + "_min_max"] = [round(min(times[k]), 2), round(max(times[k]), 2)]
            row[k + "_S_bytes"] = up[k]
            row[k + "_best_loss"] = best[k]
    rows.append(row)
    print(json.dumps(row), flush=True)
ctx.close()

print("\n| L | K | N_v | nnz(S) | dense us/iter | sparse us/iter | dense S upload | sparse S upload |")
print("|---|---|---|---|---|---|---|---|")
for r in rows:
    d = f"{r['dense_us_per_iter']:.1f}" if "dense_us_per_iter" in r else "refused"
    db = f"{r['dense_S_bytes'] / 1e6:.1f} MB" if "dense_S_bytes" in r else f"({4 * r['L'] * r['Nv'] / 1e6:.1f} MB)"
    print(f"| {r['L']} | {r['K']} | {r['Nv']} | {r['nnz']} | {d} | {r['sparse_us_per_iter']:.1f} | {db} | {r['sparse_S_bytes'] / 1e6:.2f} MB |")
