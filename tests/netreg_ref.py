"""fp64 restatement of the pathway-graph regularizers for the tests: dense numpy, exact solve by numpy.linalg.solve.
Written from the mathematics of src/regularizers.jl:249-306 / src/util.jl:269-314, independently of the package's
regularizers.py.  Also: the f32 restatement of the device's CG rule and the seeded graph families."""
import numpy as np

EPS = 0.1
RTOL = 1e-6


def dense_blocks(feature_ids, edgelist, epsilon=EPS, weight=1.0):
    """(AA, AB, BB) of one edge list: symmetric, -w off the diagonal, epsilon + sum |w| on it, the last of repeated
    edges counts; nodes outside `feature_ids` are virtual, sorted, appended."""
    obs = {f: i for i, f in enumerate(feature_ids)}
    virt = sorted({e[q] for e in edgelist for q in (0, 1)} - set(obs))
    idx = dict(obs)
    idx.update({f: len(obs) + i for i, f in enumerate(virt)})
    T = len(idx)
    last = {}
    for a, b, w in edgelist:
        i, j = idx[a], idx[b]
        last[(max(i, j), min(i, j))] = float(w)
    A = np.zeros((T, T))
    A[np.arange(T), np.arange(T)] = epsilon
    for (i, j), w in last.items():
        A[i, j] += -w
        A[j, i] += -w
        A[i, i] += abs(w)
        A[j, j] += abs(w)
    A *= weight
    n = len(obs)
    return A[:n, :n].copy(), A[:n, n:].copy(), A[n:, n:].copy()


def exact_one(AA, AB, BB, p):
    """(loss, gradient, u) of one factor in f64 with the exact Schur complement."""
    p = np.asarray(p, np.float64)
    t = AB.T @ p
    u = -np.linalg.solve(BB, t) if BB.shape[0] else np.zeros(0)
    loss = 0.5 * p @ AA @ p + t @ u + 0.5 * u @ BB @ u
    return loss, AA @ p + AB @ u, u


def exact(blocks, P):
    """blocks: per factor (AA, AB, BB); P: K x n.  -> loss, gradient K x n, list of u_k."""
    out = [exact_one(*b, P[k]) for k, b in enumerate(blocks)]
    return sum(o[0] for o in out), np.stack([o[1] for o in out]), [o[2] for o in out]


def _mv32(A32, x32):
    """f32 operands, the row sums accumulated in f64 and rounded once."""
    return (A32.astype(np.float64) @ x32.astype(np.float64)).astype(np.float32)


def cg_f32(BB, t, u0=None, rtol=RTOL):
    """The device's rule: solve BB u = -t in f32 vectors with f64 dot products, from u0, until |r| <= rtol |t| or
    2 v iterations; t = 0 gives u = 0.  -> (u f32, iterations)."""
    v = BB.shape[0]
    B64 = BB.astype(np.float32).astype(np.float64)          # the f32 matrix, widened once
    t = np.asarray(t, np.float32)
    u = np.zeros(v, np.float32) if u0 is None else np.asarray(u0, np.float32).copy()
    tt = float(t.astype(np.float64) @ t.astype(np.float64))
    if v == 0 or tt == 0.0:
        return np.zeros(v, np.float32), 0
    r = (-t.astype(np.float64) - B64 @ u.astype(np.float64)).astype(np.float32)
    d = r.copy()
    rr = float(r.astype(np.float64) @ r.astype(np.float64))
    it = 0
    while rr > rtol * rtol * tt and it < 2 * v:
        q = (B64 @ d.astype(np.float64)).astype(np.float32)      # row sums in f64, rounded once
        dq = float(d.astype(np.float64) @ q.astype(np.float64))
        alpha = np.float32(rr / dq)
        u = u + alpha * d
        r = r - alpha * q
        rr_new = float(r.astype(np.float64) @ r.astype(np.float64))
        d = r + np.float32(rr_new / rr) * d
        rr = rr_new
        it += 1
    return u, it


def restated_one(AA, AB, BB, p, u0=None):
    """(loss, gradient f32, u f32, iterations) of one factor as the device computes it."""
    p32 = np.asarray(p, np.float32)
    A32, C32, B32 = AA.astype(np.float32), AB.astype(np.float32), BB.astype(np.float32)
    t = _mv32(C32.T, p32) if BB.shape[0] else np.zeros(0, np.float32)
    u, it = cg_f32(BB, t, u0)
    Ap = A32.astype(np.float64) @ p32.astype(np.float64)
    g = (Ap + C32.astype(np.float64) @ u.astype(np.float64)).astype(np.float32)
    u64 = u.astype(np.float64)
    loss = 0.5 * p32.astype(np.float64) @ Ap + t.astype(np.float64) @ u64 + 0.5 * u64 @ (B32.astype(np.float64) @ u64)
    return loss, g, u, it


def restated(blocks, P, u0=None):
    out = [restated_one(*b, P[k], None if u0 is None else u0[k]) for k, b in enumerate(blocks)]
    return sum(o[0] for o in out), np.stack([o[1] for o in out]), [o[2] for o in out], [o[3] for o in out]


# ---- seeded graph families (observed nodes 0 .. n-1 are the feature ids, virtual nodes are ("v", i)) -------------------
def random_graph(rng, n, n_virtual, n_edges, signed=True, n_used=None):
    """n_edges random edges among `n_used` observed nodes (default all) and n_virtual virtual ones, weights in
    +-[0.5, 1.5]; every virtual node gets at least one edge to an observed node."""
    n_used = n if n_used is None else n_used
    nodes = list(range(n_used)) + [("v", i) for i in range(n_virtual)]
    el = []
    for i in range(n_virtual):
        el.append([("v", i), int(rng.integers(n_used)), float(rng.uniform(0.5, 1.5))])
    while len(el) < n_edges:
        a, b = rng.integers(len(nodes), size=2)
        if a == b:
            continue
        w = float(rng.uniform(0.5, 1.5)) * (float(rng.choice([-1.0, 1.0])) if signed else 1.0)
        el.append([nodes[a], nodes[b], w])
    return el


def hub_graph(n_obs_leaves, n_virtual_leaves=0):
    """a virtual hub ("v", 0) joined to observed nodes 0 .. n_obs_leaves-1 and to n_virtual_leaves virtual leaves"""
    hub = ("v", 0)
    return [[hub, i, 1.0] for i in range(n_obs_leaves)] + [[hub, ("v", 1 + i), 1.0] for i in range(n_virtual_leaves)]


def chain_graph(n_total, n_virtual):
    """a chain of n_total nodes whose first n_total - n_virtual are observed (0 ..), the rest virtual"""
    n_obs = n_total - n_virtual
    node = lambda i: i if i < n_obs else ("v", i - n_obs)   # noqa: E731
    return [[node(i), node(i + 1), 1.0] for i in range(n_total - 1)]


def to_csr(M):
    import scipy.sparse as sp
    return sp.csr_matrix(M)
