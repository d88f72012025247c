"""numpy restatement of fit_lbfgs! (src/fit_lbfgs.jl:114-243) as DESIGN.md section 2 ("Deviation 2 / L-BFGS") states it, for
the tests: written from that text, independently of csrc/pmf_lbfgs.hip.  The vectors are (X, Y) pairs of a `real` dtype; loss
and gradient come from a callable, for model problems the C oracle's (`oracle_fun`).  real = float64 is the reference run,
real = float32 its twin: f32 vectors and f32 products summed in f64, what the device does in another summation order.

Besides the library's trace (loss, trial count, flags per iteration) a run records the MARGIN of every decision it took:
    Armijo, per trial : |(l0 + c1 s dd) - l1| / |l0|
    reset             : |sy - sy_min| / max(|sy|, sy_min)
    descent           : |dd| / |g|
A run in other arithmetic can only decide differently where a margin is of the size of its rounding, so the tests compare
trajectories over the leading iterations whose margins all stay above GUARD (`horizon`)."""
import numpy as np

TERM = {0: "max_epochs", 2: "abs_tol", 3: "rel_tol", 4: "nonfinite"}

# twice the project's 2e-5 loss tolerance on each of the two losses a decision compares, times ten
GUARD = 4e-4
MIN_HORIZON = 8
MAX_ITER = 14        # iterations every table case runs for

# Tolerances of the device against the fp64 run: 10 x the f32 twin's own worst deviation from fp64 over the tables below
# (floor 2e-6, the section-2 precedent); x 10 because the device sums in another order than the twin.  Measured by
# tests/test_lbfgs_host.py (which asserts the twin stays within a tenth of each): direction, worst |p32 - p64|_inf / |p64|_inf
# = 2.7e-7 over DIRECTION_SHAPES x DIRECTION_PAIRS; loss traces, worst relative deviation over the case's horizon: 4.6e-5,
# 3.4e-6, 2.4e-6, 3.7e-7 in the order below (the runs are 14 iterations long: late iterates differ by the early roundings
# the search has amplified).
DIR_TOL = 3e-6
LOSS_TOL = {"normal_l2": 5e-4, "mixed_group_fsard_m3": 4e-5, "exhaust_bt2": 3e-5, "pad_rows_k33": 4e-6}

# model problems (tests/problems.make_problem keywords) with the L-BFGS options of the run
CASES = [
    dict(name="normal_l2", m=10, backtrack_max_iter=100,
         problem=dict(M=48, N=36, K=3, seed=1, xreg="l2", yreg="l2", random_init=True)),
    dict(name="mixed_group_fsard_m3", m=3, backtrack_max_iter=100,
         problem=dict(M=70, N=50, K=4, seed=2, bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2,
                      n_batches=3, nan_frac=0.1, weights=True, col_params=True, xreg="group", yreg="fsard",
                      random_init=True)),
    dict(name="exhaust_bt2", m=10, backtrack_max_iter=2,
         problem=dict(M=40, N=33, K=2, seed=3, xreg="l2", yreg="l2", random_init=True)),
    dict(name="pad_rows_k33", m=5, backtrack_max_iter=100,
         problem=dict(M=37, N=29, K=33, seed=4, nan_frac=0.1, xreg="l2", yreg="group", random_init=True)),
]

# (K, M, N) of the direction checks: one element; pad rows live; several workgroups (500 of the 1024 a grid holds: no
# grid-stride trip -- EDGE_DIRECTIONS below has those)
DIRECTION_SHAPES = [(1, 1, 1), (33, 7, 5), (64, 5000, 3000)]
DIRECTION_PAIRS = [0, 1, 10]

# (K, M, N, n_pairs) past one grid and at full history.  A vector has 32 ceil(K / 32) (M + N) floats; a grid of 1024
# workgroups x 256 threads x 4 floats covers 1,048,576 of them, longer vectors take grid-stride trips.
EDGE_DIRECTIONS = [
    (32, 20000, 13000, 0), (32, 20000, 13000, 2),   # 1,056,000 floats: a second trip for the first workgroups only
    (64, 20000, 13000, 1),                          # a third trip
    (32, 1, 33000, 3), (32, 33000, 1, 3),           # the X / Y seam one column from either end
    (1, 16400, 16400, 2),                           # K = 1: 31 pad rows per column
    (33, 7, 5, 32), (64, 5000, 3000, 32),           # full history (LB_MAX_M pairs: 65 sweeps)
    (32, 8193, 24600, 32),                          # ... beyond one grid
]
# 10 x the f32 twin's worst deviation over EDGE_DIRECTIONS, 4.62e-7 at the last row (tests/test_lbfgs_host.py)
DIR_TOL_EDGE = 5e-6

# trajectories (same record as CASES, MAX_ITER iterations) at the decisions CASES does not take: a vector beyond one grid
# with a reset, a reset at every iteration, the non-descent fallback, a wrapping m = 2 queue.  sy_min absent: the default.
EDGE_CASES = [
    dict(name="wide_k32", m=3, backtrack_max_iter=100,
         problem=dict(M=2, N=33000, K=32, seed=6, nan_frac=0.1, xreg="l2", yreg="group", random_init=True)),
    dict(name="reset_every", m=10, backtrack_max_iter=100, sy_min=1e30,
         problem=dict(M=40, N=33, K=2, seed=3, xreg="l2", yreg="l2", random_init=True)),
    dict(name="non_descent", m=10, backtrack_max_iter=2, sy_min=-1e30,
         problem=dict(M=40, N=33, K=2, seed=11, xreg="l2", yreg="l2", random_init=True)),
    dict(name="m2_wrap", m=2, backtrack_max_iter=100,
         problem=dict(M=48, N=36, K=3, seed=1, xreg="l2", yreg="l2", random_init=True)),
]
# 10 x the twin's worst relative loss deviation over the case's horizon (floor 2e-6), measured by tests/test_lbfgs_host.py:
# 3.49e-5, 1.94e-5, 1.99e-5, 4.18e-5 in the order above
LOSS_TOL_EDGE = {"wide_k32": 3.5e-4, "reset_every": 2e-4, "non_descent": 2e-4, "m2_wrap": 4.2e-4}


def case_by_name(name):
    return next(c for c in CASES + EDGE_CASES if c["name"] == name)


def inner(a, b):
    """inner_prod of two (X, Y) pairs: products in the vectors' dtype, sums in f64."""
    return float(np.sum(a[0] * b[0], dtype=np.float64) + np.sum(a[1] * b[1], dtype=np.float64))


def _axpy(p, coef, u, real):
    """p - coef * u with an f64 coefficient, rounded once per element (Float32 .- Float32 .* Float64 in the reference)."""
    return tuple((p[i].astype(np.float64) - coef * u[i].astype(np.float64)).astype(real) for i in (0, 1))


def two_loop(g, s_list, y_list, real=np.float64):
    """inner_loop! (:151-167) applied to p = -g.  s_list / y_list newest first."""
    p = tuple((-np.asarray(v, real)).copy() for v in g)
    s_list = [tuple(np.asarray(v, real) for v in s) for s in s_list]
    y_list = [tuple(np.asarray(v, real) for v in y) for y in y_list]
    n = len(s_list)
    rho = [1.0 / inner(y_list[k], s_list[k]) for k in range(n)]
    alpha = [0.0] * n
    for k in range(n):
        alpha[k] = rho[k] * inner(s_list[k], p)
        p = _axpy(p, alpha[k], y_list[k], real)
    if n:
        gamma = real(inner(s_list[0], y_list[0]) / inner(y_list[0], y_list[0]))
        p = tuple(v * gamma for v in p)
    for k in range(n - 1, -1, -1):
        beta = rho[k] * inner(y_list[k], p)
        p = _axpy(p, beta - alpha[k], s_list[k], real)
    return p


def fit_lbfgs(fun, X0, Y0, real=np.float64, m=10, max_iter=1000, backtrack_max_iter=100, rel_tol=1e-9, abs_tol=1e-6,
              backtrack_shrinkage=0.8, c1=1e-4, sy_min=1e-4):
    """fun(X, Y) -> (loss, (gX, gY)).  Returns the trace record and the final point; `log` holds per iteration what the
    quirk tests look at (queue length after the push / reset, p_norm and dd the backtrack used, the step vector left)."""
    x = (np.array(X0, real), np.array(Y0, real))
    shrink32 = real(backtrack_shrinkage)
    out = dict(loss=[], trials=[], flags=[], margin=[], log=[], loss_evals=0, grad_evals=0, resets=0)

    def loss_at(v):
        out["loss_evals"] += 1
        return float(fun(v[0], v[1])[0])

    cur_loss = loss_at(x)
    term, it = 0, 0
    final = cur_loss
    sq, yq = [], []
    old_grad, p = None, None
    while it < max_iter:
        g = fun(x[0], x[1])[1]
        g = (np.asarray(g[0], real), np.asarray(g[1], real))
        out["grad_evals"] += 1
        flags, margins = 0, []
        sy = 1.0
        if old_grad is not None:
            if len(yq) >= m:
                sq.pop()
                yq.pop()
            sq.insert(0, p)
            yq.insert(0, (g[0] - old_grad[0], g[1] - old_grad[1]))
            sy = inner(yq[0], sq[0])
            margins.append(abs(sy - sy_min) / max(abs(sy), sy_min))
        if sy > sy_min:
            p = two_loop(g, sq, yq, real)
        else:
            p = (-g[0], -g[1])
            sq, yq = [], []
            if old_grad is not None:    # a reset forgets a history: on the first iteration there is none (sy_min >= 1)
                flags |= 1
                out["resets"] += 1
        qlen = len(sq)
        # backtrack!
        p_norm = np.sqrt(inner(p, p))
        if p_norm == 0.0:
            term = 2
            break
        dd = inner(p, g) / p_norm
        margins.append(abs(dd) / np.sqrt(inner(g, g)))
        p_norm0, p_first = p_norm, p
        if dd >= 0:
            p = (-g[0], -g[1])
            flags |= 2
        orig = (x[0].copy(), x[1].copy())
        l1, trials, accepted = np.inf, 0, False
        for _ in range(backtrack_max_iter):
            x = (orig[0] + p[0], orig[1] + p[1])
            l1 = loss_at(x)
            trials += 1
            thr = cur_loss + c1 * p_norm * dd
            margins.append(abs(thr - l1) / abs(cur_loss) if np.isfinite(l1) else np.inf)
            if l1 <= thr:
                accepted = True
                break
            p = (p[0] * shrink32, p[1] * shrink32)
            p_norm *= backtrack_shrinkage
        if not accepted:
            flags |= 4
        new_loss = l1
        out["loss"].append(new_loss)
        out["trials"].append(trials)
        out["flags"].append(flags)
        out["margin"].append(min(margins))
        out["log"].append(dict(qlen=qlen, p_norm=p_norm, p_norm0=p_norm0, p_first=p_first, g=g, dd=dd, p=p, step=(x[0] - orig[0], x[1] - orig[1]), sy=sy))
        final = new_loss
        it += 1
        if not np.isfinite(new_loss):
            term = 4
            break
        diff = cur_loss - new_loss
        if abs(diff) < abs_tol:
            term = 2
            break
        if abs(diff / new_loss) < rel_tol:
            term = 3
            break
        cur_loss = new_loss
        old_grad = g
    out.update(term_code=TERM[term], iters=it, final_loss=final, X=x[0], Y=x[1])
    for k in ("loss", "margin"):
        out[k] = np.array(out[k], np.float64)
    for k in ("trials", "flags"):
        out[k] = np.array(out[k], np.int32)
    return out


def horizon(run, guard=GUARD):
    """Leading iterations of a run whose every decision margin stays above the guard."""
    below = np.nonzero(~(run["margin"] > guard))[0]
    return int(below[0]) if below.size else len(run["margin"])


def oracle_fun(p, precision):
    """(fun, model) over the C oracle of problem dict `p`: data loss + X_reg + Y_reg and its gradient (full_loss /
    full_gradient, :3-57, with the thread buffers summed)."""
    from problems import to_oracle
    mdl = to_oracle(p, precision=precision)

    def fun(X, Y):
        mdl.X[...] = X
        mdl.Y[...] = Y
        loss, g = mdl.loss_and_grads(update_X=True, update_Y=True)
        return loss, (g["X"].copy(), g["Y"].copy())
    return fun, mdl


_RUNS = {}


def case_run(name, precision):
    """The table case's run in fp64 (precision 64) or as the f32 twin (32), computed once per process."""
    from problems import make_problem
    key = (name, precision)
    if key not in _RUNS:
        c = case_by_name(name)
        p = make_problem(**c["problem"])
        fun, _ = oracle_fun(p, precision)
        real = np.float64 if precision == 64 else np.float32
        kw = dict(sy_min=c["sy_min"]) if "sy_min" in c else {}
        _RUNS[key] = (p, fit_lbfgs(fun, p["X"], p["Y"], real=real, m=c["m"], max_iter=MAX_ITER,
                                   backtrack_max_iter=c["backtrack_max_iter"], rel_tol=0.0, abs_tol=0.0, **kw))
    return _RUNS[key]


def random_history(K, M, N, n_pairs, seed):
    """g and n_pairs (s, y) pairs with <s, y> > 0 in f32: y = a positive diagonal times s plus a little noise."""
    rng = np.random.default_rng(seed)

    def vec(scale=1.0):
        return ((rng.standard_normal((K, M)) * scale).astype(np.float32), (rng.standard_normal((K, N)) * scale).astype(np.float32))
    g = vec()
    s_list, y_list = [], []
    for _ in range(n_pairs):
        s = vec(0.3)
        d = ((0.5 + rng.random((K, M))).astype(np.float32), (0.5 + rng.random((K, N))).astype(np.float32))
        e = vec(0.02)
        y = (d[0] * s[0] + e[0], d[1] * s[1] + e[1])
        if inner(s, y) <= 0:        # (one element: the noise may outweigh it)
            y = (d[0] * s[0], d[1] * s[1])
        s_list.append(s)
        y_list.append(y)
    return g, s_list, y_list
