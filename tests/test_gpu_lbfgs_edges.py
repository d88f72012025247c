"""GPU tests of csrc/pmf_lbfgs.hip where tests/test_gpu_lbfgs.py stops: vectors longer than one grid (1024 workgroups x 256
threads x 4 floats = 1,048,576 floats, then grid-stride trips), the full history of 32 pairs, k_lb_grad element by element
against the fp64 oracle, the device-side decisions CASES never takes (tests/lbfgs_ref.py EDGE_CASES: a reset on a long
vector, a reset at every iteration, the non-descent fallback, a wrapping m = 2 queue), a history that never fills, and a
context with a past.  Tables and tolerances: tests/lbfgs_ref.py, measured by tests/test_lbfgs_host.py."""
import numpy as np
import pytest

import lbfgs_ref as R
from problems import make_problem, to_context
from test_gpu_parity import GRAD_TOL

pytestmark = pytest.mark.gpu


# ---- a. directions -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized_ctx(pkg):
    """One context at a time, resized only when (M, N) or K changes (the data matrix only fixes M and N)."""
    state = dict(c=None, MN=None, K=None)

    def get(K, M, N):
        if state["MN"] != (M, N):
            if state["c"] is not None:
                state["c"].close()
            state.update(c=pkg.Context(0), MN=(M, N), K=None)
            state["c"].set_data(np.zeros((M, N), np.float32, order="F"))
        if state["K"] != K:
            state["c"].set_factors(np.zeros((K, M), np.float32, order="F"), np.zeros((K, N), np.float32, order="F"))
            state["K"] = K
        return state["c"]
    yield get
    if state["c"] is not None:
        state["c"].close()


@pytest.mark.parametrize("case", R.EDGE_DIRECTIONS, ids=lambda s: "x".join(map(str, s[:3])) + f"-{s[3]}pairs")
def test_edge_direction_matches_fp64_restatement(sized_ctx, case):
    K, M, N, n_pairs = case
    c = sized_ctx(K, M, N)
    g, s, y = R.random_history(K, M, N, n_pairs, seed=K + n_pairs)
    want = R.two_loop(g, s, y, np.float64)
    got = c.debug_lbfgs_direction(s, y, g)
    den = max(float(np.max(np.abs(want[i]))) for i in (0, 1))
    err = max(float(np.max(np.abs(got[i] - want[i]))) for i in (0, 1)) / den
    print(f"{case}: direction error {err:.3g} (tolerance {R.DIR_TOL_EDGE:.3g})")
    assert err <= R.DIR_TOL_EDGE
    again = c.debug_lbfgs_direction(s, y, g)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


# ---- b. the total gradient, element by element -------------------------------------------------------------------------
# m = 1, one iteration, one trial, no history: p = -g and the trial writes X1 = fl(X0 - g) whether or not it is accepted, so
# X0 - X1 is k_lb_grad's output up to the rounding of that one subtraction (half an ulp of X1: the 2^-23 max(|X0|, |X1|) term
# is twice that).  No Poisson columns: exp at the full step would overflow the trial's loss, not the step.
GRAD_SHAPES = [(1, 33, 70), (31, 5, 9), (33, 37, 29), (64, 3, 2), (32, 33000, 2), (32, 2, 33000)]
GRAD_REGS = [("l2", "l2"), ("group", "fsard"), ("composite", "ard_gap")]


def grad_problem(K, M, N, xreg, yreg):
    return make_problem(M=M, N=N, K=K, seed=13, bernoulli_frac=0.2, n_views=2, batch_views=2, n_batches=min(4, M),
                        nan_frac=0.1, weights=True, col_params=True, xreg=xreg, yreg=yreg, scale=0.5 if K > 8 else 1.0)


def one_full_step(ctx, p):
    to_context(p, ctx)
    r = ctx.fit_lbfgs(m=1, max_iter=1, backtrack_max_iter=1, rel_tol=0, abs_tol=0)
    assert r["iters"] == 1 and r["trials"].tolist() == [1] and r["grad_evals"] == 1 and (r["flags"][0] & 3) == 0
    # get_factors shows rows k < K only.  The pad rows k >= K must have stayed zero: one that took a value (NaN from an
    # ARD term, whose beta is zero there) would reach the trial's loss through X'Y
    assert np.isfinite(r["final_loss"]) and r["final_loss"] == r["loss"][0]
    X1, Y1 = ctx.get_factors()
    g64 = R.oracle_fun(p, 64)[0](p["X"], p["Y"])[1]
    return [(w, np.asarray(a0, np.float64), np.asarray(a1, np.float64), np.asarray(g, np.float64))
            for w, a0, a1, g in (("X", p["X"], X1, g64[0]), ("Y", p["Y"], Y1, g64[1]))]


@pytest.mark.parametrize("regs", GRAD_REGS, ids="-".join)
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_total_gradient_element_by_element(ctx, shape, regs):
    K, M, N = shape
    p = grad_problem(K, M, N, *regs)
    assert "poisson" not in p["noise_kinds"]
    bad = []
    for w, a0, a1, g64 in one_full_step(ctx, p):
        assert np.max(np.abs(g64)) > 0
        bound = GRAD_TOL * np.max(np.abs(g64)) + 2.0 ** -23 * np.maximum(np.abs(a0), np.abs(a1))
        ratio = float(np.max(np.abs((a0 - a1) - g64) / bound))
        print(f"{shape} {regs} {w}: worst |g - g64| / bound = {ratio:.3g}")
        if not ratio <= 1.0:
            bad.append((w, ratio))
    assert not bad, bad
    # no data term: what is left is the regularizer's gradient alone, a few f32 roundings per element (2^-21 = eight half
    # ulps, of the gradient and of the subtraction's operand); a weight, centre or alpha of the neighbouring column or
    # group is off by its full size
    q = dict(p, D=np.asfortranarray(np.full((M, N), np.nan, np.float32)))
    for w, a0, a1, g64 in one_full_step(ctx, q):
        assert np.max(np.abs(g64)) > 0
        bound = 2.0 ** -21 * (np.abs(g64) + np.abs(a0))
        err = np.abs((a0 - a1) - g64)
        ratio = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"{shape} {regs} {w} (no data): worst |g - g64| / bound = {ratio:.3g}")
        if not np.all(err <= bound):
            bad.append((w + " (no data)", ratio))
    assert not bad, bad


# ---- c. trajectories ---------------------------------------------------------------------------------------------------
def _edge_fit(ctx, case, p, h, **kw):
    to_context(p, ctx)
    opts = dict(m=case["m"], max_iter=h, backtrack_max_iter=case["backtrack_max_iter"], rel_tol=0, abs_tol=0)
    if "sy_min" in case:
        opts["sy_min"] = case["sy_min"]
    opts.update(kw)
    return ctx.fit_lbfgs(**opts), ctx.get_factors()


@pytest.mark.parametrize("name", [c["name"] for c in R.EDGE_CASES])
def test_edge_trajectory_takes_the_fp64_decisions(ctx, name):
    case = R.case_by_name(name)
    p, r64 = R.case_run(name, 64)
    h = R.horizon(r64)
    assert h >= R.MIN_HORIZON
    r, (X, Y) = _edge_fit(ctx, case, p, h)
    assert r["iters"] == h and len(r["loss"]) == h
    dev = float(np.max(np.abs(r["loss"] - r64["loss"][:h]) / np.abs(r64["loss"][:h])))
    print(f"{name}: horizon {h}, trials {r['trials'].tolist()}, flags {r['flags'].tolist()}, loss deviation {dev:.3g} "
          f"(tolerance {R.LOSS_TOL_EDGE[name]:.3g})")
    np.testing.assert_array_equal(r["trials"], r64["trials"][:h])
    np.testing.assert_array_equal(r["flags"], r64["flags"][:h])
    assert dev <= R.LOSS_TOL_EDGE[name]
    assert r["loss_evals"] == 1 + int(r64["trials"][:h].sum()) and r["grad_evals"] == h
    assert r["resets"] == int((r64["flags"][:h] & 1).sum())
    if name == "reset_every":
        assert r["resets"] == r["iters"] - 1
        r1, (X1, Y1) = _edge_fit(ctx, case, p, h, m=1)       # no pair ever survives: the queue's length cannot matter
        for k in ("loss", "trials", "flags"):
            np.testing.assert_array_equal(r1[k], r[k], err_msg=k)
        assert r1["resets"] == r["resets"] and np.array_equal(X1, X) and np.array_equal(Y1, Y)


# ---- d. a history that never fills -------------------------------------------------------------------------------------
def test_unfilled_history_does_not_depend_on_m(ctx):
    case = R.case_by_name("normal_l2")
    p, _ = R.case_run("normal_l2", 64)
    runs = [_edge_fit(ctx, case, p, R.MAX_ITER, m=m) for m in (32, R.MAX_ITER)]      # at most 13 pairs: neither queue fills
    (ra, (Xa, Ya)), (rb, (Xb, Yb)) = runs
    assert ra["iters"] == rb["iters"] == R.MAX_ITER
    for k in ("loss", "trials", "flags"):
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    assert np.array_equal(Xa, Xb) and np.array_equal(Ya, Yb)


# ---- e. the context's past does not matter -----------------------------------------------------------------------------
def test_fits_on_a_used_context_equal_fits_on_fresh_ones(pkg, ctx):
    pa = make_problem(**R.case_by_name("normal_l2")["problem"])
    pb = make_problem(**R.case_by_name("pad_rows_k33")["problem"])                   # another M, N and K_p
    assert (pa["M"], pa["N"], pa["K"]) != (pb["M"], pb["N"], pb["K"])

    def fit(c, p, m):
        to_context(p, c)
        r = c.fit_lbfgs(m=m, max_iter=8, rel_tol=0, abs_tol=0)
        assert r["iters"] == 8
        return [r["loss"], r["trials"], r["flags"], np.array(r["resets"])] + list(c.get_factors())

    to_context(pa, ctx)
    g, s, y = R.random_history(pa["K"], pa["M"], pa["N"], 3, seed=5)
    ctx.debug_lbfgs_direction(s, y, g)
    steps = [(pa, 10), (pa, 3), (pb, 10), (pa, 10)]
    used = [fit(ctx, p, m) for p, m in steps]
    for i, (p, m) in enumerate(steps):
        fresh = pkg.Context(0)
        try:
            want = fit(fresh, p, m)
        finally:
            fresh.close()
        for a, b in zip(used[i], want):
            np.testing.assert_array_equal(a, b, err_msg=f"fit {i} (m = {m})")
