"""L-BFGS on the host: the restatement tests/lbfgs_ref.py against dense BFGS and against each quirk DESIGN.md section 2
("Deviation 2 / L-BFGS") lists, the decision horizon of every table case, and the tolerance constants the GPU tests use."""
import ctypes

import numpy as np
import pytest

import lbfgs_ref as R


# ---- the recursion equals -H g for the dense BFGS inverse built from the same pairs
@pytest.mark.parametrize("n,n_pairs,seed", [(1, 1, 0), (7, 3, 1), (40, 10, 2), (40, 25, 3)])
def test_two_loop_equals_dense_bfgs(n, n_pairs, seed):
    rng = np.random.default_rng(seed)
    nx = n // 2
    A = rng.standard_normal((n, n))
    A = A @ A.T + n * np.eye(n)                        # y = A s: <s, y> > 0
    g = rng.standard_normal(n)
    S = [rng.standard_normal(n) for _ in range(n_pairs)]
    Y = [A @ s for s in S]
    split = lambda v: (v[:nx].reshape(1, -1), v[nx:].reshape(1, -1))
    p = R.two_loop(split(g), [split(s) for s in S], [split(y) for y in Y])
    p = np.concatenate([p[0].ravel(), p[1].ravel()])
    H = (S[0] @ Y[0]) / (Y[0] @ Y[0]) * np.eye(n)      # gamma I of the NEWEST pair
    for s, y in zip(S[::-1], Y[::-1]):                 # oldest first
        rho = 1.0 / (y @ s)
        V = np.eye(n) - rho * np.outer(s, y)
        H = V @ H @ V.T + rho * np.outer(s, s)
    want = -H @ g
    assert np.max(np.abs(p - want)) <= 1e-12 * np.max(np.abs(want))


# ---- quirks on hand-made objectives
def quad(a):
    """0.5 sum a x^2 over (X, Y) with per-element curvatures a = (aX, aY)."""
    def fun(X, Y):
        return 0.5 * float(np.sum(a[0] * X * X) + np.sum(a[1] * Y * Y)), (a[0] * X, a[1] * Y)
    return fun


def test_dd_nonnegative_keeps_stale_norm_and_dd():
    # negative curvature along the first coordinate makes <s, y> < 0; sy_min = -inf keeps that pair in the queue (the reset
    # test would drop it), the recursion then returns an ascent direction and the dd >= 0 branch is reached
    def f(X, Y):
        v = np.concatenate([X.ravel(), Y.ravel()])
        return float(-0.25 * v[0] ** 2 + v[1] ** 2 + v[2] ** 2 + 5.0), (np.array([[-0.5 * v[0], 2 * v[1]]]), np.array([[2 * v[2]]]))
    r = R.fit_lbfgs(f, np.array([[4.0, 1.0]]), np.array([[1.0]]), max_iter=3, sy_min=-np.inf, abs_tol=0, rel_tol=0)
    fl = r["flags"]
    assert (fl & 2).any(), fl
    lg = r["log"][int(np.nonzero(fl & 2)[0][0])]
    g, rejected = lg["g"], lg["p_first"]
    assert lg["dd"] >= 0
    # p_norm and dd are the REJECTED direction's ...
    assert lg["p_norm0"] == np.sqrt(R.inner(rejected, rejected)) != np.sqrt(R.inner(g, g))
    assert lg["dd"] == R.inner(rejected, g) / lg["p_norm0"]
    # ... while the step taken is along -g
    step = np.concatenate([lg["step"][0].ravel(), lg["step"][1].ravel()])
    mg = -np.concatenate([g[0].ravel(), g[1].ravel()])
    assert abs(step @ mg - np.linalg.norm(step) * np.linalg.norm(mg)) <= 1e-12 * np.linalg.norm(step) * np.linalg.norm(mg)


def test_reset_clears_the_pushed_pair_and_queue_is_bounded():
    # concave along one coordinate: <s, y> < 0 <= sy_min at the second iteration
    def f(X, Y):
        return float(-np.sum(X * X) + np.sum(Y * Y) + 100.0), (-2 * X, 2 * Y)
    r = R.fit_lbfgs(f, np.array([[1.0]]), np.array([[0.0]]), max_iter=3, abs_tol=0, rel_tol=0, backtrack_max_iter=5)
    assert r["flags"][1] & 1 and r["log"][1]["qlen"] == 0 and r["resets"] >= 1
    # the queue never exceeds m
    rng = np.random.default_rng(0)
    a = (1.0 + 9.0 * rng.random((2, 5)), 1.0 + 9.0 * rng.random((2, 4)))
    r = R.fit_lbfgs(quad(a), rng.standard_normal((2, 5)), rng.standard_normal((2, 4)), m=3, max_iter=9, abs_tol=0, rel_tol=0)
    q = [l["qlen"] for l in r["log"]]
    assert max(q) == 3 and q[:4] == [0, 1, 2, 3]


def test_exhaustion_leaves_p_one_shrink_past_the_step():
    a = (np.full((1, 2), 1e4), np.full((1, 1), 1e4))               # the unit step along -g overshoots by far
    r = R.fit_lbfgs(quad(a), np.ones((1, 2)), np.ones((1, 1)), max_iter=1, backtrack_max_iter=3, backtrack_shrinkage=0.5,
                    abs_tol=0, rel_tol=0)
    assert r["flags"][0] & 4 and r["trials"][0] == 3
    lg = r["log"][0]
    np.testing.assert_allclose(lg["p"][0], 0.5 * lg["step"][0], rtol=1e-15)
    np.testing.assert_allclose(lg["p"][1], 0.5 * lg["step"][1], rtol=1e-15)
    assert r["final_loss"] == r["loss"][0]                          # l1 is returned whatever its value


def test_zero_direction_stops_at_once():
    a = (np.ones((2, 3)), np.ones((2, 2)))
    r = R.fit_lbfgs(quad(a), np.zeros((2, 3)), np.zeros((2, 2)), max_iter=5)
    assert r["term_code"] == "abs_tol" and r["iters"] == 0 and r["loss_evals"] == 1 and len(r["loss"]) == 0
    assert not r["X"].any() and not r["Y"].any()


# ---- decision horizon of the table cases, and the f32 twin over it
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_case_horizon_and_twin(name):
    c = R.case_by_name(name)
    _, r64 = R.case_run(name, 64)
    _, r32 = R.case_run(name, 32)
    h = R.horizon(r64)
    assert h >= R.MIN_HORIZON, (h, r64["margin"])
    assert len(r32["loss"]) >= h
    np.testing.assert_array_equal(r32["trials"][:h], r64["trials"][:h])
    np.testing.assert_array_equal(r32["flags"][:h], r64["flags"][:h])
    dev = float(np.max(np.abs(r32["loss"][:h] - r64["loss"][:h]) / np.abs(r64["loss"][:h])))
    print(f"{name}: horizon {h}, twin loss deviation {dev:.3g}, tolerance {R.LOSS_TOL[name]:.3g}")
    assert R.LOSS_TOL[name] >= 2e-6 and dev <= R.LOSS_TOL[name] / 10
    if c["m"] == 3:
        assert max(l["qlen"] for l in r64["log"][:h]) == 3         # a full queue inside the horizon
    if c["backtrack_max_iter"] == 2:
        assert (r64["flags"][:h] & 4).any()                        # an exhausted backtrack inside the horizon


def test_table_covers_multi_trial_full_queue_and_exhaustion():
    runs = {c["name"]: R.case_run(c["name"], 64)[1] for c in R.CASES}
    assert any((r["trials"][:R.horizon(r)] > 1).any() for r in runs.values())
    assert any(c["m"] == 3 for c in R.CASES) and any(c["backtrack_max_iter"] == 2 for c in R.CASES)


def test_direction_tolerance_constant():
    worst = 0.0
    for K, M, N in R.DIRECTION_SHAPES:
        for n in R.DIRECTION_PAIRS:
            g, s, y = R.random_history(K, M, N, n, seed=K + n)
            p64, p32 = R.two_loop(g, s, y, np.float64), R.two_loop(g, s, y, np.float32)
            num = max(float(np.max(np.abs(p32[i] - p64[i]))) for i in (0, 1))
            den = max(float(np.max(np.abs(p64[i]))) for i in (0, 1))
            worst = max(worst, num / den)
    print(f"direction: twin deviation {worst:.3g}, tolerance {R.DIR_TOL:.3g}")
    assert R.DIR_TOL >= 2e-6 and worst <= R.DIR_TOL / 10


# ---- the edge tables: what each case is there for, and the tolerance constants of tests/test_gpu_lbfgs_edges.py
def test_first_iteration_is_no_reset():
    # sy_min >= 1 fails the reset test on the first iteration too (sy = 1 without a pair): the direction is -g as ever, but
    # with no history to forget neither the flag nor the count moves
    rng = np.random.default_rng(0)
    a = (1.0 + 9.0 * rng.random((2, 5)), 1.0 + 9.0 * rng.random((2, 4)))
    X0, Y0 = rng.standard_normal((2, 5)), rng.standard_normal((2, 4))
    r = R.fit_lbfgs(quad(a), X0, Y0, max_iter=4, sy_min=1e30, abs_tol=0, rel_tol=0)
    assert r["flags"].tolist() == [0, 1, 1, 1] and r["resets"] == 3
    assert [l["qlen"] for l in r["log"]] == [0, 0, 0, 0]
    g = quad(a)(X0, Y0)[1]
    assert np.array_equal(r["log"][0]["p_first"][0], -g[0]) and np.array_equal(r["log"][0]["p_first"][1], -g[1])
    r1 = R.fit_lbfgs(quad(a), X0, Y0, max_iter=1, sy_min=1.0, abs_tol=0, rel_tol=0)      # sy = 1 > 1 fails as well
    assert r1["flags"].tolist() == [0] and r1["resets"] == 0


@pytest.mark.parametrize("name", [c["name"] for c in R.EDGE_CASES])
def test_edge_case_horizon_and_twin(name):
    c = R.case_by_name(name)
    assert c["problem"]["random_init"]
    _, r64 = R.case_run(name, 64)
    _, r32 = R.case_run(name, 32)
    h = R.horizon(r64)
    assert h >= R.MIN_HORIZON, (h, r64["margin"])
    assert len(r32["loss"]) >= h
    np.testing.assert_array_equal(r32["trials"][:h], r64["trials"][:h])
    np.testing.assert_array_equal(r32["flags"][:h], r64["flags"][:h])
    dev = float(np.max(np.abs(r32["loss"][:h] - r64["loss"][:h]) / np.abs(r64["loss"][:h])))
    print(f"{name}: horizon {h}, flags {r64['flags'][:h].tolist()}, twin loss deviation {dev:.3g}, "
          f"tolerance {R.LOSS_TOL_EDGE[name]:.3g}")
    assert R.LOSS_TOL_EDGE[name] >= 2e-6 and dev <= R.LOSS_TOL_EDGE[name] / 10
    fl, q = r64["flags"][:h], [l["qlen"] for l in r64["log"][:h]]
    if name == "wide_k32":
        p = c["problem"]
        assert 32 * (p["M"] + p["N"]) > 1024 * 256 * 4             # beyond one grid of four-element threads
        assert (fl[1:] & 1).any() and max(q) == c["m"]             # a reset and a full queue inside the horizon
    if name == "reset_every":
        assert fl[0] == 0 and (fl[1:] & 1).all() and max(q) == 0 and int((fl & 1).sum()) == h - 1
    if name == "non_descent":
        assert (fl & 2).any() and ((fl & 6) == 6).any()            # dd >= 0, once together with an exhausted backtrack
    if name == "m2_wrap":
        assert c["m"] == 2 and q[2:] == [2] * (h - 2) and h - 3 >= 6   # every push from the fourth iteration evicts a pair


def test_edge_direction_tolerance_constant():
    worst, shapes = 0.0, set()
    for K, M, N, n in R.EDGE_DIRECTIONS:
        g, s, y = R.random_history(K, M, N, n, seed=K + n)
        p64, p32 = R.two_loop(g, s, y, np.float64), R.two_loop(g, s, y, np.float32)
        num = max(float(np.max(np.abs(p32[i] - p64[i]))) for i in (0, 1))
        den = max(float(np.max(np.abs(p64[i]))) for i in (0, 1))
        worst = max(worst, num / den)
        shapes.add((32 * -(-K // 32) * (M + N) > 1024 * 256 * 4, n == 32))
    print(f"edge directions: twin deviation {worst:.3g}, tolerance {R.DIR_TOL_EDGE:.3g}")
    assert R.DIR_TOL_EDGE >= 2e-6 and worst <= R.DIR_TOL_EDGE / 10
    assert shapes == {(True, False), (False, True), (True, True)}  # beyond one grid, full history, and both at once


# ---- ABI
def test_lbfgs_struct_sizes(pkg):
    # pmf_lbfgs_opts: 6 int32 + 5 double ; pmf_lbfgs_result: 8 int32 + 2 double + 3 pointers
    assert ctypes.sizeof(pkg._lib.LbfgsOpts) == 6 * 4 + 5 * 8
    assert ctypes.sizeof(pkg._lib.LbfgsResult) == 8 * 4 + 2 * 8 + 3 * 8
