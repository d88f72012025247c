"""GPU tests of the L-BFGS factor initialisation (csrc/pmf_lbfgs.hip; DESIGN.md section 2 "Deviation 2 / L-BFGS", section
4.12): pmf_loss against the fp64 oracle, the recursion kernels against the fp64 restatement (tests/lbfgs_ref.py), whole
trajectories over each table case's decision horizon, the whole call, its edges and refusals, and the Python stage."""
import numpy as np
import pytest

import lbfgs_ref as R
from problems import make_problem, to_context, to_oracle
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

LOSS_RTOL = 2e-5          # the project's loss tolerance
INIT_TOLS = dict(rel_tol=1e-5, abs_tol=1e-5)   # init_factors! (src/fit.jl:256-257)


# ---- pmf_loss ----------------------------------------------------------------------------------------------------------
LOSS_CASES = {"k1": (33, 70, 1, "f32"), "k33": (601, 70, 33, "f32"), "k96": (257, 130, 96, "f32"), "k128": (64, 40, 128, "f32"),
              "k33_bf16": (601, 70, 33, "bf16")}


def loss_problem(name):
    M, N, K, store = LOSS_CASES[name]
    p = make_problem(M=M, N=N, K=K, seed=11, bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2, n_batches=4,
                     nan_frac=0.1, weights=True, col_params=True, xreg="group", yreg="fsard", scale=0.5 if K > 8 else 1.0)
    if store == "bf16":
        p["D"] = np.asfortranarray(bf16_round(p["D"]))
    return p, store


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_loss_matches_oracle_and_ignores_precision_mode(ctx, name):
    p, store = loss_problem(name)
    to_context(p, ctx)
    if store != "f32":
        ctx.set_data(p["D"], store=store)
    try:
        v = ctx.loss()
        m = to_oracle(p)
        want, g = m.loss_and_grads(update_X=True, update_Y=True)
        print(f"{name}: pmf_loss {v['total']:.9g} oracle {want:.9g} rel {abs(v['total'] - want) / abs(want):.3g}")
        assert abs(v["total"] - want) <= LOSS_RTOL * abs(want)
        assert abs(v["data"] - g["data_loss"]) <= LOSS_RTOL * abs(g["data_loss"])
        assert v["total"] == v["data"] + v["xreg"] + v["yreg"] and v["xreg"] > 0 and v["yreg"] > 0
        ctx.set_precision("bf16x3")
        n0 = ctx.get_precision()[1]
        assert ctx.loss() == v                                  # bitwise, and through the exact kernel
        assert ctx.get_precision()[1] == n0 and ctx.last_kernel() == 0
    finally:
        ctx.set_precision("f32")


def test_fit_after_loss_is_bitwise_the_fit_without_it(ctx):
    p, _ = loss_problem("k33")

    def run(with_loss):
        to_context(p, ctx)
        ctx.set_optimizer("adagrad", lr=0.05)
        if with_loss:
            ctx.loss()
        r = ctx.fit(update_X=True, update_Y=True, max_epochs=5, abs_tol=0, rel_tol=0)
        return r["loss"], ctx.get_factors()
    la, (Xa, Ya) = run(False)
    lb, (Xb, Yb) = run(True)
    assert np.array_equal(la, lb) and np.array_equal(Xa, Xb) and np.array_equal(Ya, Yb)


# ---- the recursion kernels ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shaped_ctx(pkg):
    """A context per direction shape (the data matrix only fixes M and N)."""
    made = {}

    def get(K, M, N):
        if (K, M, N) not in made:
            c = pkg.Context(0)
            c.set_data(np.zeros((M, N), np.float32, order="F"))
            c.set_factors(np.zeros((K, M), np.float32, order="F"), np.zeros((K, N), np.float32, order="F"))
            made[(K, M, N)] = c
        return made[(K, M, N)]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("n_pairs", R.DIRECTION_PAIRS)
@pytest.mark.parametrize("shape", R.DIRECTION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_direction_matches_fp64_restatement(shaped_ctx, shape, n_pairs):
    K, M, N = shape
    c = shaped_ctx(K, M, N)
    g, s, y = R.random_history(K, M, N, n_pairs, seed=K + n_pairs)
    want = R.two_loop(g, s, y, np.float64)
    got = c.debug_lbfgs_direction(s, y, g)
    den = max(float(np.max(np.abs(want[i]))) for i in (0, 1))
    err = max(float(np.max(np.abs(got[i] - want[i]))) for i in (0, 1)) / den
    print(f"{shape} n_pairs {n_pairs}: direction error {err:.3g} (tolerance {R.DIR_TOL:.3g})")
    assert err <= R.DIR_TOL
    again = c.debug_lbfgs_direction(s, y, g)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])


def test_direction_refuses_33_pairs(pkg, shaped_ctx):
    c = shaped_ctx(1, 1, 1)
    g, s, y = R.random_history(1, 1, 1, 33, seed=0)
    with pytest.raises(pkg.PMFError, match="n_pairs = 33"):
        c.debug_lbfgs_direction(s, y, g)


# ---- trajectories over the decision horizon ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_trajectory_takes_the_fp64_decisions(ctx, name):
    case = R.case_by_name(name)
    p, r64 = R.case_run(name, 64)
    h = R.horizon(r64)
    assert h >= R.MIN_HORIZON
    to_context(p, ctx)
    r = ctx.fit_lbfgs(m=case["m"], max_iter=h, backtrack_max_iter=case["backtrack_max_iter"], rel_tol=0, abs_tol=0)
    assert r["iters"] == h and len(r["loss"]) == h
    dev = float(np.max(np.abs(r["loss"] - r64["loss"][:h]) / np.abs(r64["loss"][:h])))
    print(f"{name}: horizon {h}, trials {r['trials'].tolist()}, flags {r['flags'].tolist()}, loss deviation {dev:.3g} "
          f"(tolerance {R.LOSS_TOL[name]:.3g})")
    np.testing.assert_array_equal(r["trials"], r64["trials"][:h])
    np.testing.assert_array_equal(r["flags"], r64["flags"][:h])
    assert dev <= R.LOSS_TOL[name]
    assert r["loss_evals"] == 1 + int(r64["trials"][:h].sum()) and r["grad_evals"] == h


# ---- the whole call ----------------------------------------------------------------------------------------------------
def whole_problem():
    return make_problem(M=300, N=200, K=4, seed=21, nan_frac=0.05, xreg="l2", yreg="l2", random_init=True)


def test_whole_call_converges_repeats_and_leaves_the_optimizer_alone(pkg, ctx):
    p = whole_problem()
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=0.05)
    ctx.fit(update_X=True, update_Y=True, max_epochs=2, abs_tol=0, rel_tol=0)      # some optimizer state to leave alone
    ctx.set_factors(p["X"], p["Y"])
    state0 = [ctx.get_opt_state(w) for w in ("X", "Y")]
    lr0 = ctx.get_lr()
    r = ctx.fit_lbfgs(max_iter=300, **INIT_TOLS)
    X1, Y1 = ctx.get_factors()
    assert r["term_code"] in ("abs_tol", "rel_tol") and r["iters"] < 300, r
    ok = (r["flags"] & 6) == 0
    prev = np.concatenate([[np.inf], r["loss"][:-1]])
    assert np.all(r["loss"][ok] <= prev[ok])
    assert r["final_loss"] == ctx.loss()["total"] == r["loss"][-1]
    for w, (a0, m0) in zip(("X", "Y"), state0):
        a1, m1 = ctx.get_opt_state(w)
        assert np.array_equal(a0, a1) and np.array_equal(m0, m1)
    assert ctx.get_lr() == lr0
    # a second run from the same start repeats bit for bit
    ctx.set_factors(p["X"], p["Y"])
    r2 = ctx.fit_lbfgs(max_iter=300, **INIT_TOLS)
    X2, Y2 = ctx.get_factors()
    assert np.array_equal(r["loss"], r2["loss"]) and np.array_equal(r["trials"], r2["trials"])
    assert np.array_equal(X1, X2) and np.array_equal(Y1, Y2)
    # a pmf_fit after it equals a pmf_fit on a fresh context started from the same factors
    ctx.set_optimizer("adagrad", lr=0.05)
    ra = ctx.fit(update_X=True, update_Y=True, max_epochs=4, abs_tol=0, rel_tol=0)
    Xa, Ya = ctx.get_factors()
    fresh = pkg.Context(0)
    try:
        q = dict(p, X=X1, Y=Y1)
        to_context(q, fresh)
        fresh.set_optimizer("adagrad", lr=0.05)
        rb = fresh.fit(update_X=True, update_Y=True, max_epochs=4, abs_tol=0, rel_tol=0)
        Xb, Yb = fresh.get_factors()
    finally:
        fresh.close()
    assert np.array_equal(ra["loss"], rb["loss"]) and np.array_equal(Xa, Xb) and np.array_equal(Ya, Yb)


# ---- edges -------------------------------------------------------------------------------------------------------------
def small_problem(**kw):
    return make_problem(M=40, N=33, K=2, seed=3, xreg="l2", yreg="l2", random_init=True, **kw)


def test_max_iter_zero_returns_the_start_loss(ctx):
    p = small_problem()
    to_context(p, ctx)
    r = ctx.fit_lbfgs(max_iter=0)
    X, Y = ctx.get_factors()
    assert r["term_code"] == "max_epochs" and r["iters"] == 0 and len(r["loss"]) == 0 and r["grad_evals"] == 0
    assert r["final_loss"] == ctx.loss()["total"]
    assert np.array_equal(X, p["X"]) and np.array_equal(Y, p["Y"])


def test_m_one_follows_the_restatement(ctx):
    p = small_problem()
    to_context(p, ctx)
    fun, _ = R.oracle_fun(p, 64)
    r64 = R.fit_lbfgs(fun, p["X"], p["Y"], m=1, max_iter=8, rel_tol=0, abs_tol=0)
    h = R.horizon(r64)
    assert h >= 4
    r = ctx.fit_lbfgs(m=1, max_iter=h, rel_tol=0, abs_tol=0)
    np.testing.assert_array_equal(r["trials"], r64["trials"][:h])
    np.testing.assert_array_equal(r["flags"], r64["flags"][:h])
    np.testing.assert_allclose(r["loss"], r64["loss"][:h], rtol=R.LOSS_TOL["exhaust_bt2"])   # (the same problem)


def test_zero_start_is_stationary(ctx):
    p = small_problem()
    p["X"][...] = 0
    p["Y"][...] = 0
    to_context(p, ctx)
    l0 = ctx.loss()["total"]
    r = ctx.fit_lbfgs(max_iter=5)
    X, Y = ctx.get_factors()
    assert r["term_code"] == "abs_tol" and r["iters"] == 0 and r["loss_evals"] == 1
    assert r["final_loss"] == l0 and np.isfinite(l0) and not X.any() and not Y.any()


def test_refusals_name_their_cause(pkg, ctx):
    fresh = pkg.Context(0)
    try:
        with pytest.raises(pkg.PMFError, match="data not set"):
            fresh.fit_lbfgs()
        with pytest.raises(pkg.PMFError, match="data not set"):
            fresh.loss()
        fresh.set_data(np.zeros((4, 3), np.float32, order="F"))
        with pytest.raises(pkg.PMFError, match="factors not set"):
            fresh.fit_lbfgs()
    finally:
        fresh.close()
    p = small_problem()
    to_context(p, ctx)
    for kw, pat in ((dict(m=0), "m = 0"), (dict(m=33), "m = 33"), (dict(backtrack_shrinkage=1.0), "backtrack_shrinkage"),
                    (dict(backtrack_shrinkage=0.0), "backtrack_shrinkage"), (dict(max_iter=-1), "max_iter"),
                    (dict(backtrack_max_iter=0), "backtrack_max_iter")):
        with pytest.raises(pkg.PMFError, match=pat):
            ctx.fit_lbfgs(**kw)
    ctx.add_reg_l1("Y", np.ones(p["K"], np.float32))
    with pytest.raises(pkg.PMFError, match="L1"):
        ctx.fit_lbfgs()
    to_context(p, ctx)
    import scipy.sparse as sp
    n, K = p["N"], p["K"]
    AA = [sp.identity(n, format="csr", dtype=np.float32) for _ in range(K)]
    AB = [sp.csr_matrix((n, 0), dtype=np.float32) for _ in range(K)]
    BB = [sp.csr_matrix((0, 0), dtype=np.float32) for _ in range(K)]
    ctx.add_reg_network("Y", AA, AB, BB)
    with pytest.raises(pkg.PMFError, match="network"):
        ctx.fit_lbfgs()
    with pytest.raises(pkg.PMFError, match="network"):
        ctx.loss()
    to_context(p, ctx)
    ctx.comm_init_host(0, 2, lambda arr: None)
    try:
        with pytest.raises(pkg.PMFError, match="2 ranks"):
            ctx.fit_lbfgs()
    finally:
        ctx.comm_destroy()
    assert ctx.fit_lbfgs(max_iter=1)["iters"] == 1               # the context is still usable


# ---- the Python stage --------------------------------------------------------------------------------------------------
def stage_model(pkg, seed=41):
    rng = np.random.default_rng(seed)
    M, N, K = 60, 60, 3
    D = (rng.standard_normal((K, M)).T @ rng.standard_normal((K, N)) + 0.1 * rng.standard_normal((M, N))).astype(np.float32)
    return pkg.make_model(D, K=K, feature_views=[1] * 30 + [2] * 30, rng=rng)


def test_init_factors_lbfgs_stage(pkg):
    model = stage_model(pkg)
    mf = model.matfac
    xr, yr = mf.X_reg, mf.Y_reg
    X0, Y0 = mf.X.copy(), mf.Y.copy()
    L2 = pkg.regularizers.L2Regularizer

    def swapped_loss():
        c = model.device_context()
        mf.X_reg, mf.Y_reg = L2(np.full(3, 0.1, np.float32)), L2(np.full(3, 0.1, np.float32))
        try:
            pkg.matfac.marshal(mf, c)
        finally:
            mf.X_reg, mf.Y_reg = xr, yr
        return c.loss()["total"]
    try:
        before = swapped_loss()
        hist = []
        pkg.init_factors_(model, init_factors_method="lbfgs", max_epochs=30, verbosity=0, history=hist)
        after = swapped_loss()
        assert after < before
        assert not np.array_equal(mf.X, X0) and not np.array_equal(mf.Y, Y0)
        assert mf.X_reg is xr and mf.Y_reg is yr
        assert hist[-1]["name"] == "init_factors_lbfgs"
    finally:
        model.release_device()


def test_fit_with_lbfgs_initialisation_completes(pkg):
    model = stage_model(pkg, seed=42)
    try:
        hist = pkg.fit_(model, init_factors_method="lbfgs", max_epochs=20, verbosity=0, keep_history=True)
        names = [h.get("name") for h in hist]
        assert "init_factors_lbfgs" in names and names[-1] == "finish"
        assert np.isfinite(model.matfac.X).all() and np.isfinite(model.matfac.Y).all()
    finally:
        model.release_device()
