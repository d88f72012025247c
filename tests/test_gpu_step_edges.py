"""The regularizer + optimizer step (k_reg_step<false> / k_reg_step<true>, the range expanders, step_param_range, step_layers
and the optimizer-state entry points) at size, range, chunk and state edges.

The step is elementwise: given the device's own data gradient (pmf_get_grad after pmf_epoch_begin) and its own parameter
and state before the step, the result is a closed formula.  tests/step_ref.py evaluates it in float64 from the ABI's
arguments; every element of the stepped parameter and of both state arrays is compared, at limits set by the float32 twin
of the same formulas (tests/test_step_cases.py guards both on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import step_ref as sr
from problems import make_problem, rel_err, to_context, to_oracle
from test_gpu_coverage import FIT_TOL, GRAD_TOL, LOSS_RTOL

pytestmark = pytest.mark.gpu
OPTS = ["adagrad", "adam"]
XY = [("X", 0), ("Y", 0)]


def _param(ctx, which, view=0):
    if which in ("X", "Y"):
        return ctx.get_factors()[0 if which == "X" else 1]
    if which in ("logsigma", "mu"):
        return ctx.get_col_params()[0 if which == "logsigma" else 1]
    return ctx.get_batch_view(view)[0 if which == "logdelta" else 1]


def _read(ctx, params, grad):
    out = {}
    for w, v in params:
        acc, mom = ctx.get_opt_state(w, v)
        out[w, v] = dict(p=_param(ctx, w, v), acc=acc, mom=mom)
        if grad:
            out[w, v]["g"] = ctx.get_grad(w, v)
    return out


def _case_opts(ctx, p, **kw):
    return ctx.make_opts(update_X=True, update_Y=True, update_col_layers=p.get("layers", False), **kw)


def one_step(ctx, p, opts, which, okw=None, fresh=True):
    """One step-level epoch.  fresh: marshal the problem and set the optimizer first (state from scratch); otherwise the
    context carries on.  Returns (before, after, local_loss, shared_terms): per parameter of `which` the device's data
    gradient, value and state before the step, and value and state after it."""
    if fresh:
        to_context(p, ctx)
        ctx.set_optimizer(**okw)
    ctx.epoch_begin(opts)
    before = _read(ctx, which, grad=True)
    ctx.epoch_step_local(opts)
    ctx.epoch_step_shared(opts)
    local, shared = ctx.epoch_loss()
    return before, _read(ctx, which, grad=False), local, shared


def data_term(ctx, p, opts):
    """The data term of the epoch: the same epoch with the regularizers cleared (the data pass does not depend on them)."""
    to_context(sr.without_regs(p), ctx)
    ctx.epoch_begin(opts)
    return ctx.epoch_loss()[0]


def check_step(p, before, after, okw, t, no_reg=(), frozen=()):
    """Every element of every parameter, acc and mom against step_ref on the device's own inputs.  no_reg: parameters that
    step on the data gradient alone; frozen: parameters that must keep value and state bit for bit.  Returns per
    parameter (value, vmag) of its regularizer."""
    vals = {}
    opt = okw["kind"]
    for (w, v), b in before.items():
        a = after[w, v]
        assert a["p"].shape == b["p"].shape == a["acc"].shape == a["mom"].shape == b["g"].shape, (w, v)
        if w in frozen:
            for k in ("p", "acc", "mom"):
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{w}[{v}].{k}")
            vals[w, v] = (0.0, 0.0)
            continue
        r = sr.expected_step(p, w, b["p"], b["g"], b["acc"], b["mom"], okw, t, v, use_reg=w not in no_reg)
        dp = sr.dev_param(a["p"], r["p"], b["p"], r["sens"], r["mag"])
        da = sr.dev_acc(a["acc"], r["acc"], b["acc"], r["mag"])
        dm = sr.dev_mom(a["mom"], r["mom"], b["mom"], r["mag"])
        print(f"{w}[{v}] {opt} t={t}: p {dp:.3g} / {sr.p_tol(opt, t):.3g}  acc {da:.3g} / {sr.ACC_TOL:.3g}  "
              f"mom {dm:.3g} / {sr.MOM_TOL:.3g}")
        assert dp <= sr.p_tol(opt, t), (w, v, dp)
        assert da <= sr.ACC_TOL, (w, v, da)
        assert dm <= sr.MOM_TOL, (w, v, dm)
        if opt == "adagrad":
            np.testing.assert_array_equal(a["mom"], b["mom"])
        vals[w, v] = (r["value"], r["vmag"])
    return vals


def check_values(vals, local, shared, data):
    """shared_terms = the value of the Y and layer regularizers; the X regularizer's value = local - shared - data (three
    f64 sums; the subtraction costs a few ulp of the loss)."""
    sv = sum(x[0] for k, x in vals.items() if k[0] != "X")
    sm = sum(x[1] for k, x in vals.items() if k[0] != "X")
    xv, xm = vals.get(("X", 0), (0.0, 0.0))
    print(f"values: shared {shared:.10g} (ref {sv:.10g}, dev {sr.dev_value(shared, sv, sm):.3g})  "
          f"X {local - shared - data:.10g} (ref {xv:.10g})  limit {sr.VAL_TOL:.3g}")
    assert abs(shared - sv) <= sr.VAL_TOL * sm, (shared, sv, sm)
    assert abs(local - shared - data - xv) <= sr.VAL_TOL * xm + 1e-14 * abs(local), (local, shared, data, xv)


# ---- the tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("table,name", sr.ALL_CASES)
def test_first_step_of_every_table_case(ctx, table, name, opt):
    """X, Y and (cases with layers) the four layer parameters, one joint epoch from fresh state."""
    p = sr.build_case(table, name)
    o = _case_opts(ctx, p)
    data = data_term(ctx, p, o)
    before, after, local, shared = one_step(ctx, p, o, sr.case_params(p), sr.OPT_KW[opt])
    for (w, v), b in before.items():              # the step starts where it is documented to start
        np.testing.assert_array_equal(b["p"], sr.param_value(p, w, v))
        acc0, mom0 = sr.fresh_state(b["p"].shape, opt, sr.OPT_KW[opt]["eps"])
        np.testing.assert_array_equal(b["acc"], acc0)
        np.testing.assert_array_equal(b["mom"], mom0)
    vals = check_step(p, before, after, sr.OPT_KW[opt], 1)
    check_values(vals, local, shared, data)


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("table,name", [("K_EDGES", "K33"), ("K_EDGES", "K100"), ("RANGE_EDGES", "batches_1_and_255")])
def test_five_consecutive_steps(ctx, table, name, opt):
    """1, 2 and 5 steps: the expected state is re-seeded from the device's before each step, so a wrong step shows where
    it happens; Adam's t runs free on the host.  The data gradient of steps 2-5 must be the oracle's on the stepped
    factors: a stepped pad row (k >= K) would enter the products."""
    p = sr.build_case(table, name)
    okw = sr.OPT_KW[opt]
    o = _case_opts(ctx, p)
    params = sr.case_params(p)
    m = to_oracle(sr.without_regs(p))
    prev = None
    for t in range(1, 6):
        before, after, _, _ = one_step(ctx, p, o, params, okw, fresh=t == 1)
        if prev is not None:                       # nothing moved between the epochs
            for k, b in before.items():
                for f in ("p", "acc", "mom"):
                    np.testing.assert_array_equal(b[f], prev[k][f])
            m.X[...], m.Y[...] = before["X", 0]["p"], before["Y", 0]["p"]
            for (w, v), b in before.items():
                if w not in ("X", "Y"):
                    (getattr(m, w)[v] if w in ("logdelta", "theta") else getattr(m, w))[...] = b["p"]
            _, go = m.loss_and_grads(update_X=True, update_Y=True, update_col_layers=p["layers"])
            for w in ("X", "Y"):
                assert rel_err(before[w, 0]["g"], go[w]) <= GRAD_TOL, (t, w, rel_err(before[w, 0]["g"], go[w]))
        check_step(p, before, after, okw, t)
        prev = after


# ---- Y stepped in column chunks by pmf_fit ---------------------------------------------------------------------------------
CHUNK_N = 200                                                             # 7 column tiles: not a multiple of 32 * chunks
STRADDLE = [(20, 40), (50, 70), (90, 100), (120, 135), (150, 170)]        # a group over every chunk boundary of 2, 3, 5
CHUNK_YREG = {
    "l2_group_ard": [("l2", 0.5), ("group", STRADDLE, 1.0), ("ard", [(1, 50), (70, 130), (140, 199)], 0.5)],
    "group_fsard": [("group", STRADDLE, 1.0), ("fsard", 1.0)],
}


def _chunk_problem(yreg):
    p = make_problem(M=150, N=CHUNK_N, K=24, seed=61, nan_frac=0.05, weights=True, random_init=True, scale=0.6, xreg="group")
    rng = np.random.default_rng(62)
    p["yreg"] = [sr._term(rng, s, 24, CHUNK_N) for s in CHUNK_YREG[yreg]]
    p["layers"] = False
    return p


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("yreg", sorted(CHUNK_YREG))
def test_chunked_y_step_through_fit(ctx, yreg, opt):
    p = _chunk_problem(yreg)
    okw = sr.OPT_KW[opt]
    for S in (2, 3, 5):
        for edge in sr.chunk_column_edges(CHUNK_N, S)[1:-1]:
            assert any(a <= edge < b for a, b in STRADDLE), (S, edge)
    kw = dict(update_X=True, update_Y=True, max_epochs=4, abs_tol=0, rel_tol=0)

    def fit():
        to_context(p, ctx)
        ctx.set_optimizer(**okw)
        r = ctx.fit(**kw)
        return (r,) + ctx.get_factors()

    r0, X0, Y0 = fit()
    try:
        for S in (2, 3, 5):
            ctx.comm_set_chunks(S)
            r1, X1, Y1 = fit()
            assert ctx.comm_info()["n_chunks"] == S
            assert r1["term_code"] == r0["term_code"] and r1["epochs"] == r0["epochs"] == 4
            np.testing.assert_allclose(r1["loss"], r0["loss"], rtol=5e-6)
            assert rel_err(X1, X0) <= FIT_TOL and rel_err(Y1, Y0) <= FIT_TOL, (S, rel_err(X1, X0), rel_err(Y1, Y0))
            if S == 3:
                # one more step-level epoch: the fifth step of X and of Y, whatever the chunking did in between
                before, after, _, _ = one_step(ctx, p, _case_opts(ctx, p), XY, fresh=False)
                np.testing.assert_array_equal(before["Y", 0]["p"], Y1)
                check_step(p, before, after, okw, 5)
    finally:
        ctx.comm_set_chunks(0)


# ---- frozen layer against frozen regularizer -------------------------------------------------------------------------------
LAYERS = [("logsigma", 0), ("mu", 0), ("logdelta", 0), ("theta", 0), ("logdelta", 1), ("theta", 1)]
BITS = [0b0001, 0b0010, 0b0100, 0b1000, 0b1111]


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("fl,fr", [(b, 0) for b in BITS] + [(0, b) for b in BITS] + [(0b0010, 0b0100)])
def test_frozen_layers_and_frozen_regs(ctx, fl, fr, opt):
    p = make_problem(M=120, N=90, K=8, seed=71, bernoulli_frac=0.2, n_views=2, batch_views=2, n_batches=4, nan_frac=0.05,
                     weights=True, col_params=True, layer_regs=True, random_init=True, scale=0.6)
    okw = sr.OPT_KW[opt]
    o = ctx.make_opts(update_col_layers=True, frozen_layers=fl, frozen_regs=fr)
    frozen = [w for w, b in sr.LAYER_BIT.items() if fl & b]
    no_reg = [w for w, b in sr.LAYER_BIT.items() if fr & b and not fl & b]
    data = data_term(ctx, p, o)
    before, after, local, shared = one_step(ctx, p, o, LAYERS, okw)
    vals = check_step(p, before, after, okw, 1, no_reg=no_reg, frozen=frozen)
    for (w, v), x in vals.items():
        if w in no_reg:
            vals[w, v] = (0.0, 0.0)                # a frozen regularizer contributes 0 to the loss
        elif w not in frozen:
            assert x[1] > 0                        # ... its neighbours do contribute
    check_values(vals, local, shared, data)
    X, Y = ctx.get_factors()
    np.testing.assert_array_equal(X, p["X"])
    np.testing.assert_array_equal(Y, p["Y"])
    # the whole epoch against the oracle
    m = to_oracle(p)
    ro = m.fit(update_col_layers=True, frozen_layers=fl, frozen_regs=fr, opt=opt, lr=okw["lr"], max_epochs=1, abs_tol=0, rel_tol=0)
    assert abs(local - ro["loss"][0]) <= LOSS_RTOL * abs(ro["loss"][0]), (local, ro["loss"][0])
    for w, v in LAYERS:
        want = getattr(m, w)[v] if w in ("logdelta", "theta") else getattr(m, w)
        assert rel_err(after[w, v]["p"], want) <= FIT_TOL, (w, v, rel_err(after[w, v]["p"], want))


# ---- state lifetime -----------------------------------------------------------------------------------------------------------
def _xy_problem(seed=81):
    p = make_problem(M=70, N=45, K=33, seed=seed, nan_frac=0.05, weights=True, random_init=True, scale=0.6, xreg="composite",
                     yreg="ard_gap", n_views=3)
    p["layers"] = False
    return p


@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("action", ["reset_optimizer_state", "set_optimizer", "set_lr"])
def test_what_restarts_the_optimizer_state(ctx, action, opt):
    """pmf_reset_optimizer_state and pmf_set_optimizer restore the starting acc / mom and Adam's t = 1: the step after them
    equals a first step.  pmf_set_lr does not: state and t carry on."""
    p = _xy_problem()
    okw = dict(sr.OPT_KW[opt])
    o = _case_opts(ctx, p)
    first = one_step(ctx, p, o, XY, okw)
    check_step(p, first[0], first[1], okw, 1)
    second = one_step(ctx, p, o, XY, fresh=False)
    check_step(p, second[0], second[1], okw, 2)
    if action == "set_lr":
        okw["lr"] = 0.5 * okw["lr"]
        ctx.set_lr(okw["lr"])
        assert ctx.get_lr() == np.float32(okw["lr"])
        third = one_step(ctx, p, o, XY, fresh=False)
        for k in XY:
            for f in ("p", "acc", "mom"):
                np.testing.assert_array_equal(third[0][k][f], second[1][k][f])
        check_step(p, third[0], third[1], okw, 3)
        return
    if action == "set_optimizer":
        ctx.set_optimizer(**okw)
    else:
        ctx.reset_optimizer_state()
    ctx.set_factors(p["X"], p["Y"])
    again = one_step(ctx, p, o, XY, fresh=False)
    for k in XY:
        acc0, mom0 = sr.fresh_state(first[0][k]["p"].shape, opt, okw["eps"])
        np.testing.assert_array_equal(again[0][k]["acc"], acc0)
        np.testing.assert_array_equal(again[0][k]["mom"], mom0)
        np.testing.assert_array_equal(again[0][k]["g"], first[0][k]["g"])       # the data pass is bitwise reproducible
        for f in ("p", "acc", "mom"):
            np.testing.assert_array_equal(again[1][k][f], first[1][k][f])
    check_step(p, again[0], again[1], okw, 1)


@pytest.mark.parametrize("opt", OPTS)
def test_state_survives_set_factors_across_two_fits(ctx, opt):
    """Two pmf_fit calls with the factors marshalled again in between (what mf_fit_adapt_lr! does between segments) are
    one fit: same bits, and the next step is the fifth -- Adam's t carries on too."""
    p = _xy_problem(82)
    okw = sr.OPT_KW[opt]
    kw = dict(update_X=True, update_Y=True, abs_tol=0, rel_tol=0)
    to_context(p, ctx)
    ctx.set_optimizer(**okw)
    ra = ctx.fit(max_epochs=4, **kw)
    Xa, Ya = ctx.get_factors()
    sa = _read(ctx, XY, grad=False)
    to_context(p, ctx)
    ctx.set_optimizer(**okw)
    rb1 = ctx.fit(max_epochs=2, **kw)
    X, Y = ctx.get_factors()
    ctx.set_factors(X, Y)
    rb2 = ctx.fit(epoch=3, max_epochs=4, **kw)
    assert (rb1["epochs"], rb2["epochs"]) == (2, 4)
    np.testing.assert_array_equal(np.concatenate([rb1["loss"], rb2["loss"]]), ra["loss"])
    sb = _read(ctx, XY, grad=False)
    for k in XY:
        for f in ("p", "acc", "mom"):
            np.testing.assert_array_equal(sb[k][f], sa[k][f])
    before, after, _, _ = one_step(ctx, p, _case_opts(ctx, p), XY, fresh=False)
    check_step(p, before, after, okw, 5)


def test_opt_state_of_batch_views_comes_in_each_views_shape(ctx):
    p = make_problem(M=60, N=50, K=8, seed=83, col_params=True, random_init=True, scale=0.6)
    rng = np.random.default_rng(84)
    p["batch_views"] = []
    for s1, e1, nb in ((1, 20, 3), (31, 50, 5)):
        bor = rng.permutation(np.concatenate([np.arange(nb), rng.integers(0, nb, size=60 - nb)])).astype(np.int32)
        p["batch_views"].append(dict(start1=s1, stop1=e1, batch_of_row=bor,
                                     logdelta=(0.25 * rng.standard_normal((nb, e1 - s1 + 1))).astype(np.float32),
                                     theta=(0.25 * rng.standard_normal((nb, e1 - s1 + 1))).astype(np.float32)))
    p["layers"] = True
    okw = sr.OPT_KW["adam"]
    o = ctx.make_opts(update_col_layers=True)
    params = [("logdelta", 0), ("theta", 0), ("logdelta", 1), ("theta", 1)]
    before, after, _, _ = one_step(ctx, p, o, params, okw)
    assert after["theta", 0]["acc"].shape == (3, 20) and after["logdelta", 1]["mom"].shape == (5, 20)
    check_step(p, before, after, okw, 1)
    # view 1's state is its own: not view 0's, not a shifted window of the flat array
    g = before["theta", 1]["g"].astype(np.float64)
    np.testing.assert_allclose(after["theta", 1]["mom"], 0.1 * g, rtol=1e-6, atol=1e-30)


@pytest.mark.parametrize("opt", OPTS)
def test_a_parameter_that_is_not_updated_keeps_value_and_state(ctx, opt):
    p = _xy_problem(85)
    okw = sr.OPT_KW[opt]
    one_step(ctx, p, _case_opts(ctx, p), XY, okw)                  # a state that is not the starting one
    for stepped, kept in (("X", "Y"), ("Y", "X")):
        o = ctx.make_opts(update_X=stepped == "X", update_Y=stepped == "Y")
        held = _read(ctx, [(kept, 0)], grad=False)[kept, 0]
        before, after, _, _ = one_step(ctx, p, o, [(stepped, 0)], fresh=False)
        now = _read(ctx, [(kept, 0)], grad=False)[kept, 0]
        for f in ("p", "acc", "mom"):
            np.testing.assert_array_equal(now[f], held[f], err_msg=f"{kept}.{f}")
        check_step(p, before, after, okw, 2)                        # the second step of either: t is kept per parameter


# ---- the stopping rule ------------------------------------------------------------------------------------------------------
def test_stopping_rule_on_the_device(pkg, ctx):
    p = make_problem(M=200, N=120, K=8, seed=91, xreg="l2", yreg="l2", random_init=True, nan_frac=0.05)
    flags = dict(update_X=True, update_Y=True)

    def fit(**kw):
        to_context(p, ctx)
        ctx.set_optimizer("adagrad", lr=0.05)
        return ctx.fit(**flags, **kw)

    full = fit(max_epochs=60, abs_tol=0, rel_tol=0)
    tr = full["loss"]
    assert len(tr) == full["epochs"] >= 30 and sr.stop_rule(tr, 0, 0, 3) == (full["term_code"], full["epochs"])
    np.testing.assert_array_equal(fit(max_epochs=60, abs_tol=0, rel_tol=0)["loss"], tr)       # run to run: bitwise
    d = tr[:-1] - tr[1:]
    for name, series in (("abs_tol", d), ("rel_tol", d / tr[1:])):
        # each series has its own descent: d falling from one epoch to the next does not make d / loss fall there too
        j = next(i for i in range(10, len(series)) if series[i - 1] > series[i] > 0)
        tol = 0.5 * (series[j - 1] + series[j])                  # between two consecutive observed differences
        assert series[j - 1] > tol > series[j], (name, j, series[j - 1], tol, series[j])
        print(f"stopping rule {name}: j={j} tol={tol:.6g}")
        tols = dict(abs_tol=tol, rel_tol=0.0) if name == "abs_tol" else dict(abs_tol=0.0, rel_tol=tol)
        for tmi in (1, 2, 3, 5):
            want = sr.stop_rule(tr, tols["abs_tol"], tols["rel_tol"], tmi)
            assert want[0] == name and want[1] < len(tr), (name, tmi, want)
            r = fit(max_epochs=60, tol_max_iters=tmi, **tols)
            assert (r["term_code"], r["epochs"]) == want, (name, tmi, r["term_code"], r["epochs"], want)
            assert (r["term_code"], r["epochs"]) == sr.stop_rule(r["loss"], tols["abs_tol"], tols["rel_tol"], tmi)
            np.testing.assert_array_equal(r["loss"], tr[:r["epochs"]])
            assert r["final_loss"] == tr[r["epochs"] - 1]
    # no epoch to run: returns cleanly with an empty trace
    r = fit(epoch=5, max_epochs=4, abs_tol=0, rel_tol=0)
    assert r["term_code"] == "max_epochs" and r["epochs"] == 4 and len(r["loss"]) == 0
    X, Y = ctx.get_factors()
    np.testing.assert_array_equal(X, p["X"])
    np.testing.assert_array_equal(Y, p["Y"])
    # a trace buffer shorter than the epochs run
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=0.05)
    o = ctx.make_opts(max_epochs=10, abs_tol=0, rel_tol=0, **flags)
    buf = np.full(6, -1.0)
    res = pkg._lib.FitResult()
    res.trace_cap = 3
    res.loss_trace = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert ctx.lib.pmf_fit(ctx._h, C.byref(o), C.byref(res)) == 0
    assert (res.n_trace, res.epochs, pkg._lib.TERM[res.term_code]) == (3, 10, "max_epochs")
    np.testing.assert_array_equal(buf, np.concatenate([tr[:3], [-1.0, -1.0, -1.0]]))
    assert res.final_loss == tr[9]
