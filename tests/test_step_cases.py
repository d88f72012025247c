"""Host-side guards of tests/step_ref.py (no GPU): the float64 restatement of the regularizer terms and of the optimizer
step reproduces the fp64 C oracle on every case of the tables (value, total gradient, parameters after 1 and 3 epochs,
both optimizers); terms the oracle does not have (L1, a ColParamReg whose ranges overlap) are held to literals written
out element by element; stop_rule reproduces the oracle's termination; and the tolerance constants cover the float32
twin's worst deviation from the float64 restatement with their margin."""
import copy

import numpy as np
import pytest

import step_ref as sr
from problems import make_problem, to_oracle

FLAGS = dict(update_X=True, update_Y=True)


def _flags(p):
    return dict(FLAGS, update_col_layers=p["layers"])


def _grad_of(g, which, view):
    return g[which][view] if which in ("logdelta", "theta") else g[which]


def _oracle_param(m, which, view):
    return getattr(m, which)[view] if which in ("logdelta", "theta") else getattr(m, which)


def _oracle_part(p):
    """The problem with only what the C oracle implements the library's way, and what was taken out."""
    q = copy.copy(p)
    q["xreg"] = [t for t in p["xreg"] if t["kind"] != "l1"]
    q["yreg"] = [t for t in p["yreg"] if t["kind"] != "l1"]
    if not p["oracle_ok"] and p["colreg"] is not None:
        q["colreg"] = None
    return q


def _literal(p, which, pv):
    """Value and gradient of the terms _oracle_part removed, element by element."""
    val, g = 0.0, np.zeros(np.shape(pv))
    if which in ("X", "Y"):
        for t in (p["xreg"] if which == "X" else p["yreg"]):
            if t["kind"] != "l1":
                continue
            K, n = pv.shape
            for j in range(n):
                for k in range(K):
                    if t["mask"] is None or t["mask"][k, j]:
                        w = float(np.float32(t["p"])) * float(t["w"][k])
                        x = float(pv[k, j])
                        val += w * abs(x)
                        g[k, j] += w if x > 0 else -w if x < 0 else 0.0
    elif which in ("logsigma", "mu") and not p["oracle_ok"] and p["colreg"] is not None:
        cr = p["colreg"]
        for j in range(pv.shape[0]):
            w = c = 0.0
            for r in range(len(cr["start1"])):
                if cr["start1"][r] <= j + 1 <= cr["stop1"][r]:
                    w, c = float(cr["w_" + which][r]), float(cr["c_" + which][r])
            d = float(pv[j]) - c
            val += 0.5 * w * d * d
            g[j] += w * d
    return val, g


@pytest.mark.parametrize("table,name", sr.ALL_CASES)
def test_value_and_gradient_match_the_oracle(table, name):
    p = sr.build_case(table, name)
    q = _oracle_part(p)
    lo, go = to_oracle(q).loss_and_grads(**_flags(p))
    _, g0 = to_oracle(sr.without_regs(q)).loss_and_grads(**_flags(p))
    l0 = go["data_loss"]
    value = vmag = extra = 0.0
    for which, view in sr.case_params(p):
        pv = sr.param_value(p, which, view)
        r = sr.reg_value_and_grad(pv, sr.param_terms(p, which, view), _grad_of(g0, which, view))
        lv, lg = _literal(p, which, np.asarray(pv, np.float64))
        want = _grad_of(go, which, view) + lg
        assert r["grad"].shape == want.shape
        assert np.all(np.abs(r["grad"] - want) <= 1e-12 * (r["mag"] + 1e-300)), (which, view)
        value, vmag, extra = value + r["value"], vmag + r["vmag"], extra + lv
    assert abs(value - (lo - l0 + extra)) <= 1e-12 * max(vmag, abs(lo)), (value, lo - l0 + extra)
    if not p["oracle_ok"]:
        assert extra != 0.0                       # the literal really carries a term


def _restated_fit(p, opt, epochs):
    """`epochs` epochs of the float64 restatement: the oracle supplies the data gradient only."""
    okw = sr.OPT_KW[opt]
    md = to_oracle(sr.without_regs(p))
    cur = {(w, v): np.array(sr.param_value(p, w, v), np.float64) for w, v in sr.case_params(p)}
    st = {k: sr.fresh_state(a.shape, opt, okw["eps"], np.float64) for k, a in cur.items()}
    for t in range(1, epochs + 1):
        for (w, v), a in cur.items():
            _oracle_param(md, w, v)[...] = a
        _, g = md.loss_and_grads(**_flags(p))
        for (w, v), a in cur.items():
            r = sr.expected_step(p, w, a, _grad_of(g, w, v), st[w, v][0], st[w, v][1], okw, t, v)
            cur[w, v], st[w, v] = r["p"], (r["acc"], r["mom"])
    return cur


ORACLE_CASES = [(t, n) for t, n in sr.ALL_CASES if sr.TABLES[t][n].get("oracle", True)]


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("table,name", ORACLE_CASES)
def test_restated_epochs_match_the_oracle_fit(table, name, opt):
    p = sr.build_case(table, name)
    okw = sr.OPT_KW[opt]
    for epochs in (1, 3):
        m = to_oracle(p)
        m.fit(opt=opt, lr=sr.f32r(okw["lr"]), eps=sr.f32r(okw["eps"]), beta1=sr.f32r(okw["beta1"]), beta2=sr.f32r(okw["beta2"]),
              max_epochs=epochs, abs_tol=0, rel_tol=0, **_flags(p))
        cur = _restated_fit(p, opt, epochs)
        for (w, v), a in cur.items():
            want = _oracle_param(m, w, v)
            assert np.max(np.abs(a - want)) <= 1e-12 * np.max(np.abs(want)), (epochs, w, v)


# ---- the termination rule -----------------------------------------------------------------------------------------------
KAT = dict(M=40, N=30, K=4, seed=7, xreg="l2", yreg="group", random_init=True)   # tests/test_oracle_kat.py::test_fit_loop_semantics


@pytest.mark.parametrize("kw", [
    dict(lr=0.05, max_epochs=30, abs_tol=0, rel_tol=0, tol_max_iters=3),
    dict(lr=50.0, max_epochs=50, abs_tol=0, rel_tol=0, tol_max_iters=3),
    dict(lr=0.05, max_epochs=2000, abs_tol=0.5, rel_tol=1e-12, tol_max_iters=3),
    dict(lr=0.05, max_epochs=2000, abs_tol=0.5, rel_tol=1e-12, tol_max_iters=1),
    dict(lr=0.05, max_epochs=2000, abs_tol=0.5, rel_tol=1e-12, tol_max_iters=5),
    dict(lr=0.05, max_epochs=2000, abs_tol=1e-12, rel_tol=1e-3, tol_max_iters=2),
    dict(lr=0.05, max_epochs=2000, abs_tol=0.05, rel_tol=1e-3, tol_max_iters=4),
])
def test_stop_rule_reproduces_the_oracle(kw):
    p = make_problem(**KAT)
    r = to_oracle(p).fit(update_X=True, update_Y=True, **kw)
    # the rule on the oracle's own trace (its sums are not bitwise reproducible run to run): it must stop at the last
    # entry with the oracle's code, neither earlier nor -- "max_epochs" short of max_epochs -- later
    assert len(r["loss"]) == r["epochs"]
    got = sr.stop_rule(r["loss"], kw["abs_tol"], kw["rel_tol"], kw["tol_max_iters"])
    assert got == (r["term_code"], r["epochs"]), (got, r["term_code"], r["epochs"])
    if kw["abs_tol"] or kw["rel_tol"]:
        assert r["term_code"] in ("abs_tol", "rel_tol") and r["epochs"] < kw["max_epochs"]


def test_stop_rule_on_hand_made_traces():
    # rises on the last allowed epoch
    assert sr.stop_rule([10.0, 9.0, 8.0, 8.5], 0, 0, 3) == ("loss_increase", 4)
    assert sr.stop_rule([10.0, 9.0, 8.0], 0, 0, 3) == ("max_epochs", 3)
    # abs_tol met on non-consecutive epochs: the counter resets (d = .05, .05, 1, .05, .05, .05)
    tr = [10.0, 9.95, 9.9, 8.9, 8.85, 8.8, 8.75, 8.7]
    assert sr.stop_rule(tr, 0.1, 0, 3) == ("abs_tol", 7)
    assert sr.stop_rule(tr, 0.1, 0, 2) == ("abs_tol", 3)
    assert sr.stop_rule(tr[:6], 0.1, 0, 3) == ("max_epochs", 6)
    # both tolerances met: abs wins; the code is that of the epoch that fills the counter
    assert sr.stop_rule([10.0, 9.99, 9.98, 9.97], 0.1, 0.1, 3) == ("abs_tol", 4)
    assert sr.stop_rule([10.0, 9.5, 9.0, 8.99], 0.1, 0.1, 3) == ("abs_tol", 4)      # rel, rel, then abs
    assert sr.stop_rule([10.0, 9.99, 9.98, 9.5], 0.1, 0.1, 3) == ("rel_tol", 4)
    # an infinity, a NaN; the first epoch is never compared
    assert sr.stop_rule([10.0, 9.0, np.inf, 8.0], 0, 0, 3) == ("nonfinite", 3)
    assert sr.stop_rule([np.nan], 0, 0, 3) == ("nonfinite", 1)
    assert sr.stop_rule([10.0], 1e9, 1e9, 1) == ("max_epochs", 1)
    assert sr.stop_rule([], 0, 0, 3) == ("max_epochs", 0)
    # zero tolerances never count, even on a flat trace
    assert sr.stop_rule([5.0, 5.0, 5.0, 5.0], 0, 0, 1) == ("max_epochs", 4)


# ---- the float32 twin sets the tolerances -------------------------------------------------------------------------------
def twin_deviations(p, opt, steps=5):
    """Worst scaled deviations of the float32 twin from the float64 restatement on the same float32 inputs, over `steps`
    consecutive steps of every parameter of the case (the data gradient: the oracle's, rounded to float32; each step
    starts from the twin's own float32 result, as the device's would).  p1: the parameter at the first step alone."""
    okw = sr.OPT_KW[opt]
    md = to_oracle(sr.without_regs(p))
    cur = {(w, v): np.array(sr.param_value(p, w, v), np.float32) for w, v in sr.case_params(p)}
    st = {k: sr.fresh_state(a.shape, opt, okw["eps"]) for k, a in cur.items()}
    worst = dict(p1=0.0, p=0.0, acc=0.0, mom=0.0, val=0.0)
    for t in range(1, steps + 1):
        for (w, v), a in cur.items():
            _oracle_param(md, w, v)[...] = a
        _, g = md.loss_and_grads(**_flags(p))
        val64 = val32 = vmag = 0.0
        for (w, v), a in cur.items():
            gd = np.asarray(_grad_of(g, w, v), np.float32)
            acc, mom = st[w, v]
            r64 = sr.expected_step(p, w, a, gd, acc, mom, okw, t, v)
            r32 = sr.expected_step(p, w, a, gd, acc, mom, okw, t, v, twin=True)
            dp = sr.dev_param(r32["p"], r64["p"], a, r64["sens"], r64["mag"])
            worst["p1" if t == 1 else "p"] = max(worst["p1" if t == 1 else "p"], dp)
            worst["acc"] = max(worst["acc"], sr.dev_acc(r32["acc"], r64["acc"], acc, r64["mag"]))
            worst["mom"] = max(worst["mom"], sr.dev_mom(r32["mom"], r64["mom"], mom, r64["mag"]))
            if r64["vmag"] > 0:
                worst["val"] = max(worst["val"], sr.dev_value(r32["value"], r64["value"], r64["vmag"]))
            val64, val32, vmag = val64 + r64["value"], val32 + r32["value"], vmag + r64["vmag"]
            cur[w, v], st[w, v] = r32["p"], (r32["acc"], r32["mom"])
        if vmag > 0:
            worst["val"] = max(worst["val"], sr.dev_value(val32, val64, vmag))
    return worst


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("table,name", sr.ALL_CASES)
def test_tolerance_constants_cover_the_f32_twin(table, name, opt):
    w = twin_deviations(sr.build_case(table, name), opt)
    assert sr.TWIN_MARGIN * w["p1"] <= sr.p_tol(opt, 1), w
    assert sr.TWIN_MARGIN * w["p"] <= sr.p_tol(opt, 2), w
    assert sr.TWIN_MARGIN * w["acc"] <= sr.ACC_TOL, w
    assert sr.TWIN_MARGIN * w["mom"] <= sr.MOM_TOL, w
    assert sr.TWIN_MARGIN * w["val"] <= sr.VAL_TOL, w
    assert w["p1"] > 0 and w["p"] > 0 and w["acc"] > 0          # the twin really runs in float32


def test_bare_parameter_scale_does_not_bound_the_twin():
    """Why dev_param carries the |d(dp)/dg| mag term: per |p| + |dp| alone, the float32 twin's own first AdaGrad step is off
    by far more than a few roundings where the gradient terms cancel (dp = lr g / (sqrt(eps + g^2) + eps) amplifies the
    rounding of the summed gradient by up to lr / sqrt(eps))."""
    p = sr.build_case("LAYER_SIZE_EDGES", "theta_8193")
    okw = sr.OPT_KW["adagrad"]
    _, g = to_oracle(sr.without_regs(p)).loss_and_grads(**_flags(p))
    bare = full = 0.0
    for w, v in sr.case_params(p):
        a = np.asarray(sr.param_value(p, w, v), np.float32)
        acc, mom = sr.fresh_state(a.shape, "adagrad", okw["eps"])
        gd = np.asarray(_grad_of(g, w, v), np.float32)
        r64 = sr.expected_step(p, w, a, gd, acc, mom, okw, 1, v)
        r32 = sr.expected_step(p, w, a, gd, acc, mom, okw, 1, v, twin=True)
        bare = max(bare, sr.dev_param(r32["p"], r64["p"], a))
        full = max(full, sr.dev_param(r32["p"], r64["p"], a, r64["sens"], r64["mag"]))
    assert bare > 1e-5 and sr.TWIN_MARGIN * full <= sr.p_tol("adagrad", 1), (bare, full)


def test_case_tables_hold_what_they_name():
    assert sorted(int(n[1:]) for n in sr.K_EDGES) == [1, 31, 32, 33, 64, 65, 100, 128]
    for name, spec in sr.SIZE_EDGES.items():       # padded element count around REG_SLOTS * 256
        pr = spec["problem"]
        Kp = -(-pr["K"] // 32) * 32
        n = pr["M"] if name.startswith("X") else pr["N"]
        assert abs(Kp * n - sr.REG_SLOTS * 256) <= Kp and 32 <= min(pr["M"], pr["N"]) <= 64
    sizes = sorted(Kp_n - sr.REG_SLOTS * 256 for Kp_n in
                   {32 * (s["problem"]["M"] if k.startswith("X") else s["problem"]["N"]) for k, s in sr.SIZE_EDGES.items()})
    assert sizes[0] < 0 and 0 in sizes and sizes[-1] > 0
    for name, spec in sr.LAYER_SIZE_EDGES.items():
        n = spec["problem"]["N"] * (spec["views"][0][2] if name.startswith("theta") else 1)
        assert abs(n - (sr.REG_SLOTS // 4) * 256) <= 8
    p = sr.build_case("RANGE_EDGES", "batches_1_and_255")
    assert [np.asarray(b["theta"]).shape[0] for b in p["batch_views"]] == [1, 255]
    assert all(len(np.unique(b["batch_of_row"])) == np.asarray(b["theta"]).shape[0] for b in p["batch_views"])
    wq = sr.quad_weights(sr.build_case("RANGE_EDGES", "x_overlap_gaps")["xreg"], 24, 40)
    assert not wq[:, :2].any() and not wq[:, 30:].any() and wq[:, 2:30].all()
    assert np.all(wq[:, 14:20] > np.maximum(wq[:, 2:3], wq[:, 29:30]))      # the overlap adds
    assert sr.chunk_column_edges(200, 3) == [0, 64, 128, 200] and sr.chunk_column_edges(200, 5) == [0, 32, 64, 128, 160, 200]
