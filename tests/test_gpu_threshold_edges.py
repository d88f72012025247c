"""The threshold pass (include/pmf_hip_thresholds.h) where tests/test_gpu_thresholds.py does not take
it: units that sweep several row panels (PMF_THRESH_RANGES caps the row ranges), a tile list with skipped tiles, full triples
and the two-step clamp, batch tables of 32 and 256 slots (the WIDE instances), kind-3 columns outside every view, groups of
more than 256 columns and more than 64 groups, column layers training next to the thresholds, the pass's two refusals.

The problems are those of tests/threshold_edge_problems.py; tests/test_threshold_edge_cases.py holds the conditions that make
the comparison mean something.  Tolerances: LAYER_TAU times the scales of threshold_ref for a gradient, step_ref's one-step
bounds for an epoch, bitwise equality where the library promises it; none is new."""
import numpy as np
import pytest

import hinge_ref as hr
import step_ref as sr
import threshold_edge_problems as ep
import threshold_ref as tr
from problems import LAYER_TAU
from test_gpu_split_bf16 import bf16_round
from test_gpu_thresholds import FLAT, check_grad, worst
from test_threshold_cases import OPT, big

pytestmark = pytest.mark.gpu

LONG = {"A-k48": lambda: big("A", 48), "B-k128": lambda: big("B", 128), "Cwide-k48-m600": lambda: ep.layout_c(48, 600, "wide"),
        "Cwide-k128-m600": lambda: ep.layout_c(128, 600, "wide"), "Cnarrow-k80-m512": lambda: ep.layout_c(80, 512, "narrow")}


def geometry(ctx, p, R=None):
    """The pass's geometry after a pass at R row ranges: the tiles are the problem's, the units tiles x R."""
    d = ctx.debug_threshold_pass()
    assert d["n_tiles"] == len(ep.tiles_of(p)), d
    if R is not None:
        assert d["n_units"] == d["n_tiles"] * R, (d, R)
    return d


def one_step(p, prev, got, kw, t, G=None):
    """The state `got` after one threshold step from the state `prev` (device values) at the parameters of problem p and the
    triples prev["thr"]: thr, acc and mom against threshold_ref.threshold_step within step_ref's one-step bounds, given the
    gradient bound of the pass.  G: the gradients stepped from (default: the reference's)."""
    opt = kw["kind"]
    t0, acc0, mom0 = (np.asarray(prev[k], np.float64) for k in ("thr", "acc", "mom"))
    p_at = tr.with_thresholds(p, t0)
    G = tr.group_grad(p_at) if G is None else np.asarray(G, np.float64)
    dG = LAYER_TAU * tr.group_scale(p_at)
    fin = np.isfinite(t0)
    raw, t1, acc1, mom1 = tr.threshold_step(t0, G, acc0, mom0, kw, t)
    assert np.array_equal(raw, t1, equal_nan=True), "the reference step crosses: compare the clamp elsewhere"
    sens = sr.step_sensitivity(np.where(fin, G, 0.0), acc0, mom0, kw, t)
    lim_p = sr.p_tol(opt, t) * (np.abs(np.where(fin, t0, 0.0)) + np.abs(np.where(fin, t1 - np.where(fin, t0, 0.0), 0.0))) + sens * dG
    assert (np.abs(got["thr"][fin] - t1[fin]) <= lim_p[fin]).all(), (got["thr"], t1, lim_p)
    b2 = 1.0 if opt == "adagrad" else 1.0 - kw["beta2"]
    lim_a = sr.ACC_TOL * (G * G + np.abs(acc0)) + b2 * (2 * np.abs(G) + dG) * dG
    assert (np.abs(got["acc"] - acc1)[fin] <= lim_a[fin]).all(), (got["acc"], acc1)
    lim_m = sr.MOM_TOL * (np.abs(G) + np.abs(mom0)) + (1.0 - kw["beta1"]) * dG
    assert (np.abs(got["mom"] - mom1)[fin] <= lim_m[fin]).all(), (got["mom"], mom1)
    for k in ("thr", "acc", "mom"):                        # infinite thresholds and their state stay, bit for bit
        assert np.array_equal(got[k][~fin], prev[k][~fin]), k
    assert (got["thr"][fin] != prev["thr"][fin]).all()


def set_opt(c, kw):
    c.set_optimizer(kw["kind"], lr=kw["lr"], eps=kw["eps"], beta1=kw["beta1"], beta2=kw["beta2"])


# ---- 1. units that sweep several row panels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LONG))
def test_long_sweeps_match_the_reference(ctx, monkeypatch, name):
    p = LONG[name]()
    hr.to_context(p, ctx)
    n_rp = ep.panels(p["M"], p["K"])
    n0 = ctx.debug_threshold_pass()["passes"]
    out = {}
    for R in (None, 1, 2):
        if R is None:
            monkeypatch.delenv("PMF_THRESH_RANGES", raising=False)
        else:
            assert n_rp > R                                 # some unit sweeps two panels or more
            monkeypatch.setenv("PMF_THRESH_RANGES", str(R))
        out[R] = check_grad(ctx, p, f"long-{name}-R{R or 'free'}")
        d = geometry(ctx, p, R)
        assert d["n_units"] <= d["n_tiles"] * n_rp
    assert ctx.debug_threshold_pass()["passes"] == n0 + 6
    # different float32 sums of the same terms: within one tolerance of each other, per column and per group
    tg, tc = LAYER_TAU * tr.group_scale(p), LAYER_TAU * tr.col_scale(p)
    k3 = hr.kinds_of(p) == 3
    for a, b in ((1, 2), (1, None), (2, None)):
        assert (np.abs(out[a][0].astype(np.float64) - out[b][0]) <= tg).all(), (a, b)
        assert (np.abs(out[a][1].astype(np.float64) - out[b][1])[k3] <= tc[k3]).all(), (a, b)


def test_one_workgroup_walks_every_unit_of_a_long_sweep(ctx, monkeypatch):
    p = LONG["Cwide-k48-m600"]()
    hr.to_context(p, ctx)
    monkeypatch.setenv("PMF_THRESH_RANGES", "2")
    monkeypatch.setenv("PMF_THRESH_GRID", "1")
    check_grad(ctx, p, "long-Cwide-k48-m600-R2-grid1")
    d = geometry(ctx, p, 2)
    assert d["grid"] == 1 and d["n_units"] == 8, d


# ---- 2. D stored as bf16 on long sweeps (K = 128: four waves, the prefetch of the next D tile) -----------------------------------
@pytest.mark.parametrize("K", [48, 128])
def test_bf16_stored_data_on_long_sweeps(ctx, monkeypatch, K):
    p = dict(ep.layout_c(K, 600, "wide"))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    hr.to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    monkeypatch.setenv("PMF_THRESH_RANGES", "1")
    try:
        assert ep.panels(600, K) > 1
        check_grad(ctx, p, f"bf16-Cwide-k{K}-m600-R1")
        geometry(ctx, p, 1)
        got = ctx.class_counts(p["noise_ranges"])
    finally:
        ctx.set_data(p["D"])
    assert np.array_equal(got, tr.class_counts(p, p["noise_ranges"]))


# ---- 3. a tile list with skipped tiles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [None, "narrow"], ids=["plain", "narrow"])
@pytest.mark.parametrize("K", hr.KS)
def test_skipped_tiles(ctx, K, variant):
    p = ep.layout_c(K, 70, variant)
    hr.to_context(p, ctx)
    g, gc = check_grad(ctx, p, f"skip-C{variant or 'plain'}-k{K}")           # (the per-column NaN pattern is asserted there)
    assert geometry(ctx, p)["n_tiles"] == 4
    assert np.isnan(gc[:40]).all() and np.isnan(gc[60:100]).all() and np.isnan(gc[130:192]).all() and np.isfinite(gc[192:]).all()


@pytest.mark.parametrize("K", [20, 80])
def test_an_epoch_rebuilds_only_the_groups_columns(pkg, K):
    p = ep.layout_c(K, 70, "narrow")
    c, d = pkg.Context(0), pkg.Context(0)
    try:
        hr.to_context(p, c)
        c.set_optimizer("adagrad", lr=0.05)
        s0 = c.get_threshold_state()
        c.fit(update_noise_models=True, max_epochs=1, **FLAT)               # thresholds alone: X and Y stay
        s1 = c.get_threshold_state()
        one_step(p, s0, s1, OPT["adagrad"], 1)
        hr.to_context(p, d)
        d.set_noise_thresholds(tr.groups_of(p), [tuple(t) for t in s1["thr"]])
        tc, td = c.get_noise_thresholds(), d.get_noise_thresholds()
        assert np.array_equal(tc, td, equal_nan=True)
        assert np.array_equal(np.isnan(tc[:, 0]), hr.kinds_of(p) != 3)
        assert c.loss() == d.loss()
        gc, gd = c.threshold_grad(), d.threshold_grad()
        assert np.array_equal(gc[0], gd[0]) and np.array_equal(gc[1], gd[1], equal_nan=True)
        check_grad(c, tr.with_thresholds(p, s1["thr"]), f"skip-Cnarrow-k{K}-after-an-epoch")
    finally:
        c.close()
        d.close()


# ---- 4. batch tables of 32 and 256 slots ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [20, 80])
def test_wide_batch_tables(ctx, K):
    p = ep.layout_c(K, 70, "wide")
    hr.to_context(p, ctx)
    check_grad(ctx, p, f"wide-C-k{K}")
    geometry(ctx, p)


def test_a_view_of_255_batches(ctx, monkeypatch):
    p = ep.many_batches_255()
    hr.to_context(p, ctx)
    check_grad(ctx, p, "wide-nb255-k128-m600")
    monkeypatch.setenv("PMF_THRESH_RANGES", "1")
    check_grad(ctx, p, "wide-nb255-k128-m600-R1")
    geometry(ctx, p, 1)


# ---- 5. full triples and the two-step clamp -------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_the_clamp_cascades_over_a_full_triple(pkg, opt):
    p, kw = ep.cascade_problem(), ep.CASCADE_OPT[opt]
    _, _, info = tr.joint_epoch(p, tr.fresh_state(p, kw), kw, 1, train_xy=False)
    raw = info["raw"]
    assert raw[0][1] < raw[0][0] and raw[0][2] < raw[0][0] and raw[0][1] < raw[0][2], raw
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        check_grad(c, p, f"cascade-{opt}")
        set_opt(c, kw)
        c.fit(update_noise_models=True, max_epochs=1, **FLAT)               # thresholds alone
        s = c.get_threshold_state()["thr"]
        assert s[0][0] == s[0][1] == s[0][2], s
        assert abs(s[0][0] - raw[0][0]) <= 1e-5 * kw["lr"], (s, raw)
        fin = np.isfinite(raw)
        fin[0] = False
        assert (np.abs(s[fin] - raw[fin]) <= 1e-5 * kw["lr"]).all()          # the other groups: stepped, not clamped
        t = c.get_noise_thresholds()
        k3 = hr.kinds_of(p) == 3
        assert (t[k3, 0] <= t[k3, 1]).all() and (t[k3, 1] <= t[k3, 2]).all() and np.isnan(t[~k3]).all()
        assert (t[40:60] == s[0]).all()
        assert np.isfinite(c.loss()["data"])                                # the rebuilt tables serve the next pass
        q = tr.with_thresholds(p, s)
        check_grad(c, q, f"cascade-{opt}-clamped")
    finally:
        c.close()


# ---- 6. big groups, many groups ----------------------------------------------------------------------------------------------------
def test_groups_of_more_than_256_columns(ctx):
    p = ep.layout_d()
    hr.to_context(p, ctx)
    check_grad(ctx, p, "groups-D")
    assert geometry(ctx, p)["n_tiles"] == 25
    assert np.array_equal(ctx.class_counts(p["noise_ranges"]), tr.class_counts(p, p["noise_ranges"]))


def test_seventy_groups_take_two_adam_epochs(pkg):
    p, kw = ep.layout_e(), OPT["adam"]
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        check_grad(c, p, "groups-E")
        counts = c.class_counts(p["noise_ranges"])
        assert counts.shape == (70, 4) and np.array_equal(counts, tr.class_counts(p, p["noise_ranges"]))
        set_opt(c, kw)
        s0 = c.get_threshold_state()
        assert s0["thr"].shape == (70, 3)
        c.fit(update_noise_models=True, max_epochs=1, **FLAT)
        s1 = c.get_threshold_state()
        one_step(p, s0, s1, kw, 1)
        c.fit(update_noise_models=True, max_epochs=2, epoch=2, **FLAT)
        s2 = c.get_threshold_state()
        one_step(p, s1, s2, kw, 2)
        thr = c.get_noise_thresholds()
        for r, (s, e) in enumerate(tr.groups_of(p)):
            assert (thr[s - 1:e] == s2["thr"][r]).all()
    finally:
        c.close()


# ---- 7. the column layers train next to the thresholds -------------------------------------------------------------------------------
ALL_ON = dict(update_X=True, update_Y=True, update_col_layers=True, update_noise_models=True)


def read_out(c, p):
    """The problem at the parameters of context c."""
    X, Y = c.get_factors()
    ls, mu = c.get_col_params()
    q = dict(p, X=X, Y=Y, logsigma=ls, mu=mu, batch_views=[])
    for v, bv in enumerate(p["batch_views"]):
        ld, th = c.get_batch_view(v)
        q["batch_views"].append(dict(bv, logdelta=np.ascontiguousarray(ld), theta=np.ascontiguousarray(th)))
    return tr.with_thresholds(q, c.get_threshold_state()["thr"])


@pytest.mark.parametrize("K", [20, 80])
def test_layers_train_next_to_the_thresholds(pkg, K):
    p, kw = ep.layout_c(K, 70, "narrow"), OPT["adagrad"]
    c, d = pkg.Context(0), pkg.Context(0)
    try:
        hr.to_context(p, d)
        set_opt(d, kw)
        d.fit(update_noise_models=True, max_epochs=1, **FLAT)               # thresholds alone
        alone = d.get_threshold_state()
        hr.to_context(p, c)
        set_opt(c, kw)
        c.fit(max_epochs=1, **ALL_ON, **FLAT)
        s1 = c.get_threshold_state()
        for k in ("thr", "acc", "mom"):                                        # the same G, the same step
            assert np.array_equal(s1[k], alone[k]), k
        q = read_out(c, p)
        assert not np.array_equal(q["logsigma"], p["logsigma"]) and not np.array_equal(q["mu"], p["mu"])
        for a, b in zip(q["batch_views"], p["batch_views"]):
            assert not np.array_equal(a["theta"], b["theta"]) and not np.array_equal(a["logdelta"], b["logdelta"])
        # a fresh context at the stepped parameters: its pass is the reference's, and the first context's second epoch steps from it
        hr.to_context(q, d)
        G, _ = check_grad(d, q, f"layers-Cnarrow-k{K}-epoch2")
        c.fit(max_epochs=2, epoch=2, **ALL_ON, **FLAT)
        s2 = c.get_threshold_state()
        one_step(q, s1, s2, kw, 2, G=G)
        one_step(q, s1, s2, kw, 2)
    finally:
        c.close()
        d.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(pkg, c, p, match):
    """threshold_grad and a joint fit are refused with `match`; factors, thresholds and their state stay; a fit with training
    off then runs."""
    set_opt(c, OPT["adagrad"])
    X0, Y0 = c.get_factors()
    t0, s0 = c.get_noise_thresholds(), c.get_threshold_state()
    with pytest.raises(pkg.PMFError, match=match):
        c.threshold_grad()
    with pytest.raises(pkg.PMFError, match=match):
        c.fit(update_X=True, update_Y=True, update_noise_models=True, max_epochs=2, **FLAT)
    X1, Y1 = c.get_factors()
    assert np.array_equal(X0, X1) and np.array_equal(Y0, Y1)
    assert np.array_equal(t0, c.get_noise_thresholds(), equal_nan=True)
    s1 = c.get_threshold_state()
    for k in ("thr", "acc", "mom"):
        assert np.array_equal(s0[k], s1[k]), k
    h = c.fit(update_X=True, update_Y=True, max_epochs=2, **FLAT)
    assert np.isfinite(h["loss"]).all() and len(h["loss"]) == 2
    assert np.array_equal(t0, c.get_noise_thresholds(), equal_nan=True)


def test_k_above_128_is_refused(pkg):
    """The library takes no K above 128 at all: pmf_set_factors refuses K = 130, so the pass's own K <= 128 refusal cannot be
    reached through the API, and no fit runs at K = 130 with training on or off.  What can be held: the refusal leaves the
    context (and the binding's K) at the K = 128 model it had, whose pass, thresholds and state are untouched and which trains."""
    p, over = ep.layout_c(128, 70, "narrow"), ep.layout_c(130, 70, "narrow")
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        set_opt(c, OPT["adagrad"])
        t0, s0 = c.get_noise_thresholds(), c.get_threshold_state()
        with pytest.raises(pkg.PMFError, match="K=130 unsupported"):
            c.set_factors(over["X"], over["Y"])
        assert c.K == 128
        X1, Y1 = c.get_factors()
        assert np.array_equal(X1, p["X"]) and np.array_equal(Y1, p["Y"])
        assert np.array_equal(t0, c.get_noise_thresholds(), equal_nan=True)
        s1 = c.get_threshold_state()
        for k in ("thr", "acc", "mom"):
            assert np.array_equal(s0[k], s1[k]), k
        check_grad(c, p, "refusal-k130-leaves-Cnarrow-k128")
        h = c.fit(update_X=True, update_Y=True, update_noise_models=True, max_epochs=2, **FLAT)
        fin = np.isfinite(s0["thr"])
        assert np.isfinite(h["loss"]).all() and (c.get_threshold_state()["thr"][fin] != s0["thr"][fin]).all()
    finally:
        c.close()


def test_a_view_of_256_batches_is_refused_and_the_context_trains_after(pkg):
    base = ep.layout_c(20, 300, "narrow")
    p = ep.with_views(base, (256, 6))
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        _refused(pkg, c, p, "dense batch table")
        c.set_batch_views(base["batch_views"])
        c.set_factors(base["X"], base["Y"])                                 # (the fit with training off moved them)
        check_grad(c, base, "refusal-Cnarrow-k20-m300-back-to-6-batches")
        set_opt(c, OPT["adagrad"])
        s0 = c.get_threshold_state()
        h = c.fit(update_X=True, update_Y=True, update_noise_models=True, max_epochs=2, **FLAT)
        s2 = c.get_threshold_state()
        fin = np.isfinite(s0["thr"])
        assert np.isfinite(h["loss"]).all() and (s2["thr"][fin] != s0["thr"][fin]).all()
    finally:
        c.close()


# ---- 9. nothing is left behind --------------------------------------------------------------------------------------------------------
def test_live_bytes_return(pkg, monkeypatch):
    before = pkg._lib.live_bytes()
    c = pkg.Context(0)
    try:
        for p, R in ((ep.layout_c(20, 70, "wide"), None), (ep.layout_c(48, 600, "wide"), 1), (ep.layout_d(), None)):
            if R:
                monkeypatch.setenv("PMF_THRESH_RANGES", str(R))
            else:
                monkeypatch.delenv("PMF_THRESH_RANGES", raising=False)
            hr.to_context(p, c)
            g, gc = c.threshold_grad()
            assert worst(g, tr.group_grad(p), tr.group_scale(p)) <= 1.0
        assert pkg._lib.live_bytes() != before
    finally:
        c.close()
    assert pkg._lib.live_bytes() == before
