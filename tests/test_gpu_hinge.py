"""The squared-hinge noise models (kind 3: bernoulli_sq_hinge, ordinal_sq_hinge3) on the device, against tests/hinge_ref.py.

Columns of kind 3 reach pmf_noise through the per-column path of every fused family, through the layer pass, k_layer_grad,
k_stats, the impute kernels and the synthetic-data kernel, each with the column's thresholds.  What goes wrong there gives
finite, plausible numbers: a column that reads its neighbour's thresholds, a class read off by one, a tile of kind-3
columns taken for the Poisson tile that code 3 used to mean, a dead column behind a kind-3 range that is not zero.

M = 70 throughout (two full 32-row blocks and a ragged one).  Layout A (N = 173, by name, the reference's sorted order):
bernoulli 1-20, bernoulli_sq_hinge 21-75, normal 76-110, ordinal_sq_hinge3 111-165, poisson 166-173 -- a whole tile of each
new model, a tile of each with a neighbouring kind, a ragged last tile.  Layout B (N = 77, raw kind 3): thresholds
(-inf, -0.5, 0.5) on 1-40, (0, inf, inf) on 41-50, (-inf, -1.2, 0.3) on 51-77 -- three threshold sets inside one tile, dead
columns behind a kind-3 range.  Both carry column weights, logsigma, mu and 10 % NaN, and run plain and with two batch
views whose seam falls inside a kind-3 tile.  tests/test_hinge_cases.py holds the conditions that make the comparison mean
something.  Tolerances: LOSS_RTOL, GRAD_TOL and FIT_TOL of tests/test_gpu_parity.py, LAYER_TAU of tests/problems.py, the
2e-5 of tests/test_gpu_stages.py and the per-entry bound of tests/impute_ref.py; none is new."""
import copy

import numpy as np
import pytest

import batch_cases as bc
import hinge_ref as hr
import step_ref as sr
from impute_ref import BATCH, KEEP, LINK, impute_tol, worst_ratio
from problems import LAYER_TAU, layer_check, rel_err
from test_gpu_batch_edges import one_pass
from test_gpu_parity import FIT_TOL, GRAD_TOL, LOSS_RTOL, factor_gate, grads_of
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

PATH_PARAMS = [pytest.param(path, id=bc.path_id(path)) for path in bc.PATHS]
INF = np.inf


def check_ref(ctx, p, tag, ref, loss, g):
    errs = {}
    for w in ("X", "Y"):
        if w in g:
            assert np.isfinite(g[w]).all(), f"non-finite g{w}"
            errs[w] = rel_err(g[w], ref[w])
    print(f"HINGE {tag} loss_rel={abs(loss - ref['data_loss']) / abs(ref['data_loss']):.3e} " +
          " ".join(f"g{w}={errs[w]:.3e}" if w in errs else f"g{w}=-" for w in ("X", "Y")))
    assert abs(loss - ref["data_loss"]) <= LOSS_RTOL * abs(ref["data_loss"]) + 1e-6, (loss, ref["data_loss"])
    for w, e in errs.items():
        assert e <= GRAD_TOL, (w, e)
    factor_gate(ctx, p, g, ref, scales=hr.scales_of(p))


def data_pass(ctx, p, path):
    """The data pass of `path`, twice: asserts the family that ran and equal bits; returns (loss, grads)."""
    if p["batch_views"]:
        loss, g, exp = one_pass(ctx, p, path)
        assert exp[2] == 1, exp                                       # the panels fit: the LDS table, not the gathers
        return loss, g
    prec, K, gname = path
    flags = bc.GRADS[gname]
    ctx.set_precision(prec)
    try:
        n0 = ctx.get_precision()[1]
        loss, g = grads_of(ctx, p, **flags)
        fam = bc.PATHS[path][0]
        got = (ctx.last_kernel(), ctx.get_precision()[1] - n0)
        assert got == (fam, 1 if fam != 0 else 0), f"(family, split launches) = {got}, expected family {fam}"
        loss2, g2 = grads_of(ctx, p, **flags)
    finally:
        ctx.set_precision("f32")
    assert loss == loss2, (loss, loss2)
    for w in g:
        assert np.array_equal(g[w], g2[w]), f"g{w}: the second pass differs"
    return loss, g


# ---- 1. every fused family, both layouts, plain and with batch views ------------------------------------------------
@pytest.mark.parametrize("batch", [False, True], ids=["plain", "batch"])
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("path", PATH_PARAMS)
def test_every_fused_family_matches_the_reference(ctx, path, name, batch):
    p = hr.layout(name, path[1], batch)
    hr.to_context(p, ctx)
    loss, g = data_pass(ctx, p, path)
    check_ref(ctx, p, f"{name}-{'batch' if batch else 'plain'}-{bc.path_id(path)}", hr.reference_of(p), loss, g)


@pytest.mark.parametrize("path", PATH_PARAMS)
def test_layout_a_with_bf16_stored_data(ctx, path):
    """D stored as bf16 (the classes are exact in bf16); the reference takes the bf16-rounded matrix."""
    p = dict(hr.layout("A", path[1], True))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    hr.to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        loss, g = data_pass(ctx, p, path)
        check_ref(ctx, p, f"A-batch-bf16-{bc.path_id(path)}", hr.reference(p), loss, g)
    finally:
        ctx.set_data(p["D"])            # back to f32 storage for the tests that follow


# ---- 2. the layer pass ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("K,old", [(20, False), (48, False), (80, False), (128, False), (20, True), (80, True)])
def test_layer_gradients_match_the_reference(ctx, monkeypatch, K, old, name):
    """All four layer gradients on the batch variant, through pmf_layer_kernel and (PMF_LAYER_OLD=1) through k_layer_grad."""
    if old:
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    p = hr.layout(name, K, True)
    hr.to_context(p, ctx)
    loss, g = grads_of(ctx, p, update_col_layers=True)
    assert ctx.last_path()["layer_path"] == (2 if old else 1), ctx.last_path()
    ref = hr.reference_of(p)
    worst = layer_check(p, g, ref, tau=LAYER_TAU, scales=hr.layer_scales(p))
    print(f"HINGE layers-{name}-k{K}-{'old' if old else 'mfma'} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert abs(loss - ref["data_loss"]) <= LOSS_RTOL * abs(ref["data_loss"]) + 1e-6, (loss, ref["data_loss"])
    assert max(worst.values()) <= 1.0, worst


# ---- 3. pmf_stats -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_factors", [False, True])
@pytest.mark.parametrize("name,K", [("A", 20), ("B", 80)])
def test_statistics_match_the_reference(ctx, name, K, use_factors):
    p = hr.layout(name, K, True)
    hr.to_context(p, ctx)
    st, so = ctx.stats(use_factors), hr.stats(p, use_factors)
    assert np.array_equal(st["n"], so["n"])
    for k in ("sum", "sumsq", "sqerr", "ssq_grad"):
        assert np.isfinite(st[k]).all(), k
        assert rel_err(st[k], so[k]) <= 2e-5, (k, rel_err(st[k], so[k]))
    h = hr.kinds_of(p) == 3
    for k in ("sqerr", "ssq_grad"):                                   # ... and on the kind-3 columns alone
        assert rel_err(st[k][h], so[k][h]) <= 2e-5, (k, rel_err(st[k][h], so[k][h]))
    for v in range(len(p["batch_views"])):
        assert np.array_equal(st["batch_count"][v], so["batch_count"][v])
        assert rel_err(st["batch_sqerr"][v], so["batch_sqerr"][v]) <= 2e-5


# ---- 4. impute --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [False, True], ids=["nobatch", "batch"])
@pytest.mark.parametrize("name,K", [("A", 20), ("A", 80), ("B", 48), ("B", 128)])
def test_impute_returns_the_class_of_z(ctx, name, K, batch):
    p = hr.layout(name, K, True)
    hr.to_context(p, ctx)
    flags = BATCH if batch else 0
    want, z = hr.impute(p, batch=batch)
    h = hr.kinds_of(p) == 3
    sure = (hr.threshold_gap(p, z) >= 1e-3) & h[None, :]
    left_out = int(h.sum() * p["M"] - sure.sum())
    assert left_out <= 0.01 * h.sum() * p["M"], left_out
    got = ctx.impute(flags)
    assert np.array_equal(got[sure], want[sure].astype(np.float32)), int(np.count_nonzero(got[sure] != want[sure]))
    legal = [{0.0, 1.0} if np.isposinf(t[1]) else {1.0, 2.0, 3.0} for t in hr.thresholds_of(p)[h]]
    for col, ok in zip(got[:, h].T, legal):
        assert set(np.unique(col)) <= ok
    rng = np.random.default_rng(K)
    rows, cols = rng.integers(1, p["M"] + 1, 500), rng.integers(1, p["N"] + 1, 500)
    ent = ctx.impute_entries(rows, cols, flags)
    s = sure[rows - 1, cols - 1]
    assert s.sum() > 100 and np.array_equal(ent[s], want[rows - 1, cols - 1][s].astype(np.float32))
    # link space: z itself for every column, at the impute suite's per-entry bound
    tol = impute_tol(p, flags | LINK, z)
    r = max(worst_ratio(ctx.impute(flags | LINK), z, tol),
            worst_ratio(ctx.impute_entries(rows, cols, flags | LINK), z[rows - 1, cols - 1], tol[rows - 1, cols - 1]))
    print(f"HINGE impute-{name}-k{K}-{'batch' if batch else 'nobatch'} left_out={left_out} link_ratio={r:.3f}")
    assert r <= 1.0, r


# ---- 5. thresholds on a live context -----------------------------------------------------------------------------------
def test_set_noise_thresholds_on_a_live_context(ctx, pkg):
    p = hr.layout("B", 20)
    hr.to_context(p, ctx)
    assert np.array_equal(ctx.get_noise_thresholds(), hr.thresholds_of(p).astype(np.float32), equal_nan=True)
    loss1, g1 = grads_of(ctx, p, **bc.BOTH)
    check_ref(ctx, p, "live-before", hr.reference_of(p), loss1, g1)
    q = copy.copy(p)
    q["noise_thr"] = [p["noise_thr"][0], (0.3, INF, INF), (-INF, -0.2, 0.9)]
    ctx.set_noise_thresholds(p["noise_ranges"][1:], q["noise_thr"][1:])
    loss2, g2 = grads_of(ctx, p, **bc.BOTH)
    assert loss2 != loss1 and not np.array_equal(g2["Y"], g1["Y"])
    check_ref(ctx, q, "live-after", hr.reference(q), loss2, g2)
    assert np.array_equal(ctx.get_noise_thresholds(), hr.thresholds_of(q).astype(np.float32), equal_nan=True)
    with pytest.raises(pkg.PMFError, match="t0 <= t1 <= t2"):
        ctx.set_noise_thresholds([(41, 50)], [(1.0, 0.5, INF)])
    with pytest.raises(pkg.PMFError, match="t0 <= t1 <= t2"):
        ctx.set_noise_thresholds([(1, 40), (41, 50)], [(-INF, 0.0, 1.0), (np.nan, 0.5, INF)])   # (nothing of a bad call is applied)
    with pytest.raises(pkg.PMFError, match="bad columns"):
        ctx.set_noise_thresholds([(41, 78)], [(0.0, INF, INF)])
    loss3, g3 = grads_of(ctx, p, **bc.BOTH)
    assert loss3 == loss2 and np.array_equal(g3["X"], g2["X"]) and np.array_equal(g3["Y"], g2["Y"])
    # a range that holds columns of another kind
    a = hr.layout("A", 20)
    hr.to_context(a, ctx)
    la, ga = grads_of(ctx, a, **bc.BOTH)
    with pytest.raises(pkg.PMFError, match="not sq_hinge"):
        ctx.set_noise_thresholds([(15, 30)], [(0.0, INF, INF)])
    with pytest.raises(pkg.PMFError, match="not sq_hinge"):
        ctx.set_noise_thresholds([(21, 75), (76, 80)], [(0.5, INF, INF), (0.0, INF, INF)])
    lb, gb = grads_of(ctx, a, **bc.BOTH)
    assert la == lb and np.array_equal(ga["X"], gb["X"]) and np.array_equal(ga["Y"], gb["Y"])
    assert np.array_equal(ctx.get_noise_thresholds(), hr.thresholds_of(a).astype(np.float32), equal_nan=True)


# ---- 6. a trajectory ----------------------------------------------------------------------------------------------------
def test_six_adagrad_epochs_follow_the_reference(ctx):
    p = copy.copy(hr.layout("A", 20))
    p["X"] = np.asfortranarray(0.5 * p["X"][:, ::-1])      # away from the factors the data were drawn from: the loss falls
    lr, eps, epochs = 0.05, 1e-8, 6
    hr.to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=lr, eps=eps)
    r = ctx.fit(update_X=True, update_Y=True, max_epochs=epochs, abs_tol=0, rel_tol=0)
    assert ctx.last_kernel() == 0 and r["term_code"] == "max_epochs" and len(r["loss"]) == epochs, r
    X, Y = ctx.get_factors()
    q = copy.copy(p)
    state = {w: (np.asarray(p[w], np.float64),) + sr.fresh_state(p[w].shape, "adagrad", eps, np.float64) for w in ("X", "Y")}
    losses = []
    for t in range(1, epochs + 1):
        q["X"], q["Y"] = state["X"][0], state["Y"][0]
        ref = hr.reference(q)
        losses.append(ref["data_loss"])
        state = {w: sr.step(state[w][0], ref[w], state[w][1], state[w][2], "adagrad", lr, eps, 0.9, 0.999, t) for w in ("X", "Y")}
    ex, ey = rel_err(X, state["X"][0]), rel_err(Y, state["Y"][0])
    print(f"HINGE trajectory X={ex:.3e} Y={ey:.3e} loss {losses[0]:.6g} -> {losses[-1]:.6g} device {r['loss'][0]:.6g} -> {r['loss'][-1]:.6g}")
    assert losses[-1] < losses[0]
    assert ex <= FIT_TOL and ey <= FIT_TOL, (ex, ey)


# ---- 7. L-BFGS ----------------------------------------------------------------------------------------------------------
def test_lbfgs_loss_trace_follows_the_reference(ctx):
    """Three iterations on layout B (no regularizer: the loss is the data loss); the n-th entry of the trace is the loss at
    the factors a run of n iterations leaves behind."""
    p = hr.layout("B", 20)
    q = copy.copy(p)
    traces = []
    for n in (1, 2, 3):
        hr.to_context(p, ctx)
        r = ctx.fit_lbfgs(m=5, max_iter=n, rel_tol=0.0, abs_tol=0.0)
        assert r["iters"] == n and len(r["loss"]) == n, r
        q["X"], q["Y"] = ctx.get_factors()
        want = hr.reference(q)["data_loss"]
        print(f"HINGE lbfgs n={n} loss={r['loss'][-1]:.8g} ref={want:.8g}")
        assert abs(r["loss"][-1] - want) <= LOSS_RTOL * abs(want), (n, r["loss"][-1], want)
        traces.append(r["loss"])
    assert np.array_equal(traces[2][:1], traces[0]) and np.array_equal(traces[2][:2], traces[1])
    assert traces[2][2] < traces[2][0] < hr.reference_of(p)["data_loss"]


# ---- 8. synthetic data ---------------------------------------------------------------------------------------------------
def test_synth_data_draws_only_classes_the_thresholds_allow(ctx):
    p = hr.layout("A", 20)
    hr.to_context(p, ctx)
    try:
        ctx.synth_data(seed=77, noise=0.5, frac_nan=0.0)
        D = ctx.impute(KEEP | LINK)                                   # no entry is missing: the stored matrix
    finally:
        ctx.set_data(p["D"])
    assert np.isfinite(D).all()
    assert set(np.unique(D[:, 20:75])) == {0.0, 1.0} and set(np.unique(D[:, 110:165])) == {1.0, 2.0, 3.0}
    assert set(np.unique(D[:, 0:20])) == {0.0, 1.0} and len(np.unique(D[:, 75:110])) > 1000
    # the classes follow z
    z, d = hr.impute(p)[1][:, 110:165], D[:, 110:165]
    assert d[z > 0.5].mean() > d[z < -0.5].mean() + 0.5, (d[z > 0.5].mean(), d[z < -0.5].mean())


# ---- 9. end to end --------------------------------------------------------------------------------------------------------
def test_fit_of_the_production_assays_end_to_end(pkg):
    rng = np.random.default_rng(91)
    M, N, K = 64, 96, 4
    assays = ["mrnaseq"] * 30 + ["methylation"] * 24 + ["mutation"] * 24 + ["cna"] * 18
    dmap = pkg.data_io.DISTRIBUTION_MAP
    Z = rng.standard_normal((M, K)) @ rng.standard_normal((K, N)) * 0.7
    D = (Z + 0.3 * rng.standard_normal((M, N))).astype(np.float32)
    D[:, 54:78] = (Z[:, 54:78] + 0.5 * rng.standard_normal((M, 24)) > 0.5)
    D[:, 78:] = 1 + (Z[:, 78:] > -0.5) + (Z[:, 78:] > 0.5)
    D[rng.random((M, N)) < 0.05] = np.nan
    batches = {a: [f"{a}{i * 2 // M}" for i in range(M)] for a in ("mrnaseq", "methylation", "mutation", "cna")}
    model = pkg.make_model(D, K=K, feature_views=assays, feature_distributions=[dmap[a] for a in assays],
                           sample_conditions=["c1"] * 30 + ["c2"] * 34, batch_dict=batches, rng=np.random.default_rng(92))
    try:
        hist = pkg.fit_(model, lr=0.05, max_epochs=20, keep_history=True, verbosity=0, stages="library", postprocess="library",
                        batch_em_max_iter=3)
        names = [str(h.get("name")) for h in hist]
        fits = [h for h in hist if "term_code" in h]
        print("HINGE fit_ stages: " + " ".join(names))
        # (basic_fit_ runs init_logsigma_ and its first reweight_col_losses_ without the history: they leave no entry)
        for stage in ("init_mu", "regress_against_sample_conditions", "init_theta", "batch_effect_EM_procedure", "init_factors",
                      "reweight_eb", "reweight_col_losses", "reorder_factors", "finish"):
            assert stage in names, (stage, names)
        assert len(fits) >= 3, names
        losses = [np.asarray(h["loss"], np.float64) for h in fits]
        assert all(np.isfinite(l).all() and len(l) for l in losses)
        assert losses[-1][-1] < losses[-1][0], losses[-1]
        nm = model.matfac.noise_model
        out = pkg.impute(model, include_batch_effects=True)
        assert np.isfinite(out).all()
        seen = {}
        for r, d in zip(nm.col_ranges, nm.noises):
            cols = out[:, r.start - 1:r.stop]
            if d == "bernoulli_sq_hinge":
                assert set(np.unique(cols)) <= {0.0, 1.0}
            elif d == "ordinal_sq_hinge3":
                assert set(np.unique(cols)) <= {1.0, 2.0, 3.0}
            seen[d] = len(np.unique(cols))
        assert seen["bernoulli_sq_hinge"] == 2 and seen["ordinal_sq_hinge3"] >= 2, seen
    finally:
        model.release_device()
