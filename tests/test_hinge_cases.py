"""The squared-hinge reference and problems of tests/test_gpu_hinge.py are what they claim to be (no GPU).

* hinge_ref restates the whole per-entry model; on kinds 0..2 (batch views, rows in no batch, NaN, weights) it equals the C
  oracle to 1e-12 relative in the loss, the factor and layer gradients and the pmf_stats vectors, and its layer scales
  equal problems.layer_scales -- everything the new reference shares with the old one is pinned;
* the literal cases of the kind-3 rule, z on both sides of every margin;
* CompositeNoise / make_model accept the production distribution map and keep the thresholds per range;
* the conditions that make the device comparison mean something, on every problem the GPU file runs: every class occurs in
  every kind-3 range; between 20 % and 90 % of the observed kind-3 entries have g != 0; at least 50 entries have both
  terms active; exchanging the thresholds of two ranges, reading the class off by one, or treating kind 3 as Poisson moves
  gX or gY by at least 10 GRAD_TOL in rel_err; at most 1 % of the kind-3 entries lie within 1e-3 of a threshold (the
  entries the impute comparison leaves out).
"""
import numpy as np
import pytest

import hinge_ref as hr
from problems import layer_scales, make_problem, rel_err, to_oracle
from test_gpu_parity import GRAD_TOL

INF = np.inf
OLD_KINDS = {
    "mixed_batch_nan": dict(M=70, N=173, K=20, seed=5, bernoulli_frac=0.2, poisson_frac=0.1, n_views=3, batch_views=2,
                            n_batches=5, nan_frac=0.1, weights=True, col_params=True, scale=0.4),
    "k48_one_view": dict(M=97, N=77, K=48, seed=6, bernoulli_frac=0.3, n_views=2, batch_views=1, n_batches=3,
                         nan_frac=0.05, weights=True, col_params=True, scale=0.3),
    "plain_poisson": dict(M=33, N=40, K=7, seed=7, poisson_frac=0.5, nan_frac=0.2, weights=True, col_params=True, scale=0.4),
}


def old_problem(name):
    p = make_problem(**OLD_KINDS[name])
    if p["batch_views"]:
        p["batch_views"][0]["batch_of_row"][[0, 31, p["M"] - 1]] = -1          # rows in no batch
    return p


@pytest.mark.parametrize("name", list(OLD_KINDS))
def test_reference_equals_the_c_oracle_on_the_existing_kinds(name):
    p = old_problem(name)
    m = to_oracle(p)
    _, go = m.loss_and_grads(update_X=True, update_Y=True, update_col_layers=True)
    r = hr.reference(p)
    assert abs(r["data_loss"] - go["data_loss"]) <= 1e-12 * abs(go["data_loss"])
    for k in ("X", "Y", "mu", "logsigma"):
        assert rel_err(r[k], go[k]) <= 1e-12, k
    for k in ("theta", "logdelta"):
        for v in range(len(p["batch_views"])):
            assert rel_err(r[k][v], go[k][v]) <= 1e-12, (k, v)
    for uf in (False, True):
        so, s = m.stats(uf), hr.stats(p, uf)
        assert np.array_equal(s["n"], so["n"])
        for k in ("sum", "sumsq", "sqerr", "ssq_grad"):
            assert rel_err(s[k], so[k]) <= 1e-12, (k, uf)
        for v in range(len(p["batch_views"])):
            assert np.array_equal(s["batch_count"][v], so["batch_count"][v])
            assert rel_err(s["batch_sqerr"][v], so["batch_sqerr"][v]) <= 1e-12
    assert rel_err(hr.forward(p)[3], m.forward()) <= 1e-12
    a, b = hr.layer_scales(p), layer_scales(p)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * b["loss"]
    for k in ("mu", "logsigma", "g"):
        assert rel_err(a[k], b[k]) <= 1e-12, k
    for k in ("theta", "logdelta"):
        for v in range(len(p["batch_views"])):
            assert rel_err(a[k][v], b[k][v]) <= 1e-12, (k, v)


# ---- the literal cases of the rule ------------------------------------------------------------------------------------
def lg(z, y, t, w=1.0):
    a, b = hr.hinge_terms(np.float64(z), np.float64(y), np.asarray(t, np.float64))
    return 0.5 * w * (a * a + b * b), w * (b - a)


def test_every_class_of_bernoulli_sq_hinge():
    t = (0.0, INF, INF)
    # y = 0: hi = 0, 0.5 relu(1 + z)^2
    assert lg(-1.5, 0, t) == (0.0, 0.0) and lg(-1.0, 0, t) == (0.0, 0.0)
    assert lg(-0.5, 0, t) == (0.125, 0.5) and lg(2.0, 0, t) == (4.5, 3.0)
    # y = 1: lo = 0, 0.5 relu(1 - z)^2
    assert lg(1.5, 1, t) == (0.0, 0.0) and lg(1.0, 1, t) == (0.0, 0.0)
    assert lg(0.5, 1, t) == (0.125, -0.5) and lg(-2.0, 1, t) == (4.5, -3.0)
    assert lg(0.5, 1, t, w=2.0) == (0.25, -1.0)


def test_every_class_of_ordinal_sq_hinge3():
    t = (-INF, -2.0, 3.0)
    # class 1: (-inf, -2]: only the upper margin, active from z > -3
    assert lg(-3.5, 1, t) == (0.0, 0.0) and lg(-2.5, 1, t) == (0.125, 0.5)
    # class 2: (-2, 3], margins at -1 and 2: free inside
    assert lg(0.0, 2, t) == (0.0, 0.0) and lg(-1.5, 2, t) == (0.125, -0.5) and lg(2.5, 2, t) == (0.125, 0.5)
    # class 3: (3, inf): only the lower margin, active below 4
    assert lg(4.5, 3, t) == (0.0, 0.0) and lg(3.5, 3, t) == (0.125, -0.5)
    # class 0 never occurs in such a column; its bin is (-inf, -inf]: nothing, and finite
    assert lg(0.3, 0, t) == (0.0, 0.0)


def test_both_terms_are_active_in_a_narrow_class():
    t = (-INF, -0.5, 0.5)                                   # t2 - t1 = 1 < 2: the margins of class 2 overlap on (-0.5, 0.5)
    a, b = hr.hinge_terms(np.float64(0.25), np.float64(2), np.asarray(t))
    assert (a, b) == (0.25, 0.75)
    assert lg(0.25, 2, t) == (0.5 * (0.0625 + 0.5625), 0.5)
    assert lg(0.0, 2, t) == (0.25, 0.0)                     # symmetric: the gradient vanishes, the loss does not


def test_a_class_whose_lower_bound_is_plus_infinity_costs_nothing():
    t = (0.0, INF, INF)
    for y in (2, 3, 7):                                    # classes bernoulli_sq_hinge never holds: lo = +inf (and hi = +inf)
        for z in (-3.0, 0.0, 3.0):
            l, g = lg(z, y, t)
            assert np.isfinite(l) and np.isfinite(g) and (l, g) == (0.0, 0.0)
    assert lg(0.2, -4, t) == lg(0.2, 0, t)                  # the class clamps at 0 ...
    assert hr.hinge_class([-0.7, 0.49, 0.5, 1.49, 2.5, 9.0]).tolist() == [0, 0, 1, 1, 3, 3]   # ... and at 3; halves round up


def test_impute_rule_counts_the_thresholds_strictly_below():
    p = hr.layout("B", 20)
    v, z = hr.impute(p)
    assert set(np.unique(v[:, :40])) <= {1, 2, 3} and set(np.unique(v[:, 40:50])) <= {0, 1}
    j = 60                                                  # thresholds (-inf, -1.2, 0.3)
    assert np.array_equal(v[:, j], 1 + (z[:, j] > -1.2) + (z[:, j] > 0.3))
    assert np.array_equal(hr.impute(p, link=True)[0], z)


# ---- the model layer --------------------------------------------------------------------------------------------------
def test_composite_noise_and_make_model_accept_the_production_map(pkg):
    mf, dio = pkg.matfac, pkg.data_io
    assert dio.DISTRIBUTION_MAP["mutation"] == "bernoulli_sq_hinge" and dio.DISTRIBUTION_MAP["cna"] == "ordinal_sq_hinge3"
    assert {"bernoulli_sq_hinge", "ordinal_sq_hinge3"} <= set(mf.SUPPORTED_LOSSES)
    assert pkg._lib.NOISE["bernoulli_sq_hinge"] == pkg._lib.NOISE["ordinal_sq_hinge3"] == 3
    assays = ["mrnaseq"] * 5 + ["methylation"] * 4 + ["mutation"] * 6 + ["cna"] * 3
    nm = mf.CompositeNoise([dio.DISTRIBUTION_MAP[a] for a in assays])
    assert nm.noises == ("normal", "bernoulli_sq_hinge", "ordinal_sq_hinge3")
    assert nm.thresholds == [None, (0.0, INF, INF), (-INF, -0.5, 0.5)]
    nm.set_thresholds_("ordinal_sq_hinge3", (-1.0, 0.25))
    nm.set_thresholds_(1, 0.5)
    assert nm.thresholds == [None, (0.5, INF, INF), (-INF, -1.0, 0.25)]
    with pytest.raises(ValueError):
        nm.set_thresholds_("normal", 0.0)
    with pytest.raises(ValueError):
        nm.set_thresholds_("ordinal_sq_hinge3", (1.0, 0.0))
    with pytest.raises(NotImplementedError, match="not implemented by the HIP path"):
        mf.CompositeNoise(["normal", "ordinal3"])
    rng = np.random.default_rng(0)
    D = rng.standard_normal((12, len(assays))).astype(np.float32)
    D[:, 9:15] = rng.integers(0, 2, (12, 6))
    D[:, 15:] = rng.integers(1, 4, (12, 3))
    model = pkg.make_model(D, K=3, feature_views=assays, feature_distributions=[dio.DISTRIBUTION_MAP[a] for a in assays],
                           rng=np.random.default_rng(1))
    got = model.matfac.noise_model
    assert set(got.noises) == {"normal", "bernoulli_sq_hinge", "ordinal_sq_hinge3"}
    assert sorted(t for t in got.thresholds if t is not None) == [(-INF, -0.5, 0.5), (0.0, INF, INF)]


# ---- the conditions of the device comparison -------------------------------------------------------------------------
PROBLEMS = hr.all_problems()


@pytest.mark.parametrize("name,p", [pytest.param(n, p, id=n) for n, p in PROBLEMS])
def test_the_problems_exercise_the_rule(name, p):
    r = hr.reference_of(p)
    kind, thr = hr.kinds_of(p), hr.thresholds_of(p)
    obs = np.isfinite(p["D"])
    for (s, e), t in zip(p["noise_ranges"], p["noise_thr"]):
        if t is None:
            continue
        d = p["D"][:, s - 1:e]
        want = {0.0, 1.0} if np.isposinf(t[1]) else {1.0, 2.0, 3.0}
        assert set(np.unique(d[np.isfinite(d)])) == want, ((s, e), t)          # every class occurs, and no other
    h = kind == 3
    oh = obs[:, h]
    frac = np.count_nonzero(r["g"][:, h][oh]) / oh.sum()
    both = int(np.count_nonzero((r["a"][:, h] > 0) & (r["b"][:, h] > 0)))
    near = int(np.count_nonzero(hr.threshold_gap(p, r["z"])[:, h] < 1e-3))
    nob = hr.impute(p, batch=False)[1]
    near_nb = int(np.count_nonzero(hr.threshold_gap(p, nob)[:, h] < 1e-3))
    moved = {}
    for fname, q, fault in (("swap", hr.swapped_thresholds(p), None), ("off_by_one", p, "off_by_one"), ("poisson", p, "poisson")):
        f = hr.reference(q, fault)
        moved[fname] = max(rel_err(f["X"], r["X"]), rel_err(f["Y"], r["Y"]))
    print(f"HINGE_CASE {name} active={frac:.3f} both={both} near={near}/{near_nb} of {h.sum() * p['M']} moved=" +
          " ".join(f"{k}:{v:.3f}" for k, v in moved.items()))
    assert 0.20 <= frac <= 0.90, frac
    assert both >= 50, both
    assert max(near, near_nb) <= 0.01 * h.sum() * p["M"], (near, near_nb)
    for fname, v in moved.items():
        assert v >= 10 * GRAD_TOL, (fname, v)
    assert np.isfinite(r["data_loss"]) and np.isfinite(r["X"]).all() and np.isfinite(r["Y"]).all()


def test_layouts_are_the_ones_the_gpu_file_describes():
    a, b = hr.layout("A", 20, True), hr.layout("B", 20, True)
    assert (a["M"], a["N"], b["M"], b["N"]) == (70, 173, 70, 77)
    assert a["noise_ranges"] == [(1, 20), (21, 75), (76, 110), (111, 165), (166, 173)]
    assert a["noise_kinds"] == ["bernoulli", "bernoulli_sq_hinge", "normal", "ordinal_sq_hinge3", "poisson"]
    assert b["noise_ranges"] == [(1, 40), (41, 50), (51, 77)] and b["noise_kinds"] == [3, 3, 3]
    assert len({tuple(t) for t in b["noise_thr"]}) == 3
    ka, kb = hr.kinds_of(a), hr.kinds_of(b)
    assert (ka[32:64] == 3).all() and (ka[128:160] == 3).all()                  # a whole tile of each new model
    assert len(set(ka[0:32])) == 2 and len(set(ka[64:96])) == 2 and len(set(ka[160:173])) == 2   # tiles shared with a neighbour
    assert len({tuple(t) for t in hr.thresholds_of(b)[32:64]}) == 3             # three threshold sets inside tile 1 (0-based)
    assert (kb == 3).all() and b["N"] % 32 == 13                                # dead columns behind a kind-3 range
    for p, name in ((a, "A"), (b, "B")):
        v0, v1 = p["batch_views"]
        assert v0["stop1"] == hr.SEAMS[name] and v1["start1"] == hr.SEAMS[name] + 1 and v1["stop1"] == p["N"]
        assert 32 < hr.SEAMS[name] < 64 and hr.kinds_of(p)[hr.SEAMS[name] - 1] == 3   # the seam is inside a kind-3 tile
        assert (v0["batch_of_row"] < 0).any()
        assert np.isnan(p["D"]).mean() > 0.05 and len(set(p["col_weight"])) > 1
