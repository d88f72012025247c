"""The library's batch-effect EM and group weights (csrc/pmf_stages.hip) past one grid and at the seams of their four-element
quads, against oracle/em_oracle.py and the fp64 formulas -- where tests/test_gpu_library_stages.py stops at tables of 1712
elements (two workgroups).  k_em_theta runs min(1024, ceil(nbt / 1024)) workgroups of 256 threads x 4 elements, so one grid
covers 1,048,576 elements of the flat theta table (nbt), then takes grid-stride trips; k_em_diff adds the workgroups'
partials, 256 per trip.

Models: M = 40, K = 2, about 10 % Bernoulli and 5 % Poisson columns, 8 % missing; three EM iterations, rtol = 0.
  E1  one view, 17 batches x 62001 columns   nbt = 1,054,017   a second stride trip of k_em_theta; nbt % 4 = 1: a partial
                                                                last quad and the unaligned source bst + nbt of k_st_widen
  E2  one view, 17 x 17001                   nbt =   289,017   283 workgroups: the second trip of k_em_diff
  E3  two views, 15 x 16501 each             nbt =   495,030   val_off[1] % 4 = 3: quads that span the view seam
Bounds: theta and delta^2 within REL of the oracle, NaN / inf positions equal; the stopping ratios within DIFF_BOUND
(tests/test_gpu_library_stages.py) of the oracle's and of the host path's.
Group weights: k_stage_group on noise ranges of 1, 256, 257 and 1025 columns (one, one full, one full + 1 and four + 1
strides of its 256 threads) against the fp64 formula on the oracle's column statistics, within RTOL."""
import numpy as np
import pytest

from problems import make_problem, rel_err, to_context, to_oracle
from test_gpu_library_stages import DIFF_BOUND, DIFF_HOST_DEV, DIFF_MIN, REL, RTOL, _em_inputs, diffs_deviation
from test_gpu_shard_fit import _batch_values, _cat

pytestmark = pytest.mark.gpu

WM, WK, W_ITERS = 40, 2, 3
# name: per batch view (columns, batches), and the column kinds of the view in model order (distribution, then view)
WIDE = {
    "E1": [(62001, 17, (("bernoulli", 6200), ("normal", 52701), ("poisson", 3100)))],
    "E2": [(17001, 17, (("bernoulli", 1700), ("normal", 14451), ("poisson", 850)))],
    "E3": [(16501, 15, (("bernoulli", 3300), ("normal", 13201))), (16501, 15, (("normal", 14851), ("poisson", 1650)))],
}
W_NBT = {"E1": 1054017, "E2": 289017, "E3": 495030}


def _make_wide(pkg, name):
    rng = np.random.default_rng(61)
    spec = WIDE[name]
    views = [f"v{i}" for i, (nv, _, _) in enumerate(spec) for _ in range(nv)]
    dists = [d for _, _, kinds in spec for d, cnt in kinds for _ in range(cnt)]
    n = len(views)
    assert len(dists) == n and sum(nv * nb for nv, nb, _ in spec) == W_NBT[name]
    batches = {f"v{i}": [f"b{i}_{(r * nb) // WM}" for r in range(WM)] for i, (_, nb, _) in enumerate(spec)}
    kind = np.array(dists)
    D = (rng.standard_normal((WM, n)) * (0.5 + rng.random(n)) + rng.standard_normal(n)).astype(np.float32)
    D[:, kind == "bernoulli"] = (D[:, kind == "bernoulli"] > 0).astype(np.float32)
    D[:, kind == "poisson"] = rng.poisson(2.0, size=(WM, int((kind == "poisson").sum()))).astype(np.float32)
    D[rng.random((WM, n)) < 0.08] = np.nan
    model = pkg.make_model(D, K=WK, sample_conditions=["c1"] * 20 + ["c2"] * 20, feature_views=views,
                           feature_distributions=dists, batch_dict=batches, rng=np.random.default_rng(62))
    assert list(model.data_idx) == list(range(1, n + 1))                 # the columns were given in model order
    th = _batch_values(model)[1]
    assert [v.shape for v in th] == [(nb, nv) for nv, nb, _ in spec]
    return model


def _seed_wide(model, seed):
    rng = np.random.default_rng(seed)
    mf, ct = model.matfac, model.matfac.col_transform
    n = model.data.shape[1]
    mf.X[...] = 0.3 * rng.standard_normal(mf.X.shape)
    mf.Y[...] = 0.3 * rng.standard_normal(mf.Y.shape)
    ct.unwrapped(3).mu[...] = 0.3 * rng.standard_normal(n)
    ct.unwrapped(1).logsigma[...] = 0.2 * rng.standard_normal(n)
    ld, th = _batch_values(model)
    for v in th:
        v[...] = (0.5 * rng.standard_normal(v.shape)).astype(np.float32)
    for v in ld:
        v[...] = (0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    mf.noise_model.set_weight_(np.ones(n, np.float32))
    return rng


def _oracle_em(model, delta2, sigma2, update_priors):
    from oracle import em_oracle
    mf, ct = model.matfac, model.matfac.col_transform
    theta_ba = ct.unwrapped(4).theta
    views = [dict(start1=cr.start, stop1=cr.stop, batch_of_row=np.asarray(rb), logdelta=np.array(ld), theta=np.array(t))
             for cr, rb, ld, t in zip(theta_ba.col_ranges, theta_ba.row_batches, ct.unwrapped(2).logdelta.values, theta_ba.values)]
    kinds = [d for d, cr in zip(mf.noise_model.noises, mf.noise_model.col_ranges) for _ in range(len(cr))]
    assert set(kinds) == {"bernoulli", "normal", "poisson"} and len(kinds) == model.data.shape[1]
    theta, d2, diffs = em_oracle.theta_delta_em(model.data, mf.X, mf.Y, ct.unwrapped(1).logsigma, ct.unwrapped(3).mu, views,
                                                kinds, delta2, sigma2, update_priors=update_priors, max_iter=W_ITERS, rtol=0.0)
    return _cat(theta), _cat(d2), np.array(diffs)


def _run_em(pkg, model, stages, update_priors):
    rng = _seed_wide(model, 301)
    delta2, sigma2 = _em_inputs(model, rng)
    want = _oracle_em(model, delta2, sigma2, update_priors) if stages == "oracle" else None
    if want is not None:
        return want
    hist = []
    theta, d2 = pkg.theta_delta_em(model, [d.copy() for d in delta2], sigma2.copy(), update_priors=update_priors, verbosity=0,
                                   history=hist, stages=stages, batch_em_max_iter=W_ITERS, batch_em_rtol=0.0)
    return _cat(theta), _cat(d2), np.array(hist[-1]["diffs"])


@pytest.mark.parametrize("update_priors", [True, False])
@pytest.mark.parametrize("name", list(WIDE))
def test_wide_em_matches_the_oracle_and_its_stopping_ratio(pkg, name, update_priors):
    model = _make_wide(pkg, name)
    try:
        want = _run_em(pkg, model, "oracle", update_priors)
        host = _run_em(pkg, model, "host", update_priors)
        got = _run_em(pkg, model, "library", update_priors)
        again = _run_em(pkg, model, "library", update_priors)          # the same context, re-marshalled
    finally:
        model.release_device()
    assert len(want[2]) == len(host[2]) == len(got[2]) == W_ITERS and np.all(want[2] >= DIFF_MIN), want[2]
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b)
    for label, g, w in (("theta", got[0], want[0]), ("delta2", got[1], want[1])):
        assert g.shape == w.shape == (W_NBT[name],)
        e = rel_err(g[np.isfinite(w)], w[np.isfinite(w)])
        print(f"LIB_STAGE_EDGE {name} update_priors={update_priors} {label} err={e:.3e} (bound {REL:g})")
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isposinf(g), np.isposinf(w))
        assert np.array_equal(np.isneginf(g), np.isneginf(w))
        assert e <= REL, (label, e)
    dev = dict(host_vs_oracle=diffs_deviation(host[2], want[2], want[2]), library_vs_oracle=diffs_deviation(got[2], want[2], want[2]),
               library_vs_host=diffs_deviation(got[2], host[2], want[2]))
    print(f"LIB_STAGE_EDGE {name} update_priors={update_priors} diffs oracle " + " ".join(f"{d:.6e}" for d in want[2]) + " | "
          + " ".join(f"{k}={v:.3e}" for k, v in dev.items()) + f" (bound {DIFF_BOUND:g})")
    assert dev["host_vs_oracle"] <= max(DIFF_HOST_DEV, DIFF_BOUND / 4)      # the measurement DIFF_BOUND rests on still holds
    assert dev["library_vs_oracle"] <= DIFF_BOUND and dev["library_vs_host"] <= DIFF_BOUND, dev


# ---- group weights ---------------------------------------------------------------------------------------------------
GROUP_RANGES = [(1, 1), (2, 257), (258, 514), (515, 1539)]             # 1, 256, 257 and 1025 columns


def test_group_weights_on_ranges_around_the_workgroup_stride(ctx):
    M, N, K = 40, 1539, 3
    assert [e - s + 1 for s, e in GROUP_RANGES] == [1, 256, 257, 1025] and GROUP_RANGES[-1][1] == N
    p = make_problem(M=M, N=N, K=K, seed=63, nan_frac=0.08, col_params=True, weights=True)
    p["D"][:, 700] = np.nan                                              # n_j = 0: the non-finite variance -> 0 rule
    p["noise_ranges"], p["noise_kinds"] = list(GROUP_RANGES), ["normal"] * len(GROUP_RANGES)
    to_context(p, ctx)
    got = ctx.stage_minimal_group_weights(M)
    again = ctx.stage_minimal_group_weights(M)
    so = to_oracle(p).stats(False)
    n, s1, s2 = (np.asarray(so[k], np.float64) for k in ("n", "sum", "sumsq"))
    assert n[700] == 0 and n.max() <= M
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = s1 / n
        var = (s2 - n * mean * mean) / np.maximum(n - 1.0, 1.0)
    var[~np.isfinite(var)] = 0.0
    var = np.maximum(var, 1.0 / M)
    sig2 = np.exp(np.asarray(p["logsigma"], np.float64)) ** 2
    want = np.array([K * np.mean(sig2[s - 1:e]) / (np.sum(var[s - 1:e] * n[s - 1:e]) / M) for s, e in GROUP_RANGES])
    print("LIB_STAGE_EDGE group weights rel err " + " ".join(f"{abs(g - w) / w:.3e}" for g, w in zip(got, want)) + f" (bound {RTOL:g})")
    assert got.shape == want.shape and np.all(np.isfinite(want)) and np.all(want > 0)
    np.testing.assert_allclose(got, want, rtol=RTOL)
    np.testing.assert_array_equal(got, again)
