"""Host-side checks of the simulation layer: the numpy twin of the Philox4x32-10 stream (tests/simulate_ref.py) against
Random123's known answers and its draws' statistics, average_precision on hand-computed cases, and simulate_params_ on a
small model (shapes, determinism, corrupt_S's counts, the planted entries of Y).  No GPU."""
import numpy as np
import pytest

import simulate_ref as sr


# ---- the generator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,k,want", sr.KAT)
def test_philox_known_answers(c, k, want):
    got = sr.philox4x32(c, k)
    assert tuple(int(x) for x in got) == want


def test_words_use_the_global_row_and_both_seed_halves():
    a = sr.words(7, np.arange(5) + 131, np.arange(4))
    b = sr.words(7, np.arange(140), np.arange(4))
    assert all(np.array_equal(x, y[131:136]) for x, y in zip(a, b))
    c = sr.words(7 + 2 ** 32, np.arange(5) + 131, np.arange(4))
    assert not np.array_equal(a[0], c[0])
    one = sr.philox4x32((131, 0, 3, 0), (7, 1))
    assert [int(x[0, 3]) for x in c] == [int(x) for x in one]
    big = sr.words(1, [2 ** 32 + 5], [0])                       # a row past 2^32 reaches the second counter word
    assert [int(x[0, 0]) for x in big] == [int(x) for x in sr.philox4x32((5, 1, 0, 0), (1, 0))]


@pytest.fixture(scope="module")
def big_draw():
    n = 1 << 22
    return sr.uniforms(sr.words(123, np.arange(n // 4), np.arange(4)))


def test_draw_ranges_and_moments(big_draw):
    u1, u2, u3, u4 = (u.ravel() for u in big_draw)
    n = u1.size
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    for u in (u3, u4):
        assert u.min() >= 0 and u.max() < 1
        assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / n)
    z = sr.normal64(u1, u2)
    # mean: standard error 1 / sqrt(n); variance of a standard normal's square is 2
    assert abs(z.mean()) <= 5 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n), z.var()
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12


def test_f32_normal_is_within_1e5_of_f64(big_draw):
    u1, u2, _, _ = big_draw
    err = np.abs(sr.normal32(u1, u2).astype(np.float64) - sr.normal64(u1, u2)).max()
    print(f"max |n32 - n64| over 2^22 draws = {err:.3e}")
    assert err < 1e-5


def test_missing_mask_edges():
    d = sr.draws(5, 64, 33)
    assert not sr.missing_mask(d, 0.0).any() and sr.missing_mask(d, 1.0).all()
    assert np.array_equal(sr.missing_mask(d, 2.0 ** -24), d["u3"] == 0)


@pytest.mark.parametrize("K,M,N", [(32, 300, 129), (97, 300, 65)])
def test_bernoulli_near_ties_are_rare(K, M, N):
    """The problems of the device's Bernoulli check: entries whose u4 lies within impute's bound of the probability (where
    the device may legitimately decide the other way) stay far below the 1 % cap; counted with the f64 and the f32 twin."""
    p = sr.sim_case(K, M, N)
    cols = np.flatnonzero(sr.kinds_of(p) == 1)
    assert cols.size
    z = sr.link_space(p, sr.BATCH)
    tol = sr.impute_tol(p, sr.BATCH, z)[:, cols]
    u4 = sr.draws(3, M, N)["u4"][:, cols]
    p64 = sr.sigmoid64(z[:, cols])
    near = np.abs(u4 - p64) <= tol
    z32 = sr.link_space(p, sr.BATCH, np.float32)[:, cols]
    p32 = (np.float32(1) / (np.float32(1) + np.exp(-z32))).astype(np.float64)
    differ = (u4 < p64) != (u4 < p32)
    print(f"near ties: {near.mean():.2e} of {near.size}; f32 twin decides otherwise at {differ.sum()}")
    assert near.mean() <= 0.01 and np.all(near[differ])


# ---- average_precision -------------------------------------------------------------------------------------------------
def test_average_precision_by_hand(pkg):
    ap = pkg.average_precision
    t = np.array([True, False, True, False])
    assert ap(np.array([4.0, 3.0, 2.0, 1.0])[[0, 2, 1, 3]], t) == 1.0                 # positives ranked first: perfect
    assert ap(np.ones(4), t) == 0.5                                                   # all ties: the base rate
    # no positive at the top: ranks 3 and 4 are the positives -> 0.5 * (1/3) + 0.5 * (2/4)
    got = ap(np.array([4.0, 3.0, 2.0, 1.0]), np.array([False, False, True, True]))
    assert abs(got - (0.5 / 3 + 0.5 * 0.5)) < 1e-15
    # a tie across a positive and a negative enters at once: thresholds {3}, {2, 2}, {1}
    got = ap(np.array([3.0, 2.0, 2.0, 1.0]), np.array([True, True, False, False]))
    assert abs(got - (0.5 * 1.0 + 0.5 * (2 / 3))) < 1e-15
    precs = pkg.Y_average_precs(np.array([[-4.0, 3.0, -2.0, 1.0], [1.0, 1.0, 1.0, 1.0]]),
                                np.array([[True, True, False, False], [True, False, True, False]]))
    assert precs == [1.0, 0.5]
    with pytest.raises(ValueError):
        pkg.Y_average_precs(np.zeros((2, 3)), np.zeros((3, 2), bool))


# ---- simulate_params_ --------------------------------------------------------------------------------------------------
M_, N_, K_ = 24, 40, 3
VIEWS = ["mrnaseq"] * 24 + ["mutation"] * 16
DISTS = ["normal"] * 16 + ["ordinal_sq_hinge3"] * 8 + ["bernoulli_sq_hinge"] * 16
SETS = {"mrnaseq": [[f"f{j}" for j in range(0, 10)], [f"f{j}" for j in range(10, 20)], [f"f{j}" for j in range(4, 16)]],
        "mutation": [[f"f{j}" for j in range(24, 34)], [f"f{j}" for j in range(30, 40)]]}


def small_model(pkg, fsard=True, seed=0):
    rng = np.random.default_rng(seed)
    kw = dict(feature_sets_dict=SETS, Y_fsard=True) if fsard else dict(Y_ard=True)
    return pkg.make_model(np.zeros((M_, N_), np.float32), K=K_, sample_conditions=["a"] * 12 + ["b"] * 12,
                          feature_ids=[f"f{j}" for j in range(N_)], feature_views=VIEWS, feature_distributions=DISTS,
                          batch_dict={"mrnaseq": ["b1"] * 8 + ["b2"] * 16}, rng=rng, **kw)


def params_of(model):
    mf = model.matfac
    ct = mf.col_transform
    out = [mf.X, mf.Y, ct.unwrapped(1).logsigma, ct.unwrapped(3).mu]
    out += list(ct.unwrapped(2).logdelta.values) + list(ct.unwrapped(4).theta.values)
    return [np.array(a) for a in out]


def test_simulate_params_shapes_and_determinism(pkg):
    a, b, c = (small_model(pkg) for _ in range(3))
    before = params_of(a)
    thr_before = list(a.matfac.noise_model.thresholds)
    pkg.simulate_params_(a, np.random.default_rng(11))
    pkg.simulate_params_(b, np.random.default_rng(11))
    pkg.simulate_params_(c, np.random.default_rng(12))
    pa, pb, pc = params_of(a), params_of(b), params_of(c)
    for x0, xa, xb in zip(before, pa, pb):
        assert xa.shape == x0.shape and xa.dtype == x0.dtype and np.array_equal(xa, xb) and np.isfinite(xa).all()
    assert not np.array_equal(pa[0], pc[0]) and not np.array_equal(pa[1], pc[1])
    assert a.matfac.X.shape == (K_, M_) and a.matfac.Y.shape == (K_, N_) and a.matfac.X.dtype == np.float32
    # column parameters follow their view's table (simulate_params.jl:124-142); logsigma then loses log(sqrt(K))
    fv = np.array(a.feature_views)
    mu, ls = pa[3], pa[2]
    assert abs(mu[fv == "mrnaseq"].mean() - 10.0) < 5 * 2.0 / np.sqrt(24) and abs(mu[fv == "mutation"].mean() + 1.5) < 0.1
    assert abs(ls[fv == "mutation"].mean() - (0.0 - np.log(np.sqrt(K_)))) < 0.01
    # thresholds: ordinal_sq_hinge3 doubled (:111-113), bernoulli_sq_hinge left alone
    nm = a.matfac.noise_model
    for name, t0, t1 in zip(nm.noises, thr_before, nm.thresholds):
        if name == "ordinal_sq_hinge3":
            assert t1 == (-np.inf, -1.0, 1.0)
        else:
            assert t0 == t1
    # the ARD and L2 / group methods
    d = small_model(pkg, fsard=False)
    pkg.simulate_params_(d, np.random.default_rng(11), ard_alpha=2.0, ard_beta=2.0)
    assert np.isfinite(d.matfac.Y).all() and d.matfac.Y.std() > 0.1


def test_corrupt_S_counts_and_planted_entries(pkg):
    from importlib import import_module
    sim = import_module(pkg.__name__ + ".simulate")
    model = small_model(pkg)
    reg = model.matfac.Y_reg
    S_before = [np.array(S) for S in reg.S]
    pkg.simulate_params_(model, np.random.default_rng(5), S_add_corruption=0.25, S_rem_corruption=0.1)
    for cr, S0, S1, A in zip(reg.col_ranges, S_before, reg.S, reg.A):
        for l in range(S0.shape[0]):
            old, new = set(np.flatnonzero(S0[l])), set(np.flatnonzero(S1[l]))
            n = len(old)
            assert len(old - new) == int(round(0.1 * n)) and len(new - old) == int(round(n * 0.25))     # :30-34
            assert np.allclose(S1[l][sorted(new)], 1 / np.sqrt(len(new)), rtol=1e-6)                    # :38
        assert ((A != 0).sum(0) == 1).all() and (A >= 0).all()                                         # one set per factor
        planted = (A.T @ S1) > 0
        Yv = model.matfac.Y[:, cr.start - 1:cr.stop]
        assert planted.any() and not planted.all()
        assert np.all(np.abs(Yv[planted]) == 1.0)                                                      # :76-77
        assert not np.any(np.abs(Yv[~planted]) == 1.0)
    # corrupt_S alone: nothing to remove or add leaves the sets and renormalises
    S = np.array([[1, 1, 0, 0], [0, 0, 0, 2]], np.float32)
    out = sim.corrupt_S(S, 0.0, 0.0, np.random.default_rng(0))
    assert np.allclose(out, [[2 ** -0.5, 2 ** -0.5, 0, 0], [0, 0, 0, 1]])


def test_simulate_params_refuses_unknown_regularizers(pkg):
    model = pkg.make_model(np.zeros((6, 5), np.float32), K=2)
    with pytest.raises(TypeError):
        pkg.simulate_params_(model, np.random.default_rng(0))
