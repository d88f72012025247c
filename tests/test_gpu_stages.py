"""GPU tests of the "next" rows: column / batch statistics kernel (N1, N2), the closed-form
initialisers and the batch-effect EM built on it, the FeatureSetARD outer loop (N3) and the full fit! orchestration."""
import numpy as np
import pytest

import fsard_ref as fr
from oracle import fsard_oracle as fo
from problems import make_problem, rel_err, to_context, to_oracle
from test_gpu_host import reference_fit_setup

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("use_factors", [False, True])
@pytest.mark.parametrize("case", [
    dict(M=301, N=143, K=8, nan_frac=0.15, col_params=True, weights=True),
    dict(M=420, N=260, K=32, bernoulli_frac=0.2, poisson_frac=0.1, n_views=3, batch_views=2, n_batches=6, nan_frac=0.1,
         weights=True, col_params=True, scale=0.4),
])
def test_statistics_kernel_matches_oracle(ctx, case, use_factors):
    p = make_problem(seed=31, **case)
    to_context(p, ctx)
    st = ctx.stats(use_factors)
    so = to_oracle(p).stats(use_factors)
    assert np.array_equal(st["n"], so["n"])                       # counts are exact
    for k in ("sum", "sumsq", "sqerr", "ssq_grad"):
        assert rel_err(st[k], so[k]) <= 2e-5, k
    for v in range(len(p["batch_views"])):
        assert np.array_equal(st["batch_count"][v], so["batch_count"][v])
        assert rel_err(st["batch_sqerr"][v], so["batch_sqerr"][v]) <= 2e-5


def test_closed_form_initialisers(pkg):
    rng = np.random.default_rng(32)
    M, N, K = 200, 60, 5
    D = (rng.standard_normal((M, N)) * (1 + np.arange(N))[None, :] * 0.1 + 2.0).astype(np.float32)
    D[rng.random((M, N)) < 0.1] = np.nan
    model = pkg.make_model(D, K=K, feature_views=[1] * 30 + [2] * 30, rng=rng)
    Dm = model.data
    ct = model.matfac.col_transform
    # init_mu!: M-estimate of a normal column = its (nan)mean
    pkg.init_mu_(model, lr_mu=0.5, max_epochs=2000, verbosity=0)
    np.testing.assert_allclose(ct.layers[2].mu, np.nanmean(Dm, axis=0), atol=0.08)   # AdaGrad stops at abs_tol 1e-3 (fit.jl:92)
    ct.layers[2].mu[...] = np.nanmean(Dm, axis=0)
    # init_logsigma!: log of the column standard deviation around mu (fit.jl:138-143)
    pkg.init_logsigma_(model)
    np.testing.assert_allclose(ct.layers[0].logsigma, np.log(np.sqrt(np.nanmean((Dm - np.nanmean(Dm, 0)) ** 2, axis=0))), rtol=1e-4)
    # reweight_col_losses!: 1 / (sqrt(sum g^2 / M) * sigma), g = (mu - D) with unit weights (fit.jl:166-176)
    pkg.reweight_col_losses_(model)
    g2 = np.nansum((np.nanmean(Dm, 0)[None, :] - Dm).astype(np.float64) ** 2, axis=0)
    np.testing.assert_allclose(model.matfac.noise_model.weights,
                               1.0 / (np.sqrt(g2 / M) * np.exp(ct.layers[0].logsigma)), rtol=1e-4)
    # construct_minimal_regularizer (regularizers.jl:750-774)
    reg = pkg.construct_minimal_regularizer(model)
    nn = np.isfinite(Dm).sum(0)
    var = np.maximum(np.nanvar(Dm.astype(np.float64), axis=0, ddof=1), 1.0 / M)
    want = K * np.mean(np.exp(ct.layers[0].logsigma) ** 2) / (np.sum(var * nn) / M)
    assert len(reg.group_idx) == 1 and tuple(reg.group_idx[0]) == (1, N)
    np.testing.assert_allclose(reg.group_weights[0], want, rtol=1e-4)
    model.release_device()


def test_batch_effect_initialisation_recovers_shifts(pkg):
    """init_batch_effects! (fit.jl:378-496) on data that is pure (condition mean + batch shift + noise)."""
    rng = np.random.default_rng(33)
    M, N = 240, 40
    conds = ["c1"] * 120 + ["c2"] * 120
    batches = [f"b{i}" for i in range(4) for _ in range(60)]
    shift = np.array([0.0, 1.0, -1.0, 0.5])
    bidx = np.repeat(np.arange(4), 60)
    D = (rng.standard_normal((M, N)) * 0.3 + shift[bidx][:, None] + 3.0).astype(np.float32)
    model = pkg.make_model(D, K=3, sample_conditions=conds, feature_views=[1] * N, batch_dict={1: batches}, rng=rng)
    pkg.init_batch_effects_(model, max_epochs=300, lr_regress=1.0, lr_theta=1.0, lr_mu=0.5, verbosity=0,
                            batch_em_max_iter=20)
    ct = model.matfac.col_transform
    th = ct.layers[3].theta.values[0]
    assert np.all(np.isfinite(th)) and np.all(np.isfinite(ct.layers[1].logdelta.values[0]))
    # batches within a condition are identifiable up to the condition mean: b1-b0 = 1, b3-b2 = 1.5
    assert abs(np.mean(th[1] - th[0]) - 1.0) < 0.15 and abs(np.mean(th[3] - th[2]) - 1.5) < 0.15
    assert abs(np.mean(np.exp(ct.layers[0].logsigma)) - 0.3) < 0.1
    model.release_device()


def test_update_A_matches_numpy_restatement(pkg):
    """update_A_ (host driver + pmf_fsard_update_A) on two small views, 200 epochs, against the float64 oracle within the
    bounds derived in fsard_ref.py (20 x the float32 restatement's discrepancy).  The oracle's trace is all "improved by
    more than atol": the loss falls monotonically, by at least 4.8e-4 (view 2) per epoch against atol = 1e-5 and a loss of
    46 (1.0e-5 of it: less than the 1000 x the loss discrepancy that fsard_ref.MARGIN asks of the edge tables, and far more
    than the device's error on a 60-term loss), so A_best is the last iterate and the termination counter never moves."""
    rng = np.random.default_rng(34)
    K, N, L = 4, 30, 5
    sets = [[list(range(1 + 3 * l, 4 + 3 * l)) for l in range(L)], [list(range(16 + 3 * l, 19 + 3 * l)) for l in range(L)]]
    reg = pkg.regularizers.construct_featureset_ard(K, list(range(1, N + 1)), [1] * 15 + [2] * 15, sets, lr=0.05)
    Y = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    Y[0, :3] += 1.0                                       # factor 1 loads on set 1 of view 1
    pkg.update_lambda_(reg, Y)
    reg.lambda_ = tuple((l * 1e-3).astype(np.float32) for l in reg.lambda_)   # weak L1 so that A stays non-trivial
    lam = [l.copy() for l in reg.lambda_]
    losses = pkg.update_A_(reg, Y, max_epochs=200, term_iter=50, verbosity=0)
    for v, cr in enumerate(reg.col_ranges):
        A = np.zeros((L, K))
        ssq = np.full((L, K), 1e-8)
        best, epochs, trace = fo.update_A_inner(A, reg.S[v].astype(np.float64), Y[:, cr.slice0()].astype(np.float64),
                                                reg.alpha[cr.slice0()].astype(np.float64), float(reg.alpha0), float(reg.v0),
                                                float(reg.lr), lam[v].astype(np.float64), ssq, max_epochs=200, term_iter=50,
                                                trace=True)
        assert epochs == 200 and all(s["branch"] == "w" for s in trace)
        assert min(s["best"] - s["new"] for s in trace) > 40 * 1e-5                 # no improvement is near atol
        beta = (float(reg.alpha0) - 1) * (float(reg.v0) + A.T @ reg.S[v].astype(np.float64))
        got = dict(A=reg.A[v], ssq=reg.ssq_grad[v], beta=reg.beta[:, cr.slice0()], best=losses[v])
        e = fr.errors(got, dict(A=A, ssq=ssq, beta=beta, best=best), np.full((L, K), 1e-8, np.float32))
        print(f"FSARD_ERR stages_small_view{v} " + " ".join(f"{k}={x:.3e}" for k, x in e.items()))
        for k, x in e.items():
            assert x <= fr.TOL[k], (v, k, x)                                         # beta: featureset_ard.jl:292
    assert max(float(A.max()) for A in reg.A) > 0          # a non-trivial assignment matrix was compared


def test_full_fit_orchestration_featureset_ard(pkg):
    """fit!(model) end to end (fit.jl:923-1018) on the reference's fit_tests setup (runtests.jl:1324-1346)."""
    model = reference_fit_setup(pkg, seed=3)
    X_start, Y_start = model.matfac.X.copy(), model.matfac.Y.copy()
    ld_start = [v.copy() for v in model.matfac.col_transform.layers[1].logdelta.values]
    hist = pkg.fit_(model, verbosity=0, lr=0.05, max_epochs=300, rel_tol=1e-5, abs_tol=1e-5, fsard_term_rtol=1e-3,
                    fsard_max_iter=3, fsard_max_A_iter=100, keep_history=True)
    mf = model.matfac
    assert not np.allclose(mf.X, X_start) and not np.allclose(mf.Y, Y_start)            # runtests.jl:1340-1341
    assert not all(np.allclose(a, b) for a, b in zip(ld_start, mf.col_transform.layers[1].logdelta.values))  # :1342
    assert np.all(np.isfinite(mf.X)) and np.all(np.isfinite(mf.Y))
    names = [d.get("name") for d in hist]
    assert names[0] == "start" and names[-1] == "finish" and "reorder_factors" in names
    ssq = np.sum(mf.Y.astype(np.float64) ** 2, axis=1)
    assert np.all(np.diff(ssq) <= 1e-6)                                                  # reorder_by_importance!
    model.release_device()


def test_update_A_kernel_on_a_wide_view_matches_numpy_restatement(pkg, ctx):
    """pmf_fsard_update_A at a realistic shape (40 feature sets x K = 64 over a 3000-column view inside a 5000-column
    model: several column slices per workgroup, sparse S), the ISTA loop entirely on the device, against
    oracle/fsard_oracle.py in float64: A_best, the optimiser's accumulator entry by entry, beta, the best loss and
    epochs_run, within the bounds derived in fsard_ref.py (20 x the float32 restatement's discrepancy)."""
    rng = np.random.default_rng(35)
    K, N, L, c0, c1 = 64, 5000, 40, 1001, 4000
    Nv = c1 - c0 + 1
    S = np.zeros((L, Nv), np.float32)
    for l in range(L):
        idx = rng.choice(Nv, size=60, replace=False)
        S[l, idx] = 1.0 / np.sqrt(60.0)                               # featuresets_to_csc: 1/sqrt(|set|)
    Y = (rng.standard_normal((K, N)) * 0.05).astype(np.float32)
    for k in range(8):
        Y[k, c0 - 1 + np.nonzero(S[3 * k])[0]] += 1.0                  # factor k loads on feature set 3k
    alpha = np.full(Nv, 1.01, np.float32)
    lam = (0.02 + 0.02 * rng.random(K)).astype(np.float32)
    alpha0, v0, lr = 1.01, 0.8, 0.05
    ctx.set_data(np.full((1, N), np.nan, np.float32))
    ctx.set_factors(np.zeros((K, 1), np.float32), Y)
    ctx.clear_yreg()
    ctx.add_yreg_fsard(np.full(N, 1.01, np.float32), np.full((K, N), 0.01, np.float32))
    ssq = np.full((L, K), 1e-8, np.float32)
    A, beta, best, epochs = ctx.fsard_update_A(c0, c1, S, alpha, lam, alpha0, v0, lr, ssq, max_epochs=150, term_iter=30, atol=1e-5)
    Ao = np.zeros((L, K))
    ssqo = np.full((L, K), 1e-8)
    best_o, epochs_o, trace = fo.update_A_inner(Ao, S.astype(np.float64), Y[:, c0 - 1:c1].astype(np.float64),
                                                alpha.astype(np.float64), alpha0, v0, lr, lam.astype(np.float64), ssqo,
                                                max_epochs=150, term_iter=30, atol=1e-5, trace=True)
    # the oracle's loss falls at every epoch, by at least 0.24 against atol = 1e-5: every epoch is "improved by more than
    # atol", A_best is the last iterate and the counter never moves.  (0.24 is 9e-7 of the loss, below fsard_ref.MARGIN:
    # a device loss off by that much would only matter at the last epoch, where it would pick the iterate before.)
    assert all(s["branch"] == "w" for s in trace) and min(s["best"] - s["new"] for s in trace) > 0.2
    assert float(Ao.max()) > 0.05 and epochs >= 30
    got = dict(A=A, ssq=ssq, beta=beta, best=best)
    want = dict(A=Ao, ssq=ssqo, beta=(alpha0 - 1) * (v0 + Ao.T @ S.astype(np.float64)), best=best_o)
    e = fr.errors(got, want, np.full((L, K), 1e-8, np.float32))
    print("FSARD_ERR stages_wide " + " ".join(f"{k}={x:.3e}" for k, x in e.items()) + f" epochs={epochs}/{epochs_o}")
    assert epochs == epochs_o == 150
    for k, x in e.items():
        assert x <= fr.TOL[k], (k, x)
    # ... and the regularizer's device beta took the view's columns (the next epoch's k_reg_step reads it): one
    # Y-regularizer evaluation must equal the closed form with the new beta inside the view and the old one outside
    ctx.set_optimizer("adagrad", lr=1e-6)
    o = ctx.make_opts(update_Y=True)
    ctx.epoch_begin(o)
    ctx.epoch_step_shared(o)
    _, shared = ctx.epoch_loss()
    bfull = np.full((K, N), 0.01)
    bfull[:, c0 - 1:c1] = beta
    want = np.sum((0.5 + 1.01) * np.log1p((0.5 / bfull) * Y.astype(np.float64) ** 2))
    assert abs(shared - want) <= 1e-4 * want, (shared, want)


def test_theta_delta_em_matches_independent_oracle(pkg):
    """theta_delta_em (src/fit.jl:326-375) and its moment estimators (:297-311): the product's EM (device statistics through
    pmf_stats + host updates, pathmatfac.jl_amd/fit.py) against oracle/em_oracle.py, an independent dense-numpy
    restatement of the reference's Julia -- same inputs, both update-prior modes ("EM" and "EB", :466-481)."""
    from oracle import em_oracle
    import test_gpu_host as th
    for update_priors in (True, False):
        model = th.reference_fit_setup(pkg, seed=11)
        rng = np.random.default_rng(12)
        mf = model.matfac
        ct = mf.col_transform
        M, N = model.data.shape
        # a model in the state init_batch_effects! hands to the EM: least-squares theta, delta2 and sigma2 from residual variances
        model.data[rng.random((M, N)) < 0.1] = np.nan
        ct.unwrapped(3).mu[...] = 0.3 * rng.standard_normal(N)
        for v in ct.unwrapped(4).theta.values:
            v[...] = 0.5 * rng.standard_normal(v.shape)
        mf.X[...] = 0.3 * rng.standard_normal(mf.X.shape)
        mf.Y[...] = 0.3 * rng.standard_normal(mf.Y.shape)
        sigma2 = (0.5 + rng.random(N)).astype(np.float64)
        theta_ba = ct.unwrapped(4).theta
        delta2 = [(0.5 + rng.random(v.shape)).astype(np.float64) for v in theta_ba.values]
        views = [dict(start1=cr.start, stop1=cr.stop, batch_of_row=np.asarray(rb), logdelta=ld.copy(), theta=t.copy())
                 for cr, rb, ld, t in zip(theta_ba.col_ranges, theta_ba.row_batches, ct.unwrapped(2).logdelta.values, theta_ba.values)]
        want_theta, want_d2, want_diffs = em_oracle.theta_delta_em(
            model.data, mf.X, mf.Y, ct.unwrapped(1).logsigma, ct.unwrapped(3).mu, views, ["normal"] * N, delta2, sigma2,
            update_priors=update_priors, max_iter=25, rtol=1e-10)
        got_theta, got_d2 = pkg.theta_delta_em(model, [d.copy() for d in delta2], sigma2.copy(), update_priors=update_priors,
                                               batch_em_max_iter=25, batch_em_rtol=1e-10, verbosity=0)
        assert len(want_diffs) >= 5
        for g, w in zip(got_theta, want_theta):
            assert rel_err(g, w) <= 2e-4, rel_err(g, w)
        for g, w in zip(got_d2, want_d2):
            assert rel_err(g, w) <= 2e-4, rel_err(g, w)
        model.release_device()


# ---- bitwise reproducibility of the layer pass and of pmf_stats (no float atomics: private partials + fixed-order sums) ----
@pytest.mark.parametrize("path", ["mfma", "valu"])
@pytest.mark.parametrize("shape", [dict(M=3000, N=700, K=32, n_batches=8), dict(M=1500, N=300, K=100, n_batches=24)])
def test_layer_gradients_and_stats_are_bitwise_reproducible(ctx, monkeypatch, path, shape):
    """grad(theta), grad(logdelta), grad(mu), grad(logsigma) and every output of pmf_stats must be the same BITS run to run, on
    the MFMA layer pass (narrow and wide batch tables) and on the scalar fall-back kernel; theta after a 10-epoch lr = 1 theta
    stage (discrete loss_increase decisions, src/fit.jl:63, 106-122) likewise."""
    from problems import make_problem, to_context
    if path == "valu":
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    p = make_problem(seed=71, bernoulli_frac=0.2, n_views=2, batch_views=2, nan_frac=0.1, weights=True, col_params=True,
                     layer_regs=True, random_init=True, scale=0.5, batch_order="mixed", **shape)
    runs = []
    for _ in range(2):
        to_context(p, ctx)
        ctx.set_optimizer("adagrad", lr=1.0)
        o = ctx.make_opts(update_col_layers=True)
        ctx.epoch_begin(o)
        loss = ctx.epoch_loss()[0]
        assert ctx.last_path()["layer_path"] == (1 if path == "mfma" else 2)
        g = [ctx.get_grad("mu"), ctx.get_grad("logsigma")] + [ctx.get_grad(w, v) for w in ("theta", "logdelta") for v in range(2)]
        st = ctx.stats(use_factors=True)
        r = ctx.fit(update_col_layers=True, frozen_layers=0b0111, max_epochs=10, abs_tol=0, rel_tol=0)
        th = [ctx.get_batch_view(v)[1] for v in range(2)]
        runs.append((loss, g, st, r["loss"], th))
    a, b = runs
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    for k in a[2]:
        if isinstance(a[2][k], (list, tuple)):
            for x, y in zip(a[2][k], b[2][k]):
                np.testing.assert_array_equal(x, y)
        else:
            np.testing.assert_array_equal(a[2][k], b[2][k])
    np.testing.assert_array_equal(a[3], b[3])
    for x, y in zip(a[4], b[4]):
        np.testing.assert_array_equal(x, y)
