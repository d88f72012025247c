"""GPU parity tests: the HIP path (through the C ABI, include/pmf_hip.h) against the fp64 CPU oracle on the
same seeded inputs, plus the reference's known-answer vectors and size-independent properties at full size.

Tolerances (north-star: "within a stated fp32 tolerance"): the HIP path computes in fp32 (exact-f32 MFMA, f32
elementwise; every sum in a fixed order -- private per-workgroup gY slabs and per-piece gX slots reduced by k_gy_reduce /
k_gx_reduce, fixed-order loss partials: the library has no float atomics); against the fp64 oracle we require
    loss            : relative 2e-5
    gradients       : max-abs error <= 2e-4 * max|gradient|   (K <= 128 f32 dot products, a few thousand f32 adds)
                      and, per element of gX and gY, |error| <= FACTOR_TAU * (the sum of the magnitudes of that element's
                      own terms): problems.factor_check through factor_gate below
    fitted factors  : max-abs error <= 2e-3 * max|param| after 10 epochs (error compounds through AdaGrad)
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest

from problems import factor_check, factor_scales, factor_worst, make_problem, rel_err, to_context, to_oracle

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"

LOSS_RTOL = 2e-5
GRAD_TOL = 2e-4
FIT_TOL = 2e-3


def grads_of(ctx, p, **flags):
    o = ctx.make_opts(**flags)
    ctx.epoch_begin(o)
    loss, _ = ctx.epoch_loss()
    g = {}
    if flags.get("update_X"):
        g["X"] = ctx.get_grad("X")
    if flags.get("update_Y"):
        g["Y"] = ctx.get_grad("Y")
    if flags.get("update_col_layers"):
        g["mu"] = ctx.get_grad("mu")
        g["logsigma"] = ctx.get_grad("logsigma")
        g["theta"] = [ctx.get_grad("theta", v) for v in range(len(p["batch_views"]))]
        g["logdelta"] = [ctx.get_grad("logdelta", v) for v in range(len(p["batch_views"]))]
    return loss, g


def factor_gate(ctx, p, g, want, scales=None, tag=""):
    """The per-element check of the factor gradients in `g` (problems.factor_check at FACTOR_TAU) against `want`, the fp64
    reference of problem `p`: prints one FACTOR_CHECK line with the kernel family of the context's last pass and the worst
    ratio of each gradient, and fails above 1 naming the worst element.  ctx: the context, or the family itself where the
    context is gone; scales: factor_scales(p) where a caller shares them between passes."""
    s = factor_scales(p) if scales is None else scales
    worst = factor_check(p, g, want, scales=s)
    tid = os.environ.get("PYTEST_CURRENT_TEST", "-").split(" ")[0] + tag
    print(f"FACTOR_CHECK {tid} family={ctx if isinstance(ctx, int) else ctx.last_kernel()} " +
          " ".join(f"{w}={worst[w]:.4f}" if w in worst else f"{w}=-" for w in ("X", "Y")))
    assert worst and max(worst.values()) <= 1.0, factor_worst(p, g, want, scales=s)
    return worst


def test_batch_array_known_answers_on_device(ctx):
    """runtests.jl:203-209, 234-235: A + ba and ones * exp(ba) through the device forward (BatchShift / BatchScale)."""
    g = json.loads((GOLD / "batch_array_5x7.json").read_text())
    cr = g["ctor"]["col_ranges"]
    rb = [np.argmax(np.array(m), axis=1).astype(np.int32) for m in g["ctor"]["row_batches"]]
    vals = [np.array(v, dtype=np.float32) for v in g["ctor"]["values"]]
    M, N = 5, 7
    ctx.set_data(np.zeros((M, N), np.float32))
    # X'Y = 0  ->  Z = theta expansion
    ctx.set_factors(np.zeros((N, M), np.float32), np.eye(N, dtype=np.float32))
    ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
    ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=b, logdelta=np.zeros_like(v), theta=v)
                         for (s, e), b, v in zip(cr, rb, vals)])
    np.testing.assert_array_equal(ctx.forward(), np.array(g["add"]["Z"], dtype=np.float32))
    # X'Y = ones -> Z = exp(logdelta) expansion
    ctx.set_factors(np.ones((N, M), np.float32) / N, np.ones((N, N), np.float32))
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=b, logdelta=v, theta=np.zeros_like(v))
                         for (s, e), b, v in zip(cr, rb, vals)])
    np.testing.assert_allclose(ctx.forward(), np.array(g["exp"]["Z"]), rtol=3e-6)
    # gradient of sum(x + y): theta_bar = rows per batch (runtests.jl:210-215) through the layer-gradient kernel
    ctx.set_factors(np.zeros((N, M), np.float32), np.eye(N, dtype=np.float32))
    ctx.set_batch_views([dict(start1=s, stop1=e, batch_of_row=b, logdelta=np.zeros_like(v), theta=v)
                         for (s, e), b, v in zip(cr, rb, vals)])
    ctx.set_data((np.array(g["add"]["Z"]) - 1.0).astype(np.float32))   # dloss/dZ = 1
    o = ctx.make_opts(update_col_layers=True)
    ctx.epoch_begin(o)
    ctx.epoch_loss()
    for v, want in enumerate(g["add"]["ba_grad_values"]):
        np.testing.assert_allclose(ctx.get_grad("theta", v), np.array(want), atol=1e-5)


CASES = {
    # config 1 of BASELINE.json: 500x200 Gaussian-only, K=4, no pathway reg
    "c1_500x200_k4": dict(M=500, N=200, K=4, xreg="l2"),
    "ragged_k32": dict(M=301, N=143, K=32, yreg="fsard", xreg="group", weights=True, col_params=True),
    "ragged_k64_nan": dict(M=777, N=333, K=64, yreg="fsard", xreg="l2", nan_frac=0.1, weights=True, col_params=True),
    "k10_pad": dict(M=260, N=70, K=10, yreg="ard", n_views=2, col_params=True),
    "k100_4wave": dict(M=200, N=150, K=100, yreg="group", xreg="l2", col_params=True),
    "k128_4wave": dict(M=140, N=65, K=128, nan_frac=0.05, col_params=True),
    # config 3 flavour: mixed Gaussian/Bernoulli + BatchArray shift/scale + NaN mask
    "mixed_batch_nan": dict(M=420, N=260, K=32, bernoulli_frac=0.2, n_views=2, batch_views=2, n_batches=8,
                            nan_frac=0.1, weights=True, col_params=True, xreg="composite", yreg="fsard"),
    "poisson_batch": dict(M=150, N=90, K=8, poisson_frac=0.3, bernoulli_frac=0.2, n_views=3, batch_views=2,
                          weights=True, col_params=True, scale=0.4),
    # more than 15 batches in a view: the fused kernel falls back from the LDS-staged dense batch table to global gathers
    "batch_20_batches": dict(M=300, N=100, K=16, n_views=2, batch_views=2, n_batches=20, nan_frac=0.05, weights=True,
                             col_params=True, bernoulli_frac=0.3),
    "tiny": dict(M=5, N=7, K=2),
    "one_row_panel_many_cols": dict(M=33, N=1500, K=16, nan_frac=0.02),
    # more work units than workgroups: a workgroup visits several row panels of one column segment (its private gY
    # slab accumulates by read-modify-write) and some workgroups cross a segment boundary; no missing values, so
    # interior tiles take the packed-math epilogue
    "many_panels_two_segments": dict(M=70000, N=600, K=8, xreg="l2", weights=True, col_params=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_loss_and_factor_gradients_match_oracle(ctx, name):
    p = make_problem(seed=11, **CASES[name])
    to_context(p, ctx)
    loss, g = grads_of(ctx, p, update_X=True, update_Y=True)
    lo, go = to_oracle(p).loss_and_grads(update_X=True, update_Y=True)
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6, (loss, go["data_loss"])
    # regularizer gradients are added in the step kernel; epoch_begin exposes the data gradients
    m = to_oracle(p)
    m.m.n_xreg = 0
    m.m.n_yreg = 0
    _, gd = m.loss_and_grads(update_X=True, update_Y=True)
    assert rel_err(g["X"], gd["X"]) <= GRAD_TOL, rel_err(g["X"], gd["X"])
    assert rel_err(g["Y"], gd["Y"]) <= GRAD_TOL, rel_err(g["Y"], gd["Y"])
    factor_gate(ctx, p, g, gd)


@pytest.mark.parametrize("which", ["X", "Y"])
@pytest.mark.parametrize("name", ["ragged_k64_nan", "mixed_batch_nan", "k100_4wave", "c1_500x200_k4"])
def test_single_factor_gradient_matches_oracle(ctx, name, which):
    """grad(X)-only launches (transform: Y fixed, transform.jl) and grad(Y)-only launches are separate compile-time
    variants of the fused kernel (no GEMM3 / no GEMM2): each against the oracle."""
    p = make_problem(seed=13, **CASES[name])
    to_context(p, ctx)
    flags = dict(update_X=which == "X", update_Y=which == "Y")
    loss, g = grads_of(ctx, p, **flags)
    m = to_oracle(p)
    m.m.n_xreg = 0
    m.m.n_yreg = 0
    _, go = m.loss_and_grads(**flags)
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6
    assert rel_err(g[which], go[which]) <= GRAD_TOL
    factor_gate(ctx, p, g, go)


@pytest.mark.parametrize("name", ["mixed_batch_nan", "poisson_batch", "ragged_k32"])
def test_layer_gradients_match_oracle(ctx, name):
    kw = dict(CASES[name])
    kw["layer_regs"] = True
    p = make_problem(seed=12, **kw)
    to_context(p, ctx)
    loss, g = grads_of(ctx, p, update_col_layers=True)
    m = to_oracle(p)
    m.m.has_colreg = 0
    m.m.has_batchreg = 0
    lo, go = m.loss_and_grads(update_col_layers=True)
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"])
    assert rel_err(g["mu"], go["mu"]) <= GRAD_TOL
    assert rel_err(g["logsigma"], go["logsigma"]) <= GRAD_TOL
    for v in range(len(p["batch_views"])):
        assert rel_err(g["theta"][v], go["theta"][v]) <= GRAD_TOL
        assert rel_err(g["logdelta"][v], go["logdelta"][v]) <= GRAD_TOL


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("name", ["c1_500x200_k4", "ragged_k64_nan", "mixed_batch_nan"])
def test_fit_trajectory_matches_oracle(ctx, name, opt):
    p = make_problem(seed=13, random_init=True, **CASES[name])
    lr = 0.05 if opt == "adagrad" else 0.01
    to_context(p, ctx)
    ctx.set_optimizer(opt, lr=lr)
    r = ctx.fit(update_X=True, update_Y=True, max_epochs=10, abs_tol=0, rel_tol=0)
    m = to_oracle(p)
    ro = m.fit(update_X=True, update_Y=True, opt=opt, lr=lr, max_epochs=10, abs_tol=0, rel_tol=0)
    assert r["term_code"] == ro["term_code"] and r["epochs"] == ro["epochs"]
    np.testing.assert_allclose(r["loss"], ro["loss"], rtol=5e-5)
    X, Y = ctx.get_factors()
    assert rel_err(X, m.X) <= FIT_TOL, rel_err(X, m.X)
    assert rel_err(Y, m.Y) <= FIT_TOL, rel_err(Y, m.Y)


def test_theta_stage_fit_matches_oracle(ctx):
    """init_theta! (fit.jl:106-122): layers 1:3 frozen, only BatchShift trained, no X/Y update."""
    p = make_problem(seed=14, **dict(CASES["mixed_batch_nan"], layer_regs=True))
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=1.0)
    kw = dict(update_col_layers=True, frozen_layers=0b0111, max_epochs=8, abs_tol=0, rel_tol=0)
    r = ctx.fit(**kw)
    m = to_oracle(p)
    ro = m.fit(lr=1.0, **kw)
    np.testing.assert_allclose(r["loss"], ro["loss"], rtol=5e-5)
    for v in range(len(p["batch_views"])):
        ld, th = ctx.get_batch_view(v)
        # lr = 1 AdaGrad: the first step is ~sign(g), which amplifies the f32 error of small gradients
        assert rel_err(th, m.theta[v]) <= 3 * FIT_TOL
        np.testing.assert_array_equal(ld, p["batch_views"][v]["logdelta"])   # frozen layer untouched
    ls, mu = ctx.get_col_params()
    np.testing.assert_array_equal(mu, p["mu"])


def test_all_layers_fit_on_a_wide_matrix_matches_oracle(ctx):
    """Every column layer trained at once on 40000 columns x 8 batches: the four layer parameters share one slab of
    loss partials in the step kernel (320000-entry batch arrays once overflowed it)."""
    p = make_problem(seed=15, M=70, N=40000, K=4, n_views=1, batch_views=1, n_batches=8, col_params=True,
                     layer_regs=True, nan_frac=0.02)
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=0.1)
    kw = dict(update_col_layers=True, max_epochs=4, abs_tol=0, rel_tol=0)
    r = ctx.fit(**kw)
    m = to_oracle(p)
    ro = m.fit(lr=0.1, **kw)
    assert r["term_code"] == ro["term_code"]
    np.testing.assert_allclose(r["loss"], ro["loss"], rtol=5e-5)
    ld, th = ctx.get_batch_view(0)
    # ~9 rows per batch: some batch-parameter gradients are near zero and AdaGrad's first steps, g / sqrt(sum g^2), turn
    # their f32 rounding into O(lr) differences (the gradients themselves are compared in
    # test_layer_gradients_match_oracle; the loss trace above agrees to 5e-5 over all four epochs).  Require the bulk
    # of the 320000 entries to agree tightly and bound the rest by two steps.
    for got, ref in ((th, m.theta[0]), (ld, m.logdelta[0])):
        err = np.abs(got - ref) / np.abs(ref).max()
        assert np.mean(err > 3 * FIT_TOL) < 2e-3, np.mean(err > 3 * FIT_TOL)
        assert err.max() <= 2 * 0.1 / np.abs(ref).max() + FIT_TOL
    ls, mu = ctx.get_col_params()
    assert rel_err(mu, m.mu) <= FIT_TOL


def test_transform_mode_updates_only_X(ctx):
    """transform (transform.jl:61-90): Y and layers constant, no regularizers, X starts at 0."""
    p = make_problem(seed=15, M=130, N=90, K=6, col_params=True, weights=True, nan_frac=0.2)
    p["X"] = np.zeros_like(p["X"])
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=1.0)
    r = ctx.fit(update_X=True, max_epochs=15, abs_tol=0, rel_tol=0)
    m = to_oracle(p)
    ro = m.fit(update_X=True, lr=1.0, max_epochs=15, abs_tol=0, rel_tol=0)
    np.testing.assert_allclose(r["loss"], ro["loss"], rtol=5e-5)
    X, Y = ctx.get_factors()
    np.testing.assert_array_equal(Y, p["Y"])
    assert rel_err(X, m.X) <= FIT_TOL


def test_loss_increase_and_lr_resume(ctx):
    p = make_problem(seed=16, M=200, N=120, K=5, random_init=True, xreg="l2")
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=50.0)
    r = ctx.fit(update_X=True, update_Y=True, max_epochs=50, abs_tol=0, rel_tol=0)
    m = to_oracle(p)
    ro = m.fit(update_X=True, update_Y=True, lr=50.0, max_epochs=50, abs_tol=0, rel_tol=0)
    assert r["term_code"] == "loss_increase" == ro["term_code"]
    assert r["epochs"] == ro["epochs"]
    # fit.jl:64-69: halve eta, resume from h["epochs"], optimizer state kept
    ctx.set_lr(ctx.get_lr() * 0.5)
    assert ctx.get_lr() == 25.0
    r2 = ctx.fit(update_X=True, update_Y=True, max_epochs=50, epoch=r["epochs"], abs_tol=0, rel_tol=0)
    assert r2["epochs"] >= r["epochs"]


def test_gaussian_gradient_is_linear_in_data_at_full_size(ctx):
    """Size-independent property at BASELINE config 2 size (20k x 10k, K=32): for the Gaussian loss the data
    gradient is affine in D, so g(D1) + g(D2) - g(0) == g(D1 + D2); and the loss equals 0.5*sum w (Z-D)^2 with
    Z from the independent (non-MFMA) device forward on a row subset."""
    M, N, K = 20000, 10000, 32
    rng = np.random.default_rng(17)
    X = (rng.standard_normal((K, M)) * 0.3).astype(np.float32)
    Y = (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    D1 = rng.standard_normal((M, N), dtype=np.float32)
    D2 = rng.standard_normal((M, N), dtype=np.float32)
    w = (0.5 + rng.random(N)).astype(np.float32)

    def run(D):
        ctx.set_data(np.asfortranarray(D))
        ctx.set_factors(X, Y)
        ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
        ctx.set_batch_views([])
        ctx.set_noise([(1, N)], ["normal"], w)
        o = ctx.make_opts(update_X=True, update_Y=True)
        ctx.epoch_begin(o)
        loss, _ = ctx.epoch_loss()
        return loss, ctx.get_grad("X"), ctx.get_grad("Y")

    l1, gx1, gy1 = run(D1)
    l2, gx2, gy2 = run(D2)
    l0, gx0, gy0 = run(np.zeros((M, N), np.float32))
    l12, gx12, gy12 = run(D1 + D2)
    assert rel_err(gx1 + gx2 - gx0, gx12) <= 1e-4
    assert rel_err(gy1 + gy2 - gy0, gy12) <= 1e-4
    # closed form of the loss on the full matrix in fp64 from X, Y (chunked to bound host memory)
    tot = 0.0
    Yd = Y.astype(np.float64)
    for i0 in range(0, M, 2000):
        Z = X[:, i0:i0 + 2000].astype(np.float64).T @ Yd
        tot += 0.5 * np.sum(w[None, :] * (Z - D1[i0:i0 + 2000]) ** 2)
    assert abs(l1 - tot) <= LOSS_RTOL * tot
    # gradient closed form on a row subset: gX[:, i] = Y * (w .* (Z_i - D_i))
    rows = rng.choice(M, 64, replace=False)
    Zr = X[:, rows].astype(np.float64).T @ Yd
    gxr = Yd @ (w[None, :] * (Zr - D1[rows])).T
    assert rel_err(gx1[:, rows], gxr) <= GRAD_TOL


def test_all_finite_tiles_and_masked_tiles_agree_with_oracle(ctx):
    """The fused kernel has two epilogues: packed math on 32x32 tiles whose entries are all finite (flag computed
    when D is laid out) and the general masked path elsewhere.  A matrix with a handful of NaN / Inf entries
    exercises both in one launch; non-finite entries contribute no loss and no gradient (transform.jl:55-57)."""
    p = make_problem(seed=21, M=300, N=200, K=16, weights=True, col_params=True)
    D = p["D"].copy()
    assert np.isfinite(D).all()
    for (i, j, v) in [(3, 5, np.nan), (40, 70, np.inf), (41, 70, -np.inf), (299, 199, np.nan), (130, 33, np.nan)]:
        D[i, j] = v
    p["D"] = D
    to_context(p, ctx)
    loss, g = grads_of(ctx, p, update_X=True, update_Y=True)
    m = to_oracle(p)
    m.m.n_xreg = 0
    m.m.n_yreg = 0
    _, go = m.loss_and_grads(update_X=True, update_Y=True)
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"])
    assert rel_err(g["X"], go["X"]) <= GRAD_TOL
    assert rel_err(g["Y"], go["Y"]) <= GRAD_TOL
    factor_gate(ctx, p, g, go, tag=":masked")
    # changing D must refresh the tile flags: make every entry finite again and compare once more
    p["D"] = np.where(np.isfinite(D), D, 0.25).astype(np.float32)
    to_context(p, ctx)
    loss2, g2 = grads_of(ctx, p, update_X=True, update_Y=True)
    m2 = to_oracle(p)
    m2.m.n_xreg = 0
    m2.m.n_yreg = 0
    _, go2 = m2.loss_and_grads(update_X=True, update_Y=True)
    assert abs(loss2 - go2["data_loss"]) <= LOSS_RTOL * abs(go2["data_loss"])
    assert rel_err(g2["Y"], go2["Y"]) <= GRAD_TOL
    factor_gate(ctx, p, g2, go2, tag=":all-finite")


def test_loss_and_grad_Y_are_bitwise_reproducible(ctx):
    """grad(Y) and the loss are summed in a fixed order (private per-workgroup slabs + k_gy_reduce, fixed-order loss
    partials): two evaluations at the same parameters give identical bits, so `loss_increase` decisions
    (src/fit.jl:63) do not depend on scheduling."""
    p = make_problem(seed=22, M=3000, N=700, K=64, nan_frac=0.01, weights=True, col_params=True)
    to_context(p, ctx)
    l1, g1 = grads_of(ctx, p, update_X=True, update_Y=True)
    l2, g2 = grads_of(ctx, p, update_X=True, update_Y=True)
    assert l1 == l2
    assert np.array_equal(g1["Y"], g2["Y"])
    assert np.array_equal(g1["X"], g2["X"])          # gX: per-piece slots + fixed-order k_gx_reduce


def test_headline_size_loss_and_gradient_consistency(ctx):
    """BASELINE.json's headline configuration (200000 x 50000, K = 64), data generated on the device with 0.1 % missing
    entries.  Size-independent properties:
      * the fused kernel's loss equals 0.5 * sum_j w_j * (column sums of squared residuals) from the independent,
        non-MFMA statistics kernel (pmf_stats);
      * the gradient is the gradient OF THAT LOSS: for p(e) = p - e*g, (L(0) - L(e)) / (e |g|^2) = 1 - c*e for the
        (quadratic in each factor) Gaussian loss, so the Richardson combination 2 r(e/2) - r(e) equals 1;
      * loss and grad(Y) are bitwise reproducible at this size too."""
    M, N, K = 200000, 50000, 64
    rng = np.random.default_rng(5)
    Xt = (rng.standard_normal((K, M)) * 0.3).astype(np.float32)
    Yt = (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    X0 = (Xt + 0.05 * rng.standard_normal((K, M))).astype(np.float32)
    Y0 = (Yt + 0.05 * rng.standard_normal((K, N))).astype(np.float32)
    w = (0.5 + rng.random(N)).astype(np.float32)
    ctx.set_data_device(None, M, N)
    ctx.set_factors(Xt, Yt)
    ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
    ctx.set_batch_views([])
    ctx.set_noise([(1, N)], ["normal"], w)
    ctx.clear_xreg()
    ctx.clear_yreg()
    ctx.synth_data(seed=99, noise=0.1, frac_nan=0.001)
    o = ctx.make_opts(update_X=True, update_Y=True)

    def loss_grad(X, Y, want_grad=True):
        ctx.set_factors(X, Y)
        ctx.epoch_begin(o)
        loss, _ = ctx.epoch_loss()
        return (loss, ctx.get_grad("X"), ctx.get_grad("Y")) if want_grad else loss

    L0, gX, gY = loss_grad(X0, Y0)
    L0b, gXb, gYb = loss_grad(X0, Y0)
    assert L0 == L0b and np.array_equal(gY, gYb)
    st = ctx.stats(use_factors=True)
    n_obs = float(st["n"].astype(np.float64).sum())
    assert abs(n_obs / (M * N) - 0.999) < 2e-4                       # the mask is live at this size
    L_stats = 0.5 * float(np.sum(w.astype(np.float64) * st["sqerr"].astype(np.float64)))
    assert abs(L0 - L_stats) <= 5e-5 * L_stats, (L0, L_stats)        # sqerr is accumulated in f32 per column
    g2 = float(np.sum(gX.astype(np.float64) ** 2) + np.sum(gY.astype(np.float64) ** 2))
    e = 0.02 * L0 / g2                                               # ~2 % first-order decrease
    r = []
    for ee in (e, 0.5 * e):
        Le = loss_grad((X0 - ee * gX).astype(np.float32), (Y0 - ee * gY).astype(np.float32), want_grad=False)
        r.append((L0 - Le) / (ee * g2))
    assert 0.5 < r[0] < 1.0 and r[0] < r[1] < 1.0, r
    assert abs(2 * r[1] - r[0] - 1.0) <= 5e-3, r


@pytest.mark.parametrize("K", [16, 64])
def test_blocks_of_missing_samples_match_oracle(ctx, K):
    """Multi-omic matrices have samples that lack a whole assay: 32 x 32 tiles with no observed entry next to partially
    and fully observed ones (packed and masked epilogues in one launch).  Loss and both gradients against the oracle,
    and a short fit.  (Skipping the arithmetic of unobserved tiles was built and measured: +3 % on the fully observed
    headline workload from the extra control flow, so it is not in the kernel)"""
    p = make_problem(seed=31, M=700, N=420, K=K, weights=True, col_params=True, xreg="l2", yreg="fsard")
    D = p["D"].copy()
    D[64:192, 32:200] = np.nan          # whole tiles (rows 64..191 x columns 32..199 cover tiles exactly and partially)
    D[300:333, :] = np.nan              # a band of samples with nothing observed
    D[:, 400:420] = np.nan              # an assay nobody has
    D[500:520, 250:260] = np.nan        # a small hole inside observed tiles
    p["D"] = D
    to_context(p, ctx)
    loss, g = grads_of(ctx, p, update_X=True, update_Y=True)
    m = to_oracle(p)
    m.m.n_xreg = 0
    m.m.n_yreg = 0
    _, go = m.loss_and_grads(update_X=True, update_Y=True)
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"])
    assert rel_err(g["X"], go["X"]) <= GRAD_TOL
    assert rel_err(g["Y"], go["Y"]) <= GRAD_TOL
    factor_gate(ctx, p, g, go)
    assert np.all(g["X"][:, 300:333] == 0.0)                      # unobserved samples get no data gradient
    to_context(p, ctx)
    ctx.set_optimizer("adagrad", lr=0.05)
    r = ctx.fit(update_X=True, update_Y=True, max_epochs=6, abs_tol=0, rel_tol=0)
    ro = to_oracle(p).fit(update_X=True, update_Y=True, lr=0.05, max_epochs=6, abs_tol=0, rel_tol=0)
    np.testing.assert_allclose(r["loss"], ro["loss"], rtol=5e-5)


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("K", [64, 128])
def test_multi_rank_grid_with_reserved_cus_matches_oracle(ctx, monkeypatch, precision, K):
    """With more than one rank the data pass leaves 4 CUs to RCCL: a 252-workgroup grid, not a multiple of the 8 XCDs
    (pmf_xcd_wg's uneven case).  PMF_RESERVE_CUS=4 runs that grid on one rank: loss and gradients against the oracle, exact
    and split kernels."""
    p = make_problem(seed=23, M=700, N=3000, K=K, nan_frac=0.03, weights=True, col_params=True, xreg="l2", yreg="fsard")
    monkeypatch.setenv("PMF_RESERVE_CUS", "4")
    ctx.set_precision(precision)
    try:
        to_context(p, ctx)
        n0 = ctx.get_precision()[1]
        loss, g = grads_of(ctx, p, update_X=True, update_Y=True)
        took_split = ctx.get_precision()[1] > n0
    finally:
        ctx.set_precision("f32")
    assert took_split == (precision == "bf16x3")
    m = to_oracle(p)
    m.m.n_xreg = 0
    m.m.n_yreg = 0
    _, gd = m.loss_and_grads(update_X=True, update_Y=True)
    assert abs(loss - gd["data_loss"]) <= LOSS_RTOL * abs(gd["data_loss"]) + 1e-6
    assert rel_err(g["X"], gd["X"]) <= GRAD_TOL and rel_err(g["Y"], gd["Y"]) <= GRAD_TOL, (rel_err(g["X"], gd["X"]), rel_err(g["Y"], gd["Y"]))
    factor_gate(ctx, p, g, gd)
