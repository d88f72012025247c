"""The exact f32 kernel's cross-wave GEMM3 (K in 33..64, both gradients: pmf_fused.hip.inc, XW) against the fp64 oracle.

With both gradients the 256-row exact kernel splits grad(Y)'s GEMM over its eight waves by output block: every wave
contracts one 16 x 16 block of the tile's gY over all 256 rows of the panel, reading the G tiles and X panels of all
waves from LDS behind the tile's single barrier, and adds it straight to the workgroup's private gY slab.  What can go
wrong is at the edges of that structure: a panel with one live row or one row short, ragged last column tiles (the
store's clamp), pieces that revisit a slab entry (store on the first visit, accumulate afterwards), the general
epilogues feeding the same G tiles, and the hand-over of LDS buffers between tiles and pieces with one barrier.
PMF_XGEMM3=0 (read at every pass) runs the per-wave-slab path on the same context, for comparison.

Every case runs in f32 and must have taken the exact kernel (family 0).
"""
import numpy as np
import pytest

from problems import factor_scales, make_problem, rel_err, to_context, to_oracle
from test_gpu_parity import FIT_TOL, GRAD_TOL, LOSS_RTOL, factor_gate, grads_of

pytestmark = pytest.mark.gpu

BOTH = dict(update_X=True, update_Y=True)


def eval_both(ctx, p):
    loss, g = grads_of(ctx, p, **BOTH)
    assert ctx.last_kernel() == 0, ctx.last_kernel()
    return loss, g


def check_oracle(ctx, p, go, loss, g, scales=None):
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6, (loss, go["data_loss"])
    for w in ("X", "Y"):
        assert np.isfinite(g[w]).all(), f"non-finite g{w}"
        assert rel_err(g[w], go[w]) <= GRAD_TOL, (w, rel_err(g[w], go[w]))
    factor_gate(ctx, p, g, go, scales=scales)


@pytest.mark.parametrize("M,N", [(1, 1), (257, 33), (511, 95), (289, 161)])
@pytest.mark.parametrize("K", [33, 64])
def test_panel_and_tile_edges_match_oracle(ctx, K, M, N):
    """One live row; a last panel holding one row, or one row short; a second row block with one row; last column tiles
    ragged at 32 and at the 64-column pad."""
    p = make_problem(M=M, N=N, K=K, seed=K * 7 + M + N, col_params=True, weights=True, nan_frac=0.05)
    to_context(p, ctx)
    loss, g = eval_both(ctx, p)
    _, go = to_oracle(p).loss_and_grads(**BOTH)
    check_oracle(ctx, p, go, loss, g)


@pytest.fixture(scope="module")
def walk():
    """9 row panels x 64 column tiles, about 2.25 tiles per workgroup (4.5 with half the CUs reserved): the 8-tile floor
    of the segment length makes ranges straddle row panels inside a segment, so workgroups revisit slab entries,
    including the second piece that covers tiles before the first piece's start.  The oracle's answer is computed once."""
    p = make_problem(M=2049, N=2048, K=64, seed=41, col_params=True, weights=True, nan_frac=0.02)
    _, go = to_oracle(p).loss_and_grads(**BOTH)
    return p, go, factor_scales(p)


@pytest.mark.parametrize("reserve", [None, "128"])
def test_multi_piece_walks_match_oracle_and_repeat_bitwise(ctx, monkeypatch, walk, reserve):
    p, go, scales = walk
    if reserve:
        monkeypatch.setenv("PMF_RESERVE_CUS", reserve)
    to_context(p, ctx)
    l1, g1 = eval_both(ctx, p)
    check_oracle(ctx, p, go, l1, g1, scales)
    l2, g2 = eval_both(ctx, p)
    assert l1 == l2
    assert np.array_equal(g1["X"], g2["X"]) and np.array_equal(g1["Y"], g2["Y"])


def test_general_epilogues_feed_the_cross_wave_gemm(ctx):
    """Bernoulli and Poisson columns and two batch views through the LDS batch table (bmode 1), one row in the last panel."""
    p = make_problem(M=257, N=161, K=64, seed=69, bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2,
                     n_batches=6, col_params=True, weights=True, nan_frac=0.05, scale=0.4)
    to_context(p, ctx)
    loss, g = eval_both(ctx, p)
    assert ctx.last_path()["bmode"] == 1
    _, go = to_oracle(p).loss_and_grads(**BOTH)
    check_oracle(ctx, p, go, loss, g)


@pytest.mark.parametrize("reserve", [None, "128"])
def test_slab_path_and_cross_wave_path_agree(ctx, monkeypatch, walk, reserve):
    """PMF_XGEMM3=0 against the default on one context and one data set.  Nothing on the way to the loss or to gX differs:
    bit-equal.  gY is one 256-term MFMA chain pair per element instead of eight 32-term partials added in wave order:
    f32 re-association, bounded at 1e-5 of the largest entry (an order below GRAD_TOL)."""
    p, go, scales = walk
    if reserve:
        monkeypatch.setenv("PMF_RESERVE_CUS", reserve)
    to_context(p, ctx)
    monkeypatch.setenv("PMF_XGEMM3", "0")
    l_old, g_old = eval_both(ctx, p)
    monkeypatch.delenv("PMF_XGEMM3")
    l_new, g_new = eval_both(ctx, p)
    print(f"gY old vs new rel_err {rel_err(g_new['Y'], g_old['Y']):.3e}; bit-equal entries "
          f"{np.mean(g_new['Y'] == g_old['Y']):.3f}")
    assert l_old == l_new
    assert np.array_equal(g_old["X"], g_new["X"])
    assert not np.array_equal(g_old["Y"], g_new["Y"]), "the switch changed nothing: both passes took one path"
    assert rel_err(g_new["Y"], g_old["Y"]) <= 1e-5, rel_err(g_new["Y"], g_old["Y"])
    check_oracle(ctx, p, go, l_old, g_old, scales)
    check_oracle(ctx, p, go, l_new, g_new, scales)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_fit_trajectory_matches_oracle(ctx, opt):
    p = make_problem(M=600, N=300, K=64, seed=13, random_init=True, col_params=True, weights=True, nan_frac=0.05)
    lr = 0.05 if opt == "adagrad" else 0.01
    to_context(p, ctx)
    ctx.set_optimizer(opt, lr=lr)
    r = ctx.fit(update_X=True, update_Y=True, max_epochs=6, abs_tol=0, rel_tol=0)
    assert ctx.last_kernel() == 0
    m = to_oracle(p)
    ro = m.fit(update_X=True, update_Y=True, opt=opt, lr=lr, max_epochs=6, abs_tol=0, rel_tol=0)
    assert r["term_code"] == ro["term_code"] and r["epochs"] == ro["epochs"]
    np.testing.assert_allclose(r["loss"], ro["loss"], rtol=5e-5)
    X, Y = ctx.get_factors()
    assert rel_err(X, m.X) <= FIT_TOL, rel_err(X, m.X)
    assert rel_err(Y, m.Y) <= FIT_TOL, rel_err(Y, m.Y)
