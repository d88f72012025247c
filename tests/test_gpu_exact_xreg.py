"""The exact f32 kernel with a piece's X operands held in registers (pmf_fused.hip.inc, XR) against the same kernel
reading them from LDS for every tile (PMF_XREG=0, read at every pass).

The cross-wave-GEMM3 instances (K in 33..64, both gradients) multiply every tile of a piece by the same X values: the
forward's B operand (this lane's row, 32 floats) and the GEMM3's A operand (64 floats over the panel's 256 rows).  The
register-resident instances read both once per piece, after the prologue's barrier, and run the same MFMAs in the same
order on the same values, so loss, gX and gY must be BIT-IDENTICAL to the LDS-read instance; only last_path()["xreg"]
tells the two apart.  The one new way to be wrong is a stale fragment: a wave that keeps the previous panel's, or the
previous launch's, X.  Instances that would spill keep the LDS reads: there xreg stays 0.

Every case computes in f32 and must have taken the exact kernel (family 0).
"""
import numpy as np
import pytest

from problems import factor_scales, make_problem, to_context, to_oracle
from test_gpu_exact_xwave import BOTH, check_oracle, eval_both
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu


def eval_pair(ctx, p, monkeypatch, expect_xreg=1):
    """(default pass, PMF_XREG=0 pass) on one context, each as (loss, grads), with the variant that ran asserted."""
    l1, g1 = eval_both(ctx, p)
    assert ctx.last_path()["xreg"] == expect_xreg, ctx.last_path()
    monkeypatch.setenv("PMF_XREG", "0")
    l0, g0 = eval_both(ctx, p)
    assert ctx.last_path()["xreg"] == 0, ctx.last_path()
    monkeypatch.delenv("PMF_XREG")
    return (l1, g1), (l0, g0)


def assert_bit_equal(a, b):
    (la, ga), (lb, gb) = a, b
    assert la == lb, (la, lb)
    assert np.array_equal(ga["X"], gb["X"]), float(np.abs(ga["X"] - gb["X"]).max())
    assert np.array_equal(ga["Y"], gb["Y"]), float(np.abs(ga["Y"] - gb["Y"]).max())


@pytest.mark.parametrize("M,N,K", [(1, 1, 33), (257, 33, 64), (511, 95, 48), (289, 161, 64)])
def test_panel_and_tile_edges_are_bit_equal(ctx, monkeypatch, M, N, K):
    """One live row; a last panel holding one row, or one row short; a second row block with one row; ragged last column
    tiles; K below and at the padded 64."""
    p = make_problem(M=M, N=N, K=K, seed=K * 5 + M + N, col_params=True, weights=True, nan_frac=0.05)
    to_context(p, ctx)
    new, old = eval_pair(ctx, p, monkeypatch)
    assert np.isfinite(new[1]["X"]).all() and np.isfinite(new[1]["Y"]).all()
    assert_bit_equal(new, old)


@pytest.fixture(scope="module")
def walk():
    """The walk of test_gpu_exact_xwave.py: 9 row panels x 64 column tiles, ranges that cross row panels inside a segment,
    so a workgroup runs several pieces with different X panels in one launch.  The oracle's answer is computed once."""
    p = make_problem(M=2049, N=2048, K=64, seed=43, col_params=True, weights=True, nan_frac=0.02)
    _, go = to_oracle(p).loss_and_grads(**BOTH)
    return p, go, factor_scales(p)


@pytest.mark.parametrize("reserve", [None, "128"])
def test_no_stale_fragments_across_pieces(ctx, monkeypatch, walk, reserve):
    p, go, scales = walk
    if reserve:
        monkeypatch.setenv("PMF_RESERVE_CUS", reserve)
    to_context(p, ctx)
    new, old = eval_pair(ctx, p, monkeypatch)
    assert_bit_equal(new, old)
    check_oracle(ctx, p, go, new[0], new[1], scales)
    again = eval_both(ctx, p)
    assert ctx.last_path()["xreg"] == 1
    assert_bit_equal(new, again)


def test_no_fragment_survives_a_launch(ctx, monkeypatch):
    """Same context and data, new factors: the second launch must multiply by the new X."""
    p = make_problem(M=511, N=161, K=64, seed=77, col_params=True, weights=True, nan_frac=0.05)
    to_context(p, ctx)
    first, _ = eval_pair(ctx, p, monkeypatch)
    rng = np.random.default_rng(78)
    X2 = (p["X"] + rng.standard_normal(p["X"].shape) * 0.5).astype(np.float32)
    ctx.set_factors(X2, p["Y"])
    new, old = eval_pair(ctx, p, monkeypatch)
    assert_bit_equal(new, old)
    assert not np.array_equal(new[1]["Y"], first[1]["Y"]), "the new X changed nothing"


def test_general_epilogue_instance(ctx, monkeypatch):
    """Bernoulli and Poisson columns and two batch views through the LDS batch table (bmode 1).  That instance starts from
    235 VGPRs and would spill with the fragments in registers: it keeps the LDS reads, and says so."""
    p = make_problem(M=257, N=161, K=64, seed=69, bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2,
                     n_batches=6, col_params=True, weights=True, nan_frac=0.05, scale=0.4)
    to_context(p, ctx)
    new, old = eval_pair(ctx, p, monkeypatch, expect_xreg=0)
    assert ctx.last_path()["bmode"] == 1
    assert_bit_equal(new, old)


@pytest.mark.parametrize("order,bmode,M,N", [("sorted", 1, 2100, 230), ("random", 2, 1000, 130)])
def test_bf16_stored_mixed_batch_instances_match_oracle(ctx, monkeypatch, order, bmode, M, N):
    """The two cross-wave instances at the register limit (D stored as bf16, mixed noise models, batch layers through the
    LDS table or the gathers): they trade the pinned addressing for recomputed addresses to stay out of scratch, keep
    the LDS reads of X, and must compute what the oracle computes on the rounded matrix."""
    p = make_problem(M=M, N=N, K=64, seed=91, n_views=3, batch_views=2, n_batches=40, batch_order=order, nan_frac=0.05,
                     weights=True, col_params=True, bernoulli_frac=0.2, poisson_frac=0.1, scale=0.5)
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        new, old = eval_pair(ctx, p, monkeypatch, expect_xreg=0)
        assert ctx.last_path()["bmode"] == bmode, ctx.last_path()
        assert_bit_equal(new, old)
        m = to_oracle(p)
        m.m.n_xreg = 0
        m.m.n_yreg = 0
        _, go = m.loss_and_grads(**BOTH)
        check_oracle(ctx, p, go, new[0], new[1])
    finally:
        ctx.set_data(p["D"])            # back to f32 storage for the tests that follow


def test_fit_trajectory_is_bit_equal(ctx, monkeypatch):
    p = make_problem(M=600, N=300, K=64, seed=13, random_init=True, col_params=True, weights=True, nan_frac=0.05)
    traces = []
    for switch in (None, "0"):
        if switch is not None:
            monkeypatch.setenv("PMF_XREG", switch)
        to_context(p, ctx)
        ctx.set_optimizer("adam", lr=0.01)
        r = ctx.fit(update_X=True, update_Y=True, max_epochs=6, abs_tol=0, rel_tol=0)
        assert ctx.last_kernel() == 0 and ctx.last_path()["xreg"] == (1 if switch is None else 0), ctx.last_path()
        traces.append((np.asarray(r["loss"], dtype=np.float64), *ctx.get_factors()))
    assert len(traces[0][0]) >= 6, traces[0][0]
    assert np.array_equal(traces[0][0], traces[1][0]), (traces[0][0], traces[1][0])
    assert np.array_equal(traces[0][1], traces[1][1]) and np.array_equal(traces[0][2], traces[1][2])
