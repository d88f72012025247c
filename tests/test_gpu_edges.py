"""Every fused kernel family at its K edges and its panel edges, against the fp64 oracle.

The data pass picks a kernel family and a row-panel height from K, the precision, the gradients wanted and the batch
layers (fused_geometry, csrc/pmf_pass.hip).  Ragged shapes go wrong at the edges of that table: K one above or below a
multiple of 32 (the k-block count KB = ceil(K/32) and its zero padding), a last row panel holding one row or missing most
of its 32-row blocks, and a last column tile that is ragged at 32 or at the 64-column pad of the tiled D.  Each case here
picks M from the panel height BM of the family it must run, pairs it with one N, asserts that family ran, and compares the
loss and the data gradients with the oracle at the tolerances of tests/test_gpu_parity.py: the max-norm at GRAD_TOL and
every element of gX and gY at the rounding of its own terms (factor_gate).  The last section runs every family on operands
whose columns span six decades and whose rows span three (range_problem): the split kernels' operand images hold one such
operand each.

The expected family is restated below from the selection rules, not asked of the library:
    exact f32 kernel (family 0): BM = 512 at K <= 32 without batch layers, 256 at K <= 64 otherwise, 128 at K > 64
    split bf16x3 kernels: K <= 32 -> sb (1, BM 256); 33..64 -> sb8 (8, BM 512) with both gradients, sb2 (2, BM 256)
    otherwise; 65..96 -> sb4 (4, BM 128); 97..128 -> sb8 (8, BM 256) with both gradients, sb4 otherwise.
"""
import numpy as np
import pytest

import hinge_ref
from problems import make_problem, rel_err, to_context, to_oracle
from test_gpu_parity import GRAD_TOL, LOSS_RTOL, factor_gate, grads_of
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

KS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
NS = [1, 33, 95, 161]
GRADS = {"both": dict(update_X=True, update_Y=True), "X": dict(update_X=True), "Y": dict(update_Y=True)}


def expected_family(K, prec, both, batch=False, sb8=True):
    """(kernel family, row-panel height BM) that a pass must run."""
    KB = (K + 31) // 32
    if prec == "f32":
        if KB == 1:
            return 0, 256 if batch else 512
        return 0, 256 if KB == 2 else 128
    if KB == 1:
        return 1, 256
    if KB == 2:
        return (8, 512) if both and sb8 else (2, 256)
    if KB == 3:
        return 4, 128
    return (8, 256) if both and sb8 else (4, 128)


def panel_shapes(BM):
    """(M, N): one row; one row in the last panel; the last panel one row short; two row blocks, the second with one row."""
    return list(zip([1, BM + 1, 2 * BM - 1, BM + 33], NS))


def data_kw(K):
    return dict(col_params=True, weights=True, nan_frac=0.05, scale=0.4 if K > 64 else 1.0)


def run_case(ctx, p, prec, flags, fam):
    """One pass on the session context in precision `prec`; asserts the kernel family, returns (loss, grads)."""
    ctx.set_precision(prec)
    try:
        n0 = ctx.get_precision()[1]
        loss, g = grads_of(ctx, p, **flags)
        assert ctx.last_kernel() == fam, (ctx.last_kernel(), fam)
        assert ctx.get_precision()[1] == n0 + (0 if prec == "f32" else 1), "split-launch count"
    finally:
        ctx.set_precision("f32")
    return loss, g


def check_oracle(ctx, p, loss, g, flags):
    _, go = to_oracle(p).loss_and_grads(**flags)
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6, (loss, go["data_loss"])
    for w in ("X", "Y"):
        if flags.get("update_" + w):
            assert np.isfinite(g[w]).all(), f"non-finite g{w}"
            assert rel_err(g[w], go[w]) <= GRAD_TOL, (w, rel_err(g[w], go[w]))
    factor_gate(ctx, p, g, go)


def _edge_cases():
    out = []
    for K in KS:
        for prec in ("f32", "bf16x3"):
            for gname in GRADS:
                fam, BM = expected_family(K, prec, gname == "both")
                for M, N in panel_shapes(BM):
                    out.append(pytest.param(K, prec, gname, M, N, fam, id=f"k{K}-{prec}-{gname}-m{M}-n{N}"))
    return out


@pytest.mark.parametrize("K,prec,gname,M,N,fam", _edge_cases())
def test_family_edges_match_oracle(ctx, K, prec, gname, M, N, fam):
    p = make_problem(M=M, N=N, K=K, seed=K * 7 + M + N, **data_kw(K))
    to_context(p, ctx)
    loss, g = run_case(ctx, p, prec, GRADS[gname], fam)
    check_oracle(ctx, p, loss, g, GRADS[gname])


@pytest.mark.parametrize("M,N", [pytest.param(M, N, id=f"k128-bf16x3-both-m{M}-n{N}") for M, N in panel_shapes(128)])
def test_k128_both_gradients_without_sb8_runs_sb4(ctx, monkeypatch, M, N):
    """PMF_SB8=0 (read at every pass) sends K = 128 with both gradients to pmf_fused_sb4_kernel's 128-row panel."""
    monkeypatch.setenv("PMF_SB8", "0")
    fam, BM = expected_family(128, "bf16x3", True, sb8=False)
    assert (fam, BM) == (4, 128)
    p = make_problem(M=M, N=N, K=128, seed=M + N, **data_kw(128))
    to_context(p, ctx)
    loss, g = run_case(ctx, p, "bf16x3", GRADS["both"], fam)
    check_oracle(ctx, p, loss, g, GRADS["both"])


def _general_cases():
    out = []
    for K in (32, 33, 64, 65, 96, 97, 128):
        for prec in ("f32", "bf16x3"):
            fam, BM = expected_family(K, prec, True, batch=True)
            out.append(pytest.param(K, prec, BM + 1, 161, fam, id=f"k{K}-{prec}-both-m{BM + 1}-n161"))
    return out


@pytest.mark.parametrize("K,prec,M,N,fam", _general_cases())
def test_general_path_edges_match_oracle(ctx, K, prec, M, N, fam):
    """Bernoulli and Poisson columns and two batch views through the LDS batch table (bmode 1), one row in the last panel."""
    p = make_problem(M=M, N=N, K=K, seed=K + 5, bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2,
                     n_batches=6, col_params=True, weights=True, nan_frac=0.05, scale=0.4)
    to_context(p, ctx)
    loss, g = run_case(ctx, p, prec, GRADS["both"], fam)
    assert ctx.last_path()["bmode"] == 1
    check_oracle(ctx, p, loss, g, GRADS["both"])


def _bf16_store_cases():
    out = []
    for K in (33, 64, 97, 128):
        for prec in ("f32", "bf16x3"):
            fam, BM = expected_family(K, prec, True)
            out.append(pytest.param(K, prec, BM + 33, 95, fam, id=f"k{K}-{prec}-both-m{BM + 33}-n95"))
    return out


@pytest.mark.parametrize("K,prec,M,N,fam", _bf16_store_cases())
def test_bf16_stored_edges_match_oracle_on_the_rounded_matrix(ctx, K, prec, M, N, fam):
    p = make_problem(M=M, N=N, K=K, seed=K + 9, **data_kw(K))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        loss, g = run_case(ctx, p, prec, GRADS["both"], fam)
        check_oracle(ctx, p, loss, g, GRADS["both"])
    finally:
        ctx.set_data(p["D"])            # back to f32 storage for the tests that follow


# ---- heterogeneous operand ranges inside one operand image ----------------------------------------------------------
def range_problem(M, N, K, mixed, seed):
    """Column scales spanning six decades and row norms spanning three, inside one problem.  Starts from make_problem (mixed:
    Bernoulli and Poisson columns and two batch views; plain: Gaussian only) and, with a generator seeded from the case,
    draws c_j = 10^U(-3, 3) on the Gaussian columns (1 elsewhere) and r_i = 10^U(-3, 0) per row; then X[:, i] *= r_i,
    logsigma += log c, mu *= c, theta[:, j] *= c_j, D is drawn again from the fp64 forward at these parameters (noise
    0.1 c_j; Bernoulli 1[z > 0]; Poisson counts of e^clip(z, -5, 3); the same NaN positions) and col_weight /= c^2, so every
    column's residuals weigh alike.  The split kernels' operand images (bf16 hi / mid / lo; sb8's f16 pair under one
    power-of-two pre-scale per operand) hold sigma_j Y and X: both now span their range inside one image."""
    kw = dict(bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2, n_batches=6) if mixed else {}
    p = make_problem(M=M, N=N, K=K, seed=seed, scale=0.4, col_params=True, weights=True, nan_frac=0.05, **kw)
    rng = np.random.default_rng(seed + 1000)
    normal = np.zeros(N, bool)
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        normal[s - 1:e] = kd == "normal"
    c = np.where(normal, 10.0 ** rng.uniform(-3, 3, N), 1.0)
    r = 10.0 ** rng.uniform(-3, 0, M)
    p["X"] = np.asfortranarray((p["X"] * r[None, :]).astype(np.float32))
    p["logsigma"] = (p["logsigma"] + np.log(c)).astype(np.float32)
    p["mu"] = (p["mu"] * c).astype(np.float32)
    for bv in p["batch_views"]:
        bv["theta"] = (bv["theta"] * c[None, bv["start1"] - 1:bv["stop1"]]).astype(np.float32)
    z = hinge_ref.forward(p)[3]
    D = z + 0.1 * c[None, :] * rng.standard_normal((M, N))
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        if kd == "bernoulli":
            D[:, s - 1:e] = z[:, s - 1:e] > 0
        elif kd == "poisson":
            D[:, s - 1:e] = rng.poisson(np.exp(np.clip(z[:, s - 1:e], -5, 3)))
    p["D"] = np.asfortranarray(np.where(np.isnan(p["D"]), np.nan, D).astype(np.float32))
    p["col_weight"] = (p["col_weight"] / c ** 2).astype(np.float32)
    return p


def range_seed(K, mixed):
    return 4000 + K + (500 if mixed else 0)


def _range_cases():
    """(K, precision, gradients, mixed, bf16 store): both gradients at every K block count, precision and problem kind; single
    gradients at K = 64 and 128 (other families on the split path); K = 128 split with D stored as bf16."""
    out = [(K, prec, "both", mixed, False) for K in (32, 64, 96, 128) for prec in ("f32", "bf16x3") for mixed in (True, False)]
    out += [(K, prec, gname, True, False) for K in (64, 128) for prec in ("f32", "bf16x3") for gname in ("X", "Y")]
    out += [(128, "bf16x3", "both", mixed, True) for mixed in (True, False)]
    return [pytest.param(*c, id=f"k{c[0]}-{c[1]}-{c[2]}-{'mixed' if c[3] else 'plain'}{'-bf16store' if c[4] else ''}") for c in out]


@pytest.mark.parametrize("K,prec,gname,mixed,store", _range_cases())
def test_operand_ranges_inside_one_image_match_oracle(ctx, K, prec, gname, mixed, store):
    fam, BM = expected_family(K, prec, gname == "both", batch=mixed)
    p = range_problem(BM + 33, 161, K, mixed, range_seed(K, mixed))
    if store:
        p["D"] = np.asfortranarray(bf16_round(p["D"]))
    to_context(p, ctx)
    if store:
        ctx.set_data(p["D"], store="bf16")
    try:
        loss, g = run_case(ctx, p, prec, GRADS[gname], fam)
        if mixed:
            assert ctx.last_path()["bmode"] == 1
        check_oracle(ctx, p, loss, g, GRADS[gname])
    finally:
        if store:
            ctx.set_data(p["D"])        # back to f32 storage for the tests that follow
