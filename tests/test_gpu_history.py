"""A pass must not depend on what ran before it on the context.

The library keeps device buffers from one pass to the next and only grows them (split-operand images, private gY slabs, gX
partial slots, tile flags, panel slots, cached work splits, the sb8 pre-scale slots); a new data shape frees the factors
but none of these.  Results are bitwise reproducible (no float atomic), so a target problem run on a
context that has first been through a poison history -- larger shapes, other kernel families, both storage types, NaN X,
infinite Y columns, NaN data, failed fits -- must give exactly the bits it gives on a fresh context, and still match the
oracle.  Only float values are poisoned: indices, ranges and sizes are validated inputs.
"""
import numpy as np
import pytest

from problems import layer_check, make_problem, rel_err, to_context, to_oracle
from test_gpu_parity import GRAD_TOL, LOSS_RTOL, grads_of
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

BOTH = dict(update_X=True, update_Y=True)
BATCH = dict(n_views=2, batch_views=2, n_batches=6, bernoulli_frac=0.2)

# name: precision, K, M, N, gradient flags, kernel family that must run (None: layer pass), extra problem arguments.
# Every M leaves a ragged last row panel and every N a ragged last column tile.
TARGETS = {
    "exact_1x2": ("f32", 20, 600, 75, BOTH, 0, {}),
    "exact_1x1_batch": ("f32", 24, 300, 100, BOTH, 0, BATCH),
    "exact_2x1": ("f32", 48, 300, 70, BOTH, 0, {}),
    "exact_3x1": ("f32", 80, 150, 70, BOTH, 0, {}),
    "exact_4x1": ("f32", 128, 150, 50, BOTH, 0, {}),
    "sb_k20": ("bf16x3", 20, 300, 70, BOTH, 1, {}),
    "sb2_k48_y": ("bf16x3", 48, 300, 70, dict(update_Y=True), 2, {}),
    "sb4_k80": ("bf16x3", 80, 150, 70, BOTH, 4, {}),
    "sb4_k128_x": ("bf16x3", 128, 150, 70, dict(update_X=True), 4, {}),
    "sb8_k64": ("bf16x3", 64, 700, 95, BOTH, 8, {}),
    "sb8_k128": ("bf16x3", 128, 300, 95, BOTH, 8, {}),
    "sb8_k100_bf16_store": ("bf16x3", 100, 300, 95, BOTH, 8, dict(store="bf16")),
    "sb8_k40_3_chunks": ("bf16x3", 40, 600, 161, BOTH, 8, dict(chunks=3)),
    "layers_k32_batch": ("f32", 32, 300, 100, dict(update_col_layers=True), None, BATCH),
    # the layer pass at KB = 3 with a wide (64-slot) table; at KB = 4, 16 slots and bf16 storage; K = 64 with 64 batches
    # (128 slots do not fit next to eight X panels: k_layer_grad)
    "layers_k96_40_batches": ("f32", 96, 300, 100, dict(update_col_layers=True), None,
                              dict(BATCH, n_batches=40, layer_path=1)),
    "layers_k128_bf16_store": ("f32", 128, 300, 100, dict(update_col_layers=True), None,
                               dict(BATCH, store="bf16", layer_path=1)),
    "layers_k64_64_batches": ("f32", 64, 300, 100, dict(update_col_layers=True), None,
                              dict(BATCH, n_batches=64, layer_path=2)),
}


def target_problem(name):
    prec, K, M, N, flags, fam, extra = TARGETS[name]
    kw = {k: v for k, v in extra.items() if k not in ("store", "chunks", "layer_path")}
    p = make_problem(M=M, N=N, K=K, seed=K + M, col_params=True, weights=True, nan_frac=0.05, scale=0.5, **kw)
    if extra.get("store") == "bf16":
        p["D"] = np.asfortranarray(bf16_round(p["D"]))
    return p


def set_target(ctx, name, p):
    """Everything the target's results may depend on, set through the ABI."""
    prec, K, M, N, flags, fam, extra = TARGETS[name]
    to_context(p, ctx)
    if extra.get("store") == "bf16":
        ctx.set_data(p["D"], store="bf16")
    ctx.set_precision(prec)
    ctx.comm_set_chunks(extra.get("chunks", 0))


def run_target(ctx, name, p):
    prec, K, M, N, flags, fam, extra = TARGETS[name]
    set_target(ctx, name, p)
    n0 = ctx.get_precision()[1]
    loss, g = grads_of(ctx, p, **flags)
    if fam is not None:
        assert ctx.last_kernel() == fam, (ctx.last_kernel(), fam)
        assert ctx.get_precision()[1] == n0 + (0 if fam == 0 else extra.get("chunks", 1))
    if "layer_path" in extra:
        assert ctx.last_path()["layer_path"] == extra["layer_path"], ctx.last_path()
    # optimizer state is kept across re-marshalling on purpose (test_adapt_lr_keeps_optimizer_state_across_segments):
    # set_optimizer resets it, so the fit does not see the history's
    ctx.set_optimizer("adagrad", lr=0.05)
    r = ctx.fit(max_epochs=3, abs_tol=0, rel_tol=0, **flags)
    X, Y = ctx.get_factors()
    return dict(loss=loss, g=g, trace=r["loss"], term=r["term_code"], X=X, Y=Y)


def fresh(pkg, name, p):
    ctx = pkg.Context(0)
    try:
        return run_target(ctx, name, p)
    finally:
        ctx.close()


_POISON = {}


def poison_problem(K):
    """Larger than every target (both dimensions ragged), mixed noise and batch layers; NaN X, +-Inf Y columns, NaN data."""
    if K not in _POISON:
        p = make_problem(M=3100, N=1517, K=K, seed=99 + K, bernoulli_frac=0.2, poisson_frac=0.1, n_views=2, batch_views=2,
                         n_batches=6, col_params=True, weights=True, nan_frac=0.1)
        p["X"][:] = np.nan
        p["Y"][:, 5::97] = np.inf
        p["Y"][:, 50::97] = -np.inf
        _POISON[K] = p
    return _POISON[K]


def poison_history(ctx, K):
    """Every pass kind in both precisions and both storage types, at this K, on the poison problem."""
    p = poison_problem(K)
    for store in ("f32", "bf16"):
        to_context(p, ctx)
        ctx.set_data(p["D"], store=store)
        for prec in ("f32", "bf16x3"):
            ctx.set_precision(prec)
            ctx.set_factors(p["X"], p["Y"])
            for flags in (BOTH, dict(update_X=True), dict(update_Y=True), dict(update_col_layers=True)):
                grads_of(ctx, p, **flags)
            ctx.comm_set_chunks(3)
            grads_of(ctx, p, **BOTH)
            ctx.comm_set_chunks(0)
            ctx.set_optimizer("adagrad", lr=0.05)
            r = ctx.fit(max_epochs=2, abs_tol=0, rel_tol=0, **BOTH)
            assert r["term_code"] == "nonfinite", r["term_code"]


def other_k(K):
    return 128 if K <= 64 else 40


def assert_same(a, b):
    assert a["loss"] == b["loss"], (a["loss"], b["loss"])
    assert a["g"].keys() == b["g"].keys()
    for k in a["g"]:
        us, vs = (a["g"][k], b["g"][k]) if isinstance(a["g"][k], list) else ([a["g"][k]], [b["g"][k]])
        for u, v in zip(us, vs):
            assert np.array_equal(u, v), f"gradient {k} differs from a fresh context"
    assert a["term"] == b["term"]
    assert np.array_equal(a["trace"], b["trace"]), (a["trace"], b["trace"])
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["Y"], b["Y"]), "fitted factors differ from a fresh context"


def assert_oracle(p, flags, r):
    m = to_oracle(p)
    m.m.has_colreg = 0
    m.m.has_batchreg = 0
    _, go = m.loss_and_grads(**flags)
    assert abs(r["loss"] - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6, (r["loss"], go["data_loss"])
    for k, v in r["g"].items():
        for w, (u, uo) in enumerate(zip(v, go[k]) if isinstance(v, list) else [(v, go[k])]):
            assert np.isfinite(u).all(), f"non-finite gradient {k}[{w}]"
            assert rel_err(u, uo) <= GRAD_TOL, (k, w, rel_err(u, uo))
    if "mu" in r["g"]:
        worst = layer_check(p, r["g"], go)
        assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", list(TARGETS))
def test_pass_does_not_depend_on_context_history(pkg, name):
    prec, K, M, N, flags, fam, extra = TARGETS[name]
    p = target_problem(name)
    want = fresh(pkg, name, p)
    ctx = pkg.Context(0)
    try:
        poison_history(ctx, K)
        poison_history(ctx, other_k(K))
        # the same shape with NaN X, right before the target, at the target's precision (X only: the split families of
        # single-gradient passes write other image layouts into the same buffers)
        set_target(ctx, name, p)
        ctx.set_factors(np.full_like(p["X"], np.nan), p["Y"])
        grads_of(ctx, p, update_X=True)
        got = run_target(ctx, name, p)
    finally:
        ctx.close()
    assert_same(got, want)
    assert_oracle(p, flags, dict(loss=got["loss"], g=got["g"]))


# ---- two named regressions: the absent row blocks of pmf_fused_sb8_kernel's ragged last panel --------------------------
def _both_pass(ctx, p):
    loss, g = grads_of(ctx, p, **BOTH)
    assert ctx.last_kernel() == 8, ctx.last_kernel()
    return loss, g


def _fresh_both(pkg, p):
    ctx = pkg.Context(0)
    try:
        to_context(p, ctx)
        ctx.set_precision("bf16x3")
        return _both_pass(ctx, p)
    finally:
        ctx.close()


def _check_regression(pkg, p, loss, g):
    assert np.isfinite(g["Y"]).all(), "non-finite gY: a stale NaN in the absent row blocks of sb8's last panel"
    assert np.isfinite(g["X"]).all(), "non-finite gX"
    l0, g0 = _fresh_both(pkg, p)
    assert loss == l0 and np.array_equal(g["X"], g0["X"]) and np.array_equal(g["Y"], g0["Y"]), \
        "the pass differs from the same pass on a fresh context"


def test_sb8_k128_after_sb4_nan_pass(pkg):
    """K = 128: an X-only pass (pmf_fused_sb4_kernel, 40-KiB image blocks) with NaN X writes over the padding behind sb8's
    32-KiB blocks.  M = 900: nRB = 29 blocks, the last 256-row panel has 5 of its 8."""
    p = make_problem(M=900, N=95, K=128, seed=31, col_params=True, weights=True, nan_frac=0.05, scale=0.4)
    ctx = pkg.Context(0)
    try:
        to_context(p, ctx)
        ctx.set_precision("bf16x3")
        ctx.set_factors(np.full_like(p["X"], np.nan), p["Y"])
        grads_of(ctx, p, update_X=True)
        assert ctx.last_kernel() == 4
        ctx.set_factors(p["X"], p["Y"])
        loss, g = _both_pass(ctx, p)
    finally:
        ctx.close()
    _check_regression(pkg, p, loss, g)


def test_sb8_k64_after_larger_m(pkg):
    """K = 64: a pass at M = 5000 with NaN X leaves NaN images where the next, smaller problem's last 512-row panel has
    no rows.  M = 700: nRB = 22, the second panel has 6 of its 16 blocks."""
    big = make_problem(M=5000, N=95, K=64, seed=37, col_params=True, weights=True, nan_frac=0.05)
    p = make_problem(M=700, N=95, K=64, seed=41, col_params=True, weights=True, nan_frac=0.05)
    ctx = pkg.Context(0)
    try:
        to_context(big, ctx)
        ctx.set_precision("bf16x3")
        ctx.set_factors(np.full_like(big["X"], np.nan), big["Y"])
        _both_pass(ctx, big)
        to_context(p, ctx)
        loss, g = _both_pass(ctx, p)
    finally:
        ctx.close()
    _check_regression(pkg, p, loss, g)
