"""Every device and pinned allocation of libpmf_hip.so has one owner (DevBuf, csrc/pmf_ctx.h), and the library counts the
bytes its owners hold (pmf_debug_live_bytes: process-wide, so exact whatever else runs on the GPU).  These tests hold the
counter against what the contexts are known to own: everything comes back with close(), a new data shape and a new K drop
what they should, a refused call owns nothing, and the capacities the extents guard reads are the allocations themselves.

tests/golden/buffer_capacities_70x100_k40.json holds the capacities the commit BEFORE the owner type reported for
capacity_sequence() below, from its hand-kept capacity fields.  It was written on an MI355X at that commit, with this file
copied into its tests/, by

    python tests/test_gpu_buffer_lifecycle.py > tests/golden/buffer_capacities_70x100_k40.json
"""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from problems import make_problem, to_context

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "buffer_capacities_70x100_k40.json"
BOTH = dict(update_X=True, update_Y=True)
M, N, K, KP = 70, 100, 40, 64          # the smallest shapes at which growth has gone wrong here (test_gpu_fresh_growth.py)
M2, N2, K2 = 33, 65, 100
NB = 3                                  # batches per view


def live(pkg):
    return pkg._lib.live_bytes()


def assert_fits(ctx, where):
    for name, e in ctx.pass_extents(**BOTH).items():
        assert e["need"] <= e["capacity"], f"{where}: the pass addresses {e['need']} bytes of {name}, {e['capacity']} allocated"


def first_problem(**kw):
    """70 x 100 at K = 40: two batch views over all columns, mixed noise, layer regularizers, group term on X, FSARD on Y."""
    kw = dict(dict(seed=11, bernoulli_frac=0.2, n_views=2, batch_views=2, n_batches=NB, nan_frac=0.05, weights=True,
                   col_params=True, layer_regs=True, xreg="group", yreg="fsard", random_init=True, scale=0.5), **kw)
    return make_problem(M=M, N=N, K=K, **kw)


def second_problem():
    return make_problem(M=M2, N=N2, K=K2, seed=12, n_views=2, batch_views=1, n_batches=NB, nan_frac=0.1, col_params=True,
                        random_init=True, scale=0.5)


def epoch(ctx, prec, **flags):
    ctx.set_precision(prec)
    ctx.set_optimizer("adagrad", lr=0.01)
    r = ctx.fit(max_epochs=1, abs_tol=0, rel_tol=0, **flags)
    assert np.isfinite(r["loss"]).all(), (prec, flags, r)


def network_blocks(n, k, v=3):
    """Per factor: AA = 1.1 I (n x n), AB with one -1 per row (n x v), BB = 2 I (v x v)."""
    import scipy.sparse as sp
    AB = sp.csr_matrix((-np.ones(n, np.float32), (np.arange(n), np.arange(n) % v)), shape=(n, v))
    return ([sp.identity(n, format="csr", dtype=np.float32) * 1.1 for _ in range(k)], [AB for _ in range(k)],
            [sp.identity(v, format="csr", dtype=np.float32) * 2.0 for _ in range(k)])


def walk_every_owner(pkg, ctx, step):
    """Every struct that owns memory gets its buffers allocated at least once; step(name) after each."""
    p = first_problem()
    to_context(p, ctx); step("marshalled: views, mixed noise, group, FSARD, layer regularizers")
    ctx.add_reg_l2("X", np.full(K, 0.5, np.float32), 0.5); step("L2 on X")
    epoch(ctx, "f32", update_col_layers=True, **BOTH); step("f32 epoch, both gradients and column layers")
    epoch(ctx, "bf16x3", **BOTH); step("bf16x3 epoch, both gradients")
    epoch(ctx, "bf16x3", update_X=True); step("X-only epoch")
    epoch(ctx, "f32", update_Y=True); step("Y-only epoch")
    ctx.comm_set_chunks(2)
    epoch(ctx, "bf16x3", **BOTH); step("two column chunks")
    ctx.comm_set_chunks(0)
    ctx.stats(); step("stats")
    assert ctx.impute().shape == (M, N); step("impute")
    assert ctx.impute_entries([1, M], [1, N]).shape == (2,); step("impute by entry")
    r = ctx.fit_lbfgs(m=3, max_iter=2); step("fit_lbfgs, m = 3")
    assert np.isfinite(r["final_loss"])
    ctx.stage_reweight_col_losses(M); step("closed-form stage")
    ctx.stage_rotate_by_svd(); step("post-processing stage")
    rng = np.random.default_rng(5)
    L = 5
    S = (rng.random((L, N // 2)) < 0.3).astype(np.float32)
    args = (np.full(N // 2, 1.001, np.float32), np.full(K, 0.1, np.float32), 1.001, 0.8, 0.05)
    ctx.fsard_update_A(1, N // 2, S, *args, np.full((L, K), 1e-3, np.float32), max_epochs=3); step("fsard_update_A, dense S")
    ctx.fsard_update_A_csr(1, N // 2, S, *args, np.full((L, K), 1e-3, np.float32), max_epochs=3); step("fsard_update_A, CSR S")
    ctx.clear_yreg()
    ctx.add_yreg_ard([(1, N // 2), (N // 2 + 1, N)], np.full(2, 1.001, np.float32), np.full(2, 0.001, np.float32))
    epoch(ctx, "f32", **BOTH); step("ARD on Y")
    ctx.add_reg_network("X", *network_blocks(M, K))
    ctx.add_reg_network("Y", *network_blocks(N, K))
    ctx.add_reg_l1("Y", np.full(K, 1e-3, np.float32))
    epoch(ctx, "f32", **BOTH); step("network terms on X and Y, L1 on Y")
    to_context(second_problem(), ctx); step("set_data to 33 x 65, set_factors at K = 100")
    epoch(ctx, "bf16x3", **BOTH); step("bf16x3 epoch at the new shape")


def test_everything_comes_back(pkg):
    """Create, walk every owner at 70 x 100 / K = 40 and 33 x 65 / K = 100, close: both counters are back where they were.
    After every step each buffer of the data pass holds what the pass addresses.
    Measured, run alone (device, pinned) bytes: before create (0, 0), peak (12191334, 128), after close (0, 0)."""
    before = live(pkg)
    peak = [before]
    ctx = pkg.Context(0)
    try:
        created = live(pkg)
        assert created[0] > before[0] and created[1] > before[1]     # the loss scalars: device and pinned

        def step(name):
            assert_fits(ctx, name)
            now = live(pkg)
            peak[0] = tuple(max(a, b) for a, b in zip(peak[0], now))

        walk_every_owner(pkg, ctx, step)
    finally:
        ctx.close()
    after = live(pkg)
    print(f"live bytes (device, pinned): before create {before}, peak {peak[0]}, after close {after}")
    assert peak[0][0] > created[0]
    assert after == before, (before, peak[0], after)


def test_shape_and_K_changes_drop_what_they_should(pkg):
    p, q = first_problem(), second_problem()
    tot = NB * N                                                       # (batch, column) values of the two views together
    dropped = (4 * 4 * KP * (M + N)                                    # X, Y: parameter, gradient, two optimizer states
               + 2 * 4 * 4 * tot                                       # logdelta, theta: the same four each
               + 2 * M * 4 + tot * 8 + tot * 4)                        # row -> batch maps, {delta, theta} table, value -> view
    ctx = pkg.Context(0)
    try:
        to_context(p, ctx)
        held = live(pkg)
        ctx.set_data(q["D"])                                           # smaller in M and N: what it allocates anew is smaller too
        assert held[0] - live(pkg)[0] >= dropped, (held, live(pkg), dropped)
        rounds = []
        for _ in range(2):
            to_context(p, ctx)
            epoch(ctx, "bf16x3", **BOTH)
            to_context(q, ctx)
            epoch(ctx, "bf16x3", **BOTH)
            assert_fits(ctx, "repeated sequence")
            rounds.append(live(pkg))
        assert rounds[0] == rounds[1], rounds
    finally:
        ctx.close()


def test_a_refused_call_owns_nothing(pkg):
    p = first_problem()
    ctx = pkg.Context(0)
    try:
        to_context(p, ctx)
        ext = ctx.pass_extents(**BOTH)
        held = live(pkg)
        # pmf_fsard_update_A_csr with L = 0, straight through the C ABI (the binding refuses an S without rows itself)
        one_i64, one_i32, one_f32 = np.zeros(1, np.int64), np.zeros(1, np.int32), np.zeros(K, np.float32)
        fp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
        rc = ctx.lib.pmf_fsard_update_A_csr(
            ctx._h, C.c_int64(1), C.c_int64(N // 2), 0, ip(one_i64), one_i32.ctypes.data_as(C.POINTER(C.c_int32)), fp(one_f32),
            fp(np.ones(N // 2, np.float32)), fp(one_f32), C.c_float(1.001), C.c_float(0.8), C.c_float(0.05), fp(one_f32),
            fp(one_f32), 3, 20, C.c_double(1e-5), None, None, None)
        assert rc != 0 and "pmf_fsard_update_A_csr: L must be >= 1 (got 0)" in ctx.lib.pmf_last_error().decode()
        assert live(pkg) == held
        for m in (0, 33):
            with pytest.raises(pkg.PMFError, match=f"m = {m}"):
                ctx.fit_lbfgs(m=m)
            assert live(pkg) == held
        need = ext["gy_slabs"]["need"]
        with pytest.raises(pkg.PMFError, match=f"data pass refused: it addresses {need} bytes of gy_slabs, {need - 1} are allocated"):
            ctx.pass_extents(capacity_override={"gy_slabs": need - 1}, **BOTH)
        assert live(pkg) == held
        assert ctx.pass_extents(**BOTH) == ext
    finally:
        ctx.close()


def capacity_sequence(pkg):
    """On a fresh context: 70 x 100 at K = 40 with one batch view, the both-gradients pass planned in f32 and then in bf16x3
    (the order in which the gX slots were once left too small).  {precision: {buffer: capacity in bytes}}."""
    p = make_problem(M=M, N=N, K=K, seed=7, n_views=2, batch_views=1, n_batches=NB, nan_frac=0.1, col_params=True)
    ctx = pkg.Context(0)
    out = {}
    try:
        to_context(p, ctx)
        for prec in ("f32", "bf16x3"):
            ctx.set_precision(prec)
            out[prec] = {k: int(e["capacity"]) for k, e in ctx.pass_extents(**BOTH).items()}
    finally:
        ctx.close()
    return out


def test_capacities_are_the_allocations(pkg):
    """What pass_extents reports as capacity is the owner's bytes(); it must equal what the hand-kept fields held."""
    want = json.loads(GOLDEN.read_text())
    got = capacity_sequence(pkg)
    assert all(len(v) == 10 for v in want.values())
    assert got == want


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    import pmf_import
    print(json.dumps(capacity_sequence(pmf_import.load()), indent=1))
