"""The fused data pass at its batch-table edges, against the fp64 oracle (problems and restated rules: batch_cases.py).

Every fused family stages a piece's slot -> batch map (Pm) and its rows' slots (Bw0) in LDS and rebuilds the 32-column x
16-slot {delta, theta} table per tile through pmf_bt_index.  What goes wrong there gives finite, plausible gradients: a row
that reads its neighbour's slot, slot 14 taken for the identity slot 15, a tile that takes the wrong view at a seam, a
slot map left over from the previous piece or from rows that have since changed.  The cases: exactly 15 and exactly 16
batches in a panel (in the ragged last panel and at the top of the first), a panel that does not fit whose halves do,
rows and whole panels in no batch, views that meet, leave gaps and end inside tiles, 16 (5, 6) batch views, per-entry
gathers at KB = 3 and 4, 255 and 256 batches, column chunks, workgroups that walk pieces of several row panels, and
set_batch_views on a live context.

Every case asserts the family, bmode, slots and split-launch count that batch_cases.expected_batch_path restates from the
selection rules, compares the loss and the gradients with the oracle at the tolerances of tests/test_gpu_parity.py (the
max-norm at GRAD_TOL, and every element at the rounding of its own terms: factor_gate, one FACTOR_CHECK line), runs
the pass twice for the same bits and prints one BATCH_EDGE line with its relative errors.  tests/test_batch_cases.py
holds the condition that makes the comparison mean something: on every problem here one row in the wrong batch, one
unbatched row in batch 0 or one view boundary off by a column moves gX or gY by at least 10 GRAD_TOL.
"""
import numpy as np
import pytest

import batch_cases as bc
from problems import rel_err, to_context
from test_gpu_parity import GRAD_TOL, LOSS_RTOL, factor_gate, grads_of
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

PATH_PARAMS = [pytest.param(path, id=bc.path_id(path)) for path in bc.PATHS]
SB8_512 = ("bf16x3", 48, "both")
SB8_256 = ("bf16x3", 128, "both")


def one_pass(ctx, p, path, launches=1):
    """The data pass of `path` on the problem the context holds, twice: asserts the expected family, bmode, slots and
    split-launch count and equal bits; returns (loss, grads, expected)."""
    prec, K, gname = path
    flags = bc.GRADS[gname]
    exp = bc.expected_of(p, path)
    ctx.set_precision(prec)
    try:
        n0 = ctx.get_precision()[1]
        loss, g = grads_of(ctx, p, **flags)
        lp = ctx.last_path()
        got = (ctx.last_kernel(), lp["bmode"], lp["slots"], ctx.get_precision()[1] - n0)
        want = (exp[0], exp[2], exp[3], launches if exp[0] != 0 else 0)
        assert got == want, f"(family, bmode, slots, split launches) = {got}, expected {want}"
        loss2, g2 = grads_of(ctx, p, **flags)
    finally:
        ctx.set_precision("f32")
    assert loss == loss2, (loss, loss2)
    for w in g:
        assert np.array_equal(g[w], g2[w]), f"g{w}: the second pass differs"
    return loss, g, exp


def check_oracle(ctx, p, name, go, loss, g):
    """ctx: the context that ran the pass (or its kernel family, where the context is closed)."""
    errs = {}
    for w in ("X", "Y"):
        if w in g:
            assert np.isfinite(g[w]).all(), f"non-finite g{w}"
            errs[w] = rel_err(g[w], go[w])
    print(f"BATCH_EDGE {name} relerr " + " ".join(f"g{w}={errs[w]:.3e}" if w in errs else f"g{w}=-" for w in ("X", "Y")))
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6, (loss, go["data_loss"])
    for w, e in errs.items():
        assert e <= GRAD_TOL, (w, e)
    factor_gate(ctx, p, g, go, scales=bc.scales_of(p))


def run_case(ctx, name, p, path, family=None, BM=None, bmode=None):
    to_context(p, ctx)
    loss, g, exp = one_pass(ctx, p, path)
    for got, want in zip(exp, (family, BM, bmode)):
        assert want is None or got == want, (exp, family, BM, bmode)      # what the case was built to reach
    check_oracle(ctx, p, f"{name}-{bc.path_id(path)}", bc.oracle_of(p), loss, g)


# ---- 1. exactly 15 and exactly 16 batches in a panel ----------------------------------------------------------------
@pytest.mark.parametrize("mirror", [False, True], ids=["last_panel", "first_panel_top"])
@pytest.mark.parametrize("path", PATH_PARAMS)
def test_fifteen_batches_in_a_panel_use_slot_14_next_to_the_identity_slot(ctx, path, mirror):
    fam, BM = bc.PATHS[path]
    p = bc.slots_edge(BM, path[1], 15, mirror)
    assert bc.panel_counts_of(p)(BM) == 15
    run_case(ctx, "slots15_mirror" if mirror else "slots15", p, path, family=fam, BM=BM, bmode=1)


@pytest.mark.parametrize("mirror", [False, True], ids=["last_panel", "first_panel_top"])
@pytest.mark.parametrize("path", PATH_PARAMS)
def test_sixteen_batches_in_a_row_block_gather_per_entry(ctx, path, mirror):
    """The 16 batches sit in one 32-row block: no shorter panel of the fall-back family fits either (sb, sb4 -> exact;
    sb8 -> sb2 or sb4 -> exact), so every path ends in the exact kernel's per-entry gathers."""
    fam, BM = bc.PATHS[path]
    p = bc.slots_edge(BM, path[1], 16, mirror)
    assert bc.panel_counts_of(p)(128) == 16
    run_case(ctx, "slots16_mirror" if mirror else "slots16", p, path, family=0, bmode=2)


# ---- 2. a panel that does not fit, whose halves do ------------------------------------------------------------------
@pytest.mark.parametrize("path,fam,BM", [pytest.param(SB8_512, 2, 256, id="k48-sb8-to-sb2"),
                                         pytest.param(SB8_256, 4, 128, id="k128-sb8-to-sb4")])
def test_sb8_falls_back_to_the_family_whose_shorter_panel_fits(ctx, path, fam, BM):
    p = bc.halves_fit(bc.PATHS[path][1], path[1])
    run_case(ctx, "halves_fit", p, path, family=fam, BM=BM, bmode=1)


# ---- 3. rows in no batch, view seams, many views --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unbatched", "view_seams", "views16"])
@pytest.mark.parametrize("path", PATH_PARAMS)
def test_unbatched_rows_view_seams_and_sixteen_views(ctx, path, name):
    fam, BM = bc.PATHS[path]
    p = bc.EVERY_PATH[name](BM, path[1])
    if name == "views16" and path == SB8_512:
        fam, BM = 2, 256                                # 16 views: the 512-row sb8 has LDS room for 5
    run_case(ctx, name, p, path, family=fam, BM=BM, bmode=1)


@pytest.mark.parametrize("n,fam,BM", [(5, 8, 512), (6, 2, 256)])
def test_five_views_fit_the_512_row_sb8_and_six_do_not(ctx, n, fam, BM):
    p = bc.many_views(512, 48, n)
    run_case(ctx, f"views{n}", p, SB8_512, family=fam, BM=BM, bmode=1)


@pytest.mark.parametrize("path", [pytest.param(SB8_256, id="sb8-k128"), pytest.param(("f32", 48, "both"), id="exact-k48")])
def test_view_seams_with_bf16_stored_data(ctx, path):
    """D stored as bf16; the oracle takes the bf16-rounded matrix."""
    fam, BM = bc.PATHS[path]
    p = dict(bc.view_seams(BM, path[1]))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        loss, g, exp = one_pass(ctx, p, path)
        assert exp[:3] == (fam, BM, 1), exp
        check_oracle(ctx, p, f"view_seams_bf16-{bc.path_id(path)}", bc.oracle_of(p), loss, g)
    finally:
        ctx.set_data(p["D"])            # back to f32 storage for the tests that follow


# ---- 4. per-entry gathers at KB = 3 and 4; 255 and 256 batches ------------------------------------------------------
@pytest.mark.parametrize("K", [80, 128])
def test_per_entry_gathers_in_the_kb3_and_kb4_exact_kernels(ctx, K):
    run_case(ctx, "gather", bc.gather(K), ("f32", K, "both"), family=0, BM=128, bmode=2)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("nb,bmode,slots", [(255, 1, 256), (256, 2, 0)])
def test_255_batches_fill_the_dense_table_and_256_have_none(ctx, prec, nb, bmode, slots):
    path = (prec, 20, "both")
    p = bc.many_batches(nb)
    assert bc.expected_of(p, path)[3] == slots
    run_case(ctx, f"nb{nb}", p, path, family=bc.PATHS[path][0] if bmode == 1 else 0, BM=256, bmode=bmode)


# ---- 5. column chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [pytest.param(("f32", 48, "both"), id="exact-k48"), pytest.param(SB8_512, id="sb8-k48")])
def test_view_seams_in_three_column_chunks(ctx, path):
    """Six column tiles in three launches: every chunk starts its table at another view.  (A chunked pass sums the row
    panels in another order than the unchunked one -- tests/test_gpu_comm.py compares them to rounding, not bit for bit --
    so the chunked pass is held to the oracle.)"""
    fam, BM = bc.PATHS[path]
    p = bc.view_seams(BM, path[1], 161)
    to_context(p, ctx)
    ctx.comm_set_chunks(3)
    try:
        loss, g, exp = one_pass(ctx, p, path, launches=3)     # (one launch per chunk: counted on the split path)
    finally:
        ctx.comm_set_chunks(0)
    assert exp[:3] == (fam, BM, 1), exp
    check_oracle(ctx, p, f"view_seams161_chunks3-{bc.path_id(path)}", bc.oracle_of(p), loss, g)


# ---- 6. workgroups that walk pieces of several row panels -----------------------------------------------------------
@pytest.mark.parametrize("path,reserve", [
    pytest.param(("f32", 64, "both"), None, id="exact-k64"), pytest.param(("f32", 64, "both"), "128", id="exact-k64-reserve128"),
    pytest.param(("bf16x3", 64, "both"), None, id="sb8-k64"), pytest.param(("bf16x3", 64, "both"), "128", id="sb8-k64-reserve128"),
    pytest.param(("bf16x3", 128, "both"), "128", id="sb8-k128-reserve128")])
def test_multi_piece_walks_restage_the_slot_map(ctx, monkeypatch, path, reserve):
    """2049 x 2048 with 40 sorted batches in two views: every row panel has its own slot map, and there are more pieces
    than workgroups, so some workgroup stages a second map and other row slots behind the piece's single barrier.
    Measured (pieces / workgroups): exact K = 64 296 / 256 and 165 / 128; sb8 K = 64 146 / 128; sb8 K = 128 183 / 128.  The
    512-row sb8 on the full grid has 250 pieces for 256 workgroups at M = 2049 and 256 at 2561, so that case runs
    batch_cases.WALK_M_SB8_512 = 3073 rows (two more panels): 280 pieces."""
    prec, K, _ = path
    fam, BM = {64: {"f32": (0, 256), "bf16x3": (8, 512)}, 128: {"bf16x3": (8, 256)}}[K][prec]
    if reserve:
        monkeypatch.setenv("PMF_RESERVE_CUS", reserve)
    p = bc.walk(K, bc.WALK_M_SB8_512 if (BM, reserve) == (512, None) else 2049)
    to_context(p, ctx)
    ctx.set_precision(prec)
    try:
        ext = ctx.pass_extents(update_X=True, update_Y=True)
    finally:
        ctx.set_precision("f32")
    Kp = (K + 31) // 32 * 32
    pieces, grid = ext["gx_part"]["need"] / (BM * Kp * 4), ext["loss_partial"]["need"] / 8
    print(f"BATCH_EDGE walk-{bc.path_id(path)}-reserve{reserve} M={p['M']} pieces={pieces:.0f} workgroups={grid:.0f}")
    assert pieces > grid, (pieces, grid)
    loss, g, exp = one_pass(ctx, p, path)
    assert exp == (fam, BM, 1, 64), exp
    check_oracle(ctx, p, f"walk-{bc.path_id(path)}-reserve{reserve}", bc.oracle_of(p), loss, g)


# ---- 7. the three slot caches follow the rows -----------------------------------------------------------------------
def test_slot_caches_follow_set_batch_views_on_a_live_context(pkg):
    """One context through: state A (both gradients: sb8, 512-row slots; X only: sb2, 256-row slots), the rows' batches
    replaced (X only, then both), then theta and logdelta replaced (both).  Every pass equals, bit for bit, the same pass
    on a fresh context that has only ever seen that state."""
    A, B, C = bc.cache_states()
    steps = [(A, "both"), (A, "X"), (B, "X"), (B, "both"), (C, "both")]
    want_fam = {"both": (8, 512, 1, 16), "X": (2, 256, 1, 16)}

    def run(c, p, gname):
        loss, g, exp = one_pass(c, p, ("bf16x3", 48, gname))
        assert exp == want_fam[gname], exp
        return loss, g

    live = pkg.Context(0)
    got = []
    try:
        to_context(A, live)
        prev = A
        for p, gname in steps:
            if p is not prev:
                live.set_batch_views(p["batch_views"])
                prev = p
            got.append(run(live, p, gname))
    finally:
        live.close()
    for (p, gname), (loss, g) in zip(steps, got):
        fresh = pkg.Context(0)
        try:
            to_context(p, fresh)
            loss_f, g_f = run(fresh, p, gname)
        finally:
            fresh.close()
        assert loss == loss_f, (gname, loss, loss_f)
        for w in g:
            assert np.array_equal(g[w], g_f[w]), f"g{w} of the {gname} pass differs from a fresh context's"
    check_oracle(want_fam["both"][0], C, "slot_caches-bf16x3-k48-both", bc.oracle_of(C), *got[-1])
