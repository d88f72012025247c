"""The layer-parameter pass, the column statistics and the device forward at their K, panel, unit and batch edges,
against the fp64 oracle.

The layer epoch (update_col_layers) runs pmf_layer_kernel<KB, NW, MIXED, DB, WIDE> (pmf_layers.hip.inc) or the VALU
kernel k_layer_grad<KB> (pmf_hip.hip).  The MFMA pass works on units of 64 columns (two 32-column tiles) and row panels of
32 NW rows, R row ranges per column segment, a dense [64 columns][slots] batch table in LDS whose last slot is the identity
(rows outside every batch), and running sums flushed when the row batch changes.  k_layer_grad and k_stats work on
64-column blocks and row chunks with per-batch sums in LDS.  Each case below picks its shape or its batches at one of
these edges, asserts the path and the slot count that must run, and compares

    the layer-only epoch's loss with the oracle's at LOSS_RTOL,
    grad mu, grad logsigma, grad theta, grad logdelta with the segment-scaled check (problems.layer_check) and, except in
    cases built to cancel, with rel_err <= GRAD_TOL.

The selection rules are restated here, not asked of the library (layer_pass_eligible, prepare, launch_layer_pass):
    slots = 16 without batch views; else the power of two >= 16 above the largest batch count of a view, up to 256;
            0 (no dense table) above 255 batches.
    NW = 8 waves for K <= 64 (4 with PMF_LAYER_NW=4 at 33 <= K <= 64), 4 above; the row panel is 32 NW rows.
    The MFMA pass runs while its LDS (LayerCfg::lds) fits in 160 KiB, i.e. up to these slot counts:
        K <= 32: 128 | 33..64: 64 (128 with 4 waves) | 65..96: 128 | 97..128: 64
    otherwise (or with PMF_LAYER_OLD=1, or without a dense table) k_layer_grad, whose 4 (4 Kp + 128 nb_max) bytes of
    dynamic LDS and 32 bytes of static LDS must fit in 160 KiB too (k_stats: the same without the static part): past
    that the epoch (pmf_stats) is refused on the host.
"""
import numpy as np
import pytest

from problems import layer_check, layer_scales, make_problem, rel_err, to_context, to_oracle
from test_gpu_parity import GRAD_TOL, LOSS_RTOL, grads_of
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

KS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
NS = [1, 33, 63, 65, 129]
LAYERS = dict(update_col_layers=True)
LDS_MAX = 160 * 1024
MFMA_MAX_SLOTS = {(1, 8): 128, (2, 8): 64, (2, 4): 128, (3, 4): 128, (4, 4): 64}
STATS_TOL = 2e-5


def slots_for(nb_max):
    if nb_max == 0:
        return 16
    if nb_max > 255:
        return 0
    s = 16
    while s < nb_max + 1:
        s *= 2
    return s


def expected_layer_path(K, nb_max, nw_env=False, old_env=False):
    """(layer path: 1 MFMA pass, 2 k_layer_grad; slots of the dense table; waves of the MFMA pass)."""
    KB = (K + 31) // 32
    NW = 8 if KB == 1 or (KB == 2 and not nw_env) else 4
    slots = slots_for(nb_max)
    mfma = not old_env and slots != 0 and slots <= MFMA_MAX_SLOTS[KB, NW]
    return (1 if mfma else 2), slots, NW


def valu_kernel_fits(K, nb_max, static=32):
    """k_layer_grad (static = 32: block_reduce_sum's four doubles) or k_stats (static = 0): four rows of X and
    [2][nb_max][64] batch sums in dynamic LDS, on top of the kernel's static LDS."""
    Kp = 32 * ((K + 31) // 32)
    return 4 * (4 * Kp + 2 * max(nb_max, 1) * 64) + static <= LDS_MAX


def test_restated_table_has_the_required_cases():
    assert expected_layer_path(80, 15)[0] == 1 and expected_layer_path(96, 127) == (1, 128, 4)
    assert expected_layer_path(64, 63) == (1, 64, 8) and expected_layer_path(64, 64) == (2, 128, 8)
    assert expected_layer_path(64, 127, nw_env=True) == (1, 128, 4)
    assert expected_layer_path(128, 63) == (1, 64, 4) and expected_layer_path(128, 64) == (2, 128, 4)
    assert expected_layer_path(32, 127) == (1, 128, 8) and expected_layer_path(32, 128) == (2, 256, 8)
    assert expected_layer_path(8, 256) == (2, 0, 8)
    assert valu_kernel_fits(32, 318) and not valu_kernel_fits(32, 319)
    assert valu_kernel_fits(32, 319, static=0) and not valu_kernel_fits(32, 320, static=0)
    assert valu_kernel_fits(128, 315) and not valu_kernel_fits(128, 316)
    assert valu_kernel_fits(128, 316, static=0) and not valu_kernel_fits(128, 317, static=0)


# ---- problems ------------------------------------------------------------------------------------------------------
def rows(M, nb, order, rng):
    """batch_of_row: every batch non-empty when M >= nb; 'sorted' (contiguous batches) or 'scrambled'."""
    bor = np.sort(np.concatenate([np.arange(min(nb, M)), rng.integers(0, nb, size=max(M - nb, 0))]))
    if order == "scrambled":
        bor = rng.permutation(bor)
    return bor.astype(np.int32)


def layer_problem(M, N, K, seed, views=(), mixed=True, nan_frac=0.05):
    """views: (start1, stop1, batch_of_row, nb) per batch view.  Mixed noise, column weights and parameters; D does not
    follow the batch effects, so every residual is O(0.3)."""
    p = make_problem(M=M, N=N, K=K, seed=seed, bernoulli_frac=0.2 if mixed else 0.0, poisson_frac=0.1 if mixed else 0.0,
                     nan_frac=nan_frac, weights=True, col_params=True, scale=0.5 if K <= 64 else 0.4)
    rng = np.random.default_rng(seed + 1)
    p["batch_views"] = [dict(start1=s, stop1=e, batch_of_row=np.asarray(bor, np.int32),
                             logdelta=(0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                             theta=(0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32))
                        for s, e, bor, nb in views]
    return p


def std_views(M, N, seed, nb=(6, 15)):
    """A sorted batch view with 6 batches and a scrambled one with 15 (slot 14 next to the identity slot 15) around a view
    without batches; the view boundaries fall inside 32-column tiles.  N < 3: one view with one batch."""
    rng = np.random.default_rng(seed)
    if N < 3:
        return [(1, N, rows(M, 1, "sorted", rng), 1)]
    a, b = N // 3, 2 * N // 3
    assert a % 32 and b % 32
    return [(1, a, rows(M, nb[0], "sorted", rng), nb[0]), (b + 1, N, rows(M, nb[1], "scrambled", rng), nb[1])]


def nb_max(p):
    return max((np.asarray(v["logdelta"]).shape[0] for v in p["batch_views"]), default=0)


def check_layers(ctx, p, expect, cancel=False, frozen=0):
    """One layer-only epoch on `ctx`: path and slots, loss, and the four gradients against the fp64 oracle."""
    flags = dict(LAYERS, frozen_layers=frozen)
    loss, g = grads_of(ctx, p, **flags)
    lp = ctx.last_path()
    assert (lp["layer_path"], lp["slots"]) == tuple(expect[:2]), (lp, expect)
    _, go = to_oracle(p).loss_and_grads(**flags)
    s = layer_scales(p)
    # the Poisson and Bernoulli terms cancel (D does not follow the batch effects here, so a total may be -47 out of
    # terms of 2.7e4 in magnitude): LOSS_RTOL of the terms' magnitudes, which is the loss itself on Gaussian columns
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * max(s["loss"], abs(go["data_loss"])) + 1e-6, \
        (loss, go["data_loss"], s["loss"])
    skip = [k for bit, k in ((1, "logsigma"), (2, "logdelta"), (4, "mu"), (8, "theta")) if frozen & bit]
    worst = layer_check(p, g, go, scales=s, skip=skip)
    assert max(worst.values(), default=0.0) <= 1.0, worst
    if not cancel:
        for k in ("mu", "logsigma", "theta", "logdelta"):
            if k in skip:
                continue
            for a, b in (zip(g[k], go[k]) if isinstance(g[k], list) else [(g[k], go[k])]):
                assert rel_err(a, b) <= GRAD_TOL, (k, rel_err(a, b))
    return g, go


def check_stats(ctx, p, use_factors):
    st = ctx.stats(use_factors)
    so = to_oracle(p).stats(use_factors)
    assert np.array_equal(st["n"], so["n"])
    for k in ("sum", "sumsq", "sqerr", "ssq_grad"):
        assert rel_err(st[k], so[k]) <= STATS_TOL, (k, rel_err(st[k], so[k]))
    assert len(st["batch_count"]) == len(p["batch_views"])
    for v in range(len(p["batch_views"])):
        assert np.array_equal(st["batch_count"][v], so["batch_count"][v]), v
        assert rel_err(st["batch_sqerr"][v], so["batch_sqerr"][v]) <= STATS_TOL, v


def panel_shapes(K, nw_env=False):
    """(M, N): one row; one row in the second panel; the second panel one row short; a 33-row second panel; one row in the
    third panel -- paired with N one above / below a 64-column unit."""
    P = 32 * expected_layer_path(K, 15, nw_env)[2]
    return list(zip([1, P + 1, 2 * P - 1, P + 33, 2 * P + 1], NS))


# ---- 1. K edges x path ---------------------------------------------------------------------------------------------
def _k_edge_cases():
    return [pytest.param(K, path, M, N, id=f"k{K}-{path}-m{M}-n{N}")
            for K in KS for path in ("mfma", "old") for M, N in panel_shapes(K)]


@pytest.mark.parametrize("K,path,M,N", _k_edge_cases())
def test_layer_pass_k_edges_match_oracle(ctx, monkeypatch, K, path, M, N):
    if path == "old":
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    seed = 7 * K + M + N
    p = layer_problem(M, N, K, seed, std_views(M, N, seed))
    to_context(p, ctx)
    # N = 1: a column's sums may cancel, only the segment check applies
    check_layers(ctx, p, expected_layer_path(K, nb_max(p), old_env=path == "old"), cancel=N == 1)


@pytest.mark.parametrize("path", ["mfma", "old"])
@pytest.mark.parametrize("variant", ["gaussian", "no_batch"])
@pytest.mark.parametrize("K", [32, 64, 96, 128])
def test_layer_pass_gaussian_and_batch_free_variants(ctx, monkeypatch, K, variant, path):
    """MIXED = false (Gaussian columns only) and btd = null (no batch view) at every KB."""
    if path == "old":
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    M, N = panel_shapes(K)[3]
    seed = 11 * K + (variant == "gaussian")
    p = layer_problem(M, N, K, seed, std_views(M, N, seed) if variant == "gaussian" else (), mixed=variant != "gaussian")
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(K, nb_max(p), old_env=path == "old"))


# ---- 2. slot and path boundaries -----------------------------------------------------------------------------------
def slot_problem(K, nb, M=300, N=95, seed=0):
    rng = np.random.default_rng(seed)
    return layer_problem(M, N, K, seed, [(1, 40, rows(M, nb, "sorted", rng), nb),
                                         (61, N, rows(M, 6, "scrambled", rng), 6)])


@pytest.mark.parametrize("nb", [15, 16, 63, 64, 127, 128])
@pytest.mark.parametrize("K", [32, 64, 96, 128])
def test_slot_and_path_boundaries(ctx, K, nb):
    p = slot_problem(K, nb, seed=K + nb)
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(K, nb))


@pytest.mark.parametrize("nb", [127, 128])
def test_k64_with_four_waves_takes_128_slots(ctx, monkeypatch, nb):
    monkeypatch.setenv("PMF_LAYER_NW", "4")
    p = slot_problem(64, nb, seed=3 + nb)
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(64, nb, nw_env=True))


@pytest.mark.parametrize("nb", [255, 256])
@pytest.mark.parametrize("K", [8, 128])
def test_dense_table_limit(ctx, K, nb):
    """255 batches: the last 256-slot table, on k_layer_grad; 256: no dense table at all."""
    p = slot_problem(K, nb, M=600, seed=5 + K + nb)
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(K, nb))
    check_stats(ctx, p, True)


def test_slot_count_is_not_left_over_from_an_earlier_problem(ctx):
    """Regression: pmf_debug_last_path reported the slot count of the last problem that had a dense table -- after a
    128-slot problem, a problem without batch views (16-slot tables) or with 256 batches (no table) still showed 128."""
    M, N = 300, 95
    for nb in (100, 0, 100, 256, 15):
        p = slot_problem(8, nb, M=M, N=N, seed=nb) if nb else layer_problem(M, N, 8, 1)
        to_context(p, ctx)
        check_layers(ctx, p, expected_layer_path(8, nb))


# ---- 3. the launch limits of k_layer_grad and k_stats --------------------------------------------------------------
@pytest.mark.parametrize("K", [32, 128])
def test_valu_kernel_limits_count_static_lds_and_refuse_on_the_host(pkg, ctx, K):
    """Regression: the host check of k_layer_grad's LDS left out its 32 B of static LDS.  At 319 batches (K <= 32) the
    160 KiB of dynamic LDS passed the check, hipFuncSetAttribute failed with "invalid argument", and the next call on the
    context reported that error again.  Past each kernel's limit the layer epoch and pmf_stats are refused before any
    launch, naming the batch count, and the context stays usable."""
    nb = max(n for n in range(250, 330) if valu_kernel_fits(K, n))     # the most batches k_layer_grad takes
    assert valu_kernel_fits(K, nb + 1, static=0) and not valu_kernel_fits(K, nb + 2, static=0)   # k_stats: one more
    p = slot_problem(K, nb, M=700, N=70, seed=K)
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(K, nb))
    check_stats(ctx, p, True)
    for extra in (1, 2):
        q = slot_problem(K, nb + extra, M=700, N=70, seed=K + extra)
        to_context(q, ctx)
        msg = rf"too many row batches per view \({nb + extra}\)"
        with pytest.raises(pkg.PMFError, match=msg):
            grads_of(ctx, q, **LAYERS)
        if extra == 1:
            check_stats(ctx, q, True)
        else:
            with pytest.raises(pkg.PMFError, match=msg):
                ctx.stats(True)
    # the same context afterwards
    M, N = panel_shapes(K)[2]
    r = layer_problem(M, N, K, 17, std_views(M, N, 17))
    to_context(r, ctx)
    check_layers(ctx, r, expected_layer_path(K, nb_max(r)))
    check_stats(ctx, r, True)


# ---- 4. row order and flushes --------------------------------------------------------------------------------------
def row_layout(name, M, P, rng):
    """(batch_of_row, nb) of the first batch view."""
    i = np.arange(M)
    if name == "aligned32":          # every lane's 16 rows of a tile share a batch: the fast path on every tile
        return ((i // 32) % 5).astype(np.int32), 5
    if name == "aligned16":          # half tiles: row by row
        return ((i // 16) % 5).astype(np.int32), 5
    if name == "alternating":        # a new batch on every row
        return (i % 3).astype(np.int32), 3
    if name == "span_panels":        # batch 1 spans the first panel boundary (a row-range boundary too: R = n_rp here)
        cuts = [P - 40, P + 40, 2 * P + 5, 3 * P - 1]
        return np.searchsorted(cuts, i, side="right").astype(np.int32), 5
    if name == "one_row_and_empty":  # batch 3 holds one row, batch 5 none
        bor = rows(M, 8, "sorted", rng)
        bor[bor == 5] = 4
        three = np.flatnonzero(bor == 3)
        bor[three[1:]] = 2
        return bor, 8
    if name == "minus_one":          # 15 batches, a few rows outside every batch (the identity slot)
        bor = rows(M, 15, "sorted", rng)
        bor[[0, 5, P - 1, P, P + 1, M - 1]] = -1
        return bor, 15
    raise ValueError(name)


LAYOUTS = ["aligned32", "aligned16", "alternating", "span_panels", "one_row_and_empty", "minus_one"]


@pytest.mark.parametrize("path", ["mfma", "old"])
@pytest.mark.parametrize("K", [16, 64, 96])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_order_and_flushes(ctx, monkeypatch, layout, K, path):
    if path == "old":
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    P = 32 * expected_layer_path(K, 15)[2]
    M, N = 3 * P + 17, 65
    rng = np.random.default_rng(K)
    bor, nb = row_layout(layout, M, P, rng)
    p = layer_problem(M, N, K, 23 + K, [(1, 30, bor, nb), (41, N, rows(M, 6, "scrambled", rng), 6)])
    to_context(p, ctx)
    # one-row batches: a segment of one row, only the segment check applies
    g, go = check_layers(ctx, p, expected_layer_path(K, max(nb, 6), old_env=path == "old"),
                         cancel=layout == "one_row_and_empty")
    if layout == "one_row_and_empty":
        assert not np.any(g["theta"][0][5]) and not np.any(g["logdelta"][0][5]), "a batch without rows has gradients"
    check_stats(ctx, p, True)


# ---- 5. grid: several units per workgroup, R = 1, R = n_rp ---------------------------------------------------------
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def layer_grid(M, N, K, cu):
    """(n_seg, n_rp, R, grid) of launch_layer_pass."""
    P = 32 * expected_layer_path(K, 15)[2]
    n_ct, n_rp = -(-N // 32), -(-M // P)
    n_seg = -(-n_ct // 2)
    R = max(1, min(n_rp, -(-4 * cu // n_seg)))
    return n_seg, n_rp, R, min(n_seg * R, cu)


@pytest.mark.parametrize("case", ["units_per_workgroup", "one_row_range", "r_is_n_rp"])
def test_layer_pass_grid_edges(ctx, case):
    cu = n_cu()
    K = 8 if case != "r_is_n_rp" else 40
    if case == "units_per_workgroup":
        M, N = 300, 64 * (cu + 17) - 5
    elif case == "one_row_range":
        M, N = 300, 64 * (4 * cu + 1) - 7
    else:
        M, N = 5 * 256 + 7, 63
    n_seg, n_rp, R, grid = layer_grid(M, N, K, cu)
    if case == "units_per_workgroup":
        assert n_seg > cu and R > 1 and n_seg * R > grid, (n_seg, R, grid)
    elif case == "one_row_range":
        assert n_seg >= 4 * cu and R == 1 and n_rp >= 2, (n_seg, R, n_rp)
    else:
        assert n_seg == 1 and R == n_rp >= 6, (n_seg, R, n_rp)
    rng = np.random.default_rng(M + N)
    # batch 2 of the sorted view spans the row-panel boundary at 256 (inside one row range when R = 1)
    bor = np.searchsorted([100, 200, 290], np.arange(M), side="right").astype(np.int32)
    a, b = N // 3, 2 * N // 3
    p = layer_problem(M, N, K, 29, [(1, a, bor, 4), (b + 1, N, rows(M, 15, "scrambled", rng), 15)], nan_frac=0.02)
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(K, 15))


# ---- 6. bf16-stored data -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["mfma", "old"])
@pytest.mark.parametrize("nb", [15, 40])
@pytest.mark.parametrize("K", [32, 64, 96, 128])
def test_bf16_stored_layer_pass_matches_oracle_on_the_rounded_matrix(ctx, monkeypatch, K, nb, path):
    if path == "old":
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    M, N = panel_shapes(K)[3]
    seed = 31 * K + nb
    p = layer_problem(M, N, K, seed, std_views(M, N, seed, nb=(nb, 6)))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        check_layers(ctx, p, expected_layer_path(K, nb, old_env=path == "old"))
        check_stats(ctx, p, True)
    finally:
        ctx.set_data(p["D"])


# ---- 7. views ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 64, 100])
@pytest.mark.parametrize("layout", ["sixteen_views", "shared_tile"])
def test_view_layouts(ctx, K, layout):
    P = 32 * expected_layer_path(K, 15)[2]
    M = P + 33
    rng = np.random.default_rng(K)
    if layout == "sixteen_views":    # PMF_MAXV batch views, batch counts 1..15, sorted and scrambled in turn
        N = 70
        views = [(4 * v + 1, 4 * v + 3, rows(M, v % 15 + 1, ("sorted", "scrambled")[v % 2], rng), v % 15 + 1)
                 for v in range(16)]
    else:                            # three batch views in one 32-column tile; one of them a single column
        N = 40
        views = [(1, 9, rows(M, 3, "sorted", rng), 3), (10, 10, rows(M, 9, "scrambled", rng), 9),
                 (11, 27, rows(M, 14, "scrambled", rng), 14)]
    p = layer_problem(M, N, K, 37 + K, views)
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(K, nb_max(p)))
    check_stats(ctx, p, True)


# ---- 8. frozen layers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["mfma", "old"])
@pytest.mark.parametrize("bit", [1, 2, 4, 8])
def test_each_frozen_layer_leaves_the_others(ctx, monkeypatch, bit, path):
    if path == "old":
        monkeypatch.setenv("PMF_LAYER_OLD", "1")
    M, N = panel_shapes(40)[3]
    p = layer_problem(M, N, 40, 41, std_views(M, N, 41))
    to_context(p, ctx)
    check_layers(ctx, p, expected_layer_path(40, nb_max(p), old_env=path == "old"), frozen=bit)


# ---- 9. pmf_stats --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_factors", [False, True])
@pytest.mark.parametrize("K", KS)
def test_stats_k_edges(ctx, K, use_factors):
    M, N = panel_shapes(K)[3]
    p = layer_problem(M, N, K, 43 + K, std_views(M, N, 43 + K))
    to_context(p, ctx)
    check_stats(ctx, p, use_factors)


@pytest.mark.parametrize("use_factors", [False, True])
@pytest.mark.parametrize("M,N", panel_shapes(32))
def test_stats_panel_edges(ctx, M, N, use_factors):
    p = layer_problem(M, N, 32, 47 + M, std_views(M, N, 47 + M))
    to_context(p, ctx)
    check_stats(ctx, p, use_factors)


@pytest.mark.parametrize("nb", [15, 16, 255])
def test_stats_batch_counts(ctx, nb):
    p = slot_problem(64, nb, M=600, seed=53 + nb)
    to_context(p, ctx)
    check_stats(ctx, p, True)


def test_stats_all_nan_column_and_row(ctx):
    M, N = panel_shapes(32)[3]
    p = layer_problem(M, N, 32, 59, std_views(M, N, 59))
    p["D"][:, 5] = np.nan          # (a column of the sorted batch view)
    p["D"][:, N - 2] = np.nan      # (a column of the scrambled batch view)
    p["D"][7, :] = np.nan
    p["D"][M - 1, :] = np.nan
    to_context(p, ctx)
    for uf in (False, True):
        check_stats(ctx, p, uf)
    check_layers(ctx, p, expected_layer_path(32, nb_max(p)))


# ---- 10. pmf_forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_forward_k_edges_match_oracle(ctx, K):
    M, N = panel_shapes(K)[3]
    p = layer_problem(M, N, K, 61 + K, std_views(M, N, 61 + K))
    p["batch_views"][0]["batch_of_row"][[0, 3, M - 1]] = -1
    to_context(p, ctx)
    Z = ctx.forward().astype(np.float64)
    Zo = to_oracle(p).forward()
    # the forward rounds sigma_j delta_bj sum_k X_ki Y_kj (K f32 products and sums) and adds mu_j + theta_bj
    X, Y = p["X"].astype(np.float64), p["Y"].astype(np.float64)
    scale = np.abs(X).T @ np.abs(Y) * np.exp(p["logsigma"].astype(np.float64))[None, :] + np.abs(p["mu"])[None, :]
    for v in p["batch_views"]:
        sl = slice(v["start1"] - 1, v["stop1"])
        has = v["batch_of_row"] >= 0
        idx = np.ix_(has, np.arange(sl.start, sl.stop))
        scale[idx] = (scale[idx] - np.abs(p["mu"][sl])[None, :]) * np.exp(v["logdelta"][v["batch_of_row"][has]]) \
            + np.abs(p["mu"][sl])[None, :] + np.abs(v["theta"][v["batch_of_row"][has]])
    err = np.abs(Z - Zo)
    tol = (K + 8) * 2.0 ** -24 * scale + 1e-30
    assert np.all(err <= tol), float(np.max(err / tol))
