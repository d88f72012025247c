"""The exact f32 kernel's plain tile loop (pmf_fused.hip.inc, "Plain runs") against the same kernel with every run in the
general loop (PMF_PLAIN=0, read at every pass).

The register-resident cross-wave instances (K in 33..64, both gradients, one noise model, no batch layers) run the tail of
a piece -- the tiles that are all-finite in all eight row blocks, not the matrix's ragged last column tile and not a first
visit of the workgroup's slab entry -- in a second instantiation of the tile loop that no longer asks those questions per
tile.  It issues the same MFMAs on the same operands in the same order, so loss, gX and gY must be BIT-IDENTICAL; only
last_path()["plain_tiles"], counted by the kernel, tells how many tiles took it.  What can go wrong is the choice of the
run: a tile with a missing value, an absent row block, the ragged tile or a first visit inside a plain run (a wrong or
stale table, a wrong split point, relative instead of absolute column tiles under chunks), and the hand-over of the
loop-carried state between the two loops.

Every case computes in f32, must have taken the exact kernel (family 0) and its register-resident instance.
"""
import numpy as np
import pytest

from problems import factor_scales, make_problem, to_context, to_oracle
from test_gpu_exact_xwave import BOTH, check_oracle, eval_both
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

M0, N0, K0 = 4096, 5120, 64          # 16 row panels of 256 rows x 160 column tiles
TILES = 16 * 160
TPS = 8                              # the segment length's floor: what PMF_TPS_SCALE below brings it to


def eval_pair(ctx, p, monkeypatch):
    """(default pass, PMF_PLAIN=0 pass) on one context: ((loss, grads), plain_tiles) of each, the instance asserted."""
    out = []
    for switch in (None, "0"):
        if switch is not None:
            monkeypatch.setenv("PMF_PLAIN", switch)
        loss, g = eval_both(ctx, p)
        lp = ctx.last_path()
        assert lp["xreg"] == 1, lp
        out.append(((loss, g), lp["plain_tiles"]))
    monkeypatch.delenv("PMF_PLAIN")
    assert out[1][1] == 0, out[1][1]          # the switch sends every run to the general loop
    return out[0], out[1]


def assert_bit_equal(a, b):
    (la, ga), (lb, gb) = a, b
    assert la == lb, (la, lb)
    assert np.array_equal(ga["X"], gb["X"]), float(np.abs(ga["X"] - gb["X"]).max())
    assert np.array_equal(ga["Y"], gb["Y"]), float(np.abs(ga["Y"] - gb["Y"]).max())


def short_segments(monkeypatch):
    """Half the CUs and segments of 8 tiles: a workgroup owns about 20 tiles, three or more pieces of one segment."""
    monkeypatch.setenv("PMF_RESERVE_CUS", "128")
    monkeypatch.setenv("PMF_TPS_SCALE", "0.001")


@pytest.fixture(scope="module")
def walk():
    """No missing values, column parameters and weights on.  The oracle's answer is computed once."""
    p = make_problem(M=M0, N=N0, K=K0, seed=51, col_params=True, weights=True)
    _, go = to_oracle(p).loss_and_grads(**BOTH)
    return p, go, factor_scales(p)


@pytest.fixture(scope="module")
def clean_plain_tiles():
    return {}


def test_walk_is_bit_equal_and_matches_oracle(ctx, monkeypatch, walk, clean_plain_tiles):
    p, go, scales = walk
    short_segments(monkeypatch)
    to_context(p, ctx)
    (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    print(f"plain tiles {n_plain} of {TILES}")
    assert 0 < n_plain < TILES, n_plain         # a segment visit's first piece is never plain
    assert_bit_equal(new, old)
    check_oracle(ctx, p, go, new[0], new[1], scales)
    clean_plain_tiles["n"] = n_plain


def test_one_nan_takes_its_pieces_out_of_the_plain_loop(ctx, monkeypatch, walk, clean_plain_tiles):
    """One NaN in row panel 6, column tile 83: with 20 tiles per workgroup that tile lies in the middle of a workgroup's
    range, in a piece that is plain on the clean matrix.  Only pieces that contain the tile may leave the plain loop, and
    they lie in one (segment, row panel) unit of TPS tiles."""
    p, _, _ = walk
    short_segments(monkeypatch)
    if "n" not in clean_plain_tiles:
        to_context(p, ctx)
        eval_both(ctx, p)
        clean_plain_tiles["n"] = ctx.last_path()["plain_tiles"]
    i, j = 6 * 256 + 77, 83 * 32 + 5
    keep = p["D"][i, j]
    p["D"][i, j] = np.nan
    try:
        to_context(p, ctx)
        (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    finally:
        p["D"][i, j] = keep
    print(f"plain tiles {n_plain} with the NaN, {clean_plain_tiles['n']} without")
    assert_bit_equal(new, old)
    assert 0 < clean_plain_tiles["n"] - n_plain <= TPS, (n_plain, clean_plain_tiles["n"])


def test_last_panel_of_one_row_runs_general(ctx, monkeypatch):
    p = make_problem(M=M0 + 1, N=N0, K=K0, seed=52, col_params=True, weights=True)
    short_segments(monkeypatch)
    to_context(p, ctx)
    (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    assert_bit_equal(new, old)
    tab = ctx.plain_table()
    assert tab.shape == (17, 161)
    assert np.array_equal(tab[16], np.arange(161)) and not tab[:16].any()      # seven absent row blocks: never plain
    assert 0 < n_plain <= TILES, n_plain


def test_ragged_last_tile_runs_general(ctx, monkeypatch):
    p = make_problem(M=M0, N=N0 + 10, K=K0, seed=53, col_params=True, weights=True)
    short_segments(monkeypatch)
    to_context(p, ctx)
    (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    assert_bit_equal(new, old)
    assert 0 < n_plain <= 16 * 161 - 16, n_plain     # 161 column tiles: the last one of every row panel is never plain


@pytest.mark.parametrize("M,N", [(256, 64), (257, 33)])
def test_first_visits_only(ctx, monkeypatch, M, N):
    """On the full grid every workgroup owns one tile: every piece is a first visit."""
    p = make_problem(M=M, N=N, K=K0, seed=M + N, col_params=True, weights=True)
    to_context(p, ctx)
    (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    assert n_plain == 0
    assert_bit_equal(new, old)


def test_chunks_index_the_table_by_absolute_tile(ctx, monkeypatch, walk):
    p, _, _ = walk
    short_segments(monkeypatch)
    to_context(p, ctx)
    ctx.comm_set_chunks(2)
    try:
        (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    finally:
        ctx.comm_set_chunks(0)
    assert n_plain > 0
    assert_bit_equal(new, old)


def test_bf16_storage_twin(ctx, monkeypatch, walk):
    p0, _, _ = walk
    p = dict(p0)
    p["D"] = np.asfortranarray(bf16_round(p0["D"]))
    short_segments(monkeypatch)
    to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        (new, n_plain), (old, _) = eval_pair(ctx, p, monkeypatch)
    finally:
        ctx.set_data(p["D"])            # back to f32 storage for the tests that follow
    assert 0 < n_plain < TILES, n_plain
    assert_bit_equal(new, old)


def test_table_follows_the_data_and_fit_is_bit_equal(ctx, monkeypatch, walk):
    """One context: the walk, new factors, then a matrix with NaNs where the first had none -- a table kept from the first
    matrix would leave those tiles in the plain loop.  Then three Adam epochs under both switch values."""
    p0, _, _ = walk
    short_segments(monkeypatch)
    to_context(p0, ctx)
    eval_both(ctx, p0)
    n_clean = ctx.last_path()["plain_tiles"]
    rng = np.random.default_rng(54)
    X2 = (p0["X"] + rng.standard_normal(p0["X"].shape) * 0.5).astype(np.float32)
    ctx.set_factors(X2, p0["Y"])
    p = dict(p0)
    p["X"] = X2
    p["D"] = np.array(p0["D"], order="F", copy=True)
    rows, cols = rng.integers(0, M0, 40), rng.integers(0, N0, 40)
    p["D"][rows, cols] = np.nan
    ctx.set_data(p["D"])
    (new, n_nan), (old, _) = eval_pair(ctx, p, monkeypatch)
    print(f"plain tiles {n_nan} with 40 NaNs, {n_clean} without")
    assert n_nan < n_clean, (n_nan, n_clean)
    assert_bit_equal(new, old)
    traces = []
    for switch in (None, "0"):
        if switch is not None:
            monkeypatch.setenv("PMF_PLAIN", switch)
        to_context(p, ctx)
        ctx.set_optimizer("adam", lr=0.01)
        r = ctx.fit(update_X=True, update_Y=True, max_epochs=3, abs_tol=0, rel_tol=0)
        lp = ctx.last_path()
        assert ctx.last_kernel() == 0 and lp["xreg"] == 1, lp
        assert (lp["plain_tiles"] > 0) == (switch is None), lp
        traces.append((np.asarray(r["loss"], dtype=np.float64), *ctx.get_factors()))
    assert len(traces[0][0]) >= 3, traces[0][0]
    assert np.array_equal(traces[0][0], traces[1][0]), (traces[0][0], traces[1][0])
    assert np.array_equal(traces[0][1], traces[1][1]) and np.array_equal(traces[0][2], traces[1][2])
