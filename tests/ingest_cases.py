"""Cases and CPU references for the data ingest (tests/test_gpu_data_ingest.py): k_tile_D, alloc_tiled_D, tile_from_device and
the two entry points pmf_set_data and pmf_set_data_device, the twenty lines that write the tile-major device copy of D which
every kernel of the library reads.

Nothing here touches the GPU.  What a case's device checks rest on is asserted in tests/test_ingest_cases.py.  Every reference
is exact: the stored matrix is D itself (f32) or its round-to-nearest-even bf16 image with NaN kept NaN (bf16), bit for bit."""
import numpy as np

from problems import make_problem
from test_gpu_split_bf16 import bf16_round

K = 5
# a ragged last row block, a ragged last 32-column tile, N on either side of the 64-column pad
DEVICE_SHAPES = [(1, 1), (31, 63), (33, 65), (70, 173), (257, 129)]
STORES = ("f32", "bf16")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def stored(D, store):
    """What the device holds after set_data(D, store), as f32; NaN where the entry is missing THERE (not finite as stored)."""
    S = np.asarray(D, np.float32) if store == "f32" else bf16_round(D)
    return np.where(np.isfinite(S), S, np.float32(np.nan)).astype(np.float32)


def problem(M, N, seed=0, nan_frac=0.1, clean_tile=None, one_nan_tile=None):
    """problems.make_problem at K = 5 with column parameters and weights, all columns normal, and a mask of its own: about
    nan_frac of the entries NaN (none at 1 x 1), the 32 x 32 tile `clean_tile` = (row block, column block) left all-finite and
    the tile `one_nan_tile` with exactly one NaN."""
    p = make_problem(M=M, N=N, K=K, seed=100 + seed, col_params=True, weights=True, scale=0.5)
    D = np.array(p["D"], order="F")
    rng = np.random.default_rng(7000 + 31 * M + N + seed)
    miss = rng.random((M, N)) < nan_frac
    if M * N == 1:
        miss[:] = False
    for t in (clean_tile, one_nan_tile):
        if t is not None:
            miss[32 * t[0]:32 * t[0] + 32, 32 * t[1]:32 * t[1] + 32] = False
    if one_nan_tile is not None:
        miss[32 * one_nan_tile[0] + 9, 32 * one_nan_tile[1] + 21] = True
    D[miss] = np.nan
    p["D"] = D
    return p


_DEVICE = {}


def device_case(M, N):
    """The problem of a shape of DEVICE_SHAPES (built once, never changed).  70 x 173 has the all-finite tile (0, 1) and the tile
    (1, 2) with a single NaN."""
    if (M, N) not in _DEVICE:
        kw = dict(clean_tile=(0, 1), one_nan_tile=(1, 2)) if (M, N) == (70, 173) else {}
        _DEVICE[(M, N)] = problem(M, N, **kw)
    return _DEVICE[(M, N)]


def col_major_flat(D):
    """The memory of the column-major M x N matrix as a flat float32 vector (what a device-resident source holds)."""
    return np.ascontiguousarray(np.asarray(D, np.float32).T).ravel()


# ---- bf16 rounding at the edges ------------------------------------------------------------------------------------------
# (class, f32 bits, the bf16 bits that round-to-nearest-even stores; None: NaN, stays missing).  The expected halves are
# written out by hand, not computed: tests/test_ingest_cases.py holds bf16_round and torch's CPU cast to them.
BF16_TABLE = [
    ("tie_even", 0x3F808000, 0x3F80), ("tie_odd", 0x3F818000, 0x3F82),
    ("tie_even_neg", 0xBF808000, 0xBF80), ("tie_odd_neg", 0xBF818000, 0xBF82),
    ("below_tie", 0x3F807FFF, 0x3F80), ("above_tie", 0x3F808001, 0x3F81),
    ("below_tie", 0x3F817FFF, 0x3F81), ("above_tie", 0x3F818001, 0x3F82),
    ("below_tie", 0xBF817FFF, 0xBF81), ("above_tie", 0xBF808001, 0xBF81),
    ("binade", 0x3FFF8000, 0x4000), ("binade", 0x3FFFFFFF, 0x4000), ("binade", 0xBFFF8000, 0xC000),
    ("overflow", 0x7F7FFFFF, 0x7F80), ("overflow", 0xFF7FFFFF, 0xFF80), ("overflow", 0x7F7F8000, 0x7F80),
    ("largest", 0x7F7F7FFF, 0x7F7F), ("largest", 0xFF7F7FFF, 0xFF7F),
    ("zero", 0x00000000, 0x0000), ("zero", 0x80000000, 0x8000),
    ("subnormal", 0x00000001, 0x0000), ("subnormal", 0x00008000, 0x0000), ("subnormal", 0x00018000, 0x0002),
    ("subnormal", 0x007FFFFF, 0x0080), ("subnormal", 0x80018000, 0x8002), ("subnormal", 0x00010000, 0x0001),
    ("nan", 0x7FC00000, None), ("nan", 0x7F800001, None), ("nan", 0x7F80FFFF, None), ("nan", 0x7FA00000, None),
    ("nan", 0xFFC00001, None),
]
BF16_CLASSES = ("tie_even", "tie_odd", "tie_even_neg", "tie_odd_neg", "below_tie", "above_tie", "binade", "overflow",
                "largest", "zero", "subnormal", "nan")
BF16_SHAPE = (70, 70)


def bf16_table_index():
    """Which table entry sits at (i, j) of the 70 x 70 matrix: (7 i + j) mod 31.  31 is odd and prime, so inside every full
    32 x 32 tile, and inside the ragged tiles of the last row block and the last column block, each pattern meets even and odd
    columns: both 16-bit halves of the packed pairs of pmf_d_off16."""
    i, j = np.indices(BF16_SHAPE)
    return (7 * i + j) % len(BF16_TABLE)


def bf16_table_matrix():
    """-> (D, want): the 70 x 70 f32 matrix of the table's patterns, Fortran-ordered, and what bf16 storage holds for it as f32
    bits, NaN where the rounded value is not finite (missing on the device)."""
    idx = bf16_table_index()
    src = np.array([b for _, b, _ in BF16_TABLE], np.uint32)
    half = np.array([0x7FC0 if h is None else h for _, _, h in BF16_TABLE], np.uint32)
    D = np.asfortranarray(from_bits(src[idx]))
    want = from_bits(half[idx] << 16)
    want = np.where(np.isfinite(want), want, np.float32(np.nan)).astype(np.float32)
    return D, np.asfortranarray(want)


# ---- non-finite entries --------------------------------------------------------------------------------------------------
INF_SHAPE = (70, 100)
INF_AT = [(5, 40, np.inf), (0, 0, -np.inf), (31, 31, np.inf), (32, 32, -np.inf), (69, 99, np.inf), (69, 0, -np.inf),
          (40, 64, np.inf), (63, 95, -np.inf), (64, 63, np.inf), (17, 96, -np.inf)]
BIG_COL, BIG_ROWS, BIG = 7, (3, 4), np.float32(3.4e38)


def inf_case():
    """-> (p, D_inf, D_nan): the 70 x 100 problem whose tile (0, 1) is all-finite, its matrix with +-Inf written over the
    observed entries INF_AT, (5, 40) being the only non-finite entry of tile (0, 1), and the same matrix with NaN there."""
    p = problem(*INF_SHAPE, seed=3, clean_tile=(0, 1))
    base = p["D"]
    D_inf, D_nan = np.array(base, order="F"), np.array(base, order="F")
    for i, j, v in INF_AT:
        if (i, j) != (5, 40):
            base[i, j] = D_inf[i, j] = D_nan[i, j] = 1.0     # observed before it is overwritten, whatever the mask drew
        D_inf[i, j] = v
        D_nan[i, j] = np.nan
    return p, D_inf, D_nan


def big_case():
    """The matrix of inf_case's problem with 3.4e38 and -3.4e38 in column BIG_COL: finite in f32, beyond the bf16 overflow
    point 0x7f7f8000 = 3.3961775e38 (the tie between the largest bf16 and 2^128), so Inf = missing under bf16 storage."""
    p = problem(*INF_SHAPE, seed=3, clean_tile=(0, 1))
    D = np.array(p["D"], order="F")
    D[BIG_ROWS[0], BIG_COL], D[BIG_ROWS[1], BIG_COL] = BIG, -BIG
    return D


# ---- chunked host upload -------------------------------------------------------------------------------------------------
CHUNK_SHAPE = (70, 173)
CHUNK_FLOATS = [70 * 33, 70 * 64, 70, 10]      # seams inside 32-column tiles; at the pad width; one column; below M: max(1, 0)
CHUNK_DEFAULT = 64 << 20
REAL_SHAPE = ((1 << 20) + 3, 70)
REAL_ROWS = [(1, 64), ((1 << 19) - 31, (1 << 19) + 32), ((1 << 20) + 3 - 66, (1 << 20) + 3)]   # 1-based, inclusive


def chunks(M, N, chunk_floats=CHUNK_DEFAULT):
    """The (first column, columns) of every round of pmf_set_data's upload loop."""
    c = max(1, min(N, chunk_floats // max(M, 1)))
    return [(c0, min(c, N - c0)) for c0 in range(0, N, c)]


def real_size_case():
    """-> (D, n, s, sq): the (2^20 + 3) x 70 matrix with entries from {0, 1, 2, 3} and 10 % NaN, Fortran-ordered (280 MiB), and
    per column the count of observed entries, their sum and their sum of squares as integers.  Every partial sum stays below
    2^24, so a float32 sum is exact in any order."""
    M, N = REAL_SHAPE
    rng = np.random.default_rng(41)
    vals = rng.integers(0, 4, size=(N, M), dtype=np.uint8)
    miss = rng.integers(0, 10, size=(N, M), dtype=np.uint8) == 0
    Dt = vals.astype(np.float32)
    Dt[miss] = np.nan
    v = np.where(miss, np.uint8(0), vals)
    return Dt.T, M - miss.sum(1), v.sum(1, dtype=np.int64), (v * v).sum(1, dtype=np.int64)


# ---- buffer reuse --------------------------------------------------------------------------------------------------------
# (M, N, store, compare the data pass with a fresh context's)
REUSE_STEPS = [(70, 60, "f32", False), (70, 50, "f32", True), (70, 50, "bf16", False), (70, 50, "f32", True),
               (70, 64, "f32", False), (40, 64, "f32", False), (70, 60, "f32", True)]


def reuse_problem(step):
    M, N, _, _ = REUSE_STEPS[step]
    return problem(M, N, seed=10 + step)
