"""Host-side conditions on tests/ingest_cases.py: the cases are in the regime they exist for and their references agree with
an independent one.  No GPU."""
import numpy as np
import pytest

import ingest_cases as ic
from test_gpu_split_bf16 import bf16_round


def tiles_of(mask):
    """{(row block, column block): entries of the boolean mask in that 32 x 32 tile}"""
    M, N = mask.shape
    return {(rb, cb): mask[32 * rb:32 * rb + 32, 32 * cb:32 * cb + 32]
            for rb in range((M + 31) // 32) for cb in range((N + 31) // 32)}


# ---- the device-source shapes --------------------------------------------------------------------------------------------
def test_device_shapes_cover_the_ragged_edges():
    assert ic.DEVICE_SHAPES == [(1, 1), (31, 63), (33, 65), (70, 173), (257, 129)]
    Ms, Ns = zip(*ic.DEVICE_SHAPES)
    assert any(m % 32 for m in Ms) and any(n % 32 for n in Ns)
    assert any(n < 64 for n in Ns) and any(64 < n < 128 for n in Ns) and any(n > 128 for n in Ns)
    assert any(m % 2 for m, n in ic.DEVICE_SHAPES if m > 1)    # odd M: the unaligned source meets every 4-byte phase


@pytest.mark.parametrize("M,N", ic.DEVICE_SHAPES)
def test_device_case_mask(M, N):
    p = ic.device_case(M, N)
    D = p["D"]
    assert D.shape == (M, N) and D.dtype == np.float32 and D.flags.f_contiguous
    miss = np.isnan(D)
    assert np.array_equal(miss, ~np.isfinite(D))
    if M * N == 1:
        assert not miss.any()
        return
    assert 0.05 < miss.mean() < 0.15
    assert p["noise_kinds"] == ["normal"] and not p["batch_views"]
    if (M, N) == (70, 173):
        t = tiles_of(miss)
        assert not t[(0, 1)].any() and t[(0, 1)].shape == (32, 32)
        assert t[(1, 2)].sum() == 1 and t[(1, 2)].shape == (32, 32)
    # the flat source is the column-major memory
    flat = ic.col_major_flat(D)
    assert np.array_equal(ic.bits(flat.reshape(N, M).T), ic.bits(D))


# ---- the bf16 table ------------------------------------------------------------------------------------------------------
def test_bf16_table_holds_every_class():
    names = [c for c, _, _ in ic.BF16_TABLE]
    assert set(names) == set(ic.BF16_CLASSES)
    pat = {b for _, b, _ in ic.BF16_TABLE}
    assert len(pat) == len(ic.BF16_TABLE) == 31
    for b in (0x3FFF8000, 0x3FFFFFFF, 0x7F7FFFFF, 0x7F7F7FFF, 0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000,
              0x007FFFFF, 0x7FC00000, 0x7F800001, 0x7F80FFFF, 0x7FA00000, 0xFFC00001):
        assert b in pat, hex(b)
    for c, b, h in ic.BF16_TABLE:
        lo, hi = b & 0xFFFF, b >> 16
        if c.startswith("tie"):
            assert lo == 0x8000 and (hi & 1) == ("odd" in c) and (b >> 31) == ("neg" in c)
        if c == "below_tie":
            assert lo == 0x7FFF and h == hi
        if c == "above_tie":
            assert lo == 0x8001 and h == hi + 1
        if c == "subnormal":
            assert (b & 0x7F800000) == 0 and (b & 0x007FFFFF) != 0
        if c == "nan":
            assert h is None and np.isnan(ic.from_bits([b])[0])
        if c == "overflow":
            assert np.isfinite(ic.from_bits([b])[0]) and np.isinf(ic.from_bits([h << 16])[0])
    assert any(c == "subnormal" and b >> 31 for c, b, _ in ic.BF16_TABLE)
    assert any(c == "nan" and (b & 0xFFFF0000) in (0x7F800000, 0xFF800000) for c, b, _ in ic.BF16_TABLE), \
        "no NaN whose payload sits only in the low 16 bits"


def test_bf16_table_against_bf16_round_and_torch():
    import torch
    src = ic.from_bits([b for _, b, _ in ic.BF16_TABLE])
    ours = bf16_round(src)
    theirs = torch.from_numpy(src.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    for (c, b, h), o, t in zip(ic.BF16_TABLE, ours, theirs):
        if h is None:
            assert np.isnan(o) and np.isnan(t), (c, hex(b))
        else:
            assert ic.bits([o])[0] == ic.bits([t])[0] == h << 16, (c, hex(b), hex(int(ic.bits([o])[0])), hex(int(ic.bits([t])[0])))


def test_bf16_round_against_torch_on_random_bit_patterns():
    import torch
    rng = np.random.default_rng(5)
    src = ic.from_bits(rng.integers(0, 1 << 32, size=1_000_000, dtype=np.uint64).astype(np.uint32))
    ours = bf16_round(src)
    theirs = torch.from_numpy(src.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    nan = np.isnan(src)
    assert nan.any() and np.array_equal(np.isnan(ours), nan) and np.array_equal(np.isnan(theirs), nan)
    assert np.array_equal(ic.bits(ours)[~nan], ic.bits(theirs)[~nan])
    assert ((ic.bits(src) & 0x7F800000) == 0).sum() > 1000      # subnormals and zeros among them


def test_bf16_table_matrix_placement():
    D, want = ic.bf16_table_matrix()
    assert D.shape == want.shape == ic.BF16_SHAPE and D.flags.f_contiguous
    idx = ic.bf16_table_index()
    j = np.indices(ic.BF16_SHAPE)[1]
    n = len(ic.BF16_TABLE)
    for (rb, cb), t in tiles_of(np.ones(ic.BF16_SHAPE, bool)).items():
        sl = (slice(32 * rb, 32 * rb + 32), slice(32 * cb, 32 * cb + 32))
        if rb == 2 and cb == 2:
            continue       # 6 x 6 entries: not every pattern fits
        for par in (0, 1):  # both halves of a packed pair (pmf_d_off16: the low bit of the column)
            assert set(idx[sl][j[sl] % 2 == par]) == set(range(n)), (rb, cb, par)
    # the reference: the hand-written halves, equal to bf16_round wherever that is finite
    r = bf16_round(D)
    fin = np.isfinite(r)
    assert np.array_equal(fin, ~np.isnan(want)) and np.array_equal(ic.bits(r)[fin], ic.bits(want)[fin])
    assert np.array_equal(ic.bits(ic.stored(D, "bf16"))[fin], ic.bits(want)[fin])
    # finite in f32, missing in bf16: the overflow class; and every column has observed and missing entries
    assert (np.isfinite(D) & ~fin).any() and (np.isnan(D) & ~fin).any()
    assert fin.any(axis=0).all() and (~fin).any(axis=0).all()


# ---- non-finite entries --------------------------------------------------------------------------------------------------
def test_inf_case():
    p, D_inf, D_nan = ic.inf_case()
    assert D_inf.shape == ic.INF_SHAPE
    at = np.zeros(ic.INF_SHAPE, bool)
    for i, j, v in ic.INF_AT:
        at[i, j] = True
        assert D_inf[i, j] == v and np.isnan(D_nan[i, j])
    assert np.array_equal(np.isinf(D_inf), at) and (D_inf[at] > 0).any() and (D_inf[at] < 0).any()
    assert np.array_equal(ic.bits(D_inf)[~at], ic.bits(D_nan)[~at])
    t = tiles_of(~np.isfinite(D_inf))
    assert t[(0, 1)].sum() == 1 and not np.isnan(D_inf[:32, 32:64]).any()
    assert 0.05 < np.isnan(D_inf).mean() < 0.15
    for store in ic.STORES:
        assert np.array_equal(ic.bits(ic.stored(D_inf, store)), ic.bits(ic.stored(D_nan, store)))


def test_big_case():
    D = ic.big_case()
    col = D[:, ic.BIG_COL]
    assert col[ic.BIG_ROWS[0]] == ic.BIG and col[ic.BIG_ROWS[1]] == -ic.BIG and np.isfinite(ic.BIG)
    assert ic.bits([ic.BIG])[0] > 0x7F7F8000      # beyond the tie between the largest bf16 and 2^128
    s32, s16 = ic.stored(D, "f32"), ic.stored(D, "bf16")
    for r, v in zip(ic.BIG_ROWS, (ic.BIG, -ic.BIG)):
        assert s32[r, ic.BIG_COL] == v and np.isnan(s16[r, ic.BIG_COL])
    assert np.isfinite(s16).sum() == np.isfinite(s32).sum() - 2


# ---- chunks --------------------------------------------------------------------------------------------------------------
def test_chunk_seams():
    M, N = ic.CHUNK_SHAPE
    assert ic.chunks(M, N) == [(0, N)]
    assert ic.chunks(M, N, 70 * 33)[:2] == [(0, 33), (33, 33)] and len(ic.chunks(M, N, 70 * 33)) == 6
    assert ic.chunks(M, N, 70 * 64) == [(0, 64), (64, 64), (128, 45)]
    assert ic.chunks(M, N, 70) == [(j, 1) for j in range(N)]
    assert ic.chunks(M, N, 10) == [(j, 1) for j in range(N)]            # 10 // 70 = 0 -> max(1, 0)
    assert any(c0 % 32 for c0, _ in ic.chunks(M, N, 70 * 33))            # a seam inside a 32-column tile
    assert ic.chunks(*ic.REAL_SHAPE) == [(0, 63), (63, 7)]
    M, N = ic.REAL_SHAPE
    assert M * N > ic.CHUNK_DEFAULT and (M * N + 255) // 256 > 65536     # two chunks; k_fill past its workgroup cap
    for s1, e1 in ic.REAL_ROWS:
        assert 1 <= s1 <= e1 <= M and e1 - s1 + 1 <= 67
    assert ic.REAL_ROWS[0] == (1, 64) and ic.REAL_ROWS[1] == (2 ** 19 - 31, 2 ** 19 + 32) and ic.REAL_ROWS[2] == (M - 66, M)


def test_real_size_sums_are_exact_in_float32():
    M, N = ic.REAL_SHAPE
    assert 3 * M < 2 ** 24 and 9 * M < 2 ** 24


# ---- buffer reuse --------------------------------------------------------------------------------------------------------
def test_reuse_steps():
    s = ic.REUSE_STEPS
    assert [(m, n, st) for m, n, st, _ in s] == [(70, 60, "f32"), (70, 50, "f32"), (70, 50, "bf16"), (70, 50, "f32"),
                                                 (70, 64, "f32"), (40, 64, "f32"), (70, 60, "f32")]
    assert [i + 1 for i, t in enumerate(s) if t[3]] == [2, 4, 7]
    pad = [(m, (n + 63) // 64 * 64, st) for m, n, st, _ in s]
    assert pad[0] == pad[1] and pad[1] != pad[2] and pad[3] == pad[4] and pad[4] != pad[5] and pad[5] != pad[6]
    for i in range(len(s)):
        p = ic.reuse_problem(i)
        assert p["D"].shape == s[i][:2] and np.isnan(p["D"]).any()
