"""The data ingest: k_tile_D, alloc_tiled_D, tile_from_device, pmf_set_data and pmf_set_data_device (csrc/pmf_hip.hip), the
lines that write the tile-major device copy of D which every kernel reads.  A wrong ingest gives finite, plausible numbers in
every downstream test, so it is checked here on its own, on the cases of tests/ingest_cases.py:

  1. a device-resident source (pmf_set_data_device with a real pointer): ragged shapes, both stores, the source overwritten
     after the call, an unaligned source, an adopted stream;
  2. bf16 storage at the rounding edges: ties, binade crossings, overflow, subnormals, NaNs with a low payload;
  3. +-Inf and bf16 overflow are missing entries, like NaN;
  4. the multi-chunk branch of pmf_set_data, through PMF_SET_DATA_CHUNK_FLOATS and once at the real chunk size;
  5. the data buffer kept across pmf_set_data calls of one padded shape and store;
  6. the Python binding's marshalling of C-ordered, float64 and strided arrays.

The device matrix is read back with impute(KEEP_OBSERVED): observed entries come back as stored, missing ones as the
prediction.  Every assertion is exact: bits or integers, no tolerance."""
import time

import numpy as np
import pytest

import ingest_cases as ic
from ingest_cases import bits
from impute_ref import KEEP
from problems import to_context
from test_gpu_parity import grads_of

pytestmark = pytest.mark.gpu

BOTH = dict(update_X=True, update_Y=True)


def check_readback(ctx, want, rows=None, where=""):
    """The KEEP read-back (of the 1-based inclusive row range `rows`, default all) against `want`, the stored matrix as f32
    with NaN at the entries that are missing on the device: observed entries bit for bit, missing ones the prediction."""
    r = (1, want.shape[0]) if rows is None else rows
    want = want[r[0] - 1:r[1]]
    base = ctx.impute(0, *r)
    got = ctx.impute(KEEP, *r)
    obs = ~np.isnan(want)
    assert got.shape == want.shape, where
    assert np.array_equal(bits(got)[obs], bits(want)[obs]), f"{where}: an observed entry is not returned as stored"
    assert np.array_equal(bits(got)[~obs], bits(base)[~obs]), f"{where}: a missing entry is not the prediction"
    return got


def check_col_n(ctx, want, where=""):
    n = ctx.stats(use_factors=False)["n"]
    assert np.array_equal(n, (~np.isnan(want)).sum(0).astype(np.float32)), where


def data_pass(ctx, p):
    loss, g = grads_of(ctx, p, **BOTH)
    return loss, g["X"], g["Y"], ctx.last_kernel()


def assert_same_pass(a, b, where=""):
    assert a[3] == b[3], f"{where}: kernel families {a[3]} and {b[3]}"
    assert a[0] == b[0], f"{where}: loss {a[0]!r} and {b[0]!r}"
    assert np.array_equal(bits(a[1]), bits(b[1])), f"{where}: gX differs"
    assert np.array_equal(bits(a[2]), bits(b[2])), f"{where}: gY differs"
    assert np.isfinite(a[0]) and np.isfinite(a[1]).all() and np.isfinite(a[2]).all(), where


def device_source(D, offset=0):
    """-> (tensor, address): the column-major memory of D on the device, `offset` floats into its allocation."""
    import torch
    flat = torch.from_numpy(ic.col_major_flat(D))
    buf = torch.full((flat.numel() + offset,), float("nan"), dtype=torch.float32, device="cuda")
    buf[offset:].copy_(flat)
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + 4 * offset


def bare(ctx, M, N):
    """K = 1 zero factors, identity column layers, no batch views, all columns normal: what a read-back needs."""
    ctx.set_precision("f32")
    ctx.set_factors(np.zeros((1, M), np.float32), np.zeros((1, N), np.float32))
    ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
    ctx.set_batch_views([])
    ctx.set_noise([(1, N)], ["normal"])


def load_params(ctx, p):
    """The problem's parameters (and its matrix as f32, which fixes the shape); exact f32 precision."""
    to_context(p, ctx)
    ctx.set_precision("f32")


def set_params_only(c, p):
    """The problem's parameters without another upload of its matrix (problems.to_context uploads it first)."""
    c.set_precision("f32")
    c.set_factors(p["X"], p["Y"])
    c.set_col_params(p["logsigma"], p["mu"])
    c.set_batch_views(p["batch_views"])
    c.set_noise(p["noise_ranges"], p["noise_kinds"], p["col_weight"])
    c.clear_xreg()
    c.clear_yreg()
    c.set_layer_regs()


# ---- 1. a device-resident source -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ic.STORES)
@pytest.mark.parametrize("M,N", ic.DEVICE_SHAPES)
def test_device_source_is_the_host_upload(ctx, M, N, store):
    """pmf_set_data_device of a real pointer stores what pmf_set_data of the same matrix stores, and it has copied: the source
    overwritten with NaN after the call changes neither the data pass nor the read-back."""
    import torch
    p = ic.device_case(M, N)
    want = ic.stored(p["D"], store)
    load_params(ctx, p)
    ctx.set_data(p["D"], store=store)
    check_readback(ctx, want, where="host upload")
    host = data_pass(ctx, p)
    buf, ptr = device_source(p["D"])
    ctx.set_data_device(ptr, M, N, store=store)
    check_readback(ctx, want, where="device source")
    check_col_n(ctx, want, "device source")
    dev = data_pass(ctx, p)
    assert_same_pass(dev, host, "device source against host upload")
    buf.fill_(float("nan"))
    torch.cuda.synchronize()
    assert_same_pass(data_pass(ctx, p), host, "after the source was overwritten")
    check_readback(ctx, want, where="after the source was overwritten")
    check_col_n(ctx, want, "after the source was overwritten")


@pytest.mark.parametrize("store", ic.STORES)
@pytest.mark.parametrize("M,N", [(33, 65), (257, 129)])
def test_unaligned_device_source(ctx, M, N, store):
    """A source one float into its allocation with odd M: the column starts fall on every 4-byte phase of 16 bytes.  k_tile_D
    reads scalars, so this holds today; a vectorised read would have to keep it."""
    p = ic.device_case(M, N)
    want = ic.stored(p["D"], store)
    load_params(ctx, p)
    ctx.set_data(p["D"], store=store)
    host = data_pass(ctx, p)
    buf, ptr = device_source(p["D"], offset=1)
    assert M % 2 == 1 and ptr % 16 == 4 and {(ptr + 4 * j * M) % 16 for j in range(N)} == {0, 4, 8, 12}
    ctx.set_data_device(ptr, M, N, store=store)
    check_readback(ctx, want, where="unaligned source")
    check_col_n(ctx, want, "unaligned source")
    assert_same_pass(data_pass(ctx, p), host, "unaligned source against host upload")


@pytest.mark.parametrize("store", ic.STORES)
def test_device_source_on_an_adopted_stream(pkg, store):
    """The copy runs on the context's stream: adopted from torch, it gives the bits of the library's own stream."""
    import torch
    M, N = 70, 173
    p = ic.device_case(M, N)
    want = ic.stored(p["D"], store)
    c = pkg.Context(0)
    try:
        load_params(c, p)
        buf, ptr = device_source(p["D"])
        c.set_data_device(ptr, M, N, store=store)
        own = data_pass(c, p)
        check_readback(c, want, where="own stream")
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            try:
                c.set_stream(torch.cuda.current_stream().cuda_stream)
                buf2, ptr2 = device_source(p["D"])
                c.set_data_device(ptr2, M, N, store=store)
                assert_same_pass(data_pass(c, p), own, "adopted stream against own stream")
                check_readback(c, want, where="adopted stream")
                check_col_n(c, want, "adopted stream")
            finally:
                c.use_own_stream()
        assert_same_pass(data_pass(c, p), own, "back on the own stream")
    finally:
        c.close()


# ---- 2. bf16 rounding at the edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["host", "device"])
def test_bf16_rounding_edges(ctx, route):
    """Ties to even on even and odd mantissas of both signs, one ulp either side, round-up into the next binade, overflow to
    Inf (= missing), the largest bf16, signed zeros, f32 subnormals kept (not flushed), and every NaN, the ones whose payload
    sits only in the low 16 bits included, still missing.  The expected halves are written out by hand in ingest_cases."""
    D, want = ic.bf16_table_matrix()
    M, N = D.shape
    if route == "host":
        ctx.set_data(D, store="bf16")
    else:
        buf, ptr = device_source(D)
        ctx.set_data_device(ptr, M, N, store="bf16")
    bare(ctx, M, N)
    got = check_readback(ctx, want, where=route)
    check_col_n(ctx, want, route)
    # (said again per class, so that a failure names it)
    idx = ic.bf16_table_index()
    for t, (cls, b, h) in enumerate(ic.BF16_TABLE):
        g = np.unique(bits(got)[idx == t])
        if h is not None and np.isfinite(ic.from_bits([h << 16])[0]):
            assert g.tolist() == [h << 16], (cls, hex(b), [hex(int(x)) for x in g])
    ctx.set_data(D)      # f32 storage holds the patterns themselves, subnormals and signed zeros included
    check_readback(ctx, ic.stored(D, "f32"), where="f32")
    check_col_n(ctx, ic.stored(D, "f32"), "f32")


# ---- 3. non-finite entries are missing -----------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ic.STORES)
def test_inf_is_missing(ctx, store):
    """+Inf and -Inf over observed entries, one of them the only non-finite entry of its tile: counts, loss, gradients and the
    read-back are those of the same matrix with NaN there."""
    p, D_inf, D_nan = ic.inf_case()
    want = ic.stored(D_nan, store)
    load_params(ctx, p)
    res = []
    for D in (D_nan, D_inf):
        ctx.set_data(D, store=store)
        check_readback(ctx, want)
        check_col_n(ctx, want)
        res.append(data_pass(ctx, p))
    assert_same_pass(res[1], res[0], "Inf against NaN")


def test_bf16_overflow_is_missing(ctx):
    """3.4e38 is finite in f32 and beyond the bf16 overflow point: observed under f32 storage, missing under bf16."""
    D = ic.big_case()
    M, N = D.shape
    j = ic.BIG_COL
    ctx.set_data(D, store="f32")
    bare(ctx, M, N)
    got = check_readback(ctx, ic.stored(D, "f32"))
    assert got[ic.BIG_ROWS[0], j] == ic.BIG and got[ic.BIG_ROWS[1], j] == -ic.BIG
    n32 = ctx.stats(use_factors=False)["n"]
    assert n32[j] == np.isfinite(D[:, j]).sum()
    ctx.set_data(D, store="bf16")
    check_readback(ctx, ic.stored(D, "bf16"))
    n16 = ctx.stats(use_factors=False)["n"]
    assert n16[j] == n32[j] - 2 and np.array_equal(np.delete(n16, j), np.delete(n32, j))
    ctx.set_data(D)


# ---- 4. chunked host upload ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ic.STORES)
def test_chunked_upload_is_the_one_chunk_upload(ctx, store, monkeypatch):
    M, N = ic.CHUNK_SHAPE
    p = ic.device_case(M, N)
    want = ic.stored(p["D"], store)
    monkeypatch.delenv("PMF_SET_DATA_CHUNK_FLOATS", raising=False)
    load_params(ctx, p)
    ctx.set_data(p["D"], store=store)
    whole_rb = check_readback(ctx, want, where="one chunk")
    whole = data_pass(ctx, p)
    for n in ic.CHUNK_FLOATS:
        assert len(ic.chunks(M, N, n)) > 1
        monkeypatch.setenv("PMF_SET_DATA_CHUNK_FLOATS", str(n))
        ctx.set_data(p["D"], store=store)
        got = check_readback(ctx, want, where=f"chunks of {n} floats")
        assert np.array_equal(bits(got), bits(whole_rb))
        check_col_n(ctx, want, f"chunks of {n} floats")
        assert_same_pass(data_pass(ctx, p), whole, f"chunks of {n} floats")


def test_the_chunk_hook_is_read(pkg, monkeypatch):
    """The staging buffer is allocated at exactly M x chunk floats (DevBuf::ensure), so the bytes a fresh context holds after
    its first upload say which chunk ran: without the hook M x N floats of staging, with 70 floats one column of it."""
    M, N = ic.CHUNK_SHAPE
    D = ic.device_case(M, N)["D"]
    held = {}
    for n in (None, 70, 70 * 33):
        if n is None:
            monkeypatch.delenv("PMF_SET_DATA_CHUNK_FLOATS", raising=False)
        else:
            monkeypatch.setenv("PMF_SET_DATA_CHUNK_FLOATS", str(n))
        c = pkg.Context(0)
        try:
            before = pkg._lib.live_bytes()[0]
            c.set_data(D)
            held[n] = pkg._lib.live_bytes()[0] - before
        finally:
            c.close()
    assert held[None] - held[70] == 4 * M * (N - 1) and held[None] - held[70 * 33] == 4 * M * (N - 33), held


def test_upload_at_the_real_chunk_size(ctx, monkeypatch):
    """(2^20 + 3) x 70, 280 MiB: two chunks of 63 and 7 columns under the library's own 64 Mi floats, and k_fill past its
    65536-workgroup cap.  Entries from {0, 1, 2, 3}: the column sums are exact in f32 in any order, so they are compared as
    integers; three row ranges of at most 67 rows are read back.  Wall time, printed: 0.4 s on an MI355X host, nearly all of it
    building the matrix and its integer reference on the host; the upload itself takes 0.01 s."""
    monkeypatch.delenv("PMF_SET_DATA_CHUNK_FLOATS", raising=False)
    t0 = time.perf_counter()
    D, n, s, sq = ic.real_size_case()
    M, N = D.shape
    assert D.flags.f_contiguous and D.dtype == np.float32
    t1 = time.perf_counter()
    ctx.set_data(D)
    t2 = time.perf_counter()
    bare(ctx, M, N)
    st = ctx.stats(use_factors=False)
    assert np.array_equal(st["n"].astype(np.int64), n)
    assert np.array_equal(st["sum"].astype(np.int64), s) and np.array_equal(st["sum"], s.astype(np.float32))
    assert np.array_equal(st["sumsq"].astype(np.int64), sq) and np.array_equal(st["sumsq"], sq.astype(np.float32))
    for r in ic.REAL_ROWS:
        check_readback(ctx, D, rows=r, where=f"rows {r}")
    t3 = time.perf_counter()
    print(f"real-size upload: case {t1 - t0:.2f} s, set_data {t2 - t1:.2f} s, checks {t3 - t2:.2f} s, total {t3 - t0:.2f} s")
    ctx.set_data(np.zeros((1, 1), np.float32))      # give the 280 MiB back


# ---- 5. the buffer kept across set_data calls ----------------------------------------------------------------------------
def test_buffer_reuse_leaves_nothing_behind(pkg):
    """alloc_tiled_D keeps the buffer when M, the padded N and the store are unchanged.  Seven uploads on one context: a
    narrower matrix into the kept buffer (columns 51..60 of the first one must be gone), a store switch and back, the pad width
    itself, fewer rows, and the first shape again.  tests/test_gpu_history.py switches the store at one shape as well (its
    poisoned history), but compares only after a re-marshal at another shape; steps 3 and 4 stay here because step 4's
    comparison with a fresh context needs the f32 buffer re-made after the bf16 one."""
    c = pkg.Context(0)
    try:
        for i, (M, N, store, against_fresh) in enumerate(ic.REUSE_STEPS):
            p = ic.reuse_problem(i)
            want = ic.stored(p["D"], store)
            where = f"step {i + 1}: {M} x {N} {store}"
            c.set_data(p["D"], store=store)      # ONE upload per step, straight over the previous step's matrix
            set_params_only(c, p)
            check_readback(c, want, where=where)
            check_col_n(c, want, where)
            if against_fresh:
                got = data_pass(c, p)
                f = pkg.Context(0)
                try:
                    load_params(f, p)
                    f.set_data(p["D"], store=store)
                    assert_same_pass(got, data_pass(f, p), where + " against a fresh context")
                finally:
                    f.close()
    finally:
        c.close()


# ---- 6. the Python binding -----------------------------------------------------------------------------------------------
def test_binding_marshals_any_array_layout(ctx):
    """set_data of a C-ordered array, a float64 array and a strided slice stores the bits of the Fortran float32 copy."""
    big = ic.device_case(257, 129)["D"]
    M, N = 70, 43
    src = {"c_order": np.ascontiguousarray(big[:M, :N]), "float64": big[:M, :N].astype(np.float64),
           "strided": big[:2 * M:2, :3 * N:3]}
    assert src["c_order"].flags.c_contiguous and not src["c_order"].flags.f_contiguous
    assert not src["strided"].flags.f_contiguous and not src["strided"].flags.c_contiguous
    for name, A in src.items():
        assert A.shape == (M, N)
        F = np.asfortranarray(A.astype(np.float32))
        want = ic.stored(F, "f32")
        assert np.isnan(want).any() and not np.isnan(want).all()
        ctx.set_data(F)
        bare(ctx, M, N)
        ref = check_readback(ctx, want, where=name + ": Fortran float32 copy")
        ctx.set_data(A)
        got = check_readback(ctx, want, where=name)
        assert np.array_equal(bits(got), bits(ref)), name
        check_col_n(ctx, want, name)
