"""pmf_remove_batch_effect / _device / _entries on the device, against the fp64 restatement of tests/debatch_ref.py (per-entry
bounds derived there) and, where the contract says so, bit for bit: the input's source, row ranges, chunk heights, ld, in
place, FILL_MISSING against pmf_impute, the entries call against the matrix call, and a fit after the call.

pmf_debatch_kernel<SRC> gives a wave one 32 x 32 tile (absolute 32-row block x column tile) at a time and strides a persistent
grid of four-wave workgroups over the tiles; the shapes below sit on the tile edges and one of them needs more than one stride."""
import ctypes as C

import numpy as np
import pytest

import hinge_ref
from debatch_ref import FILL, LINK, debatch_ref, debatch_tol, has_batch, link_kinds, same_bits, worst_ratio
from impute_ref import BATCH as I_BATCH, LINK as I_LINK, case_problem, impute_ref, impute_tol
from problems import to_context
from test_gpu_impute import batch_edge_problem
from test_gpu_layer_edges import layer_problem, rows
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
FLAG_SETS = [0, LINK, FILL, LINK | FILL]
SHAPES = [(M, 65) for M in (1, 31, 33, 257)] + [(300, N) for N in (1, 33, 65, 129)]
K = 20


def check_plain(got, p, src, flags, what=""):
    """`got` (no FILL_MISSING) against the float64 rule on the input `src`: bounds, NaN pattern, entries returned as given."""
    want, _, _ = debatch_ref(p, src, flags)
    r = worst_ratio(got, want, debatch_tol(p, src, flags))
    print(f"{what} flags={flags}: worst |error| / bound = {r:.3f}")
    assert r <= 1.0, (what, flags, r)
    keep = ~has_batch(p) | (link_kinds(p, flags) == 3)[None, :]
    assert same_bits(got[keep], np.asarray(src, np.float32)[keep]), "an entry outside every batch is not returned as given"


def check_all_flags(ctx, p, src, Z, what=""):
    """The four flag sets on one input (Z = None: the resident matrix, whose values are `src`).  Returns the plain result."""
    obs = np.isfinite(src)
    plain = {}
    for flags in (0, LINK):
        plain[flags] = ctx.remove_batch_effect(flags, Z=Z).copy()
        assert plain[flags].shape == src.shape and plain[flags].dtype == np.float32
        check_plain(plain[flags], p, src, flags, what)
        filled = ctx.remove_batch_effect(flags | FILL, Z=Z)
        pred = ctx.impute(I_LINK if flags & LINK else 0)
        assert same_bits(filled[obs], plain[flags][obs]), "FILL_MISSING changed an observed entry"
        assert same_bits(filled[~obs], pred[~obs]), "FILL_MISSING: a missing entry is not pmf_impute's prediction"
    return plain[0]


def device_matrix(V):
    """A rows x N float32 matrix as a device tensor in column-major order (leading dimension = rows)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(V, np.float32).T)).cuda()


def device_call(ctx, flags, V=None, s1=1, e1=None, pad=0, in_place=False):
    """pmf_remove_batch_effect_device on a device copy of V (None: the resident matrix) -> (rows x N result, padding rows)."""
    import torch
    e1 = ctx.M if e1 is None else e1
    n = e1 - s1 + 1
    z = None if V is None else device_matrix(V)
    if in_place:
        out = z
    else:
        out = torch.full((ctx.N, n + pad), float(SENTINEL), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.remove_batch_effect_device(out.data_ptr(), flags, s1, e1, z_ptr=None if z is None else z.data_ptr(), ldz=n, ld=n + pad)
    got = out.cpu().numpy().T
    return got[:n], got[n:]


# ---- 1. shapes, flags and the three sources ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", SHAPES)
def test_shapes_flags_and_sources(ctx, M, N):
    p = case_problem(K, M, N)
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    resident = check_all_flags(ctx, p, D, None, f"{M}x{N} resident")
    host = check_all_flags(ctx, p, D, D, f"{M}x{N} host")
    assert same_bits(resident, host)
    for flags in FLAG_SETS:
        want = ctx.remove_batch_effect(flags).copy()
        assert same_bits(device_call(ctx, flags, D)[0], want), flags
        assert same_bits(device_call(ctx, flags, None)[0], want), flags


@pytest.mark.parametrize("name", [n for n, _ in hinge_ref.all_problems()])
def test_kind3_layouts(ctx, name):
    p = dict(hinge_ref.all_problems())[name]
    hinge_ref.to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    resident = check_all_flags(ctx, p, D, None, name)
    assert same_bits(resident, ctx.remove_batch_effect(0, Z=D))
    k3 = hinge_ref.kinds_of(p) == 3
    assert k3.any() and same_bits(resident[:, k3], D[:, k3])          # class labels are never touched


def test_fractional_probabilities_and_rates(ctx):
    p = case_problem(K, 300, 129)
    to_context(p, ctx)
    V = impute_ref(p, I_BATCH)[0].astype(np.float32)
    V[np.isnan(p["D"])] = np.nan
    check_all_flags(ctx, p, V, V, "predictions as input")
    # outside a link's domain: NaN, no fault; exact 0 / 1 / 0 counts come back exactly (the data hold them)
    kind = hinge_ref.kinds_of(p)
    W = np.array(p["D"], np.float32)
    W[5:9, kind == 1] = np.float32(1.5)
    W[5:9, kind == 2] = np.float32(-1.0)
    got = ctx.remove_batch_effect(0, Z=W)
    bad = has_batch(p) & (kind != 0)[None, :]
    bad[:5] = False
    bad[9:] = False
    assert bad.any() and np.isnan(got[bad]).all()
    D = np.asarray(p["D"], np.float32)
    got = ctx.remove_batch_effect(0)
    exact = np.isfinite(D) & ((kind == 1)[None, :] | ((kind == 2)[None, :] & (D == 0)))
    assert exact.sum() > 1000 and np.array_equal(got[exact], D[exact])


# ---- 2. batch counts ---------------------------------------------------------------------------------------------------
def test_one_batch_and_three_hundred(ctx):
    M, N = 300, 129
    rng = np.random.default_rng(15)
    p = layer_problem(M, N, K, 93, [(1, 70, rows(M, 1, "sorted", rng), 1)])
    p["batch_views"][0]["batch_of_row"][[0, 3, M - 1]] = -1
    to_context(p, ctx)
    check_all_flags(ctx, p, np.asarray(p["D"], np.float32), None, "nb=1")
    p = batch_edge_problem("300_batches")
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    got = check_all_flags(ctx, p, D, None, "nb=300")
    assert ctx.last_path()["slots"] == 0          # the library built no dense table for this model
    r, c = np.array([0, 3, 319, 17, 200]), np.array([0, 39, 5, 40, 99])
    assert same_bits(ctx.remove_batch_effect_entries(r + 1, c + 1), got[r, c])


# ---- 3. the two stores -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_stores(ctx, store):
    p = case_problem(K, 257, 129, seed=1311)
    to_context(p, ctx)
    try:
        if store == "bf16":
            ctx.set_data(p["D"], store="bf16")
        stored = np.asarray(p["D"], np.float32) if store == "f32" else bf16_round(p["D"])
        resident = check_all_flags(ctx, p, stored, None, store)
        assert same_bits(resident, ctx.remove_batch_effect(0, Z=stored))     # the same values from the host: the same bits
        r, c = np.array([0, 1, 100, 256, 256, 77]), np.array([0, 128, 64, 128, 0, 33])
        assert same_bits(ctx.remove_batch_effect_entries(r + 1, c + 1), resident[r, c])
    finally:
        ctx.set_data(p["D"])     # back to f32 storage for the tests that share the context


# ---- 4. more tiles than one stride of the persistent grid --------------------------------------------------------------
def test_more_tiles_than_cus(ctx):
    p = case_problem(4, 2100, 161, seed=1411)          # 66 x 6 = 396 tiles
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    got = ctx.remove_batch_effect(0).copy()
    check_plain(got, p, D, 0, "2100x161")
    assert same_bits(device_call(ctx, 0, D)[0], got)
    assert same_bits(ctx.remove_batch_effect(0, 5, 2090), got[4:2090])


def test_more_tiles_than_resident_waves(ctx):
    # 66 x 66 = 4356 tiles: above sixteen waves on each of 256 CUs, so waves take a second tile whatever the grid
    M = N = 2100
    rng = np.random.default_rng(16)
    p = layer_problem(M, N, 2, 1412, [(1, 1000, rows(M, 7, "sorted", rng), 7), (1011, N, rows(M, 20, "scrambled", rng), 20)])
    p["batch_views"][0]["batch_of_row"][[0, 3, M - 1]] = -1
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    got = ctx.remove_batch_effect(0).copy()
    check_plain(got, p, D, 0, "2100x2100")
    assert same_bits(device_call(ctx, 0, D)[0], got)


# ---- 5. ranges, chunks, ld, in place -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def range_case():
    return case_problem(K, 257, 129, seed=1511)


def test_row_range_is_the_rows_of_the_full_call(ctx, range_case):
    p = range_case
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    for flags in FLAG_SETS:
        full = ctx.remove_batch_effect(flags).copy()
        for s1, e1 in [(5, 70), (1, 1), (33, 64), (257, 257), (32, 33)]:
            assert same_bits(ctx.remove_batch_effect(flags, s1, e1), full[s1 - 1:e1]), (flags, s1, e1)
            assert same_bits(ctx.remove_batch_effect(flags, s1, e1, Z=D[s1 - 1:e1]), full[s1 - 1:e1]), (flags, s1, e1)
        assert same_bits(device_call(ctx, flags, D[4:70], 5, 70)[0], full[4:70])
        assert same_bits(device_call(ctx, flags, None, 5, 70)[0], full[4:70])


@pytest.mark.parametrize("chunk", [1, 32, 100])
def test_chunk_heights_do_not_change_a_bit(ctx, range_case, monkeypatch, chunk):
    p = range_case
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    for flags in (0, LINK | FILL):
        for Z, (s1, e1) in ((None, (1, 257)), (D[4:250], (5, 250))):
            monkeypatch.delenv("PMF_DEBATCH_CHUNK_ROWS", raising=False)
            want = ctx.remove_batch_effect(flags, s1, e1, Z=Z).copy()
            monkeypatch.setenv("PMF_DEBATCH_CHUNK_ROWS", str(chunk))
            out = np.full((e1 - s1 + 6, p["N"]), SENTINEL, np.float32, order="F")
            ctx.remove_batch_effect(flags, s1, e1, Z=Z, out=out)
            assert same_bits(out[:e1 - s1 + 1], want) and np.all(out[e1 - s1 + 1:] == SENTINEL), (flags, chunk)


def test_ld_padding_is_left_alone(ctx, range_case):
    p = range_case
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    for flags in (0, FILL):
        full = ctx.remove_batch_effect(flags).copy()
        for s1, e1 in [(5, 70), (1, 257)]:
            n = e1 - s1 + 1
            out = np.full((n + 5, p["N"]), SENTINEL, np.float32, order="F")
            ctx.remove_batch_effect(flags, s1, e1, out=out, out_row=3)
            assert same_bits(out[3:3 + n], full[s1 - 1:e1]) and np.all(out[:3] == SENTINEL) and np.all(out[3 + n:] == SENTINEL)
            got, pad = device_call(ctx, flags, D[s1 - 1:e1], s1, e1, pad=5)
            assert same_bits(got, full[s1 - 1:e1]) and np.all(pad == SENTINEL)
            # a host input wider than the range: ldz > rows
            Zw = np.asfortranarray(np.vstack([D[s1 - 1:e1], np.full((7, p["N"]), SENTINEL, np.float32)]))
            o2 = np.zeros((n, p["N"]), np.float32, order="F")
            rc = ctx.lib.pmf_remove_batch_effect(ctx._h, flags, C.c_int64(s1), C.c_int64(e1), Zw.ctypes.data_as(C.POINTER(C.c_float)),
                                                 C.c_int64(n + 7), o2.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(n))
            assert rc == 0 and same_bits(o2, full[s1 - 1:e1])


def test_in_place_equals_out_of_place(ctx, range_case):
    p = range_case
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    for flags in (0, LINK):
        want = ctx.remove_batch_effect(flags, 5, 70).copy()
        buf = np.asfortranarray(D[4:70].copy())
        got = ctx.remove_batch_effect(flags, 5, 70, Z=buf, out=buf)
        assert got is not None and same_bits(buf, want)
        assert same_bits(device_call(ctx, flags, D[4:70], 5, 70, in_place=True)[0], want)
    # the host call stages its input, so FILL_MISSING works in place there too
    want = ctx.remove_batch_effect(FILL, 5, 70).copy()
    buf = np.asfortranarray(D[4:70].copy())
    ctx.remove_batch_effect(FILL, 5, 70, Z=buf, out=buf)
    assert same_bits(buf, want)


# ---- 6. listed entries -------------------------------------------------------------------------------------------------
def test_entries(ctx, range_case):
    p = range_case
    M, N = p["M"], p["N"]
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    rng = np.random.default_rng(17)
    r = np.concatenate([rng.integers(0, M, 990), [0, 0, M - 1, M - 1], [5, 5, 5, 0, 3, M - 1]])
    c = np.concatenate([rng.integers(0, N, 990), [0, N - 1, 0, N - 1], [9, 9, 9, 2, 2, 2]])
    for flags in (0, LINK):
        full = ctx.remove_batch_effect(flags).copy()
        got = ctx.remove_batch_effect_entries(r + 1, c + 1, flags=flags)
        assert got.shape == (1000,) and got.dtype == np.float32
        assert same_bits(got, full[r, c])                                   # the same function of the same inputs: no sum
        assert same_bits(ctx.remove_batch_effect_entries(r + 1, c + 1, D[r, c], flags), full[r, c])
        assert same_bits(got[994:997], np.repeat(got[994], 3))             # duplicates
        assert ctx.remove_batch_effect_entries(np.zeros(0, np.int64), np.zeros(0, np.int64), flags=flags).shape == (0,)
    assert ctx.lib.pmf_remove_batch_effect_entries(ctx._h, 0, C.c_int64(0), None, None, None, None) == 0


# ---- 7. the inverse of the batch layers, on the device -------------------------------------------------------------------
def test_device_identity(ctx):
    import torch
    p = case_problem(33, 300, 129, seed=1711)
    M, N = p["M"], p["N"]
    to_context(p, ctx)
    zb = torch.empty((N, M), dtype=torch.float32, device="cuda")
    z0 = torch.empty((N, M), dtype=torch.float32, device="cuda")
    out = torch.empty((N, M), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.impute_device(zb.data_ptr(), I_BATCH | I_LINK)
    ctx.impute_device(z0.data_ptr(), I_LINK)
    ctx.remove_batch_effect_device(out.data_ptr(), LINK, z_ptr=zb.data_ptr())
    V, want_dev, got = zb.cpu().numpy().T, z0.cpu().numpy().T, out.cpu().numpy().T
    _, z64b = impute_ref(p, I_BATCH | I_LINK)
    want64, z64 = impute_ref(p, I_LINK)
    e_in = impute_tol(p, I_BATCH | I_LINK, z64b)
    tol = debatch_tol(p, V, LINK, e_in=e_in)
    r = worst_ratio(got, want64, tol)
    print(f"device identity against float64: worst |error| / bound = {r:.3f}")
    assert r <= 1.0, r
    r = worst_ratio(got, want_dev, tol + impute_tol(p, I_LINK, z64))
    print(f"device identity against pmf_impute_device(LINK): worst |error| / bound = {r:.3f}")
    assert r <= 1.0, r


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def refused(ctx, rc, *words):
    assert rc != 0
    msg = ctx.lib.pmf_last_error().decode()
    assert all(w in msg for w in words), msg


def test_refusals_leave_the_context_usable(pkg):
    p = case_problem(K, 70, 40, seed=1811)
    M, N = p["M"], p["N"]
    out = np.full((M, N), SENTINEL, np.float32, order="F")
    Z = np.asfortranarray(np.asarray(p["D"], np.float32))
    op, zp = out.ctypes.data_as(C.POINTER(C.c_float)), Z.ctypes.data_as(C.POINTER(C.c_float))
    i64 = lambda *v: np.array(v, np.int64)    # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))    # noqa: E731
    c = pkg.Context(0)
    try:
        L, h = c.lib, c._h
        call = lambda fl, s, e, z, ldz, o, ld: L.pmf_remove_batch_effect(h, fl, C.c_int64(s), C.c_int64(e), z, C.c_int64(ldz), o, C.c_int64(ld))    # noqa: E731,E501
        calld = lambda fl, s, e, z, ldz, o, ld: L.pmf_remove_batch_effect_device(h, fl, C.c_int64(s), C.c_int64(e), z, C.c_int64(ldz), o, C.c_int64(ld))    # noqa: E731,E501
        ent = lambda fl, r, cc, v, o: L.pmf_remove_batch_effect_entries(h, fl, C.c_int64(len(r)), ip(r), ip(cc), v, o)    # noqa: E731
        one = i64(1)
        # nothing set at all
        refused(c, call(0, 1, 1, None, 1, op, 1), "data not set")
        refused(c, calld(0, 1, 1, None, 1, op, 1), "data not set")
        refused(c, ent(0, one, one, None, op), "data not set")
        refused(c, call(0, 1, 1, zp, 1, op, 1), "factors not set")
        c.set_data(p["D"])
        refused(c, call(0, 1, M, None, M, op, M), "factors not set")
        to_context(p, c)
        good = c.remove_batch_effect(0).copy()
        for attempt, words in [
            (lambda: call(0, 1, M, zp, M, None, M), ("null output",)),
            (lambda: calld(0, 1, M, None, M, None, M), ("null output",)),
            (lambda: ent(0, one, one, None, None), ("null output",)),
            (lambda: call(4, 1, M, zp, M, op, M), ("flag",)),
            (lambda: call(-1, 1, M, None, M, op, M), ("flag",)),
            (lambda: calld(8 | LINK, 1, M, None, M, op, M), ("flag",)),
            (lambda: ent(16, one, one, None, op), ("flag",)),
            (lambda: call(0, 0, M, zp, M, op, M), ("row range",)),
            (lambda: call(0, 1, M + 1, zp, M + 1, op, M + 1), ("row range",)),
            (lambda: call(0, 5, 4, None, M, op, M), ("row range",)),
            (lambda: calld(0, M + 1, M + 1, None, M, op, M), ("row range",)),
            (lambda: call(0, 1, M, zp, M, op, M - 1), ("ld",)),
            (lambda: call(0, 3, 10, None, 0, op, 7), ("ld",)),
            (lambda: call(0, 1, M, zp, M - 1, op, M), ("ldz",)),
            (lambda: call(FILL, 3, 10, zp, 7, op, 8), ("ldz",)),
            (lambda: calld(0, 1, M, op, 0, op, M), ("ldz",)),
            (lambda: ent(FILL, one, one, None, op), ("FILL_MISSING",)),
            (lambda: ent(FILL | LINK, one, one, zp, op), ("FILL_MISSING",)),
            (lambda: ent(0, i64(1, 0), i64(1, 1), None, op), ("outside",)),
            (lambda: ent(0, i64(M + 1), one, zp, op), ("outside",)),
            (lambda: ent(LINK, i64(1, M), i64(1, N + 1), None, op), ("outside",)),
            (lambda: L.pmf_remove_batch_effect_entries(h, 0, C.c_int64(-1), ip(one), ip(one), None, op), ("n=",)),
        ]:
            refused(c, attempt(), *words)
            assert np.all(out == SENTINEL), "a refused call wrote to the output"
            assert same_bits(c.remove_batch_effect(0), good)              # the context is still usable
        assert L.pmf_remove_batch_effect_entries(h, FILL | 64, C.c_int64(0), None, None, None, None) == 0   # n = 0: nothing to do
    finally:
        c.close()


def test_device_overlap_is_refused(ctx, range_case):
    import torch
    p = range_case
    to_context(p, ctx)
    M, N = p["M"], p["N"]
    buf = device_matrix(np.nan_to_num(np.asarray(p["D"], np.float32)))
    torch.cuda.synchronize()
    before = buf.clone()
    with pytest.raises(Exception, match="overlap"):
        ctx.remove_batch_effect_device(buf.data_ptr(), FILL, z_ptr=buf.data_ptr())
    with pytest.raises(Exception, match="overlap"):
        ctx.remove_batch_effect_device(buf.data_ptr() + 4, 0, 1, M - 1, z_ptr=buf.data_ptr(), ldz=M, ld=M)
    assert torch.equal(before, buf)
    assert ctx.remove_batch_effect(0).shape == (M, N)


# ---- 9. nothing a fit reads is touched -----------------------------------------------------------------------------------
def test_fit_after_debatch_is_the_fit_without_it(pkg):
    p = case_problem(48, 300, 129, seed=1911)
    D = np.asarray(p["D"], np.float32)
    res = []
    for with_call in (False, True):
        c = pkg.Context(0)
        try:
            to_context(p, c)
            c.set_optimizer("adagrad", lr=0.05)
            if with_call:
                for flags in FLAG_SETS:
                    c.remove_batch_effect(flags)
                    c.remove_batch_effect(flags, 3, 77, Z=D[2:77])
                c.remove_batch_effect_entries([1, 2, 300], [1, 129, 5])
            r = c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=3, abs_tol=0, rel_tol=0)
            st = [c.get_opt_state(w)[0] for w in ("X", "Y", "mu", "logsigma")]
            st += [c.get_opt_state("theta", v)[0] for v in range(len(p["batch_views"]))]
            res.append((r["loss"], *c.get_factors(), *c.get_col_params(), *st))
        finally:
            c.close()
    for u, v in zip(*res):
        assert np.array_equal(u, v)


# ---- 10. the Python level ------------------------------------------------------------------------------------------------
def test_python_level(pkg):
    import test_gpu_host as th
    model = th.reference_fit_setup(pkg, seed=5)
    rng = np.random.default_rng(18)
    mf = model.matfac
    mf.X[...] = 0.5 * rng.standard_normal(mf.X.shape)
    mf.Y[...] = 0.5 * rng.standard_normal(mf.Y.shape)
    M, N = model.data.shape
    try:
        out = pkg.remove_batch_effect(model)
        assert out.shape == (M, N) and out.dtype == np.float32
        ctx = model.device_context()
        assert same_bits(out, ctx.remove_batch_effect(0))
        Z = np.asarray(model.data, np.float32)
        assert same_bits(pkg.remove_batch_effect(model, Z), out)
        assert same_bits(pkg.remove_batch_effect(model, Z, link=True), ctx.remove_batch_effect(LINK))
        filled = pkg.remove_batch_effect(model, fill_missing=True)
        assert same_bits(filled, ctx.remove_batch_effect(FILL)) and np.isfinite(filled).all()
        assert same_bits(pkg.remove_batch_effect(model, rows=range(3, 37)), out[3:37])
        assert same_bits(pkg.remove_batch_effect(model, Z[3:37], rows=(3, 37)), out[3:37])
        assert same_bits(pkg.remove_batch_effect(model, Z, capacity=N * 14), out)      # 40 rows in blocks of 14
        with pytest.raises(ValueError):
            pkg.remove_batch_effect(model, Z[:5])
        r, c = np.array([0, 39, 7, 7]), np.array([0, 59, 30, 30])
        assert same_bits(pkg.remove_batch_effect_entries(model, r, c), out[r, c])
        assert same_bits(pkg.remove_batch_effect_entries(model, r, c, Z[r, c], link=True), ctx.remove_batch_effect(LINK)[r, c])
    finally:
        model.release_device()
