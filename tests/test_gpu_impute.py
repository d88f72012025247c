"""pmf_impute / pmf_impute_device / pmf_impute_entries on the device, against the fp64 restatement of tests/impute_ref.py
(per-entry bounds derived there) and, where the contract says so, bit for bit: row ranges, chunk heights, ld, the device
output, repeated calls, history of the context, precision mode, and a fit before or after.

pmf_impute_kernel<KB, NW, DB> works on absolute 32-row blocks in panels of 32 NW rows (NW = 8 up to K = 64, 4 above) and
units of two 32-column tiles; the shapes below sit on those edges.  They all leave the persistent grid at one unit per
workgroup and one panel per unit: the unit and grid edges live in tests/test_gpu_output_grid.py."""
import ctypes as C

import numpy as np
import pytest

import debatch_ref as dref
from impute_ref import (BATCH, CASES, FLAG_SETS, KEEP, LINK, case_problem, impute_ref, impute_tol, kinds_of, scale_of,
                        worst_ratio)
from problems import rel_err, to_context
from test_gpu_layer_edges import layer_problem, rows
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def check_tol(ctx, p, flags, cols=None):
    """Every entry of the device's matrix inside its bound (restricted to `cols` when given); returns the matrix."""
    got = ctx.impute(flags)
    want, z = impute_ref(p, flags)
    tol = impute_tol(p, flags, z)
    sl = slice(None) if cols is None else cols
    r = worst_ratio(got[:, sl], want[:, sl], tol[:, sl])
    assert r <= 1.0, f"flags={flags}: worst |error| / bound = {r}"
    return got


# ---- 1. K, M and N edges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", CASES)
def test_k_and_shape_edges(ctx, K, M, N):
    p = case_problem(K, M, N)
    to_context(p, ctx)
    for flags in FLAG_SETS:
        got = check_tol(ctx, p, flags)
        assert got.shape == (M, N) and got.dtype == np.float32


# ---- 2. batch views and the default -----------------------------------------------------------------------------------
def test_batch_views_are_ignored_without_batch(ctx):
    p = case_problem(64, 300, 129)
    to_context(p, ctx)
    with_views = ctx.impute(0).copy()
    with_views_b = ctx.impute(BATCH).copy()
    to_context(dict(p, batch_views=[]), ctx)
    assert same_bits(with_views, ctx.impute(0))
    assert same_bits(ctx.impute(0), ctx.impute(BATCH))          # no views: BATCH changes nothing
    assert not same_bits(with_views, with_views_b)               # ... and with views it does


def test_agrees_with_pmf_forward(ctx):
    for K, M, N in ((32, 300, 129), (97, 300, 65)):
        p = case_problem(K, M, N)
        to_context(p, ctx)
        Z = ctx.forward().astype(np.float64)
        got = ctx.impute(BATCH | LINK).astype(np.float64)
        ez = (K + 8) * 2.0 ** -24 * scale_of(p, BATCH)
        r = worst_ratio(got, Z, 2 * ez)          # the same quantity in another sum order: each within e_z of the truth
        assert r <= 1.0, r


def batch_edge_problem(name):
    if name == "std_views":          # rows with batch -1 at 0, 3, M - 1; boundaries inside tiles; a scrambled view of 15
        return case_problem(32, 300, 129)
    if name == "300_batches":        # more than 255 batches: no dense table anywhere in the library, the gather path
        M, N = 320, 129
        rng = np.random.default_rng(5)
        p = layer_problem(M, N, 20, 91, [(1, 40, rows(M, 300, "scrambled", rng), 300), (50, 100, rows(M, 6, "sorted", rng), 6)])
        p["batch_views"][0]["batch_of_row"][[0, 3, M - 1]] = -1
        return p
    if name == "bernoulli_view":     # layer_problem puts the Bernoulli columns first: round(0.2 N) = 26 of them
        M, N = 300, 129
        rng = np.random.default_rng(6)
        p = layer_problem(M, N, 40, 92, [(1, 26, rows(M, 7, "scrambled", rng), 7)])
        assert np.all(kinds_of(p)[:26] == 1) and kinds_of(p)[26] != 1
        return p
    raise KeyError(name)


@pytest.mark.parametrize("name", ["std_views", "300_batches", "bernoulli_view"])
def test_batch_edges(ctx, name):
    p = batch_edge_problem(name)
    to_context(p, ctx)
    for flags in (BATCH, BATCH | LINK):
        check_tol(ctx, p, flags)
    if name == "300_batches":
        assert ctx.last_path()["slots"] == 0          # the library built no dense table for this model
        r, c = np.array([0, 3, 319, 17, 200]), np.array([0, 39, 5, 40, 99])
        e = ctx.impute_entries(r + 1, c + 1, BATCH)
        want, z = impute_ref(p, BATCH)
        assert worst_ratio(e, want[r, c], impute_tol(p, BATCH, z)[r, c]) <= 1.0


# ---- 3. KEEP_OBSERVED -------------------------------------------------------------------------------------------------
def keep_problem(variant):
    p = case_problem(33, 300, 129, seed=311)
    if variant == "nan_row_and_column":
        p["D"][37, :] = np.nan
        p["D"][:, 70] = np.nan
        p["D"][299, :] = np.nan
    elif variant == "nothing_missing":
        p["D"] = np.asfortranarray(np.where(np.isnan(p["D"]), np.float32(0.25), p["D"]))
    return p


@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["five_percent", "nan_row_and_column", "nothing_missing"])
def test_keep_observed(ctx, variant, store):
    p = keep_problem(variant)
    to_context(p, ctx)
    try:
        if store == "bf16":
            ctx.set_data(p["D"], store="bf16")
        stored = p["D"] if store == "f32" else bf16_round(p["D"])
        obs = np.isfinite(p["D"])
        assert obs.all() == (variant == "nothing_missing")
        for flags in (0, BATCH, LINK | BATCH):
            base = ctx.impute(flags).copy()
            got = ctx.impute(flags | KEEP)
            assert np.array_equal(bits(got)[obs], bits(stored)[obs]), "an observed entry is not returned as stored"
            assert np.array_equal(bits(got)[~obs], bits(base)[~obs]), "a missing entry is not the prediction"
            assert np.isfinite(got).all()
    finally:
        ctx.set_data(p["D"])     # back to f32 storage for the tests that share the context


# ---- 4. ranges, ld, chunks, device output ------------------------------------------------------------------------------
RANGES = [(1, 1), (1, 31), (2, 33), (32, 32), (33, 64), (257, 300), (300, 300), (1, 300)]


@pytest.fixture(scope="module")
def range_case(ctx):
    p = case_problem(64, 300, 129, seed=411)
    return p


def test_row_ranges_are_the_rows_of_the_full_call(ctx, range_case):
    p = range_case
    to_context(p, ctx)
    for flags in (0, BATCH, KEEP):
        full = ctx.impute(flags).copy()
        for s1, e1 in RANGES:
            got = ctx.impute(flags, s1, e1)
            assert got.shape == (e1 - s1 + 1, p["N"])
            assert same_bits(got, full[s1 - 1:e1]), (flags, s1, e1)
    # at K > 64 the panel is 128 rows: ranges around its edge
    p = case_problem(97, 300, 65, seed=412)
    to_context(p, ctx)
    full = ctx.impute(BATCH).copy()
    for s1, e1 in [(128, 129), (129, 129), (97, 160), (257, 300)]:
        assert same_bits(ctx.impute(BATCH, s1, e1), full[s1 - 1:e1]), (s1, e1)


def test_ld_padding_is_left_alone(ctx, range_case):
    p = range_case
    to_context(p, ctx)
    full = ctx.impute(BATCH).copy()
    for s1, e1 in [(2, 33), (1, 300), (300, 300)]:
        n = e1 - s1 + 1
        out = np.full((n + 5, p["N"]), SENTINEL, np.float32, order="F")
        ctx.impute(BATCH, s1, e1, out=out, out_row=0)
        assert same_bits(out[:n], full[s1 - 1:e1])
        assert np.all(out[n:] == SENTINEL), "padding rows were written"
        out = np.full((n + 5, p["N"]), SENTINEL, np.float32, order="F")
        ctx.impute(BATCH, s1, e1, out=out, out_row=3)
        assert same_bits(out[3:3 + n], full[s1 - 1:e1]) and np.all(out[:3] == SENTINEL) and np.all(out[3 + n:] == SENTINEL)


@pytest.mark.parametrize("chunk", [1, 31, 32, 100, 1000])
def test_chunk_heights_do_not_change_a_bit(ctx, range_case, monkeypatch, chunk):
    p = range_case
    to_context(p, ctx)
    monkeypatch.delenv("PMF_IMPUTE_CHUNK_ROWS", raising=False)
    for flags, (s1, e1) in ((0, (1, 300)), (BATCH | KEEP, (2, 290))):
        monkeypatch.delenv("PMF_IMPUTE_CHUNK_ROWS", raising=False)
        want = ctx.impute(flags, s1, e1).copy()
        monkeypatch.setenv("PMF_IMPUTE_CHUNK_ROWS", str(chunk))
        out = np.full((e1 - s1 + 6, p["N"]), SENTINEL, np.float32, order="F")
        ctx.impute(flags, s1, e1, out=out)
        assert same_bits(out[:e1 - s1 + 1], want) and np.all(out[e1 - s1 + 1:] == SENTINEL), (flags, chunk)


def test_device_output(ctx, range_case):
    import torch
    p = range_case
    to_context(p, ctx)
    N = p["N"]
    for flags, (s1, e1) in ((0, (1, 300)), (BATCH, (33, 64)), (KEEP | BATCH, (2, 290))):
        n = e1 - s1 + 1
        want = ctx.impute(flags, s1, e1).copy()
        t = torch.full((N, n + 5), float(SENTINEL), dtype=torch.float32, device="cuda")    # column-major (n + 5) x N
        torch.cuda.synchronize()
        ctx.impute_device(t.data_ptr(), flags, s1, e1, ld=n + 5)
        got = t.cpu().numpy().T
        assert same_bits(got[:n], want), (flags, s1, e1)
        assert np.all(got[n:] == SENTINEL)


# ---- 5. listed entries -------------------------------------------------------------------------------------------------
def test_entries(ctx):
    p = case_problem(65, 300, 129, seed=511)
    M, N = p["M"], p["N"]
    to_context(p, ctx)
    rng = np.random.default_rng(7)
    r = np.concatenate([rng.integers(0, M, 990), [0, 0, M - 1, M - 1], [5, 5, 5, 0, 3, M - 1]])
    c = np.concatenate([rng.integers(0, N, 990), [0, N - 1, 0, N - 1], [9, 9, 9, 2, 2, 2]])
    assert r.size == 1000
    for flags in FLAG_SETS:
        want, z = impute_ref(p, flags)
        tol = impute_tol(p, flags, z)
        got = ctx.impute_entries(r + 1, c + 1, flags)
        assert got.shape == (1000,) and got.dtype == np.float32
        ratio = worst_ratio(got, want[r, c], tol[r, c])
        assert ratio <= 1.0, (flags, ratio)
        assert got[994] == got[995] == got[996]                         # duplicates
        one = ctx.impute_entries(r[:1] + 1, c[:1] + 1, flags)
        assert one.shape == (1,) and bits(one)[0] == bits(got)[0]
        assert ctx.impute_entries(np.zeros(0, np.int64), np.zeros(0, np.int64), flags).shape == (0,)
    assert ctx.lib.pmf_impute_entries(ctx._h, 0, C.c_int64(0), None, None, None) == 0


def test_entry_chunk_seam(ctx):
    """pmf_impute_entries and pmf_remove_batch_effect_entries stage 1 << 22 entries at a time: three entries more than one
    chunk, so that a second round runs with the staging buffer carved for the first.  Every entry against the full matrix of
    the fp64 restatements under their own bounds, and bit for bit the two calls that stop and start at the seam: an entry's
    bits do not depend on the chunk it falls in."""
    CH, M, N = 1 << 22, 70, 100
    rng = np.random.default_rng(2207)
    bor = rows(M, 3, "sorted", rng)
    bor[[0, 3, 41, M - 1]] = -1                                  # rows in no batch
    p = layer_problem(M, N, 8, 2208, [(10, 77, bor, 3)])         # columns outside the view on both sides, mixed noise kinds
    assert {0, 1, 2} <= set(kinds_of(p).tolist())
    to_context(p, ctx)
    D = np.asarray(p["D"], np.float32)
    n = CH + 3
    r, c = rng.integers(0, M, n), rng.integers(0, N, n)
    r[[CH - 1, CH, CH + 2]], c[[CH - 1, CH, CH + 2]] = (5, 69, 41), (11, 76, 99)
    r1, c1, v = r + 1, c + 1, D[r, c]
    want, z = impute_ref(p, BATCH)
    wd, _, _ = dref.debatch_ref(p, D, 0)
    calls = [("impute", lambda s: ctx.impute_entries(r1[s], c1[s], BATCH), worst_ratio, want, impute_tol(p, BATCH, z)),
             ("debatch, given values", lambda s: ctx.remove_batch_effect_entries(r1[s], c1[s], v[s]), dref.worst_ratio, wd,
              dref.debatch_tol(p, D, 0)),
             ("debatch, resident", lambda s: ctx.remove_batch_effect_entries(r1[s], c1[s]), dref.worst_ratio, wd,
              dref.debatch_tol(p, D, 0))]
    for what, call, ratio, ref, tol in calls:
        got = call(slice(None))
        assert got.shape == (n,) and got.dtype == np.float32
        q = ratio(got, ref[r, c], tol[r, c])
        print(f"{what}: worst |error| / bound = {q:.3f}")
        assert q <= 1.0, (what, q)
        assert same_bits(got, np.concatenate([call(slice(0, CH)), call(slice(CH, n))])), what


# ---- 6. saturation ----------------------------------------------------------------------------------------------------
def test_saturation(ctx):
    p = case_problem(32, 70, 129, seed=611)
    kind = kinds_of(p)
    pc, bc = np.flatnonzero(kind == 2), np.flatnonzero(kind == 1)
    assert pc.size >= 2 and bc.size >= 2
    p["mu"][pc[0]], p["mu"][pc[1]] = 100.0, -200.0
    p["mu"][bc[0]], p["mu"][bc[1]] = 200.0, -200.0
    sat = np.array([pc[0], pc[1], bc[0], bc[1]])
    rest = np.setdiff1d(np.arange(p["N"]), sat)
    to_context(p, ctx)
    for flags in (0, BATCH):
        got = check_tol(ctx, p, flags, cols=rest)
        assert not np.isnan(got).any()
        assert np.all(np.isposinf(got[:, pc[0]])) and np.all(got[:, pc[1]] == 0.0)
        assert np.all(got[:, bc[0]] == 1.0) and np.all(got[:, bc[1]] == 0.0)
        e = ctx.impute_entries(np.full(4, 2), sat + 1, flags)
        assert np.isposinf(e[0]) and e[1] == 0.0 and e[2] == 1.0 and e[3] == 0.0


# ---- 7. state -----------------------------------------------------------------------------------------------------------
ALL_FLAGS = [0, BATCH, LINK, BATCH | LINK, KEEP, KEEP | BATCH]


def all_outputs(ctx):
    return [ctx.impute(f).copy() for f in ALL_FLAGS]


def state_problem():
    return case_problem(48, 300, 129, seed=711)


def fresh_outputs(pkg, p, precision="f32"):
    c = pkg.Context(0)
    try:
        to_context(p, c)
        c.set_precision(precision)
        return all_outputs(c)
    finally:
        c.close()


def assert_all_same(a, b):
    for f, u, v in zip(ALL_FLAGS, a, b):
        assert same_bits(u, v), f"flags={f}"


def test_two_calls_and_precision_mode(pkg):
    p = state_problem()
    c = pkg.Context(0)
    try:
        to_context(p, c)
        a = all_outputs(c)
        assert_all_same(a, all_outputs(c))
        c.set_precision("bf16x3")
        assert_all_same(a, all_outputs(c))
        # ... and after a data pass in that mode has filled the context's operand images
        c.epoch_begin(c.make_opts(update_X=True, update_Y=True))
        c.epoch_loss()
        assert_all_same(a, all_outputs(c))
    finally:
        c.close()


def test_impute_after_fit_is_impute_of_the_fitted_model(pkg):
    p = state_problem()
    c = pkg.Context(0)
    try:
        to_context(p, c)
        c.set_optimizer("adagrad", lr=0.05)
        c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=5, abs_tol=0, rel_tol=0)
        after = all_outputs(c)
        X, Y = c.get_factors()
        ls, mu = c.get_col_params()
        views = []
        for v, bv in enumerate(p["batch_views"]):
            ld, th = c.get_batch_view(v)
            views.append(dict(bv, logdelta=ld, theta=th))
    finally:
        c.close()
    assert not np.array_equal(X, p["X"]) and not np.array_equal(mu, p["mu"])
    q = dict(p, X=X, Y=Y, logsigma=ls, mu=mu, batch_views=views)
    assert_all_same(after, fresh_outputs(pkg, q))
    got, (want, z) = after[1], impute_ref(q, BATCH)
    assert worst_ratio(got, want, impute_tol(q, BATCH, z)) <= 1.0


def test_fit_after_impute_is_the_fit_without_it(pkg):
    p = state_problem()
    res = []
    for with_impute in (False, True):
        c = pkg.Context(0)
        try:
            to_context(p, c)
            c.set_optimizer("adagrad", lr=0.05)
            if with_impute:
                all_outputs(c)
                c.impute_entries([1, 2, 300], [1, 129, 5], BATCH)
                c.impute(BATCH, 3, 77)
            r = c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=3, abs_tol=0, rel_tol=0)
            if with_impute:
                all_outputs(c)
            st = [c.get_opt_state(w)[0] for w in ("X", "Y", "mu", "logsigma")]
            st += [c.get_opt_state("theta", v)[0] for v in range(len(p["batch_views"]))]
            res.append((r["loss"], *c.get_factors(), *c.get_col_params(), *st))
        finally:
            c.close()
    for u, v in zip(*res):
        assert np.array_equal(u, v)


def test_history_of_the_context_does_not_matter(pkg):
    p = state_problem()
    want = fresh_outputs(pkg, p)
    big = case_problem(128, 700, 300, seed=712)
    big["X"][:] = np.nan
    c = pkg.Context(0)
    try:
        for store in ("f32", "bf16"):
            to_context(big, c)
            c.set_data(big["D"], store=store)
            all_outputs(c)
            c.impute_entries([1, 700], [1, 300], BATCH)
        # the target's own shape with NaN factors right before it
        to_context(p, c)
        c.set_factors(np.full_like(p["X"], np.nan), np.full_like(p["Y"], np.nan))
        assert np.isnan(c.impute(0)).all()
        c.set_factors(p["X"], p["Y"])
        assert_all_same(want, all_outputs(c))
    finally:
        c.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def refused(ctx, rc, *words):
    assert rc != 0
    msg = ctx.lib.pmf_last_error().decode()
    assert all(w in msg for w in words), msg


def test_refusals_leave_the_context_usable(pkg):
    p = case_problem(20, 70, 40, seed=811)
    M, N = p["M"], p["N"]
    out = np.full((M, N), SENTINEL, np.float32, order="F")
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    i64 = lambda *v: np.array(v, np.int64)    # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))    # noqa: E731
    c = pkg.Context(0)
    try:
        L, h = c.lib, c._h
        call = lambda fl, s, e, o, ld: L.pmf_impute(h, fl, C.c_int64(s), C.c_int64(e), o, C.c_int64(ld))    # noqa: E731
        calld = lambda fl, s, e, o, ld: L.pmf_impute_device(h, fl, C.c_int64(s), C.c_int64(e), o, C.c_int64(ld))    # noqa: E731
        ent = lambda fl, r, cc, o: L.pmf_impute_entries(h, fl, C.c_int64(len(r)), ip(r), ip(cc), o)    # noqa: E731
        # nothing set at all
        refused(c, call(KEEP, 1, 1, op, 1), "KEEP_OBSERVED", "data")
        refused(c, call(0, 1, 1, op, 1), "factors not set")
        refused(c, ent(0, i64(1), i64(1), op), "factors not set")
        c.set_data(p["D"])
        refused(c, call(0, 1, M, op, M), "factors not set")
        refused(c, calld(0, 1, M, op, M), "factors not set")
        to_context(p, c)
        good = c.impute(BATCH).copy()
        one = i64(1)
        for attempt, words in [
            (lambda: call(0, 1, M, None, M), ("null output",)),
            (lambda: calld(0, 1, M, None, M), ("null output",)),
            (lambda: ent(0, one, one, None), ("null output",)),
            (lambda: call(8, 1, M, op, M), ("flag",)),
            (lambda: call(-1, 1, M, op, M), ("flag",)),
            (lambda: calld(16 | BATCH, 1, M, op, M), ("flag",)),
            (lambda: ent(32, one, one, op), ("flag",)),
            (lambda: call(0, 0, M, op, M), ("row range",)),
            (lambda: call(0, 1, M + 1, op, M + 1), ("row range",)),
            (lambda: call(0, 5, 4, op, M), ("row range",)),
            (lambda: calld(0, M + 1, M + 1, op, M), ("row range",)),
            (lambda: call(0, 1, M, op, M - 1), ("ld",)),
            (lambda: call(0, 3, 10, op, 7), ("ld",)),
            (lambda: calld(0, 1, M, op, 0), ("ld",)),
            (lambda: ent(KEEP, one, one, op), ("KEEP_OBSERVED",)),
            (lambda: ent(0, i64(1, 0), i64(1, 1), op), ("outside",)),
            (lambda: ent(0, i64(M + 1), one, op), ("outside",)),
            (lambda: ent(0, one, i64(0), op), ("outside",)),
            (lambda: ent(BATCH, i64(1, M), i64(1, N + 1), op), ("outside",)),
            (lambda: L.pmf_impute_entries(h, 0, C.c_int64(-1), ip(one), ip(one), op), ("n=",)),
        ]:
            refused(c, attempt(), *words)
            assert np.all(out == SENTINEL), "a refused call wrote to the output"
            assert same_bits(c.impute(BATCH), good)              # the context is still usable
        assert L.pmf_impute_entries(h, KEEP | 64, C.c_int64(0), None, None, None) == 0   # n = 0: nothing to do
    finally:
        c.close()


# ---- 9. the Python level ------------------------------------------------------------------------------------------------
def test_python_level(pkg):
    import test_gpu_host as th
    model = th.reference_fit_setup(pkg, seed=5)
    rng = np.random.default_rng(8)
    mf = model.matfac
    mf.X[...] = 0.5 * rng.standard_normal(mf.X.shape)
    mf.Y[...] = 0.5 * rng.standard_normal(mf.Y.shape)
    M, N = model.data.shape
    try:
        out = pkg.impute(model)
        assert out.shape == (M, N) and out.dtype == np.float32
        ctx = model.device_context()
        assert same_bits(out, ctx.impute(0))
        outb = pkg.impute(model, include_batch_effects=True, link=True)
        assert same_bits(outb, ctx.impute(BATCH | LINK))
        assert rel_err(outb, th.oracle_of(model).forward()) <= 1e-5
        assert same_bits(pkg.impute(model, keep_observed=True), ctx.impute(KEEP))
        assert same_bits(pkg.impute(model, rows=range(3, 37)), out[3:37])
        assert same_bits(pkg.impute(model, rows=(39, 40)), out[39:40])
        calls = []
        real = ctx.impute
        ctx.impute = lambda *a, **k: (calls.append(a[1:3]), real(*a, **k))[1]
        try:
            assert same_bits(pkg.impute(model, capacity=N * 14), out)       # 40 rows in blocks of 14: three calls
        finally:
            del ctx.impute
        assert calls == [(1, 14), (15, 28), (29, 40)], calls
        r, c = np.array([0, 39, 7, 7]), np.array([0, 59, 30, 30])
        e = pkg.impute_entries(model, r, c, include_batch_effects=True)
        assert same_bits(e, ctx.impute_entries(r + 1, c + 1, BATCH))
        assert np.allclose(e, pkg.impute(model, include_batch_effects=True)[r, c], rtol=1e-5, atol=1e-6)
    finally:
        model.release_device()
