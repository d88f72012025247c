"""pmf_simulate_data / _device / _resident on the device against the numpy twin of tests/simulate_ref.py: the forward is
pmf_impute's bit for bit, the uniforms (missing mask, Bernoulli draws) are the twin's exactly, the normal within a derived
bound, and an entry depends on (parameters, seed, global row, column, noise, frac_missing) alone.

The kernel is pmf_impute_kernel with a sampling epilogue: absolute 32-row blocks in panels of 32 NW rows (NW = 8 up to
K = 64, 4 above), units of two 32-column tiles; the shapes are impute_ref.CASES, which sit on those edges.  The unit and grid
edges (several units per workgroup, several panels per unit), rows past 2^32 and a seed with both words set live in
tests/test_gpu_output_grid.py."""
import ctypes as C

import numpy as np
import pytest

import hinge_ref as hr
import simulate_ref as sr
from impute_ref import BATCH, CASES, KEEP, LINK
from problems import shard_problem, to_context
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. the forward is impute's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", CASES)
def test_forward_identity(ctx, K, M, N):
    p = sr.sim_case(K, M, N)
    to_context(p, ctx)
    out = ctx.simulate_data(seed=9, noise=0.0, frac_missing=0.0)
    assert out.shape == (M, N) and out.dtype == np.float32
    z = ctx.impute(BATCH | LINK)
    kind = sr.kinds_of(p)
    assert same_bits(out[:, kind == 0], z[:, kind == 0])
    assert np.isin(out[:, kind == 1], (0.0, 1.0)).all()


@pytest.mark.parametrize("batch", [True, False])
@pytest.mark.parametrize("name,K", [("A", 20), ("A", 80), ("B", 48), ("B", 128)])
def test_forward_identity_hinge(ctx, name, K, batch):
    p = sr.hinge_case(name, K)
    if not batch:
        p = dict(p, batch_views=[])
    hr.to_context(p, ctx)
    out = ctx.simulate_data(seed=9, noise=0.0, frac_missing=0.0)
    kind = sr.kinds_of(p)
    z, cls = ctx.impute(BATCH | LINK), ctx.impute(BATCH)
    assert same_bits(out[:, kind == 0], z[:, kind == 0])
    assert (kind == 3).any() and same_bits(out[:, kind == 3], cls[:, kind == 3])
    # noise does not enter a class column
    noisy = ctx.simulate_data(seed=9, noise=2.0, frac_missing=0.0)
    assert same_bits(noisy[:, kind == 3], cls[:, kind == 3])


# ---- 2. the normal draw -------------------------------------------------------------------------------------------------
def test_normal_draw_alone(ctx):
    p = sr.sim_case(33, 300, 129)
    M, N = p["M"], p["N"]
    p = dict(p, X=np.zeros_like(p["X"]), mu=np.zeros_like(p["mu"]), batch_views=[], noise_ranges=[(1, N)], noise_kinds=["normal"])
    to_context(p, ctx)
    out = ctx.simulate_data(seed=4, noise=1.0, frac_missing=0.0).astype(np.float64)
    err = np.abs(out - sr.draws(4, M, N)["n"]).max()
    print(f"max |out - n64| = {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("K,M,N", [(32, 300, 129), (97, 300, 65)])
def test_normal_draw_on_a_model(ctx, K, M, N):
    p = sr.sim_case(K, M, N)
    to_context(p, ctx)
    noise = 0.3
    out = ctx.simulate_data(seed=4, noise=noise, frac_missing=0.0).astype(np.float64)
    z = ctx.impute(BATCH | LINK).astype(np.float64)
    c = sr.kinds_of(p) == 0
    err = np.abs(out - (z + noise * sr.draws(4, M, N)["n"]))[:, c]
    bound = (noise * 1e-5 + 2.0 ** -23 * np.abs(out))[:, c]
    print(f"worst |error| / bound = {(err / bound).max():.3f}")
    assert np.all(err <= bound)


# ---- 3. the missing mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.0, 2.0 ** -24, 0.05, 1.0])
def test_missing_mask(ctx, frac):
    p = sr.sim_case(64, 300, 129)
    to_context(p, ctx)
    out = ctx.simulate_data(seed=6, noise=0.1, frac_missing=frac)
    want = sr.missing_mask(sr.draws(6, p["M"], p["N"]), frac)
    assert np.array_equal(np.isnan(out), want)
    assert want.any() == (frac >= 0.05) and want.all() == (frac == 1.0)


# ---- 4. Bernoulli -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", [(32, 300, 129), (97, 300, 65)])
def test_bernoulli(ctx, K, M, N):
    p = sr.sim_case(K, M, N)
    to_context(p, ctx)
    out = ctx.simulate_data(seed=3, noise=0.1, frac_missing=0.0)
    cols = np.flatnonzero(sr.kinds_of(p) == 1)
    z = sr.link_space(p, BATCH)
    p64 = sr.sigmoid64(z[:, cols])
    u4 = sr.draws(3, M, N)["u4"][:, cols]
    near = np.abs(u4 - p64) <= sr.impute_tol(p, BATCH, z)[:, cols]
    got = out[:, cols]
    assert np.isin(got, (0.0, 1.0)).all()
    wrong = (got == 1.0) != (u4 < p64)
    print(f"{cols.size} columns: {near.sum()} near ties, {wrong.sum()} decided the other way")
    assert near.mean() <= 0.01
    assert not np.any(wrong & ~near)


# ---- 5. invariance ------------------------------------------------------------------------------------------------------
OPTS = dict(seed=5, noise=0.3, frac_missing=0.05)
RANGES = [(1, 300), (33, 64), (31, 34), (17, 17), (289, 300)]


@pytest.fixture(scope="module")
def inv_case():
    return sr.sim_case(64, 300, 129, seed=411)


def test_row_ranges_and_ld(ctx, inv_case):
    p = inv_case
    to_context(p, ctx)
    full = ctx.simulate_data(**OPTS).copy()
    assert np.isnan(full).any() and same_bits(full, ctx.simulate_data(**OPTS))         # a second call
    for s1, e1 in RANGES:
        n = e1 - s1 + 1
        assert same_bits(ctx.simulate_data(row_start1=s1, row_stop1=e1, **OPTS), full[s1 - 1:e1]), (s1, e1)
        out = np.full((n + 5, p["N"]), SENTINEL, np.float32, order="F")
        ctx.simulate_data(row_start1=s1, row_stop1=e1, out=out, out_row=3, **OPTS)
        assert same_bits(out[3:3 + n], full[s1 - 1:e1]), (s1, e1)
        assert np.all(out[:3] == SENTINEL) and np.all(out[3 + n:] == SENTINEL), "elements outside the block were written"
    # at K > 64 the panel is 128 rows
    q = sr.sim_case(97, 300, 65, seed=412)
    to_context(q, ctx)
    full = ctx.simulate_data(**OPTS).copy()
    for s1, e1 in [(128, 129), (97, 160), (257, 300)]:
        assert same_bits(ctx.simulate_data(row_start1=s1, row_stop1=e1, **OPTS), full[s1 - 1:e1]), (s1, e1)


@pytest.mark.parametrize("chunk", [1, 32, 33])
def test_chunk_heights(ctx, inv_case, monkeypatch, chunk):
    p = inv_case
    to_context(p, ctx)
    monkeypatch.delenv("PMF_SIMULATE_CHUNK_ROWS", raising=False)
    s1, e1 = (1, 300) if chunk > 1 else (200, 290)
    want = ctx.simulate_data(row_start1=s1, row_stop1=e1, **OPTS).copy()
    monkeypatch.setenv("PMF_SIMULATE_CHUNK_ROWS", str(chunk))
    out = np.full((e1 - s1 + 6, p["N"]), SENTINEL, np.float32, order="F")
    ctx.simulate_data(row_start1=s1, row_stop1=e1, out=out, **OPTS)
    assert same_bits(out[:e1 - s1 + 1], want) and np.all(out[e1 - s1 + 1:] == SENTINEL)


def test_device_output(ctx, inv_case):
    import torch
    p = inv_case
    to_context(p, ctx)
    N = p["N"]
    for s1, e1 in [(1, 300), (31, 34), (289, 300)]:
        n = e1 - s1 + 1
        want = ctx.simulate_data(row_start1=s1, row_stop1=e1, **OPTS).copy()
        t = torch.full((N, n + 5), float(SENTINEL), dtype=torch.float32, device="cuda")    # column-major (n + 5) x N
        torch.cuda.synchronize()
        ctx.simulate_data_device(t.data_ptr(), row_start1=s1, row_stop1=e1, ld=n + 5, **OPTS)
        got = t.cpu().numpy().T
        assert same_bits(got[:n], want), (s1, e1)
        assert np.all(got[n:] == SENTINEL)


def test_history_and_precision_mode(pkg, inv_case):
    p = inv_case
    c = pkg.Context(0)
    try:
        to_context(p, c)
        want = c.simulate_data(**OPTS).copy()
        c.set_optimizer("adagrad", lr=0.05)
        c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=1, abs_tol=0, rel_tol=0)
        assert not same_bits(c.simulate_data(**OPTS), want)           # the fitted model's draw ...
        to_context(p, c)
        assert same_bits(c.simulate_data(**OPTS), want)               # ... and the model's own again, after the fit
        c.set_precision("bf16x3")
        assert same_bits(c.simulate_data(**OPTS), want)
        c.epoch_begin(c.make_opts(update_X=True, update_Y=True))
        c.epoch_loss()
        assert same_bits(c.simulate_data(**OPTS), want)
    finally:
        c.close()


# ---- 6. global rows -----------------------------------------------------------------------------------------------------
def test_shards_concatenate(ctx):
    p = sr.sim_case(33, 300, 65)
    to_context(p, ctx)
    whole = ctx.simulate_data(**OPTS).copy()
    parts = []
    for lo, hi in ((0, 131), (131, 300)):
        to_context(shard_problem(p, lo, hi), ctx)
        parts.append(ctx.simulate_data(row_offset=lo, **OPTS).copy())
        if lo:
            assert not same_bits(ctx.simulate_data(row_offset=0, **OPTS), whole[lo:hi])
    assert same_bits(np.concatenate(parts), whole)


# ---- 7. seeds -----------------------------------------------------------------------------------------------------------
def test_seeds(ctx, inv_case):
    to_context(inv_case, ctx)
    kw = dict(noise=0.3, frac_missing=0.05)
    a, b, c = (ctx.simulate_data(seed=s, **kw).copy() for s in (1, 2, 1 + 2 ** 32))
    assert not same_bits(a, b) and not same_bits(a, c) and not same_bits(b, c)
    assert same_bits(a, ctx.simulate_data(seed=1, **kw))


# ---- 8 / 9. the resident matrix -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("K,M,N", [(33, 257, 65), (64, 300, 129)])
def test_resident_is_set_data_of_the_host_matrix(pkg, K, M, N, store):
    p = sr.sim_case(K, M, N)
    res = []
    for resident in (True, False):
        c = pkg.Context(0)
        try:
            to_context(p, c)
            H = c.simulate_data(**OPTS).copy()
            if resident:
                c.set_data(p["D"], store=store)
                c.simulate_data_resident(**OPTS)
                stored = H if store == "f32" else bf16_round(H)
                got = c.impute(KEEP | BATCH | LINK)
                obs = np.isfinite(H)
                assert obs.any() and not obs.all()
                assert np.array_equal(bits(got)[obs], bits(stored)[obs])
                assert np.array_equal(bits(got)[~obs], bits(c.impute(BATCH | LINK))[~obs])
            else:
                c.set_data(H, store=store)
            c.set_optimizer("adagrad", lr=0.05)
            loss = c.loss()
            st = c.stats(use_factors=True)
            r = c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=1, abs_tol=0, rel_tol=0)
            res.append((np.array([loss["total"], loss["data"]]), st["n"], st["sqerr"], r["loss"], *c.get_factors()))
        finally:
            c.close()
    for u, v in zip(*res):
        assert np.array_equal(u, v)


# ---- 10. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(pkg):
    p = sr.sim_case(20, 70, 40, seed=811)
    M, N = p["M"], p["N"]
    out = np.full((M, N), SENTINEL, np.float32, order="F")
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    c = pkg.Context(0)
    try:
        L, h = c.lib, c._h

        def call(o, s=1, e=M, ptr=op, ld=M, fn=L.pmf_simulate_data):
            return fn(h, C.byref(o) if o is not None else None, C.c_int64(s), C.c_int64(e), ptr, C.c_int64(ld))

        def refused(rc, *wds):
            assert rc != 0
            msg = L.pmf_last_error().decode()
            assert all(w in msg for w in wds), msg

        good_o = c.sim_opts(seed=5, noise=0.3, frac_missing=0.05)
        refused(call(good_o), "factors not set")
        refused(L.pmf_simulate_data_resident(h, C.byref(good_o)), "factors not set")
        to_context(p, c)
        good = c.simulate_data(**OPTS).copy()
        so = c.sim_opts
        for attempt, wds in [
            (lambda: call(None), ("null options",)),
            (lambda: call(good_o, ptr=None), ("null output",)),
            (lambda: call(good_o, ptr=None, fn=L.pmf_simulate_data_device), ("null output",)),
            (lambda: L.pmf_simulate_data_resident(h, None), ("null options",)),
            (lambda: call(so(noise=-0.1)), ("noise",)),
            (lambda: call(so(noise=float("inf"))), ("noise",)),
            (lambda: call(so(noise=float("nan"))), ("noise",)),
            (lambda: call(so(frac_missing=-0.01)), ("frac_missing",)),
            (lambda: call(so(frac_missing=1.01)), ("frac_missing",)),
            (lambda: call(so(frac_missing=float("nan"))), ("frac_missing",)),
            (lambda: call(so(row_offset=-1)), ("row_offset",)),
            (lambda: L.pmf_simulate_data_resident(h, C.byref(so(row_offset=-1))), ("row_offset",)),
            (lambda: call(good_o, s=0), ("row range",)),
            (lambda: call(good_o, e=M + 1, ld=M + 1), ("row range",)),
            (lambda: call(good_o, s=5, e=4), ("row range",)),
            (lambda: call(good_o, s=M + 1, e=M + 1, fn=L.pmf_simulate_data_device), ("row range",)),
            (lambda: call(good_o, ld=M - 1), ("ld",)),
            (lambda: call(good_o, s=3, e=10, ld=7), ("ld",)),
        ]:
            refused(attempt(), *wds)
            assert np.all(out == SENTINEL), "a refused call wrote to the output"
            assert same_bits(c.simulate_data(**OPTS), good)              # the context is still usable
        # a Poisson range: refused by all three entries; the same columns declared normal are accepted again
        kinds = list(p["noise_kinds"])
        c.set_noise(p["noise_ranges"], kinds[:-1] + ["poisson"], p["col_weight"])
        refused(call(good_o), "Poisson")
        refused(call(good_o, fn=L.pmf_simulate_data_device), "Poisson")
        refused(L.pmf_simulate_data_resident(h, C.byref(good_o)), "Poisson")
        assert np.all(out == SENTINEL)
        c.set_noise(p["noise_ranges"], kinds, p["col_weight"])
        assert same_bits(c.simulate_data(**OPTS), good)
        # a declared batch view that was never set
        c.lib.pmf_set_n_batch_views(h, len(p["batch_views"]) + 1)
        refused(call(good_o), "batch view")
        c.set_batch_views(p["batch_views"])
        assert same_bits(c.simulate_data(**OPTS), good)
    finally:
        c.close()
    # the resident entry without a data buffer: nothing was ever uploaded, so it is the readiness check that refuses
    c = pkg.Context(0)
    try:
        assert c.lib.pmf_simulate_data_resident(c._h, C.byref(c.sim_opts())) != 0
    finally:
        c.close()


# ---- 11. the Python level -----------------------------------------------------------------------------------------------
def test_python_round_trip(pkg):
    M, N, K = 96, 70, 4
    views = ["mrnaseq"] * 40 + ["mutation"] * 30
    dists = ["normal"] * 30 + ["ordinal_sq_hinge3"] * 10 + ["bernoulli_sq_hinge"] * 30
    rng = np.random.default_rng(3)

    def build():
        return pkg.make_model(np.zeros((M, N), np.float32), K=K, sample_conditions=["a"] * 48 + ["b"] * 48,
                              feature_views=views, feature_distributions=dists,
                              batch_dict={"mrnaseq": ["b1"] * 30 + ["b2"] * 66}, Y_ard=True, rng=np.random.default_rng(0))

    model = build()
    pkg.simulate_params_(model, rng)
    frac = 0.1
    try:
        D = pkg.simulate_data_(model, noise=0.1, seed=21, frac_missing=frac, to="host", capacity=N * 25)
        assert D is not None and D.shape == (M, N) and np.shares_memory(D, model.data)
        nm = model.matfac.noise_model
        for r, name in zip(nm.col_ranges, nm.noises):
            v = D[:, r.start - 1:r.stop]
            v = v[np.isfinite(v)]
            if name == "bernoulli_sq_hinge":
                assert np.isin(v, (0.0, 1.0)).all() and len(np.unique(v)) == 2
            elif name == "ordinal_sq_hinge3":
                assert np.isin(v, (1.0, 2.0, 3.0)).all()
            else:
                assert len(np.unique(v)) > v.size // 2
        share = np.isnan(D).mean()
        assert abs(share - frac) <= 5 * np.sqrt(frac * (1 - frac) / D.size), share
        whole = D.copy()
        assert same_bits(pkg.simulate_data_(model, noise=0.1, seed=21, frac_missing=frac), whole)       # one block
        part = pkg.simulate_data_(model, noise=0.1, seed=21, frac_missing=frac, rows=(31, 34))
        assert same_bits(part, whole[31:34])
        kw = dict(lr=0.05, max_epochs=3, update_X=True, update_Y=True, verbosity=0, abs_tol=0, rel_tol=0)
        h_host = pkg.mf_fit_(model, **kw)
        # the same model again, its data drawn on the device: the host array stays zero and the fit starts from the same loss
        other = build()
        pkg.simulate_params_(other, np.random.default_rng(3))
        try:
            assert pkg.simulate_data_(other, noise=0.1, seed=21, frac_missing=frac, to="device") is None
            assert not other.data.any()
            h_dev = pkg.mf_fit_(other, **kw)
            assert h_dev["loss"][0] == h_host["loss"][0]
        finally:
            other.release_device()
    finally:
        model.release_device()
