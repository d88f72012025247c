"""pmf_impute_kernel past one grid of workgroups: impute, simulate_data (the SimEpi epilogue) and the FILL_MISSING half of
remove_batch_effect on the two problems of tests/output_grid_cases.py, whose shapes follow the device's CU count.

Every other shape of the suite leaves the kernel at one unit per workgroup and one panel per unit.  Here a workgroup walks
several units (the barrier at the loop top, the re-staging of Ys / Cmu / Cmt / Cbase, tk[] computed again, nt going from 2 to
1), a unit sweeps two panels with its waves' private X and batch panels reused, the panels split unevenly over R < n_rp ranges
(case A), and a ragged tail gives only some workgroups a second unit (case B).  The checks are those of test_gpu_impute.py and
test_gpu_simulate.py: per entry against the fp64 restatement under impute_tol, bit for bit wherever the contract says so, the
uniforms against the numpy twin exactly.  The regime is asserted, never assumed.  The last section holds the Philox counter and
key to 64 bits on the device: rows across 2^32 and a seed with both words set.

The problems and their fp64 references are built once per module and never changed."""
import numpy as np
import pytest

import output_grid_cases as og
import simulate_ref as sr
from debatch_ref import FILL
from impute_ref import BATCH, FLAG_SETS, KEEP, LINK, impute_ref, impute_tol, worst_ratio
from problems import shard_problem, to_context
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
NOISE = 0.3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Case:
    """A problem, its grid at the device's CU count, the fp64 references of the flag sets its tests use, and (on first use)
    the twin's draws under og.SEED."""

    def __init__(self, name, cu):
        self.name, self.cu = name, cu
        self.shape = og.shape_a(cu) if name == "A" else og.shape_b(cu)
        self.grid = (og.regime_a if name == "A" else og.regime_b)(*self.shape, cu)
        self.p = sr.sim_case(*self.shape)
        self.kind = sr.kinds_of(self.p)
        self.ref = {}
        for flags in ((BATCH, LINK) if name == "A" else FLAG_SETS):
            want, z = impute_ref(self.p, flags)
            self.ref[flags] = (want, impute_tol(self.p, flags, z))
            if flags == BATCH:
                self.z = z
        self._draws = None

    @property
    def draws(self):
        if self._draws is None:
            self._draws = sr.draws(og.SEED, self.p["M"], self.p["N"])
        return self._draws


@pytest.fixture(scope="module")
def cases():
    import torch
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    return {name: Case(name, cu) for name in ("A", "B")}


def load(ctx, case):
    to_context(case.p, ctx)
    return case.p


# ---- 0. the regime -------------------------------------------------------------------------------------------------------
def test_the_cases_are_past_one_grid(cases):
    a, b = cases["A"], cases["B"]
    ga = og.regime_a(*a.shape, a.cu)
    print(f"A {a.shape} on {a.cu} CUs: {ga}")
    assert ga["units"] >= 4 * ga["grid"] and ga["R"] < ga["n_rp"] and ga["n_ct"] % 2 == 1
    assert any(hi - lo == 2 for lo, hi in ga["panels"])
    og.regime_a(*a.shape, a.cu, 128, a.shape[1])
    gb = og.regime_b(*b.shape, b.cu)
    print(f"B {b.shape} on {b.cu} CUs: {gb}")
    assert gb["grid"] < gb["units"] < 2 * gb["grid"] and gb["R"] == gb["n_rp"]
    # the tile-major store writes the all-pad tile of the odd tile count
    for c in (a, b):
        assert og.impute_grid(*c.shape, c.cu, tile_major=True)["n_ct"] == c.grid["n_ct"] + 1


# ---- 1. impute, per entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags", [("A", BATCH), ("A", LINK)] + [("B", f) for f in FLAG_SETS])
def test_impute_per_entry(ctx, cases, name, flags):
    c = cases[name]
    p = load(ctx, c)
    got = ctx.impute(flags)
    assert got.shape == (p["M"], p["N"]) and got.dtype == np.float32
    want, tol = c.ref[flags]
    r = worst_ratio(got, want, tol)
    print(f"{name} flags={flags}: worst |error| / bound = {r:.3f}")
    assert r <= 1.0, r


# ---- 2. KEEP_OBSERVED ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,store", [("A", "f32"), ("B", "bf16")])
def test_keep_observed(ctx, cases, name, store):
    c = cases[name]
    p = load(ctx, c)
    try:
        if store == "bf16":
            ctx.set_data(p["D"], store="bf16")
        stored = p["D"] if store == "f32" else bf16_round(p["D"])
        obs = np.isfinite(p["D"])
        assert obs.any() and not obs.all()
        base = ctx.impute(BATCH).copy()
        got = ctx.impute(KEEP | BATCH)
        assert np.array_equal(bits(got)[obs], bits(stored)[obs]), "an observed entry is not returned as stored"
        assert np.array_equal(bits(got)[~obs], bits(base)[~obs]), "a missing entry is not the prediction"
    finally:
        ctx.set_data(p["D"])     # back to f32 storage for the tests that share the context


# ---- 3. ranges and chunks are the rows of the full call ------------------------------------------------------------------
@pytest.mark.parametrize("name,ranges", [("A", [(129, 993), (130, 800)]), ("B", [(257, 1800)])])
def test_row_ranges_are_the_rows_of_the_full_call(ctx, cases, name, ranges):
    c = cases[name]
    p = load(ctx, c)
    full = ctx.impute(BATCH).copy()
    for s1, e1 in ranges:
        g = og.impute_grid(*c.shape, c.cu, s1 - 1, e1)
        # panels numbered from panel 1; at A again more units than workgroups (B's 7 x 34 units fit the grid: its range
        # is about rp0 = 1 under eight waves)
        assert g["rp0"] == 1 and (name == "B" or g["units"] > g["grid"]), g
        got = ctx.impute(BATCH, s1, e1)
        assert got.shape == (e1 - s1 + 1, p["N"]) and same_bits(got, full[s1 - 1:e1]), (s1, e1)


def test_chunks_of_300_rows(ctx, cases, monkeypatch):
    c = cases["A"]
    p = load(ctx, c)
    M, N = p["M"], p["N"]
    monkeypatch.delenv("PMF_IMPUTE_CHUNK_ROWS", raising=False)
    full = ctx.impute(BATCH).copy()
    # launches of 3, 3, 4 and 1 panels: another R than the full call's, and again more units than workgroups
    grids = [og.impute_grid(*c.shape, c.cu, r0, min(r0 + 300, M)) for r0 in range(0, M, 300)]
    assert any(g["R"] not in (1, c.grid["R"]) and g["units"] > g["grid"] for g in grids), grids
    monkeypatch.setenv("PMF_IMPUTE_CHUNK_ROWS", "300")
    out = np.full((M + 5, N), SENTINEL, np.float32, order="F")
    ctx.impute(BATCH, out=out)
    assert same_bits(out[:M], full)
    assert np.all(out[M:] == SENTINEL), "padding rows were written"


# ---- 4. remove_batch_effect(FILL_MISSING) runs the same launch -----------------------------------------------------------
def test_debatch_fill_is_impute_on_the_missing_entries(ctx, cases):
    c = cases["A"]
    p = load(ctx, c)
    obs = np.isfinite(p["D"])
    pred = ctx.impute(0).copy()
    plain = ctx.remove_batch_effect(0).copy()
    filled = ctx.remove_batch_effect(FILL)
    assert np.array_equal(np.isnan(plain), ~obs)
    assert np.array_equal(bits(filled)[~obs], bits(pred)[~obs]), "a missing entry is not pmf_impute's prediction"
    assert np.array_equal(bits(filled)[obs], bits(plain)[obs]), "FILL_MISSING changed an observed entry"
    # flags = 0 is not among A's shared references (two flag sets there): built here, for this one check
    want, z = impute_ref(p, 0)
    tol = impute_tol(p, 0, z)
    r = worst_ratio(filled[~obs], want[~obs], tol[~obs])
    print(f"A, filled entries: worst |error| / bound = {r:.3f}")
    assert r <= 1.0, r


# ---- 5. simulate_data, column-major --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_simulate_forward_identity(ctx, cases, name):
    c = cases[name]
    load(ctx, c)
    out = ctx.simulate_data(seed=og.SEED, noise=0.0, frac_missing=0.0)
    z = ctx.impute(BATCH | LINK)
    assert same_bits(out[:, c.kind == 0], z[:, c.kind == 0])
    assert np.isin(out[:, c.kind == 1], (0.0, 1.0)).all()


@pytest.mark.parametrize("name", ["A", "B"])
def test_simulate_missing_mask(ctx, cases, name):
    c = cases[name]
    load(ctx, c)
    out = ctx.simulate_data(seed=og.SEED, noise=NOISE, frac_missing=0.05)
    want = sr.missing_mask(c.draws, 0.05)
    assert 0.04 < want.mean() < 0.06
    assert np.array_equal(np.isnan(out), want)


@pytest.mark.parametrize("name", ["A", "B"])
def test_simulate_bernoulli(ctx, cases, name):
    c = cases[name]
    p = load(ctx, c)
    out = ctx.simulate_data(seed=og.SEED, noise=0.1, frac_missing=0.0)
    cols = np.flatnonzero(c.kind == 1)
    near, want = og.bernoulli_near(p, c.z, c.ref[BATCH][1], c.draws["u4"][:, cols], cols)
    got = out[:, cols]
    assert np.isin(got, (0.0, 1.0)).all()
    wrong = (got == 1.0) != want
    print(f"{name}: {cols.size} columns: {near.sum()} near ties, {wrong.sum()} decided the other way")
    assert near.mean() <= 0.01
    assert not np.any(wrong & ~near)


@pytest.mark.parametrize("name", ["A", "B"])
def test_simulate_normal_draw(ctx, cases, name):
    """The bound of test_gpu_simulate.test_normal_draw_on_a_model, noise 1e-5 + 2^-23 |out| per entry, on every normal draw of
    the case: at A (256 CUs) 8.7 M draws with u1 down to 2 2^-24 and |n| up to 5.34, where the f32 numpy twin is within
    1.7e-6 of the fp64 normal.  Measured on the MI355X: the device's normal is within 2.1e-6 (A) and 2.5e-6 (B) of the fp64
    one, 0.18 of the bound at the worst entry of either case."""
    c = cases[name]
    load(ctx, c)
    out = ctx.simulate_data(seed=og.SEED, noise=NOISE, frac_missing=0.0).astype(np.float64)
    z = ctx.impute(BATCH | LINK).astype(np.float64)
    nc = c.kind == 0
    n64 = c.draws["n"][:, nc]
    err = np.abs(out[:, nc] - (z[:, nc] + NOISE * n64))
    bound = NOISE * 1e-5 + 2.0 ** -23 * np.abs(out[:, nc])
    n_err = np.abs((out[:, nc] - z[:, nc]) / NOISE - n64).max()
    print(f"{name}: {n64.size} normal draws, max |n| = {np.abs(n64).max():.3f}: worst |error| / bound = {(err / bound).max():.3f}, "
          f"max |(out - z) / noise - n64| = {n_err:.3e}")
    assert np.all(err <= bound)


def test_simulate_row_range(ctx, cases):
    c = cases["A"]
    p = load(ctx, c)
    M = p["M"]
    kw = dict(seed=og.SEED, noise=NOISE, frac_missing=0.05)
    full = ctx.simulate_data(**kw).copy()
    assert np.isnan(full).any()
    assert same_bits(ctx.simulate_data(row_start1=129, row_stop1=M, row_offset=0, **kw), full[128:M])


# ---- 6. simulate_data_resident: the tile-major store from second units ---------------------------------------------------
@pytest.mark.parametrize("name,store", [("A", "f32"), ("B", "bf16")])
def test_resident_is_set_data_of_the_host_matrix(pkg, cases, name, store):
    """The pattern of test_gpu_simulate.test_resident_is_set_data_of_the_host_matrix: the NaN pads and the all-pad tile of the
    odd tile count are written by units past the first grid; a wrong tile shows in the loss, the statistics or the fit."""
    p = cases[name].p
    kw = dict(seed=og.SEED, noise=NOISE, frac_missing=0.05)
    res = []
    for resident in (True, False):
        c = pkg.Context(0)
        try:
            to_context(p, c)
            H = c.simulate_data(**kw).copy()
            if resident:
                c.set_data(p["D"], store=store)
                c.simulate_data_resident(**kw)
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


# ---- 7. the 64-bit counter and key on the device -------------------------------------------------------------------------
def test_counter_and_key_are_64_bit(pkg, ctx):
    p = sr.sim_case(*og.EDGE_SHAPE)
    K, M, N = og.EDGE_SHAPE
    to_context(p, ctx)
    kw = dict(noise=NOISE, frac_missing=0.3)
    out = ctx.simulate_data(seed=og.EDGE_SEED, row_offset=og.EDGE_ROW0, **kw).copy()
    d = sr.draws(og.EDGE_SEED, M, N, row_offset=og.EDGE_ROW0)
    # the missing mask is the twin's, bit for bit
    mask = sr.missing_mask(d, 0.3)
    assert 0.2 < mask.mean() < 0.4 and np.array_equal(np.isnan(out), mask)
    # Bernoulli decisions and the normal draws, on the entries that are there
    z = sr.link_space(p, BATCH)
    tol = sr.impute_tol(p, BATCH, z)
    kind = sr.kinds_of(p)
    cols = np.flatnonzero(kind == 1)
    near, want = og.bernoulli_near(p, z, tol, d["u4"][:, cols], cols)
    got, there = out[:, cols], ~mask[:, cols]
    assert there.sum() > 200 and np.isin(got[there], (0.0, 1.0)).all()
    wrong = ((got == 1.0) != want) & there
    assert near.mean() <= 0.01 and not np.any(wrong & ~near)
    zd = ctx.impute(BATCH | LINK).astype(np.float64)
    nc = np.flatnonzero(kind == 0)
    o = out[:, nc].astype(np.float64)
    ok = ~mask[:, nc]
    err = np.abs(o - (zd[:, nc] + NOISE * d["n"][:, nc]))[ok]
    assert np.all(err <= (NOISE * 1e-5 + 2.0 ** -23 * np.abs(o))[ok])
    # not the draw of the seed's low word, and not that of rows reduced mod 2^32 (below)
    assert not same_bits(out, ctx.simulate_data(seed=og.EDGE_SEED & 0xFFFFFFFF, row_offset=og.EDGE_ROW0, **kw))
    assert not same_bits(out, ctx.simulate_data(seed=og.EDGE_SEED >> 32, row_offset=og.EDGE_ROW0, **kw))
    # rows 35..70 held as a shard at row_offset = 2^32 are rows 35..70 of the draw; at row_offset = 0, the rows a counter
    # truncated to 32 bits would give them, they are not (in any row)
    c = pkg.Context(0)
    try:
        to_context(shard_problem(p, 35, 70), c)
        assert same_bits(c.simulate_data(seed=og.EDGE_SEED, row_offset=2 ** 32, **kw), out[35:70])
        low = c.simulate_data(seed=og.EDGE_SEED, row_offset=0, **kw)
        assert (np.isnan(low) != np.isnan(out[35:70])).any(axis=1).all()
    finally:
        c.close()
