"""pmf_factor_importance where tests/test_gpu_importance.py does not take it: a unit that sweeps so many row panels that its
float32 chain is flushed to float64 several times, more units than the grid has workgroups (by the problem's own size, and by
the PMF_IMPORTANCE_GRID / PMF_IMPORTANCE_RANGES hooks on small ones), column tiles walked in several launches (the slab cap's
path, through PMF_IMPORTANCE_TILES), and the buffers returned on close.  pmf_debug_factor_importance tells each test that it
reached the edge it aims at.  References and bounds: tests/importance_ref.py."""
import copy

import numpy as np
import pytest

import hinge_ref as hr
import importance_ref as ir

pytestmark = pytest.mark.gpu
NAMES = ("delta", "full", "null", "n_obs")


def tiled(name, reps):
    """The table's problem `name` with its rows repeated `reps` times (X and the row -> batch maps with them)."""
    p = ir.cases()[name]
    q = copy.copy(p)
    q.update(M=p["M"] * reps, D=np.asfortranarray(np.tile(p["D"], (reps, 1))), X=np.asfortranarray(np.tile(p["X"], (1, reps))),
             batch_views=[dict(v, batch_of_row=np.tile(v["batch_of_row"], reps)) for v in p["batch_views"]])
    return q


def long_sweep():
    """20000 x 33, K = 2: 79 panels of 256 rows, two column tiles (one of a single column)."""
    p = ir.cases()["mix-45x37-k2"]
    q = tiled("mix-45x37-k2", 445)
    q.update(M=20000, N=33, D=np.asfortranarray(q["D"][:20000, :33]), X=np.asfortranarray(q["X"][:, :20000]),
             Y=np.asfortranarray(p["Y"][:, :33]), logsigma=p["logsigma"][:33], mu=p["mu"][:33], col_weight=p["col_weight"][:33],
             noise_ranges=[(s, min(e, 33)) for s, e in p["noise_ranges"] if s <= 33],
             noise_kinds=[k for (s, e), k in zip(p["noise_ranges"], p["noise_kinds"]) if s <= 33])
    return q


_CACHE = {}


def problem(key, make):
    """One problem and one reference per key, shared by the tests that need them."""
    if key not in _CACHE:
        p = make()
        r = ir.reference(p)
        _CACHE[key] = (p, (r, ir.bounds(r)))
    return _CACHE[key]


def run(ctx, p):
    hr.to_context(p, ctx)
    return dict(zip(NAMES, ctx.factor_importance()))


def test_a_long_sweep_flushes_its_chain(ctx, monkeypatch):
    p, ref = problem("long", long_sweep)
    assert not p["batch_views"] and p["M"] == 20000 and p["N"] == 33
    monkeypatch.setenv("PMF_IMPORTANCE_RANGES", "1")
    one = run(ctx, p)
    d = ctx.debug_factor_importance()
    assert (d["kb"], d["nw"], d["ranges"], d["n_units"]) == (1, 8, 1, 2), d
    # 79 panels, a flush every 16: the geometry the host handed over (the kernel does not report its flushes back; what this
    # run holds of them is that four mid-unit flushes and the last one neither lose, keep nor double anything)
    assert d["flushes"] == 5 >= 2, d
    ir.check(one, p, ref=ref)
    monkeypatch.delenv("PMF_IMPORTANCE_RANGES")
    free = run(ctx, p)                                        # the host's own row ranges: one panel per unit
    d = ctx.debug_factor_importance()
    assert d["ranges"] == 79 and d["flushes"] == 1, d
    ir.check(free, p, ref=ref)
    assert np.array_equal(free["n_obs"], one["n_obs"])


def test_more_units_than_workgroups(ctx):
    """7680 x 288, K = 2: nine column tiles x 30 row ranges = 270 units on a grid of at most one workgroup per CU."""
    p, ref = problem("wide", lambda: tiled_wide())
    got = run(ctx, p)
    d = ctx.debug_factor_importance()
    assert d["n_units"] == 9 * d["ranges"] and d["n_units"] > d["grid"] >= 1 and d["launches"] == 1, d
    ir.check(got, p, ref=ref)


def tiled_wide():
    base = ir.firm(ir.mix_problem(64, 288, 2, seed=21, batch=True), 21)
    q = copy.copy(base)
    reps = 120
    q.update(M=64 * reps, D=np.asfortranarray(np.tile(base["D"], (reps, 1))), X=np.asfortranarray(np.tile(base["X"], (1, reps))),
             batch_views=[dict(v, batch_of_row=np.tile(v["batch_of_row"], reps)) for v in base["batch_views"]])
    return q


@pytest.mark.parametrize("name,reps", [("hinge-A-k20-batch", 9), ("hinge-A-k128-batch", 5)])
def test_one_workgroup_walks_every_unit(ctx, monkeypatch, name, reps):
    """630 rows at eight waves (3 panels), 350 at four (3 panels): two row ranges, six tiles, a grid of one and of five."""
    p, ref = problem((name, reps), lambda: tiled(name, reps))
    outs = []
    for grid in (1, 5, None):
        monkeypatch.setenv("PMF_IMPORTANCE_RANGES", "2")
        if grid:
            monkeypatch.setenv("PMF_IMPORTANCE_GRID", str(grid))
        else:
            monkeypatch.delenv("PMF_IMPORTANCE_GRID")
        got = run(ctx, p)
        d = ctx.debug_factor_importance()
        assert d["ranges"] == 2 and d["n_units"] == 12 and d["grid"] == (grid or 12), d
        ir.check(got, p, ref=ref)
        outs.append(got)
    for k in NAMES:                                           # a unit's sums do not depend on the workgroup that ran it
        assert np.array_equal(outs[0][k], outs[1][k]) and np.array_equal(outs[0][k], outs[2][k]), k


def test_column_tiles_in_several_launches(ctx, monkeypatch):
    p, ref = problem(("hinge-A-k48-plain", 1), lambda: ir.cases()["hinge-A-k48-plain"])
    whole = run(ctx, p)
    assert ctx.debug_factor_importance()["launches"] == 1
    monkeypatch.setenv("PMF_IMPORTANCE_TILES", "4")
    got = run(ctx, p)
    d = ctx.debug_factor_importance()
    assert d["launches"] == 2 and d["n_units"] == 6 * d["ranges"], d       # six tiles: four, then two
    ir.check(got, p, ref=ref)
    for k in NAMES:
        assert np.array_equal(got[k], whole[k]), k


def test_live_bytes_return(pkg):
    before = pkg._lib.live_bytes()
    c = pkg.Context(0)
    try:
        for name in ("mix-45x37-k2", "hinge-A-k128-batch"):
            p = ir.cases()[name]
            ir.check(run(c, p), p)
        assert pkg._lib.live_bytes() != before
    finally:
        c.close()
    assert pkg._lib.live_bytes() == before
