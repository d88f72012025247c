"""Hold-out entries on the device (include/pmf_hip_holdout.h): masking and restoring the resident data in both storage types,
the tile-flag trap, pmf_holdout_loss against tests/holdout_ref.py at the edges of its geometry, refusals and lifecycle.
Tracking and early stopping: tests/test_gpu_holdout_fit.py."""
import numpy as np
import pytest

import hinge_ref as hr
import holdout_ref as ho
from problems import make_problem

pytestmark = pytest.mark.gpu


@pytest.fixture()
def fresh(pkg):
    """Contexts of this test's own, closed at its end (the session's context keeps no set and no switch of these tests)."""
    made = []

    def make(p=None, store="f32"):
        c = pkg.Context(0)
        made.append(c)
        if p is not None:
            hr.to_context(p, c)
            if store != "f32":
                c.set_data(p["D"], store=store)
        return c

    yield make
    for c in made:
        c.close()


def bf16_round(v):
    """Round to nearest even to bfloat16, as float32 (finite values)."""
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


# ---- 1. mask and restore ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("nan_frac", [0.0, 0.05])
def test_the_set_is_a_host_mask_and_restore_undoes_it(fresh, store, nan_frac):
    p = ho.problem(33, nan_frac)
    rows, cols = ho.held_sets(p)["wide"]
    r, c, v, _ = ho.held_after_set(np.asarray(p["D"]), rows, cols)
    a = fresh(p, store)
    before = a.loss()
    assert a.set_holdout(rows + 1, cols + 1) == r.size
    gr, gc, gv = a.get_holdout()
    assert np.array_equal(gr, r + 1) and np.array_equal(gc, c + 1)                 # sorted by (column, row), the missing dropped
    assert np.array_equal(gv, bf16_round(v) if store == "bf16" else v)             # the STORED value
    b = fresh(ho.masked(p, rows, cols), store)
    held, masked = a.loss(), b.loss()
    assert held == masked and held["data"] != before["data"]                       # bitwise: dicts of floats
    sa, sb = a.stats(True), b.stats(True)
    assert all(np.array_equal(sa[k], sb[k]) for k in ("n", "sum", "sumsq", "sqerr"))   # the statistics see them as missing
    a.clear_holdout(restore=True)
    assert a.loss() == before and a.get_holdout()[0].size == 0
    assert a.set_holdout(rows + 1, cols + 1) == r.size                             # ... and the set can be taken again
    a.clear_holdout(restore=False)
    assert a.loss() == masked                                                      # dropped without write-back


def plain_problem():
    """1024 x 12288, K = 40, all-normal, no batch views, fully observed: four row panels x 384 column tiles in segments of
    eight, twelve tiles per workgroup of a grid of 128.  A workgroup that goes on into the next row panel of its segment
    meets column tiles it has visited: those the exact pass runs in its plain tile loop."""
    return make_problem(M=1024, N=12288, K=40, seed=77, random_init=True)


def test_a_set_on_fully_observed_data_invalidates_the_tile_flags(fresh, monkeypatch):
    """The trap: the all-finite flags and the plain-run table of a fully observed D are cached by the first pass.  A set, and
    a restore, must invalidate them, or the plain loop trains through NaN."""
    monkeypatch.setenv("PMF_RESERVE_CUS", "128")
    monkeypatch.setenv("PMF_TPS_SCALE", "0.001")
    p = plain_problem()
    rng = np.random.default_rng(5)
    at = rng.choice(p["M"] * p["N"], 60, replace=False)                            # sixty entries all over the matrix
    rows, cols = at % p["M"], at // p["M"]
    opts = dict(update_X=True, update_Y=True, max_epochs=3, abs_tol=0, rel_tol=0)

    def start(c):
        c.set_factors(p["X"], p["Y"])
        c.set_optimizer("adagrad", lr=0.05)

    a = fresh(p)
    start(a)
    full = a.fit(**opts)
    plain = a.last_path()["plain_tiles"]
    assert plain > 0                                                               # the plain loop ran: the flags are cached
    fx, fy = a.get_factors()
    start(a)
    assert a.set_holdout(rows + 1, cols + 1) == 60
    held = a.fit(**opts)
    assert a.last_path()["plain_tiles"] < plain                                    # ... now without the tile of the set
    b = fresh(ho.masked(p, rows, cols))
    start(b)
    ref = b.fit(**opts)
    assert np.isfinite(held["loss"]).all() and np.array_equal(held["loss"], ref["loss"])
    assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
    # set -> fit -> clear(restore) -> fit equals a fresh context's fit on the full data
    a.clear_holdout(restore=True)
    start(a)
    again = a.fit(**opts)
    assert a.last_path()["plain_tiles"] == plain
    assert np.array_equal(again["loss"], full["loss"])
    assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), (fx, fy)))


# ---- 2. the loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ho.KS)
def test_the_loss_is_within_its_bound_whatever_the_geometry(fresh, monkeypatch, K):
    p = ho.problem(K)
    rows, cols = ho.held_sets(p)["wide"]                                           # unsorted, with entries that are missing
    a = fresh(p)
    n = a.set_holdout(rows + 1, cols + 1)
    total, lc, nc = a.holdout_loss()
    d = a.debug_holdout_pass()
    assert nc.sum() == n and nc[7] == 0 and lc[7] == 0.0                           # a column with none held
    assert d["n_units"] == int((nc > 0).sum()) and d["passes"] == 1                # one unit per column at the default size
    worst = ho.check(lc, nc, total, p, rows, cols)
    print(f"K = {K}: worst error / bound = {worst:.3f}")
    assert total == float(np.cumsum(lc)[-1])                                       # ascending columns, one after the other
    again = a.holdout_loss()
    assert again[0] == total and np.array_equal(again[1], lc)                      # from call to call
    monkeypatch.setenv("PMF_HOLDOUT_GRID", "1")
    one = a.holdout_loss()
    assert a.debug_holdout_pass()["grid"] == 1 and d["grid"] > 1
    assert one[0] == total and np.array_equal(one[1], lc)                          # whatever the grid
    monkeypatch.setenv("PMF_HOLDOUT_UNIT", "16")
    cut = a.holdout_loss()
    d2 = a.debug_holdout_pass()
    assert d2["n_units"] == int(((nc + 15) // 16).sum()) > d["n_units"] and nc[40] > 32    # column 41 crosses two seams
    assert cut[0] == total and np.array_equal(cut[1], lc)                          # ... and whatever the units
    monkeypatch.delenv("PMF_HOLDOUT_GRID")
    assert np.array_equal(a.holdout_loss()[1], lc)
    a.set_precision("bf16x3")
    assert np.array_equal(a.holdout_loss()[1], lc)                                 # always exact f32


@pytest.mark.parametrize("K", [4, 128])
def test_the_loss_at_the_corners_and_beside_the_padding(fresh, K):
    p = ho.problem(K)
    rows, cols = ho.held_sets(p)["corners"]
    a = fresh(p, "bf16" if K == 4 else "f32")
    n = a.set_holdout(rows + 1, cols + 1)
    q = dict(p)
    if K == 4:
        D = np.array(p["D"])
        D[np.isfinite(D)] = bf16_round(D[np.isfinite(D)])
        q["D"] = np.asfortranarray(D)                                              # the held values are the stored ones
    total, lc, nc = a.holdout_loss()
    assert n == nc.sum() > 0
    ho.check(lc, nc, total, q, rows, cols)


def test_the_loss_follows_the_parameters_and_changes_nothing(fresh):
    p = ho.problem(33)
    rows, cols = ho.held_sets(p)["wide"]
    a = fresh(p)
    a.set_holdout(rows + 1, cols + 1)
    before = a.loss()
    X, Y = a.get_factors()
    t0, lc0, _ = a.holdout_loss()
    assert a.loss() == before and all(np.array_equal(u, w) for u, w in zip(a.get_factors(), (X, Y)))
    q = dict(p, X=np.asfortranarray(0.5 * np.asarray(p["X"])), mu=(np.asarray(p["mu"]) + 0.25).astype(np.float32))
    a.set_factors(q["X"], q["Y"])
    a.set_col_params(q["logsigma"], q["mu"])
    t1, lc1, nc1 = a.holdout_loss()
    assert t1 != t0
    ho.check(lc1, nc1, t1, q, rows, cols)


# ---- 5. refusals and lifecycle --------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable_and_the_data_intact(pkg, fresh):
    p = ho.problem(4)
    rows, cols = ho.held_sets(p)["wide"]
    e = fresh()
    with pytest.raises(pkg.PMFError, match="data not set"):
        e.set_holdout([1], [1])
    a = fresh(p)
    before = a.loss()
    assert a.set_holdout([], []) == 0 and a.get_holdout()[0].size == 0             # n = 0: legal, no set
    for r1, c1, word in (([1, p["M"] + 1], [1, 1], r"entry 1 = \(71, 1\) is outside"), ([0], [1], "outside"), ([1], [p["N"] + 1], "outside"),
                         ([5, 9, 5, 9], [2, 2, 2, 2], r"entry 2 = \(5, 2\) is a duplicate")):
        with pytest.raises(pkg.PMFError, match=word):
            a.set_holdout(r1, c1)
        assert a.loss() == before and a.get_holdout()[0].size == 0
    nan_r, nan_c = np.nonzero(np.isnan(np.asarray(p["D"])))
    assert a.set_holdout(nan_r[:7] + 1, nan_c[:7] + 1) == 0 and a.loss() == before     # all missing already: no set
    assert a.holdout_loss()[0] == 0.0
    n = a.set_holdout(rows + 1, cols + 1)
    held = a.loss()
    with pytest.raises(pkg.PMFError, match="already present"):
        a.set_holdout([1], [1])
    assert a.loss() == held and a.get_holdout()[0].size == n
    a.set_data(p["D"])                                                             # new data: the set goes, nothing is written
    assert a.get_holdout()[0].size == 0 and a.loss() == before and a.holdout_loss()[0] == 0.0
    a.clear_holdout(restore=True)                                                  # no set: nothing happens
    assert a.loss() == before


def test_tracking_refusals_come_before_anything_is_launched(pkg, fresh):
    p = ho.problem(4)
    rows, cols = ho.held_sets(p)["wide"]
    a = fresh(p)
    a.set_optimizer("adagrad", lr=0.05)
    a.set_holdout(rows + 1, cols + 1)
    before, X0 = a.loss(), a.get_factors()
    a.set_holdout_tracking(every=1, patience=2, restore_best=True)
    with pytest.raises(pkg.PMFError, match="update_col_layers"):
        a.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=2)
    with pytest.raises(pkg.PMFError, match="threshold training"):
        a.fit(update_X=True, update_Y=True, update_noise_models=True, max_epochs=2)
    with pytest.raises(pkg.PMFError, match="must not be negative"):
        a.set_holdout_tracking(every=-1)
    assert a.loss() == before and all(np.array_equal(u, w) for u, w in zip(a.get_factors(), X0))
    assert a.get_holdout_trace()["epochs"].size == 0
    a.set_holdout_tracking(every=1, patience=0, restore_best=False)               # tracking alone goes with both
    h = a.fit(update_X=True, update_Y=True, update_col_layers=True, update_noise_models=True, max_epochs=2, abs_tol=0, rel_tol=0)
    assert h["holdout_epochs"].tolist() == [1, 2]
    a.comm_init_host(0, 2, lambda arr: None)                                      # (never called: the fit is refused first)
    with pytest.raises(pkg.PMFError, match="not supported with 2 ranks"):
        a.fit(update_X=True, update_Y=True, max_epochs=2)
    a.comm_destroy()
    b = fresh(p)                                                                  # a rank whose rows hold no entry refuses alike
    b.set_holdout_tracking(every=1)
    b.comm_init_host(0, 2, lambda arr: None)
    with pytest.raises(pkg.PMFError, match="not supported with 2 ranks"):
        b.fit(update_X=True, update_Y=True, max_epochs=2)
    b.comm_destroy()
    a.set_holdout_tracking(0)
    assert "holdout_loss" not in a.fit(update_X=True, update_Y=True, max_epochs=2)
