"""Host-side conditions of tests/test_gpu_threshold_edges.py: on every problem of tests/threshold_edge_problems.py that the
device tests compare, every finite threshold's group gradient is more than 100 tolerances (LAYER_TAU times its scale), and
every fault the new geometry could hide -- a running sum not carried along the row sweep, the list's entry used for the tile,
a column outside every view given view 0's batch effects, a group's columns past the first 256 left out, a wide batch index
cut to 4 bits -- moves some finite gradient by more than 10 tolerances; the cascade problem's raw step has both upper
thresholds below the lowest.  No GPU."""
import numpy as np
import pytest

import batch_cases as bc
import hinge_ref as hr
import threshold_edge_problems as ep
import threshold_ref as tr
from problems import LAYER_TAU
from test_threshold_cases import big

LONG = {"A-k48": lambda: big("A", 48), "B-k128": lambda: big("B", 128), "Cwide-k48-m600": lambda: ep.layout_c(48, 600, "wide"),
        "Cwide-k128-m600": lambda: ep.layout_c(128, 600, "wide"), "Cnarrow-k80-m512": lambda: ep.layout_c(80, 512, "narrow")}
SKIPPED = {f"C{v or 'plain'}-k{K}": (lambda K=K, v=v: ep.layout_c(K, 70, v)) for K in hr.KS for v in (None, "narrow")}
WIDE = {"Cwide-k20": lambda: ep.layout_c(20, 70, "wide"), "Cwide-k80": lambda: ep.layout_c(80, 70, "wide"),
        "nb255-k128": ep.many_batches_255}
OTHER = {"cascade": ep.cascade_problem, "D": ep.layout_d, "E": ep.layout_e}
ALL = {**LONG, **SKIPPED, **WIDE, **OTHER}
assert len(ALL) == len(LONG) + len(SKIPPED) + len(WIDE) + len(OTHER)


def tolerances(p):
    return tr.group_grad(p), LAYER_TAU * tr.group_scale(p), np.isfinite(tr.group_thresholds(p))


def shows(p, bad_group, tag, by=10):
    """The mutant's group gradients differ from the reference's by more than `by` tolerances on some finite threshold."""
    G, tol, fin = tolerances(p)
    r = float(np.max(np.abs(bad_group - G)[fin] / tol[fin]))
    print(f"THRESH mutant {tag} ratio={r:.0f}")
    assert r > by, (tag, r)
    return r


def test_the_layouts_are_what_the_device_tests_assume():
    p = ep.layout_c(20, 70, "narrow")
    assert p["N"] == 200 and ep.tiles_of(p) == ep.C_TILES == [1, 3, 4, 6]
    k3 = hr.kinds_of(p) == 3
    assert k3[128:160].sum() == 2 and k3[192:200].all()                       # tile 4 holds two; the ragged tile is all kind 3
    covered = np.zeros(200, bool)
    for v, (s, e) in zip(p["batch_views"], ep.C_VIEWS):
        assert (v["start1"], v["stop1"]) == (s, e) and (np.asarray(v["batch_of_row"]) < 0).sum() == 5
        covered[s - 1:e] = True
    out = np.flatnonzero(k3 & ~covered) + 1
    assert out.tolist() == [j for s, e in ep.C_UNVIEWED for j in range(s, e + 1)]
    for variant, nbs in ep.C_BATCHES.items():
        for v, nb in zip(ep.layout_c(20, 70, variant)["batch_views"], nbs):
            b = np.asarray(v["batch_of_row"])
            assert v["logdelta"].shape[0] == nb and set(b[b >= 0].tolist()) == set(range(nb))
    assert bc.dense_slots(20) == 32 and bc.dense_slots(6) == 16 and bc.dense_slots(255) == 256 and bc.dense_slots(256) == 0
    tg = tr.group_thresholds(p)
    assert np.isfinite(tg[0]).all() and np.allclose(tg[0], np.add(ep.FULL, ep.SHIFT))
    d, e = ep.layout_d(), ep.layout_e()
    assert [b - a + 1 for a, b in tr.groups_of(d)] == [520, 257] and -(-520 // 256) == 3 and -(-257 // 256) == 2
    assert len(tr.groups_of(e)) == 70 > 64 and e["N"] == 350
    kinds = {tuple(np.isfinite(t)) for t in tr.group_thresholds(e)}
    assert kinds == {(True, True, True), (False, True, True), (True, False, False)}
    b = np.asarray(ep.many_batches_255()["batch_views"][0]["batch_of_row"])
    assert b.max() == 254 and set(b[b >= 0].tolist()) == set(range(255)) and (b < 0).sum() == 5


@pytest.mark.parametrize("name", list(ALL))
def test_every_finite_threshold_is_exercised(name):
    """|G| > 100 tolerances for every finite threshold of every problem the device tests use."""
    G, tol, fin = tolerances(ALL[name]())
    print(f"THRESH ratio {name} min={np.min(np.abs(G[fin]) / tol[fin]):.0f}")
    assert fin.any() and (np.abs(G[fin]) > 100 * tol[fin]).all(), (G, tol)


@pytest.mark.parametrize("R", [1, 2])
@pytest.mark.parametrize("name", list(LONG))
def test_a_sweep_that_drops_its_later_panels_shows(name, R):
    p = LONG[name]()
    assert ep.panels(p["M"], p["K"]) > R                                      # some unit sweeps more than one panel
    shows(p, tr.group_grad(ep.later_panels_dropped(p, R)), f"later_panels_dropped {name} R={R}")


def test_no_ragged_panel_at_512_rows():
    assert 512 % (32 * 8) == 0 and 512 % (32 * 4) == 0 and ep.layout_c(80, 512, "narrow")["M"] == 512


@pytest.mark.parametrize("name", list(SKIPPED) + ["Cwide-k48-m600", "Cnarrow-k80-m512", "Cwide-k20"])
def test_a_tile_read_by_its_list_index_shows(name):
    p = ALL[name]()
    assert ep.tiles_of(p) != list(range(len(ep.tiles_of(p))))
    q = ep.tile_identity(p)
    shows(p, tr.group_grad(q), f"tile_identity {name}")
    gc, tc = tr.col_grad(p), LAYER_TAU * tr.col_scale(p)
    k3 = ~np.isnan(gc[:, 0])
    assert (np.abs(tr.col_grad(q) - gc)[k3] > 10 * tc[k3]).any()


@pytest.mark.parametrize("name", [n for n in ALL if n.startswith(("Cnarrow", "Cwide", "nb255", "cascade"))])
def test_an_unviewed_column_given_view_0_shows(name):
    p = ALL[name]()
    shows(p, tr.group_grad(ep.unviewed_as_view0(p)), f"unviewed_as_view0 {name}")


@pytest.mark.parametrize("name", ["Cwide-k20", "Cwide-k80", "Cwide-k48-m600", "Cwide-k128-m600", "nb255-k128"])
def test_a_batch_index_cut_to_four_bits_shows(name):
    p = ALL[name]()
    assert max(v["logdelta"].shape[0] for v in p["batch_views"]) > 15
    shows(p, tr.group_grad(ep.wide_as_16(p)), f"wide_as_16 {name}")


def test_a_group_sum_that_drops_its_tail_shows():
    p = ep.layout_d()
    G, tol, fin = tolerances(p)
    bad = ep.group_tail_dropped(p)
    with np.errstate(invalid="ignore"):                                      # (an infinite threshold: 0 / 0, masked by fin)
        r = np.abs(bad - G) / tol
    print("THRESH mutant group_tail_dropped", np.round(r[fin], 0))
    assert (r[0][fin[0]] > 10).all() and (r[1][fin[1]] > 10).all()           # both groups: 264 columns lost, and one
    # the per-column gradients of D answer for the entry faults as those of A and B do (test_threshold_cases)
    gc, tc = tr.col_grad(p), LAYER_TAU * tr.col_scale(p)
    k3 = ~np.isnan(gc[:, 0])
    assert k3.sum() == 777
    for fault in ("off_by_one", "swap_ab", "drop_ragged", "neighbour"):
        assert (np.abs(tr.group_grad(p, fault) - G)[fin] > 10 * tol[fin]).any(), fault
        assert (np.abs(tr.col_grad(p, fault) - gc)[k3] > 10 * tc[k3]).any(), fault
    # and the last column of each group, the one a partial last thread adds, is itself far above its tolerance
    for s, e in tr.groups_of(p):
        m = np.isfinite(hr.thresholds_of(p)[e - 1])
        assert (np.abs(gc[e - 1][m]) > 10 * tc[e - 1][m]).all()


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_the_cascade_problem_lands_both_upper_thresholds_below_the_lowest(opt):
    p, kw = ep.cascade_problem(), ep.CASCADE_OPT[opt]
    assert np.isfinite(tr.group_thresholds(p)[0]).all()
    _, _, info = tr.joint_epoch(p, tr.fresh_state(p, kw), kw, 1, train_xy=False)
    raw = info["raw"][0]
    assert raw[1] < raw[0] and raw[2] < raw[0], raw
    assert raw[2] > raw[1]                                                   # t2 moves only because t1 was moved first
    assert tr.clamp(raw).tolist() == [raw[0]] * 3
    # the other groups do not cross: what the clamp does there is nothing
    assert np.array_equal(tr.clamp(info["raw"][1:]), info["raw"][1:])
