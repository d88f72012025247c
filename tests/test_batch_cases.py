"""The batch-edge problems of tests/test_gpu_batch_edges.py are what they claim to be (no GPU).

* the restated selection rules give the families of the table in csrc/pmf_pass.hip (fused_geometry) on spot values;
* every builder has the per-panel batch counts its case is about, ascending disjoint views and batch ids below nb;
* sensitivity: on every problem the GPU file runs, one batched row moved to another batch of its panel, one unbatched row
  given batch 0, or one view boundary moved by a column changes the fp64 oracle's gX or gY by at least 10 GRAD_TOL in
  rel_err -- the GPU comparison at GRAD_TOL would see a kernel that made any of these mistakes on a single row or column.
"""
import numpy as np
import pytest

import batch_cases as bc
from problems import rel_err, to_oracle
from test_gpu_parity import GRAD_TOL


def counts(n128, n256=None, n512=None):
    n256 = n128 if n256 is None else n256
    n512 = n256 if n512 is None else n512
    return {128: n128, 256: n256, 512: n512}.__getitem__


def test_restated_rules_on_spot_values():
    e = bc.expected_batch_path
    # every family where everything fits; slots follow nb_max
    assert e(20, "f32", True, 2, counts(6), 6) == (0, 256, 1, 16)
    assert e(48, "f32", True, 2, counts(6), 15) == (0, 256, 1, 16)
    assert e(80, "f32", True, 2, counts(6), 16) == (0, 128, 1, 32)
    assert e(128, "f32", False, 2, counts(6), 31) == (0, 128, 1, 32)
    assert e(32, "bf16x3", True, 16, counts(15), 32) == (1, 256, 1, 64)
    assert e(33, "bf16x3", True, 5, counts(15), 200) == (8, 512, 1, 256)
    assert e(64, "bf16x3", False, 5, counts(15), 255) == (2, 256, 1, 256)
    assert e(65, "bf16x3", True, 16, counts(15), 6) == (4, 128, 1, 16)
    assert e(128, "bf16x3", True, 16, counts(15), 6) == (8, 256, 1, 16)
    assert e(97, "bf16x3", False, 16, counts(15), 6) == (4, 128, 1, 16)
    # the 512-row sb8 has room for 5 views
    assert e(48, "bf16x3", True, 6, counts(3), 6) == (2, 256, 1, 16)
    # a panel over the limit: the next family of the chain whose panel fits, else the exact kernel's gathers
    assert e(48, "bf16x3", True, 1, counts(8, 8, 16), 16) == (2, 256, 1, 32)
    assert e(48, "bf16x3", True, 1, counts(8, 16, 16), 16) == (0, 256, 2, 32)
    assert e(128, "bf16x3", True, 1, counts(8, 16, 16), 16) == (4, 128, 1, 32)
    assert e(128, "bf16x3", True, 1, counts(16), 16) == (0, 128, 2, 32)
    assert e(20, "bf16x3", True, 1, counts(15, 16), 20) == (0, 256, 2, 32)
    assert e(80, "bf16x3", True, 1, counts(16), 20) == (0, 128, 2, 32)
    assert e(80, "f32", True, 1, counts(15, 16), 20) == (0, 128, 1, 32)
    assert e(48, "f32", True, 1, counts(15, 16), 20) == (0, 256, 2, 32)
    # 256 batches: no dense table, whatever the panels meet
    assert e(20, "bf16x3", True, 1, counts(14), 256) == (0, 256, 2, 0)
    assert e(20, "f32", True, 1, counts(14), 255) == (0, 256, 1, 256)
    assert [bc.dense_slots(n) for n in (1, 15, 16, 31, 32, 127, 128, 255, 256)] == [16, 16, 32, 32, 64, 128, 256, 256, 0]


def test_paths_are_the_families_without_batch_trouble():
    for (prec, K, gname), (fam, BM) in bc.PATHS.items():
        assert bc.expected_batch_path(K, prec, gname == "both", 1, counts(1), 1) == (fam, BM, 1, 16)


def panel_profile(p, BM, v=0):
    """Distinct non-negative batches of view v per panel of BM rows."""
    bor = np.asarray(p["batch_views"][v]["batch_of_row"])
    return [len(np.unique(b[b >= 0])) for b in (bor[i:i + BM] for i in range(0, len(bor), BM))]


def check_wellformed(p):
    M, N = p["D"].shape
    kind = np.empty(N, dtype=object)
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        kind[s - 1:e] = kd
    in_view = np.zeros(N, bool)
    last = 0
    for bv in p["batch_views"]:
        s, e = bv["start1"], bv["stop1"]
        assert last < s <= e <= N, "views ascending and disjoint"
        last = e
        in_view[s - 1:e] = True
        nb = bv["logdelta"].shape[0]
        assert bv["logdelta"].shape == bv["theta"].shape == (nb, e - s + 1)
        bor = bv["batch_of_row"]
        assert bor.shape == (M,) and bor.dtype == np.int32 and bor.min() >= -1 and bor.max() < nb
        centres = bv["theta"].mean(axis=1)
        assert nb == 1 or np.min(np.diff(np.sort(centres))) > 0, "distinct batch centres"
    assert (in_view & (kind == "bernoulli")).any() and (kind == "normal").any()
    if "poisson" in p["noise_kinds"]:
        assert (in_view & (kind == "poisson")).any()
    assert np.isnan(p["D"]).any()


@pytest.mark.parametrize("BM,K", sorted({(BM, path[1]) for path, (fam, BM) in bc.PATHS.items()}))
def test_builders_have_the_panel_counts_they_claim(BM, K):
    for n in (15, 16):
        p = bc.slots_edge(BM, K, n)
        assert p["M"] == BM + n and panel_profile(p, BM) == [3, n]
        assert panel_profile(p, 32)[-1] == n                    # ... all in one 32-row block
        q = bc.slots_edge(BM, K, n, mirror=True)
        assert q["M"] == BM + n and panel_profile(q, BM) == [n, 3] and panel_profile(q, 32)[0] == n
        bq = q["batch_views"][0]["batch_of_row"]
        assert bq[n - 1] == n - 1 and bq[n] == -1               # slot n - 1 right above a row with the identity slot
        for r in (p, q):
            assert len(r["batch_views"]) == 1 and (r["batch_views"][0]["start1"], r["batch_views"][0]["stop1"]) == (1, r["N"])
            check_wellformed(r)
    p = bc.unbatched(BM, K)
    b0, b1 = (bv["batch_of_row"] for bv in p["batch_views"])
    assert p["M"] == 2 * BM + 33 and (b0[BM:2 * BM] == -1).all() and (b0[[0, BM - 1, BM, p["M"] - 1]] == -1).all()
    assert panel_profile(p, BM) == [4, 0, 2] and (b1 == -1).all() and p["batch_views"][1]["logdelta"].shape[0] == 1
    assert p["batch_views"][0]["logdelta"].shape[0] == 7 and sorted(set(b0[b0 >= 0])) == [0, 1, 2, 3, 5, 6]
    check_wellformed(p)
    for N in (75, 161):
        p = bc.view_seams(BM, K, N)
        assert [(bv["start1"], bv["stop1"]) for bv in p["batch_views"]] == [(3, 10), (11, 11), (20, 40), (42, N)]
        assert p["M"] == BM + 33 and bc.panel_counts_of(p)(BM) == 15 and N % 32 != 0
        for v, is_sorted in enumerate((True, False, True, False)):
            bor = p["batch_views"][v]["batch_of_row"]
            assert (np.diff(bor) >= 0).all() == is_sorted
        check_wellformed(p)
    p = bc.many_views(BM, K)
    assert len(p["batch_views"]) == 16 and p["N"] == 70
    assert [bv["logdelta"].shape[0] for bv in p["batch_views"]] == [1, 6, 15] * 5 + [1]
    widths = [bv["stop1"] - bv["start1"] + 1 for bv in p["batch_views"]]
    gaps = [b["start1"] - a["stop1"] - 1 for a, b in zip(p["batch_views"], p["batch_views"][1:])]
    assert 2 <= min(widths) and max(widths) <= 6 and max(gaps) > 0 and bc.panel_counts_of(p)(BM) == 15
    check_wellformed(p)


def test_special_builders_have_the_panel_counts_they_claim():
    for BM, K in ((512, 48), (256, 128)):
        p = bc.halves_fit(BM, K)
        assert p["M"] == BM and panel_profile(p, BM) == [16] and panel_profile(p, BM // 2) == [8, 8]
        check_wellformed(p)
    for n in (5, 6):
        p = bc.many_views(512, 48, n)
        assert len(p["batch_views"]) == n and bc.panel_counts_of(p)(512) == 15
        check_wellformed(p)
    for K in (80, 128):
        p = bc.gather(K)
        assert (p["M"], p["N"]) == (161, 95) and panel_profile(p, 128)[0] == 20 and min(panel_profile(p, 128)) > 15
        check_wellformed(p)
    for nb, M in ((255, 5100), (256, 5120)):
        p = bc.many_batches(nb)
        assert (p["M"], p["N"], p["K"]) == (M, 33, 20) and bc.nb_max_of(p) == nb
        assert max(panel_profile(p, 256)) == 14 and max(panel_profile(p, 512)) > 15
        check_wellformed(p)
    for K, M in ((64, 2049), (128, 2049), (64, bc.WALK_M_SB8_512)):
        p = bc.walk(K, M)
        assert (p["M"], p["N"]) == (M, 2048) and p["batch_views"][0]["stop1"] % 32 != 0
        assert p["batch_views"][1]["start1"] == p["batch_views"][0]["stop1"] + 1
        for v in (0, 1):
            prof = panel_profile(p, 512, v)
            assert max(prof) <= 15 and bc.nb_max_of(p) == 40
            bor = p["batch_views"][v]["batch_of_row"]
            assert (np.diff(bor) >= 0).all() and len(set(bor)) == 40
            assert len({tuple(np.unique(bor[i:i + 256])) for i in range(0, M, 256)}) == (M + 255) // 256     # a slot map per panel
        check_wellformed(p)
    A, B, C = bc.cache_states()
    for a, b, c in zip(A["batch_views"], B["batch_views"], C["batch_views"]):
        assert not np.array_equal(a["batch_of_row"], b["batch_of_row"]) and np.array_equal(b["batch_of_row"], c["batch_of_row"])
        assert np.array_equal(a["theta"], b["theta"]) and not np.array_equal(b["theta"], c["theta"])
        assert a["theta"].shape == c["theta"].shape and (a["start1"], a["stop1"]) == (c["start1"], c["stop1"])
    for p in (A, B, C):
        assert bc.panel_counts_of(p)(512) <= 15
        check_wellformed(p)


def test_expected_paths_of_the_gpu_cases():
    """The fall-backs the cases are built for come out of the restated rules on the builders' own counts."""
    exp = {cid: bc.expected_of(fn(), path) for cid, fn, path, BM in bc.all_cases()}
    for path, (fam, BM) in bc.PATHS.items():
        pid = bc.path_id(path)
        KB = (path[1] + 31) // 32
        exact = (0, 256 if KB <= 2 else 128, 2, 32)
        assert exp[f"slots15-{pid}"] == exp[f"slots15_mirror-{pid}"] == (fam, BM, 1, 32)
        assert exp[f"slots16-{pid}"] == exp[f"slots16_mirror-{pid}"] == exact
        assert exp[f"unbatched-{pid}"] == exp[f"view_seams-{pid}"] == (fam, BM, 1, 16)
        assert exp[f"views16-{pid}"] == ((2, 256, 1, 16) if path == ("bf16x3", 48, "both") else (fam, BM, 1, 16))
    assert exp["halves_fit-bf16x3-k48-both"] == (2, 256, 1, 32) and exp["halves_fit-bf16x3-k128-both"] == (4, 128, 1, 32)
    assert exp["views5-bf16x3-k48-both"] == (8, 512, 1, 16) and exp["views6-bf16x3-k48-both"] == (2, 256, 1, 16)
    assert exp["gather-f32-k80-both"] == exp["gather-f32-k128-both"] == (0, 128, 2, 32)
    assert exp["nb255-f32-k20-both"] == (0, 256, 1, 256) and exp["nb255-bf16x3-k20-both"] == (1, 256, 1, 256)
    assert exp["nb256-f32-k20-both"] == exp["nb256-bf16x3-k20-both"] == (0, 256, 2, 0)


def _sensitivity_cases():
    seen, out = set(), []
    for cid, fn, path, BM in bc.all_cases():
        key = (fn.func, fn.args, BM)                 # one problem serves several paths
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(fn, BM, id=cid))
    return out


@pytest.mark.parametrize("fn,BM", _sensitivity_cases())
def test_one_wrong_row_or_column_moves_the_gradients(fn, BM):
    p = fn()
    go = bc.oracle_of(p)
    muts = bc.mutants(p, BM)
    assert "c" in muts and ("a" in muts or "b" in muts), sorted(muts)
    has_unbatched = any((bv["batch_of_row"] < 0).any() for bv in p["batch_views"])
    assert ("b" in muts) == has_unbatched
    for k, q in muts.items():
        _, gq = to_oracle(q).loss_and_grads(**bc.BOTH)
        moved = max(rel_err(gq["X"], go["X"]), rel_err(gq["Y"], go["Y"]))
        assert moved >= 10 * GRAD_TOL, (k, moved)
