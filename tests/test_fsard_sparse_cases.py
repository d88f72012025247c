"""CPU guard of the rows that tests/test_gpu_fsard_csr.py runs through pmf_fsard_update_A_csr above the dense entry's
capacity (tests/fsard_sparse_ref.py): on the float64 oracle and the float32 restatement alone, every row lies above
fsard_ref.CAPACITY, has a non-trivial A, keeps every decision of its loop at least fsard_ref.MARGIN from its threshold, and
the float32 restatement stays within fsard_ref.MEASURED -- so the device bound of these rows is fsard_ref.TOL, the same as
for the dense entry.  Also: the dense -> CSR helper against np.nonzero, and the `kernel=` argument of update_A_.
At the end: the rows past one grid (fsard_sparse_ref.GRID_ROWS, run by tests/test_gpu_fsard_csr_grid.py) -- the launch
geometry restated from the text of pmf_fsard_csr.hip, what each row makes the kernels do, and the same per-row guard."""
import types

import numpy as np
import pytest

import fsard_ref as fr
import fsard_sparse_ref as fs

F = np.float32


def test_rows_lie_above_the_dense_capacity_and_on_the_lane_mapping_edges():
    rows = fs.SPARSE_ROWS
    assert all(s["L"] * s["K"] > fr.CAPACITY for s in rows.values())
    assert {fr.CAPACITY + 1} == {s["L"] * s["K"] for s in rows.values() if s["K"] == 1}      # the first value past the cap
    assert min(s["L"] * s["K"] for s in rows.values() if s["K"] == 128) == 129 * 128           # ... and the first with K = 128
    assert sorted(s["K"] for s in rows.values() if s["K"] != 25) == [1, 31, 33, 64, 65, 100, 128]
    assert any(s.get("dense") for s in rows.values())
    mid = [s for s in rows.values() if s.get("c0", 1) > 1]
    assert mid and all(s["c0"] + s["Nv"] - 1 < s["N"] for s in mid)                            # a view at neither end
    assert all("max_epochs" not in s for s in rows.values())                                   # the default 6 epochs
    assert set(fs.REPRO) <= set(rows) and len(fs.AGAINST_DENSE) == 2
    for t, n in fs.AGAINST_DENSE:                                                              # legal for the dense entry
        assert fr.TABLES[t][n]["L"] * fr.TABLES[t][n]["K"] <= fr.CAPACITY


@pytest.mark.parametrize("name", list(fs.SPARSE_ROWS))
def test_row_is_not_vacuous_and_float32_stays_within_the_recorded_discrepancy(name):
    c, o = fs.sparse_row(name)
    assert c["L"] * c["K"] > fr.CAPACITY
    S = c["S"]
    assert not S[c["zero_row"]].any() and not S[:, c["zero_col"]].any()        # an empty set and an uncovered column
    assert np.mean(o["A"] > 0) >= 0.10 and o["A"].max() > 0.05, (np.mean(o["A"] > 0), o["A"].max())
    margin = fr.decision_margin(o["trace"], c["atol"])
    r = fr.run_f32(c)
    e = fr.errors(r, o, fr.fresh_ssq(c))
    print(f"FSARD_SPARSE_CPU {name} " + " ".join(f"{k}={v:.3e}" for k, v in e.items())
          + f" margin={margin:.3e} epochs={o['epochs']} branches={''.join(s['branch'] for s in o['trace'])}")
    assert margin >= fr.MARGIN, margin
    assert o["epochs"] == c["max_epochs"] == 6 and r["epochs"] == o["epochs"]
    for k, v in e.items():
        assert v <= fr.MEASURED[k], (k, v)


# ---- the dense -> CSR helper ------------------------------------------------------------------------------------------------
def _matrices():
    rng = np.random.default_rng(5)
    base = np.where(rng.random((7, 11)) < 0.3, rng.uniform(0.5, 1.5, (7, 11)), 0).astype(F)
    empty_row, empty_col, full_row = base.copy(), base.copy(), base.copy()
    empty_row[3] = 0
    empty_col[:, 4] = 0
    full_row[2] = rng.uniform(0.5, 1.5, 11).astype(F)
    return {"empty_row": empty_row, "empty_col": empty_col, "full_row": full_row, "all_zero": np.zeros((3, 5), F),
            "one_by_one": np.ones((1, 1), F), "case": fr.make_case(**fr.BASE)["S"]}


@pytest.mark.parametrize("name", ["empty_row", "empty_col", "full_row", "all_zero", "one_by_one", "case"])
def test_dense_to_csr_is_the_row_major_scan(pkg, name):
    S = _matrices()[name]
    rowptr, col, val = pkg._lib.dense_to_csr(S)
    rp, c, v = fs.csr_by_nonzero(S)
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and val.dtype == F
    assert np.array_equal(rowptr, rp) and np.array_equal(col, c) and np.array_equal(val, v)
    assert rowptr[0] == 0 and rowptr[-1] == col.size == np.count_nonzero(S) and np.all(np.diff(rowptr) >= 0)
    for l in range(S.shape[0]):
        assert np.all(np.diff(col[rowptr[l]:rowptr[l + 1]]) > 0)                # strictly ascending within a row
    assert np.array_equal(fs.csr_to_dense(rowptr, col, val, S.shape[1]), S)
    if name == "empty_row":
        assert rowptr[3] == rowptr[4]
    if name == "empty_col":
        assert 4 not in col
    if name == "full_row":
        assert np.array_equal(col[rowptr[2]:rowptr[3]], np.arange(11))


def test_a_stored_zero_triple_is_the_same_matrix():
    """Stored zeros are legal in the library's CSR: a triple with explicit zeros densifies to the matrix without them, and
    the helper never emits one."""
    S = _matrices()["empty_col"]
    rowptr, col, val = fs.csr_by_nonzero(S)
    # add column 4 (all zero in S) to every row that lacks it, as a stored zero
    rp2, c2, v2 = [0], [], []
    for l in range(S.shape[0]):
        cols = list(col[rowptr[l]:rowptr[l + 1]]) + [4]
        vals = list(val[rowptr[l]:rowptr[l + 1]]) + [0.0]
        order = np.argsort(cols)
        c2 += [cols[i] for i in order]
        v2 += [vals[i] for i in order]
        rp2.append(len(c2))
    assert len(c2) == col.size + S.shape[0] and v2.count(0.0) == S.shape[0]
    assert np.array_equal(fs.csr_to_dense(np.array(rp2), np.array(c2), np.array(v2, F), S.shape[1]), S)


def test_view_csr_converts_once_per_array(pkg):
    reg = types.SimpleNamespace(S=(_matrices()["empty_row"], _matrices()["full_row"]))
    a = pkg.featureset_ard.view_csr(reg, 0)
    assert pkg.featureset_ard.view_csr(reg, 0) is a                             # kept on the regularizer
    assert np.array_equal(a[1], fs.csr_by_nonzero(reg.S[0])[1])
    b = pkg.featureset_ard.view_csr(reg, 1)
    assert np.array_equal(b[2], fs.csr_by_nonzero(reg.S[1])[2])
    reg.S = (reg.S[1], reg.S[1])                                                # another array in the view's place
    c = pkg.featureset_ard.view_csr(reg, 0)
    assert c is not a and np.array_equal(c[0], b[0])


@pytest.mark.parametrize("kernel", ["csr", "", None, "Dense"])
def test_update_A_refuses_an_unknown_kernel(pkg, kernel):
    """Raised before a context is made or touched: no GPU needed."""
    reg = types.SimpleNamespace(S=(), A=(), col_ranges=())
    with pytest.raises(ValueError, match="kernel"):
        pkg.update_A_(reg, np.zeros((2, 3), F), kernel=kernel)
    assert pkg.featureset_ard.FSARD_DENSE_CAPACITY == fr.CAPACITY


# ---- the rows past one grid (fs.GRID_ROWS; tests/test_gpu_fsard_csr_grid.py) ---------------------------------------------------
def test_launch_constants_are_read_from_the_source():
    """A changed cap or block size fails here; an unmatched pattern gives None and fails too, instead of emptying the rows."""
    sc = fs.csr_source_constants()
    assert sc == dict(N_WG_CAP=2048, G_UPD_CAP=4096, UPD_THREADS=256, WAVES=4, LANES=64, KP_WIDE=64, K_PACKED=32, PER=True,
                      DECIDE_THREADS=1024, UPD_BLOCK=256, FORWARD_TRIP=True), sc
    assert sc["UPD_THREADS"] == sc["UPD_BLOCK"]                                 # g_upd counts blocks of the size it launches


def test_grid_rows_leave_one_grid_where_they_say():
    rows, sc = fs.GRID_ROWS, fs.csr_source_constants()
    assert list(rows) == ["Nv8197_K33", "Nv16500_K65", "Nv16390_K25", "Nv32800_K16_mid", "LK_8200x128"]
    assert fs.GRID_WIDE == tuple(rows)[:4]
    geo = {n: fs.launch_geometry(s["L"], s["K"], s["Nv"]) for n, s in rows.items()}
    want = {"Nv8197_K33": dict(kp=64, step=4, per=5, trips=2, empty=408), "Nv16500_K65": dict(kp=64, step=4, per=9, trips=3),
            "Nv16390_K25": dict(kp=32, step=8, per=9, trips=2), "Nv32800_K16_mid": dict(kp=16, step=16, per=17, trips=2)}
    for n in fs.GRID_WIDE:
        g = geo[n]
        assert g["n_wg"] == sc["N_WG_CAP"] > sc["DECIDE_THREADS"]               # k_fsc_decide: more than one partial per thread
        assert g["per"] > g["step"] and g["trips"] >= 2                         # k_fsc_forward: more than one trip over the slice
        assert {k: g[k] for k in want[n]} == want[n], (n, g)
        assert g["upd_trips"] == 1
    assert sum(1 for n in fs.GRID_WIDE if geo[n]["per"] % geo[n]["step"]) >= 2   # slices that are no multiple of the step
    assert any(g["n_wg"] * g["per"] - rows[n]["Nv"] >= g["per"] and g["empty"] > 0 for n, g in geo.items())   # workgroups without a column
    assert rows["Nv16500_K65"]["K"] > 64                                        # two factors per lane
    assert [64 // geo[n]["kp"] for n in fs.GRID_WIDE] == [1, 1, 2, 4]           # columns per wave
    mid = rows["Nv32800_K16_mid"]
    assert mid["c0"] > 1 and mid["c0"] + mid["Nv"] - 1 < mid["N"]               # a view at neither end of the model
    big = rows["LK_8200x128"]
    assert big["L"] * big["K"] > sc["G_UPD_CAP"] * sc["UPD_BLOCK"] and geo["LK_8200x128"]["g_upd"] == sc["G_UPD_CAP"]
    assert geo["LK_8200x128"]["upd_trips"] == 2                                 # k_fsc_update: the second grid-stride trip
    # no row of the first table does any of this
    for s in fs.SPARSE_ROWS.values():
        g = fs.launch_geometry(s["L"], s["K"], s["Nv"])
        assert g["trips"] == 1 and g["empty"] == 0 and g["n_wg"] <= sc["DECIDE_THREADS"] and g["upd_trips"] == 1
    assert all("max_epochs" not in s for s in rows.values())                    # the default 6 epochs
    assert fs.GRID_AGAINST_DENSE == fs.GRID_WIDE[:3] and all(rows[n]["L"] * rows[n]["K"] <= fr.CAPACITY for n in fs.GRID_AGAINST_DENSE)
    assert set(fs.GRID_REPRO) == {"Nv8197_K33", "LK_8200x128"} and fs.GRID_EARLY_STOP[0] == "Nv8197_K33"


@pytest.mark.parametrize("name", list(fs.GRID_ROWS))
def test_grid_row_is_not_vacuous_and_float32_stays_within_the_recorded_discrepancy(name):
    c, o = fs.grid_row(name)
    S = c["S"]
    assert not S[c["zero_row"]].any() and not S[:, c["zero_col"]].any()        # an empty set and an uncovered column
    assert np.mean(o["A"] > 0) >= 0.10 and o["A"].max() > 0.05, (np.mean(o["A"] > 0), o["A"].max())
    margin = fr.decision_margin(o["trace"], c["atol"])
    r = fr.run_f32(c)
    e = fr.errors(r, o, fr.fresh_ssq(c))
    print(f"FSARD_GRID_CPU {name} " + " ".join(f"{k}={v:.3e}" for k, v in e.items())
          + f" margin={margin:.3e} epochs={o['epochs']} branches={''.join(s['branch'] for s in o['trace'])}")
    assert margin >= fr.MARGIN, margin
    assert o["epochs"] == c["max_epochs"] == 6 and r["epochs"] == o["epochs"]
    for k, v in e.items():
        assert v <= fr.MEASURED[k], (k, v)


def test_the_early_stop_at_width_ends_before_max_epochs_with_its_margin():
    rule = fs.early_stop_rule()
    assert fs.GRID_EARLY_STOP[1] in fr.STOP_RULES and rule == {k: fr.STOP_RULES[fs.GRID_EARLY_STOP[1]][k] for k in rule}
    c, o = fs.early_stop_run()
    margin = fr.decision_margin(o["trace"], rule["atol"])
    r = fr.run_f32(c, **rule)
    e = fr.errors(r, o, fr.fresh_ssq(c))
    print(f"FSARD_GRID_CPU early stop {fs.GRID_EARLY_STOP} " + " ".join(f"{k}={v:.3e}" for k, v in e.items())
          + f" margin={margin:.3e} epochs={o['epochs']} branches={''.join(s['branch'] for s in o['trace'])}")
    assert margin >= fr.MARGIN, margin
    assert 0 < o["epochs"] == r["epochs"] < rule["max_epochs"]                 # the counter ends the loop, not max_epochs
    assert (o["epochs"] + 1) % max(8, rule["term_iter"]) != 0                   # ... inside a batch: launches are queued past the end
    assert o["A"].max() > 0.05
    for k, v in e.items():
        assert v <= fr.MEASURED[k], (k, v)
