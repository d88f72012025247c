"""CPU guard of the FeatureSetARD outer-loop tables (tests/fsard_ref.py), on the float64 oracle and the float32
restatement alone, so that no row of tests/test_gpu_fsard_edges.py can pass vacuously: every compared run has a
non-trivial A, every decision of its loop (improved / by more than atol) is far from its threshold, the stopping rows
take the branches they are named for, the rows sit on the geometry edges they claim (with the constants read out of
csrc/pmf_fsard.hip), and the float32 restatement stays within the recorded discrepancy that the device bounds derive from."""
import numpy as np
import pytest

import fsard_ref as fr

CASES = [pytest.param(name, spec, id=f"{t}-{name}") for t, name, spec in fr.all_cases()]


def branches(o):
    return "".join(s["branch"] for s in o["trace"])


def test_geometry_constants_are_the_ones_in_the_kernel_source():
    """A change of geometry in pmf_fsard.hip must fail here instead of silently moving the cases off their edges."""
    got = fr.source_constants()
    assert got["CW_MAX"] == fr.CW_MAX == 256
    assert got["LDS_LIMIT"] == [fr.LDS_LIMIT] == [150 * 1024]
    assert got["MAXO"] == fr.MAXO == 64
    assert got["THREADS"] == 256
    assert got["CAPACITY"] == fr.CAPACITY == got["MAXO"] * got["THREADS"] == 16384
    assert got["MAX_WG"] == fr.MAX_WG == 32


def test_cw_rows_lie_on_both_sides_of_the_lds_rule():
    for (La, K), (Lb, Kb) in (fr.CW_PAIRS[:2], fr.CW_PAIRS[2:]):
        assert K == Kb and Lb == La + 1
        assert fr.lds_bytes(La, K, 256) <= fr.LDS_LIMIT < fr.lds_bytes(Lb, K, 256)       # the last 256 and the first 128
        assert fr.sub_slice_width(La, K) == 256 and fr.sub_slice_width(Lb, K) == 128
        assert fr.lds_bytes(Lb, K, 128) <= fr.LDS_LIMIT
    for name, spec in fr.CW_EDGES.items():
        cw = fr.sub_slice_width(spec["L"], spec["K"])
        assert spec["Nv"] in (cw - 1, cw, cw + 1, fr.MAX_WG * cw + 1), name
    big = fr.CW_EDGES["44x128_Nv4097"]
    cw = fr.sub_slice_width(big["L"], big["K"])
    assert cw == 128 and fr.n_workgroups(big["L"], big["K"], big["Nv"]) == fr.MAX_WG
    assert -(-big["Nv"] // fr.MAX_WG) > cw                     # a workgroup's slice is wider than one sub-slice
    assert {(s["L"], s["K"], s["Nv"]) for s in fr.CW_EDGES.values()} >= {
        (L, K, fr.sub_slice_width(L, K) + d) for L, K in fr.CW_PAIRS for d in (-1, 0, 1)}


def test_tables_hold_the_edges_they_are_named_for():
    assert sorted(s["K"] for s in fr.K_EDGES.values()) == [1, 31, 32, 33, 64, 65, 100, 128]
    assert all(fr.sub_slice_width(s["L"], s["K"]) == 256 and s["Nv"] % 256 for s in fr.K_EDGES.values())
    lk = sorted(s["L"] * s["K"] for s in fr.OUTPUTS.values())
    assert {255, 256, 257, fr.CAPACITY} <= set(lk) and lk.count(fr.CAPACITY) == 2
    assert any(s["L"] == 1 for s in fr.OUTPUTS.values())
    assert {(s["L"], s["K"]) for s in fr.OUTPUTS.values()} >= {(128, 128), (16384, 1)}
    nv = {s["Nv"] for s in fr.NV_POSITIONS.values()}
    assert nv == {1, 255, 256, 257, 32 * 256, 32 * 256 + 1}
    for s in fr.NV_POSITIONS.values():
        assert fr.sub_slice_width(s["L"], s["K"]) == 256
    for Nv in nv:
        pos = {(s["c0"] == 1, s["c0"] + s["Nv"] - 1 == s["N"]) for s in fr.NV_POSITIONS.values() if s["Nv"] == Nv}
        assert pos == {(True, False), (False, True), (False, False)}                      # first, last, middle
    assert sorted(s["max_epochs"] for s in fr.MAX_EPOCHS.values()) == [0, 1, 7, 8, 9, 16, 17]
    assert all(s["term_iter"] > s["max_epochs"] for s in fr.MAX_EPOCHS.values())
    assert sorted(s["term_iter"] for s in fr.TERM_ITER.values()) == [1, 3, 8, 9]
    assert fr.BASE["K"] % 32 != 0                                                           # K < Kp: beta_out's pitch
    assert any(fr.sub_slice_width(s["L"], s["K"]) == 128 for s in fr.REPRO.values())
    assert any(s["Nv"] == 8193 for s in fr.REPRO.values())


def test_generator_plants_the_structure_the_cases_rely_on():
    c = fr.make_case(**fr.BASE)
    S, Yv = c["S"], fr.view_Y(c)
    assert not S[c["zero_row"]].any() and not S[:, c["zero_col"]].any()                     # an empty set, an uncovered column
    w = S[S > 0]
    assert w.min() > 0 and w.max() / w.min() > 1.5                                          # non-uniform positive weights
    assert np.ptp(c["alpha"]) > 0.1
    assert (Yv == 0).sum() >= 3 and (Yv > 0.5).any() and (Yv < -0.5).any()
    d = fr.make_case(**fr.OUTPUTS["dense_12x20"])["S"]
    assert (d > 0).mean() > 0.9


@pytest.mark.parametrize("name, spec", CASES)
def test_case_is_not_vacuous_and_float32_stays_within_the_recorded_discrepancy(name, spec):
    c = fr.make_case(**spec)
    o = fr.run_oracle(c)
    if name in fr.ZERO_A:
        assert not o["A"].any()
    else:
        assert np.mean(o["A"] > 0) >= 0.10 and o["A"].max() > 0.05, (np.mean(o["A"] > 0), o["A"].max())
    assert fr.decision_margin(o["trace"], c["atol"]) >= fr.MARGIN, fr.decision_margin(o["trace"], c["atol"])
    r = fr.run_f32(c)
    assert r["epochs"] == o["epochs"]
    e = fr.errors(r, o, fr.fresh_ssq(c))
    for k, v in e.items():
        assert v <= fr.MEASURED[k], (k, v)


def test_margin_bound_follows_from_the_measured_loss_discrepancy():
    assert fr.MARGIN == 1000 * fr.MEASURED["loss"] and fr.A_BEST_GAP == 100 * 20 * fr.MEASURED["A"]
    assert all(fr.TOL[k] == 20 * fr.MEASURED[k] for k in fr.MEASURED)


def test_mixed_trace_resets_the_counter_and_ends_away_from_the_last_iterate():
    full = fr.run_oracle(fr.make_case(**fr.TERM_ITER["term_iter9"]))
    br = branches(full)
    assert br[0] == "w"                                                                     # term_iter = 1 still moves A
    assert any(a == "b" and b == "w" for a, b in zip(br, br[1:])), br                      # a reset after a rise
    assert br.endswith("b" * 9) and full["epochs"] < fr.MIXED["max_epochs"], br             # ended by the counter
    epochs = []
    for name, spec in fr.TERM_ITER.items():
        c = fr.make_case(**spec)
        o = fr.run_oracle(c)
        t = spec["term_iter"]
        assert branches(o) == br[:o["epochs"]] and branches(o).endswith("b" * t) and o["trace"][-1]["term_count"] == t
        assert o["epochs"] < c["max_epochs"]
        last = fr.last_iterate(c, o["epochs"])
        assert fr.norm_err(last, o["A"]) > fr.A_BEST_GAP, name                              # returning the last A fails
        epochs.append(o["epochs"])
    assert len(set(epochs)) == 4, epochs                                                     # each term_iter ends elsewhere


def test_stop_rule_rows_take_the_branches_they_are_named_for():
    for name in ("strong_lambda", "strong_lambda_negative_atol"):
        c = fr.make_case(**fr.STOP_RULES[name])
        o = fr.run_oracle(c)
        assert branches(o) == "b" * c["term_iter"] and all(s["same_A"] for s in o["trace"]) and not o["A"].any()
        assert o["epochs"] == c["term_iter"] < c["max_epochs"]
        grown = o["ssq"][np.arange(c["L"]) != c["zero_row"]]
        assert np.all(grown > 2e-8) and np.median(grown) > 1.0                               # ... while ssq_grad still grows
        assert not fr.run_f32(c)["A"].any()
    assert fr.STOP_RULES["strong_lambda_negative_atol"]["atol"] < 0
    c = fr.make_case(**fr.STOP_RULES["atol_1e30"])
    o = fr.run_oracle(c)
    assert branches(o) == "s" * c["term_iter"] and o["epochs"] == c["term_iter"] < c["max_epochs"]
    assert fr.norm_err(fr.last_iterate(c, o["epochs"]), o["A"]) == 0                        # A is the last iterate
    assert branches(fr.run_oracle(c, atol=1e-5)) == "w" * c["max_epochs"]                   # atol alone ends this run
    c = fr.make_case(**fr.STOP_RULES["atol_0"])
    o = fr.run_oracle(c)
    assert branches(o) == "w" * c["max_epochs"]
    for spec in fr.MAX_EPOCHS.values():
        assert fr.run_oracle(fr.make_case(**spec))["epochs"] == spec["max_epochs"]


def test_second_calls_of_the_state_rows():
    """The float32 restatement carried across two calls, against the oracle doing the same."""
    c = fr.make_case(**fr.STATE["two_calls"])
    o1, r1 = fr.run_oracle(c), fr.run_f32(c)
    o2, r2 = fr.run_oracle(c, ssq_in=o1["ssq"]), fr.run_f32(c, ssq_in=r1["ssq"])
    assert fr.decision_margin(o2["trace"], c["atol"]) >= fr.MARGIN
    assert np.mean(o2["A"] > 0) >= 0.10 and o2["A"].max() > 0.05
    assert fr.norm_err(o2["A"], o1["A"]) > fr.A_BEST_GAP                                    # a fresh accumulator would show
    fresh = fr.run_oracle(c)
    assert fr.ssq_err(fresh["ssq"], fr.fresh_ssq(c), o2["ssq"], o1["ssq"]) > 100 * fr.TOL["ssq"]
    for k, v in fr.errors(r2, o2, r1["ssq"], o1["ssq"]).items():
        assert v <= fr.MEASURED[k], (k, v)
    a, b = fr.make_case(**fr.STATE["after_set_Y"]), fr.make_case(**fr.STATE["after_set_Y_second"])
    oa, ob = fr.run_oracle(a), fr.run_oracle(a, Y=b["Y"])
    assert fr.decision_margin(ob["trace"], a["atol"]) >= fr.MARGIN
    assert np.mean(ob["A"] > 0) >= 0.10 and ob["A"].max() > 0.05
    assert fr.norm_err(oa["A"], ob["A"]) > fr.A_BEST_GAP                                    # the old Y would show
    for k, v in fr.errors(fr.run_f32(a, Y=b["Y"]), ob, fr.fresh_ssq(a)).items():
        assert v <= fr.MEASURED[k], (k, v)


@pytest.mark.parametrize("name", sorted(fr.NV_POSITIONS) + ["beta_dest"])
def test_one_overwritten_column_outside_the_view_moves_the_regularizer_value(name):
    spec = fr.NV_POSITIONS.get(name, fr.BETA_DEST)
    c = fr.make_case(**spec)
    o = fr.run_oracle(c)
    assert fr.BETA_UPLOADED >= 10 * o["beta"].max()
    al = fr.reg_alpha(c["N"])
    b = fr.beta_after(c, o["beta"])
    want = fr.reg_value(al, b, c["Y"])
    typical = float(np.median(o["beta"]))
    neighbours = [j for j in (c["c0"] - 2, c["c1"]) if 0 <= j < c["N"]]                     # 0-based, next to the view
    assert neighbours and len(neighbours) == (2 if c["c0"] > 1 and c["c1"] < c["N"] else 1)
    for j in neighbours + [0, c["N"] - 1]:
        if c["c0"] - 1 <= j < c["c1"]:
            continue
        b2 = b.copy()
        b2[:, j] = typical
        assert abs(fr.reg_value(al, b2, c["Y"]) - want) > 10 * fr.REG_TOL * want, (name, j)
    # ... and a view that was not written at all (beta as uploaded) is further off still
    assert abs(fr.reg_value(al, fr.beta_after(c, fr.BETA_UPLOADED), c["Y"]) - want) > 100 * fr.REG_TOL * want
