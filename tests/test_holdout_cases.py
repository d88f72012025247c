"""Hold-out entries without a device: the extension header against its signature table and struct mirror, the symbols the
library exports, the float32 twin of tests/holdout_ref.py against the rounding bound (and the measured constant against the
twin), the bookkeeping of the Python layer, and the early-stopping rule on the CPU oracle's trace of the overfitting problem."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import abi_header
import holdout_ref as ho
from problems import to_oracle

CASES = [(name, s) for name in ho.cases() for s in ("wide", "corners")]


def test_the_extension_header_matches_its_signature_table(pkg, monkeypatch):
    from test_abi import signature_errors, struct_errors
    monkeypatch.setattr(abi_header, "HEADER", abi_header.HEADER.parent / "pmf_hip_holdout.h")
    protos, structs = abi_header.parse()
    abi = pkg._abi
    assert list(structs) == ["pmf_holdout_opts"] and len(protos) == 7
    assert list(protos) == list(abi.HOLDOUT_SIGNATURES)
    both = SimpleNamespace(STRUCTS={**abi.STRUCTS, **abi.HOLDOUT_STRUCTS}, HOST_ALLREDUCE_FN=abi.HOST_ALLREDUCE_FN)
    assert signature_errors(both, abi.HOLDOUT_SIGNATURES, protos) == []
    assert struct_errors(both, abi.HOLDOUT_STRUCTS, structs) == []
    assert ctypes.sizeof(abi.HoldoutOpts) == 24
    assert not set(abi.HOLDOUT_SIGNATURES) & (set(abi.SIGNATURES) | set(abi.THRESHOLD_SIGNATURES) | set(abi.IMPORTANCE_SIGNATURES))
    lib = pkg._lib.load_library()
    for name, (restype, argtypes) in abi.HOLDOUT_SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    with pytest.raises(ctypes.ArgumentError):
        lib.pmf_set_holdout(None, 1.5, None, None, None)
    txt = abi_header.HEADER.read_text()
    assert f"#define PMF_TERM_HOLDOUT {abi.TERM_HOLDOUT} " in txt and abi.TERM[abi.TERM_HOLDOUT] == "holdout_increase"
    assert "pmf_hip_holdout" not in (abi_header.HEADER.parent / "pmf_hip.h").read_text()      # pmf_hip.h stays untouched


def test_every_new_symbol_is_exported(pkg):
    lib = ctypes.CDLL(str(pkg._lib.LIB_PATH))
    for name in pkg._abi.HOLDOUT_SIGNATURES:
        assert hasattr(lib, name), f"{name} declared in include/pmf_hip_holdout.h but not exported"
    for name in ("sample_holdout", "set_holdout_", "clear_holdout_", "holdout_scores"):
        assert getattr(pkg, name) is getattr(pkg.holdout, name)


@pytest.mark.parametrize("name,which", CASES)
def test_the_float32_twin_is_within_a_bound_that_says_something(name, which):
    p = ho.cases()[name]
    rows, cols = ho.held_sets(p)[which]
    ref, tw = ho.reference(p, rows, cols), ho.twin(p, rows, cols)
    ratio = ho.worst_ratio(p, rows, cols)
    print(f"{name}/{which}: twin error / (eps x bracket) = {ratio:.3f} (C = {ho.C})")
    assert 2 * ratio <= ho.C, ratio                                              # C is twice the worst measured ratio
    worst = ho.check(tw["loss_col"], tw["n_col"], tw["total"], p, rows, cols)
    share = float(np.mean(ho.bound(ref) > 0.1 * np.abs(ref["loss_col"])))
    print(f"{name}/{which}: twin at {worst:.3f} of the bound; bound above a tenth of the value on {100 * share:.1f} % of the columns")
    assert share <= 0.05
    assert ref["n_col"][7] == 0 and ref["loss_col"][7] == 0 if which == "wide" else True
    assert abs(ref["total"] - ref["loss_col"].sum()) <= 1e-12 * abs(ref["total"])


def test_the_constant_is_the_measured_one():
    worst = max(ho.worst_ratio(p, *ho.held_sets(p)[s]) for p in ho.cases().values() for s in ("wide", "corners"))
    print(f"worst ratio over the case table: {worst:.3f}")
    assert ho.C / 2 * 0.95 <= worst <= ho.C / 2                                  # neither stale nor outgrown


def test_the_held_sets_reach_their_edges():
    p = ho.cases()["k33"]
    rows, cols = ho.held_sets(p)["wide"]
    r, c, v, Dm = ho.held_after_set(np.asarray(p["D"]), rows, cols)
    assert not np.array_equal(np.lexsort((rows, cols)), np.arange(rows.size))     # the input is unsorted
    assert np.array_equal(np.lexsort((r, c)), np.arange(r.size))                  # ... the kept set sorted by (column, row)
    assert r.size < rows.size and np.isnan(np.asarray(p["D"])[rows, cols]).any()  # entries that were missing already
    assert (p["M"] - 1) in r[c == p["N"] - 1] or (r == p["M"] - 1).any() and (c == p["N"] - 1).any()
    assert not (c == 7).any() and (c == 40).sum() > 32                            # a column with none; one past two units of 16
    assert np.isfinite(v).all() and np.isnan(Dm[r, c]).all()
    assert np.array_equal(np.isnan(Dm).sum(), np.isnan(np.asarray(p["D"])).sum() + r.size)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_entries_are_sorted_and_bad_ones_refused(pkg):
    chk = pkg.holdout._check_entries
    r, c = chk([5, 0, 3, 2], [1, 1, 0, 1], 7, 4)
    assert r.tolist() == [3, 0, 2, 5] and c.tolist() == [0, 1, 1, 1]
    sr, sc = ho.sort_entries([5, 0, 3, 2], [1, 1, 0, 1], 7)
    assert np.array_equal(sr, r) and np.array_equal(sc, c)
    with pytest.raises(ValueError, match=r"entry 2 = \(7, 0\) is outside"):
        chk([0, 1, 7], [0, 0, 0], 7, 4)
    with pytest.raises(ValueError, match=r"entry 1 = \(0, -1\) is outside"):
        chk([0, 0], [0, -1], 7, 4)
    with pytest.raises(ValueError, match=r"entry 3 = \(2, 1\) is a duplicate"):
        chk([2, 4, 6, 2, 4], [1, 1, 1, 1, 1], 7, 4)                              # the first repeat in the caller's order
    with pytest.raises(ValueError, match="3 rows but 2 columns"):
        chk([0, 1, 2], [0, 1], 7, 4)


def test_sample_holdout_draws_observed_entries_reproducibly(pkg):
    p = ho.cases()["k4"]
    D = np.array(p["D"])
    D[3:, 5] = np.nan                                                            # three observed entries at most in column 5
    D[:, 6] = np.nan                                                             # none in column 6
    model = SimpleNamespace(data=D)
    r, c = pkg.sample_holdout(model, 0.3, seed=1)
    assert np.isfinite(D[r, c]).all() and r.size > 0
    assert np.array_equal(np.lexsort((r, c)), np.arange(r.size)) and np.unique(c * D.shape[0] + r).size == r.size
    n_obs, n_held = np.isfinite(D).sum(0), np.bincount(c, minlength=D.shape[1])
    assert ((n_obs - n_held >= 2) | (n_held == 0)).all() and n_held[6] == 0
    assert abs(r.size - 0.3 * n_obs.sum()) <= 0.02 * n_obs.sum()
    r2, c2 = pkg.sample_holdout(model, 0.3, seed=1)
    assert np.array_equal(r, r2) and np.array_equal(c, c2)
    r3, c3 = pkg.sample_holdout(model, 0.3, seed=2)
    assert not (np.array_equal(r, r3) and np.array_equal(c, c3))
    # min_train_per_column: with 90 % drawn, a column keeps its draws only if enough would remain
    r4, c4 = pkg.sample_holdout(model, 0.9, seed=3, min_train_per_column=8)
    held4 = np.bincount(c4, minlength=D.shape[1])
    assert ((n_obs - held4 >= 8) | (held4 == 0)).all() and (held4 == 0).any() and (held4 > 0).any()
    with pytest.raises(ValueError):
        pkg.sample_holdout(model, 1.5, seed=0)


def test_a_sharded_model_and_a_second_set_are_refused(pkg):
    with pytest.raises(ValueError, match="row-sharded"):
        pkg.set_holdout_(SimpleNamespace(sharded=True, data=np.zeros((3, 3), np.float32)), [0], [0])
    with pytest.raises(ValueError, match="already has a hold-out set"):
        pkg.set_holdout_(SimpleNamespace(sharded=False, holdout={}, data=np.zeros((3, 3), np.float32)), [0], [0])


# ---- the early-stopping rule -------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_made_traces():
    rule = ho.stopping_rule
    assert rule([1, 2, 3, 4, 5, 6], [5, 4, 4.5, 4.2, 4.1, 3], 3) == (5, 2, 4.0, 5)
    assert rule([1, 2, 3, 4, 5, 6], [5, 4, 4.5, 4.2, 4.1, 3], 0) == (None, 6, 3.0, 6)        # patience 0 only records
    assert rule([1, 4, 7], [5, 4.95, 4.93], 2, min_delta=0.1) == (7, 1, 5.0, 3)               # not better by min_delta
    assert rule([1, 2, 3], [np.nan, np.nan, 2.0], 2)[0] == 2                                   # no finite value in `patience`
    assert rule([1, 2], [3.0, 2.0], 1) == (None, 2, 2.0, 2)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_oracle_overfits_where_the_rule_can_see_it(seed):
    """The overfitting problem on the CPU oracle, one epoch per call (its optimizer state persists): the hold-out minimum e*
    satisfies 3 <= e* <= max_epochs - patience - 2, and no rule on the training loss fires before e* + patience."""
    o = ho.OVERFIT
    p, rows, cols = ho.overfit_problem(seed)
    m = to_oracle(ho.masked(p, rows, cols))
    H, L = [], []
    for e in range(1, o["max_epochs"] + 1):
        H.append(ho.normal_holdout_loss(m.X, m.Y, p["D"], rows, cols))            # the parameters epoch e's data pass sees
        r = m.fit(update_X=True, update_Y=True, lr=o["lr"], max_epochs=e, epoch=e, abs_tol=0, rel_tol=0)
        assert r["term_code"] == "max_epochs" and len(r["loss"]) == 1
        L.append(r["loss"][0])
    H, L = np.array(H), np.array(L)
    e_star = int(np.argmin(H)) + 1
    stop, best, _, _ = ho.stopping_rule(range(1, len(H) + 1), H, o["patience"])
    print(f"seed {seed}: e* = {e_star}, stop = {stop}, best = {best}, H(e*) = {H[e_star - 1]:.4f}, H(1) = {H[0]:.4f}, H(end) = {H[-1]:.4f}")
    assert 3 <= e_star <= o["max_epochs"] - o["patience"] - 2
    until = min(e_star + o["patience"], len(L))
    d = L[:until - 1] - L[1:until]                                                # prev - loss, as pmf_fit forms it
    assert (d >= 0).all()                                                         # no loss increase
    assert (np.abs(d) >= 1e-9).all() and (np.abs(d / L[1:until]) >= 1e-6).all()   # neither default tolerance
    assert stop is not None and best <= stop - o["patience"] and H[best - 1] <= H[:stop].min() + 1e-12
