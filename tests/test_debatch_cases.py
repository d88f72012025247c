"""tests/debatch_ref.py checked on the CPU: the float32 twin against the float64 rule inside the derived bound, what must be
exact is exact, debatch undoes the batch layers of impute_ref's link-space values, and the problems can tell a wrong rule
from the right one (a neighbouring column's mu, a row in the neighbouring batch, the reference's old-order formula)."""
import numpy as np
import pytest

import hinge_ref
from debatch_ref import LINK, MUTATIONS, debatch_ref, debatch_tol, has_batch, link_kinds, same_bits, worst_ratio
from impute_ref import BATCH, LINK as I_LINK, case_problem, impute_ref, impute_tol, link_space


def problems():
    ps = [("mixed-300x129", case_problem(33, 300, 129)), ("mixed-257x65", case_problem(33, 257, 65))]
    ps += [(name, p) for name, p in hinge_ref.all_problems() if name in ("A-k20-batch", "B-k20-batch")]
    return ps


PROBLEMS = problems()
IDS = [n for n, _ in PROBLEMS]


def inputs(p):
    """The data itself (0/1, counts, class labels, NaN), and the model's own predictions with batch effects (fractional
    probabilities and rates) with the data's missing pattern."""
    D = np.asarray(p["D"], np.float32)
    if any(k == 3 for k in hinge_ref.kinds_of(p)):
        return [("data", D)]
    pred = impute_ref(p, BATCH)[0].astype(np.float32)
    return [("data", D), ("predictions", np.where(np.isnan(D), np.float32(np.nan), pred))]


def test_the_problems_exercise_the_rule():
    kinds = set()
    for _, p in PROBLEMS:
        kinds |= set(int(k) for k in hinge_ref.kinds_of(p))
        has = has_batch(p)
        assert has.any() and not has.all()
        bors = [np.asarray(v["batch_of_row"]) for v in p["batch_views"]]
        assert any((b < 0).any() for b in bors), "no row without a batch"
        seams = [v["stop1"] for v in p["batch_views"]] + [v["start1"] - 1 for v in p["batch_views"]]
        assert any(s % 32 and 0 < s < p["N"] for s in seams), "no view seam inside a 32-column tile"
    assert kinds == {0, 1, 2, 3}


@pytest.mark.parametrize("name,p", PROBLEMS, ids=IDS)
def test_twin_is_within_the_bound(name, p):
    for vname, V in inputs(p):
        for flags in (0, LINK):
            want, _, _ = debatch_ref(p, V, flags)
            got, _, _ = debatch_ref(p, V, flags, np.float32)
            assert got.dtype == np.float32
            r = worst_ratio(got, want, debatch_tol(p, V, flags))
            print(f"{name} {vname} flags={flags}: twin worst |error| / bound = {r:.3f}")
            assert r <= 1.0, (vname, flags, r)


@pytest.mark.parametrize("name,p", PROBLEMS, ids=IDS)
def test_entries_returned_as_given_are_bitwise(name, p):
    V = np.array(p["D"], np.float32)
    V[1, :] = np.float32(np.inf)                                  # not finite, but in a batch or not as the row says
    for flags in (0, LINK):
        got, _, _ = debatch_ref(p, V, flags, np.float32)
        keep = ~has_batch(p) | (link_kinds(p, flags) == 3)[None, :]
        all_labels = bool((link_kinds(p, flags) == 3).all())          # layout B without LINK: nothing but class labels
        assert keep.any() and keep.all() == all_labels
        assert same_bits(got[keep], V[keep])
        missing = ~np.isfinite(V) & ~keep
        assert missing.any() != all_labels and np.isnan(got[missing]).all()


def test_zero_one_and_zero_counts_come_back_exactly():
    p = case_problem(33, 300, 129)
    kind = hinge_ref.kinds_of(p)
    V = np.asarray(p["D"], np.float32)
    for dtype in (np.float64, np.float32):
        got, lp, _ = debatch_ref(p, V, 0, dtype)
        b = np.isfinite(V) & (kind == 1)[None, :]
        assert b.any() and set(np.unique(V[b])) == {0.0, 1.0}
        assert np.array_equal(got[b], V[b])
        z = (V == 0) & (kind == 2)[None, :]
        assert z.any() and np.all(got[z] == 0)
        assert np.isinf(lp[b & has_batch(p)]).all()
    # outside a link's domain: NaN, nothing raised
    W = V.copy()
    W[:, kind == 1] = np.float32(1.5)
    W[:, kind == 2] = np.float32(-1.0)
    got, _, _ = debatch_ref(p, W, 0, np.float32)
    bad = has_batch(p) & (kind != 0)[None, :]
    assert np.isnan(got[bad]).all() and same_bits(got[~has_batch(p)], W[~has_batch(p)])


@pytest.mark.parametrize("name,p", PROBLEMS[:2], ids=IDS[:2])
def test_debatch_undoes_the_batch_layers_of_the_link_space_values(name, p):
    want = link_space(p, 0)
    zb = link_space(p, BATCH)
    # float64 all the way: the rule is the inverse of the layers up to float64 rounding
    got64, _, _ = debatch_ref(p, zb, LINK)
    assert np.max(np.abs(got64 - want) / (1 + np.abs(want))) < 1e-12
    # float32: within the sum of the two bounds -- the input's own (divided by delta on the way) and the correction's
    V = link_space(p, BATCH, np.float32)
    e_in = impute_tol(p, BATCH | I_LINK, zb)
    got, _, _ = debatch_ref(p, V, LINK, np.float32)
    r = worst_ratio(got, want, debatch_tol(p, V, LINK, e_in=e_in))
    print(f"{name}: identity worst |error| / bound = {r:.3f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("mutate", MUTATIONS)
@pytest.mark.parametrize("name,p", PROBLEMS[:2], ids=IDS[:2])
def test_a_wrong_rule_is_ten_bounds_away(name, p, mutate):
    for vname, V in inputs(p):
        for flags in (0, LINK):
            want, lp, _ = debatch_ref(p, V, flags)
            wrong, _, _ = debatch_ref(p, V, flags, mutate=mutate)
            tol = debatch_tol(p, V, flags)
            ok = np.isfinite(want) & np.isfinite(wrong) & np.isfinite(lp) & has_batch(p) & (tol > 0)
            with np.errstate(invalid="ignore", divide="ignore"):
                far = np.abs(wrong - want)[ok] >= 10 * tol[ok]
            assert far.sum() >= 0.5 * ok.sum(), (vname, flags, mutate, far.sum(), ok.sum())
