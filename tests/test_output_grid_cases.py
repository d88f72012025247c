"""Host-side checks of tests/output_grid_cases.py: the two problems that take pmf_impute_kernel past one grid of workgroups
are in the regime they exist for, the conditions their device checks rest on hold from the fp64 reference alone, and the numpy
twin of the Philox stream is right where the counter's and the key's second words come in.  No GPU."""
import numpy as np
import pytest

import output_grid_cases as og
import simulate_ref as sr
from impute_ref import BATCH, FLAG_SETS, impute_ref, impute_tol


# ---- the geometry ------------------------------------------------------------------------------------------------------
def test_case_a_geometry():
    K, M, N = og.shape_a()
    assert (K, M, N) == (65, 993, 10950)
    g = og.regime_a(K, M, N, og.CU_DEFAULT)
    assert (g["n_ct"], g["n_seg"], g["n_rp"], g["R"], g["units"], g["grid"]) == (343, 172, 8, 6, 1032, 256)
    assert g["panels"] == [(0, 1), (1, 2), (2, 4), (4, 5), (5, 6), (6, 8)]
    # rows 129..993: seven panels from panel 1 over six ranges, uneven again
    s = og.regime_a(K, M, N, og.CU_DEFAULT, 128, 993)
    assert (s["rp0"], s["n_rp"], s["R"]) == (1, 7, 6) and s["panels"] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 7)]
    # the resident store writes the all-pad tile of the odd tile count: the last segment has two tiles there
    assert og.impute_grid(K, M, N, og.CU_DEFAULT, tile_major=True)["n_ct"] == 344
    # chunks of 300 rows: other panel counts, another R, still several units per workgroup
    for r0 in range(0, M, 300):
        c = og.impute_grid(K, M, N, og.CU_DEFAULT, r0, min(r0 + 300, M))
        assert c["R"] == c["n_rp"] in (1, 3, 4) and c["rp0"] == r0 // 128
        assert c["units"] > c["grid"] or c["n_rp"] == 1


def test_case_b_geometry():
    K, M, N = og.shape_b()
    assert (K, M, N) == (33, 1800, 2120)
    g = og.regime_b(K, M, N, og.CU_DEFAULT)
    assert (g["n_ct"], g["n_seg"], g["n_rp"], g["R"], g["units"], g["grid"]) == (67, 34, 8, 8, 272, 256)
    assert og.impute_grid(K, M, N, og.CU_DEFAULT, tile_major=True)["n_ct"] == 68
    s = og.impute_grid(K, M, N, og.CU_DEFAULT, 256, 1800)                      # rows 257..1800
    assert (s["rp0"], s["n_rp"], s["R"], s["units"]) == (1, 7, 7, 238)


@pytest.mark.parametrize("cu", [64, 104, 120, 228, 256, 304])
def test_the_regimes_hold_at_other_cu_counts(cu):
    K, M, N = og.shape_a(cu)
    assert (N // 3) % 32 and (2 * N // 3) % 32
    og.regime_a(K, M, N, cu)
    og.regime_a(K, M, N, cu, 128, 993)
    K, M, N = og.shape_b(cu)
    assert (N // 3) % 32 and (2 * N // 3) % 32
    og.regime_b(K, M, N, cu)


def test_impute_grid_on_the_shapes_the_suite_had():
    """Every shape the other files run through the kernel is one unit per workgroup and one panel per unit."""
    for K, M, N in sr.CASES + [(128, 700, 300)]:
        g = og.impute_grid(K, M, N, og.CU_DEFAULT)
        assert g["units"] == g["grid"] <= 30 and g["R"] == g["n_rp"], (K, M, N, g)


# ---- the conditions of the device checks ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["A", "B"])
def case(request):
    p = og.problem_a() if request.param == "A" else og.problem_b()
    want, z = impute_ref(p, BATCH)
    return request.param, p, want, z, impute_tol(p, BATCH, z)


def test_bernoulli_near_ties_are_rare(case):
    """The cap of test_simulate_cases.test_bernoulli_near_ties_are_rare on the two cases: 1.6e-5 (35 entries of 2190 columns)
    at A, 7.9e-6 at B."""
    name, p, _, z, tol = case
    cols = np.flatnonzero(sr.kinds_of(p) == 1)
    assert cols.size >= 400
    u4 = og.draws_at(og.SEED, np.arange(p["M"]), cols)["u4"]
    near, _ = og.bernoulli_near(p, z, tol, u4, cols)
    print(f"{name}: near ties {near.mean():.2e} ({near.sum()} of {near.size})")
    assert near.mean() <= 0.01


@pytest.mark.parametrize("what", ["mu", "Y"])
def test_stale_staging_would_break_the_bound(case, what):
    """A unit that computed with the previous segment's column parameters (mu) or factor tiles (Y) gives the fp64 values of the
    problem with that array rolled by 64 columns: outside impute_tol on at least 99 % of the entries, under every flag set the
    device tests run (measured: at least 99.995 % everywhere)."""
    name, p, want, z, tol = case
    q = og.stale(p, what)
    share = float((np.abs(impute_ref(q, BATCH)[0] - want) > tol).mean())
    shares = {BATCH: share}
    if name == "B":
        shares.update({f: og.broken_share(p, q, f) for f in FLAG_SETS if f != BATCH})
    print(f"{name}, stale {what}: outside the bound at {({f: round(s, 7) for f, s in shares.items()})}")
    assert min(shares.values()) >= 0.99


# ---- the twin where the second counter word and the second key word come in ------------------------------------------------
def test_twin_at_the_counter_and_key_edges():
    rows = np.arange(70, dtype=np.int64) + og.EDGE_ROW0
    assert rows[34] == 2 ** 32 - 1 and rows[35] == 2 ** 32
    cols = np.arange(og.EDGE_SHAPE[2])
    w = sr.words(og.EDGE_SEED, rows, cols)
    k = (og.EDGE_SEED & 0xFFFFFFFF, og.EDGE_SEED >> 32)
    assert k == (0x7F4A7C15, 0x9E3779B9)
    for a, i in enumerate(rows):
        for j in (0, 1, 39):
            one = sr.philox4x32((int(i) & 0xFFFFFFFF, int(i) >> 32, j, 0), k)
            assert [int(x[a, j]) for x in w] == [int(x) for x in one], (a, j)
    assert int(rows[35]) >> 32 == 1 and int(rows[34]) >> 32 == 0
    mask = sr.missing_mask(dict(u3=sr.uniforms(w)[2]), 0.3)
    assert 0.2 < mask.mean() < 0.4
    # rows reduced mod 2^32: the same mask below 2^32, another one in every row at or past it
    low = sr.missing_mask(dict(u3=sr.uniforms(sr.words(og.EDGE_SEED, rows % 2 ** 32, cols))[2]), 0.3)
    differs = (mask != low).any(axis=1)
    assert np.array_equal(np.flatnonzero(differs), np.arange(35, 70))
    # the key's low word alone: another mask in every row
    lowkey = sr.missing_mask(dict(u3=sr.uniforms(sr.words(og.EDGE_SEED & 0xFFFFFFFF, rows, cols))[2]), 0.3)
    assert (mask != lowkey).any(axis=1).all()
    # draws() at a row offset is words() at the global rows
    d = sr.draws(og.EDGE_SEED, 70, cols.size, row_offset=og.EDGE_ROW0)
    assert np.array_equal(d["u3"], sr.uniforms(w)[2])
