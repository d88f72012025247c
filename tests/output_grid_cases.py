"""The grid of pmf_impute_kernel restated, and the two problems that take it past one grid of workgroups.

pmf_impute_kernel (impute, the SimEpi epilogue of simulate_data, the FILL_MISSING half of remove_batch_effect) is a persistent
grid over units.  `impute_grid` restates impute_args (csrc/pmf_outputs.hip), not asked of the library:

    NW = 8 waves up to K = 64, 4 above; a row panel is BM = 32 NW rows, numbered from row 0 of the matrix
    n_ct = ceil(N / 32) column tiles (the tile-major stores of simulate_data_resident: those of N padded to a multiple of 64)
    n_seg = ceil(n_ct / 2) column segments of two tiles (the last one holds one tile when n_ct is odd)
    rp0 = row0 // BM, n_rp = (row1 - 1) // BM + 1 - rp0          the panels that meet rows [row0, row1)
    R = max(1, min(n_rp, ceil(4 cu / n_seg)))                    row ranges per segment
    units = n_seg R, unit u = (segment u // R, range rr = u % R) sweeps panels rp0 + rr n_rp // R .. rp0 + (rr + 1) n_rp // R
    grid = min(units, cu) workgroups; workgroup b walks u = b, b + grid, ...

Case A (K = 65: four waves, 128-row panels) has at least four units per workgroup, R < n_rp with an uneven split (units of one
and of two panels) and an odd tile count; case B (K = 33: eight waves, 256-row panels) has R = n_rp and a ragged tail in which
only some workgroups take a second unit.  Both are simulate_ref.sim_case problems (mixed noise with Poisson re-declared normal,
two batch views, rows in no batch), so one model serves impute, simulate_data and remove_batch_effect.  Plain numpy."""
import numpy as np

import simulate_ref as sr
from impute_ref import impute_ref

CU_DEFAULT = 256           # the CU count of the CPU-side geometry checks; the GPU tests take the device's
SEED = 3                   # the seed of every draw of the two cases (that of test_bernoulli_near_ties_are_rare)
EDGE_SEED = 0x9E3779B97F4A7C15        # both key words set, the high one with its top bit
EDGE_ROW0 = 2 ** 32 - 35              # global row of local row 0: 70 rows straddle the 2^32 boundary of the counter's first word
EDGE_SHAPE = (20, 70, 40)


def impute_grid(K, M, N, cu, row0=0, row1=None, tile_major=False):
    """impute_args for rows [row0, row1) (0-based): dict(NW, BM, n_ct, n_seg, rp0, n_rp, R, units, grid, panels), panels[rr]
    = the (lo, hi) panel range, relative to rp0, of row range rr (every segment has the same R ranges)."""
    row1 = M if row1 is None else row1
    assert 0 <= row0 < row1 <= M
    NW = 8 if K <= 64 else 4
    BM = 32 * NW
    n_ct = (64 * -(-N // 64)) // 32 if tile_major else -(-N // 32)
    n_seg = -(-n_ct // 2)
    rp0 = row0 // BM
    n_rp = (row1 - 1) // BM + 1 - rp0
    R = max(1, min(n_rp, -(-4 * cu // n_seg)))
    units = n_seg * R
    panels = [(rr * n_rp // R, (rr + 1) * n_rp // R) for rr in range(R)]
    return dict(NW=NW, BM=BM, n_ct=n_ct, n_seg=n_seg, rp0=rp0, n_rp=n_rp, R=R, units=units, grid=min(units, cu), panels=panels)


def _off_tile_edges(N):
    """N, or N + 1 when a boundary of std_views (N // 3, 2 N // 3) is a multiple of 32 (std_views asserts they are not)."""
    return N if (N // 3) % 32 and (2 * N // 3) % 32 else N + 1


def shape_a(cu=CU_DEFAULT):
    """(K, M, N) of case A: one segment more than gives R = 6 of 8 panels, an odd tile count, 6 columns in the last tile."""
    n_seg = -(-4 * cu // 6) + 1
    n_ct = 2 * n_seg - 1
    return 65, 993, _off_tile_edges(32 * (n_ct - 1) + 6)


def shape_b(cu=CU_DEFAULT):
    """(K, M, N) of case B: 8 (cu / 8 + 2) = cu + 16 units, an odd tile count, 8 columns in the last tile."""
    n_seg = cu // 8 + 2
    n_ct = 2 * n_seg - 1
    return 33, 1800, _off_tile_edges(32 * (n_ct - 1) + 8)


def regime_a(K, M, N, cu, row0=0, row1=None):
    """Asserts what case A exists for, at this CU count; returns the grid."""
    g = impute_grid(K, M, N, cu, row0, row1)
    assert g["NW"] == 4 and g["units"] >= 4 * g["grid"] and g["R"] < g["n_rp"] and g["n_ct"] % 2 == 1, g
    spans = {hi - lo for lo, hi in g["panels"]}
    assert 2 in spans and 1 in spans and min(spans) >= 1, g                  # an uneven split: units of one and of two panels
    return g


def regime_b(K, M, N, cu):
    g = impute_grid(K, M, N, cu)
    assert g["NW"] == 8 and g["grid"] < g["units"] < 2 * g["grid"] and g["R"] == g["n_rp"] and g["n_ct"] % 2 == 1, g
    return g


def problem_a(cu=CU_DEFAULT):
    return sr.sim_case(*shape_a(cu))


def problem_b(cu=CU_DEFAULT):
    return sr.sim_case(*shape_b(cu))


def draws_at(seed, rows, cols):
    """simulate_ref.draws for the listed GLOBAL rows and the listed columns only (the Bernoulli columns of a wide case)."""
    u1, u2, u3, u4 = sr.uniforms(sr.words(seed, rows, cols))
    return dict(n=sr.normal64(u1, u2), u3=u3, u4=u4)


def bernoulli_near(p, z, tol, u4, cols):
    """(near ties, the f64 decisions) on the Bernoulli columns `cols`: z, tol the full matrices of impute under BATCH, u4 of
    those columns.  A near tie is an entry whose draw lies within impute's bound of the fp64 probability."""
    p64 = sr.sigmoid64(z[:, cols])
    return np.abs(u4 - p64) <= tol[:, cols], u4 < p64


def stale(p, what, shift=64):
    """The problem a unit would compute from had it kept the previous segment's staging: `what` ("mu": the column parameters
    Cmu, "Y": the factor tiles Ys) rolled by one segment's 64 columns."""
    q = dict(p)
    q[what] = np.asfortranarray(np.roll(p[what], shift, axis=-1))
    return q


def broken_share(p, q, flags):
    """The share of entries at which the fp64 values of problem q are outside impute_tol of problem p's."""
    want, z = impute_ref(p, flags)
    other, _ = impute_ref(q, flags)
    return float((np.abs(other - want) > sr.impute_tol(p, flags, z)).mean())
