"""Inputs and bounds shared by tests/test_gpu_postprocess.py and tests/test_eig_standalone.py.

Shapes (K, M, N): (1, 5, 7), (6, 331, 96), (33, 257, 1068) -- Kp > K -- and (128, 4099, 1068): M = 4099 is two column chunks
of the Gram kernel (2048) plus a last one of 3.  The views of N = 1068 are 1, 2, 1025 and 40 columns.
Y = Q1 diag(s) Q2' with s = linspace(2, 1, K), rounded to float32: the spectrum is separated, so U is determined up to sign.

Bounds (derived, not tuned):
  (a) Gram      |G_ab - ref| <= n 2^-52 ||row a|| ||row b||, n the group's column count: an n-term float64 dot product with a
                factor 2 of slack; ref is numpy float64 on the float32 inputs.
  (b) stored    |got - ref64| <= 2^-23 |ref64| + 1e-10 max|ref64|: one float32 rounding of a float64 value whose own error is
                far below 1e-10; NaN and +-inf positions identical.  (whiten! stores Y twice, as the host does: two roundings
                of 2^-24 each, 2^-23 + 2^-48 in all, the last term far inside the absolute one.)

EDGE_SHAPES / EDGE_VIEWS (tests/test_gpu_postprocess_edges.py on the device, guarded on the CPU by
tests/test_postprocess_edge_cases.py) sit on the seams of csrc/pmf_postprocess.hip that SHAPES does not reach: K = 31, 32, 64,
65, 96, 97 around the template classes of k_pp_gram / k_pp_rotate and Kp = 96; N of 2049, 2176, 4100 (two and three Gram pieces
of Y, a last piece of 1 and of 4 columns) and 2047 (one column short of a piece); M and N one short of, equal to and one past
a tile of the in-place kernels k_pp_rotate (256, 128, 64 columns by K class) and k_pp_permute (64).  EDGE_VIEWS leaves columns
in no view (the -1 of pp_find_range), puts views across and exactly on piece seams, and has 3, 2, 36, 3, 65 and 1 ranges."""
from functools import lru_cache

import numpy as np

SHAPES = [(1, 5, 7), (6, 331, 96), (33, 257, 1068), (128, 4099, 1068)]
GRAM_CHUNK = 2048
VIEWS = {7: [(1, 3), (4, 7)], 96: [(1, 48), (49, 96)], 1068: [(1, 1), (2, 3), (4, 1028), (1029, 1068)]}

# (K, M, N) on the seams of pmf_postprocess.hip; what each one hits is asserted in tests/test_postprocess_edge_cases.py
EDGE_SHAPES = [(31, 255, 257), (32, 256, 2049), (64, 129, 2176), (65, 63, 4100), (96, 70, 130), (97, 64, 2047)]
EDGE_VIEWS = {
    257: [(1, 1), (2, 2), (4, 256)],                                         # columns 3 and 257 are in no view
    2049: [(2, 2040), (2045, 2049)],                                         # 1 and 2041..2044 in no view; view 2 across the seam
    2176: [(61 * i + 1, 61 * i + 60) for i in range(35)] + [(2136, 2176)],   # 36 views, a one-column gap between each pair
    4100: [(1, 2048), (2049, 4096), (4097, 4100)],                           # views end exactly on the seams
    130: [(2 * i + 1, 2 * i + 2) for i in range(65)],
    2047: [(1, 2047)],
}


@lru_cache(maxsize=None)
def _factors(K, M, N):
    rng = np.random.default_rng(1000 * K + M + N)
    Q1 = np.linalg.qr(rng.standard_normal((K, K)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((N, K)))[0]
    Y = ((Q1 * np.linspace(2.0, 1.0, K)[None, :]) @ Q2.T).astype(np.float32)
    X = (rng.standard_normal((K, M)) * (0.5 + rng.random(K))[:, None]).astype(np.float32)
    ls = (0.2 * rng.standard_normal(N)).astype(np.float32)
    mu = (0.3 * rng.standard_normal(N)).astype(np.float32)
    D = (rng.standard_normal((M, N))).astype(np.float32)
    D[rng.random((M, N)) < 0.05] = np.nan
    out = dict(X=np.asfortranarray(X), Y=np.asfortranarray(Y), logsigma=ls, mu=mu, D=np.asfortranarray(D))
    for a in out.values():
        a.setflags(write=False)
    return out


def make_factors(K, M, N):
    """dict(X K x M, Y K x N, logsigma N, mu N, D M x N), float32, read-only and shared: copy before changing."""
    return _factors(K, M, N)


def check_gram(got, P, ranges, label):
    """Bound (a) for every group.  Returns the worst ratio error / bound."""
    P64 = np.asarray(P, np.float64)
    worst = 0.0
    for g, (a, b) in enumerate(ranges):
        blk = P64[:, a - 1:b]
        ref = blk @ blk.T
        nrm = np.sqrt(np.sum(blk * blk, axis=1))
        bound = (b - a + 1) * 2.0 ** -52 * np.outer(nrm, nrm)
        err = np.abs(got[g] - ref)
        assert np.all(err <= bound), (label, g, float(np.max(err - bound)))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(bound > 0, err / bound, 0.0)
        worst = max(worst, float(np.max(r)) if r.size else 0.0)
    return worst


def stored_deviation(got, ref64):
    """Worst |got - ref64| / (2^-23 |ref64| + 1e-10 max|ref64|) over the finite entries (<= 1 holds bound (b)); asserts that
    NaN and +-inf sit at the same places."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref64)), "NaN positions differ"
    assert np.array_equal(np.isposinf(got), np.isposinf(ref64)) and np.array_equal(np.isneginf(got), np.isneginf(ref64))
    fin = np.isfinite(ref64)
    if not fin.any():
        return 0.0
    tol = 2.0 ** -23 * np.abs(ref64[fin]) + 1e-10 * np.max(np.abs(ref64[fin]))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(tol > 0, np.abs(got[fin] - ref64[fin]) / tol, np.where(got[fin] == ref64[fin], 0.0, np.inf))
    return float(np.max(r))
