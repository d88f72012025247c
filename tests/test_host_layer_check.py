"""The segment-scaled check of the layer gradients (problems.layer_check) on the CPU oracle alone.

(a) The f32 build of the oracle -- sequential f32 sums over every row, the same roundings as a correct kernel -- passes
    with at least 10x margin on the problem shapes of tests/test_gpu_layer_edges.py (a representative subset).
(b) The check fails when the problem is mutated the way a flush or segment bug would corrupt a sum: one observed row
    dropped from one (batch, column) segment, one row moved to the neighbouring batch, or batch nb-1 merged into the
    identity slot.  The dropped and moved rows are drawn, seeded, from rows whose gradient is not negligible: |g_ij| more
    than twice the tolerance tau * scale of its (batch, column) segment.  Such rows must be most rows, or the check could
    not see a dropped row at all.
(c) A problem built to cancel (M = 31, N = 1: every segment's residuals sum to ~0, like the outliers of
    scripts/fuzz_parity.py) passes with the f32 oracle, where rel_err does not.
"""
import copy

import numpy as np
import pytest

from problems import LAYER_TAU, layer_check, layer_scales, make_problem, rel_err, to_oracle
from test_gpu_layer_edges import (layer_grid, layer_problem, panel_shapes, row_layout, rows, slot_problem, std_views,
                                  expected_layer_path)

N_CU = 256   # MI355X


def _k_edge(K, s):
    M, N = panel_shapes(K)[s]
    seed = 7 * K + M + N
    return layer_problem(M, N, K, seed, std_views(M, N, seed))


def _layout(name, K):
    P = 32 * expected_layer_path(K, 15)[2]
    M, N = 3 * P + 17, 65
    rng = np.random.default_rng(K)
    bor, nb = row_layout(name, M, P, rng)
    return layer_problem(M, N, K, 23 + K, [(1, 30, bor, nb), (41, N, rows(M, 6, "scrambled", rng), 6)])


def _grid(K=8):
    M, N = 300, 64 * (N_CU + 17) - 5
    n_seg, n_rp, R, grid = layer_grid(M, N, K, N_CU)
    assert n_seg > N_CU and R > 1
    rng = np.random.default_rng(M + N)
    bor = np.searchsorted([100, 200, 290], np.arange(M), side="right").astype(np.int32)
    return layer_problem(M, N, K, 29, [(1, N // 3, bor, 4), (2 * N // 3 + 1, N, rows(M, 15, "scrambled", rng), 15)],
                         nan_frac=0.02)


SHAPES = {f"k{K}-shape{s}": (lambda K=K, s=s: _k_edge(K, s)) for K in (1, 32, 33, 64, 65, 96, 97, 128) for s in range(5)}
SHAPES.update({f"slots-k{K}-nb{nb}": (lambda K=K, nb=nb: slot_problem(K, nb, seed=K + nb))
               for K in (32, 96, 128) for nb in (15, 64, 127)})
SHAPES.update({f"{name}-k{K}": (lambda name=name, K=K: _layout(name, K))
               for name in ("aligned16", "alternating", "span_panels", "one_row_and_empty", "minus_one") for K in (16, 96)})
SHAPES["units_per_workgroup"] = _grid


@pytest.mark.parametrize("name", list(SHAPES))
def test_f32_oracle_passes_with_margin(name):
    p = SHAPES[name]()
    _, g64 = to_oracle(p).loss_and_grads(update_col_layers=True)
    _, g32 = to_oracle(p, 32).loss_and_grads(update_col_layers=True)
    worst = layer_check(p, g32, g64)
    assert max(worst.values()) <= 0.1, worst


def _segment_entries(p, s, v):
    """(row, column of the view) of view v's observed entries, and which of them are not negligible."""
    bv = p["batch_views"][v]
    sl = slice(bv["start1"] - 1, bv["stop1"])
    bor = np.asarray(bv["batch_of_row"])
    i, jl = np.nonzero(np.isfinite(p["D"][:, sl]) & (bor >= 0)[:, None])
    g = np.abs(s["g"][:, sl][i, jl])
    tol = LAYER_TAU * s["theta"][v][bor[i], jl]
    return i, jl, g > 2 * tol


def _fails(p, q):
    _, want = to_oracle(p).loss_and_grads(update_col_layers=True)
    _, got = to_oracle(q).loss_and_grads(update_col_layers=True)
    worst = layer_check(p, got, want)
    return max(worst.values()) > 1.0, worst


MUTATED = ["k33-shape3", "k96-shape2", "k128-shape4", "slots-k96-nb127", "minus_one-k16", "alternating-k96"]


@pytest.mark.parametrize("name", MUTATED)
def test_a_dropped_row_fails(name):
    p = SHAPES[name]()
    s = layer_scales(p)
    rng = np.random.default_rng(1)
    for v in range(len(p["batch_views"])):
        i, jl, big = _segment_entries(p, s, v)
        assert big.mean() >= 0.8, big.mean()
        for e in rng.choice(np.flatnonzero(big), size=3, replace=False):
            q = copy.deepcopy(p)
            q["D"][i[e], p["batch_views"][v]["start1"] - 1 + jl[e]] = np.nan
            bad, worst = _fails(p, q)
            assert bad, (v, i[e], jl[e], worst)


@pytest.mark.parametrize("name", MUTATED)
def test_a_row_in_the_neighbouring_batch_fails(name):
    p = SHAPES[name]()
    s = layer_scales(p)
    rng = np.random.default_rng(2)
    for v in range(len(p["batch_views"])):
        bv = p["batch_views"][v]
        nb = bv["logdelta"].shape[0]
        if nb < 2:
            continue
        i, jl, big = _segment_entries(p, s, v)
        for r in rng.choice(np.unique(i[big]), size=3, replace=False):
            q = copy.deepcopy(p)
            b = q["batch_views"][v]["batch_of_row"][r]
            q["batch_views"][v]["batch_of_row"][r] = b + 1 if b + 1 < nb else b - 1
            bad, worst = _fails(p, q)
            assert bad, (v, r, worst)


@pytest.mark.parametrize("name", MUTATED)
def test_the_last_batch_in_the_identity_slot_fails(name):
    p = SHAPES[name]()
    for v in range(len(p["batch_views"])):
        q = copy.deepcopy(p)
        bor = q["batch_views"][v]["batch_of_row"]
        bor[bor == q["batch_views"][v]["logdelta"].shape[0] - 1] = -1
        bad, worst = _fails(p, q)
        assert bad, (v, worst)


def test_cancelling_sums_pass_with_the_f32_oracle():
    """M = 31, N = 1, three batches: D = z + e with e summing to zero in every batch, so grad mu and every grad theta
    cancel to rounding noise.  rel_err divides by that noise; the segment check does not."""
    M, N, K = 31, 1, 4
    p = make_problem(M=M, N=N, K=K, seed=5, col_params=True, weights=True)
    bor = (np.arange(M) % 3).astype(np.int32)
    rng = np.random.default_rng(6)
    p["batch_views"] = [dict(start1=1, stop1=1, batch_of_row=bor,
                             logdelta=(0.25 * rng.standard_normal((3, 1))).astype(np.float32),
                             theta=(0.25 * rng.standard_normal((3, 1))).astype(np.float32))]
    z = to_oracle(p).forward()[:, 0]
    e = rng.standard_normal(M)
    for b in range(3):
        e[bor == b] -= e[bor == b].mean()
    p["D"] = np.asfortranarray((z + 0.3 * e)[:, None].astype(np.float32))
    _, g64 = to_oracle(p).loss_and_grads(update_col_layers=True)
    _, g32 = to_oracle(p, 32).loss_and_grads(update_col_layers=True)
    s = layer_scales(p)
    assert abs(g64["mu"][0]) < 1e-5 * s["mu"][0], "the problem does not cancel"
    assert rel_err(g32["mu"], g64["mu"]) > 2e-4          # (GRAD_TOL of the GPU tests: rel_err misfires here)
    worst = layer_check(p, g32, g64)
    assert max(worst.values()) <= 0.1, worst
