"""The host side of impute, without a GPU: the numpy restatement against the fp64 oracle, the reachability of the device
tolerance by a plain float32 evaluation, the 64-bit output offsets and the Python row blocking."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from impute_ref import BATCH, CASES, FLAG_SETS, KEEP, LINK, case_problem, impute_ref, impute_tol, scale_of, worst_ratio
from problems import to_oracle

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("K,M,N", [CASES[0], CASES[4], CASES[8], CASES[9], CASES[13]])
def test_restatement_is_the_oracle_forward(K, M, N):
    p = case_problem(K, M, N)
    _, z = impute_ref(p, BATCH | LINK)
    Zo = to_oracle(p).forward()
    # the same fp64 expression up to the order of the sums: held per entry to the magnitude of its own terms
    assert np.all(np.abs(z - Zo) <= 1e-12 * scale_of(p, BATCH | LINK)), float(np.max(np.abs(z - Zo)))


@pytest.mark.parametrize("K,M,N", CASES)
def test_float32_twin_is_inside_the_tolerance(K, M, N):
    """The bounds the device is held to are reachable by a plain float32 evaluation of the same formulas."""
    p = case_problem(K, M, N)
    for flags in FLAG_SETS:
        want, z = impute_ref(p, flags)
        got, _ = impute_ref(p, flags, np.float32)
        assert got.dtype == np.float32
        r = worst_ratio(got, want, impute_tol(p, flags, z))
        assert r <= 1.0, (flags, r)


def test_keep_observed_restatement_keeps_the_data():
    p = case_problem(32, 33, 65)
    out, _ = impute_ref(p, KEEP)
    obs = np.isfinite(p["D"])
    assert np.array_equal(out[obs], p["D"][obs].astype(np.float64)) and np.isfinite(out).all()


def test_output_offsets_are_64_bit_at_the_headline_size():
    lib = ctypes.CDLL(str(ROOT / "pathmatfac.jl_amd" / "libpmf_hip.so"))
    f = lib.pmf_debug_impute_offset
    f.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    m, N = 200000, 50000
    off = ctypes.c_int64(0)
    for r, j, ld in [(0, 0, m), (m - 1, 0, m), (0, 1, m), (m - 1, N - 1, m), (17, 10737, m), (17, 10738, m),
                     (m - 1, N - 1, m + 5), (0, 21474, m), (0, 21475, m + 3)]:
        assert f(r, j, ld, ctypes.byref(off)) == 0
        assert off.value == j * ld + r, (r, j, ld, off.value)       # Python integers do not wrap
    assert (m - 1) + (N - 1) * m > 2 ** 31 and off.value > 2 ** 32
    assert f(0, 0, m, None) != 0


class StubContext:
    """Records the blocks impute() asks for; fills each with its absolute row number."""

    def __init__(self, M, N):
        self.M, self.N, self.calls = M, N, []

    @staticmethod
    def impute_flags(b, l, k):
        return (1 if b else 0) | (2 if l else 0) | (4 if k else 0)

    def impute(self, flags, row_start1, row_stop1, out, out_row):
        self.calls.append((flags, row_start1, row_stop1, out_row))
        n = row_stop1 - row_start1 + 1
        out[out_row:out_row + n] = np.arange(row_start1 - 1, row_stop1, dtype=np.float32)[:, None]


class StubModel:
    matfac = None

    def __init__(self, ctx):
        self.ctx = ctx

    def device_context(self, device=0):
        return self.ctx


@pytest.mark.parametrize("capacity,blocks", [(6, 10), (7, 10), (8, 10), (13, 10), (14, 5), (20, 5), (21, 4), (69, 2), (70, 1),
                                             (10 ** 8, 1)])
def test_row_blocking_follows_capacity(pkg, monkeypatch, capacity, blocks):
    """capacity below, equal to and above one row of N = 7 entries, and up to the whole matrix."""
    M, N = 10, 7
    monkeypatch.setattr(pkg.matfac, "marshal", lambda *a, **k: None)
    ctx = StubContext(M, N)
    out = pkg.impute(StubModel(ctx), capacity=capacity, include_batch_effects=True)
    assert out.shape == (M, N) and out.dtype == np.float32 and out.flags.f_contiguous
    assert len(ctx.calls) == blocks, ctx.calls
    assert np.array_equal(out, np.arange(M, dtype=np.float32)[:, None] * np.ones((1, N), np.float32))
    step = max(1, capacity // N)
    assert [c[1:] for c in ctx.calls] == [(r + 1, min(r + step, M), r) for r in range(0, M, step)]
    assert all(c[0] == 1 for c in ctx.calls)


def test_row_blocking_of_a_row_range(pkg, monkeypatch):
    monkeypatch.setattr(pkg.matfac, "marshal", lambda *a, **k: None)
    ctx = StubContext(10, 7)
    out = pkg.impute(StubModel(ctx), capacity=21, rows=range(2, 9), link=True, keep_observed=True)
    assert out.shape == (7, 7) and np.array_equal(out[:, 3], np.arange(2, 9, dtype=np.float32))
    assert ctx.calls == [(6, 3, 5, 0), (6, 6, 8, 3), (6, 9, 9, 6)]
    for bad in (range(0, 11), range(5, 5), (3, 2), range(0, 10, 2)):
        with pytest.raises(ValueError):
            pkg.impute(StubModel(StubContext(10, 7)), rows=bad)
    assert pkg.impute.__module__.endswith("impute") and callable(pkg.impute_entries)
