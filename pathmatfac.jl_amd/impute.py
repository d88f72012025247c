"""impute (src/impute.jl): the fitted model's predictions, computed on the device."""
import numpy as np

from . import matfac as MF


def row_blocks(n_rows, N, capacity):
    """Blocks of `capacity // N` rows (at least one), the reference's `capacity` idiom: [(first, count), ...]."""
    step = max(1, int(capacity) // max(int(N), 1))
    return [(r0, min(step, n_rows - r0)) for r0 in range(0, n_rows, step)]


def row_range(name, rows, M):
    """`rows` of `name` (None: all M; a contiguous range; or a (start, stop) pair; 0-based, stop exclusive) -> (lo, hi)."""
    if rows is None:
        lo, hi = 0, M
    elif isinstance(rows, range):
        if rows.step != 1:
            raise ValueError(f"{name}: rows must be a contiguous range")
        lo, hi = rows.start, rows.stop
    else:
        lo, hi = int(rows[0]), int(rows[1])
    if lo < 0 or hi > M or lo >= hi:
        raise ValueError(f"{name}: rows {lo}:{hi} are empty or outside 0:{M}")
    return lo, hi


def _context(model, device):
    ctx = model.device_context(device)
    MF.marshal(model.matfac, ctx, with_xreg=False, with_yreg=False)
    return ctx


def impute(model, include_batch_effects=False, link=False, keep_observed=False, capacity=10 ** 8, rows=None, device=0):
    """impute(model; include_batch_effects=false) (impute.jl:37-56): Z = X'Y through the column scale and shift (and the
    batch scale and shift when asked for), then the inverse link of every column's noise model (:3-13, 27-35).

    link=True returns Z itself; keep_observed=True returns the observed entries of model.data and fills only the missing
    ones.  rows: a range or (start, stop) pair of 0-based rows, stop exclusive (default: all M); the result is
    len(rows) x N float32.  The device computes blocks of capacity // N rows, so a caller bounds host memory with `rows`.
    On a row-sharded model this is per rank: the rows are the local ones and nothing is exchanged."""
    ctx = _context(model, device)
    N = ctx.N
    lo, hi = row_range("impute", rows, ctx.M)
    flags = ctx.impute_flags(include_batch_effects, link, keep_observed)
    out = np.empty((hi - lo, N), np.float32, order="F")
    for r0, nr in row_blocks(hi - lo, N, capacity):
        # each block is written in place: rows r0 .. r0 + nr - 1 of every column, leading dimension = all rows of `out`
        ctx.impute(flags, lo + r0 + 1, lo + r0 + nr, out=out, out_row=r0)
    return out


def impute_entries(model, rows, cols, include_batch_effects=False, link=False, device=0):
    """The predictions at the listed entries (0-based numpy indices; duplicates are legal): held-out scoring without an
    M x N temporary.  On a row-sharded model `rows` index the local rows of the calling rank."""
    ctx = _context(model, device)
    r = np.asarray(rows, dtype=np.int64).ravel() + 1
    c = np.asarray(cols, dtype=np.int64).ravel() + 1
    return ctx.impute_entries(r, c, ctx.impute_flags(include_batch_effects, link, False))
