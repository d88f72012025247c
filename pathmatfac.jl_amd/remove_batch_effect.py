"""remove_batch_effect (src/remove_batch_effect.jl): the data with the fitted batch effects taken out, on the device."""
import numpy as np

from .impute import _context, row_blocks, row_range


def remove_batch_effect(model, Z=None, link=False, fill_missing=False, capacity=10 ** 8, rows=None, device=0):
    """remove_batch_effect(model, Z) (remove_batch_effect.jl:3-16) against the layer order this package implements: every
    observed value goes to link space, loses the batch shift and scale of its (row's batch, column) --
    l' = ((l - theta) - mu) / delta + mu -- and comes back through the inverse link.  Entries of rows in no batch and of
    columns in no batch view, and squared-hinge class labels, are returned as given.

    Z: the values of exactly the requested rows (len(rows) x N); None takes model.data as resident on the device.
    link=True: Z and the result are in link space.  fill_missing=True: missing entries take the batch-free prediction
    (impute(model)) instead of NaN.  rows, capacity: as in `impute`; the result is len(rows) x N float32.
    On a row-sharded model this is per rank: the rows are the local ones and nothing is exchanged."""
    ctx = _context(model, device)
    N = ctx.N
    lo, hi = row_range("remove_batch_effect", rows, ctx.M)
    if Z is not None:
        Z = np.asarray(Z)
        if Z.shape != (hi - lo, N):
            raise ValueError(f"remove_batch_effect: Z must hold the requested rows, {hi - lo} x {N}")
    flags = ctx.debatch_flags(link, fill_missing)
    out = np.empty((hi - lo, N), np.float32, order="F")
    for r0, nr in row_blocks(hi - lo, N, capacity):
        ctx.remove_batch_effect(flags, lo + r0 + 1, lo + r0 + nr, Z=None if Z is None else Z[r0:r0 + nr], out=out, out_row=r0)
    return out


def remove_batch_effect_entries(model, rows, cols, values=None, link=False, device=0):
    """The corrected values at the listed entries (0-based numpy indices; duplicates are legal) of `values`, or of
    model.data as resident on the device when values is None.  On a row-sharded model `rows` index the local rows."""
    ctx = _context(model, device)
    r = np.asarray(rows, dtype=np.int64).ravel() + 1
    c = np.asarray(cols, dtype=np.int64).ravel() + 1
    return ctx.remove_batch_effect_entries(r, c, values, ctx.debatch_flags(link, False))
