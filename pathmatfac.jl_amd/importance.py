"""Factor importance (not in the reference; DESIGN.md section 2, Deviation 6): what every factor explains of every column's
loss and of every view's, from one pass over the resident data (include/pmf_hip_importance.h)."""
from collections import namedtuple

import numpy as np

from .impute import _context
from .util import unique

FactorImportance = namedtuple("FactorImportance", ["delta", "full", "null", "n_obs"])


def factor_importance(model, reduce=True, device=0):
    """Per column j, at the model's current parameters and over its observed entries, with l the entry loss of the column's
    noise model including the column weight:

        full[j]     = sum_i l(a_ij)                 a the model's output, batch effects included
        null[j]     = sum_i l(mu_j + theta_bj)      every factor left out
        delta[k, j] = sum_i (l(a_ij without term k of the inner product) - l(a_ij))
        n_obs[j]    = the number of those entries (0 for a column of weight 0, which adds nothing anywhere)

    Returns FactorImportance(delta (K, N) float64, full (N,), null (N,), n_obs (N,) int64).  delta[k, j] / null[j] is the
    variance explained by factor k in a normal column, the explained deviance otherwise.  Factors are not orthogonal, so
    sum_k delta[k, j] is in general NOT null[j] - full[j].  The factors are not refit.

    The model's live context is reused and resident data are not uploaded again.  On a row-sharded model the device sums the
    local rows; reduce=True adds the ranks in ONE model.allreduce (a collective: every rank calls), reduce=False returns the
    local sums."""
    ctx = _context(model, device)
    delta, full, null, n_obs = ctx.factor_importance()
    if reduce and model.sharded:
        K, N = delta.shape
        buf = np.concatenate([delta.ravel(), full, null, n_obs.astype(np.float64)])   # (counts are exact below 2^53)
        model.allreduce(buf)
        delta = buf[:K * N].reshape(K, N).copy()
        full, null = buf[K * N:K * N + N].copy(), buf[K * N + N:K * N + 2 * N].copy()
        n_obs = np.rint(buf[K * N + 2 * N:]).astype(np.int64)
    return FactorImportance(delta, full, null, n_obs)


def explained_deviance(model, imp=None):
    """dict(views, factor (K, V), total (V,)) over the views of unique(model.feature_views), in that order:

        factor[k, v] = sum_{j in v} delta[k, j] / sum_{j in v} null[j]        total[v] = 1 - sum_{j in v} full[j] / sum_{j in v} null[j]

    imp: a FactorImportance of the WHOLE matrix (default: factor_importance(model)).  A view whose null sum is 0 -- no
    observed entry, or zero weights -- gives NaN."""
    if imp is None:
        imp = factor_importance(model)
    delta, full, null = (np.asarray(x, np.float64) for x in (imp[0], imp[1], imp[2]))
    views = unique(model.feature_views)
    fv = np.asarray(model.feature_views, dtype=object)
    factor, total = np.full((delta.shape[0], len(views)), np.nan), np.full(len(views), np.nan)
    for v, name in enumerate(views):
        cols = np.flatnonzero(np.array([x == name for x in fv], dtype=bool))
        s_null = null[cols].sum()
        if s_null != 0.0:
            factor[:, v] = delta[:, cols].sum(1) / s_null
            total[v] = 1.0 - full[cols].sum() / s_null
    return dict(views=list(views), factor=factor, total=total)
