"""What pmf_remove_batch_effect must compute, restated in numpy, and how closely.

Per entry with input v, b the batch of row i in column j's view, delta = e^logdelta[b, j], theta = theta[b, j]:

    column in no batch view, or row in no batch (batch_of_row = -1)   -> v, bit for bit
    kind 3 (squared hinge, class labels; without LINK)                -> v, bit for bit
    v not finite                                                      -> NaN
    else   l = link(v) ;  l' = ((l - theta) - mu_j) / delta + mu_j ;  out = invlink(l')
           normal: identity ; bernoulli: log v - log(1 - v) in, 1 / (1 + e^-l') out ; poisson: log v in, e^l' out
           LINK: the identity link for every column, kind 3 included

`debatch_ref(p, V, flags)` evaluates this in float64 and `debatch_ref(p, V, flags, np.float32)` is its float32 twin (every
operation, np.exp and np.log included, in float32, in the kernel's order; the fused multiply-add is a float64 product and sum
rounded once to float32).  FILL_MISSING is not restated: it is pmf_impute's
values at the missing entries, which tests/impute_ref.py restates.

`debatch_tol` is the per-entry bound on |device - float64|, derived from the arithmetic, not from any output:

    link space  the kernel evaluates l' = fma((l - theta) - mu, r, mu) with r = rcp(delta).  To first order its roundings are
                  (l - theta)            2^-24 (|l| + |theta|)                   later multiplied by r
                  (. - mu)               2^-24 (|l| + |theta| + |mu|)            later multiplied by r
                  delta = expf(logdelta) 1 ulp (the documented bound of the device's expf) = 2 x 2^-24 relative, on the quotient
                  r = v_rcp_f32(delta)   1 ulp (the instruction's documented accuracy) = 2 x 2^-24 relative, on the quotient:
                                         this is the kernel's division
                  fma(., r, mu)          one rounding of the result: 2^-24 (|quotient| + |mu|)
                every unit at most 2^-24 s with s = (|l| + |theta| + |mu|) / delta + |mu|: seven units, and an eighth for the
                products of these errors:  e' = e_l / delta + 8 x 2^-24 s, where e_l is the error of the link of the input:
                  normal, LINK  e_l = 0
                  poisson       e_l = 2^-22 |l|: v_log_f32 is 1 ulp of log2 v (2^-23 relative), the product with ln 2 adds one
                                rounding and the constant's own, 2^-24 + 2^-25
                  bernoulli     e_l = 2^-22 (|log v| + |log(1 - v)|) + 2^-24 (1 + |l|): the two logarithms, the rounding of
                                1 - v (2^-24 relative in the argument is 2^-24 absolute in its logarithm), the subtraction
    normal      e'
    poisson     e^l' (expm1(e') + (|l'| + 4) 2^-23)                 as impute_ref.impute_tol
    bernoulli   (e' + (|l'| + 4) 2^-23) / 4 + 2^-22                 as impute_ref.impute_tol
    l' infinite (0 and 1 of a Bernoulli column, 0 of a Poisson column): the value is exact, the bound 0.
"""
import numpy as np

from hinge_ref import kinds_of
from impute_ref import _batch_terms

LINK, FILL = 1, 2
N_ROUND = 8
MUTATIONS = ("mu_neighbour", "batch_neighbour", "old_order")


def has_batch(p):
    """M x N bool: the column is in a batch view and the row in one of its batches."""
    has = np.zeros((p["M"], p["N"]), bool)
    for v in p["batch_views"]:
        has[:, v["start1"] - 1:v["stop1"]] = (np.asarray(v["batch_of_row"]) >= 0)[:, None]
    return has


def link_kinds(p, flags):
    return np.zeros(p["N"], np.int8) if flags & LINK else kinds_of(p)


def _link(V, kind, dtype):
    l = np.array(V, dtype)
    one = dtype(1)
    b, q = kind == 1, kind == 2
    with np.errstate(divide="ignore", invalid="ignore"):
        if dtype == np.float64:
            l[:, b] = np.log(l[:, b]) - np.log1p(-l[:, b])
        else:
            l[:, b] = np.log(l[:, b]) - np.log(one - l[:, b])
        l[:, q] = np.log(l[:, q])
    return l


def _invlink(lp, kind):
    out = lp.copy()
    one = lp.dtype.type(1)
    b, q = kind == 1, kind == 2
    with np.errstate(over="ignore", invalid="ignore"):
        z = lp[:, b]
        e = np.exp(-np.abs(z))
        r = one / (one + e)
        out[:, b] = np.where(z >= 0, r, e * r)
        out[:, q] = np.exp(lp[:, q])
    return out


def _mutated(p, mutate):
    if mutate != "batch_neighbour":
        return p
    views = [dict(v, batch_of_row=np.where(np.asarray(v["batch_of_row"]) >= 0,
                                           (np.asarray(v["batch_of_row"]) + 1) % np.asarray(v["logdelta"]).shape[0], -1))
             for v in p["batch_views"]]
    return dict(p, batch_views=views)


def debatch_ref(p, V, flags, dtype=np.float64, mutate=None):
    """(values, l', l): the corrected matrix of input V (M x N), and the link-space values after and before the
    correction (both V outside the corrected entries).  mutate: one of MUTATIONS, a wrong rule for the sensitivity check."""
    assert mutate is None or mutate in MUTATIONS
    dtype = np.dtype(dtype).type
    V = np.asarray(V)
    kind = link_kinds(p, flags)
    has = has_batch(p)
    dl, th = _batch_terms(_mutated(p, mutate), dtype)
    mu = np.asarray(p["mu"], dtype)
    if mutate == "mu_neighbour":
        mu = np.roll(mu, -1)
    l = _link(V, kind, dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if mutate == "old_order":
            lp = (l - th) / dl
        elif dtype == np.float32:       # the kernel's form: the reciprocal, then one fused multiply-add
            r = (dtype(1) / dl).astype(np.float64)
            lp = (((l - th) - mu[None, :]).astype(np.float64) * r + mu[None, :].astype(np.float64)).astype(np.float32)
        else:
            lp = ((l - th) - mu[None, :]) / dl + mu[None, :]
        o = _invlink(lp, kind)
    assert lp.dtype == dtype and o.dtype == dtype
    corrected = has & (kind != 3)[None, :]
    out = np.where(corrected, np.where(np.isfinite(V), o, dtype(np.nan)), V.astype(dtype))
    return out, np.where(corrected, lp, V.astype(dtype)), np.where(corrected, l, V.astype(dtype))


def debatch_tol(p, V, flags, e_in=None):
    """Per-entry bound on |device - float64| (0 on the entries returned as given).  e_in: a bound on the error the INPUT
    already carries in link space (LINK only), propagated through the division by delta."""
    V64 = np.asarray(V, np.float64)
    kind = link_kinds(p, flags)
    corrected = has_batch(p) & (kind != 3)[None, :]
    _, lp, l = debatch_ref(p, V64, flags)
    dl, th = _batch_terms(p, np.float64)
    amu = np.abs(np.asarray(p["mu"], np.float64))[None, :]
    b, q = kind == 1, kind == 2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        e_l = np.zeros_like(V64)
        e_l[:, q] = 2.0 ** -22 * np.abs(l[:, q])
        vb = V64[:, b]
        e_l[:, b] = 2.0 ** -22 * (np.abs(np.log(vb)) + np.abs(np.log1p(-vb))) + 2.0 ** -24 * (1 + np.abs(l[:, b]))
        if e_in is not None:
            e_l = e_l + e_in
        s = (np.abs(l) + np.abs(th) + amu) / dl + amu
        e = e_l / dl + N_ROUND * 2.0 ** -24 * s
        tol = e.copy()
        arg = (np.abs(lp) + 4) * 2.0 ** -23
        tol[:, b] = 0.25 * (e[:, b] + arg[:, b]) + 2.0 ** -22
        tol[:, q] = np.exp(lp[:, q]) * (np.expm1(e[:, q]) + arg[:, q])
    tol = np.where(np.isfinite(lp), tol, 0.0)        # +-Inf in link space: 0 and 1 come back exactly
    return np.where(corrected, tol, e_in if e_in is not None else 0.0)


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the entries where `want` is finite (0 / 0 counts as 0).  inf when the NaN patterns or the
    infinities differ."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    inf = np.isinf(want)
    if not np.array_equal(got[inf], want[inf]) or np.isinf(got[~inf]).any():
        return np.inf
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / np.broadcast_to(tol, want.shape)[fin])
    return float(r.max()) if r.size else 0.0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
