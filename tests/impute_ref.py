"""What pmf_impute must compute, restated in numpy, and how closely.

    z = a sigma_j + mu_j                                   (flags = 0; a = sum_k X[k,i] Y[k,j])
    z = a sigma_j delta_v[b,j] + mu_j + theta_v[b,j]       (BATCH; a row in no batch: delta = 1, theta = 0)
    normal -> z ; bernoulli -> 1 / (1 + e^-z) ; poisson -> e^z          (LINK: z for every column)

`impute_ref(p, flags)` evaluates this in float64 and `impute_ref(p, flags, np.float32)` is its float32 twin (every
operation, np.exp included, in float32).  `impute_tol` is the per-entry bound against the float64 values:

    link space   e_z = (K + 8) 2^-24 scale, scale = sigma_j delta sum_k |X_ki Y_kj| + |mu_j| + |theta| (the scale of
                 test_forward_k_edges_match_oracle; without the batch terms when BATCH is off)
    normal       e_z
    poisson      e^z (expm1(e_z) + (|z| + 4) 2^-23): the argument's product with log2(e) rounds to |z| 2^-24 relative,
                 v_exp_f32 is 1 ulp, one more rounding, and a factor of two on top
    bernoulli    (e_z + (|z| + 4) 2^-23) / 4 + 2^-22      (the logistic function's slope is at most 1/4)
"""
import numpy as np

from test_gpu_layer_edges import layer_problem, std_views

BATCH, LINK, KEEP = 1, 2, 4
KIND = {"normal": 0, "bernoulli": 1, "poisson": 2}

K_EDGES = [1, 31, 32, 33, 64, 65, 96, 97, 128]
# (K, M, N): every K edge at (300, 129); every M edge at K = 33 (eight waves: 256-row panels); every N edge at K = 97
# (four waves: 128-row panels)
CASES = [(K, 300, 129) for K in K_EDGES] + [(33, M, 65) for M in (1, 31, 33, 257)] + [(97, 300, N) for N in (1, 33, 65)]
FLAG_SETS = [0, BATCH, LINK, BATCH | LINK]


def case_problem(K, M, N, seed=None):
    """Mixed noise, column parameters, 5 % NaN and the std_views batch layout, with rows in no batch at 0, 3 and M - 1."""
    seed = 700 + K + M + N if seed is None else seed
    p = layer_problem(M, N, K, seed, std_views(M, N, seed))
    bor = p["batch_views"][0]["batch_of_row"]
    bor[[i for i in (0, 3, M - 1) if i < M]] = -1
    return p


def kinds_of(p):
    kind = np.zeros(p["N"], np.int8)
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        kind[s - 1:e] = KIND[kd]
    return kind


def _batch_terms(p, dtype):
    """delta, theta as M x N arrays (1 and 0 outside the batch views and for rows in no batch)."""
    M, N = p["M"], p["N"]
    dl, th = np.ones((M, N), dtype), np.zeros((M, N), dtype)
    for v in p["batch_views"]:
        bor = np.asarray(v["batch_of_row"])
        has = bor >= 0
        idx = np.ix_(has, np.arange(v["start1"] - 1, v["stop1"]))
        dl[idx] = np.exp(np.asarray(v["logdelta"], dtype))[bor[has]]
        th[idx] = np.asarray(v["theta"], dtype)[bor[has]]
    return dl, th


def link_space(p, flags, dtype=np.float64):
    X, Y = np.asarray(p["X"], dtype), np.asarray(p["Y"], dtype)
    sig, mu = np.exp(np.asarray(p["logsigma"], dtype)), np.asarray(p["mu"], dtype)
    z1 = (X.T @ Y) * sig[None, :]
    if flags & BATCH:
        dl, th = _batch_terms(p, dtype)
        return z1 * dl + (mu[None, :] + th)
    return z1 + mu[None, :]


def inv_link(p, z, flags):
    out = z.copy()
    if flags & LINK:
        return out
    one = z.dtype.type(1)
    kind = kinds_of(p)
    with np.errstate(over="ignore"):
        out[:, kind == 1] = one / (one + np.exp(-z[:, kind == 1]))
        out[:, kind == 2] = np.exp(z[:, kind == 2])
    return out


def impute_ref(p, flags, dtype=np.float64):
    """(values, z) of the whole matrix; KEEP_OBSERVED puts the finite entries of p["D"] back."""
    z = link_space(p, flags, dtype)
    out = inv_link(p, z, flags)
    assert out.dtype == dtype and z.dtype == dtype
    if flags & KEEP:
        obs = np.isfinite(p["D"])
        out[obs] = p["D"][obs]
    return out, z


def scale_of(p, flags):
    X, Y = np.abs(np.asarray(p["X"], np.float64)), np.abs(np.asarray(p["Y"], np.float64))
    s = (X.T @ Y) * np.exp(np.asarray(p["logsigma"], np.float64))[None, :]
    amu = np.abs(np.asarray(p["mu"], np.float64))[None, :]
    if flags & BATCH:
        dl, th = _batch_terms(p, np.float64)
        return s * dl + amu + np.abs(th)
    return s + amu


def impute_tol(p, flags, z):
    """Per-entry bound on |device - float64| (z: the float64 link-space values)."""
    ez = (p["K"] + 8) * 2.0 ** -24 * scale_of(p, flags)
    tol = ez.copy()
    if flags & LINK:
        return tol
    kind = kinds_of(p)
    arg = (np.abs(z) + 4) * 2.0 ** -23
    b, q = kind == 1, kind == 2
    tol[:, b] = 0.25 * (ez[:, b] + arg[:, b]) + 2.0 ** -22
    with np.errstate(over="ignore"):
        tol[:, q] = np.exp(z[:, q]) * (np.expm1(ez[:, q]) + arg[:, q])
    return tol


def worst_ratio(got, want, tol):
    """max |got - want| / tol over the entries (0 / 0 counts as 0); inf if `got` is not finite somewhere `want` is."""
    got = np.asarray(got, np.float64)
    bad = ~np.isfinite(got) & np.isfinite(want)
    if bad.any():
        return np.inf
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    return float(np.nanmax(r)) if r.size else 0.0
