"""The per-entry model of the library restated in float64 numpy, for all four noise kinds, and the squared-hinge problems.

    z1 = sigma_j sum_k X_ki Y_kj,   z = z1 delta_bj + mu_j + theta_bj      (delta = 1, theta = 0 for a row in no batch and
                                                                            for a column outside every batch view)
    normal     l = 0.5 w (z - y)^2           g = w (z - y)
    bernoulli  l = w (softplus(z) - y z)     g = w (sigmoid(z) - y)
    poisson    l = w (e^z - y z)             g = w (e^z - y)
    sq_hinge   thresholds t0 <= t1 <= t2 of the column, each possibly +-inf.  class c = clamp(trunc(y + 0.5), 0, 3),
               lo = (-inf, t0, t1, t2)[c], hi = (t0, t1, t2, +inf)[c],
               a = relu(1 - (z - lo)) if lo is finite else 0,  b = relu(1 - (hi - z)) if hi is finite else 0,
               l = 0.5 w (a^2 + b^2)         g = w (b - a)
    bernoulli_sq_hinge = sq_hinge with (0, inf, inf) on 0/1 data; ordinal_sq_hinge3 = sq_hinge with (-inf, t1, t2) on 1/2/3 data.

Entries whose datum is not finite contribute nothing.  Pull-backs: gX_ki = sum_j g sigma_j delta Y_kj, gY_kj = sum_i g sigma_j
delta X_ki, grad mu_j = sum_i g, grad theta_bj = sum_{i in b} g, grad logdelta_bj = delta_bj sum_{i in b} g z1, and
grad logsigma_j = sigma_j sum_i g delta (the reference's form, which leaves the input factor out: csrc/pmf_hip.hip).
pmf_stats: residual r = invlink(z) - y for kinds 0..2 and r = b - a for sq_hinge; col_sqerr = sum r^2, col_ssq_grad =
sum (w r)^2.  impute: normal z, bernoulli sigmoid(z), poisson e^z, sq_hinge the number of thresholds strictly below z.

A problem is a dict as tests/problems.py makes them, plus "noise_thr": one entry per noise range, None or (t0, t1, t2).
Plain numpy; neither the package nor the C oracle is imported here."""
import copy
import functools

import numpy as np

import batch_cases as bc
from problems import factor_scales, make_problem

KIND = {"normal": 0, "bernoulli": 1, "poisson": 2, "bernoulli_sq_hinge": 3, "ordinal_sq_hinge3": 3}
INF = np.inf
THR = {"bernoulli_sq_hinge": (0.0, INF, INF), "ordinal_sq_hinge3": (-INF, -0.5, 0.5)}


# ---- the model -------------------------------------------------------------------------------------------------------
def kinds_of(p):
    kind = np.zeros(p["N"], np.int8)
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        kind[s - 1:e] = KIND[kd] if isinstance(kd, str) else int(kd)
    return kind


def thresholds_of(p):
    """(N, 3) float64: the thresholds of the kind-3 columns, NaN elsewhere (what pmf_get_noise_thresholds reports)."""
    t = np.full((p["N"], 3), np.nan)
    thr = p.get("noise_thr") or [None] * len(p["noise_ranges"])
    for (s, e), kd, tr in zip(p["noise_ranges"], p["noise_kinds"], thr):
        if (KIND[kd] if isinstance(kd, str) else int(kd)) == 3:
            t[s - 1:e] = np.asarray(tr if tr is not None else THR.get(kd, THR["bernoulli_sq_hinge"]), np.float64)
    return t


def batch_terms(p):
    """delta, theta as M x N arrays, and per view (c0, c1, bor, one-hot M x nb)."""
    M, N = p["M"], p["N"]
    dl, th, views = np.ones((M, N)), np.zeros((M, N)), []
    for v in p["batch_views"]:
        bor = np.asarray(v["batch_of_row"])
        nb = np.asarray(v["logdelta"]).shape[0]
        has = bor >= 0
        idx = np.ix_(has, np.arange(v["start1"] - 1, v["stop1"]))
        dl[idx] = np.exp(np.asarray(v["logdelta"], np.float64))[bor[has]]
        th[idx] = np.asarray(v["theta"], np.float64)[bor[has]]
        views.append((v["start1"] - 1, v["stop1"], bor, (bor[:, None] == np.arange(nb)[None, :]).astype(np.float64)))
    return dl, th, views


def forward(p, use_factors=True, batch=True):
    """z1, delta, theta, z (M x N, float64)."""
    X, Y = np.asarray(p["X"], np.float64), np.asarray(p["Y"], np.float64)
    sig, mu = np.exp(np.asarray(p["logsigma"], np.float64)), np.asarray(p["mu"], np.float64)
    z1 = (X.T @ Y) * sig[None, :] if use_factors else np.zeros((p["M"], p["N"]))
    if batch:
        dl, th, _ = batch_terms(p)
    else:
        dl, th = np.ones_like(z1), np.zeros_like(z1)
    return z1, dl, th, z1 * dl + mu[None, :] + th


def hinge_class(y):
    """clamp(trunc(y + 0.5), 0, 3) of finite data."""
    return np.clip(np.trunc(np.asarray(y, np.float64) + 0.5), 0, 3).astype(np.int64)


def hinge_terms(z, y, t, class_shift=0):
    """a, b of the rule above; z, y broadcastable arrays, t (..., 3) thresholds of every entry's column.  class_shift: the
    class read off by that much (a fault of the sensitivity condition; 0 is the model)."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    c = np.clip(hinge_class(y) + class_shift, 0, 3)
    ext = np.concatenate([np.full(t.shape[:-1] + (1,), -INF), t, np.full(t.shape[:-1] + (1,), INF)], axis=-1)
    ext = np.broadcast_to(ext, z.shape + (5,))
    lo = np.take_along_axis(ext, c[..., None], axis=-1)[..., 0]
    hi = np.take_along_axis(ext, c[..., None] + 1, axis=-1)[..., 0]
    with np.errstate(invalid="ignore"):
        a = np.where(np.isfinite(lo), np.maximum(0.0, 1.0 - (z - np.where(np.isfinite(lo), lo, 0.0))), 0.0)
        b = np.where(np.isfinite(hi), np.maximum(0.0, 1.0 - (np.where(np.isfinite(hi), hi, 0.0) - z)), 0.0)
    return a, b


def sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * z))


def entry_model(p, z, fault=None):
    """Per entry, unweighted and unmasked: loss l, dl/dz g, residual r, prediction (inverse link), and the hinge terms a, b
    (0 on the other kinds).  y = 0 stands in for a missing datum.  fault: None, "off_by_one" or "poisson" (kind 3 read as
    Poisson) -- the sensitivity condition's mutants."""
    kind, t = kinds_of(p), thresholds_of(p)
    D = np.asarray(p["D"], np.float64)
    y = np.where(np.isfinite(D), D, 0.0)
    l, g, pred = np.zeros_like(z), np.zeros_like(z), z.copy()
    a, b = np.zeros_like(z), np.zeros_like(z)
    n, be, po, hg = kind == 0, kind == 1, kind == 2, kind == 3
    if fault == "poisson":
        po, hg = po | hg, np.zeros_like(hg)
    g[:, n] = z[:, n] - y[:, n]
    l[:, n] = 0.5 * g[:, n] ** 2
    pred[:, be] = sigmoid(z[:, be])
    g[:, be] = pred[:, be] - y[:, be]
    l[:, be] = np.logaddexp(0.0, z[:, be]) - y[:, be] * z[:, be]
    pred[:, po] = np.exp(z[:, po])
    g[:, po] = pred[:, po] - y[:, po]
    l[:, po] = pred[:, po] - y[:, po] * z[:, po]
    if hg.any():
        th = np.where(np.isnan(t[hg]), 0.0, t[hg])
        a[:, hg], b[:, hg] = hinge_terms(z[:, hg], y[:, hg], th[None, :, :], 1 if fault == "off_by_one" else 0)
        g[:, hg] = b[:, hg] - a[:, hg]
        l[:, hg] = 0.5 * (a[:, hg] ** 2 + b[:, hg] ** 2)
        pred[:, hg] = (th[None, :, :] < z[:, hg][:, :, None]).sum(-1)
    r = np.where(hg[None, :], g, pred - y)
    return dict(l=l, g=g, r=r, pred=pred, a=a, b=b)


def reference(p, fault=None):
    """data_loss, X, Y (factor gradients), mu, logsigma, theta[v], logdelta[v] (layer gradients), g (M x N, weighted and
    masked), z, and the hinge terms a, b (masked)."""
    X, Y = np.asarray(p["X"], np.float64), np.asarray(p["Y"], np.float64)
    sig, w = np.exp(np.asarray(p["logsigma"], np.float64)), np.asarray(p["col_weight"], np.float64)
    z1, dl, th, z = forward(p)
    obs = np.isfinite(p["D"])
    e = entry_model(p, z, fault)
    g = np.where(obs, w[None, :] * e["g"], 0.0)
    out = dict(data_loss=float(np.sum(np.where(obs, w[None, :] * e["l"], 0.0))), g=g, z=z,
               a=np.where(obs, e["a"], 0.0), b=np.where(obs, e["b"], 0.0))
    ga = g * dl * sig[None, :]                              # dloss / d(X'Y)
    out["X"], out["Y"] = Y @ ga.T, X @ ga
    out["mu"], out["logsigma"] = g.sum(0), sig * (g * dl).sum(0)
    out["theta"], out["logdelta"] = [], []
    for v, (c0, c1, bor, onehot) in zip(p["batch_views"], batch_terms(p)[2]):
        out["theta"].append(onehot.T @ g[:, c0:c1])
        out["logdelta"].append(np.exp(np.asarray(v["logdelta"], np.float64)) * (onehot.T @ (g * z1)[:, c0:c1]))
    return out


def stats(p, use_factors):
    """The vectors of pmf_stats (n, sum, sumsq, sqerr, ssq_grad) and the per-(batch, column) counts and squared errors."""
    _, _, _, z = forward(p, use_factors)
    w = np.asarray(p["col_weight"], np.float64)
    obs = np.isfinite(p["D"])
    y = np.where(obs, np.asarray(p["D"], np.float64), 0.0)
    r = np.where(obs, entry_model(p, z)["r"], 0.0)
    out = dict(n=obs.sum(0).astype(np.float64), sum=y.sum(0), sumsq=(y * y).sum(0), sqerr=(r * r).sum(0),
               ssq_grad=((w[None, :] * r) ** 2).sum(0), batch_count=[], batch_sqerr=[])
    for c0, c1, bor, onehot in batch_terms(p)[2]:
        out["batch_count"].append(onehot.T @ obs[:, c0:c1].astype(np.float64))
        out["batch_sqerr"].append(onehot.T @ (r * r)[:, c0:c1])
    return out


def impute(p, batch=False, link=False):
    """(values, z): the predictions of every entry and their link-space values."""
    _, _, _, z = forward(p, batch=batch)
    return (z.copy() if link else entry_model(p, z)["pred"]), z


def threshold_gap(p, z):
    """M x N: the distance of z from the nearest finite threshold of its column (inf on the other kinds)."""
    t = thresholds_of(p)
    d = np.abs(z[:, :, None] - np.where(np.isfinite(t), t, np.inf)[None, :, :])
    return np.where(np.isnan(d), np.inf, d).min(-1)


def entry_scales(p, c0=0, c1=None):
    """problems.entry_scales with kind 3: per observed entry sG = w (|a| + |b| + |lo|[a > 0] + |hi|[b > 0] + link' r) with
    link' = [a > 0] + [b > 0] in {0, 1, 2} -- g = w (b - a), a = 1 - z + lo, b = 1 + z - hi: the magnitudes the kernel
    rounds are the two terms, the bounds they are formed from, and z (through r) once per active term -- and the loss
    magnitude 0.5 w (a^2 + b^2), the loss itself.  Kinds 0..2 as there (tests/test_hinge_cases.py holds the two equal).
    The whole matrix is evaluated (these problems are small) and the columns [c0, c1) returned."""
    X, Y = np.asarray(p["X"], np.float64), np.asarray(p["Y"], np.float64)
    sig, mu = np.exp(np.asarray(p["logsigma"], np.float64)), np.asarray(p["mu"], np.float64)
    w, kind, t = np.asarray(p["col_weight"], np.float64), kinds_of(p), thresholds_of(p)
    z1, dl, th, z = forward(p)
    Aabs = np.abs(X).T @ np.abs(Y)
    obs = np.isfinite(p["D"])
    y = np.where(obs, np.asarray(p["D"], np.float64), 0.0)
    e = entry_model(p, z)
    link, dlink = z.copy(), np.ones_like(z)
    be, po, hg = kind == 1, kind == 2, kind == 3
    link[:, be], dlink[:, be] = e["pred"][:, be], e["pred"][:, be] * (1.0 - e["pred"][:, be])
    link[:, po] = dlink[:, po] = e["pred"][:, po]
    g = np.where(obs, w[None, :] * e["g"], 0.0)
    r = sig[None, :] * Aabs * dl + np.abs(mu)[None, :] + np.abs(th)
    mag = np.abs(link) + np.abs(y) + dlink * r
    if hg.any():
        a, b = e["a"][:, hg], e["b"][:, hg]
        c = hinge_class(y[:, hg])
        ext = np.concatenate([np.zeros((hg.sum(), 1)), np.where(np.isfinite(t[hg]), np.abs(t[hg]), 0.0), np.zeros((hg.sum(), 1))], 1)
        ext = np.broadcast_to(ext[None], c.shape + (5,))
        lo = np.take_along_axis(ext, c[..., None], -1)[..., 0]
        hi = np.take_along_axis(ext, c[..., None] + 1, -1)[..., 0]
        mag[:, hg] = a + b + lo * (a > 0) + hi * (b > 0) + ((a > 0).astype(float) + (b > 0)) * r[:, hg]
    sG = np.where(obs, w[None, :] * mag, 0.0)
    sQ = np.abs(z1) * sG + np.abs(g) * sig[None, :] * Aabs
    lm = np.where(kind[None, :] == 0, 0.5 * (z - y) ** 2,
                  np.where(kind[None, :] == 3, e["l"],
                           np.where(kind[None, :] == 1, np.logaddexp(0.0, z), np.exp(np.minimum(z, 700.0))) + np.abs(y * z)))
    out = dict(g=g, sG=sG, sQ=sQ, sd=sig[None, :] * dl, delta=dl, loss=np.where(obs, w[None, :] * lm, 0.0))
    return {k: v[:, c0:c1] for k, v in out.items()}


def layer_scales(p):
    """problems.layer_scales from the entry terms above (kind 3 included)."""
    sig = np.exp(np.asarray(p["logsigma"], np.float64))
    e = entry_scales(p)
    sG, sQ = e["sG"], e["sQ"]
    out = dict(mu=sG.sum(0), logsigma=sig * (e["delta"] * sG).sum(0), theta=[], logdelta=[], g=e["g"],
               loss=float(np.sum(e["loss"])))
    for v, (c0, c1, bor, onehot) in zip(p["batch_views"], batch_terms(p)[2]):
        out["theta"].append(onehot.T @ sG[:, c0:c1])
        out["logdelta"].append(np.exp(np.asarray(v["logdelta"], np.float64)) * (onehot.T @ sQ[:, c0:c1]))
    return out


# ---- the problems ----------------------------------------------------------------------------------------------------
M = 70                                      # two full 32-row blocks and a ragged one
KS = (20, 48, 80, 128)
LAYOUT_A = [((1, 20), "bernoulli", None), ((21, 75), "bernoulli_sq_hinge", None), ((76, 110), "normal", None),
            ((111, 165), "ordinal_sq_hinge3", None), ((166, 173), "poisson", None)]
LAYOUT_B = [((1, 40), 3, (-INF, -0.5, 0.5)), ((41, 50), 3, (0.0, INF, INF)), ((51, 77), 3, (-INF, -1.2, 0.3))]
SEAMS = {"A": 50, "B": 45}                  # last column of the first batch view: inside tile 1, which holds kind-3 columns


def factor_scale(K):
    return 0.4 * (20.0 / K) ** 0.25


def layout_from(spec, M, K, seed, views=None, **make_kw):
    """The problem of a spec [((start1, stop1), kind, triple or None)] at M rows: make_problem(M, N, K, seed, **make_kw) with
    column weights, logsigma, mu, 10 % NaN; X and Y scaled by 0.4 (20 / K)^(1/4); the data of the kind-3 columns are the class
    of z + 0.5 N(0, 1) under the column's thresholds, those of a Bernoulli range that make_problem did not draw as one are
    1[D > 0].  views: None, or a function (M, N, rng) -> [(start1, stop1, batch_of_row, nb)] called after the classes are
    drawn (it may draw from rng); D does not follow the batch effects."""
    N = spec[-1][0][1]
    p = make_problem(M=M, N=N, K=K, seed=seed, nan_frac=0.1, weights=True, col_params=True, scale=factor_scale(K), **make_kw)
    drawn = kinds_of(p)
    p["noise_ranges"] = [r for r, _, _ in spec]
    p["noise_kinds"] = [k for _, k, _ in spec]
    p["noise_thr"] = [t if t is not None else THR.get(k) for _, k, t in spec]
    rng = np.random.default_rng(seed + 1)
    _, _, _, z = forward(p, batch=False)
    t = thresholds_of(p)
    D = np.array(p["D"], np.float32)
    for j in np.flatnonzero(kinds_of(p) == 3):
        cls = (t[j][None, :] < (z[:, j] + 0.5 * rng.standard_normal(M))[:, None]).sum(1)
        D[:, j] = np.where(np.isnan(D[:, j]), np.nan, cls)
    for j in np.flatnonzero((kinds_of(p) == 1) & (drawn != 1)):
        D[:, j] = np.where(np.isnan(D[:, j]), np.nan, D[:, j] > 0)
    p["D"] = np.asfortranarray(D)
    if views is not None:
        bvs = []
        for s, e, bor, nb in views(M, N, rng):
            cd, ct = rng.standard_normal(nb)[:, None] * 0.25, rng.standard_normal(nb)[:, None] * 0.25
            bvs.append(dict(start1=s, stop1=e, batch_of_row=np.asarray(bor, np.int32),
                            logdelta=(cd + 0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                            theta=(ct + 0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32)))
        p["batch_views"] = bvs
    return p


@functools.lru_cache(maxsize=None)
def layout(name, K, batch=False):
    """Layout A (N = 173, the reference's sorted order, kinds by name) or B (N = 77, raw kind 3 with explicit thresholds),
    M = 70, column weights, logsigma, mu, 10 % NaN; X and Y scaled by 0.4 (20 / K)^(1/4); the data of the kind-3 columns are
    the class of z + 0.5 N(0, 1) under the column's thresholds.  batch: two batch views (4 sorted batches with a few rows
    in no batch; 6 scrambled) whose seam falls inside a kind-3 tile; D does not follow the batch effects."""
    spec = LAYOUT_A if name == "A" else LAYOUT_B
    N = spec[-1][0][1]
    seed = 1000 + K + (0 if name == "A" else 500)

    def views(M, N, rng):
        b0 = bc.sorted_rows(M, 4)
        b0[[0, 33, M - 1]] = -1
        return [(1, SEAMS[name], b0, 4), (SEAMS[name] + 1, N, bc.scrambled_rows(M, 6, rng), 6)]

    kw = dict(bernoulli_frac=20 / N, poisson_frac=8 / N) if name == "A" else {}
    return layout_from(spec, M, K, seed, views if batch else None, **kw)


def all_problems():
    return [(f"{name}-k{K}-{'batch' if b else 'plain'}", layout(name, K, b)) for name in "AB" for K in KS for b in (False, True)]


_REF = {}


def reference_of(p):
    """reference(p), once per problem (the builders return shared objects: do not modify them)."""
    if id(p) not in _REF:
        _REF[id(p)] = (p, reference(p))
    return _REF[id(p)][1]


_SCALES = {}


def scales_of(p):
    """problems.factor_scales(p) -- it takes the entry terms of a problem with "noise_thr" from entry_scales above -- once
    per problem (cached by identity, like reference_of)."""
    if id(p) not in _SCALES:
        _SCALES[id(p)] = (p, factor_scales(p))
    return _SCALES[id(p)][1]


def to_context(p, ctx):
    """problems.to_context, then the thresholds of the kind-3 ranges (as matfac.marshal sends them after set_noise)."""
    import problems
    problems.to_context(p, ctx)
    rt = [(r, t) for r, t in zip(p["noise_ranges"], p.get("noise_thr") or []) if t is not None]
    if rt:
        ctx.set_noise_thresholds([r for r, _ in rt], [t for _, t in rt])
    return ctx


# ---- the sensitivity condition's faults ------------------------------------------------------------------------------
def swapped_thresholds(p):
    """The thresholds of the first two kind-3 ranges that differ, exchanged."""
    idx = [i for i, t in enumerate(p["noise_thr"]) if t is not None]
    q = copy.copy(p)
    q["noise_thr"] = list(p["noise_thr"])
    for n, i in enumerate(idx):
        for j in idx[n + 1:]:
            if tuple(p["noise_thr"][i]) != tuple(p["noise_thr"][j]):
                q["noise_thr"][i], q["noise_thr"][j] = p["noise_thr"][j], p["noise_thr"][i]
                return q
    raise AssertionError("no two kind-3 ranges with different thresholds")
