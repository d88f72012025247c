"""Factor importance (include/pmf_hip_importance.h, DESIGN.md section 2, Deviation 6) restated in float64 numpy on the model
of tests/hinge_ref.py, a float32 twin of the kernel's arithmetic, and the rounding bound the device is held to.

    a_ij      = z1_ij delta_bj + mu_j + theta_bj,   z1_ij = sigma_j sum_k x_ki y_kj           (hinge_ref.forward)
    a^(-k)_ij = (z1_ij - sigma_j x_ki y_kj) delta_bj + mu_j + theta_bj,   a^(0)_ij = mu_j + theta_bj
    full[j] = sum_i l(a_ij)   null[j] = sum_i l(a^(0)_ij)   delta[k, j] = sum_i (l(a^(-k)_ij) - l(a_ij))   n_obs[j] = #i
over the observed entries of the columns whose weight is not 0; l includes the column weight (hinge_ref.entry_model).

THE BOUND, per output element, with eps = 2^-24, g = dl/da and T_ij = K sum_k |sigma_j x_ki y_kj delta_bj|:
    delta[k, j]:  eps (C_DELTA sum_i (|l(a^(-k))| + |l(a)| + |g(a^(-k)) - g(a)| T_ij) + CHAIN sum_i |l(a^(-k)) - l(a)|)
    full[j]:      eps (C_FULL sum_i |l(a)| + CHAIN sum_i |l(a)|)
    null[j]:      eps (C_NULL sum_i |l(a^(0))| + CHAIN sum_i |l(a^(0))|)
The first bracket is what the float32 evaluation of the entry terms can lose (the losses themselves, and the error of z1 --
common to both arguments of a difference -- through the change of slope), the second the float32 accumulation: CHAIN = 512
(PMF_IMPORTANCE_CHAIN) entries at most are added in float32 before the sum goes to float64, each addition rounding a
partial sum that is at most sum_i |term|.  full and null have the same form without the difference term: the losses alone,
each with a constant of its own (the rounding of the argument reaches full through the slope and is inside C_FULL; null's
argument mu + theta holds no product).

The constants are MEASURED, as tests/step_ref.py derives its constants: the worst ratio of the float32 twin's whole error (its
float32 accumulation included: the conservative side, since the CHAIN term then counts that part again) to the first bracket
over the case table below (cases()), times 4 for the device's fast exp / log / rcp and its different (fused, MFMA-ordered)
roundings:
    delta: worst ratio 1.16 (mix-45x37-k1)                      ->  C_DELTA = 5
    full:  worst ratio 41.6 (hinge-A-k48-plain)                 ->  C_FULL = 167
    null:  worst ratio 21.8 (hinge-A-k48-plain)                 ->  C_NULL = 88
tests/test_importance_cases.py re-measures all three and fails if a ratio has grown past a quarter of its constant.

Plain numpy; neither the package nor the C oracle is imported here."""
import functools

import numpy as np

import batch_cases as bc
import hinge_ref as hr
from problems import make_problem

CHAIN = 512
EPS = 2.0 ** -24
C_DELTA = 5.0
C_FULL = 167.0
C_NULL = 88.0


def _weights(p):
    return np.asarray(p["col_weight"], np.float64)


def _observed(p):
    return np.isfinite(p["D"]) & (_weights(p) != 0)[None, :]


def _loss(p, a):
    """Weighted entry loss and slope at the outputs a (M x N), unmasked."""
    e = hr.entry_model(p, a)
    w = _weights(p)[None, :]
    return w * e["l"], w * e["g"]


def reference(p):
    """dict(delta (K, N), full, null (N,), n_obs (N,) int64) in float64, with the brackets of the bound: b_delta, c_delta
    (K, N), b_full, c_full, b_null, c_null (N,) -- bound = EPS (C b + CHAIN c) (bounds())."""
    X, Y = np.asarray(p["X"], np.float64), np.asarray(p["Y"], np.float64)
    sig, mu = np.exp(np.asarray(p["logsigma"], np.float64)), np.asarray(p["mu"], np.float64)
    K = X.shape[0]
    z1, dl, th, a = hr.forward(p)
    obs = _observed(p)
    mt = mu[None, :] + th
    T = K * (np.abs(X).T @ np.abs(Y)) * sig[None, :] * np.abs(dl)
    lf, gf = _loss(p, a)
    l0, _ = _loss(p, mt)
    m = lambda v: np.where(obs, v, 0.0)                                      # noqa: E731
    out = dict(full=m(lf).sum(0), null=m(l0).sum(0), n_obs=obs.sum(0).astype(np.int64),
               b_full=m(np.abs(lf)).sum(0), c_full=m(np.abs(lf)).sum(0), b_null=m(np.abs(l0)).sum(0), c_null=m(np.abs(l0)).sum(0),
               delta=np.zeros((K, p["N"])), b_delta=np.zeros((K, p["N"])), c_delta=np.zeros((K, p["N"])))
    for k in range(K):
        ak = (z1 - sig[None, :] * np.outer(X[k], Y[k])) * dl + mt
        lk, gk = _loss(p, ak)
        same = ak == a                                                        # an absent term: exactly absent
        d = np.where(same, 0.0, lk - lf)
        out["delta"][k] = m(d).sum(0)
        out["b_delta"][k] = m(np.where(same, 0.0, np.abs(lk) + np.abs(lf) + np.abs(gk - gf) * T)).sum(0)
        out["c_delta"][k] = m(np.abs(d)).sum(0)
    return out


def bounds(ref):
    """The bound of every output element: dict(delta (K, N), full (N,), null (N,))."""
    return dict(delta=EPS * (C_DELTA * ref["b_delta"] + CHAIN * ref["c_delta"]),
                full=EPS * (C_FULL * ref["b_full"] + CHAIN * ref["c_full"]),
                null=EPS * (C_NULL * ref["b_null"] + CHAIN * ref["c_null"]))


# ---- the float32 twin ----------------------------------------------------------------------------------------------------
F = np.float32


def _loss32(p, a, y):
    """The expressions of pmf_noise in float32 (a, y: M x N float32; y = 0 where masked)."""
    kind, t = hr.kinds_of(p), hr.thresholds_of(p)
    w = np.asarray(p["col_weight"], F)[None, :]
    l = np.zeros_like(a)
    n, be, po, hg = kind == 0, kind == 1, kind == 2, kind == 3
    d = a[:, n] - y[:, n]
    g = w[:, n] * d
    l[:, n] = F(0.5) * g * d
    e = np.exp(-np.abs(a[:, be]))
    l[:, be] = w[:, be] * ((np.maximum(a[:, be], F(0)) + np.log(F(1) + e)) - y[:, be] * a[:, be])
    with np.errstate(over="ignore"):
        l[:, po] = w[:, po] * (np.exp(a[:, po]) - y[:, po] * a[:, po])
    if hg.any():
        z, yy = a[:, hg], y[:, hg]
        th = np.where(np.isnan(t[hg]), 0.0, t[hg]).astype(F)
        c = np.clip(np.trunc(yy + F(0.5)), 0, 3).astype(np.int64)
        ext = np.concatenate([np.full((th.shape[0], 1), -np.inf, F), th, np.full((th.shape[0], 1), np.inf, F)], 1)
        ext = np.broadcast_to(ext[None], z.shape + (5,))
        lo = np.take_along_axis(ext, c[..., None], -1)[..., 0]
        hi = np.take_along_axis(ext, c[..., None] + 1, -1)[..., 0]
        with np.errstate(invalid="ignore"):
            ta = np.where(np.isfinite(lo), np.maximum(F(0), F(1) - (z - np.where(np.isfinite(lo), lo, F(0)))), F(0))
            tb = np.where(np.isfinite(hi), np.maximum(F(0), F(1) - (np.where(np.isfinite(hi), hi, F(0)) - z)), F(0))
        l[:, hg] = F(0.5) * w[:, hg] * (ta * ta + tb * tb)
    assert l.dtype == F
    return l


def _chain_sum(v):
    """Column sums of a float32 M x N array as the kernel forms them: float32 in row order for CHAIN rows, then float64."""
    out = np.zeros(v.shape[1])
    for r0 in range(0, v.shape[0], CHAIN):
        out += np.cumsum(v[r0:r0 + CHAIN], axis=0, dtype=F)[-1].astype(np.float64)
    return out


def twin(p):
    """dict(delta, full, null, n_obs): the definition in float32 arithmetic with the kernel's chain length."""
    X, Y = np.asarray(p["X"], F), np.asarray(p["Y"], F)
    sig, mu = np.exp(np.asarray(p["logsigma"], F)), np.asarray(p["mu"], F)
    M, N, K = p["M"], p["N"], X.shape[0]
    Ys = Y * sig[None, :]
    z1 = X.T @ Ys
    dl, th = np.ones((M, N), F), np.zeros((M, N), F)
    for v in p["batch_views"]:
        bor = np.asarray(v["batch_of_row"])
        has = bor >= 0
        idx = np.ix_(has, np.arange(v["start1"] - 1, v["stop1"]))
        dl[idx] = np.exp(np.asarray(v["logdelta"], F))[bor[has]]
        th[idx] = np.asarray(v["theta"], F)[bor[has]]
    obs = _observed(p)
    y = np.where(obs, np.asarray(p["D"], F), F(0))
    mt = mu[None, :] + th
    z0 = np.zeros((), F)
    z1, dl, mt = np.where(obs, z1, z0), np.where(obs, dl, z0), np.where(obs, mt, z0)   # a masked entry sits at 0
    lf = _loss32(p, z1 * dl + mt, y)
    l0 = _loss32(p, mt, y)
    out = dict(full=_chain_sum(np.where(obs, lf, z0)), null=_chain_sum(np.where(obs, l0, z0)),
               n_obs=obs.sum(0).astype(np.int64), delta=np.zeros((K, N)))
    for k in range(K):
        lk = _loss32(p, (z1 - Ys[k][None, :] * X[k][:, None]) * dl + mt, y)
        out["delta"][k] = _chain_sum(lk - lf)
    return out


def worst_ratios(p, ref=None, tw=None):
    """(delta, full, null): the twin's whole error over the first bracket of the bound -- what C_DELTA, C_FULL and C_NULL are
    four times the worst of.  Where the bracket is 0 the twin is exact."""
    ref = reference(p) if ref is None else ref
    tw = twin(p) if tw is None else tw

    def ratio(k):
        err, b = np.abs(tw[k] - ref[k]), ref["b_" + k]
        assert (err[b == 0] == 0).all()
        return float(np.max(err[b > 0] / (EPS * b[b > 0]), initial=0.0))

    return ratio("delta"), ratio("full"), ratio("null")


# ---- the case table ----------------------------------------------------------------------------------------------------------
def mix_problem(M, N, K, seed=11, batch=True, **kw):
    """Normal, Bernoulli and Poisson columns (the kinds the C oracle has), weights, column parameters, 10 % missing, two batch
    views of 4 batches; factors at hinge_ref's scale."""
    return make_problem(M=M, N=N, K=K, seed=seed, bernoulli_frac=0.25, poisson_frac=0.2, n_views=2, batch_views=2 if batch else 0,
                        n_batches=4, nan_frac=0.1, weights=True, col_params=True, scale=hr.factor_scale(K), **kw)


def firm(p, seed=0):
    """A copy of p with FIRM factors -- every entry of X and Y has a magnitude in [0.5, 1.5] x hinge_ref.factor_scale(K), random
    signs -- and data redrawn from that model by the rules of make_problem / hinge_ref.layout_from; the missing entries stay
    missing.  The bound of delta[k, j] grows with K sum_k |x y| / |x_k y_k|: with Gaussian factors, at K = 128, a fifth of the
    (k, j) have a factor so nearly absent that their delta is below ten bounds, which says nothing about the kernel."""
    rng = np.random.default_rng(1234 + seed)
    K, M, N = p["K"], p["M"], p["N"]
    q = dict(p)
    s = hr.factor_scale(K)
    for name, n in (("X", M), ("Y", N)):
        q[name] = np.asfortranarray((rng.choice([-1.0, 1.0], (K, n)) * (0.5 + rng.random((K, n))) * s).astype(np.float32))
    _, _, _, z = hr.forward(q)
    kind, t = hr.kinds_of(q), hr.thresholds_of(q)
    D = z + 0.1 * rng.standard_normal((M, N))
    for j in range(N):
        if kind[j] == 1:
            D[:, j] = D[:, j] > 0
        elif kind[j] == 2:
            D[:, j] = rng.poisson(np.exp(np.clip(z[:, j], -5, 3)))
        elif kind[j] == 3:
            D[:, j] = (t[j][None, :] < (z[:, j] + 0.5 * rng.standard_normal(M))[:, None]).sum(1)
    q["D"] = np.asfortranarray(np.where(np.isnan(p["D"]), np.nan, D).astype(np.float32))
    return q


GEOMETRY_KS = (1, 2, 32, 33, 64, 65, 128)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> problem (shared objects: do not modify them): the problems of the CPU checks AND of the device tests' geometry
    and model-mix cases.  mix-*: normal, Bernoulli and Poisson columns (what the C oracle has); hinge-A: all four kinds,
    hinge-B: kind 3 alone, both with a batch-view seam inside a tile and rows in no batch."""
    out = {"mix-70x100-k40": firm(mix_problem(70, 100, 40))}
    for K in GEOMETRY_KS:
        out[f"mix-45x37-k{K}"] = firm(mix_problem(45, 37, K, batch=K != 2), K)
    for M in (31, 32, 33):
        out[f"mix-{M}x37-k20"] = firm(mix_problem(M, 37, 20), M)
    out["normal-45x1-k20"] = firm(make_problem(M=45, N=1, K=20, seed=5, nan_frac=0.1, weights=True, col_params=True), 1)
    for name, K, b in (("A", 20, True), ("A", 48, False), ("A", 128, True), ("B", 80, True), ("B", 20, False)):
        out[f"hinge-{name}-k{K}-{'batch' if b else 'plain'}"] = firm(hr.layout(name, K, b), K)
    # one 32-column tile that holds all four kinds, then a ragged tile of one
    spec = [((1, 8), "bernoulli", None), ((9, 16), "bernoulli_sq_hinge", None), ((17, 24), "normal", None), ((25, 40), "poisson", None)]
    out["allkinds-tile-k20"] = firm(hr.layout_from(spec, 70, 20, 71, bernoulli_frac=8 / 40, poisson_frac=16 / 40), 71)
    # every kind alone in a full tile and a ragged one (the wave-uniform branch)
    for kind, thr in (("normal", None), ("bernoulli", None), ("poisson", None), ("ordinal_sq_hinge3", (-1.0, 0.0, hr.INF))):
        kw = dict(bernoulli_frac=1.0) if kind == "bernoulli" else dict(poisson_frac=1.0) if kind == "poisson" else {}
        out[f"alone-{kind}-k20"] = firm(hr.layout_from([((1, 40), kind, thr)], 70, 20, 72, **kw), 72)

    # two batch views of 8 and 33 batches, columns 21..29 in no view, rows in no batch, the second view ending inside a tile
    def views(M, N, rng):
        b0 = bc.sorted_rows(M, 8)
        b0[[1, 40]] = -1
        return [(1, 20, b0, 8), (30, 50, bc.scrambled_rows(M, 33, rng), 33)]

    out["views-8-33-gap-k20"] = firm(hr.layout_from(hr.LAYOUT_B, 70, 20, 73, views), 73)
    return out


_REF = {}


def reference_of(p):
    """reference(p) and bounds(reference(p)), once per problem object."""
    if id(p) not in _REF:
        r = reference(p)
        _REF[id(p)] = (p, r, bounds(r))
    return _REF[id(p)][1:]


def check(got, p, what=("delta", "full", "null", "n_obs"), ref=None):
    """The device's (or the twin's) outputs against the reference, element by element within the bound; n_obs exactly."""
    r, b = reference_of(p) if ref is None else ref
    for k in what:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        assert g.shape == r[k].shape, (k, g.shape, r[k].shape)
        if k == "n_obs":
            assert np.array_equal(g, r[k]), k
            continue
        err = np.abs(g - r[k])
        bad = ~(err <= b[k])
        assert not bad.any(), (k, int(bad.sum()), float(np.nanmax(np.where(b[k] > 0, err / np.where(b[k] > 0, b[k], 1), 0))),
                               np.argwhere(bad)[:4].tolist())
