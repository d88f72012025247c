"""Seeded synthetic problem instances shared by the oracle-side and HIP-side tests.

A problem is a plain dict of numpy arrays in the reference's conventions (column-major semantics,
1-based inclusive ranges).  `to_oracle` feeds it to the C oracle, `to_context` to libpmf_hip.so through
the ctypes binding, so every parity test runs the SAME inputs through both.
Distributions follow src/simulate_params.jl.
"""
import numpy as np


def split_ranges(n, parts):
    """n items into `parts` contiguous 1-based inclusive ranges."""
    edges = np.linspace(0, n, parts + 1).astype(int)
    return [(int(edges[i]) + 1, int(edges[i + 1])) for i in range(parts) if edges[i + 1] > edges[i]]


def make_problem(M, N, K, seed=0, bernoulli_frac=0.0, poisson_frac=0.0, n_views=1, batch_views=0, n_batches=4,
                 nan_frac=0.0, xreg=None, yreg=None, weights=False, col_params=False, layer_regs=False,
                 n_groups=3, noise=0.1, scale=1.0, random_init=False, batch_order="mixed"):
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((K, M)) * scale).astype(np.float32)
    Y = (rng.standard_normal((K, N)) * scale).astype(np.float32)
    logsigma = (rng.standard_normal(N) * 0.1).astype(np.float32) if col_params else np.zeros(N, np.float32)
    mu = rng.standard_normal(N).astype(np.float32) if col_params else np.zeros(N, np.float32)
    # noise model: contiguous ranges normal | bernoulli | poisson (columns sorted by distribution: model.jl:50-54)
    n_b = int(round(N * bernoulli_frac))
    n_p = int(round(N * poisson_frac))
    n_n = N - n_b - n_p
    noise_ranges, kinds = [], []
    c = 1
    for cnt, kd in ((n_b, "bernoulli"), (n_n, "normal"), (n_p, "poisson")):  # alphabetical like the reference sort
        if cnt > 0:
            noise_ranges.append((c, c + cnt - 1))
            kinds.append(kd)
            c += cnt
    kind_of_col = np.empty(N, dtype=object)
    for (s, e), kd in zip(noise_ranges, kinds):
        kind_of_col[s - 1:e] = kd
    view_ranges = split_ranges(N, n_views)
    # batch views: the first `batch_views` feature views get row batches
    bviews = []
    for v in range(min(batch_views, len(view_ranges))):
        s, e = view_ranges[v]
        Nv = e - s + 1
        if batch_order == "mixed":
            bor = np.sort(rng.integers(0, n_batches, size=M)).astype(np.int32)  # contiguous batches like real data
            if v % 2 == 1:
                bor = rng.permutation(bor).astype(np.int32)                      # ... and a scrambled one
            bor[:n_batches] = np.arange(n_batches)                                # every batch non-empty
        else:
            # "sorted": every view has contiguous batches (samples grouped by batch, as assemble_model lays them out);
            # "random": every view scrambled.  Every batch non-empty.
            bor = np.sort(np.concatenate([np.arange(n_batches), rng.integers(0, n_batches, size=M - n_batches)]))
            if batch_order == "random":
                bor = rng.permutation(bor)
            bor = bor.astype(np.int32)
        centers_d = rng.standard_normal(n_batches)[:, None] * 0.25
        centers_t = rng.standard_normal(n_batches)[:, None] * 0.25
        bviews.append(dict(start1=s, stop1=e, batch_of_row=bor,
                           logdelta=(centers_d + 0.25 * rng.standard_normal((n_batches, Nv))).astype(np.float32),
                           theta=(centers_t + 0.25 * rng.standard_normal((n_batches, Nv))).astype(np.float32)))
    # data: Z = layers(X'Y) + noise; Bernoulli 1[Z>0]; Poisson counts
    A = X.astype(np.float64).T @ Y.astype(np.float64)
    Z = A * np.exp(logsigma.astype(np.float64))[None, :]
    for b in bviews:
        sl = slice(b["start1"] - 1, b["stop1"])
        Z[:, sl] *= np.exp(b["logdelta"].astype(np.float64))[b["batch_of_row"], :]
    Z += mu.astype(np.float64)[None, :]
    for b in bviews:
        sl = slice(b["start1"] - 1, b["stop1"])
        Z[:, sl] += b["theta"].astype(np.float64)[b["batch_of_row"], :]
    D = Z + noise * rng.standard_normal((M, N))
    for j in range(N):
        if kind_of_col[j] == "bernoulli":
            D[:, j] = (D[:, j] > 0).astype(np.float64)
        elif kind_of_col[j] == "poisson":
            D[:, j] = rng.poisson(np.exp(np.clip(Z[:, j], -5, 3)))
    D = D.astype(np.float32)
    if nan_frac > 0:
        D[rng.random((M, N)) < nan_frac] = np.nan
    col_weight = (0.5 + rng.random(N)).astype(np.float32) if weights else np.ones(N, np.float32)
    if random_init:  # start the fit away from the generating factors
        X = (rng.standard_normal((K, M)) * 0.3).astype(np.float32)
        Y = (rng.standard_normal((K, N)) * 0.3).astype(np.float32)
    p = dict(M=M, N=N, K=K, D=np.asfortranarray(D), X=np.asfortranarray(X), Y=np.asfortranarray(Y),
             logsigma=logsigma, mu=mu, batch_views=bviews, noise_ranges=noise_ranges, noise_kinds=kinds,
             col_weight=col_weight, view_ranges=view_ranges, xreg=[], yreg=[], colreg=None, batchreg=None)
    # regularizers
    if xreg == "l2":
        p["xreg"] = [dict(kind="l2", w=(0.5 + rng.random(K)).astype(np.float32), p=1.0)]
    elif xreg == "group":
        gr = split_ranges(M, n_groups)
        p["xreg"] = [dict(kind="group", start1=[g[0] for g in gr], stop1=[g[1] for g in gr],
                          w=(0.5 + rng.random((len(gr), K))).astype(np.float32), p=1.0)]
    elif xreg == "composite":
        gr = split_ranges(M, n_groups)
        p["xreg"] = [dict(kind="l2", w=(0.5 + rng.random(K)).astype(np.float32), p=0.5),
                     dict(kind="group", start1=[g[0] for g in gr], stop1=[g[1] for g in gr],
                          w=(0.5 + rng.random((len(gr), K))).astype(np.float32), p=0.5)]
    if yreg == "group":
        p["yreg"] = [dict(kind="group", start1=[g[0] for g in noise_ranges], stop1=[g[1] for g in noise_ranges],
                          w=(0.5 + rng.random((len(noise_ranges), K))).astype(np.float32), p=1.0)]
    elif yreg == "ard":
        p["yreg"] = [dict(kind="ard", start1=[g[0] for g in view_ranges], stop1=[g[1] for g in view_ranges],
                          a=np.full(len(view_ranges), 1.001, np.float32),
                          b=np.full(len(view_ranges), 0.001, np.float32), p=1.0)]
    elif yreg == "l2":
        p["yreg"] = [dict(kind="l2", w=(0.5 + rng.random(K)).astype(np.float32), p=1.0)]
    elif yreg == "ard_gap":
        # ARDRegularizer with distinct (alpha, beta) per view range and one view left uncovered (regularizers.jl:546-585
        # loops over its col_ranges only; the library encodes "not regularized" as alpha = -0.5)
        keep = [g for i, g in enumerate(view_ranges) if i != 1 or len(view_ranges) == 1]
        p["yreg"] = [dict(kind="ard", start1=[g[0] for g in keep], stop1=[g[1] for g in keep],
                          a=(1.001 + 0.5 * rng.random(len(keep))).astype(np.float32),
                          b=(0.001 + 0.01 * rng.random(len(keep))).astype(np.float32), p=1.0)]
    elif yreg == "fsard":
        alpha = np.full(N, 1.001, np.float32)
        beta = (0.001 * (0.8 + 2.0 * rng.random((K, N)) * (rng.random((K, N)) < 0.2))).astype(np.float32)
        p["yreg"] = [dict(kind="fsard", alpha=alpha, beta=np.asfortranarray(beta), p=1.0)]
    if layer_regs:
        nr = len(view_ranges)
        p["colreg"] = dict(start1=[g[0] for g in view_ranges], stop1=[g[1] for g in view_ranges],
                           w_logsigma=(0.5 + rng.random(nr)).astype(np.float32),
                           c_logsigma=(0.1 * rng.standard_normal(nr)).astype(np.float32),
                           w_mu=(0.5 + rng.random(nr)).astype(np.float32),
                           c_mu=(0.1 * rng.standard_normal(nr)).astype(np.float32))
        if bviews:
            p["batchreg"] = dict(
                w_logdelta=[(0.5 + rng.random(n_batches)).astype(np.float32) for _ in bviews],
                c_logdelta=[(0.1 * rng.standard_normal(n_batches)).astype(np.float32) for _ in bviews],
                w_theta=[(0.5 + rng.random(n_batches)).astype(np.float32) for _ in bviews],
                c_theta=[(0.1 * rng.standard_normal(n_batches)).astype(np.float32) for _ in bviews])
    return p


def to_oracle(p, precision=64):
    from oracle.pmf_oracle import OracleModel
    noise = [(s, e, k) for (s, e), k in zip(p["noise_ranges"], p["noise_kinds"])]
    return OracleModel(p["D"], p["X"], p["Y"], logsigma=p["logsigma"], mu=p["mu"],
                       batch_views=p["batch_views"] if p["batch_views"] else None,
                       noise=noise, col_weight=p["col_weight"], xreg=p["xreg"], yreg=p["yreg"],
                       colreg=p["colreg"], batchreg=p["batchreg"], precision=precision)


def to_context(p, ctx):
    """Marshals the problem through the C ABI (what the Julia shim's mf_fit! does before ccall(:pmf_fit))."""
    ctx.set_data(p["D"])
    ctx.set_factors(p["X"], p["Y"])
    ctx.set_col_params(p["logsigma"], p["mu"])
    ctx.set_batch_views(p["batch_views"])
    ctx.set_noise(p["noise_ranges"], p["noise_kinds"], p["col_weight"])
    ctx.clear_xreg()
    for t in p["xreg"]:
        _add_term(ctx, "X", t)
    ctx.clear_yreg()
    for t in p["yreg"]:
        _add_term(ctx, "Y", t)
    cr, br = p["colreg"], p["batchreg"]
    if cr is not None or br is not None:
        kw = {}
        if cr is not None:
            kw.update(ranges=list(zip(cr["start1"], cr["stop1"])), w_logsigma=cr["w_logsigma"],
                      c_logsigma=cr["c_logsigma"], w_mu=cr["w_mu"], c_mu=cr["c_mu"])
        if br is not None:
            kw.update(w_logdelta=br["w_logdelta"], c_logdelta=br["c_logdelta"], w_theta=br["w_theta"],
                      c_theta=br["c_theta"])
        ctx.set_layer_regs(**kw)
    else:
        ctx.set_layer_regs()
    return ctx


def _add_term(ctx, which, t):
    if t["kind"] == "l2":
        ctx.add_reg_l2(which, t["w"], t.get("p", 1.0))
    elif t["kind"] == "group":
        ctx.add_reg_group(which, list(zip(t["start1"], t["stop1"])), t["w"], t.get("p", 1.0))
    elif t["kind"] == "ard":
        ctx.add_yreg_ard(list(zip(t["start1"], t["stop1"])), t["a"], t["b"], t.get("p", 1.0))
    elif t["kind"] == "fsard":
        ctx.add_yreg_fsard(t["alpha"], t["beta"], t.get("p", 1.0))
    elif t["kind"] == "l1":
        ctx.add_reg_l1(which, t["w"], t.get("mask"), t.get("p", 1.0))
    else:
        raise ValueError(t["kind"])


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    denom = max(np.max(np.abs(b)), 1e-30)
    return float(np.max(np.abs(a - b)) / denom)


def shard_problem(p, lo, hi):
    """Rows [lo, hi) of the problem as a problem of its own (what one rank of the row-sharded fit holds): D, X and the
    row -> batch maps are sliced, X-regularizer groups (ranges over the GLOBAL rows) are clipped to the shard, everything
    indexed by columns is replicated."""
    import copy
    q = copy.deepcopy(p)
    q["D"] = np.asfortranarray(p["D"][lo:hi])
    q["X"] = np.asfortranarray(p["X"][:, lo:hi])
    q["M"] = hi - lo
    for b in q["batch_views"]:
        b["batch_of_row"] = np.ascontiguousarray(b["batch_of_row"][lo:hi])
    for t in q["xreg"]:
        if t["kind"] == "group":
            s = [max(a, lo + 1) - lo for a in t["start1"]]
            e = [min(b, hi) - lo for b in t["stop1"]]
            keep = [i for i in range(len(s)) if e[i] >= s[i]]
            t["start1"], t["stop1"] = [s[i] for i in keep], [e[i] for i in keep]
            t["w"] = np.asarray(t["w"])[keep]
    return q


# ---- a segment-scaled check for the layer-parameter gradients --------------------------------------------------------
LAYER_TAU = 2e-5


def _batch_views_of(p):
    """(c0, c1, batch_of_row, has a batch, nb, delta, theta, one-hot M x nb) per batch view, in fp64."""
    bvs = []
    for bv in p["batch_views"]:
        bor = np.asarray(bv["batch_of_row"])
        nb = np.asarray(bv["logdelta"]).shape[0]
        bvs.append((bv["start1"] - 1, bv["stop1"], bor, bor >= 0, nb, np.exp(np.asarray(bv["logdelta"], np.float64)),
                    np.asarray(bv["theta"], np.float64), (bor[:, None] == np.arange(nb)[None, :]).astype(np.float64)))
    return bvs


def entry_scales(p, c0=0, c1=None, bvs=None):
    """The per-entry part of the error scales, in fp64, on the columns [c0, c1) of problem `p` (all of them by default).
    z comes from the fp64 forward of DESIGN section 4.3 (restated here, per noise kind): z1 = sigma_j a_ij,
    z = z1 delta_bj + mu_j + theta_bj (delta = 1, theta = 0 for rows with batch -1 and for columns outside every batch
    view), g = w_j (link(z) - y) on observed entries.  Per observed entry

        sG_ij = w_j (|link(z)| + |y| + link'(z) r_ij),   r_ij = sigma_j delta_bj sum_k |X_ki Y_kj| + |mu_j| + |theta_bj|
        sQ_ij = |z1_ij| sG_ij + |g_ij| sigma_j sum_k |X_ki Y_kj|

    (r bounds what the forward rounds, link' carries it into g; the second term of sQ is the rounding of z1 itself).
    Returns M x (c1 - c0) arrays, 0 on unobserved entries: g, sG, sQ, sd = sigma_j delta_bj (on every entry: the factor
    that takes dloss/dz to dloss/d(X'Y)), and "loss", the magnitudes of the loss terms: 0.5 w (z - y)^2 (Gaussian: the loss
    itself), w (softplus(z) + |y z|) (Bernoulli), w (e^z + |y z|) (Poisson) -- the last two cancel term by term.  A problem
    with squared-hinge columns ("noise_thr") takes the same quantities from hinge_ref.entry_scales."""
    if p.get("noise_thr"):
        import hinge_ref
        return hinge_ref.entry_scales(p, c0, c1)
    N = p["D"].shape[1]
    c1 = N if c1 is None else c1
    bvs = _batch_views_of(p) if bvs is None else bvs
    X = np.asarray(p["X"], np.float64)
    Y = np.asarray(p["Y"], np.float64)
    kind = np.zeros(N, np.int8)                                   # 0 normal, 1 bernoulli, 2 poisson
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        kind[s - 1:e] = {"normal": 0, "bernoulli": 1, "poisson": 2}[kd]
    sig = np.exp(np.asarray(p["logsigma"], np.float64))[c0:c1]
    mu = np.asarray(p["mu"], np.float64)[c0:c1]
    w = np.asarray(p["col_weight"], np.float64)[c0:c1]
    kd = kind[c0:c1]
    A = X.T @ Y[:, c0:c1]
    Aabs = np.abs(X).T @ np.abs(Y[:, c0:c1])
    dl = np.ones_like(A)
    th = np.zeros_like(A)
    for s, e, bor, has, nb, delta, theta, onehot in bvs:
        a, b = max(s, c0), min(e, c1)
        if a < b:
            dl[np.ix_(has, np.arange(a - c0, b - c0))] = delta[bor[has]][:, a - s:b - s]
            th[np.ix_(has, np.arange(a - c0, b - c0))] = theta[bor[has]][:, a - s:b - s]
    z1 = A * sig[None, :]
    z = z1 * dl + mu[None, :] + th
    link, dlink = z.copy(), np.ones_like(z)
    bern, pois = kd == 1, kd == 2
    sg = 0.5 * (1.0 + np.tanh(0.5 * z[:, bern]))
    link[:, bern], dlink[:, bern] = sg, sg * (1.0 - sg)
    link[:, pois] = dlink[:, pois] = np.exp(z[:, pois])
    Dc = np.asarray(p["D"][:, c0:c1], np.float64)
    obs = np.isfinite(Dc)
    y = np.where(obs, Dc, 0.0)
    g = np.where(obs, w[None, :] * (link - y), 0.0)
    r = sig[None, :] * Aabs * dl + np.abs(mu)[None, :] + np.abs(th)
    sG = np.where(obs, w[None, :] * (np.abs(link) + np.abs(y) + dlink * r), 0.0)
    sQ = np.abs(z1) * sG + np.abs(g) * sig[None, :] * Aabs
    lm = np.where(kd[None, :] == 0, 0.5 * (z - y) ** 2,
                  np.where(kd[None, :] == 1, np.logaddexp(0.0, z), np.exp(np.minimum(z, 700.0))) + np.abs(y * z))
    return dict(g=g, sG=sG, sQ=sQ, sd=sig[None, :] * dl, delta=dl, loss=np.where(obs, w[None, :] * lm, 0.0))


def layer_scales(p, cols=4096):
    """fp64 error scales of the four layer gradients of problem `p`: the per-(batch, column) sums of the magnitudes a
    kernel rounds on the way to each gradient.  With sG, sQ and delta of entry_scales,

        grad theta[b, j]    ~ sum_{i in b} sG           grad mu[j]       ~ sum_i sG
        grad logdelta[b, j] ~ delta_bj sum_{i in b} sQ  grad logsigma[j] ~ sigma_j sum_i delta_bj sG

    The scales only set tolerances; the reference value of every gradient stays the oracle's.  Also returns g (M x N)
    and, as "loss", the sum of the magnitudes of the loss terms.  Works on blocks of `cols` columns (wide problems)."""
    M, N = p["D"].shape
    bvs = _batch_views_of(p)
    sig_all = np.exp(np.asarray(p["logsigma"], np.float64))
    out = dict(mu=np.zeros(N), logsigma=np.zeros(N), theta=[np.zeros((b[4], b[1] - b[0])) for b in bvs],
               logdelta=[np.zeros((b[4], b[1] - b[0])) for b in bvs], g=np.zeros((M, N)), loss=0.0)
    for c0 in range(0, N, cols):
        c1 = min(N, c0 + cols)
        e = entry_scales(p, c0, c1, bvs)
        sG, sQ = e["sG"], e["sQ"]
        out["loss"] += float(np.sum(e["loss"]))
        out["g"][:, c0:c1] = e["g"]
        out["mu"][c0:c1] = sG.sum(0)
        out["logsigma"][c0:c1] = sig_all[c0:c1] * (e["delta"] * sG).sum(0)
        for v, (s, e_, bor, has, nb, delta, theta, onehot) in enumerate(bvs):   # rows with batch -1: no segment
            a, b = max(s, c0), min(e_, c1)
            if a < b:
                out["theta"][v][:, a - s:b - s] = onehot.T @ sG[:, a - c0:b - c0]
                out["logdelta"][v][:, a - s:b - s] = delta[:, a - s:b - s] * (onehot.T @ sQ[:, a - c0:b - c0])
    return out


def layer_check(p, got, want, tau=LAYER_TAU, tiny=1e-30, scales=None, skip=()):
    """Worst ratio |got - want| / (tau * scale + tiny) over every (batch, column) segment of grad mu, grad logsigma,
    grad theta and grad logdelta (<= 1 passes; `skip` names gradients that are not compared, e.g. frozen layers).
    `got` and `want` are dicts of those arrays (theta and logdelta as per-view lists), `want` normally the fp64 oracle's.

    Unlike rel_err, which divides by the largest entry of a whole array, each segment is held to the rounding of its own
    terms: a (batch, column) sum that loses one row, or gains one of the neighbouring batch, is off by |g_ij|, far more
    than tau * scale unless the segment is large or the row's gradient is negligible.  A sum that cancels (M = 31,
    N = 1) is not held to its tiny result either.  tau = 2e-5 covers sequential f32 sums of a few hundred terms (the f32
    build of the oracle stays below 1/10 of it on the shapes of tests/test_gpu_layer_edges.py)."""
    s = layer_scales(p) if scales is None else scales
    worst = dict()
    for k in ("mu", "logsigma", "theta", "logdelta"):
        if k in skip:
            continue
        gs, ws, ss = (got[k], want[k], s[k]) if k in ("theta", "logdelta") else ([got[k]], [want[k]], [s[k]])
        assert len(gs) == len(ws) == len(ss), k
        r = 0.0
        for a, b, c in zip(gs, ws, ss):
            a = np.asarray(a, np.float64)
            b = np.asarray(b, np.float64)
            assert a.shape == b.shape == c.shape, (k, a.shape, b.shape, c.shape)
            if a.size:
                if not np.isfinite(a).all():
                    return dict(worst, **{k: np.inf})
                r = max(r, float(np.max(np.abs(a - b) / (tau * c + tiny))))
        worst[k] = r
    return worst


# ---- an element-scaled check for the factor gradients ----------------------------------------------------------------
FACTOR_TAU = LAYER_TAU


def factor_scales(p, cols=None):
    """fp64 error scales of the two factor gradients of problem `p`.  gX_ki = sum_j G_ij Y_kj and gY_kj = sum_i G_ij X_ki
    with G_ij = sigma_j delta_bj g_ij; what a kernel rounds on the way to G_ij is bounded by sigma_j delta_bj sG_ij (sG of
    entry_scales: the magnitudes g is formed from, and the forward's through link'), and rounding G_ij itself or the other
    operand is relative to |G_ij| |Y_kj| <= sigma_j delta_bj sG_ij |Y_kj|.  So every element is held to the sum of the
    magnitudes of its own terms:

        X (K x M): sGX[k, i] = sum_j sigma_j delta_ij sG_ij |Y_kj|
        Y (K x N): sGY[k, j] = sum_i sigma_j delta_ij sG_ij |X_ki|

    Works on blocks of `cols` columns (default: about 4M entries per block), so tall problems stay cheap."""
    M, N = p["D"].shape
    Xa = np.abs(np.asarray(p["X"], np.float64))
    Ya = np.abs(np.asarray(p["Y"], np.float64))
    cols = max(32, min(4096, (1 << 22) // max(M, 1))) if cols is None else cols
    bvs = None if p.get("noise_thr") else _batch_views_of(p)
    out = dict(X=np.zeros(Xa.shape), Y=np.zeros(Ya.shape))
    for c0 in range(0, N, cols):
        c1 = min(N, c0 + cols)
        e = entry_scales(p, c0, c1, bvs)
        W = e["sd"] * e["sG"]
        out["X"] += Ya[:, c0:c1] @ W.T
        out["Y"][:, c0:c1] = Xa @ W
    return out


def factor_check(p, got, want, tau=FACTOR_TAU, scales=None):
    """{"X": worst, "Y": worst} over the factor gradients present in `got`: the worst ratio |got - want| / (tau * scale +
    1e-30) over the elements of each (<= 1 passes; a non-finite `got` gives inf).  `want` is normally the fp64 oracle's.

    rel_err divides by the largest entry of the whole array; on mixed problems a few Poisson entries set it, and a
    Gaussian column or a quiet row can be wrong by a third and pass.  Here every element answers for the rounding of its
    own terms.  tau = FACTOR_TAU = LAYER_TAU = 2e-5, not fitted to any device output: the split kernels' gradient products
    run on bf16 hi + mid of both operands, 16 significant bits each, so each operand is rounded by at most 2^-17 and the
    product by 1.5e-5 of sum |G| |X|; the exact kernel's f32 roundings are two orders below
    (tests/test_host_factor_check.py)."""
    s = factor_scales(p) if scales is None else scales
    worst = {}
    for k in ("X", "Y"):
        if k not in got:
            continue
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        assert a.shape == b.shape == s[k].shape, (k, a.shape, b.shape, s[k].shape)
        if not np.isfinite(a).all():
            worst[k] = np.inf
        else:
            worst[k] = float(np.max(np.abs(a - b) / (tau * s[k] + 1e-30))) if a.size else 0.0
    return worst


def factor_worst(p, got, want, tau=FACTOR_TAU, scales=None):
    """One line per gradient present in `got` on its worst element: k, the row (gX) or column (gY), the ratio; for a
    column its noise kind and feature view; for either the 32 x 32 tile (row block, column block) of D whose removal
    would explain most of the deviation, and whether that tile is all-finite (the packed epilogue) or not."""
    s = factor_scales(p) if scales is None else scales
    D = p["D"]
    M, N = D.shape
    X, Y = np.asarray(p["X"], np.float64), np.asarray(p["Y"], np.float64)
    lines = []
    for w in ("X", "Y"):
        if w not in got:
            continue
        a, b = np.asarray(got[w], np.float64), np.asarray(want[w], np.float64)
        ratio = np.where(np.isfinite(a), np.abs(a - b), np.inf) / (tau * s[w] + 1e-30)
        k, n = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        txt = f"g{w}[k={k}, {'row' if w == 'X' else 'column'}={n}]: got {a[k, n]:.6g}, want {b[k, n]:.6g}, " \
              f"ratio {ratio[k, n]:.3g} of tau * scale = {tau * s[w][k, n]:.3g}"
        if w == "X":
            e = entry_scales(p)
            term = e["sd"][n] * e["g"][n] * Y[k]                               # the N terms of gX[k, n]
            part = np.add.reduceat(term, np.arange(0, N, 32))
            tj = int(np.argmin(np.abs(part - (b[k, n] - a[k, n]))))
            ti = n // 32
        else:
            e = entry_scales(p, n, n + 1)
            term = e["sd"][:, 0] * e["g"][:, 0] * X[k]                         # the M terms of gY[k, n]
            part = np.add.reduceat(term, np.arange(0, M, 32))
            ti = int(np.argmin(np.abs(part - (b[k, n] - a[k, n]))))
            tj = n // 32
            kind = next((kd for (s0, e0), kd in zip(p["noise_ranges"], p["noise_kinds"]) if s0 - 1 <= n < e0), "?")
            view = next((v for v, (s0, e0) in enumerate(p.get("view_ranges", [])) if s0 - 1 <= n < e0), None)
            bview = next((v for v, bv in enumerate(p["batch_views"]) if bv["start1"] - 1 <= n < bv["stop1"]), None)
            txt += f"; noise {kind}, view {view}, batch view {bview}"
        tile = D[32 * ti:32 * ti + 32, 32 * tj:32 * tj + 32]
        txt += f"; tile (row block {ti}, column block {tj}) fits a missing tile best and is " \
               f"{'all-finite' if np.isfinite(tile).all() else 'masked'}"
        lines.append(txt)
    return "\n".join(lines)
