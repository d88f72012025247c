"""Helpers of the regularizer + optimizer step tests (k_reg_step<false> / k_reg_step<true> and the code around them): the dense
regularizer terms built in float64 straight from the C ABI's arguments (1-based inclusive ranges, as tests/problems.py
carries them; none of the library's expanders is called), the closed formulas of the regularizer value / gradient and of
the AdaGrad / Adam step in float64, a float32 twin of both (the same formulas, every operation in np.float32 and in the
kernel's order: it sets the tolerances, it is never the expected value), the termination rule of pmf_fit applied to a
loss trace, the error measures, and the case tables that tests/test_gpu_step_edges.py runs on the device and
tests/test_step_cases.py guards on the CPU.  Plain numpy; the package is not imported."""
import copy

import numpy as np

from problems import make_problem, split_ranges

F = np.float32
D = np.float64
TINY = 1e-30

# ---- tolerances ---------------------------------------------------------------------------------------------------------
# Limits of the scaled deviations below (dev_param, dev_acc, dev_mom, dev_value): 4 x the worst deviation of the float32
# twin from the float64 restatement on the same float32 inputs, over every case of the tables, both optimizers, five
# consecutive steps (tests/test_step_cases.py measures it again and asserts that 4 x the twin still fits).  The factor 4
# covers the device's logf / sqrtf / division against numpy's and fused multiply-adds.  Adam's parameter has two limits:
# from the second step on 1 - beta2^t is formed from a running float32 power (an ulp of ~1 under a difference of ~0.002:
# 3e-5 of c2, half of that in dp), which the twin reproduces; the first step has 1 - beta exactly.
#                               twin's worst
P_TOL = {"adagrad": 8.0e-7,     # 1.95e-07   stepped parameter, per |p| + |dp| + |d(dp)/dg| mag (dev_param)
         "adam_first": 3.7e-7,  # 9.11e-08   ... Adam, t = 1
         "adam": 2.9e-5}        # 7.00e-06   ... Adam, t > 1
ACC_TOL = 2.3e-6                # 5.50e-07   acc (AdaGrad's accumulator, Adam's second moment), per mag^2 + |acc_prev|
MOM_TOL = 4.0e-7                # 9.74e-08   Adam's first moment, per |m_prev| + mag
VAL_TOL = 1.5e-7                # 3.59e-08   regularizer value, per sum of the magnitudes of its per-element terms
TWIN_MARGIN = 4.0


def p_tol(opt, t):
    return P_TOL["adagrad"] if opt == "adagrad" else P_TOL["adam_first" if t == 1 else "adam"]


REG_SLOTS = 1024     # workgroups (= loss partials) of an X / Y step; a layer parameter gets a quarter
PARAMS = ("X", "Y", "logsigma", "mu", "logdelta", "theta")
LAYER_BIT = {"logsigma": 1, "logdelta": 2, "mu": 4, "theta": 8}   # layer l <-> bit l - 1 of frozen_layers / frozen_regs


def f32r(x):
    """A host scalar as the C ABI carries it (float), back in double."""
    return float(np.float32(x))


# ---- dense terms ----------------------------------------------------------------------------------------------------------
def _in_range(n, s1, e1):
    i = np.arange(1, n + 1)
    return (i >= s1) & (i <= e1)


def quad_weights(terms, K, n, R=D):
    """wq[k, i] = sum_terms p_t sum_{g contains i} w_t[g, k]; overlaps add, uncovered rows / columns get 0.  None without
    a quadratic term.  R = float32: in the order k_expand_group accumulates (groups in order, then wq += p * add)."""
    wq = None
    for t in terms:
        if t["kind"] not in ("l2", "group"):
            continue
        if wq is None:
            wq = np.zeros((K, n), R)
        if t["kind"] == "l2":
            ranges, w = [(1, n)], np.asarray(t["w"], F).reshape(1, K)
        else:
            ranges, w = list(zip(t["start1"], t["stop1"])), np.asarray(t["w"], F).reshape(len(t["start1"]), K)
        add = np.zeros((K, n), R)
        for g, (s1, e1) in enumerate(ranges):
            add[:, _in_range(n, s1, e1)] += w[g].astype(R)[:, None]
        wq = wq + R(F(t.get("p", 1.0))) * add
    return wq


def ard_dense(terms, K, N, R=D):
    """(scale, alpha[N], beta[K x N]) of the one ARD-type term, or None.  ARD: alpha, beta per range, columns in no range
    are unregularized (alpha = -0.5 makes the factor 0.5 + alpha vanish).  FeatureSetARD: alpha[N], beta[K x N]."""
    for t in terms:
        if t["kind"] == "ard":
            alpha, beta = np.full(N, -0.5, R), np.ones((K, N), R)
            for r, (s1, e1) in enumerate(zip(t["start1"], t["stop1"])):
                sel = _in_range(N, s1, e1)
                alpha[sel] = R(np.asarray(t["a"], F).ravel()[r])
                beta[:, sel] = R(np.asarray(t["b"], F).ravel()[r])
            return R(F(t.get("p", 1.0))), alpha, beta
        if t["kind"] == "fsard":
            return R(F(t.get("p", 1.0))), np.asarray(t["alpha"], F).astype(R), np.asarray(t["beta"], F).astype(R)
    return None


def l1_dense(terms, K, n, R=D):
    """wl1[k, j] = sum_terms p w_k m_kj (L1Regularizer: no mask; SelectiveL1Reg: mask K x n).  None without an L1 term."""
    wl1 = None
    for t in terms:
        if t["kind"] != "l1":
            continue
        if wl1 is None:
            wl1 = np.zeros((K, n), R)
        m = np.ones((K, n), bool) if t.get("mask") is None else np.asarray(t["mask"]).astype(bool)
        wl1 = wl1 + np.where(m, R(F(t.get("p", 1.0))) * np.asarray(t["w"], F).astype(R)[:, None], R(0))
    return wl1


def colparam_dense(cr, N, name, R=D):
    """ColParamReg of `name` (logsigma / mu): per-range weight and centre, the last range that holds a column wins,
    uncovered columns get weight 0."""
    w, c = np.zeros(N, R), np.zeros(N, R)
    for r, (s1, e1) in enumerate(zip(cr["start1"], cr["stop1"])):
        sel = _in_range(N, s1, e1)
        w[sel] = R(np.asarray(cr["w_" + name], F)[r])
        c[sel] = R(np.asarray(cr["c_" + name], F)[r])
    return w, c


def batchreg_dense(br, views, name, v, R=D):
    """BatchArrayReg of `name` (logdelta / theta), view v: per (view, batch) weight and centre over the view's columns."""
    nb, Nv = np.asarray(views[v][name]).shape
    w = np.repeat(np.asarray(br["w_" + name][v], F).astype(R)[:, None], Nv, axis=1)
    c = np.repeat(np.asarray(br["c_" + name][v], F).astype(R)[:, None], Nv, axis=1)
    assert w.shape == (nb, Nv)
    return w, c


def param_terms(p, which, view=0, R=D):
    """The dense regularizer terms of one parameter of problem p: dict(wq, cq, ard, wl1), each possibly None."""
    K = p["K"]
    out = dict(wq=None, cq=None, ard=None, wl1=None)
    if which in ("X", "Y"):
        n = p["M"] if which == "X" else p["N"]
        terms = p["xreg"] if which == "X" else p["yreg"]
        out["wq"] = quad_weights(terms, K, n, R)
        out["wl1"] = l1_dense(terms, K, n, R)
        if which == "Y":
            out["ard"] = ard_dense(terms, K, n, R)
    elif which in ("logsigma", "mu"):
        if p["colreg"] is not None:
            out["wq"], out["cq"] = colparam_dense(p["colreg"], p["N"], which, R)
    elif p["batchreg"] is not None:
        out["wq"], out["cq"] = batchreg_dense(p["batchreg"], p["batch_views"], which, view, R)
    return out


NO_TERMS = dict(wq=None, cq=None, ard=None, wl1=None)


# ---- the formulas ---------------------------------------------------------------------------------------------------------
def _value_and_grad(pv, terms, g0, R):
    pv = np.asarray(pv).astype(R)
    g = np.zeros_like(pv) if g0 is None else np.asarray(g0).astype(R)
    mag = np.abs(g).astype(D)
    value, vmag = 0.0, 0.0
    half, one = R(0.5), R(1)
    if terms["wq"] is not None:                          # 0.5 wq (p - c)^2, gradient wq (p - c)
        d = pv - terms["cq"] if terms["cq"] is not None else pv
        gr = terms["wq"] * d
        v = 0.5 * (gr * d).astype(D)
        value += float(v.sum()); vmag += float(np.abs(v).sum())
        g = g + gr
        mag += np.abs(gr)
    if terms["ard"] is not None:                         # s (0.5 + a_j) log(1 + p^2 / (2 beta)), gradient s (a_j + 0.5) p / (b beta)
        s, al, be = terms["ard"]
        b = one + (half / be) * (pv * pv)
        v = (s * (half + al)[None, :] * np.log(b)).astype(D)
        value += float(v.sum()); vmag += float(np.abs(v).sum())
        gr = s * ((al + half)[None, :] * pv / (b * be))
        g = g + gr
        mag += np.abs(gr)
    if terms["wl1"] is not None:                         # w |p|, gradient w sign(p) with sign(0) = 0
        w = terms["wl1"]
        v = (w * np.abs(pv)).astype(D)
        value += float(v.sum()); vmag += float(np.abs(v).sum())
        gr = np.where(pv > 0, w, np.where(pv < 0, -w, R(0)))
        g = g + gr
        mag += np.abs(gr)
    assert g.dtype == R
    return dict(value=value, vmag=vmag, grad=g, mag=mag)


def reg_value_and_grad(pv, terms, g0=None):
    """float64.  value: the regularizer's value; grad: g0 (the data gradient; 0 if None) plus the terms' gradients; mag:
    |g0| + the sum of the magnitudes of the gradient terms, per element; vmag: the sum of the magnitudes of the
    per-element values."""
    return _value_and_grad(pv, terms, g0, D)


def reg_value_and_grad_f32(pv, terms, g0=None):
    """The float32 twin (terms from param_terms(..., R=np.float32)): per-element values in float32, summed in float64."""
    return _value_and_grad(pv, terms, g0, F)


def _step(pv, g, acc, mom, opt, lr, eps, b1, b2, t, R):
    pv, g, acc, mom = (np.asarray(a).astype(R) for a in (pv, g, acc, mom))
    lr, eps, b1, b2 = R(F(lr)), R(F(eps)), R(F(b1)), R(F(b2))
    one = R(1)
    if opt == "adagrad":                                 # acc starts at eps
        acc = acc + g * g
        return pv - g * (lr / (np.sqrt(acc) + eps)), acc, mom
    assert opt == "adam" and t >= 1                      # both moments start at 0; t = steps taken of this parameter
    bp1, bp2 = b1, b2
    for _ in range(int(t) - 1):                          # (the running powers, as the library keeps them)
        bp1, bp2 = bp1 * b1, bp2 * b2
    c1, c2 = one - bp1, one - bp2
    m = b1 * mom + (one - b1) * g
    v = b2 * acc + (one - b2) * g * g
    return pv - m / c1 / (np.sqrt(v / c2) + eps) * lr, v, m


def step(pv, g_total, acc, mom, opt, lr, eps, b1, b2, t):
    """float64: (p, acc, mom) after one step.  AdaGrad: acc += g^2; p -= lr g / (sqrt(acc) + eps).  Adam: m = b1 m +
    (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)."""
    out = _step(pv, g_total, acc, mom, opt, lr, eps, b1, b2, t, D)
    assert out[0].dtype == D
    return out


def step_f32(pv, g_total, acc, mom, opt, lr, eps, b1, b2, t):
    out = _step(pv, g_total, acc, mom, opt, lr, eps, b1, b2, t, F)
    assert out[0].dtype == F
    return out


def fresh_state(shape, opt, eps, R=F):
    return (np.full(shape, R(F(eps)) if opt == "adagrad" else R(0), R), np.zeros(shape, R))


def expected_step(p, which, pv, g_data, acc, mom, opt_kw, t, view=0, use_reg=True, twin=False):
    """What one step of parameter `which` must give from the device's own inputs.  Returns the dict of
    reg_value_and_grad plus p, acc, mom after the step.  opt_kw: dict(kind, lr, eps, beta1, beta2)."""
    R = F if twin else D
    terms = param_terms(p, which, view, R) if use_reg else NO_TERMS
    r = _value_and_grad(pv, terms, g_data, R)
    r["sens"] = step_sensitivity(np.asarray(r["grad"], D), acc, mom, opt_kw, t)
    r["p"], r["acc"], r["mom"] = _step(pv, r["grad"], acc, mom, opt_kw["kind"], opt_kw["lr"], opt_kw["eps"],
                                       opt_kw["beta1"], opt_kw["beta2"], t, R)
    return r


# ---- error measures -------------------------------------------------------------------------------------------------------
def _worst(err, scale):
    err, scale = np.asarray(err, D), np.asarray(scale, D)
    if not np.isfinite(err).all():
        return np.inf
    return float(np.max(err / (scale + TINY))) if err.size else 0.0


def step_sensitivity(g, acc_prev, mom_prev, opt_kw, t):
    """|d(dp) / dg| of one step in float64, as a sum of magnitudes.  AdaGrad: dp = lr g / (s + eps), s = sqrt(A + g^2):
    d(dp)/dg = lr (A / s + eps) / (s + eps)^2.  Adam: dp = lr (m / c1) / (r + eps), r = sqrt(v / c2):
    |d(dp)/dg| <= lr ((1 - b1) / c1 / (r + eps) + |m / c1| (1 - b2) |g| / (c2 r) / (r + eps)^2)."""
    g, A, m0 = (np.asarray(a, D) for a in (g, acc_prev, mom_prev))
    lr, eps, b1, b2 = (D(F(opt_kw[k])) for k in ("lr", "eps", "beta1", "beta2"))
    if opt_kw["kind"] == "adagrad":
        s = np.sqrt(A + g * g)
        return lr * (A / (s + TINY) + eps) / (s + eps) ** 2
    c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    m = b1 * m0 + (1.0 - b1) * g
    r = np.sqrt((b2 * A + (1.0 - b2) * g * g) / c2)
    return lr * ((1.0 - b1) / c1 / (r + eps) + np.abs(m / c1) * (1.0 - b2) * np.abs(g) / (c2 * (r + TINY)) / (r + eps) ** 2)


def dev_param(got, ref, p_prev, sens=0.0, mag=0.0):
    """Worst |got - ref| per |p| + |dp| + |d(dp)/dg| mag over every element.  The last term is what the step makes of the
    rounding of the summed gradient (mag = |g_data| + sum |g_term|): where the terms cancel, g is known to an ulp of mag,
    not of itself, and dp = lr g / (sqrt(acc) + eps) passes that on amplified by up to lr / sqrt(eps) -- without it the
    float32 twin itself is off by 2.4e-4 of |p| + |dp| on the first AdaGrad step of the 65537-element cases.  Where
    nothing cancels the term is at most |dp|."""
    ref, p_prev = np.asarray(ref, D), np.asarray(p_prev, D)
    return _worst(np.abs(np.asarray(got, D) - ref),
                  np.abs(p_prev) + np.abs(ref - p_prev) + np.asarray(sens, D) * np.asarray(mag, D))


def dev_acc(got, ref, acc_prev, mag):
    return _worst(np.abs(np.asarray(got, D) - np.asarray(ref, D)), np.asarray(mag, D) ** 2 + np.abs(np.asarray(acc_prev, D)))


def dev_mom(got, ref, mom_prev, mag):
    return _worst(np.abs(np.asarray(got, D) - np.asarray(ref, D)), np.abs(np.asarray(mom_prev, D)) + np.asarray(mag, D))


def dev_value(got, ref, vmag):
    return abs(got - ref) / (vmag + TINY) if np.isfinite(got) else np.inf


# ---- the termination rule of pmf_fit ------------------------------------------------------------------------------------
def stop_rule(trace, abs_tol, rel_tol, tol_max_iters=3):
    """MF.fit!'s rule on a loss trace (one entry per epoch that would run): (term_code, epochs run).  A non-finite loss
    stops with "nonfinite"; an increase with "loss_increase"; otherwise |d| < abs_tol counts as "abs_tol", failing that
    |d / loss| < rel_tol as "rel_tol"; the counter resets on an epoch that meets neither; the fit stops when the counter
    reaches tol_max_iters, with the code of the epoch that filled it."""
    count, prev = 0, 0.0
    for n, loss in enumerate(trace, 1):
        if not np.isfinite(loss):
            return "nonfinite", n
        if n > 1:
            diff = prev - loss
            if diff < 0:
                return "loss_increase", n
            which = "abs_tol" if abs(diff) < abs_tol else "rel_tol" if abs(diff / loss) < rel_tol else None
            if which is not None:
                count += 1
                if count >= tol_max_iters:
                    return which, n
            else:
                count = 0
        prev = loss
    return "max_epochs", len(trace)


# ---- chunk geometry of pmf_fit (column tiles of 32, chunk s = tiles [n_ct s / S, n_ct (s + 1) / S)) --------------------
def chunk_column_edges(N, S):
    n_ct = (N + 31) // 32
    return [min(N, 32 * (n_ct * s // S)) for s in range(S + 1)]


# ---- the case tables --------------------------------------------------------------------------------------------------------
# A case: problem = keyword arguments of make_problem; xreg / yreg = term specs ("l2", p) | ("group", ranges, p) |
# ("ard", ranges, p) | ("fsard", p) | ("l1", p) | ("sl1", p); colreg = ColParamReg ranges; views = (start1, stop1, nb) per
# batch view (with layer regularizers); oracle = False: a term or a convention the C oracle does not have (L1; its
# ColParamReg adds overlapping ranges where the library takes the last).  Every p is exact in float32.
_BASE = dict(nan_frac=0.05, weights=True, random_init=True, scale=0.6)
_SMALL = dict(_BASE, M=40, N=50)


def _third(n):
    return split_ranges(n, 3)


K_EDGES = {
    f"K{K}": dict(problem=dict(_SMALL, K=K, seed=100 + K, bernoulli_frac=0.2),
                  xreg=[("l2", 0.5), ("group", _third(40), 0.5)], yreg=[("ard", [(1, 16), (34, 50)], 1.0)])
    for K in (1, 31, 32, 33, 64, 65, 100, 128)
}

# Kp * n around REG_SLOTS * 256 (K = 24 pads to Kp = 32: 8192 rows / columns fill 1024 workgroups exactly)
SIZE_EDGES = {}
for _w, _nm in (("X", "M"), ("Y", "N")):
    for _n in (8191, 8192, 8193):
        _pr = dict(_BASE, M=40, N=40, K=24, seed=200 + _n)
        _pr[_nm] = _n
        SIZE_EDGES[f"{_w}_{_n}"] = dict(problem=_pr, xreg=[("group", [(1, 20), (15, _pr["M"])], 0.5)],
                                        yreg=[("l2", 1.0), ("ard", [(2, _pr["N"] - 1)], 1.0)])

# the same around (REG_SLOTS / 4) * 256 = 65536 for mu / logsigma (N) and for theta / logdelta (nb * N_v, nb = 8)
LAYER_SIZE_EDGES = {}
for _n in (65535, 65536, 65537):
    LAYER_SIZE_EDGES[f"mu_{_n}"] = dict(problem=dict(_BASE, M=32, N=_n, K=4, seed=300, col_params=True), layers=True,
                                        colreg=[(1, 30000), (30001, _n - 2)], xreg=[], yreg=[("l2", 1.0)])
for _n in (8191, 8192, 8193):
    LAYER_SIZE_EDGES[f"theta_{_n}"] = dict(problem=dict(_BASE, M=32, N=_n, K=4, seed=301, col_params=True), layers=True,
                                           colreg=[(1, _n)], views=[(1, _n, 8)], xreg=[], yreg=[("l2", 1.0)])

RANGE_EDGES = {
    # groups of one row; a group ending at row 1, a group starting at row n
    "x_one_row_groups": dict(problem=dict(_SMALL, K=24, seed=401), xreg=[("group", [(1, 1), (7, 7), (40, 40)], 1.0)], yreg=[]),
    "y_one_column_groups": dict(problem=dict(_SMALL, K=24, seed=402), xreg=[], yreg=[("group", [(1, 1), (33, 33), (50, 50)], 1.0)]),
    # two overlapping groups, an uncovered gap at each end
    "x_overlap_gaps": dict(problem=dict(_SMALL, K=24, seed=403), xreg=[("group", [(3, 20), (15, 30)], 1.0)], yreg=[]),
    "y_overlap_gaps": dict(problem=dict(_SMALL, K=24, seed=404), xreg=[], yreg=[("group", [(2, 33), (32, 47)], 1.0)]),
    # two and three quadratic terms with different p on one parameter
    "x_two_quadratic": dict(problem=dict(_SMALL, K=24, seed=405), xreg=[("l2", 0.5), ("group", _third(40), 2.0)], yreg=[]),
    "y_three_quadratic": dict(problem=dict(_SMALL, K=24, seed=406), xreg=[],
                              yreg=[("l2", 0.5), ("group", [(1, 25), (26, 50)], 1.5), ("group", [(10, 40), (30, 45)], 0.25)]),
    # ARD ranges over views 2 and 4 of 5: the first, the middle and the last view uncovered
    "ard_uncovered_first_middle_last": dict(problem=dict(_SMALL, K=24, seed=407), xreg=[], yreg=[("ard", [(11, 20), (31, 40)], 1.0)]),
    "ard_one_column": dict(problem=dict(_SMALL, K=24, seed=408), xreg=[], yreg=[("ard", [(1, 1), (32, 32), (33, 49)], 1.0)]),
    # ColParamReg ranges that overlap (the last wins) and that leave columns uncovered
    "colreg_overlap_uncovered": dict(problem=dict(_SMALL, K=24, seed=409, col_params=True), layers=True, oracle=False,
                                     colreg=[(3, 30), (20, 41), (25, 28)], xreg=[], yreg=[]),
    # batch views with 1 and with 255 batches
    "batches_1_and_255": dict(problem=dict(_BASE, M=300, N=50, K=24, seed=410, col_params=True), layers=True,
                              colreg=[(1, 25), (26, 50)], views=[(1, 20, 1), (21, 50, 255)], xreg=[], yreg=[]),
}

TERM_MIXES = {
    "y_l2_group_ard": dict(problem=dict(_SMALL, K=24, seed=501), xreg=[],
                           yreg=[("l2", 0.5), ("group", [(1, 30), (20, 50)], 1.0), ("ard", [(1, 20), (31, 50)], 0.5)]),
    "y_group_fsard": dict(problem=dict(_SMALL, K=24, seed=502), xreg=[], yreg=[("group", _third(50), 1.0), ("fsard", 1.0)]),
    "x_group_l1": dict(problem=dict(_SMALL, K=24, seed=503), oracle=False, xreg=[("group", _third(40), 1.0), ("l1", 0.5)], yreg=[]),
    "y_fsard_selective_l1": dict(problem=dict(_SMALL, K=24, seed=504), oracle=False, xreg=[], yreg=[("fsard", 1.0), ("sl1", 2.0)]),
    "quadratic_p_zero_and_negative": dict(problem=dict(_SMALL, K=24, seed=505), xreg=[("l2", 0.0), ("group", _third(40), -0.5)],
                                          yreg=[("group", _third(50), 0.0), ("l2", -0.25)]),
}

TABLES = dict(K_EDGES=K_EDGES, SIZE_EDGES=SIZE_EDGES, LAYER_SIZE_EDGES=LAYER_SIZE_EDGES, RANGE_EDGES=RANGE_EDGES,
              TERM_MIXES=TERM_MIXES)
ALL_CASES = [(t, n) for t, tab in TABLES.items() for n in tab]
OPT_KW = dict(adagrad=dict(kind="adagrad", lr=0.05, eps=1e-8, beta1=0.9, beta2=0.999),
              adam=dict(kind="adam", lr=0.01, eps=1e-8, beta1=0.9, beta2=0.999))


def _term(rng, spec, K, n):
    kind = spec[0]
    if kind == "l2":
        return dict(kind="l2", w=(0.5 + rng.random(K)).astype(F), p=spec[1])
    if kind == "group":
        r = spec[1]
        return dict(kind="group", start1=[a for a, _ in r], stop1=[b for _, b in r],
                    w=(0.5 + rng.random((len(r), K))).astype(F), p=spec[2])
    if kind == "ard":
        r = spec[1]
        return dict(kind="ard", start1=[a for a, _ in r], stop1=[b for _, b in r],
                    a=(1.001 + 0.5 * rng.random(len(r))).astype(F), b=(0.001 + 0.01 * rng.random(len(r))).astype(F), p=spec[2])
    if kind == "fsard":
        beta = (0.001 * (0.8 + 2.0 * rng.random((K, n)) * (rng.random((K, n)) < 0.2))).astype(F)
        return dict(kind="fsard", alpha=(1.001 + 0.5 * rng.random(n)).astype(F), beta=np.asfortranarray(beta), p=spec[1])
    if kind in ("l1", "sl1"):
        mask = np.asfortranarray(rng.random((K, n)) < 0.4) if kind == "sl1" else None
        return dict(kind="l1", w=(0.05 + 0.1 * rng.random(K)).astype(F), mask=mask, p=spec[1])
    raise ValueError(kind)


def build_case(table, name):
    """The problem of one case (a dict as tests/problems.py makes them, plus "layers": the layer parameters train too,
    and "oracle_ok")."""
    spec = TABLES[table][name]
    p = make_problem(**spec["problem"])
    rng = np.random.default_rng(spec["problem"]["seed"] + 7919)
    M, N, K = p["M"], p["N"], p["K"]
    p["xreg"] = [_term(rng, s, K, M) for s in spec["xreg"]]
    p["yreg"] = [_term(rng, s, K, N) for s in spec["yreg"]]
    p["layers"] = bool(spec.get("layers", False))
    p["oracle_ok"] = bool(spec.get("oracle", True))
    if spec.get("views"):
        views = []
        for s1, e1, nb in spec["views"]:
            bor = rng.permutation(np.concatenate([np.arange(nb), rng.integers(0, nb, size=M - nb)])).astype(np.int32)
            views.append(dict(start1=s1, stop1=e1, batch_of_row=bor,
                              logdelta=(0.25 * rng.standard_normal((nb, e1 - s1 + 1))).astype(F),
                              theta=(0.25 * rng.standard_normal((nb, e1 - s1 + 1))).astype(F)))
        p["batch_views"] = views
        nbs = [v[2] for v in spec["views"]]
        p["batchreg"] = {k + "_" + nm: [((0.5 + rng.random(nb)) if k == "w" else 0.1 * rng.standard_normal(nb)).astype(F)
                                        for nb in nbs] for k in ("w", "c") for nm in ("logdelta", "theta")}
    if spec.get("colreg"):
        r = spec["colreg"]
        p["colreg"] = dict(start1=[a for a, _ in r], stop1=[b for _, b in r],
                           **{k + "_" + nm: ((0.5 + rng.random(len(r))) if k == "w" else 0.1 * rng.standard_normal(len(r))).astype(F)
                              for k in ("w", "c") for nm in ("logsigma", "mu")})
    # a few exact zeros: sign(0) = 0 for L1, and p^2 = 0 for the ARD terms
    p["X"][0, ::7] = 0.0
    p["Y"][0, ::5] = 0.0
    return p


def case_params(p):
    """(name, view) of every parameter a case steps: X, Y, and with layers mu, logsigma and per view logdelta, theta."""
    out = [("X", 0), ("Y", 0)]
    if p["layers"]:
        out += [("logsigma", 0), ("mu", 0)]
        for v in range(len(p["batch_views"])):
            out += [("logdelta", v), ("theta", v)]
    return out


def param_value(p, which, view=0):
    if which in ("X", "Y", "logsigma", "mu"):
        return p[which]
    return p["batch_views"][view][which]


def without_regs(p):
    q = copy.copy(p)
    q["xreg"], q["yreg"], q["colreg"], q["batchreg"] = [], [], None, None
    return q
