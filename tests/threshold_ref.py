"""The trainable squared-hinge thresholds restated in float64 numpy, on top of tests/hinge_ref.py (include/pmf_hip_thresholds.h,
DESIGN.md section 2, Deviation 5).

    g_t[m][j] = sum_i w_j (a_ij [c_ij = m + 1] - b_ij [c_ij = m])      m = 0..2, over the observed entries; 0 for an infinite t_m
    G[r][m]   = sum_{j in range r} g_t[m][j]                            one group per noise range of kind 3

Joint epoch: data-term gradients of X and Y (hinge_ref.reference) and G at the same parameters, then one step of each with
step_ref.step's closed forms (no regularizer here), thresholds included; infinite thresholds are not stepped; afterwards, for
m = 0, 1, if both are finite and t_{m+1} < t_m then t_{m+1} = t_m.  Initialisation from class counts: p_c = (n_c + 1) /
sum (n_c + 1) over the allowed classes, every finite t_m = inv_logistic(sum_{allowed c <= m} p_c), inv_logistic(x) =
log(0.5 + 0.99 (x / (1 - x) - 0.5)).

Error scale of a gradient: the sum of hinge_ref.entry_scales(p)["sG"] over the entries that contribute to that threshold;
tolerance LAYER_TAU (tests/problems.py).  Plain numpy; the package is not imported here."""
import copy

import numpy as np

import hinge_ref as hr
import step_ref as sr

INF = np.inf


def groups_of(p):
    """[(start1, stop1)] of the noise ranges of kind 3, in order."""
    return [tuple(r) for r, kd in zip(p["noise_ranges"], p["noise_kinds"]) if (hr.KIND[kd] if isinstance(kd, str) else int(kd)) == 3]


def group_thresholds(p):
    """(groups, 3) float64: the triple of every group."""
    t = hr.thresholds_of(p)
    return np.array([t[s - 1] for s, _ in groups_of(p)], np.float64).reshape(-1, 3)


def _entry_terms(p, fault=None):
    """Per entry, masked by observation: wa = w a, wb = w b, class c, and whether the entry is of a kind-3 column."""
    ref = hr.reference(p, "off_by_one" if fault == "off_by_one" else None) if fault else hr.reference_of(p)
    w = np.asarray(p["col_weight"], np.float64)
    obs = np.isfinite(p["D"])
    y = np.where(obs, np.asarray(p["D"], np.float64), 0.0)
    c = np.clip(hr.hinge_class(y) + (1 if fault == "off_by_one" else 0), 0, 3)
    a, b = ref["a"], ref["b"]
    if fault == "swap_ab":
        a, b = b, a
    if fault == "drop_ragged":
        obs = obs & (np.arange(p["M"]) < (p["M"] // 32) * 32)[:, None]
    k3 = (hr.kinds_of(p) == 3)[None, :]
    use = obs & k3
    return np.where(use, w[None, :] * a, 0.0), np.where(use, w[None, :] * b, 0.0), c, use


def col_grad(p, fault=None):
    """(N, 3) float64: g_t[m][j] at [j, m]; NaN for the columns of the other kinds.  fault: None, or one of the mutants
    "off_by_one", "swap_ab", "neighbour" (the first two differing kind-3 ranges exchange their triples), "drop_ragged"."""
    if fault == "neighbour":
        return col_grad(hr.swapped_thresholds(p))
    wa, wb, c, _ = _entry_terms(p, fault)
    t = hr.thresholds_of(p)
    g = np.full((p["N"], 3), np.nan)
    k3 = hr.kinds_of(p) == 3
    for m in range(3):
        gm = (wa * (c == m + 1)).sum(0) - (wb * (c == m)).sum(0)
        g[k3, m] = np.where(np.isfinite(t[k3, m]), gm[k3], 0.0)
    return g


def col_scale(p):
    """(N, 3): the sum of entry_scales(p)["sG"] over the entries that contribute to threshold m of column j."""
    sG = hr.entry_scales(p)["sG"]
    wa, wb, c, use = _entry_terms(p)
    s = np.zeros((p["N"], 3))
    for m in range(3):                                   # (an entry contributes where its term is not zero)
        s[:, m] = (np.where(use & (((c == m) & (wb > 0)) | ((c == m + 1) & (wa > 0))), sG, 0.0)).sum(0)
    return s


def group_sum(p, per_col):
    """(groups, 3): the columns of every group added up (NaN columns do not occur inside a group)."""
    return np.array([per_col[s - 1:e].sum(0) for s, e in groups_of(p)], np.float64).reshape(-1, 3)


def group_grad(p, fault=None):
    return group_sum(p, col_grad(p, fault))


def group_scale(p):
    return group_sum(p, col_scale(p))


def clamp(t):
    """Order restored after a step: for m = 0, 1, if both are finite and t_{m+1} < t_m then t_{m+1} = t_m."""
    t = np.array(t, np.float64)
    for m in range(2):
        bad = np.isfinite(t[..., m]) & np.isfinite(t[..., m + 1]) & (t[..., m + 1] < t[..., m])
        t[..., m + 1] = np.where(bad, t[..., m], t[..., m + 1])
    return t


def with_thresholds(p, tg):
    """A copy of the problem whose kind-3 ranges hold the triples tg (groups, 3)."""
    q = copy.copy(p)
    thr, k = list(p.get("noise_thr") or [None] * len(p["noise_ranges"])), 0
    for i, kd in enumerate(p["noise_kinds"]):
        if (hr.KIND[kd] if isinstance(kd, str) else int(kd)) == 3:
            thr[i] = tuple(float(x) for x in tg[k])
            k += 1
    q["noise_thr"] = thr
    return q


def fresh_state(p, opt_kw):
    n = len(groups_of(p))
    z = lambda shape: sr.fresh_state(shape, opt_kw["kind"], opt_kw["eps"], np.float64)
    return dict(X=z(np.shape(p["X"])), Y=z(np.shape(p["Y"])), T=z((n, 3)))


def threshold_step(tg, G, acc, mom, opt_kw, t, do_clamp=True):
    """One step of the triples tg from the group gradients G: (unclamped, new, acc, mom); infinite thresholds and their state stay."""
    fin = np.isfinite(tg)
    safe = np.where(fin, tg, 0.0)
    pn, an, mn = sr.step(safe, np.where(fin, G, 0.0), acc, mom, opt_kw["kind"], opt_kw["lr"], opt_kw["eps"], opt_kw["beta1"],
                         opt_kw["beta2"], t)
    raw = np.where(fin, pn, tg)
    return raw, (clamp(raw) if do_clamp else raw), np.where(fin, an, acc), np.where(fin, mn, mom)


def joint_epoch(p, state, opt_kw, t, train_xy=True):
    """One epoch of X, Y and the thresholds together at the parameters of p.  Returns (q, state', info): the stepped problem,
    the stepped optimizer state and dict(loss, G, raw) -- the epoch's data loss, the group gradients it stepped from and the
    thresholds before the clamp."""
    ref = hr.reference(p)
    G = group_grad(p)
    tg = group_thresholds(p)
    raw, tn, ta, tm = threshold_step(tg, G, *state["T"], opt_kw, t)
    q = with_thresholds(p, tn)
    new = dict(T=(ta, tm), X=state["X"], Y=state["Y"])
    if train_xy:
        for w in ("X", "Y"):
            pn, an, mn = sr.step(np.asarray(p[w], np.float64), ref[w], *state[w], opt_kw["kind"], opt_kw["lr"], opt_kw["eps"],
                                 opt_kw["beta1"], opt_kw["beta2"], t)
            q[w] = pn
            new[w] = (an, mn)
    return q, new, dict(loss=ref["data_loss"], G=G, raw=raw)


# ---- initialisation from class counts ----------------------------------------------------------------------------------
def inv_logistic(x):
    return np.log(0.5 + 0.99 * (x / (1.0 - x) - 0.5))


def class_counts(p, ranges):
    """(ranges, 4) int64: the observed entries of class c in the columns of every 1-based inclusive range."""
    D = np.asarray(p["D"], np.float32)
    out = np.zeros((len(ranges), 4), np.int64)
    for r, (s, e) in enumerate(ranges):
        blk = D[:, s - 1:e]
        obs = np.isfinite(blk)
        c = np.clip(np.trunc(np.where(obs, blk, 0).astype(np.float32) + np.float32(0.5)), 0, 3).astype(np.int64)
        for k in range(4):
            out[r, k] = int((obs & (c == k)).sum())
    return out


def init_thresholds(counts, triple):
    """The triple the rule gives a range with these class counts; `triple` tells which thresholds are finite (the allowed
    classes are those whose bin is not between two infinite thresholds of one sign).  float64, rounded once to float32."""
    t = np.asarray(triple, np.float64)
    ext = np.concatenate([[-INF], t, [INF]])
    allowed = np.array([not (np.isinf(ext[c]) and ext[c] == ext[c + 1]) for c in range(4)])
    n1 = np.where(allowed, np.asarray(counts, np.float64) + 1.0, 0.0)
    pr = n1 / n1.sum()
    out = t.copy()
    for m in range(3):
        if np.isfinite(t[m]):
            out[m] = inv_logistic(pr[:m + 1].sum())
    return out.astype(np.float32)
