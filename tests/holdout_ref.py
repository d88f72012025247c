"""Hold-out entries (include/pmf_hip_holdout.h, DESIGN.md section 2, Deviation 7) restated in numpy on the model of
tests/hinge_ref.py: the set's bookkeeping, the hold-out loss in float64, a float32 twin of the kernel's arithmetic, the
rounding bound the device is held to, the early-stopping rule, and the problems of the tests.

    z_ij = z1_ij delta_bj + mu_j + theta_bj,  z1_ij = sigma_j sum_k x_ki y_kj                      (hinge_ref.forward)
    loss_col[j] = sum over the held (i, j) of w_j l(z_ij, y_ij)      n_col[j] = their number      total = sum_j loss_col[j]
y is the value the entry held before it was blanked; l is the column's entry loss (hinge_ref.entry_model).

THE BOUND, per column, with eps = 2^-24, g = dl/dz and T_ij = K sum_k |sigma_j x_ki y_kj delta_bj|:
    eps (C sum (|l| + |g| T) + CHAIN sum |l|)
The first bracket is what the float32 evaluation of an entry can lose: the loss itself, and the error of z through the slope.
The second is the accumulation: the kernel rounds an entry's loss to float32 ONCE and sums in float64 from there on, so
CHAIN = 1 (the float64 additions lose 2^-53 relative per step, far below eps).
C is MEASURED: the worst ratio of the float32 twin's error to eps x the first bracket over cases() x held_sets(), times two:
    worst ratio 3.526 (k1, set "wide")         ->  C = 7.06
tests/test_holdout_cases.py re-measures it and fails if the ratio has grown past half of C.

Plain numpy; neither the package nor the C oracle is imported here."""
import functools

import numpy as np

import batch_cases as bc
import hinge_ref as hr
import importance_ref as ir
from problems import make_problem

EPS = 2.0 ** -24
CHAIN = 1.0
C = 7.06                                                   # 2 x 3.526, measured (see above)
F = np.float32
M, N = 70, 75                                              # three ragged row blocks, three ragged column tiles
KS = (1, 4, 33, 64, 128)
SPEC = [((1, 12), "bernoulli", None), ((13, 27), "bernoulli_sq_hinge", None), ((28, 45), "normal", None),
        ((46, 63), "ordinal_sq_hinge3", None), ((64, 75), "poisson", None)]


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
def sort_entries(rows, cols, M):
    """The library's order: by (column, row).  0-based in, 0-based out."""
    r, c = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    o = np.argsort(c * M + r, kind="stable")
    return r[o], c[o]


def held_after_set(D, rows, cols):
    """(rows, cols, values) the library keeps: sorted, the already-missing entries dropped; and the masked matrix."""
    r, c = sort_entries(rows, cols, D.shape[0])
    ok = np.isfinite(D[r, c])
    r, c = r[ok], c[ok]
    Dm = np.array(D, np.float32, order="F")
    v = Dm[r, c].copy()
    Dm[r, c] = np.nan
    return r, c, v, Dm


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def reference(p, rows, cols):
    """p: the problem with its ORIGINAL data.  dict(loss_col, n_col, total, b, c): float64 sums over the held entries that
    are observed in p["D"], and the two brackets of the bound."""
    r, c, _, _ = held_after_set(np.asarray(p["D"]), rows, cols)
    X, Y = np.asarray(p["X"], np.float64), np.asarray(p["Y"], np.float64)
    sig, w = np.exp(np.asarray(p["logsigma"], np.float64)), np.asarray(p["col_weight"], np.float64)
    _, dl, _, z = hr.forward(p)
    e = hr.entry_model(p, z)
    T = p["K"] * (np.abs(X).T @ np.abs(Y)) * sig[None, :] * np.abs(dl)
    l, g = w[None, :] * e["l"], w[None, :] * e["g"]
    held = np.zeros((p["M"], p["N"]), bool)
    held[r, c] = True
    m = lambda v: np.where(held, v, 0.0).sum(0)                               # noqa: E731
    out = dict(loss_col=m(l), n_col=held.sum(0).astype(np.int64), b=m(np.abs(l) + np.abs(g) * T), c=m(np.abs(l)))
    out["total"] = float(np.cumsum(out["loss_col"])[-1])                      # ascending columns, one after the other
    return out


def bound(ref):
    return EPS * (C * ref["b"] + CHAIN * ref["c"])


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; one rounding to float64 first, which the twin tolerates."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def twin(p, rows, cols):
    """dict(loss_col, n_col, total): the kernel's arithmetic in float32 -- sixteen fma partial sums over k (partial s takes
    k = 4 s .. 4 s + 3, then 64 + 4 s ..), the butterfly s ^ 8, 4, 2, 1, z = fma(z1 sigma, delta, mu + theta), the expressions
    of pmf_noise (importance_ref._loss32), one float32 per entry, float64 sums."""
    r, c, _, _ = held_after_set(np.asarray(p["D"]), rows, cols)
    K, Mp, Np = p["K"], p["M"], p["N"]
    Kp = -(-K // 32) * 32
    X, Y = np.zeros((Kp, Mp), F), np.zeros((Kp, Np), F)
    X[:K], Y[:K] = np.asarray(p["X"], F), np.asarray(p["Y"], F)
    sig, mu = np.exp(np.asarray(p["logsigma"], F)), np.asarray(p["mu"], F)
    part = []
    for s in range(16):
        acc = np.zeros((Mp, Np), F)
        for k in [k0 + 4 * s + q for k0 in (0, 64) for q in range(4) if k0 + 4 * s + q < Kp]:
            acc = _fma(X[k][:, None], Y[k][None, :], acc)
        part.append(acc)
    for off in (8, 4, 2, 1):
        part = [part[s] + part[s ^ off] for s in range(16)]
    dl, th = np.ones((Mp, Np), F), np.zeros((Mp, Np), F)
    for v in p["batch_views"]:
        bor = np.asarray(v["batch_of_row"])
        has = bor >= 0
        idx = np.ix_(has, np.arange(v["start1"] - 1, v["stop1"]))
        dl[idx] = np.exp(np.asarray(v["logdelta"], F))[bor[has]]
        th[idx] = np.asarray(v["theta"], F)[bor[has]]
    z = _fma(part[0] * sig[None, :], dl, mu[None, :] + th)
    held = np.zeros((Mp, Np), bool)
    held[r, c] = True
    y = np.where(held, np.asarray(p["D"], F), F(0))
    l = ir._loss32(p, np.where(held, z, F(0)), y)
    loss_col = np.where(held, l, F(0)).astype(np.float64).sum(0)
    return dict(loss_col=loss_col, n_col=held.sum(0).astype(np.int64), total=float(np.cumsum(loss_col)[-1]))


def worst_ratio(p, rows, cols):
    """The twin's error over eps x the first bracket: what C is twice the worst of.  Where the bracket is 0 the twin is exact."""
    ref, tw = reference(p, rows, cols), twin(p, rows, cols)
    err, b = np.abs(tw["loss_col"] - ref["loss_col"]), ref["b"]
    assert (err[b == 0] == 0).all()
    return float(np.max(err[b > 0] / (EPS * b[b > 0]), initial=0.0))


def check(got_loss_col, got_n_col, got_total, p, rows, cols):
    ref = reference(p, rows, cols)
    assert np.array_equal(np.asarray(got_n_col), ref["n_col"])
    err, bd = np.abs(np.asarray(got_loss_col) - ref["loss_col"]), bound(ref)
    bad = ~(err <= bd)
    assert not bad.any(), (np.flatnonzero(bad)[:5].tolist(), float(np.max(err[bad] / bd[bad])))
    assert abs(got_total - ref["total"]) <= bd.sum(), (got_total, ref["total"])
    return float(np.max(np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), 0.0)))


# ---- the problems ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(K, nan_frac=0.05):
    """70 x 75: all four kinds and both squared-hinge ranges, weights, column parameters, nan_frac missing, two batch views (4
    sorted batches over columns 1..30 with three rows in no batch, 6 scrambled over columns 41..75; columns 31..40 in no
    view), by the rules of hinge_ref.layout_from.  Shared objects: do not modify them."""
    seed = 4200 + K
    p = make_problem(M=M, N=N, K=K, seed=seed, nan_frac=nan_frac, weights=True, col_params=True, scale=hr.factor_scale(K),
                     bernoulli_frac=12 / N, poisson_frac=12 / N)
    drawn = hr.kinds_of(p)
    p["noise_ranges"] = [r for r, _, _ in SPEC]
    p["noise_kinds"] = [k for _, k, _ in SPEC]
    p["noise_thr"] = [hr.THR.get(k) for _, k, _ in SPEC]
    rng = np.random.default_rng(seed + 1)
    _, _, _, z = hr.forward(p, batch=False)
    t = hr.thresholds_of(p)
    D = np.array(p["D"], np.float32)
    for j in np.flatnonzero(hr.kinds_of(p) == 3):
        cls = (t[j][None, :] < (z[:, j] + 0.5 * rng.standard_normal(M))[:, None]).sum(1)
        D[:, j] = np.where(np.isnan(D[:, j]), np.nan, cls)
    for j in np.flatnonzero((hr.kinds_of(p) == 1) & (drawn != 1)):
        D[:, j] = np.where(np.isnan(D[:, j]), np.nan, D[:, j] > 0)
    p["D"] = np.asfortranarray(D)
    b0 = bc.sorted_rows(M, 4)
    b0[[0, 33, M - 1]] = -1
    bvs = []
    for s, e, bor, nb in [(1, 30, b0, 4), (41, N, bc.scrambled_rows(M, 6, rng), 6)]:
        cd, ct = rng.standard_normal(nb)[:, None] * 0.25, rng.standard_normal(nb)[:, None] * 0.25
        bvs.append(dict(start1=s, stop1=e, batch_of_row=np.asarray(bor, np.int32),
                        logdelta=(cd + 0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                        theta=(ct + 0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32)))
    p["batch_views"] = bvs
    return p


def cases():
    return {f"k{K}": problem(K) for K in KS}


def masked(p, rows, cols):
    """A copy of p whose data have the set blanked: what a host that masks by hand would upload."""
    q = dict(p)
    q["D"] = held_after_set(np.asarray(p["D"]), rows, cols)[3]
    return q


def held_sets(p, seed=0):
    """name -> (rows, cols), 0-based, UNSORTED: "wide" 15 % of all positions (missing ones among them), row M and column N
    always in, column 7 left out, column 40 with 40 entries (it crosses a unit seam at PMF_HOLDOUT_UNIT=16);
    "corners": the four corner entries and the pad-adjacent ones of the last row block and column tile alone."""
    rng = np.random.default_rng(900 + seed)
    Mp, Np = p["M"], p["N"]
    pick = rng.random((Mp, Np)) < 0.15
    pick[Mp - 1, :] |= rng.random(Np) < 0.5
    pick[:, Np - 1] |= rng.random(Mp) < 0.5
    pick[Mp - 1, Np - 1] = True
    pick[:, 7] = False
    pick[:, 40] = False
    pick[rng.permutation(Mp)[:40], 40] = True
    r, c = np.nonzero(pick)
    o = rng.permutation(r.size)
    cr = np.array([0, Mp - 1, 0, Mp - 1, 63, 64, 68, 31, 32], np.int64)
    cc = np.array([0, 0, Np - 1, Np - 1, 63, 64, 73, 31, 32], np.int64)
    return {"wide": (r[o].astype(np.int64), c[o].astype(np.int64)), "corners": (cr, cc)}


# ---- the early-stopping rule ----------------------------------------------------------------------------------------------
def stopping_rule(epochs, losses, patience, min_delta=0.0):
    """The rule of pmf_hip_holdout.h on a trace of evaluations: (stop_epoch or None, best_epoch, best_loss, evaluations used).
    An evaluation improves if H < best - min_delta (the first finite one always does); after `patience` > 0 evaluations in
    a row without improvement the fit stops at that epoch."""
    best, best_epoch, bad = None, 0, 0
    for n, (e, H) in enumerate(zip(epochs, losses)):
        if (np.isfinite(H) if best is None else H < best - min_delta):
            best, best_epoch, bad = float(H), int(e), 0
        else:
            bad += 1
            if patience > 0 and bad >= patience:
                return int(e), best_epoch, best, n + 1
    return None, best_epoch, best, len(losses)


OVERFIT = dict(M=70, N=75, K=16, rank=2, held=0.4, lr=0.1, max_epochs=60, patience=5)


@functools.lru_cache(maxsize=None)
def overfit_problem(seed=0):
    """(p, rows, cols): D = a rank-2 product + unit Gaussian noise, all-normal columns, fully observed; 40 % of the entries
    held; factors 0.3 N(0, 1) at K = 16; no regularizers."""
    o = OVERFIT
    rng = np.random.default_rng(7000 + seed)
    D = rng.standard_normal((o["M"], o["rank"])) @ rng.standard_normal((o["rank"], o["N"])) + rng.standard_normal((o["M"], o["N"]))
    p = make_problem(M=o["M"], N=o["N"], K=o["K"], seed=seed)
    p["D"] = np.asfortranarray(D.astype(np.float32))
    p["X"] = np.asfortranarray((0.3 * rng.standard_normal((o["K"], o["M"]))).astype(np.float32))
    p["Y"] = np.asfortranarray((0.3 * rng.standard_normal((o["K"], o["N"]))).astype(np.float32))
    r, c = np.nonzero(rng.random((o["M"], o["N"])) < o["held"])
    return p, r.astype(np.int64), c.astype(np.int64)


def normal_holdout_loss(X, Y, D, rows, cols):
    """The hold-out loss of an all-normal model without layers or weights: 0.5 sum (x_i'y_j - d_ij)^2, float64."""
    z = np.einsum("ke,ke->e", np.asarray(X, np.float64)[:, rows], np.asarray(Y, np.float64)[:, cols])
    return 0.5 * float(np.sum((z - np.asarray(D, np.float64)[rows, cols]) ** 2))
