"""Helpers of the FeatureSetARD outer-loop tests (pmf_fsard_update_A): the seeded case generator, a float32 numpy
restatement of update_A_inner! + ISTAOptimiser.update! (src/featureset_ard.jl:154-276, src/optimizers.jl:26-62; written
from the reference's text, every array operation in Float32 as the reference runs it), the float64 oracle with its
per-epoch trace, the error measures, the launch geometry restated from csrc/pmf_fsard.hip, and the case tables that
tests/test_gpu_fsard_edges.py runs on the device and tests/test_fsard_cases.py guards on the CPU."""
import re
from pathlib import Path

import numpy as np

from oracle import fsard_oracle as fo

F = np.float32
HIP_SOURCE = Path(__file__).resolve().parent.parent / "pathmatfac.jl_amd" / "csrc" / "pmf_fsard.hip"

# ---- launch geometry of pmf_fsard_update_A, restated (test_fsard_cases.py checks these against the source text) -------
LDS_LIMIT = 150 * 1024      # bytes of dynamic LDS above which the sub-slice width halves
CW_MAX = 256                # columns per sub-slice = live threads of a 256-thread workgroup
MAXO = 64                   # (l, k) outputs per thread
CAPACITY = MAXO * 256       # L * K
MAX_WG = 32


def lds_bytes(L, K, cw):
    return (L * K + K * (cw + 1)) * 4


def sub_slice_width(L, K):
    cw = CW_MAX
    while cw > 32 and lds_bytes(L, K, cw) > LDS_LIMIT:
        cw >>= 1
    return cw


def n_workgroups(L, K, Nv):
    cw = sub_slice_width(L, K)
    return max(1, min(MAX_WG, -(-Nv // cw)))


def source_constants():
    """The geometry constants as the kernel source states them."""
    txt = HIP_SOURCE.read_text()
    out = {}
    m = re.search(r"int CW = (\d+);", txt)
    out["CW_MAX"] = int(m.group(1)) if m else None
    m = re.findall(r"\* 4 > (\d+) \* (\d+)", txt)
    out["LDS_LIMIT"] = sorted({int(a) * int(b) for a, b in m})
    m = re.search(r"constexpr int MAXO = (\d+);", txt)
    out["MAXO"] = int(m.group(1)) if m else None
    m = re.search(r"if \(n > (\d+) \* (\d+)\) return pmf_fail", txt)
    out["CAPACITY"] = int(m.group(1)) * int(m.group(2)) if m else None
    m = re.search(r"std::min<int64_t>\((\d+), \(Nv \+ CW - 1\) / CW\)", txt)
    out["MAX_WG"] = int(m.group(1)) if m else None
    m = re.search(r"__launch_bounds__\((\d+)\) void k_fsard_grad", txt)
    out["THREADS"] = int(m.group(1)) if m else None
    return out


# ---- the case generator -------------------------------------------------------------------------------------------------
def make_case(L, K, Nv, seed, dense=False, N=None, c0=1, alpha0=1.01, v0=0.8, lr=0.1, lam=0.01, noise=0.05, n_zero=5,
              max_epochs=6, term_iter=50, atol=1e-5):
    """One view of a FeatureSetARD model: S (L x Nv float32, non-uniform positive weights; one all-zero row = a feature set
    without a member in the view when L >= 3, one all-zero column when Nv >= 3; `dense`: every other entry positive),
    alpha varying per column, lambda per factor around `lam`, and Y (K x N float32, the view at 1-based columns
    c0 .. c0 + Nv - 1): small noise, every factor loaded (both signs) on the members of several feature sets, a few exact
    zeros.  Columns of Y outside the view carry unit-scale noise.  Returns a dict."""
    rng = np.random.default_rng(seed)
    N = Nv if N is None else N
    assert 1 <= c0 and c0 + Nv - 1 <= N
    S = np.zeros((L, Nv), F)
    size = Nv if dense else max(1, min(Nv, max(3, Nv // 12)))
    for l in range(L):
        idx = np.arange(Nv) if dense else rng.choice(Nv, size=size, replace=False)
        S[l, idx] = (rng.uniform(0.5, 1.5, size=len(idx)) / np.sqrt(len(idx))).astype(F)
    zero_row = L // 2 if L >= 3 else None
    zero_col = Nv // 3 if Nv >= 3 else None
    if zero_row is not None:
        S[zero_row] = 0
    if zero_col is not None:
        S[:, zero_col] = 0
    Y = (rng.standard_normal((K, N))).astype(F)
    view = slice(c0 - 1, c0 - 1 + Nv)
    Yv = (rng.standard_normal((K, Nv)) * noise).astype(F)
    rows = [l for l in range(L) if l != zero_row]
    n_planted = min(len(rows), max(4, L // 8))
    for k in range(K):
        for l in rng.choice(rows, size=n_planted, replace=False):
            members = np.nonzero(S[l])[0]
            Yv[k, members] += F(rng.choice([-1.0, 1.0]) * rng.uniform(0.7, 1.3))
    Yv.ravel()[rng.choice(K * Nv, size=min(n_zero, K * Nv), replace=False)] = 0        # log(|y| + 1e-9)
    Y[:, view] = Yv
    alpha = (1.01 + 0.5 * rng.random(Nv)).astype(F)
    lam_v = (lam * (0.5 + rng.random(K))).astype(F)
    return dict(L=L, K=K, Nv=Nv, N=N, c0=c0, c1=c0 + Nv - 1, S=S, Y=np.asfortranarray(Y), alpha=alpha, lam=lam_v,
                alpha0=float(F(alpha0)), v0=float(F(v0)), lr=float(F(lr)), max_epochs=max_epochs, term_iter=term_iter,
                atol=atol, zero_row=zero_row, zero_col=zero_col)


def view_Y(case, Y=None):
    Y = case["Y"] if Y is None else Y
    return Y[:, case["c0"] - 1:case["c1"]]


def fresh_ssq(case, value=1e-8):
    return np.full((case["L"], case["K"]), value, F)


# ---- the float64 oracle, with its trace -----------------------------------------------------------------------------------
def run_oracle(case, ssq_in=None, Y=None, **over):
    """oracle/fsard_oracle.py on the case's float32 inputs widened to float64.  -> dict(A, ssq, beta, best, epochs, trace)"""
    kw = dict(max_epochs=case["max_epochs"], term_iter=case["term_iter"], atol=case["atol"])
    kw.update(over)
    S = case["S"].astype(np.float64)
    A = np.zeros((case["L"], case["K"]))
    ssq = (fresh_ssq(case) if ssq_in is None else ssq_in).astype(np.float64)
    best, epochs, trace = fo.update_A_inner(A, S, view_Y(case, Y).astype(np.float64), case["alpha"].astype(np.float64),
                                            case["alpha0"], case["v0"], case["lr"], case["lam"].astype(np.float64), ssq,
                                            trace=True, **kw)
    beta = (case["alpha0"] - 1) * (case["v0"] + A.T @ S)
    return dict(A=A, ssq=ssq, beta=beta, best=float(best), epochs=epochs, trace=trace)


def last_iterate(case, epochs, ssq_in=None, Y=None):
    """The oracle's A after exactly `epochs` updates (not A_best)."""
    S = case["S"].astype(np.float64)
    A = np.zeros((case["L"], case["K"]))
    ssq = (fresh_ssq(case) if ssq_in is None else ssq_in).astype(np.float64)
    Yv, al, lam = view_Y(case, Y).astype(np.float64), case["alpha"].astype(np.float64), case["lam"].astype(np.float64)
    for _ in range(epochs):
        g = fo.grad_A(A, S, al, case["alpha0"], case["v0"], Yv)
        ssq += g * g
        eta = case["lr"] / np.sqrt(ssq)
        A = np.maximum(A - eta * g, 0)
        A = np.maximum(np.abs(A) - lam[None, :] * eta, 0)
    return A


# ---- the float32 restatement ------------------------------------------------------------------------------------------------
def _loss_f32(A, S, alpha, alpha0, v0, Y):                      # featureset_ard.jl:154-162
    """Every term in Float32; the sums over the K x Nv terms are taken in float64, so that the figure measures the
    rounding of the terms and not numpy's summation order (a float32 sum of 1e6 terms alone is off by 1e-6)."""
    beta0 = F(alpha0) - F(1)
    beta = beta0 * (F(v0) + A.T @ S)
    a5 = alpha + F(0.5)
    lss = -np.sum(alpha[None, :] * np.log(beta), dtype=np.float64) \
        + np.sum(a5[None, :] * np.log(beta + F(0.5) * (Y * Y)), dtype=np.float64)
    lss -= np.sum(a5 * np.log(a5) - alpha * np.log(alpha), dtype=np.float64) \
        + np.sum(np.log(np.abs(Y) + F(1e-9)), dtype=np.float64)
    return float(lss)


def _grad_f32(A, S, alpha, alpha0, v0, Y):                      # featureset_ard.jl:164-178
    beta0 = F(alpha0) - F(1)
    beta = beta0 * (F(v0) + A.T @ S)
    g = beta0 * ((-alpha[None, :] / beta) + (alpha + F(0.5))[None, :] / (beta + F(0.5) * (Y * Y)))
    return S @ g.T


def run_f32(case, ssq_in=None, Y=None, **over):
    """update_A! of one view with every array and scalar in Float32 (featureset_ard.jl:214-292, optimizers.jl:46-62)."""
    kw = dict(max_epochs=case["max_epochs"], term_iter=case["term_iter"], atol=case["atol"])
    kw.update(over)
    S, alpha, lam = case["S"], case["alpha"], case["lam"]
    Yv = np.ascontiguousarray(view_Y(case, Y), dtype=F)
    alpha0, v0, lr = case["alpha0"], case["v0"], F(case["lr"])
    A = np.zeros((case["L"], case["K"]), F)                                        # :286
    ssq = (fresh_ssq(case) if ssq_in is None else ssq_in).astype(F).copy()

    def total(Am):
        return _loss_f32(Am, S, alpha, alpha0, v0, Yv) + float(np.sum(lam[None, :] * np.abs(Am), dtype=np.float64))
    best = total(A)
    A_best = A.copy()
    term_count = epochs = 0
    for _ in range(kw["max_epochs"]):
        g = _grad_f32(A, S, alpha, alpha0, v0, Yv)
        ssq += g * g                                                               # optimizers.jl:50
        eta = lr / np.sqrt(ssq)
        A -= eta * g
        A = np.maximum(A, F(0))
        A = np.maximum(np.abs(A) - lam[None, :] * eta, F(0))                       # ist_proj!
        epochs += 1
        new = total(A)
        if new < best:
            diff = best - new
            best = new
            A_best = A.copy()
            term_count = 0 if diff > kw["atol"] else term_count + 1
        else:
            term_count += 1
        if term_count >= kw["term_iter"]:
            break
    A = A_best
    assert A.dtype == F and ssq.dtype == F
    beta = (F(alpha0) - F(1)) * (F(v0) + A.T @ S)
    return dict(A=A, ssq=ssq, beta=beta, best=float(best), epochs=epochs)


# ---- error measures -----------------------------------------------------------------------------------------------------------
def norm_err(a, b):
    """|a - b| / |b| in the Frobenius norm, b the float64 oracle's value (|b| = 0: the absolute norm)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))


SSQ_FLOOR = 1e-6     # entries whose accumulated g^2 is below this fraction of the case's largest one are measured against it


def ssq_err(ssq, ssq_in, ssq_o, ssq_in_o=None):
    """max over (l, k) of |d - d_o| / max(d_o, SSQ_FLOOR * max d_o), d = what the call added to the accumulator.  The
    floor covers the entries whose gradient is structurally zero (an all-zero row of S: d_o = 0 exactly)."""
    ssq_in_o = ssq_in if ssq_in_o is None else ssq_in_o
    d = np.asarray(ssq, np.float64) - np.asarray(ssq_in, np.float64)
    do = np.asarray(ssq_o, np.float64) - np.asarray(ssq_in_o, np.float64)
    floor = SSQ_FLOOR * float(do.max()) if do.size and do.max() > 0 else 1e-30
    return float(np.max(np.abs(d - do) / np.maximum(do, floor)))


def loss_err(a, b):
    return abs(a - b) / abs(b)


# ---- the case tables: name -> arguments of make_case (shape, seed, run length and stopping rule) ------------------------
BASE = dict(L=12, K=20, Nv=300, seed=7)                    # CW = 256, two workgroups, K < Kp = 32
# an oscillating run: a dense S couples every feature set to every column, so the first AdaGrad steps (each of size lr,
# whatever the gradient) overshoot together and the loss rises and falls by far more than rounding
MIXED = dict(L=12, K=20, Nv=300, seed=1, dense=True, alpha0=2.0, v0=0.1, lr=30.0, noise=0.3, atol=0.5, max_epochs=60)

K_EDGES = {f"K{K}": dict(L=12, K=K, Nv=777, seed=100 + K) for K in (1, 31, 32, 33, 64, 65, 100, 128)}

OUTPUTS = {                                                # L * K against 256 threads x MAXO outputs
    "LK255_15x17": dict(L=15, K=17, Nv=300, seed=32),
    "LK256_16x16": dict(L=16, K=16, Nv=300, seed=33),
    "LK257_257x1": dict(L=257, K=1, Nv=300, seed=34),
    "LK16384_128x128": dict(L=128, K=128, Nv=300, seed=35),
    "LK16384_16384x1": dict(L=16384, K=1, Nv=300, seed=36),
    "L1_1x40": dict(L=1, K=40, Nv=300, seed=37),
    "dense_12x20": dict(L=12, K=20, Nv=300, seed=38, dense=True),
}

CW_PAIRS = ((43, 128), (44, 128), (143, 96), (144, 96))    # (L, K): the last shape with CW = 256 and the first with 128
CW_EDGES = {}
for _L, _K in CW_PAIRS:
    _cw = sub_slice_width(_L, _K)
    for _d in (-1, 0, 1):
        CW_EDGES[f"{_L}x{_K}_Nv{_cw + _d}"] = dict(L=_L, K=_K, Nv=_cw + _d, seed=1000 + _L + _d)
CW_EDGES["44x128_Nv4097"] = dict(L=44, K=128, Nv=32 * 128 + 1, seed=1100)      # a workgroup walks two sub-slices

PAD = 37                                                   # columns of the model outside the view
NV_POSITIONS = {}
for _Nv in (1, 255, 256, 257, 8192, 8193):
    for _pos in ("first", "last", "middle"):
        _c0 = {"first": 1, "last": PAD + 1, "middle": 20}[_pos]
        NV_POSITIONS[f"Nv{_Nv}_{_pos}"] = dict(L=12, K=20, Nv=_Nv, N=_Nv + PAD, c0=_c0, seed=2000 + _Nv)

BETA_DEST = dict(BASE, N=300 + PAD, c0=20)                 # one case, four destinations of beta

# term_iter = max_epochs + 1: the counter cannot end the run, and the host's batch of max(8, term_iter) queued iterations is
# 8, 8, 8, 9, 10, 17, 18 -- cut short by max_epochs in every row
MAX_EPOCHS = {f"max_epochs{m}": dict(BASE, max_epochs=m, term_iter=m + 1) for m in (0, 1, 7, 8, 9, 16, 17)}
TERM_ITER = {f"term_iter{t}": dict(MIXED, term_iter=t) for t in (1, 3, 8, 9)}
STOP_RULES = {
    "strong_lambda": dict(BASE, lam=1e6, term_iter=5, max_epochs=40),          # A stays 0: every epoch "not improved"
    # the same with atol < 0: an equal loss taken for an improvement (<= for <) would beat atol and reset the counter
    "strong_lambda_negative_atol": dict(BASE, lam=1e6, term_iter=5, max_epochs=40, atol=-1.0),
    "atol_1e30": dict(BASE, atol=1e30, term_iter=5, max_epochs=40),           # every improvement counts towards the end
    "atol_0": dict(BASE, atol=0.0, term_iter=50, max_epochs=12),
}
ZERO_A = {"max_epochs0", "strong_lambda", "strong_lambda_negative_atol"}                  # the cases built to return A = 0

STATE = {
    "two_calls": dict(BASE, seed=41),
    "after_set_Y": dict(BASE, seed=42),
    "after_set_Y_second": dict(BASE, seed=43),
    "L40": dict(L=40, K=20, Nv=300, seed=44),
    "L5": dict(L=5, K=20, Nv=300, seed=45),
}
REPRO = {"cw128_44x128_Nv129": CW_EDGES["44x128_Nv129"], "Nv8193_middle": NV_POSITIONS["Nv8193_middle"],
         "mixed_term_iter9": TERM_ITER["term_iter9"]}
REFUSAL_ROWS = {"good_after_refusal": dict(BASE, seed=46), "good_after_refusal_K1": dict(BASE, seed=47, K=1)}

TABLES = dict(K_EDGES=K_EDGES, OUTPUTS=OUTPUTS, CW_EDGES=CW_EDGES, NV_POSITIONS=NV_POSITIONS,
              BETA_DEST={"beta_dest": BETA_DEST}, MAX_EPOCHS=MAX_EPOCHS, TERM_ITER=TERM_ITER, STOP_RULES=STOP_RULES,
              STATE=STATE, REFUSALS=REFUSAL_ROWS)


def all_cases():
    """(table, name, spec) of every row that a device test compares with the oracle."""
    for t, rows in TABLES.items():
        for name, spec in rows.items():
            yield t, name, spec


# ---- decision margins ------------------------------------------------------------------------------------------------------
def decision_margin(trace, atol):
    """The smallest distance, relative to |best_loss|, between a quantity the loop compares and its threshold: new_loss
    against best_loss at every update whose A is not identical to A_best (an equal loss from an identical A is structural),
    and best_loss - new_loss against atol at every improvement."""
    m = np.inf
    for s in trace:
        if s["same_A"]:
            continue
        b = abs(s["best"])
        m = min(m, abs(s["new"] - s["best"]) / b)
        if s["branch"] != "b":
            m = min(m, abs((s["best"] - s["new"]) - atol) / b)
    return m


# ---- bounds ------------------------------------------------------------------------------------------------------------
# MEASURED: the worst discrepancy of the float32 restatement from the float64 oracle over every row of the tables above
# (and the second calls of the state rows), rounded up; test_fsard_cases.py measures it again on every run and fails if a
# row exceeds it.  TOL = 20 x MEASURED is what the device is held to: its arithmetic differs from numpy's in logf and in
# the order of fmaf and of the sums, not in what is computed.
MEASURED = dict(A=5.0e-7, beta=4.5e-7, ssq=1.9e-5, loss=2.1e-7)
TOL = {k: 20 * v for k, v in MEASURED.items()}
MARGIN = 1000 * MEASURED["loss"]          # every decision of every compared run is at least this far from its threshold
A_BEST_GAP = 100 * TOL["A"]               # A_best differs from the last iterate by more than this where a test says so


def errors(got, want, ssq_in, ssq_in_want=None):
    """The four compared figures of one call (got: device or float32 restatement; want: run_oracle)."""
    return dict(A=norm_err(got["A"], want["A"]), beta=norm_err(got["beta"], want["beta"]),
                ssq=ssq_err(got["ssq"], ssq_in, want["ssq"], ssq_in_want), loss=loss_err(got["best"], want["best"]))


# ---- the Y regularizer's value: the only window on the device copy of its beta -------------------------------------------
BETA_UPLOADED = 0.5      # beta of the attached term before the call: > 10 x any beta the call computes (0.001 .. 0.03)
# one evaluation of the term against its closed form.  Every summand (alpha + 0.5) log(1 + (0.5 / beta) y^2) is positive
# and carries a few float32 roundings (2e-7 relative), the sum is taken in double: 1e-5 leaves a factor of ten or more
REG_TOL = 1e-5


def reg_alpha(N):
    return np.linspace(1.1, 1.4, N).astype(F)


def reg_value(alpha_full, beta_full, Y):
    """FeatureSetARDReg / ARDRegularizer value in float64: sum (alpha_j + 0.5) log(1 + 0.5 y_kj^2 / beta_kj)."""
    Y = np.asarray(Y, np.float64)
    return float(np.sum((0.5 + np.asarray(alpha_full, np.float64))[None, :]
                        * np.log1p((0.5 / np.asarray(beta_full, np.float64)) * Y * Y)))


def beta_after(case, beta_view, uploaded=BETA_UPLOADED):
    """K x N beta of the attached term after the call: `uploaded` outside the view, beta_view inside."""
    b = np.full((case["K"], case["N"]), uploaded, np.float64)
    b[:, case["c0"] - 1:case["c1"]] = beta_view
    return b
