"""simulate_params! / simulate_data! (src/simulate_params.jl) and the scores of the simulation study (src/scores.jl).

simulate_params_ draws a model's parameters on the host (numpy); simulate_data_ draws the data matrix from them on the
device (pmf_simulate_data*, include/pmf_hip.h); average_precision / Y_average_precs score a recovered Y against the planted
feature sets.  The study of analyses/scripts/julia/simulate_matfac.jl is simulate_params_, simulate_data_, fit_, score."""
import numpy as np

from .impute import _context, row_blocks, row_range
from .layers import BatchScale, BatchShift, ColScale, ColShift, FrozenLayer, Identity
from .regularizers import ARDRegularizer, FeatureSetARDReg, GroupRegularizer, L2Regularizer
from .util import unique

# simulate_params.jl:124-142
VIEW_MU_MEAN = {"mrnaseq": 10.0, "methylation": 0.0, "cna": 0.0, "mutation": -1.5}
VIEW_MU_STD = {"mrnaseq": 2.0, "methylation": 0.1, "cna": 0.1, "mutation": 0.1}
VIEW_LOGSIGMA_MEAN = {"mrnaseq": 0.5, "methylation": 0.1, "cna": np.log(2.0), "mutation": np.log(1.0)}
VIEW_LOGSIGMA_STD = {"mrnaseq": 0.1, "methylation": 0.1, "cna": 0.001, "mutation": 0.001}


# ---- factor parameters (simulate_params.jl:7-79) -------------------------------------------------------------------------
def _gamma(rng, shape_param, rate, size):
    """rand(Gamma(alpha, 1 / rate), size): Distributions.jl's Gamma takes (shape, scale)."""
    return rng.gamma(shape_param, 1.0 / rate, size)


def corrupt_S(S, S_add_corruption, S_rem_corruption, rng):
    """corrupt_S (:24-42): per feature set, round(rem * n) members leave, round(add * n) non-members join (n = the set's
    size before; Julia's and Python's round both go to even), and the row is 1 / sqrt(new size) on the new set."""
    S_new = np.array(S, dtype=np.float32)
    L, N = S_new.shape
    for l in range(L):
        cur_set = np.flatnonzero(S_new[l] != 0)
        cur_N = cur_set.size
        rm_N = int(round(S_rem_corruption * cur_N))                                    # :30
        to_remove = rng.choice(cur_set, rm_N, replace=False) if rm_N else np.zeros(0, np.int64)
        cur_complement = np.flatnonzero(S_new[l] == 0)
        add_N = int(round(cur_N * S_add_corruption))                                   # :33
        to_add = rng.choice(cur_complement, add_N, replace=False) if add_N else np.zeros(0, np.int64)
        corrupted = np.union1d(np.setdiff1d(cur_set, to_remove), to_add)               # :36
        S_new[l, :] = 0
        S_new[l, corrupted] = np.float32(1.0 / np.sqrt(corrupted.size)) if corrupted.size else 0   # :38
    return S_new


def _simulate_factor(P, reg, rng, ard_alpha=1.01, ard_beta=0.01, beta0=0.001, S_add_corruption=0.1, S_rem_corruption=0.1,
                     A_nnz=1, **kwargs):
    """simulate_params!(X or Y, reg) (:7-79), dispatched on the regularizer as the reference's methods are."""
    K, N = P.shape
    if isinstance(reg, (GroupRegularizer, L2Regularizer)):                             # :7-11
        P[...] = rng.standard_normal((K, N))
    elif isinstance(reg, ARDRegularizer):                                              # :14-21
        tau = _gamma(rng, ard_alpha, ard_beta, (K, N))
        P[...] = rng.standard_normal((K, N)) / np.sqrt(tau)
    elif isinstance(reg, FeatureSetARDReg):                                            # :45-79
        S_out = []
        for cr, A_mat, S_mat in zip(reg.col_ranges, reg.A, reg.S):
            Nv = len(cr)
            L = S_mat.shape[0]
            A_mat[...] = 0                                                             # :60
            for k in range(K):
                A_mat[rng.integers(L), k] = abs(rng.standard_normal() * 5)             # :62-63
            S_new = corrupt_S(S_mat, S_add_corruption, S_rem_corruption, rng)          # :67
            S_out.append(S_new)
            tau = _gamma(rng, ard_alpha, beta0, (K, Nv))                               # :73
            beta = A_mat.T @ S_new                                                     # :74
            Yv = rng.standard_normal((K, Nv)) / np.sqrt(tau)                           # :75
            Yv *= beta == 0                                                            # :76
            Yv += (beta > 0) * rng.choice(np.array([-1.0, 1.0]), (K, Nv))              # :77
            P[:, cr.start - 1:cr.stop] = Yv
        reg.S = tuple(S_out)
    else:
        raise TypeError(f"simulate_params_: no method for a factor regularized by {type(reg).__name__} (the reference has "
                        "L2Regularizer, GroupRegularizer, ARDRegularizer and FeatureSetARDReg, simulate_params.jl:7-79)")


# ---- layer parameters (:82-187) ----------------------------------------------------------------------------------------
def _simulate_batch_array(ba, rng, b_mean=0.0, between_batch_std=0.95, within_batch_std=0.05, **kwargs):
    for v in ba.values:                                                                # :96-101
        centers = rng.standard_normal(v.shape[0]) * between_batch_std + b_mean
        v[...] = centers[:, None] + rng.standard_normal(v.shape) * within_batch_std


def _simulate_col_param(v, rng, feature_views, view_mean, view_std):
    fv = np.asarray(list(feature_views), dtype=object)
    for uv in unique(list(feature_views)):                                             # :164-174
        idx = fv == uv
        v[idx] = rng.standard_normal(int(idx.sum())) * view_std[uv] + view_mean[uv]


def _simulate_layer(layer, rng, feature_views, **kwargs):
    if isinstance(layer, BatchShift):                                                  # :88-90
        kw = dict(b_mean=kwargs.get("b_shift_mean", 0.0), between_batch_std=kwargs.get("b_shift_std", 0.25), within_batch_std=0.25)
        _simulate_batch_array(layer.theta, rng, **{**kw, **kwargs})
    elif isinstance(layer, BatchScale):                                                # :92-94
        kw = dict(b_mean=kwargs.get("b_scale_mean", 0.0), between_batch_std=kwargs.get("b_scale_std", 0.25), within_batch_std=0.25)
        _simulate_batch_array(layer.logdelta, rng, **{**kw, **kwargs})
    elif isinstance(layer, ColScale):                                                  # :144-152
        _simulate_col_param(layer.logsigma, rng, feature_views, kwargs.get("view_mean", VIEW_LOGSIGMA_MEAN),
                            kwargs.get("view_std", VIEW_LOGSIGMA_STD))
    elif isinstance(layer, ColShift):                                                  # :154-162
        _simulate_col_param(layer.mu, rng, feature_views, kwargs.get("view_mean", VIEW_MU_MEAN),
                            kwargs.get("view_std", VIEW_MU_STD))
    else:
        raise TypeError(f"simulate_params_: no method for layer {type(layer).__name__}")


def simulate_params_(model, rng=None, use_sample_conditions=True, sample_condition_var=0.15, **kwargs):
    """simulate_params!(model; kwargs...) (simulate_params.jl:193-216): Y, X, the four layers, the noise model, in that
    order, from `rng` (a numpy Generator).  Keywords and defaults are the reference's: ard_alpha=1.01, ard_beta=0.01,
    beta0=0.001, S_add_corruption=0.1, S_rem_corruption=0.1, A_nnz=1 (:14-16, 45-50; A_nnz is read and, as there, unused),
    b_shift_mean=0, b_shift_std=0.25, b_scale_mean=0, b_scale_std=0.25 (:88-93), view_mean / view_std (tables per view name:
    VIEW_LOGSIGMA_* for the column scale, VIEW_MU_* for the shift, :124-142; one given here replaces both, as the reference's
    keyword forwarding does).  use_sample_conditions and sample_condition_var are accepted and, as in the reference, unused
    by every method.  A FeatureSetARDReg gets a random A, its S corrupted (corrupt_S) and Y with the planted +-1 entries
    where A'S > 0.  Host only; returns the model."""
    rng = rng if rng is not None else np.random.default_rng()
    mf = model.matfac
    K = mf.X.shape[0]
    _simulate_factor(mf.Y, mf.Y_reg, rng, **kwargs)                                    # :199
    _simulate_factor(mf.X, mf.X_reg, rng, **kwargs)                                    # :206
    ct = mf.col_transform                                                              # :179-187, 210
    for layer in ct.layers:
        layer = layer.layer if isinstance(layer, FrozenLayer) else layer
        if isinstance(layer, Identity):                                                # `isa(layer, Function)`, :182
            continue
        _simulate_layer(layer, rng, model.feature_views, **kwargs)
    l1 = ct.unwrapped(1)
    if isinstance(l1, ColScale):
        l1.logsigma -= np.log(np.sqrt(K))                                              # :212
    nm = mf.noise_model                                                                # :108-119, 215
    for r, name in enumerate(nm.noises):
        if name == "ordinal_sq_hinge3":                                                # ext_thresholds .*= 2 (:111-113)
            nm.thresholds[r] = tuple(float(t) * 2.0 for t in nm.thresholds[r])
    return model


# ---- data (:219-255) ---------------------------------------------------------------------------------------------------
def simulate_data_(model, noise=0.1, seed=0, frac_missing=0.0, to="host", rows=None, capacity=10 ** 8, device=0):
    """simulate_data!(model; noise) (simulate_params.jl:244-255) on the device: the forward of all four layers, then per
    column range normal noise (:240-242) or the class of the noise-free value (bernoulli_sq_hinge :224-228,
    ordinal_sq_hinge3 :230-238); a logit-Bernoulli range draws 0 / 1 with the predicted probability and a Poisson range is
    refused (no reference method for either; DESIGN.md section 2, Deviation 4).  `frac_missing` of the entries, drawn
    independently, become NaN.  The draws are Philox4x32-10 on (seed, global row, column): the same seed gives the same
    matrix whatever the row blocks, and a row shard (row_offset = model.row_shard[0]) draws its rows of the whole matrix.

    to="host": fills model.data (rows `rows`: a range or (start, stop) pair of 0-based local rows, default all) in blocks of
               capacity // N rows and returns the filled block; the device copy is invalidated.
    to="device": pmf_simulate_data_resident overwrites the device's copy of the data, which is then the current one for
               this context: a following fit_ runs on it.  model.data on the host is NOT updated and is stale until the
               next simulate_data_(to="host") or assignment."""
    ctx = _context(model, device)
    N = ctx.N
    off = int(model.row_shard[0])
    if to == "device":
        if rows is not None:
            raise ValueError("simulate_data_: to='device' overwrites the whole resident matrix; `rows` is for to='host'")
        ctx.simulate_data_resident(seed=seed, noise=noise, frac_missing=frac_missing, row_offset=off)
        # device_context() above recorded the device copy as the one of this host array: keep it so (the host array is stale)
        model._ctx_data_id = (id(model.data), model.data.shape)
        return None
    if to != "host":
        raise ValueError(f"simulate_data_: to={to!r} (host | device)")
    lo, hi = row_range("simulate_data_", rows, ctx.M)
    data = model.data
    direct = isinstance(data, np.ndarray) and data.dtype == np.float32 and data.flags.f_contiguous and data.flags.writeable
    out = data if direct else np.empty((hi - lo, N), np.float32, order="F")
    base = lo if direct else 0
    for r0, nr in row_blocks(hi - lo, N, capacity):
        ctx.simulate_data(seed=seed, noise=noise, frac_missing=frac_missing, row_offset=off, row_start1=lo + r0 + 1,
                          row_stop1=lo + r0 + nr, out=out, out_row=base + r0)
    if not direct:
        data[lo:hi] = out
    model.invalidate_device_data()
    return data[lo:hi]


# ---- scores (scores.jl) ------------------------------------------------------------------------------------------------
def average_precision(y_pred, y_true):
    """average_precision(y_pred, y_true) (scores.jl:11-50): the area under the precision-recall steps, thresholds taken in
    decreasing order of y_pred and equal predictions entering together.  y_true is boolean.  Like the reference, no
    positives at all gives NaN (0 / 0)."""
    y_pred = np.asarray(y_pred).ravel()
    y_true = np.asarray(y_true).ravel().astype(bool)
    srt = np.argsort(-y_pred, kind="stable")                                           # sortperm(y_pred; rev=true), :13
    pred_srt, true_srt = y_pred[srt], y_true[srt]
    cur_threshold = pred_srt[0]
    TP_total = float(y_true.sum())
    TP = FP = 0
    R = 0.0
    ave_prec = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for yp, yt in zip(pred_srt, true_srt):
            if yp != cur_threshold:                                                    # :28-35
                Rnew = np.float64(TP) / TP_total
                P = np.float64(TP) / (TP + FP)
                ave_prec += P * (Rnew - R)
                R = Rnew
                cur_threshold = yp
            if yt:                                                                     # :38-42
                TP += 1
            else:
                FP += 1
        P = np.float64(TP) / (TP + FP)                                                 # :45-47
        ave_prec += P * (1.0 - R)
    return float(ave_prec)


def Y_average_precs(Y, truth_mask):
    """model_Y_average_precs (scores.jl:53-61) per factor: average_precision(|Y[k, :]|, truth_mask[k, :]).  The truth is a
    boolean K x N mask (e.g. A'S > 0 of the simulated FeatureSetARDReg): the reference reads it from a field of the Y
    regularizer (l1_reg.l1_idx) that no longer exists."""
    Y = np.abs(np.asarray(Y))
    truth_mask = np.asarray(truth_mask).astype(bool)
    if Y.shape != truth_mask.shape:
        raise ValueError(f"Y_average_precs: Y is {Y.shape}, the mask {truth_mask.shape}")
    return [average_precision(Y[k], truth_mask[k]) for k in range(Y.shape[0])]
