"""The mirror of include/pmf_hip.h: its constants, its structs and the signature of every function, as data.

load_library (_lib.py) installs SIGNATURES on every CDLL it creates, so ctypes converts a Python int to the declared width,
a Python float to the declared precision, and refuses an argument of another kind before the call is made.
tests/test_abi.py compares every entry, and every struct, with the header.
"""
import ctypes as C
from math import inf

# bernoulli_sq_hinge and ordinal_sq_hinge3 are one kind (3) with different thresholds per column (set_noise_thresholds)
NOISE = {"normal": 0, "bernoulli": 1, "poisson": 2, "bernoulli_sq_hinge": 3, "ordinal_sq_hinge3": 3}
# the thresholds (t0, t1, t2) a kind-3 range gets by name.  ordinal_sq_hinge3's default is OURS (symmetric about 0, unit spacing)
HINGE_THRESHOLDS = {"bernoulli_sq_hinge": (0.0, inf, inf), "ordinal_sq_hinge3": (-inf, -0.5, 0.5)}
OPT = {"adagrad": 0, "adam": 1}
STORE = {"f32": 0, "bf16": 1}
TERM = {0: "max_epochs", 1: "loss_increase", 2: "abs_tol", 3: "rel_tol", 4: "nonfinite",
        5: "holdout_increase"}                             # PMF_TERM_HOLDOUT (include/pmf_hip_holdout.h)
IMPUTE_BATCH, IMPUTE_LINK, IMPUTE_KEEP_OBSERVED = 1, 2, 4
DEBATCH_LINK, DEBATCH_FILL_MISSING = 1, 2
PARAM = {"X": 0, "Y": 1, "logsigma": 2, "mu": 3, "logdelta": 4, "theta": 5}
COMM_ID_BYTES = 128
PASS_EXTENTS_MAX = 16


class FitOpts(C.Structure):
    _fields_ = [("update_X", C.c_int32), ("update_Y", C.c_int32), ("update_col_layers", C.c_int32),
                ("frozen_layers", C.c_int32), ("frozen_regs", C.c_int32), ("max_epochs", C.c_int32),
                ("epoch", C.c_int32), ("tol_max_iters", C.c_int32), ("keep_trace", C.c_int32),
                ("verbosity", C.c_int32), ("print_iter", C.c_int32), ("reserved", C.c_int32),
                ("abs_tol", C.c_double), ("rel_tol", C.c_double), ("capacity", C.c_int64)]


class FitResult(C.Structure):
    _fields_ = [("term_code", C.c_int32), ("epochs", C.c_int32), ("n_trace", C.c_int32),
                ("trace_cap", C.c_int32), ("final_loss", C.c_double), ("loss_trace", C.POINTER(C.c_double)),
                ("seconds", C.c_double)]


class LbfgsOpts(C.Structure):
    _fields_ = [("m", C.c_int32), ("max_iter", C.c_int32), ("backtrack_max_iter", C.c_int32), ("keep_trace", C.c_int32),
                ("verbosity", C.c_int32), ("print_iter", C.c_int32), ("rel_tol", C.c_double), ("abs_tol", C.c_double),
                ("backtrack_shrinkage", C.c_double), ("c1", C.c_double), ("sy_min", C.c_double)]


class LbfgsResult(C.Structure):
    _fields_ = [("term_code", C.c_int32), ("iters", C.c_int32), ("loss_evals", C.c_int32), ("grad_evals", C.c_int32),
                ("resets", C.c_int32), ("n_trace", C.c_int32), ("trace_cap", C.c_int32), ("reserved", C.c_int32),
                ("final_loss", C.c_double), ("seconds", C.c_double), ("loss_trace", C.POINTER(C.c_double)),
                ("trial_trace", C.POINTER(C.c_int32)), ("flag_trace", C.POINTER(C.c_int32))]


class EmOpts(C.Structure):
    """pmf_em_opts"""
    _fields_ = [("update_priors", C.c_int32), ("max_iter", C.c_int32), ("verbosity", C.c_int32), ("reserved", C.c_int32),
                ("rtol", C.c_double)]


class EmResult(C.Structure):
    """pmf_em_result"""
    _fields_ = [("iters", C.c_int32), ("n_diffs", C.c_int32), ("diffs_cap", C.c_int32), ("reserved", C.c_int32),
                ("diffs", C.POINTER(C.c_double)), ("seconds", C.c_double)]


class SimOpts(C.Structure):
    """pmf_sim_opts"""
    _fields_ = [("seed", C.c_uint64), ("row_offset", C.c_int64), ("noise", C.c_float), ("frac_missing", C.c_float)]


class Csr(C.Structure):
    """pmf_csr: one sparse block in 0-based CSR with sorted rows."""
    _fields_ = [("n_rows", C.c_int64), ("n_cols", C.c_int64), ("rowptr", C.POINTER(C.c_int64)),
                ("col", C.POINTER(C.c_int32)), ("val", C.POINTER(C.c_float))]


# the header's name of every mirror
STRUCTS = {"pmf_fit_opts": FitOpts, "pmf_fit_result": FitResult, "pmf_lbfgs_opts": LbfgsOpts,
           "pmf_lbfgs_result": LbfgsResult, "pmf_em_opts": EmOpts, "pmf_em_result": EmResult, "pmf_sim_opts": SimOpts,
           "pmf_csr": Csr}

HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)    # pmf_host_allreduce_fn

# ---- the signatures: name -> (restype, argtypes), in the header's order ----------------------------------------------------
_P = C.POINTER
i, i64, u64, f32, f64 = C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double
ctx = vp = C.c_void_p                                      # pmf_ctx *; void *
pi, pi32, pi64, pu8, pf, pd = _P(i), _P(C.c_int32), _P(i64), _P(C.c_uint8), _P(f32), _P(f64)
pcsr, fit_o, sim_o = _P(Csr), _P(FitOpts), _P(SimOpts)


def _int(*argtypes):
    return C.c_int, list(argtypes)


_UPDATE_A_TAIL = (pf, pf, f32, f32, f32, pf, pf, i, i, f64, pd, pi, pf)    # alpha .. beta_out of the two update_A! entries

SIGNATURES = {
    "pmf_last_error": (C.c_char_p, []),
    "pmf_version": _int(),
    "pmf_device_count": _int(pi),
    "pmf_create": _int(i, _P(ctx)),
    "pmf_destroy": _int(ctx),
    "pmf_set_stream": _int(ctx, vp),
    "pmf_synchronize": _int(ctx),
    "pmf_set_data": _int(ctx, pf, i64, i64, i),
    "pmf_set_data_device": _int(ctx, vp, i64, i64, i),
    "pmf_set_factors": _int(ctx, pf, pf, i),
    "pmf_set_X": _int(ctx, pf, i),
    "pmf_set_Y": _int(ctx, pf, i),
    "pmf_get_factors": _int(ctx, pf, pf),
    "pmf_set_col_params": _int(ctx, pf, pf),
    "pmf_get_col_params": _int(ctx, pf, pf),
    "pmf_set_n_batch_views": _int(ctx, i),
    "pmf_set_batch_view": _int(ctx, i, i64, i64, i, pi32, pf, pf),
    "pmf_get_batch_view": _int(ctx, i, pf, pf),
    "pmf_set_noise": _int(ctx, i, pi64, pi64, pi32, pf),
    "pmf_set_noise_thresholds": _int(ctx, i, pi64, pi64, pf),
    "pmf_get_noise_thresholds": _int(ctx, pf),
    "pmf_clear_xreg": _int(ctx),
    "pmf_add_xreg_l2": _int(ctx, pf, f32),
    "pmf_add_xreg_group": _int(ctx, i, pi64, pi64, pf, f32),
    "pmf_clear_yreg": _int(ctx),
    "pmf_add_yreg_l2": _int(ctx, pf, f32),
    "pmf_add_yreg_group": _int(ctx, i, pi64, pi64, pf, f32),
    "pmf_add_yreg_ard": _int(ctx, i, pi64, pi64, pf, pf, f32),
    "pmf_add_yreg_fsard": _int(ctx, pf, pf, f32),
    "pmf_add_xreg_network": _int(ctx, i, pcsr, pcsr, pcsr, _P(pf), f32),
    "pmf_add_yreg_network": _int(ctx, i, pcsr, pcsr, pcsr, _P(pf), f32),
    "pmf_get_reg_network_state": _int(ctx, i, i, pf, pi),
    "pmf_add_xreg_l1": _int(ctx, pf, pu8, f32),
    "pmf_add_yreg_l1": _int(ctx, pf, pu8, f32),
    "pmf_set_layer_regs": _int(ctx, i, pi64, pi64, pf, pf, pf, pf, pf, pf, pf, pf),
    "pmf_set_optimizer": _int(ctx, i, f32, f32, f32, f32),
    "pmf_set_lr": _int(ctx, f32),
    "pmf_get_lr": _int(ctx, pf),
    "pmf_reset_optimizer_state": _int(ctx),
    "pmf_get_opt_state": _int(ctx, i, i, pf, pf),
    "pmf_fit": _int(ctx, fit_o, _P(FitResult)),
    "pmf_loss": _int(ctx, pd, pd, pd, pd),
    "pmf_fit_lbfgs": _int(ctx, _P(LbfgsOpts), _P(LbfgsResult)),
    "pmf_debug_lbfgs_direction": _int(ctx, i, pf, pf, pf, pf, pf, pf, pf, pf),
    "pmf_epoch_begin": _int(ctx, fit_o),
    "pmf_epoch_step_local": _int(ctx, fit_o),
    "pmf_epoch_step_shared": _int(ctx, fit_o),
    "pmf_epoch_loss": _int(ctx, pd, pd),
    "pmf_comm_get_unique_id": _int(vp),
    "pmf_comm_init": _int(ctx, i, i, vp),
    "pmf_comm_init_host": _int(ctx, i, i, HOST_ALLREDUCE_FN, vp),
    "pmf_comm_destroy": _int(ctx),
    "pmf_comm_set_chunks": _int(ctx, i),
    "pmf_comm_allreduce": _int(ctx, vp, i64, i, i),
    "pmf_comm_info": _int(ctx, pi, pi, pi, pi, pi, pi64),
    "pmf_debug_last_path": _int(ctx, pi, pi, pi, pi, pi64),
    "pmf_debug_plain_table": _int(ctx, pi32, i64, pi64, pi64),
    "pmf_debug_last_kernel": _int(ctx, pi),
    "pmf_debug_pass_extents": _int(ctx, i, i, pi64, i, _P(C.c_char_p), pi64, pi64, pi),
    "pmf_debug_live_bytes": _int(pi64, pi64),
    "pmf_grad_device_ptr": _int(ctx, i, _P(vp), pi64),
    "pmf_get_grad": _int(ctx, i, i, pf),
    "pmf_forward": _int(ctx, pf),
    "pmf_impute": _int(ctx, i, i64, i64, pf, i64),
    "pmf_impute_device": _int(ctx, i, i64, i64, pf, i64),
    "pmf_impute_entries": _int(ctx, i, i64, pi64, pi64, pf),
    "pmf_debug_impute_offset": _int(i64, i64, i64, pi64),
    "pmf_simulate_data": _int(ctx, sim_o, i64, i64, pf, i64),
    "pmf_simulate_data_device": _int(ctx, sim_o, i64, i64, pf, i64),
    "pmf_simulate_data_resident": _int(ctx, sim_o),
    "pmf_remove_batch_effect": _int(ctx, i, i64, i64, pf, i64, pf, i64),
    "pmf_remove_batch_effect_device": _int(ctx, i, i64, i64, pf, i64, pf, i64),
    "pmf_remove_batch_effect_entries": _int(ctx, i, i64, pi64, pi64, pf, pf),
    "pmf_stats": _int(ctx, i, pf, pf, pf, pf, pf, pf, pf),
    "pmf_stage_init_logsigma": _int(ctx),
    "pmf_stage_reweight_col_losses": _int(ctx, i64),
    "pmf_get_noise_weights": _int(ctx, pf),
    "pmf_stage_minimal_group_weights": _int(ctx, i64, pf),
    "pmf_stage_theta_delta_em": _int(ctx, _P(EmOpts), pf, pd, _P(EmResult)),
    "pmf_gram": _int(ctx, i, i, pi64, pi64, i, pd),
    "pmf_stage_lambda_max": _int(ctx, i, i, pi64, pi64, pd),
    "pmf_stage_whiten": _int(ctx, i64, i, pi64, pi64, pd, pd),
    "pmf_stage_rotate_by_svd": _int(ctx, pd, pd),
    "pmf_stage_reorder_by_importance": _int(ctx, pi32),
    "pmf_debug_postprocess_times": _int(ctx, pd, pd, pd),
    "pmf_fsard_update_A": _int(ctx, i64, i64, i, pf, *_UPDATE_A_TAIL),
    "pmf_fsard_update_A_csr": _int(ctx, i64, i64, i, pi64, pi32, pf, *_UPDATE_A_TAIL),
    "pmf_set_precision": _int(ctx, i),
    "pmf_get_precision": _int(ctx, pi, pi64),
    "pmf_kernel_time": _int(ctx, pd, pi64, i),
    "pmf_synth_data": _int(ctx, u64, f32, f32),
}

# every symbol include/pmf_hip.h declares (checked by tests/test_abi.py against the header and the .so)
EXPORTS = list(SIGNATURES)

# include/pmf_hip_thresholds.h, the extension header of the trainable squared-hinge thresholds, in its order
# (tests/test_threshold_cases.py compares this table with that header)
THRESHOLD_SIGNATURES = {
    "pmf_set_threshold_training": _int(ctx, i),
    "pmf_get_threshold_groups": _int(ctx, pi, pi64, pi64, i),
    "pmf_threshold_grad": _int(ctx, pf, pf),
    "pmf_get_threshold_state": _int(ctx, pf, pf, pf),
    "pmf_class_counts": _int(ctx, i, pi64, pi64, pi64),
    "pmf_debug_threshold_pass": _int(ctx, pi, pi, pi, pi64),
}


# include/pmf_hip_importance.h, the extension header of factor importance, in its order
# (tests/test_importance_cases.py compares this table with that header)
IMPORTANCE_CHAIN = 512                                     # PMF_IMPORTANCE_CHAIN
IMPORTANCE_SIGNATURES = {
    "pmf_factor_importance": _int(ctx, pd, pd, pd, pi64),
    "pmf_debug_factor_importance": _int(ctx, pi, pi, pi, pi, pi, pi, pi, pi, pi64),
}


# include/pmf_hip_holdout.h, the extension header of the hold-out entries, in its order
# (tests/test_holdout_cases.py compares this table and the struct with that header)
TERM_HOLDOUT = 5                                           # PMF_TERM_HOLDOUT


class HoldoutOpts(C.Structure):
    """pmf_holdout_opts"""
    _fields_ = [("every", C.c_int32), ("patience", C.c_int32), ("restore_best", C.c_int32), ("reserved", C.c_int32),
                ("min_delta", C.c_double)]


HOLDOUT_STRUCTS = {"pmf_holdout_opts": HoldoutOpts}
HOLDOUT_SIGNATURES = {
    "pmf_set_holdout": _int(ctx, i64, pi64, pi64, pi64),
    "pmf_clear_holdout": _int(ctx, i),
    "pmf_get_holdout": _int(ctx, pi64, pi64, pi64, pf, i64),
    "pmf_holdout_loss": _int(ctx, pd, pd, pi64),
    "pmf_debug_holdout_pass": _int(ctx, pi, pi, pi64),
    "pmf_set_holdout_tracking": _int(ctx, _P(HoldoutOpts)),
    "pmf_get_holdout_trace": _int(ctx, pi, pi, pd, pi32, pd, i),
}


def bind(lib):
    """Installs SIGNATURES and the extension headers' tables on a CDLL.  AttributeError if a declared symbol is not
    exported."""
    for name, (restype, argtypes) in {**SIGNATURES, **THRESHOLD_SIGNATURES, **IMPORTANCE_SIGNATURES,
                                      **HOLDOUT_SIGNATURES}.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib
