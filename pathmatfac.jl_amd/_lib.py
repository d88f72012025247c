"""ctypes binding of libpmf_hip.so (include/pmf_hip.h).

This is the Python counterpart of the Julia `ccall` shim (julia/PathMatFacHIP.jl): it marshals numpy arrays
in the reference's conventions (column-major matrices, 1-based inclusive ranges) to the C ABI.  There is NO
CPU fallback: if the shared library is missing or a call fails, a PMFError is raised.

The header's mirror -- structs, constants and the signature of every function -- is _abi.py; load_library installs the
signatures, so the calls below hand plain Python numbers over and ctypes converts them to the declared types.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

from ._abi import (COMM_ID_BYTES, DEBATCH_FILL_MISSING, DEBATCH_LINK, EXPORTS, HINGE_THRESHOLDS,  # noqa: F401
                   HOST_ALLREDUCE_FN, IMPUTE_BATCH, IMPUTE_KEEP_OBSERVED, IMPUTE_LINK, NOISE, OPT, PARAM, PASS_EXTENTS_MAX,
                   STORE, TERM, Csr, EmOpts, EmResult, FitOpts, FitResult, HoldoutOpts, LbfgsOpts, LbfgsResult, SimOpts, bind)

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libpmf_hip.so"


class PMFError(RuntimeError):
    pass


def csr_arrays(A):
    """A scipy sparse matrix -> (shape, rowptr int64, col int32, val float32) as pmf_csr wants them."""
    import scipy.sparse as sp
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return (A.shape, np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float32))


def dense_to_csr(S):
    """A dense L x N_v array -> (rowptr int64 [L + 1], col int32, val float32): the 0-based CSR of its non-zero entries, by
    a row-major scan, so the columns of a row come out ascending (pmf_fsard_update_A_csr).  No scipy."""
    S = np.ascontiguousarray(S, dtype=np.float32)
    if S.ndim != 2:
        raise ValueError("dense_to_csr: S must be a matrix")
    L, Nv = S.shape
    flat = np.flatnonzero(S.ravel())                       # ascending = row by row, columns ascending within a row
    rowptr = np.zeros(L + 1, np.int64)
    if Nv:
        np.cumsum(np.bincount(flat // Nv, minlength=L), out=rowptr[1:])
        col = (flat % Nv).astype(np.int32)
    else:
        col = np.zeros(0, np.int32)
    return rowptr, col, S.ravel()[flat].astype(np.float32)


def comm_unique_id(lib_path=None):
    """ncclGetUniqueId through the library (call on ONE rank; hand the 128 bytes to every rank)."""
    lib = load_library(lib_path)
    buf = C.create_string_buffer(COMM_ID_BYTES)
    if lib.pmf_comm_get_unique_id(buf) != 0:
        raise PMFError(lib.pmf_last_error().decode())
    return buf.raw


def live_bytes(lib_path=None):
    """pmf_debug_live_bytes: (device, pinned) bytes the library holds in this process, over all of its contexts."""
    lib = load_library(lib_path)
    d, h = C.c_int64(0), C.c_int64(0)
    if lib.pmf_debug_live_bytes(C.byref(d), C.byref(h)) != 0:
        raise PMFError(lib.pmf_last_error().decode())
    return d.value, h.value


def device_count(lib_path=None):
    """HIP devices visible to this process (pmf_device_count)."""
    lib = load_library(lib_path)
    n = C.c_int(0)
    if lib.pmf_device_count(C.byref(n)) != 0:
        raise PMFError(lib.pmf_last_error().decode())
    return n.value


_lib = None


def load_library(path=None):
    """Loads libpmf_hip.so (does not touch the GPU) and declares every function's types.  Raises PMFError when it is
    missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise PMFError(f"{p} not found: build it with pathmatfac.jl_amd/csrc/build.sh "
                       "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64; a process must run ONE HIP runtime.  If torch is installed, load it
    # first so that libpmf_hip.so binds to the same runtime (loading the library first and torch later leaves
    # torch.cuda unusable).  A host without torch (the Julia shim) simply uses the system ROCm runtime.
    # PMF_NO_TORCH=1: a process that never uses torch (bench.py's ranks) keeps to ONE runtime, the system ROCm's.
    if os.environ.get("PMF_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = bind(C.CDLL(str(p)))  # AttributeError if a declared symbol is not exported
    _lib = lib
    return lib


_PF, _PD, _PI32, _PI64 = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_int32, C.c_int64))


def _f32(a, order="F"):
    return np.require(np.asarray(a, dtype=np.float32), requirements=["F" if order == "F" else "C", "A"])


def _fp(a):
    return a.ctypes.data_as(_PF) if a is not None else _PF()


def _dp(a):
    return a.ctypes.data_as(_PD)


def _i32p(a):
    return a.ctypes.data_as(_PI32)


def _i64p(a):
    return a.ctypes.data_as(_PI64)


def _at(addr, ptype=_PF):
    """A raw address (an int; None or 0 for NULL) as the pointer type the header declares for it."""
    return C.cast(addr, ptype)


def _flat(a):
    """None, a flat vector, or a list of per-view vectors -> one contiguous float32 vector."""
    if a is None:
        return None
    if isinstance(a, (list, tuple)) and len(a) and np.ndim(a[0]) > 0:
        a = np.concatenate([np.asarray(x, dtype=np.float32).ravel() for x in a])
    return _f32(np.asarray(a, dtype=np.float32).ravel())


def _ranges(ranges):
    s = np.ascontiguousarray([r[0] for r in ranges], dtype=np.int64)
    e = np.ascontiguousarray([r[1] for r in ranges], dtype=np.int64)
    return s, e


class Context:
    """One pmf_ctx = one GPU.  Mirrors `gpu(model)`: owns the device copies of data and parameters."""

    def __init__(self, device=0, lib_path=None):
        self.lib = load_library(lib_path)
        self._h = C.c_void_p()
        self._chk(self.lib.pmf_create(device, C.byref(self._h)))
        self.M = self.N = self.K = 0
        self.view_shapes = []
        self.n_noise_ranges = 0     # ranges of the last set_noise (the library forgets them with a new data shape: so does this)
        self.holdout_tracking = dict(every=0)   # the options of the last set_holdout_tracking

    def _chk(self, rc):
        if rc != 0:
            raise PMFError(self.lib.pmf_last_error().decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.lib.pmf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- data / parameters
    def set_stream(self, stream_ptr):
        """Runs the library's kernels on the caller's HIP stream, e.g. torch.cuda.current_stream().cuda_stream, so that
        they order with the caller's collectives.  torch reports its DEFAULT stream as handle 0, which pmf_set_stream
        reads as "back to the library's own (non-blocking) stream" -- kernels there would NOT be ordered with work torch
        or RCCL issue behind the default stream -- so 0 is passed on as hipStreamLegacy, the legacy default stream itself."""
        HIP_STREAM_LEGACY = 1   # hip_runtime_api.h: #define hipStreamLegacy ((hipStream_t)1)
        self._chk(self.lib.pmf_set_stream(self._h, stream_ptr if stream_ptr else HIP_STREAM_LEGACY))
        self._stream_adopted = True

    def use_own_stream(self):
        """Back to the library's own non-blocking stream (pmf_set_stream(ctx, NULL))."""
        self._chk(self.lib.pmf_set_stream(self._h, None))
        self._stream_adopted = False

    def synchronize(self):
        self._chk(self.lib.pmf_synchronize(self._h))

    def set_data(self, D, store="f32"):
        """store = "bf16": the device copy of D is kept as bfloat16 (PMF_STORE_BF16; read by the split-bf16 data pass)."""
        D = _f32(D)
        if D.shape != (self.M, self.N):
            self.n_noise_ranges = 0
        self.M, self.N = D.shape
        self._chk(self.lib.pmf_set_data(self._h, _fp(D), self.M, self.N, STORE[store]))

    def set_data_device(self, ptr, M, N, store="f32"):
        if (int(M), int(N)) != (self.M, self.N):
            self.n_noise_ranges = 0
        self.M, self.N = int(M), int(N)
        self._chk(self.lib.pmf_set_data_device(self._h, _at(ptr, C.c_void_p), self.M, self.N, STORE[store]))

    def set_factors(self, X, Y):
        X, Y = _f32(X), _f32(Y)
        K = X.shape[0]
        if X.shape != (K, self.M) or Y.shape != (K, self.N):
            raise PMFError(f"factor shapes {X.shape}, {Y.shape} do not match data {self.M} x {self.N}")
        self._chk(self.lib.pmf_set_factors(self._h, _fp(X), _fp(Y), K))
        self.K = K   # (after the call: a refused K leaves the context, and this mirror of it, at the factors it had)

    def set_X(self, X):
        X = _f32(X)
        self._chk(self.lib.pmf_set_X(self._h, _fp(X), X.shape[0]))

    def set_Y(self, Y):
        Y = _f32(Y)
        self._chk(self.lib.pmf_set_Y(self._h, _fp(Y), Y.shape[0]))

    def get_factors(self):
        X = np.zeros((self.K, self.M), np.float32, order="F")
        Y = np.zeros((self.K, self.N), np.float32, order="F")
        self._chk(self.lib.pmf_get_factors(self._h, _fp(X), _fp(Y)))
        return X, Y

    def set_col_params(self, logsigma=None, mu=None):
        ls = None if logsigma is None else _f32(logsigma)
        m = None if mu is None else _f32(mu)
        self._chk(self.lib.pmf_set_col_params(self._h, _fp(ls), _fp(m)))

    def get_col_params(self):
        ls = np.zeros(self.N, np.float32)
        mu = np.zeros(self.N, np.float32)
        self._chk(self.lib.pmf_get_col_params(self._h, _fp(ls), _fp(mu)))
        return ls, mu

    def set_batch_views(self, views):
        """views: list of dict(start1, stop1, batch_of_row (M, 0-based), logdelta (nb x Nv), theta (nb x Nv))."""
        self._chk(self.lib.pmf_set_n_batch_views(self._h, len(views)))
        self.view_shapes = []
        for v, b in enumerate(views):
            ld, th = _f32(b["logdelta"]), _f32(b["theta"])
            nb, Nv = ld.shape
            bor = np.ascontiguousarray(b["batch_of_row"], dtype=np.int32)
            if bor.shape != (self.M,):
                raise PMFError("batch_of_row must have one entry per row")
            self._chk(self.lib.pmf_set_batch_view(self._h, v, b["start1"], b["stop1"], nb, _i32p(bor), _fp(ld), _fp(th)))
            self.view_shapes.append((nb, Nv))

    def update_batch_values(self, v, start1, stop1, batch_of_row, logdelta, theta):
        ld, th = _f32(logdelta), _f32(theta)
        bor = np.ascontiguousarray(batch_of_row, dtype=np.int32)
        self._chk(self.lib.pmf_set_batch_view(self._h, v, start1, stop1, ld.shape[0], _i32p(bor), _fp(ld), _fp(th)))

    def get_batch_view(self, v):
        nb, Nv = self.view_shapes[v]
        ld = np.zeros((nb, Nv), np.float32, order="F")
        th = np.zeros((nb, Nv), np.float32, order="F")
        self._chk(self.lib.pmf_get_batch_view(self._h, v, _fp(ld), _fp(th)))
        return ld, th

    def set_noise(self, ranges, kinds, weights=None):
        s, e = _ranges(ranges)
        k = np.ascontiguousarray([NOISE[x] if isinstance(x, str) else int(x) for x in kinds], dtype=np.int32)
        w = None if weights is None else _f32(weights)
        self._chk(self.lib.pmf_set_noise(self._h, len(k), _i64p(s), _i64p(e), _i32p(k), _fp(w)))
        self.n_noise_ranges = len(k)
        # a range named ordinal_sq_hinge3 gets that model's default thresholds (the library's default for kind 3 is bernoulli_sq_hinge's)
        named = [(r, HINGE_THRESHOLDS[x]) for r, x in zip(ranges, kinds) if x == "ordinal_sq_hinge3"]
        if named:
            self.set_noise_thresholds([r for r, _ in named], [t for _, t in named])

    def set_noise_thresholds(self, ranges, thresholds):
        """pmf_set_noise_thresholds: (t0, t1, t2), t0 <= t1 <= t2 and each possibly +-inf, for every listed (1-based, inclusive)
        column range; every column of a range must be of kind 3 (bernoulli_sq_hinge / ordinal_sq_hinge3)."""
        s, e = _ranges(ranges)
        t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(len(s), 3))
        self._chk(self.lib.pmf_set_noise_thresholds(self._h, len(s), _i64p(s), _i64p(e), _fp(t)))

    def get_noise_thresholds(self):
        """pmf_get_noise_thresholds: (N, 3) thresholds, NaN for the columns of the other kinds."""
        t = np.zeros((self.N, 3), np.float32)
        self._chk(self.lib.pmf_get_noise_thresholds(self._h, _fp(t)))
        return t

    # ---- regularizers
    def clear_xreg(self):
        self._chk(self.lib.pmf_clear_xreg(self._h))

    def clear_yreg(self):
        self._chk(self.lib.pmf_clear_yreg(self._h))

    def add_reg_l2(self, which, w, p=1.0):
        w = _f32(np.asarray(w).ravel())
        f = self.lib.pmf_add_xreg_l2 if which == "X" else self.lib.pmf_add_yreg_l2
        self._chk(f(self._h, _fp(w), p))

    def add_reg_group(self, which, ranges, w, p=1.0):
        s, e = _ranges(ranges)
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float32))  # (n_groups, K), K contiguous
        if w.shape != (len(s), self.K):
            raise PMFError(f"group weights must be (n_groups, K) = ({len(s)}, {self.K}); got {w.shape}")
        f = self.lib.pmf_add_xreg_group if which == "X" else self.lib.pmf_add_yreg_group
        self._chk(f(self._h, len(s), _i64p(s), _i64p(e), _fp(w), p))

    def add_yreg_ard(self, ranges, alpha, beta, p=1.0):
        s, e = _ranges(ranges)
        a, b = _f32(np.asarray(alpha).ravel()), _f32(np.asarray(beta).ravel())
        self._chk(self.lib.pmf_add_yreg_ard(self._h, len(s), _i64p(s), _i64p(e), _fp(a), _fp(b), p))

    def add_yreg_fsard(self, alpha, beta, p=1.0):
        a, b = _f32(np.asarray(alpha).ravel()), _f32(beta)
        if a.shape != (self.N,) or b.shape != (self.K, self.N):
            raise PMFError("FeatureSetARD: alpha must be N, beta K x N")
        self._chk(self.lib.pmf_add_yreg_fsard(self._h, _fp(a), _fp(b), p))

    def add_reg_network(self, which, AA, AB, BB, u0=None, p=1.0):
        """NetworkRegularizer: per factor the scipy sparse blocks AA (n x n), AB (n x v_k), BB (v_k x v_k); u0: per factor
        the initial u_k (the reference's x_virtual) or None for zeros."""
        K = len(AA)
        keep, blocks = [], []
        for mats in (AA, AB, BB):
            arr = (Csr * K)()
            for k, A in enumerate(mats):
                shape, rp, col, val = csr_arrays(A)
                keep.append((rp, col, val))
                arr[k] = Csr(shape[0], shape[1], _i64p(rp), _i32p(col), _fp(val))
            blocks.append(arr)
        up = None
        if u0 is not None:
            us = [_f32(np.asarray(u).ravel()) for u in u0]
            for k, (u, B) in enumerate(zip(us, BB)):
                if u.shape != (B.shape[0],):
                    raise PMFError(f"network regularizer: u0[{k}] has {u.shape[0]} entries, BB[{k}] {B.shape[0]} rows")
            keep.append(us)
            up = (_PF * K)(*[_fp(u) for u in us])
        f = self.lib.pmf_add_xreg_network if which == "X" else self.lib.pmf_add_yreg_network
        self._chk(f(self._h, K, blocks[0], blocks[1], blocks[2], up, p))
        if not hasattr(self, "_net_v"):
            self._net_v = {}
        self._net_v[which] = [int(B.shape[0]) for B in BB]

    def get_reg_network_state(self, which, k):
        """(u_k, CG iterations of the last solve) of factor k (0-based) of the network term on X / Y."""
        v = getattr(self, "_net_v", {}).get(which)
        n = v[k] if v is not None and 0 <= k < len(v) else 0
        u = np.zeros(n, np.float32)
        it = C.c_int(0)
        self._chk(self.lib.pmf_get_reg_network_state(self._h, PARAM[which], k, _fp(u) if n else None, C.byref(it)))
        return u, it.value

    def add_reg_l1(self, which, w, mask=None, p=1.0):
        """L1Regularizer (mask None) / SelectiveL1Reg (mask = l1_idx, K x n booleans)."""
        w = _f32(np.asarray(w).ravel())
        n = self.M if which == "X" else self.N
        if w.shape != (self.K,):
            raise PMFError(f"L1 weights must have K = {self.K} entries; got {w.shape}")
        mp = None
        if mask is not None:
            m = np.require(np.asarray(mask, dtype=np.uint8), requirements=["F", "A"])
            if m.shape != (self.K, n):
                raise PMFError(f"L1 mask must be K x n = ({self.K}, {n}); got {m.shape}")
            mp = m.ctypes.data_as(C.POINTER(C.c_uint8))
        f = self.lib.pmf_add_xreg_l1 if which == "X" else self.lib.pmf_add_yreg_l1
        self._chk(f(self._h, _fp(w), mp, p))

    def set_layer_regs(self, ranges=None, w_logsigma=None, c_logsigma=None, w_mu=None, c_mu=None,
                       w_logdelta=None, c_logdelta=None, w_theta=None, c_theta=None):
        ranges = ranges or []
        s, e = _ranges(ranges) if ranges else (np.zeros(1, np.int64), np.zeros(1, np.int64))
        arrs = [_flat(a) for a in (w_logsigma, c_logsigma, w_mu, c_mu, w_logdelta, c_logdelta, w_theta, c_theta)]
        self._keep = arrs
        self._chk(self.lib.pmf_set_layer_regs(self._h, len(ranges), _i64p(s), _i64p(e), *[_fp(a) for a in arrs]))

    # ---- optimizer
    def set_optimizer(self, kind="adagrad", lr=1.0, eps=1e-8, beta1=0.9, beta2=0.999):
        self._chk(self.lib.pmf_set_optimizer(self._h, OPT[kind], lr, eps, beta1, beta2))

    def set_lr(self, lr):
        self._chk(self.lib.pmf_set_lr(self._h, lr))

    def get_lr(self):
        v = C.c_float(0)
        self._chk(self.lib.pmf_get_lr(self._h, C.byref(v)))
        return v.value

    def reset_optimizer_state(self):
        self._chk(self.lib.pmf_reset_optimizer_state(self._h))

    # ---- fitting
    @staticmethod
    def make_opts(update_X=False, update_Y=False, update_col_layers=False, frozen_layers=0, frozen_regs=0,
                  max_epochs=1000, epoch=1, tol_max_iters=3, keep_trace=True, verbosity=0, print_iter=10,
                  abs_tol=1e-9, rel_tol=1e-6, capacity=10 ** 8):
        o = FitOpts()
        o.update_X, o.update_Y, o.update_col_layers = int(update_X), int(update_Y), int(update_col_layers)
        o.frozen_layers, o.frozen_regs = int(frozen_layers), int(frozen_regs)
        o.max_epochs, o.epoch, o.tol_max_iters = int(max_epochs), int(epoch), int(tol_max_iters)
        o.keep_trace, o.verbosity, o.print_iter = int(keep_trace), int(verbosity), int(print_iter)
        o.abs_tol, o.rel_tol, o.capacity = float(abs_tol), float(rel_tol), int(capacity)
        return o

    def fit(self, update_noise_models=False, **kw):
        """pmf_fit.  update_noise_models: the squared-hinge thresholds train in this call (set_threshold_training for its
        duration; include/pmf_hip_thresholds.h); False leaves the context's switch as it is."""
        o = self.make_opts(**kw)
        cap = max(o.max_epochs - o.epoch + 1, 1)
        trace = np.zeros(cap, np.float64)
        r = FitResult()
        r.trace_cap = cap
        r.loss_trace = _dp(trace)
        if update_noise_models:
            self.set_threshold_training(True)
        try:
            self._chk(self.lib.pmf_fit(self._h, C.byref(o), C.byref(r)))
        finally:
            if update_noise_models:
                self.set_threshold_training(False)
        h = {"term_code": TERM[r.term_code], "epochs": r.epochs, "loss": trace[:r.n_trace].copy(),
             "final_loss": r.final_loss, "seconds": r.seconds}
        ho = self.get_holdout_trace()
        if len(ho["epochs"]):                          # hold-out tracking ran in this fit (include/pmf_hip_holdout.h)
            h.update(holdout_loss=ho["losses"], holdout_epochs=ho["epochs"], best_epoch=ho["best_epoch"])
        return h

    # ---- hold-out entries (include/pmf_hip_holdout.h)
    def set_holdout(self, rows1, cols1):
        """pmf_set_holdout: holds the 1-based entries out of the resident data; returns how many were observed and are held."""
        r, c, _ = self._entries("set_holdout", rows1, cols1)
        n = C.c_int64(0)
        self._chk(self.lib.pmf_set_holdout(self._h, len(r), _i64p(r), _i64p(c), C.byref(n)))
        return n.value

    def clear_holdout(self, restore=True):
        self._chk(self.lib.pmf_clear_holdout(self._h, int(bool(restore))))

    def get_holdout(self):
        """pmf_get_holdout: (rows1, cols1, values) in the library's (column, row) order."""
        n = C.c_int64(0)
        self._chk(self.lib.pmf_get_holdout(self._h, C.byref(n), None, None, None, 0))
        r, c, v = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64), np.zeros(n.value, np.float32)
        if n.value:
            self._chk(self.lib.pmf_get_holdout(self._h, C.byref(n), _i64p(r), _i64p(c), _fp(v), n.value))
        return r, c, v

    def holdout_loss(self):
        """pmf_holdout_loss at the current parameters: (total, loss_col (N,) float64, n_col (N,) int64)."""
        t, lc, nc = C.c_double(0), np.zeros(self.N, np.float64), np.zeros(self.N, np.int64)
        self._chk(self.lib.pmf_holdout_loss(self._h, C.byref(t), _dp(lc), _i64p(nc)))
        return t.value, lc, nc

    def debug_holdout_pass(self):
        """pmf_debug_holdout_pass: dict(n_units, grid, passes) of the last hold-out pass."""
        a, b, p = C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(self.lib.pmf_debug_holdout_pass(self._h, C.byref(a), C.byref(b), C.byref(p)))
        return dict(n_units=a.value, grid=b.value, passes=p.value)

    def set_holdout_tracking(self, every=0, patience=0, min_delta=0.0, restore_best=False):
        """pmf_set_holdout_tracking (sticky): every = 0 turns tracking off.  holdout_tracking holds what was last set."""
        o = HoldoutOpts(int(every), int(patience), int(bool(restore_best)), 0, float(min_delta))
        self._chk(self.lib.pmf_set_holdout_tracking(self._h, C.byref(o) if every else None))
        self.holdout_tracking = dict(every=int(every), patience=int(patience), min_delta=float(min_delta),
                                     restore_best=bool(restore_best)) if every else dict(every=0)

    def holdout_count(self):
        """The number of entries the context holds out (0: no set)."""
        n = C.c_int64(0)
        self._chk(self.lib.pmf_get_holdout(self._h, C.byref(n), None, None, None, 0))
        return n.value

    def get_holdout_trace(self):
        """pmf_get_holdout_trace: dict(epochs, losses, best_epoch, best_loss) of the last fit's evaluations."""
        n, be, bl = C.c_int(0), C.c_int(0), C.c_double(0)
        self._chk(self.lib.pmf_get_holdout_trace(self._h, C.byref(n), C.byref(be), C.byref(bl), None, None, 0))
        ep, ls = np.zeros(n.value, np.int32), np.zeros(n.value, np.float64)
        if n.value:
            self._chk(self.lib.pmf_get_holdout_trace(self._h, C.byref(n), C.byref(be), C.byref(bl), _i32p(ep), _dp(ls), n.value))
        return dict(epochs=ep, losses=ls, best_epoch=be.value, best_loss=bl.value)

    # ---- trainable squared-hinge thresholds (include/pmf_hip_thresholds.h)
    def set_threshold_training(self, on):
        self._chk(self.lib.pmf_set_threshold_training(self._h, int(bool(on))))

    def get_threshold_groups(self):
        """The 1-based inclusive column ranges whose thresholds train as one triple (the all-kind-3 noise ranges)."""
        n = C.c_int(0)
        self._chk(self.lib.pmf_get_threshold_groups(self._h, C.byref(n), None, None, 0))
        s, e = np.zeros(max(n.value, 1), np.int64), np.zeros(max(n.value, 1), np.int64)
        self._chk(self.lib.pmf_get_threshold_groups(self._h, C.byref(n), _i64p(s), _i64p(e), n.value))
        return [(int(a), int(b)) for a, b in zip(s[:n.value], e[:n.value])]

    def threshold_grad(self, per_column=True):
        """pmf_threshold_grad: (groups x 3, N x 3 or None) -- one threshold pass at the current parameters."""
        g = np.zeros((len(self.get_threshold_groups()), 3), np.float32)
        gc = np.zeros((self.N, 3), np.float32) if per_column else None
        self._chk(self.lib.pmf_threshold_grad(self._h, _fp(g), _fp(gc)))
        return g, gc

    def get_threshold_state(self):
        """pmf_get_threshold_state: dict(thr, acc, mom), each groups x 3."""
        out = {k: np.zeros((len(self.get_threshold_groups()), 3), np.float32) for k in ("thr", "acc", "mom")}
        self._chk(self.lib.pmf_get_threshold_state(self._h, _fp(out["thr"]), _fp(out["acc"]), _fp(out["mom"])))
        return out

    def class_counts(self, ranges):
        """pmf_class_counts: (ranges x 4) int64 counts of the observed entries of class 0..3 in the local rows."""
        s, e = _ranges(ranges)
        n = np.zeros((len(s), 4), np.int64)
        self._chk(self.lib.pmf_class_counts(self._h, len(s), _i64p(s), _i64p(e), _i64p(n)))
        return n

    def debug_threshold_pass(self):
        """pmf_debug_threshold_pass: dict(n_tiles, n_units, grid, passes) of the last threshold pass."""
        a, b, c, p = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        self._chk(self.lib.pmf_debug_threshold_pass(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(p)))
        return dict(n_tiles=a.value, n_units=b.value, grid=c.value, passes=p.value)

    # ---- factor importance (include/pmf_hip_importance.h)
    def factor_importance(self, delta=True, full=True, null=True, n_obs=True):
        """pmf_factor_importance at the current parameters over the local rows: (delta (K, N) float64, full (N,), null (N,),
        n_obs (N,) int64).  An output switched off is passed as NULL and returned as None."""
        K, N = self.K, self.N
        d = np.zeros((N, K), np.float64) if delta else None            # factor fastest: delta[j * K + k]
        f, z = (np.zeros(N, np.float64) if w else None for w in (full, null))
        n = np.zeros(N, np.int64) if n_obs else None
        self._chk(self.lib.pmf_factor_importance(self._h, _dp(d) if delta else None, _dp(f) if full else None,
                                                 _dp(z) if null else None, _i64p(n) if n_obs else None))
        return (np.ascontiguousarray(d.T) if delta else None), f, z, n

    def debug_factor_importance(self):
        """pmf_debug_factor_importance: dict(kb, nw, db, ranges, n_units, grid, launches, flushes, calls) of the last call."""
        v = [C.c_int(0) for _ in range(8)]
        calls = C.c_int64(0)
        self._chk(self.lib.pmf_debug_factor_importance(self._h, *[C.byref(x) for x in v], C.byref(calls)))
        names = ("kb", "nw", "db", "ranges", "n_units", "grid", "launches", "flushes")
        return dict(zip(names, (x.value for x in v)), calls=calls.value)

    def loss(self):
        """pmf_loss: dict(total, data, xreg, yreg) at the current parameters (full_loss, src/fit_lbfgs.jl:3-8)."""
        v = [C.c_double(0) for _ in range(4)]
        self._chk(self.lib.pmf_loss(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("total", "data", "xreg", "yreg"), (x.value for x in v)))

    def fit_lbfgs(self, m=10, max_iter=1000, backtrack_max_iter=100, rel_tol=1e-9, abs_tol=1e-6, backtrack_shrinkage=0.8,
                  c1=1e-4, sy_min=1e-4, keep_trace=True, verbosity=0, print_iter=10):
        """pmf_fit_lbfgs (fit_lbfgs!, src/fit_lbfgs.jl:170-243).  Returns the result fields and the three traces."""
        o = LbfgsOpts(int(m), int(max_iter), int(backtrack_max_iter), int(keep_trace), int(verbosity), int(print_iter),
                      float(rel_tol), float(abs_tol), float(backtrack_shrinkage), float(c1), float(sy_min))
        cap = max(int(max_iter), 1)
        loss, trials, flags = np.zeros(cap, np.float64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        r = LbfgsResult()
        r.trace_cap = cap
        r.loss_trace, r.trial_trace, r.flag_trace = _dp(loss), _i32p(trials), _i32p(flags)
        self._chk(self.lib.pmf_fit_lbfgs(self._h, C.byref(o), C.byref(r)))
        n = r.n_trace
        return {"term_code": TERM[r.term_code], "iters": r.iters, "loss": loss[:n].copy(), "trials": trials[:n].copy(),
                "flags": flags[:n].copy(), "final_loss": r.final_loss, "loss_evals": r.loss_evals,
                "grad_evals": r.grad_evals, "resets": r.resets, "seconds": r.seconds}

    def debug_lbfgs_direction(self, s_pairs, y_pairs, g):
        """pmf_debug_lbfgs_direction: s_pairs / y_pairs are lists (newest first) of (X-part K x M, Y-part K x N); g likewise
        one such pair.  Returns p = (K x M, K x N)."""
        n = len(s_pairs)
        def stack(pairs, i, cols):
            if not pairs:
                return None
            return np.ascontiguousarray(np.stack([np.asfortranarray(q[i], dtype=np.float32).ravel(order="F") for q in pairs]))
        sX, sY, yX, yY = stack(s_pairs, 0, self.M), stack(s_pairs, 1, self.N), stack(y_pairs, 0, self.M), stack(y_pairs, 1, self.N)
        gX, gY = _f32(g[0]), _f32(g[1])
        pX = np.zeros((self.K, self.M), np.float32, order="F")
        pY = np.zeros((self.K, self.N), np.float32, order="F")
        self._chk(self.lib.pmf_debug_lbfgs_direction(self._h, n, _fp(sX), _fp(sY), _fp(yX), _fp(yY), _fp(gX), _fp(gY),
                                                     _fp(pX), _fp(pY)))
        return pX, pY

    def epoch_begin(self, o):
        self._chk(self.lib.pmf_epoch_begin(self._h, C.byref(o)))

    def epoch_step_local(self, o):
        self._chk(self.lib.pmf_epoch_step_local(self._h, C.byref(o)))

    def epoch_step_shared(self, o):
        self._chk(self.lib.pmf_epoch_step_shared(self._h, C.byref(o)))

    def epoch_loss(self):
        a, b = C.c_double(0), C.c_double(0)
        self._chk(self.lib.pmf_epoch_loss(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def grad_device_ptr(self, which):
        p, n = C.c_void_p(), C.c_int64(0)
        self._chk(self.lib.pmf_grad_device_ptr(self._h, PARAM[which], C.byref(p), C.byref(n)))
        return p.value, n.value

    def _param_shape(self, which, view):
        """The shape of a parameter group (view: the batch view of logdelta / theta)."""
        if which in ("X", "Y"):
            return (self.K, self.M if which == "X" else self.N)
        return (self.N,) if which in ("logsigma", "mu") else self.view_shapes[view]

    def get_grad(self, which, view=0):
        out = np.zeros(self._param_shape(which, view), np.float32, order="F")
        self._chk(self.lib.pmf_get_grad(self._h, PARAM[which], view, _fp(out)))
        return out

    def get_opt_state(self, which, view=0):
        """(acc, mom) of a parameter group in the parameter's shape (pmf_get_opt_state)."""
        shape = self._param_shape(which, view)
        acc, mom = np.zeros(shape, np.float32, order="F"), np.zeros(shape, np.float32, order="F")
        self._chk(self.lib.pmf_get_opt_state(self._h, PARAM[which], view, _fp(acc), _fp(mom)))
        return acc, mom

    def _fsard_call(self, entry, start1, stop1, L, Nv, s_args, alpha, lam, alpha0, v0, lr, ssq_grad, max_epochs, term_iter,
                    atol):
        """What the two update_A! entries share: alpha, lambda and ssq_grad as the library takes them, the outputs, the call
        (s_args: the entry's form of S) and the returned tuple."""
        al = np.ascontiguousarray(alpha, dtype=np.float32)
        lm = np.ascontiguousarray(lam, dtype=np.float32)
        if ssq_grad.dtype != np.float32 or not ssq_grad.flags.c_contiguous or ssq_grad.shape != (L, self.K):
            raise PMFError("ssq_grad must be a C-contiguous float32 L x K array")
        A = np.zeros((L, self.K), np.float32)
        beta = np.zeros((self.K, max(Nv, 0)), np.float32, order="F")
        best, ep = C.c_double(0), C.c_int(0)
        self._chk(entry(self._h, start1, stop1, L, *s_args, _fp(al), _fp(lm), alpha0, v0, lr, _fp(ssq_grad), _fp(A),
                        int(max_epochs), int(term_iter), atol, C.byref(best), C.byref(ep), _fp(beta)))
        return A, beta, best.value, ep.value

    def fsard_update_A(self, start1, stop1, S, alpha, lam, alpha0, v0, lr, ssq_grad, max_epochs=1000, term_iter=20,
                       atol=1e-5):
        """update_A! for one view on the device (pmf_fsard_update_A).  S: L x Nv, ssq_grad: L x K (updated in place).
        Returns (A [L x K], beta [K x Nv], best_loss, epochs_run)."""
        S = np.ascontiguousarray(S, dtype=np.float32)
        L, Nv = S.shape
        if Nv != stop1 - start1 + 1:
            raise PMFError("S must have one column per column of the view")
        return self._fsard_call(self.lib.pmf_fsard_update_A, start1, stop1, L, Nv, (_fp(S),), alpha, lam, alpha0, v0, lr,
                                ssq_grad, max_epochs, term_iter, atol)

    def fsard_update_A_csr(self, start1, stop1, S, alpha, lam, alpha0, v0, lr, ssq_grad, max_epochs=1000, term_iter=20,
                           atol=1e-5):
        """update_A! for one view on a sparse S, without the L x K bound of fsard_update_A (pmf_fsard_update_A_csr).
        S: a dense L x Nv array, or the (rowptr, col, val) triple of its 0-based CSR (dense_to_csr); ssq_grad: L x K
        (updated in place).  Returns (A [L x K], beta [K x Nv], best_loss, epochs_run)."""
        Nv = stop1 - start1 + 1
        if isinstance(S, (tuple, list)):
            if len(S) != 3:
                raise PMFError("S must be a dense L x Nv array or a (rowptr, col, val) triple")
            rowptr, col, val = S
        else:
            S = np.asarray(S)
            if S.ndim != 2 or S.shape[1] != Nv:
                raise PMFError("S must have one column per column of the view")
            rowptr, col, val = dense_to_csr(S)
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float32)
        L = rowptr.size - 1
        if L < 1 or col.shape != val.shape or col.ndim != 1 or rowptr[-1] != col.size:
            raise PMFError("S: rowptr must have L + 1 >= 2 entries and end at the length of col and val")
        if col.size == 0:                                  # (a pointer the library may look at, never through)
            col, val = np.zeros(1, np.int32), np.zeros(1, np.float32)
        al = np.ascontiguousarray(alpha, dtype=np.float32)
        lm = np.ascontiguousarray(lam, dtype=np.float32)
        if al.size != Nv or lm.size != self.K:
            raise PMFError("alpha must have one entry per column of the view and lambda one per factor")
        return self._fsard_call(self.lib.pmf_fsard_update_A_csr, start1, stop1, L, Nv, (_i64p(rowptr), _i32p(col), _fp(val)),
                                al, lm, alpha0, v0, lr, ssq_grad, max_epochs, term_iter, atol)

    def forward(self):
        Z = np.zeros((self.M, self.N), np.float32, order="F")
        self._chk(self.lib.pmf_forward(self._h, _fp(Z)))
        return Z

    # ---- what the predictions, the simulated data and the batch-corrected data share
    def _rows(self, row_start1, row_stop1):
        """-> (row_stop1, defaulting to the last row; the number of rows of the 1-based inclusive range, possibly <= 0)."""
        row_stop1 = self.M if row_stop1 is None else int(row_stop1)
        return row_stop1, row_stop1 - int(row_start1) + 1

    def _row_block(self, name, rows, out, out_row):
        """The host output of a block of `rows` rows x N columns: `out`, allocated when None and validated otherwise, the
        block's first row in it and the pointer to that row of its first column -> (out, out_row, pointer)."""
        if out is None:
            out, out_row = np.zeros((rows, self.N), np.float32, order="F"), 0
        elif out.dtype != np.float32 or out.ndim != 2 or not out.flags.f_contiguous or out.shape[1] != self.N:
            raise PMFError(f"{name}: out must be a Fortran-ordered float32 array with N columns")
        if out_row < 0 or out_row + rows > out.shape[0]:
            raise PMFError(f"{name}: the block does not fit in out")
        return out, out_row, _at(out.ctypes.data + 4 * int(out_row) if out.size else None)

    @staticmethod
    def _entries(name, rows1, cols1):
        """The 1-based entry lists as the library takes them, and the output vector -> (rows, cols, out)."""
        r = np.ascontiguousarray(rows1, dtype=np.int64).ravel()
        c = np.ascontiguousarray(cols1, dtype=np.int64).ravel()
        if r.shape != c.shape:
            raise PMFError(f"{name}: rows and columns must have the same length")
        return r, c, np.zeros(max(r.size, 1), np.float32)

    # ---- predictions
    @staticmethod
    def impute_flags(include_batch_effects=False, link=False, keep_observed=False):
        return ((IMPUTE_BATCH if include_batch_effects else 0) | (IMPUTE_LINK if link else 0)
                | (IMPUTE_KEEP_OBSERVED if keep_observed else 0))

    def impute(self, flags=0, row_start1=1, row_stop1=None, out=None, out_row=0):
        """pmf_impute: the predictions of rows row_start1..row_stop1 (1-based, inclusive; default all) x all columns.
        `out` (optional): a float32 Fortran-ordered array with N columns; the block is written to its rows out_row ..
        out_row + rows - 1 with its row count as the leading dimension, and nothing else in it is touched.
        Returns the rows x N block."""
        row_stop1, rows = self._rows(row_start1, row_stop1)
        rows = max(rows, 0)
        out, out_row, ptr = self._row_block("impute", rows, out, out_row)
        self._chk(self.lib.pmf_impute(self._h, flags, row_start1, row_stop1, ptr, out.shape[0]))
        return out[out_row:out_row + rows]

    def impute_device(self, ptr, flags=0, row_start1=1, row_stop1=None, ld=None):
        """pmf_impute_device: the same into device memory at address `ptr` (e.g. a torch tensor's data_ptr())."""
        row_stop1, rows = self._rows(row_start1, row_stop1)
        self._chk(self.lib.pmf_impute_device(self._h, flags, row_start1, row_stop1, _at(ptr), rows if ld is None else ld))

    def impute_entries(self, rows1, cols1, flags=0):
        """pmf_impute_entries: the predictions at the listed (row, column) entries, 1-based."""
        r, c, out = self._entries("impute_entries", rows1, cols1)
        self._chk(self.lib.pmf_impute_entries(self._h, flags, r.size, _i64p(r), _i64p(c), _fp(out)))
        return out[:r.size]

    # ---- simulated data
    @staticmethod
    def sim_opts(seed=0, noise=0.1, frac_missing=0.0, row_offset=0):
        return SimOpts(int(seed) & 0xFFFFFFFFFFFFFFFF, int(row_offset), float(noise), float(frac_missing))

    def simulate_data(self, seed=0, noise=0.1, frac_missing=0.0, row_offset=0, row_start1=1, row_stop1=None, out=None,
                      out_row=0):
        """pmf_simulate_data: rows row_start1..row_stop1 (1-based, inclusive; default all) x all columns drawn from the
        current parameters; `out` and `out_row` as in `impute`.  row_offset: the global index of local row 1."""
        row_stop1, rows = self._rows(row_start1, row_stop1)
        rows = max(rows, 0)
        out, out_row, ptr = self._row_block("simulate_data", rows, out, out_row)
        o = self.sim_opts(seed, noise, frac_missing, row_offset)
        self._chk(self.lib.pmf_simulate_data(self._h, C.byref(o), row_start1, row_stop1, ptr, out.shape[0]))
        return out[out_row:out_row + rows]

    def simulate_data_device(self, ptr, seed=0, noise=0.1, frac_missing=0.0, row_offset=0, row_start1=1, row_stop1=None,
                             ld=None):
        """pmf_simulate_data_device: the same into device memory at address `ptr`."""
        row_stop1, rows = self._rows(row_start1, row_stop1)
        o = self.sim_opts(seed, noise, frac_missing, row_offset)
        self._chk(self.lib.pmf_simulate_data_device(self._h, C.byref(o), row_start1, row_stop1, _at(ptr),
                                                    rows if ld is None else ld))

    def simulate_data_resident(self, seed=0, noise=0.1, frac_missing=0.0, row_offset=0):
        """pmf_simulate_data_resident: overwrites the data matrix resident on the device."""
        o = self.sim_opts(seed, noise, frac_missing, row_offset)
        self._chk(self.lib.pmf_simulate_data_resident(self._h, C.byref(o)))

    # ---- batch-corrected data
    @staticmethod
    def debatch_flags(link=False, fill_missing=False):
        return (DEBATCH_LINK if link else 0) | (DEBATCH_FILL_MISSING if fill_missing else 0)

    def remove_batch_effect(self, flags=0, row_start1=1, row_stop1=None, Z=None, out=None, out_row=0):
        """pmf_remove_batch_effect: rows row_start1..row_stop1 (1-based, inclusive; default all) x all columns with the batch
        layers taken out.  Z: the values of exactly those rows (rows x N, any layout; copied to a Fortran-ordered float32
        array unless it is one), or None for the data matrix resident on the device.  `out` as in `impute`; passing the same
        Fortran-ordered array as Z and out (out_row = 0, its row count = rows) corrects it in place.  Returns the rows x N
        block."""
        row_stop1, rows = self._rows(row_start1, row_stop1)
        rows = max(rows, 0)
        Zf, ldz = None, 0
        if Z is not None:
            Zf, ldz = _f32(Z), max(rows, 1)
            if Zf.shape != (rows, self.N):
                raise PMFError(f"remove_batch_effect: Z must be rows x N = {rows} x {self.N}")
        out, out_row, ptr = self._row_block("remove_batch_effect", rows, out, out_row)
        self._chk(self.lib.pmf_remove_batch_effect(self._h, flags, row_start1, row_stop1, _fp(Zf), ldz, ptr, out.shape[0]))
        return out[out_row:out_row + rows]

    def remove_batch_effect_device(self, out_ptr, flags=0, row_start1=1, row_stop1=None, z_ptr=None, ldz=None, ld=None):
        """pmf_remove_batch_effect_device: the same between device matrices (addresses, e.g. a torch tensor's data_ptr());
        z_ptr = None: the resident data matrix."""
        row_stop1, rows = self._rows(row_start1, row_stop1)
        self._chk(self.lib.pmf_remove_batch_effect_device(self._h, flags, row_start1, row_stop1, _at(z_ptr),
                                                          rows if ldz is None else ldz, _at(out_ptr),
                                                          rows if ld is None else ld))

    def remove_batch_effect_entries(self, rows1, cols1, values=None, flags=0):
        """pmf_remove_batch_effect_entries: the corrected values at the listed (row, column) entries, 1-based; values = None:
        the entries of the resident data matrix."""
        r, c, out = self._entries("remove_batch_effect_entries", rows1, cols1)
        v = None
        if values is not None:
            v = np.ascontiguousarray(values, dtype=np.float32).ravel()
            if v.shape != r.shape:
                raise PMFError("remove_batch_effect_entries: one value per entry")
            if v.size == 0:
                v = np.zeros(1, np.float32)
        self._chk(self.lib.pmf_remove_batch_effect_entries(self._h, flags, r.size, _i64p(r), _i64p(c), _fp(v), _fp(out)))
        return out[:r.size]

    def _by_view(self, flat):
        """A vector flat over (view, column, batch) -> per view its nb x N_v array (a copy)."""
        out, off = [], 0
        for nb, nv in self.view_shapes:
            out.append(flat[off:off + nb * nv].reshape((nb, nv), order="F").copy())
            off += nb * nv
        return out

    def stats(self, use_factors=False):
        """Masked column and (batch, column) statistics (pmf_stats).  Returns a dict of float32 arrays."""
        N = self.N
        out = {k: np.zeros(N, np.float32) for k in ("n", "sum", "sumsq", "sqerr", "ssq_grad")}
        nbt = sum(nb * nv for nb, nv in self.view_shapes)
        bc, bs = np.zeros(max(nbt, 1), np.float32), np.zeros(max(nbt, 1), np.float32)
        self._chk(self.lib.pmf_stats(self._h, int(use_factors), _fp(out["n"]), _fp(out["sum"]), _fp(out["sumsq"]),
                                     _fp(out["sqerr"]), _fp(out["ssq_grad"]), _fp(bc), _fp(bs)))
        out["batch_count"], out["batch_sqerr"] = self._by_view(bc), self._by_view(bs)
        return out

    # ---- the closed-form stages in the library (pmf_stage_*): the statistics never leave the device
    def stage_init_logsigma(self):
        """pmf_stage_init_logsigma: logsigma <- log sqrt(sqerr / n) with X'Y = 0, on the device (get_col_params reads it)."""
        self._chk(self.lib.pmf_stage_init_logsigma(self._h))

    def stage_reweight_col_losses(self, M_total):
        """pmf_stage_reweight_col_losses: the noise weights <- 1 / (rms column gradient * sigma) (get_noise_weights)."""
        self._chk(self.lib.pmf_stage_reweight_col_losses(self._h, int(M_total)))

    def get_noise_weights(self):
        w = np.zeros(self.N, np.float32)
        self._chk(self.lib.pmf_get_noise_weights(self._h, _fp(w)))
        return w

    def stage_minimal_group_weights(self, M_total):
        """pmf_stage_minimal_group_weights: one weight per column range of the noise model (as many as the last set_noise
        on this data shape passed; without one the library refuses and writes nothing)."""
        w = np.zeros(max(self.n_noise_ranges, 1), np.float32)
        self._chk(self.lib.pmf_stage_minimal_group_weights(self._h, int(M_total), _fp(w)))
        return w[:self.n_noise_ranges]

    def stage_theta_delta_em(self, delta2, sigma2, update_priors=True, max_iter=100, rtol=1e-8, verbosity=0):
        """pmf_stage_theta_delta_em on the context's theta.  delta2: per view an nb x N_v array (float64); sigma2: N values.
        Returns dict(theta=[per view, float32], delta2=[per view, float64], diffs, iters, seconds)."""
        if len(delta2) != len(self.view_shapes) or any(np.shape(d) != s for d, s in zip(delta2, self.view_shapes)):
            raise PMFError(f"delta2 must hold one array per batch view, shaped {self.view_shapes}")
        s2 = _f32(np.asarray(sigma2).ravel())
        if s2.shape != (self.N,):
            raise PMFError("sigma2 must have N entries")
        flat = np.ascontiguousarray(np.concatenate([np.asarray(d, np.float64).ravel(order="F") for d in delta2] or
                                                   [np.zeros(1)]))
        cap = max(int(max_iter), 1)
        diffs = np.zeros(cap, np.float64)
        o = EmOpts(int(bool(update_priors)), int(max_iter), int(verbosity), 0, float(rtol))
        r = EmResult()
        r.diffs_cap = cap
        r.diffs = _dp(diffs)
        self._chk(self.lib.pmf_stage_theta_delta_em(self._h, C.byref(o), _fp(s2), _dp(flat), C.byref(r)))
        theta = [self.get_batch_view(v)[1] for v in range(len(self.view_shapes))]
        return dict(theta=theta, delta2=self._by_view(flat), diffs=diffs[:r.n_diffs].copy(), iters=r.iters, seconds=r.seconds)

    # ---- the factor post-processing stages in the library: X and Y never leave the device
    def gram(self, which, ranges, diag_only=False):
        """pmf_gram of X (which = 0) or Y (1) over 1-based inclusive column ranges: (n_groups, K, K) float64, or with
        diag_only (n_groups, K).  X on a communicator of more than one rank: summed over the ranks."""
        s, e = _ranges(ranges)
        out = np.zeros((len(s), self.K) if diag_only else (len(s), self.K, self.K), np.float64)
        self._chk(self.lib.pmf_gram(self._h, which, len(s), _i64p(s), _i64p(e), int(bool(diag_only)), _dp(out)))
        return out

    def stage_lambda_max(self, which, ranges):
        """pmf_stage_lambda_max: the largest eigenvalue of each range's Gram matrix (float64)."""
        s, e = _ranges(ranges)
        lam = np.zeros(max(len(s), 1), np.float64)
        self._chk(self.lib.pmf_stage_lambda_max(self._h, which, len(s), _i64p(s), _i64p(e), _dp(lam)))
        return lam[:len(s)]

    def stage_whiten(self, M_total, view_ranges):
        """pmf_stage_whiten on the context's X, Y and logsigma.  Returns (x_rms [K], y_rms_max [views])."""
        s, e = _ranges(view_ranges)
        xr, c = np.zeros(max(self.K, 1), np.float64), np.zeros(max(len(s), 1), np.float64)
        self._chk(self.lib.pmf_stage_whiten(self._h, int(M_total), len(s), _i64p(s), _i64p(e), _dp(xr), _dp(c)))
        return xr[:self.K], c[:len(s)]

    def stage_rotate_by_svd(self):
        """pmf_stage_rotate_by_svd on the context's X and Y.  Returns (singular values [K], U [K x K], U[:, r] the r-th vector)."""
        sing, U = np.zeros(max(self.K, 1), np.float64), np.zeros((max(self.K, 1),) * 2, np.float64)
        self._chk(self.lib.pmf_stage_rotate_by_svd(self._h, _dp(sing), _dp(U)))
        return sing[:self.K], U[:self.K, :self.K]

    def stage_reorder_by_importance(self):
        """pmf_stage_reorder_by_importance on the context's X and Y.  Returns the 0-based permutation (new row r = old row p[r])."""
        p = np.zeros(max(self.K, 1), np.int32)
        self._chk(self.lib.pmf_stage_reorder_by_importance(self._h, _i32p(p)))
        return p[:self.K].astype(np.int64)

    def postprocess_times(self):
        """pmf_debug_postprocess_times: dict(gram, eig, apply) seconds of the last post-processing call's phases."""
        g, e, a = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self.lib.pmf_debug_postprocess_times(self._h, C.byref(g), C.byref(e), C.byref(a)))
        return dict(gram=g.value, eig=e.value, apply=a.value)

    # ---- multi-GPU
    def comm_init(self, rank, nranks, unique_id):
        """Attaches an RCCL communicator (pmf_comm_init; collective over the ranks).  pmf_fit then shards by rows."""
        if len(unique_id) != COMM_ID_BYTES:
            raise PMFError("unique id must be 128 bytes (comm_unique_id())")
        self._chk(self.lib.pmf_comm_init(self._h, rank, nranks, bytes(unique_id)))

    def comm_init_host(self, rank, nranks, allreduce):
        """Host-staged transport: `allreduce(array)` must sum a numpy array in place over the ranks (tests: gloo)."""
        def _cb(_user, buf, count, dtype):
            try:
                arr = np.ctypeslib.as_array(_at(buf, _PD if dtype == 1 else _PF), shape=(int(count),))
                allreduce(arr)
                return 0
            except Exception:   # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return -1
        self._host_cb = HOST_ALLREDUCE_FN(_cb)   # keep alive as long as the communicator
        self._chk(self.lib.pmf_comm_init_host(self._h, rank, nranks, self._host_cb, None))

    def comm_destroy(self):
        self._chk(self.lib.pmf_comm_destroy(self._h))
        self._host_cb = None

    def comm_set_chunks(self, n):
        self._chk(self.lib.pmf_comm_set_chunks(self._h, n))

    def comm_allreduce(self, arr, op="sum"):
        """In-place sum / max over the ranks of a float32 or float64 numpy array (pmf_comm_allreduce)."""
        if arr.dtype not in (np.float32, np.float64) or not arr.flags.c_contiguous:
            raise PMFError("comm_allreduce needs a contiguous float32 / float64 array")
        self._chk(self.lib.pmf_comm_allreduce(self._h, arr.ctypes.data_as(C.c_void_p), arr.size,
                                              1 if arr.dtype == np.float64 else 0, {"sum": 0, "max": 1}[op]))
        return arr

    def comm_info(self):
        r, n, t, ch, cu = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        nc = C.c_int64(0)
        self._chk(self.lib.pmf_comm_info(self._h, C.byref(r), C.byref(n), C.byref(t), C.byref(ch), C.byref(cu), C.byref(nc)))
        return dict(rank=r.value, nranks=n.value, transport=("none", "rccl", "host")[t.value], n_chunks=ch.value,
                    reserved_cus=cu.value, n_collectives=nc.value)

    def last_path(self):
        """Variants of the last launches: dict(bmode=0|1|2, layer_path=0|1|2, slots=..., xreg=0|1, plain_tiles=...), see
        pmf_hip.h."""
        b, l, s, x = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        pt = C.c_int64(0)
        self._chk(self.lib.pmf_debug_last_path(self._h, C.byref(b), C.byref(l), C.byref(s), C.byref(x), C.byref(pt)))
        return dict(bmode=b.value, layer_path=l.value, slots=s.value, xreg=x.value, plain_tiles=pt.value)

    def plain_table(self):
        """pmf_debug_plain_table: int32 [row panels of 256 rows][column tiles + 1], the running counts of not-all-finite
        tiles that the exact kernel chooses its plain tile loop from."""
        n_rp, n_ct = C.c_int64(0), C.c_int64(0)
        self._chk(self.lib.pmf_debug_plain_table(self._h, None, 0, C.byref(n_rp), C.byref(n_ct)))
        out = np.zeros((n_rp.value, n_ct.value + 1), np.int32)
        self._chk(self.lib.pmf_debug_plain_table(self._h, _i32p(out), out.size, None, None))
        return out

    def last_kernel(self):
        """Kernel family of the last fused data pass: 0 exact, 1 / 2 / 4 / 8 the split kernels sb / sb2 / sb4 / sb8."""
        k = C.c_int(0)
        self._chk(self.lib.pmf_debug_last_kernel(self._h, C.byref(k)))
        return k.value

    def pass_extents(self, update_X=False, update_Y=False, capacity_override=None):
        """pmf_debug_pass_extents: {buffer: dict(need=bytes, capacity=bytes)} of the data pass epoch_begin would run with
        these flags, prepared but not launched.  capacity_override ({buffer: bytes}, tests of the refusal) replaces recorded
        capacities and makes the call end with the pass's own check: PMFError naming the buffer if it would be refused."""
        n_max = PASS_EXTENTS_MAX
        names, n = (C.c_char_p * n_max)(), C.c_int(0)
        need, cap = (C.c_int64 * n_max)(), (C.c_int64 * n_max)()
        ov = None
        if capacity_override is not None:
            plain = self.pass_extents(update_X, update_Y)
            unknown = set(capacity_override) - set(plain)
            if unknown:
                raise PMFError(f"pass_extents: unknown buffers {sorted(unknown)}")
            ov = (C.c_int64 * n_max)(*([-1] * n_max))
            for i, k in enumerate(plain):
                ov[i] = int(capacity_override.get(k, -1))
        self._chk(self.lib.pmf_debug_pass_extents(self._h, int(update_X), int(update_Y), ov, n_max, names, need, cap,
                                                  C.byref(n)))
        return {names[i].decode(): dict(need=need[i], capacity=cap[i]) for i in range(n.value)}

    def set_precision(self, mode):
        """'f32' (exact f32 MFMA, default) or 'bf16x3' (split-bf16 products where a kernel variant exists)."""
        self._chk(self.lib.pmf_set_precision(self._h, {"f32": 0, "bf16x3": 1}[mode]))

    def get_precision(self):
        mode, n = C.c_int(0), C.c_int64(0)
        self._chk(self.lib.pmf_get_precision(self._h, C.byref(mode), C.byref(n)))
        return ("f32", "bf16x3")[mode.value], n.value

    def kernel_time(self, reset=False):
        ms, n = C.c_double(0), C.c_int64(0)
        self._chk(self.lib.pmf_kernel_time(self._h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def synth_data(self, seed=20260104, noise=0.1, frac_nan=0.0):
        self._chk(self.lib.pmf_synth_data(self._h, seed, noise, frac_nan))
