/*
 * pmf_hip.h -- C ABI of libpmf_hip.so, the MI355X (gfx950) implementation of PathMatFac's
 * `fit!` gradient-descent loop.
 *
 * Drop-in boundary.  In the reference the ONLY caller of the inner loop is `mf_fit!`
 * (src/fit.jl:9-38), which forwards to `MF.fit!(model.matfac, model.data; ...)` (src/fit.jl:24);
 * `gpu(model)` / `cpu(model)` move the parameters (analyses/scripts/julia/fit_matfac.jl:325-340).
 * A host (the Julia shim in pathmatfac.jl_amd/julia/PathMatFacHIP.jl via `ccall`, or the Python
 * ctypes binding in pathmatfac.jl_amd/_lib.py) re-implements `mf_fit!` as
 *     marshal (pmf_set_*)  ->  pmf_fit  ->  unmarshal (pmf_get_*)
 * and everything above `mf_fit!` in src/fit.jl runs unchanged.  Each entry point below cites the
 * reference interface it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; pmf_last_error() gives the (thread-local) message.
 *    (The reference throws Julia exceptions / @assert: src/model.jl:125-184, src/util.jl:189.)
 *  - matrices are COLUMN-MAJOR as in Julia.  D is M x N float32 with NaN = missing; X is K x M; Y is K x N.
 *    "Missing" is decided on the entry AS STORED on the device, and it means "not finite": +Inf and -Inf are missing exactly
 *    as NaN is (counts, loss, gradients and PMF_IMPUTE_KEEP_OBSERVED treat the three alike), and under PMF_STORE_BF16 so is a
 *    finite float32 that rounds to a bf16 infinity (|d| >= 0x7f7f8000 = 3.3961775e38).
 *  - column / row ranges are 1-BASED INCLUSIVE (Julia UnitRange, src/util.jl:187-197) so the shim passes
 *    ranges verbatim; `batch_of_row` is 0-based int32 (rowval-1 of the one-hot CSC row_batches matrix,
 *    src/util.jl:200-210, 588-593).
 *  - host pointers are borrowed only for the duration of a call (copy-in / copy-out); the library owns all
 *    device memory.  One pmf_ctx = one device = one host thread at a time.  Calls are synchronous.
 *  - no torch / HIP types in the signatures: `void*` stream and device pointers are raw hipStream_t / addresses.
 */
#ifndef PMF_HIP_H
#define PMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmf_ctx pmf_ctx;

/* noise-model kinds (src/util.jl:128 VALID_LOSSES; MatFac NormalNoise / BernoulliNoise / PoissonNoise, and
 * SquaredHingeNoise / OrdinalSqHingeNoise as two instances of one kind with three thresholds per column) */
#define PMF_NOISE_NORMAL 0
#define PMF_NOISE_BERNOULLI 1
#define PMF_NOISE_POISSON 2
#define PMF_NOISE_SQ_HINGE 3

/* optimizers: AdaGrad = Flux.Optimise.AdaGrad as constructed at src/fit.jl:41-43 and applied through
 * src/optimizers.jl:6-13 ; Adam = Flux.Optimise.Adam (named by the north-star; no reference call site) */
#define PMF_OPT_ADAGRAD 0
#define PMF_OPT_ADAM 1

/* storage type of the data matrix on the device.  PMF_STORE_BF16 rounds every entry once, at upload, to the nearest
 * bfloat16, ties to even: float32 subnormals round like any other value (nothing is flushed to zero), every NaN stays a
 * NaN whatever its payload, and a finite entry at or above the overflow point 0x7f7f8000 (3.3961775e38, the tie between the
 * largest bf16 and 2^128) becomes an infinity, which is a MISSING entry like every non-finite one (conventions above). */
#define PMF_STORE_F32 0
#define PMF_STORE_BF16 1

/* termination codes of pmf_fit == MatFac.fit!'s history["term_code"] (src/fit.jl:63) */
#define PMF_TERM_MAX_EPOCHS 0
#define PMF_TERM_LOSS_INCREASE 1
#define PMF_TERM_ABS_TOL 2
#define PMF_TERM_REL_TOL 3
#define PMF_TERM_NONFINITE 4

/* parameter groups (for pmf_get_grad / pmf_grad_device_ptr) */
#define PMF_PARAM_X 0
#define PMF_PARAM_Y 1
#define PMF_PARAM_LOGSIGMA 2
#define PMF_PARAM_MU 3
#define PMF_PARAM_LOGDELTA 4
#define PMF_PARAM_THETA 5

/* kwargs of mf_fit! / MF.fit! (src/fit.jl:9-36) that reach the kernel library */
typedef struct pmf_fit_opts {
  int32_t update_X;            /* src/fit.jl:10 */
  int32_t update_Y;            /* src/fit.jl:11 */
  int32_t update_col_layers;   /* src/fit.jl:13 */
  int32_t frozen_layers;       /* bit (l-1): layer l is a FrozenLayer (src/layers.jl:299-363, freeze_layer! :337) */
  int32_t frozen_regs;         /* bit (l-1): regs[l] is a FrozenRegularizer (src/regularizers.jl:950-999) */
  int32_t max_epochs;          /* src/fit.jl:58 */
  int32_t epoch;               /* 1-based starting epoch (src/fit.jl:56-58, :69) */
  int32_t tol_max_iters;       /* MatFac default 3 */
  int32_t keep_trace;          /* keep_history (src/fit.jl:20) */
  int32_t verbosity;           /* src/fit.jl:59 */
  int32_t print_iter;          /* test/runtests.jl:1335 */
  int32_t reserved;
  double abs_tol;              /* src/fit.jl:935 */
  double rel_tol;              /* src/fit.jl:934 */
  int64_t capacity;            /* src/fit.jl:938 -- accepted for API compatibility; D is streamed in one fused pass */
} pmf_fit_opts;

/* history Dict returned by MF.fit! (src/fit.jl:61-69): "term_code", "epochs", loss trace */
typedef struct pmf_fit_result {
  int32_t term_code;
  int32_t epochs;      /* last epoch index executed (src/fit.jl:69 resumes from h["epochs"]) */
  int32_t n_trace;     /* number of losses written to loss_trace */
  int32_t trace_cap;   /* in: capacity of loss_trace */
  double final_loss;
  double *loss_trace;  /* in: host buffer (may be NULL) */
  double seconds;      /* wall time of the epoch loop */
} pmf_fit_result;

const char *pmf_last_error(void);
int pmf_version(void);

/* gpu(model) / cpu(model): analyses/scripts/julia/fit_matfac.jl:325-340, src/transform.jl:78-94.
 * pmf_device_count: HIP devices visible to this process (CUDA.device! / the per-process device choice of
 * analyses/scripts/julia/script_util.jl:278-306): a launcher that pins one device per rank leaves ONE, device 0. */
int pmf_device_count(int *n);
int pmf_create(int device, pmf_ctx **out);
int pmf_destroy(pmf_ctx *ctx);
/* adopt an existing hipStream_t (e.g. the host framework's current stream); NULL = library-owned (non-blocking) stream.
 * The legacy DEFAULT stream is not NULL here: pass hipStreamLegacy ((hipStream_t)1).  A host whose collectives are
 * ordered behind the default stream (torch reports it as handle 0) must do so, or the library's kernels on its own
 * stream are not ordered with them. */
int pmf_set_stream(pmf_ctx *ctx, void *hip_stream);
int pmf_synchronize(pmf_ctx *ctx);

/* model.data (src/model.jl:12), from host or from device memory.  Either way the library COPIES: the matrix is re-laid out
 * (and rounded under PMF_STORE_BF16) into a tile-major buffer that the context owns, and the source may be changed or freed
 * as soon as the call returns.  `M` is the number of LOCAL rows when the samples are sharded across GPUs.
 *   pmf_set_data        : a host matrix, uploaded in column chunks of at most 64 Mi floats (256 MiB; one column where a
 *                         column alone is longer) through a staging buffer of that size that the context keeps.
 *                         PMF_SET_DATA_CHUNK_FLOATS=n, read at every call, replaces the 64 Mi: a test hook that makes small
 *                         shapes upload in several chunks.
 *   pmf_set_data_device : D_device is a column-major M x N float32 matrix in DEVICE memory (leading dimension M, 4-byte
 *                         alignment is enough), read by one kernel on the context's stream.  It must be COMPLETE before the
 *                         call: the copy is ordered behind the work that produced it only if that work ran on the stream the
 *                         context has adopted (pmf_set_stream); in every other case the caller synchronizes first.
 *                         D_device = NULL allocates the buffer for an M x N matrix and leaves it all-missing
 *                         (pmf_synth_data, pmf_simulate_data_resident fill it). */
int pmf_set_data(pmf_ctx *ctx, const float *D_colmajor, int64_t M, int64_t N, int store);
int pmf_set_data_device(pmf_ctx *ctx, const void *D_device, int64_t M, int64_t N, int store);

/* model.matfac.X / .Y (K x M, K x N; src/model.jl:69-72, fields used at src/fit.jl:133-136) */
int pmf_set_factors(pmf_ctx *ctx, const float *X, const float *Y, int K);
int pmf_set_X(pmf_ctx *ctx, const float *X, int K);
int pmf_set_Y(pmf_ctx *ctx, const float *Y, int K);
int pmf_get_factors(pmf_ctx *ctx, float *X, float *Y);

/* col_transform.layers[1].logsigma (ColScale, src/layers.jl:9-22), layers[3].mu (ColShift, :53-66) */
int pmf_set_col_params(pmf_ctx *ctx, const float *logsigma, const float *mu);
int pmf_get_col_params(pmf_ctx *ctx, float *logsigma, float *mu);

/* col_transform.layers[2].logdelta / layers[4].theta : BatchArray (src/batch_array.jl:5-15).
 * n views = length(ba.col_ranges); view v: col_range, nb = size(values[v],1), one-hot row_batches[v]
 * given as batch_of_row, values nb x Nv column-major.  n = 0 makes layers 2 and 4 the identity
 * (src/layers.jl:243, src/transform.jl:64-65). */
int pmf_set_n_batch_views(pmf_ctx *ctx, int n);
int pmf_set_batch_view(pmf_ctx *ctx, int v, int64_t col_start1, int64_t col_stop1, int nb,
                       const int32_t *batch_of_row, const float *logdelta, const float *theta);
int pmf_get_batch_view(pmf_ctx *ctx, int v, float *logdelta, float *theta);

/* matfac.noise_model: CompositeNoise{noises, col_ranges} (src/fit.jl:227) + per-column weights set through
 * MF.set_weight! (src/fit.jl:157, 180) */
int pmf_set_noise(pmf_ctx *ctx, int n_ranges, const int64_t *starts1, const int64_t *stops1, const int32_t *kinds,
                  const float *weights);

/* Thresholds t0 <= t1 <= t2 (each may be +-Inf) of the columns of kind PMF_NOISE_SQ_HINGE.  SELF-SPECIFIED model (DESIGN.md
 * section 2): an observed entry y has class c = clamp((int)(y + 0.5), 0, 3) and the bin (lo, hi] = ((-Inf, t0, t1, t2)[c],
 * (t0, t1, t2, +Inf)[c]); its loss is 0.5 w (relu(1 - (z - lo))^2 + relu(1 - (hi - z))^2), an infinite bound contributing
 * nothing.  pmf_set_noise gives every kind-3 column (0, +Inf, +Inf): bernoulli_sq_hinge on 0/1 data.  ordinal_sq_hinge3
 * on 1/2/3 data is (-Inf, t1, t2).  The thresholds are constants of the fit.
 *   pmf_set_noise_thresholds : thr holds 3 floats per range; fails (and changes nothing) unless every column of every range is
 *                              of kind 3 and t0 <= t1 <= t2.
 *   pmf_get_noise_thresholds : 3 x N floats (column j at thr[3 j]), NaN for the columns of the other kinds. */
int pmf_set_noise_thresholds(pmf_ctx *ctx, int n_ranges, const int64_t *starts1, const int64_t *stops1, const float *thr);
int pmf_get_noise_thresholds(pmf_ctx *ctx, float *thr);

/* matfac.X_reg.  A regularizer is a sum of terms p_t * reg_t (CompositeRegularizer, src/regularizers.jl:616-643).
 *   pmf_clear_xreg            : `X -> 0`                    (src/fit.jl:769, src/transform.jl:70)
 *   pmf_add_xreg_l2           : L2Regularizer(weights[K])   (src/regularizers.jl:11-33)
 *   pmf_add_xreg_group        : GroupRegularizer            (src/regularizers.jl:345-359, 423-446);
 *                               w is n_groups x K with K contiguous (group_weights[g][k]) */
int pmf_clear_xreg(pmf_ctx *ctx);
int pmf_add_xreg_l2(pmf_ctx *ctx, const float *w, float p);
int pmf_add_xreg_group(pmf_ctx *ctx, int n_groups, const int64_t *starts1, const int64_t *stops1, const float *w,
                       float p);

/* matfac.Y_reg.
 *   pmf_add_yreg_group : GroupRegularizer on feature ranges (construct_minimal_regularizer,
 *                        src/regularizers.jl:750-774; construct_Y_reg :715-717)
 *   pmf_add_yreg_l2    : L2Regularizer
 *   pmf_add_yreg_ard   : ARDRegularizer(alpha, beta per view range)  (src/regularizers.jl:526-585)
 *   pmf_add_yreg_fsard : FeatureSetARDReg call + rrule (src/featureset_ard.jl:135-150); alpha[N], beta[K x N] */
int pmf_clear_yreg(pmf_ctx *ctx);
int pmf_add_yreg_l2(pmf_ctx *ctx, const float *w, float p);
int pmf_add_yreg_group(pmf_ctx *ctx, int n_groups, const int64_t *starts1, const int64_t *stops1, const float *w,
                       float p);
int pmf_add_yreg_ard(pmf_ctx *ctx, int n_ranges, const int64_t *starts1, const int64_t *stops1, const float *alpha,
                     const float *beta, float p);
int pmf_add_yreg_fsard(pmf_ctx *ctx, const float *alpha, const float *beta, float p);

/* The pathway-graph regularizers (fit_non_ard!, src/fit.jl:730-745), on X (n = local rows) or Y (n = N).
 *
 * One sparse block in 0-based CSR with sorted rows.  AA and BB are symmetric, so a Julia host passes `colptr` and
 * `rowval .- 1` of its SparseMatrixCSC as they are; the library builds AB' itself. */
typedef struct pmf_csr { int64_t n_rows, n_cols; const int64_t *rowptr; const int32_t *col; const float *val; } pmf_csr;
/*   pmf_add_xreg_network / pmf_add_yreg_network : NetworkRegularizer call + rrule (src/regularizers.jl:249-306) with the
 *     blocks its constructor makes (:189-238): per factor k, AA[k] (n x n), AB[k] (n x v_k), BB[k] (v_k x v_k);
 *     loss = sum_k 0.5 p_k'AA_k p_k + p_k'AB_k u_k + 0.5 u_k'BB_k u_k with u_k = -BB_k^{-1} AB_k' p_k (`x_virtual[k]`)
 *     found by conjugate gradients on the device every epoch (stop at |r| <= 1e-6 |AB_k' p_k| or after 2 v_k
 *     iterations; warm start: the previous epoch's u_k).  v_k = 0 and empty graphs are legal.
 *     `K` must equal the context's K.  u0: K pointers to initial u_k (or NULL pointers / NULL for zeros); the state
 *     lives until the regularizer is cleared.  One network term per parameter.  With more than one rank a network
 *     term on X makes pmf_fit fail (rows are sharded); one on Y is evaluated by every rank alike.
 *   pmf_get_reg_network_state : u_k (v_k floats; `u` may be NULL) and the CG iterations of the last solve of factor k
 *     (0-based) of the term on `which` (PMF_PARAM_X | PMF_PARAM_Y): what `nr.x_virtual[k]` holds after a call (:257).
 *   pmf_add_xreg_l1 / pmf_add_yreg_l1 : sum_k w[k] sum_j |m_kj P_kj|, gradient w[k] sign(m_kj P_kj), sign(0) = 0:
 *     SelectiveL1Reg (src/regularizers.jl:130-146; mask = l1_idx, K x n column-major bytes) and L1Regularizer
 *     (:71-82; mask NULL = every entry). */
int pmf_add_xreg_network(pmf_ctx *ctx, int K, const pmf_csr *AA, const pmf_csr *AB, const pmf_csr *BB,
                         const float *const *u0, float p);
int pmf_add_yreg_network(pmf_ctx *ctx, int K, const pmf_csr *AA, const pmf_csr *AB, const pmf_csr *BB,
                         const float *const *u0, float p);
int pmf_get_reg_network_state(pmf_ctx *ctx, int which, int k, float *u, int *cg_iters);
int pmf_add_xreg_l1(pmf_ctx *ctx, const float *w, const uint8_t *mask, float p);
int pmf_add_yreg_l1(pmf_ctx *ctx, const float *w, const uint8_t *mask, float p);

/* matfac.col_transform_reg = SequenceReg (src/regularizers.jl:896-926):
 *   regs[1], regs[3] : ColParamReg(col_ranges, weights, centers) on logsigma / mu   (:462-487)
 *   regs[2], regs[4] : BatchArrayReg(centers, weights) on logdelta / theta          (:781-815)
 * Pass n_ranges = 0 / NULL arrays for `x -> 0`.  Batch arrays are flat over (view, batch). */
int pmf_set_layer_regs(pmf_ctx *ctx, int n_ranges, const int64_t *starts1, const int64_t *stops1,
                       const float *w_logsigma, const float *c_logsigma, const float *w_mu, const float *c_mu,
                       const float *w_logdelta, const float *c_logdelta, const float *w_theta,
                       const float *c_theta);

/* construct_optimizer (src/fit.jl:41-43) ; `opt.eta *= 0.5` (src/fit.jl:64) ; fresh state per stage (src/fit.jl:55) */
int pmf_set_optimizer(pmf_ctx *ctx, int kind, float lr, float eps, float beta1, float beta2);
int pmf_set_lr(pmf_ctx *ctx, float lr);
int pmf_get_lr(pmf_ctx *ctx, float *lr);
int pmf_reset_optimizer_state(pmf_ctx *ctx);
/* the optimizer's per-parameter state in the parameter's own shape (view: batch view for logdelta / theta): AdaGrad's
 * `acc` (Flux.Optimise.AdaGrad, applied through src/optimizers.jl:6-13; starts at eps) or Adam's second moment, and
 * Adam's first moment.  The state lives as long as the optimizer object does in the reference: across the mf_fit! calls
 * of one mf_fit_adapt_lr! (src/fit.jl:55-69), whatever is re-marshalled in between. */
int pmf_get_opt_state(pmf_ctx *ctx, int which, int view, float *acc, float *mom);

/* MF.fit!(model.matfac, model.data; ...) as called from mf_fit! (src/fit.jl:24-36) */
int pmf_fit(pmf_ctx *ctx, const pmf_fit_opts *opts, pmf_fit_result *result);

/* full_loss(model, D) (src/fit_lbfgs.jl:3-8): data loss + X_reg(X) + Y_reg(Y) at the context's CURRENT parameters, the
 * layer regularizers not included.  total = data + xreg + yreg (each output may be NULL).  The data term is always the
 * exact-f32 pass, whatever pmf_set_precision says, summed in a fixed order: a value is bitwise the same run to run.
 * Touches no parameter, gradient, optimizer state or communicator (it does overwrite the loss partials of the
 * step-level API: do not call it between pmf_epoch_begin and pmf_epoch_loss).  Refused with a network term attached
 * (evaluating it would move its warm-start state). */
int pmf_loss(pmf_ctx *ctx, double *total, double *data, double *xreg, double *yreg);

/* fit_lbfgs!(matfac, D; ...) (src/fit_lbfgs.jl:170-243): L-BFGS over X and Y together with the backtracking line search
 * of backtrack! (:114-148) and the two-loop recursion of inner_loop! (:151-167); layers, noise weights and regularizer
 * weights are constants.  The rules, the reference's quirks included, are restated in DESIGN.md section 2 ("Deviation 2 /
 * L-BFGS").  Loss = pmf_loss; gradient = the fused data pass (in the context's precision mode) + the gradients of the
 * attached quadratic (L2, group) and ARD-type terms.  Every inner product is a fixed-order f64 sum: a call repeats
 * bit for bit.
 *   m                   history length, 1..32 (the bound is the library's: scalars per pair live in fixed device slots);
 *                       the call holds 2 m + 4 vectors of K_p (M + N) floats on the device, kept until (K, M, N, m) change
 *   max_iter            fit_lbfgs!'s max_iter (0: only the start loss is evaluated)
 *   backtrack_max_iter  backtrack!'s max_iter (reference: 100), >= 1
 *   rel_tol, abs_tol    :230-236; backtrack_shrinkage in (0, 1); c1 = 1e-4 (sufficient_decrease :111); sy_min = 1e-4 (:216)
 *   verbosity, print_iter  "(iter) L-BFGS; Loss=..." every print_iter iterations (:195-197)
 * Result: term_code PMF_TERM_ABS_TOL / REL_TOL / NONFINITE (a non-finite loss after a backtrack; the reference would go
 * on) / MAX_EPOCHS (max_iter reached); iters = line searches run; final_loss = the loss at the parameters the call
 * leaves (bitwise pmf_loss there); loss_evals / grad_evals = data passes of either kind; resets = history resets.
 * Traces (caller-owned, trace_cap entries each, any may be NULL; filled when keep_trace): per iteration the loss after
 * the backtrack, its trial count, and flags: bit 0 reset (<s,y> <= sy_min), bit 1 the direction was no descent direction
 * and -g was taken, bit 2 the backtrack ran out of trials.
 * A start with a zero direction (e.g. X = Y = 0) returns PMF_TERM_ABS_TOL at once, parameters untouched.
 * Refused: no data / factors; a network or L1 / SelectiveL1 term on X or Y; a communicator of more than one rank; m,
 * backtrack_shrinkage, max_iter or backtrack_max_iter out of range.  Leaves the optimizer state, Adam's powers and the
 * learning rate alone. */
typedef struct pmf_lbfgs_opts {
  int32_t m;
  int32_t max_iter;
  int32_t backtrack_max_iter;
  int32_t keep_trace;
  int32_t verbosity;
  int32_t print_iter;
  double rel_tol;
  double abs_tol;
  double backtrack_shrinkage;
  double c1;
  double sy_min;
} pmf_lbfgs_opts;
typedef struct pmf_lbfgs_result {
  int32_t term_code;
  int32_t iters;
  int32_t loss_evals;
  int32_t grad_evals;
  int32_t resets;
  int32_t n_trace;     /* entries written to the traces */
  int32_t trace_cap;   /* in: capacity of each trace */
  int32_t reserved;
  double final_loss;
  double seconds;
  double *loss_trace;   /* in: host buffers (may be NULL) */
  int32_t *trial_trace;
  int32_t *flag_trace;
} pmf_lbfgs_result;
int pmf_fit_lbfgs(pmf_ctx *ctx, const pmf_lbfgs_opts *opts, pmf_lbfgs_result *result);
/* The recursion kernels of pmf_fit_lbfgs on a handed-in history (tests): n_pairs (0..32) pairs (s, y) stacked NEWEST
 * FIRST, each in the reference's shapes (sX, yX: n_pairs x K x M; sY, yY: n_pairs x K x N), the gradient g, and the
 * direction p = -H g out.  No reset test.  Needs data and factors set (they fix K, M, N). */
int pmf_debug_lbfgs_direction(pmf_ctx *ctx, int n_pairs, const float *sX, const float *sY, const float *yX,
                              const float *yY, const float *gX, const float *gY, float *pX, float *pY);

/* Step-level API (what pmf_fit is made of), exposed so that a multi-GPU host can place the cross-GPU
 * reduction of grad(Y) and of the loss between the two halves of an epoch (DESIGN.md "multi-GPU"):
 *   pmf_epoch_begin     : fused data pass -> local data loss partials + data gradients (async on the stream)
 *   pmf_epoch_step_local: regularizer gradient + optimizer step of the row-local parameters (X)
 *   pmf_epoch_step_shared: same for the replicated parameters (Y and column layers), after their gradients
 *                          have been summed across ranks
 *   pmf_epoch_loss      : finishes the deterministic loss reduction and returns the local loss
 *                         (data partial + regularizer terms); `shared_terms` receives the part that is
 *                         replicated on every rank (so the host can avoid counting it once per rank) */
int pmf_epoch_begin(pmf_ctx *ctx, const pmf_fit_opts *opts);
int pmf_epoch_step_local(pmf_ctx *ctx, const pmf_fit_opts *opts);
int pmf_epoch_step_shared(pmf_ctx *ctx, const pmf_fit_opts *opts);
int pmf_epoch_loss(pmf_ctx *ctx, double *local_loss, double *shared_terms);

/* Multi-GPU (the reference is single-GPU -- one process per GPU is its habit for independent fits,
 * analyses/scripts/julia/script_util.jl:278-306).  The samples (rows of D, columns of X, batch_of_row) are sharded over
 * the ranks, one process and one pmf_ctx per GPU; Y, the column layers, the noise model and their regularizers are
 * replicated.  With a communicator attached, pmf_fit sums over the ranks, once per epoch: the partial grad(Y) (in a few
 * column chunks, each all-reduced beside the data pass of the other chunks), the rank-local part of the loss (data term +
 * X regularizer, two doubles) and -- when the column layers train -- their gradients; every rank then takes the same
 * steps of the replicated parameters and the same termination decision.  The step-level API below does not use the
 * communicator (there the host places its own collectives).
 *   pmf_comm_get_unique_id : ncclGetUniqueId; call on ONE rank, hand the PMF_COMM_ID_BYTES bytes to all (any side channel)
 *   pmf_comm_init          : ncclCommInitRank[Config] over RCCL / xGMI; collective over the ranks.  librccl.so.1 is loaded
 *                            here (dlopen), never before.  With nranks > 1 the data pass leaves PMF_COMM_CTAS CUs (env,
 *                            DEFAULT 4; 0 = none) to the collective's kernels, and this communicator alone is configured
 *                            for as many workgroups (ncclConfig_t.maxCTAs): the library sets NO environment variable and
 *                            touches nothing process-wide; other communicators of the host keep RCCL's defaults.
 *   pmf_comm_init_host     : the same protocol over a host callback `fn(user, host_buf, count, dtype)` that must sum
 *                            host_buf (dtype 0 = float32, 1 = float64) in place over the ranks and return 0; the library
 *                            stages device <-> pinned host memory around it.  For hosts without a usable RCCL ring
 *                            (tests: two ranks sharing one GPU).
 *   pmf_comm_set_chunks    : column chunks per data pass; 0 = automatic (1 on one rank, up to 4 with more; chosen from N, K
 *                            and the MEAN rows per rank, all-reduced once per pmf_fit, so that ranks with shards of
 *                            different heights issue the same collectives).  A non-zero value must be the same on all ranks.
 *   A pmf_fit that FAILS on a rank of a multi-rank communicator drains its streams and marks the communicator unusable
 *   (the peers may be waiting in a collective it never issued): a rank failure is fatal for the group.
 *   pmf_comm_allreduce     : sum (op 0) / maximum (op 1) over the ranks of a HOST buffer (dtype 0 = float32, 1 = float64),
 *                            for what the host keeps between the GD stages: the statistics of pmf_stats that feed
 *                            init_logsigma! / reweight_col_losses! / theta_delta_em (src/fit.jl:125-187, 326-375) must be
 *                            summed over the row shards.  No-op without a communicator.
 *   pmf_comm_info          : rank, size, transport, chunks of the last pmf_fit, reserved CUs, collectives issued */
#define PMF_COMM_ID_BYTES 128
#define PMF_COMM_NONE 0
#define PMF_COMM_RCCL 1
#define PMF_COMM_HOST 2
typedef int (*pmf_host_allreduce_fn)(void *user, void *host_buf, int64_t count, int dtype);
int pmf_comm_get_unique_id(void *id_out);
int pmf_comm_init(pmf_ctx *ctx, int rank, int nranks, const void *unique_id);
int pmf_comm_init_host(pmf_ctx *ctx, int rank, int nranks, pmf_host_allreduce_fn fn, void *user);
int pmf_comm_destroy(pmf_ctx *ctx);
int pmf_comm_set_chunks(pmf_ctx *ctx, int n_chunks);
int pmf_comm_allreduce(pmf_ctx *ctx, void *host_buf, int64_t count, int dtype, int op);
int pmf_comm_info(pmf_ctx *ctx, int *rank, int *nranks, int *transport, int *n_chunks, int *reserved_cus,
                  int64_t *n_collectives);

/* Diagnostics: the batch-layer variant the last data pass took (0 none, 1 LDS table with panel-local slots, 2 per-entry
 * gathers), the last layer pass (1 MFMA layer pass, 2 VALU kernel) and the columns of the dense batch table as of the
 * last prepared epoch (16 without batch views, 0 when a view has more than 255 batches and no table is built).  Views with
 * more than 15 batches stay on variant 1 as long as no 256-row (128-row for K > 64) panel holds more than 15 distinct
 * batches of one view (src/batch_array.jl:78-147 places no bound on the batch count).
 * xreg: 1 when the last fused launch ran an instance of the exact kernel that holds a piece's X operands in registers
 * (32 < K <= 64, both gradients, PMF_XREG unset or non-zero), 0 when it read them from LDS per tile; the two are
 * bit-identical in every result, so this field is the only way to tell which one ran.
 * plain_tiles: the (row panel, column tile) pairs the last data pass ran in the plain tile loop of those instances (runs of
 * all-finite, full, already visited tiles; 0 under PMF_PLAIN=0, read at every pass, and for every other kernel); again
 * bit-identical, and counted by the kernel itself.  Asking for it waits for the pass.  Any out-pointer may be null. */
int pmf_debug_last_path(pmf_ctx *ctx, int *bmode, int *layer_path, int *slots, int *xreg, int64_t *plain_tiles);
/* Diagnostics: the table the plain loop is chosen from, built for the context's data as a pass of 256-row panels would
 * build it: int32 [n_rp][n_ct + 1], entry (rp, c) = the number of column tiles < c whose 32 x 32 tiles in row panel rp are
 * not all finite (row blocks beyond the matrix count as not finite).  out may be NULL (shape only); cap = its entries. */
int pmf_debug_plain_table(pmf_ctx *ctx, int32_t *out, int64_t cap, int64_t *n_rp, int64_t *n_ct);
/* the kernel family the last fused data pass ran on: 0 exact f32 (pmf_fused_kernel), 1 pmf_fused_sb_kernel, 2 pmf_fused_sb2_kernel,
 * 4 pmf_fused_sb4_kernel, 8 pmf_fused_sb8_kernel (split modes; tests assert that the intended variant really ran) */
int pmf_debug_last_kernel(pmf_ctx *ctx, int *kernel);

/* Diagnostics: per grow-only device buffer of the fused data pass (gx_part, gy_slabs, xsb, ysb, btd, colview, tflags,
 * loss_partial, pm, row_slot; ptab and plain_count besides when the pass runs a kernel with the plain tile loop), the bytes the kernels of the pass pmf_epoch_begin would run with these gradient flags address
 * ("need", from the kernels' index expressions) and the bytes allocated ("capacity"); 0 / 0 for a buffer the pass does not
 * use.  The call chooses the kernel family and prepares the buffers exactly as the pass would and launches no data pass.
 * Every data pass makes the same comparison before its first launch and refuses to run when a need exceeds its capacity.
 * names / need / capacity: arrays of n_max entries (PMF_PASS_EXTENTS_MAX is enough; names point to static strings), *n the
 * entries filled.  cap_override (tests of the refusal; normally NULL): n_max capacities that replace the recorded ones
 * where >= 0; the call then ends with the pass's own comparison and fails, naming the buffer, if it would be refused. */
#define PMF_PASS_EXTENTS_MAX 16
int pmf_debug_pass_extents(pmf_ctx *ctx, int update_X, int update_Y, const int64_t *cap_override, int n_max,
                           const char **names, int64_t *need, int64_t *capacity, int *n);

/* Diagnostics: the bytes of device memory and of pinned host memory that the library holds at this moment, summed over every
 * context of the PROCESS (its contexts' buffers and the temporaries of a running call).  Every allocation of the library is
 * counted where it is made and where it is freed, so the figures are exact whatever else runs on the GPU: a context's
 * pmf_destroy brings both back to what they were before its pmf_create.  Either pointer may be NULL. */
int pmf_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes);

/* raw device addresses of the gradient buffers (float32) and their element counts, for in-place collectives */
int pmf_grad_device_ptr(pmf_ctx *ctx, int which, void **ptr, int64_t *n_elements);
/* copy a gradient of the last pmf_epoch_begin to the host in the reference's shape (tests / diagnostics) */
int pmf_get_grad(pmf_ctx *ctx, int which, int view, float *out);

/* MF.forward(matfac) (src/simulate_params.jl:247): Z = layers(X'Y) for all local rows, M x N column-major */
int pmf_forward(pmf_ctx *ctx, float *Z_host);

/* impute(model; include_batch_effects=false) (src/impute.jl:37-56) and the per-noise inverse links it ends with
 * (src/impute.jl:3-13, 27-35): the model's predictions from the context's CURRENT X, Y, column parameters, batch views and
 * noise ranges.  Per entry, with a = sum_k X[k,i] Y[k,j]:
 *     z = a sigma_j + mu_j                                       (flags = 0: the reference's default)
 *     z = a sigma_j delta_v[b,j] + mu_j + theta_v[b,j]           (PMF_IMPUTE_BATCH: layers 2 and 4 as everywhere else in
 *                                                                 this library; a row in no batch has delta = 1, theta = 0)
 *     normal -> z ; bernoulli -> 1 / (1 + e^-z) ; poisson -> e^z  (PMF_IMPUTE_LINK: z itself for every column)
 * PMF_IMPUTE_KEEP_OBSERVED returns the finite entries of the data matrix as stored on the device (bf16-rounded under
 * PMF_STORE_BF16) and predicts only the missing ones.
 *   pmf_impute          : local rows row_start1..row_stop1 (1-based, inclusive) x all N columns into a HOST matrix, column-major
 *                         with leading dimension ld >= rows.  Computed in row chunks through a staging buffer of at most
 *                         256 MiB that the context owns (PMF_IMPUTE_CHUNK_ROWS=n, read at every call, overrides the chunk
 *                         height); elements of out_host between the rows of a column (ld > rows) are not written.
 *   pmf_impute_device   : the same into DEVICE memory, one launch, no staging.
 *   pmf_impute_entries  : the predictions at n listed entries (rows1[e], cols1[e], 1-based; duplicates are legal): held-out
 *                         scoring without an M x N temporary.  n = 0 succeeds and does nothing.
 * The arithmetic is exact f32 (v_mfma_f32_32x32x2_f32 / fmaf) whatever pmf_set_precision says.  An entry's value does not
 * depend on the row range, the chunking, ld, or what the context ran before.  The calls change nothing a later pmf_fit
 * reads: no optimizer state, no gradient, no parameter.  LOCAL ROWS ONLY: no communicator traffic; the host of a sharded
 * fit calls them on every rank for that rank's rows.
 * A data matrix must have been set (it fixes M and N); its values are read only for PMF_IMPUTE_KEEP_OBSERVED.
 * Refused before anything is launched (the context stays usable): a null output, unknown flag bits, an empty or
 * out-of-range row range, ld below the row count, factors not set, PMF_IMPUTE_KEEP_OBSERVED without data or passed to
 * pmf_impute_entries, an entry outside 1..M x 1..N.
 *   pmf_debug_impute_offset : the 64-bit element offset of (0-based row of the range, 0-based column) in an output of
 *                         leading dimension ld, by the function the kernels use (tests). */
#define PMF_IMPUTE_BATCH 1          /* apply layers 2 and 4 (batch scale / shift): include_batch_effects=true */
#define PMF_IMPUTE_LINK 2           /* return z itself, no inverse link */
#define PMF_IMPUTE_KEEP_OBSERVED 4  /* entries of D that are finite are returned as stored; only missing ones are predicted */
int pmf_impute(pmf_ctx *ctx, int flags, int64_t row_start1, int64_t row_stop1, float *out_host, int64_t ld);
int pmf_impute_device(pmf_ctx *ctx, int flags, int64_t row_start1, int64_t row_stop1, float *out_device, int64_t ld);
int pmf_impute_entries(pmf_ctx *ctx, int flags, int64_t n, const int64_t *rows1, const int64_t *cols1, float *out_host);
int pmf_debug_impute_offset(int64_t row, int64_t col, int64_t ld, int64_t *offset);

/* simulate_data!(model) (src/simulate_params.jl:219-251): a data matrix drawn from the context's CURRENT X, Y, column
 * parameters, batch views, noise ranges and thresholds.  SELF-SPECIFIED where the reference is silent (DESIGN.md section 2,
 * Deviation 4).  Per entry (i = GLOBAL 0-based row = local row + row_offset, j = 0-based column):
 *     z = the value of pmf_impute with PMF_IMPUTE_BATCH | PMF_IMPUTE_LINK, bit for bit (MF.forward(matfac), :247)
 *     Philox4x32-10 (Salmon et al., SC'11) with counter (i_lo, i_hi, j_lo, j_hi) and key (seed_lo, seed_hi) gives r0..r3;
 *     u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, n = sqrtf(-2 logf(u1)) cosf(6.28318530718f u2),
 *     u3 = (r2 >> 8) 2^-24 (missingness), u4 = (r3 >> 8) 2^-24 (Bernoulli)
 *     normal            -> fmaf(noise, n, z)  (:240-242; noise = 0 gives z itself)
 *     kind 3 (sq hinge) -> the number of the column's thresholds strictly below z: the class of the noise-free z (:224-238),
 *                          pmf_impute with PMF_IMPUTE_BATCH bit for bit
 *     bernoulli (logit) -> u4 < 1 / (1 + e^-z) ? 1 : 0   (no reference method)
 *     poisson           -> the call is refused (no reference method, no sampler)
 *     then u3 < frac_missing -> NaN  (frac_missing = 0: never; 1: always)
 * An entry's value depends on (parameters, seed, i, j, noise, frac_missing) alone: not on the row range, the chunking, ld,
 * the kind of output, pmf_set_precision or what the context ran before; a row shard with its row_offset reproduces its
 * rows of the whole matrix.
 *   pmf_simulate_data          : local rows row_start1..row_stop1 (1-based, inclusive) x all N columns into a HOST matrix,
 *                                column-major with leading dimension ld >= rows, as pmf_impute: through the context's staging
 *                                buffer of at most 256 MiB (PMF_SIMULATE_CHUNK_ROWS=n, read at every call, overrides the chunk
 *                                height); elements between the rows of a column are not written.
 *   pmf_simulate_data_device   : the same into DEVICE memory, one launch, no staging.
 *   pmf_simulate_data_resident : overwrites the whole data matrix resident on the device (bf16-rounded under PMF_STORE_BF16
 *                                exactly as pmf_set_data rounds): a later pmf_fit / pmf_loss / pmf_stats sees what
 *                                pmf_set_data of pmf_simulate_data's host matrix would give.  Needs the buffer that
 *                                pmf_set_data_device(ctx, NULL, M, N, store) or an earlier pmf_set_data allocated.
 * The calls change no parameter, gradient or optimizer state.  LOCAL ROWS ONLY: no communicator traffic.
 * Refused before anything is launched (the context stays usable): null options or output, noise negative or not finite,
 * frac_missing outside [0, 1] or NaN, row_offset < 0, an empty or out-of-range row range, ld below the row count, factors
 * or batch views not set, a noise range of kind poisson, pmf_simulate_data_resident without a data buffer. */
typedef struct pmf_sim_opts {
  uint64_t seed;
  int64_t row_offset;     /* global index of local row 1 (0 on one GPU; the shard's first row otherwise) */
  float noise;            /* standard deviation of the normal columns' noise (simulate_data!'s `noise`) */
  float frac_missing;     /* probability that an entry is NaN */
} pmf_sim_opts;
int pmf_simulate_data(pmf_ctx *ctx, const pmf_sim_opts *opts, int64_t row_start1, int64_t row_stop1, float *out_host, int64_t ld);
int pmf_simulate_data_device(pmf_ctx *ctx, const pmf_sim_opts *opts, int64_t row_start1, int64_t row_stop1, float *out_device,
                             int64_t ld);
int pmf_simulate_data_resident(pmf_ctx *ctx, const pmf_sim_opts *opts);

/* remove_batch_effect(model, Z) (src/remove_batch_effect.jl:3-16): the data with the fitted batch effects taken out, from
 * the context's CURRENT column parameters and batch views.  SELF-SPECIFIED (Deviation 3): the
 * reference's body reads fields that no longer exist and inverts an older layer order; this inverts the order the library
 * implements everywhere (src/layers.jl:240-253: z = (a sigma_j) delta_v[b,j] + mu_j + theta_v[b,j]).  Per entry with input
 * v, b = the batch of row i in column j's view:
 *     column in no batch view, or row in no batch (batch_of_row = -1)  ->  v, bit for bit
 *     kind 3 (squared hinge: class labels, there is no link)           ->  v, bit for bit
 *     v not finite (missing)                                           ->  NaN
 *     else  l = link(v) ; l' = ((l - theta_v[b,j]) - mu_j) / delta_v[b,j] + mu_j ; out = invlink(l')      (f32, in that order;
 *           the division is a multiplication by the hardware reciprocal of delta, 1 ulp, fused with the last addition)
 *           normal: identity ; bernoulli: log v - log(1 - v) in, 1 / (1 + e^-l') out (0 and 1 come back exactly) ;
 *           poisson: log v in, e^l' out (0 comes back as 0) ; a value outside a link's domain gives NaN
 * PMF_DEBATCH_LINK: input and output are both in link space; every column, kind 3 included, uses the identity link.
 * PMF_DEBATCH_FILL_MISSING: a non-finite input is replaced by the batch-free prediction, exactly pmf_impute with flags 0
 * (PMF_IMPUTE_LINK when PMF_DEBATCH_LINK is set): the prediction is written first, the observed entries over it.
 *   pmf_remove_batch_effect         : local rows row_start1..row_stop1 (1-based, inclusive) x all N columns.  Z_host points at
 *                         the first row of the range, column-major with leading dimension ldz >= rows; Z_host = NULL (ldz
 *                         ignored): the data matrix resident on the device is the input (bf16-rounded under PMF_STORE_BF16).
 *                         out_host: column-major, leading dimension ld >= rows; elements between the rows of a column are
 *                         not written.  Z_host == out_host with ldz == ld (in place) is legal.  Computed in row chunks of
 *                         whole 32-row blocks through the staging buffer of pmf_impute (at most 256 MiB;
 *                         PMF_DEBATCH_CHUNK_ROWS=n, read at every call, overrides the chunk height).
 *   pmf_remove_batch_effect_device  : the same between DEVICE matrices (Z_device = NULL: the resident data), one launch (two with
 *                         PMF_DEBATCH_FILL_MISSING), no staging.  In place is legal without PMF_DEBATCH_FILL_MISSING; any
 *                         other overlap of input and output is refused.
 *   pmf_remove_batch_effect_entries : the corrected values at n listed entries (rows1[e], cols1[e], 1-based; duplicates are
 *                         legal) of values[e], or of the resident data with values = NULL.  n = 0 succeeds and does nothing.
 * An entry's value does not depend on the row range, the chunking, ld / ldz, the input's source (for the same f32 value) or
 * what the context ran before.  The calls change nothing a later pmf_fit reads.  LOCAL ROWS ONLY: no communicator traffic.
 * Data and factors must have been set, as for pmf_impute.  Refused before anything is launched (the context stays usable):
 * a null output, unknown flag bits, an empty or out-of-range row range, ld or ldz below the row count,
 * PMF_DEBATCH_FILL_MISSING passed to pmf_remove_batch_effect_entries, an entry outside 1..M x 1..N, no resident data when
 * the input is NULL. */
#define PMF_DEBATCH_LINK 1          /* input and output in link space: the identity link for every column */
#define PMF_DEBATCH_FILL_MISSING 2  /* missing entries take pmf_impute's batch-free prediction instead of NaN */
int pmf_remove_batch_effect(pmf_ctx *ctx, int flags, int64_t row_start1, int64_t row_stop1, const float *Z_host, int64_t ldz,
                            float *out_host, int64_t ld);
int pmf_remove_batch_effect_device(pmf_ctx *ctx, int flags, int64_t row_start1, int64_t row_stop1, const float *Z_device,
                                   int64_t ldz, float *out_device, int64_t ld);
int pmf_remove_batch_effect_entries(pmf_ctx *ctx, int flags, int64_t n, const int64_t *rows1, const int64_t *cols1,
                                    const float *values, float *out_host);

/* Masked column statistics for the closed-form initialisers that sit between the GD stages (local rows only; a
 * multi-GPU host sums them across ranks).  All outputs are optional (NULL = not wanted).
 *   col_n[N]        MF.column_nonnan                         (src/fit.jl:140, 447; src/regularizers.jl:765)
 *   col_sum, col_sumsq[N]  -> MF.batched_column_nanvar       (src/regularizers.jl:766)
 *   col_sqerr[N]    MF.link_col_sqerr                        (src/fit.jl:138, 444)
 *   col_ssq_grad[N] MF.batched_column_ssq_grads              (src/fit.jl:166)
 *   batch_count / batch_sqerr: ba_map(isfinite), ba_map(MF.sqerr_func) (src/fit.jl:332, 355, 454-456;
 *                   src/batch_array.jl:305-334), flat over (view, column, batch) like logdelta / theta
 * use_factors = 0 evaluates the model with X'Y = 0, which is how the reference calls these (src/fit.jl:133-136, 160-163). */
int pmf_stats(pmf_ctx *ctx, int use_factors, float *col_n, float *col_sum, float *col_sumsq, float *col_sqerr,
              float *col_ssq_grad, float *batch_count, float *batch_sqerr);

/* The closed-form stages between the gradient-descent stages, each as ONE call on the context's current parameters.  Every
 * data pass is the column walk of pmf_stats; the statistics stay on the device, all arithmetic on them is float64 there, and a
 * result is rounded to float32 where the parameter is float32.  Every sum has a fixed order: an output is bitwise the same run
 * to run.  With a communicator of more than one rank (rows sharded) the statistics of a pass are widened to float64 and summed
 * over the ranks in ONE collective per pass before any arithmetic, so every rank computes the same bits and takes the same
 * stopping decision; a call that fails after its first launch drains both streams and marks the communicator unusable, as
 * pmf_fit does.  No entry touches X, Y, a gradient, the optimizer state, Adam's powers or the learning rate.
 *   pmf_stage_init_logsigma         : init_logsigma! (src/fit.jl:125-148).  Statistics with X'Y = 0;
 *                                     logsigma[j] <- log(sqrt(sqerr[j] / n[j])), written into the context's logsigma (read it
 *                                     with pmf_get_col_params).  IEEE results are kept: n = 0 gives NaN, a zero residual -inf.
 *   pmf_stage_reweight_col_losses   : reweight_col_losses! (src/fit.jl:151-187).  The noise weights are set to 1 (:157), the
 *                                     statistics taken with X'Y = 0 (:160-163), w[j] <- 1 / (sqrt(ssq_grad[j] / M_total) *
 *                                     exp(logsigma[j])) (:170-176), non-finite -> 1 (:177), written into the context's noise
 *                                     weights (:180).  M_total: all samples (the sum of the ranks' rows).
 *   pmf_get_noise_weights           : the context's per-column noise weights (MF.set_weight!, src/fit.jl:157, 180), N floats.
 *   pmf_stage_minimal_group_weights : construct_minimal_regularizer (src/regularizers.jl:750-774).  Per column range of the
 *                                     noise model (pmf_set_noise), K * mean(sigma^2) / (sum_j var[j] n[j] / M_total) with var
 *                                     the unbiased variance from sum / sumsq, non-finite -> 0, floored at 1 / M_total (:767).
 *                                     Output only (one float per noise range): the host builds the regularizer.
 *   pmf_stage_theta_delta_em        : theta_delta_em (src/fit.jl:326-375) with theta_mom / delta2_mom (:297-311).  theta is the
 *                                     context's theta, updated in place (read it with pmf_get_batch_view); delta2 (in / out,
 *                                     float64, flat over (view, column, batch) like theta) stays float64 on the device across
 *                                     the iterations; sigma2 has N entries.  batch_count is taken once, before the loop (:332).
 *                                     Per iteration: the theta update (:350, non-finite -> 0), one statistics pass with only the
 *                                     batch outputs (:355), the delta2 update (:359; batch_sqerr non-finite -> 0, the result
 *                                     non-finite -> 1), and ONE double read back, sum((theta - theta')^2) / sum(theta^2) (:363),
 *                                     on which the host loop decides (diff < rtol, :367).  iters = iterations run; the diffs
 *                                     go to a caller-owned buffer of diffs_cap entries (may be NULL), n_diffs written.
 * Refused before anything is launched (the context stays usable): no data or factors; pmf_stage_theta_delta_em without batch
 * views or with max_iter < 1; M_total below the context's row count; a NULL required pointer; more row batches per view than the
 * statistics kernel's LDS holds (pmf_stats' own message). */
typedef struct pmf_em_opts {
  int32_t update_priors;   /* re-estimate the priors' moments every iteration ("EM") or only at the first ("EB"), src/fit.jl:343 */
  int32_t max_iter;        /* batch_em_max_iter, >= 1 */
  int32_t verbosity;       /* > 0: one line per iteration (:365) */
  int32_t reserved;
  double rtol;             /* batch_em_rtol */
} pmf_em_opts;
typedef struct pmf_em_result {
  int32_t iters;
  int32_t n_diffs;     /* entries written to diffs */
  int32_t diffs_cap;   /* in: capacity of diffs */
  int32_t reserved;
  double *diffs;       /* in: host buffer (may be NULL) */
  double seconds;
} pmf_em_result;
int pmf_stage_init_logsigma(pmf_ctx *ctx);
int pmf_stage_reweight_col_losses(pmf_ctx *ctx, int64_t M_total);
int pmf_get_noise_weights(pmf_ctx *ctx, float *w);
int pmf_stage_minimal_group_weights(pmf_ctx *ctx, int64_t M_total, float *w_out);
int pmf_stage_theta_delta_em(pmf_ctx *ctx, const pmf_em_opts *opts, const float *sigma2, double *delta2,
                             pmf_em_result *result);

/* The factor post-processing stages that fit! runs between the gradient-descent stages, each as ONE call on the context's
 * resident X (K x M, the local rows) and Y (K x N).  Every sum is float64 with a fixed order (no atomics): an output is bitwise
 * the same run to run.  Every store of a float32 is ONE rounding of a float64 result (pmf_stage_whiten stores Y twice, where
 * the host stores it: see below).  With a communicator of more than one rank the
 * X-side sums are summed over the ranks in float64, in ONE collective per call, before any arithmetic; Y is replicated, so the
 * Y-side calls issue no collective and every rank computes the same bits.  Column ranges are 1-based and inclusive, disjoint
 * and ascending (gaps allowed).  The symmetric eigen-decomposition is the library's own cyclic Jacobi (no LAPACK): eigenvalues
 * descending, ties by original index; each eigenvector signed so that its largest-magnitude component is positive, ties by
 * lowest index; singular values sqrt(max(lambda, 0)).
 *   pmf_gram                        : G_g = P[:, a_g..b_g] P[:, a_g..b_g]' of P = X (which = 0) or Y (1): n_groups x K x K doubles,
 *                                     or with diag_only the n_groups x K diagonals (bitwise the diagonal of the full result).  A
 *                                     group a..a-1 has no columns (a row-sharded group without local rows) and gives zeros.
 *                                     X on more than one rank: the sums over all ranks (one collective).
 *   pmf_stage_lambda_max            : the largest eigenvalue of each group's (reduced) Gram matrix = the largest squared singular
 *                                     value of the block, by which reweight_eb! of L2Regularizer (one group, every column) and
 *                                     GroupRegularizer divide mixture_p (src/regularizers.jl:39-47, 406-420).  One collective on X.
 *   pmf_stage_whiten                : whiten! (src/fit.jl:504-527).  x_rms[k] = sqrt(sum_i X[k,i]^2 / M_total) (:505, one
 *                                     collective); X[k,:] /= x_rms[k] (:506); Y[k,:] *= x_rms[k] (:507); per view range
 *                                     c = max_k rms(Y[k, range]) of the rescaled Y (:513-517); c > 0: Y[:, range] /= c and
 *                                     logsigma[range] += log c (:519-520), else Y[:, range] = 0 and logsigma[range] = -1e9
 *                                     (:522-523).  Every step is float64 arithmetic that rounds once where it stores, in the
 *                                     host's order (Y is stored after :507 and again after :519); c is taken from the float64
 *                                     products Y * x_rms, so logsigma does not inherit Y's rounding.  IEEE results are kept: an
 *                                     all-zero factor of X gives NaN in that row of X and leaves Y's row zero.  Outputs (either
 *                                     may be NULL): x_rms[K], c[n_views].
 *   pmf_stage_rotate_by_svd         : rotate_by_svd! (src/fit.jl:530-543) through the Gram matrix: Y Y' = U S^2 U', Y <- U'Y (= S Vt,
 *                                     :538), X <- U'X (X' <- X'U, :541).  No collective.  Outputs (either may be NULL): the K
 *                                     singular values; U, K x K row-major, U[k*K + r] = component k of singular vector r.
 *   pmf_stage_reorder_by_importance : reorder_by_importance! (src/fit.jl:546-555): the rows of X and Y in the stable descending order
 *                                     of sum_j Y[k,j]^2 (:549).  perm_out[r] (0-based, K entries) = the old row now at r: the host
 *                                     permutes its regularizers with it (reorder_reg!, :552-553).  No collective.
 * Each entry invalidates the prepared column parameters where it rewrote logsigma (the split-precision images of X and Y are
 * rebuilt by every data pass).  None touches a gradient, the optimizer state, Adam's powers, the learning rate, the noise
 * weights or a layer parameter other than logsigma.
 * Refused before anything is launched (the context and the communicator stay usable): no data or factors; n_groups < 1; a range
 * outside the matrix; overlapping or descending ranges; M_total below the context's row count; a NULL required pointer.  A call
 * that fails after its first launch drains both streams and marks a communicator of more than one rank unusable. */
int pmf_gram(pmf_ctx *ctx, int which, int n_groups, const int64_t *starts1, const int64_t *stops1, int diag_only, double *out);
int pmf_stage_lambda_max(pmf_ctx *ctx, int which, int n_groups, const int64_t *starts1, const int64_t *stops1, double *lam_out);
int pmf_stage_whiten(pmf_ctx *ctx, int64_t M_total, int n_views, const int64_t *starts1, const int64_t *stops1,
                     double *x_rms_out, double *y_rms_max_out);
int pmf_stage_rotate_by_svd(pmf_ctx *ctx, double *sing_out, double *U_out);
int pmf_stage_reorder_by_importance(pmf_ctx *ctx, int32_t *perm_out);
/* host-clock seconds of the phases of the last of the five calls above on this context, each phase closed by a stream
 * synchronisation: the Gram / diagonal passes (with their collective and download), the eigen-solver, and the kernels that
 * rewrite X, Y and logsigma.  Any pointer may be NULL.  (scripts/kbench_postprocess.py) */
int pmf_debug_postprocess_times(pmf_ctx *ctx, double *gram_s, double *eig_s, double *apply_s);

/* FeatureSetARD outer loop, one view: update_A! / update_A_inner! (src/featureset_ard.jl:214-294) with ISTAOptimiser.update!
 * (src/optimizers.jl:26-62) and gamma_normal_loss + its pull-back (:154-186), run on the device against the context's
 * resident Y (columns col_start1:col_stop1 = the view's col_range).  A starts from 0 (:286); S is the view's L x N_v
 * feature-set matrix ROW-major (S[l*N_v + j]; the reference holds it as a sparse CSC, src/util.jl:453-477); alpha = the
 * regularizer's alpha[cr]; lambda = the optimiser's per-factor L1 weights (update_lambda!, :189-209); ssq_grad is the
 * optimiser's accumulator (in / out, persists across calls like A_opts); A and ssq_grad are L x K with the factor index
 * contiguous (A[l*K + k]).  On return A = A_best, *best_loss its loss, *epochs_run the updates performed, and
 * beta[:, cr] = (alpha0 - 1) (v0 + A'S) (:292) is written to beta_out (K x N_v column-major, may be NULL) and into the
 * device copy of the Y regularizer's beta when one is attached (pmf_add_yreg_fsard).
 * Refused before anything is launched: an empty or out-of-range column range, L < 1, L * K > 16384, max_epochs < 0 and
 * term_iter < 1 (the reference's loop makes its first update before it looks at the counter). */
int pmf_fsard_update_A(pmf_ctx *ctx, int64_t col_start1, int64_t col_stop1, int L, const float *S, const float *alpha,
                       const float *lambda, float alpha0, float v0, float lr, float *ssq_grad, float *A, int max_epochs,
                       int term_iter, double atol, double *best_loss, int *epochs_run, float *beta_out);
/* The same call on a sparse S, without a bound on L * K other than device memory: the arguments, outputs and semantics of
 * pmf_fsard_update_A, except that S comes as its 0-based CSR (rowptr[L + 1], col[nnz], val[nnz]; L rows = feature sets,
 * N_v columns = the view's columns; columns strictly ascending within a row; stored zeros are legal), as the reference
 * holds it (a SparseMatrixCSC, src/featureset_ard.jl:22).  A, the pull-back and the gradient live in device memory
 * (csrc/pmf_fsard_csr.hip: four launches per iteration, no atomics, every sum in an order fixed by the shapes, the loss in
 * f64); results agree with pmf_fsard_update_A to rounding, not bit for bit.
 * Refused before anything is allocated or launched, the message naming the argument, no output touched and the context
 * usable: an empty or out-of-range column range, L < 1, max_epochs < 0, term_iter < 1, a NULL rowptr / col / val / alpha /
 * lambda / ssq_grad / A, rowptr[0] != 0, a decreasing rowptr, a column index outside 0 .. N_v - 1, unsorted or repeated
 * columns in a row.  A failed allocation names its size. */
int pmf_fsard_update_A_csr(pmf_ctx *ctx, int64_t col_start1, int64_t col_stop1, int L, const int64_t *rowptr,
                           const int32_t *col, const float *val, const float *alpha, const float *lambda, float alpha0,
                           float v0, float lr, float *ssq_grad, float *A, int max_epochs, int term_iter, double atol,
                           double *best_loss, int *epochs_run, float *beta_out);

/* Arithmetic of the three matrix products of the fused data pass (no reference counterpart: the reference computes
 * in Float32 on the GPU, src/fit.jl:24 via MatFac):
 *   PMF_PREC_F32    (default) exact f32 MFMA, v_mfma_f32_32x32x2_f32
 *   PMF_PREC_BF16X3 split-bf16: every f32 operand as a bf16 hi/lo pair, three bf16 MFMAs per product, f32 accumulation;
 *                   a six-term forward product as accurate as the f32 MFMA (2e-7 of max|Z|), three-term gradient products
 *                   (4e-6).  Used where a kernel variant exists (every K <= 128; batch layers unless a 256-row panel meets more
 *                   than 15 batches of one view, pmf_debug_last_path); every other launch silently stays exact.
 * pmf_get_precision also reports how many fused launches of this context took the split-bf16 kernel. */
#define PMF_PREC_F32 0
#define PMF_PREC_BF16X3 1
int pmf_set_precision(pmf_ctx *ctx, int mode);
int pmf_get_precision(pmf_ctx *ctx, int *mode, int64_t *split_launches);

/* per-launch timing of the fused data-pass kernel (HIP events on the library's stream): mean milliseconds and
 * number of launches since the last reset */
int pmf_kernel_time(pmf_ctx *ctx, double *mean_ms, int64_t *launches, int reset);
/* fill the data matrix on the device with synthetic values (benchmarks; no host transfer):
 * D = X'Y*exp(logsigma)+mu + noise*N(0,1) by a counter-based RNG; frac_nan entries set to NaN */
int pmf_synth_data(pmf_ctx *ctx, uint64_t seed, float noise, float frac_nan);

#ifdef __cplusplus
}
#endif
#endif /* PMF_HIP_H */
