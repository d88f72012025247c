// pmf_ctx.h -- internal to libpmf_hip.so: the context behind the opaque `pmf_ctx` of include/pmf_hip.h and the host
// helpers its translation units share; DevBuf / PinnedBuf, the one type that allocates and frees device and pinned memory
// (every buffer below is a member of that type, or a local of one call: no capacity fields, no free lists).
//   pmf_hip.hip       C ABI (marshalling, step-level API, statistics), small kernels, the scalar column walk, layer-pass launches
//   pmf_pass.hip      host driver of the fused data pass: work split, family table, geometry, buffers, extents, launches
//   pmf_outputs.hip   pmf_forward, pmf_synth_data, pmf_impute*, pmf_remove_batch_effect* and the staging path they share
//   pmf_comm_fit.hip  cross-rank exchange (RCCL via dlopen / host-staged transport) and the epoch loop pmf_fit
//   pmf_fsard.hip     the FeatureSetARD update_A! solver (ISTA on the device; dense S, A in LDS, L x K <= 16384)
//   pmf_fsard_csr.hip the same solver on a sparse S with A in device memory (no bound on L x K)
//   pmf_fsard_loop.h  what those two share: the loop's formulas, bookkeeping and ISTA update, its checks and host driver
//   pmf_netreg.hip    NetworkRegularizer (per-factor CG solve + sparse gradient) and the L1 / SelectiveL1 weights
//   pmf_lbfgs.hip     L-BFGS over (X, Y): total gradient, history, two-loop recursion, backtracking (pmf_fit_lbfgs)
//   pmf_stages.hip    the closed-form stages between the GD stages on the device statistics (pmf_stage_*)
//   pmf_postprocess.hip  the factor post-processing stages (whiten, rotate_by_svd, reorder, lambda_max) on the resident X, Y
//   pmf_holdout.hip   hold-out entries: the set beside the resident D, the hold-out loss, tracking inside pmf_fit
#ifndef PMF_CTX_H
#define PMF_CTX_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "pmf_common.h"

// hipMemset on device memory is queued on the NULL stream and may return before it has run; the library's kernels and
// copies run on a NON-BLOCKING stream, which the NULL stream does not order (memset_now, pmf_hip.hip).
int memset_now(void *p, int v, size_t bytes);
// The one owner of device and pinned host memory: every allocation of the library is a DevBuf (PinnedBuf: the same
// type on hipHostMalloc), a member of the struct that uses it or a local of one call, and is freed by its destructor.
// size() is what is allocated, in elements: the capacity that grow sites (ensure) and the extents guard (bytes()) read.
// pmf_live_bytes counts what every DevBuf of the process holds: [0] device, [1] pinned (pmf_debug_live_bytes).
inline std::atomic<int64_t> pmf_live_bytes[2];
template <typename T, bool PINNED = false>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { free(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DevBuf() { free(); }
  operator T *() const { return p; }
  size_t size() const { return n; }
  size_t bytes() const { return n * sizeof(T); }
  void free() {
    if (p) {
      (void)(PINNED ? hipHostFree(p) : hipFree(p));
      pmf_live_bytes[PINNED] -= (int64_t)bytes();
    }
    p = nullptr; n = 0;
  }
  // always a fresh allocation of exactly max(count, 1) elements (the old contents are gone); `zero` fills it in NULL-stream
  // order (memset_now).  On failure the buffer is empty and the message names the size and `what`.
  int alloc(size_t count, bool zero, const char *what = nullptr) {
    free();
    count = std::max<size_t>(count, 1);
    const hipError_t e = PINNED ? hipHostMalloc((void **)&p, count * sizeof(T)) : hipMalloc((void **)&p, count * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      (void)hipGetLastError();
      return pmf_fail("cannot allocate %zu bytes of %s memory for %s: %s", count * sizeof(T), PINNED ? "pinned host" : "device",
                      what ? what : "a library buffer", hipGetErrorString(e));
    }
    n = count;
    pmf_live_bytes[PINNED] += (int64_t)bytes();
    if (zero) {
      if (PINNED) memset(p, 0, bytes());
      else PMFCHK(memset_now(p, 0, bytes()));
    }
    return 0;
  }
  // grow-only, exact, and never a copy of the old contents: a no-op while count <= size()
  int ensure(size_t count, bool zero, const char *what = nullptr) { return count <= n ? 0 : alloc(count, zero, what); }
  int upload(const T *src, size_t count) {
    if (count) HIPCHK(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
};
template <typename T>
using PinnedBuf = DevBuf<T, true>;

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct ParamBuf {  // one trainable parameter tensor with its gradient, optimizer state and quadratic regularizer
  DevBuf<float> p, g, acc, mom;
  DevBuf<float> wq, cq;  // dense quadratic weights / centres: 0.5*wq*(p-cq)^2 (empty = none)
  DevBuf<float> wl1;     // dense L1 weights w_k m_kj p: wl1*|p| (L1Regularizer / SelectiveL1Reg; empty = none)
  int64_t n = 0;         // logical length (Kp x rows for X, Y)
  float bp1 = 0.f, bp2 = 0.f;  // Adam running beta powers
};

// Panel-local batch slots.  The fused kernels look the batch parameters of (row, column) up in a 16-slot per-column table
// in LDS.  With more than 15 batches in a view the slots are numbered PER ROW PANEL: slot s of (panel, view) is the s-th
// distinct batch among the panel's rows (rows are normally sorted by batch: a 256-row panel holds a few), slot 15 the
// identity.  pm[(rp * n_bv + v) * 16 + s] = that batch (255 = unused), row_slot[v * M + i] = the slot of row i.
// ok = every (panel, view) has at most 15 distinct batches; otherwise the launch takes the gather fallback.
struct PanelSlots {
  int64_t serial = -1;
  int BM = 0;
  bool ok = false;
  DevBuf<uint8_t> pm, row_slot;
};

// Cached work split of one column chunk of the fused data pass (see compute_work_split).
struct WorkSplit {
  int64_t key[11] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
  int grid = 0;
  int64_t tps = 0, n_cseg = 0;     // column segmentation the split was made for (chunk_segments): tiles per segment, segments
  int64_t serial = 0;
  DevBuf<int64_t> wg_begin;        // [grid + 1] device: first work item of each workgroup
  DevBuf<int32_t> c_off, c_idx;    // per column tile of the chunk: the workgroups that visit it (CSR; k_gy_reduce)
  DevBuf<int32_t> piece_base;      // [grid] device: chunk-relative slot of each workgroup's first piece (gX partial buffer)
  std::vector<int32_t> h_piece_base;
  std::vector<int32_t> piece_rp;   // host: row panel of every piece, in slot order
  int32_t slot_base = 0;           // first slot of this chunk in the flat gX partial buffer (set with the CSR)
  DevBuf<int32_t> d_piece_base_abs;      // [grid] device: piece_base + slot_base
};

// Cross-rank exchange of the sharded fit: rows are sharded, Y / column layers replicated; per epoch the
// partial grad(Y) (and layer gradients, and the local loss) are summed over the ranks.  Two transports behind one
// interface: RCCL (ncclAllReduce on a communication stream of the library's own, overlapped with the data pass), or a
// host-staged callback (tests: two ranks sharing one GPU cannot form an RCCL ring).
struct Comm {
  int rank = 0, nranks = 1;
  void *nccl = nullptr;            // ncclComm_t (RCCL transport)
  pmf_host_allreduce_fn host_fn = nullptr;
  void *host_user = nullptr;
  hipStream_t stream = nullptr;    // communication stream
  PinnedBuf<char> stage;           // pinned staging buffer of the host-staged transport, grown on demand
  int reserve_cus = 0;             // CUs left to the collective's kernels by the fused pass (RCCL transport)
  int cta_cap = 0;                 // workgroups the communicator is configured for (ncclConfig_t.maxCTAs); 0 = RCCL's default
  DevBuf<char> dstage;             // device staging buffer of pmf_comm_allreduce (host buffers), grown on demand
  bool broken = false;             // a fit failed with collectives possibly unmatched: the communicator must be destroyed
  int64_t m_mean = 0;              // rows per rank averaged over the ranks (pmf_fit): the rank-invariant size behind the chunk count
  std::vector<hipEvent_t> ev_ready, ev_done;   // per chunk: gY slice complete / its all-reduce complete
  hipEvent_t ev_loss_ready = nullptr, ev_loss_done = nullptr, ev_layer_ready = nullptr, ev_layer_done = nullptr;
  hipEvent_t ev_thr_ready = nullptr, ev_thr_done = nullptr;   // the threshold group sums of a training fit (pmf_thresh.hip)
  int64_t n_allreduce = 0;         // collectives issued (diagnostics / tests)
};

// NetworkRegularizer on X (n = M) or Y (n = N): per factor k the sparse blocks AA_k (n x n), AB_k (n x v_k), AB_k' and
// BB_k (v_k x v_k), each family concatenated over the factors into one CSR whose row pointers are absolute (factor k's
// rows start at k * (n + 1) for AA / AB and at voff[k] + k for AB' / BB).  State: u (the reference's x_virtual), kept from
// epoch to epoch as the warm start of the next solve.  See pmf_netreg.hip.
struct NetReg {
  int K = 0;
  int64_t n = 0, V = 0;            // V = sum of v_k
  float p = 1.f;                   // mixture weight
  std::vector<int64_t> h_voff;     // [K + 1]
  DevBuf<int64_t> voff;            // device copy
  DevBuf<int64_t> aa_rp, ab_rp, abt_rp, bb_rp;
  DevBuf<int32_t> aa_col, ab_col, abt_col, bb_col;
  DevBuf<float> aa_val, ab_val, abt_val, bb_val;
  DevBuf<float> u;                 // [V]
  DevBuf<float> work;              // [4 V] t, r, d, BB d of the factors whose v_k exceeds the LDS budget
  DevBuf<float> PT;                // [K][n] factor-major copy of the parameter, rebuilt every epoch
  DevBuf<float> grad;              // [Kp * n] p * (AA_k p_k + AB_k u_k), in the parameter's own layout (read by k_reg_step<true>)
  DevBuf<int32_t> iters;           // [K] CG iterations of the last solve
  DevBuf<double> uloss;            // [K] t'u + 0.5 u'BB u of the last solve
  int rb = 1;                      // row blocks per factor of the gradient kernel (= loss partials per factor)
  int64_t vmax = 0;                // largest v_k
};

// Trainable thresholds of the squared-hinge noise models (pmf_thresh.hip; include/pmf_hip_thresholds.h).  A group is a
// noise range whose columns are all of kind 3; the triples and their optimizer state live per group, the per-column images
// (thr, htab) are rebuilt from them on the device after every step.
struct ThreshState {
  bool train = false;                   // pmf_set_threshold_training
  std::vector<int64_t> g_s1, g_e1;      // the groups (1-based inclusive) the state below belongs to
  DevBuf<float> t, acc, mom;            // [3 groups] thresholds, optimizer state
  float bp1 = 0.f, bp2 = 0.f;           // Adam's running beta powers
  bool state_init = false;              // (init_opt_state clears it with the other parameters' state)
  std::vector<int32_t> h_tiles;         // the column tiles that hold a kind-3 column, ascending
  DevBuf<int32_t> tiles, col_group;     // device copy; [N] group of every column (-1: none)
  DevBuf<int64_t> g_c0, g_c1;           // [groups] 0-based first column, one past the last
  DevBuf<float> slots;                  // [R * waves][tiles][PMF_TSLOT] private partial sums of the pass
  DevBuf<double> gcol, G;               // [3 N] per column, [3 groups] per group: float64 sums of the last pass
  int n_tiles = 0, n_units = 0, grid = 0;   // geometry of the last pass (pmf_debug_threshold_pass)
  int64_t passes = 0;
};

// Factor importance (pmf_factor_importance, pmf_outputs.hip; include/pmf_hip_importance.h): the private float64 slabs of the
// pass, its device outputs, and the geometry of the last call (pmf_debug_factor_importance).
struct ImportanceState {
  DevBuf<double> slabs;                 // [column tiles of a launch][R][Kp + 4][32]
  DevBuf<double> out;                   // [K N] delta | [N] full | [N] null | [N] n_obs
  int kb = 0, nw = 0, db = 0, R = 0, n_units = 0, grid = 0, launches = 0, flushes = 0;
  int64_t calls = 0;
};

// Hold-out entries (pmf_holdout.hip; include/pmf_hip_holdout.h): the set in CSC form beside the resident D, the work units
// and outputs of the hold-out pass, the tracking options, and what the last pmf_fit recorded.
struct HoldoutState {
  int64_t n = 0;                        // entries held (0: no set)
  std::vector<int64_t> h_colptr;        // [N + 1] host copy of colptr (unit table, n_col)
  DevBuf<int64_t> colptr;               // [N + 1]
  DevBuf<int32_t> rows;                 // [n] 0-based, sorted by (column, row)
  DevBuf<float> vals;                   // [n] the values D held (bf16 store: the stored, rounded ones)
  int unit_cap = 0;                     // PMF_HOLDOUT_UNIT the unit table was built for (0: not built)
  int n_units = 0, grid = 0;            // geometry of the last pass (pmf_debug_holdout_pass)
  DevBuf<int32_t> u_col, u_cnt;         // [n_units]
  DevBuf<int64_t> u_e0;
  DevBuf<float> lbuf;                   // [n] per-entry losses of the last pass
  DevBuf<double> loss_col;              // [N]
  DevBuf<double> d_total;               // [1] the total of a pmf_holdout_loss call (a fit's goes to d_loss[5])
  int64_t passes = 0;
  // tracking (pmf_set_holdout_tracking)
  int every = 0, patience = 0, restore_best = 0;
  double min_delta = 0.0;
  // the last pmf_fit
  std::vector<int32_t> tr_epoch;
  std::vector<double> tr_loss;
  int best_epoch = 0;
  double best_loss = 0.0;
  DevBuf<float> cand[2], best[2];       // X / Y of the evaluation epoch under way, of the best one (restore_best only)
};

struct pmf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  int n_cu = 256;
  int64_t M = 0, N = 0;
  int K = 0, Kp = 0, KB = 0;
  DevBuf<char> D;      // tile-major copy of the data matrix, f32 (pmf_d_off) or bf16 (pmf_d_off16, `store`), always library-owned
  bool own_D = false;
  int64_t D_M = 0, D_Npad = 0, nRB = 0;
  DevBuf<uint32_t> tflags;        // per 32x32 tile of D: 1 = all 1024 entries finite (fast epilogue path of the fused kernel)
  bool tflags_valid = false;
  // plain-run table of the exact kernel's 256-row panels (k_plain_table): [ptab_n_rp][ptab_n_ct + 1] running counts along a
  // panel's column tiles of the tiles with a row block that is not all-finite.  Follows tflags: D changes, both are rebuilt.
  DevBuf<int32_t> ptab;
  int64_t ptab_bm = 0, ptab_n_rp = 0, ptab_n_ct = 0;   // panel height and shape it was built for (ptab_bm 0: not built)
  DevBuf<int32_t> plain_count;    // per workgroup and chunk: tiles the last pass ran in the plain loop (beside loss_partial)
  int64_t last_plain_n = -1;      // live entries of plain_count written by the last pass (-1: it had no plain loop)
  int store = PMF_STORE_F32;
  ParamBuf P[6];  // X, Y, logsigma, mu, logdelta, theta
  // batch views
  int n_bv = 0;
  std::vector<ViewDesc> views;
  std::vector<int64_t> val_off;  // per view offset into the flat logdelta/theta arrays
  std::vector<int64_t> bvb_off;  // per view offset into the flat per-(view,batch) arrays
  DevBuf<int32_t> bor;
  DevBuf<float2> btab;
  bool views_dirty = true;        // `views` changed since the last upload
  DevBuf<ViewDesc> d_views;       // device copy of `views` for the fused kernel's global-gather fallback
  DevBuf<float2> LG;              // [R * waves * 2][N][nbs] {S_G, S_Q}: the private tables of the layer pass (pmf_layers.hip.inc)
  DevBuf<float> lgrad_part;       // [block rows][2N + 2 nbt] private partials of k_layer_grad (fixed-order k_sum_parts)
  DevBuf<float2> btd;             // dense per-column batch table [ceil(N/32)*32][nbs] (fused kernels, layer pass); see k_dense_btab
  bool btd_ok = false;            // the dense table is built (every view has <= 255 batches)
  int nbs = 16;                   // slots per column of the dense table: 16, or the power of two above the largest batch count (0: no table)
  DevBuf<uint8_t> colview;        // [ceil(N/32)*32] view of every column, 255 = none (k_dense_btab)
  std::vector<std::vector<int32_t>> h_bor;   // host copy of batch_of_row per view (panel-local slot maps)
  PanelSlots pslots[3];           // panel-local batch slots for row panels of 128 / 256 / 512 rows (ensure_panel_slots)
  int64_t views_serial = 0;       // bumped whenever a view's rows / shape change
  int last_kernel = 0;            // fused kernel family of the last data pass (pmf_debug_last_kernel)
  int last_bmode = 0, last_layer_path = 0, last_xreg = 0;   // diagnostics (pmf_debug_last_path)
  DevBuf<int32_t> d_val_view;     // per flat value element: view id
  // noise model / prepared column parameters
  DevBuf<int32_t> colmeta;     // kind | (view+1)<<2
  DevBuf<float> colw;
  DevBuf<float4> colp;
  DevBuf<float4> thr;          // per column {t0, t1, t2, 0}, N padded to a multiple of PMF_DPAD: thresholds of the kind-3 columns ((0, +Inf, +Inf)
                               // elsewhere).  thr and htab exist while the noise model has a column that is not normal (upload_thresholds)
  DevBuf<float> htab;          // per column the PMF_HT-float table of class bounds built from thr (pmf_hinge_terms), same padding
  std::vector<float> h_thr;    // host copy, 3 per column (pmf_get_noise_thresholds; NaN for the other kinds)
  bool mixed = false;
  bool prepared = false;
  // ARD-type regularizer on Y
  DevBuf<float> ard_alpha, ard_beta;
  float ard_scale = 0.f;
  bool has_ard = false;
  bool ard_is_fsard = false;       // the attached term came from pmf_add_yreg_fsard (the only kind pmf_fsard_update_A writes beta into)
  // optimizer
  int opt_kind = PMF_OPT_ADAGRAD;
  float lr = 1.f, eps = 1e-8f, b1 = 0.9f, b2 = 0.999f;
  bool state_init = false;
  // loss plumbing
  DevBuf<double> loss_partial;    // the data pass's loss partials: n_macro of them are live (k_loss_reduce)
  std::vector<uint8_t> h_kind;    // host copy of the per-column noise kind (cost model of the work split)
  std::vector<int64_t> noise_s1, noise_e1;   // the noise model's column ranges as pmf_set_noise got them (pmf_stage_minimal_group_weights)
  std::vector<WorkSplit> splits;  // cached work split of every column chunk of the fused pass (compute_work_split)
  int n_chunks_req = 0;           // column chunks per data pass: 0 = automatic (1 on one GPU; pmf_comm_set_chunks)
  DevBuf<float> gx_part;          // [pieces][BM x Kp] per-piece partial sums of gX (fused kernel), summed by k_gx_reduce
  DevBuf<int32_t> gx_off, gx_idx; // per row panel: the slots of its pieces, in work-sequence order (CSR)
  int64_t gx_serial = -1;         // sum of the splits' serials the CSR was built for
  int64_t split_serial = 0;       // bumped whenever a split is recomputed
  Comm comm;                      // cross-rank exchange (pmf_comm_init*); nranks == 1: none
  int last_chunks = 1;            // column chunks of the last pmf_fit's data pass (pmf_comm_info)
  hipEvent_t ev_host = nullptr;   // "the epoch's loss has reached the host" (pmf_fit)
  int64_t kind_version = 0;
  DevBuf<float> gy_slabs;         // [grid][Kp x N] private per-workgroup gY partial sums of the fused kernel, the padding tile included
  int precision = PMF_PREC_F32;   // products of the fused data pass: exact f32 MFMA, or split-bf16 (pmf_set_precision)
  DevBuf<char> xsb, ysb;          // split-bf16 operand images of X / sigma*Y, rebuilt every epoch (k_sb_split; xsb: its sixteen blocks of padding included)
  DevBuf<float> sb8_scale;        // [1 + chunks] power-of-two pre-scales of pmf_fused_sb8_kernel's f16 images: X, then Y per chunk
  DevBuf<uint32_t> sb8_max;       // [1 + chunks] bit patterns of max |operand| (k_sb8_absmax)
  int64_t sb_launches = 0;        // fused launches that took the split-bf16 kernel (pmf_get_precision)
  int64_t n_macro = 0;
  DevBuf<double> reg_partial;     // [4][REG_SLOTS]
  DevBuf<double> d_loss;          // device [8]
  PinnedBuf<double> h_loss;       // pinned host [8]
  // fused-kernel timing
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  double kernel_ms_sum = 0.0;
  int64_t kernel_launches = 0;
  NetReg *net[2] = {nullptr, nullptr};   // NetworkRegularizer on X / Y (nullptr = none)
  int reg_counts[4] = {0, 0, 0, 0};  // used slots of the regularizer partial slabs (0 X, 1 Y, 2 column layers)
  // scratch
  DevBuf<char> scratch;
  // staging buffer of pmf_impute / pmf_impute_entries (at most 256 MiB unless one row of N predictions is larger), grown
  // lazily; not `scratch`, which those calls leave alone
  DevBuf<char> impute_stage;
  // largest dynamic-LDS size set so far per kernel ON THIS CONTEXT'S DEVICE (hipFuncSetAttribute is per device: a
  // process-wide cache would leave a second GPU's kernels without the attribute)
  PmfDynLds dyn_lds;
  double pp_seconds[3] = {0.0, 0.0, 0.0};   // phases of the last post-processing call (pmf_postprocess.hip, PpClock)
  struct LbfgsState *lbfgs = nullptr;   // vectors and scalars of pmf_fit_lbfgs (pmf_lbfgs.hip), allocated on its first call
  ThreshState th;                       // trainable squared-hinge thresholds (pmf_thresh.hip)
  ImportanceState imp;                  // factor importance (pmf_outputs.hip)
  HoldoutState ho;                      // hold-out entries (pmf_holdout.hip)
};

#define REG_SLOTS 1024
#define PMF_MAX_CHUNKS 16

// The PMF_* environment switches of the data pass as fused_geometry found them (read_pass_switches in pmf_pass.hip, the one
// place that reads them; DESIGN.md section 10 has their meanings).  -1: not set.
struct PassSwitches {
  bool sb2 = true, xgemm3 = true, xreg = true, plain = true;   // PMF_SB2 / PMF_XGEMM3 / PMF_XREG / PMF_PLAIN: false when = 0
  int sb8 = 1;                                                  // PMF_SB8
  bool rbw1 = false;                                            // PMF_RBW=1
  bool dbg_set = false; int dbg = 0;                            // PMF_DEBUG_FLAGS: set at all (even to 0); its bits
  int reserve_cus = -1;                                         // PMF_RESERVE_CUS, clamped to [0, n_cu / 2]
  double tps_scale = 1.0, algbw_gbps = 60.0;                    // PMF_TPS_SCALE; PMF_COMM_ALGBW_GBPS where > 0
  int w_bern = -1, w_pois = -1, w_hinge = -1, w_batch = -1;     // PMF_W_*: at least 16, PMF_W_BATCH at least 0
};

// One fused data pass as decided before its first launch (fused_geometry): kernel family and instance, what it computes,
// the switches it runs under, row panels, column chunks.
struct FusedFamily;   // a row of the family table (pmf_pass.hip): kernel, panel height, operand images, launchers
struct FusedGeom {
  const FusedFamily *fam = nullptr;
  bool want_gx = false, want_gy = false;
  FusedInstance inst;   // the instance of the family's kernel: batch mode, mixed noise models, gradient mode, xw / xr
  PassSwitches sw;
  int grid_max = 256, S = 1;
  PanelSlots *ps = nullptr;
  int64_t n_rp = 0, n_ct_all = 0;
  int64_t ct0[PMF_MAX_CHUNKS], nct[PMF_MAX_CHUNKS];
  // the instance has the plain tile loop: the pass reads the plain-run table and writes the per-workgroup counts
  bool has_plain_loop() const { return inst.xw && inst.xr; }
};

struct RegCounts { int c[4]; };

__device__ __forceinline__ double block_reduce_sum(double v, double *sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) s += sh[q];
  return s;  // valid on thread 0
}
// sum over a workgroup of 256 threads in a fixed order: lanes by shuffles, the four waves in index order; every thread
// gets it, and sh (4 doubles) is free again on return
__device__ __forceinline__ double block_all_sum_256(double v, double *sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return s;
}

// ---- the regularizer + optimizer step kernel's arguments (k_reg_step, pmf_hip.hip) and the per-entry value and gradient
// of the smooth element-wise terms, shared with the total-gradient kernel of pmf_lbfgs.hip
struct StepArgs {
  float *p, *g, *acc, *mom;
  const float *wq, *cq;          // quadratic regularizer (may be null)
  const float *ard_alpha, *ard_beta;  // ARD-type regularizer (Y only; may be null)
  float ard_scale;
  int64_t n;   // elements
  int Kp, K;   // leading dimension and number of live rows (Kp == K == 1 for vectors)
  int opt_kind;
  float lr, eps, b1, b2, c1, c2;  // c1 = 1 - beta1^t, c2 = 1 - beta2^t
  int do_step;   // 0: only evaluate the regularizer loss (parameter frozen for stepping)
  int use_reg;
  double *reg_partial;  // [REG_SLOTS]
};
// quadratic : 0.5 w (p - c)^2, gradient w (p - c)
__device__ __forceinline__ void pmf_reg_quad(float p, float w, float cq, float &g, double &lacc) {
  const float d = p - cq;
  const float gr = w * d;
  lacc += 0.5 * (double)(gr * d);
  g += gr;
}
// ARD-type  : scale (0.5 + alpha) log(1 + (0.5 / beta) p^2), gradient scale (alpha + 0.5) p / (b beta)
__device__ __forceinline__ void pmf_reg_ard(float p, float be, float al, float scale, float &g, double &lacc) {
  const float b = 1.f + (0.5f / be) * (p * p);
  lacc += (double)(scale * (0.5f + al) * logf(b));
  g += scale * ((al + 0.5f) * p / (b * be));
}

// ---- small host helpers
inline int nblocks(int64_t n, int bs) { return (int)((n + bs - 1) / bs); }
// the by-value copy of the batch views (and of their offsets into logdelta / theta) a kernel's argument struct carries
inline void fill_views(const pmf_ctx *c, ViewDesc *views, int64_t *val_off = nullptr) {
  for (int v = 0; v < c->n_bv; ++v) {
    views[v] = c->views[v];
    if (val_off) val_off[v] = c->val_off[v];
  }
}
// room for the n loss partials of the pass about to be launched, which k_loss_reduce will then sum
inline int ensure_loss_partials(pmf_ctx *c, int64_t n) {
  PMFCHK(c->loss_partial.ensure((size_t)n, true));
  c->n_macro = n;
  return 0;
}
// a call's temporary: n elements (not zeroed) holding a copy of src
template <typename T>
int upload_new(DevBuf<T> &b, const T *src, size_t n) {
  PMFCHK(b.alloc(n, false));
  return b.upload(src, n);
}
template <typename T>
int upload_vec(pmf_ctx *c, std::common_type_t<T> *dst, const T *src, size_t n) {   // (T is deduced from src alone: dst may be a DevBuf)
  if (n == 0) return 0;
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- defined in pmf_hip.hip
int ctx_bind(pmf_ctx *c);
int ensure_dyn_lds(pmf_ctx *c, const void *kern, size_t lds);
int check_ready(pmf_ctx *c);
int prepare(pmf_ctx *c);   // the column / batch tables (colp, btab, the dense table) from the current layer parameters
int upload_padded(pmf_ctx *c, float *dst, const float *src, int64_t n, float padval);   // host K x n -> device Kp x n
int download_padded(pmf_ctx *c, float *dst_host, const float *src_dev, int64_t n);      // and back
int epoch_open(pmf_ctx *c, const pmf_fit_opts *o);
int epoch_layer_pass(pmf_ctx *c, const pmf_fit_opts *o, bool with_loss);
int step_param_range(pmf_ctx *c, int which, int64_t e0, int64_t n, bool do_step, bool use_reg, int reg_slot, int *reg_count,
                     int max_blocks, bool advance);
int step_param(pmf_ctx *c, int which, bool do_step, bool use_reg, int reg_slot, int *reg_count);
int step_layers(pmf_ctx *c, const pmf_fit_opts *o, int *reg_count);
// fixed-order reduction of the loss partial slabs into d_loss[which] for every bit `which` of mask (0 data term, 1 X reg,
// 2 Y reg, 3 layer regs, 4 spare)
int launch_loss_reduce(pmf_ctx *c, const RegCounts &rc, int mask);
// the k_reg_step arguments of X (0) / Y (1) over the whole tensor, without optimizer or loss slab: its element-wise terms
void step_args_xy(pmf_ctx *c, int which, StepArgs *s);
// data loss + X regularizer + Y regularizer at the current parameters: out = {total, data, xreg, yreg}.  Always the exact
// f32 data pass; writes no parameter, gradient or optimizer state (pmf_loss).
int eval_full_loss(pmf_ctx *c, double out[4]);
// the fused data pass with both gradients in the context's precision mode: grad(X), grad(Y) of the data term, on the stream
int eval_data_grads(pmf_ctx *c);
// One k_stats pass over the local rows at the current parameters (prepare() + column walk + fixed-order sum of the block
// rows), left ON THE DEVICE in the context's scratch buffer, valid until the next call that uses it: *cols = {n, sum, sumsq,
// sqerr, ssq_grad}, N floats each (null unless want_cols), *batch = {count, sqerr}, flat like theta each (null unless
// want_batch and the model has batch views).  No host synchronisation.  stats_pass_check: the pass's LDS refusal, and
// nothing else, ahead of a caller that must not launch anything before it knows the pass will run.
int stats_pass_check(pmf_ctx *c);
int stats_pass(pmf_ctx *c, int use_factors, bool want_cols, bool want_batch, const float **cols, const float **batch);
// ---- defined in pmf_pass.hip
int harvest_events(pmf_ctx *c);
int launch_fused(pmf_ctx *c, bool want_gx, bool want_gy);   // the whole data pass in one go (chunks only on request)
FusedGeom fused_geometry(pmf_ctx *c, bool want_gx, bool want_gy, bool allow_chunks);   // (reads the PMF_* switches of the pass)
int prepare_fused_pass(pmf_ctx *c, const FusedGeom &g);
int launch_fused_chunk(pmf_ctx *c, const FusedGeom &g, int s);
// What the kernels of a prepared data pass address in every grow-only buffer against what is allocated, in bytes
// ("Extents").  fused_pass_extents fills out[PMF_PASS_EXTENTS] and returns the count;
// check_pass_extents fails on the first need > cap, naming the buffer; guard_fused_pass is both, between
// prepare_fused_pass and the first launch of the pass: a few integer compares, no device work.
struct PassExtent { const char *name; int64_t need, cap; };
constexpr int PMF_PASS_EXTENTS = 12;   // ten rows of every pass + ptab and plain_count of a pass whose kernel has the plain loop
int fused_pass_extents(pmf_ctx *c, const FusedGeom &g, PassExtent *out);
int check_pass_extents(const PassExtent *e, int n);
int guard_fused_pass(pmf_ctx *c, const FusedGeom &g);
// ---- defined in pmf_lbfgs.hip
void lbfgs_free(pmf_ctx *c);
// ---- defined in pmf_netreg.hip
void netreg_free(pmf_ctx *c, int which);   // drops the network term of X (0) / Y (1) and its state
// evaluates the network term from the current parameter: u_k, its gradient buffer and its loss partials (appended to
// slab `which`, *reg_count moved on).  No-op without a term.
int netreg_eval(pmf_ctx *c, int which, int *reg_count);
// ---- defined in pmf_thresh.hip: the thresholds inside pmf_fit (include/pmf_hip_thresholds.h)
// what a training fit checks before anything is launched: *active = training is on and the noise model has a group; fails
// when a group's columns do not all hold the same triple.  Brings the groups' device state up to date with the noise model.
int thresh_fit_check(pmf_ctx *c, bool *active);
int thresh_fit_begin(pmf_ctx *c);   // after the first epoch_open: the pass's own refusals, the optimizer state
int thresh_pass(pmf_ctx *c);        // one threshold pass at the current parameters: th.gcol, th.G (float64, on the stream)
int thresh_step(pmf_ctx *c);        // optimizer step from th.G, order clamp, the per-column images
int thresh_fit_end(pmf_ctx *c);     // h_thr <- the groups' triples (the stream is idle)
// ---- defined in pmf_holdout.hip: the hold-out set inside pmf_fit and beside the data (include/pmf_hip_holdout.h)
void holdout_drop(pmf_ctx *c);        // the resident data is being replaced: the set goes, nothing is written back
// what a tracking fit checks before anything is launched: *active = tracking is on and a set is held; the refusals of
// pmf_hip_holdout.h; clears the last fit's trace, builds the unit table and the restore buffers
int holdout_fit_check(pmf_ctx *c, const pmf_fit_opts *o, bool th_on, bool *active);
// one hold-out pass at the current parameters on the stream: ho.loss_col, and the total at *d_total (device).  No host sync.
int holdout_pass(pmf_ctx *c, double *d_total);
int holdout_fit_snapshot(pmf_ctx *c, bool ux, bool uy);   // restore_best: the factors about to be stepped -> the candidate
// the evaluation of `epoch` has reached the host: records it; true when `patience` evaluations in a row did not improve
bool holdout_fit_record(pmf_ctx *c, int epoch, double H);
int holdout_fit_end(pmf_ctx *c, bool ux, bool uy);        // (the stream is idle) restore_best: X, Y <- the best epoch's
// ---- defined in pmf_comm_fit.hip
int comm_release(pmf_ctx *c);
bool comm_active(const pmf_ctx *c);
// in-place sum over the ranks of `count` elements (f32 / f64) at device address p, ordered on the communication stream
int comm_allreduce(pmf_ctx *c, void *p, int64_t count, bool f64);
// the error exit of a call that may have left collectives unmatched: drains both streams, marks a communicator of more than
// one rank unusable and appends that to the message; returns rc
int comm_error_exit(pmf_ctx *c, int rc);
#endif
