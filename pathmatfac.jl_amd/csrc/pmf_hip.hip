// pmf_hip.hip -- libpmf_hip.so : MI355X (gfx950) implementation of PathMatFac's fit! loop behind the C ABI of
// include/pmf_hip.h.  Written for CDNA4 only (wave64, v_mfma_f32_32x32x2_f32, 160 KiB LDS).
#include "pmf_ctx.h"

// ------------------------------------------------------------------------------------------------
// error handling
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int pmf_fail(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}
extern "C" const char *pmf_last_error(void) { return g_err.c_str(); }
extern "C" int pmf_version(void) { return 1; }

int ctx_bind(pmf_ctx *c) {
  if (!c) return pmf_fail("null context");
  HIPCHK(hipSetDevice(c->device));
  return 0;
}

// hipMemset on device memory is queued on the NULL stream and may return before it has run; the library's kernels and
// copies run on a NON-BLOCKING stream, which the NULL stream does not order.  Without the wait a later upload on the
// library's stream can be overtaken by the fill (seen with two processes sharing one GPU: a regularizer's beta zeroed
// after its upload).
int memset_now(void *p, int v, size_t bytes) {
  HIPCHK(hipMemset(p, v, bytes));
  HIPCHK(hipStreamSynchronize(nullptr));
  return 0;
}

static int param_alloc(ParamBuf &b, int64_t n) {
  b.n = n;
  for (auto *t : {&b.p, &b.g, &b.acc, &b.mom}) PMFCHK(t->alloc((size_t)n, true));   // (always fresh: the optimizer state restarts)
  for (auto *t : {&b.wq, &b.cq, &b.wl1}) t->free();
  return 0;
}

int pmf_ensure_dyn_lds(PmfDynLds *cache, const void *kern, size_t lds) {
  auto it = cache->find(kern);
  if (it != cache->end() && it->second >= lds) return 0;
  HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  (*cache)[kern] = lds;
  return 0;
}
int ensure_dyn_lds(pmf_ctx *c, const void *kern, size_t lds) { return pmf_ensure_dyn_lds(&c->dyn_lds, kern, lds); }

// ------------------------------------------------------------------------------------------------
// small kernels
// ------------------------------------------------------------------------------------------------
__global__ void k_fill(float *p, int64_t n, float v) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) p[e] = v;
}

// colp[j] = {exp(logsigma_j), mu_j, w_j, meta_j}; btab[e] = {exp(logdelta_e), theta_e}
__global__ void k_prepare(const float *logsigma, const float *mu, const float *colw, const int32_t *colmeta,
                          float4 *colp, int64_t N, const float *logdelta, const float *theta, float2 *btab,
                          int64_t nbt) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e < N) colp[e] = make_float4(expf(logsigma[e]), mu[e], colw[e], __int_as_float(colmeta[e]));
  if (e < nbt) btab[e] = make_float2(expf(logdelta[e]), theta[e]);
}

// Dense form of the batch tables for the fused kernel: btd[j*16 + b] = {exp(logdelta), theta} of (column j's view,
// batch b), identity {1, 0} for b >= the view's batch count (slot 15 is always identity: rows outside every batch),
// for columns outside every view and for the pad columns up to the next multiple of 32.  A tile's 32 columns are then
// one contiguous 4-KiB read, staged in LDS, and the epilogue needs no view arithmetic.
struct DenseBtabArgs {
  const int32_t *colmeta;
  const float2 *btab;
  float2 *btd;
  uint8_t *colview;
  int64_t N, Npad;
  int32_t nbs_shift;
  ViewDesc views[PMF_MAXV];
};
// (nbs = 1 << nbs_shift slots per column; the LAST slot is always the identity: rows outside every batch)
__global__ void k_dense_btab(const DenseBtabArgs a) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= (a.Npad << a.nbs_shift)) return;
  const int64_t j = e >> a.nbs_shift;
  const int b = (int)(e & ((1 << a.nbs_shift) - 1));
  float2 out = make_float2(1.f, 0.f);
  int v = -1;
  if (j < a.N) {
    v = pmf_meta_view(a.colmeta[j]);
    if (v >= 0 && b < a.views[v].nb && b < (1 << a.nbs_shift) - 1) out = a.btab[pmf_btab_index(a.views[v], j, b)];
  }
  a.btd[e] = out;
  if (b == 0) a.colview[j] = (uint8_t)(v < 0 ? 255 : v);
}

// dense quadratic weights from ranges: wq[k, i] += p * w[g, k] for i in range g   (GroupRegularizer / L2Regularizer)
__global__ void k_expand_group(float *wq, int Kp, int K, int64_t n, const int64_t *s1, const int64_t *e1,
                               const float *w, int n_groups, float p) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n * Kp) return;
  const int k = (int)(e % Kp);
  const int64_t i = e / Kp;
  if (k >= K) return;
  float add = 0.f;
  for (int g = 0; g < n_groups; ++g)
    if (i + 1 >= s1[g] && i + 1 <= e1[g]) add += w[(int64_t)g * K + k];
  wq[e] += p * add;
}
// same for a 1-D parameter (ColParamReg): per range weight and centre
__global__ void k_expand_colparam(float *wq, float *cq, int64_t n, const int64_t *s1, const int64_t *e1,
                                  const float *w, const float *c, int n_ranges) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= n) return;
  float ww = 0.f, cc = 0.f;
  for (int r = 0; r < n_ranges; ++r)
    if (j + 1 >= s1[r] && j + 1 <= e1[r]) { ww = w[r]; cc = c[r]; }
  wq[j] = ww;
  cq[j] = cc;
}
// BatchArrayReg: per (view, batch) weight and centre broadcast over the view's columns
__global__ void k_expand_batchreg(float *wq, float *cq, int64_t n, const int32_t *val_view, const int64_t *val_off,
                                  const int32_t *nbs, const int64_t *bvb_off, const float *w, const float *c) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int v = val_view[e];
  const int b = (int)((e - val_off[v]) % nbs[v]);
  wq[e] = w[bvb_off[v] + b];
  cq[e] = c[bvb_off[v] + b];
}
// ARDRegularizer ranges -> dense alpha[N], beta[Kp x N]
__global__ void k_expand_ard(float *alpha, float *beta, int Kp, int64_t N, const int64_t *s1, const int64_t *e1,
                             const float *a, const float *b, int n_ranges) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= N * Kp) return;
  const int64_t j = e / Kp;
  float aa = 0.f, bb = 1.f;
  bool hit = false;
  for (int r = 0; r < n_ranges; ++r)
    if (j + 1 >= s1[r] && j + 1 <= e1[r]) { aa = a[r]; bb = b[r]; hit = true; }
  // columns outside every range are not regularized: encode as alpha = -0.5 (factor (0.5+alpha) = 0), beta = 1
  if (!hit) { aa = -0.5f; bb = 1.f; }
  beta[e] = bb;
  if (e % Kp == 0) alpha[j] = aa;
}
__global__ void k_pad_copy(float *dst, const float *src, int Kp, int K, int64_t n, float padval) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n * Kp) return;
  const int k = (int)(e % Kp);
  dst[e] = k < K ? src[(e / Kp) * K + k] : padval;
}

// column-major source block (rows 0..M-1, columns col0..col0+ncols-1, leading dimension M) -> tile-major D
// (bf16 storage: the cast is one v_cvt_pk_bf16_f32 under the kernel's default mode: round to nearest even, f32 subnormals
// kept, every NaN stays NaN whatever its payload; held to that by tests/test_gpu_data_ingest.py)
__global__ void k_tile_D(const float *src, int64_t M, int64_t col0, int64_t ncols, void *dst, int64_t nRB, int bf16) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= M * ncols) return;
  const int64_t i = e % M, jl = e / M;
  if (bf16) reinterpret_cast<__bf16 *>(dst)[pmf_d_off16(i, col0 + jl, nRB)] = (__bf16)src[e];
  else reinterpret_cast<float *>(dst)[pmf_d_off(i, col0 + jl, nRB)] = src[e];
}
__global__ void k_fill16(uint16_t *p, int64_t n, uint16_t v) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) p[e] = v;
}
// one entry of the tile-major data matrix, whatever its storage type (the rarely-run scalar kernels)
__device__ __forceinline__ float pmf_d_get(const void *D, int64_t i, int64_t j, int64_t nRB, int bf16) {
  if (bf16) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(D)[pmf_d_off16(i, j, nRB)] << 16);
  return reinterpret_cast<const float *>(D)[pmf_d_off(i, j, nRB)];
}

struct StepArgsGraph : StepArgs {   // k_reg_step<true>: the same, plus the pathway-graph terms (at least one of them set)
  const float *gpre;             // gradient of a term evaluated beforehand (NetworkRegularizer, pmf_netreg.hip; may be null)
  const float *wl1;              // dense L1 weights (L1Regularizer / SelectiveL1Reg; may be null)
};

// Regularizer gradient + optimizer step, one pass over a parameter tensor.
//   quadratic : 0.5*wq*(p-cq)^2  (L2Regularizer regularizers.jl:21-33, GroupRegularizer :423-446,
//               ColParamReg :482-487, BatchArrayReg :795-815)
//   ARD       : (0.5+alpha_j) log(1 + (0.5/beta) p^2), grad (alpha_j+0.5) p / (b beta)
//               (ARDRegularizer :546-585, FeatureSetARDReg featureset_ard.jl:135-150)
//   network   : gradient read from `gpre`, loss partials written by k_netreg_grad (NetworkRegularizer :249-306)
//   L1        : wl1 |p|, grad wl1 sign(p), sign(0) = 0  (L1Regularizer :71-82, SelectiveL1Reg :130-146)
//   AdaGrad   : acc += g^2 ; p -= eta g/(sqrt(acc)+eps)   (optimizers.jl:6-13 ; acc starts at eps)
//   Adam      : Flux.Optimise.Adam
// GRAPH: the instance with the pathway-graph terms (network, L1), launched only when one of them is set.  The plain
// instance neither takes nor tests them: a context without these terms runs the arguments and the code it always ran.
template <bool GRAPH>
__global__ __launch_bounds__(256) void k_reg_step(const std::conditional_t<GRAPH, StepArgsGraph, StepArgs> a) {
  __shared__ double sh[4];
  double lacc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < a.n; e += stride) {
    const int k = (int)(e % a.Kp);
    if (k >= a.K) continue;
    float p = a.p[e];
    float g = a.g[e];
    if (a.use_reg) {
      if (a.wq) pmf_reg_quad(p, a.wq[e], a.cq ? a.cq[e] : 0.f, g, lacc);
      if (a.ard_beta) pmf_reg_ard(p, a.ard_beta[e], a.ard_alpha[e / a.Kp], a.ard_scale, g, lacc);
      if constexpr (GRAPH) {
        if (a.gpre) g += a.gpre[e];
        if (a.wl1) {
          const float w = a.wl1[e];
          lacc += (double)(w * fabsf(p));
          g += p > 0.f ? w : p < 0.f ? -w : 0.f;
        }
      }
    }
    if (a.do_step) {
      if (a.opt_kind == PMF_OPT_ADAGRAD) {
        const float acc = a.acc[e] + g * g;
        a.acc[e] = acc;
        p -= g * (a.lr / (sqrtf(acc) + a.eps));
      } else {
        const float m = a.b1 * a.mom[e] + (1.f - a.b1) * g;
        const float v = a.b2 * a.acc[e] + (1.f - a.b2) * g * g;
        a.mom[e] = m;
        a.acc[e] = v;
        p -= m / a.c1 / (sqrtf(v / a.c2) + a.eps) * a.lr;
      }
      a.p[e] = p;
    }
  }
  const double s = block_reduce_sum(lacc, sh);
  if (threadIdx.x == 0 && a.reg_partial) a.reg_partial[blockIdx.x] = s;
}

// fixed-order reduction of the loss partial slabs -> out[0..4]
__global__ __launch_bounds__(256) void k_loss_reduce(const double *data_partial, int64_t n_data, const double *reg_partial,
                                                     const RegCounts reg_counts, double *out, int mask) {
  __shared__ double sh[4];
  for (int which = 0; which < 5; ++which) {
    if (!((mask >> which) & 1)) continue;   // (uniform) the pipelined loop of pmf_fit reduces the rank-local and the replicated terms separately
    const double *src = which == 0 ? data_partial : reg_partial + (int64_t)(which - 1) * REG_SLOTS;
    const int64_t n = which == 0 ? n_data : reg_counts.c[which - 1];
    double v = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += blockDim.x) v += src[e];
    const double s = block_reduce_sum(v, sh);
    if (threadIdx.x == 0) out[which] = s;
    __syncthreads();
  }
}
int launch_loss_reduce(pmf_ctx *c, const RegCounts &rc, int mask) {
  k_loss_reduce<<<1, 256, 0, c->stream>>>(c->loss_partial, c->n_macro, c->reg_partial, rc, c->d_loss, mask);
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the column walk k_layer_grad<KB> and k_stats<KB> share.  One wave per workgroup: thread = column (64 consecutive
// columns), sequential over a chunk of rows.  The column of Y lives in registers (32*KB floats), four rows of X at a time are
// staged in LDS and read back as broadcast 16-B reads (a single wave needs no barrier: LDS operations of one wave complete
// in order), per-(batch, column) sums in LDS (no contention: a thread only touches its own column), one plain store per
// (batch, column) per workgroup at the end (private partials per block row, added in fixed order by k_sum_parts).
struct ColWalkArgs {
  const void *D;
  int d_bf16;
  const float *X, *Y;
  const float4 *colp;
  const float *htab;    // per column table of class bounds of the kind-3 columns (pmf_hinge_terms)
  const int32_t *bor;
  const float2 *btab;
  int64_t M, N, nRB;
  int Kp, K, rows_per_block, max_nb;
  ViewDesc views[PMF_MAXV];
  int64_t val_off[PMF_MAXV];
};
#define PMF_WALK_RG 4   // rows of X per group
// dynamic LDS: [RG][Kp] current rows of X | [2][max_nb][64] per-(batch, column) sums
__host__ __device__ constexpr size_t col_walk_lds(int Kp, int max_nb) { return sizeof(float) * (size_t)(PMF_WALK_RG * Kp + 2 * max_nb * 64); }

template <int KB>
struct ColWalk {
  static constexpr int Kp = 32 * KB, RG = PMF_WALK_RG;
  const ColWalkArgs &a;
  float *xs, *bacc;
  int tid;
  int64_t j, jc, r0, r1;   // column, column clamped to the matrix, row range of this block row
  bool col_ok;
  float4 cp;        // column parameters of column jc
  const float *ht;  // its table of class bounds (kind 3)
  int kind, v;
  ViewDesc vd;
  float4 yr[Kp / 4];

  __device__ __forceinline__ ColWalk(const ColWalkArgs &a_, char *smem) : a(a_) {
    xs = reinterpret_cast<float *>(smem);
    bacc = xs + RG * Kp;
    tid = threadIdx.x;
    j = blockIdx.x * 64 + tid;
    col_ok = j < a.N;
    jc = col_ok ? j : a.N - 1;
    r0 = (int64_t)blockIdx.y * a.rows_per_block;
    r1 = r0 + a.rows_per_block;
    if (r1 > a.M) r1 = a.M;
    cp = a.colp[jc];
    ht = a.htab + jc * PMF_HT;
    const int meta = __float_as_int(cp.w);
    kind = pmf_meta_kind(meta);
    v = pmf_meta_view(meta);
    vd = a.views[v >= 0 ? v : 0];
    for (int e = tid; e < 2 * a.max_nb * 64; e += 64) bacc[e] = 0.f;
    const float4 *y4 = reinterpret_cast<const float4 *>(a.Y + jc * Kp);
#pragma unroll
    for (int q = 0; q < Kp / 4; ++q) yr[q] = y4[q];
  }
  // stage RG rows of X (contiguous in memory: X is Kp x M column-major); rows past the chunk are clamped
  __device__ __forceinline__ void stage_x(int64_t ib) const {
    __builtin_amdgcn_wave_barrier();
    for (int e4 = tid; e4 < RG * Kp / 4; e4 += 64) {
      const int rr = (e4 * 4) / Kp;
      const int64_t i = ib + rr < r1 ? ib + rr : r1 - 1;
      reinterpret_cast<float4 *>(xs)[e4] = reinterpret_cast<const float4 *>(a.X + i * Kp)[(e4 * 4 % Kp) / 4];
    }
    __builtin_amdgcn_wave_barrier();
  }
  // x_i . y_j of staged row rr
  __device__ __forceinline__ float dot(int rr) const {
    const float4 *x4 = reinterpret_cast<const float4 *>(xs + rr * Kp);
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int q = 0; q < Kp / 4; ++q) {
      const float4 xv = x4[q];
      acc0 = fmaf(xv.x, yr[q].x, acc0);
      acc1 = fmaf(xv.y, yr[q].y, acc1);
      acc0 = fmaf(xv.z, yr[q].z, acc0);
      acc1 = fmaf(xv.w, yr[q].w, acc1);
    }
    return acc0 + acc1;
  }
  __device__ __forceinline__ int batch(int64_t i) const { return pmf_row_batch(a.bor, a.M, v, i); }
  __device__ __forceinline__ float2 batch_dt(int b) const { return pmf_batch_dt(vd, a.btab, jc, b); }
  __device__ __forceinline__ float data(int64_t i) const { return pmf_d_get(a.D, i, jc, a.nRB, a.d_bf16); }
  __device__ __forceinline__ float &sum(int which, int b) const { return bacc[(which * a.max_nb + b) * 64 + tid]; }   // which = 0, 1
  __device__ __forceinline__ int64_t val_index(int b) const { return a.val_off[v] + pmf_view_index(vd, j, b); }   // in logdelta / theta
};

// ------------------------------------------------------------------------------------------------
// Layer-parameter gradient pass (update_col_layers stages S2/S7: init_theta! fit.jl:106-122, fit_joint :987-1000).
// Pull-backs as coded in the reference:
//   theta_bar[b,j]    = sum_{i in b} g                      (batch_array.jl:141-143)
//   mu_bar[j]         = sum_i g                             (layers.jl:83)
//   logdelta_bar[b,j] = delta[b,j] * sum_{i in b} g * (a*sigma_j)   (batch_array.jl:203-204, 250)
//   logsigma_bar[j]   = sigma_j * sum_i g * delta           (layers.jl:40-41; Q1: omits the input factor)
// ------------------------------------------------------------------------------------------------
struct LayerGradArgs : ColWalkArgs {
  float *g_logsigma, *g_mu, *g_logdelta, *g_theta;  // any may be null (only nullness is used by the kernel: see part)
  // per block row (blockIdx.y) one private vector [mu N][logsigma N][theta nbt][logdelta nbt] of part_stride floats, every entry
  // written by exactly one thread; k_sum_parts adds the block rows in fixed order (no float atomics: bitwise reproducible)
  float *part;
  int64_t part_stride, nbt;
  double *loss_partial;                             // may be null; one slot per block (flattened grid)
};

// out[e] = sum over p = 0 .. n_parts-1, in that order, of part[p * stride + e]
__global__ __launch_bounds__(256) void k_sum_parts(const float *__restrict__ part, int64_t stride, int n_parts, float *__restrict__ out, int64_t n) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  float t = 0.f;
  for (int p = 0; p < n_parts; ++p) t += part[(int64_t)p * stride + e];
  out[e] = t;
}
static int sum_parts(pmf_ctx *c, const float *part, int64_t stride, int n_parts, float *out, int64_t n) {
  if (!out || n <= 0) return 0;
  k_sum_parts<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(part, stride, n_parts, out, n);
  HIPCHK(hipGetLastError());
  return 0;
}

template <int KB>
__global__ __launch_bounds__(64) void k_layer_grad(const LayerGradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_lg[];
  __shared__ double sh[4];
  ColWalk<KB> w(a, smem_lg);
  const int kind = w.kind;   // (pad columns walk the last column again; zeroed below)
  const float4 cp = w.cp;
  float smu = 0.f, sls = 0.f;
  double lacc = 0.0;
  for (int64_t ib = w.r0; ib < w.r1; ib += w.RG) {
    w.stage_x(ib);
#pragma unroll
    for (int rr = 0; rr < w.RG; ++rr) {
      const int64_t i = ib + rr;
      if (i >= w.r1) break;
      const float acc = w.dot(rr);
      const int b = w.batch(i);
      const float2 dt = w.batch_dt(b);
      const float yv = w.data(i);
      const float z1 = acc * cp.x;
      const float z = fmaf(z1, dt.x, cp.y + dt.y);
      float l, g;
      pmf_noise(kind, z, yv, cp.z, w.ht, l, g);
      const bool ok = w.col_ok && pmf_finite(yv);
      if (!ok) { l = 0.f; g = 0.f; }
      lacc += (double)l;
      smu += g;
      sls += g * dt.x;
      if (b >= 0) {
        w.sum(0, b) += g;
        w.sum(1, b) += g * z1;
      }
    }
  }
  if (w.col_ok) {
    float *pp = a.part + (int64_t)blockIdx.y * a.part_stride;
    if (a.g_mu) pp[w.j] = smu;
    if (a.g_logsigma) pp[a.N + w.j] = sls * cp.x;
    if (w.v >= 0) {
      for (int b = 0; b < w.vd.nb; ++b) {
        const int64_t e = w.val_index(b);
        if (a.g_theta) pp[2 * a.N + e] = w.sum(0, b);
        if (a.g_logdelta) pp[2 * a.N + a.nbt + e] = w.sum(1, b) * a.btab[pmf_btab_index(w.vd, w.j, b)].x;
      }
    }
  }
  const double s = block_reduce_sum(lacc, sh);
  if (w.tid == 0 && a.loss_partial) a.loss_partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// Column and batch statistics.  Called a handful of times per fit, not per epoch.
// ------------------------------------------------------------------------------------------------
struct StatsArgs : ColWalkArgs {
  float *col_n, *col_sum, *col_sumsq, *col_sqerr, *col_ssqg;  // N each: block row 0's vector of the PRIVATE partials -- block row y
  float *b_n, *b_sqerr;                                       // writes at + y * part_stride; flat like theta (may be null)
  int64_t part_stride;                                        // k_sum_parts adds the block rows in fixed order (no float atomics)
  int use_factors;                                            // 0: the prediction without the factor term (no staging, no product)
};

template <int KB>
__global__ __launch_bounds__(64) void k_stats(const StatsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_st[];
  ColWalk<KB> w(a, smem_st);
  const float4 cp = w.cp;
  float sn = 0.f, s1 = 0.f, s2 = 0.f, se = 0.f, sg = 0.f;
  for (int64_t ib = w.r0; ib < w.r1; ib += w.RG) {
    if (a.use_factors) w.stage_x(ib);
#pragma unroll
    for (int rr = 0; rr < w.RG; ++rr) {
      const int64_t i = ib + rr;
      if (i >= w.r1) break;
      float acc = 0.f;
      if (a.use_factors) acc = w.dot(rr);
      const int b = w.batch(i);
      const float2 dt = w.batch_dt(b);
      const float yv = w.data(i);
      if (!pmf_finite(yv)) continue;
      const float z = fmaf(acc * cp.x, dt.x, cp.y + dt.y);
      float r;   // residual: prediction - y; squared hinge: the signed margin violation b - a (= g / w, as z - y is for a normal column)
      if (w.kind == PMF_NOISE_NORMAL) r = z - yv;
      else if (w.kind == PMF_NOISE_BERNOULLI) r = 1.f / (1.f + __expf(-z)) - yv;
      else if (w.kind == PMF_NOISE_POISSON) r = __expf(z) - yv;
      else {
        float ha, hb;
        pmf_hinge_terms(z, yv, w.ht, ha, hb);
        r = hb - ha;
      }
      const float g = cp.z * r;
      sn += 1.f; s1 += yv; s2 += yv * yv; se += r * r; sg += g * g;
      if (b >= 0) {
        w.sum(0, b) += 1.f;
        w.sum(1, b) += r * r;
      }
    }
  }
  if (w.col_ok) {
    const int64_t po = (int64_t)blockIdx.y * a.part_stride, j = w.j;
    if (a.col_n) a.col_n[po + j] = sn;
    if (a.col_sum) a.col_sum[po + j] = s1;
    if (a.col_sumsq) a.col_sumsq[po + j] = s2;
    if (a.col_sqerr) a.col_sqerr[po + j] = se;
    if (a.col_ssqg) a.col_ssqg[po + j] = sg;
    if (w.v >= 0 && a.b_n) {
      for (int b = 0; b < w.vd.nb; ++b) {
        const int64_t e = w.val_index(b);
        a.b_n[po + e] = w.sum(0, b);
        a.b_sqerr[po + e] = w.sum(1, b);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side helpers
// ------------------------------------------------------------------------------------------------
int upload_padded(pmf_ctx *c, float *dst, const float *src, int64_t n, float padval) {
  // src: host K x n ; dst: device Kp x n
  if (c->K == c->Kp) {
    HIPCHK(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)(n * c->K), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
  }
  PMFCHK(c->scratch.ensure(sizeof(float) * (size_t)(n * c->K), false));
  HIPCHK(hipMemcpyAsync(c->scratch, src, sizeof(float) * (size_t)(n * c->K), hipMemcpyHostToDevice, c->stream));
  k_pad_copy<<<nblocks(n * c->Kp, 256), 256, 0, c->stream>>>(dst, (const float *)c->scratch.p, c->Kp, c->K, n, padval);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
int download_padded(pmf_ctx *c, float *dst_host, const float *src_dev, int64_t n) {
  HIPCHK(hipMemcpy2DAsync(dst_host, sizeof(float) * c->K, src_dev, sizeof(float) * c->Kp, sizeof(float) * c->K,
                          (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// what set_K resets with the factors: the ARD-type term of Y; what data_shape_changed resets with the shape: everything
// built from the batch views
static void drop_ard(pmf_ctx *c) {
  c->ard_alpha.free();
  c->ard_beta.free();
  c->has_ard = false;
  c->ard_is_fsard = false;
}
static void drop_views(pmf_ctx *c) {
  c->bor.free(); c->btab.free(); c->d_val_view.free(); c->d_views.free();   // the views as uploaded
  c->btd.free(); c->colview.free();                                         // the dense table prepare() builds from them
  c->LG.free(); c->lgrad_part.free();                                       // the layer pass's tables, sized by them
  c->btd_ok = false;
  c->views_dirty = true;
}

static int set_K(pmf_ctx *c, int K) {
  if (K <= 0 || K > 128) return pmf_fail("K=%d unsupported (1..128)", K);
  if (c->M <= 0 || c->N <= 0) return pmf_fail("pmf_set_data must be called before pmf_set_factors");
  if (K == c->K && c->P[0].n == (int64_t)c->Kp * c->M && c->P[1].n == (int64_t)c->Kp * c->N) return 0;
  c->K = K;
  c->KB = (K + 31) / 32;
  c->Kp = 32 * c->KB;
  PMFCHK(param_alloc(c->P[0], (int64_t)c->Kp * c->M));
  PMFCHK(param_alloc(c->P[1], (int64_t)c->Kp * c->N));
  netreg_free(c, 0);
  netreg_free(c, 1);
  drop_ard(c);
  c->state_init = false;
  return 0;
}

extern "C" int pmf_device_count(int *n) {
  if (!n) return pmf_fail("null output");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  *n = ndev;
  return 0;
}

extern "C" int pmf_create(int device, pmf_ctx **out) {
  if (!out) return pmf_fail("null out");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return pmf_fail("device %d out of range (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return pmf_fail("libpmf_hip is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
  std::unique_ptr<pmf_ctx> c(new pmf_ctx());   // (a failure below frees the context and what it owns)
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->own_stream = true;
  if (c->d_loss.alloc(8, false) < 0 || c->h_loss.alloc(8, false) < 0 || c->reg_partial.alloc(4 * REG_SLOTS, true) < 0) {
    (void)hipStreamDestroy(c->stream);
    return -1;
  }
  {
    const char *pe = getenv("PMF_PRECISION");   // development / benchmark override of the default (exact f32)
    if (pe && std::string(pe) == "bf16x3") c->precision = PMF_PREC_BF16X3;
  }
  *out = c.release();
  return 0;
}

extern "C" int pmf_destroy(pmf_ctx *c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  // what is not memory: the communicator with its stream and events, the context's events and stream; every buffer goes
  // with its owner in `delete c`
  comm_release(c);
  netreg_free(c, 0);
  netreg_free(c, 1);
  lbfgs_free(c);
  if (c->ev_host) (void)hipEventDestroy(c->ev_host);
  for (auto &e : c->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

extern "C" int pmf_set_precision(pmf_ctx *c, int mode) {
  if (!c) return pmf_fail("null context");
  if (mode != PMF_PREC_F32 && mode != PMF_PREC_BF16X3) return pmf_fail("unknown precision mode %d", mode);
  c->precision = mode;
  return 0;
}

extern "C" int pmf_get_precision(pmf_ctx *c, int *mode, int64_t *split_launches) {
  if (!c) return pmf_fail("null context");
  if (mode) *mode = c->precision;
  if (split_launches) *split_launches = c->sb_launches;
  return 0;
}

extern "C" int pmf_set_stream(pmf_ctx *c, void *s) {
  PMFCHK(ctx_bind(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (s == nullptr) {
    if (!c->own_stream) {
      HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
      c->own_stream = true;
    }
    return 0;
  }
  if (c->own_stream && c->stream) HIPCHK(hipStreamDestroy(c->stream));
  c->stream = (hipStream_t)s;
  c->own_stream = false;
  return 0;
}
extern "C" int pmf_synchronize(pmf_ctx *c) {
  PMFCHK(ctx_bind(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

static int data_shape_changed(pmf_ctx *c, int64_t M, int64_t N) {
  if (M <= 0 || N <= 0) return pmf_fail("empty data matrix (%lld x %lld)", (long long)M, (long long)N);
  if (M == c->M && N == c->N) return 0;
  c->M = M;
  c->N = N;
  for (auto &b : c->P) b = ParamBuf();
  netreg_free(c, 0);
  netreg_free(c, 1);
  c->K = c->Kp = c->KB = 0;
  PMFCHK(param_alloc(c->P[2], N));
  PMFCHK(param_alloc(c->P[3], N));
  c->n_bv = 0;
  c->h_bor.clear();
  c->views_serial++;
  c->views.clear();
  c->val_off.clear();
  c->bvb_off.clear();
  drop_views(c);
  PMFCHK(c->colmeta.alloc((size_t)N, true));
  PMFCHK(c->colw.alloc((size_t)N, true));
  PMFCHK(c->colp.alloc((size_t)N, true));
  c->thr.free();     // (allocated by the first noise model that is not all-normal: upload_thresholds)
  c->htab.free();
  c->h_thr.clear();
  k_fill<<<nblocks(N, 256), 256, 0, c->stream>>>(c->colw, N, 1.f);
  HIPCHK(hipGetLastError());
  c->mixed = false;
  c->noise_s1.clear();   // (the noise model is reset with the shape: its ranges indexed the old columns)
  c->noise_e1.clear();
  c->prepared = false;
  c->state_init = false;
  return 0;
}

// The device copy of D is tile-major (pmf_d_off): nRB = ceil(M/32) row blocks x ceil(N/64)*2 column blocks of
// 32 x 32 floats, NaN-filled outside the matrix.
static int alloc_tiled_D(pmf_ctx *c, int64_t M, int64_t N, int store) {
  const int64_t Npad = (N + PMF_DPAD - 1) / PMF_DPAD * PMF_DPAD;
  const int64_t nRB = (M + 31) / 32;
  const int64_t nfl = nRB * 32 * Npad;
  const size_t esz = store == PMF_STORE_BF16 ? 2 : 4;
  if (!(c->D && c->D_M == M && c->D_Npad == Npad && c->store == store)) {   // same shape and store: keep the buffer
    PMFCHK(c->D.alloc(esz * (size_t)nfl, false));
    c->own_D = true;
    c->D_M = M;
    c->D_Npad = Npad;
    c->nRB = nRB;
  }
  c->tflags_valid = false;
  holdout_drop(c);   // a hold-out set belonged to the old values: it goes without write-back (pmf_hip_holdout.h)
  c->store = store;
  if (store == PMF_STORE_BF16) k_fill16<<<(int)std::min<int64_t>(nblocks(nfl, 256), 65536), 256, 0, c->stream>>>((uint16_t *)c->D.p, nfl, (uint16_t)0x7fc0);
  else k_fill<<<(int)std::min<int64_t>(nblocks(nfl, 256), 65536), 256, 0, c->stream>>>((float *)c->D.p, nfl, __builtin_nanf(""));
  HIPCHK(hipGetLastError());
  return 0;
}

static int tile_from_device(pmf_ctx *c, const float *src, int64_t col0, int64_t ncols) {
  const int64_t n = c->M * ncols;
  c->tflags_valid = false;
  k_tile_D<<<nblocks(n, 256), 256, 0, c->stream>>>(src, c->M, col0, ncols, c->D, c->nRB, c->store == PMF_STORE_BF16);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmf_set_data(pmf_ctx *c, const float *D, int64_t M, int64_t N, int store) {
  PMFCHK(ctx_bind(c));
  if (!D) return pmf_fail("null data pointer");
  if (store != PMF_STORE_F32 && store != PMF_STORE_BF16) return pmf_fail("unknown storage type %d", store);
  PMFCHK(data_shape_changed(c, M, N));
  PMFCHK(alloc_tiled_D(c, M, N, store));
  // upload in column chunks of <= 256 MiB (one column where a column alone is longer) through a staging buffer, tiling
  // each chunk on the device
  int64_t chunk_floats = 64ll << 20;
  const char *ce = getenv("PMF_SET_DATA_CHUNK_FLOATS");   // test hook, read at every call: small shapes upload in several chunks
  if (ce && atoll(ce) > 0) chunk_floats = atoll(ce);
  const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(N, chunk_floats / std::max<int64_t>(M, 1)));
  PMFCHK(c->scratch.ensure(sizeof(float) * (size_t)(M * chunk), false));
  for (int64_t c0 = 0; c0 < N; c0 += chunk) {
    const int64_t nc = std::min(chunk, N - c0);
    HIPCHK(hipMemcpyAsync(c->scratch, D + c0 * M, sizeof(float) * (size_t)(M * nc), hipMemcpyHostToDevice, c->stream));
    PMFCHK(tile_from_device(c, (const float *)c->scratch.p, c0, nc));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}
extern "C" int pmf_set_data_device(pmf_ctx *c, const void *D, int64_t M, int64_t N, int store) {
  PMFCHK(ctx_bind(c));
  if (store != PMF_STORE_F32 && store != PMF_STORE_BF16) return pmf_fail("unknown storage type %d", store);
  PMFCHK(data_shape_changed(c, M, N));
  PMFCHK(alloc_tiled_D(c, M, N, store));      // D == NULL: left all-NaN for pmf_synth_data
  if (D) PMFCHK(tile_from_device(c, (const float *)D, 0, N));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pmf_set_factors(pmf_ctx *c, const float *X, const float *Y, int K) {
  PMFCHK(ctx_bind(c));
  if (!X || !Y) return pmf_fail("null factor pointer");
  PMFCHK(set_K(c, K));
  PMFCHK(upload_padded(c, c->P[0].p, X, c->M, 0.f));
  PMFCHK(upload_padded(c, c->P[1].p, Y, c->N, 0.f));
  return 0;
}
extern "C" int pmf_set_X(pmf_ctx *c, const float *X, int K) {
  PMFCHK(ctx_bind(c));
  if (K != c->K) return pmf_fail("pmf_set_X: K=%d differs from the current K=%d (use pmf_set_factors)", K, c->K);
  return upload_padded(c, c->P[0].p, X, c->M, 0.f);
}
extern "C" int pmf_set_Y(pmf_ctx *c, const float *Y, int K) {
  PMFCHK(ctx_bind(c));
  if (K != c->K) return pmf_fail("pmf_set_Y: K=%d differs from the current K=%d (use pmf_set_factors)", K, c->K);
  return upload_padded(c, c->P[1].p, Y, c->N, 0.f);
}
extern "C" int pmf_get_factors(pmf_ctx *c, float *X, float *Y) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0) return pmf_fail("factors not set");
  if (X) PMFCHK(download_padded(c, X, c->P[0].p, c->M));
  if (Y) PMFCHK(download_padded(c, Y, c->P[1].p, c->N));
  return 0;
}

extern "C" int pmf_set_col_params(pmf_ctx *c, const float *logsigma, const float *mu) {
  PMFCHK(ctx_bind(c));
  if (c->N == 0) return pmf_fail("data not set");
  if (logsigma) PMFCHK(upload_vec(c, c->P[2].p, logsigma, (size_t)c->N));
  if (mu) PMFCHK(upload_vec(c, c->P[3].p, mu, (size_t)c->N));
  c->prepared = false;
  return 0;
}
extern "C" int pmf_get_col_params(pmf_ctx *c, float *logsigma, float *mu) {
  PMFCHK(ctx_bind(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (logsigma) HIPCHK(hipMemcpy(logsigma, c->P[2].p, sizeof(float) * (size_t)c->N, hipMemcpyDeviceToHost));
  if (mu) HIPCHK(hipMemcpy(mu, c->P[3].p, sizeof(float) * (size_t)c->N, hipMemcpyDeviceToHost));
  return 0;
}

// ---- batch views -------------------------------------------------------------------------------
static int rebuild_colmeta_views(pmf_ctx *c) {
  // refresh the view id bits of colmeta from the current views (kind bits are kept)
  std::vector<int32_t> meta((size_t)c->N);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(meta.data(), c->colmeta, sizeof(int32_t) * (size_t)c->N, hipMemcpyDeviceToHost));
  for (auto &m : meta) m &= 3;
  for (int v = 0; v < c->n_bv; ++v) {
    const ViewDesc &vd = c->views[v];
    if (vd.nb <= 0) continue;
    for (int64_t j = vd.c0; j < vd.c1; ++j) meta[(size_t)j] |= (v + 1) << 2;
  }
  HIPCHK(hipMemcpy(c->colmeta, meta.data(), sizeof(int32_t) * (size_t)c->N, hipMemcpyHostToDevice));
  c->prepared = false;
  return 0;
}

extern "C" int pmf_set_n_batch_views(pmf_ctx *c, int n) {
  PMFCHK(ctx_bind(c));
  if (n < 0 || n > PMF_MAXV) return pmf_fail("n_batch_views=%d out of range (0..%d)", n, PMF_MAXV);
  if (c->N == 0) return pmf_fail("data not set");
  // Same number of views as before: keep the views, their values and -- above all -- the optimizer state.  Both hosts
  // re-marshal the model before every MF.fit! call, and mf_fit_adapt_lr! (src/fit.jl:55-69) resumes with the SAME
  // AdaGrad object after halving eta: its accumulators must survive.  pmf_set_batch_view replaces what changed.
  if (n == c->n_bv && (int)c->views.size() == n && (n == 0 || c->bor)) return 0;
  c->n_bv = n;
  c->h_bor.assign((size_t)n, std::vector<int32_t>());
  c->views_serial++;
  c->views.assign((size_t)n, ViewDesc{0, 0, 0, 0, 0});
  c->views_dirty = true;
  c->val_off.assign((size_t)n + 1, 0);
  c->bvb_off.assign((size_t)n + 1, 0);
  c->P[4] = ParamBuf();
  c->P[5] = ParamBuf();
  c->btab.free();
  c->d_val_view.free();
  PMFCHK(c->bor.alloc((size_t)((int64_t)n * c->M), true));
  if (n > 0) PMFCHK(memset_now(c->bor, 0xFF, sizeof(int32_t) * (size_t)((int64_t)n * c->M)));
  PMFCHK(rebuild_colmeta_views(c));
  c->state_init = false;
  return 0;
}

extern "C" int pmf_set_batch_view(pmf_ctx *c, int v, int64_t s1, int64_t e1, int nb, const int32_t *batch_of_row,
                                  const float *logdelta, const float *theta) {
  PMFCHK(ctx_bind(c));
  if (v < 0 || v >= c->n_bv) return pmf_fail("batch view %d out of range (n=%d)", v, c->n_bv);
  if (s1 < 1 || e1 > c->N || s1 > e1) return pmf_fail("batch view %d: bad column range %lld:%lld", v, (long long)s1, (long long)e1);
  if (nb <= 0) return pmf_fail("batch view %d: nb=%d", v, nb);
  if (v > 0 && c->views[v - 1].nb == 0) return pmf_fail("batch views must be set in order (view %d is unset)", v - 1);
  if (v > 0 && s1 - 1 < c->views[v - 1].c1) return pmf_fail("batch view %d overlaps / precedes view %d", v, v - 1);
  const int64_t Nv = e1 - s1 + 1;
  for (int64_t i = 0; i < c->M; ++i)
    if (batch_of_row[i] < -1 || batch_of_row[i] >= nb) return pmf_fail("batch view %d: batch_of_row[%lld]=%d out of range", v, (long long)i, batch_of_row[i]);
  const bool same_shape = c->views[v].nb == nb && c->views[v].c0 == s1 - 1 && c->views[v].c1 == e1 && c->P[4].n > 0 &&
                          c->val_off[v + 1] - c->val_off[v] == Nv * nb;
  c->views[v].c0 = s1 - 1;
  c->views[v].c1 = e1;
  c->views[v].nb = nb;
  c->views_dirty = true;
  HIPCHK(hipMemcpy(c->bor + (int64_t)v * c->M, batch_of_row, sizeof(int32_t) * (size_t)c->M, hipMemcpyHostToDevice));
  if ((int)c->h_bor.size() < c->n_bv) c->h_bor.resize((size_t)c->n_bv);
  if (c->h_bor[(size_t)v].size() != (size_t)c->M || memcmp(c->h_bor[(size_t)v].data(), batch_of_row, sizeof(int32_t) * (size_t)c->M) != 0) {
    c->h_bor[(size_t)v].assign(batch_of_row, batch_of_row + c->M);
    c->views_serial++;
  }
  if (!same_shape) {
    // (re)compute offsets for views >= v and reallocate the flat arrays once the last view is known
    for (int u = v; u < c->n_bv; ++u) {
      const int64_t sz = c->views[u].nb > 0 ? (c->views[u].c1 - c->views[u].c0) * c->views[u].nb : 0;
      c->val_off[u + 1] = c->val_off[u] + sz;
      c->bvb_off[u + 1] = c->bvb_off[u] + c->views[u].nb;
      c->views[u].tab_off = c->val_off[u];
    }
    const int64_t tot = c->val_off[c->n_bv];
    // keep already uploaded values of earlier views
    std::vector<float> old_ld, old_th;
    const int64_t keep = c->val_off[v];
    if (c->P[4].n >= keep && keep > 0) {
      old_ld.resize((size_t)keep);
      old_th.resize((size_t)keep);
      HIPCHK(hipMemcpy(old_ld.data(), c->P[4].p, sizeof(float) * (size_t)keep, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(old_th.data(), c->P[5].p, sizeof(float) * (size_t)keep, hipMemcpyDeviceToHost));
    }
    PMFCHK(param_alloc(c->P[4], tot));
    PMFCHK(param_alloc(c->P[5], tot));
    if (!old_ld.empty()) {
      HIPCHK(hipMemcpy(c->P[4].p, old_ld.data(), sizeof(float) * old_ld.size(), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(c->P[5].p, old_th.data(), sizeof(float) * old_th.size(), hipMemcpyHostToDevice));
    }
    PMFCHK(c->btab.alloc((size_t)tot, true));
    std::vector<int32_t> vv((size_t)std::max<int64_t>(1, tot), 0);
    for (int u = 0; u < c->n_bv; ++u)
      for (int64_t e = c->val_off[u]; e < c->val_off[u + 1]; ++e) vv[(size_t)e] = u;
    PMFCHK(c->d_val_view.alloc(vv.size(), true));
    PMFCHK(c->d_val_view.upload(vv.data(), vv.size()));
    c->state_init = false;
  }
  const int64_t off = c->val_off[v];
  if (logdelta) HIPCHK(hipMemcpy(c->P[4].p + off, logdelta, sizeof(float) * (size_t)(Nv * nb), hipMemcpyHostToDevice));
  if (theta) HIPCHK(hipMemcpy(c->P[5].p + off, theta, sizeof(float) * (size_t)(Nv * nb), hipMemcpyHostToDevice));
  PMFCHK(rebuild_colmeta_views(c));
  return 0;
}

extern "C" int pmf_get_batch_view(pmf_ctx *c, int v, float *logdelta, float *theta) {
  PMFCHK(ctx_bind(c));
  if (v < 0 || v >= c->n_bv) return pmf_fail("batch view %d out of range (n=%d)", v, c->n_bv);
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t off = c->val_off[v], n = c->val_off[v + 1] - off;
  if (logdelta) HIPCHK(hipMemcpy(logdelta, c->P[4].p + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  if (theta) HIPCHK(hipMemcpy(theta, c->P[5].p + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// ---- noise model -------------------------------------------------------------------------------
// The table pmf_hinge_terms reads, from the thresholds t0 <= t1 <= t2 of one column: T[c] = lower bound of class c =
// (-Inf, t0, t1, t2)[c], T[4 + c] = its upper bound = (t0, t1, t2, +Inf)[c].  An infinite bound of either sign contributes
// nothing: a lower bound of +Inf (a class the column never holds) is stored as -Inf, an upper bound of -Inf as +Inf, so that
// relu(1 - (z - lo)) and relu(1 - (hi - z)) are 0 there without a select per entry.
static void hinge_table(const float t[3], float *T) {
  T[0] = -INFINITY;
  T[7] = INFINITY;
  for (int k = 0; k < 3; ++k) {
    T[1 + k] = std::isinf(t[k]) ? -INFINITY : t[k];
    T[4 + k] = std::isinf(t[k]) ? INFINITY : t[k];
  }
}
// device images of h_thr: {t0, t1, t2, 0} and the table per column; the columns of the other kinds and the pad columns hold
// bernoulli_sq_hinge's (0, +Inf, +Inf).  Only a model with a column that is not normal has them: nothing else reads them
// (the MIXED kernels do, for the dead columns of a ragged tile too), and an all-normal fit allocates what it always did.
static int upload_thresholds(pmf_ctx *c) {
  if (!c->mixed) return 0;
  const size_t np = (size_t)((c->N + PMF_DPAD - 1) / PMF_DPAD * PMF_DPAD);
  PMFCHK(c->thr.ensure(np, false, "the noise thresholds"));
  PMFCHK(c->htab.ensure(np * PMF_HT, false, "the noise threshold tables"));
  std::vector<float4> t(np, make_float4(0.f, INFINITY, INFINITY, 0.f));
  std::vector<float> T(np * PMF_HT);
  for (size_t j = 0; j < np; ++j) {
    if ((int64_t)j < c->N && !std::isnan(c->h_thr[j * 3])) t[j] = make_float4(c->h_thr[j * 3], c->h_thr[j * 3 + 1], c->h_thr[j * 3 + 2], 0.f);
    const float tj[3] = {t[j].x, t[j].y, t[j].z};
    hinge_table(tj, &T[j * PMF_HT]);
  }
  PMFCHK(c->thr.upload(t.data(), np));
  return c->htab.upload(T.data(), T.size());
}

extern "C" int pmf_set_noise(pmf_ctx *c, int n_ranges, const int64_t *s1, const int64_t *e1, const int32_t *kinds,
                             const float *weights) {
  PMFCHK(ctx_bind(c));
  if (c->N == 0) return pmf_fail("data not set");
  std::vector<int32_t> meta((size_t)c->N, 0);
  std::vector<uint8_t> covered((size_t)c->N, 0);
  bool mixed = false;
  for (int r = 0; r < n_ranges; ++r) {
    if (s1[r] < 1 || e1[r] > c->N || s1[r] > e1[r]) return pmf_fail("noise range %d: bad columns %lld:%lld", r, (long long)s1[r], (long long)e1[r]);
    if (kinds[r] < 0 || kinds[r] > 3) return pmf_fail("noise range %d: unsupported kind %d (normal=0, bernoulli=1, poisson=2, sq_hinge=3)", r, kinds[r]);
    if (kinds[r] != PMF_NOISE_NORMAL) mixed = true;
    for (int64_t j = s1[r] - 1; j < e1[r]; ++j) { meta[(size_t)j] = kinds[r]; covered[(size_t)j] = 1; }
  }
  for (int64_t j = 0; j < c->N; ++j)
    if (!covered[(size_t)j]) return pmf_fail("noise model does not cover column %lld", (long long)(j + 1));
  // thresholds: (0, +Inf, +Inf) -- bernoulli_sq_hinge -- for the kind-3 columns (pmf_set_noise_thresholds changes them);
  // the other kinds never read theirs (the same finite-or-Inf values on the device, NaN in what the getter reports)
  std::vector<float> h_thr((size_t)c->N * 3);
  for (int64_t j = 0; j < c->N; ++j) {
    const bool hg = meta[(size_t)j] == PMF_NOISE_SQ_HINGE;
    h_thr[(size_t)j * 3 + 0] = hg ? 0.f : NAN;
    h_thr[(size_t)j * 3 + 1] = h_thr[(size_t)j * 3 + 2] = hg ? INFINITY : NAN;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(c->colmeta, meta.data(), sizeof(int32_t) * (size_t)c->N, hipMemcpyHostToDevice));
  c->h_thr.swap(h_thr);
  if (weights) HIPCHK(hipMemcpy(c->colw, weights, sizeof(float) * (size_t)c->N, hipMemcpyHostToDevice));
  c->mixed = mixed;
  PMFCHK(upload_thresholds(c));
  c->noise_s1.assign(s1, s1 + n_ranges);
  c->noise_e1.assign(e1, e1 + n_ranges);
  c->h_kind.assign(meta.begin(), meta.end());
  c->kind_version++;
  PMFCHK(rebuild_colmeta_views(c));
  return 0;
}

extern "C" int pmf_set_noise_thresholds(pmf_ctx *c, int n_ranges, const int64_t *s1, const int64_t *e1, const float *thr) {
  PMFCHK(ctx_bind(c));
  if (c->N == 0 || (int64_t)c->h_kind.size() != c->N || (int64_t)c->h_thr.size() != 3 * c->N)
    return pmf_fail("the noise model must be set before its thresholds");
  for (int r = 0; r < n_ranges; ++r) {
    if (s1[r] < 1 || e1[r] > c->N || s1[r] > e1[r]) return pmf_fail("threshold range %d: bad columns %lld:%lld", r, (long long)s1[r], (long long)e1[r]);
    const float *t = thr + 3 * r;
    if (!(t[0] <= t[1] && t[1] <= t[2])) return pmf_fail("threshold range %d: need t0 <= t1 <= t2, got (%g, %g, %g)", r, t[0], t[1], t[2]);
    for (int64_t j = s1[r] - 1; j < e1[r]; ++j)
      if (c->h_kind[(size_t)j] != PMF_NOISE_SQ_HINGE)
        return pmf_fail("threshold range %d: column %lld is of noise kind %d, not sq_hinge (3)", r, (long long)(j + 1), (int)c->h_kind[(size_t)j]);
  }
  for (int r = 0; r < n_ranges; ++r)
    for (int64_t j = s1[r] - 1; j < e1[r]; ++j)
      for (int q = 0; q < 3; ++q) c->h_thr[(size_t)j * 3 + q] = thr[3 * r + q];
  HIPCHK(hipStreamSynchronize(c->stream));
  return upload_thresholds(c);
}

extern "C" int pmf_get_noise_thresholds(pmf_ctx *c, float *thr) {
  PMFCHK(ctx_bind(c));
  if (c->N == 0 || (int64_t)c->h_thr.size() != 3 * c->N) return pmf_fail("the noise model is not set");
  memcpy(thr, c->h_thr.data(), sizeof(float) * c->h_thr.size());
  return 0;
}

// ---- regularizers ------------------------------------------------------------------------------
static int add_quad_ranges(pmf_ctx *c, int which, int n_groups, const int64_t *s1, const int64_t *e1, const float *w, float p) {
  if (c->K == 0) return pmf_fail("factors must be set before their regularizers");
  ParamBuf &b = c->P[which];
  const int64_t n = which == 0 ? c->M : c->N;
  for (int g = 0; g < n_groups; ++g)
    if (s1[g] < 1 || e1[g] > n || s1[g] > e1[g]) return pmf_fail("regularizer range %d: bad %lld:%lld (n=%lld)", g, (long long)s1[g], (long long)e1[g], (long long)n);
  if (!b.wq) PMFCHK(b.wq.alloc((size_t)b.n, true));
  DevBuf<int64_t> ds, de;
  DevBuf<float> dw;
  PMFCHK(upload_new(ds, s1, (size_t)n_groups));
  PMFCHK(upload_new(de, e1, (size_t)n_groups));
  PMFCHK(upload_new(dw, w, (size_t)n_groups * c->K));
  k_expand_group<<<nblocks(b.n, 256), 256, 0, c->stream>>>(b.wq, c->Kp, c->K, n, ds, de, dw, n_groups, p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
static int add_quad_l2(pmf_ctx *c, int which, const float *w, float p) {
  const int64_t s1 = 1, e1 = which == 0 ? c->M : c->N;
  return add_quad_ranges(c, which, 1, &s1, &e1, w, p);
}
extern "C" int pmf_clear_xreg(pmf_ctx *c) {
  PMFCHK(ctx_bind(c));
  c->P[0].wq.free();
  c->P[0].wl1.free();
  netreg_free(c, 0);
  return 0;
}
extern "C" int pmf_add_xreg_l2(pmf_ctx *c, const float *w, float p) {
  PMFCHK(ctx_bind(c));
  return add_quad_l2(c, 0, w, p);
}
extern "C" int pmf_add_xreg_group(pmf_ctx *c, int n, const int64_t *s1, const int64_t *e1, const float *w, float p) {
  PMFCHK(ctx_bind(c));
  return add_quad_ranges(c, 0, n, s1, e1, w, p);
}
extern "C" int pmf_clear_yreg(pmf_ctx *c) {
  PMFCHK(ctx_bind(c));
  c->P[1].wq.free();
  c->P[1].wl1.free();
  netreg_free(c, 1);
  c->has_ard = false;
  c->ard_is_fsard = false;
  return 0;
}
extern "C" int pmf_add_yreg_l2(pmf_ctx *c, const float *w, float p) {
  PMFCHK(ctx_bind(c));
  return add_quad_l2(c, 1, w, p);
}
extern "C" int pmf_add_yreg_group(pmf_ctx *c, int n, const int64_t *s1, const int64_t *e1, const float *w, float p) {
  PMFCHK(ctx_bind(c));
  return add_quad_ranges(c, 1, n, s1, e1, w, p);
}
extern "C" int pmf_add_yreg_ard(pmf_ctx *c, int n_ranges, const int64_t *s1, const int64_t *e1, const float *alpha,
                                const float *beta, float p) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0) return pmf_fail("factors must be set before their regularizers");
  if (c->has_ard) return pmf_fail("only one ARD-type term (ARD or FeatureSetARD) is supported on Y");
  for (int r = 0; r < n_ranges; ++r)
    if (s1[r] < 1 || e1[r] > c->N || s1[r] > e1[r]) return pmf_fail("ARD range %d: bad %lld:%lld", r, (long long)s1[r], (long long)e1[r]);
  if (!c->ard_alpha) PMFCHK(c->ard_alpha.alloc((size_t)c->N, true));
  if (!c->ard_beta) PMFCHK(c->ard_beta.alloc((size_t)c->P[1].n, true));
  DevBuf<int64_t> ds, de;
  DevBuf<float> da, db;
  PMFCHK(upload_new(ds, s1, (size_t)n_ranges));
  PMFCHK(upload_new(de, e1, (size_t)n_ranges));
  PMFCHK(upload_new(da, alpha, (size_t)n_ranges));
  PMFCHK(upload_new(db, beta, (size_t)n_ranges));
  k_expand_ard<<<nblocks(c->P[1].n, 256), 256, 0, c->stream>>>(c->ard_alpha, c->ard_beta, c->Kp, c->N, ds, de, da, db, n_ranges);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ard_scale = p;
  c->has_ard = true;
  c->ard_is_fsard = false;
  return 0;
}
extern "C" int pmf_add_yreg_fsard(pmf_ctx *c, const float *alpha, const float *beta, float p) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0) return pmf_fail("factors must be set before their regularizers");
  if (c->has_ard) return pmf_fail("only one ARD-type term (ARD or FeatureSetARD) is supported on Y");
  if (!c->ard_alpha) PMFCHK(c->ard_alpha.alloc((size_t)c->N, true));
  if (!c->ard_beta) PMFCHK(c->ard_beta.alloc((size_t)c->P[1].n, true));
  PMFCHK(upload_vec(c, c->ard_alpha, alpha, (size_t)c->N));
  PMFCHK(upload_padded(c, c->ard_beta, beta, c->N, 1.f));
  c->ard_scale = p;
  c->has_ard = true;
  c->ard_is_fsard = true;
  return 0;
}

extern "C" int pmf_set_layer_regs(pmf_ctx *c, int n_ranges, const int64_t *s1, const int64_t *e1,
                                  const float *w_ls, const float *c_ls, const float *w_mu, const float *c_mu,
                                  const float *w_ld, const float *c_ld, const float *w_th, const float *c_th) {
  PMFCHK(ctx_bind(c));
  if (c->N == 0) return pmf_fail("data not set");
  for (int which = 2; which <= 5; ++which) { c->P[which].wq.free(); c->P[which].cq.free(); }
  if (n_ranges > 0) {
    DevBuf<int64_t> ds, de;
    DevBuf<float> dw, dc;
    PMFCHK(upload_new(ds, s1, (size_t)n_ranges));
    PMFCHK(upload_new(de, e1, (size_t)n_ranges));
    for (int t = 0; t < 2; ++t) {
      const float *w = t == 0 ? w_ls : w_mu, *cc = t == 0 ? c_ls : c_mu;
      if (!w || !cc) continue;
      ParamBuf &b = c->P[2 + t];
      PMFCHK(b.wq.alloc((size_t)c->N, true));
      PMFCHK(b.cq.alloc((size_t)c->N, true));
      PMFCHK(upload_new(dw, w, (size_t)n_ranges));
      PMFCHK(upload_new(dc, cc, (size_t)n_ranges));
      k_expand_colparam<<<nblocks(c->N, 256), 256, 0, c->stream>>>(b.wq, b.cq, c->N, ds, de, dw, dc, n_ranges);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));
    }
  }
  if (c->n_bv > 0 && c->P[4].n > 0) {
    const int64_t nbt = c->bvb_off[c->n_bv];
    std::vector<int32_t> nbs((size_t)c->n_bv);
    for (int v = 0; v < c->n_bv; ++v) nbs[v] = c->views[v].nb;
    DevBuf<int32_t> dnb;
    DevBuf<int64_t> dvo, dbo;
    DevBuf<float> dw, dc;
    PMFCHK(upload_new(dnb, nbs.data(), (size_t)c->n_bv));
    PMFCHK(upload_new(dvo, c->val_off.data(), (size_t)c->n_bv + 1));
    PMFCHK(upload_new(dbo, c->bvb_off.data(), (size_t)c->n_bv + 1));
    for (int t = 0; t < 2; ++t) {
      const float *w = t == 0 ? w_ld : w_th, *cc = t == 0 ? c_ld : c_th;
      if (!w || !cc) continue;
      ParamBuf &b = c->P[4 + t];
      PMFCHK(b.wq.alloc((size_t)b.n, true));
      PMFCHK(b.cq.alloc((size_t)b.n, true));
      PMFCHK(upload_new(dw, w, (size_t)nbt));
      PMFCHK(upload_new(dc, cc, (size_t)nbt));
      k_expand_batchreg<<<nblocks(b.n, 256), 256, 0, c->stream>>>(b.wq, b.cq, b.n, c->d_val_view, dvo, dnb, dbo, dw, dc);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));
    }
  }
  return 0;
}

// ---- optimizer ---------------------------------------------------------------------------------
extern "C" int pmf_set_optimizer(pmf_ctx *c, int kind, float lr, float eps, float b1, float b2) {
  PMFCHK(ctx_bind(c));
  if (kind != PMF_OPT_ADAGRAD && kind != PMF_OPT_ADAM) return pmf_fail("unknown optimizer kind %d", kind);
  c->opt_kind = kind;
  c->lr = lr;
  c->eps = eps;
  c->b1 = b1;
  c->b2 = b2;
  c->state_init = false;
  return 0;
}
extern "C" int pmf_set_lr(pmf_ctx *c, float lr) {
  PMFCHK(ctx_bind(c));
  c->lr = lr;
  return 0;
}
extern "C" int pmf_get_lr(pmf_ctx *c, float *lr) {
  PMFCHK(ctx_bind(c));
  *lr = c->lr;
  return 0;
}
extern "C" int pmf_reset_optimizer_state(pmf_ctx *c) {
  PMFCHK(ctx_bind(c));
  c->state_init = false;
  return 0;
}
static int init_opt_state(pmf_ctx *c) {
  for (int w = 0; w < 6; ++w) {
    ParamBuf &b = c->P[w];
    if (b.n == 0) continue;
    k_fill<<<nblocks(b.n, 256), 256, 0, c->stream>>>(b.acc, b.n, c->opt_kind == PMF_OPT_ADAGRAD ? c->eps : 0.f);
    k_fill<<<nblocks(b.n, 256), 256, 0, c->stream>>>(b.mom, b.n, 0.f);
    HIPCHK(hipGetLastError());
    b.bp1 = c->b1;
    b.bp2 = c->b2;
  }
  c->state_init = true;
  c->th.state_init = false;   // the thresholds' state resets with every other parameter's (thresh_fit_begin)
  return 0;
}

// ------------------------------------------------------------------------------------------------
// epoch machinery
// ------------------------------------------------------------------------------------------------
int prepare(pmf_ctx *c) {
  const int64_t nbt = c->n_bv > 0 ? c->val_off[c->n_bv] : 0;
  const int64_t n = std::max(c->N, nbt);
  k_prepare<<<nblocks(n, 256), 256, 0, c->stream>>>(c->P[2].p, c->P[3].p, c->colw, c->colmeta, c->colp, c->N,
                                                    c->P[4].p, c->P[5].p, c->btab, nbt);
  HIPCHK(hipGetLastError());
  c->btd_ok = false;
  c->nbs = c->n_bv > 0 ? 0 : 16;   // (0: no dense table; 16: the layer pass's tables without batch views)
  if (c->n_bv > 0) {
    PMFCHK(c->d_views.ensure((size_t)PMF_MAXV, false));   // (prepare() runs every layer epoch: no re-allocation)
    if (c->views_dirty) {
      HIPCHK(hipMemcpyAsync(c->d_views, c->views.data(), sizeof(ViewDesc) * (size_t)c->n_bv, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      c->views_dirty = false;
    }
    int nb_max = 0;
    for (int v = 0; v < c->n_bv; ++v) nb_max = std::max(nb_max, (int)c->views[v].nb);
    int shift = 4;
    while ((1 << shift) < nb_max + 1) ++shift;
    const int64_t Npad = (c->N + 31) / 32 * 32;
    if (nb_max <= 255 && (Npad << shift) < (1ll << 31)) {   // (the kernels index the table with 32 bits)
      c->nbs = 1 << shift;
      PMFCHK(c->btd.ensure((size_t)(Npad * c->nbs), false));
      PMFCHK(c->colview.ensure((size_t)Npad, false));
      DenseBtabArgs da;
      memset(&da, 0, sizeof(da));
      da.colmeta = c->colmeta; da.btab = c->btab; da.btd = c->btd; da.colview = c->colview; da.N = c->N; da.Npad = Npad; da.nbs_shift = shift;
      fill_views(c, da.views);
      k_dense_btab<<<nblocks(Npad * c->nbs, 256), 256, 0, c->stream>>>(da);
      HIPCHK(hipGetLastError());
      c->btd_ok = true;
    }
  }
  c->prepared = true;
  return 0;
}

// ---- host side of the column walk (k_layer_grad / k_stats)
// The shared arguments and the grid: gx blocks of 64 columns x gy block rows of a.rows_per_block rows.
static void col_walk_fill(pmf_ctx *c, ColWalkArgs &a, int &gx, int64_t &gy) {
  a.D = c->D; a.d_bf16 = c->store == PMF_STORE_BF16; a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.htab = c->htab; a.bor = c->bor; a.btab = c->btab;
  a.M = c->M; a.N = c->N; a.nRB = c->nRB; a.Kp = c->Kp; a.K = c->K;
  fill_views(c, a.views, a.val_off);
  a.max_nb = 1;
  for (int v = 0; v < c->n_bv; ++v) a.max_nb = std::max(a.max_nb, c->views[v].nb);
  gx = nblocks(c->N, 64);
  // ~32 single-wave workgroups per CU hide the FMA / LDS latencies; at least 256 rows per workgroup keep the final
  // partial stores (64 * (2 + 2 nb) per workgroup, added by k_sum_parts) negligible
  gy = std::max<int64_t>(1, std::min<int64_t>((32ll * c->n_cu + gx - 1) / gx, (c->M + 255) / 256));
  a.rows_per_block = (int)((c->M + gy - 1) / gy);
  gy = (c->M + a.rows_per_block - 1) / a.rows_per_block;
}
// Launches kerns[KB - 1].  The [2][max_nb][64] batch sums are dynamic LDS on top of the kernel's static LDS (k_layer_grad:
// block_reduce_sum's slots): past 160 KiB together the launch is refused (col_walk_check), naming the batch count.
static int col_walk_check(pmf_ctx *c, const void *const (&kerns)[4], int max_nb, const char *what, size_t *lds_out) {
  if (c->KB < 1 || c->KB > 4) return pmf_fail("unsupported KB=%d", c->KB);
  const void *kern = kerns[c->KB - 1];
  const size_t lds = col_walk_lds(c->Kp, max_nb);
  hipFuncAttributes fa;
  HIPCHK(hipFuncGetAttributes(&fa, kern));
  if (lds + fa.sharedSizeBytes > 160 * 1024)
    return pmf_fail("too many row batches per view (%d) for the %s kernel", max_nb, what);
  if (lds_out) *lds_out = lds;
  return 0;
}
template <typename Args>
static int col_walk_launch(pmf_ctx *c, void (*const (&kerns)[4])(const Args), const Args &a, int gx, int64_t gy, const char *what) {
  size_t lds = 0;
  PMFCHK(col_walk_check(c, {(const void *)kerns[0], (const void *)kerns[1], (const void *)kerns[2], (const void *)kerns[3]}, a.max_nb, what, &lds));
  PMFCHK(ensure_dyn_lds(c, (const void *)kerns[c->KB - 1], lds));
  hipLaunchKernelGGL(kerns[c->KB - 1], dim3(gx, (unsigned)gy), dim3(64), lds, c->stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

// where the layer gradients go: null for a frozen layer (bits of frozen_layers: 1 logsigma, 2 logdelta, 4 mu, 8 theta) and
// for the batch layers of a model without batch views
static void layer_grad_targets(pmf_ctx *c, const pmf_fit_opts *o, float *&g_logsigma, float *&g_logdelta, float *&g_mu, float *&g_theta) {
  const int fl = o->frozen_layers;
  g_logsigma = (fl & 1) ? nullptr : c->P[2].g;
  g_logdelta = ((fl & 2) || c->n_bv == 0) ? nullptr : c->P[4].g;
  g_mu = (fl & 4) ? nullptr : c->P[3].g;
  g_theta = ((fl & 8) || c->n_bv == 0) ? nullptr : c->P[5].g;
}

static int launch_layer_grad(pmf_ctx *c, const pmf_fit_opts *o, bool with_loss) {
  LayerGradArgs a;
  memset(&a, 0, sizeof(a));
  int gx; int64_t gy;
  col_walk_fill(c, a, gx, gy);
  layer_grad_targets(c, o, a.g_logsigma, a.g_logdelta, a.g_mu, a.g_theta);
  if (with_loss) {
    PMFCHK(ensure_loss_partials(c, (int64_t)gx * gy));
    a.loss_partial = c->loss_partial;
  }
  // private partials per block row, summed in fixed order afterwards (every entry of a vector is written by its block)
  const int64_t nbt = c->n_bv > 0 ? c->val_off[c->n_bv] : 0;
  a.nbt = nbt;
  a.part_stride = 2 * c->N + 2 * nbt;
  PMFCHK(c->lgrad_part.ensure((size_t)(a.part_stride * gy), false));
  a.part = c->lgrad_part;
  PMFCHK(col_walk_launch(c, {k_layer_grad<1>, k_layer_grad<2>, k_layer_grad<3>, k_layer_grad<4>}, a, gx, gy, "layer-gradient"));
  PMFCHK(sum_parts(c, a.part, a.part_stride, (int)gy, a.g_mu, c->N));
  PMFCHK(sum_parts(c, a.part + c->N, a.part_stride, (int)gy, a.g_logsigma, c->N));
  PMFCHK(sum_parts(c, a.part + 2 * c->N, a.part_stride, (int)gy, a.g_theta, nbt));
  PMFCHK(sum_parts(c, a.part + 2 * c->N + nbt, a.part_stride, (int)gy, a.g_logdelta, nbt));
  return 0;
}

// Layer-parameter gradients through the MFMA layer pass (its own loss only in layer-only epochs) while its LDS, with the
// unit's [64 columns][nbs] batch table, fits in 160 KiB: up to 127 batches per view at K <= 32 and 65..96 (and at 33..64
// with PMF_LAYER_NW=4), 63 at 33..64 and 97..128.  Otherwise, and without a dense table (more than
// 255 batches), the VALU kernel above (PMF_LAYER_OLD=1 forces it, for comparison).
static int layer_pass_waves(pmf_ctx *c) {   // waves per workgroup of the layer pass
  const char *lnwenv = getenv("PMF_LAYER_NW");
  return (c->KB <= 2 && !(lnwenv && atoi(lnwenv) == 4)) ? 8 : 4;
}
static bool layer_pass_eligible(pmf_ctx *c) {
  const char *e = getenv("PMF_LAYER_OLD");
  if (e && atoi(e) == 1) return false;
  if (c->KB > 4 || (c->n_bv > 0 && !c->btd_ok)) return false;
  // the batch table of the unit's 64 columns (nbs slots each) lives in LDS next to the Y tiles and the X panels
  return pmf_layer_pass_lds(c->KB, layer_pass_waves(c), c->n_bv > 0 ? c->nbs : 16) <= 160 * 1024;
}
static int launch_layer_pass(pmf_ctx *c, const pmf_fit_opts *o, bool with_loss) {
  const int lnw = layer_pass_waves(c);
  const int nbs = c->n_bv > 0 ? c->nbs : 16;
  int nbs_shift = 0;
  while ((1 << nbs_shift) < nbs) ++nbs_shift;
  const int64_t n_ct = (c->N + PMF_BN - 1) / PMF_BN, n_rp = (c->M + 32 * lnw - 1) / (32 * lnw);
  const int64_t n_seg = (n_ct + PMF_LS - 1) / PMF_LS;
  int64_t R = std::max<int64_t>(1, std::min<int64_t>(n_rp, (4ll * c->n_cu + n_seg - 1) / n_seg));
  const int grid = (int)std::min<int64_t>(n_seg * R, c->n_cu);
  // one private [N][nbs] table per (row range, wave, lane half): plain read-modify-writes, no float atomics, summed in
  // fixed order by k_layer_reduce.  R <= ceil(4 n_cu / n_seg) keeps R * N near 4 n_cu * 64 columns (~130 MB of tables at
  // nbs = 16) while n_seg < 4 n_cu; from n_seg >= 4 n_cu on R = 1 and the tables grow with N (2 NW * N * nbs float2).
  const int64_t lg_stride = c->N * nbs, n_parts = R * lnw * 2;
  PMFCHK(c->LG.ensure((size_t)(lg_stride * n_parts), false));
  HIPCHK(hipMemsetAsync(c->LG, 0, sizeof(float2) * (size_t)(lg_stride * n_parts), c->stream));
  if (with_loss) PMFCHK(ensure_loss_partials(c, grid));
  LayerPassArgs a;
  memset(&a, 0, sizeof(a));
  a.D = c->D; a.d_bf16 = c->store == PMF_STORE_BF16; a.nRB = c->nRB; a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.htab = c->htab; a.bor = c->bor;
  a.btd = c->n_bv > 0 ? c->btd : nullptr; a.LG = c->LG; a.lg_stride = lg_stride; a.loss_partial = with_loss ? c->loss_partial : nullptr;
  a.M = c->M; a.N = c->N; a.n_bv = c->n_bv; a.n_ct = (int)n_ct; a.n_rp = (int)n_rp; a.n_seg = (int)n_seg; a.R = (int)R;
  a.nbs_shift = nbs_shift;
  PMFCHK(pmf_launch_layer_pass(&c->dyn_lds, c->stream, c->KB, lnw, c->mixed, grid, a));
  LayerMapArgs m;
  memset(&m, 0, sizeof(m));
  m.LG = c->LG; m.lg_stride = lg_stride; m.n_parts = (int32_t)n_parts; m.btd = a.btd; m.colp = c->colp; m.N = c->N; m.n_bv = c->n_bv; m.nbs_shift = nbs_shift;
  layer_grad_targets(c, o, m.g_logsigma, m.g_logdelta, m.g_mu, m.g_theta);
  fill_views(c, m.views, m.val_off);
  return pmf_launch_layer_map(c->stream, m);
}

int check_ready(pmf_ctx *c) {
  if (!c->D) return pmf_fail("data not set");
  if (c->K == 0) return pmf_fail("factors not set");
  for (int v = 0; v < c->n_bv; ++v)
    if (c->views[v].nb == 0) return pmf_fail("batch view %d declared but not set", v);
  return 0;
}

// Regularizer + optimizer step of elements [e0, e0 + n) of parameter `which` (whole tensor: e0 = 0, n = b.n).  For X / Y,
// e0 and n are multiples of Kp (whole columns): the pipelined loop of pmf_fit steps Y one column chunk at a time.
// `max_blocks` bounds the grid (= loss partials appended to the slab); `advance` moves Adam's running beta powers on
// (once per epoch, with the last slice).
int step_param_range(pmf_ctx *c, int which, int64_t e0, int64_t n, bool do_step, bool use_reg, int reg_slot,
                            int *reg_count, int max_blocks, bool advance) {
  ParamBuf &b = c->P[which];
  if (b.n == 0 || n == 0) return 0;
  StepArgsGraph s;   // (the plain instance takes its StepArgs part)
  memset(&s, 0, sizeof(s));
  s.p = b.p + e0; s.g = b.g + e0; s.acc = b.acc + e0; s.mom = b.mom + e0;
  s.wq = b.wq ? b.wq + e0 : nullptr; s.cq = b.cq ? b.cq + e0 : nullptr;
  s.Kp = which <= 1 ? c->Kp : 1;
  s.K = which <= 1 ? c->K : 1;
  if (which == 1 && c->has_ard) { s.ard_alpha = c->ard_alpha + e0 / s.Kp; s.ard_beta = c->ard_beta + e0; s.ard_scale = c->ard_scale; }
  s.gpre = which <= 1 && c->net[which] ? c->net[which]->grad + e0 : nullptr;
  s.wl1 = b.wl1 ? b.wl1 + e0 : nullptr;
  s.n = n;
  s.opt_kind = c->opt_kind; s.lr = c->lr; s.eps = c->eps; s.b1 = c->b1; s.b2 = c->b2;
  s.c1 = 1.f - b.bp1; s.c2 = 1.f - b.bp2;
  s.do_step = do_step; s.use_reg = use_reg;
  const int grid = (int)std::min<int64_t>(max_blocks, nblocks(n, 256));
  s.reg_partial = c->reg_partial + (int64_t)reg_slot * REG_SLOTS + *reg_count;
  if (*reg_count + grid > REG_SLOTS) return pmf_fail("internal: regularizer partial slab overflow");
  if (use_reg && (s.gpre || s.wl1)) k_reg_step<true><<<grid, 256, 0, c->stream>>>(s);
  else k_reg_step<false><<<grid, 256, 0, c->stream>>>(s);
  HIPCHK(hipGetLastError());
  *reg_count += grid;
  if (advance && do_step && c->opt_kind == PMF_OPT_ADAM) { b.bp1 *= c->b1; b.bp2 *= c->b2; }
  return 0;
}
int step_param(pmf_ctx *c, int which, bool do_step, bool use_reg, int reg_slot, int *reg_count) {
  // the four layer parameters share one slab of loss partials: each gets a quarter (k_reg_step is grid-stride); X / Y get
  // what a network term evaluated before the step has left of theirs
  return step_param_range(c, which, 0, c->P[which].n, do_step, use_reg, reg_slot, reg_count, reg_slot == 2 ? REG_SLOTS / 4 : REG_SLOTS - *reg_count, true);
}
void step_args_xy(pmf_ctx *c, int which, StepArgs *s) {
  ParamBuf &b = c->P[which];
  memset(s, 0, sizeof(*s));
  s->p = b.p; s->g = b.g; s->wq = b.wq; s->cq = b.cq;
  s->Kp = c->Kp; s->K = c->K; s->n = b.n;
  if (which == 1 && c->has_ard) { s->ard_alpha = c->ard_alpha; s->ard_beta = c->ard_beta; s->ard_scale = c->ard_scale; }
  s->use_reg = 1;
}
// layer l <-> param: 1 logsigma(2), 2 logdelta(4), 3 mu(3), 4 theta(5)
int step_layers(pmf_ctx *c, const pmf_fit_opts *o, int *reg_count) {
  const int fl = o->frozen_layers, fr = o->frozen_regs;
  const int pmap[4] = {2, 4, 3, 5};
  for (int l = 0; l < 4; ++l) {
    const bool frozen = (fl >> l) & 1;
    const bool reg_on = !frozen && !((fr >> l) & 1);
    if (frozen) continue;  // FrozenLayer: no step, regularizer evaluates to 0 (regularizers.jl:508-510, 887-889)
    PMFCHK(step_param(c, pmap[l], true, reg_on, 2, reg_count));
  }
  c->prepared = false;
  return 0;
}

// what every epoch starts with: optimizer state, prepared column / batch tables, cleared layer gradients
int epoch_open(pmf_ctx *c, const pmf_fit_opts *o) {
  if (!c->state_init) PMFCHK(init_opt_state(c));
  if (!c->prepared || o->update_col_layers) PMFCHK(prepare(c));
  // (grad(X) and grad(Y) need no clearing: k_gx_reduce / k_gy_reduce overwrite every element)
  if (o->update_col_layers)
    for (int w = 2; w < 6; ++w)
      if (c->P[w].n) HIPCHK(hipMemsetAsync(c->P[w].g, 0, sizeof(float) * (size_t)c->P[w].n, c->stream));
  return 0;
}
int epoch_layer_pass(pmf_ctx *c, const pmf_fit_opts *o, bool with_loss) {
  if (layer_pass_eligible(c)) { c->last_layer_path = 1; return launch_layer_pass(c, o, with_loss); }
  c->last_layer_path = 2;
  return launch_layer_grad(c, o, with_loss);
}

extern "C" int pmf_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes) {
  if (device_bytes) *device_bytes = pmf_live_bytes[0].load();
  if (pinned_bytes) *pinned_bytes = pmf_live_bytes[1].load();
  return 0;
}

extern "C" int pmf_epoch_begin(pmf_ctx *c, const pmf_fit_opts *o) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  if (!o) return pmf_fail("null opts");
  PMFCHK(epoch_open(c, o));
  for (int q = 0; q < 4; ++q) c->reg_counts[q] = 0;
  const bool fused = o->update_X || o->update_Y || !o->update_col_layers;
  if (fused) PMFCHK(launch_fused(c, o->update_X != 0, o->update_Y != 0));
  if (o->update_col_layers) PMFCHK(epoch_layer_pass(c, o, !fused));
  return 0;
}

extern "C" int pmf_epoch_step_local(pmf_ctx *c, const pmf_fit_opts *o) {
  PMFCHK(ctx_bind(c));
  if (o->update_X) {
    PMFCHK(netreg_eval(c, 0, &c->reg_counts[0]));
    PMFCHK(step_param(c, 0, true, true, 0, &c->reg_counts[0]));
  }
  return 0;
}

extern "C" int pmf_epoch_step_shared(pmf_ctx *c, const pmf_fit_opts *o) {
  PMFCHK(ctx_bind(c));
  if (o->update_Y) {
    PMFCHK(netreg_eval(c, 1, &c->reg_counts[1]));
    PMFCHK(step_param(c, 1, true, true, 1, &c->reg_counts[1]));
  }
  if (o->update_col_layers) PMFCHK(step_layers(c, o, &c->reg_counts[2]));
  return 0;
}

extern "C" int pmf_epoch_loss(pmf_ctx *c, double *local_loss, double *shared_terms) {
  PMFCHK(ctx_bind(c));
  RegCounts rc;
  for (int q = 0; q < 4; ++q) rc.c[q] = c->reg_counts[q];
  PMFCHK(launch_loss_reduce(c, rc, 0x1f));
  HIPCHK(hipMemcpyAsync(c->h_loss, c->d_loss, sizeof(double) * 5, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  harvest_events(c);
  const double shared = c->h_loss[2] + c->h_loss[3];
  if (local_loss) *local_loss = c->h_loss[0] + c->h_loss[1] + shared;
  if (shared_terms) *shared_terms = shared;
  return 0;
}

// ---- full loss / data gradients at the current parameters (pmf_loss, pmf_fit_lbfgs)
int eval_full_loss(pmf_ctx *c, double out[4]) {
  if (c->net[0] || c->net[1])
    return pmf_fail("pmf_loss: a network term is attached; evaluating it would move its warm-start state");
  if (!c->prepared) PMFCHK(prepare(c));
  PMFCHK(launch_fused(c, false, false));
  RegCounts rc = {{0, 0, 0, 0}};
  PMFCHK(step_param(c, 0, false, true, 0, &rc.c[0]));
  PMFCHK(step_param(c, 1, false, true, 1, &rc.c[1]));
  PMFCHK(launch_loss_reduce(c, rc, 0x7));
  HIPCHK(hipMemcpyAsync(c->h_loss, c->d_loss, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  harvest_events(c);
  out[1] = c->h_loss[0]; out[2] = c->h_loss[1]; out[3] = c->h_loss[2];
  out[0] = out[1] + out[2] + out[3];
  return 0;
}
int eval_data_grads(pmf_ctx *c) {
  if (!c->prepared) PMFCHK(prepare(c));
  return launch_fused(c, true, true);
}
extern "C" int pmf_loss(pmf_ctx *c, double *total, double *data, double *xreg, double *yreg) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  double v[4];
  PMFCHK(eval_full_loss(c, v));
  if (total) *total = v[0];
  if (data) *data = v[1];
  if (xreg) *xreg = v[2];
  if (yreg) *yreg = v[3];
  return 0;
}

extern "C" int pmf_grad_device_ptr(pmf_ctx *c, int which, void **ptr, int64_t *n) {
  PMFCHK(ctx_bind(c));
  if (which < 0 || which > 5) return pmf_fail("bad parameter id %d", which);
  if (ptr) *ptr = c->P[which].g;
  if (n) *n = c->P[which].n;
  return 0;
}

extern "C" int pmf_get_grad(pmf_ctx *c, int which, int view, float *out) {
  PMFCHK(ctx_bind(c));
  if (which < 0 || which > 5) return pmf_fail("bad parameter id %d", which);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (which <= 1) return download_padded(c, out, c->P[which].g, which == 0 ? c->M : c->N);
  if (which <= 3) {
    HIPCHK(hipMemcpy(out, c->P[which].g, sizeof(float) * (size_t)c->N, hipMemcpyDeviceToHost));
    return 0;
  }
  if (view < 0 || view >= c->n_bv) return pmf_fail("batch view %d out of range", view);
  const int64_t off = c->val_off[view], n = c->val_off[view + 1] - off;
  HIPCHK(hipMemcpy(out, c->P[which].g + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// optimizer state of one parameter group in the reference's shape: AdaGrad's accumulator (or Adam's second moment)
// and Adam's first moment (Flux.Optimise.AdaGrad.acc / Adam's (mt, vt), reached through src/optimizers.jl:6-13)
extern "C" int pmf_get_opt_state(pmf_ctx *c, int which, int view, float *acc, float *mom) {
  PMFCHK(ctx_bind(c));
  if (which < 0 || which > 5) return pmf_fail("bad parameter id %d", which);
  if (!c->state_init) return pmf_fail("optimizer state not initialised yet (no epoch has run since pmf_set_optimizer)");
  HIPCHK(hipStreamSynchronize(c->stream));
  const ParamBuf &b = c->P[which];
  if (which <= 1) {
    const int64_t n = which == 0 ? c->M : c->N;
    if (acc) PMFCHK(download_padded(c, acc, b.acc, n));
    if (mom) PMFCHK(download_padded(c, mom, b.mom, n));
    return 0;
  }
  int64_t off = 0, n = c->N;
  if (which >= 4) {
    if (view < 0 || view >= c->n_bv) return pmf_fail("batch view %d out of range", view);
    off = c->val_off[view];
    n = c->val_off[view + 1] - off;
  }
  if (acc) HIPCHK(hipMemcpy(acc, b.acc + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  if (mom) HIPCHK(hipMemcpy(mom, b.mom + off, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// ---- the statistics pass behind pmf_stats and the stage entries of pmf_stages.hip
static void (*const k_stats_kb[4])(const StatsArgs) = {k_stats<1>, k_stats<2>, k_stats<3>, k_stats<4>};
int stats_pass_check(pmf_ctx *c) {
  int max_nb = 1;
  for (int v = 0; v < c->n_bv; ++v) max_nb = std::max(max_nb, (int)c->views[v].nb);
  return col_walk_check(c, {(const void *)k_stats_kb[0], (const void *)k_stats_kb[1], (const void *)k_stats_kb[2], (const void *)k_stats_kb[3]}, max_nb, "statistics", nullptr);
}
int stats_pass(pmf_ctx *c, int use_factors, bool want_cols, bool want_batch, const float **cols, const float **batch) {
  PMFCHK(prepare(c));
  const int64_t nbt = (want_batch && c->n_bv > 0) ? c->val_off[c->n_bv] : 0;
  const int64_t ncol = want_cols ? 5 * c->N : 0;
  const size_t nfl = (size_t)(ncol + 2 * nbt);
  StatsArgs a;
  memset(&a, 0, sizeof(a));
  int gx; int64_t gy;
  col_walk_fill(c, a, gx, gy);
  a.use_factors = use_factors;
  // scratch: [results nfl][gy private partial vectors of nfl]; every entry of a partial vector is written by its block row,
  // the block rows are then added in fixed order (k_sum_parts): no float atomics, bitwise reproducible statistics
  PMFCHK(c->scratch.ensure(sizeof(float) * std::max<size_t>(nfl * (size_t)(gy + 1), 1), false));
  float *buf = (float *)c->scratch.p, *part = buf + nfl;
  a.part_stride = (int64_t)nfl;
  if (want_cols) { a.col_n = part; a.col_sum = part + c->N; a.col_sumsq = part + 2 * c->N; a.col_sqerr = part + 3 * c->N; a.col_ssqg = part + 4 * c->N; }
  a.b_n = nbt ? part + ncol : nullptr;
  a.b_sqerr = nbt ? part + ncol + nbt : nullptr;
  PMFCHK(col_walk_launch(c, k_stats_kb, a, gx, gy, "statistics"));
  PMFCHK(sum_parts(c, part, (int64_t)nfl, (int)gy, buf, (int64_t)nfl));
  if (cols) *cols = want_cols ? buf : nullptr;
  if (batch) *batch = nbt ? buf + ncol : nullptr;
  return 0;
}

extern "C" int pmf_stats(pmf_ctx *c, int use_factors, float *col_n, float *col_sum, float *col_sumsq, float *col_sqerr,
                         float *col_ssq_grad, float *batch_count, float *batch_sqerr) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  const int64_t nbt = c->n_bv > 0 ? c->val_off[c->n_bv] : 0;
  const float *buf = nullptr, *bbuf = nullptr;
  PMFCHK(stats_pass(c, use_factors, true, true, &buf, &bbuf));
  HIPCHK(hipStreamSynchronize(c->stream));
  float *outs[5] = {col_n, col_sum, col_sumsq, col_sqerr, col_ssq_grad};
  for (int q = 0; q < 5; ++q)
    if (outs[q]) HIPCHK(hipMemcpy(outs[q], buf + (int64_t)q * c->N, sizeof(float) * (size_t)c->N, hipMemcpyDeviceToHost));
  if (batch_count && nbt) HIPCHK(hipMemcpy(batch_count, bbuf, sizeof(float) * (size_t)nbt, hipMemcpyDeviceToHost));
  if (batch_sqerr && nbt) HIPCHK(hipMemcpy(batch_sqerr, bbuf + nbt, sizeof(float) * (size_t)nbt, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int pmf_kernel_time(pmf_ctx *c, double *mean_ms, int64_t *launches, int reset) {
  PMFCHK(ctx_bind(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  harvest_events(c);
  if (mean_ms) *mean_ms = c->kernel_launches > 0 ? c->kernel_ms_sum / (double)c->kernel_launches : 0.0;
  if (launches) *launches = c->kernel_launches;
  if (reset) { c->kernel_ms_sum = 0.0; c->kernel_launches = 0; }
  return 0;
}
