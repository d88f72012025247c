// pmf_stages.hip -- the closed-form stages that sit between the gradient-descent stages (src/fit.jl:125-187, 297-375;
// src/regularizers.jl:750-774), run on the device behind one C entry each (pmf_stage_*, include/pmf_hip.h).
//
// Every data pass is the k_stats column walk of pmf_hip.hip (stats_pass); its f32 sums stay on the device, are widened to
// f64 (k_st_widen) into a buffer this file owns and -- with a communicator of more than one rank -- summed over the ranks
// there, ONE collective per pass, before any arithmetic.  All arithmetic on the statistics is f64; a result is rounded
// to f32 where the parameter is f32.  The rules are those of pathmatfac.jl_amd/fit.py:181-283, which cites the reference.
//   k_stage_logsigma      logsigma_j = log sqrt(sqerr_j / n_j)                                    (init_logsigma!)
//   k_stage_reweight      w_j = 1 / (sqrt(ssq_grad_j / M) exp(logsigma_j)), non-finite -> 1       (reweight_col_losses!)
//   k_stage_group         per noise range K mean(sigma^2) / (sum_j var_j n_j / M)                 (construct_minimal_regularizer)
//   k_em_moments          per (view, batch) row: mean / sample variance of theta, (alpha, beta) of delta^2 (theta_mom, delta2_mom)
//   k_em_theta            the theta update, with the partial sums of the stopping rule            (theta_delta_em :350, :363)
//                         (theta lives in f64 for the length of the EM, as in fit.py and like delta^2: the moments and the
//                         stopping rule read that copy; the f32 parameter, which the statistics pass reads, is its rounding)
//   k_em_diff             the two sums of the stopping rule, one workgroup, index order
//   k_em_delta2           the delta^2 update                                                      (:359)
// Sums: per thread over its strided elements, lanes by shuffles, the four waves in index order, workgroups through a slab
// that one workgroup adds in index order.  No atomics: every output is bitwise the same run to run, and -- all ranks
// holding the same reduced statistics and the same replicated parameters -- rank to rank.
#include "pmf_ctx.h"

static inline unsigned st_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }
#define ST_MAXB 1024   // workgroups of the theta update at most = partials per sum of the stopping rule

__device__ __forceinline__ bool st_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // (false for NaN)

// Four consecutive elements per thread: 128-bit loads and stores for a whole quad at a 16-byte aligned address (`vec`:
// the array's base is; e0 is a multiple of 4), element by element for the partial last quad and for an unaligned base.
template <typename T>
__device__ __forceinline__ void st_ld4(const T *__restrict__ p, int64_t e0, int cnt, bool vec, T (&o)[4]) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- or 8-byte elements");
  if (cnt == 4 && vec) {
    if constexpr (sizeof(T) == 4) {
      const uint4 v = *reinterpret_cast<const uint4 *>(p + e0);
      __builtin_memcpy(o, &v, 16);
    } else {
      const uint4 v0 = *reinterpret_cast<const uint4 *>(p + e0), v1 = *reinterpret_cast<const uint4 *>(p + e0 + 2);
      __builtin_memcpy(&o[0], &v0, 16);
      __builtin_memcpy(&o[2], &v1, 16);
    }
  } else {
    for (int k = 0; k < cnt; ++k) o[k] = p[e0 + k];
  }
}
template <typename T>
__device__ __forceinline__ void st_st4(T *__restrict__ p, int64_t e0, int cnt, bool vec, const T (&o)[4]) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- or 8-byte elements");
  if (cnt == 4 && vec) {
    if constexpr (sizeof(T) == 4) {
      uint4 v;
      __builtin_memcpy(&v, o, 16);
      *reinterpret_cast<uint4 *>(p + e0) = v;
    } else {
      uint4 v0, v1;
      __builtin_memcpy(&v0, &o[0], 16);
      __builtin_memcpy(&v1, &o[2], 16);
      *reinterpret_cast<uint4 *>(p + e0) = v0;
      *reinterpret_cast<uint4 *>(p + e0 + 2) = v1;
    }
  } else {
    for (int k = 0; k < cnt; ++k) p[e0 + k] = o[k];
  }
}
static inline bool st_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline unsigned st_grid4(int64_t n) { return (unsigned)std::max<int64_t>(1, ((n + 3) / 4 + 255) / 256); }

__global__ __launch_bounds__(256) void k_st_widen(const float *__restrict__ src, double *__restrict__ dst, int64_t n, int src_vec) {
  const int64_t e0 = 4 * (blockIdx.x * 256ll + threadIdx.x);
  if (e0 >= n) return;
  const int cnt = (int)(n - e0 < 4 ? n - e0 : 4);
  float s[4];
  double d[4];
  st_ld4(src, e0, cnt, src_vec != 0, s);
  for (int k = 0; k < cnt; ++k) d[k] = (double)s[k];
  st_st4(dst, e0, cnt, true, d);   // (dst is the base of an allocation of the caller's)
}
__global__ __launch_bounds__(256) void k_st_fill(float *p, int64_t n, float v) {
  const int64_t e0 = 4 * (blockIdx.x * 256ll + threadIdx.x);
  if (e0 >= n) return;
  const float o[4] = {v, v, v, v};
  st_st4(p, e0, (int)(n - e0 < 4 ? n - e0 : 4), true, o);
}

// st = {n, sum, sumsq, sqerr, ssq_grad}, N doubles each
__global__ __launch_bounds__(256) void k_stage_logsigma(const double *__restrict__ st, float *__restrict__ logsigma, int64_t N) {
  const int64_t j = blockIdx.x * 256ll + threadIdx.x;
  if (j < N) logsigma[j] = (float)log(sqrt(st[3 * N + j] / st[j]));   // n = 0: NaN; a zero residual: -inf (kept, as on the host)
}
__global__ __launch_bounds__(256) void k_stage_reweight(const double *__restrict__ st, const float *__restrict__ logsigma,
                                                         float *__restrict__ colw, int64_t N, double M_total) {
  const int64_t j = blockIdx.x * 256ll + threadIdx.x;
  if (j >= N) return;
  const double rms = sqrt(st[4 * N + j] / M_total) * exp((double)logsigma[j]);
  double w = 1.0 / rms;
  if (!st_finite(w)) w = 1.0;
  colw[j] = (float)w;
}
// one workgroup per noise range r: columns s1[r] .. e1[r] (1-based, inclusive)
__global__ __launch_bounds__(256) void k_stage_group(const double *__restrict__ st, const float *__restrict__ logsigma,
                                                      const int64_t *__restrict__ s1, const int64_t *__restrict__ e1, int64_t N,
                                                      double K, double M_total, float *__restrict__ out) {
  __shared__ double sh[4];
  const int64_t j0 = s1[blockIdx.x] - 1, j1 = e1[blockIdx.x];
  double ssig = 0.0, svar = 0.0;
  for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) {
    const double n = st[j], mean = st[N + j] / n;
    double var = (st[2 * N + j] - n * mean * mean) / fmax(n - 1.0, 1.0);   // unbiased, from sum / sumsq
    if (!st_finite(var)) var = 0.0;
    var = fmax(var, 1.0 / M_total);
    const double sig = exp((double)logsigma[j]);
    ssig += sig * sig;
    svar += var * n;
  }
  const double a = block_all_sum_256(ssig, sh), b = block_all_sum_256(svar, sh);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(K * (a / (double)(j1 - j0)) / (b / M_total));
}

// ---- batch-effect EM
struct EmGeom {
  int n_bv;
  ViewDesc views[PMF_MAXV];
  int64_t val_off[PMF_MAXV + 1];   // per view: offset into the arrays that are flat like theta (nb x N_v column-major per view)
  int64_t bvb_off[PMF_MAXV + 1];   // per view: offset into the per-(view, batch) arrays
};
// mean and sample variance (two-pass) of row (view, batch) = blockIdx.x of x over the view's columns
template <typename T>
__device__ __forceinline__ void em_row_moments(const T *__restrict__ x, int64_t base, int64_t nb, int64_t Nv, double *sh,
                                               double &mean, double &var) {
  double s = 0.0;
  for (int64_t jj = threadIdx.x; jj < Nv; jj += 256) s += (double)x[base + jj * nb];
  mean = block_all_sum_256(s, sh) / (double)Nv;
  double q = 0.0;
  for (int64_t jj = threadIdx.x; jj < Nv; jj += 256) {
    const double d = (double)x[base + jj * nb] - mean;
    q += d * d;
  }
  var = block_all_sum_256(q, sh) / (double)(Nv - 1);   // N_v = 1: 0 / 0 = NaN, absorbed by the updates' NaN rules
}
// mom = [theta mean | theta var | alpha | beta], n_rows doubles each
__global__ __launch_bounds__(256) void k_em_moments(const double *__restrict__ theta, const double *__restrict__ delta2,
                                                     const EmGeom g, int64_t n_rows, double *__restrict__ mom) {
  __shared__ double sh[4];
  const int64_t r = blockIdx.x;
  int v = 0;
  while (v + 1 < g.n_bv && r >= g.bvb_off[v + 1]) ++v;
  const int64_t nb = g.views[v].nb, Nv = g.views[v].c1 - g.views[v].c0, base = g.val_off[v] + (r - g.bvb_off[v]);
  double tm, tv, dm, dv;
  em_row_moments(theta, base, nb, Nv, sh, tm, tv);
  em_row_moments(delta2, base, nb, Nv, sh, dm, dv);
  if (threadIdx.x == 0) {
    const double alpha = 2.0 + (dm * dm) / (dv + 1e-9);
    mom[r] = tm;
    mom[n_rows + r] = tv;
    mom[2 * n_rows + r] = alpha;
    mom[3 * n_rows + r] = dm * (alpha - 1.0);
  }
}
struct EmArgs {
  float *theta;          // the parameter: the rounding of theta64, read by the statistics pass
  double *theta64;       // theta for the length of the EM
  const float *theta_lsq, *sigma2;
  double *delta2;
  const double *bcount, *bsq, *mom;
  const int32_t *val_view;
  double *part;          // [2][ST_MAXB]
  int64_t nbt, n_rows;
  EmGeom g;
};
// flat element e -> its view, its (view, batch) row and its column
__device__ __forceinline__ void em_locate(const EmArgs &a, int64_t e, int64_t &row, int64_t &col) {
  const int v = a.val_view[e];
  const int64_t local = e - a.g.val_off[v], nb = a.g.views[v].nb;
  row = a.g.bvb_off[v] + local % nb;
  col = a.g.views[v].c0 + local / nb;
}
// (the flat arrays are whole allocations: every quad of four consecutive elements moves as 128-bit loads and stores)
__global__ __launch_bounds__(256) void k_em_theta(const EmArgs a) {
  __shared__ double sh[4];
  double num = 0.0, den = 0.0;
  const int64_t nq = (a.nbt + 3) / 4;
  for (int64_t q = blockIdx.x * 256ll + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    const int64_t e0 = 4 * q;
    const int cnt = (int)(a.nbt - e0 < 4 ? a.nbt - e0 : 4);
    float lsq[4], tn[4];
    double to[4], t64[4], d2[4], bs[4];
    st_ld4(a.theta64, e0, cnt, true, to);
    st_ld4(a.theta_lsq, e0, cnt, true, lsq);
    st_ld4(a.delta2, e0, cnt, true, d2);
    st_ld4(a.bcount, e0, cnt, true, bs);
    for (int k = 0; k < cnt; ++k) {
      int64_t row, col;
      em_locate(a, e0 + k, row, col);
      const double mean = a.mom[row], var = a.mom[a.n_rows + row], s2 = (double)a.sigma2[col];
      double t = (mean * d2[k] * s2 + (double)lsq[k] * bs[k] * var) / (s2 * d2[k] + bs[k] * var);
      if (!st_finite(t)) t = 0.0;
      t64[k] = t;
      tn[k] = (float)t;
      const double d = t - to[k];
      num += d * d;
      den += t * t;
    }
    st_st4(a.theta64, e0, cnt, true, t64);
    st_st4(a.theta, e0, cnt, true, tn);
  }
  const double sn = block_all_sum_256(num, sh), sd = block_all_sum_256(den, sh);
  if (threadIdx.x == 0) {
    a.part[blockIdx.x] = sn;
    a.part[ST_MAXB + blockIdx.x] = sd;
  }
}
__global__ __launch_bounds__(256) void k_em_diff(const double *__restrict__ part, int nblk, double *__restrict__ out) {
  __shared__ double sh[4];
  double num = 0.0, den = 0.0;
  for (int q = threadIdx.x; q < nblk; q += 256) {
    num += part[q];
    den += part[ST_MAXB + q];
  }
  const double sn = block_all_sum_256(num, sh), sd = block_all_sum_256(den, sh);
  if (threadIdx.x == 0) out[0] = sn / sd;
}
__global__ __launch_bounds__(256) void k_em_delta2(const EmArgs a) {
  const int64_t e0 = 4 * (blockIdx.x * 256ll + threadIdx.x);
  if (e0 >= a.nbt) return;
  const int cnt = (int)(a.nbt - e0 < 4 ? a.nbt - e0 : 4);
  double sq[4], bs[4], d2[4];
  st_ld4(a.bsq, e0, cnt, true, sq);
  st_ld4(a.bcount, e0, cnt, true, bs);
  for (int k = 0; k < cnt; ++k) {
    int64_t row, col;
    em_locate(a, e0 + k, row, col);
    if (!st_finite(sq[k])) sq[k] = 0.0;
    const double alpha = a.mom[2 * a.n_rows + row], beta = a.mom[3 * a.n_rows + row];
    d2[k] = (beta + 0.5 * (sq[k] / (double)a.sigma2[col])) / (alpha + 0.5 * bs[k] - 1.0);
    if (!st_finite(d2[k])) d2[k] = 1.0;
  }
  st_st4(a.delta2, e0, cnt, true, d2);
}

// ---- host side
// dst (f64, owned by the caller) <- n statistics at src (f32, the stats pass's scratch), summed over the ranks in one collective
static int widen_and_reduce(pmf_ctx *c, const float *src, double *dst, int64_t n) {
  k_st_widen<<<st_grid4(n), 256, 0, c->stream>>>(src, dst, n, st_aligned16(src) ? 1 : 0);
  HIPCHK(hipGetLastError());
  if (!comm_active(c) || c->comm.nranks <= 1) return 0;
  Comm &m = c->comm;
  HIPCHK(hipEventRecord(m.ev_loss_ready, c->stream));
  HIPCHK(hipStreamWaitEvent(m.stream, m.ev_loss_ready, 0));
  PMFCHK(comm_allreduce(c, dst, n, true));
  HIPCHK(hipEventRecord(m.ev_loss_done, m.stream));
  HIPCHK(hipStreamWaitEvent(c->stream, m.ev_loss_done, 0));
  return 0;
}

// what every stage entry refuses before anything is launched
static int stage_ready(pmf_ctx *c, const char *who, int64_t M_total) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  if (c->comm.broken) return pmf_fail("%s: the communicator is unusable after a failed call: pmf_comm_destroy it on every rank", who);
  if (M_total < c->M) return pmf_fail("%s: M_total = %lld is below the context's %lld rows", who, (long long)M_total, (long long)c->M);
  PMFCHK(stats_pass_check(c));
  return 0;
}
// Every entry allocates what it owns BEFORE its body: a failed allocation is a plain refusal (nothing launched, no
// collective issued, the communicator stays usable); only the body runs under comm_error_exit.
// the column statistics with X'Y = 0, widened (and reduced) into st (5 N doubles)
static int col_stats_zero(pmf_ctx *c, DevBuf<double> &st) {
  const float *cols = nullptr;
  PMFCHK(stats_pass(c, 0, true, false, &cols, nullptr));
  return widen_and_reduce(c, cols, st.p, 5 * c->N);
}

static int init_logsigma_body(pmf_ctx *c, DevBuf<double> &st) {
  PMFCHK(col_stats_zero(c, st));
  k_stage_logsigma<<<st_grid(c->N), 256, 0, c->stream>>>(st.p, c->P[2].p, c->N);
  HIPCHK(hipGetLastError());
  c->prepared = false;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int pmf_stage_init_logsigma(pmf_ctx *c) {
  PMFCHK(stage_ready(c, "pmf_stage_init_logsigma", c ? c->M : 0));
  DevBuf<double> st;
  PMFCHK(st.alloc((size_t)(5 * c->N), false));
  return comm_error_exit(c, init_logsigma_body(c, st));
}

static int reweight_body(pmf_ctx *c, int64_t M_total, DevBuf<double> &st) {
  k_st_fill<<<st_grid4(c->N), 256, 0, c->stream>>>(c->colw, c->N, 1.f);
  HIPCHK(hipGetLastError());
  c->prepared = false;
  PMFCHK(col_stats_zero(c, st));
  k_stage_reweight<<<st_grid(c->N), 256, 0, c->stream>>>(st.p, c->P[2].p, c->colw, c->N, (double)M_total);
  HIPCHK(hipGetLastError());
  c->prepared = false;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int pmf_stage_reweight_col_losses(pmf_ctx *c, int64_t M_total) {
  PMFCHK(stage_ready(c, "pmf_stage_reweight_col_losses", M_total));
  DevBuf<double> st;
  PMFCHK(st.alloc((size_t)(5 * c->N), false));
  return comm_error_exit(c, reweight_body(c, M_total, st));
}
extern "C" int pmf_get_noise_weights(pmf_ctx *c, float *w) {
  PMFCHK(ctx_bind(c));
  if (!w) return pmf_fail("pmf_get_noise_weights: null output");
  if (c->N == 0 || !c->colw) return pmf_fail("data not set");
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(w, c->colw, sizeof(float) * (size_t)c->N, hipMemcpyDeviceToHost));
  return 0;
}

static int group_weights_body(pmf_ctx *c, int64_t M_total, float *w_out, DevBuf<double> &st, DevBuf<int64_t> &rng,
                              DevBuf<float> &out) {
  const size_t nr = c->noise_s1.size();
  HIPCHK(hipMemcpyAsync(rng.p, c->noise_s1.data(), sizeof(int64_t) * nr, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(rng.p + nr, c->noise_e1.data(), sizeof(int64_t) * nr, hipMemcpyHostToDevice, c->stream));
  PMFCHK(col_stats_zero(c, st));
  k_stage_group<<<(unsigned)nr, 256, 0, c->stream>>>(st.p, c->P[2].p, rng.p, rng.p + nr, c->N, (double)c->K, (double)M_total, out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(w_out, out.p, sizeof(float) * nr, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int pmf_stage_minimal_group_weights(pmf_ctx *c, int64_t M_total, float *w_out) {
  PMFCHK(stage_ready(c, "pmf_stage_minimal_group_weights", M_total));
  if (!w_out) return pmf_fail("pmf_stage_minimal_group_weights: null output");
  if (c->noise_s1.empty()) return pmf_fail("pmf_stage_minimal_group_weights: the noise model is not set");
  const size_t nr = c->noise_s1.size();
  for (size_t r = 0; r < nr; ++r)   // (pmf_set_noise checked them against the N of its time; the kernel indexes N columns)
    if (c->noise_s1[r] < 1 || c->noise_e1[r] > c->N || c->noise_s1[r] > c->noise_e1[r])
      return pmf_fail("pmf_stage_minimal_group_weights: noise range %zu = %lld:%lld does not lie in 1..%lld", r,
                      (long long)c->noise_s1[r], (long long)c->noise_e1[r], (long long)c->N);
  DevBuf<double> st;
  DevBuf<int64_t> rng;
  DevBuf<float> out;
  PMFCHK(st.alloc((size_t)(5 * c->N), false));
  PMFCHK(rng.alloc(2 * nr, false));
  PMFCHK(out.alloc(nr, false));
  return comm_error_exit(c, group_weights_body(c, M_total, w_out, st, rng, out));
}

struct EmBufs {   // what one pmf_stage_theta_delta_em call owns
  DevBuf<float> d_sigma2, theta_lsq;
  DevBuf<double> d_delta2, theta64, bcount, bsq, mom, part, d_diff;
  PinnedBuf<double> h_diff;
  int alloc(int64_t N, int64_t nbt, int64_t n_rows) {
    PMFCHK(d_sigma2.alloc((size_t)N, false));
    PMFCHK(theta_lsq.alloc((size_t)nbt, false));
    PMFCHK(theta64.alloc((size_t)nbt, false));
    PMFCHK(d_delta2.alloc((size_t)nbt, false));
    PMFCHK(bcount.alloc((size_t)nbt, false));
    PMFCHK(bsq.alloc((size_t)nbt, false));
    PMFCHK(mom.alloc((size_t)(4 * n_rows), false));
    PMFCHK(part.alloc(2 * ST_MAXB, false));
    PMFCHK(d_diff.alloc(1, false));
    PMFCHK(h_diff.alloc(1, false));
    return 0;
  }
};
static int em_body(pmf_ctx *c, const pmf_em_opts *o, const float *sigma2, double *delta2, pmf_em_result *res, EmBufs &B) {
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t nbt = c->val_off[c->n_bv], n_rows = c->bvb_off[c->n_bv];
  DevBuf<float> &d_sigma2 = B.d_sigma2, &theta_lsq = B.theta_lsq;
  DevBuf<double> &theta64 = B.theta64, &d_delta2 = B.d_delta2, &bcount = B.bcount, &bsq = B.bsq, &mom = B.mom, &part = B.part, &d_diff = B.d_diff;
  PinnedBuf<double> &h_diff = B.h_diff;
  HIPCHK(hipMemcpyAsync(d_sigma2.p, sigma2, sizeof(float) * (size_t)c->N, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_delta2.p, delta2, sizeof(double) * (size_t)nbt, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(theta_lsq.p, c->P[5].p, sizeof(float) * (size_t)nbt, hipMemcpyDeviceToDevice, c->stream));
  EmArgs a;
  memset(&a, 0, sizeof(a));
  a.theta = c->P[5].p; a.theta64 = theta64.p; a.theta_lsq = theta_lsq.p; a.sigma2 = d_sigma2.p; a.delta2 = d_delta2.p;
  a.bcount = bcount.p; a.bsq = bsq.p; a.mom = mom.p; a.val_view = c->d_val_view; a.part = part.p; a.nbt = nbt; a.n_rows = n_rows;
  a.g.n_bv = c->n_bv;
  for (int v = 0; v < c->n_bv; ++v) a.g.views[v] = c->views[v];
  for (int v = 0; v <= c->n_bv; ++v) { a.g.val_off[v] = c->val_off[v]; a.g.bvb_off[v] = c->bvb_off[v]; }
  const int nblk = (int)std::min<int64_t>(ST_MAXB, st_grid4(nbt));
  k_st_widen<<<st_grid4(nbt), 256, 0, c->stream>>>(c->P[5].p, theta64.p, nbt, st_aligned16(c->P[5].p) ? 1 : 0);
  HIPCHK(hipGetLastError());
  // the batch sizes, once, at the incoming parameters (:332)
  const float *bst = nullptr;
  PMFCHK(stats_pass(c, 1, false, true, nullptr, &bst));
  PMFCHK(widen_and_reduce(c, bst, bcount.p, nbt));
  res->iters = 0;
  res->n_diffs = 0;
  for (int it = 1; it <= o->max_iter; ++it) {
    if (o->update_priors || it == 1) {
      k_em_moments<<<(unsigned)n_rows, 256, 0, c->stream>>>(theta64.p, d_delta2.p, a.g, n_rows, mom.p);
      HIPCHK(hipGetLastError());
    }
    k_em_theta<<<nblk, 256, 0, c->stream>>>(a);
    HIPCHK(hipGetLastError());
    k_em_diff<<<1, 256, 0, c->stream>>>(part.p, nblk, d_diff.p);
    HIPCHK(hipGetLastError());
    c->prepared = false;
    PMFCHK(stats_pass(c, 1, false, true, nullptr, &bst));   // (k_prepare, one k_stats launch with the batch outputs only)
    PMFCHK(widen_and_reduce(c, bst + nbt, bsq.p, nbt));
    k_em_delta2<<<st_grid4(nbt), 256, 0, c->stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_diff.p, d_diff.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double diff = h_diff.p[0];
    res->iters = it;
    if (res->diffs && res->n_diffs < res->diffs_cap) res->diffs[res->n_diffs++] = diff;
    if (o->verbosity > 0) printf("(%d) ||theta - theta'||^2/||theta||^2 : %g\n", it, diff);
    if (diff < o->rtol) break;   // (:367; the same double on every rank)
  }
  HIPCHK(hipMemcpyAsync(delta2, d_delta2.p, sizeof(double) * (size_t)nbt, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}
extern "C" int pmf_stage_theta_delta_em(pmf_ctx *c, const pmf_em_opts *o, const float *sigma2, double *delta2, pmf_em_result *res) {
  PMFCHK(stage_ready(c, "pmf_stage_theta_delta_em", c ? c->M : 0));
  if (!o || !sigma2 || !delta2 || !res) return pmf_fail("pmf_stage_theta_delta_em: null opts / sigma2 / delta2 / result");
  if (c->n_bv == 0 || c->val_off[c->n_bv] == 0) return pmf_fail("pmf_stage_theta_delta_em: the model has no batch views");
  if (o->max_iter < 1) return pmf_fail("pmf_stage_theta_delta_em: max_iter = %d must be at least 1", o->max_iter);
  EmBufs B;
  PMFCHK(B.alloc(c->N, c->val_off[c->n_bv], c->bvb_off[c->n_bv]));
  return comm_error_exit(c, em_body(c, o, sigma2, delta2, res, B));
}
