// pmf_postprocess.hip -- the factor post-processing stages that fit! runs between the gradient-descent stages (src/fit.jl:
// 504-555; src/regularizers.jl:39-47, 406-420), on the context's resident X (Kp x M) and Y (Kp x N), one C entry each
// (pmf_gram, pmf_stage_lambda_max, pmf_stage_whiten, pmf_stage_rotate_by_svd, pmf_stage_reorder_by_importance).
//
// Every sum is f64 and has a fixed order; no atomics.  The columns of a group are cut at the multiples of PP_CHUNK into
// PIECES; one workgroup owns one piece and adds its columns in index order into a private slab; k_pp_piece_sum adds a
// group's slabs in piece order.  The pieces depend on the ranges alone, not on the grid: an output is bitwise the same run
// to run, and -- after the one all-reduce of the X-side sums -- rank to rank.
//   k_pp_gram<T>     G = P_piece P_piece' (K x K f64), 256 threads x (T x T) accumulators, columns staged through LDS
//   k_pp_diag        the diagonal only: one thread per factor, the same chain of fma's as k_pp_gram's diagonal
//   k_pp_piece_sum   slabs of a group -> its output, piece order
//   k_pp_rotate<R>   P[:, j] <- U' P[:, j], K products per element in f64, one rounding to f32; tile staged in LDS first
//   k_pp_permute     P[r, j] <- P[perm[r], j], tile staged in LDS first
//   k_pp_scale       P[k, j] <- (float)((double)P[k, j] * s_k), / s_k or / c_range(j): a true f64 division; c <= 0 or NaN: 0
//   k_pp_logsigma    logsigma_j <- (float)((double)logsigma_j + log c_range(j)), or (float)-1e9 where c <= 0 or NaN
// The symmetric eigen-decomposition is cyclic Jacobi on the host (pmf_eig.h): the Gram matrix comes down (<= 128 KB), U
// goes up.  Pad rows K..Kp-1 are never read and are written as zero by every kernel that stores whole columns.
#include "pmf_ctx.h"
#include "pmf_eig.h"

#define PP_CHUNK 2048   // columns per piece (a piece never crosses a multiple of it)

struct PpPiece { int64_t j0, j1; };   // columns [j0, j1), 0-based

// ---- Gram
template <int T>
__global__ __launch_bounds__(256) void k_pp_gram(const float *__restrict__ P, int Kp, int K, const PpPiece *__restrict__ pieces,
                                                  double *__restrict__ slab) {
  constexpr int R = 16 * T, CT = 32, LD = R + 4;
  __shared__ __attribute__((aligned(16))) float sh[CT * LD];
  const PpPiece pc = pieces[blockIdx.x];
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  double acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int l = 0; l < T; ++l) acc[i][l] = 0.0;
  for (int64_t j = pc.j0; j < pc.j1; j += CT) {
    const int nc = (int)(pc.j1 - j < CT ? pc.j1 - j : CT);
    for (int e = threadIdx.x; e < CT * R; e += 256) {
      const int cc = e / R, k = e % R;
      sh[cc * LD + k] = (cc < nc && k < K) ? P[(j + cc) * (int64_t)Kp + k] : 0.f;
    }
    __syncthreads();
    for (int cc = 0; cc < nc; ++cc) {
      double av[T], bv[T];
#pragma unroll
      for (int i = 0; i < T; ++i) {
        av[i] = (double)sh[cc * LD + ti * T + i];
        bv[i] = (double)sh[cc * LD + tj * T + i];
      }
#pragma unroll
      for (int i = 0; i < T; ++i)
#pragma unroll
        for (int l = 0; l < T; ++l) acc[i][l] = fma(av[i], bv[l], acc[i][l]);
    }
    __syncthreads();
  }
  double *out = slab + (int64_t)blockIdx.x * K * K;
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int l = 0; l < T; ++l) {
      const int a = ti * T + i, b = tj * T + l;
      if (a < K && b < K) out[a * K + b] = acc[i][l];
    }
}
// rs (may be null): the factor is scaled by rs[k] in f64 before it is squared (whiten!'s rms of the rescaled Y)
__global__ __launch_bounds__(128) void k_pp_diag(const float *__restrict__ P, int Kp, int K, const PpPiece *__restrict__ pieces,
                                                  const double *__restrict__ rs, double *__restrict__ slab) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const PpPiece pc = pieces[blockIdx.x];
  const double s = rs ? rs[k] : 1.0;
  double acc = 0.0;
#pragma unroll 8
  for (int64_t j = pc.j0; j < pc.j1; ++j) {
    double a = (double)P[j * (int64_t)Kp + k];
    if (rs) a *= s;
    acc = fma(a, a, acc);
  }
  slab[(int64_t)blockIdx.x * K + k] = acc;
}
// out[g * E + e] = the slabs gfirst[g] .. gfirst[g + 1] - 1 at e, added in that order (no piece: 0)
__global__ __launch_bounds__(256) void k_pp_piece_sum(const double *__restrict__ slab, const int32_t *__restrict__ gfirst, int64_t E,
                                                       int64_t total, double *__restrict__ out) {
  const int64_t idx = blockIdx.x * 256ll + threadIdx.x;
  if (idx >= total) return;
  const int64_t g = idx / E, e = idx % E;
  const int32_t p0 = gfirst[g], p1 = gfirst[g + 1];
  double s = 0.0;
  if (p0 < p1) s = slab[(int64_t)p0 * E + e];
  for (int32_t p = p0 + 1; p < p1; ++p) s += slab[(int64_t)p * E + e];
  out[idx] = s;
}

// ---- rotation: U is K x K row-major, U[k * K + r] = component k of eigenvector r; out[r, j] = sum_k U[k, r] P[k, j]
template <int R>
__global__ __launch_bounds__(256) void k_pp_rotate(float *__restrict__ P, int Kp, int K, int64_t n, const double *__restrict__ U) {
  constexpr int NG = 256 / R, CJ = 32, TC = NG * CJ, LD = TC + 4;
  __shared__ __attribute__((aligned(16))) float sh[R * LD];
  const int64_t j0 = (int64_t)blockIdx.x * TC;
  const int nc = (int)(n - j0 < TC ? n - j0 : TC);
  for (int e = threadIdx.x; e < TC * R; e += 256) {
    const int cc = e / R, k = e % R;
    sh[k * LD + cc] = (cc < nc && k < K) ? P[(j0 + cc) * (int64_t)Kp + k] : 0.f;
  }
  __syncthreads();   // every column of the tile is in LDS before any of it is written
  const int r = threadIdx.x % R, g = threadIdx.x / R;
  if (r >= Kp) return;
  double acc[CJ];
#pragma unroll
  for (int cc = 0; cc < CJ; ++cc) acc[cc] = 0.0;
  if (r < K) {
    for (int k = 0; k < K; ++k) {
      const double u = U[k * K + r];
      const float4 *row = reinterpret_cast<const float4 *>(&sh[k * LD + g * CJ]);
#pragma unroll
      for (int q = 0; q < CJ / 4; ++q) {
        const float4 v = row[q];
        acc[4 * q + 0] = fma(u, (double)v.x, acc[4 * q + 0]);
        acc[4 * q + 1] = fma(u, (double)v.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fma(u, (double)v.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fma(u, (double)v.w, acc[4 * q + 3]);
      }
    }
  }
#pragma unroll
  for (int cc = 0; cc < CJ; ++cc) {
    const int col = g * CJ + cc;
    if (col < nc) P[(j0 + col) * (int64_t)Kp + r] = (float)acc[cc];   // (pad rows: 0)
  }
}
// ---- row permutation
#define PP_PERM_TC 64
__global__ __launch_bounds__(256) void k_pp_permute(float *__restrict__ P, int Kp, int K, int64_t n, const int32_t *__restrict__ perm) {
  constexpr int LD = 129;
  __shared__ float sh[PP_PERM_TC * LD];
  const int64_t j0 = (int64_t)blockIdx.x * PP_PERM_TC;
  const int nc = (int)(n - j0 < PP_PERM_TC ? n - j0 : PP_PERM_TC);
  for (int e = threadIdx.x; e < PP_PERM_TC * 128; e += 256) {
    const int cc = e >> 7, k = e & 127;
    if (cc < nc && k < K) sh[cc * LD + k] = P[(j0 + cc) * (int64_t)Kp + k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < PP_PERM_TC * 128; e += 256) {
    const int cc = e >> 7, r = e & 127;
    if (cc < nc && r < K) P[(j0 + cc) * (int64_t)Kp + r] = sh[cc * LD + perm[r]];
  }
}
// ---- scaling.  Column ranges [r0, r1) (0-based, ascending, disjoint) with one scalar each; a column in no range keeps c = 1.
__device__ __forceinline__ int pp_find_range(int64_t j, int n_rng, const int64_t *__restrict__ r0, const int64_t *__restrict__ r1) {
  int lo = 0, hi = n_rng;   // first range with r1 > j
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r1[mid] > j) hi = mid; else lo = mid + 1;
  }
  return (lo < n_rng && r0[lo] <= j) ? lo : -1;
}
// one thread per (column, four rows); rs_mode 0: no row scale, 1: multiply by rs[k], 2: divide by rs[k]
__global__ __launch_bounds__(256) void k_pp_scale(float *__restrict__ P, int Kp, int K, int64_t n, const double *__restrict__ rs, int rs_mode,
                                                   int n_rng, const int64_t *__restrict__ r0, const int64_t *__restrict__ r1,
                                                   const double *__restrict__ cs) {
  const int qpc = Kp >> 2;
  const int64_t q = blockIdx.x * 256ll + threadIdx.x;
  if (q >= n * qpc) return;
  const int64_t j = q / qpc;
  const int k0 = 4 * (int)(q % qpc);
  const int rg = n_rng > 0 ? pp_find_range(j, n_rng, r0, r1) : -1;
  const double cval = rg >= 0 ? cs[rg] : 1.0;
  float4 *ptr = reinterpret_cast<float4 *>(P + j * (int64_t)Kp + k0);
  const float4 v = *ptr;
  float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = k0 + i;
    if (k >= K) { o[i] = 0.f; continue; }
    double x = (double)o[i];
    if (rs_mode == 1) x = x * rs[k];
    else if (rs_mode == 2) x = x / rs[k];
    if (rg >= 0) x = (cval > 0.0) ? x / cval : 0.0;
    o[i] = (float)x;
  }
  *ptr = make_float4(o[0], o[1], o[2], o[3]);
}
__global__ __launch_bounds__(256) void k_pp_logsigma(float *__restrict__ ls, int64_t N, int n_rng, const int64_t *__restrict__ r0,
                                                      const int64_t *__restrict__ r1, const double *__restrict__ cs) {
  const int64_t j = blockIdx.x * 256ll + threadIdx.x;
  if (j >= N) return;
  const int rg = pp_find_range(j, n_rng, r0, r1);
  if (rg < 0) return;
  const double cval = cs[rg];
  ls[j] = (cval > 0.0) ? (float)((double)ls[j] + log(cval)) : (float)-1e9;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// host-clock seconds of the phases of the last call, each closed by a stream synchronisation: [0] the Gram / diagonal passes
// with their collective and download, [1] the eigen-solver, [2] the kernels that rewrite X, Y and logsigma
// (pmf_debug_postprocess_times; scripts/kbench_postprocess.py)
struct PpClock {
  pmf_ctx *c;
  std::chrono::steady_clock::time_point t;
  explicit PpClock(pmf_ctx *c_) : c(c_), t(std::chrono::steady_clock::now()) { c->pp_seconds[0] = c->pp_seconds[1] = c->pp_seconds[2] = 0.0; }
  void lap(int phase) {
    const auto now = std::chrono::steady_clock::now();
    c->pp_seconds[phase] += std::chrono::duration<double>(now - t).count();
    t = now;
  }
};
extern "C" int pmf_debug_postprocess_times(pmf_ctx *c, double *gram_s, double *eig_s, double *apply_s) {
  if (!c) return pmf_fail("null context");
  if (gram_s) *gram_s = c->pp_seconds[0];
  if (eig_s) *eig_s = c->pp_seconds[1];
  if (apply_s) *apply_s = c->pp_seconds[2];
  return 0;
}

static inline unsigned pp_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + 255) / 256); }

// what every entry refuses before anything is launched
static int pp_ready(pmf_ctx *c, const char *who) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0) return pmf_fail("%s: factors not set", who);
  PMFCHK(check_ready(c));
  if (c->comm.broken) return pmf_fail("%s: the communicator is unusable after a failed call: pmf_comm_destroy it on every rank", who);
  return 0;
}
// 1-based inclusive ranges inside 1..limit, ascending and disjoint (gaps allowed).  allow_empty: start1 .. start1 - 1 is a
// group without columns (a row-sharded group with no local rows).
static int pp_check_ranges(const char *who, int n, const int64_t *s1, const int64_t *e1, int64_t limit, bool allow_empty) {
  if (n < 1) return pmf_fail("%s: n_groups = %d must be at least 1", who, n);
  if (!s1 || !e1) return pmf_fail("%s: null range pointer", who);
  int64_t prev = 0;
  for (int g = 0; g < n; ++g) {
    const bool empty = allow_empty && e1[g] == s1[g] - 1;
    if (s1[g] < 1 || e1[g] > limit || (!empty && s1[g] > e1[g]) || (empty && s1[g] > limit + 1))
      return pmf_fail("%s: range %d = %lld:%lld does not lie in 1..%lld", who, g, (long long)s1[g], (long long)e1[g], (long long)limit);
    if (s1[g] <= prev)
      return pmf_fail("%s: range %d = %lld:%lld overlaps or precedes the range before it (ranges must be disjoint and ascending)", who, g,
                      (long long)s1[g], (long long)e1[g]);
    prev = std::max(prev, e1[g]);
  }
  return 0;
}

// One Gram (or diagonal) computation: the pieces of its groups, its slabs and its output, all allocated by plan()
struct GramPlan {
  int n_groups = 0, K = 0;
  bool diag = false;
  int64_t E = 0;   // outputs per group
  std::vector<PpPiece> pieces;
  std::vector<int32_t> gfirst;
  DevBuf<PpPiece> d_pieces;
  DevBuf<int32_t> d_gfirst;
  DevBuf<double> slab, out;
  int plan(int K_, int n, const int64_t *s1, const int64_t *e1, bool diag_) {
    n_groups = n; K = K_; diag = diag_;
    E = diag ? K : (int64_t)K * K;
    gfirst.assign((size_t)n + 1, 0);
    for (int g = 0; g < n; ++g) {
      gfirst[g] = (int32_t)pieces.size();
      for (int64_t j = s1[g] - 1; j < e1[g];) {
        const int64_t stop = std::min<int64_t>(e1[g], (j / PP_CHUNK + 1) * PP_CHUNK);
        pieces.push_back({j, stop});
        j = stop;
      }
    }
    gfirst[n] = (int32_t)pieces.size();
    PMFCHK(d_pieces.alloc(pieces.size(), false));
    PMFCHK(d_gfirst.alloc(gfirst.size(), false));
    PMFCHK(slab.alloc(pieces.size() * (size_t)E, false));
    PMFCHK(out.alloc((size_t)n * (size_t)E, false));
    return 0;
  }
};
// the groups' Gram matrices (diagonals) of P (Kp x n) into g.out, on the stream
static int gram_launch(pmf_ctx *c, const float *P, GramPlan &g, const double *rs = nullptr) {
  const unsigned np = (unsigned)g.pieces.size();
  HIPCHK(hipMemcpyAsync(g.d_gfirst.p, g.gfirst.data(), sizeof(int32_t) * g.gfirst.size(), hipMemcpyHostToDevice, c->stream));
  if (np > 0) {
    HIPCHK(hipMemcpyAsync(g.d_pieces.p, g.pieces.data(), sizeof(PpPiece) * np, hipMemcpyHostToDevice, c->stream));
    if (g.diag) k_pp_diag<<<np, 128, 0, c->stream>>>(P, c->Kp, c->K, g.d_pieces.p, rs, g.slab.p);
    else if (c->K <= 32) k_pp_gram<2><<<np, 256, 0, c->stream>>>(P, c->Kp, c->K, g.d_pieces.p, g.slab.p);
    else if (c->K <= 64) k_pp_gram<4><<<np, 256, 0, c->stream>>>(P, c->Kp, c->K, g.d_pieces.p, g.slab.p);
    else k_pp_gram<8><<<np, 256, 0, c->stream>>>(P, c->Kp, c->K, g.d_pieces.p, g.slab.p);
    HIPCHK(hipGetLastError());
  }
  const int64_t total = (int64_t)g.n_groups * g.E;
  k_pp_piece_sum<<<pp_grid(total), 256, 0, c->stream>>>(g.slab.p, g.d_gfirst.p, g.E, total, g.out.p);
  HIPCHK(hipGetLastError());
  return 0;
}
// in-place sum over the ranks of n doubles at p (device), ONE collective, ordered after the stream's work and before its next
static int pp_allreduce(pmf_ctx *c, double *p, int64_t n) {
  if (!comm_active(c) || c->comm.nranks <= 1) return 0;
  Comm &m = c->comm;
  HIPCHK(hipEventRecord(m.ev_loss_ready, c->stream));
  HIPCHK(hipStreamWaitEvent(m.stream, m.ev_loss_ready, 0));
  PMFCHK(comm_allreduce(c, p, n, true));
  HIPCHK(hipEventRecord(m.ev_loss_done, m.stream));
  HIPCHK(hipStreamWaitEvent(c->stream, m.ev_loss_done, 0));
  return 0;
}
static int pp_download(pmf_ctx *c, double *dst, const double *src, size_t n) {
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
static int rotate_launch(pmf_ctx *c, float *P, int64_t n, const double *U) {
  if (c->K <= 32) k_pp_rotate<32><<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(P, c->Kp, c->K, n, U);
  else if (c->K <= 64) k_pp_rotate<64><<<(unsigned)((n + 127) / 128), 256, 0, c->stream>>>(P, c->Kp, c->K, n, U);
  else k_pp_rotate<128><<<(unsigned)((n + 63) / 64), 256, 0, c->stream>>>(P, c->Kp, c->K, n, U);
  HIPCHK(hipGetLastError());
  return 0;
}
static int eig_or_fail(const char *who, const double *G, int K, double *lam, double *U) {
  const int rc = pmf_eig_sym(G, K, lam, U, nullptr);
  if (rc == -2) return pmf_fail("%s: the Jacobi eigen-solver did not converge in %d sweeps (a non-finite Gram matrix?)", who, PMF_EIG_MAX_SWEEPS);
  if (rc != 0) return pmf_fail("%s: bad argument to the eigen-solver", who);
  return 0;
}

// ---- pmf_gram / pmf_stage_lambda_max
static int gram_body(pmf_ctx *c, int which, GramPlan &g, double *out, size_t n_out) {
  PpClock clk(c);
  PMFCHK(gram_launch(c, c->P[which].p, g));
  if (which == 0) PMFCHK(pp_allreduce(c, g.out.p, (int64_t)n_out));
  PMFCHK(pp_download(c, out, g.out.p, n_out));
  clk.lap(0);
  return 0;
}
static int gram_args(pmf_ctx *c, const char *who, int which, int n_groups, const int64_t *s1, const int64_t *e1) {
  PMFCHK(pp_ready(c, who));
  if (which != 0 && which != 1) return pmf_fail("%s: which = %d: 0 (X) or 1 (Y)", who, which);
  return pp_check_ranges(who, n_groups, s1, e1, which == 0 ? c->M : c->N, true);
}
extern "C" int pmf_gram(pmf_ctx *c, int which, int n_groups, const int64_t *starts1, const int64_t *stops1, int diag_only, double *out) {
  PMFCHK(gram_args(c, "pmf_gram", which, n_groups, starts1, stops1));
  if (!out) return pmf_fail("pmf_gram: null output");
  GramPlan g;
  PMFCHK(g.plan(c->K, n_groups, starts1, stops1, diag_only != 0));
  return comm_error_exit(c, gram_body(c, which, g, out, (size_t)n_groups * (size_t)g.E));
}
static int lambda_max_body(pmf_ctx *c, int which, GramPlan &g, std::vector<double> &G, std::vector<double> &lam, double *lam_out) {
  PMFCHK(gram_body(c, which, g, G.data(), G.size()));
  const double gram_s = c->pp_seconds[0];
  PpClock clk(c);
  for (int i = 0; i < g.n_groups; ++i) {
    PMFCHK(eig_or_fail("pmf_stage_lambda_max", G.data() + (size_t)i * g.E, c->K, lam.data(), nullptr));
    lam_out[i] = lam[0];
  }
  clk.lap(1);
  c->pp_seconds[0] = gram_s;
  return 0;
}
extern "C" int pmf_stage_lambda_max(pmf_ctx *c, int which, int n_groups, const int64_t *starts1, const int64_t *stops1, double *lam_out) {
  PMFCHK(gram_args(c, "pmf_stage_lambda_max", which, n_groups, starts1, stops1));
  if (!lam_out) return pmf_fail("pmf_stage_lambda_max: null output");
  GramPlan g;
  PMFCHK(g.plan(c->K, n_groups, starts1, stops1, false));
  std::vector<double> G((size_t)n_groups * (size_t)g.E), lam((size_t)c->K);
  return comm_error_exit(c, lambda_max_body(c, which, g, G, lam, lam_out));
}

// ---- pmf_stage_whiten
struct WhitenBufs {
  GramPlan gx, gy;
  DevBuf<double> d_xr, d_cs;
  DevBuf<int64_t> d_rng;   // [r0 | r1], 0-based half-open
  std::vector<double> xr, yd, cs;
  std::vector<int64_t> rng;
};
static int whiten_body(pmf_ctx *c, int64_t M_total, int n_views, double *x_rms_out, double *y_rms_max_out, WhitenBufs &B) {
  const int K = c->K;
  PpClock clk(c);
  // x_rms = sqrt(sum_i X[k, i]^2 / M_total)                                   (:505)
  PMFCHK(gram_launch(c, c->P[0].p, B.gx));
  PMFCHK(pp_allreduce(c, B.gx.out.p, K));
  PMFCHK(pp_download(c, B.xr.data(), B.gx.out.p, (size_t)K));
  for (int k = 0; k < K; ++k) B.xr[k] = std::sqrt(B.xr[k] / (double)M_total);
  HIPCHK(hipMemcpyAsync(B.d_xr.p, B.xr.data(), sizeof(double) * (size_t)K, hipMemcpyHostToDevice, c->stream));
  // per view: c = max_k rms of the rescaled Y's row k over the view (:513, :517), from the f64 products Y * x_rms
  PMFCHK(gram_launch(c, c->P[1].p, B.gy, B.d_xr.p));
  PMFCHK(pp_download(c, B.yd.data(), B.gy.out.p, (size_t)n_views * (size_t)K));
  for (int v = 0; v < n_views; ++v) {
    const double nv = (double)(B.rng[(size_t)n_views + v] - B.rng[v]);
    double cmax = -1.0;
    for (int k = 0; k < K; ++k) {
      const double r = std::sqrt(B.yd[(size_t)v * K + k] / nv);
      if (r != r) { cmax = r; break; }   // (a NaN rms makes the maximum NaN, as on the host)
      cmax = std::max(cmax, r);
    }
    B.cs[v] = cmax;
  }
  clk.lap(0);
  HIPCHK(hipMemcpyAsync(B.d_cs.p, B.cs.data(), sizeof(double) * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(B.d_rng.p, B.rng.data(), sizeof(int64_t) * 2 * (size_t)n_views, hipMemcpyHostToDevice, c->stream));
  const int64_t *r0 = B.d_rng.p, *r1 = B.d_rng.p + n_views;
  // X /= x_rms (:506), Y *= x_rms (:507): stored as f32 here, as the host's arrays are
  k_pp_scale<<<pp_grid(c->M * (c->Kp / 4)), 256, 0, c->stream>>>(c->P[0].p, c->Kp, K, c->M, B.d_xr.p, 2, 0, nullptr, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  k_pp_scale<<<pp_grid(c->N * (c->Kp / 4)), 256, 0, c->stream>>>(c->P[1].p, c->Kp, K, c->N, B.d_xr.p, 1, 0, nullptr, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  // c > 0: Y[:, view] /= c, logsigma[view] += log c (:519-520); else Y[:, view] = 0, logsigma[view] = -1e9 (:522-523)
  k_pp_scale<<<pp_grid(c->N * (c->Kp / 4)), 256, 0, c->stream>>>(c->P[1].p, c->Kp, K, c->N, nullptr, 0, n_views, r0, r1, B.d_cs.p);
  HIPCHK(hipGetLastError());
  k_pp_logsigma<<<pp_grid(c->N), 256, 0, c->stream>>>(c->P[2].p, c->N, n_views, r0, r1, B.d_cs.p);
  HIPCHK(hipGetLastError());
  c->prepared = false;
  HIPCHK(hipStreamSynchronize(c->stream));
  clk.lap(2);
  if (x_rms_out) memcpy(x_rms_out, B.xr.data(), sizeof(double) * (size_t)K);
  if (y_rms_max_out) memcpy(y_rms_max_out, B.cs.data(), sizeof(double) * (size_t)n_views);
  return 0;
}
extern "C" int pmf_stage_whiten(pmf_ctx *c, int64_t M_total, int n_views, const int64_t *starts1, const int64_t *stops1,
                                double *x_rms_out, double *y_rms_max_out) {
  PMFCHK(pp_ready(c, "pmf_stage_whiten"));
  if (M_total < c->M) return pmf_fail("pmf_stage_whiten: M_total = %lld is below the context's %lld rows", (long long)M_total, (long long)c->M);
  PMFCHK(pp_check_ranges("pmf_stage_whiten", n_views, starts1, stops1, c->N, false));
  WhitenBufs B;
  const int64_t one = 1, all = c->M;
  PMFCHK(B.gx.plan(c->K, 1, &one, &all, true));
  PMFCHK(B.gy.plan(c->K, n_views, starts1, stops1, true));
  PMFCHK(B.d_xr.alloc((size_t)c->K, false));
  PMFCHK(B.d_cs.alloc((size_t)n_views, false));
  PMFCHK(B.d_rng.alloc(2 * (size_t)n_views, false));
  B.xr.assign((size_t)c->K, 0.0);
  B.yd.assign((size_t)n_views * (size_t)c->K, 0.0);
  B.cs.assign((size_t)n_views, 0.0);
  B.rng.resize(2 * (size_t)n_views);
  for (int v = 0; v < n_views; ++v) { B.rng[v] = starts1[v] - 1; B.rng[(size_t)n_views + v] = stops1[v]; }
  return comm_error_exit(c, whiten_body(c, M_total, n_views, x_rms_out, y_rms_max_out, B));
}

// ---- pmf_stage_rotate_by_svd
struct RotateBufs {
  GramPlan g;
  DevBuf<double> d_U;
  std::vector<double> G, lam, U;
};
static int rotate_body(pmf_ctx *c, double *sing_out, double *U_out, RotateBufs &B) {
  const int K = c->K;
  PpClock clk(c);
  PMFCHK(gram_launch(c, c->P[1].p, B.g));
  PMFCHK(pp_download(c, B.G.data(), B.g.out.p, (size_t)K * K));
  clk.lap(0);
  PMFCHK(eig_or_fail("pmf_stage_rotate_by_svd", B.G.data(), K, B.lam.data(), B.U.data()));
  clk.lap(1);
  HIPCHK(hipMemcpyAsync(B.d_U.p, B.U.data(), sizeof(double) * (size_t)K * K, hipMemcpyHostToDevice, c->stream));
  PMFCHK(rotate_launch(c, c->P[1].p, c->N, B.d_U.p));   // Y <- U'Y = S Vt   (:538)
  PMFCHK(rotate_launch(c, c->P[0].p, c->M, B.d_U.p));   // X' <- X' U       (:541)
  HIPCHK(hipStreamSynchronize(c->stream));
  clk.lap(2);
  if (sing_out)
    for (int k = 0; k < K; ++k) sing_out[k] = std::sqrt(std::max(B.lam[k], 0.0));
  if (U_out) memcpy(U_out, B.U.data(), sizeof(double) * (size_t)K * K);
  return 0;
}
extern "C" int pmf_stage_rotate_by_svd(pmf_ctx *c, double *sing_out, double *U_out) {
  PMFCHK(pp_ready(c, "pmf_stage_rotate_by_svd"));
  RotateBufs B;
  const int64_t one = 1, all = c->N;
  PMFCHK(B.g.plan(c->K, 1, &one, &all, false));
  PMFCHK(B.d_U.alloc((size_t)c->K * c->K, false));
  B.G.assign((size_t)c->K * c->K, 0.0);
  B.U.assign((size_t)c->K * c->K, 0.0);
  B.lam.assign((size_t)c->K, 0.0);
  return comm_error_exit(c, rotate_body(c, sing_out, U_out, B));
}

// ---- pmf_stage_reorder_by_importance
struct ReorderBufs {
  GramPlan g;
  DevBuf<int32_t> d_perm;
  std::vector<double> ssq;
  std::vector<int32_t> perm;
};
static int reorder_body(pmf_ctx *c, int32_t *perm_out, ReorderBufs &B) {
  const int K = c->K;
  PpClock clk(c);
  PMFCHK(gram_launch(c, c->P[1].p, B.g));
  PMFCHK(pp_download(c, B.ssq.data(), B.g.out.p, (size_t)K));
  clk.lap(0);
  for (int k = 0; k < K; ++k) B.perm[k] = k;
  // sortperm(rev = true) is stable (:549); a NaN sum goes last, as numpy's argsort of the negated sums puts it
  std::stable_sort(B.perm.begin(), B.perm.end(), [&](int32_t a, int32_t b) {
    const double x = B.ssq[a], y = B.ssq[b];
    if (x != x || y != y) return y != y && x == x;
    return x > y;
  });
  HIPCHK(hipMemcpyAsync(B.d_perm.p, B.perm.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, c->stream));
  k_pp_permute<<<(unsigned)((c->M + PP_PERM_TC - 1) / PP_PERM_TC), 256, 0, c->stream>>>(c->P[0].p, c->Kp, K, c->M, B.d_perm.p);
  HIPCHK(hipGetLastError());
  k_pp_permute<<<(unsigned)((c->N + PP_PERM_TC - 1) / PP_PERM_TC), 256, 0, c->stream>>>(c->P[1].p, c->Kp, K, c->N, B.d_perm.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  clk.lap(2);
  if (perm_out) memcpy(perm_out, B.perm.data(), sizeof(int32_t) * (size_t)K);
  return 0;
}
extern "C" int pmf_stage_reorder_by_importance(pmf_ctx *c, int32_t *perm_out) {
  PMFCHK(pp_ready(c, "pmf_stage_reorder_by_importance"));
  ReorderBufs B;
  const int64_t one = 1, all = c->N;
  PMFCHK(B.g.plan(c->K, 1, &one, &all, true));
  PMFCHK(B.d_perm.alloc((size_t)c->K, false));
  B.ssq.assign((size_t)c->K, 0.0);
  B.perm.assign((size_t)c->K, 0);
  return comm_error_exit(c, reorder_body(c, perm_out, B));
}
