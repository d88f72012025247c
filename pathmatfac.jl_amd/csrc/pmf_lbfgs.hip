// pmf_lbfgs.hip -- L-BFGS over the factors (X, Y) on the device: fit_lbfgs! (src/fit_lbfgs.jl:170-243) with backtrack!
// (:114-148) and inner_loop! (:151-167), restated in DESIGN.md section 2 ("Deviation 2 / L-BFGS") and section 4.12.
//
// Loss and data gradient come from the library's own passes (eval_full_loss / eval_data_grads, pmf_hip.hip).  What lives
// here is everything over the parameter VECTORS: K_p x M floats of X followed by K_p x N floats of Y, in the padded factor
// layout (pad rows k >= K hold zero in every vector, so they add nothing to any sum).  X and Y are separate allocations, so
// every kernel addresses a vector as two segments (LbVec); the library's own vectors are one allocation cut in two.
//   k_lb_grad   : g = data gradient + gradient of the smooth element-wise regularizer terms (pmf_reg_quad / pmf_reg_ard, the
//                 functions k_reg_step calls); with a previous gradient also y = g - g_old and the partials of <y,s>, <y,y>
//   k_lb_sweep  : one step of the two-loop recursion: applies the pending update to p and accumulates the next product
//   k_lb_trial  : X = X0 + p.X, Y = Y0 + p.Y; on a rejected trial p <- shrinkage * p first
//   k_lb_dot, k_lb_sum2, k_lb_finish : products of handed-in pairs, and the one-workgroup sums behind the host's readback
// Inner products: f32 products accumulated in f64, per thread over its strided elements, lanes by shuffles, the four waves
// in index order, workgroups through a slab of partials that the NEXT kernel's workgroups each sum in index order (the
// CG convention of section 2).  The grid depends on the element count alone, so a product is bitwise the same run to run;
// no atomics, no grid barrier.  The coefficients alpha_k, beta, gamma never reach the host.
#include "pmf_ctx.h"

#define LB_MAX_M 32
#define LB_MAXB 1024                    // workgroups of a vector sweep at most = partials per product
#define LB_SLABS (2 * LB_MAX_M + 3)     // one slab of 3 x LB_MAXB partials per sweep of a recursion (2 m + 1) + k_lb_grad's
#define LB_GRAD_SLAB (LB_SLABS - 1)
#define CF_SY 0                         // device scalars: <s,y> per history slot
#define CF_YY LB_MAX_M                  //                 <y,y> per history slot
#define CF_AL (2 * LB_MAX_M)            //                 alpha per history slot (first loop of the recursion)
#define CF_OUT (3 * LB_MAX_M)           //                 {sy of the newest pair, <p,p>, <p,g>}: the host's readback
#define CF_N (3 * LB_MAX_M + 8)

struct LbVec { float *x, *y; };         // the X segment and the Y segment of one vector

struct LbfgsState {
  int K = 0, m = 0;
  int64_t M = 0, N = 0, nX = 0, nY = 0;
  DevBuf<float> pool;                   // (2 m + 4) vectors: g, g_old, orig, m + 1 step vectors (p and S), m of Y
  DevBuf<double> part;                  // [LB_SLABS][3][LB_MAXB]
  DevBuf<double> cf;                    // [CF_N]
  PinnedBuf<double> h_out;              // pinned [8]
};

void lbfgs_free(pmf_ctx *c) {
  delete c->lbfgs;
  c->lbfgs = nullptr;
}

static int lbfgs_ensure(pmf_ctx *c, int m) {
  LbfgsState *st = c->lbfgs;
  if (st && st->K == c->K && st->M == c->M && st->N == c->N && st->m == m) return 0;
  lbfgs_free(c);
  st = new LbfgsState();
  c->lbfgs = st;
  st->K = c->K; st->M = c->M; st->N = c->N; st->m = m;
  st->nX = (int64_t)c->Kp * c->M;
  st->nY = (int64_t)c->Kp * c->N;
  char what[96];
  snprintf(what, sizeof(what), "pmf_fit_lbfgs: %d vectors of %lld floats (m = %d)", 2 * m + 4, (long long)(st->nX + st->nY), m);
  if (st->pool.alloc((size_t)(2 * m + 4) * (size_t)(st->nX + st->nY), false, what) < 0 ||
      st->part.alloc((size_t)LB_SLABS * 3 * LB_MAXB, true) < 0 || st->cf.alloc((size_t)CF_N, true) < 0 || st->h_out.alloc(8, false) < 0) {
    lbfgs_free(c);   // (sets no error of its own)
    return -1;
  }
  return 0;
}

static inline LbVec lb_vec(const LbfgsState *st, int idx) {
  float *b = st->pool + (size_t)idx * (size_t)(st->nX + st->nY);
  return LbVec{b, b + st->nX};
}
static inline int lb_grid(int64_t n4) { return (int)std::max<int64_t>(1, std::min<int64_t>(LB_MAXB, (n4 + 255) / 256)); }
static inline double *lb_slab(const LbfgsState *st, int t) { return st->part + (size_t)t * 3 * LB_MAXB; }

// ---- device helpers
__device__ __forceinline__ float4 *lb_at(const LbVec &v, int64_t i, int64_t n04) {
  return i < n04 ? reinterpret_cast<float4 *>(v.x) + i : reinterpret_cast<float4 *>(v.y) + (i - n04);
}
// the sum of a slab row of nb partials, by every workgroup alike
__device__ __forceinline__ double lb_slab_sum(const double *row, int nb, double *sh) {
  double v = 0.0;
  for (int q = threadIdx.x; q < nb; q += 256) v += row[q];
  return block_all_sum_256(v, sh);
}
__device__ __forceinline__ void lb_acc(double &d, const float4 &a, const float4 &b) {
  d += (double)(a.x * b.x);
  d += (double)(a.y * b.y);
  d += (double)(a.z * b.z);
  d += (double)(a.w * b.w);
}

// ---- total gradient
struct LbGradArgs {
  StepArgs sx, sy;        // parameter, data gradient and element-wise regularizer of X / Y (step_args_xy)
  LbVec g, gold, s, yv;   // g (out); with have_old: yv = g - gold (out), partials of <yv, s> and <yv, yv>
  int64_t n04, n4;
  int have_old;
  double *part;
};
__global__ __launch_bounds__(256) void k_lb_grad(const LbGradArgs a) {
  __shared__ double sh[4];
  double d0 = 0.0, d1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += stride) {
    const bool isx = i < a.n04;
    const int64_t e = (isx ? i : i - a.n04) * 4;
    const int Kp = a.sx.Kp, K = a.sx.K;       // (the same for X and Y)
    const int k0 = (int)(e % Kp);             // (the four elements share a column: Kp is a multiple of 32)
    const float *rp = isx ? a.sx.p : a.sy.p, *rg = isx ? a.sx.g : a.sy.g, *rwq = isx ? a.sx.wq : a.sy.wq,
                *rcq = isx ? a.sx.cq : a.sy.cq, *rbe = isx ? a.sx.ard_beta : a.sy.ard_beta,
                *ral = isx ? a.sx.ard_alpha : a.sy.ard_alpha;
    const float ard_scale = isx ? a.sx.ard_scale : a.sy.ard_scale;
    const float4 p4 = *reinterpret_cast<const float4 *>(rp + e);
    const float4 gd = *reinterpret_cast<const float4 *>(rg + e);
    float4 w4 = {0.f, 0.f, 0.f, 0.f}, c4 = w4, b4 = w4;
    if (rwq) w4 = *reinterpret_cast<const float4 *>(rwq + e);
    if (rwq && rcq) c4 = *reinterpret_cast<const float4 *>(rcq + e);
    float al = 0.f;
    if (rbe) { b4 = *reinterpret_cast<const float4 *>(rbe + e); al = ral[e / Kp]; }
    const float pv[4] = {p4.x, p4.y, p4.z, p4.w}, gv[4] = {gd.x, gd.y, gd.z, gd.w}, wv[4] = {w4.x, w4.y, w4.z, w4.w},
                cv[4] = {c4.x, c4.y, c4.z, c4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
    float o[4];
    double unused = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float g = 0.f;
      if (k0 + q < K) {
        g = gv[q];
        if (rwq) pmf_reg_quad(pv[q], wv[q], cv[q], g, unused);
        if (rbe) pmf_reg_ard(pv[q], bv[q], al, ard_scale, g, unused);
      }
      o[q] = g;
    }
    const float4 g4 = {o[0], o[1], o[2], o[3]};
    *lb_at(a.g, i, a.n04) = g4;
    if (a.have_old) {
      const float4 go = *lb_at(a.gold, i, a.n04), s4 = *lb_at(a.s, i, a.n04);
      const float4 y4 = {g4.x - go.x, g4.y - go.y, g4.z - go.z, g4.w - go.w};
      *lb_at(a.yv, i, a.n04) = y4;
      lb_acc(d0, y4, s4);
      lb_acc(d1, y4, y4);
    }
  }
  if (a.have_old) {
    const double s0 = block_all_sum_256(d0, sh), s1 = block_all_sum_256(d1, sh);
    if (threadIdx.x == 0) { a.part[blockIdx.x] = s0; a.part[LB_MAXB + blockIdx.x] = s1; }
  }
}

// ---- <a, b> and <a, a> of two handed-in vectors (pmf_debug_lbfgs_direction)
__global__ __launch_bounds__(256) void k_lb_dot(const LbVec va, const LbVec vb, int64_t n04, int64_t n4, double *part) {
  __shared__ double sh[4];
  double d0 = 0.0, d1 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    const float4 x = *lb_at(va, i, n04), y = *lb_at(vb, i, n04);
    lb_acc(d0, x, y);
    lb_acc(d1, x, x);
  }
  const double s0 = block_all_sum_256(d0, sh), s1 = block_all_sum_256(d1, sh);
  if (threadIdx.x == 0) { part[blockIdx.x] = s0; part[LB_MAXB + blockIdx.x] = s1; }
}
// one workgroup: <s,y> and <y,y> of history slot k from the partials of k_lb_grad / k_lb_dot
__global__ __launch_bounds__(256) void k_lb_sum2(const double *part, int nb, double *cf, int k) {
  __shared__ double sh[4];
  const double s0 = lb_slab_sum(part, nb, sh), s1 = lb_slab_sum(part + LB_MAXB, nb, sh);
  if (threadIdx.x == 0) { cf[CF_SY + k] = s0; cf[CF_YY + k] = s1; }
}

// ---- one sweep of the two-loop recursion
struct LbSweepArgs {
  LbVec p, g, u, d;   // p (in / out); g: the gradient (mode 0, and <p,g>); u: the vector of the pending update; d: of the next product
  int64_t n04, n4;
  int mode;           // 0: p = -g    1: p -= alpha u, alpha = <d_prev, p> / sy[ku]    2: as 1, then p *= sy[knew] / yy[knew]
                      // 3: p -= (beta - alpha[ku]) u, beta = <d_prev, p> / sy[ku]
  int ku, knew;       // history slots of u and of the newest pair (-1: none)
  int dots;           // bit 0: <d, p> -> row 0 of part; bit 1: <p,p> -> row 1, <p,g> -> row 2
  int check;          // the reset test of fit_lbfgs! on the device: when sy[knew] > sy_min fails, only mode 0 does anything
  double sy_min;
  const double *prev; // row 0 of the previous sweep's slab
  double *part;
  double *cf;
};
__global__ __launch_bounds__(256) void k_lb_sweep(const LbSweepArgs a) {
  __shared__ double sh[4];
  if (a.mode != 0 && a.check && !(a.cf[CF_SY + a.knew] > a.sy_min)) return;   // (uniform)
  double cd = 0.0;
  float gamma = 1.f;
  if (a.mode != 0) {
    const double S = lb_slab_sum(a.prev, (int)gridDim.x, sh);
    cd = (1.0 / a.cf[CF_SY + a.ku]) * S;
    if (a.mode == 3) cd -= a.cf[CF_AL + a.ku];
    else if (blockIdx.x == 0 && threadIdx.x == 0) a.cf[CF_AL + a.ku] = cd;   // (read by the mode-3 sweep of this slot, a later launch)
    if (a.mode == 2) gamma = (float)(a.cf[CF_SY + a.knew] / a.cf[CF_YY + a.knew]);
  }
  double d0 = 0.0, d1 = 0.0, d2 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += stride) {
    float4 p, g4 = {0.f, 0.f, 0.f, 0.f};
    if (a.mode == 0 || (a.dots & 2)) g4 = *lb_at(a.g, i, a.n04);
    if (a.mode == 0) {
      p = float4{-g4.x, -g4.y, -g4.z, -g4.w};
    } else {
      p = *lb_at(a.p, i, a.n04);
      const float4 u = *lb_at(a.u, i, a.n04);
      // (the reference subtracts Float32 .* Float64 from Float32: one rounding per element)
      p.x = (float)((double)p.x - (double)u.x * cd);
      p.y = (float)((double)p.y - (double)u.y * cd);
      p.z = (float)((double)p.z - (double)u.z * cd);
      p.w = (float)((double)p.w - (double)u.w * cd);
      if (a.mode == 2) { p.x *= gamma; p.y *= gamma; p.z *= gamma; p.w *= gamma; }
    }
    *lb_at(a.p, i, a.n04) = p;
    if (a.dots & 1) lb_acc(d0, *lb_at(a.d, i, a.n04), p);
    if (a.dots & 2) { lb_acc(d1, p, p); lb_acc(d2, p, g4); }
  }
  if (a.dots & 1) {
    const double s = block_all_sum_256(d0, sh);
    if (threadIdx.x == 0) a.part[blockIdx.x] = s;
  }
  if (a.dots & 2) {
    const double s1 = block_all_sum_256(d1, sh), s2 = block_all_sum_256(d2, sh);
    if (threadIdx.x == 0) { a.part[LB_MAXB + blockIdx.x] = s1; a.part[2 * LB_MAXB + blockIdx.x] = s2; }
  }
}
// one workgroup: {sy of the newest pair (1 without one), <p,p>, <p,g>} of the direction the sweeps left -- the steepest
// descent of the first sweep when the reset test failed
__global__ __launch_bounds__(256) void k_lb_finish(const double *slab_last, const double *slab_first, int nb, double *cf,
                                                   int knew, int check, double sy_min) {
  __shared__ double sh[4];
  const bool reset = knew >= 0 && check && !(cf[CF_SY + knew] > sy_min);
  const double *src = reset ? slab_first : slab_last;
  const double pp = lb_slab_sum(src + LB_MAXB, nb, sh), pg = lb_slab_sum(src + 2 * LB_MAXB, nb, sh);
  if (threadIdx.x == 0) {
    cf[CF_OUT + 0] = knew >= 0 ? cf[CF_SY + knew] : 1.0;
    cf[CF_OUT + 1] = pp;
    cf[CF_OUT + 2] = pg;
  }
}

// ---- trial point of the backtrack
struct LbTrialArgs {
  LbVec par, orig, p;
  int64_t n04, n4;
  float scale;      // != 1: p <- scale * p first (f32, rounded every time, as scalar_mult! does)
  int save_orig;    // first trial: orig <- the parameters
  int write_par;    // 0: only rescale p (after the last rejected trial of an exhausted backtrack)
};
__global__ __launch_bounds__(256) void k_lb_trial(const LbTrialArgs a) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += stride) {
    float4 p = *lb_at(a.p, i, a.n04);
    if (a.scale != 1.f) {
      p.x *= a.scale; p.y *= a.scale; p.z *= a.scale; p.w *= a.scale;
      *lb_at(a.p, i, a.n04) = p;
    }
    if (!a.write_par) continue;
    float4 o;
    if (a.save_orig) { o = *lb_at(a.par, i, a.n04); *lb_at(a.orig, i, a.n04) = o; }
    else o = *lb_at(a.orig, i, a.n04);
    *lb_at(a.par, i, a.n04) = float4{o.x + p.x, o.y + p.y, o.z + p.z, o.w + p.w};
  }
}

// ---- host: one direction.  sq / yq: the history newest first (step vectors; slots of the Y vectors, which are also the
// slots of their scalars).  Leaves p and, in cf[CF_OUT..], {sy, <p,p>, <p,g>}.  2 n + 1 sweeps + 1 small launch, no sync.
static int lb_direction(pmf_ctx *c, LbfgsState *st, LbVec p, LbVec g, const std::vector<LbVec> &sq, const std::vector<int> &yq,
                        const std::vector<LbVec> &ybuf, int check, double sy_min) {
  const int n = (int)sq.size();
  const int64_t n04 = st->nX / 4, n4 = (st->nX + st->nY) / 4;
  const int grid = lb_grid(n4);
  LbSweepArgs a;
  memset(&a, 0, sizeof(a));
  a.p = p; a.g = g; a.n04 = n04; a.n4 = n4; a.cf = st->cf; a.check = check; a.sy_min = sy_min;
  a.knew = n > 0 ? yq[0] : -1;
  int t = 0;
  auto launch = [&](int mode, const LbVec *u, int ku, const LbVec *d, int dots) -> int {
    a.mode = mode; a.ku = ku; a.dots = dots;
    a.u = u ? *u : LbVec{nullptr, nullptr};
    a.d = d ? *d : LbVec{nullptr, nullptr};
    a.prev = t > 0 ? lb_slab(st, t - 1) : nullptr;
    a.part = lb_slab(st, t);
    k_lb_sweep<<<grid, 256, 0, c->stream>>>(a);
    HIPCHK(hipGetLastError());
    ++t;
    return 0;
  };
  if (n == 0) {
    PMFCHK(launch(0, nullptr, 0, nullptr, 2));
  } else {
    PMFCHK(launch(0, nullptr, 0, &sq[0], 1 | 2));
    for (int k = 1; k < n; ++k) PMFCHK(launch(1, &ybuf[(size_t)yq[(size_t)k - 1]], yq[(size_t)k - 1], &sq[(size_t)k], 1));
    PMFCHK(launch(2, &ybuf[(size_t)yq[(size_t)n - 1]], yq[(size_t)n - 1], &ybuf[(size_t)yq[(size_t)n - 1]], 1));
    for (int k = n - 1; k >= 0; --k)
      PMFCHK(launch(3, &sq[(size_t)k], yq[(size_t)k], k > 0 ? &ybuf[(size_t)yq[(size_t)k - 1]] : nullptr, k > 0 ? 1 : 2));
  }
  k_lb_finish<<<1, 256, 0, c->stream>>>(lb_slab(st, t - 1), lb_slab(st, 0), grid, st->cf, a.knew, check, sy_min);
  HIPCHK(hipGetLastError());
  return 0;
}

static int lb_refuse(pmf_ctx *c, const char *fn) {
  PMFCHK(check_ready(c));
  if (c->net[0] || c->net[1]) return pmf_fail("%s: a network term is attached to X or Y (not element-wise); L-BFGS takes quadratic and ARD-type terms only", fn);
  if (c->P[0].wl1 || c->P[1].wl1) return pmf_fail("%s: an L1 / SelectiveL1 term is attached to X or Y (not smooth); L-BFGS takes quadratic and ARD-type terms only", fn);
  if (c->comm.nranks > 1) return pmf_fail("%s: the communicator has %d ranks; the inner products are not summed across ranks", fn, c->comm.nranks);
  return 0;
}

extern "C" int pmf_fit_lbfgs(pmf_ctx *c, const pmf_lbfgs_opts *o, pmf_lbfgs_result *res) {
  PMFCHK(ctx_bind(c));
  if (!o || !res) return pmf_fail("pmf_fit_lbfgs: null opts / result");
  PMFCHK(lb_refuse(c, "pmf_fit_lbfgs"));
  if (o->m < 1 || o->m > LB_MAX_M) return pmf_fail("pmf_fit_lbfgs: m = %d out of range (1..%d)", o->m, LB_MAX_M);
  if (!(o->backtrack_shrinkage > 0.0 && o->backtrack_shrinkage < 1.0))
    return pmf_fail("pmf_fit_lbfgs: backtrack_shrinkage = %g out of range (0 < shrinkage < 1)", o->backtrack_shrinkage);
  if (o->max_iter < 0 || o->backtrack_max_iter < 1)
    return pmf_fail("pmf_fit_lbfgs: max_iter = %d (>= 0) / backtrack_max_iter = %d (>= 1) out of range", o->max_iter, o->backtrack_max_iter);
  PMFCHK(lbfgs_ensure(c, o->m));
  LbfgsState *st = c->lbfgs;
  const auto t0 = std::chrono::steady_clock::now();
  const int m = o->m;
  const int64_t n04 = st->nX / 4, n4 = (st->nX + st->nY) / 4;
  const int grid = lb_grid(n4);
  const float shrink = (float)o->backtrack_shrinkage;
  LbVec g = lb_vec(st, 0), gold = lb_vec(st, 1);
  const LbVec orig = lb_vec(st, 2), par = LbVec{c->P[0].p, c->P[1].p};
  std::vector<LbVec> sfree, ybuf, sq;
  std::vector<int> yfree, yq;
  for (int k = 0; k <= m; ++k) sfree.push_back(lb_vec(st, 3 + k));
  for (int k = 0; k < m; ++k) { ybuf.push_back(lb_vec(st, 4 + m + k)); yfree.push_back(m - 1 - k); }
  LbVec p = sfree.back();
  sfree.pop_back();

  res->term_code = PMF_TERM_MAX_EPOCHS;
  res->iters = 0; res->loss_evals = 0; res->grad_evals = 0; res->resets = 0; res->n_trace = 0;
  double L[4];
  PMFCHK(eval_full_loss(c, L));
  res->loss_evals = 1;
  double cur_loss = L[0], final_loss = L[0];
  bool have_old = false;
  int iter = 0;
  while (iter < o->max_iter) {
    if (o->verbosity > 0 && o->print_iter > 0 && iter % o->print_iter == 0) {
      printf("(%d) L-BFGS; Loss=%.8g\n", iter, cur_loss);
      fflush(stdout);
    }
    PMFCHK(eval_data_grads(c));
    res->grad_evals += 1;
    LbGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    step_args_xy(c, 0, &ga.sx);
    step_args_xy(c, 1, &ga.sy);
    ga.g = g; ga.gold = gold; ga.n04 = n04; ga.n4 = n4;
    int knew = -1;
    if (have_old) {
      if ((int)sq.size() >= m) {
        sfree.push_back(sq.back()); sq.pop_back();
        yfree.push_back(yq.back()); yq.pop_back();
      }
      knew = yfree.back();
      yfree.pop_back();
      sq.insert(sq.begin(), p);          // the previous step, as the backtrack left it
      yq.insert(yq.begin(), knew);
      p = sfree.back();
      sfree.pop_back();
      ga.have_old = 1; ga.s = sq[0]; ga.yv = ybuf[(size_t)knew]; ga.part = lb_slab(st, LB_GRAD_SLAB);
    }
    k_lb_grad<<<grid, 256, 0, c->stream>>>(ga);
    HIPCHK(hipGetLastError());
    if (have_old) {
      k_lb_sum2<<<1, 256, 0, c->stream>>>(lb_slab(st, LB_GRAD_SLAB), grid, st->cf, knew);
      HIPCHK(hipGetLastError());
    }
    PMFCHK(lb_direction(c, st, p, g, sq, yq, ybuf, 1, o->sy_min));
    HIPCHK(hipMemcpyAsync(st->h_out, st->cf + CF_OUT, sizeof(double) * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double sy = st->h_out[0], pp = st->h_out[1], pg = st->h_out[2];
    int flags = 0;
    if (knew >= 0 && !(sy > o->sy_min)) {   // the device took p = -g; forget the history, the pair just pushed included
      for (auto &v : sq) sfree.push_back(v);
      for (int k : yq) yfree.push_back(k);
      sq.clear(); yq.clear();
      flags |= 1;
      res->resets += 1;
    }
    double p_norm = std::sqrt(pp);
    if (p_norm == 0.0) {   // stationary start: the reference would spend its 100 trials on an unchanged point
      res->term_code = PMF_TERM_ABS_TOL;
      final_loss = cur_loss;
      break;
    }
    const double dd = pg / p_norm;
    if (dd >= 0) {   // p <- -g; p_norm and dd keep the rejected direction's values (backtrack! :123-128)
      LbSweepArgs a;
      memset(&a, 0, sizeof(a));
      a.p = p; a.g = g; a.n04 = n04; a.n4 = n4; a.cf = st->cf; a.knew = -1; a.part = lb_slab(st, 0);
      k_lb_sweep<<<grid, 256, 0, c->stream>>>(a);
      HIPCHK(hipGetLastError());
      flags |= 2;
    }
    double l1 = INFINITY;
    int trials = 0;
    bool accepted = false;
    LbTrialArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.par = par; ta.orig = orig; ta.p = p; ta.n04 = n04; ta.n4 = n4; ta.write_par = 1;
    for (int bt = 1; bt <= o->backtrack_max_iter; ++bt) {
      ta.scale = bt == 1 ? 1.f : shrink;
      ta.save_orig = bt == 1;
      k_lb_trial<<<grid, 256, 0, c->stream>>>(ta);
      HIPCHK(hipGetLastError());
      PMFCHK(eval_full_loss(c, L));
      res->loss_evals += 1;
      l1 = L[0];
      ++trials;
      if (l1 <= cur_loss + o->c1 * p_norm * dd) { accepted = true; break; }
      p_norm *= o->backtrack_shrinkage;
    }
    if (!accepted) {   // the reference's loop shrinks p once more before it gives up; the parameters stay at the last trial
      ta.scale = shrink; ta.save_orig = 0; ta.write_par = 0;
      k_lb_trial<<<grid, 256, 0, c->stream>>>(ta);
      HIPCHK(hipGetLastError());
      flags |= 4;
    }
    const double new_loss = l1;
    if (o->keep_trace && res->n_trace < res->trace_cap) {
      if (res->loss_trace) res->loss_trace[res->n_trace] = new_loss;
      if (res->trial_trace) res->trial_trace[res->n_trace] = trials;
      if (res->flag_trace) res->flag_trace[res->n_trace] = flags;
      res->n_trace += 1;
    }
    res->iters = iter + 1;
    final_loss = new_loss;
    if (!std::isfinite(new_loss)) { res->term_code = PMF_TERM_NONFINITE; break; }
    const double diff = cur_loss - new_loss;
    if (std::fabs(diff) < o->abs_tol) {
      if (o->verbosity > 0) printf("Loss decrease < %g\n", o->abs_tol);
      res->term_code = PMF_TERM_ABS_TOL;
      break;
    }
    if (std::fabs(diff / new_loss) < o->rel_tol) {
      if (o->verbosity > 0) printf("Relative loss decrease < %g\n", o->rel_tol);
      res->term_code = PMF_TERM_REL_TOL;
      break;
    }
    cur_loss = new_loss;
    std::swap(g, gold);
    have_old = true;
    ++iter;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  res->final_loss = final_loss;
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

// host K x n (n columns) -> a zeroed padded segment
static int lb_upload(pmf_ctx *c, float *dst, const float *src, int64_t n) {
  PMFCHK(memset_now(dst, 0, sizeof(float) * (size_t)c->Kp * (size_t)n));
  HIPCHK(hipMemcpy2D(dst, sizeof(float) * c->Kp, src, sizeof(float) * c->K, sizeof(float) * c->K, (size_t)n, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int pmf_debug_lbfgs_direction(pmf_ctx *c, int n_pairs, const float *sX, const float *sY, const float *yX,
                                         const float *yY, const float *gX, const float *gY, float *pX, float *pY) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0 || c->M <= 0 || c->N <= 0) return pmf_fail("pmf_debug_lbfgs_direction: factors not set");
  if (n_pairs < 0 || n_pairs > LB_MAX_M) return pmf_fail("pmf_debug_lbfgs_direction: n_pairs = %d out of range (0..%d)", n_pairs, LB_MAX_M);
  if (!gX || !gY || !pX || !pY || (n_pairs > 0 && (!sX || !sY || !yX || !yY))) return pmf_fail("pmf_debug_lbfgs_direction: null array");
  PMFCHK(lbfgs_ensure(c, std::max(1, n_pairs)));
  LbfgsState *st = c->lbfgs;
  const int m = st->m;
  const int64_t n04 = st->nX / 4, n4 = (st->nX + st->nY) / 4;
  const int grid = lb_grid(n4);
  const LbVec g = lb_vec(st, 0), p = lb_vec(st, 3 + m);
  std::vector<LbVec> sq, ybuf;
  std::vector<int> yq;
  for (int k = 0; k < m; ++k) ybuf.push_back(lb_vec(st, 4 + m + k));
  PMFCHK(lb_upload(c, g.x, gX, c->M));
  PMFCHK(lb_upload(c, g.y, gY, c->N));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int k = 0; k < n_pairs; ++k) {
    const LbVec s = lb_vec(st, 3 + k);
    PMFCHK(lb_upload(c, s.x, sX + (size_t)k * c->K * c->M, c->M));
    PMFCHK(lb_upload(c, s.y, sY + (size_t)k * c->K * c->N, c->N));
    PMFCHK(lb_upload(c, ybuf[(size_t)k].x, yX + (size_t)k * c->K * c->M, c->M));
    PMFCHK(lb_upload(c, ybuf[(size_t)k].y, yY + (size_t)k * c->K * c->N, c->N));
    sq.push_back(s);
    yq.push_back(k);
    k_lb_dot<<<grid, 256, 0, c->stream>>>(ybuf[(size_t)k], s, n04, n4, lb_slab(st, LB_GRAD_SLAB));
    HIPCHK(hipGetLastError());
    k_lb_sum2<<<1, 256, 0, c->stream>>>(lb_slab(st, LB_GRAD_SLAB), grid, st->cf, k);
    HIPCHK(hipGetLastError());
  }
  PMFCHK(lb_direction(c, st, p, g, sq, yq, ybuf, 0, 0.0));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy2D(pX, sizeof(float) * c->K, p.x, sizeof(float) * c->Kp, sizeof(float) * c->K, (size_t)c->M, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy2D(pY, sizeof(float) * c->K, p.y, sizeof(float) * c->Kp, sizeof(float) * c->K, (size_t)c->N, hipMemcpyDeviceToHost));
  return 0;
}
