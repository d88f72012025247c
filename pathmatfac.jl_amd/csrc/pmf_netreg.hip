// pmf_netreg.hip -- the pathway-graph regularizers on the device: NetworkRegularizer (src/regularizers.jl:169-338) and the
// dense weights of L1Regularizer / SelectiveL1Reg (:60-163).
#include "pmf_ctx.h"

// ------------------------------------------------------------------------------------------------
// NetworkRegularizer call + rrule (src/regularizers.jl:249-306).  For the parameter P (K x n) and per factor k the blocks
// AA_k, AB_k, BB_k with p_k = P[k, :]:
//     t_k = AB_k' p_k,   u_k = -BB_k^{-1} t_k,
//     loss = sum_k 0.5 p_k'AA_k p_k + t_k'u_k + 0.5 u_k'BB_k u_k,     P_bar[k, :] = AA_k p_k + AB_k u_k
// Three kernels per evaluation, no atomics, every sum in a fixed order:
//   k_netreg_transpose : PT[k][i] = P[i * Kp + k].  P keeps the factor index contiguous, so a gather of p_k[j] from it
//                        would use 4 bytes of every line it touches; the factor-major copy (n x 4 B per factor) is made
//                        once per evaluation and every gather below reads it.
//   k_netreg_solve     : one workgroup per factor.  t_k by a CSR product with AB_k', then the whole conjugate-gradient
//                        loop inside the workgroup: t, u, r, d, BB d in LDS while v_k <= NETREG_V_LDS, in a global
//                        workspace beyond that (same code, the vectors' base pointers differ).  Dot products: every
//                        thread sums its strided elements in f64, the wave by shuffles, the four waves in index order.
//                        The vectors are f32; the row sums of the sparse products are accumulated in f64 too and
//                        rounded once (a hub row has hundreds of terms).
//                        Writes u_k, the iteration count and t'u + 0.5 u'BB u (f64).
//   k_netreg_grad      : (row block, factor): p * (AA_k p_k + AB_k u_k) per row into a buffer in P's own layout that
//                        k_reg_step<true> adds to the gradient, and p * 0.5 p'AA p summed in f64 into one loss partial per
//                        workgroup (the factor's first workgroup adds the solve's p * (t'u + 0.5 u'BB u)).
// The stopping rule is the library's own (Krylov.jl's is not reproduced): stop at |r| <= 1e-6 |t_k| or after 2 v_k
// iterations, t_k = 0 gives u_k = 0; the warm start is the previous u_k.
// ------------------------------------------------------------------------------------------------
#define NETREG_V_LDS 4096       // largest v_k whose five CG vectors live in LDS (5 x 4096 x 4 B = 80 KiB of the CU's 160)
#define NETREG_SLOTS 512        // loss partials (= gradient workgroups) a network term may use of its slab's REG_SLOTS
#define NETREG_RTOL 1e-6

__global__ __launch_bounds__(256) void k_netreg_transpose(const float *__restrict__ P, float *__restrict__ PT, int64_t n, int Kp, int K) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int64_t i0 = (int64_t)blockIdx.x * 32;
  const int k0 = blockIdx.y * 32;
  for (int r = ty; r < 32; r += 8) {
    const int64_t i = i0 + r;
    tile[r][tx] = i < n ? P[i * Kp + k0 + tx] : 0.f;        // (k0 + tx < Kp: Kp is a multiple of 32)
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int k = k0 + r;
    const int64_t i = i0 + tx;
    if (k < K && i < n) PT[(int64_t)k * n + i] = tile[tx][r];
  }
}

struct NetSolveArgs {
  const float *PT;
  const int64_t *voff, *abt_rp, *bb_rp;
  const int32_t *abt_col, *bb_col;
  const float *abt_val, *bb_val;
  float *u, *work;
  int32_t *iters;
  double *uloss;
  int64_t n;
};

__global__ __launch_bounds__(256) void k_netreg_solve(const NetSolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_nr[];
  __shared__ double sh[4];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int64_t v0 = a.voff[k];
  const int v = (int)(a.voff[k + 1] - v0);
  if (v == 0) {                                   // every node of this factor's graph is observed
    if (tid == 0) { a.iters[k] = 0; a.uloss[k] = 0.0; }
    return;
  }
  const bool lds = v <= NETREG_V_LDS;
  float *ug = a.u + v0;
  float *base = lds ? reinterpret_cast<float *>(smem_nr) : a.work + 4 * v0;
  float *t = base, *r = base + v, *d = base + 2 * (int64_t)v, *q = base + 3 * (int64_t)v;
  float *u = lds ? base + 4 * (int64_t)v : ug;
  const float *pk = a.PT + (int64_t)k * a.n;
  const int64_t *trp = a.abt_rp + v0 + k, *brp = a.bb_rp + v0 + k;

  // t = AB' p_k ; |t|^2
  double acc = 0.0;
  for (int i = tid; i < v; i += 256) {
    double sd = 0.0;
    for (int64_t e = trp[i]; e < trp[i + 1]; ++e) sd += (double)a.abt_val[e] * (double)pk[a.abt_col[e]];
    const float s = (float)sd;
    t[i] = s;
    acc += (double)s * (double)s;
    if (lds) u[i] = ug[i];
  }
  const double tt = block_all_sum_256(acc, sh);       // (its barriers also publish t and u)
  if (tt == 0.0) {                                // t = 0: u = 0 exactly
    for (int i = tid; i < v; i += 256) ug[i] = 0.f;
    if (tid == 0) { a.iters[k] = 0; a.uloss[k] = 0.0; }
    return;
  }
  // r = -t - BB u ; d = r
  acc = 0.0;
  for (int i = tid; i < v; i += 256) {
    double s = 0.0;
    for (int64_t e = brp[i]; e < brp[i + 1]; ++e) s += (double)a.bb_val[e] * (double)u[a.bb_col[e]];
    const float ri = (float)(-(double)t[i] - s);
    r[i] = ri;
    d[i] = ri;
    acc += (double)ri * (double)ri;
  }
  double rr = block_all_sum_256(acc, sh);
  const double stop2 = (NETREG_RTOL * NETREG_RTOL) * tt;
  int it = 0;
  while (rr > stop2 && it < 2 * v) {
    acc = 0.0;
    for (int i = tid; i < v; i += 256) {
      double sd = 0.0;
      for (int64_t e = brp[i]; e < brp[i + 1]; ++e) sd += (double)a.bb_val[e] * (double)d[a.bb_col[e]];
      const float s = (float)sd;
      q[i] = s;
      acc += (double)d[i] * (double)s;
    }
    const double dq = block_all_sum_256(acc, sh);
    if (!(dq > 0.0)) break;                       // (BB is positive definite: only reachable with a malformed matrix)
    const float alpha = (float)(rr / dq);
    acc = 0.0;
    for (int i = tid; i < v; i += 256) {
      u[i] += alpha * d[i];
      const float ri = r[i] - alpha * q[i];
      r[i] = ri;
      acc += (double)ri * (double)ri;
    }
    const double rr_new = block_all_sum_256(acc, sh);
    const float beta = (float)(rr_new / rr);
    for (int i = tid; i < v; i += 256) d[i] = r[i] + beta * d[i];
    rr = rr_new;
    ++it;
    __syncthreads();
  }
  // t'u + 0.5 u'BB u, and u back to global memory
  acc = 0.0;
  for (int i = tid; i < v; i += 256) {
    double s = 0.0;
    for (int64_t e = brp[i]; e < brp[i + 1]; ++e) s += (double)a.bb_val[e] * (double)u[a.bb_col[e]];
    const double ui = (double)u[i];
    acc += (double)t[i] * ui + 0.5 * ui * s;
  }
  const double ul = block_all_sum_256(acc, sh);
  if (lds)
    for (int i = tid; i < v; i += 256) ug[i] = u[i];
  if (tid == 0) { a.iters[k] = it; a.uloss[k] = ul; }
}

struct NetGradArgs {
  const float *PT, *u;
  const int64_t *voff, *aa_rp, *ab_rp;
  const int32_t *aa_col, *ab_col;
  const float *aa_val, *ab_val;
  const double *uloss;
  float *grad;
  double *reg_partial;
  int64_t n;
  int Kp, rb;
  float p;
};

// blockIdx.x = k * rb + b: rows b * 256 + tid, stepping rb * 256
__global__ __launch_bounds__(256) void k_netreg_grad(const NetGradArgs a) {
  __shared__ double sh[4];
  const int k = blockIdx.x / a.rb, b = blockIdx.x % a.rb;
  const float *pk = a.PT + (int64_t)k * a.n;
  const float *uk = a.u + a.voff[k];
  const int64_t *arp = a.aa_rp + (int64_t)k * (a.n + 1), *brp = a.ab_rp + (int64_t)k * (a.n + 1);
  double lacc = 0.0;
  for (int64_t i = (int64_t)b * 256 + threadIdx.x; i < a.n; i += (int64_t)a.rb * 256) {
    double s = 0.0;
    for (int64_t e = arp[i]; e < arp[i + 1]; ++e) s += (double)a.aa_val[e] * (double)pk[a.aa_col[e]];
    lacc += 0.5 * (double)pk[i] * s;
    for (int64_t e = brp[i]; e < brp[i + 1]; ++e) s += (double)a.ab_val[e] * (double)uk[a.ab_col[e]];
    a.grad[i * a.Kp + k] = (float)((double)a.p * s);
  }
  const double s = block_reduce_sum(lacc, sh);
  if (threadIdx.x == 0) a.reg_partial[blockIdx.x] = (double)a.p * (s + (b == 0 ? a.uloss[k] : 0.0));
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
void netreg_free(pmf_ctx *c, int which) {
  NetReg *r = c->net[which];
  if (!r) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete r;
  c->net[which] = nullptr;
}

int netreg_eval(pmf_ctx *c, int which, int *reg_count) {
  NetReg *r = c->net[which];
  if (!r) return 0;
  const int grid = r->K * r->rb;
  if (*reg_count + grid > REG_SLOTS) return pmf_fail("internal: regularizer partial slab overflow (network term)");
  k_netreg_transpose<<<dim3((unsigned)((r->n + 31) / 32), (unsigned)((r->K + 31) / 32)), 256, 0, c->stream>>>(c->P[which].p, r->PT, r->n, c->Kp, r->K);
  HIPCHK(hipGetLastError());
  NetSolveArgs s;
  s.PT = r->PT; s.voff = r->voff; s.abt_rp = r->abt_rp; s.bb_rp = r->bb_rp; s.abt_col = r->abt_col; s.bb_col = r->bb_col;
  s.abt_val = r->abt_val; s.bb_val = r->bb_val; s.u = r->u; s.work = r->work; s.iters = r->iters; s.uloss = r->uloss; s.n = r->n;
  const size_t lds = sizeof(float) * 5 * (size_t)std::min<int64_t>(r->vmax, NETREG_V_LDS);
  PMFCHK(ensure_dyn_lds(c, (const void *)k_netreg_solve, lds));
  k_netreg_solve<<<r->K, 256, lds, c->stream>>>(s);
  HIPCHK(hipGetLastError());
  NetGradArgs g;
  g.PT = r->PT; g.u = r->u; g.voff = r->voff; g.aa_rp = r->aa_rp; g.ab_rp = r->ab_rp; g.aa_col = r->aa_col;
  g.ab_col = r->ab_col; g.aa_val = r->aa_val; g.ab_val = r->ab_val; g.uloss = r->uloss; g.grad = r->grad;
  g.reg_partial = c->reg_partial + (int64_t)which * REG_SLOTS + *reg_count;
  g.n = r->n; g.Kp = c->Kp; g.rb = r->rb; g.p = r->p;
  k_netreg_grad<<<grid, 256, 0, c->stream>>>(g);
  HIPCHK(hipGetLastError());
  *reg_count += grid;
  return 0;
}

// shape, monotone row pointers, sorted in-range columns of one CSR block
static int check_csr(const pmf_csr &m, int64_t rows, int64_t cols, const char *name, int k) {
  if (m.n_rows != rows || m.n_cols != cols)
    return pmf_fail("network regularizer: %s[%d] is %lld x %lld, expected %lld x %lld", name, k, (long long)m.n_rows, (long long)m.n_cols, (long long)rows, (long long)cols);
  if (rows == 0) return 0;
  if (!m.rowptr) return pmf_fail("network regularizer: %s[%d] has a null rowptr", name, k);
  if (m.rowptr[0] != 0) return pmf_fail("network regularizer: %s[%d].rowptr[0] = %lld, expected 0 (0-based CSR)", name, k, (long long)m.rowptr[0]);
  for (int64_t i = 0; i < rows; ++i)
    if (m.rowptr[i + 1] < m.rowptr[i]) return pmf_fail("network regularizer: %s[%d].rowptr decreases at row %lld", name, k, (long long)i);
  const int64_t nnz = m.rowptr[rows];
  if (nnz > 0 && (!m.col || !m.val)) return pmf_fail("network regularizer: %s[%d] has entries but a null col / val", name, k);
  for (int64_t i = 0; i < rows; ++i)
    for (int64_t e = m.rowptr[i]; e < m.rowptr[i + 1]; ++e) {
      if (m.col[e] < 0 || m.col[e] >= cols) return pmf_fail("network regularizer: %s[%d] row %lld: column %d out of range (0..%lld)", name, k, (long long)i, m.col[e], (long long)cols - 1);
      if (e > m.rowptr[i] && m.col[e] <= m.col[e - 1]) return pmf_fail("network regularizer: %s[%d] row %lld: columns not sorted / repeated", name, k, (long long)i);
    }
  return 0;
}

template <typename T>
static int upload_new(DevBuf<T> &dst, const std::vector<T> &h) {
  PMFCHK(dst.alloc(h.size(), false));
  return dst.upload(h.data(), h.size());
}

// one family of blocks concatenated: row pointers made absolute, `rows(k)` rows for factor k (plus one closing entry each)
struct CsrCat {
  std::vector<int64_t> rp;
  std::vector<int32_t> col;
  std::vector<float> val;
  void append(const pmf_csr &m) {
    const int64_t base = (int64_t)col.size();
    for (int64_t i = 0; i < m.n_rows; ++i) rp.push_back(base + m.rowptr[i]);
    const int64_t nnz = m.n_rows ? m.rowptr[m.n_rows] : 0;
    rp.push_back(base + nnz);
    col.insert(col.end(), m.col, m.col + nnz);
    val.insert(val.end(), m.val, m.val + nnz);
  }
  int upload(DevBuf<int64_t> &d_rp, DevBuf<int32_t> &d_col, DevBuf<float> &d_val) const {
    PMFCHK(upload_new(d_rp, rp));
    PMFCHK(upload_new(d_col, col));
    return upload_new(d_val, val);
  }
};

static int add_network(pmf_ctx *c, int which, int K, const pmf_csr *AA, const pmf_csr *AB, const pmf_csr *BB, const float *const *u0, float p) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0) return pmf_fail("factors must be set before their regularizers");
  if (K != c->K) return pmf_fail("network regularizer: %d factors given, the context has K=%d", K, c->K);
  if (c->net[which]) return pmf_fail("only one network term is supported on %s (clear the regularizer first)", which ? "Y" : "X");
  if (!AA || !AB || !BB) return pmf_fail("network regularizer: null block array");
  const int64_t n = which == 0 ? c->M : c->N;
  std::vector<int64_t> voff((size_t)K + 1, 0);
  for (int k = 0; k < K; ++k) {
    const int64_t v = BB[k].n_rows;
    if (v < 0) return pmf_fail("network regularizer: BB[%d] has %lld rows", k, (long long)v);
    PMFCHK(check_csr(AA[k], n, n, "AA", k));
    PMFCHK(check_csr(AB[k], n, v, "AB", k));
    PMFCHK(check_csr(BB[k], v, v, "BB", k));
    voff[(size_t)k + 1] = voff[(size_t)k] + v;
  }
  const int64_t V = voff[(size_t)K];
  CsrCat aa, ab, abt, bb;
  for (int k = 0; k < K; ++k) {
    aa.append(AA[k]);
    ab.append(AB[k]);
    bb.append(BB[k]);
    // AB_k' by a counting sort over the columns of AB_k: rows come out sorted
    const int64_t v = BB[k].n_rows, nnz = AB[k].rowptr[n];
    std::vector<int64_t> cnt((size_t)v + 1, 0);
    for (int64_t e = 0; e < nnz; ++e) cnt[(size_t)AB[k].col[e] + 1]++;
    for (int64_t j = 0; j < v; ++j) cnt[(size_t)j + 1] += cnt[(size_t)j];
    const int64_t base = (int64_t)abt.col.size();
    for (int64_t j = 0; j <= v; ++j) abt.rp.push_back(base + cnt[(size_t)j]);
    abt.col.resize((size_t)(base + nnz));
    abt.val.resize((size_t)(base + nnz));
    for (int64_t i = 0; i < n; ++i)
      for (int64_t e = AB[k].rowptr[i]; e < AB[k].rowptr[i + 1]; ++e) {
        const int64_t dst = base + cnt[(size_t)AB[k].col[e]]++;
        abt.col[(size_t)dst] = (int32_t)i;
        abt.val[(size_t)dst] = AB[k].val[e];
      }
  }
  std::vector<float> hu((size_t)V, 0.f);
  if (u0)
    for (int k = 0; k < K; ++k)
      if (u0[k]) std::copy(u0[k], u0[k] + (voff[(size_t)k + 1] - voff[(size_t)k]), hu.begin() + voff[(size_t)k]);
  NetReg *r = new NetReg;
  c->net[which] = r;
  r->K = K; r->n = n; r->V = V; r->p = p; r->h_voff = voff;
  for (int k = 0; k < K; ++k) r->vmax = std::max(r->vmax, voff[(size_t)k + 1] - voff[(size_t)k]);
  r->rb = (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, NETREG_SLOTS / K));
  const int rc = [&]() -> int {
    PMFCHK(upload_new(r->voff, voff));
    PMFCHK(aa.upload(r->aa_rp, r->aa_col, r->aa_val));
    PMFCHK(ab.upload(r->ab_rp, r->ab_col, r->ab_val));
    PMFCHK(abt.upload(r->abt_rp, r->abt_col, r->abt_val));
    PMFCHK(bb.upload(r->bb_rp, r->bb_col, r->bb_val));
    PMFCHK(upload_new(r->u, hu));
    PMFCHK(r->work.alloc(r->vmax > NETREG_V_LDS ? (size_t)(4 * V) : 0, true));
    PMFCHK(r->PT.alloc((size_t)(K * n), true));
    PMFCHK(r->grad.alloc((size_t)c->P[which].n, true));
    PMFCHK(r->iters.alloc((size_t)K, true));
    return r->uloss.alloc((size_t)K, true);
  }();
  if (rc < 0) netreg_free(c, which);   // (sets no error of its own: the message of the failed step stays)
  return rc;
}

extern "C" int pmf_add_xreg_network(pmf_ctx *c, int K, const pmf_csr *AA, const pmf_csr *AB, const pmf_csr *BB, const float *const *u0, float p) {
  return add_network(c, 0, K, AA, AB, BB, u0, p);
}
extern "C" int pmf_add_yreg_network(pmf_ctx *c, int K, const pmf_csr *AA, const pmf_csr *AB, const pmf_csr *BB, const float *const *u0, float p) {
  return add_network(c, 1, K, AA, AB, BB, u0, p);
}

extern "C" int pmf_get_reg_network_state(pmf_ctx *c, int which, int k, float *u, int *cg_iters) {
  PMFCHK(ctx_bind(c));
  if (which != PMF_PARAM_X && which != PMF_PARAM_Y) return pmf_fail("pmf_get_reg_network_state: parameter %d is neither X nor Y", which);
  const NetReg *r = c->net[which];
  if (!r) return pmf_fail("no network term on %s", which ? "Y" : "X");
  if (k < 0 || k >= r->K) return pmf_fail("pmf_get_reg_network_state: factor %d out of range (0..%d)", k, r->K - 1);
  HIPCHK(hipStreamSynchronize(c->stream));
  const int64_t v0 = r->h_voff[(size_t)k], v = r->h_voff[(size_t)k + 1] - v0;
  if (u && v > 0) HIPCHK(hipMemcpy(u, r->u + v0, sizeof(float) * (size_t)v, hipMemcpyDeviceToHost));
  if (cg_iters) {
    int32_t it = 0;
    HIPCHK(hipMemcpy(&it, r->iters + k, sizeof(int32_t), hipMemcpyDeviceToHost));
    *cg_iters = it;
  }
  return 0;
}

// L1Regularizer / SelectiveL1Reg: dense weights wl1[k, j] += p w_k m_kj in the parameter's layout (like wq)
static int add_l1(pmf_ctx *c, int which, const float *w, const uint8_t *mask, float p) {
  PMFCHK(ctx_bind(c));
  if (c->K == 0) return pmf_fail("factors must be set before their regularizers");
  if (!w) return pmf_fail("L1 regularizer: null weights");
  ParamBuf &b = c->P[which];
  const int64_t n = which == 0 ? c->M : c->N;
  std::vector<float> h((size_t)b.n, 0.f);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (b.wl1) HIPCHK(hipMemcpy(h.data(), b.wl1, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
  for (int64_t j = 0; j < n; ++j)
    for (int k = 0; k < c->K; ++k)
      if (!mask || mask[j * c->K + k]) h[(size_t)(j * c->Kp + k)] += p * w[k];
  PMFCHK(b.wl1.ensure((size_t)b.n, false));
  HIPCHK(hipMemcpy(b.wl1, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice));
  return 0;
}
extern "C" int pmf_add_xreg_l1(pmf_ctx *c, const float *w, const uint8_t *mask, float p) { return add_l1(c, 0, w, mask, p); }
extern "C" int pmf_add_yreg_l1(pmf_ctx *c, const float *w, const uint8_t *mask, float p) { return add_l1(c, 1, w, mask, p); }
