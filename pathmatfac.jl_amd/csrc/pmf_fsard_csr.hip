// pmf_fsard_csr.hip -- FeatureSetARD outer loop on a sparse S, without a bound on L x K (pmf_fsard_update_A_csr).
#include "pmf_ctx.h"

#include <climits>
#include <new>

// ------------------------------------------------------------------------------------------------
// The second device path of update_A! (src/featureset_ard.jl:214-294).  pmf_fsard.hip keeps A in one workgroup's LDS and
// walks a dense S; this file keeps A, the pull-back G = d loss / d (A'S) and grad_A in device memory and walks S in
// compressed form, as the reference does (a SparseMatrixCSC, featureset_ard.jl:22).  Same arguments, outputs and loop as
// pmf_fsard_update_A (k_fsard_step is the specification of the bookkeeping); the per-entry formulas of k_fsard_grad are
// restated in fsc_entry.  Four launches per iteration, no host round trip inside a batch of iterations:
//   k_fsc_forward : (column slices) lanes along k; (A'S)[k, j] over the sets that contain column j in ascending l (the CSC
//                   of S, built once per call on the host), the loss terms in f64, G[j][k]; one f64 partial per workgroup
//   k_fsc_grad    : (one feature set per wave, or per part of one) grad_A[l][k] = sum_j S[l, j] G[j][k] in ascending j
//                   (the CSR), every output one fixed-order sum written once; sum_k lambda_k |A[l, k]| of the row in f64
//   k_fsc_decide  : (one workgroup) loss = partials in a fixed order; best loss, termination counter, `improved`, `done`
//   k_fsc_update  : (grid over L x K) A_best = A when improved; ISTAOptimiser.update! unless the loop has ended
// Lane mapping of the first two: K <= 32 packs 64 / kp items (columns / feature sets) into a wave, kp = the power of two
// at or above K; above that a wave holds one item and a lane the factors k0 + lane and k0 + 64 + lane of every chunk
// k0 = 0, 128, ... of K.  No atomics; every sum runs in an order fixed by the shapes alone.
// ------------------------------------------------------------------------------------------------
struct FscArgs {
  const float *Y;            // context Y, Kp x N, column j at Y + j*Kp
  const int64_t *rowptr;     // CSR of S (L rows): grad_A
  const int32_t *col;
  const float *val;
  const int64_t *colptr;     // CSC of S (Nv columns, feature sets ascending within a column): A'S
  const int32_t *rowidx;
  const float *cval;
  const float *alpha;        // Nv
  const float *lambda;       // K
  float *A, *A_best, *ssq;   // L x K (k contiguous)
  float *G;                  // [Nv][K] pull-back of the loss at A'S
  float *grad;               // [L][K] grad_A
  double *lpart;             // [n_wg] data-loss partials of k_fsc_forward
  double *rpart;             // [L] sum_k lambda_k |A_lk|
  double *state;             // [0] best loss, [1] loss of the last evaluated A
  int32_t *istate;           // [0] done, [1] term_count, [2] evaluations so far, [3] max_epochs, [4] term_iter, [5] improved
  float *beta_dev;           // the FeatureSetARD term's ard_beta + c0*Kp, or a temporary (may be null)
  int64_t c0, Nv, L, per;    // per: columns of one workgroup's slice in k_fsc_forward
  int32_t K, Kp, kp, kp_shift, n_wg;
  float alpha0, v0, lr;
  double atol;
};

// one entry (k, j) of gamma_normal_loss and of its pull-back (featureset_ard.jl:154-178), as k_fsard_grad has them
__device__ __forceinline__ float fsc_entry(float as, float y, float al, float beta0, float v0, double &lacc) {
  const float beta = beta0 * (v0 + as);
  const float b2 = beta + 0.5f * y * y;
  lacc += (double)(-al * logf(beta) + (al + 0.5f) * logf(b2) - logf(fabsf(y) + 1e-9f));
  return beta0 * (-al / beta + (al + 0.5f) / b2);
}

// FINAL: only write beta = beta0 (v0 + A_best'S) (no loss, no G)
template <bool FINAL>
__global__ __launch_bounds__(256) void k_fsc_forward(const FscArgs a) {
  __shared__ double sh[4];
  if (!FINAL && a.istate[0]) return;                    // the loop has ended: nothing left to evaluate
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane >> a.kp_shift, kl = lane & (a.kp - 1), pw = 64 >> a.kp_shift;
  const float *Asrc = FINAL ? a.A_best : a.A;
  const int64_t j_lo = blockIdx.x * a.per, j_hi = j_lo + a.per < a.Nv ? j_lo + a.per : a.Nv;
  const float beta0 = a.alpha0 - 1.f;
  const int K = a.K;
  double lacc = 0.0;
  for (int64_t j = j_lo + wave * pw + sub; j < j_hi; j += 4 * pw) {
    const int64_t p0 = a.colptr[j], p1 = a.colptr[j + 1];
    const float al = a.alpha[j];
    for (int k0 = 0; k0 < K; k0 += 128) {
      const int ka = k0 + kl, kb = ka + 64;
      const bool la = ka < K, lb = kb < K;
      float acc0 = 0.f, acc1 = 0.f;
      for (int64_t p = p0; p < p1; ++p) {
        const float sv = a.cval[p];
        const float *ar = Asrc + (int64_t)a.rowidx[p] * K;
        if (la) acc0 = fmaf(ar[ka], sv, acc0);
        if (lb) acc1 = fmaf(ar[kb], sv, acc1);
      }
      if (FINAL) {
        if (la) a.beta_dev[j * a.Kp + ka] = beta0 * (a.v0 + acc0);
        if (lb) a.beta_dev[j * a.Kp + kb] = beta0 * (a.v0 + acc1);
      } else {
        const float *y = a.Y + (a.c0 + j) * a.Kp;
        if (la) a.G[j * K + ka] = fsc_entry(acc0, y[ka], al, beta0, a.v0, lacc);
        if (lb) a.G[j * K + kb] = fsc_entry(acc1, y[kb], al, beta0, a.v0, lacc);
        if (ka == 0) lacc -= (double)((al + 0.5f) * logf(al + 0.5f) - al * logf(al));   // calibration term, once per column
      }
    }
  }
  if (FINAL) return;
  const double ls = block_reduce_sum(lacc, sh);
  if (threadIdx.x == 0) a.lpart[blockIdx.x] = ls;
}

__global__ __launch_bounds__(256) void k_fsc_grad(const FscArgs a) {
  if (a.istate[0]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane >> a.kp_shift, kl = lane & (a.kp - 1), pw = 64 >> a.kp_shift;
  const int64_t l = (int64_t)blockIdx.x * (4 * pw) + wave * pw + sub;
  const bool live = l < a.L;
  const int K = a.K;
  double racc = 0.0;
  if (live) {
    const int64_t p0 = a.rowptr[l], p1 = a.rowptr[l + 1];
    for (int k0 = 0; k0 < K; k0 += 128) {
      const int ka = k0 + kl, kb = ka + 64;
      const bool la = ka < K, lb = kb < K;
      float acc0 = 0.f, acc1 = 0.f;
      for (int64_t p = p0; p < p1; ++p) {
        const float sv = a.val[p];
        const float *gr = a.G + (int64_t)a.col[p] * K;
        if (la) acc0 = fmaf(sv, gr[ka], acc0);
        if (lb) acc1 = fmaf(sv, gr[kb], acc1);
      }
      if (la) { a.grad[l * K + ka] = acc0; racc += (double)(a.lambda[ka] * fabsf(a.A[l * K + ka])); }
      if (lb) { a.grad[l * K + kb] = acc1; racc += (double)(a.lambda[kb] * fabsf(a.A[l * K + kb])); }
    }
  }
  for (int off = a.kp >> 1; off > 0; off >>= 1) racc += __shfl_xor(racc, off, 64);   // the row's lanes: a fixed tree
  if (live && kl == 0) a.rpart[l] = racc;
}

// one workgroup: loss(A_t) = data partials + row partials, each thread a strided run in index order, then a fixed tree;
// the bookkeeping of update_A_inner! (:239-268) word for word as k_fsard_step has it
__global__ __launch_bounds__(1024) void k_fsc_decide(const FscArgs a) {
  __shared__ double sh[16];
  if (a.istate[0]) return;
  const int tid = threadIdx.x, NT = blockDim.x;
  double s = 0.0;
  for (int64_t i = tid; i < a.n_wg; i += NT) s += a.lpart[i];
  for (int64_t i = tid; i < a.L; i += NT) s += a.rpart[i];
  const double loss = block_reduce_sum(s, sh);
  if (tid == 0) {
    const int evals = a.istate[2];
    int improved = 0, term = a.istate[1];
    if (evals == 0) { a.state[0] = loss; improved = 1; }                 // "Iteration 0": best_loss = loss(A), A_best = A
    else if (loss < a.state[0]) {
      const double diff = a.state[0] - loss;
      a.state[0] = loss;
      improved = 1;
      term = diff > a.atol ? 0 : term + 1;
    } else {
      term += 1;
    }
    a.state[1] = loss;
    a.istate[1] = term;
    a.istate[2] = evals + 1;
    a.istate[5] = improved;
    if ((term >= a.istate[4]) || (evals >= a.istate[3])) a.istate[0] = 1;   // evals == max_epochs: the last update has been evaluated
  }
}

// t: the evaluation this launch belongs to.  k_fsc_decide has run for it exactly when istate[2] == t + 1; an iteration
// enqueued after the end of the loop finds an older count and changes nothing.
__global__ __launch_bounds__(256) void k_fsc_update(const FscArgs a, int t) {
  if (a.istate[2] != t + 1) return;
  const bool improved = a.istate[5] != 0, done = a.istate[0] != 0;
  const int64_t n = a.L * a.K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    float av = a.A[e];
    if (improved) a.A_best[e] = av;
    if (!done) {
      const float g = a.grad[e];
      const float lam = a.lambda[e % a.K];
      const float ssq = a.ssq[e] + g * g;                                 // optimizers.jl:50
      a.ssq[e] = ssq;
      const float eta = a.lr / sqrtf(ssq);                                // :51
      av = fmaxf(av - eta * g, 0.f);                                      // :55-56
      av = fmaxf(fabsf(av) - lam * eta, 0.f);                             // ist_proj! :40-42, :61
      a.A[e] = av;
    }
  }
}

extern "C" int pmf_fsard_update_A_csr(pmf_ctx *c, int64_t col_start1, int64_t col_stop1, int L, const int64_t *rowptr,
                                      const int32_t *col, const float *val, const float *alpha, const float *lambda,
                                      float alpha0, float v0, float lr, float *ssq_grad, float *A, int max_epochs,
                                      int term_iter, double atol, double *best_loss, int *epochs_run, float *beta_out) {
  PMFCHK(ctx_bind(c));
  // ---- argument checks: nothing is allocated or launched before the last of them
  if (c->K == 0) return pmf_fail("pmf_fsard_update_A_csr: factors not set");
  if (col_start1 < 1 || col_stop1 > c->N || col_start1 > col_stop1)
    return pmf_fail("pmf_fsard_update_A_csr: bad column range col_start1:col_stop1 = %lld:%lld (N = %lld)", (long long)col_start1,
                    (long long)col_stop1, (long long)c->N);
  if (L < 1) return pmf_fail("pmf_fsard_update_A_csr: L must be >= 1 (got %d)", L);
  if (max_epochs < 0) return pmf_fail("pmf_fsard_update_A_csr: max_epochs must be >= 0 (got %d)", max_epochs);
  // (the reference's loop makes its first update before it looks at term_iter, this one would end at "Iteration 0")
  if (term_iter < 1) return pmf_fail("pmf_fsard_update_A_csr: term_iter must be >= 1 (got %d)", term_iter);
  if (!rowptr) return pmf_fail("pmf_fsard_update_A_csr: rowptr is NULL");
  if (!col) return pmf_fail("pmf_fsard_update_A_csr: col is NULL");
  if (!val) return pmf_fail("pmf_fsard_update_A_csr: val is NULL");
  if (!alpha) return pmf_fail("pmf_fsard_update_A_csr: alpha is NULL");
  if (!lambda) return pmf_fail("pmf_fsard_update_A_csr: lambda is NULL");
  if (!ssq_grad) return pmf_fail("pmf_fsard_update_A_csr: ssq_grad is NULL");
  if (!A) return pmf_fail("pmf_fsard_update_A_csr: A is NULL");
  const int K = c->K;
  const int64_t Nv = col_stop1 - col_start1 + 1, n = (int64_t)L * K;
  if (Nv > INT32_MAX) return pmf_fail("pmf_fsard_update_A_csr: a view of %lld columns does not fit col's 32-bit indices", (long long)Nv);
  if (rowptr[0] != 0) return pmf_fail("pmf_fsard_update_A_csr: rowptr[0] must be 0 (got %lld)", (long long)rowptr[0]);
  for (int l = 0; l < L; ++l)
    if (rowptr[l + 1] < rowptr[l])
      return pmf_fail("pmf_fsard_update_A_csr: rowptr decreases at row %d (%lld after %lld)", l, (long long)rowptr[l + 1], (long long)rowptr[l]);
  const int64_t nnz = rowptr[L];
  for (int l = 0; l < L; ++l)
    for (int64_t p = rowptr[l]; p < rowptr[l + 1]; ++p) {
      if (col[p] < 0 || col[p] >= Nv)
        return pmf_fail("pmf_fsard_update_A_csr: col[%lld] = %d of row %d is outside 0 .. %lld", (long long)p, col[p], l, (long long)(Nv - 1));
      if (p > rowptr[l] && col[p] <= col[p - 1])
        return pmf_fail("pmf_fsard_update_A_csr: col of row %d is not strictly ascending at col[%lld] = %d", l, (long long)p, col[p]);
    }
  // ---- the CSC of S by a counting sort of the CSR: feature sets come out ascending within every column
  std::vector<int64_t> colptr;
  std::vector<int32_t> rowidx;
  std::vector<float> cval;
  try {
    colptr.assign((size_t)Nv + 1, 0);
    rowidx.resize((size_t)nnz);
    cval.resize((size_t)nnz);
  } catch (const std::bad_alloc &) {
    return pmf_fail("pmf_fsard_update_A_csr: cannot allocate %zu bytes of host memory for the transpose of S",
                    (size_t)(Nv + 1) * 8 + (size_t)nnz * 8);
  }
  for (int64_t p = 0; p < nnz; ++p) colptr[(size_t)col[p] + 1] += 1;
  for (int64_t j = 0; j < Nv; ++j) colptr[(size_t)j + 1] += colptr[(size_t)j];
  {
    std::vector<int64_t> next(colptr.begin(), colptr.end() - 1);
    for (int l = 0; l < L; ++l)
      for (int64_t p = rowptr[l]; p < rowptr[l + 1]; ++p) {
        const int64_t q = next[(size_t)col[p]]++;
        rowidx[(size_t)q] = l;
        cval[(size_t)q] = val[p];
      }
  }
  // ---- geometry
  int kp = 64, kp_shift = 6;
  if (K <= 32) { kp = 1; kp_shift = 0; while (kp < K) { kp <<= 1; ++kp_shift; } }
  const int pw = 64 / kp;                                  // columns / feature sets per wave
  const int64_t step = 4 * pw;                             // ... per workgroup and pass
  const int n_wg = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (Nv + step - 1) / step));
  const int64_t per = (Nv + n_wg - 1) / n_wg;
  const int g_rows = (int)((L + step - 1) / step);
  const int g_upd = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256));
  // ---- device buffers (freed on return)
  DevBuf<int64_t> d_rp, d_cp;
  DevBuf<int32_t> d_col, d_ri, d_is;
  DevBuf<float> d_val, d_cv, d_al, d_lam, d_A, d_Ab, d_ssq, d_G, d_grad, d_beta_tmp;
  DevBuf<double> d_lp, d_rpart, d_st;
  PMFCHK(d_rp.alloc((size_t)L + 1, false, "rowptr"));
  PMFCHK(d_col.alloc((size_t)nnz, false, "col"));
  PMFCHK(d_val.alloc((size_t)nnz, false, "val"));
  PMFCHK(d_cp.alloc((size_t)Nv + 1, false, "the column pointers of S"));
  PMFCHK(d_ri.alloc((size_t)nnz, false, "the row indices of S by column"));
  PMFCHK(d_cv.alloc((size_t)nnz, false, "the values of S by column"));
  PMFCHK(d_al.alloc((size_t)Nv, false, "alpha"));
  PMFCHK(d_lam.alloc((size_t)K, false, "lambda"));
  PMFCHK(d_A.alloc((size_t)n, true, "A"));                 // A .= 0 (featureset_ard.jl:286)
  PMFCHK(d_Ab.alloc((size_t)n, true, "A_best"));
  PMFCHK(d_ssq.alloc((size_t)n, false, "ssq_grad"));
  PMFCHK(d_G.alloc((size_t)(Nv * K), false, "the pull-back G"));
  PMFCHK(d_grad.alloc((size_t)n, false, "grad_A"));
  PMFCHK(d_lp.alloc((size_t)n_wg, true, "the loss partials"));
  PMFCHK(d_rpart.alloc((size_t)L, true, "the row partials"));
  PMFCHK(d_st.alloc(8, true, "the loop state"));
  PMFCHK(d_is.alloc(8, false, "the loop counters"));
  PMFCHK(d_rp.upload(rowptr, (size_t)L + 1));
  PMFCHK(d_col.upload(col, (size_t)nnz));
  PMFCHK(d_val.upload(val, (size_t)nnz));
  PMFCHK(d_cp.upload(colptr.data(), (size_t)Nv + 1));
  PMFCHK(d_ri.upload(rowidx.data(), (size_t)nnz));
  PMFCHK(d_cv.upload(cval.data(), (size_t)nnz));
  PMFCHK(d_al.upload(alpha, (size_t)Nv));
  PMFCHK(d_lam.upload(lambda, (size_t)K));
  PMFCHK(d_ssq.upload(ssq_grad, (size_t)n));
  const int32_t is0[8] = {0, 0, 0, max_epochs, term_iter, 0, 0, 0};
  PMFCHK(d_is.upload(is0, 8));
  FscArgs a;
  memset(&a, 0, sizeof(a));
  a.Y = c->P[1].p; a.rowptr = d_rp.p; a.col = d_col.p; a.val = d_val.p; a.colptr = d_cp.p; a.rowidx = d_ri.p; a.cval = d_cv.p;
  a.alpha = d_al.p; a.lambda = d_lam.p; a.A = d_A.p; a.A_best = d_Ab.p; a.ssq = d_ssq.p; a.G = d_G.p; a.grad = d_grad.p;
  a.lpart = d_lp.p; a.rpart = d_rpart.p; a.state = d_st.p; a.istate = d_is.p;
  a.beta_dev = (c->has_ard && c->ard_is_fsard && c->ard_beta) ? c->ard_beta + (col_start1 - 1) * c->Kp : nullptr;
  a.c0 = col_start1 - 1; a.Nv = Nv; a.L = L; a.per = per; a.K = K; a.Kp = c->Kp; a.kp = kp; a.kp_shift = kp_shift; a.n_wg = n_wg;
  a.alpha0 = alpha0; a.v0 = v0; a.lr = lr; a.atol = atol;
  int32_t h_is[8];
  hipError_t e = hipSuccess;
  // evaluations 0 .. max_epochs (the update after evaluation t gives A_{t+1}); the host looks at the `done` flag once
  // per batch of iterations
  const int batch = std::max(8, term_iter);
  bool done = false;
  for (int t = 0; t <= max_epochs && !done; t += batch) {
    for (int q = 0; q < batch && t + q <= max_epochs; ++q) {
      hipLaunchKernelGGL(k_fsc_forward<false>, dim3(n_wg), dim3(256), 0, c->stream, a);
      hipLaunchKernelGGL(k_fsc_grad, dim3(g_rows), dim3(256), 0, c->stream, a);
      hipLaunchKernelGGL(k_fsc_decide, dim3(1), dim3(1024), 0, c->stream, a);
      hipLaunchKernelGGL(k_fsc_update, dim3(g_upd), dim3(256), 0, c->stream, a, t + q);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_is, d_is.p, sizeof(h_is), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return pmf_fail("pmf_fsard_update_A_csr: %s", hipGetErrorString(e));
    done = h_is[0] != 0;
  }
  // A .= A_best ; beta[:, cr] = beta0 (v0 + A'S)   (featureset_ard.jl:272, 292)
  if (beta_out && !a.beta_dev) {   // no device regularizer array to write into: a temporary with the view's columns
    PMFCHK(d_beta_tmp.alloc((size_t)(Nv * c->Kp), true, "beta"));
    a.beta_dev = d_beta_tmp.p;
  }
  if (a.beta_dev) hipLaunchKernelGGL(k_fsc_forward<true>, dim3(n_wg), dim3(256), 0, c->stream, a);
  double h_st[8];
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h_st, d_st.p, sizeof(h_st), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h_is, d_is.p, sizeof(h_is), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(A, d_Ab.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(ssq_grad, d_ssq.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && beta_out)
    e = hipMemcpy2D(beta_out, sizeof(float) * K, a.beta_dev, sizeof(float) * c->Kp, sizeof(float) * K, (size_t)Nv, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return pmf_fail("pmf_fsard_update_A_csr: %s", hipGetErrorString(e));
  if (best_loss) *best_loss = h_st[0];
  if (epochs_run) *epochs_run = h_is[2] - 1;
  return 0;
}
