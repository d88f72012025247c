// pmf_fsard_csr.hip -- FeatureSetARD outer loop on a sparse S, without a bound on L x K (pmf_fsard_update_A_csr).
#include "pmf_fsard_loop.h"

#include <climits>
#include <new>

// ------------------------------------------------------------------------------------------------
// The second device path of update_A! (src/featureset_ard.jl:214-294).  pmf_fsard.hip keeps A in one workgroup's LDS and
// walks a dense S; this file keeps A, the pull-back G = d loss / d (A'S) and grad_A in device memory and walks S in
// compressed form, as the reference does (a SparseMatrixCSC, featureset_ard.jl:22).  Same arguments, outputs and loop as
// pmf_fsard_update_A: the loop -- the per-entry formulas, the bookkeeping, the ISTA update, the host driver -- is in
// pmf_fsard_loop.h.  Four launches per iteration, no host round trip inside a batch of iterations:
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
struct FscArgs : FsardLoopArgs {
  const int64_t *rowptr;     // CSR of S (L rows): grad_A
  const int32_t *col;
  const float *val;
  const int64_t *colptr;     // CSC of S (Nv columns, feature sets ascending within a column): A'S
  const int32_t *rowidx;
  const float *cval;
  float *G;                  // [Nv][K] pull-back of the loss at A'S
  float *grad;               // [L][K] grad_A
  double *lpart;             // [n_wg] data-loss partials of k_fsc_forward
  double *rpart;             // [L] sum_k lambda_k |A_lk|
  int64_t L, per;            // per: columns of one workgroup's slice in k_fsc_forward
  int32_t kp, kp_shift, n_wg;
};

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
        if (la) a.beta_dev[j * a.Kp + ka] = fsard_beta(acc0, beta0, a.v0);
        if (lb) a.beta_dev[j * a.Kp + kb] = fsard_beta(acc1, beta0, a.v0);
      } else {
        const float *y = a.Y + (a.c0 + j) * a.Kp;
        if (la) a.G[j * K + ka] = fsard_entry(fsard_beta(acc0, beta0, a.v0), y[ka], al, beta0, lacc);
        if (lb) a.G[j * K + kb] = fsard_entry(fsard_beta(acc1, beta0, a.v0), y[kb], al, beta0, lacc);
        if (ka == 0) lacc -= fsard_calibration(al);   // once per column
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
// the loop's bookkeeping; `improved` and `done` reach k_fsc_update, the next launches and the host through istate
__global__ __launch_bounds__(1024) void k_fsc_decide(const FscArgs a) {
  __shared__ double sh[16];
  if (a.istate[0]) return;
  const int tid = threadIdx.x, NT = blockDim.x;
  double s = 0.0;
  for (int64_t i = tid; i < a.n_wg; i += NT) s += a.lpart[i];
  for (int64_t i = tid; i < a.L; i += NT) s += a.rpart[i];
  const double loss = block_reduce_sum(s, sh);
  if (tid == 0) {
    const FsardDecision d = fsard_decide(a, loss);
    a.istate[5] = d.improved;
    if (d.done) a.istate[0] = 1;
  }
}

// t: the evaluation this launch belongs to.  k_fsc_decide has run for it exactly when istate[2] == t + 1; an iteration
// enqueued after the end of the loop finds an older count and changes nothing.
__global__ __launch_bounds__(256) void k_fsc_update(const FscArgs a, int t) {
  if (a.istate[2] != t + 1) return;
  const bool improved = a.istate[5] != 0, done = a.istate[0] != 0;
  const int64_t n = a.L * a.K;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const float av = a.A[e];
    if (improved) a.A_best[e] = av;
    if (!done) a.A[e] = fsard_ista(av, a.grad[e], a.lambda[e % a.K], a.ssq[e], a.lr);
  }
}

extern "C" int pmf_fsard_update_A_csr(pmf_ctx *c, int64_t col_start1, int64_t col_stop1, int L, const int64_t *rowptr,
                                      const int32_t *col, const float *val, const float *alpha, const float *lambda,
                                      float alpha0, float v0, float lr, float *ssq_grad, float *A, int max_epochs,
                                      int term_iter, double atol, double *best_loss, int *epochs_run, float *beta_out) {
  PMFCHK(ctx_bind(c));
  // ---- argument checks: nothing is allocated or launched before the last of them
  PMFCHK(fsard_check_args("pmf_fsard_update_A_csr", c, col_start1, col_stop1, L, max_epochs, term_iter,
                          {{"rowptr", rowptr}, {"col", col}, {"val", val}}, alpha, lambda, ssq_grad, A));
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
  // ---- the loop's buffers, then S in both forms and the intermediates (freed on return)
  FscArgs a;
  memset(&a, 0, sizeof(a));
  FsardLoop loop;
  PMFCHK(loop.init("pmf_fsard_update_A_csr", c, a, col_start1, col_stop1, L, alpha, lambda, ssq_grad, alpha0, v0, lr, max_epochs,
                   term_iter, atol));
  DevBuf<int64_t> d_rp, d_cp;
  DevBuf<int32_t> d_col, d_ri;
  DevBuf<float> d_val, d_cv, d_G, d_grad;
  DevBuf<double> d_lp, d_rpart;
  PMFCHK(d_rp.alloc((size_t)L + 1, false, "rowptr"));
  PMFCHK(d_col.alloc((size_t)nnz, false, "col"));
  PMFCHK(d_val.alloc((size_t)nnz, false, "val"));
  PMFCHK(d_cp.alloc((size_t)Nv + 1, false, "the column pointers of S"));
  PMFCHK(d_ri.alloc((size_t)nnz, false, "the row indices of S by column"));
  PMFCHK(d_cv.alloc((size_t)nnz, false, "the values of S by column"));
  PMFCHK(d_G.alloc((size_t)(Nv * K), false, "the pull-back G"));
  PMFCHK(d_grad.alloc((size_t)n, false, "grad_A"));
  PMFCHK(d_lp.alloc((size_t)n_wg, true, "the loss partials"));
  PMFCHK(d_rpart.alloc((size_t)L, true, "the row partials"));
  PMFCHK(d_rp.upload(rowptr, (size_t)L + 1));
  PMFCHK(d_col.upload(col, (size_t)nnz));
  PMFCHK(d_val.upload(val, (size_t)nnz));
  PMFCHK(d_cp.upload(colptr.data(), (size_t)Nv + 1));
  PMFCHK(d_ri.upload(rowidx.data(), (size_t)nnz));
  PMFCHK(d_cv.upload(cval.data(), (size_t)nnz));
  a.rowptr = d_rp; a.col = d_col; a.val = d_val; a.colptr = d_cp; a.rowidx = d_ri; a.cval = d_cv;
  a.G = d_G; a.grad = d_grad; a.lpart = d_lp; a.rpart = d_rpart;
  a.L = L; a.per = per; a.kp = kp; a.kp_shift = kp_shift; a.n_wg = n_wg;
  PMFCHK(loop.run([&](int t) {
    hipLaunchKernelGGL(k_fsc_forward<false>, dim3(n_wg), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_fsc_grad, dim3(g_rows), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_fsc_decide, dim3(1), dim3(1024), 0, c->stream, a);
    hipLaunchKernelGGL(k_fsc_update, dim3(g_upd), dim3(256), 0, c->stream, a, t);
  }));
  return loop.finish(a, [&] { hipLaunchKernelGGL(k_fsc_forward<true>, dim3(n_wg), dim3(256), 0, c->stream, a); }, A, ssq_grad,
                     best_loss, epochs_run, beta_out);
}
