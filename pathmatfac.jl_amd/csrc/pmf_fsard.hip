// pmf_fsard.hip -- FeatureSetARD outer loop on the device, dense S (pmf_fsard_update_A).
#include "pmf_fsard_loop.h"

// ------------------------------------------------------------------------------------------------
// update_A! (src/featureset_ard.jl:214-294) with A in one workgroup's LDS and a dense S: L x K <= 16384.  The loop itself
// -- the per-entry formulas, the bookkeeping of update_A_inner!, the ISTA update, the host driver -- is in
// pmf_fsard_loop.h; this file has the two kernels of an iteration and what is particular to a dense S.  Up to max_epochs
// serial iterations of two small kernels per view, no host round trip inside a batch of iterations:
//   k_fsard_grad  : (column slices of the view) A'S, the loss at A, grad_{A'S}, partial S * grad' per workgroup
//   k_fsard_step  : (one workgroup) fixed-order sum of the partials, the loop's bookkeeping, then the ISTA update of A
//                   unless the loop has ended.
// Y stays where the fit left it (the context's device copy); beta = beta0 (v0 + A'S) is written straight into the
// device array of an attached FeatureSetARD term (featureset_ard.jl:292; never into a plain ARD term's) as well as returned.
// ------------------------------------------------------------------------------------------------
struct FsardArgs : FsardLoopArgs {
  const float *S;          // L x Nv row-major (feature set l's weights over the view's columns)
  float *gpart;            // [n_wg][L*K] partial gradients
  double *lpart;           // [n_wg] partial data losses
  int32_t L, CW, n_wg;
};

// thread = column (CW = blockDim.x columns per sub-slice); A in LDS; the sub-slice's grad_{A'S} tile [K][CW] in LDS;
// then thread -> (l, k) outputs, each a dot product over the sub-slice.  final_beta != 0: only write beta (no gradient).
__global__ __launch_bounds__(256) void k_fsard_grad(const FsardArgs a, int final_beta) {
  extern __shared__ __attribute__((aligned(16))) char smem_fs[];
  float *As = reinterpret_cast<float *>(smem_fs);      // [L][K]
  float *Gt = As + a.L * a.K;                           // [K][CW + 1] (odd row stride: the dot products below read a column of rows)
  const int GS = a.CW + 1;
  __shared__ double sh[4];
  if (!final_beta && a.istate[0]) return;               // the loop has ended: nothing left to evaluate
  const int tid = threadIdx.x, NT = blockDim.x;
  const float *Asrc = final_beta ? a.A_best : a.A;
  for (int e = tid; e < a.L * a.K; e += NT) As[e] = Asrc[e];
  const int64_t per = (a.Nv + a.n_wg - 1) / a.n_wg;
  const int64_t j_lo = blockIdx.x * per, j_hi = j_lo + per < a.Nv ? j_lo + per : a.Nv;
  const float beta0 = a.alpha0 - 1.f;
  constexpr int MAXO = 64;                              // (l, k) outputs per thread: L*K <= 64 * 256
  float gacc[MAXO];
#pragma unroll
  for (int o = 0; o < MAXO; ++o) gacc[o] = 0.f;
  double lacc = 0.0;
  __syncthreads();
  for (int64_t js = j_lo; js < j_hi; js += a.CW) {
    const int64_t j = js + tid;
    const bool live = tid < a.CW && j < j_hi;
    // ---- A'S for this column, k in chunks of 32 (accumulators in registers)
    for (int k0 = 0; k0 < a.K; k0 += 32) {
      float acc[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) acc[q] = 0.f;
      if (live) {
        for (int l = 0; l < a.L; ++l) {
          const float sv = a.S[(int64_t)l * a.Nv + j];
          if (sv != 0.f) {
            const float *ar = As + l * a.K + k0;
#pragma unroll
            for (int q = 0; q < 32; ++q)
              if (k0 + q < a.K) acc[q] = fmaf(ar[q], sv, acc[q]);
          }
        }
      }
      const float al = live ? a.alpha[j] : 0.f;
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        const int k = k0 + q;
        if (k < a.K) {
          float g = 0.f;
          if (live) {
            const float beta = fsard_beta(acc[q], beta0, a.v0);
            if (final_beta) {
              if (a.beta_dev) a.beta_dev[(j) * a.Kp + k] = beta;
            } else {
              g = fsard_entry(beta, a.Y[(a.c0 + j) * a.Kp + k], al, beta0, lacc);
            }
          }
          if (!final_beta && tid < a.CW) Gt[k * GS + tid] = g;
        }
      }
      if (!final_beta && live && k0 == 0) lacc -= fsard_calibration(al);   // once per column
    }
    if (final_beta) continue;
    __syncthreads();
    // ---- partial grad_A[l][k] += sum_j S[l][js + j] * Gt[k][j]
    const int ncol = (int)(j_hi - js < a.CW ? j_hi - js : a.CW);
#pragma unroll
    for (int o = 0; o < MAXO; ++o) {
      const int e = tid + o * NT;
      if (e < a.L * a.K) {
        const int l = e / a.K, k = e - l * a.K;
        const float *sr = a.S + (int64_t)l * a.Nv + js;
        const float *gr = Gt + k * GS;
        float sacc = 0.f;
        for (int jj = 0; jj < ncol; ++jj) {
          const float sv = sr[jj];                       // (S is sparse: most feature sets skip most columns)
          if (sv != 0.f) sacc = fmaf(sv, gr[jj], sacc);
        }
        gacc[o] += sacc;
      }
    }
    __syncthreads();
  }
  if (final_beta) return;
#pragma unroll
  for (int o = 0; o < MAXO; ++o) {
    const int e = tid + o * NT;
    if (e < a.L * a.K) a.gpart[(int64_t)blockIdx.x * a.L * a.K + e] = gacc[o];
  }
  const double ls = block_reduce_sum(lacc, sh);
  if (tid == 0) a.lpart[blockIdx.x] = ls;
}

// one workgroup: loss(A_t) = sum lambda_k |A_lk| (waves in index order) + the partials in index order; the loop's
// bookkeeping; then the ISTA update unless the loop has ended.  `done` reaches the host and the next launches only
// after the update: istate[0] is written last.
__global__ __launch_bounds__(1024) void k_fsard_step(const FsardArgs a) {
  __shared__ double sh[16];
  __shared__ int s_improved, s_done;
  if (a.istate[0]) return;
  const int tid = threadIdx.x, NT = blockDim.x, n = a.L * a.K;
  double reg = 0.0;
  for (int e = tid; e < n; e += NT) reg += (double)(a.lambda[e % a.K] * fabsf(a.A[e]));
  double loss = block_reduce_sum(reg, sh);
  if (tid == 0) {
    for (int w = 0; w < a.n_wg; ++w) loss += a.lpart[w];
    const FsardDecision d = fsard_decide(a, loss);
    s_improved = d.improved;
    s_done = d.done;
  }
  __syncthreads();
  const bool improved = s_improved != 0, done = s_done != 0;
  for (int e = tid; e < n; e += NT) {
    const float av = a.A[e];
    if (improved) a.A_best[e] = av;
    if (!done) {
      float g = 0.f;
      for (int w = 0; w < a.n_wg; ++w) g += a.gpart[(int64_t)w * n + e];   // fixed order
      a.A[e] = fsard_ista(av, g, a.lambda[e % a.K], a.ssq[e], a.lr);
    }
  }
  __syncthreads();
  if (tid == 0 && done) a.istate[0] = 1;
}

extern "C" int pmf_fsard_update_A(pmf_ctx *c, int64_t col_start1, int64_t col_stop1, int L, const float *S, const float *alpha,
                                  const float *lambda, float alpha0, float v0, float lr, float *ssq_grad, float *A,
                                  int max_epochs, int term_iter, double atol, double *best_loss, int *epochs_run,
                                  float *beta_out) {
  static const char fn[] = "pmf_fsard_update_A";
  PMFCHK(ctx_bind(c));
  PMFCHK(fsard_check_args(fn, c, col_start1, col_stop1, L, max_epochs, term_iter, {{"S", S}}, alpha, lambda, ssq_grad, A));
  const int K = c->K;
  const int64_t Nv = col_stop1 - col_start1 + 1, n = (int64_t)L * K;
  if (n > 64 * 256) return pmf_fail("%s: L x K = %lld exceeds the ISTA kernel's capacity (16384)", fn, (long long)n);
  int CW = 256;
  while (CW > 32 && (size_t)(n + (int64_t)K * (CW + 1)) * 4 > 150 * 1024) CW >>= 1;
  const size_t lds = (size_t)(n + (int64_t)K * (CW + 1)) * 4;
  if (lds > 150 * 1024) return pmf_fail("%s: L x K too large for LDS", fn);
  const int n_wg = (int)std::max<int64_t>(1, std::min<int64_t>(32, (Nv + CW - 1) / CW));
  FsardArgs a;
  memset(&a, 0, sizeof(a));
  FsardLoop loop;
  PMFCHK(loop.init(fn, c, a, col_start1, col_stop1, L, alpha, lambda, ssq_grad, alpha0, v0, lr, max_epochs, term_iter, atol));
  DevBuf<float> dS, dgp;
  DevBuf<double> dlp;
  PMFCHK(dS.alloc((size_t)(L * Nv), false, "S"));
  PMFCHK(dgp.alloc((size_t)(n_wg * n), true, "the gradient partials"));
  PMFCHK(dlp.alloc((size_t)n_wg, true, "the loss partials"));
  PMFCHK(dS.upload(S, (size_t)(L * Nv)));
  a.S = dS; a.gpart = dgp; a.lpart = dlp; a.L = L; a.CW = CW; a.n_wg = n_wg;
  PMFCHK(ensure_dyn_lds(c, (const void *)k_fsard_grad, lds));
  PMFCHK(loop.run([&](int) {
    hipLaunchKernelGGL(k_fsard_grad, dim3(n_wg), dim3(256), lds, c->stream, a, 0);
    hipLaunchKernelGGL(k_fsard_step, dim3(1), dim3(1024), 0, c->stream, a);
  }));
  return loop.finish(a, [&] { hipLaunchKernelGGL(k_fsard_grad, dim3(n_wg), dim3(256), lds, c->stream, a, 1); }, A, ssq_grad,
                     best_loss, epochs_run, beta_out);
}
