// pmf_fsard_loop.h -- the loop of update_A! (src/featureset_ard.jl:214-294) that pmf_fsard.hip (dense S, A in LDS) and
// pmf_fsard_csr.hip (sparse S, A in device memory) share: nonnegative projected ISTA with AdaGrad step sizes
// (ISTAOptimiser, src/optimizers.jl:26-62) on the view's assignment matrix A (L feature sets x K factors), minimising
// gamma_normal_loss(A) + sum_k lambda_k |A_lk| (src/featureset_ard.jl:154-162 and its rrule :164-186).  Here, once:
//   device  the per-entry loss and pull-back, the per-column calibration term, the bookkeeping of update_A_inner!
//           (best loss, termination counter), the ISTA element update
//   host    the argument checks, the loop's device buffers, the batched launch loop, the final beta and the read-backs
// The two units keep what differs: how S is stored and walked, the order of their sums, and how `improved` / `done`
// reach the threads that update A.
#ifndef PMF_FSARD_LOOP_H
#define PMF_FSARD_LOOP_H
#include "pmf_ctx.h"

#include <initializer_list>
#include <utility>

// what both units' kernels take, whatever the form of S (FsardArgs and FscArgs derive from it)
struct FsardLoopArgs {
  const float *Y;          // context Y, Kp x N, column j at Y + j*Kp
  const float *alpha;      // Nv
  const float *lambda;     // K
  float *A, *A_best, *ssq; // L x K (k contiguous)
  double *state;           // [0] best loss, [1] loss of the last evaluated A
  int32_t *istate;         // [0] done, [1] term_count, [2] evaluations so far, [3] max_epochs, [4] term_iter, [5] improved (sparse S)
  float *beta_dev;         // the FeatureSetARD term's ard_beta + c0*Kp, or a temporary (may be null)
  int64_t c0, Nv;
  int32_t K, Kp;
  float alpha0, v0, lr;
  double atol;
};

// beta of one entry (k, j): as = (A'S)[k, j]   (featureset_ard.jl:292)
__device__ __forceinline__ float fsard_beta(float as, float beta0, float v0) { return beta0 * (v0 + as); }
// one entry (k, j) of gamma_normal_loss and of its pull-back (featureset_ard.jl:154-178) at that beta
__device__ __forceinline__ float fsard_entry(float beta, float y, float al, float beta0, double &lacc) {
  const float b2 = beta + 0.5f * y * y;
  lacc += (double)(-al * logf(beta) + (al + 0.5f) * logf(b2) - logf(fabsf(y) + 1e-9f));
  return beta0 * (-al / beta + (al + 0.5f) / b2);
}
// the calibration term of a column, subtracted from the loss once per column
__device__ __forceinline__ double fsard_calibration(float al) { return (double)((al + 0.5f) * logf(al + 0.5f) - al * logf(al)); }

// The bookkeeping of update_A_inner! (:239-268) for one evaluation, by ONE thread with the summed loss.
struct FsardDecision { bool improved, done; };
__device__ __forceinline__ FsardDecision fsard_decide(const FsardLoopArgs &a, double loss) {
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
  return {improved != 0, (term >= a.istate[4]) || (evals >= a.istate[3])};   // evals == max_epochs: the last update has been evaluated
}

// ISTAOptimiser.update! (optimizers.jl:46-62) of one element: -> the new A_lk; the AdaGrad accumulator is stored
__device__ __forceinline__ float fsard_ista(float av, float g, float lam, float &ssq, float lr) {
  const float s = ssq + g * g;                                        // optimizers.jl:50
  ssq = s;
  const float eta = lr / sqrtf(s);                                    // :51
  av = fmaxf(av - eta * g, 0.f);                                      // :55-56
  return fmaxf(fabsf(av) - lam * eta, 0.f);                           // ist_proj! :40-42, :61
}

// ---- host
// The checks both entries make, in one order and one wording; `fn` is the entry's name, `s_ptrs` the (name, pointer) pairs
// of its form of S.  Nothing is allocated or launched before the last check of an entry.
inline int fsard_check_args(const char *fn, const pmf_ctx *c, int64_t col_start1, int64_t col_stop1, int L, int max_epochs, int term_iter,
                            std::initializer_list<std::pair<const char *, const void *>> s_ptrs, const float *alpha,
                            const float *lambda, const float *ssq_grad, const float *A) {
  if (c->K == 0) return pmf_fail("%s: factors not set", fn);
  if (col_start1 < 1 || col_stop1 > c->N || col_start1 > col_stop1)
    return pmf_fail("%s: bad column range col_start1:col_stop1 = %lld:%lld (N = %lld)", fn, (long long)col_start1, (long long)col_stop1,
                    (long long)c->N);
  if (L < 1) return pmf_fail("%s: L must be >= 1 (got %d)", fn, L);
  if (max_epochs < 0) return pmf_fail("%s: max_epochs must be >= 0 (got %d)", fn, max_epochs);
  // (the reference's loop makes its first update before it looks at term_iter, this one would end at "Iteration 0")
  if (term_iter < 1) return pmf_fail("%s: term_iter must be >= 1 (got %d)", fn, term_iter);
  for (const auto &s : s_ptrs)
    if (!s.second) return pmf_fail("%s: %s is NULL", fn, s.first);
  if (!alpha) return pmf_fail("%s: alpha is NULL", fn);
  if (!lambda) return pmf_fail("%s: lambda is NULL", fn);
  if (!ssq_grad) return pmf_fail("%s: ssq_grad is NULL", fn);
  if (!A) return pmf_fail("%s: A is NULL", fn);
  return 0;
}

// The loop's device buffers (freed with it) and its host side.  An entry checks its arguments, calls init, uploads its S,
// then run and finish with two callables that launch its kernels on c->stream.
struct FsardLoop {
  const char *fn = nullptr;
  pmf_ctx *c = nullptr;
  int64_t n = 0;                   // L x K
  int max_epochs = 0, term_iter = 0;
  DevBuf<float> alpha, lambda, A, A_best, ssq, beta_tmp;
  DevBuf<double> state;
  DevBuf<int32_t> istate;

  // allocates and uploads; fills `args` (the base of the entry's argument struct)
  int init(const char *fn_, pmf_ctx *c_, FsardLoopArgs &args, int64_t col_start1, int64_t col_stop1, int L, const float *h_alpha,
           const float *h_lambda, const float *ssq_grad, float alpha0, float v0, float lr, int max_epochs_, int term_iter_, double atol) {
    fn = fn_; c = c_; max_epochs = max_epochs_; term_iter = term_iter_;
    const int64_t Nv = col_stop1 - col_start1 + 1;
    n = (int64_t)L * c->K;
    PMFCHK(alpha.alloc((size_t)Nv, false, "alpha"));
    PMFCHK(lambda.alloc((size_t)c->K, false, "lambda"));
    PMFCHK(A.alloc((size_t)n, true, "A"));                   // A .= 0 (featureset_ard.jl:286)
    PMFCHK(A_best.alloc((size_t)n, true, "A_best"));
    PMFCHK(ssq.alloc((size_t)n, false, "ssq_grad"));
    PMFCHK(state.alloc(8, true, "the loop state"));
    PMFCHK(istate.alloc(8, false, "the loop counters"));
    PMFCHK(alpha.upload(h_alpha, (size_t)Nv));
    PMFCHK(lambda.upload(h_lambda, (size_t)c->K));
    PMFCHK(ssq.upload(ssq_grad, (size_t)n));
    const int32_t is0[8] = {0, 0, 0, max_epochs, term_iter, 0, 0, 0};
    PMFCHK(istate.upload(is0, 8));
    args.Y = c->P[1].p; args.alpha = alpha; args.lambda = lambda; args.A = A; args.A_best = A_best; args.ssq = ssq;
    args.state = state; args.istate = istate;
    args.beta_dev = (c->has_ard && c->ard_is_fsard && c->ard_beta) ? c->ard_beta + (col_start1 - 1) * c->Kp : nullptr;
    args.c0 = col_start1 - 1; args.Nv = Nv; args.K = c->K; args.Kp = c->Kp;
    args.alpha0 = alpha0; args.v0 = v0; args.lr = lr; args.atol = atol;
    return 0;
  }

  // evaluations 0 .. max_epochs (the update after evaluation t gives A_{t+1}): enqueue(t) launches iteration t; the host
  // looks at the `done` flag once per batch of iterations
  template <typename Enqueue>
  int run(Enqueue &&enqueue) {
    const int batch = std::max(8, term_iter);
    int32_t h_is[8];
    bool done = false;
    for (int t = 0; t <= max_epochs && !done; t += batch) {
      for (int q = 0; q < batch && t + q <= max_epochs; ++q) enqueue(t + q);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(h_is, istate, sizeof(h_is), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) return pmf_fail("%s: %s", fn, hipGetErrorString(e));
      done = h_is[0] != 0;
    }
    return 0;
  }

  // A .= A_best ; beta[:, cr] = beta0 (v0 + A'S)   (featureset_ard.jl:272, 292): final_beta() launches the kernel that
  // writes beta from A_best into a.beta_dev, which this call may set to a temporary first (a: the struct given to init)
  template <typename FinalBeta>
  int finish(FsardLoopArgs &a, FinalBeta &&final_beta, float *h_A, float *ssq_grad, double *best_loss, int *epochs_run, float *beta_out) {
    if (beta_out && !a.beta_dev) {   // no device regularizer array to write into: a temporary with the view's columns
      PMFCHK(beta_tmp.alloc((size_t)(a.Nv * a.Kp), true, "beta"));
      a.beta_dev = beta_tmp;
    }
    if (a.beta_dev) final_beta();
    double h_st[8];
    int32_t h_is[8];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_st, state, sizeof(h_st), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h_is, istate, sizeof(h_is), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(h_A, A_best, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(ssq_grad, ssq, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && beta_out)
      e = hipMemcpy2D(beta_out, sizeof(float) * a.K, a.beta_dev, sizeof(float) * a.Kp, sizeof(float) * a.K, (size_t)a.Nv, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return pmf_fail("%s: %s", fn, hipGetErrorString(e));
    if (best_loss) *best_loss = h_st[0];
    if (epochs_run) *epochs_run = h_is[2] - 1;
    return 0;
  }
};
#endif
