// pmf_eig.h -- symmetric eigen-decomposition of a K x K float64 matrix (K <= 128) by cyclic Jacobi, in the library's own
// code: no LAPACK, no HIP.  Plain C++ on the host, so a stand-alone program can test it (tests/eig_check.cpp).
//
// Why Jacobi: the matrix is the K x K Gram matrix of a factor (<= 128 KB), the work is O(K^3) per sweep on the host and
// negligible next to the passes over X and Y; the method is backward stable, uses only + - * / sqrt (all correctly rounded
// by IEEE 754), and visits the pivots in a fixed order -- so the same input gives the same bits on every rank and run.
//
// Method.  Sweeps over the pivots (p, q), p < q, row by row.  A pivot is rotated away unless |a_pq| <= tiny, with
// tiny = 2^-53 * ||A||_F / K taken once from the input.  Stop when a whole sweep rotated nothing, or when
// off(A) = sqrt(2 sum_{p<q} a_pq^2) <= 2^-53 * ||A||_F before a sweep; PMF_EIG_MAX_SWEEPS sweeps at most (convergence is
// quadratic: K = 128 takes about ten), beyond which the call fails.
// Conventions (fixed, so that ranks and runs agree bit for bit):
//   eigenvalues descending, ties by original index (the index of the diagonal entry they ended on);
//   each eigenvector scaled by +-1 so that its largest-magnitude component is positive, ties by lowest index;
//   singular values of the factor = sqrt(max(lambda, 0)).
#ifndef PMF_EIG_H
#define PMF_EIG_H
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#define PMF_EIG_MAX_K 128
#define PMF_EIG_MAX_SWEEPS 30

// A: K x K symmetric, row-major (only read).  lam[K]: eigenvalues, descending.  U (may be null): K x K row-major,
// U[k * K + r] = component k of eigenvector r.  sweeps_out (may be null): sweeps run.
// Returns 0, -1 for a bad argument, -2 if the sweep limit was reached (or the input holds a non-finite value).
static inline int pmf_eig_sym(const double *A, int K, double *lam, double *U, int *sweeps_out) {
  if (!A || !lam || K < 1 || K > PMF_EIG_MAX_K) return -1;
  const size_t n = (size_t)K;
  std::vector<double> a(A, A + n * n);
  std::vector<double> vt;   // vt[r * K + k] = component k of the vector now at diagonal position r (rows are contiguous)
  if (U) {
    vt.assign(n * n, 0.0);
    for (size_t r = 0; r < n; ++r) vt[r * n + r] = 1.0;
  }
  double fro2 = 0.0;
  for (size_t i = 0; i < n * n; ++i) fro2 += a[i] * a[i];
  const double fro = std::sqrt(fro2);
  if (!(fro <= 1.7976931348623157e308)) return -2;   // NaN or inf in the input
  const double eps = 1.1102230246251565e-16;          // 2^-53
  const double tiny = eps * fro / (double)K;
  int sweep = 0;
  bool done = false;
  for (; sweep < PMF_EIG_MAX_SWEEPS; ++sweep) {
    double off2 = 0.0;
    for (size_t p = 0; p < n; ++p)
      for (size_t q = p + 1; q < n; ++q) off2 += a[p * n + q] * a[p * n + q];
    if (std::sqrt(2.0 * off2) <= eps * fro) { done = true; break; }
    int rotated = 0;
    for (size_t p = 0; p + 1 < n; ++p) {
      for (size_t q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (std::fabs(apq) <= tiny) continue;
        ++rotated;
        const double app = a[p * n + p], aqq = a[q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        double *rp = &a[p * n], *rq = &a[q * n];
        for (size_t k = 0; k < n; ++k) {   // rows p and q
          const double x = rp[k], y = rq[k];
          rp[k] = c * x - s * y;
          rq[k] = s * x + c * y;
        }
        for (size_t k = 0; k < n; ++k) {   // their mirror images, columns p and q
          a[k * n + p] = rp[k];
          a[k * n + q] = rq[k];
        }
        rp[p] = app - t * apq;
        rq[q] = aqq + t * apq;
        rp[q] = 0.0;
        rq[p] = 0.0;
        if (U) {
          double *vp = &vt[p * n], *vq = &vt[q * n];
          for (size_t k = 0; k < n; ++k) {
            const double x = vp[k], y = vq[k];
            vp[k] = c * x - s * y;
            vq[k] = s * x + c * y;
          }
        }
      }
    }
    if (rotated == 0) { done = true; break; }
  }
  if (sweeps_out) *sweeps_out = sweep;
  if (!done) return -2;
  std::vector<int> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return a[(size_t)i * n + i] > a[(size_t)j * n + j]; });
  for (size_t r = 0; r < n; ++r) lam[r] = a[(size_t)order[r] * n + order[r]];
  if (U) {
    for (size_t r = 0; r < n; ++r) {
      const double *v = &vt[(size_t)order[r] * n];
      size_t kmax = 0;
      for (size_t k = 1; k < n; ++k)
        if (std::fabs(v[k]) > std::fabs(v[kmax])) kmax = k;
      const double sg = v[kmax] < 0.0 ? -1.0 : 1.0;
      for (size_t k = 0; k < n; ++k) U[k * n + r] = sg * v[k];
    }
  }
  return 0;
}
#endif
