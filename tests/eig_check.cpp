// Stand-alone check of csrc/pmf_eig.h (no HIP, no GPU): compiled and run by tests/test_eig_standalone.py.
//   eig_check                      the built-in cases; exit status 0 if every check holds
//   eig_check K in.bin out.bin     decomposes the K x K float64 matrix in in.bin (row-major) and writes lam[K] then U[K x K]
// Checked per matrix (bound (c) of the test file): ||G U - U L||_F and ||U'U - I||_F <= 64 K 2^-53 ||G||_F (resp. 64 K 2^-53),
// eigenvalues descending, and for every eigenvector the largest-magnitude component (lowest index on ties) positive.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pmf_eig.h"

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      ++g_fail;                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
    }                                    \
  } while (0)

static double lcg(unsigned long long &s) {   // uniform in (-1, 1)
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((s >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0;
}

// residual and orthogonality, returned relative to their bounds' scale
static void residuals(const std::vector<double> &G, int K, const std::vector<double> &lam, const std::vector<double> &U,
                      double &res, double &orth, double &fro) {
  double r2 = 0.0, o2 = 0.0, f2 = 0.0;
  for (int i = 0; i < K; ++i)
    for (int r = 0; r < K; ++r) {
      double gu = 0.0, uu = 0.0;
      for (int k = 0; k < K; ++k) {
        gu += G[(size_t)i * K + k] * U[(size_t)k * K + r];
        uu += U[(size_t)k * K + i] * U[(size_t)k * K + r];
      }
      const double d = gu - U[(size_t)i * K + r] * lam[r], e = uu - (i == r ? 1.0 : 0.0);
      r2 += d * d;
      o2 += e * e;
      f2 += G[(size_t)i * K + r] * G[(size_t)i * K + r];
    }
  res = std::sqrt(r2); orth = std::sqrt(o2); fro = std::sqrt(f2);
}

static void check_matrix(const char *name, const std::vector<double> &G, int K, bool conventions, std::vector<double> *lam_out = nullptr,
                         std::vector<double> *U_out = nullptr) {
  std::vector<double> lam((size_t)K), U((size_t)K * K), lam2((size_t)K);
  int sweeps = -1;
  const int rc = pmf_eig_sym(G.data(), K, lam.data(), U.data(), &sweeps);
  CHECK(rc == 0, "%s: pmf_eig_sym returned %d", name, rc);
  if (rc != 0) return;
  double res, orth, fro;
  residuals(G, K, lam, U, res, orth, fro);
  const double bound = 64.0 * K * 1.1102230246251565e-16;
  std::printf("EIG %s K=%d sweeps=%d residual=%.3e (bound %.3e) orthogonality=%.3e (bound %.3e)\n", name, K, sweeps, res, bound * fro,
              orth, bound);
  CHECK(res <= bound * fro, "%s: residual %.3e above %.3e", name, res, bound * fro);
  CHECK(orth <= bound, "%s: orthogonality %.3e above %.3e", name, orth, bound);
  for (int r = 0; r + 1 < K; ++r) CHECK(lam[r] >= lam[r + 1], "%s: eigenvalues %d, %d ascend", name, r, r + 1);
  // the eigenvalues alone (U = null) are the same bits
  CHECK(pmf_eig_sym(G.data(), K, lam2.data(), nullptr, nullptr) == 0 && std::memcmp(lam.data(), lam2.data(), sizeof(double) * K) == 0,
        "%s: eigenvalues differ without U", name);
  if (conventions)
    for (int r = 0; r < K; ++r) {
      int kmax = 0;
      for (int k = 1; k < K; ++k)
        if (std::fabs(U[(size_t)k * K + r]) > std::fabs(U[(size_t)kmax * K + r])) kmax = k;
      CHECK(U[(size_t)kmax * K + r] > 0.0, "%s: vector %d has a negative largest component", name, r);
    }
  if (lam_out) *lam_out = lam;
  if (U_out) *U_out = U;
}

// G = Q diag(d) Q' with Q from Gram-Schmidt of a random matrix
static std::vector<double> with_spectrum(const std::vector<double> &d, unsigned long long seed) {
  const int K = (int)d.size();
  std::vector<double> Q((size_t)K * K), G((size_t)K * K, 0.0);
  for (auto &q : Q) q = lcg(seed);
  for (int r = 0; r < K; ++r) {
    for (int pass = 0; pass < 2; ++pass)
      for (int p = 0; p < r; ++p) {
        double dot = 0.0;
        for (int k = 0; k < K; ++k) dot += Q[(size_t)k * K + r] * Q[(size_t)k * K + p];
        for (int k = 0; k < K; ++k) Q[(size_t)k * K + r] -= dot * Q[(size_t)k * K + p];
      }
    double nrm = 0.0;
    for (int k = 0; k < K; ++k) nrm += Q[(size_t)k * K + r] * Q[(size_t)k * K + r];
    nrm = std::sqrt(nrm);
    for (int k = 0; k < K; ++k) Q[(size_t)k * K + r] /= nrm;
  }
  for (int i = 0; i < K; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int r = 0; r < K; ++r) s += Q[(size_t)i * K + r] * d[r] * Q[(size_t)j * K + r];
      G[(size_t)i * K + j] = G[(size_t)j * K + i] = s;
    }
  return G;
}

int main(int argc, char **argv) {
  if (argc == 4) {
    const int K = std::atoi(argv[1]);
    if (K < 1 || K > PMF_EIG_MAX_K) return 2;
    std::vector<double> G((size_t)K * K), lam((size_t)K), U((size_t)K * K);
    FILE *f = std::fopen(argv[2], "rb");
    if (!f || std::fread(G.data(), sizeof(double), G.size(), f) != G.size()) return 2;
    std::fclose(f);
    if (pmf_eig_sym(G.data(), K, lam.data(), U.data(), nullptr) != 0) return 3;
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(lam.data(), sizeof(double), lam.size(), f) != lam.size() ||
        std::fwrite(U.data(), sizeof(double), U.size(), f) != U.size())
      return 2;
    std::fclose(f);
    return 0;
  }
  std::vector<double> lam, U;
  // 1 x 1
  check_matrix("one_by_one", {3.5}, 1, true, &lam, &U);
  CHECK(lam.size() == 1 && lam[0] == 3.5 && U[0] == 1.0, "one_by_one: lambda = %g, U = %g", lam.empty() ? 0.0 : lam[0], U.empty() ? 0.0 : U[0]);
  check_matrix("one_by_one_negative", {-2.0}, 1, true, &lam, &U);
  CHECK(lam[0] == -2.0 && U[0] == 1.0, "one_by_one_negative");
  // diagonal, with a tie: descending, ties by original index, U a permutation of the identity
  {
    const int K = 5;
    const double d[K] = {2.0, 7.0, 2.0, -1.0, 7.0};
    const int want[K] = {1, 4, 0, 2, 3};
    std::vector<double> G((size_t)K * K, 0.0);
    for (int k = 0; k < K; ++k) G[(size_t)k * K + k] = d[k];
    check_matrix("diagonal", G, K, true, &lam, &U);
    for (int r = 0; r < K; ++r) {
      CHECK(lam[r] == d[want[r]], "diagonal: lambda[%d] = %g", r, lam[r]);
      for (int k = 0; k < K; ++k) CHECK(U[(size_t)k * K + r] == (k == want[r] ? 1.0 : 0.0), "diagonal: U[%d, %d] = %g", k, r, U[(size_t)k * K + r]);
    }
  }
  // the sign convention on a 2 x 2 whose vectors are (1, 1) / sqrt 2 and (1, -1) / sqrt 2: equal magnitudes, lowest index positive
  {
    check_matrix("two_by_two", {2.0, 1.0, 1.0, 2.0}, 2, false, &lam, &U);
    CHECK(std::fabs(lam[0] - 3.0) < 1e-15 && std::fabs(lam[1] - 1.0) < 1e-15, "two_by_two: lambda = %g, %g", lam[0], lam[1]);
    CHECK(U[0] > 0.0 && U[2] > 0.0 && U[1] > 0.0 && U[3] < 0.0, "two_by_two: signs %g %g %g %g", U[0], U[1], U[2], U[3]);
  }
  // separated spectra at the sizes the library meets
  for (int K : {2, 6, 33, 64, 128}) {
    std::vector<double> d((size_t)K);
    for (int k = 0; k < K; ++k) { const double s = K > 1 ? 2.0 - (double)k / (K - 1) : 2.0; d[k] = s * s; }
    char name[64];
    std::snprintf(name, sizeof(name), "separated_%d", K);
    const std::vector<double> G = with_spectrum(d, 1000 + K);
    check_matrix(name, G, K, true, &lam, &U);
    for (int k = 0; k < K && !lam.empty(); ++k) CHECK(std::fabs(lam[k] - d[k]) <= 1e-12 * d[0], "%s: lambda[%d] = %.17g, want %.17g", name, k, lam[k], d[k]);
    std::vector<double> lam_b, U_b;   // the same bits on a second call
    check_matrix(name, G, K, true, &lam_b, &U_b);
    CHECK(lam == lam_b && U == U_b, "%s: two calls differ", name);
  }
  // a repeated eigenvalue and a rank-deficient matrix: residual and orthogonality only
  {
    std::vector<double> d = {5.0, 3.0, 3.0, 3.0, 1.0, 1.0, 0.5};
    check_matrix("repeated", with_spectrum(d, 77), (int)d.size(), false);
    std::vector<double> z(40, 0.0);
    for (int k = 0; k < 25; ++k) z[k] = 1.0 + k;
    check_matrix("rank_deficient", with_spectrum(z, 78), 40, false, &lam, &U);
    for (int k = 25; k < 40 && !lam.empty(); ++k) CHECK(std::fabs(lam[k]) <= 1e-12 * 25.0, "rank_deficient: lambda[%d] = %g", k, lam[k]);
    std::vector<double> zero(9, 0.0);
    check_matrix("zero", zero, 3, false, &lam, &U);
  }
  // refusals
  {
    double a = 1.0, l = 0.0;
    CHECK(pmf_eig_sym(nullptr, 1, &l, nullptr, nullptr) == -1 && pmf_eig_sym(&a, 0, &l, nullptr, nullptr) == -1 &&
              pmf_eig_sym(&a, PMF_EIG_MAX_K + 1, &l, nullptr, nullptr) == -1,
          "bad arguments are not refused");
    a = NAN;
    CHECK(pmf_eig_sym(&a, 1, &l, nullptr, nullptr) == -2, "a NaN matrix is not refused");
  }
  std::printf(g_fail ? "EIG %d checks FAILED\n" : "EIG all checks passed\n", g_fail);
  return g_fail ? 1 : 0;
}
