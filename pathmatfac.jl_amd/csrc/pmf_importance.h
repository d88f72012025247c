// pmf_importance.h -- the factor-importance pass (pmf_importance.hip.inc, pmf_k_importance.hip) and its host side
// (pmf_outputs.hip): argument structs and launchers.  include/pmf_hip_importance.h has the definition.
#ifndef PMF_IMPORTANCE_H
#define PMF_IMPORTANCE_H
#include "pmf_common.h"

#define PMF_IMP_FLUSH 16   // row panels of a unit between two float64 flushes: 32 entries per slot and panel -> PMF_IMPORTANCE_CHAIN = 512
#define PMF_IMP_LDS_LIMIT (160 * 1024)   // LDS of a gfx950 workgroup

// rows of an accumulation panel: Kp per-factor sums, then full, null, n_obs and one spare row; 32 columns each
__host__ __device__ constexpr int pmf_imp_rows(int KB) { return 32 * KB + 4; }

struct ImportanceArgs {
  const void *D;           // tile-major f32 or bf16 (the instance's DB)
  int64_t nRB;
  const float *X, *Y;
  const float4 *colp;      // {sigma, mu, weight, meta}
  const float *htab;       // per column the PMF_HT class bounds (pmf_hinge_terms); null while every column is normal
  const int32_t *bor;      // n_bv x M row -> batch (or -1)
  const float2 *btab;      // {delta, theta}, view v at views[v].tab_off, nb x Nv column-major
  const ViewDesc *views;   // device array [n_bv]
  double *slabs;           // [n_ct][R][pmf_imp_rows][32]: one slab PRIVATE to (column tile of the launch, row range)
  int64_t M, N;
  int32_t K, n_bv;
  int32_t ct0, n_ct;       // the launch's column tiles [ct0, ct0 + n_ct)
  int32_t n_rp, R;         // row panels of 32 NW rows, row ranges
};

// slabs -> the outputs: per (column, panel row) the row ranges in ascending order, float64
struct ImportanceReduceArgs {
  const double *slabs;
  int32_t ct0, n_ct, R, KB, K;
  int64_t N;
  double *delta;           // [N][K] factor fastest
  double *full, *null_, *n_obs;   // [N]
};

int pmf_importance_waves(int KB);    // 8 up to K = 64, 4 above
size_t pmf_importance_lds(int KB);   // dynamic LDS of the instance
int pmf_launch_importance(PmfDynLds *cache, hipStream_t stream, int KB, bool d_bf16, int grid, const ImportanceArgs &a);
int pmf_launch_importance_reduce(hipStream_t stream, const ImportanceReduceArgs &a);
#endif
