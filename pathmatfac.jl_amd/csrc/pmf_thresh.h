// pmf_thresh.h -- the threshold pass of the squared-hinge noise models (pmf_thresh.hip.inc, pmf_k_thresh.hip) and its host
// side (pmf_thresh.hip): argument structs and launchers.  include/pmf_hip_thresholds.h has the model.
#ifndef PMF_THRESH_H
#define PMF_THRESH_H
#include "pmf_common.h"

#define PMF_TSLOT 96   // floats of one slot: [32 columns of the tile][3 thresholds]

struct ThreshPassArgs {
  const void *D;           // tile-major f32 or bf16 (d_bf16)
  int32_t d_bf16;
  int64_t nRB;
  const float *X, *Y;
  const float4 *colp;
  const float *htab;       // per column the PMF_HT class bounds (pmf_hinge_terms)
  const int32_t *bor;      // n_bv x M row -> batch (or -1)
  const float2 *btd;       // dense batch table [N padded to 32][1 << nbs_shift]; null without batch views
  const int32_t *tiles;    // [n_tiles] the column tiles that hold a kind-3 column, ascending
  float *slots;            // [R * NW][n_tiles][PMF_TSLOT]: one slot PRIVATE to (row range, wave, tile), every one written
  int64_t M, N;
  int32_t n_bv, n_tiles, n_rp, R, nbs_shift;
};

// slots -> per column float64 sums (fixed order: row range, then wave) -> per group float64 sums (ascending columns)
struct ThreshReduceArgs {
  const float *slots;
  const int32_t *tiles;
  const float4 *thr;          // per column {t0, t1, t2, 0}
  int32_t n_tiles, n_parts;   // n_parts = R * NW
  int64_t N;
  double *gcol;               // [3 N] g_t[m][j] at 3 j + m, written for the tiles' columns; 0 for an infinite threshold
  const int64_t *g_c0, *g_c1; // [n_groups] 0-based first column, one past the last
  int32_t n_groups;
  double *G;                  // [3 n_groups]
};

// optimizer step of the thresholds (k_reg_step's expressions), the order clamp, and the per-column images
struct ThreshStepArgs {
  float *t, *acc, *mom;       // [3 n_groups]
  const double *G;
  int32_t n_groups, opt_kind;
  float lr, eps, b1, b2, c1, c2;
};
struct ThreshImageArgs {
  const float *t;             // [3 n_groups]
  const int32_t *col_group;
  int64_t N;
  float4 *thr;
  float *htab;
};

struct ClassCountArgs {
  const void *D;
  int32_t d_bf16;
  int64_t nRB, M, N;
  const int64_t *c0, *c1;     // [n_ranges] 0-based first column, one past the last
  int32_t n_ranges, row_chunks;
  unsigned long long *counts; // [4 n_ranges], zeroed before the launch
};

size_t pmf_thresh_pass_lds(int KB, int nw, int nbs);
int pmf_thresh_waves(int KB);   // 8 up to K = 64, 4 above (as the layer pass)
int pmf_launch_thresh_pass(PmfDynLds *cache, hipStream_t stream, int KB, int grid, const ThreshPassArgs &a);
int pmf_launch_thresh_reduce(hipStream_t stream, const ThreshReduceArgs &a);
int pmf_launch_thresh_step(hipStream_t stream, const ThreshStepArgs &a);
int pmf_launch_thresh_images(hipStream_t stream, const ThreshImageArgs &a);
int pmf_launch_class_counts(hipStream_t stream, const ClassCountArgs &a);
#endif
