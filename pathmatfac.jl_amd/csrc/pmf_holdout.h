// pmf_holdout.h -- the hold-out pass (pmf_holdout.hip.inc, pmf_k_holdout.hip) and its host side (pmf_holdout.hip): argument
// structs and launchers.  include/pmf_hip_holdout.h has the model and the order of every sum.
#ifndef PMF_HOLDOUT_H
#define PMF_HOLDOUT_H
#include "pmf_common.h"

#define PMF_HOLDOUT_UNIT_DEFAULT 512   // entries of a work unit (one wave sweeps a unit, four entries at a time)

// the set's walk over the resident D, one wave per column: read the entries' values, blank them, write them back
#define PMF_HOLDOUT_D_GATHER 0
#define PMF_HOLDOUT_D_BLANK 1
#define PMF_HOLDOUT_D_RESTORE 2
struct HoldoutDArgs {
  void *D;                 // tile-major f32 (pmf_d_off) or bf16 (pmf_d_off16)
  int32_t d_bf16, mode;
  int64_t nRB, N;
  const int64_t *colptr;   // [N + 1]
  const int32_t *rows;     // 0-based, ascending inside a column
  float *vals;             // written by GATHER, read by RESTORE
};

struct HoldoutPassArgs {
  const float *X, *Y;
  const float4 *colp;      // per column {sigma, mu, weight, meta}
  const float *htab;       // per column the PMF_HT class bounds of the kind-3 columns; null while every column is normal
  const int32_t *bor;      // n_bv x M row -> batch (or -1)
  const float2 *btab;
  const ViewDesc *views;   // device array [n_bv]
  const int32_t *rows;
  const float *vals;
  const int32_t *u_col, *u_cnt;   // per unit: its column, its entries
  const int64_t *u_e0;            //           its first entry
  float *lbuf;             // [n] the loss of every entry
  int64_t M;
  int32_t n_units, n_bv, Kp;
};

// lbuf -> loss_col (one wave per column), then loss_col -> *total (one thread, ascending columns)
struct HoldoutSumArgs {
  const float *lbuf;
  const int64_t *colptr;
  int64_t N;
  double *loss_col;        // [N]
  double *total;
};

int pmf_launch_holdout_d(hipStream_t stream, int grid, const HoldoutDArgs &a);
int pmf_launch_holdout_pass(hipStream_t stream, int grid, const HoldoutPassArgs &a);
int pmf_launch_holdout_sums(hipStream_t stream, int grid, const HoldoutSumArgs &a);
#endif
