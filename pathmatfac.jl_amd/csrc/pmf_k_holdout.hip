// pmf_k_holdout.hip -- k_holdout_d, k_holdout_pass, k_holdout_colsum, k_holdout_total (pmf_holdout.hip.inc) and their launchers.
#include "pmf_holdout.h"
#include "pmf_holdout.hip.inc"

int pmf_launch_holdout_d(hipStream_t stream, int grid, const HoldoutDArgs &a) {
  k_holdout_d<<<grid, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_holdout_pass(hipStream_t stream, int grid, const HoldoutPassArgs &a) {
  if (a.n_units <= 0) return 0;
  k_holdout_pass<<<grid, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_holdout_sums(hipStream_t stream, int grid, const HoldoutSumArgs &a) {
  k_holdout_colsum<<<grid, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  k_holdout_total<<<1, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
