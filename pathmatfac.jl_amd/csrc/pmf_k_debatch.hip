// pmf_k_debatch.hip -- pmf_debatch_kernel + k_debatch_entries (pmf_debatch.hip.inc) and their launchers.
#include "pmf_common.h"
#include "pmf_debatch.hip.inc"

#include <algorithm>

// Persistent grid: workgroups of four waves, each wave striding over the 32 x 32 tiles; PMF_DEBATCH_WG_PER_CU resident
// workgroups per CU keep enough 16-byte loads in flight to cover HBM latency (the kernel holds no LDS and few registers).
#define PMF_DEBATCH_WG_PER_CU 4

int pmf_launch_debatch(hipStream_t stream, int src, int n_cu, const DebatchArgs &a) {
  const int64_t units = a.n_rb * a.n_ct;
  if (units <= 0) return 0;
  void (*kern)(const DebatchArgs) = src == 0 ? pmf_debatch_kernel<0> : (src == 1 ? pmf_debatch_kernel<1> : pmf_debatch_kernel<2>);
  const int grid = (int)std::min<int64_t>((units + 3) / 4, (int64_t)PMF_DEBATCH_WG_PER_CU * std::max(n_cu, 1));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_debatch_entries(hipStream_t stream, const DebatchEntriesArgs &a) {
  if (a.n <= 0) return 0;
  k_debatch_entries<<<(unsigned)((a.n + 255) / 256), 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
