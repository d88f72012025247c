// pmf_k_impute.hip -- pmf_impute_kernel + k_impute_entries (pmf_impute.hip.inc) and their launchers.
#include "pmf_common.h"
#include "pmf_impute.hip.inc"

int pmf_impute_waves(int KB) { return KB <= 2 ? 8 : 4; }

int pmf_launch_impute(PmfDynLds *cache, hipStream_t stream, int KB, bool d_bf16, int grid, const ImputeArgs &a) {
  void (*kern)(const ImputeArgs, const ImputeEpi) = nullptr;
  size_t lds = 0;
  const bool batch = (a.flags & PMF_IMPUTE_BATCH) != 0 && a.n_bv > 0;
  // the storage type of D matters to PMF_IMPUTE_KEEP_OBSERVED alone
  const bool db = d_bf16 && (a.flags & PMF_IMPUTE_KEEP_OBSERVED) != 0;
#define PMF_IK(KBv, NWv) kern = db ? pmf_impute_kernel<KBv, NWv, true> : pmf_impute_kernel<KBv, NWv, false>; lds = ImputeCfg<KBv, NWv>::lds(batch)
  switch (KB) {
    case 1: PMF_IK(1, 8); break;
    case 2: PMF_IK(2, 8); break;
    case 3: PMF_IK(3, 4); break;
    case 4: PMF_IK(4, 4); break;
    default: return pmf_fail("pmf_impute: unsupported KB=%d", KB);
  }
#undef PMF_IK
  PMFCHK(pmf_ensure_dyn_lds(cache, (const void *)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * pmf_impute_waves(KB)), lds, stream, a, ImputeEpi{});
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_impute_entries(hipStream_t stream, const ImputeEntriesArgs &a) {
  if (a.n <= 0) return 0;
  k_impute_entries<<<(unsigned)((a.n + 255) / 256), 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
