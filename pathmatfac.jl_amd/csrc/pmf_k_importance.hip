// pmf_k_importance.hip -- pmf_importance_kernel + k_importance_reduce (pmf_importance.hip.inc) and their launchers.
#include "pmf_importance.h"
#include "pmf_importance.hip.inc"

// The [Kp + 4][32] accumulation panels stand beside the X panels: eight waves fit up to K = 64 (146 KiB at K = 64), four
// above (150 KiB at K = 128; eight would need 282 KiB).
int pmf_importance_waves(int KB) { return KB <= 2 ? 8 : 4; }

size_t pmf_importance_lds(int KB) {
  switch (KB) {
    case 1: return ImportanceCfg<1, 8>::lds;
    case 2: return ImportanceCfg<2, 8>::lds;
    case 3: return ImportanceCfg<3, 4>::lds;
    default: return ImportanceCfg<4, 4>::lds;
  }
}

int pmf_launch_importance(PmfDynLds *cache, hipStream_t stream, int KB, bool d_bf16, int grid, const ImportanceArgs &a) {
  void (*kern)(const ImportanceArgs) = nullptr;
#define PMF_FK(KBv, NWv) kern = d_bf16 ? pmf_importance_kernel<KBv, NWv, true> : pmf_importance_kernel<KBv, NWv, false>
  switch (KB) {
    case 1: PMF_FK(1, 8); break;
    case 2: PMF_FK(2, 8); break;
    case 3: PMF_FK(3, 4); break;
    case 4: PMF_FK(4, 4); break;
    default: return pmf_fail("pmf_factor_importance: unsupported KB=%d", KB);
  }
#undef PMF_FK
  const size_t lds = pmf_importance_lds(KB);
  // dynamic + static LDS against what a workgroup can have
  hipFuncAttributes fa;
  HIPCHK(hipFuncGetAttributes(&fa, (const void *)kern));
  if (lds + fa.sharedSizeBytes > PMF_IMP_LDS_LIMIT)
    return pmf_fail("pmf_factor_importance: %zu + %zu bytes of LDS exceed the %d of a workgroup", lds, (size_t)fa.sharedSizeBytes, PMF_IMP_LDS_LIMIT);
  PMFCHK(pmf_ensure_dyn_lds(cache, (const void *)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * pmf_importance_waves(KB)), lds, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_importance_reduce(hipStream_t stream, const ImportanceReduceArgs &a) {
  const int64_t n = (int64_t)a.n_ct * pmf_imp_rows(a.KB) * 32;
  k_importance_reduce<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
