// pmf_k_sb.hip -- pmf_fused_sb_kernel and k_sb_split for ONE K-block count (-DPMF_KB=1|2), with their launchers.
#include "pmf_common.h"
#include "pmf_fused_sb.hip.inc"
#include "pmf_split_launch.h"

#ifndef PMF_KB
#error "compile with -DPMF_KB=<1|2>"
#endif
#ifndef PMF_DB
#define PMF_DB 0
#endif

template <bool MIXED, bool GX, bool GY, bool BATCH>
struct SbKern {
  static FusedKernel fn() { return pmf_fused_sb_kernel<PMF_KB, MIXED, GX, GY, BATCH, PMF_DB != 0>; }
};
template <>
int pmf_launch_fused<1, PMF_KB, 1, PMF_DB != 0>(PmfDynLds *cache, hipStream_t stream, const FusedArgs &a, int grid, const FusedInstance &i) {
  return pmf_launch_split<SbKern>(cache, stream, a, grid, i, 512, SbCfg<PMF_KB>::lds_bytes + (i.bmode ? SbCfg<PMF_KB>::lds_batch(a.n_bv) : 0));
}

#if !PMF_DB
template <>
int pmf_launch_sb_split<PMF_KB>(hipStream_t stream, const SbSplitArgs &a) {
  const int64_t n = a.nblk * 32 * (4 * PMF_KB);   // one thread per (row, 16-B chunk)
  k_sb_split<PMF_KB><<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
#endif
