// pmf_k_sb4.hip -- pmf_fused_sb4_kernel (64 < K <= 128) for one K-block count and one storage type of D
// (-DPMF_KB=4 -DPMF_DB=0|1), k_sb4_split, and their launchers.
#ifndef PMF_KB
#error "compile with -DPMF_KB=<3|4> -DPMF_DB=<0|1>"
#endif
#ifndef PMF_DB
#define PMF_DB 0
#endif
#include "pmf_common.h"
#include "pmf_fused_sb4.hip.inc"
#include "pmf_split_launch.h"

template <bool MIXED, bool GX, bool GY, bool BATCH>
struct Sb4Kern {
  static FusedKernel fn() { return pmf_fused_sb4_kernel<PMF_KB, MIXED, GX, GY, BATCH, PMF_DB != 0>; }
};
template <>
int pmf_launch_fused<4, PMF_KB, 1, PMF_DB != 0>(PmfDynLds *cache, hipStream_t stream, const FusedArgs &a, int grid, const FusedInstance &i) {
  return pmf_launch_split<Sb4Kern>(cache, stream, a, grid, i, 256, Sb4Cfg<PMF_KB>::lds_bytes + (i.bmode ? Sb4Cfg<PMF_KB>::lds_batch(a.n_bv) : 0));
}

#if !PMF_DB && PMF_KB == 4   // (one copy: see k_sb4_split)
int pmf_launch_sb4_split(hipStream_t stream, const Sb4SplitArgs &a) {
  if (a.nblk <= 0) return 0;
  k_sb4_split<<<(unsigned)a.nblk, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}
#endif
