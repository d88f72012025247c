// pmf_k_sb2.hip -- pmf_fused_sb2_kernel (32 < K <= 64; four waves x two row blocks) for one storage type of D
// (-DPMF_DB=0|1) and its launcher.
#ifndef PMF_DB
#define PMF_DB 0
#endif
#include "pmf_common.h"
#include "pmf_fused_sb2.hip.inc"
#include "pmf_split_launch.h"

template <bool MIXED, bool GX, bool GY, bool BATCH>
struct Sb2Kern {
  static FusedKernel fn() { return pmf_fused_sb2_kernel<MIXED, GX, GY, BATCH, PMF_DB != 0>; }
};
template <>
int pmf_launch_fused<2, 2, 2, PMF_DB != 0>(PmfDynLds *cache, hipStream_t stream, const FusedArgs &a, int grid, const FusedInstance &i) {
  return pmf_launch_split<Sb2Kern>(cache, stream, a, grid, i, 256, Sb2Cfg::lds_bytes + (i.bmode ? Sb2Cfg::lds_batch(a.n_bv) : 0));
}
