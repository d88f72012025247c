// pmf_split_launch.h -- the instance selection that the launchers of the split-bf16 families sb, sb2 and sb4 share
// (pmf_k_sb.hip, pmf_k_sb2.hip, pmf_k_sb4.hip).  Each unit names its kernels through
//   template <bool MIXED, bool GX, bool GY, bool BATCH> struct Kern { static FusedKernel fn(); };
// and calls pmf_launch_split<Kern>.  (sb8 has one gradient variant and selects for itself, pmf_k_sb8.hip.)
#ifndef PMF_SPLIT_LAUNCH_H
#define PMF_SPLIT_LAUNCH_H
#include "pmf_common.h"

template <template <bool, bool, bool, bool> class Kern, bool MIXED, bool BATCH>
static FusedKernel pmf_split_pick_gm(int gm) {
  switch (gm) {
    case 0: return Kern<MIXED, true, true, BATCH>::fn();
    case 1: return Kern<MIXED, true, false, BATCH>::fn();
    case 2: return Kern<MIXED, false, true, BATCH>::fn();
  }
  return nullptr;   // (no run-time gradient flags: fused_geometry sends a pass without gradients to the exact kernel)
}

// lds: the family's dynamic LDS for this pass, its batch tables included
template <template <bool, bool, bool, bool> class Kern>
static int pmf_launch_split(PmfDynLds *cache, hipStream_t stream, const FusedArgs &a, int grid, const FusedInstance &i, int threads, size_t lds) {
  // (the batch-layer variants exist with the per-tile noise-model dispatch only: MIXED = true also serves uniform models;
  //  there is no gather fallback, bmode 2, and nothing of the exact kernel's xw / xr)
  const FusedKernel kern = i.xw || i.xr ? nullptr
                           : i.bmode == 1 ? pmf_split_pick_gm<Kern, true, true>(i.gm)
                           : i.bmode != 0 ? nullptr
                           : i.mixed ? pmf_split_pick_gm<Kern, true, false>(i.gm) : pmf_split_pick_gm<Kern, false, false>(i.gm);
  if (!kern) return pmf_fail("split-bf16 kernel: no instance bmode %d, mixed %d, gm %d, xw %d, xr %d is built", i.bmode, (int)i.mixed, i.gm, (int)i.xw, (int)i.xr);
  PMFCHK(pmf_ensure_dyn_lds(cache, (const void *)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}
#endif
