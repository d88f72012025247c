// pmf_k_fused.hip -- pmf_fused_kernel for ONE (K blocks, row blocks per wave) pair, chosen at compile time
// (-DPMF_KB=.. -DPMF_RBW=..; csrc/Makefile builds the five pairs in parallel), and its launcher.  Which instance a pass
// runs is decided on the host (fused_geometry, pmf_pass.hip) by the rules of pmf_common.h (pmf_exact_gm_built,
// pmf_exact_has_xw, pmf_exact_has_xr); this unit builds the instances those rules allow and selects among them by the
// FusedInstance it is handed.  It reads no switch and reports nothing back.
#ifndef PMF_KB
#error "compile with -DPMF_KB=<1..4> -DPMF_RBW=<1|2> -DPMF_DB=<0|1>"
#endif
#ifndef PMF_DB
#define PMF_DB 0
#endif
#include "pmf_common.h"
#include "pmf_fused.hip.inc"

constexpr int KB = PMF_KB, NW = PMF_KB <= 2 ? 8 : 4, RBW = PMF_RBW;
constexpr bool DB = PMF_DB != 0;

// the instance (BM, MX, GM, i.xw, i.xr), or null where it is not built
template <int BM, bool MX, int GM>
static FusedKernel pick_xw(const FusedInstance &i) {
  if constexpr (!pmf_exact_gm_built(BM, GM)) return nullptr;
  else {
    if constexpr (pmf_exact_has_xw(KB, NW, RBW, BM, MX, GM, DB)) {
      if constexpr (pmf_exact_has_xr(KB, NW, RBW, BM, MX, GM, DB))
        if (i.xw && i.xr) return pmf_fused_kernel<KB, NW, RBW, BM, MX, GM, DB, true, true>;
      if (i.xw && !i.xr) return pmf_fused_kernel<KB, NW, RBW, BM, MX, GM, DB, true, false>;
    }
    if (i.xw || i.xr) return nullptr;
    return pmf_fused_kernel<KB, NW, RBW, BM, MX, GM, DB>;
  }
}
template <int BM, bool MX>
static FusedKernel pick_gm(const FusedInstance &i) {
  switch (i.gm) {
    case 0: return pick_xw<BM, MX, 0>(i);
    case 1: return pick_xw<BM, MX, 1>(i);
    case 2: return pick_xw<BM, MX, 2>(i);
    case 3: return pick_xw<BM, MX, 3>(i);
  }
  return nullptr;
}
template <int BM>
static FusedKernel pick_mixed(const FusedInstance &i) { return i.mixed ? pick_gm<BM, true>(i) : pick_gm<BM, false>(i); }

template <>
int pmf_launch_fused<0, KB, RBW, DB>(PmfDynLds *cache, hipStream_t stream, const FusedArgs &a, int grid, const FusedInstance &i) {
  using Cfg = FusedCfg<KB, NW, RBW>;
  const size_t lds = Cfg::lds_bytes + (i.bmode != 0 ? Cfg::lds_batch_extra : 0);
  const FusedKernel kern = i.bmode == 0 ? pick_mixed<0>(i) : (i.bmode == 1 ? pick_mixed<1>(i) : (i.bmode == 2 ? pick_mixed<2>(i) : nullptr));
  if (!kern)
    return pmf_fail("pmf_fused_kernel<%d, %d, %d>: no instance bmode %d, mixed %d, gm %d, bf16 %d, xw %d, xr %d is built", KB, NW, RBW,
                    i.bmode, (int)i.mixed, i.gm, (int)DB, (int)i.xw, (int)i.xr);
  PMFCHK(pmf_ensure_dyn_lds(cache, (const void *)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}
