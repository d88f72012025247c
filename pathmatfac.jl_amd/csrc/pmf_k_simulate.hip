// pmf_k_simulate.hip -- pmf_impute_kernel with the sampling epilogue SimEpi (pmf_simulate.hip.inc) and its launcher.
#include "pmf_common.h"
#define PMF_IMPUTE_KERNEL_ONLY
#include "pmf_impute.hip.inc"
#include "pmf_simulate.hip.inc"

template <int KB, int NW, int FORM>
static int launch_form(PmfDynLds *cache, hipStream_t stream, int grid, const ImputeArgs &a, const SimArgs &s) {
  void (*kern)(const ImputeArgs, const SimEpi<FORM>) = pmf_impute_kernel<KB, NW, false, SimEpi<FORM>>;
  const size_t lds = ImputeCfg<KB, NW>::lds((a.flags & PMF_IMPUTE_BATCH) != 0 && a.n_bv > 0);
  PMFCHK(pmf_ensure_dyn_lds(cache, (const void *)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), lds, stream, a, SimEpi<FORM>{s});
  HIPCHK(hipGetLastError());
  return 0;
}

template <int KB, int NW>
static int launch_kb(PmfDynLds *cache, hipStream_t stream, int form, int grid, const ImputeArgs &a, const SimArgs &s) {
  switch (form) {
    case PMF_SIM_COLMAJOR: return launch_form<KB, NW, PMF_SIM_COLMAJOR>(cache, stream, grid, a, s);
    case PMF_SIM_TILE_F32: return launch_form<KB, NW, PMF_SIM_TILE_F32>(cache, stream, grid, a, s);
    case PMF_SIM_TILE_BF16: return launch_form<KB, NW, PMF_SIM_TILE_BF16>(cache, stream, grid, a, s);
    default: return pmf_fail("pmf_simulate_data: unknown store form %d", form);
  }
}

// (KB, NW) as pmf_launch_impute pairs them: pmf_impute_waves
int pmf_launch_simulate(PmfDynLds *cache, hipStream_t stream, int KB, int form, int grid, const ImputeArgs &a, const SimArgs &s) {
  switch (KB) {
    case 1: return launch_kb<1, 8>(cache, stream, form, grid, a, s);
    case 2: return launch_kb<2, 8>(cache, stream, form, grid, a, s);
    case 3: return launch_kb<3, 4>(cache, stream, form, grid, a, s);
    case 4: return launch_kb<4, 4>(cache, stream, form, grid, a, s);
    default: return pmf_fail("pmf_simulate_data: unsupported KB=%d", KB);
  }
}
