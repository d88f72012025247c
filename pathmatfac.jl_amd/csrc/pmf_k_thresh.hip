// pmf_k_thresh.hip -- pmf_thresh_kernel and the small kernels of the threshold pass (pmf_thresh.hip.inc), their launchers.
#include "pmf_thresh.h"
#include "pmf_thresh.hip.inc"

int pmf_thresh_waves(int KB) { return KB <= 2 ? 8 : 4; }

size_t pmf_thresh_pass_lds(int KB, int nw, int nbs) {
  switch (KB) {
    case 1: return ThreshCfg<1, 8>::lds(nbs);
    case 2: return ThreshCfg<2, 8>::lds(nbs);
    case 3: return ThreshCfg<3, 4>::lds(nbs);
    default: return ThreshCfg<4, 4>::lds(nbs);
  }
}

int pmf_launch_thresh_pass(PmfDynLds *cache, hipStream_t stream, int KB, int grid, const ThreshPassArgs &a) {
  void (*kern)(const ThreshPassArgs) = nullptr;
#define PMF_TK2(KBv, NWv, Wv) (a.d_bf16 ? pmf_thresh_kernel<KBv, NWv, true, Wv> : pmf_thresh_kernel<KBv, NWv, false, Wv>)
#define PMF_TK(KBv, NWv) (a.nbs_shift > 4 ? PMF_TK2(KBv, NWv, true) : PMF_TK2(KBv, NWv, false))
  switch (KB) {
    case 1: kern = PMF_TK(1, 8); break;
    case 2: kern = PMF_TK(2, 8); break;
    case 3: kern = PMF_TK(3, 4); break;
    case 4: kern = PMF_TK(4, 4); break;
    default: return pmf_fail("the threshold pass is built for K <= 128 (KB = %d)", KB);
  }
#undef PMF_TK
#undef PMF_TK2
  const int nw = pmf_thresh_waves(KB);
  const size_t lds = pmf_thresh_pass_lds(KB, nw, 1 << a.nbs_shift);
  PMFCHK(pmf_ensure_dyn_lds(cache, (const void *)kern, lds));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_thresh_reduce(hipStream_t stream, const ThreshReduceArgs &a) {
  const int64_t n = (int64_t)a.n_tiles * PMF_TSLOT;
  k_thresh_cols<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  k_thresh_groups<<<(unsigned)a.n_groups, 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_thresh_step(hipStream_t stream, const ThreshStepArgs &a) {
  k_thresh_step<<<(unsigned)((a.n_groups + 63) / 64), 64, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_thresh_images(hipStream_t stream, const ThreshImageArgs &a) {
  k_thresh_images<<<(unsigned)((a.N + 255) / 256), 256, 0, stream>>>(a);
  HIPCHK(hipGetLastError());
  return 0;
}

int pmf_launch_class_counts(hipStream_t stream, const ClassCountArgs &a) {
  k_class_counts<<<dim3((unsigned)((a.N + 63) / 64), (unsigned)a.row_chunks), 64, 0, stream>>>(a);   // (a.counts: zeroed by the caller)
  HIPCHK(hipGetLastError());
  return 0;
}
