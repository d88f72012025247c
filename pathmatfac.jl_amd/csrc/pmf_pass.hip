// pmf_pass.hip -- host driver of the fused data pass: tile flags and the fixed-order gX / gY reductions, the work split, the
// kernel-family table with its geometry, buffers, extents guard and launches, and the debug entries that read the pass state.
// fused_geometry decides a pass once: the PMF_* switches (read_pass_switches), the family (fused_families) and the instance
// of its kernel (FusedInstance, by the rules of pmf_common.h).  Buffers, extents, kernel arguments, the launcher's selection
// and the diagnostics read that FusedGeom and decide nothing again.
#include "pmf_ctx.h"

// One workgroup per 32x32 tile of the tile-major D: flag = 1 iff all 1024 entries are finite.  The fused kernel takes
// its packed-math epilogue (no per-entry missing-value mask) on flagged tiles.  Recomputed lazily whenever D changes.
__global__ void k_tile_flags(const void *__restrict__ D, int64_t ntiles, uint32_t *__restrict__ flags, int bf16) {
  const int64_t t = blockIdx.x;
  if (t >= ntiles) return;
  bool ok;
  if (bf16) {   // 256 threads x 8 B; finite <=> the exponent field is not all ones
    const uint2 v = reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(D) + t * 1024)[threadIdx.x];
    ok = (v.x & 0x7f80u) != 0x7f80u && (v.x & 0x7f800000u) != 0x7f800000u && (v.y & 0x7f80u) != 0x7f80u && (v.y & 0x7f800000u) != 0x7f800000u;
  } else {
    const float4 v = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(D) + t * 1024)[threadIdx.x];   // 256 threads x 16 B
    ok = fabsf(v.x) <= 3.402823466e38f && fabsf(v.y) <= 3.402823466e38f && fabsf(v.z) <= 3.402823466e38f && fabsf(v.w) <= 3.402823466e38f;
  }
  const int all_ok = __syncthreads_and(ok ? 1 : 0);
  if (threadIdx.x == 0) flags[t] = all_ok ? 1u : 0u;
}

static int ensure_tile_flags(pmf_ctx *c) {
  if (c->tflags_valid) return 0;
  const int64_t ntiles = c->nRB * (c->D_Npad / 32);
  PMFCHK(c->tflags.ensure((size_t)ntiles, false));
  if (ntiles > 0x7fffffff) return pmf_fail("too many tiles");
  k_tile_flags<<<(unsigned)ntiles, 256, 0, c->stream>>>(c->D, ntiles, c->tflags, c->store == PMF_STORE_BF16);
  HIPCHK(hipGetLastError());
  c->tflags_valid = true;
  c->ptab_bm = 0;   // the plain-run table was made from the old flags
  return 0;
}

// The plain-run table of the exact kernel (pmf_fused.hip.inc, "Plain runs"): one workgroup per row panel of nblk row
// blocks walks the panel's column tiles in strips of 256 and writes, for every column tile c, the number of tiles < c
// with a row block that is absent or not flagged all-finite: out[rp][0 .. n_ct].  A run of tiles [c0, c1) of the panel
// is all-finite iff out[rp][c1] == out[rp][c0].  Like the flags it is made once per data matrix, not per pass.
__global__ __launch_bounds__(256) void k_plain_table(const uint32_t *__restrict__ flags, int64_t nRB, int nblk, int64_t n_ct,
                                                     int32_t *__restrict__ out) {
  __shared__ int sc[256];
  const int64_t rp = blockIdx.x;
  int32_t *o = out + rp * (n_ct + 1);
  int carry = 0;
  if (threadIdx.x == 0) o[0] = 0;
  for (int64_t c0 = 0; c0 < n_ct; c0 += 256) {
    const int64_t ct = c0 + threadIdx.x;
    int bad = 0;
    if (ct < n_ct)
      for (int r = 0; r < nblk; ++r) {
        const int64_t rb = rp * nblk + r;
        if (rb >= nRB || flags[ct * nRB + rb] == 0) bad = 1;
      }
    sc[threadIdx.x] = bad;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {   // inclusive scan of the strip
      const int v = threadIdx.x >= d ? sc[threadIdx.x - d] : 0;
      __syncthreads();
      sc[threadIdx.x] += v;
      __syncthreads();
    }
    if (ct < n_ct) o[ct + 1] = carry + sc[threadIdx.x];
    carry += sc[255];
    __syncthreads();
  }
}

// (after ensure_tile_flags) the table for panels of bm rows over n_ct column tiles; rebuilt when D, and with it the flags,
// changed, or when it was made for another panel height or shape
static int ensure_plain_table(pmf_ctx *c, int64_t bm, int64_t n_ct) {
  const int64_t n_rp = (c->M + bm - 1) / bm;
  if (c->ptab_bm == bm && c->ptab_n_rp == n_rp && c->ptab_n_ct == n_ct) return 0;
  if (n_ct + 1 > 0x7fffffff || n_rp > 0x7fffffff) return pmf_fail("too many tiles");
  PMFCHK(c->ptab.ensure((size_t)n_rp * (size_t)(n_ct + 1), false));
  k_plain_table<<<(unsigned)n_rp, 256, 0, c->stream>>>(c->tflags, c->nRB, (int)(bm / 32), n_ct, c->ptab);
  HIPCHK(hipGetLastError());
  c->ptab_bm = bm; c->ptab_n_rp = n_rp; c->ptab_n_ct = n_ct;
  return 0;
}

// gY = sum of the private slabs of the workgroups that visited a column tile, in workgroup order (fixed summation
// order: grad(Y) is bitwise reproducible).  The work sequence (pmf_fused_kernel) is segment-major, then row panel,
// then tile; workgroup g owns [g*T/G, (g+1)*T/G).  Inside segment cs (tiles [cs*S, cs*S + n_rp*tps_cs) of the
// sequence) it touched tile ti iff its range, taken relative to the segment start, contains an index == ti mod tps_cs.
__global__ __launch_bounds__(64) void k_gy_reduce(const float *__restrict__ slabs, int64_t stride,
                                                  const int32_t *__restrict__ c_off, const int32_t *__restrict__ c_idx,
                                                  int Kp, int64_t N, float *__restrict__ gY, int ct0,
                                                  const float4 *__restrict__ colscale) {   // non-null: the slabs hold sums NOT yet scaled by sigma_j (pmf_fused_sb8_kernel)
  // blockIdx.x = column tile of the chunk that starts at tile ct0, blockIdx.y = 256-float slice of its 32 x Kp elements (one float4 per thread).  The
  // workgroups that visited the tile are listed in c_idx[c_off[ct] .. c_off[ct+1]) (built on the host with the work
  // split, compute_work_split); their slabs are summed four at a time so that four independent loads are in flight.
  const int ct = blockIdx.x;   // (chunk-relative: indexes c_off)
  const int64_t e0 = (int64_t)(ct0 + ct) * 32 * Kp;
  const int64_t rem = (int64_t)Kp * N - e0;
  const int nel = rem > 32 * Kp ? 32 * Kp : (int)rem;   // a multiple of Kp, Kp a multiple of 32
  const int q = (blockIdx.y * 64 + threadIdx.x) * 4;
  if (q >= nel) return;
  const float *base = slabs + e0 + q;
  const int c0 = c_off[ct], n = c_off[ct + 1] - c0;
  const int32_t *ci = c_idx + c0;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
  int c = 0;
  for (; c + 4 <= n; c += 4) {   // fixed order: ((s0 + s4 + ...) + (s1 + s5 + ...)) + ... -> bitwise reproducible
    const float4 v0 = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c] * stride);
    const float4 v1 = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c + 1] * stride);
    const float4 v2 = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c + 2] * stride);
    const float4 v3 = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c + 3] * stride);
    a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
    a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
    a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
  }
  for (; c < n; ++c) {
    const float4 v = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c] * stride);
    a0.x += v.x; a0.y += v.y; a0.z += v.z; a0.w += v.w;
  }
  const float sg = colscale ? colscale[(e0 + q) / Kp].x : 1.f;   // (the four elements belong to one column: Kp is a multiple of 4)
  *reinterpret_cast<float4 *>(gY + e0 + q) =
      make_float4(((a0.x + a1.x) + (a2.x + a3.x)) * sg, ((a0.y + a1.y) + (a2.y + a3.y)) * sg, ((a0.z + a1.z) + (a2.z + a3.z)) * sg,
                  ((a0.w + a1.w) + (a2.w + a3.w)) * sg);
}

// gX = sum of the per-piece partial slabs of a row panel, in work-sequence order (fixed summation order: grad(X) is
// bitwise reproducible).  blockIdx.x = row panel, blockIdx.y = 256-float4 slice of its BM x Kp elements; the slots of
// the panel's pieces are listed in gx_idx[gx_off[rp] .. gx_off[rp+1]) (built on the host with the work split).
__global__ __launch_bounds__(256) void k_gx_reduce(const float *__restrict__ part, int64_t slot_stride,
                                                   const int32_t *__restrict__ gx_off, const int32_t *__restrict__ gx_idx,
                                                   int64_t panel_floats, int64_t total_floats, float *__restrict__ gX) {
  const int rp = blockIdx.x;
  const int64_t q = ((int64_t)blockIdx.y * 256 + threadIdx.x) * 4;
  if (q >= panel_floats) return;
  const int64_t e = (int64_t)rp * panel_floats + q;
  if (e >= total_floats) return;   // rows past M (Kp*M is a multiple of 4: a float4 is all in or all out)
  const int c0 = gx_off[rp], n = gx_off[rp + 1] - c0;
  const int32_t *ci = gx_idx + c0;
  const float *base = part + q;
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
  int c = 0;
  for (; c + 2 <= n; c += 2) {   // fixed order: (s0 + s2 + ...) + (s1 + s3 + ...)
    const float4 v0 = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c] * slot_stride);
    const float4 v1 = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c + 1] * slot_stride);
    a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
  }
  if (c < n) {
    const float4 v = *reinterpret_cast<const float4 *>(base + (int64_t)ci[c] * slot_stride);
    a0.x += v.x; a0.y += v.y; a0.z += v.z; a0.w += v.w;
  }
  *reinterpret_cast<float4 *>(gX + e) = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
}

// Cost-balanced split of the fused kernel's work sequence for one column chunk (tiles [ct0, ct0 + n_ct); sequence =
// segment-major, row panel, tile) into `grid` contiguous ranges.  A tile's estimated cost depends on the noise models of
// its 32 columns (measured on MI355X: a Bernoulli tile costs 1.4x a Gaussian one, Poisson 1.3x); with Gaussian-only
// data this is the even split g*T/G.  Also numbers the pieces (the part of one (segment, row panel) unit inside one
// workgroup's range) in sequence order: piece p of the chunk owns slot p of the chunk's gX partial slabs.
// Cost of a Bernoulli / Poisson tile in sixteenths of a Gaussian tile's, per kernel family and k-block count.  MEASURED: the
// weight that minimises the launch time at 100000 x 50000 with 20 % Bernoulli columns (scripts/kbench_mixed.py ... mixed under
// PMF_W_BERN=w; round 3).  It is not the ratio of the two tiles' times in isolation (1.19-1.58): the workgroups that own the
// Bernoulli columns do VALU work at the clock the OTHER workgroups' matrix work leaves them.  One weight for all kernels
// (22, right for the exact kernel at K = 64) cost the split kernels 7-22 % and the exact kernel at K <= 32 12 %.
// With batch layers EVERY tile pays the table look-ups (w_batch, from the batch-only against the plain launch at the same size),
// which lowers the Bernoulli tiles' relative weight.
// A squared-hinge tile always runs the per-column path (its thresholds are per column).  Its weight is UNMEASURED: it starts
// from the Poisson tile's (PMF_W_HINGE overrides it).
static void noise_tile_weights(const PassSwitches &sw, int KB, bool split, bool batch, int64_t &w_gauss, int64_t &w_bern, int64_t &w_pois, int64_t &w_hinge) {
  static const int64_t wb_exact[4] = {26, 22, 20, 20}, wb_split[4] = {31, 30, 24, 24};
  static const int64_t we_exact[4] = {6, 6, 5, 4}, we_split[4] = {12, 8, 6, 6};   // (swept on the all-features launch: PMF_W_BATCH)
  w_bern = (split ? wb_split : wb_exact)[KB - 1];
  if (sw.w_bern >= 0) w_bern = sw.w_bern;
  w_pois = 16 + ((w_bern - 16) * 5 + 3) / 6;       // (exp only against exp + log + rcp: the exact kernel's 21 against 22)
  if (sw.w_pois >= 0) w_pois = sw.w_pois;
  w_hinge = w_pois;                                // (unmeasured)
  if (sw.w_hinge >= 0) w_hinge = sw.w_hinge;
  int64_t w_batch = batch ? (split ? we_split : we_exact)[KB - 1] : 0;
  if (batch && sw.w_batch >= 0) w_batch = sw.w_batch;
  w_gauss = 16 + w_batch;
  w_bern += w_batch;
  w_pois += w_batch;
  w_hinge += w_batch;
}

static int compute_work_split(pmf_ctx *c, const PassSwitches &sw, WorkSplit &ws, int grid, int64_t n_rp, int64_t ct0, int64_t n_ct, int64_t tps, int64_t n_cseg, bool split) {
  int64_t w_gauss, w_bern, w_pois, w_hinge;
  noise_tile_weights(sw, c->KB, split, c->n_bv > 0, w_gauss, w_bern, w_pois, w_hinge);
  const int64_t key[11] = {c->M, c->N, c->Kp, grid, n_rp, tps, n_cseg, c->kind_version, ct0, n_ct,
                           c->mixed ? ((w_gauss * 64 + w_bern) * 64 + w_pois) * 64 + w_hinge : 0};
  if (ws.wg_begin && memcmp(key, ws.key, sizeof(key)) == 0) return 0;
  std::vector<int64_t> tw((size_t)n_ct, w_gauss);
  if (c->mixed && (int64_t)c->h_kind.size() == c->N) {
    for (int64_t ct = 0; ct < n_ct; ++ct) {
      int64_t wmax = w_gauss;
      for (int64_t j = (ct0 + ct) * 32; j < std::min<int64_t>(c->N, (ct0 + ct) * 32 + 32); ++j) {
        const int k = c->h_kind[(size_t)j];
        wmax = std::max<int64_t>(wmax, k == PMF_NOISE_BERNOULLI ? w_bern : (k == PMF_NOISE_POISSON ? w_pois : (k == PMF_NOISE_SQ_HINGE ? w_hinge : w_gauss)));
      }
      tw[(size_t)ct] = wmax;
    }
  }
  // per segment: first tile, tile count, weight of one row panel's sweep
  std::vector<int64_t> seg_t0((size_t)n_cseg), seg_nt((size_t)n_cseg), seg_w((size_t)n_cseg), seg_pref((size_t)n_cseg + 1, 0);
  for (int64_t cs = 0; cs < n_cseg; ++cs) {
    seg_t0[(size_t)cs] = cs * tps;
    seg_nt[(size_t)cs] = cs == n_cseg - 1 ? n_ct - cs * tps : tps;
    int64_t w = 0;
    for (int64_t t = 0; t < seg_nt[(size_t)cs]; ++t) w += tw[(size_t)(seg_t0[(size_t)cs] + t)];
    seg_w[(size_t)cs] = w;
    seg_pref[(size_t)cs + 1] = seg_pref[(size_t)cs] + w * n_rp;
  }
  const int64_t W = seg_pref[(size_t)n_cseg], T = n_rp * n_ct;
  std::vector<int64_t> wb((size_t)grid + 1, 0);
  for (int g = 1; g < grid; ++g) {
    const int64_t target = (int64_t)((__int128)W * g / grid);
    int64_t cs = 0;
    while (cs + 1 < n_cseg && seg_pref[(size_t)cs + 1] <= target) ++cs;
    int64_t rem = target - seg_pref[(size_t)cs];
    const int64_t rp = std::min<int64_t>(n_rp - 1, rem / seg_w[(size_t)cs]);
    rem -= rp * seg_w[(size_t)cs];
    int64_t ti = 0;
    while (ti + 1 < seg_nt[(size_t)cs] && rem >= tw[(size_t)(seg_t0[(size_t)cs] + ti)]) { rem -= tw[(size_t)(seg_t0[(size_t)cs] + ti)]; ++ti; }
    int64_t idx = cs * n_rp * tps + rp * seg_nt[(size_t)cs] + ti;
    idx = std::max(idx, wb[(size_t)g - 1]);      // monotone
    wb[(size_t)g] = std::min(idx, T);
  }
  wb[(size_t)grid] = T;
  // which workgroups visit a column tile: inside segment cs (items [s0, s1) of the sequence) workgroup g visits tile
  // ti iff its range, clipped to the segment, contains an index == ti modulo the segment's tile count
  std::vector<int32_t> h_off((size_t)n_ct + 1, 0), h_idx;
  for (int64_t ct = 0; ct < n_ct; ++ct) {
    const int64_t cs = std::min<int64_t>(ct / tps, n_cseg - 1);
    const int64_t tps_cs = seg_nt[(size_t)cs], ti = ct - cs * tps;
    const int64_t s0 = cs * n_rp * tps, s1 = s0 + n_rp * tps_cs;
    int g_lo = (int)(std::upper_bound(wb.begin(), wb.begin() + grid, s0) - wb.begin()) - 1;
    if (g_lo < 0) g_lo = 0;
    for (int g = g_lo; g < grid && wb[(size_t)g] < s1; ++g) {
      const int64_t lo = std::max(wb[(size_t)g], s0), hi = std::min(wb[(size_t)g + 1], s1);
      if (hi <= lo) continue;
      const int64_t first = (lo - s0) % tps_cs;
      const int64_t d = (ti - first + tps_cs) % tps_cs;
      if (d < hi - lo) h_idx.push_back(g);
    }
    h_off[(size_t)ct + 1] = (int32_t)h_idx.size();
  }
  if (h_idx.empty()) h_idx.push_back(0);
  // the pieces, walked exactly as the kernel walks them
  ws.h_piece_base.assign((size_t)grid, 0);
  ws.piece_rp.clear();
  const int64_t seg_block = n_rp * tps;
  for (int g = 0; g < grid; ++g) {
    ws.h_piece_base[(size_t)g] = (int32_t)ws.piece_rp.size();
    for (int64_t widx = wb[(size_t)g]; widx < wb[(size_t)g + 1];) {
      const int64_t cs = std::min<int64_t>(widx / seg_block, n_cseg - 1);
      const int64_t tps_cs = seg_nt[(size_t)cs];
      const int64_t rem = widx - cs * seg_block;
      const int64_t rp = rem / tps_cs, ti0 = rem - rp * tps_cs;
      widx += std::min<int64_t>(tps_cs - ti0, wb[(size_t)g + 1] - widx);
      ws.piece_rp.push_back((int32_t)rp);
    }
  }
  PMFCHK(ws.wg_begin.alloc((size_t)grid + 1, false));
  PMFCHK(ws.c_off.alloc((size_t)n_ct + 1, false));
  PMFCHK(ws.c_idx.alloc(h_idx.size(), false));
  PMFCHK(ws.piece_base.alloc((size_t)grid, false));
  PMFCHK(ws.d_piece_base_abs.alloc((size_t)grid, false));
  HIPCHK(hipMemcpyAsync(ws.wg_begin, wb.data(), sizeof(int64_t) * ((size_t)grid + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(ws.c_off, h_off.data(), sizeof(int32_t) * h_off.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(ws.c_idx, h_idx.data(), sizeof(int32_t) * h_idx.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));   // the sources are pageable host memory
  memcpy(ws.key, key, sizeof(key));
  ws.grid = grid; ws.tps = tps; ws.n_cseg = n_cseg;   // (all three are in the key)
  ws.serial = ++c->split_serial;
  return 0;
}

#ifdef PMF_STAMPS
static unsigned long long *g_stamps = nullptr;
extern "C" int pmf_debug_stamps(unsigned long long *out, int n) {
  if (!g_stamps) return -1;
  return hipMemcpy(out, g_stamps, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

int harvest_events(pmf_ctx *c) {
  for (size_t e = 0; e < c->ev_used; ++e) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev_pool[e].first, c->ev_pool[e].second) == hipSuccess) {
      c->kernel_ms_sum += ms;
      c->kernel_launches += 1;
    }
  }
  c->ev_used = 0;
  return 0;
}

// Panel-local batch slots for row panels of BM rows (PanelSlots): built on the host from the views' row -> batch maps,
// cached until a view's rows change.  Returns through ps.ok whether every (panel, view) has at most 15 distinct batches.
static int ensure_panel_slots(pmf_ctx *c, int BM, PanelSlots **out) {
  PanelSlots &ps = c->pslots[BM == 128 ? 0 : (BM == 256 ? 1 : 2)];
  *out = &ps;
  if (ps.serial == c->views_serial && ps.BM == BM) return 0;
  const int64_t n_rp = (c->M + BM - 1) / BM;
  std::vector<uint8_t> pm((size_t)(n_rp * c->n_bv * 16), 255), rs((size_t)((int64_t)c->n_bv * c->M), 15);
  bool ok = true;
  std::vector<int> slot_of;
  for (int v = 0; v < c->n_bv && ok; ++v) {
    if ((int64_t)c->h_bor[(size_t)v].size() != c->M) { ok = false; break; }
    const int32_t *bor = c->h_bor[(size_t)v].data();
    slot_of.assign((size_t)std::max<int>(c->views[v].nb, 1), -1);
    for (int64_t rp = 0; rp < n_rp && ok; ++rp) {
      uint8_t *pmv = pm.data() + (rp * c->n_bv + v) * 16;
      int used = 0;
      const int64_t i1 = std::min<int64_t>(c->M, (rp + 1) * BM);
      for (int64_t i = rp * BM; i < i1; ++i) {
        const int b = bor[i];
        if (b < 0) continue;             // row in no batch: identity slot 15
        if (b > 254) { ok = false; break; }
        int sl = slot_of[(size_t)b];
        if (sl < 0) {
          if (used == 15) { ok = false; break; }
          sl = used++;
          slot_of[(size_t)b] = sl;
          pmv[sl] = (uint8_t)b;
        }
        rs[(size_t)((int64_t)v * c->M + i)] = (uint8_t)sl;
      }
      for (int q = 0; q < used; ++q) slot_of[pmv[q]] = -1;
    }
  }
  ps.ok = ok;
  ps.BM = BM;
  ps.serial = c->views_serial;
  if (ok) {
    PMFCHK(upload_new(ps.pm, pm.data(), pm.size()));
    PMFCHK(upload_new(ps.row_slot, rs.data(), rs.size()));
  }
  return 0;
}

// The kernel families of the fused data pass: one row per (family, KB) -- the exact kernel's per (KB, row blocks per wave)
// -- with everything the host needs to run it.  fused_geometry picks the row; the buffers, the operand images, the launch
// and the diagnostics of the pass read it.
enum FusedImages { IMG_NONE, IMG_SB, IMG_SB4, IMG_SB8 };   // operand images: none, k_sb_split, k_sb4_split, k_sb8_split
struct FusedFamily {
  int kernel;          // pmf_debug_last_kernel: 0 exact, 1 sb, 2 sb2, 4 sb4, 8 sb8
  int KB, NW, RBW;     // K blocks; waves x 32-row blocks per wave
  int max_bv;          // batch views its LDS has room for
  FusedImages img;     // how its operand images are split (sb_split_x, sb_split_y)
  int img_kb;          // K blocks of an image row (pmf_fused_sb4_kernel's images have 256-byte rows whatever K)
  int xblk, yblk;      // image bytes per 32 rows of X / per 32 columns of sigma*Y
  int nblk;            // X images are split in whole panels of nblk row blocks (pmf_fused_sb8_kernel reads them unclamped)
  PmfFusedLaunch *launch[2];
  constexpr int BM() const { return 32 * NW * RBW; }   // row-panel height
};
static constexpr FusedFamily fused_families[] = {
    // kernel, KB, NW, RBW, max_bv, images, img_kb, xblk, yblk, nblk, launchers (D stored as f32, as bf16)
    {0, 1, 8,             2,             PMF_MAXV,          IMG_NONE, 0, 0,               0,               1,               {pmf_launch_fused<0, 1, 2, false>, pmf_launch_fused<0, 1, 2, true>}},
    {0, 1, 8,             1,             PMF_MAXV,          IMG_NONE, 0, 0,               0,               1,               {pmf_launch_fused<0, 1, 1, false>, pmf_launch_fused<0, 1, 1, true>}},
    {0, 2, 8,             1,             PMF_MAXV,          IMG_NONE, 0, 0,               0,               1,               {pmf_launch_fused<0, 2, 1, false>, pmf_launch_fused<0, 2, 1, true>}},
    {0, 3, 4,             1,             PMF_MAXV,          IMG_NONE, 0, 0,               0,               1,               {pmf_launch_fused<0, 3, 1, false>, pmf_launch_fused<0, 3, 1, true>}},
    {0, 4, 4,             1,             PMF_MAXV,          IMG_NONE, 0, 0,               0,               1,               {pmf_launch_fused<0, 4, 1, false>, pmf_launch_fused<0, 4, 1, true>}},
    {1, 1, SbCfg<1>::NW,  1,             SbCfg<1>::max_bv,  IMG_SB,   1, SbCfg<1>::BLK,   SbCfg<1>::BLK,   1,               {pmf_launch_fused<1, 1, 1, false>, pmf_launch_fused<1, 1, 1, true>}},
    {1, 2, SbCfg<2>::NW,  1,             SbCfg<2>::max_bv,  IMG_SB,   2, SbCfg<2>::BLK,   SbCfg<2>::BLK,   1,               {pmf_launch_fused<1, 2, 1, false>, pmf_launch_fused<1, 2, 1, true>}},
    {2, 2, 4,             2,             Sb2Cfg::max_bv,    IMG_SB,   2, SbCfg<2>::BLK,   SbCfg<2>::BLK,   1,               {pmf_launch_fused<2, 2, 2, false>, pmf_launch_fused<2, 2, 2, true>}},
    {4, 3, Sb4Cfg<3>::NW, 1,             Sb4Cfg<3>::max_bv, IMG_SB4,  4, Sb4Cfg<3>::XBLK, Sb4Cfg<3>::YBLK, 1,               {pmf_launch_fused<4, 3, 1, false>, pmf_launch_fused<4, 3, 1, true>}},
    {4, 4, Sb4Cfg<4>::NW, 1,             Sb4Cfg<4>::max_bv, IMG_SB4,  4, Sb4Cfg<4>::XBLK, Sb4Cfg<4>::YBLK, 1,               {pmf_launch_fused<4, 4, 1, false>, pmf_launch_fused<4, 4, 1, true>}},
    {8, 2, Sb8Cfg<2>::NW, Sb8Cfg<2>::RB, Sb8Cfg<2>::max_bv, IMG_SB8,  2, Sb8Cfg<2>::XBLK, Sb8Cfg<2>::YBLK, Sb8Cfg<2>::NBLK, {pmf_launch_fused<8, 2, Sb8Cfg<2>::RB, false>, pmf_launch_fused<8, 2, Sb8Cfg<2>::RB, true>}},
    {8, 4, Sb8Cfg<4>::NW, Sb8Cfg<4>::RB, Sb8Cfg<4>::max_bv, IMG_SB8,  4, Sb8Cfg<4>::XBLK, Sb8Cfg<4>::YBLK, Sb8Cfg<4>::NBLK, {pmf_launch_fused<8, 4, Sb8Cfg<4>::RB, false>, pmf_launch_fused<8, 4, Sb8Cfg<4>::RB, true>}},
};
constexpr int PMF_XSB_PAD = 16;   // xsb's image blocks beyond nRB: sb_split_x writes the last panel of every family whole
static_assert([] { for (const FusedFamily &f : fused_families) if (f.nblk - 1 > PMF_XSB_PAD) return false; return true; }(), "PMF_XSB_PAD");

// kernel code, KB and (RBW > 0) row blocks per wave -> the family's row
static const FusedFamily *find_family(int kernel, int KB, int RBW = 0) {
  for (const FusedFamily &f : fused_families)
    if (f.kernel == kernel && f.KB == KB && (RBW == 0 || f.RBW == RBW)) return &f;
  return nullptr;
}

// Every PMF_* environment switch of the data pass, read here and nowhere else, once per fused_geometry, i.e. at every pass
// (a fit reads them once, for all its epochs); each with the meaning, default and clamping DESIGN.md section 10 lists.
static PassSwitches read_pass_switches(const pmf_ctx *c) {
  PassSwitches sw;
  auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
  auto at_least = [](const char *name, int lo) { const char *e = getenv(name); return e ? std::max(lo, atoi(e)) : -1; };
  // PMF_SB2 alone is read once per process: its first value holds for every later pass, whatever the variable is set to then
  static const bool sb2 = num("PMF_SB2", 1) != 0;
  sw.sb2 = sb2; sw.sb8 = num("PMF_SB8", 1); sw.rbw1 = num("PMF_RBW", 0) == 1;
  sw.dbg_set = getenv("PMF_DEBUG_FLAGS") != nullptr; sw.dbg = num("PMF_DEBUG_FLAGS", 0);
  sw.xgemm3 = num("PMF_XGEMM3", 1) != 0; sw.xreg = num("PMF_XREG", 1) != 0; sw.plain = num("PMF_PLAIN", 1) != 0;
  sw.reserve_cus = std::min(at_least("PMF_RESERVE_CUS", 0), c->n_cu / 2);
  if (const char *e = getenv("PMF_TPS_SCALE")) sw.tps_scale = atof(e);
  if (const char *e = getenv("PMF_COMM_ALGBW_GBPS")) if (atof(e) > 0) sw.algbw_gbps = atof(e);
  sw.w_bern = at_least("PMF_W_BERN", 16); sw.w_pois = at_least("PMF_W_POIS", 16); sw.w_hinge = at_least("PMF_W_HINGE", 16);
  sw.w_batch = at_least("PMF_W_BATCH", 0);
  return sw;
}

// Family and chunking of a fused data pass.
//   family (a row of fused_families): split-bf16 products (pmf_set_precision), at least one gradient, no PMF_DEBUG_FLAGS:
//     K <= 32 sb;  32 < K <= 64 sb8 with both gradients unless PMF_SB8=0 or 4, else sb2 (sb under PMF_SB2=0);
//     64 < K <= 96 sb4;  96 < K <= 128 sb8 with both gradients unless PMF_SB8=0, else sb4.
//   With batch layers a family also needs the dense batch table, LDS room for the views and at most 15 batches of a view per
//   row panel of ITS height (panel-local slots): sb8 falls back to sb2 / sb / sb4, these to the exact kernel, which has the
//   per-entry gathers besides (bmode 2).  Everything else runs the exact kernel, with two row blocks per wave at K <= 32
//   without batch layers (per-tile overheads amortised over twice the MFMA work; PMF_RBW=1: one; the batch-layer epilogue
//   of two row blocks does not fit the 256-register budget: it spills and is 1.5x slower).
//   chunks: the column tiles are walked in S contiguous chunks, one launch each.  S = 1 unless the context has a
//   communicator with more than one rank (then the all-reduce of chunk s's grad(Y) runs beside the launches of the later
//   chunks and of the next epoch's earlier ones, pmf_fit) or pmf_comm_set_chunks asked for it.
FusedGeom fused_geometry(pmf_ctx *c, bool want_gx, bool want_gy, bool allow_chunks) {
  FusedGeom g;
  g.want_gx = want_gx; g.want_gy = want_gy;
  g.sw = read_pass_switches(c);
  const PassSwitches &sw = g.sw;
  int bmode = 0;
  auto batch_fits = [&](const FusedFamily *f) {
    if (c->n_bv == 0) return true;
    PanelSlots *ps = nullptr;
    if (!c->btd_ok || c->n_bv > f->max_bv || ensure_panel_slots(c, f->BM(), &ps) != 0 || !ps || !ps->ok) return false;
    g.ps = ps;
    return true;
  };
  if (c->precision == PMF_PREC_BF16X3 && (want_gx || want_gy) && !sw.dbg_set) {
    const bool both = want_gx && want_gy;
    int base = 0;       // the family without sb8
    bool sb8 = false;
    switch (c->KB) {
      case 1: base = 1; break;
      case 2: base = sw.sb2 ? 2 : 1; sb8 = both && sw.sb8 != 0 && sw.sb8 != 4; break;
      case 3: base = 4; break;
      case 4: base = 4; sb8 = both && sw.sb8 != 0; break;
    }
    const FusedFamily *f8 = sb8 ? find_family(8, c->KB) : nullptr, *fb = find_family(base, c->KB);
    g.fam = f8 && batch_fits(f8) ? f8 : (fb && batch_fits(fb) ? fb : nullptr);
    bmode = g.fam && c->n_bv > 0 ? 1 : 0;
  }
  if (!g.fam) {
    g.fam = find_family(0, c->KB, c->KB == 1 && c->n_bv == 0 && !sw.rbw1 ? 2 : 1);
    if (!g.fam) return g;   // (prepare_fused_pass fails)
    if (c->n_bv > 0) bmode = batch_fits(g.fam) ? 1 : 2;
  }
  // the instance of the family's kernel: the split families' per gradient pair (gm 0 .. 2), the exact kernel's by the rules of
  // pmf_common.h; PMF_XGEMM3=0 / PMF_XREG=0 keep the instance without (bit-identical results: the A/B inside one library)
  const FusedFamily &f = *g.fam;
  const bool db = c->store == PMF_STORE_BF16;
  FusedInstance &in = g.inst;
  in.bmode = bmode; in.mixed = c->mixed;
  in.gm = pmf_exact_gm(f.kernel == 0 ? bmode : 0, want_gx, want_gy, sw.dbg);
  in.xw = f.kernel == 0 && sw.xgemm3 && pmf_exact_has_xw(f.KB, f.NW, f.RBW, in.bmode, in.mixed, in.gm, db);
  in.xr = in.xw && sw.xreg && pmf_exact_has_xr(f.KB, f.NW, f.RBW, in.bmode, in.mixed, in.gm, db);
  g.n_rp = (c->M + f.BM() - 1) / f.BM();
  g.n_ct_all = (c->N + PMF_BN - 1) / PMF_BN;
  int reserve = c->comm.nranks > 1 ? c->comm.reserve_cus : 0;
  if (sw.reserve_cus >= 0) reserve = sw.reserve_cus;   // (tests / A-B: a one-rank run with the multi-rank grid)
  g.grid_max = std::max(1, c->n_cu - reserve);
  int S = 1;
  if (allow_chunks && want_gy) {
    S = c->n_chunks_req > 0 ? c->n_chunks_req : 1;
    if (c->n_chunks_req <= 0 && c->comm.nranks > 1) {
      // Automatic.  In the pipelined loop of pmf_fit the all-reduce of chunk s has until the Y step of chunk s, i.e. it
      // runs beside the data pass of the other S - 1 chunks (this epoch's s+1.. and the next epoch's ..s-1): with one
      // chunk the collective is fully exposed, with two or more it is hidden as long as it is shorter than (S-1)/S of a
      // pass.  Every extra launch costs ~0.06 ms of prologue, tail and launch gap (measured with a one-rank communicator,
      // 25000 rows x 50000, K = 64: 1 / 2 / 4 / 8 chunks = 4.27 / 4.33 / 4.45 / 4.79 ms per epoch), so: two chunks, more
      // only while a chunk's all-reduce (~30 us + bytes / algorithm bandwidth; 60 GB/s assumed for an 8-GPU xGMI ring
      // at these sizes, PMF_COMM_ALGBW_GBPS overrides) would not fit beside the rest of the pass.
      const double algbw = sw.algbw_gbps * 1e9;
      // Rank-invariant inputs only (every rank must choose the same S: it is the number and size of the collectives):
      // N, Kp, the arithmetic mode and the MEAN rows per rank that pmf_fit has all-reduced (comm.m_mean), never the local
      // row count or the kernel variant this rank's batch layout happens to allow.
      const int64_t Mref = c->comm.m_mean > 0 ? c->comm.m_mean : c->M;
      const double bytes = 4.0 * (double)c->Kp * (double)c->N;
      const double t_pass = 6.0 * (double)Mref * (double)c->N * (double)c->Kp / (c->precision == PMF_PREC_BF16X3 ? 200e12 : 115e12);
      S = 2;
      while (S < 4 && 30e-6 + bytes / S / algbw > t_pass * (S - 1) / S) ++S;
      // a chunk should give every workgroup a few dozen tiles at least (each launch pays its prologue and its tail).  Counted
      // in REFERENCE panels of 256 rows, the unit the threshold was calibrated in -- not the family's BM: the panel height belongs
      // to the kernel family THIS rank runs (512 rows for pmf_fused_sb8_kernel at K <= 64, 256 where a rank's batch layout sends
      // it to pmf_fused_sb2_kernel), and two ranks that disagreed on it chose different S, i.e. different collectives.
      constexpr int64_t REF_PANEL = 256;
      const int64_t n_rp_ref = (Mref + REF_PANEL - 1) / REF_PANEL;
      const int64_t min_tiles = 32ll * std::max(1, c->n_cu - c->comm.reserve_cus);
      while (S > 1 && (n_rp_ref * g.n_ct_all) / S < min_tiles) --S;
    }
    S = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(S, PMF_MAX_CHUNKS), g.n_ct_all));
  }
  g.S = S;
  for (int s = 0; s < S; ++s) {
    g.ct0[s] = g.n_ct_all * s / S;
    g.nct[s] = g.n_ct_all * (s + 1) / S - g.ct0[s];
  }
  return g;
}

// Column segmentation of one chunk.  The work split is balanced to a tile whatever the segmentation, so the segment
// length only trades
//   (a) the fixed cost of a piece (X panel, first Y / D tile, gX flush: ~8 us) -- a workgroup walks
//       (T/G)/tps + 2 pieces -- against
//   (b) k_gy_reduce, which reads the private slabs of the ~G*tps/n_ct + 1 workgroups that visited a column tile
//       (Kp*N*4 bytes each at ~4 TB/s).
// tps* = sqrt(a/b) minimises a/tps + b*tps.
static void chunk_segments(pmf_ctx *c, const FusedGeom &g, int s, int &grid, int64_t &tps, int64_t &n_cseg) {
  const int64_t n_ct = g.nct[s], n_rp = g.n_rp;
  grid = (int)std::min<int64_t>(n_rp * n_ct, (int64_t)g.grid_max);
  const double tiles_per_wg = (double)(n_rp * n_ct) / grid;
  const double a_cost = tiles_per_wg * 8e-6;
  const double b_cost = (double)grid * (double)c->Kp * (double)n_ct * 32.0 * 4.0 / ((double)n_ct * 4e12);
  tps = (int64_t)std::llround(std::sqrt(a_cost / std::max(b_cost, 1e-12)));
  tps = (int64_t)std::llround((double)tps * g.sw.tps_scale);   // (PMF_TPS_SCALE, development: scale the model's segment length; 1 unless set)
  tps = std::max<int64_t>(std::min<int64_t>(8, n_ct), std::min<int64_t>(tps, n_ct));
  // equal segments; the LAST one takes the remainder (it is longer, never tiny: every piece of work pays the fixed
  // prologue, so a 5-tile last segment once made one workgroup 20 % late)
  n_cseg = std::max<int64_t>(1, n_ct / tps);
}

// Everything a data pass needs before its first launch: work splits of all chunks (cached), the gX slot map, buffers.
int prepare_fused_pass(pmf_ctx *c, const FusedGeom &g) {
  if (!g.fam) return pmf_fail("unsupported KB=%d", c->KB);
  const FusedFamily &f = *g.fam;
  const bool want_gx = g.want_gx, want_gy = g.want_gy;
  if ((int)c->splits.size() < g.S) c->splits.resize((size_t)g.S);
  int64_t grid_sum = 0, serial_sum = 0;
  for (int s = 0; s < g.S; ++s) {
    int grid; int64_t tps, n_cseg;
    chunk_segments(c, g, s, grid, tps, n_cseg);
    PMFCHK(compute_work_split(c, g.sw, c->splits[(size_t)s], grid, g.n_rp, g.ct0[s], g.nct[s], tps, n_cseg, f.kernel != 0));
    grid_sum += grid;
  }
  serial_sum = c->split_serial * PMF_MAX_CHUNKS + g.S;   // (split_serial is bumped by every recomputed split)
  PMFCHK(ensure_loss_partials(c, grid_sum));   // one per workgroup and chunk
  const int64_t slab_stride = (int64_t)c->Kp * c->N;
  // never read before written, EXCEPT by pmf_fused_sb8_kernel, which loads the old values of a ragged last tile's absent
  // columns without clamping (they are accumulated and never stored): one tile of padding at THIS Kp keeps those loads in
  // bounds (the capacity counts the padding: a buffer allocated at a smaller Kp has less of it)
  const size_t gy_need = (size_t)g.grid_max * (size_t)slab_stride + (size_t)PMF_BN * (size_t)c->Kp;
  if (want_gy) PMFCHK(c->gy_slabs.ensure(gy_need, false));
  if (want_gx && serial_sum != c->gx_serial) {
    // slot map of the gX partial slabs: chunk s owns slots [slot_base, slot_base + pieces); per row panel, its slots in
    // work-sequence order (chunk, then segment, then position inside the unit) -- the order k_gx_reduce sums them in
    std::vector<std::vector<int32_t>> lists((size_t)g.n_rp);
    int32_t base = 0;
    for (int s = 0; s < g.S; ++s) {
      WorkSplit &ws = c->splits[(size_t)s];
      ws.slot_base = base;
      for (size_t p = 0; p < ws.piece_rp.size(); ++p) lists[(size_t)ws.piece_rp[p]].push_back(base + (int32_t)p);
      std::vector<int32_t> abs(ws.h_piece_base);
      for (auto &v : abs) v += base;
      PMFCHK(ws.d_piece_base_abs.upload(abs.data(), abs.size()));
      base += (int32_t)ws.piece_rp.size();
    }
    std::vector<int32_t> off((size_t)g.n_rp + 1, 0), idx;
    for (int64_t rp = 0; rp < g.n_rp; ++rp) {
      idx.insert(idx.end(), lists[(size_t)rp].begin(), lists[(size_t)rp].end());
      off[(size_t)rp + 1] = (int32_t)idx.size();
    }
    if (idx.empty()) idx.push_back(0);
    PMFCHK(upload_new(c->gx_off, off.data(), off.size()));
    PMFCHK(upload_new(c->gx_idx, idx.data(), idx.size()));
    c->gx_serial = serial_sum;
  }
  if (want_gx) {
    // sized on EVERY pass, not with the slot map: a slot holds BM x Kp floats of the family that runs, and neither the family
    // nor its panel height is in the work split's key (70 rows are one panel of 256 and of 512 rows alike: an exact f32 pass
    // followed by an sb8 pass reuses the split and the slot map, and needs twice the bytes)
    size_t pieces = 0;
    for (int s = 0; s < g.S; ++s) pieces += c->splits[(size_t)s].piece_rp.size();
    PMFCHK(c->gx_part.ensure(pieces * (size_t)f.BM() * (size_t)c->Kp, false));   // every slot is written whole by its piece before it is read
  }
  PMFCHK(ensure_tile_flags(c));
  if (g.has_plain_loop()) {
    PMFCHK(ensure_plain_table(c, f.BM(), g.n_ct_all));
    PMFCHK(c->plain_count.ensure((size_t)grid_sum, false));   // one per workgroup and chunk, like the loss partials
  }
  if (f.img != IMG_NONE) {
    // the image buffers are sized for the largest block of every family whose image rows are as wide as f's
    size_t xblk = 0, yblk = 0;
    for (const FusedFamily &o : fused_families)
      if (o.img_kb == f.img_kb) { xblk = std::max<size_t>(xblk, o.xblk); yblk = std::max<size_t>(yblk, o.yblk); }
    // X images + PMF_XSB_PAD row blocks: sb_split_x writes whole panels, roundup(nRB, nblk) blocks.  The capacity counts
    // the padding at THIS xblk (a buffer allocated for narrower images may hold fewer bytes of it).
    const size_t xb = ((size_t)c->nRB + PMF_XSB_PAD) * xblk, yb = (size_t)g.n_ct_all * yblk;
    PMFCHK(c->xsb.ensure(xb, true));    // (the padding blocks are zeroed here, once)
    PMFCHK(c->ysb.ensure(yb, false));
    if (f.img == IMG_SB8) {
      PMFCHK(c->sb8_scale.ensure((size_t)(1 + PMF_MAX_CHUNKS), false));
      PMFCHK(c->sb8_max.ensure((size_t)(1 + PMF_MAX_CHUNKS), true));
    }
  }
  return 0;
}

// ---- extents: what a prepared pass addresses against what is allocated ("Extents")
// Every need is taken from the index expressions of the kernels the pass launches (the fused kernel of g.fam, its operand
// splits, k_gy_reduce, k_gx_reduce, k_loss_reduce) with the values launch_fused_chunk hands them, not from the sizing
// formulas of prepare_fused_pass.  Bytes.
int fused_pass_extents(pmf_ctx *c, const FusedGeom &g, PassExtent *out) {
  const FusedFamily &f = *g.fam;
  const bool want_gx = g.want_gx, want_gy = g.want_gy;
  const int64_t Kp = c->Kp, Npad = g.n_ct_all * PMF_BN;
  int64_t pieces = 0, grid_sum = 0, grid_top = 0;
  for (int s = 0; s < g.S; ++s) {
    const WorkSplit &ws = c->splits[(size_t)s];
    pieces += (int64_t)ws.piece_rp.size();
    grid_sum += ws.grid;
    grid_top = std::max<int64_t>(grid_top, ws.grid);
  }
  const bool bt = g.inst.bmode == 1;
  int nbs_shift = 0;
  while ((1 << nbs_shift) < c->nbs) ++nbs_shift;
  const int64_t gx_slot_stride = (int64_t)f.BM() * Kp, slab_stride = Kp * c->N;
  int n = 0;
  // every piece stores its whole BM x Kp partial at slot * gx_slot_stride; the slots of all chunks are numbered through
  out[n++] = {"gx_part", want_gx ? pieces * gx_slot_stride * 4 : 0, (int64_t)c->gx_part.bytes()};
  // workgroup wg < grid works in gy_slabs + wg * slab_stride: the live columns of its tiles, sb8 the whole last tile
  out[n++] = {"gy_slabs", want_gy ? ((grid_top - 1) * slab_stride + (f.img == IMG_SB8 ? Npad * Kp : slab_stride)) * 4 : 0,
              (int64_t)c->gy_slabs.bytes()};
  // row blocks < nRB (clamped); sb8 and its split whole panels of nblk blocks
  out[n++] = {"xsb", f.img != IMG_NONE ? (c->nRB + f.nblk - 1) / f.nblk * f.nblk * f.xblk : 0, (int64_t)c->xsb.bytes()};
  out[n++] = {"ysb", f.img != IMG_NONE ? g.n_ct_all * f.yblk : 0, (int64_t)c->ysb.bytes()};
  // all 32 columns of every tile, the last slot of a column the identity
  out[n++] = {"btd", bt ? (Npad << nbs_shift) * (int64_t)sizeof(float2) : 0, (int64_t)c->btd.bytes()};
  out[n++] = {"colview", bt ? Npad : 0, (int64_t)c->colview.bytes()};
  out[n++] = {"tflags", g.n_ct_all * c->nRB * 4, (int64_t)c->tflags.bytes()};
  out[n++] = {"loss_partial", grid_sum * 8, (int64_t)c->loss_partial.bytes()};
  out[n++] = {"pm", bt ? g.n_rp * c->n_bv * 16 : 0, bt ? (int64_t)g.ps->pm.bytes() : 0};
  out[n++] = {"row_slot", bt ? (int64_t)c->n_bv * c->M : 0, bt ? (int64_t)g.ps->row_slot.bytes() : 0};
  if (g.has_plain_loop()) {
    // rows of a pass whose kernel has the plain loop only: row panel rp < n_rp reads entries [0, n_ct_all] of its line (the
    // absolute column tile of a run's end is at most n_ct_all); one count per workgroup and chunk
    out[n++] = {"ptab", g.n_rp * (g.n_ct_all + 1) * 4, c->ptab_bm == f.BM() ? (int64_t)c->ptab.bytes() : 0};
    out[n++] = {"plain_count", grid_sum * 4, (int64_t)c->plain_count.bytes()};
  }
  static_assert(PMF_PASS_EXTENTS == 12, "fused_pass_extents");
  return n;
}
int check_pass_extents(const PassExtent *e, int n) {
  for (int i = 0; i < n; ++i)
    if (e[i].need > e[i].cap)
      return pmf_fail("data pass refused: it addresses %lld bytes of %s, %lld are allocated", (long long)e[i].need, e[i].name,
                      (long long)e[i].cap);
  return 0;
}
int guard_fused_pass(pmf_ctx *c, const FusedGeom &g) {
  PassExtent e[PMF_PASS_EXTENTS];
  return check_pass_extents(e, fused_pass_extents(c, g, e));
}

// split-bf16 operand images (k_sb_split): X once per pass, sigma*Y per chunk (its columns only: the Y step of a later
// chunk of the previous epoch may not have run yet when an earlier chunk is launched, pmf_fit)
// pmf_fused_sb8_kernel's images: the power-of-two pre-scale of the f16 pair first (a device scalar: no host round trip)
static int sb8_split(pmf_ctx *c, const FusedFamily &f, const float *src, const float4 *colp, int64_t n, int64_t nblk, int slot,
                     int transposed, char *out) {
  Sb8ScaleArgs sa = {src, colp, n, c->Kp, c->sb8_max + slot, c->sb8_scale + slot};
  PMFCHK(pmf_launch_sb8_scale(c->stream, sa));
  Sb8SplitArgs sp = {src, colp, c->sb8_scale + slot, n, nblk, transposed, out};
  return pmf_launch_sb8_split(c->stream, sp, f.KB);
}
static int sb_split_x(pmf_ctx *c, const FusedFamily &f) {
  if (f.img == IMG_SB8) {
    // whole panels: k_sb8_split writes zero images for the absent row blocks of a ragged last panel, which the kernel reads
    // unclamped (GEMM3's transposed X fragments; G is zero there, but 0 x a stale NaN is not).  Within the allocation:
    // roundup(nRB, nblk) <= nRB + PMF_XSB_PAD blocks (prepare_fused_pass)
    return sb8_split(c, f, c->P[0].p, nullptr, c->M, (c->nRB + f.nblk - 1) / f.nblk * f.nblk, 0, 1, c->xsb);
  }
  if (f.img == IMG_SB4) {
    Sb4SplitArgs s4 = {c->P[0].p, nullptr, c->M, c->nRB, c->Kp, 1, c->xsb};
    return pmf_launch_sb4_split(c->stream, s4);
  }
  SbSplitArgs sx = {c->P[0].p, nullptr, c->M, c->nRB, c->xsb};
  return f.KB == 1 ? pmf_launch_sb_split<1>(c->stream, sx) : pmf_launch_sb_split<2>(c->stream, sx);
}
static int sb_split_y(pmf_ctx *c, const FusedFamily &f, int64_t ct0, int64_t nct, int chunk) {
  const int64_t c0 = ct0 * 32;
  const float *src = c->P[1].p + c0 * c->Kp;
  char *out = c->ysb + (size_t)ct0 * (size_t)f.yblk;
  if (f.img == IMG_SB8) return sb8_split(c, f, src, c->colp + c0, std::min<int64_t>(c->N - c0, nct * 32), nct, 1 + chunk, 0, out);
  if (f.img == IMG_SB4) {
    Sb4SplitArgs s4 = {src, c->colp + c0, c->N - c0, nct, c->Kp, 0, out};
    return pmf_launch_sb4_split(c->stream, s4);
  }
  SbSplitArgs sy = {src, c->colp + c0, c->N - c0, nct, out};
  return f.KB == 1 ? pmf_launch_sb_split<1>(c->stream, sy) : pmf_launch_sb_split<2>(c->stream, sy);
}

// One chunk of the data pass: the fused kernel over column tiles [ct0, ct0 + nct) and the fixed-order reduction of its
// private gY slabs; after the LAST chunk, the fixed-order reduction of the gX partial slabs.
int launch_fused_chunk(pmf_ctx *c, const FusedGeom &g, int s) {
  const FusedFamily &f = *g.fam;
  const bool want_gx = g.want_gx, want_gy = g.want_gy;
  WorkSplit &ws = c->splits[(size_t)s];
  const int grid = ws.grid;
  const int64_t n_ct = g.nct[s], n_rp = g.n_rp;
  const int64_t slab_stride = (int64_t)c->Kp * c->N;
  int64_t loss_off = 0;
  for (int q = 0; q < s; ++q) loss_off += c->splits[(size_t)q].grid;
  FusedArgs a;
  memset(&a, 0, sizeof(a));
  a.tflags = c->tflags;
  a.wg_begin = ws.wg_begin;
  a.D = c->D; a.X = c->P[0].p; a.Y = c->P[1].p; a.gX = c->P[0].g; a.gY = c->P[1].g;
  a.colp = c->colp; a.htab = c->htab; a.bor = c->bor; a.btab = c->btab; a.loss_partial = c->loss_partial + loss_off;
  a.btd = g.inst.bmode == 1 ? c->btd : nullptr; a.n_bv = c->n_bv;
  if (g.inst.bmode == 1) {
    a.pm = g.ps->pm; a.row_slot = g.ps->row_slot; a.colview = c->colview;
    a.nbs_shift = 0;
    while ((1 << a.nbs_shift) < c->nbs) ++a.nbs_shift;
  }
  c->last_bmode = g.inst.bmode;
  a.nRB = c->nRB; a.gy_slabs = c->gy_slabs; a.slab_stride = slab_stride; a.n_rp = n_rp;
  a.M = c->M; a.N = c->N; a.n_tiles = n_rp * n_ct; a.tps = (int)ws.tps; a.n_ct = (int)n_ct; a.n_cseg = (int)ws.n_cseg;
  a.want_gx = want_gx; a.want_gy = want_gy;
  a.ct0 = (int32_t)g.ct0[s];
  if (g.has_plain_loop()) {
    // PMF_PLAIN=0: every run takes the general tile loop; bit-identical results
    a.ptab = c->ptab; a.ptab_stride = (int32_t)(g.n_ct_all + 1); a.plain = g.sw.plain;
    a.plain_count = c->plain_count + loss_off;
  }
  a.gx_part = c->gx_part; a.piece_base = ws.d_piece_base_abs; a.gx_slot_stride = (int64_t)f.BM() * c->Kp;
  a.dbg = g.sw.dbg;
#ifdef PMF_STAMPS
  {
    static DevBuf<unsigned long long> d_stamps;
    PMFCHK(d_stamps.ensure((size_t)16 * 8 * 1024, false));
    HIPCHK(hipMemsetAsync(d_stamps, 0, sizeof(unsigned long long) * 16 * 8 * 1024, c->stream));
    a.stamps = d_stamps;
    g_stamps = d_stamps;
  }
#endif
  a.views = c->d_views;
  if (f.img != IMG_NONE) {
    if (s == 0) PMFCHK(sb_split_x(c, f));
    PMFCHK(sb_split_y(c, f, g.ct0[s], n_ct, s));
    a.Xsb = c->xsb; a.Ysb = c->ysb;
    if (f.img == IMG_SB8) { a.sb_scale_x = c->sb8_scale; a.sb_scale_y = c->sb8_scale + 1 + s; }
  }
  // timing events
  if (c->ev_used == c->ev_pool.size()) {
    if (c->ev_pool.size() >= 4096) {
      HIPCHK(hipStreamSynchronize(c->stream));
      harvest_events(c);
    } else {
      hipEvent_t e0, e1;
      HIPCHK(hipEventCreate(&e0));
      HIPCHK(hipEventCreate(&e1));
      c->ev_pool.emplace_back(e0, e1);
    }
  }
  auto &ev = c->ev_pool[c->ev_used++];
  HIPCHK(hipEventRecord(ev.first, c->stream));
  c->last_kernel = f.kernel;
  const int rc = f.launch[c->store == PMF_STORE_BF16](&c->dyn_lds, c->stream, a, grid, g.inst);
  c->last_xreg = g.inst.xr;
  // the counts the pass leaves in plain_count: those of its chunks so far, if its instance writes them
  c->last_plain_n = g.has_plain_loop() ? loss_off + grid : -1;
  if (f.kernel != 0) c->sb_launches += 1;
  PMFCHK(rc);
  HIPCHK(hipEventRecord(ev.second, c->stream));   // the events bracket pmf_fused_kernel alone (= rocprofv3's kernel duration)
  if (want_gy && !(a.dbg & 8)) {
    k_gy_reduce<<<dim3((unsigned)n_ct, (unsigned)(32 * c->Kp / 256)), 64, 0, c->stream>>>(c->gy_slabs, slab_stride, ws.c_off, ws.c_idx,
                                                                                      c->Kp, c->N, c->P[1].g, (int)g.ct0[s],
                                                                                      f.img == IMG_SB8 ? c->colp : nullptr);
    HIPCHK(hipGetLastError());
  }
  if (want_gx && s == g.S - 1) {
    const int64_t panel = (int64_t)f.BM() * c->Kp;
    k_gx_reduce<<<dim3((unsigned)g.n_rp, (unsigned)((panel / 4 + 255) / 256)), 256, 0, c->stream>>>(
        c->gx_part, panel, c->gx_off, c->gx_idx, panel, (int64_t)c->Kp * c->M, c->P[0].g);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// the whole data pass in one go (step-level API, single-chunk callers)
int launch_fused(pmf_ctx *c, bool want_gx, bool want_gy) {
  const FusedGeom g = fused_geometry(c, want_gx, want_gy, /*allow_chunks=*/c->n_chunks_req > 0);   // (chunks only on request)
  PMFCHK(prepare_fused_pass(c, g));
  PMFCHK(guard_fused_pass(c, g));
  for (int s = 0; s < g.S; ++s) PMFCHK(launch_fused_chunk(c, g, s));
  return 0;
}

// Which batch-layer variants the last launches took (tests and benchmarks: a silent fall-back to the slow paths is a
// performance bug).  bmode: 0 none, 1 LDS table with panel-local slots, 2 per-entry gathers; layer_path: 1 MFMA layer
// pass, 2 VALU layer kernel; slots: columns of the dense batch table; xreg: 1 = the last fused launch held its X
// fragments in registers (the only way to tell: its results are bit-identical to the LDS-read instance's).
extern "C" int pmf_debug_last_kernel(pmf_ctx *c, int *kernel) {
  if (!c) return pmf_fail("null context");
  if (kernel) *kernel = c->last_kernel;
  return 0;
}

extern "C" int pmf_debug_last_path(pmf_ctx *c, int *bmode, int *layer_path, int *slots, int *xreg, int64_t *plain_tiles) {
  if (!c) return pmf_fail("null context");
  if (plain_tiles) {
    *plain_tiles = 0;
    if (c->last_plain_n > 0) {
      PMFCHK(ctx_bind(c));
      std::vector<int32_t> h((size_t)c->last_plain_n);
      HIPCHK(hipMemcpyAsync(h.data(), c->plain_count, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int32_t v : h) *plain_tiles += v;
    }
  }
  if (xreg) *xreg = c->last_xreg;
  if (bmode) *bmode = c->last_bmode;
  if (layer_path) *layer_path = c->last_layer_path;
  if (slots) *slots = c->nbs;
  return 0;
}

// The plain-run table of the context's data for 256-row panels, built as a pass builds it (ensure_plain_table).
extern "C" int pmf_debug_plain_table(pmf_ctx *c, int32_t *out, int64_t cap, int64_t *n_rp, int64_t *n_ct) {
  PMFCHK(ctx_bind(c));
  if (!c->D) return pmf_fail("data not set");
  PMFCHK(ensure_tile_flags(c));
  const int64_t nct = (c->N + PMF_BN - 1) / PMF_BN;
  PMFCHK(ensure_plain_table(c, 256, nct));
  if (n_rp) *n_rp = c->ptab_n_rp;
  if (n_ct) *n_ct = nct;
  if (out) {
    const int64_t n = c->ptab_n_rp * (nct + 1);
    if (cap < n) return pmf_fail("pmf_debug_plain_table: room for %lld entries, %lld needed", (long long)cap, (long long)n);
    HIPCHK(hipMemcpyAsync(out, c->ptab, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

// The extents of the data pass pmf_epoch_begin would run with these gradient flags (fused_pass_extents), after the same
// geometry and preparation, without launching the pass.  cap_override (may be null; entries < 0 keep the recorded
// capacity) replaces capacities in the report and makes the call end with the guard's own comparison on them.
extern "C" int pmf_debug_pass_extents(pmf_ctx *c, int update_X, int update_Y, const int64_t *cap_override, int n_max,
                                      const char **names, int64_t *need, int64_t *capacity, int *n_out) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  if (!c->prepared) PMFCHK(prepare(c));
  const FusedGeom g = fused_geometry(c, update_X != 0, update_Y != 0, /*allow_chunks=*/c->n_chunks_req > 0);
  PMFCHK(prepare_fused_pass(c, g));
  PassExtent e[PMF_PASS_EXTENTS];
  const int n = fused_pass_extents(c, g, e);
  if (n_max < n) return pmf_fail("pmf_debug_pass_extents: room for %d entries, %d needed", n_max, n);
  for (int i = 0; i < n; ++i) {
    if (cap_override && cap_override[i] >= 0) e[i].cap = cap_override[i];
    if (names) names[i] = e[i].name;
    if (need) need[i] = e[i].need;
    if (capacity) capacity[i] = e[i].cap;
  }
  if (n_out) *n_out = n;
  return cap_override ? check_pass_extents(e, n) : 0;
}
