// pmf_fused.hip.inc -- the fused data-pass kernel (included by pmf_k_fused.hip).
//
// One launch per epoch computes, for the local rows of D, everything the reference does in ~10 full
// M x N round trips (SURVEY 3.2): A = X'Y (MatFac forward; layers.jl:283), the four column layers
// (layers.jl:20-22, 120-122, 64-66, 199-201), the masked noise-model loss and its gradient, the
// pull-back through the layers (layers.jl:34-48; batch_array.jl:192-209, 136-147) and both gradient
// GEMMs (Zygote adjoint of transpose(X)*Y), reading D exactly once and never writing an M x N temporary.
//
// Geometry (gfx950, wave64, v_mfma_f32_32x32x2_f32 = exact f32):
//   workgroup = NW waves, owns BM = 32*NW rows (one 32-row block per wave) and sweeps a column segment in
//   tiles of 32 columns.  The Y tile is staged in LDS pre-multiplied by the column scale,
//   Ys[k,j] = sigma_j * Y[k,j] (ColScale folded into the operand), so per tile a wave runs
//     forward : Z[j,i]   = mu_j + sum_k Ys[k,j] X[k,i]   K/2 MFMAs  (mu_j is the accumulator's initial value;
//                                                                     A = Ys, B = X panel, both from LDS)
//     epilogue: G[j,i]   = dloss/dZ (* delta for batch views), in the 16 accumulator registers
//                          (lane = row i, register = column j); sigma_j*G is also written, transposed, to a
//                          wave-private XOR-swizzled LDS tile
//     GEMM2   : gX[i,k] += sum_j G[j,i] Ys[k,j]           16*KB MFMAs (A = the accumulator itself, B = Ys)
//     GEMM3   : gY[j,k]  = sum_i sigma_j G[j,i] X[k,i]    16*KB MFMAs (A = the transposed tile, B = X panel in LDS)
//   gX lives in registers for the whole sweep of a work unit (row panel x column segment; flushed once per unit).
//   The per-wave gY partials of a tile are written to per-wave LDS slabs with plain stores; after barrier B1 all
//   waves sum the NW slabs (16-B LDS reads, interleaved with the next tile's forward MFMAs) and add the result to
//   the workgroup's PRIVATE copy of gY in HBM with a plain read-modify-write (the old values are prefetched half a
//   tile earlier); barrier B2 frees the slabs.  k_gy_reduce (pmf_pass.hip) then sums the private copies of the
//   workgroups that visited each column segment, in fixed order: no float atomics on the gY path and a bitwise
//   reproducible gY.  (Measured alternatives: LDS float atomics, ds_add_f32, 3.5x slower than the whole rest of
//   the kernel; global atomics per tile, 10.6 % of the wave time in issue stalls -- the CU retires one 256-B
//   atomic instruction per ~120 cycles.)
//   The X fragments live in a wave-private LDS panel rather than in VGPRs: with them in registers hipcc ran out
//   of VGPRs and serialised every LDS read behind s_waitcnt 0 (profiles/, DESIGN.md).  That was the slab path at 254
//   VGPRs; the cross-wave instances below that have the room hold them in registers (XR).
//   Both outputs have lane = factor index k, so every global access is a full 128-B row segment.
//   What bounds the kernel (profiles/r1_micro_mfma_valu.txt): v_mfma_f32_32x32x2_f32 runs at exactly the packed-f32
//   VALU rate and does NOT co-execute with VALU instructions -- every VALU instruction issued by either wave of a
//   SIMD costs ~3.5 cycles of matrix time (LDS reads are free, ds_write_b128 ~13, global_load_dwordx4 ~18).  The
//   design therefore minimises the NUMBER of VALU / LDS-store / VMEM instructions per tile, not their placement.
//
// XW (KB = 2, NW = 8, RBW = 1, both gradients) splits GEMM3 over the waves by OUTPUT block instead of by rows: the waves
// publish their G tiles (by tile parity, in the space of the slabs), and after the tile's single barrier wave w contracts
// one 16 k x 16 j block of gY over all 256 rows of the panel with v_mfma_f32_16x16x4_f32 (A = the X panels, B = the G
// tiles, both b32 LDS reads), scales it by sigma_j and adds it straight to the private gY slab in HBM.  No per-wave
// slabs, no 8-way reduction between the forward's MFMAs and no second barrier (DESIGN.md section 4.1).
//
// XR (on XW instances that stay within 256 VGPRs without scratch: pmf_k_fused.hip, pmf_xreg_instance) holds a piece's X
// operands in registers.  They do not change within a piece, yet the XW loop read them from LDS for every tile: 8
// ds_read_b128 for the forward's B operand and 32 ds_read2st64_b32 for GEMM3's A operand, 40 of its 105 LDS reads and
// 24 KiB of the ~64 KiB a wave reads per tile.  With XR each wave reads both fragments once, after the piece prologue's
// barrier (the panels are still staged through LDS: that is how a wave gets the other waves' rows), and every MFMA takes
// the same values in the same order from registers: loss, gX and gY are bit-identical, 96 more VGPRs (144 -> 239 in the
// headline instance), 65 LDS reads per tile and wave.  PMF_XREG=0 (read at every pass) selects the LDS-read instance;
// pmf_debug_last_path's xreg tells which one ran.
//
// The XR instances (PLAINB) have a second instantiation of the tile loop for plain runs -- consecutive tiles of a piece
// that are all-finite, full and already visited -- which no longer asks those three questions per tile (at the loop,
// "Plain runs"), and read GEMM2's Y operand off one pinned base (Y1BASE).  Bit-identical again; PMF_PLAIN=0 (read at
// every pass) runs everything in the general loop, pmf_debug_last_path's plain_tiles counts the tiles that ran plain.

// RBW = 32-row blocks per wave.  RBW = 2 amortises everything that is per (wave, tile) but not per row -- the slab
// write, the cross-wave reduction, the Y staging, the barriers -- over twice the MFMA work; it is used where that
// overhead weighs most (K <= 32: half the MFMAs per tile of K = 64).
template <int KB, int NW, int RBW = 1>
struct FusedCfg {
  static constexpr int Kp = 32 * KB;
  static constexpr int KpS = Kp + 4;                      // padded LDS row (16-B aligned, conflict-free b128 reads)
  static constexpr int SLAB = 32 * Kp;                    // floats per wave slab: [KB][32 j][32 k]
  static constexpr int YT = PMF_BN * KpS;                 // floats per Y tile buffer
  static constexpr int XP = 32 * KpS;                     // floats per X panel of one row block: [32 i][KpS]
  static constexpr int TT = (RBW - 1) * 1024;             // floats per wave of G^T tiles that do not alias the slab
  static constexpr int FIXED = NW * SLAB + NW * RBW * XP + NW * TT + 8 * PMF_BN + 4;   // (+4: the tile's noise-kind summary)
  static constexpr int LDS_BUDGET = 160 * 1024;
  static constexpr int NYB = (2 * YT + FIXED) * 4 + 8 * NW <= LDS_BUDGET ? 2 : 1;  // Y double buffered?
  static constexpr size_t lds_bytes = (sizeof(float) * (NYB * YT + FIXED) + sizeof(double) * NW + 15) / 16 * 16;
  // batch-layer variants add: the tile's dense batch table [32 columns][16] float2 + per row block [16 views][32 rows] batch ids
  static constexpr size_t lds_batch_extra = PMF_BN * 16 * sizeof(float2) + PMF_PM_BYTES + NW * RBW * 16 * 32;
};

// The 4-wave variants run one wave per SIMD with the whole 512-entry register file (launch_bounds(256, 1): hipcc keeps
// the gX / gY accumulators in AGPRs, no spills).  An early version of this kernel returned a wrong gX in that
// configuration (DESIGN.md "toolchain notes"); the parity tests k100_4wave / k128_4wave guard it.
// -DPMF_NW4_WAVES=2 restores the 256-register build (spills).
#ifndef PMF_NW4_WAVES
#define PMF_NW4_WAVES 1
#endif
// -DPMF_Y1BASE=0: GEMM2's Y operand through the compiler's own addressing in every instance (the A/B of Y1BASE below)
#ifndef PMF_Y1BASE
#define PMF_Y1BASE 1
#endif
template <bool B> struct PmfFlag { static constexpr bool value = B; };
// GM = which gradients the launch produces, as a compile-time constant: 0 both (fit!), 1 grad(X) only (transform: Y
// fixed), 2 grad(Y) only, 3 decided at run time by FusedArgs (ablation flags, loss-only evaluations).  With GM < 3 the
// steady-state loop is branch-free apart from the loop itself, which lets hipcc emit exact counted s_waitcnt vmcnt(N)
// instead of draining the queue at every join (the run-time variant measured 2x slower on grad(Y)-only epochs).
// BMODE: 0 = no batch layers, 1 = batch tables staged through LDS (<= 15 batches per view), 2 = global gathers
template <int KB, int NW, int RBW, int BMODE, bool MIXED, int GM, bool DB, bool XW = false, bool XR = false>
__global__ __launch_bounds__(64 * NW, (NW == 8 ? 2 : PMF_NW4_WAVES)) void pmf_fused_kernel(const FusedArgs a) {
  using Cfg = FusedCfg<KB, NW, RBW>;
  constexpr bool FULL = GM != 3;   // no run-time flags
  // (XW) The two instances that would otherwise need scratch (D stored as bf16, mixed noise models and batch layers: 1 and 7
  // spilled registers at the 256 of two waves per SIMD): they give up the launch-long pinned addressing -- HOIST below
  // and the GEMM3 read bases, which they recompute per tile (~30 VALU) -- for 16 registers.  Same addresses, same results.
  constexpr bool TIGHT = XW && DB && MIXED && BMODE != 0;
  constexpr bool BATCH = BMODE != 0;
  constexpr bool bt_lds = BMODE == 1;
  constexpr int Kp = Cfg::Kp;
  constexpr int KS = Kp / 2;    // forward k-steps
  constexpr int KpS = Cfg::KpS;
  constexpr int BM = 32 * NW * RBW;
  constexpr int BN = PMF_BN;
  constexpr int NT = 64 * NW;
  constexpr int SLAB = Cfg::SLAB;
  constexpr int NYB = Cfg::NYB;
  constexpr int YV = (BN * Kp / 4 + NT - 1) / NT;  // float4 per thread per Y tile
  constexpr int RV4 = (BN * Kp / 4 + NT - 1) / NT; // gY float4 per thread in the slab reduction
  constexpr int NBT = (BN * 16 + NT - 1) / NT;     // float2 of the dense batch table per thread and tile
  static_assert(!XW || (KB == 2 && NW == 8 && RBW == 1 && GM == 0 && NYB == 2 && RV4 == 1 && 2 * NW * 1024 <= NW * SLAB),
                "cross-wave GEMM3: 8 waves x one row block, Kp = 64, both gradients");
  static_assert(!XR || XW, "register-resident X fragments: the cross-wave GEMM3 instances only");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Ys = reinterpret_cast<float *>(smem);        // [NYB][BN*KpS]      sigma_j * Y[k,j]
  float *Xs = Ys + NYB * Cfg::YT;                     // [NW*RBW][32*KpS]   32 rows of X per row block (both MFMA layouts read it)
  float *Sl = Xs + NW * RBW * Cfg::XP;                // [NW][SLAB]         per-wave gY partials (and the first G^T tile)
  float *Tt = Sl + NW * SLAB;                         // [NW][RBW-1][1024]  the other G^T tiles
  float *Cmu = Tt + NW * Cfg::TT;                     // [2][BN] column parameters of the tile (by tile parity)
  float *Cw = Cmu + 2 * BN;
  float *Csg = Cw + 2 * BN;
  int *Cmt = reinterpret_cast<int *>(Csg + 2 * BN);
  int *Ck = Cmt + 2 * BN;                             // [2] noise kind of the whole tile: 0/1/2 uniform, 3 mixed
  double *red = reinterpret_cast<double *>(Ck + 4);
  // (BATCH, LDS table) the tile's dense batch table as two planes [16 slots][32 columns]: delta, and theta + mu_j (the column
  // shift folded in at staging).  A lane's slot is fixed for a tile whose columns share one view (nearly always: views are
  // column ranges), so four consecutive columns' entries are ONE 16-B read per plane at a constant offset.
  float *Btd = reinterpret_cast<float *>(smem + Cfg::lds_bytes), *Btt = Btd + BN * 16;
  unsigned char *Pm = reinterpret_cast<unsigned char *>(Btd + 2 * BN * 16);           // (BATCH) the piece's slot -> batch map [n_bv][16]
  unsigned char *Bw0 = Pm + PMF_PM_BYTES + (threadIdx.x >> 6) * RBW * 16 * 32;        // (BATCH) this wave: [RBW][16][32] slot of every row

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int l31 = lane & 31;
  const int h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  const bool want_gx = GM == 3 ? a.want_gx != 0 : GM != 2, want_gy = GM == 3 ? a.want_gy != 0 : GM != 1;
  const int dbg = FULL ? 0 : a.dbg;
  float *Sw = Sl + w * SLAB;            // this wave's slab
  float *Xw[RBW], *T[RBW];
#pragma unroll
  for (int rb = 0; rb < RBW; ++rb) {
    Xw[rb] = Xs + (w * RBW + rb) * Cfg::XP;
    // the first G^T tile aliases the LAST k-block of the slab (which is written last); the others have their own space
    T[rb] = rb == 0 ? Sw + (KB - 1) * 1024 : Tt + (w * (RBW - 1) + rb - 1) * 1024;
  }
  // (XW) The G tiles live in the slab space as [tile parity][wave][1024].  Wave w owns the block (16 k from 16 (w >> 1),
  // 16 j from 16 (w & 1)) of the tile's gY; lane (g = lane >> 4, c = lane & 15) supplies, at step s of row block p, row
  // i = 4 g + (s >> 1) + 16 (s & 1) of the block to both operands (A[k = c][i] from the X panel, B[i][j = c] from the G
  // tile: the two 16-lane groups of a 32-lane half then sit on opposite halves of the 32 banks in both reads) and ends
  // with k = xw_k .. xw_k + 3 of column xw_j in its four accumulator registers: one 16-B element of the slab.
  const int xw_j = 16 * (w & 1) + (lane & 15), xw_k = 16 * (w >> 1) + 4 * (lane >> 4);
  const int xw_e = xw_j * Kp + xw_k;                           // this lane's float4 of the [32 j][Kp] gY tile
  const int xw_x = 4 * (lane >> 4) * KpS + 16 * (w >> 1) + (lane & 15);
  int xw_g[4];
  // the four X read bases as LDS byte addresses the compiler cannot re-derive inside the tile loop (it would, one VALU
  // instruction per base and tile): every X read of GEMM3 is base + a compile-time offset
  typedef const __attribute__((address_space(3))) float *lds_cptr;
  unsigned xw_xa[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = 4 * (lane >> 4) + u;
    xw_g[u] = i * 32 + 4 * ((xw_j >> 2) ^ (i & 7)) + (xw_j & 3);
    xw_xa[u] = (unsigned)(uintptr_t)(lds_cptr)(Xs + xw_x + u * KpS);
    if (XW && !TIGHT && !XR) asm volatile("" : "+v"(xw_xa[u]));   // (XR reads the panels once per piece: nothing to pin)
  }

  // (HOIST: the KB = 2 instances) Tile-invariant addressing.  The lane-dependent part of the Y, column-parameter and
  // old-slab load addresses is the same for every full tile and differs only in the matrix's last, ragged column tile
  // (the clamps that keep dead columns' loads in bounds).  Both sets are byte offsets computed once per launch and
  // pinned in registers; a tile selects one by a wave-uniform condition and adds it to a scalar base, so that a load
  // costs one VALU instruction instead of the clamp, the shifts and a 64-bit add.
  // (Not where the eight registers would only add to an instance's spills: the run-time-flag builds, the per-wave-slab
  // builds with batch layers, which already exceed the 256-register budget, and the TIGHT cross-wave builds.)
  constexpr bool HOIST = KB == 2 && NW == 8 && RBW == 1 && GM != 3 && !TIGHT && (XW || GM != 0 || BMODE == 0);
  // (PLAINB) the instances with a second tile loop for plain runs (below, at the loop)
  constexpr bool PLAINB = XW && XR && HOIST && !MIXED && !BATCH;
  // (PLAINB pins set 0 only, for the registers of the second loop: its general loop meets the ragged tile once per row
  // panel and computes that tile's clamps where it loads, behind a scalar branch)
  constexpr int HOZ = PLAINB ? 1 : 2;
  unsigned ho_y[HOZ][YV], ho_s[HOZ][YV], ho_c[HOZ], ho_g[HOZ][RV4];
  if (HOIST) {
#pragma unroll
    for (int z = 0; z < HOZ; ++z) {
      const int ncol = z == 0 || N % BN == 0 ? BN : (int)(N % BN);   // z = 1: the live columns of the ragged tile
#pragma unroll
      for (int q = 0; q < YV; ++q) {
        int e4 = tid + NT * q;
        if (e4 > BN * Kp / 4 - 1) e4 = BN * Kp / 4 - 1;
        int jl = (e4 * 4) / Kp;
        if (jl >= ncol) { jl = ncol - 1; e4 = jl * (Kp / 4); }
        ho_y[z][q] = 16u * e4;
        ho_s[z][q] = 16u * jl;
        asm volatile("" : "+v"(ho_y[z][q]), "+v"(ho_s[z][q]));
      }
      ho_c[z] = 16u * (tid < ncol ? tid : ncol - 1);
      asm volatile("" : "+v"(ho_c[z]));
#pragma unroll
      for (int q = 0; q < RV4; ++q) {
        int e = xw_e;
        if (!XW) {
          const int f = tid + NT * q, ff = f < BN * Kp / 4 ? f : 0;   // (slab_map below)
          e = ((ff % (BN * 8)) / 8) * Kp + 32 * (ff / (BN * 8)) + 4 * (ff % 8);
        }
        ho_g[z][q] = 4u * (e < ncol * Kp ? e : e % Kp);
        asm volatile("" : "+v"(ho_g[z][q]));
      }
    }
  }
  // (PLAINB) The offset is made opaque again where it is used: its zero extension then stays next to the add, which lets
  // the load take the base from scalar registers and the offset from ONE vector register.  Hoisted out of the loops, every
  // offset was a 64-bit pair with a register of zeros, every load a 64-bit vector add, and launch-invariant bases (the
  // private slab) were pre-added into further pairs: the registers the second tile loop needs.
  // (Y1BASE) GEMM2's B operand, Ys[tile parity][rowmap(s, h)][l31 + 32 kb]: the lane's part of the LDS byte address, pinned
  // for the launch.  A tile adds its buffer once and reads all 32 values at compile-time offsets from that ONE register;
  // left to itself the compiler pairs the reads (ds_read2_b32) off eight bases that it recomputes for every tile.
  constexpr bool Y1BASE = PLAINB && PMF_Y1BASE != 0;
  unsigned g2_lane = (unsigned)(uintptr_t)(lds_cptr)(Ys + 4 * h * KpS + l31);
  if (Y1BASE) asm volatile("" : "+v"(g2_lane));
  auto ho_at = [](const void *base, unsigned &off) {
    if (PLAINB) asm volatile("" : "+v"(off));
    return reinterpret_cast<const char *>(base) + off;
  };
#ifdef PMF_STAMPS
  unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long st_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long st_t0 = st_prev, st_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  // Work = all (row panel, column tile) pairs, ordered segment-major, then row panel, then tile.  Workgroup g owns the
  // contiguous range [wg_begin[g], wg_begin[g+1]) of that sequence (equal estimated cost, see launch_fused) and walks
  // it in pieces, a piece being the part of one (segment, row panel) unit inside the range (only a workgroup's first
  // and last piece can be partial).  Consecutive pieces share the column segment, so the workgroup's PRIVATE gY slab
  // (plain read-modify-write in HBM, no atomics in the loop) accumulates over its row panels; k_gy_reduce sums the
  // slabs of the workgroups that touched each column tile, in fixed order (bitwise reproducible gY).
  // XCD-aware range index: workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8), each with its own L2.
  // Giving the workgroups of one XCD CONSECUTIVE ranges keeps them inside one or two column segments, whose Y tiles
  // (2 MB per segment at K = 64) then stay in that XCD's 4 MB L2 instead of being re-fetched per workgroup.
  const int wg = pmf_xcd_wg(blockIdx.x, gridDim.x);
  const int64_t w_begin = a.wg_begin[wg];
  const int64_t w_end = a.wg_begin[wg + 1];
  float *myslab = a.gy_slabs + (int64_t)wg * a.slab_stride;
  const int64_t seg_block = a.n_rp * a.tps;        // tiles of one full segment
  double lossacc = 0.0;
  int n_plain = 0;                                 // (PLAINB) tiles this workgroup runs in the plain loop (scalar)
  int seg_cur = -1, pidx = 0, t0_first = 0;        // slab bookkeeping: piece index within the current segment visit
  int gx_slot = (GM == 2) ? 0 : a.piece_base[wg];  // slot of this workgroup's next piece in the gX partial buffer
  for (int64_t widx = w_begin; widx < w_end;) {
    int cs = (int)(widx / seg_block);
    if (cs > a.n_cseg - 1) cs = a.n_cseg - 1;
    const int tps_cs = cs == a.n_cseg - 1 ? a.n_ct - (a.n_cseg - 1) * a.tps : a.tps;
    const int64_t rem = widx - (int64_t)cs * seg_block;
    const int64_t rp = rem / tps_cs;
    const int ti0 = (int)(rem - rp * tps_cs);       // first tile of this piece within its segment
    const int ntiles = (int)(tps_cs - ti0 < w_end - widx ? tps_cs - ti0 : w_end - widx);
    widx += ntiles;
    if (cs != seg_cur) { seg_cur = cs; pidx = 0; t0_first = ti0; } else { ++pidx; }
    // a column tile's slab entry is STORED on the workgroup's first visit and accumulated afterwards: the first
    // piece of a segment visit covers tiles >= ti0 only, so tiles < t0_first are first seen by the second piece
    bool slab_first = true;
    // (PLAINB) the piece's plain run [t_plain, t_pend), see the tile loop below.  The two table entries are loaded here and
    // compared there, behind the prologue's loads and barrier.
    int pl_b = ntiles, pl_e = ntiles;
    int32_t pl_c0 = 0, pl_c1 = 0;
    if (PLAINB && a.plain) {
      const int64_t c_abs = (int64_t)a.ct0 + (int64_t)cs * a.tps + ti0;   // absolute column tile of the piece's tile 0
      const bool rag = (c_abs + ntiles) * PMF_BN > N;                      // the piece ends with the matrix's ragged tile
      pl_b = pidx == 0 ? ntiles : (pidx == 1 ? (t0_first - ti0 < 0 ? 0 : (t0_first - ti0 < ntiles ? t0_first - ti0 : ntiles)) : 0);
      pl_e = rag ? ntiles - 2 : ntiles;
      if (pl_b < pl_e) {
        const int32_t *pt = a.ptab + rp * a.ptab_stride;
        pl_c0 = pt[c_abs + pl_b];
        pl_c1 = pt[c_abs + (rag ? ntiles - 1 : ntiles)];
      } else {
        pl_b = pl_e = ntiles;
      }
    }
    const int64_t col_begin = ((int64_t)a.ct0 + (int64_t)cs * a.tps + ti0) * BN;
    int64_t row0[RBW], irow_c[RBW];
    bool row_ok[RBW];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) {
      row0[rb] = rp * BM + (int64_t)(w * RBW + rb) * 32;
      const int64_t irow = row0[rb] + l31;
      row_ok[rb] = irow < M;
      irow_c[rb] = row_ok[rb] ? irow : (M - 1);
    }

    // ---- this wave's rows of X -> wave-private LDS panels Xw[rb][i][KpS] (rows past M are zero).
    //      forward B operand : lane (i = l31, half h) reads Xw[l31][h*Kp/2 + s]      (b128)
    //      GEMM3   B operand : lane (k = l31 + 32kb, half h) reads Xw[2s + h][k]     (b32)
    // (the panel's global loads are only ISSUED here; they are written to LDS after the first Y tile's loads have been
    //  issued as well, so that the piece's start-up pays one memory round trip, not two)
    constexpr int XV = (32 * Kp / 4) / 64;
    float4 xv0[RBW][XV];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) {
#pragma unroll
      for (int q = 0; q < XV; ++q) {   // 32 consecutive rows are contiguous in X (K x M column-major)
        const int e4 = lane + 64 * q;        // float4 index in the 32 x Kp block
        const int il = (e4 * 4) / Kp;
        const int64_t ir = row0[rb] + il < M ? row0[rb] + il : M - 1;   // clamped; rows past M are zeroed at the store
        xv0[rb][q] = *reinterpret_cast<const float4 *>(a.X + ir * Kp + (e4 * 4) % Kp);
      }
    }
    f32x16 gx[RBW][KB];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gx[rb][kb][r] = 0.f;
    // (XR) the X values this wave multiplies by do not change within a piece: both fragments are read from the panels
    // once, after the prologue's barrier, and stay in registers for all of its tiles (every index a compile-time constant)
    //   xf[q]: the forward's B operand of k-steps 4 q .. 4 q + 3 (this lane's row, its half of k)
    //   xg[q]: the cross-wave GEMM3's A operand of step q = 8 p + 2 u + hi
    float4 xf[XR ? KS / 4 : 1];
    float xg[XR ? 8 * NW : 1];

    // Y tile staging: global -> registers -> (scaled by sigma_j) -> LDS.  The scaling is applied at store time so
    // that nothing waits on the loads when they are issued.
    // The loads are issued unconditionally from clamped in-bounds addresses and their results are NOT touched until
    // stage_store (dead columns are zeroed there): nothing waits on a load where it is issued, and the compiler
    // knows how many VMEM operations are in flight (counted s_waitcnt vmcnt(N)).
    // (plain: a constant at every call; true = the tile is known to be a full one, PLAIN below)
    auto stage_load_y = [&](int64_t jt, int q, float4 (&yv)[YV], float (&sgv)[YV], bool plain = false) {
      const float *yb = a.Y + jt * Kp;       // the BN x Kp tile is contiguous in Y
      const float4 *cb = a.colp + jt;
      const int64_t rem = N - jt;
      if (HOIST && !(PLAINB && !plain && rem < BN)) {
        const bool rag = HOZ == 2 && rem < BN;
        yv[q] = *reinterpret_cast<const float4 *>(ho_at(yb, rag ? ho_y[HOZ - 1][q] : ho_y[0][q]));
        sgv[q] = *reinterpret_cast<const float *>(ho_at(cb, rag ? ho_s[HOZ - 1][q] : ho_s[0][q]));
        return;
      }
      const int ncol = rem > BN ? BN : (int)rem;  // live columns of this tile (>= 1)
      int e4 = tid + NT * q;
      if (e4 > BN * Kp / 4 - 1) e4 = BN * Kp / 4 - 1;
      int jl = (e4 * 4) / Kp;
      if (jl >= ncol) { jl = ncol - 1; e4 = jl * (Kp / 4); }
      yv[q] = *reinterpret_cast<const float4 *>(yb + e4 * 4);
      sgv[q] = cb[jl].x;
    };
    auto stage_load_c = [&](int64_t jt, float4 &cv, bool plain = false) {
      const float4 *cb = a.colp + jt;
      const int64_t rem = N - jt;
      if (HOIST && !(PLAINB && !plain && rem < BN)) {
        cv = *reinterpret_cast<const float4 *>(ho_at(cb, HOZ == 2 && rem < BN ? ho_c[HOZ - 1] : ho_c[0]));
        return;
      }
      const int ncol = rem > BN ? BN : (int)rem;
      cv = cb[tid < ncol ? tid : ncol - 1];
    };
    auto stage_load = [&](int64_t jt, float4 (&yv)[YV], float (&sgv)[YV], float4 &cv) {
#pragma unroll
      for (int q = 0; q < YV; ++q) stage_load_y(jt, q, yv, sgv);
      stage_load_c(jt, cv);
    };
    // jt = first column of the staged tile (decides which columns are dead)
    auto stage_store = [&](int ybuf, int cbuf, int64_t jt, const float4 (&yv)[YV], const float (&sgv)[YV], const float4 &cv, bool plain = false) {
      float *Yn = Ys + ybuf * Cfg::YT;
      const int64_t rem = N - jt;
      const int ncol = plain || rem > BN ? BN : (int)rem;
#pragma unroll
      for (int q = 0; q < YV; ++q) {
        const int e4 = tid + NT * q;
        if (e4 < BN * Kp / 4) {
          const int jl = (e4 * 4) / Kp, kf = (e4 * 4) % Kp;
          const float sg = plain || jl < ncol ? sgv[q] : 0.f;
          *reinterpret_cast<float4 *>(Yn + jl * KpS + kf) = make_float4(yv[q].x * sg, yv[q].y * sg, yv[q].z * sg, yv[q].w * sg);
        }
      }
      asm volatile("" ::"v"(cv.x), "v"(cv.y), "v"(cv.z), "v"(cv.w));   // counted wait here, not vmcnt(0) inside the branch
      if (tid < BN) {
        const bool livec = plain || tid < ncol;
        Csg[cbuf * BN + tid] = livec ? cv.x : 0.f;
        Cmu[cbuf * BN + tid] = livec ? cv.y : 0.f;
        Cw[cbuf * BN + tid] = livec ? cv.z : 0.f;
        Cmt[cbuf * BN + tid] = livec ? __float_as_int(cv.w) : 3;
        if (MIXED) {
          // noise kind of the tile as a whole (dead columns agree with anything): lets the epilogue take ONE model's
          // code path for the 32 columns instead of evaluating every model per entry
          const int kd = __float_as_int(cv.w) & 3;
          const unsigned m0 = (unsigned)__ballot(!livec || kd == 0), m1 = (unsigned)__ballot(!livec || kd == 1),
                         m2 = (unsigned)__ballot(!livec || kd == 2);
          if (tid == 0) Ck[cbuf] = m0 == 0xffffffffu ? 0 : (m1 == 0xffffffffu ? 1 : (m2 == 0xffffffffu ? 2 : 3));
        }
        if (bt_lds) {   // the view of the tile's columns when they all share one (-1: in no view); -2: the tile straddles views
          const int vw = (__float_as_int(cv.w) >> 2) - 1;
          const int vw0 = __builtin_amdgcn_readfirstlane(vw);
          const unsigned mv = (unsigned)__ballot(!livec || vw == vw0);
          if (tid == 0) Ck[2 + cbuf] = mv == 0xffffffffu ? vw0 : -2;
        }
      }
    };
    // (BATCH, LDS table) staging: thread tid takes entries (column tid & 31, slots (tid >> 5) + (NT / 32) q) -- a wave writes 32
    // consecutive words of two slot rows of each plane
    auto bt_e = [&](int q) { return (tid & 31) * 16 + (tid >> 5) + (NT / 32) * q; };
    auto bt_mu = [&](int64_t jt, int e) -> float { const int64_t j = jt + (e >> 4); return j < N ? a.colp[j].y : 0.f; };
    auto bt_store = [&](int e, const float2 &dt, float mu) __attribute__((always_inline)) {
      const int o = (e & 15) * 32 + (e >> 4);
      Btd[o] = dt.x;
      Btt[o] = dt.y + mu;
    };
    // gY of a finished tile: the NW per-wave LDS slabs are summed (16-B reads, slab-contiguous thread mapping) and
    // added to the workgroup's PRIVATE gY slab in HBM with a plain read-modify-write (no atomics in the loop).  The
    // old slab values are prefetched with the other loads of the tile (gold), half a tile before they are needed.
    // Thread -> float4 f of the [kb][j][32 k] slab; the same element of the [j][Kp] gY tile is e = j*Kp + 32 kb + k.
    float4 gold[RV4];
    PmfDTile<DB> dcur[RBW];   // this wave's D tiles (MFMA accumulator layout; raw bf16 words when D is stored as bf16)
    constexpr int DCH = PmfDTile<DB>::NCH;   // 1-KiB wave loads per tile: 4 (f32) or 2 (bf16)
    auto slab_map = [&](int q, int &so, int &e) -> bool {
      const int f = tid + NT * q;
      const bool in = f < BN * Kp / 4;
      const int ff = in ? f : 0;
      so = 4 * ff;
      e = ((ff % (BN * 8)) / 8) * Kp + 32 * (ff / (BN * 8)) + 4 * (ff % 8);
      return in;
    };
    auto slab_prefetch_one = [&](int64_t jt, int q, bool plain = false) {
      const float *sb = myslab + jt * Kp;
      const int64_t rem = N - jt;
      if (HOIST && !(PLAINB && !plain && rem < BN)) {
        gold[q] = pmf_load_stream(reinterpret_cast<const float4 *>(ho_at(sb, HOZ == 2 && rem < BN ? ho_g[HOZ - 1][q] : ho_g[0][q])));
        return;
      }
      const int nel = (rem > BN ? BN : (int)rem) * Kp;   // live elements of this gY tile (>= Kp)
      int so, e;
      if (XW) e = xw_e;
      else slab_map(q, so, e);
      gold[q] = pmf_load_stream(reinterpret_cast<const float4 *>(sb + (e < nel ? e : (e % Kp))));
    };
    // forward: acc[j,i] = mu_j + sum_k sigma_j Y[k,j] X[k,i]   (A = Y tile, B = X panel, both b128 LDS reads; the RBW
    // row blocks are independent accumulator chains sharing the A operand), with the slab reduction of the PREVIOUS
    // tile (jt_red) interleaved between its MFMAs.
    auto forward_reduce = [&](f32x16 (&acc)[RBW], int ybuf, int cbuf, bool do_red, int64_t jt_red) {
      const int cb0 = cbuf * BN + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float m0 = BATCH ? 0.f : Cmu[cb0 + (r & 3) + 8 * (r >> 2)];
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) acc[rb][r] = m0;
      }
      const float4 *yr = reinterpret_cast<const float4 *>(Ys + ybuf * Cfg::YT + l31 * KpS + h * (Kp / 2));
      const float4 *xr[RBW];
      float4 yv = yr[0], xv[RBW];
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb) {
        xr[rb] = reinterpret_cast<const float4 *>(Xw[rb] + l31 * KpS + h * (Kp / 2));
        xv[rb] = XR ? xf[0] : xr[rb][0];
      }
      constexpr int NIT = KS / 4, RTOT = NW * RV4, RPI = (RTOT + NIT - 1) / NIT;
      float4 racc[RV4];
      int so[RV4], eo[RV4];
      bool in[RV4];
#pragma unroll
      for (int q = 0; q < RV4; ++q) {
        racc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        in[q] = slab_map(q, so[q], eo[q]);
      }
#pragma unroll
      for (int q = 0; q < NIT; ++q) {
        float4 yn = yv, xn[RBW];
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) xn[rb] = xv[rb];
        if (q + 1 < NIT) {
          yn = yr[q + 1];
#pragma unroll
          for (int rb = 0; rb < RBW; ++rb) xn[rb] = XR ? xf[XR ? q + 1 : 0] : xr[rb][q + 1];
        }
        if (do_red) {
#pragma unroll
          for (int z = 0; z < RPI; ++z) {
            const int idx = q * RPI + z;
            if (idx < RTOT) {
              const float4 v = *reinterpret_cast<const float4 *>(Sl + (idx / RV4) * SLAB + so[idx % RV4]);
              float4 &ra = racc[idx % RV4];
              ra.x += v.x; ra.y += v.y; ra.z += v.z; ra.w += v.w;
            }
          }
        }
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.x, xv[rb].x, acc[rb], 0, 0, 0);
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.y, xv[rb].y, acc[rb], 0, 0, 0);
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.z, xv[rb].z, acc[rb], 0, 0, 0);
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.w, xv[rb].w, acc[rb], 0, 0, 0);
        yv = yn;
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) xv[rb] = xn[rb];
        __builtin_amdgcn_sched_barrier(0);
      }
      if (do_red && (FULL || !(dbg & 8))) {
        // make the (long finished) D loads count as consumed BEFORE the stores below are issued: otherwise the next
        // epilogue's wait for them becomes vmcnt(0) and also waits for these stores
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) {
          dcur[rb].touch();
        }
        const int64_t rem = N - jt_red;
        const int nel = (rem > BN ? BN : (int)rem) * Kp;
        float *sb = myslab + jt_red * Kp;
#pragma unroll
        for (int q = 0; q < RV4; ++q) {
          float4 v = racc[q];
          const float sgj = Csg[(cbuf ^ 1) * BN + eo[q] / Kp];   // ColScale pull-back: gY[:, j] *= sigma_j (tile t = other parity)
          v.x *= sgj; v.y *= sgj; v.z *= sgj; v.w *= sgj;
          if (!slab_first) { v.x += gold[q].x; v.y += gold[q].y; v.z += gold[q].z; v.w += gold[q].w; }
          if (in[q] && eo[q] < nel) pmf_store_stream(reinterpret_cast<float4 *>(sb + eo[q]), v);
        }
      }
    };

    // (issued before the staging below and its barrier: they are not needed until the first epilogue)
    // D tile loads: four contiguous 1-KiB wave loads per row block (see pmf_d_off).  Row blocks past the matrix are
    // clamped (their rows are masked by row_ok); pad rows / columns inside the matrix' last blocks are NaN.
    bool rows_in[RBW];
    int rb_u[RBW];
    uint32_t tflag[RBW];   // 'all finite' flags of the current tiles (raw: compared at use)
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) {
      const int rb_raw = __builtin_amdgcn_readfirstlane((int)(row0[rb] >> 5));   // wave-uniform row block (scalar)
      rows_in[rb] = rb_raw < a.nRB;   // false: these 32 rows lie entirely beyond the matrix
      rb_u[rb] = rows_in[rb] ? rb_raw : (int)a.nRB - 1;
      tflag[rb] = a.tflags[(col_begin >> 5) * a.nRB + rb_u[rb]];
#pragma unroll
      for (int q = 0; q < DCH; ++q) dcur[rb].load(a.D, (col_begin >> 5) * a.nRB + rb_u[rb], lane, q);
    }
    {
      float4 yv[YV], cv;
      float sgv[YV];
      stage_load(col_begin, yv, sgv, cv);
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
        for (int q = 0; q < XV; ++q) {
          const int e4 = lane + 64 * q;
          const int il = (e4 * 4) / Kp, kf = (e4 * 4) % Kp;
          *reinterpret_cast<float4 *>(Xw[rb] + il * KpS + kf) = row0[rb] + il < M ? xv0[rb][q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      stage_store(0, 0, col_begin, yv, sgv, cv);
      if (bt_lds) {
#pragma unroll
        for (int q = 0; q < NBT; ++q) {   // first tile: slot map straight from global memory (the LDS copy is not published yet)
          const int e = bt_e(q);
          bt_store(e, pmf_bt_entry(a, a.pm + rp * a.n_bv * 16, col_begin, e, pmf_bt_view(a, col_begin, e)), bt_mu(col_begin, e));
        }
        if (tid < a.n_bv * 16) Pm[tid] = a.pm[rp * a.n_bv * 16 + tid];
        if (h == 0)   // panel-local slot of this wave's rows in every view (15 = the identity slot: row in no batch)
#pragma unroll
          for (int rb = 0; rb < RBW; ++rb)
            for (int v = 0; v < a.n_bv; ++v) Bw0[rb * 512 + v * 32 + l31] = a.row_slot[(int64_t)v * M + irow_c[rb]];
      }
    }
    __syncthreads();
    if (XR) {
      const float4 *xr0 = reinterpret_cast<const float4 *>(Xw[0] + l31 * KpS + h * (Kp / 2));
#pragma unroll
      for (int q = 0; q < KS / 4; ++q) xf[XR ? q : 0] = xr0[q];
#pragma unroll
      for (int q = 0; q < 8 * NW; ++q) {
        const int p = q >> 3, u = (q >> 1) & 3, hi = q & 1;
        xg[XR ? q : 0] = *(lds_cptr)(uintptr_t)(xw_xa[u] + 4 * (p * Cfg::XP + 16 * hi * KpS));
      }
    }

    f32x16 acc[RBW];
    forward_reduce(acc, 0, 0, false, 0);

    // Steady state, per 32-column tile t (acc already holds the forward of tile t; the slabs are free):
    //   epilogue(t) | issue loads of tile t+1 | GEMM2(t) | GEMM3(t) -> slab | publish Y(t+1)
    //   -- barrier B1: slabs complete, Y(t+1) visible --
    //   reduce slabs(t) -> private gY slab (plain RMW) | forward(t+1)
    //   -- barrier B2: slabs free --
    // XW:  epilogue(t) -> G tile [t & 1] | issue loads of tile t+1 | GEMM2(t) | publish Y(t+1)
    //   -- the tile's barrier: the eight G tiles complete, Y(t+1) visible --
    //   cross-wave GEMM3(t) -> private gY slab (plain RMW) | forward(t+1)
    //
    // (PLAINB) Plain runs.  Three questions of the loop have the same answer for every tile of a run of consecutive
    // tiles of a piece, for all eight waves: is the tile all-finite (the packed epilogue), is it the matrix's ragged last
    // column tile (load offsets, dead columns, store predicate), is this the workgroup's first visit of the slab entry
    // (store or accumulate).  The loop body is one routine with a compile-time flag; a piece runs its first t_plain tiles
    // in the general instantiation and the rest in the PLAIN one, which answers "finite, full, not first" without asking:
    // no tile-flag load and test, offset set 0 only, gold always added, unpredicated store, no dead-column selects, the
    // packed epilogue only.  Same MFMAs on the same operands in the same order: bit-identical results.  The loop-carried
    // state (acc, dcur, gx, the loss sums) passes straight from one instantiation to the other; have_next still refers to
    // the piece's end.  The run starts at the first tile that is not a first visit and ends with the piece, if the tiles
    // in between are all-finite in all eight row blocks (two loads from the running counts of k_plain_table, by absolute
    // column tile); there is none in a segment visit's first piece and under PMF_PLAIN=0.
    // The ragged tile ends a piece of the last segment in every row panel (three tiles in ten at the headline size sit
    // in such pieces): there the run stops two tiles short, so that a general iteration issues the ragged tile's clamped
    // loads and its flag; the table answers for the tile in between (its flag was never loaded: set below).
    int t_plain = ntiles, t_pend = ntiles;
    if (PLAINB && a.plain) {
      const bool run = pl_b < pl_e && pl_c0 == pl_c1;
      t_plain = __builtin_amdgcn_readfirstlane(run ? pl_b : ntiles);
      t_pend = __builtin_amdgcn_readfirstlane(run ? pl_e : ntiles);
      n_plain += t_pend - t_plain;
    }
    auto tile_loop = [&](auto plain_flag, const int t_begin, const int t_end) __attribute__((always_inline)) {
    constexpr bool PLAIN = decltype(plain_flag)::value;
    for (int t = t_begin; t < t_end; ++t) {
      const int par = t & 1;
      const int cur = NYB == 2 ? par : 0, nxt = NYB == 2 ? (par ^ 1) : 0;
      const int64_t j0 = col_begin + (int64_t)t * BN;
      const float *Yc = Ys + cur * Cfg::YT;
      const bool have_next = (t + 1 < ntiles);
      const int cb0 = par * BN + 4 * h;  // column-parameter index of register 0
      float4 ynext[YV], cnext;
      float2 btn[NBT];   // (BATCH) the next tile's slice of the dense batch table
      float btm[NBT];    //         and its columns' mu
      int btv[NBT];
      float sgnext[YV];
      PMF_STAMP(0);   // (loop overhead / previous B2 exit)
      // (XW) sigma of this lane's gY column, read BEFORE the tile's barrier: past it a faster wave may already be
      // staging tile t+2's column parameters into this parity
      const float xw_sg = XW ? Csg[par * BN + xw_j] : 0.f;

      // ---- epilogue: (batch layers,) masked loss, dloss/dZ in place (acc becomes G).  G is also written, transposed,
      //      to the wave-private tile T, 16 B (four registers) at a time: element (i, j) lives at
      //      T[i*32 + 4*((j>>2) ^ (i&7)) + (j&3)] -- conflict-free b128 writes here, conflict-free b32 reads in GEMM3.
      //      (T holds G itself; the column scale sigma_j of gY is applied once per tile in the slab reduction.)
      //      VALU instructions do not overlap with f32 MFMAs, so their COUNT is what matters: tiles whose 1024 entries
      //      are all finite (flag computed when D is laid out) take a packed-math path without the per-entry mask.
      float lsum = 0.f;
      const int tkind = MIXED ? __builtin_amdgcn_readfirstlane(Ck[par]) : 0;   // wave-uniform: a scalar branch per entry group
      const int tview = bt_lds ? __builtin_amdgcn_readfirstlane(Ck[2 + par]) : -1;   // the tile's view; -2: it straddles two
      // General epilogue of ONE accumulator register r of row block rb (column j = rowmap(r,h) of the tile, row = this lane's
      // row), given the batch scale dl and the shift th = theta + mu_j of the entry (batch layers only).
      // Gaussian columns mask by substitution -- a missing entry takes y := z, hence d = 0, g = 0, no loss -- and sum g d
      // (halved once per tile): one select per entry instead of two, the loss in one fma; all-finite tiles (fast) skip it.
      float lnorm = 0.f;
      auto epi_reg = [&](int rb, int r, float dl, float th, float wj, int kmode, bool fast) __attribute__((always_inline)) {   // kmode: 0/1/2 = the whole tile is that noise model, 3 = per column
        if (dbg & 4) return;
        float z = acc[rb][r];
        if (BATCH) z = fmaf(z, dl, th);   // (without batch layers mu_j was the accumulator's initial value: acc is z)
        float y = dcur[rb].get(r);
        if (kmode == PMF_NOISE_NORMAL) {
          if (!fast) y = (pmf_finite(y) && row_ok[rb]) ? y : z;
          const float d = z - y, g = wj * d;
          lnorm = fmaf(g, d, lnorm);
          acc[rb][r] = BATCH ? g * dl : g;
        } else {
          const bool ok = pmf_finite(y) && row_ok[rb];
          float l, g;
          if (kmode == 3) pmf_noise<MIXED>(Cmt[cb0 + (r & 3) + 8 * (r >> 2)] & 3, z, y, wj, a.htab + (j0 + 4 * h) * PMF_HT + PMF_HT * ((r & 3) + 8 * (r >> 2)), l, g);
          else pmf_noise(kmode, z, y, wj, nullptr, l, g);
          lsum += ok ? l : 0.f;
          acc[rb][r] = ok ? (BATCH ? g * dl : g) : 0.f;
        }
      };
      // {delta, theta + mu} of the four columns of register chunk c4 (this lane's half h) for row block rb
      auto grp_load = [&](int rb, int c4, bool uni, const float *bdl, const float *btl, float4 &dl4, float4 &th4) __attribute__((always_inline)) {
        if (!BATCH) {
          th4 = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (bt_lds && uni) {
          dl4 = *reinterpret_cast<const float4 *>(bdl + 8 * c4);
          th4 = *reinterpret_cast<const float4 *>(btl + 8 * c4);
        } else {
          float dv[4], tv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int cl = 8 * c4 + 4 * h + u;
            const int v = (Cmt[par * BN + cl] >> 2) - 1;
            dv[u] = 1.f;
            if (bt_lds) {   // the tile straddles two views: view and slot per entry
              const int bsr = v < 0 ? 15 : Bw0[rb * 512 + v * 32 + l31];
              dv[u] = Btd[bsr * 32 + cl];
              tv[u] = Btt[bsr * 32 + cl];
            } else {        // per-entry gathers from the global table (a row panel that meets more than 15 batches of a view)
              tv[u] = Cmu[par * BN + cl];
              if (v >= 0) {
                const int64_t vc0 = a.views[v].c0, vto = a.views[v].tab_off;
                const int vnb = a.views[v].nb;
                const int b = a.bor[(int64_t)v * M + irow_c[rb]];
                if (b >= 0) {
                  const float2 dt = a.btab[vto + (j0 + cl - vc0) * vnb + b];
                  dv[u] = dt.x;
                  tv[u] += dt.y;
                }
              }
            }
          }
          dl4 = make_float4(dv[0], dv[1], dv[2], dv[3]);
          th4 = make_float4(tv[0], tv[1], tv[2], tv[3]);
        }
      };
      // column parameters of the 4 columns of register chunk c4 (this lane's half h): one 16-B LDS read per array,
      // constant offsets from two per-tile base pointers (no per-register address arithmetic)
      const float4 *cw4 = reinterpret_cast<const float4 *>(Cw + cb0);
      auto f4get = [](const float4 &v, int u) { return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w)); };

      // The tile's global loads (old private-slab values of tile t; Y, column parameters, D and flags of tile t+1)
      // are issued one per GEMM2 step: eight waves issuing all of them at once queue up behind the CU's single address
      // path (measured: 12 % of the wave time); spread between the MFMAs they cost nothing.  (The last tile of a
      // piece re-loads itself: unconditional loads keep the loop branch-free.)
      const int64_t jn = have_next ? j0 + BN : j0;
      constexpr int NOTH = YV + 1 + RV4 + (BATCH ? NBT : 0);     // the non-D loads, in the order they are needed
      constexpr int DPR = DCH + (PLAIN ? 0 : 1);
      constexpr int NVM = NOTH + DPR * RBW;                        // + per row block: the D chunks and (not PLAIN) the tile flag
      bool tile_fast[RBW];
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb) tile_fast[rb] = PLAIN || (rows_in[rb] && tflag[rb] != 0);
      auto vmem_op = [&](int i) {
        if (i == 0 && bt_lds) {   // the views of the table entries this thread fetches below (address of those loads)
#pragma unroll
          for (int q = 0; q < NBT; ++q) btv[q] = pmf_bt_view(a, jn, bt_e(q));
        }
        if (i < YV) stage_load_y(jn, i, ynext, sgnext, PLAIN);
        else if (i == YV) stage_load_c(jn, cnext, PLAIN);
        else if (i < YV + 1 + RV4) { if (want_gy) slab_prefetch_one(j0, i - YV - 1, PLAIN); }
        else if (i < NOTH) {
          const int q = i - YV - 1 - RV4;
          if (bt_lds) { btn[q] = pmf_bt_entry(a, Pm, jn, bt_e(q), btv[q]); btm[q] = bt_mu(jn, bt_e(q)); }
        }
        else if (i < NVM) {
          const int rb = (i - NOTH) / DPR, q = (i - NOTH) % DPR;
          if (q < DCH) {
            if (FULL || !(dbg & 2)) dcur[rb].load(a.D, (jn >> 5) * a.nRB + rb_u[rb], lane, q);
          } else {
            tflag[rb] = a.tflags[(jn >> 5) * a.nRB + rb_u[rb]];
          }
        }
      };
      typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb) {
        if (!BATCH && tile_fast[rb] && (!MIXED || tkind == 0)) {
          // all 1024 entries finite (which also means: no pad rows): g = w (z - y), loss = 0.5 sum g (z - y), packed
          f32x2 ls2 = {0.f, 0.f};
          if (!(dbg & 4)) {
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
              const float4 w4 = cw4[2 * c4];
#pragma unroll
              for (int p2 = 0; p2 < 2; ++p2) {
                const int r = 4 * c4 + 2 * p2;
                const f32x2 zz = {acc[rb][r], acc[rb][r + 1]}, yy = {dcur[rb].get(r), dcur[rb].get(r + 1)};
                const f32x2 ww = p2 == 0 ? f32x2{w4.x, w4.y} : f32x2{w4.z, w4.w};
                f32x2 dd;   // packed z - y (kept out of the compiler's hands: it would split it into two v_sub_f32)
                asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(dd) : "v"(zz), "v"(yy));
                const f32x2 gg = ww * dd;
                ls2 = gg * dd + ls2;
                acc[rb][r] = gg.x; acc[rb][r + 1] = gg.y;
              }
            }
          }
          lsum += 0.5f * (ls2.x + ls2.y);
        } else {
          // one specialised copy of the general epilogue per noise model (the model is a compile-time constant inside)
          int bs = 15;
          if (bt_lds && tview >= 0) bs = Bw0[rb * 512 + tview * 32 + l31];   // this row's slot in the tile's view: once per tile
          const float *bdl = Btd + bs * 32 + 4 * h, *btl = Btt + bs * 32 + 4 * h;
          auto epi_all = [&](int kmode, bool uni, bool fast) __attribute__((always_inline)) {
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
              const float4 w4 = cw4[2 * c4];
              float4 dl4 = make_float4(1.f, 1.f, 1.f, 1.f), th4;
              grp_load(rb, c4, uni, bdl, btl, dl4, th4);
#pragma unroll
              for (int u = 0; u < 4; ++u) epi_reg(rb, 4 * c4 + u, f4get(dl4, u), f4get(th4, u), f4get(w4, u), kmode, fast);
            }
          };
          const bool uni = !bt_lds || tview != -2;
          if (!uni) epi_all(3, false, false);
          // (the mask-free copy is for the batch variants: without batch layers an all-finite Gaussian tile took the packed path above)
          else if (!MIXED || tkind == 0) { if (BATCH && tile_fast[rb]) epi_all(PMF_NOISE_NORMAL, true, true); else epi_all(PMF_NOISE_NORMAL, true, false); }
          else if (tkind == 1) epi_all(PMF_NOISE_BERNOULLI, true, false);
          else if (tkind == 2) epi_all(PMF_NOISE_POISSON, true, false);
          else epi_all(3, true, false);
        }
        if (want_gy) {
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4)
            *reinterpret_cast<float4 *>((XW ? Sl + (par * NW + w) * 1024 : T[rb]) + l31 * 32 + 4 * ((2 * c4 + h) ^ (l31 & 7))) =
                make_float4(acc[rb][4 * c4], acc[rb][4 * c4 + 1], acc[rb][4 * c4 + 2], acc[rb][4 * c4 + 3]);
        }
      }
      PMF_STAMP(1);   // epilogue
      // ---- GEMM2: gX[i,k] += sum_j G[j,i] * sigma_j Y[k,j]   (A = acc register s, B from the Y tile, shared by the
      //      row blocks).  Every step is fenced (sched_barrier) so that the order written here is the order issued:
      //      the B operands of step s+2 are read, one global load is issued, then the MFMAs of step s.
      if (want_gx) {
        float bq[3][KB];
        unsigned g2_y = g2_lane + (unsigned)(cur * Cfg::YT * 4);   // (Y1BASE) this tile's base, opaque: nothing to re-derive
        if (Y1BASE) asm volatile("" : "+v"(g2_y));
        auto g2_read = [&](int s, int kb) -> float {
          // (volatile: keeps each read a ds_read_b32 at its own offset; merged into pairs they need the eight bases again)
          if (Y1BASE) return *(const volatile __attribute__((address_space(3))) float *)(uintptr_t)(g2_y + 4 * (pmf_rowmap(s, 0) * KpS + 32 * kb));
          return (Yc + pmf_rowmap(s, h) * KpS + l31)[32 * kb];
        };
#pragma unroll
        for (int s0 = 0; s0 < 2; ++s0) {
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) bq[s0][kb] = g2_read(s0, kb);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          if (s + 2 < 16) {
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) bq[(s + 2) % 3][kb] = g2_read(s + 2, kb);
          }
          if (s < NVM) vmem_op(s);
#pragma unroll
          for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
              gx[rb][kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[rb][s], bq[s % 3][kb], gx[rb][kb], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 16; i < NVM; ++i) vmem_op(i);
      } else if (GM != 2) {
#pragma unroll
        for (int i = 0; i < NVM; ++i) vmem_op(i);
      }
      lossacc += (double)fmaf(0.5f, lnorm, lsum);

      PMF_STAMP(3);   // GEMM2
      // ---- GEMM3: gY[j,k] = sum_i G[j,i] * X[k,i] over the wave's 32*RBW rows; results go to this wave's slab
      //      [kb][j][32] with plain stores (the last k block overwrites the first transposed tile, which it has just
      //      consumed: same wave, in-order LDS)
      if (want_gy && !XW) {
        __builtin_amdgcn_wave_barrier();
        // all KB k-blocks advance together: KB independent accumulator chains, and the A operand (one element of a
        // transposed tile) is read once per step instead of once per k block
        f32x16 gy[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) gy[kb][r] = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const int i = 2 * s + h;
          if (GM == 2 && s < NVM) vmem_op(s);   // grad(Y)-only launches have no GEMM2: the tile's loads are spread here
#pragma unroll
          for (int rb = 0; rb < RBW; ++rb) {
            const float av = T[rb][i * 32 + 4 * ((l31 >> 2) ^ (i & 7)) + (l31 & 3)];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
              gy[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, Xw[rb][i * KpS + 32 * kb + l31], gy[kb], 0, 0, 0);
          }
        }
        if (GM == 2) {
#pragma unroll
          for (int i = 16; i < NVM; ++i) vmem_op(i);
        }
        // the slab's last k block aliases T[0]: it is written last, after every read of T has been issued (in-order LDS)
        if (!(dbg & 32)) {
#pragma unroll
          for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) Sw[kb * 1024 + pmf_rowmap(r, h) * 32 + l31] = gy[kb][r];
        } else {
          f32x16 keep = gy[0];
#pragma unroll
          for (int kb = 1; kb < KB; ++kb) keep += gy[kb];
          asm volatile("" ::"v"(keep));
        }
      }

      PMF_STAMP(4);   // GEMM3 + slab writes
      // ---- publish Y(t+1); B1 also completes this tile's slabs
      if (NYB == 1) __syncthreads();   // single Y buffer: every wave is done reading Y(t)
      stage_store(nxt, par ^ 1, jn, ynext, sgnext, cnext, PLAIN);
      PMF_STAMP(5);   // stage_store (waits for the Y loads)
      __syncthreads();                 // B1
      PMF_STAMP(6);   // B1 wait

      if (bt_lds) {   // every wave is past its epilogue(t): the single table buffer can take tile t+1 (read after B2)
#pragma unroll
        for (int q = 0; q < NBT; ++q) bt_store(bt_e(q), btn[q], btm[q]);
      }
      // ---- forward of tile t+1 with the reduction of tile t's slabs into the private gY slab inside it
      slab_first = !PLAIN && (pidx == 0 || (pidx == 1 && ti0 + t < t0_first));
      if (XW) {
        // ---- cross-wave GEMM3: gY[xw_j, xw_k..+3] = sum over the panel's 256 rows of X[k, i] G[i, j].  64 MFMAs in two
        //      independent accumulator chains (32-cycle issue, 40-cycle dependent latency), operands read XW_AHEAD steps
        //      ahead into a ring of registers; every step is fenced so that the order written is the order issued.
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        constexpr int XW_RING = 8, XW_AHEAD = 6;
        const float *Gp = Sl + par * (NW * 1024);
        int xt_g[4];        // (TIGHT) xw_g / xw_xa again, from a lane id the compiler cannot hoist out of the tile loop
        unsigned xt_xa[4];
        if (TIGHT) {
          int lo = lane;
          asm volatile("" : "+v"(lo));
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int i = 4 * (lo >> 4) + u, j = 16 * (w & 1) + (lo & 15);
            xt_g[u] = i * 32 + 4 * ((j >> 2) ^ (i & 7)) + (j & 3);
            xt_xa[u] = (unsigned)(uintptr_t)(lds_cptr)(Xs + 4 * (lo >> 4) * KpS + 16 * (w >> 1) + (lo & 15) + u * KpS);
          }
        }
        float xa[XW_RING], xb[XW_RING];   // (XR: xa is unused, the A operand of step q is xg[q])
        // steps q = 8 p + 2 u + hi: rows i and i + 16 of one block are read together -- both strides (16 rows of X or G, one
        // block of either) are multiples of 256 B, so every read is one half of a ds_read2st64_b32 off four bases per operand
        auto xw_read = [&](int q) __attribute__((always_inline)) {
          const int p = q >> 3, u = (q >> 1) & 3;
#pragma unroll
          for (int hi = 0; hi < 2; ++hi) {
            if (!XR) xa[(q + hi) % XW_RING] = *(lds_cptr)(uintptr_t)((TIGHT ? xt_xa[u] : xw_xa[u]) + 4 * (p * Cfg::XP + 16 * hi * KpS));
            xb[(q + hi) % XW_RING] = Gp[p * 1024 + (TIGHT ? xt_g[u] : xw_g[u]) + 512 * hi];
          }
        };
#pragma unroll
        for (int q = 0; q < XW_AHEAD; q += 2) xw_read(q);
        f32x4 gy0 = {0.f, 0.f, 0.f, 0.f}, gy1 = {0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 8 * NW; q += 2) {
          if (q + XW_AHEAD < 8 * NW) xw_read(q + XW_AHEAD);
          gy0 = __builtin_amdgcn_mfma_f32_16x16x4f32(XR ? xg[XR ? q : 0] : xa[q % XW_RING], xb[q % XW_RING], gy0, 0, 0, 0);
          gy1 = __builtin_amdgcn_mfma_f32_16x16x4f32(XR ? xg[XR ? q + 1 : 0] : xa[(q + 1) % XW_RING], xb[(q + 1) % XW_RING], gy1, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        // make the (long finished) D loads count as consumed BEFORE the store below is issued: otherwise the next
        // epilogue's wait for them becomes vmcnt(0) and also waits for this store
        dcur[0].touch();
        const int64_t rem = N - j0;
        const int nel = (rem > BN ? BN : (int)rem) * Kp;
        float4 v = make_float4((gy0[0] + gy1[0]) * xw_sg, (gy0[1] + gy1[1]) * xw_sg, (gy0[2] + gy1[2]) * xw_sg, (gy0[3] + gy1[3]) * xw_sg);
        if (!slab_first) { v.x += gold[0].x; v.y += gold[0].y; v.z += gold[0].z; v.w += gold[0].w; }
        // (PLAIN: through the pinned offset the old values were loaded from -- one address for both, not two induction pointers)
        if (PLAIN) pmf_store_stream(reinterpret_cast<float4 *>(const_cast<char *>(ho_at(myslab + j0 * Kp, ho_g[0][0]))), v);
        else if (xw_e < nel) pmf_store_stream(reinterpret_cast<float4 *>(myslab + j0 * Kp + xw_e), v);
        PMF_STAMP(4);   // GEMM3 + gY store
        // forward of tile t+1 (unconditional, as everything in this loop: a piece's last tile repeats its own, and a
        // branch would cost the sixteen register copies of a conditional acc per tile).  G(t+2) and Y(t+2) overwrite
        // G(t) and Y(t) only after the barrier of tile t+1, which every wave reaches after this GEMM3(t) and its
        // GEMM2(t+1); the LDS batch table has one buffer and keeps the second barrier
        forward_reduce(acc, nxt, par ^ 1, false, 0);
        PMF_STAMP(8);   // forward
        if (bt_lds) __syncthreads();
        PMF_STAMP(9);
      } else {
        if (FULL || have_next) forward_reduce(acc, nxt, par ^ 1, want_gy && !(dbg & 1), j0);
        else if (want_gy && !(dbg & 1)) { f32x16 dummy[RBW]; forward_reduce(dummy, nxt, par ^ 1, true, j0); }
        PMF_STAMP(8);   // forward + slab reduce
        // B2: slabs (and the transposed tiles, and the batch table) are free again; a grad(X)-only launch has none of them
        if ((GM != 1 || bt_lds) && !(dbg & 16)) __syncthreads();
        PMF_STAMP(9);   // B2 wait
      }
    }
    };
    if constexpr (PLAINB) {
      // at most three runs: general, plain, general (the two tiles up to the ragged one)
      tile_loop(PmfFlag<false>{}, 0, t_plain);
      tile_loop(PmfFlag<PLAINB>{}, t_plain, t_pend);
      if (t_pend < ntiles) {
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) tflag[rb] = 1;   // of tile t_pend: all-finite by the table, its flag was not loaded
        tile_loop(PmfFlag<false>{}, t_pend, ntiles);
      }
    } else {
      tile_loop(PmfFlag<false>{}, 0, ntiles);
    }
    // (XW) the next piece's prologue overwrites this wave's X panel, which the other waves read in the last GEMM3.
    // (XR) The panels are read only right after the prologue's barrier, but this barrier protects more than them: the
    // next piece's first epilogue writes G tile parity 0 and its stage_store writes Y buffer 0, both of which slower
    // waves may still be reading in their last GEMM3 and forward.
    if (XW && !bt_lds) __syncthreads();

    PMF_STAMP(10);
    // ---- flush gX (lane = factor index k, register = row): plain stores of the piece's whole BM x Kp partial to its own
    //      slot (rows past M hold exact zeros: their G is masked), summed in fixed order by k_gx_reduce -- no atomics
    if (want_gx) {
      float *gp = a.gx_part + (int64_t)gx_slot * a.gx_slot_stride + (int64_t)(w * RBW) * 32 * Kp + l31;
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) gp[(rb * 32 + pmf_rowmap(r, h)) * Kp + 32 * kb] = gx[rb][kb][r];
    }
    ++gx_slot;
    PMF_STAMP(11);  // piece prologue/epilogue (X panel, first tile, gX flush)
  }
  // ---- deterministic loss partial of this workgroup (its pieces in order, waves in order)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossacc += __shfl_xor(lossacc, off, 64);
  if (lane == 0) red[w] = lossacc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int q = 0; q < NW; ++q) s += red[q];
    a.loss_partial[wg] = s;
    if (PLAINB && a.plain_count) a.plain_count[wg] = n_plain;
  }
#ifdef PMF_STAMPS
  st_acc[14] = __builtin_amdgcn_s_memtime() - st_t0;          // shader clocks over the whole kernel
  st_acc[15] = __builtin_amdgcn_s_memrealtime() - st_r0;      // 100 MHz reference clocks over the same span
  if (a.stamps && (threadIdx.x & 63) == 0) {
    for (int q = 0; q < 16; ++q) a.stamps[((int64_t)blockIdx.x * NW + (threadIdx.x >> 6)) * 16 + q] = st_acc[q];
  }
#endif
}
