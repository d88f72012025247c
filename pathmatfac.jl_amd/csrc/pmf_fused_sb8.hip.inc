// pmf_fused_sb8.hip.inc -- the fused data pass on a TALL ROW PANEL: 256 rows for 96 < K <= 128 (KB = 4), 512 rows for
// 32 < K <= 64 (KB = 2) (included by pmf_k_sb8.hip).  The text below describes KB = 4; KB = 2 has half the per-row state, so
// each wave owns FOUR row blocks, and its cross-wave GEMM3 gives every wave 16 factors over all 512 rows on
// v_mfma_f32_16x16x32_bf16 (same matrix cycles as 32x32x16, no padding of the 32-wide shape).
//
// Why: with the 128-row panel of pmf_fused_sb4_kernel the private gY slab's read-modify-write is 2 x 16 KiB per (panel,
// tile) against 8 KiB of bf16 D -- 100 GB of the 174 GB that kernel moves per launch at 125000 x 100000 (DESIGN.md 4.7).
// Slab traffic and the re-streamed Y operand images both scale with 1 / (panel height).  What bounds the height is the
// register file: per row the kernel holds grad(X) accumulators (512 B), the forward's X fragments and GEMM3's transposed X
// fragments.  This kernel fits 256 rows by
//   * running the FORWARD on f16 pairs (pmf_common.h, Sb8Cfg): two terms instead of bf16's three (X fragments 512 B per row
//     instead of 768 B) and three MFMAs per k-step instead of six, at 1e-7 of max|Z| (scripts/f16x2_probe.hip);
//   * a CROSS-WAVE GEMM3: wave w computes the tile's gY for factors 32 w .. 32 w + 31 over all 256 rows, reading the eight row
//     blocks' G images from LDS -- no per-wave partial tiles, no LDS slabs, the accumulator goes straight into the private slab
//     (one 128-byte line per half-wave and register);
//   * keeping the hi term of GEMM3's transposed X operand in LDS (64 KiB, staged once per piece) and only the mid term in
//     registers.
// Four waves, one per SIMD, each owning two 32-row blocks (rows 64 w .. 64 w + 63 of the panel): 512 registers per lane.
// Per tile and wave: 2 x (24 forward + 24 GEMM2) + 48 GEMM3 = 144 MFMAs for 64 rows (pmf_fused_sb4_kernel: 96 for 32).
// Same work split, private gY slabs, gX slots, epilogue arithmetic and outputs as the other fused kernels.

// ---- operand images (one workgroup of 256 threads per 32 rows of X / 32 columns of Y; see Sb8Cfg)
#if !PMF_DB && PMF_KB == 4   // (one copy: the translation unit of the K = 128, f32-storage variant holds the small kernels)
__global__ __launch_bounds__(256) void k_sb8_absmax(const Sb8ScaleArgs a) {
  const int k4 = a.Kp / 4;       // float4 per row
  const int64_t n4 = a.n * k4;
  float m = 0.f;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4 *>(a.src)[e];
    const float s = a.colp ? fabsf(a.colp[e / k4].x) : 1.f;
    // (a NaN must win: fmaxf drops it)
    const float q = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))) * s;
    const bool bad = !(v.x == v.x) || !(v.y == v.y) || !(v.z == v.z) || !(v.w == v.w);
    m = bad ? __uint_as_float(0x7fc00000u) : (m == m ? fmaxf(m, q) : m);
  }
  uint32_t u = __float_as_uint(m);   // non-negative floats (and NaN above them) order like their bit patterns
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)u, off, 64); u = o > u ? o : u; }
  if ((threadIdx.x & 63) == 0) atomicMax(a.max_bits, u);   // (an integer maximum: order-independent, deterministic)
}
// scale = 2^(12 - floor(log2 max)): max|s a| in [2^12, 2^13); 1 when there is nothing to scale by (zero, Inf, NaN: those
// reach the loss unchanged and end the fit as "nonfinite", like the exact kernel)
__global__ void k_sb8_scale_fin(const Sb8ScaleArgs a) {
  const float m = __uint_as_float(*a.max_bits);
  float s = 1.f;
  if (m > 0.f && m <= 3.0e38f) {
    int e = 12 - ilogbf(m);
    e = e < -60 ? -60 : (e > 60 ? 60 : e);
    s = ldexpf(1.f, e);
  }
  *a.scale_out = s;
}

// thread = (row, 16 factors as two 16-B chunks) at Kp = 128, (row, 8 factors) at Kp = 64
template <int KB>
__global__ __launch_bounds__(256) void k_sb8_split(const Sb8SplitArgs a) {
  constexpr int IMG = Sb8Cfg<KB>::IMG, Kp = 32 * KB, CPT = KB / 2;   // chunks per thread
  __shared__ __attribute__((aligned(16))) __bf16 tr[2][Kp][32 + 8];   // [term][k][i]
  const int64_t blk = blockIdx.x;
  if (blk >= a.nblk) return;
  const int tid = threadIdx.x, r = tid >> 3, c0 = (tid & 7) * CPT;
  const int64_t row = blk * 32 + r;
  char *ob = a.out + blk * (int64_t)(4 * IMG);
  const float sc = *a.scale;
#pragma unroll
  for (int cc = 0; cc < CPT; ++cc) {
    const int ch = c0 + cc;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < a.n) {
      const float4 p0 = *reinterpret_cast<const float4 *>(a.src + row * Kp + ch * 8);
      const float4 p1 = *reinterpret_cast<const float4 *>(a.src + row * Kp + ch * 8 + 4);
      const float s = a.colp ? a.colp[row].x : 1.f;
      v[0] = p0.x * s; v[1] = p0.y * s; v[2] = p0.z * s; v[3] = p0.w * s;
      v[4] = p1.x * s; v[5] = p1.y * s; v[6] = p1.z * s; v[7] = p1.w * s;
    }
    f16x8 fh, fl;
    bf16x8 bh, bm;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float vs = v[q] * sc;
      fh[q] = (_Float16)vs;
      fl[q] = (_Float16)((vs - (float)fh[q]) * 2048.f);
      bh[q] = (__bf16)v[q];
      bm[q] = (__bf16)(v[q] - (float)bh[q]);
      if (a.transposed) { tr[0][ch * 8 + q][r] = bh[q]; tr[1][ch * 8 + q][r] = bm[q]; }
    }
    const int off = pmf_sb8_y_off<KB>(r, ch), foff = pmf_sb8_f_off<KB>(r, ch);
    *reinterpret_cast<f16x8 *>(ob + foff) = fh;
    *reinterpret_cast<f16x8 *>(ob + IMG + foff) = fl;
    if (!a.transposed) {
      *reinterpret_cast<bf16x8 *>(ob + 2 * IMG + off) = bh;
      *reinterpret_cast<bf16x8 *>(ob + 3 * IMG + off) = bm;
    }
  }
  if (a.transposed) {
    __syncthreads();
    // [k][i]: Kp rows of 64 bytes per image = 4 Kp 16-B pieces per image
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < CPT; ++q) {
        const int pc = tid + 256 * q, k = pc >> 2, c = pc & 3;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = tr[t][k][8 * c + e];
        *reinterpret_cast<bf16x8 *>(ob + (2 + t) * IMG + pmf_sb8_xt_off(k, c)) = o;
      }
  }
}
#endif

#ifndef PMF_ABLATE
#define PMF_ABLATE 0   // measurement-only builds (WRONG results), one cost at a time: 1 no private-slab read-modify-write in HBM
                       // 2 no GEMM3 (reads + MFMAs)  4 no GEMM2 (reads + MFMAs)  8 no epilogue arithmetic  16 no forward (reads + MFMAs)
                       // 32 no G image writes  64 no staging of the next Y tile  128 no loads of D
#endif

// The register file is full (512 per lane) and split in two halves of 256: hipcc must be TOLD which half a value lives in, or
// it parks MFMA operands in the wrong one and copies them back and forth (270 copies and 50 scratch reloads per tile in the
// first build of this kernel: 99 ms instead of 47).  The accumulator half holds what only MFMAs touch for a whole piece --
// grad(X) accumulators ("+a") and the forward's X fragments ("a") = 256 registers exactly; everything else is a VGPR.
// Inline-asm MFMAs get no hazard padding from the compiler (cdna_hip_programming.md 5.7): every string opens with s_nop 1
// (a just-written operand -> MFMA), and the last MFMA of a chain whose result the VALU reads next closes with s_nop 11.
#define PMF_SB8_FWD(acc, yA, xB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(yA), "a"(xB))
#define PMF_SB8_FWD0(acc, yA, xB) /* first of a chain: C = 0 instead of sixteen zeroed registers */ \
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(yA), "a"(xB))
#define PMF_SB8_FWD_LAST(acc, yA, xB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_f16 %0, %1, %2, %0\n\ts_nop 11" : "+v"(acc) : "v"(yA), "a"(xB))
#define PMF_SB8_GY(acc, gA, xB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(gA), "v"(xB))
#define PMF_SB8_GY_LAST(acc, gA, xB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0\n\ts_nop 11" : "+v"(acc) : "v"(gA), "v"(xB))
#define PMF_SB8_GY16(acc, gA, xB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(gA), "v"(xB))
#define PMF_SB8_GY16_LAST(acc, gA, xB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0\n\ts_nop 11" : "+v"(acc) : "v"(gA), "v"(xB))
#define PMF_SB8_GX(acc, gA, yB) \
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(gA), "v"(yB))
typedef float pmf_acc4 __attribute__((ext_vector_type(4)));
#ifndef PMF_B3R_ALL
#define PMF_B3R_ALL 0
#endif
#ifndef PMF_B3LATE
#define PMF_B3LATE 1
#endif
template <int KB, bool MIXED, bool BATCH, bool DB>
__global__ __launch_bounds__(256, 1) void pmf_fused_sb8_kernel(const FusedArgs a) {
  using Cfg = Sb8Cfg<KB>;
  constexpr int NW = Cfg::NW, RB = Cfg::RB, NBLK = Cfg::NBLK, NT = 256, Kp = Cfg::Kp, BN = PMF_BN, BM = Cfg::BM;
  constexpr int IMG = Cfg::IMG, XBLK = Cfg::XBLK, YBLK = Cfg::YBLK;
  constexpr int FS = 2 * KB;        // k-steps of the forward (16 factors each)
  constexpr int NG = 2 * KB;        // (16-column step, k block) groups of GEMM2, per row block
  constexpr int NI = 16;            // steps of the cross-wave GEMM3: sixteen 16-row steps of 32 factors (KB = 4, 256 rows) or
                                    // sixteen 32-row steps of 16 factors (KB = 2, 512 rows); one X^T fragment each
  constexpr int NYC = KB;           // 16-B chunks per thread of a staged image pair (2 IMG bytes / 256 threads)
  constexpr int YRS = 64 * KB;      // bytes per row of the bf16 Y image
  // The mid term of GEMM3's transposed X operand (64 registers per lane) stays in registers for a whole piece only in the
  // plain variant.  The general epilogues (noise models, batch layers) need those registers: their variants fetch the
  // fragments again every tile (16 x 16 B per lane from L2, issued during GEMM2 of the second row block: 64 KiB per tile and CU,
  // hot in L2) instead of spilling to scratch, which cost 4x the kernel time.
  constexpr bool B3R = PMF_B3R_ALL ? true : (!MIXED && !BATCH);
  // (Tried and dropped, round 3: issuing the epilogue of row block b between the forward MFMAs of row block b + 1 -- a wave is
  //  alone on its SIMD, so nothing else fills the matrix pipe during the epilogue.  Parity-green, SLOWER: K = 64 16.2 -> 16.9 ms,
  //  K = 128 33.9 -> 39.0 ms; the second set of accumulators costs 140 spills and the interleaved stream breaks the
  //  back-to-back MFMA issue.)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Yb = smem;                                         // [2][bf16 hi image, bf16 mid image]  (GEMM2's B operand, read transposed)
  char *Yf = Yb + 4 * IMG;                                 // [f16 hi image, f16 lo' image]       (forward's A operand; single buffer)
  char *Gi = Yf + 2 * IMG;                                 // [NBLK row blocks][hi 2 KiB, lo 2 KiB]  the G images (read by every wave)
  char *Xt = Gi + NBLK * 4096;                             // [NBLK row blocks][IMG]  X^T hi of the panel (GEMM3's B operand, hi term)
  float *Cmu = reinterpret_cast<float *>(Xt + NBLK * IMG);      // [2][BN]
  float *Cw = Cmu + 2 * BN;
  float *Csg = Cw + 2 * BN;
  int *Cmt = reinterpret_cast<int *>(Csg + 2 * BN);
  int *Ck = Cmt + 2 * BN;
  double *red = reinterpret_cast<double *>(Ck + 4);
  // (BATCH) the tile's dense batch table as two planes [16 slots][32 columns]: delta, and theta + mu_j (the column shift
  // folded in when the table is staged).  A lane's slot is fixed for a tile (its row's batch in the tile's view), so the
  // entries of four consecutive columns are ONE 16-B read per plane at an immediate offset, already in packed-math order.
  float *Btd = reinterpret_cast<float *>(smem + Cfg::lds_bytes), *Btt = Btd + BN * 16;
  unsigned char *Pm = reinterpret_cast<unsigned char *>(Btd + 2 * BN * 16);                              // (BATCH) slot -> batch map [n_bv][16]
  unsigned char *Bw0 = Pm + PMF_PM_BYTES + (threadIdx.x >> 6) * RB * a.n_bv * 32;                   // (BATCH) this wave: [RB][n_bv][32]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;

  // ---- per-lane LDS byte offsets (constant for the whole kernel)
  const uint32_t foff = (uint32_t)(512 * h + 16 * l31);   // forward fragments (f16 images, pmf_sb8_f_off): lane = row l31, chunk FS h + S at foff + 1024 S
  const int G4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  // The per-lane byte offsets of the transposed reads, kept to the registers that are really distinct (the register file is
  // full: what can be an instruction's immediate offset must be one).
  // GEMM2 B (Y bf16 image, transposed read): rows j = 16S + 8b + 4h + q, chunk = 4kb + 2(G4&1) + (p>>1):
  //   pmf_sb8_y_off(row, chunk) + 8(p&1) = 16 YRS S + ytr[b][kb]   (the swizzle of row 16S + 8b + 4h + q does not depend on S)
  int ytr[2][KB];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
      ytr[b][kb] = pmf_sb8_y_off<KB>(8 * b + 4 * h + tq, 4 * kb + 2 * (G4 & 1) + (tp >> 1)) + 8 * (tp & 1);
  // The K = 128 batch-layer variant has no room for the eight of them (they came back from scratch every tile, each reload a
  // wait for every load in flight): there ytr[b][kb] = ytr[b][0] ^ 64 kb ^ ... is rebuilt at each use from ytr[b][0] and the
  // lane's swizzle bits -- pmf_sb4_off puts kb into address bits 6..7 as kb ^ (row & 3), and row & 3 = tq.
  constexpr bool YTR_REBUILD = BATCH && KB == 4;
  const int tq64 = 64 * tq;
  auto ytr_of = [&](int b, int kb) __attribute__((always_inline)) -> int {
    if (!YTR_REBUILD) return ytr[b][kb];
    int x = tq64;
    asm volatile("" : "+v"(x));                    // (opaque: otherwise the eight values are hoisted back into registers)
    return (ytr[b][0] - tq64) + ((64 * kb) ^ x);   // ytr[b][0] = base + 64 (0 ^ tq)
  };
  // GEMM3 A (G image of a row block, 64-B rows, 8-B chunk cj of row i at cj ^ ((i >> 1) & 7)), read transposed:
  //   KB = 4 (32x32x16: lane = column j = l31, rows 16S + 8h .. + 7): rows i = 16S + 8h + 4b + q, cj = 4(G4&1) + p: 1024 S + ttr[b]
  //   KB = 2 (16x16x32: lane = column 16 jh + (lane & 15), rows 8 G4 .. + 7): rows i = 8 G4 + 4b + q, cj = 4 jh + p: ttr[b] ^ (32 jh)
  int ttr[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int i = (KB == 4 ? 8 * h : 8 * G4) + 4 * b + tq;
    ttr[b] = 64 * i + 8 * (((KB == 4 ? 4 * (G4 & 1) : 0) + tp) ^ ((i >> 1) & 7));
  }
  // GEMM3 B (X^T image of a row block): KB = 4: lane = factor 32 w + l31, rows 16 s + 8 h .. + 7 (two steps per block);
  //   KB = 2: lane = factor 16 w + (lane & 15), rows 8 G4 .. + 7 (one step per block: xtoff[0])
  // (unsigned: a uniform base + a zero-extended 32-bit lane offset is ONE address register; a signed offset makes hipcc
  //  build 64-bit per-lane pointers, 32 registers of them for the sixteen X^T fragments alone)
  const uint32_t xtoff[2] = {(uint32_t)(KB == 4 ? pmf_sb8_xt_off(32 * w + l31, h) : pmf_sb8_xt_off(16 * w + (lane & 15), G4)),
                             (uint32_t)pmf_sb8_xt_off(32 * w + l31, 2 + h)};
  const uint32_t tid16 = (uint32_t)tid * 16u, lane16 = (uint32_t)lane * 16u;
  const int gimg_w = 64 * l31 + 8 * (h ^ ((l31 >> 1) & 7));   // G image write of register group g: chunk (2g + h) ^ x = 2 (g ^ (x >> 1)) + (h ^ (x & 1))

  const int wg = pmf_xcd_wg(blockIdx.x, gridDim.x);
  const int64_t w_begin = a.wg_begin[wg];
  const int64_t w_end = a.wg_begin[wg + 1];
  float *myslab = a.gy_slabs + (int64_t)wg * a.slab_stride;
  const int64_t seg_block = a.n_rp * a.tps;
  // the forward accumulators carry sx sy: c1 undoes it for the hi hi sum, c2 = c1 2^-11 for the hi lo' + lo' hi sum
  const float c1 = 1.f / (a.sb_scale_x[0] * a.sb_scale_y[0]);
  const float c2 = c1 * (1.f / 2048.f);
  double lossacc = 0.0;
  int seg_cur = -1, pidx = 0, t0_first = 0;
  int gx_slot = a.piece_base[wg];
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  for (int64_t widx = w_begin; widx < w_end;) {
    int cs = (int)(widx / seg_block);
    if (cs > a.n_cseg - 1) cs = a.n_cseg - 1;
    const int tps_cs = cs == a.n_cseg - 1 ? a.n_ct - (a.n_cseg - 1) * a.tps : a.tps;
    const int64_t rem = widx - (int64_t)cs * seg_block;
    const int64_t rp = rem / tps_cs;
    const int ti0 = (int)(rem - rp * tps_cs);
    const int ntiles = (int)(tps_cs - ti0 < w_end - widx ? tps_cs - ti0 : w_end - widx);
    widx += ntiles;
    if (cs != seg_cur) { seg_cur = cs; pidx = 0; t0_first = ti0; } else { ++pidx; }
    bool slab_first = true;
    const int64_t col_begin = ((int64_t)a.ct0 + (int64_t)cs * a.tps + ti0) * BN;
    // this wave's RB row blocks: RB w .. RB w + RB - 1 of the panel's NBLK
    bool row_ok[RB], rows_in[RB];
    int rb_u[RB];
    int64_t row0[RB];
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      row0[b] = rp * BM + (int64_t)(RB * w + b) * 32;
      row_ok[b] = row0[b] + l31 < M;
      const int rb_raw = __builtin_amdgcn_readfirstlane((int)(row0[b] >> 5));
      rows_in[b] = rb_raw < a.nRB;
      rb_u[b] = rows_in[b] ? rb_raw : (int)a.nRB - 1;
    }

    // ---- this wave's X operands: forward fragments (f16 hi, lo') of its two row blocks and the mid term of GEMM3's transposed
    //      fragments for ITS k block over all eight row blocks, global images -> registers for the whole piece; the hi term of
    //      the transposed operand of all eight row blocks -> LDS (every wave reads its own k rows of it)
    f16x8 xh[RB][FS], xl[RB][FS];
    bf16x8 b3m[NI];   // (B3R: loaded here for the piece; otherwise per tile)
    // One scalar base for the panel's NBLK row blocks, unclamped: sb_split_x writes whole panels, so the absent blocks of a
    // ragged last panel hold zero images rewritten by every pass (their G is zero, and 0 x a stale NaN left in the buffer by
    // an earlier pass would not be; the buffer's sixteen blocks of padding hold the rounding up, prepare_fused_pass).  In
    // the per-tile variant the lane offset is made opaque before the block's stride is added, or hipcc hoists sixteen
    // 64-bit addresses out of the tile loop (32 registers).
    const char *xt_mid = a.Xsb + rp * (int64_t)NBLK * XBLK + 3 * IMG;
    auto b3m_load = [&](int g) __attribute__((always_inline)) {
      uint32_t o = xtoff[KB == 4 ? (g & 1) : 0];
      if (!B3R) asm volatile("" : "+v"(o));
      o += (uint32_t)(KB == 4 ? (g >> 1) : g) * (uint32_t)XBLK;
      b3m[g] = *reinterpret_cast<const bf16x8 *>(xt_mid + o);
    };
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      const char *xblk = a.Xsb + (int64_t)rb_u[b] * XBLK;
#pragma unroll
      for (int S = 0; S < FS; ++S) {
        xh[b][S] = *reinterpret_cast<const f16x8 *>(xblk + foff + 1024 * S);
        xl[b][S] = *reinterpret_cast<const f16x8 *>(xblk + IMG + foff + 1024 * S);
      }
    }
    if (B3R) {
#pragma unroll
      for (int g = 0; g < NI; ++g) b3m_load(g);
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {   // NBLK x IMG bytes = 4096 16-B chunks, 16 per thread, in two rounds of 8 registers
      u32x4 xv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        constexpr int CPI = IMG / 16;                             // chunks per image
        const int ch = tid + NT * (8 * half + q);                 // chunk of the [NBLK][IMG] LDS array
        const int64_t rbi = rp * NBLK + ch / CPI;
        const char *xb = a.Xsb + (rbi < a.nRB ? rbi : a.nRB - 1) * (int64_t)XBLK + 2 * IMG;
        xv[q] = reinterpret_cast<const u32x4 *>(xb)[ch % CPI];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) reinterpret_cast<u32x4 *>(Xt)[tid + NT * (8 * half + q)] = xv[q];
    }
    f32x16 gx[RB][KB];
#pragma unroll
    for (int b = 0; b < RB; ++b)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gx[b][kb][r] = 0.f;

    // Staging the next Y tile (4 images = 2048 16-B chunks, 8 per thread): chunks 0..3 the f16 pair, 4..7 the bf16 pair, each
    // half through four registers of its own (the bf16 pair goes to the free buffer as soon as it has arrived, the f16 pair
    // waits in registers for barrier B1: short live ranges, the register file is full)
    auto stage_load_y = [&](int64_t jt, int c, u32x4 (&yv)[NYC]) __attribute__((always_inline)) {   // c = 0 .. 2 NYC - 1
      const char *ybase = a.Ysb + (jt >> 5) * (int64_t)YBLK + 4096 * c;   // (uniform: a scalar base, the lane adds tid * 16)
      if (!(PMF_ABLATE & 64) || jt == col_begin) yv[c % NYC] = *reinterpret_cast<const u32x4 *>(ybase + tid16);
      else yv[c % NYC] = u32x4{0u, 0u, 0u, 0u};
    };
    auto stage_load_c = [&](int64_t jt, float4 &cv) __attribute__((always_inline)) {
      const float4 *cb = a.colp + jt;
      const int64_t remc = N - jt;
      const int ncol = remc > BN ? BN : (int)remc;
      cv = cb[tid < ncol ? tid : ncol - 1];
    };
    auto stage_store_f16 = [&](const u32x4 (&yv)[NYC]) __attribute__((always_inline)) {
#pragma unroll
      for (int c = 0; c < NYC; ++c) reinterpret_cast<u32x4 *>(Yf)[tid + NT * c] = yv[c];
    };
    auto stage_store_b16 = [&](int ybuf, const u32x4 (&yv)[NYC]) __attribute__((always_inline)) {
#pragma unroll
      for (int c = 0; c < NYC; ++c) reinterpret_cast<u32x4 *>(Yb + ybuf * 2 * IMG)[tid + NT * c] = yv[c];
    };
    auto stage_store_c = [&](int cbuf, int64_t jt, const float4 &cv) __attribute__((always_inline)) {
      const int64_t remc = N - jt;
      const int ncol = remc > BN ? BN : (int)remc;
      asm volatile("" ::"v"(cv.x), "v"(cv.y), "v"(cv.z), "v"(cv.w));
      if (tid < BN) {
        const bool livec = tid < ncol;
        Csg[cbuf * BN + tid] = livec ? cv.x : 0.f;
        Cmu[cbuf * BN + tid] = livec ? cv.y : 0.f;
        Cw[cbuf * BN + tid] = livec ? cv.z : 0.f;
        Cmt[cbuf * BN + tid] = livec ? __float_as_int(cv.w) : 3;
        if (MIXED) {
          const int kd = __float_as_int(cv.w) & 3;
          const unsigned m0 = (unsigned)__ballot(!livec || kd == 0), m1 = (unsigned)__ballot(!livec || kd == 1),
                         m2 = (unsigned)__ballot(!livec || kd == 2);
          if (tid == 0) Ck[cbuf] = m0 == 0xffffffffu ? 0 : (m1 == 0xffffffffu ? 1 : (m2 == 0xffffffffu ? 2 : 3));
        }
        if (BATCH) {   // the view of the tile's columns when they all share one (-1: in no view); -2: the tile straddles views
          const int vw = (__float_as_int(cv.w) >> 2) - 1;
          const int vw0 = __builtin_amdgcn_readfirstlane(vw);
          const unsigned mv = (unsigned)__ballot(!livec || vw == vw0);
          if (tid == 0) Ck[2 + cbuf] = mv == 0xffffffffu ? vw0 : -2;
        }
      }
    };
    // (BATCH) staging of the tile's batch table: thread tid takes entries (column tid & 31, slots tid >> 5 and 8 + (tid >> 5)) --
    // a wave's 64 lanes write 32 consecutive words of two slot rows (no bank conflict worth the name), at the price of one
    // 8-B gather per lane from 32 different lines of the L2-resident global table, issued a phase ahead of its use.
    auto bt_e = [&](int q) { return (tid & 31) * 16 + (tid >> 5) + 8 * q; };
    auto bt_mu = [&](int64_t jt, int e) -> float { const int64_t j = jt + (e >> 4); return j < N ? a.colp[j].y : 0.f; };
    auto bt_store = [&](int e, const float2 &dt, float mu) __attribute__((always_inline)) {
      const int o = (e & 15) * 32 + (e >> 4);
      Btd[o] = dt.x;
      Btt[o] = dt.y + mu;
    };
    // private-slab update: wave w owns factors 32 w .. 32 w + 31 of the tile's gY; lane (k = l31, h) holds, in accumulator
    // register r, column j = rowmap(r, h): element e = j Kp + 32 w + k.  One dword per lane and register: the 32 lanes of a
    // half-wave cover one 128-byte line of the slab.
    // The slab holds the UNSCALED sums (sigma_j is applied once by k_gy_reduce): the old values are requested a whole tile
    // ahead straight into the registers of GEMM3's accumulator, whose C input they are -- no second set of registers, no adds.
    // KB = 4: gy[r], r = 0..15: column j = rowmap(r, h), factor 32 w + l31: element [Kp (r & 3) + 8 Kp (r >> 2)] + slab_lane.
    // KB = 2: two 16x16 accumulators of four registers: register 4 jh + r: column j = 16 jh + 4 G4 + r, factor 16 w + (lane & 15):
    //         element [Kp (16 jh + r)] + slab_lane.
    // The uniform part goes into the scalar base / the immediate offset, one register holds the lane's part.  (No clamping of a
    // ragged last tile: the slab buffer is allocated one tile longer than N columns; columns >= N are loaded, accumulated and
    // never stored.)
    constexpr int NGY = KB == 4 ? 16 : 8;
    float gy[NGY];
    auto gy_col = [&](int r) __attribute__((always_inline)) { return KB == 4 ? pmf_rowmap(r, h) : 16 * (r >> 2) + 4 * G4 + (r & 3); };
    auto gy_elem = [&](int r) __attribute__((always_inline)) { return KB == 4 ? Kp * (r & 3) + 8 * Kp * (r >> 2) : Kp * (16 * (r >> 2) + (r & 3)); };
    const uint32_t slab_lane = 4u * (uint32_t)(KB == 4 ? 4 * h * Kp + 32 * w + l31 : 4 * G4 * Kp + 16 * w + (lane & 15));   // BYTES
    auto slab_prefetch = [&](int64_t jt) __attribute__((always_inline)) {
      const float *sb = myslab + jt * Kp;
#pragma unroll
      for (int r = 0; r < NGY; ++r)
        gy[r] = __builtin_nontemporal_load(reinterpret_cast<const float *>(reinterpret_cast<const char *>(sb + gy_elem(r)) + slab_lane));
    };

    // D tiles in registers: two sets, row block b uses set b & 1.  Block b + 1's tile is requested during GEMM2 of block b, the
    // next tile's block 0 during GEMM3 (RB is even: set 0 is free from GEMM2 of block RB - 2 on).
    PmfDTile<DB> dcur[2];
    uint32_t tflag[RB];
    auto d_load = [&](PmfDTile<DB> &d, int64_t tile, int q) __attribute__((always_inline)) {   // (PmfDTile::load with an unsigned lane offset)
      if (PMF_ABLATE & 128) return;
      if constexpr (DB) {
        const char *tb = reinterpret_cast<const char *>(a.D) + tile * 2048 + 1024 * q;
        const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(tb + lane16));
        d.w[4 * q + 0] = x.x; d.w[4 * q + 1] = x.y; d.w[4 * q + 2] = x.z; d.w[4 * q + 3] = x.w;
      } else {
        const char *tb = reinterpret_cast<const char *>(a.D) + tile * 4096 + 1024 * q;
        const pmf_f32x4 x = __builtin_nontemporal_load(reinterpret_cast<const pmf_f32x4 *>(tb + lane16));
        d.v[4 * q + 0] = x.x; d.v[4 * q + 1] = x.y; d.v[4 * q + 2] = x.z; d.v[4 * q + 3] = x.w;
      }
    };
    constexpr int NDL = PmfDTile<DB>::NCH;
    if (!(PMF_ABLATE & 1)) slab_prefetch(col_begin);
#pragma unroll
    for (int b = 0; b < RB; ++b) tflag[b] = a.tflags[(col_begin >> 5) * a.nRB + rb_u[b]];
#pragma unroll
    for (int q = 0; q < NDL; ++q) d_load(dcur[0], (col_begin >> 5) * a.nRB + rb_u[0], q);
    {
      u32x4 yf[NYC], yb[NYC];
      float4 cv;
#pragma unroll
      for (int c = 0; c < NYC; ++c) { stage_load_y(col_begin, c, yf); stage_load_y(col_begin, NYC + c, yb); }
      stage_load_c(col_begin, cv);
      stage_store_f16(yf);
      stage_store_b16(0, yb);
      stage_store_c(0, col_begin, cv);
      if (BATCH) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {   // 32 columns x 16 slots = 512 entries (first tile: slot map straight from global memory)
          const int e = bt_e(q);
          const float2 dt = pmf_bt_entry(a, a.pm + rp * a.n_bv * 16, col_begin, e, pmf_bt_view(a, col_begin, e));
          bt_store(e, dt, bt_mu(col_begin, e));
        }
        if (tid < a.n_bv * 16) Pm[tid] = a.pm[rp * a.n_bv * 16 + tid];
        if (h == 0) {   // panel-local slot of this wave's rows in every view (15 = identity: row in no batch)
#pragma unroll
          for (int b = 0; b < RB; ++b) {
            const int64_t irow_c = row_ok[b] ? row0[b] + l31 : M - 1;
            for (int v = 0; v < a.n_bv; ++v) Bw0[(b * a.n_bv + v) * 32 + l31] = a.row_slot[(int64_t)v * M + irow_c];
          }
        }
      }
    }
    __syncthreads();

    for (int t = 0; t < ntiles; ++t) {
      const int par = t & 1;
      const int64_t j0 = col_begin + (int64_t)t * BN;
      const char *Yc = Yb + par * 2 * IMG;
      const bool have_next = (t + 1 < ntiles);
      const int cb0 = par * BN + 4 * h;
      const int64_t jn = have_next ? j0 + BN : j0;
      float4 cnext;
      float2 btn[2];     // (BATCH) this thread's entries of the next tile's dense batch table
      float btm[2];      //         and their columns' mu
      int btv[2] = {255, 255};
      const int tkind = MIXED ? __builtin_amdgcn_readfirstlane(Ck[par]) : 0;
      const int tview = BATCH ? __builtin_amdgcn_readfirstlane(Ck[2 + par]) : -1;

      // The tile's global loads, each issued where its destination registers have just died and as far ahead of its use as
      // that allows, spread over the NG groups of a row block's GEMM2 (list position i, a few per group):
      //   GEMM2 of row block b < RB - 1 : D(t) of row block b + 1 (consumed by its epilogue); block 0 also takes the bf16 images
      //                                   of Y(t+1) (stored to the free buffer right after that GEMM2)
      //   GEMM2 of the last row block   : column parameters and batch table of tile t+1
      //   GEMM2 of row blocks >= 1      : (general variants) GEMM3's X^T mid fragments of this tile
      //   GEMM3                         : the f16 images of Y(t+1) (stored before barrier B2); D(t+1) of row block 0; the tile flags
      u32x4 yb16[NYC];
      // X^T mid loads per GEMM2 group (general variants).  PMF_B3LATE: all of them in the LAST row block's GEMM2, after the last
      // epilogue -- the fragments are then live during no epilogue at all (64 registers at the pass's register peak).
      constexpr int B3B = PMF_B3LATE ? 1 : RB - 1;                        // row blocks (the last B3B) whose GEMM2 carries the loads
      constexpr int B3P = B3R ? 0 : (NI + B3B * NG - 1) / (B3B * NG);
      auto vmem_op = [&](int b, int g, int z) __attribute__((always_inline)) {     // z-th slot of group g of row block b's GEMM2
        const int i = 2 * g + z;                                                    // (two list slots per group)
        if (z < 2) {
          if (b == 0 && i < NYC) stage_load_y(jn, NYC + i, yb16);
          else if (b < RB - 1 && i - (b == 0 ? NYC : 0) >= 0 && i - (b == 0 ? NYC : 0) < NDL)
            d_load(dcur[(b + 1) & 1], (j0 >> 5) * a.nRB + rb_u[b + 1], i - (b == 0 ? NYC : 0));
          else if (b == RB - 1 && i == 0) stage_load_c(jn, cnext);
          // (BATCH) the views of this thread's two columns of the next tile's table, a row block or more ahead of the gathers
          // that depend on them (requested in the group before the gathers, the view load's L2 latency stood in the middle
          // of GEMM2 every tile)
          else if (BATCH && !(PMF_ABLATE & 256) && b == 0 && i == NYC + NDL) { btv[0] = pmf_bt_view(a, jn, bt_e(0)); btv[1] = pmf_bt_view(a, jn, bt_e(1)); }
          else if ((PMF_ABLATE & 256) && b == RB - 1 && BATCH && (i == 1 || i == 2)) { btn[i - 1] = make_float2(1.f, 0.f); btm[i - 1] = 0.f; }
          else if (b == RB - 1 && BATCH && (i == 1 || i == 2)) {
            // (Issuing these gathers during GEMM3 and storing them before B2 instead -- so that the wait after B1 does not drain
            // every load in flight -- was measured: the longer live ranges cost the K <= 64 variant 90 scratch reloads per tile,
            // 14.6 -> 17.2 ms; no change at K = 128.)
            btn[i - 1] = pmf_bt_entry(a, Pm, jn, bt_e(i - 1), btv[i - 1]);
            btm[i - 1] = bt_mu(jn, bt_e(i - 1));
          }
        } else if (!B3R && b >= RB - B3B) {
          const int idx = ((b - (RB - B3B)) * NG + g) * B3P + (z - 2);
          if (idx < NI) b3m_load(idx);
        }
      };
      static_assert(NYC + NDL + 1 <= 2 * NG, "load schedule");

      // split G into bf16 hi / lo, write the row block's G image, GEMM2 (with the tile's global loads between its groups)
      auto grad_x_block = [&](int b, const f32x16 &G) __attribute__((always_inline)) {
        // ---- split G into bf16 hi / lo; registers 8S..8S+7 are GEMM2's A fragment of step S
        bf16x8 gh[2], gl[2];
#pragma unroll
        for (int S = 0; S < 2; ++S)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float g = G[8 * S + e];
            const __bf16 hi = (__bf16)g;
            gh[S][e] = hi;
            gl[S][e] = (__bf16)(g - (float)hi);
          }
        // this row block's [i][j] image of G for GEMM3: registers 4g..4g+3 = columns j = 8g + 4h .. +3 = 8-B chunk 2g + h of row i
        char *Tw = Gi + (RB * w + b) * 4096;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int o = gimg_w ^ (16 * g);   // = 64 l31 + 8 ((2g + h) ^ ((l31 >> 1) & 7)): bits 4..5 carry g ^ (x >> 1)
          const bf16x4 vh = {gh[g >> 1][4 * (g & 1)], gh[g >> 1][4 * (g & 1) + 1], gh[g >> 1][4 * (g & 1) + 2], gh[g >> 1][4 * (g & 1) + 3]};
          const bf16x4 vl = {gl[g >> 1][4 * (g & 1)], gl[g >> 1][4 * (g & 1) + 1], gl[g >> 1][4 * (g & 1) + 2], gl[g >> 1][4 * (g & 1) + 3]};
          if (!(PMF_ABLATE & 32)) {
            *reinterpret_cast<bf16x4 *>(Tw + o) = vh;
            *reinterpret_cast<bf16x4 *>(Tw + 2048 + o) = vl;
          } else {
            asm volatile("" ::"v"(vh), "v"(vl));
          }
        }

        // ---- GEMM2: gX[i,k] += sum_j G[j,i] Ys[k,j]   (A = G registers, B = the Y bf16 images read transposed)
        bf16x8 b2h[2], b2l[2];
        auto g2_read = [&](int g, int slot) __attribute__((always_inline)) {
          const int S = g / KB, kb = g % KB;
          const int y0 = ytr_of(0, kb), y1 = ytr_of(1, kb);
          b2h[slot] = pmf_sb_tr8(Yc + y0 + 16 * YRS * S, Yc + y1 + 16 * YRS * S);
          b2l[slot] = pmf_sb_tr8(Yc + y0 + 16 * YRS * S + IMG, Yc + y1 + 16 * YRS * S + IMG);
        };
        if (!(PMF_ABLATE & 4)) g2_read(0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int S = g / KB, kb = g % KB;
          if (g + 1 < NG && !(PMF_ABLATE & 4)) g2_read(g + 1, (g + 1) & 1);
#pragma unroll
          for (int z = 0; z < 2 + B3P; ++z) vmem_op(b, g, z);
          __builtin_amdgcn_sched_barrier(0);
          if (!(PMF_ABLATE & 4)) {
            PMF_SB8_GX(gx[b][kb], gl[S], b2h[g & 1]);
            PMF_SB8_GX(gx[b][kb], gh[S], b2l[g & 1]);
            PMF_SB8_GX(gx[b][kb], gh[S], b2h[g & 1]);
          } else {
            asm volatile("" ::"v"(gl[S]), "v"(gh[S]));
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      };

#pragma unroll
      for (int b = 0; b < RB; ++b) {
        // ---- forward of row block b: acc1 = sum yh xh ; acc2 = sum (yl' xh + yh xl')   (f16, scaled: see c1, c2)
        f32x16 acc1, acc2;
        if (PMF_ABLATE & 16) {
#pragma unroll
          for (int r = 0; r < 16; ++r) { acc1[r] = 1.f + (float)lane; acc2[r] = 0.5f; }
        } else {
          f16x8 yh = *reinterpret_cast<const f16x8 *>(Yf + foff);
          f16x8 yl = *reinterpret_cast<const f16x8 *>(Yf + IMG + foff);
#pragma unroll
          for (int S = 0; S < FS; ++S) {
            f16x8 yhn = yh, yln = yl;
            if (S + 1 < FS) {
              yhn = *reinterpret_cast<const f16x8 *>(Yf + foff + 1024 * (S + 1));
              yln = *reinterpret_cast<const f16x8 *>(Yf + IMG + foff + 1024 * (S + 1));
            }
            __builtin_amdgcn_sched_barrier(0);
            if (S == 0) PMF_SB8_FWD0(acc2, yl, xh[b][S]);
            else PMF_SB8_FWD(acc2, yl, xh[b][S]);
            PMF_SB8_FWD(acc2, yh, xl[b][S]);
            if (S == 0) PMF_SB8_FWD0(acc1, yh, xh[b][S]);
            else if (S + 1 < FS) PMF_SB8_FWD(acc1, yh, xh[b][S]);
            else PMF_SB8_FWD_LAST(acc1, yh, xh[b][S]);
            yh = yhn; yl = yln;
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        PmfDTile<DB> &dB = dcur[b & 1];
        // ---- epilogue: acc1 becomes G
        float lsum = 0.f;
        const float4 *cw4 = reinterpret_cast<const float4 *>(Cw + cb0);
        auto f4get = [](const float4 &v, int u) { return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w)); };
        const bool tile_fast = rows_in[b] && tflag[b] != 0;
        if (PMF_ABLATE & 8) {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc1[r] = fmaf(acc2[r], c2, acc1[r] * c1) - dB.get(r);
        } else if (!BATCH && tile_fast && (!MIXED || tkind == 0)) {
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) {
            const float4 w4 = cw4[2 * c4];
            const float4 mu4 = *reinterpret_cast<const float4 *>(Cmu + cb0 + 8 * c4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int r = 4 * c4 + u;
              const float z = fmaf(acc2[r], c2, fmaf(acc1[r], c1, f4get(mu4, u)));
              const float d = z - dB.get(r);
              const float g = f4get(w4, u) * d;
              lsum = fmaf(g, d, lsum);
              acc1[r] = g;
            }
          }
          lsum *= 0.5f;
        } else {
          // General path.  z' = z delta + (theta + mu_j) with the lane's entries of the batch planes (BATCH), or z + mu_j.
          // Views are column ranges, so the 32 columns of a tile nearly always share one view (uni): the lane's slot is ONE
          // byte for the tile and the planes are read 16 B at a time at immediate offsets; a tile that straddles two views
          // looks view and slot up per entry.  Each four-column group's reads are issued one group ahead.
          // Gaussian columns mask by substitution -- a missing entry takes y := z', hence d = 0, g = 0 and no loss -- and
          // sum g d (halved at the end): one select per entry instead of two, the loss in one fma.
          int bs = 15;
          if (BATCH && tview >= 0) bs = Bw0[(b * a.n_bv + tview) * 32 + l31];
          const float *bdl = Btd + bs * 32 + 4 * h, *btl = Btt + bs * 32 + 4 * h;
          float lnorm = 0.f;
          auto grp_load = [&](int c4, bool uni, float4 &dl4, float4 &th4, float4 &w4) __attribute__((always_inline)) {
            w4 = cw4[2 * c4];
            if (!BATCH) {
              th4 = *reinterpret_cast<const float4 *>(Cmu + cb0 + 8 * c4);
            } else if (uni) {
              dl4 = *reinterpret_cast<const float4 *>(bdl + 8 * c4);
              th4 = *reinterpret_cast<const float4 *>(btl + 8 * c4);
            } else {
              float dv[4], tv[4];
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                const int cl = 8 * c4 + 4 * h + u;
                const int v = (Cmt[par * BN + cl] >> 2) - 1;
                const int bsr = v < 0 ? 15 : Bw0[(b * a.n_bv + v) * 32 + l31];
                dv[u] = Btd[bsr * 32 + cl];
                tv[u] = Btt[bsr * 32 + cl];
              }
              dl4 = make_float4(dv[0], dv[1], dv[2], dv[3]);
              th4 = make_float4(tv[0], tv[1], tv[2], tv[3]);
            }
          };
          auto epi_reg = [&](int r, float dl, float th, float wj, int kmode, bool fast) __attribute__((always_inline)) {
            float z = fmaf(acc2[r], c2, acc1[r] * c1);
            z = BATCH ? fmaf(z, dl, th) : z + th;
            float y = dB.get(r);
            if (kmode == PMF_NOISE_NORMAL) {
              if (!fast) y = (pmf_finite(y) && row_ok[b]) ? y : z;
              const float d = z - y, g = wj * d;
              lnorm = fmaf(g, d, lnorm);
              acc1[r] = BATCH ? g * dl : g;
            } else {
              const bool ok = pmf_finite(y) && row_ok[b];
              float l, g;
              if (kmode == 3) pmf_noise<MIXED>(Cmt[cb0 + (r & 3) + 8 * (r >> 2)] & 3, z, y, wj, a.htab + (j0 + 4 * h) * PMF_HT + PMF_HT * ((r & 3) + 8 * (r >> 2)), l, g);
              else pmf_noise(kmode, z, y, wj, nullptr, l, g);
              lsum += ok ? l : 0.f;
              acc1[r] = ok ? (BATCH ? g * dl : g) : 0.f;
            }
          };
          auto epi_all = [&](int kmode, bool uni, bool fast) __attribute__((always_inline)) {
            float4 dl4 = make_float4(1.f, 1.f, 1.f, 1.f), th4, w4, dl4n = dl4, th4n, w4n;
            grp_load(0, uni, dl4n, th4n, w4n);
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
              dl4 = dl4n; th4 = th4n; w4 = w4n;
              if (c4 + 1 < 4) grp_load(c4 + 1, uni, dl4n, th4n, w4n);
              __builtin_amdgcn_sched_barrier(0);   // (the next group's reads stay HERE: one group in flight, not all four -- 80 registers)
#pragma unroll
              for (int u = 0; u < 4; ++u) epi_reg(4 * c4 + u, f4get(dl4, u), f4get(th4, u), f4get(w4, u), kmode, fast);
              __builtin_amdgcn_sched_barrier(0);
            }
          };
          if (BATCH && tview == -2) epi_all(3, false, false);
          // (the mask-free copy is for the batch variants: without batch layers an all-finite Gaussian tile took the packed path above;
          // in pmf_fused_sb_kernel a second branch on the freshly loaded tile flag cost the non-batch variant 11 %)
          else if (!MIXED || tkind == 0) { if (BATCH && tile_fast) epi_all(PMF_NOISE_NORMAL, true, true); else epi_all(PMF_NOISE_NORMAL, true, false); }
          else if (tkind == 1) epi_all(PMF_NOISE_BERNOULLI, true, false);
          else if (tkind == 2) epi_all(PMF_NOISE_POISSON, true, false);
          else epi_all(3, true, false);
          lsum = fmaf(0.5f, lnorm, lsum);
        }
        lossacc += (double)lsum;

        grad_x_block(b, acc1);
        if (b == 0) stage_store_b16(par ^ 1, yb16);   // (the other buffer: GEMM2 of tile t - 1 was its last reader, two barriers ago)
      }

      // ---- barrier B1: all G images are written (GEMM3 reads them all) and every wave is past its forwards and epilogues of
      //      tile t (the single f16 buffer, the column parameters' other buffer and the batch table can take tile t + 1)
      __syncthreads();
      stage_store_c(par ^ 1, jn, cnext);
      if (BATCH) {
#pragma unroll
        for (int q = 0; q < 2; ++q) bt_store(bt_e(q), btn[q], btm[q]);
      }

      // ---- GEMM3, cross-wave: this wave computes the tile's gY for ITS factors over all rows of the panel,
      //      gY[j, k] (+)= sum_rb sum_i G_rb[i, j] X_rb[k, i]   (A = the G images read transposed, M = j; B = X^T fragments, N = k:
      //      hi term from LDS, mid term from registers; C = the old slab values, already in the accumulator)
      {
        u32x4 yf16[NYC];
        slab_first = pidx == 0 || (pidx == 1 && ti0 + t < t0_first);
        if (slab_first || (PMF_ABLATE & 1)) {
#pragma unroll
          for (int r = 0; r < NGY; ++r) gy[r] = 0.f;
        }
        auto vmem_op3 = [&](int i) __attribute__((always_inline)) {
          if (i < NYC) stage_load_y(jn, i, yf16);
          else if (i < NYC + NDL) d_load(dcur[0], (jn >> 5) * a.nRB + rb_u[0], i - NYC);
          else if (i < NYC + NDL + RB) tflag[i - NYC - NDL] = a.tflags[(jn >> 5) * a.nRB + rb_u[i - NYC - NDL]];
        };
        static_assert(NYC + NDL + RB <= NI, "load schedule");
        if constexpr (KB == 4) {
          f32x16 acc;
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = gy[r];
          bf16x8 a3h[2], a3l[2], b3h[2];
          auto g3_read = [&](int g) __attribute__((always_inline)) {
            const char *Tr = Gi + (g >> 1) * 4096;
            const int S = g & 1;
            a3h[g & 1] = pmf_sb_tr8(Tr + ttr[0] + 1024 * S, Tr + ttr[1] + 1024 * S);
            a3l[g & 1] = pmf_sb_tr8(Tr + ttr[0] + 1024 * S + 2048, Tr + ttr[1] + 1024 * S + 2048);
            b3h[g & 1] = *reinterpret_cast<const bf16x8 *>(Xt + (g >> 1) * IMG + xtoff[S]);
          };
          if (!(PMF_ABLATE & 2)) g3_read(0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int g = 0; g < NI; ++g) {
            if (g + 1 < NI && !(PMF_ABLATE & 2)) g3_read(g + 1);
            vmem_op3(g);
            __builtin_amdgcn_sched_barrier(0);
            if (!(PMF_ABLATE & 2)) {
              PMF_SB8_GY(acc, a3l[g & 1], b3h[g & 1]);
              PMF_SB8_GY(acc, a3h[g & 1], b3m[g]);
              if (g + 1 < NI) PMF_SB8_GY(acc, a3h[g & 1], b3h[g & 1]);
              else PMF_SB8_GY_LAST(acc, a3h[g & 1], b3h[g & 1]);
            } else {
              asm volatile("" ::"v"(b3m[g]));
            }
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) gy[r] = acc[r];
        } else {
          // one step = one row block (32 rows = the K of v_mfma_f32_16x16x32_bf16); two accumulators: columns 0..15 and 16..31
          pmf_acc4 acc[2];
#pragma unroll
          for (int jh = 0; jh < 2; ++jh)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[jh][r] = gy[4 * jh + r];
          bf16x8 a3h[2][2], a3l[2][2], b3h[2];   // [buffer][column half]
          auto g3_read = [&](int g) __attribute__((always_inline)) {
            const char *Tr = Gi + g * 4096;
#pragma unroll
            for (int jh = 0; jh < 2; ++jh) {
              a3h[g & 1][jh] = pmf_sb_tr8(Tr + (ttr[0] ^ (32 * jh)), Tr + (ttr[1] ^ (32 * jh)));
              a3l[g & 1][jh] = pmf_sb_tr8(Tr + (ttr[0] ^ (32 * jh)) + 2048, Tr + (ttr[1] ^ (32 * jh)) + 2048);
            }
            b3h[g & 1] = *reinterpret_cast<const bf16x8 *>(Xt + g * IMG + xtoff[0]);
          };
          if (!(PMF_ABLATE & 2)) g3_read(0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int g = 0; g < NI; ++g) {
            if (g + 1 < NI && !(PMF_ABLATE & 2)) g3_read(g + 1);
            vmem_op3(g);
            __builtin_amdgcn_sched_barrier(0);
            if (PMF_ABLATE & 2) asm volatile("" ::"v"(b3m[g]));
#pragma unroll
            for (int jh = 0; jh < 2 && !(PMF_ABLATE & 2); ++jh) {
              PMF_SB8_GY16(acc[jh], a3l[g & 1][jh], b3h[g & 1]);
              PMF_SB8_GY16(acc[jh], a3h[g & 1][jh], b3m[g]);
              if (g + 1 < NI) PMF_SB8_GY16(acc[jh], a3h[g & 1][jh], b3h[g & 1]);
              else PMF_SB8_GY16_LAST(acc[jh], a3h[g & 1][jh], b3h[g & 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
#pragma unroll
          for (int jh = 0; jh < 2; ++jh)
#pragma unroll
            for (int r = 0; r < 4; ++r) gy[4 * jh + r] = acc[jh][r];
        }
        dcur[0].touch();   // the D loads issued above count as consumed before the stores below are issued
        const int64_t remc = N - j0;
        const int ncol = remc > BN ? BN : (int)remc;
        float *sb = myslab + j0 * Kp;
        if (!(PMF_ABLATE & 1)) {
          if (ncol == BN) {   // (uniform) every tile but a ragged last one
#pragma unroll
            for (int r = 0; r < NGY; ++r)
              __builtin_nontemporal_store(gy[r], reinterpret_cast<float *>(reinterpret_cast<char *>(sb + gy_elem(r)) + slab_lane));
          } else {
#pragma unroll
            for (int r = 0; r < NGY; ++r)
              if (gy_col(r) < ncol)
                __builtin_nontemporal_store(gy[r], reinterpret_cast<float *>(reinterpret_cast<char *>(sb + gy_elem(r)) + slab_lane));
          }
        } else {
#pragma unroll
          for (int r = 0; r < NGY; ++r) asm volatile("" ::"v"(gy[r]));
        }
        // the next tile's old values into the same registers (they are dead now): a whole tile of latency to hide behind
        if (!(PMF_ABLATE & 1)) slab_prefetch(jn);
        // ---- the f16 images of tile t + 1 (every wave is past its forwards since B1); barrier B2: tile t + 1 is complete in LDS
        //      and every wave has read the G images of tile t
        stage_store_f16(yf16);
      }
      __syncthreads();
    }

    // ---- flush gX (lane = factor index k, register = row): plain stores to the piece's own slot (see pmf_fused_kernel)
#pragma unroll
    for (int b = 0; b < RB; ++b) {
      float *gp = a.gx_part + (int64_t)gx_slot * a.gx_slot_stride + (int64_t)(RB * w + b) * 32 * Kp + l31;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gp[pmf_rowmap(r, h) * Kp + 32 * kb] = gx[b][kb][r];
    }
    ++gx_slot;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossacc += __shfl_xor(lossacc, off, 64);
  if (lane == 0) red[w] = lossacc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int q = 0; q < NW; ++q) s += red[q];
    a.loss_partial[wg] = s;
  }
}
