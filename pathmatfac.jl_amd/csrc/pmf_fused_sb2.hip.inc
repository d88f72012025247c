// pmf_fused_sb2.hip.inc -- the split-bf16 data pass for 32 < K <= 64 as FOUR waves with TWO 32-row blocks each
// (included by pmf_k_sb2.hip).  Same arithmetic, operand images (SbCfg<2>, k_sb_split<2>), work split, private gY slabs,
// gX slots and outputs as pmf_fused_sb_kernel<2>; same 256-row panel.  What changes is who does the work:
//
//   pmf_fused_sb_kernel : 8 waves x 1 row block, two waves per SIMD (256 registers each).  Measured (DESIGN 4.5): the
//     older wave of each SIMD wins the matrix-pipe arbitration and waits 16-18 % of its time at barrier B1 for the
//     younger one; every wave reads the whole Y tile and its own X panel from LDS for every product; eight slabs per
//     tile go through LDS.
//   this kernel : 4 waves, one per SIMD, 512 registers each.  A wave owns rows 64 w .. 64 w + 63 of the panel.
//     * no second wave on the SIMD: no arbitration, the four waves reach the barriers together;
//     * the forward's X fragments (hi, mid, lo of both row blocks: 24 x 16 B per lane) live in registers for the whole
//       piece, loaded straight from the global operand images;
//     * each Y fragment read from LDS (forward rows, GEMM2 transposed) feeds BOTH row blocks: half the LDS reads per row;
//     * GEMM3 contracts over the wave's 64 rows: four slabs per tile instead of eight (half the slab writes, half the
//       cross-wave reads), and half as many private-slab threads;
//   LDS: Y tile (hi + mid double buffered, lo single) 20 KiB, X hi + mid images of the eight row blocks 64 KiB (GEMM3's
//   transposed B operand), four slabs 32 KiB (the first G image of a wave aliases the last k block of its slab), the
//   second G images 16 KiB, column parameters: 133 KiB.
#ifndef PMF_ABLATE
#define PMF_ABLATE 0   // measurement-only builds: 64 no epilogue math, 128 cheap G split (hi only), 256 no G image writes, 512 G image writes twice
#endif
template <bool MIXED, bool GX, bool GY, bool BATCH, bool DB>
__global__ __launch_bounds__(256, 1) void pmf_fused_sb2_kernel(const FusedArgs a) {
  constexpr int KB = 2, NW = 4, RBW = 2, NT = 256, Kp = 64, BN = PMF_BN, BM = 32 * NW * RBW, SLAB = 32 * Kp;
  using Cfg = SbCfg<2>;
  constexpr int IMG = Cfg::IMG, BLK = Cfg::BLK, LDSP = 2 * IMG;
  constexpr int FS = 2 * KB;        // k-steps of the forward (16 factors each)
  constexpr int NG = 2 * KB;        // (16-row / 16-column step, k block) groups of GEMM2 / GEMM3
  constexpr int RV4 = 2;            // float4 of the [64 x 32] gY tile per thread (512 / 256)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Yi = smem;                                         // [2][hi image, mid image]
  char *Yl = Yi + 2 * LDSP;                                // lo image (single buffer)
  char *Xi = Yl + IMG;                                     // [NW * RBW][hi, mid]
  float *Sl = reinterpret_cast<float *>(Xi + NW * RBW * LDSP);   // [NW][SLAB]
  char *T1 = reinterpret_cast<char *>(Sl + NW * SLAB);     // [NW][4 KiB] G image of the waves' second row block
  float *Cmu = reinterpret_cast<float *>(T1 + NW * 4096);  // [2][BN]
  float *Cw = Cmu + 2 * BN;
  float *Csg = Cw + 2 * BN;
  int *Cmt = reinterpret_cast<int *>(Csg + 2 * BN);
  int *Ck = Cmt + 2 * BN;
  double *red = reinterpret_cast<double *>(Ck + 4);
  float2 *Bt = reinterpret_cast<float2 *>(smem + Sb2Cfg::lds_bytes);                            // (BATCH) [BN][16]
  unsigned char *Pm = reinterpret_cast<unsigned char *>(Bt + BN * 16);                             // (BATCH) the piece's slot -> batch map [n_bv][16]
  unsigned char *Bw0 = Pm + PMF_PM_BYTES + (threadIdx.x >> 6) * RBW * a.n_bv * 32;                 // (BATCH) this wave: [RBW][n_bv][32] slot of every row

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  float *Sw = Sl + w * SLAB;
  char *Tw[RBW] = {reinterpret_cast<char *>(Sw + (KB - 1) * 1024), T1 + w * 4096};
  char *Xw[RBW] = {Xi + (w * RBW) * LDSP, Xi + (w * RBW + 1) * LDSP};

  int rowoff[FS];   // row reads (forward): lane = row l31, chunk FS h + S
#pragma unroll
  for (int S = 0; S < FS; ++S) rowoff[S] = pmf_sb_off<KB>(l31, FS * h + S);
  const int G4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  auto y_tr_off = [&](int S, int b, int kb) {   // GEMM2 B (Y image): rows j = 16S + 8b + 4h + q; chunk = 4kb + 2(G4&1) + (p>>1)
    return pmf_sb_off<KB>(16 * S + 8 * b + 4 * h + tq, 4 * kb + 2 * (G4 & 1) + (tp >> 1)) + 8 * (tp & 1);
  };
  auto x_tr_off = [&](int S, int b, int kb) {   // GEMM3 B (X image): rows i = 16S + 8h + 4b + q
    return pmf_sb_off<KB>(16 * S + 8 * h + 4 * b + tq, 4 * kb + 2 * (G4 & 1) + (tp >> 1)) + 8 * (tp & 1);
  };
  auto t_tr_off = [&](int S, int b) {           // GEMM3 A (G image, 64-B rows, 8-B chunk cj = 4(G4&1) + p, XOR (i>>1)&7)
    const int i = 16 * S + 8 * h + 4 * b + tq;
    return 64 * i + 8 * ((4 * (G4 & 1) + tp) ^ ((i >> 1) & 7));
  };

#ifdef PMF_STAMPS   // slots: 0 loop top, 1 epilogue math, 2 G split + image writes, 3 GEMM2 (+ load issue), 4 GEMM3, 9 slab writes,
                    // 5 stage_store, 6 B1 wait, 8 forward + slab reduce, 7 private-slab stores, 10 B2 wait, 11 piece prologue / flush
  unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long st_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long st_t0 = st_prev, st_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  const int wg = pmf_xcd_wg(blockIdx.x, gridDim.x);
  const int64_t w_begin = a.wg_begin[wg];
  const int64_t w_end = a.wg_begin[wg + 1];
  float *myslab = a.gy_slabs + (int64_t)wg * a.slab_stride;
  const int64_t seg_block = a.n_rp * a.tps;
  double lossacc = 0.0;
  int seg_cur = -1, pidx = 0, t0_first = 0;
  int gx_slot = GX ? a.piece_base[wg] : 0;
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
    int64_t row0[RBW];
    bool row_ok[RBW], rows_in[RBW];
    int rb_u[RBW];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) {
      row0[rb] = rp * BM + (int64_t)(w * RBW + rb) * 32;
      row_ok[rb] = row0[rb] + l31 < M;
      const int rb_raw = __builtin_amdgcn_readfirstlane((int)(row0[rb] >> 5));
      rows_in[rb] = rb_raw < a.nRB;
      rb_u[rb] = rows_in[rb] ? rb_raw : (int)a.nRB - 1;
    }

    // ---- this wave's X operands: forward fragments global -> registers (for the whole piece); hi + mid images -> LDS
    bf16x8 xh[RBW][FS], xm[RBW][FS], xl[RBW][FS];
    u32x4 xv0[RBW][8];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) {
      const char *xblk = a.Xsb + (int64_t)rb_u[rb] * BLK;
#pragma unroll
      for (int q = 0; q < 8; ++q) xv0[rb][q] = (reinterpret_cast<const u32x4 *>(xblk))[lane + 64 * q];   // hi + mid: 512 chunks
#pragma unroll
      for (int S = 0; S < FS; ++S) {
        xh[rb][S] = *reinterpret_cast<const bf16x8 *>(xblk + rowoff[S]);
        xm[rb][S] = *reinterpret_cast<const bf16x8 *>(xblk + IMG + rowoff[S]);
        xl[rb][S] = *reinterpret_cast<const bf16x8 *>(xblk + 2 * IMG + rowoff[S]);
      }
    }
    f32x16 gx[RBW][KB];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gx[rb][kb][r] = 0.f;

    // Staging the next Y tile: hi + mid images = 512 16-B chunks (2 per thread), lo = 256 (1 per thread).
    auto stage_load_y = [&](int64_t jt, int c, u32x4 (&yv)[3]) __attribute__((always_inline)) {
      yv[c] = (reinterpret_cast<const u32x4 *>(a.Ysb + (jt >> 5) * (int64_t)BLK))[tid + NT * c];   // c = 0, 1: hi, mid; 2: lo
    };
    auto stage_load_c = [&](int64_t jt, float4 &cv) __attribute__((always_inline)) {
      const float4 *cb = a.colp + jt;
      const int64_t rem = N - jt;
      const int ncol = rem > BN ? BN : (int)rem;
      cv = cb[tid < ncol ? tid : ncol - 1];
    };
    auto stage_store = [&](int ybuf, int cbuf, int64_t jt, const u32x4 (&yv)[3], const float4 &cv) __attribute__((always_inline)) {
#pragma unroll
      for (int c = 0; c < 2; ++c) reinterpret_cast<u32x4 *>(Yi + ybuf * LDSP)[tid + NT * c] = yv[c];
      reinterpret_cast<u32x4 *>(Yl)[tid] = yv[2];
      const int64_t rem = N - jt;
      const int ncol = rem > BN ? BN : (int)rem;
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
      }
    };
    // slab reduction mapping: thread -> float4 f = tid + 256 q of the [kb][j][32 k] slab (kb = q);
    // element e = j*Kp + 32 kb + k of the [j][Kp] gY tile
    float4 gold[RV4];
    PmfDTile<DB> dcur[RBW];
    const int s_j = tid >> 3, s_k4 = (tid & 7) * 4;
    auto slab_prefetch_one = [&](int64_t jt, int q) __attribute__((always_inline)) {
      const float *sb = myslab + jt * Kp;
      const int64_t rem = N - jt;
      const int nel = (rem > BN ? BN : (int)rem) * Kp;
      const int e = s_j * Kp + 32 * q + s_k4;
      gold[q] = pmf_load_stream(reinterpret_cast<const float4 *>(sb + (e < nel ? e : (e % Kp))));
    };
    // forward of one tile for both row blocks (12 MFMAs per k-step: every Y fragment is read once and used twice) with
    // the reduction of the previous tile's four slabs between them
    auto forward_reduce = [&](f32x16 (&acc)[RBW], int ybuf, int cbuf, bool do_red, int64_t jt_red) __attribute__((always_inline)) {
      const int cb0 = cbuf * BN + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float m0 = BATCH ? 0.f : Cmu[cb0 + (r & 3) + 8 * (r >> 2)];   // (mu joins after the batch scale)
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) acc[rb][r] = m0;
      }
      const char *Yc = Yi + ybuf * LDSP;
      float4 racc[RV4];
#pragma unroll
      for (int q = 0; q < RV4; ++q) racc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      bf16x8 yh = *reinterpret_cast<const bf16x8 *>(Yc + rowoff[0]);
      bf16x8 ym = *reinterpret_cast<const bf16x8 *>(Yc + IMG + rowoff[0]);
      bf16x8 yl = *reinterpret_cast<const bf16x8 *>(Yl + rowoff[0]);
      // One wave per SIMD: whatever sits BETWEEN two MFMAs issues while the first one runs (about four VALU or one LDS read
      // per MFMA are free, scripts/mfma_bf16_valu.hip); whatever sits between two GROUPS of MFMAs is exposed.  The next
      // step's operand reads, the slab reads and their adds are therefore placed one at a time behind the step's MFMAs.
#define PMF_F() __builtin_amdgcn_sched_barrier(0)
#pragma unroll
      for (int S = 0; S < FS; ++S) {
        bf16x8 yhn = yh, ymn = ym, yln = yl;
        float4 sv[2];   // 2 float4 x 4 slabs per thread over 4 k-steps: two per step
        const bool nx = S + 1 < FS;
        PMF_F();
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yl, xh[0][S], acc[0], 0, 0, 0); PMF_F();
        if (nx) yhn = *reinterpret_cast<const bf16x8 *>(Yc + rowoff[S + 1]);
        PMF_F();
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yl, xh[1][S], acc[1], 0, 0, 0); PMF_F();
        if (nx) ymn = *reinterpret_cast<const bf16x8 *>(Yc + IMG + rowoff[S + 1]);
        PMF_F();
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xl[0][S], acc[0], 0, 0, 0); PMF_F();
        if (nx) yln = *reinterpret_cast<const bf16x8 *>(Yl + rowoff[S + 1]);
        PMF_F();
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xl[1][S], acc[1], 0, 0, 0); PMF_F();
        if (do_red) { const int idx = 2 * S, q = idx >> 2, sl = idx & 3; sv[0] = *reinterpret_cast<const float4 *>(Sl + sl * SLAB + 4 * (tid + NT * q)); }
        PMF_F();
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xm[0][S], acc[0], 0, 0, 0); PMF_F();
        if (do_red) { const int idx = 2 * S + 1, q = idx >> 2, sl = idx & 3; sv[1] = *reinterpret_cast<const float4 *>(Sl + sl * SLAB + 4 * (tid + NT * q)); }
        PMF_F();
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xm[1][S], acc[1], 0, 0, 0); PMF_F();
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xh[0][S], acc[0], 0, 0, 0); PMF_F();
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xh[1][S], acc[1], 0, 0, 0); PMF_F();
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xm[0][S], acc[0], 0, 0, 0); PMF_F();
        if (do_red) { float4 &ra = racc[(2 * S) >> 2]; ra.x += sv[0].x; ra.y += sv[0].y; ra.z += sv[0].z; ra.w += sv[0].w; }
        PMF_F();
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xm[1][S], acc[1], 0, 0, 0); PMF_F();
        if (do_red) { float4 &ra = racc[(2 * S + 1) >> 2]; ra.x += sv[1].x; ra.y += sv[1].y; ra.z += sv[1].z; ra.w += sv[1].w; }
        PMF_F();
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xh[0][S], acc[0], 0, 0, 0); PMF_F();
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xh[1][S], acc[1], 0, 0, 0); PMF_F();
        yh = yhn; ym = ymn; yl = yln;
      }
      PMF_STAMP(8);
      if (do_red) {
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb) dcur[rb].touch();
        const int64_t rem = N - jt_red;
        const int nel = (rem > BN ? BN : (int)rem) * Kp;
        float *sb = myslab + jt_red * Kp;
        const float sgj = Csg[(cbuf ^ 1) * BN + s_j];   // ColScale pull-back: gY[:, j] *= sigma_j
#pragma unroll
        for (int q = 0; q < RV4; ++q) {
          float4 v = racc[q];
          v.x *= sgj; v.y *= sgj; v.z *= sgj; v.w *= sgj;
          if (!slab_first) { v.x += gold[q].x; v.y += gold[q].y; v.z += gold[q].z; v.w += gold[q].w; }
          const int e = s_j * Kp + 32 * q + s_k4;
          if (e < nel) pmf_store_stream(reinterpret_cast<float4 *>(sb + e), v);
        }
      }
    };

    uint32_t tflag[RBW];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb) {
      tflag[rb] = a.tflags[(col_begin >> 5) * a.nRB + rb_u[rb]];
#pragma unroll
      for (int q = 0; q < PmfDTile<DB>::NCH; ++q) dcur[rb].load(a.D, (col_begin >> 5) * a.nRB + rb_u[rb], lane, q);
    }
    {
      u32x4 yv[3];
      float4 cv;
#pragma unroll
      for (int c = 0; c < 3; ++c) stage_load_y(col_begin, c, yv);
      stage_load_c(col_begin, cv);
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
        for (int q = 0; q < 8; ++q) reinterpret_cast<u32x4 *>(Xw[rb])[lane + 64 * q] = xv0[rb][q];
      stage_store(0, 0, col_begin, yv, cv);
      if (BATCH) {
#pragma unroll
        for (int q = 0; q < 2; ++q)   // 32 columns x 16 slots = 512 float2 (first tile: slot map straight from global memory)
          Bt[tid + NT * q] = pmf_bt_entry(a, a.pm + rp * a.n_bv * 16, col_begin, tid + NT * q, pmf_bt_view(a, col_begin, tid + NT * q));
        if (tid < a.n_bv * 16) Pm[tid] = a.pm[rp * a.n_bv * 16 + tid];
        if (h == 0) {   // panel-local slot of this wave's rows in every view (15 = identity: row in no batch)
#pragma unroll
          for (int rb = 0; rb < RBW; ++rb) {
            const int64_t irow_c = row_ok[rb] ? row0[rb] + l31 : M - 1;
            for (int v = 0; v < a.n_bv; ++v) Bw0[(rb * a.n_bv + v) * 32 + l31] = a.row_slot[(int64_t)v * M + irow_c];
          }
        }
      }
    }
    __syncthreads();

    // GEMM3's B fragments (the wave's own X images read transposed) do not change during the piece: registers
    bf16x8 b3h[RBW][NG], b3l[RBW][NG];
#pragma unroll
    for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int S = g / KB, kb = g % KB;
        b3h[rb][g] = pmf_sb_tr8(Xw[rb] + x_tr_off(S, 0, kb), Xw[rb] + x_tr_off(S, 1, kb));
        b3l[rb][g] = pmf_sb_tr8(Xw[rb] + IMG + x_tr_off(S, 0, kb), Xw[rb] + IMG + x_tr_off(S, 1, kb));
      }

    f32x16 acc[RBW];
    forward_reduce(acc, 0, 0, false, 0);
    PMF_STAMP(11);

    for (int t = 0; t < ntiles; ++t) {
      PMF_STAMP(0);
      const int par = t & 1;
      const int64_t j0 = col_begin + (int64_t)t * BN;
      const char *Yc = Yi + par * LDSP;
      const bool have_next = (t + 1 < ntiles);
      const int cb0 = par * BN + 4 * h;
      u32x4 ynext[3];
      float4 cnext;
      float2 btn[2];     // (BATCH) this thread's entries of the next tile's dense batch table
      int btv[2] = {255, 255};
      const int64_t jn = have_next ? j0 + BN : j0;

      // ---- epilogue (as pmf_fused_sb_kernel), once per row block: acc becomes G
      float lsum = 0.f;
      const int tkind = MIXED ? __builtin_amdgcn_readfirstlane(Ck[par]) : 0;
      const float4 *cw4 = reinterpret_cast<const float4 *>(Cw + cb0);
      auto f4get = [](const float4 &v, int u) { return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w)); };
      typedef float f32x2 __attribute__((ext_vector_type(2)));
      bf16x8 gh[RBW][2], gl[RBW][2];
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb) {
        auto epi_reg = [&](int r, float wj, int kmode) __attribute__((always_inline)) {
          const int ci = cb0 + (r & 3) + 8 * (r >> 2);
          const float y = dcur[rb].get(r);
          const bool ok = pmf_finite(y) && row_ok[rb];
          float z = acc[rb][r], dl = 1.f;
          if (BATCH) {
            const int v = (Cmt[ci] >> 2) - 1;
            const int b = Bw0[(rb * a.n_bv + (v < 0 ? 0 : v)) * 32 + l31];
            const float2 dt = Bt[pmf_rowmap(r, h) * 16 + (v < 0 ? 15 : b)];
            dl = dt.x;
            z = fmaf(z, dl, Cmu[ci] + dt.y);
          }
          float l, g;
          if (kmode == 3) pmf_noise<MIXED>(Cmt[ci] & 3, z, y, wj, a.htab + (j0 + 4 * h) * PMF_HT + PMF_HT * ((r & 3) + 8 * (r >> 2)), l, g);
          else pmf_noise(kmode, z, y, wj, nullptr, l, g);
          lsum += ok ? l : 0.f;
          acc[rb][r] = ok ? (BATCH ? g * dl : g) : 0.f;
        };
        const bool tile_fast = rows_in[rb] && tflag[rb] != 0;
        if (PMF_ABLATE & 64) {
          lsum += acc[rb][0];
        } else if (!BATCH && tile_fast && (!MIXED || tkind == 0)) {
          f32x2 ls2 = {0.f, 0.f};
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) {
            const float4 w4 = cw4[2 * c4];
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2) {
              const int r = 4 * c4 + 2 * p2;
              const f32x2 zz = {acc[rb][r], acc[rb][r + 1]}, yy = {dcur[rb].get(r), dcur[rb].get(r + 1)};
              const f32x2 ww = p2 == 0 ? f32x2{w4.x, w4.y} : f32x2{w4.z, w4.w};
              const f32x2 dd = zz - yy;
              const f32x2 gg = ww * dd;
              ls2 = gg * dd + ls2;
              acc[rb][r] = gg.x; acc[rb][r + 1] = gg.y;
            }
          }
          lsum += 0.5f * (ls2.x + ls2.y);
        } else {
          auto epi_all = [&](int kmode) __attribute__((always_inline)) {
#pragma unroll
            for (int c4 = 0; c4 < 4; ++c4) {
              const float4 w4 = cw4[2 * c4];
#pragma unroll
              for (int u = 0; u < 4; ++u) epi_reg(4 * c4 + u, f4get(w4, u), kmode);
            }
          };
          if (!MIXED || tkind == 0) epi_all(PMF_NOISE_NORMAL);
          else if (tkind == 1) epi_all(PMF_NOISE_BERNOULLI);
          else if (tkind == 2) epi_all(PMF_NOISE_POISSON);
          else epi_all(3);
        }
        PMF_STAMP(1);
        // split G into bf16 hi / lo; registers 8S..8S+7 are GEMM2's A fragment of step S; the [i][j] image for GEMM3
#pragma unroll
        for (int S = 0; S < 2; ++S)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float g = acc[rb][8 * S + e];
            const __bf16 hi = (__bf16)g;
            gh[rb][S][e] = hi;
            gl[rb][S][e] = (PMF_ABLATE & 128) ? hi : (__bf16)(g - (float)hi);
          }
#pragma unroll
        for (int g = 0; GY && g < 4 && !(PMF_ABLATE & 256); ++g) {
          const int o = 64 * l31 + 8 * ((2 * g + h) ^ ((l31 >> 1) & 7));
          const bf16x4 vh = {gh[rb][g >> 1][4 * (g & 1)], gh[rb][g >> 1][4 * (g & 1) + 1], gh[rb][g >> 1][4 * (g & 1) + 2], gh[rb][g >> 1][4 * (g & 1) + 3]};
          const bf16x4 vl = {gl[rb][g >> 1][4 * (g & 1)], gl[rb][g >> 1][4 * (g & 1) + 1], gl[rb][g >> 1][4 * (g & 1) + 2], gl[rb][g >> 1][4 * (g & 1) + 3]};
          *reinterpret_cast<bf16x4 *>(Tw[rb] + o) = vh;
          *reinterpret_cast<bf16x4 *>(Tw[rb] + 2048 + o) = vl;
          if (PMF_ABLATE & 512) {   // (measurement only: the image writes a second time, to price them)
            asm volatile("" ::: "memory");
            *reinterpret_cast<volatile bf16x4 *>(Tw[rb] + o) = vh;
            *reinterpret_cast<volatile bf16x4 *>(Tw[rb] + 2048 + o) = vl;
          }
        }
        PMF_STAMP(2);
      }
      lossacc += (double)lsum;

      // the tile's global loads, in the order their results are needed
      constexpr int NDL = PmfDTile<DB>::NCH;
      constexpr int V_C = 3, V_B = V_C + 1, V_S = V_B + (BATCH ? 2 : 0), V_D = V_S + (GY ? RV4 : 0), V_F = V_D + RBW * NDL, NVM = V_F + RBW;
      auto vmem_op = [&](int i) __attribute__((always_inline)) {
        if (i == 0 && BATCH) { btv[0] = pmf_bt_view(a, jn, tid); btv[1] = pmf_bt_view(a, jn, tid + NT); }
        if (i < V_C) stage_load_y(jn, i, ynext);
        else if (i < V_B) stage_load_c(jn, cnext);
        else if (i < V_S) { if (BATCH) btn[i - V_B] = pmf_bt_entry(a, Pm, jn, tid + NT * (i - V_B), btv[i - V_B]); }
        else if (i < V_D) { if (GY) slab_prefetch_one(j0, i - V_S); }
        else if (i < V_F) { const int rb = (i - V_D) / NDL, q = (i - V_D) % NDL; dcur[rb].load(a.D, (jn >> 5) * a.nRB + rb_u[rb], lane, q); }
        else { const int rb = i - V_F; tflag[rb] = a.tflags[(jn >> 5) * a.nRB + rb_u[rb]]; }
      };

      // ---- GEMM2: gX[i,k] += sum_j G[j,i] Ys[k,j]   (A = G registers, B = the Y image read transposed, once for both
      //      row blocks); the tile's global loads are spread over its groups
      bf16x8 b2h[2], b2l[2];
      auto g2_read = [&](int g, int slot) __attribute__((always_inline)) {
        const int S = g / KB, kb = g % KB;
        b2h[slot] = pmf_sb_tr8(Yc + y_tr_off(S, 0, kb), Yc + y_tr_off(S, 1, kb));
        b2l[slot] = pmf_sb_tr8(Yc + IMG + y_tr_off(S, 0, kb), Yc + IMG + y_tr_off(S, 1, kb));
      };
      if (GX) g2_read(0, 0);
      bf16x8 a3h[RBW][2], a3l[RBW][2];   // GEMM3's A fragments (the G images read transposed): requested between GEMM2's MFMAs
      auto a3_read = [&](int i) __attribute__((always_inline)) {   // i = 0..7: (rb, S, hi | mid)
        const int rb = i >> 2, S = (i >> 1) & 1;
        if (i & 1) a3l[rb][S] = pmf_sb_tr8(Tw[rb] + 2048 + t_tr_off(S, 0), Tw[rb] + 2048 + t_tr_off(S, 1));
        else a3h[rb][S] = pmf_sb_tr8(Tw[rb] + t_tr_off(S, 0), Tw[rb] + t_tr_off(S, 1));
      };
      constexpr int OPG = (NVM + NG - 1) / NG;
      static_assert(OPG <= 8, "load schedule");
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int S = g / KB, kb = g % KB;
        // six MFMAs, five gaps: gap 0 the next group's B reads, gaps 1..4 one global load + (GY) one G-image read each
        auto gap = [&](int z) __attribute__((always_inline)) {
          PMF_F();
          if (z == 0) { if (g + 1 < NG && GX) g2_read(g + 1, (g + 1) & 1); }
          else {
#pragma unroll
            for (int k = z - 1; k < OPG; k += 4)   // the group's OPG loads over the four gaps
              if (OPG * g + k < NVM) vmem_op(OPG * g + k);
            if (GY && z <= 2) a3_read(2 * g + z - 1);
          }
          PMF_F();
        };
        if (GX) {
          gx[0][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[0][S], b2h[g & 1], gx[0][kb], 0, 0, 0); gap(0);
          gx[1][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[1][S], b2h[g & 1], gx[1][kb], 0, 0, 0); gap(1);
          gx[0][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[0][S], b2l[g & 1], gx[0][kb], 0, 0, 0); gap(2);
          gx[1][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[1][S], b2l[g & 1], gx[1][kb], 0, 0, 0); gap(3);
          gx[0][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[0][S], b2h[g & 1], gx[0][kb], 0, 0, 0); gap(4);
          gx[1][kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[1][S], b2h[g & 1], gx[1][kb], 0, 0, 0);
          PMF_F();
        } else {
          gap(0); gap(1); gap(2); gap(3); gap(4);
        }
      }
#undef PMF_F

      PMF_STAMP(3);
      // ---- GEMM3: gY[j,k] = sum_i G[j,i] X[k,i] over the wave's 64 rows (A = the G images transposed, B = the X images
      //      transposed), one accumulator pair for both row blocks
      if (GY) {
        f32x16 gy[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) gy[kb][r] = 0.f;
#pragma unroll
        for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const int S = g / KB, kb = g % KB;
            gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3l[rb][S], b3h[rb][g], gy[kb], 0, 0, 0);
            gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3h[rb][S], b3l[rb][g], gy[kb], 0, 0, 0);
            gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3h[rb][S], b3h[rb][g], gy[kb], 0, 0, 0);
          }
        PMF_STAMP(4);
        // the slab's last k block aliases the first G image: every read of it has been issued (in-order LDS)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) Sw[kb * 1024 + pmf_rowmap(r, h) * 32 + l31] = gy[kb][r];
      }

      PMF_STAMP(9);
      // ---- publish Y(t+1) into the other buffer; B1 also completes this tile's slabs
      stage_store(par ^ 1, par ^ 1, jn, ynext, cnext);
      PMF_STAMP(5);
      __syncthreads();                 // B1
      PMF_STAMP(6);
      if (BATCH) {
#pragma unroll
        for (int q = 0; q < 2; ++q) Bt[tid + NT * q] = btn[q];
      }
      slab_first = pidx == 0 || (pidx == 1 && ti0 + t < t0_first);
      forward_reduce(acc, par ^ 1, par ^ 1, GY, j0);
      PMF_STAMP(7);
      __syncthreads();                 // B2: slabs, G images, the lo image and the batch table are free again
      PMF_STAMP(10);
    }

    // ---- flush gX (lane = factor index k, register = row): plain stores to the piece's own slot (see pmf_fused_kernel)
    if (GX) {
      float *gp = a.gx_part + (int64_t)gx_slot * a.gx_slot_stride + (int64_t)(w * RBW) * 32 * Kp + l31;
#pragma unroll
      for (int rb = 0; rb < RBW; ++rb)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) gp[(rb * 32 + pmf_rowmap(r, h)) * Kp + 32 * kb] = gx[rb][kb][r];
    }
    ++gx_slot;
    PMF_STAMP(11);
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
#ifdef PMF_STAMPS
  st_acc[14] = __builtin_amdgcn_s_memtime() - st_t0;
  st_acc[15] = __builtin_amdgcn_s_memrealtime() - st_r0;
  if (a.stamps && (threadIdx.x & 63) == 0) {
    for (int q = 0; q < 16; ++q) a.stamps[((int64_t)blockIdx.x * NW + (threadIdx.x >> 6)) * 16 + q] = st_acc[q];
  }
#endif
}
