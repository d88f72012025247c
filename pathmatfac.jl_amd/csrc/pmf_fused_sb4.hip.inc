// pmf_fused_sb4.hip.inc -- the fused data pass on split-bf16 products for 64 < K <= 128 (included by pmf_k_sb4.hip).
//
// Same computation, work split, private gY slabs, gX slots and outputs as pmf_fused_kernel / pmf_fused_sb_kernel; the
// arithmetic is pmf_fused_sb_kernel's (six-term bf16 forward as accurate as the f32 MFMA, three-term gradient products).
// What differs is where the operands live.  At K = 128 a 32-row operand image is 8 KiB per term, so eight X panels,
// two Y tiles and eight slabs do not fit the CU's 160 KiB of LDS.  This variant runs FOUR waves per workgroup, one per
// SIMD, with the whole 512-entry register file per lane (launch_bounds(256, 1)):
//   * a wave's X operands never touch LDS: the forward's B fragments (hi, mid, lo rows: 24 x 16 B per lane at K = 128)
//     and GEMM3's B fragments (hi, mid, pre-transposed by k_sb4_split: 16 x 16 B) are loaded from the global operand
//     images straight into registers once per piece and stay there for the whole column sweep;
//   * LDS holds the Y tile (hi + mid double buffered, lo single), the four per-wave gY slabs (the wave's G image
//     aliases the last k block of its slab) and the tile's column parameters: 106 KiB.
// Row panel = 128 rows (BM = 32 * 4), as the exact kernel's K > 64 variants.
//
// Image layout (Sb4Cfg, pmf_common.h): 256-byte rows whatever K, 16-B chunk ch of row r at
//     256 r + 16 (ch ^ f(r)),  f(r) = ((r & 3) << 2) | ((r >> 2) & 3)
// conflict-free for the row reads (ds_read_b128, lane = row: the 16 lanes of a read group hit 16 different 16-B slots of
// the 256-B bank window) and for the transposed reads (ds_read_b64_tr_b16: four rows x four chunks of a 16-lane group hit
// 16 different slots).  The forward walks the chunks in the order ch = FS h + S (FS = 2 KB k-steps), the same for X and Y.

// Operand images of 32 rows of X (samples) or 32 columns of Y (features), K padded to 128: hi, mid, lo row images in the
// LDS layout above and -- for X -- the hi and mid images TRANSPOSED ([k][i], 64-byte rows: GEMM3's B fragment of lane
// (k, h) is the 16 contiguous bytes i = 16 S + 8 h .. + 7).  One workgroup of 256 threads per 32-row block.
// src: [n][Ksrc] f32 (Ksrc = the context's padded K: 96 or 128); scale = colp (.x = sigma) or null.

#if !PMF_DB && PMF_KB == 4   // (one copy: the translation unit of the K = 128, f32-storage variants holds it)
__global__ __launch_bounds__(256) void k_sb4_split(const Sb4SplitArgs a) {
  constexpr int IMG = Sb4Cfg<4>::IMG;
  __shared__ __attribute__((aligned(16))) __bf16 tr[2][128][32 + 8];   // [term][k][i] (+8: the scatter below spreads over banks)
  const int64_t blk = blockIdx.x;
  if (blk >= a.nblk) return;
  const int tid = threadIdx.x, r = tid >> 3, c0 = (tid & 7) * 2;   // thread = (row, two 16-B chunks = 16 factors)
  const int64_t row = blk * 32 + r;
  char *ob = a.out + blk * (int64_t)(a.transposed ? 5 : 3) * IMG;
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const int ch = c0 + cc;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < a.n && ch * 8 < a.Ksrc) {
      const float4 p0 = *reinterpret_cast<const float4 *>(a.src + row * a.Ksrc + ch * 8);
      const float4 p1 = *reinterpret_cast<const float4 *>(a.src + row * a.Ksrc + ch * 8 + 4);
      const float s = a.colp ? a.colp[row].x : 1.f;
      v[0] = p0.x * s; v[1] = p0.y * s; v[2] = p0.z * s; v[3] = p0.w * s;
      v[4] = p1.x * s; v[5] = p1.y * s; v[6] = p1.z * s; v[7] = p1.w * s;
    }
    bf16x8 hi, mid, lo;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      hi[q] = (__bf16)v[q];
      const float r1 = v[q] - (float)hi[q];
      mid[q] = (__bf16)r1;
      lo[q] = (__bf16)(r1 - (float)mid[q]);
      if (a.transposed) { tr[0][ch * 8 + q][r] = hi[q]; tr[1][ch * 8 + q][r] = mid[q]; }
    }
    const int off = pmf_sb4_off(r, ch);
    *reinterpret_cast<bf16x8 *>(ob + off) = hi;
    *reinterpret_cast<bf16x8 *>(ob + IMG + off) = mid;
    *reinterpret_cast<bf16x8 *>(ob + 2 * IMG + off) = lo;
  }
  if (a.transposed) {
    __syncthreads();
    // [k][i]: 128 rows of 64 bytes per image = 512 16-B pieces per image, two per thread
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int pc = tid + 256 * q, k = pc >> 2, i0 = (pc & 3) * 8;
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = tr[t][k][i0 + e];
        *reinterpret_cast<bf16x8 *>(ob + (3 + t) * IMG + k * 64 + i0 * 2) = o;
      }
  }
}
#endif

// -DPMF_ABLATE=<bits>: measurement-only builds (WRONG results) that price one cost at a time:
//   1 no private-slab read-modify-write in HBM   2 no per-wave slab writes (LDS)   4 no cross-wave slab reads (LDS)
//   8 no staging of the next Y tile (global loads + LDS stores)   16 no loads of D   32 no G image / GEMM3 operand reads
#ifndef PMF_ABLATE
#define PMF_ABLATE 0
#endif
template <int KB, bool MIXED, bool GX, bool GY, bool BATCH, bool DB>
__global__ __launch_bounds__(256, 1) void pmf_fused_sb4_kernel(const FusedArgs a) {
  using Cfg = Sb4Cfg<KB>;
  constexpr int NW = 4, NT = 256, Kp = Cfg::Kp, BN = PMF_BN, BM = 32 * NW, SLAB = Cfg::SLAB;
  constexpr int IMG = Cfg::IMG, XBLK = Cfg::XBLK, YBLK = Cfg::YBLK, LDSP = 2 * IMG;
  constexpr int FS = 2 * KB;        // k-steps of the forward (16 factors each)
  constexpr int NG = 2 * KB;        // (16-row / 16-column step, k block) groups of GEMM2 / GEMM3
  constexpr int RV4 = KB;           // float4 of the [Kp x 32] gY tile per thread (1024 KB / 4 / 256)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Yi = smem;                                         // [2][hi image, mid image]
  char *Yl = Yi + 2 * LDSP;                                // lo image of the tile whose forward runs next (single buffer)
  float *Sl = reinterpret_cast<float *>(Yl + IMG);         // [NW][SLAB]
  float *Cmu = Sl + NW * SLAB;                             // [2][BN]
  float *Cw = Cmu + 2 * BN;
  float *Csg = Cw + 2 * BN;
  int *Cmt = reinterpret_cast<int *>(Csg + 2 * BN);
  int *Ck = Cmt + 2 * BN;
  double *red = reinterpret_cast<double *>(Ck + 4);
  // (BATCH) the tile's dense batch table as two planes [16 slots][32 columns]: delta, and theta + mu_j (pmf_fused_sb8.hip.inc)
  float *Btd = reinterpret_cast<float *>(smem + Cfg::lds_bytes), *Btt = Btd + BN * 16;
  unsigned char *Pm = reinterpret_cast<unsigned char *>(Btd + 2 * BN * 16);                             // (BATCH) the piece's slot -> batch map [n_bv][16]
  unsigned char *Bw0 = Pm + PMF_PM_BYTES + (threadIdx.x >> 6) * a.n_bv * 32;                       // (BATCH) this wave: [n_bv][32] slot of every row

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  float *Sw = Sl + w * SLAB;
  char *Tw = reinterpret_cast<char *>(Sw + (KB - 1) * 1024);   // the wave's G image (hi 2 KiB, lo 2 KiB) aliases the slab's last k block

  // ---- per-lane LDS byte offsets (constant for the whole kernel)
  int rowoff[FS];   // row reads (forward): lane = row l31, chunk FS h + S
#pragma unroll
  for (int S = 0; S < FS; ++S) rowoff[S] = pmf_sb4_off(l31, FS * h + S);
  // transposed reads: lane 4q+p of the 16-lane group G4 supplies row (r0 + q), columns 16 (G4&1) + 4p .. +3 (+ 32 kb)
  const int G4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  // GEMM2 B (Y image): rows j = 16S + 8b + 4h + q; chunk = 4kb + 2(G4&1) + (p>>1)
  auto y_tr_off = [&](int S, int b, int kb) {
    return pmf_sb4_off(16 * S + 8 * b + 4 * h + tq, 4 * kb + 2 * (G4 & 1) + (tp >> 1)) + 8 * (tp & 1);
  };
  // GEMM3 A (G image, 64-B rows, 8-B chunk cj = 4(G4&1) + p, XOR (i>>1)&7): rows i = 16S + 8h + 4b + q
  auto t_tr_off = [&](int S, int b) {
    const int i = 16 * S + 8 * h + 4 * b + tq;
    return 64 * i + 8 * ((4 * (G4 & 1) + tp) ^ ((i >> 1) & 7));
  };

  const int wg = pmf_xcd_wg(blockIdx.x, gridDim.x);
  const int64_t w_begin = a.wg_begin[wg];
  const int64_t w_end = a.wg_begin[wg + 1];
  float *myslab = a.gy_slabs + (int64_t)wg * a.slab_stride;
  const int64_t seg_block = a.n_rp * a.tps;
  double lossacc = 0.0;
  int seg_cur = -1, pidx = 0, t0_first = 0;
  int gx_slot = GX ? a.piece_base[wg] : 0;
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
    const int64_t col_begin_first = (PMF_ABLATE & 8) ? col_begin : -1;   // (ablation 8 stages the piece's first tile only)
    const int64_t row0 = rp * BM + (int64_t)w * 32;
    const bool row_ok = row0 + l31 < M;
    const int rb_raw = __builtin_amdgcn_readfirstlane((int)(row0 >> 5));
    const bool rows_in = rb_raw < a.nRB;
    const int rb_u = rows_in ? rb_raw : (int)a.nRB - 1;

    // ---- this wave's X operands, global images -> registers (they stay there for the whole piece)
    bf16x8 xh[FS], xm[FS], xl[FS];   // forward B fragments: lane = row l31, factors of chunk FS h + S
    bf16x8 b3h[NG], b3l[NG];         // GEMM3 B fragments: lane = factor 32 kb + l31, rows 16 S + 8 h .. + 7 (transposed images)
    {
      const char *xblk = a.Xsb + (int64_t)rb_u * XBLK;
#pragma unroll
      for (int S = 0; S < FS; ++S) {
        xh[S] = *reinterpret_cast<const bf16x8 *>(xblk + rowoff[S]);
        xm[S] = *reinterpret_cast<const bf16x8 *>(xblk + IMG + rowoff[S]);
        xl[S] = *reinterpret_cast<const bf16x8 *>(xblk + 2 * IMG + rowoff[S]);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int S = g / KB, kb = g % KB;
        const int o = (32 * kb + l31) * 64 + (16 * S + 8 * h) * 2;
        b3h[g] = *reinterpret_cast<const bf16x8 *>(xblk + 3 * IMG + o);
        b3l[g] = *reinterpret_cast<const bf16x8 *>(xblk + 4 * IMG + o);
      }
    }
    f32x16 gx[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) gx[kb][r] = 0.f;

    // Staging the next Y tile: hi + mid images = 1024 16-B chunks (4 per thread), lo = 512 (2 per thread).
    // (Loads from in-bounds addresses, untouched until stage_store.)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    auto stage_load_y = [&](int64_t jt, int c, u32x4 (&yv)[6]) __attribute__((always_inline)) {
      yv[c] = (reinterpret_cast<const u32x4 *>(a.Ysb + (jt >> 5) * (int64_t)YBLK))[tid + NT * c];   // c = 0..3: hi, mid; 4..5: lo
    };
    auto stage_load_c = [&](int64_t jt, float4 &cv) __attribute__((always_inline)) {
      const float4 *cb = a.colp + jt;
      const int64_t rem = N - jt;
      const int ncol = rem > BN ? BN : (int)rem;
      cv = cb[tid < ncol ? tid : ncol - 1];
    };
    auto stage_store = [&](int ybuf, int cbuf, int64_t jt, const u32x4 (&yv)[6], const float4 &cv) __attribute__((always_inline)) {
      if (!(PMF_ABLATE & 8) || jt == col_begin_first) {
#pragma unroll
        for (int c = 0; c < 4; ++c) reinterpret_cast<u32x4 *>(Yi + ybuf * LDSP)[tid + NT * c] = yv[c];
#pragma unroll
        for (int c = 0; c < 2; ++c) reinterpret_cast<u32x4 *>(Yl)[tid + NT * c] = yv[4 + c];
      }
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
        if (BATCH) {   // the view of the tile's columns when they all share one (-1: in no view); -2: the tile straddles views
          const int vw = (__float_as_int(cv.w) >> 2) - 1;
          const int vw0 = __builtin_amdgcn_readfirstlane(vw);
          const unsigned mv = (unsigned)__ballot(!livec || vw == vw0);
          if (tid == 0) Ck[2 + cbuf] = mv == 0xffffffffu ? vw0 : -2;
        }
      }
    };
    // (BATCH) staging: thread tid takes entries (column tid & 31, slots tid >> 5 and 8 + (tid >> 5)): a wave writes 32 consecutive
    // words of two slot rows of each plane
    auto bt_e = [&](int q) { return (tid & 31) * 16 + (tid >> 5) + 8 * q; };
    auto bt_mu = [&](int64_t jt, int e) -> float { const int64_t j = jt + (e >> 4); return j < N ? a.colp[j].y : 0.f; };
    auto bt_store = [&](int e, const float2 &dt, float mu) __attribute__((always_inline)) {
      const int o = (e & 15) * 32 + (e >> 4);
      Btd[o] = dt.x;
      Btt[o] = dt.y + mu;
    };
    // slab reduction mapping: thread -> float4 f = tid + 256 q of the [kb][j][32 k] slab (kb = q);
    // element e = j*Kp + 32 kb + k of the [j][Kp] gY tile
    float4 gold[RV4];
    PmfDTile<DB> dcur;
    const int s_j = tid >> 3, s_k4 = (tid & 7) * 4;
    auto slab_prefetch_one = [&](int64_t jt, int q) __attribute__((always_inline)) {
      const float *sb = myslab + jt * Kp;
      const int64_t rem = N - jt;
      const int nel = (rem > BN ? BN : (int)rem) * Kp;
      const int e = s_j * Kp + 32 * q + s_k4;
      gold[q] = pmf_load_stream(reinterpret_cast<const float4 *>(sb + (e < nel ? e : (e % Kp))));
    };
    // forward of one tile (6 FS MFMAs) with the reduction of the previous tile's slabs between them
    auto forward_reduce = [&](f32x16 &acc, int ybuf, int cbuf, bool do_red, int64_t jt_red) __attribute__((always_inline)) {
      const int cb0 = cbuf * BN + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = BATCH ? 0.f : Cmu[cb0 + (r & 3) + 8 * (r >> 2)];   // (mu joins after the batch scale)
      const char *Yc = Yi + ybuf * LDSP;
      float4 racc[RV4];
#pragma unroll
      for (int q = 0; q < RV4; ++q) racc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      // the operand reads run one k-step ahead of the MFMAs
      bf16x8 yh = *reinterpret_cast<const bf16x8 *>(Yc + rowoff[0]);
      bf16x8 ym = *reinterpret_cast<const bf16x8 *>(Yc + IMG + rowoff[0]);
      bf16x8 yl = *reinterpret_cast<const bf16x8 *>(Yl + rowoff[0]);
#pragma unroll
      for (int S = 0; S < FS; ++S) {
        bf16x8 yhn = yh, ymn = ym, yln = yl;
        if (S + 1 < FS) {
          yhn = *reinterpret_cast<const bf16x8 *>(Yc + rowoff[S + 1]);
          ymn = *reinterpret_cast<const bf16x8 *>(Yc + IMG + rowoff[S + 1]);
          yln = *reinterpret_cast<const bf16x8 *>(Yl + rowoff[S + 1]);
        }
        // 4 KB slab reads per thread (KB float4 x 4 slabs) over 2 KB k-steps: two per step
        float4 sv[2];
        if (do_red) {
#pragma unroll
          for (int z = 0; z < 2; ++z) {
            const int idx = 2 * S + z, q = idx >> 2, sl = idx & 3;      // idx = 4 q + slab
            if (PMF_ABLATE & 4) sv[z] = make_float4(1.f, 2.f, 3.f, 4.f);
            else sv[z] = *reinterpret_cast<const float4 *>(Sl + sl * SLAB + 4 * (tid + NT * q));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        // six of the nine partial products (mid*lo, lo*mid, lo*lo are below 2^-24 of the product): Z as accurate as the
        // exact-f32 MFMA's, which matters because G = w (Z - D) cancels most of Z once the model fits
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yl, xh[S], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xl[S], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xm[S], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xh[S], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xm[S], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xh[S], acc, 0, 0, 0);
        if (do_red) {
#pragma unroll
          for (int z = 0; z < 2; ++z) {
            float4 &ra = racc[(2 * S + z) >> 2];
            ra.x += sv[z].x; ra.y += sv[z].y; ra.z += sv[z].z; ra.w += sv[z].w;
          }
        }
        yh = yhn; ym = ymn; yl = yln;
        __builtin_amdgcn_sched_barrier(0);
      }
      if (do_red) {
        dcur.touch();   // the (long finished) D loads count as consumed before the stores below are issued
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
          if (e < nel && !(PMF_ABLATE & 1)) pmf_store_stream(reinterpret_cast<float4 *>(sb + e), v);
          if (PMF_ABLATE & 1) asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w));
        }
      }
    };

    uint32_t tflag = a.tflags[(col_begin >> 5) * a.nRB + rb_u];
#pragma unroll
    for (int q = 0; q < PmfDTile<DB>::NCH; ++q) dcur.load(a.D, (col_begin >> 5) * a.nRB + rb_u, lane, q);
    {
      u32x4 yv[6];
      float4 cv;
#pragma unroll
      for (int c = 0; c < 6; ++c) stage_load_y(col_begin, c, yv);
      stage_load_c(col_begin, cv);
      stage_store(0, 0, col_begin, yv, cv);
      if (BATCH) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {   // 32 columns x 16 slots = 512 entries (first tile: slot map straight from global memory)
          const int e = bt_e(q);
          bt_store(e, pmf_bt_entry(a, a.pm + rp * a.n_bv * 16, col_begin, e, pmf_bt_view(a, col_begin, e)), bt_mu(col_begin, e));
        }
        if (tid < a.n_bv * 16) Pm[tid] = a.pm[rp * a.n_bv * 16 + tid];
        if (h == 0) {   // panel-local slot of this wave's rows in every view (15 = identity: row in no batch)
          const int64_t irow_c = row_ok ? row0 + l31 : M - 1;
          for (int v = 0; v < a.n_bv; ++v) Bw0[v * 32 + l31] = a.row_slot[(int64_t)v * M + irow_c];
        }
      }
    }
    __syncthreads();

    f32x16 acc;
    forward_reduce(acc, 0, 0, false, 0);

    for (int t = 0; t < ntiles; ++t) {
      const int par = t & 1;
      const int64_t j0 = col_begin + (int64_t)t * BN;
      const char *Yc = Yi + par * LDSP;
      const bool have_next = (t + 1 < ntiles);
      const int cb0 = par * BN + 4 * h;
      u32x4 ynext[6];
      float4 cnext;
      float2 btn[2];     // (BATCH) this thread's entries of the next tile's dense batch table
      float btm[2] = {0.f, 0.f};   //    and their columns' mu
      int btv[2] = {255, 255};

      // ---- epilogue (identical to pmf_fused_sb_kernel): acc becomes G
      float lsum = 0.f;
      const int tkind = MIXED ? __builtin_amdgcn_readfirstlane(Ck[par]) : 0;
      const int tview = BATCH ? __builtin_amdgcn_readfirstlane(Ck[2 + par]) : -1;   // the tile's view; -2: it straddles two
      // General epilogue of one register, given the entry's batch scale dl and shift th = theta + mu_j (batch layers only: without
      // them mu_j was the accumulator's initial value).  Gaussian columns mask by substitution (y := z: d = 0, g = 0, no loss)
      // and sum g d, halved once per tile; all-finite tiles (fast, batch variants only) skip the mask.
      float lnorm = 0.f;
      auto epi_reg = [&](int r, float dl, float th, float wj, int kmode, bool fast) __attribute__((always_inline)) {
        float z = acc[r];
        if (BATCH) z = fmaf(z, dl, th);
        float y = dcur.get(r);
        if (kmode == PMF_NOISE_NORMAL) {
          if (!fast) y = (pmf_finite(y) && row_ok) ? y : z;
          const float d = z - y, g = wj * d;
          lnorm = fmaf(g, d, lnorm);
          acc[r] = BATCH ? g * dl : g;
        } else {
          const bool ok = pmf_finite(y) && row_ok;
          float l, g;
          if (kmode == 3) pmf_noise<MIXED>(Cmt[cb0 + (r & 3) + 8 * (r >> 2)] & 3, z, y, wj, a.htab + (j0 + 4 * h) * PMF_HT + PMF_HT * ((r & 3) + 8 * (r >> 2)), l, g);
          else pmf_noise(kmode, z, y, wj, nullptr, l, g);
          lsum += ok ? l : 0.f;
          acc[r] = ok ? (BATCH ? g * dl : g) : 0.f;
        }
      };
      auto grp_load = [&](int c4, bool uni, const float *bdl, const float *btl, float4 &dl4, float4 &th4) __attribute__((always_inline)) {
        if (!BATCH) {
          th4 = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (uni) {
          dl4 = *reinterpret_cast<const float4 *>(bdl + 8 * c4);
          th4 = *reinterpret_cast<const float4 *>(btl + 8 * c4);
        } else {   // the tile straddles two views: view and slot per entry
          float dv[4], tv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int cl = 8 * c4 + 4 * h + u;
            const int v = (Cmt[par * BN + cl] >> 2) - 1;
            const int bsr = v < 0 ? 15 : Bw0[v * 32 + l31];
            dv[u] = Btd[bsr * 32 + cl];
            tv[u] = Btt[bsr * 32 + cl];
          }
          dl4 = make_float4(dv[0], dv[1], dv[2], dv[3]);
          th4 = make_float4(tv[0], tv[1], tv[2], tv[3]);
        }
      };
      const float4 *cw4 = reinterpret_cast<const float4 *>(Cw + cb0);
      auto f4get = [](const float4 &v, int u) { return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w)); };
      const int64_t jn = have_next ? j0 + BN : j0;
      const bool tile_fast = rows_in && tflag != 0;
      // the tile's global loads, in the order their results are needed: Y(t+1) and its column parameters (stage_store),
      // the batch table, the old private-slab values of tile t (slab reduction), D(t+1) and its flag (next epilogue)
      constexpr int NDL = PmfDTile<DB>::NCH;
      constexpr int NVM = 6 + 1 + (BATCH ? 2 : 0) + (GY ? RV4 : 0) + NDL + 1;
      constexpr int V_C = 6, V_B = V_C + 1, V_S = V_B + (BATCH ? 2 : 0), V_D = V_S + (GY ? RV4 : 0), V_F = V_D + NDL;
      static_assert(V_F + 1 == NVM, "load schedule");
      auto vmem_op = [&](int i) __attribute__((always_inline)) {
        if (i == 0 && BATCH) { btv[0] = pmf_bt_view(a, jn, bt_e(0)); btv[1] = pmf_bt_view(a, jn, bt_e(1)); }
        if (i < V_C) { if (!(PMF_ABLATE & 8)) stage_load_y(jn, i, ynext); }
        else if (i < V_B) stage_load_c(jn, cnext);
        else if (i < V_S) { if (BATCH) { btn[i - V_B] = pmf_bt_entry(a, Pm, jn, bt_e(i - V_B), btv[i - V_B]); btm[i - V_B] = bt_mu(jn, bt_e(i - V_B)); } }
        else if (i < V_D) { if (GY && !(PMF_ABLATE & 1)) slab_prefetch_one(j0, i - V_S); }
        else if (i < V_F) { if (!(PMF_ABLATE & 16)) dcur.load(a.D, (jn >> 5) * a.nRB + rb_u, lane, i - V_D); }
        else tflag = a.tflags[(jn >> 5) * a.nRB + rb_u];
      };
      typedef float f32x2 __attribute__((ext_vector_type(2)));
      if (!BATCH && tile_fast && (!MIXED || tkind == 0)) {
        f32x2 ls2 = {0.f, 0.f};
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
          const float4 w4 = cw4[2 * c4];
#pragma unroll
          for (int p2 = 0; p2 < 2; ++p2) {
            const int r = 4 * c4 + 2 * p2;
            const f32x2 zz = {acc[r], acc[r + 1]}, yy = {dcur.get(r), dcur.get(r + 1)};
            const f32x2 ww = p2 == 0 ? f32x2{w4.x, w4.y} : f32x2{w4.z, w4.w};
            const f32x2 dd = zz - yy;
            const f32x2 gg = ww * dd;
            ls2 = gg * dd + ls2;
            acc[r] = gg.x; acc[r + 1] = gg.y;
          }
        }
        lsum += 0.5f * (ls2.x + ls2.y);
      } else {
        int bs = 15;
        if (BATCH && tview >= 0) bs = Bw0[tview * 32 + l31];   // this row's slot in the tile's view: once per tile
        const float *bdl = Btd + bs * 32 + 4 * h, *btl = Btt + bs * 32 + 4 * h;
        auto epi_all = [&](int kmode, bool uni, bool fast) __attribute__((always_inline)) {
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) {
            const float4 w4 = cw4[2 * c4];
            float4 dl4 = make_float4(1.f, 1.f, 1.f, 1.f), th4;
            grp_load(c4, uni, bdl, btl, dl4, th4);
#pragma unroll
            for (int u = 0; u < 4; ++u) epi_reg(4 * c4 + u, f4get(dl4, u), f4get(th4, u), f4get(w4, u), kmode, fast);
          }
        };
        if (BATCH && tview == -2) epi_all(3, false, false);
        // (the mask-free copy is for the batch variants: without batch layers an all-finite Gaussian tile took the packed path above)
        else if (!MIXED || tkind == 0) { if (BATCH && tile_fast) epi_all(PMF_NOISE_NORMAL, true, true); else epi_all(PMF_NOISE_NORMAL, true, false); }
        else if (tkind == 1) epi_all(PMF_NOISE_BERNOULLI, true, false);
        else if (tkind == 2) epi_all(PMF_NOISE_POISSON, true, false);
        else epi_all(3, true, false);
      }
      lossacc += (double)fmaf(0.5f, lnorm, lsum);

      // ---- split G into bf16 hi / lo; registers 8S..8S+7 are GEMM2's A fragment of step S
      bf16x8 gh[2], gl[2];
#pragma unroll
      for (int S = 0; S < 2; ++S)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = acc[8 * S + e];
          const __bf16 hi = (__bf16)g;
          gh[S][e] = hi;
          gl[S][e] = (__bf16)(g - (float)hi);
        }
      // the wave's [i][j] image of G for GEMM3: registers 4g..4g+3 = columns j = 8g + 4h .. +3 = 8-B chunk 2g + h of row i
#pragma unroll
      for (int g = 0; GY && g < 4; ++g) {
        const int o = 64 * l31 + 8 * ((2 * g + h) ^ ((l31 >> 1) & 7));
        const bf16x4 vh = {gh[g >> 1][4 * (g & 1)], gh[g >> 1][4 * (g & 1) + 1], gh[g >> 1][4 * (g & 1) + 2], gh[g >> 1][4 * (g & 1) + 3]};
        const bf16x4 vl = {gl[g >> 1][4 * (g & 1)], gl[g >> 1][4 * (g & 1) + 1], gl[g >> 1][4 * (g & 1) + 2], gl[g >> 1][4 * (g & 1) + 3]};
        *reinterpret_cast<bf16x4 *>(Tw + o) = vh;
        *reinterpret_cast<bf16x4 *>(Tw + 2048 + o) = vl;
      }

      // ---- GEMM2: gX[i,k] += sum_j G[j,i] Ys[k,j]   (A = G registers, B = the Y image read transposed); the tile's
      //      global loads are spread over its groups
      bf16x8 b2h[2], b2l[2];
      auto g2_read = [&](int g, int slot) __attribute__((always_inline)) {
        const int S = g / KB, kb = g % KB;
        b2h[slot] = pmf_sb_tr8(Yc + y_tr_off(S, 0, kb), Yc + y_tr_off(S, 1, kb));
        b2l[slot] = pmf_sb_tr8(Yc + IMG + y_tr_off(S, 0, kb), Yc + IMG + y_tr_off(S, 1, kb));
      };
      bf16x8 a3h[2], a3l[2];
      auto g3_read_a = [&](int S) __attribute__((always_inline)) {
        a3h[S] = pmf_sb_tr8(Tw + t_tr_off(S, 0), Tw + t_tr_off(S, 1));
        a3l[S] = pmf_sb_tr8(Tw + 2048 + t_tr_off(S, 0), Tw + 2048 + t_tr_off(S, 1));
      };
      if (GX) g2_read(0, 0);
      __builtin_amdgcn_sched_barrier(0);
      constexpr int OPG = (NVM + NG - 1) / NG;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int S = g / KB, kb = g % KB;
        if (g + 1 < NG) { if (GX) g2_read(g + 1, (g + 1) & 1); }
        else if (GY) { g3_read_a(0); g3_read_a(1); }
#pragma unroll
        for (int z = 0; z < OPG; ++z)
          if (OPG * g + z < NVM) vmem_op(OPG * g + z);
        __builtin_amdgcn_sched_barrier(0);
        if (GX) {
          gx[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[S], b2h[g & 1], gx[kb], 0, 0, 0);
          gx[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[S], b2l[g & 1], gx[kb], 0, 0, 0);
          gx[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[S], b2h[g & 1], gx[kb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }

      // ---- GEMM3: gY[j,k] = sum_i G[j,i] X[k,i] over the wave's 32 rows (A = the G image transposed, B = registers)
      if (GY) {
        f32x16 gy[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) gy[kb][r] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int S = g / KB, kb = g % KB;
          gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3l[S], b3h[g], gy[kb], 0, 0, 0);
          gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3h[S], b3l[g], gy[kb], 0, 0, 0);
          gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3h[S], b3h[g], gy[kb], 0, 0, 0);
        }
        // the slab's last k block aliases the G image: every read of it has been issued (in-order LDS)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (PMF_ABLATE & 2) { if (gy[kb][r] == 12345.678f) Sw[0] = 1.f; }
            else Sw[kb * 1024 + pmf_rowmap(r, h) * 32 + l31] = gy[kb][r];
          }
      }

      // ---- publish Y(t+1) into the other buffer; B1 also completes this tile's slabs
      stage_store(par ^ 1, par ^ 1, jn, ynext, cnext);
      __syncthreads();                 // B1
      if (BATCH) {                     // every wave is past its epilogue(t): the single table buffer takes tile t+1 (read after B2)
#pragma unroll
        for (int q = 0; q < 2; ++q) bt_store(bt_e(q), btn[q], btm[q]);
      }
      slab_first = pidx == 0 || (pidx == 1 && ti0 + t < t0_first);
      forward_reduce(acc, par ^ 1, par ^ 1, GY, j0);
      __syncthreads();                 // B2: slabs, G images, the lo image and the batch table are free again
    }

    // ---- flush gX (lane = factor index k, register = row): plain stores to the piece's own slot (see pmf_fused_kernel)
    if (GX) {
      float *gp = a.gx_part + (int64_t)gx_slot * a.gx_slot_stride + (int64_t)w * 32 * Kp + l31;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gp[pmf_rowmap(r, h) * Kp + 32 * kb] = gx[kb][r];
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
