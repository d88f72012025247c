// pmf_fused_sb.hip.inc -- the fused data pass on split-bf16 ("bf16x3") matrix products (included by pmf_k_sb.hip).
//
// Same computation, work split, private gY slabs and outputs as pmf_fused_kernel (pmf_fused.hip.inc); what changes is
// how the three products are evaluated.  v_mfma_f32_32x32x2_f32 is exact but runs at 1/16 of the bf16 rate and blocks
// the VALU for its 64 cycles.  Here every f32 operand x is carried as two bf16 numbers, hi = bf16(x) and
// mid = bf16(x - hi) (round to nearest even), and a product of two operands as three v_mfma_f32_32x32x16_bf16
// (mid*hi + hi*mid + hi*hi, f32 accumulation; mid*mid ~ 2^-18 of the product is dropped).  Measured error of a K = 64
// product: 4e-6 of max|Z| (scripts/bf16x3_probe.hip) against 2.3e-7 for the f32 MFMA.  That is enough for the two
// gradient products (12 MFMAs each) but NOT for the forward: G = w (Z - D) cancels most of Z once the model fits, and
// the 4e-6 |Z| became 1e-3 of the gradient in the parity tests.  The forward therefore carries a third term,
// lo = bf16(x - hi - mid), and six of the nine partial products (24 MFMAs; the dropped ones are < 2^-24): Z is then as
// accurate as the exact kernel's.  48 bf16 MFMAs (1536 matrix cycles) per tile and wave instead of 96 f32 ones (6144).
// Results are inside the parity tolerances of DESIGN.md section 2 but NOT bit-compatible with the exact kernel, so this
// path is opt-in (pmf_set_precision(ctx, PMF_PREC_BF16X3)).
//
// Scope of this first version: K <= 64 (KB = 1 or 2), 8 waves, one row block per wave, batch layers with <= 15 batches per view; both gradients
// (fit!), grad(X) only (transform) or grad(Y) only.  Everything else falls back to pmf_fused_kernel.
//
// Operands (cdna_hip_programming.md "An accumulator tile as the next MFMA's operand", T10):
//   X and sigma_j*Y are split once per epoch by k_sb_split into per-32-row "images" [32 rows][64 k] bf16 (hi, mid
//   and lo image, 4 KiB each), already in the LDS layout: byte offset of 16-B chunk ch (8 k) of row r
//       off(r, ch) = 128 r + 16 (ch ^ f(r)),  f(r) = x ^ ((x & 1) << 2), x = (r >> 1) & 7
//   which is conflict-free both for the row reads (ds_read_b128: lane = row, chunk 4h + S; the forward's A and B
//   operands) and for the transposed reads (ds_read_b64_tr_b16: lane = k, four rows per instruction; the B operands
//   of GEMM2 and GEMM3).  Staging a Y tile or an X panel is therefore a straight 16-B copy global -> LDS.
//   forward : Z[j,i]  = mu_j + sum_k Ys[k,j] X[k,i]        A = Y image rows, B = X image rows           24 MFMAs
//   epilogue: G[j,i] in the accumulator (lane = row i, register = column j), split to bf16 hi/lo pairs; registers
//             8S .. 8S+7 ARE the A fragment of GEMM2's k-step S (contraction order j = 16S + 8(e>>2) + 4h + (e&3));
//             the pairs are also written to the wave's [i][j] image T (64-B rows, 8-B chunks XOR (i>>1)&7)
//   GEMM2   : gX[i,k] += sum_j G[j,i] Ys[k,j]              A = G registers, B = Y image, transposed     12 MFMAs
//   GEMM3   : gY[j,k]  = sum_i G[j,i] X[k,i]               A = T transposed, B = X image transposed     12 MFMAs
//   then the slab write, the cross-wave slab reduction inside the next forward and the private-slab RMW, unchanged.

template <int KB>
__global__ __launch_bounds__(256) void k_sb_split(const SbSplitArgs a) {
  using Cfg = SbCfg<KB>;
  constexpr int CPR = 4 * KB, Kp = 32 * KB;   // 16-B chunks per row
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t row = idx / CPR;
  const int ch = (int)(idx % CPR);
  if (row >= a.nblk * 32) return;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (row < a.n) {
    const float4 p0 = *reinterpret_cast<const float4 *>(a.src + row * Kp + ch * 8);
    const float4 p1 = *reinterpret_cast<const float4 *>(a.src + row * Kp + ch * 8 + 4);
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
  }
  char *blk = a.out + (row >> 5) * Cfg::BLK + pmf_sb_off<KB>((int)(row & 31), ch);
  *reinterpret_cast<bf16x8 *>(blk) = hi;
  *reinterpret_cast<bf16x8 *>(blk + Cfg::IMG) = mid;
  *reinterpret_cast<bf16x8 *>(blk + 2 * Cfg::IMG) = lo;
}

// GY = false: grad(X) only (transform: Y and the layers fixed) -- no G image, no GEMM3, no slabs, one barrier per tile.
// GX = false: grad(Y) only -- no GEMM2, no gX flush (the tile's loads keep their place).
// BATCH: batch scale / shift layers through the LDS-staged dense table of pmf_fused_kernel's BMODE 1 (<= 15 batches per
// view; the per-wave batch-id table is sized by the number of views, which K = 64 limits to what LDS is left).
template <int KB, bool MIXED, bool GX, bool GY, bool BATCH, bool DB>
__global__ __launch_bounds__(512, 2) void pmf_fused_sb_kernel(const FusedArgs a) {
  using Cfg = SbCfg<KB>;
  constexpr int NW = 8, Kp = Cfg::Kp, BN = PMF_BN, BM = 32 * NW, SLAB = Cfg::SLAB;
  constexpr int IMG = Cfg::IMG, BLK = Cfg::BLK, LDSP = Cfg::LDSP;
  constexpr int FS = 2 * KB;        // k-steps of the forward (16 factors each)
  constexpr int NG = 2 * KB;        // (k-step, k block) groups of GEMM2 / GEMM3
  constexpr int TS = 256 * KB;      // threads that own a float4 of the [Kp x 32] gY tile (all 512 at K = 64)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *Yi = smem;                                         // [2][hi image, mid image]
  char *Yl = Yi + 2 * LDSP;                          // lo image of the tile whose forward runs next (single buffer)
  char *Xi = Yl + IMG;                              // [NW][hi, mid]
  float *Sl = reinterpret_cast<float *>(Xi + NW * LDSP);   // [NW][SLAB]
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
  const bool w_lo = __builtin_amdgcn_readfirstlane(w) < 4;   // wave-uniform (a scalar branch)
  float *Sw = Sl + w * SLAB;
  char *Xw = Xi + w * LDSP;
  char *Tw = reinterpret_cast<char *>(Sw + (KB - 1) * 1024);   // the wave's G image aliases the slab's last k block

  // ---- per-lane LDS byte offsets (constant for the whole kernel)
  // row reads (forward): lane = row l31, chunk FS h + S
  int rowoff[FS];
#pragma unroll
  for (int S = 0; S < FS; ++S) rowoff[S] = pmf_sb_off<KB>(l31, FS * h + S);
  // transposed reads: lane 4q+p of the 16-lane group G4 supplies row (r0 + q), columns 16 (G4&1) + 4p .. +3 (+ 32 kb)
  const int G4 = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  // GEMM2 B (Y image): rows j = 16S + 8b + 4h + q; chunk = 4kb + 2(G4&1) + (p>>1)
  auto y_tr_off = [&](int S, int b, int kb) {
    return pmf_sb_off<KB>(16 * S + 8 * b + 4 * h + tq, 4 * kb + 2 * (G4 & 1) + (tp >> 1)) + 8 * (tp & 1);
  };
  // GEMM3 B (X image): rows i = 16S + 8h + 4b + q
  auto x_tr_off = [&](int S, int b, int kb) {
    return pmf_sb_off<KB>(16 * S + 8 * h + 4 * b + tq, 4 * kb + 2 * (G4 & 1) + (tp >> 1)) + 8 * (tp & 1);
  };
  // GEMM3 A (G image, 64-B rows, 8-B chunk cj = 4(G4&1) + p, XOR (i>>1)&7): rows i as above
  auto t_tr_off = [&](int S, int b) {
    const int i = 16 * S + 8 * h + 4 * b + tq;
    return 64 * i + 8 * ((4 * (G4 & 1) + tp) ^ ((i >> 1) & 7));
  };

#ifdef PMF_STAMPS
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
  int gx_slot = GX ? a.piece_base[wg] : 0;   // slot of this workgroup's next piece in the gX partial buffer
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
    const int64_t row0 = rp * BM + (int64_t)w * 32;
    PMF_STAMP(10);
    const bool row_ok = row0 + l31 < M;
    const int rb_raw = __builtin_amdgcn_readfirstlane((int)(row0 >> 5));
    const bool rows_in = rb_raw < a.nRB;
    const int rb_u = rows_in ? rb_raw : (int)a.nRB - 1;

    // ---- this wave's X image (8 KiB): issue the loads now, store after the first Y / D loads are in flight
    uint4 xv0[4 * KB];
    bf16x8 xl[FS];  // the forward's lo fragments of X stay in registers (lane = row l31, k = 16 KB h + 8S .. +7)
    {
      const char *xblk = a.Xsb + (int64_t)rb_u * BLK;
      const uint4 *xb = reinterpret_cast<const uint4 *>(xblk) + lane;
#pragma unroll
      for (int q = 0; q < 4 * KB; ++q) xv0[q] = xb[64 * q];
#pragma unroll
      for (int S = 0; S < FS; ++S) xl[S] = *reinterpret_cast<const bf16x8 *>(xblk + 2 * IMG + rowoff[S]);
    }
    f32x16 gx[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) gx[kb][r] = 0.f;

    // Staging the next Y tile (6 KB KiB = 384 KB 16-B chunks: hi and mid image, then lo) is the job of waves 0-3 alone,
    // chunk c*256 + tid for c = 0, 1(, 2): they are the OLDER wave of each SIMD, win the MFMA arbitration and would
    // otherwise wait at barrier B1 for waves 4-7 (4.5 in DESIGN.md).  (Loads from clamped indices, stores predicated.)
    auto stage_load_y = [&](int64_t jt, uint4 &yv) { yv = (reinterpret_cast<const uint4 *>(a.Ysb + (jt >> 5) * BLK))[tid & 255]; };
    auto stage_load_yl = [&](int64_t jt, uint4 &yv, uint4 &yv2) {
      yv = (reinterpret_cast<const uint4 *>(a.Ysb + (jt >> 5) * BLK))[256 + (tid & (KB == 1 ? 127 : 255))];
      if (KB == 2) yv2 = (reinterpret_cast<const uint4 *>(a.Ysb + (jt >> 5) * BLK))[512 + (tid & 255)];
    };
    auto stage_load_c = [&](int64_t jt, float4 &cv) {
      const float4 *cb = a.colp + jt;
      const int64_t rem = N - jt;
      const int ncol = rem > BN ? BN : (int)rem;
      cv = cb[tid < ncol ? tid : ncol - 1];
    };
    auto stage_store = [&](int ybuf, int cbuf, int64_t jt, const uint4 &yv, const uint4 &yv1, const uint4 &ylv, const float4 &cv) {
      if (w_lo) {
        // (without GEMM3 there is no barrier B2 to protect a single lo buffer: the idle slab area holds two)
        uint4 *lo_dst = reinterpret_cast<uint4 *>(GY ? Yl : reinterpret_cast<char *>(Sl) + ybuf * IMG);
        reinterpret_cast<uint4 *>(Yi + ybuf * LDSP)[tid] = yv;
        if (KB == 2) {
          reinterpret_cast<uint4 *>(Yi + ybuf * LDSP)[256 + tid] = yv1;
          lo_dst[tid] = ylv;
        } else if (tid < 128) {
          lo_dst[tid] = yv1;
        }
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
    // (BATCH) staging: thread tid takes entry (column tid & 31, slot tid >> 5): a wave writes 32 consecutive words of two slot rows
    const int bte = (tid & 31) * 16 + (tid >> 5);
    auto bt_mu = [&](int64_t jt) -> float { const int64_t j = jt + (bte >> 4); return j < N ? a.colp[j].y : 0.f; };
    auto bt_store = [&](const float2 &dt, float mu) __attribute__((always_inline)) {
      const int o = (bte & 15) * 32 + (bte >> 4);
      Btd[o] = dt.x;
      Btt[o] = dt.y + mu;
    };
    // slab reduction mapping: thread -> float4 f of the [kb][j][32 k] slab; element e = j*Kp + 32 kb + k of the gY tile
    float4 gold;
    PmfDTile<DB> dcur;
    const int ts = tid & (TS - 1);          // (K <= 32: the gY tile has 256 float4, waves 4-7 mirror 0-3 and do not store)
    const bool s_own = tid < TS;
    const int s_so = 4 * ts;
    const int s_e = ((ts % (BN * 8)) / 8) * Kp + 32 * (ts / (BN * 8)) + 4 * (ts % 8);
    auto slab_prefetch = [&](int64_t jt) {
      const float *sb = myslab + jt * Kp;
      const int64_t rem = N - jt;
      const int nel = (rem > BN ? BN : (int)rem) * Kp;
      gold = pmf_load_stream(reinterpret_cast<const float4 *>(sb + (s_e < nel ? s_e : (s_e % Kp))));   // (read once per pass)
    };
    // forward of one tile (12 MFMAs) with the reduction of the previous tile's slabs between them
    auto forward_reduce = [&](f32x16 &acc, int ybuf, int cbuf, bool do_red, int64_t jt_red) {
      const int cb0 = cbuf * BN + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = BATCH ? 0.f : Cmu[cb0 + (r & 3) + 8 * (r >> 2)];   // (mu joins after the batch scale)
      const char *Yc = Yi + ybuf * LDSP;
      float4 racc = make_float4(0.f, 0.f, 0.f, 0.f);
      // the operand reads run one k-step ahead of the MFMAs (two waves per SIMD do not hide an LDS round trip)
      bf16x8 yh = *reinterpret_cast<const bf16x8 *>(Yc + rowoff[0]);
      bf16x8 ym = *reinterpret_cast<const bf16x8 *>(Yc + IMG + rowoff[0]);
      const char *Ylc = GY ? Yl : reinterpret_cast<const char *>(Sl) + ybuf * IMG;
      bf16x8 yl = *reinterpret_cast<const bf16x8 *>(Ylc + rowoff[0]);
      bf16x8 xh = *reinterpret_cast<const bf16x8 *>(Xw + rowoff[0]);
      bf16x8 xm = *reinterpret_cast<const bf16x8 *>(Xw + IMG + rowoff[0]);
#pragma unroll
      for (int S = 0; S < FS; ++S) {
        bf16x8 yhn = yh, ymn = ym, yln = yl, xhn = xh, xmn = xm;
        if (S + 1 < FS) {
          yhn = *reinterpret_cast<const bf16x8 *>(Yc + rowoff[S + 1]);
          ymn = *reinterpret_cast<const bf16x8 *>(Yc + IMG + rowoff[S + 1]);
          yln = *reinterpret_cast<const bf16x8 *>(Ylc + rowoff[S + 1]);
          xhn = *reinterpret_cast<const bf16x8 *>(Xw + rowoff[S + 1]);
          xmn = *reinterpret_cast<const bf16x8 *>(Xw + IMG + rowoff[S + 1]);
        }
        constexpr int SPS = 8 / FS;   // slabs summed per k-step
        float4 sv[SPS];
        if (do_red) {
#pragma unroll
          for (int z = 0; z < SPS; ++z) sv[z] = *reinterpret_cast<const float4 *>(Sl + (SPS * S + z) * SLAB + s_so);
        }
        __builtin_amdgcn_sched_barrier(0);
        // six of the nine partial products: what is dropped (mid*lo, lo*mid, lo*lo) is below 2^-24 of the product, so
        // Z is as accurate as the exact-f32 MFMA's -- which matters because G = w (Z - D) cancels most of Z once the
        // model fits (the two-term split's 4e-6 |Z| became 1e-3 of the gradient in the parity tests)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yl, xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xl[S], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ym, xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(yh, xh, acc, 0, 0, 0);
        if (do_red) {
#pragma unroll
          for (int z = 0; z < SPS; ++z) { racc.x += sv[z].x; racc.y += sv[z].y; racc.z += sv[z].z; racc.w += sv[z].w; }
        }
        yh = yhn; ym = ymn; yl = yln; xh = xhn; xm = xmn;
        __builtin_amdgcn_sched_barrier(0);
      }
      if (do_red) {
        dcur.touch();
        const int64_t rem = N - jt_red;
        const int nel = (rem > BN ? BN : (int)rem) * Kp;
        float *sb = myslab + jt_red * Kp;
        float4 v = racc;
        const float sgj = Csg[(cbuf ^ 1) * BN + s_e / Kp];
        v.x *= sgj; v.y *= sgj; v.z *= sgj; v.w *= sgj;
        if (!slab_first) { v.x += gold.x; v.y += gold.y; v.z += gold.z; v.w += gold.w; }
        if (s_own && s_e < nel) {   // streaming store: the entry is not touched again before the workgroup's next row panel
          const pmf_f32x4 vv = {v.x, v.y, v.z, v.w};
          __builtin_nontemporal_store(vv, reinterpret_cast<pmf_f32x4 *>(sb + s_e));
        }
      }
    };

    uint32_t tflag = a.tflags[(col_begin >> 5) * a.nRB + rb_u];
#pragma unroll
    for (int q = 0; q < PmfDTile<DB>::NCH; ++q) dcur.load(a.D, (col_begin >> 5) * a.nRB + rb_u, lane, q);
    {
      uint4 yv, yv1, ylv;
      float4 cv;
      stage_load_y(col_begin, yv);
      stage_load_yl(col_begin, yv1, ylv);
      stage_load_c(col_begin, cv);
#pragma unroll
      for (int q = 0; q < 4 * KB; ++q) reinterpret_cast<uint4 *>(Xw)[lane + 64 * q] = xv0[q];
      stage_store(0, 0, col_begin, yv, yv1, ylv, cv);
      if (BATCH) {
        // 32 columns x 16 slots = 512 float2: one per thread (first tile: slot map straight from global memory)
        bt_store(pmf_bt_entry(a, a.pm + rp * a.n_bv * 16, col_begin, bte, pmf_bt_view(a, col_begin, bte)), bt_mu(col_begin));
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
      uint4 ynext, ynext1, ylnext;
      float4 cnext;
      float2 btn;     // (BATCH) this thread's entry of the next tile's dense batch table
      float btm = 0.f;  //         and its column's mu
      int btv = 255;
      PMF_STAMP(0);

      // ---- epilogue (identical to pmf_fused_kernel without batch layers): acc becomes G
      float lsum = 0.f;
      const int tkind = MIXED ? __builtin_amdgcn_readfirstlane(Ck[par]) : 0;
      const int tview = BATCH ? __builtin_amdgcn_readfirstlane(Ck[2 + par]) : -1;   // the tile's view; -2: it straddles two
      // General epilogue of one register, given the entry's batch scale dl and shift th = theta + mu_j (batch layers only: without
      // them mu_j was the accumulator's initial value).  Gaussian columns mask by substitution (y := z: d = 0, g = 0, no loss)
      // and sum g d, halved once per tile; all-finite tiles (fast) skip the mask.
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
      auto vmem_op = [&](int i) {
        if (i == 0) { if (BATCH) btv = pmf_bt_view(a, jn, bte); if (w_lo) stage_load_y(jn, ynext); }
        else if (i == 1) { if (w_lo) stage_load_yl(jn, ynext1, ylnext); stage_load_c(jn, cnext); }
        else if (i == 2) { if (GY) slab_prefetch(j0); if (BATCH) { btn = pmf_bt_entry(a, Pm, jn, bte, btv); btm = bt_mu(jn); } }
        else if (i < 7) {
          // streaming load: D is read once, and a default-policy load would push the Y images of the column segment
          // (3.3 MB at K = 64) out of the XCD's 4 MB L2 (measured: -1.3 % kernel time)
          if (i - 3 < PmfDTile<DB>::NCH) dcur.load(a.D, (jn >> 5) * a.nRB + rb_u, lane, i - 3);
        } else {
          tflag = a.tflags[(jn >> 5) * a.nRB + rb_u];
        }
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
            f32x2 dd;
            asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(dd) : "v"(zz), "v"(yy));
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
        // (the mask-free copy exists for the batch variants only: without batch layers an all-finite Gaussian tile took the packed
        // path above, and a second branch on the freshly loaded tile flag here cost the non-batch variant 11 %, measured)
        else if (!MIXED || tkind == 0) { if (BATCH && tile_fast) epi_all(PMF_NOISE_NORMAL, true, true); else epi_all(PMF_NOISE_NORMAL, true, false); }
        else if (tkind == 1) epi_all(PMF_NOISE_BERNOULLI, true, false);
        else if (tkind == 2) epi_all(PMF_NOISE_POISSON, true, false);
        else epi_all(3, true, false);
      }
      lossacc += (double)fmaf(0.5f, lnorm, lsum);
      PMF_STAMP(1);   // epilogue

      // ---- split G into bf16 hi / lo; registers 8S..8S+7 are GEMM2's A fragment of k-step S
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

      PMF_STAMP(2);   // split of G + image writes
      // ---- GEMM2: gX[i,k] += sum_j G[j,i] Ys[k,j]   (A = G registers, B = the Y image read transposed)
      // (operand reads run ahead of the MFMAs: group g = 2S + kb reads group g + 1's fragments first; GEMM3's first
      //  fragments are requested before GEMM2's last MFMAs)
      bf16x8 b2h[2], b2l[2];
      auto g2_read = [&](int g, int slot) __attribute__((always_inline)) {
        const int S = g / KB, kb = g % KB;
        b2h[slot] = pmf_sb_tr8(Yc + y_tr_off(S, 0, kb), Yc + y_tr_off(S, 1, kb));
        b2l[slot] = pmf_sb_tr8(Yc + IMG + y_tr_off(S, 0, kb), Yc + IMG + y_tr_off(S, 1, kb));
      };
      bf16x8 a3h[2], a3l[2], b3h[2], b3l[2];
      auto g3_read_a = [&](int S) __attribute__((always_inline)) {
        a3h[S] = pmf_sb_tr8(Tw + t_tr_off(S, 0), Tw + t_tr_off(S, 1));
        a3l[S] = pmf_sb_tr8(Tw + 2048 + t_tr_off(S, 0), Tw + 2048 + t_tr_off(S, 1));
      };
      auto g3_read_b = [&](int g, int slot) __attribute__((always_inline)) {
        const int S = g / KB, kb = g % KB;
        b3h[slot] = pmf_sb_tr8(Xw + x_tr_off(S, 0, kb), Xw + x_tr_off(S, 1, kb));
        b3l[slot] = pmf_sb_tr8(Xw + IMG + x_tr_off(S, 0, kb), Xw + IMG + x_tr_off(S, 1, kb));
      };
      if (GX) g2_read(0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const int S = g / KB, kb = g % KB;
        if (g + 1 < NG) { if (GX) g2_read(g + 1, (g + 1) & 1); }
        else if (GY) { g3_read_a(0); g3_read_b(0, 0); }
        constexpr int OPG = 8 / NG;   // the tile's global loads, spread over the groups
#pragma unroll
        for (int z = 0; z < OPG; ++z) vmem_op(OPG * g + z);
        __builtin_amdgcn_sched_barrier(0);
        if (GX) {
          gx[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gl[S], b2h[g & 1], gx[kb], 0, 0, 0);
          gx[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[S], b2l[g & 1], gx[kb], 0, 0, 0);
          gx[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gh[S], b2h[g & 1], gx[kb], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }

      PMF_STAMP(3);   // GEMM2
      // ---- GEMM3: gY[j,k] = sum_i G[j,i] X[k,i] over the wave's 32 rows (A = T transposed, B = X image transposed)
      if (GY) {
        f32x16 gy[KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) gy[kb][r] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          const int S = g / KB, kb = g % KB;
          if (g + 1 < NG) {
            if (g == 0) g3_read_a(1);
            g3_read_b(g + 1, (g + 1) & 1);
          }
          __builtin_amdgcn_sched_barrier(0);
          gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3l[S], b3h[g & 1], gy[kb], 0, 0, 0);
          gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3h[S], b3l[g & 1], gy[kb], 0, 0, 0);
          gy[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3h[S], b3h[g & 1], gy[kb], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
        // the slab's last k block aliases the G image: written last, after every read of it has been issued (in-order LDS)
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
          for (int r = 0; r < 16; ++r) Sw[kb * 1024 + pmf_rowmap(r, h) * 32 + l31] = gy[kb][r];
      }

      // ---- publish Y(t+1) into the other buffer; B1 also completes this tile's slabs
      PMF_STAMP(4);   // GEMM3 + slab writes
      stage_store(par ^ 1, par ^ 1, jn, ynext, ynext1, ylnext, cnext);
      PMF_STAMP(5);   // stage_store
      __syncthreads();                 // B1
      PMF_STAMP(6);   // B1 wait
      if (BATCH) bt_store(btn, btm);        // every wave is past its epilogue(t): the single table buffer takes tile t+1 (read after B2)

      slab_first = pidx == 0 || (pidx == 1 && ti0 + t < t0_first);
      forward_reduce(acc, par ^ 1, par ^ 1, GY, j0);
      PMF_STAMP(8);   // forward + slab reduce
      if (GY || BATCH) __syncthreads();   // B2: slabs, G images and the batch table are free again
      PMF_STAMP(9);   // B2 wait
    }
    PMF_STAMP(10);

    // ---- flush gX (lane = factor index k, register = row): plain stores to the piece's own slot (see pmf_fused_kernel)
    if (GX) {
      float *gp = a.gx_part + (int64_t)gx_slot * a.gx_slot_stride + (int64_t)w * 32 * Kp + l31;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) gp[pmf_rowmap(r, h) * Kp + 32 * kb] = gx[kb][r];
    }
    ++gx_slot;
    PMF_STAMP(11);  // piece prologue + gX flush
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
