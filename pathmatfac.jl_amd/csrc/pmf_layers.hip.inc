// pmf_layers.hip.inc -- the layer-parameter pass (included by pmf_k_layers.hip).
//
// Epochs that train only the column layers (init_mu!, init_theta!, the batch-effect fits: src/fit.jl:82-122, 378-496)
// need, per column j and row batch b of j's view, S_G[b,j] = sum_{i in b} g_ij and S_Q[b,j] = sum_{i in b} g_ij z1_ij
// (g = dloss/dz, z1 = sigma_j * a_ij), from which every layer gradient follows (k_layer_map):
//   grad mu_j = sum_b S_G ; grad theta[b,j] = S_G[b,j] ; grad logdelta[b,j] = delta_bj S_Q[b,j] ;
//   grad logsigma_j = sigma_j sum_b delta_bj S_G[b,j]            (as coded in the reference, SURVEY Q1)
// i.e. the BatchArray scatter-adds of src/batch_array.jl:136-147, 192-209 as column sums segmented by row batch.
//
// Structure (gfx950): a workgroup of 8 waves owns PMF_LS = 2 column tiles (64 columns) and a range of row panels.
// The sigma-scaled Y tiles, their column parameters and their dense batch tables are staged in LDS ONCE per unit;
// inside the row sweep every wave works alone (no workgroup barrier): its 32 rows of X go through registers into a
// private LDS panel, the forward is K/2 v_mfma_f32_32x32x2_f32 per tile, the general
// epilogue produces G and Q in the accumulator layout (lane = row), both are transposed through a private LDS tile so
// that lane = column, and each lane adds its 16 rows to RUNNING sums that live in registers across the row sweep and
// are flushed only when the row batch changes or the unit ends.  D is read once.
// No float atomics: a flush is a plain read-modify-write of a table PRIVATE to (row range of the unit, wave, lane half)
// -- exactly one lane ever touches an entry, in program order -- and k_layer_map adds the tables in a fixed order, so
// the layer gradients are bitwise reproducible run to run (as the loss, grad(X) and grad(Y) are).

template <int KB, int NW>
struct LayerCfg {
  static constexpr int Kp = 32 * KB, KpS = Kp + 4, YT = PMF_BN * KpS, XP = 32 * KpS;
  static constexpr size_t lds(int nbs) {   // nbs = slots per column of the batch table (16, or more for views with > 15 batches)
    return sizeof(float) * (PMF_LS * YT + NW * XP + NW * 1024) + sizeof(float) * 4 * PMF_LS * 32 +
           sizeof(float2) * PMF_LS * 32 * nbs + NW * 512 + sizeof(double) * NW;
  }
};

// NW = 8 waves (two per SIMD, 256 registers) for K <= 64; 4 waves (one per SIMD, the whole register file) for K <= 128,
// whose X panels would not fit in LDS eight times.
// WIDE: more than 16 slots per column in the batch table (views with > 15 batches); the common 16-slot case keeps
// compile-time strides (the run-time shift costs 24 registers, which the 8-wave variants do not have).
template <int KB, int NW, bool MIXED, bool DB, bool WIDE>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void pmf_layer_kernel(const LayerPassArgs a) {
  using Cfg = LayerCfg<KB, NW>;
  constexpr int NT = 64 * NW;
  constexpr int Kp = Cfg::Kp, KpS = Cfg::KpS, KS = Kp / 2, BN = PMF_BN, LS = PMF_LS;
  constexpr int XV = (32 * Kp / 4) / 64;   // float4 of a 32-row X panel per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Ys = reinterpret_cast<float *>(smem);                 // [LS][BN*KpS]  sigma_j * Y[k,j]
  float *Xs = Ys + LS * Cfg::YT;                               // [NW][32*KpS]
  float *Tt = Xs + NW * Cfg::XP;                               // [NW][1024] transposed tile (G, then Q)
  float *Cmu = Tt + NW * 1024;                                 // [LS][32] mu_j, w_j, meta_j (structure of arrays: 16-B reads per 4 columns)
  float *Cw = Cmu + LS * 32;
  int *Cmt = reinterpret_cast<int *>(Cw + LS * 32);
  const int bsh = WIDE ? a.nbs_shift : 4, ident = (1 << bsh) - 1;   // batch-table slots per column; the last one is the identity
  float2 *Bt = reinterpret_cast<float2 *>(Cmt + 2 * LS * 32);  // [LS][32][nbs] {delta, theta}   (the fourth array slot keeps the 16-B layout of LayerCfg)
  unsigned char *Bw = reinterpret_cast<unsigned char *>(Bt + ((LS * 32) << bsh)) + (threadIdx.x >> 6) * 512;   // this wave: [16][32] batch of every row
  double *red = reinterpret_cast<double *>(reinterpret_cast<unsigned char *>(Bt + ((LS * 32) << bsh)) + NW * 512);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  float *Xw = Xs + w * Cfg::XP, *T = Tt + w * 1024;
  double lossacc = 0.0;

  const int n_units = a.n_seg * a.R;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int sg = u / a.R, rr = u - sg * a.R;
    const int ct0 = sg * LS;
    const int nt = a.n_ct - ct0 < LS ? a.n_ct - ct0 : LS;
    const int64_t rp_lo = (int64_t)rr * a.n_rp / a.R, rp_hi = (int64_t)(rr + 1) * a.n_rp / a.R;
    float2 *LGp = a.LG + ((int64_t)(rr * NW + w) * 2 + h) * a.lg_stride;   // this lane's private table
    __syncthreads();   // the previous unit is done with the shared tiles
    // ---- stage the unit's Y tiles (scaled by sigma_j), column parameters and batch tables
    for (int e4 = tid; e4 < nt * (BN * Kp / 4); e4 += NT) {
      const int t = e4 / (BN * Kp / 4), r4 = e4 - t * (BN * Kp / 4);
      const int jl = (r4 * 4) / Kp, kf = (r4 * 4) % Kp;
      const int64_t j = (int64_t)(ct0 + t) * BN + jl;
      float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < N) {
        const float sgm = a.colp[j].x;
        y = *reinterpret_cast<const float4 *>(a.Y + j * Kp + kf);
        y.x *= sgm; y.y *= sgm; y.z *= sgm; y.w *= sgm;
      }
      *reinterpret_cast<float4 *>(Ys + t * Cfg::YT + jl * KpS + kf) = y;
    }
    for (int c = tid; c < nt * 32; c += NT) {
      const int64_t j = (int64_t)ct0 * BN + c;
      const float4 cp = j < N ? a.colp[j] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));   // pad column: meta < 0 (no view, masked below)
      Cmu[c] = cp.y; Cw[c] = cp.z; Cmt[c] = __float_as_int(cp.w);
    }
    for (int e = tid; e < ((nt * 32) << bsh); e += NT)
      Bt[e] = a.btd ? a.btd[(((int64_t)ct0 * BN) << bsh) + e] : make_float2(1.f, 0.f);
    // running sums of this lane's COLUMN (l31 of every tile) over this lane's half of the rows, per tile
    int cb[LS], cq[LS];   // batch of the rows summed so far (one tracker per sum: the two passes run separately)
    float sG[LS], sQ[LS];
#pragma unroll
    for (int t = 0; t < LS; ++t) { cb[t] = -1; cq[t] = -1; sG[t] = 0.f; sQ[t] = 0.f; }
    __syncthreads();

    auto load_x = [&](int64_t rp, float4 (&xr)[XV]) {
      const int64_t row0 = rp * (32 * NW) + (int64_t)w * 32;
      const float *xsrc = a.X + row0 * Kp;
#pragma unroll
      for (int q = 0; q < XV; ++q) {
        const int e4 = lane + 64 * q;
        const int il = (e4 * 4) / Kp;
        xr[q] = row0 + il < M ? *reinterpret_cast<const float4 *>(xsrc + e4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    auto load_d = [&](int64_t rp, int t, PmfDTile<DB> &d) {
      int64_t rb = rp * NW + w;
      if (rb >= a.nRB) rb = a.nRB - 1;
      // (streaming loads: D is read once per epoch; keep it from displacing X, re-read by every unit, in L2)
#pragma unroll
      for (int q = 0; q < PmfDTile<DB>::NCH; ++q) d.load(a.D, (int64_t)(ct0 + t) * a.nRB + rb, lane, q);
    };

    float4 xr[XV];
    PmfDTile<DB> dcur;
    constexpr bool XPF = NW == 4;   // one wave per SIMD: 512 registers, room to prefetch the next X panel (with two waves per SIMD it spills: 13.5 -> 19.4 ms)
    if (rp_lo < rp_hi) { load_d(rp_lo, 0, dcur); if (XPF) load_x(rp_lo, xr); }
    for (int64_t rp = rp_lo; rp < rp_hi; ++rp) {
      const int64_t row0 = rp * (32 * NW) + (int64_t)w * 32;
      const int64_t irow = row0 + l31;
      const bool row_ok = irow < M;
      const int64_t irow_c = row_ok ? irow : M - 1;
      // ---- this wave's X panel: registers -> private LDS panel; prefetch the next one
      __builtin_amdgcn_wave_barrier();
      if (!XPF) load_x(rp, xr);
#pragma unroll
      for (int q = 0; q < XV; ++q) {
        const int e4 = lane + 64 * q;
        *reinterpret_cast<float4 *>(Xw + ((e4 * 4) / Kp) * KpS + (e4 * 4) % Kp) = xr[q];
      }
      if (a.n_bv > 0 && h == 0)
        for (int v = 0; v < a.n_bv; ++v) {
          const int b = a.bor[(int64_t)v * M + irow_c];
          Bw[v * 32 + l31] = (unsigned char)(b < 0 || b >= ident ? ident : b);
        }
      __builtin_amdgcn_wave_barrier();
      if (XPF && rp + 1 < rp_hi) load_x(rp + 1, xr);
#pragma unroll
      for (int t = 0; t < LS; ++t) {
        if (t >= nt) break;
        // ---- forward: z1[j,i] = sum_k sigma_j Y[k,j] X[k,i]
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
          const float4 *yr = reinterpret_cast<const float4 *>(Ys + t * Cfg::YT + l31 * KpS + h * (Kp / 2));
          const float4 *xq = reinterpret_cast<const float4 *>(Xw + l31 * KpS + h * (Kp / 2));
#pragma unroll
          for (int q = 0; q < KS / 4; ++q) {
            const float4 yv = yr[q], xv = xq[q];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.x, xv.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.y, xv.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.z, xv.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yv.w, xv.w, acc, 0, 0, 0);
          }
        }
        // ---- epilogue in the accumulator layout (lane = row, register = column): acc <- g, qv <- g * z1
        f32x16 qv;
        float lsum = 0.f;
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
          // four consecutive columns jl = 8 c4 + 4 h + u: their parameters are one 16-B read per array
          const int jb = t * 32 + 8 * c4 + 4 * h;
          const float4 mu4 = *reinterpret_cast<const float4 *>(Cmu + jb);
          const float4 w4 = *reinterpret_cast<const float4 *>(Cw + jb);
          const int4 mt4 = *reinterpret_cast<const int4 *>(Cmt + jb);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = 4 * c4 + u;
            const int meta = u == 0 ? mt4.x : (u == 1 ? mt4.y : (u == 2 ? mt4.z : mt4.w));
            const float muj = u == 0 ? mu4.x : (u == 1 ? mu4.y : (u == 2 ? mu4.z : mu4.w));
            const float wj = u == 0 ? w4.x : (u == 1 ? w4.y : (u == 2 ? w4.z : w4.w));
            const int v = (meta >> 2) - 1;
            const int b = a.n_bv > 0 ? Bw[(v < 0 ? 0 : v) * 32 + l31] : ident;
            const float2 dt = Bt[((jb + u) << bsh) + b];
            const float z1 = acc[r];
            const float z = fmaf(z1, dt.x, muj + dt.y);
            const float y = dcur.get(r);
            float l, g;
            if (MIXED) pmf_noise(meta & 3, z, y, wj, a.htab + ((int64_t)(ct0 + t) * BN + 4 * h) * PMF_HT + PMF_HT * (8 * c4 + u), l, g);
            else pmf_noise(PMF_NOISE_NORMAL, z, y, wj, nullptr, l, g);
            const bool ok = pmf_finite(y) && row_ok && meta >= 0;   // (meta < 0: a pad column)
            lsum += ok ? l : 0.f;
            g = ok ? g : 0.f;
            acc[r] = g;
            qv[r] = g * z1;
          }
          __builtin_amdgcn_sched_barrier(0);   // keep the chunks apart: hoisting all 16 columns' parameters costs 80 registers
        }
        lossacc += (double)lsum;
        // the D registers are dead: fetch the next tile (same rows, next column tile; or the next row panel's first
        // tile) -- it lands under the transposes, the sums and the next forward
        if (t + 1 < nt) load_d(rp, t + 1, dcur);
        else if (rp + 1 < rp_hi) load_d(rp + 1, 0, dcur);
        // ---- transpose G, then Q, through the wave's LDS tile: lane (j = l31, h) gets rows i = 2s + h and adds them
        //      to the running sums of column j, segmented by the row batch of j's view
        const int vj = (Cmt[t * 32 + l31] >> 2) - 1;
        const unsigned char *bwj = Bw + (vj < 0 ? 0 : vj) * 32;
        // Rows are normally sorted by batch, so a lane's 16 rows of one tile almost always share one batch: that case
        // (checked once per tile for the whole wave) is 16 adds and one comparison; otherwise row by row.
        const int b0 = a.n_bv > 0 ? bwj[h] : ident;
        int uni = 1;
        if (a.n_bv > 0) {
#pragma unroll
          for (int s = 1; s < 16; ++s) uni &= (bwj[2 * s + h] == b0) ? 1 : 0;
        }
        const bool fast = __all(uni) != 0;   // wave-uniform
        auto segmented = [&](const f32x16 &src, int &cbt, float &st, bool is_q) __attribute__((always_inline)) {
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4)
            *reinterpret_cast<float4 *>(T + l31 * 32 + 4 * ((2 * c4 + h) ^ (l31 & 7))) =
                make_float4(src[4 * c4], src[4 * c4 + 1], src[4 * c4 + 2], src[4 * c4 + 3]);
          __builtin_amdgcn_wave_barrier();
          const int64_t j = (int64_t)(ct0 + t) * BN + l31;
          if (fast) {
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int s = 0; s < 16; s += 2) {
              const int i0 = 2 * s + h, i1 = 2 * s + 2 + h;
              s0 += T[i0 * 32 + 4 * ((l31 >> 2) ^ (i0 & 7)) + (l31 & 3)];
              s1 += T[i1 * 32 + 4 * ((l31 >> 2) ^ (i1 & 7)) + (l31 & 3)];
            }
            if (b0 != cbt) {
              if (j < N && cbt >= 0) { float *dst = is_q ? &LGp[(j << bsh) + cbt].y : &LGp[(j << bsh) + cbt].x; *dst += st; }
              cbt = b0;
              st = 0.f;
            }
            st += s0 + s1;
          } else {
#pragma unroll 1
            for (int s = 0; s < 16; ++s) {   // rare: re-read the tile row by row (no register array)
              const int i = 2 * s + h;
              const float v = T[i * 32 + 4 * ((l31 >> 2) ^ (i & 7)) + (l31 & 3)];
              const int bi = bwj[i];
              if (bi != cbt) {
                if (j < N && cbt >= 0) { float *dst = is_q ? &LGp[(j << bsh) + cbt].y : &LGp[(j << bsh) + cbt].x; *dst += st; }
                cbt = bi;
                st = 0.f;
              }
              st += v;
            }
          }
        };
        segmented(acc, cb[t], sG[t], false);
        segmented(qv, cq[t], sQ[t], true);
      }
    }
#pragma unroll
    for (int t = 0; t < LS; ++t)
      if (t < nt) {
        const int64_t j = (int64_t)(ct0 + t) * BN + l31;
        if (j < N && cb[t] >= 0) LGp[(j << bsh) + cb[t]].x += sG[t];
        if (j < N && cq[t] >= 0) LGp[(j << bsh) + cq[t]].y += sQ[t];
      }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) lossacc += __shfl_xor(lossacc, off, 64);
  __syncthreads();
  if (lane == 0) red[w] = lossacc;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int q = 0; q < NW; ++q) s += red[q];
    if (a.loss_partial) a.loss_partial[blockIdx.x] = s;
  }
}

// The private tables of the layer pass, added in table order into table 0 (thread = one {S_G, S_Q} entry; consecutive
// threads read consecutive entries of every table): a fixed summation order, bitwise reproducible.
__global__ __launch_bounds__(256) void k_layer_reduce(float2 *LG, int64_t lg_stride, int n_parts) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= lg_stride) return;
  float2 t = LG[e];
  for (int p = 1; p < n_parts; ++p) { const float2 v = LG[(int64_t)p * lg_stride + e]; t.x += v.x; t.y += v.y; }
  LG[e] = t;
}

// LG (table 0 after k_layer_reduce) -> the four layer gradients (one thread per column; written, not accumulated)

__global__ void k_layer_map(const LayerMapArgs a) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= a.N) return;
  const float4 cp = a.colp[j];
  const int v = (__float_as_int(cp.w) >> 2) - 1;
  float smu = 0.f, sls = 0.f;
  const int bsh = a.nbs_shift;
  for (int s = 0; s < (1 << bsh); ++s) {
    const float2 e = a.LG[(j << bsh) + s];
    const float dl = a.btd ? a.btd[(j << bsh) + s].x : 1.f;
    smu += e.x;
    sls += e.x * dl;
  }
  if (a.g_mu) a.g_mu[j] = smu;
  if (a.g_logsigma) a.g_logsigma[j] = sls * cp.x;
  if (v >= 0) {
    const ViewDesc vd = a.views[v];
    for (int b = 0; b < vd.nb; ++b) {
      const int64_t e = a.val_off[v] + (j - vd.c0) * vd.nb + b;
      const float2 s = a.LG[(j << bsh) + b];
      if (a.g_theta) a.g_theta[e] = s.x;
      if (a.g_logdelta) a.g_logdelta[e] = s.y * a.btd[(j << bsh) + b].x;
    }
  }
}
