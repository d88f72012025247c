// pmf_thresh.hip.inc -- the threshold pass of the squared-hinge noise models (included by pmf_k_thresh.hip).
//
// Per kind-3 column j and threshold m = 0..2 (include/pmf_hip_thresholds.h):
//   g_t[m][j] = sum_i w_j (a_ij [c_ij = m + 1] - b_ij [c_ij = m])
// with a, b the two margin violations of pmf_hinge_terms at z = z1 delta + mu + theta: an entry of class c adds w a to the
// threshold below its bin (t_{c-1}) and takes w b from the one above it (t_c).  An infinite bound's term is 0 by the
// column's table, so an infinite threshold collects exact zeros.
//
// Structure (gfx950), modelled on the layer pass (pmf_layers.hip.inc): a unit is ONE column tile of the host's list of
// tiles that hold a kind-3 column, times one range of row panels.  The sigma-scaled Y tile, its column parameters and its
// dense batch table are staged in LDS once per unit; inside the row sweep every wave works alone: its 32 rows of X go
// through registers into a private LDS panel, the forward is K/2 v_mfma_f32_32x32x2_f32, and the epilogue runs in the
// accumulator layout (lane = row, register = column): each lane keeps 16 columns x 3 thresholds of RUNNING sums in
// registers across the unit's row sweep.  At the end of the unit the sums are joined over the 32 row lanes by a fixed
// butterfly and stored to a slot private to (row range, wave, tile); k_thresh_cols adds the slots of a column in a fixed
// order in float64, k_thresh_groups the columns of a group.  No float atomics: bitwise the same run to run.
// Ragged rows (row_ok), pad columns (meta < 0) and the columns of other kinds inside a tile contribute nothing.

template <int KB, int NW>
struct ThreshCfg {
  static constexpr int Kp = 32 * KB, KpS = Kp + 4, YT = PMF_BN * KpS, XP = 32 * KpS;
  static constexpr size_t lds(int nbs) {
    return sizeof(float) * (YT + NW * XP) + sizeof(float) * 4 * 32 + sizeof(float) * 32 * PMF_HT + sizeof(float2) * 32 * nbs + NW * 512;
  }
};

template <int KB, int NW, bool DB, bool WIDE>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void pmf_thresh_kernel(const ThreshPassArgs a) {
  using Cfg = ThreshCfg<KB, NW>;
  constexpr int NT = 64 * NW;
  constexpr int Kp = Cfg::Kp, KpS = Cfg::KpS, KS = Kp / 2, BN = PMF_BN;
  constexpr int XV = (32 * Kp / 4) / 64;   // float4 of a 32-row X panel per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Ys = reinterpret_cast<float *>(smem);                 // [BN*KpS]  sigma_j * Y[k,j]
  float *Xs = Ys + Cfg::YT;                                    // [NW][32*KpS]
  float *Cmu = Xs + NW * Cfg::XP;                              // [32] mu_j, w_j, meta_j (+ one spare array: 16-B layout)
  float *Cw = Cmu + 32;
  int *Cmt = reinterpret_cast<int *>(Cw + 32);
  const int bsh = WIDE ? a.nbs_shift : 4, ident = (1 << bsh) - 1;
  float *Ht = reinterpret_cast<float *>(Cmt + 2 * 32);         // [32][PMF_HT] the columns' tables of class bounds
  float2 *Bt = reinterpret_cast<float2 *>(Ht + 32 * PMF_HT);   // [32][nbs] {delta, theta}
  unsigned char *Bw = reinterpret_cast<unsigned char *>(Bt + (32 << bsh)) + (threadIdx.x >> 6) * 512;   // this wave: [16][32] batch of every row

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  float *Xw = Xs + w * Cfg::XP;

  const int n_units = a.n_tiles * a.R;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int ti = u / a.R, rr = u - ti * a.R;
    const int ct = a.tiles[ti];
    const int64_t rp_lo = (int64_t)rr * a.n_rp / a.R, rp_hi = (int64_t)(rr + 1) * a.n_rp / a.R;
    __syncthreads();   // the previous unit is done with the shared tile
    for (int e4 = tid; e4 < BN * Kp / 4; e4 += NT) {
      const int jl = (e4 * 4) / Kp, kf = (e4 * 4) % Kp;
      const int64_t j = (int64_t)ct * BN + jl;
      float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < N) {
        const float sgm = a.colp[j].x;
        y = *reinterpret_cast<const float4 *>(a.Y + j * Kp + kf);
        y.x *= sgm; y.y *= sgm; y.z *= sgm; y.w *= sgm;
      }
      *reinterpret_cast<float4 *>(Ys + jl * KpS + kf) = y;
    }
    if (tid < 32) {
      const int64_t j = (int64_t)ct * BN + tid;
      const float4 cp = j < N ? a.colp[j] : make_float4(0.f, 0.f, 0.f, __int_as_float(-1));   // pad column: meta < 0
      Cmu[tid] = cp.y; Cw[tid] = cp.z; Cmt[tid] = __float_as_int(cp.w);
    }
    if (tid >= 64 && tid < 64 + 32 * PMF_HT / 4)   // (the table array is padded like D: a ragged tile reads in range)
      reinterpret_cast<float4 *>(Ht)[tid - 64] = reinterpret_cast<const float4 *>(a.htab + (int64_t)ct * BN * PMF_HT)[tid - 64];
    for (int e = tid; e < (32 << bsh); e += NT)
      Bt[e] = a.btd ? a.btd[(((int64_t)ct * BN) << bsh) + e] : make_float2(1.f, 0.f);
    // running sums of this lane's ROW half: register r = column pmf_rowmap(r, h) of the tile, three thresholds each
    if (a.n_bv == 0 && h == 0) Bw[l31] = (unsigned char)ident;   // without batch views every row reads the identity slot
    float s0[16], s1[16], s2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { s0[r] = 0.f; s1[r] = 0.f; s2[r] = 0.f; }
    __syncthreads();

    auto load_d = [&](int64_t rp, PmfDTile<DB> &d) {
      int64_t rb = rp * NW + w;
      if (rb >= a.nRB) rb = a.nRB - 1;   // (a wave past the last row block re-reads it; its rows are masked by row_ok)
#pragma unroll
      for (int q = 0; q < PmfDTile<DB>::NCH; ++q) d.load(a.D, (int64_t)ct * a.nRB + rb, lane, q);
    };
    PmfDTile<DB> dcur;
    constexpr bool DPF = NW == 4;   // four waves prefetch the next D tile a whole iteration ahead; eight have no registers to hold it across the X staging
    if (DPF && rp_lo < rp_hi) load_d(rp_lo, dcur);
    for (int64_t rp = rp_lo; rp < rp_hi; ++rp) {
      const int64_t row0 = rp * (32 * NW) + (int64_t)w * 32;
      const int64_t irow = row0 + l31;
      const bool row_ok = irow < M;
      const int64_t irow_c = row_ok ? irow : M - 1;
      __builtin_amdgcn_wave_barrier();
      // this wave's 32 rows of X: registers -> its private LDS panel.  A row past M reads row M - 1: in range, and masked by
      // row_ok in the epilogue (no branch per load).
      {
        float4 xr[XV];
#pragma unroll
        for (int q = 0; q < XV; ++q) {
          const int e4 = lane + 64 * q;
          const int64_t row = row0 + (e4 * 4) / Kp;
          xr[q] = *reinterpret_cast<const float4 *>(a.X + (row < M ? row : M - 1) * Kp + (e4 * 4) % Kp);
        }
#pragma unroll
        for (int q = 0; q < XV; ++q) {
          const int e4 = lane + 64 * q;
          *reinterpret_cast<float4 *>(Xw + ((e4 * 4) / Kp) * KpS + (e4 * 4) % Kp) = xr[q];
        }
      }
      if (a.n_bv > 0 && h == 0)
        for (int v = 0; v < a.n_bv; ++v) {
          const int b = a.bor[(int64_t)v * M + irow_c];
          Bw[v * 32 + l31] = (unsigned char)(b < 0 || b >= ident ? ident : b);
        }
      __builtin_amdgcn_wave_barrier();
      if (!DPF) load_d(rp, dcur);   // (lands under the forward)
      // ---- forward: z1[j,i] = sum_k sigma_j Y[k,j] X[k,i]
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      // (the Y fragments do not change along the row sweep: four waves, with 512 registers each, keep them in registers; eight
      //  waves have 256 and re-read them from LDS)
      if (NW == 8) PMF_SCHED_FENCE();
      {
        const float4 *yr = reinterpret_cast<const float4 *>(Ys + l31 * KpS + h * (Kp / 2));
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
      // ---- epilogue in the accumulator layout (lane = row, register = column)
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        PMF_SCHED_FENCE();   // the column parameters are re-read from LDS here: hoisted out of the row sweep they cost 48 registers
        const int jb = 8 * c4 + 4 * h;   // four consecutive columns jl = jb + u: their parameters are one 16-B read per array
        const float4 mu4 = *reinterpret_cast<const float4 *>(Cmu + jb);
        const float4 w4 = *reinterpret_cast<const float4 *>(Cw + jb);
        const int4 mt4 = *reinterpret_cast<const int4 *>(Cmt + jb);
#pragma unroll
        for (int u4 = 0; u4 < 4; ++u4) {
          const int r = 4 * c4 + u4;
          const int meta = u4 == 0 ? mt4.x : (u4 == 1 ? mt4.y : (u4 == 2 ? mt4.z : mt4.w));
          const float muj = u4 == 0 ? mu4.x : (u4 == 1 ? mu4.y : (u4 == 2 ? mu4.z : mu4.w));
          const float wj = u4 == 0 ? w4.x : (u4 == 1 ? w4.y : (u4 == 2 ? w4.z : w4.w));
          const int v = (meta >> 2) - 1;
          const int b = Bw[(v < 0 ? 0 : v) * 32 + l31];   // (no branch on n_bv here: control flow inside the epilogue lets the compiler merge the 16 columns' arithmetic, with every column's operands live at once)
          const float2 dt = Bt[((jb + u4) << bsh) + b];
          const float z = fmaf(acc[r], dt.x, muj + dt.y);
          const float y = dcur.get(r);
          float ta, tb;
          pmf_hinge_terms(z, y, Ht + (jb + u4) * PMF_HT, ta, tb);
          const int c = (int)fminf(fmaxf(y + 0.5f, 0.f), 3.f);
          const bool ok = pmf_finite(y) && row_ok && meta >= 0 && (meta & 3) == PMF_NOISE_SQ_HINGE;
          const float wa = ok ? wj * ta : 0.f, wb = ok ? wj * tb : 0.f;
          s0[r] += (c == 1 ? wa : 0.f) - (c == 0 ? wb : 0.f);
          s1[r] += (c == 2 ? wa : 0.f) - (c == 1 ? wb : 0.f);
          s2[r] += (c == 3 ? wa : 0.f) - (c == 2 ? wb : 0.f);
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the chunks apart (as the layer pass: hoisted parameters cost registers)
      }
      if (DPF && rp + 1 < rp_hi) load_d(rp + 1, dcur);
    }
    // ---- join the 32 row lanes of each half by a fixed butterfly; lane 0 / 32 stores its half's 16 columns
    float *slot = a.slots + ((int64_t)(rr * NW + w) * a.n_tiles + ti) * PMF_TSLOT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v0 = s0[r], v1 = s1[r], v2 = s2[r];
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) {
        v0 += __shfl_xor(v0, off, 64);
        v1 += __shfl_xor(v1, off, 64);
        v2 += __shfl_xor(v2, off, 64);
      }
      if (l31 == 0) {
        const int jl = pmf_rowmap(r, h);
        slot[jl * 3 + 0] = v0; slot[jl * 3 + 1] = v1; slot[jl * 3 + 2] = v2;
      }
    }
  }
}

// The slots of a column, added in slot order (row range, then wave) in float64: one thread per (tile, column, threshold).
// An infinite threshold gets exactly 0 (the columns of the other kinds inside a tile collected zeros).
__global__ __launch_bounds__(256) void k_thresh_cols(const ThreshReduceArgs a) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= (int64_t)a.n_tiles * PMF_TSLOT) return;
  const int ti = (int)(e / PMF_TSLOT), q = (int)(e - (int64_t)ti * PMF_TSLOT);
  const int64_t j = (int64_t)a.tiles[ti] * PMF_BN + q / 3;
  if (j >= a.N) return;
  const int m = q % 3;
  double s = 0.0;
  for (int p = 0; p < a.n_parts; ++p) s += (double)a.slots[((int64_t)p * a.n_tiles + ti) * PMF_TSLOT + q];
  const float4 t = a.thr[j];
  const float tm = m == 0 ? t.x : (m == 1 ? t.y : t.z);
  a.gcol[3 * j + m] = pmf_finite(tm) ? s : 0.0;
}

// G[r][m]: the columns of group r in ascending order, float64.  One workgroup per group: thread t adds a contiguous run of
// columns, thread 0 the 256 runs in order -- a fixed association.
__global__ __launch_bounds__(256) void k_thresh_groups(const ThreshReduceArgs a) {
  __shared__ double sh[3][256];
  const int r = blockIdx.x;
  const int64_t c0 = a.g_c0[r], n = a.g_c1[r] - c0;
  const int64_t per = (n + 255) / 256;
  const int64_t lo = c0 + threadIdx.x * per, hi = lo + per < c0 + n ? lo + per : c0 + n;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  for (int64_t j = lo; j < hi; ++j) { v0 += a.gcol[3 * j]; v1 += a.gcol[3 * j + 1]; v2 += a.gcol[3 * j + 2]; }
  sh[0][threadIdx.x] = v0; sh[1][threadIdx.x] = v1; sh[2][threadIdx.x] = v2;
  __syncthreads();
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int q = 0; q < 256; ++q) s += sh[threadIdx.x][q];
    a.G[3 * r + threadIdx.x] = s;
  }
}

// One thread per group: the optimizer step of its finite thresholds (the expressions of k_reg_step, no regularizer), then
// the order clamp.  An infinite threshold is not stepped and its state does not move.
__global__ __launch_bounds__(64) void k_thresh_step(const ThreshStepArgs a) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_groups) return;
  float t[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int e = 3 * r + m;
    float p = a.t[e];
    if (pmf_finite(p)) {
      const float g = (float)a.G[e];
      if (a.opt_kind == PMF_OPT_ADAGRAD) {
        const float acc = a.acc[e] + g * g;
        a.acc[e] = acc;
        p -= g * (a.lr / (sqrtf(acc) + a.eps));
      } else {
        const float mm = a.b1 * a.mom[e] + (1.f - a.b1) * g;
        const float v = a.b2 * a.acc[e] + (1.f - a.b2) * g * g;
        a.mom[e] = mm;
        a.acc[e] = v;
        p -= mm / a.c1 / (sqrtf(v / a.c2) + a.eps) * a.lr;
      }
    }
    t[m] = p;
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
    if (pmf_finite(t[m]) && pmf_finite(t[m + 1]) && t[m + 1] < t[m]) t[m + 1] = t[m];
#pragma unroll
  for (int m = 0; m < 3; ++m) a.t[3 * r + m] = t[m];
}

// The per-column images of the groups' columns from the groups' triples: the values the host writes for the same triple
// (hinge_table / upload_thresholds, pmf_hip.hip) -- selects and copies only, so the bits are the same.
__global__ __launch_bounds__(256) void k_thresh_images(const ThreshImageArgs a) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= a.N) return;
  const int r = a.col_group[j];
  if (r < 0) return;
  const float t[3] = {a.t[3 * r], a.t[3 * r + 1], a.t[3 * r + 2]};
  a.thr[j] = make_float4(t[0], t[1], t[2], 0.f);
  float *T = a.htab + j * PMF_HT;
  T[0] = -INFINITY;
  T[7] = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const bool inf = !pmf_finite(t[k]);
    T[1 + k] = inf ? -INFINITY : t[k];
    T[4 + k] = inf ? INFINITY : t[k];
  }
}

// Class counts: one wave per (64 columns, chunk of rows); thread = column.  Every thread counts the observed entries of its
// column by class, then for every range that holds the column the wave's counts are joined and added by one 64-bit integer
// atomic per class: exact whatever the order.
__global__ __launch_bounds__(64) void k_class_counts(const ClassCountArgs a) {
  const int64_t j = blockIdx.x * 64ll + threadIdx.x;
  const int64_t rows = (a.M + a.row_chunks - 1) / a.row_chunks;
  const int64_t i0 = blockIdx.y * rows, i1 = i0 + rows < a.M ? i0 + rows : a.M;
  unsigned n[4] = {0u, 0u, 0u, 0u};
  if (j < a.N)
    for (int64_t i = i0; i < i1; ++i) {
      const float y = a.d_bf16 ? __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(a.D)[pmf_d_off16(i, j, a.nRB)] << 16)
                               : reinterpret_cast<const float *>(a.D)[pmf_d_off(i, j, a.nRB)];
      if (pmf_finite(y)) {
        const int c = (int)fminf(fmaxf(y + 0.5f, 0.f), 3.f);
        n[0] += c == 0; n[1] += c == 1; n[2] += c == 2; n[3] += c == 3;
      }
    }
  for (int r = 0; r < a.n_ranges; ++r) {
    const bool in = j >= a.c0[r] && j < a.c1[r];
    if (!__any(in)) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      unsigned v = in ? n[c] : 0u;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (threadIdx.x == 0 && v) atomicAdd(&a.counts[4 * r + c], (unsigned long long)v);
    }
  }
}
