// pmf_impute.hip.inc -- the model's predictions (included by pmf_k_impute.hip).
//
// impute(model; include_batch_effects) of the reference (src/impute.jl:37-56): Z = layers(X'Y), then the inverse link of
// every column's noise model (:3-13, 27-35).  Per entry, with z1 = sigma_j a_ij:
//   z = z1 + mu_j                                  (default)
//   z = z1 delta_bj + mu_j + theta_bj              (PMF_IMPUTE_BATCH; delta = 1, theta = 0 for a row in no batch)
//   normal -> z ; bernoulli -> 1 / (1 + e^-z) ; poisson -> e^z ; sq_hinge -> the number of the column's thresholds strictly
//   below z (the bin rule of impute.jl:15-25: 0/1 for bernoulli_sq_hinge, 1..3 for ordinal_sq_hinge3)
//                                                                  (PMF_IMPUTE_LINK: z for every column)
// and, with PMF_IMPUTE_KEEP_OBSERVED, the stored entry of D wherever it is finite.
//
// Structure (gfx950): that of pmf_layer_kernel.  A workgroup owns PMF_LS = 2 column tiles and a range of 32 NW-row panels;
// the sigma-scaled Y tiles and the column parameters are staged in LDS once per unit; inside the row sweep every wave
// works alone: its 32 rows of X go through registers into a private LDS panel, the forward is K/2
// v_mfma_f32_32x32x2_f32 per tile (mu_j is the accumulator's initial value without BATCH), and the epilogue runs in the 16
// accumulator registers (lane = row, register = column) and ends in one 4-byte streaming store per register: for a given
// register the 32 lanes of a half-wave write 32 consecutive rows of one column, 128 B contiguous.
// Panels and 32-row blocks are ABSOLUTE (block rb = rows 32 rb .. 32 rb + 31 of the matrix, the rows of a D tile), whatever
// row range is asked for: an entry is always computed by the same lane of the same block in the same order, and the range
// only masks the stores.  The three flags are run-time, wave-uniform branches (one instance per (KB, NW, DB)).

// the two rules the MFMA kernel and the per-entry kernel share (pmf_impute_invlink: pmf_common.h, shared with pmf_debatch.hip.inc)
__device__ __forceinline__ float pmf_impute_batch(float z1, float mu, float2 dt) { return fmaf(z1, dt.x, mu + dt.y); }

template <int KB, int NW>
struct ImputeCfg {
  static constexpr int Kp = 32 * KB, KpS = Kp + 4, YT = PMF_BN * KpS, XP = 32 * KpS;
  // Y tiles | X panels | mu, meta per column | btab base per column (int64) | with BATCH: [NW][views][32 rows] batch ids
  static constexpr size_t lds(bool batch) {
    return sizeof(float) * (PMF_LS * YT + NW * XP) + sizeof(float) * 2 * PMF_LS * 32 + sizeof(int64_t) * PMF_LS * 32 +
           (batch ? sizeof(int32_t) * NW * PMF_MAXV * 32 : 0);
  }
};

// impute's epilogue: the inverse link of the tile's noise kind, the observed entries of D with KEEP_OBSERVED, and one
// streaming 4-byte store per register.  An epilogue policy Epi of pmf_impute_kernel (the other one: pmf_simulate.hip.inc) has
//   KEEP           whether PMF_IMPUTE_KEEP_OBSERVED is honoured (the D tile is loaded before the forward),
//   finish(...)    everything after the forward and the batch step, the stores included.
// finish sees: the accumulators (register r of lane (l31, h) = row irow, column 32 ct + pmf_rowmap(r, h)), the tile's noise
// kind tkt (3: per column), the tile's 32 metas in LDS, the column tile ct, the row block rb, and the D tile d when keep.
struct ImputeEpi {
  static constexpr bool KEEP = true;
  template <bool DB>
  __device__ __forceinline__ void finish(f32x16 acc, const ImputeArgs &a, int tkt, const int *Cmt_t, int64_t ct, int64_t rb, int lane,
                                         int64_t irow, bool row_ok, const PmfDTile<DB> &d, bool keep) const {
    constexpr int BN = PMF_BN;
    const int h = lane >> 5;
    const int64_t N = a.N;
    if (tkt == PMF_NOISE_BERNOULLI) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = pmf_impute_invlink(PMF_NOISE_BERNOULLI, acc[r], nullptr);
    } else if (tkt == PMF_NOISE_POISSON) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = pmf_impute_invlink(PMF_NOISE_POISSON, acc[r], nullptr);
    } else if (tkt == 3) {
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const int4 mt4 = *reinterpret_cast<const int4 *>(Cmt_t + 8 * c4 + 4 * h);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int meta = u == 0 ? mt4.x : (u == 1 ? mt4.y : (u == 2 ? mt4.z : mt4.w));
          acc[4 * c4 + u] = pmf_impute_invlink(pmf_meta_kind(meta), acc[4 * c4 + u], a.thr + ct * BN + 4 * h + (8 * c4 + u));
        }
      }
    }
    if (keep) {
      // pad rows and columns of D are NaN: they take the prediction, which the store masks
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float y = d.get(r);
        acc[r] = pmf_finite(y) ? y : acc[r];
      }
    }
    // ---- store: one streaming 4-byte store per register; a half-wave covers 128 contiguous bytes of one column
    const int64_t rrel = irow - a.row0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t j = ct * BN + pmf_rowmap(r, h);
      if (row_ok && j < N) __builtin_nontemporal_store(acc[r], a.out + pmf_impute_off(rrel, j, a.ld));
    }
  }
};

// One kernel template for impute (Epi = ImputeEpi) and simulate_data (Epi = SimEpi<FORM>, pmf_simulate.hip.inc): staging, the
// forward and the batch step are this one piece of code, so both issue the same FMAs in the same order for an entry; only
// Epi::finish differs.  The epilogue is a kernel ARGUMENT (an empty one for impute) and the body stays in the __global__
// function: moved into a __device__ function that both kernels call, the same text compiled to 16 to 75 more VGPRs and, at
// K = 64, to scratch.
template <int KB, int NW, bool DB, class Epi = ImputeEpi>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void pmf_impute_kernel(const ImputeArgs a, const Epi epi) {
  using Cfg = ImputeCfg<KB, NW>;
  constexpr int NT = 64 * NW;
  constexpr int Kp = Cfg::Kp, KpS = Cfg::KpS, KS = Kp / 2, BN = PMF_BN, LS = PMF_LS;
  constexpr int XV = (32 * Kp / 4) / 64;   // float4 of a 32-row X panel per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Ys = reinterpret_cast<float *>(smem);                 // [LS][BN*KpS]  sigma_j * Y[k,j]
  float *Xs = Ys + LS * Cfg::YT;                               // [NW][32*KpS]
  float *Cmu = Xs + NW * Cfg::XP;                              // [LS][32] mu_j
  int *Cmt = reinterpret_cast<int *>(Cmu + LS * 32);           // [LS][32] meta_j = kind | (view + 1) << 2
  int64_t *Cbase = reinterpret_cast<int64_t *>(Cmt + LS * 32); // [LS][32] offset in btab of (column j, batch 0) of j's view
  int32_t *Bw = reinterpret_cast<int32_t *>(Cbase + LS * 32) + (threadIdx.x >> 6) * (PMF_MAXV * 32);   // this wave: [views][32] batch of every row

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  const bool batch = (a.flags & PMF_IMPUTE_BATCH) != 0 && a.n_bv > 0, keep = Epi::KEEP && (a.flags & PMF_IMPUTE_KEEP_OBSERVED) != 0;
  const bool link = (a.flags & PMF_IMPUTE_LINK) != 0;
  float *Xw = Xs + w * Cfg::XP;

  const int n_units = a.n_seg * a.R;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int sg = u / a.R, rr = u - sg * a.R;
    const int ct0 = sg * LS;
    const int nt = a.n_ct - ct0 < LS ? a.n_ct - ct0 : LS;
    const int64_t rp_lo = a.rp0 + (int64_t)rr * a.n_rp / a.R, rp_hi = a.rp0 + (int64_t)(rr + 1) * a.n_rp / a.R;
    __syncthreads();   // the previous unit is done with the shared tiles
    // ---- stage the unit's Y tiles (scaled by sigma_j) and column parameters
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
      // pad columns take the last column's parameters (their results are never stored): a tile that ends the matrix
      // keeps one noise kind
      const int64_t j = (int64_t)ct0 * BN + c, jc = j < N ? j : N - 1;
      const float4 cp = a.colp[jc];
      const int meta = __float_as_int(cp.w);
      Cmu[c] = cp.y;
      Cmt[c] = meta;
      Cbase[c] = batch && pmf_meta_view(meta) >= 0 ? pmf_btab_index(a.views[pmf_meta_view(meta)], jc, 0) : 0;
    }
    __syncthreads();
    // one noise kind in the whole tile (the usual case: columns are sorted by distribution): a wave-uniform branch
    // (a tile of kind-3 columns takes the per-column path, tk = 3: its thresholds are per column)
    int tk[LS];
#pragma unroll
    for (int t = 0; t < LS; ++t) {
      const int kd = link || t >= nt ? PMF_NOISE_NORMAL : pmf_meta_kind(Cmt[t * 32 + l31]);
      const int k0 = __builtin_amdgcn_readfirstlane(kd);
      tk[t] = __all(kd == k0) ? k0 : 3;
    }

    for (int64_t rp = rp_lo; rp < rp_hi; ++rp) {
      const int64_t row0 = rp * (32 * NW) + (int64_t)w * 32;
      if (row0 >= a.row1 || row0 + 32 <= a.row0) continue;   // (wave-uniform) none of this wave's rows is asked for
      const int64_t irow = row0 + l31;
      const bool row_ok = irow >= a.row0 && irow < a.row1;
      const int64_t irow_c = irow < M ? irow : M - 1;
      // ---- this wave's X panel: registers -> private LDS panel
      __builtin_amdgcn_wave_barrier();
      {
        const float *xsrc = a.X + row0 * Kp;
        float4 xr[XV];
#pragma unroll
        for (int q = 0; q < XV; ++q) {
          const int e4 = lane + 64 * q;
          const int il = (e4 * 4) / Kp;
          xr[q] = row0 + il < M ? *reinterpret_cast<const float4 *>(xsrc + e4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < XV; ++q) {
          const int e4 = lane + 64 * q;
          *reinterpret_cast<float4 *>(Xw + ((e4 * 4) / Kp) * KpS + (e4 * 4) % Kp) = xr[q];
        }
      }
      if (batch && h == 0)
        for (int v = 0; v < a.n_bv; ++v) Bw[v * 32 + l31] = a.bor[(int64_t)v * M + irow_c];
      __builtin_amdgcn_wave_barrier();
      int64_t rb = rp * NW + w;
      if (rb >= a.nRB) rb = a.nRB - 1;
#pragma unroll
      for (int t = 0; t < LS; ++t) {
        if (t >= nt) break;
        PmfDTile<DB> d;
        if (keep) {
#pragma unroll
          for (int q = 0; q < PmfDTile<DB>::NCH; ++q) d.load(a.D, (int64_t)(ct0 + t) * a.nRB + rb, lane, q);
        }
        // ---- forward: z1[j,i] = sum_k sigma_j Y[k,j] X[k,i], on top of mu_j when the batch layers are off
        f32x16 acc;
#pragma unroll
        for (int c4 = 0; c4 < 4; ++c4) {
          const float4 mu4 = batch ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4 *>(Cmu + t * 32 + 8 * c4 + 4 * h);
          acc[4 * c4 + 0] = mu4.x; acc[4 * c4 + 1] = mu4.y; acc[4 * c4 + 2] = mu4.z; acc[4 * c4 + 3] = mu4.w;
        }
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
        // ---- epilogue in the accumulator layout: register r = 4 c4 + u of lane (l31, h) is column 8 c4 + 4 h + u
        if (batch) {
          // per entry: the {delta, theta} of (this row's batch in the column's view, column), gathered from btab -- one path
          // for any batch count, views that end inside the tile and rows in no batch
#pragma unroll
          for (int c4 = 0; c4 < 4; ++c4) {
            const int jb = t * 32 + 8 * c4 + 4 * h;
            const float4 mu4 = *reinterpret_cast<const float4 *>(Cmu + jb);
            const int4 mt4 = *reinterpret_cast<const int4 *>(Cmt + jb);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int r = 4 * c4 + u;
              const int meta = u == 0 ? mt4.x : (u == 1 ? mt4.y : (u == 2 ? mt4.z : mt4.w));
              const float muj = u == 0 ? mu4.x : (u == 1 ? mu4.y : (u == 2 ? mu4.z : mu4.w));
              const int v = pmf_meta_view(meta);
              float2 dt = make_float2(1.f, 0.f);
              if (v >= 0) {
                const int b = Bw[v * 32 + l31];
                if (b >= 0) dt = a.btab[Cbase[jb + u] + b];
              }
              acc[r] = pmf_impute_batch(acc[r], muj, dt);
            }
          }
        }
        epi.finish(acc, a, tk[t], Cmt + t * 32, (int64_t)(ct0 + t), rb, lane, irow, row_ok, d, keep);
      }
    }
  }
}

#ifndef PMF_IMPUTE_KERNEL_ONLY   // (pmf_k_simulate.hip takes pmf_impute_kernel alone)
// The predictions at listed entries: one entry per lane, the dot product over K in index order, the same two rules.
__global__ __launch_bounds__(256) void k_impute_entries(const ImputeEntriesArgs a) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const int64_t i = a.rows1[e] - 1, j = a.cols1[e] - 1;
  const float *x = a.X + i * a.Kp, *y = a.Y + j * a.Kp;
  float acc = 0.f;
  for (int k = 0; k < a.K; ++k) acc = fmaf(x[k], y[k], acc);
  const float4 cp = a.colp[j];
  const int meta = __float_as_int(cp.w);
  float z = acc * cp.x;
  if ((a.flags & PMF_IMPUTE_BATCH) != 0) {
    float2 dt = make_float2(1.f, 0.f);
    const int v = pmf_meta_view(meta);
    if (v >= 0) dt = pmf_batch_dt(a.views[v], a.btab, j, pmf_row_batch(a.bor, a.M, v, i));
    z = pmf_impute_batch(z, cp.y, dt);
  } else {
    z += cp.y;
  }
  a.out[e] = pmf_impute_invlink((a.flags & PMF_IMPUTE_LINK) != 0 ? PMF_NOISE_NORMAL : pmf_meta_kind(meta), z, a.thr + j);
}
#endif
