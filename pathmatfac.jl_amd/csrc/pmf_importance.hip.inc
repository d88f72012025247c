// pmf_importance.hip.inc -- factor importance: every leave-one-factor-out loss from one pass over D (included by
// pmf_k_importance.hip; include/pmf_hip_importance.h has the definition, DESIGN.md section 4.18 the numbers).
//
// Per observed entry, with z1 = sigma_j sum_k x_ki y_kj and a(z) = z delta_bj + mu_j + theta_bj:
//   full += l(a(z1)) ; null += l(mu_j + theta_bj) ; delta[k] += l(a(z1 - sigma_j y_kj x_ki)) - l(a(z1))   for every k
// Leaving factor k out is a rank-1 change of the entry's inner product: one forward product, then K evaluations of the
// entry's loss (pmf_noise).  Those are VALU work and set the time; the MFMA forward is there because the staging serves it.
//
// Structure (gfx950), that of pmf_impute_kernel / pmf_thresh_kernel: a unit is ONE column tile times one range of row
// panels (one tile, not PMF_LS: the accumulation panel below is per tile).  The sigma-scaled Y tile and the column parameters
// are staged in LDS once per unit; inside the row sweep every wave works alone: its 32 rows of X go through registers into
// a private LDS panel, its D entries are loaded, the forward is K/2 v_mfma_f32_32x32x2_f32 with the operands EXCHANGED
// against impute: lane = column, register = row (register r of lane (l31, h) = row pmf_rowmap(r, h) of the block, column
// l31).  A column's parameters, noise kind and class bounds are then per lane, a row's x_ki one LDS broadcast, and a lane's
// partial of factor k over its 16 rows is ONE value.
// The epilogue loops over k, four at a time: y_kj is a 16-byte read of the lane's row of the staged Y tile, x_ki a 16-byte
// broadcast read of the wave's X panel -- no second product.  If x_ki = 0 or y_kj = 0 the product is +-0, z1 - 0 is z1, and
// the loss is evaluated on the same argument as the full one: the entry adds exactly 0.0.
// Masked entries (missing, pad row, pad column, w_j = 0) are computed at z1 = delta = mu + theta = y = 0, where every
// leave-one-out argument is 0 too: exactly 0.0 to every delta, and selects keep them out of full, null and n_obs.
//
// Accumulation, no atomics: the lane adds its 16 differences in register order, the two lane halves (rows 4h..) are joined
// by one lane exchange, and lane (l31, 0) adds the sum with a plain read-modify-write to ITS slot of the wave's LDS panel
// [Kp + 4][32] (rows Kp.. = full, null, n_obs).  Every PMF_IMP_FLUSH = 16 row panels, and at the end of the unit, the
// workgroup adds its waves' panels in wave order in float64 into the unit's private slab (the same thread owns a slab slot
// at every flush) and clears them.  LONGEST FLOAT32 CHAIN: 32 entries per slot and row panel x 16 panels = 512 entries
// (PMF_IMPORTANCE_CHAIN) before a value goes to float64.  k_importance_reduce adds the slabs of a column in row-range
// order, float64.  Bitwise the same run to run.
//
// D is read with sixteen 4-byte (2-byte: bf16) loads per lane at pmf_d_off / pmf_d_off16 -- the tile is stored for lane =
// row; the sixteen loads of a wave touch the tile's 32 (16) cache lines, all of them.  They are issued before the forward.
// The batch terms are impute's gathers from btab (any batch count: no table in LDS, so LDS does not depend on the batches).

template <int KB, int NW>
struct ImportanceCfg {
  static constexpr int Kp = 32 * KB, KpS = Kp + 4, YT = PMF_BN * KpS, XP = 32 * KpS;
  static constexpr int PR = pmf_imp_rows(KB), PN = PR * 32;   // rows / floats of a wave's accumulation panel
  // Y tile | X panels | accumulation panels | mu, w, meta, spare | btab base per column (int64) | class bounds
  static constexpr size_t lds = sizeof(float) * (YT + NW * XP + NW * PN) + sizeof(float) * 4 * 32 + sizeof(int64_t) * 32 + sizeof(float) * 32 * PMF_HT;
  static_assert(lds <= PMF_IMP_LDS_LIMIT, "pmf_importance_kernel: the instance does not fit the LDS of a workgroup");
};

// Entry (i0 + di, j) of D given the element offset o0 of (i0, j), for i0 + di inside i0's 32-row block: inside a tile a
// row is 4 elements (pmf_d_off) or 4 words of two bf16 (pmf_d_off16) further, so a lane's 16 rows are one address plus
// immediate offsets.
template <bool DB>
__device__ __forceinline__ float pmf_imp_load_d(const void *D, int64_t o0, int di) {
  if (DB) return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(D)[o0 + 8 * di] << 16);
  return reinterpret_cast<const float *>(D)[o0 + 4 * di];
}

// l(a^(-k)) - l(a), never fused with the multiplication that produced l: contracted into fma(p, q, -lf) the difference is
// the UNROUNDED product minus lf, half an ulp of lf where l == lf -- an absent term would leave rounding noise, not 0.0.
__device__ __forceinline__ float pmf_imp_diff(float l, float lf) {
#pragma clang fp contract(off)
  return l - lf;
}

template <int KB, int NW, bool DB>
__global__ __launch_bounds__(64 * NW, 1) void pmf_importance_kernel(const ImportanceArgs a) {
  using Cfg = ImportanceCfg<KB, NW>;
  constexpr int NT = 64 * NW;
  constexpr int Kp = Cfg::Kp, KpS = Cfg::KpS, KS = Kp / 2, BN = PMF_BN, PN = Cfg::PN;
  constexpr int XV = (32 * Kp / 4) / 64;   // float4 of a 32-row X panel per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *Ys = reinterpret_cast<float *>(smem);                 // [BN*KpS]  sigma_j * Y[k,j]
  float *Xs = Ys + Cfg::YT;                                    // [NW][32*KpS]
  float *Ps = Xs + NW * Cfg::XP;                               // [NW][PR][32] accumulation panels
  float *Cmu = Ps + NW * PN;                                   // [32] mu_j, w_j, meta_j (+ one spare array: 16-B layout)
  float *Cw = Cmu + 32;
  int *Cmt = reinterpret_cast<int *>(Cw + 32);
  int64_t *Cbase = reinterpret_cast<int64_t *>(Cmt + 2 * 32);  // [32] offset in btab of (column j, batch 0) of j's view
  float *Ht = reinterpret_cast<float *>(Cbase + 32);           // [32][PMF_HT] the columns' tables of class bounds

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int64_t M = a.M, N = a.N;
  float *Xw = Xs + w * Cfg::XP, *Pw = Ps + w * PN;
  const int nq = (a.K + 3) / 4;   // the factors in fours; a padded one among them has x = y = 0 and adds exact zeros

  const int n_units = a.n_ct * a.R;
  for (int u = blockIdx.x; u < n_units; u += gridDim.x) {
    const int ctl = u / a.R, rr = u - ctl * a.R;
    const int64_t ct = a.ct0 + ctl;
    const int64_t rp_lo = (int64_t)rr * a.n_rp / a.R, rp_hi = (int64_t)(rr + 1) * a.n_rp / a.R;
    double *slab = a.slabs + (int64_t)u * PN;
    __syncthreads();   // the previous unit is done with the shared tile
    for (int e4 = tid; e4 < BN * Kp / 4; e4 += NT) {
      const int jl = (e4 * 4) / Kp, kf = (e4 * 4) % Kp;
      const int64_t j = ct * BN + jl;
      float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < N) {
        const float sgm = a.colp[j].x;
        y = *reinterpret_cast<const float4 *>(a.Y + j * Kp + kf);
        y.x *= sgm; y.y *= sgm; y.z *= sgm; y.w *= sgm;
      }
      *reinterpret_cast<float4 *>(Ys + jl * KpS + kf) = y;
    }
    if (tid < 32) {
      const int64_t j = ct * BN + tid;
      // a pad column: weight 0 (masked), in no view, of the last column's kind (a tile that ends the matrix keeps one kind)
      const float4 cp = j < N ? a.colp[j] : make_float4(0.f, 0.f, 0.f, __int_as_float(pmf_meta_kind(__float_as_int(a.colp[N - 1].w))));
      const int meta = __float_as_int(cp.w);
      Cmu[tid] = cp.y; Cw[tid] = cp.z; Cmt[tid] = meta;
      Cbase[tid] = a.n_bv > 0 && pmf_meta_view(meta) >= 0 ? pmf_btab_index(a.views[pmf_meta_view(meta)], j, 0) : 0;
    }
    if (tid >= 64 && tid < 64 + 32 * PMF_HT / 4)   // (the table array is padded like D: a ragged tile reads in range)
      reinterpret_cast<float4 *>(Ht)[tid - 64] = a.htab ? reinterpret_cast<const float4 *>(a.htab + ct * BN * PMF_HT)[tid - 64]
                                                        : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = tid; e < NW * PN; e += NT) Ps[e] = 0.f;
    __syncthreads();

    // this lane's column
    const float muj = Cmu[l31], wj = Cw[l31];
    const int meta = Cmt[l31], kd = pmf_meta_kind(meta), vw = a.n_bv > 0 ? pmf_meta_view(meta) : -1;
    const int64_t base = Cbase[l31];
    const bool col_ok = wj != 0.f;
    const float *Htl = Ht + l31 * PMF_HT, *Ysl = Ys + l31 * KpS;
    // one noise kind in the whole tile (the usual case: columns are sorted by distribution): a wave-uniform branch
    const int k0 = __builtin_amdgcn_readfirstlane(kd);
    const int tk = __all(kd == k0) ? k0 : 4;

    bool first = true;
    int since = 0;
    // adds the waves' panels, in wave order and float64, to the unit's slab and clears them
    auto flush = [&]() {
      __syncthreads();
      for (int e = tid; e < PN; e += NT) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < NW; ++q) { s += (double)Ps[q * PN + e]; Ps[q * PN + e] = 0.f; }
        slab[e] = first ? s : slab[e] + s;
      }
      __syncthreads();
      first = false;
      since = 0;
    };

    for (int64_t rp = rp_lo; rp < rp_hi; ++rp) {
      const int64_t row0 = rp * (32 * NW) + (int64_t)w * 32;
      if (row0 < M) {   // (wave-uniform) some of this wave's rows exist
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
        __builtin_amdgcn_wave_barrier();
        // ---- the lane's 16 entries of D (rows of an existing row block: row0 < M; pad rows and columns are NaN)
        float yv[16];
        {
          const int64_t i0 = row0 + 4 * h, j = ct * BN + l31;   // row pmf_rowmap(r, h) = 4 h + pmf_rowmap(r, 0)
          const int64_t o0 = DB ? pmf_d_off16(i0, j, a.nRB) : pmf_d_off(i0, j, a.nRB);
#pragma unroll
          for (int r = 0; r < 16; ++r) yv[r] = pmf_imp_load_d<DB>(a.D, o0, pmf_rowmap(r, 0));
        }
        // ---- forward: z1[i,j] = sum_k X[k,i] sigma_j Y[k,j]; lane = column, register = row
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
          const float4 *yr = reinterpret_cast<const float4 *>(Ysl + h * (Kp / 2));
          const float4 *xq = reinterpret_cast<const float4 *>(Xw + l31 * KpS + h * (Kp / 2));
#pragma unroll
          for (int q = 0; q < KS / 4; ++q) {
            const float4 yq = yr[q], xv = xq[q];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.x, yq.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.y, yq.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.z, yq.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xv.w, yq.w, acc, 0, 0, 0);
          }
        }
        // ---- per entry: the batch step's {delta, mu + theta}, the full and the null loss.  A masked entry sits at 0.
        // (one instance per noise kind; `mine`: this lane's column is of that kind and has a weight)
        auto body = [&](auto kc, const bool mine) {
          constexpr int kind = decltype(kc)::value;
          float zf[16], dl[16], mt[16], lf[16], ym[16];
          float s_full = 0.f, s_null = 0.f, s_n = 0.f;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int64_t i = row0 + pmf_rowmap(r, h);
            if ((r & 3) == 0) __builtin_amdgcn_sched_barrier(0);   // (as in the factor loop below)
            const bool ok = mine && i < M && pmf_finite(yv[r]);
            float2 dt = make_float2(1.f, 0.f);
            if (vw >= 0 && ok) {
              const int b = a.bor[(int64_t)vw * M + i];
              if (b >= 0) dt = a.btab[base + b];
            }
            zf[r] = ok ? acc[r] : 0.f;
            dl[r] = ok ? dt.x : 0.f;
            mt[r] = ok ? muj + dt.y : 0.f;
            ym[r] = ok ? yv[r] : 0.f;
            float l0, g;
            pmf_noise<true>(kind, fmaf(zf[r], dl[r], mt[r]), ym[r], wj, Htl, lf[r], g);   // (the fmaf(z1, delta, mu + theta) of pmf_impute_batch)
            pmf_noise<true>(kind, mt[r], ym[r], wj, Htl, l0, g);
            s_full += ok ? lf[r] : 0.f;
            s_null += ok ? l0 : 0.f;
            s_n += ok ? 1.f : 0.f;
          }
          s_full += __shfl_xor(s_full, 32, 64);
          s_null += __shfl_xor(s_null, 32, 64);
          s_n += __shfl_xor(s_n, 32, 64);
          if (h == 0) {
            Pw[(Kp + 0) * 32 + l31] += s_full;
            Pw[(Kp + 1) * 32 + l31] += s_null;
            Pw[(Kp + 2) * 32 + l31] += s_n;
          }
          // ---- the factors, four at a time
          for (int q = 0; q < nq; ++q) {
            const float4 y4 = *reinterpret_cast<const float4 *>(Ysl + 4 * q);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              // four rows at a time: the x reads stay with their rows (hoisted, the sixteen cost 64 registers) and the 64 loss
              // evaluations of a step are not interleaved (merged, every one's temporaries are live at once)
              if ((r & 3) == 0) { PMF_SCHED_FENCE(); __builtin_amdgcn_sched_barrier(0); }
              const float4 x4 =*reinterpret_cast<const float4 *>(Xw + pmf_rowmap(r, h) * KpS + 4 * q);
              float l, g;
              pmf_noise<true>(kind, fmaf(zf[r] - y4.x * x4.x, dl[r], mt[r]), ym[r], wj, Htl, l, g);
              s0 += pmf_imp_diff(l, lf[r]);
              pmf_noise<true>(kind, fmaf(zf[r] - y4.y * x4.y, dl[r], mt[r]), ym[r], wj, Htl, l, g);
              s1 += pmf_imp_diff(l, lf[r]);
              pmf_noise<true>(kind, fmaf(zf[r] - y4.z * x4.z, dl[r], mt[r]), ym[r], wj, Htl, l, g);
              s2 += pmf_imp_diff(l, lf[r]);
              pmf_noise<true>(kind, fmaf(zf[r] - y4.w * x4.w, dl[r], mt[r]), ym[r], wj, Htl, l, g);
              s3 += pmf_imp_diff(l, lf[r]);
            }
            s0 += __shfl_xor(s0, 32, 64);
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            s3 += __shfl_xor(s3, 32, 64);
            if (h == 0) {
              float *pk = Pw + (4 * q) * 32 + l31;
              pk[0] += s0; pk[32] += s1; pk[64] += s2; pk[96] += s3;
            }
          }
        };
        // A tile of one kind runs that kind's instance.  A mixed tile runs the instance of every kind it holds with the
        // other kinds' lanes masked: they add exact zeros.  (One instance with the kind per lane -- divergent branches in
        // every one of the 64 unrolled evaluations -- compiled to scratch at eight waves.)
        if (tk == PMF_NOISE_NORMAL || (tk == 4 && __any(kd == PMF_NOISE_NORMAL)))
          body(std::integral_constant<int, PMF_NOISE_NORMAL>{}, col_ok && kd == PMF_NOISE_NORMAL);
        if (tk == PMF_NOISE_BERNOULLI || (tk == 4 && __any(kd == PMF_NOISE_BERNOULLI)))
          body(std::integral_constant<int, PMF_NOISE_BERNOULLI>{}, col_ok && kd == PMF_NOISE_BERNOULLI);
        if (tk == PMF_NOISE_POISSON || (tk == 4 && __any(kd == PMF_NOISE_POISSON)))
          body(std::integral_constant<int, PMF_NOISE_POISSON>{}, col_ok && kd == PMF_NOISE_POISSON);
        if (tk == PMF_NOISE_SQ_HINGE || (tk == 4 && __any(kd == PMF_NOISE_SQ_HINGE)))
          body(std::integral_constant<int, PMF_NOISE_SQ_HINGE>{}, col_ok && kd == PMF_NOISE_SQ_HINGE);
      }
      if (++since == PMF_IMP_FLUSH && rp + 1 < rp_hi) flush();
    }
    flush();
  }
}

// The slabs of a column tile, added in row-range order in float64: one thread per (tile of the launch, panel slot).
__global__ __launch_bounds__(256) void k_importance_reduce(const ImportanceReduceArgs a) {
  const int PR = pmf_imp_rows(a.KB), PN = PR * 32, Kp = 32 * a.KB;
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= (int64_t)a.n_ct * PN) return;
  const int ctl = (int)(e / PN), q = (int)(e - (int64_t)ctl * PN), row = q >> 5;
  const int64_t j = (int64_t)(a.ct0 + ctl) * PMF_BN + (q & 31);
  if (j >= a.N) return;
  double s = 0.0;
  for (int rr = 0; rr < a.R; ++rr) s += a.slabs[((int64_t)ctl * a.R + rr) * PN + q];
  if (row < a.K) { if (a.delta) a.delta[j * a.K + row] = s; }
  else if (row == Kp) a.full[j] = s;
  else if (row == Kp + 1) a.null_[j] = s;
  else if (row == Kp + 2) a.n_obs[j] = s;
}
