// pmf_simulate.hip.inc -- simulate_data!(model) of the reference (src/simulate_params.jl:219-251): a data matrix drawn from
// the model's current parameters (included by pmf_k_simulate.hip, after pmf_impute.hip.inc).
//
// Per entry (global 0-based row i = local row + row_offset, 0-based column j), with z = the link-space value of pmf_impute
// under PMF_IMPUTE_BATCH | PMF_IMPUTE_LINK (MF.forward(matfac), :247, all four layers), bit for bit, and the draws n, u3, u4
// of pmf_sim_draws(seed, i, j) (pmf_common.h):
//   normal                    out = fmaf(noise, n, z)                     (:240-242; noise == 0: z itself, no draw)
//   kind 3 (squared hinge)    out = pmf_hinge_class(z, thr[j])            (:224-238: the class of the noise-free z)
//   bernoulli (logit)         out = u4 < pmf_impute_invlink(BERNOULLI, z) ? 1 : 0      (SELF-SPECIFIED: no reference method)
//   poisson                   refused on the host before the launch (no sampler)
//   then                      u3 < frac_missing -> NaN                    (exact in f32: 0 never, 1 always)
// An entry depends on (parameters, seed, i, j, noise, frac_missing) alone.
//
// The kernel is pmf_impute_kernel with this epilogue: staging, forward and batch step are impute's code.  The Philox block of
// an entry is computed only where a draw is read: never in a kind-3 tile or a noise-free normal tile with frac_missing == 0.
// Store forms: impute's column-major streaming store, or the tile-major layout of the resident data matrix -- a lane's 16
// accumulator registers ARE its 16 floats of the tile (pmf_d_off), so a tile is four 1-KiB wave stores (two as packed bf16,
// pmf_d_off16), pad rows and columns NaN.

template <int FORM>
struct SimEpi {
  static constexpr bool KEEP = false;
  SimArgs s;
  // one entry: z -> the drawn value of a column of kind `kind` (wave-uniform where the tile has one kind)
  __device__ __forceinline__ float entry(int kind, float z, uint64_t gi, int64_t j, const float4 *thr, bool miss) const {
    const bool want_n = kind == PMF_NOISE_NORMAL && s.noise != 0.f;
    float out = z;
    if (kind == PMF_NOISE_SQ_HINGE) out = pmf_hinge_class(z, thr[j]);
    if (want_n || miss || kind == PMF_NOISE_BERNOULLI) {
      const PmfSimDraws d = pmf_sim_draws(s.seed, gi, (uint64_t)j, want_n);
      if (want_n) out = fmaf(s.noise, d.n, z);
      if (kind == PMF_NOISE_BERNOULLI) out = d.u4 < pmf_impute_invlink(PMF_NOISE_BERNOULLI, z, nullptr) ? 1.f : 0.f;
      if (miss && d.u3 < s.frac_missing) out = __int_as_float(0x7fc00000);
    }
    return out;
  }
  template <bool DB>
  __device__ __forceinline__ void finish(f32x16 acc, const ImputeArgs &a, int tkt, const int *Cmt_t, int64_t ct, int64_t rb, int lane,
                                         int64_t irow, bool row_ok, const PmfDTile<DB> &, bool) const {
    constexpr int BN = PMF_BN;
    const int h = lane >> 5;
    const uint64_t gi = (uint64_t)(irow + s.row_offset);
    const bool miss = s.frac_missing > 0.f;
    // The 16 entries of a lane in a ROLLED loop (the register index is wave-uniform): unrolled, the 16 Philox / logf / cosf
    // chains of a lane cost up to 1 KB of scratch per lane and sixteen copies of cosf's argument reduction.  tkt == 3: the
    // kind is per column (a tile of kind-3 columns, or one where two noise ranges meet).  Nothing to do in a normal tile
    // without noise and missingness.
    if (tkt != PMF_NOISE_NORMAL || miss || s.noise != 0.f) {
#pragma nounroll
      for (int r = 0; r < 16; ++r) {
        const int jl = pmf_rowmap(r, h);
        // (a pad column carries the last column's meta; its threshold read stays inside thr through the clamp)
        const int64_t j = ct * BN + jl, jc = j < a.N ? j : a.N - 1;
        const int kind = tkt == 3 ? pmf_meta_kind(Cmt_t[jl]) : tkt;
        acc[r] = entry(kind, acc[r], gi, jc, a.thr, miss);
      }
    }
    if (FORM == PMF_SIM_COLMAJOR) {
      const int64_t rrel = irow - a.row0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t j = ct * BN + pmf_rowmap(r, h);
        if (row_ok && j < a.N) __builtin_nontemporal_store(acc[r], a.out + pmf_impute_off(rrel, j, a.ld));
      }
    } else {
      // the whole tile (ct, rb) of D, pads included: rows >= M and columns >= N are NaN as pmf_set_data leaves them
      const float nan = __int_as_float(0x7fc00000);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = irow < a.M && ct * BN + pmf_rowmap(r, h) < a.N ? acc[r] : nan;
      const int64_t tile = ct * a.nRB + rb;
      if (FORM == PMF_SIM_TILE_F32) {
        float4 *dst = reinterpret_cast<float4 *>(a.out + tile * 1024) + lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) pmf_store_stream(dst + 64 * q, make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]));
      } else {
        // word e of chunk q = registers 8q + 2e (low half) and 8q + 2e + 1 (high half), rounded as k_tile_D rounds
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 *dst = reinterpret_cast<u32x4 *>(reinterpret_cast<uint16_t *>(a.out) + tile * 1024) + lane;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          u32x4 w;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t lo = __builtin_bit_cast(uint16_t, (__bf16)acc[8 * q + 2 * e]);
            const uint32_t hi = __builtin_bit_cast(uint16_t, (__bf16)acc[8 * q + 2 * e + 1]);
            w[e] = lo | (hi << 16);
          }
          __builtin_nontemporal_store(w, dst + 64 * q);
        }
      }
    }
  }
};
