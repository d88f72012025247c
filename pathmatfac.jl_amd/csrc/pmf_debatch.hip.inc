// pmf_debatch.hip.inc -- the data with the batch effects taken out (included by pmf_k_debatch.hip).
//
// remove_batch_effect(model, Z) of the reference (src/remove_batch_effect.jl:3-16), against the layer order this library
// implements everywhere (src/layers.jl:240-253: z = (a sigma_j) delta_bj + mu_j + theta_bj).  Per entry, with input v, b the
// batch of row i in column j's view and {delta, theta} = btab[(b, j)]:
//   column in no view, or row in no batch            -> v, bit for bit (selected before any arithmetic)
//   kind 3 (squared hinge: class labels, no link)    -> v, bit for bit        (without PMF_DEBATCH_LINK)
//   v not finite                                     -> NaN
//   else   l = link(v) ; l' = ((l - theta) - mu_j) / delta + mu_j ; out = invlink(l')
//          normal: identity ; bernoulli: log v - log(1 - v) in, the logistic of pmf_impute_invlink out ;
//          poisson: log v in, e^l' out               (PMF_DEBATCH_LINK: the identity for every column, kind 3 included)
// f32 in that order; the division is a multiplication by v_rcp_f32(delta) (1 ulp) fused with the last addition:
// l' = fma((l - theta) - mu_j, rcp(delta), mu_j) -- written as fmaf so that every copy of the rule rounds alike.  0 and 1 of a
// Bernoulli column and 0 of a Poisson column go through -Inf / +Inf and come back exactly; a value outside a link's domain is NaN.
//
// Structure (gfx950): a streaming kernel, one read and one write per entry.  A wave owns one 32 x 32 tile at a time --
// ABSOLUTE row block rb (rows 32 rb .. 32 rb + 31, the rows of a D tile) x column tile ct -- in the accumulator layout of
// the data matrix (lane = row, register r of lane (l31, h) = column pmf_rowmap(r, h)); consecutive waves take consecutive
// row blocks of one column tile, whose D tiles are contiguous.  SRC 0 / 1: the resident tile-major D, f32 or bf16, through
// PmfDTile (16-byte streaming loads); SRC 2: a column-major f32 matrix (a half-wave reads 128 contiguous bytes of one
// column per register).  One non-temporal 4-byte store per register: a half-wave writes 32 consecutive rows of one column.
// The range only masks the stores, so an entry's bits do not depend on it.  With PMF_DEBATCH_FILL_MISSING the output already
// holds pmf_impute's prediction and only observed entries are stored.
// The kernel is bound by vector-ALU issue before it is bound by HBM (a wave64 operation takes four cycles), so a tile is
// classified once, wave-uniformly: lane l31 loads the parameters of column 32 ct + l31, and when the 32 columns exist and
// share one meta word (noise kind and batch view: the usual case, columns are sorted by distribution) the tile takes the
// UNIFORM path -- the rule compiled for that kind, mu_j from the lane that holds it (ds_bpermute), the row's batch and the
// view's descriptor loaded once per (row block, view), {delta, theta} gathered per register from btab through a
// wave-uniform base and one per-lane offset, scalar address arithmetic.  Any other tile (a view seam or a change of kind
// inside it, the last columns of the matrix) takes the GENERAL path: per register the column's parameters, the batch of the
// lane's row re-read when the view changes (the columns of a lane ascend), the same rule with a per-lane kind.  Both gather
// {delta, theta} from btab: the one path that serves any batch count, including above 255 batches where no dense table exists.

// the link of `kind` (the caller passes PMF_NOISE_NORMAL under PMF_DEBATCH_LINK)
__device__ __forceinline__ float pmf_debatch_link(int kind, float v) {
  if (kind == PMF_NOISE_BERNOULLI) return __logf(v) - __logf(1.f - v);
  if (kind == PMF_NOISE_POISSON) return __logf(v);
  return v;
}

// THE per-entry rule (every path of both kernels).  kind: the column's noise kind, already PMF_NOISE_NORMAL under
// PMF_DEBATCH_LINK; has: the column is in a view and the row in one of its batches (dt is meaningful only then).
__device__ __forceinline__ float pmf_debatch_entry(int kind, float v, float mu, bool has, float2 dt) {
  if (kind == PMF_NOISE_SQ_HINGE) return v;
  const float l = pmf_debatch_link(kind, v);
  const float lp = fmaf((l - dt.y) - mu, __builtin_amdgcn_rcpf(dt.x), mu);
  const float o = pmf_impute_invlink(kind, lp, nullptr);   // (kind != 3: no thresholds are read)
  return has ? (pmf_finite(v) ? o : __int_as_float(0x7fc00000)) : v;
}

// A uniform tile (see above): KIND is the tile's link, gather says whether its columns are in a batch view.
template <int KIND>
__device__ __forceinline__ void pmf_debatch_uniform_tile(const float (&tv)[16], float mu_l, int h, bool gather, bool has, const float2 *tb,
                                                         uint32_t lb, int64_t nb, float *ob, int64_t lo, int64_t ld, bool row_ok, bool fill) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = (r & 3) + 8 * (r >> 2);                 // pmf_rowmap(r, h) = c + 4 h
    const float v = tv[r];
    float o = v;
    if (KIND != PMF_NOISE_SQ_HINGE && gather) {
      const float mu = __shfl(mu_l, 4 * h + c);
      const float2 dt = (tb + c * nb)[lb];
      o = pmf_debatch_entry(KIND, v, mu, has, dt);
    }
    if (row_ok && (!fill || pmf_finite(v))) __builtin_nontemporal_store(o, ob + c * ld + lo);
  }
}

template <int SRC>
__global__ __launch_bounds__(256) void pmf_debatch_kernel(const DebatchArgs a) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t M = a.M, N = a.N;
  const bool link = (a.flags & PMF_DEBATCH_LINK) != 0, fill = (a.flags & PMF_DEBATCH_FILL_MISSING) != 0;
  const uint32_t n_units = (uint32_t)(a.n_rb * a.n_ct), n_rb = (uint32_t)a.n_rb;   // (the host keeps the product below 2^31)
  for (uint32_t u = blockIdx.x * 4u + (uint32_t)w; u < n_units; u += gridDim.x * 4u) {
    const int64_t ct = u / n_rb, rb = a.rb0 + (u - (uint32_t)ct * n_rb);
    const int64_t irow = rb * 32 + l31;
    const bool row_ok = irow >= a.row0 && irow < a.row1;
    const int64_t irow_c = irow < M ? irow : M - 1;
    const int64_t rrel = irow - a.row0;
    // ---- classify the tile: lane l31 (of either half) holds the parameters of column 32 ct + l31
    const int64_t jl = ct * PMF_BN + l31;
    const float4 cpl = a.colp[jl < N ? jl : N - 1];
    const int m0 = __builtin_amdgcn_readfirstlane(__float_as_int(cpl.w));
    const bool uniform = (ct + 1) * PMF_BN <= N && __all(__float_as_int(cpl.w) == m0);
    // ---- the tile
    float tv[16];
    if constexpr (SRC == 2) {
      const float *Z = reinterpret_cast<const float *>(a.Z);
      if (uniform) {
        const float *zb = Z + ct * PMF_BN * a.ldz + (rb * 32 - a.row0);
        const int64_t lz = l31 + 4 * h * a.ldz;
#pragma unroll
        for (int r = 0; r < 16; ++r) tv[r] = row_ok ? __builtin_nontemporal_load(zb + ((r & 3) + 8 * (r >> 2)) * a.ldz + lz) : 0.f;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t j = ct * PMF_BN + pmf_rowmap(r, h);
          tv[r] = row_ok && j < N ? __builtin_nontemporal_load(Z + pmf_impute_off(rrel, j, a.ldz)) : 0.f;
        }
      }
    } else {
      PmfDTile<SRC == 1> d;
#pragma unroll
      for (int q = 0; q < PmfDTile<SRC == 1>::NCH; ++q) d.load(a.Z, ct * a.nRB + rb, lane, q);
#pragma unroll
      for (int r = 0; r < 16; ++r) tv[r] = d.get(r);
    }
    if (uniform) {
      // ---- one kind, one view: everything but the row's batch and the gather's per-lane offset is scalar
      const int kind = link ? PMF_NOISE_NORMAL : pmf_meta_kind(m0);
      const int vw = a.n_bv > 0 ? pmf_meta_view(m0) : -1;
      int b = -1;
      int64_t nb = 0;
      const float2 *tb = a.btab;
      if (vw >= 0) {
        const ViewDesc vd = a.views[vw];
        b = a.bor[(int64_t)vw * M + irow_c];
        nb = vd.nb;
        tb = a.btab + vd.tab_off + (ct * PMF_BN - vd.c0) * nb;      // (column 32 ct of the view, batch 0)
      }
      const bool has = b >= 0;
      const uint32_t lb = (uint32_t)(has ? b : 0) + 4u * (uint32_t)h * (uint32_t)nb;   // (32 nb < 2^32: nb is an int32)
      float *ob = a.out + ct * PMF_BN * a.ld + (rb * 32 - a.row0);
      const int64_t lo = l31 + 4 * h * a.ld;
      if (kind == PMF_NOISE_NORMAL) pmf_debatch_uniform_tile<PMF_NOISE_NORMAL>(tv, cpl.y, h, vw >= 0, has, tb, lb, nb, ob, lo, a.ld, row_ok, fill);
      else if (kind == PMF_NOISE_BERNOULLI) pmf_debatch_uniform_tile<PMF_NOISE_BERNOULLI>(tv, cpl.y, h, vw >= 0, has, tb, lb, nb, ob, lo, a.ld, row_ok, fill);
      else if (kind == PMF_NOISE_POISSON) pmf_debatch_uniform_tile<PMF_NOISE_POISSON>(tv, cpl.y, h, vw >= 0, has, tb, lb, nb, ob, lo, a.ld, row_ok, fill);
      else pmf_debatch_uniform_tile<PMF_NOISE_SQ_HINGE>(tv, cpl.y, h, false, false, tb, lb, nb, ob, lo, a.ld, row_ok, fill);
      continue;
    }
    // ---- the general path.  Per register: the column's parameters, the row's batch in the column's view, the rule, the store
    int vcur = -2, bcur = -1;          // the view whose batch id and descriptor this lane holds
    int64_t tab0 = 0, c0 = 0, nb = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t j = ct * PMF_BN + pmf_rowmap(r, h);
      const int64_t jc = j < N ? j : N - 1;      // pad columns take the last column's parameters; they are never stored
      const float4 cp = a.colp[jc];
      const int meta = __float_as_int(cp.w);
      const int vw = a.n_bv > 0 ? pmf_meta_view(meta) : -1;
      if (vw != vcur) {
        vcur = vw;
        bcur = -1;
        if (vw >= 0) {
          const ViewDesc vd = a.views[vw];
          bcur = a.bor[(int64_t)vw * M + irow_c];
          tab0 = vd.tab_off; c0 = vd.c0; nb = vd.nb;
        }
      }
      const bool has = bcur >= 0;
      float2 dt = make_float2(1.f, 0.f);
      if (has) dt = a.btab[tab0 + (jc - c0) * nb + bcur];
      const float v = tv[r];
      const float o = pmf_debatch_entry(link ? PMF_NOISE_NORMAL : pmf_meta_kind(meta), v, cp.y, has, dt);
      if (row_ok && j < N && (!fill || pmf_finite(v))) __builtin_nontemporal_store(o, a.out + pmf_impute_off(rrel, j, a.ld));
    }
  }
}

// The listed entries: one entry per lane, the same rule.  values == null: the entry of the resident D.
__global__ __launch_bounds__(256) void k_debatch_entries(const DebatchEntriesArgs a) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e >= a.n) return;
  const int64_t i = a.rows1[e] - 1, j = a.cols1[e] - 1;
  float v;
  if (a.values) {
    v = a.values[e];
  } else if (a.d_bf16) {
    v = __uint_as_float((uint32_t) reinterpret_cast<const uint16_t *>(a.D)[pmf_d_off16(i, j, a.nRB)] << 16);
  } else {
    v = reinterpret_cast<const float *>(a.D)[pmf_d_off(i, j, a.nRB)];
  }
  const float4 cp = a.colp[j];
  const int meta = __float_as_int(cp.w);
  const int vw = a.n_bv > 0 ? pmf_meta_view(meta) : -1;
  const int b = pmf_row_batch(a.bor, a.M, vw, i);
  float2 dt = make_float2(1.f, 0.f);
  if (b >= 0) dt = pmf_batch_dt(a.views[vw], a.btab, j, b);
  a.out[e] = pmf_debatch_entry((a.flags & PMF_DEBATCH_LINK) != 0 ? PMF_NOISE_NORMAL : pmf_meta_kind(meta), v, cp.y, b >= 0, dt);
}
