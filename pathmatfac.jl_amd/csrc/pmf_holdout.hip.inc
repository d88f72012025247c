// pmf_holdout.hip.inc -- the hold-out set's kernels (included by pmf_k_holdout.hip): the walk over the resident D that reads,
// blanks and restores the held entries, the hold-out loss pass, and its fixed-order sums.
//
// The pass is gather-bound: an entry costs its X column (Kp contiguous floats), four bytes of row index and four of value.
// A unit is at most PMF_HOLDOUT_UNIT entries of ONE column, swept by one wave.  The wave keeps the column's Y vector in
// registers (lane s of a 16-lane group holds k = 4 s .. 4 s + 3 and 64 + 4 s ..), loads 64 rows, values and batch
// parameters at a time with one coalesced access each, and hands every entry to a 16-lane group: the group reads the X column
// as float4s (256 contiguous bytes per instruction), each lane sums its eight products by fma in index order, and a
// butterfly over the sixteen lanes gives every lane a_ij.  The entry's loss goes to lbuf[e] (4 bytes beside 4 Kp + 8 read):
// the sums are then taken over lbuf in an order that knows entries and columns only, so units, waves and the grid decide
// where the work runs and nothing else (include/pmf_hip_holdout.h).

// one wave per column, lanes over the column's entries
__global__ __launch_bounds__(256) void k_holdout_d(const HoldoutDArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  for (int64_t j = wave; j < a.N; j += n_waves) {
    const int64_t e1 = a.colptr[j + 1];
    for (int64_t e = a.colptr[j] + lane; e < e1; e += 64) {
      const int64_t i = a.rows[e];
      if (a.d_bf16) {
        uint16_t *p = reinterpret_cast<uint16_t *>(a.D) + pmf_d_off16(i, j, a.nRB);
        if (a.mode == PMF_HOLDOUT_D_GATHER) a.vals[e] = __uint_as_float((uint32_t)*p << 16);
        else *p = a.mode == PMF_HOLDOUT_D_BLANK ? (uint16_t)0x7fc0 : (uint16_t)(__float_as_uint(a.vals[e]) >> 16);
      } else {
        float *p = reinterpret_cast<float *>(a.D) + pmf_d_off(i, j, a.nRB);
        if (a.mode == PMF_HOLDOUT_D_GATHER) a.vals[e] = *p;
        else *p = a.mode == PMF_HOLDOUT_D_BLANK ? __builtin_nanf("") : a.vals[e];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_holdout_pass(const HoldoutPassArgs a) {
  const int lane = threadIdx.x & 63, s = lane & 15, grp = lane >> 4;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
  const int Kp = a.Kp;
  const bool k0 = 4 * s < Kp, k1 = 64 + 4 * s < Kp;   // Kp = 32, 64, 96 or 128: this lane's two float4s of a column
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int u = wave; u < a.n_units; u += n_waves) {
    const int64_t j = a.u_col[u], e0 = a.u_e0[u];
    const int cnt = a.u_cnt[u];
    const float4 cp = a.colp[j];
    const int meta = __float_as_int(cp.w), kind = pmf_meta_kind(meta), v = a.n_bv > 0 ? pmf_meta_view(meta) : -1;
    const float *tp = a.htab ? a.htab + j * PMF_HT : nullptr;   // (read for kind 3 only; null: no such column)
    const float *yj = a.Y + j * Kp + 4 * s;
    const float4 y0 = k0 ? *reinterpret_cast<const float4 *>(yj) : zero4;
    const float4 y1 = k1 ? *reinterpret_cast<const float4 *>(yj + 64) : zero4;
    for (int b0 = 0; b0 < cnt; b0 += 64) {
      const int nb = cnt - b0 < 64 ? cnt - b0 : 64;
      // 64 entries: row, value and {delta, theta}, entry b0 + lane in lane `lane` (row 0 past the unit's end: never stored)
      const bool live = lane < nb;
      const int32_t r_l = live ? a.rows[e0 + b0 + lane] : 0;
      const float v_l = live ? a.vals[e0 + b0 + lane] : 0.f;
      float2 dt_l = make_float2(1.f, 0.f);
      if (v >= 0 && live) dt_l = pmf_batch_dt(a.views[v], a.btab, j, pmf_row_batch(a.bor, a.M, v, r_l));
      // four entries per step, four steps per trip: sixteen independent gathers in flight per wave (a trip's steps past
      // the unit's end read row 0 and store nothing)
      for (int t0 = 0; 4 * t0 < nb; t0 += 4)
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int q = 4 * (t0 + tt) + grp;
        const int64_t i = __shfl(r_l, q, 64);
        const float y = __shfl(v_l, q, 64);
        const float2 dt = make_float2(__shfl(dt_l.x, q, 64), __shfl(dt_l.y, q, 64));
        const float *xi = a.X + i * Kp + 4 * s;
        const float4 x0 = k0 ? *reinterpret_cast<const float4 *>(xi) : zero4;
        const float4 x1 = k1 ? *reinterpret_cast<const float4 *>(xi + 64) : zero4;
        float acc = 0.f;
        acc = fmaf(x0.x, y0.x, acc); acc = fmaf(x0.y, y0.y, acc); acc = fmaf(x0.z, y0.z, acc); acc = fmaf(x0.w, y0.w, acc);
        acc = fmaf(x1.x, y1.x, acc); acc = fmaf(x1.y, y1.y, acc); acc = fmaf(x1.z, y1.z, acc); acc = fmaf(x1.w, y1.w, acc);
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        const float z = fmaf(acc * cp.x, dt.x, cp.y + dt.y);
        float l, g;
        pmf_noise(kind, z, y, cp.z, tp, l, g);
        if (s == 0 && q < nb) a.lbuf[e0 + b0 + q] = l;
      }
    }
  }
}

// loss_col[j]: lane p sums the column's entries p, p + 64, ... in float64, then a butterfly over the 64 lanes
__global__ __launch_bounds__(256) void k_holdout_colsum(const HoldoutSumArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
  for (int64_t j = wave; j < a.N; j += n_waves) {
    const int64_t e1 = a.colptr[j + 1];
    double sum = 0.0;
    for (int64_t e = a.colptr[j] + lane; e < e1; e += 64) sum += (double)a.lbuf[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (lane == 0) a.loss_col[j] = sum;
  }
}

// *total: loss_col over ascending j, one addition after the other (one workgroup: 256 threads stage, thread 0 adds)
__global__ __launch_bounds__(256) void k_holdout_total(const HoldoutSumArgs a) {
  __shared__ double sh[2048];
  double sum = 0.0;
  for (int64_t j0 = 0; j0 < a.N; j0 += 2048) {
    const int n = a.N - j0 < 2048 ? (int)(a.N - j0) : 2048;
    for (int q = threadIdx.x; q < n; q += 256) sh[q] = a.loss_col[j0 + q];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int q = 0; q < n; ++q) sum += sh[q];
    __syncthreads();
  }
  if (threadIdx.x == 0) *a.total = sum;
}
