// pmf_outputs.hip -- what a fitted model gives back: pmf_forward / pmf_synth_data (k_forward), pmf_impute* (pmf_impute.hip.inc),
// pmf_simulate_data* (pmf_simulate.hip.inc) and pmf_remove_batch_effect* (pmf_debatch.hip.inc) with the one host path their staged calls share,
// and pmf_factor_importance (pmf_importance.hip.inc).
#include "pmf_ctx.h"
#include "pmf_importance.h"
#include "../../include/pmf_hip_importance.h"

// Z = layers(X'Y) materialised (MF.forward, simulate_params.jl:247); also used by pmf_synth_data.
struct ForwardArgs {
  const float *X, *Y;
  const float4 *colp;
  const float4 *thr;
  const int32_t *bor;
  const float2 *btab;
  float *Z;
  int64_t M, N, nRB;   // nRB > 0: write Z in the tile-major data layout (synthetic data; z_bf16: as bf16), else column-major
  int z_bf16;
  int Kp, K;
  int synth;
  uint64_t seed;
  float noise, frac_nan;
  ViewDesc views[PMF_MAXV];
};
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__global__ __launch_bounds__(256) void k_forward(const ForwardArgs a) {
  // block: 256 consecutive rows of one column -> coalesced stores along i
  const int64_t j = blockIdx.x;
  const int64_t i = blockIdx.y * 256ll + threadIdx.x;
  __shared__ float ys[128];
  for (int k = threadIdx.x; k < a.Kp; k += 256) ys[k] = a.Y[j * a.Kp + k];
  __syncthreads();
  if (i >= a.M) return;
  const float *x = a.X + i * a.Kp;
  float acc = 0.f;
  for (int k = 0; k < a.K; ++k) acc = fmaf(x[k], ys[k], acc);
  const float4 cp = a.colp[j];
  const int meta = __float_as_int(cp.w);
  const int v = pmf_meta_view(meta);
  float2 dt = make_float2(1.f, 0.f);
  if (v >= 0) dt = pmf_batch_dt(a.views[v], a.btab, j, pmf_row_batch(a.bor, a.M, v, i));
  float z = fmaf(acc * cp.x, dt.x, cp.y + dt.y);
  if (a.synth) {
    const uint64_t ctr = (uint64_t)(j * a.M + i);
    const uint64_t r1 = splitmix64(a.seed ^ (ctr * 2ull));
    const uint64_t r2 = splitmix64(a.seed ^ (ctr * 2ull + 1ull));
    const float u1 = ((r1 >> 40) + 1.0f) * (1.0f / 16777217.0f);
    const float u2 = (r1 & 0xFFFFFFull) * (1.0f / 16777216.0f);
    const float nrm = sqrtf(-2.f * logf(u1)) * cosf(6.28318530718f * u2);
    const int kind = pmf_meta_kind(meta);
    if (kind == PMF_NOISE_NORMAL) z += a.noise * nrm;
    else if (kind == PMF_NOISE_BERNOULLI) z = (z + a.noise * nrm) > 0.f ? 1.f : 0.f;
    else if (kind == PMF_NOISE_SQ_HINGE) z = pmf_hinge_class(z + a.noise * nrm, a.thr[j]);   // the class of the noisy prediction
    else z = floorf(__expf(fminf(z, 10.f)));
    const float u3 = (r2 >> 40) * (1.0f / 16777216.0f);
    if (u3 < a.frac_nan) z = __int_as_float(0x7fc00000);
  }
  if (a.nRB > 0 && a.z_bf16) reinterpret_cast<__bf16 *>(a.Z)[pmf_d_off16(i, j, a.nRB)] = (__bf16)z;
  else a.Z[a.nRB > 0 ? pmf_d_off(i, j, a.nRB) : j * a.M + i] = z;
}

static int run_forward(pmf_ctx *c, float *Zdev, int synth, uint64_t seed, float noise, float frac_nan, int64_t nRB = 0) {
  PMFCHK(check_ready(c));
  PMFCHK(prepare(c));
  ForwardArgs a;
  memset(&a, 0, sizeof(a));
  a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.thr = c->thr; a.bor = c->bor; a.btab = c->btab; a.Z = Zdev;
  a.z_bf16 = nRB > 0 && c->store == PMF_STORE_BF16;
  a.M = c->M; a.N = c->N; a.nRB = nRB; a.Kp = c->Kp; a.K = c->K; a.synth = synth; a.seed = seed; a.noise = noise; a.frac_nan = frac_nan;
  fill_views(c, a.views);
  if ((c->M + 255) / 256 > 65535) return pmf_fail("M too large for the forward kernel grid");
  hipLaunchKernelGGL(k_forward, dim3((unsigned)c->N, (unsigned)((c->M + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int pmf_forward(pmf_ctx *c, float *Z_host) {
  PMFCHK(ctx_bind(c));
  if (!Z_host) return pmf_fail("null output");
  const size_t bytes = sizeof(float) * (size_t)(c->M * c->N);
  DevBuf<float> Z;
  PMFCHK(Z.alloc((size_t)(c->M * c->N), false));
  int rc = run_forward(c, Z, 0, 0, 0.f, 0.f);
  if (rc == 0) {
    hipError_t e = hipMemcpyAsync(Z_host, Z, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = pmf_fail("copy back failed: %s", hipGetErrorString(e));
  }
  return rc;
}

extern "C" int pmf_synth_data(pmf_ctx *c, uint64_t seed, float noise, float frac_nan) {
  PMFCHK(ctx_bind(c));
  if (!c->D) return pmf_fail("data buffer not allocated (pmf_set_data_device(ctx, NULL, M, N, store))");
  c->tflags_valid = false;
  holdout_drop(c);
  PMFCHK(run_forward(c, (float *)c->D.p, 1, seed, noise, frac_nan, c->nRB));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the host path impute and remove_batch_effect share: readiness, and the two loops that stage a call through the context's
// impute_stage buffer (whole rows in chunks of rows, listed entries in chunks of entries)
#define PMF_IMPUTE_STAGE_MAX ((size_t)256 << 20)   // the bound of pmf_set_data's upload chunks

// The context needs M, N (a data matrix has been set: it is what fixes them), factors and complete batch views.
static int outputs_ready(pmf_ctx *c, const char *fn) {
  if (c->K == 0 || c->M <= 0 || c->N <= 0) return pmf_fail("%s: factors not set", fn);
  for (int v = 0; v < c->n_bv; ++v)
    if (c->views[v].nb == 0) return pmf_fail("%s: batch view %d declared but not set", fn, v);
  return 0;
}

// chunk height of a staged call: what 256 MiB hold of `parts` N-column rows per row (whole 32-row blocks when there are that
// many), at least one row; the environment variable `env`, read at every call, lowers it
static int64_t stage_chunk_rows(int64_t N, int parts, const char *env) {
  const int64_t cap = std::max<int64_t>(1, (int64_t)(PMF_IMPUTE_STAGE_MAX / sizeof(float)) / N / parts);
  const int64_t ch = cap >= 32 ? cap - cap % 32 : cap;
  const char *e = getenv(env);
  return e && atoll(e) > 0 ? std::min<int64_t>(atoll(e), cap) : ch;
}

// Rows [row0, row1) (0-based) to out_host (leading dimension ld) in chunks of stage_chunk_rows.  The stage holds `parts` chunks:
// the output part first, then (parts == 2) the part a host input `in_host` (leading dimension ldin; may be null) is uploaded
// to; with one part an input is corrected in place.  launch(r0, r1, in_stage or null, out_stage, nr) runs after prepare().
template <typename Launch>
static int staged_rows(pmf_ctx *c, int64_t row0, int64_t row1, int parts, const char *env, const float *in_host, int64_t ldin,
                       float *out_host, int64_t ld, Launch launch) {
  const int64_t ch = std::min(stage_chunk_rows(c->N, parts, env), row1 - row0);
  PMFCHK(c->impute_stage.ensure(sizeof(float) * (size_t)(ch * c->N * parts), false));
  PMFCHK(prepare(c));
  float *s_out = (float *)c->impute_stage.p, *s_in = s_out + (parts - 1) * ch * c->N;
  for (int64_t r0 = row0; r0 < row1; r0 += ch) {
    const int64_t nr = std::min(ch, row1 - r0), rel = r0 - row0;
    const size_t w = sizeof(float) * (size_t)nr;   // bytes of a staged column
    if (in_host) HIPCHK(hipMemcpy2DAsync(s_in, w, in_host + rel, sizeof(float) * (size_t)ldin, w, (size_t)c->N, hipMemcpyHostToDevice, c->stream));
    PMFCHK(launch(r0, r0 + nr, in_host ? s_in : nullptr, s_out, nr));
    HIPCHK(hipMemcpy2DAsync(out_host + rel, sizeof(float) * (size_t)ld, s_out, w, w, (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

// The whole of an *_entries call: n listed entries (1-based rows1, cols1; `values` may be null) to out_host.  n == 0 returns before
// anything else is looked at; check() is the call's own test.  At most 1 << 22 entries are staged at a time, laid out rows | cols |
// [values] | out (20 bytes per entry, 24 with values); launch(d_rows, d_cols, d_values or null, d_out, ne) runs after prepare().
template <typename Check, typename Launch>
static int staged_entries(pmf_ctx *c, const char *fn, int64_t n, const int64_t *rows1, const int64_t *cols1, const float *values,
                          float *out_host, Check check, Launch launch) {
  PMFCHK(ctx_bind(c));
  if (n < 0) return pmf_fail("%s: n=%lld", fn, (long long)n);
  if (n == 0) return 0;
  PMFCHK(check());
  if (!rows1 || !cols1) return pmf_fail("%s: null index pointer", fn);
  for (int64_t e = 0; e < n; ++e)
    if (rows1[e] < 1 || rows1[e] > c->M || cols1[e] < 1 || cols1[e] > c->N)
      return pmf_fail("%s: entry %lld = (%lld, %lld) is outside 1..%lld x 1..%lld", fn, (long long)e, (long long)rows1[e],
                      (long long)cols1[e], (long long)c->M, (long long)c->N);
  const int64_t ch = std::min<int64_t>(n, 1ll << 22);
  PMFCHK(c->impute_stage.ensure((size_t)ch * (2 * sizeof(int64_t) + (values ? 2 : 1) * sizeof(float)), false));
  PMFCHK(prepare(c));
  int64_t *d_rows = (int64_t *)c->impute_stage.p, *d_cols = d_rows + ch;
  float *d_val = values ? (float *)(d_cols + ch) : nullptr, *d_out = (float *)(d_cols + ch) + (values ? ch : 0);
  for (int64_t e0 = 0; e0 < n; e0 += ch) {
    const int64_t ne = std::min(ch, n - e0);
    HIPCHK(hipMemcpyAsync(d_rows, rows1 + e0, sizeof(int64_t) * (size_t)ne, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_cols, cols1 + e0, sizeof(int64_t) * (size_t)ne, hipMemcpyHostToDevice, c->stream));
    if (values) HIPCHK(hipMemcpyAsync(d_val, values + e0, sizeof(float) * (size_t)ne, hipMemcpyHostToDevice, c->stream));
    PMFCHK(launch(d_rows, d_cols, d_val, d_out, ne));
    HIPCHK(hipMemcpyAsync(out_host + e0, d_out, sizeof(float) * (size_t)ne, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// impute (src/impute.jl): predictions from the current parameters, whole rows or listed entries
// ------------------------------------------------------------------------------------------------
// what every impute call checks before it touches the device: the values of D only for PMF_IMPUTE_KEEP_OBSERVED
static int impute_check(pmf_ctx *c, const char *fn, int flags, const void *out, bool entries) {
  if (!out) return pmf_fail("%s: null output pointer", fn);
  if (flags & ~(PMF_IMPUTE_BATCH | PMF_IMPUTE_LINK | PMF_IMPUTE_KEEP_OBSERVED)) return pmf_fail("%s: unknown flag bits 0x%x", fn, flags);
  if (entries && (flags & PMF_IMPUTE_KEEP_OBSERVED)) return pmf_fail("%s: PMF_IMPUTE_KEEP_OBSERVED is not accepted here (the caller holds the observed entries)", fn);
  if ((flags & PMF_IMPUTE_KEEP_OBSERVED) && !c->D) return pmf_fail("%s: PMF_IMPUTE_KEEP_OBSERVED needs the data matrix (data not set)", fn);
  return outputs_ready(c, fn);
}

static int impute_check_range(pmf_ctx *c, const char *fn, int64_t s1, int64_t e1, int64_t ld) {
  if (s1 < 1 || e1 > c->M || s1 > e1) return pmf_fail("%s: empty or out-of-range row range %lld:%lld (rows 1..%lld)", fn, (long long)s1, (long long)e1, (long long)c->M);
  if (ld < e1 - s1 + 1) return pmf_fail("%s: ld=%lld is below the row count %lld", fn, (long long)ld, (long long)(e1 - s1 + 1));
  return 0;
}

// The arguments and the grid of a sweep (pmf_impute_kernel, pmf_simulate_kernel) over rows [row0, row1) (0-based) and n_ct
// column tiles; prepare() has run.
static int impute_args(pmf_ctx *c, const char *fn, int flags, int64_t row0, int64_t row1, int64_t n_ct, float *out_dev, int64_t ld,
                       ImputeArgs &a, int &grid) {
  const int nw = pmf_impute_waves(c->KB);
  const int64_t BM = 32 * nw;
  memset(&a, 0, sizeof(a));
  a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.thr = c->thr; a.bor = c->bor; a.btab = c->btab; a.views = c->d_views;
  a.D = c->D; a.nRB = c->nRB; a.out = out_dev; a.ld = ld; a.M = c->M; a.N = c->N; a.row0 = row0; a.row1 = row1;
  a.rp0 = row0 / BM;
  a.n_rp = (row1 - 1) / BM + 1 - a.rp0;
  a.n_bv = c->n_bv; a.flags = flags;
  const int64_t n_seg = (n_ct + PMF_LS - 1) / PMF_LS;
  if (n_ct >= (1ll << 31)) return pmf_fail("%s: N too large", fn);
  // a unit = (column segment, 1/R of the panels); R as in the layer pass: a few units per CU, consecutive units share a segment
  const int64_t R = std::max<int64_t>(1, std::min<int64_t>(a.n_rp, (4ll * c->n_cu + n_seg - 1) / n_seg));
  a.n_ct = (int)n_ct; a.n_seg = (int)n_seg; a.R = (int)R;
  if (n_seg * R >= (1ll << 31)) return pmf_fail("%s: too many units", fn);
  grid = (int)std::min<int64_t>(n_seg * R, c->n_cu);
  return 0;
}

// rows [row0, row1) (0-based) into out_dev (leading dimension ld); prepare() has run
static int impute_launch(pmf_ctx *c, int flags, int64_t row0, int64_t row1, float *out_dev, int64_t ld) {
  ImputeArgs a;
  int grid = 0;
  PMFCHK(impute_args(c, "pmf_impute", flags, row0, row1, (c->N + PMF_BN - 1) / PMF_BN, out_dev, ld, a, grid));
  return pmf_launch_impute(&c->dyn_lds, c->stream, c->KB, c->store == PMF_STORE_BF16, grid, a);
}

extern "C" int pmf_impute_device(pmf_ctx *c, int flags, int64_t row_start1, int64_t row_stop1, float *out_device, int64_t ld) {
  PMFCHK(ctx_bind(c));
  PMFCHK(impute_check(c, "pmf_impute_device", flags, out_device, false));
  PMFCHK(impute_check_range(c, "pmf_impute_device", row_start1, row_stop1, ld));
  PMFCHK(prepare(c));
  PMFCHK(impute_launch(c, flags, row_start1 - 1, row_stop1, out_device, ld));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pmf_impute(pmf_ctx *c, int flags, int64_t row_start1, int64_t row_stop1, float *out_host, int64_t ld) {
  PMFCHK(ctx_bind(c));
  PMFCHK(impute_check(c, "pmf_impute", flags, out_host, false));
  PMFCHK(impute_check_range(c, "pmf_impute", row_start1, row_stop1, ld));
  return staged_rows(c, row_start1 - 1, row_stop1, 1, "PMF_IMPUTE_CHUNK_ROWS", nullptr, 0, out_host, ld,
                     [&](int64_t r0, int64_t r1, const float *, float *s_out, int64_t nr) { return impute_launch(c, flags, r0, r1, s_out, nr); });
}

extern "C" int pmf_impute_entries(pmf_ctx *c, int flags, int64_t n, const int64_t *rows1, const int64_t *cols1, float *out_host) {
  static const char *fn = "pmf_impute_entries";
  return staged_entries(c, fn, n, rows1, cols1, nullptr, out_host, [&] { return impute_check(c, fn, flags, out_host, true); },
                        [&](const int64_t *d_rows, const int64_t *d_cols, const float *, float *d_out, int64_t ne) {
                          ImputeEntriesArgs a;
                          memset(&a, 0, sizeof(a));
                          a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.thr = c->thr; a.bor = c->bor; a.btab = c->btab; a.views = c->d_views;
                          a.rows1 = d_rows; a.cols1 = d_cols; a.out = d_out; a.n = ne; a.M = c->M; a.Kp = c->Kp; a.K = c->K; a.flags = flags;
                          return pmf_launch_impute_entries(c->stream, a);
                        });
}

// ------------------------------------------------------------------------------------------------
// simulate_data! (src/simulate_params.jl:219-251): seeded draws from the current parameters (pmf_simulate.hip.inc)
// ------------------------------------------------------------------------------------------------
// what every call checks before it touches the device
static int simulate_check(pmf_ctx *c, const char *fn, const pmf_sim_opts *o) {
  if (!o) return pmf_fail("%s: null options", fn);
  if (!(o->noise >= 0.f) || !std::isfinite(o->noise)) return pmf_fail("%s: noise=%g must be finite and >= 0", fn, (double)o->noise);
  if (!(o->frac_missing >= 0.f && o->frac_missing <= 1.f)) return pmf_fail("%s: frac_missing=%g is outside [0, 1]", fn, (double)o->frac_missing);
  if (o->row_offset < 0) return pmf_fail("%s: row_offset=%lld is negative", fn, (long long)o->row_offset);
  PMFCHK(outputs_ready(c, fn));
  for (size_t j = 0; j < c->h_kind.size(); ++j)
    if ((c->h_kind[j] & 3) == PMF_NOISE_POISSON)
      return pmf_fail("%s: column %lld has Poisson noise, for which there is no sampler", fn, (long long)(j + 1));
  return 0;
}

// rows [row0, row1) (0-based) in store form `form`: into out_dev (column-major, leading dimension ld) or the resident D
static int simulate_launch(pmf_ctx *c, const pmf_sim_opts *o, int form, int64_t row0, int64_t row1, float *out_dev, int64_t ld) {
  ImputeArgs a;
  int grid = 0;
  // the tile-major forms write every column tile of D, the all-pad one of an odd tile count included
  const int64_t n_ct = form == PMF_SIM_COLMAJOR ? (c->N + PMF_BN - 1) / PMF_BN : c->D_Npad / PMF_BN;
  PMFCHK(impute_args(c, "pmf_simulate_data", PMF_IMPUTE_BATCH, row0, row1, n_ct, out_dev, ld, a, grid));
  SimArgs s;
  s.seed = o->seed; s.row_offset = o->row_offset; s.noise = o->noise; s.frac_missing = o->frac_missing;
  return pmf_launch_simulate(&c->dyn_lds, c->stream, c->KB, form, grid, a, s);
}

extern "C" int pmf_simulate_data_device(pmf_ctx *c, const pmf_sim_opts *opts, int64_t row_start1, int64_t row_stop1, float *out_device,
                                        int64_t ld) {
  static const char *fn = "pmf_simulate_data_device";
  PMFCHK(ctx_bind(c));
  if (!out_device) return pmf_fail("%s: null output pointer", fn);
  PMFCHK(simulate_check(c, fn, opts));
  PMFCHK(impute_check_range(c, fn, row_start1, row_stop1, ld));
  PMFCHK(prepare(c));
  PMFCHK(simulate_launch(c, opts, PMF_SIM_COLMAJOR, row_start1 - 1, row_stop1, out_device, ld));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pmf_simulate_data(pmf_ctx *c, const pmf_sim_opts *opts, int64_t row_start1, int64_t row_stop1, float *out_host, int64_t ld) {
  static const char *fn = "pmf_simulate_data";
  PMFCHK(ctx_bind(c));
  if (!out_host) return pmf_fail("%s: null output pointer", fn);
  PMFCHK(simulate_check(c, fn, opts));
  PMFCHK(impute_check_range(c, fn, row_start1, row_stop1, ld));
  return staged_rows(c, row_start1 - 1, row_stop1, 1, "PMF_SIMULATE_CHUNK_ROWS", nullptr, 0, out_host, ld,
                     [&](int64_t r0, int64_t r1, const float *, float *s_out, int64_t nr) {
                       return simulate_launch(c, opts, PMF_SIM_COLMAJOR, r0, r1, s_out, nr);
                     });
}

extern "C" int pmf_simulate_data_resident(pmf_ctx *c, const pmf_sim_opts *opts) {
  static const char *fn = "pmf_simulate_data_resident";
  PMFCHK(ctx_bind(c));
  PMFCHK(simulate_check(c, fn, opts));
  if (!c->D) return pmf_fail("%s: data buffer not allocated (pmf_set_data_device(ctx, NULL, M, N, store) or pmf_set_data)", fn);
  PMFCHK(prepare(c));
  c->tflags_valid = false;   // what pmf_set_data invalidates: the per-tile all-finite flags of the old values
  holdout_drop(c);           // ... and a hold-out set, without write-back
  PMFCHK(simulate_launch(c, opts, c->store == PMF_STORE_BF16 ? PMF_SIM_TILE_BF16 : PMF_SIM_TILE_F32, 0, c->M, (float *)c->D.p, c->M));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pmf_debug_impute_offset(int64_t row, int64_t col, int64_t ld, int64_t *offset) {
  if (!offset) return pmf_fail("null output");
  *offset = pmf_impute_off(row, col, ld);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// factor importance (include/pmf_hip_importance.h; not in the reference): pmf_importance.hip.inc
// ------------------------------------------------------------------------------------------------
// The cap on the pass's private float64 slabs, one of (Kp + 4) x 32 doubles per (column tile, row range): what pmf_set_data's
// upload chunks and impute's stage are held to.  The row ranges R are lowered to stay under it, and where the column tiles
// alone exceed it at R = 1 (N above 480 000 at K = 64) the tiles are walked in several launches.
#define PMF_IMPORTANCE_SLAB_MAX ((size_t)256 << 20)

static int env_cap(const char *name, int64_t v) {
  const char *e = getenv(name);   // test hooks, read at every call
  return (int)(e && atoll(e) > 0 ? std::min<int64_t>(v, atoll(e)) : v);
}

extern "C" int pmf_factor_importance(pmf_ctx *c, double *delta, double *full, double *null_, int64_t *n_obs) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  if (c->KB < 1 || c->KB > 4) return pmf_fail("pmf_factor_importance: built for K <= 128 (K = %d)", c->K);
  PMFCHK(prepare(c));
  ImportanceState &s = c->imp;
  const int nw = pmf_importance_waves(c->KB);
  const int64_t K = c->K, N = c->N, n_ct = (N + PMF_BN - 1) / PMF_BN, n_rp = (c->M + 32 * nw - 1) / (32 * nw);
  const size_t slab = sizeof(double) * (size_t)pmf_imp_rows(c->KB) * 32;
  // column tiles per launch (all of them unless the slabs of R = 1 exceed the cap), then the row ranges: about eight units per
  // CU, so that the tail of the persistent grid stays short, as far as the cap allows
  const int64_t tiles = env_cap("PMF_IMPORTANCE_TILES", std::min<int64_t>(n_ct, std::max<int64_t>(1, (int64_t)(PMF_IMPORTANCE_SLAB_MAX / slab))));
  int64_t R = std::max<int64_t>(1, std::min<int64_t>(n_rp, (8ll * c->n_cu + tiles - 1) / tiles));
  R = std::max<int64_t>(1, std::min<int64_t>(R, (int64_t)(PMF_IMPORTANCE_SLAB_MAX / slab) / tiles));
  R = env_cap("PMF_IMPORTANCE_RANGES", R);
  if (tiles * R >= (1ll << 31)) return pmf_fail("pmf_factor_importance: too many units");
  PMFCHK(s.slabs.ensure((size_t)(tiles * R) * (slab / sizeof(double)), false, "the factor-importance slabs"));
  PMFCHK(s.out.ensure((size_t)((K + 3) * N), false, "the factor-importance sums"));
  ImportanceArgs a;
  memset(&a, 0, sizeof(a));
  a.D = c->D; a.nRB = c->nRB; a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.bor = c->bor; a.btab = c->btab;
  a.htab = c->mixed ? c->htab.p : nullptr;   // (the tables follow the noise model only while it has a column that is not normal)
  a.views = c->d_views; a.slabs = s.slabs; a.M = c->M; a.N = N; a.K = c->K; a.n_bv = c->n_bv; a.n_rp = (int)n_rp; a.R = (int)R;
  ImportanceReduceArgs r;
  memset(&r, 0, sizeof(r));
  r.slabs = s.slabs; r.R = (int)R; r.KB = c->KB; r.K = c->K; r.N = N;
  r.delta = s.out.p; r.full = s.out.p + K * N; r.null_ = r.full + N; r.n_obs = r.null_ + N;
  s.kb = c->KB; s.nw = nw; s.db = c->store == PMF_STORE_BF16; s.R = (int)R; s.n_units = 0; s.grid = 0; s.launches = 0;
  s.flushes = (int)(((n_rp + R - 1) / R + PMF_IMP_FLUSH - 1) / PMF_IMP_FLUSH);   // (the host's arithmetic on the geometry: not observed in the kernel)
  for (int64_t ct0 = 0; ct0 < n_ct; ct0 += tiles) {
    a.ct0 = r.ct0 = (int)ct0;
    a.n_ct = r.n_ct = (int)std::min(tiles, n_ct - ct0);
    const int grid = env_cap("PMF_IMPORTANCE_GRID", std::min<int64_t>((int64_t)a.n_ct * R, c->n_cu));
    PMFCHK(pmf_launch_importance(&c->dyn_lds, c->stream, c->KB, s.db != 0, grid, a));
    PMFCHK(pmf_launch_importance_reduce(c->stream, r));   // (stream order: the next launch reuses the slabs after it)
    s.n_units += a.n_ct * (int)R; s.grid = std::max(s.grid, grid); s.launches++;
  }
  s.calls++;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (delta) HIPCHK(hipMemcpy(delta, r.delta, sizeof(double) * (size_t)(K * N), hipMemcpyDeviceToHost));
  if (full) HIPCHK(hipMemcpy(full, r.full, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
  if (null_) HIPCHK(hipMemcpy(null_, r.null_, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
  if (n_obs) {
    std::vector<double> cnt((size_t)N);
    HIPCHK(hipMemcpy(cnt.data(), r.n_obs, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < N; ++j) n_obs[j] = (int64_t)cnt[(size_t)j];   // (exact: sums of small integers in float64)
  }
  return 0;
}

extern "C" int pmf_debug_factor_importance(pmf_ctx *c, int *kb, int *nw, int *db, int *n_ranges, int *n_units, int *grid, int *launches,
                                           int *flushes, int64_t *calls) {
  PMFCHK(ctx_bind(c));
  const ImportanceState &s = c->imp;
  if (kb) *kb = s.kb;
  if (nw) *nw = s.nw;
  if (db) *db = s.db;
  if (n_ranges) *n_ranges = s.R;
  if (n_units) *n_units = s.n_units;
  if (grid) *grid = s.grid;
  if (launches) *launches = s.launches;
  if (flushes) *flushes = s.flushes;
  if (calls) *calls = s.calls;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// remove_batch_effect (src/remove_batch_effect.jl): the data with layers 2 and 4 taken out (pmf_debatch.hip.inc)
// ------------------------------------------------------------------------------------------------
// what every call checks before it touches the device: impute's readiness, and resident data when that is the input
static int debatch_check(pmf_ctx *c, const char *fn, int flags, bool resident, const void *out, bool entries) {
  if (!out) return pmf_fail("%s: null output pointer", fn);
  if (flags & ~(PMF_DEBATCH_LINK | PMF_DEBATCH_FILL_MISSING)) return pmf_fail("%s: unknown flag bits 0x%x", fn, flags);
  if (entries && (flags & PMF_DEBATCH_FILL_MISSING)) return pmf_fail("%s: PMF_DEBATCH_FILL_MISSING is not accepted here (predictions at entries: pmf_impute_entries)", fn);
  if (resident && !c->D) return pmf_fail("%s: a null input means the resident data matrix (data not set)", fn);
  return outputs_ready(c, fn);
}

// rows [row0, row1) (0-based) of Z_dev (column-major from row0, leading dimension ldz; null: the resident D) into out_dev;
// prepare() has run.  FILL_MISSING: pmf_impute_kernel writes the batch-free prediction first, then only observed entries are stored.
static int debatch_launch(pmf_ctx *c, int flags, int64_t row0, int64_t row1, const float *Z_dev, int64_t ldz, float *out_dev, int64_t ld) {
  if (flags & PMF_DEBATCH_FILL_MISSING)
    PMFCHK(impute_launch(c, (flags & PMF_DEBATCH_LINK) ? PMF_IMPUTE_LINK : 0, row0, row1, out_dev, ld));
  DebatchArgs a;
  memset(&a, 0, sizeof(a));
  a.Z = Z_dev ? (const void *)Z_dev : (const void *)c->D.p; a.ldz = ldz; a.nRB = c->nRB;
  a.colp = c->colp; a.bor = c->bor; a.btab = c->btab; a.views = c->d_views;
  a.out = out_dev; a.ld = ld; a.M = c->M; a.N = c->N; a.row0 = row0; a.row1 = row1;
  a.rb0 = row0 / 32;
  a.n_rb = (row1 - 1) / 32 + 1 - a.rb0;
  a.n_ct = (c->N + PMF_BN - 1) / PMF_BN;
  a.n_bv = c->n_bv; a.flags = flags;
  if (a.n_rb * a.n_ct >= (1ll << 31)) return pmf_fail("pmf_remove_batch_effect: too many tiles in one call (split the row range)");
  return pmf_launch_debatch(c->stream, Z_dev ? 2 : (c->store == PMF_STORE_BF16 ? 1 : 0), c->n_cu, a);
}

extern "C" int pmf_remove_batch_effect_device(pmf_ctx *c, int flags, int64_t row_start1, int64_t row_stop1, const float *Z_device,
                                              int64_t ldz, float *out_device, int64_t ld) {
  static const char *fn = "pmf_remove_batch_effect_device";
  PMFCHK(ctx_bind(c));
  PMFCHK(debatch_check(c, fn, flags, !Z_device, out_device, false));
  PMFCHK(impute_check_range(c, fn, row_start1, row_stop1, ld));
  const int64_t rows = row_stop1 - row_start1 + 1;
  if (Z_device) {
    if (ldz < rows) return pmf_fail("%s: ldz=%lld is below the row count %lld", fn, (long long)ldz, (long long)rows);
    const float *ze = Z_device + pmf_impute_off(rows, c->N - 1, ldz), *oe = out_device + pmf_impute_off(rows, c->N - 1, ld);
    const bool in_place = Z_device == out_device && ldz == ld && !(flags & PMF_DEBATCH_FILL_MISSING);
    if (Z_device < oe && out_device < ze && !in_place)
      return pmf_fail("%s: input and output overlap (in place needs Z == out, ldz == ld and no PMF_DEBATCH_FILL_MISSING)", fn);
  }
  PMFCHK(prepare(c));
  PMFCHK(debatch_launch(c, flags, row_start1 - 1, row_stop1, Z_device, ldz, out_device, ld));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int pmf_remove_batch_effect(pmf_ctx *c, int flags, int64_t row_start1, int64_t row_stop1, const float *Z_host, int64_t ldz,
                                       float *out_host, int64_t ld) {
  static const char *fn = "pmf_remove_batch_effect";
  PMFCHK(ctx_bind(c));
  PMFCHK(debatch_check(c, fn, flags, !Z_host, out_host, false));
  PMFCHK(impute_check_range(c, fn, row_start1, row_stop1, ld));
  const int64_t rows = row_stop1 - row_start1 + 1;
  if (Z_host && ldz < rows) return pmf_fail("%s: ldz=%lld is below the row count %lld", fn, (long long)ldz, (long long)rows);
  // the prediction of FILL_MISSING must not land on a host input's chunk: then the staging buffer holds an input and an
  // output part; otherwise the chunk is corrected in place
  const int parts = Z_host && (flags & PMF_DEBATCH_FILL_MISSING) ? 2 : 1;
  return staged_rows(c, row_start1 - 1, row_stop1, parts, "PMF_DEBATCH_CHUNK_ROWS", Z_host, ldz, out_host, ld,
                     [&](int64_t r0, int64_t r1, const float *s_in, float *s_out, int64_t nr) { return debatch_launch(c, flags, r0, r1, s_in, nr, s_out, nr); });
}

extern "C" int pmf_remove_batch_effect_entries(pmf_ctx *c, int flags, int64_t n, const int64_t *rows1, const int64_t *cols1,
                                               const float *values, float *out_host) {
  static const char *fn = "pmf_remove_batch_effect_entries";
  return staged_entries(c, fn, n, rows1, cols1, values, out_host, [&] { return debatch_check(c, fn, flags, !values, out_host, true); },
                        [&](const int64_t *d_rows, const int64_t *d_cols, const float *d_val, float *d_out, int64_t ne) {
                          DebatchEntriesArgs a;
                          memset(&a, 0, sizeof(a));
                          a.values = d_val; a.D = c->D.p; a.nRB = c->nRB; a.d_bf16 = c->store == PMF_STORE_BF16; a.n_bv = c->n_bv;
                          a.colp = c->colp; a.bor = c->bor; a.btab = c->btab; a.views = c->d_views;
                          a.rows1 = d_rows; a.cols1 = d_cols; a.out = d_out; a.n = ne; a.M = c->M; a.flags = flags;
                          return pmf_launch_debatch_entries(c->stream, a);
                        });
}
