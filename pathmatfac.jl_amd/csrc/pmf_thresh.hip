// pmf_thresh.hip -- host side of the trainable squared-hinge thresholds (include/pmf_hip_thresholds.h): the groups of the
// noise model, the threshold pass and its geometry, the thresholds' optimizer step inside pmf_fit, class counts.
// The kernels are in pmf_k_thresh.hip (pmf_thresh.hip.inc).
#include "../../include/pmf_hip_thresholds.h"
#include "pmf_ctx.h"
#include "pmf_thresh.h"

// the noise ranges whose columns are all of kind 3, in the order pmf_set_noise got them
static void thresh_groups(const pmf_ctx *c, std::vector<int64_t> &s1, std::vector<int64_t> &e1) {
  s1.clear(); e1.clear();
  if ((int64_t)c->h_kind.size() != c->N) return;
  for (size_t r = 0; r < c->noise_s1.size(); ++r) {
    bool all3 = true;
    for (int64_t j = c->noise_s1[r] - 1; j < c->noise_e1[r] && all3; ++j) all3 = c->h_kind[(size_t)j] == PMF_NOISE_SQ_HINGE;
    if (all3) { s1.push_back(c->noise_s1[r]); e1.push_back(c->noise_e1[r]); }
  }
}

// Brings the groups' device state up to date with the noise model: the maps (tile list, column -> group, group bounds), the
// triples (from h_thr: the host may have set new ones) and, when the groups changed, a reset optimizer state.
static int thresh_sync(pmf_ctx *c) {
  ThreshState &t = c->th;
  std::vector<int64_t> s1, e1;
  thresh_groups(c, s1, e1);
  const size_t ng = s1.size();
  if (s1 != t.g_s1 || e1 != t.g_e1 || t.t.size() < 3 * ng) {
    t.g_s1 = s1; t.g_e1 = e1;
    t.state_init = false;
    PMFCHK(t.t.alloc(3 * ng, true, "the threshold groups"));
    PMFCHK(t.acc.alloc(3 * ng, true, "the threshold groups"));
    PMFCHK(t.mom.alloc(3 * ng, true, "the threshold groups"));
    PMFCHK(t.G.alloc(3 * ng, true, "the threshold groups"));
    PMFCHK(t.g_c0.alloc(ng, true, "the threshold groups"));
    PMFCHK(t.g_c1.alloc(ng, true, "the threshold groups"));
  }
  t.h_tiles.clear();
  if (ng == 0) return 0;
  std::vector<int32_t> cg((size_t)c->N, -1);
  std::vector<int64_t> c0(ng), c1(ng);
  std::vector<float> tt(3 * ng);
  for (size_t r = 0; r < ng; ++r) {
    c0[r] = s1[r] - 1; c1[r] = e1[r];
    for (int64_t j = c0[r]; j < c1[r]; ++j) cg[(size_t)j] = (int32_t)r;
    for (int m = 0; m < 3; ++m) tt[3 * r + m] = c->h_thr[(size_t)c0[r] * 3 + m];
  }
  for (int64_t ct = 0; ct < (c->N + PMF_BN - 1) / PMF_BN; ++ct) {
    bool any = false;
    for (int64_t j = ct * PMF_BN; j < std::min<int64_t>(c->N, (ct + 1) * PMF_BN) && !any; ++j) any = c->h_kind[(size_t)j] == PMF_NOISE_SQ_HINGE;
    if (any) t.h_tiles.push_back((int32_t)ct);
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  PMFCHK(t.tiles.ensure(t.h_tiles.size(), false, "the threshold pass"));
  PMFCHK(t.col_group.ensure((size_t)c->N, false, "the threshold pass"));
  PMFCHK(t.gcol.ensure(3 * (size_t)c->N, true, "the threshold pass"));
  PMFCHK(t.tiles.upload(t.h_tiles.data(), t.h_tiles.size()));
  PMFCHK(t.col_group.upload(cg.data(), cg.size()));
  PMFCHK(t.g_c0.upload(c0.data(), ng));
  PMFCHK(t.g_c1.upload(c1.data(), ng));
  return t.t.upload(tt.data(), tt.size());
}

static int thresh_init_state(pmf_ctx *c) {
  ThreshState &t = c->th;
  const size_t n = 3 * t.g_s1.size();
  std::vector<float> a(n, c->opt_kind == PMF_OPT_ADAGRAD ? c->eps : 0.f), z(n, 0.f);
  HIPCHK(hipStreamSynchronize(c->stream));
  PMFCHK(t.acc.upload(a.data(), n));
  PMFCHK(t.mom.upload(z.data(), n));
  t.bp1 = c->b1; t.bp2 = c->b2;
  t.state_init = true;
  return 0;
}

// what the pass itself cannot run on
static int thresh_pass_check(pmf_ctx *c) {
  if (c->KB < 1 || c->KB > 4) return pmf_fail("the threshold pass is built for K <= 128 (K = %d)", c->K);
  if (c->n_bv > 0 && !c->btd_ok) return pmf_fail("the threshold pass needs the dense batch table (a batch view has more than 255 batches)");
  const int nbs = c->n_bv > 0 ? c->nbs : 16;
  if (pmf_thresh_pass_lds(c->KB, pmf_thresh_waves(c->KB), nbs) > 160 * 1024)
    return pmf_fail("too many row batches per view (%d slots) for the threshold pass", nbs);
  if (!c->htab || !c->thr) return pmf_fail("internal: the threshold tables are not allocated");
  return 0;
}

int thresh_pass(pmf_ctx *c) {
  ThreshState &t = c->th;
  const int nw = pmf_thresh_waves(c->KB);
  const int nbs = c->n_bv > 0 ? c->nbs : 16;
  int nbs_shift = 0;
  while ((1 << nbs_shift) < nbs) ++nbs_shift;
  const int64_t n_tiles = (int64_t)t.h_tiles.size(), n_rp = (c->M + 32 * nw - 1) / (32 * nw);
  // row ranges: enough units to fill the device a few times over while the tiles alone do not
  int64_t R = std::max<int64_t>(1, std::min<int64_t>(n_rp, (4ll * c->n_cu + n_tiles - 1) / n_tiles));
  const char *re = getenv("PMF_THRESH_RANGES");   // test hook, read at every pass: caps the row ranges so that small shapes sweep several panels per unit
  if (re && atoi(re) > 0) R = std::min<int64_t>(R, atoi(re));
  int grid = (int)std::min<int64_t>(n_tiles * R, c->n_cu);
  const char *ge = getenv("PMF_THRESH_GRID");   // test hook, read at every pass: caps the grid so that small shapes reach the unit loop
  if (ge && atoi(ge) > 0) grid = std::min(grid, atoi(ge));
  PMFCHK(t.slots.ensure((size_t)(R * nw * n_tiles * PMF_TSLOT), false, "the threshold pass"));
  ThreshPassArgs a;
  memset(&a, 0, sizeof(a));
  a.D = c->D; a.d_bf16 = c->store == PMF_STORE_BF16; a.nRB = c->nRB; a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.htab = c->htab;
  a.bor = c->bor; a.btd = c->n_bv > 0 ? c->btd : nullptr; a.tiles = t.tiles; a.slots = t.slots;
  a.M = c->M; a.N = c->N; a.n_bv = c->n_bv; a.n_tiles = (int)n_tiles; a.n_rp = (int)n_rp; a.R = (int)R; a.nbs_shift = nbs_shift;
  PMFCHK(pmf_launch_thresh_pass(&c->dyn_lds, c->stream, c->KB, grid, a));
  ThreshReduceArgs r;
  memset(&r, 0, sizeof(r));
  r.slots = t.slots; r.tiles = t.tiles; r.thr = c->thr; r.n_tiles = (int)n_tiles; r.n_parts = (int)(R * nw); r.N = c->N;
  r.gcol = t.gcol; r.g_c0 = t.g_c0; r.g_c1 = t.g_c1; r.n_groups = (int)t.g_s1.size(); r.G = t.G;
  PMFCHK(pmf_launch_thresh_reduce(c->stream, r));
  t.n_tiles = (int)n_tiles; t.n_units = (int)(n_tiles * R); t.grid = grid;
  t.passes++;
  return 0;
}

int thresh_fit_check(pmf_ctx *c, bool *active) {
  *active = false;
  if (!c->th.train) return 0;
  std::vector<int64_t> s1, e1;
  thresh_groups(c, s1, e1);
  if (s1.empty()) return 0;
  for (size_t r = 0; r < s1.size(); ++r)
    for (int64_t j = s1[r]; j < e1[r]; ++j)   // (0-based column j against the range's first, s1[r] - 1)
      if (memcmp(&c->h_thr[(size_t)j * 3], &c->h_thr[(size_t)(s1[r] - 1) * 3], 3 * sizeof(float)) != 0)
        return pmf_fail("threshold training: the columns of noise range %lld:%lld do not all hold the same thresholds (column %lld differs from column %lld)",
                        (long long)s1[r], (long long)e1[r], (long long)(j + 1), (long long)s1[r]);
  PMFCHK(thresh_sync(c));
  *active = true;
  return 0;
}

int thresh_fit_begin(pmf_ctx *c) {
  PMFCHK(thresh_pass_check(c));
  if (!c->th.state_init) PMFCHK(thresh_init_state(c));
  return 0;
}

int thresh_step(pmf_ctx *c) {
  ThreshState &t = c->th;
  ThreshStepArgs s;
  memset(&s, 0, sizeof(s));
  s.t = t.t; s.acc = t.acc; s.mom = t.mom; s.G = t.G; s.n_groups = (int)t.g_s1.size();
  s.opt_kind = c->opt_kind; s.lr = c->lr; s.eps = c->eps; s.b1 = c->b1; s.b2 = c->b2;
  s.c1 = 1.f - t.bp1; s.c2 = 1.f - t.bp2;
  PMFCHK(pmf_launch_thresh_step(c->stream, s));
  if (c->opt_kind == PMF_OPT_ADAM) { t.bp1 *= c->b1; t.bp2 *= c->b2; }
  ThreshImageArgs im;
  memset(&im, 0, sizeof(im));
  im.t = t.t; im.col_group = t.col_group; im.N = c->N; im.thr = c->thr; im.htab = c->htab;
  return pmf_launch_thresh_images(c->stream, im);
}

int thresh_fit_end(pmf_ctx *c) {
  ThreshState &t = c->th;
  const size_t ng = t.g_s1.size();
  std::vector<float> tt(3 * ng);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (ng) HIPCHK(hipMemcpy(tt.data(), t.t, sizeof(float) * 3 * ng, hipMemcpyDeviceToHost));
  for (size_t r = 0; r < ng; ++r)
    for (int64_t j = t.g_s1[r] - 1; j < t.g_e1[r]; ++j)
      for (int m = 0; m < 3; ++m) c->h_thr[(size_t)j * 3 + m] = tt[3 * r + m];
  return 0;
}

// ---- C ABI --------------------------------------------------------------------------------------
extern "C" int pmf_set_threshold_training(pmf_ctx *c, int on) {
  PMFCHK(ctx_bind(c));
  c->th.train = on != 0;
  return 0;
}

extern "C" int pmf_get_threshold_groups(pmf_ctx *c, int *n_groups, int64_t *starts1, int64_t *stops1, int cap) {
  PMFCHK(ctx_bind(c));
  std::vector<int64_t> s1, e1;
  thresh_groups(c, s1, e1);
  if (n_groups) *n_groups = (int)s1.size();
  for (int r = 0; r < cap && r < (int)s1.size(); ++r) {
    if (starts1) starts1[r] = s1[(size_t)r];
    if (stops1) stops1[r] = e1[(size_t)r];
  }
  return 0;
}

extern "C" int pmf_threshold_grad(pmf_ctx *c, float *g_group, float *g_col) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  PMFCHK(thresh_sync(c));
  ThreshState &t = c->th;
  const size_t ng = t.g_s1.size();
  if (g_col)
    for (int64_t e = 0; e < 3 * c->N; ++e) g_col[e] = NAN;
  if (t.h_tiles.empty()) return 0;   // no kind-3 column: nothing is launched
  if (!c->prepared) PMFCHK(prepare(c));
  PMFCHK(thresh_pass_check(c));
  PMFCHK(thresh_pass(c));
  std::vector<double> G(3 * ng), gc(g_col ? 3 * (size_t)c->N : 0);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (ng) HIPCHK(hipMemcpy(G.data(), t.G, sizeof(double) * G.size(), hipMemcpyDeviceToHost));
  if (g_group)
    for (size_t e = 0; e < G.size(); ++e) g_group[e] = (float)G[e];
  if (g_col) {
    HIPCHK(hipMemcpy(gc.data(), t.gcol, sizeof(double) * gc.size(), hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < c->N; ++j)
      if (c->h_kind[(size_t)j] == PMF_NOISE_SQ_HINGE)
        for (int m = 0; m < 3; ++m) g_col[3 * j + m] = (float)gc[(size_t)(3 * j + m)];
  }
  return 0;
}

extern "C" int pmf_get_threshold_state(pmf_ctx *c, float *thr, float *acc, float *mom) {
  PMFCHK(ctx_bind(c));
  if (c->N == 0 || (int64_t)c->h_thr.size() != 3 * c->N) return pmf_fail("the noise model is not set");
  PMFCHK(thresh_sync(c));
  ThreshState &t = c->th;
  const size_t n = 3 * t.g_s1.size();
  if (n == 0) return 0;
  if (!t.state_init) PMFCHK(thresh_init_state(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (thr) HIPCHK(hipMemcpy(thr, t.t, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (acc) HIPCHK(hipMemcpy(acc, t.acc, sizeof(float) * n, hipMemcpyDeviceToHost));
  if (mom) HIPCHK(hipMemcpy(mom, t.mom, sizeof(float) * n, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int pmf_class_counts(pmf_ctx *c, int n_ranges, const int64_t *s1, const int64_t *e1, int64_t *counts) {
  PMFCHK(ctx_bind(c));
  if (!c->D) return pmf_fail("data not set");
  if (n_ranges < 0 || (n_ranges > 0 && (!s1 || !e1 || !counts))) return pmf_fail("pmf_class_counts: null argument");
  if (n_ranges == 0) return 0;
  std::vector<int64_t> c0((size_t)n_ranges), c1((size_t)n_ranges);
  for (int r = 0; r < n_ranges; ++r) {
    if (s1[r] < 1 || e1[r] > c->N || s1[r] > e1[r]) return pmf_fail("class-count range %d: bad columns %lld:%lld", r, (long long)s1[r], (long long)e1[r]);
    c0[(size_t)r] = s1[r] - 1; c1[(size_t)r] = e1[r];
  }
  DevBuf<int64_t> d0, d1;
  DevBuf<unsigned long long> dc;
  HIPCHK(hipStreamSynchronize(c->stream));
  PMFCHK(upload_new(d0, c0.data(), c0.size()));
  PMFCHK(upload_new(d1, c1.data(), c1.size()));
  PMFCHK(dc.alloc(4 * (size_t)n_ranges, true, "the class counts"));
  ClassCountArgs a;
  memset(&a, 0, sizeof(a));
  a.D = c->D; a.d_bf16 = c->store == PMF_STORE_BF16; a.nRB = c->nRB; a.M = c->M; a.N = c->N; a.c0 = d0; a.c1 = d1; a.n_ranges = n_ranges;
  // enough waves to fill the device, at least 256 rows each; a wave's 32-bit counts hold 64 x 2^20 entries with room to spare
  const int64_t gx = (c->N + 63) / 64;
  a.row_chunks = (int)std::max<int64_t>(std::max<int64_t>(1, (c->M + (1 << 20) - 1) >> 20),
                                        std::min<int64_t>((32ll * c->n_cu + gx - 1) / gx, (c->M + 255) / 256));
  a.row_chunks = std::min(a.row_chunks, 65535);
  a.counts = dc;
  PMFCHK(pmf_launch_class_counts(c->stream, a));
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(counts, dc, sizeof(int64_t) * 4 * (size_t)n_ranges, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int pmf_debug_threshold_pass(pmf_ctx *c, int *n_tiles, int *n_units, int *grid, int64_t *passes) {
  PMFCHK(ctx_bind(c));
  if (n_tiles) *n_tiles = c->th.n_tiles;
  if (n_units) *n_units = c->th.n_units;
  if (grid) *grid = c->th.grid;
  if (passes) *passes = c->th.passes;
  return 0;
}
