// pmf_holdout.hip -- hold-out entries (include/pmf_hip_holdout.h): the set beside the resident data, the hold-out loss, and
// what pmf_fit's loop calls for tracking, early stopping and best-parameter restore.
#include <numeric>

#include "../../include/pmf_hip_holdout.h"
#include "pmf_ctx.h"
#include "pmf_holdout.h"

static int env_int(const char *name) {
  const char *e = getenv(name);
  return e && atoi(e) > 0 ? atoi(e) : 0;
}
// a wave per column (k_holdout_d, k_holdout_colsum): enough workgroups of four waves for N, at most eight per CU
static int column_grid(const pmf_ctx *c) { return (int)std::max<int64_t>(1, std::min<int64_t>((c->N + 3) / 4, 8ll * c->n_cu)); }

// D changed under the caches made from it: the per-tile all-finite flags, and with them the plain-run table
// (ensure_tile_flags), exactly as after a new upload
static void d_changed(pmf_ctx *c) { c->tflags_valid = false; }

static void holdout_forget(pmf_ctx *c) {
  HoldoutState &h = c->ho;
  h.n = 0;
  h.h_colptr.clear();
  h.colptr.free(); h.rows.free(); h.vals.free(); h.u_col.free(); h.u_cnt.free(); h.u_e0.free(); h.lbuf.free(); h.loss_col.free(); h.d_total.free();
  h.unit_cap = 0;
}
void holdout_drop(pmf_ctx *c) { holdout_forget(c); }

static int launch_d(pmf_ctx *c, int mode) {
  HoldoutState &h = c->ho;
  HoldoutDArgs a;
  memset(&a, 0, sizeof(a));
  a.D = c->D.p; a.d_bf16 = c->store == PMF_STORE_BF16; a.mode = mode; a.nRB = c->nRB; a.N = c->N;
  a.colptr = h.colptr; a.rows = h.rows; a.vals = h.vals;
  return pmf_launch_holdout_d(c->stream, column_grid(c), a);
}

// the device copy of a sorted set: column pointers and rows (vals allocated, not filled)
static int upload_set(pmf_ctx *c, const std::vector<int64_t> &colptr, const std::vector<int32_t> &rows) {
  HoldoutState &h = c->ho;
  PMFCHK(upload_new(h.colptr, colptr.data(), colptr.size()));
  PMFCHK(upload_new(h.rows, rows.data(), rows.size()));
  PMFCHK(h.vals.alloc(rows.size(), false, "the held values"));
  return 0;
}

extern "C" int pmf_set_holdout(pmf_ctx *c, int64_t n, const int64_t *rows1, const int64_t *cols1, int64_t *n_held) {
  static const char *fn = "pmf_set_holdout";
  PMFCHK(ctx_bind(c));
  if (n_held) *n_held = 0;
  if (!c->D || c->M <= 0 || c->N <= 0) return pmf_fail("%s: data not set", fn);
  if (c->ho.n > 0) return pmf_fail("%s: a hold-out set of %lld entries is already present (pmf_clear_holdout first)", fn, (long long)c->ho.n);
  if (n < 0) return pmf_fail("%s: n=%lld", fn, (long long)n);
  if (n == 0) return 0;
  if (!rows1 || !cols1) return pmf_fail("%s: null index pointer", fn);
  const int64_t M = c->M, N = c->N;
  for (int64_t e = 0; e < n; ++e)
    if (rows1[e] < 1 || rows1[e] > M || cols1[e] < 1 || cols1[e] > N)
      return pmf_fail("%s: entry %lld = (%lld, %lld) is outside 1..%lld x 1..%lld", fn, (long long)e, (long long)rows1[e], (long long)cols1[e],
                      (long long)M, (long long)N);
  // sort by (column, row): the key is the entry's column-major position; ties keep the caller's order
  std::vector<int64_t> ord((size_t)n);
  std::iota(ord.begin(), ord.end(), (int64_t)0);
  auto key = [&](int64_t e) { return (cols1[e] - 1) * M + (rows1[e] - 1); };
  std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { const int64_t ka = key(a), kb = key(b); return ka != kb ? ka < kb : a < b; });
  int64_t dup = -1;   // the first entry, in the caller's order, that repeats an earlier one
  for (int64_t q = 1; q < n; ++q)
    if (key(ord[(size_t)q]) == key(ord[(size_t)q - 1]) && (dup < 0 || ord[(size_t)q] < dup)) dup = ord[(size_t)q];
  if (dup >= 0)
    return pmf_fail("%s: entry %lld = (%lld, %lld) is a duplicate of an earlier entry", fn, (long long)dup, (long long)rows1[dup], (long long)cols1[dup]);
  std::vector<int64_t> colptr((size_t)N + 1, 0);
  std::vector<int32_t> rows((size_t)n);
  for (int64_t q = 0; q < n; ++q) {
    const int64_t e = ord[(size_t)q];
    rows[(size_t)q] = (int32_t)(rows1[e] - 1);
    colptr[(size_t)cols1[e]]++;
  }
  for (int64_t j = 0; j < N; ++j) colptr[(size_t)j + 1] += colptr[(size_t)j];
  // the values D holds there; what is missing already leaves the set
  HoldoutState &h = c->ho;
  std::vector<float> vals((size_t)n);
  int rc = upload_set(c, colptr, rows);
  if (rc == 0) rc = launch_d(c, PMF_HOLDOUT_D_GATHER);
  if (rc == 0) {
    hipError_t e = hipMemcpyAsync(vals.data(), h.vals, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = pmf_fail("%s: reading the held values failed: %s", fn, hipGetErrorString(e));
  }
  if (rc < 0) { holdout_forget(c); return rc; }
  int64_t kept = 0;
  {
    std::vector<int64_t> cp2((size_t)N + 1, 0);
    for (int64_t j = 0; j < N; ++j) {
      for (int64_t q = colptr[(size_t)j]; q < colptr[(size_t)j + 1]; ++q)
        if (std::isfinite(vals[(size_t)q])) { rows[(size_t)kept] = rows[(size_t)q]; vals[(size_t)kept] = vals[(size_t)q]; ++kept; }
      cp2[(size_t)j + 1] = kept;
    }
    colptr.swap(cp2);
  }
  if (kept == 0) { holdout_forget(c); return 0; }
  if (kept != n) {
    rows.resize((size_t)kept);
    rc = upload_set(c, colptr, rows);
  }
  if (rc == 0 && kept != n) rc = h.vals.upload(vals.data(), (size_t)kept);
  if (rc == 0) rc = h.loss_col.alloc((size_t)N, true, "the hold-out column losses");
  if (rc == 0) rc = h.lbuf.alloc((size_t)kept, false, "the hold-out entry losses");
  if (rc == 0) rc = h.d_total.alloc(1, true, "the hold-out loss");
  if (rc < 0) { holdout_forget(c); return rc; }   // (D has not been written yet)
  h.n = kept;
  h.h_colptr = colptr;
  PMFCHK(launch_d(c, PMF_HOLDOUT_D_BLANK));
  d_changed(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (n_held) *n_held = kept;
  return 0;
}

extern "C" int pmf_clear_holdout(pmf_ctx *c, int restore) {
  PMFCHK(ctx_bind(c));
  if (c->ho.n > 0 && restore) {
    if (!c->D) return pmf_fail("pmf_clear_holdout: data not set");
    PMFCHK(launch_d(c, PMF_HOLDOUT_D_RESTORE));
    d_changed(c);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  holdout_forget(c);
  return 0;
}

extern "C" int pmf_get_holdout(pmf_ctx *c, int64_t *n, int64_t *rows1, int64_t *cols1, float *values, int64_t cap) {
  PMFCHK(ctx_bind(c));
  HoldoutState &h = c->ho;
  if (n) *n = h.n;
  const int64_t m = std::min(h.n, cap);
  if (m <= 0) return 0;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rows1) {
    std::vector<int32_t> r((size_t)m);
    HIPCHK(hipMemcpy(r.data(), h.rows, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    for (int64_t e = 0; e < m; ++e) rows1[e] = (int64_t)r[(size_t)e] + 1;
  }
  if (cols1)
    for (int64_t j = 0; j < c->N; ++j)
      for (int64_t e = h.h_colptr[(size_t)j]; e < std::min(m, h.h_colptr[(size_t)j + 1]); ++e) cols1[e] = j + 1;
  if (values) HIPCHK(hipMemcpy(values, h.vals, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
  return 0;
}

// the unit table for units of at most `cap` entries: a column's segment cut from its first entry on
static int ensure_units(pmf_ctx *c) {
  HoldoutState &h = c->ho;
  const int env = env_int("PMF_HOLDOUT_UNIT");
  const int cap = env > 0 ? env : PMF_HOLDOUT_UNIT_DEFAULT;
  if (h.unit_cap == cap) return 0;
  std::vector<int32_t> u_col, u_cnt;
  std::vector<int64_t> u_e0;
  for (int64_t j = 0; j < c->N; ++j)
    for (int64_t e = h.h_colptr[(size_t)j]; e < h.h_colptr[(size_t)j + 1]; e += cap) {
      u_col.push_back((int32_t)j);
      u_e0.push_back(e);
      u_cnt.push_back((int32_t)std::min<int64_t>(cap, h.h_colptr[(size_t)j + 1] - e));
    }
  if (u_col.size() > 0x7fffffffu) return pmf_fail("hold-out pass: too many work units (raise PMF_HOLDOUT_UNIT)");
  HIPCHK(hipStreamSynchronize(c->stream));   // (a pass that reads the old table may be running)
  PMFCHK(upload_new(h.u_col, u_col.data(), u_col.size()));
  PMFCHK(upload_new(h.u_cnt, u_cnt.data(), u_cnt.size()));
  PMFCHK(upload_new(h.u_e0, u_e0.data(), u_e0.size()));
  h.n_units = (int)u_col.size();
  h.unit_cap = cap;
  return 0;
}

int holdout_pass(pmf_ctx *c, double *d_total) {
  HoldoutState &h = c->ho;
  PMFCHK(ensure_units(c));
  const int grid_cap = env_int("PMF_HOLDOUT_GRID");
  int grid = (int)std::min<int64_t>(((int64_t)h.n_units + 3) / 4, 8ll * c->n_cu);
  if (grid_cap > 0) grid = std::min(grid, grid_cap);
  grid = std::max(grid, 1);
  HoldoutPassArgs a;
  memset(&a, 0, sizeof(a));
  a.X = c->P[0].p; a.Y = c->P[1].p; a.colp = c->colp; a.htab = c->htab; a.bor = c->bor; a.btab = c->btab; a.views = c->d_views;
  a.rows = h.rows; a.vals = h.vals; a.u_col = h.u_col; a.u_cnt = h.u_cnt; a.u_e0 = h.u_e0; a.lbuf = h.lbuf;
  a.M = c->M; a.n_units = h.n_units; a.n_bv = c->n_bv; a.Kp = c->Kp;
  PMFCHK(pmf_launch_holdout_pass(c->stream, grid, a));
  HoldoutSumArgs s;
  memset(&s, 0, sizeof(s));
  s.lbuf = h.lbuf; s.colptr = h.colptr; s.N = c->N; s.loss_col = h.loss_col; s.total = d_total;
  PMFCHK(pmf_launch_holdout_sums(c->stream, grid_cap > 0 ? std::min(column_grid(c), grid_cap) : column_grid(c), s));
  h.grid = grid;
  h.passes++;
  return 0;
}

extern "C" int pmf_holdout_loss(pmf_ctx *c, double *total, double *loss_col, int64_t *n_col) {
  PMFCHK(ctx_bind(c));
  PMFCHK(check_ready(c));
  HoldoutState &h = c->ho;
  if (total) *total = 0.0;
  if (h.n == 0) {
    for (int64_t j = 0; j < c->N; ++j) {
      if (loss_col) loss_col[j] = 0.0;
      if (n_col) n_col[j] = 0;
    }
    return 0;
  }
  PMFCHK(prepare(c));   // the column and batch tables of the current layer parameters (as pmf_impute_entries)
  PMFCHK(holdout_pass(c, h.d_total));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (total) HIPCHK(hipMemcpy(total, h.d_total, sizeof(double), hipMemcpyDeviceToHost));
  if (loss_col) HIPCHK(hipMemcpy(loss_col, h.loss_col, sizeof(double) * (size_t)c->N, hipMemcpyDeviceToHost));
  if (n_col)
    for (int64_t j = 0; j < c->N; ++j) n_col[j] = h.h_colptr[(size_t)j + 1] - h.h_colptr[(size_t)j];
  return 0;
}

extern "C" int pmf_debug_holdout_pass(pmf_ctx *c, int *n_units, int *grid, int64_t *passes) {
  PMFCHK(ctx_bind(c));
  if (n_units) *n_units = c->ho.n_units;
  if (grid) *grid = c->ho.grid;
  if (passes) *passes = c->ho.passes;
  return 0;
}

// ---- tracking inside pmf_fit ----------------------------------------------------------------------
extern "C" int pmf_set_holdout_tracking(pmf_ctx *c, const pmf_holdout_opts *o) {
  PMFCHK(ctx_bind(c));
  HoldoutState &h = c->ho;
  if (!o || o->every == 0) { h.every = h.patience = h.restore_best = 0; h.min_delta = 0.0; return 0; }
  if (o->every < 0 || o->patience < 0) return pmf_fail("pmf_set_holdout_tracking: every=%d, patience=%d must not be negative", o->every, o->patience);
  if (!(o->min_delta >= 0.0) || !std::isfinite(o->min_delta)) return pmf_fail("pmf_set_holdout_tracking: min_delta=%g must be finite and >= 0", o->min_delta);
  h.every = o->every; h.patience = o->patience; h.restore_best = o->restore_best != 0; h.min_delta = o->min_delta;
  return 0;
}

extern "C" int pmf_get_holdout_trace(pmf_ctx *c, int *n, int *best_epoch, double *best_loss, int32_t *epochs, double *losses, int cap) {
  PMFCHK(ctx_bind(c));
  const HoldoutState &h = c->ho;
  if (n) *n = (int)h.tr_epoch.size();
  if (best_epoch) *best_epoch = h.best_epoch;
  if (best_loss) *best_loss = h.best_loss;
  for (int e = 0; e < cap && e < (int)h.tr_epoch.size(); ++e) {
    if (epochs) epochs[e] = h.tr_epoch[(size_t)e];
    if (losses) losses[e] = h.tr_loss[(size_t)e];
  }
  return 0;
}

int holdout_fit_check(pmf_ctx *c, const pmf_fit_opts *o, bool th_on, bool *active) {
  HoldoutState &h = c->ho;
  *active = false;
  h.tr_epoch.clear(); h.tr_loss.clear();
  h.best_epoch = 0; h.best_loss = 0.0;
  if (h.every <= 0) return 0;
  // every rank holds the same switch and refuses alike, whatever its local set holds (a rank with no held entry in its rows
  // that went on alone would wait in its first collective for ranks that have returned)
  if (comm_active(c) && c->comm.nranks > 1)
    return pmf_fail("hold-out tracking is not supported with %d ranks (pmf_holdout_loss works per rank; turn tracking off: pmf_set_holdout_tracking(ctx, NULL))", c->comm.nranks);
  if (h.n == 0) return 0;
  if (h.restore_best && o->update_col_layers)
    return pmf_fail("hold-out tracking: restore_best is not supported together with update_col_layers (the layer parameters are not copied)");
  if (h.restore_best && th_on)
    return pmf_fail("hold-out tracking: restore_best is not supported together with threshold training (the thresholds are not copied)");
  PMFCHK(ensure_units(c));
  if (h.restore_best)
    for (int w = 0; w < 2; ++w)
      if (w == 0 ? o->update_X != 0 : o->update_Y != 0) {
        PMFCHK(h.cand[w].ensure((size_t)c->P[w].n, false, "the hold-out candidate factors"));
        PMFCHK(h.best[w].ensure((size_t)c->P[w].n, false, "the hold-out best factors"));
      }
  *active = true;
  return 0;
}

int holdout_fit_snapshot(pmf_ctx *c, bool ux, bool uy) {
  HoldoutState &h = c->ho;
  if (!h.restore_best) return 0;
  for (int w = 0; w < 2; ++w)
    if (w == 0 ? ux : uy)
      HIPCHK(hipMemcpyAsync(h.cand[w], c->P[w].p, sizeof(float) * (size_t)c->P[w].n, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

bool holdout_fit_record(pmf_ctx *c, int epoch, double H) {
  HoldoutState &h = c->ho;
  h.tr_epoch.push_back(epoch);
  h.tr_loss.push_back(H);
  const bool first = h.best_epoch == 0;
  if (first ? std::isfinite(H) : H < h.best_loss - h.min_delta) {
    h.best_epoch = epoch;
    h.best_loss = H;
    if (h.restore_best)   // (the candidate was copied at the top of this epoch, in stream order before the steps)
      for (int w = 0; w < 2; ++w) std::swap(h.cand[w], h.best[w]);
    return false;
  }
  // evaluations since the best one (or since the start, while none was finite)
  int bad = 0;
  for (size_t q = h.tr_epoch.size(); q-- > 0 && h.tr_epoch[q] != h.best_epoch;) ++bad;
  return h.patience > 0 && bad >= h.patience;
}

int holdout_fit_end(pmf_ctx *c, bool ux, bool uy) {
  HoldoutState &h = c->ho;
  if (!h.restore_best || h.best_epoch == 0) return 0;
  for (int w = 0; w < 2; ++w)
    if (w == 0 ? ux : uy)
      HIPCHK(hipMemcpyAsync(c->P[w].p, h.best[w], sizeof(float) * (size_t)c->P[w].n, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
