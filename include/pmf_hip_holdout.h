/*
 * pmf_hip_holdout.h -- hold-out entries: a validation set that lives on the device next to the resident data, its loss, and
 * tracking / early stopping / best-parameter restore inside pmf_fit.  An extension of include/pmf_hip.h (same conventions,
 * same library): every entry returns 0 on success, < 0 on error with the message in pmf_last_error().
 *
 * SELF-SPECIFIED (Deviation 7).
 *
 * THE SET.  pmf_set_holdout takes n 1-based entries (i, j) of the resident data matrix in any order.  The library sorts them
 * by (column, row), reads their values from the resident D (for PMF_STORE_BF16 the stored, already rounded value), keeps
 * them in a CSC-like device copy (column pointers, rows, values) and overwrites those entries of D with NaN.  Entries that
 * were already missing are dropped from the set.  From then on every entry of the library sees the held entries as missing:
 * nothing of them reaches a loss, a gradient, a statistic or a count.  pmf_clear_holdout drops the set, with restore != 0
 * after writing the kept values back (bitwise what D held before).  Whatever replaces the resident data (pmf_set_data,
 * pmf_set_data_device, pmf_simulate_data_resident, pmf_synth_data) drops the set WITHOUT write-back.
 *
 * THE LOSS.  For a held entry (i, j, y):
 *     z = fma(sigma_j a_ij, delta_v[b,j], mu_j + theta_v[b,j])     delta = 1, theta = 0 for a row in no batch or a column in
 *                                                                  no view: the link-space prediction of pmf_impute_entries
 *                                                                  with PMF_IMPUTE_BATCH | PMF_IMPUTE_LINK
 *     l = the per-entry loss of column j's noise model at (z, y) with the column's weight and current thresholds: the term
 *         the training loss sums over the observed entries
 * a_ij = sum_k X[k,i] Y[k,j] in float32: sixteen partial sums (partial s takes k = 4 s .. 4 s + 3, then 64 + 4 s .. in index
 * order, by fma) combined by a butterfly (s ^ 8, s ^ 4, s ^ 2, s ^ 1).  loss_col[j] is the float64 sum of l over column j's
 * entries: 64 partial sums (partial p takes the column's entries p, p + 64, ... in sorted order) combined by a butterfly
 * (p ^ 32 .. p ^ 1).  total is the float64 sum of loss_col over ascending j, one addition after the other.  Every order is
 * defined over entries and columns, never over workgroups: the results are bitwise the same from call to call and whatever
 * the launch geometry.  No float atomics.  Always exact f32, whatever pmf_set_precision says; local rows only, no collective;
 * nothing a later call could see is changed.
 *
 * TRACKING.  With pmf_set_holdout_tracking (sticky) on and a non-empty set, pmf_fit evaluates the hold-out loss H in every
 * epoch e with (e - opts->epoch) % every == 0, at the parameters that epoch's data pass saw (those the epoch's entry of the
 * loss trace belongs to); the value reaches the host with the epoch's own synchronisation.  An evaluation IMPROVES if
 * H < best - min_delta (the first finite H always does).  After `patience` > 0 consecutive evaluations without improvement
 * the fit ends with PMF_TERM_HOLDOUT; patience = 0 only records.  The existing termination checks run first and win in the
 * same epoch; the epoch's training loss, the loss trace and those checks are otherwise unchanged, and so are X, Y and the
 * optimizer state of a fit that does not stop early.
 * restore_best: at every evaluation epoch the factors this fit updates are copied (device to device) before they are stepped;
 * on improvement that copy becomes the best.  On return, whatever the term code, X and Y are those of the best epoch (as after
 * pmf_set_X / pmf_set_Y with them), provided at least one evaluation improved.  THE OPTIMIZER STATE IS NOT ROLLED BACK: it
 * is that of the last epoch run, and so is the virtual-node state of a network regularizer (the warm start of its solve,
 * pmf_get_reg_network_state), which is solved from the factors every epoch.
 * pmf_fit refuses, before anything is launched and leaving the context usable: restore_best together with
 * update_col_layers or with threshold training (those parameters are not copied), and tracking on a communicator of more than
 * one rank, whether or not the rank's own rows hold an entry of a set (pmf_holdout_loss itself works per rank).
 * pmf_fit_lbfgs and the pmf_epoch_* API do not track.
 * With no set and tracking off every result of the library is bitwise what it was.
 */
#ifndef PMF_HIP_HOLDOUT_H
#define PMF_HIP_HOLDOUT_H

#include "pmf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PMF_TERM_HOLDOUT 5   /* pmf_fit_result.term_code: `patience` evaluations of the hold-out loss without improvement */

typedef struct pmf_holdout_opts {
  int32_t every;          /* evaluate every `every` epochs, the fit's first epoch included; 0: tracking off */
  int32_t patience;       /* evaluations without improvement that end the fit; 0: record only */
  int32_t restore_best;   /* != 0: on return X, Y are those of the best evaluation epoch */
  int32_t reserved;
  double min_delta;       /* an evaluation improves if H < best - min_delta */
} pmf_holdout_opts;

/* Holds the n entries (rows1[e], cols1[e]) out of the resident data.  *n_held (may be NULL): how many were observed and are
 * now held.  Refused, with D untouched and the context usable: no data; an entry outside 1..M x 1..N; a duplicate (the
 * message names the first entry, in the caller's order, that repeats an earlier one); a set already present.  n = 0 is legal
 * and means no set; a call whose entries were all missing already leaves no set either. */
int pmf_set_holdout(pmf_ctx *ctx, int64_t n, const int64_t *rows1, const int64_t *cols1, int64_t *n_held);

/* drops the set; restore != 0: the kept values are written back to the resident D first.  No set: nothing happens. */
int pmf_clear_holdout(pmf_ctx *ctx, int restore);

/* *n = entries held; the first min(*n, cap) of them in sorted (column, row) order (any array may be NULL) */
int pmf_get_holdout(pmf_ctx *ctx, int64_t *n, int64_t *rows1, int64_t *cols1, float *values, int64_t cap);

/* The hold-out loss at the current parameters: *total, loss_col[N] (or NULL), n_col[N] (or NULL; exact).  Without a set all
 * of them are 0.  Refused without data or factors. */
int pmf_holdout_loss(pmf_ctx *ctx, double *total, double *loss_col, int64_t *n_col);

/* geometry of the last hold-out pass: work units, workgroups launched, and the passes run on this context so far.
 * PMF_HOLDOUT_GRID=n caps the workgroups, PMF_HOLDOUT_UNIT=n the entries of a work unit (a unit never crosses a column);
 * both are test hooks, read at every pass.  Any pointer may be NULL. */
int pmf_debug_holdout_pass(pmf_ctx *ctx, int *n_units, int *grid, int64_t *passes);

/* sticky; NULL or every = 0 turns tracking off */
int pmf_set_holdout_tracking(pmf_ctx *ctx, const pmf_holdout_opts *opts);

/* The evaluations of the last pmf_fit: *n of them, the first min(*n, cap) as (epochs[e], losses[e]); *best_epoch (0: no
 * evaluation improved) and *best_loss.  Any pointer may be NULL. */
int pmf_get_holdout_trace(pmf_ctx *ctx, int *n, int *best_epoch, double *best_loss, int32_t *epochs, double *losses, int cap);

#ifdef __cplusplus
}
#endif
#endif /* PMF_HIP_HOLDOUT_H */
