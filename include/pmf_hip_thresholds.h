/*
 * pmf_hip_thresholds.h -- trainable thresholds of the squared-hinge noise models, and their initialisation from class
 * counts.  An extension of include/pmf_hip.h (same conventions, same library): every entry returns 0 on success, < 0 on
 * error with the message in pmf_last_error().
 *
 * SELF-SPECIFIED (Deviation 5).  A column of kind PMF_NOISE_SQ_HINGE has thresholds t0 <= t1 <= t2; an
 * observed entry has class c = clamp((int)(y + 0.5), 0, 3), bounds lo / hi and the terms a = relu(1 - (z - lo)),
 * b = relu(1 - (hi - z)), an infinite bound contributing 0 (pmf_hip.h, pmf_set_noise_thresholds).  t_m is the upper bound
 * of class m and the lower bound of class m + 1, so per column j and m = 0..2
 *     g_t[m][j] = sum_i w_j (a_ij [c_ij = m + 1] - b_ij [c_ij = m])      over the finite entries of the local rows,
 * exactly 0 for an infinite t_m.
 *
 * GROUPS.  A trainable triple belongs to a noise RANGE, not to a column: every range of the last pmf_set_noise whose columns
 * are all of kind 3 is one group, in that order.  G[r][m] = sum_{j in r} g_t[m][j], summed in float64 over ascending
 * columns (and over the ranks of the library's communicator) and rounded once to float32.
 *
 * TRAINING.  With pmf_set_threshold_training(ctx, 1) and at least one group, every epoch of pmf_fit runs, after its data
 * pass and at the same pre-update parameters, one threshold pass; the thresholds then take the context's optimizer step
 * (AdaGrad or Adam: the formulas, lr and eps every other parameter gets; no regularizer term; one acc and one mom per
 * (group, m)).  Infinite thresholds are never stepped and their state never moves.  After the step order is restored (for
 * m = 0, 1: if t_m and t_{m+1} are finite and t_{m+1} < t_m then t_{m+1} = t_m) and the per-column images of the group's
 * columns are rebuilt on the device: no host round trip inside the epoch loop.  The epoch's loss and every termination rule
 * are unchanged.  pmf_fit refuses (before anything is launched; the context stays usable) a group whose columns do not all
 * hold the same triple.  On return pmf_get_noise_thresholds reports the trained values.  The thresholds' optimizer state
 * survives pmf_set_noise + pmf_set_noise_thresholds with the same groups and pmf_set_lr; pmf_set_optimizer,
 * pmf_reset_optimizer_state and a change of the groups reset it.  The threshold pass is always exact f32, whatever
 * pmf_set_precision says.  With training off (the default) every result of the library is bitwise what it was.
 * pmf_loss, pmf_fit_lbfgs and the step-level API pmf_epoch_* KEEP THE THRESHOLDS CONSTANT.
 */
#ifndef PMF_HIP_THRESHOLDS_H
#define PMF_HIP_THRESHOLDS_H

#include "pmf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sticky switch of the context, default 0 */
int pmf_set_threshold_training(pmf_ctx *ctx, int on);

/* the groups of the current noise model: *n_groups, and the first min(*n_groups, cap) 1-based inclusive column ranges
 * (starts1 / stops1 may be NULL with cap = 0) */
int pmf_get_threshold_groups(pmf_ctx *ctx, int *n_groups, int64_t *starts1, int64_t *stops1, int cap);

/* One threshold pass at the current parameters: g_group[3 r + m] = G[r][m] (local rows only: no collective), and, unless
 * NULL, g_col[3 j + m] = g_t[m][j], NaN for the columns that are not of kind 3.  Changes nothing and works with training
 * off; refused without data or factors.  Bitwise the same from call to call. */
int pmf_threshold_grad(pmf_ctx *ctx, float *g_group, float *g_col);

/* per group 3 floats each (any may be NULL): the thresholds and their optimizer state as the last training fit left them
 * (before the first one: the thresholds of the groups' first columns, acc / mom as a reset leaves them) */
int pmf_get_threshold_state(pmf_ctx *ctx, float *thr, float *acc, float *mom);

/* counts[4 r + c] = the observed entries of class c = clamp((int)(y + 0.5), 0, 3) in the columns starts1[r]..stops1[r] of
 * the LOCAL rows (exact 64-bit integers; the host sums over the ranks).  Any column ranges, whatever their noise kind. */
int pmf_class_counts(pmf_ctx *ctx, int n_ranges, const int64_t *starts1, const int64_t *stops1, int64_t *counts);

/* geometry of the last threshold pass: column tiles that hold a kind-3 column, units (tiles x row ranges), workgroups
 * launched (PMF_THRESH_GRID=n caps them), and the passes run on this context so far.  PMF_THRESH_RANGES=n caps the row
 * ranges R (units = tiles x R), so that a unit of a small problem sweeps several row panels.  Both are test hooks, read at
 * every pass.  Any pointer may be NULL. */
int pmf_debug_threshold_pass(pmf_ctx *ctx, int *n_tiles, int *n_units, int *grid, int64_t *passes);

#ifdef __cplusplus
}
#endif
#endif /* PMF_HIP_THRESHOLDS_H */
