/*
 * pmf_hip_importance.h -- factor importance: what every factor explains of every column's loss, from one pass over the
 * resident data.  An extension of include/pmf_hip.h (same conventions, same library): every entry returns 0 on success,
 * < 0 on error with the message in pmf_last_error().
 *
 * SELF-SPECIFIED (Deviation 6; not in the reference).  At the context's current parameters, for entry
 * (i, j):  z1_ij = sigma_j sum_k x_ki y_kj,  a_ij = z1_ij delta_bj + mu_j + theta_bj  (delta = 1, theta = 0 for a row in no
 * batch and a column in no view: the fit's forward).  l_j(a, d) is the entry loss of column j's noise model INCLUDING the
 * column weight w_j (for kind 3 with the column's class bounds).  a^(-k)_ij is a_ij with term k left out of the inner
 * product, a^(0)_ij = mu_j + theta_bj the output with every factor left out.  Over the observed (finite) entries of column j
 * among the LOCAL rows:
 *     full[j]     = sum_i l_j(a_ij, d_ij)
 *     null[j]     = sum_i l_j(a^(0)_ij, d_ij)
 *     delta[k, j] = sum_i ( l_j(a^(-k)_ij, d_ij) - l_j(a_ij, d_ij) )      the per-entry difference is what is summed
 *     n_obs[j]    = the number of those entries
 * For normal columns delta[k, j] / null[j] is the variance explained by factor k; for the other noise models the explained
 * deviance.  Factors are not orthogonal: sum_k delta[k, j] != null[j] - full[j] in general.
 *
 * A column of weight 0 contributes exactly 0 to all four outputs (n_obs included), as do missing entries.  If x_ki = 0 or
 * y_kj = 0 the entry contributes exactly 0.0 to delta[k, j].  The pass is always exact f32, whatever pmf_set_precision
 * says, on f32- and bf16-stored data; sums leave f32 for f64 after at most PMF_IMPORTANCE_CHAIN entries.  No float atomics:
 * bitwise the same from call to call.  Nothing of the context changes: no parameter, gradient, optimizer or threshold
 * state, loss partial of the step-level API, or communicator.  On a row-sharded context the sums are those of the local
 * rows; the host adds the ranks.
 */
#ifndef PMF_HIP_IMPORTANCE_H
#define PMF_HIP_IMPORTANCE_H

#include "pmf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* longest float32 chain: entries added into one float32 slot before it is added to a float64 sum */
#define PMF_IMPORTANCE_CHAIN 512

/* delta: K x N doubles, factor fastest (delta[j*K + k]); full, null_: N doubles; n_obs: N int64.  Any may be NULL.
 * Refused without data ("data not set") or factors ("factors not set"). */
int pmf_factor_importance(pmf_ctx *ctx, double *delta, double *full, double *null_, int64_t *n_obs);

/* geometry of the last pmf_factor_importance on this context: the kernel instance (K blocks of 32, waves per workgroup,
 * 1 = bf16-stored data), the row ranges R, the units (column tiles x R, summed over the launches) and the workgroups of
 * the largest launch, the launches (column chunks: the slab cap), the float64 flushes of the longest unit, and the calls so
 * far.  PMF_IMPORTANCE_RANGES=n caps R, PMF_IMPORTANCE_GRID=n the workgroups, PMF_IMPORTANCE_TILES=n the column tiles per
 * launch: test hooks, read at every call.  Any pointer may be NULL.  All of it is what the HOST chose and handed to the
 * kernel: `flushes` is computed from the row panels per unit and the flush interval, the kernel does not report it back. */
int pmf_debug_factor_importance(pmf_ctx *ctx, int *kb, int *nw, int *db, int *n_ranges, int *n_units, int *grid, int *launches,
                                int *flushes, int64_t *calls);

#ifdef __cplusplus
}
#endif
#endif /* PMF_HIP_IMPORTANCE_H */
