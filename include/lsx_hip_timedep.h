/* lsx_hip_timedep.h -- time-dependent populations: an implicit step of the rate equation, per column, on the device; entries of
 * the HIP library alone, included by lsx_hip.h.  Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error();
 * float64, C-contiguous arrays. */
#ifndef LSX_HIP_TIMEDEP_H
#define LSX_HIP_TIMEDEP_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rate equation dn/dt = Gamma n, advanced over a time step dt by implicit Euler in the MALI sense: (I - dt Gamma) n_new =
 * n_prev, iterated with the formal solution like the statistical equilibrium, which it becomes as dt -> infinity.  Unused by
 * default; while no step has been started every result of the library is bit for bit what it is without these entries, and so
 * are lsx_effective_options / lsx_options_signature (they never change).  Device memory, from the first start on:
 * ncol * (NLtot * Nspace + 1) doubles.
 *
 * Per column the context keeps dt (0: no step started) and n_prev [NLtot][Nspace], the populations at the start of the step.
 * An update solves, per active column, atom and depth, with n the current iterate (LSX_N) and Gamma what the last formal
 * solution left (LSX_GAMMA: Gamma[i][j] is the rate j -> i, every column sums to zero):
 *   iE            the first maximum of n (the statistical equilibrium's rule)
 *   row i != iE   A[i][j] = delta_ij - dt Gamma[i][j] (formed in one rounding),  b[i] = n_prev[i]
 *   row iE        ones,  b[iE] = n_prev[0] + n_prev[1] + ... (plain adds in ascending level order)
 *   A n_new = b   LU with partial pivoting, in the operation order of the statistical equilibrium's kernels
 * and stores n_new over n.  Row iE is the sum of all rows of the unreplaced system (the columns of Gamma sum to zero), so the
 * solution is the same; replacing it keeps the system well-conditioned at every dt and conserves the atom's number density by
 * construction.  nTotal of the context is not read.  LSX_DPOPS_COL of a column becomes the maximum of |1 - n / n_new| over its
 * levels and depths -- n the iterate the call started from, not n_prev -- with the NaN rules of lsx_stat_equil.  A singular system
 * (or one with a NaN where the pivot search meets it) keeps its populations and is reported by lsx_sync / lsx_sync_end /
 * lsx_last_error exactly as lsx_stat_equil's are.  A thread owns one (column, depth): a column's bits depend neither on the
 * context's column count nor on the column's index.  At most 16 levels per atom, as for lsx_stat_equil (lsx_create refuses more).
 *
 * lsx_hip_time_dep_start begins a step for columns [col0, col0 + ncol): dt [ncol] is stored; n_prev [ncol][NLtot][Nspace] is
 * uploaded, or, where NULL, the columns' current LSX_N is copied on the device, behind everything enqueued (no host copy).  The
 * Ng history of the range is discarded (counter = -delay), as when its populations are replaced.  LSX_N itself is not touched.
 * LSX_EINVAL before anything is touched: a dt that is <= 0, NaN or infinite, a range outside the context, a null dt. */
int lsx_hip_time_dep_start(lsx_ctx* ctx, int32_t col0, int32_t ncol, const double* dt, const double* n_prev);

/* One update of every active column (lsx_set_active_columns), enqueued on the context's stream.  It stands exactly where
 * lsx_stat_equil_async stands in a call sequence and leaves the context as that call does: lsx_sync, lsx_sync_begin[_populations]
 * / lsx_sync_end, lsx_fetch_populations, lsx_monitors, lsx_get(LSX_DPOPS_COL) and a speculative formal solution behind it work
 * unchanged; with Ng on, the same one launch follows the solves.  A second update without a formal solution in between works on
 * the same Gamma.  LSX_EINVAL, with nothing launched: an active column has no step started. */
int lsx_hip_time_dep_update_async(lsx_ctx* ctx);

/* lsx_hip_time_dep_update_async + lsx_sync: -> the maximum of LSX_DPOPS_COL over the columns (dPops_max may be NULL). */
int lsx_hip_time_dep_update(lsx_ctx* ctx, double* dPops_max);

/* The state of columns [col0, col0 + ncol): dt [ncol] and n_prev [ncol][NLtot][Nspace]; host memory, either may be NULL.  Zeros
 * for columns without a step (n_prev: until the context's first start).  Ordered on the context's stream behind everything
 * enqueued, like lsx_get.  LSX_EINVAL: a bad range. */
int lsx_hip_time_dep_state(lsx_ctx* ctx, int32_t col0, int32_t ncol, double* dt, double* n_prev);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_TIMEDEP_H */
