/* lsx_hip_ng.h -- Ng acceleration of the MALI loop, per column, on the device; entries of the HIP library alone, included by
 * lsx_hip.h.  Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_NG_H
#define LSX_HIP_NG_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ng extrapolation of the populations (Ng 1974; Olson, Auer & Buchler 1986) on top of the MALI loop.  Off by default; with it
 * off every result of the library is bit for bit what it is without these entries, and so are lsx_effective_options /
 * lsx_options_signature.  With it on, the options string ends in ";ng=<order>,<delay>".
 *
 * order 0 switches it off and frees the history; orders 1 and 2 are accepted; any other order, or delay < 0, is LSX_EINVAL before
 * anything is allocated.  Device memory: (order + 2) * ncol * NLtot * Nspace doubles.  Every column is reset (counter = -delay,
 * applied = rejected = 0, coefficients 0).
 *
 * When on, lsx_stat_equil_async (and so lsx_stat_equil) enqueues ONE more launch on the context's stream behind its own kernels;
 * nothing else in the call sequence changes.  Per column that is active (lsx_set_active_columns), with a counter cnt:
 *   cnt < 0:  cnt += 1, nothing else.
 *   else:     the populations the statistical equilibrium has just written are stored in history slot cnt; cnt += 1;
 *             when cnt == order + 2 the column extrapolates (below) and cnt = 0: the history restarts empty, the accelerated
 *             populations are not stored.
 * The extrapolation, per atom of the column, over that atom's levels x depths: x0 the newest stored vector, x1 .. x_{order+1} the
 * older ones, w = 1 / x0^2, d0 = x0 - x1, D_j = d0 - (x_j - x_{j+1}) (j = 1..order), A_ij = sum w D_i D_j, b_i = sum w d0 D_i,
 * A c = b, x_acc = (1 - sum c_j) x0 + sum c_j x_j.
 * The step is taken only if every atom's system is regular and every entry of every atom's x_acc is finite and > 0; then LSX_N of
 * the column becomes x_acc and its LSX_DPOPS_COL becomes max |1 - x1 / x_acc| over all its levels and depths (x1 is what this
 * iteration's statistical equilibrium started from: the monitor still is the relative change over the iteration).  Otherwise the
 * column keeps what the statistical equilibrium wrote and its `rejected` count goes up; the history restarts all the same.
 * The history of a column range is discarded (cnt = -delay) when its populations are replaced from outside: lsx_set(LSX_N),
 * lsx_set_columns, lsx_set_atmosphere with lte_pops.  Frozen columns are not touched.
 * Every sum has a fixed order that depends neither on the context's column count nor on the column's index: a column's bits do
 * not depend on where it sits or on how a job is sharded. */
int lsx_hip_ng_configure(lsx_ctx* ctx, int32_t order, int32_t delay);

/* The state of columns [col0, col0 + ncol): stored [ncol] (the counter: -delay .. -1 while the delay runs, then the number of
 * vectors in the history), applied [ncol] and rejected [ncol] (steps taken / refused since lsx_hip_ng_configure), coef
 * [ncol][Natoms][2] (c_1, c_2 of the last step taken; c_2 = 0 at order 1; 0 before the first step).  Host memory; any pointer may
 * be NULL.  Ordered on the context's stream behind everything enqueued, like lsx_get.  LSX_EINVAL: Ng is off, or a bad range. */
int lsx_hip_ng_state(lsx_ctx* ctx, int32_t col0, int32_t ncol, int32_t* stored, int32_t* applied, int32_t* rejected, double* coef);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_NG_H */
