/* lsx_hip_rates.h -- radiative rates from what a context holds; an entry of the HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_RATES_H
#define LSX_HIP_RATES_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The per-transition radiative rates the reference's Context leaves in t.Rij / t.Rji (rh_method.py:691-692; U01 eq. 28, RH92
 * eq. 2.8), as ONE formal solution gives them from what the context holds at this moment, for columns [col0, col0 + ncol):
 *   - the rays are the context's own muz / wmu, both directions, under the context's rule (lsx_set_formal_solver);
 *   - opacity, emissivity and source function as rh_method.py:599-632 from the CURRENT populations (LSX_N), the background and
 *     the scattering term sigma J, where J is what lsx_get(LSX_J) would return at this moment;
 *   - the recurrence is the sweeps': its boundary values (0 at the top, thermalised at the bottom, formal_solver.py:203-209; or what lsx_hip_set_boundary set, lsx_hip_boundary.h) and
 *     its end-point quirk (formal_solver.py:138-139);
 *   - wlamu = wla (wmu / 2) 4 pi as rh_method.py:661-665, wla as rh_method.py:425-455;
 *   - line profiles are the context's own, of every ray and both directions, whichever entry set them (lsx_set_columns with
 *     arrays, lsx_set_line_profiles, lsx_set_atmosphere; ray dependent or not): nothing is re-evaluated.
 * With the sum over wavelengths, rays and directions:
 *   Rij     = sum I Vij wlamu
 *   Rji_ref = sum (Uji + I Vij) wlamu        the reference's line 692 for one call, from zero: it has Vij where the equation has Vji
 *   Rji     = sum (Uji + I Vji) wlamu        Vji = gij Vij: the physical downward rate, with which the rate equations close
 * THE REFERENCE ACCUMULATES t.Rij / t.Rji OVER ALL ITS CALLS and never zeroes them; this entry does not accumulate: every call
 * starts from zero.  On a freshly loaded context (J = 0) Rij and Rji_ref are the reference's t.Rij / t.Rji after its first
 * formal_sol_gamma_matrices().
 * Each output is [ncol][Ntrans][Nspace], host memory, nbytes_each = ncol * Ntrans * Nspace * 8; transitions in the problem's table
 * order.  Any of the three pointers may be NULL, not all three.
 * Read-only: I, J, Gamma, n, the monitors and everything the following calls compute are bitwise what they would have been
 * without the call; frozen columns (lsx_set_active_columns) are computed like any other.  The work is ordered on the context's
 * stream behind everything enqueued, like lsx_get; with a speculative formal solution outstanding it sees what lsx_get sees.
 * Every sum has a fixed order (no atomics): a column's result does not depend on its place in the context, on the column range
 * of the call or on how the call is cut into passes.
 * Device work memory: (Nspect + 2 sum of the lines' Nlambda) * Nspace doubles per column.  The columns are processed in passes
 * so that it stays under 256 MiB (one column's need where that alone is more); it is allocated at the first call and freed by
 * lsx_destroy.
 * LSX_EINVAL, found on the host before anything is launched: a column range outside the context, nbytes_each that does not
 * match, all three pointers NULL, a column whose line profiles have not been set yet. */
int lsx_hip_radiative_rates(lsx_ctx* ctx, int32_t col0, int32_t ncol, double* Rij, double* Rji, double* Rji_ref, size_t nbytes_each);

/* The cap of that work memory in bytes for this context (0: the default, 256 MiB).  Frees what is allocated; the next call allocates
 * under the new cap.  The results do not depend on it. */
int lsx_hip_radiative_rates_work_cap(lsx_ctx* ctx, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_RATES_H */
