/* lsx_hip_boundary.h -- radiation boundary conditions at both ends of a column: zero, thermalised or given; entries of the HIP
 * library alone, included by lsx_hip.h.  Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64,
 * C-contiguous arrays. */
#ifndef LSX_HIP_BOUNDARY_H
#define LSX_HIP_BOUNDARY_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The value a ray starts with.  Up-going rays start at the LOWER end (depth Nspace - 1), down-going rays at the UPPER end (depth 0):
 *   ZERO          I = 0
 *   THERMALISED   lower: B(T[Ns-1]) - (B(T[Ns-2]) - B(T[Ns-1])) / dtau_uw, dtau_uw of the last interval along the ray
 *                 (formal_solver.py:203-207); upper, its mirror image: B(T[0]) - (B(T[1]) - B(T[0])) / dtau_uw,
 *                 dtau_uw = zmu (chi[0] + chi[1]) / 2 |z[0] - z[1]|
 *   GIVEN         I_lower[col][la][mu] / I_upper[col][la][mu]: on the context's wavelength grid and its own rays, SI units as LSX_I
 * Everything behind the start value is as it was: the recurrence, Psi* = 0 at a ray's first point, the end-point rule. */
#define LSX_BOUNDARY_ZERO 0
#define LSX_BOUNDARY_THERMALISED 1
#define LSX_BOUNDARY_GIVEN 2

/* Sets the boundary of columns [col0, col0 + ncol).  I_lower / I_upper: host memory, [ncol][Nspect][Nrays]; a pointer is required
 * exactly where its kind is GIVEN and must be NULL otherwise.  Kinds and arrays are kept per column: one context may hold columns
 * with different boundaries, and a column's bits do not depend on what the columns beside it have.
 * A context on which this entry has never been called computes, bit for bit, what it did without it: (THERMALISED, ZERO), the
 * reference's hard-wired pair.  Setting that pair explicitly gives the same bits through the other branch of the kernels.
 * The boundary is context state: lsx_set_columns and lsx_set_atmosphere (which reset J) do NOT reset it; it holds for every
 * following formal solution (frozen columns, Ng acceleration, the time-dependent step and the speculative call included), for
 * lsx_hip_radiative_rates and for lsx_hip_radiative_losses.  The entries that follow rays the context does not have --
 * lsx_hip_emergent_rays, lsx_hip_depth_rays, lsx_hip_spectrum -- use the LOWER kind only (their rays go up); ZERO and THERMALISED
 * hold at any angle and wavelength, a GIVEN lower boundary in any column of their range is LSX_EUNSUPPORTED before anything is
 * launched (the intensity was not handed over at that angle or wavelength).  The unit entries without a context keep their own
 * start value.
 * The call waits for the context's stream (twice: before it writes, and until the caller's arrays have been read), uploads the kinds
 * of ALL columns (8 * ncol bytes) and the given arrays of the range, and drops the captured formal-solution graphs (their kernel
 * arguments are stale): tens of microseconds plus the copy, cheap between time steps, not something for an inner loop; set a
 * range of columns that share their kinds with one call.
 * Device memory: 16 + 8 * ncol bytes at the first call, 2 * ncol * Nspect * Nrays doubles more from the first GIVEN on.
 * LSX_EINVAL, before anything changes: an unknown kind, a missing or a superfluous array, a column range outside the context.
 * LSX_EDEVICE (an allocation, a copy or a synchronisation of the runtime failed) can arrive after the context's own record of the
 * kinds has been updated: the boundary of the range is then undefined until the call is repeated with success. */
int lsx_hip_set_boundary(lsx_ctx* ctx, int32_t col0, int32_t ncol, int32_t lower_kind, int32_t upper_kind, const double* I_lower,
                         const double* I_upper);

/* kinds: [ncol][2] (lower, upper) of columns [col0, col0 + ncol), host memory; (THERMALISED, ZERO) where nothing was set. */
int lsx_hip_boundary_state(lsx_ctx* ctx, int32_t col0, int32_t ncol, int32_t* kinds);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_BOUNDARY_H */
