/* lsx_hip_spectrum.h -- emergent spectra at arbitrary wavelengths from what a context holds; an entry of the HIP library alone,
 * included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_SPECTRUM_H
#define LSX_HIP_SPECTRUM_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The emergent intensity I(lambda', mu) at nla wavelengths that need NOT be points of the context's grid -- an instrument's sampling
 * of a line, a finer grid, continuum points outside the grid -- for the up-going rays with direction cosines mu[] (each in (0, 1],
 * any nmu >= 1) and columns [col0, col0 + ncol): what the reference offers through
 * RadiativeSet.compute_wavelength_grid(extraWavelengths=...) (atomic_set.py:377-383), a Context on the finer grid that holds these
 * populations, and one formal_sol_gamma_matrices().  No second context, no second upload of the columns.
 *   - Up-going rays only, thermalised lower boundary (formal_solver.py:203-207; ZERO where lsx_hip_set_boundary set it, GIVEN is refused: lsx_hip_boundary.h), the recurrence and its end-point quirk
 *     (formal_solver.py:46-142; emergent value I[0], rh_method.py:638), under the context's rule (lsx_set_formal_solver), as
 *     lsx_hip_emergent_rays has them.  Planck function and Boltzmann factor are taken at the new wavelength.
 *   - Active set.  Transition kr, whose window in the context's grid lambda is [Nblue, Nblue + Nlambda), is active at lambda' iff
 *     lambda[Nblue] <= lambda' <= lambda[Nblue + Nlambda - 1], both ends inclusive, compared as exact doubles: the reference's
 *     rule on a merged grid (atomic_set.py:401-453).
 *   - Lines.  phi = H(a, v + mu vlos / vBroad) / (sqrt(pi) vBroad) with v = (lambda' - lambda0) c / (vBroad lambda0)
 *     (rh_method.py:231-239), from the aDamp, vBroad and vlos the library keeps per column when it builds the profiles itself
 *     (lsx_set_line_profiles, lsx_set_atmosphere; vlos is zero where the profiles were built without a velocity).  EVERY column of
 *     the range must have profiles built that way: a column whose profiles were handed over as arrays (lsx_set_columns with
 *     phi != NULL) returns LSX_EUNSUPPORTED, phi_compact or not.  wphi is not needed.
 *   - Continua.  Vij = alpha', gij = (nStar_i / nStar_j) exp(-hc / k lambda' T), Uji = (2hc / lambda'^3) Vji (rh_method.py:281-287,
 *     453).  alpha: [Ncont][nla], the cross-section of every continuum (continua in table order) at every wavelength of the call
 *     (lsx_continuum_alpha); a value outside the continuum's active window is not read.  NULL only if the context has no continuum.
 *   - J.  With N = Nspect >= 2: l = clamp(upper_bound(lambda, lambda') - 1, 0, N - 2), t = clamp((lambda' - lambda[l]) /
 *     (lambda[l+1] - lambda[l]), 0, 1), both computed on the host in float64; J' = (1 - t) J[l] + t J[l+1] as two products and a sum:
 *     exact at grid points, held constant outside the grid.  N = 1: the single value.  J is what lsx_get(LSX_J) would return at
 *     the moment of the call.
 *   - Background.  bg_chi, bg_eta: each [ncol][nla][Nspace], the background opacity and emissivity at the call's wavelengths for
 *     the columns of the call (column col0 first); bg_sca: [ncol][nla][Nspace], given if and only if the context is sca_per_lambda
 *     and bg_chi is given (otherwise the context's scattering coefficient per depth is used).  bg_chi == bg_eta == NULL:
 *     interpolation mode -- the same (l, t) interpolate the context's own background chi, eta (and sigma where it is per
 *     wavelength).  That is an APPROXIMATION between grid points (exact at them): a background with an edge or a line haze between
 *     two grid points is not resolved; hand the arrays over where that matters.
 * dst: [ncol][nla][nmu], host memory; nbytes = ncol * nla * nmu * 8.
 * Read-only: I, J, Gamma, n, the monitors and everything the following calls compute are bitwise what they would have been
 * without the call; frozen columns (lsx_set_active_columns) are computed like any other.  The work is ordered on the context's
 * stream behind everything enqueued, like lsx_get; with a speculative formal solution outstanding it sees what lsx_get sees.
 * One writer per value, every sum in a fixed order: a column's result does not depend on its place in the context, on the column
 * range, on how the call is cut into passes, or on which other wavelengths and angles are in the call.
 * Device memory: nla nmu doubles per column, and 4 nla Nspace more (6 with bg_sca) where the background is handed over; the
 * columns are processed in passes so that it stays under 256 MiB (one column's need where that alone is more).  It is allocated at
 * the first call and freed by lsx_destroy.
 * LSX_EINVAL, found on the host before anything is launched: nla < 1; wavelengths that are not strictly ascending, not finite or
 * <= 0; nmu < 1, a mu outside (0, 1] or NaN; a column range outside the context; nbytes that does not match; only one of bg_chi /
 * bg_eta; bg_sca given or missing against the rule above; alpha == NULL with Ncont > 0; a column whose line profiles have not been
 * set yet.  LSX_EUNSUPPORTED: Nspace < 3 (as the other final passes); profiles handed over as arrays; more transitions overlapping
 * at one wavelength than a workgroup's tables hold (about eighty). */
int lsx_hip_spectrum(lsx_ctx* ctx, int32_t nla, const double* wavelength, const double* alpha, const double* bg_chi,
                     const double* bg_eta, const double* bg_sca, int32_t nmu, const double* mu, int32_t col0, int32_t ncol,
                     double* dst, size_t nbytes);

/* The cap of that device memory in bytes for this context (0: the default, 256 MiB).  Frees what is allocated; the next call
 * allocates under the new cap.  The results do not depend on it. */
int lsx_hip_spectrum_work_cap(lsx_ctx* ctx, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_SPECTRUM_H */
