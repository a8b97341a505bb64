/* lsx_hip_losses.h -- radiative energy balance from what a context holds: flux, net cooling and its division among the transitions;
 * an entry of the HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_LOSSES_H
#define LSX_HIP_LOSSES_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the radiation does to the gas, as ONE formal solution gives it from what the context holds at this moment, for columns
 * [col0, col0 + ncol).  The formal solution is that of lsx_hip_rates.h (the radiative rates), word for word:
 *   - the rays are the context's own muz / wmu, both directions, under the context's rule (lsx_set_formal_solver);
 *   - opacity and emissivity as rh_method.py:599-632 from the CURRENT populations (LSX_N), the background and the scattering term
 *     sigma J, where J is what lsx_get(LSX_J) would return at this moment;
 *   - the recurrence is the sweeps': boundary values 0 at the top and thermalised at the bottom (formal_solver.py:203-209) unless
 *     lsx_hip_set_boundary has set others for the column (lsx_hip_boundary.h: all three kinds at both ends), the end-point quirk
 *     (formal_solver.py:138-139);
 *   - line profiles are the context's own, of every ray and both directions, whichever entry set them: nothing is re-evaluated.
 * Per wavelength la of the merged grid, depth k, ray m and direction d, with
 *   chi = sum_t (n_i Vij - n_j Vji) + chi_bg,   eta = sum_t n_j Uji + eta_bg + sigma J,   I = the recurrence's value at depth k
 * (I+ up-going, towards the observer; I- down-going), the pass forms
 *   H[la][k] = sum_m   (wmu_m / 2) mu_m (I+ - I-)        the Eddington flux, POSITIVE TOWARDS THE OBSERVER (outwards, +z)
 *   D[la][k] = sum_m,d (wmu_m / 2) (eta - chi I)         net emission per steradian; chi and eta depend on ray and direction
 *                                                         (line profiles) and stay inside the sum
 * and, with the weights wnu [Nspect] in Hz,
 *   F[k]     = 4 pi sum_la wnu[la] H[la][k]              radiative flux, W m^-2, positive outwards
 *   Q[k]     = 4 pi sum_la wnu[la] D[la][k]              net radiative cooling, W m^-3: POSITIVE MEANS THE GAS LOSES ENERGY.
 *                                                         With z upwards dF/dz = Q in the continuum limit.
 *   Qt[t][k] = sum_{la in t, m, d} (hc / lambda_la) wlamu [ n_j (Uji + Vji I) - n_i Vij I ]      W m^-3
 * Qt is the net radiative bracket of transition t with the photon energy INSIDE the wavelength sum (across a continuum it varies
 * by a large factor: h nu_0 (n_j Rji - n_i Rij) is not the cooling of a continuum); wlamu = wla (wmu / 2) 4 pi, Uji, Vij, Vji and
 * the active mask are exactly those of lsx_hip_rates.h; n is LSX_N.  Its wavelength weights are the transition's own (wla), not wnu.
 * wnu == NULL: the trapezoid rule in frequency over the merged grid, nu = c / lambda, wnu[la] = |nu[la - 1] - nu[la + 1]| / 2 with
 * half intervals at the two ends (the last entry below).  A caller's own wnu can zero everything outside a band or pick
 * out one wavelength: a single 1 at la gives Q = 4 pi D[la] and F = 4 pi H[la] bit for bit.
 * Q OVER THE CONTEXT'S GRID IS ONLY AS BOLOMETRIC AS THAT GRID IS: the merged grid covers the active transitions (and the
 * reference wavelength), not the whole spectrum of the background; F and Q are the flux and the cooling carried by the
 * wavelengths the context has.
 * Outputs, host memory; any pointer may be NULL, not all five:
 *   F, Q     [ncol][Nspace]              nbytes_FQ = ncol * Nspace * 8
 *   Qt       [ncol][Ntrans][Nspace]      nbytes_Qt = ncol * Ntrans * Nspace * 8       transitions in the problem's table order
 *   H, D     [ncol][Nspect][Nspace]      nbytes_HD = ncol * Nspect * Nspace * 8       the monochromatic sums themselves
 * (a byte count is checked where one of its pointers is given).
 * Read-only: I, J, Gamma, n, the monitors and everything the following calls compute are bitwise what they would have been
 * without the call; frozen columns (lsx_set_active_columns) are computed like any other.  The work is ordered on the context's
 * stream behind everything enqueued, like lsx_get; with a speculative formal solution outstanding it sees what lsx_get sees.
 * Every sum has a fixed order (no atomics): a column's result does not depend on its place in the context, on the column range
 * of the call or on how the call is cut into passes.
 * Device work memory: (3 Nspect + 2 sum of the lines' Nlambda) * Nspace doubles per column.  The columns are processed in passes
 * so that it stays under 256 MiB (one column's need where that alone is more); it is allocated at the first call and freed by
 * lsx_destroy.
 * LSX_EINVAL, found on the host before anything is launched: a column range outside the context, a byte count that does not
 * match, all five pointers NULL, a column whose line profiles have not been set yet, a wnu entry that is not finite. */
int lsx_hip_radiative_losses(lsx_ctx* ctx, int32_t col0, int32_t ncol, const double* wnu, double* F, double* Q, double* Qt, double* H,
                             double* D, size_t nbytes_FQ, size_t nbytes_Qt, size_t nbytes_HD);

/* The cap of that work memory in bytes for this context (0: the default, 256 MiB).  Frees what is allocated; the next call allocates
 * under the new cap.  The results do not depend on it. */
int lsx_hip_radiative_losses_work_cap(lsx_ctx* ctx, size_t nbytes);

/* The weights lsx_hip_radiative_losses uses for wnu == NULL, formed on the host: the trapezoid rule in frequency over an ascending
 * wavelength grid in nm, in Hz.  One point: weight 0. */
int lsx_hip_frequency_weights(int32_t Nspect, const double* wavelength, double* wnu);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_LOSSES_H */
