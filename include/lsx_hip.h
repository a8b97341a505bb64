/* lsx_hip.h -- entries that only the HIP library (lightspinner_amd/csrc/liblsx_hip.so) exports, on top of the common ABI of
 * lsx.h.  The oracle does not have them; a host that binds both libraries looks them up by name.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_H
#define LSX_HIP_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Emergent spectra at arbitrary viewing angles from what a context holds: the final-pass formal solution the reference
 * offers through Atmosphere.rays(mu) (atmosphere.py:386-393) followed by one formal_sol_gamma_matrices().
 * For columns [col0, col0 + ncol) and the nmu direction cosines mu[] (each in (0, 1], any nmu >= 1 -- not bound by the ray limit
 * of a context) it computes the intensity that leaves the top of the atmosphere, I(lambda, mu):
 *   - up-going rays only, thermalised lower boundary (formal_solver.py:203-207; ZERO where lsx_hip_set_boundary set it, GIVEN is refused: lsx_hip_boundary.h), the recurrence and its end-point quirk as the
 *     sweeps have them (formal_solver.py:46-142; emergent value I[0], rh_method.py:638); the context's rule (lsx_set_formal_solver);
 *   - opacity, emissivity and source function as rh_method.py:599-632 from the CURRENT populations (LSX_N), the background and
 *     the scattering term sigma J, where J is what lsx_get(LSX_J) would return at this moment;
 *   - line profiles at the new angle: a ray-independent profile (phi_compact, or vlos == NULL) is the one the formal solution
 *     uses; a ray-dependent one is re-evaluated for the up-going direction, phi = H(a, v + mu vlos / vBroad) / (sqrt(pi) vBroad)
 *     (rh_method.py:231-239), from aDamp, vBroad and vlos, which the library keeps per column when it builds the profiles
 *     (lsx_set_line_profiles, lsx_set_atmosphere).  A context with ray-dependent profiles that were handed over as arrays
 *     (lsx_set_columns with phi != NULL) cannot know them at another angle: LSX_EUNSUPPORTED.
 * dst: [ncol][Nspect][nmu], host memory; nbytes = ncol * Nspect * nmu * 8.
 * Read-only: I, J, Gamma, n, the monitors and everything the following calls compute are bitwise what they would have been
 * without the call; frozen columns (lsx_set_active_columns) are computed like any other.  The work is ordered on the context's
 * stream behind everything enqueued, like lsx_get; with a speculative formal solution outstanding it sees what lsx_get sees.
 * LSX_EINVAL, found on the host before anything is launched: nmu < 1, a mu outside (0, 1] or NaN, a column range outside the
 * context, nbytes that does not match, a column whose line profiles have not been set yet. */
int lsx_hip_emergent_rays(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, double* dst, size_t nbytes);

/* Radiative rates Rij / Rji of every transition from what a context holds: lsx_hip_rates.h, included below. */

/* Radiative flux, net radiative cooling and its division among the transitions from what a context holds: lsx_hip_losses.h,
 * included below. */

/* Opacity, source function, optical depth, intensity and contribution function at every depth along arbitrary rays:
 * lsx_hip_depth.h, included below. */

/* Ng acceleration of the MALI loop, per column, opt-in: lsx_hip_ng.h, included below. */

/* Emergent spectra at arbitrary wavelengths from what a context holds: lsx_hip_spectrum.h, included below. */

/* The background of a column on the device -- the Wittmann equation of state and the continuous opacity of the reference's
 * Background(atmos, spect): lsx_hip_background.h, included below. */

/* Depth-scale conversion on the device -- column mass, height and tau500 from any one of them, the reference's
 * AtmosphereConstructor.convert_scales: lsx_hip_scales.h, included below. */

/* LTE populations of any atoms, active in the context or not -- the reference's RadiativeSet.compute_eq_pops, which supplies
 * lsx_set_atmosphere's nHGround and nTotal: lsx_hip_eqpops.h, included below. */

/* Time-dependent populations -- an implicit step of the rate equation dn/dt = Gamma n in the place of the statistical
 * equilibrium: lsx_hip_timedep.h, included below. */

/* Radiation boundary conditions at both ends of a column -- zero, thermalised or given, per column: lsx_hip_boundary.h, included
 * below. */

/* Launch counters of the kernels behind the sweep (introspection for the tests): lsx_hip_epilogue.h, included below. */

/* GPU_MAX_HW_QUEUES=n for this process unless the caller has set it: call before the first HIP call. */
int lsx_hip_request_hw_queues(int32_t n);

/* Diagnostic: fill the LDS of every compute unit of `device` with NaN, `rounds` times (tests/test_lds_hygiene.py). */
int lsx_hip_poison_lds(int32_t device, int32_t rounds);

#ifdef __cplusplus
}
#endif

#include "lsx_hip_rates.h"
#include "lsx_hip_losses.h"
#include "lsx_hip_depth.h"
#include "lsx_hip_ng.h"
#include "lsx_hip_spectrum.h"
#include "lsx_hip_background.h"
#include "lsx_hip_scales.h"
#include "lsx_hip_eqpops.h"
#include "lsx_hip_timedep.h"
#include "lsx_hip_epilogue.h"
#include "lsx_hip_boundary.h"
#include "lsx_hip_stokes.h"
#include "lsx_hip_stokes_response.h"
#include "lsx_hip_fit.h"
#include "lsx_hip_fit_regular.h"
#include "lsx_hip_stokes_velocity.h"

#endif /* LSX_HIP_H */
