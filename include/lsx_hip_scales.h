/* lsx_hip_scales.h -- depth-scale conversion on the device: column mass, geometric height and the optical depth at 500 nm of a
 * column from any one of them, as the reference's AtmosphereConstructor.convert_scales does it (atmosphere.py:70-144); an entry
 * of the HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays; everything is
 * checked on the host before anything is launched. */
#ifndef LSX_HIP_SCALES_H
#define LSX_HIP_SCALES_H

#include "lsx_hip_background.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which scale depth_scale is on: the values of the reference's ScaleType (atmosphere.py:13-16) */
enum { LSX_SCALE_GEOMETRIC = 0, LSX_SCALE_COLUMN_MASS = 1, LSX_SCALE_TAU500 = 2 };

/* For ncol columns of the context's Nspace depths: the equation of state and the continuous opacity at 500 nm
 * (chi_c = witt.contOpacity(T, pgas, pe, [5000 A]) / CM_TO_M, the path of lsx_hip_background with one wavelength), then the
 * integration along depth of atmosphere.py:93-141, operation by operation, with rhoSI = (Amu weightPerH) nHTot:
 *   LSX_SCALE_COLUMN_MASS  depth_scale is cmass [kg m^-2].  height[0] = 0, tau[0] = chi_c[0] / rhoSI[0] * cmass[0], the recurrences
 *                          of :101-102, then height -= hTau1.
 *   LSX_SCALE_GEOMETRIC    depth_scale is height [m], returned bit for bit (no shift).  cmass[0] = (nHTot[0] weightPerH + ne[0])
 *                          (kB T[0] / gravity); tau[0] = 0.5 chi_c[0] (h[0] - h[1]), set to exactly 0 if it is > 1 (the
 *                          reference's rule, :117-118); the recurrences of :121-122.
 *   LSX_SCALE_TAU500       depth_scale is tau500.  cmass[0] = (tau[0] / chi_c[0]) rhoSI[0], height[0] = 0, the recurrences of
 *                          :133-134 (cmass integrates chi_c there, as the reference has it), then height -= hTau1.
 *   hTau1 = numpy.interp(1.0, tau, height): height[0] where 1 < tau[0], height[-1] where 1 >= tau[-1], else with the j of
 *   tau[j] <= 1 < tau[j+1]: height[j] if tau[j] == 1, else slope (1 - tau[j]) + height[j], slope = (height[j+1] - height[j]) /
 *   (tau[j+1] - tau[j]).
 * depth_scale, temperature, nHTot, ne: [ncol][Nspace], SI, as after AtmosphereConstructor.nondimensionalise().  ne and gravity
 *   are read for the geometric scale only (ne may be NULL otherwise); gravity is the reference's 10**logG (:115), formed by the
 *   caller.
 * height, cmass, tau_ref, chi_ref: [ncol][Nspace], host memory; chi_ref is chi_c in m^-1.  Any of them may be NULL.
 * install = 1 copies the resulting height, device to device, into the context as the height of columns [col0, col0 + ncol)
 *   (col0 is read only then; without install any ncol >= 1 is computed).  The columns must have been set before
 *   (lsx_set_columns).  It invalidates what lsx_set_columns invalidates for a new height and nothing else -- the ray-serial
 *   sweeps' operand table and a speculative formal solution's claim to be discardable: populations, J, profiles, background and
 *   Ng state keep their bits.
 * LSX_EINVAL, found on the host before anything is launched: Nspace < 2; a scale outside the enum; ncol < 1; install outside
 *   {0, 1}, a column range outside the context or a column lsx_set_columns has not set; non-finite or non-positive temperature,
 *   nHTot, and ne / gravity where they are read; a temperature below 2500 K (the reference's ValueError, :75-76); a depth scale that
 *   is not strictly monotonic -- cmass and tau500 strictly ascending and positive, height strictly descending and finite (the
 *   reference does NOT check this: it integrates whatever it is given); bad tables (lsx_hip_background.h).
 * LSX_ENOCONV (a point of the equation of state hit a cap): nothing is installed and nothing is written. */
int lsx_hip_convert_scales(lsx_ctx* ctx, const lsx_eos_tables* tab, int32_t scale, int32_t col0, int32_t ncol,
                           const double* depth_scale, const double* temperature, const double* nHTot, const double* ne,
                           double gravity, double* height, double* cmass, double* tau_ref, double* chi_ref, int32_t install);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_SCALES_H */
