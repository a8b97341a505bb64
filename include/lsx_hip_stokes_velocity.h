/* lsx_hip_stokes_velocity.h -- the line-of-sight velocity as a quantity of the call in the polarised final pass, its response
 * functions and the field fit: a Doppler shift handed over per call, its response at every depth, and the fit of B, gammaB, chiB and
 * vlos together.  Entries of the HIP library alone; included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays.
 *
 * vlos is in m/s with the sign of the context's own vlos (lsx_set_line_profiles): a line's Doppler offset on an up-going ray is
 * v + mu vlos / vBroad.
 * THE APPROXIMATION.  Populations, J, background and boundary are the context's: they do NOT follow the velocity handed over here.
 * This is what the field-free method already does for B (lsx_hip_stokes.h): with them held, the velocity of a depth enters that
 * depth's absorption matrix only.  It holds for shifts that are small against the line's width; a shift of the size of the width
 * or more belongs into the atmosphere the context was converged with.
 *
 * (The names do not begin with lsx_hip_stokes or lsx_hip_fit: those prefixes stay the entries of lsx_hip_stokes.h and lsx_hip_fit.h.) */
#ifndef LSX_HIP_STOKES_VELOCITY_H
#define LSX_HIP_STOKES_VELOCITY_H

#include "lsx_hip_fit_instrument.h"
#include "lsx_hip_stokes_response.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the fourth parameter of the response, as a bit of `params` and as place 3 of `amplitude` */
#define LSX_STOKES_RESPONSE_VLOS 8u

/* The Stokes pass (the entry of lsx_hip_stokes.h) with the velocity of the call: its arguments, then vlos [ncol][Nspace] in m/s.
 * vlos == NULL: that entry itself, the same code path and the same bits.
 * vlos given: it stands in the place of the context's velocity in this pass alone.  Every line that is active in the window is
 * evaluated from the kept damping and Doppler width at every angle, with or without a Zeeman pattern, whether the column's own
 * profiles were built with a velocity, without one, or compact: the context's profile store is not read.  On a column that was
 * built with a velocity, handing that velocity over gives the bits of the entry without one.
 * Refused before anything is launched: what that entry refuses, and with LSX_EINVAL a vlos that is not finite (the message
 * names the point).  One more Nspace doubles of device memory per column. */
int lsx_hip_velocity_stokes_rays(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                 const double* B, const double* gammaB, const double* chiB,
                                 const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                 double* out, size_t nbytes, const double* vlos);

/* lsx_hip_response_stokes with the velocity of the call and the response to it: the old arguments with amplitude[4] = a_B [T],
 * a_gammaB, a_chiB [rad], a_vlos [m/s], then vlos [ncol][Nspace].
 *     RF_vlos[k] = ( S(vlos_k + a / 2) - S(vlos_k - a / 2) ) / a        per m/s; the geometry is unchanged, the profiles are re-formed
 * rf: [ncol][npar][4][nla][nk][nmu] in the order B, gammaB, chiB, vlos; up to nine fields per depth.  The rows of B, gammaB and chiB
 * do not depend on whether vlos is requested, and on a column built with a velocity that is handed over here they have the bits
 * of lsx_hip_response_stokes.  stokes has the bits of lsx_hip_velocity_stokes_rays.  There is no lower bound on vlos.
 * vlos == NULL: lsx_hip_response_stokes itself; LSX_STOKES_RESPONSE_VLOS is then refused (the response to a velocity is that of
 * the velocity handed over).
 * Refused before anything is launched, besides what that entry refuses: LSX_EINVAL for a vlos that is not finite and for a
 * requested a_vlos that is not finite and positive; LSX_EUNSUPPORTED where Nspace (1 + 2 npar) passes 65535. */
int lsx_hip_velocity_response_stokes(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                     const double* B, const double* gammaB, const double* chiB,
                                     const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                     uint32_t params, const double amplitude[4], int32_t nk, const int32_t* ks,
                                     double* rf, size_t rf_bytes, double* stokes, size_t stokes_bytes, const double* vlos);

/* lsx_hip_fit_field_normal and lsx_hip_fit_field_chi2 with four quantities: B, gammaB, chiB and vlos.
 *     nnode[4]; basis [P][Nspace], the rows of B, then gammaB, chiB, vlos; base [ncol][4][Nspace] or NULL for zeros;
 *     amplitude[4]; field_out [ncol][4][Nspace] (may be NULL); inst: the instrument (lsx_hip_fit_instrument.h), NULL for none.
 * The velocity is always explicit here: vlos[k] = base_3[k] + sum_n x[3][n] basis_3[n][k], never the context's -- a caller who
 * wants the context's velocity under the nodes puts it into base_3.  Still 1 <= P <= LSX_FIT_MAX_PARAMS; the sums, their order and
 * lsx_hip_fit_field_step are those of lsx_hip_fit.h.  With nnode[3] = 0 and base_3 the velocity a column was built with, chi2,
 * grad and hess have the bits of lsx_hip_fit_field_normal.
 * Refused before anything is launched: what those entries refuse (base and the expanded velocity must be finite). */
int lsx_hip_velocity_fit_normal(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                const int32_t nnode[4], const double* basis, const double* base, const double* nodes,
                                const double amplitude[4], const double* obs, const double* weight,
                                double* chi2, double* grad, double* hess, double* field_out, const lsx_fit_instrument* inst);

int lsx_hip_velocity_fit_chi2(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                              const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                              const int32_t nnode[4], const double* basis, const double* base, const double* nodes,
                              const double* obs, const double* weight, double* chi2, double* field_out,
                              const lsx_fit_instrument* inst);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_STOKES_VELOCITY_H */
