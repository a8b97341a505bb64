/* lsx_hip_stokes.h -- full-Stokes emergent spectra in a magnetic field (Zeeman effect) from what a context holds; an entry of the
 * HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_STOKES_H
#define LSX_HIP_STOKES_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest number of Zeeman components a line's pattern may have */
#define LSX_STOKES_MAX_COMPONENTS 64
/* ... and of all the patterns of the lines that are active in the window of one call together (they are kept in LDS) */
#define LSX_STOKES_MAX_WINDOW_COMPONENTS 1024

/* The "field-free" method: populations and J are those of the unpolarised iteration the context has run; only this final formal
 * solution is polarised.  For the up-going rays with direction cosines mu[] (each in (0, 1], any nmu >= 1), columns
 * [col0, col0 + ncol) and the window [la0, la0 + nla) of the merged wavelength grid, the emergent Stokes vector (I, Q, U, V).
 * The state read is that of lsx_hip_emergent_rays: the CURRENT populations, the background, sigma J with the J lsx_get(LSX_J)
 * would return at this moment.
 *
 * Field: B [T] >= 0, gammaB, chiB [rad], each [ncol][Nspace] for the columns of the call: inclination against the vertical and
 * azimuth, b = (sin gammaB cos chiB, sin gammaB sin chiB, cos gammaB).  A ray lies in the x-z plane and points to the observer,
 * l = (sqrt(1 - mu^2), 0, mu); the sky-plane basis is e1 = (mu, 0, -sqrt(1 - mu^2)), e2 = (0, 1, 0); +Q is linear polarisation
 * along e1, +U at 45 degrees from e1 towards e2.
 *
 * Patterns: per LINE of the transition table, in table order (the order of aDamp's rows), ncomp[line] components, ncomp = 0: the
 * line stays unpolarised.  alpha, strength, shift: the components of all lines one after the other (sum of ncomp entries each).
 *   alpha = M_l - M_u in {-1, 0, +1}: -1 sigma_b, 0 pi, +1 sigma_r;  shift = g_l M_l - g_u M_u;  strengths sum to 1 per alpha.
 * A component sits at v - shift vB, vB = (e / 4 pi m_e) lambda0 B / vBroad in Doppler widths; v > 0 is red and carries
 * mu vlos / vBroad as in lsx_hip_emergent_rays.  With phi_q, psi_q the sums of strength H resp. strength F over the components of
 * alpha = q, w(v + i a) = H + i F, both divided by sqrt(pi) vBroad, and c, s^2, sQ = s^2 cos 2 chi', sU = s^2 sin 2 chi' the
 * field's cosine, squared sine and azimuth terms against the ray and its basis:
 *   phi_I = [phi_0 s^2 + (phi_+1 + phi_-1)(1 + c^2) / 2] / 2     phi_Q,U = [phi_0 - (phi_+1 + phi_-1) / 2] sQ,U / 2
 *   phi_V = (phi_+1 - phi_-1) c / 2                              psi_Q, psi_U, psi_V likewise
 * so that a field pointing AT the observer gives V > 0 on the blue flank of an absorption line.  Background, continua, unpolarised
 * lines and sigma J enter eta_I and eps_I only, as in lsx_hip_emergent_rays.  The transfer equation dI/ds = -K I + eps is solved
 * with the DELO-linear rule (Rees, Murphy & Durrant 1989) from the bottom: I thermalised (formal_solver.py:203-207; 0 where
 * lsx_hip_set_boundary set ZERO; GIVEN: LSX_EUNSUPPORTED), Q = U = V = 0.  At the ray's end point I carries, as a scalar term from
 * eps_I / eta_I, what the reference's linear rule does there (formal_solver.py:138-139: the previous interval's weights): with no
 * pattern at all Q = U = V = 0.0 exactly and I is what lsx_hip_emergent_rays returns under the linear rule, to rounding.  The
 * polarised step itself is the plain DELO step at the end point too.  The context's formal solver setting is not looked at.
 *
 * out: [ncol][4][nla][nmu] (I, Q, U, V), host memory, nbytes = ncol * 4 * nla * nmu * 8.
 * Read-only on the context, ordered on its stream like lsx_get.  One writer per value, no atomics: a column's result does not
 * depend on the column range, on the window's placement, on the other angles of the call or on how the call is cut into passes.
 * The line profiles of every column of the range must have been BUILT by the library (lsx_set_line_profiles,
 * lsx_set_atmosphere), compact or not: the kept aDamp, vBroad and vlos are what the split profiles are formed from.  Otherwise
 * LSX_EUNSUPPORTED.  Also LSX_EUNSUPPORTED, before anything is launched: ncomp[line] > LSX_STOKES_MAX_COMPONENTS; the patterns of
 * the lines active in the window sum to more than LSX_STOKES_MAX_WINDOW_COMPONENTS.
 * LSX_EINVAL, before anything is launched: a null argument, nmu < 1, a mu outside (0, 1] or NaN, a column range outside the context,
 * nla < 1, a window outside [0, Nspect), a byte count that does not match, a non-finite B, gammaB or chiB, B < 0, ncomp < 0, an
 * alpha outside {-1, 0, +1}, a non-finite strength or shift, a pattern whose strengths per alpha do not sum to 1 within 1e-12.
 * Device memory: 4 nla nmu + 3 Nspace doubles per column; the columns are processed in passes so that it stays under 256 MiB (one
 * column's need where that alone is more); allocated at the first call and freed by lsx_destroy. */
int lsx_hip_stokes_rays(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                        const double* B, const double* gammaB, const double* chiB,
                        const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                        double* out, size_t nbytes);

/* The cap of that device memory in bytes for this context (0: the default, 256 MiB).  Frees what is allocated; the next call
 * allocates under the new cap.  The results do not depend on it. */
int lsx_hip_stokes_rays_work_cap(lsx_ctx* ctx, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_STOKES_H */
