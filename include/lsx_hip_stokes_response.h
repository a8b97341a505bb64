/* lsx_hip_stokes_response.h -- response functions of the emergent Stokes vector to the magnetic field vector at every depth, from
 * what a context holds; an entry of the HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_STOKES_RESPONSE_H
#define LSX_HIP_STOKES_RESPONSE_H

#include "lsx.h"
#include "lsx_hip_stokes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the parameters of the field, as bits of `params` and as places in `amplitude` */
#define LSX_STOKES_RESPONSE_B 1u
#define LSX_STOKES_RESPONSE_GAMMAB 2u
#define LSX_STOKES_RESPONSE_CHIB 4u

/* In the field-free method (lsx_hip_stokes.h) populations and J do not depend on the field: the response of the emergent Stokes
 * vector to the field at one depth is the change of ONE polarised formal solution, with no NLTE solve.  For a parameter p of
 * {B, gammaB, chiB}, its amplitude a_p > 0 and a depth k:
 *     RF_p[k] = ( S(p_k + a_p / 2) - S(p_k - a_p / 2) ) / a_p
 * S = (I, Q, U, V): what the Stokes pass (lsx_hip_stokes.h) returns for the field changed at that one depth of that column only.  The full
 * amplitude convention of the other response functions; per unit of the parameter (1 / T, 1 / rad), not per unit height.  Angles,
 * columns, window, field, patterns, the state read, the conventions, the boundary handling and the end-point term of I are those of
 * that pass.
 *
 * params: LSX_STOKES_RESPONSE_* bits, at least one.  amplitude[3]: a_B [T], a_gammaB, a_chiB [rad]; those of the requested
 * parameters are read.  ks: nk depths, strictly increasing, inside [0, Nspace); NULL: all depths (nk is then ignored).
 * rf:     [ncol][npar][4][nla][nk][nmu], npar the number of set bits, in the order B, gammaB, chiB; rf_bytes its size.
 * stokes: [ncol][4][nla][nmu], the vector of the call's own field with the bits that pass returns; may be NULL
 *         (stokes_bytes is then ignored).
 * Read-only on the context, ordered on its stream like lsx_get.  One writer per value, no atomics: a column's result does not depend
 * on the column range, on the window's placement, on the other angles, depths or parameters of the call or on how the call is cut
 * into passes.
 * How: per depth the solver's node (eta_I, K', S') is formed once for each of up to seven fields; one walk up keeps the ray's state
 * at every depth, one walk down carries the 4 x 4 matrix that takes a change of the vector at a depth to the surface, and at each
 * requested depth only the steps that depth's node enters are redone.
 *
 * Refused before anything is launched: everything the Stokes pass refuses, with its codes.  LSX_EINVAL: params 0 or with an
 * unknown bit; a requested amplitude that is not finite and positive; nk < 1, a depth outside [0, Nspace) or ks not strictly
 * increasing; a byte count that does not match; B requested and B < a_B / 2 at a requested depth of a column (B >= 0 holds for the
 * changed field too; the message names column and depth: leave field-free depths out with ks).
 * Device memory per column: (1 + 2 npar) 11 Nspace nla' nmu doubles for the nodes and 5 Nspace nla' nmu for the kept states (nla':
 * nla rounded up to a multiple of 64), rf and the field; the columns are processed in passes so that it stays under 256 MiB (one
 * column's need where that alone is more); allocated at the first call and freed by lsx_destroy.  stokes comes from the Stokes
 * pass itself, run behind the response on the same arguments. */
/* (The entry is not called lsx_hip_stokes_...: the exported names of that form are the entries of lsx_hip_stokes.h, and
 * tests/test_stokes_host.py holds that set closed.) */
int lsx_hip_response_stokes(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                            const double* B, const double* gammaB, const double* chiB,
                            const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                            uint32_t params, const double amplitude[3], int32_t nk, const int32_t* ks,
                            double* rf, size_t rf_bytes, double* stokes, size_t stokes_bytes);

/* The cap of that device memory in bytes for this context (0: the default, 256 MiB).  Frees what is allocated; the next call
 * allocates under the new cap.  The results do not depend on it. */
int lsx_hip_response_stokes_work_cap(lsx_ctx* ctx, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_STOKES_RESPONSE_H */
