/* lsx_hip_depth.h -- depth-resolved final pass along arbitrary rays from what a context holds; an entry of the HIP library alone,
 * included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_DEPTH_H
#define LSX_HIP_DEPTH_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* WHERE in the atmosphere the emergent intensity forms: what the reference builds per (wavelength, angle, direction) inside one
 * formal_sol_gamma_matrices() and throws away (rh_method.py:601-638 keeps I[0] only), for the up-going rays with direction cosines
 * mu[] (each in (0, 1], any nmu >= 1), columns [col0, col0 + ncol) and the contiguous window [la0, la0 + nla) of the merged
 * wavelength grid.  The state read is exactly that of the emergent-ray entry of lsx_hip.h: the CURRENT populations (LSX_N), the
 * background, and sigma J with the J that lsx_get(LSX_J) would return at this moment.  Per (column, mu, wavelength), k = depth index:
 *   chi[k], S[k]   chiTot and S of rh_method.py:601-632 for the up-going direction at that mu.  A ray-independent profile is the one
 *                  the formal solution uses; a ray-dependent one is re-evaluated, phi = H(a, v + mu vlos / vBroad) / (sqrt(pi) vBroad)
 *                  (rh_method.py:231-239), from the aDamp, vBroad and vlos the library keeps.  Ray-dependent profiles that were
 *                  handed over as arrays (lsx_set_columns with phi != NULL): LSX_EUNSUPPORTED, as there.
 *   tau[k]         tau[0] = 0, tau[k] = tau[k-1] + 0.5 (chi[k-1] + chi[k]) (1 / mu) |z[k-1] - z[k]|: the dtau of formal_solver.py:129
 *                  summed from the top in index order.
 *   I[k]           the up-going intensity at every depth under the context's rule (lsx_set_formal_solver): thermalised lower
 *                  boundary (formal_solver.py:203-207; I[Nspace-1] is that value; 0 where lsx_hip_set_boundary set ZERO, GIVEN is refused), the recurrence and its end-point quirk
 *                  (formal_solver.py:46-142).  I[0] is what lsx_hip_emergent_rays returns, to rounding.
 *   contrib[k]     chi[k] S[k] exp(-tau[k]) / mu: the contribution function to the emergent intensity per unit height.  It
 *                  underflows to 0 at large tau.
 *   z_tau1         with k the first index at which tau[k] >= 1: z[k-1] + (1 - tau[k-1]) / (tau[k] - tau[k-1]) (z[k] - z[k-1]);
 *                  NaN if tau never reaches 1.
 * chi, S, tau, I, contrib: each [ncol][nmu][Nspace][nla] (the wavelength runs fastest), host memory,
 * nbytes_each = ncol * nmu * Nspace * nla * 8.  z_tau1: [ncol][nmu][nla], nbytes_z = ncol * nmu * nla * 8.  Any of the six pointers
 * may be NULL, not all six; a byte count is looked at where an array it describes is asked for.
 * Read-only: I, J, Gamma, n, the monitors and everything the following calls compute are bitwise what they would have been
 * without the call; frozen columns (lsx_set_active_columns) are computed like any other.  The work is ordered on the context's
 * stream behind everything enqueued, like lsx_get; with a speculative formal solution outstanding it sees what lsx_get sees.
 * One writer per value and no atomics: a result does not depend on the column's place in the context, on the column range, on
 * the window (a window is a slice of the full-grid call), on the other angles of the call or on how the call is cut into passes.
 * Device memory: (5 Nspace + 1) nmu nla doubles per column, whichever outputs are asked for.  The columns are processed in passes
 * so that it stays under 256 MiB (one column's need where that alone is more); it is allocated at the first call and freed by
 * lsx_destroy.
 * LSX_EINVAL, found on the host before anything is launched: nmu < 1, a mu outside (0, 1] or NaN, a column range outside the
 * context, nla < 1, a window outside [0, Nspect), all six pointers NULL, a byte count that does not match, a column whose line
 * profiles have not been set yet. */
int lsx_hip_depth_rays(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                       double* chi, double* S, double* tau, double* I, double* contrib, double* z_tau1,
                       size_t nbytes_each, size_t nbytes_z);

/* The cap of that device memory in bytes for this context (0: the default, 256 MiB).  Frees what is allocated; the next call
 * allocates under the new cap.  The results do not depend on it. */
int lsx_hip_depth_rays_work_cap(lsx_ctx* ctx, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_DEPTH_H */
