/* lsx_hip_fit.h -- fitting the magnetic field vector of a column to observed Stokes profiles: the normal equations of the fit reduced
 * on the device from the response pass's own arrays, the damped (Levenberg-Marquardt) step and the chi2 of a trial field; entries of
 * the HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays. */
#ifndef LSX_HIP_FIT_H
#define LSX_HIP_FIT_H

#include "lsx.h"
#include "lsx_hip_stokes.h"
#include "lsx_hip_stokes_response.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSX_FIT_MAX_PARAMS 24

/* The field of a column is
 *     field_p[k] = base_p[k] + sum_n x[p][n] basis_p[n][k],      p of {B, gammaB, chiB}, k a depth
 * nnode[3]: the node counts per parameter, 0: the parameter is not fitted and is base_p alone.  P = nnode[0] + nnode[1] + nnode[2],
 * 1 <= P <= LSX_FIT_MAX_PARAMS.  basis [P][Nspace]: the rows of B first, then gammaB's, then chiB's; shared by all columns (hat
 * functions over depth, a constant, anything finite).  base [ncol][3][Nspace] or NULL for zeros.  nodes [ncol][P], in the rows' order.
 * The sum runs over n ascending from base, once per call, and the passes below read its result.
 *
 * Like the response this is field-free (lsx_hip_stokes.h): no NLTE solve, populations and J are what the context holds.  Read-only
 * on the context, ordered on its stream like lsx_get.
 *
 * lsx_hip_fit_field_normal: chi2 and the normal equations of the fit at `nodes`.  A data point d is (Stokes parameter, wavelength,
 * angle); obs [ncol][4][nla][nmu], laid out as the Stokes pass (lsx_hip_stokes.h) lays its result; weight the same shape, >= 0,
 * or NULL for 1; a point of weight 0 is masked: its obs does not enter.  With
 *     r_d       = obs_d - S_d            S: what the Stokes pass forms for the expanded field (that pass's own vector)
 *     J_d,(p,n) = sum_k RF_p[k]_d basis_p[n][k]   RF: what the response pass (lsx_hip_stokes_response.h) forms for it with
 *                                                  `amplitude`, at all depths
 * it returns  chi2 [ncol] = sum_d w_d r_d^2,  grad [ncol][P] = J^T W r,  hess [ncol][P][P] = J^T W J (symmetric, both triangles
 * written), and, if field_out is not NULL, the expanded field [ncol][3][Nspace].  nmu, mu, col0, ncol, la0, nla, the patterns:
 * as in the Stokes pass.  amplitude[3]: those of the fitted parameters are read.
 * rf never leaves the device: pass by pass of the response (under that pass's work cap) it is contracted over depth and the products
 * are summed over the data points in fp64, one writer per value, no atomics.  The order of every sum depends on (nla, nmu, Nspace,
 * nnode) alone: a column's chi2, grad and hess keep their bits whatever the column range, the other columns or any work cap.
 * Refused before anything is launched: null ctx, nnode, basis, nodes, obs or outputs (LSX_EINVAL); nnode negative or P outside
 * [1, LSX_FIT_MAX_PARAMS]; a basis, base, nodes, obs or weight that is not finite; a negative weight; then everything
 * the response pass refuses, with its codes, of the expanded field -- among it B < a_B / 2 at a depth where B is fitted (the
 * message names column and depth).
 *
 * lsx_hip_fit_field_chi2: chi2 alone, by one Stokes pass at the expanded field and the same reduction: the bits
 * lsx_hip_fit_field_normal gives for the same nodes. */
int lsx_hip_fit_field_normal(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                             const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                             const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                             const double amplitude[3], const double* obs, const double* weight,
                             double* chi2, double* grad, double* hess, double* field_out);

int lsx_hip_fit_field_chi2(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                           const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                           const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                           const double* obs, const double* weight, double* chi2, double* field_out);

/* The damped step, per column c of ncol (any count: the columns need not be the context's):
 *     A = hess + lambda[c] diag(hess),   A delta = grad   (Cholesky, A = L L^T, in fp64)
 *     trial = clamp(nodes + delta, lo, hi)               lo, hi [P]; infinities are allowed
 *     predicted = 2 d.grad - d.hess d,  d = trial - nodes: the decrease of chi2 in the linear model
 * hess [ncol][P][P] (the lower triangle is read for A), grad, nodes, trial [ncol][P], lambda, predicted [ncol], status [ncol].
 * status 1: a pivot of the factorisation is not positive or not a number (a singular system, a NaN in hess), or delta is not
 * finite; then trial = nodes and predicted = 0.  Refused: null arguments, ncol < 1, P outside [1, LSX_FIT_MAX_PARAMS], a lambda
 * that is negative or not finite, lo > hi or not a number. */
int lsx_hip_fit_field_step(lsx_ctx* ctx, int32_t ncol, int32_t P, const double* hess, const double* grad, const double* lambda,
                           const double* nodes, const double* lo, const double* hi, double* trial, double* predicted, int32_t* status);

/* The cap of the fit's own device memory in bytes for this context (0: the default, 64 MiB): per column 3 x 4 nla nmu doubles for
 * obs, weight and S, (P + 2) x 4 nla nmu for the Jacobian, the residual and the weight in use, and the sums; the columns of a call
 * are taken in groups that stay under it (one column's need where that alone is more).  With an instrument (below) obs, weight, the
 * residual, the weight in use, S' and J' are over M' = 4 nobs nmu points a column, S and J over M = 4 nla nmu as before:
 * (4 + P) M' + (1 + P) M doubles and the sums.  The passes it runs keep their own caps.
 * Frees what is allocated.  The results do not depend on it. */
int lsx_hip_fit_field_work_cap(lsx_ctx* ctx, size_t nbytes);

/* The instrument: a banded matrix over the wavelengths of a call's window, shared by all columns, Stokes parameters and angles of
 * the call as `basis` is.  An observed point is
 *     S'[s][o][m] = sum_{i = 0 .. width - 1} weight[o][i] S[s][first[o] + i][m]        i ascending, from 0.0
 * and so is every row of the Jacobian.  The entries that take one are declared in lsx_hip_fit_instrument.h. */
typedef struct lsx_fit_instrument {
    int32_t nobs, width;      /* pixels; grid points a pixel reads: 1 <= width <= nla                */
    const int32_t* first;     /* [nobs]: 0 <= first[o] <= nla - width                               */
    const double*  weight;    /* [nobs][width], finite, any sign; pad a shorter row with zeros       */
} lsx_fit_instrument;

#ifdef __cplusplus
}
#endif

#include "lsx_hip_fit_instrument.h"

#endif /* LSX_HIP_FIT_H */
