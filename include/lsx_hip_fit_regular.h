/* lsx_hip_fit_regular.h -- what a field fit (lsx_hip_fit.h) needs on data with noise: a quadratic penalty on the node values added to
 * chi2 and the normal equations, and the uncertainties of the fitted nodes from the normal equations at the solution; entries of the
 * HIP library alone, included by lsx_hip.h.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays.  Both calls are
 * ordered on the context's stream and read-only on the context, like lsx_hip_fit_field_step; the columns need not be the context's. */
#ifndef LSX_HIP_FIT_REGULAR_H
#define LSX_HIP_FIT_REGULAR_H

#include "lsx.h"
#include "lsx_hip_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSX_REGULAR_MAX_ROWS 96          /* 4 x LSX_FIT_MAX_PARAMS */

/* A penalty is Q extra data points of unit weight whose Jacobian is the constant matrix L: the pseudo-residual of row q of column c is
 *     rho_q = target[c][q] - sum_j L[q][j] nodes[c][j]          j ascending, from 0.0
 * and the penalty is sum_q rho_q^2, q ascending.  (A row that measures something with the standard deviation sigma, in the units of
 * the fit's weights, is that something's coefficients times 1 / sigma.) */
typedef struct lsx_fit_penalty {
    int32_t nrow;            /* Q, 1 .. LSX_REGULAR_MAX_ROWS                                   */
    const double* L;         /* [Q][P], finite, shared by all columns as `basis` is            */
    const double* target;    /* [ncol][Q], finite, or NULL for zeros                           */
} lsx_fit_penalty;

/* Adds the penalty to what lsx_hip_fit_field_normal / _chi2 returned for `nodes` [ncol][P]; chi2 [ncol], grad [ncol][P] and hess
 * [ncol][P][P] are read and written in place:
 *     chi2 += sum_q rho_q^2      grad[a] += sum_q L[q][a] rho_q      hess[a][b] += sum_q L[q][a] L[q][b]
 * every sum over q ascending from 0.0, then added to the value handed in.  (a, b) and (b, a) are written from one sum: a symmetric
 * hess stays exactly symmetric.  grad and hess may both be NULL (the chi2 of a trial: the bits the full call gives); penalty_out
 * [ncol] or NULL receives the penalty alone.  One writer per value, no atomics: a column's numbers depend neither on the other columns
 * nor on ncol.
 * Refused before anything is launched (LSX_EINVAL): null ctx, pen, pen->L, nodes or chi2; one of grad and hess null and the other not;
 * ncol < 1; P outside [1, LSX_FIT_MAX_PARAMS]; nrow outside [1, LSX_REGULAR_MAX_ROWS]; an L, target or nodes that is not finite.  A
 * chi2, grad or hess that is not finite is data: it flows through. */
int lsx_hip_regular_penalty(lsx_ctx* ctx, int32_t ncol, int32_t P, const lsx_fit_penalty* pen, const double* nodes,
                            double* chi2, double* grad, double* hess, double* penalty_out);

/* The uncertainties of the nodes of a fit from its normal equations hess = J^T W J [ncol][P][P] (the DATA's alone, at the solution).
 * Per column c:
 *     A = hess + L^T L                 (pen NULL: A = hess; nrow and L of pen are read, the sums as above; hess' lower triangle is read)
 *     A = G G^T                        Cholesky without damping, the formulas of the damped step in their order
 *     ainv [P][P]: column j solves A x = e_j by the factor's two triangular solves
 *     cov[a][b] = s sum_i ainv[i][a] (sum_k hess[i][k] ainv[k][b])        b <= a, i and k ascending from 0.0; (b, a) mirrored
 * the sandwich A^-1 (J^T W J) A^-1: the covariance of the penalised estimate when the data have the covariance W^-1.  With pen NULL
 * the product is not formed: cov is s x the lower triangle of ainv, mirrored.  s = scale[c], finite and >= 0; scale NULL: 1, and the
 * multiplication is not done.  sigma[a] = sqrt(cov[a][a]).
 * field_sigma [ncol][npar][Nspace] or NULL: the standard deviation of the expanded field at every depth.  npar is 3 or 4, nnode[npar]
 * and basis [P][Nspace] are the fit's; for a parameter p with nodes
 *     field_sigma_p[k] = sqrt(sum_n basis[n][k] (sum_m cov[n][m] basis[m][k]))       n, m the rows of p, ascending from 0.0
 * and 0.0 for one without.  ainv may be NULL.
 * status[c] = 1: a pivot is not positive or not a number, or a solution is not finite; every output of that column is then NaN, the
 * other columns are untouched.
 * Refused before anything is launched (LSX_EINVAL): null ctx, hess, cov, sigma or status; ncol < 1; P outside
 * [1, LSX_FIT_MAX_PARAMS]; with pen: a null L, nrow outside [1, LSX_REGULAR_MAX_ROWS], an L that is not finite; a scale that is
 * negative or not finite; null nnode or basis, npar not 3 or 4, nnode negative or not summing to P, Nspace < 1, a basis that is not
 * finite (with or without field_sigma).  A hess that is not finite is data (status 1). */
int lsx_hip_regular_uncertainty(lsx_ctx* ctx, int32_t ncol, int32_t P, const double* hess, const lsx_fit_penalty* pen,
                                const double* scale, int32_t npar, const int32_t* nnode, const double* basis, int32_t Nspace,
                                double* ainv, double* cov, double* sigma, double* field_sigma, int32_t* status);

#ifdef __cplusplus
}
#endif

#endif /* LSX_HIP_FIT_REGULAR_H */
