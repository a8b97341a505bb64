// lsx_fit_regular_dev.h -- the arithmetic of the fit's penalty and of the nodes' uncertainties (include/lsx_hip_fit_regular.h; DESIGN.md
// 4.27) as __host__ __device__ functions that a host compiler also accepts: lsx_fit_regular.hip runs them in its kernels,
// lsx_fit_regular_host.cpp on arrays handed over (tests, the sanitizer program).  Built on lsx_fit_dev.h (tri, entries, entry_pair).
//   pseudo        the pseudo-residual of a row of the penalty
//   entry_sum     an entry of the penalty's reduction: a sum over the rows
//   entry_add     the value handed in plus that sum, written to its place(s)
//   factor        the Cholesky factor of a packed lower triangle, in place: lsxfit::step_solve's, without damping
//   unit_solve    a column of the inverse: the factor's two triangular solves of A x = e_j, in step_solve's order
//   hess_times    a column of hess x ainv;  sandwich  an entry of ainv^T (hess ainv)
//   band          the variance of the expanded field at a depth from a parameter's block of cov
//   penalty_args, uncertainty_args   the argument rules of the two entries (host code)
// Every sum runs in one fixed order that depends on the sizes alone.
#pragma once
#include <cstdio>

#include "../../include/lsx_hip_fit_regular.h"
#include "lsx_fit_dev.h"

namespace lsxreg {

constexpr int kMaxRows = LSX_REGULAR_MAX_ROWS;

// rho = target - sum_j L[j] x[j], j ascending from 0.0; L: the row
template <class PL>
LSXFIT_HD double pseudo(double target, int P, PL L, const double* x)
{
    double s = 0.0;
    for (int j = 0; j < P; ++j) s += L[j] * x[j];
    return target - s;
}

// the entry (a, b) of lsxfit::entry_pair: sum_q u_q v_q, q ascending from 0.0, with u = L[.][a] (a < 0: rho) and v = L[.][b] (b < 0: rho)
template <class PL, class PR>
LSXFIT_HD double entry_sum(int P, int Q, int a, int b, PL L, PR rho)
{
    double s = 0.0;
    for (int q = 0; q < Q; ++q) {
        const double u = a >= 0 ? L[q * P + a] : rho[q];
        const double v = b >= 0 ? L[q * P + b] : rho[q];
        s += u * v;
    }
    return s;
}

// the entry's value(s) += sum: hess (a, b) and (b, a) from the one sum, grad a, or chi2 (then penalty_out, if given, takes the sum alone).
// An array that is null is not the caller's to update: its entries are left out
LSXFIT_HD void entry_add(int P, int a, int b, double sum, double* chi2, double* grad, double* hess, double* penalty_out)
{
    if (b >= 0) {
        if (!hess) return;
        hess[(size_t)a * P + b] += sum;
        if (a != b) hess[(size_t)b * P + a] += sum;
    } else if (a >= 0) {
        if (grad) grad[a] += sum;
    } else {
        if (chi2) *chi2 += sum;
        if (penalty_out) *penalty_out = sum;
    }
}

// f: the packed lower triangle of A (lsxfit::tri), element e at f[e fs] -> its Cholesky factor in place, or 1 at the first pivot that is
// not positive or not a number (lsxfit::step_solve's loop with lambda = 0)
template <class PF>
LSXFIT_HD int factor(int P, PF f, size_t fs)
{
    using lsxfit::tri;
    for (int j = 0; j < P; ++j) {
        double d = f[tri(j, j) * fs];
        for (int k = 0; k < j; ++k) d -= f[tri(j, k) * fs] * f[tri(j, k) * fs];
        if (!(d > 0.0) || !(d < INFINITY)) return 1;
        const double l = sqrt(d);
        f[tri(j, j) * fs] = l;
        for (int i = j + 1; i < P; ++i) {
            double s = f[tri(i, j) * fs];
            for (int k = 0; k < j; ++k) s -= f[tri(i, k) * fs] * f[tri(j, k) * fs];
            f[tri(i, j) * fs] = s / l;
        }
    }
    return 0;
}

// G y = e_j, G^T x = y with the factor f: x element i at x[i xs] -> 0, or 1 where an element is not finite
template <class PF, class PX>
LSXFIT_HD int unit_solve(int P, int j, PF f, size_t fs, PX x, size_t xs)
{
    using lsxfit::tri;
    for (int i = 0; i < P; ++i) {
        double s = i == j ? 1.0 : 0.0;
        for (int k = 0; k < i; ++k) s -= f[tri(i, k) * fs] * x[(size_t)k * xs];
        x[(size_t)i * xs] = s / f[tri(i, i) * fs];
    }
    for (int i = P - 1; i >= 0; --i) {
        double s = x[(size_t)i * xs];
        for (int k = i + 1; k < P; ++k) s -= f[tri(k, i) * fs] * x[(size_t)k * xs];
        x[(size_t)i * xs] = s / f[tri(i, i) * fs];
    }
    int bad = 0;
    for (int i = 0; i < P; ++i)
        if (!(fabs(x[(size_t)i * xs]) < INFINITY)) bad = 1;
    return bad;
}

// m[i] = sum_k hess[i][k] x[k], k ascending from 0.0; hess [P][P], its lower triangle is read
template <class PX, class PM>
LSXFIT_HD void hess_times(int P, const double* hess, PX x, PM m, size_t xs)
{
    for (int i = 0; i < P; ++i) {
        double s = 0.0;
        for (int k = 0; k < P; ++k) s += (k <= i ? hess[(size_t)i * P + k] : hess[(size_t)k * P + i]) * x[(size_t)k * xs];
        m[(size_t)i * xs] = s;
    }
}

// sum_i xa[i] mb[i], i ascending from 0.0: the entry (a, b) of ainv^T (hess ainv) from column a of ainv and column b of hess ainv
template <class PX, class PM>
LSXFIT_HD double sandwich(int P, PX xa, PM mb, size_t xs)
{
    double s = 0.0;
    for (int i = 0; i < P; ++i) s += xa[(size_t)i * xs] * mb[(size_t)i * xs];
    return s;
}

// sum_n basis[n][k] (sum_m cov[n][m] basis[m][k]); cov: the parameter's block [nn][nn], basis: its rows, Ns apart
template <class PC>
LSXFIT_HD double band(int nn, PC cov, const double* basis, size_t Ns, size_t k)
{
    double v = 0.0;
    for (int n = 0; n < nn; ++n) {
        double t = 0.0;
        for (int m = 0; m < nn; ++m) t += cov[n * nn + m] * basis[(size_t)m * Ns + k];
        v += basis[(size_t)n * Ns + k] * t;
    }
    return v;
}

// ---- the argument rules (host code): -> LSX_OK, or LSX_EINVAL and the message in msg ----
inline bool first_not_finite(const double* a, size_t n, size_t& bad)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) { bad = i; return true; }
    return false;
}

inline int penalty_rows_args(const char* who, int32_t P, const lsx_fit_penalty* pen, char* msg, size_t nmsg)
{
    size_t bad = 0;
    if (!pen->L) return snprintf(msg, nmsg, "%s: the penalty has no L", who), LSX_EINVAL;
    if (pen->nrow < 1 || pen->nrow > LSX_REGULAR_MAX_ROWS)
        return snprintf(msg, nmsg, "%s: the penalty has nrow = %d; between 1 and %d", who, (int)pen->nrow, LSX_REGULAR_MAX_ROWS), LSX_EINVAL;
    if (first_not_finite(pen->L, (size_t)pen->nrow * P, bad))
        return snprintf(msg, nmsg, "%s: L[%zu][%zu] of the penalty is not finite", who, bad / P, bad % P), LSX_EINVAL;
    return LSX_OK;
}

inline int penalty_args(const char* who, int32_t ncol, int32_t P, const lsx_fit_penalty* pen, const double* nodes, const double* chi2,
                        const double* grad, const double* hess, char* msg, size_t nmsg)
{
    size_t bad = 0;
    if (!pen || !nodes || !chi2 || (grad != nullptr) != (hess != nullptr))
        return snprintf(msg, nmsg, "%s: null argument (grad and hess: both or neither)", who), LSX_EINVAL;
    if (ncol < 1) return snprintf(msg, nmsg, "%s: ncol = %d, need at least one column", who, (int)ncol), LSX_EINVAL;
    if (P < 1 || P > LSX_FIT_MAX_PARAMS) return snprintf(msg, nmsg, "%s: P = %d; between 1 and %d", who, (int)P, LSX_FIT_MAX_PARAMS), LSX_EINVAL;
    if (int rc = penalty_rows_args(who, P, pen, msg, nmsg)) return rc;
    if (pen->target && first_not_finite(pen->target, (size_t)ncol * pen->nrow, bad))
        return snprintf(msg, nmsg, "%s: target[%zu] of column %zu is not finite", who, bad % pen->nrow, bad / pen->nrow), LSX_EINVAL;
    if (first_not_finite(nodes, (size_t)ncol * P, bad))
        return snprintf(msg, nmsg, "%s: node %zu of column %zu is not finite", who, bad % P, bad / P), LSX_EINVAL;
    return LSX_OK;
}

inline int uncertainty_args(const char* who, int32_t ncol, int32_t P, const double* hess, const lsx_fit_penalty* pen, const double* scale,
                            int32_t npar, const int32_t* nnode, const double* basis, int32_t Nspace, const double* cov,
                            const double* sigma, const int32_t* status, char* msg, size_t nmsg)
{
    size_t bad = 0;
    if (!hess || !nnode || !basis || !cov || !sigma || !status) return snprintf(msg, nmsg, "%s: null argument", who), LSX_EINVAL;
    if (ncol < 1) return snprintf(msg, nmsg, "%s: ncol = %d, need at least one column", who, (int)ncol), LSX_EINVAL;
    if (P < 1 || P > LSX_FIT_MAX_PARAMS) return snprintf(msg, nmsg, "%s: P = %d; between 1 and %d", who, (int)P, LSX_FIT_MAX_PARAMS), LSX_EINVAL;
    if (pen)
        if (int rc = penalty_rows_args(who, P, pen, msg, nmsg)) return rc;
    if (scale)
        for (int q = 0; q < ncol; ++q)
            if (!(std::isfinite(scale[q]) && scale[q] >= 0.0))
                return snprintf(msg, nmsg, "%s: scale of column %d is %g: it must be finite and not negative", who, q, scale[q]), LSX_EINVAL;
    if (npar != 3 && npar != 4) return snprintf(msg, nmsg, "%s: npar = %d; 3 (B, gammaB, chiB) or 4 (with vlos)", who, (int)npar), LSX_EINVAL;
    int64_t sum = 0;
    for (int a = 0; a < npar; ++a) {
        if (nnode[a] < 0) return snprintf(msg, nmsg, "%s: nnode[%d] = %d is negative", who, a, (int)nnode[a]), LSX_EINVAL;
        sum += nnode[a];
    }
    if (sum != P) return snprintf(msg, nmsg, "%s: nnode sums to %lld, P = %d", who, (long long)sum, (int)P), LSX_EINVAL;
    if (Nspace < 1) return snprintf(msg, nmsg, "%s: Nspace = %d, need at least one depth", who, (int)Nspace), LSX_EINVAL;
    if (first_not_finite(basis, (size_t)P * Nspace, bad))
        return snprintf(msg, nmsg, "%s: basis[%zu][%zu] is not finite", who, bad / Nspace, bad % Nspace), LSX_EINVAL;
    return LSX_OK;
}

} // namespace lsxreg
