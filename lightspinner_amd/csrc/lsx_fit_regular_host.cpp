// lsx_fit_regular_host.cpp -- the arithmetic of lsx_fit_regular_dev.h compiled for the CPU, on arrays handed over (tests and the sanitizer
// program only: `make fitregularhost`, `make fitregularsan`).  What lsx_fit_regular.hip does in k_regular_penalty, k_regular_covariance
// and k_regular_band, value by value in the kernels' order, with the entries' own argument rules.  Built with -ffp-contract=off.
#include <cmath>
#include <vector>

#include "lsx_fit_regular_dev.h"

using namespace lsxreg;

extern "C" {

// lsx_hip_regular_penalty on the CPU
int lsx_fit_regular_host_penalty(int32_t ncol, int32_t P, const lsx_fit_penalty* pen, const double* nodes, double* chi2, double* grad,
                                 double* hess, double* penalty_out)
{
    char msg[256];
    if (penalty_args("lsx_fit_regular_host_penalty", ncol, P, pen, nodes, chi2, grad, hess, msg, sizeof msg)) return LSX_EINVAL;
    const int Q = pen->nrow, nent = lsxfit::entries(P);
    std::vector<double> rho((size_t)Q);
    for (size_t c = 0; c < (size_t)ncol; ++c) {
        for (int q = 0; q < Q; ++q) rho[q] = pseudo(pen->target ? pen->target[c * Q + q] : 0.0, P, pen->L + (size_t)q * P, nodes + c * P);
        for (int e = grad ? 0 : nent - 1; e < nent; ++e) {
            int a, b;
            lsxfit::entry_pair(P, e, a, b);
            const double sum = entry_sum(P, Q, a, b, pen->L, rho.data());
            entry_add(P, a, b, sum, chi2 + c, grad ? grad + c * P : nullptr, hess ? hess + c * P * P : nullptr, penalty_out ? penalty_out + c : nullptr);
        }
    }
    return LSX_OK;
}

// lsx_hip_regular_uncertainty on the CPU
int lsx_fit_regular_host_uncertainty(int32_t ncol, int32_t P, const double* hess, const lsx_fit_penalty* pen, const double* scale,
                                     int32_t npar, const int32_t* nnode, const double* basis, int32_t Nspace, double* ainv, double* cov,
                                     double* sigma, double* field_sigma, int32_t* status)
{
    char msg[256];
    if (uncertainty_args("lsx_fit_regular_host_uncertainty", ncol, P, hess, pen, scale, npar, nnode, basis, Nspace, cov, sigma, status, msg,
                         sizeof msg))
        return LSX_EINVAL;
    const size_t PP = (size_t)P * P, Ns = (size_t)Nspace;
    std::vector<double> A(PP), f((size_t)P * (P + 1) / 2), x(PP), m(PP), block(PP);        // x, m: element i of column j at [i][j]
    for (size_t c = 0; c < (size_t)ncol; ++c) {
        const double* H = hess + c * PP;
        for (size_t e = 0; e < PP; ++e) A[e] = H[e];
        for (int e = 0; pen && e < P * (P + 1) / 2; ++e) {
            int a, b;
            lsxfit::entry_pair(P, e, a, b);
            entry_add(P, a, b, entry_sum(P, pen->nrow, a, b, pen->L, (const double*)nullptr), nullptr, nullptr, A.data(), nullptr);
        }
        for (int i = 0; i < P; ++i)
            for (int j = 0; j <= i; ++j) f[lsxfit::tri(i, j)] = A[(size_t)i * P + j];
        int bad = factor(P, f.data(), 1);
        for (int j = 0; j < P && !bad; ++j) bad |= unit_solve(P, j, (const double*)f.data(), 1, x.data() + j, (size_t)P);
        status[c] = bad;
        if (bad) {
            for (size_t e = 0; e < PP; ++e) {
                if (ainv) ainv[c * PP + e] = NAN;
                cov[c * PP + e] = NAN;
            }
            for (int a = 0; a < P; ++a) sigma[c * P + a] = NAN;
        } else {
            for (int j = 0; pen && j < P; ++j) hess_times(P, H, (const double*)x.data() + j, m.data() + j, (size_t)P);
            for (size_t e = 0; ainv && e < PP; ++e) ainv[c * PP + e] = x[e];
            for (int a = 0; a < P; ++a)
                for (int b = 0; b <= a; ++b) {
                    double v = pen ? sandwich(P, (const double*)x.data() + a, (const double*)m.data() + b, (size_t)P) : x[(size_t)a * P + b];
                    if (scale) v = scale[c] * v;
                    cov[c * PP + (size_t)a * P + b] = cov[c * PP + (size_t)b * P + a] = v;
                    if (a == b) sigma[c * P + a] = sqrt(v);
                }
        }
        for (int q = 0, r0 = 0; field_sigma && q < npar; r0 += nnode[q], ++q) {
            const int nn = nnode[q];
            for (int n = 0; n < nn; ++n)
                for (int mm = 0; mm < nn; ++mm) block[(size_t)n * nn + mm] = cov[c * PP + (size_t)(r0 + n) * P + r0 + mm];
            for (size_t k = 0; k < Ns; ++k)
                field_sigma[(c * npar + q) * Ns + k] =
                    bad ? NAN : nn ? sqrt(band(nn, (const double*)block.data(), basis + (size_t)r0 * Ns, Ns, k)) : 0.0;
        }
    }
    return LSX_OK;
}

} // extern "C"
