// lsx_fit_regular_san_main.cpp -- the penalty and the uncertainties of lsx_fit_regular_host.cpp (lsx_fit_regular_dev.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (`make fitregularsan`; nothing is loaded into python): the
// smallest shape (P = Q = 1), the largest (P = 24, Q = 96, Nspace = 82) and a singular column among good ones, every array sized
// exactly, the sums checked against long double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_fit_regular.h"

extern "C" {
int lsx_fit_regular_host_penalty(int32_t, int32_t, const lsx_fit_penalty*, const double*, double*, double*, double*, double*);
int lsx_fit_regular_host_uncertainty(int32_t, int32_t, const double*, const lsx_fit_penalty*, const double*, int32_t, const int32_t*,
                                     const double*, int32_t, double*, double*, double*, double*, int32_t*);
}

namespace {

int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) { ++failures; printf("line %d: %s\n", __LINE__, #cond); } \
    } while (0)

double noise(uint64_t& s)      // in (-1, 1)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(s >> 11) / 4503599627370496.0 - 1.0;
}

// ncol columns; hess = K^T K + I of a made-up K (positive definite); column `singular` (if >= 0) gets a zero last row and column
void run(int ncol, int P, int Q, int Ns, const int32_t (&nnode)[4], int npar, bool with_target, int singular)
{
    const size_t PP = (size_t)P * P;
    uint64_t seed = 991u + (uint64_t)P * 131 + Q;
    std::vector<double> L((size_t)Q * P), target((size_t)ncol * Q), nodes((size_t)ncol * P), chi2((size_t)ncol), grad((size_t)ncol * P),
        hess((size_t)ncol * PP), pout((size_t)ncol, NAN), basis((size_t)P * Ns), scale((size_t)ncol);
    for (auto& x : L) x = noise(seed);
    for (auto& x : target) x = noise(seed);
    for (auto& x : nodes) x = noise(seed);
    for (auto& x : basis) x = 0.5 + 0.5 * noise(seed);
    for (auto& x : grad) x = noise(seed);
    for (int c = 0; c < ncol; ++c) {
        chi2[c] = 10.0 + noise(seed);
        scale[c] = 1.5 + noise(seed);
        std::vector<double> K(PP);
        for (auto& x : K) x = noise(seed);
        for (int a = 0; a < P; ++a)
            for (int b = 0; b <= a; ++b) {
                double s = a == b ? 1.0 : 0.0;
                for (int k = 0; k < P; ++k) s += K[(size_t)k * P + a] * K[(size_t)k * P + b];
                hess[c * PP + (size_t)a * P + b] = hess[c * PP + (size_t)b * P + a] = s;
            }
    }
    const lsx_fit_penalty pen{Q, L.data(), with_target ? target.data() : nullptr};
    const std::vector<double> chi0 = chi2, grad0 = grad, hess0 = hess;
    std::vector<double> chib = chi2;
    EXPECT(lsx_fit_regular_host_penalty(ncol, P, &pen, nodes.data(), chi2.data(), grad.data(), hess.data(), pout.data()) == LSX_OK);
    EXPECT(lsx_fit_regular_host_penalty(ncol, P, &pen, nodes.data(), chib.data(), nullptr, nullptr, nullptr) == LSX_OK);
    const double u = std::ldexp(1.0, -53), tol = (Q + 2.0 * P + 8.0) * u;
    for (int c = 0; c < ncol; ++c) {
        EXPECT(chi2[c] == chib[c]);
        std::vector<long double> rho((size_t)Q), rabs((size_t)Q);
        long double pv = 0, pa = 0;
        for (int q = 0; q < Q; ++q) {
            long double s = with_target ? target[(size_t)c * Q + q] : 0.0L, sa = fabsl(s);
            for (int j = 0; j < P; ++j) {
                s -= (long double)L[(size_t)q * P + j] * nodes[(size_t)c * P + j];
                sa += fabsl((long double)L[(size_t)q * P + j] * nodes[(size_t)c * P + j]);
            }
            rho[q] = s;
            rabs[q] = sa;
            pv += s * s;
            pa += sa * sa;
        }
        EXPECT(fabsl(pout[c] - pv) <= tol * pa);
        EXPECT(fabsl(chi2[c] - (chi0[c] + pv)) <= tol * (fabsl((long double)chi0[c]) + pa));
        for (int a = 0; a < P; ++a) {
            long double g = grad0[(size_t)c * P + a], ga = fabsl(g);
            for (int q = 0; q < Q; ++q) {
                g += (long double)L[(size_t)q * P + a] * rho[q];
                ga += fabsl((long double)L[(size_t)q * P + a]) * rabs[q];
            }
            EXPECT(fabsl(grad[(size_t)c * P + a] - g) <= tol * ga);
            for (int b = 0; b < P; ++b) {
                long double h = hess0[c * PP + (size_t)a * P + b], ha = fabsl(h);
                for (int q = 0; q < Q; ++q) {
                    h += (long double)L[(size_t)q * P + a] * L[(size_t)q * P + b];
                    ha += fabsl((long double)L[(size_t)q * P + a] * L[(size_t)q * P + b]);
                }
                EXPECT(fabsl(hess[c * PP + (size_t)a * P + b] - h) <= tol * ha);
                EXPECT(hess[c * PP + (size_t)a * P + b] == hess[c * PP + (size_t)b * P + a]);
            }
        }
    }

    // the uncertainties of the data's hess, with and without the penalty
    std::vector<double> H = hess0;
    if (singular >= 0)
        for (int a = 0; a < P; ++a) H[singular * PP + (size_t)(P - 1) * P + a] = H[singular * PP + (size_t)a * P + P - 1] = 0.0;
    for (int with_pen = 0; with_pen < 2; ++with_pen) {
        std::vector<double> ainv((size_t)ncol * PP, 7.0), cov((size_t)ncol * PP, 7.0), sigma((size_t)ncol * P, 7.0),
            fs((size_t)ncol * npar * Ns, 7.0);
        std::vector<int32_t> status((size_t)ncol, -1);
        EXPECT(lsx_fit_regular_host_uncertainty(ncol, P, H.data(), with_pen ? &pen : nullptr, with_pen ? scale.data() : nullptr, npar, nnode,
                                                basis.data(), Ns, ainv.data(), cov.data(), sigma.data(), fs.data(), status.data()) == LSX_OK);
        for (int c = 0; c < ncol; ++c) {
            // (a zero row and column stays singular under a penalty only if L's column is zero too: it is not, so only the plain run must fail)
            const bool must_fail = c == singular && !with_pen;
            if (must_fail) {
                EXPECT(status[c] == 1 && std::isnan(ainv[c * PP]) && std::isnan(cov[c * PP + PP - 1]) && std::isnan(sigma[(size_t)c * P]) &&
                       std::isnan(fs[(size_t)c * npar * Ns]));
                continue;
            }
            EXPECT(status[c] == 0);
            // A ainv = 1 to the backward error of a Cholesky solve
            long double worst = 0, nA = 0, nx = 0;
            std::vector<long double> A(PP);
            for (int a = 0; a < P; ++a)
                for (int b = 0; b < P; ++b) {
                    long double h = H[c * PP + (size_t)(a > b ? a : b) * P + (a > b ? b : a)];
                    for (int q = 0; with_pen && q < Q; ++q) h += (long double)L[(size_t)q * P + a] * L[(size_t)q * P + b];
                    A[(size_t)a * P + b] = h;
                }
            for (int a = 0; a < P; ++a) {
                long double row = 0;
                for (int b = 0; b < P; ++b) row += fabsl(A[(size_t)a * P + b]);
                nA = fmaxl(nA, row);
                for (int j = 0; j < P; ++j) {
                    long double r = a == j ? 1.0L : 0.0L;
                    for (int b = 0; b < P; ++b) r -= A[(size_t)a * P + b] * ainv[c * PP + (size_t)b * P + j];
                    worst = fmaxl(worst, fabsl(r));
                    nx = fmaxl(nx, fabsl((long double)ainv[c * PP + (size_t)a * P + j]));
                }
            }
            EXPECT(worst / (nA * nx + 1.0L) <= P * (3.0 * P + 1.0) * u);
            for (int a = 0; a < P; ++a) {
                EXPECT(cov[c * PP + (size_t)a * P + a] > 0.0);
                EXPECT(sigma[(size_t)c * P + a] == std::sqrt(cov[c * PP + (size_t)a * P + a]));
                for (int b = 0; b < P; ++b) EXPECT(cov[c * PP + (size_t)a * P + b] == cov[c * PP + (size_t)b * P + a]);
                if (!with_pen)
                    for (int b = 0; b <= a; ++b) EXPECT(cov[c * PP + (size_t)a * P + b] == ainv[c * PP + (size_t)a * P + b]);
            }
            for (int q = 0, r0 = 0; q < npar; r0 += nnode[q], ++q)
                for (int k = 0; k < Ns; ++k) {
                    const double v = fs[((size_t)c * npar + q) * Ns + k];
                    EXPECT(nnode[q] ? std::isfinite(v) && v >= 0.0 : v == 0.0);
                }
        }
    }
    printf("ncol %d, P %d, Q %d, Nspace %d, target %d, singular column %d: chi2 %.17g\n", ncol, P, Q, Ns, (int)with_target, singular, chi2[0]);
}

} // namespace

int main()
{
    const int32_t one[4] = {1, 0, 0, 0}, all3[4] = {8, 8, 8, 0}, all4[4] = {6, 6, 6, 6}, mid[4] = {3, 2, 0, 1};
    run(1, 1, 1, 1, one, 3, false, -1);
    run(1, 1, 1, 3, one, 4, true, -1);
    run(2, 24, 96, 82, all3, 3, true, -1);
    run(3, 24, 96, 82, all4, 4, false, 1);
    run(4, 6, 5, 13, mid, 4, true, 2);
    // the argument rules
    double x = 1.0, y = NAN;
    int32_t st = 0;
    const lsx_fit_penalty ok{1, &x, nullptr}, norow{0, &x, nullptr}, many{97, &x, nullptr}, noL{1, nullptr, nullptr}, nanL{1, &y, nullptr},
        nant{1, &x, &y};
    EXPECT(lsx_fit_regular_host_penalty(1, 1, &ok, &x, &x, nullptr, nullptr, nullptr) == LSX_OK);
    x = 1.0;
    for (const lsx_fit_penalty* p : {&norow, &many, &noL, &nanL, &nant, (const lsx_fit_penalty*)nullptr})
        EXPECT(lsx_fit_regular_host_penalty(1, 1, p, &x, &x, nullptr, nullptr, nullptr) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_penalty(0, 1, &ok, &x, &x, nullptr, nullptr, nullptr) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_penalty(1, 25, &ok, &x, &x, nullptr, nullptr, nullptr) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_penalty(1, 1, &ok, &y, &x, nullptr, nullptr, nullptr) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_penalty(1, 1, &ok, &x, &x, &x, nullptr, nullptr) == LSX_EINVAL);
    const int32_t neg[4] = {2, -1, 0, 0}, two[4] = {2, 0, 0, 0};
    double o[6];       // ainv, cov, sigma, field_sigma [1][3][1]
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, nullptr, 3, one, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_OK && st == 0);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, nullptr, 2, one, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, nullptr, 3, neg, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, nullptr, 3, two, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, nullptr, 3, one, &x, 0, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, nullptr, 3, one, &y, 1, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, nullptr, &y, 3, one, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &x, &many, nullptr, 3, one, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_EINVAL);
    EXPECT(lsx_fit_regular_host_uncertainty(1, 1, &y, nullptr, nullptr, 3, one, &x, 1, o, o + 1, o + 2, o + 3, &st) == LSX_OK && st == 1);
    printf(failures ? "lsx_fit_regular_san: %d FAILURES\n" : "lsx_fit_regular_san: ok\n", failures);
    return failures ? 1 : 0;
}
