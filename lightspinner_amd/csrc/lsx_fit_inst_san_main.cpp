// lsx_fit_inst_san_main.cpp -- the instrument's smear and the normal equations through it (lsx_fit_host.cpp: lsx_fit_host_smear,
// lsx_fit_host_normal_inst; lsx_fit_dev.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program
// (`make fitinstsan`; nothing is loaded into python): the smallest shape (nla = nobs = width = 1, P = 1), the largest of
// tests/fit_instrument_cases.py (nla = width = 130, nobs = 261, three angles, P = 24) and a band at each end of the window (first = 0
// and first = nla - width), on made-up responses, every array sized exactly, the sums checked against long double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_fit.h"

extern "C" {
int lsx_fit_host_normal(int32_t, int32_t, int32_t, const int32_t*, const double*, const double*, const double*, const double*, const double*,
                        double*, double*, double*);
int lsx_fit_host_smear(int32_t, int32_t, int32_t, int32_t, int32_t, const int32_t*, const double*, const double*, double*);
int lsx_fit_host_normal_inst(int32_t, int32_t, int32_t, const int32_t*, const double*, const double*, const double*, const double*,
                             const double*, int32_t, int32_t, const int32_t*, const double*, double*, double*, double*);
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

// first[o]: 0 for the first half of the pixels, nla - width for the rest (one band at each end; width = nla: 0 everywhere)
void run(int Ns, int nla, int nmu, int nobs, int width, const int32_t (&nnode)[3], bool with_weight)
{
    const int P = nnode[0] + nnode[1] + nnode[2], npar = (nnode[0] > 0) + (nnode[1] > 0) + (nnode[2] > 0);
    const int Mg = 4 * nla * nmu, M = 4 * nobs * nmu;
    uint64_t seed = 999u + (uint64_t)M * 7 + P;
    std::vector<double> rf((size_t)npar * Mg * Ns), S((size_t)Mg), obs((size_t)M), wt((size_t)M), basis((size_t)P * Ns),
        iw((size_t)nobs * width), Sp((size_t)M);
    std::vector<int32_t> first((size_t)nobs);
    for (auto& x : rf) x = noise(seed);
    for (auto& x : S) x = 1.0 + 0.5 * noise(seed);
    for (auto& x : obs) x = 1.0 + 0.5 * noise(seed);
    for (auto& x : wt) x = 1.0 + noise(seed);
    for (int d = 0; d < M; d += 5) wt[d] = 0.0;
    for (auto& x : basis) x = 0.5 + 0.5 * noise(seed);
    for (auto& x : iw) x = (0.6 + noise(seed)) / width;               // some negative
    for (int o = 0; o < nobs; ++o) first[o] = o < (nobs + 1) / 2 ? 0 : nla - width;

    // the smear alone: the Stokes vector as 4 rows, against long double
    EXPECT(lsx_fit_host_smear(nla, nmu, 4, nobs, width, first.data(), iw.data(), S.data(), Sp.data()) == LSX_OK);
    const double u = std::ldexp(1.0, -53);
    for (int d = 0; d < M; ++d) {
        const int so = d / nmu, m = d % nmu, s = so / nobs, o = so % nobs;
        long double v = 0, va = 0;
        for (int i = 0; i < width; ++i) {
            const long double t = (long double)iw[(size_t)o * width + i] * S[((size_t)s * nla + first[o] + i) * nmu + m];
            v += t;
            va += fabsl(t);
        }
        EXPECT(fabsl(Sp[d] - v) <= (width + 1.0) * u * va);
    }

    double chi2 = NAN, chi2b = NAN;
    std::vector<double> grad((size_t)P, NAN), hess((size_t)P * P, NAN);
    const double* w = with_weight ? wt.data() : nullptr;
    EXPECT(lsx_fit_host_normal_inst(Ns, nla, nmu, nnode, rf.data(), S.data(), obs.data(), w, basis.data(), nobs, width, first.data(), iw.data(),
                                    &chi2, grad.data(), hess.data()) == LSX_OK);
    EXPECT(lsx_fit_host_normal_inst(Ns, nla, nmu, nnode, nullptr, S.data(), obs.data(), w, nullptr, nobs, width, first.data(), iw.data(), &chi2b,
                                    nullptr, nullptr) == LSX_OK);
    EXPECT(chi2 == chi2b);
    // chi2 and grad in long double, plainly, every term's absolute value beside it
    const double tol = (M + 2.0 * Ns + 2.0 * width + 8.0) * u;
    std::vector<long double> r((size_t)M), ra((size_t)M);
    long double c = 0, ca = 0;
    for (int d = 0; d < M; ++d) {
        const int so = d / nmu, m = d % nmu, s = so / nobs, o = so % nobs;
        long double v = 0, va = 0;
        for (int i = 0; i < width; ++i) {
            const long double t = (long double)iw[(size_t)o * width + i] * S[((size_t)s * nla + first[o] + i) * nmu + m];
            v += t;
            va += fabsl(t);
        }
        const long double wd = w ? w[d] : 1.0;
        r[d] = wd > 0 ? (long double)obs[d] - v : 0;
        ra[d] = wd > 0 ? fabsl((long double)obs[d]) + va : 0;
        c += wd * r[d] * r[d];
        ca += wd * ra[d] * ra[d];
    }
    EXPECT(fabsl(chi2 - c) <= tol * ca);
    for (int a = 0; a < P; ++a) {
        const int ip = (a >= nnode[0] && nnode[0] > 0) + (a >= nnode[0] + nnode[1] && nnode[1] > 0);
        long double g = 0, ga = 0;
        for (int d = 0; d < M; ++d) {
            const int so = d / nmu, m = d % nmu, s = so / nobs, o = so % nobs;
            long double j = 0, ja = 0;
            for (int i = 0; i < width; ++i)
                for (int k = 0; k < Ns; ++k) {
                    const long double t = (long double)iw[(size_t)o * width + i] *
                                          rf[((((size_t)ip * 4 + s) * nla + first[o] + i) * Ns + k) * nmu + m] * basis[(size_t)a * Ns + k];
                    j += t;
                    ja += fabsl(t);
                }
            const long double wd = w ? w[d] : 1.0;
            g += wd * j * r[d];
            ga += wd * ja * ra[d];
        }
        EXPECT(fabsl(grad[a] - g) <= tol * ga);
        for (int b = 0; b < P; ++b) EXPECT(hess[(size_t)a * P + b] == hess[(size_t)b * P + a]);
    }
    printf("Ns %d, nla %d, nmu %d, nobs %d, width %d, P %d, weights %d: chi2 %.17g\n", Ns, nla, nmu, nobs, width, P, (int)with_weight, chi2);
}

} // namespace

int main()
{
    const int32_t one[3] = {1, 0, 0}, all[3] = {8, 8, 8};
    run(3, 1, 1, 1, 1, one, false);
    run(3, 1, 1, 1, 1, one, true);
    run(13, 130, 3, 261, 130, all, false);
    run(13, 130, 3, 261, 130, all, true);
    run(5, 65, 3, 17, 5, all, true);          // first = 0 and first = nla - width
    run(5, 64, 1, 64, 1, one, false);
    // without an instrument: lsx_fit_host_normal itself; the instrument's rules
    {
        const int32_t nn[3] = {1, 0, 0};
        std::vector<double> rf(4 * 2 * 3, 0.5), S(8, 1.0), obs(8, 1.25), basis(3, 1.0);
        double c0 = NAN, c1 = NAN, g0 = NAN, g1 = NAN, h0 = NAN, h1 = NAN;
        EXPECT(lsx_fit_host_normal(3, 2, 1, nn, rf.data(), S.data(), obs.data(), nullptr, basis.data(), &c0, &g0, &h0) == LSX_OK);
        EXPECT(lsx_fit_host_normal_inst(3, 2, 1, nn, rf.data(), S.data(), obs.data(), nullptr, basis.data(), 0, 0, nullptr, nullptr, &c1, &g1,
                                        &h1) == LSX_OK);
        EXPECT(c0 == c1 && g0 == g1 && h0 == h1 && c0 == 0.5);
        const int32_t f_ok[2] = {0, 1}, f_hi[2] = {0, 2}, f_lo[2] = {-1, 0};
        const double w_ok[2] = {1.0, 1.0}, w_nan[2] = {1.0, NAN};
        std::vector<double> out(2 * 4);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 2, 1, f_ok, w_ok, S.data(), out.data()) == LSX_OK);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 2, 1, f_hi, w_ok, S.data(), out.data()) == LSX_EINVAL);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 2, 1, f_lo, w_ok, S.data(), out.data()) == LSX_EINVAL);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 2, 1, f_ok, w_nan, S.data(), out.data()) == LSX_EINVAL);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 0, 1, f_ok, w_ok, S.data(), out.data()) == LSX_EINVAL);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 1, 3, f_ok, w_ok, S.data(), out.data()) == LSX_EINVAL);
        EXPECT(lsx_fit_host_smear(2, 1, 4, 2, 1, nullptr, w_ok, S.data(), out.data()) == LSX_EINVAL);
    }
    printf(failures ? "lsx_fit_inst_san: %d FAILURES\n" : "lsx_fit_inst_san: ok\n", failures);
    return failures ? 1 : 0;
}
