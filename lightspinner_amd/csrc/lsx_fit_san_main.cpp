// lsx_fit_san_main.cpp -- the normal equations and the damped step of lsx_fit_host.cpp (lsx_fit_dev.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a stand-alone program (`make fitsan`; nothing is loaded into python): the smallest and the largest
// shape of tests/fit_cases.py on made-up responses, every array sized exactly, the sums checked against long double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_fit.h"

extern "C" {
int lsx_fit_host_expand(int32_t, int32_t, const int32_t*, const double*, const double*, const double*, double*);
int lsx_fit_host_normal(int32_t, int32_t, int32_t, const int32_t*, const double*, const double*, const double*, const double*, const double*,
                        double*, double*, double*);
int lsx_fit_host_step(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, const double*, double*,
                      double*, int32_t*, double*);
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

void run(int Ns, int nla, int nmu, const int32_t (&nnode)[3], bool with_weight)
{
    const int P = nnode[0] + nnode[1] + nnode[2], npar = (nnode[0] > 0) + (nnode[1] > 0) + (nnode[2] > 0), M = 4 * nla * nmu;
    uint64_t seed = 12345u + (uint64_t)M * 7 + P;
    std::vector<double> rf((size_t)npar * M * Ns), S((size_t)M), obs((size_t)M), wt((size_t)M), basis((size_t)P * Ns), nodes((size_t)P),
        base(3 * (size_t)Ns), field(3 * (size_t)Ns);
    for (auto& x : rf) x = noise(seed);
    for (auto& x : S) x = 1.0 + 0.5 * noise(seed);
    for (auto& x : obs) x = 1.0 + 0.5 * noise(seed);
    for (auto& x : wt) x = 1.0 + noise(seed);
    for (int d = 0; d < M; d += 5) wt[d] = 0.0;
    for (auto& x : basis) x = 0.5 + 0.5 * noise(seed);
    for (auto& x : nodes) x = noise(seed);
    for (auto& x : base) x = noise(seed);
    EXPECT(lsx_fit_host_expand(Ns, 1, nnode, basis.data(), base.data(), nodes.data(), field.data()) == LSX_OK);
    EXPECT(std::isfinite(field[0]) && std::isfinite(field[3 * (size_t)Ns - 1]));

    double chi2 = NAN, chi2b = NAN;
    std::vector<double> grad((size_t)P, NAN), hess((size_t)P * P, NAN);
    const double* w = with_weight ? wt.data() : nullptr;
    EXPECT(lsx_fit_host_normal(Ns, nla, nmu, nnode, rf.data(), S.data(), obs.data(), w, basis.data(), &chi2, grad.data(), hess.data()) == LSX_OK);
    EXPECT(lsx_fit_host_normal(Ns, nla, nmu, nnode, nullptr, S.data(), obs.data(), w, nullptr, &chi2b, nullptr, nullptr) == LSX_OK);
    EXPECT(chi2 == chi2b);
    // the same sums in long double, plainly
    std::vector<long double> J((size_t)P * M);
    for (int a = 0, i = 0, j = 0; a < 3; ++a) {
        for (int n = 0; n < nnode[a]; ++n, ++j)
            for (int d = 0; d < M; ++d) {
                long double s = 0;
                for (int k = 0; k < Ns; ++k)
                    s += (long double)rf[(((size_t)i * 4 * nla + d / nmu) * Ns + k) * nmu + d % nmu] * basis[(size_t)j * Ns + k];
                J[(size_t)j * M + d] = s;
            }
        i += nnode[a] > 0;
    }
    const double tol = (M + 2.0 * Ns + 8.0) * std::ldexp(1.0, -53);
    long double c = 0, ca = 0;
    for (int d = 0; d < M; ++d) {
        const long double wd = w ? w[d] : 1.0, r = wd > 0 ? (long double)obs[d] - S[d] : 0;
        c += wd * r * r;
        ca += fabsl(wd * r * r);
    }
    EXPECT(fabsl(chi2 - c) <= tol * ca);
    for (int a = 0; a < P; ++a) {
        long double g = 0, ga = 0;
        for (int d = 0; d < M; ++d) {
            const long double wd = w ? w[d] : 1.0, r = wd > 0 ? (long double)obs[d] - S[d] : 0;
            g += wd * J[(size_t)a * M + d] * r;
            long double ja = 0;
            for (int k = 0; k < Ns; ++k) {
                const int i = (a >= nnode[0] && nnode[0] > 0) + (a >= nnode[0] + nnode[1] && nnode[1] > 0);
                ja += fabsl((long double)rf[(((size_t)i * 4 * nla + d / nmu) * Ns + k) * nmu + d % nmu] * basis[(size_t)a * Ns + k]);
            }
            ga += fabsl(wd * r) * ja;
        }
        EXPECT(fabsl(grad[a] - g) <= tol * ga);
        for (int b = 0; b < P; ++b) EXPECT(hess[(size_t)a * P + b] == hess[(size_t)b * P + a]);
    }

    // the step: two columns, the second singular (a zero row and column)
    std::vector<double> H2(2 * (size_t)P * P), g2(2 * (size_t)P), x2(2 * (size_t)P, 0.25), lo((size_t)P, 0.24), hi((size_t)P, INFINITY),
        trial(2 * (size_t)P, NAN), delta(2 * (size_t)P, NAN);
    for (int q = 0; q < 2; ++q) {
        for (size_t e = 0; e < (size_t)P * P; ++e) H2[q * P * P + e] = hess[e];
        for (int a = 0; a < P; ++a) g2[(size_t)q * P + a] = grad[a];
    }
    for (int a = 0; a < P; ++a) H2[(size_t)P * P + (size_t)(P - 1) * P + a] = H2[(size_t)P * P + (size_t)a * P + P - 1] = 0.0;
    const double lambda[2] = {1e-2, 1e-2};
    double pred[2] = {NAN, NAN};
    int32_t status[2] = {-1, -1};
    EXPECT(lsx_fit_host_step(2, P, H2.data(), g2.data(), lambda, x2.data(), lo.data(), hi.data(), trial.data(), pred, status, delta.data()) == LSX_OK);
    // (with more nodes than data points the matrix is singular but for the damping: either status is a valid answer there)
    EXPECT(status[0] == 0 || M < P);
    EXPECT(status[1] == 1 && pred[1] == 0.0);
    for (int a = 0; a < P; ++a) {
        EXPECT(trial[(size_t)P + a] == 0.25);
        if (status[0] == 0) EXPECT(trial[a] >= 0.24);
    }
    if (status[0] == 0) {
        long double worst = 0, nA = 0, nd = 0, ng = 0;
        for (int a = 0; a < P; ++a) {
            long double r = g2[a], row = 0;
            for (int b = 0; b < P; ++b) {
                const long double A = (long double)H2[(size_t)a * P + b] * (a == b ? 1.0L + lambda[0] : 1.0L);
                r -= A * delta[b];
                row += fabsl(A);
            }
            worst = fmaxl(worst, fabsl(r));
            nA = fmaxl(nA, row);
            nd = fmaxl(nd, fabsl((long double)delta[a]));
            ng = fmaxl(ng, fabsl((long double)g2[a]));
        }
        EXPECT(worst / (nA * nd + ng) <= P * (3.0 * P + 1.0) * std::ldexp(1.0, -53));
    }
    printf("Ns %d, nla %d, nmu %d, P %d, weights %d: chi2 %.17g, status %d %d\n", Ns, nla, nmu, P, (int)with_weight, chi2, status[0], status[1]);
}

} // namespace

int main()
{
    const int32_t one[3] = {1, 0, 0}, all[3] = {8, 8, 8};
    run(3, 1, 1, one, false);
    run(3, 1, 1, one, true);
    run(13, 130, 3, all, false);
    run(13, 130, 3, all, true);
    // the argument rules
    const int32_t none[3] = {0, 0, 0}, many[3] = {9, 8, 8}, neg[3] = {1, -1, 0};
    double x = 0.0;
    EXPECT(lsx_fit_host_expand(3, 1, none, &x, nullptr, &x, &x) == LSX_EINVAL);
    EXPECT(lsx_fit_host_expand(3, 1, many, &x, nullptr, &x, &x) == LSX_EINVAL);
    EXPECT(lsx_fit_host_expand(3, 1, neg, &x, nullptr, &x, &x) == LSX_EINVAL);
    printf(failures ? "lsx_fit_san: %d FAILURES\n" : "lsx_fit_san: ok\n", failures);
    return failures ? 1 : 0;
}
