// lsx_stokes_san_main.cpp -- a stand-alone program (`make stokessan`) that runs the formulas of lsx_stokes_dev.h through the entries
// of lsx_stokes_host.cpp, built with -fsanitize=address,undefined (tests/test_stokes_host.py runs it as a subprocess): the
// Faraday-Voigt function over the (a, v) plane, the geometry, the argument rules with a pattern at and over the cap, and whole
// windows with a pattern of the largest size, depths without a field between depths with one, and no pattern at all.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_stokes.h"

extern "C" {
void lsx_stokes_host_w(int64_t, const double*, const double*, double*, double*, double*);
void lsx_stokes_host_geometry(int64_t, const double*, const double*, const double*, double*);
int lsx_stokes_host_check(int64_t, const double*, const double*, const double*, int32_t, const int32_t*, const int32_t*, const double*,
                          const double*);
int lsx_stokes_host_window(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, int32_t,
                           const double*, const double*, const double*, const double*, const double*, const uint8_t*, const int32_t*,
                           const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*,
                           double, int32_t, int32_t, int32_t, double*);
}

static int fail(const char* what) { fprintf(stderr, "%s\n", what); return 1; }

// a pattern of n components per alpha (3 n in all), equal strengths
static void pattern(int n, std::vector<int32_t>& al, std::vector<double>& st, std::vector<double>& sh)
{
    for (int q = -1; q <= 1; ++q)
        for (int k = 0; k < n; ++k) { al.push_back(q); st.push_back(1.0 / n); sh.push_back(1.2 * q + 0.1 * (k - 0.5 * (n - 1))); }
}

int main()
{
    // ---- the function: finite everywhere, H equal to dev_voigt's, F odd ----
    {
        std::vector<double> a, v;
        for (double av : {0.0, 1e-12, 1e-3, 0.3, 1.0, 6.0, 6.2831853071795862, 7.0, 1e3})
            for (double x = -40.0; x <= 40.0; x += 0.0625) { a.push_back(av); v.push_back(x + 1e-3); }
        const int64_t n = (int64_t)a.size();
        std::vector<double> H(n), F(n), Hv(n), vm(n), H2(n), F2(n);
        lsx_stokes_host_w(n, a.data(), v.data(), H.data(), F.data(), Hv.data());
        for (int64_t i = 0; i < n; ++i) vm[i] = -v[i];
        lsx_stokes_host_w(n, a.data(), vm.data(), H2.data(), F2.data(), nullptr);
        for (int64_t i = 0; i < n; ++i) {
            if (!std::isfinite(H[i]) || !std::isfinite(F[i])) return fail("the Faraday-Voigt function is not finite");
            if (H[i] != Hv[i]) return fail("H differs from dev_voigt");
            if (H2[i] != H[i] || F2[i] != -F[i]) return fail("H is not even or F is not odd");
        }
    }
    // ---- the geometry: c^2 + s^2 = 1 ----
    {
        std::vector<double> g, x, m;
        for (int i = 0; i <= 12; ++i)
            for (int j = 0; j < 7; ++j)
                for (double mu : {1.0, 0.6, 0.1}) { g.push_back(M_PI * i / 12.0); x.push_back(0.9 * j - 2.0); m.push_back(mu); }
        std::vector<double> o(4 * g.size());
        lsx_stokes_host_geometry((int64_t)g.size(), g.data(), x.data(), m.data(), o.data());
        for (size_t i = 0; i < g.size(); ++i)
            if (std::fabs(o[4 * i] * o[4 * i] + o[4 * i + 1] - 1.0) > 1e-15) return fail("c^2 + s^2 != 1");
    }
    // ---- the rules ----
    {
        const double B[3] = {0.1, 0.0, 0.2}, g[3] = {0.0, 1.0, 3.0}, x[3] = {0.0, -1.0, 7.0};
        std::vector<int32_t> al; std::vector<double> st, sh;
        pattern(21, al, st, sh);                                     // 63 components
        int32_t nc[1] = {63};
        if (lsx_stokes_host_check(3, B, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_OK) return fail("63 components refused");
        al.push_back(0); st.push_back(0.0); sh.push_back(0.0);       // 64: at the cap
        nc[0] = LSX_STOKES_MAX_COMPONENTS;
        if (lsx_stokes_host_check(3, B, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_OK) return fail("the cap itself refused");
        al.push_back(0); st.push_back(0.0); sh.push_back(0.0);       // one over
        nc[0] = LSX_STOKES_MAX_COMPONENTS + 1;
        if (lsx_stokes_host_check(3, B, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_EUNSUPPORTED) return fail("one over the cap accepted");
        nc[0] = 63;
        al[5] = 2;
        if (lsx_stokes_host_check(3, B, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_EINVAL) return fail("alpha = 2 accepted");
        al[5] = -1; st[5] += 1e-11;
        if (lsx_stokes_host_check(3, B, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_EINVAL) return fail("a strength sum off 1 accepted");
        st[5] -= 1e-11;
        nc[0] = -1;
        if (lsx_stokes_host_check(3, B, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_EINVAL) return fail("ncomp < 0 accepted");
        nc[0] = 63;
        for (double bad : {-1e-9, (double)NAN, (double)INFINITY}) {
            const double Bb[3] = {0.1, bad, 0.2};
            if (lsx_stokes_host_check(3, Bb, g, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_EINVAL) return fail("a bad B accepted");
        }
        const double gb[3] = {0.0, (double)NAN, 3.0};
        if (lsx_stokes_host_check(3, B, gb, x, 1, nc, al.data(), st.data(), sh.data()) != LSX_EINVAL) return fail("a NaN gammaB accepted");
        // many lines: over the window's cap
        std::vector<int32_t> ncs(17, 63), als; std::vector<double> sts, shs;
        for (int l = 0; l < 17; ++l) pattern(21, als, sts, shs);
        if (lsx_stokes_host_check(0, nullptr, nullptr, nullptr, 17, ncs.data(), als.data(), sts.data(), shs.data()) != LSX_EUNSUPPORTED)
            return fail("1071 components in a window accepted");
    }
    // ---- windows: two lines (one of 63 components, one unpolarised or a triplet) over a continuum, Ns = 3 and 13 ----
    for (int Ns : {3, 13})
        for (int variant = 0; variant < 3; ++variant) {
            const int nla = 9, nl = 2;
            std::vector<double> z(Ns), T(Ns), wav(nla), chi((size_t)nla * Ns), eta((size_t)nla * Ns), vl(Ns), B(Ns), g(Ns), x(Ns);
            std::vector<double> l0 = {500.0, 500.004}, nd((size_t)nl * Ns), ne((size_t)nl * Ns), aD((size_t)nl * Ns), vB((size_t)nl * Ns);
            std::vector<uint8_t> act((size_t)nl * nla, 1);
            for (int q = 0; q < nla; ++q) wav[q] = 499.99 + 0.0025 * q;
            for (int k = 0; k < Ns; ++k) {
                const double d = (double)k / (Ns - 1);
                z[k] = 2.0e6 * (1.0 - d); T[k] = 4500.0 + 4000.0 * d;
                vl[k] = 3.0e3 * std::sin(5.0 * d); B[k] = (k % 3 == 1) ? 0.0 : 0.15; g[k] = 0.3 + 2.0 * d; x[k] = 1.0 - 3.0 * d;
                for (int q = 0; q < nla; ++q) { chi[(size_t)q * Ns + k] = 1e-9 * std::exp(9.0 * d); eta[(size_t)q * Ns + k] = 3e-9 * chi[(size_t)q * Ns + k]; }
                for (int l = 0; l < nl; ++l) {
                    nd[(size_t)l * Ns + k] = 2e-3 * std::exp(7.0 * d); ne[(size_t)l * Ns + k] = 2e-9 * nd[(size_t)l * Ns + k];
                    aD[(size_t)l * Ns + k] = 1e-3 + 0.02 * d; vB[(size_t)l * Ns + k] = 2.0e3 + 1.0e3 * d;
                }
            }
            std::vector<int32_t> nc(nl, 0), al; std::vector<double> st, sh;
            if (variant >= 1) { pattern(21, al, st, sh); nc[0] = 63; }
            if (variant == 2) { pattern(1, al, st, sh); nc[1] = 3; }
            for (double mu : {1.0, 0.1}) {
                std::vector<double> out(4 * (size_t)nla, NAN);
                if (lsx_stokes_host_window(Ns, nla, z.data(), T.data(), wav.data(), chi.data(), eta.data(), nl, l0.data(), nd.data(), ne.data(),
                                           aD.data(), vB.data(), act.data(), nc.data(), al.data(), st.data(), sh.data(), vl.data(), B.data(), g.data(),
                                           x.data(), mu, variant == 2, variant - 1, variant != 1, out.data()) != LSX_OK) return fail("a window refused");
                for (int q = 0; q < nla; ++q) {
                    const double I = out[q], Q = out[nla + q], U = out[2 * nla + q], V = out[3 * nla + q];
                    if (!std::isfinite(I) || !std::isfinite(Q) || !std::isfinite(U) || !std::isfinite(V)) return fail("a Stokes parameter is not finite");
                    if (variant != 2 && !(I > 0.0)) return fail("I <= 0");
                    if (Q * Q + U * U + V * V > I * I * (1.0 + 1e-9)) return fail("more than fully polarised");
                    if (variant == 0 && (Q != 0.0 || U != 0.0 || V != 0.0)) return fail("no pattern, but Q, U, V are not 0.0");
                }
            }
        }
    printf("STOKES SANITIZED RUN COMPLETE\n");
    return 0;
}
