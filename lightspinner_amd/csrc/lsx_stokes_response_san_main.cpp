// lsx_stokes_response_san_main.cpp -- a stand-alone program (`make stokesrespsan`) that runs the host response
// (lsx_stokes_host_response of lsx_stokes_host.cpp: the two stages of lsx_stokes_response.hip through the functions of
// lsx_stokes_dev.h) built with -fsanitize=address,undefined (tests/test_stokes_response_host.py runs it as a subprocess): columns of
// 3, 4 and 40 depths, all depths and subsets of them, every set of parameters, both lower boundaries, and every refusal.  The output
// arrays have exactly the size the call needs, so that a store past a requested depth, parameter or wavelength is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_stokes_response.h"

extern "C" {
int lsx_stokes_host_window(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, int32_t,
                           const double*, const double*, const double*, const double*, const double*, const uint8_t*, const int32_t*,
                           const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*,
                           double, int32_t, int32_t, int32_t, double*);
int lsx_stokes_host_response(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, int32_t,
                             const double*, const double*, const double*, const double*, const double*, const uint8_t*, const int32_t*,
                             const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*,
                             double, int32_t, int32_t, uint32_t, const double*, int32_t, const int32_t*, double*, double*);
}

static int fail(const char* what) { fprintf(stderr, "%s\n", what); return 1; }

static void pattern(int n, std::vector<int32_t>& al, std::vector<double>& st, std::vector<double>& sh)
{
    for (int q = -1; q <= 1; ++q)
        for (int k = 0; k < n; ++k) { al.push_back(q); st.push_back(1.0 / n); sh.push_back(1.2 * q + 0.1 * (k - 0.5 * (n - 1))); }
}

int main()
{
    for (int Ns : {3, 4, 40}) {
        const int nla = 7, nl = 2;
        std::vector<double> z(Ns), T(Ns), wav(nla), chi((size_t)nla * Ns), eta((size_t)nla * Ns), vl(Ns), B(Ns), g(Ns), x(Ns);
        std::vector<double> l0 = {500.0, 500.004}, nd((size_t)nl * Ns), ne((size_t)nl * Ns), aD((size_t)nl * Ns), vB((size_t)nl * Ns);
        std::vector<uint8_t> act((size_t)nl * nla, 1);
        for (int q = 0; q < nla; ++q) wav[q] = 499.99 + 0.003 * q;
        for (int k = 0; k < Ns; ++k) {
            const double d = (double)k / (Ns - 1);
            z[k] = 2.0e6 * (1.0 - d); T[k] = 4500.0 + 4000.0 * d;
            vl[k] = 3.0e3 * std::sin(5.0 * d); B[k] = 0.08 + 0.1 * d; g[k] = 0.3 + 2.0 * d; x[k] = 1.0 - 3.0 * d;
            for (int q = 0; q < nla; ++q) { chi[(size_t)q * Ns + k] = 1e-9 * std::exp(9.0 * d); eta[(size_t)q * Ns + k] = 3e-9 * chi[(size_t)q * Ns + k]; }
            for (int l = 0; l < nl; ++l) {
                nd[(size_t)l * Ns + k] = 2e-3 * std::exp(7.0 * d); ne[(size_t)l * Ns + k] = 2e-9 * nd[(size_t)l * Ns + k];
                aD[(size_t)l * Ns + k] = 1e-3 + 0.02 * d; vB[(size_t)l * Ns + k] = 2.0e3 + 1.0e3 * d;
            }
        }
        std::vector<int32_t> nc(nl, 0), al; std::vector<double> st, sh;
        pattern(9, al, st, sh); nc[0] = 27;
        pattern(1, al, st, sh); nc[1] = 3;
        const double amp[3] = {0.01, 0.02, 0.03};
        auto call = [&](const double* Bf, double mu, int lower_zero, uint32_t params, const double* a, int32_t nk, const int32_t* ks, double* rf,
                        double* S) {
            return lsx_stokes_host_response(Ns, nla, z.data(), T.data(), wav.data(), chi.data(), eta.data(), nl, l0.data(), nd.data(), ne.data(),
                                            aD.data(), vB.data(), act.data(), nc.data(), al.data(), st.data(), sh.data(), vl.data(), Bf, g.data(),
                                            x.data(), mu, lower_zero, 0, params, a, nk, ks, rf, S);
        };
        // ---- all depths, every set of parameters, both boundaries; stokes has the window call's bits ----
        std::vector<double> full;
        for (double mu : {1.0, 0.1})
            for (int lower_zero = 0; lower_zero < 2; ++lower_zero)
                for (uint32_t params = 1; params < 8; ++params) {
                    const int npar = (params & 1) + ((params >> 1) & 1) + ((params >> 2) & 1);
                    std::vector<double> rf((size_t)npar * 4 * nla * Ns, NAN), S(4 * (size_t)nla, NAN), W(4 * (size_t)nla, NAN);
                    if (call(B.data(), mu, lower_zero, params, amp, Ns, nullptr, rf.data(), S.data()) != LSX_OK) return fail("a response refused");
                    if (lsx_stokes_host_window(Ns, nla, z.data(), T.data(), wav.data(), chi.data(), eta.data(), nl, l0.data(), nd.data(), ne.data(),
                                               aD.data(), vB.data(), act.data(), nc.data(), al.data(), st.data(), sh.data(), vl.data(), B.data(),
                                               g.data(), x.data(), mu, lower_zero, 0, 1, W.data()) != LSX_OK) return fail("a window refused");
                    for (size_t i = 0; i < S.size(); ++i)
                        if (!(S[i] == W[i])) return fail("stokes is not the window call's");
                    bool any = false;
                    for (double v : rf) {
                        if (!std::isfinite(v)) return fail("a response is not finite");
                        any = any || v != 0.0;
                    }
                    if (!any) return fail("every response is 0");
                    if (call(B.data(), mu, lower_zero, params, amp, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("stokes == null refused");
                    if (mu == 1.0 && !lower_zero && params == 7) full = rf;
                }
        // ---- subsets of the depths: the entries of the full call ----
        const std::vector<std::vector<int32_t>> subsets = {{0}, {Ns - 1}, {0, Ns - 1}, {1, 2}, {Ns - 2}, {0, 1, 2}, {Ns / 2}};
        for (const auto& ks : subsets) {
            const int nk = (int)ks.size();
            std::vector<double> rf((size_t)3 * 4 * nla * nk, NAN);
            if (call(B.data(), 1.0, 0, 7, amp, nk, ks.data(), rf.data(), nullptr) != LSX_OK) return fail("a subset refused");
            for (int i = 0; i < 3 * 4 * nla; ++i)
                for (int j = 0; j < nk; ++j)
                    if (!(rf[(size_t)i * nk + j] == full[(size_t)i * Ns + ks[j]])) return fail("a subset's entry is not the full call's");
        }
        // ---- every refusal ----
        std::vector<double> rf((size_t)3 * 4 * nla * Ns, NAN);
        const int32_t k0[1] = {0};
        if (call(B.data(), 1.0, 0, 0, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("params = 0 accepted");
        if (call(B.data(), 1.0, 0, 8, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("an unknown bit accepted");
        if (call(B.data(), 1.0, 0, 7, nullptr, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("null amplitudes accepted");
        for (int b = 0; b < 3; ++b)
            for (double bad : {0.0, -1e-3, (double)NAN, (double)INFINITY}) {
                double a[3] = {amp[0], amp[1], amp[2]};
                a[b] = bad;
                if (call(B.data(), 1.0, 0, 1u << b, a, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("a bad amplitude accepted");
                if (call(B.data(), 1.0, 0, 7u & ~(1u << b), a, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("an amplitude that is not requested was read");
            }
        if (call(B.data(), 1.0, 0, 7, amp, 0, k0, rf.data(), nullptr) != LSX_EINVAL) return fail("nk = 0 accepted");
        for (const std::vector<int32_t>& bad : std::vector<std::vector<int32_t>>{{-1}, {Ns}, {1, 1}, {2, 1}})
            if (call(B.data(), 1.0, 0, 7, amp, (int)bad.size(), bad.data(), rf.data(), nullptr) != LSX_EINVAL) return fail("bad depths accepted");
        std::vector<double> Bg(B);
        Bg[1] = 0.0;
        if (call(Bg.data(), 1.0, 0, 7, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("B below half its amplitude accepted");
        Bg[1] = 0.5 * amp[0];
        if (call(Bg.data(), 1.0, 0, 7, amp, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("B at half its amplitude refused");
        Bg[1] = 0.0;
        if (call(Bg.data(), 1.0, 0, 6, amp, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("B = 0 with only the angles requested refused");
        const int32_t skip[2] = {0, 2};
        if (call(Bg.data(), 1.0, 0, 7, amp, 2, skip, rf.data(), nullptr) != LSX_OK) return fail("B = 0 at a depth that is left out refused");
        Bg[1] = -1.0;
        if (call(Bg.data(), 1.0, 0, 6, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("B < 0 accepted");
        if (call(B.data(), 0.0, 0, 7, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("mu = 0 accepted");
        nc[0] = LSX_STOKES_MAX_COMPONENTS + 1;
        if (call(B.data(), 1.0, 0, 7, amp, Ns, nullptr, rf.data(), nullptr) == LSX_OK) return fail("a pattern over the cap accepted");
    }
    printf("STOKES RESPONSE SANITIZED RUN COMPLETE\n");
    return 0;
}
