// lsx_stokes_velocity_san_main.cpp -- a stand-alone program (`make stokesvelsan`) that runs the host twins of the velocity of a call
// (include/lsx_hip_stokes_velocity.h: lsx_stokes_host_response_v of lsx_stokes_host.cpp, lsx_fit_host_expand4 and lsx_fit_host_normal4 of
// lsx_fit_host.cpp) built with -fsanitize=address,undefined (tests/test_stokes_velocity_host.py runs it as a subprocess): columns of 3, 4
// and 40 depths, every set of the four parameters, subsets of the depths, both lower boundaries, the refusals, and the sums with 1 to
// 24 rows with and without an instrument.  The output arrays have exactly the size the call needs, so that a store past a requested
// depth, parameter or row is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_stokes_velocity.h"

extern "C" {
int lsx_stokes_host_window(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, int32_t,
                           const double*, const double*, const double*, const double*, const double*, const uint8_t*, const int32_t*,
                           const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*,
                           double, int32_t, int32_t, int32_t, double*);
int lsx_stokes_host_response(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, int32_t,
                             const double*, const double*, const double*, const double*, const double*, const uint8_t*, const int32_t*,
                             const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*,
                             double, int32_t, int32_t, uint32_t, const double*, int32_t, const int32_t*, double*, double*);
int lsx_stokes_host_response_v(int32_t, int32_t, const double*, const double*, const double*, const double*, const double*, int32_t,
                               const double*, const double*, const double*, const double*, const double*, const uint8_t*, const int32_t*,
                               const int32_t*, const double*, const double*, const double*, const double*, const double*, const double*,
                               double, int32_t, int32_t, uint32_t, const double*, int32_t, const int32_t*, double*, double*);
int lsx_fit_host_expand4(int32_t, int32_t, const int32_t*, const double*, const double*, const double*, double*);
int lsx_fit_host_normal4(int32_t, int32_t, int32_t, const int32_t*, const double*, const double*, const double*, const double*,
                         const double*, int32_t, int32_t, const int32_t*, const double*, double*, double*, double*);
}

static int fail(const char* what) { fprintf(stderr, "%s\n", what); return 1; }

static void pattern(int n, std::vector<int32_t>& al, std::vector<double>& st, std::vector<double>& sh)
{
    for (int q = -1; q <= 1; ++q)
        for (int k = 0; k < n; ++k) { al.push_back(q); st.push_back(1.0 / n); sh.push_back(1.2 * q + 0.1 * (k - 0.5 * (n - 1))); }
}

static int popcount4(uint32_t p) { return (p & 1) + ((p >> 1) & 1) + ((p >> 2) & 1) + ((p >> 3) & 1); }

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
        // one line with a pattern, one without: the velocity moves both
        std::vector<int32_t> nc(nl, 0), al; std::vector<double> st, sh;
        pattern(9, al, st, sh); nc[0] = 27;
        const double amp[4] = {0.01, 0.02, 0.03, 250.0};
        auto call = [&](const double* v, double mu, int lower_zero, uint32_t params, const double* a, int32_t nk, const int32_t* ks, double* rf,
                        double* S) {
            return lsx_stokes_host_response_v(Ns, nla, z.data(), T.data(), wav.data(), chi.data(), eta.data(), nl, l0.data(), nd.data(), ne.data(),
                                              aD.data(), vB.data(), act.data(), nc.data(), al.data(), st.data(), sh.data(), v, B.data(), g.data(),
                                              x.data(), mu, lower_zero, 0, params, a, nk, ks, rf, S);
        };
        // ---- all depths, every set of the four parameters, both boundaries; stokes has the window call's bits ----
        std::vector<double> full, old3;
        for (double mu : {1.0, 0.1})
            for (int lower_zero = 0; lower_zero < 2; ++lower_zero)
                for (uint32_t params = 1; params < 16; ++params) {
                    const int npar = popcount4(params);
                    std::vector<double> rf((size_t)npar * 4 * nla * Ns, NAN), S(4 * (size_t)nla, NAN), W(4 * (size_t)nla, NAN);
                    if (call(vl.data(), mu, lower_zero, params, amp, Ns, nullptr, rf.data(), S.data()) != LSX_OK) return fail("a response refused");
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
                    if (call(vl.data(), mu, lower_zero, params, amp, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("stokes == null refused");
                    if (mu == 1.0 && !lower_zero && params == 15) full = rf;
                    if (mu == 1.0 && !lower_zero && params == 7) old3 = rf;
                }
        // ---- the rows of B, gammaB, chiB: those of the entry without vlos, and of the four-parameter call ----
        {
            std::vector<double> rf((size_t)3 * 4 * nla * Ns, NAN);
            if (lsx_stokes_host_response(Ns, nla, z.data(), T.data(), wav.data(), chi.data(), eta.data(), nl, l0.data(), nd.data(), ne.data(),
                                         aD.data(), vB.data(), act.data(), nc.data(), al.data(), st.data(), sh.data(), vl.data(), B.data(), g.data(),
                                         x.data(), 1.0, 0, 0, 7, amp, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("the old entry refused");
            for (size_t i = 0; i < rf.size(); ++i)
                if (!(rf[i] == old3[i]) || !(rf[i] == full[i])) return fail("a field row depends on the velocity's being requested");
        }
        // ---- subsets of the depths: the entries of the full call ----
        const std::vector<std::vector<int32_t>> subsets = {{0}, {Ns - 1}, {0, Ns - 1}, {1, 2}, {Ns - 2}, {0, 1, 2}, {Ns / 2}};
        for (const auto& ks : subsets) {
            const int nk = (int)ks.size();
            std::vector<double> rf((size_t)4 * 4 * nla * nk, NAN);
            if (call(vl.data(), 1.0, 0, 15, amp, nk, ks.data(), rf.data(), nullptr) != LSX_OK) return fail("a subset refused");
            for (int i = 0; i < 4 * 4 * nla; ++i)
                for (int j = 0; j < nk; ++j)
                    if (!(rf[(size_t)i * nk + j] == full[(size_t)i * Ns + ks[j]])) return fail("a subset's entry is not the full call's");
            std::vector<double> one((size_t)4 * nla * nk, NAN);
            if (call(vl.data(), 1.0, 0, 8, amp, nk, ks.data(), one.data(), nullptr) != LSX_OK) return fail("vlos alone refused");
            for (size_t i = 0; i < one.size(); ++i)
                if (!(one[i] == rf[(size_t)3 * 4 * nla * nk + i])) return fail("vlos alone is not the fourth row of the full call");
        }
        // ---- refusals ----
        std::vector<double> rf((size_t)4 * 4 * nla * Ns, NAN);
        if (call(vl.data(), 1.0, 0, 0, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("params = 0 accepted");
        if (call(vl.data(), 1.0, 0, 16, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("an unknown bit accepted");
        if (call(vl.data(), 1.0, 0, 15, nullptr, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("null amplitudes accepted");
        if (call(nullptr, 1.0, 0, 15, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("a null velocity accepted");
        for (double bad : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
            double a[4] = {amp[0], amp[1], amp[2], bad};
            if (call(vl.data(), 1.0, 0, 8, a, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("a bad amplitude of vlos accepted");
            if (call(vl.data(), 1.0, 0, 7, a, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("an amplitude that is not requested was read");
        }
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
            std::vector<double> v(vl);
            v[Ns / 2] = bad;
            if (call(v.data(), 1.0, 0, 15, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("a velocity that is not finite accepted");
            if (call(v.data(), 1.0, 0, 1, amp, Ns, nullptr, rf.data(), nullptr) != LSX_EINVAL) return fail("a velocity that is not finite accepted (B alone)");
        }
        {   // no lower bound: a large negative velocity is a velocity
            std::vector<double> v(Ns, -9.0e4);
            if (call(v.data(), 1.0, 0, 15, amp, Ns, nullptr, rf.data(), nullptr) != LSX_OK) return fail("a negative velocity refused");
        }

        // ---- the sums with four quantities: 1 to 24 rows, with and without an instrument ----
        const int nmu = 2;
        for (const std::vector<int32_t>& nn : std::vector<std::vector<int32_t>>{{0, 0, 0, 1}, {1, 0, 0, 2}, {2, 2, 2, 2}, {6, 6, 6, 6}, {0, 3, 0, 0}}) {
            int P = 0, npar = 0;
            for (int a = 0; a < 4; ++a) { P += nn[a]; npar += nn[a] > 0; }
            std::vector<double> basis((size_t)P * Ns), base((size_t)4 * Ns), nodes(P), fld((size_t)4 * Ns, NAN);
            for (int j = 0; j < P; ++j)
                for (int k = 0; k < Ns; ++k) basis[(size_t)j * Ns + k] = std::cos(0.3 * j + 0.2 * k);
            for (size_t i = 0; i < base.size(); ++i) base[i] = 0.01 * (double)i;
            for (int j = 0; j < P; ++j) nodes[j] = 1.0 + 0.1 * j;
            if (lsx_fit_host_expand4(Ns, 1, nn.data(), basis.data(), base.data(), nodes.data(), fld.data()) != LSX_OK) return fail("expand4 refused");
            if (lsx_fit_host_expand4(Ns, 1, nn.data(), basis.data(), nullptr, nodes.data(), fld.data()) != LSX_OK) return fail("expand4 without base refused");
            for (double v : fld)
                if (!std::isfinite(v)) return fail("an expanded value is not finite");
            const size_t M = (size_t)4 * nla * nmu;
            std::vector<double> rfx((size_t)npar * 4 * nla * Ns * nmu), S(M), obs(M), w(M);
            for (size_t i = 0; i < rfx.size(); ++i) rfx[i] = std::sin(0.01 * (double)i);
            for (size_t i = 0; i < M; ++i) { S[i] = 1.0 + 0.01 * (double)i; obs[i] = S[i] + 0.05 * std::cos((double)i); w[i] = i % 5 ? 1.0 + 0.1 * (double)(i % 3) : 0.0; }
            double chi2 = NAN, c2 = NAN;
            std::vector<double> grad(P, NAN), hess((size_t)P * P, NAN);
            if (lsx_fit_host_normal4(Ns, nla, nmu, nn.data(), rfx.data(), S.data(), obs.data(), w.data(), basis.data(), 0, 0, nullptr, nullptr,
                                     &chi2, grad.data(), hess.data()) != LSX_OK) return fail("normal4 refused");
            if (lsx_fit_host_normal4(Ns, nla, nmu, nn.data(), nullptr, S.data(), obs.data(), w.data(), nullptr, 0, 0, nullptr, nullptr, &c2, nullptr,
                                     nullptr) != LSX_OK) return fail("normal4 (chi2 alone) refused");
            if (!(c2 == chi2)) return fail("chi2 alone is not the normal call's");
            for (double v : grad)
                if (!std::isfinite(v)) return fail("grad is not finite");
            for (int a = 0; a < P; ++a)
                for (int b = 0; b < P; ++b)
                    if (!std::isfinite(hess[(size_t)a * P + b]) || !(hess[(size_t)a * P + b] == hess[(size_t)b * P + a])) return fail("hess is not symmetric");
            // through an instrument: 3 pixels of width 3
            const int nobs = 3, width = 3;
            const int32_t first[nobs] = {0, 2, nla - width};
            std::vector<double> iw((size_t)nobs * width, 1.0 / width), ob2((size_t)4 * nobs * nmu, 1.0), w2((size_t)4 * nobs * nmu, 1.0);
            if (lsx_fit_host_normal4(Ns, nla, nmu, nn.data(), rfx.data(), S.data(), ob2.data(), w2.data(), basis.data(), nobs, width, first, iw.data(),
                                     &chi2, grad.data(), hess.data()) != LSX_OK) return fail("normal4 through an instrument refused");
            if (!std::isfinite(chi2)) return fail("chi2 through an instrument is not finite");
        }
        const int32_t none[4] = {0, 0, 0, 0}, many[4] = {6, 6, 6, 7}, neg[4] = {1, 0, 0, -1};
        std::vector<double> big((size_t)25 * Ns, 1.0), out((size_t)4 * Ns);
        for (const int32_t* nn : {none, many, neg})
            if (lsx_fit_host_expand4(Ns, 1, nn, big.data(), nullptr, big.data(), out.data()) != LSX_EINVAL) return fail("bad node counts accepted");
    }
    printf("STOKES VELOCITY SANITIZED RUN COMPLETE\n");
    return 0;
}
