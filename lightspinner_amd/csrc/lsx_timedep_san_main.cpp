// lsx_timedep_san_main.cpp -- a stand-alone program (`make tdsan`) that runs the solve of lsx_solve_dev.h through the entries of
// lsx_timedep_host.cpp -- the implicit rate-equation step, then the statistical equilibrium -- built with
// -fsanitize=address,undefined (tests/test_time_dependent_host.py runs it as a subprocess): 13 depths x 25 columns = 325 systems
// of every size 2 ... 16, rates over twelve decades, dt over sixteen, in the register form and the in-memory form (work strides 1
// and 64), one frozen column, one singular and one NaN system, and the refusals.  Each result must be finite and positive,
// conserve the number density (the step: the sum of n_prev; the equilibrium: nTotal), and agree between the two forms bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int lsx_timedep_host(int32_t, int32_t, int32_t, const double*, const double*, const double*, double*, double*, uint8_t*,
                                const uint8_t*, int32_t, int32_t);
extern "C" int lsx_statequil_host(int32_t, int32_t, int32_t, const double*, const double*, double*, double*, uint8_t*, const uint8_t*,
                                  int32_t, int32_t);

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static double uniform()         // xorshift64*: [0, 1)
{
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return (double)((g_state * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}

// se: the statistical equilibrium on the same systems (np[level 0] of a point stands in for its nTotal)
static int run(int Nl, bool se)
{
    const int Ns = 13, nc = 25, sc = 7, sk = 5, nanc = 11, nank = 2, frozen = 19;
    const size_t per = (size_t)Nl * Ns;
    std::vector<double> G((size_t)nc * Nl * Nl * Ns), np(nc * per), n0(nc * per), dt(nc);
    std::vector<uint8_t> active(nc, 1);
    active[frozen] = 0;
    for (int c = 0; c < nc; ++c) {
        dt[c] = std::pow(10.0, -8.0 + 16.0 * c / (nc - 1));
        for (int k = 0; k < Ns; ++k) {
            double* g = G.data() + (size_t)c * Nl * Nl * Ns + k;
            for (int j = 0; j < Nl; ++j) {
                double sum = 0.0;
                for (int i = 0; i < Nl; ++i)
                    if (i != j) { const double r = std::pow(10.0, -6.0 + 12.0 * uniform()); g[(size_t)(i * Nl + j) * Ns] = r; sum += r; }
                g[(size_t)(j * Nl + j) * Ns] = -sum;
            }
            for (int l = 0; l < Nl; ++l) {
                np[c * per + (size_t)l * Ns + k] = 1e14 * std::pow(10.0, -3.0 * uniform());
                n0[c * per + (size_t)l * Ns + k] = 1e14 * std::pow(10.0, -3.0 * uniform());
            }
        }
    }
    // a singular system: Gamma = I / dt (dt a power of two: exact), for the equilibrium Gamma = 0, leaves rows of zeros beside
    // the row of ones
    dt[sc] = 0.25;
    for (int i = 0; i < Nl; ++i)
        for (int j = 0; j < Nl; ++j) G[(size_t)sc * Nl * Nl * Ns + (size_t)(i * Nl + j) * Ns + sk] = i == j && !se ? 1.0 / dt[sc] : 0.0;
    G[(size_t)nanc * Nl * Nl * Ns + (size_t)(1 * Nl + 0) * Ns + nank] = NAN;
    G[(size_t)nanc * Nl * Nl * Ns + (size_t)(0 * Nl + 0) * Ns + nank] = NAN;

    std::vector<double> out[3];
    std::vector<double> dP[3];
    const int forms[3][2] = {{0, 1}, {1, 1}, {1, 64}};
    for (int f = 0; f < 3; ++f) {
        out[f] = n0;
        dP[f].assign(nc, -1.0);
        std::vector<uint8_t> sing((size_t)nc * Ns, 9);
        // (the equilibrium's nTotal [nc][Ns]: the first Ns entries of each column of np, i.e. level 0)
        std::vector<double> ntot((size_t)nc * Ns);
        for (int c = 0; c < nc; ++c) memcpy(&ntot[(size_t)c * Ns], &np[c * per], Ns * sizeof(double));
        const int rc = se ? lsx_statequil_host(Nl, Ns, nc, G.data(), ntot.data(), out[f].data(), dP[f].data(), sing.data(), active.data(),
                                               forms[f][0], forms[f][1])
                          : lsx_timedep_host(Nl, Ns, nc, G.data(), np.data(), dt.data(), out[f].data(), dP[f].data(), sing.data(),
                                             active.data(), forms[f][0], forms[f][1]);
        if (rc) { fprintf(stderr, "Nl %d: refused\n", Nl); return 1; }
        for (int c = 0; c < nc; ++c)
            for (int k = 0; k < Ns; ++k) {
                const bool want_sing = (c == sc && k == sk) || (c == nanc && k == nank);
                if ((sing[(size_t)c * Ns + k] != 0) != (want_sing && c != frozen)) { fprintf(stderr, "Nl %d form %d: flag at (%d, %d)\n", Nl, f, c, k); return 1; }
                double sum = 0.0, want = 0.0;
                for (int l = 0; l < Nl; ++l) {
                    const size_t e = c * per + (size_t)l * Ns + k;
                    const double v = out[f][e];
                    if (c == frozen || want_sing) {
                        if (memcmp(&v, &n0[e], 8)) { fprintf(stderr, "Nl %d form %d: (%d, %d) touched\n", Nl, f, c, k); return 1; }
                        continue;
                    }
                    if (!std::isfinite(v) || !(v > 0.0)) { fprintf(stderr, "Nl %d form %d: level %d at (%d, %d): %g\n", Nl, f, l, c, k, v); return 1; }
                    sum += v;
                    want += np[e];
                }
                if (se && c != frozen && !want_sing) want = ntot[(size_t)c * Ns + k];
                if (std::fabs(sum - want) > 1e-9 * want) { fprintf(stderr, "Nl %d form %d: (%d, %d): %.17g levels sum, %.17g wanted\n", Nl, f, c, k, sum, want); return 1; }
            }
        if (dP[f][frozen] != 0.0) { fprintf(stderr, "Nl %d form %d: monitor of the frozen column\n", Nl, f); return 1; }
        for (int c = 0; c < nc; ++c)
            if (!(dP[f][c] >= 0.0)) { fprintf(stderr, "Nl %d form %d: monitor %g\n", Nl, f, dP[f][c]); return 1; }
    }
    // the register form (2 ... 8 levels) and the in-memory form at both strides: the same bits
    for (int f = 1; f < 3; ++f)
        if (memcmp(out[0].data(), out[f].data(), out[0].size() * 8) || memcmp(dP[0].data(), dP[f].data(), dP[0].size() * 8)) {
            fprintf(stderr, "Nl %d: form %d differs from form 0\n", Nl, f);
            return 1;
        }
    return 0;
}

int main()
{
    for (int se = 0; se < 2; ++se)
        for (int Nl = 2; Nl <= 16; ++Nl)
            if (run(Nl, se != 0)) return 1;
    // refusals: nothing is read past what the checks allow
    std::vector<double> x(2 * 2 * 3, 1.0), dt(1, 1.0), dp(1);
    std::vector<uint8_t> s(3);
    int refused = 0;
    refused += lsx_timedep_host(1, 3, 1, x.data(), x.data(), dt.data(), x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    refused += lsx_timedep_host(17, 3, 1, x.data(), x.data(), dt.data(), x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    refused += lsx_timedep_host(2, 3, 1, nullptr, x.data(), dt.data(), x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    refused += lsx_timedep_host(2, 3, 1, x.data(), x.data(), nullptr, x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    for (double bad : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
        dt[0] = bad;
        refused += lsx_timedep_host(2, 3, 1, x.data(), x.data(), dt.data(), x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    }
    dt[0] = 1.0;
    refused += lsx_statequil_host(1, 3, 1, x.data(), x.data(), x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    refused += lsx_statequil_host(17, 3, 1, x.data(), x.data(), x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    refused += lsx_statequil_host(2, 3, 1, x.data(), nullptr, x.data(), dp.data(), s.data(), nullptr, 0, 1) == 1;
    refused += lsx_statequil_host(2, 3, 1, x.data(), x.data(), x.data(), dp.data(), s.data(), nullptr, 0, 0) == 1;
    if (refused != 12) { fprintf(stderr, "%d of 12 refusals\n", refused); return 1; }
    printf("TIMEDEP SANITIZED RUN COMPLETE\n");
    return 0;
}
