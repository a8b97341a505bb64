// lsx_eqpops_san_main.cpp -- a stand-alone program (`make eqpopssan`) that runs the LTE populations of lsx_eqpops_dev.h through
// the entry of lsx_eqpops_host.cpp, built with -fsanitize=address,undefined (tests/test_eqpops_host.py runs it as a subprocess):
// one to five atoms in a call, atoms of 1, 2 and 12 levels, dZ = 0 ... 3 inside one atom, 400 K and 1e6 K beside solar values, one
// and several columns, with and without nTotal, and every refusal.  Each result must be finite, non-negative and sum to nTotal.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/lsx_hip_eqpops.h"

extern "C" {
const char* lsx_eqpops_host_error(void);
int lsx_eqpops_host(int32_t, int32_t, const lsx_eq_atom*, int32_t, const double*, const double*, const double*, double*, double*);
}

static const double EV = 1.60217733E-19;

struct AtomSpec { std::vector<lsx_level> lev; double abundance; };

static AtomSpec make_atom(int nl, int stage0, int top_dZ, double abundance)
{
    AtomSpec a;
    a.abundance = abundance;
    for (int i = 0; i < nl; ++i) {
        lsx_level l{};
        const int dZ = nl == 1 ? 0 : (i * (top_dZ + 1)) / nl;          // 0 ... top_dZ, ascending
        l.E_SI = EV * (1.7 * i + 6.0 * dZ);
        l.g = 2.0 * (i % 4) + 1.0;
        l.stage = stage0 + dZ;
        a.lev.push_back(l);
    }
    return a;
}

static int run(const std::vector<AtomSpec>& specs, int ncol, int Ns, bool with_total)
{
    std::vector<lsx_eq_atom> atoms;
    int NLtot = 0;
    for (const AtomSpec& s : specs) {
        lsx_eq_atom a{};
        a.Nlevel = (int)s.lev.size(); a.levels = s.lev.data(); a.abundance = s.abundance;
        atoms.push_back(a);
        NLtot += a.Nlevel;
    }
    const size_t npts = (size_t)ncol * Ns;
    std::vector<double> T(npts), ne(npts), nH(npts), ns(npts * NLtot, -1.0), nt(npts * atoms.size(), -1.0);
    const double Ts[4] = {400.0, 4400.0, 9.0e4, 1.0e6}, nes[3] = {1.0e12, 1.0e18, 1.0e23};
    for (size_t i = 0; i < npts; ++i) { T[i] = Ts[i % 4]; ne[i] = nes[(i / 4) % 3]; nH[i] = i % 7 == 6 ? 0.0 : 1.0e16 * (1 + i % 5); }
    if (lsx_eqpops_host(Ns, (int)atoms.size(), atoms.data(), ncol, T.data(), ne.data(), nH.data(), ns.data(), with_total ? nt.data() : nullptr)) {
        fprintf(stderr, "refused: %s\n", lsx_eqpops_host_error());
        return 1;
    }
    for (int c = 0; c < ncol; ++c)
        for (int k = 0; k < Ns; ++k) {
            int o = 0;
            for (size_t a = 0; a < atoms.size(); ++a) {
                const double want = atoms[a].abundance * nH[(size_t)c * Ns + k];
                if (with_total && nt[((size_t)c * atoms.size() + a) * Ns + k] != want) { fprintf(stderr, "nTotal\n"); return 1; }
                double sum = 0.0;
                for (int i = 0; i < atoms[a].Nlevel; ++i) {
                    const double v = ns[((size_t)c * NLtot + o + i) * Ns + k];
                    if (!std::isfinite(v) || v < 0.0) { fprintf(stderr, "atom %zu level %d at (%d, %d): %g\n", a, i, c, k, v); return 1; }
                    sum += v;
                }
                if (atoms[a].Nlevel == 1 ? sum != want : std::fabs(sum - want) > 1e-12 * want) {
                    fprintf(stderr, "atom %zu at (%d, %d): levels sum to %.17g, nTotal %.17g\n", a, c, k, sum, want);
                    return 1;
                }
                o += atoms[a].Nlevel;
            }
        }
    return 0;
}

int main()
{
    const AtomSpec one = make_atom(1, 0, 0, 1.0), two = make_atom(2, 0, 1, 1e-4), twelve = make_atom(12, 0, 3, 2e-6),
                   flat = make_atom(5, 1, 0, 0.0), high = make_atom(12, 1, 2, 3e-5);
    const std::vector<AtomSpec> all = {one, two, twelve, flat, high};
    for (size_t n = 1; n <= all.size(); ++n)
        for (int ncol : {1, 3})
            for (int Ns : {1, 13})
                for (bool wt : {false, true})
                    if (run(std::vector<AtomSpec>(all.begin(), all.begin() + n), ncol, Ns, wt)) return 1;
    for (const AtomSpec& s : all)
        if (run({s}, 2, 12, true)) return 1;
    // refusals: nothing is read past what the checks allow
    std::vector<double> x(12, 5000.0), out(12 * 12);
    lsx_eq_atom a{};
    a.Nlevel = 12; a.levels = twelve.lev.data(); a.abundance = 1.0;
    int refused = 0;
    refused += lsx_eqpops_host(12, 0, &a, 1, x.data(), x.data(), x.data(), out.data(), nullptr) == LSX_EINVAL;
    refused += lsx_eqpops_host(12, 1, nullptr, 1, x.data(), x.data(), x.data(), out.data(), nullptr) == LSX_EINVAL;
    refused += lsx_eqpops_host(12, 1, &a, 0, x.data(), x.data(), x.data(), out.data(), nullptr) == LSX_EINVAL;
    refused += lsx_eqpops_host(12, 1, &a, 1, nullptr, x.data(), x.data(), out.data(), nullptr) == LSX_EINVAL;
    a.Nlevel = 0;
    refused += lsx_eqpops_host(12, 1, &a, 1, x.data(), x.data(), x.data(), out.data(), nullptr) == LSX_EINVAL;
    a.Nlevel = 12; a.abundance = -1.0;
    refused += lsx_eqpops_host(12, 1, &a, 1, x.data(), x.data(), x.data(), out.data(), nullptr) == LSX_EINVAL;
    if (refused != 6) { fprintf(stderr, "%d of 6 refusals\n", refused); return 1; }
    printf("EQPOPS SANITIZED RUN COMPLETE\n");
    return 0;
}
