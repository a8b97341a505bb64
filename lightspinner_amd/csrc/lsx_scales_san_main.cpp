// lsx_scales_san_main.cpp -- a stand-alone program (`make scalessan`) that runs the depth-scale conversion of lsx_scales_dev.h,
// through the equation of state and the opacity of lsx_background_dev.h, on the columns of a binary dump, built with
// -fsanitize=address,undefined (tests/test_scales_host.py writes the dump and runs it as a subprocess).  Every column is
// converted on its own scale, then its height and its tau500 are fed back on the other two, with every combination of outputs left out.
// Dump, native byte order: int32 npf, nelem, ncol, Ns; tpf[npf]; int32 nstage[nelem]; pf[nelem][6][npf]; eion[nelem][6]; abund[99];
// amass[99]; weight_per_H; gravity; cmass[ncol][Ns]; temperature[ncol][Ns]; nHTot[ncol][Ns]; ne[ncol][Ns]; doubles where not said.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/lsx_hip_scales.h"

extern "C" {
const char* lsx_scales_host_error(void);
double lsx_scales_host_tau1(int32_t, const double*, const double*);
int lsx_scales_host_convert(const lsx_eos_tables*, int32_t, int64_t, int32_t, const double*, const double*, const double*, const double*,
                            double, double*, double*, double*, double*);
}

template <typename T>
static std::vector<T> take(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short dump\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s dump\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> h = take<int32_t>(f, 4);
    const int npf = h[0], nelem = h[1], ncol = h[2], Ns = h[3];
    if (npf < 2 || nelem < 1 || nelem > 99 || ncol < 1 || Ns < 2) { fprintf(stderr, "bad header\n"); return 2; }
    const auto tpf = take<double>(f, (size_t)npf);
    const auto nstage = take<int32_t>(f, (size_t)nelem);
    const auto pf = take<double>(f, (size_t)nelem * 6 * npf);
    const auto eion = take<double>(f, (size_t)nelem * 6);
    const auto abund = take<double>(f, 99), amass = take<double>(f, 99), wph = take<double>(f, 1), grav = take<double>(f, 1);
    const size_t npts = (size_t)ncol * Ns;
    const auto cm = take<double>(f, npts), T = take<double>(f, npts), nH = take<double>(f, npts), ne = take<double>(f, npts);
    fclose(f);
    lsx_eos_tables tab{};
    tab.npf = npf; tab.nelem = nelem; tab.tpf = tpf.data(); tab.nstage = nstage.data(); tab.pf = pf.data(); tab.eion = eion.data();
    tab.abund = abund.data(); tab.amass = amass.data(); tab.weight_per_H = wph[0];
    std::vector<double> hgt(npts), tau(npts), chi(npts), a(npts), b(npts), c(npts);
    if (lsx_scales_host_convert(&tab, LSX_SCALE_COLUMN_MASS, ncol, Ns, cm.data(), T.data(), nH.data(), nullptr, grav[0], hgt.data(), a.data(),
                                tau.data(), chi.data())) { fprintf(stderr, "column mass: %s\n", lsx_scales_host_error()); return 1; }
    printf("column mass: height %.17g .. %.17g, tau %.17g .. %.17g\n", hgt[0], hgt[npts - 1], tau[0], tau[npts - 1]);
    const double* in[3] = {hgt.data(), cm.data(), tau.data()};
    for (int scale = 0; scale < 3; ++scale)
        for (int mask = 0; mask < 8; ++mask) {
            const int rc = lsx_scales_host_convert(&tab, scale, ncol, Ns, in[scale], T.data(), nH.data(), scale == 0 ? ne.data() : nullptr, grav[0],
                                                   mask & 1 ? a.data() : nullptr, mask & 2 ? b.data() : nullptr, mask & 4 ? c.data() : nullptr,
                                                   chi.data());
            if (rc) { fprintf(stderr, "scale %d, outputs %d: %d %s\n", scale, mask, rc, lsx_scales_host_error()); return 1; }
        }
    // a column of two depths, and the rule for tau = 1 at a grid point, below the first and above the last
    if (lsx_scales_host_convert(&tab, LSX_SCALE_TAU500, 1, 2, tau.data(), T.data(), nH.data(), nullptr, grav[0], a.data(), b.data(), c.data(), chi.data())) return 1;
    const double t3[3] = {0.5, 1.0, 2.0}, h3[3] = {3.0, 2.0, 1.0}, t2[2] = {2.0, 3.0}, t1[2] = {0.25, 0.5};
    if (lsx_scales_host_tau1(3, t3, h3) != 2.0 || lsx_scales_host_tau1(2, t2, h3) != 3.0 || lsx_scales_host_tau1(2, t1, h3) != 2.0) {
        fprintf(stderr, "tau = 1 rule\n");
        return 1;
    }
    tab.iter_cap = 3;       // a cap every point hits: LSX_ENOCONV, nothing integrated
    if (lsx_scales_host_convert(&tab, LSX_SCALE_COLUMN_MASS, ncol, Ns, cm.data(), T.data(), nH.data(), nullptr, grav[0], a.data(), b.data(),
                                c.data(), chi.data()) != LSX_ENOCONV) { fprintf(stderr, "cap 3 did not give LSX_ENOCONV\n"); return 1; }
    printf("SCALES SANITIZED RUN COMPLETE\n");
    return 0;
}
