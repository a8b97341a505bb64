// lsx_background_san_main.cpp -- a stand-alone program (`make bgsan`) that runs the formulas of lsx_background_dev.h on the points
// and wavelengths of a binary dump, built with -fsanitize=address,undefined: the clamped table indices of COULFF, Mg1OP, Si1OP,
// Si2OP and _itep1 are what it is for (tests/test_background_host.py writes the dump and runs it as a subprocess).
// Dump, native byte order: int32 npf, nelem, npts, nla; tpf[npf]; int32 nstage[nelem]; pf[nelem][6][npf]; eion[nelem][6]; abund[99];
// amass[99]; weight_per_H; temperature[npts]; nHTot[npts]; wavelength[nla] (nm); doubles where not said otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/lsx_hip_background.h"

extern "C" {
const char* lsx_bg_host_error(void);
int lsx_bg_host_eos(const lsx_eos_tables*, int64_t, const double*, const double*, double*, double*, double*, int32_t*);
int lsx_bg_host_opacity(int64_t, const double*, const double*, const double*, const double*, int32_t, const double*, double*, double*);
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
    const int npf = h[0], nelem = h[1], npts = h[2], nla = h[3];
    if (npf < 2 || nelem < 1 || nelem > 99 || npts < 1 || nla < 1) { fprintf(stderr, "bad header\n"); return 2; }
    const auto tpf = take<double>(f, (size_t)npf);
    const auto nstage = take<int32_t>(f, (size_t)nelem);
    const auto pf = take<double>(f, (size_t)nelem * 6 * npf);
    const auto eion = take<double>(f, (size_t)nelem * 6);
    const auto abund = take<double>(f, 99), amass = take<double>(f, 99), wph = take<double>(f, 1);
    const auto T = take<double>(f, (size_t)npts), nH = take<double>(f, (size_t)npts), wl = take<double>(f, (size_t)nla);
    fclose(f);
    lsx_eos_tables tab{};
    tab.npf = npf; tab.nelem = nelem; tab.tpf = tpf.data(); tab.nstage = nstage.data(); tab.pf = pf.data(); tab.eion = eion.data();
    tab.abund = abund.data(); tab.amass = amass.data(); tab.weight_per_H = wph[0];
    std::vector<double> pg((size_t)npts), pe((size_t)npts), part((size_t)npts * 17), chi((size_t)npts * nla), eta((size_t)npts * nla);
    std::vector<int32_t> st((size_t)npts);
    for (int cap : {0, 3}) {      // the reference's caps, then a cap every point hits
        tab.iter_cap = cap;
        const int rc = lsx_bg_host_eos(&tab, npts, T.data(), nH.data(), pg.data(), pe.data(), part.data(), st.data());
        if (rc != (cap ? LSX_ENOCONV : LSX_OK)) { fprintf(stderr, "eos (cap %d): %d %s\n", cap, rc, lsx_bg_host_error()); return 1; }
        if (!cap && lsx_bg_host_opacity(npts, T.data(), pg.data(), pe.data(), part.data(), nla, wl.data(), chi.data(), eta.data())) return 1;
        double s = 0.0;
        for (double x : chi) s += x;
        printf("cap %d: %d points x %d wavelengths, sum chi %.17g, status[0] %d\n", cap, npts, nla, s, st[0]);
    }
    printf("BG SANITIZED RUN COMPLETE\n");
    return 0;
}
