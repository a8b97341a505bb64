// lsx_background_prep.h -- host side of the background entries: checks of lsx_eos_tables and what witt.__init__ derives from the
// abundances (witt.py:166-176), shared by lsx_background.hip and the CPU build of the formulas (lsx_background_host.cpp).
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lsx_hip_background.h"
#include "lsx_background_dev.h"

namespace lsxbg {

struct HostTables {              // the normalised abundances and the scalars; pointers of P still refer to the caller's arrays
    EosParams P{};
    std::vector<double> abund;
};

// "" if tab is usable, else what is wrong with it
inline std::string prepare_tables(const lsx_eos_tables* t, HostTables* H)
{
    char b[160];
    if (!t || !t->tpf || !t->nstage || !t->pf || !t->eion || !t->abund || !t->amass) return "null table pointer";
    if (t->nelem < NCONTR || t->nelem > 99) { snprintf(b, sizeof b, "nelem = %d, need %d .. 99", t->nelem, NCONTR); return b; }
    if (t->npf < 2) return "npf < 2";
    if (t->iter_cap < 0) return "iter_cap < 0";
    for (int i = 0; i < t->npf; ++i)
        if (!std::isfinite(t->tpf[i]) || (i && !(t->tpf[i] > t->tpf[i - 1]))) { snprintf(b, sizeof b, "tpf is not strictly ascending at %d", i); return b; }
    for (int e = 0; e < t->nelem; ++e)
        if (t->nstage[e] < 1 || t->nstage[e] > 6) { snprintf(b, sizeof b, "nstage[%d] = %d outside 1..6", e, t->nstage[e]); return b; }
    // the stages witt.getBackgroundPartials reads (witt.py:676-737); H: pe_pg / gasc read two
    static const int need[10][2] = {{0, 2}, {1, 3}, {5, 1}, {6, 1}, {7, 1}, {11, 2}, {12, 1}, {13, 2}, {19, 2}, {25, 1}};
    for (auto& n : need)
        if (t->nstage[n[0]] < n[1]) { snprintf(b, sizeof b, "element %d has %d stages, the opacity reads %d", n[0] + 1, t->nstage[n[0]], n[1]); return b; }
    for (int i = 0; i < 99; ++i)
        if (!std::isfinite(t->abund[i]) || !std::isfinite(t->amass[i]) || t->abund[i] < 0.0) return "non-finite abundance or mass";
    if (!(t->abund[0] > 0.0) || !std::isfinite(t->weight_per_H) || !(t->weight_per_H > 0.0)) return "abund[0] or weight_per_H not positive";

    H->abund.assign(t->abund, t->abund + 99);
    double abtot = 0.0;
    for (double a : H->abund) abtot += a;
    for (double& a : H->abund) a /= abtot;
    double others = 0.0, avw = 0.0;
    for (int i = 1; i < 99; ++i) others += H->abund[i];
    for (int i = 0; i < 99; ++i) avw += H->abund[i] * t->amass[i];
    EosParams& P = H->P;
    P.npf = t->npf; P.nelem = t->nelem;
    P.cap_pg = t->iter_cap > 0 ? t->iter_cap : 250;
    P.cap_rho = t->iter_cap > 0 ? t->iter_cap : 250;
    P.cap_pgrho = t->iter_cap > 0 ? t->iter_cap : 100;
    P.tpf = t->tpf; P.pf = t->pf; P.eion = t->eion; P.nstage = t->nstage; P.abund = H->abund.data();
    P.ab_others = others / H->abund[0];
    const double muH = avw / t->amass[0] / H->abund[0];
    P.rho_from_H = muH * t->amass[0] * AMU / BK;
    P.avw = avw * AMU;
    P.saha_fac = std::pow((2.0 * PI * ME * BK) / (HH * HH), 1.5);
    P.rho_unit = 1.6605402E-27 * t->weight_per_H;      // constants.py:6, background.py:32
    P.cm3 = std::pow(1.0E-02, 3.0);
    P.g_to_kg = 1.0E-03;
    return "";
}

// the first value of a[0..n) that is not finite or not > 0, or -1
inline long first_bad_positive(const double* a, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i]) || !(a[i] > 0.0)) return (long)i;
    return -1;
}

// background.py:10-13
inline double thomson_sigma()
{
    const double QElectron = 1.60217733E-19, Epsilon0 = 8.854187817E-12, MElectron = 9.1093897E-31, CLight = 2.99792458E+08;
    const double pi = 3.141592653589793;
    return 8.0 * pi / 3.0 * std::pow(QElectron / (std::sqrt(4.0 * pi * Epsilon0) * (std::sqrt(MElectron) * CLight)), 4.0);
}

} // namespace lsxbg
