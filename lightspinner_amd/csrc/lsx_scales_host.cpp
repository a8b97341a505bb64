// lsx_scales_host.cpp -- the formulas of lsx_scales_dev.h compiled for the CPU (g++ -ffp-contract=off): a test-only library
// (liblsx_scales_host.so, `make scaleshost`, built together with lsx_background_host.cpp) that integrates columns given chi_c, or
// through lsx_bg_host_eos / lsx_bg_host_opacity for the whole path, so that a deviation from the reference can be traced without
// a GPU, and so that the integration runs under -fsanitize=address,undefined (lsx_scales_san_main.cpp).
#include <vector>

#include "lsx_scales_dev.h"
#include "lsx_scales_prep.h"

using namespace lsxsc;

extern "C" {
int lsx_bg_host_eos(const lsx_eos_tables*, int64_t, const double*, const double*, double*, double*, double*, int32_t*);
int lsx_bg_host_opacity(int64_t, const double*, const double*, const double*, const double*, int32_t, const double*, double*, double*);
const char* lsx_bg_host_error(void);
}

static thread_local std::string g_sc_err;

template <int SCALE>
static void column(int Ns, double wph, double gravity, const double* ds, const double* T, const double* nH, const double* ne,
                   const double* chi, double* height, double* cmass, double* tau)
{
    const double amu_wph = 1.6605402E-27 * wph;        // constants.py:6 (EosParams::rho_unit)
    Run R{};
    for (int k = 0; k < Ns; ++k) {
        const double rho = rho_si(amu_wph, nH[k]);
        if (k == 0) start<SCALE>(R, ds[0], ds[1], rho, chi[0], T[0], nH[0], ne ? ne[0] : 0.0, wph, gravity);
        else step<SCALE>(R, ds[k], rho, chi[k]);
        if (height) height[k] = R.height;
        if (cmass) cmass[k] = R.cmass;
        if (tau) tau[k] = R.tau;
    }
    if (SCALE != GEOMETRIC && height) {
        const double h1 = tau1_last(R.t1, R.height);
        for (int k = 0; k < Ns; ++k) height[k] -= h1;
    }
}

extern "C" {

const char* lsx_scales_host_error(void) { return g_sc_err.c_str(); }

// the checks of lsx_hip_convert_scales that need no device
int lsx_scales_host_check(int32_t scale, int64_t ncol, int32_t Ns, const double* ds, const double* T, const double* nH, const double* ne,
                          double gravity)
{
    g_sc_err = check_arrays(scale, (long)ncol, Ns, ds, T, nH, ne, gravity);
    return g_sc_err.empty() ? LSX_OK : LSX_EINVAL;
}

// np.interp(1.0, tau, height) by the on-the-fly rule of lsx_scales_dev.h
double lsx_scales_host_tau1(int32_t n, const double* tau, const double* height)
{
    Tau1 q;
    tau1_first(q, tau[0], height[0]);
    for (int32_t k = 1; k < n; ++k) tau1_next(q, tau[k - 1], height[k - 1], tau[k], height[k]);
    return tau1_last(q, height[n - 1]);
}

// the integration alone: columns [ncol][Ns] given chi_c; any of height, cmass, tau may be NULL
int lsx_scales_host_integrate(int32_t scale, int64_t ncol, int32_t Ns, double weight_per_H, const double* ds, const double* T,
                              const double* nH, const double* ne, double gravity, const double* chi_c, double* height, double* cmass,
                              double* tau)
{
    const int rc = lsx_scales_host_check(scale, ncol, Ns, ds, T, nH, ne, gravity);
    if (rc) return rc;
    for (int64_t c = 0; c < ncol; ++c) {
        const size_t o = (size_t)c * Ns;
        auto at = [o](auto* p) { return p ? p + o : p; };
        if (scale == COLUMN_MASS) column<COLUMN_MASS>(Ns, weight_per_H, gravity, ds + o, T + o, nH + o, at(ne), chi_c + o, at(height), at(cmass), at(tau));
        else if (scale == GEOMETRIC) column<GEOMETRIC>(Ns, weight_per_H, gravity, ds + o, T + o, nH + o, at(ne), chi_c + o, at(height), at(cmass), at(tau));
        else column<TAU500>(Ns, weight_per_H, gravity, ds + o, T + o, nH + o, at(ne), chi_c + o, at(height), at(cmass), at(tau));
    }
    return LSX_OK;
}

// the whole chain: equation of state, opacity at 500 nm, integration; chi_c [ncol][Ns] is written too (not NULL)
int lsx_scales_host_convert(const lsx_eos_tables* tab, int32_t scale, int64_t ncol, int32_t Ns, const double* ds, const double* T,
                            const double* nH, const double* ne, double gravity, double* height, double* cmass, double* tau, double* chi_c)
{
    int rc = lsx_scales_host_check(scale, ncol, Ns, ds, T, nH, ne, gravity);
    if (rc) return rc;
    const size_t npts = (size_t)ncol * Ns;
    std::vector<double> pg(npts), pe(npts), part(npts * lsxbg::NPART), eta(npts);
    std::vector<int32_t> st(npts);
    rc = lsx_bg_host_eos(tab, (int64_t)npts, T, nH, pg.data(), pe.data(), part.data(), st.data());
    if (rc) { g_sc_err = lsx_bg_host_error(); return rc; }
    const double w = 500.0;
    lsx_bg_host_opacity((int64_t)npts, T, pg.data(), pe.data(), part.data(), 1, &w, chi_c, eta.data());
    return lsx_scales_host_integrate(scale, ncol, Ns, tab->weight_per_H, ds, T, nH, ne, gravity, chi_c, height, cmass, tau);
}

} // extern "C"
