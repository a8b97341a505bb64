// lsx_background_host.cpp -- the formulas of lsx_background_dev.h compiled for the CPU (g++ -ffp-contract=off): a test-only
// library (liblsx_bg_host.so, `make bghost`) that evaluates the equation of state and the opacity per point, so that a deviation
// from the reference can be traced operation by operation without a GPU, and so that the clamped table indices run under
// -fsanitize=address,undefined (lsx_background_san_main.cpp).
#include <cstring>

#include "lsx_background_prep.h"

using namespace lsxbg;

static thread_local std::string g_bg_err;

extern "C" {

const char* lsx_bg_host_error(void) { return g_bg_err.c_str(); }

// out[0..3): avw (g), ab_others, rho_from_H as witt.__init__ leaves them
int lsx_bg_host_derived(const lsx_eos_tables* tab, double* out)
{
    HostTables H;
    g_bg_err = prepare_tables(tab, &H);
    if (!g_bg_err.empty()) return LSX_EINVAL;
    out[0] = H.P.avw; out[1] = H.P.ab_others; out[2] = H.P.rho_from_H;
    return LSX_OK;
}

// npts points: pgas, pe [npts], partials [npts][17], status [npts] (lsx_hip_eos per point); the iteration cap is tab->iter_cap
int lsx_bg_host_eos(const lsx_eos_tables* tab, int64_t npts, const double* temperature, const double* nHTot, double* pgas, double* pe,
                    double* partials, int32_t* status)
{
    HostTables H;
    g_bg_err = prepare_tables(tab, &H);
    if (!g_bg_err.empty()) return LSX_EINVAL;
    if (first_bad_positive(temperature, (size_t)npts) >= 0 || first_bad_positive(nHTot, (size_t)npts) >= 0) {
        g_bg_err = "temperature / nHTot not finite and positive";
        return LSX_EINVAL;
    }
    int rc = LSX_OK;
    for (int64_t i = 0; i < npts; ++i) {
        status[i] = eos_solve(H.P, temperature[i], nHTot[i], pgas + i, pe + i, partials + i * NPART, 1);
        if (status[i] < 0 && rc == LSX_OK) {
            char b[96];
            snprintf(b, sizeof b, "equation of state: point %lld hit an iteration cap", (long long)i);
            g_bg_err = b;
            rc = LSX_ENOCONV;
        }
    }
    return rc;
}

// chi, eta [npts][nla] (SI, as background.py:40-43) from the outputs of lsx_bg_host_eos; wavelength in nm
int lsx_bg_host_opacity(int64_t npts, const double* temperature, const double* pgas, const double* pe, const double* partials,
                        int32_t nla, const double* wavelength, double* chi, double* eta)
{
    std::vector<OpWave> W((size_t)nla);
    for (int32_t l = 0; l < nla; ++l) make_wave(wavelength[l] * 10, &W[(size_t)l]);
    for (int64_t i = 0; i < npts; ++i) {
        OpLane L;
        make_lane(temperature[i], pgas[i], pe[i], partials + i * NPART, 1, &L);
        for (int32_t l = 0; l < nla; ++l) {
            const double x = cop_point(L, W[(size_t)l]) / 1.0E-02;
            chi[i * nla + l] = x;
            eta[i * nla + l] = planck_nm(temperature[i], wavelength[l]) * x;
        }
    }
    return LSX_OK;
}

} // extern "C"
