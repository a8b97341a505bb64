// lsx_scales_prep.h -- host side of lsx_hip_convert_scales: the checks of its arrays, shared by lsx_background.hip and the CPU
// build of the formulas (lsx_scales_host.cpp).
#pragma once
#include "../../include/lsx_hip_scales.h"
#include "lsx_background_prep.h"

namespace lsxsc {

// "" if the arrays of a call are usable, else what is wrong with them (include/lsx_hip_scales.h: LSX_EINVAL)
inline std::string check_arrays(int scale, long ncol, int Ns, const double* ds, const double* T, const double* nH, const double* ne,
                                double gravity)
{
    char b[200];
    if (scale != LSX_SCALE_GEOMETRIC && scale != LSX_SCALE_COLUMN_MASS && scale != LSX_SCALE_TAU500) { snprintf(b, sizeof b, "scale = %d is none of LSX_SCALE_*", scale); return b; }
    if (Ns < 2) return "Nspace < 2: a depth scale needs two depths";
    if (ncol < 1) return "ncol < 1";
    const bool geo = scale == LSX_SCALE_GEOMETRIC;
    if (!ds || !T || !nH || (geo && !ne)) return "a null input array";
    if (geo && (!std::isfinite(gravity) || !(gravity > 0.0))) return "gravity is not finite and positive";
    const size_t npts = (size_t)ncol * Ns;
    const double* arr[3] = {T, nH, ne};
    const char* name[3] = {"temperature", "nHTot", "ne"};
    for (int a = 0; a < (geo ? 3 : 2); ++a) {
        const long q = lsxbg::first_bad_positive(arr[a], npts);
        if (q >= 0) { snprintf(b, sizeof b, "%s of column %ld, depth %ld is not finite and positive", name[a], q / Ns, q % Ns); return b; }
    }
    for (size_t i = 0; i < npts; ++i)
        if (T[i] < 2500.0) { snprintf(b, sizeof b, "temperature of column %zu, depth %zu is below 2500 K", i / Ns, i % Ns); return b; }
    for (size_t i = 0; i < npts; ++i) {
        const size_t k = i % Ns;
        const bool ok = geo ? std::isfinite(ds[i]) && (k == 0 || ds[i] < ds[i - 1])
                            : std::isfinite(ds[i]) && ds[i] > 0.0 && (k == 0 || ds[i] > ds[i - 1]);
        if (!ok) {
            snprintf(b, sizeof b, "depth_scale of column %zu is not %s at depth %zu", i / Ns,
                     geo ? "finite and strictly descending" : "finite, positive and strictly ascending", k);
            return b;
        }
    }
    return "";
}

} // namespace lsxsc
