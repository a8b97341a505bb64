// lsx_stokes_prep.h -- host side of lsx_hip_stokes_rays that needs no device: the rules for the field and for the Zeeman patterns,
// and the packing of the patterns into the table the kernel reads (lsx_stokes.hip; lsx_stokes_host.cpp and the sanitized program run
// the same functions).  Plain C++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lsx_hip_stokes.h"
#include "../../include/lsx_hip_stokes_response.h"
#include "lsx_stokes_dev.h"

namespace lsxst {

// B, gammaB, chiB: [count] each.  -> LSX_OK or LSX_EINVAL with a message
inline int check_field(size_t count, const double* B, const double* gammaB, const double* chiB, std::string& msg)
{
    char buf[160];
    for (size_t i = 0; i < count; ++i) {
        if (!std::isfinite(B[i]) || !std::isfinite(gammaB[i]) || !std::isfinite(chiB[i])) {
            snprintf(buf, sizeof buf, "the field at point %zu is not finite (B %g, gammaB %g, chiB %g)", i, B[i], gammaB[i], chiB[i]);
            msg = buf;
            return LSX_EINVAL;
        }
        if (B[i] < 0.0) {
            snprintf(buf, sizeof buf, "B = %g at point %zu is negative (turn the field round with gammaB)", B[i], i);
            msg = buf;
            return LSX_EINVAL;
        }
    }
    return LSX_OK;
}

// the patterns of nlines lines, one after the other.  -> LSX_OK, LSX_EINVAL or LSX_EUNSUPPORTED (a line over the cap) with a message
inline int check_patterns(int nlines, const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                          std::string& msg)
{
    char buf[200];
    size_t o = 0;
    for (int l = 0; l < nlines; ++l) {
        const int nc = ncomp[l];
        if (nc < 0) { snprintf(buf, sizeof buf, "line %d: ncomp = %d", l, nc); msg = buf; return LSX_EINVAL; }
        if (nc > LSX_STOKES_MAX_COMPONENTS) {
            snprintf(buf, sizeof buf, "line %d has %d Zeeman components; at most %d are supported", l, nc, LSX_STOKES_MAX_COMPONENTS);
            msg = buf;
            return LSX_EUNSUPPORTED;
        }
        if (nc == 0) continue;
        if (!alpha || !strength || !shift) { msg = "patterns are given (ncomp > 0) without alpha, strength or shift"; return LSX_EINVAL; }
        double sum[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < nc; ++k, ++o) {
            if (alpha[o] < -1 || alpha[o] > 1) {
                snprintf(buf, sizeof buf, "line %d, component %d: alpha = %d is not -1, 0 or +1", l, k, (int)alpha[o]);
                msg = buf;
                return LSX_EINVAL;
            }
            if (!std::isfinite(strength[o]) || !std::isfinite(shift[o])) {
                snprintf(buf, sizeof buf, "line %d, component %d: strength %g, shift %g", l, k, strength[o], shift[o]);
                msg = buf;
                return LSX_EINVAL;
            }
            sum[alpha[o] + 1] += strength[o];
        }
        for (int q = 0; q < 3; ++q)
            if (!(std::fabs(sum[q] - 1.0) <= 1e-12)) {
                snprintf(buf, sizeof buf, "line %d: the strengths of alpha = %d sum to %.17g, not to 1", l, q - 1, sum[q]);
                msg = buf;
                return LSX_EINVAL;
            }
    }
    return LSX_OK;
}

// The table of a call: the components of the lines marked in `wanted` (the lines active in the call's window), kCompDoubles doubles
// each (shift, weight of phi_-1, of phi_0, of phi_+1), and per line (ncomp, first component in the table); a line that is not wanted
// or has no pattern: (0, 0).  -> LSX_OK or LSX_EUNSUPPORTED (the window's patterns over the cap)
inline int pack_patterns(int nlines, const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                         const std::vector<uint8_t>& wanted, std::vector<int32_t>& line, std::vector<double>& tab, std::string& msg)
{
    line.assign(2 * (size_t)(nlines > 0 ? nlines : 1), 0);
    tab.clear();
    size_t o = 0;
    for (int l = 0; l < nlines; ++l) {
        const int nc = ncomp[l];
        if (nc > 0 && wanted[l]) {
            line[2 * l] = nc;
            line[2 * l + 1] = (int32_t)(tab.size() / kCompDoubles);
            for (int k = 0; k < nc; ++k) {
                const int al = alpha[o + k];
                tab.push_back(shift[o + k]);
                tab.push_back(al < 0 ? strength[o + k] : 0.0);
                tab.push_back(al == 0 ? strength[o + k] : 0.0);
                tab.push_back(al > 0 ? strength[o + k] : 0.0);
            }
        }
        o += (size_t)nc;
    }
    if (tab.size() / kCompDoubles > LSX_STOKES_MAX_WINDOW_COMPONENTS) {
        char buf[200];
        snprintf(buf, sizeof buf, "the lines active in the window have %zu Zeeman components together; at most %d are supported: "
                                  "narrow the window", tab.size() / kCompDoubles, LSX_STOKES_MAX_WINDOW_COMPONENTS);
        msg = buf;
        return LSX_EUNSUPPORTED;
    }
    return LSX_OK;
}

// ---- the velocity of a call (include/lsx_hip_stokes_velocity.h) ----
// vlos: [count].  -> LSX_OK or LSX_EINVAL with a message.  Any finite velocity is taken: there is no bound
inline int check_velocity(size_t count, const double* vlos, std::string& msg)
{
    char buf[120];
    for (size_t i = 0; i < count; ++i)
        if (!std::isfinite(vlos[i])) {
            snprintf(buf, sizeof buf, "vlos at point %zu is not finite (%g)", i, vlos[i]);
            msg = buf;
            return LSX_EINVAL;
        }
    return LSX_OK;
}

// ---- the rules lsx_hip_response_stokes adds (include/lsx_hip_stokes_response.h) ----
constexpr int kMaxResponseParams = 4;      // B, gammaB, chiB and, in a call with a velocity, vlos
// the requested parameters in the order B, gammaB, chiB, vlos -> par[npar] (0, 1, 2, 3); returns npar
inline int response_params(uint32_t params, int par[kMaxResponseParams])
{
    int n = 0;
    for (int b = 0; b < kMaxResponseParams; ++b)
        if (params & (1u << b)) par[n++] = b;
    return n;
}

// params, amplitude[nmax], the depths (ks null: all Ns, nk is not looked at) and, where B is requested, B >= a_B / 2 at every requested
// depth of the ncol columns of B [ncol][Ns] (col0: the first one's number, for the message).  nmax: 3, or 4 in a call with a velocity
// (bit 8, vlos, is known only there; vlos has no rule like B's).  -> LSX_OK or LSX_EINVAL with a message
inline int check_response(uint32_t params, const double* amplitude, int Ns, int32_t nk, const int32_t* ks, size_t ncol, int col0,
                          const double* B, std::string& msg, int nmax = 3)
{
    static const char* const name[kMaxResponseParams] = {"B", "gammaB", "chiB", "vlos"};
    char buf[200];
    if (params == 0 || (params & ~((1u << nmax) - 1u))) {
        snprintf(buf, sizeof buf, "params = 0x%x: need at least one of the bits B (1), gammaB (2), chiB (4)%s and no other", (unsigned)params,
                 nmax > 3 ? ", vlos (8)" : "");
        msg = buf;
        return LSX_EINVAL;
    }
    if (!amplitude) { msg = "null amplitude"; return LSX_EINVAL; }
    for (int b = 0; b < nmax; ++b)
        if ((params & (1u << b)) && !(std::isfinite(amplitude[b]) && amplitude[b] > 0.0)) {
            snprintf(buf, sizeof buf, "the amplitude of %s is %g: it must be finite and positive", name[b], amplitude[b]);
            msg = buf;
            return LSX_EINVAL;
        }
    if (ks) {
        if (nk < 1) { snprintf(buf, sizeof buf, "nk = %d, need at least one depth", (int)nk); msg = buf; return LSX_EINVAL; }
        for (int i = 0; i < nk; ++i)
            if (ks[i] < 0 || ks[i] >= Ns || (i && ks[i] <= ks[i - 1])) {
                snprintf(buf, sizeof buf, "ks[%d] = %d: the depths must increase strictly inside [0, %d)", i, (int)ks[i], Ns);
                msg = buf;
                return LSX_EINVAL;
            }
    }
    if (params & 1u) {
        const int n = ks ? nk : Ns;
        for (size_t c = 0; c < ncol; ++c)
            for (int i = 0; i < n; ++i) {
                const int k = ks ? ks[i] : i;
                if (B[c * Ns + k] < 0.5 * amplitude[0]) {
                    snprintf(buf, sizeof buf, "column %d, depth %d: B = %g is below half the amplitude %g: the changed field would be "
                                              "negative (leave field-free depths out with ks)", col0 + (int)c, k, B[c * Ns + k], amplitude[0]);
                    msg = buf;
                    return LSX_EINVAL;
                }
            }
    }
    return LSX_OK;
}

} // namespace lsxst
