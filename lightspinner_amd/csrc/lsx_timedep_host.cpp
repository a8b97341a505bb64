// lsx_timedep_host.cpp -- the formulas of lsx_timedep_dev.h compiled for the CPU: a test-only library (liblsx_td_host.so,
// `make tdhost`) that runs one atom's systems as the kernels of lsx_timedep.hip do, so that a deviation from the exact solve can be
// traced without a GPU, and so that the formulas run under -fsanitize=address,undefined (lsx_timedep_san_main.cpp).
#include <vector>

#include "lsx_timedep_dev.h"

using namespace lsxtd;

template <int NL>
static bool reg(const double* G, const double* np, double* nk, size_t s, double dt, double* ch) { return solve_reg<NL>(G, np, nk, s, dt, ch); }

extern "C" {

// One atom of Nl levels in ncol columns of Ns depths: Gamma [ncol][Nl * Nl][Ns], n_prev and n [ncol][Nl][Ns], dt [ncol];
// active [ncol] or NULL.  in_memory != 0: the form the LDS kernel runs, for every size (the option se_lds); otherwise the
// register form up to 8 levels.  work_stride: the distance of a point's work entries (64 on the device).
// -> n overwritten, dPcol [ncol] (the maximum over depths, NaN dropped), singular [ncol][Ns] (1: flagged, populations kept).
// Returns 0, or 1 for an argument the kernels' launcher refuses.
int lsx_timedep_host(int32_t Nl, int32_t Ns, int32_t ncol, const double* Gamma, const double* n_prev, const double* dt, double* n,
                     double* dPcol, uint8_t* singular, const uint8_t* active, int32_t in_memory, int32_t work_stride)
{
    if (Nl < 2 || Nl > 16 || Ns < 1 || ncol < 1 || work_stride < 1 || !Gamma || !n_prev || !dt || !n || !dPcol || !singular) return 1;
    for (int c = 0; c < ncol; ++c)
        if ((!active || active[c]) && !(dt[c] > 0.0 && std::isfinite(dt[c]))) return 1;
    std::vector<double> work(work_doubles(Nl) * (size_t)work_stride);
    for (size_t c = 0; c < (size_t)ncol; ++c) {
        dPcol[c] = 0.0;
        for (int k = 0; k < Ns; ++k) {
            singular[c * Ns + k] = 0;
            if (active && !active[c]) continue;
            const double* G = Gamma + c * Nl * Nl * Ns + k;
            const double* np = n_prev + c * Nl * Ns + k;
            double* nk = n + c * Nl * Ns + k;
            double ch = 0.0;
            bool ok;
            switch (in_memory ? 0 : Nl) {
            case 2: ok = reg<2>(G, np, nk, Ns, dt[c], &ch); break;
            case 3: ok = reg<3>(G, np, nk, Ns, dt[c], &ch); break;
            case 4: ok = reg<4>(G, np, nk, Ns, dt[c], &ch); break;
            case 5: ok = reg<5>(G, np, nk, Ns, dt[c], &ch); break;
            case 6: ok = reg<6>(G, np, nk, Ns, dt[c], &ch); break;
            case 7: ok = reg<7>(G, np, nk, Ns, dt[c], &ch); break;
            case 8: ok = reg<8>(G, np, nk, Ns, dt[c], &ch); break;
            default: ok = solve_mem(Nl, work.data() + (work_stride - 1), (size_t)work_stride, G, np, nk, Ns, dt[c], &ch);
            }
            if (!ok) singular[c * Ns + k] = 1;
            else if (ch == ch && ch > dPcol[c]) dPcol[c] = ch;
        }
    }
    return 0;
}

} // extern "C"
