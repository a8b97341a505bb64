// lsx_timedep_host.cpp -- the solve of lsx_solve_dev.h compiled for the CPU: a test-only library (liblsx_td_host.so, `make tdhost`)
// that runs one atom's systems as the kernels of lsx_timedep.hip (lsx_timedep_host) and the statistical equilibrium's of
// lsx_hip.hip (lsx_statequil_host) do, so that a deviation from the exact solve can be traced without a GPU, and so that the
// solve runs under -fsanitize=address,undefined (lsx_timedep_san_main.cpp).
#include <vector>

#include "lsx_solve_dev.h"

using namespace lsxsolve;

// The walk over the points of one atom of Nl levels in ncol columns of Ns depths that both entries make: Gamma [ncol][Nl * Nl][Ns],
// n [ncol][Nl][Ns]; active [ncol] or NULL.  in_memory != 0: the form the LDS kernel runs, for every size (the option se_lds);
// otherwise the register form up to 8 levels.  work_stride: the distance of a point's work entries (64 on the device).
// system(c, k): the System of column c, depth k.
// -> n overwritten, dPcol [ncol] (the maximum over depths, NaN dropped), singular [ncol][Ns] (1: flagged, populations kept).
template <class SystemAt>
static void solve_points(int Nl, int Ns, int ncol, const double* Gamma, double* n, double* dPcol, uint8_t* singular, const uint8_t* active,
                         int in_memory, int work_stride, SystemAt system)
{
    std::vector<double> work(work_doubles(Nl) * (size_t)work_stride);
    for (size_t c = 0; c < (size_t)ncol; ++c) {
        dPcol[c] = 0.0;
        for (int k = 0; k < Ns; ++k) {
            singular[c * Ns + k] = 0;
            if (active && !active[c]) continue;
            const double* G = Gamma + c * Nl * Nl * Ns + k;
            double* nk = n + c * Nl * Ns + k;
            const auto sys = system(c, k);
            double ch = 0.0;
            bool ok = false;
            if (!in_memory && has_register_form(Nl))
                with_register_form(Nl, [&](auto nl) { ok = solve_reg<decltype(nl)::value>(sys, G, nk, Ns, &ch); });
            else
                ok = solve_mem(sys, Nl, work.data() + (work_stride - 1), work_stride, G, nk, Ns, &ch);
            if (!ok) singular[c * Ns + k] = 1;
            else if (ch == ch && ch > dPcol[c]) dPcol[c] = ch;
        }
    }
}

static bool bad_shape(int32_t Nl, int32_t Ns, int32_t ncol, int32_t work_stride) { return Nl < 2 || Nl > 16 || Ns < 1 || ncol < 1 || work_stride < 1; }

extern "C" {

// The implicit step: n_prev like n, dt [ncol].  Returns 0, or 1 for an argument the kernels' launcher refuses.
int lsx_timedep_host(int32_t Nl, int32_t Ns, int32_t ncol, const double* Gamma, const double* n_prev, const double* dt, double* n,
                     double* dPcol, uint8_t* singular, const uint8_t* active, int32_t in_memory, int32_t work_stride)
{
    if (bad_shape(Nl, Ns, ncol, work_stride) || !Gamma || !n_prev || !dt || !n || !dPcol || !singular) return 1;
    for (int c = 0; c < ncol; ++c)
        if ((!active || active[c]) && !(dt[c] > 0.0 && std::isfinite(dt[c]))) return 1;
    solve_points(Nl, Ns, ncol, Gamma, n, dPcol, singular, active, in_memory, work_stride,
                 [=](size_t c, int k) { return TimeStep{dt[c], n_prev + c * Nl * Ns + k, Ns}; });
    return 0;
}

// The statistical equilibrium: nTotal [ncol][Ns] of the atom.  Returns 0, or 1 for a bad argument.
int lsx_statequil_host(int32_t Nl, int32_t Ns, int32_t ncol, const double* Gamma, const double* nTotal, double* n, double* dPcol,
                       uint8_t* singular, const uint8_t* active, int32_t in_memory, int32_t work_stride)
{
    if (bad_shape(Nl, Ns, ncol, work_stride) || !Gamma || !nTotal || !n || !dPcol || !singular) return 1;
    solve_points(Nl, Ns, ncol, Gamma, n, dPcol, singular, active, in_memory, work_stride,
                 [=](size_t c, int k) { return StatEquil{nTotal + c * Ns + k}; });
    return 0;
}

} // extern "C"
