// lsx_eqpops_host.cpp -- the formulas of lsx_eqpops_dev.h compiled for the CPU: a test-only library (liblsx_eqpops_host.so,
// `make eqpopshost`) with the arguments and the checks of lsx_hip_eq_pops, so that a deviation from the reference can be traced
// without a GPU, and so that the formulas run under -fsanitize=address,undefined (lsx_eqpops_san_main.cpp).
#include "lsx_eqpops_prep.h"

using namespace lsxeq;

static thread_local std::string g_eq_err;

extern "C" {

const char* lsx_eqpops_host_error(void) { return g_eq_err.c_str(); }

// lsx_hip_eq_pops with Nspace handed over instead of a context
int lsx_eqpops_host(int32_t Ns, int32_t natoms, const lsx_eq_atom* atoms, int32_t ncol, const double* temperature, const double* ne,
                    const double* nHTot, double* nStar, double* nTotal)
{
    HostTables H;
    g_eq_err = prepare(natoms, atoms, ncol, Ns, temperature, ne, nHTot, nStar, &H);
    if (!g_eq_err.empty()) return LSX_EINVAL;
    const Levels lev{H.E.data(), H.g.data(), H.dZ.data(), H.nDebye.data()};
    for (size_t col = 0; col < (size_t)ncol; ++col)
        for (int k = 0; k < Ns; ++k) {
            const size_t gid = col * Ns + k;
            const Point P = make_point(temperature[gid], ne[gid]);
            for (int a = 0; a < natoms; ++a) {
                const Atom& A = H.atoms[a];
                const double nTot = A.abundance * nHTot[gid];
                if (nTotal) nTotal[(col * natoms + a) * Ns + k] = nTot;
                lte_point(P, A, lev, nTot, nStar + (col * H.NLtot + A.lev_off) * Ns + k, (size_t)Ns);
            }
        }
    return LSX_OK;
}

} // extern "C"
