// lsx_eqpops_dev.h -- lte_pops(debye=True) of the reference (atomic_set.py:105-145) at one (column, depth) point, restated as a
// __host__ __device__ function that a host compiler also accepts (lsx_eqpops.hip runs it on the device, one thread per point;
// lsx_eqpops_host.cpp on the CPU for the tests).  The expressions are those of k_setup_lte_pops (lsx_setup.hip), one for one and
// in the reference's operation order, so that an atom that is active in a context gets the bits lsx_set_atmosphere gives it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LSXEQ_HD __host__ __device__ inline
#else
#define LSXEQ_HD inline
#endif

namespace lsxeq {

// constants.py:1-27
constexpr double kHPlanck = 6.6260755E-34, kKBoltzmann = 1.380658E-23, kMElectron = 9.1093897E-31, kQElectron = 1.60217733E-19,
                 kEpsilon0 = 8.854187817E-12;

struct Atom {                    // one atom of a call: where its levels start in the level tables and in a column's nStar
    int32_t Nl, lev_off;
    double abundance;
};

struct Levels {                  // [sum of Nlevel], the atoms concatenated
    const double* E;             // E_SI
    const double* g;
    const int32_t* dZ;           // stage - stage of the atom's level 0
    const double* nDebye;        // atomic_set.py:113-119
};

// nDebye of a level (atomic_set.py:113-119): stage + (stage + 1) + ... with dZ terms; 0 for level 0.  Host side.
inline double n_debye(int level, int stage, int stage0)
{
    double nD = 0.0;
    int Z = stage;
    for (int s = 1; level >= 1 && s < stage - stage0 + 1; ++s) { nD += Z; Z += 1; }
    return nD;
}

// what every atom of a point shares (:107-111, :120-121)
struct Point { double T, dEion, cNe_T; };

LSXEQ_HD Point make_point(double T, double ne)
{
    const double c1 = (kHPlanck / (2.0 * M_PI * kMElectron)) * (kHPlanck / kKBoltzmann);
    const double c2 = sqrt(8.0 * M_PI / kKBoltzmann) * pow(kQElectron * kQElectron / (4.0 * M_PI * kEpsilon0), 1.5);
    Point P;
    P.T = T;
    P.dEion = c2 * sqrt(ne / T);
    P.cNe_T = 0.5 * ne * pow(c1 / T, 1.5);
    return P;
}

// one atom at one point: ns[i * stride], i < Nl (:122-143).  nTotal: the atom's total population there.
LSXEQ_HD void lte_point(const Point& P, const Atom& A, const Levels& L, double nTotal, double* ns, size_t stride)
{
    double total = 1.0;
    for (int i = 1; i < A.Nl; ++i) {
        const int gi = A.lev_off + i;
        const double dE = L.E[gi] - L.E[A.lev_off];
        const double gi0 = L.g[gi] / L.g[A.lev_off];
        const int dZ = L.dZ[gi];
        const double dE_kT = (dE - L.nDebye[gi] * P.dEion) / (kKBoltzmann * P.T);
        double nst = gi0 * exp(-dE_kT);
        // cNe_T ** dZ with an integer exponent (numpy: 0 -> 1, 1 -> x, 2 -> x x, else pow)
        const double den = dZ == 0 ? 1.0 : (dZ == 1 ? P.cNe_T : (dZ == 2 ? P.cNe_T * P.cNe_T : pow(P.cNe_T, (double)dZ)));
        nst /= den;
        ns[(size_t)i * stride] = nst;
        total += nst;
    }
    const double n0 = nTotal / total;
    ns[0] = n0;
    for (int i = 1; i < A.Nl; ++i) ns[(size_t)i * stride] *= n0;
}

} // namespace lsxeq
