// lsx_eqpops_prep.h -- host side of lsx_hip_eq_pops: the checks of its arguments and the flat level tables, shared by
// lsx_eqpops.hip and the CPU build of the formulas (lsx_eqpops_host.cpp).
#pragma once
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lsx_hip_eqpops.h"
#include "lsx_eqpops_dev.h"

namespace lsxeq {

struct HostTables {
    std::vector<Atom> atoms;
    std::vector<double> E, g, nDebye;
    std::vector<int32_t> dZ;
    int NLtot = 0;
};

// "" if the arguments of a call are usable (then H holds the tables), else what is wrong with them (LSX_EINVAL)
inline std::string prepare(int natoms, const lsx_eq_atom* atoms, long ncol, int Ns, const double* T, const double* ne, const double* nH,
                           const double* nStar, HostTables* H)
{
    char b[200];
    if (natoms < 1 || !atoms) return "natoms < 1 or null atoms";
    if (ncol < 1) return "ncol < 1";
    if (Ns < 1) return "Nspace < 1";
    if (!T || !ne || !nH || !nStar) return "a null input array or null nStar";
    *H = HostTables();
    for (int a = 0; a < natoms; ++a) {
        const lsx_eq_atom& m = atoms[a];
        if (m.Nlevel < 1 || !m.levels) { snprintf(b, sizeof b, "atom %d: Nlevel < 1 or null levels", a); return b; }
        if (!std::isfinite(m.abundance) || m.abundance < 0.0) { snprintf(b, sizeof b, "atom %d: abundance is negative or not finite", a); return b; }
        Atom A{};
        A.Nl = m.Nlevel; A.lev_off = H->NLtot; A.abundance = m.abundance;
        for (int i = 0; i < m.Nlevel; ++i) {
            const lsx_level& l = m.levels[i];
            if (!std::isfinite(l.g) || !(l.g > 0.0)) { snprintf(b, sizeof b, "atom %d level %d: g is not finite and positive", a, i); return b; }
            if (!std::isfinite(l.E_SI)) { snprintf(b, sizeof b, "atom %d level %d: E_SI is not finite", a, i); return b; }
            if (l.stage < m.levels[0].stage) { snprintf(b, sizeof b, "atom %d level %d: stage %d lies below level 0's %d", a, i, l.stage, m.levels[0].stage); return b; }
            H->E.push_back(l.E_SI);
            H->g.push_back(l.g);
            H->dZ.push_back(l.stage - m.levels[0].stage);
            H->nDebye.push_back(n_debye(i, l.stage, m.levels[0].stage));
        }
        H->NLtot += m.Nlevel;
        H->atoms.push_back(A);
    }
    const size_t npts = (size_t)ncol * Ns;
    for (size_t i = 0; i < npts; ++i) {
        const char* what = nullptr;
        if (!std::isfinite(T[i]) || !(T[i] > 0.0)) what = "temperature is not finite and positive";
        else if (!std::isfinite(ne[i]) || !(ne[i] > 0.0)) what = "ne is not finite and positive";
        else if (!std::isfinite(nH[i]) || nH[i] < 0.0) what = "nHTot is negative or not finite";
        if (what) { snprintf(b, sizeof b, "column %zu, depth %zu: %s", i / Ns, i % Ns, what); return b; }
    }
    return "";
}

} // namespace lsxeq
