// lsx_eqpops.hip -- LTE populations of any atoms on the device (include/lsx_hip_eqpops.h): the reference's
// RadiativeSet.compute_eq_pops (atomic_set.py:361-375) over lte_pops(debye=True) (:105-145).  gfx950.
//   k_eq_pops   one thread per (column, depth): the point's dEion and cNe_T once, then atom after atom, level after level, straight
//               to nStar [col][level][k] (consecutive lanes, consecutive depths); no LDS, no private array
// The formulas are lsx_eqpops_dev.h, the expressions of k_setup_lte_pops (lsx_setup.hip) one for one; this unit is built with the
// flags of lsx_setup.hip, so that an atom active in a context gets the bits lsx_set_atmosphere(lte_pops = 1) gives it.
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_eqpops_prep.h"

using namespace lsxd;

namespace {

struct EqParams {
    int Ns, Natoms, NLtot;
    long npts;
    const lsxeq::Atom* atoms;
    lsxeq::Levels lev;
    const double* T;            // [ncol][Ns]
    const double* ne;
    const double* nH;
    double* nStar;              // [ncol][NLtot][Ns]
    double* nTotal;             // [ncol][Natoms][Ns], or null
};

__global__ __launch_bounds__(128) void k_eq_pops(const EqParams q)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= q.npts) return;
    const size_t col = gid / q.Ns;
    const int k = gid % q.Ns;
    const lsxeq::Point P = lsxeq::make_point(q.T[gid], q.ne[gid]);
    const double nH = q.nH[gid];
    for (int a = 0; a < q.Natoms; ++a) {
        const lsxeq::Atom A = q.atoms[a];
        const double nTot = A.abundance * nH;                                       // atomic_set.py:368
        if (q.nTotal) q.nTotal[(col * q.Natoms + a) * q.Ns + k] = nTot;
        lsxeq::lte_point(P, A, q.lev, nTot, q.nStar + (col * q.NLtot + A.lev_off) * q.Ns + k, (size_t)q.Ns);
    }
}

struct Bufs {        // device memory of one call, freed when the call returns
    std::vector<void*> ptrs;
    ~Bufs() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T>
    int get(T** p, size_t count)
    {
        int rc = dmalloc(p, count);
        if (!rc) ptrs.push_back(*p);
        return rc;
    }
    template <typename T>
    int put(T** p, const T* src, size_t count, hipStream_t st)
    {
        int rc = get(p, count);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(*p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        return LSX_OK;
    }
};

} // namespace

extern "C" int lsx_hip_eq_pops(lsx_ctx* c, int32_t natoms, const lsx_eq_atom* atoms, int32_t ncol, const double* temperature,
                               const double* ne, const double* nHTot, double* nStar, double* nTotal)
{
    static const char* who = "lsx_hip_eq_pops";
    if (!c) return fail(LSX_EINVAL, "%s: null context", who);
    const int Ns = c->Nspace;
    lsxeq::HostTables H;
    {
        const std::string bad = lsxeq::prepare(natoms, atoms, ncol, Ns, temperature, ne, nHTot, nStar, &H);
        if (!bad.empty()) return fail(LSX_EINVAL, "%s: %s", who, bad.c_str());
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t npts = (size_t)ncol * Ns;
    Bufs B;
    int rc;
#define TRY(x) do { rc = (x); if (rc) return rc; } while (0)
    lsxeq::Atom* d_atoms;
    double *d_E, *d_g, *d_nD, *d_T, *d_ne, *d_nH, *d_ns, *d_nt = nullptr;
    int32_t* d_dZ;
    TRY(B.put(&d_atoms, (const lsxeq::Atom*)H.atoms.data(), H.atoms.size(), c->stream));
    TRY(B.put(&d_E, (const double*)H.E.data(), H.E.size(), c->stream));
    TRY(B.put(&d_g, (const double*)H.g.data(), H.g.size(), c->stream));
    TRY(B.put(&d_nD, (const double*)H.nDebye.data(), H.nDebye.size(), c->stream));
    TRY(B.put(&d_dZ, (const int32_t*)H.dZ.data(), H.dZ.size(), c->stream));
    TRY(B.put(&d_T, temperature, npts, c->stream));
    TRY(B.put(&d_ne, ne, npts, c->stream));
    TRY(B.put(&d_nH, nHTot, npts, c->stream));
    TRY(B.get(&d_ns, npts * H.NLtot));
    if (nTotal) TRY(B.get(&d_nt, npts * natoms));
#undef TRY
    EqParams q{};
    q.Ns = Ns; q.Natoms = natoms; q.NLtot = H.NLtot; q.npts = (long)npts;
    q.atoms = d_atoms;
    q.lev.E = d_E; q.lev.g = d_g; q.lev.dZ = d_dZ; q.lev.nDebye = d_nD;
    q.T = d_T; q.ne = d_ne; q.nH = d_nH; q.nStar = d_ns; q.nTotal = d_nt;
    hipLaunchKernelGGL(k_eq_pops, dim3((unsigned)((npts + 127) / 128)), dim3(128), 0, c->stream, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(nStar, d_ns, npts * H.NLtot * 8, hipMemcpyDeviceToHost, c->stream));
    if (nTotal) HIPCHK(hipMemcpyAsync(nTotal, d_nt, npts * natoms * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LSX_OK;
}
