// lsx_timedep.hip -- time-dependent populations: one implicit step of the rate equation dn/dt = Gamma n per column, atom and
// depth, on the device (include/lsx_hip_timedep.h: the scheme and the entries).  Unused unless lsx_hip_time_dep_start is called;
// gfx950 only.
//
// The kernels are the statistical equilibrium's (lsx_hip.hip: k_stat_equil, k_stat_equil_reg) with another system assembled in
// front of the same elimination: one thread per (column, depth) of one atom, the system in registers for 2 ... 8 levels and in
// thread-private LDS columns above (or for every size under the option se_lds).  The formulas live in lsx_timedep_dev.h, which
// the CPU tests compile for the host.  A thread reads and writes its own point only: a column's bits depend neither on the
// context's column count nor on the column's index.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_timedep_dev.h"

using namespace lsxd;

namespace {

// the singular flag and the per-column monitor: the protocol of the statistical equilibrium (lsx_hip.hip: flag_singular,
// atomic_max_nonneg), which lsx_sync / lsx_last_error decode -- keep the two in step
constexpr unsigned long long kSingBase = 1ull << 48;
__device__ __forceinline__ void td_flag_singular(unsigned long long* flag, int col, int atom, int k, int Ns)
{
    atomicMax(flag, kSingBase - ((((unsigned long long)col << 8) | (unsigned)atom) * (unsigned long long)Ns + (unsigned)k));
}

__device__ __forceinline__ void td_atomic_max_nonneg(double* addr, double v)
{
    // for non-negative doubles the IEEE bit pattern orders like the value
    atomicMax(reinterpret_cast<unsigned long long*>(addr), static_cast<unsigned long long>(__double_as_longlong(fabs(v))));
}

struct TdParams {
    const double* Gamma;            // [col][NL2tot][k]
    const double* n_prev;           // [col][NLtot][k]
    const double* dt;               // [col]
    double* n;                      // [col][NLtot][k]
    double* dPcol;                  // [col]
    unsigned long long* singular;
    const uint8_t* colmask;         // nullptr: every column is active
    int lev_off, lev2_off, atom, NLtot, NL2tot, Ns, ncol;
};

template <int NL>
__global__ void __launch_bounds__(64)
k_time_dep_reg(const TdParams p)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)p.ncol * p.Ns) return;
    const int col = gid / p.Ns, k = gid % p.Ns;
    if (p.colmask && !p.colmask[col]) return;
    const size_t o = ((size_t)col * p.NLtot + p.lev_off) * p.Ns + k;
    double ch;
    if (!lsxtd::solve_reg<NL>(p.Gamma + ((size_t)col * p.NL2tot + p.lev2_off) * p.Ns + k, p.n_prev + o, p.n + o, (size_t)p.Ns,
                              p.dt[col], &ch)) {
        td_flag_singular(p.singular, col, p.atom, k, p.Ns);
        return;
    }
    // the maximum over depths drops a NaN, as the statistical equilibrium's does (rh_method.py:741)
    if (ch == ch) td_atomic_max_nonneg(&p.dPcol[col], ch);
}

__global__ void __launch_bounds__(64)
k_time_dep(const TdParams p, int Nl)
{
    extern __shared__ double sm[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const long gid = (long)blockIdx.x * nt + tid;
    if (gid >= (long)p.ncol * p.Ns) return;
    const int col = gid / p.Ns, k = gid % p.Ns;
    if (p.colmask && !p.colmask[col]) return;
    const size_t o = ((size_t)col * p.NLtot + p.lev_off) * p.Ns + k;
    double ch;
    if (!lsxtd::solve_mem(Nl, sm + tid, (size_t)nt, p.Gamma + ((size_t)col * p.NL2tot + p.lev2_off) * p.Ns + k, p.n_prev + o,
                          p.n + o, (size_t)p.Ns, p.dt[col], &ch)) {
        td_flag_singular(p.singular, col, p.atom, k, p.Ns);
        return;
    }
    if (ch == ch) td_atomic_max_nonneg(&p.dPcol[col], ch);
}

size_t lds_bytes(int Nl) { return lsxtd::work_doubles(Nl) * 64 * sizeof(double); }

int ensure_state(lsx_ctx* c)
{
    if (c->d_td_dt) return LSX_OK;
    const size_t nc = (size_t)c->ncol;
    int rc;
    if ((rc = dmalloc(&c->d_td_n_prev, nc * c->NLtot * c->Nspace)) || (rc = dmalloc(&c->d_td_dt, nc))) {
        td_free(c);
        return rc;
    }
    HIPCHK(hipMemsetAsync(c->d_td_dt, 0, nc * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(c->d_td_n_prev, 0, nc * c->NLtot * c->Nspace * sizeof(double), c->stream));
    c->td_dt.assign(nc, 0.0);
    return LSX_OK;
}

bool bad_range(const lsx_ctx* c, int32_t col0, int32_t ncol) { return col0 < 0 || ncol < 1 || (long)col0 + ncol > c->ncol; }

} // namespace

namespace lsxd {

void td_free(lsx_ctx* c)
{
    if (c->d_td_n_prev) (void)hipFree(c->d_td_n_prev);
    if (c->d_td_dt) (void)hipFree(c->d_td_dt);
    c->d_td_n_prev = c->d_td_dt = nullptr;
    c->td_dt.clear();
}

} // namespace lsxd

extern "C" int lsx_hip_time_dep_start(lsx_ctx* c, int32_t col0, int32_t ncol, const double* dt, const double* n_prev)
{
    if (!c) return fail(LSX_EINVAL, "lsx_hip_time_dep_start: null context");
    if (bad_range(c, col0, ncol))
        return fail(LSX_EINVAL, "lsx_hip_time_dep_start: columns [%d, %d) are outside the context's %d", (int)col0, (int)col0 + (int)ncol, c->ncol);
    if (!dt) return fail(LSX_EINVAL, "lsx_hip_time_dep_start: null dt");
    for (int32_t q = 0; q < ncol; ++q)
        if (!(dt[q] > 0.0) || !std::isfinite(dt[q]))
            return fail(LSX_EINVAL, "lsx_hip_time_dep_start: dt = %g of column %d is not a positive finite time step", dt[q], (int)(col0 + q));
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_state(c);
    if (rc) return rc;
    const size_t per = (size_t)c->NLtot * c->Nspace;
    if (n_prev)
        HIPCHK(hipMemcpyAsync(c->d_td_n_prev + (size_t)col0 * per, n_prev, (size_t)ncol * per * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else        // the populations as they are on the device, behind everything enqueued: no host copy
        HIPCHK(hipMemcpyAsync(c->d_td_n_prev + (size_t)col0 * per, c->d_n + (size_t)col0 * per, (size_t)ncol * per * sizeof(double),
                              hipMemcpyDeviceToDevice, c->stream));
    memcpy(c->td_dt.data() + col0, dt, (size_t)ncol * sizeof(double));
    HIPCHK(hipMemcpyAsync(c->d_td_dt + col0, c->td_dt.data() + col0, (size_t)ncol * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // a new step: what the Ng history holds of these columns belongs to the last one
    if (c->ng_order && (rc = ng_reset(c, (size_t)col0, (size_t)ncol))) return rc;
    if (n_prev) HIPCHK(hipStreamSynchronize(c->stream));        // (the caller's array is pageable host memory)
    return LSX_OK;
}

extern "C" int lsx_hip_time_dep_update_async(lsx_ctx* c)
{
    if (!c) return fail(LSX_EINVAL, "lsx_hip_time_dep_update_async: null context");
    // nothing is touched or launched unless every active column has a step and every atom's system can be solved
    for (int q = 0; q < c->ncol; ++q)
        if ((c->colmask_host.empty() || c->colmask_host[q]) && !(q < (int)c->td_dt.size() && c->td_dt[q] > 0.0))
            return fail(LSX_EINVAL, "lsx_hip_time_dep_update: no step has been started for column %d (lsx_hip_time_dep_start)", q);
    for (int a = 0; a < c->Natoms; ++a)
        if ((c->opt_se_lds || c->Nlevel[a] > 8) && lds_bytes(c->Nlevel[a]) > 160 * 1024)
            return fail(LSX_EUNSUPPORTED, "time_dep_update: Nlevel = %d needs %zu B of LDS", c->Nlevel[a], lds_bytes(c->Nlevel[a]));
    c->spec_valid = false;            // the populations now build on the last formal solution
    c->optab_fresh = false;           // the populations change
    HIPCHK(hipSetDevice(c->device));
    // dPcol and the singular flag behind it start at zero: the Gamma epilogue of the formal solution has done that, unless this
    // is a second update on the same Gamma
    if (!c->dp_zeroed) HIPCHK(hipMemsetAsync(c->d_dPcol, 0, ((size_t)c->ncol + 1) * 8, c->stream));
    c->dp_zeroed = false;
    const long nthreads = (long)c->ncol * c->Nspace;
    const int nt = 64;
    const dim3 grid((unsigned)((nthreads + nt - 1) / nt));
    TdParams p;
    p.Gamma = c->d_Gamma; p.n_prev = c->d_td_n_prev; p.dt = c->d_td_dt; p.n = c->d_n; p.dPcol = c->d_dPcol;
    p.singular = c->d_singular; p.colmask = c->d_colmask; p.NLtot = c->NLtot; p.NL2tot = c->NL2tot; p.Ns = c->Nspace; p.ncol = c->ncol;
    for (int a = 0; a < c->Natoms; ++a) {
        const int Nl = c->Nlevel[a];
        p.lev_off = c->lev_off[a]; p.lev2_off = c->lev2_off[a]; p.atom = a;
#define TD_REG(NLC) case NLC: hipLaunchKernelGGL((k_time_dep_reg<NLC>), grid, dim3(nt), 0, c->stream, p); break;
        switch (c->opt_se_lds ? 0 : Nl) {
        TD_REG(2) TD_REG(3) TD_REG(4) TD_REG(5) TD_REG(6) TD_REG(7) TD_REG(8)
        default: hipLaunchKernelGGL(k_time_dep, grid, dim3(nt), lds_bytes(Nl), c->stream, p, Nl);
        }
#undef TD_REG
        HIPCHK(hipGetLastError());
    }
    // Ng acceleration, where configured (lsx_ng.hip): one launch behind the solves, ahead of any read-back of this call's results
    if (c->ng_order) {
        const int rc = ng_enqueue(c);
        if (rc) return rc;
    }
    c->se_pending = true;
    return LSX_OK;
}

extern "C" int lsx_hip_time_dep_update(lsx_ctx* c, double* dPops_max)
{
    const int rc = lsx_hip_time_dep_update_async(c);
    if (rc) return rc;
    return lsx_sync(c, nullptr, dPops_max);
}

extern "C" int lsx_hip_time_dep_state(lsx_ctx* c, int32_t col0, int32_t ncol, double* dt, double* n_prev)
{
    if (!c) return fail(LSX_EINVAL, "lsx_hip_time_dep_state: null context");
    if (bad_range(c, col0, ncol))
        return fail(LSX_EINVAL, "lsx_hip_time_dep_state: columns [%d, %d) are outside the context's %d", (int)col0, (int)col0 + (int)ncol, c->ncol);
    const size_t per = (size_t)c->NLtot * c->Nspace;
    if (!c->d_td_dt) {              // no step has ever been started: nothing is allocated for the answer
        if (dt) memset(dt, 0, (size_t)ncol * sizeof(double));
        if (n_prev) memset(n_prev, 0, (size_t)ncol * per * sizeof(double));
        return LSX_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    if (dt) HIPCHK(hipMemcpyAsync(dt, c->d_td_dt + col0, (size_t)ncol * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n_prev)
        HIPCHK(hipMemcpyAsync(n_prev, c->d_td_n_prev + (size_t)col0 * per, (size_t)ncol * per * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LSX_OK;
}
