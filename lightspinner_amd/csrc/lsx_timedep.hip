// lsx_timedep.hip -- time-dependent populations: one implicit step of the rate equation dn/dt = Gamma n per column, atom and
// depth, on the device (include/lsx_hip_timedep.h: the scheme and the entries).  Unused unless lsx_hip_time_dep_start is called;
// gfx950 only.
//
// The kernels are the statistical equilibrium's (lsx_hip.hip: k_stat_equil, k_stat_equil_reg) with another system in front of the
// one elimination both call (lsx_solve_dev.h, which the CPU tests compile for the host): one thread per (column, depth) of one
// atom, the system in registers for 2 ... 8 levels and in thread-private LDS columns above (or for every size under the option
// se_lds).  A thread reads and writes its own point only: a column's bits depend neither on the context's column count nor on
// the column's index.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_solve_dev.h"
#include "lsx_solve_flag.h"

using namespace lsxd;

namespace {

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
    const bool ok = lsxsolve::solve_reg<NL>(lsxsolve::TimeStep{p.dt[col], p.n_prev + o, p.Ns},
                                            p.Gamma + ((size_t)col * p.NL2tot + p.lev2_off) * p.Ns + k, p.n + o, p.Ns, &ch);
    record_solve(ok, ch, p.singular, p.dPcol, col, p.atom, k, p.Ns);
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
    const bool ok = lsxsolve::solve_mem(lsxsolve::TimeStep{p.dt[col], p.n_prev + o, p.Ns}, Nl, sm + tid, nt,
                                        p.Gamma + ((size_t)col * p.NL2tot + p.lev2_off) * p.Ns + k, p.n + o, p.Ns, &ch);
    record_solve(ok, ch, p.singular, p.dPcol, col, p.atom, k, p.Ns);
}

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
    // nothing is touched or launched unless every active column has a step
    for (int q = 0; q < c->ncol; ++q)
        if ((c->colmask_host.empty() || c->colmask_host[q]) && !(q < (int)c->td_dt.size() && c->td_dt[q] > 0.0))
            return fail(LSX_EINVAL, "lsx_hip_time_dep_update: no step has been started for column %d (lsx_hip_time_dep_start)", q);
    return enqueue_solves(c, "time_dep_update", [](lsx_ctx* c, int a, dim3 grid, dim3 block, size_t lds) {
        TdParams p;
        p.Gamma = c->d_Gamma; p.n_prev = c->d_td_n_prev; p.dt = c->d_td_dt; p.n = c->d_n; p.dPcol = c->d_dPcol;
        p.singular = c->d_singular; p.colmask = c->d_colmask; p.NLtot = c->NLtot; p.NL2tot = c->NL2tot; p.Ns = c->Nspace; p.ncol = c->ncol;
        p.lev_off = c->lev_off[a]; p.lev2_off = c->lev2_off[a]; p.atom = a;
        if (lds) hipLaunchKernelGGL(k_time_dep, grid, block, lds, c->stream, p, c->Nlevel[a]);
        else lsxsolve::with_register_form(c->Nlevel[a], [&](auto nl) { hipLaunchKernelGGL((k_time_dep_reg<decltype(nl)::value>), grid, block, 0, c->stream, p); });
    });
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
