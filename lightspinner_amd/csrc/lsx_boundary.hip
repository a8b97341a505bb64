// lsx_boundary.hip -- radiation boundary conditions as context state (include/lsx_hip_boundary.h): the two entries; the kernels that
// read the state are the sweeps (lsx_sweep.hip, lsx_sweep_rs.hip) and the final passes.  Host code only; gfx950 only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_boundary_prep.h"
#include "lsx_ctx.h"

using namespace lsxd;

void lsxd::boundary_free(lsx_ctx* c)
{
    if (c->d_bnd) (void)hipFree(c->d_bnd);
    c->d_bnd = nullptr;
    c->bnd_values = false;
    c->bnd_kind.clear();
}

extern "C" int lsx_hip_set_boundary(lsx_ctx* c, int32_t col0, int32_t ncol, int32_t lower, int32_t upper, const double* I_lower,
                                    const double* I_upper)
{
    // ---- everything is checked on the host before anything changes ----
    if (!c) return fail(LSX_EINVAL, "lsx_hip_set_boundary: null context");
    if (const char* why = lsxbnd::check_args(c->ncol, col0, ncol, lower, upper, I_lower, I_upper))
        return fail(LSX_EINVAL, "lsx_hip_set_boundary: %s (columns [%d, %d) of %d, kinds %d / %d)", why, (int)col0, (int)col0 + (int)ncol,
                    c->ncol, (int)lower, (int)upper);
    HIPCHK(hipSetDevice(c->device));
    // the store is what a kernel argument points at: nothing enqueued may still read it, and a captured formal solution holds the
    // pointer of the moment it was captured (null before the first call): dropped, the next call captures anew
    HIPCHK(hipStreamSynchronize(c->stream));
    for (auto& g : c->fs_graphs) if (g.second) (void)hipGraphExecDestroy(g.second);
    c->fs_graphs.clear();
    c->fs_graph_epi.clear();

    // the store (lsx_dev.h): header, kinds, and -- from the first GIVEN on -- the start values.  It is allocated without the values and
    // re-allocated with them (zeroed; there were none to keep) when the first column asks for them
    const size_t nc = (size_t)c->ncol, per = (size_t)c->Nspect * c->Nrays;
    const bool want_values = c->bnd_values || lower == LSX_BOUNDARY_GIVEN || upper == LSX_BOUNDARY_GIVEN;
    if (!c->d_bnd || want_values != c->bnd_values) {
        char* fresh = nullptr;
        const size_t bytes = boundary_store_bytes(nc, per, want_values);
        int rc = dmalloc(&fresh, bytes);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(fresh, 0, bytes, c->stream));
        if (c->d_bnd) (void)hipFree(c->d_bnd);
        c->d_bnd = reinterpret_cast<int32_t*>(fresh);
        c->bnd_values = want_values;
    }
    if (c->bnd_kind.empty()) {
        c->bnd_kind.resize(2 * nc);
        lsxbnd::default_kinds(c->bnd_kind.data(), nc);
    }
    lsxbnd::set_kinds(c->bnd_kind.data(), (size_t)col0, (size_t)ncol, lower, upper);
    std::vector<int32_t> head(LSX_BND_HEADER + 2 * nc, 0);
    head[0] = (int32_t)nc;
    head[1] = c->bnd_values ? 1 : 0;
    std::copy(c->bnd_kind.begin(), c->bnd_kind.end(), head.begin() + LSX_BND_HEADER);
    HIPCHK(hipMemcpyAsync(c->d_bnd, head.data(), head.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    double* values = reinterpret_cast<double*>(c->d_bnd + LSX_BND_HEADER + 2 * nc);
    if (lower == LSX_BOUNDARY_GIVEN)
        HIPCHK(hipMemcpyAsync(values + lsxbnd::store_offset(LSX_BND_LOWER, nc, (size_t)col0, per), I_lower, (size_t)ncol * per * sizeof(double),
                              hipMemcpyHostToDevice, c->stream));
    if (upper == LSX_BOUNDARY_GIVEN)
        HIPCHK(hipMemcpyAsync(values + lsxbnd::store_offset(LSX_BND_UPPER, nc, (size_t)col0, per), I_upper, (size_t)ncol * per * sizeof(double),
                              hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));       // the caller's arrays and `head` may go out of scope
    return LSX_OK;
}

extern "C" int lsx_hip_boundary_state(lsx_ctx* c, int32_t col0, int32_t ncol, int32_t* kinds)
{
    if (!c || !kinds) return fail(LSX_EINVAL, "lsx_hip_boundary_state: null argument");
    if (col0 < 0 || ncol < 1 || (int64_t)col0 + ncol > c->ncol)
        return fail(LSX_EINVAL, "lsx_hip_boundary_state: columns [%d, %d) are outside the context's %d", (int)col0, (int)col0 + (int)ncol, c->ncol);
    if (c->bnd_kind.empty()) lsxbnd::default_kinds(kinds, (size_t)ncol);
    else
        for (size_t q = 0; q < 2 * (size_t)ncol; ++q) kinds[q] = c->bnd_kind[2 * (size_t)col0 + q];
    return LSX_OK;
}
