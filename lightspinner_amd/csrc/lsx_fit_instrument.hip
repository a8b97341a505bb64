// lsx_fit_instrument.hip -- the instrument of the field fit (include/lsx_hip_fit_instrument.h): smearing by a
// line-spread function and sampling on the instrument's pixels, one banded matrix over the wavelengths of the window, applied on the
// device to the Stokes vector and to every row of the Jacobian between the passes and the reduction of lsx_fit.hip.  gfx950 only.
// The arithmetic is lsx_fit_dev.h's (lsxfit::smear).
//   k_fit_smear   lane = observed point d' = (s nobs + o) nmu + m of one row, grid y = column, z = row (the P rows of J, then S): one
//                 register accumulator a lane over the `width` grid points of pixel o, i ascending.  For fixed i neighbouring lanes
//                 read x[(s nla + first[o] + i) nmu + m]: consecutive pixels have nearly consecutive first[o], so a wave's loads are
//                 nearly contiguous.  The weights come straight from the cache: the lanes of a pixel read one address (a broadcast),
//                 the whole table is nobs x width doubles that every block of the launch reads; staging a block's rows in LDS would
//                 take up to (64 / nmu + 2) x width doubles a block (68 KB at width 130, one angle) for values that are read once
//                 per lane either way.  No LDS, no scratch, no atomics; one writer per value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_fit_dev.h"
#include "lsx_fit_inst.h"
#include "lsx_plan.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)64 << 20;        // bytes (include/lsx_hip_fit.h)

struct SmearParams {
    int32_t nla, nmu, nobs, width, P, Mo;     // Mo = ns nobs nmu: the observed points of a row
    size_t M;                                 // ns nla nmu: the grid points of a row
    size_t cl0;                               // the column of grid y = 0
    const int32_t* first;                     // [nobs]
    const double* weight;                     // [nobs][width]
    const double *J, *S;
    double *Jo, *So;
};

__global__ void __launch_bounds__(64) k_fit_smear(const SmearParams p)
{
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= p.Mo) return;
    const size_t cl = p.cl0 + blockIdx.y;
    const int z = blockIdx.z;
    const int so = d / p.nmu, m = d - so * p.nmu;     // d' = (s nobs + o) nmu + m
    const int s = so / p.nobs, o = so - s * p.nobs;
    const double* in = z < p.P ? p.J + (cl * p.P + z) * p.M : p.S + cl * p.M;         // (block-uniform)
    double* out = z < p.P ? p.Jo + (cl * p.P + z) * (size_t)p.Mo : p.So + cl * (size_t)p.Mo;
    out[d] = lsxfit::smear(p.weight + (size_t)o * p.width, p.width, in + ((size_t)s * p.nla + p.first[o]) * p.nmu + m, (size_t)p.nmu);
}

} // namespace

namespace lsxd {

int fit_instrument_check(const char* who, const lsx_fit_instrument* inst, int32_t nla, int32_t nmu, int32_t ns)
{
    if (!inst || !inst->first || !inst->weight) return fail(LSX_EINVAL, "%s: null instrument, first or weight", who);
    if (inst->nobs < 1) return fail(LSX_EINVAL, "%s: the instrument has nobs = %d pixels, need at least one", who, (int)inst->nobs);
    if (inst->width < 1 || inst->width > nla)
        return fail(LSX_EINVAL, "%s: the instrument's width = %d is outside [1, nla = %d]", who, (int)inst->width, (int)nla);
    if ((int64_t)ns * inst->nobs * nmu > INT32_MAX / 2)
        return fail(LSX_EUNSUPPORTED, "%s: %d nobs nmu = %lld observed points a row", who, (int)ns, (long long)ns * inst->nobs * nmu);
    for (int o = 0; o < inst->nobs; ++o)
        if (inst->first[o] < 0 || inst->first[o] > nla - inst->width)
            return fail(LSX_EINVAL, "%s: first[%d] = %d of the instrument: pixel %d reads outside [0, nla - width = %d]", who, o,
                        (int)inst->first[o], o, (int)(nla - inst->width));
    for (size_t i = 0; i < (size_t)inst->nobs * inst->width; ++i)
        if (!std::isfinite(inst->weight[i]))
            return fail(LSX_EINVAL, "%s: weight[%zu][%zu] of the instrument is not finite", who, i / inst->width, i % inst->width);
    return LSX_OK;
}

int fit_instrument_upload(lsx_ctx* c, const lsx_fit_instrument* inst, double* d_head)
{
    const size_t nw = (size_t)inst->nobs * inst->width;
    HIPCHK(hipMemcpyAsync(d_head, inst->weight, nw * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_head + nw, inst->first, (size_t)inst->nobs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    return LSX_OK;
}

void fit_smear_launch(lsx_ctx* c, const FitSmear& f, size_t cl0, size_t ncol)
{
    SmearParams p{};
    p.nla = f.nla; p.nmu = f.nmu; p.nobs = f.nobs; p.width = f.width; p.P = f.P;
    p.Mo = f.ns * f.nobs * f.nmu;
    p.M = (size_t)f.ns * f.nla * f.nmu;
    p.cl0 = cl0;
    p.weight = f.d_inst;
    p.first = (const int32_t*)(f.d_inst + (size_t)f.nobs * f.width);
    p.J = f.J; p.S = f.S; p.Jo = f.Jo; p.So = f.So;
    hipLaunchKernelGGL(k_fit_smear, dim3((unsigned)((p.Mo + 63) / 64), (unsigned)ncol, (unsigned)(f.P + 1)), dim3(64), 0, c->stream, p);
}

} // namespace lsxd

extern "C" int lsx_hip_instrument_apply(lsx_ctx* c, const lsx_fit_instrument* inst, int32_t nla, int32_t nmu, int32_t nrow,
                                        const double* in, double* out)
{
    const char* who = "lsx_hip_instrument_apply";
    if (!c || !inst || !in || !out) return fail(LSX_EINVAL, "%s: null argument", who);
    if (nla < 1 || nmu < 1 || nrow < 1)
        return fail(LSX_EINVAL, "%s: nla = %d, nmu = %d, nrow = %d: need at least one of each", who, (int)nla, (int)nmu, (int)nrow);
    if ((int64_t)nla * nmu > INT32_MAX / 2) return fail(LSX_EUNSUPPORTED, "%s: nla nmu = %lld points a row", who, (long long)nla * nmu);
    int rc = fit_instrument_check(who, inst, nla, nmu, 1);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t M = (size_t)nla * nmu, Mo = (size_t)inst->nobs * nmu, head = fit_instrument_doubles(inst);
    GrowBuf& work = c->buf[BUF_FIT_WORK];
    const size_t G = pass_columns((size_t)nrow, work.cap, kWorkCapDefault, M + Mo, kGridYLimit);
    if ((rc = work.reserve(c, (head + G * (M + Mo)) * 8))) return rc;
    double* d_inst = work.as<double>();
    double* d_in = d_inst + head;
    double* d_out = d_in + G * M;
    if ((rc = fit_instrument_upload(c, inst, d_inst))) return rc;
    const FitSmear f{1, nla, nmu, inst->nobs, inst->width, 0, d_inst, nullptr, d_in, nullptr, d_out};
    for (size_t g0 = 0; g0 < (size_t)nrow; g0 += G) {
        const size_t ng = std::min(G, (size_t)nrow - g0);
        HIPCHK(hipMemcpyAsync(d_in, in + g0 * M, ng * M * 8, hipMemcpyHostToDevice, c->stream));
        fit_smear_launch(c, f, 0, ng);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + g0 * Mo, d_out, ng * Mo * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next group
    }
    return LSX_OK;
}
