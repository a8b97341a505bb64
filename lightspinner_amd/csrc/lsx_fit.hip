// lsx_fit.hip -- fitting the field vector of a column to observed Stokes profiles (include/lsx_hip_fit.h): the normal
// equations reduced on the device from the response pass's own arrays, the chi2 of a trial field, the damped step.  Read-only on the
// context; gfx950 only.  The arithmetic is lsx_fit_dev.h's.
//
// The field is expanded from the nodes ONCE, on the host, where the refusals need it (B >= a_B / 2 is known only then): that array is
// what the Stokes pass and the response pass are handed.  Per group of columns (the fit's own cap):
//   lsxd::stokes_rays_run      the body of lsx_hip_stokes_rays; its sink copies a pass's vectors into the group's S on the device
//   lsxd::response_stokes_run  the body of lsx_hip_response_stokes; its sink launches, on the pass's rf, behind the pass's kernels
//     k_fit_jac     lane = data point d of M = 4 nla nmu, block z = row j of the Jacobian: J[j][d] = sum_k rf_p[k]_d basis[j][k], the basis
//                   row in LDS; the last z forms the weight and the residual of the point.  One register accumulator a lane.
//     k_fit_reduce  one block of 256 lanes per (column, entry): the entries are the P (P + 1) / 2 sums of hess' lower triangle, the P
//                   of grad and chi2.  A lane sums the points d = lane, lane + 256, ... of (w x) y with x, y rows of J or the residual;
//                   a tree in LDS joins the 256 parts; lane 0 writes (both (a, b) and (b, a) of hess).  One accumulator a lane, one
//                   writer per value, no atomics; the order depends on M alone.
// lsx_hip_fit_field_chi2 runs the Stokes pass, the last z of k_fit_jac and the last entry of k_fit_reduce: the same instructions on the
// same numbers, hence the same bits.
// With an instrument (include/lsx_hip_fit_instrument.h) k_fit_jac forms the rows of J on the grid as above, k_fit_smear
// (lsx_fit_instrument.hip) forms J' and S' from them and from S, the z = P slice of k_fit_jac forms the weight and the residual over
// the M' = 4 nobs nmu observed points, and k_fit_reduce runs with M' in the place of M.  Without one nothing here changes.
//   k_fit_step    lane = column: lsxfit::step_solve / step_finish with the packed triangle and the right-hand side in LDS, element e of
//                 lane l at [e][l] as solve_mem has its work space (lsx_solve_dev.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_final_host.h"
#include "lsx_fit_dev.h"
#include "lsx_fit_inst.h"
#include "lsx_stokes_prep.h"

using namespace lsxd;

static_assert(lsxfit::kMaxParams == LSX_FIT_MAX_PARAMS, "the header's limit is the device code's");

namespace {

constexpr size_t kWorkCapDefault = (size_t)64 << 20;        // bytes (include/lsx_hip_fit.h)
constexpr size_t kStepLdsBytes = (size_t)48 << 10;          // what a block of k_fit_step may take for its work space

struct FitParams {
    int32_t Ns, nla, nmu, M, P, npar;
    int32_t e0;                       // the first entry of this launch of k_fit_reduce
    int32_t cl0;                      // the group-local column of the launch's first column
    int8_t row_par[lsxfit::kMaxParams];   // per row of the Jacobian: its parameter's place among rf's parameters
    const double* rf;                 // the response pass's array, [launch column][npar][4][nla][Ns][nmu]
    const double* basis;              // [P][Ns]
    const double *obs, *weight, *S;   // [group column][M]; weight may be null
    double *R, *W, *J;                // [group column][M], [group column][M], [group column][P][M]
    double *chi2, *grad, *hess;       // [group column], [..][P], [..][P][P]
};

__global__ void __launch_bounds__(64) k_fit_jac(const FitParams p)
{
    extern __shared__ double smem[];                  // the basis row
    const int j = blockIdx.z;
    const int M = p.M;
    const size_t cl = (size_t)p.cl0 + blockIdx.y;
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (j == p.P) {                                   // (block-uniform) the weight in use and the residual
        if (d < M) {
            double w, r;
            lsxfit::residual(p.weight ? p.weight + cl * M : nullptr, p.obs + cl * M, p.S + cl * M, (size_t)d, w, r);
            p.W[cl * M + d] = w;
            p.R[cl * M + d] = r;
        }
        return;
    }
    for (int k = threadIdx.x; k < p.Ns; k += 64) smem[k] = p.basis[(size_t)j * p.Ns + k];
    __syncthreads();
    if (d >= M) return;
    const size_t block = (size_t)p.Ns * p.nmu;        // one (parameter, Stokes parameter, wavelength) of rf: [Ns][nmu]
    const int sl = d / p.nmu, m = d - sl * p.nmu;     // d = (s nla + la) nmu + m
    const double* rf = p.rf + ((size_t)blockIdx.y * p.npar + p.row_par[j]) * 4 * p.nla * block + (size_t)sl * block + m;
    p.J[(cl * p.P + j) * M + d] = lsxfit::contract(rf, (size_t)p.nmu, (const lds_f64*)smem, p.Ns);
}

__global__ void __launch_bounds__(lsxfit::kReduceLanes) k_fit_reduce(const FitParams p)
{
    __shared__ double v[lsxfit::kReduceLanes];
    const int lane = threadIdx.x, M = p.M, P = p.P;
    const size_t cl = (size_t)p.cl0 + blockIdx.y;
    int a, b;
    lsxfit::entry_pair(P, p.e0 + (int)blockIdx.x, a, b);
    const double* R = p.R + cl * M;
    const double* x = a >= 0 ? p.J + (cl * P + a) * M : R;
    const double* y = b >= 0 ? p.J + (cl * P + b) * M : R;
    lds_f64* vl = (lds_f64*)v;
    vl[lane] = lsxfit::lane_sum(lane, M, p.W + cl * M, x, y);
    __syncthreads();
    for (int s = lsxfit::kReduceLanes / 2; s > 0; s >>= 1) {
        if (lane < s) lsxfit::tree_step(vl, lane, s);
        __syncthreads();
    }
    if (lane) return;
    const double sum = vl[0];
    if (b >= 0) {
        p.hess[(cl * P + a) * P + b] = sum;
        if (a != b) p.hess[(cl * P + b) * P + a] = sum;
    } else if (a >= 0) {
        p.grad[cl * P + a] = sum;
    } else {
        p.chi2[cl] = sum;
    }
}

struct StepParams {
    int32_t ncol, P, cpb;             // columns of the launch, parameters, columns (lanes) per block
    const double *hess, *grad, *lambda, *nodes, *lo, *hi;
    double *trial, *predicted;
    int32_t* status;
};

__global__ void __launch_bounds__(64) k_fit_step(const StepParams p)
{
    extern __shared__ double smem[];                  // [step_doubles(P)][cpb]
    const size_t c = (size_t)blockIdx.x * p.cpb + threadIdx.x;
    if (c >= (size_t)p.ncol) return;
    const int P = p.P;
    lds_f64* w = (lds_f64*)smem + threadIdx.x;
    const double* H = p.hess + c * P * P;
    const double* g = p.grad + c * P;
    const int st = lsxfit::step_solve(P, H, g, p.lambda[c], w, (size_t)p.cpb);
    p.predicted[c] = lsxfit::step_finish(P, st, H, g, p.nodes + c * P, p.lo, p.hi, w + (size_t)P * (P + 1) / 2 * p.cpb, (size_t)p.cpb,
                                         p.trial + c * P);
    p.status[c] = st;
}

bool all_finite(const double* a, size_t n, size_t& bad)
{
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i])) { bad = i; return false; }
    return true;
}

// the sink of the Stokes pass: the pass's vectors into the group's S
struct KeepStokes final : PassSink {
    lsx_ctx* c;
    double* d_S;
    size_t M;
    int pass(size_t b0, size_t nb, const double* d_out) override
    {
        HIPCHK(hipMemcpyAsync(d_S + b0 * M, d_out, nb * M * 8, hipMemcpyDeviceToDevice, c->stream));
        return LSX_OK;
    }
};

// the same with an instrument: p is the reduction's (M = M', J = J', S = S'), grid the Jacobian's on the window's wavelengths
void launch_sums_inst(lsx_ctx* c, const FitParams& p, FitSmear f, const FitParams& grid, size_t b0, size_t nb, const double* d_rf, bool normal)
{
    const int nent = lsxfit::entries(p.P);
    if (normal) {
        FitParams g = grid;
        g.cl0 = (int32_t)b0;
        g.rf = d_rf;
        hipLaunchKernelGGL(k_fit_jac, dim3((unsigned)((g.M + 63) / 64), (unsigned)nb, (unsigned)g.P), dim3(64), (size_t)g.Ns * 8, c->stream, g);
    } else {
        f.P = 0;                      // the Stokes vector alone
    }
    fit_smear_launch(c, f, b0, nb);
    FitParams q = p;                  // the residual's slice of k_fit_jac over the observed points
    q.cl0 = (int32_t)b0;
    q.P = 0;
    hipLaunchKernelGGL(k_fit_jac, dim3((unsigned)((q.M + 63) / 64), (unsigned)nb, 1u), dim3(64), (size_t)q.Ns * 8, c->stream, q);
    q.P = p.P;
    q.e0 = normal ? 0 : nent - 1;
    hipLaunchKernelGGL(k_fit_reduce, dim3(normal ? (unsigned)nent : 1u, (unsigned)nb), dim3(lsxfit::kReduceLanes), 0, c->stream, q);
}

void launch_sums(lsx_ctx* c, FitParams p, size_t b0, size_t nb, const double* d_rf, bool normal)
{
    p.cl0 = (int32_t)b0;
    p.rf = d_rf;
    const unsigned nblk = (unsigned)((p.M + 63) / 64);
    const int nent = lsxfit::entries(p.P);
    if (normal) {
        hipLaunchKernelGGL(k_fit_jac, dim3(nblk, (unsigned)nb, (unsigned)(p.P + 1)), dim3(64), (size_t)p.Ns * 8, c->stream, p);
        p.e0 = 0;
        hipLaunchKernelGGL(k_fit_reduce, dim3((unsigned)nent, (unsigned)nb), dim3(lsxfit::kReduceLanes), 0, c->stream, p);
    } else {
        // the residual's slice of k_fit_jac alone (its z is P: the launch says P = 0, and no row of J is read), then the last entry
        FitParams q = p;
        q.P = 0;
        hipLaunchKernelGGL(k_fit_jac, dim3(nblk, (unsigned)nb, 1u), dim3(64), (size_t)p.Ns * 8, c->stream, q);
        p.e0 = nent - 1;
        hipLaunchKernelGGL(k_fit_reduce, dim3(1u, (unsigned)nb), dim3(lsxfit::kReduceLanes), 0, c->stream, p);
    }
}

// the sink of the response pass: the sums of the pass's columns from the pass's rf
struct SumPass final : PassSink {
    lsx_ctx* c;
    FitParams p, grid;
    FitSmear smear;
    bool inst;
    int pass(size_t b0, size_t nb, const double* d_rf) override
    {
        if (inst) launch_sums_inst(c, p, smear, grid, b0, nb, d_rf, true);
        else launch_sums(c, p, b0, nb, d_rf, true);
        HIPCHK(hipGetLastError());
        return LSX_OK;
    }
};

// both entries: normal (grad, hess, amplitude given) or chi2 alone.  nq: the quantities of the parameterisation -- 3 (B, gammaB, chiB:
// include/lsx_hip_fit.h) or 4 (with vlos: include/lsx_hip_stokes_velocity.h; the passes are then handed the expanded velocity);
// nnode, amplitude hold nq entries, base and field_out nq rows a column
int fit_run(lsx_ctx* c, const char* who, bool normal, int nq, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
            const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift, const int32_t* nnode,
            const double* basis, const double* base, const double* nodes, const double* amplitude, const double* obs,
            const double* weight, double* chi2, double* grad, double* hess, double* field_out, const lsx_fit_instrument* inst)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c || !mu || !nnode || !basis || !nodes || !obs || !chi2 || (normal && (!grad || !hess || !amplitude)))
        return fail(LSX_EINVAL, "%s: null argument", who);
    int rc = final_check_angles(who, nmu, mu);
    if (!rc) rc = final_check_range(c, who, col0, ncol);
    if (!rc) rc = final_check_window(c, who, la0, nla);
    if (rc) return rc;
    if (inst && (rc = fit_instrument_check(who, inst, nla, nmu, 4))) return rc;
    int64_t Psum = 0;
    for (int a = 0; a < nq; ++a) {
        if (nnode[a] < 0) return fail(LSX_EINVAL, "%s: nnode[%d] = %d is negative", who, a, (int)nnode[a]);
        Psum += nnode[a];
    }
    if (Psum < 1 || Psum > LSX_FIT_MAX_PARAMS)
        return fail(LSX_EINVAL, "%s: %lld node values; between 1 and %d can be fitted", who, (long long)Psum, LSX_FIT_MAX_PARAMS);
    const int P = (int)Psum, Ns = c->Nspace;
    if ((int64_t)4 * nla * nmu > INT32_MAX / 2) return fail(LSX_EUNSUPPORTED, "%s: 4 nla nmu = %lld data points a column", who, 4LL * nla * nmu);
    const size_t Mg = (size_t)4 * nla * nmu, NC = (size_t)ncol;       // the points of the window's grid a column
    const size_t M = inst ? (size_t)4 * inst->nobs * nmu : Mg;        // the data points a column
    size_t bad = 0;
    if (!all_finite(basis, (size_t)P * Ns, bad))
        return fail(LSX_EINVAL, "%s: basis[%zu][%zu] is not finite", who, bad / Ns, bad % Ns);
    if (base && !all_finite(base, NC * nq * Ns, bad))
        return fail(LSX_EINVAL, "%s: base of column %d, parameter %zu, depth %zu is not finite", who, col0 + (int)(bad / (nq * (size_t)Ns)),
                    bad / Ns % nq, bad % Ns);
    if (!all_finite(nodes, NC * P, bad)) return fail(LSX_EINVAL, "%s: node %zu of column %d is not finite", who, bad % P, col0 + (int)(bad / P));
    if (!all_finite(obs, NC * M, bad)) return fail(LSX_EINVAL, "%s: obs of column %d is not finite (entry %zu)", who, col0 + (int)(bad / M), bad % M);
    if (weight) {
        if (!all_finite(weight, NC * M, bad))
            return fail(LSX_EINVAL, "%s: weight of column %d is not finite (entry %zu)", who, col0 + (int)(bad / M), bad % M);
        for (size_t i = 0; i < NC * M; ++i)
            if (weight[i] < 0.0)
                return fail(LSX_EINVAL, "%s: weight of column %d is negative (entry %zu): %g", who, col0 + (int)(i / M), i % M, weight[i]);
    }
    // the expansion, in this one place: what is checked below is what the passes are handed
    constexpr int kQ = lsxst::kMaxResponseParams;
    std::vector<double> fld((size_t)nq * NC * Ns);
    double* F[kQ] = {nullptr, nullptr, nullptr, nullptr};
    int row0[kQ] = {0, 0, 0, 0};
    for (int a = 0; a < nq; ++a) {
        F[a] = fld.data() + (size_t)a * NC * Ns;
        row0[a] = a ? row0[a - 1] + nnode[a - 1] : 0;
    }
    for (size_t q = 0; q < NC; ++q)
        for (int a = 0; a < nq; ++a)
            for (int k = 0; k < Ns; ++k)
                F[a][q * Ns + k] = lsxfit::expand(base ? base[(q * nq + a) * Ns + k] : 0.0, nnode[a], nodes + q * P + row0[a],
                                                  basis + (size_t)row0[a] * Ns, (size_t)Ns, (size_t)k);
    uint32_t params = 0;
    for (int a = 0; a < nq; ++a) params |= nnode[a] > 0 ? 1u << a : 0u;
    // what the passes are asked for columns [g0, g0 + ng) of the fit's
    const auto call = [&](size_t g0, size_t ng) {
        return StokesCall{nmu, mu, col0 + (int32_t)g0, (int32_t)ng, la0, nla, F[0] + g0 * Ns, F[1] + g0 * Ns, F[2] + g0 * Ns,
                          ncomp, alpha, strength, shift, nq > 3 ? F[3] + g0 * Ns : nullptr};
    };
    // chi2 alone: the response's rules without an amplitude's (the Stokes pass's rules are their first part, in its order)
    static const double unit_amp[kQ] = {0.0, 1.0, 1.0, 1.0};
    if ((rc = response_stokes_check(c, who, call(0, NC), normal ? params : 2u, normal ? amplitude : unit_amp, 0, nullptr))) return rc;
    if (field_out)
        for (size_t q = 0; q < NC; ++q)
            for (int a = 0; a < nq; ++a) std::copy(F[a] + q * Ns, F[a] + (q + 1) * Ns, field_out + (q * nq + a) * Ns);

    // ---- groups of columns under the fit's cap ----
    HIPCHK(hipSetDevice(c->device));
    const size_t nW = weight ? 1 : 0;
    const size_t sums = 1 + (normal ? (size_t)P + (size_t)P * P : 0);
    // obs, S, weight; R, W; J; the sums -- with an instrument S and J on the grid besides S' and J' on the pixels
    const size_t wcol = (2 + nW) * M + 2 * M + (normal ? (size_t)P * M : 0) + sums + (inst ? Mg + (normal ? (size_t)P * Mg : 0) : 0);
    const size_t head = (size_t)P * Ns + (inst ? fit_instrument_doubles(inst) : 0);
    GrowBuf& work = c->buf[BUF_FIT_WORK];
    const size_t G = pass_columns(NC, work.cap, kWorkCapDefault, wcol, kGridYLimit);
    if ((rc = work.reserve(c, (head + G * wcol) * 8))) return rc;
    double* d_basis = work.as<double>();
    double* d_inst = d_basis + (size_t)P * Ns;
    double* d_obs = d_basis + head;
    double* d_S = d_obs + G * M;
    double* d_wt = d_S + G * M;
    double* d_R = d_wt + nW * G * M;
    double* d_W = d_R + G * M;
    double* d_J = d_W + G * M;
    double* d_chi2 = d_J + (normal ? G * P * M : 0);
    double* d_grad = d_chi2 + G;
    double* d_hess = d_grad + (normal ? G * P : 0);
    double* d_Sg = d_hess + (normal ? G * P * P : 0);                 // with an instrument: S and J on the grid
    double* d_Jg = d_Sg + G * Mg;
    HIPCHK(hipMemcpyAsync(d_basis, basis, (size_t)P * Ns * 8, hipMemcpyHostToDevice, c->stream));
    if (inst && (rc = fit_instrument_upload(c, inst, d_inst))) return rc;

    FitParams p{};
    p.Ns = Ns; p.nla = nla; p.nmu = nmu; p.M = (int32_t)M; p.P = P;
    int par[kQ] = {0, 0, 0, 0};
    p.npar = lsxst::response_params(params, par);
    for (int i = 0, j = 0; i < p.npar; ++i)
        for (int n = 0; n < nnode[par[i]]; ++n) p.row_par[j++] = (int8_t)i;
    p.basis = d_basis; p.obs = d_obs; p.weight = weight ? d_wt : nullptr; p.S = d_S;
    p.R = d_R; p.W = d_W; p.J = d_J; p.chi2 = d_chi2; p.grad = d_grad; p.hess = d_hess;
    FitParams grid = p;               // with an instrument: k_fit_jac's rows on the grid; p is what is reduced
    FitSmear smear{};
    if (inst) {
        grid.M = (int32_t)Mg; grid.J = d_Jg; grid.S = d_Sg;
        smear = FitSmear{4, nla, nmu, inst->nobs, inst->width, P, d_inst, d_Jg, d_Sg, d_J, d_S};
    }

    for (size_t g0 = 0; g0 < NC; g0 += G) {
        const size_t ng = std::min(G, NC - g0);
        HIPCHK(hipMemcpyAsync(d_obs, obs + g0 * M, ng * M * 8, hipMemcpyHostToDevice, c->stream));
        if (weight) HIPCHK(hipMemcpyAsync(d_wt, weight + g0 * M, ng * M * 8, hipMemcpyHostToDevice, c->stream));
        const StokesCall s = call(g0, ng);
        KeepStokes keep;
        keep.c = c; keep.d_S = inst ? d_Sg : d_S; keep.M = Mg;
        if ((rc = stokes_rays_run(c, who, s, nullptr, 0, &keep))) return rc;
        if (normal) {
            SumPass sum;
            sum.c = c; sum.p = p; sum.grid = grid; sum.smear = smear; sum.inst = inst != nullptr;
            if ((rc = response_stokes_run(c, who, s, params, amplitude, 0, nullptr, nullptr, 0, nullptr, &sum))) return rc;
        } else {
            if (inst) launch_sums_inst(c, p, smear, grid, 0, ng, nullptr, false);
            else launch_sums(c, p, 0, ng, nullptr, false);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(chi2 + g0, d_chi2, ng * 8, hipMemcpyDeviceToHost, c->stream));
        if (normal) {
            HIPCHK(hipMemcpyAsync(grad + g0 * P, d_grad, ng * P * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(hess + g0 * P * P, d_hess, ng * P * P * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next group
    }
    return LSX_OK;
}

} // namespace

extern "C" int lsx_hip_fit_field_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_FIT_WORK, "lsx_hip_fit_field_work_cap", nbytes);
}

extern "C" int lsx_hip_fit_field_normal(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                        const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                        const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                                        const double amplitude[3], const double* obs, const double* weight,
                                        double* chi2, double* grad, double* hess, double* field_out)
{
    return fit_run(c, "lsx_hip_fit_field_normal", true, 3, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base,
                   nodes, amplitude, obs, weight, chi2, grad, hess, field_out, nullptr);
}

extern "C" int lsx_hip_fit_field_chi2(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                      const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                      const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                                      const double* obs, const double* weight, double* chi2, double* field_out)
{
    return fit_run(c, "lsx_hip_fit_field_chi2", false, 3, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base, nodes,
                   nullptr, obs, weight, chi2, nullptr, nullptr, field_out, nullptr);
}

// through an instrument (include/lsx_hip_fit_instrument.h); inst == NULL: the two entries above
extern "C" int lsx_hip_instrument_fit_normal(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                             const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                             const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                                             const double amplitude[3], const double* obs, const double* weight,
                                             double* chi2, double* grad, double* hess, double* field_out, const lsx_fit_instrument* inst)
{
    if (!inst)
        return lsx_hip_fit_field_normal(c, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base, nodes, amplitude,
                                        obs, weight, chi2, grad, hess, field_out);
    return fit_run(c, "lsx_hip_instrument_fit_normal", true, 3, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base,
                   nodes, amplitude, obs, weight, chi2, grad, hess, field_out, inst);
}

extern "C" int lsx_hip_instrument_fit_chi2(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                           const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                           const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                                           const double* obs, const double* weight, double* chi2, double* field_out,
                                           const lsx_fit_instrument* inst)
{
    if (!inst)
        return lsx_hip_fit_field_chi2(c, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base, nodes, obs, weight,
                                      chi2, field_out);
    return fit_run(c, "lsx_hip_instrument_fit_chi2", false, 3, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base,
                   nodes, nullptr, obs, weight, chi2, nullptr, nullptr, field_out, inst);
}

// with four quantities (include/lsx_hip_stokes_velocity.h): the velocity is a row of the expanded field like the others
extern "C" int lsx_hip_velocity_fit_normal(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                           const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                           const int32_t nnode[4], const double* basis, const double* base, const double* nodes,
                                           const double amplitude[4], const double* obs, const double* weight,
                                           double* chi2, double* grad, double* hess, double* field_out, const lsx_fit_instrument* inst)
{
    return fit_run(c, "lsx_hip_velocity_fit_normal", true, 4, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base,
                   nodes, amplitude, obs, weight, chi2, grad, hess, field_out, inst);
}

extern "C" int lsx_hip_velocity_fit_chi2(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                         const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                         const int32_t nnode[4], const double* basis, const double* base, const double* nodes,
                                         const double* obs, const double* weight, double* chi2, double* field_out,
                                         const lsx_fit_instrument* inst)
{
    return fit_run(c, "lsx_hip_velocity_fit_chi2", false, 4, nmu, mu, col0, ncol, la0, nla, ncomp, alpha, strength, shift, nnode, basis, base, nodes,
                   nullptr, obs, weight, chi2, nullptr, nullptr, field_out, inst);
}

extern "C" int lsx_hip_fit_field_step(lsx_ctx* c, int32_t ncol, int32_t P, const double* hess, const double* grad, const double* lambda,
                                      const double* nodes, const double* lo, const double* hi, double* trial, double* predicted,
                                      int32_t* status)
{
    const char* who = "lsx_hip_fit_field_step";
    if (!c || !hess || !grad || !lambda || !nodes || !lo || !hi || !trial || !predicted || !status)
        return fail(LSX_EINVAL, "%s: null argument", who);
    if (ncol < 1) return fail(LSX_EINVAL, "%s: ncol = %d, need at least one column", who, (int)ncol);
    if (P < 1 || P > LSX_FIT_MAX_PARAMS) return fail(LSX_EINVAL, "%s: P = %d; between 1 and %d", who, (int)P, LSX_FIT_MAX_PARAMS);
    for (int q = 0; q < ncol; ++q)
        if (!(std::isfinite(lambda[q]) && lambda[q] >= 0.0))
            return fail(LSX_EINVAL, "%s: lambda of column %d is %g: it must be finite and not negative", who, q, lambda[q]);
    for (int i = 0; i < P; ++i)
        if (!(lo[i] <= hi[i])) return fail(LSX_EINVAL, "%s: bounds of node %d: lo = %g, hi = %g", who, i, lo[i], hi[i]);
    HIPCHK(hipSetDevice(c->device));
    // per column: hess, grad, nodes, trial, lambda, predicted, status (a double's place)
    const size_t PP = (size_t)P * P, wcol = PP + 3 * (size_t)P + 3, head = 2 * (size_t)P;
    GrowBuf& work = c->buf[BUF_FIT_WORK];
    const size_t G = pass_columns((size_t)ncol, work.cap, kWorkCapDefault, wcol, kNoColumnLimit);      // (the columns are the grid's x)
    const int rc = work.reserve(c, (head + G * wcol) * 8);
    if (rc) return rc;
    double* d_lo = work.as<double>();
    double* d_hi = d_lo + P;
    double* d_hess = d_hi + P;
    double* d_grad = d_hess + G * PP;
    double* d_nodes = d_grad + G * P;
    double* d_trial = d_nodes + G * P;
    double* d_lambda = d_trial + G * P;
    double* d_pred = d_lambda + G;
    int32_t* d_status = (int32_t*)(d_pred + G);
    HIPCHK(hipMemcpyAsync(d_lo, lo, (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_hi, hi, (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
    // lanes per block: a power of two whose work space fits
    int cpb = 64;
    while (cpb > 1 && (size_t)cpb * lsxfit::step_doubles(P) * 8 > kStepLdsBytes) cpb >>= 1;
    StepParams p{};
    p.P = P; p.cpb = cpb;
    p.hess = d_hess; p.grad = d_grad; p.lambda = d_lambda; p.nodes = d_nodes; p.lo = d_lo; p.hi = d_hi;
    p.trial = d_trial; p.predicted = d_pred; p.status = d_status;
    for (size_t g0 = 0; g0 < (size_t)ncol; g0 += G) {
        const size_t ng = std::min(G, (size_t)ncol - g0);
        HIPCHK(hipMemcpyAsync(d_hess, hess + g0 * PP, ng * PP * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_grad, grad + g0 * P, ng * P * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_nodes, nodes + g0 * P, ng * P * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_lambda, lambda + g0, ng * 8, hipMemcpyHostToDevice, c->stream));
        p.ncol = (int32_t)ng;
        hipLaunchKernelGGL(k_fit_step, dim3((unsigned)((ng + cpb - 1) / cpb)), dim3((unsigned)cpb), (size_t)cpb * lsxfit::step_doubles(P) * 8,
                           c->stream, p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(trial + g0 * P, d_trial, ng * P * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(predicted + g0, d_pred, ng * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status + g0, d_status, ng * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return LSX_OK;
}
