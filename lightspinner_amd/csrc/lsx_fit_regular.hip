// lsx_fit_regular.hip -- the penalty of a regularised field fit and the uncertainties of the fitted nodes (include/lsx_hip_fit_regular.h;
// DESIGN.md 4.27).  Read-only on the context; gfx950 only.  The arithmetic is lsx_fit_regular_dev.h's.
//   k_regular_penalty     one block of 256 lanes per column.  L (at most 96 x 24 doubles, 18 KiB) is copied to LDS; the lanes q form the
//                         pseudo-residuals rho_q there; after a barrier lane = entry in the numbering of lsxfit::entries / entry_pair
//                         (hess' lower triangle, grad, chi2; 325 at P = 24, so some lanes take two): a sum over q ascending, added to
//                         the value handed in.  A launch takes a range of entries: all of them, chi2 alone, or hess alone (the A of the
//                         uncertainties: nothing of rho is formed then).
//   k_regular_covariance  one wavefront per column.  The packed lower triangle of A goes to LDS, lane 0 factorises it in place; lane j < P
//                         solves A x = e_j with its work space at [i][lane] (as k_fit_step has it), then the column j of hess ainv
//                         beside it, then row j of cov's lower triangle from both.  Without a penalty cov is ainv's lower triangle.
//   k_regular_band        lane = depth, grid y = column, z = parameter: the parameter's block of cov in LDS, the quadratic form per depth.
// One writer per value; no atomics, no scratch.  All three are launch-latency bound at every size the entries accept.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_dev.h"
#include "lsx_fit_regular_dev.h"
#include "lsx_plan.h"

using namespace lsxd;

static_assert(lsxfit::kMaxParams == LSX_FIT_MAX_PARAMS && lsxreg::kMaxRows == 4 * LSX_FIT_MAX_PARAMS, "the headers' limits are the device code's");

namespace {

constexpr size_t kWorkCapDefault = (size_t)64 << 20;        // bytes (include/lsx_hip_fit.h: the fit's own buffer)
constexpr int kPenaltyLanes = 256;
constexpr int kTriangle = lsxfit::kMaxParams * (lsxfit::kMaxParams + 1) / 2;

struct PenaltyParams {
    int32_t P, Q, e0, ne;             // the entries [e0, e0 + ne) of lsxfit::entries(P)
    const double *L, *target, *nodes; // [Q][P]; [column][Q] or null; [column][P] (null: no entry of the launch reads rho)
    double *chi2, *grad, *hess, *penalty_out;
};

__global__ void __launch_bounds__(kPenaltyLanes) k_regular_penalty(const PenaltyParams p)
{
    __shared__ double sL[lsxreg::kMaxRows * lsxfit::kMaxParams];
    __shared__ double srho[lsxreg::kMaxRows];
    lds_f64* L = (lds_f64*)sL;
    lds_f64* rho = (lds_f64*)srho;
    const int lane = threadIdx.x, P = p.P, Q = p.Q;
    const size_t c = blockIdx.x;
    for (int i = lane; i < Q * P; i += kPenaltyLanes) L[i] = p.L[i];
    __syncthreads();
    if (p.nodes)                                      // (block-uniform)
        for (int q = lane; q < Q; q += kPenaltyLanes)
            rho[q] = lsxreg::pseudo(p.target ? p.target[c * Q + q] : 0.0, P, (const lds_f64*)L + q * P, p.nodes + c * P);
    __syncthreads();
    for (int e = p.e0 + lane; e < p.e0 + p.ne; e += kPenaltyLanes) {
        int a, b;
        lsxfit::entry_pair(P, e, a, b);
        const double sum = lsxreg::entry_sum(P, Q, a, b, (const lds_f64*)L, (const lds_f64*)rho);
        // (a launch holds only the arrays its range of entries writes: the others are null, and entry_add writes through no null)
        lsxreg::entry_add(P, a, b, sum, p.chi2 ? p.chi2 + c : nullptr, p.grad ? p.grad + c * P : nullptr, p.hess ? p.hess + c * P * P : nullptr,
                          p.penalty_out ? p.penalty_out + c : nullptr);
    }
}

struct CovParams {
    int32_t P, sandwich;              // sandwich: A is not hess, cov = ainv^T hess ainv
    const double *A, *hess, *scale;   // [column][P][P] both; [column] or null
    double *ainv, *cov, *sigma;       // ainv may be null
    int32_t* status;
};

__global__ void __launch_bounds__(64) k_regular_covariance(const CovParams p)
{
    __shared__ double sf[kTriangle];                          // the packed triangle of A, then its factor
    __shared__ double sx[lsxfit::kMaxParams * 64];            // element i of lane j's column of ainv at [i][j]
    __shared__ double sm[lsxfit::kMaxParams * 64];            // ... of hess ainv
    __shared__ int sbad;
    lds_f64* f = (lds_f64*)sf;
    lds_f64* x = (lds_f64*)sx;
    lds_f64* m = (lds_f64*)sm;
    const int lane = threadIdx.x, P = p.P;
    const size_t c = blockIdx.x, PP = (size_t)P * P;
    for (int e = lane; e < P * P; e += 64) {
        const int i = e / P, j = e - i * P;
        if (j <= i) f[lsxfit::tri(i, j)] = p.A[c * PP + e];
    }
    __syncthreads();
    if (lane == 0) sbad = lsxreg::factor(P, f, 1);
    __syncthreads();
    int bad = sbad;
    int mine = 0;
    if (!bad && lane < P) mine = lsxreg::unit_solve(P, lane, (const lds_f64*)f, 1, x + lane, 64);
    bad |= __any(mine) ? 1 : 0;                               // (the block is one wavefront)
    if (bad) {
        for (int e = lane; e < P * P; e += 64) {
            if (p.ainv) p.ainv[c * PP + e] = NAN;
            p.cov[c * PP + e] = NAN;
        }
        if (lane < P) p.sigma[c * P + lane] = NAN;
        if (lane == 0) p.status[c] = 1;
        return;
    }
    if (p.sandwich && lane < P) lsxreg::hess_times(P, p.hess + c * PP, (const lds_f64*)x + lane, m + lane, 64);
    __syncthreads();
    if (lane == 0) p.status[c] = 0;
    if (lane >= P) return;
    if (p.ainv)
        for (int i = 0; i < P; ++i) p.ainv[c * PP + (size_t)i * P + lane] = x[i * 64 + lane];
    for (int b = 0; b <= lane; ++b) {
        double v = p.sandwich ? lsxreg::sandwich(P, (const lds_f64*)x + lane, (const lds_f64*)m + b, 64) : x[lane * 64 + b];
        if (p.scale) v = p.scale[c] * v;
        p.cov[c * PP + (size_t)lane * P + b] = v;
        if (b != lane) p.cov[c * PP + (size_t)b * P + lane] = v;
        else p.sigma[c * P + lane] = sqrt(v);
    }
}

struct BandParams {
    int32_t P, Ns, npar;
    int32_t row0[4], nn[4];           // per parameter: its first row of basis and its node count
    const double *cov, *basis;        // [column][P][P]; [P][Ns]
    const int32_t* status;
    double* out;                      // [column][npar][Ns]
};

__global__ void __launch_bounds__(64) k_regular_band(const BandParams p)
{
    __shared__ double sc[lsxfit::kMaxParams * lsxfit::kMaxParams];
    lds_f64* cv = (lds_f64*)sc;
    const int lane = threadIdx.x, q = blockIdx.z, nn = p.nn[q], r0 = p.row0[q];
    const size_t c = blockIdx.y;
    for (int e = lane; e < nn * nn; e += 64) {
        const int n = e / nn, mm = e - n * nn;
        cv[e] = p.cov[(c * p.P + r0 + n) * p.P + r0 + mm];
    }
    __syncthreads();
    const int k = blockIdx.x * 64 + lane;
    if (k >= p.Ns) return;
    double v = 0.0;
    if (p.status[c]) v = NAN;
    else if (nn) v = sqrt(lsxreg::band(nn, (const lds_f64*)cv, p.basis + (size_t)r0 * p.Ns, (size_t)p.Ns, (size_t)k));
    p.out[(c * p.npar + q) * p.Ns + k] = v;
}

} // namespace

extern "C" int lsx_hip_regular_penalty(lsx_ctx* c, int32_t ncol, int32_t P, const lsx_fit_penalty* pen, const double* nodes,
                                       double* chi2, double* grad, double* hess, double* penalty_out)
{
    const char* who = "lsx_hip_regular_penalty";
    char msg[256];
    if (!c) return fail(LSX_EINVAL, "%s: null argument", who);
    if (lsxreg::penalty_args(who, ncol, P, pen, nodes, chi2, grad, hess, msg, sizeof msg)) return fail(LSX_EINVAL, "%s", msg);
    HIPCHK(hipSetDevice(c->device));
    const bool full = grad != nullptr;
    const size_t Q = (size_t)pen->nrow, PP = (size_t)P * P, NC = (size_t)ncol;
    const size_t nT = pen->target ? Q : 0;
    // per column: nodes, target, chi2, the penalty alone, grad, hess
    const size_t wcol = (size_t)P + nT + 2 + (full ? (size_t)P + PP : 0), head = Q * P;
    GrowBuf& work = c->buf[BUF_FIT_WORK];
    const size_t G = pass_columns(NC, work.cap, kWorkCapDefault, wcol, kNoColumnLimit);        // (the columns are the grid's x)
    const int rc = work.reserve(c, (head + G * wcol) * 8);
    if (rc) return rc;
    double* d_L = work.as<double>();
    double* d_nodes = d_L + head;
    double* d_target = d_nodes + G * P;
    double* d_chi2 = d_target + G * nT;
    double* d_pen = d_chi2 + G;
    double* d_grad = d_pen + G;
    double* d_hess = d_grad + (full ? G * P : 0);
    HIPCHK(hipMemcpyAsync(d_L, pen->L, head * 8, hipMemcpyHostToDevice, c->stream));
    PenaltyParams p{};
    p.P = P; p.Q = (int32_t)Q;
    const int nent = lsxfit::entries(P);
    p.e0 = full ? 0 : nent - 1;
    p.ne = full ? nent : 1;
    p.L = d_L; p.target = nT ? d_target : nullptr; p.nodes = d_nodes;
    p.chi2 = d_chi2; p.grad = full ? d_grad : nullptr; p.hess = full ? d_hess : nullptr; p.penalty_out = d_pen;
    for (size_t g0 = 0; g0 < NC; g0 += G) {
        const size_t ng = std::min(G, NC - g0);
        HIPCHK(hipMemcpyAsync(d_nodes, nodes + g0 * P, ng * P * 8, hipMemcpyHostToDevice, c->stream));
        if (nT) HIPCHK(hipMemcpyAsync(d_target, pen->target + g0 * Q, ng * Q * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_chi2, chi2 + g0, ng * 8, hipMemcpyHostToDevice, c->stream));
        if (full) {
            HIPCHK(hipMemcpyAsync(d_grad, grad + g0 * P, ng * P * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_hess, hess + g0 * PP, ng * PP * 8, hipMemcpyHostToDevice, c->stream));
        }
        hipLaunchKernelGGL(k_regular_penalty, dim3((unsigned)ng), dim3(kPenaltyLanes), 0, c->stream, p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(chi2 + g0, d_chi2, ng * 8, hipMemcpyDeviceToHost, c->stream));
        if (penalty_out) HIPCHK(hipMemcpyAsync(penalty_out + g0, d_pen, ng * 8, hipMemcpyDeviceToHost, c->stream));
        if (full) {
            HIPCHK(hipMemcpyAsync(grad + g0 * P, d_grad, ng * P * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(hess + g0 * PP, d_hess, ng * PP * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next group
    }
    return LSX_OK;
}

extern "C" int lsx_hip_regular_uncertainty(lsx_ctx* c, int32_t ncol, int32_t P, const double* hess, const lsx_fit_penalty* pen,
                                           const double* scale, int32_t npar, const int32_t* nnode, const double* basis, int32_t Nspace,
                                           double* ainv, double* cov, double* sigma, double* field_sigma, int32_t* status)
{
    const char* who = "lsx_hip_regular_uncertainty";
    char msg[256];
    if (!c) return fail(LSX_EINVAL, "%s: null argument", who);
    if (lsxreg::uncertainty_args(who, ncol, P, hess, pen, scale, npar, nnode, basis, Nspace, cov, sigma, status, msg, sizeof msg))
        return fail(LSX_EINVAL, "%s", msg);
    HIPCHK(hipSetDevice(c->device));
    const size_t Q = pen ? (size_t)pen->nrow : 0, PP = (size_t)P * P, NC = (size_t)ncol, Ns = (size_t)Nspace;
    const size_t nA = pen ? PP : 0, nI = ainv ? PP : 0, nS = scale ? 1 : 0, nF = field_sigma ? (size_t)npar * Ns : 0;
    // per column: hess, A, ainv, cov, sigma, scale, status (a double's place), field_sigma
    const size_t wcol = PP + nA + nI + PP + (size_t)P + nS + 1 + nF, head = Q * P + (field_sigma ? (size_t)P * Ns : 0);
    GrowBuf& work = c->buf[BUF_FIT_WORK];
    const size_t G = pass_columns(NC, work.cap, kWorkCapDefault, wcol, kGridYLimit);            // (k_regular_band: the columns are the grid's y)
    const int rc = work.reserve(c, (head + G * wcol) * 8);
    if (rc) return rc;
    double* d_L = work.as<double>();
    double* d_basis = d_L + Q * P;
    double* d_hess = d_L + head;
    double* d_A = d_hess + G * PP;
    double* d_ainv = d_A + G * nA;
    double* d_cov = d_ainv + G * nI;
    double* d_sigma = d_cov + G * PP;
    double* d_scale = d_sigma + G * P;
    int32_t* d_status = (int32_t*)(d_scale + G * nS);
    double* d_fs = d_scale + G * nS + G;
    if (pen) HIPCHK(hipMemcpyAsync(d_L, pen->L, Q * P * 8, hipMemcpyHostToDevice, c->stream));
    if (field_sigma) HIPCHK(hipMemcpyAsync(d_basis, basis, (size_t)P * Ns * 8, hipMemcpyHostToDevice, c->stream));
    PenaltyParams a{};                // A = hess + L^T L: the hess entries of k_regular_penalty on a copy
    a.P = P; a.Q = (int32_t)Q; a.e0 = 0; a.ne = P * (P + 1) / 2;
    a.L = d_L; a.hess = d_A;
    CovParams v{};
    v.P = P; v.sandwich = pen ? 1 : 0;
    v.A = pen ? d_A : d_hess; v.hess = d_hess; v.scale = scale ? d_scale : nullptr;
    v.ainv = ainv ? d_ainv : nullptr; v.cov = d_cov; v.sigma = d_sigma; v.status = d_status;
    BandParams b{};
    b.P = P; b.Ns = Nspace; b.npar = npar;
    for (int q = 0; q < npar; ++q) {
        b.nn[q] = nnode[q];
        b.row0[q] = q ? b.row0[q - 1] + nnode[q - 1] : 0;
    }
    b.cov = d_cov; b.basis = d_basis; b.status = d_status; b.out = d_fs;
    for (size_t g0 = 0; g0 < NC; g0 += G) {
        const size_t ng = std::min(G, NC - g0);
        HIPCHK(hipMemcpyAsync(d_hess, hess + g0 * PP, ng * PP * 8, hipMemcpyHostToDevice, c->stream));
        if (scale) HIPCHK(hipMemcpyAsync(d_scale, scale + g0, ng * 8, hipMemcpyHostToDevice, c->stream));
        if (pen) {
            HIPCHK(hipMemcpyAsync(d_A, d_hess, ng * PP * 8, hipMemcpyDeviceToDevice, c->stream));
            hipLaunchKernelGGL(k_regular_penalty, dim3((unsigned)ng), dim3(kPenaltyLanes), 0, c->stream, a);
        }
        hipLaunchKernelGGL(k_regular_covariance, dim3((unsigned)ng), dim3(64), 0, c->stream, v);
        if (field_sigma)
            hipLaunchKernelGGL(k_regular_band, dim3((unsigned)((Ns + 63) / 64), (unsigned)ng, (unsigned)npar), dim3(64), 0, c->stream, b);
        HIPCHK(hipGetLastError());
        if (ainv) HIPCHK(hipMemcpyAsync(ainv + g0 * PP, d_ainv, ng * PP * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(cov + g0 * PP, d_cov, ng * PP * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(sigma + g0 * P, d_sigma, ng * P * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status + g0, d_status, ng * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        if (field_sigma) HIPCHK(hipMemcpyAsync(field_sigma + g0 * nF, d_fs, ng * nF * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next group
    }
    return LSX_OK;
}
