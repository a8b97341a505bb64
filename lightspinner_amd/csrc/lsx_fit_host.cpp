// lsx_fit_host.cpp -- the arithmetic of lsx_fit_dev.h compiled for the CPU, on arrays handed over (tests and the sanitizer program only:
// `make fithost`, `make fitsan`, `make fitinstsan`).  What lsx_fit.hip does in k_fit_jac, k_fit_reduce and k_fit_step and
// lsx_fit_instrument.hip in k_fit_smear, in the kernels' order: the same lanes' parts, the same tree.  Built with -ffp-contract=off.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lsx_hip_fit.h"
#include "lsx_fit_dev.h"

using namespace lsxfit;

namespace {

// nq: the quantities of the parameterisation, 3 (B, gammaB, chiB) or 4 (with vlos: include/lsx_hip_stokes_velocity.h)
int count_params(const int32_t* nnode, int nq = 3)
{
    if (!nnode) return -1;
    int64_t P = 0;
    for (int a = 0; a < nq; ++a) {
        if (nnode[a] < 0) return -1;
        P += nnode[a];
    }
    return P >= 1 && P <= LSX_FIT_MAX_PARAMS ? (int)P : -1;
}

// sum_d w x y as a block of k_fit_reduce forms it
double block_sum(int M, const double* w, const double* x, const double* y)
{
    double v[kReduceLanes];
    for (int lane = 0; lane < kReduceLanes; ++lane) v[lane] = lane_sum(lane, M, w, x, y);
    for (int s = kReduceLanes / 2; s > 0; s >>= 1)
        for (int lane = 0; lane < s; ++lane) tree_step(v, lane, s);
    return v[0];
}

// the instrument's rules (include/lsx_hip_fit_instrument.h)
bool instrument_ok(int32_t nla, int32_t nobs, int32_t width, const int32_t* first, const double* iweight)
{
    if (!first || !iweight || nobs < 1 || width < 1 || width > nla) return false;
    for (int o = 0; o < nobs; ++o)
        if (first[o] < 0 || first[o] > nla - width) return false;
    for (size_t i = 0; i < (size_t)nobs * width; ++i)
        if (!std::isfinite(iweight[i])) return false;
    return true;
}

// a row of ns blocks [nla][nmu] -> ns blocks [nobs][nmu], point by point as a lane of k_fit_smear forms it
void smear_row(int ns, int nla, int nmu, int nobs, int width, const int32_t* first, const double* iweight, const double* in, double* out)
{
    for (int d = 0; d < ns * nobs * nmu; ++d) {
        const int so = d / nmu, m = d - so * nmu;
        const int s = so / nobs, o = so - s * nobs;
        out[d] = smear(iweight + (size_t)o * width, width, in + ((size_t)s * nla + first[o]) * nmu + m, (size_t)nmu);
    }
}

// the sums of one column; first null: no instrument
int normal_run(int nq, int32_t Ns, int32_t nla, int32_t nmu, const int32_t* nnode, const double* rf, const double* S, const double* obs,
               const double* weight, const double* basis, int32_t nobs, int32_t width, const int32_t* first, const double* iweight,
               double* chi2, double* grad, double* hess)
{
    const int P = count_params(nnode, nq);
    const bool normal = grad || hess;
    if (P < 0 || Ns < 1 || nla < 1 || nmu < 1 || !S || !obs || !chi2 || (normal && (!grad || !hess || !rf || !basis))) return LSX_EINVAL;
    if (first && !instrument_ok(nla, nobs, width, first, iweight)) return LSX_EINVAL;
    const int Mg = 4 * nla * nmu, M = first ? 4 * nobs * nmu : Mg;
    std::vector<double> W((size_t)M), R((size_t)M), J(normal ? (size_t)P * Mg : 0), Ss, Js;
    if (first) {
        Ss.resize((size_t)M);
        smear_row(4, nla, nmu, nobs, width, first, iweight, S, Ss.data());
        S = Ss.data();
    }
    for (int d = 0; d < M; ++d) residual(weight, obs, S, (size_t)d, W[d], R[d]);
    *chi2 = block_sum(M, W.data(), R.data(), R.data());
    if (!normal) return LSX_OK;
    const size_t block = (size_t)Ns * nmu;
    for (int a = 0, i = 0, j = 0; a < nq; ++a) {
        for (int n = 0; n < nnode[a]; ++n, ++j)
            for (int d = 0; d < Mg; ++d) {
                const int sl = d / nmu, m = d - sl * nmu;
                J[(size_t)j * Mg + d] = contract(rf + (size_t)i * 4 * nla * block + (size_t)sl * block + m, (size_t)nmu, basis + (size_t)j * Ns, Ns);
            }
        i += nnode[a] > 0;
    }
    const double* Jr = J.data();
    if (first) {
        Js.resize((size_t)P * M);
        for (int j = 0; j < P; ++j) smear_row(4, nla, nmu, nobs, width, first, iweight, J.data() + (size_t)j * Mg, Js.data() + (size_t)j * M);
        Jr = Js.data();
    }
    for (int e = 0; e < entries(P) - 1; ++e) {
        int a, b;
        entry_pair(P, e, a, b);
        const double sum = block_sum(M, W.data(), Jr + (size_t)a * M, b >= 0 ? Jr + (size_t)b * M : R.data());
        if (b >= 0) hess[(size_t)a * P + b] = hess[(size_t)b * P + a] = sum;
        else grad[a] = sum;
    }
    return LSX_OK;
}

} // namespace

extern "C" {

static int expand_run(int nq, int32_t Ns, int32_t ncol, const int32_t* nnode, const double* basis, const double* base, const double* nodes,
                      double* field)
{
    const int P = count_params(nnode, nq);
    if (P < 0 || Ns < 1 || ncol < 1 || !basis || !nodes || !field) return LSX_EINVAL;
    int row0[4] = {0, 0, 0, 0};
    for (int a = 1; a < nq; ++a) row0[a] = row0[a - 1] + nnode[a - 1];
    for (size_t q = 0; q < (size_t)ncol; ++q)
        for (int a = 0; a < nq; ++a)
            for (int k = 0; k < Ns; ++k)
                field[(q * nq + a) * Ns + k] = expand(base ? base[(q * nq + a) * Ns + k] : 0.0, nnode[a], nodes + q * P + row0[a],
                                                      basis + (size_t)row0[a] * Ns, (size_t)Ns, (size_t)k);
    return LSX_OK;
}

// the field of ncol columns from their nodes: basis [P][Ns], base [ncol][3][Ns] or null, nodes [ncol][P] -> field [ncol][3][Ns]
int lsx_fit_host_expand(int32_t Ns, int32_t ncol, const int32_t* nnode, const double* basis, const double* base, const double* nodes,
                        double* field)
{
    return expand_run(3, Ns, ncol, nnode, basis, base, nodes, field);
}

// ... with four quantities (include/lsx_hip_stokes_velocity.h): nnode[4], base and field [ncol][4][Ns], the velocity the fourth row
int lsx_fit_host_expand4(int32_t Ns, int32_t ncol, const int32_t* nnode, const double* basis, const double* base, const double* nodes,
                         double* field)
{
    return expand_run(4, Ns, ncol, nnode, basis, base, nodes, field);
}

// One column's sums from its response and its Stokes vector: rf [npar][4][nla][Ns][nmu] (npar: the parameters with nodes, in the order
// B, gammaB, chiB), S, obs, weight (or null) [4][nla][nmu], basis [P][Ns] -> chi2 [1], grad [P], hess [P][P].  grad and hess null
// (then rf may be null too): chi2 alone.
int lsx_fit_host_normal(int32_t Ns, int32_t nla, int32_t nmu, const int32_t* nnode, const double* rf, const double* S, const double* obs,
                        const double* weight, const double* basis, double* chi2, double* grad, double* hess)
{
    return normal_run(3, Ns, nla, nmu, nnode, rf, S, obs, weight, basis, 0, 0, nullptr, nullptr, chi2, grad, hess);
}

// lsx_fit_host_normal_inst with four quantities: nnode[4], rf [npar][4][nla][Ns][nmu] in the order B, gammaB, chiB, vlos.  first null
// (then iweight must be null too): no instrument
int lsx_fit_host_normal4(int32_t Ns, int32_t nla, int32_t nmu, const int32_t* nnode, const double* rf, const double* S,
                         const double* obs, const double* weight, const double* basis, int32_t nobs, int32_t width,
                         const int32_t* first, const double* iweight, double* chi2, double* grad, double* hess)
{
    if (!first && iweight) return LSX_EINVAL;
    return normal_run(4, Ns, nla, nmu, nnode, rf, S, obs, weight, basis, nobs, width, first, iweight, chi2, grad, hess);
}

// the instrument on arrays handed over: in [nrow][nla][nmu] -> out [nrow][nobs][nmu]; first [nobs], iweight [nobs][width]
int lsx_fit_host_smear(int32_t nla, int32_t nmu, int32_t nrow, int32_t nobs, int32_t width, const int32_t* first, const double* iweight,
                       const double* in, double* out)
{
    if (nla < 1 || nmu < 1 || nrow < 1 || !in || !out || !instrument_ok(nla, nobs, width, first, iweight)) return LSX_EINVAL;
    for (size_t r = 0; r < (size_t)nrow; ++r)
        smear_row(1, nla, nmu, nobs, width, first, iweight, in + r * nla * nmu, out + r * nobs * nmu);
    return LSX_OK;
}

// lsx_fit_host_normal through an instrument: obs, weight [4][nobs][nmu]; S and rf on the window's grid as there.  first null: that one.
int lsx_fit_host_normal_inst(int32_t Ns, int32_t nla, int32_t nmu, const int32_t* nnode, const double* rf, const double* S,
                             const double* obs, const double* weight, const double* basis, int32_t nobs, int32_t width,
                             const int32_t* first, const double* iweight, double* chi2, double* grad, double* hess)
{
    if (!first && iweight) return LSX_EINVAL;
    return normal_run(3, Ns, nla, nmu, nnode, rf, S, obs, weight, basis, nobs, width, first, iweight, chi2, grad, hess);
}

// lsx_hip_fit_field_step on the CPU; delta [ncol][P] (may be null): the unclamped solution (NaN where status is 1)
int lsx_fit_host_step(int32_t ncol, int32_t P, const double* hess, const double* grad, const double* lambda, const double* nodes,
                      const double* lo, const double* hi, double* trial, double* predicted, int32_t* status, double* delta)
{
    if (ncol < 1 || P < 1 || P > LSX_FIT_MAX_PARAMS || !hess || !grad || !lambda || !nodes || !lo || !hi || !trial || !predicted || !status)
        return LSX_EINVAL;
    std::vector<double> w(step_doubles(P));
    double* const d = w.data() + (size_t)P * (P + 1) / 2;
    for (size_t c = 0; c < (size_t)ncol; ++c) {
        const double* H = hess + c * P * P;
        const int st = step_solve(P, H, grad + c * P, lambda[c], w.data(), 1);
        for (int i = 0; i < P && delta; ++i) delta[c * P + i] = st ? NAN : d[i];
        predicted[c] = step_finish(P, st, H, grad + c * P, nodes + c * P, lo, hi, d, 1, trial + c * P);
        status[c] = st;
    }
    return LSX_OK;
}

} // extern "C"
