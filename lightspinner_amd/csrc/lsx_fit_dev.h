// lsx_fit_dev.h -- the arithmetic of the field fit (include/lsx_hip_fit.h) as __host__ __device__ functions that a host
// compiler also accepts: lsx_fit.hip runs them in its kernels, lsx_fit_host.cpp on arrays handed over (tests, the sanitizer program).
//   expand        the field of a column from its nodes
//   contract      a row of the Jacobian at one data point: the response summed over depth against a basis row
//   smear         an observed point of the instrument: a pixel's weights against the grid points it reads
//   residual      the weight and the residual of a data point
//   lane_sum      a lane's part of a sum over the data points, tree_step one level of the tree that joins the kReduceLanes parts
//   entry_pair    which sum an entry of the reduction is
//   step_solve    the damped step: Cholesky factorisation of A = hess + lambda diag(hess) in packed storage, two triangular solves
//   step_finish   the clamped trial nodes and the decrease the linear model predicts
// Every sum runs in one fixed order that depends on the sizes alone.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LSXFIT_HD __host__ __device__ __forceinline__
#else
#define LSXFIT_HD inline
#endif

namespace lsxfit {

constexpr int kMaxParams = 24;          // LSX_FIT_MAX_PARAMS
constexpr int kReduceLanes = 256;       // the lanes that share one sum over the data points

// field_p[k] = base + sum_n x[n] basis[n][k], n ascending; basis: the parameter's rows, Ns apart
LSXFIT_HD double expand(double base, int nn, const double* x, const double* basis, size_t Ns, size_t k)
{
    double f = base;
    for (int n = 0; n < nn; ++n) f += x[n] * basis[(size_t)n * Ns + k];
    return f;
}

// J = sum_k rf[k stride] basis[k], k ascending
template <class PB>
LSXFIT_HD double contract(const double* rf, size_t stride, PB basis, int Ns)
{
    double j = 0.0;
    for (int k = 0; k < Ns; ++k) j += rf[(size_t)k * stride] * basis[k];
    return j;
}

// an observed point of the instrument (lsx_fit_instrument): sum_i weight[i] x[i stride], i ascending from 0.0; weight: the pixel's row,
// x: the first grid point the pixel reads
template <class PW>
LSXFIT_HD double smear(PW weight, int width, const double* x, size_t stride)
{
    double s = 0.0;
    for (int i = 0; i < width; ++i) s += weight[i] * x[(size_t)i * stride];
    return s;
}

// the weight (null: 1) and the residual of a data point; a point of weight zero has residual zero: its obs does not enter
LSXFIT_HD void residual(const double* weight, const double* obs, const double* S, size_t d, double& w, double& r)
{
    w = weight ? weight[d] : 1.0;
    r = w > 0.0 ? obs[d] - S[d] : 0.0;
}

// a lane's part of sum_d w x y: the points lane, lane + kReduceLanes, ...
template <class PW, class PX, class PY>
LSXFIT_HD double lane_sum(int lane, int M, PW w, PX x, PY y)
{
    double a = 0.0;
    for (int d = lane; d < M; d += kReduceLanes) a += (w[d] * x[d]) * y[d];
    return a;
}

// one level of the tree over v[kReduceLanes]: s = kReduceLanes / 2, ..., 1; the lanes below s take part
template <class PV>
LSXFIT_HD void tree_step(PV v, int lane, int s)
{
    v[lane] += v[lane + s];
}

// the entries of a column's reduction, P (P + 1) / 2 + P + 1 of them: first hess (a, b), b <= a, row by row; then grad a (b = -1);
// last chi2 (a = b = -1)
LSXFIT_HD int entries(int P) { return P * (P + 1) / 2 + P + 1; }
LSXFIT_HD void entry_pair(int P, int e, int& a, int& b)
{
    const int nh = P * (P + 1) / 2;
    if (e >= nh) {
        a = e - nh < P ? e - nh : -1;
        b = -1;
        return;
    }
    a = 0;
    while ((a + 1) * (a + 2) / 2 <= e) ++a;
    b = e - a * (a + 1) / 2;
}

// ---- the damped step ----
// doubles of work space per column: the packed lower triangle and the right-hand side
LSXFIT_HD size_t step_doubles(int P) { return (size_t)P * (P + 1) / 2 + (size_t)P; }
LSXFIT_HD size_t tri(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }          // j <= i

// A = hess + lambda diag(hess) (hess [P][P], its lower triangle is read), A = L L^T, L y = grad, L^T delta = y.  w: the work space,
// element e at w[e ws].  -> 0 and delta in the work space's last P elements, or 1 where a pivot is not positive or not a number
template <class PW>
LSXFIT_HD int step_solve(int P, const double* hess, const double* grad, double lambda, PW w, size_t ws)
{
    const size_t rhs = (size_t)P * (P + 1) / 2;
    for (int i = 0; i < P; ++i) {
        for (int j = 0; j < i; ++j) w[tri(i, j) * ws] = hess[(size_t)i * P + j];
        const double h = hess[(size_t)i * P + i];
        w[tri(i, i) * ws] = h + lambda * h;
        w[(rhs + i) * ws] = grad[i];
    }
    for (int j = 0; j < P; ++j) {
        double d = w[tri(j, j) * ws];
        for (int k = 0; k < j; ++k) d -= w[tri(j, k) * ws] * w[tri(j, k) * ws];
        if (!(d > 0.0) || !(d < INFINITY)) return 1;
        const double l = sqrt(d);
        w[tri(j, j) * ws] = l;
        for (int i = j + 1; i < P; ++i) {
            double s = w[tri(i, j) * ws];
            for (int k = 0; k < j; ++k) s -= w[tri(i, k) * ws] * w[tri(j, k) * ws];
            w[tri(i, j) * ws] = s / l;
        }
    }
    for (int i = 0; i < P; ++i) {
        double s = w[(rhs + i) * ws];
        for (int k = 0; k < i; ++k) s -= w[tri(i, k) * ws] * w[(rhs + k) * ws];
        w[(rhs + i) * ws] = s / w[tri(i, i) * ws];
    }
    for (int i = P - 1; i >= 0; --i) {
        double s = w[(rhs + i) * ws];
        for (int k = i + 1; k < P; ++k) s -= w[tri(k, i) * ws] * w[(rhs + k) * ws];
        w[(rhs + i) * ws] = s / w[tri(i, i) * ws];
    }
    for (int i = 0; i < P; ++i) {
        const double x = w[(rhs + i) * ws];
        if (!(fabs(x) < INFINITY)) return 1;
    }
    return 0;
}

// trial = clamp(nodes + delta, lo, hi); predicted = 2 d.grad - d.hess d for d = trial - nodes.  status != 0: trial = nodes, predicted = 0.
// w: where step_solve left delta (the work space from element P (P + 1) / 2 on), element e at w[e ws]; d takes its place
template <class PW>
LSXFIT_HD double step_finish(int P, int status, const double* hess, const double* grad, const double* nodes, const double* lo,
                             const double* hi, PW w, size_t ws, double* trial)
{
    if (status) {
        for (int i = 0; i < P; ++i) trial[i] = nodes[i];
        return 0.0;
    }
    for (int i = 0; i < P; ++i) {
        double t = nodes[i] + w[(size_t)i * ws];
        t = t < lo[i] ? lo[i] : t;
        t = t > hi[i] ? hi[i] : t;
        trial[i] = t;
        w[(size_t)i * ws] = t - nodes[i];
    }
    double dg = 0.0, dHd = 0.0;
    for (int i = 0; i < P; ++i) {
        double hd = 0.0;
        for (int j = 0; j < P; ++j) hd += hess[(size_t)i * P + j] * w[(size_t)j * ws];
        dg += w[(size_t)i * ws] * grad[i];
        dHd += w[(size_t)i * ws] * hd;
    }
    return 2.0 * dg - dHd;
}

} // namespace lsxfit
