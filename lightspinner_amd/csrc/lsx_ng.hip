// lsx_ng.hip -- Ng acceleration of the MALI loop: extrapolation of the populations, per column, on the device
// (include/lsx_hip_ng.h: the scheme, lsx_hip_ng_configure, lsx_hip_ng_state).  Off unless configured; gfx950 only.
//
// k_ng_step runs behind the kernels of every statistical equilibrium (lsx_stat_equil_async), one workgroup of 256 threads per
// column; the workgroup walks the column's atoms itself, so everything the column owns has one writer and no atomics are needed.
//   phase 1  the populations the solve has just written -> history slot `counter`: thread t copies elements t, t + 256, ... of the
//            column's NLtot x Nspace block, so a wavefront's loads and stores are contiguous runs.  On order + 1 of every
//            order + 2 calls the workgroup ends here.
//   phase 2  per atom: every thread accumulates its elements' terms of A_ij and b_i (elements first + t, first + t + 256, ... of
//            the atom's levels x depths, in that order), the 256 partial sums are added by a tree of fixed shape in LDS
//            (128, 64, ... 1), thread 0 eliminates with partial pivoting.
//   phase 3  every thread forms its elements' candidates x_acc (all atoms) and the terms of the monitor; the workgroup agrees
//            whether all of them are finite and > 0 and every system was regular.
//   phase 4  step taken: the same threads form the same candidates again and store them over n (an element is read and
//            written by one thread only); thread 0 stores the monitor, the counters, the coefficients.
// The association of every sum is fixed by the atom's place in the column's block and the block size alone: a column's bits do
// not depend on the context's column count or on the column's index.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"

using namespace lsxd;

namespace {

constexpr int kNgThreads = 256;
constexpr int kNgMaxAtoms = 256;     // the coefficients of a column's atoms wait in LDS for the verdict of phase 3

struct NgParams {
    double* n;                      // [col][NLtot][k]
    double* hist;                   // [col][order + 2][NLtot][k]
    double* dPcol;                  // [col]: the monitor the statistical equilibrium has just written
    double* coef;                   // [col][Natoms][2]
    int32_t *cnt, *applied, *rejected;      // [col] each
    const int* off;                 // [Natoms + 1]
    const uint8_t* colmask;         // nullptr: every column is active
    int per, Natoms;                // per = NLtot * Nspace
};

// maximum of the workgroup's 256 values, the same tree for every column; the result is s[0] for every thread
__device__ __forceinline__ void tree_max(double* s, int tid)
{
    __syncthreads();
    for (int h = kNgThreads / 2; h > 0; h >>= 1) {
        if (tid < h) s[tid] = fmax(s[tid], s[tid + h]);
        __syncthreads();
    }
}

// x_acc = (1 - sum c_j) x0 + sum c_j x_j, in ONE order of operations (phases 3 and 4 must agree to the bit)
template <int ORDER>
__device__ __forceinline__ double ng_candidate(double s, double c1, double c2, double x0, double x1, double x2)
{
    if (ORDER == 1) return fma(s, x0, c1 * x1);
    return fma(s, x0, fma(c1, x1, c2 * x2));
}

template <int ORDER>
__global__ void __launch_bounds__(kNgThreads)
k_ng_step(const NgParams p)
{
    constexpr int NSLOT = ORDER + 2;
    constexpr int NSUM = ORDER == 1 ? 2 : 5;
    __shared__ double s_red[NSUM][kNgThreads];
    __shared__ double s_c[kNgMaxAtoms][2];
    __shared__ int s_regular;
    const int tid = threadIdx.x, col = blockIdx.x, per = p.per;
    if (p.colmask && !p.colmask[col]) return;           // a frozen column: neither its history nor its counter moves
    int cnt = p.cnt[col];
    __syncthreads();                                    // every thread has read the counter before thread 0 writes it
    if (cnt < 0) {                                      // the delay is still running
        if (tid == 0) p.cnt[col] = cnt + 1;
        return;
    }
    if (cnt >= NSLOT) cnt = 0;                          // (never: the counter restarts at order + 2)
    double* __restrict__ n = p.n + (size_t)col * per;
    double* __restrict__ hist = p.hist + (size_t)col * NSLOT * per;
    // ---- phase 1: store
    {
        double* __restrict__ dst = hist + (size_t)cnt * per;
        for (int e = tid; e < per; e += kNgThreads) dst[e] = n[e];
    }
    if (cnt + 1 < NSLOT) {
        if (tid == 0) p.cnt[col] = cnt + 1;
        return;
    }
    // ---- phase 2: the history is full; x0 = n (slot order + 1, just stored), x_j = slot order + 1 - j
    const double* __restrict__ h1 = hist + (size_t)(NSLOT - 2) * per;
    const double* __restrict__ h2 = hist + (size_t)(NSLOT - 3) * per;
    const double* __restrict__ h3 = hist;               // order 2 only (slot 0)
    if (tid == 0) s_regular = 1;
    for (int a = 0; a < p.Natoms; ++a) {
        const int e1 = p.off[a + 1];
        double a11 = 0.0, a12 = 0.0, a22 = 0.0, b1 = 0.0, b2 = 0.0;
        for (int e = p.off[a] + tid; e < e1; e += kNgThreads) {
            const double x0 = n[e], x1 = h1[e], x2 = h2[e];
            const double w = 1.0 / (x0 * x0);
            const double d0 = x0 - x1;
            const double D1 = d0 - (x1 - x2);
            a11 += w * D1 * D1;
            b1 += w * d0 * D1;
            if (ORDER == 2) {
                const double D2 = d0 - (x2 - h3[e]);
                a12 += w * D1 * D2;
                a22 += w * D2 * D2;
                b2 += w * d0 * D2;
            }
        }
        s_red[0][tid] = a11;
        s_red[1][tid] = b1;
        if (ORDER == 2) { s_red[2][tid] = a12; s_red[3][tid] = a22; s_red[4][tid] = b2; }
        __syncthreads();
        for (int h = kNgThreads / 2; h > 0; h >>= 1) {
            if (tid < h) {
#pragma unroll
                for (int q = 0; q < NSUM; ++q) s_red[q][tid] += s_red[q][tid + h];
            }
            __syncthreads();
        }
        if (tid == 0) {
            double c1 = 0.0, c2 = 0.0;
            bool ok;
            if (ORDER == 1) {
                const double A = s_red[0][0];
                ok = A != 0.0 && isfinite(A);
                if (ok) c1 = s_red[1][0] / A;
            } else {
                // A = (r0; r1) with A21 = A12: Gaussian elimination, the row with the larger first entry is the pivot row
                double p0 = s_red[0][0], p1 = s_red[2][0], pb = s_red[1][0];        // pivot row: A11 A12 | b1
                double q0 = s_red[2][0], q1 = s_red[3][0], qb = s_red[4][0];        // other row: A21 A22 | b2
                if (fabs(q0) > fabs(p0)) {
                    double t = p0; p0 = q0; q0 = t;
                    t = p1; p1 = q1; q1 = t;
                    t = pb; pb = qb; qb = t;
                }
                ok = p0 != 0.0 && isfinite(p0);
                if (ok) {
                    const double m = q0 / p0;
                    const double u22 = q1 - m * p1;
                    ok = u22 != 0.0 && isfinite(u22);
                    if (ok) {
                        c2 = (qb - m * pb) / u22;
                        c1 = (pb - p1 * c2) / p0;
                    }
                }
            }
            if (!(ok && isfinite(c1) && isfinite(c2))) s_regular = 0;
            s_c[a][0] = c1;
            s_c[a][1] = c2;
        }
        // (thread 0 reads s_red[.][0] only, which nobody else writes in the next round; s_c and s_regular are read behind the
        // barriers of phase 3's reduction)
    }
    __syncthreads();
    // ---- phase 3: candidates of all atoms: finite and > 0?  and the monitor max |1 - x1 / x_acc|
    double mx = 0.0, bad = 0.0;
    for (int a = 0; a < p.Natoms; ++a) {
        const double c1 = s_c[a][0], c2 = s_c[a][1];
        const double s = 1.0 - (c1 + c2);
        const int e1 = p.off[a + 1];
        for (int e = p.off[a] + tid; e < e1; e += kNgThreads) {
            const double x1 = h1[e];
            const double xa = ng_candidate<ORDER>(s, c1, c2, n[e], x1, h2[e]);
            if (!(isfinite(xa) && xa > 0.0)) bad = 1.0;
            mx = fmax(mx, fabs(1.0 - x1 / xa));
        }
    }
    s_red[0][tid] = mx;
    s_red[1][tid] = bad;
    tree_max(s_red[0], tid);
    tree_max(s_red[1], tid);
    const bool take = s_regular && s_red[1][0] == 0.0;
    if (!take) {                                        // the column keeps what the statistical equilibrium wrote
        if (tid == 0) {
            p.rejected[col] += 1;
            p.cnt[col] = 0;
        }
        return;
    }
    // ---- phase 4
    for (int a = 0; a < p.Natoms; ++a) {
        const double c1 = s_c[a][0], c2 = s_c[a][1];
        const double s = 1.0 - (c1 + c2);
        const int e1 = p.off[a + 1];
        for (int e = p.off[a] + tid; e < e1; e += kNgThreads) n[e] = ng_candidate<ORDER>(s, c1, c2, n[e], h1[e], h2[e]);
    }
    for (int a = tid; a < p.Natoms; a += kNgThreads) {
        p.coef[((size_t)col * p.Natoms + a) * 2] = s_c[a][0];
        p.coef[((size_t)col * p.Natoms + a) * 2 + 1] = s_c[a][1];
    }
    if (tid == 0) {
        p.dPcol[col] = s_red[0][0];
        p.applied[col] += 1;
        p.cnt[col] = 0;
    }
}

__global__ void __launch_bounds__(256)
k_ng_reset(int32_t* __restrict__ cnt, int ncol, int value)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < ncol) cnt[c] = value;
}

} // namespace

namespace lsxd {

void ng_free(lsx_ctx* c)
{
    for (void* p : {(void*)c->d_ng_hist, (void*)c->d_ng_state, (void*)c->d_ng_coef, (void*)c->d_ng_off})
        if (p) (void)hipFree(p);
    c->d_ng_hist = nullptr; c->d_ng_state = nullptr; c->d_ng_coef = nullptr; c->d_ng_off = nullptr;
    c->ng_order = c->ng_delay = 0;
}

int ng_reset(lsx_ctx* c, size_t col0, size_t ncol)
{
    if (!c->ng_order || ncol == 0) return LSX_OK;
    hipLaunchKernelGGL(k_ng_reset, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, c->stream, c->d_ng_state + col0, (int)ncol,
                       -c->ng_delay);
    HIPCHK(hipGetLastError());
    return LSX_OK;
}

int ng_enqueue(lsx_ctx* c)
{
    if (!c->ng_order) return LSX_OK;
    NgParams p;
    p.n = c->d_n; p.hist = c->d_ng_hist; p.dPcol = c->d_dPcol; p.coef = c->d_ng_coef;
    p.cnt = c->d_ng_state; p.applied = c->d_ng_state + c->ncol; p.rejected = c->d_ng_state + 2 * (size_t)c->ncol;
    p.off = c->d_ng_off; p.colmask = c->d_colmask; p.per = c->NLtot * c->Nspace; p.Natoms = c->Natoms;
    if (c->ng_order == 1)
        hipLaunchKernelGGL(k_ng_step<1>, dim3((unsigned)c->ncol), dim3(kNgThreads), 0, c->stream, p);
    else
        hipLaunchKernelGGL(k_ng_step<2>, dim3((unsigned)c->ncol), dim3(kNgThreads), 0, c->stream, p);
    HIPCHK(hipGetLastError());
    return LSX_OK;
}

} // namespace lsxd

extern "C" int lsx_hip_ng_configure(lsx_ctx* c, int32_t order, int32_t delay)
{
    if (!c) return fail(LSX_EINVAL, "lsx_hip_ng_configure: null context");
    if (order < 0 || order > 2) return fail(LSX_EINVAL, "lsx_hip_ng_configure: order = %d; 1 and 2 are offered, 0 switches it off", (int)order);
    if (delay < 0) return fail(LSX_EINVAL, "lsx_hip_ng_configure: delay = %d is negative", (int)delay);
    const size_t per = (size_t)c->NLtot * c->Nspace;
    if (order && (c->Natoms > kNgMaxAtoms || per > (size_t)0x7fffffff))
        return fail(LSX_EUNSUPPORTED, "lsx_hip_ng_configure: at most %d atoms and 2^31 - 1 levels x depths per column", kNgMaxAtoms);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    ng_free(c);
    if (order == 0) return LSX_OK;
    const size_t nc = (size_t)c->ncol;
    int rc;
    if ((rc = dmalloc(&c->d_ng_hist, (size_t)(order + 2) * nc * per)) || (rc = dmalloc(&c->d_ng_state, 3 * nc)) ||
        (rc = dmalloc(&c->d_ng_coef, nc * c->Natoms * 2)) || (rc = dmalloc(&c->d_ng_off, (size_t)c->Natoms + 1))) {
        ng_free(c);
        return rc;
    }
    std::vector<int> off((size_t)c->Natoms + 1);
    for (int a = 0; a < c->Natoms; ++a) off[a] = c->lev_off[a] * c->Nspace;
    off[c->Natoms] = (int)per;
    HIPCHK(hipMemcpyAsync(c->d_ng_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->d_ng_state, 0, 3 * nc * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(c->d_ng_coef, 0, nc * c->Natoms * 2 * sizeof(double), c->stream));
    c->ng_order = order;
    c->ng_delay = delay;
    if ((rc = ng_reset(c, 0, nc))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));            // (`off` is pageable host memory)
    return LSX_OK;
}

extern "C" int lsx_hip_ng_state(lsx_ctx* c, int32_t col0, int32_t ncol, int32_t* stored, int32_t* applied, int32_t* rejected, double* coef)
{
    if (!c) return fail(LSX_EINVAL, "lsx_hip_ng_state: null context");
    if (!c->ng_order) return fail(LSX_EINVAL, "lsx_hip_ng_state: Ng acceleration is off (lsx_hip_ng_configure)");
    if (col0 < 0 || ncol < 1 || (long)col0 + ncol > c->ncol)
        return fail(LSX_EINVAL, "lsx_hip_ng_state: columns [%d, %d) are outside the context's %d", (int)col0, (int)col0 + (int)ncol, c->ncol);
    HIPCHK(hipSetDevice(c->device));
    int32_t* const dst[3] = {stored, applied, rejected};
    for (int q = 0; q < 3; ++q)
        if (dst[q])
            HIPCHK(hipMemcpyAsync(dst[q], c->d_ng_state + (size_t)q * c->ncol + col0, (size_t)ncol * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (coef)
        HIPCHK(hipMemcpyAsync(coef, c->d_ng_coef + (size_t)col0 * c->Natoms * 2, (size_t)ncol * c->Natoms * 2 * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return LSX_OK;
}
