// lsx_timedep_dev.h -- one implicit step of the rate equation dn/dt = Gamma n at one (column, depth) point of one atom
// (include/lsx_hip_timedep.h: the scheme), as __host__ __device__ functions that a host compiler also accepts (lsx_timedep.hip
// runs them on the device, one thread per point; lsx_timedep_host.cpp on the CPU for the tests).
//
//   iE            the first maximum of the current iterate n
//   row i != iE   A[i][j] = delta_ij - dt Gamma[i][j] (ONE rounding: fma),  b[i] = n_prev[i]
//   row iE        ones,  b[iE] = n_prev[0] + n_prev[1] + ... (plain adds, ascending)
//   A x = b       dense LU with partial pivoting in the operation order of LAPACK dgetf2 / dgetrs -- the elimination of
//                 k_stat_equil / k_stat_equil_reg (lsx_hip.hip), statement for statement
//   n <- x,       change = max_i |1 - n_old[i] / x[i]| (NaN if any term is)
// Two forms of the same operations in the same order, so that they give the same bits: solve_reg<NL> keeps the system in
// registers (NL a compile-time constant, every loop unrolled, the data-dependent row choices predicated selects), solve_mem keeps
// it in work arrays of a given stride (the device: thread-private LDS columns).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LSXTD_HD __host__ __device__ inline
#define LSXTD_UNROLL _Pragma("unroll")
#else
#define LSXTD_HD inline
#define LSXTD_UNROLL
#endif

namespace lsxtd {

// doubles of work space solve_mem needs per point: the matrix, the right-hand side, the iterate the call started from
LSXTD_HD size_t work_doubles(int Nl) { return (size_t)Nl * Nl + 2 * (size_t)Nl; }

LSXTD_HD double nan_max(double mx, double ch)       // change.max(): NaN wins inside one point
{
    return (ch != ch || mx != mx) ? (double)NAN : fmax(mx, ch);
}

// G[(i * NL + j) * s]: Gamma[i][j] of the point; np[l * s]: n_prev; nk[l * s]: the iterate, overwritten with the solution unless
// the system is singular (or holds a NaN where the pivot search meets it).  -> false: singular, nothing written.
template <int NL>
LSXTD_HD bool solve_reg(const double* G, const double* np, double* nk, size_t s, double dt, double* change)
{
    double a[NL][NL], b[NL], nOld[NL];           // a[i][j]: row i, column j

    int iE = 0;
    double nmax = nk[0];
    LSXTD_UNROLL
    for (int l = 0; l < NL; ++l) {
        nOld[l] = nk[(size_t)l * s];
        if (nOld[l] > nmax) { nmax = nOld[l]; iE = l; }      // np.argmax: first maximum
    }
    double ntot = np[0];
    b[0] = ntot;
    LSXTD_UNROLL
    for (int l = 1; l < NL; ++l) {
        b[l] = np[(size_t)l * s];
        ntot += b[l];
    }
    LSXTD_UNROLL
    for (int i = 0; i < NL; ++i) {
        LSXTD_UNROLL
        for (int j = 0; j < NL; ++j) {
            const double g = G[(size_t)(i * NL + j) * s];
            a[i][j] = (i == iE) ? 1.0 : fma(-dt, g, i == j ? 1.0 : 0.0);
        }
        b[i] = (i == iE) ? ntot : b[i];
    }
    bool sing = false;
    LSXTD_UNROLL
    for (int j = 0; j < NL; ++j) {
        int pv = j;
        double amax = fabs(a[j][j]), apv = a[j][j];
        LSXTD_UNROLL
        for (int i = j + 1; i < NL; ++i) {
            const double v = fabs(a[i][j]);
            if (v > amax) { amax = v; pv = i; apv = a[i][j]; }
        }
        if (!sing && (apv == 0.0 || amax != amax)) sing = true;
        LSXTD_UNROLL
        for (int r = j + 1; r < NL; ++r) {
            const bool sw = r == pv;
            LSXTD_UNROLL
            for (int q = 0; q < NL; ++q) {
                const double t = a[j][q];
                a[j][q] = sw ? a[r][q] : t;
                a[r][q] = sw ? t : a[r][q];
            }
            const double t = b[j];
            b[j] = sw ? b[r] : t;
            b[r] = sw ? t : b[r];
        }
        const double rr = 1.0 / a[j][j];
        LSXTD_UNROLL
        for (int i = j + 1; i < NL; ++i) a[i][j] *= rr;
        LSXTD_UNROLL
        for (int q = j + 1; q < NL; ++q) {
            const double ajq = a[j][q];
            LSXTD_UNROLL
            for (int i = j + 1; i < NL; ++i) a[i][q] -= a[i][j] * ajq;
        }
    }
    if (sing) return false;
    LSXTD_UNROLL
    for (int j = 0; j < NL; ++j) {
        LSXTD_UNROLL
        for (int i = j + 1; i < NL; ++i) b[i] -= a[i][j] * b[j];
    }
    LSXTD_UNROLL
    for (int j = NL - 1; j >= 0; --j) {
        b[j] /= a[j][j];
        LSXTD_UNROLL
        for (int i = 0; i < j; ++i) b[i] -= a[i][j] * b[j];
    }
    double mx = 0.0;
    LSXTD_UNROLL
    for (int i = 0; i < NL; ++i) {
        mx = nan_max(mx, fabs(1.0 - nOld[i] / b[i]));
        nk[(size_t)i * s] = b[i];
    }
    *change = mx;
    return true;
}

// The same with the system in memory: w holds work_doubles(Nl) entries `ws` apart (A[(i + j Nl) ws], column-major, then b, then
// the iterate the call started from).
LSXTD_HD bool solve_mem(int Nl, double* w, size_t ws, const double* G, const double* np, double* nk, size_t s, double dt,
                        double* change)
{
    double* A = w;
    double* b = w + (size_t)Nl * Nl * ws;
    double* nOld = b + (size_t)Nl * ws;

    int iE = 0;
    double nmax = nk[0];
    for (int l = 0; l < Nl; ++l) {
        const double v = nk[(size_t)l * s];
        nOld[l * ws] = v;
        if (v > nmax) { nmax = v; iE = l; }      // np.argmax: first maximum
    }
    double ntot = np[0];
    b[0] = ntot;
    for (int l = 1; l < Nl; ++l) {
        const double v = np[(size_t)l * s];
        b[l * ws] = v;
        ntot += v;
    }
    for (int i = 0; i < Nl; ++i)
        for (int j = 0; j < Nl; ++j)
            A[(i + j * Nl) * ws] = (i == iE) ? 1.0 : fma(-dt, G[(size_t)(i * Nl + j) * s], i == j ? 1.0 : 0.0);
    b[iE * ws] = ntot;

    for (int j = 0; j < Nl; ++j) {
        int pv = j;
        double amax = fabs(A[(j + j * Nl) * ws]);
        for (int i = j + 1; i < Nl; ++i) {
            const double v = fabs(A[(i + j * Nl) * ws]);
            if (v > amax) { amax = v; pv = i; }
        }
        if (A[(pv + j * Nl) * ws] == 0.0 || amax != amax) return false;
        if (pv != j) {
            for (int q = 0; q < Nl; ++q) {
                const double t = A[(j + q * Nl) * ws];
                A[(j + q * Nl) * ws] = A[(pv + q * Nl) * ws];
                A[(pv + q * Nl) * ws] = t;
            }
            const double t = b[j * ws]; b[j * ws] = b[pv * ws]; b[pv * ws] = t;
        }
        const double r = 1.0 / A[(j + j * Nl) * ws];
        for (int i = j + 1; i < Nl; ++i) A[(i + j * Nl) * ws] *= r;
        for (int q = j + 1; q < Nl; ++q) {
            const double ajq = A[(j + q * Nl) * ws];
            for (int i = j + 1; i < Nl; ++i) A[(i + q * Nl) * ws] -= A[(i + j * Nl) * ws] * ajq;
        }
    }
    for (int j = 0; j < Nl; ++j)
        for (int i = j + 1; i < Nl; ++i) b[i * ws] -= A[(i + j * Nl) * ws] * b[j * ws];
    for (int j = Nl - 1; j >= 0; --j) {
        b[j * ws] /= A[(j + j * Nl) * ws];
        for (int i = 0; i < j; ++i) b[i * ws] -= A[(i + j * Nl) * ws] * b[j * ws];
    }
    double mx = 0.0;
    for (int i = 0; i < Nl; ++i) {
        const double nn = b[i * ws];
        mx = nan_max(mx, fabs(1.0 - nOld[i * ws] / nn));
        nk[(size_t)i * s] = nn;
    }
    *change = mx;
    return true;
}

} // namespace lsxtd
