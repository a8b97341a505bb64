// lsx_solve_dev.h -- the dense solve that turns Gamma into populations at one (column, depth) point of one atom, once for the
// statistical equilibrium (rh_method.py:710-745) and the implicit step of the rate equation dn/dt = Gamma n
// (include/lsx_hip_timedep.h: the scheme), as __host__ __device__ functions that a host compiler also accepts (lsx_hip.hip and
// lsx_timedep.hip run them on the device, one thread per point; lsx_timedep_host.cpp on the CPU for the tests).
//
//   iE            the first maximum of the current iterate n
//   row i != iE   A[i][j] = System::coef(Gamma[i][j], i == j),  b[i] = System::rhs(i)
//   row iE        ones,  b[iE] = System::rhs_replaced(Nl)
//   A x = b       dense LU with partial pivoting in the operation order of LAPACK dgetf2 / dgetrs
//   n <- x,       change = max_i |1 - n_old[i] / x[i]| (NaN if any term is)
//
//                 coef(g, diagonal)                 rhs(i)       rhs_replaced(Nl)
//   StatEquil     g                                 0            nTotal
//   TimeStep      delta_ij - dt g (ONE rounding)    n_prev[i]    n_prev[0] + n_prev[1] + ... (plain adds, ascending)
//
// Two forms of the same operations in the same order, so that they give the same bits: solve_reg<NL> keeps the system in
// registers (NL a compile-time constant, every loop unrolled, the data-dependent row choices predicated selects), solve_mem keeps
// it in work arrays of a given stride (the device: thread-private LDS columns) and swaps rows for real.  On the device
// solve_reg<NL>(StatEquil) is written out once more, in k_stat_equil_reg (lsx_hip.hip, which says why): a change here is made there too.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#if defined(__HIPCC__)
#define LSXSOLVE_HD __host__ __device__ __forceinline__
#define LSXSOLVE_UNROLL _Pragma("unroll")
#else
#define LSXSOLVE_HD inline
#define LSXSOLVE_UNROLL
#endif

namespace lsxsolve {

struct StatEquil {
    const double* ntot;             // the point's nTotal, read where the right-hand side is assembled
    LSXSOLVE_HD double coef(double g, bool) const { return g; }
    LSXSOLVE_HD double rhs(int) const { return 0.0; }
    LSXSOLVE_HD double rhs_replaced(int) const { return *ntot; }
};

struct TimeStep {
    double dt;
    const double* n_prev;           // n_prev[l * stride]
    int stride;
    LSXSOLVE_HD double coef(double g, bool diagonal) const { return fma(-dt, g, diagonal ? 1.0 : 0.0); }
    LSXSOLVE_HD double rhs(int i) const { return n_prev[(size_t)i * stride]; }
    LSXSOLVE_HD double rhs_replaced(int Nl) const
    {
        double sum = n_prev[0];
        LSXSOLVE_UNROLL
        for (int l = 1; l < Nl; ++l) sum += n_prev[(size_t)l * stride];
        return sum;
    }
};

// doubles of work space solve_mem needs per point: the matrix, the right-hand side, the iterate the call started from
LSXSOLVE_HD size_t work_doubles(int Nl) { return (size_t)Nl * Nl + 2 * (size_t)Nl; }

LSXSOLVE_HD double nan_max(double mx, double ch)       // change.max(): NaN wins inside one point
{
    return (ch != ch || mx != mx) ? (double)NAN : fmax(mx, ch);
}

// the level counts that have a register instance, and f(std::integral_constant<int, Nl>()) for one of them
inline bool has_register_form(int Nl) { return Nl >= 2 && Nl <= 8; }
template <class F>
inline void with_register_form(int Nl, F&& f)
{
    switch (Nl) {
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: f(std::integral_constant<int, 4>()); break;
    case 5: f(std::integral_constant<int, 5>()); break;
    case 6: f(std::integral_constant<int, 6>()); break;
    case 7: f(std::integral_constant<int, 7>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    }
}

// G[(i * NL + j) * s]: Gamma[i][j] of the point; nk[l * s]: the iterate, overwritten with the solution unless the system is
// singular (or holds a NaN where the pivot search meets it).  -> false: singular, nothing written.
template <int NL, class System>
LSXSOLVE_HD bool solve_reg(const System sys, const double* __restrict__ G, double* __restrict__ nk, int s, double* change)
{
    double a[NL][NL], b[NL], nOld[NL];           // a[i][j]: row i, column j

    int iE = 0;
    double nmax = nk[0];
    LSXSOLVE_UNROLL
    for (int l = 0; l < NL; ++l) {
        nOld[l] = nk[(size_t)l * s];
        if (nOld[l] > nmax) { nmax = nOld[l]; iE = l; }      // np.argmax: first maximum
    }
    const double bE = sys.rhs_replaced(NL);
    LSXSOLVE_UNROLL
    for (int i = 0; i < NL; ++i) {
        LSXSOLVE_UNROLL
        for (int j = 0; j < NL; ++j) {
            const double c = sys.coef(G[(size_t)(i * NL + j) * s], i == j);     // (read in every row: a select, no branch)
            a[i][j] = (i == iE) ? 1.0 : c;
        }
        const double r = sys.rhs(i);
        b[i] = (i == iE) ? bE : r;
    }
    bool sing = false;
    LSXSOLVE_UNROLL
    for (int j = 0; j < NL; ++j) {
        int pv = j;
        double amax = fabs(a[j][j]), apv = a[j][j];
        LSXSOLVE_UNROLL
        for (int i = j + 1; i < NL; ++i) {
            const double v = fabs(a[i][j]);
            if (v > amax) { amax = v; pv = i; apv = a[i][j]; }
        }
        if (!sing && (apv == 0.0 || amax != amax)) sing = true;
        LSXSOLVE_UNROLL
        for (int r = j + 1; r < NL; ++r) {
            const bool sw = r == pv;
            LSXSOLVE_UNROLL
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
        LSXSOLVE_UNROLL
        for (int i = j + 1; i < NL; ++i) a[i][j] *= rr;
        LSXSOLVE_UNROLL
        for (int q = j + 1; q < NL; ++q) {
            const double ajq = a[j][q];
            LSXSOLVE_UNROLL
            for (int i = j + 1; i < NL; ++i) a[i][q] -= a[i][j] * ajq;
        }
    }
    if (sing) return false;
    LSXSOLVE_UNROLL
    for (int j = 0; j < NL; ++j) {
        LSXSOLVE_UNROLL
        for (int i = j + 1; i < NL; ++i) b[i] -= a[i][j] * b[j];
    }
    LSXSOLVE_UNROLL
    for (int j = NL - 1; j >= 0; --j) {
        b[j] /= a[j][j];
        LSXSOLVE_UNROLL
        for (int i = 0; i < j; ++i) b[i] -= a[i][j] * b[j];
    }
    double mx = 0.0;
    LSXSOLVE_UNROLL
    for (int i = 0; i < NL; ++i) {
        mx = nan_max(mx, fabs(1.0 - nOld[i] / b[i]));
        nk[(size_t)i * s] = b[i];
    }
    *change = mx;
    return true;
}

// The same with the system in memory: w holds work_doubles(Nl) entries `ws` apart (A[(i + j Nl) ws], column-major, then b, then
// the iterate the call started from).
template <class System>
LSXSOLVE_HD bool solve_mem(const System sys, int Nl, double* w, int ws, const double* G, double* nk, int s, double* change)
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
    for (int i = 0; i < Nl; ++i)
        for (int j = 0; j < Nl; ++j) A[(i + j * Nl) * ws] = (i == iE) ? 1.0 : sys.coef(G[(size_t)(i * Nl + j) * s], i == j);
    for (int i = 0; i < Nl; ++i) b[i * ws] = sys.rhs(i);
    b[iE * ws] = sys.rhs_replaced(Nl);

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

} // namespace lsxsolve
