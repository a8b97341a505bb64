// lsx_background_dev.h -- every formula of the background: the Wittmann equation of state (witt.py:198-740) and the ATLAS-style
// continuous opacity (witt.py:744-1362), restated as __host__ __device__ functions that a host compiler also accepts
// (lsx_background.hip runs them on the device, lsx_background_host.cpp on the CPU for the tests).
// The reference's operation order is kept expression by expression (C and Python associate + - * / alike; build with
// -ffp-contract=off): the quadratic of pe_pg and the (BOLTEX - EXLIM) terms are differences of near-equal numbers.
// numpy's .sum() of 8..128 contiguous doubles adds in eight lanes and folds them as a tree (pairwise_sum); sum8() restates that.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LSXBG_HD __host__ __device__ inline
#else
#define LSXBG_HD inline
#endif
#if defined(__clang__)
#define LSXBG_UNROLL _Pragma("unroll")
#else
#define LSXBG_UNROLL
#endif

namespace lsxbg {

// witt.py:42-52 (cgs)
constexpr double BK = 1.3806488E-16, HH = 6.62606957E-27, PI = 3.14159265358979323846, CC = 2.99792458E10, AMU = 1.660538921E-24,
                 EV = 1.602176565E-12, ME = 9.10938188E-28;
constexpr int NCONTR = 28;      // witt.py:156
constexpr int NPART = 17;       // witt.getBackgroundPartials

// what the host forms once per call from lsx_eos_tables (witt.py:166-176, background.py:32); pointers are device or host memory
struct EosParams {
    int32_t npf, nelem, cap_pg, cap_rho, cap_pgrho, pad;      // caps of pe_from_pg (250), pe_from_rho (250), pg_from_rho (100)
    const double* tpf;
    const double* pf;          // [nelem][6][npf]
    const double* eion;        // [nelem][6]
    const int32_t* nstage;     // [nelem]
    const double* abund;       // [99] normalised
    double ab_others, avw, rho_from_H, saha_fac, rho_unit, cm3, g_to_kg;     // rho = rho_unit * nHTot * cm3 / g_to_kg
};

LSXBG_HD double acota(double x, double x0, double x1)     // witt.py:126-131
{
    if (x < x0) x = x0;
    if (x > x1) x = x1;
    return x;
}
LSXBG_HD double acotasig(double x, double x0, double x1)     // witt.py:135-143
{
    if (x < 0) return -acota(-x, x0, x1);
    return acota(x, x0, x1);
}

// witt._itep1 (witt.py:479-499) for a fixed temperature: the interval and the weights, found once
struct Itep {
    int32_t p0, p1;
    double u0, u1;
};
LSXBG_HD Itep itep_find(const double* x, int n, double xx)
{
    Itep q;
    if (xx <= x[0]) { q.p0 = q.p1 = 0; q.u0 = 1.0; q.u1 = 0.0; return q; }
    if (xx >= x[n - 1]) { q.p0 = q.p1 = n - 1; q.u0 = 1.0; q.u1 = 0.0; return q; }
    int lo = 0, hi = n - 1;      // x[lo] <= xx < x[hi]: the first index whose x is > xx
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] > xx) hi = mid; else lo = mid;
    }
    q.p0 = hi; q.p1 = hi - 1;
    const double dx = x[q.p1] - x[q.p0];
    q.u1 = (xx - x[q.p0]) / dx;
    q.u0 = 1.0 - q.u1;
    return q;
}
LSXBG_HD double itep_eval(const Itep& q, const double* y)
{
    if (q.p0 == q.p1) return y[q.p0];
    return q.u0 * y[q.p0] + q.u1 * y[q.p1];
}
// partition_f(n, t)[stage], zero beyond the element's stages (witt.py:504-528)
LSXBG_HD double pfun(const EosParams& P, const Itep& q, int el, int stage)
{
    if (stage >= P.nstage[el]) return 0.0;
    return itep_eval(q, P.pf + ((size_t)el * 6 + stage) * P.npf);
}

struct EosPoint {      // what is fixed for a point: temperature-only terms
    double t, theta, th25, cmol0, cmol1, uH0, uH1;
    Itep q;
};

// witt.saha (witt.py:204-206) with theta**2.5 taken once
LSXBG_HD double saha(const EosPoint& E, double eion, double u1, double u2, double pe)
{
    return u2 * exp(2.302585093 * (9.0804625434325867 - E.theta * eion)) / (u1 * pe * E.th25);
}

LSXBG_HD EosPoint eos_point(const EosParams& P, double t)
{
    EosPoint E;
    E.t = t;
    E.theta = 5040.0 / t;
    E.th25 = pow(E.theta, 2.5);
    const double X = E.theta;      // witt.molecb (witt.py:329-338)
    E.cmol0 = -11.206998 + X * (2.7942767 + X * (7.9196803E-2 - X * 2.4790744E-2));
    E.cmol1 = -12.533505 + X * (4.9251644 + X * (-5.6191273E-2 + X * 3.2687661E-3));
    E.q = itep_find(P.tpf, P.npf, t);
    E.uH0 = pfun(P, E.q, 0, 0);
    E.uH1 = pfun(P, E.q, 0, 1);
    return E;
}

// electrons from the first two ionised stages of the 27 donors (witt.py:374-382, 561-575)
LSXBG_HD double donors(const EosParams& P, const EosPoint& E, double pe)
{
    double g1 = 0.0;
    for (int ii = 1; ii < NCONTR; ++ii) {
        const double alfai = P.abund[ii] / P.abund[0];
        const double u0 = pfun(P, E.q, ii, 0), u1 = pfun(P, E.q, ii, 1), u2 = pfun(P, E.q, ii, 2);
        const double a = saha(E, P.eion[ii * 6 + 0], u0, u1, pe);
        const double b = saha(E, P.eion[ii * 6 + 1], u1, u2, pe);
        const double c = 1. + a * (1. + b);
        g1 += alfai / c * a * (1. + 2. * b);
    }
    return g1;
}

struct Hparts { double f1, f2, f3, f5, phtot, fe; };

// witt.pe_pg (witt.py:342-431) -> pe; fe_out
LSXBG_HD double pe_pg(const EosParams& P, const EosPoint& E, double pe, double pgas, double* fe_out)
{
    double g4, g5;
    if (pe < 0.0) {
        pe = 1.e-15; g4 = 0.0; g5 = 0.0;
    } else {
        const double c0 = acota(E.cmol0, -30., 30.), c1 = acota(E.cmol1, -30., 30.);
        g4 = pe * pow(10.0, c0);
        g5 = pe * pow(10.0, c1);
    }
    const double g2 = saha(E, P.eion[0], E.uH0, E.uH1, pe);
    double g3 = saha(E, 0.754, 1.0, E.uH0, pe);
    g3 = 1.0 / acota(g3, 1.e-30, 1.0e30);
    const double g1 = donors(P, E, pe);

    double a = 1. + g2 + g3;
    const double b = 2. * (1. + g2 / g5 * g4);
    const double c = g5;
    double d = g2 - g3;
    const double e = g2 / g5 * g4;
    a = acotasig(a, 1.e-15, 1.e15);
    d = acotasig(d, 1.e-15, 1.e15);
    const double c1 = c * b * b + a * d * b - e * a * a;
    const double c2 = 2.0 * a * e - d * b + a * b * g1;
    const double c3 = -(e + b * g1);
    double f1 = 0.5 * c2 / c1;
    f1 = -f1 + (fabs(1.) * (c1 / fabs(c1))) * sqrt(f1 * f1 - c3 / c1);
    double f5 = (1. - a * f1) / b;
    double f4 = e * f5;
    const double f3 = g3 * f1;
    const double f2 = g2 * f1;
    double fe = acota(f2 - f3 + f4 + g1, 1.e-30, 1.e30);
    double phtot = pe / fe;
    if (f5 <= 1.e-4) {
        double diff = 1.0;
        const double const6 = g5 / pe * f1 * f1, const7 = f2 - f3 + g1;
        int it = 0;
        while ((diff > 1.e-5) && (it < 5)) {
            const double of5 = f5;
            f5 = phtot * const6;
            f4 = e * f5;
            fe = const7 + f4;
            phtot = pe / fe;
            diff = 0.5 * fabs(f5 - of5) / (f5 + of5);
            it += 1;
        }
    }
    pe = pgas / (1. + (f1 + f2 + f3 + f4 + f5 + P.ab_others) / fe);
    if (pe <= 0.0) pe = 1.e-15;
    *fe_out = fe;
    return pe;
}

// witt.gasc (witt.py:541-621) -> pg; the six trailing entries of pp
LSXBG_HD double gasc(const EosParams& P, const EosPoint& E, double pe, Hparts* H)
{
    const double g4 = pow(10.0, E.cmol0), g5 = pow(10.0, E.cmol1);
    const double g2 = saha(E, P.eion[0], E.uH0, E.uH1, pe);
    const double g3 = 1.0 / saha(E, 0.754, 1.0, E.uH0, pe);
    const double g1 = donors(P, E, pe);

    const double a = 1. + g2 + g3;
    const double e = g2 / g5 * g4;
    const double b = 2.0 * (1.0 + e);
    const double c = g5;
    const double d = g2 - g3;
    const double c1 = c * b * b + a * d * b - e * a * a;
    const double c2 = 2. * a * e - d * b + a * b * g1;
    const double c3 = -(e + b * g1);
    double f1 = 0.5 * c2 / c1;
    f1 = -f1 + (fabs(1.0) * (c1 / fabs(c1))) * sqrt(f1 * f1 - c3 / c1);
    double f5 = (1.0 - a * f1) / b;
    double f4 = e * f5;
    const double f3 = g3 * f1;
    const double f2 = g2 * f1;
    double fe = f2 - f3 + f4 + g1;
    double phtot = pe / fe;
    if (f5 <= 1.e-5) {
        double diff = 1.0;
        const double const6 = g5 / pe * f1 * f1, const7 = f2 - f3 + g1;
        int it = 0;
        while ((diff > 1.e-5) && (it < 5)) {
            const double of5 = f5;
            f5 = phtot * const6;
            f4 = e * f5;
            fe = const7 + f4;
            phtot = pe / fe;
            diff = 0.5 * fabs(f5 - of5) / (f5 + of5);
            it += 1;
        }
    }
    const double pg = pe * (1.0 + (f1 + f2 + f3 + f4 + f5 + P.ab_others) / fe);
    H->f1 = f1; H->f2 = f2; H->f5 = f5; H->f3 = f3; H->phtot = phtot; H->fe = fe;
    return pg;
}

struct EosCount { int32_t npepg; int32_t capped; };      // pe_pg evaluations; a loop ended at its cap

// witt.pe_from_pg (witt.py:210-244)
LSXBG_HD double pe_from_pg(const EosParams& P, const EosPoint& E, double pg, EosCount* n)
{
    const double t = E.t;
    const double nu = P.abund[0];
    const double sah = pow(10.0, -0.4771 + 2.5 * log10(t) - log10(pg) - (13.6 * 5040.0 / t));
    const double aaa = 1.0 + sah;
    const double bbb = -(nu - 1.0) * sah;
    const double ccc = -sah * nu;
    const double ybh = (-bbb + sqrt(bbb * bbb - 4. * aaa * ccc)) / (2. * aaa);
    double pe = pg * ybh / (1. + ybh);
    double dif = 1.1, ope = pe, fe;
    int it = 0;
    while ((fabs(dif) > 1.e-5) && (it < P.cap_pg)) {
        pe = (ope + pe) * 0.5;
        ope = pe;
        pe = pe_pg(P, E, pe, pg, &fe);
        n->npepg += 1;
        dif = 2.0 * fabs(pe - ope) / (pe + ope);
        it += 1;
    }
    if (it >= P.cap_pg) n->capped = 1;      // the loop ran to its cap (whether or not its last pass met the stop test)
    return pe;
}

LSXBG_HD double start_fraction(double t)      // witt.py:257-260, 287-290
{
    if (t > 8000) return 0.5;
    if (t > 4000) return 0.1;
    if (t > 2000) return 0.01;
    return 0.001;
}

// witt.pe_from_rho (witt.py:248-279); its loop is capped here (the reference never increments the counter)
LSXBG_HD double pe_from_rho(const EosParams& P, const EosPoint& E, double rho, EosCount* n)
{
    const double t = E.t;
    const double xna = rho / P.avw;
    const double BKT = BK * t;
    const double a = start_fraction(t);
    const double xne = a * xna / (1.0 - a);
    double Pgas = (xna + xne) * BKT;
    int it = 0;
    double dif = 1.0, Pe = 0.0;
    while ((it < P.cap_rho) && (fabs(dif) > 1.e-5)) {
        Pe = pe_from_pg(P, E, Pgas, n);
        const double xna_guessed = (Pgas - Pe) / BKT;
        dif = fabs(xna - xna_guessed) / xna;
        Pgas *= xna / xna_guessed;
        it += 1;
    }
    if (it >= P.cap_rho) n->capped = 1;
    return Pe;
}

LSXBG_HD double rho_from_pe(const EosParams& P, const EosPoint& E, double pe)     // witt.py:312-316
{
    Hparts H;
    (void)gasc(P, E, pe, &H);
    return pe * P.rho_from_H / (H.fe * E.t);
}

// witt.pg_from_rho (witt.py:283-308)
LSXBG_HD double pg_from_rho(const EosParams& P, const EosPoint& E, double rho, EosCount* n)
{
    const double temp = E.t;
    const double xna = (rho / P.avw);
    const double a = start_fraction(temp);
    const double xne = a * xna / (1.0 - a);
    double pgas = (xna + xne) * BK * temp;
    double Pe = pe_from_pg(P, E, pgas, n);
    double irho = rho_from_pe(P, E, Pe);
    double dif = 1.0;
    int it = 0;
    while ((dif >= 1.e-5) && (it < P.cap_pgrho)) {
        Pe *= (1.0 + rho / irho) * 0.5;
        irho = rho_from_pe(P, E, Pe);
        dif = fabs((irho - rho) / (rho));
        it += 1;
    }
    if (it >= P.cap_pgrho) n->capped = 1;
    Hparts H;
    return gasc(P, E, Pe, &H);
}

// witt.getXparts(iatom, t, pg, pe, divide_by_u=True) (witt.py:625-667): the first `want` (<= 3) stages into out[]
LSXBG_HD void xparts(const EosParams& P, const EosPoint& E, int iatom, double pg, double pe, double t15, int want, double* out)
{
    const double t = E.t;
    const double TBK = t * BK, xna = (pg - pe) / TBK, xne = pe / TBK;
    const double n_tot = xna * P.abund[iatom] / 1.0;
    const int nLev = P.nstage[iatom];
    double u[6], xpa[6];
    LSXBG_UNROLL
    for (int ii = 0; ii < 6; ++ii) u[ii] = ii < nLev ? pfun(P, E.q, iatom, ii) : 1.0;
    xpa[0] = 1.0;
    LSXBG_UNROLL
    for (int ii = 1; ii < 6; ++ii)      // witt.nsaha (witt.py:198-200)
        xpa[ii] = ii < nLev ? 2.0 * P.saha_fac * (u[ii] / u[ii - 1]) * t15 * exp(-P.eion[iatom * 6 + ii - 1] * EV / (t * BK)) / xne : 0.0;
    LSXBG_UNROLL
    for (int ii = 5; ii > 0; --ii)
        if (ii < nLev) xpa[0] = 1.0 + xpa[0] * xpa[ii];
    xpa[0] = 1.0 / xpa[0];
    LSXBG_UNROLL
    for (int ii = 1; ii < 6; ++ii) xpa[ii] *= xpa[ii - 1];
    LSXBG_UNROLL
    for (int ii = 0; ii < 3; ++ii)
        if (ii < want) out[ii] = xpa[ii] * (n_tot / u[ii]);
}

// witt.getBackgroundPartials(t, pg, pe, divide_by_u=True) (witt.py:671-740): n[q] -> n[q * stride]
LSXBG_HD void background_partials(const EosParams& P, const EosPoint& E, double pg, double pe, double* n, size_t stride)
{
    const double t15 = pow(E.t, 1.5);
    const double tbk = E.t * BK;
    double x[3];
    xparts(P, E, 1, pg, pe, t15, 3, x);  n[3 * stride] = x[0]; n[4 * stride] = x[1]; n[5 * stride] = x[2];      // He
    xparts(P, E, 5, pg, pe, t15, 1, x);  n[6 * stride] = x[0];                                                  // C
    xparts(P, E, 12, pg, pe, t15, 1, x); n[7 * stride] = x[0];                                                  // Al
    xparts(P, E, 13, pg, pe, t15, 2, x); n[8 * stride] = x[0]; n[9 * stride] = x[1];                            // Si
    xparts(P, E, 19, pg, pe, t15, 2, x); n[10 * stride] = x[0]; n[11 * stride] = x[1];                          // Ca
    xparts(P, E, 11, pg, pe, t15, 2, x); n[12 * stride] = x[0]; n[13 * stride] = x[1];                          // Mg
    xparts(P, E, 25, pg, pe, t15, 1, x); n[14 * stride] = x[0];                                                 // Fe
    xparts(P, E, 6, pg, pe, t15, 1, x);  n[15 * stride] = x[0];                                                 // N
    xparts(P, E, 7, pg, pe, t15, 1, x);  n[16 * stride] = x[0];                                                 // O
    Hparts H;
    (void)gasc(P, E, pe, &H);
    n[0] = H.f1 * H.phtot / tbk * 0.5;
    n[1 * stride] = H.f2 * H.phtot / tbk;
    n[2 * stride] = H.f3 * H.phtot / tbk;
}

// one point of background.py:32-35 + the partials -> status (pe_pg evaluations, negated at a cap)
LSXBG_HD int32_t eos_solve(const EosParams& P, double t, double nHTot, double* pgas, double* pe, double* partials, size_t stride)
{
    const EosPoint E = eos_point(P, t);
    const double rho = P.rho_unit * nHTot * P.cm3 / P.g_to_kg;
    EosCount n{0, 0};
    *pgas = pg_from_rho(P, E, rho, &n);
    *pe = pe_from_rho(P, E, rho, &n);
    background_partials(P, E, *pgas, *pe, partials, stride);
    return n.capped ? -n.npepg : n.npepg;
}

// ---------------------------------------------------------------------------------------------------- continuous opacity
// coefficient tables: numbers from the literature (Kurucz's ATLAS: Karzas & Latter free-free Gaunt factors, Peach's Mg I /
// Si I / Si II cross-sections, the He I levels, the Fe I level list), as witt.py restates them at the lines cited
static constexpr double Z4LOG[6] = {0., 1.20412, 1.90849, 2.40824, 2.79588, 3.11261};      // witt.py:784
static constexpr double A0[12 * 11] = {                                                      // witt.py:785-797
    5.53, 5.49, 5.46, 5.43, 5.40, 5.25, 5.00, 4.69, 4.48, 4.16, 3.85,
    4.91, 4.87, 4.84, 4.80, 4.77, 4.63, 4.40, 4.13, 3.87, 3.52, 3.27,
    4.29, 4.25, 4.22, 4.18, 4.15, 4.02, 3.80, 3.57, 3.27, 2.98, 2.70,
    3.64, 3.61, 3.59, 3.56, 3.54, 3.41, 3.22, 2.97, 2.70, 2.45, 2.20,
    3.00, 2.98, 2.97, 2.95, 2.94, 2.81, 2.65, 2.44, 2.21, 2.01, 1.81,
    2.41, 2.41, 2.41, 2.41, 2.41, 2.32, 2.19, 2.02, 1.84, 1.67, 1.50,
    1.87, 1.89, 1.91, 1.93, 1.95, 1.90, 1.80, 1.68, 1.52, 1.41, 1.30,
    1.33, 1.39, 1.44, 1.49, 1.55, 1.56, 1.51, 1.42, 1.33, 1.25, 1.17,
    0.90, 0.95, 1.00, 1.08, 1.17, 1.30, 1.32, 1.30, 1.20, 1.15, 1.11,
    0.55, 0.58, 0.62, 0.70, 0.85, 1.01, 1.15, 1.18, 1.15, 1.11, 1.08,
    0.33, 0.36, 0.39, 0.46, 0.59, 0.76, 0.97, 1.09, 1.13, 1.10, 1.08,
    0.19, 0.21, 0.24, 0.28, 0.38, 0.53, 0.76, 0.96, 1.08, 1.09, 1.09};
static constexpr double A1[6] = {0.9916, 1.105, 1.101, 1.101, 1.102, 1.0986};              // witt.py:819-821
static constexpr double B1[6] = {2.719e3, -2.375e4, -9.863e3, -5.765e3, -3.909e3, -2.704e3};
static constexpr double C1[6] = {-2.268e10, 4.077e8, 1.035e8, 4.593e7, 2.371e7, 1.229e7};
static constexpr double G0[10] = {1., 3., 1., 9., 3., 3., 1., 9., 20., 3.};                // witt.py:929-934
static constexpr double HEFREQ0[10] = {5.9452090e15, 1.1528440e15, 0.9803331e15, .8761076e15, 0.8147100e15,
                                       0.4519048e15, 0.4030971e15, .8321191e15, 0.3660215e15, 0.3627891e15};
static constexpr double CHI0[10] = {0., 19.819, 20.615, 20.964, 21.217, 22.718, 22.920, 23.006, 23.073, 23.086};
static constexpr double PEACH0[15 * 7] = {                                                   // witt.py:1022-1036
    -42.474, -42.350, -42.109, -41.795, -41.467, -41.159, -40.883,
    -41.808, -41.735, -41.582, -41.363, -41.115, -40.866, -40.631,
    -41.273, -41.223, -41.114, -40.951, -40.755, -40.549, -40.347,
    -45.583, -44.008, -42.957, -42.205, -41.639, -41.198, -40.841,
    -44.324, -42.747, -41.694, -40.939, -40.370, -39.925, -39.566,
    -50.969, -48.388, -46.630, -45.344, -44.355, -43.568, -42.924,
    -50.633, -48.026, -46.220, -44.859, -43.803, -42.957, -42.264,
    -53.028, -49.643, -47.367, -45.729, -44.491, -43.520, -42.736,
    -51.785, -48.352, -46.050, -44.393, -43.140, -42.157, -41.363,
    -52.285, -48.797, -46.453, -44.765, -43.486, -42.480, -41.668,
    -52.028, -48.540, -46.196, -44.507, -43.227, -42.222, -41.408,
    -52.384, -48.876, -46.513, -44.806, -43.509, -42.488, -41.660,
    -52.363, -48.856, -46.493, -44.786, -43.489, -42.467, -41.639,
    -54.704, -50.772, -48.107, -46.176, -44.707, -43.549, -42.611,
    -54.359, -50.349, -47.643, -45.685, -44.198, -43.027, -42.418};
static constexpr double FREQMG[7] = {1.9341452e15, 1.8488510e15, 1.1925797e15, 7.9804046e14, 4.5772110e14, 4.1440977e14,
                                     4.1113514e14};                                          // witt.py:1037-1040
static constexpr double FLOG0[9] = {35.32123, 35.19844, 35.15334, 34.71490, 34.31318, 33.75728, 33.65788, 33.64994, 33.43947};
static constexpr double TLG0[7] = {8.29405, 8.51719, 8.69951, 8.85367, 8.98720, 9.10498, 9.21034};
static constexpr double PEACH1[19 * 9] = {                                                   // witt.py:1086-1104
    38.136, 38.138, 38.140, 38.141, 38.143, 38.144, 38.144, 38.145, 38.145,
    37.834, 37.839, 37.843, 37.847, 37.850, 37.853, 37.855, 37.857, 37.858,
    37.898, 37.898, 37.897, 37.897, 37.897, 37.896, 37.895, 37.895, 37.894,
    40.737, 40.319, 40.047, 39.855, 39.714, 39.604, 39.517, 39.445, 39.385,
    40.581, 40.164, 39.893, 39.702, 39.561, 39.452, 39.366, 39.295, 39.235,
    45.521, 44.456, 43.753, 43.254, 42.878, 42.580, 42.332, 42.119, 41.930,
    45.520, 44.455, 43.752, 43.251, 42.871, 42.569, 42.315, 42.094, 41.896,
    55.068, 51.783, 49.553, 47.942, 46.723, 45.768, 44.997, 44.360, 43.823,
    53.868, 50.369, 48.031, 46.355, 45.092, 44.104, 43.308, 42.652, 42.100,
    54.133, 50.597, 48.233, 46.539, 45.261, 44.262, 43.456, 42.790, 42.230,
    54.051, 50.514, 48.150, 46.454, 45.176, 44.175, 43.368, 42.702, 42.141,
    54.442, 50.854, 48.455, 46.733, 45.433, 44.415, 43.592, 42.912, 42.340,
    54.320, 50.722, 48.313, 46.583, 45.277, 44.251, 43.423, 42.738, 42.160,
    55.691, 51.965, 49.444, 47.615, 46.221, 45.119, 44.223, 43.478, 42.848,
    55.661, 51.933, 49.412, 47.582, 46.188, 45.085, 44.189, 43.445, 42.813,
    55.973, 52.193, 49.630, 47.769, 46.349, 45.226, 44.314, 43.555, 42.913,
    55.922, 52.141, 49.577, 47.715, 46.295, 45.172, 44.259, 43.500, 42.858,
    56.828, 52.821, 50.110, 48.146, 46.654, 45.477, 44.522, 43.730, 43.061,
    56.657, 52.653, 49.944, 47.983, 46.491, 45.315, 44.360, 43.569, 42.901};
static constexpr double FREQSI1[9] = {2.1413750e15, 1.97231650e15, 1.7879689e15, 1.5152920e15, 0.55723927e15, 5.3295914e14,
                                      4.7886458e14, 4.72164220e14, 4.6185133e14};            // witt.py:1105-1107
static constexpr double FLOG1[11] = {35.45438, 35.30022, 35.21799, 35.11986, 34.95438, 33.95402, 33.90947, 33.80244, 33.78835,
                                     33.76626, 33.70518};
static constexpr double TLG1[9] = {8.29405, 8.51719, 8.69951, 8.85367, 8.98720, 9.10498, 9.21034, 9.30565, 9.39266};
static constexpr double G1FE[48] = {25., 35., 21., 15., 9.,  35., 33., 21., 27., 49., 9.,  21., 27., 9.,  9.,  25.,     // witt.py:1130-1147
                                    33., 15., 35., 3.,  5.,  11., 15., 13., 15., 9.,  21., 15., 21., 25., 35., 9.,
                                    5.,  45., 27., 21., 15., 21., 15., 25., 21., 35., 5.,  15., 45., 35., 55., 25.};
static constexpr double E1FE[48] = {500.,   7500.,  12500., 17500., 19000., 19500., 19500., 21000., 22000., 23000., 23000., 24000.,
                                    24000., 24500., 24500., 26000., 26500., 26500., 27000., 27500., 28500., 29000., 29500., 29500.,
                                    29500., 30000., 31500., 31500., 33500., 33500., 34000., 34500., 34500., 35000., 35500., 37000.,
                                    37000., 37000., 38500., 40000., 40000., 41000., 41000., 43000., 43000., 43000., 43000., 44000.};
static constexpr double WNO1FE[48] = {63500., 58500., 53500., 59500., 45000., 44500., 44500., 43000., 58000., 41000., 54000., 40000.,
                                      40000., 57500., 55500., 38000., 57500., 57500., 37000., 54500., 53500., 55000., 34500., 34500.,
                                      34500., 34000., 32500., 32500., 32500., 32500., 32000., 29500., 29500., 31000., 30500., 29000.,
                                      27000., 54000., 27500., 24000., 47000., 23000., 44000., 42000., 42000., 21000., 42000., 42000.};
static constexpr double PEACH2[14 * 6] = {                                                   // witt.py:1219-1232
    -43.8941, -43.8941, -43.8941, -43.8941, -43.8941, -43.8941,
    -42.2444, -42.2444, -42.2444, -42.2444, -42.2444, -42.2444,
    -40.6054, -40.6054, -40.6054, -40.6054, -40.6054, -40.6054,
    -54.2389, -52.2906, -50.8799, -49.8033, -48.9485, -48.2490,
    -50.4108, -48.4892, -47.1090, -46.0672, -45.2510, -44.5933,
    -52.0936, -50.0741, -48.5999, -47.4676, -46.5649, -45.8246,
    -51.9548, -49.9371, -48.4647, -47.3340, -46.4333, -45.6947,
    -54.2407, -51.7319, -49.9178, -48.5395, -47.4529, -46.5709,
    -52.7355, -50.2218, -48.4059, -47.0267, -45.9402, -45.0592,
    -53.5387, -50.9189, -49.0200, -47.5750, -46.4341, -45.5082,
    -53.2417, -50.6234, -48.7252, -47.2810, -46.1410, -45.2153,
    -53.5097, -50.8535, -48.9263, -47.4586, -46.2994, -45.3581,
    -54.0561, -51.2365, -49.1980, -47.6497, -46.4302, -45.4414,
    -53.8469, -51.0256, -48.9860, -47.4368, -46.2162, -45.2266};
static constexpr double FREQSI2[7] = {4.9965417e15, 3.9466738e15, 1.5736321e15, 1.5171539e15, 9.2378947e14, 8.3825004e14,
                                      7.6869872e14};                                          // witt.py:1234-1236
static constexpr double FLOG2[9] = {36.32984, 36.14752, 35.91165, 34.99216, 34.95561, 34.45941, 34.36234, 34.27572, 34.20161};
static constexpr double TLG2[6] = {9.21034, 9.39266, 9.54681, 9.68034, 9.79813, 9.90349};

// numpy's sum of n (8 <= n <= 128) contiguous doubles: eight running sums, folded as a tree, the remainder added in order
template <int N, typename F>
LSXBG_HD double sum8(F term)
{
    static_assert(N >= 8, "sequential below 8");
    double r[8];
    LSXBG_UNROLL
    for (int j = 0; j < 8; ++j) r[j] = term(j);
    for (int i = 8; i < N - (N % 8); i += 8) {
    LSXBG_UNROLL
        for (int j = 0; j < 8; ++j) r[j] += term(i + j);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    LSXBG_UNROLL
    for (int i = N - (N % 8); i < N; ++i) res += term(i);
    return res;
}

LSXBG_HD double seaton(double FREQ0, double XSECT, double POWER, double A, double FREQ)      // witt.py:779-780
{
    return XSECT * (A + (1. - A) * (FREQ0 / FREQ)) * pow(FREQ0 / FREQ, floor(2. * POWER + 0.01) * 0.5);
}

LSXBG_HD double coulx(int N, double freq, double Z)      // witt.py:824-837
{
    const double n = (N + 1.0) * (N + 1.0);
    if (freq >= (Z * Z * 3.28805e15 / n)) {
        const double FREQ1 = freq * 1.e-10;
        double CLX = 0.2815 / FREQ1 / FREQ1 / FREQ1 / n / n / (N + 1.0) * Z * Z * Z * Z;
        if (N >= 6) return CLX;
        CLX *= (A1[N] + (B1[N] + C1[N] * (Z * Z / FREQ1)) * (Z * Z / FREQ1));
        return CLX;
    }
    return 0.0;
}

// what depends on the wavelength alone: the same in every lane of a wave at a loop step (made once per call, k_bg_wave)
struct OpWave {
    double FREQ, FREQLG, FREQ15, FREQ3, contH[8], contHe2[9], he1trans[10];
    double h2pl_FR, h2pl_ES, hmin_B, hmin_C, hmin_BF, sigH, heFREQ3b, hemi_A, hemi_B, hemi_C, sigHe, sigH2w;
    double c1_1100, c1_1240, c1_1444, al1, n1_853, n1_1020, n1_1130, o1, mg2_824, mg2_1169, ca2_1044, ca2_1218, ca2_1420;
    double mgD, si1D, si2D, fe_xsect[48];
    int32_t mgN, si1N, si2N, fe_on;
};

LSXBG_HD void make_wave(double wl_angstrom, OpWave* Wp)      // witt.py:1330-1332 and the frequency-only terms of every source
{
    OpWave& W = *Wp;
    const double FREQ = 2.997925E18 / wl_angstrom;
    const double FREQLG = log(FREQ);
    W.FREQ = FREQ; W.FREQLG = FREQLG; W.FREQ15 = FREQ * 1.E-15;
    W.FREQ3 = pow(FREQ * 1.E-10, 3.0);      // HOP, HE1OP
    LSXBG_UNROLL
    for (int N = 0; N < 8; ++N) W.contH[N] = coulx(N, FREQ, 1.0);
    LSXBG_UNROLL
    for (int N = 0; N < 9; ++N) W.contHe2[N] = coulx(N, FREQ, 2.0);
    // HE1OP (witt.py:950-955): every level from the first whose edge lies at or below FREQ
    int NMIN = 9;
    for (int n = 0; n < 10; ++n) if (HEFREQ0[n] <= FREQ) { NMIN = n; break; }
    const double dum[10] = {33.32 - 2. * FREQLG, -390.026 + (21.035 - 0.318 * FREQLG) * FREQLG, 26.83 - 1.91 * FREQLG, 61.21 - 2.9 * FREQLG,
                            81.35 - 3.5 * FREQLG, 12.69 - 1.54 * FREQLG, 23.85 - 1.86 * FREQLG, 49.30 - 2.60 * FREQLG, 85.20 - 3.69 * FREQLG,
                            58.81 - 2.89 * FREQLG};
    LSXBG_UNROLL
    for (int n = 0; n < 10; ++n) W.he1trans[n] = n >= NMIN ? exp(dum[n]) : 0.0;
    // H2PLOP (witt.py:889-898)
    W.h2pl_FR = -3.0233E3 + (3.7797E2 + (-1.82496E1 + (3.9207E-1 - 3.1672E-3 * FREQLG) * FREQLG) * FREQLG) * FREQLG;
    W.h2pl_ES = -7.342E-3 + (-2.409 + (1.028 + (-0.4230 + (0.1224 - 0.01351 * W.FREQ15) * W.FREQ15) * W.FREQ15) * W.FREQ15) * W.FREQ15;
    {   // HMINOP (witt.py:904-912)
        const double FREQ1 = FREQ * 1.E-10;
        W.hmin_B = (1.3727E-15 + 4.3748 / FREQ) / FREQ1;
        W.hmin_C = -2.5993E-7 / pow(FREQ1, 2.0);
        if (FREQ <= 1.8259E14) W.hmin_BF = 0.;
        else if (FREQ >= 2.111E14) W.hmin_BF = 6.801E-10 + (5.358E-3 + (1.481E3 + (-5.519E7 + 4.808E11 / FREQ1) / FREQ1) / FREQ1) / FREQ1;
        else W.hmin_BF = 3.695E-6 + (-1.251E-1 + 1.052E3 / FREQ1) / FREQ1;
    }
    {   // HRAYOP (witt.py:876-884)
        double WAVE = fmin(FREQ, 2.463e15);
        WAVE = 2.997925e18 / WAVE;
        const double WW = WAVE * WAVE, WW2 = WW * WW;
        W.sigH = (5.799e-13 + 1.422e-6 / WW + 2.784 / (WW2)) / (WW2);
    }
    W.heFREQ3b = pow(FREQ * 1.E-5, 3.0);     // HE2OP
    W.hemi_A = 3.397E-26 + (-5.216E-11 + 7.039E05 / FREQ) / FREQ;      // HEMIOP (witt.py:1005-1009)
    W.hemi_B = -4.116E-22 + (1.067E-06 + 8.135E09 / FREQ) / FREQ;
    W.hemi_C = 5.081E-17 + (-8.724E-03 - 5.659E12 / FREQ) / FREQ;
    {   // HERAOP (witt.py:1014-1018)
        const double WW = pow(2.997925E+03 / fmin(FREQ * 1.E-15, 5.15), 2.0);
        const double arg = 1. + (2.44E5 + 5.94E10 / (WW - 2.90E5)) / WW;
        W.sigHe = 5.484E-14 / WW / WW * arg * arg;
    }
    {   // H2RAOP (witt.py:1309-1312)
        const double WW = pow(2.997925E18 / fmin(FREQ, 2.922E15), 2.0);
        const double WW2 = WW * WW;
        W.sigH2w = (8.14E-13 + 1.28e-6 / WW + 1.61e0 / WW2) / WW2;
    }
    // C1OP (witt.py:1071-1073), Al1OP (:1081), N1OP (:1188-1190), O1OP (:1198), Mg2OP (:1212-1213), Ca2OP (:1269-1274)
    W.c1_1100 = FREQ >= 2.7254E15 ? seaton(2.7254E15, 1.219E-17, 2.0E0, 3.317E0, FREQ) : 0.0;
    W.c1_1240 = FREQ >= 2.4196E15 ? seaton(2.4196E15, 1.030E-17, 1.5E0, 2.789E0, FREQ) : 0.0;
    W.c1_1444 = FREQ >= 2.0761E15 ? seaton(2.0761E15, 9.590E-18, 1.5E0, 3.501E0, FREQ) : 0.0;
    W.al1 = FREQ > 1.443E15 ? 2.1E-17 * (pow(1.443E15 / FREQ, 3.0)) * 6.0 : 0.0;
    W.n1_853 = FREQ >= 3.517915E15 ? seaton(3.517915E15, 1.142E-17, 2.0E0, 4.29E0, FREQ) : 0.;
    W.n1_1020 = FREQ >= 2.941534E15 ? seaton(2.941534E15, 4.410E-18, 1.5E0, 3.85E0, FREQ) : 0.;
    W.n1_1130 = FREQ >= 2.653317E15 ? seaton(2.653317E15, 4.200E-18, 1.5E0, 4.34E0, FREQ) : 0.;
    W.o1 = FREQ >= 3.28805E15 ? 9. * seaton(3.28805E15, 2.94E-18, 1.E0, 2.66E0, FREQ) : 0.0;
    W.mg2_824 = FREQ >= 3.635492E15 ? seaton(3.635492E15, 1.40E-19, 4.E0, 6.7E0, FREQ) : 0.0;
    W.mg2_1169 = FREQ >= 2.564306E15 ? 5.11E-19 * pow(2.564306E15 / FREQ, 3.0) : 0.0;
    W.ca2_1044 = FREQ >= 2.870454e15 ? 1.08e-19 * pow(2.870454e15 / FREQ, 3.0) : 0.;
    W.ca2_1218 = FREQ >= 2.460127e15 ? 1.64e-17 * sqrt(2.460127e15 / FREQ) : 0.;
    W.ca2_1420 = FREQ >= 2.110779e15 ? seaton(2.110779e15, 4.13e-18, 3., 0.69, FREQ) : 0.;
    {   // Mg1OP (witt.py:1048-1052), Si1OP (:1115-1120), Si2OP (:1245-1252): the frequency interval
        int N = 6;
        for (int q = 0; q < 7; ++q) if (FREQ > FREQMG[q]) { N = q; break; }
        W.mgD = (FREQLG - FLOG0[N]) / (FLOG0[N + 1] - FLOG0[N]);
        if (N > 1) N = 2 * N - 1;
        W.mgN = N;
        N = 8;
        for (int q = 0; q < 9; ++q) if (FREQ > FREQSI1[q]) { N = q; break; }
        W.si1D = (FREQLG - FLOG1[N]) / (FLOG1[N + 1] - FLOG1[N]);
        if (N > 1) N = 2 * N - 1;
        W.si1N = N;
        N = 6;
        for (int q = 0; q < 7; ++q) if (FREQ > FREQSI2[q]) { N = q; break; }
        W.si2D = (FREQLG - FLOG2[N]) / (FLOG2[N + 1] - FLOG2[N]);
        if (N > 1) N = 2 * N - 2;
        if (N == 13) N = 12;
        W.si2N = N;
    }
    {   // Fe1OP (witt.py:1150-1159)
        const double WAVENO = FREQ / 2.99792458E10;
        W.fe_on = WAVENO < 21000. ? 0 : 1;
        for (int q = 0; q < 48; ++q) {
            const double XXX = ((WNO1FE[q] + 3000. - WAVENO) / WNO1FE[q] / .1);
            W.fe_xsect[q] = WNO1FE[q] < WAVENO ? 3.e-18 / (1. + pow(XXX, 4.0)) : 0.0;
        }
    }
}

// what depends on the temperature and the 17 partials alone: once per (column, depth), kept in registers
struct OpLane {
    double T, TKEV, HKT, TLOG, XNE, sqrtT;
    double H1, H2, HE1, HE2, HE3, C1, AL1, SI1, SI2, CA2, MG1, MG2, FE1, N1, O1;
    double hbolt[8], h_boltex, h_exlim, he1bolt[10], he1_freet, he1_boltex, he1_exlim, he2bolt[9], he2_freet, he2_boltex, he2_exlim;
    double hmin, h2ra, c1240, c1444, n1130, n1020, mg1169, ca1218, ca1420, mgDT, si1DT, si2DT, gamlog1, gamlog2;
    int32_t mgNT, si1NT, si2NT, cool, luke;
};

LSXBG_HD void make_lane(double T, double pgas, double pe, const double* n, size_t stride, OpLane* Lp)      // witt.py:744-763
{
    OpLane& L = *Lp;
    const double TK = T * BK, TKEV = TK / EV;
    L.T = T; L.TKEV = TKEV; L.HKT = HH / TK; L.TLOG = log(T); L.XNE = pe / TK; L.sqrtT = sqrt(T);
    (void)pgas;
    const double XH1 = n[0], XHMIN = n[2 * stride];
    L.H1 = XH1; L.H2 = n[stride]; L.HE1 = n[3 * stride]; L.HE2 = n[4 * stride]; L.HE3 = n[5 * stride]; L.C1 = n[6 * stride];
    L.AL1 = n[7 * stride]; L.SI1 = n[8 * stride]; L.SI2 = n[9 * stride]; L.CA2 = n[11 * stride]; L.MG1 = n[12 * stride];
    L.MG2 = n[13 * stride]; L.FE1 = n[14 * stride]; L.N1 = n[15 * stride]; L.O1 = n[16 * stride];
    // HOP (witt.py:850-857)
    LSXBG_UNROLL
    for (int q = 0; q < 8; ++q) { const double n1 = (q + 1.0) * (q + 1.0); L.hbolt[q] = exp(-13.595 * (1. - 1. / n1) / TKEV) * 2. * n1 * XH1; }
    {
        const double XR = XH1 / 13.595 * TKEV;
        L.h_boltex = exp(-13.427 / TKEV) * XR;
        L.h_exlim = exp(-13.595 / TKEV) * XR;
    }
    // HE1OP (witt.py:940-945)
    LSXBG_UNROLL
    for (int q = 0; q < 10; ++q) L.he1bolt[q] = exp(-CHI0[q] / TKEV) * G0[q] * L.HE1;
    L.he1_freet = L.XNE * 1.E-10 * L.HE2 * 1.E-10 / L.sqrtT * 1.E-10;
    {
        const double XRLOG = log(L.HE1 * (2. / 13.595) * TKEV);
        L.he1_boltex = exp(-23.730 / TKEV + XRLOG);
        L.he1_exlim = exp(-24.587 / TKEV + XRLOG);
    }
    // HE2OP (witt.py:977-983)
    LSXBG_UNROLL
    for (int q = 0; q < 9; ++q) { const double N12 = (q + 1.0) * (q + 1.0); L.he2bolt[q] = exp(-(54.403 - 54.403 / N12) / TKEV) * 2. * N12 * L.HE2; }
    L.he2_freet = L.XNE * L.HE3 / L.sqrtT;
    {
        const double XR = L.HE2 / 13.595 * TKEV;
        L.he2_boltex = exp(-53.859 / TKEV) * XR;
        L.he2_exlim = exp(-54.403 / TKEV) * XR;
    }
    // HMINOP (witt.py:921-922)
    if (T < 7730.) L.hmin = XHMIN;
    else L.hmin = exp(0.7552 / TKEV) / (2. * 2.4148E15 * T * L.sqrtT) * XH1 * L.XNE;
    {   // H2RAOP (witt.py:1313-1317)
        const double ARG = 4.477 / TKEV - 4.6628E1 + (1.8031E-3 + (-5.023E-7 + (8.1424E-11 - 5.0501E-15 * T) * T) * T) * T - 1.5 * L.TLOG;
        const double H1 = XH1 * 2.0;
        L.h2ra = ARG > -80.0 ? exp(ARG) * H1 * H1 : 0.0;
    }
    L.c1240 = 5. * exp(-1.264 / TKEV); L.c1444 = exp(-2.683 / TKEV);                 // witt.py:1065-1066
    L.n1130 = 6. * exp(-3.575 / TKEV); L.n1020 = 10. * exp(-2.384 / TKEV);            // :1182-1183
    L.mg1169 = 6. * exp(-4.43 / TKEV);                                              // :1208
    L.ca1218 = 10. * exp(-1.697 / TKEV); L.ca1420 = 6. * exp(-3.142 / TKEV);         // :1265-1266
    {   // the temperature interval of the Peach tables (witt.py:1044-1047, 1111-1113, 1241-1243)
        int NT = (int)floor(T / 1000.) - 3; if (NT > 6) NT = 6; if (NT < 1) NT = 1;
        L.mgNT = NT; L.mgDT = (L.TLOG - TLG0[NT - 1]) / (TLG0[NT] - TLG0[NT - 1]);
        NT = (int)floor(T / 1000.) - 3; if (NT > 8) NT = 8; if (NT < 1) NT = 1;
        L.si1NT = NT; L.si1DT = (L.TLOG - TLG1[NT - 1]) / (TLG1[NT] - TLG1[NT - 1]);
        NT = (int)floor(T / 2000.) - 4; if (NT > 5) NT = 5; if (NT < 1) NT = 1;
        L.si2NT = NT; L.si2DT = (L.TLOG - TLG2[NT - 1]) / (TLG2[NT] - TLG2[NT - 1]);
    }
    L.gamlog1 = 10.39638 - L.TLOG / 1.15129 + Z4LOG[0];      // COULFF (witt.py:802)
    L.gamlog2 = 10.39638 - L.TLOG / 1.15129 + Z4LOG[1];
    L.cool = T < 12000. ? 1 : 0;      // witt.py:1347-1350
    L.luke = T < 30000. ? 1 : 0;
}

LSXBG_HD double coulff(double GAMLOG, double TLOG, double FREQLG)      // witt.py:801-814
{
    int IGAM = (int)(GAMLOG + 7.); if (IGAM > 10) IGAM = 10;
    if (IGAM < 1) IGAM = 1;
    const double HVKTLG = (FREQLG - TLOG) / 1.15129 - 20.63764;
    int IHVKT = (int)(HVKTLG + 9.); if (IHVKT > 11) IHVKT = 11;
    if (IHVKT < 1) IHVKT = 1;
    const double Pq = GAMLOG - (IGAM - 7);
    const double Q = HVKTLG - (IHVKT - 9);
    return (1. - Pq) * ((1. - Q) * A0[(IHVKT - 1) * 11 + IGAM - 1] + Q * A0[IHVKT * 11 + IGAM - 1]) +
           Pq * ((1. - Q) * A0[(IHVKT - 1) * 11 + IGAM] + Q * A0[IHVKT * 11 + IGAM]);
}

// witt.cop for one wavelength (witt.py:1322-1362): OPACITY = A + B, in cm^-1
LSXBG_HD double cop_point(const OpLane& L, const OpWave& W)
{
    const double FREQ = W.FREQ, FREQLG = W.FREQLG, T = L.T, TKEV = L.TKEV, XNE = L.XNE;
    const double EHVKT = exp(-FREQ * L.HKT);
    const double STIM = 1.0 - EHVKT;
    const double ff1 = coulff(L.gamlog1, L.TLOG, FREQLG);

    double AHYD;
    {   // HOP (witt.py:842-871)
        const double CFREE = 3.6919E-22 / W.FREQ3;
        const double FREET = XNE * CFREE * L.H2 / L.sqrtT;
        double BOLTEX = L.h_boltex;
        const double EXLIM = L.h_exlim;
        const double C = 0.2815 / W.FREQ3;
        if (FREQ < 4.05933E13) BOLTEX = EXLIM / EHVKT;
        double H = (W.contH[6] * L.hbolt[6] + W.contH[7] * L.hbolt[7] + (BOLTEX - EXLIM) * C + ff1 * FREET) * STIM;
        double s = 0.0;
    LSXBG_UNROLL
        for (int q = 0; q < 6; ++q) s += W.contH[q] * L.hbolt[q];
        H += s * (1. - EHVKT);
        AHYD = H;
    }
    double AH2P = 0.0;      // H2PLOP (witt.py:889-898)
    if (!(FREQ > 3.28805E15)) AH2P = exp(-W.h2pl_ES / TKEV + W.h2pl_FR) * 2. * L.H1 * L.H2 * STIM;
    double AHMIN;
    {   // HMINOP (witt.py:904-925)
        const double HMINFF = (W.hmin_B + W.hmin_C / T) * L.H1 * XNE * 2.E-20;
        const double H = W.hmin_BF * (1 - EHVKT) * L.hmin * 1.E-10;
        AHMIN = H + HMINFF;
    }
    const double SIGH = W.sigH * L.H1 * 2.0;      // HRAYOP
    double AHE1;
    {   // HE1OP (witt.py:937-964)
        const double CFREE = 3.6919E8 / W.FREQ3;
        const double C = 2.815E-1 / W.FREQ3;
        double EX = L.he1_boltex;
        if (FREQ < 2.055E14) EX = L.he1_exlim / EHVKT;
        double HE1 = (EX - L.he1_exlim) * C;
        HE1 += sum8<10>([&](int q) { return W.he1trans[q] * L.he1bolt[q]; });
        AHE1 = (HE1 + ff1 * L.he1_freet * CFREE) * STIM;
    }
    double AHE2;
    {   // HE2OP (witt.py:969-999)
        const double CFREE = 3.6919E-07 / W.heFREQ3b * 4.0;
        const double C = 2.815E14 * 2.0 * 2.0 / W.heFREQ3b;
        double EX = L.he2_boltex;
        if (FREQ < 1.31522E14) EX = L.he2_exlim / EHVKT;
        double HE2 = (EX - L.he2_exlim) * C;
        HE2 += sum8<9>([&](int q) { return W.contHe2[q] * L.he2bolt[q]; });
        HE2 = (HE2 + coulff(L.gamlog2, L.TLOG, FREQLG) * CFREE * L.he2_freet) * STIM;
        AHE2 = HE2 >= 1.E-20 ? HE2 : 0.0;
    }
    const double AHEMIN = (W.hemi_A * T + W.hemi_B + W.hemi_C / T) * XNE * L.HE1 * 1.E-20;      // HEMIOP
    const double SIGHE = W.sigHe * L.HE1;                                                       // HERAOP
    double ACOOL = 0.0, ALUKE = 0.0;
    if (L.cool) {   // COOLOP (witt.py:1166-1173)
        const double c1op = W.c1_1100 * 9. + W.c1_1240 * L.c1240 + W.c1_1444 * L.c1444;
        double mg1op, si1op, fe1op = 0.0;
        {
            const int N = W.mgN, NT = L.mgNT;
            const double D = W.mgD, D1 = 1.0 - D, DT = L.mgDT;
            const double XWL1 = PEACH0[(N + 1) * 7 + NT - 1] * D + PEACH0[N * 7 + NT - 1] * D1;
            const double XWL2 = PEACH0[(N + 1) * 7 + NT] * D + PEACH0[N * 7 + NT] * D1;
            mg1op = exp(XWL1 * (1. - DT) + XWL2 * DT);
        }
        {
            const int N = W.si1N, NT = L.si1NT;
            const double D = W.si1D, DD = 1. - D, DT = L.si1DT;
            const double XWL1 = PEACH1[(N + 1) * 9 + NT - 1] * D + PEACH1[N * 9 + NT - 1] * DD;
            const double XWL2 = PEACH1[(N + 1) * 9 + NT] * D + PEACH1[N * 9 + NT] * DD;
            si1op = exp(-(XWL1 * (1. - DT) + XWL2 * DT)) * 9.;
        }
        if (W.fe_on) fe1op = sum8<48>([&](int q) { return W.fe_xsect[q] * (G1FE[q] * exp(-E1FE[q] * 2.99792458e10 * L.HKT)); });
        ACOOL = (c1op * L.C1 + mg1op * L.MG1 + W.al1 * L.AL1 + si1op * L.SI1 + fe1op * L.FE1) * STIM;
    }
    if (L.luke) {   // LUKEOP (witt.py:1281-1289)
        const double n1op = W.n1_853 * 4. + W.n1_1020 * L.n1020 + W.n1_1130 * L.n1130;
        const double mg2op = W.mg2_824 * 2. + W.mg2_1169 * L.mg1169;
        double si2op;
        {
            const int N = W.si2N, NT = L.si2NT;
            const double D = W.si2D, D1 = 1. - D, DT = L.si2DT;
            const double XWL1 = PEACH2[(N + 1) * 6 + NT - 1] * D + PEACH2[N * 6 + NT - 1] * D1;
            const double XWL2 = PEACH2[(N + 1) * 6 + NT] * D + PEACH2[N * 6 + NT] * D1;
            si2op = exp(XWL1 * (1. - DT) + XWL2 * DT) * 6.;
        }
        const double ca2op = W.ca2_1044 + W.ca2_1218 * L.ca1218 + W.ca2_1420 * L.ca1420;
        ALUKE = (n1op * L.N1 + W.o1 * L.O1 + mg2op * L.MG2 + si2op * L.SI2 + ca2op * L.CA2) * STIM;
    }
    const double SIGEL = 0.6653E-24 * XNE;              // ELECOP
    const double SIGH2 = L.h2ra * W.sigH2w;             // H2RAOP
    const double A = AHYD + AHMIN + AH2P + AHE1 + AHE2 + AHEMIN + ACOOL + ALUKE + 0.0;
    const double B = SIGH + SIGHE + SIGEL + SIGH2;
    return A + B;
}

// utils.py:17-22, in the form the sweeps' device function has it
LSXBG_HD double planck_nm(double temp, double wav)
{
    constexpr double kHC = 6.6260755E-34 * 2.99792458E+08, kKB = 1.380658E-23, kNM = 1.0E-09;
    const double hc_Tkla = kHC / (kKB * kNM * wav) / temp;
    const double x = kNM * wav;
    const double twohnu3_c2 = (2.0 * kHC) / (x * x * x);
    return twohnu3_c2 / (exp(hc_Tkla) - 1.0);
}

} // namespace lsxbg
