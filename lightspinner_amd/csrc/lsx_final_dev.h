// lsx_final_dev.h -- what the five read-only final passes over a converged context have in common, as inlined device functions
// (lsx_rays.hip, lsx_rates.hip, lsx_losses.hip, lsx_depth.hip, lsx_spectrum.hip).  The kernels stay five kernels:
// each keeps its walk, its parameter struct and what it does with the intensity; only text they all had moved here.  gfx950 only.
//
// Reference lines restated here:
//   utils.py:17-22                     planck
//   formal_solver.py:46-142, 203-209   the recurrence with its end-point quirk; boundary values 0 (top), thermalised (bottom)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "lsx_dev.h"

namespace lsxd {

constexpr double kCLight = 2.99792458E+08;
constexpr double kHPlanck = 6.6260755E-34;
constexpr double kKBoltzmann = 1.380658E-23;
constexpr double kNM_TO_M = 1.0E-09;
constexpr double kHC = kHPlanck * kCLight;

// utils.py:17-22 (as lsx_sweep.hip has it)
__device__ __forceinline__ double planck(double temp, double wav)
{
    const double hc_Tkla = kHC / (kKBoltzmann * kNM_TO_M * wav) / temp;
    const double x = kNM_TO_M * wav;
    const double twohnu3_c2 = (2.0 * kHC) / (x * x * x);
    return twohnu3_c2 / (exp(hc_Tkla) - 1.0);
}

// one transition as one wavelength of the context's grid sees it; the entries of a wavelength are in table order
// (final_tables, lsx_final_host.h)
struct FinalEnt {
    int32_t is_line;
    int32_t li, lj;             // rows of n
    int32_t row;                // lines: row of aDamp; continua: row of nsr
    int32_t atom;               // lines: row of vBroad
    int32_t phi_base, phi_len, phi_l;   // lines: the (tile, line) block of the profile store and the wavelength's place in it
    double a;                   // lines: (hc/4pi) Bij; continua: alpha at this wavelength
    double g;                   // lines: Bji / Bij
    double Uc;                  // lines: (Aji / Bji) g (hc/4pi) Bij
    double lambda0;             // lines: rest wavelength [nm]
    int32_t cell, pad_;         // lines: the wavelength's place in the line pool of a work array (DevTrans.phi_off + lt)
};

// what a lane (one wavelength of the grid, one column) reads at every depth: its place in the tile-major streams the context keeps
// ([col][tile][k][j < L]: + k L, the scattering coefficient + k sstr), the column's heights, populations and nStar ratios, and its
// run of the entry table.  P: the kernel's parameter struct
struct FinalColumn {
    const double *bgchi, *bgeta, *Jd, *Eb, *sca, *z, *n_col, *nsr_col;
    int sstr, e0, e1;
};
template <class P>
__device__ __forceinline__ FinalColumn final_column(const P& p, size_t col, int la)
{
    const int Ns = p.Ns, L = p.L;
    const int tile = p.la_tile[2 * la], j = p.la_tile[2 * la + 1];
    const size_t toff = (size_t)tile * Ns * L + j;
    FinalColumn f;
    f.bgchi = p.bgchi_T + col * p.til_col + toff;
    f.bgeta = p.bgeta_T + col * p.til_col + toff;
    f.Jd = p.J_T + col * p.til_col + toff;
    f.Eb = p.E_T ? p.E_T + col * p.til_col + toff : nullptr;
    f.sca = p.sca_per_lambda ? p.sca + col * p.sca_col + toff : p.sca + col * p.sca_col;
    f.sstr = p.sca_per_lambda ? L : 1;
    f.z = p.height + col * Ns;
    f.n_col = p.n + col * (size_t)p.NLtot * Ns;
    f.nsr_col = p.nsr ? p.nsr + col * (size_t)p.Ncont * Ns : nullptr;
    f.e0 = p.la_ptr[la];
    f.e1 = p.la_ptr[la + 1];
    return f;
}

// the up-going ray at the angles of a call (lsx_rays.hip, lsx_depth.hip): where the column was built with a line-of-sight velocity
// (raydep) the profile of a line is the Voigt function at every angle (rh_method.py:231-239) from the kept broadening arrays of the
// column; else the profile the formal solution uses is read (compact: row k; else the up-going row of ray 0).
// (The assembly of chi and eta from the entries, rh_method.py:599-632, is each unit's own text: DESIGN.md 4.21)
struct FinalAngles {
    bool raydep;
    const double *aD, *vB, *vL;
};
template <class P>
__device__ __forceinline__ FinalAngles final_angles(const P& p, size_t col)
{
    FinalAngles f;
    f.raydep = !p.phi_compact && p.prof_kind && p.prof_kind[col] == 2;
    f.aD = f.raydep ? p.aDamp + col * (size_t)p.NlinesA * p.Ns : nullptr;
    f.vB = f.raydep ? p.vBroad + col * (size_t)p.Natoms * p.Ns : nullptr;
    f.vL = f.raydep ? p.vlos + col * p.Ns : nullptr;
    return f;
}

// ---- the recurrence along a ray.  State per ray (lsx_sweep.hip, generic path): the intensity Iu; linear rule c_k = chi, S_k = S and
// dtau_prev of the depth behind; parabolic rule the window (c_u, S_u), (c_k, S_k) of the two depths behind the one that arrives ----
template <int NM>
__device__ __forceinline__ void final_state_init(double (&Iu)[NM], double (&c_k)[NM], double (&S_k)[NM], double (&c_u)[NM], double (&S_u)[NM],
                                                 double (&dtau_prev)[NM])
{
#pragma unroll
    for (int m = 0; m < NM; ++m) { Iu[m] = 0.0; c_k[m] = 1.0; S_k[m] = 0.0; c_u[m] = 1.0; S_u[m] = 0.0; dtau_prev[m] = 1.0; }
}

// the value a ray starts with at a thermalised end (formal_solver.py:203-207), at the second depth of the walk: Be, Bn the Planck
// function at the end's depth and at the next one, adz the distance between them, c_k and chi their opacities
template <int NM>
__device__ __forceinline__ void thermal_start(double Be, double Bn, double adz, const double (&zmu)[NM], const double (&c_k)[NM],
                                              const double (&chi)[NM], double (&Iu)[NM])
{
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const double dtau_uw = zmu[m] * (c_k[m] + chi[m]) * 0.5 * adz;
        Iu[m] = Be - (Bn - Be) / dtau_uw;
    }
}

// the values the context's own rays mu0 .. mu0 + NM - 1 start with at their end of the column (lsx_rates.hip, lsx_losses.hip), at
// the second depth of the walk: k1 the end's depth, k the next one.  No boundary set (p.bnd null): thermalised below, zero above;
// else the kind of this direction's end (include/lsx_hip_boundary.h; wave-uniform: a block is one column), the thermalised value of
// the upper end being the mirror image of the lower one
template <int NM, class P>
__device__ __forceinline__ void final_start(const P& p, size_t col, int la, bool up, int k1, int k, double wav, double adz,
                                            const double (&zmu)[NM], const double (&c_k)[NM], const double (&chi)[NM], double (&Iu)[NM])
{
    if (p.bnd == nullptr) {
        if (up) thermal_start(planck(p.temperature[col * p.Ns + k1], wav), planck(p.temperature[col * p.Ns + k], wav), adz, zmu, c_k, chi, Iu);
        return;                        // (down: Iu is still 0)
    }
    const int end = up ? LSX_BND_LOWER : LSX_BND_UPPER;
    const int kind = boundary_kind(p.bnd, col, end);
    if (kind == 1) {
        thermal_start(planck(p.temperature[col * p.Ns + k1], wav), planck(p.temperature[col * p.Ns + k], wav), adz, zmu, c_k, chi, Iu);
    } else if (kind == 2) {
        const double* given = boundary_given(p.bnd, end, col, (size_t)p.Nspect * p.Nrays) + (size_t)la * p.Nrays + p.mu0;
#pragma unroll
        for (int m = 0; m < NM; ++m) Iu[m] = given[m];
    }
}

// the linear rule, formal_solver.py:107-139, as the sweep's generic path has it: the two divisions of a step share one reciprocal.
// s: step along the ray (0: only the state is set), last: the ray's end point, hdz: half the distance to the depth behind
template <int NM>
__device__ __forceinline__ void linear_step(int s, bool last, double hdz, const double (&zmu)[NM], const double (&chi)[NM],
                                            const double (&eta)[NM], double (&Iu)[NM], double (&c_k)[NM], double (&S_k)[NM],
                                            double (&dtau_prev)[NM], const lds_f64* etab)
{
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        if (s == 0) {
            const double rchi = rcp(chi[m]);
            S_k[m] = eta[m] * rchi;
            c_k[m] = chi[m];
            continue;
        }
        const double dtau = (c_k[m] + chi[m]) * (hdz * zmu[m]);
        const double rcd = rcp(chi[m] * dtau);
        const double rchi = rcd * dtau, rdt = rcd * chi[m];
        const double S = eta[m] * rchi;                    // :632
        const double dS = (S_k[m] - S) * rdt;
        // formal_solver.py:138-139: the end point re-uses the previous interval's w and S[kEnd - dk] with the fresh dS
        double w0, w1;
        w2(last ? dtau_prev[m] : dtau, w0, w1, etab);
        const double Sx = last ? S_k[m] : S;
        Iu[m] = Iu[m] * (1.0 - w0) + w0 * Sx + w1 * dS;
        dtau_prev[m] = dtau;
        c_k[m] = chi[m];
        S_k[m] = S;
    }
}

// the linear rule operation by operation, in the reference's order and without contraction into fused multiply-adds: two divisions
// per step where linear_step shares one reciprocal (lsx_depth.hip, lsx_spectrum.hip).  I is handed out at EVERY depth there, and some
// of those values are heavy cancellations (the end point adds w1 dS of ITS interval to the previous interval's w0 S, :138-139:
// 2e5-fold on a three-depth column of the tests); there a reciprocal's 4e-15 would show as 1e-9, while the reference's own operations
// on the same chi and S give the reference's bits wherever no exponential is involved.  S: the source function of this depth,
// adz: the distance to the depth behind
template <int NM>
__device__ __forceinline__ void linear_step_ref(int s, bool last, double adz, const double (&zmu)[NM], const double (&chi)[NM],
                                                const double (&S)[NM], double (&Iu)[NM], double (&c_k)[NM], double (&S_k)[NM],
                                                double (&dtau_prev)[NM], const lds_f64* etab)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        if (s == 0) {
            S_k[m] = S[m];
            c_k[m] = chi[m];
            continue;
        }
        const double dtau = 0.5 * (c_k[m] + chi[m]) * zmu[m] * adz;         // :107, :129
        const double dS = (S_k[m] - S[m]) / dtau;                           // :111, :130
        double w0, w1;
        w2(last ? dtau_prev[m] : dtau, w0, w1, etab);
        const double Sx = last ? S_k[m] : S[m];
        Iu[m] = Iu[m] * (1.0 - w0) + w0 * Sx + w1 * dS;                     // :126
        dtau_prev[m] = dtau;
        c_k[m] = chi[m];
        S_k[m] = S[m];
    }
}

// monotonic parabolic rule (include/lsx.h, N4) as the sweep's generic instance, for ONE ray: a depth is finished when its downwind
// neighbour is known.  (c_d, S_d): the depth that arrives, at height zk; zk1, zk2: the heights of the two depths behind.  From step 2
// on Iu becomes the intensity at the depth behind; then the window shifts: u = two behind, k = one behind.  The caller loops over its
// rays, so that its S_d = eta / chi stays inside that loop
__device__ __forceinline__ void parabolic_step(int s, double zk, double zk1, double zk2, double zmu, double c_d, double S_d, double& Iu,
                                               double& c_k, double& S_k, double& c_u, double& S_u, const lds_f64* etab)
{
    if (s >= 2) {
        const double dtau_u = (c_u + c_k) * (0.5 * fabs(zk2 - zk1)) * zmu;
        const double dtau_d = (c_k + c_d) * (0.5 * fabs(zk1 - zk)) * zmu;
        Iu = parabolic_point(Iu, S_u, S_k, S_d, dtau_u, dtau_d, true, etab).I;
    }
    c_u = c_k; S_u = S_k;
    c_k = c_d; S_k = S_d;
}

// ... and its end point: no downwind neighbour (the linear rule with its own interval's weights)
template <int NM>
__device__ __forceinline__ void parabolic_end(double zk1, double zk2, const double (&zmu)[NM], double (&Iu)[NM], const double (&c_k)[NM],
                                              const double (&S_k)[NM], const double (&c_u)[NM], const double (&S_u)[NM], const lds_f64* etab)
{
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const double dtau_u = (c_u[m] + c_k[m]) * (0.5 * fabs(zk2 - zk1)) * zmu[m];
        Iu[m] = parabolic_point(Iu[m], S_u[m], S_k[m], 0.0, dtau_u, 1.0, false, etab).I;
    }
}

} // namespace lsxd
