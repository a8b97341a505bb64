// lsx_stokes_dev.h -- the formulas of the polarised final pass (include/lsx_hip_stokes.h) as functions that a host
// compiler also accepts: lsx_stokes.hip and lsx_stokes_response.hip run them on the device, lsx_stokes_host.cpp on the CPU for the tests.
//
//   faraday_voigt     w(v + i a) = H + i F: the trapezoid sum and pole term of dev_voigt (lsx_voigt.h) with the imaginary parts kept
//   geometry          the field's direction cosines against a ray and its sky-plane basis
//   line_profiles     phi_q, psi_q, q = -1, 0, +1: the sums over a line's Zeeman components
//   line_add          a line's share of the propagation matrix and the emission vector (Landi Degl'Innocenti & Landolfi 2004, 9.32)
//   delo_step         one step of the DELO-linear rule (Rees, Murphy & Durrant 1989) with the 4 x 4 solve in registers
//   response_walk     the two walks of the response functions to the field (lsx_stokes_response.hip): up over stored nodes keeping the
//                     ray's state, down with the 4 x 4 transfer matrix (transfer_step) and the replay of the steps a depth's node enters
// Nothing here comes from the reference, which has no polarised formal solution.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LSXST_HD __device__ __forceinline__
#define LSXST_UNROLL _Pragma("unroll")
#define LSXST_UNROLL4 _Pragma("unroll 4")
#else
#define LSXST_HD inline
#define LSXST_UNROLL
#define LSXST_UNROLL4
#endif

namespace lsxst {

constexpr double kCLight = 2.99792458E+08;
constexpr double kHPlanck = 6.6260755E-34;
constexpr double kKBoltzmann = 1.380658E-23;
constexpr double kNM_TO_M = 1.0E-09;
constexpr double kHC = kHPlanck * kCLight;
constexpr double kQElectron = 1.60217733E-19;
constexpr double kMElectron = 9.1093897E-31;
// e / (4 pi m_e) [1 / (T s)]: the Larmor frequency per tesla.  vB = kLarmor lambda0[m] B / vBroad is the splitting of a component with
// unit shift in Doppler widths
constexpr double kLarmor = kQElectron / (4.0 * M_PI * kMElectron);
// a component of a pattern as the kernels read it: its shift and its strength as the weight of phi_-1, phi_0 or phi_+1 (two of the
// three are zero: no register array is indexed by alpha)
constexpr int kCompDoubles = 4;

// utils.py:17-22.  planck, thermal_start below and the constants above RESTATE lsx_final_dev.h (which a host compiler cannot read: it
// includes the HIP runtime) and must move with it: tests/test_stokes_host.py compares the two texts, and with no pattern the
// kernel's I is held against the pass that uses the other copy (tests/test_stokes.py, FALC)
LSXST_HD double planck(double temp, double wav)
{
    const double hc_Tkla = kHC / (kKBoltzmann * kNM_TO_M * wav) / temp;
    const double x = kNM_TO_M * wav;
    const double twohnu3_c2 = (2.0 * kHC) / (x * x * x);
    return twohnu3_c2 / (exp(hc_Tkla) - 1.0);
}

// w(v + i a) = H + i F, a >= 0.  dev_voigt's rule (lsx_voigt.h) term by term: the real parts are its operations in its order (on a host
// build without contraction H has its bits); the imaginary part of a node's term is (x - g_n) / ((x - g_n)^2 + a^2), that of the pole's
// residue -2 exp(a^2 - x^2) (c1 di + s1 dr) / |D|^2.  F is odd in v: it is formed at |v| and takes v's sign.
template <typename WP>
LSXST_HD void faraday_voigt(double a, double v, WP W, double& H, double& F)
{
    const double h = 0.5;
    const double x = fabs(v);
    const double t = x * 2.0, fr = t - floor(t);
    const bool half = !(fr >= 0.25 && fr < 0.75);
    const double shift = half ? 0.5 : 0.0;
    const WP w = W + (half ? 28 : 0);
    const double a2 = a * a;
    double s = 0.0, sf = 0.0;
    LSXST_UNROLL4
    for (int n = -14; n <= 13; ++n) {
        const double d = x - ((double)n + shift) * h;
        const double q = w[n + 14] / (d * d + a2);
        s += q;
        sf += q * d;
    }
    double Hh = (h / M_PI) * a * s;
    double Fh = (h / M_PI) * sf;
    if (x < 27.0 && a < 2.0 * M_PI) {
        double s1, c1, st, ct;
        sincos(2.0 * x * a, &s1, &c1);
        sincospi(4.0 * x, &st, &ct);
        const double er = exp(a2 - x * x), E = exp(4.0 * M_PI * a), sg = half ? 1.0 : -1.0;
        const double dr = 1.0 + sg * E * ct, di = -sg * E * st;
        const double den = dr * dr + di * di;
        Hh += 2.0 * er * (c1 * dr - s1 * di) / den;
        Fh -= 2.0 * er * (c1 * di + s1 * dr) / den;
    }
    H = Hh;
    F = v < 0.0 ? -Fh : Fh;
}

// The field b = (sin g cos x, sin g sin x, cos g) (g, x: inclination and azimuth against the vertical) seen along the ray
// l = (sqrt(1 - mu^2), 0, mu) with the sky-plane basis e1 = (mu, 0, -sqrt(1 - mu^2)), e2 = (0, 1, 0); +Q along e1.
//   c = b.l = cos g',  s2 = sin^2 g',  sQ = sin^2 g' cos 2x',  sU = sin^2 g' sin 2x'   (g', x': against the ray).  No division.
struct Geo { double c, s2, sQ, sU; };
LSXST_HD Geo geometry(double gammaB, double chiB, double mu)
{
    double sg, cg, sx, cx;
    sincos(gammaB, &sg, &cg);
    sincos(chiB, &sx, &cx);
    const double st = sqrt((1.0 - mu) * (1.0 + mu));
    const double bx = sg * cx, by = sg * sx, bz = cg;
    const double b1 = bx * mu - bz * st, b2 = by;
    Geo g;
    g.c = bx * st + bz * mu;
    g.s2 = b1 * b1 + b2 * b2;
    g.sQ = b1 * b1 - b2 * b2;
    g.sU = 2.0 * b1 * b2;
    return g;
}

// phi_q = sum_{k: alpha_k = q} strength_k H(a, v - shift_k vB), psi_q the same with F (not yet divided by sqrt(pi) vBroad).
// tab: ncomp x (shift, weight of q = -1, of q = 0, of q = +1).  vB == 0 (no field at this depth, or an unpolarised line; wave-uniform):
// every component sits at v and every strength sum is 1: ONE evaluation with the weights (1, 1, 1), through the same loop (one copy
// of the function in a kernel).  Then phi_0 - (phi_+1 + phi_-1) / 2 and phi_+1 - phi_-1 are 0.0 exactly.
struct Prof { double pm, p0, pp, fm, f0, fp; };
template <typename WP, typename TP>
LSXST_HD Prof line_profiles(int ncomp, TP tab, double a, double v, double vB, WP W)
{
    Prof p;
    p.pm = p.p0 = p.pp = p.fm = p.f0 = p.fp = 0.0;
    const bool one = vB == 0.0;
    const int n = one ? 1 : ncomp;
    for (int k = 0; k < n; ++k) {
        const double sh = one ? 0.0 : tab[kCompDoubles * k], wm = one ? 1.0 : tab[kCompDoubles * k + 1];
        const double w0 = one ? 1.0 : tab[kCompDoubles * k + 2], wp = one ? 1.0 : tab[kCompDoubles * k + 3];
        double H, F;
        faraday_voigt(a, v - sh * vB, W, H, F);
        p.pm += wm * H; p.p0 += w0 * H; p.pp += wp * H;
        p.fm += wm * F; p.f0 += w0 * F; p.fp += wp * F;
    }
    return p;
}

// absorption eta_I..V, anomalous dispersion rho_Q..V, emission eps_I..V at one depth of one ray
struct Acc { double eI, eQ, eU, eV, rQ, rU, rV, mI, mQ, mU, mV; };
LSXST_HD void acc_init(Acc& a, double chi_c, double eta_c)
{
    a.eI = chi_c; a.mI = eta_c;
    a.eQ = a.eU = a.eV = a.rQ = a.rU = a.rV = a.mQ = a.mU = a.mV = 0.0;
}

// a polarised line: nd = (h nu / 4 pi)(n_i B_ij - n_j B_ji), ne = n_j A_ji h nu / 4 pi, rn = 1 / (sqrt(pi) vBroad)
LSXST_HD void line_add(Acc& a, double nd, double ne, const Prof& p, double rn, const Geo& g)
{
    const double ps = 0.5 * (p.pp + p.pm), fs = 0.5 * (p.fp + p.fm);
    const double phiI = 0.5 * (p.p0 * g.s2 + ps * (1.0 + g.c * g.c)) * rn;
    const double dq = 0.5 * (p.p0 - ps) * rn, df = 0.5 * (p.f0 - fs) * rn;
    const double phiQ = dq * g.sQ, phiU = dq * g.sU, phiV = 0.5 * (p.pp - p.pm) * g.c * rn;
    const double psiQ = df * g.sQ, psiU = df * g.sU, psiV = 0.5 * (p.fp - p.fm) * g.c * rn;
    a.eI += nd * phiI; a.eQ += nd * phiQ; a.eU += nd * phiU; a.eV += nd * phiV;
    a.rQ += nd * psiQ; a.rU += nd * psiU; a.rV += nd * psiV;
    a.mI += ne * phiI; a.mQ += ne * phiQ; a.mU += ne * phiU; a.mV += ne * phiV;
}

// a line without a pattern (ray dependent: its profile is formed here): H rn into eta_I and eps_I alone, as k_emergent_rays adds it
// -- not through the geometry, whose c^2 + s^2 is 1 only to rounding: an unpolarised line does not feel the field's direction
LSXST_HD void line_add_plain(Acc& a, double nd, double ne, const Prof& p, double rn)
{
    const double pv = p.p0 * rn;
    a.eI += nd * pv;
    a.mI += ne * pv;
}

// The state of a ray: the Stokes vector at the depth behind, and that depth's eta_I, K' = K / eta_I - 1 (its six distinct
// off-diagonal entries) and S' = eps / eta_I, and the optical thickness of the interval behind that depth (the end point's weights)
struct Ray { double I, Q, U, V, eI, q, u, v, rq, ru, rv, SI, SQ, SU, SV, dt; };
LSXST_HD void ray_init(Ray& r)
{
    r.I = r.Q = r.U = r.V = 0.0;
    r.eI = 1.0;
    r.dt = 1.0;
    r.q = r.u = r.v = r.rq = r.ru = r.rv = r.SI = r.SQ = r.SU = r.SV = 0.0;
}
LSXST_HD void ray_set(Ray& r, const Acc& a)
{
    const double rI = 1.0 / a.eI;
    r.eI = a.eI;
    r.q = a.eQ * rI; r.u = a.eU * rI; r.v = a.eV * rI;
    r.rq = a.rQ * rI; r.ru = a.rU * rI; r.rv = a.rV * rI;
    r.SI = a.mI * rI; r.SQ = a.mQ * rI; r.SU = a.mU * rI; r.SV = a.mV * rI;
}

// the value a ray starts with at a thermalised lower end (formal_solver.py:203-207), unpolarised: Be, Bn the Planck function at the
// end's depth and at the next one, adz_zmu = |dz| / mu, c_k and chi their eta_I
LSXST_HD double thermal_start(double Be, double Bn, double adz_zmu, double c_k, double chi)
{
    const double dtau_uw = (c_k + chi) * 0.5 * adz_zmu;
    return Be - (Bn - Be) / dtau_uw;
}

// DELO-linear from the depth behind (u: the ray's state) to this depth (k: acc), adz_zmu = |dz| / mu:
//   dtau = (eta_I,u + eta_I,k) / 2 |dz| / mu,  E = exp(-dtau),  F = 1 - E = w0,  G = w1 / dtau  (w0, w1: wf, the linear rule's weights)
//   [1 + (F - G) K'_k] I_k = [E - G K'_u] I_u + (F - G) S'_k + G S'_u
// The system's symmetric part 1 + (F - G) [eta' block] is positive definite (F - G < 1, |eta_Q,U,V| <= eta_I) and the rho' block is
// antisymmetric: Gaussian elimination without pivoting meets no zero pivot.  With K' = 0 this is the linear rule.
// last (the ray's end point, wave-uniform): the reference's linear rule treats its end point apart (formal_solver.py:138-139: the
// weights of the PREVIOUS interval and the source function of the depth behind, with this interval's slope), and that is what the
// unpolarised final passes restate.  So that I without a field is their I, the same scalar term is carried here as a correction of I
// from S'_I: the difference between that end-point form and the plain linear step (zero where the two intervals and source
// functions agree; the top interval is optically thin: measured 2e-9 I on FALC Ca II).  The polarised step itself stays the DELO step:
// the end-point form put INTO the system would weight K'_k with -w1 / dtau, which is not bounded by 1.
template <class W2F>
LSXST_HD void delo_step(Ray& r, const Acc& a, double adz_zmu, const W2F& wf, bool last)
{
    Ray n;
    ray_set(n, a);
    const double dtau = 0.5 * (r.eI + a.eI) * adz_zmu;
    double w0, w1;
    wf(dtau, w0, w1);
    const double E = 1.0 - w0, G = w1 / dtau, Fa = w0 - G;
    const double k0 = r.q * r.Q + r.u * r.U + r.v * r.V;
    const double k1 = r.q * r.I + r.rv * r.U - r.ru * r.V;
    const double k2 = r.u * r.I - r.rv * r.Q + r.rq * r.V;
    const double k3 = r.v * r.I + r.ru * r.Q - r.rq * r.U;
    double b[4] = {E * r.I - G * k0 + Fa * n.SI + G * r.SI, E * r.Q - G * k1 + Fa * n.SQ + G * r.SQ,
                   E * r.U - G * k2 + Fa * n.SU + G * r.SU, E * r.V - G * k3 + Fa * n.SV + G * r.SV};
    double A[4][4] = {{1.0, Fa * n.q, Fa * n.u, Fa * n.v},
                      {Fa * n.q, 1.0, Fa * n.rv, -(Fa * n.ru)},
                      {Fa * n.u, -(Fa * n.rv), 1.0, Fa * n.rq},
                      {Fa * n.v, Fa * n.ru, -(Fa * n.rq), 1.0}};
    LSXST_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double rp = 1.0 / A[k][k];
        LSXST_UNROLL
        for (int i = k + 1; i < 4; ++i) {
            const double f = A[i][k] * rp;
            LSXST_UNROLL
            for (int j = k + 1; j < 4; ++j) A[i][j] -= f * A[k][j];
            b[i] -= f * b[k];
        }
    }
    const double x3 = b[3] / A[3][3];
    const double x2 = (b[2] - A[2][3] * x3) / A[2][2];
    const double x1 = (b[1] - A[1][2] * x2 - A[1][3] * x3) / A[1][1];
    const double x0 = b[0] - A[0][1] * x1 - A[0][2] * x2 - A[0][3] * x3;
    n.I = x0; n.Q = x1; n.U = x2; n.V = x3;
    n.dt = dtau;
    if (last) {
        double w0p, w1p;
        wf(r.dt, w0p, w1p);
        const double dS = (r.SI - n.SI) / dtau;
        n.I += r.I * (w0 - w0p) + (w0p * r.SI - w0 * n.SI) + (w1p - w1) * dS;
    }
    r = n;
}

// ---- response functions of the emergent Stokes vector to the field at one depth (include/lsx_hip_stokes_response.h) ----
// A NODE is what the solver needs of a depth, 11 doubles.  It is kept as the depth's Acc (eta, rho, eps), not as what ray_set makes of
// it (eta_I, K', S'): every step of a walk over nodes is then delo_step itself, ray_set included -- one text, and on the host build
// (no contraction) the walk up has the bits of the walk of lsx_stokes_host.cpp.  The division by eta_I is redone per step.
// Stage 1 stores the node of every depth for every field VARIANT: 0 the call's field, 1 + 2 i + s the i-th requested parameter moved
// by +a/2 (s = 0) or -a/2 (s = 1) AT THAT DEPTH.  Stage 2 (response_walk) never forms a profile.
constexpr int kNodeDoubles = 11;
constexpr int kStateDoubles = 5;       // the ray's I, Q, U, V and dt after the step into a depth

// (With a velocity in the call there are up to nine variants: the fourth parameter is vlos.)
// the field of a variant: par 0 B, 1 gammaB, 2 chiB; up: +a/2, else -a/2 (p + a/2 and p - a/2 as a caller forms them)
LSXST_HD void field_variant(int par, bool up, double amp, double& B, double& g, double& x)
{
    const double h = 0.5 * amp;
    double& t = par == 0 ? B : (par == 1 ? g : x);
    t = up ? t + h : t - h;
}
// ... in a call with a velocity (include/lsx_hip_stokes_velocity.h): par 3 moves the depth's line-of-sight velocity vl and leaves the
// field, and so the geometry, alone; par 0, 1, 2 are the function above (its text, so that those variants keep their bits)
LSXST_HD void field_variant(int par, bool up, double amp, double& B, double& g, double& x, double& vl)
{
    if (par == 3) {
        const double h = 0.5 * amp;
        vl = up ? vl + h : vl - h;
    } else {
        field_variant(par, up, amp, B, g, x);
    }
}

// node <-> 11 doubles `stride` apart (the wavelength runs fastest in the stores: stride = the window's length)
template <class P>
LSXST_HD void node_store(const Acc& a, P dst, size_t stride)
{
    dst[0] = a.eI; dst[stride] = a.eQ; dst[2 * stride] = a.eU; dst[3 * stride] = a.eV;
    dst[4 * stride] = a.rQ; dst[5 * stride] = a.rU; dst[6 * stride] = a.rV;
    dst[7 * stride] = a.mI; dst[8 * stride] = a.mQ; dst[9 * stride] = a.mU; dst[10 * stride] = a.mV;
}
template <class P>
LSXST_HD void node_load(Acc& a, P src, size_t stride)
{
    a.eI = src[0]; a.eQ = src[stride]; a.eU = src[2 * stride]; a.eV = src[3 * stride];
    a.rQ = src[4 * stride]; a.rU = src[5 * stride]; a.rV = src[6 * stride];
    a.mI = src[7 * stride]; a.mQ = src[8 * stride]; a.mU = src[9 * stride]; a.mV = src[10 * stride];
}

// The emergent vector is affine in the vector at depth m: S_0 = T_m S_m + c_m under the call's own nodes.  T <- T M, M the linear
// part of the DELO step from the depth behind (u) into this one (n):  M = A^-1 (E - G K'_u), A = 1 + (F - G) K'_n as in delo_step,
// plus, at the end point, r.I (w0 - w0p) in the I row (dt_prev: the optical thickness of the interval behind u).
// Row by row: y A = t  <=>  A^T y^T = t^T (A^T: A with the rho' block's signs turned, the same pivots' argument), then y (E - G K'_u).
template <class W2F>
LSXST_HD void transfer_step(double (&T)[4][4], const Acc& au, const Acc& an, double adz_zmu, const W2F& wf, bool last, double dt_prev)
{
    Ray u, n;
    ray_set(u, au);
    ray_set(n, an);
    const double dtau = 0.5 * (u.eI + n.eI) * adz_zmu;
    double w0, w1;
    wf(dtau, w0, w1);
    const double E = 1.0 - w0, G = w1 / dtau, Fa = w0 - G;
    double ends = 0.0;
    if (last) {
        double w0p, w1p;
        wf(dt_prev, w0p, w1p);
        ends = w0 - w0p;
    }
    double A[4][4] = {{1.0, Fa * n.q, Fa * n.u, Fa * n.v},
                      {Fa * n.q, 1.0, -(Fa * n.rv), Fa * n.ru},
                      {Fa * n.u, Fa * n.rv, 1.0, -(Fa * n.rq)},
                      {Fa * n.v, -(Fa * n.ru), Fa * n.rq, 1.0}};
    double b[4][4];                    // b[.][i]: the i-th row of T as a right-hand side
    LSXST_UNROLL
    for (int i = 0; i < 4; ++i) {
        LSXST_UNROLL
        for (int j = 0; j < 4; ++j) b[j][i] = T[i][j];
    }
    LSXST_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double rp = 1.0 / A[k][k];
        LSXST_UNROLL
        for (int i = k + 1; i < 4; ++i) {
            const double f = A[i][k] * rp;
            LSXST_UNROLL
            for (int j = k + 1; j < 4; ++j) A[i][j] -= f * A[k][j];
            LSXST_UNROLL
            for (int c = 0; c < 4; ++c) b[i][c] -= f * b[k][c];
        }
    }
    LSXST_UNROLL
    for (int c = 0; c < 4; ++c) {
        const double y3 = b[3][c] / A[3][3];
        const double y2 = (b[2][c] - A[2][3] * y3) / A[2][2];
        const double y1 = (b[1][c] - A[1][2] * y2 - A[1][3] * y3) / A[1][1];
        const double y0 = b[0][c] - A[0][1] * y1 - A[0][2] * y2 - A[0][3] * y3;
        const double t0 = T[c][0];
        T[c][0] = E * y0 - G * (y1 * u.q + y2 * u.u + y3 * u.v) + t0 * ends;
        T[c][1] = E * y1 - G * (y0 * u.q - y2 * u.rv + y3 * u.ru);
        T[c][2] = E * y2 - G * (y0 * u.u + y1 * u.rv - y3 * u.rq);
        T[c][3] = E * y3 - G * (y0 * u.v - y1 * u.ru + y2 * u.rq);
    }
}

// What a walk needs of its surroundings, as small function objects so that the device and the host run this text:
//   z(k)                      the height of depth k
//   nodes(a, var, k)          the node of depth k under variant var -> the Acc a
//   state.put(k, r)           keep r's I, Q, U, V, dt (the ray after the step into k);  state.get(k, r) the reverse
//   out(i, jk, d[4])          the response to the i-th requested parameter at the jk-th requested depth
// The steps the node of depth j enters, and so what is replayed with the node of a variant in j's place:
//   the step into j and the step into j - 1 (as the depth behind);
//   j >= Ns - 2: the thermalised start value, which reads eta_I of the two lowest depths -- the replay starts at the beginning (it
//   does so under a ZERO lower boundary too: the start is then 0 either way);
//   j <= 2: the end point's I reads dt of the interval behind it, dtau(2, 1), as well as its own -- the replay runs to the surface
//   and no T is applied.
// Otherwise the replay starts from the kept state of depth j + 1 and ends at m = j - 1, and the response is T_m (S_m^+ - S_m^-) / a.
template <class ZAt, class Nodes, class W2F>
struct ResponseRay {
    int Ns;
    double zmu;
    bool thermal;
    double Be, Bn;
    const ZAt& z;
    const Nodes& nodes;
    const W2F& wf;

    LSXST_HD void step(Ray& ray, int var, int k) const
    {
        Acc a;
        nodes(a, var, k);
        const double adz = fabs(z(k + 1) - z(k));
        if (k == Ns - 2 && thermal) ray.I = thermal_start(Be, Bn, adz * zmu, ray.eI, a.eI);
        delo_step(ray, a, adz * zmu, wf, k == 0);
    }
};

template <class ZAt, class Nodes, class State, class W2F, class Out>
LSXST_HD void response_walk(int Ns, const ZAt& z, double zmu, bool thermal, double Be, double Bn, const W2F& wf, const Nodes& nodes,
                            const State& state, int npar, const double* amp, int nk, const int32_t* ks, const Out& out, double (&S)[4])
{
    const ResponseRay<ZAt, Nodes, W2F> rr{Ns, zmu, thermal, Be, Bn, z, nodes, wf};
    // ---- up: the walk of the Stokes pass over the stored nodes of the call's own field ----
    Ray ray;
    Acc a0;
    ray_init(ray);
    nodes(a0, 0, Ns - 1);
    ray_set(ray, a0);
    for (int k = Ns - 2; k >= 0; --k) {
        rr.step(ray, 0, k);
        state.put(k, ray);
    }
    S[0] = ray.I; S[1] = ray.Q; S[2] = ray.U; S[3] = ray.V;
    // ---- down from the surface ----
    double T[4][4];
    LSXST_UNROLL
    for (int i = 0; i < 4; ++i) {
        LSXST_UNROLL
        for (int j = 0; j < 4; ++j) T[i][j] = i == j ? 1.0 : 0.0;
    }
    int m = 0;
    for (int jk = 0; jk < nk; ++jk) {
        const int j = ks ? ks[jk] : jk;
        const int k_end = j <= 2 ? 0 : j - 1;
        for (; m < k_end; ++m) {
            Acc u, n;
            nodes(u, 0, m + 1);
            nodes(n, 0, m);
            double dtp = 1.0;
            if (m == 0) {
                Ray s1;
                state.get(1, s1);
                dtp = s1.dt;
            }
            transfer_step(T, u, n, fabs(z(m + 1) - z(m)) * zmu, wf, m == 0, dtp);
        }
        for (int i = 0; i < npar; ++i) {
            double d[4] = {0.0, 0.0, 0.0, 0.0};
            for (int sg = 0; sg < 2; ++sg) {
                const int var = 1 + 2 * i + sg;
                Ray r;
                Acc a;
                ray_init(r);
                int k;
                if (j >= Ns - 2) {
                    nodes(a, j == Ns - 1 ? var : 0, Ns - 1);
                    ray_set(r, a);
                    k = Ns - 2;
                } else {
                    nodes(a, 0, j + 1);
                    ray_set(r, a);
                    state.get(j + 1, r);
                    k = j;
                }
                for (; k >= k_end; --k) rr.step(r, k == j ? var : 0, k);
                if (sg == 0) { d[0] = r.I; d[1] = r.Q; d[2] = r.U; d[3] = r.V; }
                else { d[0] -= r.I; d[1] -= r.Q; d[2] -= r.U; d[3] -= r.V; }
            }
            double o[4];
            LSXST_UNROLL
            for (int c = 0; c < 4; ++c)
                o[c] = (k_end == 0 ? d[c] : T[c][0] * d[0] + T[c][1] * d[1] + T[c][2] * d[2] + T[c][3] * d[3]) / amp[i];
            out(i, jk, o);
        }
    }
}

} // namespace lsxst
