// lsx_stokes_host.cpp -- the formulas of lsx_stokes_dev.h compiled for the CPU: a test-only library (liblsx_stokes_host.so,
// `make stokeshost`) that evaluates the Faraday-Voigt function, the geometry, the propagation matrix and the DELO-linear solve as the
// kernel of lsx_stokes.hip does, so that the kernel can be compared with them and their properties checked without a GPU, and so that
// they run under -fsanitize=address,undefined (lsx_stokes_san_main.cpp).  Built with -ffp-contract=off.
// `ulp` (test only): every exp(-dtau) is moved by that many ulp (+1 / -1: the envelope hook of tests/envelope.py, applied here).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

// lsx_voigt.h and the device header are written for the device compiler: what they need from it, for g++
#define __device__
#define __forceinline__ inline
static inline void sincospi(double x, double* s, double* c)
{
    const double r = std::fmod(x, 2.0);          // exact
    *s = std::sin(M_PI * r);
    *c = std::cos(M_PI * r);
}
#include "lsx_stokes_dev.h"
#include "lsx_stokes_prep.h"
#include "lsx_voigt.h"

using namespace lsxst;

namespace {

struct W2Host {                 // formal_solver.py:14-44 in the regimes of the device's w2 (lsx_dev.h)
    int ulp;
    void operator()(double dtau, double& w0, double& w1) const
    {
        if (dtau < 5e-4) {
            w0 = dtau * (1.0 - 0.5 * dtau);
            w1 = (dtau * dtau) * (0.5 - dtau * (1.0 / 3.0));
            return;
        }
        const double dc = dtau < 700.0 ? dtau : 700.0;
        double e = std::exp(-dc);
        for (int u = 0; u < ulp; ++u) e = std::nextafter(e, INFINITY);
        for (int u = 0; u > ulp; --u) e = std::nextafter(e, -INFINITY);
        w0 = 1.0 - e;
        w1 = w0 - dc * e;
    }
};

const double* voigt_table()
{
    static double W[56];
    static bool made = false;
    if (!made) {
        for (int g = 0; g < 2; ++g)
            for (int n = -14; n <= 13; ++n) { const double x = (n + 0.5 * g) * 0.5; W[g * 28 + n + 14] = std::exp(-x * x); }
        made = true;
    }
    return W;
}

void acc_out(const Acc& a, double* o)
{
    const double v[11] = {a.eI, a.eQ, a.eU, a.eV, a.rQ, a.rU, a.rV, a.mI, a.mQ, a.mU, a.mV};
    std::memcpy(o, v, sizeof v);
}

Acc acc_in(const double* o)
{
    Acc a;
    a.eI = o[0]; a.eQ = o[1]; a.eU = o[2]; a.eV = o[3]; a.rQ = o[4]; a.rU = o[5]; a.rV = o[6];
    a.mI = o[7]; a.mQ = o[8]; a.mU = o[9]; a.mV = o[10];
    return a;
}

// the walk of k_stokes_rays along one ray: acc(k) gives the depth's eta, rho, eps
template <class AccAt>
void walk(int Ns, const double* z, double mu, bool thermal, double Be, double Bn, int ulp, bool endpoint, AccAt acc_at, double* out)
{
    const W2Host wf{ulp};
    const double zmu = 1.0 / mu;
    Ray ray;
    ray_init(ray);
    double zk1 = 0.0;
    for (int k = Ns - 1; k >= 0; --k) {
        const int s = Ns - 1 - k;
        const double zk = z[k];
        const Acc a = acc_at(k);
        const double adz = std::fabs(zk1 - zk);
        if (s == 0) ray_set(ray, a);
        else {
            if (s == 1 && thermal) ray.I = thermal_start(Be, Bn, adz * zmu, ray.eI, a.eI);
            delo_step(ray, a, adz * zmu, wf, endpoint && k == 0);
        }
        zk1 = zk;
    }
    out[0] = ray.I; out[1] = ray.Q; out[2] = ray.U; out[3] = ray.V;
}

// the lines handed over to lsx_stokes_host_window / lsx_stokes_host_response and what a point of a ray makes of them: eta, rho, eps
// of wavelength q at depth k with the field (Bk, gk, xk) and the line-of-sight velocity vl there
struct WindowLines {
    int Ns, nla, nlines;
    const double *wav, *chi_c, *eta_c, *lambda0, *nd, *ne, *aD, *vB, *vlos;
    const uint8_t* active;
    const int32_t* line;
    const double *tab, *W;

    Acc at(int q, int k, double Bk, double gk, double xk, double vl, double mu) const
    {
        const double w = wav[q];
        Acc a;
        acc_init(a, chi_c[(size_t)q * Ns + k], eta_c[(size_t)q * Ns + k]);
        const Geo g = geometry(gk, xk, mu);
        for (int l = 0; l < nlines; ++l) {
            if (!active[(size_t)l * nla + q]) continue;
            const size_t x = (size_t)l * Ns + k;
            const int nc = line[2 * l];
            const double vb = vB[x], l0 = lambda0[l];
            const double v = (w - l0) * kCLight / (vb * l0);
            const double rn = 1.0 / (std::sqrt(M_PI) * vb);
            const double vZ = nc > 0 ? kLarmor * (kNM_TO_M * l0) * Bk / vb : 0.0;
            const Prof pr = line_profiles(nc, tab + kCompDoubles * line[2 * l + 1], aD[x], v + 1.0 * (mu * vl / vb), vZ, W);
            if (nc > 0) line_add(a, nd[x], ne[x], pr, rn, g);
            else line_add_plain(a, nd[x], ne[x], pr, rn);
        }
        return a;
    }
};

} // namespace

extern "C" {

// w(v + i a) = H + i F for n pairs; Hv: dev_voigt's H (lsx_voigt.h) of the same pairs
void lsx_stokes_host_w(int64_t n, const double* a, const double* v, double* H, double* F, double* Hv)
{
    const double* W = voigt_table();
    for (int64_t i = 0; i < n; ++i) {
        faraday_voigt(a[i], v[i], W, H[i], F[i]);
        if (Hv) Hv[i] = dev_voigt(a[i], v[i], W);
    }
}

// n triples (gammaB, chiB, mu) -> out [n][4] = (c, s2, sQ, sU)
void lsx_stokes_host_geometry(int64_t n, const double* gammaB, const double* chiB, const double* mu, double* out)
{
    for (int64_t i = 0; i < n; ++i) {
        const Geo g = geometry(gammaB[i], chiB[i], mu[i]);
        out[4 * i] = g.c; out[4 * i + 1] = g.s2; out[4 * i + 2] = g.sQ; out[4 * i + 3] = g.sU;
    }
}

// the argument rules of the entry: -> the code lsx_hip_stokes_rays returns for this field (count points) and these patterns
int lsx_stokes_host_check(int64_t count, const double* B, const double* gammaB, const double* chiB, int32_t nlines,
                          const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift)
{
    std::string msg;
    int rc = count > 0 ? check_field((size_t)count, B, gammaB, chiB, msg) : LSX_OK;
    if (!rc) rc = check_patterns(nlines, ncomp, alpha, strength, shift, msg);
    if (!rc) {
        std::vector<uint8_t> wanted((size_t)(nlines > 0 ? nlines : 1), 1);
        std::vector<int32_t> line;
        std::vector<double> tab;
        rc = pack_patterns(nlines, ncomp, alpha, strength, shift, wanted, line, tab, msg);
    }
    return rc;
}

// The propagation matrix and the emission vector at ONE point of one ray: chi_c, eta_c the unpolarised part; nlines lines with
// nd, ne (the line's opacity and emissivity without its profile), aD, v (the Doppler offset, velocity included), vZ (the splitting of
// unit shift in Doppler widths), rn = 1 / (sqrt(pi) vBroad), each [nlines]; patterns as the entry takes them.
// -> out[11] = eta_I, eta_Q, eta_U, eta_V, rho_Q, rho_U, rho_V, eps_I, eps_Q, eps_U, eps_V.  Returns the code of the rules.
int lsx_stokes_host_K(double chi_c, double eta_c, int32_t nlines, const double* nd, const double* ne, const double* aD, const double* v,
                      const double* vZ, const double* rn, const int32_t* ncomp, const int32_t* alpha, const double* strength,
                      const double* shift, double gammaB, double chiB, double mu, double* out)
{
    std::string msg;
    int rc = check_patterns(nlines, ncomp, alpha, strength, shift, msg);
    if (rc) return rc;
    std::vector<uint8_t> wanted((size_t)(nlines > 0 ? nlines : 1), 1);
    std::vector<int32_t> line;
    std::vector<double> tab;
    if ((rc = pack_patterns(nlines, ncomp, alpha, strength, shift, wanted, line, tab, msg))) return rc;
    tab.resize(tab.size() + kCompDoubles, 0.0);
    const Geo g = geometry(gammaB, chiB, mu);
    Acc a;
    acc_init(a, chi_c, eta_c);
    for (int l = 0; l < nlines; ++l) {
        const Prof pr = line_profiles(line[2 * l], tab.data() + kCompDoubles * line[2 * l + 1], aD[l], v[l], line[2 * l] > 0 ? vZ[l] : 0.0,
                                      voigt_table());
        if (line[2 * l] > 0) line_add(a, nd[l], ne[l], pr, rn[l], g);
        else line_add_plain(a, nd[l], ne[l], pr, rn[l]);
    }
    acc_out(a, out);
    return LSX_OK;
}

// One ray through Ns depths of given matrices: z [Ns] heights, K [Ns][11] as lsx_stokes_host_K writes them, mu; thermal != 0: the
// start value of the thermalised lower end from Be, Bn (the Planck function at the last and the last but one depth), else 0.
// endpoint != 0: as the kernel does it, with the reference's end-point term in I; 0: the plain DELO-linear step at the end point too
// (test only: the rule's order of convergence).  -> out[4] = I, Q, U, V at depth 0
int lsx_stokes_host_ray(int32_t Ns, const double* z, const double* K, double mu, int32_t thermal, double Be, double Bn, int32_t ulp,
                        int32_t endpoint, double* out)
{
    if (Ns < 3 || !z || !K || !out || !(mu > 0.0 && mu <= 1.0)) return LSX_EINVAL;
    walk(Ns, z, mu, thermal != 0, Be, Bn, ulp, endpoint != 0, [&](int k) { return acc_in(K + 11 * (size_t)k); }, out);
    return LSX_OK;
}

// What k_stokes_rays computes for one column, one angle and a window of nla wavelengths wav [nla] (nm): chi_c, eta_c [nla][Ns] hold
// everything that is NOT one of the nlines lines handed over here (background, sigma J, continua, lines whose profile is read from
// the context's store); a line l has lambda0 [nm], nd, ne, aD, vB [nlines][Ns] (opacity and emissivity without the profile, damping,
// Doppler width of its atom), active [nlines][nla] and its pattern (ncomp 0: unpolarised, one evaluation of the same function).
// vlos, B, gammaB, chiB, temperature, z: [Ns]; endpoint as in lsx_stokes_host_ray.  -> out [4][nla].  Returns the code of the entry's rules for field and patterns.
int lsx_stokes_host_window(int32_t Ns, int32_t nla, const double* z, const double* temperature, const double* wav, const double* chi_c,
                           const double* eta_c, int32_t nlines, const double* lambda0, const double* nd, const double* ne,
                           const double* aD, const double* vB, const uint8_t* active, const int32_t* ncomp, const int32_t* alpha,
                           const double* strength, const double* shift, const double* vlos, const double* B, const double* gammaB,
                           const double* chiB, double mu, int32_t lower_zero, int32_t ulp, int32_t endpoint, double* out)
{
    if (Ns < 3 || nla < 1 || !(mu > 0.0 && mu <= 1.0)) return LSX_EINVAL;
    std::string msg;
    int rc = check_field((size_t)Ns, B, gammaB, chiB, msg);
    if (!rc) rc = check_patterns(nlines, ncomp, alpha, strength, shift, msg);
    if (rc) return rc;
    std::vector<uint8_t> wanted((size_t)(nlines > 0 ? nlines : 1), 1);
    std::vector<int32_t> line;
    std::vector<double> tab;
    if ((rc = pack_patterns(nlines, ncomp, alpha, strength, shift, wanted, line, tab, msg))) return rc;
    tab.resize(tab.size() + kCompDoubles, 0.0);
    const WindowLines wl{Ns, nla, nlines, wav, chi_c, eta_c, lambda0, nd, ne, aD, vB, vlos, active, line.data(), tab.data(), voigt_table()};
    for (int q = 0; q < nla; ++q) {
        const double w = wav[q];
        auto acc_at = [&](int k) { return wl.at(q, k, B[k], gammaB[k], chiB[k], vlos[k], mu); };
        double o[4];
        walk(Ns, z, mu, !lower_zero, planck(temperature[Ns - 1], w), planck(temperature[Ns - 2], w), ulp, endpoint != 0, acc_at, o);
        for (int s = 0; s < 4; ++s) out[(size_t)s * nla + q] = o[s];
    }
    return LSX_OK;
}

} // extern "C"

namespace {

// lsx_stokes_host_response (nmax 3) and lsx_stokes_host_response_v (nmax 4: bit 8, vlos, and amplitude[4]) below
int response_host(int nmax, int32_t Ns, int32_t nla, const double* z, const double* temperature, const double* wav, const double* chi_c,
                  const double* eta_c, int32_t nlines, const double* lambda0, const double* nd, const double* ne,
                  const double* aD, const double* vB, const uint8_t* active, const int32_t* ncomp, const int32_t* alpha,
                  const double* strength, const double* shift, const double* vlos, const double* B, const double* gammaB,
                  const double* chiB, double mu, int32_t lower_zero, int32_t ulp, uint32_t params, const double* amplitude,
                  int32_t nk, const int32_t* ks, double* rf, double* stokes)
{
    if (Ns < 3 || nla < 1 || !(mu > 0.0 && mu <= 1.0) || !rf || !vlos) return LSX_EINVAL;
    std::string msg;
    int rc = check_field((size_t)Ns, B, gammaB, chiB, msg);
    if (!rc && nmax > 3) rc = check_velocity((size_t)Ns, vlos, msg);
    if (!rc) rc = check_patterns(nlines, ncomp, alpha, strength, shift, msg);
    if (!rc) rc = check_response(params, amplitude, Ns, nk, ks, 1, 0, B, msg, nmax);
    if (rc) return rc;
    std::vector<uint8_t> wanted((size_t)(nlines > 0 ? nlines : 1), 1);
    std::vector<int32_t> line;
    std::vector<double> tab;
    if ((rc = pack_patterns(nlines, ncomp, alpha, strength, shift, wanted, line, tab, msg))) return rc;
    tab.resize(tab.size() + kCompDoubles, 0.0);
    int par[kMaxResponseParams] = {0, 0, 0, 0};
    const int npar = response_params(params, par);
    const int nvar = 1 + 2 * npar, nkk = ks ? nk : Ns;
    double amp[kMaxResponseParams] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < npar; ++i) amp[i] = amplitude[par[i]];
    std::vector<uint8_t> kreq((size_t)Ns, ks ? 0 : 1);
    for (int i = 0; i < nkk && ks; ++i) kreq[ks[i]] = 1;
    const WindowLines wl{Ns, nla, nlines, wav, chi_c, eta_c, lambda0, nd, ne, aD, vB, vlos, active, line.data(), tab.data(), voigt_table()};
    // ---- stage 1: [nvar][Ns][11][nla]; a variant's node is formed (and read) at requested depths only ----
    const size_t S = (size_t)nla;
    std::vector<double> nodes((size_t)nvar * Ns * kNodeDoubles * S, NAN), state((size_t)Ns * kStateDoubles * S, NAN);
    for (int k = 0; k < Ns; ++k)
        for (int var = 0; var < nvar; ++var) {
            if (var > 0 && !kreq[k]) continue;
            double Bk = B[k], gk = gammaB[k], xk = chiB[k], vlk = vlos[k];
            if (var > 0) field_variant(par[(var - 1) >> 1], ((var - 1) & 1) == 0, amp[(var - 1) >> 1], Bk, gk, xk, vlk);
            for (int q = 0; q < nla; ++q)
                node_store(wl.at(q, k, Bk, gk, xk, vlk, mu), nodes.data() + ((size_t)var * Ns + k) * kNodeDoubles * S + q, S);
        }
    // ---- stage 2 ----
    const W2Host wf{ulp};
    for (int q = 0; q < nla; ++q) {
        const auto zat = [&](int k) { return z[k]; };
        const auto nod = [&](Acc& n, int var, int k) { node_load(n, nodes.data() + ((size_t)var * Ns + k) * kNodeDoubles * S + q, S); };
        struct StateHost {
            double* base;
            size_t S;
            void put(int k, const Ray& r) const
            {
                double* s = base + (size_t)k * kStateDoubles * S;
                s[0] = r.I; s[S] = r.Q; s[2 * S] = r.U; s[3 * S] = r.V; s[4 * S] = r.dt;
            }
            void get(int k, Ray& r) const
            {
                const double* s = base + (size_t)k * kStateDoubles * S;
                r.I = s[0]; r.Q = s[S]; r.U = s[2 * S]; r.V = s[3 * S]; r.dt = s[4 * S];
            }
        };
        const StateHost st{state.data() + q, S};
        const auto out = [&](int i, int jk, const double (&o)[4]) {
            for (int c = 0; c < 4; ++c) rf[(((size_t)i * 4 + c) * nla + q) * nkk + jk] = o[c];
        };
        double Sv[4];
        response_walk(Ns, zat, 1.0 / mu, !lower_zero, planck(temperature[Ns - 1], wav[q]), planck(temperature[Ns - 2], wav[q]), wf, nod, st,
                      npar, amp, nkk, ks, out, Sv);
        for (int c = 0; c < 4 && stokes; ++c) stokes[(size_t)c * nla + q] = Sv[c];
    }
    return LSX_OK;
}

} // namespace

extern "C" {

// What lsx_hip_response_stokes computes for one column, one angle and a window (include/lsx_hip_stokes_response.h), by its two
// stages through the same header functions: the nodes of every depth under every field variant (node_store), then response_walk.
// Arguments as lsx_stokes_host_window (the end point as the kernel has it), then params, amplitude[3], nk, ks (null: all depths).
// -> rf [npar][4][nla][nk], stokes [4][nla] (may be null).  Returns the code of the entry's rules for field, patterns and these.
int lsx_stokes_host_response(int32_t Ns, int32_t nla, const double* z, const double* temperature, const double* wav, const double* chi_c,
                             const double* eta_c, int32_t nlines, const double* lambda0, const double* nd, const double* ne,
                             const double* aD, const double* vB, const uint8_t* active, const int32_t* ncomp, const int32_t* alpha,
                             const double* strength, const double* shift, const double* vlos, const double* B, const double* gammaB,
                             const double* chiB, double mu, int32_t lower_zero, int32_t ulp, uint32_t params, const double* amplitude,
                             int32_t nk, const int32_t* ks, double* rf, double* stokes)
{
    return response_host(3, Ns, nla, z, temperature, wav, chi_c, eta_c, nlines, lambda0, nd, ne, aD, vB, active, ncomp, alpha, strength, shift, vlos,
                         B, gammaB, chiB, mu, lower_zero, ulp, params, amplitude, nk, ks, rf, stokes);
}

// What lsx_hip_velocity_response_stokes computes (include/lsx_hip_stokes_velocity.h): the same arguments, the velocity handed over IS
// vlos here, with bit 8 of params (the response to vlos, the fourth of rf's parameters) and amplitude[4].  The rows of B, gammaB and
// chiB are those of lsx_stokes_host_response bit for bit: one function, and the variants of the field leave the velocity alone.
int lsx_stokes_host_response_v(int32_t Ns, int32_t nla, const double* z, const double* temperature, const double* wav, const double* chi_c,
                               const double* eta_c, int32_t nlines, const double* lambda0, const double* nd, const double* ne,
                               const double* aD, const double* vB, const uint8_t* active, const int32_t* ncomp, const int32_t* alpha,
                               const double* strength, const double* shift, const double* vlos, const double* B, const double* gammaB,
                               const double* chiB, double mu, int32_t lower_zero, int32_t ulp, uint32_t params, const double* amplitude,
                               int32_t nk, const int32_t* ks, double* rf, double* stokes)
{
    return response_host(4, Ns, nla, z, temperature, wav, chi_c, eta_c, nlines, lambda0, nd, ne, aD, vB, active, ncomp, alpha, strength, shift, vlos,
                         B, gammaB, chiB, mu, lower_zero, ulp, params, amplitude, nk, ks, rf, stokes);
}

} // extern "C"
