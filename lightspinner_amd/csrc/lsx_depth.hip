// lsx_depth.hip -- depth-resolved final pass: opacity, source function, optical depth, intensity and contribution function at every
// depth along up-going rays at arbitrary viewing angles, from what a context holds (include/lsx_hip_depth.h, lsx_hip_depth_rays).
// Read-only on the context; gfx950 only.
//
// Reference lines restated here (the rest: lsx_final_dev.h, whose column set-up, start value and recurrence steps the walks use):
//   rh_method.py:599-632           opacity, emissivity, source function of the up-going ray
//   rh_method.py:231-239           line profile of the up-going ray at the new angle (ray-dependent profiles)
//   formal_solver.py:129           dtau of an interval (summed from the top: tau)
//   formal_solver.py:117           I[kStart] = Istart: I at EVERY depth
//
// Mapping (that of k_emergent_rays, lsx_rays.hip): one wavefront = 64 consecutive wavelengths of the call's window of one column, a
// lane owns one wavelength and carries a compile-time chunk of NM angles in registers.  Two walks per lane:
//   down  k = 0 .. Ns - 1: chi, eta -> S once per depth (the Voigt function once per line wavelength, depth and angle), the running
//         tau, the contribution function chi S exp(-tau) / mu and the height of tau = 1; chi, S, tau, contrib are stored;
//   up    k = Ns - 1 .. 0: the SAME lane reloads its own chi and S and runs the recurrence (the linear rule in the reference's own
//         order of operations, the parabolic rule as the sweep's generic instance); I is stored at every depth.
// The arrays are [launch column][angle][k][wavelength of the window]: a lane is a wavelength, so every store of a wavefront is one
// contiguous run, and they ARE the results -- they are copied to the host as they lie.  One writer per cell, in program order, no
// atomics.  The depth's operands of the tile-major streams are fetched one depth ahead, before the depth's stores are issued.
// LDS: the exponential's table and the Voigt function's (1.5 kB); no depth limit.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"
#include "lsx_voigt.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)256 << 20;      // bytes (include/lsx_hip_depth.h)

struct DepthParams {
    int32_t Ns, Nspect, NLtot, Natoms, NlinesA, Ncont, L, Nrays;
    int32_t col0, nmu, mu0;     // first column of the launch; angles of the call; first angle of this launch's chunk
    int32_t la0, nla;           // the call's window of the merged wavelength grid
    int32_t phi_compact, sca_per_lambda, phi_G;
    int64_t til_col, phi_col, sca_col;
    const double *wavelength, *u_la, *exp2_tab, *voigt_W, *mu;
    const int32_t* la_ptr;      // [Nspect + 1] into ents
    const FinalEnt* ents;
    const int32_t* la_tile;     // [Nspect][2]: tile, place in the tile
    const double *height, *temperature, *n, *nsr, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    const double *aDamp, *vBroad, *vlos;
    const uint8_t* prof_kind;   // per column: 2 = profiles built by the library with a line-of-sight velocity (ray dependent)
    double *chi, *S, *tau, *I, *contrib;    // each [launch column][nmu][Ns][nla]
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store), or null
    double* ztau1;              // [launch column][nmu][nla]
};

template <int NM, bool PAR>
__global__ void __launch_bounds__(64) k_depth_rays(const DepthParams p)
{
    __shared__ double etab_s[LSX_EXP_TAB + 64];      // the exponential's table and the Voigt function's (lsx_voigt.h: 56 doubles)
    for (int e = threadIdx.x; e < LSX_EXP_TAB; e += 64) etab_s[e] = p.exp2_tab[e];
    if (p.voigt_W && threadIdx.x < 56) etab_s[LSX_EXP_TAB + threadIdx.x] = p.voigt_W[threadIdx.x];
    __syncthreads();
    const lds_f64* etab = (const lds_f64*)etab_s;
    const lds_f64* vtab = etab + LSX_EXP_TAB;

    const int Ns = p.Ns, L = p.L;
    const int q_raw = blockIdx.x * 64 + threadIdx.x;       // place in the window
    const bool valid = q_raw < p.nla;
    const int q = valid ? q_raw : p.nla - 1;               // every lane walks a wavelength (w2 / w3 are wave-wide); spare ones store nothing
    const int la = p.la0 + q;
    const size_t col = (size_t)p.col0 + blockIdx.y;
    // the lower boundary (include/lsx_hip_boundary.h): thermalised unless the column has been given ZERO (GIVEN is refused on the host)
    const bool lower_zero = p.bnd != nullptr && boundary_kind(p.bnd, col, LSX_BND_LOWER) == 0;
    const FinalColumn f = final_column(p, col, la);
    const FinalAngles fa = final_angles(p, col);
    const double wav = p.wavelength[la], u_la = p.u_la[la];
    // this lane's cells: + (m Ns + k) nla
    const size_t plane = (size_t)Ns * p.nla;
    const size_t obase = ((size_t)blockIdx.y * p.nmu + p.mu0) * plane + q;
    double* const o_chi = p.chi + obase;
    double* const o_S = p.S + obase;
    double* const o_tau = p.tau + obase;
    double* const o_I = p.I + obase;
    double* const o_con = p.contrib + obase;

    double mu[NM], zmu[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        mu[m] = p.mu[p.mu0 + m];
        zmu[m] = 1.0 / mu[m];
    }

    // ================= down: chi, S, tau, contrib, z(tau = 1) =================
    {
        double tau[NM], c_prev[NM], zt1[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) { tau[m] = 0.0; c_prev[m] = 0.0; zt1[m] = __builtin_nan(""); }
        double zprev = 0.0;
        // the stream operands of a depth are fetched a depth ahead: their loads are in flight before the depth's stores are issued
        double f_c0 = f.bgchi[0], f_h0 = f.bgeta[0], f_sc = f.sca[0], f_J = f.Jd[0], f_E = f.Eb ? f.Eb[0] : 0.0;
        for (int k = 0; k < Ns; ++k) {
            const double zk = f.z[k];
            const double Ev = f_E;
            const double c0 = f_c0, h0 = f_h0 + f_sc * f_J;
            if (k + 1 < Ns) {
                const size_t kn = (size_t)(k + 1);
                f_c0 = f.bgchi[kn * L]; f_h0 = f.bgeta[kn * L]; f_sc = f.sca[kn * f.sstr]; f_J = f.Jd[kn * L];
                f_E = f.Eb ? f.Eb[kn * L] : 0.0;
            }
            // ---- opacity and emissivity at this depth (rh_method.py:599-632) ----
            double chi[NM], eta[NM];
#pragma unroll
            for (int m = 0; m < NM; ++m) { chi[m] = c0; eta[m] = h0; }
            for (int e = f.e0; e < f.e1; ++e) {
                const FinalEnt& t = p.ents[e];
                const double ni = f.n_col[(size_t)t.li * Ns + k], nj = f.n_col[(size_t)t.lj * Ns + k];
                if (t.is_line) {
                    const double nd = t.a * (ni - t.g * nj);          // n_i Vij - n_j Vji = nd phi, :279-280, :613
                    if (fa.raydep) {
                        const double vb = fa.vB[(size_t)t.atom * Ns + k], ad = fa.aD[(size_t)t.row * Ns + k], vl = fa.vL[k];
                        const double v = (wav - t.lambda0) * kCLight / (vb * t.lambda0);          // :234
                        const double nrm = sqrt(M_PI) * vb;
#pragma unroll
                        for (int m = 0; m < NM; ++m) {
                            const double pv = dev_voigt(ad, v + 1.0 * (mu[m] * vl / vb), vtab) / nrm;   // up-going: :231, :238-239
                            chi[m] += nd * pv;
                            eta[m] += nj * (t.Uc * pv);
                        }
                    } else {
                        // ray-independent profile: the one the formal solution uses (compact: row k; else the up-going row of ray 0)
                        const size_t x = p.phi_compact ? (size_t)k : ((size_t)Ns + k) * p.Nrays;
                        const double pv = p.phi_T[phi_elem(col, p.phi_G, (size_t)p.phi_col, (size_t)t.phi_base, x, t.phi_len, t.phi_l)];
                        const double c1 = nd * pv, h1 = nj * (t.Uc * pv);
#pragma unroll
                        for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
                    }
                } else {
                    const double pv = (f.nsr_col[(size_t)t.row * Ns + k] * Ev) * t.a;     // Vji = g_ij alpha, :284-285, :453-454
                    const double c1 = ni * t.a - nj * pv, h1 = nj * (u_la * pv);        // :286, :613-614
#pragma unroll
                    for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
                }
            }
            const double hdz = 0.5 * fabs(zprev - zk);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const double S = eta[m] / chi[m];                                   // :632
                if (k > 0) {
                    const double tp = tau[m];
                    tau[m] = tp + (c_prev[m] + chi[m]) * (hdz * zmu[m]);           // formal_solver.py:129, from the top in index order
                    if (!(zt1[m] == zt1[m]) && tau[m] >= 1.0)                       // the first depth at which tau reaches 1
                        zt1[m] = zprev + (1.0 - tp) / (tau[m] - tp) * (zk - zprev);
                }
                c_prev[m] = chi[m];
                // the argument is held in the table's range; beyond 700 the value only has to stay below exp(-700)
                const double ex = exp_tab64(fmax(-tau[m], -740.0), etab);
                const double con = (chi[m] * S) * ex / mu[m];
                if (valid) {
                    const size_t o = ((size_t)m * Ns + k) * p.nla;
                    o_chi[o] = chi[m];
                    o_S[o] = S;
                    o_tau[o] = tau[m];
                    o_con[o] = con;
                }
            }
            zprev = zk;
        }
        if (valid) {
            double* zo = p.ztau1 + ((size_t)blockIdx.y * p.nmu + p.mu0) * p.nla + q;
#pragma unroll
            for (int m = 0; m < NM; ++m) zo[(size_t)m * p.nla] = zt1[m];
        }
    }

    // ================= up: the recurrence on the lane's own chi and S; I at every depth =================
    double Iu[NM], c_k[NM], S_k[NM], c_u[NM], S_u[NM], dtau_prev[NM];
    final_state_init(Iu, c_k, S_k, c_u, S_u, dtau_prev);
    double zk1 = 0.0, zk2 = 0.0;       // heights of the two depths below the current one

    for (int k = Ns - 1; k >= 0; --k) {
        const int s = Ns - 1 - k;      // step along the up-going ray
        const double zk = f.z[k];
        double chi[NM], Sd[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const size_t o = ((size_t)m * Ns + k) * p.nla;
            chi[m] = valid ? o_chi[o] : 1.0;       // (a spare lane keeps a harmless state of its own)
            Sd[m] = valid ? o_S[o] : 0.0;
        }
        // the start value belongs to the depth below (Iu is still 0 there): I[kStart] = Istart, :117
        if (s == 1 && !lower_zero)
            thermal_start(planck(p.temperature[col * Ns + Ns - 1], wav), planck(p.temperature[col * Ns + Ns - 2], wav), fabs(zk1 - zk), zmu,
                          c_k, chi, Iu);
        if constexpr (!PAR) {
            if (s == 1 && valid) {
#pragma unroll
                for (int m = 0; m < NM; ++m) o_I[((size_t)m * Ns + k + 1) * p.nla] = Iu[m];
            }
            linear_step_ref(s, k == 0, fabs(zk1 - zk), zmu, chi, Sd, Iu, c_k, S_k, dtau_prev, etab);
            if (s >= 1 && valid) {
#pragma unroll
                for (int m = 0; m < NM; ++m) o_I[((size_t)m * Ns + k) * p.nla] = Iu[m];
            }
        } else {
            // a depth is finished when its downwind neighbour is known: from step 2 on Iu belongs to the depth below
#pragma unroll
            for (int m = 0; m < NM; ++m) parabolic_step(s, zk, zk1, zk2, zmu[m], chi[m], Sd[m], Iu[m], c_k[m], S_k[m], c_u[m], S_u[m], etab);
            if (s >= 1 && valid) {
#pragma unroll
                for (int m = 0; m < NM; ++m) o_I[((size_t)m * Ns + k + 1) * p.nla] = Iu[m];
            }
        }
        zk2 = zk1;
        zk1 = zk;
    }
    if constexpr (PAR) {
        parabolic_end(zk1, zk2, zmu, Iu, c_k, S_k, c_u, S_u, etab);
        if (valid) {
#pragma unroll
            for (int m = 0; m < NM; ++m) o_I[(size_t)m * Ns * p.nla] = Iu[m];
        }
    }
}

template <int NM>
void launch_chunk(const DepthParams& p, bool par, dim3 grid, hipStream_t st)
{
    if (par) hipLaunchKernelGGL((k_depth_rays<NM, true>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((k_depth_rays<NM, false>), grid, dim3(64), 0, st, p);
}

} // namespace

extern "C" int lsx_hip_depth_rays_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_DEPTH_WORK, "lsx_hip_depth_rays_work_cap", nbytes);
}

extern "C" int lsx_hip_depth_rays(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                  double* chi, double* S, double* tau, double* I, double* contrib, double* z_tau1,
                                  size_t nbytes_each, size_t nbytes_z)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c || !mu) return fail(LSX_EINVAL, "lsx_hip_depth_rays: null argument");
    if (!chi && !S && !tau && !I && !contrib && !z_tau1) return fail(LSX_EINVAL, "lsx_hip_depth_rays: all six outputs are NULL");
    int rc = final_check_angles("lsx_hip_depth_rays", nmu, mu);
    if (!rc) rc = final_check_range(c, "lsx_hip_depth_rays", col0, ncol);
    if (rc) return rc;
    if ((rc = final_check_window(c, "lsx_hip_depth_rays", la0, nla))) return rc;
    const size_t zper = (size_t)nmu * nla;                       // doubles of z_tau1 per column
    const size_t per = zper * c->Nspace;                         // ... of each of the five depth-resolved arrays
    if ((chi || S || tau || I || contrib) && nbytes_each != (size_t)ncol * per * 8)
        return fail(LSX_EINVAL, "lsx_hip_depth_rays: nbytes_each does not match [ncol][nmu][Nspace][nla]");
    if (z_tau1 && nbytes_z != (size_t)ncol * zper * 8) return fail(LSX_EINVAL, "lsx_hip_depth_rays: nbytes_z does not match [ncol][nmu][nla]");
    if ((rc = final_check_depths(c, "lsx_hip_depth_rays"))) return rc;
    if ((rc = final_check_columns(c, "lsx_hip_depth_rays", col0, ncol, FINAL_OTHER_ANGLE))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = final_tables(c, "lsx_hip_depth_rays"))) return rc;

    // columns per pass: the arrays of a pass stay under the cap (one column's need if that alone is more)
    GrowBuf& work = c->buf[BUF_DEPTH_WORK];
    const size_t wcol = 5 * per + zper;
    const size_t chunk = pass_columns(ncol, work.cap, kWorkCapDefault, wcol, kGridYLimit);
    if ((rc = work.reserve(c, chunk * wcol * 8))) return rc;
    if ((rc = ensure_stage(c, (size_t)nmu))) return rc;          // the angles go through the staging buffer
    double* d_mu = c->d_stage;
    HIPCHK(hipMemcpyAsync(d_mu, mu, (size_t)nmu * 8, hipMemcpyHostToDevice, c->stream));

    DepthParams p{};
    final_fill(p, c);
    final_fill_angles(p, c);
    p.nmu = nmu; p.la0 = la0; p.nla = nla; p.mu = d_mu;
    const bool par = c->solver == LSX_SOLVER_PARABOLIC;

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(col0 + b0);
        double* w = work.as<double>();
        p.chi = w; p.S = w + nb * per; p.tau = w + 2 * nb * per; p.I = w + 3 * nb * per; p.contrib = w + 4 * nb * per;
        p.ztau1 = w + 5 * nb * per;
        const dim3 grid((unsigned)((nla + 63) / 64), (unsigned)nb);
        for (int m0 = 0; m0 < nmu;) {                 // angles in register chunks of 4, 2, 1
            const int left = nmu - m0;
            p.mu0 = m0;
            if (left >= 4) { launch_chunk<4>(p, par, grid, c->stream); m0 += 4; }
            else if (left >= 2) { launch_chunk<2>(p, par, grid, c->stream); m0 += 2; }
            else { launch_chunk<1>(p, par, grid, c->stream); m0 += 1; }
        }
        HIPCHK(hipGetLastError());
        double* const dst[5] = {chi, S, tau, I, contrib};
        const double* const src[5] = {p.chi, p.S, p.tau, p.I, p.contrib};
        for (int a = 0; a < 5; ++a)
            if (dst[a]) HIPCHK(hipMemcpyAsync(dst[a] + b0 * per, src[a], nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        if (z_tau1) HIPCHK(hipMemcpyAsync(z_tau1 + b0 * zper, p.ztau1, nb * zper * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next pass
    }
    return LSX_OK;
}
