// lsx_rays.hip -- final-pass formal solution: the emergent intensity of a converged context at arbitrary viewing angles
// (include/lsx_hip.h, lsx_hip_emergent_rays).  Read-only on the context; gfx950 only.
//
// Reference lines restated here (the rest: lsx_final_dev.h, whose column set-up, start value and recurrence steps this walk uses):
//   rh_method.py:599-632           opacity, emissivity, source function
//   rh_method.py:231-239           line profile of the up-going ray at the new angle (ray-dependent profiles)
//   atmosphere.py:386-393          Atmosphere.rays(mu): the angles of a final pass
//   rh_method.py:638               emergent value I[0] of the up-going ray
//
// Mapping: one wavefront = 64 consecutive wavelengths of one column, a lane owns one wavelength and carries a compile-time
// chunk of NM angles in registers.  The lanes of a tile read one contiguous run of the tile-major streams per depth; populations,
// nStar ratios and the kept broadening arrays are uniform over the lanes that share a transition (one column per wavefront).  The
// only LDS is the exponential's table and the Voigt function's (1.5 kB); the depth count is unlimited.  The arithmetic of a depth is
// the sweep's generic path (lsx_sweep.hip: same reciprocal, same w2 / w3 / planck forms), so the quadrature's own angles reproduce
// LSX_I to rounding.  A ray-dependent profile costs one evaluation of the Voigt function per (line wavelength, depth, angle): that,
// not the memory traffic, is what the kernel's time is made of on contexts with a line-of-sight velocity.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"
#include "lsx_voigt.h"

using namespace lsxd;

namespace {

struct RaysParams {
    int32_t Ns, Nspect, NLtot, Natoms, NlinesA, Ncont, L, Nrays;
    int32_t col0, nmu, mu0;     // first column of the launch; angles of the call; first angle of this launch's chunk
    int32_t phi_compact, sca_per_lambda, phi_G;
    int64_t til_col, phi_col, sca_col;
    const double *wavelength, *u_la, *exp2_tab, *voigt_W, *mu;
    const int32_t* la_ptr;      // [Nspect + 1] into ents
    const FinalEnt* ents;
    const int32_t* la_tile;     // [Nspect][2]: tile, place in the tile
    const double *height, *temperature, *n, *nsr, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    const double *aDamp, *vBroad, *vlos;
    const uint8_t* prof_kind;   // per column: 2 = profiles built by the library with a line-of-sight velocity (ray dependent)
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store), or null
    double* out;                // [launch column][Nspect][nmu]
};

template <int NM, bool PAR>
__global__ void __launch_bounds__(64) k_emergent_rays(const RaysParams p)
{
    __shared__ double etab_s[LSX_EXP_TAB + 64];      // the exponential's table and the Voigt function's (lsx_voigt.h: 56 doubles)
    for (int e = threadIdx.x; e < LSX_EXP_TAB; e += 64) etab_s[e] = p.exp2_tab[e];
    if (p.voigt_W && threadIdx.x < 56) etab_s[LSX_EXP_TAB + threadIdx.x] = p.voigt_W[threadIdx.x];
    __syncthreads();
    const lds_f64* etab = (const lds_f64*)etab_s;
    const lds_f64* vtab = etab + LSX_EXP_TAB;

    const int Ns = p.Ns, L = p.L;
    const int la_raw = blockIdx.x * 64 + threadIdx.x;
    const bool valid = la_raw < p.Nspect;
    const int la = valid ? la_raw : p.Nspect - 1;          // every lane walks a wavelength (w2 / w3 are wave-wide); spare ones store nothing
    const size_t col = (size_t)p.col0 + blockIdx.y;
    // the lower boundary (include/lsx_hip_boundary.h): thermalised unless the column has been given ZERO (GIVEN is refused on the host)
    const bool lower_zero = p.bnd != nullptr && boundary_kind(p.bnd, col, LSX_BND_LOWER) == 0;
    const FinalColumn f = final_column(p, col, la);
    const FinalAngles fa = final_angles(p, col);
    const double wav = p.wavelength[la], u_la = p.u_la[la];

    double mu[NM], zmu[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        mu[m] = p.mu[p.mu0 + m];
        zmu[m] = 1.0 / mu[m];
    }
    double Iu[NM], c_k[NM], S_k[NM], c_u[NM], S_u[NM], dtau_prev[NM];
    final_state_init(Iu, c_k, S_k, c_u, S_u, dtau_prev);
    double zk1 = 0.0, zk2 = 0.0;       // heights of the two depths below the current one

    for (int k = Ns - 1; k >= 0; --k) {
        const int s = Ns - 1 - k;      // step along the up-going ray
        const double zk = f.z[k];
        const double Ev = f.Eb ? f.Eb[(size_t)k * L] : 0.0;
        const double c0 = f.bgchi[(size_t)k * L];
        const double h0 = f.bgeta[(size_t)k * L] + f.sca[(size_t)k * f.sstr] * f.Jd[(size_t)k * L];
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
        // ---- the up-going ray's recurrence at this depth; its start value belongs to the depth below (Iu is still 0 there) ----
        if (s == 1 && !lower_zero)
            thermal_start(planck(p.temperature[col * Ns + Ns - 1], wav), planck(p.temperature[col * Ns + Ns - 2], wav), fabs(zk1 - zk), zmu,
                          c_k, chi, Iu);
        if constexpr (!PAR) {
            linear_step(s, k == 0, 0.5 * fabs(zk1 - zk), zmu, chi, eta, Iu, c_k, S_k, dtau_prev, etab);
        } else {
#pragma unroll
            for (int m = 0; m < NM; ++m)
                parabolic_step(s, zk, zk1, zk2, zmu[m], chi[m], eta[m] / chi[m], Iu[m], c_k[m], S_k[m], c_u[m], S_u[m], etab);
        }
        zk2 = zk1;
        zk1 = zk;
    }
    if constexpr (PAR) parabolic_end(zk1, zk2, zmu, Iu, c_k, S_k, c_u, S_u, etab);
    if (valid) {
        double* o = p.out + ((size_t)blockIdx.y * p.Nspect + la) * p.nmu + p.mu0;    // emergent value I[0], rh_method.py:638
#pragma unroll
        for (int m = 0; m < NM; ++m) o[m] = Iu[m];
    }
}

template <int NM>
void launch_chunk(const RaysParams& p, bool par, dim3 grid, hipStream_t st)
{
    if constexpr (NM <= 4) {
        if (par) { hipLaunchKernelGGL((k_emergent_rays<NM, true>), grid, dim3(64), 0, st, p); return; }
    }
    hipLaunchKernelGGL((k_emergent_rays<NM, false>), grid, dim3(64), 0, st, p);
}

} // namespace

extern "C" int lsx_hip_emergent_rays(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, double* dst, size_t nbytes)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c || !mu || !dst) return fail(LSX_EINVAL, "lsx_hip_emergent_rays: null argument");
    int rc = final_check_angles("lsx_hip_emergent_rays", nmu, mu);
    if (!rc) rc = final_check_range(c, "lsx_hip_emergent_rays", col0, ncol);
    if (rc) return rc;
    const size_t per = (size_t)c->Nspect * nmu;
    if (nbytes != (size_t)ncol * per * 8) return fail(LSX_EINVAL, "lsx_hip_emergent_rays: nbytes does not match [ncol][Nspect][nmu]");
    if ((rc = final_check_depths(c, "lsx_hip_emergent_rays"))) return rc;
    if ((rc = final_check_columns(c, "lsx_hip_emergent_rays", col0, ncol, FINAL_OTHER_ANGLE))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = final_tables(c, "lsx_hip_emergent_rays"))) return rc;

    // the result of a chunk of columns and the angles go through the staging buffer: [nmu angles | chunk][Nspect][nmu]
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(ncol, ((size_t)32 << 20) / per));
    const size_t head = ((size_t)nmu + 1) & ~(size_t)1;
    if ((rc = ensure_stage(c, head + chunk * per))) return rc;
    double* d_mu = c->d_stage;
    double* d_out = c->d_stage + head;
    HIPCHK(hipMemcpyAsync(d_mu, mu, (size_t)nmu * 8, hipMemcpyHostToDevice, c->stream));

    RaysParams p{};
    final_fill(p, c);
    final_fill_angles(p, c);
    p.nmu = nmu; p.mu = d_mu;
    p.out = d_out;
    const bool par = c->solver == LSX_SOLVER_PARABOLIC;

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(col0 + b0);
        const dim3 grid((unsigned)((c->Nspect + 63) / 64), (unsigned)nb);
        for (int m0 = 0; m0 < nmu;) {                 // angles in register chunks of 8, 4, 2, 1 (the parabolic rule's window: at most 4)
            const int left = nmu - m0;
            p.mu0 = m0;
            if (left >= 8 && !par) { launch_chunk<8>(p, par, grid, c->stream); m0 += 8; }
            else if (left >= 4) { launch_chunk<4>(p, par, grid, c->stream); m0 += 4; }
            else if (left >= 2) { launch_chunk<2>(p, par, grid, c->stream); m0 += 2; }
            else { launch_chunk<1>(p, par, grid, c->stream); m0 += 1; }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dst + b0 * per, d_out, nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the staging buffer is re-used by the next chunk
    }
    return LSX_OK;
}
