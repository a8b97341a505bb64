// lsx_rays.hip -- final-pass formal solution: the emergent intensity of a converged context at arbitrary viewing angles
// (include/lsx_hip.h, lsx_hip_emergent_rays).  Read-only on the context; gfx950 only.
//
// Reference lines restated here:
//   atmosphere.py:386-393          Atmosphere.rays(mu): the angles of a final pass
//   rh_method.py:599-638           opacity, emissivity, source function, emergent value I[0] of the up-going ray
//   rh_method.py:231-239           line profile of the up-going ray at the new angle (ray-dependent profiles)
//   formal_solver.py:46-142, 203-207   the recurrence with its end-point quirk, thermalised lower boundary
//
// Mapping: one wavefront = 64 consecutive wavelengths of one column, a lane owns one wavelength and carries a compile-time
// chunk of NM angles in registers.  Everything but the profile of a ray-dependent line is independent of the angle and is
// formed once per depth.  The background, J and the Boltzmann factor are read from the tile-major streams the context keeps
// ([col][tile][k][j < L]): the lanes of a tile read one contiguous run per depth.  Populations, nStar ratios and the kept
// broadening arrays are uniform over the lanes that share a transition (one column per wavefront).  The only LDS is the
// exponential's table and the Voigt function's (1.5 kB); the depth count is unlimited.  The arithmetic of a depth is the sweep's
// generic path (lsx_sweep.hip: same reciprocal, same w2 / w3 / planck forms), so the quadrature's own angles reproduce LSX_I to
// rounding.  A ray-dependent profile costs one evaluation of the Voigt function per (line wavelength, depth, angle): that, not the
// memory traffic, is what the kernel's time is made of on contexts with a line-of-sight velocity.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_ctx.h"
#include "lsx_voigt.h"

using namespace lsxd;

namespace {

constexpr double kCLight = 2.99792458E+08;
constexpr double kHPlanck = 6.6260755E-34;
constexpr double kKBoltzmann = 1.380658E-23;
constexpr double kNM_TO_M = 1.0E-09;
constexpr double kHC = kHPlanck * kCLight;

// one transition as one wavelength sees it; the entries of a wavelength are in table order (rays_tables)
struct RayEnt {
    int32_t is_line;
    int32_t li, lj;             // rows of n
    int32_t row;                // lines: row of aDamp; continua: row of nsr
    int32_t atom;               // lines: row of vBroad
    int32_t phi_base, phi_len, phi_l;   // lines: the (tile, line) block of the profile store and the wavelength's place in it
    double a;                   // lines: (hc/4pi) Bij; continua: alpha at this wavelength
    double g;                   // lines: Bji / Bij
    double Uc;                  // lines: (Aji / Bji) g (hc/4pi) Bij
    double lambda0;             // lines: rest wavelength [nm]
};

struct RaysParams {
    int32_t Ns, Nspect, NLtot, Natoms, NlinesA, Ncont, L, Nrays;
    int32_t col0, nmu, mu0;     // first column of the launch; angles of the call; first angle of this launch's chunk
    int32_t phi_compact, sca_per_lambda, phi_G;
    int64_t til_col, phi_col, sca_col;
    const double *wavelength, *u_la, *exp2_tab, *voigt_W, *mu;
    const int32_t* la_ptr;      // [Nspect + 1] into ents
    const RayEnt* ents;
    const int32_t* la_tile;     // [Nspect][2]: tile, place in the tile
    const double *height, *temperature, *n, *nsr, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    const double *aDamp, *vBroad, *vlos;
    const uint8_t* prof_kind;   // per column: 2 = profiles built by the library with a line-of-sight velocity (ray dependent)
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store), or null
    double* out;                // [launch column][Nspect][nmu]
};

// utils.py:17-22 (as lsx_sweep.hip has it)
__device__ __forceinline__ double planck(double temp, double wav)
{
    const double hc_Tkla = kHC / (kKBoltzmann * kNM_TO_M * wav) / temp;
    const double x = kNM_TO_M * wav;
    const double twohnu3_c2 = (2.0 * kHC) / (x * x * x);
    return twohnu3_c2 / (exp(hc_Tkla) - 1.0);
}

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
    const int tile = p.la_tile[2 * la], j = p.la_tile[2 * la + 1];
    const size_t toff = (size_t)tile * Ns * L + j;         // + k L: this wavelength in a tile-major stream
    const double* __restrict__ bgchi = p.bgchi_T + col * p.til_col + toff;
    const double* __restrict__ bgeta = p.bgeta_T + col * p.til_col + toff;
    const double* __restrict__ Jd = p.J_T + col * p.til_col + toff;
    const double* __restrict__ Eb = p.E_T ? p.E_T + col * p.til_col + toff : nullptr;
    const double* __restrict__ sca = p.sca_per_lambda ? p.sca + col * p.sca_col + toff : p.sca + col * p.sca_col;
    const int sstr = p.sca_per_lambda ? L : 1;
    const double* __restrict__ z = p.height + col * Ns;
    const double* __restrict__ n_col = p.n + col * (size_t)p.NLtot * Ns;
    const double* __restrict__ nsr_col = p.nsr ? p.nsr + col * (size_t)p.Ncont * Ns : nullptr;
    const int e0 = p.la_ptr[la], e1 = p.la_ptr[la + 1];
    const bool raydep = !p.phi_compact && p.prof_kind && p.prof_kind[col] == 2;
    const double* __restrict__ aD = raydep ? p.aDamp + col * (size_t)p.NlinesA * Ns : nullptr;
    const double* __restrict__ vB = raydep ? p.vBroad + col * (size_t)p.Natoms * Ns : nullptr;
    const double* __restrict__ vL = raydep ? p.vlos + col * Ns : nullptr;
    const double wav = p.wavelength[la], u_la = p.u_la[la];

    double mu[NM], zmu[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        mu[m] = p.mu[p.mu0 + m];
        zmu[m] = 1.0 / mu[m];
    }
    // state of the recurrence per angle (lsx_sweep.hip, generic path): linear rule chi_prev, S_prev, dtau_prev; parabolic rule the
    // window (upwind, local, downwind) of the depth being finished
    double Iu[NM], c_k[NM], S_k[NM], c_u[NM], S_u[NM], dtau_prev[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) { Iu[m] = 0.0; c_k[m] = 1.0; S_k[m] = 0.0; c_u[m] = 1.0; S_u[m] = 0.0; dtau_prev[m] = 1.0; }
    double zk1 = 0.0, zk2 = 0.0;       // heights of the two depths below the current one

    for (int k = Ns - 1; k >= 0; --k) {
        const int s = Ns - 1 - k;      // step along the up-going ray
        const double zk = z[k];
        // ---- opacity and emissivity at this depth (rh_method.py:599-632) ----
        const double Ev = Eb ? Eb[(size_t)k * L] : 0.0;
        double chi[NM], eta[NM];
        {
            const double c0 = bgchi[(size_t)k * L];
            const double h0 = bgeta[(size_t)k * L] + sca[(size_t)k * sstr] * Jd[(size_t)k * L];
#pragma unroll
            for (int m = 0; m < NM; ++m) { chi[m] = c0; eta[m] = h0; }
        }
        for (int e = e0; e < e1; ++e) {
            const RayEnt& t = p.ents[e];
            const double ni = n_col[(size_t)t.li * Ns + k], nj = n_col[(size_t)t.lj * Ns + k];
            if (t.is_line) {
                const double nd = t.a * (ni - t.g * nj);          // n_i Vij - n_j Vji = nd phi, :279-280, :613
                if (raydep) {
                    const double vb = vB[(size_t)t.atom * Ns + k], ad = aD[(size_t)t.row * Ns + k], vl = vL[k];
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
                const double pv = (nsr_col[(size_t)t.row * Ns + k] * Ev) * t.a;     // Vji = g_ij alpha, :284-285, :453-454
                const double c1 = ni * t.a - nj * pv, h1 = nj * (u_la * pv);        // :286, :613-614
#pragma unroll
                for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
            }
        }
        // ---- the up-going ray's recurrence at this depth ----
        if constexpr (!PAR) {
            // formal_solver.py:107-139 as the sweep's generic path has it: the two divisions of a step share one reciprocal
            const double hdz = 0.5 * fabs(zk1 - zk);
            double B0 = 0.0, B1 = 0.0;
            if (s == 1) { B0 = planck(p.temperature[col * Ns + Ns - 2], wav); B1 = planck(p.temperature[col * Ns + Ns - 1], wav); }
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                if (s == 0) {
                    const double rchi = rcp(chi[m]);
                    S_k[m] = eta[m] * rchi;
                    c_k[m] = chi[m];
                    continue;
                }
                if (s == 1) {                                      // thermalised lower boundary, formal_solver.py:203-207
                    const double dtau_uw = zmu[m] * (c_k[m] + chi[m]) * 0.5 * fabs(zk1 - zk);
                    Iu[m] = lower_zero ? 0.0 : B1 - (B0 - B1) / dtau_uw;
                }
                const double dtau = (c_k[m] + chi[m]) * (hdz * zmu[m]);
                const double rcd = rcp(chi[m] * dtau);
                const double rchi = rcd * dtau, rdt = rcd * chi[m];
                const double S = eta[m] * rchi;                    // :632
                const double dS = (S_k[m] - S) * rdt;
                // formal_solver.py:138-139: the end point re-uses the previous interval's w and S[kEnd - dk] with the fresh dS
                const bool last = k == 0;
                double w0, w1;
                w2(last ? dtau_prev[m] : dtau, w0, w1, etab);
                const double Sx = last ? S_k[m] : S;
                Iu[m] = Iu[m] * (1.0 - w0) + w0 * Sx + w1 * dS;
                dtau_prev[m] = dtau;
                c_k[m] = chi[m];
                S_k[m] = S;
            }
        } else {
            // monotonic parabolic rule (include/lsx.h, N4) as the sweep's generic instance: a depth is finished when its downwind
            // neighbour is known.  Window after the shift: u = k + 2, k = k + 1, d = this depth
            double B0 = 0.0, B1 = 0.0;
            if (s == 1) { B0 = planck(p.temperature[col * Ns + Ns - 2], wav); B1 = planck(p.temperature[col * Ns + Ns - 1], wav); }
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const double c_d = chi[m], S_d = eta[m] / chi[m];
                if (s == 1) {
                    const double dtau_uw = zmu[m] * (c_k[m] + c_d) * 0.5 * fabs(zk1 - zk);
                    Iu[m] = lower_zero ? 0.0 : B1 - (B0 - B1) / dtau_uw;
                }
                if (s >= 2) {
                    const double dtau_u = (c_u[m] + c_k[m]) * (0.5 * fabs(zk2 - zk1)) * zmu[m];
                    const double dtau_d = (c_k[m] + c_d) * (0.5 * fabs(zk1 - zk)) * zmu[m];
                    Iu[m] = parabolic_point(Iu[m], S_u[m], S_k[m], S_d, dtau_u, dtau_d, true, etab).I;
                }
                c_u[m] = c_k[m]; S_u[m] = S_k[m];
                c_k[m] = c_d; S_k[m] = S_d;
            }
        }
        zk2 = zk1;
        zk1 = zk;
    }
    if constexpr (PAR) {            // the end point: no downwind neighbour (the linear rule with its own interval's weights)
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const double dtau_u = (c_u[m] + c_k[m]) * (0.5 * fabs(zk2 - zk1)) * zmu[m];
            Iu[m] = parabolic_point(Iu[m], S_u[m], S_k[m], 0.0, dtau_u, 1.0, false, etab).I;
        }
    }
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

// column-independent tables of the entry, made on first use: per wavelength its active transitions in table order and its
// place in the tile-major streams
int rays_tables(lsx_ctx* c)
{
    if (c->d_rays_ptr) return LSX_OK;
    const int Nspect = c->Nspect;
    std::vector<int32_t> la_tile(2 * (size_t)Nspect, 0), ptr(Nspect + 1, 0);
    std::vector<int> tile_of(Nspect, -1);
    for (size_t t = 0; t < c->tiles.size(); ++t)
        for (int q = 0; q < c->tiles[t].nla; ++q) {
            const int la = c->tiles[t].la0 + q;
            tile_of[la] = (int)t;
            la_tile[2 * la] = (int32_t)t;
            la_tile[2 * la + 1] = q;
        }
    std::vector<RayEnt> ents;
    for (int la = 0; la < Nspect; ++la) {
        if (tile_of[la] < 0) return fail(LSX_EDEVICE, "lsx_hip_emergent_rays: wavelength %d belongs to no tile", la);
        const DevTile& tl = c->tiles[tile_of[la]];
        for (int t = 0; t < c->Ntrans; ++t) {
            if (!c->active[(size_t)t * Nspect + la]) continue;
            const DevTrans& h = c->htrans[t];
            RayEnt e{};
            e.is_line = h.is_line; e.li = h.li; e.lj = h.lj; e.row = c->trans_row[t]; e.atom = h.atom;
            if (h.is_line) {
                const DevSlot* sl = nullptr;
                for (int u = 0; u < tl.nL; ++u)
                    if (c->slots[tl.slot0 + u].trans == t) sl = &c->slots[tl.slot0 + u];
                if (!sl || !(sl->flags & SLOT_LINE) || la < sl->first || la >= sl->first + sl->len)
                    return fail(LSX_EDEVICE, "lsx_hip_emergent_rays: line %d has no profile block at wavelength %d", t, la);
                e.phi_base = sl->base; e.phi_len = sl->len; e.phi_l = la - sl->first;
                e.a = h.cB; e.g = h.gij; e.Uc = h.AB * (h.gij * h.cB); e.lambda0 = h.lambda0;
            } else {
                e.a = c->alpha[h.wl_off + (la - h.Nblue)];
            }
            ents.push_back(e);
        }
        ptr[la + 1] = (int32_t)ents.size();
    }
    if (ents.empty()) ents.push_back(RayEnt{});
    std::vector<char> bytes((const char*)ents.data(), (const char*)ents.data() + ents.size() * sizeof(RayEnt));
    int rc = upload(&c->d_rays_tile, la_tile, c->stream);
    if (!rc) rc = upload(&c->d_rays_ent, bytes, c->stream);
    if (!rc) rc = upload(&c->d_rays_ptr, ptr, c->stream);        // (last: its presence marks the set complete)
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));                      // the host vectors go out of scope
    return LSX_OK;
}

} // namespace

extern "C" int lsx_hip_emergent_rays(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, double* dst, size_t nbytes)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c || !mu || !dst) return fail(LSX_EINVAL, "lsx_hip_emergent_rays: null argument");
    if (nmu < 1) return fail(LSX_EINVAL, "lsx_hip_emergent_rays: nmu = %d, need at least one angle", (int)nmu);
    for (int m = 0; m < nmu; ++m)
        if (!(mu[m] > 0.0 && mu[m] <= 1.0)) return fail(LSX_EINVAL, "lsx_hip_emergent_rays: mu[%d] = %g is outside (0, 1]", m, mu[m]);
    if (col0 < 0 || ncol < 1 || (int64_t)col0 + ncol > c->ncol)
        return fail(LSX_EINVAL, "lsx_hip_emergent_rays: columns [%d, %d) are outside the context's %d", (int)col0, (int)col0 + (int)ncol, c->ncol);
    const size_t per = (size_t)c->Nspect * nmu;
    if (nbytes != (size_t)ncol * per * 8) return fail(LSX_EINVAL, "lsx_hip_emergent_rays: nbytes does not match [ncol][Nspect][nmu]");
    if (c->Nspace < 3) return fail(LSX_EUNSUPPORTED, "lsx_hip_emergent_rays: needs Nspace >= 3");
    for (int q = col0; q < col0 + ncol; ++q) {
        if (!c->bnd_kind.empty() && c->bnd_kind[2 * (size_t)q] == LSX_BOUNDARY_GIVEN)
            return fail(LSX_EUNSUPPORTED, "lsx_hip_emergent_rays: column %d has a GIVEN lower boundary (lsx_hip_set_boundary): its intensity was handed "
                                          "over on the context's own rays and wavelengths and is not known at another angle", q);
        if (!c->phi_set[q])
            return fail(LSX_EINVAL, "lsx_hip_emergent_rays: column %d has no line profiles (lsx_set_columns with phi == NULL must be "
                                    "followed by lsx_set_line_profiles)", q);
        if (c->Nlines && !c->phi_compact && (c->prof_kind.empty() || !c->prof_kind[q]))
            return fail(LSX_EUNSUPPORTED, "lsx_hip_emergent_rays: the ray-dependent line profiles of column %d were handed over as arrays "
                                          "(lsx_set_columns): the library cannot know them at another angle.  Build them with "
                                          "lsx_set_line_profiles or lsx_set_atmosphere", q);
    }
    HIPCHK(hipSetDevice(c->device));
    int rc = rays_tables(c);
    if (rc) return rc;

    // the result of a chunk of columns and the angles go through the staging buffer: [nmu angles | chunk][Nspect][nmu]
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(ncol, ((size_t)32 << 20) / per));
    const size_t head = ((size_t)nmu + 1) & ~(size_t)1;
    if ((rc = ensure_stage(c, head + chunk * per))) return rc;
    double* d_mu = c->d_stage;
    double* d_out = c->d_stage + head;
    HIPCHK(hipMemcpyAsync(d_mu, mu, (size_t)nmu * 8, hipMemcpyHostToDevice, c->stream));

    RaysParams p{};
    p.Ns = c->Nspace; p.Nspect = c->Nspect; p.NLtot = c->NLtot; p.Natoms = c->Natoms; p.NlinesA = std::max(1, c->Nlines);
    p.Ncont = c->Ncont; p.L = c->L; p.Nrays = c->Nrays; p.nmu = nmu;
    p.phi_compact = c->phi_compact; p.sca_per_lambda = c->sca_per_lambda; p.phi_G = c->phi_group;
    p.til_col = (int64_t)c->til_col; p.phi_col = (int64_t)c->phi_col; p.sca_col = (int64_t)c->sca_col;
    p.wavelength = c->d_wavelength; p.u_la = c->d_u_la; p.exp2_tab = c->d_exp2_tab; p.voigt_W = c->d_voigt_w; p.mu = d_mu;
    p.la_ptr = c->d_rays_ptr; p.ents = reinterpret_cast<const RayEnt*>(c->d_rays_ent); p.la_tile = c->d_rays_tile;
    p.height = c->d_height; p.temperature = c->d_temperature; p.n = c->d_n; p.nsr = c->d_nsr;
    p.bnd = c->d_bnd;
    p.bgchi_T = c->d_bgchi; p.bgeta_T = c->d_bgeta; p.J_T = c->d_J[c->jcur];      // what lsx_get(LSX_J) returns at this moment
    p.E_T = c->d_E; p.sca = c->d_sca; p.phi_T = c->d_phi;
    p.aDamp = c->d_aDamp; p.vBroad = c->d_vBroad; p.vlos = c->d_vlos; p.prof_kind = c->d_prof_kind;
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
