// lsx_spectrum.hip -- final-pass formal solution at arbitrary WAVELENGTHS: the emergent intensity of a converged context at wavelengths
// that need not be points of the grid the populations were iterated on, at arbitrary viewing angles
// (include/lsx_hip_spectrum.h, lsx_hip_spectrum).  Read-only on the context; gfx950 only.
//
// Reference lines restated here:
//   atomic_set.py:377-383, 401-453 compute_wavelength_grid(extraWavelengths): which transitions a merged wavelength belongs to
//   rh_method.py:599-638           opacity, emissivity, source function, emergent value I[0] of the up-going ray
//   rh_method.py:231-239           line profile of the up-going ray at a wavelength and an angle
//   rh_method.py:281-287, 453      continua: Vij = alpha, gij = (nStar_i / nStar_j) exp(-hc / k lambda T), Uji = (2hc / lambda^3) Vji
// (the recurrence, its start value, the constants and planck: lsx_final_dev.h)
//
// Mapping (that of k_emergent_rays, lsx_rays.hip): one wavefront = 64 consecutive wavelengths of the CALL of one column, a lane owns
// one wavelength and carries a compile-time chunk of NM angles in registers.  What a wavelength sees does not change with depth --
// its active transitions, the cross-sections alpha' of its continua, the two places of the context's grid that bracket it -- so the
// host builds it once per call and the wavefront stages it in LDS before the depth loop, entry-major ([entry][lane]: a wavefront's
// read of an entry is one conflict-free row), next to the column-independent constants of every transition.  The depth loop reads no
// table from global memory: per depth a lane fetches J (and, in interpolation mode, the background) at its two bracketing places
// of the context's tile-major streams, the populations and broadening arrays of its transitions (uniform over the lanes that share a
// transition), and -- with a background of the caller's -- one contiguous run per stream of the pass's transposed copy
// ([column][k][wavelength], k_spectrum_transpose).  Line profiles are evaluated with the library's Voigt function at every (line
// wavelength, depth, angle), once per depth where the column has no line-of-sight velocity.  The Boltzmann factor and the Planck
// function are formed in the lane at the new wavelength.  The linear rule runs in the reference's own order of operations
// (linear_step_ref), as in lsx_depth.hip; the parabolic rule is the sweep's generic instance.
// One writer per value, fixed order of every sum: a result does not depend on the column's place, the column range, the cut into
// passes, the other wavelengths or the other angles of the call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"
#include "lsx_voigt.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)256 << 20;      // bytes (include/lsx_hip_spectrum.h)
constexpr size_t kLdsLimit = (size_t)64 << 10;             // a workgroup's LDS without opting in to more
constexpr int kTrD = 4, kTrI = 4;                          // doubles / integers of a transition's constants

typedef __attribute__((address_space(3))) int32_t lds_i32;

struct SpecParams {
    int32_t Ns, NLtot, Natoms, NlinesA, Ncont, Ntrans, L;
    int32_t col0, nmu, mu0, nla;        // first column of the launch; angles of the call; first angle of this launch's chunk; wavelengths
    int32_t Emax;                       // entries of the call's busiest wavelength: the stride of a block's staged tables
    int32_t sca_per_lambda, explicit_bg;
    int64_t til_col, sca_col;
    // per call, column independent (spec_tables)
    const double *wav, *ula, *t;        // [nla]: wavelength [nm], 2hc / lambda^3, weight of the upper bracketing place
    const int32_t *off0, *off1;         // [nla]: the two bracketing places in a tile-major stream (+ k L)
    const int32_t* blk_ne;              // [blocks]: entries of the block's busiest lane
    const int32_t* ent_tid;             // [blocks][Emax][64]: transition of the lane's e-th entry, -1 none
    const double* ent_alpha;            // [blocks][Emax][64]: continua: alpha at the lane's wavelength
    const double* tr_d;                 // [Ntrans][4]: lines (hc/4pi) Bij, Bji / Bij, (Aji / Bji) g (hc/4pi) Bij, lambda0
    const int32_t* tr_i;                // [Ntrans][4]: rows of n (i, j); lines: row of aDamp, continua: row of nsr; lines: row of vBroad, continua -1
    const double *exp2_tab, *voigt_W, *mu;
    // the context's
    const double *height, *temperature, *n, *nsr, *bgchi_T, *bgeta_T, *J_T, *sca;
    const double *aDamp, *vBroad, *vlos;
    const uint8_t* prof_kind;
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store), or null
    // the pass's: the caller's background, wavelength fastest ([launch column][k][nla]); the result [launch column][nla][nmu]
    const double *xchi, *xeta, *xsca;
    double* out;
};

// (1 - t) a + t b as two products and a sum, never contracted: the bits numpy gives, exact at t = 0 and t = 1
__device__ __forceinline__ double lerp2(double a, double b, double t)
{
#pragma clang fp contract(off)
    const double x = (1.0 - t) * a;
    const double y = t * b;
    return x + y;
}

template <int NM, bool PAR>
__global__ void __launch_bounds__(64) k_spectrum(const SpecParams p)
{
    __shared__ double etab_s[LSX_EXP_TAB + 64];      // the exponential's table and the Voigt function's (lsx_voigt.h: 56 doubles)
    extern __shared__ double dyn_s[];                // [Emax][64] alpha | [Ntrans][4] constants | [Emax][64] transition | [Ntrans][4] rows
    const int lane = threadIdx.x;
    for (int e = lane; e < LSX_EXP_TAB; e += 64) etab_s[e] = p.exp2_tab[e];
    if (p.voigt_W && lane < 56) etab_s[LSX_EXP_TAB + lane] = p.voigt_W[lane];
    const int nE = p.blk_ne[blockIdx.x];             // wave-uniform
    {
        double* al = dyn_s;
        double* trd = al + (size_t)p.Emax * 64;
        int32_t* tid = reinterpret_cast<int32_t*>(trd + (size_t)p.Ntrans * kTrD);
        int32_t* tri = tid + (size_t)p.Emax * 64;
        const size_t b = (size_t)blockIdx.x * p.Emax * 64;
        for (int e = 0; e < nE; ++e) {
            al[e * 64 + lane] = p.ent_alpha[b + e * 64 + lane];
            tid[e * 64 + lane] = p.ent_tid[b + e * 64 + lane];
        }
        for (int i = lane; i < p.Ntrans * kTrD; i += 64) { trd[i] = p.tr_d[i]; tri[i] = p.tr_i[i]; }
    }
    __syncthreads();
    const lds_f64* etab = (const lds_f64*)etab_s;
    const lds_f64* vtab = etab + LSX_EXP_TAB;
    const lds_f64* al_s = (const lds_f64*)dyn_s;
    const lds_f64* trd_s = al_s + (size_t)p.Emax * 64;
    const lds_i32* tid_s = (const lds_i32*)(trd_s + (size_t)p.Ntrans * kTrD);
    const lds_i32* tri_s = tid_s + (size_t)p.Emax * 64;

    const int Ns = p.Ns, L = p.L;
    const int q_raw = blockIdx.x * 64 + lane;              // place in the call's wavelengths
    const bool valid = q_raw < p.nla;
    const int q = valid ? q_raw : p.nla - 1;               // every lane walks a wavelength (w2 / w3 are wave-wide); spare ones store nothing
    const size_t col = (size_t)p.col0 + blockIdx.y;
    // the lower boundary (include/lsx_hip_boundary.h): thermalised unless the column has been given ZERO (GIVEN is refused on the host)
    const bool lower_zero = p.bnd != nullptr && boundary_kind(p.bnd, col, LSX_BND_LOWER) == 0;
    const size_t o0 = (size_t)p.off0[q], o1 = (size_t)p.off1[q];
    const double tq = p.t[q];
    const double* __restrict__ bgchi = p.bgchi_T + col * p.til_col;
    const double* __restrict__ bgeta = p.bgeta_T + col * p.til_col;
    const double* __restrict__ Jd = p.J_T + col * p.til_col;
    const double* __restrict__ sca = p.sca + col * p.sca_col;
    const size_t xb = (size_t)blockIdx.y * Ns * p.nla + q; // + k nla: this wavelength in the pass's transposed background
    const double* __restrict__ z = p.height + col * Ns;
    const double* __restrict__ T = p.temperature + col * Ns;
    const double* __restrict__ n_col = p.n + col * (size_t)p.NLtot * Ns;
    const double* __restrict__ nsr_col = p.nsr ? p.nsr + col * (size_t)p.Ncont * Ns : nullptr;
    const bool raydep = p.prof_kind && p.prof_kind[col] == 2;          // wave-uniform: the column has a line-of-sight velocity
    const double* __restrict__ aD = p.aDamp ? p.aDamp + col * (size_t)p.NlinesA * Ns : nullptr;
    const double* __restrict__ vB = p.vBroad ? p.vBroad + col * (size_t)p.Natoms * Ns : nullptr;
    const double* __restrict__ vL = p.vlos ? p.vlos + col * Ns : nullptr;
    const double wav = p.wav[q], u_la = p.ula[q];
    const double bc = boltzmann_lane_constant(wav);

    double mu[NM], zmu[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        mu[m] = p.mu[p.mu0 + m];
        zmu[m] = 1.0 / mu[m];
    }
    double Iu[NM], c_k[NM], S_k[NM], c_u[NM], S_u[NM], dtau_prev[NM];
    final_state_init(Iu, c_k, S_k, c_u, S_u, dtau_prev);
    double zk1 = 0.0, zk2 = 0.0;       // heights of the two depths below the current one
    const double B0 = planck(T[Ns - 2], wav), B1 = planck(T[Ns - 1], wav);

    for (int k = Ns - 1; k >= 0; --k) {
        const int s = Ns - 1 - k;      // step along the up-going ray
        const double zk = z[k];
        const size_t kL = (size_t)k * L;
        // ---- J, background and scattering coefficient at this wavelength ----
        const double Jv = lerp2(Jd[o0 + kL], Jd[o1 + kL], tq);
        double c0, h0, sc;
        if (p.explicit_bg) {
            const size_t x = xb + (size_t)k * p.nla;
            c0 = p.xchi[x];
            h0 = p.xeta[x];
            sc = p.sca_per_lambda ? p.xsca[x] : sca[k];
        } else {
            c0 = lerp2(bgchi[o0 + kL], bgchi[o1 + kL], tq);
            h0 = lerp2(bgeta[o0 + kL], bgeta[o1 + kL], tq);
            sc = p.sca_per_lambda ? lerp2(sca[o0 + kL], sca[o1 + kL], tq) : sca[k];
        }
        h0 += sc * Jv;
        // ---- opacity and emissivity at this depth (rh_method.py:599-632) ----
        const double Ev = nsr_col ? boltzmann_factor(bc, 1.0 / T[k], etab) : 0.0;       // exp(-hc / k lambda T), :453
        double chi[NM], eta[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) { chi[m] = c0; eta[m] = h0; }
        for (int e = 0; e < nE; ++e) {
            const int tr = tid_s[e * 64 + lane];
            if (tr < 0) continue;
            const int li = tri_s[tr * kTrI], lj = tri_s[tr * kTrI + 1], row = tri_s[tr * kTrI + 2], atom = tri_s[tr * kTrI + 3];
            const double ni = n_col[(size_t)li * Ns + k], nj = n_col[(size_t)lj * Ns + k];
            if (atom >= 0) {
                const double cB = trd_s[tr * kTrD], g = trd_s[tr * kTrD + 1], Uc = trd_s[tr * kTrD + 2], lam0 = trd_s[tr * kTrD + 3];
                const double nd = cB * (ni - g * nj);             // n_i Vij - n_j Vji = nd phi, :279-280, :613
                const double vb = vB[(size_t)atom * Ns + k], ad = aD[(size_t)row * Ns + k];
                const double v = (wav - lam0) * kCLight / (vb * lam0);                    // :234
                const double nrm = sqrt(M_PI) * vb;
                if (raydep) {
                    const double vl = vL[k];
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const double pv = dev_voigt(ad, v + 1.0 * (mu[m] * vl / vb), vtab) / nrm;   // up-going: :231, :238-239
                        chi[m] += nd * pv;
                        eta[m] += nj * (Uc * pv);
                    }
                } else {                                          // no velocity: one profile for every angle
                    const double pv = dev_voigt(ad, v, vtab) / nrm;
                    const double c1 = nd * pv, h1 = nj * (Uc * pv);
#pragma unroll
                    for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
                }
            } else {
                const double a = al_s[e * 64 + lane];
                const double pv = (nsr_col[(size_t)row * Ns + k] * Ev) * a;          // Vji = g_ij alpha, :284-285, :453-454
                const double c1 = ni * a - nj * pv, h1 = nj * (u_la * pv);           // :286, :613-614
#pragma unroll
                for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
            }
        }
        // ---- the up-going ray's recurrence at this depth (lsx_final_dev.h): the linear rule in the reference's own order, as
        // lsx_depth.hip has it (the end point of a ray can be a heavy cancellation, where a shared reciprocal's 4e-15 shows); the
        // start value belongs to the depth below (Iu is still 0 there) ----
        if (s == 1 && !lower_zero) thermal_start(B1, B0, fabs(zk1 - zk), zmu, c_k, chi, Iu);
        double S[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) S[m] = eta[m] / chi[m];                       // :632
        if constexpr (!PAR) {
            linear_step_ref(s, k == 0, fabs(zk1 - zk), zmu, chi, S, Iu, c_k, S_k, dtau_prev, etab);
        } else {
#pragma unroll
            for (int m = 0; m < NM; ++m) parabolic_step(s, zk, zk1, zk2, zmu[m], chi[m], S[m], Iu[m], c_k[m], S_k[m], c_u[m], S_u[m], etab);
        }
        zk2 = zk1;
        zk1 = zk;
    }
    if constexpr (PAR) parabolic_end(zk1, zk2, zmu, Iu, c_k, S_k, c_u, S_u, etab);
    if (valid) {
        double* o = p.out + ((size_t)blockIdx.y * p.nla + q) * p.nmu + p.mu0;    // emergent value I[0], rh_method.py:638
#pragma unroll
        for (int m = 0; m < NM; ++m) o[m] = Iu[m];
    }
}

// the caller's background of a pass, [matrix][nla][Ns] (depth fastest) -> [matrix][Ns][nla] (wavelength fastest), through a
// 32 x 32 tile in LDS (33 doubles a row: the transposed read walks the banks); both sides move contiguous runs
__global__ void __launch_bounds__(256) k_spectrum_transpose(const double* __restrict__ in, double* __restrict__ out, int nla, int Ns)
{
    __shared__ double tile[32][33];
    const size_t mat = (size_t)blockIdx.x * nla * Ns;
    const int k0 = blockIdx.y * 32, q0 = blockIdx.z * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int qq = q0 + r, k = k0 + threadIdx.x;
        if (qq < nla && k < Ns) tile[r][threadIdx.x] = in[mat + (size_t)qq * Ns + k];
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int k = k0 + r, qq = q0 + threadIdx.x;
        if (k < Ns && qq < nla) out[mat + (size_t)k * nla + qq] = tile[threadIdx.x][r];
    }
}

template <int NM>
void launch_chunk(const SpecParams& p, bool par, dim3 grid, size_t lds, hipStream_t st)
{
    if constexpr (NM <= 4) {
        if (par) { hipLaunchKernelGGL((k_spectrum<NM, true>), grid, dim3(64), lds, st, p); return; }
    }
    hipLaunchKernelGGL((k_spectrum<NM, false>), grid, dim3(64), lds, st, p);
}

// what the host makes of the call's wavelengths: everything a lane needs that does not depend on the column
struct SpecTables {
    std::vector<double> ula, t, ent_alpha, tr_d;
    std::vector<int32_t> off0, off1, blk_ne, ent_tid, tr_i;
    int Emax = 1;
};

template <typename T>
size_t put(std::vector<char>& buf, const std::vector<T>& v)
{
    const size_t at = (buf.size() + 15) & ~(size_t)15;
    buf.resize(at + v.size() * sizeof(T));
    if (!v.empty()) std::memcpy(buf.data() + at, v.data(), v.size() * sizeof(T));
    return at;
}

int spec_tables(const lsx_ctx* c, int nla, const double* w, const double* alpha, SpecTables* S)
{
    const int N = c->Nspect, Nt = c->Ntrans, L = c->L, Ns = c->Nspace;
    const std::vector<double>& lam = c->wave;
    // the context's grid in its tile-major streams
    std::vector<int32_t> place(N, -1);
    for (size_t t = 0; t < c->tiles.size(); ++t)
        for (int j = 0; j < c->tiles[t].nla; ++j) place[c->tiles[t].la0 + j] = (int32_t)(t * (size_t)Ns * L + j);
    for (int la = 0; la < N; ++la)
        if (place[la] < 0) return fail(LSX_EDEVICE, "lsx_hip_spectrum: wavelength %d of the grid belongs to no tile", la);
    // constants of every transition
    S->tr_d.assign((size_t)std::max(1, Nt) * kTrD, 0.0);
    S->tr_i.assign((size_t)std::max(1, Nt) * kTrI, 0);
    std::vector<int> cont_of(Nt, -1);
    int ncont = 0;
    for (int t = 0; t < Nt; ++t) {
        const DevTrans& h = c->htrans[t];
        int32_t* ti = &S->tr_i[(size_t)t * kTrI];
        ti[0] = h.li; ti[1] = h.lj; ti[2] = c->trans_row[t]; ti[3] = h.is_line ? h.atom : -1;
        if (h.is_line) {
            double* td = &S->tr_d[(size_t)t * kTrD];
            td[0] = h.cB; td[1] = h.gij; td[2] = h.AB * (h.gij * h.cB); td[3] = h.lambda0;
        } else {
            cont_of[t] = ncont++;
        }
    }
    // per wavelength: bracket of the grid (upper_bound - 1, clamped; held constant outside), active transitions in table order
    S->ula.resize(nla); S->t.resize(nla); S->off0.resize(nla); S->off1.resize(nla);
    std::vector<std::vector<int32_t>> act(nla);
    S->Emax = 1;
    for (int q = 0; q < nla; ++q) {
        const double x = w[q];
        S->ula[q] = 2.0 * kHC / std::pow(kNM_TO_M * x, 3.0);       // :286
        int l = 0;
        double tt = 0.0;
        if (N >= 2) {
            l = (int)(std::upper_bound(lam.begin(), lam.end(), x) - lam.begin()) - 1;
            l = std::min(std::max(l, 0), N - 2);
            tt = (x - lam[l]) / (lam[l + 1] - lam[l]);
            tt = std::min(std::max(tt, 0.0), 1.0);
        }
        S->t[q] = tt;
        S->off0[q] = place[l];
        S->off1[q] = place[std::min(l + 1, N - 1)];
        for (int t = 0; t < Nt; ++t) {
            const DevTrans& h = c->htrans[t];
            if (h.Nlam < 1) continue;
            if (lam[h.Nblue] <= x && x <= lam[h.Nblue + h.Nlam - 1]) act[q].push_back(t);
        }
        S->Emax = std::max(S->Emax, (int)act[q].size());
    }
    const int nblk = (nla + 63) / 64;
    S->blk_ne.assign(nblk, 0);
    S->ent_tid.assign((size_t)nblk * S->Emax * 64, -1);
    S->ent_alpha.assign((size_t)nblk * S->Emax * 64, 0.0);
    for (int b = 0; b < nblk; ++b)
        for (int lane = 0; lane < 64; ++lane) {
            const int q = std::min(b * 64 + lane, nla - 1);          // a spare lane walks the last wavelength
            const std::vector<int32_t>& a = act[q];
            S->blk_ne[b] = std::max(S->blk_ne[b], (int32_t)a.size());
            for (size_t e = 0; e < a.size(); ++e) {
                const size_t at = ((size_t)b * S->Emax + e) * 64 + lane;
                S->ent_tid[at] = a[e];
                if (cont_of[a[e]] >= 0) S->ent_alpha[at] = alpha[(size_t)cont_of[a[e]] * nla + q];
            }
        }
    return LSX_OK;
}

} // namespace

extern "C" int lsx_hip_spectrum_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_SPEC_WORK, "lsx_hip_spectrum_work_cap", nbytes);
}

extern "C" int lsx_hip_spectrum(lsx_ctx* c, int32_t nla, const double* wavelength, const double* alpha, const double* bg_chi,
                                const double* bg_eta, const double* bg_sca, int32_t nmu, const double* mu, int32_t col0, int32_t ncol,
                                double* dst, size_t nbytes)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c || !wavelength || !mu || !dst) return fail(LSX_EINVAL, "lsx_hip_spectrum: null argument");
    if (nla < 1) return fail(LSX_EINVAL, "lsx_hip_spectrum: nla = %d, need at least one wavelength", (int)nla);
    for (int q = 0; q < nla; ++q) {
        if (!(std::isfinite(wavelength[q]) && wavelength[q] > 0.0))
            return fail(LSX_EINVAL, "lsx_hip_spectrum: wavelength[%d] = %g is not a finite positive number", q, wavelength[q]);
        if (q && !(wavelength[q] > wavelength[q - 1]))
            return fail(LSX_EINVAL, "lsx_hip_spectrum: the wavelengths are not strictly ascending at [%d]", q);
    }
    int rc = final_check_angles("lsx_hip_spectrum", nmu, mu);
    if (!rc) rc = final_check_range(c, "lsx_hip_spectrum", col0, ncol);
    if (rc) return rc;
    const size_t per = (size_t)nla * nmu;
    if (nbytes != (size_t)ncol * per * 8) return fail(LSX_EINVAL, "lsx_hip_spectrum: nbytes does not match [ncol][nla][nmu]");
    if ((bg_chi == nullptr) != (bg_eta == nullptr))
        return fail(LSX_EINVAL, "lsx_hip_spectrum: bg_chi and bg_eta are given together or both NULL");
    const bool xbg = bg_chi != nullptr;
    const bool want_sca = xbg && c->sca_per_lambda;
    if (want_sca != (bg_sca != nullptr))
        return fail(LSX_EINVAL, "lsx_hip_spectrum: bg_sca is %s", want_sca ? "needed: the context's scattering coefficient is per wavelength"
                                                                           : "given, but only read next to bg_chi in a sca_per_lambda context");
    if (c->Ncont > 0 && !alpha) return fail(LSX_EINVAL, "lsx_hip_spectrum: alpha is NULL and the context has %d continua", c->Ncont);
    if ((rc = final_check_depths(c, "lsx_hip_spectrum"))) return rc;
    if ((rc = final_check_columns(c, "lsx_hip_spectrum", col0, ncol, FINAL_OTHER_WAVELENGTH))) return rc;
    SpecTables S;
    if ((rc = spec_tables(c, nla, wavelength, alpha, &S))) return rc;
    const size_t lds = ((size_t)S.Emax * 64 + (size_t)c->Ntrans * 4) * (sizeof(double) + sizeof(int32_t));
    if (lds + (LSX_EXP_TAB + 64) * sizeof(double) > kLdsLimit)
        return fail(LSX_EUNSUPPORTED, "lsx_hip_spectrum: %d transitions overlap at one wavelength: their tables (%zu bytes) do not fit "
                                      "a workgroup's LDS", S.Emax, lds);

    HIPCHK(hipSetDevice(c->device));
    // ---- the call's tables: one buffer, one copy ----
    std::vector<char> buf;
    const std::vector<double> wv(wavelength, wavelength + nla), muv(mu, mu + nmu);
    const size_t a_wav = put(buf, wv), a_ula = put(buf, S.ula), a_t = put(buf, S.t), a_al = put(buf, S.ent_alpha), a_trd = put(buf, S.tr_d),
                 a_mu = put(buf, muv), a_o0 = put(buf, S.off0), a_o1 = put(buf, S.off1), a_ne = put(buf, S.blk_ne),
                 a_tid = put(buf, S.ent_tid), a_tri = put(buf, S.tr_i);
    GrowBuf& tab = c->buf[BUF_SPEC_TAB];
    if ((rc = tab.reserve(c, buf.size()))) return rc;
    HIPCHK(hipMemcpyAsync(tab.p, buf.data(), buf.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                     // (the host buffer may go out of scope on any return below)

    // ---- columns per pass: the pass's arrays stay under the cap (one column's need if that alone is more) ----
    const size_t mat = (size_t)nla * c->Nspace;                  // one background array of a column
    const size_t nstream = xbg ? (want_sca ? 3 : 2) : 0;
    const size_t wcol = per + 2 * nstream * mat;                 // the result; the caller's arrays as they come and transposed
    GrowBuf& work = c->buf[BUF_SPEC_WORK];
    const size_t chunk = pass_columns(ncol, work.cap, kWorkCapDefault, wcol, kGridYLimit);
    if ((rc = work.reserve(c, chunk * wcol * 8))) return rc;

    SpecParams p{};
    final_fill_angles(p, c);       // (final_fill is not for this unit: its tables are the call's, and SpecParams names no grid of the context)
    p.Ns = c->Nspace; p.NLtot = c->NLtot; p.Ncont = c->Ncont;
    p.Ntrans = c->Ntrans; p.L = c->L; p.nmu = nmu; p.nla = nla; p.Emax = S.Emax;
    p.sca_per_lambda = c->sca_per_lambda; p.explicit_bg = xbg ? 1 : 0;
    p.til_col = (int64_t)c->til_col; p.sca_col = (int64_t)c->sca_col;
    const char* tb = tab.p;
    p.wav = (const double*)(tb + a_wav); p.ula = (const double*)(tb + a_ula); p.t = (const double*)(tb + a_t);
    p.ent_alpha = (const double*)(tb + a_al); p.tr_d = (const double*)(tb + a_trd); p.mu = (const double*)(tb + a_mu);
    p.off0 = (const int32_t*)(tb + a_o0); p.off1 = (const int32_t*)(tb + a_o1); p.blk_ne = (const int32_t*)(tb + a_ne);
    p.ent_tid = (const int32_t*)(tb + a_tid); p.tr_i = (const int32_t*)(tb + a_tri);
    p.exp2_tab = c->d_exp2_tab;
    p.height = c->d_height; p.temperature = c->d_temperature; p.n = c->d_n; p.nsr = c->d_nsr;
    p.bnd = c->d_bnd;
    p.bgchi_T = c->d_bgchi; p.bgeta_T = c->d_bgeta; p.J_T = c->d_J[c->jcur];      // what lsx_get(LSX_J) returns at this moment
    p.sca = c->d_sca;
    const bool par = c->solver == LSX_SOLVER_PARABOLIC;
    const double* const src[3] = {bg_chi, bg_eta, bg_sca};

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(col0 + b0);
        double* wk = work.as<double>();
        p.out = wk;
        double* raw = wk + nb * per;                              // [stream][nb][nla][Ns] as the caller has them
        double* tr = raw + nstream * nb * mat;                    // [stream][nb][Ns][nla]
        if (xbg) {
            for (size_t a = 0; a < nstream; ++a)
                HIPCHK(hipMemcpyAsync(raw + a * nb * mat, src[a] + b0 * mat, nb * mat * 8, hipMemcpyHostToDevice, c->stream));
            const dim3 tg((unsigned)(nstream * nb), (unsigned)((c->Nspace + 31) / 32), (unsigned)((nla + 31) / 32));
            hipLaunchKernelGGL(k_spectrum_transpose, tg, dim3(32, 8), 0, c->stream, raw, tr, (int)nla, c->Nspace);
            HIPCHK(hipGetLastError());
            p.xchi = tr; p.xeta = tr + nb * mat; p.xsca = want_sca ? tr + 2 * nb * mat : nullptr;
        }
        const dim3 grid((unsigned)((nla + 63) / 64), (unsigned)nb);
        for (int m0 = 0; m0 < nmu;) {                 // angles in register chunks of 8, 4, 2, 1 (the parabolic rule's window: at most 4)
            const int left = nmu - m0;
            p.mu0 = m0;
            if (left >= 8 && !par) { launch_chunk<8>(p, par, grid, lds, c->stream); m0 += 8; }
            else if (left >= 4) { launch_chunk<4>(p, par, grid, lds, c->stream); m0 += 4; }
            else if (left >= 2) { launch_chunk<2>(p, par, grid, lds, c->stream); m0 += 2; }
            else { launch_chunk<1>(p, par, grid, lds, c->stream); m0 += 1; }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dst + b0 * per, p.out, nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the pass's arrays are re-used by the next pass; the host tables go out of scope
    }
    return LSX_OK;
}
