// lsx_losses.hip -- final-pass formal solution: the radiative flux, its divergence (the net radiative cooling) and how that cooling
// divides among the transitions, from what a context holds (include/lsx_hip_losses.h, lsx_hip_radiative_losses).  Read-only on the
// context; gfx950 only.  A file of its own beside lsx_rates.hip, with the same walk.
//
// Reference lines restated here (the rest: lsx_final_dev.h, whose column set-up, start values and recurrence steps the walk uses):
//   rh_method.py:599-632           opacity, emissivity, source function
//   rh_method.py:661-665           wlamu = wla (wmu / 2) 4 pi
//   rh_method.py:425-455, 157-196  wla of a line (wlambda wphi / hc) and of a continuum (wlambda / lambda / h), g_ij
//
// Two stages, no atomics, every sum in a fixed order:
//   k_losses_pass<NM, PAR>  the mapping of k_rates_pass: one wavefront = 64 consecutive wavelengths of one column, a lane owns one
//     wavelength and carries NM of the context's rays in registers, first down, then up.  Per depth it adds to five angle sums in the
//     work array:  H = sum (wmu / 2) mu (+-I),  D = sum (wmu / 2) (eta - chi I)  with the ray- and direction-dependent chi and eta
//     inside the sum,  Jp = sum (wmu / 2) I  (every continuum at that wavelength),  and per wavelength of a line  P = sum (wmu / 2)
//     phi I,  Phi = sum (wmu / 2) phi.  The down-going half of a depth is parked there and completed by the SAME lane on its way up
//     (and by the next group of rays, a launch later on the same stream): one writer per cell.  Layout [column][k][lambda]: every
//     access of a wavefront is one contiguous run.  The next depth's stream operands (background, sigma, J, Boltzmann factor) are
//     fetched before this depth's stores are issued.  LDS: the exponential's table (1 kB); no depth limit.
//   k_losses_flux           one thread per (column, depth): F = 4 pi sum wnu H, Q = 4 pi sum wnu D over ascending wavelength.
//   k_losses_trans          one thread per (column, transition, depth): Qt, the transition's own wavelengths in ascending order with
//     (hc / lambda) 4 pi wla; a line through P and Phi, a continuum through Jp, g = nStar_i / nStar_j E and W = sum (wmu / 2).
//   k_losses_transpose      H and D of a pass from [k][lambda] to the entry's [lambda][k].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)256 << 20;      // bytes (include/lsx_hip_losses.h)

struct LossParams {
    int32_t Ns, Nspect, NLtot, Ncont, L, Nrays, SNl, Ntrans;
    int32_t col0, mu0, first;   // first column of the launch; first ray of this launch's group; the group is the call's first
    int32_t phi_compact, sca_per_lambda, phi_G, ncols;      // ncols: columns of the launch (second stage)
    int32_t Nlines, pad_;
    int64_t til_col, phi_col, sca_col;
    const double *wavelength, *u_la, *exp2_tab, *zmu, *muz, *wmuh, *wl, *alpha, *wnu;
    const int32_t* la_ptr;      // [Nspect + 1] into ents
    const FinalEnt* ents;
    const int32_t* la_tile;     // [Nspect][2]: tile, place in the tile
    const DevTrans* trans;
    const int32_t* trans_row;   // per transition: continua: row of nsr
    const uint8_t* active;
    const double *height, *temperature, *n, *nsr, *wphi, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    double *Hw, *Dw, *Jp;       // work: [launch column][k][Nspect] each
    double2* PP;                // work: [launch column][k][SNl] (P, Phi)
    double wsum;                // sum of wmu / 2 over rays and directions
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store): null = thermalised below, zero above, as it was
    double *F, *Q, *Qt, *Ht, *Dt;   // device results of a pass: [launch column][k], [launch column][Ntrans][k], [launch column][Nspect][k]
};

// waves per SIMD of the pass's instances by rays per lane, as DESIGN.md 4.19 states them: asked of the compiler, so that the boundary's
// arm of the start values moves no instance to another count.  What holds this table, the one in DESIGN.md and the
// compiler together is tests/test_radiative_losses_host.py: it reads every instance's waves per SIMD from the compiler's report and compares
// them with the same table (a count the allocator cannot reach shows there as another count or as scratch)
constexpr int losses_waves(int nm, bool par) { return nm == 1 ? (par ? 4 : 5) : nm == 2 ? (par ? 3 : 4) : nm == 3 ? 3 : nm == 4 ? (par ? 2 : 3) : 2; }
static_assert(losses_waves(1, false) >= losses_waves(5, false) && losses_waves(5, true) == 2, "more rays per lane never means more waves; five rays: two");

template <int NM, bool PAR>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(losses_waves(NM, PAR), losses_waves(NM, PAR))))
k_losses_pass(const LossParams p)
{
    __shared__ double etab_s[LSX_EXP_TAB];
    for (int e = threadIdx.x; e < LSX_EXP_TAB; e += 64) etab_s[e] = p.exp2_tab[e];
    __syncthreads();
    const lds_f64* etab = (const lds_f64*)etab_s;

    const int Ns = p.Ns, L = p.L;
    const int la_raw = blockIdx.x * 64 + threadIdx.x;
    const bool valid = la_raw < p.Nspect;
    const int la = valid ? la_raw : p.Nspect - 1;          // every lane walks a wavelength (w2 / w3 are wave-wide); spare ones store nothing
    const size_t col = (size_t)p.col0 + blockIdx.y;
    const FinalColumn f = final_column(p, col, la);
    const double wav = p.wavelength[la], u_la = p.u_la[la];
    const size_t wbase = (size_t)blockIdx.y * Ns * p.Nspect + la;          // + k Nspect: this wavelength's cell of H, D and Jp
    double2* PP = p.PP + (size_t)blockIdx.y * Ns * p.SNl;                  // + k SNl + cell

    double zmu[NM], hw[NM], hwmu[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        zmu[m] = p.zmu[p.mu0 + m];
        hw[m] = p.wmuh[p.mu0 + m];
        hwmu[m] = hw[m] * p.muz[p.mu0 + m];
    }

    for (int dir = 0; dir < 2; ++dir) {                    // down, then up (the profile store's order of directions)
        const bool up = dir == 1;
        const bool fresh = p.first && !up;                 // the first visit of the call: the sums start here
        // the profile of line entry t at depth kd for ray m of this group
        auto phi_at = [&](const FinalEnt& t, int kd, int m) -> double {
            const size_t x = p.phi_compact ? (size_t)kd : ((size_t)dir * Ns + kd) * p.Nrays + (p.mu0 + m);
            return p.phi_T[phi_elem(col, p.phi_G, (size_t)p.phi_col, (size_t)t.phi_base, x, t.phi_len, t.phi_l)];
        };
        // add this group's rays at depth kd to the angle sums; cv, ev: opacity and emissivity of that depth per ray
        auto accumulate = [&](int kd, const double (&Iv)[NM], const double (&cv)[NM], const double (&ev)[NM]) {
            if (!valid) return;
            double js = 0.0, hs = 0.0, ds = 0.0;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                js += hw[m] * Iv[m];
                hs += hwmu[m] * Iv[m];
                ds += hw[m] * (ev[m] - cv[m] * Iv[m]);
            }
            const size_t w = wbase + (size_t)kd * p.Nspect;
            p.Jp[w] = (fresh ? 0.0 : p.Jp[w]) + js;
            p.Hw[w] = (fresh ? 0.0 : p.Hw[w]) + (up ? hs : -hs);
            p.Dw[w] = (fresh ? 0.0 : p.Dw[w]) + ds;
            for (int e = f.e0; e < f.e1; ++e) {
                const FinalEnt& t = p.ents[e];
                if (!t.is_line) continue;
                double ps = 0.0, fs = 0.0;
                if (p.phi_compact) {
                    const double pv = phi_at(t, kd, 0);
#pragma unroll
                    for (int m = 0; m < NM; ++m) { ps += (hw[m] * pv) * Iv[m]; fs += hw[m] * pv; }
                } else {
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const double wp = hw[m] * phi_at(t, kd, m);
                        ps += wp * Iv[m];
                        fs += wp;
                    }
                }
                double2* c = PP + (size_t)kd * p.SNl + t.cell;
                double2 v = fresh ? make_double2(0.0, 0.0) : *c;
                v.x += ps;
                v.y += fs;
                *c = v;
            }
        };
        // the same from a depth's opacity and source function (the depth behind the current one: the start value, the parabolic rule)
        auto accumulate_cs = [&](int kd, const double (&Iv)[NM], const double (&cv)[NM], const double (&Sv)[NM]) {
            double ev[NM];
#pragma unroll
            for (int m = 0; m < NM; ++m) ev[m] = Sv[m] * cv[m];
            accumulate(kd, Iv, cv, ev);
        };

        double Iu[NM], c_k[NM], S_k[NM], c_u[NM], S_u[NM], dtau_prev[NM];
        final_state_init(Iu, c_k, S_k, c_u, S_u, dtau_prev);
        double zk1 = 0.0, zk2 = 0.0;       // heights of the two depths behind the current one
        int k1 = 0;                        // the depth behind the current one

        // the stream operands of a depth, fetched one depth ahead
        const int kfirst = up ? Ns - 1 : 0;
        double n_c0 = f.bgchi[(size_t)kfirst * L], n_be = f.bgeta[(size_t)kfirst * L], n_sc = f.sca[(size_t)kfirst * f.sstr],
               n_jd = f.Jd[(size_t)kfirst * L], n_ev = f.Eb ? f.Eb[(size_t)kfirst * L] : 0.0;

        for (int s = 0; s < Ns; ++s) {     // step along the ray
            const int k = up ? Ns - 1 - s : s;
            const double zk = f.z[k];
            const double c0 = n_c0, h0 = n_be + n_sc * n_jd, Ev = n_ev;
            if (s + 1 < Ns) {              // the next depth's operands: in flight before this depth's stores
                const int kn = up ? k - 1 : k + 1;
                n_c0 = f.bgchi[(size_t)kn * L];
                n_be = f.bgeta[(size_t)kn * L];
                n_sc = f.sca[(size_t)kn * f.sstr];
                n_jd = f.Jd[(size_t)kn * L];
                n_ev = f.Eb ? f.Eb[(size_t)kn * L] : 0.0;
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
                    if (p.phi_compact) {
                        const double pv = phi_at(t, k, 0);
                        const double c1 = nd * pv, h1 = nj * (t.Uc * pv);
#pragma unroll
                        for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
                    } else {
#pragma unroll
                        for (int m = 0; m < NM; ++m) {
                            const double pv = phi_at(t, k, m);
                            chi[m] += nd * pv;
                            eta[m] += nj * (t.Uc * pv);
                        }
                    }
                } else {
                    const double pv = (f.nsr_col[(size_t)t.row * Ns + k] * Ev) * t.a;     // Vji = g_ij alpha, :284-285, :453-454
                    const double c1 = ni * t.a - nj * pv, h1 = nj * (u_la * pv);        // :286, :613-614
#pragma unroll
                    for (int m = 0; m < NM; ++m) { chi[m] += c1; eta[m] += h1; }
                }
            }
            // ---- the recurrence at this depth ----
            if (s == 1) {                  // the value the rays start with belongs to the depth behind
                final_start(p, col, la, up, k1, k, wav, fabs(zk1 - zk), zmu, c_k, chi, Iu);
                accumulate_cs(k1, Iu, c_k, S_k);
            }
            if constexpr (!PAR) {
                linear_step(s, s == Ns - 1, 0.5 * fabs(zk1 - zk), zmu, chi, eta, Iu, c_k, S_k, dtau_prev, etab);
                if (s >= 1) accumulate(k, Iu, chi, eta);
            } else {
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    parabolic_step(s, zk, zk1, zk2, zmu[m], chi[m], eta[m] / chi[m], Iu[m], c_k[m], S_k[m], c_u[m], S_u[m], etab);
                if (s >= 2) accumulate_cs(k1, Iu, c_u, S_u);      // (after the shift the finished depth is the window's u)
            }
            zk2 = zk1;
            zk1 = zk;
            k1 = k;
        }
        if constexpr (PAR) {
            parabolic_end(zk1, zk2, zmu, Iu, c_k, S_k, c_u, S_u, etab);
            accumulate_cs(k1, Iu, c_k, S_k);
        }
    }
}


// one thread per (launch column, depth): the sums over the merged grid, ascending, with wnu; then 4 pi
__global__ void __launch_bounds__(256) k_losses_flux(const LossParams p)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)p.ncols * p.Ns) return;
    const double* __restrict__ hrow = p.Hw + id * p.Nspect;       // id = launch column * Ns + k
    const double* __restrict__ drow = p.Dw + id * p.Nspect;
    double f = 0.0, q = 0.0;
    for (int la = 0; la < p.Nspect; ++la) {
        const double w = p.wnu[la];
        f += w * hrow[la];
        q += w * drow[la];
    }
    p.F[id] = (4.0 * M_PI) * f;
    p.Q[id] = (4.0 * M_PI) * q;
}

// one thread per (launch column, transition, depth): the sum over the transition's own wavelengths, ascending, with
// (hc / lambda) 4 pi wla:  Qt = sum [ n_j (Uji + Vji I) - n_i Vij I ]
__global__ void __launch_bounds__(256) k_losses_trans(const LossParams p)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int Ns = p.Ns;
    if (id >= (size_t)p.ncols * p.Ntrans * Ns) return;
    const int k = (int)(id % Ns);
    const int t = (int)((id / Ns) % p.Ntrans);
    const size_t cb = id / ((size_t)Ns * p.Ntrans);
    const size_t col = (size_t)p.col0 + cb;
    const DevTrans h = p.trans[t];
    const uint8_t* __restrict__ act = p.active + (size_t)t * p.Nspect + h.Nblue;
    const double* __restrict__ wl = p.wl + h.wl_off;
    const double* __restrict__ lam = p.wavelength + h.Nblue;
    const double ni = p.n[(col * p.NLtot + h.li) * Ns + k], nj = p.n[(col * p.NLtot + h.lj) * Ns + k];
    double q = 0.0;
    if (h.is_line) {
        // Vij = cB phi, Vji = g Vij, Uji = (Aji / Bji) Vji (rh_method.py:279-281); wla = wlambda wphi / hc (:451)
        const double w4 = (4.0 * M_PI) * p.wphi[(col * p.Nlines + h.line_idx) * Ns + k];
        const double2* __restrict__ pp = p.PP + (cb * Ns + k) * p.SNl + h.phi_off;
        const double vji = h.gij * h.cB, uji = h.AB * vji;
        for (int lt = 0; lt < h.Nlam; ++lt) {
            if (!act[lt]) continue;
            const double w = (kHC / (kNM_TO_M * lam[lt])) * (w4 * wl[lt]);
            const double2 v = pp[lt];
            q += w * (nj * (uji * v.y + vji * v.x) - ni * (h.cB * v.x));
        }
    } else {
        // Vij = alpha, Vji = g_ij alpha, Uji = (2hc / lambda^3) Vji, g_ij = nStar_i / nStar_j exp(-hc / k lambda T) (:284-286, :453-455)
        const double* __restrict__ al = p.alpha + h.wl_off;
        const double nsr = p.nsr[(col * p.Ncont + p.trans_row[t]) * Ns + k];
        const double* __restrict__ jp = p.Jp + (cb * Ns + k) * p.Nspect + h.Nblue;
        const double* __restrict__ Ecol = p.E_T + col * p.til_col;
        for (int lt = 0; lt < h.Nlam; ++lt) {
            if (!act[lt]) continue;
            const int la = h.Nblue + lt;
            const double E = Ecol[((size_t)p.la_tile[2 * la] * Ns + k) * p.L + p.la_tile[2 * la + 1]];
            const double w = (kHC / (kNM_TO_M * lam[lt])) * ((4.0 * M_PI) * wl[lt]);
            const double a = al[lt], Jv = jp[lt];
            const double vji = (nsr * E) * a, uji = p.u_la[la] * vji;
            q += w * (nj * (uji * p.wsum + vji * Jv) - ni * (a * Jv));
        }
    }
    p.Qt[id] = q;
}

// H and D of a pass from the work array's [launch column][k][lambda] to the entry's [launch column][lambda][k]
__global__ void __launch_bounds__(256) k_losses_transpose(const LossParams p)
{
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)p.Ns * p.Nspect;
    if (id >= (size_t)p.ncols * per) return;
    const size_t cb = id / per, r = id % per;
    const size_t k = r / p.Nspect, la = r % p.Nspect;             // consecutive threads read consecutive wavelengths
    const size_t o = cb * per + la * p.Ns + k;
    if (p.Ht) p.Ht[o] = p.Hw[id];
    if (p.Dt) p.Dt[o] = p.Dw[id];
}

template <int NM>
void launch_pass(const LossParams& p, bool par, dim3 grid, hipStream_t st)
{
    if (par) hipLaunchKernelGGL((k_losses_pass<NM, true>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((k_losses_pass<NM, false>), grid, dim3(64), 0, st, p);
}

// H, D, Jp and the (P, Phi) pairs of the lines
size_t work_doubles_per_column(const lsx_ctx* c) { return (size_t)c->Nspace * (3 * (size_t)c->Nspect + 2 * (size_t)c->SNl); }

} // namespace

extern "C" int lsx_hip_radiative_losses_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_LOSSES_WORK, "lsx_hip_radiative_losses_work_cap", nbytes);
}

extern "C" int lsx_hip_radiative_losses(lsx_ctx* c, int32_t col0, int32_t ncol, const double* wnu, double* F, double* Q, double* Qt,
                                        double* H, double* D, size_t nbytes_FQ, size_t nbytes_Qt, size_t nbytes_HD)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c) return fail(LSX_EINVAL, "lsx_hip_radiative_losses: null context");
    if (!F && !Q && !Qt && !H && !D) return fail(LSX_EINVAL, "lsx_hip_radiative_losses: all five outputs are NULL");
    int rc = final_check_depths(c, "lsx_hip_radiative_losses");
    if (!rc) rc = final_check_range(c, "lsx_hip_radiative_losses", col0, ncol);
    if (rc) return rc;
    const size_t Ns = (size_t)c->Nspace, Nspect = (size_t)c->Nspect;
    const size_t per_t = (size_t)c->Ntrans * Ns, per_m = Nspect * Ns;
    if ((F || Q) && nbytes_FQ != (size_t)ncol * Ns * 8) return fail(LSX_EINVAL, "lsx_hip_radiative_losses: nbytes_FQ does not match [ncol][Nspace]");
    if (Qt && nbytes_Qt != (size_t)ncol * per_t * 8) return fail(LSX_EINVAL, "lsx_hip_radiative_losses: nbytes_Qt does not match [ncol][Ntrans][Nspace]");
    if ((H || D) && nbytes_HD != (size_t)ncol * per_m * 8) return fail(LSX_EINVAL, "lsx_hip_radiative_losses: nbytes_HD does not match [ncol][Nspect][Nspace]");
    if ((rc = final_check_columns(c, "lsx_hip_radiative_losses", col0, ncol, FINAL_OWN_RAYS))) return rc;
    if (wnu)
        for (size_t la = 0; la < Nspect; ++la)
            if (!std::isfinite(wnu[la])) return fail(LSX_EINVAL, "lsx_hip_radiative_losses: wnu[%zu] is not finite", la);
    HIPCHK(hipSetDevice(c->device));
    if ((rc = final_tables(c, "lsx_hip_radiative_losses"))) return rc;
    if (!c->d_losses_wnu) {        // the trapezoid rule in frequency over the merged grid, formed once in the grid code (lsx_grid.cpp)
        c->losses_wnu.assign(Nspect, 0.0);
        if ((rc = lsx_hip_frequency_weights(c->Nspect, c->wave.data(), c->losses_wnu.data()))) return rc;
        if ((rc = dmalloc(&c->d_losses_wnu, Nspect))) return rc;
    }

    // columns per pass: the work arrays stay under the cap (one column's need if that alone is more; a grid's y limit)
    GrowBuf& work = c->buf[BUF_LOSSES_WORK];
    const size_t wcol = work_doubles_per_column(c);
    const size_t chunk = pass_columns(ncol, work.cap, kWorkCapDefault, wcol, kGridYLimit);
    if ((rc = work.reserve(c, (chunk * wcol + 2) * 8))) return rc;       // (+ 2: the pairs start on a 16-byte boundary)
    // the results of a chunk leave through the staging buffer: F, Q, Qt, and H / D in the entry's layout where asked for
    const size_t stage_need = chunk * (2 * Ns + per_t + (H ? per_m : 0) + (D ? per_m : 0));
    if ((rc = ensure_stage(c, stage_need))) return rc;
    HIPCHK(hipMemcpyAsync(c->d_losses_wnu, wnu ? wnu : c->losses_wnu.data(), Nspect * 8, hipMemcpyHostToDevice, c->stream));

    LossParams p{};
    final_fill(p, c);
    p.SNl = c->SNl; p.Ntrans = c->Ntrans; p.Nlines = c->Nlines;
    p.zmu = c->d_zmu; p.muz = c->d_muz; p.wmuh = c->d_wmuh; p.wl = c->d_wl; p.alpha = c->d_alpha; p.wnu = c->d_losses_wnu;
    p.trans = c->d_trans; p.trans_row = c->d_final_row; p.active = c->d_active;
    p.wphi = c->d_wphi;
    p.wsum = 0.0;
    for (int dir = 0; dir < 2; ++dir)
        for (int m = 0; m < c->Nrays; ++m) p.wsum += c->wmuh[m];
    const bool par = c->solver == LSX_SOLVER_PARABOLIC;
    const int group = 5;                       // rays a lane carries at a time (registers: DESIGN.md 4.19)

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(col0 + b0);
        p.ncols = (int32_t)nb;
        p.Hw = work.as<double>();
        p.Dw = p.Hw + nb * per_m;
        p.Jp = p.Dw + nb * per_m;
        p.PP = reinterpret_cast<double2*>(p.Hw + ((3 * nb * per_m + 1) & ~(size_t)1));
        double* st = c->d_stage;
        p.F = st; st += nb * Ns;
        p.Q = st; st += nb * Ns;
        p.Qt = st; st += nb * per_t;
        p.Ht = H ? st : nullptr; st += H ? nb * per_m : 0;
        p.Dt = D ? st : nullptr;
        const dim3 grid((unsigned)((c->Nspect + 63) / 64), (unsigned)nb);
        for (int m0 = 0; m0 < c->Nrays;) {
            const int take = std::min(group, c->Nrays - m0);
            p.mu0 = m0;
            p.first = m0 == 0;
            switch (take) {
            case 5: launch_pass<5>(p, par, grid, c->stream); break;
            case 4: launch_pass<4>(p, par, grid, c->stream); break;
            case 3: launch_pass<3>(p, par, grid, c->stream); break;
            case 2: launch_pass<2>(p, par, grid, c->stream); break;
            default: launch_pass<1>(p, par, grid, c->stream); break;
            }
            m0 += take;
        }
        if (F || Q) hipLaunchKernelGGL(k_losses_flux, dim3((unsigned)((nb * Ns + 255) / 256)), dim3(256), 0, c->stream, p);
        if (Qt && per_t) hipLaunchKernelGGL(k_losses_trans, dim3((unsigned)((nb * per_t + 255) / 256)), dim3(256), 0, c->stream, p);
        if (H || D) hipLaunchKernelGGL(k_losses_transpose, dim3((unsigned)((nb * per_m + 255) / 256)), dim3(256), 0, c->stream, p);
        HIPCHK(hipGetLastError());
        if (F) HIPCHK(hipMemcpyAsync(F + b0 * Ns, p.F, nb * Ns * 8, hipMemcpyDeviceToHost, c->stream));
        if (Q) HIPCHK(hipMemcpyAsync(Q + b0 * Ns, p.Q, nb * Ns * 8, hipMemcpyDeviceToHost, c->stream));
        if (Qt && per_t) HIPCHK(hipMemcpyAsync(Qt + b0 * per_t, p.Qt, nb * per_t * 8, hipMemcpyDeviceToHost, c->stream));
        if (H) HIPCHK(hipMemcpyAsync(H + b0 * per_m, p.Ht, nb * per_m * 8, hipMemcpyDeviceToHost, c->stream));
        if (D) HIPCHK(hipMemcpyAsync(D + b0 * per_m, p.Dt, nb * per_m * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the work arrays and the staging buffer are re-used by the next chunk
    }
    return LSX_OK;
}
