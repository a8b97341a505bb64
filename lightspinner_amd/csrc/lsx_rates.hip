// lsx_rates.hip -- final-pass formal solution: the radiative rates Rij / Rji of every transition from what a context holds
// (include/lsx_hip_rates.h, lsx_hip_radiative_rates).  Read-only on the context; gfx950 only.
//
// Reference lines restated here (the rest: lsx_final_dev.h, whose column set-up, start values and recurrence steps the walk uses):
//   rh_method.py:599-632           opacity, emissivity, source function
//   rh_method.py:661-665, 691-692  wlamu = wla (wmu / 2) 4 pi; Rij += I Vij wlamu; Rji += (Uji + I Vij) wlamu
//   rh_method.py:425-455, 157-196  wla of a line (wlambda wphi / hc) and of a continuum (wlambda / lambda / h), g_ij
//
// Two stages, no atomics, every sum in a fixed order:
//   k_rates_pass<NM, PAR>   one wavefront = 64 consecutive wavelengths of one column, a lane owns one wavelength and carries NM of the
//     context's rays in registers, first down, then up.  What the rates need of the intensity factors through three angle sums per
//     depth:  Jp[la][k] = sum (wmu / 2) I  (every continuum at that wavelength: Vij = alpha does not depend on the ray),  and per
//     wavelength of a line  P[l][k] = sum (wmu / 2) phi I,  Phi[l][k] = sum (wmu / 2) phi.  They live in the work array; the
//     down-going half of a depth is parked there and completed by the SAME lane on its way up (and by the next group of rays, a
//     launch later on the same stream): no ordering problem, no second writer.  The profile of every ray and direction is read from
//     the context's store through phi_elem (either layout): no Voigt evaluation, and profiles handed over as arrays work like any other.
//     LDS: the exponential's table (1 kB); no depth limit.
//   k_rates_reduce          one thread per (column, transition, depth) sums the transition's own wavelengths in ascending order with
//     4 pi wla, and forms the three rates.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)256 << 20;      // bytes (include/lsx_hip_rates.h)

struct RatesParams {
    int32_t Ns, Nspect, NLtot, Ncont, L, Nrays, SNl, Ntrans;
    int32_t col0, mu0, first;   // first column of the launch; first ray of this launch's group; the group is the call's first
    int32_t phi_compact, sca_per_lambda, phi_G, ncols;      // ncols: columns of the launch (k_rates_reduce)
    int32_t Nlines, pad_;
    int64_t til_col, phi_col, sca_col;
    const double *wavelength, *u_la, *exp2_tab, *zmu, *wmuh, *wl, *alpha;
    const int32_t* la_ptr;      // [Nspect + 1] into ents
    const FinalEnt* ents;
    const int32_t* la_tile;     // [Nspect][2]: tile, place in the tile
    const DevTrans* trans;
    const int32_t* trans_row;   // per transition: continua: row of nsr (the entry's own copy: the context makes its table only for the ray-serial sweep)
    const uint8_t* active;
    const double *height, *temperature, *n, *nsr, *wphi, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    double* Jp;                 // work: [launch column][k][Nspect]
    double2* PP;                // work: [launch column][k][SNl] (P, Phi)
    double wsum;                // sum of wmu / 2 over rays and directions
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store): null = thermalised below, zero above, as it was
    double *Rij, *Rji, *Rji_ref;   // [launch column][Ntrans][k], device
};

// waves per SIMD of the pass's instances by rays per lane, as DESIGN.md 4.11 states them: asked of the compiler, so that the boundary's
// arm of the start values moves no instance to another count.  What holds this table, the one in DESIGN.md and the
// compiler together is tests/test_radiative_rates_host.py: it reads every instance's waves per SIMD from the compiler's report and compares
// them with the same table (a count the allocator cannot reach shows there as another count or as scratch)
constexpr int rates_waves(int nm, bool par) { return nm == 1 ? (par ? 4 : 6) : nm == 2 ? (par ? 4 : 5) : nm == 3 ? (par ? 3 : 4) : nm == 4 ? 3 : 2; }
static_assert(rates_waves(1, false) >= rates_waves(5, false) && rates_waves(5, true) == 2, "more rays per lane never means more waves; five rays: two");

template <int NM, bool PAR>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(rates_waves(NM, PAR), rates_waves(NM, PAR))))
k_rates_pass(const RatesParams p)
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
    double* Jp = p.Jp + (size_t)blockIdx.y * Ns * p.Nspect + la;           // + k Nspect
    double2* PP = p.PP + (size_t)blockIdx.y * Ns * p.SNl;                  // + k SNl + cell

    double zmu[NM], hw[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        zmu[m] = p.zmu[p.mu0 + m];
        hw[m] = p.wmuh[p.mu0 + m];
    }

    for (int dir = 0; dir < 2; ++dir) {                    // down, then up (the profile store's order of directions)
        const bool up = dir == 1;
        const bool fresh = p.first && !up;                 // the first visit of the call: the sums start here
        // the profile of line entry t at depth kd for ray m of this group
        auto phi_at = [&](const FinalEnt& t, int kd, int m) -> double {
            const size_t x = p.phi_compact ? (size_t)kd : ((size_t)dir * Ns + kd) * p.Nrays + (p.mu0 + m);
            return p.phi_T[phi_elem(col, p.phi_G, (size_t)p.phi_col, (size_t)t.phi_base, x, t.phi_len, t.phi_l)];
        };
        // add this group's rays at depth kd to the angle sums
        auto accumulate = [&](int kd, const double (&Iv)[NM]) {
            if (!valid) return;
            double js = 0.0;
#pragma unroll
            for (int m = 0; m < NM; ++m) js += hw[m] * Iv[m];
            double* jc = Jp + (size_t)kd * p.Nspect;
            *jc = (fresh ? 0.0 : *jc) + js;
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

        double Iu[NM], c_k[NM], S_k[NM], c_u[NM], S_u[NM], dtau_prev[NM];
        final_state_init(Iu, c_k, S_k, c_u, S_u, dtau_prev);
        double zk1 = 0.0, zk2 = 0.0;       // heights of the two depths behind the current one
        int k1 = 0;                        // the depth behind the current one

        for (int s = 0; s < Ns; ++s) {     // step along the ray
            const int k = up ? Ns - 1 - s : s;
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
                accumulate(k1, Iu);
            }
            if constexpr (!PAR) {
                linear_step(s, s == Ns - 1, 0.5 * fabs(zk1 - zk), zmu, chi, eta, Iu, c_k, S_k, dtau_prev, etab);
                if (s >= 1) accumulate(k, Iu);
            } else {
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    parabolic_step(s, zk, zk1, zk2, zmu[m], chi[m], eta[m] / chi[m], Iu[m], c_k[m], S_k[m], c_u[m], S_u[m], etab);
                if (s >= 2) accumulate(k1, Iu);
            }
            zk2 = zk1;
            zk1 = zk;
            k1 = k;
        }
        if constexpr (PAR) {
            parabolic_end(zk1, zk2, zmu, Iu, c_k, S_k, c_u, S_u, etab);
            accumulate(k1, Iu);
        }
    }
}


// one thread per (launch column, transition, depth): the sum over the transition's own wavelengths, ascending, with 4 pi wla
__global__ void __launch_bounds__(256) k_rates_reduce(const RatesParams p)
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
    double rij, rji, rref;
    if (h.is_line) {
        // Vij = cB phi, Vji = g Vij, Uji = (Aji / Bji) Vji (rh_method.py:279-281); wla = wlambda wphi / hc (:451)
        const double w4 = (4.0 * M_PI) * p.wphi[(col * p.Nlines + h.line_idx) * Ns + k];
        const double2* __restrict__ pp = p.PP + (cb * Ns + k) * p.SNl + h.phi_off;
        double sp = 0.0, sf = 0.0;
        for (int lt = 0; lt < h.Nlam; ++lt) {
            if (!act[lt]) continue;
            const double w = w4 * wl[lt];
            const double2 v = pp[lt];
            sp += w * v.x;
            sf += w * v.y;
        }
        const double u = h.AB * (h.gij * h.cB) * sf;
        rij = h.cB * sp;
        rref = u + rij;
        rji = u + (h.gij * h.cB) * sp;
    } else {
        // Vij = alpha, Vji = g_ij alpha, Uji = (2hc / lambda^3) Vji, g_ij = nStar_i / nStar_j exp(-hc / k lambda T) (:284-286, :453-455)
        const double* __restrict__ al = p.alpha + h.wl_off;
        const double nsr = p.nsr[(col * p.Ncont + p.trans_row[t]) * Ns + k];
        const double* __restrict__ jp = p.Jp + (cb * Ns + k) * p.Nspect + h.Nblue;
        const double* __restrict__ Ecol = p.E_T + col * p.til_col;
        double sij = 0.0, sji = 0.0, sref = 0.0;
        for (int lt = 0; lt < h.Nlam; ++lt) {
            if (!act[lt]) continue;
            const int la = h.Nblue + lt;
            const double E = Ecol[((size_t)p.la_tile[2 * la] * Ns + k) * p.L + p.la_tile[2 * la + 1]];
            const double w = (4.0 * M_PI) * wl[lt], a = al[lt], Jv = jp[lt];
            const double vji = (nsr * E) * a, uji = p.u_la[la] * vji;
            sij += w * (a * Jv);
            sref += w * (uji * p.wsum + a * Jv);
            sji += w * (uji * p.wsum + vji * Jv);
        }
        rij = sij;
        rref = sref;
        rji = sji;
    }
    const size_t o = (cb * p.Ntrans + t) * Ns + k;
    p.Rij[o] = rij;
    p.Rji[o] = rji;
    p.Rji_ref[o] = rref;
}

template <int NM>
void launch_pass(const RatesParams& p, bool par, dim3 grid, hipStream_t st)
{
    if (par) hipLaunchKernelGGL((k_rates_pass<NM, true>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((k_rates_pass<NM, false>), grid, dim3(64), 0, st, p);
}

size_t work_doubles_per_column(const lsx_ctx* c) { return (size_t)c->Nspace * ((size_t)c->Nspect + 2 * (size_t)c->SNl); }

} // namespace

extern "C" int lsx_hip_radiative_rates_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_RATES_WORK, "lsx_hip_radiative_rates_work_cap", nbytes);
}

extern "C" int lsx_hip_radiative_rates(lsx_ctx* c, int32_t col0, int32_t ncol, double* Rij, double* Rji, double* Rji_ref, size_t nbytes_each)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!c) return fail(LSX_EINVAL, "lsx_hip_radiative_rates: null context");
    if (!Rij && !Rji && !Rji_ref) return fail(LSX_EINVAL, "lsx_hip_radiative_rates: all three outputs are NULL");
    int rc = final_check_depths(c, "lsx_hip_radiative_rates");
    if (!rc) rc = final_check_range(c, "lsx_hip_radiative_rates", col0, ncol);
    if (rc) return rc;
    const size_t per = (size_t)c->Ntrans * c->Nspace;
    if (nbytes_each != (size_t)ncol * per * 8) return fail(LSX_EINVAL, "lsx_hip_radiative_rates: nbytes_each does not match [ncol][Ntrans][Nspace]");
    if ((rc = final_check_columns(c, "lsx_hip_radiative_rates", col0, ncol, FINAL_OWN_RAYS))) return rc;
    if (c->Ntrans == 0) return LSX_OK;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = final_tables(c, "lsx_hip_radiative_rates"))) return rc;

    // columns per pass: the work arrays stay under the cap (one column's need if that alone is more)
    // (no limit: the pass's grid has the columns in its y like the other passes', whose 65535 this entry has never honoured)
    GrowBuf& work = c->buf[BUF_RATES_WORK];
    const size_t wcol = work_doubles_per_column(c);
    const size_t chunk = pass_columns(ncol, work.cap, kWorkCapDefault, wcol, kNoColumnLimit);
    if ((rc = work.reserve(c, (chunk * wcol + 2) * 8))) return rc;       // (+ 2: the pairs start on a 16-byte boundary)
    if ((rc = ensure_stage(c, 3 * chunk * per))) return rc;      // the three results of a chunk leave through the staging buffer

    RatesParams p{};
    final_fill(p, c);
    p.SNl = c->SNl; p.Ntrans = c->Ntrans; p.Nlines = c->Nlines;
    p.zmu = c->d_zmu; p.wmuh = c->d_wmuh; p.wl = c->d_wl; p.alpha = c->d_alpha;
    p.trans = c->d_trans; p.trans_row = c->d_final_row; p.active = c->d_active;
    p.wphi = c->d_wphi;
    p.wsum = 0.0;
    for (int dir = 0; dir < 2; ++dir)
        for (int m = 0; m < c->Nrays; ++m) p.wsum += c->wmuh[m];
    const bool par = c->solver == LSX_SOLVER_PARABOLIC;
    const int group = 5;                       // rays a lane carries at a time (registers: DESIGN.md 4.11)

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(col0 + b0);
        p.ncols = (int32_t)nb;
        p.Jp = work.as<double>();
        p.PP = reinterpret_cast<double2*>(p.Jp + ((nb * (size_t)c->Nspace * c->Nspect + 1) & ~(size_t)1));
        p.Rij = c->d_stage; p.Rji = c->d_stage + nb * per; p.Rji_ref = c->d_stage + 2 * nb * per;
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
        const size_t nthreads = nb * per;
        hipLaunchKernelGGL(k_rates_reduce, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, c->stream, p);
        HIPCHK(hipGetLastError());
        if (Rij) HIPCHK(hipMemcpyAsync(Rij + b0 * per, p.Rij, nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        if (Rji) HIPCHK(hipMemcpyAsync(Rji + b0 * per, p.Rji, nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        if (Rji_ref) HIPCHK(hipMemcpyAsync(Rji_ref + b0 * per, p.Rji_ref, nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));       // the work arrays and the staging buffer are re-used by the next chunk
    }
    return LSX_OK;
}
