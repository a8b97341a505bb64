// lsx_stokes.hip -- final-pass formal solution of the polarised transfer equation: the emergent Stokes vector of a converged context in
// a magnetic field at arbitrary viewing angles (include/lsx_hip_stokes.h, lsx_hip_stokes_rays).  Read-only on the context; gfx950 only.
//
// The "field-free" method: populations and J are the unpolarised iteration's; the lines that were given a Zeeman pattern get split
// profiles and a propagation matrix here (formulas: lsx_stokes_dev.h), everything else enters eta_I and eps_I as in k_emergent_rays
// (lsx_rays.hip; rh_method.py:599-632, 231-239), whose column set-up (lsx_final_dev.h) this walk uses.
//
// Mapping (that of k_emergent_rays): one wavefront = 64 consecutive wavelengths of the call's window of one column, a lane owns one
// wavelength and carries a compile-time chunk of NM angles in registers: per angle the Stokes vector and K', S' of the depth behind
// (15 doubles), the depth's eta, rho, eps (11) and the field's geometry (4).  LDS: the exponential's table, the Voigt function's and
// the pattern table of the call (4 doubles a component), loaded once per wavefront.  The field of a depth and the broadening of a
// line are uniform over the wavefront.  DELO-linear, the 4 x 4 solve unrolled in registers; no depth limit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"
#include "lsx_stokes_dev.h"
#include "lsx_stokes_prep.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)256 << 20;      // bytes (include/lsx_hip_stokes.h)

struct StokesParams {
    int32_t Ns, Nspect, NLtot, Natoms, NlinesA, Ncont, L, Nrays;
    int32_t col0, nmu, mu0;     // first column of the launch; angles of the call; first angle of this launch's chunk
    int32_t la0, nla;           // the call's window of the merged wavelength grid
    int32_t phi_compact, sca_per_lambda, phi_G;
    int32_t ntab;               // doubles of the pattern table
    int64_t til_col, phi_col, sca_col, fstride;
    const double *wavelength, *u_la, *exp2_tab, *voigt_W, *mu;
    const int32_t* la_ptr;      // [Nspect + 1] into ents
    const FinalEnt* ents;
    const int32_t* la_tile;     // [Nspect][2]: tile, place in the tile
    const double *height, *temperature, *n, *nsr, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    const double *aDamp, *vBroad, *vlos;
    const uint8_t* prof_kind;   // per column: 1 = profiles built by the library, 2 = with a line-of-sight velocity (ray dependent)
    const int32_t* bnd;         // the radiation boundary (lsx_dev.h, the boundary store), or null
    const int32_t* pat_line;    // [Nlines][2]: components of the line's pattern (0: unpolarised), the first one's place in pat_tab
    const double* pat_tab;      // [ntab]: per component (shift, weight of phi_-1, of phi_0, of phi_+1)
    const double* field;        // B, gammaB, chiB (and, in a call with a velocity, vlos): [3 or 4][launch columns][Ns], fstride apart
    double* out;                // [launch column][4][nla][nmu]
};

struct W2Dev {                  // the linear rule's weights as the other final passes form them (lsx_dev.h)
    const lds_f64* etab;
    __device__ __forceinline__ void operator()(double dtau, double& w0, double& w1) const { w2(dtau, w0, w1, etab); }
};

// VEL: the call has a velocity (include/lsx_hip_stokes_velocity.h) -- the fourth array of p.field in the place of the context's vlos,
// and every line formed from the kept broadening arrays: the context's profile store is not read.  VEL = false is the kernel as it was.
template <int NM, bool VEL>
__global__ void __launch_bounds__(64) k_stokes_rays(const StokesParams p)
{
    extern __shared__ double smem[];                  // the exponential's table, the Voigt function's (56 doubles), the patterns
    for (int e = threadIdx.x; e < LSX_EXP_TAB; e += 64) smem[e] = p.exp2_tab[e];
    if (threadIdx.x < 56) smem[LSX_EXP_TAB + threadIdx.x] = p.voigt_W ? p.voigt_W[threadIdx.x] : 0.0;
    for (int e = threadIdx.x; e < p.ntab; e += 64) smem[LSX_EXP_TAB + 64 + e] = p.pat_tab[e];
    __syncthreads();
    const lds_f64* etab = (const lds_f64*)smem;
    const lds_f64* vtab = etab + LSX_EXP_TAB;
    const lds_f64* ptab = vtab + 64;

    const int Ns = p.Ns, L = p.L;
    const int q_raw = blockIdx.x * 64 + threadIdx.x;       // place in the window
    const bool valid = q_raw < p.nla;
    const int q = valid ? q_raw : p.nla - 1;               // every lane walks a wavelength (w2 is wave-wide); spare ones store nothing
    const int la = p.la0 + q;
    const size_t col = (size_t)p.col0 + blockIdx.y;
    // the lower boundary (include/lsx_hip_boundary.h): thermalised unless the column has been given ZERO (GIVEN is refused on the host)
    const bool lower_zero = p.bnd != nullptr && boundary_kind(p.bnd, col, LSX_BND_LOWER) == 0;
    const FinalColumn f = final_column(p, col, la);
    const FinalAngles fa = final_angles(p, col);
    // the kept broadening arrays of the column (every column of a call has them: checked on the host)
    const double* aD_c = p.aDamp + col * (size_t)p.NlinesA * Ns;
    const double* vB_c = p.vBroad + col * (size_t)p.Natoms * Ns;
    const double* fld = p.field + (size_t)blockIdx.y * Ns;
    const double* vL_c = VEL ? fld + 3 * p.fstride : p.vlos + col * Ns;
    const double wav = p.wavelength[la], u_la = p.u_la[la];
    const W2Dev wf{etab};

    double mu[NM], zmu[NM];
    lsxst::Ray ray[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        mu[m] = p.mu[p.mu0 + m];
        zmu[m] = 1.0 / mu[m];
        lsxst::ray_init(ray[m]);
    }
    double zk1 = 0.0;                  // height of the depth below the current one

    for (int k = Ns - 1; k >= 0; --k) {
        const int s = Ns - 1 - k;      // step along the up-going ray
        const double zk = f.z[k];
        const double Ev = f.Eb ? f.Eb[(size_t)k * L] : 0.0;
        const double c0 = f.bgchi[(size_t)k * L];
        const double h0 = f.bgeta[(size_t)k * L] + f.sca[(size_t)k * f.sstr] * f.Jd[(size_t)k * L];
        const double Bk = fld[k], gk = fld[p.fstride + k], xk = fld[2 * p.fstride + k];
        lsxst::Acc acc[NM];
        lsxst::Geo geo[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            lsxst::acc_init(acc[m], c0, h0);
            geo[m] = lsxst::geometry(gk, xk, mu[m]);
        }
        for (int e = f.e0; e < f.e1; ++e) {
            const FinalEnt& t = p.ents[e];
            const double ni = f.n_col[(size_t)t.li * Ns + k], nj = f.n_col[(size_t)t.lj * Ns + k];
            if (t.is_line) {
                const double nd = t.a * (ni - t.g * nj);          // n_i Vij - n_j Vji = nd phi, :279-280, :613
                const int nc = p.pat_line[2 * t.row];
                if (VEL || nc > 0 || fa.raydep) {
                    // a polarised line: split profiles from the kept broadening arrays (vlos is zero where none was given); a
                    // ray-dependent unpolarised one: the same profile function without a splitting (one evaluation), into eta_I and eps_I alone
                    const lds_f64* tab = ptab + lsxst::kCompDoubles * p.pat_line[2 * t.row + 1];
                    const double vb = vB_c[(size_t)t.atom * Ns + k], ad = aD_c[(size_t)t.row * Ns + k], vl = vL_c[k];
                    const double v = (wav - t.lambda0) * kCLight / (vb * t.lambda0);          // :234
                    const double rn = 1.0 / (sqrt(M_PI) * vb);
                    const double vZ = nc > 0 ? lsxst::kLarmor * (kNM_TO_M * t.lambda0) * Bk / vb : 0.0;
                    const double ne = nj * t.Uc;
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const lsxst::Prof pr = lsxst::line_profiles(nc, tab, ad, v + 1.0 * (mu[m] * vl / vb), vZ, vtab);   // up-going: :231, :238-239
                        if (nc > 0) lsxst::line_add(acc[m], nd, ne, pr, rn, geo[m]);
                        else lsxst::line_add_plain(acc[m], nd, ne, pr, rn);
                    }
                } else {
                    // ray-independent profile: the one the formal solution uses (compact: row k; else the up-going row of ray 0)
                    const size_t x = p.phi_compact ? (size_t)k : ((size_t)Ns + k) * p.Nrays;
                    const double pv = p.phi_T[phi_elem(col, p.phi_G, (size_t)p.phi_col, (size_t)t.phi_base, x, t.phi_len, t.phi_l)];
                    const double c1 = nd * pv, h1 = nj * (t.Uc * pv);
#pragma unroll
                    for (int m = 0; m < NM; ++m) { acc[m].eI += c1; acc[m].mI += h1; }
                }
            } else {
                const double pv = (f.nsr_col[(size_t)t.row * Ns + k] * Ev) * t.a;     // Vji = g_ij alpha, :284-285, :453-454
                const double c1 = ni * t.a - nj * pv, h1 = nj * (u_la * pv);        // :286, :613-614
#pragma unroll
                for (int m = 0; m < NM; ++m) { acc[m].eI += c1; acc[m].mI += h1; }
            }
        }
        // ---- the up-going ray's DELO step at this depth (k == 0: with the reference's end-point term in I); its start value belongs
        // to the depth below (I is still 0 there) ----
        const double adz = fabs(zk1 - zk);
        if (s == 0) {
#pragma unroll
            for (int m = 0; m < NM; ++m) lsxst::ray_set(ray[m], acc[m]);
        } else {
            if (s == 1 && !lower_zero) {
                const double Be = lsxst::planck(p.temperature[col * Ns + Ns - 1], wav), Bn = lsxst::planck(p.temperature[col * Ns + Ns - 2], wav);
#pragma unroll
                for (int m = 0; m < NM; ++m) ray[m].I = lsxst::thermal_start(Be, Bn, adz * zmu[m], ray[m].eI, acc[m].eI);
            }
#pragma unroll
            for (int m = 0; m < NM; ++m) lsxst::delo_step(ray[m], acc[m], adz * zmu[m], wf, k == 0);
        }
        zk1 = zk;
    }
    if (valid) {
        const size_t plane = (size_t)p.nla * p.nmu;
        double* o = p.out + (size_t)blockIdx.y * 4 * plane + (size_t)q * p.nmu + p.mu0;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            o[m] = ray[m].I;
            o[plane + m] = ray[m].Q;
            o[2 * plane + m] = ray[m].U;
            o[3 * plane + m] = ray[m].V;
        }
    }
}

template <int NM>
void launch_chunk(const StokesParams& p, bool vel, dim3 grid, size_t lds, hipStream_t st)
{
    if (vel) hipLaunchKernelGGL((k_stokes_rays<NM, true>), grid, dim3(64), lds, st, p);
    else hipLaunchKernelGGL((k_stokes_rays<NM, false>), grid, dim3(64), lds, st, p);
}

} // namespace

extern "C" int lsx_hip_stokes_rays_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_STOKES_WORK, "lsx_hip_stokes_rays_work_cap", nbytes);
}

// ---- what lsx_hip_stokes_rays shares with lsx_hip_response_stokes and the fit (declared in lsx_ctx.h) ----
int lsxd::stokes_check_call(const lsx_ctx* c, const char* who, const StokesCall& s)
{
    if (!c || !s.mu || !s.B || !s.gammaB || !s.chiB) return fail(LSX_EINVAL, "%s: null argument", who);
    if (c->Nlines && !s.ncomp) return fail(LSX_EINVAL, "%s: null ncomp (one count per line; zeros for no pattern)", who);
    int rc = final_check_angles(who, s.nmu, s.mu);
    if (!rc) rc = final_check_range(c, who, s.col0, s.ncol);
    if (!rc) rc = final_check_window(c, who, s.la0, s.nla);
    return rc;
}

int lsxd::stokes_check_state(const lsx_ctx* c, const char* who, const StokesCall& s)
{
    int rc;
    std::string msg;
    if ((rc = lsxst::check_field((size_t)s.ncol * c->Nspace, s.B, s.gammaB, s.chiB, msg))) return fail(rc, "%s: %s", who, msg.c_str());
    if (s.vlos && (rc = lsxst::check_velocity((size_t)s.ncol * c->Nspace, s.vlos, msg))) return fail(rc, "%s: %s", who, msg.c_str());
    if ((rc = lsxst::check_patterns(c->Nlines, s.ncomp, s.alpha, s.strength, s.shift, msg))) return fail(rc, "%s: %s", who, msg.c_str());
    if ((rc = final_check_depths(c, who))) return rc;
    if ((rc = final_check_columns(c, who, s.col0, s.ncol, FINAL_OTHER_ANGLE))) return rc;
    // split profiles are formed from the kept broadening arrays, whether the context's own profiles depend on the ray or not
    for (int q = s.col0; q < s.col0 + s.ncol && c->Nlines; ++q)
        if (c->prof_kind.empty() || !c->prof_kind[q])
            return fail(LSX_EUNSUPPORTED, "%s: the line profiles of column %d were handed over as arrays (lsx_set_columns): the library "
                                          "cannot know them at another angle.  Build them with lsx_set_line_profiles or "
                                          "lsx_set_atmosphere", who, q);
    return LSX_OK;
}

int lsxd::stokes_patterns(const lsx_ctx* c, const char* who, const StokesCall& s, std::vector<int32_t>& pat_line, std::vector<double>& pat_tab)
{
    std::vector<uint8_t> wanted(std::max(1, c->Nlines), 0);
    for (int t = 0; t < c->Ntrans; ++t) {
        if (!c->htrans[t].is_line) continue;
        const uint8_t* act = c->active.data() + (size_t)t * c->Nspect;
        for (int la = s.la0; la < s.la0 + s.nla; ++la)
            if (act[la]) { wanted[c->trans_row[t]] = 1; break; }
    }
    std::string msg;
    const int rc = lsxst::pack_patterns(c->Nlines, s.ncomp, s.alpha, s.strength, s.shift, wanted, pat_line, pat_tab, msg);
    return rc ? fail(rc, "%s: %s", who, msg.c_str()) : LSX_OK;
}

int lsxd::stokes_upload_field(lsx_ctx* c, const StokesCall& s, size_t b0, size_t nb, double* d_field)
{
    const size_t Ns = (size_t)c->Nspace;
    const double* const src[4] = {s.B, s.gammaB, s.chiB, s.vlos};
    for (int a = 0; a < s.nfield(); ++a)
        HIPCHK(hipMemcpyAsync(d_field + (size_t)a * nb * Ns, src[a] + b0 * Ns, nb * Ns * 8, hipMemcpyHostToDevice, c->stream));
    return LSX_OK;
}

// The body of lsx_hip_stokes_rays.  sink null: the entry itself -- every pass is copied to out.  An internal caller (lsx_fit.hip) hands a
// sink instead and out null: a pass's result stays in the pass's device array and the sink is called in the copy's place.
int lsxd::stokes_rays_run(lsx_ctx* c, const char* who, const StokesCall& s, double* out, size_t nbytes, PassSink* sink)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!out && !sink) return fail(LSX_EINVAL, "%s: null argument", who);
    int rc = stokes_check_call(c, who, s);
    if (rc) return rc;
    const int32_t nmu = s.nmu, ncol = s.ncol, nla = s.nla;
    const size_t plane = (size_t)nla * nmu, per = 4 * plane;
    if (!sink && nbytes != (size_t)ncol * per * 8) return fail(LSX_EINVAL, "%s: nbytes does not match [ncol][4][nla][nmu]", who);
    if ((rc = stokes_check_state(c, who, s))) return rc;
    const int Ns = c->Nspace;
    std::vector<int32_t> pat_line;
    std::vector<double> pat_tab;
    if ((rc = stokes_patterns(c, who, s, pat_line, pat_tab))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = final_tables(c, who))) return rc;

    // the tables of the call: [pat_line | pat_tab]
    const size_t line_bytes = (pat_line.size() * sizeof(int32_t) + 7) & ~(size_t)7;
    GrowBuf& tab = c->buf[BUF_STOKES_TAB];
    if ((rc = tab.reserve(c, line_bytes + std::max<size_t>(1, pat_tab.size()) * 8))) return rc;
    HIPCHK(hipMemcpyAsync(tab.p, pat_line.data(), pat_line.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (!pat_tab.empty())
        HIPCHK(hipMemcpyAsync(tab.p + line_bytes, pat_tab.data(), pat_tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                      // the host vectors may go out of scope on any return below

    // columns per pass: the field and the result of a pass stay under the cap (one column's need if that alone is more)
    GrowBuf& work = c->buf[BUF_STOKES_WORK];
    const size_t head = ((size_t)nmu + 1) & ~(size_t)1;
    const size_t nf = (size_t)s.nfield();
    const size_t wcol = per + nf * (size_t)Ns;
    const size_t chunk = pass_columns(ncol, work.cap, kWorkCapDefault, wcol, kGridYLimit);
    if ((rc = work.reserve(c, (head + chunk * wcol) * 8))) return rc;
    double* d_mu = work.as<double>();
    double* d_field = d_mu + head;
    double* d_out = d_field + chunk * nf * (size_t)Ns;
    HIPCHK(hipMemcpyAsync(d_mu, s.mu, (size_t)nmu * 8, hipMemcpyHostToDevice, c->stream));

    StokesParams p{};
    final_fill(p, c);
    final_fill_angles(p, c);
    p.nmu = nmu; p.la0 = s.la0; p.nla = nla; p.mu = d_mu;
    p.ntab = (int32_t)pat_tab.size();
    p.pat_line = tab.as<const int32_t>();
    p.pat_tab = (const double*)(tab.p + line_bytes);
    p.field = d_field;
    p.out = d_out;
    const size_t lds = ((size_t)LSX_EXP_TAB + 64 + pat_tab.size() + lsxst::kCompDoubles) * 8;

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(s.col0 + b0);
        p.fstride = (int64_t)(nb * Ns);
        if ((rc = stokes_upload_field(c, s, b0, nb, d_field))) return rc;
        const dim3 grid((unsigned)((nla + 63) / 64), (unsigned)nb);
        // angles in register chunks of NM.  The compiler's report decides the instances: NM = 1 is the only one
        // without a spilled vector register (NM = 2 spills 8, NM = 4 spills 20 into accumulator registers at one wave per SIMD), and
        // the profile function is evaluated per angle whatever NM is; what does not depend on the angle (populations, continua, the
        // tables) is redone per launch.  That the former outweighs the latter is supposed, not measured
        for (int m0 = 0; m0 < nmu; ++m0) {
            p.mu0 = m0;
            launch_chunk<1>(p, s.vlos != nullptr, grid, lds, c->stream);
        }
        HIPCHK(hipGetLastError());
        if (sink) {
            if ((rc = sink->pass(b0, nb, d_out))) return rc;
        } else {
            HIPCHK(hipMemcpyAsync(out + b0 * per, d_out, nb * per * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next pass
    }
    return LSX_OK;
}

extern "C" int lsx_hip_stokes_rays(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                   const double* B, const double* gammaB, const double* chiB,
                                   const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                   double* out, size_t nbytes)
{
    const StokesCall s{nmu, mu, col0, ncol, la0, nla, B, gammaB, chiB, ncomp, alpha, strength, shift};
    return stokes_rays_run(c, "lsx_hip_stokes_rays", s, out, nbytes, nullptr);
}

extern "C" int lsx_hip_velocity_stokes_rays(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                            const double* B, const double* gammaB, const double* chiB,
                                            const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                            double* out, size_t nbytes, const double* vlos)
{
    if (!vlos) return lsx_hip_stokes_rays(c, nmu, mu, col0, ncol, la0, nla, B, gammaB, chiB, ncomp, alpha, strength, shift, out, nbytes);
    const StokesCall s{nmu, mu, col0, ncol, la0, nla, B, gammaB, chiB, ncomp, alpha, strength, shift, vlos};
    return stokes_rays_run(c, "lsx_hip_velocity_stokes_rays", s, out, nbytes, nullptr);
}
