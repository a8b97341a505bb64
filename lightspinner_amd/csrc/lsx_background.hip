// lsx_background.hip -- the background of a column on the device (include/lsx_hip_background.h): the Wittmann equation of state
// and the ATLAS-style continuous opacity of the reference's Background(atmos, spect) (background.py:15-53, witt.py).  gfx950.
//   k_eos                 one thread per (column, depth): pgas, pe, the 17 partials, the count of pe_pg evaluations.  The waves
//                         diverge on the iteration counts; that is accepted (about a hundred passes per point, once per column).
//   k_bg_wave             one thread per wavelength: everything that depends on the wavelength alone (OpWave), so that the
//                         opacity kernel reads it through wave-uniform (scalar) loads and its edge branches are wave-uniform
//   k_background_opacity  one lane per flattened (column, depth) pair, a chunk of wavelengths per blockIdx.y: the temperature-
//                         and partial-only terms once per lane in registers, then chi and eta to [col][la][k]
//   k_depth_scales        the depth-scale conversion behind the two (include/lsx_hip_scales.h): one lane per column, the recurrence
//                         of atmosphere.py:93-141 along depth with the running values in registers, the [col][k] arrays moved
//                         through LDS in chunks of SC_KC depths so that global memory is touched in contiguous runs
// The formulas are lsx_background_dev.h and lsx_scales_dev.h; this unit is built with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/lsx_hip.h"
#include "../../include/lsx_hip_background.h"
#include "../../include/lsx_hip_scales.h"
#include "lsx_background_prep.h"
#include "lsx_ctx.h"
#include "lsx_scales_dev.h"
#include "lsx_scales_prep.h"

using namespace lsxd;
using namespace lsxbg;

namespace {

__global__ __launch_bounds__(64) void k_eos(EosParams P, long npts, const double* __restrict__ T, const double* __restrict__ nH,
                                            double* __restrict__ pgas, double* __restrict__ pe, double* __restrict__ partials,
                                            int32_t* __restrict__ status)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= npts) return;
    double pg, pel;
    status[i] = eos_solve(P, T[i], nH[i], &pg, &pel, partials + i, (size_t)npts);      // partials: [17][npts]
    pgas[i] = pg;
    pe[i] = pel;
}

__global__ void k_bg_wave(const double* __restrict__ wavelength_nm, int nla, OpWave* __restrict__ W)
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < nla) make_wave(wavelength_nm[l] * 10, &W[l]);
}

// points [p0, p0 + np) of the call (np = nb * Ns: whole columns) -> chi, eta [nb][nla][Ns]
__global__ __launch_bounds__(64) void k_background_opacity(long p0, long np, long npts, int Ns, int nla, int la_chunk,
                                                           const double* __restrict__ T, const double* __restrict__ pgas,
                                                           const double* __restrict__ pe, const double* __restrict__ partials,
                                                           const double* __restrict__ wavelength_nm, const OpWave* __restrict__ W,
                                                           double* __restrict__ chi, double* __restrict__ eta)
{
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= np) return;
    const long col = i / Ns;
    const int k = (int)(i - col * Ns);
    const long g = p0 + i;
    const double t = T[g];
    OpLane L;
    make_lane(t, pgas[g], pe[g], partials + g, (size_t)npts, &L);
    const int la0 = blockIdx.y * la_chunk, la1 = min(nla, la0 + la_chunk);
    for (int la = la0; la < la1; ++la) {
        const double x = cop_point(L, W[la]) / 1.0E-02;
        const size_t o = ((size_t)col * nla + la) * Ns + k;
        chi[o] = x;
        eta[o] = planck_nm(t, wavelength_nm[la]) * x;
    }
}

// sca = ne sigma_T: [nb][Ns], or broadcast over the wavelengths [nb][nla][Ns]
__global__ void k_bg_sca(const double* __restrict__ ne, long np, int Ns, int nla, double sigma, double* __restrict__ sca)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const double v = ne[i] * sigma;
    if (nla <= 0) { sca[i] = v; return; }
    const long col = i / Ns;
    const int k = (int)(i - col * Ns);
    for (int la = 0; la < nla; ++la) sca[((size_t)col * nla + la) * Ns + k] = v;
}

// Depth chunk of k_depth_scales' staging, and the padded row of a column in LDS (an odd count of 8-byte words: the 64 lanes, each
// on its own row at the same depth, fall on different banks).  Three tiles of 64 x SC_ROW doubles: 25.5 KiB per workgroup.
constexpr int SC_KC = 16, SC_ROW = SC_KC + 1;

// columns [64 blockIdx.x, +64) of the call; chi: chi_c [ncol][Ns] from k_background_opacity at 500 nm.  height, cmass, tau may
// be null.  The geometric scale's height is its input: it is not written.
template <int SCALE>
__global__ __launch_bounds__(64) void k_depth_scales(int ncol, int Ns, double amu_wph, double wph, double gravity,
                                                     const double* __restrict__ ds, const double* __restrict__ T,
                                                     const double* __restrict__ nH, const double* __restrict__ ne,
                                                     const double* __restrict__ chi, double* __restrict__ height,
                                                     double* __restrict__ cmass, double* __restrict__ tau)
{
    __shared__ double s_a[64 * SC_ROW], s_b[64 * SC_ROW], s_c[64 * SC_ROW];      // in: depth scale, nHTot, chi_c; out: height, cmass, tau
    __shared__ double s_h1[64];
    const int lane = threadIdx.x;
    const long c0 = (long)blockIdx.x * 64;
    const int nc = (int)min((long)64, (long)ncol - c0);
    const size_t base = (size_t)c0 * Ns;
    lsxsc::Run R{};
    for (int k0 = 0; k0 < Ns; k0 += SC_KC) {
        const int kc = min(SC_KC, Ns - k0);
        for (int i = lane; i < 64 * SC_KC; i += 64) {          // 16 consecutive lanes read 16 consecutive depths of a column
            const int col = i / SC_KC, kk = i % SC_KC;
            if (col < nc && kk < kc) {
                const size_t g = base + (size_t)col * Ns + k0 + kk;
                s_a[col * SC_ROW + kk] = ds[g];
                s_b[col * SC_ROW + kk] = nH[g];
                s_c[col * SC_ROW + kk] = chi[g];
            }
        }
        __syncthreads();
        if (lane < nc) {
            double* a = s_a + lane * SC_ROW;
            double* b = s_b + lane * SC_ROW;
            double* x = s_c + lane * SC_ROW;
            for (int kk = 0; kk < kc; ++kk) {
                const double rho = lsxsc::rho_si(amu_wph, b[kk]);
                if (k0 + kk == 0) {
                    const size_t g0 = base + (size_t)lane * Ns;
                    lsxsc::start<SCALE>(R, a[0], a[1], rho, x[0], SCALE == lsxsc::GEOMETRIC ? T[g0] : 0.0, b[0],
                                        SCALE == lsxsc::GEOMETRIC ? ne[g0] : 0.0, wph, gravity);
                } else {
                    lsxsc::step<SCALE>(R, a[kk], rho, x[kk]);
                }
                a[kk] = R.height;
                b[kk] = R.cmass;
                x[kk] = R.tau;
            }
        }
        __syncthreads();
        for (int i = lane; i < 64 * SC_KC; i += 64) {
            const int col = i / SC_KC, kk = i % SC_KC;
            if (col < nc && kk < kc) {
                const size_t g = base + (size_t)col * Ns + k0 + kk;
                if (SCALE != lsxsc::GEOMETRIC && height) height[g] = s_a[col * SC_ROW + kk];
                if (cmass) cmass[g] = s_b[col * SC_ROW + kk];
                if (tau) tau[g] = s_c[col * SC_ROW + kk];
            }
        }
        __syncthreads();
    }
    if (SCALE == lsxsc::GEOMETRIC || !height) return;
    // second pass: height -= hTau1 (:105, :137), the workgroup's columns as one contiguous run
    s_h1[lane] = lane < nc ? lsxsc::tau1_last(R.t1, R.height) : 0.0;
    __syncthreads();
    const long n = (long)nc * Ns;
    for (long i = lane; i < n; i += 64) height[base + i] -= s_h1[i / Ns];
}

struct DevBuf {      // device memory of one call, freed when the call returns
    std::vector<void*> ptrs;
    ~DevBuf() { for (void* p : ptrs) (void)hipFree(p); }
    template <typename T>
    int get(T** p, size_t count)
    {
        int rc = dmalloc(p, count);
        if (!rc) ptrs.push_back(*p);
        return rc;
    }
    template <typename T>
    int put(T** p, const T* src, size_t count, hipStream_t st)
    {
        int rc = get(p, count);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(*p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        return LSX_OK;
    }
};

struct EosOnDevice {
    HostTables H;
    EosParams P{};
    double *T = nullptr, *nH = nullptr, *pgas = nullptr, *pe = nullptr, *partials = nullptr;
    int32_t* status = nullptr;
    std::vector<int32_t> h_status;
};

// checks + uploads + k_eos for npts = ncol * Ns points; on return the status is on the host (LSX_ENOCONV named, outputs valid)
int run_eos(lsx_ctx* c, const char* who, const lsx_eos_tables* tab, long ncol, const double* temperature, const double* nHTot,
            DevBuf& B, EosOnDevice& E)
{
    if (!c) return fail(LSX_EINVAL, "%s: null context", who);
    const std::string bad = prepare_tables(tab, &E.H);
    if (!bad.empty()) return fail(LSX_EINVAL, "%s: %s", who, bad.c_str());
    if (ncol < 1 || !temperature || !nHTot) return fail(LSX_EINVAL, "%s: ncol < 1 or a null input array", who);
    const int Ns = c->Nspace;
    const size_t npts = (size_t)ncol * Ns;
    long q;
    if ((q = first_bad_positive(temperature, npts)) >= 0) return fail(LSX_EINVAL, "%s: temperature of column %ld, depth %ld is not finite and positive", who, q / Ns, q % Ns);
    if ((q = first_bad_positive(nHTot, npts)) >= 0) return fail(LSX_EINVAL, "%s: nHTot of column %ld, depth %ld is not finite and positive", who, q / Ns, q % Ns);
    HIPCHK(hipSetDevice(c->device));
    int rc;
#define TRY(x) do { rc = (x); if (rc) return rc; } while (0)
    E.P = E.H.P;
    double *d_tpf, *d_pf, *d_eion, *d_abund;
    int32_t* d_nstage;
    TRY(B.put(&d_tpf, tab->tpf, (size_t)tab->npf, c->stream));
    TRY(B.put(&d_pf, tab->pf, (size_t)tab->nelem * 6 * tab->npf, c->stream));
    TRY(B.put(&d_eion, tab->eion, (size_t)tab->nelem * 6, c->stream));
    TRY(B.put(&d_nstage, tab->nstage, (size_t)tab->nelem, c->stream));
    TRY(B.put(&d_abund, (const double*)E.H.abund.data(), (size_t)99, c->stream));
    E.P.tpf = d_tpf; E.P.pf = d_pf; E.P.eion = d_eion; E.P.nstage = d_nstage; E.P.abund = d_abund;
    TRY(B.put(&E.T, temperature, npts, c->stream));
    TRY(B.put(&E.nH, nHTot, npts, c->stream));
    TRY(B.get(&E.pgas, npts));
    TRY(B.get(&E.pe, npts));
    TRY(B.get(&E.partials, npts * NPART));
    TRY(B.get(&E.status, npts));
#undef TRY
    hipLaunchKernelGGL(k_eos, dim3((unsigned)((npts + 63) / 64)), dim3(64), 0, c->stream, E.P, (long)npts, E.T, E.nH, E.pgas, E.pe,
                       E.partials, E.status);
    HIPCHK(hipGetLastError());
    E.h_status.resize(npts);
    HIPCHK(hipMemcpyAsync(E.h_status.data(), E.status, npts * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < npts; ++i)
        if (E.h_status[i] < 0)
            return fail(LSX_ENOCONV, "%s: the equation of state of column %zu, depth %zu ended at an iteration cap after %d pe_pg evaluations",
                        who, i / Ns, i % Ns, -E.h_status[i]);
    return LSX_OK;
}

} // namespace

extern "C" int lsx_hip_eos(lsx_ctx* c, const lsx_eos_tables* tab, int32_t ncol, const double* temperature, const double* nHTot,
                           double* pgas, double* pe, double* partials, int32_t* status)
{
    DevBuf B;
    EosOnDevice E;
    const int rc = run_eos(c, "lsx_hip_eos", tab, ncol, temperature, nHTot, B, E);
    if (rc != LSX_OK && rc != LSX_ENOCONV) return rc;
    const std::string msg = g_err;
    const int Ns = c->Nspace;
    const size_t npts = (size_t)ncol * Ns;
    if (pgas) HIPCHK(hipMemcpy(pgas, E.pgas, npts * 8, hipMemcpyDeviceToHost));
    if (pe) HIPCHK(hipMemcpy(pe, E.pe, npts * 8, hipMemcpyDeviceToHost));
    if (partials) {       // device [17][col][k] -> [col][17][k]
        std::vector<double> h(npts * NPART);
        HIPCHK(hipMemcpy(h.data(), E.partials, npts * NPART * 8, hipMemcpyDeviceToHost));
        for (size_t col = 0; col < (size_t)ncol; ++col)
            for (int q = 0; q < NPART; ++q)
                std::copy(h.begin() + q * npts + col * Ns, h.begin() + q * npts + (col + 1) * Ns, partials + (col * NPART + q) * Ns);
    }
    if (status) std::copy(E.h_status.begin(), E.h_status.end(), status);
    if (rc) g_err = msg;
    return rc;
}

extern "C" int lsx_hip_background(lsx_ctx* c, const lsx_eos_tables* tab, int32_t col0, int32_t ncol, const double* temperature,
                                  const double* nHTot, const double* ne, int32_t nla, const double* wavelength, double* chi, double* eta,
                                  double* sca, int32_t install)
{
    static const char* who = "lsx_hip_background";
    if (!c) return fail(LSX_EINVAL, "%s: null context", who);
    if (install != 0 && install != 1) return fail(LSX_EINVAL, "%s: install must be 0 or 1", who);
    if (install && wavelength) return fail(LSX_EINVAL, "%s: install = 1 needs the context's own grid (wavelength == NULL)", who);
    if (ncol < 1) return fail(LSX_EINVAL, "%s: ncol < 1", who);
    if (install && (col0 < 0 || (long)col0 + ncol > c->ncol)) return fail(LSX_EINVAL, "%s: columns [%d, %d) outside the context's %d", who, col0, col0 + ncol, c->ncol);
    if (wavelength) {
        if (nla < 1) return fail(LSX_EINVAL, "%s: nla < 1", who);
        for (int l = 0; l < nla; ++l)
            if (!std::isfinite(wavelength[l]) || !(wavelength[l] > 0.0) || (l && !(wavelength[l] > wavelength[l - 1])))
                return fail(LSX_EINVAL, "%s: wavelength[%d] is not finite, positive and above its predecessor", who, l);
    } else {
        nla = c->Nspect;
    }
    if (install)
        for (int q = 0; q < ncol; ++q)
            if (!c->cols_set[(size_t)col0 + q]) return fail(LSX_EINVAL, "%s: install into column %d, which lsx_set_columns has not set", who, col0 + q);
    if (!temperature || !nHTot || !ne) return fail(LSX_EINVAL, "%s: a null input array", who);
    const int Ns = c->Nspace;
    const size_t npts = (size_t)ncol * Ns;
    {
        const double* arr[3] = {temperature, nHTot, ne};
        const char* name[3] = {"temperature", "nHTot", "ne"};
        for (int a = 0; a < 3; ++a) {
            const long q = first_bad_positive(arr[a], npts);
            if (q >= 0) return fail(LSX_EINVAL, "%s: %s of column %ld, depth %ld is not finite and positive", who, name[a], q / Ns, q % Ns);
        }
    }
    DevBuf B;
    EosOnDevice E;
    int rc = run_eos(c, who, tab, ncol, temperature, nHTot, B, E);
    if (rc) return rc;          // LSX_ENOCONV: nothing is installed
#define TRY(x) do { rc = (x); if (rc) return rc; } while (0)
    double *d_ne, *d_wl = c->d_wavelength;
    OpWave* d_wave;
    TRY(B.put(&d_ne, ne, npts, c->stream));
    if (wavelength) TRY(B.put(&d_wl, wavelength, (size_t)nla, c->stream));
    TRY(B.get(&d_wave, (size_t)nla));
    hipLaunchKernelGGL(k_bg_wave, dim3((unsigned)((nla + 63) / 64)), dim3(64), 0, c->stream, d_wl, (int)nla, d_wave);
    HIPCHK(hipGetLastError());

    // columns in sub-chunks under lsx_set_columns' staging limit (chi and eta side by side, sigma behind them where it is per wavelength)
    const bool sca_l = install && c->sca_per_lambda;
    const size_t per_col = (size_t)nla * Ns;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>((size_t)ncol, ((size_t)32 << 20) / ((sca_l ? 3 : 2) * per_col)));
    TRY(ensure_stage(c, (sca_l ? 3 : 2) * chunk * per_col + chunk * Ns));
    const double sigma = thomson_sigma();
    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        const long np = (long)(nb * Ns);
        double *s_chi = c->d_stage, *s_eta = s_chi + chunk * per_col, *s_sca = s_eta + chunk * per_col;
        const int la_chunk = np >= 65536 ? 64 : 16;
        hipLaunchKernelGGL(k_background_opacity, dim3((unsigned)((np + 63) / 64), (unsigned)((nla + la_chunk - 1) / la_chunk)), dim3(64), 0,
                           c->stream, (long)(b0 * Ns), np, (long)npts, Ns, (int)nla, la_chunk, E.T, E.pgas, E.pe, E.partials, d_wl, d_wave, s_chi,
                           s_eta);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_bg_sca, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, d_ne + b0 * Ns, np, Ns, sca_l ? (int)nla : 0,
                           sigma, s_sca);
        HIPCHK(hipGetLastError());
        if (install) TRY(background_from_device(c, (size_t)col0 + b0, nb, s_chi, s_eta, s_sca));
        if (chi) HIPCHK(hipMemcpyAsync(chi + b0 * per_col, s_chi, nb * per_col * 8, hipMemcpyDeviceToHost, c->stream));
        if (eta) HIPCHK(hipMemcpyAsync(eta + b0 * per_col, s_eta, nb * per_col * 8, hipMemcpyDeviceToHost, c->stream));
        if (sca) {
            if (!sca_l) {
                HIPCHK(hipMemcpyAsync(sca + b0 * Ns, s_sca, nb * Ns * 8, hipMemcpyDeviceToHost, c->stream));
            } else {       // (the per-depth value: row 0 of every column's broadcast)
                for (size_t q = 0; q < nb; ++q)
                    HIPCHK(hipMemcpyAsync(sca + (b0 + q) * Ns, s_sca + q * per_col, (size_t)Ns * 8, hipMemcpyDeviceToHost, c->stream));
            }
        }
        HIPCHK(hipStreamSynchronize(c->stream));      // the staging buffer is re-used by the next sub-chunk
    }
#undef TRY
    return LSX_OK;
}

extern "C" int lsx_hip_convert_scales(lsx_ctx* c, const lsx_eos_tables* tab, int32_t scale, int32_t col0, int32_t ncol,
                                      const double* depth_scale, const double* temperature, const double* nHTot, const double* ne,
                                      double gravity, double* height, double* cmass, double* tau_ref, double* chi_ref, int32_t install)
{
    static const char* who = "lsx_hip_convert_scales";
    if (!c) return fail(LSX_EINVAL, "%s: null context", who);
    if (install != 0 && install != 1) return fail(LSX_EINVAL, "%s: install must be 0 or 1", who);
    const int Ns = c->Nspace;
    {
        const std::string bad = lsxsc::check_arrays(scale, ncol, Ns, depth_scale, temperature, nHTot, ne, gravity);
        if (!bad.empty()) return fail(LSX_EINVAL, "%s: %s", who, bad.c_str());
    }
    if (install) {
        if (col0 < 0 || (long)col0 + ncol > c->ncol) return fail(LSX_EINVAL, "%s: columns [%d, %d) outside the context's %d", who, col0, col0 + ncol, c->ncol);
        for (int q = 0; q < ncol; ++q)
            if (!c->cols_set[(size_t)col0 + q]) return fail(LSX_EINVAL, "%s: install into column %d, which lsx_set_columns has not set", who, col0 + q);
    }
    const bool geo = scale == LSX_SCALE_GEOMETRIC;
    const size_t npts = (size_t)ncol * Ns;
    DevBuf B;
    EosOnDevice E;
    int rc = run_eos(c, who, tab, ncol, temperature, nHTot, B, E);
    if (rc) return rc;          // LSX_ENOCONV: nothing is installed, nothing is written
#define TRY(x) do { rc = (x); if (rc) return rc; } while (0)
    // chi_c: the opacity path with one wavelength, 500.0 nm (witt.contOpacity(..., [5000.0]), atmosphere.py:91)
    const double w500 = 500.0;
    double *d_wl, *d_chi, *d_eta, *d_ds, *d_ne = nullptr, *d_h = nullptr, *d_cm = nullptr, *d_tau = nullptr;
    OpWave* d_wave;
    TRY(B.put(&d_wl, &w500, (size_t)1, c->stream));
    TRY(B.get(&d_wave, (size_t)1));
    TRY(B.get(&d_chi, npts));
    TRY(B.get(&d_eta, npts));
    TRY(B.put(&d_ds, depth_scale, npts, c->stream));
    if (geo) TRY(B.put(&d_ne, ne, npts, c->stream));
    if (!geo && (height || install)) TRY(B.get(&d_h, npts));
    if (cmass) TRY(B.get(&d_cm, npts));
    if (tau_ref) TRY(B.get(&d_tau, npts));
    hipLaunchKernelGGL(k_bg_wave, dim3(1), dim3(64), 0, c->stream, d_wl, 1, d_wave);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_background_opacity, dim3((unsigned)((npts + 63) / 64), 1), dim3(64), 0, c->stream, 0L, (long)npts, (long)npts, Ns, 1, 16,
                       E.T, E.pgas, E.pe, E.partials, d_wl, d_wave, d_chi, d_eta);
    HIPCHK(hipGetLastError());
    if (d_h || d_cm || d_tau) {
        const dim3 grid((unsigned)((ncol + 63) / 64));
        const double wph = tab->weight_per_H;
#define SC_LAUNCH(S) hipLaunchKernelGGL(k_depth_scales<S>, grid, dim3(64), 0, c->stream, (int)ncol, Ns, E.P.rho_unit, wph, gravity, d_ds, E.T, \
                                        E.nH, d_ne, d_chi, d_h, d_cm, d_tau)
        if (scale == LSX_SCALE_COLUMN_MASS) SC_LAUNCH(lsxsc::COLUMN_MASS);
        else if (geo) SC_LAUNCH(lsxsc::GEOMETRIC);
        else SC_LAUNCH(lsxsc::TAU500);
#undef SC_LAUNCH
        HIPCHK(hipGetLastError());
    }
    if (install) {      // what lsx_set_columns invalidates for a new height: the operand table of the ray-serial sweeps, a discardable formal solution
        c->optab_fresh = false;
        c->spec_valid = false;
        HIPCHK(hipMemcpyAsync(c->d_height + (size_t)col0 * Ns, geo ? d_ds : d_h, npts * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    if (height) {
        if (geo) std::copy(depth_scale, depth_scale + npts, height);       // the input, bit for bit
        else HIPCHK(hipMemcpyAsync(height, d_h, npts * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (cmass) HIPCHK(hipMemcpyAsync(cmass, d_cm, npts * 8, hipMemcpyDeviceToHost, c->stream));
    if (tau_ref) HIPCHK(hipMemcpyAsync(tau_ref, d_tau, npts * 8, hipMemcpyDeviceToHost, c->stream));
    if (chi_ref) HIPCHK(hipMemcpyAsync(chi_ref, d_chi, npts * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
#undef TRY
    return LSX_OK;
}
