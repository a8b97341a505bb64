// lsx_stokes_response.hip -- response functions of the emergent Stokes vector to the field strength, inclination and azimuth at every
// depth (include/lsx_hip_stokes_response.h, lsx_hip_response_stokes).  Read-only on the context; gfx950 only.
//
// In the field-free method the response to the field at one depth is the change of one polarised formal solution.  The absorption
// matrix of a depth depends on the field at that depth only and the DELO-linear recursion is affine in the Stokes vector, so two
// stages do for all depths what 6 Nspace + 1 runs of k_stokes_rays (lsx_stokes.hip) would:
//   k_response_nodes   one wavefront = 64 wavelengths of the window of one column at ONE depth under ONE field variant (the call's
//                      field, or one parameter moved by +-a/2 at that depth): the depth's eta, rho, eps by the text of k_stokes_rays
//                      (final_column, line_profiles, line_add, line_add_plain, the LDS tables), stored as the depth's NODE (lsx_stokes_dev.h:
//                      the 11 doubles the solver needs of it) with the wavelength running fastest.  No ray state: depths and variants
//                      are the grid's z.
//                      The variants of gammaB and chiB repeat the profiles of the call's field (only `geometry` differs): that is NOT
//                      exploited.  A rolled loop over the variants of a depth that kept the profiles would have to keep them per line
//                      while several lines add into one Acc, i.e. carry five Accs (55 doubles) beside the profile function, whose
//                      kernel already stands at 242 vector registers with one; and sums free of the geometry would change the bits
//                      of the unperturbed node.  So every variant is a block of its own and forms its profiles.
//   k_response_walk    lane = wavelength, block z = angle; no profile function.  response_walk (lsx_stokes_dev.h): the walk up over
//                      the stored nodes keeps the ray's state at every depth; the walk down carries the 4 x 4 matrix T_m and redoes,
//                      per requested depth, parameter and sign, the steps that depth's node enters.
// With a velocity in the call (include/lsx_hip_stokes_velocity.h) vlos is a fourth parameter of exactly this
// structure: its variants move the velocity of one depth, leave the geometry and re-form the profiles, so there are up to nine blocks
// a depth; k_response_nodes<true> reads the call's velocity in the context's place and forms every line of the window itself.  The
// walk sees only more variants.
// The work arrays are padded to whole wavefronts of wavelengths, so that a spare lane (it walks the window's last wavelength: the
// exponential's table is read wave-wide) has a slot of its own: one writer per value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lsx_hip.h"
#include "lsx_final_host.h"
#include "lsx_stokes_dev.h"
#include "lsx_stokes_prep.h"
#include "lsx_stokes_response_nodes.h"

using namespace lsxd;

namespace {

constexpr size_t kWorkCapDefault = (size_t)256 << 20;      // bytes (include/lsx_hip_stokes_response.h)

struct W2Dev {                  // the linear rule's weights as the other final passes form them (lsx_dev.h)
    const lds_f64* etab;
    __device__ __forceinline__ void operator()(double dtau, double& w0, double& w1) const { w2(dtau, w0, w1, etab); }
};

// ---- stage 2: the walks of one ray ----
struct ZDev {
    const double* z;
    __device__ __forceinline__ double operator()(int k) const { return z[k]; }
};
struct NodesDev {
    const double* base;         // the lane's wavelength of [nvar][Ns][11][nlaP]
    size_t Ns, nlaP;
    __device__ __forceinline__ void operator()(lsxst::Acc& n, int var, int k) const
    {
        lsxst::node_load(n, base + ((size_t)var * Ns + k) * lsxst::kNodeDoubles * nlaP, nlaP);
    }
};
struct StateDev {
    double* base;               // the lane's wavelength of [Ns][5][nlaP]
    size_t nlaP;
    __device__ __forceinline__ void put(int k, const lsxst::Ray& r) const
    {
        double* s = base + (size_t)k * lsxst::kStateDoubles * nlaP;
        s[0] = r.I; s[nlaP] = r.Q; s[2 * nlaP] = r.U; s[3 * nlaP] = r.V; s[4 * nlaP] = r.dt;
    }
    __device__ __forceinline__ void get(int k, lsxst::Ray& r) const
    {
        const double* s = base + (size_t)k * lsxst::kStateDoubles * nlaP;
        r.I = s[0]; r.Q = s[nlaP]; r.U = s[2 * nlaP]; r.V = s[3 * nlaP]; r.dt = s[4 * nlaP];
    }
};
struct OutDev {
    double* rf;                 // the lane's (wavelength, angle) of [npar][4][nla][nk][nmu]; null for a spare lane
    size_t comp, nmu;           // nla nk nmu
    __device__ __forceinline__ void operator()(int i, int jk, const double (&o)[4]) const
    {
        if (!rf) return;
        double* d = rf + (size_t)i * 4 * comp + (size_t)jk * nmu;
        d[0] = o[0]; d[comp] = o[1]; d[2 * comp] = o[2]; d[3 * comp] = o[3];
    }
};

__global__ void __launch_bounds__(64) k_response_walk(const RespParams p)
{
    extern __shared__ double smem[];                  // the exponential's table
    for (int e = threadIdx.x; e < LSX_EXP_TAB; e += 64) smem[e] = p.exp2_tab[e];
    __syncthreads();
    const W2Dev wf{(const lds_f64*)smem};

    const int Ns = p.Ns;
    const int q_raw = blockIdx.x * 64 + threadIdx.x;
    const bool valid = q_raw < p.nla;
    const int q = valid ? q_raw : p.nla - 1;
    const int m = blockIdx.z;
    const size_t cl = blockIdx.y, col = (size_t)p.col0 + cl;
    const bool lower_zero = p.bnd != nullptr && boundary_kind(p.bnd, col, LSX_BND_LOWER) == 0;
    const double wav = p.wavelength[p.la0 + q];
    const double Be = lsxst::planck(p.temperature[col * Ns + Ns - 1], wav), Bn = lsxst::planck(p.temperature[col * Ns + Ns - 2], wav);
    const ZDev z{p.height + col * Ns};
    const NodesDev nodes{p.nodes + node_offset(p, cl, m, 0, 0) + q_raw, (size_t)Ns, (size_t)p.nlaP};
    const StateDev state{p.state + ((cl * p.nmu + m) * Ns) * (size_t)lsxst::kStateDoubles * p.nlaP + q_raw, (size_t)p.nlaP};
    const size_t comp = (size_t)p.nla * p.nk * p.nmu;
    const OutDev out{valid ? p.rf + cl * p.npar * 4 * comp + (size_t)q * p.nk * p.nmu + m : nullptr, comp, (size_t)p.nmu};
    double S[4];                                      // (the walk's own emergent vector is not handed out: see the entry)
    lsxst::response_walk(Ns, z, 1.0 / p.mu[m], !lower_zero, Be, Bn, wf, nodes, state, p.npar, p.amp, p.nk, p.ks, out, S);
}

} // namespace

extern "C" int lsx_hip_response_stokes_work_cap(lsx_ctx* c, size_t nbytes)
{
    return GrowBuf::set_cap(c, BUF_STRESP_WORK, "lsx_hip_response_stokes_work_cap", nbytes);
}

// The argument rules of lsx_hip_response_stokes but the byte counts; nothing is launched.  (lsx_fit.hip asks them of its expanded
// field before its first launch.)
int lsxd::response_stokes_check(lsx_ctx* c, const char* who, const StokesCall& s, uint32_t params, const double* amplitude, int32_t nk,
                                const int32_t* ks)
{
    // ---- first what lsx_hip_stokes_rays checks, in its order ----
    int rc = stokes_check_call(c, who, s);
    if (!rc) rc = stokes_check_state(c, who, s);
    if (rc) return rc;
    // ---- ... then the response's own rules ----
    const int Ns = c->Nspace;
    std::string msg;
    if ((rc = lsxst::check_response(params, amplitude, Ns, nk, ks, (size_t)s.ncol, s.col0, s.B, msg, s.nfield())))
        return fail(rc, "%s: %s", who, msg.c_str());
    int par[lsxst::kMaxResponseParams] = {0, 0, 0, 0};
    const int nvar = 1 + 2 * lsxst::response_params(params, par);
    if ((int64_t)Ns * nvar > 65535 || s.nmu > 65535)
        return fail(LSX_EUNSUPPORTED, "%s: Nspace x (1 + 2 parameters) = %lld or nmu = %d is above a grid's 65535", who,
                    (long long)Ns * nvar, (int)s.nmu);
    return LSX_OK;
}

// The body of lsx_hip_response_stokes without its `stokes`.  sink null: the entry itself -- every pass is copied to rf.  An internal
// caller (lsx_fit.hip) hands a sink instead and rf null: a pass's rf stays in the pass's device array and the sink is called in the
// copy's place.  stokes_bytes: null, or the byte count of the entry's `stokes` to be checked with the others.
int lsxd::response_stokes_run(lsx_ctx* c, const char* who, const StokesCall& s, uint32_t params, const double* amplitude, int32_t nk,
                              const int32_t* ks, double* rf, size_t rf_bytes, const size_t* stokes_bytes, PassSink* sink)
{
    // ---- everything is checked on the host before anything is launched ----
    if (!rf && !sink) return fail(LSX_EINVAL, "%s: null argument", who);
    int rc = response_stokes_check(c, who, s, params, amplitude, nk, ks);
    if (rc) return rc;
    const int32_t nmu = s.nmu, ncol = s.ncol, nla = s.nla;
    const int Ns = c->Nspace;
    int par[lsxst::kMaxResponseParams] = {0, 0, 0, 0};
    const int npar = lsxst::response_params(params, par);
    const int nvar = 1 + 2 * npar;
    const int nkk = ks ? nk : Ns;
    const size_t plane = (size_t)nla * nmu, per_rf = (size_t)npar * 4 * plane * nkk;
    if (!sink && rf_bytes != (size_t)ncol * per_rf * 8) return fail(LSX_EINVAL, "%s: rf_bytes does not match [ncol][npar][4][nla][nk][nmu]", who);
    if (stokes_bytes && *stokes_bytes != (size_t)ncol * 4 * plane * 8) return fail(LSX_EINVAL, "%s: stokes_bytes does not match [ncol][4][nla][nmu]", who);

    std::vector<int32_t> pat_line;
    std::vector<double> pat_tab;
    if ((rc = stokes_patterns(c, who, s, pat_line, pat_tab))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = final_tables(c, who))) return rc;

    // the tables of the call: [pat_line | par | kreq | ks], [amp | pat_tab]; par and amp hold kMaxResponseParams entries, the first
    // npar in use
    std::vector<int32_t> ints(pat_line);
    const size_t o_par = ints.size();
    ints.insert(ints.end(), par, par + lsxst::kMaxResponseParams);
    const size_t o_kreq = ints.size();
    ints.resize(o_kreq + Ns, ks ? 0 : 1);
    const size_t o_ks = ints.size();
    for (int i = 0; i < nkk && ks; ++i) {
        ints[o_kreq + ks[i]] = 1;
        ints.push_back(ks[i]);
    }
    const size_t int_bytes = (ints.size() * sizeof(int32_t) + 7) & ~(size_t)7;
    double amps[lsxst::kMaxResponseParams] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < npar; ++i) amps[i] = amplitude[par[i]];
    GrowBuf& tab = c->buf[BUF_STRESP_TAB];
    if ((rc = tab.reserve(c, int_bytes + (lsxst::kMaxResponseParams + std::max<size_t>(1, pat_tab.size())) * 8))) return rc;
    HIPCHK(hipMemcpyAsync(tab.p, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(tab.p + int_bytes, amps, sizeof amps, hipMemcpyHostToDevice, c->stream));
    if (!pat_tab.empty())
        HIPCHK(hipMemcpyAsync(tab.p + int_bytes + sizeof amps, pat_tab.data(), pat_tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                      // the host vectors may go out of scope on any return below

    // columns per pass: the arrays of a pass stay under the cap (one column's need if that alone is more)
    GrowBuf& work = c->buf[BUF_STRESP_WORK];
    const size_t nblk = ((size_t)nla + 63) / 64, nlaP = nblk * 64;
    const size_t head = ((size_t)nmu + 1) & ~(size_t)1;
    const size_t w_nodes = (size_t)nmu * nvar * Ns * lsxst::kNodeDoubles * nlaP, w_state = (size_t)nmu * Ns * lsxst::kStateDoubles * nlaP;
    const size_t nf = (size_t)s.nfield();
    const size_t wcol = w_nodes + w_state + per_rf + nf * (size_t)Ns;
    const size_t chunk = pass_columns(ncol, work.cap, kWorkCapDefault, wcol, kGridYLimit);
    if ((rc = work.reserve(c, (head + chunk * wcol) * 8))) return rc;
    double* d_mu = work.as<double>();
    double* d_field = d_mu + head;
    double* d_nodes = d_field + chunk * nf * (size_t)Ns;
    double* d_state = d_nodes + chunk * w_nodes;
    double* d_rf = d_state + chunk * w_state;
    HIPCHK(hipMemcpyAsync(d_mu, s.mu, (size_t)nmu * 8, hipMemcpyHostToDevice, c->stream));

    RespParams p{};
    final_fill(p, c);
    final_fill_angles(p, c);
    p.nmu = nmu; p.la0 = s.la0; p.nla = nla; p.mu = d_mu;
    p.ntab = (int32_t)pat_tab.size();
    const int32_t* d_ints = tab.as<const int32_t>();
    p.pat_line = d_ints;
    p.kreq = d_ints + o_kreq;
    p.ks = ks ? d_ints + o_ks : nullptr;
    p.par = d_ints + o_par;
    p.amp = (const double*)(tab.p + int_bytes);
    p.pat_tab = p.amp + lsxst::kMaxResponseParams;
    p.field = d_field;
    p.npar = npar; p.nvar = nvar; p.nk = nkk; p.nlaP = (int32_t)nlaP;
    p.nodes = d_nodes; p.state = d_state; p.rf = d_rf;
    const size_t lds_nodes = ((size_t)64 + pat_tab.size() + lsxst::kCompDoubles) * 8;
    const size_t lds_walk = (size_t)LSX_EXP_TAB * 8;

    for (size_t b0 = 0; b0 < (size_t)ncol; b0 += chunk) {
        const size_t nb = std::min(chunk, (size_t)ncol - b0);
        p.col0 = (int32_t)(s.col0 + b0);
        p.fstride = (int64_t)(nb * Ns);
        if ((rc = stokes_upload_field(c, s, b0, nb, d_field))) return rc;
        // one launch of the nodes per angle (the profile function is evaluated per angle, as in lsx_stokes.hip), one of the walks for all
        for (int m0 = 0; m0 < nmu; ++m0) {
            p.mu0 = m0;
            const dim3 grid((unsigned)nblk, (unsigned)nb, (unsigned)(Ns * nvar));
            if (s.vlos) response_nodes_velocity(p, grid, lds_nodes, c->stream);
            else hipLaunchKernelGGL(k_response_nodes<false>, grid, dim3(64), lds_nodes, c->stream, p);
        }
        p.mu0 = 0;
        hipLaunchKernelGGL(k_response_walk, dim3((unsigned)nblk, (unsigned)nb, (unsigned)nmu), dim3(64), lds_walk, c->stream, p);
        HIPCHK(hipGetLastError());
        if (sink) {
            if ((rc = sink->pass(b0, nb, d_rf))) return rc;
        } else {
            HIPCHK(hipMemcpyAsync(rf + b0 * per_rf, d_rf, nb * per_rf * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(hipStreamSynchronize(c->stream));       // the arrays are re-used by the next pass
    }
    return LSX_OK;
}

extern "C" int lsx_hip_response_stokes(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                       const double* B, const double* gammaB, const double* chiB,
                                       const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                       uint32_t params, const double amplitude[3], int32_t nk, const int32_t* ks,
                                       double* rf, size_t rf_bytes, double* stokes, size_t stokes_bytes)
{
    const char* who = "lsx_hip_response_stokes";
    if (!rf) return fail(LSX_EINVAL, "%s: null argument", who);
    const StokesCall s{nmu, mu, col0, ncol, la0, nla, B, gammaB, chiB, ncomp, alpha, strength, shift};
    const int rc = response_stokes_run(c, who, s, params, amplitude, nk, ks, rf, rf_bytes, stokes ? &stokes_bytes : nullptr, nullptr);
    if (rc) return rc;
    // The vector of the call's own field comes from the Stokes pass itself, so that it has that pass's bits by construction.  The
    // walk up forms the same vector through the same functions (the host build's is bit for bit lsx_stokes_host_window's), but in
    // another kernel the device compiler contracts products and sums into fused operations differently: measured on an MI355X, a
    // quarter of the entries differ from k_stokes_rays' in the last bits (at most 1.2e-14 of I).  One more launch per angle
    if (stokes) return stokes_rays_run(c, "lsx_hip_stokes_rays", s, stokes, stokes_bytes, nullptr);
    return LSX_OK;
}

extern "C" int lsx_hip_velocity_response_stokes(lsx_ctx* c, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                                const double* B, const double* gammaB, const double* chiB,
                                                const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                                uint32_t params, const double amplitude[4], int32_t nk, const int32_t* ks,
                                                double* rf, size_t rf_bytes, double* stokes, size_t stokes_bytes, const double* vlos)
{
    const char* who = "lsx_hip_velocity_response_stokes";
    if (!rf) return fail(LSX_EINVAL, "%s: null argument", who);
    // (without a velocity: the rules and the kernels of lsx_hip_response_stokes, so bit 8 is refused as an unknown bit)
    const StokesCall s{nmu, mu, col0, ncol, la0, nla, B, gammaB, chiB, ncomp, alpha, strength, shift, vlos};
    const int rc = response_stokes_run(c, who, s, params, amplitude, nk, ks, rf, rf_bytes, stokes ? &stokes_bytes : nullptr, nullptr);
    if (rc) return rc;
    if (stokes) return stokes_rays_run(c, vlos ? "lsx_hip_velocity_stokes_rays" : "lsx_hip_stokes_rays", s, stokes, stokes_bytes, nullptr);
    return LSX_OK;
}
