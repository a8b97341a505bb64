// lsx_stokes_response_nodes.h -- stage 1 of the Stokes response functions (lsx_stokes_response.hip, whose header comment describes it; DESIGN.md
// 4.23): the parameters of the two stages and k_response_nodes, in a header because the kernel has two instances in two units:
//   k_response_nodes<false>   lsx_stokes_response.hip: the kernel as it always was, the velocity is the context's
//   k_response_nodes<true>    lsx_stokes_velocity.hip: a call with a velocity of its own (include/lsx_hip_stokes_velocity.h)
// Each unit's resource report (build/<unit>.ru.log) lists the instances it holds.
#pragma once
#include <hip/hip_runtime.h>

#include "lsx_final_host.h"
#include "lsx_stokes_dev.h"

namespace lsxd {

struct RespParams {
    // ---- what k_stokes_rays reads (lsx_stokes.hip, StokesParams) ----
    int32_t Ns, Nspect, NLtot, Natoms, NlinesA, Ncont, L, Nrays;
    int32_t col0, nmu, mu0;     // first column of the launch; angles of the call; the angle of this launch of k_response_nodes
    int32_t la0, nla;
    int32_t phi_compact, sca_per_lambda, phi_G;
    int32_t ntab;
    int64_t til_col, phi_col, sca_col, fstride;
    const double *wavelength, *u_la, *exp2_tab, *voigt_W, *mu;
    const int32_t* la_ptr;
    const FinalEnt* ents;
    const int32_t* la_tile;
    const double *height, *temperature, *n, *nsr, *bgchi_T, *bgeta_T, *J_T, *E_T, *sca, *phi_T;
    const double *aDamp, *vBroad, *vlos;
    const uint8_t* prof_kind;
    const int32_t* bnd;
    const int32_t* pat_line;
    const double* pat_tab;
    const double* field;
    // ---- the response's own ----
    int32_t npar, nvar, nk, nlaP;       // requested parameters, 1 + 2 npar, requested depths, nla rounded up to whole wavefronts
    const int32_t* par;                 // [npar] the requested parameters (0 B, 1 gammaB, 2 chiB, 3 vlos)
    const double* amp;                  // [npar] their amplitudes
    const int32_t* ks;                  // [nk] requested depths, or null: all
    const int32_t* kreq;                // [Ns]: 1 where the depth is requested
    double* nodes;                      // [launch column][nmu][nvar][Ns][11][nlaP]
    double* state;                      // [launch column][nmu][Ns][5][nlaP]
    double* rf;                         // [launch column][npar][4][nla][nk][nmu]
};

__device__ __forceinline__ size_t node_offset(const RespParams& p, size_t cl, int m, int var, int k)
{
    return ((((cl * p.nmu + m) * p.nvar + var) * p.Ns + k) * (size_t)lsxst::kNodeDoubles) * p.nlaP;
}

// ---- stage 1: the node of one depth under one variant of the field ----
// VEL: the call has a velocity -- the fourth array of p.field in the place of the context's vlos, moved by the variants of vlos, and
// every line formed from the kept broadening arrays (as k_stokes_rays<NM, true>).  VEL = false is the kernel as it was.
template <bool VEL>
__global__ void __launch_bounds__(64) k_response_nodes(const RespParams p)
{
    const int Ns = p.Ns, L = p.L;
    const int k = blockIdx.z / p.nvar, var = blockIdx.z - k * p.nvar;
    if (var > 0 && !p.kreq[k]) return;                    // (block-uniform) a variant is read at requested depths only
    extern __shared__ double smem[];                      // the Voigt function's table (56 doubles), the patterns
    if (threadIdx.x < 56) smem[threadIdx.x] = p.voigt_W ? p.voigt_W[threadIdx.x] : 0.0;
    for (int e = threadIdx.x; e < p.ntab; e += 64) smem[64 + e] = p.pat_tab[e];
    __syncthreads();
    const lds_f64* vtab = (const lds_f64*)smem;
    const lds_f64* ptab = vtab + 64;

    const int q_raw = blockIdx.x * 64 + threadIdx.x;
    const int q = q_raw < p.nla ? q_raw : p.nla - 1;
    const int la = p.la0 + q;
    const size_t col = (size_t)p.col0 + blockIdx.y;
    const FinalColumn f = final_column(p, col, la);
    const FinalAngles fa = final_angles(p, col);
    const double* aD_c = p.aDamp + col * (size_t)p.NlinesA * Ns;
    const double* vB_c = p.vBroad + col * (size_t)p.Natoms * Ns;
    const double* fld = p.field + (size_t)blockIdx.y * Ns;
    const double* vL_c = VEL ? fld + 3 * p.fstride : p.vlos + col * Ns;
    const double wav = p.wavelength[la], u_la = p.u_la[la];
    const double mu = p.mu[p.mu0];

    const double Ev = f.Eb ? f.Eb[(size_t)k * L] : 0.0;
    const double c0 = f.bgchi[(size_t)k * L];
    const double h0 = f.bgeta[(size_t)k * L] + f.sca[(size_t)k * f.sstr] * f.Jd[(size_t)k * L];
    double Bk = fld[k], gk = fld[p.fstride + k], xk = fld[2 * p.fstride + k];
    double vlk = VEL ? vL_c[k] : 0.0;                     // (without a velocity the context's is read where a line needs it, as ever)
    if (var > 0) {
        if (VEL) lsxst::field_variant(p.par[(var - 1) >> 1], ((var - 1) & 1) == 0, p.amp[(var - 1) >> 1], Bk, gk, xk, vlk);
        else lsxst::field_variant(p.par[(var - 1) >> 1], ((var - 1) & 1) == 0, p.amp[(var - 1) >> 1], Bk, gk, xk);
    }
    lsxst::Acc acc;
    lsxst::acc_init(acc, c0, h0);
    const lsxst::Geo geo = lsxst::geometry(gk, xk, mu);
    for (int e = f.e0; e < f.e1; ++e) {
        const FinalEnt& t = p.ents[e];
        const double ni = f.n_col[(size_t)t.li * Ns + k], nj = f.n_col[(size_t)t.lj * Ns + k];
        if (t.is_line) {
            const double nd = t.a * (ni - t.g * nj);
            const int nc = p.pat_line[2 * t.row];
            if (VEL || nc > 0 || fa.raydep) {
                const lds_f64* tab = ptab + lsxst::kCompDoubles * p.pat_line[2 * t.row + 1];
                const double vb = vB_c[(size_t)t.atom * Ns + k], ad = aD_c[(size_t)t.row * Ns + k], vl = VEL ? vlk : vL_c[k];
                const double v = (wav - t.lambda0) * kCLight / (vb * t.lambda0);
                const double rn = 1.0 / (sqrt(M_PI) * vb);
                const double vZ = nc > 0 ? lsxst::kLarmor * (kNM_TO_M * t.lambda0) * Bk / vb : 0.0;
                const double ne = nj * t.Uc;
                const lsxst::Prof pr = lsxst::line_profiles(nc, tab, ad, v + 1.0 * (mu * vl / vb), vZ, vtab);
                if (nc > 0) lsxst::line_add(acc, nd, ne, pr, rn, geo);
                else lsxst::line_add_plain(acc, nd, ne, pr, rn);
            } else {
                const size_t x = p.phi_compact ? (size_t)k : ((size_t)Ns + k) * p.Nrays;
                const double pv = p.phi_T[phi_elem(col, p.phi_G, (size_t)p.phi_col, (size_t)t.phi_base, x, t.phi_len, t.phi_l)];
                const double c1 = nd * pv, h1 = nj * (t.Uc * pv);
                acc.eI += c1; acc.mI += h1;
            }
        } else {
            const double pv = (f.nsr_col[(size_t)t.row * Ns + k] * Ev) * t.a;
            const double c1 = ni * t.a - nj * pv, h1 = nj * (u_la * pv);
            acc.eI += c1; acc.mI += h1;
        }
    }
    lsxst::node_store(acc, p.nodes + node_offset(p, blockIdx.y, p.mu0, var, k) + q_raw, (size_t)p.nlaP);
}

// the launch of k_response_nodes<true> (lsx_stokes_velocity.hip); the caller asks hipGetLastError
void response_nodes_velocity(const RespParams& p, dim3 grid, size_t lds, hipStream_t stream);

} // namespace lsxd
