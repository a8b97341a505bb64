/* lsx_hip_eqpops.h -- LTE populations of any atoms on the device, active in the context or not: the reference's
 * RadiativeSet.compute_eq_pops (atomic_set.py:361-375) over lte_pops(debye=True) (:105-145); an entry of the HIP library alone,
 * included by lsx_hip.h.  It is the link between an atmosphere and lsx_set_atmosphere, which takes nHGround (the LTE ground
 * population of hydrogen, an atom that need not be in the context) and nTotal from its caller.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays; everything is
 * checked on the host before anything is launched. */
#ifndef LSX_HIP_EQPOPS_H
#define LSX_HIP_EQPOPS_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsx_eq_atom {
    int32_t Nlevel, reserved;
    const lsx_level* levels;         /* [Nlevel]: E_SI, g, stage (lsx.h); level 0 is the ground level the others are counted from */
    double abundance;                /* relative to hydrogen: nTotal = abundance * nHTot (atomic_set.py:368)                       */
} lsx_eq_atom;

/* For ncol columns of the context's Nspace depths and each of the natoms atoms, per (column, depth):
 *   dEion = c2 sqrt(ne / T), cNe_T = 0.5 ne (c1 / T)^1.5                                                  (:120-121)
 *   nStar_i / nStar_0 = (g_i / g_0) exp(-(dE_i - nDebye_i dEion) / (kB T)) / cNe_T ** dZ_i, i >= 1        (:127-137)
 *   nStar_0 = nTotal / (1 + sum_i nStar_i / nStar_0), nStar_i *= nStar_0                                  (:138-143)
 * with dE_i = E_i - E_0, dZ_i = stage_i - stage_0, nDebye_i = sum of stage_i, stage_i + 1, ... (dZ_i terms, :113-118; formed on
 * the host, as lsx_set_atomic_data forms it), and cNe_T ** dZ with numpy's cases for an integer exponent (0 -> 1, 1 -> x,
 * 2 -> x x, otherwise pow).  One thread per (column, depth), in the reference's operation order.
 * For an atom that is also active in the context, nStar is bit for bit what lsx_set_atmosphere(lte_pops = 1) leaves in LSX_NSTAR
 * on the same temperature, ne and nTotal = abundance * nHTot.
 * ctx supplies Nspace, the device and the stream (as for lsx_hip_eos).  The call does not touch the context's state and needs
 * neither lsx_set_atomic_data nor set columns; any ncol >= 1.
 * temperature, ne, nHTot: [ncol][Nspace], SI.
 * nStar:  [ncol][sum of Nlevel][Nspace], the atoms' levels concatenated in the order of `atoms`; host memory.
 * nTotal: [ncol][natoms][Nspace]; may be NULL.
 * LSX_EINVAL, found on the host before anything is launched: a null context, atoms, input array or nStar; natoms < 1; ncol < 1;
 *   Nlevel < 1 or null levels; g <= 0 or not finite; a non-finite E_SI; a level whose stage lies below level 0's; abundance < 0
 *   or not finite; temperature or ne not finite or <= 0; nHTot not finite or < 0. */
int lsx_hip_eq_pops(lsx_ctx* ctx, int32_t natoms, const lsx_eq_atom* atoms, int32_t ncol, const double* temperature,
                    const double* ne, const double* nHTot, double* nStar, double* nTotal);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_EQPOPS_H */
