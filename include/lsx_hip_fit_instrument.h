/* lsx_hip_fit_instrument.h -- the field fit on profiles as an instrument saw them: smeared by a line-spread function and sampled on
 * the instrument's own pixels (lsx_fit_instrument, lsx_hip_fit.h).  Entries of the HIP library alone; included by lsx_hip_fit.h.
 * Smearing and sampling are linear in the spectrum, S' = K S and J' = K J: no new physics, one more step on the device between the
 * Stokes pass and the response pass on one side and the reduction on the other.
 * Conventions as in lsx.h: 0 = ok, otherwise an LSX_E* code and lsx_last_error(); float64, C-contiguous arrays.
 *
 * (The names do not begin with lsx_hip_fit: that prefix stays the four entries of lsx_hip_fit.h.) */
#ifndef LSX_HIP_FIT_INSTRUMENT_H
#define LSX_HIP_FIT_INSTRUMENT_H

#include "lsx_hip_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lsx_hip_fit_field_normal and lsx_hip_fit_field_chi2 through an instrument: their arguments, then `inst`.  obs and weight are
 * [ncol][4][nobs][nmu]; a data point is (Stokes parameter, pixel, angle), M' = 4 nobs nmu a column.  With
 *     r = obs - S',   S' = K S,   J' = K J        S, J: what the entries of lsx_hip_fit.h form on the window's grid
 * they return chi2 = sum w r^2, grad = J'^T W r, hess = J'^T W J'.  rf never leaves the device, one writer per value, no atomics;
 * the order of every sum depends on (nla, nobs, width, nmu, Nspace, nnode) alone: a column's numbers keep their bits whatever the
 * column range, the other columns or any work cap, and the chi2 entry gives the bits of the normal entry's chi2.
 * inst == NULL: the entries of lsx_hip_fit.h themselves, the same code path and the same bits.
 * Refused before anything is launched, with LSX_EINVAL: null inst->first or inst->weight; nobs < 1; width < 1 or width > nla; a
 * first[o] outside [0, nla - width] (the message names the pixel); a weight of the instrument that is not finite; with
 * LSX_EUNSUPPORTED: 4 nobs nmu over the limit 4 nla nmu has; then everything the entries of lsx_hip_fit.h refuse, obs and weight
 * checked at their size here.  Read-only on the context. */
int lsx_hip_instrument_fit_normal(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                  const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                  const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                                  const double amplitude[3], const double* obs, const double* weight,
                                  double* chi2, double* grad, double* hess, double* field_out, const lsx_fit_instrument* inst);

int lsx_hip_instrument_fit_chi2(lsx_ctx* ctx, int32_t nmu, const double* mu, int32_t col0, int32_t ncol, int32_t la0, int32_t nla,
                                const int32_t* ncomp, const int32_t* alpha, const double* strength, const double* shift,
                                const int32_t nnode[3], const double* basis, const double* base, const double* nodes,
                                const double* obs, const double* weight, double* chi2, double* field_out,
                                const lsx_fit_instrument* inst);

/* The instrument applied to arrays handed over, on the device, by the kernel the fit runs: in [nrow][nla][nmu] -> out
 * [nrow][nobs][nmu] (nrow = 4 ncol for Stokes vectors as the Stokes pass lays them).  The synthetic profiles to lay over the data;
 * what the fit forms inside for the same numbers, bit for bit.  `in` is not checked for finiteness (the sum is what it is).
 * Refused: null arguments, nla, nmu or nrow < 1, and the instrument's rules above.  The rows are taken in groups under the fit's
 * work cap (lsx_hip_fit_field_work_cap).  Read-only on the context. */
int lsx_hip_instrument_apply(lsx_ctx* ctx, const lsx_fit_instrument* inst, int32_t nla, int32_t nmu, int32_t nrow, const double* in,
                             double* out);

#ifdef __cplusplus
}
#endif
#endif /* LSX_HIP_FIT_INSTRUMENT_H */
