// lsx_fit_inst.h -- what lsx_fit.hip asks of lsx_fit_instrument.hip (include/lsx_hip_fit_instrument.h): the rules of an
// instrument, its place in the head of a device buffer, and the launch of k_fit_smear on the fit's arrays.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lsx_hip_fit.h"
#include "lsx_ctx.h"

namespace lsxd {

// the instrument's rules for a window of nla wavelengths and nmu angles (`who`: the entry's name in the messages); ns: the Stokes
// blocks of a row (4 in the fit, 1 in lsx_hip_instrument_apply)
int fit_instrument_check(const char* who, const lsx_fit_instrument* inst, int32_t nla, int32_t nmu, int32_t ns);

// doubles the instrument takes in the head of a device buffer: weight [nobs][width], then first [nobs] as int32
inline size_t fit_instrument_doubles(const lsx_fit_instrument* inst)
{
    return (size_t)inst->nobs * inst->width + ((size_t)inst->nobs + 1) / 2;
}
// ... and its upload there, behind the context's stream
int fit_instrument_upload(lsx_ctx* c, const lsx_fit_instrument* inst, double* d_head);

// One launch of k_fit_smear behind the context's stream: lane = observed point d' of M' = ns nobs nmu, grid y = column, z = row.
// Row z < P of column y is J + ((cl0 + y) P + z) M -> Jo + ((cl0 + y) P + z) M'; row z = P is S + (cl0 + y) M -> So + (cl0 + y) M'
// (M = ns nla nmu).  nz rows from the first: P + 1 (the Jacobian and the Stokes vector), or P = 0 and 1 (the Stokes vector alone).
struct FitSmear {
    int32_t ns, nla, nmu, nobs, width, P;
    const double* d_inst;             // where fit_instrument_upload put it
    const double *J, *S;
    double *Jo, *So;
};
void fit_smear_launch(lsx_ctx* c, const FitSmear& f, size_t cl0, size_t ncol);

} // namespace lsxd
