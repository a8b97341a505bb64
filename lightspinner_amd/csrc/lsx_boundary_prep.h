// lsx_boundary_prep.h -- the host-side argument rules of lsx_hip_set_boundary (include/lsx_hip_boundary.h) and the scatter of a
// call's arrays into the context's store; plain C++, shared by lsx_boundary.hip and the stand-alone sanitizer program
// (lsx_boundary_san_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/lsx_hip_boundary.h"

namespace lsxbnd {

// nullptr if the arguments are acceptable for a context of ncol_ctx columns, else what is wrong with them (LSX_EINVAL)
inline const char* check_args(int64_t ncol_ctx, int64_t col0, int64_t ncol, int32_t lower, int32_t upper, const double* I_lower,
                              const double* I_upper)
{
    auto known = [](int32_t k) { return k == LSX_BOUNDARY_ZERO || k == LSX_BOUNDARY_THERMALISED || k == LSX_BOUNDARY_GIVEN; };
    if (!known(lower)) return "unknown lower kind (LSX_BOUNDARY_ZERO, _THERMALISED or _GIVEN)";
    if (!known(upper)) return "unknown upper kind (LSX_BOUNDARY_ZERO, _THERMALISED or _GIVEN)";
    if (col0 < 0 || ncol < 1 || col0 + ncol > ncol_ctx) return "the column range is outside the context";
    if (lower == LSX_BOUNDARY_GIVEN && !I_lower) return "the lower kind is GIVEN and I_lower is NULL";
    if (upper == LSX_BOUNDARY_GIVEN && !I_upper) return "the upper kind is GIVEN and I_upper is NULL";
    if (lower != LSX_BOUNDARY_GIVEN && I_lower) return "I_lower is given and the lower kind is not GIVEN";
    if (upper != LSX_BOUNDARY_GIVEN && I_upper) return "I_upper is given and the upper kind is not GIVEN";
    return nullptr;
}

// the host copy of the kinds, [ncol_ctx][2]: what a context holds before the first call
inline void default_kinds(int32_t* kinds, size_t ncol_ctx)
{
    for (size_t c = 0; c < ncol_ctx; ++c) {
        kinds[2 * c + 0] = LSX_BOUNDARY_THERMALISED;
        kinds[2 * c + 1] = LSX_BOUNDARY_ZERO;
    }
}

inline void set_kinds(int32_t* kinds, size_t col0, size_t ncol, int32_t lower, int32_t upper)
{
    for (size_t c = col0; c < col0 + ncol; ++c) {
        kinds[2 * c + 0] = lower;
        kinds[2 * c + 1] = upper;
    }
}

// element offset of (end, column) in the store [end: 0 lower, 1 upper][ncol_ctx][per], per = Nspect * Nrays
inline size_t store_offset(int end, size_t ncol_ctx, size_t col, size_t per) { return ((size_t)end * ncol_ctx + col) * per; }

} // namespace lsxbnd
