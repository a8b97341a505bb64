/* lsx_hip_epilogue.h -- which kernels behind the sweep a context of the HIP library has launched: the fast-continuum pre-pass,
 * the row-mapped and column-mapped fast-continuum epilogue, the Gamma epilogue.  HIP library only (lsx_hip.h includes this file);
 * tests/test_epilogue_instances.py reads it to assert that the instance a case was made for did run. */
#ifndef LSX_HIP_EPILOGUE_H
#define LSX_HIP_EPILOGUE_H

#include "lsx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Introspection for the tests: how often each kernel behind the sweep has been launched since the context was made.
 * out[LSX_HIP_EPILOGUE_INFO_N]:
 *   [0 .. 35]   the row-mapped fast-continuum epilogue, one (code, launches) pair per compiled instance,
 *               code = 1024 lanes per depth row + 2 threads per workgroup + 1 if the column's operands are staged in segments;
 *   [36 .. 42]  the column-mapped epilogue, per tile list: 0 / 1 / 2 lines fed by linked continua, unused, the same for big sets;
 *   [43], [44]  the fast-continuum pre-pass: the whole column staged at once, in segments;
 *   [45 .. 47]  the Gamma epilogue: small batches, a thread per level, a thread's matrix in LDS;  [48] the threads of the last.
 * Returns the number of values written (0: no context or no array).  Host only: nothing is launched or waited for. */
#define LSX_HIP_EPILOGUE_INFO_N 49
int32_t lsx_hip_epilogue_info(const lsx_ctx* ctx, int64_t* out);

#ifdef __cplusplus
}
#endif

#endif /* LSX_HIP_EPILOGUE_H */
