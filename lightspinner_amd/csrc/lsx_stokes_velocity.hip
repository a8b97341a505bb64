// lsx_stokes_velocity.hip -- the instance of the response's stage 1 for a call with a velocity of its own
// (include/lsx_hip_stokes_velocity.h, lsx_hip_velocity_response_stokes): k_response_nodes<true> of
// lsx_stokes_response_nodes.h, in a unit of its own so that the unit of lsx_stokes_response.hip holds the kernels it always held and
// this one's resource report (build/lsx_stokes_velocity.ru.log) is this instance's.  The host side of the call, the walk and the
// entry are lsx_stokes_response.hip's; the Stokes pass's instance with a velocity is k_stokes_rays<NM, true> of lsx_stokes.hip.
// gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/lsx_hip.h"
#include "lsx_stokes_response_nodes.h"

void lsxd::response_nodes_velocity(const RespParams& p, dim3 grid, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL(k_response_nodes<true>, grid, dim3(64), lds, stream, p);
}
