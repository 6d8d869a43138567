// row32_model.hip -- the row-layout MeritFunction kernels (kernels/ilqr_row32.hip) with a compiled-in device model past the (12, 4)
// tile: MODEL_QUADROTOR13 at (13, 4), the model ilqr_generic_model_supported (ilqr_launch_generic.hip) knows.  A unit of its own: every
// lane of the kernel evaluates the model and its two Jacobians in registers.
#include <hip/hip_runtime.h>

#include "kernels/ilqr_generic.hip"
#include "kernels/ilqr_row32.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

int row32_model_launch(hipStream_t stream, const RouteStep& st, const IlqrGenArgs<double>& a) {
  if (a.mp.kind != MODEL_QUADROTOR13 || a.n != 13 || a.m != 4) return 1;
  const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
  // One wave per SIMD: the model's Jacobians next to the kernel's ring of fetched blocks want ~420 registers, and a wave that spills
  // them (187 registers at two waves per SIMD) waits for its scratch reloads behind the ring's loads: 1.04 ms per evaluation of 4096
  // vehicles x 30 knot points against 0.31 like this (generic_merit_kernel<.., MK>: 0.96).
  switch (st.id) {
    case K_ROW_MERIT | KF_MODEL: hipLaunchKernelGGL((row32_merit_kernel<double, 13, 4, 1, false, MODEL_QUADROTOR13>), grid, block, st.lds, stream, a); break;
    case K_ROW_EXPAND_DYN | KF_MODEL: hipLaunchKernelGGL((row32_expand_dyn_kernel<double, 13, 4, MODEL_QUADROTOR13>), grid, block, st.lds, stream, a); break;
    case K_ROW_MERIT | KF_DUAL | KF_MODEL: hipLaunchKernelGGL((row32_merit_kernel<double, 13, 4, 1, true, MODEL_QUADROTOR13>), grid, block, st.lds, stream, a); break;
    default: return 1;
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace altro_hip
