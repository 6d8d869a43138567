// row32_unit.inc -- one of eight translation units with the row-layout MeritFunction kernels of plan MFMA32's shapes
// (kernels/ilqr_row32.hip: n, m compile-time): the shapes with n mod 8 == R32_UNIT (included by row32_u0.hip .. row32_u7.hip, which
// define R32_UNIT and R32_UNIT_FN).  The same spread as the backward kernel's (tile32_bwd_unit.inc).
#include <hip/hip_runtime.h>

#include "kernels/ilqr_generic.hip"
#include "kernels/ilqr_row32.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

// waves per SIMD an instantiation is budgeted for: two while eight waves' images (two problems each) fit a compute unit's LDS
constexpr int row32_wps(int n, int m) { return r32_image_doubles(n, m) <= 1150 ? 2 : 1; }
constexpr int row32_wps_dual(int n, int m) { return r32_image_doubles(n, m) <= 2300 ? 2 : 1; }   // (the two-trial pass: one image per wave)

// the kernels of one shape: instantiated for plan MFMA32's shapes (tile32_shape_ok).  0 launched, 1 = not carried, 2 = launch error
template <int N_, int M_>
static int row32_static(hipStream_t stream, const RouteStep& st, const IlqrGenArgs<double>& a) {
  if constexpr (tile32_shape_ok(N_, M_)) {
    const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
    switch (st.id) {
      case K_ROW_MERIT: hipLaunchKernelGGL((row32_merit_kernel<double, N_, M_, row32_wps(N_, M_)>), grid, block, st.lds, stream, a); break;
      case K_ROW_MERIT | KF_DUAL: hipLaunchKernelGGL((row32_merit_kernel<double, N_, M_, row32_wps_dual(N_, M_), true>), grid, block, st.lds, stream, a); break;
      case K_ROW_INIT: hipLaunchKernelGGL((row32_rollout_init_kernel<double, N_, M_, row32_wps(N_, M_)>), grid, block, st.lds, stream, a); break;
      case K_ROW_STAT: hipLaunchKernelGGL((row32_stationarity_kernel<double, N_, M_, 2>), grid, block, st.lds, stream, a); break;
      case K_ROW_STAT_REDUCE: hipLaunchKernelGGL(row32_stat_reduce_kernel<double>, grid, block, st.lds, stream, a, st.chunks); break;
      case K_ROW_EXPAND: hipLaunchKernelGGL((row32_expand_kernel<double, N_, M_, 2>), grid, block, st.lds, stream, a); break;
      default: return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
  } else {
    return 1;
  }
}

#define R32_ROW(N_)                                              \
  case (N_):                                                     \
    switch (a.m) {                                               \
      case 1: return row32_static<(N_), 1>(stream, st, a);       \
      case 2: return row32_static<(N_), 2>(stream, st, a);       \
      case 3: return row32_static<(N_), 3>(stream, st, a);       \
      case 4: return row32_static<(N_), 4>(stream, st, a);       \
      case 5: return row32_static<(N_), 5>(stream, st, a);       \
      case 6: return row32_static<(N_), 6>(stream, st, a);       \
      case 7: return row32_static<(N_), 7>(stream, st, a);       \
      case 8: return row32_static<(N_), 8>(stream, st, a);       \
      default: break;                                            \
    }                                                            \
    break;

int R32_UNIT_FN(hipStream_t stream, const RouteStep& st, const IlqrGenArgs<double>& a) {
  switch (a.n) {
    R32_ROW(R32_UNIT + 0 == 0 ? 32 : R32_UNIT)   // (n = 0 does not exist; 32 has no kernel)
    R32_ROW(R32_UNIT + 8)
    R32_ROW(R32_UNIT + 16)
    R32_ROW(R32_UNIT + 24)
    default: break;
  }
  return 1;
}
#undef R32_ROW

}  // namespace altro_hip
