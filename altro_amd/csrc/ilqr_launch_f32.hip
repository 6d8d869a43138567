// Kernel instantiations of the batched iLQR loop for element type float (see kernels/ilqr_types.h); which of them runs, and with which grid: loop_route.h.
#include <hip/hip_runtime.h>

#include "kernels/ilqr_lane.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

template <>
int ilqr_launch_kernel<float>(hipStream_t stream, const RouteStep& st, int kind, int n, int m, const IlqrArgs<float>& a) {
  using T = float;
  const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
  bool done = false;
#define GO(...) hipLaunchKernelGGL((__VA_ARGS__), grid, block, st.lds, stream, a); break
#define X(K_, N_, M_)                                                                        \
  if (!done && kind == K_ && n == N_ && m == M_) {                                           \
    done = true;                                                                             \
    switch (st.id) {   /* (dense: the instantiation for the dense quadratic cost, kernels/ilqr_lane.hip) */ \
      case lane_id(RTC_ROLLOUT): GO(ilqr_rollout_kernel<K_, N_, M_, T>);                     \
      case lane_id(RTC_ACCEPT): GO(ilqr_accept_kernel<N_, M_, T>);                           \
      case lane_id(RTC_EXPAND, true): GO(ilqr_expand_kernel<K_, N_, M_, T, 1>);              \
      case lane_id(RTC_EXPAND): GO(ilqr_expand_kernel<K_, N_, M_, T>);                       \
      case lane_id(RTC_MERIT_ROLL): GO(ilqr_merit_roll_kernel<K_, N_, M_, T>);               \
      case lane_id(RTC_MERIT_POINT, true): GO(ilqr_merit_point_kernel<K_, N_, M_, T, 1>);    \
      case lane_id(RTC_MERIT_POINT): GO(ilqr_merit_point_kernel<K_, N_, M_, T>);             \
      case lane_id(RTC_MERIT_SUM): GO(ilqr_merit_sum_kernel<K_, N_, M_, T>);                 \
      case lane_id(RTC_MERIT, true): GO(ilqr_merit_kernel<K_, N_, M_, T, 1>);                \
      case lane_id(RTC_MERIT): GO(ilqr_merit_kernel<K_, N_, M_, T>);                         \
      case lane_id(RTC_SPEC_SELECT): GO(ilqr_spec_select_kernel<N_, M_, T>);                 \
      case lane_id(RTC_DUAL): GO(ilqr_dual_update_kernel<N_, M_, T>);                        \
      case lane_id(RTC_SHIFT): GO(ilqr_shift_kernel<N_, M_, T>);                             \
      case lane_id(RTC_ZERO_RESIDUALS): GO(ilqr_zero_residuals_kernel<T>);                   \
      case lane_id(RTC_STATIONARITY): GO(ilqr_stationarity_kernel<N_, M_, T>);               \
      default: return 1;                                                                     \
    }                                                                                        \
  }
  ILQR_LANE_MODELS(X)
#undef X
#undef GO
  if (!done) return 1;
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace altro_hip
