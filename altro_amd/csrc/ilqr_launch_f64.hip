// Kernel instantiations of the batched iLQR loop for element type double (see kernels/ilqr_types.h); which of them runs, and with which grid: loop_route.h.
#include <hip/hip_runtime.h>

#include "kernels/ilqr_lane.hip"
#include "kernels/ilqr_loop_kernels.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

template <>
int ilqr_launch_kernel<double>(hipStream_t stream, const RouteStep& st, int kind, int n, int m, const IlqrArgs<double>& a) {
  using T = double;
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

bool ilqr_supported(int kind, int n, int m) { return lane_model_supported(kind, n, m); }

int ilqr_launch_results(hipStream_t stream, const IlqrProb* prob, IlqrResult* out, int batch) {
  hipLaunchKernelGGL(ilqr_results_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, prob, out, batch);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int ilqr_launch_list_running(hipStream_t stream, const int* flags, const int* list_in, int count_in, int* list_out, int resident) {
  hipLaunchKernelGGL(ilqr_list_running_kernel, dim3(1), dim3(1024), 0, stream, flags, list_in, count_in, list_out, resident);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int ilqr_launch_loop(hipStream_t stream, int which, const IlqrLoopArgs& a) {
  const dim3 gb((a.batch + 255) / 256), bb(256);
  switch (which) {
    case ILK_LOOP_INIT: hipLaunchKernelGGL(ilqr_loop_init_kernel, gb, bb, 0, stream, a); break;
    case ILK_LS_BEGIN: hipLaunchKernelGGL(ilqr_ls_begin_kernel, gb, bb, 0, stream, a); break;
    case ILK_LS_FEED: hipLaunchKernelGGL(ilqr_ls_feed_kernel, gb, bb, 0, stream, a); break;
    case ILK_FINISH_ITER: hipLaunchKernelGGL(ilqr_finish_iter_kernel, gb, bb, 0, stream, a); break;
    case ILK_MARK_RUNNING: hipLaunchKernelGGL(ilqr_mark_running_kernel, gb, bb, 0, stream, a); break;
    case ILK_SET_PENALTY: hipLaunchKernelGGL(ilqr_set_penalty_kernel, gb, bb, 0, stream, a); break;
    case ILK_PENALTY_UPDATE: hipLaunchKernelGGL(ilqr_penalty_update_kernel, gb, bb, 0, stream, a); break;
    case ILK_REG_RETRY: hipLaunchKernelGGL(ilqr_reg_retry_kernel, gb, bb, 0, stream, a); break;
    default: return 1;
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace altro_hip
