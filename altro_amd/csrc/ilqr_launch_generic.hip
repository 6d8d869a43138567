// Kernel instantiations of the iLQR loop for plan GENERIC (kernels/ilqr_generic.hip): any (n, m) up to 32, dynamics as data, and the
// kernels that step a compiled-in device model (fp64 handles).  Which of them runs, and with which grid: loop_route.h.
#include <hip/hip_runtime.h>

#include "kernels/ilqr_generic.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

bool ilqr_generic_model_supported(int kind, int n, int m) { return gen_model_supported(kind, n, m); }

template <typename T>
static int gen_launch(hipStream_t stream, const RouteStep& st, const IlqrGenArgs<T>& a) {
  const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
#define GO(...) hipLaunchKernelGGL((__VA_ARGS__), grid, block, st.lds, stream, a); break
  if constexpr (sizeof(T) == 8) {
    if (st.id & KF_MODEL) {
      if (a.mp.kind != MODEL_QUADROTOR13) return 1;
      switch (st.id) {
        case K_GEN_ROLLOUT | KF_MODEL: GO(generic_model_rollout_kernel<double, MODEL_QUADROTOR13, 13, 4>);
        case K_GEN_MERIT | KF_MODEL: GO(generic_merit_kernel<double, false, MODEL_QUADROTOR13, 13, 4>);
        case K_GEN_EXPAND_DYN | KF_MODEL: GO(generic_model_expand_dyn_kernel<double, MODEL_QUADROTOR13, 13, 4>);
        default: return 1;
      }
      return hipGetLastError() == hipSuccess ? 0 : 2;
    }
  }
  switch (st.id) {
    case K_GEN_ROLLOUT: GO(generic_rollout_kernel<T>);
    case K_GEN_ACCEPT: GO(generic_accept_kernel<T>);
    case K_GEN_EXPAND_AL: GO(generic_expand_al_kernel<T>);
    case K_GEN_EXPAND: GO(generic_expand_kernel<T>);
    case K_GEN_DUAL: GO(generic_dual_update_kernel<T>);
    case K_GEN_MERIT | KF_STAGED: GO(generic_merit_kernel<T, true>);
    case K_GEN_MERIT: GO(generic_merit_kernel<T, false>);
    case K_GEN_STATIONARITY: GO(generic_stationarity_kernel<T>);
    case K_GEN_SHIFT: GO(generic_shift_kernel<T>);
    default: return 1;
  }
#undef GO
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
template <>
int ilqr_generic_launch<double>(hipStream_t stream, const RouteStep& st, const IlqrGenArgs<double>& a) { return gen_launch<double>(stream, st, a); }
template <>
int ilqr_generic_launch<float>(hipStream_t stream, const RouteStep& st, const IlqrGenArgs<float>& a) { return gen_launch<float>(stream, st, a); }

}  // namespace altro_hip
