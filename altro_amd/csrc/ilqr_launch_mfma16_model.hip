// Kernel instantiations of plan MFMA16's iLQR loop for NONLINEAR device models (kernels/ilqr_tile_model.hip and the MK
// instantiations of wave_merit_dpp_kernel): a translation unit of their own so that they compile next to the data-dynamics ones.
#include <hip/hip_runtime.h>

#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

#define TILE_MODELS(X) X(MODEL_QUADROTOR)

bool ilqr_tile_model_supported(int kind, int n, int m) {
#define X(K_) if (kind == K_ && n == 12 && m == 4) return true;
  TILE_MODELS(X)
#undef X
  return false;
}

template <>
int ilqr_wave_launch_model<double>(hipStream_t stream, const RouteStep& st, const IlqrWaveArgs<double>& a) {
  using S = double;
  const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
  bool done = false;
#define GO(...) hipLaunchKernelGGL((__VA_ARGS__), grid, block, st.lds, stream, a); break
#define MERIT(K_, AL_, DUAL_, DENSE_) case merit_id(AL_, DUAL_, DENSE_, true, false, KF_MODEL): GO(wave_merit_dpp_kernel<S, AL_, DUAL_, DENSE_, K_>)
#define X(K_)                                                                             \
  if (!done && a.mp.kind == K_) {                                                         \
    done = true;                                                                          \
    switch (st.id) {                                                                      \
      case K_WAVE_ROLLOUT | KF_MODEL: GO(wave_rollout_model_kernel<S, K_>);               \
      case K_WAVE_EXPAND_DYN | KF_MODEL: GO(wave_expand_dyn_kernel<S, K_>);               \
      MERIT(K_, true, false, true); MERIT(K_, false, false, true); MERIT(K_, true, false, false); MERIT(K_, false, false, false); \
      MERIT(K_, true, true, true); MERIT(K_, false, true, true); MERIT(K_, true, true, false); MERIT(K_, false, true, false);     \
      default: return 1;                                                                  \
    }                                                                                     \
  }
  TILE_MODELS(X)
#undef X
#undef MERIT
#undef GO
  if (!done) return 1;
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
template <>
int ilqr_wave_launch_model<float>(hipStream_t, const RouteStep&, const IlqrWaveArgs<float>&) { return 1; }   // (fp64 records only)

}  // namespace altro_hip
