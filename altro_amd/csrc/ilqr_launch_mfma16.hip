// Kernel instantiations of the iLQR loop for plan MFMA16 (see kernels/ilqr_mfma16.hip, kernels/ilqr_types.h): dynamics as data, at most
// AL_MAXC constraint slots per knot point.  Which of them runs, and with which grid: loop_route.h.
#include <hip/hip_runtime.h>

#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

#define GO(...) hipLaunchKernelGGL((__VA_ARGS__), grid, block, st.lds, stream, a); break
// wave_merit_dpp_kernel<S, AL, DUAL, DENSE, model, SOC, AFF>: the cone's code for handles that have one, and without blocks
#define MERIT(DUAL_, DENSE_, AFF_)                                                                                              \
  case merit_id(true, DUAL_, DENSE_, false, AFF_): GO(wave_merit_dpp_kernel<S, true, DUAL_, DENSE_, 0, false, AFF_>);           \
  case merit_id(true, DUAL_, DENSE_, true, AFF_): GO(wave_merit_dpp_kernel<S, true, DUAL_, DENSE_, 0, true, AFF_>);             \
  case merit_id(false, DUAL_, DENSE_, true, AFF_): GO(wave_merit_dpp_kernel<S, false, DUAL_, DENSE_, 0, true, AFF_>)

template <typename S>
static int wave_launch(hipStream_t stream, const RouteStep& st, const IlqrWaveArgs<S>& a) {
  const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
  if constexpr (sizeof(S) == 8) {   // affine trials: fp64 records
    if ((st.id & KF_AFF) || st.id == K_WAVE_AFF_REDUCE) {
      switch (st.id) {
        MERIT(false, false, true);
        MERIT(false, true, true);
        case K_WAVE_AFF_REDUCE: hipLaunchKernelGGL(wave_aff_reduce_kernel<S>, grid, block, 0, stream, a, st.chunks); break;
        default: return 1;
      }
      return hipGetLastError() == hipSuccess ? 0 : 2;
    }
  }
  switch (st.id) {
    case K_WAVE_ROLLOUT: GO(wave_rollout_kernel<S>);
    case K_WAVE_ACCEPT: GO(wave_accept_kernel<S>);
    case K_WAVE_EXPAND_DPP | KF_DENSE: GO(wave_expand_dpp_kernel<S, true>);
    case K_WAVE_EXPAND_DPP | KF_ALLSEL: GO(wave_expand_dpp_kernel<S, false, true>);
    case K_WAVE_EXPAND_DPP: GO(wave_expand_dpp_kernel<S, false>);
    case K_WAVE_EXPAND_LDS: GO(wave_expand_kernel<S>);
    case K_WAVE_EXPAND_GRAD | KF_DENSE: GO(wave_expand_grad_dense_kernel<S>);
    case K_WAVE_EXPAND_GRAD: GO(wave_expand_grad_kernel<S>);
    case K_WAVE_DUAL_DPP: GO(wave_dual_update_dpp_kernel<S>);
    case K_WAVE_DUAL_LDS: GO(wave_dual_update_kernel<S>);
    MERIT(false, false, false);
    MERIT(false, true, false);
    MERIT(true, false, false);
    MERIT(true, true, false);
    case K_WAVE_MERIT_LDS | KF_AL: GO(wave_merit_kernel<S, true>);
    case K_WAVE_MERIT_LDS: GO(wave_merit_kernel<S, false>);
    case K_WAVE_SPEC_SELECT: GO(wave_spec_select_kernel<S>);
    case K_WAVE_STATIONARITY: GO(wave_stationarity_kernel<S>);
    case K_WAVE_FEAS_DPP: GO(wave_feasibility_dpp_kernel<S>);
    case K_WAVE_SHIFT: GO(wave_shift_kernel<S>);
    default: return 1;
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
#undef MERIT
#undef GO
template <>
int ilqr_wave_launch_kernel<double>(hipStream_t stream, const RouteStep& st, const IlqrWaveArgs<double>& a) { return wave_launch<double>(stream, st, a); }
template <>
int ilqr_wave_launch_kernel<float>(hipStream_t stream, const RouteStep& st, const IlqrWaveArgs<float>& a) { return wave_launch<float>(stream, st, a); }

}  // namespace altro_hip
