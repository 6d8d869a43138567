// Kernel instantiations of plan MFMA16's merit and expansion passes for handles with more than AL_MAXC constraint slots at a knot
// point (kernels/al_types.h: AL_TILE_MAXC slots of AL_MAXP rows -- an input box AND a state box on a (12, 4) problem): the
// NC = AL_TILE_MAXC instantiations of wave_merit_dpp_kernel and wave_expand_dpp_kernel.  A translation unit of their own: the two-slot
// kernels of ilqr_launch_mfma16.hip stay what they were, register for register.  (What keeps the six-slot merit kernel at two waves
// per SIMD without spills -- 251 registers -- is in kernels/ilqr_merit2_dpp.hip: one set of (z, g) registers, asked for after use,
// and the gradient's column sums taken with the rows.  Before those two changes: one wave per SIMD or 64-114 spilled registers,
// the two-trial pass of C1 + input box + state box 2.4-2.5 ms; a four-slot instantiation 1.04 ms)
#include <hip/hip_runtime.h>

#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
#include "loop_route.h"

namespace altro_hip {

using namespace capi;

#define WIDE_MODELS(X) X(MODEL_QUADROTOR)

template <>
int ilqr_wave_launch_wide<double>(hipStream_t stream, const RouteStep& st, const IlqrWaveArgs<double>& a) {
  using S = double;
  constexpr int W = AL_TILE_MAXC;
  const dim3 grid(st.gx, st.gy, st.gz), block(st.block);
#define GO(...) hipLaunchKernelGGL((__VA_ARGS__), grid, block, st.lds, stream, a); break
  if (st.id & KF_MODEL) {
    bool done = false;
#define MERIT(K_, DUAL_, DENSE_) case merit_id(true, DUAL_, DENSE_, true, false, KF_MODEL | KF_WIDE): GO(wave_merit_dpp_kernel<S, true, DUAL_, DENSE_, K_, true, false, W>)
#define X(K_)                                                                                                           \
    if (!done && a.mp.kind == K_) {                                                                                     \
      done = true;                                                                                                      \
      switch (st.id) {                                                                                                  \
        MERIT(K_, false, true); MERIT(K_, false, false); MERIT(K_, true, true); MERIT(K_, true, false);                 \
        default: return 1;                                                                                              \
      }                                                                                                                 \
    }
    WIDE_MODELS(X)
#undef X
#undef MERIT
    if (!done) return 1;
    return hipGetLastError() == hipSuccess ? 0 : 2;
  }
  // (SOC_: the second-order cone's code only for handles that have one -- it costs the kernel ~20 registers)
#define MERIT(DUAL_, DENSE_, AFF_)                                                                                                                   \
  case merit_id(true, DUAL_, DENSE_, true, AFF_, KF_WIDE): GO(wave_merit_dpp_kernel<S, true, DUAL_, DENSE_, 0, true, AFF_, W>);                      \
  case merit_id(true, DUAL_, DENSE_, false, AFF_, KF_WIDE): GO(wave_merit_dpp_kernel<S, true, DUAL_, DENSE_, 0, false, AFF_, W>)
  switch (st.id) {
    case K_WAVE_EXPAND_DPP | KF_WIDE | KF_DENSE: GO(wave_expand_dpp_kernel<S, true, false, W>);
    case K_WAVE_EXPAND_DPP | KF_WIDE | KF_ALLSEL: GO(wave_expand_dpp_kernel<S, false, true, W>);
    case K_WAVE_EXPAND_DPP | KF_WIDE: GO(wave_expand_dpp_kernel<S, false, false, W>);
    MERIT(false, true, true); MERIT(false, false, true);
    case K_WAVE_AFF_REDUCE | KF_WIDE: hipLaunchKernelGGL(wave_aff_reduce_kernel<S>, grid, block, 0, stream, a, st.chunks); break;
    MERIT(false, true, false); MERIT(false, false, false);
    MERIT(true, true, false); MERIT(true, false, false);
    default: return 1;
  }
#undef MERIT
#undef GO
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
// (fp32 records: the wide form is not instantiated -- altro_hip_add_linear_constraint says so when a block would need it)
template <>
int ilqr_wave_launch_wide<float>(hipStream_t, const RouteStep&, const IlqrWaveArgs<float>&) { return 1; }

}  // namespace altro_hip
