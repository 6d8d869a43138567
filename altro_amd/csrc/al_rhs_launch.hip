// Kernel instantiations and launchers of kernels/al_rhs.hip: a constraint block's right-hand side written in place and shifted, on both
// element types.  They serve every plan alike (one g pool, al_types.h: al_g_index), so they are no operation of the iLQR loop's route table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels/al_rhs.hip"

namespace altro_hip {

// form: 0 the LDS tile (the default: tools/rhs_update_bench measures both), 1 the direct form.  0 ok, 2 launch failed
template <typename T>
static int scatter_launch(hipStream_t stream, T* dst, const double* src, int C, int nb, int batch, int form) {
  if (C <= 0 || batch <= 0) return 0;
  if (nb == 1) {   // shared by the batch: [C] -> [C]
    hipLaunchKernelGGL((al_rhs_copy_kernel<T>), dim3(std::min((C + 255) / 256, 1024)), dim3(256), 0, stream, dst, src, C);
  } else {
    const dim3 grid((batch + AL_RHS_TB - 1) / AL_RHS_TB, (C + AL_RHS_TC - 1) / AL_RHS_TC);
    if (form == 1) hipLaunchKernelGGL((al_rhs_scatter_direct_kernel<T>), grid, dim3(AL_RHS_TB), 0, stream, dst, src, C, batch);
    else if (C % 2 == 0 && ((uintptr_t)src & 15) == 0) hipLaunchKernelGGL((al_rhs_scatter_kernel<T, true>), grid, dim3(AL_RHS_BLOCK), 0, stream, dst, src, C, batch);
    else hipLaunchKernelGGL((al_rhs_scatter_kernel<T, false>), grid, dim3(AL_RHS_BLOCK), 0, stream, dst, src, C, batch);
  }
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
// dst: the first element of the range's first knot point in the block's segment; src: fp64 [nb][C] on the device, C = nk * p
int al_rhs_scatter_launch(hipStream_t stream, void* dst, int esz, const double* src, int C, int nb, int batch, int form) {
  return esz == 8 ? scatter_launch(stream, (double*)dst, src, C, nb, batch, form) : scatter_launch(stream, (float*)dst, src, C, nb, batch, form);
}

template <typename T>
static int rhs_shift_launch(hipStream_t stream, T* g, int K, int64_t stride) {
  if (K < 2 || stride <= 0) return 0;
  hipLaunchKernelGGL((al_rhs_shift_kernel<T, AL_RHS_SHIFT_DEPTH>), dim3((unsigned)((stride + AL_RHS_SHIFT_BLOCK - 1) / AL_RHS_SHIFT_BLOCK)), dim3(AL_RHS_SHIFT_BLOCK), 0,
                     stream, g, K, stride);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
// g: a block's segment [K][stride] (stride = p * batch per problem, p shared)
int al_rhs_shift_launch(hipStream_t stream, void* g, int esz, int K, int64_t stride) {
  return esz == 8 ? rhs_shift_launch(stream, (double*)g, K, stride) : rhs_shift_launch(stream, (float*)g, K, stride);
}

}  // namespace altro_hip
