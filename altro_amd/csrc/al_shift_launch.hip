// Kernel instantiations and launchers of kernels/al_shift.hip: the duals' shift on both element types and the penalty setter / getter.
// They serve every plan alike (one dual array z[rows][batch], al_shift.h), so they are no operation of the iLQR loop's route table.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels/al_shift.hip"

namespace altro_hip {

// 0 ok, 2 launch failed
template <typename T>
static int shift_launch(hipStream_t stream, T* z, const int* order, const int* start, int nchains, int batch, int tail) {
  if (nchains <= 0 || batch <= 0) return 0;
  const dim3 grid((batch + AL_SHIFT_BLOCK - 1) / AL_SHIFT_BLOCK, std::min(nchains, 65535));
  hipLaunchKernelGGL((al_shift_duals_kernel<T, AL_SHIFT_DEPTH>), grid, dim3(AL_SHIFT_BLOCK), 0, stream, z, order, start, nchains, batch, tail);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
int al_shift_duals_launch(hipStream_t stream, void* z, int esz, const int* order, const int* start, int nchains, int batch, int tail) {
  return esz == 8 ? shift_launch(stream, (double*)z, order, start, nchains, batch, tail) : shift_launch(stream, (float*)z, order, start, nchains, batch, tail);
}
int al_set_penalty_launch(hipStream_t stream, IlqrProb* prob, const double* rho, int stride, int batch) {
  hipLaunchKernelGGL(al_set_penalty_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, prob, rho, stride, batch);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
int al_get_penalty_launch(hipStream_t stream, const IlqrProb* prob, double* rho, int batch) {
  hipLaunchKernelGGL(al_get_penalty_kernel, dim3((batch + 255) / 256), dim3(256), 0, stream, prob, rho, batch);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace altro_hip
