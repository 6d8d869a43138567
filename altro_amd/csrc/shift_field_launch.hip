// Kernel instantiations and the launcher of kernels/shift_field.hip: one field of the problem data moved one knot point forward in place,
// on both element types, by 16-byte accesses where the field allows them.  The field arrives as shift_fields.h describes it, so there is
// no plan switch here, and it is no operation of the iLQR loop's route table.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels/shift_field.hip"
#include "shift_fields.h"

namespace altro_hip {

template <typename T, int VEC>
static int field_launch(hipStream_t stream, T* base, const capi::ShiftRun& r) {
  const int64_t runv = r.run / VEC, cols = r.rows * runv;
  const int64_t blocks = (cols + SHIFT_FIELD_BLOCK - 1) / SHIFT_FIELD_BLOCK;
  if (blocks > 0x7fffffff) return 1;
  constexpr int DEPTH = VEC > 1 ? SHIFT_FIELD_DEPTH_VEC : SHIFT_FIELD_DEPTH;
  hipLaunchKernelGGL((shift_field_kernel<T, VEC, DEPTH>), dim3((unsigned)blocks), dim3(SHIFT_FIELD_BLOCK), 0, stream, base + r.first, cols, runv,
                     r.rs / VEC, r.ks / VEC, r.K);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
// buf: the field's buffer, in the handle's element type.  0 ok (fewer than two knot points: nothing to move), 1 the description does not
// pass shift_run_safe, 2 launch failed
int shift_field_launch(hipStream_t stream, void* buf, int esz, const capi::ShiftRun& r) {
  if (!r.ok || (r.vec != 1 && r.vec != 16 / esz)) return 1;
  if (r.K < 2) return 0;
  if (esz == 8) return r.vec == 2 ? field_launch<double, 2>(stream, (double*)buf, r) : field_launch<double, 1>(stream, (double*)buf, r);
  return r.vec == 4 ? field_launch<float, 4>(stream, (float*)buf, r) : field_launch<float, 1>(stream, (float*)buf, r);
}

}  // namespace altro_hip
