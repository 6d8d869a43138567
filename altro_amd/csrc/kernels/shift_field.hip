// shift_field.hip -- one field of the problem data moved one knot point forward IN PLACE (altro_hip_shift_dynamics,
// altro_hip_shift_linear_costs), on every plan and both element types.  The field comes as shift_fields.h describes it (ShiftRun):
// element e < run of row r < rows at knot point k is base[r * rs + k * ks + e]; knot points 0 .. K-2 take what k + 1 held, K-1 keeps
// its values.  No kernel of the sweeps or of the iLQR loop knows of this: they index the same records by k afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace altro_hip {

constexpr int SHIFT_FIELD_BLOCK = 64;    // one wave per workgroup: 64 consecutive accesses of one row
// knot points whose values a lane holds before it stores them (kernels/al_shift.hip): 16 of one element, 8 of 16 bytes -- two groups
// of 8 x 16 bytes are 64 registers; at 16 the kernel would hold 128 and run at less than half the waves per SIMD
constexpr int SHIFT_FIELD_DEPTH = 16, SHIFT_FIELD_DEPTH_VEC = 8;

// VEC elements of T as one access: 16 bytes for (double, 2) and (float, 4).  The compiler's own vector types: arrays of them stay in
// registers (arrays of HIP's double2 / float4 structs went to scratch memory here: 528 bytes per lane, 2.3 x the copy's time).
template <typename T, int VEC> struct ShiftAccess { typedef T type; };
template <> struct ShiftAccess<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct ShiftAccess<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };

// One lane owns one column -- access a of row r, a < runv = run / VEC -- and walks k ascending: col[k] = col[k + 1].  Consecutive lanes
// take consecutive accesses of a row (elements of a record; problems of a LANE row), so a wave's load or store is one contiguous run.
// The host has checked (shift_run_safe) that (row, k, element) -> address is one to one over the walk: a lane reads only what it alone
// writes, and reads k + 1 before it writes k, so there is no fence and no second buffer.  As in al_shift_duals_kernel the values of DEPTH
// knot points are loaded before any is stored, and those of the FOLLOWING group before this group's stores (a group stores below
// everything the next one loads): a horizon of 256 is 16 or 32 overlapped round trips, not 256.  Loads past the end of the walk read knot
// point K - 1 again (inside the buffer, never stored to) and the values are dropped.
// rs, ks: in accesses (the host divided them by VEC).
template <typename T, int VEC, int DEPTH>
__global__ __launch_bounds__(SHIFT_FIELD_BLOCK) void shift_field_kernel(T* base, int64_t cols, int64_t runv, int64_t rs, int64_t ks, int K) {
  typedef typename ShiftAccess<T, VEC>::type V;
  const int64_t t = (int64_t)blockIdx.x * SHIFT_FIELD_BLOCK + threadIdx.x;
  if (t >= cols) return;
  const int64_t r = t / runv, a = t - r * runv;
  V* col = (V*)base + r * rs + a;
  const int last = K - 1;
  V v[DEPTH];
#pragma unroll
  for (int i = 0; i < DEPTH; ++i) v[i] = col[(int64_t)min(i + 1, last) * ks];
  for (int k0 = 0; k0 < last; k0 += DEPTH) {
    V ahead[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) ahead[i] = col[(int64_t)min(k0 + DEPTH + i + 1, last) * ks];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i)
      if (k0 + i < last) col[(int64_t)(k0 + i) * ks] = v[i];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) v[i] = ahead[i];
  }
}

}  // namespace altro_hip
