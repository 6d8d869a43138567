// sweep_route.h -- which instantiation of plan GENERIC's TVLQR sweep kernels (kernels/tvlqr_generic.hip) a launch takes: the size of
// the backward kernel's carve, the choice {blocks in LDS, "late Q", work block in global memory} and the staged / unstaged choice of the
// forward kernel.  The one place that decides: launch_backward / launch_forward (capi_tvlqr.hip) and the single-problem drop-in
// (tvlqr_dropin.hip) both ask here, and altro_hip_sweep_variant reports what the last launch was given.  Host code, no HIP includes:
// tests/cpp/sweep_route_test.cpp checks it with g++ against rows written out by hand.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "altro_hip/altro_hip.h"

namespace altro_hip {

constexpr size_t kGenericLdsLimit = 64 * 1024;   // dynamic LDS a launch gets without asking for more; beyond it plan GENERIC works in global memory
constexpr size_t kGenericForwardStageLimit = 10 * 1024;   // batched forward sweep: stage the knot point in LDS up to this much per problem (sixteen waves per CU)
constexpr size_t kGenericCuLds = 160 * 1024;     // LDS of one compute unit
constexpr int kGenericCuWaves = 16;              // generic_backward_kernel's waves per compute unit by registers (four per SIMD)
constexpr int kGenericCus = 256;                 // compute units the occupancy rule counts on

// bytes of generic_backward_kernel's carve (its blocks in LDS, or the per-problem work block in global memory); late_q: the form
// without a block for Qxx, 3 n^2 instead of 4 n^2 elements
inline size_t generic_backward_lds_bytes(int nm, int mm, size_t esz, bool late_q = false) {
  size_t el = (size_t)(late_q ? 3 : 4) * nm * nm + (size_t)4 * nm * mm + (size_t)2 * mm * mm + (size_t)5 * nm + (size_t)3 * mm;   // (the carve of generic_backward_kernel)
  return el * esz + 64;
}

// bytes of generic_forward_kernel<T, STAGE = true>'s carve
inline size_t generic_forward_lds_bytes(int nm, int mm, int want_y, size_t esz) {
  size_t el = (size_t)3 * nm + mm + (size_t)nm * nm + (size_t)2 * nm * mm + nm + mm + (want_y ? (size_t)nm * nm + nm : 0);
  return el * esz + 64;
}

// problems of one compute unit at `lds` bytes each
inline int generic_backward_per_cu(size_t lds) { return (int)std::min<size_t>(kGenericCuWaves, kGenericCuLds / std::max<size_t>(lds, 1)); }

struct GenericBackwardRoute {
  bool late_q;    // generic_backward_kernel<.., LQ = true>
  bool big;       // generic_backward_kernel<T, BIG = true>: the carve is a work block in global memory
  size_t bytes;   // the carve: dynamic LDS of the launch, or (rounded up to 16) the work block of one problem
  int variant() const { return (late_q ? ALTRO_HIP_SWEEP_LATE_Q : 0) | (big ? ALTRO_HIP_SWEEP_GLOBAL_WORKSPACE : 0); }
};

// The knot point's blocks in LDS while they fit; late Q where that keeps more problems on a compute unit than the batch otherwise
// gets, or keeps the blocks in LDS at all; past that the same kernel on a per-problem work block in global memory (n, m beyond ~37 in
// fp64).  ALTRO_HIP_FORM_GENERIC_LATE_Q_ON: late Q wherever its carve fits; _OFF: never (the two together are refused by
// altro_hip_set_forms; a solve whose options add the second bit gets _ON).  The drop-in asks with batch = 1 and no forms.
inline GenericBackwardRoute generic_backward_route(int nmax, int mmax, size_t esz, int64_t batch, unsigned forms) {
  const size_t lds4 = generic_backward_lds_bytes(nmax, mmax, esz), lds3 = generic_backward_lds_bytes(nmax, mmax, esz, true);
  bool late_q = lds4 > kGenericLdsLimit ? lds3 <= kGenericLdsLimit
                                        : (generic_backward_per_cu(lds3) > generic_backward_per_cu(lds4) &&
                                           batch > (int64_t)kGenericCus * generic_backward_per_cu(lds4));
  if (forms & ALTRO_HIP_FORM_GENERIC_LATE_Q_ON) late_q = lds3 <= kGenericLdsLimit;
  else if (forms & ALTRO_HIP_FORM_GENERIC_LATE_Q_OFF) late_q = false;
  const size_t bytes = late_q ? lds3 : lds4;
  return {late_q, bytes > kGenericLdsLimit, bytes};
}

struct GenericForwardRoute {
  bool staged;    // generic_forward_kernel<T, STAGE = true>
  size_t bytes;   // dynamic LDS of the launch
  int variant() const { return staged ? ALTRO_HIP_SWEEP_FORWARD_STAGED : 0; }
};

// The knot point's blocks staged in LDS up to `limit` bytes per problem (kGenericForwardStageLimit for a batch, kGenericLdsLimit for
// the drop-in's single problem); else the rows from global memory and x, u, x+ alone in LDS.
inline GenericForwardRoute generic_forward_route(int nmax, int mmax, int want_y, size_t esz, size_t limit) {
  const size_t staged = generic_forward_lds_bytes(nmax, mmax, want_y, esz);
  if (staged <= limit) return {true, staged};
  return {false, (size_t)(2 * nmax + mmax) * esz + 64};
}

}  // namespace altro_hip
