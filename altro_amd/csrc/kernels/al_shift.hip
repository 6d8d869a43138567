// al_shift.hip -- the duals' receding-horizon shift (altro_hip_shift_duals) and the per-problem penalty setter / getter, on every plan:
// the duals of a handle are z[rows][batch] in the handle's element type, and al_shift.h gives the chains of rows that hold the same
// (block definition, row in block) at consecutive knot points, each written out in walking order (order[], start[]).
#pragma once
#include <hip/hip_runtime.h>

#include "al_types.h"
#include "ilqr_types.h"

namespace altro_hip {

constexpr int AL_SHIFT_BLOCK = 64;    // one wave per workgroup: 64 consecutive problems of one chain
constexpr int AL_SHIFT_DEPTH = 16;    // links whose values a lane holds in registers before it stores them (at most 32: AL_SHIFT_PAD)

// One lane = one (chain, problem): blockIdx.y picks the chain, consecutive lanes take consecutive problems, so every access is one
// coalesced run z[row][b .. b + 63].  The lane walks its chain in ascending k IN PLACE, z[order[i]] = z[order[i + 1]]: it owns the chain,
// and order[i + 1] > order[i] (al_shift.h asserts it), so a row is read before it is overwritten.  The chain index is uniform over the
// wave: the rows come from the constant address space as runs of order[] (wide s_loads into scalar registers, no load depends on
// another), and no lane diverges but those past the batch.
// The values of DEPTH links are loaded before any is stored, and those of the FOLLOWING group before this group's stores (the rows a
// group stores to lie before every row the next one loads): a horizon of 256 knot points is 16 overlapped round trips to HBM, not 256.
// There is no branch between loads: past a chain's end they read the rows that follow in order[] (its zero padding at the very end) and
// the values are dropped.
// tail: what the last row of a chain becomes -- ALTRO_HIP_DUAL_TAIL_KEEP (0) nothing, ALTRO_HIP_DUAL_TAIL_ZERO (1) zero.
template <typename T, int DEPTH>
__global__ __launch_bounds__(AL_SHIFT_BLOCK) void al_shift_duals_kernel(T* __restrict__ z, const int* __restrict__ order_, const int* __restrict__ start_,
                                                                        int nchains, int batch, int tail) {
  const int b = blockIdx.x * AL_SHIFT_BLOCK + threadIdx.x;
  if (b >= batch) return;
  const int ALTRO_CONST_AS* order = (const int ALTRO_CONST_AS*)order_;
  const int ALTRO_CONST_AS* start = (const int ALTRO_CONST_AS*)start_;
  const int64_t B = batch;
  for (int c = blockIdx.y; c < nchains; c += gridDim.y) {
    const int base = start[c], len = start[c + 1] - base;
    // group i0: v[i] = old z[order[base + i0 + i + 1]], to be stored to z[order[base + i0 + i]]
    T v[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) v[i] = z[(int64_t)order[base + i + 1] * B + b];
    for (int i0 = 0; i0 < len; i0 += DEPTH) {
      T ahead[DEPTH];
#pragma unroll
      for (int i = 0; i < DEPTH; ++i) ahead[i] = z[(int64_t)order[base + i0 + DEPTH + i + 1] * B + b];
#pragma unroll
      for (int i = 0; i < DEPTH; ++i) {
        const int at = i0 + i;
        if (at + 1 < len) z[(int64_t)order[base + at] * B + b] = v[i];
        else if (at + 1 == len && tail) z[(int64_t)order[base + at] * B + b] = T(0);   // the chain's last row
      }
#pragma unroll
      for (int i = 0; i < DEPTH; ++i) v[i] = ahead[i];
    }
  }
}

// rho[b * stride] (stride 0: one value for all) into IlqrProb::rho and ::rho_est, as altro_hip_reset_duals sets them; nothing else moves
__global__ void al_set_penalty_kernel(IlqrProb* __restrict__ prob, const double* __restrict__ rho, int stride, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const double r = rho[(int64_t)b * stride];
  prob[b].rho = r;
  prob[b].rho_est = r;
}
__global__ void al_get_penalty_kernel(const IlqrProb* __restrict__ prob, double* __restrict__ rho, int batch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < batch) rho[b] = prob[b].rho;
}

}  // namespace altro_hip
