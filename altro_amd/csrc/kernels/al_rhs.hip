// al_rhs.hip -- right-hand sides of linear constraint blocks written in place (altro_hip_set_constraint_rhs) and moved one knot point
// forward (altro_hip_shift_constraint_rhs), on every plan and both element types: a block's segment of the g pool is [K][p] shared by
// the batch or [K][p][batch] (al_types.h: al_g_index), K = 1 for a block without ALTRO_HIP_RHS_PER_KNOT.  The caller's array is the
// reference layout [nb][nk][p] in fp64; no kernel of the iLQR loop knows of any of this -- they read a knot point's run through
// AlKnot::g_off.
#pragma once
#include <hip/hip_runtime.h>

#include "al_types.h"

namespace altro_hip {

constexpr int AL_RHS_TB = 64;        // problems of one tile: a wave stores one run dst[c][b0 .. b0 + 63]
constexpr int AL_RHS_TC = 32;        // columns (knot point, row) of one tile: 256 B of one problem's fp64 run
constexpr int AL_RHS_PITCH = AL_RHS_TB + 1;   // doubles: a wave writing 32 columns of one problem strides 130 banks = 2 mod 64, no conflict
constexpr int AL_RHS_BLOCK = 256;
constexpr int AL_RHS_SHIFT_BLOCK = 64;
constexpr int AL_RHS_SHIFT_DEPTH = 16;   // knot points whose values a lane holds before it stores them (kernels/al_shift.hip)

// Per-problem right-hand sides: src is a batch x C matrix (C = nk * p columns, a problem's run contiguous), dst its transpose
// dst[c][batch] in T.  One workgroup moves a tile of AL_RHS_TB problems x AL_RHS_TC columns through LDS: 32 lanes read one problem's
// 256-byte run (VEC2: 16 lanes, 16 bytes each; needs C even and src 16-byte aligned), 64 lanes store one column's run of 64 problems.
// Tiles at the end of the batch and of the columns are partial: nothing outside [0, batch) x [0, C) is read or written.
template <typename T, bool VEC2>
__global__ __launch_bounds__(AL_RHS_BLOCK) void al_rhs_scatter_kernel(T* __restrict__ dst, const double* __restrict__ src, int C, int batch) {
  __shared__ double tile[AL_RHS_TC * AL_RHS_PITCH];
  const int b0 = blockIdx.x * AL_RHS_TB, c0 = blockIdx.y * AL_RHS_TC;
  const int tid = threadIdx.x;
  if (VEC2) {
#pragma unroll
    for (int i = 0; i < AL_RHS_TB * AL_RHS_TC / 2 / AL_RHS_BLOCK; ++i) {
      const int idx = i * AL_RHS_BLOCK + tid, r = idx / (AL_RHS_TC / 2), c = 2 * (idx % (AL_RHS_TC / 2));
      if (b0 + r < batch && c0 + c < C) {   // (C even: c0 + c + 1 < C too)
        const double2 v = *(const double2*)(src + (int64_t)(b0 + r) * C + c0 + c);
        tile[c * AL_RHS_PITCH + r] = v.x;
        tile[(c + 1) * AL_RHS_PITCH + r] = v.y;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < AL_RHS_TB * AL_RHS_TC / AL_RHS_BLOCK; ++i) {
      const int idx = i * AL_RHS_BLOCK + tid, r = idx / AL_RHS_TC, c = idx % AL_RHS_TC;
      if (b0 + r < batch && c0 + c < C) tile[c * AL_RHS_PITCH + r] = src[(int64_t)(b0 + r) * C + c0 + c];
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < AL_RHS_TB * AL_RHS_TC / AL_RHS_BLOCK; ++i) {
    const int idx = i * AL_RHS_BLOCK + tid, c = idx / AL_RHS_TB, r = idx % AL_RHS_TB;
    if (b0 + r < batch && c0 + c < C) dst[(int64_t)(c0 + c) * batch + b0 + r] = (T)tile[c * AL_RHS_PITCH + r];
  }
}

// The direct form: one lane per problem reads its own run of AL_RHS_TC columns (blockIdx.y picks them) and stores column by column, a
// wave's 64 problems one coalesced run each.  The reads of a wave touch 64 cache lines at a time and come back to each of them: fine
// while those lines stay in L1.
template <typename T>
__global__ __launch_bounds__(AL_RHS_TB) void al_rhs_scatter_direct_kernel(T* __restrict__ dst, const double* __restrict__ src, int C, int batch) {
  const int b = blockIdx.x * AL_RHS_TB + threadIdx.x, c0 = blockIdx.y * AL_RHS_TC;
  if (b >= batch) return;
  const double* run = src + (int64_t)b * C;
#pragma unroll 8
  for (int c = c0; c < c0 + AL_RHS_TC && c < C; ++c) dst[(int64_t)c * batch + b] = (T)run[c];
}

// A shared right-hand side: a converting copy of `count` elements.
template <typename T>
__global__ void al_rhs_copy_kernel(T* __restrict__ dst, const double* __restrict__ src, int count) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x) dst[i] = (T)src[i];
}

// The shift of one block's segment g[K][stride] (stride = p * batch, or p for a shared block): one lane owns one (row, problem) and
// walks k ascending IN PLACE, g[k] = g[k + 1]; the last knot point keeps its values.  As in al_shift_duals_kernel the values of DEPTH
// knot points are loaded before any is stored, and those of the following group before this group's stores -- the rows a group
// stores to lie before every row the next one loads.  Loads past the end read knot point K - 1 again (never stored to) and are dropped.
template <typename T, int DEPTH>
__global__ __launch_bounds__(AL_RHS_SHIFT_BLOCK) void al_rhs_shift_kernel(T* g, int K, int64_t stride) {
  const int64_t e = (int64_t)blockIdx.x * AL_RHS_SHIFT_BLOCK + threadIdx.x;
  if (e >= stride) return;
  T* col = g + e;
  const int last = K - 1;
  T v[DEPTH];
#pragma unroll
  for (int i = 0; i < DEPTH; ++i) v[i] = col[(int64_t)min(i + 1, last) * stride];
  for (int k0 = 0; k0 < last; k0 += DEPTH) {
    T ahead[DEPTH];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) ahead[i] = col[(int64_t)min(k0 + DEPTH + i + 1, last) * stride];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i)
      if (k0 + i < last) col[(int64_t)(k0 + i) * stride] = v[i];
#pragma unroll
    for (int i = 0; i < DEPTH; ++i) v[i] = ahead[i];
  }
}

}  // namespace altro_hip
