// capi_tvlqr.hip -- C ABI: the TVLQR sweep (altro_hip_backward / forward_ltv / sweep) and its per-plan kernel launchers.
// This unit instantiates the sweep kernels of all three plans (GENERIC, LANE, MFMA16 in fp64 / fp32 storage / pure fp32).
#include "capi_internal.h"
#include "models.h"

#include "kernels/tvlqr_mfma16.hip"
#include "kernels/tvlqr_mfma16_f32.hip"
#include "kernels/tvlqr_mfma16_f32x4.hip"
#include "kernels/tvlqr_mfma16_fwd_f32x4.hip"
#include "kernels/tvlqr_mfma16_fwd_group.hip"
#include "kernels/tvlqr_mfma16_bwd_group.hip"

using namespace altro_hip;
using namespace altro_hip::capi;

namespace {

template <typename T>
int lane_sweep(altro_hip_batch* h, const SweepRoute& rt, bool backward, double reg, const BackwardMask& pp) {
  LaneArgs<T> a{(const T*)h->l_in, (const T*)h->l_term, (T*)h->l_out, (T*)h->l_outn, (const T*)h->l_x0,
                (T*)h->l_xuy, (T*)h->delta_V, h->status, h->N, h->batch, (T)reg, backward ? pp.active : nullptr,
                backward ? pp.reg_pp : nullptr};
  const dim3 grid(rt.grid), block(rt.block);
  switch (rt.id) {
    case SK_QUAD_FORWARD: PROF_LAUNCH((quad_forward_kernel<2, T>), grid, block, 0, h->stream, a); return 0;
    case SK_QUAD_FORWARD | SF_FUSED: PROF_LAUNCH((quad_forward_kernel_fused<2, T>), grid, block, 0, h->stream, a); return 0;
    case SK_QUAD_BACKWARD: PROF_LAUNCH((quad_backward_kernel<2, T>), grid, block, 0, h->stream, a); return 0;
    case SK_QUAD_BACKWARD | SF_FUSED: PROF_LAUNCH((quad_backward_kernel_fused<2, T>), grid, block, 0, h->stream, a); return 0;
    case SK_QUAD2_BACKWARD: PROF_LAUNCH((quad2_backward_kernel<T>), grid, block, 0, h->stream, a); return 0;
    case SK_QUAD2_BACKWARD | SF_FUSED: PROF_LAUNCH((quad2_backward_kernel_fused<T>), grid, block, 0, h->stream, a); return 0;
    default: break;
  }
#define X(N_, M_)                                                                                                                        \
  if (h->n == N_ && h->m == M_) switch (rt.id) {                                                                                         \
    case SK_LANE_BACKWARD: PROF_LAUNCH((lane_backward_kernel<N_, M_, T>), grid, block, 0, h->stream, a); return 0;                       \
    case SK_LANE_BACKWARD | SF_FUSED: PROF_LAUNCH((lane_backward_kernel_fused<N_, M_, T>), grid, block, 0, h->stream, a); return 0;      \
    case SK_LANE_FORWARD: PROF_LAUNCH((lane_forward_kernel<N_, M_, T>), grid, block, 0, h->stream, a); return 0;                         \
    case SK_LANE_FORWARD | SF_FUSED: PROF_LAUNCH((lane_forward_kernel_fused<N_, M_, T>), grid, block, 0, h->stream, a); return 0;        \
    default: break;                                                                                                                      \
  }
  LANE_SHAPES(X)
#undef X
  return 1;
}

template <typename T>
GenericArgs<T> generic_args(altro_hip_batch* h, double reg, const BackwardMask& pp) {
  GenericArgs<T> a;
  for (int i = 0; i < G_NUM; ++i) {
    a.base[i] = (T*)h->g_arr[i];
    a.bstride[i] = h->g_bstride[i];
  }
  a.off = h->g_off;
  a.nx = h->g_nx;
  a.nu = h->g_nu;
  a.x0 = (const T*)h->x0;
  a.x0_stride = h->n;
  a.delta_V = (T*)h->delta_V;
  a.status = h->status;
  a.N = h->N;
  a.batch = h->batch;
  a.nmax = h->n;
  a.mmax = h->m;
  a.reg = (T)reg;
  a.is_diag = h->is_diag;
  a.store_q = (h->flags & ALTRO_HIP_STORE_QBLOCKS) ? 1 : 0;
  a.want_y = 1;
  a.no_f = h->ilqr_linear ? 1 : 0;
  // A solve with the regularisation schedule on (it alone passes reg_pp): per-problem reg, and only the problems the mask names --
  // the running ones at the head of a sweep, the failed ones in a retry (a problem that succeeded has relaxed its reg already and must
  // not be swept with it).  Any other launch is the one it always was: every problem, including those a solve has stopped.
  if (pp.reg_pp) { a.active = pp.active; a.reg_pp = pp.reg_pp; }
  return a;
}

// plan GENERIC's kernels (also plan MFMA32's backward sweep of a diagonal cost); rt.lds: sweep_route.h
template <typename T>
int generic_sweep(altro_hip_batch* h, const SweepRoute& rt, bool backward, double reg, const BackwardMask& pp) {
  auto a = generic_args<T>(h, reg, pp);
  const dim3 grid(rt.grid), block(rt.block);
  if (backward) {   // the work block of one problem in global memory, where the route says so: allocated on first use
    const size_t ws = (rt.lds + 15) / 16 * 16;
    if ((rt.id & SF_GLOBAL_WS) && !h->g_ws)
      if (int rc = dmalloc(h, &h->g_ws, (size_t)h->batch * ws)) return rc;
    a.ws = (T*)h->g_ws; a.ws_stride = (int64_t)(ws / sizeof(T));
  }
  switch (rt.id) {
    case SK_GENERIC_BACKWARD: PROF_LAUNCH((generic_backward_kernel<T, false>), grid, block, rt.lds, h->stream, a); return 0;
    case SK_GENERIC_BACKWARD | SF_LATE_Q: PROF_LAUNCH((generic_backward_kernel<T, false, false, true>), grid, block, rt.lds, h->stream, a); return 0;
    case SK_GENERIC_BACKWARD | SF_GLOBAL_WS: PROF_LAUNCH((generic_backward_kernel<T, true>), grid, block, 0, h->stream, a); return 0;
    case SK_GENERIC_FORWARD: PROF_LAUNCH((generic_forward_kernel<T, false>), grid, block, rt.lds, h->stream, a); return 0;
    case SK_GENERIC_FORWARD | SF_STAGED: PROF_LAUNCH((generic_forward_kernel<T, true>), grid, block, rt.lds, h->stream, a); return 0;
    default: break;
  }
  if constexpr (sizeof(T) == sizeof(double)) switch (rt.id) {   // the products on the matrix cores (ALTRO_HIP_GENERIC_MATRIX_CORES)
    case SK_GENERIC_BACKWARD | SF_MATRIX_CORES: PROF_LAUNCH((generic_backward_kernel<double, false, true>), grid, block, rt.lds, h->stream, a); return 0;
    case SK_GENERIC_BACKWARD | SF_MATRIX_CORES | SF_LATE_Q: PROF_LAUNCH((generic_backward_kernel<double, false, true, true>), grid, block, rt.lds, h->stream, a); return 0;
    case SK_GENERIC_BACKWARD | SF_MATRIX_CORES | SF_GLOBAL_WS: PROF_LAUNCH((generic_backward_kernel<double, true, true>), grid, block, 0, h->stream, a); return 0;
    default: break;
  }
  return 1;
}

// One profiled kernel launch (altro_hip_profile_enable).  The launch itself carries the two events -- hipExtLaunchKernelGGL
// stamps them from the dispatch's own completion signal -- instead of two hipEventRecord calls around it: those are marker
// packets with barriers on the handle's stream, 15 us per sweep of a timed region whose sweeps take 1.45 ms
// (profiles/r03zc_event_overhead.txt), and they time the packets' turnaround along with the kernel.
struct ProfScope {
  altro_hip_batch* h;
  int slot, idx = -1;
  ProfScope(altro_hip_batch* h_, int slot_) : h(h_), slot(slot_) {
    h->launch_ev0 = nullptr; h->launch_ev1 = nullptr;
    if (h->prof == 1) { h->launch_ev0 = h->ev0; h->launch_ev1 = h->ev1; }
    else if (h->prof == 2) {
      if (2 * (h->prof_n + 1) <= (int)h->prof_ev.size()) {
        idx = h->prof_n++;
        h->prof_slot[idx] = slot;
        h->launch_ev0 = h->prof_ev[2 * idx]; h->launch_ev1 = h->prof_ev[2 * idx + 1];
      } else {
        h->prof_dropped[slot] += 1;   // the ring is full: say so instead of averaging over a silent prefix
      }
    }
  }
  ~ProfScope() {
    if (h->prof == 1 && h->launch_ev1) {
      (void)hipEventSynchronize(h->ev1);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) profile_add(h, slot, ms);
    }
    h->launch_ev0 = nullptr; h->launch_ev1 = nullptr;   // (mode 2: altro_hip_profile_get reads the pairs, no wait here)
  }
};

template <typename S>
Mfma16Args<S> mfma16_args(altro_hip_batch* h, double reg, const BackwardMask& pp) {
  Mfma16Args<S> a;
  a.in = (const S*)h->m_in;
  a.cin = (const S*)h->m_cin;
  a.cin_bs = h->m_st.cin_bs; a.cin_ks = h->m_st.cin_ks;
  a.in_bs = h->m_st.in_bs; a.in_ks = h->m_st.in_ks; a.out_bs = h->m_st.out_bs; a.out_ks = h->m_st.out_ks;
  a.xuy_bs = h->m_st.xuy_bs; a.xuy_ks = h->m_st.xuy_ks;
  a.term = (const S*)h->m_term; a.out = (S*)h->m_out; a.outn = (S*)h->m_outn; a.qblk = (S*)h->m_qblk;
  a.trash = (S*)h->m_trash; a.x0 = (const S*)h->x0; a.xuy = (S*)h->m_xuy; a.delta_V = (S*)h->delta_V;
  a.status = h->status; a.N = h->N; a.batch = h->batch; a.reg = reg; a.has_f = h->has_f && !h->ilqr_linear;
  a.active = pp.active; a.reg_pp = pp.reg_pp;   // (a solve's backward sweep; the forward sweeps pass none)
  return a;
}

// the group kernels' dynamic LDS is more than 64 KB: that has to be asked for, once per device (a handle stays on its own)
int group_lds_ready(bool* ready, std::initializer_list<const void*> kernels, size_t lds, const char* what) {
  for (const void* kernel : kernels) {
    if (*ready) break;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(ALTRO_HIP_ERR_HIP, "%s group kernel: %s", what, hipGetErrorString(e));
  }
  *ready = true;
  return 0;
}

constexpr int kFwdGroupDepth = 2;   // the forward group kernel's register ring, in knot points (sweep_route.h)

template <typename S>
int mfma16_sweep(altro_hip_batch* h, const SweepRoute& rt, double reg, const BackwardMask& pp) {
  const auto a = mfma16_args<S>(h, reg, pp);
  const dim3 grid(rt.grid), block(rt.block);
  switch (rt.id) {
    case SK_MFMA16_BACKWARD: PROF_LAUNCH((mfma16_backward_kernel<false, false, S>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_BACKWARD | SF_HAS_F: PROF_LAUNCH((mfma16_backward_kernel<false, true, S>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_BACKWARD | SF_STORE_Q: PROF_LAUNCH((mfma16_backward_kernel<true, false, S>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_BACKWARD | SF_STORE_Q | SF_HAS_F: PROF_LAUNCH((mfma16_backward_kernel<true, true, S>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_FORWARD: PROF_LAUNCH((mfma16_forward_kernel<S, 3>), grid, block, 0, h->stream, a); return 0;
    default: break;
  }
  if constexpr (sizeof(S) == sizeof(double)) {
    constexpr int G = kSweepGroup;
    const size_t fwd_lds = Mfma16FwdGroup<G>::lds_bytes(kFwdGroupDepth), bwd_lds = Mfma16BwdGroup<G>::lds_bytes();
    if (rt.id == SK_MFMA16_FORWARD_GROUP)
      if (int rc = group_lds_ready(&h->fwd_group_ready, {(const void*)mfma16_forward_group_kernel<double, G, kFwdGroupDepth>}, fwd_lds, "forward")) return rc;
    if ((rt.id & ~SF_MASK) == SK_MFMA16_BACKWARD_GROUP)
      if (int rc = group_lds_ready(&h->bwd_group_ready, {(const void*)mfma16_backward_group_kernel<true, G>, (const void*)mfma16_backward_group_kernel<false, G>}, bwd_lds, "backward")) return rc;
    switch (rt.id) {
      case SK_MFMA16_FORWARD_GROUP: PROF_LAUNCH((mfma16_forward_group_kernel<double, G, kFwdGroupDepth>), grid, block, fwd_lds, h->stream, a); return 0;
      case SK_MFMA16_BACKWARD_GROUP: PROF_LAUNCH((mfma16_backward_group_kernel<false, G>), grid, block, bwd_lds, h->stream, a); return 0;
      case SK_MFMA16_BACKWARD_GROUP | SF_HAS_F: PROF_LAUNCH((mfma16_backward_group_kernel<true, G>), grid, block, bwd_lds, h->stream, a); return 0;
      default: break;
    }
  } else switch (rt.id) {   // pure fp32 on v_mfma_f32_16x16x4_f32 (ALTRO_HIP_F32_PURE)
    case SK_MFMA16_BACKWARD_F32X4: PROF_LAUNCH((mfma16_backward_f32x4_kernel<false, 2, 2>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_BACKWARD_F32X4 | SF_HAS_F: PROF_LAUNCH((mfma16_backward_f32x4_kernel<true, 2, 2>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_BACKWARD_F32: PROF_LAUNCH((mfma16_backward_f32_kernel<false, 3>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_BACKWARD_F32 | SF_HAS_F: PROF_LAUNCH((mfma16_backward_f32_kernel<true, 3>), grid, block, 0, h->stream, a); return 0;
    case SK_MFMA16_FORWARD_F32X4: PROF_LAUNCH((mfma16_forward_f32x4_kernel<2, 2>), grid, block, 0, h->stream, a); return 0;
    default: break;
  }
  return 1;
}

// One sweep launch: ask the route (sweep_route.h), keep it on the handle, run the kernel it names.
int sweep_launch(altro_hip_batch* h, int slot, double reg, const BackwardMask& pp) {
  ProfScope ps(h, slot);
  const bool backward = slot == 0, f64 = h->dtype == ALTRO_HIP_F64;
  const SweepRoute rt = h->last_sweep[slot] = sweep_route(sweep_shape(h), SweepCall{backward, backward && pp.active != nullptr});
  h->sweep_launched[slot] = true;
  if (rt.error) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "plan MFMA32 has no forward kernel for (n, m) = (%d, %d)", h->n, h->m);
  int rc = 1;   // (1: no launcher below carries the id)
  switch (rt.id & ~SF_MASK) {
    case SK_TILE32_BACKWARD: rc = tile32_launch_backward(h, reg, pp); break;
    case SK_TILE32_FORWARD: rc = tile32_launch_forward(h); break;
    case SK_GENERIC_BACKWARD: case SK_GENERIC_FORWARD:
      rc = f64 ? generic_sweep<double>(h, rt, backward, reg, pp) : generic_sweep<float>(h, rt, backward, reg, pp); break;
    case SK_LANE_BACKWARD: case SK_LANE_FORWARD: case SK_QUAD_BACKWARD: case SK_QUAD2_BACKWARD: case SK_QUAD_FORWARD:
      rc = f64 ? lane_sweep<double>(h, rt, backward, reg, pp) : lane_sweep<float>(h, rt, backward, reg, pp); break;
    default: rc = f64 ? mfma16_sweep<double>(h, rt, reg, pp) : mfma16_sweep<float>(h, rt, reg, pp); break;
  }
  if (rc == 1) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "internal error: sweep kernel %#x has no launcher", rt.id);
  if (rc) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(ALTRO_HIP_ERR_HIP, "%s launch: %s", backward ? "backward" : "forward", hipGetErrorString(e));
  return 0;
}

}  // namespace

namespace altro_hip {
namespace capi {

void profile_add(altro_hip_batch* h, int slot, float ms) {
  h->prof_min[slot] = h->prof_launches[slot] ? std::min(h->prof_min[slot], (double)ms) : (double)ms;
  h->prof_max[slot] = std::max(h->prof_max[slot], (double)ms);
  h->prof_ms[slot] += ms;
  h->prof_launches[slot] += 1;
}

int launch_backward(altro_hip_batch* h, double reg, const BackwardMask& pp) {
  h->aff_base = false;   // (new gains: altro_hip_merit_affine's stored base is the last sweep's)
  return sweep_launch(h, 0, reg, pp);
}

int launch_forward(altro_hip_batch* h) {
  h->expansion_current = false;   // the sweep writes the candidate trajectory: whatever expansion a merit pass left is not of this point
  return sweep_launch(h, 1, 0.0, {});
}

}  // namespace capi
}  // namespace altro_hip

extern "C" {

int altro_hip_backward(altro_hip_batch* h, double reg) {
  int rc = check(h);
  if (rc) return rc;
  if (!h->dyn_set || !h->cost_set) return fail(ALTRO_HIP_ERR_NOT_SET, "set_dynamics and set_cost must precede backward");
  rc = launch_backward(h, reg, {});
  if (!rc) h->backward_done = true;
  return rc;
}

int altro_hip_backward_per_problem(altro_hip_batch* h, const double* reg) {
  int rc = check(h);
  if (rc) return rc;
  if (!reg) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "reg is null");
  if (!h->dyn_set || !h->cost_set) return fail(ALTRO_HIP_ERR_NOT_SET, "set_dynamics and set_cost must precede backward");
  // (the solve loop's own per-problem vector: every solve initialises it before it reads it)
  HIP_TRY(hipMemcpyAsync(h->i_reg, reg, (size_t)h->batch * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));   // the caller's array is free on return
  rc = launch_backward(h, 0.0, BackwardMask{nullptr, h->i_reg});
  if (!rc) h->backward_done = true;
  return rc;
}

int altro_hip_forward_ltv(altro_hip_batch* h) {
  int rc = check(h);
  if (rc) return rc;
  if (!h->backward_done) return fail(ALTRO_HIP_ERR_NOT_SET, "backward must precede forward_ltv");
  if (!h->x0_set) return fail(ALTRO_HIP_ERR_NOT_SET, "set_initial_state must precede forward_ltv");
  rc = launch_forward(h);
  if (!rc) h->forward_done = true;
  return rc;
}

int altro_hip_sweep(altro_hip_batch* h, double reg) {
  int rc = altro_hip_backward(h, reg);
  if (!rc) rc = altro_hip_forward_ltv(h);
  return rc;
}

// MFMA layout self-test (tests/test_gpu_parity.py): max |D - (A B + C)| for random operands.
namespace {
__global__ void sincos_selftest_kernel(const double* x, int n, double* s, double* c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) sincos_hd<double>(x[i], &s[i], &c[i]);
}
}  // namespace
// the device's fp64 sincos (models.h) on n arguments: the accuracy test of tests/test_gpu_trig.py
int altro_hip_selftest_sincos(int device, const double* x, int n, double* s, double* c) {
  if (!x || !s || !c || n <= 0) return ALTRO_HIP_ERR_BAD_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return ALTRO_HIP_ERR_NO_DEVICE;
  DevTemp dx, ds, dc;
  const size_t bytes = (size_t)n * sizeof(double);
  if (!dx.alloc(bytes) || !ds.alloc(bytes) || !dc.alloc(bytes)) return ALTRO_HIP_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(dx.p, x, bytes, hipMemcpyHostToDevice) != hipSuccess) return ALTRO_HIP_ERR_HIP;
  hipLaunchKernelGGL(sincos_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, dx.as<const double>(), n, ds.as<double>(), dc.as<double>());
  if (hipMemcpy(s, ds.p, bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(c, dc.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return ALTRO_HIP_ERR_HIP;
  return 0;
}
double altro_hip_selftest_mfma_f64(int device) {
  if (hipSetDevice(device) != hipSuccess) return -1.0;
  double hA[64], hB[64], hC[256], hD[256];
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1 << 24) - 0.5; };
  for (double& v : hA) v = rnd();
  for (double& v : hB) v = rnd();
  for (double& v : hC) v = rnd();
  DevTemp dA, dB, dC, dD;
  if (!dA.alloc(sizeof(hA)) || !dB.alloc(sizeof(hB)) || !dC.alloc(sizeof(hC)) || !dD.alloc(sizeof(hD))) return -1.0;
  (void)hipMemcpy(dA.p, hA, sizeof(hA), hipMemcpyHostToDevice);
  (void)hipMemcpy(dB.p, hB, sizeof(hB), hipMemcpyHostToDevice);
  (void)hipMemcpy(dC.p, hC, sizeof(hC), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(mfma16_selftest_kernel, dim3(1), dim3(64), 0, 0, dA.as<double>(), dB.as<double>(), dC.as<double>(), dD.as<double>());
  if (hipMemcpy(hD, dD.p, sizeof(hD), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
  double worst = 0.0;
  for (int i = 0; i < 16; ++i)
    for (int j = 0; j < 16; ++j) {
      double ref = hC[i * 16 + j];
      for (int k = 0; k < 4; ++k) ref += hA[i * 4 + k] * hB[k * 16 + j];
      worst = std::max(worst, std::abs(ref - hD[i * 16 + j]));
    }
  return worst;
}

// 4-block layout self-test (tests/test_gpu_parity.py): max |D_b - (A_b B_b + C_b)| over the four blocks of
// v_mfma_f32_16x16x1_4b_f32 with the layout kernels/tvlqr_mfma16_f32x4.hip assumes.
double altro_hip_selftest_mfma_f32_4b(int device) {
  if (hipSetDevice(device) != hipSuccess) return -1.0;
  float hA[64], hB[64], hC[1024], hD[1024];
  unsigned s = 2468u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / (1 << 24) - 0.5f; };
  for (float& v : hA) v = rnd();
  for (float& v : hB) v = rnd();
  for (float& v : hC) v = rnd();
  DevTemp dA, dB, dC, dD;
  if (!dA.alloc(sizeof(hA)) || !dB.alloc(sizeof(hB)) || !dC.alloc(sizeof(hC)) || !dD.alloc(sizeof(hD))) return -1.0;
  (void)hipMemcpy(dA.p, hA, sizeof(hA), hipMemcpyHostToDevice);
  (void)hipMemcpy(dB.p, hB, sizeof(hB), hipMemcpyHostToDevice);
  (void)hipMemcpy(dC.p, hC, sizeof(hC), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(mfma16_selftest_4b_kernel, dim3(1), dim3(64), 0, 0, dA.as<float>(), dB.as<float>(), dC.as<float>(), dD.as<float>());
  if (hipMemcpy(hD, dD.p, sizeof(hD), hipMemcpyDeviceToHost) != hipSuccess) return -1.0;
  double worst = 0.0;
  for (int b = 0; b < 4; ++b)
    for (int i = 0; i < 16; ++i)
      for (int j = 0; j < 16; ++j) {
        const double ref = (double)hC[b * 256 + i * 16 + j] + (double)hA[16 * b + i] * (double)hB[16 * b + j];
        worst = std::max(worst, std::abs(ref - (double)hD[b * 256 + i * 16 + j]));
      }
  return worst;
}

}  // extern "C"
