// sweep_route.h -- which TVLQR sweep kernel a launch takes, on every plan: sweep_route(shape, call) returns the kernel id with its template
// switches, the ALTRO_HIP_SWEEP_* bits, grid, block and (plan GENERIC) the carve.  The one place that decides: launch_backward /
// launch_forward (capi_tvlqr.hip) execute the route and keep it on the handle, altro_hip_sweep_variant and altro_hip_profile_get report
// that record.  Plan GENERIC's own choices -- the size of the backward kernel's carve, {blocks in LDS, "late Q", work block in global
// memory}, the staged / unstaged forward kernel -- are generic_backward_route / generic_forward_route, which the single-problem drop-in
// (tvlqr_dropin.hip) asks directly.  Host code, no HIP includes: tests/cpp/sweep_route_test.cpp checks it with g++ against rows written
// out by hand.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "altro_hip/altro_hip.h"
// (the layout header marks its constexpr functions for both sides; a plain host compiler that has seen no HIP header reads past that)
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#include "kernels/mfma16_layout.h"
#undef __host__
#undef __device__
#else
#include "kernels/mfma16_layout.h"
#endif

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

// ---- every plan -------------------------------------------------------------------------------------------------------------------
// A sweep kernel id: the kernel family and the flags that pick among its instantiations (the element type is the handle's, plan LANE's
// (n, m) the shape's: the launcher supplies both).
enum SweepKernelId : int {
  // template switches
  SF_HAS_F = 1,          // plan MFMA16's backward kernels: the affine term f is read
  SF_STORE_Q = 2,        // mfma16_backward_kernel: also writes the Q blocks (ALTRO_HIP_STORE_QBLOCKS)
  SF_FUSED = 4,          // plan LANE: the *_fused instantiation (ALTRO_HIP_LANE_FUSED)
  SF_LATE_Q = 8,         // generic_backward_kernel<.., LQ = true>
  SF_GLOBAL_WS = 16,     // generic_backward_kernel<T, BIG = true>
  SF_MATRIX_CORES = 32,  // generic_backward_kernel<double, .., MFMA = true>
  SF_STAGED = 64,        // generic_forward_kernel<T, STAGE = true>
  SF_MASK = 255,
  // families
  SK_GENERIC_BACKWARD = 1 << 8, SK_GENERIC_FORWARD = 2 << 8,
  SK_MFMA16_BACKWARD = 3 << 8,   // fp64, or fp32 records with fp64 tiles
  SK_MFMA16_BACKWARD_F32 = 4 << 8, SK_MFMA16_BACKWARD_F32X4 = 5 << 8,   // pure fp32: a problem per wave, four problems per wave
  SK_MFMA16_BACKWARD_GROUP = 6 << 8,   // fp64: one workgroup of 16 waves per 16 problems
  SK_MFMA16_FORWARD = 7 << 8, SK_MFMA16_FORWARD_F32X4 = 8 << 8, SK_MFMA16_FORWARD_GROUP = 9 << 8,
  SK_LANE_BACKWARD = 10 << 8, SK_LANE_FORWARD = 11 << 8,
  SK_QUAD_BACKWARD = 12 << 8 /* (4, 2) */, SK_QUAD2_BACKWARD = 13 << 8 /* (2, 1) */, SK_QUAD_FORWARD = 14 << 8 /* (4, 2) */,
  SK_TILE32_BACKWARD = 15 << 8, SK_TILE32_FORWARD = 16 << 8   // plan MFMA32 (capi_tile32.hip picks the shape's instantiation)
};
// the name altro_hip_profile_get reports (the fused and unfused instantiations share one); null: not an id
inline const char* sweep_kernel_name(int id) {
  switch (id & ~SF_MASK) {
    case SK_GENERIC_BACKWARD: return "generic_backward_kernel";
    case SK_GENERIC_FORWARD: return "generic_forward_kernel";
    case SK_MFMA16_BACKWARD: return "mfma16_backward_kernel";
    case SK_MFMA16_BACKWARD_F32: return "mfma16_backward_f32_kernel";
    case SK_MFMA16_BACKWARD_F32X4: return "mfma16_backward_f32x4_kernel";
    case SK_MFMA16_BACKWARD_GROUP: return "mfma16_backward_group_kernel";
    case SK_MFMA16_FORWARD: return "mfma16_forward_kernel";
    case SK_MFMA16_FORWARD_F32X4: return "mfma16_forward_f32x4_kernel";
    case SK_MFMA16_FORWARD_GROUP: return "mfma16_forward_group_kernel";
    case SK_LANE_BACKWARD: return "lane_backward_kernel";
    case SK_LANE_FORWARD: return "lane_forward_kernel";
    case SK_QUAD_BACKWARD: return "quad_backward_kernel";
    case SK_QUAD2_BACKWARD: return "quad2_backward_kernel";
    case SK_QUAD_FORWARD: return "quad_forward_kernel";
    case SK_TILE32_BACKWARD: return "tile32_backward_kernel";
    case SK_TILE32_FORWARD: return "tile32_forward_kernel";
    default: return nullptr;
  }
}

// everything a choice may depend on
struct SweepShape {
  int plan;             // ALTRO_HIP_PLAN_GENERIC / _MFMA16 / _LANE (plan MFMA32 is GENERIC with g_tile)
  bool f64;             // the records' element type
  unsigned flags, forms;
  int n, m, N, batch;
  bool is_diag;
  bool has_f;           // the affine term is given AND read (not a linearised iLQR sweep)
  bool g_tile, g_mfma;  // plan MFMA32; plan GENERIC fp64 with ALTRO_HIP_GENERIC_MATRIX_CORES
  int64_t in_bs, in_ks, cin_bs, cin_ks, out_bs, out_ks;   // plan MFMA16: Mfma16Strides of the DYN, COST and OUT records
};
struct SweepCall {
  bool backward;
  bool masked;          // a backward launch with an `active` mask (a per-problem regularisation alone is not one)
};
enum SweepError { SWEEP_OK = 0, SWEEP_NO_FORWARD /* "plan MFMA32 has no forward kernel for (n, m)" */ };
struct SweepRoute {
  int id = 0;           // SweepKernelId
  int variant = 0;      // ALTRO_HIP_SWEEP_* (altro_hip_sweep_variant)
  unsigned grid = 0, block = 0;
  size_t lds = 0;       // plan GENERIC's kernels: the carve (with SF_GLOBAL_WS the work block of one problem, no dynamic LDS); the group
                        // and tile kernels take theirs from their layout structs at the launch
  int error = SWEEP_OK;
};

// plan MFMA32's forward kernel is instantiated per (ceil(n / 4), ceil(m / 4)): every shape the plan takes has one
#define TILE32_FORWARD_TILES(X) X(2, 2) X(3, 2) X(4, 1) X(4, 2) X(5, 1) X(5, 2) X(6, 1) X(6, 2) X(7, 1) X(7, 2) X(8, 1)
constexpr bool tile32_forward_ok(int n, int m) {
#define X(KC_, MC_) if ((n + 3) / 4 == KC_ && (m + 3) / 4 == MC_) return true;
  TILE32_FORWARD_TILES(X)
#undef X
  return false;
}

constexpr int kSweepGroup = 16;   // problems of one workgroup of plan MFMA16's group kernels (a wave each)
// whole groups of problems in the contiguous [k][b] slabs
inline bool mfma16_group_slabs(const SweepShape& s) {
  const int64_t B = s.batch;
  return s.batch % kSweepGroup == 0 && s.in_bs == MF_DYN && s.in_ks == B * MF_DYN && s.out_bs == MF_OUT && s.out_ks == B * MF_OUT;
}

// Plan MFMA16.  fp64, whole groups of 16 problems, backward: one workgroup of 16 waves per group fetches the group's DYN and COST records
// as contiguous runs (kernels/tvlqr_mfma16_bwd_group.hip).  127 KB of dynamic LDS: one workgroup per CU, sixteen waves, the occupancy of
// the wave-per-problem kernel.  A launch with an `active` mask keeps that kernel: a masked wave must not leave a workgroup that has
// barriers, and a launch with few active problems is better served by waves that return at once.  ALTRO_HIP_FORM_BACKWARD_WAVE keeps
// the wave-per-problem kernel, and so does ALTRO_HIP_STORE_QBLOCKS.
// Forward, fp64: the same form (kernels/tvlqr_mfma16_fwd_group.hip).  G = 16 with a register ring two knot points deep is the form
// tools/membench.hip `group` measured fastest (G = 8 or the LDS-DMA fetch: 4-9 % slower; depth 3: no faster).  136 KB of dynamic LDS:
// one workgroup per CU, sixteen waves.  ALTRO_HIP_FORM_FORWARD_WAVE keeps the wave-per-problem kernel (register-ring depth 3: depths
// 1..4 were measured, DESIGN.md section 4.2, 3 is the knee).
// fp32 records: fp64 tiles unless ALTRO_HIP_F32_PURE asks for v_mfma_f32_16x16x4_f32 (and, backward, no Q blocks are stored).  Pure
// fp32 takes four problems per wave (kernels/tvlqr_mfma16_f32x4.hip, tvlqr_mfma16_fwd_f32x4.hip) whenever the batch is whole quads; the
// one-problem kernel stays for the others.  Backward ring depth 2, two waves per SIMD: measured on C4 against (1,2) (1,3) (3,1) (3,2)
// (4,1) -- 3.40 ms against 4.1-4.4 (profiles/r02g_c4_quad_variants.txt); forward ring depth 2, two waves per SIMD: measured on C4 on two
// boxes against seven other (depth, waves) pairs and the one-problem kernel (profiles/r03e_ / r03f_c4_fwd_variants.txt: 2.47 / 2.375 ms;
// the others 2.39-2.84).
inline SweepRoute sweep_route_mfma16(const SweepShape& s, const SweepCall& c) {
  const bool sq = (s.flags & ALTRO_HIP_STORE_QBLOCKS) != 0, pure = !s.f64 && (s.flags & ALTRO_HIP_F32_PURE), quads = s.batch % 4 == 0;
  const unsigned wave = (unsigned)mf_grid(s.batch), group = (unsigned)mf_grid(s.batch / kSweepGroup), block = 64 * kSweepGroup;
  if (!c.backward) {
    if (s.f64 && !(s.forms & ALTRO_HIP_FORM_FORWARD_WAVE) && mfma16_group_slabs(s)) return {SK_MFMA16_FORWARD_GROUP, 0, group, block};
    if (pure && quads) return {SK_MFMA16_FORWARD_F32X4, 0, (unsigned)mf_grid(s.batch / 4), 64};
    return {SK_MFMA16_FORWARD, 0, wave, 64};
  }
  const int f = s.has_f ? SF_HAS_F : 0;
  if (s.f64 && !(s.forms & ALTRO_HIP_FORM_BACKWARD_WAVE) && !sq && !c.masked && mfma16_group_slabs(s) && s.cin_bs == MF_COST &&
      s.cin_ks == (int64_t)s.batch * MF_COST)
    return {SK_MFMA16_BACKWARD_GROUP | f, ALTRO_HIP_SWEEP_GROUP, group, block};
  if (!pure || sq) return {SK_MFMA16_BACKWARD | f | (sq ? SF_STORE_Q : 0), 0, wave, 64};
  if (quads) return {SK_MFMA16_BACKWARD_F32X4 | f, 0, (unsigned)mf_grid(s.batch / 4), 64};
  return {SK_MFMA16_BACKWARD_F32 | f, 0, wave, 64};
}

// Plan LANE: a lane per problem, 64 problems per workgroup, workgroups in whole eights.
// (4, 2) and (2, 1): four lanes per problem (kernels/tvlqr_quad_body.inc, tvlqr_quad2_body.inc), same records, bit-identical
// results -- while the batch leaves the chip idle; the forward sweep of (4, 2) as well.  Measured on MI355X (tools/c3_quad_ab.sh,
// profiles/r03i_quad_ab.txt, backward + forward ms, quad / lane-per-problem): (4, 2) 0.12 / 0.21 at 4096 problems, 0.16 / 0.23 at 8192,
// 0.28 / 0.27 at 16384, 0.56 / 0.44 at 32768, 1.10 / 0.84 at 65536; (2, 1) 0.10 / 0.12, 0.11 / 0.12, 0.16 / 0.14, 0.31 / 0.25,
// 0.60 / 0.49.  The quad form shortens the chain of one wave (what bounds small batches); once every SIMD has its waves the sweep is
// HBM-bound and the lane-per-problem form's 512-byte runs stream better than the quad's four 128-byte segments.
// ALTRO_HIP_FORM_LANE_QUAD_OFF / _ON forces one or the other.
inline SweepRoute sweep_route_lane(const SweepShape& s, const SweepCall& c) {
  const bool quad_on = (s.forms & ALTRO_HIP_FORM_LANE_QUAD_ON) ? true : (s.forms & ALTRO_HIP_FORM_LANE_QUAD_OFF) ? false : s.batch <= 12288;
  const bool q42 = s.n == 4 && s.m == 2, q21 = s.n == 2 && s.m == 1;
  const int f = (s.flags & ALTRO_HIP_LANE_FUSED) ? SF_FUSED : 0;
  const unsigned lane = 8u * (unsigned)(((s.batch + 63) / 64 + 7) / 8), quad = 8u * (unsigned)(((s.batch + 15) / 16 + 7) / 8);
  if (quad_on && q42) return {(c.backward ? SK_QUAD_BACKWARD : SK_QUAD_FORWARD) | f, 0, quad, 64};
  if (quad_on && q21 && c.backward) return {SK_QUAD2_BACKWARD | f, 0, quad, 64};
  return {(c.backward ? SK_LANE_BACKWARD : SK_LANE_FORWARD) | f, 0, lane, 64};
}

// Plans GENERIC and MFMA32: a wave per problem.  Plan MFMA32 takes the tile kernels, but a diagonal cost keeps its diagonals packed and
// plan GENERIC's own backward kernel reads those.  Plan GENERIC backward: generic_backward_route above.  Forward (always with the
// multipliers y): the knot point's blocks staged in LDS and fetched a knot point ahead while sixteen waves still fit a CU (10 KB each:
// measured at 4096 problems, (13, 4) 1.53 -> 1.21 ms, (16, 4) 1.62 -> 1.27, but (24, 8) at 13 KB 2.37 -> 3.58); else rows from global
// memory.
inline SweepRoute sweep_route_generic(const SweepShape& s, const SweepCall& c) {
  const size_t esz = s.f64 ? sizeof(double) : sizeof(float);
  if (s.g_tile && !c.backward)
    return {SK_TILE32_FORWARD, 0, (unsigned)mf_grid(s.batch), 64, 0, tile32_forward_ok(s.n, s.m) ? SWEEP_OK : SWEEP_NO_FORWARD};
  if (s.g_tile && !s.is_diag) return {SK_TILE32_BACKWARD, 0, (unsigned)mf_grid(s.batch), 64};
  if (!c.backward) {
    const GenericForwardRoute rt = generic_forward_route(s.n, s.m, 1, esz, kGenericForwardStageLimit);
    return {SK_GENERIC_FORWARD | (rt.staged ? SF_STAGED : 0), rt.variant(), (unsigned)s.batch, 64, rt.bytes};
  }
  const GenericBackwardRoute rt = generic_backward_route(s.n, s.m, esz, s.batch, s.forms);
  const bool mc = s.f64 && s.g_mfma;
  return {SK_GENERIC_BACKWARD | (rt.late_q ? SF_LATE_Q : 0) | (rt.big ? SF_GLOBAL_WS : 0) | (mc ? SF_MATRIX_CORES : 0),
          rt.variant() | (mc ? ALTRO_HIP_SWEEP_MATRIX_CORES : 0), (unsigned)s.batch, 64, rt.bytes};
}

inline SweepRoute sweep_route(const SweepShape& s, const SweepCall& c) {
  return s.plan == ALTRO_HIP_PLAN_MFMA16 ? sweep_route_mfma16(s, c) : s.plan == ALTRO_HIP_PLAN_LANE ? sweep_route_lane(s, c) : sweep_route_generic(s, c);
}

}  // namespace altro_hip
