// tvlqr_mfma16_bwd_group.hip -- plan MFMA16, fp64: the backward sweep with one workgroup of G waves per G adjacent problems.
//
// Why.  mfma16_backward_kernel is 4096 independent waves that each fetch their own 1,632-byte DYN and 1,280-byte COST record
// whenever they get there.  In the [k][b] slabs the records of G adjacent problems are ONE contiguous run per knot point and
// array (G = 16: 26,112 bytes of DYN, 20,480 bytes of COST), and a workgroup that fetches both runs in order, as consecutive
// 16-byte chunks over all its threads, streams them faster: tools/membench.hip `group` prices the traffic of this kernel's
// form (register stage one knot point deep, two LDS slots, OUT stored per wave) with no arithmetic at 0.94 of the time of the
// wave-per-problem form: 0.795-0.799 against 0.843-0.846 ms (profiles/r08a_membench_bwd_group_run1.txt, _run2.txt).
//
// What changes is the fetch alone.  Wave w of a group owns problem b0 + w exactly as a wave owns a problem in
// mfma16_backward_kernel: it reads the same Mfma16Knot out of the slot with mfma16_load_knot's lane-to-element mapping and runs
// the same mfma16_bwd_step on it, with its own exchange areas, so K, d, P, p, delta_V and status come out bit for bit the same.
//
//   thread t of the 64 G:   three 16-byte chunks of the 182 G chunks of a knot point, dealt so that every wave-instruction lies
//                           inside one run: its address is a wave-uniform base (stepped per trip on the scalar unit) plus one
//                           32-bit per-thread offset.  global_load_dwordx4 into a register stage ONE knot point deep (12 VGPRs:
//                           the ring two deep of the forward group kernel does not fit beside this sweep's arithmetic).
//   step k (walked down):   every wave reads its operands of knot point k out of slot s = (N - 1 - k) % 2; every thread writes
//                           the chunks it holds (knot point k - 1, requested one step ago) into slot 1 - s and requests knot
//                           point k - 2 into the freed registers; the step's arithmetic and stores; ONE bare barrier.
//                           Slot 1 - s was last read in step k + 1, before that step's barrier; slot s was written in step
//                           k + 1, before that step's barrier.
//   stores:                 every wave stores its own OUT record, 8 bytes per lane, as in the wave-per-problem kernel (a failed
//                           problem's go to its trash record, nothing below the failing knot point is written).
//
// Barrier safety: a group is G whole problems and the launcher routes no launch with an `active` mask here, a workgroup past the
// end of a ragged eighth returns as a whole before any barrier, a failed problem keeps iterating, and the trip count depends on
// N only.
//
// Figures (hipcc -O3, gfx950, G = 16): 120 VGPRs with f (112 without), 44 SGPRs, no scratch; the loop is 266 instructions per
// knot point (8 MFMA, 83 fp64 VALU, 35 other VALU of which 3 v_lshl_add_u64 and no integer multiply, 39 LDS, 3 loads, 4 stores)
// against the wave-per-problem kernel's 258 (124 VGPRs).  LDS: two slots of 46,592 bytes + sixteen private areas of 82 + 204
// doubles = 129,792 bytes of dynamic LDS, one workgroup of sixteen waves per CU.  No exec-masked VMEM in the loop; hipcc waits for
// the staged chunks with vmcnt(6), (5), (4): the step's four stores, issued after the requests, are not drained.
#pragma once
#include "tvlqr_mfma16.hip"

namespace altro_hip {

typedef double mf_f64x2 __attribute__((ext_vector_type(2)));

template <int G>
struct Mfma16BwdGroup {
  static constexpr int T = 64 * G;                                  // threads
  static constexpr int NA = G * MF_DYN / 2, NB = G * MF_COST / 2;   // 16-byte chunks of the DYN run and of the COST run
  static constexpr int SLOT = NA + NB;                              // ring slot in chunks: the DYN run, then the COST run
  // Rounds of T chunks, each wave-instruction inside one run: FA whole rounds of the DYN run; a mixed round whose first WA waves
  // finish the DYN run (past its end: the last chunk again, same bytes to the same place) while the others begin the COST run
  // with B0 chunks; the rest of the COST run.
  static constexpr int FA = NA / T, REMA = NA - FA * T, WA = (REMA + 63) / 64;
  static constexpr int B0 = REMA ? T - 64 * WA : 0;
  static constexpr int ROUNDS = FA + (REMA ? 1 : 0) + (NB - B0 + T - 1) / T;
  static constexpr int PRIV = MF_BWD_XCH + MF_BWD_PTILE;            // doubles of a wave's own exchange areas
  static constexpr size_t lds_bytes() { return ((size_t)2 * SLOT * 2 + (size_t)G * PRIV) * sizeof(double); }
};
static_assert(MF_DYN % 2 == 0 && MF_COST % 2 == 0 && MF_BWD_XCH % 2 == 0, "records and areas are whole 16-byte chunks");

template <bool HAS_F, int G>
__global__ __launch_bounds__(64 * G) void mfma16_backward_group_kernel(Mfma16Args<double> a) {
  using GR = Mfma16BwdGroup<G>;
  static_assert(GR::ROUNDS * 4 <= 12, "at most 12 staging VGPRs");
  static_assert(GR::lds_bytes() <= 160 * 1024, "LDS of one CU");
  constexpr unsigned SLOTB = GR::SLOT * 16;   // bytes
  extern __shared__ __attribute__((aligned(16))) double mf_bwd_group_lds[];
  char* const ring = (char*)mf_bwd_group_lds;
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  double* const xch = mf_bwd_group_lds + (size_t)2 * GR::SLOT * 2 + (size_t)wv * GR::PRIV;   // this wave's own areas
  double* const ptile = xch + MF_BWD_XCH;
  const int ngrp = a.batch / G;
  const int grp = mf_problem(blockIdx.x, ngrp);
  if (grp >= ngrp) return;   // the whole workgroup
  const int b0 = grp * G, b = b0 + wv;
  const int N = a.N;
  if (lane < 2) xch[80 + lane] = 0.0;
  const Mfma16BwdLane ln = mfma16_bwd_lane(lane);
  const Mfma16QOff qo = mfma16_q_offsets(ln.j, ln.g);
  double* __restrict__ trash = a.trash + (size_t)b * MF_OUT;

  // this thread's chunk of every round: which run (the same for its whole wave), the byte offset inside it, and the byte
  // offset inside a slot
  bool isa[GR::ROUNDS];
  unsigned srcb[GR::ROUNDS], dstb[GR::ROUNDS];
#pragma unroll
  for (int r = 0; r < GR::ROUNDS; ++r) {
    int c;
    if (r < GR::FA) { isa[r] = true; c = r * GR::T + t; }
    else if (GR::REMA && r == GR::FA) {
      isa[r] = wv < GR::WA;
      c = isa[r] ? (r * GR::T + t < GR::NA ? r * GR::T + t : GR::NA - 1) : t - 64 * GR::WA;
    } else {
      isa[r] = false;
      c = GR::B0 + (r - GR::FA - (GR::REMA ? 1 : 0)) * GR::T + t;
      c = c < GR::NB ? c : GR::NB - 1;
    }
    srcb[r] = 16u * (unsigned)c;
    dstb[r] = srcb[r] + (isa[r] ? 0u : 16u * GR::NA);
  }
  // the runs of knot point N - 1; stepped down per request (the library's own [k][b] slabs: the launcher checks the strides)
  const char* pa = (const char*)(a.in + ((size_t)(N - 1) * a.in_ks + (size_t)b0 * MF_DYN));
  const char* pb = (const char*)(a.cin + ((size_t)(N - 1) * a.cin_ks + (size_t)b0 * MF_COST));
  const int64_t sa = a.in_ks * (int64_t)sizeof(double), sb = a.cin_ks * (int64_t)sizeof(double);
  mf_f64x2 regs[GR::ROUNDS];
  auto fetch = [&]() {
#pragma unroll
    for (int r = 0; r < GR::ROUNDS; ++r) regs[r] = *(const mf_f64x2*)((isa[r] ? pa : pb) + srcb[r]);
  };
  auto stage = [&](unsigned slot_off) {
#pragma unroll
    for (int r = 0; r < GR::ROUNDS; ++r) *(mf_f64x2*)(ring + slot_off + dstb[r]) = regs[r];
  };

  Mfma16BwdState st;
  mfma16_bwd_terminal<double>(st, ln, a.term + (size_t)b * MF_TERM, a.outn + (size_t)b * MF_TERM);
  const double reg = a.reg_pp ? a.reg_pp[b] : a.reg;

  fetch();                                // knot point N - 1 -> slot 0
  __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
  stage(0);
  if (N >= 2) { pa -= sa; pb -= sb; }
  fetch();                                // knot point N - 2 stays in the stage (N == 1: record 0 again, nobody reads it)
  // vmcnt(0): drained before the loop (see mfma16_backward_kernel), or every step waits for all its requests
  __builtin_amdgcn_s_waitcnt(0x0F70);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  double* outk = a.out + ((size_t)(N - 1) * a.out_ks + (size_t)b * a.out_bs);
  unsigned slot_off = 0;
  for (int k = N - 1; k >= 0; --k) {
    // this wave's own operands out of the slot, in the lane order of mfma16_load_knot
    Mfma16Knot cur;
    {
      const double* __restrict__ rec = (const double*)(ring + slot_off) + wv * MF_DYN;
      const double* __restrict__ crec = (const double*)(ring + slot_off) + 2 * GR::NA + wv * MF_COST;
      mfma16_load_knot<HAS_F, double>(cur, rec, crec, lane, ln.j, ln.g, qo);
    }
    stage(SLOTB - slot_off);              // knot point k - 1
    if (k >= 2) { pa -= sa; pb -= sb; }
    fetch();                              // knot point k - 2 (k < 2: record 0 again, harmless)
    mfma16_bwd_step<false, HAS_F, true, double>(cur, st, ln, xch, ptile, lane, k, reg, outk, trash, nullptr);
    outk -= a.out_ks;
    slot_off = SLOTB - slot_off;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();         // the other slot is whole, this one is free (a bare barrier: the requests stay in flight)
    asm volatile("" ::: "memory");
  }
  mfma16_bwd_finish<double>(st, ln, a, b);
}

}  // namespace altro_hip
