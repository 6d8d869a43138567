// tvlqr_mfma16_fwd_group.hip -- plan MFMA16, fp64: the forward sweep with one workgroup of G waves per G adjacent problems.
//
// Why.  mfma16_forward_kernel is 4096 independent waves that each fetch their own 1,632-byte DYN and 1,152-byte OUT record
// whenever they get there: the random-rows case of an HBM gather (5.1 TB/s).  In the [k][b] slabs the records of G adjacent
// problems are ONE contiguous run per knot point and array (G = 16: 26,112 bytes of DYN, 18,432 bytes of OUT), and a
// workgroup that fetches both runs in order, as consecutive 16-byte chunks over all its threads, streams them faster:
// tools/membench.hip `group` prices the same traffic with no arithmetic at 0.90 (one run) and 0.89 (another) of the time of the
// wave-per-problem form: 0.513 against 0.571 ms, 0.570 against 0.640 (profiles/r07a_membench_group_run1.txt, _run2.txt).
//
// What changes is the fetch alone.  Wave w of a group owns problem b0 + w exactly as a wave owns a problem in
// mfma16_forward_kernel: it builds the same 17-pitch LDS image with mfma16_fwd_stage and runs the same mfma16_fwd_step on it,
// so x, u and y come out bit for bit the same.
//
//   thread t of the 64 G:   chunk t, t + 64 G, t + 128 G of the 174 G chunks of a knot point (DYN run, then OUT run),
//                           global_load_dwordx4 into a register ring DEPTH knot points deep, ds_write_b128 into ring slot
//                           k % DEPTH at step k, and at once the request for knot point k + DEPTH into the freed registers
//   one barrier per step:   the slot is whole.  Then every wave reads its own record out of it.  Slot k % DEPTH is written again
//                           at step k + DEPTH >= k + 2, and no wave gets there before every wave has passed the barrier of
//                           step k + 1, i.e. has finished reading at step k: the ring of DEPTH >= 2 slots needs no second
//                           barrier.  (The LDS-DMA form -- global_load_lds into the slot -- does need one before the refill, and
//                           measured 4 % slower than this one in the probe.)
//
// Barrier safety: a group is G whole problems (the launcher routes only batches that are multiples of G here), a workgroup
// past the end of a ragged eighth returns as a whole before any barrier, and the trip count depends on N only.
#pragma once
#include "tvlqr_mfma16.hip"

namespace altro_hip {

typedef double mf_f64x2 __attribute__((ext_vector_type(2)));

template <int G>
struct Mfma16FwdGroup {
  static constexpr int T = 64 * G;                               // threads
  static constexpr int CD = MF_DYN / 2, CO = MF_OUT / 2;         // 16-byte chunks per record
  static constexpr int CIN = G * (CD + CO);                      // chunks per knot point: the DYN run, then the OUT run
  static constexpr int ROUNDS = (CIN + T - 1) / T;
  static constexpr int SLOT = CIN;                               // ring slot pitch in chunks
  static constexpr int IMG = MF_FWD_LDS + 4;                     // doubles per private image (as in mfma16_forward_kernel)
  static constexpr size_t lds_bytes(int depth) { return ((size_t)depth * SLOT * 2 + (size_t)G * IMG) * sizeof(double); }
};
static_assert(MF_DYN % 2 == 0 && MF_OUT % 2 == 0, "records are whole 16-byte chunks");

template <typename S, int G, int DEPTH>
__global__ __launch_bounds__(64 * G) void mfma16_forward_group_kernel(Mfma16Args<S> a) {
  static_assert(sizeof(S) == 8, "fp64 records (handles that store fp32 keep their own kernels)");
  static_assert(DEPTH >= 2, "one barrier per step needs two ring slots");
  using GR = Mfma16FwdGroup<G>;
  static_assert(GR::lds_bytes(DEPTH) <= 160 * 1024, "LDS of one CU");
  extern __shared__ __attribute__((aligned(16))) double mf_fwd_group_lds[];
  mf_f64x2* const ring = (mf_f64x2*)mf_fwd_group_lds;
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  double* const img = mf_fwd_group_lds + (size_t)DEPTH * GR::SLOT * 2 + (size_t)wv * GR::IMG;   // this wave's own image
  const int ngrp = a.batch / G;
  const int grp = mf_problem(blockIdx.x, ngrp);
  if (grp >= ngrp) return;   // the whole workgroup
  const int b0 = grp * G, b = b0 + wv;
  const int N = a.N;
  S* __restrict__ xuy = a.xuy + (size_t)b * a.xuy_bs;
  S* __restrict__ trash = a.trash + (size_t)b * MF_OUT;
  const Mfma16FwdRole ro = mfma16_fwd_role(lane);

  // this thread's chunk of every round: which run, and where inside it (past the end: the last chunk again, same bytes to the same place)
  const mf_f64x2* src[GR::ROUNDS];
  int64_t sstride[GR::ROUNDS];
  int dst[GR::ROUNDS];
#pragma unroll
  for (int r = 0; r < GR::ROUNDS; ++r) {
    int c = r * GR::T + t;
    c = c < GR::CIN ? c : GR::CIN - 1;
    dst[r] = c;
    const bool dyn = c < G * GR::CD;
    src[r] = dyn ? (const mf_f64x2*)(a.in + (size_t)b0 * MF_DYN) + c : (const mf_f64x2*)(a.out + (size_t)b0 * MF_OUT) + (c - G * GR::CD);
    sstride[r] = (dyn ? a.in_ks : a.out_ks) / 2;
  }
  mf_f64x2 regs[DEPTH][GR::ROUNDS];
  auto fetch = [&](mf_f64x2* rg, int k) {   // knot point k, clamped: the padding steps re-read the last record
    const int64_t kk = k < N ? k : N - 1;
#pragma unroll
    for (int r = 0; r < GR::ROUNDS; ++r) rg[r] = src[r][kk * sstride[r]];
  };

  double xcur = (double)a.x0[(size_t)b * 12 + ro.row];   // meaningful in group 0: x_k[row]
#pragma unroll
  for (int dd = 0; dd < DEPTH; ++dd) fetch(regs[dd], dd);
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): drain before the loop (see the backward kernel), or every step waits for all its requests

  const int Npad = ((N + DEPTH - 1) / DEPTH) * DEPTH;
  for (int k0 = 0; k0 < Npad; k0 += DEPTH) {
#pragma unroll
    for (int dd = 0; dd < DEPTH; ++dd) {
      const int k = k0 + dd;
      const bool live = k < N;     // padding steps (N not a multiple of DEPTH) compute on a clamped record
      mf_f64x2* const slot = ring + dd * GR::SLOT;
#pragma unroll
      for (int r = 0; r < GR::ROUNDS; ++r) slot[dst[r]] = regs[dd][r];
      fetch(regs[dd], k + DEPTH);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();          // the slot is whole (a bare barrier: the requests stay in flight across it)
      asm volatile("" ::: "memory");
      // this wave's own record out of the slot, in the lane order of mfma16_fwd_load, and its 17-pitch image
      {
        const double* __restrict__ rec = (const double*)slot + wv * MF_DYN;
        const double* __restrict__ orec = (const double*)slot + G * MF_DYN + wv * MF_OUT;
        Mfma16FwdRegs rr;
        mfma16_fwd_load(rr, rec, orec, lane);
        mfma16_fwd_stage(rr, img, lane);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // one wave, in-order LDS: the image is visible to the wave's own reads
      __builtin_amdgcn_wave_barrier();
      S* __restrict__ o = live ? xuy + (size_t)k * a.xuy_ks : trash;
      const double xn = mfma16_fwd_step<S>(img, nullptr, ro, lane, xcur, o);
      xcur = live ? xn : xcur;
    }
  }
  mfma16_fwd_terminal<S>(a.outn + (size_t)b * MF_TERM, ro, xcur, xuy + (size_t)N * a.xuy_ks);
}

}  // namespace altro_hip
