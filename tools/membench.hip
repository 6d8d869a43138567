// tools/membench.hip -- HBM streaming probes on MI355X: what bandwidth can the backward sweep's access
// pattern reach with NO arithmetic?  (Practical roof next to the 8 TB/s datasheet number.)
//   hipcc --offload-arch=gfx950 -O3 tools/membench.hip -o /tmp/membench && /tmp/membench
//   /tmp/membench multi    just the problems-per-wave table (profiles/r03g_membench_multi.txt)
//   /tmp/membench group    just the workgroup-run table: G adjacent problems' records fetched as contiguous runs (profiles/r07a_*, r08a_*)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__global__ void copy16(const double2* __restrict__ src, double2* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
__global__ void read16(const double2* __restrict__ src, double* sink, size_t n) {
  double acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { double2 v = src[i]; acc += v.x + v.y; }
  if (acc == 1.2345) sink[0] = acc;
}
__global__ void write16nt(double2* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    __builtin_nontemporal_store(1.0, &dst[i].x); __builtin_nontemporal_store(2.0, &dst[i].y);
  }
}
__global__ void write8(double* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = 1.0;
}
__global__ void write8nt(double* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) __builtin_nontemporal_store(1.0, &dst[i]);
}
__global__ void read8(const double* __restrict__ src, double* sink, size_t n) {
  double acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc += src[i];
  if (acc == 1.2345) sink[0] = acc;
}
__global__ void write16(double2* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = make_double2(1.0, 2.0);
}

// wave-per-problem record streaming: per step read RIN doubles, write ROUT doubles, 8 B per lane,
// software prefetch DEPTH steps ahead.  LAY = 0: [b][k], 1: [k][b].
template <int DEPTH, int LAY, int W>
__global__ __launch_bounds__(64) void stream_records(const double* __restrict__ in, double* __restrict__ out, int N, int batch) {
  constexpr int RIN = 428, ROUT = 208;
  const int lane = threadIdx.x, b = blockIdx.x;
  const size_t in_bs = LAY ? RIN : (size_t)N * RIN, in_ks = LAY ? (size_t)batch * RIN : RIN;
  const size_t out_bs = LAY ? ROUT : (size_t)N * ROUT, out_ks = LAY ? (size_t)batch * ROUT : ROUT;
  const double* ip = in + b * in_bs;
  double* op = out + b * out_bs;
  double buf[DEPTH + 1][7];
  auto load = [&](double* r, int k) {
    const double* rec = ip + (size_t)k * in_ks;
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = rec[c * 64 + lane];
    r[6] = rec[384 + (lane < 44 ? lane : 43)];
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load(buf[d], N - 1 - d);
  double acc = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    int kp = k - DEPTH; if (kp < 0) kp = 0;
    load(buf[DEPTH], kp);
    double s = 0;
#pragma unroll
    for (int c = 0; c < 7; ++c) s += buf[0][c];
    acc += s;
    double* o = op + (size_t)k * out_ks;
#pragma unroll
    for (int c = 0; c < 3; ++c) { if (W) __builtin_nontemporal_store(s + c, &o[c * 64 + lane]); else o[c * 64 + lane] = s + c; }
    if (W) __builtin_nontemporal_store(acc, &o[192 + (lane & 15)]); else o[192 + (lane & 15)] = acc;
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int c = 0; c < 7; ++c) buf[d][c] = buf[d + 1][c];
  }
}

// forward-sweep pattern: per step read two fully-used records (204 + RO doubles: RO = 208 full, 144 packed), write 28 doubles;
// MAP = 1: the XCD-aware block -> problem mapping
template <int DEPTH, int RO = 208, int MAP = 0>
__global__ __launch_bounds__(64) void stream_fwd(const double* __restrict__ dyn, const double* __restrict__ outr, double* __restrict__ xuy, int N, int batch) {
  constexpr int CO = RO / 64;   // whole 64-lane pieces of the second record; its last 16 elements ride with f
  static_assert(RO == CO * 64 + 16 && CO <= 3, "208 or 144");
  const int lane = threadIdx.x;
  const int b = MAP ? (int)((blockIdx.x & 7) * (batch / 8) + (blockIdx.x >> 3)) : (int)blockIdx.x;
  double buf[DEPTH + 1][7];
  auto load = [&](double* r, int k) {
    const double* d = dyn + ((size_t)k * batch + b) * 204;
    const double* o = outr + ((size_t)k * batch + b) * RO;
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = d[c * 64 + lane];
#pragma unroll
    for (int c = 0; c < 3; ++c) r[3 + c] = c < CO ? o[c * 64 + lane] : 0.0;
    r[6] = o[CO * 64 + (lane & 15)] + d[192 + (lane < 12 ? lane : 11)];
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load(buf[d], d);
  double acc = 0.0;
  for (int k = 0; k < N; ++k) {
    int kp = k + DEPTH; if (kp >= N) kp = N - 1;
    load(buf[DEPTH], kp);
    double s = 0;
#pragma unroll
    for (int c = 0; c < 7; ++c) s += buf[0][c];
    acc += s;
    xuy[((size_t)k * batch + b) * 28 + (lane % 28)] = acc;
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int c = 0; c < 7; ++c) buf[d][c] = buf[d + 1][c];
  }
}


// generic record streaming, [k][b] layout: per step read RIN doubles and write ROUT doubles (8 B per lane, unit
// stride), prefetch one step ahead.  Used to price symmetric-packed record layouts before building them.
template <int RIN, int ROUT>
__global__ __launch_bounds__(64) void stream_generic(const double* __restrict__ in, double* __restrict__ out, int N, int batch) {
  constexpr int LI = (RIN + 63) / 64, LO = (ROUT + 63) / 64;
  const int lane = threadIdx.x, b = blockIdx.x;
  double cur[LI], nxt[LI];
  auto load = [&](double* r, int k) {
    const double* rec = in + ((size_t)k * batch + b) * RIN;
#pragma unroll
    for (int c = 0; c < LI; ++c) { int e = c * 64 + lane; r[c] = rec[e < RIN ? e : RIN - 1]; }
  };
  load(cur, N - 1);
  double acc = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    load(nxt, k > 0 ? k - 1 : 0);
    double s = 0;
#pragma unroll
    for (int c = 0; c < LI; ++c) s += cur[c];
    acc += s;
    double* o = out + ((size_t)k * batch + b) * ROUT;
#pragma unroll
    for (int c = 0; c < LO; ++c) { int e = c * 64 + lane; o[e < ROUT ? e : ROUT - 1] = acc + c; }
#pragma unroll
    for (int c = 0; c < LI; ++c) cur[c] = nxt[c];
  }
}

// the same with 16 bytes per lane (double2 loads and stores; RIN, ROUT multiples of 2)
template <int RIN, int ROUT>
__global__ __launch_bounds__(64) void stream_generic16(const double* __restrict__ in, double* __restrict__ out, int N, int batch) {
  constexpr int PI = RIN / 2, PO = ROUT / 2;
  constexpr int LI = (PI + 63) / 64, LO = (PO + 63) / 64;
  const int lane = threadIdx.x, b = blockIdx.x;
  double2 cur[LI], nxt[LI];
  auto load = [&](double2* r, int k) {
    const double2* rec = (const double2*)(in + ((size_t)k * batch + b) * RIN);
#pragma unroll
    for (int c = 0; c < LI; ++c) { int e = c * 64 + lane; r[c] = rec[e < PI ? e : PI - 1]; }
  };
  load(cur, N - 1);
  double acc = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    load(nxt, k > 0 ? k - 1 : 0);
    double s = 0;
#pragma unroll
    for (int c = 0; c < LI; ++c) s += cur[c].x + cur[c].y;
    acc += s;
    double2* o = (double2*)(out + ((size_t)k * batch + b) * ROUT);
#pragma unroll
    for (int c = 0; c < LO; ++c) { int e = c * 64 + lane; o[e < PO ? e : PO - 1] = make_double2(acc + c, acc); }
#pragma unroll
    for (int c = 0; c < LI; ++c) cur[c] = nxt[c];
  }
}

// generic record streaming with (MAP) the XCD-aware block -> problem mapping and WPB waves (adjacent problems) per block
template <int RIN, int ROUT, int MAP, int WPB>
__global__ __launch_bounds__(64 * WPB) void stream_mapped(const double* __restrict__ in, double* __restrict__ out, int N, int batch) {
  constexpr int LI = (RIN + 63) / 64, LO = (ROUT + 63) / 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nblk = batch / WPB, chunk = nblk / 8;
  const int blk = MAP ? (int)((blockIdx.x & 7) * chunk + (blockIdx.x >> 3)) : (int)blockIdx.x;
  const int b = blk * WPB + wv;
  double cur[LI], nxt[LI];
  auto load = [&](double* r, int k) {
    const double* rec = in + ((size_t)k * batch + b) * RIN;
#pragma unroll
    for (int c = 0; c < LI; ++c) { int e = c * 64 + lane; r[c] = rec[e < RIN ? e : RIN - 1]; }
  };
  load(cur, N - 1);
  double acc = 0.0;
  for (int k = N - 1; k >= 0; --k) {
    load(nxt, k > 0 ? k - 1 : 0);
    double s = 0;
#pragma unroll
    for (int c = 0; c < LI; ++c) s += cur[c];
    acc += s;
    double* o = out + ((size_t)k * batch + b) * ROUT;
#pragma unroll
    for (int c = 0; c < LO; ++c) { int e = c * 64 + lane; o[e < ROUT ? e : ROUT - 1] = acc + c; }
#pragma unroll
    for (int c = 0; c < LI; ++c) cur[c] = nxt[c];
  }
}

// P adjacent problems per wave ([k][b] slabs: their records are one contiguous run of P * RIN doubles), V doubles per lane
// and access (8 or 16 bytes), records requested DEPTH knot points ahead, XCD-aware block -> problem mapping.  Prices the
// "two problems per wave, two doubles per lane" form of the fp64 backward sweep before it is built.
template <int RIN, int ROUT, int P, int V, int DEPTH>
__global__ __launch_bounds__(64) void stream_multi(const double* __restrict__ in, double* __restrict__ out, int N, int batch) {
  constexpr int EI = P * RIN / V, EO = P * ROUT / V;            // V-wide elements per knot point
  constexpr int LI = (EI + 63) / 64, LO = (EO + 63) / 64;
  typedef double vec __attribute__((ext_vector_type(V)));
  const int lane = threadIdx.x;
  const int nblk = batch / P, chunk = nblk / 8;
  const int blk = (int)((blockIdx.x & 7) * chunk + (blockIdx.x >> 3));
  const size_t b0 = (size_t)blk * P;
  vec ring[DEPTH][LI];
  auto load = [&](vec* r, int k) {
    const vec* rec = (const vec*)(in + ((size_t)k * batch + b0) * RIN);
#pragma unroll
    for (int c = 0; c < LI; ++c) { int e = c * 64 + lane; r[c] = rec[e < EI ? e : EI - 1]; }
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load(ring[d], N - 1 - d > 0 ? N - 1 - d : 0);
  double acc = 0.0;
  for (int k0 = N - 1; k0 >= 0; k0 -= DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const int k = k0 - d;
      if (k < 0) break;
      double s = 0;
#pragma unroll
      for (int c = 0; c < LI; ++c)
#pragma unroll
        for (int v = 0; v < V; ++v) s += ring[d][c][v];
      acc += s;
      load(ring[d], k - DEPTH > 0 ? k - DEPTH : 0);
      vec* o = (vec*)(out + ((size_t)k * batch + b0) * ROUT);
#pragma unroll
      for (int c = 0; c < LO; ++c) {
        int e = c * 64 + lane;
        vec w;
#pragma unroll
        for (int v = 0; v < V; ++v) w[v] = acc + c + v;
        o[e < EO ? e : EO - 1] = w;
      }
    }
  }
}

// ---- workgroup-contiguous runs: one block of G waves owns G adjacent problems -----------------------------------------
// In the [k][b] slabs the G problems' records of one knot point are one contiguous run per array (G * RA and G * RB doubles).
// The block's 64 * G threads fetch both runs as consecutive 16-byte chunks (thread t: chunk t, then t + 64 G, ...) into an
// LDS ring of DEPTH slots, knot point k + DEPTH while knot point k is consumed; wave w then reads its own record out of the
// slot.  DMA = 1: __builtin_amdgcn_global_load_lds (16 bytes per lane, no VGPR destination), counted vmcnt waits and raw
// s_barrier, so that DEPTH - 1 knot points stay in flight across the barriers.  DMA = 0: global_load_dwordx4 into a register
// ring, ds_write_b128 into the slot at the step that consumes it.  OUTRUN = 0: every wave stores WOUT doubles itself (the
// forward sweep's x | y | u); OUTRUN = 1: the waves put their WOUT-double records into an LDS stage and the block stores the
// G-problem run as 16-byte chunks (the backward sweep's OUT records); OUTRUN = 2: every wave stores its whole WOUT-double record
// itself, 8 bytes per lane.  DIR = 1 walks the horizon backwards.  No arithmetic.
typedef double mb_f64x2 __attribute__((ext_vector_type(2)));
template <int NCNT>
__device__ __forceinline__ void mb_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NCNT) : "memory"); }
__device__ __forceinline__ void mb_barrier() {   // LDS traffic of this wave retired, then the bare barrier: no vmcnt(0)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// a wave that issues L loads and S stores per step, loads first: the loads of step k have landed when at most the
// (DEPTH - 1) younger steps' operations and step k - DEPTH's own stores are outstanding; during the first DEPTH steps
// fewer stores sit in the queue, so the count without them is used
template <int L, int S, int DEPTH>
__device__ __forceinline__ void mb_wait_step(bool first) {
  if (first) mb_wait_vm<(DEPTH - 1) * L>(); else mb_wait_vm<(DEPTH - 1) * (L + S) + S>();
}
template <int RA, int RB, int WOUT, int OUTRUN, int DIR, int G, int DEPTH, int DMA>
__global__ __launch_bounds__(64 * G) void stream_group(const double* __restrict__ ina, const double* __restrict__ inb,
                                                       double* __restrict__ out, int N, int batch) {
  constexpr int T = 64 * G;
  constexpr int CA = RA / 2, CB = RB / 2;             // 16-byte chunks per record
  constexpr int CIN = G * (CA + CB);                  // chunks per knot point and group: run A, then run B
  constexpr int ROUNDS = (CIN + T - 1) / T;
  constexpr int LASTW = (CIN - (ROUNDS - 1) * T + 63) / 64;   // waves that have chunks in the last round
  constexpr int SLOT = ((CIN + 63) / 64) * 64;        // slot pitch in chunks: whole wave-instructions
  constexpr int COUT = OUTRUN == 1 ? G * WOUT / 2 : 0;     // chunks of the output run
  constexpr int OROUNDS = OUTRUN == 1 ? (COUT + T - 1) / T : (OUTRUN == 2 ? (WOUT + 63) / 64 : 1);
  constexpr int OLASTW = OUTRUN == 1 ? (COUT - (OROUNDS - 1) * T) / 64 : G;
  static_assert(RA % 2 == 0 && RB % 2 == 0 && (OUTRUN != 1 || COUT % 64 == 0), "16-byte chunks, whole wave-instructions");
  static_assert(LASTW >= 1 && LASTW <= G && OLASTW >= 1 && OLASTW <= G, "wave classes");
  static_assert((DEPTH * SLOT + COUT) * 16 <= 160 * 1024, "LDS of one CU");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  mb_f64x2* const ring = (mb_f64x2*)smem;
  double* const ostage = (double*)(ring + DEPTH * SLOT);
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ngrp = batch / G, chunk = ngrp / 8;
  const int grp = (int)((blockIdx.x & 7) * chunk + (blockIdx.x >> 3));
  const size_t b0 = (size_t)grp * G;
  const bool lastw = wv < LASTW, olastw = wv < OLASTW;
  // this thread's chunk of every round: which run, and where inside it (DMA = 0 clamps past the end: same bytes, same place)
  const mb_f64x2* src[ROUNDS];
  size_t sstride[ROUNDS];
  int dst[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    int c = r * T + t;
    dst[r] = DMA ? c : (c < CIN ? c : CIN - 1);
    c = c < CIN ? c : CIN - 1;
    const bool isa = c < G * CA;
    src[r] = isa ? (const mb_f64x2*)(ina + b0 * RA) + c : (const mb_f64x2*)(inb + b0 * RB) + (c - G * CA);
    sstride[r] = (size_t)batch * (isa ? CA : CB);
  }
  auto knot = [&](int step) { const int s = step < N ? step : N - 1; return DIR ? N - 1 - s : s; };
  mb_f64x2 regs[DMA ? 1 : DEPTH][ROUNDS];
  auto fetch = [&](int d, int step) {
    const size_t kk = knot(step);
    if constexpr (DMA) {
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) {
        if (r < ROUNDS - 1 || LASTW == G || lastw)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[r] + kk * sstride[r]),
                                           (__attribute__((address_space(3))) void*)(ring + d * SLOT + r * T + wv * 64), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int r = 0; r < ROUNDS; ++r) regs[d][r] = src[r][kk * sstride[r]];
    }
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) fetch(d, d);
  // register ring: drain before the loop -- hipcc merges the pre-header's pending loads into the loop header's count and would
  // wait vmcnt(0) at the top of every trip (the LDS-DMA form counts for itself and keeps its requests in flight)
  if constexpr (!DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  double acc = 0.0;
  for (int k0 = 0; k0 < N; k0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const int k = k0 + d;
      if (k >= N) break;   // the same for every wave of every block
      const size_t kk = knot(k);
      if constexpr (DMA) {
        const bool first = k < DEPTH;
        if (LASTW == G || lastw) {
          if (olastw) mb_wait_step<ROUNDS, OROUNDS, DEPTH>(first); else mb_wait_step<ROUNDS, OROUNDS - 1, DEPTH>(first);
        } else {
          if (olastw) mb_wait_step<ROUNDS - 1, OROUNDS, DEPTH>(first); else mb_wait_step<ROUNDS - 1, OROUNDS - 1, DEPTH>(first);
        }
      } else {
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) ring[d * SLOT + dst[r]] = regs[d][r];
      }
      mb_barrier();                                   // the slot is whole
      const double* ra = (const double*)(ring + d * SLOT) + wv * RA;
      const double* rb = (const double*)(ring + d * SLOT) + G * RA + wv * RB;
      double s = 0;
#pragma unroll
      for (int c = 0; c < (RA + 63) / 64; ++c) { const int e = c * 64 + lane; s += ra[e < RA ? e : RA - 1]; }
#pragma unroll
      for (int c = 0; c < (RB + 63) / 64; ++c) { const int e = c * 64 + lane; s += rb[e < RB ? e : RB - 1]; }
      acc += s;
      if constexpr (OUTRUN == 1) {
#pragma unroll
        for (int c = 0; c < (WOUT + 63) / 64; ++c) { const int e = c * 64 + lane; ostage[wv * WOUT + (e < WOUT ? e : WOUT - 1)] = acc + c; }
      }
      mb_barrier();                                   // every wave has read the slot: it may be refilled
      fetch(d, k + DEPTH);
      if constexpr (OUTRUN == 1) {
        mb_f64x2* orun = (mb_f64x2*)(out + (kk * batch + b0) * WOUT);
#pragma unroll
        for (int r = 0; r < OROUNDS; ++r) {
          const int c = r * T + t;
          if constexpr (DMA) { if (r < OROUNDS - 1 || OLASTW == G || olastw) orun[c] = ((const mb_f64x2*)ostage)[c]; }
          else { const int cc = c < COUT ? c : COUT - 1; orun[cc] = ((const mb_f64x2*)ostage)[cc]; }
        }
      } else if constexpr (OUTRUN == 2) {             // every wave stores its whole WOUT-double record itself, 8 bytes per lane
        double* o = out + (kk * batch + b0 + wv) * WOUT;
#pragma unroll
        for (int c = 0; c < (WOUT + 63) / 64; ++c) { const int e = c * 64 + lane; o[e < WOUT ? e : WOUT - 1] = acc + c; }
      } else {
        out[(kk * batch + b0 + wv) * WOUT + (lane % WOUT)] = acc;
      }
    }
  }
}
// The same runs behind a register stage ONE knot point deep and a two-slot LDS ring (12 staging VGPRs at G = 16 instead of
// 24): in step s every wave first reads its own records of knot point s out of slot s % 2, then every thread writes the
// chunks it holds (knot point s + 1, requested one step ago) into slot (s + 1) % 2, requests knot point s + 2 into the freed
// registers and crosses ONE bare barrier.  Slot (s + 1) % 2 was last read in step s - 1, before that step's barrier.
// Chunks are dealt to whole waves: every wave-instruction lies inside one run, so its address is a wave-uniform base
// (stepped per trip on the scalar unit) plus one 32-bit per-thread offset.  OUTRUN = 1: the OUT run leaves through a
// double-buffered LDS stage, one step late, as 16-byte chunks; 2: every wave stores its own record, 8 bytes per lane.
template <int RA, int RB, int WOUT, int OUTRUN, int G>
struct StageOne {
  static constexpr int T = 64 * G, NA = G * RA / 2, NB = G * RB / 2, CIN = NA + NB;
  static constexpr int FA = NA / T, REMA = NA - FA * T, WA = (REMA + 63) / 64;   // full rounds of run A; waves of the mixed round on run A
  static constexpr int B0 = REMA ? T - 64 * WA : 0;                            // chunks of run B fetched in the mixed round
  static constexpr int ROUNDS = FA + (REMA ? 1 : 0) + (NB - B0 + T - 1) / T;
  static constexpr int COUT = OUTRUN == 1 ? G * WOUT / 2 : 0;
  static constexpr size_t lds_bytes = (size_t)(2 * CIN + 2 * COUT) * 16;
};
template <int RA, int RB, int WOUT, int OUTRUN, int G>
__global__ __launch_bounds__(64 * G) void stream_group_stage1(const double* __restrict__ ina, const double* __restrict__ inb,
                                                              double* __restrict__ out, int N, int batch) {
  using SO = StageOne<RA, RB, WOUT, OUTRUN, G>;
  constexpr int T = SO::T, ROUNDS = SO::ROUNDS, CIN = SO::CIN, COUT = SO::COUT;
  constexpr int OROUNDS = (COUT + T - 1) / T;
  static_assert(SO::lds_bytes <= 160 * 1024, "LDS of one CU");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  mb_f64x2* const ring = (mb_f64x2*)smem;
  double* const ostage = (double*)(ring + 2 * CIN);
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int ngrp = batch / G, chunk = ngrp / 8;
  const int grp = (int)((blockIdx.x & 7) * chunk + (blockIdx.x >> 3));
  const size_t b0 = (size_t)grp * G;
  bool isa[ROUNDS];   // wave-uniform
  int off[ROUNDS];    // chunk inside its run (past the end: the last chunk again)
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    if (r < SO::FA) { isa[r] = true; off[r] = r * T + t; }
    else if (SO::REMA && r == SO::FA) {
      isa[r] = wv < SO::WA;
      off[r] = isa[r] ? (r * T + t < SO::NA ? r * T + t : SO::NA - 1) : t - 64 * SO::WA;
    } else {
      const int c = SO::B0 + (r - SO::FA - (SO::REMA ? 1 : 0)) * T + t;
      isa[r] = false; off[r] = c < SO::NB ? c : SO::NB - 1;
    }
  }
  const mb_f64x2* pa = (const mb_f64x2*)(ina + ((size_t)(N - 1) * batch + b0) * RA);   // knot point N - 1; stepped down per request
  const mb_f64x2* pb = (const mb_f64x2*)(inb + ((size_t)(N - 1) * batch + b0) * RB);
  const ptrdiff_t sa = (ptrdiff_t)batch * (RA / 2), sb = (ptrdiff_t)batch * (RB / 2);
  mb_f64x2 regs[ROUNDS];
  auto fetch = [&]() {
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) regs[r] = (isa[r] ? pa : pb)[off[r]];
  };
  auto stage = [&](int slot) {
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) ring[slot * CIN + (isa[r] ? 0 : SO::NA) + off[r]] = regs[r];
  };
  fetch();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  stage(0);
  if (N > 1) { pa -= sa; pb -= sb; }
  fetch();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drained before the loop (see stream_group)
  mb_barrier();
  double acc = 0.0;
  for (int s = 0; s < N; ++s) {
    const size_t kk = N - 1 - s;
    const int slot = s & 1;
    const double* ra = (const double*)(ring + slot * CIN) + wv * RA;
    const double* rb = (const double*)(ring + slot * CIN + SO::NA) + wv * RB;
    double sum = 0;
#pragma unroll
    for (int c = 0; c < (RA + 63) / 64; ++c) { const int e = c * 64 + lane; sum += ra[e < RA ? e : RA - 1]; }
#pragma unroll
    for (int c = 0; c < (RB + 63) / 64; ++c) { const int e = c * 64 + lane; sum += rb[e < RB ? e : RB - 1]; }
    acc += sum;
    stage(slot ^ 1);                       // knot point s + 1 (the last steps re-stage knot point 0: nobody reads it)
    if (s + 2 < N) { pa -= sa; pb -= sb; }
    fetch();
    if constexpr (OUTRUN == 1) {
      if (s > 0) {   // the run of step s - 1, whole since that step's barrier
        mb_f64x2* orun = (mb_f64x2*)(out + ((kk + 1) * batch + b0) * WOUT);
#pragma unroll
        for (int r = 0; r < OROUNDS; ++r) { const int c = r * T + t < COUT ? r * T + t : COUT - 1; orun[c] = ((const mb_f64x2*)ostage)[(slot ^ 1) * COUT + c]; }
      }
#pragma unroll
      for (int c = 0; c < (WOUT + 63) / 64; ++c) { const int e = c * 64 + lane; ostage[slot * COUT * 2 + wv * WOUT + (e < WOUT ? e : WOUT - 1)] = acc + c; }
    } else {
      double* o = out + (kk * batch + b0 + wv) * WOUT;
#pragma unroll
      for (int c = 0; c < (WOUT + 63) / 64; ++c) { const int e = c * 64 + lane; o[e < WOUT ? e : WOUT - 1] = acc + c; }
    }
    mb_barrier();
  }
  if constexpr (OUTRUN == 1) {
    mb_f64x2* orun = (mb_f64x2*)(out + b0 * WOUT);
#pragma unroll
    for (int r = 0; r < OROUNDS; ++r) { const int c = r * T + t < COUT ? r * T + t : COUT - 1; orun[c] = ((const mb_f64x2*)ostage)[((N - 1) & 1) * COUT + c]; }
  }
}
// the two record sets it is run on: the forward sweep's (DYN 204 + OUT 144 in, x | y | u 28 out per wave) and the backward sweep's
// (DYN 204 + COST 160 in, the OUT run of 144 out through LDS, last knot point first)
template <int G, int DEPTH, int DMA>
constexpr auto stream_fwd_group = stream_group<204, 144, 28, 0, 0, G, DEPTH, DMA>;
template <int G, int DEPTH, int DMA>
constexpr auto stream_bwd_group = stream_group<204, 160, 144, 1, 1, G, DEPTH, DMA>;
template <int RA, int RB, int WOUT, int OUTRUN, int DIR, int G, int DEPTH, int DMA>
static int stream_group_prepare(size_t* lds_bytes) {
  constexpr int CIN = G * (RA / 2 + RB / 2), SLOT = ((CIN + 63) / 64) * 64, COUT = OUTRUN == 1 ? G * WOUT / 2 : 0;
  *lds_bytes = (size_t)(DEPTH * SLOT + COUT) * 16;
  CK(hipFuncSetAttribute((const void*)stream_group<RA, RB, WOUT, OUTRUN, DIR, G, DEPTH, DMA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds_bytes));
  return 0;
}

int main(int argc, char** argv) {
  const bool only_group = argc > 1 && !strcmp(argv[1], "group");   // "group": just the workgroup-run table
  const bool only_multi = argc > 1 && !only_group;                 // any other argument: just the problems-per-wave table
  const int N = 256, batch = 4096;
  const size_t in_n = (size_t)batch * N * 428, out_n = (size_t)batch * N * 208;
  double *in, *out, *sink;
  CK(hipMalloc(&in, in_n * 8)); CK(hipMalloc(&out, out_n * 8)); CK(hipMalloc(&sink, 64));
  CK(hipMemset(in, 0, in_n * 8)); CK(hipMemset(out, 0, out_n * 8));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  auto timeit = [&](const char* name, double bytes, auto launch) {
    for (int i = 0; i < 3; ++i) launch();
    hipEventRecord(e0); for (int i = 0; i < 10; ++i) launch(); hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1); ms /= 10;
    printf("%-44s %8.3f ms  %8.1f GB/s\n", name, ms, bytes / ms / 1e6);
  };
  if (only_group) {
    const double* dyn = in;
    const double* outr = in + (size_t)batch * N * 204;   // the second input array: OUT records (forward) or COST records (backward)
    printf("# forward-sweep record set (204 + 144 r, 28 w doubles per knot point and problem, 3.15 GB), [k][b] slabs, XCD-aware mapping:\n"
           "# one block of G waves fetches its G problems' runs as 16-byte chunks into an LDS ring (no arithmetic)\n");
    for (int rep = 0; rep < 2; ++rep) {
      auto fwd = [&](const char* name, auto launch) { timeit(name, (double)batch * N * (348 + 28) * 8, launch); };
      size_t l;
#define FWD_GROUP(G, DEPTH, DMA, label)                                                                                  \
      if (stream_group_prepare<204, 144, 28, 0, 0, G, DEPTH, DMA>(&l)) return 1;                                         \
      fwd(label, [&] { stream_fwd_group<G, DEPTH, DMA><<<batch / G, 64 * G, l>>>(dyn, outr, out, N, batch); });
      FWD_GROUP(8, 2, 1, "group G = 8,  depth 2, LDS-DMA")
      FWD_GROUP(8, 3, 1, "group G = 8,  depth 3, LDS-DMA")
      FWD_GROUP(16, 2, 1, "group G = 16, depth 2, LDS-DMA")
      FWD_GROUP(16, 3, 1, "group G = 16, depth 3, LDS-DMA")
      FWD_GROUP(8, 2, 0, "group G = 8,  depth 2, load + ds_write")
      FWD_GROUP(8, 3, 0, "group G = 8,  depth 3, load + ds_write")
      FWD_GROUP(16, 2, 0, "group G = 16, depth 2, load + ds_write")
      FWD_GROUP(16, 3, 0, "group G = 16, depth 3, load + ds_write")
#undef FWD_GROUP
      fwd("today: stream_mapped<348, 28> 1/wave depth 1", [&] { stream_mapped<348, 28, 1, 1><<<batch, 64>>>(in, out, N, batch); });
      fwd("today: stream_fwd packed, mapped, depth 3", [&] { stream_fwd<3, 144, 1><<<batch, 64>>>(dyn, outr, out, N, batch); });
      fwd("today: stream_fwd packed, mapped, depth 1", [&] { stream_fwd<1, 144, 1><<<batch, 64>>>(dyn, outr, out, N, batch); });
    }
    printf("# backward-sweep record set (204 + 160 r, 144 w doubles, 4.26 GB) in the group form: the OUT run leaves through LDS\n");
    for (int rep = 0; rep < 2; ++rep) {
      auto bwd = [&](const char* name, auto launch) { timeit(name, (double)batch * N * (364 + 144) * 8, launch); };
      size_t l;
#define BWD_GROUP(G, DEPTH, DMA, label)                                                                                  \
      if (stream_group_prepare<204, 160, 144, 1, 1, G, DEPTH, DMA>(&l)) return 1;                                        \
      bwd(label, [&] { stream_bwd_group<G, DEPTH, DMA><<<batch / G, 64 * G, l>>>(dyn, outr, out, N, batch); });
      BWD_GROUP(8, 2, 1, "backward group G = 8,  depth 2, LDS-DMA")
      BWD_GROUP(16, 2, 1, "backward group G = 16, depth 2, LDS-DMA")
      BWD_GROUP(16, 3, 1, "backward group G = 16, depth 3, LDS-DMA")
      BWD_GROUP(16, 2, 0, "backward group G = 16, depth 2, load + ds_write")
      // the OUT records stored by each wave itself, 8 bytes per lane, and the register stage one knot point deep (profiles/r08a_*)
#define BWD_GROUP_DIRECT(G, DEPTH, DMA, label)                                                                           \
      if (stream_group_prepare<204, 160, 144, 2, 1, G, DEPTH, DMA>(&l)) return 1;                                        \
      bwd(label, [&] { stream_group<204, 160, 144, 2, 1, G, DEPTH, DMA><<<batch / G, 64 * G, l>>>(dyn, outr, out, N, batch); });
      BWD_GROUP_DIRECT(16, 2, 1, "backward group G = 16, depth 2, LDS-DMA, OUT per wave")
      BWD_GROUP_DIRECT(16, 2, 0, "backward group G = 16, depth 2, load + ds_write, OUT per wave")
#define BWD_STAGE1(OUTRUN, label)                                                                                        \
      {                                                                                                                  \
        const auto kernel = stream_group_stage1<204, 160, 144, OUTRUN, 16>;                                              \
        l = StageOne<204, 160, 144, OUTRUN, 16>::lds_bytes;                                                              \
        CK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l));                \
        bwd(label, [&] { kernel<<<batch / 16, 64 * 16, l>>>(dyn, outr, out, N, batch); });                               \
      }
      BWD_STAGE1(1, "backward group G = 16, stage 1 deep + 2 slots")
      BWD_STAGE1(2, "backward group G = 16, stage 1 deep + 2 slots, OUT per wave")
#undef BWD_STAGE1
#undef BWD_GROUP_DIRECT
#undef BWD_GROUP
      bwd("today: stream_mapped<364, 144> 1/wave depth 1", [&] { stream_mapped<364, 144, 1, 1><<<batch, 64>>>(in, out, N, batch); });
    }
    return 0;
  }
  if (only_multi) {
    auto gen = [&](const char* name, auto launch) { timeit(name, (double)batch * N * (364 + 144) * 8, launch); };
    printf("# backward-sweep record set (364 r + 144 w doubles per knot point and problem, 4.26 GB), [k][b] slabs, XCD-aware mapping:\n"
           "# problems per wave x bytes per lane x prefetch depth (no arithmetic)\n");
    for (int rep = 0; rep < 2; ++rep) {
      gen("1 problem/wave,  8 B/lane, depth 1", [&] { stream_multi<364, 144, 1, 1, 1><<<batch, 64>>>(in, out, N, batch); });
      gen("1 problem/wave,  8 B/lane, depth 2", [&] { stream_multi<364, 144, 1, 1, 2><<<batch, 64>>>(in, out, N, batch); });
      gen("1 problem/wave, 16 B/lane, depth 1", [&] { stream_multi<364, 144, 1, 2, 1><<<batch, 64>>>(in, out, N, batch); });
      gen("1 problem/wave, 16 B/lane, depth 2", [&] { stream_multi<364, 144, 1, 2, 2><<<batch, 64>>>(in, out, N, batch); });
      gen("2 problems/wave,  8 B/lane, depth 1", [&] { stream_multi<364, 144, 2, 1, 1><<<batch / 2, 64>>>(in, out, N, batch); });
      gen("2 problems/wave,  8 B/lane, depth 2", [&] { stream_multi<364, 144, 2, 1, 2><<<batch / 2, 64>>>(in, out, N, batch); });
      gen("2 problems/wave, 16 B/lane, depth 1", [&] { stream_multi<364, 144, 2, 2, 1><<<batch / 2, 64>>>(in, out, N, batch); });
      gen("2 problems/wave, 16 B/lane, depth 2", [&] { stream_multi<364, 144, 2, 2, 2><<<batch / 2, 64>>>(in, out, N, batch); });
      gen("2 problems/wave, 16 B/lane, depth 3", [&] { stream_multi<364, 144, 2, 2, 3><<<batch / 2, 64>>>(in, out, N, batch); });
      gen("4 problems/wave, 16 B/lane, depth 1", [&] { stream_multi<364, 144, 4, 2, 1><<<batch / 4, 64>>>(in, out, N, batch); });
      gen("4 problems/wave, 16 B/lane, depth 2", [&] { stream_multi<364, 144, 4, 2, 2><<<batch / 4, 64>>>(in, out, N, batch); });
      gen("today: stream_mapped 1/wave 8 B depth 1", [&] { stream_mapped<364, 144, 1, 1><<<batch, 64>>>(in, out, N, batch); });
    }
    return 0;
  }
  const size_t n16 = in_n / 2;
  timeit("copy16 in->in2 (full 3.59 GB r + w)", 2.0 * out_n * 8, [&] { copy16<<<256 * 8, 256>>>((const double2*)in, (double2*)out, out_n / 2); });
  timeit("read-only 16B/lane (3.59 GB)", 1.0 * in_n * 8, [&] { read16<<<256 * 8, 256>>>((const double2*)in, sink, n16); });
  timeit("write-only 16B/lane (1.74 GB)", 1.0 * out_n * 8, [&] { write16<<<256 * 8, 256>>>((double2*)out, out_n / 2); });
  timeit("write-only 16B/lane nontemporal", 1.0 * out_n * 8, [&] { write16nt<<<256 * 8, 256>>>((double2*)out, out_n / 2); });
  timeit("write-only 8B/lane", 1.0 * out_n * 8, [&] { write8<<<256 * 8, 256>>>(out, out_n); });
  timeit("write-only 8B/lane nontemporal", 1.0 * out_n * 8, [&] { write8nt<<<256 * 8, 256>>>(out, out_n); });
  timeit("write-only 16B/lane, 64K blocks", 1.0 * out_n * 8, [&] { write16<<<65536, 256>>>((double2*)out, out_n / 2); });
  timeit("read-only 8B/lane (3.59 GB)", 1.0 * in_n * 8, [&] { read8<<<256 * 8, 256>>>(in, sink, in_n); });
  timeit("read-only 16B/lane, 64K blocks", 1.0 * in_n * 8, [&] { read16<<<65536, 256>>>((const double2*)in, sink, n16); });
  const double rb = (double)in_n * 8 + (double)out_n * 8;
  timeit("records [b][k] depth1", rb, [&] { stream_records<1, 0, 0><<<batch, 64>>>(in, out, N, batch); });
  timeit("records [k][b] depth1", rb, [&] { stream_records<1, 1, 0><<<batch, 64>>>(in, out, N, batch); });
  timeit("records [k][b] depth2", rb, [&] { stream_records<2, 1, 0><<<batch, 64>>>(in, out, N, batch); });
  timeit("records [k][b] depth3", rb, [&] { stream_records<3, 1, 0><<<batch, 64>>>(in, out, N, batch); });
  timeit("records [k][b] depth1 nt stores", rb, [&] { stream_records<1, 1, 1><<<batch, 64>>>(in, out, N, batch); });
  timeit("records [b][k] depth1 nt stores", rb, [&] { stream_records<1, 0, 1><<<batch, 64>>>(in, out, N, batch); });
  timeit("records [b][k] depth3", rb, [&] { stream_records<3, 0, 0><<<batch, 64>>>(in, out, N, batch); });
  {
    const double fb = (double)batch * N * (204 + 208 + 28) * 8;
    timeit("forward pattern (412 r + 28 w) depth1", fb, [&] { stream_fwd<1><<<batch, 64>>>(in, in + (size_t)batch * N * 204, out, N, batch); });
    timeit("forward pattern (412 r + 28 w) depth3", fb, [&] { stream_fwd<3><<<batch, 64>>>(in, in + (size_t)batch * N * 204, out, N, batch); });
  }
  {
    auto gen = [&](const char* name, int rin, int rout, auto launch) {
      timeit(name, (double)batch * N * (rin + rout) * 8, launch);
    };
    gen("generic 428 r + 208 w (today's backward)", 428, 208, [&] { stream_generic<428, 208><<<batch, 64>>>(in, out, N, batch); });
    gen("generic 428 r + 144 w (P packed)", 428, 144, [&] { stream_generic<428, 144><<<batch, 64>>>(in, out, N, batch); });
    gen("generic 364 r + 144 w (Q and P packed)", 364, 144, [&] { stream_generic<364, 144><<<batch, 64>>>(in, out, N, batch); });
    gen("generic 360 r + 144 w (Q, R and P packed)", 360, 144, [&] { stream_generic<360, 144><<<batch, 64>>>(in, out, N, batch); });
    gen("generic 412 r + 28 w (today's forward)", 412, 28, [&] { stream_generic<412, 28><<<batch, 64>>>(in, out, N, batch); });
    gen("generic 348 r + 28 w (forward, P packed)", 348, 28, [&] { stream_generic<348, 28><<<batch, 64>>>(in, out, N, batch); });
    gen("16 B/lane: 364 r + 144 w", 364, 144, [&] { stream_generic16<364, 144><<<batch, 64>>>(in, out, N, batch); });
    gen("16 B/lane: 348 r + 28 w", 348, 28, [&] { stream_generic16<348, 28><<<batch, 64>>>(in, out, N, batch); });
    gen("8 B/lane again: 364 r + 144 w", 364, 144, [&] { stream_generic<364, 144><<<batch, 64>>>(in, out, N, batch); });
    gen("8 B/lane again: 348 r + 28 w", 348, 28, [&] { stream_generic<348, 28><<<batch, 64>>>(in, out, N, batch); });
    gen("364 r + 144 w, plain, 1 wave/block", 364, 144, [&] { stream_mapped<364, 144, 0, 1><<<batch, 64>>>(in, out, N, batch); });
    gen("364 r + 144 w, XCD map, 1 wave/block", 364, 144, [&] { stream_mapped<364, 144, 1, 1><<<batch, 64>>>(in, out, N, batch); });
    gen("364 r + 144 w, XCD map, 2 waves/block", 364, 144, [&] { stream_mapped<364, 144, 1, 2><<<batch / 2, 128>>>(in, out, N, batch); });
    gen("364 r + 144 w, XCD map, 4 waves/block", 364, 144, [&] { stream_mapped<364, 144, 1, 4><<<batch / 4, 256>>>(in, out, N, batch); });
    gen("364 r + 144 w, plain, 4 waves/block", 364, 144, [&] { stream_mapped<364, 144, 0, 4><<<batch / 4, 256>>>(in, out, N, batch); });
    gen("364 r + 144 w, XCD map, 8 waves/block", 364, 144, [&] { stream_mapped<364, 144, 1, 8><<<batch / 8, 512>>>(in, out, N, batch); });
  }
  return 0;
}
