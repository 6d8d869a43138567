// sweep_route.h against rows written out by hand from the launchers' arithmetic: which instantiation of generic_backward_kernel /
// generic_forward_kernel a launch takes; and, for every plan, which sweep kernel (sweep_route: id, name, ALTRO_HIP_SWEEP_* bits, grid,
// block) from the launchers it replaced.  Plain g++, nothing of the library linked.
//   carve of the backward kernel: (4 | 3) n^2 + 4 n m + 2 m^2 + 5 n + 3 m elements + 64 bytes; a compute unit holds
//   min(16, 163840 / carve) problems; late Q from batch 256 * per_cu(4 n^2 carve) + 1 up where the 3 n^2 carve holds more.
//     (24, 8) fp64: 2304 + 768 + 128 + 120 + 24 = 3344 el -> 26816 B (6 per CU); 2768 el -> 22208 B (7 per CU): late Q past 1536.
//     (33, 7) fp64: 4356 + 924 + 98 + 165 + 21 = 5564 el -> 44576 B (3); 4475 el -> 35864 B (4): past 768.
//     (40, 10) fp64: 6400 + 1600 + 200 + 200 + 30 = 8430 el -> 67504 B > 64 KB; 6830 el -> 54704 B: late Q at every batch.
//     (40, 6) fp64: 6400 + 960 + 72 + 200 + 18 = 7650 el -> 61264 B (2); 6050 el -> 48464 B (3): past 512, NOT at a batch of one.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <set>

#include "sweep_route.h"

using namespace altro_hip;

static int failures = 0;
static const unsigned ON = ALTRO_HIP_FORM_GENERIC_LATE_Q_ON, OFF = ALTRO_HIP_FORM_GENERIC_LATE_Q_OFF;
static const int LQ = ALTRO_HIP_SWEEP_LATE_Q, WS = ALTRO_HIP_SWEEP_GLOBAL_WORKSPACE, ST = ALTRO_HIP_SWEEP_FORWARD_STAGED;

static void backward(int n, int m, size_t esz, long long batch, unsigned forms, int variant, size_t bytes) {
  const GenericBackwardRoute r = generic_backward_route(n, m, esz, batch, forms);
  if (r.variant() != variant || r.bytes != bytes || r.late_q != ((variant & LQ) != 0) || r.big != ((variant & WS) != 0)) {
    ++failures;
    std::printf("backward (%d, %d) esz %zu batch %lld forms %#x: variant %d bytes %zu; want %d, %zu\n", n, m, esz, batch, forms, r.variant(), r.bytes, variant, bytes);
  }
}

// NEVER: no batch takes late Q unforced; ALWAYS: every batch does; else the last batch that does not
enum { NEVER = -1, ALWAYS = 0 };
static void threshold(int n, int m, size_t esz, long long last_without, size_t lds4, size_t lds3) {
  const long long probe[] = {1, 5, 144, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 1537, 1792, 1793, 2048, 2049, 2304, 2305, 2816, 2817, 3072, 3073, 4096, 65536, 1 << 20};
  for (long long b : probe) {
    const bool late = last_without == ALWAYS || (last_without != NEVER && b > last_without);
    backward(n, m, esz, b, 0u, late ? LQ : 0, late ? lds3 : lds4);
  }
  if (last_without > 0) {   // the two batches on either side of the rule
    backward(n, m, esz, last_without, 0u, 0, lds4);
    backward(n, m, esz, last_without + 1, 0u, LQ, lds3);
  }
  // forced: late Q wherever the three-block carve fits 64 KB, never with _OFF; both bits together (a solve's options on top of the
  // handle's: altro_hip_set_forms itself refuses the pair) are _ON
  for (long long b : {1LL, 5LL, 4096LL}) {
    backward(n, m, esz, b, ON, LQ, lds3);
    backward(n, m, esz, b, ON | OFF, LQ, lds3);
    backward(n, m, esz, b, OFF, lds4 > 65536 ? WS : 0, lds4);
  }
}
static void global_ws(int n, int m, size_t esz, size_t lds4) {   // neither carve fits: the work block in global memory whatever is asked
  for (long long b : {1LL, 3LL, 769LL, 4096LL})
    for (unsigned f : {0u, ON, OFF, ON | OFF}) backward(n, m, esz, b, f, WS, lds4);
}

static void forward(int n, int m, int want_y, size_t esz, size_t limit, int variant, size_t bytes) {
  const GenericForwardRoute r = generic_forward_route(n, m, want_y, esz, limit);
  if (r.variant() != variant || r.bytes != bytes) {
    ++failures;
    std::printf("forward (%d, %d) y %d esz %zu limit %zu: variant %d bytes %zu; want %d, %zu\n", n, m, want_y, esz, limit, r.variant(), r.bytes, variant, bytes);
  }
}

// ---- every plan: sweep_route ------------------------------------------------------------------------------------------------------
//   mf_grid(b) = 8 * ceil(b / 8): 5 -> 8, 8 -> 8, 9 -> 16, 16 -> 16, 17 -> 24; the group kernels launch mf_grid(b / 16) blocks of 1024, the
//   four-problem kernels mf_grid(b / 4) of 64.  Plan LANE: 8 * ceil(ceil(b / 64) / 8) blocks of 64, the quad forms with 16 for 64.
static std::set<int> ids;
static const SweepCall BWD{true, false}, BWD_MASKED{true, true}, FWD{false, false};
static void route(const char* what, const SweepShape& s, const SweepCall& c, int id, const char* name, int variant, unsigned grid, unsigned block,
                  size_t lds = 0, int error = SWEEP_OK) {
  const SweepRoute r = sweep_route(s, c);
  ids.insert(r.id);
  const char* got = sweep_kernel_name(r.id);
  if (r.id != id || !got || std::strcmp(got, name) != 0 || r.variant != variant || r.grid != grid || r.block != block || r.lds != lds || r.error != error) {
    ++failures;
    std::printf("%s (%s): id %#x %s variant %d grid %u block %u lds %zu error %d; want %#x %s %d %u %u %zu %d\n", what, c.backward ? "backward" : "forward", r.id,
                got ? got : "(null)", r.variant, r.grid, r.block, r.lds, r.error, id, name, variant, grid, block, lds, error);
  }
}
// plan MFMA16, (12, 4), the records in contiguous [k][b] slabs: DYN 204, COST 160, OUT 144 elements
static SweepShape tile16(bool f64, unsigned flags, unsigned forms, int batch, bool has_f = true) {
  const int64_t B = batch;
  return SweepShape{ALTRO_HIP_PLAN_MFMA16, f64, flags, forms, 12, 4, 2, batch, false, has_f, false, false, 204, B * 204, 160, B * 160, 144, B * 144};
}
static SweepShape lane(int n, int m, int batch, unsigned forms = 0, unsigned flags = 0) {
  return SweepShape{ALTRO_HIP_PLAN_LANE, true, flags, forms, n, m, 2, batch, false, true, false, false, 0, 0, 0, 0, 0, 0};
}
static SweepShape gen(int n, int m, int batch, bool g_tile, bool is_diag, bool g_mfma = false, bool f64 = true) {
  return SweepShape{ALTRO_HIP_PLAN_GENERIC, f64, 0, 0, n, m, 2, batch, is_diag, true, g_tile, g_mfma, 0, 0, 0, 0, 0, 0};
}

static void all_plans() {
  const unsigned SQ = ALTRO_HIP_STORE_QBLOCKS, PURE = ALTRO_HIP_F32_PURE;
  const int GROUP = ALTRO_HIP_SWEEP_GROUP;
  const char *B16 = "mfma16_backward_kernel", *F16 = "mfma16_forward_kernel", *BG = "mfma16_backward_group_kernel", *FG = "mfma16_forward_group_kernel";
  // plan MFMA16, fp64 backward: whole groups of 16 take the group kernel (8 = mf_grid(1) = mf_grid(2) workgroups of 16 waves)
  route("fp64 16", tile16(true, 0, 0, 16), BWD, SK_MFMA16_BACKWARD_GROUP | SF_HAS_F, BG, GROUP, 8, 1024);
  route("fp64 17", tile16(true, 0, 0, 17), BWD, SK_MFMA16_BACKWARD | SF_HAS_F, B16, 0, 24, 64);
  route("fp64 32", tile16(true, 0, 0, 32), BWD, SK_MFMA16_BACKWARD_GROUP | SF_HAS_F, BG, GROUP, 8, 1024);
  route("fp64 16 no f", tile16(true, 0, 0, 16, false), BWD, SK_MFMA16_BACKWARD_GROUP, BG, GROUP, 8, 1024);
  route("fp64 17 no f", tile16(true, 0, 0, 17, false), BWD, SK_MFMA16_BACKWARD, B16, 0, 24, 64);
  route("fp64 16 masked", tile16(true, 0, 0, 16), BWD_MASKED, SK_MFMA16_BACKWARD | SF_HAS_F, B16, 0, 16, 64);
  route("fp64 16 BACKWARD_WAVE", tile16(true, 0, ALTRO_HIP_FORM_BACKWARD_WAVE, 16), BWD, SK_MFMA16_BACKWARD | SF_HAS_F, B16, 0, 16, 64);
  route("fp64 16 BACKWARD_WAVE", tile16(true, 0, ALTRO_HIP_FORM_BACKWARD_WAVE, 16), FWD, SK_MFMA16_FORWARD_GROUP, FG, 0, 8, 1024);   // (the other sweep's form)
  route("fp64 16 STORE_QBLOCKS", tile16(true, SQ, 0, 16), BWD, SK_MFMA16_BACKWARD | SF_STORE_Q | SF_HAS_F, B16, 0, 16, 64);
  route("fp64 16 STORE_QBLOCKS no f", tile16(true, SQ, 0, 16, false), BWD, SK_MFMA16_BACKWARD | SF_STORE_Q, B16, 0, 16, 64);
  for (int field = 0; field < 6; ++field) {   // one stride of the six not that of the contiguous slabs
    SweepShape s = tile16(true, 0, 0, 16);
    int64_t* const st[6] = {&s.in_bs, &s.in_ks, &s.cin_bs, &s.cin_ks, &s.out_bs, &s.out_ks};
    *st[field] += 8;
    route("fp64 16 stride", s, BWD, SK_MFMA16_BACKWARD | SF_HAS_F, B16, 0, 16, 64);
    const bool cost = field == 2 || field == 3;   // the forward sweep does not read the COST records
    route("fp64 16 stride", s, FWD, cost ? SK_MFMA16_FORWARD_GROUP : SK_MFMA16_FORWARD, cost ? FG : F16, 0, cost ? 8 : 16, cost ? 1024 : 64);
  }
  // fp64 forward
  route("fp64 16", tile16(true, 0, 0, 16), FWD, SK_MFMA16_FORWARD_GROUP, FG, 0, 8, 1024);
  route("fp64 17", tile16(true, 0, 0, 17), FWD, SK_MFMA16_FORWARD, F16, 0, 24, 64);
  route("fp64 16 FORWARD_WAVE", tile16(true, 0, ALTRO_HIP_FORM_FORWARD_WAVE, 16), FWD, SK_MFMA16_FORWARD, F16, 0, 16, 64);
  route("fp64 16 FORWARD_WAVE", tile16(true, 0, ALTRO_HIP_FORM_FORWARD_WAVE, 16), BWD, SK_MFMA16_BACKWARD_GROUP | SF_HAS_F, BG, GROUP, 8, 1024);
  // fp32 records, fp64 tiles: the wave-per-problem kernels on floats, whatever the batch
  route("fp32 storage 16", tile16(false, 0, 0, 16), BWD, SK_MFMA16_BACKWARD | SF_HAS_F, B16, 0, 16, 64);
  route("fp32 storage 16", tile16(false, 0, 0, 16), FWD, SK_MFMA16_FORWARD, F16, 0, 16, 64);
  // pure fp32: whole quads four problems per wave (mf_grid(8 / 4) = 8), else one (mf_grid(9) = 16)
  route("pure fp32 8", tile16(false, PURE, 0, 8), BWD, SK_MFMA16_BACKWARD_F32X4 | SF_HAS_F, "mfma16_backward_f32x4_kernel", 0, 8, 64);
  route("pure fp32 8", tile16(false, PURE, 0, 8), FWD, SK_MFMA16_FORWARD_F32X4, "mfma16_forward_f32x4_kernel", 0, 8, 64);
  route("pure fp32 8 no f", tile16(false, PURE, 0, 8, false), BWD, SK_MFMA16_BACKWARD_F32X4, "mfma16_backward_f32x4_kernel", 0, 8, 64);
  route("pure fp32 9", tile16(false, PURE, 0, 9), BWD, SK_MFMA16_BACKWARD_F32 | SF_HAS_F, "mfma16_backward_f32_kernel", 0, 16, 64);
  route("pure fp32 9", tile16(false, PURE, 0, 9), FWD, SK_MFMA16_FORWARD, F16, 0, 16, 64);
  route("pure fp32 9 no f", tile16(false, PURE, 0, 9, false), BWD, SK_MFMA16_BACKWARD_F32, "mfma16_backward_f32_kernel", 0, 16, 64);
  route("pure fp32 8 STORE_QBLOCKS", tile16(false, PURE | SQ, 0, 8), BWD, SK_MFMA16_BACKWARD | SF_STORE_Q | SF_HAS_F, B16, 0, 8, 64);
  route("pure fp32 8 STORE_QBLOCKS", tile16(false, PURE | SQ, 0, 8), FWD, SK_MFMA16_FORWARD_F32X4, "mfma16_forward_f32x4_kernel", 0, 8, 64);
  route("pure fp32 16", tile16(false, PURE, 0, 16), FWD, SK_MFMA16_FORWARD_F32X4, "mfma16_forward_f32x4_kernel", 0, 8, 64);   // (no group form on fp32 records)
  route("fp64 16 F32_PURE", tile16(true, PURE, 0, 16), BWD, SK_MFMA16_BACKWARD_GROUP | SF_HAS_F, BG, GROUP, 8, 1024);         // (a flag only fp32 handles read)

  // plan LANE: (4, 2) and (2, 1) four lanes per problem up to 12288 problems, (4, 2) in both directions
  const unsigned ON = ALTRO_HIP_FORM_LANE_QUAD_ON, OFF = ALTRO_HIP_FORM_LANE_QUAD_OFF, FUSED = ALTRO_HIP_LANE_FUSED;
  const char *LB = "lane_backward_kernel", *LF = "lane_forward_kernel", *QB = "quad_backward_kernel", *QF = "quad_forward_kernel";
  route("(4, 2) 16", lane(4, 2, 16), BWD, SK_QUAD_BACKWARD, QB, 0, 8, 64);
  route("(4, 2) 16", lane(4, 2, 16), FWD, SK_QUAD_FORWARD, QF, 0, 8, 64);
  route("(2, 1) 16", lane(2, 1, 16), BWD, SK_QUAD2_BACKWARD, "quad2_backward_kernel", 0, 8, 64);
  route("(2, 1) 16", lane(2, 1, 16), FWD, SK_LANE_FORWARD, LF, 0, 8, 64);
  route("(3, 1) 16", lane(3, 1, 16), BWD, SK_LANE_BACKWARD, LB, 0, 8, 64);
  route("(3, 1) 16", lane(3, 1, 16), FWD, SK_LANE_FORWARD, LF, 0, 8, 64);
  // 12288 / 16 = 768 workgroups; 12289: ceil(12289 / 64) = 193 -> 25 eights = 200; forced quad: ceil(12289 / 16) = 769 -> 97 eights = 776
  route("(4, 2) 12288", lane(4, 2, 12288), BWD, SK_QUAD_BACKWARD, QB, 0, 768, 64);
  route("(4, 2) 12288", lane(4, 2, 12288), FWD, SK_QUAD_FORWARD, QF, 0, 768, 64);
  route("(4, 2) 12289", lane(4, 2, 12289), BWD, SK_LANE_BACKWARD, LB, 0, 200, 64);
  route("(4, 2) 12289", lane(4, 2, 12289), FWD, SK_LANE_FORWARD, LF, 0, 200, 64);
  route("(2, 1) 12289", lane(2, 1, 12289), BWD, SK_LANE_BACKWARD, LB, 0, 200, 64);
  route("(4, 2) 12289 QUAD_ON", lane(4, 2, 12289, ON), BWD, SK_QUAD_BACKWARD, QB, 0, 776, 64);
  route("(4, 2) 12289 QUAD_ON", lane(4, 2, 12289, ON), FWD, SK_QUAD_FORWARD, QF, 0, 776, 64);
  route("(4, 2) 16 QUAD_OFF", lane(4, 2, 16, OFF), BWD, SK_LANE_BACKWARD, LB, 0, 8, 64);
  route("(4, 2) 16 QUAD_OFF", lane(4, 2, 16, OFF), FWD, SK_LANE_FORWARD, LF, 0, 8, 64);
  route("(3, 1) 16 QUAD_ON", lane(3, 1, 16, ON), BWD, SK_LANE_BACKWARD, LB, 0, 8, 64);   // (no quad form of this shape)
  route("(4, 2) 16 fused", lane(4, 2, 16, 0, FUSED), BWD, SK_QUAD_BACKWARD | SF_FUSED, QB, 0, 8, 64);
  route("(4, 2) 16 fused", lane(4, 2, 16, 0, FUSED), FWD, SK_QUAD_FORWARD | SF_FUSED, QF, 0, 8, 64);
  route("(2, 1) 16 fused", lane(2, 1, 16, 0, FUSED), BWD, SK_QUAD2_BACKWARD | SF_FUSED, "quad2_backward_kernel", 0, 8, 64);
  route("(3, 1) 16 fused", lane(3, 1, 16, 0, FUSED), BWD, SK_LANE_BACKWARD | SF_FUSED, LB, 0, 8, 64);
  route("(3, 1) 16 fused", lane(3, 1, 16, 0, FUSED), FWD, SK_LANE_FORWARD | SF_FUSED, LF, 0, 8, 64);
  // grids: 65 problems are 2 lane workgroups / 5 quad workgroups -> one eight each; 1025 are 17 -> 24 and 65 -> 72
  route("(4, 2) 65 lane", lane(4, 2, 65, OFF), BWD, SK_LANE_BACKWARD, LB, 0, 8, 64);
  route("(4, 2) 65 quad", lane(4, 2, 65), BWD, SK_QUAD_BACKWARD, QB, 0, 8, 64);
  route("(4, 2) 1025 lane", lane(4, 2, 1025, OFF), FWD, SK_LANE_FORWARD, LF, 0, 24, 64);
  route("(4, 2) 1025 quad", lane(4, 2, 1025), FWD, SK_QUAD_FORWARD, QF, 0, 72, 64);
  route("(2, 1) 1025 quad", lane(2, 1, 1025), BWD, SK_QUAD2_BACKWARD, "quad2_backward_kernel", 0, 72, 64);

  // plan MFMA32 (plan GENERIC's arrays, g_tile), (13, 4), 5 problems: mf_grid(5) = 8 waves; a diagonal cost takes plan GENERIC's
  // backward kernel, a wave per problem on the 8008-byte carve, and the tile forward kernel
  route("(13, 4) dense", gen(13, 4, 5, true, false), BWD, SK_TILE32_BACKWARD, "tile32_backward_kernel", 0, 8, 64);
  route("(13, 4) dense", gen(13, 4, 5, true, false), FWD, SK_TILE32_FORWARD, "tile32_forward_kernel", 0, 8, 64);
  route("(13, 4) diagonal", gen(13, 4, 5, true, true), BWD, SK_GENERIC_BACKWARD, "generic_backward_kernel", 0, 5, 64, 8008);
  route("(13, 4) diagonal", gen(13, 4, 5, true, true), FWD, SK_TILE32_FORWARD, "tile32_forward_kernel", 0, 8, 64);
  route("(31, 1) dense", gen(31, 1, 5, true, false), FWD, SK_TILE32_FORWARD, "tile32_forward_kernel", 0, 8, 64);      // tiles (8, 1)
  route("(24, 8) dense", gen(24, 8, 5, true, false), FWD, SK_TILE32_FORWARD, "tile32_forward_kernel", 0, 8, 64);      // tiles (6, 2)
  // tiles (2, 1) and (8, 2) have no forward instantiation (no shape the plan takes has them)
  route("(8, 4) tile", gen(8, 4, 5, true, false), FWD, SK_TILE32_FORWARD, "tile32_forward_kernel", 0, 8, 64, 0, SWEEP_NO_FORWARD);
  route("(29, 5) tile", gen(29, 5, 5, true, false), FWD, SK_TILE32_FORWARD, "tile32_forward_kernel", 0, 8, 64, 0, SWEEP_NO_FORWARD);

  // plan GENERIC: the rows of generic_backward_route / generic_forward_route above, a wave per problem
  const char *GB = "generic_backward_kernel", *GF = "generic_forward_kernel";
  const int MC = ALTRO_HIP_SWEEP_MATRIX_CORES;
  route("(24, 8) 1536", gen(24, 8, 1536, false, false), BWD, SK_GENERIC_BACKWARD, GB, 0, 1536, 64, 26816);
  route("(24, 8) 1537", gen(24, 8, 1537, false, false), BWD, SK_GENERIC_BACKWARD | SF_LATE_Q, GB, LQ, 1537, 64, 22208);
  route("(24, 8) 1537 matrix cores", gen(24, 8, 1537, false, false, true), BWD, SK_GENERIC_BACKWARD | SF_LATE_Q | SF_MATRIX_CORES, GB, LQ | MC, 1537, 64, 22208);
  route("(24, 8) 5 matrix cores", gen(24, 8, 5, false, false, true), BWD, SK_GENERIC_BACKWARD | SF_MATRIX_CORES, GB, MC, 5, 64, 26816);
  route("(24, 8) 5 matrix cores fp32", gen(24, 8, 5, false, false, true, false), BWD, SK_GENERIC_BACKWARD, GB, 0, 5, 64, 13440);   // (fp64 only)
  route("(50, 4) 3", gen(50, 4, 3, false, false), BWD, SK_GENERIC_BACKWARD | SF_GLOBAL_WS, GB, WS, 3, 64, 88816);
  route("(50, 4) 3 matrix cores", gen(50, 4, 3, false, false, true), BWD, SK_GENERIC_BACKWARD | SF_GLOBAL_WS | SF_MATRIX_CORES, GB, WS | MC, 3, 64, 88816);
  route("(20, 8) 5", gen(20, 8, 5, false, false), FWD, SK_GENERIC_FORWARD | SF_STAGED, GF, ST, 5, 64, 9952);
  route("(24, 8) 5", gen(24, 8, 5, false, false, true), FWD, SK_GENERIC_FORWARD, GF, 0, 5, 64, 512);
  route("(24, 8) 5 fp32", gen(24, 8, 5, false, false, false, false), FWD, SK_GENERIC_FORWARD | SF_STAGED, GF, ST, 5, 64, 6752);
  for (bool mc : {false, true}) {   // ... and equal to what the plan's own functions say
    const SweepRoute b = sweep_route(gen(24, 8, 1537, false, false, mc), BWD), f = sweep_route(gen(24, 8, 1537, false, false, mc), FWD);
    const GenericBackwardRoute gb = generic_backward_route(24, 8, 8, 1537, 0u);
    const GenericForwardRoute gf = generic_forward_route(24, 8, 1, 8, kGenericForwardStageLimit);
    if (b.variant != (gb.variant() | (mc ? MC : 0)) || b.lds != gb.bytes || ((b.id & SF_LATE_Q) != 0) != gb.late_q || ((b.id & SF_GLOBAL_WS) != 0) != gb.big ||
        f.variant != gf.variant() || f.lds != gf.bytes || ((f.id & SF_STAGED) != 0) != gf.staged) {
      ++failures;
      std::printf("plan GENERIC through sweep_route differs from generic_*_route (matrix cores %d)\n", (int)mc);
    }
  }

  // every id a row above was given has a name; what is no id has none
  for (int id : ids)
    if (!sweep_kernel_name(id)) { ++failures; std::printf("id %#x has no name\n", id); }
  if (ids.size() < 30 || sweep_kernel_name(0) || sweep_kernel_name(17 << 8)) { ++failures; std::printf("ids: %zu distinct\n", ids.size()); }
}

int main() {
  all_plans();
  // carve sizes
  if (generic_backward_lds_bytes(24, 8, 8) != 26816 || generic_backward_lds_bytes(24, 8, 8, true) != 22208 ||
      generic_backward_lds_bytes(12, 4, 4) != 3552 || generic_backward_lds_bytes(12, 4, 4, true) != 2976 || generic_backward_per_cu(26816) != 6 ||
      generic_backward_per_cu(22208) != 7 || generic_backward_per_cu(376) != 16 || generic_backward_per_cu(170944) != 0) {
    ++failures;
    std::printf("carve sizes\n");
  }
  // shape, element size, last batch without late Q, four-block carve, three-block carve
  threshold(2, 1, 8, NEVER, 376, 344);
  threshold(7, 3, 8, NEVER, 2800, 2408);
  threshold(9, 6, 8, NEVER, 5464, 4816);
  threshold(12, 4, 8, NEVER, 7040, 5888);
  threshold(13, 4, 8, NEVER, 8008, 6656);
  threshold(14, 5, 8, NEVER, 9656, 8088);
  threshold(12, 4, 4, NEVER, 3552, 2976);
  threshold(13, 4, 4, NEVER, 4036, 3360);
  threshold(14, 5, 4, NEVER, 4860, 4076);
  threshold(16, 8, 8, 2816, 14208, 12160);
  threshold(16, 8, 4, NEVER, 7136, 6112);
  threshold(17, 5, 8, 3072, 13232, 10920);
  threshold(17, 5, 4, NEVER, 6648, 5492);
  threshold(20, 8, 8, 2048, 20000, 16800);
  threshold(20, 8, 4, NEVER, 10032, 8432);
  threshold(24, 8, 8, 1536, 26816, 22208);
  threshold(24, 8, 4, 3072, 13440, 11136);
  threshold(31, 1, 8, 1024, 33088, 25400);
  threshold(31, 1, 4, 2304, 16576, 12732);
  threshold(33, 7, 8, 768, 44576, 35864);
  threshold(33, 7, 4, 1792, 22320, 17964);
  threshold(40, 10, 8, ALWAYS, 67504, 54704);
  threshold(40, 10, 4, 1024, 33784, 27384);
  threshold(40, 6, 8, 512, 61264, 48464);
  threshold(62, 4, 4, ALWAYS, 66952, 51576);
  threshold(32, 32, 4, 768, 42048, 37952);
  global_ws(62, 4, 8, 133840);
  global_ws(32, 32, 8, 84032);
  global_ws(50, 4, 8, 88816);
  global_ws(64, 16, 8, 170944);
  global_ws(64, 16, 4, 85504);
  // the drop-in's call (one problem, no forms): late Q only where the four-block carve does not fit
  backward(40, 10, 8, 1, 0u, LQ, 54704);
  backward(40, 6, 8, 1, 0u, 0, 61264);
  backward(20, 8, 8, 1, 0u, 0, 20000);
  backward(50, 4, 8, 1, 0u, WS, 88816);

  // forward sweep, 3 n + m + n^2 + 2 n m + n + m (+ n^2 + n with y) elements + 64 bytes staged, 2 n + m elements + 64 bytes unstaged.
  // A batch stages up to 10 KB a problem: (13, 4) 515 el -> 4184 B and (20, 8) 1236 el -> 9952 B staged; (24, 8) 1672 el -> 13440 B not
  forward(13, 4, 1, 8, kGenericForwardStageLimit, ST, 4184);
  forward(7, 3, 1, 8, kGenericForwardStageLimit, ST, 1512);
  forward(20, 8, 1, 8, kGenericForwardStageLimit, ST, 9952);
  forward(24, 8, 1, 8, kGenericForwardStageLimit, 0, 512);
  forward(24, 8, 1, 4, kGenericForwardStageLimit, ST, 6752);
  forward(64, 16, 1, 4, kGenericForwardStageLimit, 0, 640);
  forward(64, 16, 1, 8, kGenericForwardStageLimit, 0, 1216);
  // the drop-in stages whatever fits 64 KB: (24, 8) and (40, 6) with y (3892 el -> 31200 B) staged, (64, 16) 84800 B not; without y less
  forward(24, 8, 1, 8, kGenericLdsLimit, ST, 13440);
  forward(24, 8, 0, 8, kGenericLdsLimit, ST, 8640);
  forward(40, 6, 1, 8, kGenericLdsLimit, ST, 31200);
  forward(64, 16, 1, 8, kGenericLdsLimit, 0, 1216);
  forward(64, 16, 0, 8, kGenericLdsLimit, ST, 51520);

  if (failures) {
    std::printf("sweep_route_test: %d failures\n", failures);
    return 1;
  }
  std::printf("sweep_route_test ok\n");
  return 0;
}
