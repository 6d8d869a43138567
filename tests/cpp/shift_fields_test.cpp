// shift_fields.h against offsets written out by hand from the record pictures (kernels/mfma16_layout.h, lane_sizes):
// where the dynamics given as data and the cost's linear terms live on plans LANE, MFMA16 and GENERIC, how the shift kernel walks them
// (ShiftRun), and the assertion that makes the in-place walk safe.  Plain g++, nothing of the library linked.  N = 3, batch = 5.
#include <cstdio>
#include <set>
#include <vector>

#include "shift_fields.h"

using namespace altro_hip;
using namespace altro_hip::capi;

static int failures = 0;
static const char* where = "";
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, where); } \
  } while (0)

struct Want { int buf, kind; long long off, bs, ks; int E, len; };
static void same(const FieldRef& r, const Want& w) {
  const bool ok = r.buf == w.buf && r.kind == w.kind && r.off == w.off && r.bs == w.bs && r.ks == w.ks && r.E == w.E && r.len == w.len;
  if (!ok) {
    ++failures;
    std::printf("%s: got buf %d kind %d off %lld bs %lld ks %lld E %d len %d, want buf %d kind %d off %lld bs %lld ks %lld E %d len %d\n", where, r.buf, r.kind,
                (long long)r.off, (long long)r.bs, (long long)r.ks, r.E, r.len, w.buf, w.kind, w.off, w.bs, w.ks, w.E, w.len);
  }
}
struct WantRun { long long first, rows, run, rs, ks; int K, vec; };
static void same_run(const ShiftRun& r, const WantRun& w) {
  const bool ok = r.ok && r.first == w.first && r.rows == w.rows && r.run == w.run && r.rs == w.rs && r.ks == w.ks && r.K == w.K && r.vec == w.vec;
  if (!ok) {
    ++failures;
    std::printf("%s: run ok %d first %lld rows %lld run %lld rs %lld ks %lld K %d vec %d, want first %lld rows %lld run %lld rs %lld ks %lld K %d vec %d\n", where,
                (int)r.ok, (long long)r.first, (long long)r.rows, (long long)r.run, (long long)r.rs, (long long)r.ks, r.K, r.vec, w.first, w.rows, w.run, w.rs, w.ks,
                w.K, w.vec);
  }
}
// the walk by brute force: every (row, k, element) has an address of its own inside a buffer of `size` elements, and the addresses are
// exactly those of the field as loop_fields.h addresses it (problem b, knot point k, element e)
static void walk(const FieldRef& f, const ShiftRun& r, long long batch, long long size) {
  std::set<long long> seen, direct;
  for (long long row = 0; row < r.rows; ++row)
    for (int k = 0; k < r.K; ++k)
      for (long long e = 0; e < r.run; ++e) {
        const long long at = r.first + row * r.rs + k * r.ks + e;
        CHECK(at >= 0 && at < size);
        CHECK(seen.insert(at).second);
      }
  for (long long b = 0; b < batch; ++b)
    for (int k = 0; k < r.K; ++k)
      for (int e = 0; e < f.len; ++e)
        direct.insert(f.kind == LK_LANE ? ((long long)k * f.E + f.off + e) * batch + b : f.off + b * f.bs + k * f.ks + e);
  CHECK(seen == direct);
  CHECK(r.vec == 1 || (r.first % r.vec == 0 && r.run % r.vec == 0 && r.rs % r.vec == 0 && r.ks % r.vec == 0));
}

int main() {
  const int N = 3;
  const long long B = 5;
  const int A = LK_AOS, L = LK_LANE;
  FieldRef f[3];

  {   // plan LANE (4, 2): the l_in record is A 16 | B 8 | f 4 | Q 16 | R 4 | H 8 | q 4 | r 2 = 62 elements, rows of 5 problems
    where = "LANE (4, 2) dynamics";
    DynShape d{ALTRO_HIP_PLAN_LANE, 4, 2, N, B, 0, 0};
    CHECK(dyn_fields(d, 0, f) == 1);
    same(f[0], {LB_L_IN, L, 0, 1, 310, 62, 28});
    CHECK(dyn_fields(d, 2, f) == 1);
    same(f[0], {LB_L_IN, L, 0, 1, 310, 62, 28});   // (LK_LANE: k is not part of the reference)
    CHECK(dyn_fields(d, -1, f) == 0 && dyn_fields(d, N, f) == 0);
    dyn_fields(d, 0, f);
    same_run(shift_run(f[0], B, N, 8), {0, 1, 140, 0, 310, 3, 2});
    same_run(shift_run(f[0], B, N, 4), {0, 1, 140, 0, 310, 3, 1});      // 310 floats are no multiple of 16 bytes
    walk(f[0], shift_run(f[0], B, N, 8), B, 62 * B * N);
    DynShape d66{ALTRO_HIP_PLAN_LANE, 4, 2, N, 66, 0, 0}, d3{ALTRO_HIP_PLAN_LANE, 4, 2, N, 3, 0, 0};   // (a LANE reference holds the batch in ks)
    dyn_fields(d66, 0, f);
    same_run(shift_run(f[0], 66, N, 8), {0, 1, 28 * 66, 0, 62 * 66, 3, 2});
    same_run(shift_run(f[0], 66, N, 4), {0, 1, 28 * 66, 0, 62 * 66, 3, 4});
    dyn_fields(d3, 0, f);
    same_run(shift_run(f[0], 3, N, 8), {0, 1, 84, 0, 186, 3, 2});
    same_run(shift_run(f[0], 3, N, 4), {0, 1, 84, 0, 186, 3, 1});
    dyn_fields(d, 0, f);

    where = "LANE (4, 2) diagonal cost";   // Qd 4 | Rd 2 | q 4 | r 2 | c = 13: q | r | c are neighbours
    LoopShape s{ALTRO_HIP_PLAN_LANE, false, false, 4, 2, N, B, 0, 0, nullptr, nullptr};
    CHECK(linear_cost_fields(s, f) == 1);
    same(f[0], {LB_L_COST, L, 6, 1, 65, 13, 7});
    same_run(shift_run(f[0], B, N, 8), {30, 1, 35, 0, 65, 3, 1});
    walk(f[0], shift_run(f[0], B, N, 8), B, 13 * B * (N + 1));
    where = "LANE (4, 2) dense cost";      // Q 16 | R 4 | H 8 | q 4 | r 2 | c = 35
    s.cost_dense = true;
    CHECK(linear_cost_fields(s, f) == 1);
    same(f[0], {LB_L_COSTQ, L, 28, 1, 175, 35, 7});
    same_run(shift_run(f[0], B, N, 4), {140, 1, 35, 0, 175, 3, 1});
    walk(f[0], shift_run(f[0], B, N, 4), B, 35 * B * (N + 1));
  }
  // plan MFMA16: DYN records of 204 (Z 192 | f 12) in a [k][b][record] slab -- in_bs 204, in_ks 5 * 204 = 1020 -- whatever the shape;
  // COSTP 36 (Qd 0 | Rd 12 | q 16 | r 28 | c 32); dense: COST-layout records of 160 ([q r] at 144, c in the pad slot 78)
  for (int shape = 0; shape < 2; ++shape) {
    const int n = shape ? 7 : 12, m = shape ? 3 : 4;
    where = shape ? "MFMA16 (7, 3)" : "MFMA16 (12, 4)";
    DynShape d{ALTRO_HIP_PLAN_MFMA16, n, m, N, B, 204, 1020};
    CHECK(dyn_fields(d, 0, f) == 1);
    same(f[0], {LB_M_IN, A, 0, 204, 1020, 0, 204});
    same_run(shift_run(f[0], B, N, 8), {0, 1, 1020, 0, 1020, 3, 2});   // the slab's records back to back: one row
    same_run(shift_run(f[0], B, N, 4), {0, 1, 1020, 0, 1020, 3, 4});
    walk(f[0], shift_run(f[0], B, N, 8), B, 204 * B * N);
    CHECK(dyn_fields(d, 2, f) == 1);
    same(f[0], {LB_M_IN, A, 2040, 204, 1020, 0, 204});
    CHECK(dyn_fields(d, N, f) == 0);

    LoopShape s{ALTRO_HIP_PLAN_MFMA16, false, false, n, m, N, B, 28, 140, nullptr, nullptr};
    if (!shape) {   // (12, 4): q 12 | r 4 | c 1 are neighbours
      CHECK(linear_cost_fields(s, f) == 1);
      same(f[0], {LB_M_COSTP, A, 16, 36, 180, 0, 17});
      same_run(shift_run(f[0], B, N, 8), {16, 5, 17, 36, 180, 3, 1});
      walk(f[0], shift_run(f[0], B, N, 8), B, 36 * B * (N + 1));
    } else {        // (7, 3): the padding between them is not the cost's
      CHECK(linear_cost_fields(s, f) == 3);
      same(f[0], {LB_M_COSTP, A, 16, 36, 180, 0, 7});
      same(f[1], {LB_M_COSTP, A, 28, 36, 180, 0, 3});
      same(f[2], {LB_M_COSTP, A, 32, 36, 180, 0, 1});
      same_run(shift_run(f[1], B, N, 4), {28, 5, 3, 36, 180, 3, 1});
      for (int i = 0; i < 3; ++i) walk(f[i], shift_run(f[i], B, N, 8), B, 36 * B * (N + 1));
    }
    s.cost_dense = true;   // the [q r] slot of the dense cost's OWN records (m_costd), never the handle's COST records
    if (!shape) {
      CHECK(linear_cost_fields(s, f) == 2);
      same(f[0], {LB_M_COSTD, A, 144, 160, 800, 0, 16});
      same(f[1], {LB_M_COSTD, A, 78, 160, 800, 0, 1});
      same_run(shift_run(f[0], B, N, 8), {144, 5, 16, 160, 800, 3, 2});
      same_run(shift_run(f[0], B, N, 4), {144, 5, 16, 160, 800, 3, 4});
      same_run(shift_run(f[1], B, N, 8), {78, 5, 1, 160, 800, 3, 1});
      for (int i = 0; i < 2; ++i) walk(f[i], shift_run(f[i], B, N, 8), B, 160 * B * N);
    } else {
      CHECK(linear_cost_fields(s, f) == 3);
      same(f[0], {LB_M_COSTD, A, 144, 160, 800, 0, 7});
      same(f[1], {LB_M_COSTD, A, 156, 160, 800, 0, 3});
      same(f[2], {LB_M_COSTD, A, 78, 160, 800, 0, 1});
      for (int i = 0; i < 3; ++i) walk(f[i], shift_run(f[i], B, N, 4), B, 160 * B * N);
    }
  }
  {   // plan GENERIC (13, 4): G_A [b][3][169], G_B [b][3][52], G_f [b][3][13]; the cost's q [b][4][13], r [b][3][4], c [b][4]
    where = "GENERIC (13, 4)";
    DynShape d{ALTRO_HIP_PLAN_GENERIC, 13, 4, N, B, 0, 0};
    CHECK(dyn_fields(d, 0, f) == 3);
    same(f[0], {LB_G_A, A, 0, 507, 169, 0, 169});
    same(f[1], {LB_G_B, A, 0, 156, 52, 0, 52});
    same(f[2], {LB_G_F, A, 0, 39, 13, 0, 13});
    same_run(shift_run(f[0], B, N, 8), {0, 5, 169, 507, 169, 3, 1});
    same_run(shift_run(f[1], B, N, 8), {0, 5, 52, 156, 52, 3, 2});
    same_run(shift_run(f[1], B, N, 4), {0, 5, 52, 156, 52, 3, 4});
    same_run(shift_run(f[2], B, N, 4), {0, 5, 13, 39, 13, 3, 1});
    const long long size[3] = {507 * B, 156 * B, 39 * B};
    for (int i = 0; i < 3; ++i) walk(f[i], shift_run(f[i], B, N, 8), B, size[i]);
    CHECK(dyn_fields(d, 1, f) == 3);
    same(f[0], {LB_G_A, A, 169, 507, 169, 0, 169});
    same(f[1], {LB_G_B, A, 52, 156, 52, 0, 52});
    same(f[2], {LB_G_F, A, 13, 39, 13, 0, 13});

    LoopShape s{ALTRO_HIP_PLAN_GENERIC, false, true, 13, 4, N, B, 0, 0, nullptr, nullptr};
    CHECK(linear_cost_fields(s, f) == 3);
    same(f[0], {LB_G_Cq, A, 0, 52, 13, 0, 13});
    same(f[1], {LB_G_Cr, A, 0, 12, 4, 0, 4});
    same(f[2], {LB_G_Cc, A, 0, 4, 1, 0, 1});
    same_run(shift_run(f[2], B, N, 8), {0, 5, 1, 4, 1, 3, 1});
    const long long csize[3] = {52 * B, 12 * B, 4 * B};
    for (int i = 0; i < 3; ++i) walk(f[i], shift_run(f[i], B, N, 8), B, csize[i]);
    // a horizon of one knot point: the array is one block per problem, nothing moves and nothing is merged into a row that would not fit
    DynShape d1{ALTRO_HIP_PLAN_GENERIC, 13, 4, 1, B, 0, 0};
    CHECK(dyn_fields(d1, 0, f) == 3);
    same_run(shift_run(f[0], B, 1, 8), {0, 5, 169, 169, 169, 1, 1});
  }
  {   // the assertion: a knot point's run longer than the knot-point stride, or rows that reach into each other, cannot be walked in place
    where = "safety";
    CHECK(!shift_run(FieldRef{LB_G_A, A, 0, 100, 8, 0, 10}, B, N, 8).ok);          // run 10 > ks 8
    CHECK(shift_run(FieldRef{LB_G_A, A, 0, 100, 10, 0, 10}, B, N, 8).ok);
    CHECK(!shift_run(FieldRef{LB_G_A, A, 0, 29, 10, 0, 10}, B, N, 8).ok);          // a problem's walk of 30 elements in a share of 29
    CHECK(shift_run(FieldRef{LB_G_A, A, 0, 30, 10, 0, 10}, B, N, 8).ok);
    CHECK(!shift_run(FieldRef{LB_M_COSTP, A, 0, 36, 160, 0, 17}, B, N, 8).ok);     // a slab of 4 * 36 + 17 = 161 elements in a knot-point stride of 160
    CHECK(shift_run(FieldRef{LB_M_COSTP, A, 0, 36, 161, 0, 17}, B, N, 8).ok);
    CHECK(!shift_run(FieldRef{LB_L_IN, L, 0, 1, 4 * B, 4, 5}, B, N, 8).ok);        // a LANE field longer than its record
    ShiftRun r{0, 2, 8, 4, 100, 3, 1, false};
    CHECK(!shift_run_safe(r));                                                       // rows closer than a run
    CHECK(shift_run(FieldRef{LB_G_A, A, 0, 10, 1, 0, 10}, B, 1, 8).ok);            // one knot point: nothing is read or written
  }
  if (failures) { std::printf("shift_fields_test: %d failures\n", failures); return 1; }
  std::printf("shift_fields_test ok\n");
  return 0;
}
