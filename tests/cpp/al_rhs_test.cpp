// Right-hand sides per knot point in the constraint tables (al_tables.h: al_build with AlDef::g_per_knot; al_types.h: al_g_index) on the
// CPU, plain g++, nothing of the library linked: pool offsets and every knot point's g_off against numbers written out by hand on plans
// LANE, MFMA16 (a 24-row block over three slots) and GENERIC -- shared and per problem, a range that starts at k > 0, a range that reaches
// N, a terminal-only block --, AlSummary::uniform under its rule, and the index function against a brute-force walk of each segment.
#include <cstdio>
#include <set>
#include <vector>

#include "al_tables.h"

using namespace altro_hip;
using namespace altro_hip::capi;

static int failures = 0;
static const char* where = "";
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, where); } \
  } while (0)

constexpr int B = 3;
// the value the caller gives as element (problem b, knot point k, row r) of block d: distinct everywhere
static double value(int d, int b, int k, int r) { return 1000.0 * d + 100.0 * k + 10.0 * r + b + 0.5; }

struct Case {
  int plan, n, m, N;
  std::vector<int> nxv, nuv;
  std::vector<AlDef> defs;
  std::vector<AlKnotBig> knots;
  std::vector<double> G;
  std::vector<std::vector<double>> g;
  std::vector<int> k_first, k_last;   // the range every block was registered on
  Case(int plan_, int N_) : plan(plan_), n(plan_ == ALTRO_HIP_PLAN_LANE ? 4 : plan_ == ALTRO_HIP_PLAN_MFMA16 ? 12 : 14),
                            m(plan_ == ALTRO_HIP_PLAN_LANE ? 2 : plan_ == ALTRO_HIP_PLAN_MFMA16 ? 4 : 9), N(N_), knots((size_t)N_ + 1, AlKnotBig{}) {}
  // as altro_hip_add_linear_constraint_rhs leaves the host description: g is [nb][nk][p]
  int add(int k0, int k1, int cone, int p, bool per_problem, bool per_knot) {
    const int w = n + m, id = (int)defs.size();
    defs.push_back(AlDef{cone, p, per_problem ? 1 : 0, (int)G.size(), 0, 0, w, per_knot ? 1 : 0, per_knot ? k0 : 0});
    for (int e = 0; e < w; ++e) for (int r = 0; r < p; ++r) G.push_back(0.3 * (r + 1) - 0.7 * (e + 1));
    std::vector<double> v;
    for (int b = 0; b < (per_problem ? B : 1); ++b)
      for (int k = k0; k <= (per_knot ? k1 : k0); ++k)
        for (int r = 0; r < p; ++r) v.push_back(value(id, b, k, r));
    g.push_back(v);
    k_first.push_back(k0); k_last.push_back(k1);
    for (int k = k0; k <= k1; ++k) knots[k].def[knots[k].ncon++] = id;
    return id;
  }
  AlTables tables() const { return al_build(AlInput{plan, n, m, N, B, 8, false, nxv, nuv, defs, knots, G, g}); }
};

// every block's segment: al_g_index against a walk of the segment in memory order ([K][p] or [K][p][batch]), the values found there,
// and that the segments tile the pool
static void brute_force(const Case& c, const AlTables& t) {
  std::set<int64_t> seen;
  int64_t at = 0;
  for (size_t i = 0; i < c.defs.size(); ++i) {
    const AlDef& d = t.defs[i];
    CHECK(d.g_off == at);
    const int k0 = c.k_first[i], K = d.g_per_knot ? c.k_last[i] - k0 + 1 : 1;
    CHECK(d.k_first == (d.g_per_knot ? k0 : 0));
    for (int kk = 0; kk < K; ++kk)
      for (int r = 0; r < d.p; ++r)
        for (int b = 0; b < (d.g_per_problem ? B : 1); ++b, ++at) {
          CHECK(al_g_index(d, B, b, k0 + kk, r) == at);
          CHECK(at < (int64_t)t.g.size() && t.g[(size_t)at] == value((int)i, b, k0 + kk, r));
          seen.insert(at);
          if (!d.g_per_knot)   // one run for every knot point of the range
            for (int k = k0; k <= c.k_last[i]; ++k) CHECK(al_g_index(d, B, b, k, r) == at);
        }
  }
  CHECK(at == (int64_t)t.g.size() && (int64_t)seen.size() == at);
}

int main() {
  {
    where = "lane: shared block 0..4, per-problem per-knot block 1..3";
    Case c(ALTRO_HIP_PLAN_LANE, 4);
    c.add(0, 4, CONE_INEQUALITY, 2, false, false);   // pool [0, 2)
    c.add(1, 3, CONE_INEQUALITY, 3, true, true);     // pool [2, 29): [3 knot points][3 rows][3 problems]
    const AlTables t = c.tables();
    CHECK(t.error == AL_BUILD_OK && t.g.size() == 29 && t.defs[0].g_off == 0 && t.defs[1].g_off == 2);
    CHECK(t.sum.uniform == 0);                       // (knot point 0 has one block, 1 has two: not uniform in any case)
    for (int k = 0; k <= 4; ++k) CHECK(t.knots[k].g_off[0] == 0 && t.big[k].g_off[0] == 0);
    const int64_t want[5] = {-1, 2, 11, 20, -1};
    for (int k = 1; k <= 3; ++k) CHECK(t.knots[k].ncon == 2 && t.knots[k].g_off[1] == want[k] && t.big[k].g_off[1] == want[k] && t.knots[k].g_per_problem[1] == 1);
    CHECK(t.knots[0].ncon == 1 && t.knots[4].ncon == 1);
    // element (b = 2, k = 2, r = 1): 2 + ((2 - 1) * 3 + 1) * 3 + 2
    CHECK(al_g_index(t.defs[1], B, 2, 2, 1) == 16 && t.g[16] == value(1, 2, 2, 1));
    brute_force(c, t);
  }
  {
    where = "lane: shared per-knot block 2..N";
    Case c(ALTRO_HIP_PLAN_LANE, 4);
    c.add(2, 4, CONE_EQUALITY, 2, false, true);      // pool [0, 6): [3 knot points][2 rows]
    const AlTables t = c.tables();
    CHECK(t.error == AL_BUILD_OK && t.g.size() == 6);
    for (int k = 2; k <= 4; ++k) CHECK(t.knots[k].g_off[0] == 2 * (k - 2) && t.knots[k].g_per_problem[0] == 0);
    CHECK(t.g[5] == value(0, 0, 4, 1));
    brute_force(c, t);
  }
  {
    where = "lane: uniform under its rule";
    Case a(ALTRO_HIP_PLAN_LANE, 4);                  // a running block with one g, a per-knot block at the terminal knot point alone
    a.add(0, 3, CONE_INEQUALITY, 2, false, false);
    a.add(4, 4, CONE_EQUALITY, 3, true, true);
    const AlTables ta = a.tables();
    CHECK(ta.sum.uniform == 1 && ta.sum.rows_per_knot == 2);
    CHECK(ta.knots[4].g_off[0] == 2 && ta.g.size() == 2 + 9);
    brute_force(a, ta);
    Case b(ALTRO_HIP_PLAN_LANE, 4);                  // the same running block with a g per knot point
    b.add(0, 3, CONE_INEQUALITY, 2, false, true);
    const AlTables tb = b.tables();
    CHECK(tb.sum.uniform == 0 && tb.sum.rows_per_knot == 2);
    for (int k = 0; k <= 3; ++k) CHECK(tb.knots[k].g_off[0] == 2 * k && tb.knots[k].z_off[0] == 2 * k);
    brute_force(b, tb);
    Case u(ALTRO_HIP_PLAN_LANE, 4);                  // ... and without: what it was
    u.add(0, 3, CONE_INEQUALITY, 2, false, false);
    CHECK(u.tables().sum.uniform == 1);
  }
  {
    where = "tile: 24-row per-problem per-knot block over three slots 0..2, shared 8-row block 0..3";
    Case c(ALTRO_HIP_PLAN_MFMA16, 3);
    c.add(0, 2, CONE_INEQUALITY, 24, true, true);    // pool [0, 216): [3 knot points][24 rows][3 problems]
    c.add(0, 3, CONE_INEQUALITY, 8, false, false);   // pool [216, 224)
    const AlTables t = c.tables();
    CHECK(t.error == AL_BUILD_OK && t.g.size() == 224 && t.sum.uniform == 0 && t.sum.max_ncon == 4);
    for (int k = 0; k <= 2; ++k) {
      CHECK(t.knots[k].ncon == 4 && t.big[k].ncon == 2 && t.big[k].g_off[0] == 72 * k && t.big[k].g_off[1] == 216);
      for (int sl = 0; sl < 3; ++sl)                 // slot sl: rows 8 sl .. 8 sl + 7 inside knot point k's run
        CHECK(t.knots[k].g_off[sl] == 72 * k + 24 * sl && t.knots[k].p[sl] == 8 && t.knots[k].def[sl] == 0 && t.knots[k].z_off[sl] == 32 * k + 8 * sl);
      CHECK(t.knots[k].g_off[3] == 216 && t.knots[k].def[3] == 1);
    }
    CHECK(t.knots[3].ncon == 1 && t.knots[3].g_off[0] == 216);
    CHECK(t.g[72 * 1 + 24 * 2 + 3 * 5 + 1] == value(0, 1, 1, 21));   // knot point 1, slot 2, row 5 of the slot = row 21, problem 1
    brute_force(c, t);
  }
  {
    where = "tile: 24-row shared per-knot block 1..N";
    Case c(ALTRO_HIP_PLAN_MFMA16, 3);
    c.add(1, 3, CONE_INEQUALITY, 24, false, true);   // pool [0, 72): [3 knot points][24 rows]
    const AlTables t = c.tables();
    CHECK(t.error == AL_BUILD_OK && t.g.size() == 72 && t.sum.uniform == 0);
    for (int k = 1; k <= 3; ++k)
      for (int sl = 0; sl < 3; ++sl) CHECK(t.knots[k].g_off[sl] == 24 * (k - 1) + 8 * sl);
    CHECK(t.knots[0].ncon == 0);
    brute_force(c, t);
  }
  {
    where = "generic: per-problem 0..N, shared 1..2, terminal-only";
    Case c(ALTRO_HIP_PLAN_GENERIC, 3);
    c.add(0, 3, CONE_INEQUALITY, 5, true, true);     // pool [0, 60): [4][5][3]
    c.add(1, 2, CONE_SOC, 2, false, true);           // pool [60, 64): [2][2]
    c.add(3, 3, CONE_EQUALITY, 1, false, true);      // pool [64, 65)
    const AlTables t = c.tables();
    CHECK(t.error == AL_BUILD_OK && t.g.size() == 65 && t.knots.empty() && t.sum.uniform == 0);
    for (int k = 0; k <= 3; ++k) CHECK(t.big[k].g_off[0] == 15 * k && t.big[k].g_per_problem[0] == 1);
    CHECK(t.big[1].ncon == 2 && t.big[1].g_off[1] == 60 && t.big[2].g_off[1] == 62 && t.big[3].ncon == 2 && t.big[3].g_off[1] == 64 && t.big[0].ncon == 1);
    brute_force(c, t);
  }
  {
    where = "generic: a terminal-only per-knot block leaves uniform as it is";
    Case c(ALTRO_HIP_PLAN_GENERIC, 3);
    c.add(0, 2, CONE_INEQUALITY, 4, true, false);
    c.add(3, 3, CONE_EQUALITY, 2, true, true);
    const AlTables t = c.tables();
    CHECK(t.sum.uniform == 1 && t.big[3].g_off[0] == 12 && t.g.size() == 12 + 6);
    brute_force(c, t);
  }
  if (failures) { std::printf("al_rhs_test: %d failure(s)\n", failures); return 1; }
  std::printf("al_rhs_test ok\n");
  return 0;
}
