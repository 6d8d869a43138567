// al_shift.h on the CPU (plain g++, nothing of the library linked): the link table next[], the chain heads and the chains in walking order
// (what altro_hip_shift_duals' kernel reads) against tables written out by hand from the row packing of al_tables.h (blocks in
// knot-point order, within a knot point in registration order, p rows each), on plans LANE, MFMA16 and GENERIC; and, for every case,
// that each row is on exactly one chain and next > row.
#include <cstdio>
#include <vector>

#include "al_shift.h"
#include "al_tables.h"

using namespace altro_hip;
using namespace altro_hip::capi;

static int failures = 0;
static const char* where = "";
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, where); } \
  } while (0)

// the host description of a handle's blocks, as altro_hip_add_linear_constraint leaves it
struct Case {
  int plan, n, m, N, batch = 3;
  std::vector<int> nxv, nuv;
  std::vector<AlDef> defs;
  std::vector<AlKnotBig> knots;
  std::vector<double> G;
  std::vector<std::vector<double>> g;
  Case(int plan_, int N_) : plan(plan_), n(plan_ == ALTRO_HIP_PLAN_LANE ? 4 : plan_ == ALTRO_HIP_PLAN_MFMA16 ? 12 : 14),
                            m(plan_ == ALTRO_HIP_PLAN_LANE ? 2 : plan_ == ALTRO_HIP_PLAN_MFMA16 ? 4 : 9), N(N_), knots((size_t)N_ + 1, AlKnotBig{}) {}
  int add(int k0, int k1, int cone, int p) {
    const int w = n + m, id = (int)defs.size();
    defs.push_back(AlDef{cone, p, 0, (int)G.size(), 0, 0, w});
    for (int e = 0; e < w; ++e) for (int r = 0; r < p; ++r) G.push_back(0.3 * (r + 1) - 0.7 * (e + 1));
    g.push_back(std::vector<double>((size_t)p, 0.25));
    for (int k = k0; k <= k1; ++k) knots[k].def[knots[k].ncon++] = id;
    return id;
  }
  AlTables tables() const { return al_build(AlInput{plan, n, m, N, batch, 8, false, nxv, nuv, defs, knots, G, g}); }
};

static void check(const Case& c, const std::vector<int>& next, const std::vector<int>& heads) {
  const AlTables t = c.tables();
  CHECK(t.error == AL_BUILD_OK);
  const AlShift s = al_shift_build(t.big, c.defs, t.rows);
  CHECK(t.rows == (int)next.size());
  CHECK(s.next == next);
  CHECK(s.heads == heads);
  if (s.next != next) { std::printf("  next:"); for (int v : s.next) std::printf(" %d", v); std::printf("\n"); }
  if (s.heads != heads) { std::printf("  heads:"); for (int v : s.heads) std::printf(" %d", v); std::printf("\n"); }
  // the device's form: the chains one after the other in walking order, AL_SHIFT_PAD zeros behind them
  CHECK(s.start.size() == heads.size() + 1 && s.order.size() == next.size() + (size_t)AL_SHIFT_PAD);
  if (s.start.size() == heads.size() + 1 && s.order.size() == next.size() + (size_t)AL_SHIFT_PAD) {
    CHECK(s.start.back() == t.rows);
    for (size_t c = 0; c < heads.size(); ++c) {
      CHECK(s.start[c] < s.start[c + 1] && s.order[(size_t)s.start[c]] == heads[c]);
      for (int i = s.start[c]; i + 1 < s.start[c + 1]; ++i) CHECK(s.order[(size_t)i + 1] == next[(size_t)s.order[(size_t)i]]);
      CHECK(next[(size_t)s.order[(size_t)s.start[c + 1] - 1]] == -1);
    }
    for (size_t i = next.size(); i < s.order.size(); ++i) CHECK(s.order[i] == 0);
  }
  // every row on exactly one chain, links ascending
  std::vector<int> seen((size_t)t.rows, 0);
  for (int h : s.heads)
    for (int r = h; r >= 0; r = s.next[(size_t)r]) {
      CHECK(r < t.rows);
      if (r >= t.rows) break;
      ++seen[(size_t)r];
      CHECK(s.next[(size_t)r] < 0 || s.next[(size_t)r] > r);
      if (s.next[(size_t)r] >= 0 && s.next[(size_t)r] <= r) break;
    }
  for (int r = 0; r < t.rows; ++r) CHECK(seen[(size_t)r] == 1);
}

int main() {
  const int plans[] = {ALTRO_HIP_PLAN_LANE, ALTRO_HIP_PLAN_MFMA16, ALTRO_HIP_PLAN_GENERIC};
  const char* names[] = {"LANE", "MFMA16", "GENERIC"};
  for (int pi = 0; pi < 3; ++pi) {
    const int plan = plans[pi];
    where = names[pi];
    {   // a running block on 0 .. N-1 (2 rows) and a terminal-only block (3 rows), N = 4:
        // rows k0: 0 1 | k1: 2 3 | k2: 4 5 | k3: 6 7 | k4: 8 9 10
      Case c(plan, 4);
      c.add(0, 3, CONE_INEQUALITY, 2);
      c.add(4, 4, CONE_EQUALITY, 3);
      check(c, {2, 3, 4, 5, 6, 7, -1, -1, -1, -1, -1}, {0, 1, 8, 9, 10});
      const AlTables t = c.tables();
      const AlShift s = al_shift_build(t.big, c.defs, t.rows);
      const std::vector<int> order = {0, 2, 4, 6, 1, 3, 5, 7, 8, 9, 10}, start = {0, 4, 8, 9, 10, 11};
      CHECK(std::vector<int>(s.order.begin(), s.order.begin() + 11) == order && s.start == start);
    }
    {   // a partial range 3 .. 7 (2 rows) and a range reaching the terminal knot point, N-2 .. N (1 row), N = 8; two blocks at k = 6, 7:
        // rows k3: 0 1 | k4: 2 3 | k5: 4 5 | k6: 6 7, 8 | k7: 9 10, 11 | k8: 12
      Case c(plan, 8);
      c.add(3, 7, CONE_INEQUALITY, 2);
      c.add(6, 8, CONE_EQUALITY, 1);
      check(c, {2, 3, 4, 5, 6, 7, 9, 10, 11, -1, -1, 12, -1}, {0, 1, 8});
    }
    {   // two overlapping blocks whose position within the knot point changes (definition 1 is the second block at k = 1, 2 and the
        // first at k = 3): the link follows the definition, N = 3:
        // rows k0: 0 | k1: 1, 2 3 | k2: 4, 5 6 | k3: 7 8
      Case c(plan, 3);
      c.add(0, 2, CONE_EQUALITY, 1);
      c.add(1, 3, CONE_INEQUALITY, 2);
      check(c, {1, 4, 5, 6, -1, 7, 8, -1, -1}, {0, 2, 3});
    }
    {   // a second-order-cone block of 3 rows on 0 .. N-1, N = 3: rows k0: 0 1 2 | k1: 3 4 5 | k2: 6 7 8
      Case c(plan, 3);
      c.add(0, 2, CONE_SOC, 3);
      check(c, {3, 4, 5, 6, 7, 8, -1, -1, -1}, {0, 1, 2});
    }
    {   // the same constraint registered knot point by knot point as separate definitions: nothing links
      Case c(plan, 2);
      for (int k = 0; k <= 2; ++k) c.add(k, k, CONE_INEQUALITY, 2);
      check(c, {-1, -1, -1, -1, -1, -1}, {0, 1, 2, 3, 4, 5});
    }
    {   // no blocks: empty tables
      Case c(plan, 3);
      check(c, {}, {});
    }
    if (plan == ALTRO_HIP_PLAN_LANE) continue;   // (8 rows per block there)
    {   // a 24-row block (plan MFMA16: three slots of eight) and an 8-row block on 0 .. 1, N = 2: one chain per ROW
        // rows k0: 0 .. 23, 24 .. 31 | k1: 32 .. 55, 56 .. 63 | k2: none
      Case c(plan, 2);
      c.add(0, 1, CONE_INEQUALITY, 24);
      c.add(0, 1, CONE_INEQUALITY, 8);
      std::vector<int> next(64, -1), heads;
      for (int r = 0; r < 32; ++r) { next[(size_t)r] = r + 32; heads.push_back(r); }
      check(c, next, heads);
      if (plan == ALTRO_HIP_PLAN_MFMA16) {   // the slots are consecutive rows of their block, so the row links cover them
        const AlTables t = c.tables();
        CHECK(t.knots[1].ncon == 4);
        const int want[4] = {32, 40, 48, 56};
        for (int s = 0; s < 4; ++s) CHECK(t.knots[1].z_off[s] == want[s]);
      }
    }
  }
  if (failures) { std::printf("al_shift_test: %d failure(s)\n", failures); return 1; }
  std::printf("al_shift_test ok\n");
  return 0;
}
