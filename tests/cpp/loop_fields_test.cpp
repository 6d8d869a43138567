// loop_fields.h against offsets written out by hand from the record pictures (kernels/mfma16_layout.h, kernels/ilqr_lane.hip,
// lane_sizes): plain g++, nothing of the library linked.  N = 3 and batch = 5 everywhere; every shape at k = 0,
// an interior k and k = N.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "loop_fields.h"

using namespace altro_hip;
using namespace altro_hip::capi;

static int failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, where); } \
  } while (0)

struct Want { int field, k, buf, kind; long long off, bs, ks; int E, len; };
static const char* where = "";

static void expect(const LoopShape& s, const char* name, const std::vector<Want>& wants) {
  where = name;
  for (const Want& w : wants) {
    const FieldRef r = loop_field(s, w.field, w.k);
    const bool same = r.buf == w.buf && (w.buf == LB_NONE || (r.kind == w.kind && r.off == w.off && r.bs == w.bs && r.ks == w.ks && r.E == w.E && r.len == w.len));
    if (!same) {
      ++failures;
      std::printf("%s: field %d k %d: got buf %d kind %d off %lld bs %lld ks %lld E %d len %d, want buf %d kind %d off %lld bs %lld ks %lld E %d len %d\n",
                  name, w.field, w.k, r.buf, r.kind, (long long)r.off, (long long)r.bs, (long long)r.ks, r.E, r.len, w.buf, w.kind, w.off, w.bs, w.ks, w.E, w.len);
    }
  }
}

// the length of the record a buffer is made of (0: one array per field -- plan GENERIC -- where a field must end inside one problem's share)
static int record_length(const LoopShape& s, const FieldRef& r) {
  switch (r.buf) {
    case LB_M_XUY: return 28;
    case LB_M_NOM: return MF_NOM;
    case LB_M_COSTP: return MF_COSTP;
    case LB_M_COSTD: return MF_COST;
    case LB_M_COSTD_TERM: return MF_TERM;
    case LB_L_XUY: case LB_L_NOM: case LB_L_COST: case LB_L_COSTQ: return r.E;
    default: (void)s; return 0;
  }
}

// every shape: the fields of one record do not overlap and end inside it; u, r, R, H (and Rd) have no terminal knot point; nothing at
// k = -1 and k = N + 1
static void structure(const LoopShape& s, const char* name) {
  where = name;
  const int N = s.N;
  for (int f : {LF_CAND_U, LF_NOM_U, LF_COST_r, LF_COST_R, LF_COST_H, LF_COST_Rd}) CHECK(loop_field(s, f, N).buf == LB_NONE);
  for (int f = 0; f < LF_NUM; ++f) { CHECK(loop_field(s, f, -1).buf == LB_NONE); CHECK(loop_field(s, f, N + 1).buf == LB_NONE); }
  for (int k = 0; k <= N; ++k) {
    struct Span { int buf; long long lo, hi; };
    std::vector<Span> spans;
    for (int f = 0; f < LF_NUM; ++f) {
      const FieldRef r = loop_field(s, f, k);
      if (r.buf == LB_NONE) continue;
      CHECK(r.len > 0);
      const int rec = record_length(s, r);
      long long lo;   // the field's place inside its record
      if (r.kind == LK_LANE) { lo = r.off; CHECK(r.E == rec && r.ks == (long long)rec * s.batch && r.bs == 1); }
      else if (rec > 0) { lo = r.off - (r.ks ? (long long)k * r.ks : 0); CHECK(r.bs == rec || r.buf == LB_M_XUY); }
      else { lo = r.off; CHECK(r.off + r.len <= r.bs); }
      if (rec > 0) { CHECK(lo >= 0 && lo + r.len <= rec); }
      spans.push_back(Span{r.buf, lo, lo + r.len});
    }
    for (size_t i = 0; i < spans.size(); ++i)
      for (size_t j = i + 1; j < spans.size(); ++j)
        if (spans[i].buf == spans[j].buf) CHECK(spans[i].hi <= spans[j].lo || spans[j].hi <= spans[i].lo);
  }
}

int main() {
  const int N = 3;
  const long long B = 5;
  const int A = LK_AOS, L = LK_LANE, none = LB_NONE;

  {   // plan LANE (4, 2), diagonal cost: cand x 4 | y 4 | u 2 (E 10), nom x 4 | u 2 (E 6), cost Qd 4 | Rd 2 | q 4 | r 2 | c (E 13)
    LoopShape s{ALTRO_HIP_PLAN_LANE, false, false, 4, 2, N, B, 0, 0, nullptr, nullptr};
    std::vector<Want> w;
    for (int k : {0, 1, 3}) {
      w.push_back({LF_CAND_X, k, LB_L_XUY, L, 0, 1, 50, 10, 4});
      w.push_back({LF_NOM_X, k, LB_L_NOM, L, 0, 1, 30, 6, 4});
      w.push_back({LF_COST_Qd, k, LB_L_COST, L, 0, 1, 65, 13, 4});
      w.push_back({LF_COST_q, k, LB_L_COST, L, 6, 1, 65, 13, 4});
      w.push_back({LF_COST_c, k, LB_L_COST, L, 12, 1, 65, 13, 1});
      w.push_back({LF_COST_Q, k, none, 0, 0, 0, 0, 0, 0});
      w.push_back({LF_COST_R, k, none, 0, 0, 0, 0, 0, 0});
      w.push_back({LF_COST_H, k, none, 0, 0, 0, 0, 0, 0});
      if (k == N) continue;
      w.push_back({LF_CAND_U, k, LB_L_XUY, L, 8, 1, 50, 10, 2});
      w.push_back({LF_NOM_U, k, LB_L_NOM, L, 4, 1, 30, 6, 2});
      w.push_back({LF_COST_Rd, k, LB_L_COST, L, 4, 1, 65, 13, 2});
      w.push_back({LF_COST_r, k, LB_L_COST, L, 10, 1, 65, 13, 2});
    }
    expect(s, "LANE (4, 2) diagonal", w);
    structure(s, "LANE (4, 2) diagonal");
    CHECK(loop_field_run(s, LF_COST_q, 1, 3) == 3);
  }
  {   // plan LANE (4, 2), dense cost: Q 16 | R 4 | H 8 | q 4 | r 2 | c (E 35)
    LoopShape s{ALTRO_HIP_PLAN_LANE, false, true, 4, 2, N, B, 0, 0, nullptr, nullptr};
    std::vector<Want> w;
    for (int k : {0, 2, 3}) {
      w.push_back({LF_CAND_X, k, LB_L_XUY, L, 0, 1, 50, 10, 4});
      w.push_back({LF_NOM_X, k, LB_L_NOM, L, 0, 1, 30, 6, 4});
      w.push_back({LF_COST_Q, k, LB_L_COSTQ, L, 0, 1, 175, 35, 16});
      w.push_back({LF_COST_q, k, LB_L_COSTQ, L, 28, 1, 175, 35, 4});
      w.push_back({LF_COST_c, k, LB_L_COSTQ, L, 34, 1, 175, 35, 1});
      w.push_back({LF_COST_Qd, k, none, 0, 0, 0, 0, 0, 0});
      w.push_back({LF_COST_Rd, k, none, 0, 0, 0, 0, 0, 0});
      if (k == N) continue;
      w.push_back({LF_CAND_U, k, LB_L_XUY, L, 8, 1, 50, 10, 2});
      w.push_back({LF_NOM_U, k, LB_L_NOM, L, 4, 1, 30, 6, 2});
      w.push_back({LF_COST_R, k, LB_L_COSTQ, L, 16, 1, 175, 35, 4});
      w.push_back({LF_COST_H, k, LB_L_COSTQ, L, 20, 1, 175, 35, 8});
      w.push_back({LF_COST_r, k, LB_L_COSTQ, L, 32, 1, 175, 35, 2});
    }
    expect(s, "LANE (4, 2) dense", w);
    structure(s, "LANE (4, 2) dense");
  }
  // plan MFMA16, [k][b][record] slabs of 5 problems: XUY 28 (x 0 | y 12 | u 24), NOM 16 (x 0 | u 12), COSTP 36 (Qd 0 | Rd 12 | q 16 | r 28 |
  // c 32); dense cost: COST-layout records of 160 ([q r] at 144, c in the pad slot 78) and q_N at 144 of the TERM record (156, one per problem)
  for (int shape = 0; shape < 2; ++shape) {
    const int n = shape ? 7 : 12, m = shape ? 3 : 4;
    const char* names[2][2] = {{"MFMA16 (12, 4) diagonal", "MFMA16 (12, 4) dense"}, {"MFMA16 (7, 3) diagonal", "MFMA16 (7, 3) dense"}};
    LoopShape s{ALTRO_HIP_PLAN_MFMA16, false, false, n, m, N, B, 28, 140, nullptr, nullptr};
    std::vector<Want> w;
    const long long xuy[4] = {0, 140, 280, 420}, nom[4] = {0, 80, 160, 240}, cp[4] = {0, 180, 360, 540};
    for (int k : {0, 1, 3}) {
      w.push_back({LF_CAND_X, k, LB_M_XUY, A, xuy[k], 28, 140, 0, n});
      w.push_back({LF_NOM_X, k, LB_M_NOM, A, nom[k], 16, 80, 0, n});
      w.push_back({LF_COST_Qd, k, LB_M_COSTP, A, cp[k], 36, 180, 0, n});
      w.push_back({LF_COST_q, k, LB_M_COSTP, A, cp[k] + 16, 36, 180, 0, n});
      w.push_back({LF_COST_c, k, LB_M_COSTP, A, cp[k] + 32, 36, 180, 0, 1});
      for (int f : {LF_COST_Q, LF_COST_R, LF_COST_H}) w.push_back({f, k, none, 0, 0, 0, 0, 0, 0});
      if (k == N) continue;
      w.push_back({LF_CAND_U, k, LB_M_XUY, A, xuy[k] + 24, 28, 140, 0, m});
      w.push_back({LF_NOM_U, k, LB_M_NOM, A, nom[k] + 12, 16, 80, 0, m});
      w.push_back({LF_COST_Rd, k, LB_M_COSTP, A, cp[k] + 12, 36, 180, 0, m});
      w.push_back({LF_COST_r, k, LB_M_COSTP, A, cp[k] + 28, 36, 180, 0, m});
    }
    expect(s, names[shape][0], w);
    structure(s, names[shape][0]);
    CHECK(loop_field_run(s, LF_COST_q, 0, 3) == 4);

    s.cost_dense = true;
    w.clear();
    const long long cd[4] = {0, 800, 1600, 2400};
    for (int k : {0, 2, 3}) {
      w.push_back({LF_CAND_X, k, LB_M_XUY, A, xuy[k], 28, 140, 0, n});
      w.push_back({LF_NOM_X, k, LB_M_NOM, A, nom[k], 16, 80, 0, n});
      w.push_back({LF_COST_c, k, LB_M_COSTD, A, cd[k] + 78, 160, 800, 0, 1});
      for (int f : {LF_COST_Qd, LF_COST_Rd, LF_COST_Q, LF_COST_R, LF_COST_H}) w.push_back({f, k, none, 0, 0, 0, 0, 0, 0});   // (Q, R, H: pack.hip's segments)
      if (k == N) { w.push_back({LF_COST_q, k, LB_M_COSTD_TERM, A, 144, 156, 0, 0, n}); continue; }
      w.push_back({LF_COST_q, k, LB_M_COSTD, A, cd[k] + 144, 160, 800, 0, n});
      w.push_back({LF_COST_r, k, LB_M_COSTD, A, cd[k] + 156, 160, 800, 0, m});
      w.push_back({LF_CAND_U, k, LB_M_XUY, A, xuy[k] + 24, 28, 140, 0, m});
      w.push_back({LF_NOM_U, k, LB_M_NOM, A, nom[k] + 12, 16, 80, 0, m});
    }
    expect(s, names[shape][1], w);
    structure(s, names[shape][1]);
    CHECK(loop_field_run(s, LF_COST_q, 1, 3) == 2);   // q_N lives in the TERM record
    CHECK(loop_field_run(s, LF_COST_q, 3, 3) == 1);
    CHECK(loop_field_run(s, LF_COST_c, 0, 3) == 4);
  }
  {   // plan GENERIC (13, 4): one [b][k][block] array per field
    LoopShape s{ALTRO_HIP_PLAN_GENERIC, false, true, 13, 4, N, B, 0, 0, nullptr, nullptr};
    std::vector<Want> w;
    for (int k : {0, 2, 3}) {
      w.push_back({LF_CAND_X, k, LB_G_X, A, 13 * k, 52, 13, 0, 13});
      w.push_back({LF_NOM_X, k, LB_G_XN, A, 13 * k, 52, 13, 0, 13});
      w.push_back({LF_COST_q, k, LB_G_Cq, A, 13 * k, 52, 13, 0, 13});
      w.push_back({LF_COST_c, k, LB_G_Cc, A, k, 4, 1, 0, 1});
      w.push_back({LF_COST_Q, k, LB_G_CQ, A, 169 * k, 676, 169, 0, 169});
      w.push_back({LF_COST_Qd, k, none, 0, 0, 0, 0, 0, 0});
      w.push_back({LF_COST_Rd, k, none, 0, 0, 0, 0, 0, 0});
      if (k == N) continue;
      w.push_back({LF_CAND_U, k, LB_G_U, A, 4 * k, 12, 4, 0, 4});
      w.push_back({LF_NOM_U, k, LB_G_UN, A, 4 * k, 12, 4, 0, 4});
      w.push_back({LF_COST_r, k, LB_G_Cr, A, 4 * k, 12, 4, 0, 4});
      w.push_back({LF_COST_R, k, LB_G_CR, A, 16 * k, 48, 16, 0, 16});
      w.push_back({LF_COST_H, k, LB_G_CH, A, 52 * k, 156, 52, 0, 52});
    }
    expect(s, "GENERIC (13, 4)", w);
    structure(s, "GENERIC (13, 4)");
    s.cost_dense = false;   // (the plan has the dense form only: the flag changes nothing)
    expect(s, "GENERIC (13, 4), flag off", w);
  }
  {   // per-knot-point dimensions nx = 3 5 2 4, nu = 2 1 3: the blocks of a problem back to back
    const int nx[4] = {3, 5, 2, 4}, nu[3] = {2, 1, 3};
    LoopShape s{ALTRO_HIP_PLAN_GENERIC, true, true, 5, 3, N, B, 0, 0, nx, nu};
    const std::vector<Want> w = {
        {LF_CAND_X, 0, LB_G_X, A, 0, 14, 3, 0, 3}, {LF_CAND_X, 1, LB_G_X, A, 3, 14, 5, 0, 5}, {LF_CAND_X, 3, LB_G_X, A, 10, 14, 4, 0, 4},
        {LF_NOM_X, 0, LB_G_XN, A, 0, 14, 3, 0, 3}, {LF_NOM_X, 2, LB_G_XN, A, 8, 14, 2, 0, 2}, {LF_NOM_X, 3, LB_G_XN, A, 10, 14, 4, 0, 4},
        {LF_COST_q, 0, LB_G_Cq, A, 0, 14, 3, 0, 3}, {LF_COST_q, 2, LB_G_Cq, A, 8, 14, 2, 0, 2}, {LF_COST_q, 3, LB_G_Cq, A, 10, 14, 4, 0, 4},
        {LF_CAND_U, 0, LB_G_U, A, 0, 6, 2, 0, 2}, {LF_CAND_U, 1, LB_G_U, A, 2, 6, 1, 0, 1}, {LF_CAND_U, 2, LB_G_U, A, 3, 6, 3, 0, 3},
        {LF_NOM_U, 0, LB_G_UN, A, 0, 6, 2, 0, 2}, {LF_NOM_U, 2, LB_G_UN, A, 3, 6, 3, 0, 3},
        {LF_COST_r, 0, LB_G_Cr, A, 0, 6, 2, 0, 2}, {LF_COST_r, 1, LB_G_Cr, A, 2, 6, 1, 0, 1},
        {LF_COST_c, 0, LB_G_Cc, A, 0, 4, 1, 0, 1}, {LF_COST_c, 2, LB_G_Cc, A, 2, 4, 1, 0, 1}, {LF_COST_c, 3, LB_G_Cc, A, 3, 4, 1, 0, 1},
        {LF_COST_Q, 0, LB_G_CQ, A, 0, 54, 9, 0, 9}, {LF_COST_Q, 1, LB_G_CQ, A, 9, 54, 25, 0, 25}, {LF_COST_Q, 2, LB_G_CQ, A, 34, 54, 4, 0, 4},
        {LF_COST_Q, 3, LB_G_CQ, A, 38, 54, 16, 0, 16},
        {LF_COST_R, 0, LB_G_CR, A, 0, 14, 4, 0, 4}, {LF_COST_R, 1, LB_G_CR, A, 4, 14, 1, 0, 1}, {LF_COST_R, 2, LB_G_CR, A, 5, 14, 9, 0, 9},
        {LF_COST_H, 0, LB_G_CH, A, 0, 17, 6, 0, 6}, {LF_COST_H, 1, LB_G_CH, A, 6, 17, 5, 0, 5}, {LF_COST_H, 2, LB_G_CH, A, 11, 17, 6, 0, 6},
        {LF_COST_Qd, 0, none, 0, 0, 0, 0, 0, 0}, {LF_COST_Rd, 1, none, 0, 0, 0, 0, 0, 0}};
    expect(s, "per-knot-point dimensions", w);
    structure(s, "per-knot-point dimensions");
    CHECK(loop_field_run(s, LF_COST_q, 1, 3) == 3);
  }
  if (failures) { std::printf("loop_fields_test: %d failures\n", failures); return 1; }
  std::printf("loop_fields_test ok\n");
  return 0;
}
