// loop_route.h against rows written out by hand from the launchers it replaced: the steps of an operation with kernel id,
// grid, block, dynamic LDS, mode and model kind.  Plain g++, nothing of the library linked.  batch = 5 (odd: (b + 1) / 2, (b + 3) / 4 and
// mf_grid all round) and N = 33 (three MD_AFF_CHUNK chunks) unless a row says otherwise; N = 8 for one chunk.
//   batch 5: mf_grid(5) = 8 waves, mf_grid(3) = 8 pairs, 2 rows of four.  N = 33: 34 knot points -> 68 = 2 * 34, 66 = 2 * 33, 170 = 5 * 34,
//   11 = ceil(5 * 34 * 16 / 256) rounded down from 2975 / 256.  N = 8: 9 knot points -> 18, 16, 45, 3.
//   Gpad_count: 162 (AL_GP_DEF) per slot definition -> 2 slots 324 elements = 2592 bytes, 4 slots 648 = 5184 bytes.
#include <cstdio>
#include <set>
#include <vector>

#include "loop_route.h"

using namespace altro_hip;
using namespace altro_hip::capi;

static int failures = 0;

struct Want { bool rtc; int id; unsigned gx, gy, gz, block, lds; int mode, kind, chunks; };

static void expect(const char* name, const RouteShape& s, const RouteCall& c, int error, const std::vector<Want>& wants) {
  const Route r = loop_route(s, c);
  bool same = r.error == error && r.count == (int)wants.size();
  for (int i = 0; same && i < r.count; ++i) {
    const RouteStep& g = r.step[i];
    const Want& w = wants[i];
    same = g.rtc == w.rtc && g.id == w.id && g.gx == w.gx && g.gy == w.gy && g.gz == w.gz && g.block == w.block && g.lds == w.lds && g.mode == w.mode &&
           g.kind == w.kind && g.chunks == w.chunks;
  }
  if (!same) {
    ++failures;
    std::printf("%s (which %d): error %d, %d steps; want error %d, %d steps\n", name, c.which, r.error, r.count, error, (int)wants.size());
    for (int i = 0; i < r.count; ++i) {
      const RouteStep& g = r.step[i];
      std::printf("  got  %d: rtc %d id %#x grid %u %u %u block %u lds %u mode %d kind %d chunks %d\n", i, (int)g.rtc, g.id, g.gx, g.gy, g.gz, g.block, g.lds, g.mode, g.kind, g.chunks);
    }
    for (size_t i = 0; i < wants.size(); ++i) {
      const Want& g = wants[i];
      std::printf("  want %d: rtc %d id %#x grid %u %u %u block %u lds %u mode %d kind %d chunks %d\n", (int)i, (int)g.rtc, g.id, g.gx, g.gy, g.gz, g.block, g.lds, g.mode, g.kind, g.chunks);
    }
  }
}

static AlSummary blocks(int max_ncon, int all_sel, int has_soc, bool has_user, int gpad) {
  AlSummary a;
  a.max_ncon = max_ncon; a.all_sel = all_sel; a.has_soc = has_soc; a.has_user = has_user; a.Gpad_count = gpad;
  return a;
}
static RouteShape tile(bool f64, int N, int model, bool dense, unsigned forms, bool al, const AlSummary& sum = AlSummary{}) {
  return RouteShape{ALTRO_HIP_PLAN_MFMA16, f64, false, 12, 4, N, 5, model, dense, false, forms, al, sum, false};
}
static RouteShape lane(bool f64, int n, int m, int N, int batch, int model, bool dense, bool split) {
  return RouteShape{ALTRO_HIP_PLAN_LANE, f64, false, n, m, N, batch, model, dense, split, 0, false, AlSummary{}, false};
}
// plans GENERIC / MFMA32, batch 5; blocks: 0 none, 1 every block fits the row layout (AlSummary::row32_ok), 2 some block does not, 3 a block from the source
static RouteShape gen(bool f64, int n, int m, int N, int model, unsigned forms, int blocks, bool ragged = false, bool row_ok = false) {
  AlSummary a;
  a.row32_ok = blocks == 1; a.has_user = blocks == 3; a.max_ncon = blocks ? 1 : 0;
  return RouteShape{ALTRO_HIP_PLAN_GENERIC, f64, ragged, n, m, N, 5, model, true, false, forms, blocks != 0, a, row_ok};
}

// what the launcher units carry (ilqr_launch_mfma16.hip, _model.hip, _wide.hip, ilqr_launch_generic.hip, row32_unit.inc, row32_model.hip, ilqr_launch_f64.hip / _f32.hip), written out: every id a route returns is one of
// these, in the unit route_unit names, and every one of these is returned by some route below
static std::set<int> carried(int unit, bool f64) {
  std::set<int> ids;
  const int KF_AL = capi::KF_AL, KF_DUAL = capi::KF_DUAL, KF_DENSE = capi::KF_DENSE, KF_SOC = capi::KF_SOC, KF_AFF = capi::KF_AFF;   // (as ints: the lists below mix them with 0)
  if (unit == RU_MFMA16) {
    ids = {K_WAVE_ROLLOUT, K_WAVE_ACCEPT, K_WAVE_EXPAND_DPP | KF_DENSE, K_WAVE_EXPAND_DPP | KF_ALLSEL, K_WAVE_EXPAND_DPP, K_WAVE_EXPAND_LDS, K_WAVE_EXPAND_GRAD | KF_DENSE,
           K_WAVE_EXPAND_GRAD, K_WAVE_DUAL_DPP, K_WAVE_DUAL_LDS, K_WAVE_MERIT_LDS | KF_AL, K_WAVE_MERIT_LDS, K_WAVE_SPEC_SELECT, K_WAVE_STATIONARITY, K_WAVE_FEAS_DPP, K_WAVE_SHIFT};
    for (int dual : {0, KF_DUAL})
      for (int dense : {0, KF_DENSE})
        for (int v : {KF_AL, KF_AL | KF_SOC, KF_SOC}) {
          ids.insert(K_WAVE_MERIT_DPP | dual | dense | v);
          if (f64 && !dual) ids.insert(K_WAVE_MERIT_DPP | dense | v | KF_AFF);
        }
    if (f64) ids.insert(K_WAVE_AFF_REDUCE);
  } else if (unit == RU_MFMA16_MODEL && f64) {
    ids = {K_WAVE_ROLLOUT | KF_MODEL, K_WAVE_EXPAND_DYN | KF_MODEL};
    for (int dual : {0, KF_DUAL})
      for (int dense : {0, KF_DENSE})
        for (int al : {0, KF_AL}) ids.insert(K_WAVE_MERIT_DPP | KF_MODEL | KF_SOC | dual | dense | al);
  } else if (unit == RU_MFMA16_WIDE && f64) {
    ids = {K_WAVE_EXPAND_DPP | KF_WIDE | KF_DENSE, K_WAVE_EXPAND_DPP | KF_WIDE | KF_ALLSEL, K_WAVE_EXPAND_DPP | KF_WIDE, K_WAVE_AFF_REDUCE | KF_WIDE};
    for (int dense : {0, KF_DENSE}) {
      for (int soc : {0, KF_SOC})
        for (int v : {0, KF_DUAL, KF_AFF}) ids.insert(K_WAVE_MERIT_DPP | KF_WIDE | KF_AL | dense | soc | v);
      for (int dual : {0, KF_DUAL}) ids.insert(K_WAVE_MERIT_DPP | KF_WIDE | KF_MODEL | KF_AL | KF_SOC | dense | dual);
    }
  } else if (unit == RU_GENERIC) {
    ids = {K_GEN_ROLLOUT, K_GEN_ACCEPT, K_GEN_EXPAND_AL, K_GEN_EXPAND, K_GEN_DUAL, K_GEN_MERIT | KF_STAGED, K_GEN_MERIT, K_GEN_STATIONARITY, K_GEN_SHIFT};
    if (f64) for (int id : {K_GEN_ROLLOUT | KF_MODEL, K_GEN_MERIT | KF_MODEL, K_GEN_EXPAND_DYN | KF_MODEL}) ids.insert(id);
  } else if (unit == RU_ROW32 && f64) {
    ids = {K_ROW_MERIT, K_ROW_MERIT | KF_DUAL, K_ROW_INIT, K_ROW_STAT, K_ROW_STAT_REDUCE, K_ROW_EXPAND};
  } else if (unit == RU_ROW32_MODEL && f64) {
    ids = {K_ROW_MERIT | KF_MODEL, K_ROW_EXPAND_DYN | KF_MODEL, K_ROW_MERIT | KF_DUAL | KF_MODEL};
  } else if (unit == RU_LANE) {
    for (int w = 0; w < RTC_NUM; ++w) ids.insert(lane_id(w));
    for (int w : {RTC_EXPAND, RTC_MERIT_POINT, RTC_MERIT}) ids.insert(lane_id(w, true));
  }
  return ids;
}

// every shape x operation x mode: the ids stay inside what the units carry, run-time steps have a slot, no route is longer than the array
// the same for plans GENERIC / MFMA32 and LANE: shapes with and without the row layout, every model, blocks of every kind
static void sweep_generic_lane() {
  const int whichs[] = {IK_ROLLOUT, IK_ACCEPT, IK_EXPAND, IK_MERIT, IK_STATIONARITY, IK_DUAL, IK_SHIFT, IK_SPEC_SELECT, IK_MERIT2};
  const int modes[] = {0, 2, ROLLOUT_INIT, EXPAND_GRADIENT, EXPAND_HESSIAN, EXPAND_GRADIENT | EXPAND_HESSIAN, EXPAND_HESSIAN | EXPAND_DIAG};
  const int nm[3][2] = {{13, 4}, {4, 2}, {20, 12}};
  std::set<int> lib[2], slots;
  const auto take = [&](const RouteShape& s, const Route& r, int f64, int slot_count) {
    if (r.count < 0 || r.count > ROUTE_MAX_STEPS || (r.error && r.count)) { ++failures; std::printf("sweep: count %d error %d\n", r.count, r.error); return; }
    for (int i = 0; i < r.count; ++i) {
      const RouteStep& st = r.step[i];
      if (st.rtc) {
        slots.insert(st.id >= K_LANE ? 100 + route_rtc_slot(st.id) : route_rtc_slot(st.id));
        if (route_rtc_slot(st.id) < 0 || route_rtc_slot(st.id) >= slot_count || s.model != MODEL_USER) { ++failures; std::printf("sweep: run-time step %#x without a slot or a source\n", st.id); }
      } else {
        lib[f64].insert(st.id);
        if (!carried(route_unit(st.id), f64 != 0).count(st.id)) { ++failures; std::printf("sweep: id %#x (f64 %d) is in no launcher unit\n", st.id, f64); }
        if ((st.id & KF_MODEL) && st.id < K_LANE && s.model != MODEL_QUADROTOR13) { ++failures; std::printf("sweep: model id %#x from the library without its model\n", st.id); }
      }
      if (!st.gx || !st.gy || st.gz != 1 || (st.block != 64 && st.block != 256)) { ++failures; std::printf("sweep: id %#x: empty grid or odd block\n", st.id); }
    }
  };
  for (int f64 = 0; f64 < 2; ++f64)
    for (const auto& d : nm)
      for (int model : {(int)MODEL_LINEAR, (int)MODEL_QUADROTOR13, (int)MODEL_USER})
        for (unsigned fm : {0u, (unsigned)ALTRO_HIP_FORM_GENERIC_MERIT_LDS})
          for (int blocks = 0; blocks < 4; ++blocks)
            for (int flags = 0; flags < 8; ++flags) {   // ragged | row_ok | stat_part
              const bool ragged = flags & 1, row_ok = flags & 2, stat_part = flags & 4;
              if ((model != MODEL_LINEAR && (!f64 || ragged)) || (model == MODEL_QUADROTOR13 && d[0] != 13) || (blocks == 3 && model != MODEL_USER)) continue;   // (what the setters refuse)
              const RouteShape s = gen(f64 != 0, d[0], d[1], 33, model, fm, blocks, ragged, row_ok);
              for (int which : whichs)
                for (int mode : modes) take(s, loop_route(s, RouteCall{which, mode, 1, false, stat_part}), f64, RTG_NUM_ALL);
            }
  for (int f64 = 0; f64 < 2; ++f64)
    for (int model : {(int)MODEL_BICYCLE, (int)MODEL_USER})
      for (int flags = 0; flags < 4; ++flags) {   // dense | split
        const RouteShape s = lane(f64 != 0, 4, 2, 33, 5, model, flags & 1, flags & 2);
        for (int which : whichs) take(s, loop_route(s, RouteCall{which, 0, 3}), f64, RTC_NUM);
      }
  for (int f64 = 0; f64 < 2; ++f64)
    for (int unit : {RU_GENERIC, RU_ROW32, RU_ROW32_MODEL, RU_LANE})
      for (int id : carried(unit, f64 != 0))
        if (!lib[f64].count(id)) { ++failures; std::printf("sweep: no route returns id %#x (f64 %d) of unit %d\n", id, f64, unit); }
  if ((int)slots.size() != RTG_NUM_ALL + RTC_NUM) { ++failures; std::printf("sweep: %d of the modules' %d slots are reached\n", (int)slots.size(), (int)(RTG_NUM_ALL + RTC_NUM)); }
}

static void sweep() {
  const int whichs[] = {IK_ROLLOUT, IK_ACCEPT, IK_EXPAND, IK_MERIT, IK_STATIONARITY, IK_DUAL, IK_SHIFT, IK_SPEC_SELECT, IK_MERIT2};
  const int modes[] = {0, 2, ROLLOUT_INIT, EXPAND_GRADIENT, EXPAND_HESSIAN, EXPAND_GRADIENT | EXPAND_HESSIAN, EXPAND_GRADIENT | EXPAND_HESSIAN | EXPAND_NEXT | EXPAND_DUAL};
  const unsigned forms[] = {0, ALTRO_HIP_FORM_MERIT_LDS, ALTRO_HIP_FORM_MERIT_DPP_ALWAYS, ALTRO_HIP_FORM_ALROWS_LDS, ALTRO_HIP_FORM_EXPAND_LDS};
  const AlSummary sums[] = {blocks(2, 1, 0, false, 324), blocks(2, 0, 0, false, 324), blocks(2, 0, 1, false, 324), blocks(4, 1, 0, false, 648),
                            blocks(4, 0, 0, false, 648), blocks(4, 0, 1, false, 648), blocks(1, 0, 0, true, 0), blocks(3, 0, 0, true, 324)};
  std::set<int> lib[2], rtc;
  for (int f64 = 0; f64 < 2; ++f64)
    for (int model : {(int)MODEL_LINEAR, (int)MODEL_QUADROTOR, (int)MODEL_USER})
      for (int dense = 0; dense < 2; ++dense)
        for (unsigned fm : forms)
          for (int ia = -1; ia < 8; ++ia)
            for (int which : whichs)
              for (int mode : modes)
                for (int aff = 0; aff < 2; ++aff) {
                  if (ia >= 0 && sums[ia].has_user && model != MODEL_USER) continue;   // (a slot from source needs the source)
                  const RouteShape s = tile(f64 != 0, 33, model, dense != 0, fm, ia >= 0, ia >= 0 ? sums[ia] : AlSummary{});
                  const Route r = loop_route(s, RouteCall{which, mode, 3, aff != 0});
                  if (r.count < 0 || r.count > ROUTE_MAX_STEPS || (r.error && r.count)) { ++failures; std::printf("sweep: count %d error %d\n", r.count, r.error); continue; }
                  for (int i = 0; i < r.count; ++i) {
                    const RouteStep& st = r.step[i];
                    if (st.rtc) {
                      rtc.insert(st.id);
                      if (route_rtc_slot(st.id) < 0 || model != MODEL_USER) { ++failures; std::printf("sweep: run-time step %#x without a slot or a source\n", st.id); }
                    } else {
                      lib[f64].insert(st.id);
                      if (!carried(route_unit(st.id), f64 != 0).count(st.id)) { ++failures; std::printf("sweep: id %#x (f64 %d) is in no launcher unit\n", st.id, f64); }
                    }
                    if (!st.gx || !st.gy || !st.gz || (st.block != 64 && st.block != 256)) { ++failures; std::printf("sweep: id %#x: empty grid or odd block\n", st.id); }
                  }
                }
  for (int f64 = 0; f64 < 2; ++f64)
    for (int unit : {RU_MFMA16, RU_MFMA16_MODEL, RU_MFMA16_WIDE})
      for (int id : carried(unit, f64 != 0))
        if (!lib[f64].count(id)) { ++failures; std::printf("sweep: no route returns id %#x (f64 %d) of unit %d\n", id, f64, unit); }
  // the run-time module's kernels (rtc_unit.h: rtc_unit_tile), by slot
  std::set<int> slots;
  for (int id : rtc) slots.insert(route_rtc_slot(id));
  if ((int)slots.size() != RTT_NUM_ALL) { ++failures; std::printf("sweep: %d of the module's %d slots are reached\n", (int)slots.size(), (int)RTT_NUM_ALL); }
}

int main() {
  const int LIN = MODEL_LINEAR, QUAD = MODEL_QUADROTOR, USER = MODEL_USER;
  const int GH = EXPAND_GRADIENT | EXPAND_HESSIAN, NF = STAT_NO_FEAS;
  const bool L = false, R = true;   // a step's origin: library, run-time module

  {   // no blocks, diagonal cost, dynamics as data
    const RouteShape s = tile(true, 33, LIN, false, 0, false);
    expect("plain", s, {IK_ROLLOUT, ROLLOUT_INIT, 1, false}, 0, {{L, K_WAVE_ROLLOUT, 8, 1, 1, 64, 0, ROLLOUT_INIT, LIN, 0}});
    expect("plain", s, {IK_ACCEPT, 0, 1, false}, 0, {{L, K_WAVE_ACCEPT, 11, 1, 1, 256, 0, 0, LIN, 0}});
    expect("plain", s, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_GRAD, 11, 1, 1, 256, 0, GH, LIN, 0}});
    expect("plain hessian only", s, {IK_EXPAND, EXPAND_HESSIAN, 1, false}, 0, {});
    expect("plain", s, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC, 8, 1, 1, 64, 0, 2, LIN, 0}});
    expect("plain 4 trials", s, {IK_MERIT, 0, 4, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC, 8, 2, 1, 64, 0, 2, LIN, 0}});
    expect("plain 5 trials", s, {IK_MERIT, 0, 5, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC, 8, 3, 1, 64, 0, 2, LIN, 0}});
    expect("plain", s, {IK_MERIT2, 2, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_DUAL, 8, 1, 1, 64, 0, 2, LIN, 0}});
    expect("plain affine", s, {IK_MERIT, 0, 4, true}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_AFF, 8, 2, 3, 64, 0, 2, LIN, 0}, {L, K_WAVE_AFF_REDUCE, 1, 1, 1, 256, 0, 2, LIN, 3}});
    expect("plain", s, {IK_STATIONARITY, 0, 1, false}, 0, {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, 0, LIN, 0}});
    expect("plain", s, {IK_DUAL, 0, 1, false}, 0, {{L, K_WAVE_DUAL_DPP, 68, 1, 1, 64, 0, NF, LIN, 0}});
    expect("plain", s, {IK_SHIFT, 0, 1, false}, 0, {{L, K_WAVE_SHIFT, 1, 1, 1, 256, 0, 0, LIN, 0}});
    expect("plain", s, {IK_SPEC_SELECT, 0, 1, false}, 0, {{L, K_WAVE_SPEC_SELECT, 5, 1, 1, 64, 0, 0, LIN, 0}});
    expect("plain, no such operation", s, {99, 0, 1, false}, ROUTE_NO_KERNEL, {});
    const RouteShape s8 = tile(true, 8, LIN, false, 0, false);   // one chunk everywhere
    expect("plain N 8", s8, {IK_ACCEPT, 0, 1, false}, 0, {{L, K_WAVE_ACCEPT, 3, 1, 1, 256, 0, 0, LIN, 0}});
    expect("plain N 8 affine", s8, {IK_MERIT, 0, 2, true}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_AFF, 8, 1, 1, 64, 0, 2, LIN, 0}, {L, K_WAVE_AFF_REDUCE, 1, 1, 1, 256, 0, 2, LIN, 1}});
    RouteShape s17 = s;   // batch 17: mf_grid(17) = 24 waves, mf_grid(9) = 16 pairs, 5 rows of four, ceil(8 * 17 / 256) = 1
    s17.batch = 17;
    expect("plain batch 17", s17, {IK_ROLLOUT, 0, 1, false}, 0, {{L, K_WAVE_ROLLOUT, 24, 1, 1, 64, 0, 0, LIN, 0}});
    expect("plain batch 17", s17, {IK_MERIT2, 2, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_DUAL, 16, 1, 1, 64, 0, 2, LIN, 0}});
    expect("plain batch 17", s17, {IK_DUAL, 0, 1, false}, 0, {{L, K_WAVE_DUAL_DPP, 170, 1, 1, 64, 0, NF, LIN, 0}});
  }
  {   // dense cost, no blocks
    const RouteShape s = tile(true, 33, LIN, true, 0, false);
    expect("dense", s, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_GRAD | KF_DENSE, 11, 1, 1, 256, 0, GH, LIN, 0}});
    expect("dense", s, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_DENSE, 8, 1, 1, 64, 0, 2, LIN, 0}});
    expect("dense", s, {IK_MERIT2, 2, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_DENSE | KF_DUAL, 8, 1, 1, 64, 0, 2, LIN, 0}});
  }
  {   // two slots, all bound-type
    const RouteShape s = tile(true, 33, LIN, false, 0, true, blocks(2, 1, 0, false, 324));
    expect("bounds", s, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_ALLSEL, 68, 1, 1, 64, 0, GH, LIN, 0}});
    expect("bounds", s, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL, 8, 1, 1, 64, 2592, 2, LIN, 0}});
    expect("bounds", s, {IK_MERIT2, 2, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_DUAL, 8, 1, 1, 64, 2592, 2, LIN, 0}});
    expect("bounds affine", s, {IK_MERIT, 0, 2, true}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_AFF, 8, 1, 3, 64, 2592, 2, LIN, 0}, {L, K_WAVE_AFF_REDUCE, 1, 1, 1, 256, 0, 2, LIN, 3}});
    expect("bounds", s, {IK_STATIONARITY, 0, 1, false}, 0, {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, NF, LIN, 0}, {L, K_WAVE_FEAS_DPP, 68, 1, 1, 64, 0, NF, LIN, 0}});
    expect("bounds", s, {IK_DUAL, 0, 1, false}, 0, {{L, K_WAVE_DUAL_DPP, 68, 1, 1, 64, 0, NF, LIN, 0}});
    const RouteShape s8 = tile(true, 8, LIN, false, 0, true, blocks(2, 1, 0, false, 324));
    expect("bounds N 8", s8, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_ALLSEL, 18, 1, 1, 64, 0, GH, LIN, 0}});
    const RouteShape f = tile(false, 33, LIN, false, 0, true, blocks(2, 1, 0, false, 324));   // fp32 records: the same kernels, no affine trials
    expect("bounds fp32", f, {IK_MERIT, 0, 2, true}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL, 8, 1, 1, 64, 2592, 2, LIN, 0}});
    expect("bounds fp32", f, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_ALLSEL, 68, 1, 1, 64, 0, GH, LIN, 0}});
  }
  {   // a dense block; a cone
    const RouteShape s = tile(true, 33, LIN, false, 0, true, blocks(1, 0, 0, false, 162));
    expect("dense block", s, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP, 68, 1, 1, 64, 0, GH, LIN, 0}});
    expect("dense block", s, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL, 8, 1, 1, 64, 1296, 2, LIN, 0}});
    const RouteShape c = tile(true, 33, LIN, false, 0, true, blocks(1, 0, 1, false, 162));
    expect("cone", c, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC, 8, 1, 1, 64, 1296, 2, LIN, 0}});
    expect("cone", c, {IK_MERIT2, 2, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_DUAL, 8, 1, 1, 64, 1296, 2, LIN, 0}});
    const RouteShape cd = tile(true, 33, LIN, true, 0, true, blocks(1, 0, 1, false, 162));
    expect("cone, dense cost", cd, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_DENSE, 68, 1, 1, 64, 0, GH, LIN, 0}});
    expect("cone, dense cost", cd, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_DENSE, 8, 1, 1, 64, 1296, 2, LIN, 0}});
  }
  {   // four slots: the wide kernels, with the diagonal and the dense cost
    const RouteShape s = tile(true, 33, LIN, false, 0, true, blocks(4, 1, 0, false, 648));
    expect("wide", s, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_WIDE | KF_ALLSEL, 68, 1, 1, 64, 0, GH, LIN, 0}});
    expect("wide", s, {IK_MERIT, 0, 4, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_WIDE, 8, 2, 1, 64, 5184, 2, LIN, 0}});
    expect("wide", s, {IK_MERIT2, 2, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_WIDE | KF_DUAL, 8, 1, 1, 64, 5184, 2, LIN, 0}});
    expect("wide affine", s, {IK_MERIT, 0, 4, true}, 0,
           {{L, K_WAVE_MERIT_DPP | KF_AL | KF_WIDE | KF_AFF, 8, 2, 3, 64, 5184, 2, LIN, 0}, {L, K_WAVE_AFF_REDUCE | KF_WIDE, 1, 1, 1, 256, 0, 2, LIN, 3}});
    expect("wide", s, {IK_DUAL, 0, 1, false}, 0, {{L, K_WAVE_DUAL_DPP, 68, 1, 1, 64, 0, NF, LIN, 0}});
    const RouteShape d = tile(true, 33, LIN, true, 0, true, blocks(4, 0, 1, false, 648));
    expect("wide dense", d, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_WIDE | KF_DENSE, 68, 1, 1, 64, 0, GH, LIN, 0}});
    expect("wide dense", d, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_WIDE | KF_DENSE, 8, 1, 1, 64, 5184, 2, LIN, 0}});
    const RouteShape f = tile(false, 33, LIN, false, 0, true, blocks(4, 1, 0, false, 648));   // fp32 records have no wide kernels
    expect("wide fp32", f, {IK_MERIT, 0, 1, false}, ROUTE_NO_KERNEL, {});
    expect("wide fp32", f, {IK_EXPAND, GH, 1, false}, ROUTE_NO_KERNEL, {});
    expect("wide fp32", f, {IK_ROLLOUT, 0, 1, false}, 0, {{L, K_WAVE_ROLLOUT, 8, 1, 1, 64, 0, 0, LIN, 0}});
  }
  {   // MODEL_QUADROTOR: the dynamics expansion before the cost's; no affine trials
    const RouteShape s = tile(true, 33, QUAD, false, 0, true, blocks(2, 1, 0, false, 324));
    expect("quadrotor", s, {IK_ROLLOUT, 0, 1, false}, 0, {{L, K_WAVE_ROLLOUT | KF_MODEL, 2, 1, 1, 64, 0, 0, QUAD, 0}});
    expect("quadrotor", s, {IK_EXPAND, GH, 1, false}, 0,
           {{L, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, QUAD, 0}, {L, K_WAVE_EXPAND_DPP | KF_ALLSEL, 68, 1, 1, 64, 0, GH | EXPAND_DYN, QUAD, 0}});
    expect("quadrotor refresh", s, {IK_EXPAND, GH | EXPAND_NEXT, 1, false}, 0, {{L, K_WAVE_EXPAND_DPP | KF_ALLSEL, 68, 1, 1, 64, 0, GH | EXPAND_NEXT, QUAD, 0}});
    expect("quadrotor", s, {IK_MERIT, 0, 4, true}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL, 8, 2, 1, 64, 2592, 2, QUAD, 0}});
    expect("quadrotor", s, {IK_MERIT2, 2, 4, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_DUAL, 8, 1, 1, 64, 2592, 2, QUAD, 0}});
    expect("quadrotor", s, {IK_STATIONARITY, 0, 1, false}, 0, {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, NF, QUAD, 0}, {L, K_WAVE_FEAS_DPP, 68, 1, 1, 64, 0, NF, QUAD, 0}});
    const RouteShape w = tile(true, 33, QUAD, true, 0, true, blocks(4, 0, 0, false, 648));
    expect("quadrotor wide", w, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_WIDE | KF_DENSE, 8, 1, 1, 64, 5184, 2, QUAD, 0}});
    expect("quadrotor wide", w, {IK_EXPAND, GH, 1, false}, 0,
           {{L, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, QUAD, 0}, {L, K_WAVE_EXPAND_DPP | KF_WIDE | KF_DENSE, 68, 1, 1, 64, 0, GH | EXPAND_DYN, QUAD, 0}});
    const RouteShape n = tile(true, 33, QUAD, false, ALTRO_HIP_FORM_MERIT_LDS, false);   // (a device model: row-layout kernels whatever the form)
    expect("quadrotor, no blocks", n, {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_SOC | KF_MODEL, 8, 1, 1, 64, 0, 0, QUAD, 0}});
    expect("quadrotor, no blocks", n, {IK_EXPAND, GH, 1, false}, 0,
           {{L, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, QUAD, 0}, {L, K_WAVE_EXPAND_GRAD, 11, 1, 1, 256, 0, GH | EXPAND_DYN, QUAD, 0}});
    expect("a model the tile plan does not carry", tile(true, 33, MODEL_BICYCLE, false, 0, false), {IK_ROLLOUT, 0, 1, false}, ROUTE_NO_KERNEL, {});
    expect("a model on fp32 records", tile(false, 33, QUAD, false, 0, false), {IK_ROLLOUT, 0, 1, false}, ROUTE_NO_KERNEL, {});
  }
  {   // MODEL_USER: the model's kernels from the run-time module; the library's kernels next to them see MODEL_LINEAR
    const RouteShape s0 = tile(true, 33, USER, false, 0, false);
    expect("source", s0, {IK_ROLLOUT, 0, 1, false}, 0, {{R, K_WAVE_ROLLOUT | KF_MODEL, 2, 1, 1, 64, 0, 0, USER, 0}});
    expect("source", s0, {IK_EXPAND, GH, 1, false}, 0,
           {{R, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}, {L, K_WAVE_EXPAND_GRAD, 11, 1, 1, 256, 0, GH | EXPAND_DYN, LIN, 0}});
    expect("source", s0, {IK_MERIT, 0, 4, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_SOC | KF_MODEL, 8, 2, 1, 64, 0, 2, USER, 0}});
    expect("source", s0, {IK_MERIT2, 2, 4, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_SOC | KF_MODEL | KF_DUAL, 8, 1, 1, 64, 0, 2, USER, 0}});
    expect("source", s0, {IK_STATIONARITY, 0, 1, false}, 0, {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, 0, LIN, 0}});
    expect("source", s0, {IK_ACCEPT, 0, 1, false}, 0, {{L, K_WAVE_ACCEPT, 11, 1, 1, 256, 0, 0, LIN, 0}});
    const RouteShape s2 = tile(true, 33, USER, true, 0, true, blocks(2, 0, 0, false, 324));
    expect("source, 2 slots", s2, {IK_MERIT, 0, 1, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_DENSE, 8, 1, 1, 64, 2592, 2, USER, 0}});
    expect("source, 2 slots", s2, {IK_EXPAND, GH, 1, false}, 0,
           {{R, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}, {L, K_WAVE_EXPAND_DPP | KF_DENSE, 68, 1, 1, 64, 0, GH | EXPAND_DYN, LIN, 0}});
    expect("source, 2 slots", s2, {IK_DUAL, 0, 1, false}, 0, {{L, K_WAVE_DUAL_DPP, 68, 1, 1, 64, 0, NF, LIN, 0}});
    expect("source, 2 slots", s2, {IK_STATIONARITY, 0, 1, false}, 0, {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, NF, LIN, 0}, {L, K_WAVE_FEAS_DPP, 68, 1, 1, 64, 0, NF, LIN, 0}});
    if (route_tile_module_key(s2) != (1 | 2)) { ++failures; std::printf("module key of a dense cost with blocks\n"); }
    // a source model with more than two slots ran the two-slot merit kernel -- the id is the wide one, in the merit slot
    const RouteShape s4 = tile(true, 33, USER, false, 0, true, blocks(4, 1, 0, false, 648));
    expect("source, 4 slots", s4, {IK_MERIT, 0, 1, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_WIDE, 8, 1, 1, 64, 5184, 2, USER, 0}});
    expect("source, 4 slots", s4, {IK_MERIT2, 2, 1, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_WIDE | KF_DUAL, 8, 1, 1, 64, 5184, 2, USER, 0}});
    expect("source, 4 slots", s4, {IK_EXPAND, GH, 1, false}, 0,
           {{R, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}, {L, K_WAVE_EXPAND_DPP | KF_WIDE | KF_ALLSEL, 68, 1, 1, 64, 0, GH | EXPAND_DYN, LIN, 0}});
    if (route_tile_module_key(s4) != (1 | 4) || route_rtc_slot(K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_WIDE) != RTT_MERIT) { ++failures; std::printf("module key / slot of the wide merit kernel\n"); }
    // a slot from the source and no block given as data: the rows' kernels from the module too; one definition's worth of LDS (162 * 8)
    const RouteShape su = tile(true, 33, USER, false, 0, true, blocks(1, 0, 0, true, 0));
    expect("source slot", su, {IK_MERIT, 0, 1, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL, 8, 1, 1, 64, 1296, 2, USER, 0}});
    expect("source slot", su, {IK_EXPAND, GH, 1, false}, 0,
           {{R, K_WAVE_EXPAND_DYN | KF_MODEL, 66, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}, {R, K_WAVE_EXPAND_DPP, 68, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}});
    expect("source slot refresh", su, {IK_EXPAND, GH | EXPAND_NEXT | EXPAND_DUAL, 1, false}, 0, {{R, K_WAVE_EXPAND_DPP, 68, 1, 1, 64, 0, GH | EXPAND_NEXT | EXPAND_DUAL, USER, 0}});
    expect("source slot", su, {IK_DUAL, 0, 1, false}, 0, {{R, K_WAVE_DUAL_DPP, 68, 1, 1, 64, 0, NF, USER, 0}});
    expect("source slot", su, {IK_STATIONARITY, 0, 1, false}, 0,
           {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, NF | STAT_FEAS_USER, LIN, 0}, {R, K_WAVE_FEAS_DPP, 68, 1, 1, 64, 0, NF | STAT_FEAS_USER, LIN, 0}});
    if (route_tile_module_key(su) != (1 | 8)) { ++failures; std::printf("module key of a slot from the source\n"); }
    const RouteShape sw = tile(true, 33, USER, true, 0, true, blocks(3, 0, 0, true, 324));   // ... with two slots given as data: 324 elements win
    expect("source slot, wide", sw, {IK_MERIT, 0, 1, false}, 0, {{R, K_WAVE_MERIT_DPP | KF_AL | KF_SOC | KF_MODEL | KF_WIDE | KF_DENSE, 8, 1, 1, 64, 2592, 2, USER, 0}});
    expect("source slot, wide", sw, {IK_EXPAND, EXPAND_HESSIAN, 1, false}, 0, {{R, K_WAVE_EXPAND_DPP | KF_WIDE | KF_DENSE, 68, 1, 1, 64, 0, EXPAND_HESSIAN, USER, 0}});
    if (route_tile_module_key(sw) != (1 | 2 | 4 | 8)) { ++failures; std::printf("module key of a wide handle with a slot from the source\n"); }
  }
  {   // the form bits that select a kernel
    const AlSummary b2 = blocks(2, 1, 0, false, 324);
    const RouteShape ml = tile(true, 33, LIN, false, ALTRO_HIP_FORM_MERIT_LDS, true, b2);
    expect("MERIT_LDS", ml, {IK_MERIT, 0, 4, true}, 0, {{L, K_WAVE_MERIT_LDS | KF_AL, 8, 4, 1, 64, 0, 0, LIN, 0}});
    expect("MERIT_LDS", ml, {IK_MERIT2, 2, 4, false}, 0, {{L, K_WAVE_MERIT_DPP | KF_AL | KF_DUAL, 8, 1, 1, 64, 2592, 2, LIN, 0}});
    expect("MERIT_LDS, no blocks", tile(false, 33, LIN, false, ALTRO_HIP_FORM_MERIT_LDS, false), {IK_MERIT, 0, 1, false}, 0, {{L, K_WAVE_MERIT_LDS, 8, 1, 1, 64, 0, 0, LIN, 0}});
    expect("MERIT_LDS, dense cost", tile(true, 33, LIN, true, ALTRO_HIP_FORM_MERIT_LDS, true, b2), {IK_MERIT, 0, 1, true}, 0,
           {{L, K_WAVE_MERIT_DPP | KF_AL | KF_DENSE, 8, 1, 1, 64, 2592, 0, LIN, 0}});
    expect("MERIT_LDS, wide", tile(true, 33, LIN, false, ALTRO_HIP_FORM_MERIT_LDS, true, blocks(4, 1, 0, false, 648)), {IK_MERIT, 0, 1, true}, 0,
           {{L, K_WAVE_MERIT_DPP | KF_AL | KF_WIDE, 8, 1, 1, 64, 5184, 0, LIN, 0}});
    expect("MERIT_DPP_ALWAYS", tile(true, 33, LIN, false, ALTRO_HIP_FORM_MERIT_DPP_ALWAYS, true, b2), {IK_MERIT, 0, 1, false}, 0,
           {{L, K_WAVE_MERIT_DPP | KF_AL, 8, 1, 1, 64, 2592, 3, LIN, 0}});
    const RouteShape ar = tile(true, 33, LIN, false, ALTRO_HIP_FORM_ALROWS_LDS, true, b2);
    expect("ALROWS_LDS", ar, {IK_DUAL, 0, 1, false}, 0, {{L, K_WAVE_DUAL_LDS, 170, 1, 1, 64, 0, 0, LIN, 0}});
    expect("ALROWS_LDS", ar, {IK_STATIONARITY, 0, 1, false}, 0, {{L, K_WAVE_STATIONARITY, 8, 1, 1, 64, 0, 0, LIN, 0}});
    const RouteShape el = tile(true, 33, LIN, false, ALTRO_HIP_FORM_EXPAND_LDS, true, b2);
    expect("EXPAND_LDS", el, {IK_EXPAND, GH, 1, false}, 0, {{L, K_WAVE_EXPAND_LDS, 170, 1, 1, 64, 0, GH | EXPAND_LDS, LIN, 0}});
    expect("EXPAND_LDS, no blocks", tile(true, 33, LIN, false, ALTRO_HIP_FORM_EXPAND_LDS, false), {IK_EXPAND, GH, 1, false}, 0,
           {{L, K_WAVE_EXPAND_GRAD, 11, 1, 1, 256, 0, GH | EXPAND_LDS, LIN, 0}});
    expect("EXPAND_LDS, dense cost", tile(true, 33, LIN, true, ALTRO_HIP_FORM_EXPAND_LDS, true, b2), {IK_EXPAND, GH, 1, false}, 0,
           {{L, K_WAVE_EXPAND_DPP | KF_DENSE, 68, 1, 1, 64, 0, GH, LIN, 0}});
    expect("EXPAND_LDS, wide", tile(true, 33, LIN, false, ALTRO_HIP_FORM_EXPAND_LDS, true, blocks(4, 0, 0, false, 648)), {IK_EXPAND, GH, 1, false}, 0,
           {{L, K_WAVE_EXPAND_DPP | KF_WIDE, 68, 1, 1, 64, 0, GH | EXPAND_LDS, LIN, 0}});
  }
  {   // plan LANE, bicycle (4, 2): batch 5 -> 1 block of lanes, 170 (problem, knot point) pairs -> 1 block of 256, 3 of 64; 30 shifted entries -> 1
    const int BIC = MODEL_BICYCLE;
    const RouteShape s = lane(true, 4, 2, 33, 5, BIC, false, false);
    expect("bicycle", s, {IK_ROLLOUT, 0, 1, false}, 0, {{L, lane_id(RTC_ROLLOUT), 1, 1, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle", s, {IK_ACCEPT, 0, 1, false}, 0, {{L, lane_id(RTC_ACCEPT), 1, 1, 1, 256, 0, 0, BIC, 0}});
    expect("bicycle", s, {IK_EXPAND, GH, 1, false}, 0, {{L, lane_id(RTC_EXPAND), 3, 1, 1, 64, 0, GH, BIC, 0}});
    expect("bicycle", s, {IK_MERIT, 0, 1, false}, 0, {{L, lane_id(RTC_MERIT), 1, 1, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle 4 trials", s, {IK_MERIT, 0, 4, false}, 0, {{L, lane_id(RTC_MERIT), 1, 4, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle", s, {IK_SPEC_SELECT, 0, 1, false}, 0, {{L, lane_id(RTC_SPEC_SELECT), 1, 1, 1, 256, 0, 0, BIC, 0}});
    expect("bicycle", s, {IK_DUAL, 0, 1, false}, 0, {{L, lane_id(RTC_DUAL), 1, 1, 1, 256, 0, 0, BIC, 0}});
    expect("bicycle", s, {IK_SHIFT, 0, 1, false}, 0, {{L, lane_id(RTC_SHIFT), 1, 1, 1, 256, 0, 0, BIC, 0}});
    expect("bicycle", s, {IK_STATIONARITY, 0, 1, false}, 0, {{L, lane_id(RTC_ZERO_RESIDUALS), 1, 1, 1, 256, 0, 0, BIC, 0}, {L, lane_id(RTC_STATIONARITY), 3, 1, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle, no two-trial pass", s, {IK_MERIT2, 2, 1, false}, ROUTE_NO_KERNEL, {});
    const RouteShape sp = lane(true, 4, 2, 33, 5, BIC, false, true);   // MeritFunction in three launches
    expect("bicycle split", sp, {IK_MERIT, 0, 4, false}, 0,
           {{L, lane_id(RTC_MERIT_ROLL), 1, 4, 1, 64, 0, 0, BIC, 0}, {L, lane_id(RTC_MERIT_POINT), 3, 4, 1, 64, 0, 0, BIC, 0}, {L, lane_id(RTC_MERIT_SUM), 1, 4, 1, 64, 0, 0, BIC, 0}});
    const RouteShape d = lane(false, 4, 2, 33, 5, BIC, true, true);   // the dense cost: the cost-reading kernels' CK = 1 instantiations; fp32 the same
    expect("bicycle dense", d, {IK_EXPAND, GH, 1, false}, 0, {{L, lane_id(RTC_EXPAND, true), 3, 1, 1, 64, 0, GH, BIC, 0}});
    expect("bicycle dense split", d, {IK_MERIT, 0, 1, false}, 0,
           {{L, lane_id(RTC_MERIT_ROLL), 1, 1, 1, 64, 0, 0, BIC, 0}, {L, lane_id(RTC_MERIT_POINT, true), 3, 1, 1, 64, 0, 0, BIC, 0}, {L, lane_id(RTC_MERIT_SUM), 1, 1, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle dense", lane(true, 4, 2, 33, 5, BIC, true, false), {IK_MERIT, 0, 1, false}, 0, {{L, lane_id(RTC_MERIT, true), 1, 1, 1, 64, 0, 0, BIC, 0}});
    // batch 300: 5 blocks of lanes; 10200 pairs -> 40 blocks of 256 (10455 / 256), 160 of 64 (10263 / 64); 1800 shifted entries -> 8; 2 blocks of residuals
    const RouteShape b = lane(true, 4, 2, 33, 300, BIC, false, false);
    expect("bicycle 300", b, {IK_ROLLOUT, 0, 1, false}, 0, {{L, lane_id(RTC_ROLLOUT), 5, 1, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle 300", b, {IK_ACCEPT, 0, 1, false}, 0, {{L, lane_id(RTC_ACCEPT), 40, 1, 1, 256, 0, 0, BIC, 0}});
    expect("bicycle 300", b, {IK_SHIFT, 0, 1, false}, 0, {{L, lane_id(RTC_SHIFT), 8, 1, 1, 256, 0, 0, BIC, 0}});
    expect("bicycle 300", b, {IK_STATIONARITY, 0, 1, false}, 0, {{L, lane_id(RTC_ZERO_RESIDUALS), 2, 1, 1, 256, 0, 0, BIC, 0}, {L, lane_id(RTC_STATIONARITY), 160, 1, 1, 64, 0, 0, BIC, 0}});
    expect("bicycle N 8", lane(true, 4, 2, 8, 5, BIC, false, false), {IK_EXPAND, GH, 1, false}, 0, {{L, lane_id(RTC_EXPAND), 1, 1, 1, 64, 0, GH, BIC, 0}});
    // the caller's source: every kernel from the run-time module, in the slot the id names
    const RouteShape u = lane(true, 3, 2, 33, 5, USER, true, true);
    expect("lane source", u, {IK_ACCEPT, 0, 1, false}, 0, {{R, lane_id(RTC_ACCEPT), 1, 1, 1, 256, 0, 0, USER, 0}});
    expect("lane source", u, {IK_MERIT, 0, 2, false}, 0,
           {{R, lane_id(RTC_MERIT_ROLL), 1, 2, 1, 64, 0, 0, USER, 0}, {R, lane_id(RTC_MERIT_POINT, true), 3, 2, 1, 64, 0, 0, USER, 0}, {R, lane_id(RTC_MERIT_SUM), 1, 2, 1, 64, 0, 0, USER, 0}});
    for (int w = 0; w < RTC_NUM; ++w)
      if (route_rtc_slot(lane_id(w)) != w || route_rtc_slot(lane_id(w, true)) != w || route_unit(lane_id(w, true)) != RU_LANE) { ++failures; std::printf("slot of lane kernel %d\n", w); }
    // a model plan LANE does not carry: "no device model for (kind, n, m)"
    expect("bicycle at (6, 3)", lane(true, 6, 3, 33, 5, BIC, false, false), {IK_ROLLOUT, 0, 1, false}, ROUTE_NO_MODEL, {});
    expect("no model", lane(true, 4, 2, 33, 5, LIN, false, false), {IK_ROLLOUT, 0, 1, false}, ROUTE_NO_MODEL, {});
    expect("double integrator (6, 3)", lane(true, 6, 3, 33, 5, MODEL_DOUBLE_INTEGRATOR, false, false), {IK_SHIFT, 0, 1, false}, 0, {{L, lane_id(RTC_SHIFT), 1, 1, 1, 256, 0, 0, MODEL_DOUBLE_INTEGRATOR, 0}});
  }
  {   // plans GENERIC / MFMA32, batch 5: 3 pairs of problems; N = 33: 170 (problem, knot point) pairs, 3 chunks of 16, 2 of 32; (13, 4): 17 lanes' worth
      // per knot point -> 12 blocks of 256 (3145 / 256); the rows' LDS vector 8 * 64 doubles = 4096 bytes; staged matrices 3 n n + 3 n m + m m =
      // 679 elements at (13, 4) = 5432 bytes fp64 (2560 + 5432 fits 10 KB, with the 4096 it does not), 2716 fp32 (2560 + 4096 + 2716 fits)
    const int Q13 = MODEL_QUADROTOR13, INIT = ROLLOUT_INIT;
    const unsigned LDSF = ALTRO_HIP_FORM_GENERIC_MERIT_LDS;
    const RouteShape s = gen(true, 13, 4, 33, LIN, 0, 0);   // data dynamics, no blocks: the row layout
    expect("13x4", s, {IK_ROLLOUT, INIT, 1}, 0, {{L, K_ROW_INIT, 3, 1, 1, 64, 0, INIT, LIN, 0}});
    expect("13x4", s, {IK_ROLLOUT, 0, 1}, 0, {{L, K_GEN_ROLLOUT, 5, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4", s, {IK_ACCEPT, 0, 1}, 0, {{L, K_GEN_ACCEPT, 12, 1, 1, 256, 0, 0, LIN, 0}});
    expect("13x4", s, {IK_EXPAND, GH, 1}, 0, {{L, K_GEN_EXPAND, 12, 1, 1, 256, 0, GH, LIN, 0}});
    expect("13x4", s, {IK_MERIT, 0, 1}, 0, {{L, K_ROW_MERIT, 3, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4", s, {IK_MERIT2, 2, 1}, 0, {{L, K_ROW_MERIT | KF_DUAL, 5, 1, 1, 64, 0, 2, LIN, 0}});
    expect("13x4 chunks", s, {IK_STATIONARITY, 0, 1, false, true}, 0, {{L, K_ROW_STAT, 3, 2, 1, 64, 0, 0, LIN, 0}, {L, K_ROW_STAT_REDUCE, 1, 1, 1, 256, 0, 0, LIN, 2}});
    expect("13x4 one chunk", s, {IK_STATIONARITY, 0, 1, false, false}, 0, {{L, K_ROW_STAT, 3, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4", s, {IK_DUAL, 0, 1}, 0, {{L, K_GEN_DUAL, 170, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4", s, {IK_SHIFT, 0, 1}, 0, {{L, K_GEN_SHIFT, 1, 1, 1, 256, 0, 0, LIN, 0}});
    expect("13x4", s, {IK_SPEC_SELECT, 0, 1}, ROUTE_NO_KERNEL, {});
    if (!route_two_trial(s) || !route_rollout_head(s) || !row32_eligible(s) || row32_model_eligible(s)) { ++failures; std::printf("13x4: the solve loop's questions\n"); }
    const RouteShape s8 = gen(true, 13, 4, 8, LIN, 0, 1);   // N = 8: one chunk everywhere
    expect("13x4 N 8", s8, {IK_STATIONARITY, 0, 1, false, false}, 0, {{L, K_ROW_STAT, 3, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4 N 8", s8, {IK_EXPAND, EXPAND_GRADIENT, 1}, 0, {{L, K_ROW_EXPAND, 3, 1, 1, 64, 0, EXPAND_GRADIENT, LIN, 0}});
    const RouteShape sb = gen(true, 13, 4, 33, LIN, 0, 1);   // bound-only blocks: the expansion's gradient / diagonal form in the row layout
    expect("13x4 bounds", sb, {IK_EXPAND, EXPAND_GRADIENT, 1}, 0, {{L, K_ROW_EXPAND, 3, 3, 1, 64, 0, EXPAND_GRADIENT, LIN, 0}});
    expect("13x4 bounds", sb, {IK_EXPAND, EXPAND_HESSIAN | EXPAND_DIAG, 1}, 0, {{L, K_ROW_EXPAND, 3, 3, 1, 64, 0, EXPAND_HESSIAN | EXPAND_DIAG, LIN, 0}});
    expect("13x4 bounds", sb, {IK_EXPAND, GH, 1}, 0, {{L, K_GEN_EXPAND_AL, 170, 1, 1, 64, 0, GH, LIN, 0}});
    expect("13x4 bounds", sb, {IK_MERIT, 0, 1}, 0, {{L, K_ROW_MERIT, 3, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4 bounds", sb, {IK_ROLLOUT, INIT, 1}, 0, {{L, K_ROW_INIT, 3, 1, 1, 64, 0, INIT, LIN, 0}});
    if (!route_two_trial(sb) || route_rollout_head(sb)) { ++failures; std::printf("13x4 bounds: the solve loop's questions\n"); }
    const RouteShape s40 = gen(true, 13, 4, 33, LIN, 0, 2);   // a 40-row block: the row layout is off
    expect("13x4 40 rows", s40, {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT, 5, 1, 1, 64, 4096, 0, LIN, 0}});
    expect("13x4 40 rows", s40, {IK_MERIT2, 2, 1}, ROUTE_NO_KERNEL, {});
    expect("13x4 40 rows", s40, {IK_STATIONARITY, 0, 1, false, true}, 0, {{L, K_GEN_STATIONARITY, 5, 1, 1, 64, 0, 0, LIN, 0}});
    expect("13x4 40 rows", s40, {IK_EXPAND, EXPAND_GRADIENT, 1}, 0, {{L, K_GEN_EXPAND_AL, 170, 1, 1, 64, 0, EXPAND_GRADIENT, LIN, 0}});
    expect("13x4 40 rows", s40, {IK_ROLLOUT, INIT, 1}, 0, {{L, K_GEN_ROLLOUT, 5, 1, 1, 64, 0, INIT, LIN, 0}});
    if (route_two_trial(s40) || route_rollout_head(s40)) { ++failures; std::printf("13x4 40 rows: the solve loop's questions\n"); }
    const RouteShape sl = gen(true, 13, 4, 33, LIN, LDSF, 0);   // ALTRO_HIP_FORM_GENERIC_MERIT_LDS
    expect("13x4 MERIT_LDS", sl, {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT | KF_STAGED, 5, 1, 1, 64, 5432, 0, LIN, 0}});
    expect("13x4 MERIT_LDS", sl, {IK_STATIONARITY, 0, 1}, 0, {{L, K_GEN_STATIONARITY, 5, 1, 1, 64, 0, 0, LIN, 0}});
    if (route_two_trial(sl) || route_rollout_head(sl)) { ++failures; std::printf("13x4 MERIT_LDS: the solve loop's questions\n"); }
    // MODEL_QUADROTOR13: the model's kernels, in the row layout; the cost expansion before the dynamics' ((5 * 33 + 1) / 2 = 83 pairs of knot points)
    const RouteShape q = gen(true, 13, 4, 33, Q13, 0, 0);
    expect("quad13", q, {IK_ROLLOUT, 0, 1}, 0, {{L, K_GEN_ROLLOUT | KF_MODEL, 1, 1, 1, 64, 0, 0, Q13, 0}});
    expect("quad13", q, {IK_MERIT, 0, 1}, 0, {{L, K_ROW_MERIT | KF_MODEL, 3, 1, 1, 64, 0, 0, Q13, 0}});
    expect("quad13", q, {IK_MERIT2, 2, 1}, 0, {{L, K_ROW_MERIT | KF_DUAL | KF_MODEL, 5, 1, 1, 64, 0, 2, Q13, 0}});
    expect("quad13", q, {IK_EXPAND, GH, 1}, 0, {{L, K_GEN_EXPAND, 12, 1, 1, 256, 0, GH | EXPAND_DYN, Q13, 0}, {L, K_ROW_EXPAND_DYN | KF_MODEL, 83, 1, 1, 64, 0, GH | EXPAND_DYN, Q13, 0}});
    expect("quad13", q, {IK_EXPAND, EXPAND_HESSIAN, 1}, 0, {{L, K_GEN_EXPAND, 12, 1, 1, 256, 0, EXPAND_HESSIAN, Q13, 0}});
    expect("quad13", q, {IK_STATIONARITY, 0, 1, false, true}, 0, {{L, K_ROW_STAT, 3, 2, 1, 64, 0, 0, Q13, 0}, {L, K_ROW_STAT_REDUCE, 1, 1, 1, 256, 0, 0, Q13, 2}});
    if (!route_two_trial(q) || route_rollout_head(q) || !row32_model_eligible(q)) { ++failures; std::printf("quad13: the solve loop's questions\n"); }
    const RouteShape ql = gen(true, 13, 4, 33, Q13, LDSF, 1);   // ... in the wave-per-problem kernels: 165 knot points -> 3 blocks of 64
    expect("quad13 MERIT_LDS", ql, {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT | KF_MODEL, 5, 1, 1, 64, 4096, 0, Q13, 0}});
    expect("quad13 MERIT_LDS", ql, {IK_EXPAND, GH, 1}, 0, {{L, K_GEN_EXPAND_AL, 170, 1, 1, 64, 0, GH | EXPAND_DYN, Q13, 0}, {L, K_GEN_EXPAND_DYN | KF_MODEL, 3, 1, 1, 64, 0, GH | EXPAND_DYN, Q13, 0}});
    // MODEL_USER: the model's kernels from the run-time module -- the row-layout ones where they compiled without scratch (row_ok)
    const RouteShape u = gen(true, 13, 4, 33, USER, 0, 0, false, true);
    expect("gen source", u, {IK_ROLLOUT, 0, 1}, 0, {{R, K_GEN_ROLLOUT | KF_MODEL, 1, 1, 1, 64, 0, 0, USER, 0}});
    expect("gen source", u, {IK_MERIT, 0, 1}, 0, {{R, K_ROW_MERIT | KF_MODEL, 3, 1, 1, 64, 0, 0, USER, 0}});
    expect("gen source", u, {IK_MERIT2, 2, 1}, 0, {{R, K_ROW_MERIT | KF_DUAL | KF_MODEL, 5, 1, 1, 64, 0, 2, USER, 0}});
    expect("gen source", u, {IK_EXPAND, GH, 1}, 0, {{L, K_GEN_EXPAND, 12, 1, 1, 256, 0, GH | EXPAND_DYN, LIN, 0}, {R, K_ROW_EXPAND_DYN | KF_MODEL, 83, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}});
    expect("gen source", u, {IK_STATIONARITY, 0, 1, false, false}, 0, {{L, K_ROW_STAT, 3, 1, 1, 64, 0, 0, USER, 0}});
    const RouteShape un = gen(true, 13, 4, 33, USER, 0, 0, false, false);   // ... a model whose row-layout kernels spill
    expect("gen source, not row_ok", un, {IK_MERIT, 0, 1}, 0, {{R, K_GEN_MERIT | KF_MODEL, 5, 1, 1, 64, 0, 0, USER, 0}});
    expect("gen source, not row_ok", un, {IK_MERIT2, 2, 1}, ROUTE_NO_KERNEL, {});
    expect("gen source, not row_ok", un, {IK_EXPAND, GH, 1}, 0, {{L, K_GEN_EXPAND, 12, 1, 1, 256, 0, GH | EXPAND_DYN, LIN, 0}, {R, K_GEN_EXPAND_DYN | KF_MODEL, 3, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}});
    expect("gen source, not row_ok", un, {IK_STATIONARITY, 0, 1}, 0, {{L, K_GEN_STATIONARITY, 5, 1, 1, 64, 0, 0, USER, 0}});
    if (route_two_trial(un) || !route_two_trial(u)) { ++failures; std::printf("gen source: the two-trial pass\n"); }
    const RouteShape ub = gen(true, 13, 4, 33, USER, 0, 3, false, true);   // a block from the source: every kernel that evaluates constraint rows from the module
    expect("gen source block", ub, {IK_MERIT, 0, 1}, 0, {{R, K_GEN_MERIT | KF_MODEL, 5, 1, 1, 64, 4096, 0, USER, 0}});
    expect("gen source block", ub, {IK_STATIONARITY, 0, 1}, 0, {{R, K_GEN_STATIONARITY, 5, 1, 1, 64, 0, 0, USER, 0}});
    expect("gen source block", ub, {IK_DUAL, 0, 1}, 0, {{R, K_GEN_DUAL, 170, 1, 1, 64, 0, 0, USER, 0}});
    expect("gen source block", ub, {IK_EXPAND, GH, 1}, 0, {{R, K_GEN_EXPAND_AL, 170, 1, 1, 64, 0, GH | EXPAND_DYN, LIN, 0}, {R, K_GEN_EXPAND_DYN | KF_MODEL, 3, 1, 1, 64, 0, GH | EXPAND_DYN, USER, 0}});
    expect("gen source block", ub, {IK_EXPAND, EXPAND_HESSIAN, 1}, 0, {{R, K_GEN_EXPAND_AL, 170, 1, 1, 64, 0, EXPAND_HESSIAN, LIN, 0}});
    for (int id : {K_GEN_ROLLOUT | KF_MODEL, K_GEN_EXPAND_DYN | KF_MODEL, K_GEN_MERIT | KF_MODEL, K_ROW_MERIT | KF_MODEL, K_ROW_MERIT | KF_DUAL | KF_MODEL, K_ROW_EXPAND_DYN | KF_MODEL,
                   (int)K_GEN_STATIONARITY, (int)K_GEN_EXPAND_AL, (int)K_GEN_DUAL})
      if (route_rtc_slot(id) < 0 || route_rtc_slot(id) >= RTG_NUM_ALL) { ++failures; std::printf("slot of id %#x\n", id); }
    // (4, 2) with blocks: 76 staged elements = 608 bytes next to the rows' 4096; (20, 12): 2064 elements = 16512 bytes do not fit; 32 lanes' worth -> 22 blocks
    expect("4x2 staged", gen(true, 4, 2, 33, LIN, 0, 2), {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT | KF_STAGED, 5, 1, 1, 64, 4704, 0, LIN, 0}});
    const RouteShape big = gen(true, 20, 12, 33, LIN, 0, 0);
    expect("20x12", big, {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT, 5, 1, 1, 64, 0, 0, LIN, 0}});
    expect("20x12", big, {IK_ACCEPT, 0, 1}, 0, {{L, K_GEN_ACCEPT, 22, 1, 1, 256, 0, 0, LIN, 0}});
    expect("20x12", big, {IK_MERIT2, 2, 1}, ROUTE_NO_KERNEL, {});
    const RouteShape rg = gen(true, 13, 4, 33, LIN, 0, 0, true);   // per-knot-point dimensions: no row layout
    expect("ragged", rg, {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT | KF_STAGED, 5, 1, 1, 64, 5432, 0, LIN, 0}});
    expect("ragged", rg, {IK_ROLLOUT, INIT, 1}, 0, {{L, K_GEN_ROLLOUT, 5, 1, 1, 64, 0, INIT, LIN, 0}});
    if (route_two_trial(rg) || route_rollout_head(rg)) { ++failures; std::printf("ragged: the solve loop's questions\n"); }
    const RouteShape f = gen(false, 13, 4, 33, LIN, 0, 1);   // fp32: no row layout; 2716 staged bytes fit next to the rows' vector
    expect("13x4 fp32", f, {IK_MERIT, 0, 1}, 0, {{L, K_GEN_MERIT | KF_STAGED, 5, 1, 1, 64, 6812, 0, LIN, 0}});
    expect("13x4 fp32", f, {IK_MERIT2, 2, 1}, ROUTE_NO_KERNEL, {});
    expect("13x4 fp32", f, {IK_EXPAND, EXPAND_GRADIENT, 1}, 0, {{L, K_GEN_EXPAND_AL, 170, 1, 1, 64, 0, EXPAND_GRADIENT, LIN, 0}});
    // the units: data kernels and the wave-per-problem model kernels in ilqr_launch_generic.hip, the row layout by n mod 8, its model kernels apart
    if (route_unit(K_GEN_MERIT | KF_MODEL) != RU_GENERIC || route_unit(K_ROW_STAT_REDUCE) != RU_ROW32 || route_unit(K_ROW_MERIT | KF_DUAL) != RU_ROW32 ||
        route_unit(K_ROW_EXPAND_DYN | KF_MODEL) != RU_ROW32_MODEL || route_unit(K_GEN_SHIFT) != RU_GENERIC) { ++failures; std::printf("units of plan GENERIC's ids\n"); }
    // the solve loop's questions on plan MFMA16
    const RouteShape t = tile(true, 33, LIN, false, 0, false);
    if (!route_two_trial(t) || !route_rollout_head(t) || route_rollout_head(tile(true, 33, LIN, true, 0, false)) || route_rollout_head(tile(true, 33, QUAD, false, 0, false)) ||
        route_two_trial(tile(true, 33, LIN, false, ALTRO_HIP_FORM_NO_MERIT2, false)) || route_two_trial(lane(true, 4, 2, 33, 5, MODEL_BICYCLE, false, false))) {
      ++failures; std::printf("the solve loop's questions on plans MFMA16 / LANE\n");
    }
  }
  sweep();
  sweep_generic_lane();
  if (failures) { std::printf("loop_route_test: %d failures\n", failures); return 1; }
  std::printf("loop_route_test ok\n");
  return 0;
}
