// loop_route.h -- which kernels run one operation (IK_*) of the iLQR loop: their order, grids, dynamic LDS, and the `mode` / model kind
// each of them sees.  The one place that decides; the launcher units (declared at the end) map a kernel id to its instantiation and
// capi_ilqr.hip executes the steps, from the library or from the handle's run-time module (capi_rtc.hip).  Host code, no heap:
// tests/cpp/loop_route_test.cpp checks the table with g++ against rows written out by hand.
#pragma once
#include <algorithm>
#include <cstdint>

#include "al_tables.h"
#include "kernels/ilqr_types.h"
#include "rtc_unit.h"

namespace altro_hip {
namespace capi {

// A kernel id: the instantiation family and the variant flags that pick among its instantiations.  Compiled-in and source models share
// ids (KF_MODEL; the step's model kind says which): route_rtc_slot maps an id to the run-time module's slot.
enum KernelId : int {
  // variant flags
  KF_AL = 1,        // the instantiation that evaluates constraint blocks
  KF_DUAL = 2,      // wave_merit_dpp_kernel: the two-trial pass (IK_MERIT2)
  KF_DENSE = 4,     // the dense quadratic cost
  KF_SOC = 8,       // wave_merit_dpp_kernel: with the second-order cone's code (~20 registers: only for handles that have one)
  KF_AFF = 16,      // wave_merit_dpp_kernel: affine trials, a chunk of knot points per wave (K_WAVE_AFF_REDUCE follows)
  KF_WIDE = 32,     // AL_TILE_MAXC constraint slots instead of AL_MAXC (ilqr_launch_mfma16_wide.hip; fp64 records)
  KF_MODEL = 64,    // a device model steps the dynamics (ilqr_launch_mfma16_model.hip or the run-time module; fp64 records)
  KF_ALLSEL = 128,  // wave_expand_dpp_kernel: every block is bound-type
  KF_STAGED = 128,  // generic_merit_kernel: the knot point's matrices staged in LDS
  KF_MASK = 255,
  // families: plan MFMA16 (kernels/ilqr_mfma16.hip, kernels/ilqr_merit2_dpp.hip, kernels/ilqr_tile_model.hip)
  K_WAVE_ROLLOUT = 1 << 8 /* with KF_MODEL: wave_rollout_model_kernel */, K_WAVE_ACCEPT = 2 << 8,
  K_WAVE_EXPAND_GRAD = 3 << 8,   // no constraint blocks: the Hessian is constant, the gradient is 16 entries
  K_WAVE_EXPAND_DPP = 4 << 8 /* four (problem, knot point) pairs per wave */, K_WAVE_EXPAND_LDS = 5 << 8,
  K_WAVE_EXPAND_DYN = 6 << 8,    // A_k, B_k of a device model at the stored trajectory
  K_WAVE_DUAL_DPP = 7 << 8, K_WAVE_DUAL_LDS = 8 << 8,
  K_WAVE_MERIT_DPP = 9 << 8,     // two problems per wave, two trials per problem
  K_WAVE_AFF_REDUCE = 10 << 8,   // the chunks' shares of phi / phi' added up (RouteStep::chunks)
  K_WAVE_MERIT_LDS = 11 << 8, K_WAVE_SPEC_SELECT = 12 << 8, K_WAVE_STATIONARITY = 13 << 8, K_WAVE_FEAS_DPP = 14 << 8, K_WAVE_SHIFT = 15 << 8,
  // families: plans GENERIC / MFMA32 (kernels/ilqr_generic.hip; K_ROW_*: the row layout of kernels/ilqr_row32.hip, one instantiation per (n, m))
  K_GEN_ROLLOUT = 16 << 8, K_GEN_ACCEPT = 17 << 8, K_GEN_EXPAND = 18 << 8, K_GEN_EXPAND_AL = 19 << 8, K_GEN_EXPAND_DYN = 20 << 8, K_GEN_DUAL = 21 << 8,
  K_GEN_MERIT = 22 << 8, K_GEN_STATIONARITY = 23 << 8, K_GEN_SHIFT = 24 << 8,
  K_ROW_MERIT = 25 << 8,         // two problems per wave; KF_DUAL: the two-trial pass, a problem per wave
  K_ROW_INIT = 26 << 8,          // rollout + CopyTrajectory + the first expansion of an unconstrained problem in one pass (ROLLOUT_INIT)
  K_ROW_STAT = 27 << 8, K_ROW_STAT_REDUCE = 28 << 8,   // the stationarity walk in chunks of R32_STAT_CHUNK knot points; their maxima meet in the reduce
  K_ROW_EXPAND = 29 << 8,        // constraint blocks: the gradient and the DIAGONAL form of the Hessian, chunks of R32_EXPAND_CHUNK
  K_ROW_EXPAND_DYN = 30 << 8,
  // families: plan LANE (kernels/ilqr_lane.hip), in the order of the run-time module's slots (rtc_unit.h: RtcKernel); KF_DENSE: the CK = 1 instantiation
  K_LANE = 32 << 8   // K_LANE + (RTC_ROLLOUT .. RTC_SHIFT << 8)
};
constexpr int lane_id(int slot, bool dense = false) { return K_LANE + (slot << 8) + (dense ? KF_DENSE : 0); }
// the compiled-in device models of plan LANE: (kind, n, m) of every instantiation (ilqr_launch_f64.hip, ilqr_launch_f32.hip)
#define ILQR_LANE_MODELS(X)                                                                 \
  X(MODEL_PENDULUM, 2, 1) X(MODEL_BICYCLE, 4, 2) X(MODEL_DOUBLE_INTEGRATOR, 2, 1)           \
  X(MODEL_DOUBLE_INTEGRATOR, 4, 2) X(MODEL_DOUBLE_INTEGRATOR, 6, 3)
constexpr bool lane_model_supported(int kind, int n, int m) {
#define X(K_, N_, M_) if (kind == K_ && n == N_ && m == M_) return true;
  ILQR_LANE_MODELS(X)
#undef X
  return false;
}
constexpr int merit_id(bool al, bool dual, bool dense, bool soc, bool aff = false, int more = 0) {
  return K_WAVE_MERIT_DPP | (al ? KF_AL : 0) | (dual ? KF_DUAL : 0) | (dense ? KF_DENSE : 0) | (soc ? KF_SOC : 0) | (aff ? KF_AFF : 0) | more;
}
// the launcher unit that holds a library kernel
enum RouteUnit { RU_MFMA16, RU_MFMA16_MODEL, RU_MFMA16_WIDE, RU_LANE, RU_GENERIC, RU_ROW32 /* row32_u0 .. u7.hip by n mod 8 */, RU_ROW32_MODEL };
constexpr int route_unit(int id) {
  return id >= K_LANE ? RU_LANE : id >= K_ROW_MERIT ? ((id & KF_MODEL) ? RU_ROW32_MODEL : RU_ROW32) : id >= K_GEN_ROLLOUT ? RU_GENERIC : (id & KF_WIDE) ? RU_MFMA16_WIDE : (id & KF_MODEL) ? RU_MFMA16_MODEL : RU_MFMA16;
}
// the run-time module's slot (rtc_unit.h: RtcTileKernel, RtcGenKernel, RtcKernel) of a kernel id; -1: the module has no such kernel
constexpr int route_rtc_slot(int id) {
  if (id >= K_LANE) return (id - K_LANE) >> 8;
  switch (id & ~KF_MASK) {
    case K_WAVE_ROLLOUT: return RTT_ROLLOUT;
    case K_WAVE_EXPAND_DYN: return RTT_EXPAND_DYN;
    case K_WAVE_MERIT_DPP: return (id & KF_DUAL) ? RTT_MERIT2 : RTT_MERIT;
    case K_WAVE_EXPAND_DPP: return RTT_EXPAND_AL;
    case K_WAVE_DUAL_DPP: return RTT_DUAL;
    case K_WAVE_FEAS_DPP: return RTT_FEAS;
    case K_GEN_ROLLOUT: return RTG_ROLLOUT;
    case K_GEN_EXPAND_DYN: return RTG_EXPAND_DYN;
    case K_GEN_MERIT: return RTG_MERIT;
    case K_ROW_MERIT: return (id & KF_DUAL) ? RTG_ROW_MERIT2 : RTG_ROW_MERIT;
    case K_ROW_EXPAND_DYN: return RTG_ROW_EXPAND_DYN;
    case K_GEN_STATIONARITY: return RTG_STATIONARITY;
    case K_GEN_EXPAND_AL: return RTG_EXPAND_AL;
    case K_GEN_DUAL: return RTG_DUAL;
    default: return -1;
  }
}

struct RouteShape {
  int plan;
  bool f64, ragged;
  int n, m, N, batch;
  int model;          // MODEL_LINEAR: dynamics as data; a compiled-in kind; MODEL_USER: the caller's source
  bool cost_dense;
  bool merit_split;   // plan LANE: MeritFunction in three launches (altro_hip_batch::merit_split == 1)
  unsigned forms;     // ALTRO_HIP_FORM_* (the kernel-selecting bits are read)
  bool al_enabled;    // the handle has constraint blocks; `al` describes them
  AlSummary al;
  bool row_ok;        // plans GENERIC / MFMA32, MODEL_USER: the module's row-layout kernels exist and none of them spills (capi_rtc.hip)
};
struct RouteCall {
  int which, mode, spec_trials;
  bool aff;           // affine line-search trials are on for this IK_MERIT (the route takes them only in the DPP form, dynamics as data)
  bool stat_part;     // plans GENERIC / MFMA32, IK_STATIONARITY: the buffer of the chunks' maxima exists (else one chunk)
};
enum RouteError { ROUTE_OK = 0, ROUTE_NO_KERNEL /* "operation %d is not available on plan ..." */, ROUTE_NO_MODEL /* "no device model for (kind, n, m)" */ };
struct RouteStep {
  bool rtc;           // from the handle's run-time module instead of the library
  int id;
  unsigned gx, gy, gz, block, lds;
  int mode, kind;     // what the step's argument struct carries: mode, mp.kind
  int chunks;         // K_WAVE_AFF_REDUCE, K_ROW_STAT_REDUCE: the chunks of knot points the step before it had (its grid z / y)
};
constexpr int ROUTE_MAX_STEPS = 4;
struct Route {
  int error = ROUTE_OK, count = 0;
  RouteStep step[ROUTE_MAX_STEPS] = {};
};

// The merit kernels' dynamic LDS: the padded constraint Jacobians.  (A run-time module with a slot from the source: at least one
// definition's worth -- such a slot's unused row read lands there when the handle has no block given as data.)
inline unsigned route_merit_lds(const RouteShape& s, bool rtc) {
  if (!s.al_enabled) return 0u;
  const unsigned padded = (unsigned)s.al.Gpad_count * 8u;
  return rtc && s.al.has_user ? std::max(padded, (unsigned)AL_GP_DEF * 8u) : padded;
}
// the key of the run-time tile module the shape's steps come from (altro_hip_batch::rtc_ck): constraint blocks | dense cost << 1 |
// more than AL_MAXC slots at some knot point << 2 | a slot from the source << 3
inline int route_tile_module_key(const RouteShape& s) {
  return (s.al_enabled ? 1 : 0) | (s.cost_dense ? 2 : 0) | ((s.al_enabled && s.al.max_ncon > AL_MAXC) ? 4 : 0) | ((s.al_enabled && s.al.has_user) ? 8 : 0);
}

// Plan MFMA16.  Dynamics as data: ilqr_launch_mfma16.hip; a compiled-in device model (MODEL_QUADROTOR, fp64): the model's rollout, merit
// and dynamics-expansion kernels from ilqr_launch_mfma16_model.hip, the dynamics expansion BEFORE the cost's; the caller's source
// (MODEL_USER, fp64): those from the run-time module, and every library kernel next to them sees MODEL_LINEAR (none of them steps the
// dynamics).  More than AL_MAXC slots at a knot point: the KF_WIDE merit and expansion kernels, whatever the forms say.  A slot from the
// source: expansion, dual update and feasibility walk from the run-time module (the library's instantiations know nothing of such a slot).
inline Route route_mfma16(const RouteShape& s, const RouteCall& c) {
  Route r;
  const auto frm = [&](unsigned bit) { return (s.forms & bit) != 0; };
  const bool al = s.al_enabled, wide = al && s.al.max_ncon > AL_MAXC, model = s.model != MODEL_LINEAR, user = s.model == MODEL_USER;
  const bool user_al = user && al && s.al.has_user;
  const int dense = s.cost_dense ? KF_DENSE : 0;
  int mode = c.mode;
  if (c.which == IK_STATIONARITY || c.which == IK_DUAL) mode = frm(ALTRO_HIP_FORM_ALROWS_LDS) ? 0 : STAT_NO_FEAS;   // constraint rows in the DPP form
  if (c.which == IK_EXPAND && frm(ALTRO_HIP_FORM_EXPAND_LDS) && !s.cost_dense) mode |= EXPAND_LDS;   // (the dense cost lives in the row-layout kernels only)
  // a device model: the dynamics expansion rides with every gradient expansion of a stored trajectory (not with the end-of-sweep
  // refresh, EXPAND_NEXT: the merit pass that made the candidate left Z already)
  if (model && c.which == IK_EXPAND && (mode & EXPAND_GRADIENT) && !(mode & EXPAND_NEXT)) mode |= EXPAND_DYN;
  if (c.which == IK_MERIT) mode = frm(ALTRO_HIP_FORM_MERIT_LDS) ? 0 : frm(ALTRO_HIP_FORM_MERIT_DPP_ALWAYS) ? 3 : 2;
  // the kind a step's arguments carry: a library kernel next to a caller's source sees MODEL_LINEAR (none of them steps the dynamics)
  const int lib_kind = user ? (int)MODEL_LINEAR : s.model;
  int rtc_kind = MODEL_USER;
  const auto add = [&](bool rtc, int id, int64_t gx, unsigned gy = 1, unsigned gz = 1, unsigned block = 64, unsigned lds = 0, int chunks = 0) {
    r.step[r.count++] = RouteStep{rtc, id, (unsigned)gx, gy, gz, block, lds, mode, rtc ? rtc_kind : lib_kind, chunks};
  };
  const auto no_kernel = [&] { r.error = ROUTE_NO_KERNEL; r.count = 0; return r; };
  // the kernels with KF_MODEL or KF_WIDE exist for fp64 records, the compiled-in ones for MODEL_QUADROTOR
  if (model && (!s.f64 || (!user && s.model != MODEL_QUADROTOR))) return no_kernel();
  if (wide && !s.f64 && (c.which == IK_EXPAND || c.which == IK_MERIT || c.which == IK_MERIT2)) return no_kernel();
  const int64_t knots = (int64_t)s.N + 1, rows4 = (s.batch + 3) / 4, flat = ((int64_t)s.batch * knots * 16 + 255) / 256;
  const unsigned waves = (unsigned)mf_grid(s.batch), pairs = (unsigned)mf_grid((s.batch + 1) / 2);
  const unsigned trials = (unsigned)std::max(c.spec_trials, 1);
  switch (c.which) {
    case IK_ROLLOUT:
      if (model) add(user, K_WAVE_ROLLOUT | KF_MODEL, rows4);
      else add(false, K_WAVE_ROLLOUT, waves);
      break;
    case IK_ACCEPT: add(false, K_WAVE_ACCEPT, std::min<int64_t>(flat, 1 << 20), 1, 1, 256); break;
    case IK_EXPAND:
      if (model && (mode & EXPAND_DYN)) add(user, K_WAVE_EXPAND_DYN | KF_MODEL, rows4 * s.N);
      if (user_al) {   // the whole AL expansion, the cost's terms included
        add(true, K_WAVE_EXPAND_DPP | dense | (wide ? KF_WIDE : 0), rows4 * knots);
        break;
      }
      if (al && (wide || dense || !(mode & EXPAND_LDS))) add(false, K_WAVE_EXPAND_DPP | (wide ? KF_WIDE : 0) | (dense ? dense : s.al.all_sel ? KF_ALLSEL : 0), rows4 * knots);
      else if (al) add(false, K_WAVE_EXPAND_LDS, s.batch * knots);
      else if (mode & EXPAND_GRADIENT) add(false, K_WAVE_EXPAND_GRAD | dense, std::min<int64_t>(flat, 262144), 1, 1, 256);
      break;
    case IK_DUAL:
      if (user_al) { add(true, K_WAVE_DUAL_DPP, rows4 * knots); break; }
      if (mode & STAT_NO_FEAS) add(false, K_WAVE_DUAL_DPP, rows4 * knots);
      else add(false, K_WAVE_DUAL_LDS, s.batch * knots);
      break;
    case IK_MERIT:
    case IK_MERIT2: {
      const bool dual = c.which == IK_MERIT2, aff = !dual && !model && s.f64 && c.aff && mode >= 2;
      const unsigned gy = dual ? 1u : (trials + 1) / 2;
      if (!model && !wide && !dual && !aff && !dense && mode != 2 && mode != 3) {   // ALTRO_HIP_FORM_MERIT_LDS keeps the LDS form
        add(false, K_WAVE_MERIT_LDS | (al ? KF_AL : 0), waves, trials);
        break;
      }
      // the DPP form: two problems per wave, two trials per problem.  (With constraint blocks and ONE trial per problem its second rows idle;
      // while the constraint Jacobians came from global memory the LDS form won those rounds on long horizons.  With G in LDS and the duals
      // fetched a step ahead the DPP form wins them too -- C1 + input bounds, cubic search, whole solves: N = 192: 69.7 vs 70.9 ms, N = 256: 105.2 vs 108.9.)
      const int id = merit_id(al, dual, s.cost_dense, model || !al || s.al.has_soc, aff, (model ? KF_MODEL : 0) | (wide ? KF_WIDE : 0));
      if (aff) {
        const int chunks = (s.N + MD_AFF_CHUNK - 1) / MD_AFF_CHUNK;
        add(false, id, pairs, gy, (unsigned)chunks, 64, route_merit_lds(s, false));
        add(false, K_WAVE_AFF_REDUCE | (wide ? KF_WIDE : 0), ((int64_t)ILQR_SPEC_TRIALS * s.batch + 255) / 256, 1, 1, 256, 0, chunks);
      } else {
        add(user, id, pairs, gy, 1, 64, route_merit_lds(s, user));
      }
      break;
    }
    case IK_SPEC_SELECT: add(false, K_WAVE_SPEC_SELECT, s.batch); break;
    case IK_STATIONARITY:
      // (STAT_FEAS_USER: no kernel reads the bit any more -- kept so that the arguments stay what they were, bit for bit)
      if (user_al) { mode |= STAT_FEAS_USER; rtc_kind = MODEL_LINEAR; }   // the residual from the library's kernel (it reads no constraint data), then the module's walk of the rows
      if (al && (mode & STAT_NO_FEAS)) {   // the residual here, the constraint rows four problems per wave
        add(false, K_WAVE_STATIONARITY, waves);
        add(user_al, K_WAVE_FEAS_DPP, rows4 * knots);
      } else {   // (the LDS form: the kernel walks the rows itself; with a slot from the source it is refused before the route is asked)
        mode &= ~STAT_NO_FEAS;
        add(false, K_WAVE_STATIONARITY, waves);
      }
      break;
    case IK_SHIFT: add(false, K_WAVE_SHIFT, ((int64_t)s.batch * 16 + 255) / 256, 1, 1, 256); break;
    default: return no_kernel();
  }
  return r;
}

// Plan LANE: every kernel steps or reads the handle's model (a compiled-in one from the library, the caller's source from the run-time
// module, all of them); MeritFunction in one launch or as rollout | per-knot-point terms on the whole chip | sums and phi'; the
// stationarity walk after its residuals are zeroed.
inline Route route_lane(const RouteShape& s, const RouteCall& c) {
  Route r;
  const bool user = s.model == MODEL_USER;
  if (!user && !lane_model_supported(s.model, s.n, s.m)) { r.error = ROUTE_NO_MODEL; return r; }
  const auto add = [&](int slot, bool dense, int64_t gx, unsigned gy, unsigned block) {
    r.step[r.count++] = RouteStep{user, lane_id(slot, dense), (unsigned)gx, gy, 1, block, 0, c.mode, s.model, 0};
  };
  const int64_t total = (int64_t)s.batch * (s.N + 1), lanes = (s.batch + 63) / 64;
  const int64_t flat = std::min<int64_t>((total + 255) / 256, 1 << 20), flat64 = std::min<int64_t>((total + 63) / 64, 1 << 20);
  const unsigned trials = (unsigned)std::max(c.spec_trials, 1);
  switch (c.which) {
    case IK_ROLLOUT: add(RTC_ROLLOUT, false, lanes, 1, 64); break;
    case IK_ACCEPT: add(RTC_ACCEPT, false, flat, 1, 256); break;
    case IK_EXPAND: add(RTC_EXPAND, s.cost_dense, flat64, 1, 64); break;
    case IK_MERIT:
      if (s.merit_split) {
        add(RTC_MERIT_ROLL, false, lanes, trials, 64);
        add(RTC_MERIT_POINT, s.cost_dense, flat64, trials, 64);
        add(RTC_MERIT_SUM, false, lanes, trials, 64);
      } else {
        add(RTC_MERIT, s.cost_dense, lanes, trials, 64);
      }
      break;
    case IK_SPEC_SELECT: add(RTC_SPEC_SELECT, false, flat, 1, 256); break;
    case IK_DUAL: add(RTC_DUAL, false, flat, 1, 256); break;
    case IK_SHIFT: add(RTC_SHIFT, false, std::min<int64_t>(((int64_t)s.batch * (s.n + s.m) + 255) / 256, 1 << 20), 1, 256); break;
    case IK_STATIONARITY:
      add(RTC_ZERO_RESIDUALS, false, (s.batch + 255) / 256, 1, 256);
      add(RTC_STATIONARITY, false, flat64, 1, 64);
      break;
    default: r.error = ROUTE_NO_KERNEL;
  }
  return r;
}

// the shapes plan MFMA32 takes (AUTO's rule: the (12, 4) tile of plan MFMA16 keeps n <= 12, m <= 4): the row layout's kernels exist for them
constexpr bool tile32_shape_ok(int n, int m) { return n >= 5 && n <= T32_MAX_N && m >= 1 && m <= T32_MAX_M && n + m <= 32 && !(n <= 12 && m <= 4); }
constexpr bool gen_model_supported(int kind, int n, int m) { return kind == MODEL_QUADROTOR13 && n == 13 && m == 4; }   // compiled-in models of plans GENERIC / MFMA32
// the loop kernels of kernels/ilqr_row32.hip serve the handle: plan MFMA32's shapes (also on a handle created as plan GENERIC), fp64, uniform
// dimensions, every constraint block in a row-wise cone with at most 32 rows; dynamics as data ...
inline bool row32_shape(const RouteShape& s) {
  return s.plan == ALTRO_HIP_PLAN_GENERIC && s.f64 && !s.ragged && tile32_shape_ok(s.n, s.m) && !(s.forms & ALTRO_HIP_FORM_GENERIC_MERIT_LDS) && (!s.al_enabled || s.al.row32_ok);
}
inline bool row32_eligible(const RouteShape& s) { return row32_shape(s) && s.model == MODEL_LINEAR; }
// ... or a device model: a compiled-in one (row32_model.hip), or the caller's source where its row-layout kernels are to be chosen
inline bool row32_model_eligible(const RouteShape& s) {
  return row32_shape(s) && s.model != MODEL_LINEAR && (gen_model_supported(s.model, s.n, s.m) || (s.model == MODEL_USER && s.row_ok));
}
// what the solve loop asks: is there a two-trial pass (IK_MERIT2: phi(0) and the first step in one pass), and a one-pass head of Solve
// (IK_ROLLOUT with ROLLOUT_INIT: rollout + CopyTrajectory + first expansion; unconstrained, dynamics as data; plan MFMA16: the diagonal cost)
inline bool route_two_trial(const RouteShape& s) {
  return (s.plan == ALTRO_HIP_PLAN_MFMA16 || row32_eligible(s) || row32_model_eligible(s)) && !(s.forms & (ALTRO_HIP_FORM_NO_SPECULATION | ALTRO_HIP_FORM_NO_MERIT2));
}
inline bool route_rollout_head(const RouteShape& s) {
  return !s.al_enabled && ((route_two_trial(s) && !s.cost_dense && s.model == MODEL_LINEAR) || row32_eligible(s));
}

// Plans GENERIC / MFMA32.  The cost expansion BEFORE the dynamics expansion.  A compiled-in model (MODEL_QUADROTOR13, fp64): rollout, merit and
// dynamics expansion are the model's kernels; the caller's source: those from the run-time module (the row-layout ones where row32_model_eligible),
// the cost expansion next to them sees MODEL_LINEAR, and with a block from the source every kernel that evaluates constraint rows comes from
// the module too (its merit kernel carries them).  MeritFunction of the data form: the row layout where it serves, else the wave-per-problem
// kernel with the knot point's matrices staged in LDS while sixteen waves still fit a CU (10 KB each, the kernel's own 2.5 KB included).
inline Route route_generic(const RouteShape& s, const RouteCall& c) {
  Route r;
  const bool al = s.al_enabled, user = s.model == MODEL_USER, q13 = s.f64 && gen_model_supported(s.model, s.n, s.m), user_al = user && al && s.al.has_user;
  const bool row32 = row32_eligible(s), row32m = row32_model_eligible(s);
  if (user && !s.f64) { r.error = ROUTE_NO_KERNEL; return r; }
  int mode = c.mode, kind = s.model;
  if (s.model != MODEL_LINEAR && c.which == IK_EXPAND && (mode & EXPAND_GRADIENT)) mode |= EXPAND_DYN;   // the dynamics expansion rides with every gradient expansion
  const auto add = [&](bool rtc, int id, int64_t gx, unsigned gy = 1, unsigned block = 64, unsigned lds = 0, int chunks = 0) {
    r.step[r.count++] = RouteStep{rtc, id, (unsigned)gx, gy, 1, block, lds, mode, kind, chunks};
  };
  const int64_t b = s.batch, knots = (int64_t)s.N + 1, pairs = (b + 1) / 2, flat = std::min<int64_t>((b * knots * (s.n + s.m) + 255) / 256, 1 << 20);
  const unsigned jv = al ? (unsigned)(GEN_AL_JV * sizeof(double)) : 0u;
  switch (c.which) {
    case IK_ROLLOUT:
      if (user || q13) add(user, K_GEN_ROLLOUT | KF_MODEL, (b + 63) / 64);
      else if (row32 && (mode & ROLLOUT_INIT)) add(false, K_ROW_INIT, pairs);
      else add(false, K_GEN_ROLLOUT, b);
      break;
    case IK_ACCEPT: add(false, K_GEN_ACCEPT, flat, 1, 256); break;
    case IK_EXPAND:
      if (user) kind = MODEL_LINEAR;   // (the model kind the cost's expansion sees is not one it steps)
      if (user_al) add(true, K_GEN_EXPAND_AL, b * knots);
      else if (al && row32 && (!(mode & EXPAND_HESSIAN) || (mode & EXPAND_DIAG)) && !(mode & EXPAND_DYN)) add(false, K_ROW_EXPAND, pairs, (unsigned)((s.N + R32_EXPAND_CHUNK - 1) / R32_EXPAND_CHUNK));
      else if (al) add(false, K_GEN_EXPAND_AL, b * knots);
      else add(false, K_GEN_EXPAND, flat, 1, 256);
      kind = s.model;
      if ((user || q13) && (mode & EXPAND_DYN)) {   // A_k, B_k at the candidate trajectory
        if (row32m) add(user, K_ROW_EXPAND_DYN | KF_MODEL, (b * s.N + 1) / 2);
        else add(user, K_GEN_EXPAND_DYN | KF_MODEL, (b * s.N + 63) / 64);
      }
      break;
    case IK_DUAL: add(user_al, K_GEN_DUAL, b * knots); break;
    case IK_MERIT:
      if (user || q13) {
        if (row32m) add(user, K_ROW_MERIT | KF_MODEL, pairs);
        else add(user, K_GEN_MERIT | KF_MODEL, b, 1, 64, jv);
      } else if (row32) {
        add(false, K_ROW_MERIT, pairs);
      } else {
        const size_t stage = generic_merit_stage_elems(s.n, s.m) * (s.f64 ? 8 : 4);
        if (2560 + jv + stage <= 10 * 1024) add(false, K_GEN_MERIT | KF_STAGED, b, 1, 64, jv + (unsigned)stage);
        else add(false, K_GEN_MERIT, b, 1, 64, jv);
      }
      break;
    case IK_MERIT2:   // the row layout's shapes only
      if (row32) add(false, K_ROW_MERIT | KF_DUAL, b);
      else if (row32m) add(user, K_ROW_MERIT | KF_DUAL | KF_MODEL, b);
      else r.error = ROUTE_NO_KERNEL;
      break;
    case IK_STATIONARITY:
      if (user_al) add(true, K_GEN_STATIONARITY, b);
      else if (row32 || row32m) {   // (it reads A_k, B_k wherever they came from)
        const int chunks = c.stat_part ? (s.N + R32_STAT_CHUNK - 1) / R32_STAT_CHUNK : 1;
        add(false, K_ROW_STAT, pairs, (unsigned)chunks);
        if (chunks > 1) add(false, K_ROW_STAT_REDUCE, (b + 255) / 256, 1, 256, 0, chunks);
      } else add(false, K_GEN_STATIONARITY, b);
      break;
    case IK_SHIFT: add(false, K_GEN_SHIFT, (b * (s.n + s.m) + 255) / 256, 1, 256); break;
    default: r.error = ROUTE_NO_KERNEL;
  }
  return r;
}

inline Route loop_route(const RouteShape& s, const RouteCall& c) {
  return s.plan == ALTRO_HIP_PLAN_GENERIC ? route_generic(s, c) : s.plan == ALTRO_HIP_PLAN_MFMA16 ? route_mfma16(s, c) : route_lane(s, c);
}

}  // namespace capi

// The launcher units: each maps a step's kernel id to its instantiation and launches it with the step's grid and dynamic LDS.
// 0 launched, 1 = the unit does not carry the id (an internal error), 2 = launch error
template <typename T> struct IlqrGenArgs;
template <typename S> int ilqr_wave_launch_kernel(hipStream_t stream, const capi::RouteStep& st, const IlqrWaveArgs<S>& a);   // ilqr_launch_mfma16.hip
template <typename S> int ilqr_wave_launch_model(hipStream_t stream, const capi::RouteStep& st, const IlqrWaveArgs<S>& a);    // ilqr_launch_mfma16_model.hip (a.mp.kind)
template <typename S> int ilqr_wave_launch_wide(hipStream_t stream, const capi::RouteStep& st, const IlqrWaveArgs<S>& a);     // ilqr_launch_mfma16_wide.hip
template <typename T> int ilqr_launch_kernel(hipStream_t stream, const capi::RouteStep& st, int kind, int n, int m, const IlqrArgs<T>& a);   // ilqr_launch_f64.hip, _f32.hip
template <typename T> int ilqr_generic_launch(hipStream_t stream, const capi::RouteStep& st, const IlqrGenArgs<T>& a);        // ilqr_launch_generic.hip
typedef int Row32Launch(hipStream_t stream, const capi::RouteStep& st, const IlqrGenArgs<double>& a);   // row32_unit.inc: eight units, the shapes by n mod 8
Row32Launch row32_merit_unit0, row32_merit_unit1, row32_merit_unit2, row32_merit_unit3, row32_merit_unit4, row32_merit_unit5, row32_merit_unit6, row32_merit_unit7;
int row32_model_launch(hipStream_t stream, const capi::RouteStep& st, const IlqrGenArgs<double>& a);   // row32_model.hip

}  // namespace altro_hip
