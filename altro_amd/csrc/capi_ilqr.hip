// capi_ilqr.hip -- C ABI: the batched AL-iLQR loop around the sweep (SolverImpl::Solve per problem), the device models' entry
// points, augmented-Lagrangian constraint blocks and the MPC receding-horizon operations.  The host sequences launches;
// every per-problem decision is taken on the device (kernels/ilqr_loop_kernels.hip).
#include "capi_internal.h"

#include <cmath>
#include <cstring>

using namespace altro_hip;
using namespace altro_hip::capi;

namespace altro_hip {
namespace capi {   // (external linkage: capi_solve.hip drives these)

// ---- iLQR loop (plan LANE) ---------------------------------------------------------------------------
// the handle's blocks as al_tables.h takes them
static AlInput al_input(const altro_hip_batch* h) {
  return AlInput{h->plan, h->n, h->m, h->N, h->batch, h->dtype == ALTRO_HIP_F64 ? sizeof(double) : sizeof(float), h->ragged, h->nxv, h->nuv,
                 h->al_defs, h->al_knots, h->al_G, h->al_g};
}
static int al_copy(altro_hip_batch* h, void** dst, const void* src, size_t bytes) {   // a host table's copy on the device
  if (const int rc = dmalloc(h, dst, bytes)) return rc;
  HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
static int al_copy_pool(altro_hip_batch* h, void** dst, const std::vector<double>& pool) {   // ... of a value pool, in the handle's element type
  if (h->dtype == ALTRO_HIP_F64) return al_copy(h, dst, pool.data(), pool.size() * sizeof(double));
  const std::vector<float> f = al_pool_as<float>(pool);
  return al_copy(h, dst, f.data(), f.size() * sizeof(float));
}
// the knot points block `id` is registered at (one contiguous range): k0 > k1 for an id that is on none
static void al_def_range(const altro_hip_batch* h, int id, int& k0, int& k1) {
  k0 = 0; k1 = -1;
  for (int k = 0; k <= h->N; ++k)
    for (int j = 0; j < h->al_knots[k].ncon; ++j)
      if (h->al_knots[k].def[j] == id) { if (k1 < 0) k0 = k; k1 = k; }
}
// The host description must not go stale: blocks whose right-hand sides the device changed without the host seeing the values
// (al_g_stale) are read back into al_g, from the pool as it stands and where the last upload put them (AlDef::g_off)
static int al_mirror_refresh(altro_hip_batch* h) {
  bool any = false;
  for (char c : h->al_g_stale) any = any || c;
  if (!any || !h->al_d_g) { h->al_g_stale.assign(h->al_defs.size(), 0); return 0; }
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int64_t B = h->batch;
  for (size_t i = 0; i < h->al_g_stale.size() && i < h->al_defs.size(); ++i) {
    if (!h->al_g_stale[i]) continue;
    const AlDef& d = h->al_defs[i];
    std::vector<double>& mirror = h->al_g[i];
    const int64_t nb = d.g_per_problem ? B : 1;
    const int K = (int)(mirror.size() / (size_t)(d.p * nb));
    auto fetch = [&](auto t) -> int {
      std::vector<decltype(t)> v(mirror.size());
      HIP_TRY(hipMemcpy(v.data(), (const decltype(t)*)h->al_d_g + d.g_off, v.size() * sizeof(t), hipMemcpyDeviceToHost));
      for (int64_t b = 0; b < nb; ++b)
        for (int kk = 0; kk < K; ++kk)
          for (int r = 0; r < d.p; ++r) mirror[((size_t)b * K + kk) * d.p + r] = v[(size_t)(al_g_index(d, B, b, d.k_first + kk, r) - d.g_off)];
      return 0;
    };
    if (const int rc = h->dtype == ALTRO_HIP_F64 ? fetch(double{}) : fetch(float{})) return rc;
  }
  h->al_g_stale.assign(h->al_defs.size(), 0);
  return 0;
}
// (re)build the device tables of the constraint blocks (al_tables.h decides what they contain); duals restart from zero when the
// structure changes
static int al_upload_tables(altro_hip_batch* h) {
  if (const int rc = al_mirror_refresh(h)) return rc;
  for (void** p : {(void**)&h->al_d_knots, (void**)&h->al_d_big, (void**)&h->al_d_gsel, (void**)&h->al_d_guser, &h->al_d_G, &h->al_d_Gpad, &h->al_d_g, &h->al_d_z,
                   (void**)&h->al_d_order, (void**)&h->al_d_start})
    dfree(h, p);
  h->al_sum = AlSummary{}; h->al_rows = 0; h->al_nchains = 0;   // (nothing on the device: what a handle without blocks has)
  const AlTables t = al_build(al_input(h));
  if (t.error == AL_BUILD_SLOTS)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "knot point %d: more constraint rows than the plan's table holds", t.err_k);
  if (t.error == AL_BUILD_WINDOW)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "plan LANE: %d dual rows x batch %d exceed the 2 GiB buffer window; split the batch", t.rows, h->batch);
  if (h->al_defs.empty()) return 0;
  int rc = 0;
  if (!t.gsel.empty() && (rc = al_copy(h, (void**)&h->al_d_gsel, t.gsel.data(), t.gsel.size() * sizeof(int)))) return rc;
  if (!t.guser.empty() && (rc = al_copy(h, (void**)&h->al_d_guser, t.guser.data(), t.guser.size() * sizeof(int)))) return rc;
  if (h->plan == ALTRO_HIP_PLAN_GENERIC && (rc = al_copy(h, (void**)&h->al_d_big, t.big.data(), t.big.size() * sizeof(AlKnotBig)))) return rc;
  if ((rc = dmalloc(h, (void**)&h->al_d_knots, std::max<size_t>(t.knots.size(), 1) * sizeof(AlKnot)))) return rc;   // (plan GENERIC: no entries)
  if (!t.knots.empty()) HIP_TRY(hipMemcpy(h->al_d_knots, t.knots.data(), t.knots.size() * sizeof(AlKnot), hipMemcpyHostToDevice));
  if ((rc = al_copy_pool(h, &h->al_d_G, t.G))) return rc;
  if ((rc = al_copy_pool(h, &h->al_d_g, t.g))) return rc;
  if (!t.Gpad.empty() && (rc = al_copy_pool(h, &h->al_d_Gpad, t.Gpad))) return rc;
  const size_t zbytes = (size_t)t.rows * h->batch * (h->dtype == ALTRO_HIP_F64 ? sizeof(double) : sizeof(float));
  if ((rc = dmalloc_zero(h, &h->al_d_z, zbytes))) return rc;
  // altro_hip_shift_duals' chains: the rows of one block definition at consecutive knot points, in walking order (al_shift.h)
  const AlShift sh = al_shift_build(t.big, h->al_defs, t.rows);
  if ((rc = al_copy(h, (void**)&h->al_d_order, sh.order.data(), sh.order.size() * sizeof(int)))) return rc;
  if ((rc = al_copy(h, (void**)&h->al_d_start, sh.start.data(), sh.start.size() * sizeof(int)))) return rc;
  h->al_nchains = (int)sh.heads.size();
  h->al_knots = t.big;
  h->al_defs = t.defs;   // (g_off: where each block's segment of the g pool starts)
  h->al_sum = t.sum; h->al_rows = t.rows;
  return 0;
}
int al_upload(altro_hip_batch* h) {
  if (!h->al_dirty) return 0;
  const int rc = al_upload_tables(h);
  if (!rc) h->al_dirty = false;
  return rc;
}

// The kernels' view of the handle's constraint tables, on every plan: what a plan does not have is null / zero on the handle (al_upload_tables:
// Gpad is plan MFMA16's; big, gsel and guser are plan GENERIC's), and max_ncon is plan MFMA16's (the route reads the summary's: loop_route.h).
template <typename T>
AlTable<T> al_table(const altro_hip_batch* h) {
  AlTable<T> t;
  t.knots = h->al_d_knots; t.big = h->al_d_big; t.G = (const T*)h->al_d_G; t.g = (const T*)h->al_d_g; t.z = (T*)h->al_d_z; t.enabled = h->al_defs.empty() ? 0 : 1;
  t.uniform = h->al_sum.uniform; t.rows_per_knot = h->al_sum.rows_per_knot; t.N = h->N; t.G_count = h->al_sum.G_count; t.Gpad = (const T*)h->al_d_Gpad; t.Gpad_count = h->al_sum.Gpad_count;
  t.all_sel = h->al_sum.all_sel; t.has_soc = h->al_sum.has_soc; t.gsel = h->al_d_gsel; t.max_ncon = h->al_sum.max_ncon; t.guser = h->al_d_guser;
  t.theta = (const T*)h->model.theta; t.theta_bs = h->batch;   // (altro_hip_set_model_params; null without)
  return t;
}

template <typename T>
IlqrArgs<T> ilqr_args(altro_hip_batch* h, const LoopCall& c) {
  IlqrArgs<T> a;
  a.al = al_table<T>(h);
  a.mode = EXPAND_GRADIENT | EXPAND_HESSIAN;
  a.in = (T*)h->l_in; a.term = (T*)h->l_term; a.out = (const T*)h->l_out; a.outn = (const T*)h->l_outn;
  a.nom = (T*)h->l_nom; a.cand = (T*)h->l_xuy; a.x0 = (const T*)h->l_x0;
  a.cost = (const T*)(h->cost_dense ? h->l_costq : h->l_cost); a.cost_kind = h->cost_dense ? 1 : 0;
  a.alpha = c.use_alpha ? h->i_alpha : nullptr;
  a.active = c.active;
  a.phi = h->i_phi; a.dphi = h->i_dphi; a.prob = h->i_prob;
  a.mp = h->model; a.N = h->N; a.batch = h->batch; a.want_derivative = c.want_deriv; a.alpha_const = c.alpha_const;
  a.cand_spec = (T*)h->i_cand_spec; a.spec_trials = h->i_cand_spec ? c.spec_trials : 1; a.spec_sel = h->i_spec_sel;
  a.spec_pre = h->i_cand_spec ? c.spec_pre : 0;
  a.spec_flip = 0;
  a.spec_stride = (int64_t)h->batch * (h->N + 1) * lane_sizes(h->n, h->m).e_xuy;
  a.ls_beta = c.ls_beta; a.ls_max_iters = c.ls_max_iters;
  a.merit_jk = h->merit_split == 1 ? (T*)h->i_merit_jk : nullptr;
  a.spec_jac = (T*)h->i_spec_jac;
  return a;
}
// Most line-search steps one merit launch of this handle can ever evaluate: the sequenced loop speculates 2 / 4 / 8 wide only
// while wavefronts x trials x 2 stays below what the chip holds (plan LANE: 512 wavefronts; the scattered searching lanes
// occupy every wave of the batch), the fused solve kernel never goes beyond 4.  The spare trajectories and the per-trial cost
// array are sized to THIS, not to ILQR_SPEC_TRIALS: at 65536 bicycles that is 3 spares instead of 7 (0.8 GB instead of 1.9).
int spec_trials_cap(const altro_hip_batch* h) {
  if (h->plan != ALTRO_HIP_PLAN_LANE) return ILQR_SPEC_TRIALS;   // MFMA16: the searching problems alone decide
  const int64_t units = (h->batch + 63) / 64;
  int t = ILQR_SPEC_TRIALS;
  while (t > 4 && units * t > 512) t /= 2;   // the solve loop widens while units * (2 * trials) <= 512: the widest launch is units * t
  return t;
}
// `count` spare candidate trajectories (grown on demand, never shrunk); false = no memory for them (nothing is changed)
bool ensure_spares(altro_hip_batch* h, int count, size_t bytes_each) {
  if (h->spare_count >= count) return true;
  if (h->spare_failed > 0 && count >= h->spare_failed) return false;   // this size did not fit before: do not ask again
  void* fresh = nullptr;
  if (dmalloc_quiet(h, &fresh, (size_t)count * bytes_each, true) != hipSuccess) { (void)hipGetLastError(); h->spare_failed = count; return false; }
  if (h->i_cand_spec) (void)hipStreamSynchronize(h->stream);
  dfree(h, &h->i_cand_spec);
  h->i_cand_spec = fresh;
  h->spare_count = count;
  return true;
}
// The buffers of the three-launch merit evaluation (first use).  No memory for them: the one-launch kernel, for good.
void merit_split_prepare(altro_hip_batch* h) {
  if (h->merit_split >= 0) return;
  h->merit_split = form(h, ALTRO_HIP_FORM_MERIT_ONE_LAUNCH) ? 0 : 1;
  if (!h->merit_split) return;
  const size_t jk = (size_t)spec_trials_cap(h) * (h->N + 1) * h->batch * h->esz;
  const size_t jac = ((size_t)h->N * (h->n * h->n + h->n * h->m + h->n + h->m) + h->n) * h->batch * h->esz;
  if (dmalloc(h, &h->i_merit_jk, jk) || dmalloc(h, &h->i_spec_jac, jac)) {
    (void)hipGetLastError();
    dfree(h, &h->i_merit_jk);
    h->merit_split = 0;
  }
}

// Affine line-search trials (kernels/ilqr_merit2_dpp.hip, AFF): who may take them, and their buffers -- one place for the solve
// (capi_solve.hip) and the step-wise entry (altro_hip_merit_affine).
// plan MFMA16's line-search rounds in the DPP form (a dense cost, a device model: row-layout kernels only)
bool merit_rounds_dpp(const altro_hip_batch* h) { return !form(h, ALTRO_HIP_FORM_MERIT_LDS) || h->cost_dense || h->model_set; }
// plan MFMA16, dynamics as data, fp64, the rounds in the DPP form; ALTRO_HIP_FORM_ROLLOUT_ROUNDS keeps every trial a rollout
bool affine_eligible(const altro_hip_batch* h) {
  return h->plan == ALTRO_HIP_PLAN_MFMA16 && h->dtype == ALTRO_HIP_F64 && !h->model_set && merit_rounds_dpp(h) &&
         !form(h, ALTRO_HIP_FORM_ROLLOUT_ROUNDS) && !h->aff_failed;
}
// The base trajectory with its sensitivity, the step it was taken at, the chunks' shares and the flags: true when the handle holds them.
bool affine_buffers(altro_hip_batch* h) {
  if (h->i_sens && h->i_sens_alpha && h->i_aff_part && h->i_aff_on) return true;
  // all four buffers or none: a partial allocation is released and remembered, so that no later solve of this handle
  // finds a null pointer behind a non-null one or retries a multi-gigabyte hipMalloc; the sensitivity buffer (192 B per knot point
  // and problem) is only taken while it stays below a quarter of what the handle already holds -- an optimisation must not be what
  // runs a large batch out of memory
  const size_t B = h->batch, chunks = (h->N + 15) / 16;
  const size_t sens_bytes = B * (h->N + 1) * 24 * sizeof(double);
  int rc = sens_bytes > h->ledger.counted_bytes() / 4 + (size_t(64) << 20) ? 1 : 0;
  if (!rc) rc = dmalloc(h, &h->i_sens, sens_bytes);
  if (!rc) rc = dmalloc(h, &h->i_sens_alpha, B * sizeof(double));
  if (!rc) rc = dmalloc(h, &h->i_aff_part, chunks * ILQR_SPEC_TRIALS * B * 2 * sizeof(double));
  if (!rc) rc = dmalloc_zero(h, &h->i_aff_on, (size_t)ILQR_SPEC_TRIALS * B * sizeof(int));
  if (rc) {   // an optimisation only: this handle's rounds stay rollouts
    for (void** q : {&h->i_sens, &h->i_sens_alpha, &h->i_aff_part, &h->i_aff_on}) dfree(h, q);
    h->aff_failed = true;
    (void)hipGetLastError();
  }
  return !rc;
}

// what the route of a loop operation may depend on (loop_route.h)
RouteShape route_shape(const altro_hip_batch* h) {
  return RouteShape{h->plan, h->dtype == ALTRO_HIP_F64, h->ragged, h->n, h->m, h->N, h->batch, h->model_set ? h->model.kind : (int)MODEL_LINEAR, h->cost_dense,
                    h->merit_split == 1, h->forms, !h->al_defs.empty(), h->al_sum, h->rtc_row32_ok};
}
// the library's launcher unit of a step (0 launched, 1 = the unit does not carry the id, 2 = launch error)
template <typename S>
static int launch_step(altro_hip_batch* h, const RouteStep& st, const IlqrWaveArgs<S>& a) {
  const int unit = route_unit(st.id);
  return unit == RU_MFMA16_WIDE ? ilqr_wave_launch_wide<S>(h->stream, st, a) : unit == RU_MFMA16_MODEL ? ilqr_wave_launch_model<S>(h->stream, st, a)
                                : ilqr_wave_launch_kernel<S>(h->stream, st, a);
}
template <typename T>
static int launch_step(altro_hip_batch* h, const RouteStep& st, const IlqrGenArgs<T>& a) {
  if constexpr (sizeof(T) == 8) {   // the row layout: fp64
    const int unit = route_unit(st.id);
    static Row32Launch* const row32_units[8] = {row32_merit_unit0, row32_merit_unit1, row32_merit_unit2, row32_merit_unit3,
                                                 row32_merit_unit4, row32_merit_unit5, row32_merit_unit6, row32_merit_unit7};
    if (unit != RU_GENERIC) return unit == RU_ROW32 ? row32_units[a.n & 7](h->stream, st, a) : row32_model_launch(h->stream, st, a);
  }
  return ilqr_generic_launch<T>(h->stream, st, a);
}
template <typename T>
static int launch_step(altro_hip_batch* h, const RouteStep& st, const IlqrArgs<T>& a) { return ilqr_launch_kernel<T>(h->stream, st, h->model.kind, h->n, h->m, a); }
// The steps of a route in order: each one's mode and model kind into the arguments, then its launch -- from the library, or (the caller's
// own model, compiled at run time: capi_rtc.hip) from the handle's module
template <typename A>
static int route_execute(altro_hip_batch* h, const RouteShape& shape, const Route& route, A a) {
  bool module_current = false;
  for (int i = 0; i < route.count; ++i) {
    const RouteStep& st = route.step[i];
    a.mode = st.mode; a.mp.kind = st.kind;
    if (st.rtc) {
      if (!module_current) {   // (once per operation: the module for the shape's cost kind / tables)
        if (const int rc = rtc_current(h, shape)) return rc;
        module_current = true;
      }
      if (const int rc = rtc_step(h, st, &a)) return rc;
      continue;
    }
    const int rc = launch_step(h, st, a);
    if (rc == 1) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "internal error: kernel %#x is not in its launcher unit", st.id);
    if (rc) return fail(ALTRO_HIP_ERR_HIP, "iLQR kernel launch failed");
  }
  return 0;
}
template <typename T>
int lane_run(altro_hip_batch* h, const LoopCall& c) {
  const IlqrArgs<T> a = ilqr_args<T>(h, c);
  const RouteShape shape = route_shape(h);
  const Route route = loop_route(shape, RouteCall{c.which, c.mode, a.spec_trials});
  if (route.error == ROUTE_NO_MODEL) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "no device model for (kind, n, m) = (%d, %d, %d)", h->model.kind, h->n, h->m);
  if (route.error) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "operation %d is not available on plan LANE", c.which);
  return route_execute(h, shape, route, a);
}
template <typename S>
int wave_run(altro_hip_batch* h, const LoopCall& c) {
  const int which = c.which, mode = c.mode;
  IlqrWaveArgs<S> a;
  a.al = al_table<S>(h);
  a.mode = mode;
  // a slot from the caller's source (altro_hip_add_user_constraint): evaluated by the row-layout kernels of the run-time module only
  const bool user_al = a.al.enabled && h->al_sum.has_user;
  if (user_al && (h->forms & (ALTRO_HIP_FORM_MERIT_LDS | ALTRO_HIP_FORM_ALROWS_LDS | ALTRO_HIP_FORM_EXPAND_LDS)))
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "constraint blocks from source on plan MFMA16 run in the row-layout kernels only: the LDS comparison forms "
                                           "(ALTRO_HIP_FORM_MERIT_LDS, _ALROWS_LDS, _EXPAND_LDS) do not evaluate them");
  a.penalty_scaling = c.penalty_scaling; a.penalty_max = c.penalty_max;
  a.costd = (const S*)h->m_costd; a.costd_term = (const S*)h->m_costd_term; a.cost_dense = h->cost_dense ? 1 : 0;
  if (h->model_set) a.mp = h->model;
  a.dyn = (const S*)h->m_in; a.dyn_bs = h->m_st.in_bs; a.dyn_ks = h->m_st.in_ks;
  a.cin = (S*)h->m_cin; a.cin_bs = h->m_st.cin_bs; a.cin_ks = h->m_st.cin_ks;
  a.term = (S*)h->m_term; a.out = (const S*)h->m_out; a.out_bs = h->m_st.out_bs; a.out_ks = h->m_st.out_ks;
  a.outn = (const S*)h->m_outn; a.nom = (S*)h->m_nom; a.cand = (S*)h->m_xuy; a.xuy_bs = h->m_st.xuy_bs;
  a.xuy_ks = h->m_st.xuy_ks; a.costp = (const S*)h->m_costp; a.x0 = (const S*)h->x0;
  a.alpha = c.use_alpha ? h->i_alpha : nullptr; a.active = c.active;
  a.phi = h->i_phi; a.dphi = h->i_dphi; a.prob = h->i_prob; a.N = h->N; a.batch = h->batch;
  a.want_derivative = c.want_deriv; a.alpha_const = c.alpha_const;
  a.cand_spec = (S*)h->i_cand_spec; a.spec_trials = h->i_cand_spec ? c.spec_trials : 1; a.spec_sel = h->i_spec_sel;
  a.spec_pre = h->i_cand_spec ? c.spec_pre : 0;
  a.spec_stride = (int64_t)h->batch * (h->N + 1) * MF_XUY;
  a.ls_beta = c.ls_beta; a.ls_max_iters = c.ls_max_iters;
  a.skip = which == IK_STATIONARITY ? c.stat_skip : nullptr;
  // affine line-search trials (the caller says which launches take part: LoopCall::aff): fp64 records, dynamics as data only
  const bool aff_on = sizeof(S) == 8 && c.aff != AFF_OFF && !h->model_set;
  const bool aff_store = aff_on && c.aff == AFF_STORE && (which == IK_MERIT2 || which == IK_MERIT);   // the sweep's phi(0) evaluation leaves base + sensitivity behind
  const RouteShape shape = route_shape(h);
  const Route route = loop_route(shape, RouteCall{which, mode, a.spec_trials, aff_on && !aff_store && which == IK_MERIT && c.aff == AFF_ROUND && !a.spec_pre});
  if (route.error) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "operation %d is not available on plan MFMA16", which);
  if constexpr (sizeof(S) == 8) {
    a.aff = route.count && (route.step[0].id & KF_AFF) ? 1 : 0;
    if (aff_store || a.aff) { a.sens = (double*)h->i_sens; a.sens_alpha = (double*)h->i_sens_alpha; }
    if (a.aff) { a.aff_part = (double*)h->i_aff_part; a.aff_on = (int*)h->i_aff_on; }   // (flags: zero when allocated, cleared again by the reduction)
  }
  return route_execute(h, shape, route, a);
}
// one problem's length of the dense arrays of plan GENERIC's iLQR loop (nominal trajectory, the cost's own blocks): the sum of the
// knot points' blocks, whatever their dimensions
struct GenSizes { int64_t sx, su, sQ, sR, sH; };
GenSizes gen_sizes(const altro_hip_batch* h) {
  GenSizes z{0, 0, 0, 0, 0};
  for (int k = 0; k <= h->N; ++k) {
    const int64_t nk = h->ragged ? h->nxv[k] : h->n, mk = k < h->N ? (h->ragged ? h->nuv[k] : h->m) : 0;
    z.sx += nk; z.su += mk; z.sQ += nk * nk; z.sR += mk * mk; z.sH += mk * nk;
  }
  return z;
}
// plan GENERIC: any (n_k, m_k) up to 64, dynamics as data, quadratic cost, linear constraint blocks (kernels/ilqr_generic.hip)
template <typename T>
int gen_run(altro_hip_batch* h, const LoopCall& c) {
  const int n = h->n, m = h->m, N = h->N, which = c.which, mode = c.mode;
  IlqrGenArgs<T> a;
  a.A = (const T*)h->g_arr[G_A]; a.A_bs = h->g_bstride[G_A]; a.B = (const T*)h->g_arr[G_B]; a.B_bs = h->g_bstride[G_B];
  a.f = (const T*)h->g_arr[G_f]; a.f_bs = h->g_bstride[G_f];
  a.Q = (T*)h->g_arr[G_Q]; a.Q_bs = h->g_bstride[G_Q]; a.R = (T*)h->g_arr[G_R]; a.R_bs = h->g_bstride[G_R];
  a.H = (T*)h->g_arr[G_H]; a.H_bs = h->g_bstride[G_H]; a.q = (T*)h->g_arr[G_q]; a.q_bs = h->g_bstride[G_q];
  a.r = (T*)h->g_arr[G_r]; a.r_bs = h->g_bstride[G_r];
  a.K = (const T*)h->g_arr[G_K]; a.K_bs = h->g_bstride[G_K]; a.d = (const T*)h->g_arr[G_d]; a.d_bs = h->g_bstride[G_d];
  a.P = (const T*)h->g_arr[G_P]; a.P_bs = h->g_bstride[G_P]; a.p = (const T*)h->g_arr[G_p]; a.p_bs = h->g_bstride[G_p];
  a.x = (T*)h->g_arr[G_x]; a.x_bs = h->g_bstride[G_x]; a.u = (T*)h->g_arr[G_u]; a.u_bs = h->g_bstride[G_u];
  a.y = (T*)h->g_arr[G_y]; a.y_bs = h->g_bstride[G_y];
  a.xn = (T*)h->g_xn; a.un = (T*)h->g_un;
  a.cQ = (const T*)h->g_cQ; a.cR = (const T*)h->g_cR; a.cH = (const T*)h->g_cH; a.cq = (const T*)h->g_cq; a.cr = (const T*)h->g_cr;
  a.cc = (const T*)h->g_cc;
  a.x0 = (const T*)h->x0; a.x0_stride = h->x0_stride;
  a.alpha = c.use_alpha ? h->i_alpha : nullptr; a.active = c.active; a.alpha_const = c.alpha_const;
  a.phi = h->i_phi; a.dphi = h->i_dphi; a.prob = h->i_prob;
  a.N = N; a.n = n; a.m = m; a.batch = h->batch; a.want_derivative = c.want_deriv; a.mode = mode;
  a.off = h->g_off; a.nx = h->g_nx; a.nu = h->g_nu;
  const GenSizes gs = gen_sizes(h);
  a.sx = gs.sx; a.su = gs.su; a.sQ = gs.sQ; a.sR = gs.sR; a.sH = gs.sH;
  a.al = al_table<T>(h);
  const RouteShape shape = route_shape(h);
  a.row32 = row32_eligible(shape) ? 1 : 0;   // (what the kernels read of the route: MeritFunction's layout)
  a.row32m = row32_model_eligible(shape) ? 1 : 0;
  if ((a.row32 || a.row32m) && which == IK_STATIONARITY && N > R32_STAT_CHUNK) {   // the stationarity walk in chunks of knot points: their maxima meet here
    const size_t need = (size_t)((N + R32_STAT_CHUNK - 1) / R32_STAT_CHUNK) * h->batch * 2 * sizeof(double);
    if (h->ledger.bytes_of(h->g_stat_part) < need) {   // (not counted: the handle's, but not part of altro_hip_batch_device_bytes)
      dfree(h, &h->g_stat_part);
      if (dmalloc_quiet(h, (void**)&h->g_stat_part, need, false) != hipSuccess) (void)hipGetLastError();   // (an optimisation only: one chunk then)
    }
    a.stat_part = h->g_stat_part;
  }
  if (h->model_set) a.mp = h->model;
  const Route route = loop_route(shape, RouteCall{which, mode, 1, false, a.stat_part != nullptr});
  if (route.error) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "operation %d is not available on plan GENERIC", which);
  return route_execute(h, shape, route, a);
}
int ilqr_run(altro_hip_batch* h, const LoopCall& c) {
  const int which = c.which;
  int rc = al_upload(h);
  if (rc) return rc;
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) return h->dtype == ALTRO_HIP_F64 ? gen_run<double>(h, c) : gen_run<float>(h, c);
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {   // linear dynamics: "expand" = cost gradient (+ AL Hessian terms when constrained)
    rc = h->dtype == ALTRO_HIP_F64 ? wave_run<double>(h, c) : wave_run<float>(h, c);
    // (altro_hip_batch::expansion_current) who writes the candidate trajectory, and who leaves its expansion behind
    if (which == IK_MERIT) h->expansion_current = !rc && c.want_deriv && !c.active && c.spec_trials == 1 && !c.spec_pre && h->al_defs.empty();
    else if (which == IK_ROLLOUT || which == IK_SHIFT || which == IK_SPEC_SELECT || which == IK_MERIT2 || which == IK_DUAL) h->expansion_current = false;
    return rc;
  }
  if (which == IK_MERIT) merit_split_prepare(h);
  return h->dtype == ALTRO_HIP_F64 ? lane_run<double>(h, c) : lane_run<float>(h, c);
}

struct CostUpload { int field; const double* src; int nk_host; };
// Cost fields of knot points 0 .. N from host arrays of nk_host knot points per problem -- N + 1 or N, with kz the {running, terminal}
// pair or the one running block: the running knot points of every field, then record N of those that have one (element N of a full
// array, or the second entry of the pair).  `dense`: the cost form being set (the handle's flag changes once all of it is in place).
int cost_fields_set(altro_hip_batch* h, bool dense, const CostUpload* up, int count, int kz, int bz) {
  LoopShape s = loop_shape(h);
  s.cost_dense = dense;
  const int N = h->N;
  int rc = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < count && !rc; ++i) {
      const FieldRef r0 = loop_field(s, up[i].field, 0), rN = loop_field(s, up[i].field, N);
      const bool zero_array = !up[i].src && r0.kind == LK_AOS;   // plan GENERIC (one array per field): src == NULL zeroes it
      if (pass == 0 && zero_array) HIP_TRY(hipMemsetAsync(loop_buffer(h, r0.buf), 0, (size_t)h->batch * r0.bs * h->esz, h->stream));
      else if (pass == 0) rc = field_set(h, s, up[i].field, 0, s.ragged && rN.buf != LB_NONE ? N + 1 : N, up[i].src, kz, bz, up[i].nk_host);
      else if (!zero_array && !s.ragged && rN.buf != LB_NONE) rc = field_set(h, s, up[i].field, N, 1, up[i].src, 1, bz, up[i].nk_host, (kz ? 1 : N) * rN.len);
    }
  return rc;
}
// plan GENERIC: the cost's own dense blocks (what the merit function and the expansion evaluate) next to the backward sweep's
// inputs, which altro_hip_set_cost fills; nominal trajectory allocated on first use.  Host arrays: Q [nb][nkx][n n], R [nb][nku][m m],
// H [nb][nku][m n], q [nb][nkx][n], r [nb][nku][m], c [nb][nkx] or NULL.
int generic_cost_def(altro_hip_batch* h, const double* Q, const double* R, const double* H, const double* q, const double* r,
                     const double* c, int kz, int bz) {
  const int N = h->N;
  const int nkx = kz ? 2 : N + 1, nku = kz ? 1 : N;
  const size_t B = h->batch, E = h->esz;
  const GenSizes gs = gen_sizes(h);
  int rc = 0;
  {   // every array has its own guard: a failed allocation in the middle leaves the later pointers null and the next call retries them
    // (one `if (!h->g_cQ)` around all eight skipped the retry and handed null arrays to the kernels)
    struct { void** p; size_t bytes; bool zero; } want[] = {
        {&h->g_cQ, B * gs.sQ * E, false}, {&h->g_cR, B * gs.sR * E, false}, {&h->g_cH, B * gs.sH * E, false},
        {&h->g_cq, B * gs.sx * E, false}, {&h->g_cr, B * gs.su * E, false}, {&h->g_cc, B * (N + 1) * E, false},
        {&h->g_xn, B * gs.sx * E, true},  {&h->g_un, B * gs.su * E, true}};
    for (auto& w : want) {
      if (*w.p) continue;
      if ((rc = w.zero ? dmalloc_zero(h, w.p, w.bytes) : dmalloc(h, w.p, w.bytes))) return rc;
    }
    // the candidate inputs (g_arr[G_u]) are NOT touched here: altro_hip_set_input_guess may come before the cost, like the reference's
    // SetInput may; they are zeroed once, when the handle is created
  }
  // (per-knot-point dimensions: the caller's packed [b][k][block_k] arrays are the device layout, one block per problem)
  if (h->ragged && kz) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "k_stride_zero needs uniform dimensions");
  const CostUpload up[] = {{LF_COST_Q, Q, nkx}, {LF_COST_R, R, nku}, {LF_COST_H, H, nku}, {LF_COST_q, q, nkx}, {LF_COST_r, r, nku}, {LF_COST_c, c, nkx}};
  return cost_fields_set(h, true, up, 6, kz, bz);
}
int generic_cost(altro_hip_batch* h, const double* Q, const double* R, const double* H, const double* q, const double* r,
                 const double* c, int kz, int bz) {
  int rc = altro_hip_set_cost(h, Q, R, H, q, r, 0, kz, bz);   // the backward sweep's blocks: lxx = Q, luu = R, lux = H (lx, lu refreshed by the loop)
  if (rc) return rc;
  rc = generic_cost_def(h, Q, R, H, q, r, c, kz, bz);
  if (!rc) { h->lqr_cost_set = true; h->ilqr_linear = true; h->cost_dense = true; h->spec_no_memory = true; /* one step per launch on this plan */ }
  return rc;
}
int ilqr_check(altro_hip_batch* h, bool need_guess) {
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {   // dynamics are data (altro_hip_set_dynamics) or a device model of the tile plan
    if (!h->dyn_set && !h->model_set)
      return fail(ALTRO_HIP_ERR_NOT_SET, "neither altro_hip_set_dynamics nor altro_hip_set_model has been called");
  } else if (h->plan == ALTRO_HIP_PLAN_GENERIC) {   // any (n, m) up to 64: dynamics as data, a quadratic cost
    if (h->n > 64 || h->m > 64)
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "the iLQR loop of plan GENERIC gives one lane to every state row and one to every input row: "
                                             "n, m <= 64 (got %d, %d); the TVLQR sweeps (altro_hip_backward / _forward_ltv / _sweep) take any size", h->n, h->m);
    if (!h->dyn_set) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_dynamics has not been called");
    if (h->ragged && h->is_diag)   // (a diagonal altro_hip_set_cost re-lays the sweep's Q / R offsets, which the loop's dense blocks share)
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "per-knot-point dimensions: the iLQR loop works on the dense blocks of altro_hip_set_quadratic_cost / "
                                              "_set_tracking_cost; a later altro_hip_set_cost(is_diag = 1) re-laid them -- set the loop's cost again");
  } else if (!h->model_set) {
    return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_model has not been called (plan LANE runs device models; for dynamics given as "
                                       "data -- altro_hip_set_dynamics -- create the handle with ALTRO_HIP_PLAN_MFMA16)");
  }
  if (!h->lqr_cost_set) return fail(ALTRO_HIP_ERR_NOT_SET, "neither altro_hip_set_tracking_cost nor altro_hip_set_quadratic_cost has been called");
  if (!h->x0_set) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_initial_state has not been called");
  if (need_guess && !h->guess_set) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_input_guess has not been called");
  // a source with per-problem parameters has no default for them (a mass of 0 divides): nothing steps the model before the setter
  if (h->model_set && h->model.kind == MODEL_USER && h->model_np > 0 && !h->model.theta)
    return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_model_params has not been called: the handle's source takes %d per-problem parameters", h->model_np);
  return 0;
}

// A device model on plan GENERIC or MFMA16: A_k, B_k (plan MFMA16: the DYN records, Z = [A B]) are the EXPANSION's from now on, written
// by the expansion / merit kernels, and f = 0.  (memsets on the handle's own stream: see dmalloc_zero)
int model_takes_dynamics(altro_hip_batch* h) {
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) for (int a : {G_f, G_A, G_B}) HIP_TRY(hipMemsetAsync(h->g_arr[a], 0, (size_t)h->batch * h->g_bstride[a] * h->esz, h->stream));
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) HIP_TRY(hipMemsetAsync(h->m_in, 0, (size_t)h->batch * h->N * MF_DYN * h->esz, h->stream));
  h->dyn_set = true; h->has_f = 0;
  return 0;
}

template IlqrArgs<double> ilqr_args<double>(altro_hip_batch*, const LoopCall&);
template IlqrArgs<float> ilqr_args<float>(altro_hip_batch*, const LoopCall&);
}  // namespace capi
}  // namespace altro_hip

extern "C" {

// ---- iLQR loop entry points -----------------------------------------------------------------------------
int altro_hip_set_model(altro_hip_batch* h, int model, float timestep, int bicycle_frame,
                        double bicycle_length, double bicycle_lr) {
  int rc = loop_entry(h);
  if (rc) return rc;
  h->expansion_current = false;
  if (!(timestep > 0.0f)) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "time step must be positive (ErrorCodes::TimestepNotPositive)");
  // plan AUTO put a small shape on the padded tile (cheaper sweeps below ~6000 problems, capi_core.hip); a compiled-in model that only
  // plan LANE carries moves the still-empty handle there
  if (h->plan == ALTRO_HIP_PLAN_MFMA16 && !ilqr_tile_model_supported(model, h->n, h->m) && ilqr_supported(model, h->n, h->m) &&
      lane_supported(h->n, h->m)) {
    if ((rc = replan_empty_handle(h, ALTRO_HIP_PLAN_LANE))) return rc;
  }
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) {   // plans GENERIC / MFMA32: the model steps inside that plan's loop kernels (kernels/ilqr_generic.hip)
    if (h->ragged) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "device models need uniform dimensions");
    if (!ilqr_generic_model_supported(model, h->n, h->m))
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "no device model %d for plan %d with (n, m) = (%d, %d): plans GENERIC / MFMA32 carry "
                                             "ALTRO_HIP_MODEL_QUADROTOR13 at (13, 4)", model, altro_hip_batch_plan(h), h->n, h->m);
    if (h->dtype != ALTRO_HIP_F64) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "device models on plans GENERIC / MFMA32 run on fp64 handles");
    h->model = ModelParams{model, timestep, 0, 2.7, 1.5};
    model_params_drop(h);
    h->model_set = true;
    return model_takes_dynamics(h);
  }
  const bool tile = h->plan == ALTRO_HIP_PLAN_MFMA16 && ilqr_tile_model_supported(model, h->n, h->m);   // kernels/ilqr_tile_model.hip
  if (tile && h->dtype != ALTRO_HIP_F64)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "device models on plan MFMA16 run on fp64 records (create the handle with ALTRO_HIP_F64)");
  if (!tile && (h->plan != ALTRO_HIP_PLAN_LANE || !ilqr_supported(model, h->n, h->m)))
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "no device model %d for plan %d with (n, m) = (%d, %d)", model, h->plan, h->n, h->m);
  h->model = ModelParams{model, timestep, bicycle_frame, bicycle_length > 0 ? bicycle_length : 2.7,
                         bicycle_lr > 0 ? bicycle_lr : 1.5};
  model_params_drop(h);
  h->model_set = true;
  return tile ? model_takes_dynamics(h) : 0;
}

// ALTROSolver::SetTimeStep per knot-point range (altro_solver.hpp:55) for device models: one float[N] on the device, which every kernel
// that steps the model at knot point k reads (models.h: ModelParams::hk, model_at)
int altro_hip_set_time_steps(altro_hip_batch* h, const float* dt) {
  int rc = loop_entry(h);   // (per-knot-point dimensions: ALTRO_HIP_ERR_UNSUPPORTED, as for altro_hip_set_model)
  if (rc) return rc;
  if (!h->model_set)
    return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_time_steps needs a device model (altro_hip_set_model / altro_hip_set_model_source): dynamics "
                                       "given as data carry their own discretisation");
  if (!dt) {   // back to the uniform step
    h->expansion_current = false;
    h->model.hk = nullptr;
    return 0;
  }
  for (int k = 0; k < h->N; ++k)
    if (!(std::isfinite(dt[k]) && dt[k] > 0.0f))
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "dt[%d] = %g: every time step must be finite and positive (ErrorCodes::TimestepNotPositive)", k, (double)dt[k]);
  if (!h->d_hk && (rc = dmalloc(h, (void**)&h->d_hk, (size_t)h->N * sizeof(float)))) return rc;
  std::vector<float> host(dt, dt + h->N);
  // (on the handle's own stream: launches already enqueued read the old steps, later ones the new)
  HIP_TRY(hipMemcpyAsync(h->d_hk, host.data(), (size_t)h->N * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->hk_host.swap(host);
  h->model.hk = h->d_hk;
  h->expansion_current = false;
  return 0;
}
int altro_hip_get_time_steps(altro_hip_batch* h, float* dt) {
  int rc = loop_entry(h);
  if (rc) return rc;
  if (!dt) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "dt == NULL");
  if (!h->model_set) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_get_time_steps needs a device model (altro_hip_set_model / altro_hip_set_model_source)");
  for (int k = 0; k < h->N; ++k) dt[k] = h->model.hk ? h->hk_host[k] : h->model.h;
  return 0;
}

int altro_hip_set_tracking_cost(altro_hip_batch* h, const double* Qd, const double* Rd, const double* xref,
                                const double* uref, int kz, int bz) {
  // ALTROSolver::SetLQRCost (altro_solver.cpp:138-172): q = -Q xref, r = -R uref,
  // c = 1/2 xref'Q xref (+ 1/2 uref'R uref for k < N) -> KnotPointData::SetDiagonalCost
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (h->plan != ALTRO_HIP_PLAN_LANE && h->plan != ALTRO_HIP_PLAN_MFMA16 && h->plan != ALTRO_HIP_PLAN_GENERIC)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "unknown plan");
  if (!Qd || !Rd || !xref || !uref) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "Qd, Rd, xref, uref are required");
  if (h->dev_ptrs)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "altro_hip_set_tracking_cost forms q = -Q xref on the host: pass host arrays "
                                           "(altro_hip_set_pointer_mode(h, 0))");
  if (h->ragged) {   // per-knot-point dimensions: Qd, xref [b][sum nx], Rd, uref [b][sum nu] -> the dense blocks the loop of plan GENERIC evaluates
    if (kz) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "k_stride_zero needs uniform dimensions");
    const int N = h->N, nb = bz ? 1 : h->batch;
    const GenSizes gs = gen_sizes(h);
    std::vector<double> Q((size_t)nb * gs.sQ, 0.0), R((size_t)nb * gs.sR, 0.0), H((size_t)nb * gs.sH, 0.0), q((size_t)nb * gs.sx),
        r((size_t)nb * gs.su), c((size_t)nb * (N + 1));
    for (int b = 0; b < nb; ++b) {
      int64_t ox = 0, ou = 0, oQ = 0, oR = 0;
      for (int k = 0; k <= N; ++k) {
        const int nk = h->nxv[k], mk = k < N ? h->nuv[k] : 0;
        const double *Q_ = Qd + (size_t)b * gs.sx + ox, *x_ = xref + (size_t)b * gs.sx + ox;
        double cc = 0.0;
        for (int i = 0; i < nk; ++i) {
          Q[(size_t)b * gs.sQ + oQ + i + (size_t)i * nk] = Q_[i];
          q[(size_t)b * gs.sx + ox + i] = -(Q_[i] * x_[i]);
          cc += x_[i] * Q_[i] * x_[i];
        }
        cc *= 0.5;
        if (k < N) {
          const double *R_ = Rd + (size_t)b * gs.su + ou, *u_ = uref + (size_t)b * gs.su + ou;
          double cu = 0.0;
          for (int i = 0; i < mk; ++i) {
            R[(size_t)b * gs.sR + oR + i + (size_t)i * mk] = R_[i];
            r[(size_t)b * gs.su + ou + i] = -(R_[i] * u_[i]);
            cu += u_[i] * R_[i] * u_[i];
          }
          cc += 0.5 * cu;
        }
        c[(size_t)b * (N + 1) + k] = cc;
        ox += nk; ou += mk; oQ += (int64_t)nk * nk; oR += (int64_t)mk * mk;
      }
    }
    return generic_cost(h, Q.data(), R.data(), H.data(), q.data(), r.data(), c.data(), 0, bz);
  }
  const int n = h->n, m = h->m, N = h->N;
  const int nb = bz ? 1 : h->batch, nkx = kz ? 2 : N + 1, nku = kz ? 1 : N;
  // host-side arithmetic exactly as the reference's setter does it, then one upload per field
  std::vector<double> q((size_t)nb * nkx * n), r((size_t)nb * nku * m), c((size_t)nb * nkx);
  for (int b = 0; b < nb; ++b)
    for (int k = 0; k < nkx; ++k) {
      const double* Q_ = Qd + ((size_t)b * nkx + k) * n;
      const double* x_ = xref + ((size_t)b * nkx + k) * n;
      double cc = 0.0;
      for (int i = 0; i < n; ++i) { q[((size_t)b * nkx + k) * n + i] = -(Q_[i] * x_[i]); cc += x_[i] * Q_[i] * x_[i]; }
      cc *= 0.5;
      const bool terminal = kz ? (k == 1) : (k == N);
      if (!terminal) {
        const int ku = kz ? 0 : k;
        const double* R_ = Rd + ((size_t)b * nku + ku) * m;
        const double* u_ = uref + ((size_t)b * nku + ku) * m;
        double cu = 0.0;
        for (int i = 0; i < m; ++i) cu += u_[i] * R_[i] * u_[i];
        cc += 0.5 * cu;
      }
      c[(size_t)b * nkx + k] = cc;
    }
  for (int b = 0; b < nb; ++b)
    for (int k = 0; k < nku; ++k)
      for (int i = 0; i < m; ++i)
        r[((size_t)b * nku + k) * m + i] = -(Rd[((size_t)b * nku + k) * m + i] * uref[((size_t)b * nku + k) * m + i]);
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) {   // the diagonal cost as dense blocks (H = 0): what kernels/ilqr_generic.hip evaluates
    std::vector<double> Qf((size_t)nb * nkx * n * n, 0.0), Rf((size_t)nb * nku * m * m, 0.0), Hf((size_t)nb * nku * m * n, 0.0);
    for (size_t t = 0; t < (size_t)nb * nkx; ++t)
      for (int i = 0; i < n; ++i) Qf[t * n * n + i + (size_t)n * i] = Qd[t * n + i];
    for (size_t t = 0; t < (size_t)nb * nku; ++t)
      for (int i = 0; i < m; ++i) Rf[t * m * m + i + (size_t)m * i] = Rd[t * m + i];
    return generic_cost(h, Qf.data(), Rf.data(), Hf.data(), q.data(), r.data(), c.data(), kz, bz);
  }
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {
    // (a) the backward sweep's blocks: lxx = diag(Qd), luu = diag(Rd), lux = 0; lx, lu are refreshed by the loop
    rc = altro_hip_set_cost(h, Qd, Rd, nullptr, q.data(), r.data(), 1, kz, bz);
    if (rc) return rc;
    // (b) the cost parameters the merit function needs: COSTP records [k][b][36] = Qd | Rd | q | r | c
    const int64_t B = h->batch;
    if (!h->m_costp) {
      if ((rc = dmalloc_zero(h, &h->m_costp, (size_t)B * (N + 1) * MF_COSTP * h->esz))) return rc;
      if ((rc = dmalloc_zero(h, &h->m_nom, (size_t)B * (N + 1) * MF_NOM * h->esz))) return rc;
    }
  }
  // plans MFMA16 and LANE: the diagonal cost's record Qd | Rd | q | r | c of every knot point (record N: Qd, q, c)
  const CostUpload up[] = {{LF_COST_Qd, Qd, nkx}, {LF_COST_Rd, Rd, nku}, {LF_COST_q, q.data(), nkx}, {LF_COST_r, r.data(), nku}, {LF_COST_c, c.data(), nkx}};
  rc = cost_fields_set(h, false, up, 5, kz, bz);
  if (!rc && h->plan == ALTRO_HIP_PLAN_MFMA16 && m < MF_M) {   // padded inputs: Rd = 1 keeps their diagonal of Quu positive (they stay at exactly 0: K, d rows are 0)
    const double ones[MF_M] = {1.0, 1.0, 1.0, 1.0};
    LoopShape s = loop_shape(h);
    s.cost_dense = false;
    FieldRef pad = loop_field(s, LF_COST_Rd, 0);
    pad.off += m; pad.len = MF_M - m;
    rc = ref_set(h, pad, 0, N, ones, 1, 1, 1, 0);
  }
  if (rc) return rc;
  h->lqr_cost_set = true; h->cost_dense = false;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) h->ilqr_linear = true;
  else { h->cost_set = true; h->dyn_set = true; h->is_diag = 0; h->has_f = 0; }
  return rc;
}

int altro_hip_set_quadratic_cost(altro_hip_batch* h, const double* Q, const double* R, const double* H, const double* q,
                                 const double* r, const double* c, int kz, int bz) {
  // ALTROSolver::SetQuadraticCost (altro_solver.cpp:118-136) -> KnotPointData::SetQuadraticCost (knotpoint_data.cpp:64-85) for the
  // device iLQR loop: the cost 1/2 x'Qx + 1/2 u'Ru + u'Hx + q'x + r'u + c per knot point, stored dense and evaluated as
  // CalcOriginalCost / Gradient / Hessian do (knotpoint_data.cpp:624-634, :659-668, :691-698).
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (!Q || !R || !H || !q || !r) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "Q, R, H, q, r are required (c may be NULL: zero)");
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) return generic_cost(h, Q, R, H, q, r, c, kz, bz);   // (per-knot-point dimensions: packed arrays)
  const int n = h->n, m = h->m, N = h->N;
  const int nkx = kz ? 2 : N + 1, nku = kz ? 1 : N;
  const size_t Ez = h->esz;
  const int64_t B = h->batch;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {
    // (a) the backward sweep's blocks: lxx = Q, luu = R, lux = H; lx, lu are refreshed by the loop
    rc = altro_hip_set_cost(h, Q, R, H, q, r, 0, kz, bz);
    if (rc) return rc;
    // (b) the cost's own record, in the COST / TERM layout, for the merit function and the expansion
    if (!h->m_costd) {
      if ((rc = dmalloc_zero(h, &h->m_costd, (size_t)B * (N + 1) * MF_COST * Ez))) return rc;
      if ((rc = dmalloc_zero(h, &h->m_costd_term, (size_t)B * MF_TERM * Ez))) return rc;
    }
    if (!h->m_nom && (rc = dmalloc_zero(h, &h->m_nom, (size_t)B * (N + 1) * MF_NOM * Ez))) return rc;
    {
      Dims d{n, m};
      DevSrc dQ, dR, dH, dq, dr;
      rc = put_src(h, Q, d.Q(0), nkx, kz, bz, &dQ);
      if (!rc) rc = put_src(h, R, d.R(0), nku, kz, bz, &dR);
      if (!rc) rc = put_src(h, H, d.H(), nku, kz, bz, &dH);
      if (!rc) rc = put_src(h, q, n, nkx, kz, bz, &dq);
      if (!rc) rc = put_src(h, r, m, nku, kz, bz, &dr);
      SrcArr none{nullptr, 0, 0, 0};
      SrcArr tQ = dQ.s, tq = dq.s;   // terminal views: knot point N, or block 1 of the {running, terminal} pair
      if (kz) { tQ.p += d.Q(0); tq.p += n; }
      if (!rc) rc = mfma16_pack_launch(h, MSEG_Q, dQ.s, none, h->m_costd, h->m_costd_term, 0);
      if (!rc) rc = mfma16_pack_launch(h, MSEG_TERM_Q, tQ, none, h->m_costd, h->m_costd_term, 0);
      if (!rc) rc = mfma16_pack_launch(h, MSEG_HR, dH.s, dR.s, h->m_costd, h->m_costd_term, 0);
      if (!rc) rc = mfma16_pack_launch(h, MSEG_QR, dq.s, dr.s, h->m_costd, h->m_costd_term, 0);
      if (!rc) rc = mfma16_pack_launch(h, MSEG_TERM_q, tq, none, h->m_costd, h->m_costd_term, 0);
      if (!rc) HIP_TRY(hipStreamSynchronize(h->stream));   // (the sources are freed on leaving this block)
    }
    if (!rc && c) {   // c_k into the record's spare slot, k = 0 .. N (record N holds nothing else)
      const CostUpload up[] = {{LF_COST_c, c, nkx}};
      rc = cost_fields_set(h, true, up, 1, kz, bz);
    } else if (!rc) {   // c == NULL: zero (a handle that carried another cost before)
      const double zero = 0.0;
      struct HostPtrs { altro_hip_batch* h; bool keep; ~HostPtrs() { h->dev_ptrs = keep; } } host_ptrs{h, h->dev_ptrs};
      h->dev_ptrs = false;   // (`zero` lives on the host whatever the caller's pointer mode)
      LoopShape s = loop_shape(h);
      s.cost_dense = true;
      rc = field_set(h, s, LF_COST_c, 0, N + 1, &zero, 1, 1, 1, 0);
    }
    if (!rc) { h->lqr_cost_set = true; h->ilqr_linear = true; h->cost_dense = true; }
    return rc;
  }
  // plan LANE: [k][Q n n | R m m | H m n | q n | r m | c][batch], column-major blocks as given (IlqrDims<n, m, 1>)
  LoopShape s = loop_shape(h);
  s.cost_dense = true;
  const int E = loop_field(s, LF_COST_c, 0).E;
  if ((uint64_t)B * (uint64_t)E * Ez >= (1ull << 31))
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "plan LANE: batch %d too large for one handle (dense cost rows exceed 2 GiB)", h->batch);
  if (!h->l_costq && (rc = dmalloc_zero(h, &h->l_costq, (size_t)B * (N + 1) * E * Ez))) return rc;
  const CostUpload up[] = {{LF_COST_Q, Q, nkx}, {LF_COST_R, R, nku}, {LF_COST_H, H, nku}, {LF_COST_q, q, nkx}, {LF_COST_r, r, nku}, {LF_COST_c, c, nkx}};   // (c == NULL: zeros)
  rc = cost_fields_set(h, true, up, 6, kz, bz);
  if (!rc) { h->lqr_cost_set = true; h->cost_set = true; h->dyn_set = true; h->is_diag = 0; h->has_f = 0; h->cost_dense = true; }
  return rc;
}

int altro_hip_set_input_guess(altro_hip_batch* h, const double* u, int kz, int bz) {
  // ALTROSolver::SetInput (altro_solver.cpp:242-251): writes the CANDIDATE inputs u_
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (!u) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "u == NULL");
  if (h->ragged && kz) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "k_stride_zero needs uniform dimensions");   // (one packed block per problem)
  rc = field_set(h, loop_shape(h), LF_CAND_U, 0, h->N, u, kz, bz);
  if (!rc) h->guess_set = true;
  return rc;
}

int altro_hip_set_state_guess(altro_hip_batch* h, const double* x, int kz, int bz) {
  // ALTROSolver::SetState (altro_solver.cpp:229-240): writes the CANDIDATE states x_
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (!x) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "x == NULL");
  if (h->ragged && kz) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "k_stride_zero needs uniform dimensions");   // (one packed block per problem)
  return field_set(h, loop_shape(h), LF_CAND_X, 0, h->N + 1, x, kz, bz);
}

int altro_hip_open_loop_rollout(altro_hip_batch* h) {
  int rc = ilqr_check(h, true);
  if (!rc) rc = ilqr_run(h, {IK_ROLLOUT});
  if (!rc) h->forward_done = true;
  return rc;
}
int altro_hip_accept(altro_hip_batch* h) {
  int rc = ilqr_check(h, false);
  if (h) h->aff_base = false;   // (a new nominal trajectory)
  if (!rc) rc = ilqr_run(h, {IK_ACCEPT});
  return rc;
}
int altro_hip_expand(altro_hip_batch* h) {
  int rc = ilqr_check(h, false);
  if (rc) return rc;
  // CalcExpansions (solver.cpp:189-201) right after a merit evaluation with derivative of an unconstrained problem: the pass left
  // lx, lu (A, B for a device model) of this very candidate, and the cost's Hessian blocks are the constants the setter stored
  // (knotpoint_data.cpp:691-705 copies them afresh each sweep) -- nothing to launch
  if (h->plan == ALTRO_HIP_PLAN_MFMA16 && h->expansion_current && h->al_defs.empty()) return 0;
  return ilqr_run(h, {IK_EXPAND});
}
int altro_hip_merit(altro_hip_batch* h, const double* alpha, int alpha_is_uniform, int want_derivative,
                    double* phi, double* dphi) {
  int rc = ilqr_check(h, false);
  if (rc) return rc;
  if (!h->backward_done) return fail(ALTRO_HIP_ERR_NOT_SET, "backward must precede merit");
  if (!alpha || !phi) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "alpha and phi are required");
  if (!alpha_is_uniform)
    HIP_TRY(hipMemcpyAsync(h->i_alpha, alpha, (size_t)h->batch * 8, hipMemcpyHostToDevice, h->stream));
  LoopCall c{IK_MERIT};
  c.want_deriv = want_derivative; c.use_alpha = !alpha_is_uniform; c.alpha_const = alpha[0];
  rc = ilqr_run(h, c);
  if (rc) return rc;
  h->forward_done = true;
  HIP_TRY(hipMemcpyAsync(phi, h->i_phi, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
  if (want_derivative && dphi)
    HIP_TRY(hipMemcpyAsync(dphi, h->i_dphi, (size_t)h->batch * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}
// One affine line-search round on its own (kernels/ilqr_merit2_dpp.hip, AFF): what a solve's search_rounds launches, for the caller's
// steps.  The first call after a backward sweep runs the sweep's phi(0) evaluation first -- first_evaluation's launch without the
// speculative first step -- which leaves x_k(0) and s_k = dx_k / dalpha behind; later calls reuse that base (altro_hip_batch::aff_base).
int altro_hip_merit_affine(altro_hip_batch* h, const double* alpha, const int* active, int trials, double* phi, double* dphi) {
  int rc = ilqr_check(h, false);
  if (rc) return rc;
  if (!h->backward_done) return fail(ALTRO_HIP_ERR_NOT_SET, "backward must precede merit_affine");
  if (!alpha || !phi) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "alpha and phi are required");
  if (trials != 1 && trials != 2) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "trials must be 1 or 2 (got %d)", trials);
  if (!affine_eligible(h))
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "affine line-search trials need plan MFMA16, fp64 records, dynamics given as data (no device model), the "
                                           "DPP merit form and no ALTRO_HIP_FORM_ROLLOUT_ROUNDS%s", h->aff_failed ? "; this handle could not allocate their buffers" : "");
  if (!affine_buffers(h)) return fail(ALTRO_HIP_ERR_OUT_OF_MEMORY, "no memory for the base trajectory and its sensitivity");
  const size_t B = h->batch;
  if (trials > 1 && !ensure_spares(h, trials - 1, B * (h->N + 1) * MF_XUY * h->esz))
    return fail(ALTRO_HIP_ERR_OUT_OF_MEMORY, "no memory for the second trial's candidate trajectory");
  LoopCall c{IK_MERIT};   // (the default search's beta_decrease / max_iters)
  c.want_deriv = 1;
  if (!h->aff_base) {
    c.aff = AFF_STORE;
    if ((rc = ilqr_run(h, c))) return rc;
    h->aff_base = true;
  }
  HIP_TRY(hipMemcpyAsync(h->i_alpha, alpha, B * 8, hipMemcpyHostToDevice, h->stream));
  if (active) {   // the kernels store nothing for a problem that is masked out: what the caller passed in phi / dphi comes back for those
    HIP_TRY(hipMemcpyAsync(h->i_active, active, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->i_phi, phi, (size_t)trials * B * 8, hipMemcpyHostToDevice, h->stream));
    if (dphi) HIP_TRY(hipMemcpyAsync(h->i_dphi, dphi, B * 8, hipMemcpyHostToDevice, h->stream));
  }
  // trial 1 is the next step of the backtracking sequence, alpha beta, which the kernel takes for a problem whose search is in that
  // stage (IlqrProb::ls): every problem is put there for this launch, and back afterwards
  const size_t pitch = sizeof(IlqrProb);
  char* const stage_p = (char*)h->i_prob + offsetof(IlqrProb, ls) + offsetof(LsState, stage);
  char* const iter_p = (char*)h->i_prob + offsetof(IlqrProb, ls) + offsetof(LsState, bt_iter);
  std::vector<int> was(2 * B), now(2 * B, 0);
  if (trials > 1) {
    for (size_t b = 0; b < B; ++b) now[b] = LS_STAGE_BACKTRACK;
    HIP_TRY(hipMemcpy2DAsync(was.data(), sizeof(int), stage_p, pitch, sizeof(int), B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpy2DAsync(was.data() + B, sizeof(int), iter_p, pitch, sizeof(int), B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpy2DAsync(stage_p, pitch, now.data(), sizeof(int), sizeof(int), B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpy2DAsync(iter_p, pitch, now.data() + B, sizeof(int), sizeof(int), B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // (`was` is read below)
  }
  c.aff = AFF_ROUND; c.use_alpha = true; c.active = active ? h->i_active : nullptr; c.spec_trials = trials;
  rc = ilqr_run(h, c);
  if (trials > 1) {
    HIP_TRY(hipMemcpy2DAsync(stage_p, pitch, was.data(), sizeof(int), sizeof(int), B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpy2DAsync(iter_p, pitch, was.data() + B, sizeof(int), sizeof(int), B, hipMemcpyHostToDevice, h->stream));
  }
  if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
  h->forward_done = true;
  HIP_TRY(hipMemcpyAsync(phi, h->i_phi, (size_t)trials * B * 8, hipMemcpyDeviceToHost, h->stream));
  if (dphi) HIP_TRY(hipMemcpyAsync(dphi, h->i_dphi, B * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}
int altro_hip_stationarity(altro_hip_batch* h, double* out) {
  int rc = ilqr_check(h, false);
  if (rc) return rc;
  rc = ilqr_run(h, {IK_STATIONARITY});
  if (rc) return rc;
  std::vector<IlqrProb> pr(h->batch);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(pr.data(), h->i_prob, pr.size() * sizeof(IlqrProb), hipMemcpyDeviceToHost));
  for (int b = 0; b < h->batch; ++b) out[b] = pr[b].stationarity;
  return 0;
}
int altro_hip_feasibility(altro_hip_batch* h, double* out) {
  // SolverImpl::Feasibility (solver.cpp:224-231) of the candidate trajectory
  int rc = ilqr_check(h, false);
  if (rc) return rc;
  if (!out) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "out == NULL");
  rc = ilqr_run(h, {IK_STATIONARITY});
  if (rc) return rc;
  std::vector<IlqrProb> pr(h->batch);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(pr.data(), h->i_prob, pr.size() * sizeof(IlqrProb), hipMemcpyDeviceToHost));
  for (int b = 0; b < h->batch; ++b) out[b] = pr[b].feasibility;
  return 0;
}

// ---- MPC receding-horizon operations on the resident batch -----------------
int altro_hip_shift_trajectory(altro_hip_batch* h) {
  int rc = ilqr_check(h, true);
  if (!rc && h->ragged)   // (the reference's ShiftTrajectory copies knot point k + 1 into k: meaningful between equal dimensions only)
    rc = fail(ALTRO_HIP_ERR_UNSUPPORTED, "altro_hip_shift_trajectory needs uniform dimensions");
  if (!rc) rc = ilqr_run(h, {IK_SHIFT});
  if (!rc) h->aff_base = false;
  return rc;
}
int altro_hip_update_linear_costs(altro_hip_batch* h, const double* q, const double* r, const double* c,
                                  int k_first, int k_last, int kz, int bz) {
  // ALTROSolver::UpdateLinearCosts (altro_solver.cpp:266-281) -> KnotPointData::UpdateLinearCosts
  // (knotpoint_data.cpp:193-226) for knot points k_first..k_last (inclusive) of every problem
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (!h->lqr_cost_set) return fail(ALTRO_HIP_ERR_NOT_SET, "no quadratic cost to update (ErrorCodes::CostNotQuadratic)");
  const int N = h->N;
  if (k_first < 0 || k_last > N || k_first > k_last)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point range [%d, %d] outside [0, %d] (ErrorCodes::BadIndex)", k_first, k_last, N);
  if (r && k_last == N)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "cannot update linear input costs at the terminal knot point "
                                            "(ErrorCodes::InvalidOptAtTerminalKnotPoint)");
  const int nk = k_last - k_first + 1;
  // per-knot-point dimensions: q [b][sum over the range of nx[k]], r likewise, c [b][nk]
  if (h->ragged && kz) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "k_stride_zero needs uniform dimensions");
  const LoopShape s = loop_shape(h);
  const struct { int field; const double* src; } up[] = {{LF_COST_q, q}, {LF_COST_r, r}, {LF_COST_c, c}};
  for (const auto& f : up) {
    if (!f.src) continue;
    for (int k = k_first; k <= k_last && !rc;) {   // (a run ends where the field changes buffer: q_N of the tile plan's dense cost)
      const int run = loop_field_run(s, f.field, k, k_last);
      rc = field_set(h, s, f.field, k, run, f.src, kz, bz, kz ? 1 : nk, kz ? 0 : (k - k_first) * loop_field(s, f.field, k).len);
      k += run;
    }
  }
  return rc;
}
int altro_hip_get_knot(altro_hip_batch* h, int k, double* x, double* u) {
  // ALTROSolver::GetState / GetInput (altro_solver.cpp:323-347) of one knot point for the whole batch:
  // x [batch][n], u [batch][m] (u must be NULL at k = N); per-knot-point dimensions: [batch][nx[k]], [batch][nu[k]]
  int rc = loop_entry(h, true);
  if (rc) return rc;
  const int N = h->N;
  if (k < 0 || k > N) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point %d outside [0, %d] (ErrorCodes::BadIndex)", k, N);
  if (u && k == N) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "no input at the terminal knot point");
  if (h->plan == ALTRO_HIP_PLAN_MFMA16 && !h->m_nom) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_tracking_cost has not been called");
  if (h->plan == ALTRO_HIP_PLAN_GENERIC && !h->g_xn) return fail(ALTRO_HIP_ERR_NOT_SET, "no cost has been set for the iLQR loop");
  const LoopShape s = loop_shape(h);
  if (x && (rc = field_get(h, s, LF_NOM_X, k, 1, x))) return rc;
  if (u) rc = field_get(h, s, LF_NOM_U, k, 1, u);
  return rc;
}

// One more block on the handle's host tables: altro_hip_add_linear_constraint (user = 0), or altro_hip_add_user_constraint with
// user = id + 1 and placeholders for G and g (AlDef::user)
static int add_block(altro_hip_batch* h, int k_first, int k_last, int cone, int p, const double* G, const double* g, int g_per_problem, int user,
                     int g_per_knot = 0) {
  // ALTROSolver::SetConstraint (altro_solver.cpp:175-215) for c(x,u) = G [x;u] - g
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (!G || !g) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "G and g are required");
  // capacities (stated in altro_hip.h; al_tables.h: al_admit)
  const bool gen = h->plan == ALTRO_HIP_PLAN_GENERIC;
  const AlAdmit ad = al_admit(al_input(h), k_first, k_last, cone, p, user);
  switch (ad.limit) {
    case AL_LIMIT_CONE: return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "unknown cone %d", cone);
    case AL_LIMIT_ROWS:
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "constraint dimension %d outside [1, %d]%s", p, ad.pmax,
                  gen ? "" : cone == CONE_SOC ? " on this plan (ALTRO_HIP_PLAN_GENERIC takes second-order cones of up to 32 rows)"
                                              : " on this plan (ALTRO_HIP_PLAN_GENERIC takes up to 64 rows per block and 8 blocks per knot point)");
    case AL_LIMIT_RANGE:
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point range [%d, %d] outside [0, %d] (ErrorCodes::BadIndex)", k_first, k_last, h->N);
    case AL_LIMIT_DEFS:
      if (h->plan != ALTRO_HIP_PLAN_MFMA16) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "at most %d constraint blocks", ad.dmax);
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "at most %d constraint slots (blocks, counted in units of %d rows) per handle on this plan: "
                                             "ALTRO_HIP_PLAN_GENERIC takes 64 blocks", ad.dmax, AL_MAXP);
    case AL_LIMIT_KNOT:
      if (h->plan != ALTRO_HIP_PLAN_MFMA16)
        return fail(ALTRO_HIP_ERR_UNSUPPORTED, "at most %d constraint blocks per knot point on this plan (k = %d)%s", ad.cmax, ad.k,
                    gen ? "" : ": ALTRO_HIP_PLAN_GENERIC takes 8");
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "at most %d constraint slots of %d rows per knot point on this plan (k = %d would need %d; a block "
                                             "takes ceil(p / %d) of them, a second-order cone one): ALTRO_HIP_PLAN_GENERIC takes 8 blocks of 64 rows",
                  ad.cmax, AL_MAXP, ad.k, ad.count, AL_MAXP);
    case AL_LIMIT_RAGGED:
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot points %d and %d differ in dimension: one constraint block takes one [x; u] size "
                                              "(register it per range, like ALTROSolver::SetConstraint per index)", k_first, ad.k);
    default: break;   // (the limits of a block from source: altro_hip_add_user_constraint has answered them)
  }
  const int w = ad.w;
  AlDef d{cone, p, g_per_problem ? 1 : 0, (int)h->al_G.size(), 0, user, w, g_per_knot ? 1 : 0, g_per_knot ? k_first : 0};
  h->al_G.insert(h->al_G.end(), G, G + (size_t)p * w);
  h->al_g.emplace_back(g, g + (size_t)p * (g_per_problem ? h->batch : 1) * (g_per_knot ? k_last - k_first + 1 : 1));   // [nb][nk][p]
  h->al_g_stale.resize(h->al_g.size(), 0);
  const int id = (int)h->al_defs.size();
  h->al_defs.push_back(d);
  for (int k = k_first; k <= k_last; ++k) {
    AlKnotBig& kn = h->al_knots[k];
    kn.def[kn.ncon++] = id;
  }
  h->al_dirty = true;
  return id;
}
int altro_hip_add_linear_constraint(altro_hip_batch* h, int k_first, int k_last, int cone, int p, const double* G,
                                    const double* g, int g_per_problem) {
  return add_block(h, k_first, k_last, cone, p, G, g, g_per_problem, 0);
}
int altro_hip_add_linear_constraint_rhs(altro_hip_batch* h, int k_first, int k_last, int cone, int p, const double* G, const double* g,
                                        int rhs_layout) {
  if (rhs_layout & ~(ALTRO_HIP_RHS_PER_PROBLEM | ALTRO_HIP_RHS_PER_KNOT))
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "unknown right-hand side layout %d (ALTRO_HIP_RHS_PER_PROBLEM = 1, ALTRO_HIP_RHS_PER_KNOT = 2)", rhs_layout);
  return add_block(h, k_first, k_last, cone, p, G, g, rhs_layout & ALTRO_HIP_RHS_PER_PROBLEM, 0, rhs_layout & ALTRO_HIP_RHS_PER_KNOT);
}
int altro_hip_add_user_constraint(altro_hip_batch* h, int k_first, int k_last, int cone, int p, int id) {
  // ALTROSolver::SetConstraint with a general callback pair (altro_solver.cpp:192-223): value and Jacobian of block `id` come
  // from the source given to altro_hip_set_model_source (altro_user_constraint / altro_user_constraint_jacobian)
  int rc = loop_entry(h);
  if (rc) return rc;
  const bool gen = h->plan == ALTRO_HIP_PLAN_GENERIC;
  // (plan MFMA16: rtc_has_constraints is only ever set on a handle created with ALTRO_HIP_TILE_USER_BLOCKS, fp64 -- capi_rtc.hip)
  const bool tile = h->plan == ALTRO_HIP_PLAN_MFMA16;
  if ((h->plan != ALTRO_HIP_PLAN_LANE && !gen && !tile) || h->model.kind != MODEL_USER || !h->rtc_has_constraints)
    return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_model_source must come first, with a source that defines "
                                       "altro_user_constraint and altro_user_constraint_jacobian (plans LANE and GENERIC / MFMA32)");
  if (id < 0) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "constraint id %d", id);
  // one slot per block and AL_TILE_USER_MAXC such slots per knot point on plan MFMA16, GEN_USER_MAXROWS rows per block and per knot
  // point on plan GENERIC (al_tables.h: al_admit); every other limit: add_block
  const AlAdmit ad = al_admit(al_input(h), k_first, k_last, cone, p, id + 1);
  if (ad.limit == AL_LIMIT_USER_CONE) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "unknown cone %d", cone);
  if (ad.limit == AL_LIMIT_USER_ROWS && tile)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "a constraint block from source has 1 .. %d rows on plan MFMA16 (%s: one slot; got %d): "
                                           "ALTRO_HIP_PLAN_GENERIC takes 32", ad.pmax, cone == CONE_SOC ? "AL_MAXSOC" : "AL_MAXP", p);
  if (ad.limit == AL_LIMIT_USER_ROWS)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "a constraint block from source has 1 .. %d rows on plan GENERIC (GEN_USER_MAXROWS; got %d)", ad.pmax, p);
  if (ad.limit == AL_LIMIT_USER_KNOT && tile)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "at most %d constraint blocks from source per knot point on plan MFMA16 (AL_TILE_USER_MAXC; k = %d "
                                           "would have %d): ALTRO_HIP_PLAN_GENERIC takes 32 rows of them", ad.cmax, ad.k, ad.count);
  if (ad.limit == AL_LIMIT_USER_KNOT)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "at most %d rows of constraint blocks from source per knot point on plan GENERIC "
                                           "(GEN_USER_MAXROWS; k = %d would have %d)", ad.cmax, ad.k, ad.count);
  std::vector<double> G((size_t)std::max(p, 0) * (h->n + h->m), 0.0), g((size_t)std::max(p, 0), 0.0);   // placeholders: never read
  return add_block(h, k_first, k_last, cone, p, G.data(), g.data(), 0, id + 1);
}
int altro_hip_clear_constraints(altro_hip_batch* h) {
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  h->al_defs.clear(); h->al_G.clear(); h->al_g.clear(); h->al_g_stale.clear();
  h->al_knots.assign((size_t)h->N + 1, AlKnotBig{});
  h->al_dirty = true;
  return al_upload(h);
}
int altro_hip_reset_duals(altro_hip_batch* h, double penalty) {
  // duals back to zero and every constraint's penalty to `penalty` (what a fresh Initialize leaves: 1)
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if (!(penalty > 0.0)) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "penalty must be positive");
  if ((rc = al_upload(h))) return rc;
  const size_t E = h->dtype == ALTRO_HIP_F64 ? 8 : 4;
  if (h->al_d_z) HIP_TRY(hipMemsetAsync(h->al_d_z, 0, (size_t)h->al_rows * h->batch * E, h->stream));
  std::vector<IlqrProb> pr(h->batch);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(pr.data(), h->i_prob, pr.size() * sizeof(IlqrProb), hipMemcpyDeviceToHost));
  for (auto& q : pr) { q.rho = penalty; q.rho_est = penalty; }
  HIP_TRY(hipMemcpy(h->i_prob, pr.data(), pr.size() * sizeof(IlqrProb), hipMemcpyHostToDevice));
  return 0;
}
int altro_hip_get_duals(altro_hip_batch* h, int k, int slot, double* z) {
  // duals of constraint block `slot` of knot point k, [batch][p]
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if ((rc = al_upload(h))) return rc;
  if (k < 0 || k > h->N || slot < 0 || slot >= h->al_knots[k].ncon || !z)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "no constraint block %d at knot point %d", slot, k);
  const AlKnotBig& kn = h->al_knots[k];
  const int p = h->al_defs[kn.def[slot]].p;
  const int64_t B = h->batch;
  HIP_TRY(hipStreamSynchronize(h->stream));
  auto fetch = [&](auto t) -> int {   // device [p][batch] of the handle's element type -> z [batch][p]
    std::vector<decltype(t)> v((size_t)p * B);
    HIP_TRY(hipMemcpy(v.data(), (const decltype(t)*)h->al_d_z + (size_t)kn.z_off[slot] * B, v.size() * sizeof(t), hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < B; ++b)
      for (int r = 0; r < p; ++r) z[(size_t)b * p + r] = v[(size_t)r * B + b];
    return 0;
  };
  return h->dtype == ALTRO_HIP_F64 ? fetch(double{}) : fetch(float{});
}
int altro_hip_set_duals(altro_hip_batch* h, int k, int slot, const double* z) {
  // the inverse of altro_hip_get_duals: z [batch][p] into block `slot` of knot point k, in the handle's element type, as given (no
  // projection onto the dual cone: the reference's SetDual* declarations, altro_solver.hpp:357-362, name none)
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if ((rc = al_upload(h))) return rc;
  if (k < 0 || k > h->N || slot < 0 || slot >= h->al_knots[k].ncon || !z)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "no constraint block %d at knot point %d", slot, k);
  const AlKnotBig& kn = h->al_knots[k];
  const int p = h->al_defs[kn.def[slot]].p;
  const int64_t B = h->batch;
  HIP_TRY(hipStreamSynchronize(h->stream));
  auto store = [&](auto t) -> int {   // z [batch][p] -> device [p][batch] of the handle's element type
    std::vector<decltype(t)> v((size_t)p * B);
    for (int64_t b = 0; b < B; ++b)
      for (int r = 0; r < p; ++r) v[(size_t)r * B + b] = (decltype(t))z[(size_t)b * p + r];
    HIP_TRY(hipMemcpy((decltype(t)*)h->al_d_z + (size_t)kn.z_off[slot] * B, v.data(), v.size() * sizeof(t), hipMemcpyHostToDevice));
    return 0;
  };
  return h->dtype == ALTRO_HIP_F64 ? store(double{}) : store(float{});
}
int altro_hip_get_penalty(altro_hip_batch* h, double* rho) {
  // the constraints' penalty of every problem (IlqrProb::rho; KnotPointData::rho_, one value for all blocks of a problem), [batch]
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if ((rc = al_upload(h))) return rc;
  if (!rho) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "rho is required");
  const size_t bytes = (size_t)h->batch * sizeof(double);
  if ((rc = ensure_stage(h, bytes))) return rc;
  if (al_get_penalty_launch(h->stream, h->i_prob, (double*)h->stage, h->batch)) return fail(ALTRO_HIP_ERR_HIP, "penalty kernel launch failed");
  HIP_TRY(hipMemcpyAsync(rho, h->stage, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}
int altro_hip_set_penalty(altro_hip_batch* h, const double* rho, int batch_stride_zero) {
  // every problem's penalty to rho[b] (batch_stride_zero: to rho[0]), rho_est with it as altro_hip_reset_duals does; duals stay
  int rc = loop_entry(h, true);
  if (rc) return rc;
  h->expansion_current = false;
  if ((rc = al_upload(h))) return rc;
  if (!rho) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "rho is required");
  const int count = batch_stride_zero ? 1 : h->batch;
  for (int b = 0; b < count; ++b)
    if (!(rho[b] > 0.0)) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "penalty must be positive (problem %d)", b);
  const size_t bytes = (size_t)count * sizeof(double);
  if ((rc = ensure_stage(h, bytes))) return rc;
  HIP_TRY(hipMemcpyAsync(h->stage, rho, bytes, hipMemcpyHostToDevice, h->stream));
  if (al_set_penalty_launch(h->stream, h->i_prob, (const double*)h->stage, batch_stride_zero ? 0 : 1, h->batch))
    return fail(ALTRO_HIP_ERR_HIP, "penalty kernel launch failed");
  HIP_TRY(hipStreamSynchronize(h->stream));   // (the caller's array and the staging buffer are free again on return)
  return 0;
}
int altro_hip_shift_duals(altro_hip_batch* h, int tail) {
  // the duals' side of altro_hip_shift_trajectory: every block definition's duals move one knot point forward (kernels/al_shift.hip)
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if (h->ragged)   // (like the trajectory's shift: knot point k + 1 into k is meaningful between equal dimensions only)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "altro_hip_shift_duals needs uniform dimensions");
  h->expansion_current = false;
  if ((rc = al_upload(h))) return rc;
  if (tail != ALTRO_HIP_DUAL_TAIL_KEEP && tail != ALTRO_HIP_DUAL_TAIL_ZERO)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "unknown tail %d (ALTRO_HIP_DUAL_TAIL_KEEP = 0, ALTRO_HIP_DUAL_TAIL_ZERO = 1)", tail);
  if (h->al_defs.empty()) return 0;
  if (al_shift_duals_launch(h->stream, h->al_d_z, h->dtype == ALTRO_HIP_F64 ? 8 : 4, h->al_d_order, h->al_d_start, h->al_nchains, h->batch, tail))
    return fail(ALTRO_HIP_ERR_HIP, "dual shift kernel launch failed");
  return 0;
}
int altro_hip_set_constraint_rhs(altro_hip_batch* h, int id, int k_first, int k_last, const double* g) {
  // new right-hand sides for block `id`, in place (kernels/al_rhs.hip): the tables are not rebuilt, duals and penalty stay
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if ((rc = al_upload(h))) return rc;
  h->expansion_current = false; h->aff_base = false;
  if (id < 0 || id >= (int)h->al_defs.size()) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "no constraint block with id %d", id);
  const AlDef& d = h->al_defs[id];
  if (d.user) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "constraint block %d comes from source: it has no right-hand side g", id);
  int r0, r1;
  al_def_range(h, id, r0, r1);
  int kf = r0, kl = r0;
  if (!d.g_per_knot) {
    if (k_first != -1 || k_last != -1)
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "constraint block %d has one right-hand side for its whole range [%d, %d] (registered without "
                                              "ALTRO_HIP_RHS_PER_KNOT): it takes k_first = k_last = -1, not [%d, %d]", id, r0, r1, k_first, k_last);
  } else if (k_first == -1 && k_last == -1) {
    kl = r1;
  } else {
    if (k_first < r0 || k_last > r1 || k_first > k_last)
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point range [%d, %d] outside the range [%d, %d] of constraint block %d", k_first, k_last, r0, r1, id);
    kf = k_first; kl = k_last;
  }
  if (!g) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "g is required");
  const int64_t B = h->batch, nb = d.g_per_problem ? B : 1;
  const int nk = kl - kf + 1, C = nk * d.p;
  const size_t count = (size_t)nb * C;
  const double* src = g;
  if (!h->dev_ptrs) {
    const bool f32 = h->dtype != ALTRO_HIP_F64;
    for (size_t i = 0; i < count; ++i)
      if (!(f32 ? std::isfinite((float)g[i]) : std::isfinite(g[i])))
        return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "g[%zu] = %g is not finite%s", i, g[i], f32 ? " as a float" : "");
    if ((rc = ensure_stage(h, count * sizeof(double)))) return rc;
    HIP_TRY(hipMemcpyAsync(h->stage, g, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
    src = (const double*)h->stage;
    // the host description follows: [nb][K][p], K knot points from r0 on
    std::vector<double>& mirror = h->al_g[id];
    const int K = d.g_per_knot ? r1 - r0 + 1 : 1;
    for (int64_t b = 0; b < nb; ++b)
      std::copy(g + (size_t)b * C, g + (size_t)(b + 1) * C, mirror.begin() + ((size_t)b * K + (kf - r0)) * d.p);
  } else {
    h->al_g_stale[id] = 1;
  }
  const size_t E = h->dtype == ALTRO_HIP_F64 ? 8 : 4;
  // (the scatter writes rows of `batch` consecutive problems, knot points and rows ascending from its base: al_g_index's layout)
  if (al_rhs_scatter_launch(h->stream, (char*)h->al_d_g + (size_t)al_g_index(d, B, 0, kf, 0) * E, (int)E, src, C, (int)nb, h->batch, 0))
    return fail(ALTRO_HIP_ERR_HIP, "right-hand side kernel launch failed");
  HIP_TRY(hipStreamSynchronize(h->stream));   // (the caller's array and the staging buffer are free again on return)
  return 0;
}
int altro_hip_get_constraint_rhs(altro_hip_batch* h, int id, int k, double* g) {
  // what the device holds as block `id`'s right-hand side at knot point k, [nb][p]
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if ((rc = al_upload(h))) return rc;
  if (id < 0 || id >= (int)h->al_defs.size()) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "no constraint block with id %d", id);
  const AlDef& d = h->al_defs[id];
  if (d.user) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "constraint block %d comes from source: it has no right-hand side g", id);
  int r0, r1;
  al_def_range(h, id, r0, r1);
  if (k < r0 || k > r1) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "knot point %d outside the range [%d, %d] of constraint block %d", k, r0, r1, id);
  if (!g) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "g is required");
  const int64_t B = h->batch, nb = d.g_per_problem ? B : 1;
  HIP_TRY(hipStreamSynchronize(h->stream));
  auto fetch = [&](auto t) -> int {   // knot point k's run of the segment, [p] or [p][batch] in the handle's element type -> g [nb][p]
    std::vector<decltype(t)> v((size_t)d.p * nb);
    const int64_t at = al_g_index(d, B, 0, k, 0);
    HIP_TRY(hipMemcpy(v.data(), (const decltype(t)*)h->al_d_g + at, v.size() * sizeof(t), hipMemcpyDeviceToHost));
    for (int64_t b = 0; b < nb; ++b)
      for (int r = 0; r < d.p; ++r) g[(size_t)b * d.p + r] = v[(size_t)(al_g_index(d, B, b, k, r) - at)];
    return 0;
  };
  return h->dtype == ALTRO_HIP_F64 ? fetch(double{}) : fetch(float{});
}
int altro_hip_shift_constraint_rhs(altro_hip_batch* h) {
  // the right-hand sides' part of altro_hip_shift_trajectory: every ALTRO_HIP_RHS_PER_KNOT block's g moves one knot point forward
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if (h->ragged) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "altro_hip_shift_constraint_rhs needs uniform dimensions");
  h->expansion_current = false; h->aff_base = false;
  if ((rc = al_upload(h))) return rc;
  const size_t E = h->dtype == ALTRO_HIP_F64 ? 8 : 4;
  for (size_t i = 0; i < h->al_defs.size(); ++i) {
    const AlDef& d = h->al_defs[i];
    if (!d.g_per_knot) continue;
    int r0, r1;
    al_def_range(h, (int)i, r0, r1);
    if (r1 <= r0) continue;
    // the segment's first element and the distance between two knot points' runs, as al_g_index has them
    const int64_t first = al_g_index(d, h->batch, 0, r0, 0), stride = al_g_index(d, h->batch, 0, r0 + 1, 0) - first;
    if (al_rhs_shift_launch(h->stream, (char*)h->al_d_g + (size_t)first * E, (int)E, r1 - r0 + 1, stride))
      return fail(ALTRO_HIP_ERR_HIP, "right-hand side shift kernel launch failed");
    h->al_g_stale[i] = 1;
  }
  return 0;
}

// per-problem results gathered on the device into the struct's own layout: 56 bytes per problem cross PCIe, through pinned memory
}  // extern "C"
int altro_hip::capi::ilqr_gather_results(altro_hip_batch* h, altro_hip_solve_result* results) {
  static_assert(sizeof(IlqrResult) == sizeof(altro_hip_solve_result), "IlqrResult mirrors altro_hip_solve_result");
  static_assert(sizeof(IlqrPollRec) == sizeof(altro_hip_poll_record), "IlqrPollRec mirrors altro_hip_poll_record");
  int rc;
  const size_t bytes = (size_t)h->batch * sizeof(IlqrResult);
  if (!h->i_results) {
    if ((rc = dmalloc(h, &h->i_results, bytes))) return rc;
    if (hmalloc_quiet(h, &h->i_results_host, bytes, false) != hipSuccess) (void)hipGetLastError();
  }
  if (ilqr_launch_results(h->stream, h->i_prob, (IlqrResult*)h->i_results, h->batch)) return fail(ALTRO_HIP_ERR_HIP, "results kernel launch failed");
  void* stage = h->i_results_host ? h->i_results_host : (void*)results;
  HIP_TRY(hipMemcpyAsync(stage, h->i_results, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (stage != (void*)results) std::memcpy(results, stage, bytes);
  return 0;
}
extern "C" {

int altro_hip_ilqr_solve_async(altro_hip_batch* h, const altro_hip_solve_options* opts) {
  if (!h) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "null handle");
  h->async_request = true;
  const int rc = altro_hip_ilqr_solve(h, opts, nullptr);
  h->async_request = false;
  return rc;
}
int altro_hip_ilqr_poll(altro_hip_batch* h, int* n_done, const altro_hip_poll_record** records) {
  if (!h) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "null handle");
  if (!h->poll_host) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_ilqr_solve_async has not been called");
  if (n_done) *n_done = __atomic_load_n(h->poll_count_host, __ATOMIC_ACQUIRE);
  if (records) *records = (const altro_hip_poll_record*)h->poll_host;
  return 0;
}
int altro_hip_ilqr_wait(altro_hip_batch* h, altro_hip_solve_result* results) {
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if (!h->poll_host) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_ilqr_solve_async has not been called");
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (h->async_pending) {   // the books of THAT solve: a later synchronous solve, or a second wait, keeps its own counts
    h->async_pending = false;
    int c4[4];
    HIP_TRY(hipMemcpy(c4, h->i_counters, sizeof(c4), hipMemcpyDeviceToHost));
    h->last_sweeps = c4[3];
    h->last_merit_launches = 0;
  }
  if (results) return ilqr_gather_results(h, results);
  return 0;
}

// altro_hip_ilqr_solve: capi_solve.hip

void altro_hip_default_solve_options(altro_hip_solve_options* o) {
  if (!o) return;
  o->iterations_max = 200;            // solver_options.hpp:16-39
  o->tol_stationarity = 1e-4;
  o->tol_primal_feasibility = 1e-4;
  o->tol_meritfun_gradient = 1e-8;
  o->use_backtracking_linesearch = 0;
  o->penalty_initial = 1.0;
  o->penalty_scaling = 10.0;
  o->penalty_max = 1e8;
  o->reg_initial = 0.0;     // the reference: reg = 0, failures ignored (solver.cpp:363, :449)
  o->reg_retry_max = 0;
  o->reg_scale = 10.0;
  o->reg_min = 1e-6;
  o->reg_max = 1e8;
  o->stop_when_running_at_most = 0;   // (extension: every problem to its own end)
  o->forms = 0;
  o->fused_sweeps = 0;
  o->decision_margin = 0.0;   // (the guard of the affine rounds is opt-in: it costs more than the rounds save -- altro_hip.h)
}
int altro_hip_set_forms(altro_hip_batch* h, unsigned forms) {
  int rc = check(h);
  if (rc) return rc;
  if ((forms & ALTRO_HIP_FORM_LANE_QUAD_OFF) && (forms & ALTRO_HIP_FORM_LANE_QUAD_ON))
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "ALTRO_HIP_FORM_LANE_QUAD_OFF and _ON exclude each other");
  if ((forms & ALTRO_HIP_FORM_GENERIC_LATE_Q_OFF) && (forms & ALTRO_HIP_FORM_GENERIC_LATE_Q_ON))
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "ALTRO_HIP_FORM_GENERIC_LATE_Q_OFF and _ON exclude each other");
  if (((h->forms ^ forms) & ALTRO_HIP_FORM_MERIT_ONE_LAUNCH) && h->merit_split >= 0) {   // decided at the first evaluation: decide again
    HIP_TRY(hipStreamSynchronize(h->stream));
    dfree(h, &h->i_merit_jk);
    dfree(h, &h->i_spec_jac);
    h->merit_split = -1;
  }
  h->forms = forms;
  return 0;
}
unsigned altro_hip_get_forms(const altro_hip_batch* h) { return h ? h->forms : 0u; }
int altro_hip_last_solve_counts(const altro_hip_batch* h, int* sweeps, int* merit_launches) {
  if (!h) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "null handle");
  if (sweeps) *sweeps = h->last_sweeps;
  if (merit_launches) *merit_launches = h->last_merit_launches;
  return 0;
}
int altro_hip_get_nominal(altro_hip_batch* h, double* x, double* u) {
  int rc = loop_entry(h, true);
  if (rc) return rc;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16 && !h->m_nom) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_tracking_cost has not been called");
  if (h->plan == ALTRO_HIP_PLAN_GENERIC && !h->g_xn) return fail(ALTRO_HIP_ERR_NOT_SET, "no cost has been set for the iLQR loop");
  const LoopShape s = loop_shape(h);   // (per-knot-point dimensions: packed [batch][sum nx], [batch][sum nu])
  if (x && (rc = field_get(h, s, LF_NOM_X, 0, h->N + 1, x))) return rc;
  if (u) rc = field_get(h, s, LF_NOM_U, 0, h->N, u);
  return rc;
}
// Expansion the backward pass will consume: A | B | lx | lu (reference layout), for parity tests.
int altro_hip_get_expansion(altro_hip_batch* h, double* A, double* B, double* lx, double* lu) {
  int rc = loop_entry(h);
  if (rc) return rc;
  const int n = h->n, m = h->m, N = h->N;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {   // Z = [A B] rows of the DYN records, [lx lu] of the COST records, lx_N of TERM
    if (h->dev_ptrs) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "altro_hip_get_expansion on plan MFMA16 writes host arrays");
    const int64_t B_ = h->batch;
    std::vector<double> raw;
    auto fetch = [&](const void* src, int64_t bs, int64_t ks, int off, int block, int nk) -> int {
      raw.assign((size_t)B_ * nk * block, 0.0);
      return aos_get(h, raw.data(), src, off, bs, ks, block, nk);
    };
    if ((A || B) && (rc = mfma16_get_z(h, 0, N, A, B))) return rc;
    if (lx || lu) {
      if ((rc = fetch(h->m_cin, h->m_st.cin_bs, h->m_st.cin_ks, MF_OFF_QR, 16, N))) return rc;
      for (int64_t b = 0; b < B_; ++b)
        for (int k = 0; k < N; ++k) {
          const double* qr = raw.data() + ((size_t)b * N + k) * 16;
          if (lx) for (int i = 0; i < n; ++i) lx[((size_t)b * (N + 1) + k) * n + i] = qr[i];
          if (lu) for (int i = 0; i < m; ++i) lu[((size_t)b * N + k) * m + i] = qr[MF_N + i];
        }
      if (lx) {
        if ((rc = fetch(h->m_term, MF_TERM, 0, MF_TERM_q, MF_N, 1))) return rc;
        for (int64_t b = 0; b < B_; ++b)
          for (int i = 0; i < n; ++i) lx[((size_t)b * (N + 1) + N) * n + i] = raw[(size_t)b * MF_N + i];
      }
    }
    return 0;
  }
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) {   // reference layout already: A, B as given, lx / lu the backward sweep's q / r
    auto get = [&](double* dst, int arr, int blk, int nk) -> int { return dst ? generic_get(h, arr, dst, blk, nk) : 0; };
    rc = get(A, G_A, n * n, N);
    if (!rc) rc = get(B, G_B, n * m, N);
    if (!rc) rc = get(lx, G_q, n, N + 1);
    if (!rc) rc = get(lu, G_r, m, N);
    return rc;
  }
  const LaneSizes z = lane_sizes(n, m);
  const int oq = 2 * n * n + 2 * n * m + m * m + n, orr = oq + n;
  auto get = [&](double* dst, int off, int len, int nk, bool with_term, int off_term) -> int {
    if (!dst) return 0;
    return lane_get(h, dst, h->l_in, 0, with_term ? h->l_term : nullptr, z.e_in, off, off_term, len, nk, N);
  };
  rc = get(A, 0, n * n, N, false, 0);
  if (!rc) rc = get(B, n * n, n * m, N, false, 0);
  if (!rc) rc = get(lx, oq, n, N + 1, true, n * n);
  if (!rc) rc = get(lu, orr, m, N, false, 0);
  return rc;
}

// The line-search state machine driven on the host by a callback: lets CPU-only tests pin it against
// the real reference line search (oracle/_ref) without a GPU.
double altro_hip_linesearch_host(altro_hip_merit_fn f, void* ctx, double alpha0, double phi0, double dphi0,
                                 int try_cubic_first, int use_backtracking, double c1, double c2,
                                 int* status, int* iters, double* phi, double* dphi) {
  LsOptions o = ls_default_options();
  o.try_cubic_first = try_cubic_first; o.use_backtracking = use_backtracking; o.c1 = c1; o.c2 = c2;
  LsState s;
  bool need = ls_begin(s, o, alpha0, phi0, dphi0);
  while (need) {
    double p = 0.0, dp = 0.0;
    f(s.alpha, &p, s.want_derivative ? &dp : nullptr, ctx);
    need = ls_feed(s, o, p, dp);
  }
  if (status) *status = s.status;
  if (iters) *iters = s.n_iters;
  if (phi) *phi = s.phi;
  if (dphi) *dphi = s.dphi;
  return s.alpha;
}

}  // extern "C"
