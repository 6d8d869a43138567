// capi_rtc.hip -- C ABI: caller-supplied dynamics in the batched AL-iLQR loop (plan LANE), compiled at run time.
//
// ALTROSolver::SetExplicitDynamics (altro_solver.cpp:68-81) takes two host callbacks (typedefs.hpp:31-53); a std::function
// cannot run on the device, so the batched path offers the device-side equivalent: the caller hands the SOURCE of the
// continuous dynamics and of its Jacobian -- hand-written HIP, two function templates -- and the library compiles its own
// lane-per-problem iLQR kernels (kernels/ilqr_lane.hip) around them with hiprtc, once per (source, n, m, element type) and
// process.  The kernels are the very ones the compiled-in models use (MODEL_PENDULUM, MODEL_BICYCLE ...): the pendulum
// supplied as source solves to the same bits as MODEL_PENDULUM (tests/test_gpu_user_model.py).  The library's own sources
// travel inside libaltro_hip.so (.incbin below); hiprtc is resolved with dlopen at first use, so the library keeps its one
// link-time dependency (the HIP runtime).  Whole solves of such a handle run on the launch-sequenced loop (the one-launch
// fused kernel is not compiled at run time: it is the library's longest compile).
#include "capi_internal.h"

#include <cmath>
#include <cstring>
#include <dlfcn.h>
#include <hip/hiprtc.h>

#include <map>
#include <mutex>
#include <string>

using namespace altro_hip;
using namespace altro_hip::capi;

// ---- the sources hiprtc needs, embedded at build time (paths relative to the -I of csrc) ------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#define ALTRO_EMBED(sym, path)                                                                                       \
  __asm__(".pushsection .rodata\n.global " #sym "\n" #sym ":\n.incbin \"" path "\"\n.byte 0\n.popsection\n"); \
  extern "C" const char sym[];
#else
#define ALTRO_EMBED(sym, path) extern "C" const char sym[];
#endif
ALTRO_EMBED(altro_rtc_src_rtc_compat, "rtc_compat.h")
ALTRO_EMBED(altro_rtc_src_fp_contract, "fp_contract.h")
ALTRO_EMBED(altro_rtc_src_models, "models.h")
ALTRO_EMBED(altro_rtc_src_linesearch, "linesearch_sm.h")
ALTRO_EMBED(altro_rtc_src_ilqr_types, "kernels/ilqr_types.h")
ALTRO_EMBED(altro_rtc_src_al_types, "kernels/al_types.h")
ALTRO_EMBED(altro_rtc_src_al_lane, "kernels/al_lane.hip")
ALTRO_EMBED(altro_rtc_src_tvlqr_lane, "kernels/tvlqr_lane.hip")
ALTRO_EMBED(altro_rtc_src_lane_body, "kernels/tvlqr_lane_body.inc")
ALTRO_EMBED(altro_rtc_src_quad_body, "kernels/tvlqr_quad_body.inc")
ALTRO_EMBED(altro_rtc_src_quad2_body, "kernels/tvlqr_quad2_body.inc")
ALTRO_EMBED(altro_rtc_src_ilqr_lane, "kernels/ilqr_lane.hip")
// ... and of the tile plan's row-layout kernels (a caller's model on plan MFMA16)
ALTRO_EMBED(altro_rtc_src_mfma16_layout, "kernels/mfma16_layout.h")
ALTRO_EMBED(altro_rtc_src_ilqr_mfma16, "kernels/ilqr_mfma16.hip")
ALTRO_EMBED(altro_rtc_src_merit2_dpp, "kernels/ilqr_merit2_dpp.hip")
ALTRO_EMBED(altro_rtc_src_tile_model, "kernels/ilqr_tile_model.hip")
// ... and of plan GENERIC's loop kernels (a caller's model on plans GENERIC / MFMA32)
ALTRO_EMBED(altro_rtc_src_generic_arrays, "kernels/generic_arrays.h")
ALTRO_EMBED(altro_rtc_src_ilqr_generic, "kernels/ilqr_generic.hip")
ALTRO_EMBED(altro_rtc_src_ilqr_row32, "kernels/ilqr_row32.hip")

namespace {

struct Hiprtc {
  void* lib = nullptr;
  decltype(&hiprtcCreateProgram) CreateProgram = nullptr;
  decltype(&hiprtcCompileProgram) CompileProgram = nullptr;
  decltype(&hiprtcDestroyProgram) DestroyProgram = nullptr;
  decltype(&hiprtcAddNameExpression) AddNameExpression = nullptr;
  decltype(&hiprtcGetLoweredName) GetLoweredName = nullptr;
  decltype(&hiprtcGetCodeSize) GetCodeSize = nullptr;
  decltype(&hiprtcGetCode) GetCode = nullptr;
  decltype(&hiprtcGetProgramLogSize) GetProgramLogSize = nullptr;
  decltype(&hiprtcGetProgramLog) GetProgramLog = nullptr;
  decltype(&hiprtcGetErrorString) GetErrorString = nullptr;
};

int hiprtc_api(const Hiprtc** out) {
  static Hiprtc r;
  static std::string why = "symbols missing";
  static std::once_flag once;
  std::call_once(once, [] {
    const char* env = std::getenv("ALTRO_HIP_HIPRTC");
    void* lib = env ? dlopen(env, RTLD_NOW | RTLD_GLOBAL) : nullptr;
    for (const char* name : {"libhiprtc.so.7", "libhiprtc.so"})
      if (!lib) lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD);       // a copy the process already has
    for (const char* name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"})
      if (!lib) {
        lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { const char* e = dlerror(); if (e) why = e; }
      }
    if (!lib) return;
    const char* missing = nullptr;
#define SYM(field, name) \
  do { r.field = (decltype(r.field))dlsym(lib, name); if (!r.field && !missing) missing = name; } while (0)
    SYM(CreateProgram, "hiprtcCreateProgram"); SYM(CompileProgram, "hiprtcCompileProgram"); SYM(DestroyProgram, "hiprtcDestroyProgram");
    SYM(AddNameExpression, "hiprtcAddNameExpression"); SYM(GetLoweredName, "hiprtcGetLoweredName"); SYM(GetCodeSize, "hiprtcGetCodeSize");
    SYM(GetCode, "hiprtcGetCode"); SYM(GetProgramLogSize, "hiprtcGetProgramLogSize"); SYM(GetProgramLog, "hiprtcGetProgramLog");
    SYM(GetErrorString, "hiprtcGetErrorString");
#undef SYM
    if (missing) why = std::string("symbol ") + missing + " not found in libhiprtc";
    else r.lib = lib;
  });
  if (!r.lib) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "hiprtc (libhiprtc.so) could not be loaded: %s", why.c_str());
  *out = &r;
  return 0;
}

}  // namespace

namespace altro_hip {
namespace capi {

const struct RtcSource { const char* name; const char* text; } kRtcSources[] = {   // every source a unit may include; hiprtc reads the ones it does
    {"rtc_compat.h", altro_rtc_src_rtc_compat}, {"fp_contract.h", altro_rtc_src_fp_contract}, {"models.h", altro_rtc_src_models},
    {"linesearch_sm.h", altro_rtc_src_linesearch}, {"kernels/ilqr_types.h", altro_rtc_src_ilqr_types}, {"kernels/al_types.h", altro_rtc_src_al_types},
    {"kernels/al_lane.hip", altro_rtc_src_al_lane}, {"kernels/tvlqr_lane.hip", altro_rtc_src_tvlqr_lane}, {"kernels/tvlqr_lane_body.inc", altro_rtc_src_lane_body},
    {"kernels/tvlqr_quad_body.inc", altro_rtc_src_quad_body}, {"kernels/tvlqr_quad2_body.inc", altro_rtc_src_quad2_body}, {"kernels/ilqr_lane.hip", altro_rtc_src_ilqr_lane},
    {"kernels/mfma16_layout.h", altro_rtc_src_mfma16_layout}, {"kernels/ilqr_mfma16.hip", altro_rtc_src_ilqr_mfma16}, {"kernels/ilqr_merit2_dpp.hip", altro_rtc_src_merit2_dpp},
    {"kernels/ilqr_tile_model.hip", altro_rtc_src_tile_model}, {"kernels/generic_arrays.h", altro_rtc_src_generic_arrays}, {"kernels/ilqr_generic.hip", altro_rtc_src_ilqr_generic},
    {"kernels/ilqr_row32.hip", altro_rtc_src_ilqr_row32},
};

struct RtcModule {
  hipModule_t module = nullptr;
  hipFunction_t fn[RTC_MAX_SLOTS] = {};   // by the unit's slots (rtc_unit.h: RtcKernel / RtcTileKernel / RtcGenKernel)
  bool row_ok = false;   // generic: the row-layout kernels exist and none of them spills (see RtcGenKernel)
};
constexpr int RTG_ROW_SCRATCH_MAX = 256;   // bytes of private segment per lane a row-layout kernel may use and still be chosen

// generic: whether the row-layout kernels are to be chosen: when the module has them and none of them spills
static void rtc_gen_probe(const RtcUnit& unit, RtcModule* m) {
  m->row_ok = !unit.exprs[RTG_ROW_MERIT].empty();
  for (int w = RTG_ROW_MERIT; w < RTG_NUM_ROW && m->row_ok; ++w) {
    int scratch = 0;
    if (hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, m->fn[w]) != hipSuccess) { (void)hipGetLastError(); scratch = 1 << 30; }
    if (scratch > RTG_ROW_SCRATCH_MAX) m->row_ok = false;
  }
}

// Compile (or fetch) the module of `unit` around `source` on the handle's device, once per process and key: the lock is held across
// the compile, so that two handles with one key compile once; a failure leaves last_error and caches nothing.
static int rtc_build(altro_hip_batch* h, const RtcUnit& unit, const std::string& source, RtcModule** out) {
  *out = nullptr;
  static std::mutex mu;
  static std::map<std::string, RtcModule*> cache;
  const std::string key = std::to_string(h->device) + "|" + unit.key;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it != cache.end()) { *out = it->second; return 0; }
  const Hiprtc* R;
  if (const int rc = hiprtc_api(&R)) return rc;
  struct Unwind {   // whatever path leaves: the program goes, and so does a module that was not handed over
    const Hiprtc* R; hiprtcProgram prog = nullptr; RtcModule* m = nullptr;
    ~Unwind() { if (prog) R->DestroyProgram(&prog); if (m && m->module) (void)hipModuleUnload(m->module); delete m; }
  } u{R};
  constexpr int kSources = (int)(sizeof(kRtcSources) / sizeof(kRtcSources[0]));
  const char *hdr_src[kSources], *hdr_name[kSources];
  for (int i = 0; i < kSources; ++i) { hdr_src[i] = kRtcSources[i].text; hdr_name[i] = kRtcSources[i].name; }
  const std::string src = rtc_unit_text(unit, source);
  hiprtcResult rr = R->CreateProgram(&u.prog, src.c_str(), unit.program, kSources, hdr_src, hdr_name);
  if (rr != HIPRTC_SUCCESS) return fail(ALTRO_HIP_ERR_HIP, "hiprtcCreateProgram: %s", R->GetErrorString(rr));
  for (const std::string& e : unit.exprs)
    if (!e.empty()) R->AddNameExpression(u.prog, e.c_str());
  hipDeviceProp_t prop;
  std::string arch = "--offload-arch=gfx950";
  if (hipGetDeviceProperties(&prop, h->device) == hipSuccess) arch = std::string("--offload-arch=") + prop.gcnArchName;
  std::vector<const char*> opts = {arch.c_str()};
  opts.insert(opts.end(), unit.options.begin(), unit.options.end());
  rr = R->CompileProgram(u.prog, (int)opts.size(), opts.data());
  if (rr != HIPRTC_SUCCESS) {
    size_t ls = 0; R->GetProgramLogSize(u.prog, &ls);
    std::string log(ls, '\0');
    if (ls) R->GetProgramLog(u.prog, &log[0]);
    if (log.size() > 1800) log.resize(1800);
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "the model source does not compile%s (hiprtc: %s):\n%s", unit.where, R->GetErrorString(rr), log.c_str());
  }
  size_t cs = 0; R->GetCodeSize(u.prog, &cs);
  std::vector<char> code(cs);
  R->GetCode(u.prog, code.data());
  u.m = new RtcModule();
  if (const hipError_t le = hipModuleLoadData(&u.m->module, code.data()); le != hipSuccess)
    return fail(ALTRO_HIP_ERR_HIP, "hipModuleLoadData of the compiled %s failed: %s", unit.noun, hipGetErrorString(le));
  for (size_t w = 0; w < unit.exprs.size(); ++w) {
    const char* lowered = nullptr;
    if (!unit.exprs[w].empty() && (R->GetLoweredName(u.prog, unit.exprs[w].c_str(), &lowered) != HIPRTC_SUCCESS || !lowered ||
                                   hipModuleGetFunction(&u.m->fn[w], u.m->module, lowered) != hipSuccess))
      return fail(ALTRO_HIP_ERR_HIP, "kernel %s missing from the compiled %s", unit.exprs[w].c_str(), unit.noun);
  }
  if (unit.kind == RtcKind::generic) rtc_gen_probe(unit, u.m);
  *out = cache[key] = u.m;
  u.m = nullptr;
  return 0;
}
// the lane and tile kinds' units from a handle
// (np: the source's per-problem parameters, altro_hip_batch::model_np once the source is the handle's)
static int rtc_lane_module(altro_hip_batch* h, const std::string& source, int ck, int np, RtcModule** out) {
  return rtc_build(h, rtc_unit_lane(h->n, h->m, h->dtype == ALTRO_HIP_F64 ? "double" : "float", ck, source, np), source, out);
}
// (ck: altro_hip_batch::rtc_ck, the bits of loop_route.h: route_tile_module_key)
static int rtc_tile_module(altro_hip_batch* h, int ck, RtcModule** out) {
  return rtc_build(h, rtc_unit_tile(h->n, h->m, ck & 1, (ck >> 1) & 1, h->rtc_source, (ck >> 2) & 1, (ck >> 3) & 1, h->model_np), h->rtc_source, out);
}
// The handle's module for the shape's route (once per operation, before its first step from the module).  Plan MFMA16: blocks, a dense cost, a
// third slot or a slot from the source came or went since the module was built; plan LANE: the handle's cost changed kind -- the
// instantiations for this combination (compiled once per key and process).  Plans GENERIC / MFMA32: one module per source.
int rtc_current(altro_hip_batch* h, const RouteShape& s) {
  if (h->rtc_source.empty() || (s.plan != ALTRO_HIP_PLAN_MFMA16 && !h->rtc)) return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_model_source has not been called");
  if (s.plan == ALTRO_HIP_PLAN_GENERIC) return 0;
  const int ck = s.plan == ALTRO_HIP_PLAN_LANE ? (s.cost_dense ? 1 : 0) : route_tile_module_key(s);
  if (h->rtc && h->rtc_ck == ck) return 0;
  RtcModule* m2 = nullptr;
  if (const int rc = s.plan == ALTRO_HIP_PLAN_LANE ? rtc_lane_module(h, h->rtc_source, ck, h->model_np, &m2) : rtc_tile_module(h, ck, &m2)) return rc;
  h->rtc = m2; h->rtc_ck = ck;
  return 0;
}
// One step of a route (loop_route.h) from the handle's run-time module; args: the kernel's one parameter (only read).  (A constraint kernel is
// routed here only for a handle with a block from the source, and altro_hip_add_user_constraint refuses one whose source lacks the pair: the slot exists.)
int rtc_step(altro_hip_batch* h, const RouteStep& st, const void* args) {
  const RtcModule* mod = (const RtcModule*)h->rtc;
  const int w = route_rtc_slot(st.id);
  if (w < 0 || !mod->fn[w]) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "kernel %#x has no run-time compiled instantiation in the handle's module", st.id);
  void* params[] = {const_cast<void*>(args)};
  const hipError_t e = hipModuleLaunchKernel(mod->fn[w], st.gx, st.gy, st.gz, st.block, 1, 1, st.lds, h->stream, params, nullptr);
  return e == hipSuccess ? 0 : fail(ALTRO_HIP_ERR_HIP, "launch of the run-time compiled kernel %d of plan %d failed: %s", w, h->plan, hipGetErrorString(e));
}

}  // namespace capi
}  // namespace altro_hip

// altro_hip_set_model_source (num_params = 0) and altro_hip_set_model_source_params: the same path, the unit's makers take the count
static int set_model_source(altro_hip_batch* h, const char* source, float timestep, int num_params) {
  int rc = loop_entry(h);
  if (rc) return rc;
  h->expansion_current = false;
  if (!source) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "source == NULL");
  if (!(timestep > 0.0f)) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "time step must be positive (ErrorCodes::TimestepNotPositive)");
  HIP_TRY(hipSetDevice(h->device));
  const std::string src(source);
  const bool c_val = defines_function(src, "altro_user_constraint"), c_jac = defines_function(src, "altro_user_constraint_jacobian");
  if (c_val != c_jac)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "the model source defines %s but not %s: constraint blocks need both",
                c_val ? "altro_user_constraint" : "altro_user_constraint_jacobian", c_val ? "altro_user_constraint_jacobian" : "altro_user_constraint");
  // nonlinear constraint blocks from source are plans LANE's and GENERIC's: an ALTRO_HIP_PLAN_AUTO handle that rides the padded tile only
  // because of its shape / batch size moves to one of them while it is still empty -- LANE for n <= 6, else GENERIC
  // (a handle created with ALTRO_HIP_TILE_USER_BLOCKS keeps them on the tile: fp64 records, kernels/ilqr_merit2_dpp.hip MD_USER_BLOCKS)
  const bool tile_user = h->plan == ALTRO_HIP_PLAN_MFMA16 && (h->flags & ALTRO_HIP_TILE_USER_BLOCKS) != 0 && h->dtype == ALTRO_HIP_F64;
  if (h->plan == ALTRO_HIP_PLAN_MFMA16 && h->auto_plan && c_val && !tile_user &&
      (rc = replan_empty_handle(h, lane_supported(h->n, h->m) ? ALTRO_HIP_PLAN_LANE : ALTRO_HIP_PLAN_GENERIC))) return rc;
  if (h->plan == ALTRO_HIP_PLAN_GENERIC) {   // plans GENERIC / MFMA32: the caller's model inside that plan's loop kernels (any n, m <= 32)
    if (h->ragged) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "device models need uniform dimensions");
    if (h->dtype != ALTRO_HIP_F64) return fail(ALTRO_HIP_ERR_UNSUPPORTED, "device models on plans GENERIC / MFMA32 run on fp64 handles");
    if (h->n > 32 || h->m > 32)
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "run-time compiled models on plan GENERIC take n, m <= 32 (got %d, %d)", h->n, h->m);
    h->rtc_source = src;
    h->model = ModelParams{MODEL_USER, timestep, 0, 2.7, 1.5};
    model_params_drop(h); h->model_np = num_params;
    RtcModule* gm = nullptr;   // compile now: a source that does not build must fail HERE, with the compiler's log
    if ((rc = rtc_build(h, rtc_unit_generic(h->n, h->m, tile32_shape_ok(h->n, h->m), src, num_params), src, &gm))) { h->rtc_source.clear(); h->model = ModelParams{MODEL_LINEAR, 0.0f, 0, 2.7, 1.5}; h->model_np = 0; return rc; }
    h->model_set = true; h->rtc_has_constraints = c_val && c_jac;
    h->rtc = gm; h->rtc_row32_ok = gm->row_ok;
    return model_takes_dynamics(h);
  }
  if (h->plan != ALTRO_HIP_PLAN_LANE && h->plan != ALTRO_HIP_PLAN_MFMA16)
    return fail(ALTRO_HIP_ERR_UNSUPPORTED, "unknown plan %d", h->plan);
  if (h->plan == ALTRO_HIP_PLAN_MFMA16) {   // the tile plan's row-layout kernels around the caller's model (kernels/ilqr_tile_model.hip)
    if (h->dtype != ALTRO_HIP_F64)
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "device models on plan MFMA16 run on fp64 records (create the handle with ALTRO_HIP_F64)");
    if ((c_val || c_jac) && !tile_user)
      return fail(ALTRO_HIP_ERR_UNSUPPORTED, "nonlinear constraint blocks from source run on plan GENERIC (ALTRO_HIP_PLAN_GENERIC, any n, m <= 32) "
                                             "and plan LANE; plan MFMA16 takes the model's two functions and linear blocks (altro_hip_add_linear_constraint)");
    h->rtc_source = src;
    h->model = ModelParams{MODEL_USER, timestep, 0, 2.7, 1.5};
    model_params_drop(h); h->model_np = num_params;
    RtcModule* tm = nullptr;   // compile now: a source that does not build must fail HERE, with the compiler's log
    if (!h->al_defs.empty() && (rc = al_upload(h))) { h->rtc_source.clear(); h->model = ModelParams{MODEL_LINEAR, 0.0f, 0, 2.7, 1.5}; h->model_np = 0; return rc; }   // (al_sum.max_ncon: the slots of the blocks so far)
    const bool user = !h->al_defs.empty() && h->al_sum.has_user;   // (a source that replaces one whose blocks the handle still has)
    if (user && !c_val) {
      h->rtc_source.clear(); h->model = ModelParams{MODEL_LINEAR, 0.0f, 0, 2.7, 1.5}; h->model_np = 0;
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "the handle has constraint blocks from source (altro_hip_add_user_constraint): the new source must define "
                                              "altro_user_constraint and altro_user_constraint_jacobian, or altro_hip_clear_constraints must come first");
    }
    // (a flagged handle whose source defines the pair announces blocks from it: the unit compiled -- and checked -- here is the one a
    //  handle with such a block launches, at the width of the blocks registered so far; rtc_tile_current builds another if it turns out otherwise)
    const bool expect_user = user || (tile_user && c_val);
    const int ck = ((h->al_defs.empty() && !expect_user) ? 0 : 1) | (h->cost_dense ? 2 : 0) | ((!h->al_defs.empty() && h->al_sum.max_ncon > AL_MAXC) ? 4 : 0) | (expect_user ? 8 : 0);
    if ((rc = rtc_tile_module(h, ck, &tm))) { h->rtc_source.clear(); h->model_np = 0; return rc; }
    h->rtc = tm; h->rtc_ck = ck; h->model_set = true; h->rtc_has_constraints = tile_user && c_val && c_jac;
    return model_takes_dynamics(h);
  }
  RtcModule* m = nullptr;
  const int ck = h->cost_dense ? 1 : 0;
  if ((rc = rtc_lane_module(h, src, ck, num_params, &m))) return rc;   // (altro_hip_last_error has the compiler's log)
  h->rtc = m; h->rtc_ck = ck; h->rtc_source = src;
  h->rtc_has_constraints = c_val && c_jac;
  h->model = ModelParams{MODEL_USER, timestep, 0, 2.7, 1.5};
  model_params_drop(h); h->model_np = num_params;
  h->model_set = true;
  return 0;
}

extern "C" {

int altro_hip_set_model_source(altro_hip_batch* h, const char* source, float timestep) { return set_model_source(h, source, timestep, 0); }

int altro_hip_set_model_source_params(altro_hip_batch* h, const char* source, float timestep, int num_params) {
  if (num_params < 0 || num_params > ALTRO_HIP_MODEL_MAX_PARAMS)
    return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "num_params = %d: a model from source takes 0 .. ALTRO_HIP_MODEL_MAX_PARAMS = %d per-problem parameters",
                num_params, ALTRO_HIP_MODEL_MAX_PARAMS);
  return set_model_source(h, source, timestep, num_params);
}

// The per-problem parameters of the handle's source (ModelParams::theta, AlTable::theta): host [batch][P] in, [P][batch] in the handle's
// element type on the device -- what std::function callbacks closing over each solver's own constants are in the reference (typedefs.hpp:31-53)
int altro_hip_set_model_params(altro_hip_batch* h, const double* theta, int batch_stride_zero) {
  int rc = loop_entry(h);
  if (rc) return rc;
  const int P = h->model_np;
  if (!h->model_set || h->model.kind != MODEL_USER || P == 0)
    return fail(ALTRO_HIP_ERR_NOT_SET, "altro_hip_set_model_params needs a model from source with parameters (altro_hip_set_model_source_params, num_params > 0)");
  if (!theta) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "theta == NULL");
  const size_t B = (size_t)h->batch;
  const bool f64 = h->dtype == ALTRO_HIP_F64;
  for (size_t e = 0; e < (batch_stride_zero ? 1 : B) * P; ++e)
    if (!std::isfinite(theta[e]) || (!f64 && !std::isfinite((float)theta[e])))   // (fp32 handles: finite in the element type)
      return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "theta[%zu][%zu] = %g: every model parameter must be finite", e / P, e % P, theta[e]);
  const size_t esz = f64 ? sizeof(double) : sizeof(float), bytes = (size_t)P * B * esz;
  std::vector<double> kept(B * P);          // [batch][P], as stored: converted once to the element type, widened
  std::vector<char> dev(bytes);             // [P][batch] in the element type
  for (size_t b = 0; b < B; ++b)
    for (int i = 0; i < P; ++i) {
      const double v = theta[(batch_stride_zero ? 0 : b * P) + i];
      if (f64) { ((double*)dev.data())[(size_t)i * B + b] = v; kept[b * P + i] = v; }
      else { const float f = (float)v; ((float*)dev.data())[(size_t)i * B + b] = f; kept[b * P + i] = (double)f; }
    }
  if (!h->d_theta && (rc = dmalloc(h, &h->d_theta, bytes))) return rc;
  // (on the handle's own stream: launches already enqueued read the old values, later ones the new)
  HIP_TRY(hipMemcpyAsync(h->d_theta, dev.data(), bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->theta_host.swap(kept);
  h->model.theta = h->d_theta; h->model.theta_bs = h->batch;
  h->expansion_current = false;
  return 0;
}
int altro_hip_get_model_params(altro_hip_batch* h, double* theta) {
  int rc = loop_entry(h);
  if (rc) return rc;
  if (!h->model_set || h->model.kind != MODEL_USER || h->model_np == 0 || !h->model.theta)
    return fail(ALTRO_HIP_ERR_NOT_SET, h->model_np ? "altro_hip_set_model_params has not been called"
                                                   : "the handle's model takes no parameters (altro_hip_set_model_source_params, num_params > 0)");
  if (!theta) return fail(ALTRO_HIP_ERR_BAD_ARGUMENT, "theta == NULL");
  std::memcpy(theta, h->theta_host.data(), h->theta_host.size() * sizeof(double));
  return 0;
}
int altro_hip_model_num_params(const altro_hip_batch* h) { return (h && h->model_set && h->model.kind == MODEL_USER) ? h->model_np : 0; }
int altro_hip_model_row_layout(const altro_hip_batch* h) { return (h && row32_model_eligible(route_shape(h))) ? 1 : 0; }

}  // extern "C"
