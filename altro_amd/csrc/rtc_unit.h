// rtc_unit.h -- WHAT capi_rtc.hip compiles at run time around a caller's model source, as plain data: the text of the translation unit,
// the kernels it instantiates, the compile options and the cache key of each of the three kinds of program (plan LANE's launch-sequenced
// loop, plan MFMA16's row-layout kernels, plans GENERIC / MFMA32's loop kernels).  Host code without a HIP header: tests/cpp/rtc_unit_test.cpp
// checks all of it with a plain C++ compiler; capi_rtc.hip's rtc_build is the one place that hands a unit to hiprtc.
#pragma once
#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace altro_hip {
namespace capi {

// the slots of a module's function table (RtcModule::fn), by kind.
// lane: the kernels of the launch-sequenced loop that depend on (model, n, m, T): ilqr_launch_f64.hip's list
enum RtcKernel { RTC_ROLLOUT = 0, RTC_ACCEPT, RTC_EXPAND, RTC_MERIT, RTC_MERIT_ROLL, RTC_MERIT_POINT, RTC_MERIT_SUM, RTC_SPEC_SELECT,
                 RTC_ZERO_RESIDUALS, RTC_STATIONARITY, RTC_DUAL, RTC_SHIFT, RTC_NUM };
// tile: the rollout, the dynamics expansion and the two merit kernels (line-search round / two-trial pass) of one (source, n, m,
// constraint blocks?, dense cost?, more than AL_MAXC slots?) -- four kernels instead of ten, the merit kernels being the library's heaviest compiles
// A unit for a handle with a slot from the caller's source (rtc_unit_tile's `user`: ALTRO_HIP_USER_CONSTRAINTS, kernels/ilqr_merit2_dpp.hip
// MD_USER_BLOCKS) has three more: the AL expansion (the cost's part included: it is one kernel), the dual update and the feasibility walk
enum RtcTileKernel { RTT_ROLLOUT = 0, RTT_EXPAND_DYN, RTT_MERIT, RTT_MERIT2, RTT_NUM, RTT_EXPAND_AL = RTT_NUM, RTT_DUAL, RTT_FEAS, RTT_NUM_ALL };
// generic: three kernels per (source, n, m): the open-loop rollout, the dynamics expansion and the merit evaluation.
// On plan MFMA32's shapes three more: the merit kernel, its two-trial pass and the dynamics expansion in the row layout
// (kernels/ilqr_row32.hip: every lane evaluates the caller's model; r32_model_step).  They are USED when they compiled without scratch
// memory (RtcModule::row_ok): a Jacobian the compiler cannot keep in registers -- a dense one of many states, a loop it cannot unroll --
// makes that formulation spill, and a spilling wave of that kernel waits for its reloads behind the prefetch (3.4 x slower
// than without); the wave-per-problem kernels above are the form for such models.
// A source that defines altro_user_constraint / _jacobian also gets the kernels that evaluate constraint blocks (ALTRO_HIP_USER_CONSTRAINTS:
// kernels/ilqr_generic.hip, GEN_USER_BLOCKS): the merit kernel above then carries them, and three more are instantiated -- the
// stationarity / feasibility walk, the AL expansion (the cost's part included: it is one kernel) and the dual update.
enum RtcGenKernel { RTG_ROLLOUT = 0, RTG_EXPAND_DYN, RTG_MERIT, RTG_NUM, RTG_ROW_MERIT = RTG_NUM, RTG_ROW_MERIT2, RTG_ROW_EXPAND_DYN, RTG_NUM_ROW,
                    RTG_STATIONARITY = RTG_NUM_ROW, RTG_EXPAND_AL, RTG_DUAL, RTG_NUM_ALL };
constexpr int RTC_MAX_SLOTS = RTC_NUM;   // the largest kind's table
static_assert(RTT_NUM_ALL <= RTC_MAX_SLOTS && RTG_NUM_ALL <= RTC_MAX_SLOTS, "RtcModule::fn holds every kind's kernels");

enum class RtcKind : char { lane = 'l', tile = 't', generic = 'g' };
struct RtcUnit {
  RtcKind kind;                      // leads the key, so that the kinds share one cache
  std::string key;                   // kind and everything below that the maker's arguments decide (rtc_build adds the device)
  std::string defines;               // the #define lines before the caller's source, after ALTRO_HIP_USER_MODEL
  std::string includes;              // the #include lines after it
  std::vector<std::string> exprs;    // name expressions of the kernels, by slot; "" = a slot this unit does not instantiate
  std::string args;                  // the kernels' one parameter, as the explicit instantiations spell it
  std::vector<const char*> options;  // compile options after --offload-arch
  const char* program = "";          // the program's name in the compiler's messages
  const char* where = "";            // "the model source does not compile<where> (hiprtc: ...)"
  const char* noun = "model";        // "... of the compiled <noun> failed", "... missing from the compiled <noun>"
};

inline const char* const kKernelExpr[RTC_NUM] = {
    "altro_hip::ilqr_rollout_kernel<altro_hip::MODEL_USER, %d, %d, %s>",
    "altro_hip::ilqr_accept_kernel<%d, %d, %s>",
    "altro_hip::ilqr_expand_kernel<altro_hip::MODEL_USER, %d, %d, %s>",
    "altro_hip::ilqr_merit_kernel<altro_hip::MODEL_USER, %d, %d, %s>",
    "altro_hip::ilqr_merit_roll_kernel<altro_hip::MODEL_USER, %d, %d, %s>",
    "altro_hip::ilqr_merit_point_kernel<altro_hip::MODEL_USER, %d, %d, %s>",
    "altro_hip::ilqr_merit_sum_kernel<altro_hip::MODEL_USER, %d, %d, %s>",
    "altro_hip::ilqr_spec_select_kernel<%d, %d, %s>",
    "altro_hip::ilqr_zero_residuals_kernel<%s>",
    "altro_hip::ilqr_stationarity_kernel<%d, %d, %s>",
    "altro_hip::ilqr_dual_update_kernel<%d, %d, %s>",
    "altro_hip::ilqr_shift_kernel<%d, %d, %s>",
};

// ck: IlqrArgs::cost_kind -- the kernels that read the cost record take it as their last template argument (kernels/ilqr_lane.hip)
inline std::string kernel_expr(int which, int n, int m, const char* T, int ck) {
  char buf[256];
  if (which == RTC_ZERO_RESIDUALS) std::snprintf(buf, sizeof(buf), kKernelExpr[which], T);
  else std::snprintf(buf, sizeof(buf), kKernelExpr[which], n, m, T);
  std::string e = buf;
  if (ck && (which == RTC_EXPAND || which == RTC_MERIT || which == RTC_MERIT_POINT)) e.insert(e.size() - 1, ", " + std::to_string(ck));
  return e;
}
// does `src` define a function of this name?  (the identifier followed by an opening parenthesis, outside // comments)
inline bool defines_function(const std::string& src, const char* name) {
  const size_t len = std::strlen(name);
  for (size_t p = src.find(name); p != std::string::npos; p = src.find(name, p + 1)) {
    if (p > 0 && (std::isalnum((unsigned char)src[p - 1]) || src[p - 1] == '_')) continue;
    size_t q = p + len;
    while (q < src.size() && std::isspace((unsigned char)src[q])) ++q;
    if (q >= src.size() || src[q] != '(') continue;
    const size_t line = src.rfind('\n', p);
    const size_t cmt = src.rfind("//", p);
    if (cmt != std::string::npos && (line == std::string::npos || cmt > line)) continue;   // inside a line comment
    return true;
  }
  return false;
}
inline bool source_has_constraints(const std::string& src) {
  return defines_function(src, "altro_user_constraint") && defines_function(src, "altro_user_constraint_jacobian");
}

// The compile options, and those of a unit with row-layout kernels.  (-unroll-threshold: these kernels -- kernels/ilqr_row32.hip, tile_model_step of
// kernels/ilqr_tile_model.hip -- find a Jacobian's structural zeros with __builtin_constant_p, which the compiler resolves right after its EARLY
// full-unroll pass: a caller's `for (e < n (n + m)) J[e] = 0` must be unrolled by then, and at the default threshold it is only unrolled later:
// every entry then counts as a nonzero, and the kernel spills 585 registers, the tile plan's merit kernels 240-330.)
inline const std::vector<const char*> kRtcOptions = {"-O3", "-std=c++17"}, kRtcRowOptions = {"-O3", "-std=c++17", "-mllvm", "-unroll-threshold=5000"};

// num_params (every maker's last argument): altro_hip_set_model_source_params' P.  P > 0: the caller's functions take `const T* p`, the
// P per-problem parameters -- ALTRO_HIP_USER_NP in the unit's defines (models.h, kernels/al_types.h gather them) and a piece of its key,
// so that one source text with and without parameters are two modules.  P = 0 adds nothing to either: the unit of altro_hip_set_model_source.
inline std::string rtc_np_key(int num_params) { return num_params > 0 ? "P" + std::to_string(num_params) + "|" : std::string(); }
inline std::string rtc_np_define(int num_params) { return num_params > 0 ? "#define ALTRO_HIP_USER_NP " + std::to_string(num_params) + "\n" : std::string(); }

// plan LANE: the launch-sequenced loop's kernels (kernels/ilqr_lane.hip) for one (source, n, m, element type, cost kind)
inline RtcUnit rtc_unit_lane(int n, int m, const char* T, int ck, const std::string& source, int num_params = 0) {
  RtcUnit u;
  u.kind = RtcKind::lane; u.program = "altro_user_model.hip";
  u.key = std::string(1, (char)u.kind) + "|" + std::to_string(n) + "|" + std::to_string(m) + "|" + T + "|" + std::to_string(ck) + "|" + rtc_np_key(num_params) + source;
  if (source_has_constraints(source)) u.defines = "#define ALTRO_HIP_USER_CONSTRAINTS 1\n";
  u.defines += rtc_np_define(num_params);
  u.includes = "#include \"kernels/ilqr_lane.hip\"\n";
  for (int w = 0; w < RTC_NUM; ++w) u.exprs.push_back(kernel_expr(w, n, m, T, ck));
  u.args = std::string("IlqrArgs<") + T + ">"; u.options = kRtcOptions;
  return u;
}
// plan MFMA16: the caller's model inside the tile plan's row-layout kernels (kernels/ilqr_tile_model.hip), fp64 records.
// wide: some knot point of the handle has more than AL_MAXC constraint slots -- the merit kernels are then the AL_TILE_MAXC-slot
// instantiations (the ones ilqr_launch_mfma16_wide.hip holds for the compiled-in models); a two-slot kernel would skip the slots past
// the second while the expansion, the dual update and the feasibility walk honour them.
// user: some slot of the handle comes from the source's altro_user_constraint / _jacobian (al != 0, and the source defines the pair):
// the unit is compiled with ALTRO_HIP_USER_CONSTRAINTS and also instantiates the three row-layout kernels that evaluate constraint
// rows outside the merit pass -- the library's own instantiations of them know nothing of such a slot.
inline RtcUnit rtc_unit_tile(int n, int m, int al, int dense, const std::string& source, int wide = 0, int user = 0, int num_params = 0) {
  RtcUnit u;
  u.kind = RtcKind::tile; u.program = "altro_user_tile_model.hip"; u.where = " for the tile plan"; u.noun = "tile model";
  u.key = std::string(1, (char)u.kind) + "|" + std::to_string(n) + "|" + std::to_string(m) + "|" + std::to_string(al) + "|" + std::to_string(dense) + "|" +
          std::to_string(wide) + (user ? "u" : "") + "|" + rtc_np_key(num_params) + source;
  u.defines = "#define ALTRO_HIP_TILE_N " + std::to_string(n) + "\n#define ALTRO_HIP_TILE_M " + std::to_string(m) + "\n";
  if (user) u.defines += "#define ALTRO_HIP_USER_CONSTRAINTS 1\n";
  u.defines += rtc_np_define(num_params);
  u.includes = "#include \"kernels/ilqr_mfma16.hip\"\n#include \"kernels/ilqr_merit2_dpp.hip\"\n";
  const char* B_[2] = {"false", "true"};
  u.exprs.resize(RTT_NUM);
  u.exprs[RTT_ROLLOUT] = "altro_hip::wave_rollout_model_kernel<double, altro_hip::MODEL_USER>";
  u.exprs[RTT_EXPAND_DYN] = "altro_hip::wave_expand_dyn_kernel<double, altro_hip::MODEL_USER>";
  const char* tail = wide ? ", altro_hip::MODEL_USER, true, false, altro_hip::AL_TILE_MAXC>" : ", altro_hip::MODEL_USER>";
  u.exprs[RTT_MERIT] = std::string("altro_hip::wave_merit_dpp_kernel<double, ") + B_[al] + ", false, " + B_[dense] + tail;
  u.exprs[RTT_MERIT2] = std::string("altro_hip::wave_merit_dpp_kernel<double, ") + B_[al] + ", true, " + B_[dense] + tail;
  if (user) {
    u.exprs.resize(RTT_NUM_ALL);
    u.exprs[RTT_EXPAND_AL] = std::string("altro_hip::wave_expand_dpp_kernel<double, ") + B_[dense] + ", false, altro_hip::" + (wide ? "AL_TILE_MAXC" : "AL_MAXC") + ">";
    u.exprs[RTT_DUAL] = "altro_hip::wave_dual_update_dpp_kernel<double>";
    u.exprs[RTT_FEAS] = "altro_hip::wave_feasibility_dpp_kernel<double>";
  }
  u.args = "IlqrWaveArgs<double>"; u.options = kRtcRowOptions;
  return u;
}
// plans GENERIC / MFMA32: the caller's model inside that plan's loop kernels (kernels/ilqr_generic.hip); row_shape: the shape is one of
// plan MFMA32's (tile32_supported), so the row-layout kernels are instantiated too
inline RtcUnit rtc_unit_generic(int n, int m, bool row_shape, const std::string& source, int num_params = 0) {
  RtcUnit u;
  u.kind = RtcKind::generic; u.program = "altro_user_generic_model.hip"; u.where = " for plan GENERIC's loop";
  u.key = std::string(1, (char)u.kind) + "|" + std::to_string(n) + "|" + std::to_string(m) + "|" + rtc_np_key(num_params) + source;
  const bool al = source_has_constraints(source);
  if (al) u.defines = "#define ALTRO_HIP_USER_CONSTRAINTS 1\n#define ALTRO_HIP_GEN_UN " + std::to_string(n) + "\n#define ALTRO_HIP_GEN_UM " + std::to_string(m) + "\n";
  u.defines += rtc_np_define(num_params);
  u.includes = std::string("#include \"kernels/ilqr_generic.hip\"\n") + (row_shape ? "#include \"kernels/ilqr_row32.hip\"\n" : "");
  const std::string nm = std::to_string(n) + ", " + std::to_string(m);
  u.exprs.resize(RTG_NUM_ALL);
  u.exprs[RTG_ROLLOUT] = "altro_hip::generic_model_rollout_kernel<double, altro_hip::MODEL_USER, " + nm + ">";
  u.exprs[RTG_EXPAND_DYN] = "altro_hip::generic_model_expand_dyn_kernel<double, altro_hip::MODEL_USER, " + nm + ">";
  u.exprs[RTG_MERIT] = "altro_hip::generic_merit_kernel<double, false, altro_hip::MODEL_USER, " + nm + ">";
  if (row_shape) {
    u.exprs[RTG_ROW_MERIT] = "altro_hip::row32_merit_kernel<double, " + nm + ", 1, false, altro_hip::MODEL_USER>";
    u.exprs[RTG_ROW_MERIT2] = "altro_hip::row32_merit_kernel<double, " + nm + ", 1, true, altro_hip::MODEL_USER>";
    u.exprs[RTG_ROW_EXPAND_DYN] = "altro_hip::row32_expand_dyn_kernel<double, " + nm + ", altro_hip::MODEL_USER>";
  }
  if (al) {
    u.exprs[RTG_STATIONARITY] = "altro_hip::generic_stationarity_kernel<double>";
    u.exprs[RTG_EXPAND_AL] = "altro_hip::generic_expand_al_kernel<double>";
    u.exprs[RTG_DUAL] = "altro_hip::generic_dual_update_kernel<double>";
  }
  u.args = "IlqrGenArgs<double>"; u.options = row_shape ? kRtcRowOptions : kRtcOptions;
  return u;
}

// The translation unit: the caller's templates under contract(on) (like every device function the solve paths share), the library's
// kernels, and explicit instantiations of the ones this unit names.
inline std::string rtc_unit_text(const RtcUnit& u, const std::string& source) {
  std::string src = "#define ALTRO_HIP_USER_MODEL 1\n" + u.defines + "#include \"rtc_compat.h\"\n#include \"fp_contract.h\"\nALTRO_FP_REGION_ON\n";
  src += "#line 1 \"user_model\"\n" + source + "\nALTRO_FP_REGION_END\n" + u.includes + "namespace altro_hip {\n";
  for (std::string e : u.exprs) {
    if (e.empty()) continue;
    for (size_t p; (p = e.find("altro_hip::")) != std::string::npos;) e.erase(p, std::strlen("altro_hip::"));
    src += "template __global__ void " + e + "(" + u.args + ");\n";
  }
  return src + "}\n";
}

}  // namespace capi
}  // namespace altro_hip
