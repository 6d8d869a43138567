// rtc_unit_test.cpp -- the units capi_rtc.hip compiles at run time around a caller's model source (altro_amd/csrc/rtc_unit.h), checked
// without a GPU and without the library: for a placeholder source, the text of the translation unit, the name expressions and the compile
// options of every kind of unit, on every branch its maker takes, against what the three builders that preceded rtc_unit.h handed to
// hiprtc for the same arguments (recorded from them, not from this header); and defines_function's two traps.
#include "rtc_unit.h"

#include <cstdio>

using namespace altro_hip::capi;

static const std::string kPlain =
    "template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}\n"
    "template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}\n";
static const std::string kCon = kPlain +
    "template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {}\n"
    "template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {}\n";

struct Case {
  const char* name;
  RtcUnit unit;
  const std::string* source;
  const char* program;   // the program's name
  const char* text;      // the translation unit
  const char* names;     // the name expressions in the order they are added, one per line
  const char* options;   // the compile options after --offload-arch, one per line
};

static int failures = 0;
static void check(bool ok, const char* name, const char* what, const std::string& got, const std::string& want) {
  if (ok) return;
  ++failures;
  std::printf("FAIL %s: %s\n--- got ---\n%s\n--- want ---\n%s\n", name, what, got.c_str(), want.c_str());
}
static std::string lines(const std::vector<std::string>& v) {
  std::string s;
  for (const std::string& e : v) if (!e.empty()) s += e + "\n";
  return s;
}

int main() {
  // lane (2, 1): fp64 / cost kind 0 / no constraint blocks, and fp32 / cost kind 1 / blocks; tile (12, 4): without and with constraint
  // blocks and dense cost; generic: (4, 2), which is no shape of plan MFMA32, and (13, 4), which is one, each without and with blocks
  const Case cases[] = {
      {"lane_f64_ck0", rtc_unit_lane(2, 1, "double", 0, kPlain), &kPlain, "altro_user_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_lane.hip"
namespace altro_hip {
template __global__ void ilqr_rollout_kernel<MODEL_USER, 2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_accept_kernel<2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_expand_kernel<MODEL_USER, 2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_merit_kernel<MODEL_USER, 2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_merit_roll_kernel<MODEL_USER, 2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_merit_point_kernel<MODEL_USER, 2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_merit_sum_kernel<MODEL_USER, 2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_spec_select_kernel<2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_zero_residuals_kernel<double>(IlqrArgs<double>);
template __global__ void ilqr_stationarity_kernel<2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_dual_update_kernel<2, 1, double>(IlqrArgs<double>);
template __global__ void ilqr_shift_kernel<2, 1, double>(IlqrArgs<double>);
}
)X",
       R"X(altro_hip::ilqr_rollout_kernel<altro_hip::MODEL_USER, 2, 1, double>
altro_hip::ilqr_accept_kernel<2, 1, double>
altro_hip::ilqr_expand_kernel<altro_hip::MODEL_USER, 2, 1, double>
altro_hip::ilqr_merit_kernel<altro_hip::MODEL_USER, 2, 1, double>
altro_hip::ilqr_merit_roll_kernel<altro_hip::MODEL_USER, 2, 1, double>
altro_hip::ilqr_merit_point_kernel<altro_hip::MODEL_USER, 2, 1, double>
altro_hip::ilqr_merit_sum_kernel<altro_hip::MODEL_USER, 2, 1, double>
altro_hip::ilqr_spec_select_kernel<2, 1, double>
altro_hip::ilqr_zero_residuals_kernel<double>
altro_hip::ilqr_stationarity_kernel<2, 1, double>
altro_hip::ilqr_dual_update_kernel<2, 1, double>
altro_hip::ilqr_shift_kernel<2, 1, double>
)X",
       R"X(-O3
-std=c++17
)X"},
      {"lane_f32_ck1_con", rtc_unit_lane(2, 1, "float", 1, kCon), &kCon, "altro_user_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_USER_CONSTRAINTS 1
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_lane.hip"
namespace altro_hip {
template __global__ void ilqr_rollout_kernel<MODEL_USER, 2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_accept_kernel<2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_expand_kernel<MODEL_USER, 2, 1, float, 1>(IlqrArgs<float>);
template __global__ void ilqr_merit_kernel<MODEL_USER, 2, 1, float, 1>(IlqrArgs<float>);
template __global__ void ilqr_merit_roll_kernel<MODEL_USER, 2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_merit_point_kernel<MODEL_USER, 2, 1, float, 1>(IlqrArgs<float>);
template __global__ void ilqr_merit_sum_kernel<MODEL_USER, 2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_spec_select_kernel<2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_zero_residuals_kernel<float>(IlqrArgs<float>);
template __global__ void ilqr_stationarity_kernel<2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_dual_update_kernel<2, 1, float>(IlqrArgs<float>);
template __global__ void ilqr_shift_kernel<2, 1, float>(IlqrArgs<float>);
}
)X",
       R"X(altro_hip::ilqr_rollout_kernel<altro_hip::MODEL_USER, 2, 1, float>
altro_hip::ilqr_accept_kernel<2, 1, float>
altro_hip::ilqr_expand_kernel<altro_hip::MODEL_USER, 2, 1, float, 1>
altro_hip::ilqr_merit_kernel<altro_hip::MODEL_USER, 2, 1, float, 1>
altro_hip::ilqr_merit_roll_kernel<altro_hip::MODEL_USER, 2, 1, float>
altro_hip::ilqr_merit_point_kernel<altro_hip::MODEL_USER, 2, 1, float, 1>
altro_hip::ilqr_merit_sum_kernel<altro_hip::MODEL_USER, 2, 1, float>
altro_hip::ilqr_spec_select_kernel<2, 1, float>
altro_hip::ilqr_zero_residuals_kernel<float>
altro_hip::ilqr_stationarity_kernel<2, 1, float>
altro_hip::ilqr_dual_update_kernel<2, 1, float>
altro_hip::ilqr_shift_kernel<2, 1, float>
)X",
       R"X(-O3
-std=c++17
)X"},
      {"tile_00", rtc_unit_tile(12, 4, 0, 0, kPlain), &kPlain, "altro_user_tile_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_TILE_N 12
#define ALTRO_HIP_TILE_M 4
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
namespace altro_hip {
template __global__ void wave_rollout_model_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_expand_dyn_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, false, false, false, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, false, true, false, MODEL_USER>(IlqrWaveArgs<double>);
}
)X",
       R"X(altro_hip::wave_rollout_model_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_expand_dyn_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, false, false, false, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, false, true, false, altro_hip::MODEL_USER>
)X",
       R"X(-O3
-std=c++17
-mllvm
-unroll-threshold=5000
)X"},
      {"tile_11", rtc_unit_tile(12, 4, 1, 1, kPlain), &kPlain, "altro_user_tile_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_TILE_N 12
#define ALTRO_HIP_TILE_M 4
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
namespace altro_hip {
template __global__ void wave_rollout_model_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_expand_dyn_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, true, false, true, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, true, true, true, MODEL_USER>(IlqrWaveArgs<double>);
}
)X",
       R"X(altro_hip::wave_rollout_model_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_expand_dyn_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, true, false, true, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, true, true, true, altro_hip::MODEL_USER>
)X",
       R"X(-O3
-std=c++17
-mllvm
-unroll-threshold=5000
)X"},
      {"gen_4_2", rtc_unit_generic(4, 2, false, kPlain), &kPlain, "altro_user_generic_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_generic.hip"
namespace altro_hip {
template __global__ void generic_model_rollout_kernel<double, MODEL_USER, 4, 2>(IlqrGenArgs<double>);
template __global__ void generic_model_expand_dyn_kernel<double, MODEL_USER, 4, 2>(IlqrGenArgs<double>);
template __global__ void generic_merit_kernel<double, false, MODEL_USER, 4, 2>(IlqrGenArgs<double>);
}
)X",
       R"X(altro_hip::generic_model_rollout_kernel<double, altro_hip::MODEL_USER, 4, 2>
altro_hip::generic_model_expand_dyn_kernel<double, altro_hip::MODEL_USER, 4, 2>
altro_hip::generic_merit_kernel<double, false, altro_hip::MODEL_USER, 4, 2>
)X",
       R"X(-O3
-std=c++17
)X"},
      {"gen_4_2_con", rtc_unit_generic(4, 2, false, kCon), &kCon, "altro_user_generic_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_USER_CONSTRAINTS 1
#define ALTRO_HIP_GEN_UN 4
#define ALTRO_HIP_GEN_UM 2
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_generic.hip"
namespace altro_hip {
template __global__ void generic_model_rollout_kernel<double, MODEL_USER, 4, 2>(IlqrGenArgs<double>);
template __global__ void generic_model_expand_dyn_kernel<double, MODEL_USER, 4, 2>(IlqrGenArgs<double>);
template __global__ void generic_merit_kernel<double, false, MODEL_USER, 4, 2>(IlqrGenArgs<double>);
template __global__ void generic_stationarity_kernel<double>(IlqrGenArgs<double>);
template __global__ void generic_expand_al_kernel<double>(IlqrGenArgs<double>);
template __global__ void generic_dual_update_kernel<double>(IlqrGenArgs<double>);
}
)X",
       R"X(altro_hip::generic_model_rollout_kernel<double, altro_hip::MODEL_USER, 4, 2>
altro_hip::generic_model_expand_dyn_kernel<double, altro_hip::MODEL_USER, 4, 2>
altro_hip::generic_merit_kernel<double, false, altro_hip::MODEL_USER, 4, 2>
altro_hip::generic_stationarity_kernel<double>
altro_hip::generic_expand_al_kernel<double>
altro_hip::generic_dual_update_kernel<double>
)X",
       R"X(-O3
-std=c++17
)X"},
      {"gen_13_4", rtc_unit_generic(13, 4, true, kPlain), &kPlain, "altro_user_generic_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_generic.hip"
#include "kernels/ilqr_row32.hip"
namespace altro_hip {
template __global__ void generic_model_rollout_kernel<double, MODEL_USER, 13, 4>(IlqrGenArgs<double>);
template __global__ void generic_model_expand_dyn_kernel<double, MODEL_USER, 13, 4>(IlqrGenArgs<double>);
template __global__ void generic_merit_kernel<double, false, MODEL_USER, 13, 4>(IlqrGenArgs<double>);
template __global__ void row32_merit_kernel<double, 13, 4, 1, false, MODEL_USER>(IlqrGenArgs<double>);
template __global__ void row32_merit_kernel<double, 13, 4, 1, true, MODEL_USER>(IlqrGenArgs<double>);
template __global__ void row32_expand_dyn_kernel<double, 13, 4, MODEL_USER>(IlqrGenArgs<double>);
}
)X",
       R"X(altro_hip::generic_model_rollout_kernel<double, altro_hip::MODEL_USER, 13, 4>
altro_hip::generic_model_expand_dyn_kernel<double, altro_hip::MODEL_USER, 13, 4>
altro_hip::generic_merit_kernel<double, false, altro_hip::MODEL_USER, 13, 4>
altro_hip::row32_merit_kernel<double, 13, 4, 1, false, altro_hip::MODEL_USER>
altro_hip::row32_merit_kernel<double, 13, 4, 1, true, altro_hip::MODEL_USER>
altro_hip::row32_expand_dyn_kernel<double, 13, 4, altro_hip::MODEL_USER>
)X",
       R"X(-O3
-std=c++17
-mllvm
-unroll-threshold=5000
)X"},
      {"gen_13_4_con", rtc_unit_generic(13, 4, true, kCon), &kCon, "altro_user_generic_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_USER_CONSTRAINTS 1
#define ALTRO_HIP_GEN_UN 13
#define ALTRO_HIP_GEN_UM 4
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_generic.hip"
#include "kernels/ilqr_row32.hip"
namespace altro_hip {
template __global__ void generic_model_rollout_kernel<double, MODEL_USER, 13, 4>(IlqrGenArgs<double>);
template __global__ void generic_model_expand_dyn_kernel<double, MODEL_USER, 13, 4>(IlqrGenArgs<double>);
template __global__ void generic_merit_kernel<double, false, MODEL_USER, 13, 4>(IlqrGenArgs<double>);
template __global__ void row32_merit_kernel<double, 13, 4, 1, false, MODEL_USER>(IlqrGenArgs<double>);
template __global__ void row32_merit_kernel<double, 13, 4, 1, true, MODEL_USER>(IlqrGenArgs<double>);
template __global__ void row32_expand_dyn_kernel<double, 13, 4, MODEL_USER>(IlqrGenArgs<double>);
template __global__ void generic_stationarity_kernel<double>(IlqrGenArgs<double>);
template __global__ void generic_expand_al_kernel<double>(IlqrGenArgs<double>);
template __global__ void generic_dual_update_kernel<double>(IlqrGenArgs<double>);
}
)X",
       R"X(altro_hip::generic_model_rollout_kernel<double, altro_hip::MODEL_USER, 13, 4>
altro_hip::generic_model_expand_dyn_kernel<double, altro_hip::MODEL_USER, 13, 4>
altro_hip::generic_merit_kernel<double, false, altro_hip::MODEL_USER, 13, 4>
altro_hip::row32_merit_kernel<double, 13, 4, 1, false, altro_hip::MODEL_USER>
altro_hip::row32_merit_kernel<double, 13, 4, 1, true, altro_hip::MODEL_USER>
altro_hip::row32_expand_dyn_kernel<double, 13, 4, altro_hip::MODEL_USER>
altro_hip::generic_stationarity_kernel<double>
altro_hip::generic_expand_al_kernel<double>
altro_hip::generic_dual_update_kernel<double>
)X",
       R"X(-O3
-std=c++17
-mllvm
-unroll-threshold=5000
)X"},
      // (more than AL_MAXC constraint slots at a knot point: the merit kernels' AL_TILE_MAXC-slot instantiations)
      {"tile_11w", rtc_unit_tile(12, 4, 1, 1, kPlain, 1), &kPlain, "altro_user_tile_model.hip",
       R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_TILE_N 12
#define ALTRO_HIP_TILE_M 4
#include "rtc_compat.h"
#include "fp_contract.h"
ALTRO_FP_REGION_ON
#line 1 "user_model"
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}

ALTRO_FP_REGION_END
#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
namespace altro_hip {
template __global__ void wave_rollout_model_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_expand_dyn_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, true, false, true, MODEL_USER, true, false, AL_TILE_MAXC>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, true, true, true, MODEL_USER, true, false, AL_TILE_MAXC>(IlqrWaveArgs<double>);
}
)X",
       R"X(altro_hip::wave_rollout_model_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_expand_dyn_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, true, false, true, altro_hip::MODEL_USER, true, false, altro_hip::AL_TILE_MAXC>
altro_hip::wave_merit_dpp_kernel<double, true, true, true, altro_hip::MODEL_USER, true, false, altro_hip::AL_TILE_MAXC>
)X",
       R"X(-O3
-std=c++17
-mllvm
-unroll-threshold=5000
)X"},
  };
  for (const Case& c : cases) {
    const std::string text = rtc_unit_text(c.unit, *c.source), names = lines(c.unit.exprs);
    std::string options;
    for (const char* o : c.unit.options) options += std::string(o) + "\n";
    check(text == c.text, c.name, "unit text", text, c.text);
    check(names == c.names, c.name, "name expressions", names, c.names);
    check(options == c.options, c.name, "compile options", options, c.options);
    check(std::string(c.unit.program) == c.program, c.name, "program name", c.unit.program, c.program);
  }
  // the slots: a lane unit fills RtcKernel's, a tile unit RtcTileKernel's, a generic unit leaves empty what it does not instantiate
  auto filled = [](const RtcUnit& u) { std::string s; for (const std::string& e : u.exprs) s += e.empty() ? '-' : 'x'; return s; };
  const char* want_slots[] = {"xxxxxxxxxxxx", "xxxxxxxxxxxx", "xxxx", "xxxx", "xxx------", "xxx---xxx", "xxxxxx---", "xxxxxxxxx", "xxxx"};
  for (size_t i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) check(filled(cases[i].unit) == want_slots[i], cases[i].name, "slots", filled(cases[i].unit), want_slots[i]);
  check(cases[7].unit.exprs[RTG_ROW_MERIT2].find("row32_merit_kernel<double, 13, 4, 1, true") != std::string::npos, "gen_13_4_con", "RTG_ROW_MERIT2", cases[7].unit.exprs[RTG_ROW_MERIT2], "");
  check(cases[5].unit.exprs[RTG_DUAL] == "altro_hip::generic_dual_update_kernel<double>", "gen_4_2_con", "RTG_DUAL", cases[5].unit.exprs[RTG_DUAL], "");
  // one cache serves the three kinds: their keys differ for the same (n, m, source), and a key tells every argument of its maker apart
  const std::string kl = rtc_unit_lane(12, 4, "double", 0, kPlain).key, kt = rtc_unit_tile(12, 4, 0, 0, kPlain).key, kg = rtc_unit_generic(12, 4, false, kPlain).key;
  check(kl != kt && kl != kg && kt != kg, "keys", "the kinds' keys differ", kl.substr(0, 24) + " / " + kt.substr(0, 24) + " / " + kg.substr(0, 24), "");
  check(cases[0].unit.key != cases[1].unit.key && cases[2].unit.key != cases[3].unit.key && cases[4].unit.key != cases[5].unit.key &&
        cases[4].unit.key != cases[6].unit.key && kt != rtc_unit_tile(12, 4, 1, 0, kPlain).key && kt != rtc_unit_tile(12, 4, 0, 1, kPlain).key &&
        cases[3].unit.key != cases[8].unit.key && rtc_unit_tile(12, 4, 1, 0, kPlain).key != rtc_unit_tile(12, 4, 1, 0, kPlain, 1).key &&
        kl != rtc_unit_lane(12, 4, "float", 0, kPlain).key && kl != rtc_unit_lane(12, 4, "double", 1, kPlain).key, "keys", "arguments", "", "");
  // defines_function: a name that appears only inside a // comment, and one that is the tail of a longer identifier, define nothing
  check(!defines_function("// altro_user_constraint(int id) is not defined here\nint f(int);\n", "altro_user_constraint"), "defines_function", "comment", "true", "false");
  check(!defines_function("void my_altro_user_constraint(int id);\n", "altro_user_constraint"), "defines_function", "suffix", "true", "false");
  check(defines_function("int f(); // note\nvoid altro_user_constraint (int id);\n", "altro_user_constraint"), "defines_function", "definition", "false", "true");
  check(!source_has_constraints(kPlain) && source_has_constraints(kCon), "source_has_constraints", "placeholders", "", "");
  std::printf(failures ? "%d check(s) failed\n" : "rtc_unit_test ok\n", failures);
  return failures ? 1 : 0;
}
