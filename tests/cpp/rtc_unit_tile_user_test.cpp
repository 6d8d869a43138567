// rtc_unit_tile_user_test.cpp -- rtc_unit_tile's `user` argument (altro_amd/csrc/rtc_unit.h): the unit a plan MFMA16 handle with a
// constraint slot from the caller's source compiles.  Without a GPU and without the library: the text of the translation unit, its
// defines, name expressions, options and key with the argument; and that without it (the default) the unit is byte for byte what
// tests/cpp/rtc_unit_test.cpp pins for the same arguments.
#include "rtc_unit.h"

#include <cstdio>

using namespace altro_hip::capi;

static const std::string kCon =
    "template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {}\n"
    "template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {}\n"
    "template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {}\n"
    "template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {}\n";

static int failures = 0;
static void check(bool ok, const char* what, const std::string& got = "", const std::string& want = "") {
  if (ok) return;
  ++failures;
  std::printf("FAIL %s\n--- got ---\n%s\n--- want ---\n%s\n", what, got.c_str(), want.c_str());
}
static std::string lines(const std::vector<std::string>& v) {
  std::string s;
  for (const std::string& e : v) s += e + "\n";
  return s;
}

int main() {
  // the two-slot, diagonal-cost unit of a (12, 4) handle with a user slot
  const RtcUnit u = rtc_unit_tile(12, 4, 1, 0, kCon, 0, 1);
  const char* text = R"X(#define ALTRO_HIP_USER_MODEL 1
#define ALTRO_HIP_TILE_N 12
#define ALTRO_HIP_TILE_M 4
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
#include "kernels/ilqr_mfma16.hip"
#include "kernels/ilqr_merit2_dpp.hip"
namespace altro_hip {
template __global__ void wave_rollout_model_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_expand_dyn_kernel<double, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, true, false, false, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_merit_dpp_kernel<double, true, true, false, MODEL_USER>(IlqrWaveArgs<double>);
template __global__ void wave_expand_dpp_kernel<double, false, false, AL_MAXC>(IlqrWaveArgs<double>);
template __global__ void wave_dual_update_dpp_kernel<double>(IlqrWaveArgs<double>);
template __global__ void wave_feasibility_dpp_kernel<double>(IlqrWaveArgs<double>);
}
)X";
  check(rtc_unit_text(u, kCon) == text, "unit text (two slots, diagonal)", rtc_unit_text(u, kCon), text);
  check(u.defines == "#define ALTRO_HIP_TILE_N 12\n#define ALTRO_HIP_TILE_M 4\n#define ALTRO_HIP_USER_CONSTRAINTS 1\n", "defines", u.defines);
  check((int)u.exprs.size() == RTT_NUM_ALL && RTT_EXPAND_AL == RTT_NUM && RTT_NUM == 4 && RTT_NUM_ALL == 7, "slots");
  const char* names = R"X(altro_hip::wave_rollout_model_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_expand_dyn_kernel<double, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, true, false, false, altro_hip::MODEL_USER>
altro_hip::wave_merit_dpp_kernel<double, true, true, false, altro_hip::MODEL_USER>
altro_hip::wave_expand_dpp_kernel<double, false, false, altro_hip::AL_MAXC>
altro_hip::wave_dual_update_dpp_kernel<double>
altro_hip::wave_feasibility_dpp_kernel<double>
)X";
  check(lines(u.exprs) == names, "name expressions", lines(u.exprs), names);
  std::string options;
  for (const char* o : u.options) options += std::string(o) + "\n";
  check(options == "-O3\n-std=c++17\n-mllvm\n-unroll-threshold=5000\n", "options", options);
  check(std::string(u.program) == "altro_user_tile_model.hip" && u.args == "IlqrWaveArgs<double>" && u.kind == RtcKind::tile, "program, args, kind");
  // the wide, dense unit: the AL_TILE_MAXC-slot merit kernels and the six-slot dense expansion
  const RtcUnit wd = rtc_unit_tile(12, 4, 1, 1, kCon, 1, 1);
  check(wd.exprs[RTT_MERIT] == "altro_hip::wave_merit_dpp_kernel<double, true, false, true, altro_hip::MODEL_USER, true, false, altro_hip::AL_TILE_MAXC>", "wide merit", wd.exprs[RTT_MERIT]);
  check(wd.exprs[RTT_MERIT2] == "altro_hip::wave_merit_dpp_kernel<double, true, true, true, altro_hip::MODEL_USER, true, false, altro_hip::AL_TILE_MAXC>", "wide merit2", wd.exprs[RTT_MERIT2]);
  check(wd.exprs[RTT_EXPAND_AL] == "altro_hip::wave_expand_dpp_kernel<double, true, false, altro_hip::AL_TILE_MAXC>", "wide expansion", wd.exprs[RTT_EXPAND_AL]);
  check(wd.exprs[RTT_DUAL] == u.exprs[RTT_DUAL] && wd.exprs[RTT_FEAS] == u.exprs[RTT_FEAS], "dual update and feasibility do not depend on width or cost");
  // a padded shape: the defines carry the problem's own n, m
  check(rtc_unit_tile(6, 2, 1, 0, kCon, 0, 1).defines == "#define ALTRO_HIP_TILE_N 6\n#define ALTRO_HIP_TILE_M 2\n#define ALTRO_HIP_USER_CONSTRAINTS 1\n", "padded defines");
  // the key tells the argument apart from every other, and the default is today's unit byte for byte
  const RtcUnit d0 = rtc_unit_tile(12, 4, 1, 0, kCon), d1 = rtc_unit_tile(12, 4, 1, 0, kCon, 0), d2 = rtc_unit_tile(12, 4, 1, 0, kCon, 0, 0);
  check(d0.key == d1.key && d1.key == d2.key && d0.key == "t|12|4|1|0|0|" + kCon, "default key", d0.key);
  check(u.key != d0.key && u.key != wd.key && wd.key != rtc_unit_tile(12, 4, 1, 1, kCon, 1).key && u.key != rtc_unit_tile(12, 4, 1, 1, kCon, 0, 1).key &&
        u.key != rtc_unit_tile(6, 2, 1, 0, kCon, 0, 1).key, "keys differ");
  check(u.key.size() > kCon.size() && u.key.compare(u.key.size() - kCon.size(), kCon.size(), kCon) == 0, "the key ends with the source");
  check((int)d0.exprs.size() == RTT_NUM && d0.defines == "#define ALTRO_HIP_TILE_N 12\n#define ALTRO_HIP_TILE_M 4\n", "default slots and defines", d0.defines);
  check(rtc_unit_text(d0, kCon).find("ALTRO_HIP_USER_CONSTRAINTS") == std::string::npos &&
        rtc_unit_text(d0, kCon).find("wave_expand_dpp_kernel") == std::string::npos, "default text has nothing of the user slots");
  {   // the default unit's text is the user unit's minus the define and the three instantiations
    std::string t = rtc_unit_text(u, kCon);
    for (const char* cut : {"#define ALTRO_HIP_USER_CONSTRAINTS 1\n", "template __global__ void wave_expand_dpp_kernel<double, false, false, AL_MAXC>(IlqrWaveArgs<double>);\n",
                            "template __global__ void wave_dual_update_dpp_kernel<double>(IlqrWaveArgs<double>);\n",
                            "template __global__ void wave_feasibility_dpp_kernel<double>(IlqrWaveArgs<double>);\n"}) {
      const size_t p = t.find(cut);
      check(p != std::string::npos, "cut", cut);
      if (p != std::string::npos) t.erase(p, std::strlen(cut));
    }
    check(t == rtc_unit_text(d0, kCon), "default text", rtc_unit_text(d0, kCon), t);
  }
  std::printf(failures ? "%d check(s) failed\n" : "rtc_unit_tile_user_test ok\n", failures);
  return failures ? 1 : 0;
}
