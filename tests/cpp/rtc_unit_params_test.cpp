// rtc_unit_params_test.cpp -- the `num_params` argument of the three unit makers (altro_amd/csrc/rtc_unit.h), checked without a GPU and
// without the library.  For each maker, on a branch without and one with constraint blocks:
//   P = 0   text, key, defines, name expressions and options of the call without the argument (altro_hip_set_model_source's unit);
//   P = 3   `#define ALTRO_HIP_USER_NP 3` in the defines (once, ahead of the caller's source in the text), another key -- also another
//           than P = 4's -- and the name expressions and options of P = 0;
// and defines_function still finds a constraint pair that takes the parameters as a fifth argument.
#include "rtc_unit.h"

#include <cstdio>

using namespace altro_hip::capi;

static const std::string kPlain =
    "template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, const T* p, T* xdot) {}\n"
    "template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, const T* p, T* J) {}\n";
static const std::string kCon = kPlain +
    "template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, const T* p, T* c) {}\n"
    "template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, const T* p, T* J) {}\n";

static int failures = 0;
#define EXPECT(cond)                                                                          \
  do {                                                                                        \
    if (!(cond)) { std::printf("  EXPECT FAILED %s line %d: %s\n", name, __LINE__, #cond); ++failures; } \
  } while (0)

static size_t count(const std::string& s, const std::string& what) {
  size_t c = 0;
  for (size_t p = s.find(what); p != std::string::npos; p = s.find(what, p + 1)) ++c;
  return c;
}
static bool same_options(const RtcUnit& a, const RtcUnit& b) {
  if (a.options.size() != b.options.size()) return false;
  for (size_t i = 0; i < a.options.size(); ++i)
    if (std::string(a.options[i]) != b.options[i]) return false;
  return true;
}

// base: the maker without the argument; p0, p3, p4: with num_params = 0, 3, 4
static void check(const char* name, const std::string& source, const RtcUnit& base, const RtcUnit& p0, const RtcUnit& p3, const RtcUnit& p4) {
  const std::string kDef = "#define ALTRO_HIP_USER_NP 3\n";
  // P = 0: byte for byte the call without the argument
  EXPECT(p0.key == base.key);
  EXPECT(p0.defines == base.defines);
  EXPECT(p0.includes == base.includes);
  EXPECT(p0.exprs == base.exprs);
  EXPECT(p0.args == base.args);
  EXPECT(same_options(p0, base));
  EXPECT(rtc_unit_text(p0, source) == rtc_unit_text(base, source));
  EXPECT(count(rtc_unit_text(p0, source), "ALTRO_HIP_USER_NP") == 0);
  // P = 3: the define and the key, nothing else
  EXPECT(count(p3.defines, kDef) == 1);
  EXPECT(p3.defines.size() == base.defines.size() + kDef.size());
  EXPECT(p3.defines == base.defines + kDef);           // (after the unit's other defines)
  EXPECT(p3.key != base.key);
  EXPECT(p3.key != p4.key);
  EXPECT(p3.key[0] == base.key[0]);                    // (the kind still leads: the kinds share one cache)
  EXPECT(p3.key.size() > source.size() && p3.key.compare(p3.key.size() - source.size(), source.size(), source) == 0);
  EXPECT(p3.exprs == base.exprs);
  EXPECT(p3.includes == base.includes);
  EXPECT(p3.args == base.args);
  EXPECT(same_options(p3, base));
  const std::string text = rtc_unit_text(p3, source);
  EXPECT(count(text, kDef) == 1);
  EXPECT(text.find(kDef) < text.find("#line 1 \"user_model\""));   // ahead of the caller's source and of every header that reads it
  EXPECT(text.size() == rtc_unit_text(base, source).size() + kDef.size());
  EXPECT(count(p4.defines, "#define ALTRO_HIP_USER_NP 4\n") == 1);
}

int main() {
  const char* name = "defines_function";
  EXPECT(source_has_constraints(kCon));
  EXPECT(!source_has_constraints(kPlain));
  EXPECT(defines_function(kCon, "altro_user_constraint") && defines_function(kCon, "altro_user_constraint_jacobian"));
  EXPECT(defines_function(kPlain, "altro_user_dynamics") && !defines_function(kPlain, "altro_user_constraint"));

  check("lane_f64", kPlain, rtc_unit_lane(2, 1, "double", 0, kPlain), rtc_unit_lane(2, 1, "double", 0, kPlain, 0),
        rtc_unit_lane(2, 1, "double", 0, kPlain, 3), rtc_unit_lane(2, 1, "double", 0, kPlain, 4));
  check("lane_f32_blocks", kCon, rtc_unit_lane(3, 2, "float", 1, kCon), rtc_unit_lane(3, 2, "float", 1, kCon, 0),
        rtc_unit_lane(3, 2, "float", 1, kCon, 3), rtc_unit_lane(3, 2, "float", 1, kCon, 4));
  check("tile", kPlain, rtc_unit_tile(12, 4, 0, 0, kPlain), rtc_unit_tile(12, 4, 0, 0, kPlain, 0, 0, 0),
        rtc_unit_tile(12, 4, 0, 0, kPlain, 0, 0, 3), rtc_unit_tile(12, 4, 0, 0, kPlain, 0, 0, 4));
  check("tile_wide_user", kCon, rtc_unit_tile(12, 4, 1, 1, kCon, 1, 1), rtc_unit_tile(12, 4, 1, 1, kCon, 1, 1, 0),
        rtc_unit_tile(12, 4, 1, 1, kCon, 1, 1, 3), rtc_unit_tile(12, 4, 1, 1, kCon, 1, 1, 4));
  check("generic", kPlain, rtc_unit_generic(4, 2, false, kPlain), rtc_unit_generic(4, 2, false, kPlain, 0),
        rtc_unit_generic(4, 2, false, kPlain, 3), rtc_unit_generic(4, 2, false, kPlain, 4));
  check("generic_row_blocks", kCon, rtc_unit_generic(13, 4, true, kCon), rtc_unit_generic(13, 4, true, kCon, 0),
        rtc_unit_generic(13, 4, true, kCon, 3), rtc_unit_generic(13, 4, true, kCon, 4));
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("rtc_unit_params_test ok\n");
  return 0;
}
