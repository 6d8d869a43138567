// al_tables.h on the CPU (plain g++, nothing of the library linked), three ways:
//  (a) every table and every summary value of al_build against RECORDINGS of the function it replaced (al_upload_typed<T> of capi_ilqr.hip
//      with its HIP calls taken out, run on the cases below): element counts, the summary, and a 64-bit FNV-1a hash of every table taken
//      field by field (AlKnot has padding) and, for the value pools, over the bit patterns in the element type;
//  (b) plan MFMA16's slot layout of cases 3 and 4 against entries written out by hand from the layout comments of kernels/al_types.h;
//  (c) al_admit with every capacity reached exactly and exceeded by one, the expected answers written out from al_types.h's constants.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "al_tables.h"

using namespace altro_hip;
using namespace altro_hip::capi;

static int failures = 0;
static const char* where = "";
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, where); } \
  } while (0)

// ---- cases -----------------------------------------------------------------------------------------------------------------------
struct Case {
  const char* name;
  int plan, n, m, N, batch;
  bool ragged = false;
  std::vector<int> nxv, nuv;
  std::vector<AlDef> defs;
  std::vector<AlKnotBig> knots;
  std::vector<double> G;
  std::vector<std::vector<double>> g;
  Case(const char* name_, int plan_, int n_, int m_, int N_, int batch_) : name(name_), plan(plan_), n(n_), m(m_), N(N_), batch(batch_), knots((size_t)N_ + 1, AlKnotBig{}) {}
};
typedef std::vector<double> Mat;   // p x w, column-major
// what altro_hip_add_linear_constraint / _user_constraint leave on the host for one more block (w: columns of G as given)
static int add(Case& c, int k0, int k1, int cone, int p, int w, const Mat& G, bool per_problem, int user = 0) {
  const int id = (int)c.defs.size();
  c.defs.push_back(AlDef{cone, p, per_problem ? 1 : 0, (int)c.G.size(), 0, user, w});
  c.G.insert(c.G.end(), G.begin(), G.begin() + (size_t)p * w);
  std::vector<double> g((size_t)p * (per_problem ? c.batch : 1));
  for (size_t i = 0; i < g.size(); ++i) g[i] = 0.1 * (double)(i % (size_t)p + 1) + 0.01 * (double)(i / (size_t)p) + 0.3 * id;   // (no float holds these)
  c.g.push_back(g);
  for (int k = k0; k <= k1; ++k) c.knots[k].def[c.knots[k].ncon++] = id;
  return id;
}
static Mat dense(int p, int w) {   // every entry nonzero, none of size 1
  Mat G((size_t)p * w);
  for (int e = 0; e < w; ++e) for (int r = 0; r < p; ++r) G[r + (size_t)e * p] = 0.3 * (r + 1) - 0.7 * (e + 1) + 0.01 * r * e;
  return G;
}
// rows +e_c, -e_c for c = first .. first + count - 1, interleaved (row 2 i = +e, row 2 i + 1 = -e)
static Mat box(int first, int count, int w) {
  Mat G((size_t)2 * count * w, 0.0);
  for (int i = 0; i < count; ++i) { G[2 * i + (size_t)(first + i) * 2 * count] = 1.0; G[2 * i + 1 + (size_t)(first + i) * 2 * count] = -1.0; }
  return G;
}
// rows +e_0 .. +e_{n-1}, then -e_0 .. -e_{n-1}
static Mat state_box(int n, int w) {
  Mat G((size_t)2 * n * w, 0.0);
  for (int i = 0; i < n; ++i) { G[i + (size_t)i * 2 * n] = 1.0; G[n + i + (size_t)i * 2 * n] = -1.0; }
  return G;
}
static Mat pins(int p, int w) {   // rows e_0 .. e_{p-1}
  Mat G((size_t)p * w, 0.0);
  for (int i = 0; i < p; ++i) G[i + (size_t)i * p] = 1.0;
  return G;
}

static std::vector<Case> cases() {
  const int N = 5, B = 3;
  std::vector<Case> cs;
  {   // 1
    Case c("1 lane box + terminal", ALTRO_HIP_PLAN_LANE, 4, 2, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 4, 6, box(4, 2, 6), true);
    Mat T = pins(4, 6);
    T[2 + 2 * 4] = 0.0; T[2 + 1 * 4] = 2.0;   // third row: 2 e_1 -- its idx is recorded, the block is not bound-type
    add(c, N, N, CONE_EQUALITY, 4, 6, T, false);
    cs.push_back(c);
  }
  {   // 2
    Case c("2 lane soc + dense, not uniform", ALTRO_HIP_PLAN_LANE, 4, 2, N, B);
    add(c, 1, N - 1, CONE_SOC, 3, 6, dense(3, 6), false);
    add(c, 1, N - 1, CONE_INEQUALITY, 2, 6, dense(2, 6), false);
    cs.push_back(c);
  }
  {   // 3
    Case c("3 tile four slots", ALTRO_HIP_PLAN_MFMA16, 12, 4, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 8, 16, box(12, 4, 16), false);
    add(c, 0, N - 1, CONE_INEQUALITY, 24, 16, state_box(12, 16), false);
    add(c, N, N, CONE_EQUALITY, 12, 16, pins(12, 16), false);
    cs.push_back(c);
  }
  {   // 4
    Case c("4 tile padded (6, 2)", ALTRO_HIP_PLAN_MFMA16, 6, 2, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 5, 8, dense(5, 8), false);
    add(c, 0, N - 1, CONE_SOC, 4, 8, dense(4, 8), false);
    cs.push_back(c);
  }
  {   // 5
    Case c("5 tile user blocks", ALTRO_HIP_PLAN_MFMA16, 12, 4, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 11, 16, dense(11, 16), true);
    add(c, 0, N - 1, CONE_EQUALITY, 3, 16, Mat((size_t)3 * 16, 0.0), false, 1);
    add(c, 0, N - 1, CONE_INEQUALITY, 3, 16, Mat((size_t)3 * 16, 0.0), false, 2);
    add(c, N, N, CONE_EQUALITY, 2, 16, pins(2, 16), false);
    cs.push_back(c);
  }
  {   // 6a
    Case c("6a generic bounds", ALTRO_HIP_PLAN_GENERIC, 13, 4, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 8, 17, box(13, 4, 17), false);
    cs.push_back(c);
  }
  {   // 6b
    Case c("6b generic bounds + dense 40 + soc 9", ALTRO_HIP_PLAN_GENERIC, 13, 4, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 8, 17, box(13, 4, 17), false);
    add(c, 0, N, CONE_INEQUALITY, 40, 17, dense(40, 17), true);
    add(c, 2, 3, CONE_SOC, 9, 17, dense(9, 17), false);
    cs.push_back(c);
  }
  {   // 7
    Case c("7 generic user block", ALTRO_HIP_PLAN_GENERIC, 13, 4, N, B);
    add(c, 0, N - 1, CONE_INEQUALITY, 5, 17, Mat((size_t)5 * 17, 0.0), false, 3);
    add(c, 0, N, CONE_EQUALITY, 2, 17, pins(2, 17), false);
    cs.push_back(c);
  }
  {   // 8
    Case c("8 generic ragged", ALTRO_HIP_PLAN_GENERIC, 5, 3, 3, B);
    c.ragged = true; c.nxv = {3, 5, 4, 2}; c.nuv = {2, 1, 3};
    for (int k = 0; k < 3; ++k) add(c, k, k, k == 1 ? CONE_EQUALITY : CONE_INEQUALITY, 2 + k, c.nxv[k] + c.nuv[k], dense(2 + k, c.nxv[k] + c.nuv[k]), k == 2);
    add(c, 3, 3, CONE_EQUALITY, 2, 2, pins(2, 2), false);
    cs.push_back(c);
  }
  cs.push_back(Case("9 empty", ALTRO_HIP_PLAN_LANE, 4, 2, N, B));
  for (int rows2 : {8, 7}) {   // 10: 16 dual rows x 2^25 problems x 4 bytes = 2^31; one row fewer fits
    Case c(rows2 == 8 ? "10 lane window, 16 rows" : "10 lane window, 15 rows", ALTRO_HIP_PLAN_LANE, 4, 2, N, 1 << 25);
    add(c, N, N, CONE_INEQUALITY, 8, 6, state_box(4, 6), false);
    add(c, N, N, CONE_INEQUALITY, rows2, 6, dense(rows2, 6), false);
    cs.push_back(c);
  }
  return cs;
}

// ---- hashes: FNV-1a, 64 bits, over the values' bytes in little-endian order, field by field ----------------------------------------------
struct Fnv {
  unsigned long long h = 14695981039346656037ull;
  void bytes(unsigned long long v, int n) { for (int i = 0; i < n; ++i) { h ^= (v >> (8 * i)) & 0xffu; h *= 1099511628211ull; } }
  void i32(int v) { bytes((unsigned)v, 4); }
  void i64(int64_t v) { bytes((unsigned long long)v, 8); }
};
template <typename T>
static unsigned long long hash_pool(const std::vector<T>& v) {
  Fnv f;
  for (const T& x : v) { unsigned long long b = 0; std::memcpy(&b, &x, sizeof(T)); f.bytes(b, (int)sizeof(T)); }
  return f.h;
}
static unsigned long long hash_ints(const std::vector<int>& v) { Fnv f; for (int x : v) f.i32(x); return f.h; }
static unsigned long long hash_knots(const std::vector<AlKnot>& v) {
  Fnv f;
  for (const AlKnot& k : v) {
    f.i32(k.ncon);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.def[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.z_off[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.cone[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.p[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.g_per_problem[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.G_off[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i64(k.g_off[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.sel[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) for (int r = 0; r < AL_MAXP; ++r) f.i32(k.sidx[j][r]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.user[j]);
    for (int j = 0; j < AL_TILE_MAXC; ++j) f.i32(k.Gp_off[j]);
  }
  return f.h;
}
static unsigned long long hash_big(const std::vector<AlKnotBig>& v) {
  Fnv f;
  for (const AlKnotBig& k : v) {
    f.i32(k.ncon);
    for (int j = 0; j < GEN_MAXC; ++j) f.i32(k.def[j]);
    for (int j = 0; j < GEN_MAXC; ++j) f.i32(k.z_off[j]);
    for (int j = 0; j < GEN_MAXC; ++j) f.i32(k.cone[j]);
    for (int j = 0; j < GEN_MAXC; ++j) f.i32(k.p[j]);
    for (int j = 0; j < GEN_MAXC; ++j) f.i32(k.g_per_problem[j]);
    for (int j = 0; j < GEN_MAXC; ++j) f.i32(k.G_off[j]);
    for (int j = 0; j < GEN_MAXC; ++j) f.i64(k.g_off[j]);
  }
  return f.h;
}
// what is recorded of one case in one element type.  error: 0 none, 1 slot overflow, 2 plan LANE's 2 GiB window (then only rows is compared)
struct Rec {
  const char* name; int esz, error, rows;
  unsigned long long count[7];   // G, Gpad, g, knots, big, gsel, guser
  int sum[10];                   // all_sel, all_gsel, row32_ok, has_soc, has_user, max_ncon, uniform, rows_per_knot, G_count, Gpad_count
  unsigned long long hash[7];
};
// ---- end of cases ----------------------------------------------------------------------------------------------------------------

// The recordings: al_upload_typed<double> / <float> of the parent of the commit that introduced al_tables.h, its hipFree / dmalloc /
// hipMemcpy / hipMemsetAsync calls removed and its tables kept, run on cases() and printed in this form.  Case 9 (no blocks) is the
// default summary by decision (the parent returned early and left its fields as they were), cases 3 and 5 exist in fp64 only.
static const Rec recordings[] = {
  {"1 lane box + terminal", 8, 0, 24, {48, 0, 16, 6, 6, 0, 0}, {0, 0, 1, 0, 0, 1, 1, 4, 48, 0},
   {0x249740b48512c178ull, 0xcbf29ce484222325ull, 0xf62eb344ca22dc7eull, 0x715f6a806e8ff87dull, 0x8a1d5956e758d0d7ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"1 lane box + terminal", 4, 0, 24, {48, 0, 16, 6, 6, 0, 0}, {0, 0, 1, 0, 0, 1, 1, 4, 48, 0},
   {0xf9f7cb777905a458ull, 0xcbf29ce484222325ull, 0x1ce4383a68495d43ull, 0x715f6a806e8ff87dull, 0x8a1d5956e758d0d7ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"2 lane soc + dense, not uniform", 8, 0, 20, {30, 0, 5, 6, 6, 0, 0}, {0, 0, 0, 1, 0, 2, 0, 0, 30, 0},
   {0x30690496c226b6b5ull, 0xcbf29ce484222325ull, 0x98cecf9a1662e8a6ull, 0x063a223be1b9b271ull, 0xfa4697ed02a15c71ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"2 lane soc + dense, not uniform", 4, 0, 20, {30, 0, 5, 6, 6, 0, 0}, {0, 0, 0, 1, 0, 2, 0, 0, 30, 0},
   {0x25032c021d0cc7a3ull, 0xcbf29ce484222325ull, 0xe70955cbc18859d8ull, 0x063a223be1b9b271ull, 0xfa4697ed02a15c71ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"3 tile four slots", 8, 0, 172, {704, 972, 44, 6, 6, 0, 0}, {1, 0, 1, 0, 0, 4, 1, 32, 704, 972},
   {0xd1cc03d3e7b50665ull, 0x7158e28b32bc8ee5ull, 0x266be370df7b1f1full, 0xe2a7bb6b6eb092e7ull, 0x7a8464b10b7387b3ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"4 tile padded (6, 2)", 8, 0, 45, {144, 324, 9, 6, 6, 0, 0}, {0, 0, 0, 1, 0, 2, 1, 9, 144, 324},
   {0x5899918d89f2b8f1ull, 0x7e9e2520a7dc0c71ull, 0x8923dfe11f96940eull, 0x223705cb7fea3cc0ull, 0x46240c9dd7702be2ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"4 tile padded (6, 2)", 4, 0, 45, {144, 324, 9, 6, 6, 0, 0}, {0, 0, 0, 1, 0, 2, 1, 9, 144, 324},
   {0x53e3a37bf055c307ull, 0xd97fb5ae00d33a17ull, 0xf688d406ceef677bull, 0x223705cb7fea3cc0ull, 0x46240c9dd7702be2ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"5 tile user blocks", 8, 0, 87, {304, 486, 41, 6, 6, 0, 0}, {0, 0, 0, 0, 1, 4, 1, 17, 304, 486},
   {0xdc2127c1aff1507dull, 0x4f7ee4a953e6c379ull, 0x9b7dfa41f3c91934ull, 0x1bcbd394914d46eeull, 0xbf0f52b72ea4184aull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"6a generic bounds", 8, 0, 40, {136, 0, 8, 0, 6, 65, 0}, {0, 1, 1, 0, 0, 1, 1, 8, 136, 0},
   {0x91283c455b1c4ba5ull, 0xcbf29ce484222325ull, 0x8e7921a711941d46ull, 0xcbf29ce484222325ull, 0x25da2476af4aff6eull, 0x9c9c6bb9347d7938ull, 0xcbf29ce484222325ull}},
  {"6a generic bounds", 4, 0, 40, {136, 0, 8, 0, 6, 65, 0}, {0, 1, 1, 0, 0, 1, 1, 8, 136, 0},
   {0x77a54c87dd523665ull, 0xcbf29ce484222325ull, 0x42e1c7e30c253981ull, 0xcbf29ce484222325ull, 0x25da2476af4aff6eull, 0x9c9c6bb9347d7938ull, 0xcbf29ce484222325ull}},
  {"6b generic bounds + dense 40 + soc 9", 8, 0, 298, {969, 0, 137, 0, 6, 195, 0}, {0, 0, 0, 1, 0, 3, 0, 48, 969, 0},
   {0x6e77a74f548ec30eull, 0xcbf29ce484222325ull, 0x07ace7552e0670caull, 0xcbf29ce484222325ull, 0x9c85ce6662d32d88ull, 0xb5201265bf709038ull, 0xcbf29ce484222325ull}},
  {"6b generic bounds + dense 40 + soc 9", 4, 0, 298, {969, 0, 137, 0, 6, 195, 0}, {0, 0, 0, 1, 0, 3, 0, 48, 969, 0},
   {0x3506da9db2bb001bull, 0xcbf29ce484222325ull, 0x7550a81696bfc8e0ull, 0xcbf29ce484222325ull, 0x9c85ce6662d32d88ull, 0xb5201265bf709038ull, 0xcbf29ce484222325ull}},
  {"7 generic user block", 8, 0, 37, {119, 0, 7, 0, 6, 130, 2}, {0, 0, 0, 0, 1, 2, 1, 7, 119, 0},
   {0x3c763956df4507a5ull, 0xcbf29ce484222325ull, 0x02ce9ea98c89e1a2ull, 0xcbf29ce484222325ull, 0xec0fa2cc9da5c973ull, 0x661d24bfdcaaf617ull, 0xc7c2bf3b330983e6ull}},
  {"7 generic user block", 4, 0, 37, {119, 0, 7, 0, 6, 130, 2}, {0, 0, 0, 0, 1, 2, 1, 7, 119, 0},
   {0xe2025f13bc6a55e5ull, 0xcbf29ce484222325ull, 0xe285bcb370260f5aull, 0xcbf29ce484222325ull, 0xec0fa2cc9da5c973ull, 0x661d24bfdcaaf617ull, 0xc7c2bf3b330983e6ull}},
  {"8 generic ragged", 8, 0, 11, {60, 0, 19, 0, 4, 0, 0}, {0, 0, 1, 0, 0, 1, 0, 2, 60, 0},
   {0xa33e8d4f33826778ull, 0xcbf29ce484222325ull, 0xfa36b1c629254774ull, 0xcbf29ce484222325ull, 0x3b903a9199a01f85ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"8 generic ragged", 4, 0, 11, {60, 0, 19, 0, 4, 0, 0}, {0, 0, 1, 0, 0, 1, 0, 2, 60, 0},
   {0x38c20a7e9808a89aull, 0xcbf29ce484222325ull, 0x7e6163de7a922a46ull, 0xcbf29ce484222325ull, 0x3b903a9199a01f85ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"9 empty", 8, 0, 0, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
   {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"9 empty", 4, 0, 0, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
   {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"10 lane window, 16 rows", 8, 2, 16, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 2, 0, 0, 0, 0},
   {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"10 lane window, 16 rows", 4, 2, 16, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 2, 0, 0, 0, 0},
   {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"10 lane window, 15 rows", 8, 2, 15, {0, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 2, 0, 0, 0, 0},
   {0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
  {"10 lane window, 15 rows", 4, 0, 15, {90, 0, 15, 6, 6, 0, 0}, {0, 0, 1, 0, 0, 2, 0, 0, 90, 0},
   {0xf7e949629fb53374ull, 0xcbf29ce484222325ull, 0x9078f5aadd71e204ull, 0x8bf66ec804b7226cull, 0xcaa0b708147ec739ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull}},
};

static AlInput input_of(const Case& c, int esz) {
  return AlInput{c.plan, c.n, c.m, c.N, c.batch, (size_t)esz, c.ragged, c.nxv, c.nuv, c.defs, c.knots, c.G, c.g};
}
static const Case& case_named(const std::vector<Case>& cs, const char* name) {
  for (const Case& c : cs) if (!std::strcmp(c.name, name)) return c;
  std::printf("no case %s\n", name); std::exit(2);
}

static void against_recordings(const std::vector<Case>& cs) {
  size_t seen = 0;
  for (const Rec& r : recordings) {
    where = r.name;
    const Case& c = case_named(cs, r.name);
    const AlTables t = al_build(input_of(c, r.esz));
    ++seen;
    CHECK(t.error == r.error);
    CHECK(t.rows == r.rows);
    if (r.error) continue;
    const unsigned long long count[7] = {t.G.size(), t.Gpad.size(), t.g.size(), t.knots.size(), t.big.size(), t.gsel.size(), t.guser.size()};
    const int sum[10] = {t.sum.all_sel, t.sum.all_gsel, t.sum.row32_ok, t.sum.has_soc, t.sum.has_user, t.sum.max_ncon, t.sum.uniform, t.sum.rows_per_knot,
                         t.sum.G_count, t.sum.Gpad_count};
    unsigned long long hash[7];
    if (r.esz == 8) { hash[0] = hash_pool(t.G); hash[1] = hash_pool(t.Gpad); hash[2] = hash_pool(t.g); }
    else { hash[0] = hash_pool(al_pool_as<float>(t.G)); hash[1] = hash_pool(al_pool_as<float>(t.Gpad)); hash[2] = hash_pool(al_pool_as<float>(t.g)); }
    hash[3] = hash_knots(t.knots); hash[4] = hash_big(t.big); hash[5] = hash_ints(t.gsel); hash[6] = hash_ints(t.guser);
    for (int i = 0; i < 7; ++i) {
      if (count[i] != r.count[i]) { ++failures; std::printf("%s esz %d: table %d has %llu elements, recorded %llu\n", r.name, r.esz, i, count[i], r.count[i]); }
      if (hash[i] != r.hash[i]) { ++failures; std::printf("%s esz %d: table %d hashes to %016llx, recorded %016llx\n", r.name, r.esz, i, hash[i], r.hash[i]); }
    }
    for (int i = 0; i < 10; ++i)
      if (sum[i] != r.sum[i]) { ++failures; std::printf("%s esz %d: summary value %d is %d, recorded %d\n", r.name, r.esz, i, sum[i], r.sum[i]); }
  }
  where = "recordings";
  CHECK(seen == 2 * cs.size() - 2);   // every case in both element types, cases 3 and 5 in fp64 only
}

// (b) kernels/al_types.h: a slot is at most AL_MAXP = 8 rows, a row-wise block takes consecutive slots with its duals in place, a
// second-order cone one; every slot is its own ps x 16 matrix in the tile's column order (states 0..11, inputs 12..15) in G and one
// [9][AL_GP_LD = 18] entry of AL_GP_DEF = 162 elements in Gpad; sidx = +-(column + 1)
static void by_hand(const std::vector<Case>& cs) {
  {
    where = "3 by hand";
    const Case& c = case_named(cs, "3 tile four slots");
    const AlTables t = al_build(input_of(c, 8));
    CHECK(t.error == 0 && t.rows == 5 * 32 + 12 && t.knots.size() == 6 && t.G.size() == 5 * 128 + 64 && t.Gpad.size() == 6 * 162);
    CHECK(t.sum.uniform == 1 && t.sum.rows_per_knot == 32 && t.sum.max_ncon == 4 && t.sum.all_sel == 1 && t.sum.has_soc == 0);
    for (int k = 0; k < 5; ++k) {   // the input box, then the state box's three slots
      const AlKnot& kn = t.knots[k];
      CHECK(kn.ncon == 4);
      const int def[4] = {0, 1, 1, 1};
      for (int s = 0; s < 4; ++s) {
        CHECK(kn.def[s] == def[s] && kn.z_off[s] == 32 * k + 8 * s && kn.p[s] == 8 && kn.G_off[s] == 128 * s && kn.Gp_off[s] == 162 * s);
        CHECK(kn.sel[s] == 1 && kn.cone[s] == CONE_INEQUALITY && kn.user[s] == 0 && kn.g_off[s] == (s == 0 ? 0 : 8 + 8 * (s - 1)));
      }
      const int box_sidx[8] = {13, -13, 14, -14, 15, -15, 16, -16};
      for (int r = 0; r < 8; ++r) CHECK(kn.sidx[0][r] == box_sidx[r]);
      for (int r = 0; r < 8; ++r) CHECK(kn.sidx[1][r] == r + 1 && kn.sidx[2][r] == (r < 4 ? 8 + r + 1 : -(r - 4 + 1)) && kn.sidx[3][r] == -(4 + r + 1));
      CHECK(t.big[k].ncon == 2 && t.big[k].z_off[0] == 32 * k && t.big[k].z_off[1] == 32 * k + 8 && t.big[k].G_off[0] == 0 && t.big[k].G_off[1] == 128);
    }
    const AlKnot& kN = t.knots[5];   // the terminal equality: twelve rows, slots of 8 and 4
    CHECK(kN.ncon == 2 && kN.def[0] == 2 && kN.def[1] == 2 && kN.z_off[0] == 160 && kN.z_off[1] == 168 && kN.p[0] == 8 && kN.p[1] == 4);
    CHECK(kN.G_off[0] == 512 && kN.G_off[1] == 640 && kN.Gp_off[0] == 4 * 162 && kN.Gp_off[1] == 5 * 162 && kN.g_off[0] == 32 && kN.g_off[1] == 40);
    CHECK(t.big[5].ncon == 1 && t.big[5].G_off[0] == 512 && t.big[5].z_off[0] == 160 && t.big[5].p[0] == 12);
    // row 3 of the input box is -e_u1 (tile column 13); row 12 of the state box is -e_0: slot 2 of the handle, its row 4; row 10 of the
    // terminal block is +e_10: slot 5, its row 2 (a slot of four rows)
    CHECK(t.G[0 + 3 + 13 * 8] == -1.0 && t.Gpad[0 * 162 + 3 * 18 + 13] == -1.0);
    CHECK(t.G[256 + 4 + 0 * 8] == -1.0 && t.Gpad[2 * 162 + 4 * 18 + 0] == -1.0);
    CHECK(t.G[640 + 2 + 10 * 4] == 1.0 && t.Gpad[5 * 162 + 2 * 18 + 10] == 1.0);
    double nz = 0, nzp = 0;
    for (double v : t.G) nz += v != 0.0;
    for (double v : t.Gpad) nzp += v != 0.0;
    CHECK(nz == 8 + 24 + 12 && nzp == 8 + 24 + 12);
  }
  {
    where = "4 by hand";
    const Case& c = case_named(cs, "4 tile padded (6, 2)");
    const AlTables t = al_build(input_of(c, 8));
    const Mat D = dense(5, 8), S = dense(4, 8);
    CHECK(t.error == 0 && t.rows == 45 && t.G.size() == 5 * 16 + 4 * 16 && t.Gpad.size() == 2 * 162);
    CHECK(t.sum.uniform == 1 && t.sum.rows_per_knot == 9 && t.sum.max_ncon == 2 && t.sum.all_sel == 0 && t.sum.has_soc == 1);
    for (int k = 0; k < 5; ++k) {
      const AlKnot& kn = t.knots[k];
      CHECK(kn.ncon == 2 && kn.def[0] == 0 && kn.def[1] == 1 && kn.z_off[0] == 9 * k && kn.z_off[1] == 9 * k + 5 && kn.p[0] == 5 && kn.p[1] == 4);
      CHECK(kn.G_off[0] == 0 && kn.G_off[1] == 80 && kn.Gp_off[0] == 0 && kn.Gp_off[1] == 162 && kn.sel[0] == 0 && kn.sel[1] == 0 && kn.cone[1] == CONE_SOC);
      for (int r = 0; r < 8; ++r) CHECK(kn.sidx[0][r] == 0 && kn.sidx[1][r] == 0);
    }
    CHECK(t.knots[5].ncon == 0);
    // the inputs are columns 6 and 7 of the caller's G and tile columns 12 and 13; tile columns 6..11 and 14, 15 stay zero
    CHECK(t.G[0 + 2 + 12 * 5] == D[2 + 6 * 5] && t.Gpad[0 + 2 * 18 + 12] == D[2 + 6 * 5]);
    CHECK(t.G[0 + 4 + 13 * 5] == D[4 + 7 * 5] && t.Gpad[0 + 4 * 18 + 13] == D[4 + 7 * 5]);
    CHECK(t.G[80 + 1 + 3 * 4] == S[1 + 3 * 4] && t.Gpad[162 + 1 * 18 + 3] == S[1 + 3 * 4]);
    CHECK(t.G[80 + 3 + 12 * 4] == S[3 + 6 * 4] && t.Gpad[162 + 3 * 18 + 12] == S[3 + 6 * 4]);
    for (int col : {6, 7, 8, 9, 10, 11, 14, 15})
      for (int r = 0; r < 5; ++r) CHECK(t.G[r + col * 5] == 0.0 && t.Gpad[r * 18 + col] == 0.0);
  }
}

// (c) the capacities.  A handle under construction: blocks are added through al_admit, as the C ABI adds them.
static AlAdmit admit(Case& c, int esz, int k0, int k1, int cone, int p, int user = 0) {
  const AlAdmit a = al_admit(input_of(c, esz), k0, k1, cone, p, user);
  if (a.limit == AL_ADMIT_OK) add(c, k0, k1, cone, p, a.w, Mat((size_t)p * a.w, 0.0), false, user);
  return a;
}
static void capacities() {
  const int N = 5;
  const int INEQ = CONE_INEQUALITY, SOC = CONE_SOC;
  {
    where = "admit: plan LANE";
    Case c("", ALTRO_HIP_PLAN_LANE, 4, 2, N, 3);
    AlAdmit a = admit(c, 8, 0, 0, INEQ, 9);
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 8);
    CHECK(admit(c, 8, 0, 0, INEQ, 0).limit == AL_LIMIT_ROWS);
    a = admit(c, 8, 0, 0, SOC, 5);
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 4);
    CHECK(admit(c, 8, 0, 0, 4, 1).limit == AL_LIMIT_CONE && admit(c, 8, 0, 0, -1, 1).limit == AL_LIMIT_CONE);
    CHECK(admit(c, 8, -1, 0, INEQ, 1).limit == AL_LIMIT_RANGE && admit(c, 8, 0, N + 1, INEQ, 1).limit == AL_LIMIT_RANGE && admit(c, 8, 2, 1, INEQ, 1).limit == AL_LIMIT_RANGE);
    a = admit(c, 8, 0, N, INEQ, 8);
    CHECK(a.limit == AL_ADMIT_OK && a.w == 6);
    CHECK(admit(c, 8, 0, 2, SOC, 4).limit == AL_ADMIT_OK);
    a = admit(c, 8, 1, 3, INEQ, 1);   // two blocks per knot point: k = 1 and 2 are full
    CHECK(a.limit == AL_LIMIT_KNOT && a.cmax == 2 && a.k == 1 && a.count == 3);
    for (int i = 2; i < 16; ++i) CHECK(admit(c, 4, 3 + i % 3, 3 + i % 3, INEQ, 1).limit == (i < 5 ? AL_ADMIT_OK : AL_LIMIT_KNOT));
    // sixteen blocks per handle (five so far; knot points hold two, so the rest of a second handle goes one per knot point and pair)
    Case d("", ALTRO_HIP_PLAN_LANE, 4, 2, 8, 3);
    for (int i = 0; i < 16; ++i) CHECK(admit(d, 8, i / 2, i / 2, INEQ, 1).limit == AL_ADMIT_OK);
    a = admit(d, 8, 8, 8, INEQ, 1);
    CHECK(a.limit == AL_LIMIT_DEFS && a.dmax == 16 && a.count == 17);
    // a block from source has no limits of its own on plan LANE
    Case e("", ALTRO_HIP_PLAN_LANE, 4, 2, N, 3);
    CHECK(admit(e, 8, 0, 0, INEQ, 8, 1).limit == AL_ADMIT_OK && admit(e, 8, 0, 0, INEQ, 9, 2).limit == AL_LIMIT_ROWS);
  }
  {
    where = "admit: plan GENERIC";
    Case c("", ALTRO_HIP_PLAN_GENERIC, 13, 4, N, 3);
    AlAdmit a = admit(c, 8, 0, 0, INEQ, 65);
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 64);
    a = admit(c, 8, 0, 0, SOC, 33);
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 32);
    a = admit(c, 8, 0, 0, INEQ, 64);
    CHECK(a.limit == AL_ADMIT_OK && a.w == 17);
    CHECK(admit(c, 8, 0, 0, SOC, 32).limit == AL_ADMIT_OK);
    for (int i = 2; i < 8; ++i) CHECK(admit(c, 8, 0, 1, INEQ, 1).limit == AL_ADMIT_OK);
    a = admit(c, 8, 0, 1, INEQ, 1);   // eight blocks per knot point
    CHECK(a.limit == AL_LIMIT_KNOT && a.cmax == 8 && a.k == 0 && a.count == 9);
    a = admit(c, 8, 1, 2, INEQ, 1);   // k = 1 has six
    CHECK(a.limit == AL_ADMIT_OK);
    CHECK(admit(c, 8, 1, 1, INEQ, 1).limit == AL_ADMIT_OK && admit(c, 8, 1, 1, INEQ, 1).limit == AL_LIMIT_KNOT);
    // sixty-four blocks per handle
    Case d("", ALTRO_HIP_PLAN_GENERIC, 13, 4, 8, 3);
    for (int i = 0; i < 64; ++i) CHECK(admit(d, 4, i / 8, i / 8, INEQ, 1).limit == AL_ADMIT_OK);
    a = admit(d, 4, 8, 8, INEQ, 1);
    CHECK(a.limit == AL_LIMIT_DEFS && a.dmax == 64 && a.count == 65);
    // blocks from source: 32 rows a block, 32 rows a knot point
    Case e("", ALTRO_HIP_PLAN_GENERIC, 13, 4, N, 3);
    a = admit(e, 8, 0, 0, INEQ, 33, 1);
    CHECK(a.limit == AL_LIMIT_USER_ROWS && a.pmax == 32);
    CHECK(admit(e, 8, 0, 0, INEQ, 0, 1).limit == AL_LIMIT_USER_ROWS);
    CHECK(admit(e, 8, -3, 99, 7, 33, 1).limit == AL_LIMIT_USER_ROWS);   // (the block's own rows are looked at before the cone and the range)
    CHECK(admit(e, 8, 0, 0, 7, 3, 1).limit == AL_LIMIT_CONE);
    CHECK(admit(e, 8, 0, 3, INEQ, 20, 1).limit == AL_ADMIT_OK && admit(e, 8, 2, 4, INEQ, 12, 2).limit == AL_ADMIT_OK);
    CHECK(admit(e, 8, 0, N, INEQ, 40, 0).limit == AL_ADMIT_OK);   // (rows of a data block do not count)
    a = admit(e, 8, 0, N, INEQ, 1, 3);
    CHECK(a.limit == AL_LIMIT_USER_KNOT && a.cmax == 32 && a.k == 2 && a.count == 33);
    CHECK(admit(e, 8, 0, 1, INEQ, 12, 3).limit == AL_ADMIT_OK);
    a = admit(e, 8, -2, 0, INEQ, 1, 4);   // (the range is clamped here and refused afterwards)
    CHECK(a.limit == AL_LIMIT_USER_KNOT && a.k == 0 && a.count == 33);
    CHECK(admit(e, 8, -2, -1, INEQ, 1, 4).limit == AL_LIMIT_RANGE);
  }
  {
    where = "admit: plan GENERIC, per-knot-point dimensions";
    Case c("", ALTRO_HIP_PLAN_GENERIC, 5, 3, 4, 3);
    c.ragged = true; c.nxv = {3, 3, 4, 2, 2}; c.nuv = {2, 2, 3, 1};
    AlAdmit a = admit(c, 8, 0, 1, INEQ, 2);
    CHECK(a.limit == AL_ADMIT_OK && a.w == 5);
    a = admit(c, 8, 0, 2, INEQ, 2);
    CHECK(a.limit == AL_LIMIT_RAGGED && a.k == 2);
    a = admit(c, 8, 3, 4, INEQ, 2);   // same nx, but the terminal knot point has no input
    CHECK(a.limit == AL_ADMIT_OK && a.w == 3);
    a = admit(c, 8, 4, 4, INEQ, 2);
    CHECK(a.limit == AL_ADMIT_OK && a.w == 2);
    c.nuv[3] = 0;
    CHECK(admit(c, 8, 3, 4, INEQ, 2).limit == AL_ADMIT_OK);
    c.nxv[4] = 3;
    a = admit(c, 8, 3, 4, INEQ, 2);
    CHECK(a.limit == AL_LIMIT_RAGGED && a.k == 4);
  }
  {
    where = "admit: plan MFMA16 fp64";
    Case c("", ALTRO_HIP_PLAN_MFMA16, 12, 4, N, 3);
    AlAdmit a = admit(c, 8, 0, 0, INEQ, 49);
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 48);
    a = admit(c, 8, 0, 0, SOC, 5);
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 4);
    a = admit(c, 8, 0, 0, INEQ, 48);   // six slots
    CHECK(a.limit == AL_ADMIT_OK && a.w == 16);
    a = admit(c, 8, 0, 1, SOC, 1);
    CHECK(a.limit == AL_LIMIT_KNOT && a.cmax == 6 && a.k == 0 && a.count == 7);
    CHECK(admit(c, 8, 1, 1, INEQ, 33).limit == AL_ADMIT_OK && admit(c, 8, 1, 1, SOC, 4).limit == AL_ADMIT_OK);   // five slots and one
    a = admit(c, 8, 1, 2, INEQ, 8);
    CHECK(a.limit == AL_LIMIT_KNOT && a.k == 1 && a.count == 7);
    // thirty-two slots per handle: 6 + 5 + 1 so far, 6 + 6 + 6 more, then 2 of a block of 3 do not fit
    for (int k = 2; k < 5; ++k) CHECK(admit(c, 8, k, k, INEQ, 41).limit == AL_ADMIT_OK);
    a = admit(c, 8, 5, 5, INEQ, 17);
    CHECK(a.limit == AL_LIMIT_DEFS && a.dmax == 32 && a.count == 33);
    CHECK(admit(c, 8, 5, 5, INEQ, 16).limit == AL_ADMIT_OK);
    a = admit(c, 8, 5, 5, SOC, 1);
    CHECK(a.limit == AL_LIMIT_DEFS && a.count == 33);
    // ... of which blocks from source take none; two of them per knot point, one slot each
    CHECK(admit(c, 8, 5, 5, INEQ, 8, 1).limit == AL_ADMIT_OK && admit(c, 8, 5, 5, SOC, 4, 2).limit == AL_ADMIT_OK);
    a = admit(c, 8, 4, 5, INEQ, 1, 3);
    CHECK(a.limit == AL_LIMIT_USER_KNOT && a.cmax == 2 && a.k == 5 && a.count == 3);
    a = admit(c, 8, 0, 0, INEQ, 9, 3);
    CHECK(a.limit == AL_LIMIT_USER_ROWS && a.pmax == 8);
    a = admit(c, 8, 0, 0, SOC, 5, 3);
    CHECK(a.limit == AL_LIMIT_USER_ROWS && a.pmax == 4);
    CHECK(admit(c, 8, 0, 0, 9, 1, 3).limit == AL_LIMIT_USER_CONE);
    a = admit(c, 8, 0, 0, INEQ, 1, 3);   // (one of the six slots like any other block)
    CHECK(a.limit == AL_LIMIT_KNOT && a.k == 0 && a.count == 7);
  }
  {
    where = "admit: plan MFMA16 fp32";
    Case c("", ALTRO_HIP_PLAN_MFMA16, 12, 4, N, 3);
    AlAdmit a = admit(c, 4, 0, 0, INEQ, 17);   // the two-slot kernels only
    CHECK(a.limit == AL_LIMIT_ROWS && a.pmax == 16);
    CHECK(admit(c, 4, 0, 0, INEQ, 16).limit == AL_ADMIT_OK);
    a = admit(c, 4, 0, 1, INEQ, 1);
    CHECK(a.limit == AL_LIMIT_KNOT && a.cmax == 2 && a.k == 0 && a.count == 3);
    CHECK(admit(c, 4, 1, 1, INEQ, 8).limit == AL_ADMIT_OK && admit(c, 4, 1, 1, SOC, 4).limit == AL_ADMIT_OK);
    CHECK(admit(c, 4, 1, 1, SOC, 1).limit == AL_LIMIT_KNOT);
  }
  where = "slots";
  CHECK(al_slots(true, INEQ, 1) == 1 && al_slots(true, INEQ, 8) == 1 && al_slots(true, INEQ, 9) == 2 && al_slots(true, INEQ, 48) == 6 && al_slots(true, SOC, 4) == 1);
  CHECK(al_slots(false, INEQ, 64) == 1 && al_slots(false, SOC, 32) == 1);
  CHECK(al_slot_rows(true, INEQ, 11, 0) == 8 && al_slot_rows(true, INEQ, 11, 1) == 3 && al_slot_rows(true, SOC, 4, 0) == 4 && al_slot_rows(false, INEQ, 40, 0) == 40);
}

int main() {
  const std::vector<Case> cs = cases();
  against_recordings(cs);
  by_hand(cs);
  capacities();
  if (failures) { std::printf("al_tables_test: %d failures\n", failures); return 1; }
  std::printf("al_tables_test ok\n");
  return 0;
}
