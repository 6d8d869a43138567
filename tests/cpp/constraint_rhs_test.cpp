// Constraint right-hand sides through device pointers (altro_hip_set_pointer_mode) and the C++ wrapper's AddLinearConstraintRhs /
// SetConstraintRhs / GetConstraintRhs / ShiftConstraintRhs: a device-mode write followed by the getter must equal the host-mode write of
// the same array, on an fp64 and an fp32 handle, per problem and shared, whole range and sub-range; and after a device-mode write and a
// shift, one more block (which rebuilds the tables) must leave the getter returning the updated values.  Needs an MI355X.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "altro_hip/altro_hip.hpp"

using altro::hip::BatchSolver;

static int failures = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) { ++failures; std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)
#define HIP_OK(call)                                                                        \
  do {                                                                                      \
    if ((call) != hipSuccess) { std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #call); return 1; } \
  } while (0)

constexpr int N = 20, n = 4, m = 2, batch = 70, p = 3, k0 = 2, k1 = 18, K = k1 - k0 + 1;

static double value(int salt, size_t i) { return 0.001 * (double)((i * 2654435761u + salt * 97u) % 100003u) - 50.0 + 1.0 / 3.0; }

// every knot point of block `id` as [nb][K][p]
static std::vector<double> read_all(BatchSolver& s, int id, int nb) {
  std::vector<double> all((size_t)nb * K * p), at((size_t)nb * p);
  for (int k = k0; k <= k1; ++k) {
    s.GetConstraintRhs(id, k, at.data());
    for (int b = 0; b < nb; ++b)
      for (int r = 0; r < p; ++r) all[((size_t)b * K + (k - k0)) * p + r] = at[(size_t)b * p + r];
  }
  return all;
}

static int run(int dtype) {
  std::vector<double> G((size_t)p * (n + m));
  for (size_t i = 0; i < G.size(); ++i) G[i] = value(1, i);
  BatchSolver host(N, n, m, batch, static_cast<altro_hip_dtype>(dtype)), dev(N, n, m, batch, static_cast<altro_hip_dtype>(dtype));
  for (int layout : {(int)ALTRO_HIP_RHS_PER_KNOT | (int)ALTRO_HIP_RHS_PER_PROBLEM, (int)ALTRO_HIP_RHS_PER_KNOT}) {
    const int nb = (layout & ALTRO_HIP_RHS_PER_PROBLEM) ? batch : 1;
    std::vector<double> g0((size_t)nb * K * p);
    for (size_t i = 0; i < g0.size(); ++i) g0[i] = value(2 + layout, i);
    const int id = host.AddLinearConstraintRhs(k0, k1, altro::hip::Cone::Inequality, p, G.data(), g0.data(), layout);
    CHECK(dev.AddLinearConstraintRhs(k0, k1, altro::hip::Cone::Inequality, p, G.data(), g0.data(), layout) == id);
    // the whole range, then knot points 5 .. 11
    for (int part = 0; part < 2; ++part) {
      const int a = part ? 5 : -1, b = part ? 11 : -1, nk = part ? 7 : K;
      std::vector<double> g((size_t)nb * nk * p);
      for (size_t i = 0; i < g.size(); ++i) g[i] = value(10 + part + layout, i);
      host.SetConstraintRhs(id, g.data(), a, b);
      double* d = nullptr;
      HIP_OK(hipMalloc((void**)&d, g.size() * sizeof(double)));
      HIP_OK(hipMemcpy(d, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
      if (altro_hip_set_pointer_mode(dev.Handle(), 1)) return 1;
      dev.SetConstraintRhs(id, d, a, b);
      if (altro_hip_set_pointer_mode(dev.Handle(), 0)) return 1;
      HIP_OK(hipFree(d));
      const std::vector<double> want = read_all(host, id, nb), got = read_all(dev, id, nb);
      CHECK(want == got);
      if (part) {   // ... and they are the values given, as the handle's element type holds them
        for (int bb = 0; bb < nb; ++bb)
          for (int c = 0; c < nk * p; ++c) {
            const double v = g[(size_t)bb * nk * p + c];
            CHECK(got[((size_t)bb * K + (a - k0)) * p + c] == (dtype == ALTRO_HIP_F64 ? v : (double)(float)v));
          }
      }
    }
  }
  // the device is ahead of the host description (a device-mode write, then a shift): one more block rebuilds the tables from the
  // values the device holds
  const std::vector<double> before0 = read_all(dev, 0, batch), before1 = read_all(dev, 1, 1);
  dev.ShiftConstraintRhs();
  std::vector<double> one((size_t)p, 0.25);
  CHECK(dev.AddLinearConstraintRhs(0, 1, altro::hip::Cone::Inequality, p, G.data(), one.data(), 0) == 2);
  const std::vector<double> after0 = read_all(dev, 0, batch), after1 = read_all(dev, 1, 1);
  for (int id = 0; id < 2; ++id) {
    const int nb = id ? 1 : batch;
    const std::vector<double>&before = id ? before1 : before0, &after = id ? after1 : after0;
    for (int b = 0; b < nb; ++b)
      for (int kk = 0; kk < K; ++kk)
        for (int r = 0; r < p; ++r)
          CHECK(after[((size_t)b * K + kk) * p + r] == before[((size_t)b * K + (kk + 1 < K ? kk + 1 : kk)) * p + r]);
  }
  double z[3];
  dev.GetConstraintRhs(2, 1, z);
  CHECK(z[0] == 0.25 && z[2] == 0.25);
  // a device-mode write and then one more block, with NO shift in between: the write alone must mark the host description stale,
  // on a per-knot block (knot points 5 .. 11 of it) and on an old-style block (which the shift never touches)
  BatchSolver st(N, n, m, batch, static_cast<altro_hip_dtype>(dtype));
  std::vector<double> ga((size_t)batch * K * p), gb((size_t)batch * p), na((size_t)batch * 7 * p), nb_((size_t)batch * p);
  for (size_t i = 0; i < ga.size(); ++i) ga[i] = value(31, i);
  for (size_t i = 0; i < gb.size(); ++i) gb[i] = value(32, i);
  for (size_t i = 0; i < na.size(); ++i) na[i] = value(33, i);
  for (size_t i = 0; i < nb_.size(); ++i) nb_[i] = value(34, i);
  CHECK(st.AddLinearConstraintRhs(k0, k1, altro::hip::Cone::Inequality, p, G.data(), ga.data(), ALTRO_HIP_RHS_PER_KNOT | ALTRO_HIP_RHS_PER_PROBLEM) == 0);
  CHECK(st.SetConstraint(0, 1, altro::hip::Cone::Inequality, p, G.data(), gb.data(), true) == 1);
  double *da = nullptr, *db = nullptr;
  HIP_OK(hipMalloc((void**)&da, na.size() * sizeof(double)));
  HIP_OK(hipMalloc((void**)&db, nb_.size() * sizeof(double)));
  HIP_OK(hipMemcpy(da, na.data(), na.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db, nb_.data(), nb_.size() * sizeof(double), hipMemcpyHostToDevice));
  if (altro_hip_set_pointer_mode(st.Handle(), 1)) return 1;
  st.SetConstraintRhs(0, da, 5, 11);
  st.SetConstraintRhs(1, db);
  if (altro_hip_set_pointer_mode(st.Handle(), 0)) return 1;
  HIP_OK(hipFree(da)); HIP_OK(hipFree(db));
  CHECK(st.AddLinearConstraintRhs(19, 20, altro::hip::Cone::Inequality, p, G.data(), one.data(), 0) == 2);   // the tables are rebuilt
  auto held = [&](double v) { return dtype == ALTRO_HIP_F64 ? v : (double)(float)v; };
  const std::vector<double> ra = read_all(st, 0, batch);
  std::vector<double> rb((size_t)batch * p);
  for (int k = 0; k <= 1; ++k) {
    st.GetConstraintRhs(1, k, rb.data());
    for (size_t i = 0; i < rb.size(); ++i) CHECK(rb[i] == held(nb_[i]));
  }
  for (int b = 0; b < batch; ++b)
    for (int kk = 0; kk < K; ++kk)
      for (int r = 0; r < p; ++r) {
        const int k = k0 + kk;
        const double want = (k >= 5 && k <= 11) ? na[((size_t)b * 7 + (k - 5)) * p + r] : ga[((size_t)b * K + kk) * p + r];
        CHECK(ra[((size_t)b * K + kk) * p + r] == held(want));
      }
  return 0;
}

int main() {
  try {
    if (run(ALTRO_HIP_F64) || run(ALTRO_HIP_F32)) { std::printf("FAILED (HIP call)\n"); return 1; }
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  if (failures) { std::printf("constraint_rhs_test: %d failure(s)\n", failures); return 1; }
  std::printf("constraint_rhs_test OK\n");
  return 0;
}
