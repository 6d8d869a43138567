// BatchSolver::SetModelSource(source, h, num_params) / SetModelParams / GetModelParams (include/altro_hip/altro_hip.hpp): plan LANE's
// test vehicle, the kinematic bicycle from source with its wheel base and CoG offset as two per-problem parameters, 70 vehicles that all differ.
// The wrapper's rollout equals, bit for bit, the one the C ABI gives for the same calls; the parameters come back as set; and a vehicle
// with another wheel base rolls out differently.  Prints "OK" and returns 0 when everything holds; needs an MI355X.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "altro_hip/altro_hip.h"
#include "altro_hip/altro_hip.hpp"

static int failures = 0;
#define EXPECT(cond)                                                                         \
  do {                                                                                       \
    if (!(cond)) { std::printf("  EXPECT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static const char* kBicycle = R"SRC(
template <typename T> struct BikeTrig { T st, ct, sb, cb, sd, cd, td, dbeta; };
template <typename T> __device__ BikeTrig<T> bike_trig(const T* x, const T* p) {
  BikeTrig<T> t;
  const T L = p[0], lr = p[1];
  const T sth = sin(x[2]), cth = cos(x[2]);
  t.sd = sin(x[3]); t.cd = cos(x[3]);
  t.td = t.sd / t.cd;
  const T by = lr * x[3], bx = L;
  const T r2 = bx * bx + by * by;
  const T ir = T(1) / sqrt(r2);
  t.cb = bx * ir; t.sb = by * ir;
  t.dbeta = bx / r2 * lr;
  t.st = sth * t.cb + cth * t.sb;
  t.ct = cth * t.cb - sth * t.sb;
  return t;
}
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, const T* p, T* xdot) {
  const BikeTrig<T> t = bike_trig<T>(x, p);
  xdot[0] = u[0] * t.ct; xdot[1] = u[0] * t.st; xdot[2] = u[0] * t.cb * t.td / p[0]; xdot[3] = u[1];
}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, const T* p, T* J) {
  const BikeTrig<T> t = bike_trig<T>(x, p);
  const T v = u[0], L = p[0];
  for (int e = 0; e < 24; ++e) J[e] = T(0);
  J[0 + 2 * 4] = v * -t.st; J[0 + 3 * 4] = v * (-t.st * t.dbeta); J[0 + 4 * 4] = t.ct;
  J[1 + 2 * 4] = v * t.ct;  J[1 + 3 * 4] = v * (t.ct * t.dbeta);  J[1 + 4 * 4] = t.st;
  J[2 + 3 * 4] = v / L * (-t.sb * t.td * t.dbeta + t.cb / (t.cd * t.cd)); J[2 + 4 * 4] = t.cb * t.td / L;
  J[3 + 5 * 4] = T(1);
}
)SRC";

int main() {
  const int N = 20, n = 4, m = 2, batch = 70, P = 2;
  const float h = 0.05f;
  std::vector<double> theta((size_t)batch * P), x0((size_t)batch * n), u((size_t)batch * N * m);
  for (int b = 0; b < batch; ++b) {
    theta[(size_t)b * P] = 2.0 + 1.4 * b / (batch - 1);
    theta[(size_t)b * P + 1] = theta[(size_t)b * P] * (0.35 + 0.3 * ((b * 37) % batch) / (double)batch);
    for (int i = 0; i < n; ++i) x0[(size_t)b * n + i] = 0.02 * ((b * 4 + i) % 7 - 3);
    for (int k = 0; k < N; ++k) { u[((size_t)b * N + k) * m] = 0.8 + 0.01 * ((b + k) % 11); u[((size_t)b * N + k) * m + 1] = 0.05 * ((b + 3 * k) % 9 - 4); }
  }
  const double Qd[2 * 4] = {0.1, 0.1, 0.1, 0.1, 1, 1, 1, 1}, Rd[2] = {0.1, 0.1}, xref[2 * 4] = {1, 0.5, 0.3, 0, 1, 0.5, 0.3, 0}, uref[2] = {0, 0};
  const size_t nx = (size_t)batch * (N + 1) * n;
  std::vector<double> x_wrap(nx), x_capi(nx), x_other(nx), got((size_t)batch * P, -1.0);
  int plan_wrap = -1;

  std::printf("[batch wrapper] SetModelSource(source, h, num_params) / SetModelParams / GetModelParams\n");
  try {
    altro::hip::BatchSolver bs(N, n, m, batch);
    plan_wrap = bs.GetPlan();
    EXPECT(plan_wrap == ALTRO_HIP_PLAN_LANE);              // (what ALTRO_HIP_PLAN_AUTO gives 70 problems of (4, 2))
    bs.SetModelSource(kBicycle, h, P);
    EXPECT(bs.ModelNumParams() == P);
    bool threw = false;
    try { bs.GetModelParams(got.data()); } catch (const std::exception&) { threw = true; }
    EXPECT(threw);                                        // nothing is stored before the setter
    bs.SetModelParams(theta.data());
    bs.GetModelParams(got.data());
    EXPECT(got == theta);
    EXPECT(altro_hip_set_tracking_cost(bs.Handle(), Qd, Rd, xref, uref, 1, 1) == 0);
    bs.SetInitialState(x0.data());
    EXPECT(altro_hip_set_input_guess(bs.Handle(), u.data(), 0, 0) == 0);
    EXPECT(altro_hip_open_loop_rollout(bs.Handle()) == 0);
    EXPECT(altro_hip_get_x(bs.Handle(), x_wrap.data()) == 0);
    // one set for every problem: vehicle 0's -- its own rollout stays, the others' move
    bs.SetModelParams(theta.data(), true);
    EXPECT(altro_hip_open_loop_rollout(bs.Handle()) == 0);
    EXPECT(altro_hip_get_x(bs.Handle(), x_other.data()) == 0);
    EXPECT(std::memcmp(x_other.data(), x_wrap.data(), (size_t)(N + 1) * n * sizeof(double)) == 0);
    EXPECT(std::memcmp(x_other.data() + (size_t)(batch - 1) * (N + 1) * n, x_wrap.data() + (size_t)(batch - 1) * (N + 1) * n, (size_t)(N + 1) * n * sizeof(double)) != 0);
  } catch (const std::exception& e) {
    std::printf("  exception: %s\n", e.what());
    ++failures;
  }
  // the same calls through the C ABI
  altro_hip_batch* c = nullptr;
  EXPECT(altro_hip_batch_create(&c, N, n, m, batch, ALTRO_HIP_F64, ALTRO_HIP_PLAN_AUTO, 0, 0, nullptr) == 0);
  EXPECT(altro_hip_batch_plan(c) == plan_wrap);   // (the wrapper creates its handle with ALTRO_HIP_PLAN_AUTO)
  EXPECT(altro_hip_set_model_source_params(c, kBicycle, h, P) == 0);
  EXPECT(altro_hip_model_num_params(c) == P);
  EXPECT(altro_hip_set_model_params(c, theta.data(), 0) == 0);
  EXPECT(altro_hip_set_tracking_cost(c, Qd, Rd, xref, uref, 1, 1) == 0);
  EXPECT(altro_hip_set_initial_state(c, x0.data(), 0) == 0);
  EXPECT(altro_hip_set_input_guess(c, u.data(), 0, 0) == 0);
  EXPECT(altro_hip_open_loop_rollout(c) == 0);
  EXPECT(altro_hip_get_x(c, x_capi.data()) == 0);
  altro_hip_batch_destroy(c);
  double worst = 0.0;
  bool finite = true;
  for (size_t e = 0; e < nx; ++e) { worst = std::fmax(worst, std::fabs(x_wrap[e] - x_capi[e])); finite = finite && std::isfinite(x_wrap[e]); }
  std::printf("  |rollout difference| wrapper - C ABI: %.3e (plan %d)\n", worst, plan_wrap);
  EXPECT(finite);
  EXPECT(std::memcmp(x_wrap.data(), x_capi.data(), nx * sizeof(double)) == 0);
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("OK\n");
  return 0;
}
