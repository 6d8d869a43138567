// ALTROSolver::SetTimeStep(h, k_start, k_stop) with a device model (SetDeviceModel): the goal-constrained pendulum of
// altro_api_test.cpp on a grid of ten steps of 0.05 followed by ten of 0.1, solved by a solver with host callbacks -- which take h as
// their argument (typedefs.hpp:31-35) and run the host loop -- and by a solver whose Solve() runs on the device, where the steps go
// over as altro_hip_set_time_steps.  Same status and iteration count, objective and trajectory within the bounds of the uniform-grid
// comparison in altro_api_test.cpp (trajectory 1e-7; the objective, a smooth function of it, 1e-7 relative).  Then SetTimeStep(0.05)
// for every knot point on the SAME solvers and a second Solve: the device solver follows without being created again.
// Also the batch wrapper's SetTimeSteps / GetTimeSteps (include/altro_hip/altro_hip.hpp).  Prints "OK" and returns 0 when everything
// holds; needs an MI355X.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "altro/altro.hpp"
#include "altro_hip/altro_hip.h"
#include "altro_hip/altro_hip.hpp"

using namespace altro;

static int failures = 0;
#define EXPECT(cond)                                                                         \
  do {                                                                                       \
    if (!(cond)) { std::printf("  EXPECT FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

// pendulum with explicit-midpoint discretisation (test_utils.cpp:43-132 equations), as in altro_api_test.cpp
static void pend_f(double* xd, const double* x, const double* u) {
  const double l = 0.5, g = 9.81, b = 0.1, mm = 1.0 * l * l;
  xd[0] = x[1];
  xd[1] = u[0] / mm - g * std::sin(x[0]) / l - b * x[1] / mm;
}
static void pend_J(double* J, const double* x, const double* u) {
  (void)u;
  const double l = 0.5, g = 9.81, b = 0.1, mm = 1.0 * l * l;
  J[0] = 0; J[1] = -g * std::cos(x[0]) / l; J[2] = 1; J[3] = -b / mm; J[4] = 0; J[5] = 1 / mm;
}
static void pend_dyn(double* xn, const double* x, const double* u, float h) {
  double xm[2];
  pend_f(xm, x, u);
  for (int i = 0; i < 2; ++i) xm[i] = x[i] + (double)(h / 2) * xm[i];
  pend_f(xn, xm, u);
  for (int i = 0; i < 2; ++i) xn[i] = x[i] + h * xn[i];
}
static void pend_jac(double* J, const double* x, const double* u, float h) {
  double xm[2], J0[6], Jm[6];
  pend_f(xm, x, u);
  for (int i = 0; i < 2; ++i) xm[i] = x[i] + (double)(h / 2) * xm[i];
  pend_J(J0, x, u);
  pend_J(Jm, xm, u);
  double T[4];
  for (int j = 0; j < 2; ++j) for (int i = 0; i < 2; ++i) T[i + 2 * j] = (i == j) + (double)(h / 2) * J0[i + 2 * j];
  for (int j = 0; j < 2; ++j)
    for (int i = 0; i < 2; ++i) {
      double s = 0;
      for (int k = 0; k < 2; ++k) s += (h * Jm[i + 2 * k]) * T[k + 2 * j];
      J[i + 2 * j] = (i == j) + s;
    }
  for (int i = 0; i < 2; ++i) {
    double s = 0;
    for (int k = 0; k < 2; ++k) s += (Jm[i + 2 * k] * (double)(h / 2)) * J0[4 + k];
    J[4 + i] = h * (s + Jm[4 + i]);
  }
}

static double dist(const std::vector<double>& a, const std::vector<double>& b) {
  double s = 0;
  for (size_t i = 0; i < a.size(); ++i) s += (a[i] - b[i]) * (a[i] - b[i]);
  return std::sqrt(s);
}

struct Outcome {
  SolveStatus status;
  int iterations;
  double objective;
  std::vector<double> traj;
};
static Outcome solve(ALTROSolver& s, int N, int n, int m) {
  Outcome o;
  o.status = s.Solve();
  o.iterations = s.GetIterations();
  o.objective = (double)s.GetFinalObjective();
  o.traj.resize((size_t)(N + 1) * n + (size_t)N * m);
  for (int k = 0; k <= N; ++k) s.GetState(o.traj.data() + (size_t)k * n, k);
  for (int k = 0; k < N; ++k) s.GetInput(o.traj.data() + (size_t)(N + 1) * n + (size_t)k * m, k);
  return o;
}
static void compare(const char* what, const Outcome& host, const Outcome& dev) {
  const double dd = dist(host.traj, dev.traj), dobj = std::fabs(host.objective - dev.objective);
  std::printf("   %s: host callbacks status %d, iterations %d, objective %.10g | device model status %d, iterations %d, objective %.10g | "
              "|trajectory difference| = %.3e\n", what, (int)host.status, host.iterations, host.objective, (int)dev.status, dev.iterations,
              dev.objective, dd);
  EXPECT(host.status == SolveStatus::Success && dev.status == SolveStatus::Success);
  EXPECT(host.iterations == dev.iterations);
  EXPECT(dd < 1e-7);
  EXPECT(dobj <= 1e-7 * std::fmax(1.0, std::fabs(host.objective)));
}

static void test_pendulum_two_step_grid() {
  std::printf("[pendulum] goal constrained, SetTimeStep(0.05, 0, 10) + SetTimeStep(0.1, 10, N)\n");
  const int n = 2, m = 1, N = 20;
  std::vector<double> Qd(n, 1e-2), Rd(m, 1e-3), Qdf(n, 1.0), x0 = {0.3, -0.2}, xf = {M_PI, 0.0}, uf(m, 0.0);
  ALTROSolver host(N), dev(N);
  ALTROSolver* both[2] = {&host, &dev};
  for (int d = 0; d < 2; ++d) {
    ALTROSolver& s = *both[d];
    EXPECT(s.SetDimension(n, m, 0, LastIndex) == ErrorCodes::NoError);
    EXPECT(s.SetTimeStep(0.05f, 0, 10) == ErrorCodes::NoError);
    EXPECT(s.SetTimeStep(0.1f, 10, N) == ErrorCodes::NoError);
    if (d) EXPECT(s.SetDeviceModel(ALTRO_HIP_MODEL_PENDULUM) == ErrorCodes::NoError);
    else EXPECT(s.SetExplicitDynamics(pend_dyn, pend_jac, 0, LastIndex) == ErrorCodes::NoError);
    EXPECT(s.SetLQRCost(n, m, Qd.data(), Rd.data(), xf.data(), uf.data(), 0, N) == ErrorCodes::NoError);
    EXPECT(s.SetLQRCost(n, m, Qdf.data(), Rd.data(), xf.data(), uf.data(), N) == ErrorCodes::NoError);
    EXPECT(s.SetInitialState(x0.data(), n) == ErrorCodes::NoError);
    const double G[4] = {1, 0, 0, 1};   // x_N - xf = 0
    EXPECT(s.SetLinearConstraint(G, xf.data(), n, ConstraintType::EQUALITY, "Goal constraint", N, N + 1) == ErrorCodes::NoError);
    EXPECT(s.Initialize() == ErrorCodes::NoError);
    std::vector<double> u0(m, 0.1);
    s.SetInput(u0.data(), m, 0, LastIndex);
    AltroOptions o; o.iterations_max = 100;
    s.SetOptions(o);
  }
  const Outcome h1 = solve(host, N, n, m), d1 = solve(dev, N, n, m);
  compare("two-step grid", h1, d1);
  std::vector<double> xN(h1.traj.begin() + (size_t)N * n, h1.traj.begin() + (size_t)(N + 1) * n);
  EXPECT(dist(xN, xf) < 1e-4);
  // the same solvers on a uniform grid: the device solver follows the new steps without being created again
  for (int d = 0; d < 2; ++d) {
    ALTROSolver& s = *both[d];
    EXPECT(s.SetTimeStep(0.05f, 0, LastIndex) == ErrorCodes::NoError);
    std::vector<double> u0(m, 0.1);
    s.SetInput(u0.data(), m, 0, LastIndex);
  }
  const Outcome h2 = solve(host, N, n, m), d2 = solve(dev, N, n, m);
  compare("uniform 0.05 on the same solvers", h2, d2);
  EXPECT(dist(h1.traj, h2.traj) > 1e-2);   // (the grid matters: another problem, another solution)
}

static void test_batch_wrapper() {
  std::printf("[batch wrapper] SetTimeSteps / GetTimeSteps\n");
  const int N = 8;
  altro::hip::BatchSolver bs(N, 2, 1, 5);
  bs.SetModel(ALTRO_HIP_MODEL_PENDULUM, 0.05f);
  std::vector<float> dt(N), got(N, 0.0f);
  for (int k = 0; k < N; ++k) dt[k] = 0.02f + 0.003f * (float)k;
  bs.GetTimeSteps(got.data());
  for (int k = 0; k < N; ++k) EXPECT(got[k] == 0.05f);
  bs.SetTimeSteps(dt.data());
  bs.GetTimeSteps(got.data());
  for (int k = 0; k < N; ++k) EXPECT(got[k] == dt[k]);
  bs.SetTimeSteps(nullptr);
  bs.GetTimeSteps(got.data());
  for (int k = 0; k < N; ++k) EXPECT(got[k] == 0.05f);
}

int main() {
  test_pendulum_two_step_grid();
  test_batch_wrapper();
  if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
  std::printf("OK\n");
  return 0;
}
