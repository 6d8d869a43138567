// tests/cpp/batch_solver_user_constraint_test.cpp -- altro::hip::BatchSolver::SetUserConstraint (include/altro_hip/altro_hip.hpp) on
// plan GENERIC: a planar point mass with two idle oscillators (n = 8, m = 2) from source on a PLAN_AUTO handle -- the source defines
// a disc to stay out of, so the still-empty handle moves from the tile to plan GENERIC -- flies past the disc.  Prints PASS / FAIL
// lines; the exit code is the number of failures.
#include <cmath>
#include <cstdio>
#include <vector>

#include "altro_hip/altro_hip.hpp"

static int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static const char* kSource = R"(
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xd) {
  for (int i = 0; i < 4; ++i) xd[i] = x[4 + i];
  xd[4] = u[0]; xd[5] = u[1]; xd[6] = -x[2]; xd[7] = -x[3];
}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {   // 8 x 10, column-major
  (void)x; (void)u;
  for (int e = 0; e < 80; ++e) J[e] = T(0);
  for (int i = 0; i < 4; ++i) J[i + (4 + i) * 8] = T(1);
  J[4 + 8 * 8] = T(1); J[5 + 9 * 8] = T(1); J[6 + 2 * 8] = T(-1); J[7 + 3 * 8] = T(-1);
}
// block 0: stay outside the disc of radius 0.4 around (1.0, 0.45)
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - T(1.0), dy = x[1] - T(0.45);
  c[0] = T(0.16) - dx * dx - dy * dy;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // 1 x 10
  (void)id; (void)u;
  for (int e = 0; e < 10; ++e) J[e] = T(0);
  J[0] = -T(2) * (x[0] - T(1.0)); J[1] = -T(2) * (x[1] - T(0.45));
}
)";

int main() {
  using altro::hip::BatchSolver;
  using altro::hip::Cone;
  const int N = 40, n = 8, m = 2, batch = 32;
  BatchSolver solver(N, n, m, batch);
  solver.SetModelSource(kSource, 0.1f);
  EXPECT(solver.GetPlan() == ALTRO_HIP_PLAN_GENERIC);
  const double Qd[2 * 8] = {1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2, 50, 50, 50, 50, 50, 50, 50, 50};
  const double Rd[2] = {1e-2, 1e-2};
  double xref[2 * 8] = {0};
  for (int t = 0; t < 2; ++t) { xref[t * 8 + 0] = 2.0; xref[t * 8 + 1] = 1.0; }
  const double uref[2] = {0, 0};
  solver.SetLQRCost(Qd, Rd, xref, uref, true, true);
  std::vector<double> x0(batch * n, 0.0);
  for (int b = 0; b < batch; ++b) x0[b * n + 1] = 0.1 * (b - batch / 2) / batch;
  solver.SetInitialState(x0.data());
  const double u0[2] = {0.1, 0.05};
  solver.SetInput(u0, true, true);
  const int bid = solver.SetUserConstraint(1, N, Cone::Inequality, 1, 0);
  EXPECT(bid == 0);
  solver.opts.iterations_max = 150;
  solver.opts.penalty_initial = 10;
  auto res = solver.Solve();
  EXPECT(res.NumConverged() >= batch / 2);
  for (const auto& r : res.problems)
    if (r.status == 0) EXPECT(r.primal_feasibility < 1e-4);
  std::vector<double> x(batch * (N + 1) * n), u(batch * N * m);
  solver.GetTrajectory(x.data(), u.data());
  double worst = 1e9;
  for (int b = 0; b < batch; ++b) {
    if (res.problems[b].status != 0) continue;
    for (int k = 0; k <= N; ++k) {
      const double* xk = &x[(b * (N + 1) + k) * n];
      worst = std::fmin(worst, std::hypot(xk[0] - 1.0, xk[1] - 0.45));
    }
    EXPECT(std::fabs(x[(b * (N + 1) + N) * n + 0] - 2.0) < 0.15 && std::fabs(x[(b * (N + 1) + N) * n + 1] - 1.0) < 0.15);
  }
  EXPECT(worst > 0.4 - 2e-3);
  std::printf("converged %d / %d, closest approach %.4f\n", res.NumConverged(), batch, worst);
  std::printf("%s\n", failures ? "FAIL" : "PASS");
  return failures;
}
