// altro_hip.hpp -- header-only C++17 convenience over the C ABI of altro_hip.h (no additional symbols: everything
// here inlines into calls of the extern "C" entry points, so it adds nothing to the drop-in boundary).
//
// altro::hip::BatchSolver is the batched sibling of altro::ALTROSolver (src/altro/altro_solver.hpp:21-442): the same
// vocabulary (SetLQRCost, SetInitialState, SetInput, SetConstraint, Solve, GetState / GetInput, UpdateLinearCosts,
// ShiftTrajectory) applied to `batch` independent problems resident on one MI355X.  Errors follow the reference's
// convention for ALTRO_ENABLE_RUNTIME_EXCEPTIONS: they throw (std::runtime_error with altro_hip_last_error()).
#pragma once
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "altro_hip/altro_hip.h"

namespace altro {
namespace hip {

enum class Cone { Equality = 0, Identity = 1, Inequality = 2, SecondOrder = 3 };   // ConstraintType, typedefs.hpp:29-34

struct SolveResult {
  std::vector<altro_hip_solve_result> problems;   // AltroStats per problem
  int sweeps = 0, merit_launches = 0;
  int NumConverged() const {
    int c = 0;
    for (const auto& r : problems) c += r.status == 0;
    return c;
  }
};

class BatchSolver {
 public:
  BatchSolver(int horizon_length, int num_states, int num_inputs, int batch, altro_hip_dtype dtype = ALTRO_HIP_F64,
              int device = 0, unsigned flags = 0, void* stream = nullptr)
      : N_(horizon_length), n_(num_states), m_(num_inputs), batch_(batch) {
    Check(altro_hip_batch_create(&h_, N_, n_, m_, batch_, dtype, ALTRO_HIP_PLAN_AUTO, flags, device, stream));
    altro_hip_default_solve_options(&opts);
  }
  ~BatchSolver() { altro_hip_batch_destroy(h_); }
  BatchSolver(const BatchSolver&) = delete;
  BatchSolver& operator=(const BatchSolver&) = delete;
  BatchSolver(BatchSolver&& o) noexcept { *this = std::move(o); }
  BatchSolver& operator=(BatchSolver&& o) noexcept {
    if (this != &o) {
      if (h_) altro_hip_batch_destroy(h_);
      h_ = o.h_; o.h_ = nullptr;
      N_ = o.N_; n_ = o.n_; m_ = o.m_; batch_ = o.batch_; opts = o.opts;
    }
    return *this;
  }

  int GetHorizonLength() const { return N_; }
  int GetStateDim() const { return n_; }
  int GetInputDim() const { return m_; }
  int GetBatch() const { return batch_; }
  int GetPlan() const { return altro_hip_batch_plan(h_); }
  altro_hip_batch* Handle() { return h_; }

  // ---- problem definition (arrays in the reference's layout, [batch][k][column-major block]) ----------------
  // KnotPointData::SetLinearDynamics for every knot point of every problem (plan MFMA16 / TVLQR sweeps)
  void SetLinearDynamics(const double* A, const double* B, const double* f, bool shared_over_k = false,
                         bool shared_over_batch = false) {
    Check(altro_hip_set_dynamics(h_, A, B, f, shared_over_k, shared_over_batch));
  }
  // SetExplicitDynamics with one of the compiled-in device models (plan LANE)
  void SetModel(altro_hip_model model, float timestep, int bicycle_frame = 0, double bicycle_length = 2.7,
                double bicycle_lr = 1.5) {
    Check(altro_hip_set_model(h_, model, timestep, bicycle_frame, bicycle_length, bicycle_lr));
  }
  // ALTROSolver::SetLQRCost for all knot points: Qd, xref [batch][N+1][n]; Rd, uref [batch][N][m]
  void SetLQRCost(const double* Qd, const double* Rd, const double* xref, const double* uref, bool shared_over_k = false,
                  bool shared_over_batch = false) {
    Check(altro_hip_set_tracking_cost(h_, Qd, Rd, xref, uref, shared_over_k, shared_over_batch));
  }
  // ALTROSolver::SetQuadraticCost (altro_solver.cpp:118-136) for all knot points: the general quadratic cost with the cross term
  // u^T H x.  Q [batch][N+1][n*n], R [batch][N][m*m], H [batch][N][m*n] (column-major blocks), q, r, c likewise (c may be null)
  void SetQuadraticCost(const double* Q, const double* R, const double* H, const double* q, const double* r, const double* c,
                        bool shared_over_k = false, bool shared_over_batch = false) {
    Check(altro_hip_set_quadratic_cost(h_, Q, R, H, q, r, c, shared_over_k, shared_over_batch));
  }
  // SetExplicitDynamics with the caller's own continuous model as HIP source, compiled at run time (altro_hip_set_model_source)
  void SetModelSource(const char* source, float timestep) { Check(altro_hip_set_model_source(h_, source, timestep)); }
  // ... whose functions take num_params per-problem parameters `p` (altro_hip_set_model_source_params); theta: host [batch][num_params],
  // or one set for every problem; nothing steps the model before SetModelParams
  void SetModelSource(const char* source, float timestep, int num_params) { Check(altro_hip_set_model_source_params(h_, source, timestep, num_params)); }
  void SetModelParams(const double* theta, bool shared_over_batch = false) { Check(altro_hip_set_model_params(h_, theta, shared_over_batch ? 1 : 0)); }
  void GetModelParams(double* theta) { Check(altro_hip_get_model_params(h_, theta)); }
  int ModelNumParams() const { return altro_hip_model_num_params(h_); }
  // ALTROSolver::SetTimeStep per knot-point range for the device model: dt[k] (N floats) = the step from knot point k to k + 1, shared by
  // the batch; nullptr: the uniform step of SetModel / SetModelSource again (altro_hip_set_time_steps)
  void SetTimeSteps(const float* dt) { Check(altro_hip_set_time_steps(h_, dt)); }
  void GetTimeSteps(float* dt) { Check(altro_hip_get_time_steps(h_, dt)); }
  // whether the device model runs the loop's row-layout model kernels (plans GENERIC / MFMA32; altro_hip_model_row_layout)
  bool ModelRowLayout() const { return altro_hip_model_row_layout(h_) != 0; }
  void SetInitialState(const double* x0, bool shared_over_batch = false) {
    Check(altro_hip_set_initial_state(h_, x0, shared_over_batch));
  }
  void SetInput(const double* u, bool shared_over_k = false, bool shared_over_batch = false) {
    Check(altro_hip_set_input_guess(h_, u, shared_over_k, shared_over_batch));
  }
  void SetState(const double* x, bool shared_over_k = false, bool shared_over_batch = false) {
    Check(altro_hip_set_state_guess(h_, x, shared_over_k, shared_over_batch));
  }
  // ALTROSolver::SetConstraint for c = G [x;u] - g in `cone` at knot points k_start .. k_stop (inclusive);
  // G is p x (n+m) column-major; returns the block id
  int SetConstraint(int k_start, int k_stop, Cone cone, int p, const double* G, const double* g, bool g_per_problem = false) {
    const int id = altro_hip_add_linear_constraint(h_, k_start, k_stop, static_cast<int>(cone), p, G, g, g_per_problem);
    if (id < 0) Check(id);
    return id;
  }
  // ALTROSolver::SetConstraint with a general callback pair: block `id` of the altro_user_constraint / _jacobian pair in the source
  // given to SetModelSource, p rows in `cone` at knot points k_start .. k_stop (plans LANE and GENERIC / MFMA32); returns the block id
  int SetUserConstraint(int k_start, int k_stop, Cone cone, int p, int id) {
    const int bid = altro_hip_add_user_constraint(h_, k_start, k_stop, static_cast<int>(cone), p, id);
    if (bid < 0) Check(bid);
    return bid;
  }
  void ClearConstraints() { Check(altro_hip_clear_constraints(h_)); }
  void ResetDuals(double penalty = 1.0) { Check(altro_hip_reset_duals(h_, penalty)); }
  // Warm-started duals for receding-horizon MPC (altro_hip.h: altro_hip_set_duals and its siblings; the reference declares SetDual*,
  // altro_solver.hpp:357-362): z [batch][p] of block `slot` at knot point k as given, the penalty per problem, and the duals' side of
  // ShiftTrajectory
  void SetDuals(int k, int slot, const double* z) { Check(altro_hip_set_duals(h_, k, slot, z)); }
  void GetPenalty(double* rho) { Check(altro_hip_get_penalty(h_, rho)); }
  void SetPenalty(const double* rho) { Check(altro_hip_set_penalty(h_, rho, 0)); }   // rho [batch]
  void SetPenalty(double rho) { Check(altro_hip_set_penalty(h_, &rho, 1)); }          // one value for every problem
  void ShiftDuals(int tail = ALTRO_HIP_DUAL_TAIL_KEEP) { Check(altro_hip_shift_duals(h_, tail)); }
  // Right-hand sides per knot point (altro_hip.h: altro_hip_add_linear_constraint_rhs and its siblings): SetConstraint with g as
  // [nb][nk][p] (rhs_layout: ALTRO_HIP_RHS_PER_PROBLEM | ALTRO_HIP_RHS_PER_KNOT), new values in place for knot points k_first .. k_last of
  // block `id` (-1, -1: its whole range; g follows the pointer mode), what the device holds at knot point k ([nb][p], host), and the
  // right-hand sides' part of ShiftTrajectory
  int AddLinearConstraintRhs(int k_start, int k_stop, Cone cone, int p, const double* G, const double* g, int rhs_layout) {
    const int id = altro_hip_add_linear_constraint_rhs(h_, k_start, k_stop, static_cast<int>(cone), p, G, g, rhs_layout);
    if (id < 0) Check(id);
    return id;
  }
  void SetConstraintRhs(int id, const double* g, int k_first = -1, int k_last = -1) { Check(altro_hip_set_constraint_rhs(h_, id, k_first, k_last, g)); }
  void GetConstraintRhs(int id, int k, double* g) { Check(altro_hip_get_constraint_rhs(h_, id, k, g)); }
  void ShiftConstraintRhs() { Check(altro_hip_shift_constraint_rhs(h_)); }

  // ---- solve ------------------------------------------------------------------------------------------------------
  altro_hip_solve_options opts;   // AltroOptions (solver_options.hpp:16-39)
  SolveResult Solve() {
    SolveResult r;
    r.problems.resize(batch_);
    Check(altro_hip_ilqr_solve(h_, &opts, r.problems.data()));
    Check(altro_hip_last_solve_counts(h_, &r.sweeps, &r.merit_launches));
    return r;
  }
  // TVLQR sweep on the data as it stands: tvlqr_BackwardPass + tvlqr_ForwardPass for every problem
  void Sweep(double reg = 0.0) { Check(altro_hip_sweep(h_, reg)); }
  void Synchronize() { Check(altro_hip_synchronize(h_)); }

  // ---- results (host arrays, reference layout) ---------------------------------------------------------------
  void GetTrajectory(double* x /*[batch][N+1][n]*/, double* u /*[batch][N][m]*/) { Check(altro_hip_get_nominal(h_, x, u)); }
  void GetKnotPoint(int k, double* x /*[batch][n]*/, double* u /*[batch][m] or nullptr*/) { Check(altro_hip_get_knot(h_, k, x, u)); }
  void GetFeedbackGain(double* K /*[batch][N][m*n]*/) { Check(altro_hip_get_K(h_, K)); }
  void GetFeedforwardGain(double* d /*[batch][N][m]*/) { Check(altro_hip_get_d(h_, d)); }
  void GetCostToGo(double* P, double* p) {
    if (P) Check(altro_hip_get_P(h_, P));
    if (p) Check(altro_hip_get_p(h_, p));
  }
  void GetBackwardStatus(int* status /*[batch]: -1 or the failing knot point*/) { Check(altro_hip_get_status(h_, status)); }

  // ---- MPC methods (altro_solver.cpp:266-293) ---------------------------------------------------------------------
  void UpdateLinearCosts(const double* q, const double* r, const double* c, int k_start, int k_stop, bool shared_over_k = false,
                         bool shared_over_batch = false) {
    Check(altro_hip_update_linear_costs(h_, q, r, c, k_start, k_stop, shared_over_k, shared_over_batch));
  }
  void ShiftTrajectory() { Check(altro_hip_shift_trajectory(h_)); }
  // The problem data's part of ShiftTrajectory for dynamics given as data and a reference that moves with the horizon (altro_hip.h:
  // altro_hip_set_dynamics_range and its siblings): knot points k_first .. k_last of the dynamics rewritten in place (A, B, f follow the
  // pointer mode), what the device holds at knot point k (host arrays, any may be null), and the one-knot-point shifts of (A, B, f) and
  // of (q, r, c) -- after which the caller writes knot point N-1 (and q_N, c_N) anew
  void SetDynamicsRange(const double* A, const double* B, const double* f, int k_first, int k_last, bool shared_over_batch = false) {
    Check(altro_hip_set_dynamics_range(h_, A, B, f, k_first, k_last, shared_over_batch));
  }
  void GetDynamicsKnot(int k, double* A, double* B, double* f) { Check(altro_hip_get_dynamics_knot(h_, k, A, B, f)); }
  void ShiftDynamics() { Check(altro_hip_shift_dynamics(h_)); }
  void ShiftLinearCosts() { Check(altro_hip_shift_linear_costs(h_)); }

 private:
  static void Check(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("altro_hip error ") + std::to_string(rc) + ": " + altro_hip_last_error());
  }
  altro_hip_batch* h_ = nullptr;
  int N_ = 0, n_ = 0, m_ = 0, batch_ = 0;
};

}  // namespace hip
}  // namespace altro
