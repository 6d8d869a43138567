"""Constraint blocks from source on plans GENERIC / MFMA32 (altro_hip_add_user_constraint past plan LANE): the caller's
altro_user_constraint / _jacobian pair, compiled by hiprtc into plan GENERIC's AL kernels (kernels/ilqr_generic.hip, GEN_USER_BLOCKS) --
ALTROSolver::SetConstraint with a general callback pair (altro_solver.cpp:192-223) for the vehicles past the tile.

* linear blocks written as source solve like the same blocks given as data (row-wise cones, both second-order-cone branches), and
  like the oracle;
* a nonlinear block (the unicycle's disc) gives plan GENERIC the decisions plan LANE takes;
* the 13-state quadrotor flies around a keep-out sphere; phi' of the merit function is the derivative of phi;
* a block added after a solve is honoured by the next one (the AL flags are current when the solve chooses its kernels);
* what the surface takes and refuses.
Each source below is compiled once per (source, n, m) and process."""
import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import cpp_build, problems

pytestmark = pytest.mark.gpu

N, n, m = 30, 13, 4
H = np.float32(0.02)
HOVER = np.array([0.5 * 9.81, 0.0, 0.0, 0.0])
THRUST_G = np.array([1.25 * HOVER[0], -0.6 * HOVER[0]])
SPHERE_C, SPHERE_R = np.array([-0.75, 0.0, 0.0]), 0.3

# tests/test_gpu_generic_model.py's quadrotor, with four constraint blocks:
#   0: the thrust bounds of its test_whole_solves, u0 - 1.25 hover <= 0, -u0 + 0.6 hover <= 0 (INEQUALITY, 2 rows)
#   1: |(u1, u2)| <= 0.02 (SOC, 3 rows)      2: |(v, u1, u2)| <= 1.2 (SOC, 6 rows: the many-row branch)
#   3: the keep-out sphere r^2 - |p - c|^2 <= 0 (INEQUALITY, 1 row)
QUADROTOR13_SRC = r"""
template <typename T>
__device__ void altro_user_dynamics(const T* x, const T* u, T* xd) {
  const T mass = T(0.5), g = T(9.81), Ix = T(0.0023), Iy = T(0.0023), Iz = T(0.004);
  const T qw = x[3], qx = x[4], qy = x[5], qz = x[6], wx = x[10], wy = x[11], wz = x[12];
  xd[0] = x[7]; xd[1] = x[8]; xd[2] = x[9];
  xd[3] = T(0.5) * (-qx * wx - qy * wy - qz * wz);
  xd[4] = T(0.5) * (qw * wx + qy * wz - qz * wy);
  xd[5] = T(0.5) * (qw * wy - qx * wz + qz * wx);
  xd[6] = T(0.5) * (qw * wz + qx * wy - qy * wx);
  const T a = u[0] * (T(1) / mass);
  xd[7] = a * (T(2) * (qx * qz + qw * qy));
  xd[8] = a * (T(2) * (qy * qz - qw * qx));
  xd[9] = a * (T(1) - T(2) * (qx * qx + qy * qy)) - g;
  xd[10] = (u[1] - (Iz - Iy) * wy * wz) * (T(1) / Ix);
  xd[11] = (u[2] - (Ix - Iz) * wz * wx) * (T(1) / Iy);
  xd[12] = (u[3] - (Iy - Ix) * wx * wy) * (T(1) / Iz);
}
template <typename T>
__device__ void altro_user_jacobian(const T* x, const T* u, T* J) {
  const int n = 13;
  const T mass = T(0.5), Ix = T(0.0023), Iy = T(0.0023), Iz = T(0.004);
  for (int e = 0; e < 13 * 17; ++e) J[e] = T(0);
  const T qw = x[3], qx = x[4], qy = x[5], qz = x[6], wx = x[10], wy = x[11], wz = x[12];
  J[0 + 7 * n] = T(1); J[1 + 8 * n] = T(1); J[2 + 9 * n] = T(1);
  J[3 + 4 * n] = T(-0.5) * wx; J[3 + 5 * n] = T(-0.5) * wy; J[3 + 6 * n] = T(-0.5) * wz; J[3 + 10 * n] = T(-0.5) * qx; J[3 + 11 * n] = T(-0.5) * qy; J[3 + 12 * n] = T(-0.5) * qz;
  J[4 + 3 * n] = T(0.5) * wx; J[4 + 5 * n] = T(0.5) * wz; J[4 + 6 * n] = T(-0.5) * wy; J[4 + 10 * n] = T(0.5) * qw; J[4 + 11 * n] = T(-0.5) * qz; J[4 + 12 * n] = T(0.5) * qy;
  J[5 + 3 * n] = T(0.5) * wy; J[5 + 4 * n] = T(-0.5) * wz; J[5 + 6 * n] = T(0.5) * wx; J[5 + 10 * n] = T(0.5) * qz; J[5 + 11 * n] = T(0.5) * qw; J[5 + 12 * n] = T(-0.5) * qx;
  J[6 + 3 * n] = T(0.5) * wz; J[6 + 4 * n] = T(0.5) * wy; J[6 + 5 * n] = T(-0.5) * wx; J[6 + 10 * n] = T(-0.5) * qy; J[6 + 11 * n] = T(0.5) * qx; J[6 + 12 * n] = T(0.5) * qw;
  const T rm = T(1) / mass, a = u[0] * rm;
  J[7 + 3 * n] = T(2) * a * qy; J[7 + 4 * n] = T(2) * a * qz; J[7 + 5 * n] = T(2) * a * qw; J[7 + 6 * n] = T(2) * a * qx;
  J[7 + 13 * n] = T(2) * (qx * qz + qw * qy) * rm;
  J[8 + 3 * n] = T(-2) * a * qx; J[8 + 4 * n] = T(-2) * a * qw; J[8 + 5 * n] = T(2) * a * qz; J[8 + 6 * n] = T(2) * a * qy;
  J[8 + 13 * n] = T(2) * (qy * qz - qw * qx) * rm;
  J[9 + 4 * n] = T(-4) * a * qx; J[9 + 5 * n] = T(-4) * a * qy;
  J[9 + 13 * n] = (T(1) - T(2) * (qx * qx + qy * qy)) * rm;
  J[10 + 11 * n] = -(Iz - Iy) * wz * (T(1) / Ix); J[10 + 12 * n] = -(Iz - Iy) * wy * (T(1) / Ix); J[10 + 14 * n] = T(1) / Ix;
  J[11 + 10 * n] = -(Ix - Iz) * wz * (T(1) / Iy); J[11 + 12 * n] = -(Ix - Iz) * wx * (T(1) / Iy); J[11 + 15 * n] = T(1) / Iy;
  J[12 + 10 * n] = -(Iy - Ix) * wy * (T(1) / Iz); J[12 + 11 * n] = -(Iy - Ix) * wx * (T(1) / Iz); J[12 + 16 * n] = T(1) / Iz;
}
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  if (id == 0) {
    const T hv = T(0.5) * T(9.81);
    const T g0 = T(1.25) * hv, g1 = T(-0.6) * hv;
    c[0] = u[0] - g0;
    c[1] = -u[0] - g1;
  } else if (id == 1) {
    c[0] = u[1]; c[1] = u[2]; c[2] = T(0.02);
  } else if (id == 2) {
    c[0] = x[7]; c[1] = x[8]; c[2] = x[9]; c[3] = u[1]; c[4] = u[2]; c[5] = T(1.2);
  } else {
    const T dx = x[0] - T(-0.75), dy = x[1], dz = x[2];
    c[0] = T(0.09) - dx * dx - dy * dy - dz * dz;
  }
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // p x 17
  (void)u;
  if (id == 0) {
    for (int e = 0; e < 2 * 17; ++e) J[e] = T(0);
    J[0 + 13 * 2] = T(1); J[1 + 13 * 2] = T(-1);
  } else if (id == 1) {
    for (int e = 0; e < 3 * 17; ++e) J[e] = T(0);
    J[0 + 14 * 3] = T(1); J[1 + 15 * 3] = T(1);
  } else if (id == 2) {
    for (int e = 0; e < 6 * 17; ++e) J[e] = T(0);
    J[0 + 7 * 6] = T(1); J[1 + 8 * 6] = T(1); J[2 + 9 * 6] = T(1); J[3 + 14 * 6] = T(1); J[4 + 15 * 6] = T(1);
  } else {
    for (int e = 0; e < 17; ++e) J[e] = T(0);
    J[0] = -T(2) * (x[0] - T(-0.75)); J[1] = -T(2) * x[1]; J[2] = -T(2) * x[2];
  }
}
"""


def linear_block(bid):
    """Block `bid` of the source as (cone, G, g) of c = G [x; u] - g."""
    if bid == 0:
        G = np.zeros((2, n + m)); G[0, n] = 1.0; G[1, n] = -1.0
        return altro_amd.CONE_INEQUALITY, G, THRUST_G
    if bid == 1:
        G = np.zeros((3, n + m)); G[0, n + 1] = 1.0; G[1, n + 2] = 1.0
        return altro_amd.CONE_SOC, G, np.array([0.0, 0.0, -0.02])
    G = np.zeros((6, n + m))
    G[0, 7] = G[1, 8] = G[2, 9] = 1.0; G[3, n + 1] = G[4, n + 2] = 1.0
    return altro_amd.CONE_SOC, G, np.array([0.0, 0.0, 0.0, 0.0, 0.0, -1.2])


def make_case(batch, seed=0, toward_sphere=False):
    """tests/test_gpu_generic_model.py's flight to hover at the origin; toward_sphere: every vehicle starts near (-1.5, 0, 0), so the
    straight path to the origin crosses the sphere around (-0.75, 0, 0)."""
    x0 = np.zeros((batch, n))
    if toward_sphere:
        x0[:, :3] = np.array([-1.5, 0.0, 0.0]) + 0.05 * problems.normal((batch, 3), 291 + seed)
    else:
        x0[:, :3] = 0.8 * problems.normal((batch, 3), 191 + seed)
    q = np.concatenate([np.ones((batch, 1)), 0.12 * problems.normal((batch, 3), 192 + seed)], axis=1)
    x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, 7:10] = 0.3 * problems.normal((batch, 3), 193 + seed)
    x0[:, 10:] = 0.2 * problems.normal((batch, 3), 194 + seed)
    xref = np.zeros(n); xref[3] = 1.0
    Qd = np.concatenate([np.full(3, 2.0), np.full(4, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
    Rd = np.array([0.05, 20.0, 20.0, 20.0])
    return dict(x0=x0, Qd=Qd, Qfd=20.0 * Qd, Rd=Rd, xref=xref, uref=HOVER, u0=HOVER.copy())


def make_hip(c, plan=altro_amd.PLAN_AUTO):
    bt = altro_amd.Batch(N, n, m, c["x0"].shape[0], plan=plan)
    bt.set_model_source(QUADROTOR13_SRC, H)
    bt.set_tracking_cost(np.stack([c["Qd"], c["Qfd"]]), c["Rd"][None], np.stack([c["xref"], c["xref"]]), c["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(c["x0"])
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    return bt


def make_oracle(c, b, blocks=()):
    s = oracle.ILQR(N, n, m, H, oracle.DYN_MODEL, oracle.MODEL_QUADROTOR13, cost_kind=oracle.COST_DIAGONAL)
    for k in range(N + 1):
        s.L.oracle_ilqr_set_lqr_cost(s.h, k, np.ascontiguousarray(c["Qfd"] if k == N else c["Qd"]), np.ascontiguousarray(c["Rd"]),
                                     np.ascontiguousarray(c["xref"]), np.ascontiguousarray(c["uref"]))
    s.L.oracle_ilqr_set_initial_state(s.h, np.ascontiguousarray(c["x0"][b]))
    for (k0, k1, cone, G, g) in blocks:
        for k in range(k0, k1 + 1):
            s.add_linear_constraint(k, cone, G, g)
    s.L.oracle_ilqr_initialize(s.h)
    for k in range(N):
        s.L.oracle_ilqr_set_input(s.h, k, np.ascontiguousarray(c["u0"]))
    return s


def solve_pair(c, plan, bid, **opts):
    """The same problems with block `bid` from the source and as a linear block."""
    out = []
    for user in (True, False):
        bt = make_hip(c, plan)
        if plan == altro_amd.PLAN_AUTO:
            assert bt.plan == altro_amd.PLAN_MFMA32
        cone, G, g = linear_block(bid)
        if user:
            bt.add_user_constraint(0, N - 1, cone, G.shape[0], bid)
        else:
            bt.add_linear_constraint(0, N - 1, cone, G, g)
        res = bt.ilqr_solve(**opts)
        x, u = bt.get_nominal()
        out.append((res, x, u))
        bt.close()
    return out


@pytest.mark.parametrize("plan", [altro_amd.PLAN_GENERIC, altro_amd.PLAN_AUTO])
def test_linear_block_as_source_equals_the_linear_block_and_the_oracle(plan):
    """The thrust bounds of test_gpu_generic_model.py::test_whole_solves as a two-row INEQUALITY block from the source: every problem
    takes the decisions of the same block given as data, on the same trajectory; three of them are the oracle's solves."""
    batch = 32
    c = make_case(batch)
    (ra, xa, ua), (rb, xb, ub) = solve_pair(c, plan, 0, iterations_max=50, tol_stationarity=1e-3)
    for key in ("status", "iterations", "dual_updates"):
        assert np.array_equal(ra[key], rb[key]), (key, ra[key], rb[key])
    assert (ra["status"] == 0).sum() >= batch - 2
    np.testing.assert_allclose(xa, xb, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ua, ub, rtol=1e-8, atol=1e-8)
    cone, G, g = linear_block(0)
    blocks = [(0, N - 1, cone, G, g)]
    for b in [0, 10, 20]:
        s = make_oracle(c, b, blocks)
        s.set_penalty(1.0, 10.0)
        s.L.oracle_ilqr_set_options(s.h, 50, 1e-3, 1e-4, 1e-8, 0)
        status, iters, log = s.solve()
        assert ra["status"][b] == status and ra["iterations"][b] == iters, (b, ra["status"][b], status, ra["iterations"][b], iters)
        if status == 0:
            np.testing.assert_allclose(xa[b], s.get("x"), rtol=2e-7, atol=2e-7)
            np.testing.assert_allclose(ua[b], s.get("u"), rtol=2e-7, atol=2e-7)


@pytest.mark.parametrize("bid,p", [(1, 3), (2, 6)])
def test_linear_second_order_cone_as_source_equals_the_linear_block(bid, p):
    """A linear second-order cone from the source against the same cone given as data: p = 3 (gen_al_rows' closed forms in one lane)
    and p = 6 (one lane per row, wave sums)."""
    batch = 32
    c = make_case(batch, seed=1)
    assert linear_block(bid)[1].shape[0] == p
    (ra, xa, ua), (rb, xb, ub) = solve_pair(c, altro_amd.PLAN_AUTO, bid, iterations_max=60, tol_stationarity=1e-3)
    for key in ("status", "iterations", "dual_updates"):
        assert np.array_equal(ra[key], rb[key]), (key, ra[key], rb[key])
    assert (ra["status"] == 0).sum() >= batch // 2
    assert ra["dual_updates"].max() >= 1          # the cone is active somewhere: the duals moved
    np.testing.assert_allclose(xa, xb, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(ua, ub, rtol=1e-8, atol=1e-8)


# ---- the unicycle of tests/test_gpu_user_model.py with its disc, on plan LANE and on plan GENERIC -----------------------------------
UNICYCLE_OBSTACLE_SRC = r"""
// x = (px, py, theta), u = (v, omega):  px' = v cos(theta), py' = v sin(theta), theta' = omega
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xdot) {
  xdot[0] = u[0] * cos(x[2]);
  xdot[1] = u[0] * sin(x[2]);
  xdot[2] = u[1];
}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {   // 3 x 5, column-major
  for (int e = 0; e < 15; ++e) J[e] = T(0);
  J[0 + 2 * 3] = -u[0] * sin(x[2]);
  J[1 + 2 * 3] = u[0] * cos(x[2]);
  J[0 + 3 * 3] = cos(x[2]);
  J[1 + 3 * 3] = sin(x[2]);
  J[2 + 4 * 3] = T(1);
}
// block 0: stay outside a disc of radius 0.4 around (1.0, 0.45):  r^2 - |p - c|^2 <= 0   (nonlinear, INEQUALITY)
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - T(1.0), dy = x[1] - T(0.45);
  c[0] = T(0.16) - dx * dx - dy * dy;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // 1 x 5
  (void)id; (void)u;
  J[0] = -T(2) * (x[0] - T(1.0)); J[1] = -T(2) * (x[1] - T(0.45)); J[2] = T(0); J[3] = T(0); J[4] = T(0);
}
"""
UN, Un, Um = 40, 3, 2


def make_unicycle(plan, batch):
    xf = np.array([2.0, 1.0, 0.0])
    x0 = np.zeros((batch, Un)); x0[:, 1] = (problems.uniform01((batch,), 47) - 0.5) * 0.2
    bt = altro_amd.Batch(UN, Un, Um, batch, plan=plan)
    bt.set_model_source(UNICYCLE_OBSTACLE_SRC, np.float32(0.1))
    assert bt.plan == plan
    bt.set_tracking_cost(np.array([[1e-2] * 3, [50.0] * 3]), np.array([[1e-2, 1e-2]]), np.stack([xf, xf]), np.zeros((1, Um)),
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(x0)
    bt.set_input_guess(np.array([[[0.5, 0.1]]]), k_stride_zero=True, batch_stride_zero=True)
    bt.add_user_constraint(1, UN, altro_amd.CONE_INEQUALITY, 1, 0)
    return bt


def test_nonlinear_block_takes_plan_lanes_decisions_on_plan_generic():
    """The disc on plan LANE (pinned by tests/test_gpu_user_model.py) and on plan GENERIC: the merit function and its derivative on one
    trajectory, then whole solves problem by problem."""
    batch = 64
    vals = []
    for plan in (altro_amd.PLAN_LANE, altro_amd.PLAN_GENERIC):
        bt = make_unicycle(plan, batch)
        bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.backward()
        vals.append([bt.merit(a) for a in (0.25, 0.5, 1.0)])
        bt.close()
    for (pl, dl), (pg, dg) in zip(*vals):
        assert np.all(np.abs(pg - pl) <= 1e-12 * np.maximum(1.0, np.abs(pl))), np.abs(pg - pl).max()
        assert np.all(np.abs(dg - dl) <= 1e-10 * np.maximum(1.0, np.abs(dl))), np.abs(dg - dl).max()
    out = []
    for plan in (altro_amd.PLAN_LANE, altro_amd.PLAN_GENERIC):
        bt = make_unicycle(plan, batch)
        res = bt.ilqr_solve(iterations_max=150, penalty_initial=10.0)
        out.append((res, bt.get_nominal()[0]))
        bt.close()
    (rl, xl), (rg, xg) = out
    for key in ("status", "iterations", "dual_updates"):
        assert np.array_equal(rl[key], rg[key]), (key, np.nonzero(rl[key] != rg[key]))
    ok = rl["status"] == 0
    assert ok.sum() >= batch - 6
    # The two plans sum the same terms in different orders (a lane per problem against wave sums); over some forty sweeps and their
    # dual updates those roundings grow along the weakly determined directions of the converged trajectories up to the solve's own
    # tolerance (stationarity 1e-4): most entries agree to 2e-7, about one in a hundred only to a few 1e-5.
    np.testing.assert_allclose(xg[ok], xl[ok], rtol=1e-4, atol=1e-4)


def sphere_clearance(x):
    return np.linalg.norm(x[:, :, :3] - SPHERE_C, axis=2).min(axis=1)


def test_quadrotor_flies_around_a_keep_out_sphere():
    """256 vehicles whose straight path to hover crosses a sphere: with the sphere as a one-row block from the source every converged
    trajectory clears it to the feasibility tolerance; without it they pass through."""
    batch = 256
    c = make_case(batch, toward_sphere=True)
    clear = []
    for blocked in (False, True):
        bt = make_hip(c)
        assert bt.plan == altro_amd.PLAN_MFMA32
        cone, G, g = linear_block(0)
        bt.add_linear_constraint(0, N - 1, cone, G, g)
        if blocked:
            bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 3)
        res = bt.ilqr_solve(iterations_max=100, tol_stationarity=1e-3, penalty_initial=10.0)
        x, _ = bt.get_nominal()
        ok = res["status"] == 0
        assert ok.sum() >= 0.9 * batch, (blocked, int(ok.sum()))
        if blocked:
            assert (res["feasibility"][ok] < 1e-4).all()
            assert (bt.feasibility()[ok] < 1e-4).all()
        clear.append(sphere_clearance(x)[ok])
        bt.close()
    assert (clear[0] < SPHERE_R - 0.01).sum() >= batch // 10, clear[0]   # free flights cut through the sphere
    assert clear[1].min() > np.sqrt(SPHERE_R ** 2 - 1e-4) - 1e-6, clear[1].min()


def test_merit_derivative_with_the_sphere_is_the_derivative_of_the_merit():
    """phi' of altro_hip_merit (the user block's gradient through gen_al_col) against a central difference of phi."""
    batch = 256
    c = make_case(batch, toward_sphere=True)
    bt = make_hip(c)
    bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 3)
    bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.backward()
    assert (bt.get("status") == -1).all()
    for alpha in (0.3, 0.8):
        _, dphi = bt.merit(alpha)
        hs = 1e-6
        pp, _ = bt.merit(alpha + hs, derivative=False)
        pm, _ = bt.merit(alpha - hs, derivative=False)
        fd = (pp - pm) / (2 * hs)
        err = np.abs(dphi - fd) / np.maximum(1.0, np.abs(fd))
        assert err.max() < 1e-5, (alpha, err.max(), int(err.argmax()))
    bt.close()


@pytest.mark.parametrize("first", ["box", "box+halfplane"])
def test_a_block_added_after_a_solve_is_honoured(first):
    """Solve with an input box (all blocks bound-type: the row-layout kernels and the diagonal Hessian expansion serve that solve) or
    with the box and a general half-plane, add the sphere, solve again: the second solve is the solve of a fresh handle that had every
    block before its first."""
    batch = 64
    c = make_case(batch, seed=2, toward_sphere=True)
    Gbox = np.zeros((8, n + m)); gbox = np.zeros(8)
    for j in range(m):
        Gbox[j, n + j] = 1.0; Gbox[m + j, n + j] = -1.0
    gbox[:m] = [1.5 * HOVER[0], 0.05, 0.05, 0.05]; gbox[m:] = [0.0, 0.05, 0.05, 0.05]
    Ghp = np.zeros((1, n + m)); Ghp[0, 2] = 1.0; Ghp[0, 9] = 0.5

    def data_blocks(bt):
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, Gbox, gbox)
        if first == "box+halfplane":
            bt.add_linear_constraint(0, N, altro_amd.CONE_INEQUALITY, Ghp, np.array([1.0]))

    opts = dict(iterations_max=100, tol_stationarity=1e-3, penalty_initial=10.0)
    a = make_hip(c)
    data_blocks(a)
    a.ilqr_solve(**opts)
    a.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 3)
    a.reset_duals(1.0)   # (a solve starts from the penalty the last one left, as the reference's does: back to a fresh handle's)
    a.set_initial_state(c["x0"])
    a.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    ra = a.ilqr_solve(**opts)
    xa, _ = a.get_nominal()
    b = make_hip(c)
    data_blocks(b)
    b.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 3)
    rb = b.ilqr_solve(**opts)
    xb, _ = b.get_nominal()
    assert np.array_equal(ra["status"], rb["status"]) and np.array_equal(ra["iterations"], rb["iterations"])
    np.testing.assert_allclose(xa, xb, rtol=1e-12, atol=1e-12)
    ok = ra["status"] == 0
    assert ok.sum() >= batch // 2 and sphere_clearance(xa)[ok].min() > np.sqrt(SPHERE_R ** 2 - 1e-4) - 1e-6
    a.close(); b.close()


# ---- the surface ---------------------------------------------------------------------------------------------------------------
CHAIN12_SRC = r"""
// twelve states, four inputs: three double-integrated axes and three idle oscillators; block 0 keeps the first input below 1
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xd) {
  for (int i = 0; i < 3; ++i) { xd[i] = x[3 + i]; xd[3 + i] = u[i]; xd[6 + i] = x[9 + i]; xd[9 + i] = -x[6 + i] + T(0.1) * u[3]; }
}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {   // 12 x 16
  (void)x; (void)u;
  for (int e = 0; e < 12 * 16; ++e) J[e] = T(0);
  for (int i = 0; i < 3; ++i) {
    J[i + (3 + i) * 12] = T(1); J[(3 + i) + (12 + i) * 12] = T(1); J[(6 + i) + (9 + i) * 12] = T(1);
    J[(9 + i) + (6 + i) * 12] = T(-1); J[(9 + i) + 15 * 12] = T(0.1);
  }
}
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  (void)id; (void)x;
  c[0] = u[0] - T(1);
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // 1 x 16
  (void)id; (void)x; (void)u;
  for (int e = 0; e < 16; ++e) J[e] = T(0);
  J[12] = T(1);
}
"""


def test_the_surface_says_what_it_takes():
    # the tile's slots keep refusing, and name the plan that takes these blocks
    tile = altro_amd.Batch(20, 12, 4, 8, plan=altro_amd.PLAN_MFMA16)
    with pytest.raises(altro_amd.AltroHipError, match="plan GENERIC"):
        tile.set_model_source(CHAIN12_SRC, 0.05)
    tile.close()
    # an empty PLAN_AUTO handle of the (12, 4) tile moves to plan GENERIC and solves
    batch = 16
    bt = altro_amd.Batch(20, 12, 4, batch)
    assert bt.plan == altro_amd.PLAN_MFMA16
    bt.set_model_source(CHAIN12_SRC, 0.05)
    assert bt.plan == altro_amd.PLAN_GENERIC
    xref = np.zeros(12); xref[:3] = 1.0
    bt.set_tracking_cost(np.array([[1.0] * 12, [100.0] * 12]), np.array([[1e-2] * 4]), np.stack([xref, xref]), np.zeros((1, 4)),
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(np.zeros((batch, 12)))
    bt.set_input_guess(np.zeros((1, 1, 4)), k_stride_zero=True, batch_stride_zero=True)
    bt.add_user_constraint(0, 19, altro_amd.CONE_INEQUALITY, 1, 0)
    res = bt.ilqr_solve(iterations_max=100, tol_stationarity=1e-3)
    _, u = bt.get_nominal()
    assert (res["status"] == 0).all() and u[:, :, 0].max() < 1.0 + 1e-4
    # capacities: rows per block and per knot point
    with pytest.raises(altro_amd.AltroHipError, match="32"):
        bt.add_user_constraint(0, 19, altro_amd.CONE_INEQUALITY, 33, 0)
    bt.add_user_constraint(0, 3, altro_amd.CONE_INEQUALITY, 20, 0)
    with pytest.raises(altro_amd.AltroHipError, match="GEN_USER_MAXROWS"):
        bt.add_user_constraint(3, 5, altro_amd.CONE_INEQUALITY, 12, 0)
    bt.close()
    # a compiled-in model has no constraint source
    q = altro_amd.Batch(N, n, m, 4, plan=altro_amd.PLAN_GENERIC)
    q.set_model(altro_amd.MODEL_QUADROTOR13, H)
    with pytest.raises(altro_amd.AltroHipError, match=r"error -5: altro_hip_set_model_source must come first"):   # ALTRO_HIP_ERR_NOT_SET
        q.add_user_constraint(0, N, altro_amd.CONE_INEQUALITY, 1, 0)
    q.close()
    # a source that defines only one of the pair names the other
    half = CHAIN12_SRC.split("template <typename T> __device__ void altro_user_constraint_jacobian")[0]
    g = altro_amd.Batch(20, 12, 4, 4, plan=altro_amd.PLAN_GENERIC)
    with pytest.raises(altro_amd.AltroHipError, match="altro_user_constraint_jacobian"):
        g.set_model_source(half, 0.05)
    g.close()


def test_batch_solver_set_user_constraint_cpp():
    """BatchSolver::SetUserConstraint (include/altro_hip/altro_hip.hpp) on plan GENERIC: tests/cpp/batch_solver_user_constraint_test.cpp."""
    rc, out, err = cpp_build.run("batch_solver_user_constraint_test")
    assert rc == 0 and out.strip().endswith("PASS"), out + err
