#!/usr/bin/env python3
"""Batched NONLINEAR MPC with obstacle avoidance past the (12, 4) tile: `batch` 13-state quaternion quadrotors, handed over as HIP
source (altro_hip_set_model_source), fly from around (-1.5, 0, 0) to hover at the origin; a keep-out sphere sits on the straight
path.  The thrust box is a linear constraint block; the sphere, r^2 - |p - c|^2 <= 0, is a constraint block from the same source
(altro_hip_add_user_constraint): hiprtc compiles it into plan GENERIC's AL kernels, and the ALTRO_HIP_PLAN_AUTO handle runs plan MFMA32
(the sweeps on matrix-core tiles).  Every MPC step applies u_0, shifts the horizon and re-solves warm-started.

    python examples/batched_quadrotor13_obstacle_nmpc.py [batch] [steps] [--no-obstacle] [--warm-duals]

--warm-duals: after the shift the duals move one knot point forward with the trajectory (shift_duals) and the penalty goes back to the
solve's penalty_initial (set_penalty), instead of the duals being zeroed (reset_duals).

Prints the ms per NMPC step (median over the warm steps) and the minimum clearance over the batch (the flown states and the last
plans, less the sphere's radius: negative means inside).
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import altro_amd  # noqa: E402

N, n, m = 30, 13, 4
H = np.float32(0.02)
HOVER = np.array([0.5 * 9.81, 0.0, 0.0, 0.0])
CENTER, RADIUS = np.array([-0.75, 0.0, 0.0]), 0.3

SOURCE = r"""
// x = (p[3], q[4] (w, x, y, z), v[3], omega[3]), u = (thrust, three body torques)
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
__device__ void altro_user_jacobian(const T* x, const T* u, T* J) {   // 13 x 17, column-major
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
// block 0: the keep-out sphere of radius 0.3 around (-0.75, 0, 0)
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - T(-0.75), dy = x[1], dz = x[2];
  c[0] = T(0.09) - dx * dx - dy * dy - dz * dz;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // 1 x 17
  (void)id; (void)u;
  for (int e = 0; e < 17; ++e) J[e] = T(0);
  J[0] = -T(2) * (x[0] - T(-0.75)); J[1] = -T(2) * x[1]; J[2] = -T(2) * x[2];
}
"""


def clearance(p):
    """distance to the sphere's surface of positions p[..., 3]"""
    return np.linalg.norm(p - CENTER, axis=-1) - RADIUS


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    batch = int(argv[0]) if argv else 1024
    steps = int(argv[1]) if len(argv) > 1 else 8
    obstacle = "--no-obstacle" not in sys.argv
    warm_duals = "--warm-duals" in sys.argv
    rng = np.random.default_rng(5)
    x0 = np.zeros((batch, n))
    x0[:, :3] = np.array([-1.5, 0.0, 0.0]) + 0.05 * rng.standard_normal((batch, 3))
    x0[:, 3] = 1.0
    xref = np.zeros(n); xref[3] = 1.0
    Qd = np.concatenate([np.full(3, 2.0), np.full(4, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
    Rd = np.array([0.05, 20.0, 20.0, 20.0])

    bt = altro_amd.Batch(N, n, m, batch)
    bt.set_model_source(SOURCE, H)
    bt.set_tracking_cost(np.stack([Qd, 20.0 * Qd]), Rd[None], np.stack([xref, xref]), HOVER[None], k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(x0)
    bt.set_input_guess(HOVER[None, None], k_stride_zero=True, batch_stride_zero=True)
    Gb = np.zeros((2, n + m)); Gb[0, n] = 1.0; Gb[1, n] = -1.0       # 0.6 hover <= thrust <= 1.25 hover
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, Gb, np.array([1.25 * HOVER[0], -0.6 * HOVER[0]]))
    if obstacle:
        bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 0)
    opts = dict(iterations_max=60, tol_stationarity=1e-3, penalty_initial=10.0)
    plan = {altro_amd.PLAN_MFMA32: "MFMA32", altro_amd.PLAN_GENERIC: "GENERIC"}.get(bt.plan, str(bt.plan))
    print("%d vehicles, (n, m) = (%d, %d), N = %d, plan %s, keep-out sphere %s" % (batch, n, m, N, plan, "on" if obstacle else "off"))

    t0 = time.perf_counter(); res = bt.ilqr_solve(**opts); bt.synchronize()
    print("first solve: %.2f ms, %d of %d converged" % ((time.perf_counter() - t0) * 1e3, int((res["status"] == 0).sum()), batch))
    flown = [x0[:, :3]]
    ts = []
    for step in range(steps):
        x1, _ = bt.get_knot(1)           # the plant follows the plan's first step (the model is the plant)
        flown.append(x1[:, :3])
        bt.set_initial_state(x1)
        bt.shift_trajectory()
        if warm_duals:   # the duals follow their knot points; the penalty starts over
            bt.shift_duals(altro_amd.DUAL_TAIL_KEEP)
            bt.set_penalty(opts["penalty_initial"])
        else:
            bt.reset_duals(opts["penalty_initial"])   # (the duals belong to the previous horizon's knot points)
        bt.synchronize(); t0 = time.perf_counter()
        res = bt.ilqr_solve(**opts); bt.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        print("step %d: %.2f ms, mean iterations %.2f, %d converged" % (step, ts[-1], float(res["iterations"].mean()), int((res["status"] == 0).sum())))
    x, _ = bt.get_nominal()
    cl = min(clearance(np.stack(flown, axis=1)).min(), clearance(x[:, :, :3]).min())
    ok = res["status"] == 0
    cl_ok = clearance(x[ok][:, :, :3]).min() if ok.any() else float("nan")
    print("median NMPC step %.2f ms; minimum clearance over the batch %+.4f, over the last solve's converged plans %+.4f "
          "(sphere radius %.2f)" % (sorted(ts)[len(ts) // 2], cl, cl_ok, RADIUS))
    bt.close()


if __name__ == "__main__":
    main()
