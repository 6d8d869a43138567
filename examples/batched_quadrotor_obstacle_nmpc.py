#!/usr/bin/env python3
"""Batched NONLINEAR MPC with obstacle avoidance ON the (12, 4) tile: `batch` 12-state quadrotors, handed over as HIP source
(altro_hip_set_model_source), fly from around (-1.5, 0, 0) to hover at the origin; a keep-out sphere sits on the straight path.  The
thrust / torque box is a linear constraint block (one slot of eight rows); the sphere, r^2 - |p - c|^2 <= 0, is a constraint block from
the same source (altro_hip_add_user_constraint).  The handle is created with ALTRO_HIP_TILE_USER_BLOCKS, so it stays on plan MFMA16:
the sphere takes one of the knot points' six slots and is evaluated inside the row-layout kernels.  Every MPC step applies
u_0, shifts the horizon and re-solves warm-started.

    python examples/batched_quadrotor_obstacle_nmpc.py [batch] [steps] [--plan generic] [--no-obstacle] [--warm-duals] [--own-spheres]

--warm-duals carries the multipliers from one step to the next: instead of zeroing them after the shift (reset_duals), the duals move one
knot point forward with the trajectory (shift_duals) and the penalty goes back to the solve's penalty_initial (set_penalty).

--own-spheres gives every vehicle a sphere of its own: the centre moves sideways by up to +-0.15 over the batch and the radius runs from
0.25 to 0.35.  The source then reads (centre, radius) from four per-problem parameters (altro_hip_set_model_source_params /
altro_hip_set_model_params) -- one handle and one compile for 1024 different keep-out regions.

--plan generic runs the same problem on plan GENERIC's wave-per-problem kernels (where such a source went before the flag), so that the
two timings can be put side by side.  Prints the ms per NMPC step (median over the warm steps) with the mean iteration counts, and the
minimum clearance over the batch (the flown states and the last plans, less the sphere's radius: negative means inside).
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import altro_amd  # noqa: E402

N, n, m = 30, 12, 4
H = np.float32(0.02)
HOVER = np.array([0.5 * 9.81, 0.0, 0.0, 0.0])
CENTER, RADIUS = np.array([-0.75, 0.0, 0.0]), 0.3

SOURCE = r"""
// x = (p[3], Euler angles (phi, theta, psi), v[3], body rates[3]), u = (thrust, three body torques)
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, T* xd) {
  const T mass = T(0.5), g = T(9.81), Ix = T(0.0023), Iy = T(0.0023), Iz = T(0.004);
  T sp, cp, st, ct, ss, cs;
  sincos(x[3], &sp, &cp); sincos(x[4], &st, &ct); sincos(x[5], &ss, &cs);
  const T tt = st / ct, wx = x[9], wy = x[10], wz = x[11];
  xd[0] = x[6]; xd[1] = x[7]; xd[2] = x[8];
  xd[3] = wx + sp * tt * wy + cp * tt * wz;
  xd[4] = cp * wy - sp * wz;
  xd[5] = (sp * wy + cp * wz) / ct;
  const T a = u[0] / mass;
  xd[6] = a * (cp * st * cs + sp * ss);
  xd[7] = a * (cp * st * ss - sp * cs);
  xd[8] = a * (cp * ct) - g;
  xd[9] = (u[1] - (Iz - Iy) * wy * wz) / Ix;
  xd[10] = (u[2] - (Ix - Iz) * wz * wx) / Iy;
  xd[11] = (u[3] - (Iy - Ix) * wx * wy) / Iz;
}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, T* J) {
  const T mass = T(0.5), Ix = T(0.0023), Iy = T(0.0023), Iz = T(0.004);
  T sp, cp, st, ct, ss, cs;
  sincos(x[3], &sp, &cp); sincos(x[4], &st, &ct); sincos(x[5], &ss, &cs);
  const T tt = st / ct, sec2 = T(1) / (ct * ct), wx = x[9], wy = x[10], wz = x[11];
  for (int e = 0; e < 192; ++e) J[e] = T(0);
  J[0 + 6 * 12] = T(1); J[1 + 7 * 12] = T(1); J[2 + 8 * 12] = T(1);
  J[3 + 3 * 12] = cp * tt * wy - sp * tt * wz; J[3 + 4 * 12] = (sp * wy + cp * wz) * sec2;
  J[3 + 9 * 12] = T(1); J[3 + 10 * 12] = sp * tt; J[3 + 11 * 12] = cp * tt;
  J[4 + 3 * 12] = -sp * wy - cp * wz; J[4 + 10 * 12] = cp; J[4 + 11 * 12] = -sp;
  J[5 + 3 * 12] = (cp * wy - sp * wz) / ct; J[5 + 4 * 12] = (sp * wy + cp * wz) * st * sec2;
  J[5 + 10 * 12] = sp / ct; J[5 + 11 * 12] = cp / ct;
  const T a = u[0] / mass;
  J[6 + 3 * 12] = a * (-sp * st * cs + cp * ss); J[6 + 4 * 12] = a * (cp * ct * cs); J[6 + 5 * 12] = a * (-cp * st * ss + sp * cs);
  J[6 + 12 * 12] = (cp * st * cs + sp * ss) / mass;
  J[7 + 3 * 12] = a * (-sp * st * ss - cp * cs); J[7 + 4 * 12] = a * (cp * ct * ss); J[7 + 5 * 12] = a * (cp * st * cs + sp * ss);
  J[7 + 12 * 12] = (cp * st * ss - sp * cs) / mass;
  J[8 + 3 * 12] = a * (-sp * ct); J[8 + 4 * 12] = a * (-cp * st); J[8 + 12 * 12] = (cp * ct) / mass;
  J[9 + 10 * 12] = -(Iz - Iy) * wz / Ix; J[9 + 11 * 12] = -(Iz - Iy) * wy / Ix; J[9 + 13 * 12] = T(1) / Ix;
  J[10 + 9 * 12] = -(Ix - Iz) * wz / Iy; J[10 + 11 * 12] = -(Ix - Iz) * wx / Iy; J[10 + 14 * 12] = T(1) / Iy;
  J[11 + 9 * 12] = -(Iy - Ix) * wy / Iz; J[11 + 10 * 12] = -(Iy - Ix) * wx / Iz; J[11 + 15 * 12] = T(1) / Iz;
}
// block 0: the keep-out sphere of radius 0.3 around (-0.75, 0, 0)
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - T(-0.75), dy = x[1], dz = x[2];
  c[0] = T(0.09) - dx * dx - dy * dy - dz * dz;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // 1 x 16
  (void)id; (void)u;
  for (int e = 0; e < 16; ++e) J[e] = T(0);
  J[0] = -T(2) * (x[0] - T(-0.75)); J[1] = -T(2) * x[1]; J[2] = -T(2) * x[2];
}
"""


def own_sphere_source(src):
    """SOURCE with the sphere read from the problem's parameters p = (centre x, y, z, radius): the four functions take `const T* p`."""
    out = src.replace("const T* x, const T* u, T* xd)", "const T* x, const T* u, const T* p, T* xd)")
    out = out.replace("const T* x, const T* u, T* J)", "const T* x, const T* u, const T* p, T* J)")
    out = out.replace("const T* x, const T* u, T* c)", "const T* x, const T* u, const T* p, T* c)")
    out = out.replace("const T dx = x[0] - T(-0.75), dy = x[1], dz = x[2];", "const T dx = x[0] - p[0], dy = x[1] - p[1], dz = x[2] - p[2];")
    out = out.replace("c[0] = T(0.09) - dx * dx", "c[0] = p[3] * p[3] - dx * dx")
    out = out.replace("J[0] = -T(2) * (x[0] - T(-0.75)); J[1] = -T(2) * x[1]; J[2] = -T(2) * x[2];",
                      "J[0] = -T(2) * (x[0] - p[0]); J[1] = -T(2) * (x[1] - p[1]); J[2] = -T(2) * (x[2] - p[2]);")
    assert out.count("const T* p") == 4 and "T(-0.75)" not in out and "T(0.09)" not in out
    return out


def clearance(p, center=CENTER, radius=RADIUS):
    """distance to the sphere's surface of positions p[batch, ..., 3]; center [3] / radius, or one per vehicle ([batch, 3] / [batch])"""
    c = np.asarray(center)
    if c.ndim == 2:
        c = c.reshape((c.shape[0],) + (1,) * (p.ndim - 2) + (3,))
        radius = np.asarray(radius).reshape((c.shape[0],) + (1,) * (p.ndim - 2))
    return np.linalg.norm(p - c, axis=-1) - radius


def main():
    args = sys.argv[1:]
    generic = "--plan" in args and args[args.index("--plan") + 1].lower() == "generic"
    if "--plan" in args:
        del args[args.index("--plan"):args.index("--plan") + 2]
    argv = [a for a in args if not a.startswith("--")]
    batch = int(argv[0]) if argv else 1024
    steps = int(argv[1]) if len(argv) > 1 else 8
    obstacle = "--no-obstacle" not in args
    warm_duals = "--warm-duals" in args
    own = "--own-spheres" in args and obstacle
    rng = np.random.default_rng(5)
    x0 = np.zeros((batch, n))
    x0[:, :3] = np.array([-1.5, 0.0, 0.0]) + 0.05 * rng.standard_normal((batch, 3))
    Qd = np.concatenate([np.full(3, 2.0), np.full(3, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
    Rd = np.array([0.05, 20.0, 20.0, 20.0])

    if generic:
        bt = altro_amd.Batch(N, n, m, batch, plan=altro_amd.PLAN_GENERIC)
    else:
        bt = altro_amd.Batch(N, n, m, batch, flags=altro_amd.TILE_USER_BLOCKS)
    # 0.6 hover <= thrust <= 1.25 hover, |torques| <= 0.05: eight rows, one slot
    Gb = np.zeros((2 * m, n + m)); Gb[:m, n:] = np.eye(m); Gb[m:, n:] = -np.eye(m)
    gb = np.concatenate([[1.25 * HOVER[0], 0.05, 0.05, 0.05], [-0.6 * HOVER[0], 0.05, 0.05, 0.05]])
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, Gb, gb)
    bt.set_tracking_cost(np.stack([Qd, 20.0 * Qd]), Rd[None], np.zeros((2, n)), HOVER[None], k_stride_zero=True, batch_stride_zero=True)
    center, radius = CENTER, RADIUS
    if own:
        center = np.tile(CENTER, (batch, 1)); center[:, 1] += 0.15 * np.linspace(-1.0, 1.0, batch)
        radius = np.linspace(0.25, 0.35, batch)
        bt.set_model_source(own_sphere_source(SOURCE), H, num_params=4)
        bt.set_model_params(np.concatenate([center, radius[:, None]], axis=1))
    else:
        bt.set_model_source(SOURCE, H)
    if obstacle:
        bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 0)
    bt.set_initial_state(x0)
    bt.set_input_guess(HOVER[None, None], k_stride_zero=True, batch_stride_zero=True)
    opts = dict(iterations_max=60, tol_stationarity=1e-3, penalty_initial=10.0)
    plan = {altro_amd.PLAN_MFMA16: "MFMA16", altro_amd.PLAN_GENERIC: "GENERIC"}.get(bt.plan, str(bt.plan))
    print("%d vehicles, (n, m) = (%d, %d), N = %d, plan %s, keep-out sphere %s" % (batch, n, m, N, plan, ("one per vehicle" if own else "on") if obstacle else "off"))

    t0 = time.perf_counter(); res = bt.ilqr_solve(**opts); bt.synchronize()
    print("first solve: %.2f ms, %d of %d converged" % ((time.perf_counter() - t0) * 1e3, int((res["status"] == 0).sum()), batch))
    flown = [x0[:, :3]]
    ts, its = [], []
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
        its.append(float(res["iterations"].mean()))
        print("step %d: %.2f ms, mean iterations %.2f, %d converged; %d sweeps, mean dual updates %.2f, worst feasibility %.2e"
              % (step, ts[-1], its[-1], int((res["status"] == 0).sum()), res["sweeps"], float(res["dual_updates"].mean()), float(res["feasibility"].max())))
    x, _ = bt.get_nominal()
    cl = min(clearance(np.stack(flown, axis=1), center, radius).min(), clearance(x[:, :, :3], center, radius).min())
    ok = res["status"] == 0
    cl_ok = float("nan")
    if ok.any():
        cl_ok = clearance(x[ok][:, :, :3], center[ok] if own else center, radius[ok] if own else radius).min()
    print("duals after the shift: %s" % ("shifted with the trajectory (--warm-duals)" if warm_duals else "reset to zero"))
    print("plan %s, %d vehicles: median NMPC step %.2f ms (mean iterations over the warm steps %.2f); minimum clearance over the batch %+.4f, "
          "over the last solve's converged plans %+.4f (sphere radius %s)" % (plan, batch, sorted(ts)[len(ts) // 2], float(np.mean(its)), cl, cl_ok, "0.25 .. 0.35, one per vehicle" if own else "%.2f" % RADIUS))
    bt.close()


if __name__ == "__main__":
    main()
