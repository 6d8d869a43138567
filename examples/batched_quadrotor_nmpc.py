#!/usr/bin/env python3
"""Batched NONLINEAR MPC at (n, m) = (12, 4) on one MI355X: `batch` quadrotors (the 12-state rigid-body model of
altro_amd/csrc/models.h; thrust and three body torques) fly a moving set-point under thrust and torque bounds.  The dynamics
are a device model (altro_hip_set_model on plan MFMA16): every rollout, merit evaluation and expansion steps the model on the
GPU in the tile plan's row layout, the backward sweeps are the benchmarked matrix-core kernel.

    python examples/batched_quadrotor_nmpc.py [batch] [steps] [sweeps-per-step] [--source] [--time-grid FINE:COARSE] [--mass-spread S]

`sweeps-per-step` caps iLQR sweeps per MPC step (real-time iteration; default 3): a batch waits for its slowest problem, and a
receding-horizon controller re-plans 50 times a second anyway.

`--time-grid FINE:COARSE` (FINE + 4 COARSE = 40) runs the same 0.8 s look-ahead a second time on FINE steps of h followed by COARSE
steps of 4 h (altro_hip_set_time_steps; ALTROSolver::SetTimeStep per knot-point range) -- FINE + COARSE knot points instead of 40 --
and prints its time per NMPC step and closed-loop tracking error next to the uniform run's.  The grid is relative to "now": it does
not move with the horizon, and such a run warm-starts from the previous plan as it is (one knot point of the coarse tail is four
plant steps: there is no whole-knot shift).

`--source --mass-spread S` gives every vehicle its own mass, 0.5 (1 - S) .. 0.5 (1 + S) over the batch -- a fleet with different
payloads on ONE handle and one compile: the source takes the mass as a per-problem parameter (altro_hip_set_model_source_params /
altro_hip_set_model_params), and each vehicle's hover thrust centres its input cost and its thrust bounds.  S = 0 runs the
parametrised source with equal masses: against plain `--source` that is the cost of the parameters themselves.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import altro_amd  # noqa: E402

MASS, GRAV, IX, IY, IZ = 0.5, 9.81, 0.0023, 0.0023, 0.004


def f_cont(x, u, mass=MASS):
    """the model's continuous dynamics for the plant (the same equations, numpy, whole batch; mass: one number or one per vehicle)"""
    sp, cp, st, ct, ss, cs = np.sin(x[:, 3]), np.cos(x[:, 3]), np.sin(x[:, 4]), np.cos(x[:, 4]), np.sin(x[:, 5]), np.cos(x[:, 5])
    tt = st / ct
    wx, wy, wz = x[:, 9], x[:, 10], x[:, 11]
    a = u[:, 0] / mass
    return np.stack([x[:, 6], x[:, 7], x[:, 8],
                     wx + sp * tt * wy + cp * tt * wz, cp * wy - sp * wz, (sp * wy + cp * wz) / ct,
                     a * (cp * st * cs + sp * ss), a * (cp * st * ss - sp * cs), a * (cp * ct) - GRAV,
                     (u[:, 1] - (IZ - IY) * wy * wz) / IX, (u[:, 2] - (IX - IZ) * wz * wx) / IY, (u[:, 3] - (IY - IX) * wx * wy) / IZ], axis=1)


def plant(x, u, h, mass=MASS):   # explicit midpoint, like the solver's discretisation (test/test_utils.cpp:84-132)
    return x + h * f_cont(x + 0.5 * h * f_cont(x, u, mass), u, mass)


def source_with_mass_parameter(src):
    """The quadrotor source with its mass read from p[0]: both functions take `const T* p`, everything else is the text as it stands."""
    out = src.replace("const T mass = T(0.5),", "const T mass = p[0],")
    out = out.replace("const T* x, const T* u, T* xd)", "const T* x, const T* u, const T* p, T* xd)")
    out = out.replace("const T* x, const T* u, T* J)", "const T* x, const T* u, const T* p, T* J)")
    assert out.count("p[0]") == 2 and out.count("const T* p") == 2
    return out


def run(batch, steps, sweeps, from_source, grid=None, spread=None):
    """One closed-loop run; grid = (fine, coarse) knot points of h and 4 h, or None: 40 of h; spread: None, or the masses' relative
    spread over the batch (the source then takes the mass as a parameter).  -> (ms per step, mean position error)"""
    n, m, h = 12, 4, 0.02
    iters = 0.0
    N = 40 if grid is None else grid[0] + grid[1]
    hk = np.full(N, h) if grid is None else np.concatenate([np.full(grid[0], h), np.full(grid[1], 4 * h)])
    tk = np.concatenate([[0.0], np.cumsum(hk)])   # knot point k lies tk[k] ahead of "now"
    mass = np.full(batch, MASS) if spread is None else MASS * (1.0 + spread * np.linspace(-1.0, 1.0, batch))
    hover = np.zeros((batch, m)); hover[:, 0] = mass * GRAV          # every vehicle's own hover thrust
    Qd = np.concatenate([np.full(3, 4.0), np.full(3, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
    Rd = np.array([0.05, 20.0, 20.0, 20.0])
    rng = np.random.default_rng(3)
    x = np.zeros((batch, n))
    x[:, :3] = rng.uniform(-1.0, 1.0, (batch, 3))
    x[:, 3:6] = rng.uniform(-0.2, 0.2, (batch, 3))
    x[:, 6:9] = rng.uniform(-0.5, 0.5, (batch, 3))
    goal = lambda t: np.concatenate([np.array([np.sin(0.8 * t), np.cos(0.8 * t) - 1.0, 0.3 * np.sin(0.4 * t)]), np.zeros(9)])  # noqa: E731

    bt = altro_amd.Batch(N, n, m, batch)
    assert bt.plan == altro_amd.PLAN_MFMA16
    if from_source:
        from tests.test_gpu_tile_model import QUADROTOR_SRC
        if spread is None:
            bt.set_model_source(QUADROTOR_SRC, np.float32(h))
        else:
            bt.set_model_source(source_with_mass_parameter(QUADROTOR_SRC), np.float32(h), num_params=1)
            bt.set_model_params(mass[:, None])
    else:
        bt.set_model(altro_amd.MODEL_QUADROTOR, np.float32(h))
    if grid is not None:
        bt.set_time_steps(hk.astype(np.float32))
    xref = np.stack([goal(tk[k]) for k in range(N + 1)])
    Q = np.tile(Qd, (1, N + 1, 1)); Q[0, N] *= 10.0
    if spread is None:
        bt.set_tracking_cost(Q, np.tile(Rd, (1, N, 1)), xref[None], np.tile(hover[0], (1, N, 1)), batch_stride_zero=True)
    else:
        bt.set_tracking_cost(np.tile(Q, (batch, 1, 1)), np.tile(Rd, (batch, N, 1)), np.tile(xref, (batch, 1, 1)), np.repeat(hover[:, None], N, axis=1))
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    bnd = np.array([3.0, 0.05, 0.05, 0.05])                       # |F - m g| <= 3 N, |tau| <= 0.05 N m
    if spread is None:
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G[:m], hover[0] + bnd)
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G[m:], -(hover[0] - bnd))
    else:                                                          # (right-hand sides per problem)
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G[:m], hover + bnd)
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G[m:], -(hover - bnd))
    bt.set_initial_state(x)
    if spread is None:
        bt.set_input_guess(hover[:1, None], k_stride_zero=True, batch_stride_zero=True)
    else:
        bt.set_input_guess(hover[:, None], k_stride_zero=True)

    t_solve, err_sum = 0.0, 0.0
    for t in range(steps):
        t0 = time.perf_counter()
        res = bt.ilqr_solve(iterations_max=(20 if t == 0 else sweeps), tol_stationarity=1e-3, use_backtracking=True)
        dt = time.perf_counter() - t0
        if t > 0:
            t_solve += dt
            iters += res["iterations"].mean()
        _, u = bt.get_knot(0)
        x = plant(x, u, h, mass)
        err = np.linalg.norm(x[:, :3] - goal((t + 1) * h)[:3], axis=1)
        err_sum += err.mean()
        if t % 10 == 0 or t == steps - 1:
            print("step %3d: %.2f ms, %5d/%d converged, sweeps %d, thrust in [%.2f, %.2f], max |tau| %.3f, position error mean %.3f max %.3f"
                  % (t, dt * 1e3, int((res["status"] == 0).sum()), batch, res["sweeps"], u[:, 0].min(), u[:, 0].max(), np.abs(u[:, 1:]).max(),
                     err.mean(), err.max()))
        xr = np.stack([goal((t + 1) * h + tk[k]) for k in range(N + 1)])
        Qk = np.tile(Qd, (N + 1, 1)); Qk[N] *= 10.0
        bt.update_linear_costs(-(Qk * xr)[None], None, (0.5 * (Qk * xr * xr).sum(1))[None], 0, N, batch_stride_zero=True)
        bt.set_initial_state(x)
        if grid is None:
            bt.shift_trajectory()
    print("%d NMPC steps x %d quadrotors (n=12, m=4, N=%d, %s, <= %d sweeps per step): %.2f ms per step in the solver (%.0f solves/s)"
          % (steps - 1, batch, N, "h=%.2f" % h if grid is None else "%d steps of %.2f + %d of %.2f" % (grid[0], h, grid[1], 4 * h), sweeps,
             t_solve / (steps - 1) * 1e3, (steps - 1) * batch / t_solve))
    if spread is not None:
        print("masses %.3f .. %.3f kg as a per-problem parameter of the source: %.2f ms per NMPC step, mean iterations %.2f, mean position error %.4f"
              % (mass.min(), mass.max(), t_solve / (steps - 1) * 1e3, iters / (steps - 1), err_sum / steps))
    else:
        print("mean iterations %.2f" % (iters / (steps - 1)))
    bt.close()
    return t_solve / (steps - 1) * 1e3, err_sum / steps


def main():
    argv = [a for i, a in enumerate(sys.argv) if not a.startswith("--") and (i == 0 or sys.argv[i - 1] not in ("--time-grid", "--mass-spread"))]
    batch = int(argv[1]) if len(argv) > 1 else 4096
    steps = int(argv[2]) if len(argv) > 2 else 50
    sweeps = int(argv[3]) if len(argv) > 3 else 3
    from_source = "--source" in sys.argv          # the same model handed over as HIP source (altro_hip_set_model_source: hiprtc)
    grid = None
    if "--time-grid" in sys.argv:
        fine, coarse = (int(v) for v in sys.argv[sys.argv.index("--time-grid") + 1].split(":"))
        if fine < 1 or coarse < 0 or fine + 4 * coarse != 40:
            sys.exit("--time-grid FINE:COARSE needs FINE + 4 COARSE = 40 (the uniform run's look-ahead), e.g. 8:8 or 12:7")
        grid = (fine, coarse)
    spread = None
    if "--mass-spread" in sys.argv:
        spread = float(sys.argv[sys.argv.index("--mass-spread") + 1])
        if not from_source or not 0.0 <= spread < 1.0:
            sys.exit("--mass-spread S needs --source (the mass is a parameter of the source) and 0 <= S < 1")
    ms_u, err_u = run(batch, steps, sweeps, from_source, spread=spread)
    if grid is not None:
        ms_g, err_g = run(batch, steps, sweeps, from_source, grid, spread)
        print("uniform 40 x h: %.2f ms per NMPC step, mean position error %.4f | grid %d x h + %d x 4h (%d knot points): %.2f ms per NMPC step, "
              "mean position error %.4f" % (ms_u, err_u, grid[0], grid[1], grid[0] + grid[1], ms_g, err_g))


if __name__ == "__main__":
    main()
