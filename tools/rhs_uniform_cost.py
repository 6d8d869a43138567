#!/usr/bin/env python3
"""What leaving the tables' uniform path costs: a handle whose constraint block carries a right-hand side per knot point
(altro_hip_add_linear_constraint_rhs, ALTRO_HIP_RHS_PER_KNOT) reads every knot point's own table record; with the SAME value at every
knot point it solves the same problem as the handle with one shared g, whose kernels read knot point 0's record throughout.  Both
handles in one process, solves in alternation, medians after warm-up:

    python tools/rhs_uniform_cost.py [solves = 21]

  C1 + input box    the (12, 4) tile, N = 256, 4096 problems (tools/c1_solve.py --al)
  bicycles          plan LANE, N = 50, 8192 vehicles with the steering bound (tests/test_gpu_al.py's C3 setup)
  (13, 4) + box     plan MFMA32, N = 64, 1024 problems with an input box
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import altro_amd  # noqa: E402
from tests import mpc_common as M  # noqa: E402
from tests import problems  # noqa: E402


def input_box(n, m):
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    return G


def c1(per_knot):
    N, n, m, batch = 256, 12, 4, 4096
    one = problems.c1_double_integrator(1, N=N)
    bt = altro_amd.Batch(N, n, m, batch)
    bt.set_dynamics(one["A"][0, :1], one["B"][0, :1], None, k_stride_zero=True, batch_stride_zero=True)
    bt.set_tracking_cost(np.stack([np.ones(n), 100.0 * np.ones(n)]), np.full((1, m), 1e-2), np.zeros((2, n)), np.zeros((1, m)),
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(2.0 * problems.uniform01((batch, n), 21) - 1.0)
    g = np.full(2 * m, 2.0)
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, input_box(n, m), np.tile(g, (N, 1)) if per_knot else g, per_knot=per_knot)
    guess = lambda: bt.set_input_guess(np.zeros((1, 1, m)), k_stride_zero=True, batch_stride_zero=True)   # noqa: E731
    return bt, guess, dict(iterations_max=40)


def bicycles(per_knot):
    N, n, m, batch = 50, 4, 2, 8192
    x_ref, u_ref = problems.bicycle_reference(N + 1)
    bt = altro_amd.Batch(N, n, m, batch)
    bt.set_model(altro_amd.MODEL_BICYCLE, np.float32(0.1))
    bt.set_tracking_cost(np.full((1, N + 1, n), 1e-2), np.full((1, N, m), 1e-3), x_ref[None, :N + 1], u_ref[None, :N], batch_stride_zero=True)
    cone, G, g = M.steering_block()
    g = np.full(2, 0.02)                                         # (active: tests/test_gpu_dual_warmstart.py's bound)
    bt.add_linear_constraint(0, N, cone, G, np.tile(g, (N + 1, 1)) if per_knot else g, per_knot=per_knot)
    bt.set_initial_state(x_ref[0] + (problems.uniform01((batch, n), 23) - 0.5) * 0.4)
    guess = lambda: bt.set_input_guess(np.array([[[u_ref[0][0], 0.0]]]), k_stride_zero=True, batch_stride_zero=True)   # noqa: E731
    return bt, guess, dict(iterations_max=40, use_backtracking=True)


def wave13(per_knot):
    N, n, m, batch = 64, 13, 4, 1024
    p = problems.ilqr12x4_problem(batch, N, True, n=n, m=m)
    bt = altro_amd.Batch(N, n, m, batch)
    assert bt.plan == altro_amd.PLAN_MFMA32
    bt.set_dynamics(p["A"], p["B"], p["f"])
    bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
    bt.set_initial_state(p["x0"])
    g = np.full(2 * m, 0.3)
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, input_box(n, m), np.tile(g, (N, 1)) if per_knot else g, per_knot=per_knot)
    guess = lambda: bt.set_input_guess(p["u0"])   # noqa: E731
    return bt, guess, dict(iterations_max=40, use_backtracking=True)


def main():
    solves = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    for name, make in (("C1 + input box, tile, N 256 x 4096", c1), ("bicycles + steering bound, LANE, N 50 x 8192", bicycles), ("(13, 4) + input box, MFMA32, N 64 x 1024", wave13)):
        pair = [make(False), make(True)]
        ts, last = [[], []], [None, None]
        for i in range(solves + 2):                              # two warm-up rounds
            for v, (bt, guess, opts) in enumerate(pair):
                guess()
                bt.reset_duals(1.0)
                bt.synchronize()
                t0 = time.perf_counter()
                last[v] = bt.ilqr_solve(**opts)
                bt.synchronize()
                if i >= 2:
                    ts[v].append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(last[0][key], last[1][key]) for key in ("status", "iterations", "dual_updates"))
        xs = [bt.get_nominal()[0] for bt, _, _ in pair]
        med = [float(np.median(t)) for t in ts]
        print("%-46s shared g (uniform) %8.3f ms [%.3f .. %.3f]   per knot point (not uniform) %8.3f ms [%.3f .. %.3f]   ratio %.3f   sweeps %d, converged %d of %d, "
              "same iterations %s, max |x difference| %.1e"
              % (name, med[0], min(ts[0]), max(ts[0]), med[1], min(ts[1]), max(ts[1]), med[1] / med[0], last[0]["sweeps"], int((last[0]["status"] == 0).sum()),
                 len(last[0]["status"]), same, float(np.abs(xs[0] - xs[1]).max())), flush=True)
        for bt, _, _ in pair:
            bt.close()


if __name__ == "__main__":
    main()
