#!/usr/bin/env python3
"""Batched linear TIME-VARYING MPC at (n, m) = (12, 4) on one MI355X: `batch` four-axis triple integrators whose velocity-to-position
coupling rotates with an angle of their own -- phase per system, advancing with time -- each following its OWN circular reference under
input bounds.  Every system carries its own A_k, B_k, f_k along the horizon and its own linear cost terms: dynamics given as data, plan
MFMA16, nothing shared by the batch.

    python examples/batched_ltv_mpc_12x4.py [batch] [steps] [--reupload | --no-check]

Default: the receding-horizon step moves the data on the device -- shift_trajectory, shift_dynamics, shift_linear_costs -- and writes only
the knot point that enters the horizon (set_dynamics_range and update_linear_costs on N-1 .. N).  --reupload poses the same problem the
only way it could be posed before: a full set_dynamics and a full update_linear_costs every step.  Both put identical data on the device,
so their closed loops are identical: the default run executes both and asserts it (--no-check skips the second run), and prints the
per-step time of the data update and of the solve for each.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import altro_amd  # noqa: E402

N, n, m, h = 40, 12, 4, 0.05
Qd = np.concatenate([10.0 * np.ones(4), np.ones(4), 0.1 * np.ones(4)])
Qf = 10.0 * Qd
Rd, umax = 1e-2 * np.ones(m), 6.0


class Systems:
    """The batch's data as functions of the absolute time index j (knot point k of the window that starts at step t is j = t + k)."""

    def __init__(self, batch):
        rng = np.random.default_rng(1)
        self.batch = batch
        self.phase = rng.uniform(0.0, 2.0 * np.pi, batch)
        self.radius = rng.uniform(0.5, 1.5, batch)
        self.x0 = np.concatenate([rng.uniform(-1, 1, (batch, 4)), np.zeros((batch, 8))], axis=1)

    def dynamics(self, j):
        """A [batch, 12, 12], B [batch, 12, 4], f [batch, 12] at time index j."""
        th = 0.3 * np.sin(0.5 * j * h + self.phase)
        c, s = np.cos(th), np.sin(th)
        rot = np.zeros((self.batch, 4, 4))
        rot[:, 0, 0] = c; rot[:, 0, 1] = -s; rot[:, 1, 0] = s; rot[:, 1, 1] = c
        rot[:, 2, 2] = c; rot[:, 2, 3] = -s; rot[:, 3, 2] = s; rot[:, 3, 3] = c
        I4 = np.eye(4)
        A = np.zeros((self.batch, n, n)); B = np.zeros((self.batch, n, m)); f = np.zeros((self.batch, n))
        A[:, :4, :4] = I4; A[:, :4, 4:8] = h * rot; A[:, :4, 8:] = 0.5 * h * h * rot
        A[:, 4:8, 4:8] = I4; A[:, 4:8, 8:] = h * I4; A[:, 8:, 8:] = I4
        B[:, :4] = h ** 3 / 6 * rot; B[:, 4:8] = 0.5 * h * h * I4; B[:, 8:] = h * I4
        f[:, 0] = 0.02 * h * np.cos(j * h + self.phase); f[:, 1] = 0.02 * h * np.sin(j * h + self.phase)
        return A, B, f

    def reference(self, j):
        """x_ref [batch, 12] at time index j: a circle of the system's own radius and phase, climbing slowly."""
        a = 0.3 * j * h + self.phase
        x = np.zeros((self.batch, n))
        x[:, 0] = self.radius * np.sin(a); x[:, 1] = self.radius * np.cos(a); x[:, 2] = 0.5 * np.sin(0.5 * a); x[:, 3] = 0.2 * j * h
        return x

    def packed(self, j):
        """The dynamics of time index j in the reference layout: column-major blocks [batch, 144], [batch, 48], [batch, 12]."""
        A, B, f = self.dynamics(j)
        return A.transpose(0, 2, 1).reshape(self.batch, -1), B.transpose(0, 2, 1).reshape(self.batch, -1), f

    def linear(self, j, terminal):
        """q [batch, 12], c [batch] of time index j as a running or the terminal knot point (u_ref = 0: r = 0)."""
        w, xr = (Qf if terminal else Qd), self.reference(j)
        return -(w * xr), 0.5 * (w * xr * xr).sum(axis=1)


def run(sys_, steps, reupload, quiet=False):
    batch = sys_.batch
    bt = altro_amd.Batch(N, n, m, batch)
    assert bt.plan == altro_amd.PLAN_MFMA16
    # host windows in the reference layout: dynamics [batch, N, .], linear terms [batch, N + 1, .]
    win = [np.stack(v, axis=1) for v in zip(*[sys_.packed(j) for j in range(N)])]
    lin = [sys_.linear(j, j == N) for j in range(N + 1)]
    q, c = np.stack([v[0] for v in lin], axis=1), np.stack([v[1] for v in lin], axis=1)
    bt.set_dynamics(*win)
    Qw = np.tile(Qd, (1, N + 1, 1)); Qw[0, N] = Qf
    bt.set_tracking_cost(Qw, np.tile(Rd, (1, N, 1)), np.zeros((1, N + 1, n)), np.zeros((1, N, m)), batch_stride_zero=True)
    bt.update_linear_costs(q, None, c, 0, N)                  # every system's own reference, from the same numbers either mode writes later
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)          # |u| <= umax
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G, np.full(2 * m, umax))
    x = sys_.x0.copy()
    bt.set_initial_state(x)
    bt.set_input_guess(np.zeros((1, 1, m)), k_stride_zero=True, batch_stride_zero=True)

    t_solve = t_data = 0.0
    us, iters = [], []
    for t in range(steps):
        bt.synchronize()
        t0 = time.perf_counter()
        res = bt.ilqr_solve(iterations_max=60, use_backtracking=True)
        t_solve += time.perf_counter() - t0
        _, u = bt.get_knot(0)
        us.append(u.copy()); iters.append(res["iterations"].copy())
        A, B, f = sys_.dynamics(t)                            # the plant: the model at the current time
        x = np.einsum("bij,bj->bi", A, x) + np.einsum("bij,bj->bi", B, u) + f
        if not quiet and (t % 10 == 0 or t == steps - 1):
            err = np.linalg.norm(x[:, :4] - sys_.reference(t + 1)[:, :4], axis=1)
            print("  step %3d: %5d/%d converged, iterations mean %.2f max %d, max |u| %.3f, position error mean %.3e"
                  % (t, int((res["status"] == 0).sum()), batch, res["iterations"].mean(), res["iterations"].max(), np.abs(u).max(), err.mean()))
        # the window moves on: time index t + N enters as knot point N-1, t + N + 1 as the terminal one
        new = [v[:, None] for v in sys_.packed(t + N)]
        qn = np.stack([sys_.linear(t + N, False)[0], sys_.linear(t + N + 1, True)[0]], axis=1)
        cn = np.stack([sys_.linear(t + N, False)[1], sys_.linear(t + N + 1, True)[1]], axis=1)
        if reupload:                                          # (the host keeps the window and hands all of it over)
            for w, v in zip(win, new):
                w[:, :-1] = w[:, 1:]; w[:, -1:] = v
            q[:, :N - 1] = q[:, 1:N]; q[:, N - 1:] = qn
            c[:, :N - 1] = c[:, 1:N]; c[:, N - 1:] = cn
        bt.set_initial_state(x)
        bt.shift_trajectory()
        bt.synchronize()
        t0 = time.perf_counter()
        if reupload:
            bt.set_dynamics(*win)
            bt.update_linear_costs(q, None, c, 0, N)
        else:
            bt.shift_dynamics()
            bt.set_dynamics_range(new[0], new[1], new[2], N - 1, N - 1)
            bt.shift_linear_costs()
            bt.update_linear_costs(qn, None, cn, N - 1, N)
        bt.synchronize()
        t_data += time.perf_counter() - t0
    bt.close()
    return dict(u=np.stack(us), iterations=np.stack(iters), x=x, data_ms=t_data / steps * 1e3, solve_ms=t_solve / steps * 1e3)


def report(name, r, steps, batch):
    print("%-44s data update %9.3f ms per step, solve %8.3f ms per step (%d steps x %d systems, N = %d, mean iterations %.2f)"
          % (name, r["data_ms"], r["solve_ms"], steps, batch, N, r["iterations"].mean()))


def main():
    flags = {a for a in sys.argv[1:] if a.startswith("--")}
    argv = [a for a in sys.argv[1:] if not a.startswith("--")]
    batch = int(argv[0]) if len(argv) > 0 else 4096
    steps = int(argv[1]) if len(argv) > 1 else 20
    sys_ = Systems(batch)
    if "--reupload" in flags:
        print("full set_dynamics + full update_linear_costs every step:")
        report("reupload", run(sys_, steps, True), steps, batch)
        return
    print("shift_dynamics + shift_linear_costs + one-knot-point writes:")
    a = run(sys_, steps, False)
    report("shifts + one-knot-point writes", a, steps, batch)
    if "--no-check" in flags:
        return
    b = run(sys_, steps, True, quiet=True)
    report("full set_dynamics + update_linear_costs", b, steps, batch)
    assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["iterations"], b["iterations"]) and np.array_equal(a["x"], b["x"]), \
        "the two modes' closed loops differ"
    print("closed loops identical: every u_0 and iteration count of %d steps; data update %.1f x faster" % (steps, b["data_ms"] / a["data_ms"]))


if __name__ == "__main__":
    main()
