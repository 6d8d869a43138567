#!/usr/bin/env python3
"""What a constraint block from source costs the merit evaluation of plan GENERIC: generic_merit_kernel with derivative at (13, 4),
N = 128, on a batch of quadrotors from source, with the keep-out sphere as a one-row block from the source against a one-row linear
block -- both on the wave-per-problem kernel (ALTRO_HIP_FORM_GENERIC_MERIT_LDS).  Host clock per altro_hip_merit call (one launch and
the copy of phi / phi'), median of `reps`.

    python tools/user_constraint_merit_time.py [batch] [reps]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import altro_amd  # noqa: E402
from tests.test_gpu_generic_user_constraint import H, QUADROTOR13_SRC, make_case, m, n  # noqa: E402

N = 128
SRC_NO_CONSTRAINTS = QUADROTOR13_SRC.split("template <typename T> __device__ void altro_user_constraint(")[0]

argv = sys.argv[1:]
batch = int(argv[0]) if argv else 4096
reps = int(argv[1]) if len(argv) > 1 else 30
c = make_case(batch, toward_sphere=True)


def merit_ms(src, user):
    bt = altro_amd.Batch(N, n, m, batch)
    bt.set_forms(altro_amd.FORM_GENERIC_MERIT_LDS)
    bt.set_model_source(src, H)
    bt.set_tracking_cost(np.stack([c["Qd"], c["Qfd"]]), c["Rd"][None], np.stack([c["xref"], c["xref"]]), c["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(c["x0"])
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    if user:
        bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 3)
    else:   # the sphere's tangent plane at the start: one row, not bound-type
        G = np.zeros((1, n + m)); G[0, 0] = -1.0; G[0, 1] = 0.1
        bt.add_linear_constraint(1, N, altro_amd.CONE_INEQUALITY, G, np.array([0.5]))
    bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.backward()
    for _ in range(3):
        bt.merit(0.5)
    ts = []
    for _ in range(reps):
        bt.synchronize(); t0 = time.perf_counter()
        bt.merit(0.5)
        ts.append((time.perf_counter() - t0) * 1e3)
    bt.close()
    return sorted(ts)[len(ts) // 2]


t_user = merit_ms(QUADROTOR13_SRC, True)
t_lin = merit_ms(QUADROTOR13_SRC, False)
t_lin0 = merit_ms(SRC_NO_CONSTRAINTS, False)
print("(n, m) = (%d, %d), N = %d, %d problems, merit with derivative, wave-per-problem kernel, median of %d:" % (n, m, N, batch, reps))
print("  1-row sphere block from source                      %.3f ms" % t_user)
print("  1-row linear block, source with constraint functions %.3f ms" % t_lin)
print("  1-row linear block, source without them              %.3f ms" % t_lin0)
print("  ratio sphere / linear (same module): %.3f   sphere / linear (module without constraint code): %.3f" % (t_user / t_lin, t_user / t_lin0))
