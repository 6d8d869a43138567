"""altro_hip_batch_device_bytes is the sum of the counted device buffers the handle holds NOW (altro_amd/csrc/device_ledger.h): a buffer
that is freed -- the constraint tables at a re-upload or after clear_constraints, the split merit evaluation's buffers when set_forms
decides the split again -- leaves the count, so two handles in the same state report the same bytes however they got there.  And
altro_hip_batch_destroy drains that ledger: handles of every plan are created, exercised and closed, twice, and the same calls run again
on fresh ones.

The smallest shapes each plan accepts, batch 64, N = 8: plan LANE at (2, 1) with the compiled-in pendulum, plan MFMA16 at (12, 4) with
dynamics as data, plan GENERIC at (14, 5), plan MFMA32 at (13, 4).  Nothing here looks at the device's free memory: it is shared."""
import numpy as np
import pytest

import altro_amd
from tests import problems

pytestmark = pytest.mark.gpu

BATCH, N = 64, 8
INEQ = altro_amd.CONE_INEQUALITY
PLANS = ["lane", "tile", "generic", "mfma32"]
SHAPE = {"lane": (2, 1), "tile": (12, 4), "generic": (14, 5), "mfma32": (13, 4)}


def make(plan):
    """A handle of the plan with everything the step-wise calls need (dynamics or model, cost, initial state, input guess), no blocks."""
    n, m = SHAPE[plan]
    if plan == "lane":
        bt = altro_amd.Batch(N, n, m, BATCH, plan=altro_amd.PLAN_LANE)
        bt.set_model(altro_amd.MODEL_PENDULUM, np.float32(0.05))
        xf = np.array([np.pi, 0.0])
        bt.set_tracking_cost(np.array([[1e-2, 1e-2], [1.0, 1.0]]), np.array([[1e-3]]), np.stack([xf, xf]), np.zeros((1, m)),
                             k_stride_zero=True, batch_stride_zero=True)
        x0 = np.zeros((BATCH, n)); x0[:, 0] = problems.uniform01((BATCH,), 41) - 0.5
        bt.set_initial_state(x0)
        bt.set_input_guess(np.array([[[0.1]]]), k_stride_zero=True, batch_stride_zero=True)
        assert bt.plan == altro_amd.PLAN_LANE
    elif plan == "tile":
        p = problems.ilqr12x4_problem(BATCH, N, True)
        bt = altro_amd.Batch(N, n, m, BATCH, plan=altro_amd.PLAN_MFMA16)
        bt.set_dynamics(p["A"], p["B"], p["f"])
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.set_initial_state(p["x0"])
        bt.set_input_guess(p["u0"])
        assert bt.plan == altro_amd.PLAN_MFMA16
    else:
        want = altro_amd.PLAN_GENERIC if plan == "generic" else altro_amd.PLAN_MFMA32
        pr = problems.random_ltv(BATCH, N, n, m)
        bt = altro_amd.Batch(N, n, m, BATCH, plan=want)
        bt.set_dynamics(pr["A"], pr["B"], pr["f"])
        bt.set_quadratic_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
        bt.set_initial_state(pr["x0"])
        bt.set_input_guess(0.2 * problems.normal((BATCH, N, m), 76))
        assert bt.plan == want
    return bt


def blocks(plan):
    """Two linear blocks: |u| <= 0.5 at knot points 0 .. N - 1, |x_0| <= 5 at 1 .. N."""
    n, m = SHAPE[plan]
    Gu = np.zeros((2 * m, n + m)); Gu[:m, n:] = np.eye(m); Gu[m:, n:] = -np.eye(m)
    Gx = np.zeros((2, n + m)); Gx[0, 0] = 1.0; Gx[1, 0] = -1.0
    return [(0, N - 1, INEQ, Gu, np.full(2 * m, 0.5)), (1, N, INEQ, Gx, np.full(2, 5.0))]


def exercise(bt):
    """A few step-wise calls that touch the loop's buffers -> what they return."""
    bt.open_loop_rollout()
    bt.accept()
    bt.expand()
    bt.backward()
    phi, dphi = bt.merit(0.5)
    return phi, dphi, bt.feasibility()


@pytest.mark.parametrize("plan", PLANS)
def test_same_state_same_bytes(plan):
    """Blocks declared one at a time, with the tables uploaded in between, against both declared before the one upload: the first
    set of tables, freed at the second upload, must not stay in the count."""
    b1, b2 = blocks(plan)
    a = make(plan)
    a.add_linear_constraint(*b1)
    fa1 = a.feasibility()
    a.add_linear_constraint(*b2)
    fa = a.feasibility()
    b = make(plan)
    b.add_linear_constraint(*b1)
    b.add_linear_constraint(*b2)
    fb = b.feasibility()
    print(plan, "bytes one at a time", a.device_bytes(), "both at once", b.device_bytes())
    assert a.device_bytes() == b.device_bytes()
    assert np.array_equal(fa, fb) and np.isfinite(fa1).all()
    a.close(); b.close()


@pytest.mark.parametrize("plan", ["lane", "generic"])
def test_clear_constraints_gives_the_tables_bytes_back(plan):
    bt = make(plan)
    before = bt.device_bytes()
    for blk in blocks(plan):
        bt.add_linear_constraint(*blk)
    bt.feasibility()
    with_tables = bt.device_bytes()
    bt.clear_constraints()
    bt.feasibility()
    print(plan, "bytes before", before, "with tables", with_tables, "after clear", bt.device_bytes())
    assert with_tables > before
    assert bt.device_bytes() == before
    bt.close()


def test_merit_split_buffers_leave_and_return_with_set_forms():
    """Plan LANE: the first merit evaluation allocates the three-launch form's buffers; set_forms that toggles FORM_MERIT_ONE_LAUNCH frees
    them (the split is decided again at the next evaluation); toggled back, the next evaluation holds what the first one held and returns
    the same bits."""
    bt = make("lane")
    bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.backward()
    first = bt.device_bytes()
    phi1, dphi1 = bt.merit(0.5)
    split = bt.device_bytes()
    assert split > first
    bt.set_forms(altro_amd.FORM_MERIT_ONE_LAUNCH)
    assert bt.device_bytes() == first
    bt.merit(0.5)                                  # the one-launch kernel takes nothing
    assert bt.device_bytes() == first
    bt.set_forms(0)
    phi2, dphi2 = bt.merit(0.5)
    print("bytes before merit", first, "split", split, "after the round trip", bt.device_bytes())
    assert bt.device_bytes() == split
    assert np.array_equal(phi1, phi2) and np.array_equal(dphi1, dphi2) and np.isfinite(phi1).all()
    bt.close()


def test_replanned_handle_counts_like_one_created_on_the_plan():
    """An empty PLAN_AUTO handle that altro_hip_set_model moves from the padded tile to plan LANE (two handles exchange their contents,
    the old one is destroyed) holds what a handle created with PLAN_LANE holds after the same calls, and solves to the same bits."""
    n, m = 6, 3
    x0 = 0.3 * problems.normal((BATCH, n), 91)
    got = {}
    for name, plan in (("auto", altro_amd.PLAN_AUTO), ("lane", altro_amd.PLAN_LANE)):
        bt = altro_amd.Batch(N, n, m, BATCH, plan=plan)
        assert bt.plan == (altro_amd.PLAN_MFMA16 if name == "auto" else altro_amd.PLAN_LANE)
        bt.set_initial_state(x0)                   # (kept on the host of an AUTO handle and set again on the plan it moves to)
        bt.set_model(altro_amd.MODEL_DOUBLE_INTEGRATOR, np.float32(0.1))
        assert bt.plan == altro_amd.PLAN_LANE
        bt.set_tracking_cost(np.full((1, N + 1, n), 1.0), np.full((1, N, m), 1e-2), np.zeros((1, N + 1, n)), np.zeros((1, N, m)),
                             batch_stride_zero=True)
        bt.set_input_guess(np.zeros((1, 1, m)), k_stride_zero=True, batch_stride_zero=True)
        res = bt.ilqr_solve(iterations_max=5)
        got[name] = (bt.device_bytes(), res, bt.get_nominal())
        bt.close()
    print("bytes replanned", got["auto"][0], "created on LANE", got["lane"][0])
    assert got["auto"][0] == got["lane"][0]
    for k in ("status", "iterations", "phi", "stationarity"):
        assert np.array_equal(got["auto"][1][k], got["lane"][1][k]), k
    assert np.array_equal(got["auto"][2][0], got["lane"][2][0]) and np.array_equal(got["auto"][2][1], got["lane"][2][1])
    assert np.isfinite(got["lane"][2][0]).all()


@pytest.mark.parametrize("plan", PLANS)
def test_create_exercise_close_twice_then_again(plan):
    """destroy drains the ledger: no double free, nothing used after it.  The third handle returns what the first did."""
    outs = []
    for _ in range(3):
        bt = make(plan)
        for blk in blocks(plan):
            bt.add_linear_constraint(*blk)
        outs.append(exercise(bt) + (bt.device_bytes(),))
        bt.close()
        bt.close()                                 # a second close is nothing
    for o in outs[1:]:
        assert o[3] == outs[0][3]
        for a, b in zip(o[:3], outs[0][:3]):
            assert np.array_equal(a, b) and np.isfinite(a).all()
