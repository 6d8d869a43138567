"""A solve leaves no per-launch switch behind.  What one launch of the iLQR loop is told -- how many trials it evaluates, whether it is the
sweep's phi(0) evaluation or an affine round, which mask it runs under, the stationarity skip mask, the penalty look-ahead, the backward
sweep's mask and per-problem regularisation -- describes that launch, not the handle: after altro_hip_ilqr_solve the step-wise entry
points must behave as on a handle that never solved.

Each case takes one handle through a full solve, puts its inputs back through the public setters (initial state, input and state guess,
duals to zero, the penalty to its initial value) and runs open_loop_rollout, accept, expand, backward, merit (a uniform and a per-problem
step, with derivative), stationarity and feasibility; every array these return is compared with array_equal against the same sequence on
a fresh handle.  Nothing is excluded: no per-problem quantity without a setter shows in these outputs.

The shapes are the smallest at which each path still engages: the (12, 4) tile with batch 3 (a half-filled wave in the two-problems-per-
wave forms) and N = 17 (two chunks of knot points, the last a single one), backtracking search with the decision guard (the two-trial
pass, speculative rounds with spares, affine rounds, the masks of the redone first step and of the guarded trials); the same with the
LDS comparison forms in the solve's options; plan LANE's bicycle in one launch and launch-sequenced; plans GENERIC (5, 2) and MFMA32
(13, 4) with a bound block and the regularisation retry, where the step-wise backward sweep must get the caller's reg, not the solve's
per-problem one."""
import numpy as np
import pytest

import altro_amd
from tests import problems

pytestmark = pytest.mark.gpu

INEQ = altro_amd.CONE_INEQUALITY
PENALTY_INITIAL = 1.0


def input_box(n, m, bound):
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    return G, np.full(2 * m, bound)


class Case:
    """make() -> a handle with dynamics, cost and blocks; put_inputs(bt): what a caller can set again after a solve."""
    reg = 0.0                   # the step-wise backward sweep's
    affine = False              # the sequence ends with merit_affine(trials = 2) under a mask
    blocks = ()                 # (k_first, k_last, rows)

    def put_inputs(self, bt):
        bt.set_initial_state(self.x0)
        bt.set_input_guess(self.u0)
        bt.set_state_guess(np.zeros((bt.batch, bt.N + 1, bt.n)))
        for k in range(bt.N + 1):
            for slot, (k0, k1, p) in enumerate(b for b in self.blocks if b[0] <= k <= b[1]):
                bt.set_duals(k, slot, np.zeros((bt.batch, p)))
        bt.set_penalty(PENALTY_INITIAL)


class Tile(Case):
    """Plan MFMA16, (12, 4), fp64, batch 3, N = 17, |u| <= 0.3."""
    affine = True
    solve = dict(iterations_max=40, use_backtracking=True, decision_margin=1e-9, penalty_initial=PENALTY_INITIAL, penalty_scaling=10.0)

    def __init__(self, forms=0):
        self.N, self.batch = 17, 3
        self.p = problems.ilqr12x4_problem(self.batch, self.N, True)
        self.x0, self.u0 = self.p["x0"], self.p["u0"]
        self.blocks = ((0, self.N - 1, 8),)
        self.solve = dict(self.solve, forms=forms)
        self.affine = forms == 0

    def make(self):
        p = self.p
        bt = altro_amd.Batch(self.N, 12, 4, self.batch)
        assert bt.plan == altro_amd.PLAN_MFMA16
        bt.set_dynamics(p["A"], p["B"], p["f"])
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.add_linear_constraint(0, self.N - 1, INEQ, *input_box(12, 4, 0.3))
        return bt

    def engaged(self, res):
        assert res["merit_launches"] > res["sweeps"] > 1      # line-search rounds past the first step, several sweeps


class Bicycle(Case):
    """Plan LANE, the bicycle with its steering bound, batch 5, N = 10."""

    def __init__(self, forms=0):
        self.N, self.batch = 10, 5
        self.x_ref, self.u_ref = problems.bicycle_reference(self.N + 1)
        self.x0 = self.x_ref[0] + (problems.uniform01((self.batch, 4), 23, 0) - 0.5) * 0.4
        self.u0 = np.tile(np.array([self.u_ref[0][0], 0.0]), (self.batch, self.N, 1))
        self.blocks = ((0, self.N, 2),)
        self.solve = dict(iterations_max=40, use_backtracking=True, penalty_initial=PENALTY_INITIAL, penalty_scaling=10.0, forms=forms)

    def make(self):
        N = self.N
        bt = altro_amd.Batch(N, 4, 2, self.batch)
        bt.set_model(altro_amd.MODEL_BICYCLE, np.float32(0.1))
        assert bt.plan == altro_amd.PLAN_LANE
        bt.set_tracking_cost(np.full((1, N + 1, 4), 1e-2), np.full((1, N, 2), 1e-3), self.x_ref[None, :N + 1], self.u_ref[None, :N],
                             batch_stride_zero=True)
        G = np.zeros((2, 6)); G[0, 3] = 1.0; G[1, 3] = -1.0
        bt.add_linear_constraint(0, N, INEQ, G, np.full(2, np.pi / 3))
        return bt

    def engaged(self, res):
        assert res["sweeps"] > 1


class Retry(Case):
    """Plans GENERIC (5, 2) and MFMA32 (13, 4), batch 3, N = 6, dynamics as data, a dense cost whose R is indefinite at one knot point of
    problem 1, an input box; the solve retries that problem's backward sweep with more regularisation.  The step-wise sweep runs with a
    reg at which every problem factors: with the solve's per-problem array still in place it would run with that instead."""
    reg = 4.0
    solve = dict(iterations_max=6, penalty_initial=PENALTY_INITIAL, penalty_scaling=10.0, reg_retry_max=6, reg_min=1.0, reg_scale=4.0,
                 reg_max=1024.0)

    def __init__(self, n, m, plan):
        self.N, self.batch, self.n, self.m, self.plan = 6, 3, n, m, plan
        self.pr = problems.random_ltv(self.batch, self.N, n, m)
        self.pr["R"][1, 2].reshape(m, m)[:] -= 2.5 * np.eye(m)
        self.x0, self.u0 = self.pr["x0"], 0.2 * problems.normal((self.batch, self.N, m), 76)
        self.blocks = ((0, self.N - 1, 2 * m),)

    def make(self):
        pr = self.pr
        bt = altro_amd.Batch(self.N, self.n, self.m, self.batch, plan=altro_amd.PLAN_GENERIC if self.plan == altro_amd.PLAN_GENERIC else altro_amd.PLAN_AUTO)
        assert bt.plan == self.plan
        bt.set_dynamics(pr["A"], pr["B"], pr["f"])
        bt.set_quadratic_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
        bt.add_linear_constraint(0, self.N - 1, INEQ, *input_box(self.n, self.m, 0.5))
        return bt

    def engaged(self, res):
        assert res["reg_retries"][1] > 0 and res["reg_retries"][0] == 0, res["reg_retries"]


LDS_FORMS = altro_amd.FORM_MERIT_LDS | altro_amd.FORM_EXPAND_LDS | altro_amd.FORM_ALROWS_LDS
CASES = {
    "tile": lambda: Tile(),
    "tile_lds_forms": lambda: Tile(LDS_FORMS),
    "lane_fused": lambda: Bicycle(),
    "lane_sequenced": lambda: Bicycle(altro_amd.FORM_SEQUENCED),
    "generic_retry": lambda: Retry(5, 2, altro_amd.PLAN_GENERIC),
    "mfma32_retry": lambda: Retry(13, 4, altro_amd.PLAN_MFMA32),
}


def stepwise(case, bt):
    """The step-wise sequence on the case's inputs -> every array it returns, by name."""
    out = {}

    def keep(step, names, arrays):
        for name, a in zip(names, arrays):
            if a is not None:
                out[step + "." + name] = np.array(a, copy=True)

    candidate = lambda: (bt.get("x"), bt.get("u"))
    case.put_inputs(bt)
    bt.open_loop_rollout()
    keep("rollout", ("x", "u"), candidate())
    bt.accept()
    keep("accept", ("x", "u"), bt.get_nominal())
    bt.expand()
    keep("expand", ("A", "B", "lx", "lu"), bt.get_expansion())
    bt.backward(case.reg)
    keep("backward", ("K", "d", "P", "p", "status", "delta_V"), [bt.get(v) for v in ("K", "d", "P", "p", "status", "delta_V")])
    alphas = np.linspace(0.2, 1.0, bt.batch)
    for step, alpha in (("merit_uniform", 0.7), ("merit_each", alphas)):
        keep(step, ("phi", "dphi"), bt.merit(alpha, derivative=True))
        keep(step, ("x", "u"), candidate())
    keep("stationarity", ("value",), [bt.stationarity()])
    keep("feasibility", ("value",), [bt.feasibility()])
    if case.affine:
        active = np.ones(bt.batch, dtype=np.int32); active[1] = 0          # one problem switched off: its entries keep what `out` held
        held = (np.full((2, bt.batch), -7.0), np.full(bt.batch, -7.0))
        keep("merit_affine", ("phi", "dphi"), bt.merit_affine(alphas, active=active, trials=2, out=held))
        keep("merit_affine", ("x", "u"), candidate())
        assert (out["merit_affine.phi"][:, 1] == -7.0).all() and (out["merit_affine.phi"][:, 0] != -7.0).all()
    assert all(np.isfinite(a).all() for a in out.values()), [k for k, a in out.items() if not np.isfinite(a).all()]
    return out


_fresh = {}


def fresh_sequence(name, case):
    """The sequence on a handle that never solved: computed once per case."""
    if name not in _fresh:
        bt = case.make()
        _fresh[name] = stepwise(case, bt)
        bt.close()
    return _fresh[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_stepwise_calls_after_a_solve_equal_a_fresh_handle(name):
    case = CASES[name]()
    want = fresh_sequence(name, case)
    bt = case.make()
    case.put_inputs(bt)
    forms = bt.L.altro_hip_get_forms(bt.h)
    res = bt.ilqr_solve(**case.solve)
    case.engaged(res)
    assert bt.L.altro_hip_get_forms(bt.h) == forms             # (the solve's own forms were its options', for its duration)
    got = stepwise(case, bt)
    bt.close()
    assert sorted(got) == sorted(want)
    differ = [key for key in sorted(want) if not np.array_equal(got[key], want[key])]
    for key in differ:
        print("%s %-22s max |difference| %.3e" % (name, key, np.abs(got[key].astype(np.float64) - want[key]).max()))
    assert not differ, differ
