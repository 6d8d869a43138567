"""The regularisation schedule of altro_hip_solve_options (reg_initial, reg_retry_max: an extension beyond the reference, which calls
the backward pass with reg = 0 and ignores a failed Cholesky, tvlqr.cpp:159-164, solver.cpp:363) on the plans past the (12, 4) tile:
plan GENERIC (uniform and per-knot-point dimensions, fp64 and fp32) and plan MFMA32 (dense cost: the tile32 sweep; diagonal cost:
plan GENERIC's sweep), dynamics as data and device models, with and without constraint blocks.

The problems: `problems.random_ltv` with s I subtracted from R at one knot point of the odd problems, s = 2.5 .. 120, and the schedule
reg = 1, 4, 16, 64, 256.  With dynamics as data, a quadratic cost and no constraints K and P depend on (A, B, Q, R, H, reg) alone, so
the oracle's backward pass says at which step of the schedule a problem first factors (`Schedule.solved`, asked again at
reg (1 +- 1e-6): a decision that close to a boundary would not be one rounding may not turn) and gives K, P at that reg.  The counts
are carried through `ilqr_reg_retry_logic`'s rule (kernels/ilqr_loop_logic.h) sweep by sweep (`Schedule.run`)."""
import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import problems
from tests.test_gpu_parity import relerr

pytestmark = pytest.mark.gpu

N, BATCH = 12, 10
SHIFTS = {1: 2.5, 3: 9.0, 5: 30.0, 7: 50.0, 9: 120.0}
ODD = np.arange(BATCH) % 2 == 1
RETRY = dict(reg_retry_max=6, reg_min=1.0, reg_scale=4.0, reg_max=1024.0)
BOX = 0.5          # |u| <= BOX: binds in every problem of the recipe's (13, 4) batch (the oracle's solves end with max |u| = BOX)


def recipe(n, m, diag=False):
    pr = problems.random_ltv(BATCH, N, n, m)
    pr["u0"] = 0.2 * problems.normal((BATCH, N, m), 76)
    if diag:
        pr["Qd"] = 1.0 + problems.uniform01((BATCH, N + 1, n), 71); pr["Rd"] = 0.1 + 0.2 * problems.uniform01((BATCH, N, m), 72)
        pr["xref"] = 0.3 * problems.normal((BATCH, N + 1, n), 73); pr["uref"] = 0.1 * problems.normal((BATCH, N, m), 74)
    rng = np.random.default_rng(5)
    for b in sorted(SHIFTS):
        k = int(rng.integers(1, N - 1))
        if diag:
            pr["Rd"][b, k] -= SHIFTS[b]
        else:
            pr["R"][b, k].reshape(m, m)[:] -= SHIFTS[b] * np.eye(m)
    return pr


class Schedule:
    """What the solve loop's retry does to one batch whose K, P depend on reg alone: the oracle's backward pass decides every step."""

    def __init__(self, arrays, is_diag=False, opts=RETRY, reg_initial=0.0):
        self.arrays, self.is_diag, self.o, self.reg_initial, self.cache = arrays, is_diag, opts, reg_initial, {}

    def backward(self, reg):
        if reg not in self.cache:
            self.cache[reg] = oracle.backward_batch(*self.arrays, reg, self.is_diag)
        return self.cache[reg]

    def solved(self, b, reg):
        ok = [self.backward(r)["status"][b] == -1 for r in (reg, reg * (1.0 + 1e-6), reg * (1.0 - 1e-6))]
        assert ok[0] == ok[1] == ok[2], ("a decision on a boundary", b, reg)
        return bool(ok[0])

    def run(self, b, sweeps):
        """-> (retries, reg of the last backward pass, whether that pass factored) after `sweeps` sweeps of problem b"""
        reg, retries, used, ok = self.reg_initial, 0, self.reg_initial, True
        for _ in range(sweeps):
            used, ok = reg, self.solved(b, reg)
            for _attempt in range(self.o["reg_retry_max"]):       # one ILK_REG_RETRY launch each, then the repeated backward pass
                if ok:
                    reg = max(reg / self.o["reg_scale"], self.reg_initial)
                    break
                r = max(reg * self.o["reg_scale"], self.o["reg_min"])
                if r > self.o["reg_max"]:
                    break
                reg = r; retries += 1
                used, ok = reg, self.solved(b, reg)
        return retries, used, ok


def dense_arrays(pr):
    return (pr["A"], pr["B"], pr["f"], pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])


def diag_arrays(pr):
    return (pr["A"], pr["B"], pr["f"], pr["Qd"], pr["Rd"], None, pr["q"], pr["r"])


def make_hip(pr, diag=False, **kw):
    bt = altro_amd.Batch(N, pr["n"], pr["m"], pr["A"].shape[0], **kw)
    bt.set_dynamics(pr["A"], pr["B"], pr["f"])
    if diag:
        bt.set_tracking_cost(pr["Qd"], pr["Rd"], pr["xref"], pr["uref"])
    else:
        bt.set_quadratic_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    bt.set_initial_state(pr["x0"]); bt.set_input_guess(pr["u0"])
    return bt


def swept(res):
    """sweeps each problem took part in: a problem that stops in sweep i reports i + 1 iterations, one at the limit one more"""
    return np.minimum(res["iterations"], res["sweeps"])


def expected(sched, res):
    """-> (retry counts, K, P) of the batch after the solve `res` reports, from the oracle"""
    B = len(res["iterations"])
    runs = [sched.run(b, int(s)) for b, s in enumerate(swept(res))]
    assert all(ok for (_, _, ok) in runs)                     # every last backward pass factored
    K = np.stack([sched.backward(runs[b][1])["K"][b] for b in range(B)])
    P = np.stack([sched.backward(runs[b][1])["P"][b] for b in range(B)])
    return np.array([r[0] for r in runs]), K, P


def check_recipe(sched):
    """the recipe as the tests rely on it: reg = 0 fails for exactly the odd problems, the schedule rescues each within reg_max"""
    first = np.array([sched.run(b, 1)[0] for b in range(BATCH)])
    assert (first[~ODD] == 0).all() and (first[ODD] >= 1).all() and (first <= 5).all(), first
    assert all(sched.run(b, 1)[2] for b in range(BATCH))
    return first


@pytest.mark.parametrize("n,m", [(14, 5), (12, 4)])
def test_retry_counts_and_gains_plan_generic(n, m):
    """Plan GENERIC by name (an AUTO handle of either shape runs a matrix-core plan), dense cost.  Without the feature the solve with
    reg_retry_max = 6 answers ALTRO_HIP_ERR_UNSUPPORTED."""
    kw = {"plan": altro_amd.PLAN_GENERIC}
    pr = recipe(n, m)
    sched = Schedule(dense_arrays(pr))
    check_recipe(sched)
    bt0 = make_hip(pr, **kw)
    assert bt0.plan == altro_amd.PLAN_GENERIC
    res0 = bt0.ilqr_solve(iterations_max=1)                  # the reference's behaviour: the failure is ignored
    st0 = bt0.get("status")
    assert (res0["reg_retries"] == 0).all() and (st0[ODD] != -1).all() and (st0[~ODD] == -1).all()
    assert bt0.stats().cholesky_failures == 5
    x0, u0 = bt0.get_nominal()
    bt = make_hip(pr, **kw)
    res = bt.ilqr_solve(iterations_max=1, **RETRY)
    assert (bt.get("status") == -1).all()
    retries, K, P = expected(sched, res)
    assert np.array_equal(res["reg_retries"], retries), (res["reg_retries"], retries)
    assert np.array_equal(bt.get("K"), K) and np.array_equal(bt.get("P"), P)      # the bit-for-bit plan
    x, u = bt.get_nominal()
    assert np.array_equal(x[~ODD], x0[~ODD]) and np.array_equal(u[~ODD], u0[~ODD])
    assert bt.stats().cholesky_failures == 0
    bt0.close(); bt.close()


@pytest.mark.parametrize("n,m", [(13, 4), (20, 6)])
@pytest.mark.parametrize("diag", [False, True])
def test_retry_plan_mfma32(n, m, diag):
    """Plan MFMA32: the tile32 sweep under a dense cost, plan GENERIC's own sweep under a diagonal one (R negative through Rd, the
    oracle's is_diag form).  Without the feature both answer ALTRO_HIP_ERR_UNSUPPORTED."""
    pr = recipe(n, m, diag)
    sched = Schedule(diag_arrays(pr) if diag else dense_arrays(pr), is_diag=diag)
    check_recipe(sched)
    bt0 = make_hip(pr, diag)
    assert bt0.plan == altro_amd.PLAN_MFMA32
    res0 = bt0.ilqr_solve(iterations_max=1)
    st0 = bt0.get("status")
    assert (res0["reg_retries"] == 0).all() and (st0[ODD] != -1).all() and (st0[~ODD] == -1).all()
    bt = make_hip(pr, diag)
    assert bt.plan == altro_amd.PLAN_MFMA32
    res = bt.ilqr_solve(iterations_max=1, **RETRY)
    assert (bt.get("status") == -1).all()
    retries, K, P = expected(sched, res)
    assert np.array_equal(res["reg_retries"], retries), (res["reg_retries"], retries)
    Kh, Ph = bt.get("K"), bt.get("P")
    assert np.abs(Kh - K).max() < 1e-8                        # tests/test_gpu_tile32.py::check's tolerances
    assert relerr(Kh, K) < 1e-9 and relerr(Ph, P) < 1e-9, (relerr(Kh, K), relerr(Ph, P))
    assert bt.stats().cholesky_failures == 0 and bt0.stats().cholesky_failures == 5
    bt0.close(); bt.close()


def test_reg_initial_is_honoured_plan_generic():
    """reg_initial = 0.37 without retries on a well-posed batch: the gains are the oracle's at that reg, not at 0.  Without the feature
    plan GENERIC's sweep drops the option and returns the reg = 0 gains."""
    pr = problems.random_ltv(BATCH, N, 14, 5)
    pr["u0"] = 0.2 * problems.normal((BATCH, N, 5), 76)
    bt = make_hip(pr, plan=altro_amd.PLAN_GENERIC)
    assert bt.plan == altro_amd.PLAN_GENERIC
    res = bt.ilqr_solve(iterations_max=1, reg_initial=0.37, reg_retry_max=0)
    assert res["sweeps"] == 1 and (res["reg_retries"] == 0).all()
    K = bt.get("K")
    assert np.array_equal(K, oracle.backward_batch(*dense_arrays(pr), 0.37, False)["K"])
    assert not np.array_equal(K, oracle.backward_batch(*dense_arrays(pr), 0.0, False)["K"])
    bt.close()


def test_retry_with_per_knot_point_dimensions():
    """A handle of altro_hip_batch_create_dims; R indefinite at one knot point of three problems.  The oracle's backward pass takes one
    (n, m): the zero-padded problem of tests/test_gpu_ragged_ilqr.py (identity in R for the padded inputs, which nothing couples to
    the real ones: the real pivots are the same sums).  Without the feature: ALTRO_HIP_ERR_UNSUPPORTED."""
    from tests import test_gpu_ragged_ilqr as rg
    batch, bad = 8, RAGGED_BAD
    p, sched = ragged_case(rg, batch)
    first = np.array([sched.run(b, 1)[0] for b in range(batch)])
    isbad = np.array([b in bad for b in range(batch)])
    assert (first[isbad] >= 1).all() and (first[~isbad] == 0).all(), first
    bt0 = rg.make_hip(p, batch, [])
    res0 = bt0.ilqr_solve(iterations_max=2)
    bt = rg.make_hip(p, batch, [])
    res = bt.ilqr_solve(iterations_max=2, **RETRY)
    assert (bt.get("status") == -1).all()                     # every backward pass was rescued
    runs = [sched.run(b, int(s)) for b, s in enumerate(swept(res))]
    assert all(r[2] for r in runs)
    assert np.array_equal(res["reg_retries"], [r[0] for r in runs]), (res["reg_retries"], runs)
    (x0, u0), (x, u) = bt0.get_nominal(), bt.get_nominal()
    assert np.array_equal(x[~isbad], x0[~isbad]) and np.array_equal(u[~isbad], u0[~isbad])
    assert np.array_equal(res["iterations"][~isbad], res0["iterations"][~isbad])
    assert np.array_equal(bt.get("K")[~isbad], bt0.get("K")[~isbad])
    assert np.isfinite(bt.get("K")).all() and np.isfinite(x).all()
    bt0.close(); bt.close()


RAGGED_BAD = {1: (4, 3.0), 4: (7, 20.0), 6: (2, 70.0)}      # problem: (knot point, s)


def ragged_case(rg, batch):
    """-> (the per-knot-point problem with s I subtracted from R_k of the problems RAGGED_BAD names, the Schedule of its padded form)"""
    p = rg.make_problem(batch, seed=977)
    for b, (k, s) in RAGGED_BAD.items():
        p["R"][k][b] -= s * np.eye(rg.NU[k])
    nm, mm, NN = rg.NMAX, rg.MMAX, rg.N
    col = lambda M_: np.ascontiguousarray(np.swapaxes(M_, -1, -2)).reshape(M_.shape[0], -1)
    A = np.zeros((batch, NN, nm * nm)); Bm = np.zeros((batch, NN, nm * mm)); f = np.zeros((batch, NN, nm))
    Q = np.zeros((batch, NN + 1, nm * nm)); R = np.zeros((batch, NN, mm * mm)); H = np.zeros((batch, NN, mm * nm))
    for k in range(NN + 1):
        n = rg.NX[k]
        Qk = np.zeros((batch, nm, nm)); Qk[:, :n, :n] = p["Q"][k]; Q[:, k] = col(Qk)
        if k == NN:
            break
        m, n2 = rg.NU[k], rg.NX[k + 1]
        Ak = np.zeros((batch, nm, nm)); Ak[:, :n2, :n] = p["A"][k]; A[:, k] = col(Ak)
        Bk = np.zeros((batch, nm, mm)); Bk[:, :n2, :m] = p["B"][k]; Bm[:, k] = col(Bk)
        Rk = np.tile(np.eye(mm), (batch, 1, 1)); Rk[:, :m, :m] = p["R"][k]; R[:, k] = col(Rk)
        Hk = np.zeros((batch, mm, nm)); Hk[:, :m, :n] = p["H"][k]; H[:, k] = col(Hk)
    return p, Schedule((A, Bm, f, Q, R, H, np.zeros((batch, NN + 1, nm)), np.zeros((batch, NN, mm))))


def test_retry_across_plans_12x4():
    """The same (12, 4) batch and options on plan MFMA16 (the retry it always had) and on plan GENERIC by name.  Two sweeps, so
    the relaxed reg of the first is the start of the second.  Without the feature the second handle answers ALTRO_HIP_ERR_UNSUPPORTED."""
    pr = recipe(12, 4)
    out = []
    for plan in (altro_amd.PLAN_MFMA16, altro_amd.PLAN_GENERIC):
        bt = make_hip(pr, plan=plan)
        assert bt.plan == plan
        res = bt.ilqr_solve(iterations_max=2, **RETRY)
        out.append((res, bt.get_nominal()[0]))
        bt.close()
    (ra, xa), (rb, xb) = out
    assert np.array_equal(ra["reg_retries"], rb["reg_retries"]), (ra["reg_retries"], rb["reg_retries"])
    assert np.array_equal(ra["status"], rb["status"]) and np.array_equal(ra["iterations"], rb["iterations"])
    assert np.abs(xa - xb).max() < 1e-9, np.abs(xa - xb).max()


def test_retry_with_a_device_model_past_the_tile():
    """ALTRO_HIP_MODEL_QUADROTOR13 on the AUTO handle (plan MFMA32), hover reference, a dense cost whose R is indefinite at one knot
    point of three problems.  Without the feature: ALTRO_HIP_ERR_UNSUPPORTED."""
    from tests import test_gpu_generic_model as gm
    batch, Nq, n, m = 8, 10, gm.n, gm.m
    c = gm.make_case(batch)
    bad = np.zeros(batch, dtype=bool); bad[[1, 4, 6]] = True
    Q = np.tile(np.diag(c["Qd"]).reshape(-1), (batch, Nq + 1, 1)); Q[:, Nq] = np.diag(c["Qfd"]).reshape(-1)
    R = np.tile(np.diag(c["Rd"]).reshape(-1), (batch, Nq, 1))
    R[bad, 4] -= 30.0 * np.eye(m).reshape(-1)
    Hc = np.zeros((batch, Nq, m * n))
    q = np.tile(-c["Qd"] * c["xref"], (batch, Nq + 1, 1)); q[:, Nq] = -c["Qfd"] * c["xref"]
    r = -np.einsum("bkij,j->bki", R.reshape(batch, Nq, m, m), c["uref"])

    def make():
        bt = altro_amd.Batch(Nq, n, m, batch)
        assert bt.plan == altro_amd.PLAN_MFMA32
        bt.set_model(altro_amd.MODEL_QUADROTOR13, gm.H)
        bt.set_quadratic_cost(Q, R, Hc, q, r)
        bt.set_initial_state(c["x0"])
        bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
        return bt
    bt0, bt = make(), make()
    rows = bt.model_row_layout()
    assert rows == bt0.model_row_layout()
    res0 = bt0.ilqr_solve(iterations_max=3)
    res = bt.ilqr_solve(iterations_max=3, **RETRY)
    assert bt.model_row_layout() == rows and bt0.model_row_layout() == rows
    assert (bt.get("status") == -1).all()
    assert (res["reg_retries"][bad] > 0).all() and (res["reg_retries"][~bad] == 0).all(), res["reg_retries"]
    (x0, u0), (x, u) = bt0.get_nominal(), bt.get_nominal()
    assert np.isfinite(bt.get("K")).all() and np.isfinite(x).all() and np.isfinite(u).all()
    assert np.array_equal(x[~bad], x0[~bad]) and np.array_equal(u[~bad], u0[~bad])
    assert np.array_equal(bt.get("K")[~bad], bt0.get("K")[~bad])
    assert np.array_equal(res["iterations"][~bad], res0["iterations"][~bad])
    bt0.close(); bt.close()


def test_retry_in_a_constrained_solve_13x4():
    """An input box on the recipe's (13, 4) batch, dynamics as data: the retry between the Hessian expansion and the line search of an
    AL-iLQR solve.  The well-posed problems converge with the iteration counts of the solve without the option (and its iterates);
    the others' backward passes are rescued.  Without the feature: ALTRO_HIP_ERR_UNSUPPORTED."""
    n, m = 13, 4
    pr = recipe(n, m)
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    opts = dict(iterations_max=40, penalty_initial=1.0, penalty_scaling=10.0)
    out = []
    for extra in ({}, RETRY):
        bt = make_hip(pr)
        assert bt.plan == altro_amd.PLAN_MFMA32
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G, np.full(2 * m, BOX))
        res = bt.ilqr_solve(**opts, **extra)
        out.append((res, bt.get_nominal(), bt.get("status")))
        bt.close()
    (r0, (x0, u0), _), (r1, (x1, u1), st1) = out
    assert (r1["status"][~ODD] == 0).all(), r1["status"]
    assert np.array_equal(r1["iterations"][~ODD], r0["iterations"][~ODD]) and np.array_equal(r1["status"][~ODD], r0["status"][~ODD])
    assert np.array_equal(x1[~ODD], x0[~ODD]) and np.array_equal(u1[~ODD], u0[~ODD])
    assert np.abs(u1[~ODD]).max() <= BOX + 1e-3
    assert (r1["reg_retries"][~ODD] == 0).all() and (r1["reg_retries"][ODD] > 0).all() and (r0["reg_retries"] == 0).all()
    assert (st1 == -1).all()                                  # the last backward pass of every problem factored
    assert np.isfinite(x1).all() and np.isfinite(u1).all()


def test_stop_when_running_at_most_with_retry():
    """altro_hip_solve_options::stop_when_running_at_most on a retrying plan GENERIC solve: the call returns once at most that many
    problems run, with the rescued problems' retries counted.  Without the feature: ALTRO_HIP_ERR_UNSUPPORTED."""
    pr = recipe(14, 5)
    bt = make_hip(pr, plan=altro_amd.PLAN_GENERIC)
    assert bt.plan == altro_amd.PLAN_GENERIC
    res = bt.ilqr_solve(iterations_max=30, stop_when_running_at_most=BATCH, **RETRY)
    assert res["sweeps"] == 1                                 # (ten or fewer run after the first sweep)
    retries, K, P = expected(Schedule(dense_arrays(pr)), res)
    assert np.array_equal(res["reg_retries"], retries) and np.array_equal(bt.get("K"), K)
    bt.close()


def test_retry_fp32_and_argument_checks():
    """fp32 records on plan GENERIC: the retry rescues the odd problems (no count is compared with fp64's).  The option checks every
    plan applies hold here too.  Without the feature the fp32 solve answers ALTRO_HIP_ERR_UNSUPPORTED, and reg_scale = 0.5 raises for
    that reason, not for its own."""
    pr = recipe(14, 5)
    bt = make_hip(pr, dtype=altro_amd.F32)
    assert bt.plan == altro_amd.PLAN_GENERIC
    res = bt.ilqr_solve(iterations_max=1, **RETRY)
    assert (bt.get("status") == -1).all() and np.isfinite(bt.get("K")).all()
    assert (res["reg_retries"][~ODD] == 0).all() and (res["reg_retries"][ODD] > 0).all()
    bt.close()
    bt = make_hip(pr, plan=altro_amd.PLAN_GENERIC)
    with pytest.raises(altro_amd.AltroHipError, match="reg_scale > 1"):
        bt.ilqr_solve(iterations_max=1, reg_retry_max=2, reg_scale=0.5)
    with pytest.raises(altro_amd.AltroHipError, match="reg_initial >= 0"):
        bt.ilqr_solve(iterations_max=1, reg_initial=-1.0)
    bt.close()
