"""Device models on the (12, 4) tile plan with MORE THAN TWO constraint slots at a knot point.

Plan MFMA16 holds AL_TILE_MAXC = 6 slots of eight rows per knot point (kernels/al_types.h).  tests/test_gpu_tile_slots.py covers such
tables with dynamics given as data, tests/test_gpu_tile_model.py covers device models with one 2-row block.  The combination runs
kernels nothing else runs:
  * a model from source (altro_hip_set_model_source): the run-time compiled merit kernels, which are instantiated for two slots or for
    AL_TILE_MAXC -- rtc_unit_tile's `wide` -- while the expansion, dual-update and feasibility kernels around them are the compiled-in
    ones and see every slot.  A two-slot merit kernel on a four-slot table evaluates a merit function without the state box: the line
    search then minimises another function than the one the sweep expanded, and the solve ends somewhere else without an error;
  * the compiled-in MODEL_QUADROTOR: ilqr_launch_mfma16_wide.hip's four instantiations.

Tables (slots of eight rows): an input box |u - hover| (1), a state box (24 rows: 3), optionally a 4-row second-order cone on the
torques u[1:4] (1), an equality pin of u_0[0] at k = 0 (1), a 24-row terminal box (3).  `slots2` = input box + pin (the control: what the
two-slot kernels carry), `slots4` = input box + state box, `slots6` = all of them (5 slots at a running knot point, 6 at k = 0);
`slots5` is `slots6` without the cone (the whole solves' soc = False), `slots1` the input box alone.

The widths below were chosen on the CPU with the oracle alone so that a test cannot pass for the wrong reason; the tests assert it:
  (a) every slot 0..5 of `slots6` has a violated row at some compared (problem, knot point) -- the cone's slot: a point outside the cone;
  (b) the oracle's phi and phi' at alpha = 1 with only the blocks of slots 0 and 1 registered differ from those with all blocks by more
      than 1e-3 relative, for every problem and both penalties: a kernel that drops slots 2..5 cannot pass.

Tolerances are those of tests/test_gpu_tile_model.py for the same comparison (phi 1e-10, phi' 1e-8 relative, candidates 2e-9 / 2e-8,
lx / lu 1e-11, gains 1e-8, feasibility and stationarity 1e-7 relative); source against compiled-in: phi 1e-10, phi' 1e-8, whole solves
equal status and iterations and trajectories 1e-10 / 1e-9; whole solves against the oracle: status and iterations equal (model handles
run no affine line-search rounds), trajectories 1e-6 / 1e-5.

Run-time compiles: (QUADROTOR_SRC: blocks, diagonal | dense, two slots | wide) = 4 and (PLANAR_SRC: blocks, diagonal, wide) = 1 tile
units, one unit of plan GENERIC's loop for PLANAR_SRC.  Blocks and cost are set BEFORE the source so that no handle compiles a unit
it does not launch.
"""
import functools

import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import problems
from tests import test_gpu_tile_model as tm
from tests.test_gpu_tile_model import HOVER, PLANAR_SRC, QUADROTOR_SRC

pytestmark = pytest.mark.gpu

n, m = 12, 4
w = n + m
H = tm.H
BATCH = 7            # merit: two problems per wave, expansion: four -- a ragged last wave in both
N_EVAL, N_SOLVE = 10, 20
RHOS = (1.0, 50.0)   # (penalty 50: the constraint term is not dwarfed by the cost)
ALPHAS = np.linspace(0.0, 1.1, BATCH)
KINDS = ("MODEL_QUADROTOR", "source")

# widths of the single-evaluation tables (chosen on the CPU, see the module docstring)
EVAL_UB = np.array([0.4, 0.004, 0.004, 0.004])
EVAL_XB = np.array([0.5, 0.5, 0.5, 0.08, 0.08, 0.08, 0.2, 0.2, 0.2, 0.1, 0.1, 0.1])
EVAL_XT = 0.8 * EVAL_XB
EVAL_CONE = 0.005
PIN = 1.03 * HOVER[0]


def tables(N, ub, xb, xt, cone, table):
    """The blocks of `table`, in slot order: input box (slot 0), state box (1..3), cone (4), pin at k = 0 (5; slot 1 of `slots2`),
    terminal box (slots 0..2 of knot point N)."""
    Gu = np.zeros((2 * m, w)); Gu[:m, n:] = np.eye(m); Gu[m:, n:] = -np.eye(m)
    Gx = np.zeros((2 * n, w)); Gx[:n, :n] = np.eye(n); Gx[n:, :n] = -np.eye(n)
    gu = np.concatenate([HOVER + ub, -HOVER + ub])
    Ge = np.zeros((1, w)); Ge[0, n] = 1.0
    box_u = (0, N - 1, altro_amd.CONE_INEQUALITY, Gu, gu)
    box_x = (0, N - 1, altro_amd.CONE_INEQUALITY, Gx, np.concatenate([xb, xb]))
    box_t = (N, N, altro_amd.CONE_INEQUALITY, Gx, np.concatenate([xt, xt]))
    pin = (0, 0, altro_amd.CONE_EQUALITY, Ge, np.array([PIN]))
    Gs = np.zeros((4, w)); Gs[0, n + 1] = Gs[1, n + 2] = Gs[2, n + 3] = 1.0
    soc = (0, N - 1, altro_amd.CONE_SOC, Gs, np.array([0.0, 0.0, 0.0, -cone]))
    return {"slots1": [box_u], "slots2": [box_u, pin], "slots4": [box_u, box_x], "slots5": [box_u, box_x, pin, box_t],
            "slots6": [box_u, box_x, soc, pin, box_t]}[table]


def eval_blocks(table):
    return tables(N_EVAL, EVAL_UB, EVAL_XB, EVAL_XT, EVAL_CONE, table)


def knot_slots(blocks, N):
    """Per knot point the slots the tile plan makes of `blocks`: (cone, G, g) of at most eight rows each, a second-order cone one slot."""
    out = [[] for _ in range(N + 1)]
    for (k0, k1, cone, G, g) in blocks:
        parts = [(cone, G, g)] if cone == altro_amd.CONE_SOC else [(cone, G[r:r + 8], g[r:r + 8]) for r in range(0, G.shape[0], 8)]
        for k in range(k0, k1 + 1):
            out[k] += parts
    return out


def first_two_slots(blocks, N):
    """What a two-slot kernel sees of `blocks`: slots 0 and 1 of every knot point, as blocks of their own."""
    return [(k, k, cone, G, g) for k, sl in enumerate(knot_slots(blocks, N)) for (cone, G, g) in sl[:2]]


def slot_violations(blocks, N, x, u):
    """viol[k][s]: the largest violation of a row of slot s at knot point k on the trajectory (x, u); a cone: the distance ||v|| - t outside it."""
    out = []
    for k, sl in enumerate(knot_slots(blocks, N)):
        z = np.concatenate([x[k], u[k] if k < N else np.zeros(m)])
        row = []
        for (cone, G, g) in sl:
            val = G @ z - g
            if cone == altro_amd.CONE_SOC:
                row.append(max(0.0, float(np.linalg.norm(val[:-1]) - val[-1])))
            elif cone == altro_amd.CONE_EQUALITY:
                row.append(float(np.abs(val).max()))
            else:
                row.append(max(0.0, float(val.max())))
        out.append(row)
    return out


@functools.lru_cache(maxsize=None)
def make_case(dense, N):
    """tests/test_gpu_tile_model.py's problem (fly from a perturbed state to hover) on the first N knot points of its horizon."""
    c = tm.make_case(BATCH, dense)
    if dense:
        for key, cnt in (("Q", N + 1), ("R", N), ("H", N), ("q", N + 1), ("r", N), ("c", N + 1)):
            c[key] = np.ascontiguousarray(c[key][:, :cnt])
    return c


def make_hip(c, dense, N, kind, blocks):
    """Blocks and cost first, the model last: a handle from source then compiles the one unit it launches."""
    bt = altro_amd.Batch(N, n, m, BATCH)
    assert bt.plan == altro_amd.PLAN_MFMA16
    for (k0, k1, cone, G, g) in blocks:
        bt.add_linear_constraint(k0, k1, cone, G, g)
    if dense:
        bt.set_quadratic_cost(c["Q"], c["R"], c["H"], c["q"], c["r"], c["c"])
    else:
        bt.set_tracking_cost(np.stack([c["Qd"], c["Qfd"]]), c["Rd"][None], np.stack([c["xref"], c["xref"]]), c["uref"][None],
                             k_stride_zero=True, batch_stride_zero=True)
    if kind == "source":
        bt.set_model_source(QUADROTOR_SRC, H)
    else:
        bt.set_model(altro_amd.MODEL_QUADROTOR, H)
    bt.set_initial_state(c["x0"])
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    return bt


def sweep(bt, c, rho=1.0):
    """The input guess rolled out and accepted, duals zero at penalty rho, expansion and backward sweep: the handle ready for merit evaluations."""
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)   # (a merit evaluation overwrites the candidate's inputs)
    bt.open_loop_rollout(); bt.accept()
    bt.reset_duals(rho)
    bt.expand(); bt.backward()
    assert (bt.get("status") == -1).all()


def make_oracle(c, b, dense, N, blocks):
    """tests/test_gpu_tile_model.py's make_oracle for a horizon of N."""
    s = oracle.ILQR(N, n, m, H, oracle.DYN_MODEL, oracle.MODEL_QUADROTOR, cost_kind=oracle.COST_QUADRATIC if dense else oracle.COST_DIAGONAL)
    for k in range(N + 1):
        kk = min(k, N - 1)
        if dense:
            s.L.oracle_ilqr_set_quadratic_cost(s.h, k, np.ascontiguousarray(c["Q"][b, k]), np.ascontiguousarray(c["R"][b, kk]).ctypes.data,
                                               np.ascontiguousarray(c["H"][b, kk]).ctypes.data, np.ascontiguousarray(c["q"][b, k]),
                                               np.ascontiguousarray(c["r"][b, kk]).ctypes.data, float(c["c"][b, k]))
        else:
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


def oracle_sweep(c, b, dense, N, blocks, rho):
    """Rollout, the expansion at penalty rho with zero duals, the backward sweep: the oracle ready for merit evaluations."""
    s = make_oracle(c, b, dense, N, blocks)
    s.L.oracle_ilqr_open_loop_rollout(s.h); s.L.oracle_ilqr_copy_trajectory(s.h)
    if rho != 1.0:                                   # every block's penalty: 1 (Initialize) times rho
        s.set_penalty(1.0, rho)
        s.L.oracle_ilqr_penalty_update(s.h)
    s.L.oracle_ilqr_calc_cost(s.h)                   # constraint values and projected duals of the rolled-out trajectory
    s.L.oracle_ilqr_calc_dynamics_expansions(s.h); s.L.oracle_ilqr_calc_cost_gradient(s.h)
    s.L.oracle_ilqr_calc_expansions(s.h)
    return s


@functools.lru_cache(maxsize=None)
def merit_reference(table, dense):
    """The oracle's side of test_wide_merit_vs_oracle, once per (table, cost) for both kinds of model: per penalty and problem lx, lu, K,
    phi / phi' at the problem's alpha and at 0, the candidate, its feasibility, stationarity and slot violations."""
    c = make_case(dense, N_EVAL)
    blocks = eval_blocks(table)
    ref = {}
    for rho in RHOS:
        for b in range(BATCH):
            s = oracle_sweep(c, b, dense, N_EVAL, blocks, rho)
            r = dict(lx=s.get("lx"), lu=s.get("lu"))
            assert s.L.oracle_ilqr_backward_pass(s.h) == -1
            r["K"] = s.get("K")
            r["phi0"], r["dphi0"] = s.merit(0.0)
            r["phi"], r["dphi"] = s.merit(ALPHAS[b])
            r["x"], r["u"] = s.get("x_cand"), s.get("u_cand")
            r["feas"] = s.feasibility()
            r["stat"] = s.L.oracle_ilqr_stationarity(s.h)
            r["viol"] = slot_violations(blocks, N_EVAL, r["x"], r["u"])
            ref[(rho, b)] = r
    return ref


@functools.lru_cache(maxsize=None)
def dropped_slots_gap(table, dense):
    """Condition (b): min over penalties and problems of the relative difference of phi (phi') at alpha = 1 between the oracle with all
    blocks and the oracle with the blocks of slots 0 and 1 only."""
    c = make_case(dense, N_EVAL)
    blocks = eval_blocks(table)
    gap_phi, gap_dphi = np.inf, np.inf
    for rho in RHOS:
        for b in range(BATCH):
            out = []
            for bl in (blocks, first_two_slots(blocks, N_EVAL)):
                s = oracle_sweep(c, b, dense, N_EVAL, bl, rho)
                assert s.L.oracle_ilqr_backward_pass(s.h) == -1
                out.append(s.merit(1.0))
            (pa, da), (pn, dn) = out
            gap_phi = min(gap_phi, abs(pa - pn) / max(1.0, abs(pa)))
            gap_dphi = min(gap_dphi, abs(da - dn) / max(1.0, abs(da)))
    return gap_phi, gap_dphi


def check_conditions(table, dense):
    """(a) and (b) of the module docstring, from the oracle and numpy alone."""
    if table == "slots2":
        return
    ref = merit_reference(table, dense)
    if table == "slots6":
        worst = np.zeros(6)
        for r in ref.values():
            for row in r["viol"]:
                for sidx, v in enumerate(row):
                    worst[sidx] = max(worst[sidx], v)
        assert (worst > 1e-4).all(), worst                     # (a): every slot has a violated row somewhere (slot 4: outside the cone)
    gap_phi, gap_dphi = dropped_slots_gap(table, dense)
    assert gap_phi > 1e-3 and gap_dphi > 1e-3, (gap_phi, gap_dphi)   # (b)


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("table", ["slots2", "slots4", "slots6"])
@pytest.mark.parametrize("kind", KINDS)
def test_wide_merit_vs_oracle(kind, table, dense):
    """One sweep's kernels against the oracle for every problem of the batch, at penalties 1 and 50: the expansion's lx, lu (1e-11), the
    gains K (1e-8), phi (1e-10) and phi' (1e-8) at a different alpha per problem in [0, 1.1] and at alpha = 0, the candidate x / u
    (2e-9 / 2e-8), its feasibility and stationarity (1e-7 relative).
    Measured maxima over the twelve cases (MI355X; the same for both kinds of model to the figures given): lx 1.8e-14 and lu 8.9e-16
    absolute, K 6.7e-16, phi 2.5e-15, phi' 5.1e-15, x 3.6e-15 and u 1.2e-14 absolute, feasibility 1.8e-15, stationarity 6.8e-15.
    With the two-slot merit kernels on the wider tables (the defect this file was written for): phi off by 0.50 -- 0.6 % -- in the first
    problem of `slots4`, 0.51 of `slots6`; `slots2` unaffected."""
    check_conditions(table, dense)
    c = make_case(dense, N_EVAL)
    ref = merit_reference(table, dense)
    bt = make_hip(c, dense, N_EVAL, kind, eval_blocks(table))
    worst = {}

    def note(key, err, tol):
        worst[key] = max(worst.get(key, 0.0), float(err))
        return err <= tol

    for rho in RHOS:
        sweep(bt, c, rho)
        _, _, lx, lu = bt.get_expansion()          # (of the rolled-out trajectory: no merit pass has run since the expansion)
        K = bt.get("K")
        phi0, dphi0 = bt.merit(np.zeros(BATCH))
        phi, dphi = bt.merit(ALPHAS)
        xc, uc = bt.get("x"), bt.get("u")
        feas = bt.feasibility()
        st = bt.stationarity()
        for b in range(BATCH):
            r = ref[(rho, b)]
            tag = (rho, b)
            note("lx", np.abs(lx[b] - r["lx"]).max(), 0.0); note("lu", np.abs(lu[b] - r["lu"]).max(), 0.0)     # (absolute, for the record)
            np.testing.assert_allclose(lx[b], r["lx"], rtol=1e-11, atol=1e-11, err_msg="lx %s" % (tag,))
            np.testing.assert_allclose(lu[b], r["lu"], rtol=1e-11, atol=1e-11, err_msg="lu %s" % (tag,))
            assert note("K", np.abs(K[b] - r["K"]).max() / max(1.0, np.abs(r["K"]).max()), 1e-8), ("K", tag)
            for name, got, want, tol in (("phi0", phi0[b], r["phi0"], 1e-10), ("dphi0", dphi0[b], r["dphi0"], 1e-8),
                                         ("phi", phi[b], r["phi"], 1e-10), ("dphi", dphi[b], r["dphi"], 1e-8)):
                assert note(name, abs(got - want) / max(1.0, abs(want)), tol), (name, tag, got, want)
            note("x", np.abs(xc[b] - r["x"]).max(), 0.0); note("u", np.abs(uc[b] - r["u"]).max(), 0.0)
            np.testing.assert_allclose(xc[b], r["x"], rtol=2e-9, atol=2e-9, err_msg="x %s" % (tag,))
            np.testing.assert_allclose(uc[b], r["u"], rtol=2e-8, atol=2e-8, err_msg="u %s" % (tag,))
            assert note("feas", abs(feas[b] - r["feas"]) / max(1.0, r["feas"]), 1e-7), ("feas", tag, feas[b], r["feas"])
            assert note("stat", abs(st[b] - r["stat"]) / max(1.0, r["stat"]), 1e-7), ("stat", tag, st[b], r["stat"])
    print("measured maxima (lx, lu, x, u absolute, the others relative):", {k: "%.1e" % v for k, v in worst.items()})
    bt.close()


# ---- whole solves -----------------------------------------------------------------------------------------------------------
# Widths chosen with the oracle (N = 20): the body-rate bound (states 9..11) lies below what every unconstrained solve reaches and
# above every initial state, so the state box binds in every problem; thrust bound, cone and terminal velocity bound bind in some.
# Diagonal cost: the oracle converges on all seven problems, with and without the cone (test_source_equals_compiled_in_on_wide_tables
# compares every problem at 1e-10, and a solve whose line search FAILS has no answer at that level: with a cone of 0.12 and a terminal
# velocity bound of 0.5 problems 5 and 6 end with status 1 after 22 and 19 sweeps in the oracle and on both kinds of handle alike, the
# two handles then 1.5e-7 and 1.9e-4 apart and 3.5e-8 .. 1.2e-4 from the oracle -- the last, failing search amplifies differences in the
# last bit -- while the five converged problems agree to 4e-15).  Dense cost: problems 2, 3 and 5 fail in the oracle; SAMPLES are three
# that converge.
SOLVE = {False: dict(ub=np.array([6.0, 0.2, 0.2, 0.2]), rate=1.0, cone=0.14, vel_t=0.8),
         True: dict(ub=np.array([2.5, 0.09, 0.09, 0.09]), rate=0.5, cone=0.095, vel_t=0.5)}
SAMPLES = {False: (0, 3, 5), True: (0, 4, 6)}


def solve_blocks(table, dense):
    wd = SOLVE[dense]
    xb = np.array([3.0] * 3 + [0.6] * 3 + [3.0] * 3 + [wd["rate"]] * 3)
    xt = np.array([3.0] * 3 + [0.6] * 3 + [wd["vel_t"]] * 3 + [wd["rate"]] * 3)
    return tables(N_SOLVE, wd["ub"], xb, xt, wd["cone"], table), xb, xt


SOLVE_OPTIONS = dict(iterations_max=50, tol_stationarity=1e-3, penalty_initial=1.0, penalty_scaling=10.0)


def test_source_equals_compiled_in_on_wide_tables():
    """QUADROTOR_SRC and MODEL_QUADROTOR on `slots4` and `slots6` (same equations, the same kernels around them): single merit
    evaluations phi 1e-10, phi' 1e-8; whole solves end with the same status and iteration count in every problem, trajectories 1e-10 / 1e-9."""
    for table in ("slots4", "slots6"):
        c = make_case(False, N_EVAL)
        out = {}
        for kind in KINDS:
            bt = make_hip(c, False, N_EVAL, kind, eval_blocks(table))
            sweep(bt, c, 50.0)
            out[kind] = bt.merit(ALPHAS)
            bt.close()
        (pa, da), (pb, db) = out["source"], out["MODEL_QUADROTOR"]
        assert (np.abs(pa - pb) <= 1e-10 * np.maximum(1.0, np.abs(pb))).all(), (table, pa, pb)
        assert (np.abs(da - db) <= 1e-8 * np.maximum(1.0, np.abs(db))).all(), (table, da, db)
        c = make_case(False, N_SOLVE)
        for kind in KINDS:
            bt = make_hip(c, False, N_SOLVE, kind, solve_blocks(table, False)[0])
            res = bt.ilqr_solve(**SOLVE_OPTIONS)
            out[kind] = (res, bt.get_nominal())
            bt.close()
        (r_src, (x_src, u_src)), (r_mod, (x_mod, u_mod)) = out["source"], out["MODEL_QUADROTOR"]
        assert np.array_equal(r_src["status"], r_mod["status"]) and np.array_equal(r_src["iterations"], r_mod["iterations"]), \
            (table, r_src["status"], r_mod["status"], r_src["iterations"], r_mod["iterations"])
        np.testing.assert_allclose(x_src, x_mod, rtol=1e-10, atol=1e-10, err_msg=table)
        np.testing.assert_allclose(u_src, u_mod, rtol=1e-9, atol=1e-9, err_msg=table)


@functools.lru_cache(maxsize=None)
def solve_reference(soc, dense):
    """The oracle's solves of the sampled problems, once for both kinds of model."""
    c = make_case(dense, N_SOLVE)
    blocks, _, _ = solve_blocks("slots6" if soc else "slots5", dense)
    ref = {}
    for b in SAMPLES[dense]:
        s = make_oracle(c, b, dense, N_SOLVE, blocks)
        s.set_penalty(1.0, 10.0)
        s.L.oracle_ilqr_set_options(s.h, 50, 1e-3, 1e-4, 1e-8, 0)
        status, iters, _ = s.solve()
        ref[b] = dict(status=status, iters=iters, x=s.get("x"), u=s.get("u"))
    return ref


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("soc", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_wide_model_solves_equal_oracle(kind, soc, dense):
    """Input box + state box (+ cone) + pinned first thrust + terminal box around a device model: the sampled problems end with the
    oracle's status and iteration count (strictly: model handles run no affine rounds), converged ones with its trajectory (1e-6 / 1e-5)
    inside the boxes (2e-4); the state box binds in a compared problem and has duals somewhere in the batch."""
    c = make_case(dense, N_SOLVE)
    blocks, xb, xt = solve_blocks("slots6" if soc else "slots5", dense)
    ub = SOLVE[dense]["ub"]
    bt = make_hip(c, dense, N_SOLVE, kind, blocks)
    res = bt.ilqr_solve(**SOLVE_OPTIONS)
    x, u = bt.get_nominal()
    ref = solve_reference(soc, dense)
    nconv = nbind = 0
    for b in SAMPLES[dense]:
        r = ref[b]
        assert res["status"][b] == r["status"] and res["iterations"][b] == r["iters"], (b, res["status"][b], r["status"], res["iterations"][b], r["iters"])
        if r["status"] != 0:
            continue
        nconv += 1
        np.testing.assert_allclose(x[b], r["x"], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(u[b], r["u"], rtol=1e-5, atol=1e-5)
        assert (np.abs(u[b] - HOVER) <= ub + 2e-4).all() and (np.abs(x[b][:N_SOLVE]) <= xb + 2e-4).all() and (np.abs(x[b][N_SOLVE]) <= xt + 2e-4).all()
        assert abs(u[b][0, 0] - PIN) < 2e-4
        if soc:
            assert np.linalg.norm(u[b][:, 1:], axis=1).max() <= SOLVE[dense]["cone"] + 2e-4
        nbind += int((np.abs(x[b][:N_SOLVE]) >= xb - 1e-3).any())
    assert nconv >= 2 and nbind >= 1, (nconv, nbind)
    z = np.stack([bt.get_duals(k, 1, 2 * n) for k in range(1, N_SOLVE)])      # block 1 of a running knot point: the state box
    assert (z <= 1e-12).all() and (z < 0).any()
    bt.close()


def test_padded_source_model_wide_table_equals_plan_generic():
    """The (6, 2) planar quadrotor from source rides the tile zero-padded with an input box (4 rows), a state box (12 rows: 2 slots)
    and a terminal box -- three slots -- against the same source and blocks on plan GENERIC (lane-per-row kernels, 8 blocks of 64
    rows): phi, phi', lx, lu, feasibility at 1e-10 relative; whole solves: the same iteration count in all problems but one at most,
    trajectories 1e-7 / 1e-6 on those."""
    nn, mm, ww = 6, 2, 8
    hp = np.float32(0.05)
    x0 = np.zeros((BATCH, nn)); x0[:, :2] = 0.6 * problems.normal((BATCH, 2), 141); x0[:, 2] = 0.2 * problems.normal((BATCH,), 142)
    Qd = np.array([2.0, 2.0, 1.0, 0.3, 0.3, 0.1]); Rd = np.array([0.1, 0.1]); uh = np.full(2, 0.5 * 9.81)
    Gu = np.zeros((2 * mm, ww)); Gu[:mm, nn:] = np.eye(mm); Gu[mm:, nn:] = -np.eye(mm)
    Gx = np.zeros((2 * nn, ww)); Gx[:nn, :nn] = np.eye(nn); Gx[nn:, :nn] = -np.eye(nn)

    def handles(N, ub, xb, xt):
        blocks = [(0, N - 1, altro_amd.CONE_INEQUALITY, Gu, np.concatenate([uh + ub, -uh + ub])),
                  (0, N - 1, altro_amd.CONE_INEQUALITY, Gx, np.concatenate([xb, xb])), (N, N, altro_amd.CONE_INEQUALITY, Gx, np.concatenate([xt, xt]))]
        for plan in (altro_amd.PLAN_MFMA16, altro_amd.PLAN_GENERIC):
            bt = altro_amd.Batch(N, nn, mm, BATCH, plan=plan)
            assert bt.plan == plan
            for (k0, k1, cone, G, g) in blocks:
                bt.add_linear_constraint(k0, k1, cone, G, g)
            bt.set_tracking_cost(np.stack([Qd, 30.0 * Qd]), Rd[None], np.zeros((2, nn)), uh[None], k_stride_zero=True, batch_stride_zero=True)
            bt.set_model_source(PLANAR_SRC, hp)
            bt.set_initial_state(x0)
            bt.set_input_guess(uh[None, None], k_stride_zero=True, batch_stride_zero=True)
            yield bt

    # single evaluations: widths inside the rolled-out trajectory, so that all three slots have violated rows
    xb = np.array([0.3, 0.3, 0.1, 0.05, 0.05, 0.05])
    out = []
    for bt in handles(N_EVAL, np.array([0.5, 0.5]), xb, 0.8 * xb):
        bt.open_loop_rollout(); bt.accept(); bt.reset_duals(50.0); bt.expand(); bt.backward()
        assert (bt.get("status") == -1).all()
        phi0, dphi0 = bt.merit(np.zeros(BATCH))
        _, _, lx, lu = bt.get_expansion()
        phi, dphi = bt.merit(np.linspace(0.05, 1.1, BATCH))
        out.append(dict(phi=phi, dphi=dphi, phi0=phi0, dphi0=dphi0, lx=lx, lu=lu, feas=bt.feasibility(), x=bt.get("x")[:, :N_EVAL + 1, :nn].copy()))
        bt.close()
    xc = out[0].pop("x"); out[1].pop("x")
    over = np.concatenate([xc[:, :N_EVAL] - xb, -xc[:, :N_EVAL] - xb], axis=2)            # the state box's 12 rows at the candidate's running knot points
    assert (over[:, :, :8] > 1e-3).any() and (over[:, :, 8:] > 1e-3).any()              # slots 1 and 2 both have a violated row
    for key in out[0]:
        a, b = np.asarray(out[0][key]), np.asarray(out[1][key])
        np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * max(1.0, float(np.abs(b).max())), err_msg=key)
    assert float(np.max(out[0]["feas"])) > 0.0
    # whole solves: a box the initial states lie in
    xb = np.array([2.5, 2.5, 0.6, 1.0, 1.0, 0.8])
    xt = np.array([2.5, 2.5, 0.6, 0.5, 0.5, 0.8])
    sol = []
    for bt in handles(N_SOLVE, np.array([2.0, 2.0]), xb, xt):
        res = bt.ilqr_solve(iterations_max=60, tol_stationarity=1e-3, penalty_initial=1.0, penalty_scaling=10.0)
        sol.append((res, *bt.get_nominal()))
        bt.close()
    (ra, xa, ua), (rb, xg, ug) = sol
    same = ra["iterations"] == rb["iterations"]
    print("padded planar solves: status", ra["status"], rb["status"], "iterations", ra["iterations"], rb["iterations"])
    assert same.sum() >= BATCH - 1, (ra["iterations"], rb["iterations"])
    np.testing.assert_allclose(xa[same], xg[same], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(ua[same], ug[same], rtol=1e-6, atol=1e-6)


def test_slot_count_changes_rebuild_the_module():
    """A handle from source whose table grows past two slots, and shrinks again, launches the merit kernels of the width it has NOW:
    phi and phi' are the bits of a fresh handle built with the same blocks (and the oracle's values, so that two handles that are wrong
    in the same way do not pass).  Fails when the handle's record of what its module was built for, or the module cache's key, lacks the width."""
    c = make_case(False, N_EVAL)
    box_u, box_x = eval_blocks("slots4")

    def merit(bt):
        sweep(bt, c)
        return bt.merit(ALPHAS)

    def equals_oracle(got, table):
        ref = merit_reference(table, False)
        return all(abs(got[0][b] - ref[(1.0, b)]["phi"]) <= 1e-10 * max(1.0, abs(ref[(1.0, b)]["phi"])) and
                   abs(got[1][b] - ref[(1.0, b)]["dphi"]) <= 1e-8 * max(1.0, abs(ref[(1.0, b)]["dphi"])) for b in range(BATCH))

    bt = make_hip(c, False, N_EVAL, "source", [box_u])
    first = merit(bt)
    bt.add_linear_constraint(*box_x)
    grown = merit(bt)
    fresh_wide = make_hip(c, False, N_EVAL, "source", [box_u, box_x])
    wide = merit(fresh_wide)
    assert np.array_equal(grown[0], wide[0]) and np.array_equal(grown[1], wide[1]), (grown, wide)
    assert equals_oracle(wide, "slots4"), wide
    bt.clear_constraints()
    bt.add_linear_constraint(*box_u)
    shrunk = merit(bt)
    fresh_narrow = make_hip(c, False, N_EVAL, "source", [box_u])
    narrow = merit(fresh_narrow)
    assert np.array_equal(shrunk[0], narrow[0]) and np.array_equal(shrunk[1], narrow[1]), (shrunk, narrow)
    assert np.array_equal(first[0], narrow[0]) and np.array_equal(first[1], narrow[1])
    assert equals_oracle(narrow, "slots1"), narrow
    assert not np.array_equal(narrow[0], wide[0])
    for h in (bt, fresh_wide, fresh_narrow):
        h.close()
