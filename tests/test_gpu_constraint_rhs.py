"""Constraint right-hand sides per knot point: altro_hip_add_linear_constraint_rhs / _set_constraint_rhs / _get_constraint_rhs /
_shift_constraint_rhs on every plan.

  1. round trips, exact (fp32: the value as a float): whole range and sub-ranges, K in {1, 2, 16, 17, 33, 70}, shared and per problem,
     p in {1, 2, 8, 24}, neighbouring blocks unchanged, old-style blocks through (-1, -1);
  2. a per-knot handle against its twin -- one old-style definition per knot point, what the library could express before --, bit for bit:
     solve results, trajectory, duals, merit / feasibility / stationarity; and again after set_constraint_rhs replaced half the range,
     against a twin built fresh with the new values;
  3. against the oracle, which registers per knot point anyway: the bicycle with a steering bound that tightens along the horizon, and
     the (12, 4) tile's input box scaled per knot point and per problem, phase by phase;
  4. shift_constraint_rhs against numpy, bit for bit, twice in a row;
  5. five closed-loop MPC steps whose bound moves with the horizon, the handle against one built fresh at every step;
  6. the host description does not go stale: a shift, then one more block (which rebuilds the tables);
  7. device pointers: tests/cpp/constraint_rhs_test.cpp;
  8. errors and no-ops.
Shapes: those of tests/test_gpu_dual_warmstart.py::SHAPES (LANE (4, 2) batch 66 in fp64 and fp32, the (12, 4) tile, MFMA32 (13, 4), GENERIC
(14, 9) in both types); the bare handles of parts 1 and 4 have N = 70 to hold the ranges, the solves N = 12 so that the twin's definitions fit.
"""
import types

import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import cone_region_cases as crc
from tests import cpp_build
from tests import mpc_common as M
from tests import problems
from tests.test_gpu_cone_regions import compare, hip_phases
from tests.test_gpu_dual_warmstart import SHAPES

pytestmark = pytest.mark.gpu

EQ, INEQ, SOC = oracle.CONE_EQUALITY, oracle.CONE_INEQUALITY, oracle.CONE_SOC
NB = 70     # horizon of the bare handles


def rhs_layout(wide):
    """(k_first, K, p, per problem, per knot) in registration order, N = 70: ranges of 70, 33, 17, 16, 2 and 1 knot points, one that reaches
    N, two old-style blocks; at most two blocks per knot point and eight rows (plan LANE's capacity) unless `wide` (a 24-row block: three
    slots on the tile)."""
    return [(0, 70, 24 if wide else 8, True, True), (0, 33, 2, False, True), (33, 17, 1, True, True), (50, 16, 8, False, True),
            (66, 2, 2, True, True), (68, 1, 1, False, True), (69, 2, 3, True, False), (70, 1, 2, False, False)]


def g_shape(batch, K, p, pp, pk):
    return ((batch,) if pp else ()) + ((K,) if pk else ()) + (p,)


def rhs_handle(name, values):
    """A handle with the layout's blocks and nothing else: the right-hand side calls need no dynamics and no cost."""
    plan, n, m, _, batch, dtype, wide = SHAPES[name]
    bt = altro_amd.Batch(NB, n, m, batch, dtype=dtype, plan=altro_amd.PLAN_GENERIC if plan == altro_amd.PLAN_GENERIC else altro_amd.PLAN_AUTO)
    assert bt.plan == plan, (name, bt.plan)
    blocks = rhs_layout(wide)
    rng = np.random.default_rng(5)
    g = []
    for j, (k0, K, p, pp, pk) in enumerate(blocks):
        g.append(values(j, g_shape(batch, K, p, pp, pk)))
        assert bt.add_linear_constraint(k0, k0 + K - 1, INEQ, rng.normal(size=(p, n + m)), g[j], per_knot=pk) == j
    return bt, blocks, g


def at_knot(gj, block, k):
    """What get_constraint_rhs(j, k) must return of a block's full array."""
    k0, K, p, pp, pk = block
    return gj[..., k - k0, :] if pk else gj


def check_all(bt, blocks, g, f32, tag):
    for j, bl in enumerate(blocks):
        for k in range(bl[0], bl[0] + bl[1]):
            want = at_knot(g[j], bl, k)
            want = want.astype(np.float32).astype(np.float64) if f32 else want
            assert np.array_equal(bt.get_constraint_rhs(j, k), want), (tag, j, k)


# ---- 1. round trips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_round_trip(name):
    rng = np.random.default_rng(11)
    bt, blocks, g = rhs_handle(name, lambda j, shape: rng.normal(size=shape))      # (all 53 bits: fp32 rounds them)
    f32 = SHAPES[name][5] == altro_amd.F32
    check_all(bt, blocks, g, f32, "as registered")
    z0 = bt.get_duals(0, 0, blocks[0][2])
    bt.set_duals(0, 0, z0 + 1.5); bt.set_penalty(7.0)
    for j, (k0, K, p, pp, pk) in enumerate(blocks):                                # one block at a time; every block checked after each
        if pk and K >= 2:                                                          # a sub-range: the middle, or all but the first
            a, b = (k0 + K // 3, k0 + (2 * K) // 3) if K > 2 else (k0 + 1, k0 + 1)
            new = rng.normal(size=g_shape(bt.batch, b - a + 1, p, pp, True))
            bt.set_constraint_rhs(j, new, a, b)
            g[j] = g[j].copy(); g[j][..., a - k0:b - k0 + 1, :] = new
        else:                                                                      # the whole range; old-style blocks take nothing else
            g[j] = rng.normal(size=g[j].shape)
            bt.set_constraint_rhs(j, g[j])
        check_all(bt, blocks, g, f32, ("after block", j))
    g[0] = rng.normal(size=g[0].shape)                                             # the whole range of the longest block, by its numbers
    bt.set_constraint_rhs(0, g[0], 0, 69)
    check_all(bt, blocks, g, f32, "whole range")
    assert np.array_equal(bt.get_duals(0, 0, blocks[0][2]), z0 + 1.5) and np.array_equal(bt.get_penalty(), np.full(bt.batch, 7.0))
    bt.close()


# ---- 4. shift against numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_shift_against_numpy(name):
    count = [0]

    def integers(j, shape):        # distinct everywhere, below 2^24: exact as floats
        v = count[0] + 1.0 + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
        count[0] += v.size
        return v
    bt, blocks, g = rhs_handle(name, integers)
    assert count[0] < 2 ** 24
    for _ in range(2):
        bt.shift_constraint_rhs()
        for j, (k0, K, p, pp, pk) in enumerate(blocks):
            if pk:
                g[j] = g[j].copy(); g[j][..., :-1, :] = g[j][..., 1:, :]
        check_all(bt, blocks, g, False, "shift")
    bt.close()


# ---- 2. a per-knot handle against its twin ------------------------------------------------------------------------------------------
OPTS = dict(use_backtracking=True, penalty_initial=1.0, penalty_scaling=10.0)
NS = 12


def bicycle_maker(N, batch, dtype=altro_amd.F64):
    x_ref, u_ref = problems.bicycle_reference(N + 8)
    off = problems.uniform01((batch, 4), 33) - 0.5
    x0s = x_ref[0] + off * np.array([0.2, 0.2, 0.04, 0.0])

    def make():
        bt = altro_amd.Batch(N, M.n, M.m, batch, dtype=dtype)
        assert bt.plan == altro_amd.PLAN_LANE
        bt.set_model(altro_amd.MODEL_BICYCLE, M.H)
        bt.set_tracking_cost(np.full((1, N + 1, M.n), M.QD), np.full((1, N, M.m), M.RD), x_ref[None, :N + 1], u_ref[None, :N], batch_stride_zero=True)
        bt.set_initial_state(x0s)
        bt.set_input_guess(np.array([u_ref[0][0], 0.0])[None, None], k_stride_zero=True, batch_stride_zero=True)
        return bt
    return make


def data_maker(N, n, m, batch, plan):
    p = problems.ilqr12x4_problem(batch, N, True, n=n, m=m)

    def make():
        bt = altro_amd.Batch(N, n, m, batch, plan=altro_amd.PLAN_GENERIC if plan == altro_amd.PLAN_GENERIC else altro_amd.PLAN_AUTO)
        assert bt.plan == plan
        bt.set_dynamics(p["A"], p["B"], p["f"])
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.set_initial_state(p["x0"])
        bt.set_input_guess(p["u0"])
        return bt
    return make


def input_box(n, m):
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    return G


def twin_case(case):
    """(make, forms, k0, k1, cone, G, g [batch][K][p] or [K][p], first solve's sweeps): g varies with the knot point and the problem."""
    kk = lambda K: np.arange(K)[None, :, None]
    bb = lambda B: np.arange(B)[:, None, None]
    if case.startswith("lane"):
        batch, (cone, G, _) = 66, M.steering_block()
        g = 0.02 * (2.0 - 1.5 * kk(NS + 1) / NS) * (1.0 + 0.05 * (bb(batch) % 4)) * np.ones((1, 1, 2))
        if case == "lane_shared":
            g = g[0]
        forms = altro_amd.FORM_SEQUENCED if case == "lane_sequenced" else 0
        return bicycle_maker(NS, batch, altro_amd.F32 if case == "lane_f32" else altro_amd.F64), forms, 0, NS, cone, G, g, 2
    if case.startswith("tile"):
        batch = 8
        g = 0.3 * (1.0 + 0.3 * np.sin(1.0 + kk(NS) + 0.7 * bb(batch))) * np.ones((1, 1, 8))
        return data_maker(NS, 12, 4, batch, altro_amd.PLAN_MFMA16), altro_amd.FORM_ROLLOUT_ROUNDS if case == "tile_rollout_rounds" else 0, 0, NS - 1, INEQ, input_box(12, 4), g, 6
    if case == "mfma32":
        batch = 9
        g = 0.3 * (1.0 + 0.3 * np.sin(1.0 + kk(NS) + 0.7 * bb(batch))) * np.ones((1, 1, 8))
        return data_maker(NS, 13, 4, batch, altro_amd.PLAN_MFMA32), 0, 0, NS - 1, INEQ, input_box(13, 4), g, 8
    assert case == "generic_soc"       # ||u[0:3]|| <= radius: rows u0, u1, u2 and a zero row whose g is -radius
    batch, n, m = 9, 14, 9
    G = np.zeros((4, n + m)); G[0, n] = G[1, n + 1] = G[2, n + 2] = 1.0
    g = np.zeros((batch, NS, 4)); g[:, :, 3] = -(0.25 * (1.0 + 0.3 * np.sin(1.0 + kk(NS) + 0.7 * bb(batch))))[:, :, 0]
    return data_maker(NS, n, m, batch, altro_amd.PLAN_GENERIC), 0, 0, NS - 1, SOC, G, g, 8


def with_per_knot(make, k0, k1, cone, G, g):
    bt = make()
    assert bt.add_linear_constraint(k0, k1, cone, G, g, per_knot=True) == 0
    return bt


def with_definitions(make, k0, k1, cone, G, g):
    bt = make()
    for k in range(k0, k1 + 1):
        bt.add_linear_constraint(k, k, cone, G, g[..., k - k0, :])
    return bt


def duals_of(bt, k0, k1, p):
    return [bt.get_duals(k, 0, p) for k in range(k0, k1 + 1)]


def assert_same(a, b, k0, k1, p, res, tag):
    for key in ("status", "iterations", "dual_updates", "penalty"):
        assert np.array_equal(res[0][key], res[1][key]), (tag, key, res[0][key], res[1][key])
    for got, want in zip(a.get_nominal(), b.get_nominal()):
        assert np.array_equal(got, want), tag
    for k, (za, zb) in enumerate(zip(duals_of(a, k0, k1, p), duals_of(b, k0, k1, p))):
        assert np.array_equal(za, zb), (tag, "duals", k)
    assert np.array_equal(a.get_penalty(), b.get_penalty()), tag


@pytest.mark.parametrize("case", ["lane_one_launch", "lane_sequenced", "lane_shared", "lane_f32", "tile_default", "tile_rollout_rounds", "mfma32", "generic_soc"])
def test_per_knot_handle_equals_its_twin(case):
    make, forms, k0, k1, cone, G, g, sweeps = twin_case(case)
    p, K = G.shape[0], k1 - k0 + 1
    assert (np.ptp(g, axis=-2) > 0).any(), "g does not vary with the knot point"
    a, twin = with_per_knot(make, k0, k1, cone, G, g), with_definitions(make, k0, k1, cone, G, g)
    first = [bt.ilqr_solve(iterations_max=sweeps, forms=forms, **OPTS) for bt in (a, twin)]
    print(case, "first solve: status", first[0]["status"].tolist(), "dual updates", first[0]["dual_updates"].tolist())
    assert_same(a, twin, k0, k1, p, first, "first solve")
    z, rho = duals_of(a, k0, k1, p), a.get_penalty()
    assert any((v != 0.0).any() for v in z), "the first solve left no duals: the bound is not active"
    _, u = a.get_nominal()
    alphas = np.linspace(0.15, 1.1, a.batch)
    phases = []
    for bt in (a, twin):                                       # the step-wise entries at the solve's end point
        bt.expand(); bt.backward()
        phases.append(bt.merit(alphas) + (bt.feasibility(), bt.stationarity()))
    for got, want in zip(*phases):
        assert np.array_equal(got, want), "merit / feasibility / stationarity"
    twin.close()
    # half the range replaced in place; the twin is built fresh with the new values and given the duals, the penalty and the guess
    h0, h1 = k0 + K // 4, k0 + K // 4 + K // 2 - 1
    g2 = g.copy(); g2[..., h0 - k0:h1 - k0 + 1, :] *= 0.8
    a.set_constraint_rhs(0, g2[..., h0 - k0:h1 - k0 + 1, :], h0, h1)
    assert all(np.array_equal(za, zb) for za, zb in zip(duals_of(a, k0, k1, p), z)) and np.array_equal(a.get_penalty(), rho)
    fresh = with_definitions(make, k0, k1, cone, G, g2)
    for k in range(k0, k1 + 1):
        fresh.set_duals(k, 0, z[k - k0])
    fresh.set_penalty(rho)
    for bt in (a, fresh):
        bt.set_input_guess(u)
    second = [bt.ilqr_solve(iterations_max=40, forms=forms, **OPTS) for bt in (a, fresh)]
    print(case, "second solve: status", second[1]["status"].tolist(), "iterations", second[1]["iterations"].tolist())
    assert_same(a, fresh, k0, k1, p, second, "second solve")
    a.close(); fresh.close()


# ---- 3. against the oracle -------------------------------------------------------------------------------------------------------------
def steering_bound(k):
    return 0.02 * (2.0 - 1.5 * k / M.N)


def test_bicycle_with_a_tightening_bound_against_the_oracle():
    """The six start states of tests/test_gpu_dual_warmstart.py's closed loop; the oracle solves them with status 0 in 3 to 6 iterations
    with the bound active.  Trajectories within 5e-5, the band of tests/test_gpu_al.py's backtracked constrained bicycle solves."""
    batch, N = 6, M.N
    x_ref, u_ref = problems.bicycle_reference(N + 8)
    off = problems.uniform01((batch, 4), 33) - 0.5
    x0s = x_ref[0] + off * np.array([0.2, 0.2, 0.04, 0.0])
    cone, G, _ = M.steering_block()
    g = np.stack([np.full(2, steering_bound(k)) for k in range(N + 1)])
    bt = altro_amd.Batch(N, M.n, M.m, batch)
    bt.set_model(altro_amd.MODEL_BICYCLE, M.H)
    bt.set_tracking_cost(np.full((1, N + 1, M.n), M.QD), np.full((1, N, M.m), M.RD), x_ref[None, :N + 1], u_ref[None, :N], batch_stride_zero=True)
    bt.add_linear_constraint(0, N, cone, G, g, per_knot=True)
    bt.set_initial_state(x0s)
    u0 = np.array([u_ref[0][0], 0.0])
    bt.set_input_guess(u0[None, None], k_stride_zero=True, batch_stride_zero=True)
    res = bt.ilqr_solve(iterations_max=80, use_backtracking=True, tol_primal_feasibility=1e-4, penalty_initial=1.0)
    x, u = bt.get_nominal()
    worst = 0.0
    for b in range(batch):
        s = oracle.ILQR(N, M.n, M.m, M.H, oracle.DYN_MODEL, oracle.MODEL_BICYCLE, cost_kind=oracle.COST_DIAGONAL)
        for k in range(N + 1):
            s.L.oracle_ilqr_set_lqr_cost(s.h, k, np.full(M.n, M.QD), np.full(M.m, M.RD), np.ascontiguousarray(x_ref[k]), np.ascontiguousarray(u_ref[min(k, N - 1)]))
        for k in range(N + 1):
            s.add_linear_constraint(k, cone, G, g[k])
        s.L.oracle_ilqr_set_initial_state(s.h, np.ascontiguousarray(x0s[b]))
        s.L.oracle_ilqr_initialize(s.h)
        for k in range(N):
            s.L.oracle_ilqr_set_input(s.h, k, u0)
        s.L.oracle_ilqr_set_options(s.h, 80, 1e-4, 1e-4, 1e-8, 1)
        status, iters, _ = s.solve()
        print("problem", b, "oracle status", status, "iterations", iters, "handle", res["status"][b], res["iterations"][b])
        assert status == 0 and 3 <= iters <= 6
        assert res["status"][b] == status and res["iterations"][b] == iters
        xo = s.get("x")
        assert (np.abs(xo[:, 3]) >= g[:, 0] - 1e-3).any(), "the bound is not active"
        worst = max(worst, np.abs(x[b] - xo).max(), np.abs(u[b] - s.get("u")).max())
    print("max trajectory difference %.3g" % worst)
    assert worst < 5e-5
    bt.close()


def test_tile_scaled_input_box_against_the_oracle_phase_by_phase():
    """problems.ilqr12x4_constraint_blocks' input box scaled per knot point and per problem; expansion, backward sweep, merit, feasibility
    and stationarity through compare of tests/test_gpu_cone_regions.py at its tolerances."""
    B, N = crc.BATCH, crc.N
    p = problems.ilqr12x4_problem(B, N, True)
    k0, k1, cone, G, g0 = problems.ilqr12x4_constraint_blocks(N)[0]
    scale = 0.5 + 0.5 * problems.uniform01((B, k1 - k0 + 1, 1), 91)
    g = g0[None, None, :] * scale
    bt = altro_amd.Batch(N, 12, 4, B)
    assert bt.plan == altro_amd.PLAN_MFMA16
    bt.set_forms(altro_amd.FORM_ROLLOUT_ROUNDS)
    bt.set_dynamics(p["A"], p["B"], p["f"])
    bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
    bt.set_initial_state(p["x0"])
    bt.set_input_guess(p["u0"])
    bt.add_linear_constraint(k0, k1, cone, G, g, per_knot=True)
    x = 0.3 * problems.normal((B, N + 1, 12), 92); x[:, 0] = p["x0"]
    u = 0.4 * problems.normal((B, N, 4), 93)                    # (inputs on both sides of the scaled bounds)
    cfg = types.SimpleNamespace(plan="MFMA16", N=N)
    worst, bad = {}, []
    for rho in crc.RHOS:
        got = hip_phases(bt, x, u, rho)
        for b in range(B):
            s = oracle.ILQR(N, 12, 4, 0.01, oracle.DYN_LINEAR, cost_kind=oracle.COST_DIAGONAL)
            c = np.ascontiguousarray
            s.L.oracle_ilqr_set_linear_dynamics(s.h, c(p["A"][b]), c(p["B"][b]), c(p["f"][b]).ctypes.data)
            for k in range(N + 1):
                kk = min(k, N - 1)
                s.L.oracle_ilqr_set_lqr_cost(s.h, k, c(p["Qd"][b, k]), c(p["Rd"][b, kk]), c(p["xref"][b, k]), c(p["uref"][b, kk]))
            s.L.oracle_ilqr_set_initial_state(s.h, c(p["x0"][b]))
            for k in range(k0, k1 + 1):
                s.add_linear_constraint(k, cone, G, c(g[b, k - k0]))
            s.L.oracle_ilqr_initialize(s.h)
            crc.set_guess(s, cfg, b, x, u)
            if rho != 1.0:
                s.set_penalty(1.0, rho)
                s.L.oracle_ilqr_penalty_update(s.h)
            crc.expand(s)
            bad += compare(cfg, got, crc.phases(s, crc.ALPHAS[b]), b, (rho, b), worst)
    print("measured maxima", {k: "%.1e" % v for k, v in worst.items()})
    assert (np.abs(u) > g[:, :, :1].repeat(4, axis=2)).any() and (np.abs(u) < g[:, :, :1].repeat(4, axis=2)).any()
    bt.close()
    assert not bad, bad


# ---- 5. closed loop --------------------------------------------------------------------------------------------------------------------
def test_closed_loop_mpc_with_a_bound_that_moves_with_the_horizon():
    nsim, batch, tol, N = 5, 6, 1e-4, M.N
    x_ref, u_ref = problems.bicycle_reference(N + nsim + 1)
    off = problems.uniform01((batch, 4), 33) - 0.5
    x0s = x_ref[0] + off * np.array([0.2, 0.2, 0.04, 0.0])
    cone, G, _ = M.steering_block()
    u0 = np.array([u_ref[0][0], 0.0])

    def bound(t):        # [batch][2] at absolute time step t: tightens as time goes on, differs from vehicle to vehicle
        return 0.02 * (2.0 - 1.5 * t / (N + nsim)) * (1.0 + 0.03 * np.arange(batch))[:, None] * np.ones((1, 2))

    def window(first):
        return np.stack([bound(first + k) for k in range(N + 1)], axis=1)

    def build(first, xs):
        bt = altro_amd.Batch(N, M.n, M.m, batch)
        bt.set_model(altro_amd.MODEL_BICYCLE, M.H)
        bt.set_tracking_cost(np.full((1, N + 1, M.n), M.QD), np.full((1, N, M.m), M.RD), x_ref[None, :N + 1], u_ref[None, :N], batch_stride_zero=True)
        bt.add_linear_constraint(0, N, cone, G, window(first), per_knot=True)
        if first:
            q, c = M.linear_costs(x_ref, first, u0)
            bt.update_linear_costs(q[None], None, c[None], 0, N, batch_stride_zero=True)
        bt.set_initial_state(xs)
        bt.set_input_guess(u0[None, None], k_stride_zero=True, batch_stride_zero=True)
        return bt
    solve = dict(iterations_max=80, use_backtracking=True, tol_primal_feasibility=tol, penalty_initial=1.0)
    bt, xs = build(0, x0s), x0s.copy()
    for it in range(nsim + 1):                                   # nsim steps: the solve after each is compared, nsim comparisons
        res = bt.ilqr_solve(**solve)
        assert (res["status"] == 0).all(), (it, res["status"])
        assert (res["feasibility"] <= tol).all(), (it, res["feasibility"])
        if it:                                                   # the handle built fresh for this step solved the same problem:
            assert_same(bt, fresh, 0, N, 2, [res, res_fresh], ("step", it))   # results, trajectory, duals, penalty
            fresh.close()
        if it == nsim:
            break
        _, u = bt.get_knot(0)
        xs = np.stack([M.plant(xs[b], u[b]) for b in range(batch)])
        q, c = M.linear_costs(x_ref, it + 1, u0)
        bt.update_linear_costs(q[None], None, c[None], 0, N, batch_stride_zero=True)
        bt.set_initial_state(xs)
        bt.shift_trajectory()
        bt.shift_duals(altro_amd.DUAL_TAIL_KEEP)
        bt.shift_constraint_rhs()
        bt.set_constraint_rhs(0, bound(it + 1 + N)[:, None, :], N, N)
        bt.set_penalty(1.0)
        # built fresh for this step: the full g, the same duals, penalty and guess
        fresh = build(it + 1, xs)
        want = window(it + 1)
        for k in range(N + 1):
            assert np.array_equal(bt.get_constraint_rhs(0, k), want[:, k]), (it, k)
            assert np.array_equal(fresh.get_constraint_rhs(0, k), want[:, k]), (it, k)
            fresh.set_duals(k, 0, bt.get_duals(k, 0, 2))
        fresh.set_penalty(1.0)
        fresh.set_input_guess(bt.get("u"))                        # the candidate inputs shift_trajectory moved: what the solve rolls out
        res_fresh = fresh.ilqr_solve(**solve)
    bt.close()


# ---- 6. the host description does not go stale ----------------------------------------------------------------------------------------
def test_rebuild_after_a_shift_keeps_the_shifted_values():
    """(A device-pointer write followed by a rebuild, with and without a shift in between: tests/cpp/constraint_rhs_test.cpp.)"""
    make, forms, k0, k1, cone, G, g, sweeps = twin_case("lane_one_launch")
    a = with_per_knot(make, k0, k1, cone, G, g)
    a.set_constraint_rhs(0, 0.9 * g[:, 2:5], 2, 4)                               # a host write, then a shift: the device is ahead of the host
    a.shift_constraint_rhs()
    g2 = g.copy(); g2[:, 2:5] *= 0.9; g2[:, :-1] = g2[:, 1:]
    Gt = np.zeros((1, M.n + M.m)); Gt[0, 2] = 1.0
    assert a.add_linear_constraint(NS, NS, INEQ, Gt, np.array([10.0])) == 1      # one more block: the tables are rebuilt
    for k in range(k0, k1 + 1):
        assert np.array_equal(a.get_constraint_rhs(0, k), g2[:, k - k0]), k
    assert np.array_equal(a.get_constraint_rhs(1, NS), np.array([10.0]))
    fresh = with_per_knot(make, k0, k1, cone, G, g2)
    fresh.add_linear_constraint(NS, NS, INEQ, Gt, np.array([10.0]))
    res = [bt.ilqr_solve(iterations_max=40, **OPTS) for bt in (a, fresh)]
    assert_same(a, fresh, k0, k1, 2, res, "after the rebuild")
    a.close(); fresh.close()


# ---- 7. device pointers ----------------------------------------------------------------------------------------------------------------
def test_device_pointer_mode_cpp():
    import os
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    rc, out, err = cpp_build.run("constraint_rhs_test", defines=["__HIP_PLATFORM_AMD__"],
                                 extra_link=["-isystem", os.path.join(rocm, "include"), "-Wno-attributes", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                                             "-Wl,-rpath," + os.path.join(rocm, "lib")])
    print(out)
    assert rc == 0 and out.strip().endswith("OK"), out + err


# ---- 8. errors and no-ops --------------------------------------------------------------------------------------------------------------
def test_errors_and_no_ops():
    rng = np.random.default_rng(3)
    bt, blocks, g = rhs_handle("lane", lambda j, shape: rng.normal(size=shape))
    E = altro_amd.AltroHipError
    G = rng.normal(size=(2, 6))
    assert bt.L.altro_hip_add_linear_constraint_rhs(bt.h, 0, 0, INEQ, 2, G.ctypes.data, g[1].ctypes.data, 4) == -2
    assert b"unknown right-hand side layout 4" in bt.L.altro_hip_last_error()
    for bad in (-1, len(blocks), 99):
        with pytest.raises(E, match=r"error -2: no constraint block with id %d" % bad):
            bt.set_constraint_rhs(bad, g[0])
        assert bt.L.altro_hip_get_constraint_rhs(bt.h, bad, 0, g[0].ctypes.data) == -2
    # block 2: knot points 33 .. 49
    for a, b in ((32, 40), (40, 50), (41, 40), (-1, 40), (33, -1), (0, 70)):
        with pytest.raises(E, match=r"error -2: knot point range \[%d, %d\] outside the range \[33, 49\] of constraint block 2" % (a, b)):
            bt.set_constraint_rhs(2, np.zeros((bt.batch, max(b - a + 1, 1), 1)), a, b)
    with pytest.raises(E, match=r"error -2: g is required"):
        bt.set_constraint_rhs(2, None)
    with pytest.raises(E, match=r"error -2: constraint block 6 has one right-hand side for its whole range \[69, 70\].*not \[69, 69\]"):
        bt.set_constraint_rhs(6, g[6], 69, 69)
    for k in (32, 50, -1, 71):
        with pytest.raises(E, match=r"error -2: knot point %d outside the range \[33, 49\] of constraint block 2" % k):
            bt.get_constraint_rhs(2, k)
    for value in (float("nan"), float("inf")):
        v = g[0].copy(); v[-1, -1, -1] = value
        with pytest.raises(E, match=r"error -2: g\[\d+\] = \S+ is not finite"):
            bt.set_constraint_rhs(0, v)
    check_all(bt, blocks, g, False, "after the errors")                          # nothing was written
    bt.close()
    f32, blocks32, g32 = rhs_handle("lane_f32", lambda j, shape: rng.normal(size=shape))
    v = g32[1].copy(); v[3, 1] = 1e39                                             # finite, but not as a float
    with pytest.raises(E, match=r"error -2: g\[7\] = 1e\+39 is not finite as a float"):
        f32.set_constraint_rhs(1, v)
    check_all(f32, blocks32, g32, True, "after the fp32 error")
    f32.close()
    # a block from source has no g: the setter and the getter say so, and its linear neighbour keeps its values
    from tests.test_gpu_generic_user_constraint import UN, Un, Um, make_unicycle
    un = make_unicycle(altro_amd.PLAN_LANE, 5)                                    # block 0: the disc from source, knot points 1 .. UN
    gl = rng.normal(size=(5, 11, 2))
    assert un.add_linear_constraint(0, 10, INEQ, rng.normal(size=(2, Un + Um)), gl, per_knot=True) == 1
    for k_range in ((None, None), (1, 1), (1, UN)):
        with pytest.raises(E, match=r"error -2: constraint block 0 comes from source: it has no right-hand side g"):
            un.set_constraint_rhs(0, np.zeros(1), *k_range)
    out = np.zeros(8)
    assert un.L.altro_hip_get_constraint_rhs(un.h, 0, 1, out.ctypes.data) == -2
    assert b"constraint block 0 comes from source: it has no right-hand side g" in un.L.altro_hip_last_error()
    for k in range(11):
        assert np.array_equal(un.get_constraint_rhs(1, k), gl[:, k]), k
    un.set_constraint_rhs(1, 2.0 * gl[:, 3:5], 3, 4)                               # (and still takes new ones)
    assert np.array_equal(un.get_constraint_rhs(1, 4), 2.0 * gl[:, 4]) and np.array_equal(un.get_constraint_rhs(1, 5), gl[:, 5])
    un.close()
    # the binding refuses an array of another shape than the block and range take, before the library reads past its end
    sh = altro_amd.Batch(6, 4, 2, 5)
    sh.add_linear_constraint(0, 5, INEQ, rng.normal(size=(2, 6)), rng.normal(size=(5, 6, 2)), per_knot=True)
    for bad, k_range in ((np.zeros((5, 2)), (1, 3)), (np.zeros((6, 2)), (None, None)), (np.zeros((5, 3, 2)), (1, 2))):
        with pytest.raises(AssertionError, match="g is "):
            sh.set_constraint_rhs(0, bad, *k_range)
    sh.close()
    # shift: nothing to do without per-knot blocks, and without blocks
    for plan, n, m in ((altro_amd.PLAN_AUTO, 4, 2), (altro_amd.PLAN_AUTO, 12, 4), (altro_amd.PLAN_GENERIC, 14, 9)):
        e = altro_amd.Batch(6, n, m, 5, plan=plan)
        assert e.L.altro_hip_shift_constraint_rhs(e.h) == 0
        old = rng.normal(size=(5, 2))
        e.add_linear_constraint(0, 5, INEQ, rng.normal(size=(2, n + m)), old)
        assert e.L.altro_hip_shift_constraint_rhs(e.h) == 0
        assert np.array_equal(e.get_constraint_rhs(0, 3), old)
        e.close()
    # per-knot-point dimensions: registration, writes and reads work; the shift is refused like shift_duals
    rg = altro_amd.Batch.with_dims([3, 3, 2], [1, 1], 4)
    gr = rng.normal(size=(4, 2, 2))
    assert rg.add_linear_constraint(0, 1, INEQ, np.ones((2, 4)), gr, per_knot=True) == 0
    assert np.array_equal(rg.get_constraint_rhs(0, 1), gr[:, 1])
    rg.set_constraint_rhs(0, 2.0 * gr[:, :1], 0, 0)
    assert np.array_equal(rg.get_constraint_rhs(0, 0), 2.0 * gr[:, 0]) and np.array_equal(rg.get_constraint_rhs(0, 1), gr[:, 1])
    with pytest.raises(E, match=r"error -3: altro_hip_shift_constraint_rhs needs uniform dimensions"):
        rg.shift_constraint_rhs()
    rg.close()
