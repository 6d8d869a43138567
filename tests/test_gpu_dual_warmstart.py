"""Warm-started duals for receding-horizon MPC: altro_hip_set_duals / _get_penalty / _set_penalty / _shift_duals on every plan.

  1. round trips: what set_duals / set_penalty store is what get_duals / get_penalty return, exactly (fp32: the value as a float);
  2. set_duals against the oracle: the oracle's duals and penalties after a truncated solve (tests/cone_region_cases.py's
     nonzero_dual_reference), given to a FRESH handle through set_duals / set_penalty, with the call sequence and tolerances of
     tests/test_gpu_cone_regions.py for the same phases;
  3. shift_duals against numpy, bit for bit, over the block layouts of tests/cpp/al_shift_test.cpp;
  4. a solve consumes what was set: duals and penalty read, reset and restored give the solve of a twin handle that simply went on;
  5. five closed-loop MPC steps of the bicycle batch with shifted duals (sweeps and dual updates printed next to the reset_duals loop);
  6. errors and no-ops.
Shapes: LANE (4, 2), N = 10, batch 66 (two waves, the last one partial), fp64 and fp32; the (12, 4) tile N = 12, batch 8, with an 8-row
and a 24-row block; MFMA32 (13, 4); GENERIC (14, 9) created explicitly.
"""
import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import cone_region_cases as crc
from tests import mpc_common as M
from tests import problems
from tests.test_gpu_cone_regions import compare, make_hip as make_cone_hip

pytestmark = pytest.mark.gpu

EQ, INEQ, SOC = oracle.CONE_EQUALITY, oracle.CONE_INEQUALITY, oracle.CONE_SOC
# (plan, n, m, N, batch, dtype, has the 24-row block)
SHAPES = {"lane": (altro_amd.PLAN_LANE, 4, 2, 10, 66, altro_amd.F64, False),
          "lane_f32": (altro_amd.PLAN_LANE, 4, 2, 10, 66, altro_amd.F32, False),
          "tile": (altro_amd.PLAN_MFMA16, 12, 4, 12, 8, altro_amd.F64, True),
          "mfma32": (altro_amd.PLAN_MFMA32, 13, 4, 10, 9, altro_amd.F64, True),
          "generic": (altro_amd.PLAN_GENERIC, 14, 9, 10, 9, altro_amd.F64, True),
          "generic_f32": (altro_amd.PLAN_GENERIC, 14, 9, 10, 9, altro_amd.F32, True)}


def layout(N, wide):
    """(k_first, k_last, cone, p) in registration order: a running block on 0 .. N-1 (with `wide` a 24-row block -- three slots on the
    tile -- and an 8-row one), a partial range 3 .. 7, a range reaching the terminal knot point, a terminal-only block, a second-order cone;
    two blocks or more at every knot point, at most two where `wide` is off (plan LANE's capacity)."""
    run = [(0, N - 1, INEQ, 24), (0, N - 1, INEQ, 8)] if wide else [(0, N - 1, INEQ, 4)]
    return run + [(3, 7, INEQ, 2), (N - 2, N, EQ, 1), (N, N, EQ, 3), (0, 2, SOC, 3)]


def bare_handle(name):
    """A handle with the layout's blocks and nothing else: the dual calls need no dynamics and no cost."""
    plan, n, m, N, batch, dtype, wide = SHAPES[name]
    bt = altro_amd.Batch(N, n, m, batch, dtype=dtype, plan=altro_amd.PLAN_GENERIC if plan == altro_amd.PLAN_GENERIC else altro_amd.PLAN_AUTO)
    assert bt.plan == plan, (name, bt.plan)
    blocks = layout(N, wide)
    rng = np.random.default_rng(5)
    for j, (k0, k1, cone, p) in enumerate(blocks):
        assert bt.add_linear_constraint(k0, k1, cone, rng.normal(size=(p, n + m)), np.zeros(p)) == j
    return bt, blocks


def at(blocks, k):
    return [j for j, (k0, k1, _, _) in enumerate(blocks) if k0 <= k <= k1]


def fill(blocks, N, batch):
    """{(definition, k): [batch][p]} of integers distinct per (definition, k, row, problem), all below 2^24 (exact as floats)."""
    z = {}
    for j, (k0, k1, _, p) in enumerate(blocks):
        for k in range(k0, k1 + 1):
            z[(j, k)] = (((k * 8 + j) * 32 + np.arange(p)[None, :]) * 128 + np.arange(batch)[:, None] + 1).astype(np.float64)
    assert max(v.max() for v in z.values()) < 2 ** 24 and len({float(e) for v in z.values() for e in v.ravel()}) == sum(v.size for v in z.values())
    return z


def put(bt, blocks, z):
    for k in range(bt.N + 1):
        for slot, j in enumerate(at(blocks, k)):
            bt.set_duals(k, slot, z[(j, k)])


def fetch(bt, blocks):
    return {(j, k): bt.get_duals(k, slot, blocks[j][3]) for k in range(bt.N + 1) for slot, j in enumerate(at(blocks, k))}


# ---- 1. round trips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_round_trip(name):
    bt, blocks = bare_handle(name)
    batch, f32 = bt.batch, SHAPES[name][5] == altro_amd.F32
    rng = np.random.default_rng(11)
    z = {key: rng.normal(size=v.shape) for key, v in fill(blocks, bt.N, batch).items()}      # (all 53 bits: fp32 rounds them)
    put(bt, blocks, z)
    got = fetch(bt, blocks)
    for key, v in z.items():
        want = v.astype(np.float32).astype(np.float64) if f32 else v
        assert np.array_equal(got[key], want), (name, key)
    assert np.array_equal(bt.get_penalty(), np.ones(batch))                                  # what a fresh handle carries
    rho = 1.0 + 100.0 * rng.uniform(size=batch)
    bt.set_penalty(rho)
    assert np.array_equal(bt.get_penalty(), rho)
    after = fetch(bt, blocks)
    assert all(np.array_equal(after[key], got[key]) for key in got)                          # duals bit-unchanged by set_penalty
    bt.set_penalty(37.5)
    assert np.array_equal(bt.get_penalty(), np.full(batch, 37.5))
    after = fetch(bt, blocks)
    assert all(np.array_equal(after[key], got[key]) for key in got)
    bt.close()


# ---- 2. set_duals against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lane_4_2", "tile_tracking", "auto32_rows", "auto32_cones"])
def test_set_duals_against_the_oracle(name):
    """The oracle after a truncated solve (rollouts, dual updates, penalty updates, refreshed expansions: nonzero duals, raised
    penalties), its duals and penalties read with oracle_ilqr_get_duals / _get_penalty; a fresh handle given the same trajectory, duals
    and penalty must produce the oracle's phases (tests/test_gpu_cone_regions.py: hip_phases' calls, compare's tolerances)."""
    cfg = crc.config(name)
    ref = crc.nonzero_dual_reference(name)
    B, N = crc.BATCH, crc.N
    bt = make_cone_hip(cfg)
    bt.set_state_guess(ref["x"]); bt.set_input_guess(ref["u"])
    bt.accept()
    partly_zero = False
    for k in range(N + 1):
        for slot, j in enumerate(cfg.at(k)):
            z = np.stack([ref["duals"][(j, b, k)] for b in range(B)])
            if cfg.blocks[j]["kind"] == "orth":
                partly_zero = partly_zero or any((z[b] == 0.0).any() and (z[b] != 0.0).any() for b in range(B))
            bt.set_duals(k, slot, z)
    rho = np.zeros(B)
    for b in range(B):
        rhos = {ref["rhos"][(j, b, k)] for k in range(N + 1) for j in cfg.at(k)}
        assert len(rhos) == 1 and max(rhos) > 1.0, (b, rhos)          # one penalty per problem, raised by the oracle's penalty updates
        rho[b] = max(rhos)
    bt.set_penalty(rho)
    if name in ("lane_4_2", "auto32_rows"):                           # the configurations with a dense orthant block
        assert partly_zero, "no orthant block with its duals partly zero"
    bt.expand()
    _, _, lx, lu = bt.get_expansion()
    bt.backward()
    assert (bt.get("status") == -1).all()
    got = dict(lx=lx, lu=lu, K=bt.get("K"), d=bt.get("d"), P=bt.get("P"), p=bt.get("p"))
    got["phi0"], got["dphi0"] = bt.merit(np.zeros(B))
    got["phi"], got["dphi"] = bt.merit(crc.ALPHAS)
    got["x"], got["u"] = bt.get("x"), bt.get("u")
    got["feas"] = bt.feasibility()
    got["stat"] = bt.stationarity()
    worst, bad = {}, []
    for b in range(B):
        bad += compare(cfg, got, ref["phases"][b], b, ("set", b), worst)
    print("measured maxima", name, {k: "%.1e" % v for k, v in worst.items()})
    assert np.array_equal(bt.get_penalty(), rho)
    bt.close()
    assert not bad, bad


# ---- 3. shift_duals against numpy ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [altro_amd.DUAL_TAIL_KEEP, altro_amd.DUAL_TAIL_ZERO])
@pytest.mark.parametrize("name", list(SHAPES))
def test_shift_duals_against_numpy(name, tail):
    bt, blocks = bare_handle(name)
    z = fill(blocks, bt.N, bt.batch)
    put(bt, blocks, z)
    bt.shift_duals(tail)
    got = fetch(bt, blocks)
    for j, (k0, k1, _, p) in enumerate(blocks):
        for k in range(k0, k1 + 1):
            want = z[(j, k + 1)] if k < k1 else (z[(j, k)] if tail == altro_amd.DUAL_TAIL_KEEP else np.zeros_like(z[(j, k)]))
            assert np.array_equal(got[(j, k)], want), (name, tail, j, k)
    bt.shift_duals(tail)                                              # and once more from the shifted state
    got2 = fetch(bt, blocks)
    for j, (k0, k1, _, p) in enumerate(blocks):
        for k in range(k0, k1 + 1):
            want = got[(j, k + 1)] if k < k1 else (got[(j, k)] if tail == altro_amd.DUAL_TAIL_KEEP else np.zeros_like(z[(j, k)]))
            assert np.array_equal(got2[(j, k)], want), (name, tail, j, k, "second shift")
    bt.close()


def test_shift_duals_long_chains():
    """Chains longer than the kernel's group of links in flight, and of every length modulo it: a running block over N = 70 and
    ranges ending everywhere."""
    N, n, m, batch = 70, 4, 2, 70
    bt = altro_amd.Batch(N, n, m, batch, plan=altro_amd.PLAN_GENERIC)
    blocks = [(0, N - 1, INEQ, 3)] + [(0, k1, EQ, 1) for k1 in (14, 15, 16, 17, 31, 32, 33)]
    for j, (k0, k1, cone, p) in enumerate(blocks):
        assert bt.add_linear_constraint(k0, k1, cone, np.ones((p, n + m)), np.zeros(p)) == j
    z = fill(blocks, N, batch)
    for tail in (altro_amd.DUAL_TAIL_KEEP, altro_amd.DUAL_TAIL_ZERO):
        put(bt, blocks, z)
        bt.shift_duals(tail)
        got = fetch(bt, blocks)
        for j, (k0, k1, _, p) in enumerate(blocks):
            for k in range(k0, k1 + 1):
                want = z[(j, k + 1)] if k < k1 else (z[(j, k)] if tail == altro_amd.DUAL_TAIL_KEEP else np.zeros_like(z[(j, k)]))
                assert np.array_equal(got[(j, k)], want), (tail, j, k)
    bt.close()


# ---- 4. a solve consumes what was set ------------------------------------------------------------------------------------------------
STEER_MAX = 0.02      # half the reference path's steering angle at the end of the horizon: the bound is active


def bicycle_handle(batch, x_ref, u_ref, x0s):
    bt = altro_amd.Batch(M.N, M.n, M.m, batch)
    assert bt.plan == altro_amd.PLAN_LANE
    bt.set_model(altro_amd.MODEL_BICYCLE, M.H)
    Qd = np.full((1, M.N + 1, M.n), M.QD); Rd = np.full((1, M.N, M.m), M.RD)
    bt.set_tracking_cost(Qd, Rd, x_ref[None, :M.N + 1], u_ref[None, :M.N], batch_stride_zero=True)
    cone, G, _ = M.steering_block()
    bt.add_linear_constraint(0, M.N, cone, G, np.full(2, STEER_MAX))
    bt.set_initial_state(x0s)
    u0 = np.array([u_ref[0][0], 0.0])
    bt.set_input_guess(u0[None, None], k_stride_zero=True, batch_stride_zero=True)
    return bt, u0


def bicycle_pair(batch):
    x_ref, u_ref = problems.bicycle_reference(M.N + 8)
    off = problems.uniform01((batch, 4), 33) - 0.5
    x0s = x_ref[0] + off * np.array([0.2, 0.2, 0.04, 0.0])
    return [bicycle_handle(batch, x_ref, u_ref, x0s)[0] for _ in range(2)], [(0, M.N, None, 2)]


def tile_pair(batch):
    N = 12
    p = problems.ilqr12x4_problem(batch, N, True)
    k0, k1, cone, G, g = problems.ilqr12x4_constraint_blocks(N)[0]              # |u| <= 0.3 at every k < N
    pair = []
    for _ in range(2):
        bt = altro_amd.Batch(N, 12, 4, batch)
        assert bt.plan == altro_amd.PLAN_MFMA16
        bt.set_dynamics(p["A"], p["B"], p["f"])
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.set_initial_state(p["x0"])
        bt.set_input_guess(p["u0"])
        bt.add_linear_constraint(k0, k1, cone, G, g)
        pair.append(bt)
    return pair, [(k0, k1, None, 8)]


@pytest.mark.parametrize("case", ["lane_one_launch", "lane_sequenced", "tile"])
def test_a_solve_consumes_what_was_set(case):
    (a, twin), blocks = tile_pair(8) if case == "tile" else bicycle_pair(66)
    opts = dict(use_backtracking=True, penalty_initial=1.0, penalty_scaling=10.0, forms=altro_amd.FORM_SEQUENCED if case == "lane_sequenced" else 0)
    # truncated where the oracle's solve of these problems has updated the duals and has not converged (bicycle: 2 sweeps, 1 update;
    # the tile's input box: 6 sweeps)
    first = [bt.ilqr_solve(iterations_max=6 if case == "tile" else 2, **opts) for bt in (a, twin)]
    for key in ("status", "iterations", "dual_updates", "penalty"):
        assert np.array_equal(first[0][key], first[1][key]), key
    print(case, "first solve: status", first[0]["status"].tolist(), "dual updates", first[0]["dual_updates"].tolist())
    z, rho = fetch(a, blocks), a.get_penalty()
    assert any((v != 0.0).any() for v in z.values()) and (rho > 1.0).any(), "the first solve left no duals to restore"
    assert np.array_equal(rho, first[0]["penalty"])
    _, u = a.get_nominal()
    a.reset_duals(1.0)
    assert all((v == 0.0).all() for v in fetch(a, blocks).values()) and (a.get_penalty() == 1.0).all()
    put(a, blocks, z)
    a.set_penalty(rho)
    for bt in (a, twin):                                                        # the same guess on both: the second solve's rollout starts from it
        bt.set_input_guess(u)
    second = [bt.ilqr_solve(iterations_max=40, **opts) for bt in (a, twin)]
    print(case, "second solve: iterations", second[1]["iterations"].tolist(), "dual updates", second[1]["dual_updates"].tolist())
    for key in ("status", "iterations", "dual_updates", "penalty"):
        assert np.array_equal(second[0][key], second[1][key]), (key, second[0][key], second[1][key])
    for got, want in zip(a.get_nominal(), twin.get_nominal()):
        assert np.array_equal(got, want)
    za, zt = fetch(a, blocks), fetch(twin, blocks)
    assert all(np.array_equal(za[key], zt[key]) for key in zt)
    a.close(); twin.close()


# ---- 5. closed-loop MPC with shifted duals -------------------------------------------------------------------------------------------
def test_closed_loop_mpc_with_shifted_duals():
    nsim, batch, tol = 5, 6, 1e-4
    x_ref, u_ref = problems.bicycle_reference(M.N + nsim + 1)
    off = problems.uniform01((batch, 4), 33) - 0.5
    x0s = x_ref[0] + off * np.array([0.2, 0.2, 0.04, 0.0])
    totals = {}
    for mode in ("warm", "reset"):
        bt, u0 = bicycle_handle(batch, x_ref, u_ref, x0s)
        xs, sweeps, updates = x0s.copy(), 0, 0
        for it in range(nsim):
            res = bt.ilqr_solve(iterations_max=80, use_backtracking=True, tol_primal_feasibility=tol, penalty_initial=1.0)
            assert (res["status"] == 0).all(), (mode, it, res["status"])
            assert (res["feasibility"] <= tol).all(), (mode, it, res["feasibility"])
            sweeps += res["sweeps"]; updates += int(res["dual_updates"].sum())
            _, u = bt.get_knot(0)
            xs = np.stack([M.plant(xs[b], u[b]) for b in range(batch)])
            q, c = M.linear_costs(x_ref, it + 1, u0)
            bt.update_linear_costs(q[None], None, c[None], 0, M.N, batch_stride_zero=True)
            bt.set_initial_state(xs)
            bt.shift_trajectory()
            if mode == "warm":
                bt.shift_duals(altro_amd.DUAL_TAIL_KEEP)
                bt.set_penalty(1.0)
            else:
                bt.reset_duals(1.0)
        totals[mode] = (sweeps, updates)
        bt.close()
    print("closed-loop MPC, %d steps x %d vehicles: sweeps / dual updates  shift_duals + set_penalty %s   reset_duals %s" % (nsim, batch, totals["warm"], totals["reset"]))


# ---- 6. errors and no-ops --------------------------------------------------------------------------------------------------------------
def test_errors_and_no_ops():
    bt, blocks = bare_handle("lane")
    z = np.zeros((bt.batch, 4))
    for k, slot in ((-1, 0), (bt.N + 1, 0), (0, 2), (0, -1), (bt.N, 2)):
        with pytest.raises(altro_amd.AltroHipError, match=r"error -2: no constraint block %d at knot point %d" % (slot, k)):
            bt.set_duals(k, slot, z)
    with pytest.raises(altro_amd.AltroHipError, match=r"error -2: no constraint block 0 at knot point 0"):
        bt.set_duals(0, 0, None)
    before = bt.get_penalty()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(altro_amd.AltroHipError, match=r"error -2: penalty must be positive"):
            bt.set_penalty(bad)
        rho = np.full(bt.batch, 2.0); rho[-1] = bad
        with pytest.raises(altro_amd.AltroHipError, match=r"error -2: penalty must be positive \(problem %d\)" % (bt.batch - 1)):
            bt.set_penalty(rho)
    assert np.array_equal(bt.get_penalty(), before)                   # nothing was written
    assert bt.L.altro_hip_set_penalty(bt.h, None, 1) == -2 and bt.L.altro_hip_get_penalty(bt.h, None) == -2
    for tail in (-1, 2):
        with pytest.raises(altro_amd.AltroHipError, match=r"error -2: unknown tail %d" % tail):
            bt.shift_duals(tail)
    bt.close()
    # per-knot-point dimensions: like shift_trajectory
    rg = altro_amd.Batch.with_dims([3, 3, 2], [1, 1], 4)
    rg.add_linear_constraint(0, 1, INEQ, np.ones((2, 4)), np.zeros(2))
    with pytest.raises(altro_amd.AltroHipError, match=r"error -3: altro_hip_shift_duals needs uniform dimensions"):
        rg.shift_duals()
    rg.set_duals(0, 0, np.full((4, 2), 0.5))                          # (the setters take such a handle)
    assert np.array_equal(rg.get_duals(0, 0, 2), np.full((4, 2), 0.5))
    rg.close()
    # no blocks: nothing to shift
    for plan, n, m in ((altro_amd.PLAN_AUTO, 4, 2), (altro_amd.PLAN_AUTO, 12, 4), (altro_amd.PLAN_GENERIC, 14, 9)):
        e = altro_amd.Batch(6, n, m, 5, plan=plan)
        assert e.L.altro_hip_shift_duals(e.h, altro_amd.DUAL_TAIL_KEEP) == 0 and e.L.altro_hip_shift_duals(e.h, altro_amd.DUAL_TAIL_ZERO) == 0
        with pytest.raises(altro_amd.AltroHipError, match=r"error -2: unknown tail 7"):
            e.shift_duals(7)
        e.set_penalty(3.0)
        assert np.array_equal(e.get_penalty(), np.full(5, 3.0))
        e.close()
