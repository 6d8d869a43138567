"""The conic augmented-Lagrangian terms of every kernel family against the fp64 oracle, phase by phase, in EVERY region of every cone.

Each family has its own copy of the region comparisons (kernels/al_lane.hip soc_projection / soc_jacobian / soc_hessian for p <= 4,
shared by plans LANE and MFMA16 and the small cones of plan GENERIC; gen_al_rows and generic_expand_al_kernel in
kernels/ilqr_generic.hip for the many-row cone, lane per row with wave sums; the row-wise cones of kernels/ilqr_mfma16.hip,
ilqr_merit2_dpp.hip and ilqr_row32.hip), so a comparison between two device forms cannot see a mistake they share.  The cases are
tests/cone_region_cases.py's: a steered trajectory guess puts every (problem, knot point, block) into a scheduled class -- below,
inside, outside with s > 0 / < 0 / == 0, the apex, v == 0, the exact ties a == s and a == -s, orthant rows at val < 0, > 0, == 0 -- and
tests/test_cone_region_cases.py shows from the oracle alone that every class is reached and that a comparison flipped at a tie moves
the Hessian and the gains by more than 1e-3.

  a. zero duals, penalties 1 and 50: set_state_guess, set_input_guess, accept, reset_duals, expand, backward, merit(0), merit(alpha_b),
     feasibility, stationarity -- lx, lu, K, d, P, p (the Hessian's evidence), phi and phi' at both alphas, the candidate, feasibility
     and stationarity of EVERY problem and knot point;
  b. nonzero duals: a truncated ilqr_solve with rollout rounds (status, iterations and dual updates equal the oracle's, as do the
     duals of every block, knot point and problem and the penalty), then a guess steered from the ORACLE's duals and penalties into
     the three regions of every cone and both sides of the orthant rows, and the comparison of part a on it.

Tolerances: those of the project's phase-level comparisons with the oracle -- plans GENERIC / MFMA32: tests/test_gpu_ilqr_generic.py's
test_merit_expansion_stationarity_generic (lx, lu 1e-12, phi 1e-11, phi' 1e-9, candidates 1e-10, stationarity 1e-8); plans LANE / MFMA16:
tests/test_gpu_tile_model_slots.py's (lx, lu 1e-11, phi 1e-10, phi' 1e-8, x 2e-9, u 2e-8, stationarity 1e-7); K 1e-8 and feasibility
1e-7 on every plan.  d, P, p and the duals had no precedent: their worst relative error (to the block's largest entry, at least 1)
over all configurations, both parts, on an MI355X was d 2.8e-14, P 2.2e-15, p 3.1e-15, duals 1.5e-14 -- differences of summation order
(wave sums, tile products) -- and TOL_NEW holds them to 32 - 67 times that: d 1e-12, P 1e-13, p 1e-13, duals 1e-12.  The quantities
with a precedent measured lx 8.9e-14, lu 4.2e-14, K 1.9e-14, phi 8.1e-15, phi' 3.5e-12, x 3.1e-14, u 1.8e-13, feasibility 5.1e-15,
stationarity 5.0e-15.  Per-test time: 0.01 - 0.23 s.
"""
import numpy as np
import pytest

import altro_amd
from tests import cone_region_cases as crc
from tests.cone_region_cases import ALPHAS, BATCH, N, RHOS

pytestmark = pytest.mark.gpu

TOL = {"wave": dict(lx=1e-12, lu=1e-12, K=1e-8, phi=1e-11, dphi=1e-9, x=1e-10, u=1e-10, feas=1e-7, stat=1e-8),      # plans GENERIC, MFMA32
       "tile": dict(lx=1e-11, lu=1e-11, K=1e-8, phi=1e-10, dphi=1e-8, x=2e-9, u=2e-8, feas=1e-7, stat=1e-7)}        # plans LANE, MFMA16
TOL_NEW = dict(d=1e-12, P=1e-13, p=1e-13, duals=1e-12)
PLAN = {"LANE": altro_amd.PLAN_LANE, "MFMA16": altro_amd.PLAN_MFMA16, "GENERIC": altro_amd.PLAN_GENERIC, "MFMA32": altro_amd.PLAN_MFMA32}


def make_hip(cfg, dtype=altro_amd.F64, flags=0):
    n, m = cfg.n, cfg.m
    bt = altro_amd.Batch(cfg.N, n, m, BATCH, dtype=dtype, plan=altro_amd.PLAN_GENERIC if cfg.plan == "GENERIC" else altro_amd.PLAN_AUTO, flags=flags)
    bt.set_forms(altro_amd.FORM_ROLLOUT_ROUNDS)
    if cfg.dyn == "di":
        bt.set_model(altro_amd.MODEL_DOUBLE_INTEGRATOR, crc.H_DI)
        bt.set_tracking_cost(np.stack([cfg.Qd, cfg.Qd]), cfg.Rd[None], np.stack([cfg.xref, cfg.xref]), np.zeros((1, m)),
                             k_stride_zero=True, batch_stride_zero=True)
    else:
        p = cfg.p
        bt.set_dynamics(p["A"], p["B"], p["f"])
        if cfg.dense:
            bt.set_quadratic_cost(p["Q"], p["R"], p["H"], p["q"], p["r"], p["c"])
        else:
            bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
    bt.set_initial_state(cfg.x0)
    bt.set_input_guess(cfg.u_start)
    for bl in cfg.blocks:
        bt.add_linear_constraint(bl["k0"], bl["k1"], bl["cone"], bl["G"], bl["g"])
    assert bt.plan == PLAN[cfg.plan]
    if cfg.name == "auto32_rows":      # kernels/ilqr_row32.hip serves a handle of plan MFMA32 whose blocks are row-wise cones of <= 32 rows
        assert all(bl["kind"] != "soc" and bl["p"] <= 32 for bl in cfg.blocks)
    return bt


def hip_phases(bt, x, u, rho=None):
    """The handle's side of cone_region_cases.phases for the whole batch; rho None: the duals and penalties stay."""
    bt.set_state_guess(x); bt.set_input_guess(u)
    bt.accept()
    if rho is not None:
        bt.reset_duals(rho)
    bt.expand()
    _, _, lx, lu = bt.get_expansion()
    bt.backward()
    assert (bt.get("status") == -1).all()
    r = dict(lx=lx, lu=lu, K=bt.get("K"), d=bt.get("d"), P=bt.get("P"), p=bt.get("p"))
    r["phi0"], r["dphi0"] = bt.merit(np.zeros(BATCH))
    r["phi"], r["dphi"] = bt.merit(ALPHAS)
    r["x"], r["u"] = bt.get("x"), bt.get("u")
    r["feas"] = bt.feasibility()
    r["stat"] = bt.stationarity()
    return r


def compare(cfg, got, ref, b, tag, worst):
    """Problem b of `got` (the batch) against the oracle's `ref`; every knot point, no filter.  Errors are noted before they are judged."""
    tol = TOL["wave" if cfg.plan in ("GENERIC", "MFMA32") else "tile"]
    bad = []

    def note(key, err, bound):
        worst[key] = max(worst.get(key, 0.0), float(err))
        if not err <= bound:
            bad.append((key, tag, float(err), bound))

    def mixed(a, want):          # assert_allclose's measure with rtol == atol: |a - want| / (1 + |want|), elementwise
        return float((np.abs(a - want) / (1.0 + np.abs(want))).max())

    def scaled(a, want):         # relative to the largest entry (at least 1)
        return float(np.abs(a - want).max() / max(1.0, np.abs(want).max()))

    for key in ("lx", "lu", "x", "u"):
        note(key, mixed(got[key][b], ref[key]), tol[key])
    note("K", scaled(got["K"][b], ref["K"]), tol["K"])
    for key in ("d", "P", "p"):
        note(key, scaled(got[key][b], ref[key]), TOL_NEW[key])
    for key, t in (("phi0", "phi"), ("dphi0", "dphi"), ("phi", "phi"), ("dphi", "dphi"), ("feas", "feas"), ("stat", "stat")):
        note(key, abs(got[key][b] - ref[key]) / max(1.0, abs(ref[key])), tol[t])
    return bad


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_zero_duals_every_region(name):
    """Part a (the measured maxima are printed; the module docstring and DESIGN.md section 2 hold the worst of them)."""
    cfg = crc.config(name)
    ref = crc.zero_dual_reference(name)
    bt = make_hip(cfg)
    worst, bad = {}, []
    for rho in RHOS:
        got = hip_phases(bt, cfg.x, cfg.u, rho)
        for b in range(BATCH):
            bad += compare(cfg, got, ref[(rho, b)], b, (rho, b), worst)
    print("measured maxima", name, {k: "%.1e" % v for k, v in worst.items()})
    bt.close()
    assert not bad, bad


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_nonzero_duals_after_a_truncated_solve(name):
    """Part b."""
    cfg = crc.config(name)
    ref = crc.nonzero_dual_reference(name)
    for b in range(BATCH):       # (what tests/test_cone_region_cases.py shows at length)
        assert ref["dual_updates"][b] >= 1 and (ref["log"][b][:, 5] < 8).all() and (ref["log"][b][:, 0] >= 1e-2).all()
    bt = make_hip(cfg)
    res = bt.ilqr_solve(iterations_max=crc.SOLVE_SWEEPS[name], forms=altro_amd.FORM_ROLLOUT_ROUNDS, penalty_initial=1.0, penalty_scaling=10.0)
    for key in ("status", "iterations", "dual_updates"):
        assert np.array_equal(res[key], np.array(ref[key])), (key, res[key], ref[key])
    worst, bad = {}, []
    for k in range(N + 1):
        for slot, j in enumerate(cfg.at(k)):
            z = bt.get_duals(k, slot, cfg.blocks[j]["p"])
            for b in range(BATCH):
                want = ref["duals"][(j, b, k)]
                err = float(np.abs(z[b] - want).max() / max(1.0, np.abs(want).max()))
                worst["duals"] = max(worst.get("duals", 0.0), err)
                if not err <= TOL_NEW["duals"]:
                    bad.append(("duals", cfg.blocks[j]["name"], b, k, err))
    for b in range(BATCH):
        assert res["penalty"][b] == max(ref["rhos"][(j, b, k)] for k in range(N + 1) for j in cfg.at(k)), (b, res["penalty"][b])
    got = hip_phases(bt, ref["x"], ref["u"])
    for b in range(BATCH):
        bad += compare(cfg, got, ref["phases"][b], b, ("solved", b), worst)
    print("measured maxima", name, {k: "%.1e" % v for k, v in worst.items()})
    bt.close()
    assert not bad, bad
