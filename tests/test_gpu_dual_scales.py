"""Nonzero duals, the dual update and the penalty update judged without the floor of 1 and at every scale, through the C ABI
(tests/loop_scale_cases.py holds the states, the transforms and the metric; tests/test_loop_scale_cases.py shows them on the oracle
alone).  Needs an MI355X; reads the fixtures tests/golden/loop_phases_duals_<config>.npz, no oracle library, no mpmath.

A state -- duals per (knot point, slot) through set_duals, one penalty per problem through set_penalty, a guess -- replaces
reset_duals in the call sequence of tests/test_gpu_loop_scales.py.  S1: the oracle's duals and raised penalties after a truncated
solve with a guess that puts every cone below, inside and outside.  S2: the same duals (the cones' last rows steered) before a dual
update at the rollout of S1's inputs, every region of every block reached.  The update is a FROZEN solve: tol_meritfun_gradient huge
takes alpha = 0, tol_stationarity = 4^200 forces the outer update, tol_primal_feasibility 0 / huge turns the penalty update on / off.

  A1  phases at S1 are covariant: back(device(T cfg, T S1)) == device(cfg, S1) bit for bit, every variant of test_gpu_loop_scales.py,
      fp32 handles at k = +-8.
  B1  phases at S1 are accurate: criterion B, blockerr <= 10 max(e_cpu, 1e-13), against the extended-precision fixture.
  A2  the update is covariant on every route that performs it (ROUTES): status, iterations, dual_updates, alpha = 0, the nominal
      trajectory equal to the rollout, duals and penalty mapped back bit-identical; with the penalty update, without it, with its clamp
      (penalty_initial = penalty_max / 2 -- a solve gives EVERY problem penalty_initial, so the clamp is a run of its own, not one
      problem of a run) and over two sweeps (the second sweep's K, d, P, p too); fp32 handles at k = +-8.
  B2  the update is accurate: z+ per kind of block, the second sweep's K, d, P, p and z++ by criterion B; rho+ by equality.
  A3  one sweep with a real line search, both searches, from loop_scale_cases.search_state: covariant on the problems of the
      fixture's mask (the oracle accepts alpha = 1 in every unit system); the others run and are printed.
  S   the state a frozen two-sweep solve leaves, written to a fresh handle through set_duals / set_penalty, gives the phases of the
      handle that carried it, bit for bit.

Measured on an MI355X.  A1, A2, A3 (on the mask), S: bit-identical everywhere, nothing had to be fixed.  On fp32 handles of the tile and
of plan GENERIC the candidate of alpha = 0 restarts from rounded states, so "u unchanged" is asserted on fp64 handles only; plan LANE's
rollout is not the oracle's bit for bit, so the nominal trajectory is compared with the handle's own rollout.  A3 outside the mask
(lane_6_3 problem 6, auto32_rows problem 3): alpha 0.5 at k = -20 against 0.357 / 0.396, as on the oracle.
B, e_gpu / max(e_cpu, 1e-13) (10 is the limit, no entry of MARGINS was needed), phases at S1 | z+ | z++ | second sweep K, d, P, p:
  plan LANE     0.13 (u of (4, 2)) | cones 0.42 on (6, 3), 0.0061 on (4, 2), orthant 0.0091 | 0.13 | 0.066      (fused = sequenced)
  plan MFMA16   0.23 (phi'(alpha_b), dense cost; else <= 0.048) | cones 1.6 dense cost (2.2e-13 against the oracle's 1.4e-13), 0.039
                tracking, orthant 0.0052 | 0.072 | 0.014      (identical under EXPAND_DUAL, FORM_EXPAND_LDS, FORM_ALROWS_LDS and both)
  plan GENERIC  0.044, 0.075 with GENERIC_MATRIX_CORES | 0.0056 | 0.0066 | 0.011
  plan MFMA32   cones 0.41 (phi'(alpha_b); else <= 0.059) | 0.0065 | 0.011 | 0.0097;  rows, also under FORM_GENERIC_MERIT_LDS: 0.21 |
                orthant 0.006, the equality block bit-identical | 0.0068 | 0.051
rho+ equal in every run, the clamp included.  Per-test time 0.01 - 0.52 s, the 84 tests together 8 s.
"""
import numpy as np
import pytest

import altro_amd
from tests import cone_region_cases as crc
from tests import loop_scale_cases as lsc
from tests import test_gpu_cone_regions as regions
from tests.cone_region_cases import ALPHAS, BATCH, N
from tests.test_gpu_loop_scales import ROUNDS, VARIANTS

pytestmark = pytest.mark.gpu

F32_TILE_BLOCKS = ("cone4", "box", "cone4_N", "cone3_N")
# id -> (configuration, forms, handle flags): every route that performs the dual update (csrc/loop_route.h, SolveRun::outer_update)
ROUTES = {
    "lane_4_2": ("lane_4_2", 0, 0),                                           # the one-launch solve's own copy of the update
    "lane_6_3": ("lane_6_3", 0, 0),
    "lane_4_2-sequenced": ("lane_4_2", altro_amd.FORM_SEQUENCED, 0),          # ilqr_dual_update_kernel
    "lane_6_3-sequenced": ("lane_6_3", altro_amd.FORM_SEQUENCED, 0),
    "tile_tracking": ("tile_tracking", 0, 0),                                 # EXPAND_DUAL of ilqr_merit2_dpp.hip
    "tile_dense": ("tile_dense", 0, 0),
    "tile_tracking-expand_lds": ("tile_tracking", altro_amd.FORM_EXPAND_LDS, 0),      # wave_dual_update_dpp_kernel
    "tile_dense-expand_lds": ("tile_dense", altro_amd.FORM_EXPAND_LDS, 0),
    "tile_tracking-alrows_lds": ("tile_tracking", altro_amd.FORM_ALROWS_LDS, 0),      # wave_dual_update_kernel
    "tile_dense-alrows_lds": ("tile_dense", altro_amd.FORM_ALROWS_LDS, 0),
    "tile_tracking-both_lds": ("tile_tracking", altro_amd.FORM_EXPAND_LDS | altro_amd.FORM_ALROWS_LDS, 0),
    "generic_14_5": ("generic_14_5", 0, 0),                                   # generic_dual_update_kernel
    "generic_14_5-matrix_cores": ("generic_14_5", 0, altro_amd.GENERIC_MATRIX_CORES),
    "auto32_cones": ("auto32_cones", 0, 0),
    "auto32_rows": ("auto32_rows", 0, 0),
    "auto32_rows-generic_merit_lds": ("auto32_rows", altro_amd.FORM_GENERIC_MERIT_LDS, 0),
}
# the frozen solves: (feasible, sweeps, penalty_initial)
UPDATES = {"infeasible": (False, 1, lsc.RHO0), "feasible": (True, 1, lsc.RHO0), "two sweeps": (False, 2, lsc.RHO0), "clamp": (False, 1, lsc.RHO_CLAMP)}
# (test, variant, quantity) -> a margin of up to 100 with its CPU explanation in DESIGN section 2.  None is needed.
MARGINS = {}


def put_state(bt, cfg, st):
    for k in range(N + 1):
        for slot, j in enumerate(cfg.at(k)):
            bl = cfg.blocks[j]
            bt.set_duals(k, slot, st["z"][bl["name"]][:, k - bl["k0"]])
    bt.set_penalty(st["rho"])


def get_duals(bt, cfg):
    return {bl["name"]: np.stack([bt.get_duals(k, cfg.at(k).index(j), bl["p"]) for k in range(bl["k0"], bl["k1"] + 1)], axis=1)
            for j, bl in enumerate(cfg.blocks)}


def phases_of(bt):
    """hip_phases' calls from expand on: the handle's trajectory, duals and penalty as they are."""
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


def device_phases(cfg, st, forms=0, flags=0, dtype=altro_amd.F64):
    """The phases of `cfg` (a configuration or a transformed one) at state `st`, in ITS units."""
    bt = regions.make_hip(cfg, dtype=dtype, flags=flags)
    bt.set_forms(ROUNDS | forms)
    bt.set_state_guess(st["x"]); bt.set_input_guess(st["u"])
    bt.accept()
    put_state(bt, cfg, st)
    out = phases_of(bt)
    bt.close()
    return out


def device_update(cfg, st, feasible, sweeps, rho0=lsc.RHO0, tolg=lsc.HUGE, backtracking=False, forms=0, flags=0, dtype=altro_amd.F64, keep=False):
    """loop_scale_cases.oracle_update on the device: the solve from state `st` in the units of `cfg`.  alpha: the last sweep's."""
    bt = regions.make_hip(cfg, dtype=dtype, flags=flags)
    bt.set_forms(ROUNDS | forms)
    bt.set_input_guess(st["u"])
    put_state(bt, cfg, st)
    res = bt.ilqr_solve(iterations_max=sweeps, use_backtracking=backtracking, forms=ROUNDS | forms, **lsc.solve_options(cfg, feasible, rho0, tolg))
    x, u = bt.get_nominal()
    out = dict(z=get_duals(bt, cfg), rho=bt.get_penalty(), alpha=res["alpha"], status=res["status"], iterations=res["iterations"], x=x, u=u,
               K=bt.get("K"), d=bt.get("d"), P=bt.get("P"), p=bt.get("p"))
    assert np.array_equal(out["rho"], res["penalty"])
    if keep:
        return out, res, bt
    bt.close()
    return out, res


def device_rollout(cfg, st, forms=0, flags=0, dtype=altro_amd.F64):
    bt = regions.make_hip(cfg, dtype=dtype, flags=flags)
    bt.set_forms(ROUNDS | forms)
    bt.set_input_guess(st["u"])
    bt.open_loop_rollout()
    x = bt.get("x")
    bt.close()
    return x


def cases(name, dtype=altro_amd.F64, blocks=None):
    """(configuration, [(T, transformed configuration)]) with the subset of blocks an fp32 handle of the tile takes."""
    cfg = crc.config(name) if blocks is None else lsc.subset(crc.config(name), blocks)
    return cfg, [(T, lsc.transform(cfg, *T)) for T in lsc.transforms(name, fp32=dtype == altro_amd.F32)]


def tag(T):
    return "k = %d, %s" % (T[0], "cost only" if lsc.cost_only(T) else "D, E")


# ---- A1, B1: the phases at S1 -------------------------------------------------------------------------------------------------------
def phases_covariance(name, forms=0, flags=0, dtype=altro_amd.F64, blocks=None):
    cfg, Ts = cases(name, dtype, blocks)
    st = lsc.restrict(cfg, lsc.state_of(lsc.load_duals(name), crc.config(name), "s1"))
    base = device_phases(cfg, st, forms, flags, dtype)
    bad = []
    for T, out in Ts:
        got = lsc.back(device_phases(out, lsc.transform_state(cfg, out, st), forms, flags, dtype), *T)
        diff = lsc.differing(got, base, lsc.covariant_keys(T))
        if diff:
            bad.append((tag(T), diff))
    return bad


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_phases_at_nonzero_duals_are_covariant(variant):
    """A1, fp64."""
    name, forms, flags = VARIANTS[variant]
    bad = phases_covariance(name, forms, flags)
    assert not bad, bad


@pytest.mark.parametrize("name,blocks", [("tile_tracking", F32_TILE_BLOCKS), ("generic_14_5", None)], ids=["tile_tracking", "generic_14_5"])
def test_phases_at_nonzero_duals_are_covariant_in_fp32(name, blocks):
    """A1 on fp32 handles (k = +-8, narrow D and E): fp32 storage on the tile with its two-slot subset, fp32 arithmetic on plan GENERIC."""
    bad = phases_covariance(name, dtype=altro_amd.F32, blocks=blocks)
    assert not bad, bad


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_phases_at_nonzero_duals_against_the_extended_precision_fixture(variant):
    """B1."""
    name, forms, flags = VARIANTS[variant]
    cfg, fx = crc.config(name), lsc.load_duals(name)
    got = device_phases(cfg, lsc.state_of(fx, cfg, "s1"), forms, flags)
    ratios = lsc.ratios(lsc.errors(got, {q: fx["ref_s1_" + q] for q in lsc.QUANTITIES}), lsc.dual_limits(fx, "s1"))
    print("B1 %-30s " % variant + " ".join("%s %.2g" % (q, r) for q, r in ratios.items()))
    bad = lsc.rejected(ratios, {q: MARGINS[("B1", variant, q)] for q in ratios if ("B1", variant, q) in MARGINS})
    assert not bad, bad


# ---- A2, B2: the update -------------------------------------------------------------------------------------------------------------
def check_frozen(out, res, st, feasible, sweeps, rho0, s, tagged, dtype=altro_amd.F64):
    """What every frozen solve must report, in its own units: status, iterations, dual updates, alpha = 0, the rollout kept, rho+."""
    assert (res["status"] == (0 if feasible else 2)).all(), (tagged, res["status"])
    assert (res["iterations"] == (sweeps if feasible else sweeps + 1)).all(), (tagged, res["iterations"])      # (the oracle's count)
    assert (res["dual_updates"] == sweeps).all(), (tagged, res["dual_updates"])
    assert (res["alpha"] == 0.0).all(), (tagged, res["alpha"])
    if dtype == altro_amd.F64:      # (an fp32 handle's candidate of alpha = 0 restarts from ROUNDED states: dx is a float's rounding, not 0)
        assert np.array_equal(out["u"], st["u"]), tagged
    want = rho0 * s if feasible else min(rho0 * lsc.PENALTY_SCALING ** sweeps, lsc.PENALTY_MAX) * s
    assert (out["rho"] == want).all(), (tagged, out["rho"], want)


def update_covariance(name, forms=0, flags=0, dtype=altro_amd.F64, blocks=None):
    cfg, Ts = cases(name, dtype, blocks)
    st = lsc.restrict(cfg, lsc.state_of(lsc.load_duals(name), crc.config(name), "s2"))
    bad = []
    for which, (feasible, sweeps, rho0) in UPDATES.items():
        kw = dict(feasible=feasible, sweeps=sweeps, rho0=rho0, forms=forms, flags=flags, dtype=dtype)
        base, res = device_update(cfg, st, **kw)
        check_frozen(base, res, st, feasible, sweeps, rho0, 1.0, (which, "old units"), dtype)
        # alpha = 0: the nominal trajectory is the handle's own rollout of the input guess (plan LANE's is not the oracle's bit for bit)
        if dtype == altro_amd.F64:
            assert np.array_equal(base["x"], device_rollout(cfg, st, forms, flags, dtype)), which
        for T, out in Ts:
            stT = lsc.transform_state(cfg, out, st, lsc.RHO0)
            raw, res = device_update(out, stT, **kw)
            check_frozen(raw, res, stT, feasible, sweeps, rho0, out.scale, (which, tag(T)), dtype)
            diff = lsc.differing_update(lsc.back(raw, *T), base, sweep=True)
            if diff:
                bad.append((which, tag(T), diff))
    return bad


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_update_is_covariant(route):
    """A2, fp64."""
    name, forms, flags = ROUTES[route]
    bad = update_covariance(name, forms, flags)
    assert not bad, bad


@pytest.mark.parametrize("name,blocks", [("lane_4_2", None), ("tile_tracking", F32_TILE_BLOCKS), ("generic_14_5", None)],
                         ids=["lane_4_2", "tile_tracking", "generic_14_5"])
def test_the_update_is_covariant_in_fp32(name, blocks):
    """A2 on fp32 handles, k = +-8: the duals are stored as floats, and every factor is a power of two."""
    bad = update_covariance(name, dtype=altro_amd.F32, blocks=blocks)
    assert not bad, bad


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_update_against_the_extended_precision_fixture(route):
    """B2: z+ per kind of block; rho+ with and without the penalty update and at the clamp, by equality; the second sweep's K, d, P, p
    (its expansion runs on z+ and rho+ through the in-solve refresh) and z++."""
    name, forms, flags = ROUTES[route]
    cfg, fx = crc.config(name), lsc.load_duals(name)
    st = lsc.state_of(fx, cfg, "s2")
    got = {which: device_update(cfg, st, feasible, sweeps, rho0, forms=forms, flags=flags)[0] for which, (feasible, sweeps, rho0) in UPDATES.items()}
    assert (got["infeasible"]["rho"] == fx["ref_rho1"]).all() and (got["two sweeps"]["rho"] == fx["ref_rho2"]).all()
    assert (got["feasible"]["rho"] == lsc.RHO0).all() and (got["clamp"]["rho"] == lsc.PENALTY_MAX).all()
    ratios = {}
    for key, which, i in (("z1", "infeasible", 1), ("z1 (no penalty update)", "feasible", 1), ("z2", "two sweeps", 2)):
        e = lsc.dual_errors(cfg, got[which]["z"], lsc.blocks_of(fx, cfg, "ref_z%d" % i))
        ratios.update({"%s:%s" % (key, q): r for q, r in lsc.ratios(e, lsc.dual_limits(fx, "z%d" % i)).items()})
        for nm, ref in lsc.blocks_of(fx, cfg, "ref_z%d" % i).items():        # an exactly zero reference entry is an exact zero
            assert (got[which]["z"][nm][ref == 0.0] == 0.0).all(), (key, nm)
    e = lsc.sweep_errors(got["two sweeps"], {q: fx["ref_sw2_" + q] for q in lsc.SWEEP})
    ratios.update({"sw2:" + q: r for q, r in lsc.ratios(e, lsc.dual_limits(fx, "sw2")).items()})
    print("B2 %-30s " % route + " ".join("%s %.2g" % (q, r) for q, r in ratios.items()))
    bad = lsc.rejected(ratios, {q: MARGINS[("B2", route, q)] for q in ratios if ("B2", route, q) in MARGINS})
    assert not bad, bad


# ---- A3: one sweep with a real line search ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backtracking", [False, True], ids=["cubic", "backtracking"])
@pytest.mark.parametrize("name", crc.CONFIGS)
def test_one_sweep_with_a_line_search_is_covariant_where_the_oracle_is(name, backtracking):
    cfg, Ts = cases(name)
    fx = lsc.load_duals(name)
    mask = fx["ls_mask"][int(backtracking)].astype(bool)
    assert (~mask).sum() <= 2
    s1 = lsc.state_of(fx, cfg, "s1")
    st = dict(s1, rho=np.full(BATCH, lsc.RHO_LS), x=fx["s2_x"])
    kw = dict(feasible=False, sweeps=1, rho0=lsc.RHO_LS, tolg=1e-8, backtracking=backtracking)
    base, res = device_update(cfg, st, **kw)
    assert (base["alpha"][mask] == 1.0).all(), base["alpha"]
    bad = []
    for T, out in Ts:
        got = lsc.back(device_update(out, lsc.transform_state(cfg, out, st), **kw)[0], *T)
        diff = lsc.differing_update(got, base, sweep=True, problems=np.flatnonzero(mask))
        if diff:
            bad.append((tag(T), diff))
        for b in np.flatnonzero(~mask):
            print("A3 %s %s problem %d (outside the mask): alpha %g against %g, differing %s"
                  % (name, tag(T), b, got["alpha"][b], base["alpha"][b], lsc.differing_update(got, base, sweep=True, problems=[b])))
    assert not bad, bad


# ---- S: set state equals carried state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["lane_4_2", "lane_4_2-sequenced", "tile_tracking", "tile_tracking-alrows_lds", "generic_14_5", "auto32_cones", "auto32_rows"])
def test_set_state_equals_carried_state(route):
    """The duals and the penalty a frozen two-sweep solve leaves, written to a fresh handle through set_duals and set_penalty, then
    expand, backward, merit, feasibility, stationarity: the handle that carried them gives the same bits.  set_penalty says the penalty
    the cached projected duals were formed with follows; this holds it to the in-solve refresh."""
    name, forms, flags = ROUTES[route]
    cfg = crc.config(name)
    st = lsc.state_of(lsc.load_duals(name), cfg, "s2")
    left, _, carried = device_update(cfg, st, False, 2, forms=forms, flags=flags, keep=True)
    want = phases_of(carried)
    carried.close()
    assert any((a != 0.0).any() for a in left["z"].values()) and (left["rho"] == lsc.RHO0 * lsc.PENALTY_SCALING ** 2).all()
    got = device_phases(cfg, dict(z=left["z"], rho=left["rho"], x=left["x"], u=left["u"]), forms, flags)
    diff = lsc.differing(got, want)
    assert not diff, diff
