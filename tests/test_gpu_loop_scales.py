"""The iLQR loop's phases -- expansion, AL terms, backward sweep, merit function, candidates, feasibility, stationarity -- judged
without the floor of 1 and at every scale, through the C ABI (tests/loop_scale_cases.py holds the transform and the metric,
tests/test_loop_scale_cases.py shows both on the oracle alone).  Needs an MI355X; reads nothing outside the repository, no mpmath.

The call sequence is tests/test_gpu_cone_regions.py's part a (hip_phases): set_state_guess, set_input_guess, accept, reset_duals(rho s),
expand, backward, merit(0), merit(alpha_b), feasibility, stationarity -- on its seven configurations (every cone region and exact tie,
plans LANE, MFMA16, GENERIC, MFMA32 and MFMA32's row layout), N = 5, batch 7, zero duals, penalties 1 and 50.

  A. Covariance.  For every change of units T of loop_scale_cases.transforms (the cost times 4^+-20; with dynamics as data also k = +-5
     with D in 2^[-10, 10], E in 2^[-6, 6]), back(device(T cfg)) == device(cfg) BIT FOR BIT on lx, lu, K, d, P, p, phi, phi' at alpha = 0
     and alpha_b, the candidates, feasibility and (under k alone) stationarity.  Also with another kernel under a phase (the tile's LDS
     merit form and its LDS expansion / constraint-row forms, FORM_GENERIC_MERIT_LDS on auto32_rows, GENERIC_MATRIX_CORES on generic_14_5), on the compiled-in device models
     (k = +-20: quadrotor on the tile, 13-state quadrotor on plan MFMA32, pendulum and bicycle on plan LANE, N = 8, batch 8, thrust box on
     the quadrotors) and in fp32 (storage on the tile, arithmetic on plan GENERIC: k = +-8, D in 2^[-4, 4], E in 2^[-3, 3]).
  B. Accuracy.  In the old units blockerr(device, fixture) <= 10 max(e_cpu, 1e-13) per quantity and penalty, against the
     extended-precision evaluation of tests/golden/loop_phases_<config>.npz; e_cpu is the fixture's stored error of the oracle.  The
     ratios e_gpu / max(e_cpu, 1e-13) are printed.

Measured on an MI355X.  A: bit-identical everywhere, nothing had to be fixed; s = 2^7 moves K, d and what follows by 1e-16 .. 5e-13.
B, e_gpu / max(e_cpu, 1e-13), worst over the penalties and forms (10 is the limit, no entry of MARGINS was needed):
  plan LANE     1.0 (K, d, phi, phi', u of (4, 2) at penalty 50: e_cpu = 1.1e-13 .. 1.5e-13 is above the floor there), else <= 0.9
  plan MFMA16   phi' 3.6 (tracking cost, penalty 50: 1.3e-12 against the oracle's 3.6e-13), phi' 0.72 (dense cost), else <= 0.13
  plan GENERIC  <= 0.027, with GENERIC_MATRIX_CORES too
  plan MFMA32   cones: phi'(0) 3.9 (penalty 50: 2.8e-12 against 7.2e-13), phi'(alpha_b) 0.15, else <= 0.03; row layout and the kernels of
                FORM_GENERIC_MERIT_LDS under it: <= 0.054
Plan LANE's loop kernels are not asserted to give the oracle's bits: the project claims 1e-13 of the oracle for them, and on these two
configurations no phase quantity, lx included, is bit-identical to the oracle (measured).  Per-test time 0.01 - 0.3 s.
"""
import numpy as np
import pytest

import altro_amd
from tests import cone_region_cases as crc
from tests import loop_scale_cases as lsc
from tests import test_gpu_cone_regions as regions
from tests.cone_region_cases import RHOS

pytestmark = pytest.mark.gpu

ROUNDS = altro_amd.FORM_ROLLOUT_ROUNDS
# id -> (configuration, forms on top of the rollout rounds, handle flags)
VARIANTS = {name: (name, 0, 0) for name in crc.CONFIGS}
VARIANTS.update({
    "tile_tracking-merit_lds": ("tile_tracking", altro_amd.FORM_MERIT_LDS, 0),
    "tile_dense-merit_lds": ("tile_dense", altro_amd.FORM_MERIT_LDS, 0),
    "tile_tracking-expand_lds": ("tile_tracking", altro_amd.FORM_EXPAND_LDS | altro_amd.FORM_ALROWS_LDS, 0),
    "tile_dense-expand_lds": ("tile_dense", altro_amd.FORM_EXPAND_LDS | altro_amd.FORM_ALROWS_LDS, 0),
    "auto32_rows-generic_merit_lds": ("auto32_rows", altro_amd.FORM_GENERIC_MERIT_LDS, 0),
    "generic_14_5-matrix_cores": ("generic_14_5", 0, altro_amd.GENERIC_MATRIX_CORES),
})
# the tile's two configurations at N = 17 and N = 33 (tests/cone_region_cases.py HORIZON_CONFIGS), rollout form: part B only -- the
# rollout kernels past one chunk of the affine trials (tests/test_gpu_affine_phases.py judges the affine form on the same fixtures)
VARIANTS_B = dict(VARIANTS, **{name: (name, 0, 0) for name in crc.HORIZON_CONFIGS})
# (variant, penalty index, quantity) -> a margin of up to 100 with its CPU explanation in DESIGN section 2.  None is needed.
MARGINS = {}


def device(cfg, forms=0, flags=0, dtype=altro_amd.F64):
    """hip_phases of `cfg` (a configuration or a transformed one) at both penalties, in ITS units: [per penalty] {quantity: batch array}."""
    bt = regions.make_hip(cfg, dtype=dtype, flags=flags)
    bt.set_forms(ROUNDS | forms)
    out = [regions.hip_phases(bt, cfg.x, cfg.u, rho * getattr(cfg, "scale", 1.0)) for rho in RHOS]
    bt.close()
    return out


def covariance(name, forms=0, flags=0, dtype=altro_amd.F64, blocks=None):
    cfg = crc.config(name) if blocks is None else lsc.subset(crc.config(name), blocks)
    base = device(cfg, forms, flags, dtype)
    bad = []
    for T in lsc.transforms(name, fp32=dtype == altro_amd.F32):
        got = device(lsc.transform(cfg, *T), forms, flags, dtype)
        for ri, rho in enumerate(RHOS):
            diff = lsc.differing(lsc.back(got[ri], *T), base[ri], lsc.covariant_keys(T))
            if diff:
                bad.append(("k = %d" % T[0], "cost only" if lsc.cost_only(T) else "D, E", "rho %g" % rho, diff))
    return bad


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_phases_are_covariant_under_changes_of_units(variant):
    """Part A, fp64."""
    name, forms, flags = VARIANTS[variant]
    bad = covariance(name, forms, flags)
    assert not bad, bad


@pytest.mark.parametrize("name", ["tile_tracking", "auto32_cones"])
def test_a_scale_that_is_no_power_of_four_is_not_exact(name):
    """The comparison of part A can fail: under s = 2^7 the factorisation's square root rounds differently and the gains move in their
    last bits, on the device as on the oracle (tests/test_loop_scale_cases.py)."""
    cfg = crc.config(name)
    T = lsc.identity(cfg)
    base, got = device(cfg), device(lsc.transform(cfg, *T, scale=2.0 ** 7))
    for ri in range(len(RHOS)):
        diff = lsc.differing(lsc.back(got[ri], *T, scale=2.0 ** 7), base[ri])
        print(name, RHOS[ri], diff)
        assert "K" in diff and "d" in diff, diff


@pytest.mark.parametrize("name,blocks", [("tile_tracking", ("cone4", "box", "cone4_N", "cone3_N")), ("generic_14_5", None)],
                         ids=["tile_tracking", "generic_14_5"])
def test_phases_are_covariant_in_fp32(name, blocks):
    """Part A on fp32 handles: fp32 storage on the tile, fp32 arithmetic on plan GENERIC.  An fp32 handle of the tile takes two constraint
    slots per knot point where tile_tracking fills six: it runs with one cone and the input box (two cones at the terminal knot point)."""
    bad = covariance(name, dtype=altro_amd.F32, blocks=blocks)
    assert not bad, bad


@pytest.mark.parametrize("variant", list(VARIANTS_B))
def test_phases_against_the_extended_precision_fixture(variant):
    """Part B."""
    name, forms, flags = VARIANTS_B[variant]
    fx = lsc.load(name)
    got = device(crc.config(name), forms, flags)
    bad = []
    for ri, rho in enumerate(RHOS):
        ratios = lsc.criterion_b(got[ri], fx, ri)
        print("%-30s rho %-3g " % (variant, rho) + " ".join("%s %.2g" % (q, r) for q, r in ratios.items()))
        bad += [(variant, rho, q, "ratio %.3g" % r) for q, r in
                lsc.rejected(ratios, {q: MARGINS[(variant, ri, q)] for q in ratios if (variant, ri, q) in MARGINS}).items()]
    assert not bad, bad


# ---- device models: the cost scale alone ---------------------------------------------------------------------------------------------
NM, BM = 8, 8
ALPHAS_M = np.linspace(0.15, 1.1, BM)


def _model_cases():
    from tests import test_gpu_generic_model as g13
    from tests import test_gpu_ilqr as lane
    from tests import test_gpu_tile_model as tile
    out = {}
    for key, mod, model, plan in (("quadrotor_tile", tile, altro_amd.MODEL_QUADROTOR, altro_amd.PLAN_MFMA16),
                                  ("quadrotor13_mfma32", g13, altro_amd.MODEL_QUADROTOR13, altro_amd.PLAN_MFMA32)):
        c = mod.make_case(BM) if mod is g13 else mod.make_case(BM, False)
        n, m = c["x0"].shape[1], 4
        Gb = np.zeros((2, n + m)); Gb[0, n] = 1.0; Gb[1, n] = -1.0         # the thrust box of those tests' constrained solves
        out[key] = dict(model=model, plan=plan, want=plan, n=n, m=m, h=mod.H, Qd=c["Qd"], Qfd=c["Qfd"], Rd=c["Rd"], xref=c["xref"],
                        uref=c["uref"], x0=c["x0"], u0=c["u0"],
                        blocks=[(0, NM - 1, altro_amd.CONE_INEQUALITY, Gb, np.array([1.25 * mod.HOVER[0], -0.6 * mod.HOVER[0]]))])
    for key in ("pendulum", "bicycle"):
        c = lane.CASES[key]
        f = lambda v: np.asarray(v, dtype=np.float64)
        out[key + "_lane"] = dict(model=c["model"], plan=altro_amd.PLAN_AUTO, want=altro_amd.PLAN_LANE, n=c["n"], m=c["m"], h=c["h"], Qd=f(c["Qd"]),
                                  Qfd=f(c["Qfd"]), Rd=f(c["Rd"]), xref=f(c["xf"]), uref=np.zeros(c["m"]), x0=c["x0"](BM), u0=f(c["u0"]), blocks=[])
    return out


def model_phases(c, s, rho):
    bt = altro_amd.Batch(NM, c["n"], c["m"], BM, plan=c["plan"])
    bt.set_forms(ROUNDS)
    bt.set_model(c["model"], c["h"])
    bt.set_tracking_cost(np.stack([c["Qd"] * s, c["Qfd"] * s]), (c["Rd"] * s)[None], np.stack([c["xref"], c["xref"]]), c["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(c["x0"])
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    for (k0, k1, cone, G, g) in c["blocks"]:
        bt.add_linear_constraint(k0, k1, cone, G, g)
    assert bt.plan == c["want"]
    bt.open_loop_rollout(); bt.accept()
    if c["blocks"]:
        bt.reset_duals(rho * s)
    bt.expand()
    _, _, lx, lu = bt.get_expansion()
    bt.backward()
    assert (bt.get("status") == -1).all()
    r = dict(lx=lx, lu=lu, K=bt.get("K"), d=bt.get("d"), P=bt.get("P"), p=bt.get("p"))
    r["phi0"], r["dphi0"] = bt.merit(np.zeros(BM))
    r["phi"], r["dphi"] = bt.merit(ALPHAS_M)
    r["x"], r["u"] = bt.get("x"), bt.get("u")
    if c["blocks"]:
        r["feas"] = bt.feasibility()
    r["stat"] = bt.stationarity()
    bt.close()
    return r


@pytest.mark.parametrize("key", ["quadrotor_tile", "quadrotor13_mfma32", "pendulum_lane", "bicycle_lane"])
def test_device_models_are_covariant_under_the_cost_scale(key):
    """Part A on the compiled-in models: scaling the cost touches no trigonometric argument, so the whole cost times 4^+-20 must give
    the unscaled phases bit for bit."""
    c = _model_cases()[key]
    one_n, one_m = np.ones(c["n"]), np.ones(c["m"])
    bad = []
    for rho in (RHOS if c["blocks"] else RHOS[:1]):
        base = model_phases(c, 1.0, rho)
        keys = [q for q in lsc.QUANTITIES if q in base]
        for k in (20, -20):
            got = lsc.back(model_phases(c, 4.0 ** k, rho), k, one_n, one_m)
            diff = lsc.differing(got, base, keys)
            if diff:
                bad.append(("k = %d" % k, "rho %g" % rho, diff))
    assert not bad, bad
