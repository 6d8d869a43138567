"""The affine line-search trials of plan MFMA16 (kernels/ilqr_merit2_dpp.hip: wave_merit_dpp_kernel<.., AFF = true> and
wave_aff_reduce_kernel) judged ONE EVALUATION AT A TIME, through altro_hip_merit_affine / Batch.merit_affine -- the default path of
every constrained solve with dynamics given as data, which whole solves judge only by how many problems end differently.

The call sequence is tests/test_gpu_cone_regions.py's hip_phases up to the backward sweep, then merit_affine(ALPHAS) where that has its
two merit calls: the first call evaluates phi(0) the way a sweep does (the base x_k(0) and its sensitivity s_k), then the trials.
Configurations: tile_tracking and tile_dense (every cone region and exact tie, six constraint slots per knot point, batch 7: a ragged
last wave) at N = 5, 17 and 33 -- one, two and three chunks of MD_AFF_CHUNK = 16 knot points, the last chunk of N = 17 and 33 holding
one knot point and the terminal one -- at penalties 1 and 50.

  a. accuracy     blockerr(device, fixture) <= 10 max(e_cpu, 1e-13) on phi, phi', x, u of the candidate: loop_scale_cases.criterion_b, the
                  yardstick the fixture's STORED oracle error (tests/golden/loop_phases_<config>.npz, extended precision).
  b. covariance   under every change of units of loop_scale_cases.transforms, back(affine(T cfg)) == affine(cfg) bit for bit:
                  powers of two commute with x_b + dalpha s, so a difference is a constant or a floor inside the kernel.
  c. second trial and second round   trials = 2: trial 1 (alpha beta) against merit(alpha beta) of the rollout form on a twin handle; a
                  second round merit_affine(0.25 ALPHAS) from the same stored base against the twin's merit.  No fixture exists at
                  those steps: each form is held to L = 10 max(e_cpu, 1e-13) of the truth at alpha_b, so the two may differ by 2 L.
  d. masks and flags   an active mask that splits the two problems of a wave and switches off the ragged last wave's only problem: what
                  is masked out keeps the sentinel (phi, phi') and the last round's candidate; the complementary mask completes the
                  full-mask call's values bit for bit; no (trial, problem) flag of aff_on survives a round.
  e. seams        tests/problems.py's random (12, 4) problems with and without its constraint blocks at N in {1, 2, 15, 16, 17, 31, 32,
                  48}, batch in {1, 2, 7} -- the terminal knot point in every position of a chunk -- against the oracle's merit function.
  f. every other handle (fp32 records, a device model, plans MFMA32 and LANE, FORM_ROLLOUT_ROUNDS) is refused and stays usable.

Measured on an MI355X; nothing in the kernels had to be fixed, no entry of MARGINS was needed.  a, e_gpu / max(e_cpu, 1e-13), worst over
the penalties, phi / phi' / x / u (10 is the limit; DESIGN section 2 has the rollout form's beside them):
  N = 5   tracking 0.0060 / 3.9 / 0.0086 / 0.034    dense 0.0064 / 0.73 / 0.011 / 0.13
  N = 17  tracking 0.022 / 0.27 / 0.013 / 0.051     dense 0.079 / 0.48 / 0.038 / 0.068
  N = 33  tracking 0.026 / 0.040 / 0.028 / 0.074    dense 0.014 / 0.61 / 0.022 / 0.071
b: bit-identical.  c: 0.0016 .. 0.13 of max(e_cpu, 1e-13), where 20 is the limit.  e: see SEAM_BOUNDS.  Per-test time 0.02 - 0.3 s.
"""
import functools
import os

import numpy as np
import pytest

import altro_amd
from tests import cone_region_cases as crc
from tests import loop_scale_cases as lsc
from tests import problems
from tests import test_gpu_cone_regions as regions
from tests.cone_region_cases import ALPHAS, BATCH, RHOS

pytestmark = pytest.mark.gpu

BETA = 0.5                                   # LsOptions::beta_decrease: trial 1 is alpha beta
KEYS = ("phi", "dphi", "x", "u")
CONFIGS = ("tile_tracking", "tile_dense") + crc.HORIZON_CONFIGS
# (configuration, penalty index, quantity) -> a margin of up to 100 with its CPU explanation in DESIGN section 2.  None is needed.
MARGINS = {}


def test_no_form_is_left_in_the_environment():
    """The binding translates ALTRO_HIP_* variables into forms for every handle of the process (altro_amd.forms_from_env).  A test or a
    tool that leaves one behind -- importing tools/fuzz_dpp.py used to leave ALTRO_HIP_AFFINE=0 -- moves every later test of the run off
    the default kernels without a trace: from there on the suite judged the rollout rounds only."""
    assert altro_amd.forms_from_env() == 0, {k: v for k, v in os.environ.items() if k.startswith("ALTRO_HIP_")}


def to_backward(bt, cfg, rho):
    """hip_phases up to the backward sweep: the guess accepted, zero duals at penalty rho, expansion, gains."""
    bt.set_state_guess(cfg.x); bt.set_input_guess(cfg.u)
    bt.accept()
    bt.reset_duals(rho)
    bt.expand()
    bt.backward()
    assert (bt.get("status") == -1).all()


def handle(cfg, forms=0, **kw):
    bt = regions.make_hip(cfg, **kw)
    bt.set_forms(forms)                      # (make_hip asks for rollout rounds)
    return bt


def candidate(bt, phi, dphi):
    return dict(phi=phi.copy(), dphi=dphi.copy(), x=bt.get("x"), u=bt.get("u"))


def affine(cfg):
    """merit_affine(ALPHAS) of `cfg` (a configuration or a transformed one) at both penalties, in ITS units."""
    bt = handle(cfg)
    out = []
    for rho in RHOS:
        to_backward(bt, cfg, rho * getattr(cfg, "scale", 1.0))
        out.append(candidate(bt, *bt.merit_affine(ALPHAS)))
    bt.close()
    return out


@functools.lru_cache(maxsize=None)
def affine_of(name):
    return affine(crc.config(name))


@pytest.mark.parametrize("name", CONFIGS)
def test_affine_trial_against_the_extended_precision_fixture(name):
    """a."""
    fx = lsc.load(name)
    got = affine_of(name)
    bad = []
    for ri, rho in enumerate(RHOS):
        ratios = lsc.criterion_b(got[ri], fx, ri)
        assert sorted(ratios) == sorted(KEYS)
        print("%-20s affine rho %-3g " % (name, rho) + " ".join("%s %.2g" % (q, ratios[q]) for q in KEYS))
        bad += [(name, rho, q, "ratio %.3g" % r) for q, r in
                lsc.rejected(ratios, {q: MARGINS[(name, ri, q)] for q in ratios if (name, ri, q) in MARGINS}).items()]
    assert not bad, bad


@pytest.mark.parametrize("name", CONFIGS)
def test_affine_trial_is_covariant_under_changes_of_units(name):
    """b."""
    cfg = crc.config(name)
    base = affine_of(name)
    Ts = lsc.transforms(name)
    assert len(Ts) == 4
    bad = []
    for T in Ts:
        got = affine(lsc.transform(cfg, *T))
        for ri, rho in enumerate(RHOS):
            diff = lsc.differing(lsc.back(got[ri], *T), base[ri], KEYS)
            if diff:
                bad.append(("k = %d" % T[0], "cost only" if lsc.cost_only(T) else "D, E", "rho %g" % rho, diff))
    assert not bad, bad


@pytest.mark.parametrize("name", CONFIGS)
def test_second_trial_and_second_round_against_the_rollout_form(name):
    """c.  (phi is what the rule is stated for; phi', x and u of the second round are held to the same rule with their own e_cpu.)"""
    cfg = crc.config(name)
    fx = lsc.load(name)
    bt, twin = handle(cfg), handle(cfg, altro_amd.FORM_ROLLOUT_ROUNDS)
    bad = []
    for ri, rho in enumerate(RHOS):
        lim = lsc.limits(fx["ecpu_%d" % ri])
        to_backward(bt, cfg, rho); to_backward(twin, cfg, rho)
        phi2, dphi = bt.merit_affine(ALPHAS, trials=2)
        assert phi2.shape == (2, BATCH) and np.array_equal(phi2[0], affine_of(name)[ri]["phi"]) and np.array_equal(dphi, affine_of(name)[ri]["dphi"])
        want, _ = twin.merit(ALPHAS * BETA)
        e = {"trial 1 phi": lsc.errors(dict(phi=phi2[1]), dict(phi=want))["phi"] / lim["phi"]}
        got = candidate(bt, *bt.merit_affine(0.25 * ALPHAS))              # the second round: the stored base again
        ref = candidate(twin, *twin.merit(0.25 * ALPHAS))
        e.update({"round 2 " + q: v / lim[q] for q, v in lsc.errors(got, ref).items()})
        print("%-20s rho %-3g |affine - rollout| / max(e_cpu, 1e-13): " % (name, rho) + " ".join("%s %.2g" % kv for kv in e.items()))
        bad += [(name, rho, what, r) for what, r in e.items() if not r <= 2 * lsc.MARGIN]
    bt.close(); twin.close()
    assert not bad, bad


MASK = np.array([1, 0, 0, 1, 1, 1, 0])       # waves (0, 1), (2, 3) split; (4, 5) whole; the ragged last wave's only problem off
SENTINEL = -7.25


@pytest.mark.parametrize("name", ("tile_tracking", "tile_dense_n17", "tile_tracking_n33"))
def test_masks_and_flags(name):
    """d."""
    cfg = crc.config(name)
    bt = handle(cfg)
    to_backward(bt, cfg, RHOS[1])
    full = affine_of(name)[1]
    prev = candidate(bt, *bt.merit_affine(0.5 * ALPHAS))                  # the round before: what a masked-out problem keeps
    assert not np.array_equal(prev["x"][:, 1:], full["x"][:, 1:])
    seen = np.zeros(BATCH, dtype=bool)
    for mask in (MASK, 1 - MASK):
        on = mask != 0
        assert on.any() and not on.all()
        phi, dphi = np.full(BATCH, SENTINEL), np.full(BATCH, SENTINEL)
        bt.merit_affine(ALPHAS, active=mask, out=(phi, dphi))
        got = candidate(bt, phi, dphi)
        seen |= on
        assert (phi[~seen] == SENTINEL).all() and (dphi[~seen] == SENTINEL).all(), (mask, phi, dphi)
        assert (phi[~on] == SENTINEL).all() and (dphi[~on] == SENTINEL).all(), ("a stale flag was picked up", mask, phi, dphi)
        for q in KEYS:
            assert np.array_equal(got[q][on], full[q][on]), (q, mask)
        for q in ("x", "u"):
            assert np.array_equal(got[q][~seen], prev[q][~seen]), (q, mask)
            assert np.array_equal(got[q][seen], full[q][seen]), (q, mask)
    assert seen.all()
    # trials = 2, then trials = 1.  No flag of either round is left for a later reduction to find: a round in which nobody is active, with
    # the sentinel in both rows, stores nothing.  (The entry writes trials * batch values: trial 1's row of the caller's array stays.)
    def nothing_is_flagged():
        probe, dprobe = np.full((2, BATCH), SENTINEL), np.full(BATCH, SENTINEL)
        bt.merit_affine(ALPHAS, active=np.zeros(BATCH, dtype=int), trials=2, out=(probe, dprobe))
        return bool((probe == SENTINEL).all() and (dprobe == SENTINEL).all())

    phi2, _ = bt.merit_affine(ALPHAS, trials=2)
    assert np.array_equal(phi2[0], full["phi"]) and np.isfinite(phi2[1]).all() and not np.array_equal(phi2[0], phi2[1])
    assert nothing_is_flagged()
    buf = phi2.copy()
    bt.merit_affine(0.5 * ALPHAS, out=(buf.reshape(-1)[:BATCH], np.zeros(BATCH)))
    assert np.array_equal(buf[0], prev["phi"]) and np.array_equal(buf[1], phi2[1])
    assert nothing_is_flagged()
    for q in ("x", "u"):
        assert np.array_equal(bt.get(q), prev[q])
    # and the handle goes on: the rollout kernels' evaluation of the same step is within 2 L of the stored round (see c)
    phi_r, _ = bt.merit(ALPHAS)
    L = lsc.MARGIN * lsc.limits(lsc.load(name)["ecpu_1"])["phi"]
    assert lsc.errors(dict(phi=full["phi"]), dict(phi=phi_r))["phi"] <= 2 * L
    bt.close()


# ---- e. seams: random problems against the oracle's merit function -------------------------------------------------------------------
class Seam:
    """What cone_region_cases.make_oracle reads of a configuration, for tests/problems.py's (12, 4) problem."""
    n, m, dyn, dense = 12, 4, "data", False

    def __init__(self, batch, N, constrained):
        self.N, self.batch = N, batch
        self.p = problems.ilqr12x4_problem(batch, N, True)
        self.x0 = self.p["x0"]
        self.blocks = [dict(k0=k0, k1=k1, cone=cone, G=G, g=g) for (k0, k1, cone, G, g) in (problems.ilqr12x4_constraint_blocks(N) if constrained else [])
                       if k0 <= k1]

    def at(self, k):
        return [j for j, bl in enumerate(self.blocks) if bl["k0"] <= k <= bl["k1"]]


SEAM_RHO = 10.0
# Bounds of part e, in the measure of the project's phase-level comparisons with the oracle (tests/test_gpu_ilqr_mfma16.py, whose
# tolerances they started from: phi 1e-11 and phi' 1e-9 of max(1, |ref|), candidates 1e-10 of 1 + |ref|), tightened to TEN TIMES the
# largest deviation the ROLLOUT form (FORM_ROLLOUT_ROUNDS, Batch.merit) shows against the oracle over these same 48 cases on an MI355X:
# rollout form  phi 1.12e-15 (N = 31, blocks), phi' 7.67e-15 (N = 48, free), x 1.45e-15 (N = 48, free), u 1.00e-14 (N = 48, free).
# The affine form measured 1.60e-15, 5.83e-15, 3.83e-15 and 1.64e-14 (its figures set nothing; the test prints both forms).
SEAM_BOUNDS = dict(phi=1.12e-14, dphi=7.67e-14, x=1.45e-14, u=1.00e-13)


def _seam_errors(got, ref):
    out = {q: abs(got[q] - ref[q]) / max(1.0, abs(ref[q])) for q in ("phi", "dphi")}
    out.update({q: float((np.abs(got[q] - ref[q]) / (1.0 + np.abs(ref[q]))).max()) for q in ("x", "u")})
    return out


@pytest.mark.parametrize("constrained", [False, True], ids=["free", "blocks"])
@pytest.mark.parametrize("N", [1, 2, 15, 16, 17, 31, 32, 48])
def test_seams_against_the_oracle(N, constrained):
    """e.  Both forms are measured; the affine one is asserted (the rollout form has its own tests)."""
    worst = {"affine": {}, "rollout": {}}
    for batch in (1, 2, 7):
        case = Seam(batch, N, constrained)
        p = case.p
        alphas = np.linspace(0.15, 1.1, batch)
        res = {}
        for form, forms in (("affine", 0), ("rollout", altro_amd.FORM_ROLLOUT_ROUNDS)):
            bt = altro_amd.Batch(N, 12, 4, batch)
            bt.set_forms(forms)
            bt.set_dynamics(p["A"], p["B"], p["f"])
            bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
            for bl in case.blocks:
                bt.add_linear_constraint(bl["k0"], bl["k1"], bl["cone"], bl["G"], bl["g"])
            bt.set_initial_state(p["x0"]); bt.set_input_guess(p["u0"])
            assert bt.plan == altro_amd.PLAN_MFMA16
            bt.open_loop_rollout(); bt.accept()
            if constrained:
                bt.reset_duals(SEAM_RHO)
            bt.expand(); bt.backward()
            assert (bt.get("status") == -1).all()
            res[form] = candidate(bt, *(bt.merit_affine(alphas) if form == "affine" else bt.merit(alphas)))
            bt.close()
        for b in range(batch):
            s = crc.make_oracle(case, b)
            for k in range(N):
                s.L.oracle_ilqr_set_input(s.h, k, crc._c(p["u0"][b, k]))
            s.L.oracle_ilqr_open_loop_rollout(s.h)
            if constrained:
                s.set_penalty(1.0, SEAM_RHO)
                s.L.oracle_ilqr_penalty_update(s.h)
            crc.expand(s)
            assert s.L.oracle_ilqr_backward_pass(s.h) == -1
            phi, dphi = s.merit(alphas[b])
            ref = dict(phi=phi, dphi=dphi, x=s.get("x_cand"), u=s.get("u_cand"))
            for form in res:
                e = _seam_errors({q: res[form][q][b] for q in KEYS}, ref)
                for q, v in e.items():
                    worst[form][q] = max(worst[form].get(q, 0.0), v)
    for form in ("rollout", "affine"):
        print("N %-2d %-6s %-7s against the oracle: " % (N, "blocks" if constrained else "free", form) + " ".join("%s %.2e" % (q, worst[form][q]) for q in KEYS))
    bad = {q: v for q, v in worst["affine"].items() if not v <= SEAM_BOUNDS[q]}
    assert not bad, bad


# ---- f. every other handle ------------------------------------------------------------------------------------------------------------
def _model_handle():
    from tests import test_gpu_loop_scales as gls
    c = gls._model_cases()["quadrotor_tile"]
    bt = altro_amd.Batch(gls.NM, c["n"], c["m"], gls.BM, plan=c["plan"])
    bt.set_model(c["model"], c["h"])
    bt.set_tracking_cost(np.stack([c["Qd"], c["Qfd"]]), c["Rd"][None], np.stack([c["xref"], c["xref"]]), c["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(c["x0"])
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.backward()
    return bt, gls.ALPHAS_M


def _config_handle(name, forms, blocks=None, **kw):
    cfg = crc.config(name) if blocks is None else lsc.subset(crc.config(name), blocks)
    bt = handle(cfg, forms, **kw)
    to_backward(bt, cfg, 1.0)
    return bt, ALPHAS


OTHERS = {
    "fp32 storage": lambda: _config_handle("tile_tracking", 0, ("cone4", "box", "cone4_N", "cone3_N"), dtype=altro_amd.F32),
    "device model": _model_handle,
    "plan MFMA32": lambda: _config_handle("auto32_cones", 0),
    "plan LANE": lambda: _config_handle("lane_4_2", 0),
    "rollout rounds": lambda: _config_handle("tile_tracking", altro_amd.FORM_ROLLOUT_ROUNDS),
}


@pytest.mark.parametrize("which", list(OTHERS))
def test_every_other_handle_is_refused_and_stays_usable(which):
    """f."""
    bt, alphas = OTHERS[which]()
    assert (bt.get("status") == -1).all()
    before = bt.merit(alphas)
    for trials in (1, 2):
        with pytest.raises(altro_amd.AltroHipError, match="affine line-search trials need"):
            bt.merit_affine(alphas, trials=trials)
    after = bt.merit(alphas)
    assert np.isfinite(before[0]).all() and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    bt.close()


def test_arguments_are_checked():
    cfg = crc.config("tile_tracking")
    bt = handle(cfg)
    bt.set_state_guess(cfg.x); bt.set_input_guess(cfg.u); bt.accept(); bt.reset_duals(1.0); bt.expand()
    with pytest.raises(altro_amd.AltroHipError, match="backward must precede"):
        bt.merit_affine(ALPHAS)
    bt.backward()
    with pytest.raises(altro_amd.AltroHipError, match="trials must be 1 or 2"):
        bt.merit_affine(ALPHAS, trials=3)
    phi, _ = bt.merit_affine(ALPHAS)
    assert np.array_equal(phi, affine_of("tile_tracking")[0]["phi"])
    bt.close()
