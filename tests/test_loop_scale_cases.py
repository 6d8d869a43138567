"""The two yardsticks of tests/test_gpu_loop_scales.py, shown on the CPU from the oracle alone (tests/loop_scale_cases.py):

  A. the oracle's phases are covariant BIT FOR BIT under every change of units the device is run under -- and not under a cost scale
     that is no power of four, so the comparison can fail;
  B. the extended-precision fixtures (tests/golden/loop_phases_<config>.npz) are the ones their inputs produce, and the criterion
     blockerr <= 10 max(e_cpu, 1e-13) has teeth: one quantity of the oracle's own phases rounded to float32 and back, or off by 1e-9
     of its size, is rejected on every configuration, as is one coordinate of lx that is off by 1e-9 of its own size.  Beside each it
     is printed whether the tolerances of tests/test_gpu_cone_regions.py, the tightest phase-by-phase test there was, would have
     accepted it.  The outcome: rounded to float32 they reject lx, K, x, phi' and accept feasibility (14 of 14
     cases) and stationarity (8 of 14: plans LANE / MFMA16); off by 1e-9 they accept K, feasibility, stationarity (14 of 14) and
     phi', x, u (8 of 14).

And those of tests/test_gpu_dual_scales.py (nonzero duals, the dual update, the penalty update): the oracle's setters round-trip and
reproduce the carried state bit for bit; S2 reaches every region away from the boundaries; the oracle is covariant bit for bit at S1
and through the frozen update (with and without the penalty update, at the clamp, over two sweeps), and s = 2^7 moves the second
sweep's gains while the frozen duals stay exact (with a real line search they move); the sweep with a real line search accepts
alpha = 1 everywhere on all but at most 2 of 7 problems; the fixtures tests/golden/loop_phases_duals_<config>.npz are what their inputs
produce; and criterion B rejects one dual block in float32 or off by 1e-9 (the largest and the smallest nonzero one per kind),
inactive rows that keep their duals, and rho+ used for rho -- all of which tests/test_gpu_cone_regions.py's 1e-12 of max(1, block)
rejects too on these states (0 of 65 accepted: the smallest nonzero dual block is 1.3e-2)."""
import numpy as np
import pytest

from tests import cone_region_cases as crc
from tests import loop_scale_cases as lsc
from tests import test_gpu_cone_regions as regions        # its tolerances and its comparison; nothing of it touches the GPU here
from tests.cone_region_cases import BATCH, RHOS
from tests.golden_cases import checksum

_oracle = {}


def oracle(name, ri):
    if (name, ri) not in _oracle:
        _oracle[(name, ri)] = lsc.oracle_phases(crc.config(name), RHOS[ri])
    return _oracle[(name, ri)]


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_oracle_is_covariant_bit_for_bit(name):
    cfg = crc.config(name)
    Ts = lsc.transforms(name)
    assert len(Ts) == (4 if cfg.dyn == "data" else 2) and sum(lsc.cost_only(T) for T in Ts) == 2
    for ri, rho in enumerate(RHOS):
        for T in Ts:
            got = lsc.back(lsc.oracle_phases(lsc.transform(cfg, *T), rho), *T)
            assert not lsc.differing(got, oracle(name, ri), lsc.covariant_keys(T)), (name, rho, T[0])
            assert ("stat" in lsc.covariant_keys(T)) == lsc.cost_only(T)


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_a_scale_that_is_no_power_of_four_is_not_exact(name):
    """s = 2^7: sqrt(s Quu) != sqrt(s) sqrt(Quu) in floating point; everything from the gains on moves in its last bits, nothing before."""
    cfg = crc.config(name)
    T = lsc.identity(cfg)
    for ri, rho in enumerate(RHOS):
        got = lsc.back(lsc.oracle_phases(lsc.transform(cfg, *T, scale=2.0 ** 7), rho), *T, scale=2.0 ** 7)
        diff = lsc.differing(got, oracle(name, ri))
        assert {"K", "d", "P", "p", "x", "u"} <= set(diff) and not {"lx", "lu"} & set(diff), diff
        assert max(diff.values()) < 1e-11, diff


def test_transform_refuses_what_is_not_exact():
    cfg = crc.config("tile_dense")
    k, D, E = lsc.identity(cfg)
    with pytest.raises(AssertionError):
        lsc.transform(cfg, k, D * 3.0, E)                       # not a power of two
    with pytest.raises(AssertionError):
        lsc.transform(cfg, -530, D, E)                          # the scaled cost leaves the normal range
    with pytest.raises(AssertionError):
        lsc.transform(crc.config("lane_4_2"), 0, 2.0 * np.ones(4), np.ones(2))        # a device model's dynamics are not data


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_fixtures_are_what_their_inputs_produce(name):
    cfg = crc.config(name)
    fx = lsc.load(name)
    assert checksum(lsc.inputs(cfg)) == fx["sum"]
    for ri, rho in enumerate(RHOS):
        assert np.array_equal(fx["tab_%d" % ri], lsc.class_tables(cfg, rho))
        assert fx["flips_%d" % ri] == 0                         # the frozen branches are the ones extended precision takes
        e = lsc.errors(oracle(name, ri), lsc.reference(fx, ri))
        assert np.array_equal(np.array([e[q] for q in lsc.QUANTITIES]), fx["ecpu_%d" % ri]), e
        assert fx["ecpu_%d" % ri].max() < 1e-12                 # (the oracle is accurate here: the limits are the floor's, 1e-12, or close)
        assert all(np.isfinite(fx["ref_%d_%s" % (ri, q)]).all() for q in lsc.QUANTITIES)
        assert not lsc.rejected(lsc.criterion_b(oracle(name, ri), fx, ri))


@pytest.mark.parametrize("name", crc.HORIZON_CONFIGS)
def test_horizon_fixtures_are_what_their_inputs_produce_and_the_oracle_meets_criterion_b(name):
    """The tile's two configurations at N = 17 and N = 33 (two and three chunks of the affine trials): the same blocks as at N = 5, the
    fixture is the one its inputs produce, and the oracle alone meets criterion B on every quantity the fixture holds -- at N = 33 the
    merit phase's (loop_scale_cases.MERIT_QUANTITIES; the file would otherwise be the largest under tests/golden)."""
    cfg, base = crc.config(name), crc.config(name.rsplit("_n", 1)[0])
    assert cfg.N == int(name.rsplit("_n", 1)[1]) and cfg.base == base.name and cfg.dense == base.dense
    assert cfg.x.shape == (BATCH, cfg.N + 1, 12) and cfg.u.shape == (BATCH, cfg.N, 4)
    assert [bl["name"] for bl in cfg.blocks] == [bl["name"] for bl in base.blocks]
    for bl, b0 in zip(cfg.blocks, base.blocks):
        assert np.array_equal(bl["G"], b0["G"]) and (bl["k0"], bl["k1"]) == ((0, cfg.N - 1) if b0["k0"] == 0 else (cfg.N, cfg.N))
        assert bl["name"] == "orth12" or np.array_equal(bl["g"], b0["g"])      # (orth12's g[0] is its tie's: set where the tie is scheduled)
    assert set(cfg.schedule.values()) == set(base.schedule.values())           # every special class and exact tie is still reached
    assert lsc.transforms(name)[2][0] == lsc.transforms(base.name)[2][0] and np.array_equal(lsc.transforms(name)[2][1], lsc.transforms(base.name)[2][1])
    fx = lsc.load(name)
    assert checksum(lsc.inputs(cfg)) == fx["sum"]
    held = [q for q in lsc.QUANTITIES if "ref_0_" + q in fx]
    assert held == list(lsc.QUANTITIES if cfg.N == 17 else [q for q in lsc.QUANTITIES if q in lsc.MERIT_QUANTITIES])
    for ri, rho in enumerate(RHOS):
        assert np.array_equal(fx["tab_%d" % ri], lsc.class_tables(cfg, rho))
        assert fx["flips_%d" % ri] == 0
        got = oracle(name, ri)
        e = lsc.errors(got, lsc.reference(fx, ri))
        assert sorted(e) == sorted(held)
        ecpu = dict(zip(lsc.QUANTITIES, fx["ecpu_%d" % ri]))
        assert all(e[q] == ecpu[q] for q in held) and all(np.isnan(ecpu[q]) for q in lsc.QUANTITIES if q not in held), (e, ecpu)
        assert max(e.values()) < 1e-12
        assert all(np.isfinite(fx["ref_%d_%s" % (ri, q)]).all() for q in held)
        ratios = lsc.criterion_b(got, fx, ri)
        print(name, "rho", rho, " ".join("%s %.2g" % (q, r) for q, r in ratios.items()))
        assert sorted(ratios) == sorted(held) and not lsc.rejected(ratios)
        spoilt = dict(got, phi=got["phi"] * (1.0 + 1e-9))                      # (the criterion has teeth at these horizons too)
        assert set(lsc.rejected(lsc.criterion_b(spoilt, fx, ri))) == {"phi"}


def _accepted_today(cfg, got, name, ri):
    """Would tests/test_gpu_cone_regions.py's comparison with the oracle have accepted `got`?"""
    ref = crc.zero_dual_reference(name)
    return not any(regions.compare(cfg, got, ref[(RHOS[ri], b)], b, "", {}) for b in range(BATCH))


ROUNDED = ("lx", "K", "x", "dphi", "feas", "stat")
SPOILT = {"in float32": lambda a: a.astype(np.float32).astype(np.float64),           # one intermediate kept in fp32: 6e-8
          "times 1 + 1e-9": lambda a: a * (1.0 + 1e-9)}                                # a dropped term of relative size 1e-9


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_criterion_b_rejects_one_spoilt_quantity(name):
    """One quantity of the oracle's phases at a time, rounded to float32 and back (lx, K, the candidate x, phi', feasibility,
    stationarity) or off by 1e-9 of its size (every quantity): criterion B rejects that quantity, and no other."""
    cfg = crc.config(name)
    fx = lsc.load(name)
    for ri, rho in enumerate(RHOS):
        base = oracle(name, ri)
        assert _accepted_today(cfg, base, name, ri)
        for how, spoil in SPOILT.items():
            for q in (ROUNDED if how == "in float32" else lsc.QUANTITIES):
                got = dict(base)
                got[q] = spoil(base[q])
                bad = lsc.rejected(lsc.criterion_b(got, fx, ri))
                today = _accepted_today(cfg, got, name, ri)
                print("%-14s rho %-3g %-5s %-14s: criterion B ratio %8.3g, today's tolerance %s"
                      % (name, rho, q, how, bad.get(q, 0.0), "ACCEPTS" if today else "rejects"))
                assert set(bad) == {q}, (name, rho, q, how, bad)


@pytest.mark.parametrize("name", [n for n in crc.CONFIGS if crc.config(n).dyn == "data"])
def test_criterion_b_rejects_one_small_coordinate_off_by_1e_9(name):
    """In the units of a mixed transform, the coordinate of lx whose D is smallest is moved by 1e-9 of its own size at every knot
    point; mapped back to the old units criterion B rejects it."""
    cfg = crc.config(name)
    fx = lsc.load(name)
    T = lsc.transforms(name)[2]
    assert not lsc.cost_only(T)
    i = int(np.argmin(T[1]))
    for ri, rho in enumerate(RHOS):
        got = lsc.oracle_phases(lsc.transform(cfg, *T), rho)
        got["lx"][:, :, i] *= 1.0 + 1e-9
        res = lsc.back(got, *T)
        res["stat"] = oracle(name, ri)["stat"]                  # (an inf-norm over coordinates: not covariant under D, E)
        bad = lsc.rejected(lsc.criterion_b(res, fx, ri))
        today = _accepted_today(cfg, res, name, ri)
        print("%-14s rho %-3g lx[%d] (D = 2^%d) off by 1e-9: criterion B ratio %.3g, today's tolerance %s"
              % (name, rho, i, np.log2(T[1][i]), bad.get("lx", 0.0), "ACCEPTS" if today else "rejects"))
        assert set(bad) == {"lx"}, (name, rho, bad)


# ---- nonzero duals and the dual update (tests/test_gpu_dual_scales.py's yardsticks) ---------------------------------------------------
# the frozen solves: (feasible, sweeps, penalty_initial)
UPDATES = {"infeasible": (False, 1, lsc.RHO0), "feasible": (True, 1, lsc.RHO0), "two sweeps": (False, 2, lsc.RHO0), "clamp": (False, 1, lsc.RHO_CLAMP)}
_updates = {}


def update(name, which):
    if (name, which) not in _updates:
        feasible, sweeps, rho0 = UPDATES[which]
        _updates[(name, which)] = lsc.oracle_update(crc.config(name), lsc.update_state(name)[0], feasible, sweeps, rho0)
    return _updates[(name, which)]


def test_oracle_setters_round_trip():
    """oracle_ilqr_set_duals / _set_block_penalties against duals() / penalty(): stored as given, no projection, every block."""
    cfg = crc.config("lane_4_2")
    h = crc.make_oracle(cfg, 0)
    rng = np.random.default_rng(3)
    want = {}
    for k in range(crc.N + 1):
        for slot, j in enumerate(cfg.at(k)):
            assert (h.duals(k, slot) == 0.0).all() and h.penalty(k, slot) == 1.0
            want[(k, slot)] = rng.normal(size=cfg.blocks[j]["p"])              # (outside every dual cone as often as not)
            h.set_duals(k, slot, want[(k, slot)])
    h.set_block_penalty(37.5)
    for (k, slot), z in want.items():
        assert np.array_equal(h.duals(k, slot), z) and h.penalty(k, slot) == 37.5
    assert h.L.oracle_ilqr_set_duals(h.h, 0, 2, want[(0, 0)].ctypes.data) == -1 and h.L.oracle_ilqr_set_duals(h.h, crc.N + 1, 0, want[(0, 0)].ctypes.data) == -1
    with pytest.raises(AssertionError):
        h.set_duals(0, 0, np.zeros(7))


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_set_state_equals_carried_state_on_the_oracle(name):
    """S1 written through the setters onto a fresh handle gives the phases of the handle whose solve left it, bit for bit."""
    got, ref = lsc.oracle_dual_phases(crc.config(name), lsc.dual_state(name)), crc.nonzero_dual_reference(name)["phases"]
    for q in lsc.QUANTITIES:
        assert np.array_equal(got[q], np.stack([np.asarray(r[q], dtype=np.float64) for r in ref])), (name, q)


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_update_state_reaches_every_region(name):
    """S2: over batch and horizon the update's ze = z - rho0 c(rollout) takes every region of every cone block and both activities of
    every orthant block, none closer than 1e-6 of its own size to a boundary (also at the clamp run's penalty); an orthant block has
    duals partly zero before the update and partly zero after it; every problem is infeasible."""
    cfg = crc.config(name)
    st, steered = lsc.update_state(name)
    print(name, "cone duals steered:", steered)
    for rho in (lsc.RHO0, lsc.RHO_CLAMP):
        assert lsc.ze_margin(cfg, st, rho) >= lsc.MARGIN_ZE
    assert lsc.covered(cfg, lsc.coverage(cfg, st, lsc.RHO0)), lsc.coverage(cfg, st, lsc.RHO0)
    after = update(name, "infeasible")["z"]
    assert all(np.isfinite(a).all() for a in after.values()) and any((a != 0.0).any() for a in after.values())
    mixed = lambda a: bool(((a == 0.0).any(axis=-1) & (a != 0.0).any(axis=-1)).any())
    orth = [bl["name"] for bl in cfg.blocks if bl["kind"] == "orth"]
    assert all(mixed(st["z"][nm]) and mixed(after[nm]) for nm in orth)
    # rows that were inactive with a nonzero dual: the update has to project them to zero
    assert all(((st["z"][nm] != 0.0) & (after[nm] == 0.0)).any() for nm in orth)


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_oracle_is_covariant_at_nonzero_duals_and_through_the_update(name):
    """back(oracle(T cfg, T state)) == oracle(cfg, state) bit for bit: the phases at S1; from S2 the update alone, with the penalty
    update, with the clamp, and the two-sweep run (its second sweep's K, d, P, p and the duals after the second update)."""
    cfg = crc.config(name)
    s1, (s2, _) = lsc.dual_state(name), lsc.update_state(name)
    base = lsc.oracle_dual_phases(cfg, s1)
    for which, (feasible, sweeps, rho0) in UPDATES.items():
        r = update(name, which)
        assert (r["status"] == (0 if feasible else 2)).all() and (r["iterations"] == (sweeps if feasible else sweeps + 1)).all() and (r["alpha"] == 0.0).all()
        assert (r["rho"] == (rho0 if feasible else min(rho0 * 10.0 ** sweeps, lsc.PENALTY_MAX))).all()
        assert np.array_equal(r["x"], s2["x"]) and np.array_equal(r["u"], s2["u"])          # alpha = 0: the trajectory is the rollout
    for T in lsc.transforms(name):
        out = lsc.transform(cfg, *T)
        got = lsc.back(lsc.oracle_dual_phases(out, lsc.transform_state(cfg, out, s1)), *T)
        assert not lsc.differing(got, base, lsc.covariant_keys(T)), (name, T[0])
        s2T = lsc.transform_state(cfg, out, s2, lsc.RHO0)
        for which, (feasible, sweeps, rho0) in UPDATES.items():
            raw = lsc.oracle_update(out, s2T, feasible, sweeps, rho0)
            assert (raw["rho"] == update(name, which)["rho"] * out.scale).all()
            assert not lsc.differing_update(lsc.back(raw, *T), update(name, which), sweep=True), (name, T[0], which)


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_a_scale_that_is_no_power_of_four_moves_the_second_sweep(name):
    """s = 2^7.  What is seen: the second sweep's K, d, P, p move in their last bits, and the duals after BOTH updates stay exact -- a
    projection is homogeneous, c is unit-free and the frozen trajectory never feels the gains.  With a real line search the gains
    reach the trajectory and the duals move too."""
    cfg = crc.config(name)
    T = lsc.identity(cfg)
    out = lsc.transform(cfg, *T, scale=2.0 ** 7)
    st = lsc.transform_state(cfg, out, lsc.update_state(name)[0], lsc.RHO0)
    diff = lsc.differing_update(lsc.back(lsc.oracle_update(out, st, False, 2), *T, scale=2.0 ** 7), update(name, "two sweeps"), sweep=True)
    print(name, "frozen, two sweeps", diff)
    assert set(diff) == set(lsc.SWEEP) and max(diff.values()) < 1e-9, diff
    ls = lsc.search_state(name)
    kw = dict(feasible=False, sweeps=1, rho0=lsc.RHO_LS, tolg=1e-8)
    diff = lsc.differing_update(lsc.back(lsc.oracle_update(out, lsc.transform_state(cfg, out, ls), **kw), *T, scale=2.0 ** 7), lsc.oracle_update(cfg, ls, **kw))
    print(name, "one sweep with a line search", diff)
    assert any(q.startswith("z:") for q in diff) and "x" in diff, diff


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_line_search_mask_is_within_its_cap(name):
    """The sweep with a real line search: the oracle accepts alpha = 1 in every unit system on all but at most 2 of the 7 problems, is
    covariant bit for bit on those, and the fixture holds that mask.  (Elsewhere cubicspline.c's absolute LS_TOL = 1e-6 on spline
    coefficients, which carry cost units, decides differently: the reference's own.)"""
    cfg, st = crc.config(name), lsc.search_state(name)
    fx = lsc.load_duals(name)
    for bi, backtracking in enumerate((False, True)):
        mask = lsc.search_mask(name, backtracking)
        assert np.array_equal(mask, fx["ls_mask"][bi].astype(bool)) and (~mask).sum() <= 2, (name, mask)
        kw = dict(feasible=False, sweeps=1, rho0=lsc.RHO_LS, tolg=1e-8, backtracking=backtracking)
        base = lsc.oracle_update(cfg, st, **kw)
        out_of = set()
        for T in lsc.transforms(name):
            out = lsc.transform(cfg, *T)
            got = lsc.back(lsc.oracle_update(out, lsc.transform_state(cfg, out, st), **kw), *T)
            assert not lsc.differing_update(got, base, sweep=True, problems=np.flatnonzero(mask)), (name, T[0])
            out_of |= {int(b) for b in np.flatnonzero(~mask) if lsc.differing_update(got, base, sweep=True, problems=[b])}
        print(name, "backtracking" if backtracking else "cubic", "left out", np.flatnonzero(~mask).tolist(), "of which not covariant", sorted(out_of))


_fixture_oracle = {}


def fixture_oracle(name):
    if name not in _fixture_oracle:
        _fixture_oracle[name] = lsc.oracle_of_fixture(crc.config(name), lsc.dual_state(name), lsc.update_state(name)[0])
    return _fixture_oracle[name]


def judge(cfg, fx, o):
    """Criterion B of an oracle_of_fixture-shaped result: {key: ratio} over the phases at S1 ("s1:<quantity>"), z+ ("z1:z_<kind>"), the
    second sweep ("sw2:<quantity>") and z++ ("z2:z_<kind>"); rho+ by equality ("rho1", "rho2": 0 or inf)."""
    r = {}
    e = lsc.errors(o["s1"], {q: fx["ref_s1_" + q] for q in lsc.QUANTITIES})
    r.update({"s1:" + q: v for q, v in lsc.ratios(e, lsc.dual_limits(fx, "s1")).items()})
    for i in (1, 2):
        e = lsc.dual_errors(cfg, o["z%d" % i], lsc.blocks_of(fx, cfg, "ref_z%d" % i))
        r.update({"z%d:%s" % (i, q): v for q, v in lsc.ratios(e, lsc.dual_limits(fx, "z%d" % i)).items()})
        r["rho%d" % i] = 0.0 if np.array_equal(o["rho%d" % i], fx["ref_rho%d" % i]) else np.inf
    e = lsc.sweep_errors(o["sw2"], {q: fx["ref_sw2_" + q] for q in lsc.SWEEP})
    r.update({"sw2:" + q: v for q, v in lsc.ratios(e, lsc.dual_limits(fx, "sw2")).items()})
    return r


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_dual_fixtures_are_what_their_inputs_produce(name):
    cfg = crc.config(name)
    fx, d = lsc.load_duals(name), lsc.dual_inputs(name)
    arrays = lsc.dual_input_arrays(cfg, d)
    assert checksum(dict(lsc.inputs(cfg), **arrays)) == fx["sum"]
    for key, a in arrays.items():
        assert np.array_equal(a, fx[key]), key
    assert fx["flips_s1"] == 0 and fx["flips_up"] == 0          # the frozen branches are the ones extended precision takes
    for key, a in lsc.dual_ecpu(cfg, d, fx).items():
        assert np.array_equal(a, fx[key]), (key, a, fx[key])
        assert a.max() < 1e-12
    o = fixture_oracle(name)
    assert not lsc.rejected(judge(cfg, fx, o))
    # rho+ by equality, the clamped one included; an exactly zero reference entry is an exact zero
    assert (fx["ref_rho1"] == lsc.PENALTY_SCALING * lsc.RHO0).all() and (fx["ref_rho2"] == lsc.PENALTY_SCALING ** 2 * lsc.RHO0).all()
    assert (update(name, "clamp")["rho"] == lsc.PENALTY_MAX).all() and (update(name, "feasible")["rho"] == lsc.RHO0).all()
    for i in (1, 2):
        for nm, ref in lsc.blocks_of(fx, cfg, "ref_z%d" % i).items():
            assert np.isfinite(ref).all() and (o["z%d" % i][nm][ref == 0.0] == 0.0).all(), (name, nm)
    assert np.array_equal(update(name, "feasible")["z"][cfg.blocks[0]["name"]], o["z1"][cfg.blocks[0]["name"]])      # (z+ does not depend on the penalty update)


def _accepted_by_tol_new(cfg, z, want):
    """tests/test_gpu_cone_regions.py's comparison of duals with the oracle's: 1e-12 of max(1, block)."""
    return all(np.abs(z[nm][b, k] - want[nm][b, k]).max() / max(1.0, np.abs(want[nm][b, k]).max()) <= regions.TOL_NEW["duals"]
               for nm in want for b in range(BATCH) for k in range(want[nm].shape[1]))


def _one_block(z, cfg, kind, spoil, largest):
    """z with ONE (problem, knot point) block of `kind` spoilt: the one whose largest entry is the largest, or the smallest that is not zero."""
    out = {nm: a.copy() for nm, a in z.items()}
    size = {nm: np.abs(z[nm]).max(axis=-1) for nm in (bl["name"] for bl in cfg.blocks if bl["kind"] == kind)}
    size = {nm: s if largest else np.where(s > 0.0, s, np.inf) for nm, s in size.items()}
    nm = (max if largest else min)(size, key=lambda nm: (size[nm].max() if largest else size[nm].min()))
    b, k = np.unravel_index(size[nm].argmax() if largest else size[nm].argmin(), size[nm].shape)
    out[nm][b, k] = spoil(z[nm][b, k])
    assert not np.array_equal(out[nm][b, k], z[nm][b, k])
    return out, float(np.abs(z[nm][b, k]).max())


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_criterion_b_rejects_a_spoilt_update(name):
    """From the oracle alone: one dual block of z+ rounded to float32 and back, or times 1 + 1e-9; an update that leaves the duals of
    inactive orthant rows at their old values; the update taken with rho+ for rho.  Criterion B rejects the kinds of block that were
    touched and nothing else.  Printed beside each: whether TOL_NEW["duals"] = 1e-12 of max(1, block) would have accepted it."""
    cfg = crc.config(name)
    fx, o = lsc.load_duals(name), fixture_oracle(name)
    st = lsc.update_state(name)[0]
    kinds = [kind for kind in lsc.KINDS if any(bl["kind"] == kind for bl in cfg.blocks)]
    cases = []
    for how, spoil in SPOILT.items():
        for kind in kinds:
            for largest in (True, False):
                z, size = _one_block(o["z1"], cfg, kind, spoil, largest)
                cases.append(("%s block of size %.1e %s" % (kind, size, how), z, {kind}))
    if "orth" in kinds:
        kept = {nm: a.copy() for nm, a in o["z1"].items()}
        for bl in cfg.blocks:
            if bl["kind"] == "orth":
                kept[bl["name"]] = np.where(o["z1"][bl["name"]] == 0.0, st["z"][bl["name"]], o["z1"][bl["name"]])
        cases.append(("inactive rows keep their duals", kept, {"orth"}))
    late = lsc.oracle_update(cfg, st, True, 1, lsc.PENALTY_SCALING * lsc.RHO0)["z"]
    cases.append(("rho+ for rho", late, set(kinds)))
    assert _accepted_by_tol_new(cfg, o["z1"], o["z1"])
    for how, z, touched in cases:
        bad = lsc.rejected(judge(cfg, fx, dict(o, z1=z)))
        today = _accepted_by_tol_new(cfg, z, o["z1"])
        print("%-14s %-36s: criterion B ratios %s, today's tolerance %s" % (name, how, {q: "%.3g" % r for q, r in bad.items()}, "ACCEPTS" if today else "rejects"))
        assert set(bad) == {"z1:z_" + kind for kind in touched}, (name, how, bad)


def test_extended_precision_update_recomputed():
    pytest.importorskip("mpmath")
    gen = _maker()
    for name, b in (("lane_6_3", 2), ("auto32_rows", 5)):
        cfg = crc.config(name)
        fx, d = lsc.load_duals(name), lsc.dual_inputs(name)
        got, flips = gen.mp_phases(cfg, b, lsc.RHO0, None, 60, state=d["s2"], update=(d["tab_u1"], d["tab_u2"]))
        assert flips == 0
        for bl in cfg.blocks:
            for i in (1, 2):
                assert np.array_equal(got["z%d:%s" % (i, bl["name"])], fx["ref_z%d_%s" % (i, bl["name"])][b]), (name, bl["name"], i)
        for q in ("K", "d"):
            assert np.array_equal(got[q], fx["ref_sw2_" + q][b]), (name, q)
        got, flips = gen.mp_phases(cfg, b, d["s1"]["rho"][b], d["tab_s1"], 60, state=d["s1"])
        assert flips == 0
        for q in ("lx", "K", "dphi", "feas", "stat"):
            assert np.array_equal(np.asarray(got[q]), fx["ref_s1_" + q][b]), (name, q)


def _maker():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_loop_phase_fixtures", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                          "golden", "make_loop_phase_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_extended_precision_result_recomputed():
    pytest.importorskip("mpmath")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_loop_phase_fixtures", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                          "golden", "make_loop_phase_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for name, ri, b in (("lane_6_3", 1, 2), ("tile_dense", 0, 5)):
        cfg = crc.config(name)
        got, flips = gen.mp_phases(cfg, b, RHOS[ri], lsc.class_tables(cfg, RHOS[ri]), 60)
        ref = lsc.reference(lsc.load(name), ri)
        assert flips == 0
        for q in lsc.QUANTITIES:
            assert np.array_equal(np.asarray(got[q]), ref[q][b]), (name, q)
