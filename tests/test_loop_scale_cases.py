"""The two yardsticks of tests/test_gpu_loop_scales.py, shown on the CPU from the oracle alone (tests/loop_scale_cases.py):

  A. the oracle's phases are covariant BIT FOR BIT under every change of units the device is run under -- and not under a cost scale
     that is no power of four, so the comparison can fail;
  B. the extended-precision fixtures (tests/golden/loop_phases_<config>.npz) are the ones their inputs produce, and the criterion
     blockerr <= 10 max(e_cpu, 1e-13) has teeth: one quantity of the oracle's own phases rounded to float32 and back, or off by 1e-9
     of its size, is rejected on every configuration, as is one coordinate of lx that is off by 1e-9 of its own size.  Beside each it
     is printed whether the tolerances of tests/test_gpu_cone_regions.py, the tightest phase-by-phase test there was, would have
     accepted it.  The outcome: rounded to float32 they reject lx, K, x, phi' and accept feasibility (14 of 14
     cases) and stationarity (8 of 14: plans LANE / MFMA16); off by 1e-9 they accept K, feasibility, stationarity (14 of 14) and
     phi', x, u (8 of 14)."""
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
