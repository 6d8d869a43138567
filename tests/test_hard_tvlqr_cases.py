"""The hard TVLQR families and their extended-precision fixtures (tests/hard_cases.py, tests/golden/hard_tvlqr_<n>x<m>.npz), pinned on
the CPU: the regenerated inputs are the ones the fixtures were made from, the oracle's own error against the extended-precision result
is what the fixtures say, every family is as hard as it declares, and -- the finding the second yardstick exists for -- on the unstable
and collinear families the double-precision oracle is the inaccurate party: a numpy double recursion that symmetrises the carried
cost-to-go is an order of magnitude closer to the extended-precision result."""
import numpy as np
import pytest

from tests import hard_cases as hc
from tests.golden_cases import checksum

QI = {k: i for i, k in enumerate(hc.QUANTITIES)}


@pytest.fixture(scope="module", params=hc.SHAPES, ids=lambda s: "%dx%d" % s)
def shape_fix(request):
    n, m = request.param
    return n, m, hc.load(n, m)


def test_inputs_and_oracle_error_are_the_fixtures(shape_fix):
    n, m, fx = shape_fix
    for fam in hc.FAMILIES:
        for which in "ds":
            pr = hc.problem(fam, n, m, which)
            assert checksum(pr) == fx["sum_%s_%s" % (fam, which)], (fam, which)
            key = "ref_%s_%s" % (fam, which)
            if key not in fx:
                assert which == "s" and (n, m) not in hc.TILE_SHAPES
                continue
            ref = hc.unpack(fx[key], n, m)
            D = hc.scale_vector(fam, n, hc.level(fam, which, n, m))
            e = hc.errors(hc.at_knots(hc.run_oracle(pr), n), ref, n, m, D)
            assert np.array_equal(np.array([e[k] for k in hc.QUANTITIES]), fx["e64_%s_%s" % (fam, which)]), (fam, which, e)


def test_every_family_sits_in_its_band(shape_fix):
    n, m, fx = shape_fix
    for fam in hc.FAMILIES:
        lo, hi = hc.band(fam, n, m)
        eK = fx["e64_%s_d" % fam][QI["K"]]
        assert lo <= eK < hi, (fam, eK)
        assert np.isfinite(fx["ref_%s_d" % fam]).all()
    P = hc.unpack(fx["ref_scales_d"], n, m)["P"]
    assert np.abs(P).max() > 1e6
    if (n, m) in hc.TILE_SHAPES:
        for fam in hc.FAMILIES:
            e32 = fx["e32_%s_s" % fam]
            assert np.isfinite(e32).all() and e32[QI["K"]] < 1e-2, (fam, e32)       # the float32 recursion factors everywhere
            if hc.level(fam, "s", n, m) != hc.level(fam, "d", n, m):
                assert 1e-5 <= e32[QI["K"]], (fam, e32)


def test_failure_cases_stay_away_from_the_boundary(shape_fix):
    n, m, fx = shape_fix
    for fam in hc.FAMILIES:
        shift, fail_margin, ok_margin = fx["fail_%s" % fam][:3]
        assert fail_margin < -1e-3 and ok_margin > 1e-6, (fam, fail_margin, ok_margin)
        assert np.log2(shift) == np.round(np.log2(shift))
        pr = hc.with_failure(hc.problem(fam, n, m, "s"), shift)
        st = hc.run_oracle(pr)["status"].tolist()
        assert st == [hc.FAIL_KNOT if b == hc.FAIL_PROBLEM else -1 for b in range(hc.BATCH)], (fam, st)


def test_symmetrised_double_recursion_beats_the_oracle():
    """The finding these fixtures exist for: where the problems are hard the oracle (the reference's recursion, which does
    not symmetrise the carried cost-to-go) is itself 10x or more further from the extended-precision result than a plain numpy double
    recursion that does.  At (12, 4), the shape the finding was made at, on the collinear family; and as the median over the shapes with
    more than one input on both families (single shapes of the unstable family scatter between 7x and 58x)."""
    ratio = {fam: {} for fam in ("unstable", "collinear")}
    for n, m in hc.SHAPES:
        if m == 1:
            continue
        fx = hc.load(n, m)
        for fam in ratio:
            pr = hc.problem(fam, n, m, "d")
            ref = hc.unpack(fx["ref_%s_d" % fam], n, m)
            e = hc.errors(hc.at_knots(hc.riccati_numpy(pr, np.float64, symmetrise=True), n), ref, n, m)
            ratio[fam][(n, m)] = fx["e64_%s_d" % fam][QI["K"]] / e["K"]
    print(ratio)
    assert ratio["collinear"][(12, 4)] >= 10.0
    for fam in ratio:
        assert np.median(list(ratio[fam].values())) >= 10.0, (fam, ratio[fam])
        assert min(ratio[fam].values()) > 1.0, (fam, ratio[fam])


def test_blockerr_has_no_floor():
    ref = np.zeros((1, 2, 3)); ref[0, 0] = [1e-6, 2e-6, -4e-6]
    a = ref.copy(); a[0, 0, 1] += 4e-9
    assert abs(hc.blockerr(a, ref) - 1e-3) < 1e-12                     # 0.1 % of a block of size 4e-6: relerr's floor of 1 hides it
    a[0, 1, 2] = 1e-300
    assert hc.blockerr(a, ref) == float("inf")                         # an exactly zero block must be exactly zero
    D = np.array([1e3, 1.0, 1e-3])
    assert abs(hc.blockerr(a[:, :1], ref[:, :1], (D,)) - 4e-9 / 1e-3) < 1e-9     # in scaled coordinates the first entry sets the size


@pytest.mark.parametrize("fam", hc.FAMILIES)
def test_extended_precision_result_recomputed(fam):
    pytest.importorskip("mpmath")
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("make_hard_tvlqr_fixtures", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                          "golden", "make_hard_tvlqr_fixtures.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    n, m, b = 12, 4, 2
    pr = hc.problem(fam, n, m, "d")
    got, _, _ = gen.mp_solve(pr, 60, problems_=[b])
    ref = hc.unpack(hc.load(n, m)["ref_%s_d" % fam], n, m)
    cut = hc.at_knots(got, n)
    for k in hc.QUANTITIES:
        assert np.array_equal(cut[k][b], ref[k][b]), (fam, k)
