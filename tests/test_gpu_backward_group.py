"""Plan MFMA16, fp64: the backward sweep with one workgroup per 16 adjacent problems (kernels/tvlqr_mfma16_bwd_group.hip) against the
wave-per-problem kernel (ALTRO_HIP_FORM_BACKWARD_WAVE forces that one) -- bit for bit -- and against the oracle's backward pass.
Horizons below, at and above the depth of the LDS ring (2); one group (seven XCDs empty), three groups, nine groups (ragged
eighths); the (12, 4) tile and a zero-padded shape; with and without the affine term; no regularisation, one value, and values that
differ inside a group.  Failing problems in the first and last wave of a group and in two adjacent waves.  Which launches take which
kernel.  A whole constrained solve with and without the form bit."""
import numpy as np
import pytest

import altro_amd
from tests import hard_cases as hc
from tests import problems
from tests.test_gpu_parity import relerr, run_oracle

pytestmark = pytest.mark.gpu

# what tests/test_gpu_parity.py asserts of K, d, P, p, delta_V on this plan (test_mfma16_random; the file names no constant to import)
PARITY_RTOL = 1e-9
PARITY_ATOL_KD = 1e-8
WAVE = altro_amd.FORM_BACKWARD_WAVE
GROUP_NAME, WAVE_NAME = "mfma16_backward_group_kernel", "mfma16_backward_kernel"
OUT = ("K", "d", "P", "p", "delta_V", "status")


def _handle(pr, forms, **kw):
    batch = pr["A"].shape[0]
    bt = altro_amd.Batch(pr["N"], pr["n"], pr["m"], batch, **kw)
    if forms:
        bt.set_forms(forms)
    bt.set_dynamics(pr["A"], pr["B"], pr.get("f"))
    bt.set_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    bt.set_initial_state(pr["x0"])
    return bt


def _ran(bt, group):
    assert bt.profile_get(0)[2] == (GROUP_NAME if group else WAVE_NAME), bt.profile_get(0)[2]
    assert bt.sweep_variant(0) == (altro_amd.SWEEP_GROUP if group else 0), bt.sweep_variant(0)


def _same(grp, wav, what):
    for k in OUT:
        g, w = grp.get(k), wav.get(k)
        assert np.array_equal(g, w, equal_nan=True), (what, k)


@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("n,m", [(12, 4), (7, 2)])
@pytest.mark.parametrize("batch", [16, 48, 144])
@pytest.mark.parametrize("N", [1, 2, 3, 7])
def test_group_backward_equals_wave_backward_and_oracle(N, batch, n, m, with_f):
    pr = problems.random_ltv(batch, N, n, m)
    ref_pr = dict(pr)
    if not with_f:
        pr["f"] = None
        ref_pr["f"] = np.zeros((batch, N, n))
    grp = _handle(pr, 0)
    wav = _handle(pr, WAVE)
    reg_a, reg_b = 0.0, 0.37
    reg_pp = np.where(np.arange(batch) % 3 == 1, reg_b, reg_a)      # differs inside every group
    try:
        assert grp.plan == altro_amd.PLAN_MFMA16 and wav.plan == altro_amd.PLAN_MFMA16
        refs = {}
        for reg in (reg_a, reg_b):
            grp.backward(reg); wav.backward(reg)
            _ran(grp, True); _ran(wav, False)
            assert (grp.get("status") == -1).all()
            _same(grp, wav, reg)
            ref = refs[reg] = run_oracle(ref_pr, reg=reg)
            assert np.abs(grp.get("K") - ref["K"]).max() < PARITY_ATOL_KD and np.abs(grp.get("d") - ref["d"]).max() < PARITY_ATOL_KD
            for k in ("K", "d", "P", "p"):
                assert grp.get(k).shape == ref[k].shape
                assert relerr(grp.get(k), ref[k]) < PARITY_RTOL, (reg, k, relerr(grp.get(k), ref[k]))
            assert relerr(grp.get("delta_V"), ref["dV"]) < PARITY_RTOL
        grp.backward_per_problem(reg_pp); wav.backward_per_problem(reg_pp)
        _ran(grp, True); _ran(wav, False)
        _same(grp, wav, "reg_pp")
        pick = reg_pp == reg_b
        for k in ("K", "d", "P", "p", "dV"):
            ref = np.where(pick.reshape((-1,) + (1,) * (refs[reg_a][k].ndim - 1)), refs[reg_b][k], refs[reg_a][k])
            got = grp.get("delta_V" if k == "dV" else k)
            assert relerr(got, ref) < PARITY_RTOL, ("reg_pp", k, relerr(got, ref))
    finally:
        grp.close(); wav.close()


def test_failing_problems_in_a_group():
    """Three groups of 12 x 4 problems, N = 24 (tests/hard_cases.py); problems whose Cholesky fails at the interior knot point FAIL_KNOT
    sit in wave 0 and wave 15 of the first group and in waves 5 and 6 of the second; the third group is healthy.  Both handles hold the
    same earlier sweep (the same problems without the failure).  The status is the failing index, every output equals the wave kernel's,
    and what lies below the failing knot point is the earlier sweep's, untouched."""
    n, m = 12, 4
    fx = hc.load(n, m)
    fams = ("collinear", "unstable", "cross", "collinear")
    slots = (0, 15, 16 + 5, 16 + 6)
    ben = hc.problem("benign", n, m, "s")
    nb = ben["A"].shape[0]
    parts_ok, parts_bad = [], []
    for i in range(48):
        if i in slots:
            fam = fams[slots.index(i)]
            base = hc.problem(fam, n, m, "s")
            parts_ok.append(hc.take(base, [hc.FAIL_PROBLEM]))
            parts_bad.append(hc.take(hc.with_failure(base, fx["fail_%s" % fam][0]), [hc.FAIL_PROBLEM]))
        else:
            parts_ok.append(hc.take(ben, [i % nb]))
            parts_bad.append(parts_ok[-1])
    ok, bad = hc.stack(parts_ok), hc.stack(parts_bad)
    ok["N"] = bad["N"] = hc.N
    want = np.array([hc.FAIL_KNOT if i in slots else -1 for i in range(48)])
    grp, wav = _handle(ok, 0), _handle(ok, WAVE)
    try:
        grp.backward(); wav.backward()
        assert (grp.get("status") == -1).all()
        _same(grp, wav, "earlier sweep")
        before = {k: grp.get(k) for k in ("K", "d", "P", "p")}
        for bt in (grp, wav):
            bt.set_cost(bad["Q"], bad["R"], bad["H"], bad["q"], bad["r"])
            bt.backward()
        _ran(grp, True); _ran(wav, False)
        assert grp.get("status").tolist() == want.tolist()
        _same(grp, wav, "failing")
        k = hc.FAIL_KNOT
        for i in slots:
            for q in ("K", "d"):                     # K_k = Qux, d_k = -Qu left unsolved at k; below it nothing is written
                assert np.array_equal(grp.get(q)[i, :k], before[q][i, :k]), (i, q)
                assert not np.array_equal(grp.get(q)[i, k], before[q][i, k]), (i, q)
            for q in ("P", "p"):                     # P_k, p_k untouched at k and below
                assert np.array_equal(grp.get(q)[i, :k + 1], before[q][i, :k + 1]), (i, q)
    finally:
        grp.close(); wav.close()


def test_backward_routing():
    """Whole groups of 16 in fp64 with no mask run the group kernel; a batch that is not a multiple of 16, a handle that stores fp32, a
    handle that stores the Q blocks, a handle with FORM_BACKWARD_WAVE, and the masked launches of a solve keep the wave-per-problem
    kernel.  Slot 0 sees one launch per sweep."""
    cases = [(16, altro_amd.F64, 0, 0, True), (32, altro_amd.F64, 0, 0, True),
             (17, altro_amd.F64, 0, 0, False),
             (16, altro_amd.F32, 0, 0, False),
             (16, altro_amd.F64, altro_amd.STORE_QBLOCKS, 0, False),
             (16, altro_amd.F64, 0, WAVE, False)]
    for batch, dtype, flags, forms, group in cases:
        pr = problems.random_ltv(batch, 4, 12, 4)
        bt = _handle(pr, forms, dtype=dtype, flags=flags)
        try:
            assert bt.plan == altro_amd.PLAN_MFMA16
            bt.profile(True)
            bt.sweep()
            launches, _, got = bt.profile_get(0)
            assert got == (GROUP_NAME if group else WAVE_NAME), (batch, dtype, flags, forms, got)
            assert bt.sweep_variant(0) == (altro_amd.SWEEP_GROUP if group else 0), (batch, dtype, flags, forms)
            assert launches == 1, (batch, dtype, flags, forms, launches)
            assert (bt.get("status") == -1).all() and np.isfinite(bt.get("K")).all()
        finally:
            bt.close()


def _solve(forms):
    N, batch = 8, 16
    p = problems.ilqr12x4_problem(batch, N, True)
    bt = altro_amd.Batch(N, 12, 4, batch)
    assert bt.plan == altro_amd.PLAN_MFMA16
    if forms:
        bt.set_forms(forms)
    bt.set_dynamics(p["A"], p["B"], p["f"])
    bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
    bt.set_initial_state(p["x0"])
    bt.set_input_guess(p["u0"])
    for (k0, k1, cone, G, g) in problems.ilqr12x4_constraint_blocks(N):
        bt.add_linear_constraint(k0, k1, cone, G, g)
    res = bt.ilqr_solve(iterations_max=60, penalty_initial=1.0, penalty_scaling=10.0)
    x, u = bt.get_nominal()
    ran = bt.profile_get(0)[2], bt.sweep_variant(0)
    bt.close()
    return res, x, u, ran


def test_constrained_solve_with_and_without_the_form_bit():
    """A solve's backward sweeps carry the mask of the problems still running: they keep the wave-per-problem kernel whatever the form
    bit says, and the solve comes out the same."""
    res0, x0, u0, ran0 = _solve(0)
    res1, x1, u1, ran1 = _solve(WAVE)
    assert ran0 == (WAVE_NAME, 0) and ran1 == (WAVE_NAME, 0)
    assert res0["sweeps"] == res1["sweeps"] and res0["sweeps"] > 0
    for k in ("status", "iterations"):
        assert np.array_equal(res0[k], res1[k]), k
    assert np.array_equal(x0, x1) and np.array_equal(u0, u1)
