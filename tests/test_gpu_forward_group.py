"""Plan MFMA16, fp64: the forward sweep with one workgroup per 16 adjacent problems (kernels/tvlqr_mfma16_fwd_group.hip) against the
wave-per-problem kernel it replaces on whole groups (ALTRO_HIP_FORM_FORWARD_WAVE keeps that one) -- bit for bit -- and against the
oracle's forward pass.  Horizons below, at and above the ring depth (2); one group (seven XCDs empty), three groups, nine groups
(ragged eighths); the (12, 4) tile and a zero-padded shape; with and without the affine term."""
import numpy as np
import pytest

import altro_amd
from tests import problems
from tests.test_gpu_parity import relerr, run_oracle

pytestmark = pytest.mark.gpu

# what tests/test_gpu_parity.py asserts of x, u, y on this plan (test_mfma16_random; the file names no constant to import)
PARITY_RTOL = 1e-9


def _handle(pr, forms, **kw):
    batch = pr["A"].shape[0]
    bt = altro_amd.Batch(pr["N"], pr["n"], pr["m"], batch, **kw)
    if forms:
        bt.set_forms(forms)
    bt.set_dynamics(pr["A"], pr["B"], pr.get("f"))
    bt.set_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    bt.set_initial_state(pr["x0"])
    return bt


@pytest.mark.parametrize("with_f", [True, False])
@pytest.mark.parametrize("n,m", [(12, 4), (7, 2)])
@pytest.mark.parametrize("batch", [16, 48, 144])
@pytest.mark.parametrize("N", [1, 2, 3, 7])
def test_group_forward_equals_wave_forward_and_oracle(N, batch, n, m, with_f):
    pr = problems.random_ltv(batch, N, n, m)
    ref_pr = dict(pr)
    if not with_f:
        pr["f"] = None
        ref_pr["f"] = np.zeros((batch, N, n))
    grp = _handle(pr, 0)
    wav = _handle(pr, altro_amd.FORM_FORWARD_WAVE)
    try:
        assert grp.plan == altro_amd.PLAN_MFMA16 and wav.plan == altro_amd.PLAN_MFMA16
        grp.sweep(); wav.sweep()
        assert (grp.get("status") == -1).all() and (wav.get("status") == -1).all()
        assert grp.profile_get(1)[2] == "mfma16_forward_group_kernel"
        assert wav.profile_get(1)[2] == "mfma16_forward_kernel"
        ref = run_oracle(ref_pr)
        for k in ("x", "u", "y"):
            g, w = grp.get(k), wav.get(k)
            assert g.shape == ref[k].shape
            assert np.array_equal(g, w), (k, float(np.abs(g - w).max()))
            assert relerr(g, ref[k]) < PARITY_RTOL, (k, relerr(g, ref[k]))
    finally:
        grp.close(); wav.close()


def test_forward_routing():
    """Whole groups of 16 in fp64 run the group kernel; a batch that is not a multiple of 16, a handle that stores fp32 and a handle
    with FORM_FORWARD_WAVE keep the wave-per-problem kernel."""
    cases = [(16, altro_amd.F64, 0, "mfma16_forward_group_kernel"),
             (17, altro_amd.F64, 0, "mfma16_forward_kernel"),
             (16, altro_amd.F32, 0, "mfma16_forward_kernel"),
             (16, altro_amd.F64, altro_amd.FORM_FORWARD_WAVE, "mfma16_forward_kernel")]
    for batch, dtype, forms, name in cases:
        pr = problems.random_ltv(batch, 4, 12, 4)
        bt = _handle(pr, forms, dtype=dtype)
        try:
            assert bt.plan == altro_amd.PLAN_MFMA16
            bt.profile(True)
            bt.sweep()
            launches, _, got = bt.profile_get(1)
            assert got == name, (batch, dtype, forms, got)
            assert launches == 1, (batch, dtype, forms, launches)     # slot 1 stays one launch per sweep
            assert (bt.get("status") == -1).all() and np.isfinite(bt.get("x")).all()
        finally:
            bt.close()
