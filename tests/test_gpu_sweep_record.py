"""altro_hip_profile_get names, and altro_hip_sweep_variant describes, the kernel of the handle's LAST launch of the slot (the route the
launcher was given and kept: altro_amd/csrc/sweep_route.h) -- not what the handle's settings would pick at the time of the query.  Two
settings that change the choice are changed between a launch and the query: the MFMA16 sweep forms, and a plan-MFMA32 handle's cost
from dense to diagonal."""
import numpy as np
import pytest

import altro_amd
from tests import problems

pytestmark = pytest.mark.gpu


def _handle(pr, **kw):
    bt = altro_amd.Batch(pr["N"], pr["n"], pr["m"], pr["A"].shape[0], **kw)
    bt.set_dynamics(pr["A"], pr["B"], pr["f"])
    bt.set_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    bt.set_initial_state(pr["x0"])
    return bt


def test_forms_set_after_a_group_sweep_do_not_rename_it():
    pr = problems.random_ltv(16, 2, 12, 4)
    bt = _handle(pr)
    try:
        assert bt.plan == altro_amd.PLAN_MFMA16
        group = ("mfma16_backward_group_kernel", "mfma16_forward_group_kernel")
        bt.sweep()
        assert (bt.profile_get(0)[2], bt.profile_get(1)[2]) == group and bt.sweep_variant(0) == altro_amd.SWEEP_GROUP
        first = {k: bt.get(k) for k in ("x", "u", "K")}
        bt.set_forms(altro_amd.FORM_FORWARD_WAVE | altro_amd.FORM_BACKWARD_WAVE)
        assert (bt.profile_get(0)[2], bt.profile_get(1)[2]) == group, (bt.profile_get(0)[2], bt.profile_get(1)[2])
        assert bt.sweep_variant(0) == altro_amd.SWEEP_GROUP
        bt.sweep()
        assert (bt.profile_get(0)[2], bt.profile_get(1)[2]) == ("mfma16_backward_kernel", "mfma16_forward_kernel")
        assert bt.sweep_variant(0) == 0 and bt.sweep_variant(1) == 0
        for k, v in first.items():
            assert np.array_equal(bt.get(k), v), k
    finally:
        bt.close()


def test_diagonal_cost_set_after_a_tile_sweep_does_not_rename_it():
    B, N, n, m = 5, 2, 13, 4
    pr = problems.random_ltv(B, N, n, m)
    Qd = np.ascontiguousarray(pr["Q"].reshape(B, N + 1, n, n).diagonal(axis1=2, axis2=3))
    Rd = np.ascontiguousarray(pr["R"].reshape(B, N, m, m).diagonal(axis1=2, axis2=3))
    dense = dict(pr)   # the diagonal cost, written out as dense blocks
    dense["Q"] = (Qd[..., :, None] * np.eye(n)).reshape(pr["Q"].shape)
    dense["R"] = (Rd[..., :, None] * np.eye(m)).reshape(pr["R"].shape)
    dense["H"] = np.zeros_like(pr["H"])
    bt = _handle(dense, plan=altro_amd.PLAN_MFMA32)
    try:
        assert bt.plan == altro_amd.PLAN_MFMA32
        bt.sweep()
        assert bt.profile_get(0)[2] == "tile32_backward_kernel" and bt.profile_get(1)[2] == "tile32_forward_kernel"
        bt.set_cost(Qd, Rd, None, pr["q"], pr["r"], is_diag=True)
        assert bt.profile_get(0)[2] == "tile32_backward_kernel", bt.profile_get(0)[2]
        bt.sweep()
        assert bt.profile_get(0)[2] == "generic_backward_kernel" and bt.sweep_variant(0) == 0
        assert bt.profile_get(1)[2] == "tile32_forward_kernel"
        assert (bt.get("status") == -1).all()
    finally:
        bt.close()
