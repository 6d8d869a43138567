"""Where the iLQR loop's setters put a field is where its getters look (altro_amd/csrc/loop_fields.h): a round trip through the real
handle on every plan and element type.  set_state_guess / set_input_guess write the CANDIDATE trajectory, accept() -- the only kernel
involved, a copy -- makes it the nominal one, get_nominal / get_knot read that back.  The values 1000 b + 10 k + i + 0.5 are exact in
fp32, so the expectation is equality: with the value itself on fp64 handles, with float32(value) on fp32 handles.  With a zero stride
the setter takes ONE block and the expectation is its broadcast over the knot points / the batch.

Every plan / element type pair takes every call of the sequence: none returns ALTRO_HIP_ERR_UNSUPPORTED (UNSUPPORTED below is empty;
a pair listed there would have to fail with exactly that code at exactly that call)."""
import re

import numpy as np
import pytest

import altro_amd

pytestmark = pytest.mark.gpu

BATCH, N = 3, 4
ERR_UNSUPPORTED = -3
RAGGED_NX, RAGGED_NU = [3, 5, 2, 4, 3], [2, 1, 3, 2]

# name -> (plan, n, m)
UNIFORM = {"lane_4_2": (altro_amd.PLAN_LANE, 4, 2), "tile_12_4": (altro_amd.PLAN_MFMA16, 12, 4), "tile_7_3": (altro_amd.PLAN_MFMA16, 7, 3),
           "generic_5_2": (altro_amd.PLAN_GENERIC, 5, 2), "generic_13_4": (altro_amd.PLAN_GENERIC, 13, 4)}
STRIDES = [(0, 0), (1, 0), (0, 1), (1, 1)]
# (case, dtype) -> the call that answers ALTRO_HIP_ERR_UNSUPPORTED for that pair
UNSUPPORTED = {}


def value(b, k, i):
    return 1000.0 * b + 10.0 * k + i + 0.5


def field(nb, nk, width):
    """[nb][nk][width] of value(b, k, i)."""
    b, k, i = np.meshgrid(np.arange(nb), np.arange(nk), np.arange(width), indexing="ij")
    return value(b, k, i)


def stored(a, dtype):
    return a.astype(np.float32).astype(np.float64) if dtype == altro_amd.F32 else a


class Steps:
    """Runs the calls of one case in order; for a pair listed in UNSUPPORTED the listed call must fail with that code (and ends the case)."""

    def __init__(self, key):
        self.refused_at = UNSUPPORTED.get(key)
        self.ended = False

    def __call__(self, name, fn, *args, **kw):
        if self.ended:
            return None
        if name == self.refused_at:
            with pytest.raises(altro_amd.AltroHipError) as e:
                fn(*args, **kw)
            code = int(re.match(r"altro_hip error (-?\d+)", str(e.value)).group(1))
            assert code == ERR_UNSUPPORTED, str(e.value)
            self.ended = True
            return None
        return fn(*args, **kw)


@pytest.mark.parametrize("dtype", [altro_amd.F64, altro_amd.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("kz,bz", STRIDES, ids=["full", "k0", "b0", "k0b0"])
@pytest.mark.parametrize("case", sorted(UNIFORM))
def test_uniform_round_trip(case, kz, bz, dtype):
    plan, n, m = UNIFORM[case]
    step = Steps((case, dtype))
    bt = step("create", altro_amd.Batch, N, n, m, BATCH, dtype=dtype, plan=plan)
    if bt is None:
        return
    assert bt.plan == plan
    if plan == altro_amd.PLAN_LANE:
        step("set_model", bt.set_model, altro_amd.MODEL_BICYCLE, 0.1)
    else:
        A = np.tile(np.eye(n).reshape(1, 1, n * n), (BATCH, N, 1))
        step("set_dynamics", bt.set_dynamics, A, np.zeros((BATCH, N, n * m)))
    step("set_tracking_cost", bt.set_tracking_cost, np.ones((BATCH, N + 1, n)), np.ones((BATCH, N, m)), np.zeros((BATCH, N + 1, n)),
         np.zeros((BATCH, N, m)))
    step("set_initial_state", bt.set_initial_state, field(BATCH, 1, n)[:, 0])
    nb = 1 if bz else BATCH
    x_in, u_in = field(nb, 1 if kz else N + 1, n), field(nb, 1 if kz else N, m)
    step("set_state_guess", bt.set_state_guess, x_in, k_stride_zero=kz, batch_stride_zero=bz)
    step("set_input_guess", bt.set_input_guess, u_in, k_stride_zero=kz, batch_stride_zero=bz)
    step("accept", bt.accept)
    x_want = stored(np.broadcast_to(x_in, (BATCH, N + 1, n)), dtype)
    u_want = stored(np.broadcast_to(u_in, (BATCH, N, m)), dtype)
    got = step("get_nominal", bt.get_nominal)
    if got is not None:
        assert np.array_equal(got[0], x_want), (got[0], x_want)
        assert np.array_equal(got[1], u_want), (got[1], u_want)
    for k in (0, 2, N):
        got = step("get_knot", bt.get_knot, k)
        if got is None:
            continue
        assert np.array_equal(got[0], x_want[:, k]), (k, got[0], x_want[:, k])
        if k < N:
            assert np.array_equal(got[1], u_want[:, k]), (k, got[1], u_want[:, k])
        else:
            assert got[1] is None
    assert step.ended == (step.refused_at is not None)
    bt.close()


@pytest.mark.parametrize("dtype", [altro_amd.F64, altro_amd.F32], ids=["f64", "f32"])
def test_per_knot_point_dimensions_round_trip(dtype):
    nx, nu = RAGGED_NX, RAGGED_NU
    sx, su = sum(nx), sum(nu)
    step = Steps(("dims", dtype))
    bt = step("create", altro_amd.Batch.with_dims, nx, nu, BATCH, dtype=dtype)
    if bt is None:
        return
    assert bt.plan == altro_amd.PLAN_GENERIC and bt.N == N
    A = np.zeros((BATCH, sum(nx[k + 1] * nx[k] for k in range(N))))
    Bm = np.zeros((BATCH, sum(nx[k + 1] * nu[k] for k in range(N))))
    step("set_dynamics", bt.set_dynamics, A, Bm)
    step("set_tracking_cost", bt.set_tracking_cost, np.ones((BATCH, sx)), np.ones((BATCH, su)), np.zeros((BATCH, sx)), np.zeros((BATCH, su)))
    step("set_initial_state", bt.set_initial_state, field(BATCH, 1, nx[0])[:, 0])
    # packed [batch][k][block_k]: knot point k contributes value(b, k, 0 .. nx[k] - 1)
    x_in = np.concatenate([field(BATCH, N + 1, nx[k])[:, k] for k in range(N + 1)], axis=1)
    u_in = np.concatenate([field(BATCH, N, nu[k])[:, k] for k in range(N)], axis=1)
    step("set_state_guess", bt.set_state_guess, x_in)
    step("set_input_guess", bt.set_input_guess, u_in)
    step("accept", bt.accept)
    got = step("get_nominal", bt.get_nominal)
    if got is not None:
        assert np.array_equal(got[0], stored(x_in, dtype)) and np.array_equal(got[1], stored(u_in, dtype)), got
    for k in (0, 2, N):
        got = step("get_knot", bt.get_knot, k)
        if got is None:
            continue
        assert np.array_equal(got[0], stored(field(BATCH, N + 1, nx[k])[:, k], dtype)), (k, got[0])
        if k < N:
            assert np.array_equal(got[1], stored(field(BATCH, N, nu[k])[:, k], dtype)), (k, got[1])
        else:
            assert got[1] is None
    assert step.ended == (step.refused_at is not None)
    bt.close()
