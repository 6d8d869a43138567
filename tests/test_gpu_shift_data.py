"""The problem data of a receding-horizon step, moved and rewritten in place: altro_hip_set_dynamics_range / _get_dynamics_knot /
_shift_dynamics (dynamics given as data) and altro_hip_shift_linear_costs, on every plan.

  1. round trips: what set_dynamics / set_dynamics_range store is what get_dynamics_knot returns, exactly (fp32: the value as a float), from
     host arrays and from torch device tensors; every knot point outside the written range keeps its bits;
  2. shift_dynamics against numpy, bit for bit, around the kernel's group depth and over batches that are no multiple of a wave;
  3. twin handles, dynamics: shifted + last knot point written == set whole, through the TVLQR sweeps on every plan and through the
     iLQR loop (merit, expansion, a constrained solve, the affine rounds' base) where the plan runs it on dynamics given as data;
  4. twin handles, linear costs: tracking cost shifted + update_linear_costs(N-1 .. N) == tracking cost of the shifted reference, and
     the same with the dense cost;
  5. five closed-loop MPC steps on the tile, the shifted handle against one built fresh at every step;
  6. errors and no-ops.
Every comparison is np.array_equal: the calls move or rewrite bits that the same kernels then read.  Where a test forms q = -Q xref on
the host next to altro_hip_set_tracking_cost doing the same, the data are dyadic rationals with few bits, so that every product and sum
is exact in whatever order (and with whatever contraction) either side evaluates it.
Shapes: those of tests/test_gpu_dual_warmstart.py (LANE (4, 2) batch 66 in both types, the (12, 4) tile batch 8, MFMA32 (13, 4), GENERIC
(14, 9) in both types), the padded tile shape (7, 3), a tile handle in fp32 and one with F32_PURE.
"""
import numpy as np
import pytest

import altro_amd
from tests import mpc_common as M
from tests import problems
from tests.test_gpu_dual_warmstart import SHAPES as DW

pytestmark = pytest.mark.gpu

INEQ = altro_amd.CONE_INEQUALITY
# name -> (plan, n, m, N, batch, dtype, flags)
CASES = {name: DW[name][:6] + (0,) for name in ("lane", "lane_f32", "tile", "mfma32", "generic", "generic_f32")}
CASES["tile_f32"] = (altro_amd.PLAN_MFMA16, 12, 4, 12, 8, altro_amd.F32, 0)
CASES["tile_pure"] = (altro_amd.PLAN_MFMA16, 12, 4, 12, 8, altro_amd.F32, altro_amd.F32_PURE)
CASES["tile_7_3"] = (altro_amd.PLAN_MFMA16, 7, 3, 12, 8, altro_amd.F64, 0)
LOOP_ON_DATA = ("tile", "tile_7_3", "mfma32", "generic")     # the iLQR loop on dynamics given as data, fp64


def handle(name, N=None, batch=None):
    plan, n, m, N0, batch0, dtype, flags = CASES[name]
    bt = altro_amd.Batch(N or N0, n, m, batch or batch0, dtype=dtype, plan=plan, flags=flags)
    assert bt.plan == plan, (name, bt.plan)
    return bt


def is_f32(name):
    return CASES[name][5] == altro_amd.F32


def stored(v, f32):
    return v.astype(np.float32).astype(np.float64) if f32 else v


def random_dyn(rng, nb, nk, n, m):
    """A [nb, nk, n*n], B [nb, nk, n*m], f [nb, nk, n], all 53 bits (fp32 rounds them)."""
    return rng.normal(size=(nb, nk, n * n)), rng.normal(size=(nb, nk, n * m)), rng.normal(size=(nb, nk, n))


def integer_dyn(batch, N, n, m):
    """Integers distinct over (array, problem, knot point, element) and below 2^24 (exact as floats)."""
    out, first = [], 1
    for blk in (n * n, n * m, n):
        out.append(first + np.arange(batch * N * blk, dtype=np.float64).reshape(batch, N, blk))
        first += batch * N * blk
    assert first < 2 ** 24
    return out


def check_dyn(bt, want, f32, tag):
    for k in range(bt.N):
        got = bt.get_dynamics_knot(k)
        for name, g, w in zip("ABf", got, want):
            assert np.array_equal(g, stored(w[:, k], f32)), (tag, name, k)


def shifted(v):
    """Knot points one forward along axis 1, the last one duplicated."""
    return np.concatenate([v[:, 1:], v[:, -1:]], axis=1)


# ---- 1. round trips -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_round_trip(name):
    import torch
    bt = handle(name)
    N, n, m, batch, f32 = bt.N, bt.n, bt.m, bt.batch, is_f32(name)
    rng = np.random.default_rng(3)
    want = [v.copy() for v in random_dyn(rng, batch, N, n, m)]
    bt.set_dynamics(*want)
    check_dyn(bt, want, f32, "set_dynamics")
    ranges = [(0, 0), (N - 1, N - 1), (N // 3, (2 * N) // 3), (0, N - 1)]

    def write(k0, k1, bz, with_f, device):
        nk = k1 - k0 + 1
        new = list(random_dyn(rng, 1 if bz else batch, nk, n, m))
        if not with_f:
            new[2] = None
        args = [None if v is None else (torch.tensor(v, device="cuda", dtype=torch.float64) if device else v) for v in new]
        bt.set_dynamics_range(args[0], args[1], args[2], k0, k1, batch_stride_zero=bz)
        for w, v in zip(want, new):
            w[:, k0:k1 + 1] = 0.0 if v is None else v        # (bz: one problem's values broadcast over the batch)
        check_dyn(bt, want, f32, ("range", k0, k1, bz, with_f, device))

    for k0, k1 in ranges:
        for bz in (False, True):
            write(k0, k1, bz, True, False)
    write(1, N - 2, False, False, False)                     # f == NULL: zeros for the range, the rest of f stays
    bt.set_pointer_mode(True)
    for k0, k1 in ranges:
        for bz in (False, True):
            write(k0, k1, bz, True, True)
    write(0, N // 2, True, False, True)
    bt.set_pointer_mode(False)
    bt.close()


# ---- 2. shift against numpy ---------------------------------------------------------------------------------------------------------
# The kernel holds a group of knot points in flight -- 16 with single-element accesses (SHIFT_FIELD_DEPTH), 8 with 16-byte ones
# (SHIFT_FIELD_DEPTH_VEC) -- and a horizon of N makes N - 1 moves.  Depth 16: N = 16, 17 fill one group (15, 16 moves), 18 is the first
# horizon with a second group, 35 has three with a tail.  Depth 8: N = 9 fills one group, 10 starts the second, 17 fills two, 18 starts
# the third.  1 and 2 are the no-op and the single move.  Which depth a shape takes: LANE (4, 2) rows of 37 or 1 problems and plan
# GENERIC's blocks of odd size go element by element, the tile's records and LANE rows of 66 / 130 doubles by 16 bytes.
@pytest.mark.parametrize("name", ["lane", "lane_f32", "tile", "tile_f32", "tile_7_3", "generic", "generic_f32"])
def test_shift_against_numpy(name):
    _, n, m, _, _, _, _ = CASES[name]
    for N in (1, 2, 9, 10, 15, 16, 17, 18, 35):
        for batch in (1, 37, 66, 130):
            bt = handle(name, N, batch)
            want = integer_dyn(batch, N, n, m)
            bt.set_dynamics(*want)
            for _ in range(2):
                bt.shift_dynamics()
                want = [shifted(v) for v in want]
            check_dyn(bt, want, False, (N, batch))
            bt.close()


# ---- 3. twin handles, dynamics ------------------------------------------------------------------------------------------------------
def input_box(n, m):
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    return G


def same(a, b, tag):
    assert np.array_equal(a, b, equal_nan=True), tag


def compare_sweeps(a, b, tag):
    for bt in (a, b):
        bt.backward()
    for what in ("K", "d", "P", "p", "status"):
        same(a.get(what), b.get(what), (tag, what))
    assert (a.get("status") == altro_amd.TVLQR_SUCCESS).all(), tag
    for bt in (a, b):
        bt.forward_ltv()
    for what in ("x", "u", "y"):
        same(a.get(what), b.get(what), (tag, what))


def loop_phases(bt, alphas):
    bt.open_loop_rollout(); bt.accept(); bt.expand()
    exp = bt.get_expansion()
    bt.backward()
    phi, dphi = bt.merit(alphas)
    return list(exp) + [bt.get("K"), bt.get("d"), phi, dphi, bt.get("x"), bt.get("u")]


def compare_loop(a, b, tag, solve=True):
    alphas = np.linspace(0.1, 1.1, a.batch)
    for i, (got, want) in enumerate(zip(loop_phases(a, alphas), loop_phases(b, alphas))):
        assert np.isfinite(want).all(), (tag, "phase", i)
        same(got, want, (tag, "phase", i))
    if not solve:
        return
    res = [bt.ilqr_solve(iterations_max=25, use_backtracking=True) for bt in (a, b)]
    for key in ("status", "iterations", "dual_updates"):
        same(res[0][key], res[1][key], (tag, key))
    for got, want in zip(a.get_nominal(), b.get_nominal()):
        same(got, want, (tag, "solve"))


@pytest.mark.parametrize("name", list(CASES))
def test_twin_dynamics(name):
    a, b = handle(name), handle(name)
    N, n, m, batch = a.N, a.n, a.m, a.batch
    pr = problems.random_ltv(batch, N + 1, n, m)              # one knot point more than the horizon: the one that enters
    D = [pr[key][:, :N] for key in "ABf"]
    D2 = [pr[key][:, 1:N + 1] for key in "ABf"]
    new = [np.ascontiguousarray(pr[key][:, N:N + 1]) for key in "ABf"]
    cost = problems.random_ltv(batch, N, n, m)
    for bt in (a, b):
        bt.set_dynamics(*D)
        bt.set_cost(cost["Q"], cost["R"], cost["H"], cost["q"], cost["r"])
        bt.set_initial_state(cost["x0"])
    a.backward(); a.forward_ltv()                             # (the handle has run on the old data)
    a.shift_dynamics()
    a.set_dynamics_range(new[0], new[1], new[2], N - 1, N - 1)
    b.set_dynamics(*D2)
    check_dyn(a, D2, is_f32(name), "shifted")
    compare_sweeps(a, b, name)                                # (LANE, GENERIC: the cost blocks that share the records did not move)
    if name not in LOOP_ON_DATA:
        a.close(); b.close()
        return
    # through the iLQR loop: both handles start on D with the loop's state primed, then A shifts and B is set whole
    p = problems.ilqr12x4_problem(batch, N, True, n=n, m=m)
    for bt in (a, b):
        bt.set_dynamics(*D)
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.set_initial_state(p["x0"]); bt.set_input_guess(p["u0"])
        bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.backward()
        bt.merit(np.full(batch, 0.5))
    alphas = np.linspace(0.2, 1.0, batch)
    if name == "tile":                                        # the affine rounds' base belongs to the dynamics it was built on
        before = a.merit_affine(alphas)
        b.merit_affine(alphas)
    a.shift_dynamics()
    a.set_dynamics_range(new[0], new[1], new[2], N - 1, N - 1)
    b.set_dynamics(*D2)
    if name == "tile":
        after, want = a.merit_affine(alphas), b.merit_affine(alphas)
        same(after[0], want[0], "affine phi"); same(after[1], want[1], "affine dphi")
        assert not np.array_equal(after[0], before[0]), "the new dynamics change nothing: the round proves nothing"
    for bt in (a, b):
        assert bt.add_linear_constraint(0, N - 1, INEQ, input_box(n, m), np.full(2 * m, 0.15)) == 0
    compare_loop(a, b, name)
    a.close(); b.close()


# ---- 4. twin handles, linear costs --------------------------------------------------------------------------------------------------
def dyadic(v, bits):
    return np.round(v * 2.0 ** bits) / 2.0 ** bits


def loop_handle(name):
    """(handle, N, n, m, batch) ready for a cost: a LANE handle with the bicycle model, every other one with dynamics given as data."""
    if name.startswith("lane"):
        bt = altro_amd.Batch(12, M.n, M.m, 66, dtype=CASES[name][5])
        assert bt.plan == altro_amd.PLAN_LANE
        bt.set_model(altro_amd.MODEL_BICYCLE, M.H)
    else:
        bt = handle(name)
        p = problems.ilqr12x4_problem(bt.batch, bt.N, True, n=bt.n, m=bt.m)
        bt.set_dynamics(p["A"], p["B"], p["f"])
    return bt


def finish(bt, name):
    if name.startswith("lane"):
        x_ref, u_ref = problems.bicycle_reference(bt.N + 8)
        off = problems.uniform01((bt.batch, 4), 33) - 0.5
        bt.set_initial_state(x_ref[0] + off * np.array([0.2, 0.2, 0.04, 0.0]))
        bt.set_input_guess(np.array([u_ref[0][0], 0.0])[None, None], k_stride_zero=True, batch_stride_zero=True)
    else:
        p = problems.ilqr12x4_problem(bt.batch, bt.N, True, n=bt.n, m=bt.m)
        bt.set_initial_state(p["x0"]); bt.set_input_guess(p["u0"])


def tracking_data(name, N, n, m, batch):
    """Qd [batch, N+1, n] (uniform over the running knot points, another terminal weight), Rd [batch, N, m], and a reference of N + 2
    states and N + 1 inputs per problem -- all dyadic rationals with few bits."""
    if name.startswith("lane"):
        x_ref, u_ref = problems.bicycle_reference(N + 8)
        off = dyadic(problems.uniform01((batch, 1, n), 41) - 0.5, 6) * np.array([0.5, 0.5, 0.125, 0.0])
        xref = dyadic(x_ref[None, :N + 2], 6) + off
        uref = np.broadcast_to(dyadic(u_ref[None, :N + 1], 6), (batch, N + 1, m)).copy()
        Qrun, Qterm, Rrun = np.full(n, 2.0 ** -6), np.full(n, 2.0 ** -4), np.full(m, 2.0 ** -10)
    else:
        xref = dyadic(0.3 * problems.normal((batch, N + 2, n), 91), 4)
        uref = dyadic(0.1 * problems.normal((batch, N + 1, m), 92), 5)
        Qrun = 2.0 ** (np.arange(n) % 3 - 1.0); Qterm = 8.0 * Qrun; Rrun = 2.0 ** (-3.0 - np.arange(m) % 2)
    Qd = np.broadcast_to(Qrun, (batch, N + 1, n)).copy(); Qd[:, N] = Qterm
    Rd = np.broadcast_to(Rrun, (batch, N, m)).copy()
    assert (np.ptp(xref, axis=0) > 0).any() and (np.ptp(xref, axis=1) > 0).any()      # per problem, per knot point
    return Qd, Rd, xref, uref


@pytest.mark.parametrize("name", ["lane", "lane_f32", "tile", "tile_f32", "tile_7_3", "mfma32", "generic"])
def test_twin_tracking_cost(name):
    a, b = loop_handle(name), loop_handle(name)
    N, n, m, batch = a.N, a.n, a.m, a.batch
    Qd, Rd, xref, uref = tracking_data(name, N, n, m, batch)
    a.set_tracking_cost(Qd, Rd, xref[:, :N + 1], uref[:, :N])
    b.set_tracking_cost(Qd, Rd, xref[:, 1:N + 2], uref[:, 1:N + 1])
    for bt in (a, b):
        finish(bt, name)
    if name.startswith("tile"):                               # the COST records' [q r] slot is the loop's expansion: the shift leaves it
        a.open_loop_rollout(); a.accept(); a.expand(); a.backward()
        K0, d0, P0, p0 = (a.get(w) for w in "KdPp")
    a.shift_linear_costs()
    if name.startswith("tile"):
        a.backward()
        for w, v in zip("KdPp", (K0, d0, P0, p0)):
            same(a.get(w), v, ("backward right after the shift", w))
    # the two knot points the shift leaves: N-1 with the running weight, N with the terminal one (r has no terminal knot point)
    xn, un = xref[:, N:N + 2], uref[:, N:N + 1]
    Qn = Qd[:, N - 1:N + 1]
    q = -(Qn * xn)
    r = -(Rd[:, N - 1:N] * un)
    c = 0.5 * (xn * Qn * xn).sum(axis=2)
    c[:, 0] += 0.5 * (un[:, 0] * Rd[:, N - 1] * un[:, 0]).sum(axis=1)
    a.update_linear_costs(q, None, c, N - 1, N)
    a.update_linear_costs(None, r, None, N - 1, N - 1)
    compare_loop(a, b, name)
    a.close(); b.close()


@pytest.mark.parametrize("name", ["lane", "lane_f32", "tile", "tile_f32", "tile_7_3", "mfma32", "generic"])
def test_twin_dense_cost(name):
    a, b = loop_handle(name), loop_handle(name)
    N, n, m, batch = a.N, a.n, a.m, a.batch
    w = problems.quadratic_cost(batch, N, n, m)
    if name.startswith("lane"):                               # the bicycle's scales (tests/mpc_common.py)
        w["Q"] = w["Q"] * M.QD; w["R"] = w["R"] * M.RD; w["H"] = w["H"] * 1e-3
    scale = 0.02 if name.startswith("lane") else 0.3
    q = scale * problems.normal((batch, N + 2, n), 95); r = scale * problems.normal((batch, N + 1, m), 96)
    c = problems.uniform01((batch, N + 2), 97)
    a.set_quadratic_cost(w["Q"], w["R"], w["H"], q[:, :N + 1], r[:, :N], c[:, :N + 1])
    b.set_quadratic_cost(w["Q"], w["R"], w["H"], q[:, 1:N + 2], r[:, 1:N + 1], c[:, 1:N + 2])
    for bt in (a, b):
        finish(bt, name)
    if name.startswith("tile"):
        a.open_loop_rollout(); a.accept(); a.expand(); a.backward()
        K0, d0 = a.get("K"), a.get("d")
    a.shift_linear_costs()
    if name.startswith("tile"):
        a.backward()
        same(a.get("K"), K0, "K right after the shift"); same(a.get("d"), d0, "d right after the shift")
    a.update_linear_costs(q[:, N:N + 2], None, c[:, N:N + 2], N - 1, N)
    a.update_linear_costs(None, r[:, N:N + 1], None, N - 1, N - 1)
    compare_loop(a, b, name)
    a.close(); b.close()


# ---- 5. five closed-loop MPC steps --------------------------------------------------------------------------------------------------
def test_closed_loop_mpc_steps():
    """The tile at batch 8, N = 12, the plant equal to the model: x+ = A_t x + B_t u + f_t with per-problem, time-varying data and a
    per-problem reference.  One handle lives through the five steps -- shifts plus one-knot-point writes --, one is built fresh at every
    step from the window's data; u_0, iterations and status agree at every step."""
    name, steps = "tile", 5
    _, n, m, N, batch, _, _ = CASES[name]
    T = N + steps + 1
    pr = problems.random_ltv(batch, T, n, m)
    A, B, f = pr["A"], pr["B"], pr["f"]
    xref = dyadic(0.3 * problems.normal((batch, T + 1, n), 101), 4)
    uref = dyadic(0.1 * problems.normal((batch, T, m), 102), 5)
    Qrun = 2.0 ** (np.arange(n) % 3 - 1.0); Rrun = 2.0 ** (-3.0 - np.arange(m) % 2)
    Qd = np.broadcast_to(Qrun, (batch, N + 1, n)).copy(); Qd[:, N] = 8.0 * Qrun
    Rd = np.broadcast_to(Rrun, (batch, N, m)).copy()

    def fresh(t, x0, u_guess):
        bt = handle(name)
        bt.set_dynamics(A[:, t:t + N], B[:, t:t + N], f[:, t:t + N])
        bt.set_tracking_cost(Qd, Rd, xref[:, t:t + N + 1], uref[:, t:t + N])
        bt.set_initial_state(x0); bt.set_input_guess(u_guess)
        return bt

    x = problems.normal((batch, n), 103)
    guess = np.zeros((batch, N, m))
    live = fresh(0, x, guess)
    for t in range(steps):
        twin = live if t == 0 else fresh(t, x, guess)
        res = live.ilqr_solve(iterations_max=10)
        _, u = live.get_nominal()
        if twin is not live:
            res2 = twin.ilqr_solve(iterations_max=10)
            _, u2 = twin.get_nominal()
            same(u[:, 0], u2[:, 0], ("u_0", t))
            same(res["iterations"], res2["iterations"], ("iterations", t)); same(res["status"], res2["status"], ("status", t))
            twin.close()
        assert (res["status"] == 0).all(), (t, res["status"])
        u0 = u[:, 0]
        At = A[:, t].reshape(batch, n, n).transpose(0, 2, 1); Bt = B[:, t].reshape(batch, m, n).transpose(0, 2, 1)
        x = np.einsum("bij,bj->bi", At, x) + np.einsum("bij,bj->bi", Bt, u0) + f[:, t]
        # the receding-horizon step on the resident handle: everything moves one knot point, only the new last one is written
        live.shift_trajectory()
        live.shift_dynamics()
        k = t + N                                              # the knot point that enters the window, as its knot point N-1
        live.set_dynamics_range(A[:, k:k + 1], B[:, k:k + 1], f[:, k:k + 1], N - 1, N - 1)
        live.shift_linear_costs()
        xn, un, Qn = xref[:, k:k + 2], uref[:, k:k + 1], Qd[:, N - 1:N + 1]
        c = 0.5 * (xn * Qn * xn).sum(axis=2)
        c[:, 0] += 0.5 * (un[:, 0] * Rd[:, N - 1] * un[:, 0]).sum(axis=1)
        live.update_linear_costs(-(Qn * xn), None, c, N - 1, N)
        live.update_linear_costs(None, -(Rd[:, N - 1:N] * un), None, N - 1, N - 1)
        live.set_initial_state(x)
        guess = shifted(u)
        live.set_input_guess(guess)
    live.close()


# ---- 6. errors and no-ops -----------------------------------------------------------------------------------------------------------
def refused(code, match, call):
    with pytest.raises(altro_amd.AltroHipError, match=match) as e:
        call()
    assert ("error %d:" % code) in str(e.value), str(e.value)


BAD_ARGUMENT, UNSUPPORTED, NOT_SET = -2, -3, -5


@pytest.mark.parametrize("name", ["lane", "tile_7_3", "generic_f32"])
def test_errors_leave_the_handle_as_it_was(name):
    bt = handle(name)
    N, n, m, batch, f32 = bt.N, bt.n, bt.m, bt.batch, is_f32(name)
    rng = np.random.default_rng(9)
    one = random_dyn(rng, batch, 1, n, m)
    # nothing set yet
    refused(NOT_SET, "altro_hip_set_dynamics has not been called", lambda: bt.set_dynamics_range(*one, 0, 0))
    refused(NOT_SET, "altro_hip_set_dynamics has not been called", lambda: bt.get_dynamics_knot(0))
    refused(NOT_SET, "altro_hip_set_dynamics has not been called", bt.shift_dynamics)
    refused(NOT_SET, "no quadratic cost", bt.shift_linear_costs)
    want = list(random_dyn(rng, batch, N, n, m))
    bt.set_dynamics(*want)
    # ranges and missing arrays
    for k0, k1 in ((-1, 0), (0, N), (N, N), (3, 2)):
        sized = random_dyn(rng, batch, max(k1 - k0 + 1, 1), n, m)
        refused(BAD_ARGUMENT, r"range \[%d, %d\]" % (k0, k1), lambda: bt.set_dynamics_range(*sized, k0, k1))
    refused(BAD_ARGUMENT, "A and B are required", lambda: bt.set_dynamics_range(None, one[1], one[2], 0, 0))
    refused(BAD_ARGUMENT, "A and B are required", lambda: bt.set_dynamics_range(one[0], None, one[2], 0, 0))
    refused(BAD_ARGUMENT, "knot point", lambda: bt.get_dynamics_knot(N))
    refused(BAD_ARGUMENT, "knot point", lambda: bt.get_dynamics_knot(-1))
    check_dyn(bt, want, f32, "after argument errors")
    # altro_hip_set_host_batch in effect
    bt.set_host_batch(2)
    refused(UNSUPPORTED, "altro_hip_set_host_batch", lambda: bt.set_dynamics_range(*one, 0, 0))
    refused(UNSUPPORTED, "altro_hip_set_host_batch", lambda: bt.get_dynamics_knot(0))
    refused(UNSUPPORTED, "altro_hip_set_host_batch", bt.shift_dynamics)
    bt.set_host_batch(0)
    check_dyn(bt, want, f32, "after host-batch errors")
    # still usable
    bt.set_dynamics_range(*one, N - 1, N - 1)
    for w, v in zip(want, one):
        w[:, N - 1:N] = v
    bt.shift_dynamics()
    check_dyn(bt, [shifted(v) for v in want], f32, "usable")
    bt.close()


def test_errors_device_model_and_dimensions():
    one = random_dyn(np.random.default_rng(1), 66, 1, M.n, M.m)
    bt = altro_amd.Batch(10, M.n, M.m, 66)
    bt.set_model(altro_amd.MODEL_BICYCLE, M.H)
    bt.set_tracking_cost(np.full((1, 11, M.n), M.QD), np.full((1, 10, M.m), M.RD), np.zeros((1, 11, M.n)), np.zeros((1, 10, M.m)), batch_stride_zero=True)
    refused(NOT_SET, "the model's", lambda: bt.set_dynamics_range(*one, 0, 0))
    refused(NOT_SET, "the model's", lambda: bt.get_dynamics_knot(0))
    refused(NOT_SET, "the model's", bt.shift_dynamics)
    bt.shift_linear_costs()                                   # (the cost of a device-model handle moves like any other)
    bt.close()
    nx, nu = [3, 4, 3, 2], [2, 1, 2]
    rg = altro_amd.Batch.with_dims(nx, nu, 5)
    refused(UNSUPPORTED, "uniform dimensions", lambda: rg.set_dynamics_range(np.zeros((5, 1, 16)), np.zeros((5, 1, 8)), None, 0, 0))
    refused(UNSUPPORTED, "uniform dimensions", lambda: rg.get_dynamics_knot(0))
    refused(UNSUPPORTED, "uniform dimensions", rg.shift_dynamics)
    refused(UNSUPPORTED, "uniform dimensions", rg.shift_linear_costs)
    rg.close()


@pytest.mark.parametrize("name", ["lane", "tile", "tile_f32", "generic"])
def test_one_knot_point_moves_nothing(name):
    bt = handle(name, N=1)
    n, m, batch = bt.n, bt.m, bt.batch
    want = integer_dyn(batch, 1, n, m)
    bt.set_dynamics(*want)
    bt.shift_dynamics()
    check_dyn(bt, want, False, "N = 1")
    if name != "lane":                                        # (plan LANE runs the loop on device models: test_errors_device_model_and_dimensions)
        p = problems.ilqr12x4_problem(batch, 1, True, n=n, m=m)
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.shift_linear_costs()                               # knot points N-1 = 0 and N = 1 keep theirs: nothing to move
        bt.set_quadratic_cost(*[problems.quadratic_cost(batch, 1, n, m)[key] for key in "QRHqrc"])
        bt.shift_linear_costs()
        check_dyn(bt, want, False, "N = 1, after the costs")
    bt.close()
