"""The instantiations of plan GENERIC's sweep kernels that a batch-size rule picks (altro_amd/csrc/sweep_route.h), reached at test-size
batches.  Needs an MI355X.

generic_backward_kernel<.., LQ = true> ("late Q") is what the library runs from 769 .. 3073 problems up at (16, 8) .. (33, 7), and for every
plan-MFMA32 handle whose cost was set diagonal (altro_hip_set_cost, is_diag) there; ALTRO_HIP_FORM_GENERIC_LATE_Q_ON / _OFF force one
form or the other at any batch.  Every case here asserts through Batch.sweep_variant that the instantiation it means to test is the one that ran, and holds it to what its
sibling is held to: the oracle's bits in fp64 (kernels/tvlqr_generic.hip follows the oracle's operation order), the sibling's bits, the
project's fp32 tolerance (2e-4 relative) in fp32.

Shapes (7, 3), (17, 5), (20, 8): n * n below 256, between, and n * m = 160 above the 128 elements reg_fetch<4> / <2> keep in registers;
m <= 4 (the gain solve in registers) and m > 4 (spread over the lanes).  N = 1, 2, 9; batch 5."""
import ctypes as C

import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import hard_cases as hc
from tests import problems
from tests.test_gpu_parity import relerr

pytestmark = pytest.mark.gpu

ON, OFF = altro_amd.FORM_GENERIC_LATE_Q_ON, altro_amd.FORM_GENERIC_LATE_Q_OFF
LQ, WS, MC, ST = altro_amd.SWEEP_LATE_Q, altro_amd.SWEEP_GLOBAL_WORKSPACE, altro_amd.SWEEP_MATRIX_CORES, altro_amd.SWEEP_FORWARD_STAGED
G, F64, F32 = altro_amd.PLAN_GENERIC, altro_amd.F64, altro_amd.F32
SHAPES = ((7, 3), (17, 5), (20, 8))
HORIZONS = (1, 2, 9)
BATCH = 5
SWEPT = ("K", "d", "P", "p", "delta_V", "x", "u", "y")


def diagonals(pr):
    N, n, m, B = pr["N"], pr["n"], pr["m"], pr["A"].shape[0]
    return (np.ascontiguousarray(pr["Q"].reshape(B, N + 1, n, n).diagonal(axis1=2, axis2=3)),
            np.ascontiguousarray(pr["R"].reshape(B, N, m, m).diagonal(axis1=2, axis2=3)))


def sweep(pr, forms, is_diag=False, with_f=True, reg=0.0, flags=0, dtype=F64, want=None, forward=True):
    """Backward and forward sweep of `pr` on plan GENERIC by name with `forms`; -> outputs, the open handle.  `want`: the backward
    launch's variant bits, asserted."""
    N, n, m, B = pr["N"], pr["n"], pr["m"], pr["A"].shape[0]
    bt = altro_amd.Batch(N, n, m, B, dtype=dtype, plan=G, flags=flags)
    assert bt.plan == G
    bt.set_forms(forms)
    bt.set_dynamics(pr["A"], pr["B"], pr["f"] if with_f else None)
    if is_diag:
        Qd, Rd = diagonals(pr)
        bt.set_cost(Qd, Rd, None, pr["q"], pr["r"], is_diag=True)
    else:
        bt.set_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    bt.set_initial_state(pr["x0"])
    bt.backward(reg)
    if want is not None:
        assert bt.sweep_variant(0) == want, (bt.sweep_variant(0), want)
        assert bt.profile_get(0)[2] == "generic_backward_kernel"
    out = {k: bt.get(k) for k in ("K", "d", "P", "p", "delta_V", "status")}
    if forward:
        bt.forward_ltv()
        out.update({k: bt.get(k) for k in ("x", "u", "y")})
    return out, bt


def reference(pr, is_diag=False, with_f=True, reg=0.0):
    f = pr["f"] if with_f else np.zeros_like(pr["f"])
    if is_diag:
        Qd, Rd = diagonals(pr)
        o = oracle.backward_batch(pr["A"], pr["B"], f, Qd, Rd, None, pr["q"], pr["r"], reg, True)
    else:
        o = oracle.backward_batch(pr["A"], pr["B"], f, pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"], reg, False)
    o["delta_V"] = o["dV"]
    if (o["status"] == -1).all():
        o.update(oracle.forward_batch(pr["A"], pr["B"], f, o["K"], o["d"], o["P"], o["p"], pr["x0"]))
    return o


def same(a, b, keys, what):
    assert np.array_equal(a["status"], b["status"]), what
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))


CASES = {"dense": {}, "no_affine_term": dict(with_f=False), "diagonal": dict(is_diag=True), "reg_in_the_pivots": dict(reg=0.75),
         "diagonal_reg": dict(is_diag=True, reg=0.75)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_late_q_equals_its_sibling_and_the_oracle(shape, case):
    """Late Q on against late Q off and the oracle, bit for bit in fp64: a dense cost with and without the affine term, a diagonal
    cost (Q's diagonal waits in K's block until P' is dead), reg > 0 (it enters the pivots only: the cost-to-go keeps Quu)."""
    n, m = shape
    kw = CASES[case]
    for N in HORIZONS:
        pr = problems.random_ltv(BATCH, N, n, m)
        on, b1 = sweep(pr, ON, want=LQ, **kw)
        off, b2 = sweep(pr, OFF, want=0, **kw)
        assert b1.sweep_variant(1) == b2.sweep_variant(1) == ST      # (these shapes stage the forward sweep: at most 9952 bytes)
        b1.close(); b2.close()
        ref = reference(pr, **kw)
        assert (ref["status"] == -1).all()
        same(on, off, SWEPT, (N, "late Q on / off"))
        same(off, ref, SWEPT, (N, "late Q off / oracle"))
        same(on, ref, SWEPT, (N, "late Q on / oracle"))
        if kw.get("reg"):                                            # (the regularisation is seen: the gains are not those of reg = 0)
            assert not np.array_equal(ref["K"], reference(pr, **dict(kw, reg=0.0))["K"])


def oracle_qblocks(pr, b, is_diag):
    """oracle_backward_flat on problem b: -> status, [N, Qxx | Quu | Qux | Qx | Qu] (what tests/test_gpu_parity.py's Q-block test
    compares altro_hip_get_qblocks with)."""
    L = oracle.lib()
    N, n, m = pr["N"], pr["n"], pr["m"]
    ws = L.oracle_ws_create(N, n, m)
    per = n * n + m * m + m * n + n + m
    qb = np.zeros((N, per)); K = np.zeros(N * n * m); d = np.zeros(N * m)
    P = np.zeros((N + 1) * n * n); p = np.zeros((N + 1) * n); dV = np.zeros(2)
    vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(pr[k][b]) for k in ("A", "B", "f", "q", "r")]
    if is_diag:
        Qd, Rd = diagonals(pr)
        cost = [np.ascontiguousarray(Qd[b]), np.ascontiguousarray(Rd[b]), None]
    else:
        cost = [np.ascontiguousarray(pr[k][b]) for k in ("Q", "R", "H")]
    st = L.oracle_backward_flat(ws, vp(keep[0]), vp(keep[1]), vp(keep[2]), vp(cost[0]), vp(cost[1]), None if cost[2] is None else vp(cost[2]),
                                vp(keep[3]), vp(keep[4]), 0.0, int(is_diag), vp(K), vp(d), vp(P), vp(p), vp(dV), vp(qb))
    L.oracle_ws_destroy(ws)
    return st, qb


@pytest.mark.parametrize("is_diag", [False, True], ids=["dense", "diagonal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_late_q_stored_q_blocks(shape, is_diag):
    """ALTRO_HIP_STORE_QBLOCKS: late Q writes Qxx BEFORE the factorisation (P_k is built over it), its sibling after.  The stored
    blocks of both equal the oracle's bit for bit."""
    n, m = shape
    for N in HORIZONS:
        pr = problems.random_ltv(BATCH, N, n, m)
        got = {}
        for forms, want in ((ON, LQ), (OFF, 0)):
            out, bt = sweep(pr, forms, is_diag=is_diag, flags=altro_amd.STORE_QBLOCKS, want=want, forward=False)
            got[forms] = bt.get("qblocks")
            bt.close()
        assert np.array_equal(got[ON], got[OFF]), N
        for b in (0, BATCH - 1):
            st, qb = oracle_qblocks(pr, b, is_diag)
            assert st == -1 and np.array_equal(got[ON][b], qb), (N, b, float(np.abs(got[ON][b] - qb).max()))


def fail_shift(n, m):
    """hc.with_failure's shift: the fixture's where the shape has one, else a power of two far above any entry of Quu on the benign family."""
    try:
        return float(hc.load(n, m)["fail_benign"][0])
    except OSError:
        return 1024.0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_late_q_stored_q_blocks_at_a_failing_knot_point(shape):
    """hc.with_failure: problem 1 of three fails at knot point 9 of 24.  With late Q the Qxx block of the failing knot point has been
    written all the same (before the factorisation) and is the oracle's; nothing is written below the failing knot point (the blocks
    of an earlier, successful sweep on the handle are still there); K_k = Qux and d_k = -Qu, unsolved; above it and in the neighbours
    everything is the oracle's.  The earlier sweep runs with the whole cost times 4: hc.with_failure changes one entry of R only, so
    with the same cost a Qxx, Qux, Qx or Qu store that was skipped at the failing knot point would leave the right bits behind;
    with this one every stale block there is four times the oracle's, which is asserted."""
    n, m = shape
    pr = hc.problem("benign", n, m, "d")
    prf = hc.with_failure(pr, fail_shift(n, m))
    b, kf = hc.FAIL_PROBLEM, hc.FAIL_KNOT
    per = (n * n, m * m, m * n, n, m)
    o = np.concatenate([[0], np.cumsum(per)])
    got = {}
    for forms, want in ((ON, LQ), (OFF, 0)):
        first, bt = sweep(hc.scaled_cost(pr, 1), forms, flags=altro_amd.STORE_QBLOCKS, want=want, forward=False)
        assert (first["status"] == -1).all()
        qb_first = bt.get("qblocks")
        bt.set_cost(prf["Q"], prf["R"], prf["H"], prf["q"], prf["r"])
        bt.backward()
        assert bt.sweep_variant(0) == want
        out = {k: bt.get(k) for k in ("K", "d", "P", "p", "status", "qblocks")}
        bt.close()
        assert out["status"].tolist() == [kf if i == b else -1 for i in range(hc.BATCH)]
        st, qb = oracle_qblocks(prf, b, False)
        assert st == kf
        for i, name in enumerate(("Qxx", "Quu", "Qux", "Qx", "Qu")):     # what the earlier sweep left at kf is not what this one must write
            assert not np.array_equal(qb_first[b, kf, o[i]:o[i + 1]], qb[kf, o[i]:o[i + 1]]), name
            assert np.array_equal(out["qblocks"][b, kf, o[i]:o[i + 1]], qb[kf, o[i]:o[i + 1]]), (name, "at the failing knot point")
        assert np.array_equal(out["qblocks"][b, kf + 1:], qb[kf + 1:]), "the blocks above the failing knot point"
        assert np.abs(out["qblocks"][b, kf, :n * n]).max() > 0
        assert np.array_equal(out["qblocks"][b, :kf], qb_first[b, :kf]), "written below the failing knot point"
        for q in ("K", "d", "P", "p"):
            assert np.array_equal(out[q][b, :kf], first[q][b, :kf]), (q, "written below the failing knot point")
        assert np.array_equal(out["K"][b, kf], out["qblocks"][b, kf, o[2]:o[3]])          # K_k = Qux
        assert np.array_equal(out["d"][b, kf], -out["qblocks"][b, kf, o[4]:o[5]])         # d_k = -Qu
        ref = oracle.backward_batch(prf["A"], prf["B"], prf["f"], prf["Q"], prf["R"], prf["H"], prf["q"], prf["r"])
        assert np.array_equal(out["K"][b, kf:], ref["K"][b, kf:]) and np.array_equal(out["d"][b, kf:], ref["d"][b, kf:])
        assert np.array_equal(out["P"][b, kf + 1:], ref["P"][b, kf + 1:]) and np.array_equal(out["p"][b, kf + 1:], ref["p"][b, kf + 1:])
        keep = [i for i in range(hc.BATCH) if i != b]
        for q in ("K", "d", "P", "p"):
            assert np.array_equal(out[q][keep], ref[q][keep]), (q, "a neighbour of the failing problem")
        got[forms] = out
    for q in ("K", "d", "P", "p", "qblocks"):
        assert np.array_equal(got[ON][q], got[OFF][q]), q


@pytest.mark.parametrize("is_diag", [False, True], ids=["dense", "diagonal"])
@pytest.mark.parametrize("which", ["shrinking", "growing", "mixed"])
def test_late_q_with_per_knot_point_dimensions(which, is_diag):
    """Per-knot-point dimensions: Q_k, n x n, arrives in the block P', n2 x n2, occupied.  tests/test_gpu_ragged.py's dimension lists
    through altro_hip_batch_create_dims, late Q on against off and, problem by problem, the oracle on the reference's pointer tables."""
    from tests.test_gpu_ragged import DIMS, make, oracle_one
    nx, nu = DIMS[which]
    p = make(nx, nu, BATCH, is_diag, seed=900 + len(nx))
    got = {}
    for forms, want in ((ON, LQ), (OFF, 0)):
        bt = altro_amd.Batch.with_dims(nx, nu, BATCH)
        assert bt.plan == G
        bt.set_forms(forms)
        bt.set_dynamics(p["A"], p["B"], p["f"])
        bt.set_cost(p["Q"], p["R"], p["H"], p["q"], p["r"], is_diag=is_diag)
        bt.set_initial_state(p["x0"])
        bt.sweep()
        assert bt.sweep_variant(0) == want
        got[forms] = {k: bt.get(k) for k in SWEPT + ("status",)}
        bt.close()
    same(got[ON], got[OFF], SWEPT, which)
    for b in (0, BATCH - 1):
        ref = oracle_one(nx, nu, p, b, is_diag)
        assert ref["status"] == -1 and got[ON]["status"][b] == -1
        for k in SWEPT:
            assert np.array_equal(got[ON][k][b], ref[k]), (which, is_diag, b, k)


def test_sweep_variant_before_any_launch_and_bad_arguments():
    bt = altro_amd.Batch(2, 7, 3, 2, plan=G)
    assert bt.sweep_variant(0) == 0 and bt.sweep_variant(1) == 0
    for slot in (-1, 2):
        with pytest.raises(altro_amd.AltroHipError):
            bt.sweep_variant(slot)
    with pytest.raises(altro_amd.AltroHipError, match="exclude each other"):      # both forms together stay refused
        bt.set_forms(ON | OFF)
    bt.close()
    bt = altro_amd.Batch(2, 12, 4, 2)                                # (the tile plan has no variants of this kind: zero after a sweep too)
    pr = problems.random_ltv(2, 2, 12, 4)
    bt.set_dynamics(pr["A"], pr["B"], pr["f"]); bt.set_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"]); bt.set_initial_state(pr["x0"])
    bt.sweep()
    assert bt.plan == altro_amd.PLAN_MFMA16 and bt.sweep_variant(0) == 0 and bt.sweep_variant(1) == 0
    bt.close()


# ---- the rule itself, unforced ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,last_without", [(24, 8, 1536), (33, 7, 768)])
def test_the_rule_takes_late_q_one_problem_past_the_threshold_fp64(n, m, last_without):
    """No forms: the last batch that keeps the block for Qxx and the first that takes late Q (sweep_route.h; 256 compute units times 6
    and 3 problems).  Every problem of both batches equals the oracle bit for bit."""
    pr = problems.random_ltv(last_without + 1, 2, n, m)
    ref = reference(pr)
    for batch, want in ((last_without, 0), (last_without + 1, LQ)):
        out, bt = sweep(hc.take(pr, slice(0, batch)), 0, want=want)
        assert bt.sweep_variant(1) == 0                              # (and the forward sweep reads its rows from global memory)
        bt.close()
        assert (out["status"] == -1).all()
        for k in SWEPT:
            assert np.array_equal(out[k], ref[k][:batch]), (batch, k)


def test_the_rule_takes_late_q_one_problem_past_the_threshold_fp32():
    """(32, 32) in fp32: 768 problems keep the block for Qxx, 769 take late Q.  The two batches' common problems are bit-identical
    ("same sums"), and a sample of 8 is within the project's fp32 tolerance of the oracle."""
    n, m, last_without = 32, 32, 768
    pr = problems.random_ltv(last_without + 1, 2, n, m)
    outs = []
    for batch, want in ((last_without, 0), (last_without + 1, LQ)):
        out, bt = sweep(hc.take(pr, slice(0, batch)), 0, dtype=F32, want=want)
        bt.close()
        assert (out["status"] == -1).all()
        outs.append(out)
    for k in SWEPT:
        assert np.array_equal(outs[0][k], outs[1][k][:last_without]), k
    sample = [0, 1, 100, 383, 384, 700, 767, 768]
    ref = reference(hc.take(pr, sample))
    for k in SWEPT:
        assert relerr(outs[1][k][sample], ref[k]) < 2e-4, (k, relerr(outs[1][k][sample], ref[k]))


# ---- the work block in global memory, the unstaged forward sweep ---------------------------------------------------------------------
def test_global_workspace_and_forward_variants():
    """(64, 16): neither carve fits 64 KB of LDS in either element type -- the work block in global memory, whatever the forms say; the
    forward sweep of (24, 8) in fp64 is past the 10 KB it stages, in fp32 it is not.  Results against the oracle as for the other
    instantiations: the oracle's bits in fp64, 2e-4 relative in fp32."""
    pr = problems.random_ltv(2, 2, 64, 16)
    ref = reference(pr)
    for forms in (0, ON, OFF):
        out, bt = sweep(pr, forms, want=WS)
        assert bt.sweep_variant(1) == 0
        bt.close()
        same(out, ref, SWEPT, ("(64, 16) fp64", forms))
    out, bt = sweep(pr, 0, dtype=F32, want=WS)
    assert bt.sweep_variant(1) == 0
    bt.close()
    for k in SWEPT:
        assert relerr(out[k], ref[k]) < 2e-4, k
    pr = problems.random_ltv(3, 2, 24, 8)
    ref = reference(pr)
    out, bt = sweep(pr, 0, want=0)
    assert bt.sweep_variant(1) == 0 and bt.profile_get(1)[2] == "generic_forward_kernel"
    bt.close()
    same(out, ref, SWEPT, "(24, 8) fp64, forward sweep from global memory")
    out, bt = sweep(pr, 0, dtype=F32, want=0)
    assert bt.sweep_variant(1) == ST
    bt.close()
    for k in SWEPT:
        assert relerr(out[k], ref[k]) < 2e-4, k


def test_matrix_cores_on_the_global_workspace():
    """generic_backward_kernel<double, BIG, matrix cores>: (50, 4), N = 3, three problems, under the criterion of
    tests/test_gpu_hard_tvlqr.py, blockerr <= 10 * max(e_cpu, 1e-13).  There is no extended-precision fixture of this shape: on
    problems.random_ltv the oracle's own error is ~1e-15 (every committed fixture's e64_benign_d is below 1e-14), so the floor 1e-13
    is the larger term and the oracle stands in for the fixture at an error a hundred times below the floor."""
    n, m = 50, 4
    pr = problems.random_ltv(3, 3, n, m)
    ref = reference(pr)
    out, bt = sweep(pr, 0, flags=altro_amd.GENERIC_MATRIX_CORES, want=WS | MC)
    bt.close()
    assert (out["status"] == -1).all()
    res = dict(out, dV=out["delta_V"])
    oref = dict(ref, dV=ref["delta_V"])
    errs = hc.errors({k: res[k] for k in hc.QUANTITIES}, {k: oref[k] for k in hc.QUANTITIES}, n, m)
    print("generic_mc (50, 4) global workspace: " + " ".join("%s %.2g" % (q, e / 1e-13) for q, e in errs.items()))
    for q, e in errs.items():
        assert e <= 10.0 * 1e-13, (q, e)


# ---- the iLQR loop ---------------------------------------------------------------------------------------------------------------------
RESULT = ("status", "iterations", "reg_retries")


def solved(bt, res):
    x, u = bt.get_nominal()
    return dict({k: np.asarray(res[k]) for k in RESULT}, x=x, u=u, K=bt.get("K"), d=bt.get("d"), P=bt.get("P"), p=bt.get("p"))


def same_solve(on, off):
    for k in RESULT + ("x", "u", "K", "d", "P", "p"):
        assert np.array_equal(on[k], off[k]), k


def test_loop_constrained_solve_plan_generic():
    """tests/test_gpu_ilqr_generic.py's constrained solve at (14, 5), late Q on against off: everything array_equal; the solve with late
    Q off meets the oracle as it does there."""
    from tests.test_gpu_ilqr_generic import _blocks, make, make_oracle
    N, batch, n, m = 16, 9, 14, 5
    blocks = _blocks(N, n, m, False)
    got = {}
    for forms, want in ((ON, LQ), (OFF, 0)):
        p, bt = make(batch, N, n, m, False)
        bt.set_forms(forms)
        for (k0, k1, cone, Gm, g) in blocks:
            bt.add_linear_constraint(k0, k1, cone, Gm, g)
        res = bt.ilqr_solve(iterations_max=60, penalty_initial=1.0, penalty_scaling=10.0)
        assert bt.sweep_variant(0) == want and bt.profile_get(0)[2] == "generic_backward_kernel"
        got[forms] = solved(bt, res)
        got[forms]["dual_updates"] = np.asarray(res["dual_updates"])
        bt.close()
    same_solve(got[ON], got[OFF])
    off = got[OFF]
    assert (off["dual_updates"] > 0).all()
    nconv = 0
    for b in (0, 4, 8):
        s = make_oracle(p, b, N, n, m, False)
        for k in range(N + 1):
            for (k0, k1, cone, Gm, g) in blocks:
                if k0 <= k <= k1:
                    s.add_linear_constraint(k, cone, Gm, g)
        s.L.oracle_ilqr_initialize(s.h)
        for k in range(N):
            s.L.oracle_ilqr_set_input(s.h, k, np.ascontiguousarray(p["u0"][b, k]))
        s.set_penalty(1.0, 10.0)
        s.L.oracle_ilqr_set_options(s.h, 60, 1e-4, 1e-4, 1e-8, 0)
        status, iters, log = s.solve()
        assert off["status"][b] == status and off["iterations"][b] == iters
        if status == 0:
            nconv += 1
            np.testing.assert_allclose(off["x"][b], s.get("x"), rtol=1e-7, atol=1e-7)
            np.testing.assert_allclose(off["u"][b], s.get("u"), rtol=1e-6, atol=1e-6)
    assert nconv >= 1


def test_diagonal_cost_plan_mfma32_keeps_the_generic_kernel():
    """A plan-MFMA32 handle whose cost is diagonal (altro_hip_set_cost with is_diag) keeps generic_backward_kernel for its backward
    sweep -- from 2817 problems up at (16, 8) the late-Q form.  Late Q on against off and the oracle, bit for bit; the forward sweep is
    the tile plan's (1e-12, as tests/test_gpu_tile32.py holds it)."""
    n, m, N = 16, 8, 9
    pr = problems.random_ltv(BATCH, N, n, m)
    Qd, Rd = diagonals(pr)
    ref = reference(pr, is_diag=True)
    got = {}
    for forms, want in ((ON, LQ), (OFF, 0)):
        bt = altro_amd.Batch(N, n, m, BATCH, plan=altro_amd.PLAN_MFMA32)
        assert bt.plan == altro_amd.PLAN_MFMA32
        bt.set_forms(forms)
        bt.set_dynamics(pr["A"], pr["B"], pr["f"])
        bt.set_cost(Qd, Rd, None, pr["q"], pr["r"], is_diag=True)
        bt.set_initial_state(pr["x0"])
        bt.sweep()
        assert bt.profile_get(0)[2] == "generic_backward_kernel" and bt.sweep_variant(0) == want
        assert bt.profile_get(1)[2] == "tile32_forward_kernel" and bt.sweep_variant(1) == 0
        got[forms] = {k: bt.get(k) for k in SWEPT + ("status",)}
        bt.close()
    same(got[ON], got[OFF], SWEPT, "late Q on / off")
    same(got[ON], ref, ("K", "d", "P", "p", "delta_V"), "late Q on / oracle")
    for k in ("x", "u", "y"):
        assert relerr(got[ON][k], ref[k]) < 1e-12, k


def test_loop_tracking_cost_plan_mfma32():
    """An iLQR solve with a tracking cost on plan MFMA32 at (16, 8).  altro_hip_set_tracking_cost lays the loop's Hessian blocks out
    dense (the handle's is_diag is 0), so the solve's backward sweep is tile32_backward_kernel, not generic_backward_kernel: the
    late-Q forms do not reach it, which this test pins -- the same kernel and no variant bit with either form; the two solves are then
    the same launches, so their equality says only that the forms are ignored.  The solve is held to the oracle as
    tests/test_gpu_tile32.py holds it.  No whole solve on a plan-MFMA32 handle reaches late Q: that plan's late-Q coverage is
    test_diagonal_cost_plan_mfma32_keeps_the_generic_kernel above."""
    from tests.test_gpu_ilqr_generic import make_oracle
    N, batch, n, m = 18, 11, 16, 8
    p = problems.ilqr12x4_problem(batch, N, True, n=n, m=m)
    got = {}
    for forms in (ON, OFF):
        bt = altro_amd.Batch(N, n, m, batch)
        assert bt.plan == altro_amd.PLAN_MFMA32
        bt.set_forms(forms)
        bt.set_dynamics(p["A"], p["B"], p["f"])
        bt.set_tracking_cost(p["Qd"], p["Rd"], p["xref"], p["uref"])
        bt.set_initial_state(p["x0"]); bt.set_input_guess(p["u0"])
        res = bt.ilqr_solve(iterations_max=10, tol_stationarity=1e-4)
        assert bt.profile_get(0)[2] == "tile32_backward_kernel" and bt.sweep_variant(0) == 0
        got[forms] = solved(bt, res)
        bt.close()
    same_solve(got[ON], got[OFF])
    off = got[OFF]
    assert (off["status"] == 0).all() and (off["iterations"] <= 3).all()
    for b in (0, 5, 10):
        s = make_oracle(p, b, N, n, m, False)
        s.L.oracle_ilqr_set_options(s.h, 10, 1e-4, 1e-4, 1e-8, 0)
        status, iters, log = s.solve()
        assert status == 0 and iters == off["iterations"][b]
        np.testing.assert_allclose(off["x"][b], s.get("x"), rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(off["u"][b], s.get("u"), rtol=1e-8, atol=1e-8)


def test_loop_per_knot_point_dimensions():
    """tests/test_gpu_ragged_ilqr.py's constrained solve with changing dimensions, late Q on against off; off against the oracle."""
    from tests import test_gpu_ragged_ilqr as rg
    batch = 9
    p = rg.make_problem(batch, seed=977)
    bounds = rg.input_bounds() + [rg.terminal_pin()]
    got = {}
    for forms, want in ((ON, LQ), (OFF, 0)):
        bt = rg.make_hip(p, batch, bounds)
        bt.set_forms(forms)
        res = bt.ilqr_solve(iterations_max=60, tol_stationarity=1e-4, penalty_initial=1.0, penalty_scaling=10.0)
        assert bt.sweep_variant(0) == want
        got[forms] = solved(bt, res)
        bt.close()
    same_solve(got[ON], got[OFF])
    off = got[OFF]
    assert (off["status"] == 0).all()
    for b in (0, 4, 8):
        s = rg.make_oracle(p, b, bounds)
        s.set_penalty(1.0, 10.0)
        s.L.oracle_ilqr_set_options(s.h, 60, 1e-4, 1e-4, 1e-8, 0)
        status, iters, log = s.solve()
        assert status == 0 and iters == off["iterations"][b]
        np.testing.assert_allclose(off["x"][b], rg.unpad_x(s.get("x")), rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(off["u"][b], rg.unpad_u(s.get("u")), rtol=1e-7, atol=1e-7)


def test_loop_indefinite_r_with_regularisation_retry():
    """tests/test_gpu_generic_reg.py's recipe at (14, 5): five problems whose R is indefinite at one knot point, rescued by the retry
    (the masked, per-problem-reg launches of the backward kernel).  Late Q on against off; off against the oracle's schedule."""
    from tests import test_gpu_generic_reg as gr
    pr = gr.recipe(14, 5)
    sched = gr.Schedule(gr.dense_arrays(pr))
    gr.check_recipe(sched)
    got = {}
    for forms, want in ((ON, LQ), (OFF, 0)):
        bt = gr.make_hip(pr, plan=G)
        assert bt.plan == G
        bt.set_forms(forms)
        res = bt.ilqr_solve(iterations_max=1, **gr.RETRY)
        assert bt.sweep_variant(0) == want
        assert (bt.get("status") == -1).all()
        got[forms] = solved(bt, res)
        got[forms]["res"] = res
        bt.close()
    same_solve(got[ON], got[OFF])
    retries, K, P = gr.expected(sched, got[OFF]["res"])
    assert (retries[gr.ODD] >= 1).all()
    assert np.array_equal(got[OFF]["reg_retries"], retries)
    assert np.array_equal(got[OFF]["K"], K) and np.array_equal(got[OFF]["P"], P)
