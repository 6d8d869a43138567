"""Per-knot-point time steps for device models (altro_hip_set_time_steps; ALTROSolver::SetTimeStep(h, k_start, k_stop),
altro_solver.hpp:55) on every plan that steps a model: LANE, MFMA16, GENERIC / MFMA32 in the row layout and the wave-per-problem
kernels, compiled in and from source.

Two grids:  G1  dt[k] = float32(0.02 + 0.003 k)  (every step differs: an index off by one shows at once),  G2  dt[k] = float32(0.05).

1. a constant array gives the bits of the uniform handle (rollout, expansion, merit, a whole solve);
2. every knot point uses its own step: x_{k+1}, A_k, B_k and the merit candidate against the oracle's model functions called with dt[k],
   knot by knot from the device's own x_k (rollout step 1e-12 on LANE, 1e-11 on the tile and GENERIC; A, B 1e-12; phi' against the
   central difference of phi 1e-6 -- the tolerances of the existing model tests of the same plan for the same quantity);
3. a whole constrained solve of the double integrator (linear in (x, u)) against the oracle with A_k, B_k of dt[k] as data: status,
   iterations, dual updates equal, trajectories 1e-11 / 1e-10 (tests/test_gpu_ilqr.py's for the double integrator);
4. errors and state of the setter / getter;
5. the tile plan's wide merit instantiation (four constraint slots), compiled in and from source.

phi' against differences: the five-point central difference with step 1e-3 (error h^4 phi^(5) / 30 ~ 1e-13 phi^(5), rounding ~ 2e-13 phi),
so that the comparison at 1e-6 tests phi', not the stencil.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import problems
from tests import test_gpu_tile_model_slots as slots
from tests.test_gpu_tile_model import QUADROTOR_SRC
from tests.test_gpu_user_model import PENDULUM_SRC

pytestmark = pytest.mark.gpu

H_UNIFORM = np.float32(0.05)
HOVER = np.array([0.5 * 9.81, 0.0, 0.0, 0.0])


def grid1(N):
    return (0.02 + 0.003 * np.arange(N)).astype(np.float32)


def grid2(N):
    return np.full(N, 0.05, dtype=np.float32)


def _quad_x0(batch, n, seed):
    x0 = np.zeros((batch, n))
    x0[:, :3] = 0.4 * problems.normal((batch, 3), seed)
    if n == 12:
        x0[:, 3:6] = 0.08 * problems.normal((batch, 3), seed + 1)
    else:
        q = np.concatenate([np.ones((batch, 1)), 0.06 * problems.normal((batch, 3), seed + 1)], axis=1)
        x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, n - 6:n - 3] = 0.2 * problems.normal((batch, 3), seed + 2)
    x0[:, n - 3:] = 0.05 * problems.normal((batch, 3), seed + 3)
    return x0


def _quad13_ref():
    xr = np.zeros(13); xr[3] = 1.0
    return xr


CASES = {
    "lane_pendulum": dict(n=2, m=1, model=altro_amd.MODEL_PENDULUM, omodel=(oracle.MODEL_PENDULUM, 0), lane=True),
    "lane_bicycle": dict(n=4, m=2, model=altro_amd.MODEL_BICYCLE, omodel=(oracle.MODEL_BICYCLE, 0), lane=True),
    "lane_double_integrator": dict(n=4, m=2, model=altro_amd.MODEL_DOUBLE_INTEGRATOR, omodel=(oracle.MODEL_DI, 2), lane=True),
    "tile_quadrotor": dict(n=12, m=4, model=altro_amd.MODEL_QUADROTOR, omodel=(oracle.MODEL_QUADROTOR, 0), lane=False),
    "row_quadrotor13": dict(n=13, m=4, model=altro_amd.MODEL_QUADROTOR13, omodel=(oracle.MODEL_QUADROTOR13, 0), lane=False, row=True),
    "lds_quadrotor13": dict(n=13, m=4, model=altro_amd.MODEL_QUADROTOR13, omodel=(oracle.MODEL_QUADROTOR13, 0), lane=False, row=False),
    "lane_pendulum_source": dict(n=2, m=1, source=PENDULUM_SRC, omodel=(oracle.MODEL_PENDULUM, 0), lane=True),
}


@functools.lru_cache(maxsize=None)
def case_data(name, N, batch):
    """Initial states, random inputs and the tracking cost of one case (computed once, shared, never written)."""
    c = CASES[name]
    n, m = c["n"], c["m"]
    if n in (12, 13):
        x0 = _quad_x0(batch, n, 301)
        u = HOVER + np.array([0.3, 0.002, 0.002, 0.002]) * problems.normal((batch, N, m), 305)
        Qd = np.concatenate([np.full(3, 2.0), np.full(n - 9, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
        Rd = np.array([0.05, 20.0, 20.0, 20.0])
        xref = np.zeros(n) if n == 12 else _quad13_ref()
        uref = HOVER
    elif name == "lane_bicycle":
        x0 = 0.2 * problems.normal((batch, n), 311); x0[:, 3] *= 0.5
        u = np.array([0.8, 0.0]) + np.array([0.3, 0.2]) * problems.normal((batch, N, m), 312)
        Qd, Rd, xref, uref = np.full(n, 1e-1), np.full(m, 1e-1), np.array([1.0, 0.5, 0.3, 0.0]), np.zeros(m)
    else:
        x0 = 0.5 * problems.normal((batch, n), 321)
        u = 0.5 * problems.normal((batch, N, m), 322)
        Qd, Rd, xref, uref = np.full(n, 1.0), np.full(m, 1e-1), np.zeros(n), np.zeros(m)
    for a in (x0, u):
        a.setflags(write=False)
    return dict(x0=x0, u=u, Qd=Qd, Qfd=10.0 * Qd, Rd=Rd, xref=xref, uref=uref)


def make_hip(name, N, batch, dt=None, h=H_UNIFORM, blocks=(), source=None):
    c, d = CASES[name], case_data(name, N, batch)
    bt = altro_amd.Batch(N, c["n"], c["m"], batch, plan=altro_amd.PLAN_LANE if c["lane"] else altro_amd.PLAN_AUTO)
    if c.get("row") is False:
        bt.set_forms(altro_amd.FORM_GENERIC_MERIT_LDS)
    # (blocks and cost first, the model last: a handle from source then compiles the one unit it launches)
    for (k0, k1, cone, G, g) in blocks:
        bt.add_linear_constraint(k0, k1, cone, G, g)
    bt.set_tracking_cost(np.stack([d["Qd"], d["Qfd"]]), d["Rd"][None], np.stack([d["xref"], d["xref"]]), d["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    src = source if source is not None else c.get("source")
    if src is not None:
        bt.set_model_source(src, h)
    else:
        bt.set_model(c["model"], h)
    if c["lane"]:
        assert bt.plan == altro_amd.PLAN_LANE
    elif c["n"] == 12:
        assert bt.plan == altro_amd.PLAN_MFMA16
    else:
        assert bt.plan == altro_amd.PLAN_MFMA32 and bt.model_row_layout() == c["row"]
    if dt is not None:
        bt.set_time_steps(dt)
    bt.set_initial_state(d["x0"])
    bt.set_input_guess(d["u"])
    return bt


def first_steps(bt):
    """Rollout, expansion, backward sweep, one merit evaluation at alpha = 0.5: everything a handle leaves behind."""
    bt.open_loop_rollout()
    x_roll, u_roll = bt.get("x"), bt.get("u")
    bt.accept(); bt.expand()
    A, B, lx, lu = bt.get_expansion()
    bt.backward()
    assert (bt.get("status") == -1).all()
    phi, dphi = bt.merit(0.5)
    return dict(x_roll=x_roll, u_roll=u_roll, A=A, B=B, lx=lx, lu=lu, phi=phi, dphi=dphi, xc=bt.get("x"), uc=bt.get("u"), yc=bt.get("y"))


# ---- 1. a constant grid is the uniform handle, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_constant_grid_equals_the_uniform_handle(name):
    c = CASES[name]
    N = 20
    batch = 70 if c["lane"] else 3
    out = []
    for dt in (None, grid2(N)):
        bt = make_hip(name, N, batch, dt)
        if dt is not None:
            assert np.array_equal(bt.get_time_steps(), dt)
        st = first_steps(bt)
        bt.set_input_guess(case_data(name, N, batch)["u"])
        res = bt.ilqr_solve(iterations_max=12, tol_stationarity=1e-3, forms=altro_amd.FORM_SEQUENCED if c["lane"] else 0)
        st.update(status=res["status"], iterations=res["iterations"], xn=bt.get_nominal()[0], un=bt.get_nominal()[1])
        out.append(st)
        bt.close()
    for key in out[0]:
        assert np.array_equal(out[0][key], out[1][key]), key
    assert np.isfinite(out[0]["xn"]).all() and np.isfinite(out[0]["phi"]).all()


# ---- 2. every knot point uses its own step -------------------------------------------------------------------------------------------
def _oracle_step(mdl, n, x, u, h):
    xn = np.zeros(n)
    oracle.lib().oracle_discrete_dynamics(C.byref(mdl), xn, np.ascontiguousarray(x), np.ascontiguousarray(u), h)
    return xn


def _oracle_jac(mdl, n, m, x, u, h):
    J = np.zeros(n * (n + m))
    oracle.lib().oracle_discrete_jacobian(C.byref(mdl), J, np.ascontiguousarray(x), np.ascontiguousarray(u), h)
    return J[:n * n], J[n * n:]


def check_knot_local(name, st, dt, N, batch, phi_fd):
    c = CASES[name]
    n, m = c["n"], c["m"]
    mdl = oracle.make_model(c["omodel"][0], c["omodel"][1])
    tol = 1e-12 if c["lane"] else 1e-11
    worst = dict(roll=0.0, cand=0.0, A=0.0, B=0.0)
    for b in range(batch):
        for k in range(N):
            h = float(dt[k])   # (passed as a C float: the value is a float32 already)
            xr = _oracle_step(mdl, n, st["x_roll"][b, k], st["u_roll"][b, k], h)
            xc = _oracle_step(mdl, n, st["xc"][b, k], st["uc"][b, k], h)
            Ar, Br = _oracle_jac(mdl, n, m, st["x_roll"][b, k], st["u_roll"][b, k], h)
            worst["A"] = max(worst["A"], np.abs(st["A"][b, k] - Ar).max()); worst["B"] = max(worst["B"], np.abs(st["B"][b, k] - Br).max())
            worst["roll"] = max(worst["roll"], np.abs(st["x_roll"][b, k + 1] - xr).max())
            worst["cand"] = max(worst["cand"], np.abs(st["xc"][b, k + 1] - xc).max())
            if c["lane"]:
                assert np.abs(st["x_roll"][b, k + 1] - xr).max() < tol, (b, k)
                assert np.abs(st["xc"][b, k + 1] - xc).max() < tol, (b, k)
            else:
                np.testing.assert_allclose(st["x_roll"][b, k + 1], xr, rtol=tol, atol=tol, err_msg="rollout %d %d" % (b, k))
                np.testing.assert_allclose(st["xc"][b, k + 1], xc, rtol=tol, atol=tol, err_msg="candidate %d %d" % (b, k))
            np.testing.assert_allclose(st["A"][b, k], Ar, rtol=1e-12, atol=1e-12, err_msg="A %d %d" % (b, k))
            np.testing.assert_allclose(st["B"][b, k], Br, rtol=1e-12, atol=1e-12, err_msg="B %d %d" % (b, k))
    print(name, "worst deviations", worst)
    if phi_fd is not None:
        print(name, "phi' - difference quotient", np.abs(st["dphi"] - phi_fd).max(), "of", np.abs(phi_fd).max())
        np.testing.assert_allclose(st["dphi"], phi_fd, rtol=1e-6, atol=1e-6)


def five_point(bt, alpha=0.5, e=1e-3):
    p = {s: bt.merit(alpha + s * e, derivative=False)[0] for s in (-2, -1, 1, 2)}
    return (p[-2] - 8.0 * p[-1] + 8.0 * p[1] - p[2]) / (12.0 * e)


@pytest.mark.parametrize("name", [k for k in CASES if k != "lane_pendulum_source"])
def test_every_knot_point_uses_its_own_step(name):
    c = CASES[name]
    N = 40 if c["n"] == 13 else 20
    batch = 70 if c["lane"] else 3
    dt = grid1(N)
    bt = make_hip(name, N, batch, dt)
    st = first_steps(bt)
    fd = five_point(bt)
    check_knot_local(name, st, dt, N, batch, fd)
    bt.close()


def test_pendulum_from_source_on_the_grid():
    """The pendulum as source: the knot-local checks, and the bits of the compiled-in pendulum on the same grid."""
    N, batch = 20, 70
    dt = grid1(N)
    bt = make_hip("lane_pendulum_source", N, batch, dt)
    st = first_steps(bt)
    check_knot_local("lane_pendulum_source", st, dt, N, batch, five_point(bt))
    b2 = make_hip("lane_pendulum", N, batch, dt)
    s2 = first_steps(b2)
    for key in st:
        assert np.array_equal(st[key], s2[key]), key
    u = case_data("lane_pendulum", N, batch)["u"]
    res = []
    for h in (bt, b2):
        h.set_input_guess(u)
        r = h.ilqr_solve(iterations_max=15, forms=altro_amd.FORM_SEQUENCED)
        res.append((r, h.get_nominal()))
    for k in ("status", "iterations", "phi", "stationarity"):
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    assert np.array_equal(res[0][1][0], res[1][1][0]) and np.array_equal(res[0][1][1], res[1][1][1])


# ---- 3. a whole constrained solve against the oracle ---------------------------------------------------------------------------------
DI_N, DI_BATCH, DI_UB = 20, 70, 2.5


@functools.lru_cache(maxsize=None)
def di_problem():
    n, m = 4, 2
    x0 = np.zeros((DI_BATCH, n))
    x0[:, :2] = 0.6 + 0.4 * problems.uniform01((DI_BATCH, 2), 331)
    x0[:, 2:] = 0.3 * (problems.uniform01((DI_BATCH, 2), 332) - 0.5)
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    x0.setflags(write=False)
    return dict(x0=x0, Qd=np.full(n, 1.0), Qfd=np.full(n, 50.0), Rd=np.full(m, 1e-2), G=G, g=np.full(2 * m, DI_UB), dt=grid1(DI_N))


def di_oracle_solve(b):
    """Problem b on the oracle with the double integrator's A_k, B_k at dt[k] as DATA (the model is linear in (x, u))."""
    p = di_problem()
    n, m, N = 4, 2, DI_N
    L = oracle.lib()
    A = np.zeros((N, n * n)); B = np.zeros((N, n * m))
    for k in range(N):
        J = np.zeros(n * (n + m))
        L.oracle_di_jacobian(J, np.zeros(n), np.zeros(m), float(p["dt"][k]), 2)
        A[k], B[k] = J[:n * n], J[n * n:]
    s = oracle.ILQR(N, n, m, p["dt"][0], oracle.DYN_LINEAR, cost_kind=oracle.COST_DIAGONAL)
    s.L.oracle_ilqr_set_linear_dynamics(s.h, A, B, None)
    for k in range(N + 1):
        s.L.oracle_ilqr_set_lqr_cost(s.h, k, p["Qfd"] if k == N else p["Qd"], p["Rd"], np.zeros(n), np.zeros(m))
    s.L.oracle_ilqr_set_initial_state(s.h, np.ascontiguousarray(p["x0"][b]))
    for k in range(N):
        s.add_linear_constraint(k, oracle.CONE_INEQUALITY, p["G"], p["g"])
    s.L.oracle_ilqr_initialize(s.h)
    for k in range(N):
        s.L.oracle_ilqr_set_input(s.h, k, np.zeros(m))
    s.set_penalty(1.0, 10.0)
    s.L.oracle_ilqr_set_options(s.h, 200, 1e-4, 1e-4, 1e-8, 0)     # the defaults of altro_hip_default_solve_options
    status, iters, log = s.solve()
    return status, iters, int((log[:, 4] < 1e-2).sum()), s.get("x"), s.get("u")


def test_constrained_solve_against_the_oracle():
    p = di_problem()
    n, m, N = 4, 2, DI_N
    bt = altro_amd.Batch(N, n, m, DI_BATCH)
    bt.set_model(altro_amd.MODEL_DOUBLE_INTEGRATOR, H_UNIFORM)
    assert bt.plan == altro_amd.PLAN_LANE
    bt.set_time_steps(p["dt"])
    bt.set_tracking_cost(np.stack([p["Qd"], p["Qfd"]]), p["Rd"][None], np.zeros((2, n)), np.zeros((1, m)), k_stride_zero=True, batch_stride_zero=True)
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, p["G"], p["g"])
    bt.set_initial_state(p["x0"])
    bt.set_input_guess(np.zeros((1, 1, m)), k_stride_zero=True, batch_stride_zero=True)
    res = bt.ilqr_solve(forms=altro_amd.FORM_SEQUENCED)
    x, u = bt.get_nominal()
    saturated = 0
    for b in range(DI_BATCH):
        status, iters, duals, xr, ur = di_oracle_solve(b)
        assert status == 0, b                                    # (chosen so on the CPU: no case needs excusing)
        assert (res["status"][b], res["iterations"][b], res["dual_updates"][b]) == (status, iters, duals), b
        np.testing.assert_allclose(x[b], xr, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(u[b], ur, rtol=1e-10, atol=1e-10)
        saturated += int(np.abs(ur).max() > DI_UB - 1e-3)
    assert saturated >= DI_BATCH // 2                            # the box is what shapes these solutions


# ---- 4. errors and state -------------------------------------------------------------------------------------------------------------
ERR_BAD_ARGUMENT, ERR_UNSUPPORTED, ERR_NOT_SET = "error -2:", "error -3:", "error -5:"


def _raises(code, fn, *args, **kw):
    with pytest.raises(altro_amd.AltroHipError) as e:
        fn(*args, **kw)
    assert code in str(e.value), str(e.value)


def test_errors_and_state():
    N, batch = 20, 70
    g1, g2 = grid1(N), grid2(N)
    # no device model: dynamics as data carry their own discretisation
    bt = altro_amd.Batch(N, 12, 4, 3)
    _raises(ERR_NOT_SET, bt.set_time_steps, g1)
    _raises(ERR_NOT_SET, bt.get_time_steps)
    bt.close()
    # per-knot-point dimensions
    bt = altro_amd.Batch.with_dims([3] * (N + 1), [2] * N, 3)
    _raises(ERR_UNSUPPORTED, bt.set_time_steps, g1)
    bt.close()
    bt = make_hip("lane_pendulum", N, batch)
    assert np.array_equal(bt.get_time_steps(), np.full(N, H_UNIFORM, dtype=np.float32))
    bt.set_time_steps(g1)
    for bad in (0.0, -0.01, np.nan, np.inf):
        d = g2.copy(); d[N - 1] = bad
        _raises(ERR_BAD_ARGUMENT, bt.set_time_steps, d)
        assert np.array_equal(bt.get_time_steps(), g1)
    with_grid = first_steps(bt)
    # the array does not move with the trajectory
    bt.shift_trajectory()
    assert np.array_equal(bt.get_time_steps(), g1)
    # a solve of a LANE handle with an array: the sequenced loop; no async
    u = case_data("lane_pendulum", N, batch)["u"]
    bt.set_input_guess(u)
    _raises(ERR_UNSUPPORTED, bt.ilqr_solve_async, iterations_max=10)
    res = bt.ilqr_solve(iterations_max=10)
    assert res["merit_launches"] > 1 and np.isfinite(bt.get_nominal()[0]).all()
    # NULL: the uniform handle again
    bt.set_time_steps(None)
    assert np.array_equal(bt.get_time_steps(), np.full(N, H_UNIFORM, dtype=np.float32))
    bt.set_input_guess(u)
    uniform = first_steps(bt)
    fresh = make_hip("lane_pendulum", N, batch)
    ref = first_steps(fresh)
    for key in ref:
        assert np.array_equal(uniform[key], ref[key]), key
    assert not np.array_equal(with_grid["x_roll"], ref["x_roll"])
    bt.set_input_guess(u); fresh.set_input_guess(u)
    ra, rb = bt.ilqr_solve(iterations_max=10), fresh.ilqr_solve(iterations_max=10)     # (both on the policy's path: one launch)
    assert np.array_equal(ra["iterations"], rb["iterations"]) and np.array_equal(bt.get_nominal()[0], fresh.get_nominal()[0])
    assert ra["merit_launches"] == rb["merit_launches"]
    # set_model clears the array
    bt.set_time_steps(g1)
    bt.set_model(altro_amd.MODEL_PENDULUM, np.float32(0.04))
    assert np.array_equal(bt.get_time_steps(), np.full(N, 0.04, dtype=np.float32))
    with pytest.raises(ValueError):
        bt.set_time_steps(g1[:-1])
    bt.close(); fresh.close()


# ---- 5. slots and the run-time path together -----------------------------------------------------------------------------------------
def test_four_slots_compiled_in_and_from_source():
    """MFMA16 quadrotor on G1 with an input box and a state box (four slots: the merit kernel's wide instantiation), compiled in and from
    source: knot-local checks for both, and the source handle's solve against the compiled-in one's (tests/test_gpu_tile_model.py:231-233)."""
    N, batch = 20, 3
    dt = grid1(N)
    xb = np.array([1.5, 1.5, 1.5, 0.3, 0.3, 0.3, 1.0, 1.0, 1.0, 0.4, 0.4, 0.4])
    blocks = slots.tables(N, np.array([0.6, 0.006, 0.006, 0.006]), xb, xb, 0.0, "slots4")   # (input box + state box; the terminal box and the cone are not in this table)
    u = case_data("tile_quadrotor", N, batch)["u"]
    out = []
    for source in (None, QUADROTOR_SRC):
        bt = make_hip("tile_quadrotor", N, batch, dt, blocks=blocks, source=source)
        st = first_steps(bt)
        check_knot_local("tile_quadrotor", st, dt, N, batch, None)   # (phi' of the AL merit function is not smooth enough for a stencil)
        bt.set_input_guess(u)
        res = bt.ilqr_solve(iterations_max=30, tol_stationarity=1e-3)
        out.append((res, bt.get_nominal()))
        bt.close()
    (r_mod, (x_mod, u_mod)), (r_src, (x_src, u_src)) = out
    assert np.array_equal(r_src["status"], r_mod["status"]) and np.array_equal(r_src["iterations"], r_mod["iterations"])
    np.testing.assert_allclose(x_src, x_mod, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(u_src, u_mod, rtol=1e-9, atol=1e-9)
