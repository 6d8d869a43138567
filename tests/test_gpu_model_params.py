"""Per-problem parameters for models and constraints from source (altro_hip_set_model_source_params / altro_hip_set_model_params): what
the reference gets for free from std::function callbacks that close over each solver's own constants (typedefs.hpp:31-53).

1. plan LANE, the kinematic bicycle from source with P = 2 (wheel base L, CoG -> rear axle lr; CoG frame), 70 vehicles that all differ,
   against the oracle's bicycle with (L_b, lr_b) per problem: knot-local (rollout / candidate step 1e-12, A, B 1e-12, phi' against the
   five-point difference 1e-6: tests/test_gpu_time_steps.py's check_knot_local), then whole solves with default options, unconstrained
   and with the steering input bounded by 0.3: status, iterations, dual updates of ALL 70, trajectories 5e-5 / 5e-4
   (tests/test_gpu_ilqr.py's bicycle tolerance);
2. the same handle on the grid dt[k] = float32(0.02 + 0.003 k): both doors of model_at compose;
3. plan MFMA16, the 12-state quadrotor from source with P = 4 (mass, Ix, Iy, Iz), two groups of vehicles interleaved A B A B A, against
   the same text with each group's numbers as literals: array_equal on everything the first steps and a 15-iteration solve leave;
4. the same on plan MFMA32 with the 13-state quadrotor, in the row layout and with FORM_GENERIC_MERIT_LDS;
5. reversing the batch (x0, u, theta rows) reverses every output, array_equal, on every plan above and plan LANE fp32;
   batch_stride_zero equals an array of identical rows;
6. parameters of the constraint pair: a disc / a sphere per vehicle on plans LANE, MFMA32 and MFMA16 (ALTRO_HIP_TILE_USER_BLOCKS);
7. errors and state.

Item 6's feasibility against numpy: the value is max over knot points of max(c, 0) with c = r^2 - |p - centre|^2 evaluated from the
device's OWN trajectory, a polynomial of numbers below 4 in fp64 -- a few ulps of 16, 1e-14; asserted at 1e-12.  Needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import problems
from tests.test_gpu_generic_model import QUADROTOR13_SRC
from tests.test_gpu_tile_model import QUADROTOR_SRC
from tests.test_gpu_time_steps import case_data, first_steps, five_point, grid1
from tests.test_gpu_user_model import PENDULUM_SRC, UNICYCLE_SRC

pytestmark = pytest.mark.gpu

H = np.float32(0.05)
HOVER = np.array([0.5 * 9.81, 0.0, 0.0, 0.0])
ERR_BAD_ARGUMENT, ERR_UNSUPPORTED, ERR_NOT_SET = "error -2:", "error -3:", "error -5:"

# ---- sources ---------------------------------------------------------------------------------------------------------------------------
BICYCLE_P_SRC = r"""
// kinematic bicycle about its centre of gravity: x = (px, py, theta, delta), u = (v, delta rate); p = (wheel base L, CoG -> rear axle lr).
// beta = atan2(lr delta, L) through one square root: cos(beta) = L / rho, sin(beta) = lr delta / rho.
template <typename T> struct BikeTrig { T st, ct, sb, cb, sd, cd, td, dbeta; };
__device__ inline void bike_sincos(double a, double* s, double* c) { sincos(a, s, c); }
__device__ inline void bike_sincos(float a, float* s, float* c) { sincosf(a, s, c); }
template <typename T> __device__ BikeTrig<T> bike_trig(const T* x, const T* p) {
  BikeTrig<T> t;
  const T L = p[0], lr = p[1];
  T sth, cth;
  bike_sincos(x[2], &sth, &cth);
  bike_sincos(x[3], &t.sd, &t.cd);
  t.td = t.sd / t.cd;
  const T by = lr * x[3], bx = L;
  const T r2 = bx * bx + by * by;
  const T ir = T(1) / sqrt(r2);
  t.cb = bx * ir;
  t.sb = by * ir;
  t.dbeta = bx / r2 * lr;
  t.st = sth * t.cb + cth * t.sb;
  t.ct = cth * t.cb - sth * t.sb;
  return t;
}
template <typename T> __device__ void altro_user_dynamics(const T* x, const T* u, const T* p, T* xdot) {
  const BikeTrig<T> t = bike_trig<T>(x, p);
  const T v = u[0], L = p[0];
  xdot[0] = v * t.ct;
  xdot[1] = v * t.st;
  xdot[2] = v * t.cb * t.td / L;
  xdot[3] = u[1];
}
template <typename T> __device__ void altro_user_jacobian(const T* x, const T* u, const T* p, T* J) {   // 4 x 6, column-major
  const BikeTrig<T> t = bike_trig<T>(x, p);
  const T v = u[0], L = p[0];
  for (int e = 0; e < 24; ++e) J[e] = T(0);
  J[0 + 2 * 4] = v * -t.st;
  J[0 + 3 * 4] = v * (-t.st * t.dbeta);
  J[0 + 4 * 4] = t.ct;
  J[1 + 2 * 4] = v * t.ct;
  J[1 + 3 * 4] = v * (t.ct * t.dbeta);
  J[1 + 4 * 4] = t.st;
  J[2 + 3 * 4] = v / L * (-t.sb * t.td * t.dbeta + t.cb / (t.cd * t.cd));
  J[2 + 4 * 4] = t.cb * t.td / L;
  J[3 + 5 * 4] = T(1);
}
"""

_QUAD_CONSTS = "const T mass = T(0.5), g = T(9.81), Ix = T(0.0023), Iy = T(0.0023), Iz = T(0.004);"
_QUAD_CONSTS_J = "const T mass = T(0.5), Ix = T(0.0023), Iy = T(0.0023), Iz = T(0.004);"
QUAD_A = (0.5, 0.0023, 0.0023, 0.004)       # the stock values of both quadrotor sources
QUAD_B = (0.65, 0.003, 0.0026, 0.005)


def quad_literals(src, v):
    """The quadrotor source with other numbers in the place of its literals (what a caller of altro_hip_set_model_source has to do)."""
    lit = "mass = T(%r), g = T(9.81), Ix = T(%r), Iy = T(%r), Iz = T(%r);" % v
    litJ = "mass = T(%r), Ix = T(%r), Iy = T(%r), Iz = T(%r);" % v
    assert src.count(_QUAD_CONSTS) == 1 and src.count(_QUAD_CONSTS_J) == 1
    return src.replace(_QUAD_CONSTS, "const T " + lit).replace(_QUAD_CONSTS_J, "const T " + litJ)


def quad_params(src):
    """... and with the four numbers read from p[0..3]: the functions take `const T* p`, everything else is the text as it stands."""
    out = src.replace(_QUAD_CONSTS, "const T mass = p[0], g = T(9.81), Ix = p[1], Iy = p[2], Iz = p[3];")
    out = out.replace(_QUAD_CONSTS_J, "const T mass = p[0], Ix = p[1], Iy = p[2], Iz = p[3];")
    assert out.count("const T* x, const T* u, T* xd)") == 1 and out.count("const T* x, const T* u, T* J)") == 1
    return out.replace("const T* x, const T* u, T* xd)", "const T* x, const T* u, const T* p, T* xd)").replace(
        "const T* x, const T* u, T* J)", "const T* x, const T* u, const T* p, T* J)")


def sphere_pair(n, m, first):
    """Stay outside a sphere: c = r^2 - |pos - centre|^2 <= 0 with (centre, r) = p[first .. first + 3]; 1 x (n + m) Jacobian."""
    return r"""
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, const T* p, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - p[%(f)d], dy = x[1] - p[%(f)d + 1], dz = x[2] - p[%(f)d + 2];
  c[0] = p[%(f)d + 3] * p[%(f)d + 3] - dx * dx - dy * dy - dz * dz;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, const T* p, T* J) {
  (void)id; (void)u;
  for (int e = 0; e < %(w)d; ++e) J[e] = T(0);
  J[0] = -T(2) * (x[0] - p[%(f)d]); J[1] = -T(2) * (x[1] - p[%(f)d + 1]); J[2] = -T(2) * (x[2] - p[%(f)d + 2]);
}
""" % dict(f=first, w=n + m)


DISC_P_SRC = UNICYCLE_SRC.replace("const T* x, const T* u, T* xdot)", "const T* x, const T* u, const T* p, T* xdot)").replace(
    "const T* x, const T* u, T* J)", "const T* x, const T* u, const T* p, T* J)") + r"""
// block 0: stay outside the disc of radius p[2] around (p[0], p[1]):  r^2 - |pos - centre|^2 <= 0
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, const T* p, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - p[0], dy = x[1] - p[1];
  c[0] = p[2] * p[2] - dx * dx - dy * dy;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, const T* p, T* J) {   // 1 x 5
  (void)id; (void)u;
  J[0] = -T(2) * (x[0] - p[0]); J[1] = -T(2) * (x[1] - p[1]); J[2] = T(0); J[3] = T(0); J[4] = T(0);
}
"""


def _raises(code, fn, *args, **kw):
    with pytest.raises(altro_amd.AltroHipError) as e:
        fn(*args, **kw)
    assert code in str(e.value), str(e.value)


# ---- 1. / 2. plan LANE: the bicycle, every vehicle its own (L, lr), against the oracle ------------------------------------------------
BN, BB = 20, 70


@functools.lru_cache(maxsize=None)
def bicycle_theta():
    L = 2.0 + 1.4 * problems.uniform01((BB,), 341)
    lr = L * (0.35 + 0.3 * problems.uniform01((BB,), 342))
    th = np.stack([L, lr], axis=1)
    th.setflags(write=False)
    return th


STEER = 0.3


def steering_block():
    """|steering input| <= 0.3 (the vehicle's second input, column n + 1 of [x; u]) at the running knot points."""
    G = np.zeros((2, 6)); G[0, 5] = 1.0; G[1, 5] = -1.0
    return G, np.array([STEER, STEER])


def make_bicycle(theta, dt=None, bound=False, dtype=altro_amd.F64, x0=None, u=None, shared=False):
    d = case_data("lane_bicycle", BN, BB)
    bt = altro_amd.Batch(BN, 4, 2, BB, dtype=dtype, plan=altro_amd.PLAN_LANE)
    if bound:
        bt.add_linear_constraint(0, BN - 1, altro_amd.CONE_INEQUALITY, *steering_block())
    bt.set_tracking_cost(np.stack([d["Qd"], d["Qfd"]]), d["Rd"][None], np.stack([d["xref"], d["xref"]]), d["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_model_source(BICYCLE_P_SRC, H, num_params=2)
    assert bt.plan == altro_amd.PLAN_LANE and bt.model_num_params == 2
    bt.set_model_params(theta[0] if shared else theta)
    if dt is not None:
        bt.set_time_steps(dt)
    bt.set_initial_state(d["x0"] if x0 is None else x0)
    bt.set_input_guess(d["u"] if u is None else u)
    return bt


def _oracle_step(mdl, n, x, u, h):
    xn = np.zeros(n)
    oracle.lib().oracle_discrete_dynamics(C.byref(mdl), xn, np.ascontiguousarray(x), np.ascontiguousarray(u), h)
    return xn


def _oracle_jac(mdl, n, m, x, u, h):
    J = np.zeros(n * (n + m))
    oracle.lib().oracle_discrete_jacobian(C.byref(mdl), J, np.ascontiguousarray(x), np.ascontiguousarray(u), h)
    return J[:n * n], J[n * n:]


def check_bicycle_knot_local(st, dt, theta, phi_fd):
    """tests/test_gpu_time_steps.py's check_knot_local (plan LANE's tolerances) with the oracle's model of EACH problem."""
    n, m = 4, 2
    worst = dict(roll=0.0, cand=0.0, A=0.0, B=0.0)
    for b in range(BB):
        mdl = oracle.make_model(oracle.MODEL_BICYCLE, 0, 0, float(theta[b, 0]), float(theta[b, 1]))
        for k in range(BN):
            h = float(dt[k])
            xr = _oracle_step(mdl, n, st["x_roll"][b, k], st["u_roll"][b, k], h)
            xc = _oracle_step(mdl, n, st["xc"][b, k], st["uc"][b, k], h)
            Ar, Br = _oracle_jac(mdl, n, m, st["x_roll"][b, k], st["u_roll"][b, k], h)
            worst["A"] = max(worst["A"], np.abs(st["A"][b, k] - Ar).max()); worst["B"] = max(worst["B"], np.abs(st["B"][b, k] - Br).max())
            worst["roll"] = max(worst["roll"], np.abs(st["x_roll"][b, k + 1] - xr).max())
            worst["cand"] = max(worst["cand"], np.abs(st["xc"][b, k + 1] - xc).max())
            assert np.abs(st["x_roll"][b, k + 1] - xr).max() < 1e-12, (b, k)
            assert np.abs(st["xc"][b, k + 1] - xc).max() < 1e-12, (b, k)
            np.testing.assert_allclose(st["A"][b, k], Ar, rtol=1e-12, atol=1e-12, err_msg="A %d %d" % (b, k))
            np.testing.assert_allclose(st["B"][b, k], Br, rtol=1e-12, atol=1e-12, err_msg="B %d %d" % (b, k))
    print("bicycle with parameters: worst knot-local deviations", worst)
    print("phi' - difference quotient", np.abs(st["dphi"] - phi_fd).max(), "of", np.abs(phi_fd).max())
    np.testing.assert_allclose(st["dphi"], phi_fd, rtol=1e-6, atol=1e-6)


@functools.lru_cache(maxsize=None)
def bicycle_oracle(b, bound, length=None, lr=None):
    """Problem b on the oracle alone, with its own (L, lr) -- or the given pair; default options."""
    d, th = case_data("lane_bicycle", BN, BB), bicycle_theta()
    s = oracle.ILQR(BN, 4, 2, H, oracle.DYN_MODEL, oracle.MODEL_BICYCLE)
    s.L.oracle_ilqr_set_bicycle(s.h, 0, float(th[b, 0]) if length is None else length, float(th[b, 1]) if lr is None else lr)
    for k in range(BN + 1):
        s.L.oracle_ilqr_set_lqr_cost(s.h, k, np.ascontiguousarray(d["Qfd"] if k == BN else d["Qd"]), np.ascontiguousarray(d["Rd"]),
                                     np.ascontiguousarray(d["xref"]), np.ascontiguousarray(d["uref"]))
    s.L.oracle_ilqr_set_initial_state(s.h, np.ascontiguousarray(d["x0"][b]))
    if bound:
        for k in range(BN):
            s.add_linear_constraint(k, oracle.CONE_INEQUALITY, *steering_block())
    s.L.oracle_ilqr_initialize(s.h)
    for k in range(BN):
        s.L.oracle_ilqr_set_input(s.h, k, np.ascontiguousarray(d["u"][b, k]))
    if bound:
        s.set_penalty(1.0, 10.0)
    s.L.oracle_ilqr_set_options(s.h, 200, 1e-4, 1e-4, 1e-8, 0)     # the defaults of altro_hip_default_solve_options
    status, iters, log = s.solve()
    return status, iters, int((log[:, 4] < 1e-2).sum()), s.get("x"), s.get("u")


@pytest.fixture(scope="module")
def bicycle_handle():
    bt = make_bicycle(bicycle_theta())
    yield bt
    bt.close()


def test_lane_bicycle_knot_local_against_the_oracle(bicycle_handle):
    bt, d = bicycle_handle, case_data("lane_bicycle", BN, BB)
    bt.set_time_steps(None)
    bt.set_input_guess(d["u"])
    assert np.array_equal(bt.get_model_params(), bicycle_theta())
    st = first_steps(bt)
    check_bicycle_knot_local(st, np.full(BN, H, dtype=np.float32), bicycle_theta(), five_point(bt))


def test_lane_bicycle_on_a_time_grid(bicycle_handle):
    """The same handle with a time-step array: dt[k] and (L_b, lr_b) both reach every step."""
    bt, d = bicycle_handle, case_data("lane_bicycle", BN, BB)
    dt = grid1(BN)
    bt.set_time_steps(dt)
    bt.set_input_guess(d["u"])
    st = first_steps(bt)
    check_bicycle_knot_local(st, dt, bicycle_theta(), five_point(bt))
    bt.set_time_steps(None)


@pytest.mark.parametrize("bound", [False, True])
def test_lane_bicycle_solves_against_the_oracle(bound):
    """Whole solves, default options: every one of the 70 takes the oracle's iterations (and dual updates) and ends on its trajectory.
    (On the CPU: the oracle converges on 70 of 70, in 2 .. 6 iterations without and 2 .. 7 with the bound, which is active in 11 problems;
    every solution is at least 3.7e-4 from the one with the stock (2.7, 1.5).  The bound is on the steering INPUT, |u_1| <= 0.3, at knot
    points 0 .. N - 1: these are the oracle's figures for it; the steering angle itself, a state, never passes 0.23 on these problems,
    so a bound of 0.3 on it would be active nowhere.)"""
    th = bicycle_theta()
    bt = make_bicycle(th, bound=bound)
    res = bt.ilqr_solve(forms=altro_amd.FORM_SEQUENCED)
    x, u = bt.get_nominal()
    worst_x = worst_u = 0.0
    active = 0
    apart = np.inf
    for b in range(BB):
        status, iters, duals, xr, ur = bicycle_oracle(b, bound)
        assert status == 0, b
        got = (res["status"][b], res["iterations"][b]) + ((res["dual_updates"][b],) if bound else ())
        assert got == (status, iters) + ((duals,) if bound else ()), (b, got, status, iters, duals)
        worst_x = max(worst_x, np.abs(x[b] - xr).max()); worst_u = max(worst_u, np.abs(u[b] - ur).max())
        np.testing.assert_allclose(x[b], xr, rtol=5e-5, atol=5e-5, err_msg="x of problem %d" % b)
        np.testing.assert_allclose(u[b], ur, rtol=5e-4, atol=5e-4, err_msg="u of problem %d" % b)
        active += int(np.abs(ur[:, 1]).max() > STEER - 1e-3)
        stock = bicycle_oracle(b, bound, 2.7, 1.5)
        apart = min(apart, max(np.abs(stock[3] - xr).max(), np.abs(stock[4] - ur).max()))
    print("bicycle solves, bound", bound, ": worst deviation x %.3e u %.3e; bound active in %d; nearest stock solution %.3e" % (worst_x, worst_u, active, apart))
    assert apart > 1e-4        # ignoring or mis-indexing the parameters cannot pass the tolerances above
    if bound:
        assert active >= 5     # the bound shapes some of these solutions
    bt.close()


# ---- 3. / 4. the quadrotors: parameters against the same text with literals ----------------------------------------------------------
def quad_case(name):
    n = 12 if name == "tile" else 13
    N = 20 if n == 12 else 40
    return n, N, 5, case_data("tile_quadrotor" if n == 12 else "row_quadrotor13", N, 5)


def quad_theta(batch=5):
    th = np.array([QUAD_A if b % 2 == 0 else QUAD_B for b in range(batch)])
    th.setflags(write=False)
    return th


def make_quad(name, source, theta=None, lds=False, order=None):
    n, N, batch, d = quad_case(name)
    o = np.arange(batch) if order is None else order
    bt = altro_amd.Batch(N, n, 4, batch)
    if lds:
        bt.set_forms(altro_amd.FORM_GENERIC_MERIT_LDS)
    Gb = np.zeros((2, n + 4)); Gb[0, n] = 1.0; Gb[1, n] = -1.0      # the input box of the existing model tests: a thrust bound
    bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, Gb, np.array([1.25 * HOVER[0], -0.6 * HOVER[0]]))
    bt.set_tracking_cost(np.stack([d["Qd"], d["Qfd"]]), d["Rd"][None], np.stack([d["xref"], d["xref"]]), d["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_model_source(source, H, num_params=0 if theta is None else 4)
    assert bt.plan == (altro_amd.PLAN_MFMA16 if n == 12 else altro_amd.PLAN_MFMA32)
    if theta is not None:
        bt.set_model_params(theta[o])
    bt.set_initial_state(d["x0"][o])
    bt.set_input_guess(d["u"][o])
    return bt


def quad_everything(bt, u):
    """first_steps, the backward sweep's gains, and a solve capped at 15 iterations."""
    st = first_steps(bt)
    st.update(K=bt.get("K"), d=bt.get("d"))
    bt.set_input_guess(u)
    res = bt.ilqr_solve(iterations_max=15, tol_stationarity=1e-3)
    xn, un = bt.get_nominal()
    st.update(status=res["status"], iterations=res["iterations"], phi_end=res["phi"], xn=xn, un=un)
    return st


@functools.lru_cache(maxsize=None)
def quad_reference(name, lds):
    """The parent's feature: one handle per group with the group's numbers as literals, all five rows on each."""
    src = QUADROTOR_SRC if name == "tile" else QUADROTOR13_SRC
    out = {}
    for group, v in (("A", QUAD_A), ("B", QUAD_B)):
        bt = make_quad(name, src if group == "A" else quad_literals(src, v), lds=lds)
        out[group] = quad_everything(bt, quad_case(name)[3]["u"])
        out[group]["row_layout"] = bt.model_row_layout()
        bt.close()
    return out


@pytest.mark.parametrize("name,lds", [("tile", False), ("row13", False), ("row13", True)])
def test_quadrotor_parameters_equal_the_literals(name, lds):
    src = QUADROTOR_SRC if name == "tile" else QUADROTOR13_SRC
    ref = quad_reference(name, lds)
    bt = make_quad(name, quad_params(src), quad_theta(), lds=lds)
    got = quad_everything(bt, quad_case(name)[3]["u"])
    if name != "tile":     # (asked where the reference handles were asked: after the constraint tables have been laid out)
        assert bt.model_row_layout() == ref["A"]["row_layout"] == ref["B"]["row_layout"] == (not lds)
    bt.close()
    assert np.isfinite(got["xn"]).all() and np.isfinite(got["phi"]).all()
    for key in got:
        for b in range(5):
            want = ref["A" if b % 2 == 0 else "B"][key][b]
            assert np.array_equal(got[key][b], want), (key, b, np.abs(np.asarray(got[key][b], dtype=float) - want).max())
    # the two groups are different vehicles: rows of one group do not pass for the other's
    assert not np.array_equal(ref["A"]["x_roll"][1], ref["B"]["x_roll"][1])


# ---- 5. permutation ------------------------------------------------------------------------------------------------------------------
def test_reversed_batch_lane():
    """fp64 and fp32: x0, u and theta rows reversed -> every output reversed; fp32: one shared set equals identical rows."""
    d, th = case_data("lane_bicycle", BN, BB), bicycle_theta()
    rev = np.arange(BB)[::-1]
    for dtype in (altro_amd.F64, altro_amd.F32):
        out = []
        for o in (np.arange(BB), rev):
            bt = make_bicycle(th[o], dtype=dtype, x0=d["x0"][o], u=d["u"][o])
            st = first_steps(bt)
            bt.set_input_guess(d["u"][o])
            res = bt.ilqr_solve(iterations_max=6, forms=altro_amd.FORM_SEQUENCED)
            st.update(iterations=res["iterations"], xn=bt.get_nominal()[0], un=bt.get_nominal()[1])
            out.append(st)
            bt.close()
        for key in out[0]:
            assert np.array_equal(out[0][key], out[1][key][::-1]), (dtype, key)
        assert np.isfinite(out[0]["xn"]).all()
    same = np.tile(th[3], (BB, 1))
    got = []
    for shared in (False, True):
        bt = make_bicycle(same, dtype=altro_amd.F32, shared=shared)
        assert np.array_equal(bt.get_model_params(), same.astype(np.float32).astype(np.float64))    # converted once, widened
        got.append(first_steps(bt))
        bt.close()
    for key in got[0]:
        assert np.array_equal(got[0][key], got[1][key]), key


@pytest.mark.parametrize("name,lds", [("tile", False), ("row13", False), ("row13", True)])
def test_reversed_batch_quadrotors(name, lds):
    src = quad_params(QUADROTOR_SRC if name == "tile" else QUADROTOR13_SRC)
    u = quad_case(name)[3]["u"]
    rev = np.arange(5)[::-1]
    out = []
    for o in (np.arange(5), rev):
        bt = make_quad(name, src, quad_theta(), lds=lds, order=o)
        out.append(quad_everything(bt, u[o]))
        bt.close()
    for key in out[0]:
        assert np.array_equal(out[0][key], out[1][key][::-1]), key


# ---- 6. parameters of the constraint pair --------------------------------------------------------------------------------------------
def test_a_disc_per_vehicle_on_plan_lane():
    """The unicycle and the disc of tests/test_gpu_user_model.py, every vehicle with its own disc (centre, radius) = p."""
    N, n, m, batch = 40, 3, 2, 70
    h = np.float32(0.1)
    xf = np.array([2.0, 1.0, 0.0])
    x0 = np.zeros((batch, n)); x0[:, 1] = (problems.uniform01((batch,), 47) - 0.5) * 0.2
    disc = np.stack([1.0 + 0.1 * (problems.uniform01((batch,), 351) - 0.5), 0.45 + 0.2 * (problems.uniform01((batch,), 352) - 0.5),
                     0.4 + 0.1 * (problems.uniform01((batch,), 353) - 0.5)], axis=1)
    bt = altro_amd.Batch(N, n, m, batch)
    bt.set_model_source(DISC_P_SRC, h, num_params=3)
    assert bt.plan == altro_amd.PLAN_LANE
    bt.set_model_params(disc)
    bt.set_tracking_cost(np.array([[1e-2] * 3, [50.0] * 3]), np.array([[1e-2, 1e-2]]), np.stack([xf, xf]), np.zeros((1, m)),
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(x0)
    bt.set_input_guess(np.array([[[0.5, 0.1]]]), k_stride_zero=True, batch_stride_zero=True)
    bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 0)
    bt.open_loop_rollout(); bt.accept()
    x = bt.get("x")
    c = disc[:, None, 2] ** 2 - (x[:, 1:, 0] - disc[:, None, 0]) ** 2 - (x[:, 1:, 1] - disc[:, None, 1]) ** 2
    want = np.maximum(c, 0.0).max(axis=1)
    feas = bt.feasibility()
    print("disc per vehicle: feasibility of the initial rollout, worst deviation from numpy", np.abs(feas - want).max(), "of", want.max())
    assert want.max() > 1e-2 and (want > 0).sum() > batch // 2      # the straight start cuts through most discs
    np.testing.assert_allclose(feas, want, rtol=0, atol=1e-12)
    res = bt.ilqr_solve(iterations_max=150, penalty_initial=10.0)
    x, _ = bt.get_nominal()
    ok = res["status"] == 0
    print("disc per vehicle: converged", int(ok.sum()), "of", batch)
    assert ok.sum() >= batch // 2
    # c of every vehicle's trajectory against every vehicle's disc: [trajectory, disc, knot point]
    call = disc[None, :, None, 2] ** 2 - (x[:, None, 1:, 0] - disc[None, :, None, 0]) ** 2 - (x[:, None, 1:, 1] - disc[None, :, None, 1]) ** 2
    own = call[np.arange(batch), np.arange(batch)].max(axis=1)
    assert (own[ok] <= 1e-4).all(), own[ok].max()                    # tol_primal_feasibility
    assert (res["feasibility"][ok] < 1e-4).all()
    other = call.max(axis=2)[ok]
    assert (other > 1e-3).any()                                      # ... and some trajectory would not clear another vehicle's disc
    bt.close()


@pytest.mark.parametrize("name", ["row13", "tile"])
def test_a_sphere_per_vehicle(name):
    """feasibility() of the initial rollout with a sphere (centre, radius) per vehicle behind the four model parameters: plan MFMA32, and
    plan MFMA16 on a handle created with ALTRO_HIP_TILE_USER_BLOCKS."""
    n, N, batch, d = quad_case(name)
    src = quad_params(QUADROTOR_SRC if name == "tile" else QUADROTOR13_SRC) + sphere_pair(n, 4, 4)
    bt = altro_amd.Batch(N, n, 4, batch, flags=altro_amd.TILE_USER_BLOCKS if name == "tile" else 0)
    bt.set_tracking_cost(np.stack([d["Qd"], d["Qfd"]]), d["Rd"][None], np.stack([d["xref"], d["xref"]]), d["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_model_source(src, H, num_params=8)
    assert bt.plan == (altro_amd.PLAN_MFMA16 if n == 12 else altro_amd.PLAN_MFMA32)
    # spheres the start sits inside of, by a different margin each: centre = x0's position + an offset, radius 0.3 .. 0.5
    off = 0.1 * problems.normal((batch, 3), 361)
    sph = np.concatenate([d["x0"][:, :3] + off, 0.3 + 0.2 * problems.uniform01((batch, 1), 362)], axis=1)
    theta = np.concatenate([quad_theta(), sph], axis=1)
    bt.set_model_params(theta)
    bt.set_initial_state(d["x0"])
    bt.set_input_guess(d["u"])
    bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 0)
    bt.open_loop_rollout(); bt.accept()
    x = bt.get("x")[:, :N + 1, :3]
    c = sph[:, None, 3] ** 2 - ((x[:, 1:] - sph[:, None, :3]) ** 2).sum(axis=2)
    want = np.maximum(c, 0.0).max(axis=1)
    feas = bt.feasibility()
    print(name, "sphere per vehicle: worst deviation from numpy", np.abs(feas - want).max(), "of", want)
    assert (want > 1e-3).all() and np.ptp(want) > 1e-3
    np.testing.assert_allclose(feas, want, rtol=0, atol=1e-12)
    bt.close()


# ---- 7. errors and state -------------------------------------------------------------------------------------------------------------
def test_errors_and_state():
    d, th = case_data("lane_bicycle", BN, BB), bicycle_theta()
    bt = altro_amd.Batch(BN, 4, 2, BB, plan=altro_amd.PLAN_LANE)
    L = bt.L
    # P out of range; nothing is taken
    for bad in (-1, 17):
        assert L.altro_hip_set_model_source_params(bt.h, BICYCLE_P_SRC.encode(), float(H), bad) == -2
    assert bt.model_num_params == 0
    # a handle without parameters
    _raises(ERR_NOT_SET, bt.set_model_params, th)
    assert L.altro_hip_get_model_params(bt.h, np.zeros((BB, 2)).ctypes.data_as(C.c_void_p)) == -5
    bt.set_model(altro_amd.MODEL_BICYCLE, H)
    assert bt.model_num_params == 0
    assert L.altro_hip_set_model_params(bt.h, th.ctypes.data_as(C.c_void_p), 0) == -5
    # an old-style source with P > 0: the compiler says so
    with pytest.raises(altro_amd.AltroHipError, match="does not compile"):
        bt.set_model_source(UNICYCLE_SRC, H, num_params=2)
    # before the setter: NOT_SET from every stepping call, and the handle stays usable
    bt.set_model_source(BICYCLE_P_SRC, H, num_params=2)
    assert bt.model_num_params == 2
    bt.set_tracking_cost(np.stack([d["Qd"], d["Qfd"]]), d["Rd"][None], np.stack([d["xref"], d["xref"]]), d["uref"][None],
                         k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(d["x0"])
    bt.set_input_guess(d["u"])
    for call in (bt.open_loop_rollout, bt.expand, lambda: bt.merit(0.5), bt.stationarity, bt.feasibility, lambda: bt.ilqr_solve(iterations_max=3)):
        _raises(ERR_NOT_SET, call)
    _raises(ERR_NOT_SET, bt.get_model_params)
    # a non-finite entry writes nothing
    before = bt.device_bytes()
    bt.set_model_params(th)
    assert bt.device_bytes() == before + 2 * BB * 8          # altro_hip_batch_device_bytes counts the array
    for bad in (np.nan, np.inf, -np.inf):
        t2 = th[::-1].copy(); t2[BB - 1, 1] = bad
        _raises(ERR_BAD_ARGUMENT, bt.set_model_params, t2)
        assert np.array_equal(bt.get_model_params(), th)
    with pytest.raises(ValueError):
        bt.set_model_params(th[:, :1])
    ref = first_steps(bt)
    # the trajectory shift does not touch the array
    bt.shift_trajectory()
    assert np.array_equal(bt.get_model_params(), th)
    # set again: other values, other results; the first values again: the first results
    bt.set_model_params(th[::-1])
    bt.set_input_guess(d["u"])
    assert not np.array_equal(first_steps(bt)["x_roll"], ref["x_roll"])
    bt.set_model_params(th)
    bt.set_input_guess(d["u"])
    again = first_steps(bt)
    for key in ref:
        assert np.array_equal(again[key], ref[key]), key
    # a later set_model drops the array (and its bytes); so does a source without parameters
    before = bt.device_bytes()
    bt.set_model(altro_amd.MODEL_BICYCLE, H)
    assert bt.model_num_params == 0 and bt.device_bytes() == before - 2 * BB * 8
    _raises(ERR_NOT_SET, bt.get_model_params)
    bt.set_model_source(BICYCLE_P_SRC, H, num_params=2)
    _raises(ERR_NOT_SET, bt.open_loop_rollout)              # (no values survive from the last time)
    bt.set_model_params(th)
    bt.set_model_source(BICYCLE_P_SRC, H, num_params=2)             # the same source again: a fresh model all the same
    _raises(ERR_NOT_SET, bt.get_model_params)
    bt.close()
    # fp32 handles: finite in the element type
    bt = make_bicycle(th, dtype=altro_amd.F32)
    t2 = th.copy(); t2[5, 0] = 1e300
    _raises(ERR_BAD_ARGUMENT, bt.set_model_params, t2)
    assert np.array_equal(bt.get_model_params(), th.astype(np.float32).astype(np.float64))
    bt.close()
    # per-knot-point dimensions
    bt = altro_amd.Batch.with_dims([3] * (BN + 1), [2] * BN, 3)
    _raises(ERR_UNSUPPORTED, bt.set_model_source, UNICYCLE_SRC, H, 3)
    assert bt.L.altro_hip_set_model_params(bt.h, np.ones((3, 3)).ctypes.data_as(C.c_void_p), 0) == -3
    bt.close()


def test_zero_parameters_is_set_model_source():
    """num_params = 0 through the new entry point: the unit, and so every bit, of altro_hip_set_model_source."""
    N, batch = 20, 70
    d = case_data("lane_pendulum", N, batch)
    out = []
    for new_entry in (False, True):
        bt = altro_amd.Batch(N, 2, 1, batch, plan=altro_amd.PLAN_LANE)
        bt.set_tracking_cost(np.stack([d["Qd"], d["Qfd"]]), d["Rd"][None], np.stack([d["xref"], d["xref"]]), d["uref"][None],
                             k_stride_zero=True, batch_stride_zero=True)
        if new_entry:
            assert bt.L.altro_hip_set_model_source_params(bt.h, PENDULUM_SRC.encode(), float(H), 0) == 0
        else:
            bt.set_model_source(PENDULUM_SRC, H)
        assert bt.model_num_params == 0
        bt.set_initial_state(d["x0"])
        bt.set_input_guess(d["u"])
        st = first_steps(bt)
        bt.set_input_guess(d["u"])
        res = bt.ilqr_solve(iterations_max=10)
        st.update(iterations=res["iterations"], xn=bt.get_nominal()[0])
        out.append(st)
        bt.close()
    for key in out[0]:
        assert np.array_equal(out[0][key], out[1][key]), key
