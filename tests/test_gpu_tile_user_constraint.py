"""Nonlinear constraint blocks from source on the (12, 4) tile plan: altro_hip_add_user_constraint on a plan MFMA16 handle created
with ALTRO_HIP_TILE_USER_BLOCKS (kernels/ilqr_merit2_dpp.hip, MD_USER_BLOCKS).  The CPU oracle has no nonlinear
constraints, so the references are
  * the same block given as DATA on the tile, for blocks that are linear (test 1: every phase of a sweep, then a truncated solve), with
    the oracle deciding on the CPU that the block matters (phi with it differs from phi without it by more than 1e-3 relative in
    every problem, both penalties) and numpy that it has a violated row at a compared point;
  * plan GENERIC's kernels for the same source and blocks (tests 2-5: a second, independently written implementation of the same
    mathematics, tests/test_gpu_generic_user_constraint.py), at the bound tests/test_gpu_tile_model_slots.py states for this pair of
    kernel families (1e-10 relative; whole solves: the same iteration count in all problems but one, trajectories 1e-7 / 1e-6);
  * a central difference of phi for phi' (test 6), the predicates of test_quadrotor_flies_around_a_keep_out_sphere (test 7), the bits
    of a fresh handle (test 8).
Every tile handle here is created with the flag: on a library without the feature each test fails at its handle's
set_model_source ("plan GENERIC").  Batch 7 (a ragged last wave in the two-per-wave and four-per-wave kernels), N = 10 for single
evaluations and 20 for solves, penalties 1 and 50; blocks that are data and the cost are set BEFORE the source (the unit compiled there
is the one launched; blocks from source can only follow it).

Run-time compiles: QUAD_USER_SRC on the tile with a user slot (diagonal two-slot / wide, dense two-slot) and without one (test 8's
linear blocks), QUADROTOR_SRC on the tile (test 1's data handles: the unit tests/test_gpu_tile_model_slots.py compiles), QUAD_USER_SRC
on plan GENERIC, PLANAR_USER_SRC on both plans.

The largest errors measured on an MI355X are in DESIGN 4.29 (the tests print theirs under -s)."""
import functools

import numpy as np
import pytest

import altro_amd
from tests import problems
from tests import test_gpu_tile_model as tm
from tests import test_gpu_tile_model_slots as ts
from tests.test_gpu_tile_model import HOVER, PLANAR_SRC, QUADROTOR_SRC

pytestmark = pytest.mark.gpu

n, m, w = 12, 4, 16
H = tm.H
BATCH, N_EVAL, N_SOLVE, RHOS, ALPHAS = ts.BATCH, ts.N_EVAL, ts.N_SOLVE, ts.RHOS, ts.ALPHAS
FLAG = getattr(altro_amd, "TILE_USER_BLOCKS", 0x2)     # (a library without the feature: the handle is created, the source refused)
TILE, GENERIC = altro_amd.PLAN_MFMA16, altro_amd.PLAN_GENERIC

# ---- the blocks -------------------------------------------------------------------------------------------------------------
# Widths chosen on the CPU with the oracle (linear_block_gap below asserts what they were chosen for): on the rolled-out
# trajectory -- alpha = 0 is one of the compared steps -- the thrust band lies below hover, the pin above it, and the torque cone
# around a point 0.54 away from the zero torque of hover (every compared point is outside it).
THRUST_G = np.array([HOVER[0] - 1.0, -(HOVER[0] - 2.0)])     # hover - 2 <= u0 <= hover - 1
PIN = 1.3 * HOVER[0]
CONE_G = np.array([0.4, -0.2, 0.3, -0.05])                   # |(u1, u2, u3) - (0.4, -0.2, 0.3)| <= 0.05
POS_T = 0.05                                                 # terminal |p| <= 0.05 per axis
SPHERE_C, SPHERE_R = np.array([0.5, 0.3, -0.2]), 0.45
VMAX2, TILT_COS = 0.25, 0.985              # single evaluations: |v| <= 0.5, cos(phi) cos(theta) >= 0.985 -- violated on the rollouts
VMAX2_SOLVE, TILT_COS_SOLVE = 4.0, 0.9     # whole solves: |v| <= 2, a tilt of 26 degrees -- limits the solves converge inside


def dense_block():
    """(b): eight rows over every state and input, through [xref; hover] shifted by 0.1 (the torques' columns scaled: tiny numbers)."""
    G = 0.3 * problems.normal((8, w), 511)
    G[:, n + 1:] *= 20.0
    return G, G @ np.concatenate([np.zeros(n), HOVER]) + 0.1


def linear_blocks(N):
    """name -> (user id, (k_first, k_last, cone, G, g)): the blocks of test 1, each also written out in QUAD_USER_SRC."""
    Ga = np.zeros((2, w)); Ga[0, n] = 1.0; Ga[1, n] = -1.0
    Gb, gb = dense_block()
    Gc = np.zeros((1, w)); Gc[0, n] = 1.0
    Gd = np.zeros((4, w)); Gd[0, n + 1] = Gd[1, n + 2] = Gd[2, n + 3] = 1.0
    Ge = np.zeros((6, w)); Ge[:3, :3] = np.eye(3); Ge[3:, :3] = -np.eye(3)
    return {"a_input_ineq": (0, (0, N - 1, altro_amd.CONE_INEQUALITY, Ga, THRUST_G)),
            "b_dense_ineq": (1, (0, N - 1, altro_amd.CONE_INEQUALITY, Gb, gb)),
            "c_equality_k0": (2, (0, 0, altro_amd.CONE_EQUALITY, Gc, np.array([PIN]))),
            "d_soc_torques": (3, (0, N - 1, altro_amd.CONE_SOC, Gd, CONE_G)),
            "e_terminal_states": (4, (N, N, altro_amd.CONE_INEQUALITY, Ge, np.full(6, POS_T)))}


def lit(v):
    return "T(%s)" % repr(float(v))


def quad_pair_source():
    G, g = dense_block()
    return r"""
__device__ const double kDenseG[128] = {%(Gl)s};   // 8 x 16, column-major
__device__ const double kDenseg[8] = {%(gl)s};
// id 0: hover - 2 <= u0 <= hover - 1 (2 rows)   1: the dense 8-row block   2: u0 = pin   3: |torques - a| <= t (SOC, 4 rows)
// 4: |p| <= pt per axis (6 rows, states only)   5: keep-out sphere r^2 - |p - c|^2 <= 0
// 6, 7: speed |v|^2 <= vmax^2 and tilt cos(phi) cos(theta) >= cmin (2 rows), with the evaluations' / the solves' limits
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  if (id == 0) {
    c[0] = u[0] - %(g0)s; c[1] = -u[0] - %(g1)s;
  } else if (id == 1) {
#pragma unroll 1
    for (int i = 0; i < 8; ++i) {
      T s = T(0);
      for (int e = 0; e < 12; ++e) s += T(kDenseG[i + 8 * e]) * x[e];
      for (int e = 0; e < 4; ++e) s += T(kDenseG[i + 8 * (12 + e)]) * u[e];
      c[i] = s - T(kDenseg[i]);
    }
  } else if (id == 2) {
    c[0] = u[0] - %(pin)s;
  } else if (id == 3) {
    c[0] = u[1] - %(s0)s; c[1] = u[2] - %(s1)s; c[2] = u[3] - %(s2)s; c[3] = -(%(s3)s);
  } else if (id == 4) {
    for (int i = 0; i < 3; ++i) { c[i] = x[i] - %(pt)s; c[3 + i] = -x[i] - %(pt)s; }
  } else if (id == 5) {
    const T dx = x[0] - %(cx)s, dy = x[1] - %(cy)s, dz = x[2] - %(cz)s;
    c[0] = %(r2)s - dx * dx - dy * dy - dz * dz;
  } else {
    c[0] = x[6] * x[6] + x[7] * x[7] + x[8] * x[8] - (id == 6 ? %(v2)s : %(v2s)s);
    c[1] = (id == 6 ? %(tc)s : %(tcs)s) - cos(x[3]) * cos(x[4]);
  }
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // p x 16, column-major
  (void)u;
  if (id == 0) {
    for (int e = 0; e < 2 * 16; ++e) J[e] = T(0);
    J[0 + 12 * 2] = T(1); J[1 + 12 * 2] = T(-1);
  } else if (id == 1) {
#pragma unroll 1
    for (int e = 0; e < 128; ++e) J[e] = T(kDenseG[e]);
  } else if (id == 2) {
    for (int e = 0; e < 16; ++e) J[e] = T(0);
    J[12] = T(1);
  } else if (id == 3) {
    for (int e = 0; e < 4 * 16; ++e) J[e] = T(0);
    J[0 + 13 * 4] = T(1); J[1 + 14 * 4] = T(1); J[2 + 15 * 4] = T(1);
  } else if (id == 4) {
    for (int e = 0; e < 6 * 16; ++e) J[e] = T(0);
    for (int i = 0; i < 3; ++i) { J[i + i * 6] = T(1); J[3 + i + i * 6] = T(-1); }
  } else if (id == 5) {
    for (int e = 0; e < 16; ++e) J[e] = T(0);
    J[0] = -T(2) * (x[0] - %(cx)s); J[1] = -T(2) * (x[1] - %(cy)s); J[2] = -T(2) * (x[2] - %(cz)s);
  } else {
    for (int e = 0; e < 2 * 16; ++e) J[e] = T(0);
    J[0 + 6 * 2] = T(2) * x[6]; J[0 + 7 * 2] = T(2) * x[7]; J[0 + 8 * 2] = T(2) * x[8];
    J[1 + 3 * 2] = sin(x[3]) * cos(x[4]); J[1 + 4 * 2] = cos(x[3]) * sin(x[4]);
  }
}
""" % dict(Gl=", ".join(repr(float(v)) for v in G.T.reshape(-1)), gl=", ".join(repr(float(v)) for v in g),
           g0=lit(THRUST_G[0]), g1=lit(THRUST_G[1]), pin=lit(PIN), s0=lit(CONE_G[0]), s1=lit(CONE_G[1]), s2=lit(CONE_G[2]), s3=lit(CONE_G[3]),
           pt=lit(POS_T), cx=lit(SPHERE_C[0]), cy=lit(SPHERE_C[1]), cz=lit(SPHERE_C[2]), r2=lit(SPHERE_R ** 2), v2=lit(VMAX2), tc=lit(TILT_COS), v2s=lit(VMAX2_SOLVE), tcs=lit(TILT_COS_SOLVE))


QUAD_USER_SRC = QUADROTOR_SRC + quad_pair_source()
SPHERE_ID, SPEED_TILT_ID, SPEED_TILT_SOLVE_ID = 5, 6, 7

DISC_C, DISC_R = np.array([0.2, -0.1]), 0.5
PLANAR_USER_SRC = PLANAR_SRC + r"""
// block 0: stay outside a disc in the (px, pz) plane
template <typename T> __device__ void altro_user_constraint(int id, const T* x, const T* u, T* c) {
  (void)id; (void)u;
  const T dx = x[0] - T(0.2), dz = x[1] - T(-0.1);
  c[0] = T(0.25) - dx * dx - dz * dz;
}
template <typename T> __device__ void altro_user_constraint_jacobian(int id, const T* x, const T* u, T* J) {   // 1 x 8
  (void)id; (void)u;
  for (int e = 0; e < 8; ++e) J[e] = T(0);
  J[0] = -T(2) * (x[0] - T(0.2)); J[1] = -T(2) * (x[1] - T(-0.1));
}
"""


# ---- handles ----------------------------------------------------------------------------------------------------------------
def make_hip(c, N, plan, source, data=(), user=(), dense=False, flags=FLAG):
    """Data blocks and the cost, the source, the blocks from it.  user: (k_first, k_last, cone, p, id)."""
    batch = c["x0"].shape[0]
    bt = altro_amd.Batch(N, n, m, batch, plan=plan, flags=flags if plan != GENERIC else 0)
    assert bt.plan == (TILE if plan != GENERIC else GENERIC)
    for (k0, k1, cone, G, g) in data:
        bt.add_linear_constraint(k0, k1, cone, G, g)
    if dense:
        bt.set_quadratic_cost(c["Q"], c["R"], c["H"], c["q"], c["r"], c["c"])
    else:
        bt.set_tracking_cost(np.stack([c["Qd"], c["Qfd"]]), c["Rd"][None], np.stack([c["xref"], c["xref"]]), c["uref"][None],
                             k_stride_zero=True, batch_stride_zero=True)
    bt.set_model_source(source, H)
    assert bt.plan == (TILE if plan != GENERIC else GENERIC)
    for (k0, k1, cone, p, cid) in user:
        bt.add_user_constraint(k0, k1, cone, p, cid)
    bt.set_initial_state(c["x0"])
    bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)
    return bt


def phases(bt, c, rho, alphas, nx=n, N=N_EVAL, gains=True):
    """open_loop_rollout; accept; reset_duals(rho); expand; backward -- then what every phase leaves behind."""
    ts.sweep(bt, c, rho)
    _, _, lx, lu = bt.get_expansion()          # (of the rolled-out trajectory: no merit pass has run since the expansion)
    out = dict(lx=lx, lu=lu)
    if gains:
        out["K"], out["d"] = bt.get("K"), bt.get("d")
    out["phi0"], out["dphi0"] = bt.merit(np.zeros(len(alphas)))
    out["phi"], out["dphi"] = bt.merit(alphas)
    out["x"], out["u"] = bt.get("x")[:, :N + 1, :nx].copy(), bt.get("u").copy()
    out["feas"] = bt.feasibility()
    out["stat"] = bt.stationarity()
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) if a.size else 0.0


def absmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


@functools.lru_cache(maxsize=None)
def eval_case(dense=False, N=N_EVAL, inside=True):
    """tests/test_gpu_tile_model.py's problem around the sphere.  inside (single evaluations): the start positions scattered 0.15 around
    its centre, all of them in it -- chosen on the CPU (the oracle's candidates with the boxes, the user rows in numpy) so that the
    two user slots carry more than 5e-3 of phi in every problem at both penalties; else (whole solves): the start positions on a sphere
    of radius 0.6 around the centre, 0.15 outside the keep-out radius -- chosen on the GPU so that plan GENERIC's solves converge in
    every problem with the sphere binding in some (clearance 0.450 in problem 5); solves that fail amplify the last bit and have no
    answer at 1e-7, as tests/test_gpu_tile_model_slots.py found."""
    c = dict(ts.make_case(dense, N))
    x0 = c["x0"].copy()
    d = problems.normal((BATCH, 3), 611)
    x0[:, :3] = SPHERE_C + (0.15 * d if inside else 0.6 * d / np.linalg.norm(d, axis=1, keepdims=True))
    c["x0"] = x0
    return c


# ---- 1: a linear block written as source equals the same block given as data ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_block_gap(name):
    """min over penalties and problems of |phi with the block - phi without it| / max(1, |phi|) at the problem's alpha (the oracle)."""
    c = ts.make_case(False, N_EVAL)
    blk = linear_blocks(N_EVAL)[name][1]
    gap = np.inf
    for rho in RHOS:
        for b in range(BATCH):
            out = []
            for bl in ([blk], []):
                s = ts.oracle_sweep(c, b, False, N_EVAL, bl, rho)
                assert s.L.oracle_ilqr_backward_pass(s.h) == -1
                out.append(s.merit(ALPHAS[b])[0])
            gap = min(gap, abs(out[0] - out[1]) / max(1.0, abs(out[0])))
    return gap


@pytest.mark.parametrize("name", sorted(linear_blocks(N_EVAL)))
def test_linear_block_as_source_equals_the_block_as_data(name):
    """Phase by phase on the tile, penalties 1 and 50: phi 1e-10, phi' 1e-8 relative at alpha = linspace(0, 1.1, 7) and at 0, the
    candidates 2e-9 / 2e-8, lx / lu 1e-11, K / d 1e-8, feasibility and stationarity 1e-7 relative; after a solve of four sweeps
    status, iterations, dual updates equal and every dual within 1e-12.
    Measured maxima over the five blocks (MI355X): see DESIGN 4.29."""
    assert linear_block_gap(name) > 1e-3, linear_block_gap(name)
    c = ts.make_case(False, N_EVAL)
    uid, blk = linear_blocks(N_EVAL)[name]
    k0, k1, cone, G, g = blk
    a = make_hip(c, N_EVAL, TILE, QUAD_USER_SRC, user=[(k0, k1, cone, G.shape[0], uid)])
    b = make_hip(c, N_EVAL, TILE, QUADROTOR_SRC, data=[blk])
    worst, violated = {}, 0.0

    def note(key, err, tol):
        worst[key] = max(worst.get(key, 0.0), float(err))
        assert err <= tol, (name, key, err, tol)

    for rho in RHOS:
        ra, rb = phases(a, c, rho, ALPHAS), phases(b, c, rho, ALPHAS)
        for key, tol in (("phi", 1e-10), ("phi0", 1e-10), ("dphi", 1e-8), ("dphi0", 1e-8), ("feas", 1e-7), ("stat", 1e-7)):
            note(key, rel(ra[key], rb[key]), tol)
        for key, tol in (("K", 1e-8), ("d", 1e-8)):
            note(key, absmax(ra[key], rb[key]) / max(1.0, float(np.abs(rb[key]).max())), tol)
        for key, tol in (("lx", 1e-11), ("lu", 1e-11), ("x", 2e-9), ("u", 2e-8)):
            worst[key] = max(worst.get(key, 0.0), absmax(ra[key], rb[key]))      # (absolute, for the record)
            np.testing.assert_allclose(ra[key], rb[key], rtol=tol, atol=tol, err_msg="%s %s rho %g" % (name, key, rho))
        for p in range(BATCH):   # numpy on the candidate: the block has a violated row (the cone: a point outside it)
            violated = max(violated, max(max(r) if r else 0.0 for r in ts.slot_violations([blk], N_EVAL, rb["x"][p], rb["u"][p])))
    assert violated > 1e-4, (name, violated)
    a.close(); b.close()
    # a truncated solve
    c = ts.make_case(False, N_SOLVE)
    uid, blk = linear_blocks(N_SOLVE)[name]
    k0, k1, cone, G, g = blk
    sol = []
    for bt in (make_hip(c, N_SOLVE, TILE, QUAD_USER_SRC, user=[(k0, k1, cone, G.shape[0], uid)]), make_hip(c, N_SOLVE, TILE, QUADROTOR_SRC, data=[blk])):
        res = bt.ilqr_solve(iterations_max=4, tol_stationarity=1e-3, penalty_initial=1.0, penalty_scaling=10.0)
        sol.append((res, np.stack([bt.get_duals(k, 0, G.shape[0]) for k in range(k0, k1 + 1)])))
        bt.close()
    (ra, za), (rb, zb) = sol
    for key in ("status", "iterations", "dual_updates"):
        assert np.array_equal(ra[key], rb[key]), (name, key, ra[key], rb[key])
    note("duals", absmax(za, zb), 1e-12)
    assert np.abs(zb).max() > 0.0                    # the duals moved
    print("measured maxima (%s):" % name, {k: "%.1e" % v for k, v in worst.items()})


# ---- 2-5: nonlinear blocks against plan GENERIC's kernels -----------------------------------------------------------------------
def against_generic(make, alphas, c, N, nx=n, solve=True, label=""):
    """make(plan) -> handle.  Single evaluations at penalty 50 and 1 (phi, phi', lx, lu, feasibility: 1e-10 relative), then whole
    solves (the same iteration count in all problems but one at most, trajectories 1e-7 / 1e-6 on those).  Returns the tile's phases."""
    worst = {}
    first = None
    tile, gen = make(TILE), make(GENERIC)
    for rho in RHOS[::-1]:
        rt, rg = phases(tile, c, rho, alphas, nx, N, gains=False), phases(gen, c, rho, alphas, nx, N, gains=False)
        first = first or (rt, rg)
        for key in ("phi", "dphi", "phi0", "dphi0", "lx", "lu", "feas"):
            a, b = np.asarray(rt[key]), np.asarray(rg[key])
            scale = max(1.0, float(np.abs(b).max()))
            worst[key] = max(worst.get(key, 0.0), absmax(a, b) / scale)
            np.testing.assert_allclose(a, b, rtol=1e-10, atol=1e-10 * scale, err_msg="%s %s rho %g" % (label, key, rho))
        assert float(np.max(rt["feas"])) > 0.0
    tile.close(); gen.close()
    if solve:
        sol = []
        for plan in (TILE, GENERIC):
            bt = make(plan, N_SOLVE)
            res = bt.ilqr_solve(iterations_max=60, tol_stationarity=1e-3, penalty_initial=10.0, penalty_scaling=10.0)
            sol.append((res, *bt.get_nominal()))
            bt.close()
        (ra, xa, ua), (rb, xg, ug) = sol
        same = ra["iterations"] == rb["iterations"]
        print(label, "solves: status", ra["status"], rb["status"], "iterations", ra["iterations"], rb["iterations"])
        assert same.sum() >= len(same) - 1, (label, ra["iterations"], rb["iterations"])
        worst["x_solve"], worst["u_solve"] = absmax(xa[same], xg[same]), absmax(ua[same], ug[same])
        np.testing.assert_allclose(xa[same], xg[same], rtol=1e-7, atol=1e-7, err_msg=label)
        np.testing.assert_allclose(ua[same], ug[same], rtol=1e-6, atol=1e-6, err_msg=label)
    print("measured maxima (%s):" % label, {k: "%.1e" % v for k, v in worst.items()})
    return first


def user_blocks(N):
    return [(1, N, altro_amd.CONE_INEQUALITY, 1, SPHERE_ID), (0, N - 1, altro_amd.CONE_INEQUALITY, 2, SPEED_TILT_ID if N == N_EVAL else SPEED_TILT_SOLVE_ID)]


def sphere_violated(x):
    """per problem: the sphere's row is violated at some knot point k >= 1 of the trajectory x"""
    return (np.linalg.norm(x[:, 1:, :3] - SPHERE_C, axis=2) < SPHERE_R - 1e-3).any(axis=1)


def test_nonlinear_blocks_equal_plan_generic():
    """A keep-out sphere (k = 1..N) and a speed / tilt limit (2 rows, running knot points) from source: two user slots."""
    def make(plan, N=N_EVAL):
        return make_hip(eval_case(False, N, N == N_EVAL), N, plan, QUAD_USER_SRC, user=user_blocks(N))
    (rt, _) = against_generic(make, ALPHAS, eval_case(), N_EVAL, label="sphere + speed/tilt")
    # (alpha = 0: the candidate of phi0's pass is the initial rollout; rt["x"] is the candidate at ALPHAS, whose first entry is 0 too)
    c = eval_case()
    bt = make(TILE)
    bt.open_loop_rollout()
    x0 = bt.get("x")[:, :N_EVAL + 1, :n]
    bt.close()
    assert sphere_violated(x0).sum() >= (BATCH + 1) // 2, sphere_violated(x0)
    v2 = (x0[:, :N_EVAL, 6:9] ** 2).sum(axis=2)
    assert (v2 > VMAX2 + 1e-3).any() and (np.cos(x0[:, :N_EVAL, 3]) * np.cos(x0[:, :N_EVAL, 4]) < TILT_COS - 1e-4).any()
    assert c["x0"].shape[0] == BATCH


def test_wide_table_with_two_user_slots_equals_plan_generic():
    """Input box (1 slot) + state box (3 slots) as data + both user blocks: six slots at a running knot point -- the AL_TILE_MAXC /
    FUSE instantiation of the merit kernel and the six-slot expansion.  Dropping the user slots moves plan GENERIC's phi by more than
    1e-3 relative in every problem."""
    def boxes(N):
        if N == N_EVAL:
            return ts.tables(N, ts.EVAL_UB, ts.EVAL_XB, ts.EVAL_XT, ts.EVAL_CONE, "slots4")
        xb = np.array([3.0] * 3 + [0.6] * 3 + [3.0] * 3 + [1.0] * 3)
        return ts.tables(N, np.array([6.0, 0.2, 0.2, 0.2]), xb, xb, 0.14, "slots4")

    def make(plan, N=N_EVAL, user=True):
        return make_hip(eval_case(False, N, N == N_EVAL), N, plan, QUAD_USER_SRC, data=boxes(N), user=user_blocks(N) if user else ())
    (rt, rg) = against_generic(make, ALPHAS, eval_case(), N_EVAL, label="boxes + sphere + speed/tilt")
    bare = make(GENERIC, user=False)
    rb = phases(bare, eval_case(), RHOS[-1], ALPHAS, gains=False)
    bare.close()
    gap = np.abs(rg["phi"] - rb["phi"]) / np.maximum(1.0, np.abs(rg["phi"]))
    assert gap.min() > 1e-3, gap


def test_dense_cost_with_the_sphere_equals_plan_generic():
    """altro_hip_set_quadratic_cost with the sphere: the DENSE instantiations, single evaluations."""
    def make(plan, N=N_EVAL):
        return make_hip(eval_case(True, N), N, plan, QUAD_USER_SRC, user=user_blocks(N)[:1], dense=True)
    against_generic(make, ALPHAS, eval_case(True), N_EVAL, solve=False, label="dense cost + sphere")


def test_padded_shape_with_a_disc_equals_plan_generic():
    """The (6, 2) planar quadrotor with a disc from source on the flagged tile handle: the caller's 1 x 8 Jacobian lands in tile
    columns 0..5 and 12..13."""
    nn, mm = 6, 2
    hp = np.float32(0.05)
    x0 = np.zeros((BATCH, nn)); x0[:, :2] = DISC_C + 0.4 * problems.normal((BATCH, 2), 641); x0[:, 2] = 0.2 * problems.normal((BATCH,), 142)
    x0[:, 3:5] = 0.3 * problems.normal((BATCH, 2), 642)
    Qd = np.array([2.0, 2.0, 1.0, 0.3, 0.3, 0.1]); Rd = np.array([0.1, 0.1]); uh = np.full(2, 0.5 * 9.81)
    c = dict(u0=uh)
    xg = np.array([1.2, 0.8, 0.0, 0.0, 0.0, 0.0])      # the goal: outside the disc

    def make(plan, N=N_EVAL):
        bt = altro_amd.Batch(N, nn, mm, BATCH, plan=plan, flags=FLAG if plan == TILE else 0)
        assert bt.plan == plan
        bt.set_tracking_cost(np.stack([Qd, 30.0 * Qd]), Rd[None], np.stack([xg, xg]), uh[None], k_stride_zero=True, batch_stride_zero=True)
        bt.set_model_source(PLANAR_USER_SRC, hp)
        assert bt.plan == plan
        bt.add_user_constraint(1, N, altro_amd.CONE_INEQUALITY, 1, 0)
        bt.set_initial_state(x0)
        bt.set_input_guess(uh[None, None], k_stride_zero=True, batch_stride_zero=True)
        return bt
    # (single evaluations: they are what the column mapping shows in.  Whole solves of this case end at the iteration limit or in a failed
    #  search in three of the seven problems on both plans alike, and such solves have no answer at 1e-7: measured 4e-8 and 2e-7 in two runs)
    (rt, _) = against_generic(make, np.linspace(0.05, 1.1, BATCH), c, N_EVAL, nx=nn, solve=False, label="planar + disc")
    inside = (np.linalg.norm(rt["x"][:, 1:, :2] - DISC_C, axis=2) < DISC_R - 1e-3).any(axis=1)
    assert inside.sum() >= (BATCH + 1) // 2, inside


def test_merit_derivative_is_the_derivative_of_the_merit():
    """phi' (the user slot's gradient through the column chain) against a central difference of phi, h = 1e-6: relative error < 1e-5."""
    c = eval_case()
    bt = make_hip(c, N_EVAL, TILE, QUAD_USER_SRC, user=user_blocks(N_EVAL)[:1])
    ts.sweep(bt, c, 50.0)
    worst = 0.0
    for alpha in (0.3, 0.8):
        _, dphi = bt.merit(np.full(BATCH, alpha))
        hs = 1e-6
        pp, _ = bt.merit(np.full(BATCH, alpha + hs), derivative=False)
        pm, _ = bt.merit(np.full(BATCH, alpha - hs), derivative=False)
        fd = (pp - pm) / (2 * hs)
        err = np.abs(dphi - fd) / np.maximum(1.0, np.abs(fd))
        worst = max(worst, float(err.max()))
        assert err.max() < 1e-5, (alpha, err.max(), int(err.argmax()))
    print("measured maximum: %.1e" % worst)
    bt.close()


# ---- 7: flight ------------------------------------------------------------------------------------------------------------------
FLY_C, FLY_R = SPHERE_C, SPHERE_R


FLY_FACTOR, FLY_LATERAL, FLY_N = 2.0, 0.2, 30      # (chosen on the GPU: 60 of 64 converge on plan GENERIC and on the tile)


def flight_case(batch, factor=FLY_FACTOR, lateral=FLY_LATERAL):
    """Every vehicle starts behind the sphere as seen from the goal (the origin), `lateral` off the line through the sphere's centre
    (less than its radius: the straight path crosses it; not zero: a path through the centre is a saddle the solves stall on)."""
    x0 = np.zeros((batch, n))
    side = np.cross(FLY_C, np.array([0.0, 0.0, 1.0])); side /= np.linalg.norm(side)
    x0[:, :3] = factor * FLY_C + lateral * side + 0.05 * problems.normal((batch, 3), 691)
    x0[:, 3:6] = 0.1 * problems.normal((batch, 3), 692)
    x0[:, 6:9] = 0.2 * problems.normal((batch, 3), 693)
    x0[:, 9:] = 0.2 * problems.normal((batch, 3), 694)
    Qd = np.concatenate([np.full(3, 2.0), np.full(3, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
    return dict(x0=x0, Qd=Qd, Qfd=20.0 * Qd, Rd=np.array([0.05, 20.0, 20.0, 20.0]), xref=np.zeros(n), uref=HOVER, u0=HOVER.copy())


def clearance(x):
    return np.linalg.norm(x[:, :, :3] - FLY_C, axis=2).min(axis=1)


def test_quadrotor_flies_around_a_keep_out_sphere_on_the_tile():
    """64 vehicles, N = 30: with the sphere as a one-row block from source every converged trajectory clears it to the feasibility
    tolerance, without it at least a tenth cut through; at least 0.9 x batch converge, on plan GENERIC's solve of the same case too."""
    batch, N = 64, FLY_N
    c = flight_case(batch)
    Gb = np.zeros((2, w)); Gb[0, n] = 1.0; Gb[1, n] = -1.0
    thrust = (0, N - 1, altro_amd.CONE_INEQUALITY, Gb, np.array([1.6 * HOVER[0], -0.4 * HOVER[0]]))
    opts = dict(iterations_max=100, tol_stationarity=1e-3, penalty_initial=10.0)
    clear = {}
    for plan, blocked in ((TILE, False), (TILE, True), (GENERIC, True)):
        bt = make_hip(c, N, plan, QUAD_USER_SRC, data=[thrust], user=[(1, N, altro_amd.CONE_INEQUALITY, 1, SPHERE_ID)] if blocked else ())
        res = bt.ilqr_solve(**opts)
        x, _ = bt.get_nominal()
        ok = res["status"] == 0
        print("flight: plan", plan, "blocked", blocked, "converged", int(ok.sum()), "mean iterations %.1f" % res["iterations"].mean())
        assert ok.sum() >= 0.9 * batch, (plan, blocked, int(ok.sum()))
        if blocked:
            assert (res["feasibility"][ok] < 1e-4).all()
            assert (bt.feasibility()[ok] < 1e-4).all()
        clear[(plan, blocked)] = clearance(x)[ok]
        bt.close()
    assert (clear[(TILE, False)] < FLY_R - 0.01).sum() >= batch // 10, clear[(TILE, False)]
    assert clear[(TILE, True)].min() > np.sqrt(FLY_R ** 2 - 1e-4) - 1e-6, clear[(TILE, True)].min()


# ---- 8: a block added after a solve ------------------------------------------------------------------------------------------------
def test_a_block_added_after_a_solve_is_honoured():
    """Solve with an input box, add the sphere, solve again: the bits of a fresh handle that had both from the start (the module
    compiled for the table with a user slot was launched: the first module's kernels do not evaluate the sphere).  Then
    clear_constraints and two linear blocks: the bits of a fresh handle again (back on the module without user slots)."""
    c = eval_case(False, N_SOLVE, inside=False)
    N = N_SOLVE
    XB8 = np.array([3.0] * 3 + [0.6] * 3 + [3.0] * 3 + [1.0] * 3)
    box_u, box_x = ts.tables(N, np.array([6.0, 0.2, 0.2, 0.2]), XB8, XB8, 0.0, "slots4")
    sphere = (1, N, altro_amd.CONE_INEQUALITY, 1, SPHERE_ID)
    opts = dict(iterations_max=40, tol_stationarity=1e-3, penalty_initial=10.0)

    def restart(bt):
        bt.reset_duals(1.0)   # (a solve starts from the penalty the last one left, as the reference's does: back to a fresh handle's)
        bt.set_initial_state(c["x0"])
        bt.set_input_guess(c["u0"][None, None], k_stride_zero=True, batch_stride_zero=True)

    def solved(bt):
        res = bt.ilqr_solve(**opts)
        return res, bt.get_nominal()

    a = make_hip(c, N, TILE, QUAD_USER_SRC, data=[box_u])
    r1, (x1, _) = solved(a)
    a.add_user_constraint(*sphere)
    restart(a)
    ra, (xa, ua) = solved(a)
    f = make_hip(c, N, TILE, QUAD_USER_SRC, data=[box_u], user=[sphere])
    rf, (xf, uf) = solved(f)
    assert np.array_equal(ra["status"], rf["status"]) and np.array_equal(ra["iterations"], rf["iterations"])
    assert np.array_equal(xa, xf) and np.array_equal(ua, uf)
    assert not np.array_equal(x1, xa)                  # the sphere moved the solution
    assert (np.linalg.norm(xa[ra["status"] == 0][:, 1:, :3] - SPHERE_C, axis=2) > np.sqrt(SPHERE_R ** 2 - 1e-4) - 1e-6).all()
    a.clear_constraints()
    a.add_linear_constraint(*box_u); a.add_linear_constraint(*box_x)
    restart(a)
    rc, (xc, uc) = solved(a)
    g = make_hip(c, N, TILE, QUAD_USER_SRC, data=[box_u, box_x])
    rg, (xg, ug) = solved(g)
    assert np.array_equal(rc["status"], rg["status"]) and np.array_equal(rc["iterations"], rg["iterations"])
    assert np.array_equal(xc, xg) and np.array_equal(uc, ug)
    for h in (a, f, g):
        h.close()


# ---- 9: the surface -----------------------------------------------------------------------------------------------------------------
def test_the_surface_says_what_it_takes():
    c = eval_case()
    ineq = altro_amd.CONE_INEQUALITY
    # the flag on an explicit MFMA16 handle accepts the source; on an AUTO handle the plan stays MFMA16
    for plan in (TILE, altro_amd.PLAN_AUTO):
        bt = altro_amd.Batch(N_EVAL, n, m, BATCH, plan=plan, flags=FLAG)
        bt.set_model_source(QUAD_USER_SRC, H)
        assert bt.plan == TILE
        assert bt.add_user_constraint(1, N_EVAL, ineq, 1, SPHERE_ID) == 0
        assert bt.get_duals(N_EVAL, 0, 1).shape == (BATCH, 1)
        bt.close()
    # capacities: errors name the cap
    bt = make_hip(c, N_EVAL, TILE, QUAD_USER_SRC)
    with pytest.raises(altro_amd.AltroHipError, match=r"1 \.\. 8 rows"):
        bt.add_user_constraint(0, N_EVAL - 1, ineq, 9, 1)
    with pytest.raises(altro_amd.AltroHipError, match=r"1 \.\. 4 rows"):
        bt.add_user_constraint(0, N_EVAL - 1, altro_amd.CONE_SOC, 5, 3)
    bt.add_user_constraint(0, N_EVAL - 1, ineq, 2, SPEED_TILT_ID)
    bt.add_user_constraint(1, N_EVAL, ineq, 1, SPHERE_ID)
    with pytest.raises(altro_amd.AltroHipError, match="AL_TILE_USER_MAXC"):
        bt.add_user_constraint(3, 5, ineq, 2, 0)
    G32 = np.zeros((32, w)); G32[np.arange(32), np.arange(32) % w] = 1.0
    bt.add_linear_constraint(0, N_EVAL - 1, ineq, G32, np.ones(32))          # four more slots: six at k = 1 .. N - 1
    with pytest.raises(altro_amd.AltroHipError, match="at most 6 constraint slots"):
        bt.add_linear_constraint(2, 2, ineq, G32[:1], np.ones(1))
    # an LDS comparison form with a user block: unsupported
    for form in (altro_amd.FORM_MERIT_LDS, altro_amd.FORM_ALROWS_LDS, altro_amd.FORM_EXPAND_LDS):
        bt.set_forms(form)
        with pytest.raises(altro_amd.AltroHipError, match=r"error -\d+: constraint blocks from source on plan MFMA16"):
            bt.open_loop_rollout(); bt.accept(); bt.expand(); bt.feasibility(); bt.merit(np.zeros(BATCH))
    bt.set_forms(0)
    bt.close()
    # the slot layout through altro_hip_get_duals: blocks in the order they were registered (data first here, then from source), a block's
    # duals [batch][p] whatever slots it takes; the table's fill has no path without the HIP runtime, so this stands in for a CPU test
    boxes = ts.tables(N_EVAL, ts.EVAL_UB, ts.EVAL_XB, ts.EVAL_XT, ts.EVAL_CONE, "slots4")
    bt = make_hip(c, N_EVAL, TILE, QUAD_USER_SRC, data=boxes, user=user_blocks(N_EVAL))
    for k, shapes in ((0, (8, 24, 2)), (1, (8, 24, 1, 2)), (N_EVAL, (1,))):      # (the sphere starts at k = 1 and is the terminal knot point's only block)
        for slot, p in enumerate(shapes):
            z = bt.get_duals(k, slot, p)
            assert z.shape == (BATCH, p) and (z == 0.0).all()
        with pytest.raises(altro_amd.AltroHipError, match="no constraint block"):
            bt.get_duals(k, len(shapes), 1)
    res = bt.ilqr_solve(iterations_max=6, tol_stationarity=1e-3)
    zs = np.concatenate([bt.get_duals(k, 2, 1) for k in range(1, N_EVAL)] + [bt.get_duals(k, 3, 2) for k in range(1, N_EVAL)], axis=1)
    assert (zs <= 0.0).all()                          # the orthant's duals, in the user blocks' places
    assert (res["dual_updates"] == 0).all() or (zs < 0.0).any()
    bt.reset_duals(1.0)
    assert (bt.get_duals(1, 2, 1) == 0.0).all()
    bt.clear_constraints()
    with pytest.raises(altro_amd.AltroHipError, match="no constraint block"):
        bt.get_duals(1, 0, 1)
    bt.close()
    # the blocks from source take none of the handle's 32 padded slot definitions: 32 one-row blocks of data fit next to two of them
    bt = make_hip(c, N_EVAL, TILE, QUAD_USER_SRC, user=user_blocks(N_EVAL))
    for i in range(32):
        bt.add_linear_constraint(2 + i // 4, 2 + i // 4, ineq, G32[:1], np.ones(1))
    with pytest.raises(altro_amd.AltroHipError, match="at most 32 constraint slots"):
        bt.add_linear_constraint(0, 0, ineq, G32[:1], np.ones(1))
    bt.close()
    # fp32 records: refused
    f32 = altro_amd.Batch(N_EVAL, n, m, BATCH, dtype=altro_amd.F32, plan=TILE, flags=FLAG)
    with pytest.raises(altro_amd.AltroHipError, match="fp64"):
        f32.set_model_source(QUAD_USER_SRC, H)
    f32.close()
    # a source without the pair: ALTRO_HIP_ERR_NOT_SET
    plain = altro_amd.Batch(N_EVAL, n, m, BATCH, plan=TILE, flags=FLAG)
    plain.set_model_source(QUADROTOR_SRC, H)
    with pytest.raises(altro_amd.AltroHipError, match=r"error -5: altro_hip_set_model_source must come first"):
        plain.add_user_constraint(0, N_EVAL, ineq, 1, 0)
    plain.close()
    # half the pair names the other half
    half = QUAD_USER_SRC.split("template <typename T> __device__ void altro_user_constraint_jacobian")[0]
    hb = altro_amd.Batch(N_EVAL, n, m, BATCH, plan=TILE, flags=FLAG)
    with pytest.raises(altro_amd.AltroHipError, match="altro_user_constraint_jacobian"):
        hb.set_model_source(half, H)
    hb.close()
