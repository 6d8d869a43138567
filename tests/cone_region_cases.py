"""Configurations that put the conic augmented-Lagrangian terms into EVERY region of every cone, with the oracle's side of the
comparison (numpy and the oracle only: no GPU, imported by tests/test_cone_region_cases.py and tests/test_gpu_cone_regions.py).

The oracle decides per block from ze = z - rho c (oracle/al_oracle.c, cones.cpp:13-123): a second-order cone with v = ze[:-1],
s = ze[-1], a = ||v|| is BELOW (a <= -s: projection 0), INSIDE (a <= s: identity) or OUTSIDE; an orthant row is active when ze <= 0.
The projection is continuous across a == s, a == -s and ze == 0, its Jacobian is not: a `<` written for `<=` shows only in the
Hessian blocks and the gains.  Classes, with zero duals (ze = -rho c):
  second-order cone  below, inside, out_pos / out_neg / out_zero (outside with s > 0, < 0, == 0), apex (c == 0), v0_pos / v0_neg
                     (v == 0 with s of either sign), tie_in (a == s > 0), tie_below (a == -s > 0)
  orthant row        neg (val < 0), pos (val > 0), zero (val == 0)

A trajectory guess (set_state_guess / set_input_guess) steers every (problem, knot point) into a scheduled class; one block per cone
and range of knot points.  How a cone block is made (cone_block):
  * its last row reads a state of its own (svar), c_s = x[svar] - 0.5: s is steered without touching any other row or block;
  * the rows of v are dense over `vvars` (never an svar), except the column of one variable, `tie_var`, which holds an integer
    pattern t with ||t|| an integer -- (3), (3, 4, 0, ...) or sixteen ones spread over the rows -- and g_v = t.  With every vvar zero
    and tie_var = 2: v = t exactly, a = ||t|| exactly under any order of summation, and s = +-a is exact: the ties.  tie_var = 1:
    v = 0 (apex, v0_*).  Any other point is a generic one: a from the dense rows, s = a times a factor (a >= 0.1 where the class is an
    outside one, so that 1 / a does not set the tolerance).
An orthant block has entries that are multiples of 1/8; at its tie the variables it reads are integers and g[0] is row 0's value
there: val[0] == 0 exactly.  At most one block is at a special class (a tie, apex, v == 0) at one (problem, knot point).

Penalties 1 and 50: the ties stay exact (integers times 50).  N = 5 with cones over the states at the terminal knot point, batch 7
(the tile and the row layout put two problems in a wave: the last wave is ragged).  The horizon is a property of a configuration
(Config.N): HORIZON_CONFIGS are the tile's two at N = 17 and N = 33, nothing else changed.
"""
import functools

import numpy as np

from oracle import oracle
from tests import problems

BATCH, N = 7, 5
RHOS = (1.0, 50.0)
ALPHAS = np.linspace(0.15, 1.1, BATCH)
SOC_SPECIAL = ("apex", "v0_pos", "v0_neg", "tie_in", "tie_below")
SOC_GENERIC = ("below", "inside", "out_pos", "out_neg", "out_zero")
SOC_CLASSES = SOC_GENERIC + SOC_SPECIAL
ORTH_CLASSES = ("neg", "pos", "zero")
G_S = 0.5                                   # g of a cone's last row
# generic classes: c_s as a multiple of a (ze_s = -rho c_s)
S_FACTOR = {"below": 2.0, "inside": -2.0, "out_pos": -0.5, "out_neg": 0.5, "out_zero": 0.0}
H_DI = np.float32(0.1)


# ---- sums in the orders a kernel may take ------------------------------------------------------------------------------------
def seq_sum(v):
    acc = 0.0
    for e in v:
        acc += float(e)
    return acc


def pair_sum(v):
    v = [float(e) for e in v]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else 0.0


def values(G, g, z):
    """c = G z - g in the oracle's order of summation."""
    return np.array([seq_sum(G[i] * z) - g[i] for i in range(G.shape[0])])


def classify_soc(ze):
    """(region, class) of ze in the oracle's order of comparisons (oracle_cone_projection)."""
    v, s = ze[:-1], float(ze[-1])
    a = np.sqrt(seq_sum(v * v))
    region = "below" if a <= -s else ("inside" if a <= s else "outside")
    if a == 0.0:
        cls = "apex" if s == 0.0 else ("v0_pos" if s > 0 else "v0_neg")
    elif a == s:
        cls = "tie_in"
    elif a == -s:
        cls = "tie_below"
    elif region == "outside":
        cls = "out_zero" if s == 0.0 else ("out_pos" if s > 0 else "out_neg")
    else:
        cls = region
    if cls in ("tie_in", "tie_below"):
        assert np.sqrt(pair_sum(v * v)) == abs(s) and a == abs(s), (a, s)       # exact whatever the order of the sum
    return region, cls, a


def classify_orth(ze):
    """Per row: the class of val = -ze / rho by sign (active: ze <= 0)."""
    return ["zero" if e == 0.0 else ("pos" if e < 0 else "neg") for e in ze]


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def tie_pattern(rows):
    t = np.zeros(rows)
    if rows >= 16:
        t[np.round(np.linspace(0, rows - 1, 16)).astype(int)] = 1.0             # norm 4
    elif rows >= 2:
        t[0], t[1] = 3.0, 4.0                                                   # norm 5
    else:
        t[0] = 3.0
    assert np.sqrt(seq_sum(t * t)) == round(np.sqrt(seq_sum(t * t)))
    return t


def cone_block(name, p, k0, k1, w, svar, vvars, tie_var, rng):
    assert tie_var in vvars and svar not in vvars
    G = np.zeros((p, w))
    G[:p - 1, vvars] = rng.normal(size=(p - 1, len(vvars)))
    t = tie_pattern(p - 1)
    G[:p - 1, tie_var] = t
    G[p - 1, svar] = 1.0
    g = np.concatenate([t, [G_S]])
    return dict(kind="soc", name=name, p=p, k0=k0, k1=k1, cone=oracle.CONE_SOC, G=G, g=g, svar=svar, vvars=list(vvars), tie_var=tie_var,
                norm=float(np.sqrt(seq_sum(t * t))))


def box_block(name, k0, k1, n, m, bound):
    """|u_i| <= bound: a bound-type block (one entry of +-1 per row)."""
    G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
    return dict(kind="orth", name=name, p=2 * m, k0=k0, k1=k1, cone=oracle.CONE_INEQUALITY, G=G, g=np.full(2 * m, bound), reads=[n], box=True)


def dense_orth_block(name, rows, k0, k1, w, reads, rng):
    G = np.zeros((rows, w))
    G[:, reads] = np.round(8.0 * rng.uniform(-1.0, 1.0, size=(rows, len(reads)))) / 8.0
    G[0, reads[0]] = 0.5                                                       # (row 0 is never empty)
    g = np.round(8.0 * rng.uniform(-0.5, 1.0, size=rows)) / 8.0
    return dict(kind="orth", name=name, p=rows, k0=k0, k1=k1, cone=oracle.CONE_INEQUALITY, G=G, g=g, reads=list(reads), box=False)


def eq_block(name, k0, k1, w, var, value):
    G = np.zeros((1, w)); G[0, var] = 1.0
    return dict(kind="eq", name=name, p=1, k0=k0, k1=k1, cone=oracle.CONE_EQUALITY, G=G, g=np.array([value]))


class Config:
    def __init__(self, name, plan, n, m, dyn, dense, blocks, seed, N=N, base=None):
        self.name, self.plan, self.n, self.m, self.dyn, self.dense, self.blocks = name, plan, n, m, dyn, dense, blocks
        self.N, self.base = N, base or name    # the horizon; the configuration this one differs from by its horizon alone
        self.w = n + m
        if dyn == "data":
            self.p = problems.ilqr12x4_problem(BATCH, N, True, n=n, m=m)
            if dense:
                self.p.update(problems.quadratic_cost(BATCH, N, n, m))
        else:
            self.Qd, self.Rd, self.xref = np.full(n, 1.0), np.full(m, 0.1), 0.3 * problems.normal((n,), 7 + seed)
        self.schedule = {}                    # (block index, b, k) -> scheduled class (cones; an orthant block's tie)
        self._steer(seed)

    def slots(self, j):
        bl = self.blocks[j]
        return [(b, k) for k in range(bl["k0"], bl["k1"] + 1) for b in range(BATCH)]

    def at(self, k):
        """Indices of the blocks of knot point k, in the order they are registered: block `slot` of get_duals / ILQR.duals."""
        return [j for j, bl in enumerate(self.blocks) if bl["k0"] <= k <= bl["k1"]]

    def _steer(self, seed):
        n, m, w, N = self.n, self.m, self.w, self.N
        z = 0.7 * problems.normal((BATCH, N + 1, w), 300 + seed)
        z[:, N, n:] = 0.0                                                      # (no inputs at the terminal knot point)
        taken = set()

        def claim(j, cls, order):
            for i in order:
                if self.slots(j)[i] not in taken:
                    taken.add(self.slots(j)[i]); self.schedule[(j,) + self.slots(j)[i]] = cls
                    return
            raise AssertionError("no free (problem, knot point) for %s of %s" % (cls, self.blocks[j]["name"]))

        # special classes: every one once per running cone; spread round-robin over the cones of the terminal knot point
        term = [j for j, bl in enumerate(self.blocks) if bl["kind"] == "soc" and bl["k0"] == N]
        for j, bl in enumerate(self.blocks):
            cnt = len(self.slots(j))
            order = [(11 * i + 3 * j) % cnt for i in range(cnt)]
            if bl["kind"] == "soc" and bl["k0"] < N:
                for cls in SOC_SPECIAL:
                    claim(j, cls, order)
            elif bl["kind"] == "orth":
                claim(j, "zero", order)
        for i, cls in enumerate(SOC_SPECIAL if term else ()):
            claim(term[i % len(term)], cls, list(range(BATCH)))
        # generic classes everywhere else
        for j, bl in enumerate(self.blocks):
            if bl["kind"] != "soc":
                continue
            i = 0
            for (b, k) in self.slots(j):
                if (j, b, k) not in self.schedule:
                    self.schedule[(j, b, k)] = SOC_GENERIC[(i + j) % len(SOC_GENERIC)]
                    i += 1
        # the points: special blocks first (they fix the variables other blocks read), then every cone's own s
        rng = np.random.default_rng(1000 + seed)
        for (j, b, k), cls in self.schedule.items():
            bl = self.blocks[j]
            if bl["kind"] == "orth":
                if bl["box"]:
                    z[b, k, bl["reads"][0]] = bl["g"][0]
                else:
                    z[b, k, bl["reads"]] = rng.integers(-2, 3, size=len(bl["reads"]))
                    bl["g"][0] = seq_sum(bl["G"][0] * z[b, k])
            elif cls in SOC_SPECIAL:
                z[b, k, bl["vvars"]] = 0.0
                z[b, k, bl["tie_var"]] = 2.0 if cls.startswith("tie") else 1.0
        cones = [bl for bl in self.blocks if bl["kind"] == "soc"]
        for k in range(N + 1):                                                 # a >= 0.1 at the generic points: draw those again that miss it
            for b in range(BATCH):
                here = [bl for bl in cones if bl["k0"] <= k <= bl["k1"]]
                norm = lambda bl: np.sqrt(seq_sum(values(bl["G"][:-1], bl["g"][:-1], z[b, k]) ** 2))
                while (b, k) not in taken and any(norm(bl) < 0.1 for bl in here):
                    z[b, k, :n if k == N else w] = 0.7 * rng.normal(size=n if k == N else w)
        for (j, b, k), cls in self.schedule.items():
            bl = self.blocks[j]
            if bl["kind"] != "soc":
                continue
            if cls in SOC_GENERIC:
                v = values(bl["G"][:-1], bl["g"][:-1], z[b, k])
                a = float(np.sqrt(seq_sum(v * v)))
                assert a >= 0.1, (self.name, bl["name"], b, k, a)
                cs = S_FACTOR[cls] * a
            else:
                cs = {"apex": 0.0, "v0_pos": -1.0, "v0_neg": 1.0, "tie_in": -bl["norm"], "tie_below": bl["norm"]}[cls]
            z[b, k, bl["svar"]] = G_S + cs
        self.x = np.ascontiguousarray(z[:, :, :n])
        self.u = np.ascontiguousarray(z[:, :N, n:])
        # the initial state: the guess's own on plan LANE; the problem's -- NOT the guess's x_0, as SetState allows -- with dynamics as data
        self.x0 = np.ascontiguousarray(self.x[:, 0] if self.dyn == "di" else self.p["x0"])
        self.u_start = np.ascontiguousarray(self.u if self.dyn == "di" else self.p["u0"])       # the input guess whole solves start from

    def z(self, b, k, x=None, u=None):
        x = self.x if x is None else x
        u = self.u if u is None else u
        return np.concatenate([x[b, k], u[b, k] if k < self.N else np.zeros(self.m)])

    def classes(self, rho=1.0, x=None, u=None, duals=None, rhos=None):
        """{(block, b, k): (region, class, a)} for cones, {...: [class per row]} for orthant blocks, from G, g, x, u, z, rho."""
        out = {}
        for j, bl in enumerate(self.blocks):
            if bl["kind"] == "eq":
                continue
            for (b, k) in self.slots(j):
                zd = np.zeros(bl["p"]) if duals is None else duals[(j, b, k)]
                r = rho if rhos is None else rhos[(j, b, k)]
                ze = zd - r * values(bl["G"], bl["g"], self.z(b, k, x, u))
                out[(j, b, k)] = classify_soc(ze) if bl["kind"] == "soc" else classify_orth(ze)
        return out


def _vars(lo, hi, skip=()):
    return [i for i in range(lo, hi) if i not in skip]


def _cones_everywhere(n, m, ps, rng, extra_run=(), extra_term=(), N=N):
    """Cones of ps[i] rows with svar = state i: one block over states and inputs at k < N, one over the states at k = N."""
    w = n + m
    sv = list(range(len(ps)))
    run = [cone_block("cone%d" % p, p, 0, N - 1, w, i, _vars(len(ps), w), len(ps) + i, rng) for i, p in enumerate(ps)]
    term = [cone_block("cone%d_N" % p, p, N, N, w, i, _vars(len(ps), n), len(ps) + i, rng) for i, p in enumerate(ps)]
    assert all(s not in bl["vvars"] for bl in run + term for s in sv)
    return run + list(extra_run) + term + list(extra_term)


@functools.lru_cache(maxsize=None)
def config(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("lane_4_2", "lane_6_3"):
        # plan LANE: two blocks per knot point -- cones of 2 and 3 rows at k = 0, 1, of 4 rows and a dense orthant block at k = 2 .. 4, two at k = N
        n, m = (4, 2) if name == "lane_4_2" else (6, 3)
        w = n + m
        blocks = [cone_block("cone2", 2, 0, 1, w, 0, _vars(2, w), 2, rng), cone_block("cone3", 3, 0, 1, w, 1, _vars(2, w), 3, rng),
                  cone_block("cone4", 4, 2, 4, w, 0, _vars(1, w), 1, rng), dense_orth_block("orth", 4, 2, 4, w, _vars(1, w), rng),
                  cone_block("cone%d_N" % (3 if n == 4 else 2), 3 if n == 4 else 2, N, N, w, 0, _vars(2, n), 2, rng),
                  cone_block("cone4_N", 4, N, N, w, 1, _vars(2, n), 3, rng)]
        return Config(name, "LANE", n, m, "di", False, blocks, 1 if n == 4 else 2)
    if name in ("tile_tracking", "tile_dense"):
        return _tile(name, name, N, rng)
    if name in HORIZON_CONFIGS:
        # the tile's two configurations at horizons of two and three chunks of the affine trials (the last chunk one knot point plus the
        # terminal one): the same blocks from the same draws, so the same special classes and exact ties, spread over more slots
        base, horizon = name.rsplit("_n", 1)
        return _tile(name, base, int(horizon), np.random.default_rng(sum(map(ord, base))))
    if name == "generic_14_5":
        n, m = 14, 5
        w = n + m
        blocks = _cones_everywhere(n, m, (4, 5, 17, 32), rng, extra_run=[box_block("box", 0, N - 1, n, m, 0.375),
                                                                          dense_orth_block("orth9", 9, 0, N - 1, w, _vars(4, w), rng)])
        return Config(name, "GENERIC", n, m, "data", True, blocks, 4)
    if name == "auto32_cones":
        n, m = 13, 4
        return Config(name, "MFMA32", n, m, "data", False, _cones_everywhere(n, m, (5, 18), rng), 5)
    if name == "auto32_rows":
        # orthant / equality blocks only: kernels/ilqr_row32.hip serves the handle
        n, m = 13, 4
        w = n + m
        Gx = np.zeros((2 * n, w)); Gx[:n, :n] = np.eye(n); Gx[n:, :n] = -np.eye(n)
        blocks = [box_block("box", 0, N - 1, n, m, 0.375), dense_orth_block("orth11", 11, 0, N - 1, w, _vars(0, w), rng),
                  eq_block("pin", 0, 0, w, n, 0.125),
                  dict(kind="orth", name="box_N", p=2 * n, k0=N, k1=N, cone=oracle.CONE_INEQUALITY, G=Gx, g=np.full(2 * n, 0.375), reads=[0], box=True)]
        return Config(name, "MFMA32", n, m, "data", True, blocks, 6)
    raise KeyError(name)


def _tile(name, base, N, rng):
    n, m = 12, 4
    w = n + m
    blocks = _cones_everywhere(n, m, (2, 3, 4), rng, extra_run=[box_block("box", 0, N - 1, n, m, 0.375),
                                                                  dense_orth_block("orth12", 12, 0, N - 1, w, _vars(3, w), rng)], N=N)
    return Config(name, "MFMA16", n, m, "data", base == "tile_dense", blocks, 3, N=N, base=base)


CONFIGS = ("lane_4_2", "lane_6_3", "tile_tracking", "tile_dense", "generic_14_5", "auto32_cones", "auto32_rows")
HORIZON_CONFIGS = ("tile_tracking_n17", "tile_dense_n17", "tile_tracking_n33", "tile_dense_n33")     # (not part of CONFIGS: judged on the merit phase)


# ---- the oracle's side -----------------------------------------------------------------------------------------------------------
def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def make_oracle(cfg, b, g_of=None):
    """The oracle's handle of problem b: dynamics, cost, x0, the blocks in registration order.  g_of: {block index: g} overrides."""
    n, m, N = cfg.n, cfg.m, cfg.N
    if cfg.dyn == "di":
        s = oracle.ILQR(N, n, m, H_DI, oracle.DYN_MODEL, oracle.MODEL_DI, model_dim=m, cost_kind=oracle.COST_DIAGONAL)
        for k in range(N + 1):
            s.L.oracle_ilqr_set_lqr_cost(s.h, k, _c(cfg.Qd), _c(cfg.Rd), _c(cfg.xref), np.zeros(m))
    else:
        p = cfg.p
        s = oracle.ILQR(N, n, m, 0.01, oracle.DYN_LINEAR, cost_kind=oracle.COST_QUADRATIC if cfg.dense else oracle.COST_DIAGONAL)
        s.L.oracle_ilqr_set_linear_dynamics(s.h, _c(p["A"][b]), _c(p["B"][b]), _c(p["f"][b]).ctypes.data)
        for k in range(N + 1):
            kk = min(k, N - 1)
            if cfg.dense:
                s.L.oracle_ilqr_set_quadratic_cost(s.h, k, _c(p["Q"][b, k]), _c(p["R"][b, kk]).ctypes.data, _c(p["H"][b, kk]).ctypes.data,
                                                   _c(p["q"][b, k]), _c(p["r"][b, kk]).ctypes.data, float(p["c"][b, k]))
            else:
                s.L.oracle_ilqr_set_lqr_cost(s.h, k, _c(p["Qd"][b, k]), _c(p["Rd"][b, kk]), _c(p["xref"][b, k]), _c(p["uref"][b, kk]))
    s.L.oracle_ilqr_set_initial_state(s.h, _c(cfg.x0[b]))
    for k in range(N + 1):
        for j in cfg.at(k):
            bl = cfg.blocks[j]
            s.add_linear_constraint(k, bl["cone"], bl["G"], bl["g"] if not g_of or j not in g_of else g_of[j])
    s.L.oracle_ilqr_initialize(s.h)
    return s


def set_guess(s, cfg, b, x=None, u=None):
    x = cfg.x if x is None else x
    u = cfg.u if u is None else u
    N = cfg.N
    for k in range(N + 1):
        s.L.oracle_ilqr_set_state(s.h, k, _c(x[b, k]))
    for k in range(N):
        s.L.oracle_ilqr_set_input(s.h, k, _c(u[b, k]))


def expand(s):
    """CopyTrajectory, constraint values and projected duals, the expansions of dynamics and cost: what accept + expand do."""
    s.L.oracle_ilqr_copy_trajectory(s.h)
    s.L.oracle_ilqr_calc_cost(s.h)
    s.L.oracle_ilqr_calc_dynamics_expansions(s.h); s.L.oracle_ilqr_calc_cost_gradient(s.h)
    s.L.oracle_ilqr_calc_expansions(s.h)


def oracle_sweep(cfg, b, rho, x=None, u=None, g_of=None):
    """The guess accepted, zero duals at penalty rho, expansion: the oracle ready for the backward pass."""
    s = make_oracle(cfg, b, g_of)
    set_guess(s, cfg, b, x, u)
    if rho != 1.0:                                   # every block's penalty: 1 (Initialize) times rho
        s.set_penalty(1.0, rho)
        s.L.oracle_ilqr_penalty_update(s.h)
    expand(s)
    return s


def phases(s, alpha):
    """Everything part a compares, in the order the handle's calls produce it (s: expanded)."""
    r = dict(lx=s.get("lx"), lu=s.get("lu"))
    assert s.L.oracle_ilqr_backward_pass(s.h) == -1
    for key in ("K", "d", "P", "p"):
        r[key] = s.get(key)
    r["phi0"], r["dphi0"] = s.merit(0.0)
    r["phi"], r["dphi"] = s.merit(alpha)
    r["x"], r["u"] = s.get("x_cand"), s.get("u_cand")
    r["feas"] = s.feasibility()
    r["stat"] = s.L.oracle_ilqr_stationarity(s.h)
    return r


@functools.lru_cache(maxsize=None)
def zero_dual_reference(name):
    """{(rho, b): phases} of configuration `name` at its steered guess with zero duals."""
    cfg = config(name)
    return {(rho, b): phases(oracle_sweep(cfg, b, rho), ALPHAS[b]) for rho in RHOS for b in range(BATCH)}


def gains(cfg, b, rho, x=None, u=None, g_of=None):
    s = oracle_sweep(cfg, b, rho, x, u, g_of)
    assert s.L.oracle_ilqr_backward_pass(s.h) == -1
    return s.get("K")


def knot_hessian(bl, n, m, zvec, zd, rho, g=None):
    """oracle_al_knot_eval's (n + m)^2 Hessian block of one constraint block at one point."""
    L = oracle.lib()
    p = bl["p"]
    Gc = _c(bl["G"].T); g = _c(bl["g"] if g is None else g); x = _c(zvec[:n]); u = _c(zvec[n:]); zd = _c(zd)
    lx = np.zeros(n); lu = np.zeros(m); lxx = np.zeros(n * n); luu = np.zeros(m * m); lux = np.zeros(n * m)
    hess = np.zeros((n + m) * (n + m)); val = np.zeros(p)
    L.oracle_al_knot_eval(bl["cone"], p, n, m, Gc.ctypes.data, g.ctypes.data, x.ctypes.data, u.ctypes.data, zd.ctypes.data, float(rho),
                          lx.ctypes.data, lu.ctypes.data, lxx.ctypes.data, luu.ctypes.data, lux.ctypes.data, hess.ctypes.data, val.ctypes.data)
    return hess.reshape(n + m, n + m)


def curvature_term(bl, zvec, zd, rho):
    """rho G^T (d/dz J^T z_proj) G of a second-order cone block: the Hessian's second term (knotpoint_data.cpp:549-570)."""
    L = oracle.lib()
    p = bl["p"]
    ze = _c(zd - rho * values(bl["G"], bl["g"], zvec))
    zp = np.zeros(p); Hs = np.zeros(p * p)
    L.oracle_cone_projection(oracle.CONE_SOC, p, ze.ctypes.data, zp.ctypes.data)
    L.oracle_cone_hessian(oracle.CONE_SOC, p, ze.ctypes.data, zp.ctypes.data, Hs.ctypes.data)
    return rho * bl["G"].T @ Hs.reshape(p, p) @ bl["G"]


# ---- nonzero duals: a truncated solve, then a guess steered from the oracle's duals and penalties -------------------------------------
# Sweeps of the truncated solves, chosen with the oracle's log (tests/test_cone_region_cases.py asserts it): by then every problem has
# taken a dual update and no line search was rounding-limited (>= 8 evaluations or a step below 1e-2).
SOLVE_SWEEPS = {"lane_4_2": 5, "lane_6_3": 5, "tile_tracking": 4, "tile_dense": 4, "generic_14_5": 4, "auto32_cones": 4, "auto32_rows": 4}
REGION_FACTOR = {"below": -2.0, "inside": 2.0, "outside": (0.5, -0.5)}            # ze_s as a multiple of a = ||ze_v||


def steer_from_duals(cfg, duals, rhos, seed):
    """A guess that puts ze = z - rho c of every cone block into a scheduled region (below, inside, outside in turn; no ties: a comes
    from dense rows and duals with all their digits).  duals / rhos: {(block, b, k): z / rho}.  Returns x, u, {(block, b, k): region}."""
    n, m, w, N = cfg.n, cfg.m, cfg.w, cfg.N
    z = 0.7 * problems.normal((BATCH, N + 1, w), 500 + seed)
    z[:, N, n:] = 0.0
    want = {}
    for j, bl in enumerate(cfg.blocks):
        if bl["kind"] != "soc":
            continue
        for i, (b, k) in enumerate(cfg.slots(j)):
            region = ("below", "inside", "outside")[(i + j) % 3]
            zd, rho = duals[(j, b, k)], rhos[(j, b, k)]
            zev = zd[:-1] - rho * values(bl["G"][:-1], bl["g"][:-1], z[b, k])
            a = float(np.sqrt(seq_sum(zev * zev)))
            assert a >= 0.1, (cfg.name, bl["name"], b, k, a)
            f = REGION_FACTOR[region]
            f = f[(i // 3) % 2] if isinstance(f, tuple) else f
            z[b, k, bl["svar"]] = G_S + (zd[-1] - f * a) / rho
            want[(j, b, k)] = region
    return np.ascontiguousarray(z[:, :, :n]), np.ascontiguousarray(z[:, :N, n:]), want


@functools.lru_cache(maxsize=None)
def nonzero_dual_reference(name):
    """The oracle's truncated solve of every problem from the rollout of cfg.u_start, its duals and penalties, the guess steered from
    them and the phases there (duals kept).  Returns dict(status, iterations, dual_updates, log, duals, rhos, x, u, want, phases)."""
    cfg = config(name)
    N = cfg.N
    sweeps = SOLVE_SWEEPS[name]
    out = dict(status=[], iterations=[], dual_updates=[], log=[], duals={}, rhos={}, handles=[])
    for b in range(BATCH):
        s = make_oracle(cfg, b)
        for k in range(N):
            s.L.oracle_ilqr_set_input(s.h, k, _c(cfg.u_start[b, k]))
        s.set_penalty(1.0, 10.0)
        s.L.oracle_ilqr_set_options(s.h, sweeps, 1e-4, 1e-4, 1e-8, 0)
        status, iters, log = s.solve()
        log = log[:min(iters, sweeps)]
        out["status"].append(status); out["iterations"].append(iters); out["log"].append(log)
        out["dual_updates"].append(int((log[:, 4] < 1e-2).sum()))               # solver.cpp:474: a dual update after every sweep that ends this stationary
        for k in range(N + 1):
            for slot, j in enumerate(cfg.at(k)):
                out["duals"][(j, b, k)] = s.duals(k, slot); out["rhos"][(j, b, k)] = s.penalty(k, slot)
        out["handles"].append(s)
    out["x"], out["u"], out["want"] = steer_from_duals(cfg, out["duals"], out["rhos"], len(name))
    out["phases"] = []
    for b, s in enumerate(out.pop("handles")):
        set_guess(s, cfg, b, out["x"], out["u"])
        expand(s)
        out["phases"].append(phases(s, ALPHAS[b]))
    return out
