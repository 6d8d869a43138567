"""The iLQR loop's phases under a change of units, and the no-floor metric they are judged by (numpy and the oracle only: no GPU, no
mpmath; shared by tests/test_loop_scale_cases.py, tests/test_gpu_loop_scales.py and tests/golden/make_loop_phase_fixtures.py).

A change of units T = (k, D, E): s = 4^k scales the cost, D (n) and E (m) hold powers of two, x~ = D x, u~ = E u.  The inputs map as
  A -> D A D^-1, B -> D B E^-1, f -> D f;   Q -> s D^-1 Q D^-1, R -> s E^-1 R E^-1, H -> s E^-1 H D^-1, q -> s D^-1 q, r -> s E^-1 r,
  c -> s c;   tracking form: Qd -> s Qd / D^2, Rd -> s Rd / E^2, xref -> D xref, uref -> E uref;   x0 and the guesses like x, u;
  G -> G diag(D, E)^-1, g unchanged;   rho -> s rho (the caller's: RHOS times `scale` of the transformed configuration)
and the outputs map back as
  lx = D lx~ / s, lu = E lu~ / s, K = E^-1 K~ D, d = E^-1 d~, P = D P~ D / s, p = D p~ / s, phi = phi~ / s, phi' = phi'~ / s,
  x = D^-1 x~, u = E^-1 u~, feasibility unchanged, stationarity / s (an inf-norm over coordinates: covariant under k alone).
Every factor is a power of two and s a power of FOUR (the factorisation takes a square root of Quu ~ s), so each mapped input is exact,
every IEEE operation, FMA and summation order commutes with the map, and the mapped-back result is the unscaled one BIT FOR BIT --
unless something absolute hides in a phase.  The constraint values c = G~ [x~; u~] - g are bit-identical, so every cone region and
every exact tie of tests/cone_region_cases.py survives the map (transform asserts it).

The metric: hard_cases.blockerr per (problem, knot point) block -- no floor of 1; each scalar (phi, phi', feasibility, stationarity)
is its own block; a block that is exactly zero in the reference must be exactly zero.  Criterion B judges a result `got` in the
old units by  blockerr(got, fixture) <= 10 max(e_cpu, 1e-13)  per quantity and penalty, e_cpu the oracle's STORED error against
the extended-precision fixture (tests/golden/loop_phases_<config>.npz).

Nonzero duals and the dual update (the second half of the module; tests/test_gpu_dual_scales.py, tests/golden/loop_phases_duals_<config>.npz).
Constraint values are unit-free, so duals map as z~ = s z and penalties as rho~ = s rho; `back` takes z~ / s per block, rho~ / s and
alpha unchanged; penalty_max -> s penalty_max and tol_meritfun_gradient -> s tol.  A STATE is what a caller writes onto a handle:
dict(z={block name: [BATCH, knot points of the block, p]}, rho=[BATCH] the penalty the handle holds, x, u the guess).
  S1 (dual_state)    after a truncated solve: cone_region_cases.nonzero_dual_reference's duals, its one raised penalty per problem and
                     its steered guess, which puts every cone below, inside and outside at these duals.  The phases are judged there.
  S2 (update_state)  before a dual update: S1's duals and penalties, S1's u as the input guess, x its rollout from x0.  A FROZEN solve
                     (tol_meritfun_gradient huge: |phi'(0)| < tol takes alpha = 0; tol_stationarity = 4^200, whose square root is exact,
                     forces the outer update in every unit system; tol_primal_feasibility = 0 makes the penalty update fire, a huge
                     one leaves the penalty alone and ends with status 0) then updates z+ = Pi_K*(z - rho0 c(rollout)) and
                     rho+ = min(10 rho0, penalty_max).  rho0 is the solve's penalty_initial: like the reference, the oracle and the
                     device form a solve's first gradient with the penalty the handle holds and only then give EVERY problem
                     penalty_initial, so the update's penalty is one per batch (RHO0 = 3; PENALTY_MAX / 2 to take the clamp) and the
                     per-problem penalty of the state enters the first expansion only.  Where S1's duals do not put every region
                     into the update's ze, the last row of every cone's duals is steered (update_state says which).
"""
import copy
import os

import numpy as np

from tests import cone_region_cases as crc
from tests import hard_cases as hc
from tests.cone_region_cases import BATCH, RHOS

QUANTITIES = ("lx", "lu", "K", "d", "P", "p", "phi0", "dphi0", "phi", "dphi", "x", "u", "feas", "stat")
SCALARS = ("phi0", "dphi0", "phi", "dphi", "feas", "stat")
# what a fixture of the merit phase alone holds a reference for (a horizon at which every quantity would make the file larger than any
# other under tests/golden): phi(0), phi'(0), phi, phi' and the candidates at ALPHAS, feasibility
MERIT_QUANTITIES = ("phi0", "dphi0", "phi", "dphi", "x", "u", "feas")
MARGIN, FLOOR = 10.0, 1e-13
PENALTY_MAX = 1e8
TINY = np.finfo(np.float64).tiny


# ---- the transforms ------------------------------------------------------------------------------------------------------------------
def identity(cfg):
    return 0, np.ones(cfg.n), np.ones(cfg.m)


def transforms(name, fp32=False):
    """The changes of units configuration `name` is run under, as (k, D, E).  Dynamics as data: the whole cost times 4^+-20, and two
    mixed ones (k = +-5, D in 2^[-10, 10], E in 2^[-6, 6], fixed seed); a device model: k alone.  fp32: k = +-8, D in 2^[-4, 4],
    E in 2^[-3, 3]."""
    cfg = crc.config(name)
    one_n, one_m = np.ones(cfg.n), np.ones(cfg.m)
    kk, kmix, dx, du = (8, 3, 4, 3) if fp32 else (20, 5, 10, 6)
    out = [(kk, one_n, one_m), (-kk, one_n, one_m)]
    if cfg.dyn == "data":
        rng = np.random.default_rng(77 + sum(map(ord, cfg.base)))     # (a configuration at another horizon: its base's changes of units)
        for k in (kmix, -kmix):
            out.append((k, 2.0 ** rng.integers(-dx, dx + 1, size=cfg.n), 2.0 ** rng.integers(-du, du + 1, size=cfg.m)))
    return out


def subset(cfg, names):
    """`cfg` with only the blocks named (its guess, and so the classes of the blocks that stay, unchanged): for handles that take fewer
    constraint slots per knot point than the configuration fills (fp32 on the tile: two)."""
    out = copy.copy(cfg)
    out.blocks = [bl for bl in cfg.blocks if bl["name"] in names]
    assert len(out.blocks) == len(names)
    return out


def cost_only(T):
    return bool((T[1] == 1.0).all() and (T[2] == 1.0).all())


def _normal(a, what):
    a = np.asarray(a, dtype=np.float64)
    nz = a[a != 0.0]
    assert np.isfinite(a).all() and (np.abs(nz) >= TINY).all(), "a scaled input left the normal range: " + what
    return np.ascontiguousarray(a)


def _cm(a, rows, cols):
    """[.., rows * cols] column-major blocks as a view [.., cols, rows]."""
    return a.reshape(a.shape[:-1] + (cols, rows))


def transform(cfg, k, D, E, scale=None):
    """Configuration `cfg` (cone_region_cases.Config) in the units of T = (k, D, E): dynamics or model, both cost forms, x0, the steered
    guess, u_start and every block's G.  `scale` overrides 4^k (only to show that a scale which is no power of four is NOT exact).
    The result carries .scale: penalties are RHOS times it."""
    n, m = cfg.n, cfg.m
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    s = 4.0 ** k if scale is None else float(scale)
    for v in (D, E, np.array([s])):
        assert (np.log2(v) == np.round(np.log2(v))).all()
    out = copy.copy(cfg)
    out.scale, out.units = s, (k, D, E)
    if cfg.dyn == "di":
        assert (D == 1.0).all() and (E == 1.0).all(), "a device model's dynamics are not data: the cost scale alone"
        out.Qd, out.Rd, out.xref = _normal(cfg.Qd * s, "Qd"), _normal(cfg.Rd * s, "Rd"), cfg.xref
    else:
        p, q = cfg.p, {}
        q["A"] = _cm(p["A"], n, n) * D[None, None, None, :] / D[None, None, :, None]
        q["B"] = _cm(p["B"], n, m) * D[None, None, None, :] / E[None, None, :, None]
        q["f"] = p["f"] * D
        q["Qd"], q["Rd"] = p["Qd"] * s / D / D, p["Rd"] * s / E / E
        q["xref"], q["uref"] = p["xref"] * D, p["uref"] * E
        q["x0"], q["u0"] = p["x0"] * D, p["u0"] * E
        if cfg.dense:
            q["Q"] = _cm(p["Q"], n, n) * s / D[None, None, None, :] / D[None, None, :, None]
            q["R"] = _cm(p["R"], m, m) * s / E[None, None, None, :] / E[None, None, :, None]
            q["H"] = _cm(p["H"], m, n) * s / E[None, None, None, :] / D[None, None, :, None]
            q["q"], q["r"], q["c"] = p["q"] * s / D, p["r"] * s / E, p["c"] * s
        out.p = {key: _normal(v.reshape(p[key].shape), key) for key, v in q.items()}
    out.x, out.u = _normal(cfg.x * D, "x"), _normal(cfg.u * E, "u")
    out.x0 = _normal(cfg.x0 * D, "x0")
    out.u_start = _normal(cfg.u_start * E, "u_start")
    out.blocks = []
    DE = np.concatenate([D, E])
    for bl in cfg.blocks:
        bl = dict(bl)
        bl["G"] = _normal(bl["G"] / DE[None, :], "G of " + bl["name"])
        out.blocks.append(bl)
    # every (problem, knot point, block) stays in its class, the exact ties included
    for rho in RHOS:
        was, now = cfg.classes(rho), out.classes(rho * s)
        assert was.keys() == now.keys()
        for key, w in was.items():
            if out.blocks[key[0]]["kind"] == "soc":
                assert w[:2] == now[key][:2] and w[2] * s == now[key][2], (cfg.name, key, w, now[key])
            else:
                assert w == now[key], (cfg.name, key, w, now[key])
    return out


def back(res, k, D, E, scale=None):
    """A phases-shaped result ({name: array}; one problem's or the batch's) from the units of T = (k, D, E) to the old ones."""
    D, E = np.asarray(D, dtype=np.float64), np.asarray(E, dtype=np.float64)
    n, m = D.size, E.size
    s = 4.0 ** k if scale is None else float(scale)
    out = {}
    for key, v in res.items():
        if key == "z":                         # duals per block: z~ / s
            out[key] = {name: np.asarray(a, dtype=np.float64) / s for name, a in v.items()}
            continue
        v = np.asarray(v, dtype=np.float64)
        if key in ("lx", "p"):
            v = v * D / s
        elif key == "lu":
            v = v * E / s
        elif key == "K":                       # m x n column-major: E^-1 K~ D
            v = (_cm(v, m, n) * D[:, None] / E[None, :]).reshape(v.shape)
        elif key == "d" or key == "u":
            v = v / E
        elif key == "P":
            v = (_cm(v, n, n) * D[:, None] * D[None, :] / s).reshape(v.shape)
        elif key == "x":
            v = v / D
        elif key in ("phi0", "dphi0", "phi", "dphi", "stat", "rho"):
            v = v / s
        else:
            assert key in ("feas", "alpha", "status", "iterations"), key
        out[key] = v
    return out


def covariant_keys(T):
    """The quantities whose mapped-back value must be the unscaled one: all, but stationarity under D, E != 1."""
    return tuple(q for q in QUANTITIES if q != "stat" or cost_only(T))


# ---- the oracle's side ---------------------------------------------------------------------------------------------------------------
def expanded(cfg, b, rho):
    """The oracle's handle of problem b at the steered guess, zero duals, penalty rho times the configuration's scale (the cap scales
    with the units: oracle_ilqr_penalty_update clamps at penalty_max), expanded."""
    s = getattr(cfg, "scale", 1.0)
    h = crc.make_oracle(cfg, b)
    crc.set_guess(h, cfg, b)
    if rho * s != 1.0:
        h.set_penalty(1.0, rho * s, PENALTY_MAX * s)
        h.L.oracle_ilqr_penalty_update(h.h)
    crc.expand(h)
    return h


def oracle_phases(cfg, rho):
    """cone_region_cases.phases of every problem of `cfg` (a configuration or a transformed one), stacked over the batch."""
    per = [crc.phases(expanded(cfg, b, rho), crc.ALPHAS[b]) for b in range(BATCH)]
    return {q: np.stack([np.asarray(r[q], dtype=np.float64) for r in per]) for q in QUANTITIES}


_tables = {}


def class_tables(cfg, rho):
    """class_table at the three points the phases evaluate the AL terms at: the guess, the oracle's candidate of alpha = 0 and its
    candidate of alpha_b, as int8 [3, blocks, BATCH, N + 1, max rows]."""
    if (cfg.name, rho) not in _tables:
        N = cfg.N
        xs = np.zeros((2, BATCH, N + 1, cfg.n)); us = np.zeros((2, BATCH, N, cfg.m))
        for b in range(BATCH):
            h = expanded(cfg, b, rho)
            assert h.L.oracle_ilqr_backward_pass(h.h) == -1
            for i, alpha in enumerate((0.0, crc.ALPHAS[b])):
                h.merit(alpha)
                xs[i, b], us[i, b] = h.get("x_cand"), h.get("u_cand")
        _tables[(cfg.name, rho)] = np.stack([class_table(cfg, rho), class_table(cfg, rho, xs[0], us[0]), class_table(cfg, rho, xs[1], us[1])])
    return _tables[(cfg.name, rho)]


def differing(a, ref, keys=QUANTITIES):
    """The quantities of `keys` on which a and ref are not bit-identical, with the largest difference relative to the block."""
    return {q: errors({q: a[q]}, {q: ref[q]})[q] for q in keys if not np.array_equal(np.asarray(a[q]), np.asarray(ref[q]))}


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
def errors(res, ref):
    """hard_cases.blockerr per quantity both hold: blocks per (problem, knot point), scalars one block each."""
    out = {}
    for q in QUANTITIES:
        if q in res and q in ref:
            a, b = np.asarray(res[q], dtype=np.float64), np.asarray(ref[q], dtype=np.float64)
            if a.ndim == 1:
                a, b = a[:, None, None], b[:, None, None]
            out[q] = hc.blockerr(a, b)
    return out


def limits(e_cpu):
    """max(e_cpu, floor) per quantity, from the fixture's stored oracle error."""
    return {q: max(float(e), FLOOR) for q, e in zip(QUANTITIES, e_cpu)}


def criterion_b(res, fx, ri):
    """{quantity: e / max(e_cpu, floor)} of `res` (old units, the batch) against penalty RHOS[ri] of fixture fx."""
    e = errors(res, reference(fx, ri))
    lim = limits(fx["ecpu_%d" % ri])
    return {q: e[q] / lim[q] for q in e}


def rejected(ratios, margins=None):
    return {q: r for q, r in ratios.items() if not r <= (margins or {}).get(q, MARGIN)}


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def fixture_path(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_phases_%s.npz" % name)


def load(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def reference(fx, ri):
    """(a fixture of the merit phase alone -- MERIT_QUANTITIES -- holds no reference for the others)"""
    return {q: fx["ref_%d_%s" % (ri, q)] for q in QUANTITIES if "ref_%d_%s" % (ri, q) in fx}


def inputs(cfg):
    """Every array the phases of `cfg` are computed from, for the fixture's checksum."""
    d = dict(x=cfg.x, u=cfg.u, x0=cfg.x0, alphas=crc.ALPHAS, rhos=np.array(RHOS))
    if cfg.dyn == "di":
        d.update(Qd=cfg.Qd, Rd=cfg.Rd, xref=cfg.xref, h=np.array([crc.H_DI]))
    else:
        keys = ("A", "B", "f") + (("Q", "R", "H", "q", "r", "c") if cfg.dense else ("Qd", "Rd", "xref", "uref"))
        d.update({key: cfg.p[key] for key in keys})
    for j, bl in enumerate(cfg.blocks):
        d["G%02d" % j], d["g%02d" % j] = bl["G"], bl["g"]
        d["k%02d" % j] = np.array([bl["k0"], bl["k1"], bl["cone"]], dtype=np.int64)
    return d


def class_table(cfg, rho, x=None, u=None):
    """The branch of every (block, problem, knot point, row) at the trajectory x, u (None: the guess) as int8 [blocks, BATCH, N + 1,
    max rows], from the fp64 classification (cone_region_cases.classify_*): a cone's region in column 0 (0 below, 1 inside, 2 outside),
    an orthant row's activity per row (1: ze <= 0), -1 where there is nothing."""
    rows = max(bl["p"] for bl in cfg.blocks)
    t = np.full((len(cfg.blocks), BATCH, cfg.N + 1, rows), -1, dtype=np.int8)
    for (j, b, k), c in cfg.classes(rho, x, u).items():
        if cfg.blocks[j]["kind"] == "soc":
            t[j, b, k, 0] = ("below", "inside", "outside").index(c[0])
        else:
            t[j, b, k, :len(c)] = [0 if e == "neg" else 1 for e in c]
    return t


# ---- nonzero duals and the dual update -----------------------------------------------------------------------------------------------
RHO0 = 3.0                      # penalty_initial of the frozen solves: 10 RHO0 stays far below PENALTY_MAX
RHO_CLAMP = PENALTY_MAX / 2     # ... and the one at which rho+ = min(10 rho, PENALTY_MAX) takes the clamp
PENALTY_SCALING = 10.0
TOL_STAT = 4.0 ** 200           # sqrt is exact: the outer update fires in every unit system
HUGE = 1e100                    # tol_meritfun_gradient of a frozen sweep (times s: finite for every s here); also "feasible at any violation"
MARGIN_ZE = 1e-6                # every ze of S2 lies this far (of its own size) from its region's boundary
KINDS = ("soc", "orth", "eq")
SWEEP = ("K", "d", "P", "p")


def block_arrays(cfg, d):
    """{(block index, b, k): [p]} as {block name: [BATCH, knot points of the block, p]}."""
    return {bl["name"]: np.array([[d[(j, b, k)] for k in range(bl["k0"], bl["k1"] + 1)] for b in range(BATCH)]) for j, bl in enumerate(cfg.blocks)}


def block_dict(cfg, z):
    return {(j, b, k): z[bl["name"]][b, k - bl["k0"]] for j, bl in enumerate(cfg.blocks) for (b, k) in cfg.slots(j)}


def dual_state(name):
    """S1 of configuration `name`."""
    cfg, ref = crc.config(name), crc.nonzero_dual_reference(name)
    rho = np.zeros(BATCH)
    for b in range(BATCH):
        rhos = {ref["rhos"][(j, b, k)] for k in range(cfg.N + 1) for j in cfg.at(k)}
        assert len(rhos) == 1 and max(rhos) > 1.0, (name, b, rhos)       # one penalty per problem, raised by the oracle's penalty updates
        rho[b] = max(rhos)
    return dict(z=block_arrays(cfg, ref["duals"]), rho=rho, x=ref["x"], u=ref["u"])


def restrict(cfg, st):
    """State `st` with the duals of the blocks `cfg` (a subset of its configuration) keeps."""
    return dict(st, z={bl["name"]: st["z"][bl["name"]] for bl in cfg.blocks})


def state_classes(cfg, st, rho=None):
    """cfg.classes at the state's guess and duals; rho None: the state's penalty per problem, else one for all."""
    duals = block_dict(cfg, st["z"])
    rhos = {key: (st["rho"][key[1]] if rho is None else rho) for key in duals}
    return cfg.classes(x=st["x"], u=st["u"], duals=duals, rhos=rhos)


def same_classes(was, now, cfg, s):
    assert was.keys() == now.keys()
    for key, w in was.items():
        if cfg.blocks[key[0]]["kind"] == "soc":
            assert w[:2] == now[key][:2] and w[2] * s == now[key][2], (cfg.name, key, w, now[key])
        else:
            assert w == now[key], (cfg.name, key, w, now[key])


def transform_state(cfg, out, st, rho0=None):
    """State `st` of `cfg` in the units of `out` = transform(cfg, ...): duals and penalties times s, the guess times D and E.  Every
    (problem, knot point, block) keeps its class with ze = z - rho c formed from the mapped values (rho0: also at that one penalty)."""
    s, (_, D, E) = out.scale, out.units
    new = dict(z={name: _normal(a * s, "duals of " + name) for name, a in st["z"].items()}, rho=_normal(st["rho"] * s, "rho"),
               x=_normal(st["x"] * D, "x"), u=_normal(st["u"] * E, "u"))
    same_classes(state_classes(cfg, st), state_classes(out, new), cfg, s)
    if rho0 is not None:
        same_classes(state_classes(cfg, st, rho0), state_classes(out, new, rho0 * s), cfg, s)
    return new


def _handle(cfg, st, b):
    """The oracle's handle of problem b with the state's duals and penalty written by the setters."""
    h = crc.make_oracle(cfg, b)
    for k in range(cfg.N + 1):
        for slot, j in enumerate(cfg.at(k)):
            bl = cfg.blocks[j]
            h.set_duals(k, slot, st["z"][bl["name"]][b, k - bl["k0"]])
    h.set_block_penalty(st["rho"][b])
    return h


def rollout(cfg, u):
    """The oracle's open-loop rollout of the input guess u from x0, [BATCH, N + 1, n]."""
    N = cfg.N
    x = np.zeros((BATCH, N + 1, cfg.n))
    for b in range(BATCH):
        h = crc.make_oracle(cfg, b)
        for k in range(N):
            h.L.oracle_ilqr_set_input(h.h, k, crc._c(u[b, k]))
        h.L.oracle_ilqr_open_loop_rollout(h.h)
        x[b] = h.get("x_cand")
    return x


def oracle_dual_phases(cfg, st):
    """cone_region_cases.phases at state `st` (its duals and penalties kept), stacked over the batch."""
    per = []
    for b in range(BATCH):
        h = _handle(cfg, st, b)
        crc.set_guess(h, cfg, b, st["x"], st["u"])
        crc.expand(h)
        per.append(crc.phases(h, crc.ALPHAS[b]))
    return {q: np.stack([np.asarray(r[q], dtype=np.float64) for r in per]) for q in QUANTITIES}


def solve_options(cfg, feasible, rho0=RHO0, tolg=HUGE):
    """The options of the frozen solve (tolg = 1e-8: one with a real line search) in the units of `cfg`."""
    s = getattr(cfg, "scale", 1.0)
    return dict(tol_stationarity=TOL_STAT, tol_meritfun_gradient=tolg * s, tol_primal_feasibility=HUGE if feasible else 0.0,
                penalty_initial=rho0 * s, penalty_scaling=PENALTY_SCALING, penalty_max=PENALTY_MAX * s)


def oracle_update(cfg, st, feasible, sweeps, rho0=RHO0, tolg=HUGE, backtracking=False):
    """The oracle's solve of `sweeps` sweeps from state `st` (its u the input guess).  Returns, in the units of `cfg`, dict(z per block,
    rho [BATCH], alpha [BATCH, sweeps] (NaN for a sweep not taken), status, iterations, x, u the nominal trajectory, K, d, P, p of the
    last sweep)."""
    o = solve_options(cfg, feasible, rho0, tolg)
    N = cfg.N
    out = dict(rho=np.zeros(BATCH), alpha=np.full((BATCH, sweeps), np.nan), status=np.zeros(BATCH), iterations=np.zeros(BATCH))
    zs, per = {}, {q: [] for q in ("x", "u") + SWEEP}
    for b in range(BATCH):
        h = _handle(cfg, st, b)
        for k in range(N):
            h.L.oracle_ilqr_set_input(h.h, k, crc._c(st["u"][b, k]))
        h.set_penalty(o["penalty_initial"], o["penalty_scaling"], o["penalty_max"])
        h.L.oracle_ilqr_set_options(h.h, sweeps, o["tol_stationarity"], o["tol_primal_feasibility"], o["tol_meritfun_gradient"], int(backtracking))
        status, iters, log = h.solve()
        taken = min(iters, sweeps)
        out["status"][b], out["iterations"][b] = status, iters
        out["alpha"][b, :taken] = log[:taken, 0]
        rhos = set()
        for k in range(N + 1):
            for slot, j in enumerate(cfg.at(k)):
                zs[(j, b, k)] = h.duals(k, slot); rhos.add(h.penalty(k, slot))
        assert len(rhos) == 1
        out["rho"][b] = rhos.pop()
        for q in per:
            per[q].append(h.get(q))
    out["z"] = block_arrays(cfg, zs)
    out.update({q: np.stack(v) for q, v in per.items()})
    return out


UPDATE_KEYS = ("rho", "alpha", "status", "iterations", "x", "u")


def differing_update(a, ref, sweep=False, problems=None):
    """The entries of an oracle_update-shaped result on which a and ref are not bit-identical (NaNs of alpha equal), over `problems`
    (None: all), as {key: largest |a - ref|}."""
    idx = slice(None) if problems is None else np.asarray(problems)
    pairs = [(q, a[q], ref[q]) for q in UPDATE_KEYS + (SWEEP if sweep else ())] + [("z:" + nm, a["z"][nm], ref["z"][nm]) for nm in ref["z"]]
    out = {}
    for q, x, y in pairs:
        x, y = np.asarray(x, dtype=np.float64)[idx], np.asarray(y, dtype=np.float64)[idx]
        if not np.array_equal(x, y, equal_nan=True):
            out[q] = float(np.nanmax(np.abs(x - y)))
    return out


def dual_errors(cfg, z, ref):
    """hard_cases.blockerr of the duals per block KIND: one block per (problem, knot point, constraint block), no floor; a reference
    entry block that is exactly zero must be exactly zero.  {"z_soc": .., "z_orth": .., "z_eq": ..} for the kinds `cfg` has."""
    out = {}
    for bl in cfg.blocks:
        e = hc.blockerr(np.asarray(z[bl["name"]], dtype=np.float64), ref[bl["name"]])
        out["z_" + bl["kind"]] = max(out.get("z_" + bl["kind"], 0.0), e)
    return out


def ratios(e, e_cpu):
    """e / max(e_cpu, floor) per key of e."""
    return {q: e[q] / max(float(e_cpu[q]), FLOOR) for q in e}


# ---- S2 -------------------------------------------------------------------------------------------------------------------------------
def ze_margin(cfg, st, rho):
    """The smallest distance of a ze = z - rho c of state `st` from its region's boundary, relative to its own size: a cone's
    |a - |s|| / max(a, |s|), an orthant row's |ze| / max(|z|, |rho c|)."""
    worst = np.inf
    for j, bl in enumerate(cfg.blocks):
        if bl["kind"] == "eq":
            continue
        for (b, k) in cfg.slots(j):
            zd = st["z"][bl["name"]][b, k - bl["k0"]]
            rc = rho * crc.values(bl["G"], bl["g"], cfg.z(b, k, st["x"], st["u"]))
            ze = zd - rc
            if bl["kind"] == "soc":
                a, s = float(np.sqrt(crc.seq_sum(ze[:-1] * ze[:-1]))), float(ze[-1])
                worst = min(worst, abs(a - abs(s)) / max(a, abs(s)))
            else:
                size = np.maximum(np.abs(zd), np.abs(rc))
                worst = min(worst, float((np.abs(ze) / size).min()))
    return worst


def coverage(cfg, st, rho):
    """{block name: the set of regions (cones) / of row activities "active", "inactive" (orthant blocks) ze takes over batch and horizon}."""
    out = {}
    for (j, b, k), c in state_classes(cfg, st, rho).items():
        got = out.setdefault(cfg.blocks[j]["name"], set())
        if cfg.blocks[j]["kind"] == "soc":
            got.add(c[0])
        else:
            got.update("inactive" if e == "neg" else "active" for e in c)
    return out


def covered(cfg, cov):
    want = {"soc": {"below", "inside", "outside"}, "orth": {"active", "inactive"}}
    return all(cov[bl["name"]] == want[bl["kind"]] for bl in cfg.blocks if bl["kind"] != "eq")


_states = {}


def update_state(name):
    """S2 of configuration `name`, and whether the cones' duals had to be steered for it."""
    if name not in _states:
        cfg, s1 = crc.config(name), dual_state(name)
        st = dict(z={nm: a.copy() for nm, a in s1["z"].items()}, rho=s1["rho"], u=s1["u"], x=rollout(cfg, s1["u"]))
        steered = not (covered(cfg, coverage(cfg, st, RHO0)) and ze_margin(cfg, st, RHO0) >= MARGIN_ZE)
        if steered:     # z_s of every cone block from a scheduled region, the way cone_region_cases.steer_from_duals chooses x[svar]
            for j, bl in enumerate(cfg.blocks):
                if bl["kind"] != "soc":
                    continue
                for i, (b, k) in enumerate(cfg.slots(j)):
                    zd = st["z"][bl["name"]][b, k - bl["k0"]]
                    c = crc.values(bl["G"], bl["g"], cfg.z(b, k, st["x"], st["u"]))
                    zev = zd[:-1] - RHO0 * c[:-1]
                    a = float(np.sqrt(crc.seq_sum(zev * zev)))
                    f = crc.REGION_FACTOR[("below", "inside", "outside")[(i + j) % 3]]
                    f = f[(i // 3) % 2] if isinstance(f, tuple) else f
                    zd[-1] = f * a + RHO0 * c[-1]
        _states[name] = (st, steered)
    return _states[name]


RHO_LS = 1.0


def search_state(name):
    """The state of the sweep with a REAL line search: S1's duals and input guess, with the penalty the handle holds EQUAL to the
    solve's penalty_initial = RHO_LS.  (From S1's own penalties, 10 .. 1000 against penalty_initial = 3, the first gradient -- formed with
    the held penalty -- and the Hessian -- formed with penalty_initial -- disagree by that factor and the oracle accepts alpha = 1 on no
    problem of any configuration; with both at 3 it rejects 3 of 7 on lane_6_3; with both at 1 at most 1 of 7 anywhere.)"""
    cfg, s1 = crc.config(name), dual_state(name)
    return dict(s1, rho=np.full(BATCH, RHO_LS), x=rollout(cfg, s1["u"]))


def search_mask(name, backtracking):
    """[BATCH] bool: the problems on which the oracle's one sweep from search_state accepts alpha = 1 in the old units and under
    every transform of transforms(name)."""
    cfg, st = crc.config(name), search_state(name)
    kw = dict(feasible=False, sweeps=1, rho0=RHO_LS, tolg=1e-8, backtracking=backtracking)
    ok = oracle_update(cfg, st, **kw)["alpha"][:, 0] == 1.0
    for T in transforms(name):
        out = transform(cfg, *T)
        ok &= oracle_update(out, transform_state(cfg, out, st), **kw)["alpha"][:, 0] == 1.0
    return ok


def state_class_tables(cfg, st):
    """class_tables for a state: the branches at its guess, at the oracle's candidate of alpha = 0 and at that of alpha_b, with the
    state's duals and penalties, int8 [3, blocks, BATCH, N + 1, max rows]."""
    N = cfg.N
    xs = np.zeros((2, BATCH, N + 1, cfg.n)); us = np.zeros((2, BATCH, N, cfg.m))
    for b in range(BATCH):
        h = _handle(cfg, st, b)
        crc.set_guess(h, cfg, b, st["x"], st["u"])
        crc.expand(h)
        assert h.L.oracle_ilqr_backward_pass(h.h) == -1
        for i, alpha in enumerate((0.0, crc.ALPHAS[b])):
            h.merit(alpha)
            xs[i, b], us[i, b] = h.get("x_cand"), h.get("u_cand")
    return np.stack([state_class_table(cfg, st)] + [state_class_table(cfg, dict(st, x=xs[i], u=us[i])) for i in range(2)])


# ---- the fixtures of the second half -----------------------------------------------------------------------------------------------
def dual_fixture_path(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_phases_duals_%s.npz" % name)


def load_duals(name):
    with np.load(dual_fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def state_arrays(cfg, st, prefix):
    """A state as flat fixture entries."""
    d = {prefix + "_rho": st["rho"], prefix + "_x": st["x"], prefix + "_u": st["u"]}
    d.update({"%s_z_%s" % (prefix, nm): a for nm, a in st["z"].items()})
    return d


def state_of(fx, cfg, prefix):
    return dict(z={bl["name"]: fx["%s_z_%s" % (prefix, bl["name"])] for bl in cfg.blocks}, rho=fx[prefix + "_rho"], x=fx[prefix + "_x"],
                u=fx[prefix + "_u"])


def blocks_of(fx, cfg, prefix):
    return {bl["name"]: fx["%s_%s" % (prefix, bl["name"])] for bl in cfg.blocks}


_dual_inputs = {}


def dual_inputs(name):
    """What the fixture of the second half is computed from: S1, S2, their class tables (tab_s1 [3, ..] of the phases at S1; tab_u1 of the
    first update, at S2 with RHO0; tab_u2 of the second sweep and update, at the oracle's z+ with 10 RHO0) and the line-search masks."""
    if name not in _dual_inputs:
        cfg = crc.config(name)
        s1, (s2, steered) = dual_state(name), update_state(name)
        z1 = oracle_update(cfg, s2, False, 1)["z"]
        _dual_inputs[name] = dict(s1=s1, s2=s2, steered=steered, tab_s1=state_class_tables(cfg, s1), tab_u1=state_class_table(cfg, s2, RHO0),
                                  tab_u2=state_class_table(cfg, dict(s2, z=z1), PENALTY_SCALING * RHO0),
                                  ls_mask=np.stack([search_mask(name, False), search_mask(name, True)]))
    return _dual_inputs[name]


def dual_input_arrays(cfg, d):
    out = dict(state_arrays(cfg, d["s1"], "s1"), **state_arrays(cfg, d["s2"], "s2"))
    out.update(s2_steered=np.array(int(d["steered"])), tab_s1=d["tab_s1"], tab_u1=d["tab_u1"], tab_u2=d["tab_u2"], ls_mask=d["ls_mask"])
    return out


def dual_reference_arrays(cfg, ref):
    """The maker's {(what, key): batch array} under the fixture's names."""
    out = {"ref_s1_" + q: ref[("s1", q)] for q in QUANTITIES}
    for bl in cfg.blocks:
        for i in (1, 2):
            out["ref_z%d_%s" % (i, bl["name"])] = ref[("up", "z%d:%s" % (i, bl["name"]))]
    out.update({"ref_rho%d" % i: ref[("up", "rho%d" % i)] for i in (1, 2)})
    out.update({"ref_sw2_" + q: ref[("up", q)] for q in SWEEP})
    return out


def oracle_of_fixture(cfg, s1, s2):
    """The oracle's side of everything the fixture holds a reference for."""
    up1, up2 = oracle_update(cfg, s2, False, 1), oracle_update(cfg, s2, False, 2)
    return dict(s1=oracle_dual_phases(cfg, s1), z1=up1["z"], rho1=up1["rho"], z2=up2["z"], rho2=up2["rho"], sw2={q: up2[q] for q in SWEEP})


def sweep_errors(res, ref):
    return {q: hc.blockerr(np.asarray(res[q], dtype=np.float64), ref[q]) for q in SWEEP}


def dual_ecpu(cfg, d, fx):
    """The oracle's blockerr against the references of `fx`: ecpu_s1 [QUANTITIES], ecpu_z1 / ecpu_z2 [KINDS] (0 for a kind the
    configuration has not), ecpu_sw2 [SWEEP]."""
    o = oracle_of_fixture(cfg, d["s1"], d["s2"])
    e = errors(o["s1"], {q: fx["ref_s1_" + q] for q in QUANTITIES})
    out = dict(ecpu_s1=np.array([e[q] for q in QUANTITIES]))
    for i in (1, 2):
        ez = dual_errors(cfg, o["z%d" % i], blocks_of(fx, cfg, "ref_z%d" % i))
        out["ecpu_z%d" % i] = np.array([ez.get("z_" + kind, 0.0) for kind in KINDS])
    es = sweep_errors(o["sw2"], {q: fx["ref_sw2_" + q] for q in SWEEP})
    out["ecpu_sw2"] = np.array([es[q] for q in SWEEP])
    return out


def dual_limits(fx, which):
    """{key: e_cpu} of fixture entry ecpu_<which>."""
    keys = {"s1": QUANTITIES, "sw2": SWEEP}.get(which, tuple("z_" + kind for kind in KINDS))
    return dict(zip(keys, fx["ecpu_" + which]))


def state_class_table(cfg, st, rho=None):
    """class_table's int8 layout for a state (rho None: its penalty per problem)."""
    rows = max(bl["p"] for bl in cfg.blocks)
    t = np.full((len(cfg.blocks), BATCH, cfg.N + 1, rows), -1, dtype=np.int8)
    for (j, b, k), c in state_classes(cfg, st, rho).items():
        if cfg.blocks[j]["kind"] == "soc":
            t[j, b, k, 0] = ("below", "inside", "outside").index(c[0])
        else:
            t[j, b, k, :len(c)] = [0 if e == "neg" else 1 for e in c]
    return t
