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
"""
import copy
import os

import numpy as np

from tests import cone_region_cases as crc
from tests import hard_cases as hc
from tests.cone_region_cases import BATCH, N, RHOS

QUANTITIES = ("lx", "lu", "K", "d", "P", "p", "phi0", "dphi0", "phi", "dphi", "x", "u", "feas", "stat")
SCALARS = ("phi0", "dphi0", "phi", "dphi", "feas", "stat")
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
        rng = np.random.default_rng(77 + sum(map(ord, name)))
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
        elif key in ("phi0", "dphi0", "phi", "dphi", "stat"):
            v = v / s
        else:
            assert key == "feas", key
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
    return {q: fx["ref_%d_%s" % (ri, q)] for q in QUANTITIES}


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
    t = np.full((len(cfg.blocks), BATCH, N + 1, rows), -1, dtype=np.int8)
    for (j, b, k), c in cfg.classes(rho, x, u).items():
        if cfg.blocks[j]["kind"] == "soc":
            t[j, b, k, 0] = ("below", "inside", "outside").index(c[0])
        else:
            t[j, b, k, :len(c)] = [0 if e == "neg" else 1 for e in c]
    return t
