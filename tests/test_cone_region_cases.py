"""The cases of tests/cone_region_cases.py do what they were chosen for -- checked from the oracle alone, no GPU:
  * coverage: every class of every cone block (orthant block) occurs at a running knot point, every class of a second-order cone occurs
    at the terminal knot point of every configuration that has cones (seven problems: over the configuration's terminal cones together);
  * the ties are ties in floating point, and a comparison flipped there cannot hide under a tolerance: the Hessian block and the gains K
    of the horizon move by more than 1e-3 relative when the point is nudged across (s (1 - 1e-9) for a cone, val = -1e-9 for a row);
  * the curvature term of the cones matters: without it K moves by more than 1e-3.
"""
import numpy as np
import pytest

from oracle import oracle
from tests import cone_region_cases as crc
from tests.cone_region_cases import BATCH, N

CONE_CONFIGS = [c for c in crc.CONFIGS if c != "auto32_rows"]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(a).max(), np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_every_class_is_reached(name):
    cfg = crc.config(name)
    cls = cfg.classes(1.0)
    terminal = set()
    for j, bl in enumerate(cfg.blocks):
        if bl["kind"] == "soc":
            seen = {cls[(j, b, k)][1] for (b, k) in cfg.slots(j)}
            for (b, k) in cfg.slots(j):
                region, c, a = cls[(j, b, k)]
                assert c == cfg.schedule[(j, b, k)], (bl["name"], b, k, c, cfg.schedule[(j, b, k)])
                assert not c.startswith("out") or a >= 0.1
                # the region each class lies in, by the oracle's order of comparisons
                assert region == {"below": "below", "inside": "inside", "apex": "below", "v0_pos": "inside", "v0_neg": "below", "tie_in": "inside",
                                  "tie_below": "below"}.get(c, "outside")
            if bl["k0"] == N:
                terminal |= seen
            else:
                assert seen == set(crc.SOC_CLASSES), (bl["name"], sorted(set(crc.SOC_CLASSES) - seen))
        elif bl["kind"] == "orth":
            seen = {c for (b, k) in cfg.slots(j) for c in cls[(j, b, k)]}
            assert seen == set(crc.ORTH_CLASSES), (bl["name"], seen)
            (tie,) = [(b, k) for (jj, b, k) in cfg.schedule if jj == j]
            assert cls[(j,) + tie][0] == "zero"
    if name in CONE_CONFIGS:
        assert terminal == set(crc.SOC_CLASSES), sorted(set(crc.SOC_CLASSES) - terminal)
    # penalty 50: the same classes, ties included
    cls50 = cfg.classes(50.0)
    for key, v in cls.items():
        assert (v[1] == cls50[key][1]) if isinstance(v, tuple) else (v == cls50[key]), key
    # what the plans take
    per_knot = max(len(cfg.at(k)) for k in range(N + 1))
    if cfg.plan == "LANE":
        assert per_knot <= 2 and len(cfg.blocks) <= 16 and all(bl["p"] <= (4 if bl["kind"] == "soc" else 8) for bl in cfg.blocks)
    if cfg.plan == "MFMA16":
        slots = lambda bl: 1 if bl["kind"] == "soc" else -(-bl["p"] // 8)
        assert max(sum(slots(cfg.blocks[j]) for j in cfg.at(k)) for k in range(N + 1)) <= 6 and sum(slots(bl) for bl in cfg.blocks) <= 32
        assert all(bl["p"] <= 4 for bl in cfg.blocks if bl["kind"] == "soc")
    if cfg.plan in ("GENERIC", "MFMA32"):
        assert per_knot <= 8 and all(bl["p"] <= 32 for bl in cfg.blocks)


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_a_flipped_comparison_at_a_tie_moves_hessian_and_gains(name):
    cfg = crc.config(name)
    n, m = cfg.n, cfg.m
    ties = [(j, b, k, c) for (j, b, k), c in cfg.schedule.items() if c in ("tie_in", "tie_below", "zero")]
    assert ties
    for (j, b, k, c) in ties:
        bl = cfg.blocks[j]
        zvec = cfg.z(b, k)
        x, g_of = cfg.x.copy(), None
        if bl["kind"] == "soc":
            cs = zvec[bl["svar"]] - crc.G_S
            assert abs(cs) == bl["norm"]
            x[b, k, bl["svar"]] = crc.G_S + cs * (1.0 - 1e-9)              # |s| below a: outside the cone and its polar
            z2 = cfg.z(b, k, x=x)
            h1, h2 = crc.knot_hessian(bl, n, m, zvec, np.zeros(bl["p"]), 1.0), crc.knot_hessian(bl, n, m, z2, np.zeros(bl["p"]), 1.0)
            assert crc.classify_soc(-crc.values(bl["G"], bl["g"], z2))[0] == "outside"
        else:
            g2 = bl["g"].copy(); g2[0] += 1e-9                             # val[0] = -1e-9: the row is inactive
            g_of = {j: g2}
            h1, h2 = crc.knot_hessian(bl, n, m, zvec, np.zeros(bl["p"]), 1.0), crc.knot_hessian(bl, n, m, zvec, np.zeros(bl["p"]), 1.0, g=g2)
        assert rel(h1, h2) > 1e-3, (bl["name"], b, k, c, rel(h1, h2))
        K1, K2 = crc.gains(cfg, b, 1.0), crc.gains(cfg, b, 1.0, x=x, g_of=g_of)
        assert rel(K1, K2) > 1e-3, (bl["name"], b, k, c, rel(K1, K2))


@pytest.mark.parametrize("name", CONE_CONFIGS)
def test_the_curvature_term_moves_the_gains(name):
    """Per cone block: K of a problem from the oracle's Hessians, and from those without the block's rho G^T (d/dz J^T z_proj) G at the
    knot points where the problem is outside the cone."""
    cfg = crc.config(name)
    n, m = cfg.n, cfg.m
    cls = cfg.classes(1.0)
    for j, bl in enumerate(cfg.blocks):
        if bl["kind"] != "soc":
            continue
        moved = 0.0
        for b in range(BATCH):
            s = crc.oracle_sweep(cfg, b, 1.0)
            H = {key: s.get(key)[None].copy() for key in ("A", "B", "lxx", "luu", "lux", "lx", "lu")}
            f = np.zeros((1, N, n))
            base = oracle.backward_batch(H["A"], H["B"], f, H["lxx"], H["luu"], H["lux"], H["lx"], H["lu"])
            assert s.L.oracle_ilqr_backward_pass(s.h) == -1 and np.array_equal(base["K"][0], s.get("K"))
            hit = False
            for (bb, k) in cfg.slots(j):
                if bb != b or cls[(j, b, k)][0] != "outside":
                    continue
                hit = True
                Hc = crc.curvature_term(bl, cfg.z(b, k), np.zeros(bl["p"]), 1.0)
                H["lxx"][0, k] -= Hc[:n, :n].reshape(-1)
                if k < N:
                    H["luu"][0, k] -= Hc[n:, n:].reshape(-1)
                    H["lux"][0, k] -= Hc[n:, :n].flatten(order="F")
            if hit:
                cut = oracle.backward_batch(H["A"], H["B"], f, H["lxx"], H["luu"], H["lux"], H["lx"], H["lu"])
                moved = max(moved, rel(base["K"][0], cut["K"][0]))
        if bl["p"] == 2:                       # (v is a scalar: the cone is a wedge, its projection piecewise linear)
            assert moved < 1e-12, (bl["name"], moved)
            continue
        assert moved > 1e-3, (bl["name"], moved)


@pytest.mark.parametrize("name", crc.CONFIGS)
def test_truncated_solves_update_duals_without_rounding_limited_searches(name):
    """What tests/test_gpu_cone_regions.py's second part relies on, from the oracle's log: after SOLVE_SWEEPS sweeps every problem has
    taken a dual update, no line search took >= 8 evaluations or a step below 1e-2; the guess steered from the duals reaches the three
    regions of every cone block and both sides of every orthant block, with nonzero duals in play."""
    cfg = crc.config(name)
    ref = crc.nonzero_dual_reference(name)
    for b in range(BATCH):
        log = ref["log"][b]
        assert ref["dual_updates"][b] >= 1, (b, log[:, 4])
        assert (log[:, 5] < 8).all() and (log[:, 0] >= 1e-2).all(), (b, log[:, 5], log[:, 0])
    cls = cfg.classes(x=ref["x"], u=ref["u"], duals=ref["duals"], rhos=ref["rhos"])
    for j, bl in enumerate(cfg.blocks):
        if bl["kind"] == "eq":
            continue
        assert max(np.abs(ref["duals"][(j, b, k)]).max() for (b, k) in cfg.slots(j)) > 0.0, bl["name"]
        if bl["kind"] == "soc":
            for (b, k) in cfg.slots(j):
                assert cls[(j, b, k)][0] == ref["want"][(j, b, k)] and cls[(j, b, k)][1] in ("below", "inside", "out_pos", "out_neg")
            assert {cls[(j, b, k)][0] for (b, k) in cfg.slots(j)} == {"below", "inside", "outside"}
        else:
            sides = {c for (b, k) in cfg.slots(j) for c in cls[(j, b, k)]}
            assert sides == {"neg", "pos"}, (bl["name"], sides)
    assert max(ref["rhos"].values()) > 1.0
