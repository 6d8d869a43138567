"""The TVLQR sweeps of every plan on the hard problem families (tests/hard_cases.py), judged against the extended-precision fixtures
(tests/golden/hard_tvlqr_<n>x<m>.npz) in a metric that respects each block's own scale (hard_cases.blockerr).  Needs an MI355X.

Plans that follow the oracle's operation order (GENERIC, LANE) must equal the oracle bit for bit here too.  Plans that reassociate
(MFMA16 fp64 / fp32 storage / pure fp32, MFMA32, GENERIC's matrix-core products) must stay within

    blockerr(kernel, fixture) <= margin * max(e_cpu, floor)

per quantity, where e_cpu is the STORED error of the straight CPU computation in the same working precision against the same
fixture (the oracle for fp64 arithmetic, a numpy float32 recursion for pure fp32) -- never anything computed from the kernel; floor is
1e-13 for fp64 (ten times what DESIGN section 2 records on benign data), 2^-23 for fp32 storage, the benign family's stored e_cpu32 for
pure fp32; margin is 10 (two sound evaluation orders of one recursion differ by a small factor; the bug this is for, DESIGN 4.16, was a
factor of 1e9).  The measured ratios e_gpu / max(e_cpu, floor) are printed, and recorded in DESIGN section 2."""
import collections

import numpy as np
import pytest

import altro_amd
from oracle import oracle
from tests import hard_cases as hc

pytestmark = pytest.mark.gpu

MARGIN = 10.0
# (configuration, family, quantity) -> a margin of up to 100, explained in DESIGN section 2.  The only ones: the trajectory of the fp32
# STORAGE variant where the closed loop is sensitive to its gains.  The forward sweep reads the gains the backward sweep stored, rounded
# to fp32 (2^-24 of the block's scale, which is what the measured 0.4 .. 0.5 on K, d, P, p is); e_cpu, fp64 arithmetic that keeps its
# gains in fp64, has no such term, and the floor 2^-23 covers the rounding of x, u, y themselves but not what A - B K makes of a K that
# is 2^-24 off.  The oracle's forward pass fed with its own gains rounded to fp32 reproduces every measured ratio to two digits (19 /
# 13 / 30 on (12, 4) collinear, 14 / 80 / 25 on (12, 2)), so the kernel's arithmetic adds nothing to it.
MARGINS = {("mfma16_f32", fam, q): 100.0 for fam, qs in (("collinear", "xuy"), ("unstable", "uy"), ("cheap", "u")) for q in qs}
Cfg = collections.namedtuple("Cfg", "name shape plan dtype flags kind")
G, T16, LN, T32 = altro_amd.PLAN_GENERIC, altro_amd.PLAN_MFMA16, altro_amd.PLAN_LANE, altro_amd.PLAN_MFMA32
F64, F32 = altro_amd.F64, altro_amd.F32
_id = lambda c: "%s-%dx%d" % ((c.name,) + c.shape)

EXACT = [Cfg("generic", s, G, F64, 0, "exact") for s in hc.SHAPES] + [Cfg("lane", s, LN, F64, 0, "exact") for s in hc.LANE_SHAPES]
REASSOC = ([Cfg("mfma16", s, T16, F64, 0, "f64") for s in hc.TILE_SHAPES] + [Cfg("mfma32", s, T32, F64, 0, "f64") for s in hc.TILE32_SHAPES]
           + [Cfg("generic_mc", s, G, F64, altro_amd.GENERIC_MATRIX_CORES, "f64") for s in hc.MC_SHAPES]
           + [Cfg("mfma16_f32", s, T16, F32, 0, "mixed") for s in hc.TILE_SHAPES]
           # the two pure-fp32 kernel pairs: one problem per wave (a batch that is no multiple of four) and four problems per wave
           + [Cfg("mfma16_pure", s, T16, F32, altro_amd.F32_PURE, "pure") for s in hc.TILE_SHAPES]
           + [Cfg("mfma16_pure_x4", s, T16, F32, altro_amd.F32_PURE, "pure") for s in hc.TILE_SHAPES])
OTHER_F32 = [Cfg("lane_f32", s, LN, F32, 0, "f32") for s in hc.LANE_SHAPES] + [Cfg("generic_f32", s, G, F32, 0, "f32") for s in ((13, 4), (20, 8))]
OUT = ("K", "d", "P", "p", "dV")
_fx = {}


def fixture(shape):
    if shape not in _fx:
        _fx[shape] = hc.load(*shape)
    return _fx[shape]


def x4(cfg):
    return cfg.name.endswith("_x4")


def open_batch(cfg, pr):
    batch = pr["A"].shape[0]
    bt = altro_amd.Batch(hc.N, pr["n"], pr["m"], batch, dtype=cfg.dtype, plan=cfg.plan, flags=cfg.flags)
    assert bt.plan == cfg.plan
    bt.set_dynamics(pr["A"], pr["B"], pr["f"]); bt.set_cost(pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    bt.set_initial_state(pr["x0"])
    return bt


def fetch(bt, forward):
    out = {k: bt.get("delta_V" if k == "dV" else k) for k in OUT}
    out["status"] = bt.get("status")
    if forward:
        for k in ("x", "u", "y"):
            out[k] = bt.get(k)
    return out


def run(cfg, pr, forward=True):
    """Backward (and forward) sweep of `pr` on `cfg`; the four-problems-per-wave kernels get a batch of whole quads (the first
    problems again), of which the caller sees the problems it gave."""
    batch = pr["A"].shape[0]
    if x4(cfg) and batch % 4:
        pr = hc.stack([pr, hc.take(pr, list(range(4 - batch % 4)))])
    bt = open_batch(cfg, pr)
    bt.backward()
    if forward:
        bt.forward_ltv()
    out = {k: v[:batch] for k, v in fetch(bt, forward).items()}
    bt.close()
    return out


def which_of(cfg):
    return "d" if cfg.dtype == F64 else "s"


def limits(cfg, fx, fam):
    """max(e_cpu, floor) per quantity for `cfg` on `fam`, from the fixture alone."""
    if cfg.kind == "f64":
        e, floor = fx["e64_%s_d" % fam], np.full(len(hc.QUANTITIES), 1e-13)
    elif cfg.kind == "mixed":
        e, floor = fx["e64_%s_s" % fam], np.full(len(hc.QUANTITIES), 2.0 ** -23)
    else:
        e, floor = fx["e32_%s_s" % fam], fx["e32_benign_s"]
    return dict(zip(hc.QUANTITIES, np.maximum(e, floor)))


def judge(cfg, fam, errs, lim, what, bad):
    ratios = {q: errs[q] / lim[q] for q in errs}
    print("%-16s %-9s %-10s " % (_id(cfg), fam, what) + " ".join("%s %.2g" % (q, r) for q, r in ratios.items()))
    for q, r in ratios.items():
        if not r <= MARGINS.get((cfg.name, fam, q), MARGIN):
            bad.append((_id(cfg), fam, what, q, "e_gpu %.3g" % errs[q], "max(e_cpu, floor) %.3g" % lim[q], "ratio %.3g" % r))


@pytest.mark.parametrize("cfg", EXACT, ids=_id)
def test_order_following_plans_equal_the_oracle(cfg):
    """GENERIC and LANE (quad, quad2 and lane kernels) claim the oracle's bits: on every family, status included."""
    n, m = cfg.shape
    for fam in hc.FAMILIES:
        pr = hc.problem(fam, n, m, "d")
        out, ref = run(cfg, pr), hc.run_oracle(pr)
        assert np.array_equal(out["status"], ref["status"]) and (out["status"] == -1).all(), fam
        for k in hc.QUANTITIES:
            assert np.array_equal(out[k], ref[k]), (fam, k)


@pytest.mark.parametrize("cfg", REASSOC, ids=_id)
def test_reassociating_plans_against_extended_precision(cfg):
    n, m = cfg.shape
    fx, w, bad = fixture(cfg.shape), which_of(cfg), []
    for fam in hc.FAMILIES:
        pr = hc.problem(fam, n, m, w)
        out = run(cfg, pr)
        assert (out["status"] == -1).all(), (fam, out["status"])
        D = hc.scale_vector(fam, n, hc.level(fam, w, n, m))
        errs = hc.errors(hc.at_knots(out, n), hc.unpack(fx["ref_%s_%s" % (fam, w)], n, m), n, m, D)
        judge(cfg, fam, errs, limits(cfg, fx, fam), "", bad)
    assert not bad, bad


def unscaled(out, k):
    s = 4.0 ** k
    return dict(out, P=out["P"] / s, p=out["p"] / s, dV=out["dV"] / s, y=out["y"] / s)


@pytest.mark.parametrize("cfg", EXACT + REASSOC, ids=_id)
def test_cost_scale_invariance(cfg):
    """The whole cost (Q, R, H, q, r) times 4^k: K, d, x, u stay, P, p, ΔV (and y = P x + p) take the factor.  Powers of four pass through
    IEEE sqrt and division exactly and nothing under- or overflows, so the order-following plans must give the same bits; the
    reassociating plans must meet the criterion of this file at both scales (whether they, too, are bit-identical is printed: it says
    whether the reciprocal-square-root seed is scale-exact)."""
    n, m = cfg.shape
    fx, w, bad = fixture(cfg.shape), which_of(cfg), []
    kk = 30 if cfg.dtype == F64 else 8
    same = True
    for fam in hc.FAMILIES:
        pr = hc.problem(fam, n, m, w)
        base = run(cfg, pr)
        for k in (kk, -kk):
            out = unscaled(run(cfg, hc.scaled_cost(pr, k)), k)
            assert np.array_equal(out["status"], base["status"]) and (out["status"] == -1).all(), (fam, k)
            bits = all(np.array_equal(out[q], base[q]) for q in hc.QUANTITIES)
            same &= bits
            if cfg.kind == "exact":
                for q in hc.QUANTITIES:
                    assert np.array_equal(out[q], base[q]), (fam, k, q)
            else:
                D = hc.scale_vector(fam, n, hc.level(fam, w, n, m))
                errs = hc.errors(hc.at_knots(out, n), hc.unpack(fx["ref_%s_%s" % (fam, w)], n, m), n, m, D)
                judge(cfg, fam, errs, limits(cfg, fx, fam), "x 4^%d" % k, bad)
    print("%-16s cost x 4^+-%d bit-identical to the unscaled run: %s" % (_id(cfg), kk, same))
    assert not bad, bad


@pytest.mark.parametrize("cfg", EXACT + REASSOC, ids=_id)
def test_failure_index_away_from_the_boundary(cfg):
    """One problem of three made to fail at a chosen knot point, its last pivot far below zero (the fixture holds the margins: below
    -1e-3 |Quu| there, above +1e-6 |Quu| everywhere else; nearer the boundary two sound kernels may disagree).  The status is the
    fixture's; K_k = Qux and d_k = -Qu are left at the failing knot point; nothing is written below it (the results of an earlier,
    successful sweep on the same handle are still there); everything above it, and the two neighbours, are what they were."""
    n, m = cfg.shape
    fx, bad = fixture(cfg.shape), []
    b, kf = hc.FAIL_PROBLEM, hc.FAIL_KNOT
    for fam in hc.FAMILIES:
        rec = fx["fail_%s" % fam]
        pr = hc.problem(fam, n, m, "s")
        prf = hc.with_failure(pr, rec[0])
        batch = hc.BATCH
        if x4(cfg):
            pr, prf = (hc.stack([p, hc.take(p, [0])]) for p in (pr, prf))
        bt = open_batch(cfg, pr)
        bt.backward()
        first = fetch(bt, False)
        assert (first["status"] == -1).all(), fam
        bt.set_cost(prf["Q"], prf["R"], prf["H"], prf["q"], prf["r"])
        bt.backward()
        out = fetch(bt, False)
        bt.close()
        assert out["status"][:batch].tolist() == [kf if i == b else -1 for i in range(batch)], (fam, out["status"])
        for q in ("K", "d", "P", "p"):
            assert np.array_equal(out[q][b, :kf], first[q][b, :kf]), (fam, q, "written below the failing knot point")
            assert np.array_equal(out[q][b, kf + 1:], first[q][b, kf + 1:]), (fam, q, "changed above the failing knot point")
            keep = [i for i in range(out[q].shape[0]) if i != b]
            assert np.array_equal(out[q][keep], first[q][keep]), (fam, q, "a neighbour of the failing problem changed")
        Kk, dk = out["K"][b:b + 1, kf:kf + 1], out["d"][b:b + 1, kf:kf + 1]
        if cfg.kind == "exact":
            ref = oracle.backward_batch(prf["A"], prf["B"], prf["f"], prf["Q"], prf["R"], prf["H"], prf["q"], prf["r"])
            assert np.array_equal(Kk[0, 0], ref["K"][b, kf]) and np.array_equal(dk[0, 0], ref["d"][b, kf]), fam
            continue
        D = hc.scale_vector(fam, n, hc.level(fam, "s", n, m))
        errs = {"K": hc.blockerr(hc._mat(Kk, m, n), hc._mat(rec[7:7 + m * n].reshape(1, 1, -1), m, n), None if D is None else (None, D)),
                "d": hc.blockerr(dk, rec[7 + m * n:].reshape(1, 1, m))}
        i0 = 5 if cfg.kind == "pure" else 3
        floor = fx["fail_benign"][5:7] if cfg.kind == "pure" else np.full(2, 1e-13 if cfg.kind == "f64" else 2.0 ** -23)
        judge(cfg, fam, errs, dict(zip(("K", "d"), np.maximum(rec[i0:i0 + 2], floor))), "unsolved", bad)
    assert not bad, bad


def nine(n, m, fx):
    """Nine problems that interleave the families: hard, benign, failing, three times over (fp32 level, fp32-representable inputs, so
    that every dtype takes the same numbers).  Returns the batch and the indices of the failing ones."""
    ben = hc.problem("benign", n, m, "s")
    parts = []
    for i, (hard, failing) in enumerate((("unstable", "collinear"), ("cheap", "unstable"), ("scales", "cross"))):
        parts.append(hc.take(hc.problem(hard, n, m, "s"), [0]))
        parts.append(hc.take(ben, [i]))
        parts.append(hc.take(hc.with_failure(hc.problem(failing, n, m, "s"), fx["fail_%s" % failing][0]), [hc.FAIL_PROBLEM]))
    return hc.stack(parts), (2, 5, 8)


@pytest.mark.parametrize("cfg", EXACT + REASSOC + OTHER_F32, ids=_id)
def test_neighbours_do_not_see_each_other(cfg):
    """A batch that interleaves hard, benign and failing problems against every one of them alone in a batch of one (of four copies of
    itself where the kernel takes four problems per wave): the same bits.  A problem that shares a wave or a tile with a failing or
    badly scaled one must not see it."""
    n, m = cfg.shape
    pr, failing = nine(n, m, fixture(cfg.shape))
    together = run(cfg, hc.stack([pr, hc.take(pr, [0, 1, 2])]) if x4(cfg) else pr)
    assert together["status"][:9].tolist() == [hc.FAIL_KNOT if i in failing else -1 for i in range(9)] or cfg.kind == "f32"
    for i in range(9):
        alone = run(cfg, hc.take(pr, [i] * (4 if x4(cfg) else 1)))
        assert alone["status"][0] == together["status"][i], i
        st = int(alone["status"][0])                                   # (what lies below a failing knot point was never written)
        lo, plo = max(st, 0), st + 1
        for q in ("K", "d"):
            assert np.array_equal(alone[q][0, lo:], together[q][i, lo:], equal_nan=True), (i, q)
        for q in ("P", "p"):
            assert np.array_equal(alone[q][0, plo:], together[q][i, plo:], equal_nan=True), (i, q)
        if alone["status"][0] == -1:
            for q in ("dV", "x", "u", "y"):
                assert np.array_equal(alone[q][0], together[q][i]), (i, q)
