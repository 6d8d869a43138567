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
Cfg = collections.namedtuple("Cfg", "name shape plan dtype flags kind forms", defaults=(0,))
G, T16, LN, T32 = altro_amd.PLAN_GENERIC, altro_amd.PLAN_MFMA16, altro_amd.PLAN_LANE, altro_amd.PLAN_MFMA32
F64, F32 = altro_amd.F64, altro_amd.F32
_id = lambda c: "%s-%dx%d" % ((c.name,) + c.shape)
LQ_ON = altro_amd.FORM_GENERIC_LATE_Q_ON
MC = altro_amd.GENERIC_MATRIX_CORES
GROUP = 16                                           # problems of one workgroup of mfma16_forward_group_kernel

# generic_lq, generic_mc_lq, generic_f32_lq: generic_backward_kernel<.., LQ = true> ("late Q"), which the launcher's rule takes from
# 769 .. 3073 problems up on these shapes (sweep_route.h), forced here at the batches of this file; mfma16_group: the forward sweep of a
# batch of whole groups of 16 (the batch is padded with the first problems again).  Each run asserts that the instantiation it means ran.
EXACT = ([Cfg("generic", s, G, F64, 0, "exact") for s in hc.SHAPES] + [Cfg("lane", s, LN, F64, 0, "exact") for s in hc.LANE_SHAPES]
         + [Cfg("generic_lq", s, G, F64, 0, "exact", LQ_ON) for s in hc.SHAPES])
REASSOC = ([Cfg("mfma16", s, T16, F64, 0, "f64") for s in hc.TILE_SHAPES] + [Cfg("mfma32", s, T32, F64, 0, "f64") for s in hc.TILE32_SHAPES]
           + [Cfg("mfma16_group", s, T16, F64, 0, "f64") for s in hc.TILE_SHAPES]
           + [Cfg("generic_mc", s, G, F64, MC, "f64") for s in hc.MC_SHAPES]
           + [Cfg("generic_mc_lq", s, G, F64, MC, "f64", LQ_ON) for s in hc.MC_SHAPES + ((16, 8), (24, 8))]
           + [Cfg("mfma16_f32", s, T16, F32, 0, "mixed") for s in hc.TILE_SHAPES]
           # the two pure-fp32 kernel pairs: one problem per wave (a batch that is no multiple of four) and four problems per wave
           + [Cfg("mfma16_pure", s, T16, F32, altro_amd.F32_PURE, "pure") for s in hc.TILE_SHAPES]
           + [Cfg("mfma16_pure_x4", s, T16, F32, altro_amd.F32_PURE, "pure") for s in hc.TILE_SHAPES])
OTHER_F32 = ([Cfg("lane_f32", s, LN, F32, 0, "f32") for s in hc.LANE_SHAPES] + [Cfg("generic_f32", s, G, F32, 0, "f32") for s in ((13, 4), (20, 8))]
             + [Cfg("generic_f32_lq", s, G, F32, 0, "f32", LQ_ON) for s in ((13, 4), (20, 8))])
OUT = ("K", "d", "P", "p", "dV")
_fx = {}


def fixture(shape):
    if shape not in _fx:
        _fx[shape] = hc.load(*shape)
    return _fx[shape]


def x4(cfg):
    return cfg.name.endswith("_x4")


def group(cfg):
    return cfg.name == "mfma16_group"


def pad_to(cfg):
    """The batch of `cfg` is a multiple of this (the kernel under test takes whole quads / whole groups)."""
    return 4 if x4(cfg) else GROUP if group(cfg) else 1


def padded(cfg, pr):
    """`pr` with the first problems again up to a whole quad / group."""
    batch, w = pr["A"].shape[0], pad_to(cfg)
    if batch % w == 0:
        return pr
    extra = [i % batch for i in range(w - batch % w)]
    return hc.stack([pr, hc.take(pr, extra)])


def check_variant(cfg, bt, forward):
    """The instantiation `cfg` names is the one the handle's last launches were (altro_hip_sweep_variant / profile_get)."""
    if cfg.plan == G:
        want = (altro_amd.SWEEP_LATE_Q if cfg.forms & LQ_ON else 0) | (altro_amd.SWEEP_MATRIX_CORES if cfg.flags & MC else 0)
        assert bt.sweep_variant(0) == want, (_id(cfg), bt.sweep_variant(0), want)
        assert bt.profile_get(0)[2] == "generic_backward_kernel"
    if forward and cfg.plan == T16 and cfg.dtype == F64:
        assert bt.profile_get(1)[2] == ("mfma16_forward_group_kernel" if group(cfg) else "mfma16_forward_kernel"), _id(cfg)


def open_batch(cfg, pr):
    batch = pr["A"].shape[0]
    bt = altro_amd.Batch(hc.N, pr["n"], pr["m"], batch, dtype=cfg.dtype, plan=cfg.plan, flags=cfg.flags)
    assert bt.plan == cfg.plan
    if cfg.forms:
        bt.set_forms(cfg.forms)
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
    """Backward (and forward) sweep of `pr` on `cfg`; the four-problems-per-wave kernels get a batch of whole quads, the group forward
    kernel one of whole groups (the first problems again), of which the caller sees the problems it gave."""
    batch = pr["A"].shape[0]
    pr = padded(cfg, pr)
    bt = open_batch(cfg, pr)
    bt.backward()
    if forward:
        bt.forward_ltv()
    check_variant(cfg, bt, forward)
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


@pytest.mark.parametrize("cfg", [c for c in EXACT + REASSOC if not group(c)], ids=_id)   # (mfma16_group's backward sweep is mfma16's)
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
        check_variant(cfg, bt, False)
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
    w = pad_to(cfg)
    together = run(cfg, padded(cfg, pr))      # (mfma16_group: the nine and the first seven again are ONE group)
    assert together["status"][:9].tolist() == [hc.FAIL_KNOT if i in failing else -1 for i in range(9)] or cfg.kind == "f32"
    for i in range(9):
        alone = run(cfg, hc.take(pr, [i] * w))
        same_as_alone(alone, 0, together, i)


def same_as_alone(alone, j, together, i):
    assert alone["status"][j] == together["status"][i], i
    st = int(alone["status"][j])                                   # (what lies below a failing knot point was never written)
    lo, plo = max(st, 0), st + 1
    for q in ("K", "d"):
        assert np.array_equal(alone[q][j, lo:], together[q][i, lo:], equal_nan=True), (i, q)
    for q in ("P", "p"):
        assert np.array_equal(alone[q][j, plo:], together[q][i, plo:], equal_nan=True), (i, q)
    if alone["status"][j] == -1:
        for q in ("dV", "x", "u", "y"):
            assert np.array_equal(alone[q][j], together[q][i]), (i, q)


def test_group_forward_failing_problems_in_the_first_and_last_wave():
    """Two groups of mfma16_forward_group_kernel; the failing problems sit in wave 0 and wave 15 of the first group, whose other
    fourteen waves and the whole second group hold hard and benign problems.  Sixteen waves share one LDS ring and one barrier per
    step: every problem must come out as it does in the wave-per-problem kernel (ALTRO_HIP_FORM_FORWARD_WAVE), bit for bit, and the
    healthy ones must meet the criterion of this file against the fixture's extended-precision trajectories."""
    n, m = 12, 4
    cfg = Cfg("mfma16_group", (n, m), T16, F64, 0, "f64")
    fx = fixture((n, m))
    pr, failing = nine(n, m, fx)
    healthy = [i for i in range(9) if i not in failing]
    order = [failing[0]] + [healthy[i % 6] for i in range(14)] + [failing[1]] + [healthy[i % 6] for i in range(15)] + [failing[2]]
    batch = hc.take(pr, order)
    assert len(order) == 2 * GROUP
    out = run(cfg, batch)
    wave = run(cfg._replace(name="mfma16", forms=altro_amd.FORM_FORWARD_WAVE), batch)
    assert out["status"].tolist() == [hc.FAIL_KNOT if i in failing else -1 for i in order]
    for j in range(2 * GROUP):
        same_as_alone(wave, j, out, j)
    # problems 0 (unstable) and 1 (benign) of the nine sit next to the failing wave 0 and wave 15 and all over the second group: their
    # trajectories against the fixture's, e_cpu the oracle's stored error on the same fp32-level inputs, floor 1e-13 (fp64 arithmetic)
    bad = []
    for fam, i in (("unstable", 0), ("benign", 1)):
        ref = hc.unpack(fx["ref_%s_s" % fam], n, m)
        lim = dict(zip(hc.QUANTITIES, np.maximum(fx["e64_%s_s" % fam], 1e-13)))
        for j in [j for j, o in enumerate(order) if o == i]:
            errs = {q: hc.blockerr(out[q][j:j + 1], ref[q][0:1]) for q in ("x", "u", "y")}
            judge(cfg, fam, errs, lim, "slot %d" % j, bad)
    assert not bad, bad


def _lq_twin(cfg):
    return cfg._replace(name=cfg.name[:-3], forms=0)


@pytest.mark.parametrize("cfg", [c for c in OTHER_F32 if c.name == "generic_f32_lq"], ids=_id)
def test_late_q_fp32_forms_the_same_sums(cfg):
    """generic_backward_kernel<float, .., LQ = true> promises the sums of the form with a block for Qxx, in the same order: the same
    bits on every family (fp32 level), status included; and the project's fp32 tolerance, 2e-4 relative, to the oracle on the benign one."""
    n, m = cfg.shape
    for fam in hc.FAMILIES:
        pr = hc.problem(fam, n, m, "s")
        out, twin = run(cfg, pr), run(_lq_twin(cfg), pr)
        assert np.array_equal(out["status"], twin["status"]), fam
        for q in hc.QUANTITIES:
            assert np.array_equal(out[q], twin[q], equal_nan=True), (fam, q)
        if fam == "benign":
            ref = hc.run_oracle(pr)
            assert (out["status"] == -1).all()
            for q in hc.QUANTITIES:
                err = np.abs(out[q] - ref[q]).max() / max(1.0, np.abs(ref[q]).max())
                print("%-16s benign %s rel err %.3g" % (_id(cfg), q, err))
                assert err < 2e-4, (q, err)


@pytest.mark.parametrize("cfg", [c for c in REASSOC if c.name == "generic_mc_lq"], ids=_id)
def test_late_q_matrix_cores_against_its_sibling(cfg):
    """The late-Q form of the matrix-core kernel against the form with a block for Qxx.  With the products on the matrix cores the
    paired pass (Qx_tmp += P' f, Quu += Qux_tmp B) is two tile products one after the other in both forms (wave_gemm_pair_sel), so
    late Q changes where Q_k comes from and nothing about any sum: the same bits, on every family.  Printed for DESIGN section 2."""
    n, m = cfg.shape
    for fam in hc.FAMILIES:
        pr = hc.problem(fam, n, m, "d")
        out, twin = run(cfg, pr), run(_lq_twin(cfg), pr)
        assert np.array_equal(out["status"], twin["status"]), fam
        diff = {q: float(np.abs(out[q] - twin[q]).max() / max(np.abs(twin[q]).max(), 1e-300)) for q in hc.QUANTITIES}
        print("%-16s %-9s bit-identical to generic_mc: %s  (max rel diff %.2g)" % (_id(cfg), fam, all(v == 0 for v in diff.values()), max(diff.values())))
        for q in hc.QUANTITIES:
            assert np.array_equal(out[q], twin[q]), (fam, q)
