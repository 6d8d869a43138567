"""Pins oracle/linesearch_oracle.c against (a) the constants in the reference's line-search tests
(src/linesearch/test/linesearch_tests.cpp:134-270) and (b) the REAL reference code: its results on 1600 seeded cases, recorded
in tests/golden/reference_linesearch.npz by tests/golden/make_linesearch_fixtures.py, and the library itself
(oracle/_ref/liblinesearch_ref.so, `make -C oracle ref`) where the reference tree was there to build it.  CPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_linesearch_fixtures as mk   # noqa: E402
from make_linesearch_fixtures import cubic, quad   # noqa: E402


def run_oracle(fn, c1=1e-4, c2=0.9, try_cubic_first=0, backtracking=0):
    L = oracle.lib()
    ls = oracle.LineSearch()
    L.oracle_ls_defaults(C.byref(ls))
    ls.c1, ls.c2, ls.try_cubic_first, ls.use_backtracking = c1, c2, try_cubic_first, backtracking
    evals = []

    def cb(a, phi, dphi, ctx):
        p, dp = fn(a)
        evals.append(a)
        phi[0] = p
        if dphi:
            dphi[0] = dp

    phi0, dphi0 = fn(0.0)
    alpha = L.oracle_ls_run(C.byref(ls), oracle.MERIT_FN(cb), None, 1.0, phi0, dphi0)
    return alpha, ls, evals


def test_reference_quadratic_cases():
    alpha, ls, _ = run_oracle(quad(1.0, 1.0))
    assert ls.n_iters == 1 and alpha == 1.0 and ls.status == 1
    alpha, ls, _ = run_oracle(quad(1.0, 1.1))
    assert ls.n_iters == 1 and alpha == 1.0
    alpha, ls, _ = run_oracle(quad(1.0, 1.1), c2=0.01)
    assert ls.n_iters == 3 and alpha == pytest.approx(1.1, rel=1e-15)
    alpha, ls, _ = run_oracle(quad(1.0, 0.8), c2=0.1)
    assert alpha == pytest.approx(0.8, rel=1e-15) and ls.status == 1
    alpha, ls, _ = run_oracle(quad(-1.0, -0.1))
    assert alpha == 2.0 and ls.sufficient_decrease and not ls.curvature and ls.status == 7


@pytest.mark.parametrize("c,c2,iters", [(1.0, 0.9, 1), (1.2, 1e-3, 3), (1.8, 0.01, 4), (0.8, 0.01, 2), (0.01, 0.01, 2)])
def test_reference_cubic_cases(c, c2, iters):
    alpha, ls, _ = run_oracle(cubic(c), c2=c2)
    assert ls.n_iters == iters
    assert alpha == pytest.approx(c, abs=1e-6)
    assert ls.status == 1


def test_against_real_reference_linesearch():
    rec = np.load(os.path.join(GOLDEN, "reference_linesearch.npz"))
    first = np.concatenate([[0], np.cumsum(rec["n_evals"])])
    R = oracle.ref_linesearch()      # the library as well, where it was built
    n_checked = 0
    for i, (fn, phi0, dphi0, tcf, bt) in enumerate(mk.cases()):
        alpha, ls, evals = run_oracle(fn, try_cubic_first=tcf, backtracking=bt)
        refs = [(int(rec["status"][i]), int(rec["iters"][i]), float(rec["alpha"][i]), float(rec["phi"][i]),
                 rec["evals"][first[i]:first[i + 1]].tolist())]
        if R is not None:
            refs.append(mk.run_reference(R, fn, phi0, dphi0, tcf, bt))
        for st, it, ralpha, ph, revals in refs:
            assert st == ls.status
            assert it == ls.n_iters
            assert revals == evals          # identical sequence of trial steps, bit for bit
            assert (np.isnan(ralpha) and np.isnan(alpha)) or ralpha == alpha
            if st != 3:
                assert ph == ls.phi
        n_checked += 1
    assert n_checked == 1600
