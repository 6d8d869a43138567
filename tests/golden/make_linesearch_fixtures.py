#!/usr/bin/env python3
"""Writes tests/golden/reference_linesearch.npz: what the reference's own line search (linesearch::CubicLineSearch::Run, built
into oracle/_ref by `make -C oracle ref` from the reference tree) returns on the 1600 seeded cases below -- status,
iterations, step, final merit value and the exact sequence of trial steps.  Results only: with them
tests/test_oracle_linesearch.py pins the oracle to the reference where the reference tree is absent.

    python tests/golden/make_linesearch_fixtures.py        # needs oracle/_ref, built where the reference tree is present
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle          # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_linesearch.npz")


def quad(a, c):
    return lambda x: (a * (x - c) ** 2, 2 * a * (x - c))


def cubic(c):
    return lambda x: ((x - c) ** 2 - (x - c) ** 3, 2 * (x - c) - 3 * (x - c) ** 2)


def cases():
    """(merit function, phi0, dphi0, try_cubic_first, use_backtracking) of the 1600 cases, in order."""
    rng = np.random.default_rng(7)
    for trial in range(400):
        kind = trial % 4
        if kind == 0:
            a, c = rng.uniform(0.1, 5), rng.uniform(-0.5, 3)
            fn = quad(a, c)
        elif kind == 1:
            fn = cubic(rng.uniform(0.01, 2.5))
        elif kind == 2:
            w, s = rng.uniform(0.5, 6), rng.uniform(0.1, 3)
            fn = lambda x, w=w, s=s: (-s * np.sin(w * x) + 0.3 * x * x, -s * w * np.cos(w * x) + 0.6 * x)
        else:
            k, c = rng.uniform(1, 30), rng.uniform(0.001, 0.5)
            fn = lambda x, k=k, c=c: (np.cosh(k * (x - c)), k * np.sinh(k * (x - c)))
        phi0, dphi0 = fn(0.0)
        for tcf in (0, 1):
            for bt in (0, 1):
                yield fn, phi0, dphi0, tcf, bt


def run_reference(R, fn, phi0, dphi0, tcf, bt):
    """-> (status, iterations, step, final phi, trial steps) of the reference library R (oracle.ref_linesearch())."""
    evals = []

    def cb(a, phi, dphi, ctx):
        p, dp = fn(a)
        evals.append(a)
        phi[0] = p
        if dphi:
            dphi[0] = dp

    st, it, ph, dph = C.c_int(), C.c_int(), C.c_double(), C.c_double()
    alpha = R.ref_ls_run(oracle.MERIT_FN(cb), None, 1.0, phi0, dphi0, tcf, bt, C.byref(st), C.byref(it), C.byref(ph), C.byref(dph))
    return st.value, it.value, alpha, ph.value, evals


def main():
    oracle.build()
    R = oracle.ref_linesearch()
    if R is None:
        raise SystemExit("oracle/_ref is not built: the reference tree is needed to record its results")
    rows = [run_reference(R, *c) for c in cases()]
    np.savez_compressed(OUT, status=np.array([r[0] for r in rows], dtype=np.int32),
                        iters=np.array([r[1] for r in rows], dtype=np.int32), alpha=np.array([r[2] for r in rows]),
                        phi=np.array([r[3] for r in rows]), n_evals=np.array([len(r[4]) for r in rows], dtype=np.int32),
                        evals=np.array([a for r in rows for a in r[4]]))
    print("wrote %s: %d cases, %d bytes" % (OUT, len(rows), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
