"""Makes tests/golden/hard_tvlqr_<n>x<m>.npz: the extended-precision reference of the hard TVLQR families (tests/hard_cases.py).

    python tests/golden/make_hard_tvlqr_fixtures.py [n m ...]      (needs mpmath; every shape when none is named)

Per (family, shape) the textbook recursion (tvlqr.cpp:65-248's formulas, the forward pass with the extended-precision gains) is run
with mpmath at 60 digits and rounded to double once; a second run at 120 digits must give the identical arrays.  Stored per case:
  sum_<family>_<d|s>    checksum of the regenerated inputs (golden_cases.checksum)
  ref_<family>_<d|s>    K, d, P, p, dV, x, u, y packed by hard_cases.pack ("s": the fp32 level on fp32-rounded inputs; tile shapes only)
  e64_<family>_<d|s>    blockerr of oracle.backward_batch / forward_batch against it, per quantity (hard_cases.QUANTITIES)
  e32_<family>_s        the same for a straight numpy float32 recursion (hard_cases.riccati_numpy)
  fail_<family>         the failure case (fp32 level, problem FAIL_PROBLEM, knot point FAIL_KNOT): [shift, failing pivot / max|Quu|, smallest
                        pivot / max|Quu| of the problems that factor, e64 of K_k, e64 of d_k, e32 of K_k, e32 of d_k, Qux (m n), -Qu (m)]
Data only: inputs come from tests/problems.py's generators, the numbers from mpmath, the oracle and numpy."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import hard_cases as hc                    # noqa: E402
from tests.golden_cases import checksum               # noqa: E402

N = hc.N


def mp_solve(pr, digits, problems_=None, stop_at=None, forward=True):
    """The recursion at `digits` decimal digits.  Returns the outputs rounded to double (full horizon), the smallest Cholesky pivot
    relative to max|Quu| per problem, and per problem the extended-precision (Qux, Qu, Quu) at knot point `stop_at` (where the
    recursion of that problem then ends)."""
    import mpmath as mp
    mp.mp.dps = digits
    n, m = pr["n"], pr["m"]
    B_ = pr["A"].shape[0]
    M = lambda a, r, c: mp.matrix(r, c) if a is None else mp.matrix([[mp.mpf(float(a[i + r * j])) for j in range(c)] for i in range(r)])
    V = lambda a: mp.matrix([mp.mpf(float(v)) for v in a])
    fl = lambda X, r, c: np.array([[float(X[i, j]) for j in range(c)] for i in range(r)])
    out = dict(K=np.zeros((B_, N, m * n)), d=np.zeros((B_, N, m)), P=np.zeros((B_, N + 1, n * n)), p=np.zeros((B_, N + 1, n)),
               dV=np.zeros((B_, 2)), x=np.zeros((B_, N + 1, n)), u=np.zeros((B_, N, m)), y=np.zeros((B_, N + 1, n)))
    margin = np.full(B_, np.inf)
    stopped = {}
    for b in (range(B_) if problems_ is None else problems_):
        P = [None] * (N + 1); p = [None] * (N + 1); K = [None] * N; d = [None] * N
        P[N] = M(pr["Q"][b, N], n, n); p[N] = V(pr["q"][b, N])
        dV0 = dV1 = mp.mpf(0)
        for k in range(N - 1, -1, -1):
            A, Bm, f = M(pr["A"][b, k], n, n), M(pr["B"][b, k], n, m), V(pr["f"][b, k])
            Q, R, H = M(pr["Q"][b, k], n, n), M(pr["R"][b, k], m, m), M(pr["H"][b, k], m, n)
            q, r = V(pr["q"][b, k]), V(pr["r"][b, k])
            AtP = A.T * P[k + 1]
            BtP = Bm.T * P[k + 1]
            Qxx = Q + AtP * A
            Quu = R + BtP * Bm
            Qux = H + BtP * A
            t = p[k + 1] + P[k + 1] * f
            Qx = q + A.T * t
            Qu = r + Bm.T * t
            if stop_at is not None and k == stop_at:
                stopped[b] = (Qux, Qu, Quu)
                break
            # unblocked lower Cholesky, pivots watched
            L = mp.matrix(m, m)
            big = max(abs(Quu[i, j]) for i in range(m) for j in range(m))
            for j in range(m):
                s = Quu[j, j] - mp.fsum(L[j, c] * L[j, c] for c in range(j))
                margin[b] = min(margin[b], float(s / big))
                assert s > 0, ("the exact recursion is indefinite", b, k, j)
                L[j, j] = mp.sqrt(s)
                for i in range(j + 1, m):
                    L[i, j] = (Quu[i, j] - mp.fsum(L[i, c] * L[j, c] for c in range(j))) / L[j, j]

            def solve(rhs, cols):
                X = mp.matrix(m, cols)
                for c in range(cols):
                    yv = [None] * m
                    for i in range(m):
                        yv[i] = (rhs[i, c] - mp.fsum(L[i, j] * yv[j] for j in range(i))) / L[i, i]
                    for i in range(m - 1, -1, -1):
                        X[i, c] = (yv[i] - mp.fsum(L[j, i] * X[j, c] for j in range(i + 1, m))) / L[i, i]
                return X
            K[k] = solve(Qux, n)
            d[k] = -solve(Qu, 1)
            QK = Quu * K[k]
            KtQux = K[k].T * Qux
            P[k] = Qxx + QK.T * K[k] - KtQux - KtQux.T
            p[k] = Qx - QK.T * d[k] - K[k].T * Qu + Qux.T * d[k]
            dV0 += (d[k].T * Qu)[0]
            dV1 += (d[k].T * (Quu * d[k]))[0] / 2
            out["K"][b, k] = fl(K[k], m, n).reshape(-1, order="F")
            out["d"][b, k] = fl(d[k], m, 1)[:, 0]
        else:
            out["dV"][b] = [float(dV0), float(dV1)]
        for k in range(N + 1):
            if P[k] is not None:
                out["P"][b, k] = fl(P[k], n, n).reshape(-1, order="F")
                out["p"][b, k] = fl(p[k], n, 1)[:, 0]
        if not forward or b in stopped:
            continue
        x = V(pr["x0"][b])
        for k in range(N + 1):
            out["x"][b, k] = fl(x, n, 1)[:, 0]
            out["y"][b, k] = fl(P[k] * x + p[k], n, 1)[:, 0]
            if k < N:
                u = d[k] - K[k] * x
                out["u"][b, k] = fl(u, m, 1)[:, 0]
                x = V(pr["f"][b, k]) + M(pr["A"][b, k], n, n) * x + M(pr["B"][b, k], n, m) * u
    return out, margin, stopped


def mp_to_np(X, r, c):
    return np.array([[float(X[i, j]) for j in range(c)] for i in range(r)])


def case(args):
    """One (shape, family): every array the fixture keeps for it."""
    n, m, family = args
    tile = (n, m) in hc.TILE_SHAPES
    D = {w: hc.scale_vector(family, n, hc.level(family, w, n, m)) for w in "ds"}
    out = {}
    for which in ("d", "s"):
        pr = hc.problem(family, n, m, which)
        out["sum_%s_%s" % (family, which)] = checksum(pr)
        full = which == "d" or tile
        if full:
            ref, margin, _ = mp_solve(pr, 60)
            ref2, _, _ = mp_solve(pr, 120)
            for k in hc.QUANTITIES:
                assert np.array_equal(ref[k], ref2[k]), ("60 and 120 digits round differently", n, m, family, which, k)
            cut = hc.at_knots(ref, n)
            out["ref_%s_%s" % (family, which)] = hc.pack(cut, n, m)
            e = hc.errors(hc.at_knots(hc.run_oracle(pr), n), cut, n, m, D[which])
            out["e64_%s_%s" % (family, which)] = np.array([e[k] for k in hc.QUANTITIES])
        if which == "s":
            r32 = hc.riccati_numpy(pr, np.float32)
            if full:
                assert (r32["status"] == -1).all(), ("the float32 recursion does not factor", n, m, family)
                e = hc.errors(hc.at_knots(r32, n), cut, n, m, D[which])
                out["e32_%s_s" % family] = np.array([e[k] for k in hc.QUANTITIES])
            else:
                _, margin, _ = mp_solve(pr, 60, problems_=[b for b in range(hc.BATCH) if b != hc.FAIL_PROBLEM], forward=False)
            # the failure case: what the recursion holds at FAIL_KNOT of FAIL_PROBLEM before the factorisation
            b, kf = hc.FAIL_PROBLEM, hc.FAIL_KNOT
            _, _, st = mp_solve(pr, 60, problems_=[b], stop_at=kf, forward=False)
            _, _, st2 = mp_solve(pr, 120, problems_=[b], stop_at=kf, forward=False)
            Qux, Qu, Quu = [mp_to_np(X, *s) for X, s in zip(st[b], ((m, n), (m, 1), (m, m)))]
            for X, Y, s in zip(st[b], st2[b], ((m, n), (m, 1), (m, m))):
                assert np.array_equal(mp_to_np(X, *s), mp_to_np(Y, *s))
            shift = 2.0 ** np.ceil(np.log2(2.0 * np.abs(Quu).max()))
            # the last pivot of Quu - shift e e^T is at most Quu[m-1, m-1] - shift (a Schur complement never exceeds its diagonal entry)
            fail_margin = (Quu[m - 1, m - 1] - shift) / (np.abs(Quu).max() + shift)
            ok_margin = float(np.delete(margin, b).min())
            assert fail_margin < -1e-3 and ok_margin > 1e-6, (n, m, family, fail_margin, ok_margin)
            prf = hc.with_failure(pr, shift)
            from oracle import oracle
            o = oracle.backward_batch(prf["A"], prf["B"], prf["f"], prf["Q"], prf["R"], prf["H"], prf["q"], prf["r"])
            want = [-1] * hc.BATCH; want[b] = kf
            assert o["status"].tolist() == want, (n, m, family, o["status"])
            Kf, df = Qux.reshape(1, 1, m, n), -Qu.reshape(1, 1, m)
            Df = None if D["s"] is None else (None, D["s"])
            eK = hc.blockerr(hc._mat(o["K"][b:b + 1, kf:kf + 1], m, n), Kf, Df)
            ed = hc.blockerr(o["d"][b:b + 1, kf:kf + 1], df)
            # the float32 recursion of the failing problem stops at kf: its Qux, Qu are what an unsolved knot point holds
            eK32, ed32 = _f32_unsolved(prf, b, kf, Kf, df, Df)
            out["fail_%s" % family] = np.concatenate([[shift, fail_margin, ok_margin, eK, ed, eK32, ed32],
                                                      Qux.reshape(-1, order="F"), -Qu.reshape(-1)])
    return out


def _f32_unsolved(prf, b, kf, Kf, df, Df):
    """Error of the float32 recursion's Qux, -Qu at the failing knot point (run on the problem without the shift down to kf + 1)."""
    n, m = prf["n"], prf["m"]
    one = hc.take(prf, [b])
    R = one["R"].copy(); R[0, kf] = np.eye(m).reshape(-1)        # any R that factors: Qux, Qu at kf do not depend on R_kf
    r32 = hc.riccati_numpy(dict(one, R=R), np.float32)
    f32 = np.float32
    Pn = hc._mat(r32["P"], n, n)[0, kf + 1].astype(f32); pn = r32["p"][0, kf + 1].astype(f32)
    A = hc._mat(one["A"], n, n)[0, kf].astype(f32); Bm = hc._mat(one["B"], n, m)[0, kf].astype(f32)
    H = hc._mat(one["H"], m, n)[0, kf].astype(f32)
    t = pn + Pn @ one["f"][0, kf].astype(f32)
    Qux = H + Bm.T @ Pn @ A
    Qu = one["r"][0, kf].astype(f32) + Bm.T @ t
    return (hc.blockerr(Qux.astype(np.float64).reshape(1, 1, m, n), Kf, Df),
            hc.blockerr(-Qu.astype(np.float64).reshape(1, 1, m), df))


def make(shape, pool):
    n, m = shape
    arrays = {}
    for res in pool.map(case, [(n, m, fam) for fam in hc.FAMILIES]):
        arrays.update(res)
    path = hc.fixture_path(n, m)
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:       # np.savez stamps the time of day into the archive: not reproducible
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), "w") as f:
                np.lib.format.write_array(f, np.asarray(arrays[k]), allow_pickle=False)
    print("%s: %d bytes" % (os.path.relpath(path, ROOT), os.path.getsize(path)), flush=True)


if __name__ == "__main__":
    import multiprocessing
    a = [int(v) for v in sys.argv[1:]]
    shapes = list(zip(a[0::2], a[1::2])) or list(hc.SHAPES)
    with multiprocessing.Pool(min(6, os.cpu_count() or 1)) as pool:
        for s in shapes:
            make(s, pool)
