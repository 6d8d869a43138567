"""Hard TVLQR problem families, graded by difficulty, and the metric the kernels are judged by on them.  Shared by the fixture
generator (tests/golden/make_hard_tvlqr_fixtures.py, which runs an extended-precision Riccati recursion), the CPU test that pins the
yardstick (tests/test_hard_tvlqr_cases.py) and the GPU test (tests/test_gpu_hard_tvlqr.py).  Nothing here needs mpmath or the GPU.

Every input is regenerated from problems.py's counter-based generators; the fixtures hold only a checksum of it.

Families (`level` is the knob; LEVELS holds the fp64 level "d" and the fp32 level "s" of each):
  benign     problems.random_ltv as it is (no knob).
  unstable   A = I + g sqrt(12 / n) N(0,1), B = 0.3 N(0,1): the cost-to-go grows along the horizon, at about the same rate for
             every n (the spectral radius of the random part goes with sqrt(n)).  level = g.
  cheap      B = N(0,1), R scaled by 10^-e, H by 10^(-e/2): Quu is dominated by B^T P B.  level = e.
  collinear  columns B_j = B_0 + eps N(0,1), R scaled by 1e-6, H by 1e-3: cond(Quu) ~ 1 / eps^2 ... 1e8.  level = eps.
  scales     state scales D = 10^linspace(-e, e, n): A -> D A D^-1, B -> D B, f -> D f, Q -> D^-1 Q D^-1, q -> D^-1 q, x0 -> D x0,
             H = 0: the blocks of one problem span 4 e orders of magnitude.  level = e.
  cross      H = (1 - c) L_R W L_Q^T with R = L_R L_R^T, Q = L_Q L_Q^T (Cholesky factors as the square roots) and W a random partial
             isometry: the stage cost [Q H^T; H R] is barely positive semidefinite.  level = c.
Every family keeps [Q H^T; H R] >= 0: where R is scaled by s, H is scaled by sqrt(s).
"""
import numpy as np

from tests import problems

N = 24
BATCH = 3
FAMILIES = ("benign", "unstable", "cheap", "collinear", "scales", "cross")
# (fp64 level, fp32 level).  The fp64 level is the one that puts the oracle's own error into the family's band (BANDS); the fp32 level is
# one at which a straight numpy float32 recursion on the fp32-rounded inputs still factors everywhere, with an error against the
# extended-precision result between 1e-5 and 1e-2 where the level had to change (tests/test_hard_tvlqr_cases.py asserts both).
LEVELS = {"benign": (None, None), "unstable": (0.25, 0.2), "cheap": (7.0, 7.0), "collinear": (1e-2, 1e-1), "scales": (3.0, 3.0),
          "cross": (1e-3, 1e-3)}
# fp64 levels of the shapes on which the family's level lands outside its band: fewer states take more growth per step to lose the
# same digits, two inputs have to be closer to collinear than four, six less close
SHAPE_LEVELS = {("unstable", (4, 2)): 0.35, ("unstable", (2, 1)): 0.47, ("unstable", (6, 3)): 0.3, ("unstable", (9, 6)): 0.3,
                ("collinear", (12, 2)): 3e-3, ("collinear", (9, 6)): 3e-2}
# e_cpu64(K), the oracle's own error in K against the extended-precision result, per family: [low, high)
BANDS = {"benign": (0.0, 1e-13), "unstable": (1e-12, 1e-10), "cheap": (0.0, 1e-13), "collinear": (1e-9, 1e-7), "scales": (0.0, 1e-13),
         "cross": (0.0, 1e-13)}


def level(family, which, n, m):
    if which == "d" and (family, (n, m)) in SHAPE_LEVELS:
        return SHAPE_LEVELS[(family, (n, m))]
    return LEVELS[family][0 if which == "d" else 1]


def band(family, n, m):
    """The band of e_cpu64(K) at the fp64 level.  One input cannot be collinear with itself: (n, 1) is benign in that family."""
    return BANDS["benign"] if (family == "collinear" and m == 1) else BANDS[family]


TILE_SHAPES = ((12, 4), (7, 3), (12, 2))            # plan MFMA16: the tile and two zero-padded shapes (fp64, fp32 storage, pure fp32)
LANE_SHAPES = ((4, 2), (2, 1), (6, 3))              # plan LANE: quad, quad2 and lane kernels
TILE32_SHAPES = ((13, 4), (9, 6), (16, 8), (24, 8))  # plan MFMA32
MC_SHAPES = ((20, 8),)                               # plan GENERIC's matrix-core option
SHAPES = TILE_SHAPES + LANE_SHAPES + TILE32_SHAPES + MC_SHAPES
FAIL_PROBLEM, FAIL_KNOT = 1, 9                       # the problem and knot point of the failure cases
QUANTITIES = ("K", "d", "P", "p", "dV", "x", "u", "y")


def knots(n):
    """Knot points whose K / P the fixtures keep (all K of the small shapes; the files stay below the largest committed fixture)."""
    big = n >= 16
    return (tuple(range(N)) if not big else (0, 1, N // 2, N - 1)), ((0, 1, N // 2, N - 1) if n < 12 else (0, 1, N // 2))


def fixture_path(n, m):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard_tvlqr_%dx%d.npz" % (n, m))


def _col(T):
    return np.ascontiguousarray(np.swapaxes(T, -1, -2)).reshape(T.shape[0], T.shape[1], -1)


def _mat(a, rows, cols):
    """[b, k, rows * cols] column-major blocks -> [b, k, rows, cols]."""
    return np.swapaxes(a.reshape(a.shape[0], a.shape[1], cols, rows), -1, -2)


def scale_vector(family, n, level):
    """The state scales D of the `scales` family at `level`, None for every other family."""
    return 10.0 ** np.linspace(-level, level, n) if family == "scales" else None


def problem(family, n, m, which="d"):
    """The three problems of (family, shape) at the fp64 level (which = "d") or at the fp32 level with every input rounded to fp32
    (which = "s"; still float64 arrays), in the layout of problems.random_ltv."""
    level_ = level(family, which, n, m)
    fi = FAMILIES.index(family)
    st = 300 + 40 * fi
    B_ = BATCH
    nrm = problems.normal
    if family == "benign":
        pr = problems.random_ltv(B_, N, n, m)
    else:
        base = problems.random_ltv(B_, N, n, m)             # Q, R, H, q, r, f, x0 of the benign recipe
        Q, R, H = _mat(base["Q"], n, n), _mat(base["R"], m, m), _mat(base["H"], m, n)
        A, Bm = _mat(base["A"], n, n), _mat(base["B"], n, m)
        f, q, r, x0 = base["f"], base["q"], base["r"], base["x0"]
        if family == "unstable":
            A = np.eye(n) + level_ * np.sqrt(12.0 / n) * nrm((B_, N, n, n), st)
            Bm = 0.3 * nrm((B_, N, n, m), st + 1)
        elif family == "cheap":
            Bm = nrm((B_, N, n, m), st + 1)
            R = R * 10.0 ** -level_
            H = H * 10.0 ** (-level_ / 2)
        elif family == "collinear":
            b0 = nrm((B_, N, n, 1), st + 1)
            Bm = b0 + level_ * nrm((B_, N, n, m), st + 2)
            R = R * 1e-6
            H = H * 1e-3
        elif family == "scales":
            D = scale_vector(family, n, level_)
            A = D[:, None] * A / D[None, :]
            Bm = D[:, None] * Bm
            f = f * D
            Q = Q / D[:, None] / D[None, :]
            q = q / D
            x0 = x0 * D
            H = np.zeros_like(H)
        elif family == "cross":
            LR = np.linalg.cholesky(R)
            LQ = np.linalg.cholesky(Q[:, :N])
            r_ = min(n, m)
            W = np.zeros((B_, N, m, n))
            G = nrm((B_, N, n, n), st + 1)
            for b in range(B_):
                for k in range(N):
                    U = np.linalg.qr(G[b, k])[0]
                    W[b, k, :r_, :] = U[:, :r_].T           # orthonormal rows: a partial isometry (m > n never occurs here)
            H = (1.0 - level_) * LR @ W @ np.swapaxes(LQ, -1, -2)
        pr = dict(N=N, n=n, m=m, A=_col(A), B=_col(Bm), f=f, Q=_col(Q), R=_col(R), H=_col(H), q=q, r=r, x0=x0)
    if which == "s":
        pr = {k: (v.astype(np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in pr.items()}
    return pr


def with_failure(pr, shift):
    """`pr` with the last diagonal entry of R of problem FAIL_PROBLEM at knot point FAIL_KNOT lowered by `shift` (the fixture's: twice the
    largest entry of the extended-precision Quu there, as a power of two): the last Cholesky pivot is then far below zero."""
    m = pr["m"]
    R = pr["R"].copy()
    R[FAIL_PROBLEM, FAIL_KNOT, m * m - 1] -= shift
    return dict(pr, R=R)


def scaled_cost(pr, k):
    """The whole cost times 4^k (exact in binary floating point)."""
    s = 4.0 ** k
    return dict(pr, **{key: pr[key] * s for key in ("Q", "R", "H", "q", "r")})


def take(pr, idx):
    """The problems `idx` of `pr` as a batch of their own."""
    return {k: (np.ascontiguousarray(v[idx]) if isinstance(v, np.ndarray) else v) for k, v in pr.items()}


def stack(prs):
    """Batches of one shape joined into one."""
    return {k: (np.concatenate([p[k] for p in prs]) if isinstance(v, np.ndarray) else v) for k, v in prs[0].items()}


# ---- the fixture's flat record -------------------------------------------------------------------------------------------------------
def layout(n, m):
    kk, pk = knots(n)
    return (("K", (BATCH, len(kk), m * n)), ("d", (BATCH, N, m)), ("P", (BATCH, len(pk), n * n)), ("p", (BATCH, N + 1, n)),
            ("dV", (BATCH, 2)), ("x", (BATCH, N + 1, n)), ("u", (BATCH, N, m)), ("y", (BATCH, N + 1, n)))


def pack(res, n, m):
    return np.concatenate([np.asarray(res[k], dtype=np.float64).reshape(-1) for k, _ in layout(n, m)])


def unpack(flat, n, m):
    out, o = {}, 0
    for k, shp in layout(n, m):
        c = int(np.prod(shp))
        out[k] = flat[o:o + c].reshape(shp)
        o += c
    assert o == flat.size
    return out


def at_knots(res, n):
    """Full-horizon outputs (K [b, N, ..], P [b, N + 1, ..]; ΔV under "dV" or "delta_V") cut down to what the fixtures keep."""
    kk, pk = knots(n)
    out = {k: np.asarray(res[k]) for k in ("d", "p", "x", "u", "y") if res.get(k) is not None}
    out["K"] = np.asarray(res["K"])[:, list(kk)]
    out["P"] = np.asarray(res["P"])[:, list(pk)]
    out["dV"] = np.asarray(res["dV"] if "dV" in res else res["delta_V"])
    return out


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
def blockerr(a, ref, scale=None):
    """max over (problem, knot point) of max|a - ref| / max|ref| taken per block.  No floor of 1 in the denominator; a block whose
    reference is exactly zero must be exactly zero (else the error is infinite).  `scale`, when given, multiplies the trailing axes of
    both first (a tuple of one vector per trailing axis, None to leave an axis alone)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.ndim == 2:                      # ΔV [b, 2]: each entry is its own block
        a, ref = a[..., None], ref[..., None]
    if scale is not None:
        for ax, s in enumerate(scale):
            if s is not None:
                shp = [1] * a.ndim
                shp[2 + ax] = -1
                a, ref = a * s.reshape(shp), ref * s.reshape(shp)
    ax = tuple(range(2, a.ndim))
    num, den = np.abs(a - ref).max(axis=ax), np.abs(ref).max(axis=ax)
    if not np.isfinite(num).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den > 0, num / den, np.where(num > 0, np.inf, 0.0))
    return float(e.max())


def errors(res, ref, n, m, D=None):
    """blockerr of every quantity both `res` and `ref` hold (in the fixtures' cut: at_knots), as {name: error}.  With the state scales D
    of the `scales` family the blocks are compared in the unscaled coordinates: K D, D P D, D p, D^-1 x, D y."""
    out = {}
    for k in QUANTITIES:
        if k not in res or k not in ref:
            continue
        a, b, sc = res[k], ref[k], None
        if k == "K":
            a, b = _mat(a, m, n), _mat(b, m, n)
            sc = None if D is None else (None, D)
        elif k == "P":
            a, b = _mat(a, n, n), _mat(b, n, n)
            sc = None if D is None else (D, D)
        elif k in ("p", "y") and D is not None:
            sc = (D,)
        elif k == "x" and D is not None:
            sc = (1.0 / D,)
        out[k] = blockerr(a, b, sc)
    return out


# ---- plain numpy recursions (the straight CPU computation in a working precision) ---------------------------------------------------
def riccati_numpy(pr, dtype=np.float64, symmetrise=False):
    """tvlqr.cpp:65-248's formulas in numpy at `dtype`, one problem after the other; with `symmetrise` the carried cost-to-go is
    replaced by (P + P^T) / 2 every step, as the tile kernels carry it.  Returns full-horizon K, d, P, p, dV, x, u, y and status."""
    n, m, B_ = pr["n"], pr["m"], pr["A"].shape[0]
    t = lambda a: a.astype(dtype)
    A, Bm, Q, R, H = t(_mat(pr["A"], n, n)), t(_mat(pr["B"], n, m)), t(_mat(pr["Q"], n, n)), t(_mat(pr["R"], m, m)), t(_mat(pr["H"], m, n))
    f, q, r, x0 = t(pr["f"]), t(pr["q"]), t(pr["r"]), t(pr["x0"])
    K = np.zeros((B_, N, m, n), dtype); d = np.zeros((B_, N, m), dtype); P = np.zeros((B_, N + 1, n, n), dtype)
    p = np.zeros((B_, N + 1, n), dtype); dV = np.zeros((B_, 2), dtype); status = np.full(B_, -1, np.int32)
    x = np.zeros((B_, N + 1, n), dtype); u = np.zeros((B_, N, m), dtype); y = np.zeros((B_, N + 1, n), dtype)
    half = dtype(0.5)
    for b in range(B_):
        P[b, N] = Q[b, N]; p[b, N] = q[b, N]
        for k in range(N - 1, -1, -1):
            Pn, pn = P[b, k + 1], p[b, k + 1]
            Qxx = Q[b, k] + A[b, k].T @ Pn @ A[b, k]
            BP = Bm[b, k].T @ Pn
            Quu = R[b, k] + BP @ Bm[b, k]
            Qux = H[b, k] + BP @ A[b, k]
            t_ = pn + Pn @ f[b, k]
            Qx = q[b, k] + A[b, k].T @ t_
            Qu = r[b, k] + Bm[b, k].T @ t_
            try:
                Lc = np.linalg.cholesky(Quu)
            except np.linalg.LinAlgError:
                status[b] = k
                break
            if not np.isfinite(Lc).all():
                status[b] = k
                break
            sol = lambda rhs: np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs)).astype(dtype)
            Kk = sol(Qux); dk = -sol(Qu)
            QK = Quu @ Kk
            Pk = Qxx + QK.T @ Kk - Kk.T @ Qux - (Kk.T @ Qux).T
            if symmetrise:
                Pk = half * (Pk + Pk.T)
            pk = Qx - QK.T @ dk - Kk.T @ Qu + Qux.T @ dk
            dV[b, 0] += dk @ Qu; dV[b, 1] += half * (dk @ (Quu @ dk))
            K[b, k], d[b, k], P[b, k], p[b, k] = Kk, dk, Pk, pk
        if status[b] != -1:
            continue
        x[b, 0] = x0[b]
        for k in range(N):
            u[b, k] = d[b, k] - K[b, k] @ x[b, k]
            x[b, k + 1] = f[b, k] + A[b, k] @ x[b, k] + Bm[b, k] @ u[b, k]
            y[b, k] = P[b, k] @ x[b, k] + p[b, k]
        y[b, N] = P[b, N] @ x[b, N] + p[b, N]
    return dict(K=_col(K).astype(np.float64), d=d.astype(np.float64), P=_col(P).astype(np.float64), p=p.astype(np.float64),
                dV=dV.astype(np.float64), x=x.astype(np.float64), u=u.astype(np.float64), y=y.astype(np.float64), status=status)


def run_oracle(pr):
    """oracle.backward_batch / forward_batch on `pr`: the double-precision CPU path, full horizon."""
    from oracle import oracle
    o = oracle.backward_batch(pr["A"], pr["B"], pr["f"], pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"])
    if (o["status"] == -1).all():
        o.update(oracle.forward_batch(pr["A"], pr["B"], pr["f"], o["K"], o["d"], o["P"], o["p"], pr["x0"]))
    return o


def load(n, m):
    """The fixture of one shape as {name: array}."""
    with np.load(fixture_path(n, m)) as z:
        return {k: z[k] for k in z.files}
