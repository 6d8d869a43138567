"""Makes tests/golden/loop_phases_<config>.npz: the extended-precision reference of the iLQR loop's phases on the seven configurations
of tests/cone_region_cases.py (N = 5, batch 7, zero duals, penalties 1 and 50) and on its HORIZON_CONFIGS (the tile's two at N = 17 and
N = 33: name them; at N = 33 only the merit phase's quantities are stored -- loop_scale_cases.MERIT_QUANTITIES -- so that the file
stays below the largest one under tests/golden; ecpu holds NaN for the others).

    python tests/golden/make_loop_phase_fixtures.py [config ...]      (needs mpmath; the seven configurations when none is named)

Per configuration and penalty the phase sequence of cone_region_cases.expand / phases is restated with mpmath at 60 digits and rounded
to double once; a second run at 120 digits must give the identical arrays:
  constraint values c = G [x; u] - g, ze = -rho c;  the projection onto the dual cone with its Jacobian J and, outside a second-order
  cone, the Hessian term d/dz (J^T z_proj);  the AL cost |z_proj|^2 / (2 rho), gradient -G^T J^T z_proj and Hessian
  rho (J G)^T (J G) + rho G^T Hs G;  the cost expansion (tracking form: q = -Qd xref, r = -Rd uref, c = the constant, all exact);
  the backward sweep (f = 0: the expansion is about the guess);  the closed-loop rollout of the merit function from x0 at alpha = 0 and
  alpha_b with phi, phi' and the candidates;  feasibility and stationarity of the last candidate.
Dynamics are linear in all seven; the two double-integrator configurations take the A, B that oracle/models_oracle.c forms with
H_DI (problems.di_blocks: b = h h / 2 in float arithmetic) as data.

Branches are FROZEN: which region a cone's ze lies in and which orthant rows are active is taken per (evaluation point, block,
problem, knot point, row) from the fp64 classification (loop_scale_cases.class_tables: cone_region_cases.classify_* at the guess and
at the oracle's two candidates), because at an exact tie the projection is continuous and its Jacobian is not; that branch's formulas
are what is evaluated here.  The table is stored, with the number of entries at which the comparison in extended precision would
have chosen otherwise (flips: zero in all seven).

Stored:  sum  checksum of the inputs (loop_scale_cases.inputs through golden_cases.checksum);  tab_<i>  the table of penalty RHOS[i];
ref_<i>_<quantity>  the results in the old units, batch-shaped, in the layouts of the oracle's getters;  ecpu_<i>  blockerr of the
oracle against them per quantity (loop_scale_cases.QUANTITIES);  flips_<i>.   Data only.

    python tests/golden/make_loop_phase_fixtures.py --duals [config ...]

makes tests/golden/loop_phases_duals_<config>.npz instead (the seven files above stay as they are): nonzero duals and the dual update.
mp_phases takes a STATE (loop_scale_cases: a dual vector per block, one penalty per problem, a guess): ze = z - rho c, and feasibility
from the value's own projection onto its cone (continuous: no branch).  Two runs per problem, at 60 and 120 digits:
  s1   the phases above at state S1 (the oracle's duals and raised penalties after a truncated solve, its steered guess), branches from
       loop_scale_cases.state_class_tables;
  up   the frozen solve from state S2 at penalty_initial = RHO0: the exact rollout of the input guess, z+ = Pi_K*(z - rho c) with the
       branches of the fp64 table at S2, rho+ = min(rho scaling, penalty_max), the second sweep's expansion and K, d, P, p at z+ (not
       rounded) and rho+, and z++ = Pi_K*(z+ - rho+ c), both with the branches of the fp64 table at the oracle's z+.
The arrays of the two runs are identical except at exact rounding ties (ties_to_even: 11 entries of P in three configurations).
Stored:  the inputs a GPU test needs to run without the oracle -- s1_* and s2_* (rho, x, u, z_<block>), s2_steered, the class tables
tab_s1 [3, ..], tab_u1, tab_u2 (int8), ls_mask [2, BATCH] (the problems on which the oracle's sweep with a real line search accepts
alpha = 1 in every unit system: cubic, backtracking);  sum  checksum of loop_scale_cases.inputs and of all of these;  ref_s1_<quantity>,
ref_z1_<block>, ref_z2_<block> ([BATCH, knot points of the block, p]), ref_rho1, ref_rho2, ref_sw2_<K, d, P, p>;  ecpu_s1 [QUANTITIES],
ecpu_z1 / ecpu_z2 [soc, orth, eq], ecpu_sw2 [K, d, P, p]: the oracle's blockerr against them;  flips_s1, flips_up.   Data only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import cone_region_cases as crc            # noqa: E402
from tests import loop_scale_cases as lsc             # noqa: E402
from tests import problems                            # noqa: E402
from tests.golden_cases import checksum               # noqa: E402

BATCH, RHOS = crc.BATCH, crc.RHOS


def mp_phases(cfg, b, rho, tab, digits, state=None, update=None):
    """Problem b of `cfg` at penalty rho with the branches of `tab` ([3, blocks, BATCH, N + 1, rows]: the guess, the candidate of
    alpha = 0, the candidate of alpha_b).  Returns ({quantity: float array in the oracle's layout}, flips).
    state (loop_scale_cases: dict(z, rho, x, u)): the guess and the duals are the state's, ze = z - rho c (rho: the caller passes the
    state's penalty of problem b).
    update = (tab_1, tab_2) ([blocks, BATCH, N + 1, rows] each) instead of the phases: the frozen solve from the state's duals and input
    guess at penalty_initial = rho.  The trajectory is the exact rollout of the state's u from x0; z+ = Pi(z - rho c) with the branches
    of tab_1; rho+ = min(rho scaling, penalty_max); the second sweep's expansion and backward sweep at z+ (not rounded) and rho+ with the
    branches of tab_2; z++ = Pi(z+ - rho+ c) with those branches too.  Returns ({"z1:<block>", "z2:<block>": [knot points, p], "rho1",
    "rho2", "K", "d", "P", "p"}, flips)."""
    import mpmath as mp
    mp.mp.dps = digits
    n, m, w, N = cfg.n, cfg.m, cfg.w, cfg.N
    F = lambda v: v if isinstance(v, mp.mpf) else mp.mpf(float(v))
    V = lambda a: [F(v) for v in a]
    M = lambda a, r, c: [[F(a[i + r * j]) for j in range(c)] for i in range(r)]          # column-major block -> rows
    dot = mp.fdot
    zero, half = mp.mpf(0), mp.mpf(1) / 2
    mv = lambda A, v: [dot(row, v) for row in A]
    mtv = lambda A, v: [dot([A[i][j] for i in range(len(A))], v) for j in range(len(A[0]))]
    add = lambda a, c: [x + y for x, y in zip(a, c)]
    rho_ = F(rho)
    flips = [0]

    # ---- inputs ----
    if cfg.dyn == "di":
        A_, B_ = problems.di_blocks(m, crc.H_DI)
        A = [[[F(v) for v in row] for row in A_]] * N
        B = [[[F(v) for v in row] for row in B_]] * N
        aff = [[zero] * n] * N
    else:
        p = cfg.p
        A = [M(p["A"][b, k], n, n) for k in range(N)]
        B = [M(p["B"][b, k], n, m) for k in range(N)]
        aff = [V(p["f"][b, k]) for k in range(N)]
    cost = []                                          # per knot point: (Q rows, R rows, H rows, q, r, c)
    for k in range(N + 1):
        kk = min(k, N - 1)
        if cfg.dense:
            p = cfg.p
            cost.append((M(p["Q"][b, k], n, n), M(p["R"][b, kk], m, m), M(p["H"][b, kk], m, n), V(p["q"][b, k]), V(p["r"][b, kk]), F(p["c"][b, k])))
        else:
            if cfg.dyn == "di":
                Qd, Rd, xr, ur = V(cfg.Qd), V(cfg.Rd), V(cfg.xref), [zero] * m
            else:
                p = cfg.p
                Qd, Rd, xr, ur = V(p["Qd"][b, k]), V(p["Rd"][b, kk]), V(p["xref"][b, k]), V(p["uref"][b, kk])
            c = half * dot([a * r for a, r in zip(Qd, xr)], xr) + (half * dot([a * r for a, r in zip(Rd, ur)], ur) if k < N else zero)
            cost.append(([[Qd[i] if i == j else zero for j in range(n)] for i in range(n)],
                         [[Rd[i] if i == j else zero for j in range(m)] for i in range(m)], [[zero] * n for _ in range(m)],
                         [-(a * r) for a, r in zip(Qd, xr)], [-(a * r) for a, r in zip(Rd, ur)], c))
    Gm = [[V(row) for row in bl["G"]] for bl in cfg.blocks]
    gm = [V(bl["g"]) for bl in cfg.blocks]

    def stage(k, x, u):
        """The cost's own value and gradient at (x, u) of knot point k."""
        Q, R, H, q, r, c = cost[k]
        Qx = mv(Q, x)
        J = half * dot(x, Qx) + dot(q, x) + c
        gx, gu = add(Qx, q), None
        if k < N:
            Ru, Hx = mv(R, u), mv(H, x)
            J += half * dot(u, Ru) + dot(r, u) + dot(u, Hx)
            gx = add(gx, mtv(H, u))
            gu = add(add(Ru, r), Hx)
        return J, gx, gu

    def constraint(j, k, x, u):
        z = x + (u if k < N else [zero] * m)
        return [dot(Gm[j][i], z) - gm[j][i] for i in range(cfg.blocks[j]["p"])]

    def project(j, ze, t):
        """ze of block j onto its dual cone with the branches t [rows]."""
        bl = cfg.blocks[j]
        pp = bl["p"]
        if bl["kind"] == "eq":
            return list(ze)
        if bl["kind"] == "orth":
            flips[0] += sum(int(int(t[i]) != (1 if ze[i] <= 0 else 0)) for i in range(pp))
            return [ze[i] if int(t[i]) else zero for i in range(pp)]
        v, s = ze[:pp - 1], ze[pp - 1]
        a = mp.sqrt(dot(v, v))
        region = int(t[0])
        flips[0] += int(region != (0 if a <= -s else (1 if a <= s else 2)))
        if region == 0:
            return [zero] * pp
        if region == 1:
            return list(ze)
        c = half * (1 + s / a)
        return [c * e for e in v] + [c * a]

    def violation(j, val):
        """max |Pi_K(val) - val| of block j (the projection onto the cone itself is continuous: no branch to freeze)."""
        bl = cfg.blocks[j]
        pp = bl["p"]
        if bl["kind"] == "eq":
            return max(abs(c) for c in val)
        if bl["kind"] == "orth":
            return max([zero] + [c for c in val if c > 0])
        vv, sv = val[:pp - 1], val[pp - 1]
        av = mp.sqrt(dot(vv, vv))
        if av <= sv:
            return zero
        if av <= -sv:
            return max(abs(c) for c in val)
        cv = half * (1 + sv / av)
        return max([abs(cv * e - e) for e in vv] + [abs(cv * av - sv)])

    duals = {}                                         # (block, knot point) -> the duals, zero where there are none
    if state is not None:
        for j, bl in enumerate(cfg.blocks):
            for k in range(bl["k0"], bl["k1"] + 1):
                duals[(j, k)] = V(state["z"][bl["name"]][b][k - bl["k0"]])

    def al(k, x, u, cls, hess, zd=None, rho_=rho_):
        """The AL terms at (x, u) of knot point k with the branches cls [blocks, rows]: cost, gradient over [x; u], Hessian (or None),
        violation.  zd: the duals {(block, knot point): [p]} (None: the state's, or zero), rho_: the penalty."""
        zd = duals if zd is None else zd
        z = x + (u if k < N else [zero] * m)
        J, gz, viol = zero, [zero] * w, zero
        W = [[zero] * w for _ in range(w)] if hess else None
        for j in cfg.at(k):
            bl, G, g, t = cfg.blocks[j], Gm[j], gm[j], cls[j]
            pp = bl["p"]
            val = [dot(G[i], z) - g[i] for i in range(pp)]
            ze = [zd[(j, k)][i] - rho_ * val[i] for i in range(pp)] if (j, k) in zd else [-(rho_ * c) for c in val]
            Jd = Jf = Hs = None
            if bl["kind"] == "eq":
                zp, Jd = ze, [1] * pp
                viol = max([viol] + [abs(c) for c in val])
            elif bl["kind"] == "orth":
                Jd = [int(t[i]) for i in range(pp)]
                flips[0] += sum(int(Jd[i] != (1 if ze[i] <= 0 else 0)) for i in range(pp))
                zp = [ze[i] if Jd[i] else zero for i in range(pp)]
                viol = max([viol] + [abs(val[i]) for i in range(pp) if Jd[i]])
            else:
                nv = pp - 1
                v, s = ze[:nv], ze[nv]
                a = mp.sqrt(dot(v, v))
                region = int(t[0])
                flips[0] += int(region != (0 if a <= -s else (1 if a <= s else 2)))
                if region == 0:                        # ze below its cone: projection 0, the value itself inside: no violation
                    continue
                if region == 1:                        # ze inside: identity; the value is below its cone: its projection is 0
                    zp, Jd = ze, [1] * pp
                    viol = max([viol] + [abs(c) for c in val])
                else:
                    c = half * (1 + s / a)
                    zp = [c * e for e in v] + [c * a]
                    Jf = [[zero] * pp for _ in range(pp)]
                    for i in range(nv):
                        for jj in range(nv):
                            Jf[i][jj] = -half * s / (a * a * a) * v[i] * v[jj] + (c if i == jj else zero)
                        Jf[i][nv] = half * v[i] / a
                        Jf[nv][i] = (-half * s / (a * a) + c / a) * v[i]
                    Jf[nv][nv] = half
                    vv, sv = val[:nv], val[nv]         # the value's own projection: outside as well
                    av = mp.sqrt(dot(vv, vv))
                    cv = half * (1 + sv / av)
                    viol = max([viol] + [abs(cv * e - e) for e in vv] + [abs(cv * av - sv)])
                    if hess:
                        bs, vbv = zp[nv], dot(v, zp[:nv])
                        Hs = [[zero] * pp for _ in range(pp)]
                        for i in range(nv):
                            hi = dot([-v[i] * v[jj] / (a * a) + (1 if i == jj else 0) for jj in range(nv)], zp[:nv])
                            Hs[i][nv] = Hs[nv][i] = hi / (2 * a)
                            for jj in range(i + 1):
                                vij = v[i] * v[jj]
                                H1 = hi * v[jj] * (-s / (a * a * a))
                                H2 = vij * (2 * vbv) / (a * a * a * a) - v[i] * zp[jj] / (a * a)
                                H3 = -vij / (a * a)
                                if i == jj:
                                    H2 -= vbv / (a * a)
                                    H3 += 1
                                Hs[i][jj] = Hs[jj][i] = (H1 + H2 * (s / a) + H3 * (bs / a)) / 2
            J += dot(zp, zp) / (2 * rho_)
            if Jd is not None:
                rows = [i for i in range(pp) if Jd[i]]
                jvp = [zp[i] if Jd[i] else zero for i in range(pp)]
                JG = [G[i] for i in rows]
            else:
                jvp = [dot([Jf[kk][i] for kk in range(pp)], zp) for i in range(pp)]
                cols = [[G[kk][e] for kk in range(pp)] for e in range(w)]
                JG = [[dot(Jf[i], cols[e]) for e in range(w)] for i in range(pp)]
            for e in range(w):
                gz[e] -= dot([G[i][e] for i in range(pp)], jvp)
            if hess:
                ct = [[row[e] for row in JG] for e in range(w)]
                for e in range(w):
                    for f in range(e + 1):
                        W[e][f] += rho_ * dot(ct[e], ct[f])
                if Hs is not None:
                    cols = [[G[kk][e] for kk in range(pp)] for e in range(w)]
                    HG = [[dot(Hs[i], cols[e]) for e in range(w)] for i in range(pp)]
                    hgc = [[row[e] for row in HG] for e in range(w)]
                    for e in range(w):
                        for f in range(e + 1):
                            W[e][f] += rho_ * dot(cols[e], hgc[f])
        if hess:
            for e in range(w):
                for f in range(e):
                    W[f][e] = W[e][f]
        if state is not None:                          # with duals the branch of ze says nothing about the value: its own projection
            viol = max([zero] + [violation(j, constraint(j, k, x, u if k < N else None)) for j in cfg.at(k)])
        return J, gz, W, viol

    # ---- the expansion about a trajectory and the backward sweep (f = 0) ----
    def sweep(xn, un, cls0, zd=None, rh=rho_):
        """lx, lu, K, d, P, p (rows) of the expansion about xn, un with the branches cls0 [blocks, BATCH, N + 1, rows], duals zd, penalty rh."""
        lx, lu, lxx, luu, lux = [], [], [], [], []
        for k in range(N + 1):
            _, gx, gu = stage(k, xn[k], un[k])
            _, gz, W, _ = al(k, xn[k], un[k], cls0[:, b, k], True, zd, rh)
            Q, R, H = cost[k][:3]
            lx.append(add(gx, gz[:n]))
            lxx.append([[Q[i][j] + W[i][j] for j in range(n)] for i in range(n)])
            if k < N:
                lu.append(add(gu, gz[n:]))
                luu.append([[R[i][j] + W[n + i][n + j] for j in range(m)] for i in range(m)])
                lux.append([[H[i][j] + W[n + i][j] for j in range(n)] for i in range(m)])
        mx = mp.matrix
        P, pv, K, d = [None] * (N + 1), [None] * (N + 1), [None] * N, [None] * N
        P[N], pv[N] = mx(lxx[N]), mx(lx[N])
        for k in range(N - 1, -1, -1):
            Ak, Bk = mx(A[k]), mx(B[k])
            AtP, BtP = Ak.T * P[k + 1], Bk.T * P[k + 1]
            Qxx, Quu, Qux = mx(lxx[k]) + AtP * Ak, mx(luu[k]) + BtP * Bk, mx(lux[k]) + BtP * Ak
            Qx, Qu = mx(lx[k]) + Ak.T * pv[k + 1], mx(lu[k]) + Bk.T * pv[k + 1]
            L = mp.matrix(m, m)
            for j in range(m):
                s = Quu[j, j] - mp.fsum(L[j, c] * L[j, c] for c in range(j))
                assert s > 0, ("the exact recursion is indefinite", cfg.name, b, k, j)
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
            K[k], d[k] = solve(Qux, n), -solve(Qu, 1)
            QK, KtQux = Quu * K[k], K[k].T * Qux
            P[k] = Qxx + QK.T * K[k] - KtQux - KtQux.T
            pv[k] = Qx - QK.T * d[k] - K[k].T * Qu + Qux.T * d[k]
        rowsof = lambda X, r, c: [[X[i, j] for j in range(c)] for i in range(r)]
        Kr, Pr = [rowsof(K[k], m, n) for k in range(N)], [rowsof(P[k], n, n) for k in range(N + 1)]
        dr, pr = [[d[k][i] for i in range(m)] for k in range(N)], [[pv[k][i] for i in range(n)] for k in range(N + 1)]
        return lx, lu, Kr, dr, Pr, pr

    fl = lambda rows: np.array([[float(v) for v in r] for r in rows])
    colmajor = lambda mats: np.array([[float(Mx[i][j]) for j in range(len(Mx[0])) for i in range(len(Mx))] for Mx in mats])
    x0v = V(cfg.x0[b])
    if update is not None:                             # ---- the frozen solve: z+, rho+, the second sweep, z++ ----
        un = [V(state["u"][b, k]) for k in range(N)] + [[zero] * m]
        xn = [x0v]
        for k in range(N):
            xn.append(add(add(mv(A[k], xn[k]), mv(B[k], un[k])), aff[k]))
        res, zd, rh = {}, duals, rho_
        for i in (1, 2):
            zd = {(j, k): project(j, [zd[(j, k)][r] - rh * c for r, c in enumerate(constraint(j, k, xn[k], un[k]))], update[i - 1][j, b, k])
                  for (j, k) in zd}
            for j, bl in enumerate(cfg.blocks):
                res["z%d:%s" % (i, bl["name"])] = fl([zd[(j, k)] for k in range(bl["k0"], bl["k1"] + 1)])
            rh = min(rh * F(lsc.PENALTY_SCALING), F(lsc.PENALTY_MAX))
            res["rho%d" % i] = float(rh)
            if i == 1:
                _, _, Kr, dr, Pr, pr = sweep(xn, un, update[1], zd, rh)
                res.update(d=fl(dr), p=fl(pr), K=colmajor(Kr), P=colmajor(Pr))
        return res, flips[0]

    if state is None:
        xn = [V(cfg.x[b, k]) for k in range(N + 1)]
        un = [V(cfg.u[b, k]) for k in range(N)] + [[zero] * m]
    else:
        xn = [V(state["x"][b, k]) for k in range(N + 1)]
        un = [V(state["u"][b, k]) for k in range(N)] + [[zero] * m]
    lx, lu, Kr, dr, Pr, pr = sweep(xn, un, tab[0])
    out = dict(lx=lx, lu=lu, K=Kr, d=dr, P=Pr, p=pr)

    # ---- the merit function ----
    def merit(alpha, ti):
        xc, uc, yc, gxc, guc = [V(cfg.x0[b])], [], [], [], []
        dxa = [zero] * n
        phi = dphi = zero
        worst = zero
        for k in range(N + 1):
            dx = [a - c for a, c in zip(xc[k], xn[k])]
            yc.append(add(mv(Pr[k], dx), pr[k]))
            if k < N:
                Kdx = mv(Kr[k], dx)
                uc.append([un[k][i] + (-Kdx[i] + alpha * dr[k][i]) for i in range(m)])
                xc.append(add(add(mv(A[k], xc[k]), mv(B[k], uc[k])), aff[k]))
            Jc, gx, gu = stage(k, xc[k], uc[k] if k < N else None)
            Ja, gz, _, viol = al(k, xc[k], uc[k] if k < N else None, tab[ti][:, b, k], False)
            phi += Jc + Ja
            worst = max(worst, viol)
            gxc.append(add(gx, gz[:n]))
            dphi += dot(gxc[k], dxa)
            if k < N:
                guc.append(add(gu, gz[n:]))
                Kda = mv(Kr[k], dxa)
                dua = [-Kda[i] + dr[k][i] for i in range(m)]
                dphi += dot(guc[k], dua)
                dxa = add(mv(A[k], dxa), mv(B[k], dua))
        return phi, dphi, xc, uc, yc, gxc, guc, worst

    out["phi0"], out["dphi0"] = merit(zero, 1)[:2]
    out["phi"], out["dphi"], xc, uc, yc, gxc, guc, out["feas"] = merit(F(crc.ALPHAS[b]), 2)
    out["x"], out["u"] = xc, uc
    stat = zero
    for k in range(N):
        ty, tu = mtv(A[k], yc[k + 1]), mtv(B[k], yc[k + 1])
        stat = max([stat] + [abs(gxc[k][i] + ty[i] - yc[k][i]) for i in range(n)] + [abs(guc[k][i] + tu[i]) for i in range(m)])
    out["stat"] = max([stat] + [abs(gxc[N][i] - yc[N][i]) for i in range(n)])

    # ---- rounded once, in the oracle's layouts ----
    fl = lambda rows: np.array([[float(v) for v in r] for r in rows])
    colmajor = lambda mats: np.array([[float(Mx[i][j]) for j in range(len(Mx[0])) for i in range(len(Mx))] for Mx in mats])
    res = {q: fl(out[q]) for q in ("lx", "lu", "d", "p", "x", "u")}
    res["K"], res["P"] = colmajor(out["K"]), colmajor(out["P"])
    for q in lsc.SCALARS:
        res[q] = float(out[q])
    return res, flips[0]


def one(args):
    name, ri, b, digits = args
    cfg = crc.config(name)
    return mp_phases(cfg, b, RHOS[ri], lsc.class_tables(cfg, RHOS[ri]), digits)


def largest_fixture():
    """The size of the largest file under tests/golden that this script does not (re)write: no new fixture may be larger."""
    here = os.path.dirname(os.path.abspath(__file__))
    new = {os.path.basename(lsc.fixture_path(nm)) for nm in crc.HORIZON_CONFIGS}
    return max(os.path.getsize(os.path.join(here, f)) for f in os.listdir(here) if f not in new and os.path.isfile(os.path.join(here, f)))


def make(name, pool):
    cfg = crc.config(name)
    arrays = {"sum": checksum(lsc.inputs(cfg))}
    jobs = [(name, ri, b, digits) for ri in range(len(RHOS)) for digits in (60, 120) for b in range(BATCH)]
    done = dict(zip(jobs, pool.map(one, jobs, chunksize=1)))
    for ri, rho in enumerate(RHOS):
        per, per2 = ([done[(name, ri, b, digits)] for b in range(BATCH)] for digits in (60, 120))
        ref = {q: np.stack([np.asarray(r[0][q], dtype=np.float64) for r in per]) for q in lsc.QUANTITIES}
        ref2 = {q: np.stack([np.asarray(r[0][q], dtype=np.float64) for r in per2]) for q in lsc.QUANTITIES}
        for q in lsc.QUANTITIES:
            if name in crc.CONFIGS:
                assert np.array_equal(ref[q], ref2[q]), ("60 and 120 digits round differently", name, rho, q)
            else:       # (more knot points, more entries: one of them may sit at an exact rounding tie, as in the fixtures of the second half)
                ref[q] = ties_to_even(ref[q], ref2[q], (name, "rho %g" % rho, q))
            arrays["ref_%d_%s" % (ri, q)] = ref[q]
        arrays["tab_%d" % ri] = lsc.class_tables(cfg, rho)
        arrays["flips_%d" % ri] = np.array(sum(r[1] for r in per), dtype=np.int64)
        e = lsc.errors(lsc.oracle_phases(cfg, rho), ref)
        arrays["ecpu_%d" % ri] = np.array([e[q] for q in lsc.QUANTITIES])
        print(name, "rho", rho, "flips", int(arrays["flips_%d" % ri]), " ".join("%s %.1e" % (q, e[q]) for q in lsc.QUANTITIES), flush=True)
    write(lsc.fixture_path(name), arrays)
    if name not in crc.CONFIGS and os.path.getsize(lsc.fixture_path(name)) > largest_fixture():
        # a horizon at which the references of every quantity make the file larger than any other here: the merit phase's alone
        for ri in range(len(RHOS)):
            for q in lsc.QUANTITIES:
                if q not in lsc.MERIT_QUANTITIES:
                    del arrays["ref_%d_%s" % (ri, q)]
                    arrays["ecpu_%d" % ri][lsc.QUANTITIES.index(q)] = np.nan      # (NaN: no reference stored)
        write(lsc.fixture_path(name), arrays)


def write(path, arrays):
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:       # np.savez stamps the time of day into the archive: not reproducible
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), "w") as f:
                np.lib.format.write_array(f, np.asarray(arrays[k]), allow_pickle=False)
    print("%s: %d bytes" % (os.path.relpath(path, ROOT), os.path.getsize(path)), flush=True)


# ---- nonzero duals and the dual update: tests/golden/loop_phases_duals_<config>.npz ------------------------------------------------------
def one_dual(args):
    name, what, b, digits = args
    cfg = crc.config(name)
    d = lsc.dual_inputs(name)
    if what == "s1":
        return mp_phases(cfg, b, d["s1"]["rho"][b], d["tab_s1"], digits, state=d["s1"])
    return mp_phases(cfg, b, lsc.RHO0, None, digits, state=d["s2"], update=(d["tab_u1"], d["tab_u2"]))


def ties_to_even(a, a2, what):
    """The arrays rounded from the 60- and the 120-digit run: identical, except where the exact value lies HALFWAY between two doubles.
    (A cone of two rows has a piecewise linear projection: outside it rho (J G)^T (J G) couples its two variables by rho g / 2, with
    rho = 10 a 56-bit number that is a midpoint one time in four, reached here through a division that is not exact.)  There the two
    runs may give the two neighbours; the one with the even mantissa is taken, as a correctly rounded exact evaluation would."""
    a, a2 = np.array(a, dtype=np.float64), np.array(a2, dtype=np.float64)
    i = a != a2
    if i.any():
        assert np.array_equal(np.nextafter(a[i], a2[i]), a2[i]), ("60 and 120 digits differ by more than a tie", what)
        a[i] = np.where(a[i].view(np.int64) & 1 == 0, a[i], a2[i])
        print("   %s: %d entries at a rounding tie" % ("/".join(what), int(i.sum())), flush=True)
    return a


def make_duals(name, pool):
    cfg = crc.config(name)
    d = lsc.dual_inputs(name)
    arrays = lsc.dual_input_arrays(cfg, d)
    arrays["sum"] = checksum(dict(lsc.inputs(cfg), **arrays))
    jobs = [(name, what, b, digits) for what in ("s1", "up") for digits in (60, 120) for b in range(BATCH)]
    done = dict(zip(jobs, pool.map(one_dual, jobs, chunksize=1)))
    ref = {}
    for what in ("s1", "up"):
        per, per2 = ([done[(name, what, b, digits)] for b in range(BATCH)] for digits in (60, 120))
        for q in per[0][0]:
            a, a2 = (np.stack([np.asarray(r[0][q], dtype=np.float64) for r in rs]) for rs in (per, per2))
            ref[(what, q)] = ties_to_even(a, a2, (name, what, q))
        arrays["flips_" + what] = np.array(sum(r[1] for r in per), dtype=np.int64)
    arrays.update(lsc.dual_reference_arrays(cfg, ref))
    arrays.update(lsc.dual_ecpu(cfg, d, arrays))
    print(name, "flips", int(arrays["flips_s1"]), int(arrays["flips_up"]), " ".join("%s %s" % (k, np.array2string(v, precision=1))
                                                                                      for k, v in arrays.items() if k.startswith("ecpu")), flush=True)
    write(lsc.dual_fixture_path(name), arrays)


if __name__ == "__main__":
    import multiprocessing
    args = sys.argv[1:]
    duals = "--duals" in args
    names = [a for a in args if a != "--duals"] or list(crc.CONFIGS)
    with multiprocessing.Pool(min(14, os.cpu_count() or 1)) as pool:
        for nm in names:
            (make_duals if duals else make)(nm, pool)
