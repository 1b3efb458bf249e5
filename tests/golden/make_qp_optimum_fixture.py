#!/usr/bin/env python
"""Independent optima and feasibility verdicts for the Bezier QP (BezierOpt::setup + optimize), written to
tests/golden/qp_optimum_independent.json.  Nothing here reads oracle/ or the kernel: each problem is assembled by the
numpy restatement of tests/golden/make_qp_fixture.py (`assemble`), then
  * t*  = the optimum of the LP  min t  s.t.  l - t <= Ax <= u + t  (scipy HiGHS): t* > 0 means the QP is infeasible
          (every problem has equality rows, so t* >= 0; feasible cases store 0, their certified x* is the proof);
  * x*  = the optimum of  min 1/2 x'Qx  s.t.  l <= Ax <= u, from a dense primal-dual interior-point method (Mehrotra
          predictor-corrector, below), then an active-set polish: the KKT system of the rows the interior point found
          active (z > s) solved exactly, the multipliers by non-negative least squares with the sign of each side;
  * the certificate of x*: stationarity ||Qx* + A'lam*||_inf <= 1e-9 scale, every active multiplier of the right sign
    (>= 0 on an upper side, <= 0 on a lower side, free on an equality row), complementarity and primal feasibility
    <= 1e-9; the generator refuses to write a case whose certificate fails.
tests/test_qp_optimum_independent.py re-checks every certificate against matrices assembled again from the stored
inputs and holds the CPU oracle's solve to the contract of tests/qp_contract.py; tests/test_qp_optimum_gpu.py holds
the kernel to it.  Every case carries the reason it exists (`why`) and the kernel path it exercises (`path`: the
kernel picks one per agent, sogm_qp.hip header comment).
Run from the repo root:   python tests/golden/make_qp_optimum_fixture.py
"""
import json
import math
import os
import sys

import numpy as np
from scipy.optimize import linprog, minimize, nnls

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_qp_fixture import assemble  # noqa: E402

TAU = 0.3                 # corridor_tau: the time allocation replan() uses
LOOSE = (2.0, 6.0)        # opt_max_vel / opt_max_acc of the planner (config.make_planner_params)
# the other regimes scale the planner's limits by one factor k per problem, found by bisection on t*(k) (t* falls
# as k grows): "tight" = 1.1 x the smallest feasible k (velocity / acceleration rows active), "infeasible" = the
# largest k with t* >= 2e-2, "near" = a k with 1e-4 <= t* <= 5e-4
SLACK_T = 1e-9            # HiGHS t* at or below this on a case with a certified x* is stored as 0

# Sanity bounds of the contract (tests/qp_contract.py): 2 x the worst value the CPU oracle's OSQP restatement gave over
# this fixture at the parity settings (eps 1e-3, max_iter 4000, adaptive rho every 25, no polish), measured with
# `pytest -s tests/test_qp_optimum_independent.py -k oracle_meets` (it prints both worst values).  They are calibrated,
# not derived: OSQP at eps 1e-3 may legitimately stop decimetres from x* when velocity rows are active.
MEASURED = {"dx": 0.347, "df_rel": 0.170}   # both from gen_16x6_tight: status 1 after 325 iterations, 35 cm from x*
SANITY = {k: 2.0 * v for k, v in MEASURED.items()}


# ---------------------------------------------------------------- corridors
def box_chain(M, nf, rng, tau_len=TAU, shift=0.0):
    """M overlapping boxes along +x (six faces each) plus nf - 6 redundant tilted faces per box that do not cut it: a
    real row of the QP that is never active.  Returns a list of M arrays [nf][4] (h . x + h3 <= 0 inside)."""
    polys = []
    for i in range(M):
        lo = np.array([i * tau_len - 0.5 + shift, -0.6, 0.4])
        hi = np.array([(i + 1) * tau_len + 0.5 + shift, 0.6, 1.6])
        polys.append(box(lo, hi, nf, rng))
    return polys


def box(lo, hi, nf=6, rng=None):
    H = []
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1.0
        H.append(np.concatenate([e, [-hi[k]]]))
        H.append(np.concatenate([-e, [lo[k]]]))
    c = 0.5 * (lo + hi)
    while len(H) < nf:
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        sup = np.sum(np.abs(n) * 0.5 * (hi - lo)) + rng.uniform(0.05, 0.5)
        H.append(np.concatenate([n, [-(n @ c + sup)]]))
    return np.round(np.array(H), 12)


def chain_ends(M, rng):
    start = np.zeros((3, 3))
    start[0] = [0.0, rng.uniform(-0.2, 0.2), 1.0 + rng.uniform(-0.2, 0.2)]
    start[1] = [rng.uniform(0.0, 0.8), 0.0, 0.0]
    end = np.zeros((3, 3))
    end[0] = [M * TAU, rng.uniform(-0.2, 0.2), 1.0]
    return np.round(start, 12), np.round(end, 12)


# ---------------------------------------------------------------- the independent solves
def rows_of(A, lb, ub):
    l = np.array([-np.inf if v is None else float(v) for v in lb])
    u = np.asarray(ub, float)
    eq = np.isfinite(l) & (l == u)
    return l, u, eq


def lp_t_star(A, lb, ub):
    """min t s.t. Ax - t <= u, -Ax - t <= -l (finite l): HiGHS"""
    l, u, _ = rows_of(A, lb, ub)
    m, n = A.shape
    fin = np.isfinite(l)
    G = np.vstack([np.hstack([A, -np.ones((m, 1))]), np.hstack([-A[fin], -np.ones((fin.sum(), 1))])])
    h = np.concatenate([u, -l[fin]])
    c = np.zeros(n + 1)
    c[-1] = 1.0
    r = linprog(c, A_ub=G, b_ub=h, bounds=[(None, None)] * (n + 1), method="highs",
                options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})
    assert r.status == 0, r.message
    return float(r.x[-1])


def ipm(Q, A, lb, ub, iters=80):
    """dense Mehrotra predictor-corrector on  min 1/2 x'Qx  s.t.  Ex = b, Gx <= h  (G: upper sides, then the finite
    lower sides negated).  Returns x, the inequality slacks s and multipliers z, and the row of A behind each
    inequality with its side (+1 upper, -1 lower)."""
    l, u, eq = rows_of(A, lb, ub)
    ineq = np.nonzero(~eq)[0]
    low = ineq[np.isfinite(l[ineq])]
    E, b = A[eq], u[eq]
    G = np.vstack([A[ineq], -A[low]])
    h = np.concatenate([u[ineq], -l[low]])
    src = np.concatenate([ineq, low])
    side = np.concatenate([np.ones(len(ineq)), -np.ones(len(low))])
    n, me, mi = Q.shape[0], E.shape[0], G.shape[0]
    x, y = np.zeros(n), np.zeros(me)
    s = np.maximum(h - G @ x, 1.0)
    z = np.ones(mi)
    reg = 1e-11
    for _ in range(iters):
        rd = Q @ x + E.T @ y + G.T @ z
        re = E @ x - b
        ri = G @ x + s - h
        mu = s @ z / mi
        if max(np.abs(rd).max(), np.abs(re).max(), np.abs(ri).max()) < 1e-12 and mu < 1e-14:
            break
        W = z / s
        K = np.block([[Q + G.T @ (W[:, None] * G) + reg * np.eye(n), E.T], [E, -reg * np.eye(me)]])

        def solve(rc):
            rhs = np.concatenate([-rd - G.T @ (W * ri - rc / s), -re])
            d = np.linalg.solve(K, rhs)
            dx, dy = d[:n], d[n:]
            dz = W * (G @ dx + ri) - rc / s
            ds = (-rc - s * dz) / z
            return dx, dy, dz, ds

        def step(d, v):
            neg = d < 0
            return min(1.0, (-v[neg] / d[neg]).min()) if neg.any() else 1.0

        dx, dy, dz, ds = solve(s * z)
        a = min(step(ds, s), step(dz, z))
        mu_aff = (s + a * ds) @ (z + a * dz) / mi
        sigma = (mu_aff / mu) ** 3
        dx, dy, dz, ds = solve(s * z + ds * dz - sigma * mu)
        a = 0.99 * min(step(ds, s), step(dz, z))
        x, y, z, s = x + a * dx, y + a * dy, z + a * dz, s + a * ds
    return x, s, z, src, side


def optimum(Q, A, lb, ub):
    """x*, the active rows with their multipliers (convention Q x* + A' lam = 0: lam >= 0 on an upper side, <= 0 on a
    lower side) and the certificate.  The interior point's active set is read first as z > s; where the feasible set
    has no interior (a start on a face with zero velocity and acceleration pins three control points to that face) the
    interior point stalls with s and z both tiny, and the active set is then read as the rows of small slack."""
    l, u, eq = rows_of(A, lb, ub)
    x0, s, z, src, side = ipm(Q, A, lb, ub)
    tries = [z > s] + [s < thr for thr in (1e-5, 1e-7, 1e-9)]
    for i in range(len(tries) + 3):
        if i == len(tries):
            # the interior point stalled: SLSQP from its point, the active set read off SLSQP's slacks
            G = np.vstack([A[src[side > 0]], -A[src[side < 0]]])
            h = np.concatenate([u[src[side > 0]], -l[src[side < 0]]])
            E, b = A[eq], u[eq]
            r = minimize(lambda v: 0.5 * v @ Q @ v, x0, jac=lambda v: Q @ v, method="SLSQP",
                         constraints=[{"type": "eq", "fun": lambda v: E @ v - b, "jac": lambda v: E},
                                      {"type": "ineq", "fun": lambda v: h - G @ v, "jac": lambda v: -G}],
                         options={"ftol": 1e-15, "maxiter": 2000})
            slack = h - G @ r.x
            order = np.concatenate([np.nonzero(side > 0)[0], np.nonzero(side < 0)[0]])
            s = np.empty_like(slack)
            s[order] = slack
            tries += [s < thr for thr in (1e-6, 1e-8, 1e-10)]
        act = tries[i]
        rows = np.concatenate([np.nonzero(eq)[0], src[act]])
        sgn = np.concatenate([np.zeros(eq.sum()), side[act]])
        tgt = np.where(sgn >= 0, u[rows], l[rows])
        # polish: the equality-constrained QP of the active rows, solved exactly (least squares: duplicated faces and
        # M = 1's 18 end rows on 15 unknowns make the active rows dependent)
        n, k = Q.shape[0], len(rows)
        Aa = A[rows]
        K = np.block([[Q, Aa.T], [Aa, np.zeros((k, k))]])
        x = np.linalg.lstsq(K, np.concatenate([np.zeros(n), tgt]), rcond=1e-14)[0][:n]
        # multipliers: non-negative least squares on the stationarity, every side's sign imposed (equality rows free)
        cols = [Aa.T[:, sgn == 0], -Aa.T[:, sgn == 0], Aa.T[:, sgn > 0], -Aa.T[:, sgn < 0]]
        w = nnls(np.hstack(cols), -Q @ x, maxiter=50 * k)[0]
        ne, npos = int((sgn == 0).sum()), int((sgn > 0).sum())
        lam = np.zeros(k)
        lam[sgn == 0] = w[:ne] - w[ne:2 * ne]
        lam[sgn > 0] = w[2 * ne:2 * ne + npos]
        lam[sgn < 0] = -w[2 * ne + npos:]
        cert = certificate(Q, A, lb, ub, x, rows, lam, sgn, tgt)
        if certified(cert):
            break
    return x, rows, lam, cert


def certificate(Q, A, lb, ub, x, rows, lam, sgn, tgt):
    l, u, _ = rows_of(A, lb, ub)
    Ax = A @ x
    r = Q @ x + A[rows].T @ lam
    scale = max(1.0, np.abs(Q @ x).max(), (np.abs(A[rows]) * np.abs(lam)[:, None]).max(initial=0.0))
    viol = np.maximum(np.maximum(Ax - u, l - Ax), 0.0).max()
    comp = (np.abs(lam) * np.abs(Ax[rows] - tgt)).max(initial=0.0)
    wrong_sign = max(float(np.maximum(-lam[sgn > 0], 0).max(initial=0.0)),
                     float(np.maximum(lam[sgn < 0], 0).max(initial=0.0)))
    return {"stationarity": float(np.abs(r).max()), "scale": float(scale), "primal": float(viol),
            "complementarity": float(comp), "wrong_sign": wrong_sign, "nAx": float(np.abs(Ax).max())}


def certified(c):
    return (c["stationarity"] <= 1e-9 * c["scale"] and c["primal"] <= 1e-9 * max(1.0, c["nAx"])
            and c["complementarity"] <= 1e-9 * c["scale"] and c["wrong_sign"] == 0.0)


# ---------------------------------------------------------------- the cases
def cases():
    """(name, why, path, start 3x3, end 3x3, t [M], polys [M] of [F][4], vmax, amax)"""
    out = []
    paths = [("reg_3x6", 3, 6, "register-resident iteration (M <= 8), the common small case"),
             ("reg_8x6", 8, 6, "register-resident iteration at its largest M"),
             ("reg_cold_8x25", 8, 25, "register-resident iteration with the cold row data in HBM scratch (S = 1000)"),
             ("reg_few_5x40", 5, 40, "few pieces with many faces (S = 1000)"),
             ("gen_lds_12x6", 12, 6, "general path (M > 8: no block factor), rows in LDS"),
             ("gen_hbm_8x30", 8, 30, "general path, row storage in HBM scratch (S = 1200)"),
             ("gen_16x6", 16, 6, "the most pieces the ABI takes (n = 240: the set-up's column quads take two trips)")]
    for name, M, nf, pwhy in paths:
        rng = np.random.default_rng(7000 + 100 * M + nf)
        polys = box_chain(M, nf, rng)
        start, end = chain_ends(M, rng)
        t = [TAU] * M
        out.append((f"{name}_loose", f"{pwhy}; the planner's limits: only safety rows can be active", name,
                    start, end, t, polys, *LOOSE))
        out.append((f"{name}_tight", f"{pwhy}; tight limits: velocity / acceleration rows active (lam* != 0 on box rows)",
                    name, start, end, t, polys, *limits(start, end, t, polys, "tight")))
        out.append((f"{name}_infeasible", f"{pwhy}; limits no trajectory meets (t* >= 2e-2)", name,
                    start, end, t, polys, *limits(start, end, t, polys, "infeasible")))
        # the same corridor with a goal 0.3 m beyond the last box: infeasible by geometry at the planner's limits
        bad = end.copy()
        bad[0, 2] = 1.6 + 0.3
        out.append((f"{name}_goal_outside", f"{pwhy}; end position 0.3 m above the last box: infeasible at the "
                    "planner's limits", name, start, bad, t, polys, *LOOSE))
    # near the boundary: 0 < t* < 1e-3 (status 2, 3, -3 and -2 all legal)
    for name, M, nf in (("reg_3x6", 3, 6), ("reg_8x6", 8, 6), ("gen_lds_12x6", 12, 6)):
        rng = np.random.default_rng(7000 + 100 * M + nf)
        polys = box_chain(M, nf, rng)
        start, end = chain_ends(M, rng)
        out.append((f"{name}_near_boundary", "0 < t* < 1e-3: infeasible by less than the solver's tolerance, so "
                    "solved inaccurate, (inaccurately) infeasible and max-iter are all legal outcomes", name,
                    start, end, [TAU] * M, polys, *limits(start, end, [TAU] * M, polys, "near")))
    # the reference's own 3-cube fixture (test_bezier_opt.cpp:57-99) and variants: non-uniform times, final acceleration
    G = json.load(open(os.path.join(HERE, "bezier_opt_fixture.json")))["three"]
    cubes = [np.array(c, float) for c in G["cubes"]]
    st, en, tv = np.array(G["start"], float), np.array(G["end"], float), np.array(G["t"], float)
    e_acc = en.copy()
    e_acc[2] = [0.3, -0.2, 0.1]
    out.append(("cubes_reference", "the reference's own 3-cube test problem, its time vector and limits 3 / 3",
                "reg_3x6", st, en, tv.tolist(), cubes, 3.0, 3.0))
    out.append(("cubes_nonuniform", "3 cubes, non-uniform time allocation [1.5, 3, 2.5]", "reg_3x6", st, en,
                [1.5, 3.0, 2.5], cubes, 3.0, 3.0))
    out.append(("cubes_end_acc", "3 cubes, non-zero final acceleration (end rows of the acceleration block)",
                "reg_3x6", st, e_acc, tv.tolist(), cubes, 3.0, 3.0))
    out.append(("cubes_fast_end_acc", "3 cubes, times x 0.8, final acceleration, limits 4 / 5", "reg_3x6", st,
                e_acc, (tv * 0.8).tolist(), cubes, 4.0, 5.0))
    out.append(("cubes_halved", "3 cubes with the times halved: infeasible at limits 3 / 3", "reg_3x6", st, en,
                (tv * 0.5).tolist(), cubes, 3.0, 3.0))
    # M = 1: 18 boundary equalities on 15 unknowns
    rng = np.random.default_rng(7101)
    P = np.array([[0.0, 0.0, 1.0], [0.1, 0.05, 1.02], [0.2, 0.0, 1.05], [0.3, -0.05, 1.0], [0.4, 0.0, 0.98]])
    T1 = 0.5
    bern = lambda d: np.diff(P, n=d, axis=0) * (math.factorial(4) / math.factorial(4 - d)) / T1 ** d if d else P
    s1 = np.stack([bern(d)[0] for d in range(3)])
    e1 = np.stack([bern(d)[-1] for d in range(3)])
    one = [box(np.array([-0.5, -0.6, 0.4]), np.array([0.9, 0.6, 1.6]))]
    out.append(("single_consistent", "M = 1: the end state of a real quartic piece, so the 18 equalities on 15 "
                "unknowns are consistent (t* = 0) and x* is that piece", "reg_1x6", s1, e1, [T1], one, 3.0, 5.0))
    e_bad = e1.copy()
    e_bad[2] += [0.5, 0.0, 0.0]
    out.append(("single_inconsistent", "M = 1 with an end acceleration no quartic piece reaches: the equalities "
                "alone are infeasible", "reg_1x6", s1, e_bad, [T1], one, 3.0, 5.0))
    polys2 = box_chain(2, 6, rng)
    s2, e2 = chain_ends(2, rng)
    out.append(("two_pieces", "M = 2: one junction", "reg_2x6", s2, e2, [0.5, 0.5], polys2, *LOOSE))
    # degenerate geometry
    rng = np.random.default_rng(7201)
    p3 = box_chain(3, 6, rng)
    s3, e3 = chain_ends(3, rng)
    roomy = (3.0, 9.0)           # 1.5 x the planner's limits: this corridor needs them (t* = 9e-3 at 2 / 6)
    out.append(("duplicated_faces", "every face twice: dependent active rows, multipliers not unique", "reg_3x6",
                s3, e3, [TAU] * 3, [np.vstack([p, p]) for p in p3], *limits(s3, e3, [TAU] * 3, p3, "tight")))
    touch = [box(np.array([-0.5, -0.6, 0.4]), np.array([0.45, 0.6, 1.6])),
             box(np.array([0.45, -0.6, 0.4]), np.array([1.4, 0.6, 1.6]))]
    ts, te = np.zeros((3, 3)), np.zeros((3, 3))
    ts[0], ts[1] = [0.0, 0.1, 1.0], [0.5, 0.0, 0.0]
    te[0] = [0.9, -0.1, 1.0]
    out.append(("touching_boxes", "two boxes that only share the plane x = 0.45: a zero-width junction (t* = 0), "
                "the junction point pinned to that plane", "reg_2x6", ts, te, [0.8, 0.8], touch, *LOOSE))
    # the first box's face -x <= 0 moved onto the start (x = 0), then 5e-4 beyond it
    on = [p.copy() for p in p3]
    on[0][1, 3] = s3[0, 0]
    out.append(("start_on_face", "start position on the first box's face x = 0 (an active safety row at the start, "
                "t* = 0)", "reg_3x6", s3, e3, [TAU] * 3, on, *roomy))
    off = [p.copy() for p in p3]
    off[0][1, 3] = s3[0, 0] + 5e-4
    out.append(("start_outside", "start position 5e-4 outside its first polytope: infeasible by less than eps",
                "reg_3x6", s3, e3, [TAU] * 3, off, *roomy))
    # row-scaling invariance: the same feasible problem, every face row (h, h3) multiplied by a factor in [1e-3, 1e3]
    rng = np.random.default_rng(7301)
    base = [c for c in out if c[0] == "reg_3x6_tight"][0]
    sc_polys = [np.round(p * 10.0 ** rng.uniform(-3, 3, (len(p), 1)), 12) for p in base[6]]
    out.append(("reg_3x6_tight_rows_scaled", "reg_3x6_tight with each face row scaled by 10^U(-3, 3): the same x* "
                "(Ruiz scaling and its unscale tested directly)", "reg_3x6", base[3], base[4], base[5], sc_polys,
                base[7], base[8]))
    return out


def limits(start, end, t, polys, regime):
    tk = lambda k: solve_case(start, end, t, polys, LOOSE[0] * k, LOOSE[1] * k)[4]
    lo, hi = 0.02, 3.0           # t*(lo) > 0 = t*(hi)
    assert tk(hi) <= SLACK_T and tk(lo) > 2e-2
    want = {"tight": (0.0, SLACK_T), "near": (1e-4, 5e-4), "infeasible": (2e-2, 4e-2)}[regime]
    for _ in range(60):
        k = 0.5 * (lo + hi)
        v = tk(k)
        if regime == "tight":
            if hi - lo < 1e-4:
                k = 1.1 * hi
                break
            lo, hi = (k, hi) if v > SLACK_T else (lo, k)
        elif want[0] <= v <= want[1]:
            break
        else:
            lo, hi = (k, hi) if v > want[1] else (lo, k)
    return round(LOOSE[0] * k, 6), round(LOOSE[1] * k, 6)


def solve_case(start, end, t, polys, vmax, amax):
    Q, A, lb, ub = assemble(start, end, t, polys, vmax, amax)
    t_star = lp_t_star(A, lb, ub)
    return Q, A, lb, ub, t_star


def main():
    recs = []
    for name, why, path, start, end, t, polys, vmax, amax in cases():
        Q, A, lb, ub, t_lp = solve_case(start, end, t, polys, vmax, amax)
        rec = {"name": name, "why": why, "path": path, "M": len(t),
               "faces": [len(p) for p in polys], "start": np.asarray(start).tolist(), "end": np.asarray(end).tolist(),
               "t": [float(v) for v in t], "polys": [np.asarray(p).tolist() for p in polys],
               "vmax": float(vmax), "amax": float(amax), "t_star_lp": t_lp}
        if t_lp > SLACK_T:
            rec.update(feasible=False, t_star=t_lp)
        else:
            x, rows, lam, cert = optimum(Q, A, lb, ub)
            assert certified(cert), (name, cert)
            keep = lam != 0
            box_rows = (rows >= 9 * (len(t) + 1)) & (rows < 30 * len(t) + 9)
            rec.update(feasible=True, t_star=0.0, x_star=x.tolist(), f_star=0.5 * float(x @ Q @ x),
                       active=[[int(r), float(v)] for r, v in zip(rows[keep], lam[keep])],
                       active_box_rows=int((keep & box_rows).sum()), kkt=cert)
        recs.append(rec)
        print(f"{name:28s} M={len(t):2d} faces={sum(rec['faces']):4d} t*={rec['t_star']:.3e} "
              + (f"f*={rec['f_star']:.6e} active={len(rec['active'])} box={rec['active_box_rows']} "
                 f"stat={rec['kkt']['stationarity']:.1e}" if rec["feasible"] else "infeasible"))
    out = {"what": "Bezier QP optima and LP feasibility verdicts from an independent numpy assembly + HiGHS + interior "
                   "point with a KKT certificate (tests/golden/make_qp_optimum_fixture.py); active = [[row, lam]] with "
                   "Q x* + A' lam = 0",
           "eps_abs": 1e-3, "eps_rel": 1e-3, "sanity": SANITY, "sanity_measured": MEASURED, "cases": recs}
    path = os.path.join(HERE, "qp_optimum_independent.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print(path, len(recs), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
