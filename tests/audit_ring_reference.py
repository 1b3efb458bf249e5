"""The body-box rule of include/sogm_abi.h ("ring obstacles") and the flight audit with SOGM_AUDIT_RINGS restated in
numpy, written from the header's text alone (fp64, the header's order of operations), vectorised over poses.  Everything
that is not a ring — record selection, samples, agents, cylinders, goal, path — is tests/swarm_audit_reference.py's: its
audit() runs on the records that are not rings, and the two results are put together by the header's rules (minima by
value, then the earliest sample, then the lowest index; events ordered by (sample, agent, kind, other)).
Test infrastructure; not collected by pytest."""
import numpy as np

import swarm_audit_reference as aref
from depth_ring_reference import frame


def mid(a, b):
    sx, sy = a[0] + b[0], a[1] + b[1]
    nn = np.sqrt(sx * sx + sy * sy)
    return np.array([sx / nn, sy / nn])


def table():
    """the 64 unit vectors by arc halving, in angular order"""
    tab = np.zeros((64, 2))
    tab[0], tab[16], tab[32], tab[48] = (1, 0), (0, 1), (-1, 0), (0, -1)
    for step in (8, 4, 2, 1):
        for i in range(step, 64, 2 * step):
            tab[i] = mid(tab[(i - step) % 64], tab[(i + step) % 64])
    return tab


TABLE = table()


def point_gap(c, R, e1, e2, lo, hi, u):
    """g(u) for N poses: c, lo, hi [N, 3]; u [N, 2] or [2]"""
    u = np.broadcast_to(u, (len(c), 2))
    dd = []
    for i in range(3):
        P = c[:, i] + R * (u[:, 0] * e1[i] + u[:, 1] * e2[i])
        q = np.where(P < lo[:, i], lo[:, i], np.where(P > hi[:, i], hi[:, i], P))
        dd.append(P - q)
    return np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])


def box_gap(c, R, rho, e1, e2, a, body, steps=12):
    """gap [N] of the ring with centres c [N, 3] against boxes of size `body` centred at a [N, 3]"""
    c, a = np.asarray(c, np.float64).reshape(-1, 3), np.asarray(a, np.float64).reshape(-1, 3)
    hb = np.array([0.5 * body[0], 0.5 * body[1], 0.5 * body[2]])
    lo, hi = a - hb, a + hb
    g_all = np.stack([point_gap(c, R, e1, e2, lo, hi, TABLE[k]) for k in range(64)], axis=1)
    best = np.argmin(g_all, axis=1)                       # the first of equal minima: the lowest index
    rows = np.arange(len(c))
    gm = g_all[rows, best]
    ul, um, ur = TABLE[(best + 63) % 64], TABLE[best], TABLE[(best + 1) % 64]
    for _ in range(steps):
        sl, sr = ul + um, um + ur
        ml = sl / np.sqrt(sl[:, 0] * sl[:, 0] + sl[:, 1] * sl[:, 1])[:, None]
        mr = sr / np.sqrt(sr[:, 0] * sr[:, 0] + sr[:, 1] * sr[:, 1])[:, None]
        gl, gr = point_gap(c, R, e1, e2, lo, hi, ml), point_gap(c, R, e1, e2, lo, hi, mr)
        left = (gl < gm) & (gl <= gr)
        right = ~left & (gr < gm)
        keep = ~left & ~right
        L, M, Rr = left[:, None], right[:, None], keep[:, None]
        ul, um, ur, gm = (np.where(L, ul, np.where(M, um, ml)), np.where(L, ml, np.where(M, mr, um)),
                          np.where(L, um, np.where(M, ur, mr)), np.where(left, gl, np.where(right, gr, gm)))
        del Rr
    return gm - rho


def dense_gap(c, R, rho, e1, e2, a, body, n=65536):
    """one pose: the gap from n sampled circle points (cos, sin): an upper bound of the true gap, at most pi R / n above it"""
    th = np.arange(n) * (2.0 * np.pi / n)
    P = np.asarray(c)[None, :] + R * (np.cos(th)[:, None] * e1[None, :] + np.sin(th)[:, None] * e2[None, :])
    hb = 0.5 * np.asarray(body, np.float64)
    q = np.clip(P, np.asarray(a) - hb, np.asarray(a) + hb)
    return float(np.sqrt(((P - q) ** 2).sum(axis=1)).min() - rho)


def new_state(n_local):
    return {"cyl": aref.new_acc(n_local), "ring_gap": np.full(n_local, np.inf), "ring_time": np.full(n_local, -1.0),
            "ring_idx": np.full(n_local, -1, np.int64), "ring_first": np.full(n_local, -1.0),
            "obstacle_samples": np.zeros(n_local, np.int64)}


def audit(tables, prev_table, fallback, goals, rows12, t0, first_tick, period, agent0, n_local, t_obstacles=0.0,
          body=aref.BODY, sample_dt=0.01, goal_tolerance=1.0, state=None):
    """One call of the audit over records (n, 12) {type, x, y, z, w, h, vx, vy, qw, qx, qy, qz} with SOGM_AUDIT_RINGS.
    Returns (acc, events [(t, agent, other, kind)], margins, state) or None where the header refuses the records."""
    rows12 = np.asarray(rows12, np.float64).reshape(-1, 12)
    frames = {}
    for i, row in enumerate(rows12):
        if row[0] == 2:
            frames[i] = frame(row)
            if frames[i] is None:
                return None
        elif row[0] != 3:
            return None
    state = new_state(n_local) if state is None else {k: (v.copy() if k != "cyl" else {q: w.copy() for q, w in v.items()})
                                                       for k, v in state.items()}
    cyl_idx = np.nonzero(rows12[:, 0] == 3)[0]
    state["cyl_idx"] = cyl_idx                             # the cylinder reading numbers the cylinders among themselves
    cyl7 = rows12[cyl_idx][:, [1, 2, 3, 4, 5, 6, 7]]
    acc_c, ev_c, margins = aref.audit(tables, prev_table, fallback, goals, cyl7, t0, first_tick, period, agent0, n_local,
                                      t_obstacles=t_obstacles, body=body, sample_dt=sample_dt,
                                      goal_tolerance=goal_tolerance, acc=state["cyl"])
    state["cyl"] = acc_c
    events = [(t, me, int(cyl_idx[o]) if kind == 1 else o, kind) for (t, me, o, kind) in ev_c]
    pos, ts = aref.positions(tables, prev_table, fallback, t0, first_tick, period, sample_dt)
    ts = np.array(ts)
    ns = len(ts)
    ring_hit = np.zeros((ns, n_local), bool)
    for i, (c0, R, rho, e1, e2, _) in sorted(frames.items()):
        dt = ts - t_obstacles
        c = np.stack([c0[0] + rows12[i, 6] * dt, c0[1] + rows12[i, 7] * dt, np.full(ns, c0[2])], axis=1)
        for j in range(n_local):
            gap = box_gap(c, R, rho, e1, e2, pos[:, agent0 + j], body)
            margins.append(np.abs(gap))
            for s in np.nonzero(gap < 0)[0]:
                events.append((float(ts[s]), agent0 + j, i, 1))
            ring_hit[:, j] |= gap < 0
            s = int(np.argmin(gap))                        # the earliest sample of equal minima
            # records come in index order: an equal gap at the same sample stays with the lower index
            if gap[s] < state["ring_gap"][j] or (gap[s] == state["ring_gap"][j] and ts[s] < state["ring_time"][j]):
                state["ring_gap"][j], state["ring_time"][j], state["ring_idx"][j] = gap[s], ts[s], i
    order = {float(t): s for s, t in enumerate(ts)}
    events.sort(key=lambda e: (order[float(e[0])], e[1], e[3], e[2]))
    cyl_hit = np.zeros((ns, n_local), bool)
    any_hit = np.zeros((ns, n_local), bool)
    for (t, me, _, kind) in ev_c:
        any_hit[order[float(t)], me - agent0] = True
        if kind == 1:
            cyl_hit[order[float(t)], me - agent0] = True
    state["obstacle_samples"] = state["obstacle_samples"] + (cyl_hit | ring_hit).sum(axis=0)
    for j in range(n_local):
        if state["ring_first"][j] < 0 and ring_hit[:, j].any():
            state["ring_first"][j] = ts[int(np.argmax(ring_hit[:, j]))]
    return merged(state), events, margins, state


def merged(state):
    """the accumulator the header describes, from the cylinder reading's and the rings' parts"""
    acc = {k: v.copy() for k, v in state["cyl"].items()}
    seen = acc["min_gap_obstacle"] >= 0
    acc["min_gap_obstacle"][seen] = state["cyl_idx"][acc["min_gap_obstacle"][seen]]
    for j in range(len(acc["min_gap"])):
        g, t, i = state["ring_gap"][j], state["ring_time"][j], state["ring_idx"][j]
        cg, ct, ci = acc["min_gap"][j], acc["min_gap_time"][j], acc["min_gap_obstacle"][j]
        if g < cg or (g == cg and np.isfinite(g) and (t, i) < (ct, ci)):
            acc["min_gap"][j], acc["min_gap_time"][j], acc["min_gap_obstacle"][j] = g, t, i
        f, cf = state["ring_first"][j], acc["first_collision_time"][j]
        if f >= 0 and (cf < 0 or f < cf):
            acc["first_collision_time"][j] = f
    acc["obstacle_samples"] = state["obstacle_samples"].copy()
    return acc
