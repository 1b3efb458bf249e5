#!/usr/bin/env python
"""An INDEPENDENT second restatement of the corridor RULES around FIRI — written straight from the reference's text in
numpy WITHOUT reading oracle/ or csrc/sogm_corridor.hip — whose results on hand-built cases are committed as
tests/golden/corridor_rules_independent.json; tests/test_corridor_rules_independent.py holds the C++ oracle
(`orc_corridor_rules`) and the HIP kernel (`sogm_corridor_rules_batched`) to them.  It does not pin either to the
REFERENCE (Eigen and ROS absent), it makes separately written readings agree.

Restated, block by block:  plan_manager/src/baseline.cpp (BaselinePlanner, "real") and baseline_fake.cpp
(FakeBaselinePlanner, "fake")
  getInitCorridor                      baseline.cpp:127-141
  checkGoalReachability                baseline.cpp:143-182  (writes the goal back through its reference argument)
  checkCorridorIntersect / Validity    baseline.cpp:184-204
  ShrinkCorridor(corridor, path)       baseline.cpp:215-228 (both tests commented out), baseline_fake.cpp:211-223
  replan, from the way-point copy to "Trajectory Optimization", with the polytope that firi::firi would have written
  taken from the case instead      baseline.cpp:298-403, baseline_fake.cpp:305-414
The LPs go through the independent sdlp restatement of make_lp_fixture.py (imported, not written a third time) in the
library's insertion order.  Where the text leaves a summation order to Eigen (n.dot(path), n.norm(), corridor * g) it is
written left to right.

Not in the text, taken over as documented limits of the library: at most 16 polytopes per route
(`pieces_capacity`), a per-segment state "capacity exceeded" that ends the chain like an invalid polytope
(`corridor_capacity`), and 0 polytopes where the text would index an empty vector (a route of 0 or 1 way-points in the
fake planner, a first segment that is invalid: `hPolys.size() - 1` underflows there).

What the text makes of the goal scan, for the record: the real planner's first checkGoalReachability call moves an
unreachable goal to the middle of the LAST polytope, so the scan that follows finds it reachable in its first
iteration, keeps every polytope and takes the goal from the route again — a truncation by the goal scan happens in
the fake planner only.  The branch lists of the two variants differ accordingly.

The generator asserts that no tolerance decides a verdict: every tested polytope holds a ball of radius >= 1e-3 or is
infeasible by >= 1e-3 (Chebyshev centre, scipy HiGHS), every cosine of a shrink test is >= 1e-6 from 0.8 (zero-length
paths aside), every reachability maximum is >= 1e-6 from 0, and every goal LP has one optimal vertex (perturbed
objectives find the same one).  A case that breaks one of them is an error here, never a skip.
Run from the repo root:   python tests/golden/make_corridor_rules_fixture.py
"""
import json
import math
import os
import sys

import numpy as np
from scipy.optimize import linprog as highs

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_lp_fixture as sdlp  # noqa: E402  (the independent sdlp restatement)

MAX_PIECES = 16
MAX_FACES = 12
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the restatement
def lp3(c, poly):
    A = [[r[0], r[1], r[2]] for r in poly]
    b = [-r[3] for r in poly]
    v, x, _ = sdlp.linprog(list(c), A, b, sdlp.library_permutation(len(b)))
    return v, x


def get_init_corridor(higher, lower):
    c = np.zeros((6, 4))
    for k in range(3):
        c[k, k] = 1.0
        c[k + 3, k] = -1.0
        c[k, 3] = -higher[k]
        c[k + 3, 3] = lower[k]
    return c


def check_corridor_validity(poly):
    v, _ = lp3([0.0, 0.0, 0.0], poly)
    return not math.isinf(v)


def check_goal_reachability(poly, start, goal, log):
    """returns (reachable, goal): the text writes the projected goal back through `goal_pos`"""
    if len(poly) <= 0:
        return True, goal
    rst = [(r[0] * goal[0] + r[1] * goal[1]) + r[2] * goal[2] + r[3] * 1.0 for r in poly]
    mx = max(rst)
    log["reach_max"].append(mx)
    if mx <= 0:
        return True, goal
    c = [-goal[k] + start[k] for k in range(3)]
    _, gmax = lp3(c, poly)
    c2 = [goal[k] - start[k] for k in range(3)]
    _, gmin = lp3(c2, poly)
    log["goal_lps"].append((c, [list(r) for r in poly], gmax))
    log["goal_lps"].append((c2, [list(r) for r in poly], gmin))
    return False, [0.5 * (gmax[k] + gmin[k]) for k in range(3)]


def shrink_corridor(fake, poly, path, shrink_size, log):
    out = [list(r) for r in poly]
    for r in out:
        A, B, C = r[0], r[1], r[2]
        if fake:
            nn = math.sqrt(A * A + B * B + C * C)
            pn = math.sqrt(path[0] * path[0] + path[1] * path[1] + path[2] * path[2])
            with np.errstate(all="ignore"):
                c1 = float(np.float64((A * path[0] + B * path[1]) + C * path[2]) / np.float64(nn) / np.float64(pn))
            log["cos"].append((c1, pn == 0.0))
            if c1 > 0.8:
                continue
            c2 = abs(C) / nn
            log["cos"].append((c2, False))
            if c2 > 0.8:
                continue
        r[3] += math.sqrt(A * A + B * B + C * C) * shrink_size
    return out


def corridor_rules(case):
    """the part of replan() between the way-point copy and "Trajectory Optimization"; returns the fixture's expected values"""
    fake, init_range, shrink = case["fake"], case["init_range"], case["shrink_size"]
    route_vel = case["route"]
    start = case["start_pva"][:3]
    log = {"cos": [], "reach_max": [], "goal_lps": [], "tested": []}
    trace = []
    exp = {"box": [], "shrunk": [], "seg_state": [], "npoly": 0, "nfaces": [], "polys": [], "goal": [0.0] * 6,
           "corridor_capacity": 0, "pieces_capacity": 0}
    L = len(route_vel)
    wpts = [list(p[:3]) for p in route_vel]
    for w in wpts:
        if w[2] < 0:
            w[2] = 0.1
    lower = [-4 + start[0], -4 + start[1], -1 + start[2]]
    higher = [4 + start[0], 4 + start[1], 1 + start[2]]
    if lower[2] < 0:
        lower[2] = 0
    if higher[2] > 4:
        higher[2] = 4
    init_corridor = get_init_corridor(higher, lower)
    # per segment: every segment of the route is restated (each is the same reading), the chain below stops at the break
    seg_valid = []
    for i in range(min(L - 1, MAX_PIECES)):
        lhc = [min(max(wpts[i][k], wpts[i + 1][k]) + init_range, higher[k]) for k in range(3)]
        llc = [max(min(wpts[i][k], wpts[i + 1][k]) - init_range, lower[k]) for k in range(3)]
        bd = init_corridor.copy()
        bd[0:3, 3] = [-v for v in lhc]
        bd[3:6, 3] = llc
        exp["box"].append([float(v) for v in bd[3:6, 3]] + [float(-v) for v in bd[0:3, 3]])
        path = [wpts[i + 1][k] - wpts[i][k] for k in range(3)]
        hp = shrink_corridor(fake, case["polys"][i], path, shrink, log)
        ok = check_corridor_validity(hp)
        log["tested"].append((hp, ok))
        exp["shrunk"].append(hp)
        state = case["seg_state"][i] if case.get("seg_state") else 1
        seg_valid.append(ok)
        exp["seg_state"].append(-3 if state == -3 else int(ok))
    trace.append(f"route_len={L}")
    if not fake and L < 2:
        trace.append("too_few_pieces")
        return exp, trace, log
    if L < 1:
        trace.append("empty")
        return exp, trace, log
    hpolys = []
    for i in range(L - 1):
        if len(hpolys) >= MAX_PIECES:
            exp["pieces_capacity"] = 1
            trace.append("pieces_capacity")
            break
        if exp["seg_state"][i] == -3:
            exp["corridor_capacity"] = 1
            trace.append(f"capacity@{i}")
            break
        if not seg_valid[i]:
            trace.append(f"seg_invalid@{i}")
            break
        hpolys.append(exp["shrunk"][i])
    if not hpolys:
        trace.append("empty")
        return exp, trace, log
    for i in range(len(hpolys) - 1):
        both = hpolys[i] + hpolys[i + 1]
        ok = check_corridor_validity(both)
        log["tested"].append((both, ok))
        if not ok:
            trace.append(f"isect_fail@{i}")
            if i < 2:
                trace.append("fail")
                return exp, trace, log
            del hpolys[(i + 1 if fake else i):]
            break
    if (len(hpolys) == 0) if fake else (len(hpolys) <= 1):
        trace.append("le1_exit")
        return exp, trace, log
    n = len(hpolys)
    goal_pos, goal_vel = list(route_vel[n - 1][:3]), list(route_vel[n - 1][3:])

    def scan(goal_pos, goal_vel):
        it = len(hpolys) - 1
        if it == 0:
            trace.append("scan_empty")
        while it != 0:
            ok, goal_pos = check_goal_reachability(hpolys[it], start, goal_pos, log)
            if ok:
                trace.append(f"scan_hit@{it}/{n - 1}")
                del hpolys[it + 1:]
                idx = len(hpolys) - 1
                goal_pos, goal_vel = list(route_vel[idx][:3]), list(route_vel[idx][3:])
                return goal_pos, goal_vel
            trace.append(f"scan_miss@{it}")
            it -= 1
        if n > 1:
            trace.append("scan_exhausted")
        return goal_pos, goal_vel

    if fake:
        goal_pos, goal_vel = scan(goal_pos, goal_vel)
    else:
        ok, goal_pos = check_goal_reachability(hpolys[-1], start, goal_pos, log)
        trace.append("first_call_in" if ok else "first_call_out")
        if not ok:
            goal_pos, goal_vel = scan(goal_pos, goal_vel)
    exp["npoly"] = len(hpolys)
    exp["nfaces"] = [len(h) for h in hpolys]
    exp["polys"] = hpolys
    exp["goal"] = [float(v) for v in goal_pos + goal_vel]
    return exp, trace, log


# ------------------------------------------------------------------------------------------------ margin conditions
def chebyshev_radius(poly):
    """largest r with a.x + |a| r <= -d for every row (negative: infeasible by that much)"""
    P = np.asarray(poly, float)
    A = np.hstack([P[:, :3], np.linalg.norm(P[:, :3], axis=1, keepdims=True)])
    res = highs([0, 0, 0, -1.0], A_ub=A, b_ub=-P[:, 3], bounds=[(None, None)] * 4, method="highs")
    assert res.status == 0, res.message
    return float(res.x[3])


def assert_margins(name, exp, log):
    for poly, ok in log["tested"]:
        r = chebyshev_radius(poly)
        assert (r >= 1e-3) if ok else (r <= -1e-3), (name, "validity margin", r, ok)
    for c, zero_path in log["cos"]:
        if zero_path:
            assert not (c > 0.8), (name, "zero path must fall through the comparison", c)
            continue
        assert abs(c - 0.8) >= 1e-6, (name, "cosine margin", c)
    for m in log["reach_max"]:
        assert abs(m) >= 1e-6, (name, "reachability margin", m)
    rng = np.random.default_rng(7)
    for c, poly, x in log["goal_lps"]:
        P = np.asarray(poly, float)
        c = np.asarray(c, float)
        ref = highs(c, A_ub=P[:, :3], b_ub=-P[:, 3], bounds=[(None, None)] * 3, method="highs")
        assert ref.status == 0 and np.abs(ref.x - np.asarray(x)).max() < 1e-9, (name, "goal LP", ref.x, x)
        for _ in range(4):
            c2 = c + 1e-4 * np.linalg.norm(c) * rng.normal(size=3)
            alt = highs(c2, A_ub=P[:, :3], b_ub=-P[:, 3], bounds=[(None, None)] * 3, method="highs")
            assert alt.status == 0 and np.abs(alt.x - ref.x).max() < 1e-7, (name, "goal LP vertex not unique")


# ------------------------------------------------------------------------------------------------ hand-built cases
def box(lo, hi, scale=(1.0,) * 6):
    rows = []
    for k in range(3):
        r = [0.0] * 4
        r[k], r[3] = 1.0, -hi[k]
        rows.append(r)
    for k in range(3):
        r = [0.0] * 4
        r[k], r[3] = -1.0, lo[k]
        rows.append(r)
    return [[v * s for v in r] for r, s in zip(rows, scale)]


def cut(n, p):
    """the half-space n.(x - p) <= 0"""
    return [float(n[0]), float(n[1]), float(n[2]), float(-(n[0] * p[0] + n[1] * p[1] + n[2] * p[2]))]


def chain(n_way, overlap, dy=0.13, dz=0.07, z0=1.0, tilt=True):
    """way-points one metre apart along x with a drift in y and z, one box per segment reaching `overlap` past both of its
    way-points, rows of unequal length (the shrink must use the norm), every other box with tilted cutting planes"""
    route = [[1.0 * i, dy * i, z0 + dz * i, 1.0 + 0.01 * i, 0.1 - 0.02 * i, 0.05 + 0.003 * i] for i in range(n_way)]
    polys = []
    for i in range(n_way - 1):
        lo = [i - overlap, dy * i - 0.8, z0 + dz * i - 0.75]
        hi = [i + 1 + overlap, dy * i + 0.9, z0 + dz * i + 0.85]
        rows = box(lo, hi, scale=(1.0, 2.0, 0.5, 1.5, 1.0, 3.0))
        if tilt and i % 2 == 1:
            c = [i + 0.5, dy * i, z0 + dz * i]
            rows.append(cut([0.3, 1.0, 0.2], [c[0], c[1] + 0.7, c[2]]))
            rows.append(cut([-0.2, -0.6, 0.9], [c[0], c[1] - 0.1, c[2] + 0.7]))
            rows.append(cut([0.5, -1.0, -0.4], [c[0], c[1] - 0.65, c[2]]))
        polys.append(rows)
    return route, polys


def empty_box(i):
    """a polytope with nothing inside: two opposing faces 0.4 apart the wrong way"""
    rows = box([i - 0.5, -0.8, 0.2], [i + 1.5, 0.9, 1.9])
    rows[0][3] = -(i + 0.1)   # x <= i + 0.1
    rows[3][3] = i + 0.9      # x >= i + 0.9  (0.8 apart: still empty after either variant's shrink)
    return rows


START = [0.05, -0.03, 0.97, 0.4, 0.0, 0.0, 0.0, 0.0, 0.0]


def base(kind, route, polys, **kw):
    c = {"kind": kind, "init_range": 1.2, "shrink_size": 0.2, "start_pva": list(START), "route": route, "polys": polys}
    c.update(kw)
    return c


def build_cases():
    """(case, predicate on (variant, exp, trace)) per kind; every kind is built for both planner variants, the predicate
    says which path that variant must take"""
    out = []

    def add(case, pred, only=None):
        out.append((case, pred, only))

    r, p = chain(5, 0.6)
    p[0] = empty_box(0)
    add(base("first_invalid", r, p), lambda v, e, t: t[1:] == ["seg_invalid@0", "empty"] and e["npoly"] == 0)

    r, p = chain(7, 0.6)
    p[3] = empty_box(3)
    add(base("k_invalid", r, p), lambda v, e, t: "seg_invalid@3" in t and e["npoly"] == 3)

    r, p = chain(6, 0.6)
    add(base("capacity", r, p, seg_state=[1, 1, 1, -3, 1]),
        lambda v, e, t: "capacity@3" in t and e["corridor_capacity"] == 1 and e["npoly"] == 3 and e["seg_state"][3] == -3)

    def gap(r, p, i):
        # polytope i + 1 starts 0.4 m past the end of polytope i: disjoint, and not empty, after either variant's shrink
        lo_x = max(-row[3] / row[0] for row in p[i] if row[0] > 0 and row[1] == 0 and row[2] == 0)
        p[i + 1].append(cut([-1.0, 0.0, 0.0], [lo_x + 0.4, 0.0, 0.0]))
        return r, p

    for i in (0, 1):
        r, p = gap(*chain(6, 0.6), i)
        add(base(f"isect_fail_{i}", r, p), lambda v, e, t, i=i: t[-2:] == [f"isect_fail@{i}", "fail"] and e["npoly"] == 0)
    r, p = gap(*chain(7, 0.6), 3)
    add(base("isect_fail_ge2", r, p),
        lambda v, e, t: "isect_fail@3" in t and e["npoly"] == (4 if v == "fake" else 3) and "fail" not in t)

    add(base("route_len_0", [], []), lambda v, e, t: e["npoly"] == 0 and t[1] == ("empty" if v == "fake" else "too_few_pieces"))
    r, p = chain(1, 0.6)
    add(base("route_len_1", r, p), lambda v, e, t: e["npoly"] == 0 and t[1] == ("empty" if v == "fake" else "too_few_pieces"))
    r, p = chain(2, 0.6)
    add(base("route_len_2", r, p), lambda v, e, t: (e["npoly"] == 1 and "scan_empty" in t) if v == "fake" else t[-1] == "le1_exit")

    r, p = chain(5, 0.6)
    p[1] = empty_box(1)
    add(base("le1_exit", r, p), lambda v, e, t: t[-1] == "le1_exit" and "seg_invalid@1" in t and e["npoly"] == 0, only="real")

    r, p = chain(19, 0.6, dy=0.05, dz=0.01, tilt=False)
    add(base("route_gt16", r, p), lambda v, e, t: "pieces_capacity" in t and e["pieces_capacity"] == 1 and e["npoly"] >= 1)

    r, p = chain(6, 0.6)
    add(base("goal_in_last", r, p),
        lambda v, e, t: e["npoly"] == 5 and t[-1] == ("scan_hit@4/4" if v == "fake" else "first_call_in"))

    # the last polytope does not hold its own first way-point (the goal), the one before holds the middle of the last
    r, p = chain(6, 2.0, tilt=False)
    p[4].append(cut([-1.0, 0.1, 0.0], [4.35, 0.52, 1.28]))
    add(base("goal_in_earlier", r, p),
        lambda v, e, t: t[-2:] == ["scan_miss@4", "scan_hit@3/4"] and e["npoly"] == 4 and e["goal"][:3] == r[3][:3],
        only="fake")
    add(base("first_call_projects", r, p),
        lambda v, e, t: t[-2:] == ["first_call_out", "scan_hit@4/4"] and e["npoly"] == 5 and e["goal"][:3] == r[4][:3],
        only="real")

    # short overlaps: the middle of polytope k lies outside polytope k - 1 every time, the projection is carried on
    r, p = chain(6, 0.3, tilt=False)
    p[4].append(cut([-1.0, 0.1, 0.0], [4.1, 0.52, 1.28]))
    add(base("goal_outside_all", r, p),
        lambda v, e, t: t[-5:] == ["scan_miss@4", "scan_miss@3", "scan_miss@2", "scan_miss@1", "scan_exhausted"] and
        e["npoly"] == 5 and all(g not in sum(r, []) for g in e["goal"][:3]), only="fake")

    r, p = chain(2, 0.6)
    p[0].append(cut([-1.0, 0.1, 0.0], [0.35, 0.0, 1.0]))
    add(base("single_poly_goal_outside", r, p),
        lambda v, e, t: e["npoly"] == 1 and "scan_empty" in t and e["goal"][:3] == r[0][:3] and
        max(row[0] * r[0][0] + row[1] * r[0][1] + row[2] * r[0][2] + row[3] for row in e["polys"][0]) > 1e-3, only="fake")

    # a way-point below the ground: lifted to 0.1 for the box and the path, not in route_vel, where the goal comes from
    r, p = chain(3, 0.6, z0=0.4, dz=0.0)
    r[0][2], r[1][2] = -0.3, -0.05
    for rows in p:
        rows[5][3] = -0.5 * 3.0   # z >= -0.5: the injected polytopes reach below the ground
    add(base("z_negative", r, p, start_pva=[0.05, -0.03, 0.5] + [0.0] * 6),
        lambda v, e, t: e["npoly"] == 2 and e["goal"][2] == -0.05 and e["box"][0][5] == 0.1 + 1.2 and e["box"][0][2] == 0.0)

    r, p = chain(4, 0.6, z0=0.5, dz=0.02)
    add(base("start_z_low", r, p, start_pva=[0.05, -0.03, 0.3] + [0.0] * 6),
        lambda v, e, t: all(b[2] == 0.0 for b in e["box"]) and all(b[5] == 1.3 for b in e["box"]))
    r, p = chain(4, 0.6, z0=3.3, dz=0.02)
    add(base("start_z_high", r, p, start_pva=[0.05, -0.03, 3.6] + [0.0] * 6),
        lambda v, e, t: all(b[5] == 4.0 for b in e["box"]) and all(b[2] > 2.0 for b in e["box"]))
    r, p = chain(4, 0.6)
    add(base("init_range_wide", r, p, init_range=7.5),
        lambda v, e, t: all(b == [0.05 - 4, -0.03 - 4, 0.0, 0.05 + 4, -0.03 + 4, 0.97 + 1] for b in e["box"]))

    # faces on both sides of both 0.8 tests: cosine to the path 0.85 / 0.75 (first test), |n_z| / |n| 0.85 / 0.75 (second)
    r, p = chain(4, 0.6, dy=0.0, dz=0.0, tilt=False)
    for i, rows in enumerate(p):
        c = [i + 0.5, 0.0, 1.0]
        for cs in (0.85, 0.75):
            s = math.sqrt(1 - cs * cs)
            rows.append(cut([cs * 1.7, s * 1.7, 0.0], [c[0] + 1.0, c[1] + 0.3, c[2]]))      # looks along the path
            rows.append(cut([0.0, s * 0.6, cs * 0.6], [c[0], c[1] + 0.3, c[2] + 0.6]))      # looks up
            rows.append(cut([0.1, -s * 1.3, -cs * 1.3], [c[0], c[1] - 0.3, c[2] - 0.6]))    # looks down
    add(base("shrink_sides", r, p), lambda v, e, t: e["npoly"] == 3)

    # a segment whose two way-points coincide: path = 0, the text divides by path.norm() = 0
    r, p = chain(5, 0.6)
    r[4][:3] = r[3][:3]
    add(base("zero_path", r, p), lambda v, e, t: e["npoly"] == 4)
    r, p = chain(5, 0.6)
    add(base("shrink_zero", r, p, shrink_size=0.0),
        lambda v, e, t: e["npoly"] == 4 and all(e["shrunk"][i] == p[i] for i in range(4)))
    return out


def main():
    cases = []
    for case, pred, only in build_cases():
        for variant in ("fake", "real"):
            if only and only != variant:
                continue
            c = dict(case)
            c["fake"] = 1 if variant == "fake" else 0
            assert all(6 <= len(rows) <= MAX_FACES for rows in c["polys"]), c["kind"]
            exp, trace, log = corridor_rules(c)
            name = f"{variant}/{c['kind']}"
            assert pred(variant, exp, trace), (name, trace, exp["npoly"], exp["goal"])
            assert_margins(name, exp, log)
            if c["kind"] == "shrink_sides" and variant == "fake":   # both outcomes of both tests occurred
                firsts = [x for x, _ in log["cos"]]
                assert any(0.8 < x < 0.9 for x in firsts) and any(0.7 < x < 0.8 for x in firsts), firsts
            if c["kind"] == "zero_path" and variant == "fake":
                assert any(z for _, z in log["cos"])
            c["branch"] = name
            c["trace"] = trace
            c["expected"] = exp
            cases.append(c)
    out = {"what": "corridor rules around FIRI restated independently in numpy (tests/golden/make_corridor_rules_fixture.py): "
                   "polytope rows h with h.x + h3 <= 0; box = llc, lhc; seg_state 1 valid, 0 invalid, -3 capacity",
           "max_faces": MAX_FACES, "cases": cases}
    path = os.path.join(HERE, "corridor_rules_independent.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(f"written {path}: {len(cases)} cases, {os.path.getsize(path)} bytes")
    print(sorted(c["branch"] for c in cases))


if __name__ == "__main__":
    main()
