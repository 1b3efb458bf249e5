#!/usr/bin/env python
"""An INDEPENDENT second reading of WHICH POINTS ParticleATC::isSafeAfterOpt compares — written straight from the
reference's text in numpy WITHOUT reading oracle/ or the HIP kernels — whose piece indices, point counts and verdicts on
seeded swarms are committed as tests/golden/safe_after_opt_independent.json; tests/test_safe_after_opt_independent.py
holds the C++ oracle (`orc_safe_after_opt`) and the HIP kernel (`isSafeAfterOpt`) to them.

Restated:
  traj_coordinator/src/particles.cpp:147-176   the trajectory callback: time_end = time_start + the durations, added one
                                               after the other in message order
  traj_coordinator/src/particles.cpp:223-283   isSafeAfterOpt: a record is skipped by its drone id (not by its place in
                                               the table), the window is strict on both sides, the passed pieces are
                                               dropped with bottomRows(rows - piece_idx * (order + 1))
  traj_utils/include/traj_utils/bernstein.hpp:164-172   Bezier::locatePiece: subtract duration after duration, the first
                                               NEGATIVE remainder names the piece; a time exactly on a boundary belongs
                                               to the later piece, past the end to the last
  utils/separator/src/separator_glpk.cpp:73-190  the feasibility LP  n.a + d >= 1,  n.b + d <= -1  — decided here by scipy
                                               HiGHS, as tests/test_deconflict.py does
Every time in the fixture is a multiple of 1/16 s near 100 s, so sums and differences are exact and "equal" means equal.

Geometry: every ego of a group owns a site 10 m from the next; its control points are a tetrahedron around the site plus
points inside it.  A piece of a record visits up to three egos' sites (two, two and one of its five points within 0.1 m
of a site: deep inside that ego's hull) and parks its other points far away, so a pair (ego, record) is unsafe exactly
when a piece that visits the ego has not been passed yet: one piece index too low or too high flips the verdict.  The generator asserts that every pair is separable
with a margin >= 1e-3 or overlaps by >= 1e-3 (still inseparable after any shift of 1e-3 along 14 directions).
Run from the repo root:   python tests/golden/make_safe_after_opt_fixture.py
"""
import json
import os

import numpy as np
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
ORDER = 4  # Bezier order: order + 1 = 5 control points per piece
EGOS = 6   # per group


# ------------------------------------------------------------------------------------------------ the second reading
def callback_time_end(time_start, durations):
    t_end = time_start
    for d in durations:
        t_end += d
    return t_end


def locate_piece(durations, t):
    for i, d in enumerate(durations):
        t -= d
        if t < 0:
            return i
    return len(durations) - 1


def separable(A, B):
    rows = np.concatenate([np.hstack([-A, -np.ones((len(A), 1))]), np.hstack([B, np.ones((len(B), 1))])])
    res = linprog(np.zeros(4), A_ub=rows, b_ub=-np.ones(len(rows)), bounds=[(None, None)] * 4, method="highs")
    return res.status == 0


def compared_points(rec, drone_id, t0):
    """(piece index, the record's points that are compared) or (None, None) when the record is passed over"""
    if rec["drone_id"] == drone_id:
        return None, None
    durations = rec["duration"]
    time_end = callback_time_end(rec["time_start"], durations)
    if not (rec["time_start"] < t0 and t0 < time_end):
        return None, None
    cpts = np.asarray(rec["cpts"], float).reshape(-1, 3)
    piece_idx = locate_piece(durations, t0 - rec["time_start"])
    return piece_idx, cpts[piece_idx * (ORDER + 1):]          # bottomRows(rows - piece_idx * order)


def is_safe_after_opt(ego_cpts, records, drone_id, t0):
    A = np.asarray(ego_cpts, float).reshape(-1, 3)
    for rec in records:
        _, B = compared_points(rec, drone_id, t0)
        if B is not None and not separable(A, B):
            return False
    return True


# ------------------------------------------------------------------------------------------------ margin condition
DIRS = [np.array(d, float) / np.linalg.norm(d) for d in
        [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] +
        [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]]


def separation_margin(A, B):
    """largest t with n.a + d >= t, n.b + d <= -t, |n|_inf <= 1: the hulls are >= 2 t / sqrt(3) apart"""
    rows = np.concatenate([np.hstack([-A, -np.ones((len(A), 1)), np.ones((len(A), 1))]),
                           np.hstack([B, np.ones((len(B), 1)), np.ones((len(B), 1))])])
    res = linprog([0, 0, 0, 0, -1.0], A_ub=rows, b_ub=np.zeros(len(rows)),
                  bounds=[(-1, 1)] * 3 + [(None, None), (None, None)], method="highs")
    assert res.status == 0
    return float(res.x[4])


def assert_margin(A, B, safe, what):
    if safe:
        assert separation_margin(A, B) >= 1e-3, what
    else:
        for d in DIRS:
            assert not separable(A, B + 1e-3 * d), what


# ------------------------------------------------------------------------------------------------ seeded swarms
TETRA = 0.5 * np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], float)   # inscribed sphere: 0.29 m


def ego_points(rng, site, M):
    pts = [site + v for v in TETRA] + [site.copy()]
    while len(pts) < 5 * M:
        pts.append(site + rng.uniform(-0.12, 0.12, 3))
    return np.asarray(pts)


def q16(x):
    return round(x * 16) / 16.0


def make_group(rng, g, timing_cases):
    sites = np.array([[10.0 * e, 3.0 * (e % 2) + 0.7 * e * e, 1.0 + 0.2 * e] for e in range(EGOS)])   # no three in a line
    ids = rng.permutation(12)[:EGOS].tolist()                      # drone ids: no relation to the place in the table
    t_now = [100.0 + q16(rng.uniform(0, 0.5)) for _ in range(EGOS)]
    npoly = [int(rng.integers(1, 9)) for _ in range(EGOS)]
    npoly[0], npoly[1] = (1, 8) if g % 2 == 0 else (8, 1)
    egos = [{"drone_id": ids[e], "t_now": t_now[e], "npoly": npoly[e],
             "cpts": ego_points(rng, sites[e], npoly[e]).reshape(-1).tolist()} for e in range(EGOS)]
    n_rec = int(rng.integers(3, 7))
    records = []
    for r in range(n_rec):
        case = timing_cases.pop() if timing_cases else "generic"
        e_star = int(rng.integers(0, EGOS))                          # the ego this record's timing is built around
        n = 0 if case == "no_pieces" else int(rng.integers(1, 9))
        if case == "piece_boundary":
            n = max(n, 2)
        durs = [float(rng.integers(2, 9)) / 8.0 for _ in range(n)]   # unequal, multiples of 1/8 s
        total = sum(durs)
        if case == "at_time_start":
            off = 0.0
        elif case == "at_time_end":
            off = total
        elif case == "piece_boundary":
            off = sum(durs[:int(rng.integers(1, n))])
        elif case == "in_last_piece":
            off = total - durs[-1] / 2.0
        elif case == "not_started":
            off = -q16(rng.uniform(0.1, 3))
        elif case == "ended":
            off = total + q16(rng.uniform(0.1, 3)) + 0.0625
        else:
            off = q16(rng.uniform(0, total)) if n else 0.0
        rec_id = 20 + r
        # a piece visits up to three egos' sites (two, two and one of its five points), or parks
        visits = [[int(v) for v in rng.permutation(EGOS)[:3] if rng.uniform() < 0.8] for _ in range(n)]
        if case == "own_record":                                     # the ego's own earlier trajectory: all over its site
            rec_id, visits = ids[e_star], [[e_star] for _ in range(n)]
            off = min(off, total - 0.0625) if off >= total else max(off, 0.0625)
        if case in ("piece_boundary", "in_last_piece", "at_time_start", "at_time_end"):
            k = locate_piece(durs, off)
            visits[k] = [e_star] + [v for v in visits[k] if v != e_star][:2]   # the piece the boundary rule decides about
            if case == "piece_boundary":
                visits[k - 1] = [e_star] + [v for v in visits[k - 1] if v != e_star][:2]   # just passed: must be dropped
                keep = rng.uniform() < 0.5
                for j in range(k, n):
                    if j > k or not keep:
                        visits[j] = [v for v in visits[j] if v != e_star]
        pts = []
        for k in range(n):
            park = np.array([5.0 + 10.0 * r, 90.0 + 4.0 * k, 2.0])
            five = [park + rng.uniform(-0.5, 0.5, 3) for _ in range(5)]
            for slot, v in zip(([0, 1], [2, 3], [4]), visits[k]):
                for q in slot:
                    five[q] = sites[v] + rng.uniform(-0.1, 0.1, 3)
            pts.append(np.asarray(five))
        records.append({"drone_id": rec_id, "n_pieces": n, "time_start": t_now[e_star] - off, "duration": durs,
                        "cpts": np.asarray(pts).reshape(-1).tolist() if n else [], "case": case, "built_around": e_star})
    # places in the table: a record built around ego e that is NOT its own sits at place e when it can (a foreign record
    # at the ego's index), an own record never sits at its ego's place
    order = list(range(n_rec))
    rng.shuffle(order)
    records = [records[i] for i in order]
    for i, rec in enumerate(records):
        e = rec["built_around"]
        if rec["case"] == "own_record" and i == e:
            j = (i + 1) % n_rec
            records[i], records[j] = records[j], records[i]
    for i, rec in enumerate(records):
        e = rec["built_around"]
        if rec["case"] == "foreign_at_index" and e < n_rec and records[e]["case"] == "generic":
            records[i], records[e] = records[e], records[i]
    return {"egos": egos, "records": records}


def main():
    rng = np.random.default_rng(0x5AFE)
    special = ["at_time_start", "at_time_end", "piece_boundary", "in_last_piece", "no_pieces", "not_started", "ended",
               "own_record", "foreign_at_index"]
    timing_cases = (special * 4)[::-1]
    groups = [make_group(rng, g, timing_cases) for g in range(10)]
    assert not timing_cases
    n_pairs = n_safe = 0
    seen = set()
    one_of_many = 0
    for grp in groups:
        for e, ego in enumerate(grp["egos"]):
            A = np.asarray(ego["cpts"]).reshape(-1, 3)
            ego["pairs"] = []
            for i, rec in enumerate(grp["records"]):
                piece, B = compared_points(rec, ego["drone_id"], ego["t_now"])
                safe = True if B is None else separable(A, B)
                if B is not None:
                    assert_margin(A, B, safe, (e, i))
                ego["pairs"].append({"piece": piece, "n_points": 0 if B is None else len(B), "safe": int(safe)})
                n_pairs += 1
                n_safe += int(safe)
                if rec["built_around"] == e:
                    seen.add((rec["case"], piece is None, safe))
                    # what each special case is there to show
                    if rec["case"] in ("at_time_start", "at_time_end", "no_pieces", "not_started", "ended", "own_record"):
                        assert piece is None, rec["case"]
                    if rec["case"] == "own_record":
                        assert i != e and rec["drone_id"] == ego["drone_id"] and not separable(
                            A, np.asarray(rec["cpts"]).reshape(-1, 3))
                    if rec["case"] == "piece_boundary":
                        off = ego["t_now"] - rec["time_start"]
                        assert off == sum(rec["duration"][:piece]) and piece >= 1
                        passed = np.asarray(rec["cpts"]).reshape(-1, 3)[(piece - 1) * 5:piece * 5]
                        assert not separable(A, passed)           # one index lower would have said unsafe
                    if rec["case"] == "in_last_piece":
                        assert piece == rec["n_pieces"] - 1 and not safe
                    if rec["case"] == "foreign_at_index" and i == e:
                        seen.add("foreign_at_index_placed")
            ego["safe"] = int(is_safe_after_opt(ego["cpts"], grp["records"], ego["drone_id"], ego["t_now"]))
            assert ego["safe"] == int(all(p["safe"] for p in ego["pairs"]))
            if len(grp["records"]) >= 3 and sum(1 - p["safe"] for p in ego["pairs"]) == 1:
                one_of_many += 1
    assert 0.25 <= n_safe / n_pairs <= 0.75, (n_safe, n_pairs)
    assert "foreign_at_index_placed" in seen and one_of_many >= 5
    assert any(c == "piece_boundary" and s for c, _, s in (x for x in seen if isinstance(x, tuple)))
    assert any(c == "piece_boundary" and not s for c, _, s in (x for x in seen if isinstance(x, tuple)))
    assert {1, 8} <= {ego["npoly"] for grp in groups for ego in grp["egos"]}
    out = {"what": "isSafeAfterOpt's choice of points restated independently (tests/golden/make_safe_after_opt_fixture.py): "
                   "per (ego, record) the piece index (null: record passed over), the number of the record's points "
                   "compared and the pair's verdict; per ego the overall verdict",
           "groups": groups}
    path = os.path.join(HERE, "safe_after_opt_independent.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print(f"written {path}: {sum(len(g['egos']) for g in groups)} egos, {n_pairs} pairs, {n_safe} safe, "
          f"{one_of_many} egos with exactly one colliding record, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
