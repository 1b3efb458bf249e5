#!/usr/bin/env python
"""An INDEPENDENT second reading of HOW A REPLAN ENDS — ParticleATC::isSafeAfterOpt against a swarm table of up to 130
records, where replan() returned, the published BezierTraj record and what the tables hold afterwards — written in numpy and
scipy (HiGHS) from the reference's text WITHOUT reading oracle/ or the HIP kernels, committed as
tests/golden/finish_independent.json; tests/test_finish_independent.py holds the C++ oracle and BOTH device forms of the
finish (the grouped kernels and the finishing wave, sogm_finish_batched) to it.

Restated:
  traj_coordinator/src/particles.cpp:147-283       the trajectory callback and isSafeAfterOpt: records in table order, the
                                                   first inseparable one ends the check (imported from
                                                   make_safe_after_opt_fixture.py with locatePiece, bernstein.hpp:164-172,
                                                   and the LP of utils/separator/src/separator_glpk.cpp)
  plan_manager/src/baseline_fake.cpp:292,405-419,447,455   where replan() returns false: no path, no corridor, the QP's status,
                                                   isSafeAfterOpt — in this order
  plan_manager/src/plan_manager.cpp:176-196        a successful replan publishes, a failed one keeps the previous trajectory
  plan_manager/src/plan_manager.cpp:364-399        the published record: drone id, start time, one duration per piece, the
                                                   control points
All times are multiples of 1/16 s near 100 s.  Coordinates are rounded to 1e-3 BEFORE anything is decided about them.

The PRE-TESTS (bounding boxes, ten fixed normals in the kernels' order, the line between the box centres, products
associated as (n0 x + n1 y) + n2 z) are stated here only to CLASSIFY a pair — never to produce a verdict:
  far       boxes disjoint by >= 1e-3                       inactive  not started, ended or n_pieces == 0
  own       the ego's own drone id, lying over its site     unsafe    overlapping by >= 1e-3
  lp_safe   no pre-test separates the pair and every projection pair overlaps by >= 1e-3, HiGHS separates it with margin
            >= 1e-3: two thin slabs either side of an oblique plane, centres offset within the plane, rejection-sampled
  capacity  5 M + the record's remaining points > 144: this library's documented deviation "treated as unsafe" (DESIGN.md);
            the reference has no such limit, the fixture marks the pair "capacity"
Groups (one swarm table and <= 16 egos each; `kind`):
  chunk        tables of 1, 63, 64, 65, 128, 130 records; per place 0 / 62 / 63 / 64 / 127 / 128 / 129 one ego whose only
               unsafe record sits there with lp_safe records in every earlier 64-record chunk and earlier in its own chunk;
               egos that are safe only because every chunk's lp_safe records are separable; own and inactive records over
               the egos' sites; npoly 1, 8, 16
  capacity     egos with M = 16: 140-row pairs (M + remaining pieces = 28) that are lp_safe / unsafe, 145-row pairs (29) that
               are far by the boxes; no unsafe record in front of an over-capacity one
  early_exit   an unsafe record IN FRONT of an over-capacity one: the reference's loop has returned before it meets it
               (capacity_sequential = 0), a form that tests every pair counts it (capacity_all = 1)
  publication  ret x npoly x status x swarm verdict x due: outcome, ok flag, record, and the tables afterwards
Run from the repo root:   python tests/golden/make_finish_fixture.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_safe_after_opt_fixture import assert_margin, compared_points, is_safe_after_opt, q16, separable  # noqa: E402

MAX_PIECES = 16
CAPACITY_ROWS = 144          # the library's LP capacity in point rows (its documented deviation)
TAU = 0.3                    # the duration of every piece of a replan's trajectory
OUTCOMES = ("replan_ok", "fail_search", "fail_corridor", "fail_qp", "fail_unsafe")


# ------------------------------------------------------------------------------------------------ the second reading
def replan_outcome(ret, npoly, status, safe):
    """where replan() returned (baseline_fake.cpp:292 no path, :405-419 no corridor, :447 the QP, :455 isSafeAfterOpt)"""
    if ret == 0:
        return 1
    if npoly <= 0:
        return 2
    if status not in (1, 2):
        return 3
    if not safe:
        return 4
    return 0


def published_record(good, drone_id, t_start, npoly):
    """publishTrajectory (plan_manager.cpp:364-399) as a description: durations and the number of control-point
    coordinates taken from the optimiser's; a failed replan's record is empty (n_pieces = 0)"""
    M = npoly if good else 0
    return {"drone_id": drone_id, "time_start": t_start, "n_pieces": M, "duration": [TAU] * M, "n_cpts": 15 * M}


def tables_afterwards(good):
    """what the agent's own table (latest trajectory) and the next swarm table hold, per which of the two exist
    (plan_manager.cpp:176-196: success publishes, failure keeps executing the previous trajectory).  "new": this replan's
    record, "prev_own" / "prev_table": what the table held before.  Without an own table nothing is published."""
    own = "new" if good else "prev_own"
    return {"own+table": [own, own], "own": [own, None], "table": [None, "prev_table"], "none": [None, None]}


# ------------------------------------------------------------------------------------------------ pre-tests (classification)
FIXED = [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1), (1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]


def project(n, P):
    return (n[0] * P[:, 0] + n[1] * P[:, 1]) + n[2] * P[:, 2]


def pretests(A, B):
    """(the first pre-test that separates: "box" | "normal" | "centre" | None, the smallest overlap of all 14 projection
    pairs, the largest box gap)"""
    first, overlaps, box_gap = None, [], -np.inf
    for k in range(3):
        gap = max(B[:, k].min() - A[:, k].max(), A[:, k].min() - B[:, k].max())
        box_gap = max(box_gap, gap)
        overlaps.append(-gap)
        if gap > 0 and first is None:
            first = "box"
    centre = 0.5 * (B.min(0) + B.max(0)) - 0.5 * (A.min(0) + A.max(0))
    for q, n in enumerate(FIXED + [tuple(centre)]):
        pa, pb = project(n, A), project(n, B)
        gap = max(pb.min() - pa.max(), pa.min() - pb.max())
        overlaps.append(-gap)
        if gap > 0 and first is None:
            first = "normal" if q < 10 else "centre"
    return first, min(overlaps), box_gap


def classify(A, rec, drone_id, t_now):
    """(category letter, piece or -1, number of compared points, verdict of the pair as this library documents it)"""
    if rec["drone_id"] == drone_id:
        assert rec["n_pieces"] > 0 and not separable(A, np.asarray(rec["cpts"]).reshape(-1, 3))   # lies over the site
        return "o", -1, 0, 1
    piece, B = compared_points(rec, drone_id, t_now) if rec["n_pieces"] > 0 else (None, None)
    if B is None:
        return "i", -1, 0, 1
    if len(A) + len(B) > CAPACITY_ROWS:                      # decided in front of everything else
        assert pretests(A, B)[2] >= 1e-3                      # ... shown by pairs the boxes would have separated
        return "c", piece, len(B), 0
    first, overlap, box_gap = pretests(A, B)
    if box_gap >= 1e-3:
        assert separable(A, B)
        return "f", piece, len(B), 1
    assert first is None and overlap >= 1e-3, (first, overlap)   # nothing but far pairs may end in a pre-test
    safe = separable(A, B)
    assert_margin(A, B, safe, "margin")
    return ("l" if safe else "u"), piece, len(B), int(safe)


# ------------------------------------------------------------------------------------------------ geometry
N_HAT = np.array([0.41, 0.56, 0.72]) / np.linalg.norm([0.41, 0.56, 0.72])     # the oblique plane's normal
U_HAT = np.cross(N_HAT, [0, 0, 1.0]) / np.linalg.norm(np.cross(N_HAT, [0, 0, 1.0]))
V_HAT = np.cross(N_HAT, U_HAT)


def frame(site, a, b, s):
    return site + a * U_HAT + b * V_HAT + s * N_HAT


def ego_points(rng, site, M):
    """a flat pyramid BELOW the plane through the site (s <= -0.02): its base in the first four points, its apex the
    fifth, so that the first five points of any M already carry the hull's extent"""
    pts = [frame(site, a, b, -0.02) for a, b in ((1, 1), (1, -1), (-1, 1), (-1, -1))] + [frame(site, 0, 0, -0.14)]
    while len(pts) < 5 * M:
        pts.append(frame(site, rng.uniform(-0.9, 0.9), rng.uniform(-0.9, 0.9), -rng.uniform(0.03, 0.12)))
    return np.round(np.asarray(pts), 3)


def slab_piece(rng, site, c):
    """five points ABOVE the plane (s >= 0.02), centre offset by c within the plane"""
    five = [frame(site, c[0] + a, c[1] + b, rng.uniform(0.02, 0.05)) for a, b in ((1, 1), (1, -1), (-1, 1), (-1, -1))]
    five.append(frame(site, c[0] + rng.uniform(-0.5, 0.5), c[1] + rng.uniform(-0.5, 0.5), rng.uniform(0.05, 0.12)))
    return np.asarray(five)


def crossing_piece(rng, site, c):
    """five points either side of the plane, through the pyramid: inseparable from it"""
    five = [frame(site, c[0] + rng.uniform(-0.4, 0.4), c[1] + rng.uniform(-0.4, 0.4), s) for s in (0.5, -0.5, 0.4, -0.6, 0.3)]
    return np.asarray(five)


def parked_piece(rng, i, k=0):
    park = np.array([5.0 + 3.0 * (i % 40), 300.0 + 4.0 * k + 7.0 * (i // 40), 2.0])
    return park + rng.uniform(-0.5, 0.5, (5, 3))


def record(drone_id, time_start, durations, pieces, case):
    pts = np.round(np.asarray(pieces).reshape(-1), 3).tolist() if len(pieces) else []
    return {"drone_id": int(drone_id), "n_pieces": len(durations), "time_start": float(time_start),
            "duration": [float(d) for d in durations], "cpts": pts, "case": case}


def timed(rng, n_passed, n_left, t_now):
    """durations (multiples of 1/8 s) and a start time such that t_now lies in piece n_passed — for half of them exactly
    on its first instant (a boundary belongs to the later piece) — and the record stays active for 1 s around it"""
    durs = [float(rng.integers(2, 9)) / 8.0 for _ in range(n_passed)] + [2.0 + float(rng.integers(0, 5)) / 8.0] + \
           [float(rng.integers(2, 9)) / 8.0 for _ in range(n_left - 1)]
    into = 0.0 if (n_passed and rng.uniform() < 0.5) else 1.0
    return durs, t_now - sum(durs[:n_passed]) - into


def active_record(rng, kind, site, t_now, drone_id, n_passed, n_left, place):
    """an lp_safe ("l") or unsafe ("u") record for the ego at `site`: the passed pieces of an lp_safe record cross the
    ego's pyramid (one piece index too low says unsafe), those of an unsafe one are parked (too high says safe: the
    pieces behind the crossing one are parked as well)"""
    th = rng.uniform(0, 2 * np.pi)
    c = rng.uniform(0.3, 0.6) * np.array([np.cos(th), np.sin(th)])
    durs, ts = timed(rng, n_passed, n_left, t_now)
    pieces = []
    for k in range(n_passed + n_left):
        if kind == "l":
            pieces.append(crossing_piece(rng, site, c) if k < n_passed else slab_piece(rng, site, c))
        else:
            # (parked above the ego's own site: the record's box stays clear of every other ego's)
            pieces.append(crossing_piece(rng, site, c) if k == n_passed else
                          site + [0.0, 0.0, 40.0 + 4.0 * k] + rng.uniform(-0.5, 0.5, (5, 3)))
    return record(drone_id, ts, durs, pieces, {"l": "lp_safe", "u": "unsafe"}[kind])


def sample_active(rng, kind, A, site, t_now, drone_id, n_passed, n_left, place):
    for _ in range(200):                                      # rejection sampling on the category
        rec = active_record(rng, kind, site, t_now, drone_id, n_passed, n_left, place)
        try:
            if classify(A, rec, -1, t_now)[0] == kind:
                return rec
        except AssertionError:
            pass
    raise AssertionError("no sample of category " + kind)


def filler(rng, place, sites, t_lo):
    """one piece: far (parked, active) or inactive — not started / ended / no pieces — over one of the sites"""
    kind = ("far", "far", "not_started", "ended", "no_pieces")[int(rng.integers(0, 5))]
    if kind == "far":
        return record(500 + place, t_lo - 1.0, [4.0], [parked_piece(rng, place)], "far")
    over = crossing_piece(rng, sites[int(rng.integers(0, len(sites)))], (0.0, 0.0))
    if kind == "no_pieces":
        return record(500 + place, t_lo - 1.0, [], [], "inactive")
    ts, d = (t_lo + 1.0 + q16(rng.uniform(0, 1)), 4.0) if kind == "not_started" else (t_lo - 3.0, 1.0 + q16(rng.uniform(0, 1)))
    return record(500 + place, ts, [d], [over], "inactive")


def site_of(e):
    return np.array([20.0 + 12.0 * e, 25.0 + 3.0 * (e % 3), 4.0 + 0.5 * e])


# ------------------------------------------------------------------------------------------------ groups
def finish_group(kind, records, egos):
    """the reading of one group: per ego the pairs, the swarm verdict, where the replan ended, the record, the tables"""
    cap_all = cap_seq = 0
    counts = dict.fromkeys(OUTCOMES, 0)
    for ego in egos:
        M = ego["npoly"]
        A = np.asarray(ego["cpts"] if ego["cpts"] is not None else ego["_cpts"]).reshape(-1, 3)[:5 * max(M, 0)]
        cat, piece, safe = "", [], ""
        if M > 0:
            for rec in records:
                c, p, _, s = classify(A, rec, ego["drone_id"], ego["t_now"])
                cat, safe = cat + c, safe + str(s)
                piece.append(p)
            verdict = int(all(s == "1" for s in safe))
            # the reference's own loop agrees wherever the capacity rule is not involved
            if "c" not in cat:
                assert verdict == int(is_safe_after_opt(A.reshape(-1), records, ego["drone_id"], ego["t_now"]))
            cap_all += cat.count("c")
            first_unsafe = safe.find("0")
            cap_seq += sum(1 for i, c in enumerate(cat) if c == "c" and i <= first_unsafe)
        else:
            verdict = 1                                       # nothing was optimised: the check is never reached
        solved = int(ego["ret"] != 0 and M > 0 and ego["status"] in (1, 2))
        outcome = replan_outcome(ego["ret"], M, ego["status"], bool(verdict))
        good = outcome == 0
        assert good == bool(solved and verdict)
        if ego["due"] is None or ego["due"] != 0:
            counts[OUTCOMES[outcome]] += 1
        ego.update({"pair_cat": cat, "pair_safe": safe, "pair_piece": piece, "safe": verdict, "solved": solved,
                    "outcome": outcome, "ok": int(good), "out": published_record(good, ego["drone_id"], ego["t_start"], M),
                    "pub": tables_afterwards(good)})
        ego.pop("_cpts", None)
    return {"kind": kind, "n_swarm": len(records), "records": records, "egos": egos, "counts": counts,
            "capacity_all": cap_all, "capacity_sequential": cap_seq}


def new_ego(rng, e, M, cpts=None, **kw):
    t_now = 100.0 + q16(rng.uniform(0, 0.25))
    ego = {"drone_id": 40 + e, "t_now": t_now, "t_start": t_now + 0.0625 * int(rng.integers(1, 9)), "ret": 1, "npoly": M,
           "status": int(rng.integers(1, 3)), "due": None,
           "cpts": (ego_points(rng, site_of(e), M) if cpts is None else cpts).reshape(-1).tolist()}
    ego.update(kw)
    return ego


def chunk_group(rng, L, plan):
    """plan: per ego (npoly, {place: "l" | "u" | "o"}); the other places are filler"""
    egos = [new_ego(rng, e, M) for e, (M, _) in enumerate(plan)]
    sites = [site_of(e) for e in range(len(plan))]
    records = [None] * L
    for e, (M, places) in enumerate(plan):
        A = np.asarray(egos[e]["cpts"]).reshape(-1, 3)
        for place, kind in places.items():
            assert records[place] is None, (L, e, place)
            if kind == "o":
                assert place != e
                records[place] = record(egos[e]["drone_id"], egos[e]["t_now"] - 1.0, [4.0],
                                        [crossing_piece(rng, sites[e], (0.0, 0.0))], "own")
            else:
                n_passed, n_left = int(rng.integers(0, 3)), int(rng.integers(1, 3))
                records[place] = sample_active(rng, kind, A, sites[e], egos[e]["t_now"], 600 + place, n_passed, n_left, place)
    for place in range(L):
        if records[place] is None:
            records[place] = filler(rng, place, sites, 100.0)
    return finish_group("chunk", records, egos)


def chunk_plans(rng, L, unsafe_egos):
    """the egos of a table of L records: one per place 0 / 62 / 63 / 64 / 127 / 128 / 129 whose only unsafe record sits
    there (unsafe_egos), then egos that are safe because the lp_safe records of EVERY chunk are separable"""
    npolys = [1, 8, 16, 3, 5, 2, 11, 16, 7, 1, 8, 4]
    special = [p for p in (0, 62, 63, 64, 127, 128, 129) if p < L and unsafe_egos]
    free = [p for p in range(L) if p not in special]

    def take(lo, hi):
        cand = [p for p in free if lo <= p < hi]
        p = cand[int(rng.integers(0, len(cand)))]
        free.remove(p)
        return p

    plan = []
    for place in special:
        places = {place: "u"}
        for c0 in range(0, place - place % 64, 64):            # an lp_safe record in every earlier chunk ...
            places[take(c0, c0 + 64)] = "l"
        if place % 64 > 1:                                      # ... and earlier in its own chunk
            places[take(place - place % 64, place)] = "l"
        if L >= 63 and place % 3 == 0:                          # the ego's own earlier trajectory somewhere
            places[take(0, L)] = "o"
        plan.append((npolys[len(plan) % len(npolys)], places))
    n_safe = 3
    for k in range(n_safe):
        e, places = len(plan), {}
        room = [len([p for p in free if c0 <= p < c0 + 64]) for c0 in range(0, L, 64)]
        if min(room) < n_safe - k:
            continue                                            # a chunk without a place left: no such ego
        for c0, r in zip(range(0, L, 64), room):
            for j in range(2 if r >= 2 * (n_safe - k) else 1):
                if c0 == 0 and j == 0 and e in free:            # a foreign record at the ego's own table place
                    free.remove(e)
                    places[e] = "l"
                else:
                    places[take(c0, c0 + 64)] = "l"
        if L > 1 and free and k == 0:
            places[take(0, L)] = "o"
        plan.append((npolys[(len(plan) + 2) % len(npolys)], places))
    return plan


def long_record(rng, kind, A, site, t_now, drone_id, n_passed, place):
    """16 pieces, t_now in piece n_passed: 5 * (16 - n_passed) points are compared"""
    if kind == "c":
        durs, ts = timed(rng, n_passed, MAX_PIECES - n_passed, t_now)
        return record(drone_id, ts, durs, [parked_piece(rng, place, k) for k in range(MAX_PIECES)], "capacity")
    return sample_active(rng, kind, A, site, t_now, drone_id, n_passed, MAX_PIECES - n_passed, place)


def capacity_groups(rng):
    groups = []
    for with_over in (False, True):
        egos = [new_ego(rng, e, MAX_PIECES) for e in range(3)]
        A = [np.asarray(g["cpts"]).reshape(-1, 3) for g in egos]
        sites = [site_of(e) for e in range(3)]
        # M + remaining pieces = 28: 140 rows, the largest LP;  29: 145 rows, over capacity
        recs = [long_record(rng, "l", A[0], sites[0], egos[0]["t_now"], 700, 4, 0)]
        if with_over:
            recs += [filler(rng, 1, sites, 100.0), long_record(rng, "c", None, None, 100.0, 702, 3, 2),
                     record(503, 99.0, [4.0], [parked_piece(rng, 3)], "far")]
        else:
            recs += [record(501, 99.0, [4.0], [parked_piece(rng, 1)], "far"),
                     long_record(rng, "u", A[1], sites[1], egos[1]["t_now"], 702, 4, 2), filler(rng, 3, sites, 100.0),
                     long_record(rng, "l", A[1], sites[1], egos[1]["t_now"], 704, 4, 4)]
        groups.append(finish_group("capacity", recs, egos))
    # in front of an over-capacity record stands an unsafe one
    egos = [new_ego(rng, 0, MAX_PIECES)]
    A0 = np.asarray(egos[0]["cpts"]).reshape(-1, 3)
    recs = [sample_active(rng, "u", A0, site_of(0), egos[0]["t_now"], 710, 0, 1, 0),
            long_record(rng, "c", None, None, 100.0, 711, 2, 1), record(512, 99.0, [4.0], [parked_piece(rng, 2)], "far")]
    groups.append(finish_group("early_exit", recs, egos))
    return groups


def publication_groups(rng):
    site = site_of(0)
    cpts = ego_points(rng, site, MAX_PIECES)
    t_now = 100.125
    unsafe = None
    while unsafe is None:                                      # inseparable from the first five points already
        rec = active_record(rng, "u", site, t_now, 720, 1, 2, 0)
        try:
            if all(classify(cpts[:5 * M], rec, -1, t_now)[0] == "u" for M in (1, 5, 16)):
                unsafe = rec
        except AssertionError:
            pass
    far = record(721, 99.0, [4.0], [parked_piece(rng, 0)], "far")
    groups = []
    for rec in (far, unsafe):
        for with_due in (False, True):
            rows = [(ret, M, st, due) for due in ((0, 1) if with_due else (None,)) for ret in (0, 1)
                    for M in (0, 1, 5, 16) for st in (-7, 0, 1, 2)]
            for g0 in range(0, len(rows), 16):
                egos = []
                for k, (ret, M, st, due) in enumerate(rows[g0:g0 + 16]):
                    egos.append({"drone_id": 300 + g0 + k, "t_now": t_now, "t_start": t_now + 0.0625 * (k + 1), "ret": ret,
                                 "npoly": M, "status": st, "due": due, "cpts": None, "_cpts": cpts.reshape(-1).tolist()})
                grp = finish_group("publication", [rec], egos)
                grp["cpts"] = cpts.reshape(-1).tolist()
                groups.append(grp)
    return groups


def previous_tables(rng):
    """recognisable previous contents of the two tables, one record per agent slot"""
    out = {}
    for name, base in (("prev_own", 1000), ("prev_table", 2000)):
        out[name] = [record(base + a, 50.0 + a, [0.25, 0.5], [np.full((5, 3), base + a + 0.5), np.full((5, 3), -base - a)],
                            name) for a in range(16)]
    return out


def main():
    rng = np.random.default_rng(0xF1215)
    groups = [chunk_group(rng, 1, [(8, {0: "u"}), (1, {})]), chunk_group(rng, 1, [(16, {0: "l"}), (5, {})])]
    groups += [chunk_group(rng, L, chunk_plans(rng, L, True)) for L in (63, 64, 65, 128, 130)]
    groups += [chunk_group(rng, L, chunk_plans(rng, L, False)) for L in (65, 130)]   # the short last chunk left to safe egos
    groups += capacity_groups(rng)
    groups += publication_groups(rng)
    # ---- what the fixture is there to show
    egos = [(g, e) for g in groups for e in g["egos"]]
    swarm_egos = [(g, e) for g, e in egos if g["kind"] != "publication"]
    n_safe = sum(e["safe"] for _, e in swarm_egos)
    assert 0.25 <= n_safe / len(swarm_egos) <= 0.75, (n_safe, len(swarm_egos))
    cats = "".join(e["pair_cat"] for _, e in egos)
    assert all(cats.count(c) > 0 for c in "fioluc"), {c: cats.count(c) for c in "fioluc"}
    assert {g["n_swarm"] for g in groups if g["kind"] == "chunk"} == {1, 63, 64, 65, 128, 130}
    assert {1, 8, 16} <= {e["npoly"] for g, e in egos if g["kind"] == "chunk"}
    only_unsafe_at, all_chunks_safe, foreign_at_own, later_chunk = set(), 0, 0, 0
    for g in groups:
        if g["kind"] != "chunk":
            continue
        for a, e in enumerate(g["egos"]):
            cat = e["pair_cat"]
            assert set(cat) <= set("fiolu")
            chunks = [cat[c0:c0 + 64] for c0 in range(0, len(cat), 64)]
            if cat.count("u") == 1:
                p = cat.index("u")
                if all("l" in c for c in chunks[:p // 64]) and (p % 64 <= 1 or "l" in cat[p - p % 64:p]):
                    only_unsafe_at.add(p)
                later_chunk += int(p >= 64 and "l" in cat[:64])   # the centre line behind an LP is its last pre-test
            if "u" not in cat and len(cat) > 1 and all("l" in c for c in chunks):
                all_chunks_safe += 1
            if a < len(cat) and cat[a] in "lu":
                foreign_at_own += 1
    assert only_unsafe_at == {0, 62, 63, 64, 127, 128, 129}, only_unsafe_at
    assert all_chunks_safe >= 5 and foreign_at_own >= 3 and later_chunk >= 7, (all_chunks_safe, foreign_at_own, later_chunk)
    cap = [g for g in groups if g["kind"] == "capacity"]
    assert sum(g["capacity_all"] for g in cap) >= 3 and all(g["capacity_all"] == g["capacity_sequential"] for g in cap)
    big = [(c, n) for g in cap for e in g["egos"] for c, p, r in zip(e["pair_cat"], e["pair_piece"], g["records"])
           for n in [5 * e["npoly"] + 5 * (r["n_pieces"] - p)] if c in "lu"]
    assert ("l", 140) in big and ("u", 140) in big
    assert all(e["pair_cat"].count("c") <= 1 and "0" not in e["pair_safe"][:e["pair_cat"].index("c")]
               for g in cap for e in g["egos"] if "c" in e["pair_cat"])
    early = [g for g in groups if g["kind"] == "early_exit"]
    assert [(g["capacity_all"], g["capacity_sequential"]) for g in early] == [(1, 0)]
    assert all(g["capacity_all"] == 0 for g in groups if g["kind"] in ("chunk", "publication"))
    pub = [e for g in groups if g["kind"] == "publication" for e in g["egos"]]
    assert len(pub) == 2 * 4 * 4 * 2 * 3 and {e["outcome"] for e in pub} == {0, 1, 2, 3, 4}
    assert all(len(g["egos"]) <= 16 for g in groups)
    out = {"what": "how a replan ends, restated independently (tests/golden/make_finish_fixture.py): per group one swarm table "
                   "and its egos; per ego and table place the category (f far, i inactive, o own, l lp_safe, u unsafe, c over "
                   "capacity), the piece index (-1: passed over) and the pair's verdict; the swarm verdict, the outcome "
                   "index, the ok flag, the record (n_cpts coordinates of the ego's control points, then zeros) and what the "
                   "own table and the next swarm table hold afterwards, per which of them exist",
           "tau": TAU, "outcomes": list(OUTCOMES), "capacity_rows": CAPACITY_ROWS, **previous_tables(rng), "groups": groups}
    path = os.path.join(HERE, "finish_independent.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
    largest = max(os.path.getsize(os.path.join(HERE, n)) for n in os.listdir(HERE)
                  if n.endswith(".json") and n != "finish_independent.json")
    assert os.path.getsize(path) <= largest, (os.path.getsize(path), largest)
    print(f"written {path}: {len(groups)} groups, {len(egos)} egos ({len(swarm_egos)} against a table, {n_safe} safe), "
          f"categories { {c: cats.count(c) for c in 'fioluc'} }, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
