#!/usr/bin/env python
"""An INDEPENDENT second restatement of velocityEstimationThread — the ground split, Euclidean clustering, cluster order, gated
optimal assignment against the previous frame, velocity labels and the order of input_cloud_with_velocity — written from the
reference's text (plan_env/include/plan_env/dsp_dynamic.h :70-81 ClusterFeature, :105-106, :165-305 update: the rotation,
current_position, delt_t_from_last_observation, :1476-1678; map_parameters.h:27-30) WITHOUT reading oracle/ or the kernel.  The
rotation is make_dsp_fixture.py's (itself oracle-blind).  tests/golden/velocity_independent.json holds, per sequence and frame,
the counts, the length and SHA-256 of the new-born list and a record per accepted cluster; a CPU test holds the C++ oracle to
it, a GPU test holds k_dsp_velocity to it directly (tests/test_velocity_independent.py).  Every comparison is exact: each value
is one IEEE float32 operation in all three readings.

The third-party pieces, from their published behaviour and by other algorithms than the oracle's:
  clustering   pcl::EuclideanClusterExtraction grows a cluster from each unprocessed point, in index order, by radius searches:
               its clusters are the connected components of the graph "FLANN L2 < radius", FLANN's L2 on three floats being
               diff = a - b; result += diff * diff in float (x, y, z, each operation rounded) and the radius
               (float)(tolerance * tolerance) with tolerance = (double)(2 * 0.15f).  Here: the full float32 distance matrix and
               scipy.sparse.csgraph.connected_components.  A cluster is listed when its first (smallest) index is met, its
               indices are sorted; 5 <= size <= 10000, points of rejected components are in no list at all.
  order        std::sort(clusters.rbegin(), clusters.rend(), size <).  For at most 16 elements libstdc++'s std::sort never
               enters the introsort loop (it needs last - first > 16) and runs __insertion_sort alone; that moves an element
               only past elements that compare strictly greater (comp(val, *prev), comp(*i, *first): both strict), so it is
               stable.  In the REVERSED view the input reads in descending extraction index and comes out ascending by size,
               equal sizes still in descending extraction index; read forwards again that is descending by size, equal sizes in
               ASCENDING extraction index = seed order.  Here: sorted by (-size, seed), asserted to be exactly that derivation's
               result by running the insertion sort on the reversed list.  Beyond 16 clusters the tie order is libstdc++'s
               introsort's: those frames have pairwise distinct sizes, or are marked `tie_free` and compared with the blocks of
               equal-sized clusters sorted by their bytes (the real std::sort holds the order itself in test_velocity_estimation).
  assignment   Munkres' role: an optimal assignment of the square problem padded with a constant; a row assigned to a gated
               pair is no match.  Here: exhaustive enumeration up to 7 x 7, scipy.optimize.linear_sum_assignment in float64
               above.  What must be unique is the OUTCOME (the set of assigned un-gated pairs; gated pairs all cost 7500 and
               swap freely).  The generator asserts: best total versus the best total of any assignment with another outcome
               differs by >= 1.0 for problems up to 20 x 20 (found by enumeration, or by forbidding each optimal pair and forcing
               each other un-gated pair in turn and re-solving).  Why 1.0 is enough for a float32 solver: costs reach 7500, where
               a float32 ulp is 4.9e-4; a potential takes at most N updates in each of N phases, each off by at most half an ulp:
               below 0.1 for N = 20, so 1.0 leaves a factor of 10.  Larger problems (64 rows) have every new cluster within the
               gate of exactly one old cluster and every old one of at most one new: the outcome is forced.
  arithmetic   centres: float32 sums in ascending index order, one division by (float)point_num; distance: sqrtf of the float32
               sum in the text's order; cost: d / 1.5f * 1000.f; velocity: one float32 division by the float32 delt_t; speed:
               sqrtf of the separately rounded sum; defaults -10000 and the constant intensity 0.55.
To keep "exact" honest the generator asserts that nothing else is marginal: centre z >= 1e-3 from 1.5, centre distances >= 1e-3
from 1.5, speeds >= 1e-3 from 5 — and that the deliberately exact cases are what they claim (world coordinates returned by the
forward transform, both evaluations of every tolerance_strict_3d pair).
Run from the repo root:   python tests/golden/make_velocity_fixture.py
"""
import base64
import hashlib
import itertools
import json
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import helpers  # noqa: E402  (the INPUTS: shared with the tests, which never import this script)
from make_dsp_fixture import DSP  # noqa: E402  (rotateVectorByQuaternion, oracle-blind)

f32 = np.float32
VRES = f32(0.15)                  # static float voxel_filtered_resolution = 0.15
R2 = helpers.vel_r2()
DIST_GATE, NUM_GATE, VMAX = f32(1.5), 100, f32(5.0)
GATED = f32(DIST_GATE * f32(5000.0))
INTENSITY = f32(0.55)
DEFAULT = f32(-10000.0)
MARGINS = {"centre_z": np.inf, "centre_distance": np.inf, "speed": np.inf, "assignment": np.inf}


def rotate_all(p, q):
    """rotateVectorByQuaternion (:1396-1418) on every point: Eigen's quaternion product q * (0, v) * q^-1 in float, each
    operation rounded — vectorised here, and held to make_dsp_fixture's scalar restatement on a sample."""
    w, x, y, z = [f32(c) for c in q]

    def mul(a, b):
        aw, ax, ay, az = a
        bw, bx, by, bz = b
        return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx)
    n2 = f32(f32(f32(x * x) + f32(y * y)) + f32(z * z)) + f32(w * w)
    inv = (f32(w / n2), f32(-x / n2), f32(-y / n2), f32(-z / n2))
    zero = np.zeros(len(p), f32)
    r = mul(mul((w, x, y, z), (zero, p[:, 0], p[:, 1], p[:, 2])), inv)
    out = np.stack([r[1], r[2], r[3]], 1).astype(f32)
    assert out.dtype == f32
    for i in range(0, len(p), max(1, len(p) // 7)):
        want = DSP.rotate(None, p[i], q)
        assert all(f32(want[k]).tobytes() == out[i, k].tobytes() for k in range(3)), (i, want, out[i])
    return out


def components(pts):
    """Connected components of "float32 squared L2, x then y then z, separately rounded, strictly below r2"; each as its
    ascending index list, listed by smallest index."""
    m = len(pts)
    rows, cols = [], []
    for lo in range(0, m, 512):
        blk = pts[lo:lo + 512]
        d = blk[:, None, 0] - pts[None, :, 0]
        s = d * d
        d = blk[:, None, 1] - pts[None, :, 1]
        t = d * d
        s = s + t
        d = blk[:, None, 2] - pts[None, :, 2]
        t = d * d
        s = s + t
        assert s.dtype == f32
        r, c = np.nonzero(s < R2)
        rows.append(r + lo)
        cols.append(c)
    g = csr_matrix((np.ones(sum(len(r) for r in rows), np.int8), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m))
    _, lab = connected_components(g, directed=False)
    groups = {}
    for i, l in enumerate(lab):
        groups.setdefault(int(l), []).append(i)
    return sorted(groups.values(), key=lambda g_: g_[0])


def sort_clusters(cl):
    """std::sort(rbegin, rend, size <): (-size, seed) — and, up to 16 clusters, asserted against the insertion sort the
    docstring derives it from."""
    out = sorted(cl, key=lambda c: (-len(c), c[0]))
    sizes = [len(c) for c in out]
    tie_beyond_16 = len(cl) > 16 and len(set(sizes)) != len(sizes)
    if len(cl) <= 16:
        rev = list(reversed(cl))                       # the reversed view
        for i in range(1, len(rev)):                   # libstdc++ __insertion_sort, comp = size <
            v = rev[i]
            if len(v) < len(rev[0]):
                rev[1:i + 1] = rev[0:i]
                rev[0] = v
            else:
                j = i
                while len(v) < len(rev[j - 1]):
                    rev[j] = rev[j - 1]
                    j -= 1
                rev[j] = v
        assert list(reversed(rev)) == out
    return out, tie_beyond_16


def outcome_of(rows, cols, gate):
    return frozenset((int(r), int(c)) for r, c in zip(rows, cols) if gate[r, c])


def assign(cost, gate):
    """The optimal assignment's outcome (row -> col over un-gated pairs) and the margin to the best other outcome."""
    R, C = cost.shape
    c64 = cost.astype(np.float64)
    n = max(R, C)
    if n <= 7:
        pad = np.zeros((n, n))
        pad[:R, :C] = c64
        best = {}
        for perm in itertools.permutations(range(n)):
            tot = sum(pad[r, perm[r]] for r in range(n))
            oc = frozenset((r, perm[r]) for r in range(R) if perm[r] < C and gate[r, perm[r]])
            if oc not in best or tot < best[oc]:
                best[oc] = tot
        oc0 = min(best, key=best.get)
        others = [t for o, t in best.items() if o != oc0]
        return oc0, (min(others) - best[oc0]) if others else np.inf
    rr, cc = linear_sum_assignment(c64)
    tot0, oc0 = c64[rr, cc].sum(), outcome_of(rr, cc, gate)
    forced = all(gate[r].sum() <= 1 for r in range(R)) and all(gate[:, c].sum() <= 1 for c in range(C))
    if n > 20:
        assert forced, "beyond 20 x 20 every cluster is within the gate of exactly one old cluster"
        assert oc0 == frozenset((int(r), int(c)) for r, c in zip(*np.nonzero(gate)))
        return oc0, None
    margin = np.inf
    for r, c in zip(*np.nonzero(gate)):
        if (r, c) in oc0:
            alt = c64.copy()
            alt[r, c] = 1e9
            a, b = linear_sum_assignment(alt)
            margin = min(margin, alt[a, b].sum() - tot0)
        else:
            sub = np.delete(np.delete(c64, r, 0), c, 1)      # (r, c) forced: the rest assigns min(R, C) - 1 pairs
            tot = c64[r, c]
            if sub.size:
                a, b = linear_sum_assignment(sub)
                tot += sub[a, b].sum()
            margin = min(margin, tot - tot0)
    return oc0, margin


def greedy(cost, gate):
    """row-wise nearest free un-gated column — what a greedy matcher would do"""
    taken, oc = set(), set()
    for r in range(cost.shape[0]):
        cand = [(cost[r, c], c) for c in range(cost.shape[1]) if gate[r, c] and c not in taken]
        if cand:
            c = min(cand)[1]
            taken.add(c)
            oc.add((r, c))
    return frozenset(oc)


class Reading:
    def __init__(self):
        self.last_pose = None
        self.last = []                    # clusters_feature_vector_dynamic_last: (cx, cy, cz, n)
        self.greedy_differs = 0

    def frame(self, points, pos, quat, stamp, note):
        pos = [f32(v) for v in pos]
        if self.last_pose is None:        # the function statics of update(): initialised by the first call
            self.last_pose = (pos, float(stamp))
        assert not any(abs(float(f32(c))) > 1.001 for c in quat)
        dt = f32(float(stamp) - self.last_pose[1])
        assert all(abs(float(f32(pos[i] - self.last_pose[0][i]))) <= 10.0 for i in range(3)) and 0 <= dt <= 10
        self.last_pose = (pos, float(stamp))
        points = np.asarray(points, f32).reshape(-1, 3)
        assert len(points)
        rot = rotate_all(points, quat)
        world = np.stack([rot[:, i] + pos[i] for i in range(3)], 1)
        assert world.dtype == f32
        ng = np.nonzero(world[:, 2] > VRES)[0]               # strict: z == 0.15f is ground
        gr = np.nonzero(~(world[:, 2] > VRES))[0]
        P = world[ng]
        dyn, info, static_pts, tie_free = [], [], [], False
        if len(ng):
            comps = [c for c in components(P) if 5 <= len(c) <= 10000]
            comps, tie_free = sort_clusters(comps)
            for c in comps:
                s = [f32(0)] * 3
                for i in c:
                    s = [f32(s[k] + P[i, k]) for k in range(3)]
                ctr = [f32(s[k] / f32(len(c))) for k in range(3)]
                is_dyn = not (len(c) > 200 or float(ctr[2]) > 1.5)
                MARGINS["centre_z"] = min(MARGINS["centre_z"], abs(float(ctr[2]) - 1.5))
                rec = {"idx": c, "n": len(c), "seed": int(ng[c[0]]), "ctr": ctr, "dyn": is_dyn, "v": [DEFAULT] * 3}
                info.append(rec)
                if is_dyn:
                    dyn.append(rec)
                else:
                    static_pts.extend(c)
            matched = 0
            if self.last and dyn and float(dt) > 0.00001 and float(dt) < 10.0:
                R, C = len(dyn), len(self.last)
                cost, gate = np.zeros((R, C), f32), np.zeros((R, C), bool)
                for r in range(R):
                    for c in range(C):
                        a, b = dyn[r]["ctr"], self.last[c]
                        d = [f32(a[k] - b[k]) for k in range(3)]
                        dist = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
                        MARGINS["centre_distance"] = min(MARGINS["centre_distance"], abs(float(dist) - 1.5))
                        if abs(dyn[r]["n"] - b[3]) > NUM_GATE or dist >= DIST_GATE:
                            cost[r, c] = GATED
                        else:
                            gate[r, c] = True
                            cost[r, c] = f32(f32(dist / DIST_GATE) * f32(1000.0))
                oc, margin = assign(cost, gate)
                if margin is not None:
                    MARGINS["assignment"] = min(MARGINS["assignment"], margin)
                    assert margin >= 1.0, (note, margin)
                if greedy(cost, gate) != oc:
                    self.greedy_differs += 1
                for r, c in oc:
                    b = self.last[c]
                    v = [f32(f32(dyn[r]["ctr"][k] - b[k]) / dt) for k in range(3)]
                    sp = f32(np.sqrt(f32(f32(f32(v[0] * v[0]) + f32(v[1] * v[1])) + f32(v[2] * v[2]))))
                    MARGINS["speed"] = min(MARGINS["speed"], abs(float(sp) - 5.0))
                    if sp > VMAX:
                        v = [f32(0)] * 3
                    dyn[r]["v"] = v
                    matched += 1
            born = []
            for rec in dyn:
                for i in rec["idx"]:
                    born.append([P[i, 0], P[i, 1], P[i, 2]] + rec["v"] + [INTENSITY])
        else:
            matched = 0
            born = []
        for i in gr:
            born.append(list(world[i]) + [f32(0)] * 4)
        for i in static_pts:
            born.append(list(P[i]) + [f32(0)] * 4)
        self.last = [(r["ctr"][0], r["ctr"][1], r["ctr"][2], r["n"]) for r in dyn]      # emptied when m == 0 too
        born = np.asarray(born, f32).reshape(-1, 7)
        return {"world": world, "born": born, "counts": [len(info), len(dyn), matched], "info": info, "tie_free": tie_free,
                "n_ground": len(gr)}


def bits(a):
    return np.ascontiguousarray(a, f32).tobytes()


def sha(b):
    return base64.b64encode(hashlib.sha256(b).digest()).decode()      # SHA-256, base64: the file has a size limit


def input_hash(fr):
    return sha(bits(fr["points"]) + bits(fr["pos"]) + bits(fr["quat"]) + np.float64(fr["stamp"]).tobytes())


def cluster_record(rec):
    hx = lambda v: "".join("%08x" % int(f32(x).view(np.uint32)) for x in v)
    v = rec["v"]
    lab = "-" if all(x == DEFAULT for x in v) else hx(v)
    return "%d,%d,%s,%s,%s" % (rec["n"], rec["seed"], hx(rec["ctr"]), lab, "D" if rec["dyn"] else "S")


def run_sequence(seq, with_records=True, clamp=None):
    rd = Reading()
    frames = []
    for k, fr in enumerate(seq["frames"]):
        if clamp is not None:
            fr = dict(fr, points=fr["points"][:clamp])
        out = rd.frame(fr["points"], fr["pos"], fr["quat"], fr["stamp"], (seq["branch"], k))
        if "world" in fr and clamp is None:     # identity attitude: the forward transform returns the intended coordinates
            assert bits(out["world"]) == bits(fr["world"]), (seq["branch"], k)
        sizes_d = [r["n"] for r in out["info"] if r["dyn"]]
        sizes_s = [r["n"] for r in out["info"] if not r["dyn"]]
        born = out["born"]
        if out["tie_free"]:
            born = helpers.vel_canonical_born(born, sizes_d, out["n_ground"], sizes_s)
        e = {"n": int(len(fr["points"])), "in": input_hash(fr), "counts": out["counts"], "n_born": int(len(born)),
             "born": sha(bits(born))}
        if out["tie_free"]:
            rle = lambda s: [[k, len(list(g))] for k, g in itertools.groupby(s)]
            e["tie_free"] = [rle(sizes_d), out["n_ground"], rle(sizes_s)]
        recs = [cluster_record(r) for r in out["info"]]
        if with_records and len(recs) <= 16:      # size, seed (input index), centre bits, label bits (-: the defaults), D / S
            e["clusters"] = recs
        frames.append((e, out))
    return frames, rd


def check_branch(seq, frames, rd):
    """what each named case must actually be"""
    b = seq["branch"]
    C = [e["counts"] for e, _ in frames]
    O = [o for _, o in frames]
    sizes = lambda o: [r["n"] for r in o["info"]]
    if b == "size_4_dropped_5_kept":
        assert all(sizes(o) == [9, 5] for o in O) and all(e["n_born"] == e["n"] - 4 for e, _ in frames)
    elif b == "size_200_dynamic_201_static":
        assert all([(r["n"], r["dyn"]) for r in o["info"]] == [(201, False), (200, True), (10, True)] for o in O)
    elif b == "centre_above_1p5_static":
        assert all([r["dyn"] for r in o["info"]] in ([True, False], [False, True]) and sizes(o) == [18, 18] for o in O)
    elif b == "ground_split_on_world_z":
        v = f32(0.15)
        up = np.nextafter(v, f32(1))
        for k, o in enumerate(O):
            z = o["world"][:, 2]
            if k % 2 == 0:
                assert (z == v).sum() == 6 and (z == up).sum() == 6
                assert sizes(o) == [8, 6], sizes(o)
            else:
                assert ((z < v) & (z > v - f32(2e-7))).sum() == 6 and ((z > v) & (z < v + f32(2e-7))).sum() == 6
                assert sorted((r["n"], r["dyn"]) for r in o["info"]) == [(6, True), (8, False), (12, False), (12, True)]
    elif b == "all_ground":
        assert C[1] == [0, 0, 0] and C[2] == [1, 1, 0] and frames[1][0]["n_born"] == frames[1][0]["n"]
    elif b == "no_accepted_cluster":
        assert C[1] == [0, 0, 0] and frames[1][0]["n_born"] == 6 and C[2] == [1, 1, 0]
    elif b == "tolerance_strict_axis":
        assert all(sorted(sizes(o)) == [5] * 6 + [10] * 3 for o in O)
    elif b == "tolerance_strict_3d":
        for i, (a, p) in enumerate(seq["pairs"]):
            s, u = helpers.vel_d2_separate(p, a), helpers.vel_d2_fused(p, a)
            assert all(f32(p[k] - a[k]) != 0 for k in range(3))
            assert (s < R2 <= u) if i < 8 else (u < R2 <= s), (i, s, u)
        for k, o in enumerate(O):                                            # the verdict of the separately rounded sum
            assert sizes(o) == ([10] * 8 if k % 2 == 0 else [5] * 16)
    elif b.startswith("chain_"):
        assert all(180 in sizes(o) for o in O)
        if b == "chain_across_trips":
            for o, (e, _) in zip(O, frames):
                idx = np.sort(np.nonzero(o["world"][:, 2] > VRES)[0])
                ch = [r for r in o["info"] if r["n"] == 180][0]
                inp = idx[ch["idx"]]
                assert inp.min() < 1024 < 2048 < inp.max() and min(ch["idx"]) < 1024 < 2048 < max(ch["idx"])
    elif b == "interleaved_combs_stay_two":
        assert all(sizes(o) == [77, 69] for o in O)
    elif b.startswith("cloud_"):
        assert all(e["n"] == int(b[6:]) for e, _ in frames) and all(c[2] == 3 for c in C[1:])
    elif b == "more_new_than_old":
        assert [c[1:] for c in C] == [[3, 0], [4, 3], [5, 4]]
    elif b == "fewer_new_than_old":
        assert [c[1:] for c in C] == [[5, 0], [3, 3], [2, 2]]
    elif b == "point_num_gate_100_in_101_out":
        assert [c[1:] for c in C] == [[2, 0], [2, 1], [2, 1]]
    elif b == "distance_gate_in_and_out":
        assert [c[1:] for c in C] == [[2, 0], [2, 1], [2, 1]]
    elif b == "faster_than_5_is_zeroed_but_matched":
        assert [c[1:] for c in C] == [[2, 0], [2, 2], [2, 2], [2, 2]]
        assert all(x == 0 for x in O[1]["info"][0]["v"]) and all(x == 0 for x in O[2]["info"][0]["v"])
        assert O[3]["info"][0]["v"][0] > 1
    elif b in ("dt_too_small", "dt_10_or_more"):
        k = 2 if b == "dt_too_small" else 1
        assert C[k] == [2, 2, 0] and C[k + 1] == [2, 2, 2]
        assert abs(float(O[k + 1]["info"][0]["v"][0]) * (seq["frames"][k + 1]["stamp"] - seq["frames"][k]["stamp"]) - 0.25) < 0.01
    elif b == "greedy_differs_from_optimum":
        assert rd.greedy_differs >= 6 and all(c == [4, 4, 4] for c in C[1:])
    elif b == "assigned_to_a_gated_pair_is_no_match":
        assert [c[1:] for c in C] == [[1, 0], [1, 0], [2, 1], [2, 1]]
    elif b == "random_swarm":
        assert max(c[1] for c in C) >= 17 and len({c[1] for c in C}) > 1
    elif b == "sixty_four_dynamic":
        assert all(c[:2] == [64, 64] for c in C) and all(c[2] == 64 for c in C[1:]) and all(e["n"] == 320 for e, _ in frames)
    elif b == "tie_order_up_to_16":
        assert all(c[0] == 16 for c in C)
    elif b == "rotated_moving_sensor":
        assert all(c[:2] == [4, 3] for c in C) and all(c[2] == 3 for c in C[1:])
    else:
        raise AssertionError("unnamed branch " + b)


def main():
    seqs = helpers.velocity_fixture_inputs()
    out = {"about": "tests/golden/make_velocity_fixture.py: velocityEstimationThread, second reading", "r2_bits": "%08x" % int(R2.view(np.uint32)),
           "sequences": [], "capacity": {}}
    for seq in seqs:
        frames, rd = run_sequence(seq)
        check_branch(seq, frames, rd)
        out["sequences"].append({"branch": seq["branch"], "frames": [e for e, _ in frames]})
        print("%-40s" % seq["branch"], [e["counts"] for e, _ in frames])
    for name, frames_in, max_points in helpers.velocity_capacity_inputs():
        clamp = max_points if frames_in[0]["points"].shape[0] > max_points else None
        frames, _ = run_sequence({"branch": name, "frames": frames_in}, with_records=False, clamp=clamp)
        out["capacity"][name] = {"max_points": max_points, "frames": [e for e, _ in frames]}
        print("%-40s" % ("capacity " + name), [e["counts"] for e, _ in frames])
    for k, v in MARGINS.items():
        print("smallest margin %-16s %.6g" % (k, v))
        assert v >= (1.0 if k == "assignment" else 1e-3), k
    out["min_assignment_margin"] = float(MARGINS["assignment"])
    out["min_decision_margins"] = {k: float(v) for k, v in MARGINS.items() if k != "assignment"}
    path = os.path.join(HERE, "velocity_independent.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
