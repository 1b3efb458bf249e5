#!/usr/bin/env python
"""DSPMap::update branch by branch: the INDEPENDENT reading of tests/golden/make_dsp_fixture.py (class DSP, written from the
reference's text plan_env/include/plan_env/dsp_dynamic.h without reading oracle/ or the kernels) run on hand-built particle
stores.  The inputs — stores, clouds, poses, cursors, small tables — come from tests/helpers.py (dsp_case_inputs, SplitMix64) and
are recorded here by SHA-256 only; this file writes the EXPECTED results to tests/golden/dsp_cases_independent.json:

  per case and update   the return value, every slot's flag, velocity and position (float bits), weight, the table cursors, the
                        observation tables (count, x / y / z / C_k / length per stored observation, max_length), the per-voxel
                        object numbers and the counters voxel_full / pyramid_full / moved_out since the store was injected
  per case              its branch labels — DERIVED below from the reading's own event trace and counters, never from the
                        builder's intent: a label whose predicate does not hold goes to "unclaimed" with the reason
  "margins"             the smallest margin of every decision a tolerance could touch, ASSERTED here: weights, C_k and object
                        numbers are compared to rtol 1e-4 (this interpreter's exp / sin against glibc's expf / sinf), so no case may
                        let that decide anything — removal at 1e-3, every acc_o > acc_n of the resampler, the truncation
                        (int)(16 p_static) and the occlusion test keep 1e-3 relative; every FOV / pyramid dot product is exactly 0
                        by construction or at least 1e-5 |p| from 0; every float truncation in voxel_index is deliberate
                        (searched, or an exact cell boundary) or at least 1e-4 of a cell from an integer
  "exact" per update    no particle has been listed in a pyramid since the store was injected: no normal-PDF entry has entered any
                        weight or C_k, which are then plain IEEE arithmetic on the inputs.  The tests hold them with NO tolerance, so
                        there is nothing for a margin to protect and the weight-dependent margins are not asked of such an update
                        (equal new-born weights make exact resampler ties: more than 14 new-borns into an empty voxel)

Arrays are stored as base85(zlib(raw little-endian bytes)), the almost empty ones (flags, observation counts, object numbers) as
the gaps between the flat indices of their non-zero entries and those entries; velocity, position and weight of the live slots only.
Run from the repo root:   python tests/golden/make_dsp_cases_fixture.py        (a few seconds)
"""
import base64
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from helpers import DSP_CASE_GRIDS, DSP_CASE_LABELS as LABELS, dsp_case_inputs, dsp_case_sha256, dsp_case_tables  # noqa: E402
from make_dsp_fixture import DSP  # noqa: E402

f32 = np.float32

NOT_BUILT = {}      # label -> why no case could be built for it


def pack(a):
    return base64.b85encode(zlib.compress(np.ascontiguousarray(a).tobytes(), 9)).decode("ascii")


def sparse(a):
    """the non-zero entries of an array: [the gaps between their flat indices (int32), their values], each packed"""
    flat = np.ascontiguousarray(a).ravel()
    nz = np.flatnonzero(flat)
    return [pack(np.diff(nz, prepend=0).astype(np.int32)), pack(flat[nz])]


def record(g, ok, counters):
    st = g.store
    occ = st[:, :, 0] > f32(0.1)
    assert np.array_equal(g.maxlen >= 0, g.nobs > 0)      # max_length is set exactly where an observation was binned
    pyr = np.flatnonzero(g.nobs > 0)
    rows = [g.pc[i, :g.nobs[i]] for i in pyr]
    live = st[:, :, 1:8][occ].T      # [7][n]: velocity, position and weight of every live slot, in (voxel, slot) order
    return {"ok": int(ok), "n_particles": int(occ.sum()), "flags": sparse(st[:, :, 0]), "live": pack(live),
            "cursors": [int(g.pseq), int(g.vseq), int(g.rseq)], "nobs": sparse(g.nobs),
            "obs": pack(np.concatenate(rows).T if rows else np.zeros((5, 0), f32)), "maxlen": pack(g.maxlen[pyr]),
            "obj": sparse(g.obj), "counters": list(counters), "exact": bool(g.weights_exact)}


def run_case(case, tables):
    g = DSP(tables, grid=DSP_CASE_GRIDS[case.grid], trace=True)
    assert g.set_state(case.store, case.last_pos, case.last_stamp, case.cursors) == 0, case.name
    recs, traces, stores, counters = [], [], [case.store.copy()], [0, 0, 0]
    for u in case.updates:
        g.trace = []
        ok = g.update(u["points"], u["labels"], u["pos"], u["quat"], u["stamp"])
        if not ok:
            assert not g.trace
        counters[0] += sum(e["voxel_full"] for e in g.trace)
        counters[1] += sum(e["pyramid_full"] for e in g.trace)
        counters[2] += sum(e["kind"] == "out" for e in g.trace)
        recs.append(record(g, ok, counters))
        traces.append(g.trace)
        stores.append(g.store.copy())
        g.obj[:, 4:] = 0      # the consumer (getOccupancyMapWithFutureStatus, :454-476) clears the future status after reading it
    return g, recs, traces, stores


def derive_labels(case, g, recs, traces, stores, all_cases):
    """{label: bool} for every label this case could claim — from the trace, the marks and the results only"""
    tr = [e for t in traces for e in t]
    t0 = traces[0] if traces else []
    m = g.marks
    V, S = g.V, g.S
    h = (float(g.hx), float(g.hy), float(g.hz))
    out = {}
    placed = [e for e in t0 if e["kind"] == "move" and e["slot"] is not None]
    arrivals = {}
    for e in t0:
        if e["kind"] == "move":
            arrivals.setdefault(e["dst_voxel"], []).append(e)
    idx = {id(e): i for i, e in enumerate(t0)}
    later_src = lambda e, v, p: any(x["src"] == (v, p) for x in t0[idx[id(e)] + 1:])
    st1 = stores[1] if len(stores) > 1 else None

    out["stay_in_fov"] = any(e["kind"] == "stay" and e["listed"] for e in t0)
    out["stay_outside_fov"] = any(e["kind"] == "stay" and e["pyramid"] < 0 and float(st1[e["src"]][7]) == e["w_before"] for e in t0)
    out["mover_into_unswept_voxel"] = any(e["dst_voxel"] > e["src"][0] and (e["dst_voxel"], e["slot"]) in g.skipped_arrivals and
                                          not later_src(e, e["dst_voxel"], e["slot"]) for e in placed) and len(traces) == 1
    out["mover_into_swept_voxel"] = any(e["dst_voxel"] < e["src"][0] for e in placed)
    out["arrivals_before_turn_see_departing_occupants"] = any(
        e["voxel_full"] and len(e["dst_occupied"]) == S and all(any(x["src"] == (e["dst_voxel"], s) and x["kind"] != "stay" for x in t0[idx[id(e)] + 1:])
                                                              for s in e["dst_occupied"]) and
        [x["slot"] for x in arrivals[e["dst_voxel"]] if x["src"][0] > e["dst_voxel"]][:2] == [0, 1] for e in t0 if e["kind"] == "move")
    out["lowest_empty_slot_with_holes"] = any(any(s < e["slot"] for s in e["dst_occupied"]) and any(s > e["slot"] for s in e["dst_occupied"]) and
                                              e["slot"] == min(set(range(S)) - set(e["dst_occupied"])) for e in placed)
    out["arrivals_in_key_order_from_three_sources"] = any(
        len({e["src"][0] for e in a}) >= 3 and [e["slot"] for e in a] == list(range(len(a))) and
        any(e["src"][0] < v for e in a) and any(e["src"][0] > v for e in a) for v, a in arrivals.items())
    out["fifteen_arrivals_one_phase"] = any(len(a) == 15 and all(e["src"][0] < v for e in a) and [e["voxel_full"] for e in a] == [False] * 14 + [True]
                                            for v, a in arrivals.items())
    out["twenty_eight_arrivals_two_phases"] = any(
        len(a) >= 28 and any(e["voxel_full"] and e["src"][0] < v for e in a) and any(e["voxel_full"] and e["src"][0] > v for e in a) and
        any(not e["voxel_full"] and e["src"][0] < v for e in a) and any(not e["voxel_full"] and e["src"][0] > v for e in a)
        for v, a in arrivals.items())
    faces = set()
    for e in tr:
        if e["kind"] == "out":
            for ax in range(3):
                if e["pos"][ax] >= h[ax]:
                    faces.add("+" + "xyz"[ax])
                if e["pos"][ax] <= -h[ax]:
                    faces.add("-" + "xyz"[ax])
    out["leaves_through_each_face"] = len(faces) == 6 and recs[-1]["counters"][2] == sum(e["kind"] == "out" for e in tr)
    out["leaving_slot_frees_at_own_turn"] = any(
        e["kind"] == "out" and any(x["kind"] == "move" and x["voxel_full"] and x["dst_voxel"] == e["src"][0] for x in t0[:idx[id(e)]]) and
        any(x["kind"] == "move" and (x["dst_voxel"], x["slot"]) == e["src"] for x in t0[idx[id(e)] + 1:]) for e in t0)
    out["exactly_on_the_bound"] = ({e["pos"][0] for e in t0 if e["kind"] == "out"} == {h[0], -h[0]} and any(e["kind"] == "stay" for e in t0))
    for ax in "xyz":
        out["one_ulp_below_the_upper_bound_" + ax] = (
            m.get("axis_index_equals_size_" + ax, 0) > 0 and
            any(e["pos"]["xyz".index(ax)] < h["xyz".index(ax)] and e["pos"]["xyz".index(ax)] > 0.99 * h["xyz".index(ax)] and
                e["kind"] == ("out" if ax == "z" else "move") for e in t0))
    out["pyramid_full_stay"] = any(e["kind"] == "stay" and e["pyramid_full"] for e in t0)
    out["pyramid_full_mover"] = any(e["kind"] == "move" and e["pyramid_full"] and
                                    any(x["kind"] == "move" and (x["dst_voxel"], x["slot"]) == e["frees"] for x in t0[idx[id(e)] + 1:]) for e in t0)
    # the cascade's length, measured: a vanish has depth 1 + the depth of the vanish whose freed slot — the only empty one of its
    # voxel — was taken by an arrival that stands in this vanish's pyramid list
    listed_by = {(e["dst_voxel"], e["slot"]): e for e in t0 if e["listed"]}
    depth_of, freed_by = {}, {}
    for e in t0:
        if e["pyramid_full"]:
            d = 1
            for entry in e["list_at_vanish"]:
                y = listed_by.get(entry)
                if y is not None and y["kind"] == "move" and len(y["dst_occupied"]) == S - 1 and entry in freed_by and idx[id(freed_by[entry])] < idx[id(y)]:
                    d = max(d, depth_of[id(freed_by[entry])] + 1)
            depth_of[id(e)] = d
            freed_by[e["frees"]] = e
    longest = max(depth_of.values()) if depth_of else 0
    for d, lab in ((1, "cascade_1"), (2, "cascade_2"), (3, "cascade_3"), (5, "cascade_at_the_limit"), (6, "cascade_one_over_the_limit")):
        out[lab] = longest == d
    zd = g.zero_dots
    out["on_a_boundary_plane"] = (any(p[1] == 0 and p[2] != 0 for p in zd) and any(p[2] == 0 and p[1] != 0 for p in zd) and
                                  any(p[1] == 0 and p[2] == 0 for p in zd) and sum(e["listed"] for e in t0) >= 3)
    out["on_the_fov_edge"] = (any(p[1] > 0 and p[2] != 0 for p in zd) and any(p[1] < 0 and p[2] != 0 for p in zd) and
                              sum(e["listed"] for e in t0) >= 4 and sum(e["kind"] == "stay" and e["pyramid"] < 0 for e in t0) >= 2)
    cand = sum(e["kind"] == "move" or (e["kind"] == "stay" and e["pyramid"] >= 0) for e in t0)
    out["candidate_pool_exactly_2V"] = cand == 2 * V and not any(e["kind"] == "out" for e in t0) and all(e["kind"] == "move" for e in t0)
    out["candidate_pool_one_over"] = cand == 2 * V + 1 and all(e["kind"] == "move" for e in t0)
    binned = {}
    for p in g.point_pyr:
        if p >= 0:
            binned[p] = binned.get(p, 0) + 1
    for n in (98, 99, 100, 150):
        full = max(binned, key=binned.get) if binned else 0
        # past the cap, max_length must come from a DROPPED point: longer than every kept row
        out["observations_%d_in_one_pyramid" % n] = bool(binned) and binned[full] == n and int(g.nobs[full]) == min(n, 99) and (
            n <= 99 or float(g.pc[full, :99, 4].max()) < float(g.maxlen[full]))
    pp = g.point_pyr
    out["observations_across_trip_boundaries"] = len(pp) > 512 and pp[255] >= 0 and len({pp[k] for k in (255, 256, 257, 511, 512)}) == 1
    trip = [c for c in all_cases if c.name == "observations_across_trip_boundaries"]
    out["observations_in_shuffled_input_order"] = bool(trip) and case is not trip[0] and len(case.updates) == 1 and (
        sorted(map(tuple, case.updates[0]["points"].tolist())) == sorted(map(tuple, trip[0].updates[0]["points"].tolist())) and
        not np.array_equal(case.updates[0]["points"], trip[0].updates[0]["points"]) and int(g.nobs.max()) == 5)
    out["empty_cloud_reuses_born_list"] = m.get("empty_cloud_reuses_born_list", 0) > 0 and recs[-1]["cursors"] != recs[0]["cursors"]
    if len(case.updates) == 2 and recs[0]["ok"] == 0 and recs[1]["ok"] == 1:
        u = case.updates[0]
        dt = f32(u["stamp"] - case.last_stamp)
        out["rejected_quaternion"] = any(abs(float(f32(q))) > 1.001 for q in u["quat"])
        out["rejected_negative_dt"] = bool(dt < 0)
        out["rejected_dt_above_10"] = bool(dt > 10)
        out["rejected_jump_above_10m"] = any(abs(float(f32(a) - f32(b))) > 10 for a, b in zip(u["pos"], case.last_pos))
        assert np.array_equal(stores[1], stores[0]) or np.array_equal(stores[1][:, :, :8], stores[0][:, :, :8])
    out["occluded_particle_keeps_weight"] = m.get("occluded", 0) > 0 and any(
        e["listed"] and float(stores[1][e["dst_voxel"], e["slot"], 7]) == e["w_before"] for e in t0)
    out["max_length_unset"] = m.get("max_length_unset", 0) > 0
    out["neighbourhood_of_4"] = m.get("listed_in_pyramid_with_4_neighbours", 0) > 0
    out["neighbourhood_of_6"] = m.get("listed_in_pyramid_with_6_neighbours", 0) > 0
    for k_, lab in (("pdf_clamp_low", "pdf_clamp_low"), ("pdf_clamp_high", "pdf_clamp_high"), ("ck_over_two_lists", "ck_over_two_lists"),
                    ("split_nan", "split_nan"), ("split_all_static", "split_all_static"), ("split_all_dynamic", "split_all_dynamic"),
                    ("split_mixed_band", "split_mixed_band"), ("split_counts_flag_7", "split_counts_flag_7"),
                    ("split_passes_over_flag_15", "split_passes_over_flag_15"), ("born_labelled", "labelled_dynamic"),
                    ("born_random_unmatched", "unmatched_label"), ("born_random_p_ge_16", "random_from_particle_16"),
                    ("point_outside_map", "point_outside_the_map"), ("newborn_dropped_voxel_full", "addAParticle_into_13_of_14"),
                    ("newborn_dropped_voxel_of_newborns_only", "more_than_14_newborns_into_an_empty_voxel"),
                    ("resample_no_empty_slot_adds_weight", "resample_no_empty_slot_adds_weight"),
                    ("resample_copy_into_slot_freed_in_this_pass_or_below", "resample_copies_into_slots_freed_in_the_pass"),
                    ("future_outside_for_some_slices_only", "future_outside_for_some_slices"), ("mean_velocity_excludes_newborns", "mean_velocity_excludes_newborns"),
                    ("mean_velocity_no_old_particles", "mean_velocity_no_old_particles")):
        out[lab] = m.get(k_, 0) > 0
    out["low_intensity_zero_velocity"] = m.get("born_labelled_low_intensity", 0) > 0 and m.get("born_random_low_intensity", 0) > 0
    out["addAParticle_into_13_of_14"] &= int((case.store[:, :, 0] > 0).sum(axis=1).max()) == 13
    n_in = sum(1 for u in case.updates[:1] for p in u["points"] if all(abs(float(a)) < b for a, b in zip(p, h)))
    out["newborn_outside_the_map"] = m.get("newborn_outside_map", 0) > 0 and len(case.updates) == 1 and (
        (recs[0]["cursors"][0] - case.cursors[0]) % len(g.pg) == (60 * n_in) % len(g.pg))
    if len(case.updates) == 1 and recs[0]["ok"]:
        n_p = len(g.pg)
        drawn = 60 * n_in
        out["position_table_wraps_inside_one_particle"] = case.cursors[0] + drawn >= n_p and (n_p - case.cursors[0]) % 3 != 0 and drawn > 0
        out["velocity_table_wraps"] = 0 < recs[0]["cursors"][1] < case.cursors[1]
        out["rand_table_wraps"] = 0 < recs[0]["cursors"][2] < case.cursors[2] and len(case.updates[0]["points"]) < 100
        for n in (1024, 1025, 2100):
            # n points of which all but the observation breed, and new-borns of the last points survive
            out["newborn_scan_%d_points" % n] = len(case.updates[0]["points"]) == n and n_in == n - 1 and recs[0]["n_particles"] > 200
    out["weight_one_float_below_removal"] = m.get("weight_at_removal_edge", 0) == 2 and m.get("weight_removed", 0) == 1
    out["weight_exactly_at_removal"] = m.get("weight_at_removal_edge", 0) == 2 and recs[0]["n_particles"] == 1
    counts = {n: m.get("voxel_with_%d_particles" % n, 0) for n in range(15)}
    after = (stores[1][:, :, 0] > 0).sum(axis=1) if st1 is not None else np.zeros(1)
    before = (case.store[:, :, 0] > 0).sum(axis=1)
    only_stays = len(traces) == 1 and all(e["kind"] == "stay" for e in t0) and not len(case.updates[0]["points"])
    out["no_resampling_below_5"] = only_stays and counts[4] > 0 and bool(((before == 4) & (after == 4)).any()) and m.get("weight_removed", 0) == 0
    for n in (5, 7, 8, 14):
        out["resampling_%d" % n] = only_stays and counts[n] > 0 and bool(((before == n) & (after == min(n, 7))).any()) and len(set(before[before > 0])) > 3
    out["flag_0_6_processed_by_next_prediction"] = len(traces) == 2 and any(e["was_copy"] for e in traces[1])
    return {k: bool(v) for k, v in out.items()}


def check_margins(case, g):
    mg = g.margins
    for key, bound in (("removal", 1e-3), ("resample", 1e-3), ("split_truncation", 1e-3), ("occlusion", 1e-3), ("dot", 1e-5), ("trunc", 1e-4)):
        assert mg.get(key, 1.0) >= bound, "%s: the margin of '%s' is %.3g < %g — redesign the case" % (case.name, key, mg[key], bound)
    if g.zero_dots:
        assert "zero_dot" in case.allow, "%s: a dot product is exactly 0 at %r" % (case.name, g.zero_dots[:3])
    if g.trunc_hits:
        assert "searched_truncation" in case.allow or "exact_cell_boundary" in case.allow, (case.name, g.trunc_hits[:3])
        if "exact_cell_boundary" in case.allow:      # only coordinates that are exactly 0: (0 + h) / res is the exact integer N / 2
            assert all(p == 0.0 for _, p, _ in g.trunc_hits), (case.name, g.trunc_hits[:3])
    return {k: float("%.3g" % v) for k, v in mg.items()}


def main():
    tables = dsp_case_tables()
    inputs = dsp_case_inputs()
    all_cases = [c for g in inputs for c in inputs[g]]
    fx = {"grids": {k: list(v) for k, v in DSP_CASE_GRIDS.items()}, "cases": [], "unclaimed": {}, "margins": {},
          "tables_sha256": hashlib.sha256(b"".join(t.tobytes() for t in tables)).hexdigest()}
    claimed = {}
    for grid in inputs:
        for case in inputs[grid]:
            g, recs, traces, stores = run_case(case, tables)
            margins = check_margins(case, g)
            labels = sorted(k for k, v in derive_labels(case, g, recs, traces, stores, all_cases).items() if v)
            for lab in labels:
                claimed.setdefault(lab, []).append(case.name)
            for k, v in margins.items():
                fx["margins"][k] = min(fx["margins"].get(k, v), v)
            fx["cases"].append({"name": case.name, "grid": grid, "in_sha256": dsp_case_sha256(case), "compare": bool(case.compare),
                                "branches": labels, "updates": recs})
            print(case.name, grid, [r["ok"] for r in recs], [r["n_particles"] for r in recs], recs[-1]["counters"], labels, margins, flush=True)
    for lab in LABELS:
        if lab not in claimed:
            fx["unclaimed"][lab] = NOT_BUILT.get(lab, "no case met the label's predicate in the reading's trace")
    assert set(claimed) <= set(LABELS), sorted(set(claimed) - set(LABELS))
    print("unclaimed:", fx["unclaimed"])
    with open(os.path.join(HERE, "dsp_cases_independent.json"), "w") as f:
        json.dump(fx, f)


if __name__ == "__main__":
    main()
