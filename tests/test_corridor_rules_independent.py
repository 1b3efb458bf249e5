"""The corridor rules around FIRI (rows a11 / a13: per-segment box, ShrinkCorridor, validity + break, adjacent-intersection
scan, goal scan, both planners' truncation arithmetic) held to tests/golden/corridor_rules_independent.json, a second
reading written from the reference text (tests/golden/make_corridor_rules_fixture.py) on hand-built polytopes injected
where FIRI's would be.  Copied numbers, integers and flags agree exactly; shrunk offsets and projected goals within
1e-9 absolute (the text leaves n.norm() and the matrix-vector products to Eigen; the generator keeps every decision
1e-6 / 1e-3 away from its threshold, so the last bits never decide)."""
import importlib
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MP = 16
TOL = 1.0e-9

_VARIANT_BOTH = ["first_invalid", "k_invalid", "capacity", "isect_fail_0", "isect_fail_1", "isect_fail_ge2", "route_len_0",
                 "route_len_1", "route_len_2", "route_gt16", "goal_in_last", "z_negative", "start_z_low", "start_z_high",
                 "init_range_wide", "shrink_sides", "zero_path", "shrink_zero"]
# the goal scan truncates in the fake planner only: the real planner's extra first call projects the goal into the last
# polytope, where the scan then finds it at once (the generator's docstring) — its list has that call and the "<= 1" exit
BRANCHES = ({f"fake/{k}" for k in _VARIANT_BOTH + ["goal_in_earlier", "goal_outside_all", "single_poly_goal_outside"]} |
            {f"real/{k}" for k in _VARIANT_BOTH + ["first_call_projects", "le1_exit"]})


@pytest.fixture(scope="module")
def fx():
    return json.load(open(os.path.join(HERE, "golden", "corridor_rules_independent.json")))


def _inputs(pop, fx, case):
    MF = fx["max_faces"]
    pp = pop.config.make_planner_params(bool(case["fake"]))
    pp.init_range, pp.shrink_size, pp.max_faces = case["init_range"], case["shrink_size"], MF
    route = np.asarray(case["route"], np.float64).reshape(-1, 6)
    polys = np.zeros((MP, MF, 4))
    nf = np.zeros(MP, np.int32)
    st = np.ones(MP, np.int32)
    for i, rows in enumerate(case["polys"][:MP]):
        polys[i, :len(rows)] = rows
        nf[i] = len(rows)
    for i, s in enumerate(case.get("seg_state", [])):
        st[i] = s
    return pp, np.asarray(case["start_pva"], np.float64), route, polys, nf, st


def _check(case, got, who):
    """got: box [16,6], shrunk [16,MF,4], seg_nfaces, seg_state, polys, nfaces, npoly, goal — against the second reading"""
    exp, name = case["expected"], f"{who} {case['branch']}"
    nseg = len(exp["box"])
    assert nseg == min(max(len(case["route"]) - 1, 0), MP), name
    assert np.array_equal(got["seg_state"][:nseg], exp["seg_state"]) and np.all(got["seg_state"][nseg:] == -2), name
    for i in range(nseg):
        assert np.array_equal(got["box"][i], exp["box"][i]), (name, "box", i)
        want = np.asarray(exp["shrunk"][i])
        assert got["seg_nfaces"][i] == len(want), (name, "seg_nfaces", i)
        g = got["shrunk"][i, :len(want)]
        assert np.array_equal(g[:, :3], want[:, :3]), (name, "face order / normals", i)
        assert np.abs(g[:, 3] - want[:, 3]).max() <= TOL, (name, "shrunk offsets", i)
        if case["shrink_size"] == 0.0:
            assert np.array_equal(g, want), (name, "shrink_size 0 copies", i)
    assert int(got["npoly"]) == exp["npoly"], (name, "npoly", int(got["npoly"]), exp["npoly"], case["trace"])
    assert np.array_equal(got["nfaces"][:exp["npoly"]], exp["nfaces"]) and np.all(got["nfaces"][exp["npoly"]:] == 0), name
    for i in range(exp["npoly"]):
        want = np.asarray(exp["polys"][i])
        g = got["polys"][i, :len(want)]
        assert np.array_equal(g[:, :3], want[:, :3]) and np.abs(g[:, 3] - want[:, 3]).max() <= TOL, (name, "polys", i)
    goal, want = np.asarray(got["goal"]), np.asarray(exp["goal"])
    route_rows = [list(r) for r in case["route"]]
    if exp["npoly"] == 0 or list(want) in route_rows:   # zeros, or copied from the route: exact
        assert np.array_equal(goal, want), (name, "goal", goal, want)
    else:                                               # projected position, velocity copied
        assert np.abs(goal[:3] - want[:3]).max() <= TOL and np.array_equal(goal[3:], want[3:]), (name, "goal", goal, want)


def test_fixture_covers_every_branch(fx):
    assert {c["branch"] for c in fx["cases"]} == BRANCHES
    assert len(fx["cases"]) == len(BRANCHES)
    projected = [c for c in fx["cases"] if c["expected"]["npoly"] and
                 c["expected"]["goal"] not in [list(r) for r in c["route"]]]
    assert {c["branch"] for c in projected} == {"fake/goal_outside_all"}   # the only case whose goal is not a route row


def test_oracle_matches_second_reading(pop, orc, fx):
    for case in fx["cases"]:
        pp, sp, route, polys, nf, st = _inputs(pop, fx, case)
        got = orc.corridor_rules(pp, sp, route, polys, nf, st if "seg_state" in case else None)
        _check(case, got, "oracle")
        assert got["corridor_capacity"] == case["expected"]["corridor_capacity"], case["branch"]
        assert got["pieces_capacity"] == case["expected"]["pieces_capacity"], case["branch"]


@pytest.mark.gpu
def test_hip_matches_second_reading_and_oracle(pop, orc, fx):
    """sogm_corridor_rules_batched, all cases in one launch: against the fixture directly, against the oracle bit for bit,
    and the two capacity counters on the cases that raise them."""
    import torch
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    cases = fx["cases"]
    n, MF, RC = len(cases), fx["max_faces"], 24
    ins = [_inputs(pop, fx, c) for c in cases]
    sp = np.zeros((n, 9))
    route = np.zeros((n, RC, 6))
    rl = np.zeros(n, np.int32)
    polys = np.zeros((n, MP, MF, 4))
    nf = np.zeros((n, MP), np.int32)
    st = np.ones((n, MP), np.int32)
    for k, (pp, s, r, p, f, t) in enumerate(ins):
        sp[k], rl[k], polys[k], nf[k], st[k] = s, len(r), p, f, t
        route[k, :len(r)] = r
    m = sogm.SogmMap(pop.config.make_spec("parity"), 1)
    P = planner.SogmPlanner(m, pop.config.make_astar_params(), pop.config.make_planner_params(True),
                            pop.config.make_qp_settings())
    before = P.counters()
    out = planner.corridor_rules_batched([i[0] for i in ins], sogm._dev(sp, np.float64), sogm._dev(route, np.float64),
                                         sogm._dev(rl, np.int32), sogm._dev(polys, np.float64), sogm._dev(nf, np.int32),
                                         sogm._dev(st, np.int32), planner=P)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    after = P.counters()
    P.close()
    m.close()
    for k, case in enumerate(cases):
        got = {key: out[key][k] for key in out}
        _check(case, got, "hip")
        pp, s, r, p, f, t = ins[k]
        want = orc.corridor_rules(pp, s, r, p, f, t)
        nseg = len(case["expected"]["box"])
        for key in ("box", "seg_nfaces", "seg_state", "nfaces", "goal"):
            assert np.array_equal(got[key], want[key]), (case["branch"], key)
        assert int(got["npoly"]) == want["npoly"], case["branch"]
        for i in range(nseg):
            assert np.array_equal(got["shrunk"][i, :f[i]], want["shrunk"][i, :f[i]]), (case["branch"], "shrunk", i)
        for i in range(want["npoly"]):
            k_ = want["nfaces"][i]
            assert np.array_equal(got["polys"][i, :k_], want["polys"][i, :k_]), (case["branch"], "polys", i)
    for key in ("corridor_capacity", "pieces_capacity"):
        raised = sum(c["expected"][key] for c in cases)
        assert raised == 2 and after[key] - before[key] == raised, (key, before, after)
