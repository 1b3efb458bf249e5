"""GPU: the consumers of per-agent tables (include/sogm_abi.h "radio links": sogm_update_world_views,
sogm_project_neighbours_views, sogm_safe_after_opt_views, sogm_planner_set_swarm_views).  Three agents on the parity grid
and views whose three blocks differ — agent 0 has heard one neighbour only, agent 1 holds a stale version of a record,
agent 2 has heard nothing.  What agent a gets from its block of the views is what it gets from the namesake entry on the
one shared table equal to that block, bit for bit."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
A = 3


def _mods():
    return (importlib.import_module("pred-occ-planner_amd.sogm"), importlib.import_module("pred-occ-planner_amd.planner"))


def _blocks(pop, sc, speed=1.0, stale_speed=1.6, stale_shift=-0.35):
    """(blocks uint8 [A][A][2064], the current table): block 0 = row 1 only, block 1 = row 0 in an earlier version (another
    speed, an earlier start) beside the current row 2, block 2 = nothing"""
    now = pop.scene.records_to_numpy(pop.scene.straight_records(sc, speed=speed)).reshape(A, -1)
    old = pop.scene.records_to_numpy(pop.scene.straight_records(
        sc, speed=stale_speed, t_start=float(sc["stamps"][0]) - 0.05 + stale_shift)).reshape(A, -1)
    blocks = np.zeros((A, A, now.shape[1]), np.uint8)
    blocks[0, 1] = now[1]
    blocks[1, 0], blocks[1, 2] = old[0], now[2]
    for b in range(A):                                     # (an empty row still names its drone)
        for j in range(A):
            if not blocks[b, j].any():
                blocks[b, j, :4] = now[j, :4]
    assert not np.array_equal(old[0], now[0])
    return blocks, now


def _frame_inputs(pop, sogm, sc, tl, k):
    f = tl.frame(k)
    poses = (sc["poses"] + np.float32([0.17 * k, -0.11 * k, 0.01 * k])).astype(np.float32)
    stamps = sc["stamps"] + 0.1 * k
    sck = dict(sc, poses=poses, stamps=stamps)
    return sck, sogm.World(f["cloud"], f["cylinders"]), sogm._dev(poses, np.float32), sogm._dev(stamps, np.float64)


@pytest.mark.parametrize("tiled,flow", [(True, 0), (False, 0), (True, 1)])
def test_update_world_views_builds_each_agents_map_from_its_own_table(pop, tiled, flow):
    """cells of agent a after sogm_update_world_views == after sogm_update_world on the shared table block a: rows and
    tiles, the plain update and the update flow; then a plain update on the same context leaves every cell equal to a
    fresh context's — the mark log named the sectors the views' overlay wrote"""
    sogm, _ = _mods()
    spec = pop.config.make_spec("parity", tiled=tiled)
    sc = pop.scene.make_scene(A, 4.95, seed=0x71, moving=True, circle_radius=2.0)
    tl = pop.scene.WorldTimeline(sc, 0.1, moving=True)
    ego = sogm._dev(sc["ego_ids"], np.int32)
    mv, ms, fresh = sogm.SogmMap(spec, A), sogm.SogmMap(spec, A), sogm.SogmMap(spec, A)
    for m in (mv, ms, fresh):
        m.set_sparse_reset(True)
        m.set_tuning("update_flow", flow)
    differ = 0
    for k in (0, 3):
        sck, w, d_poses, d_stamps = _frame_inputs(pop, sogm, sc, tl, k)
        blocks, _ = _blocks(pop, sck, speed=1.0 + 0.05 * k)
        mv.updateWorldViews(w, d_poses, d_stamps, sogm._dev(blocks.reshape(A * A, -1)), A, ego)
        got = [mv.download(a) for a in range(A)]
        per_block = []
        for b in range(A):
            ms.updateWorld(w, d_poses, d_stamps, sogm._dev(blocks[b]), A, ego)
            per_block.append([ms.download(a) for a in range(A)])
        for a in range(A):
            assert np.array_equal(got[a], per_block[a][a]), f"frame {k}, agent {a}: {(got[a] != per_block[a][a]).sum()} cells"
            differ += sum(not np.array_equal(per_block[b][a], per_block[a][a]) for b in range(A))
    assert differ >= 4, differ                              # the blocks do give different maps: the views matter
    # the next plain update (no records) on the context that took the views, against a context that never did
    sck, w, d_poses, d_stamps = _frame_inputs(pop, sogm, sc, tl, 4)
    mv.updateWorld(w, d_poses, d_stamps)
    fresh.updateWorld(w, d_poses, d_stamps)
    for a in range(A):
        assert np.array_equal(mv.download(a), fresh.download(a)), a
    state = mv.sparse_reset_state()
    print("sparse reset:", state)
    assert state["enabled"]
    for m in (mv, ms, fresh):
        m.close()


@pytest.mark.parametrize("kind", ["fake", "riskvoxel"])
def test_project_neighbours_views_on_both_map_kinds(pop, kind):
    """the overlay alone, on a FAKE map (it adds) and on a RiskVoxel map (it sets): the grid under it is a dense random one
    written through sogm_set_future_risk, the same in both contexts"""
    import torch
    sogm, _ = _mods()
    mk = pop._abi.SOGM_MAP_FAKE if kind == "fake" else pop._abi.SOGM_MAP_RISKVOXEL
    spec = pop.config.make_spec("parity", map_kind=mk)
    sc = pop.scene.make_scene(A, 4.95, seed=0x72, circle_radius=2.0)
    blocks, _ = _blocks(pop, sc)
    ego = sogm._dev(sc["ego_ids"], np.int32)
    V = spec.L * spec.W * spec.H
    base = (np.random.default_rng(3).random((A, V, spec.T)) < 0.01).astype(np.float32) * 0.5
    d_base, d_poses, d_stamps = sogm._dev(base, np.float32), sogm._dev(sc["poses"], np.float32), sogm._dev(sc["stamps"], np.float64)
    mv, ms = sogm.SogmMap(spec, A), sogm.SogmMap(spec, A)
    mv.futureRiskCallback(d_base, d_poses, d_stamps)
    mv.addOtherAgentsViews(sogm._dev(blocks.reshape(A * A, -1)), A, ego)
    torch.cuda.synchronize()
    differ = 0
    for b in range(A):
        ms.futureRiskCallback(d_base, d_poses, d_stamps)
        ms.addOtherAgents(sogm._dev(blocks[b]), A, ego)
        want = ms.download(b)
        got = mv.download(b)
        assert np.array_equal(got, want), (kind, b, int((got != want).sum()))
        differ += not np.array_equal(want, base[b])
    assert differ == 2                                      # blocks 0 and 1 add marks, block 2 (nothing heard) adds none
    mv.close()
    ms.close()


def _candidates(sc, rng):
    """short straight stubs from each start towards the circle's centre"""
    cpts, npoly = np.zeros((A, 16 * 15)), np.zeros(A, np.int32)
    for a in range(A):
        M = 3 + a
        npoly[a] = M
        d = -sc["starts"][a] * np.array([1, 1, 0])
        d /= np.linalg.norm(d)
        for k in range(5 * M):
            cpts[a, k * 3:(k + 1) * 3] = sc["starts"][a] + d * 0.2 * k + rng.normal(0, 0.01, 3)
    return cpts, npoly


def test_safe_after_opt_views_checks_each_agent_against_its_own_table(pop, orc):
    sogm, planner = _mods()
    spec = pop.config.make_spec("parity")
    sc = pop.scene.make_scene(A, 4.95, seed=5, circle_radius=2.0, n_cyl=0)
    blocks, now = _blocks(pop, sc, speed=1.5)
    # every agent also meets a record that flies its own line under another drone's name: unsafe wherever it is heard
    ghost = now[0].copy()
    ghost[:4] = now[1, :4]
    blocks[0, 1] = ghost
    cpts, npoly = _candidates(sc, np.random.default_rng(4))
    m = sogm.SogmMap(spec, A)
    P = planner.SogmPlanner(m, pop.config.make_astar_params(), pop.config.make_planner_params(True),
                            pop.config.make_qp_settings())
    ego, t_now = sogm._dev(sc["ego_ids"], np.int32), sogm._dev(sc["stamps"], np.float64)
    d_cpts, d_npoly = sogm._dev(cpts, np.float64), sogm._dev(npoly, np.int32)
    got = P.isSafeAfterOptViews(d_cpts, d_npoly, sogm._dev(blocks.reshape(A * A, -1)).view(A, A, -1), A, ego, t_now).cpu().numpy()
    shared = np.stack([P.isSafeAfterOpt(d_cpts, d_npoly, sogm._dev(blocks[b]), A, ego, t_now).cpu().numpy() for b in range(A)])
    want = np.array([shared[a, a] for a in range(A)])
    print("views:", got, "shared tables, block by block:", shared.tolist())
    assert np.array_equal(got, want)
    recs = [planner.records_from_bytes(blocks[b]) for b in range(A)]
    oracle = np.array([orc.safe_after_opt(cpts[a], int(npoly[a]), recs[a], A, int(sc["ego_ids"][a]), float(sc["stamps"][a]))
                       for a in range(A)])
    assert np.array_equal(got, oracle)
    assert got[0] == 0 and got[2] == 1                      # the ghost on agent 0's line; nothing heard by agent 2
    assert (shared != shared[0]).any()                      # and the blocks do give different verdicts
    P.close()
    m.close()


@pytest.mark.parametrize("flow", ["1", "0"])
def test_replan_after_set_swarm_views_ends_like_the_per_agent_shared_tables(pop, monkeypatch, flow):
    """both forms of the replan's end: the dataflow replan's finishing wave (SOGM_FLOW=1) and the grouped path's
    k_safe_after_opt (SOGM_FLOW=0)"""
    from helpers import hard_cases
    sogm, planner = _mods()
    monkeypatch.setenv("SOGM_FLOW", flow)                   # read by sogm_planner_create
    spec = pop.config.make_spec("parity")
    sc, pva = hard_cases(pop, A, 17)
    dev = sogm.upload_scene(sc)
    m = sogm.SogmMap(spec, A)
    m.updateMap(dev["cloud"], dev["cloud_range"], dev["cylinders"], dev["n_cyl"], dev["poses"], dev["stamps"])
    P = planner.SogmPlanner(m, pop.config.make_astar_params(), pop.config.make_planner_params(True),
                            pop.config.make_qp_settings())
    t_start = sc["stamps"] + 0.05
    d_pva, d_ts, d_goal = sogm._dev(pva, np.float64), sogm._dev(t_start, np.float64), sogm._dev(sc["goals"], np.float64)
    rec0, ok0 = P.replan(d_pva, d_goal, d_ts, dev["ego_ids"])
    rec0, ok0 = rec0.cpu().numpy().copy(), ok0.cpu().numpy().copy()
    assert ok0.sum() >= 2, ok0
    # the tables: every agent's own solution under the NEXT drone's name (it flies through whoever hears it), stale and
    # empty rows as in the other tests
    blocks = np.zeros((A, A, rec0.shape[1]), np.uint8)
    ids = np.ascontiguousarray(sc["ego_ids"], np.int32).view(np.uint8).reshape(A, 4)
    for b in range(A):
        for j in range(A):
            blocks[b, j, :4] = ids[j]
    for a in (0, 1):
        j = (a + 1) % A
        blocks[a, j] = rec0[a]
        blocks[a, j, :4] = ids[j]
        # time_start: already in the air at the check's `now` (a record that has not started is not checked)
        blocks[a, j, 8:16] = np.frombuffer(np.float64(sc["stamps"][a] - 0.05).tobytes(), np.uint8)
    d_now = sogm._dev(sc["stamps"], np.float64)
    views = sogm._dev(blocks.reshape(A * A, -1)).view(A, A, -1)
    P.set_swarm_views(views, A, dev["ego_ids"], d_now)
    rec_v, ok_v = P.replan(d_pva, d_goal, d_ts, dev["ego_ids"])
    rec_v, ok_v = rec_v.cpu().numpy().copy(), ok_v.cpu().numpy().copy()
    shared_ok, shared_rec = [], []
    for b in range(A):
        P.setSwarm(sogm._dev(blocks[b]), A, dev["ego_ids"], d_now)      # also switches the views off
        r, o = P.replan(d_pva, d_goal, d_ts, dev["ego_ids"])
        shared_ok.append(o.cpu().numpy().copy())
        shared_rec.append(r.cpu().numpy().copy())
    want = np.array([shared_ok[a][a] for a in range(A)])
    print("flow", flow, "ok without a swarm", ok0, "with views", ok_v, "shared, block by block", [o.tolist() for o in shared_ok])
    assert np.array_equal(ok_v, want)
    for a in range(A):
        assert np.array_equal(rec_v[a], shared_rec[a][a]), a
    assert np.array_equal(ok_v[2:], ok0[2:]) and (ok_v[:2] < ok0[:2]).any()   # nothing heard: as without a swarm; the ghosts bite
    P.setSwarm(None, 0, None, None)
    _, ok2 = P.replan(d_pva, d_goal, d_ts, dev["ego_ids"])
    assert np.array_equal(ok2.cpu().numpy(), ok0)
    P.close()
    m.close()
