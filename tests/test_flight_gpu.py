"""GPU: sogm_flight_run — n ticks of every agent in one call, every agent on its own clock (sogm_abi.h "Flight").

The reference's drones replan asynchronously and read whatever trajectories arrived last
(plan_manager/src/plan_manager.cpp:92-233, traj_coordinator/src/particles.cpp:179-190).  The flight fixes the RESULTS
with a staleness rule (tick k reads the agent's own record of tick k - 1 and the neighbours' records of tick k - 2) and
leaves the SCHEDULE free.  Checked here:
  * the flight's per-tick records and ok flags equal, bit for bit, those of the same rule flown lock-step through the
    per-tick entry points (sogm_update_world + sogm_replan, SwarmTick(neighbour_lag=2)) — whatever order the device ran
    the agents in;
  * that lock-step reference is held to the CPU oracle flown with the same rule, stage by stage (cells, A* pop order,
    polytopes, QP);
  * a flight continues a flight; the full-size swarm (128 agents, 200^3 x 20) flies with no failed tick;
  * LIVENESS (round 6).  Round 5's driver box lost one 60-tick flight of five to the 3 s device time-out.  Cause: the
    corridor kernel's compute-unit mask held four units in one shader engine and eight in another, the workgroup
    dispatcher rotates over a mask's engines and stops at the first full one, so 120 of its 384 workgroups waited in the
    dispatcher for the whole flight; whenever the hardware scheduler saved and restored the process's queues (any queue
    created or destroyed on the device does that) they started in the freed slots ahead of the restored waves, and a
    saved wave per XCD stayed saved until the other kernels left.  Held here: every workgroup of every flight starts
    within 1 ms (hdr[15] == 0, asserted after EVERY flight of this file), full-size flights survive a queue being
    created and destroyed in their middle with identical records, and 5 x 60 full-size ticks after a lock-step swarm has
    lived in the process end with no error and the lock-step rule's ok fraction."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _lockstep_lag2(driver, grid, A, n, lag=2, maps=None, **kw):
    """`maps`: a list that receives every agent's grid of the last tick (downloaded before the swarm is closed)"""
    import torch
    sw = driver.SwarmTick(grid, A, moving_world=True, prestamp=False, neighbour_lag=lag, **kw)
    oks, recs = [], []
    for _ in range(n):
        oks.append(sw.step().cpu().numpy().copy())
        recs.append(sw.new.cpu().numpy().copy())
    torch.cuda.synchronize()
    assert sw.planner.flow_failures() == (0, 0)
    own = sw.own.cpu().numpy().copy()
    cnt = sw.planner.counters()
    if maps is not None:
        maps.extend(sw.map.download(a) for a in range(A))
    sw.close()
    return np.stack(oks), np.stack(recs), own, cnt


def _flight(driver, grid, A, chunks, **kw):
    import torch
    pop_abi = importlib.import_module("pred-occ-planner_amd")._abi
    sw = driver.SwarmTick(grid, A, moving_world=True, prestamp=False, **kw)
    oks, recs = [], []
    for n in chunks:
        ok, rec = sw.fly(n)
        torch.cuda.synchronize()
        ms, hdr = sw.planner.flight_stats()
        E, F = sw.planner._abi_idx = (pop_abi.FLIGHT_HDR_ERR, pop_abi.FLIGHT_HDR_FINISHED)
        assert hdr[E] == 0 and sw.planner.flow_failures() == (0, 0), (hdr.tolist(), sw.planner.flow_failures())
        assert hdr[F] == A * n and (ms[:, 7] == n).all(), (hdr.tolist(), ms[:, 7])
        # every workgroup of the four kernels was running from the start (sogm_flight_stats hdr[15] = workgroups that started
        # more than 1 ms late): what the flight's liveness under a queue save / restore rests on (csrc flight_layout)
        assert hdr[pop_abi.FLIGHT_HDR_LATE_WGS] == 0, hdr.tolist()
        oks.append(ok.cpu().numpy().copy())
        recs.append(rec.cpu().numpy().copy())
    own = sw.own.cpu().numpy().copy()
    last = sw.all.cpu().numpy().copy()
    cnt = sw.planner.counters()
    sw.close()
    return np.concatenate(oks), np.concatenate(recs), own, last, cnt, ms


def test_flight_records_equal_the_lockstep_flight_with_the_same_staleness_rule(pop):
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    K, A = 10, 6
    ok_l, rec_l, own_l, cnt_l = _lockstep_lag2(driver, "parity", A, K)
    ok_f, rec_f, own_f, last_f, cnt_f, ms = _flight(driver, "parity", A, [K])
    assert ok_l.sum() > K * A // 3  # (a flight in which replans succeed)
    assert np.array_equal(ok_f, ok_l), (ok_f, ok_l)
    for k in range(K):
        assert np.array_equal(rec_f[k], rec_l[k]), f"tick {k}: records differ in agents {np.flatnonzero((rec_f[k] != rec_l[k]).any(axis=1))}"
    assert np.array_equal(own_f, own_l) and np.array_equal(last_f, own_l)
    assert cnt_f == cnt_l
    print("flight, per-agent ms per tick:", dict(zip(pop._abi.FLIGHT_STAT_NAMES, (ms[:, :7].sum(axis=0) / ms[:, 7].sum()).round(3))))


def test_a_flights_grids_equal_the_lockstep_rules_grids(pop):
    """The cells themselves, not the records planned in them: a call builds no map beyond its last tick, so after fly(4) every
    agent's grid is its map of tick 3 — frame 3's stamp plus the overlay of table ver(1), the first table that holds records
    (the smallest flight whose overlay adds anything) — and must equal, cell for cell, the grid the per-tick entry points leave
    after the same four ticks (stores of 1.0 and additions of 1.0f: exact in any order)."""
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    K, A = 4, 6
    want = []
    ok_l, _, _, _ = _lockstep_lag2(driver, "parity", A, K, maps=want)
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False)
    sw.fly(K)
    torch.cuda.synchronize()
    _, hdr = sw.planner.flight_stats()
    pop_abi = importlib.import_module("pred-occ-planner_amd")._abi
    assert hdr[pop_abi.FLIGHT_HDR_ERR] == 0 and hdr[pop_abi.FLIGHT_HDR_FINISHED] == A * K, hdr.tolist()
    got = [sw.map.download(a) for a in range(A)]
    sw.close()
    assert ok_l[1].any()  # (table ver(1) holds records: tick 3's overlay had something to add)
    for a in range(A):
        assert np.count_nonzero(want[a]) > 0 and np.count_nonzero(got[a]) > 0, a
        assert np.array_equal(got[a], want[a]), f"agent {a}: {np.count_nonzero(got[a] != want[a])} cells differ"


def test_a_flight_continues_a_flight(pop):
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    one = _flight(driver, "parity", 5, [9])
    two = _flight(driver, "parity", 5, [1, 3, 5])
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    assert np.array_equal(one[2], two[2]) and np.array_equal(one[3], two[3])


def test_the_staleness_rule_flown_lockstep_against_the_oracle_stage_by_stage(pop, orc):
    """the reference path of the first test against the CPU oracle under the same rule: every tick's map (this tick's frame,
    overlay of table ver(k - 2)), A* pop order, polytopes and QP of every agent"""
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    fp = importlib.import_module("test_full_size_parity")
    sw = driver.SwarmTick("parity", 6, moving_world=True, prestamp=False, neighbour_lag=2)
    acc = {}
    for _ in range(7):
        fp._sum(acc, fp._tick_with_parity(pop, orc, sw, list(range(6))))
    print("staleness rule, lock-step vs oracle:", acc)
    assert acc["agents"] == 42 and acc["qp_ok"] >= 18 and acc["fused_checked"] == 42
    sw.close()


def test_flight_with_and_without_masks_and_speculation_gives_the_same_records(pop):
    """scheduling knobs must not change results: unmasked streams, sequential search attempts, other ticket counts, the
    urgent lane"""
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    base = _flight(driver, "parity", 6, [6])
    for tuning in ({"flight_spec": 0}, {"flight_reset": 2, "flight_bits": 3, "flight_marks": 5, "flight_splat": 1},
                   {"flight_qp_units": 2, "flight_search_units": 1, "flight_map_units": 6},
                   # the urgent lane of the map kernel: none, a few agents with the plain ticket counts, nearly all
                   # agents with the finest tickets on a handful of workers
                   {"flight_urgent": 0}, {"flight_urgent": 2, "flight_urgent_fine": 1},
                   {"flight_urgent": 5, "flight_urgent_waves": 7, "flight_urgent_fine": 16}):
        other = _flight(driver, "parity", 6, [6], tuning=tuning)
        assert np.array_equal(base[0], other[0]) and np.array_equal(base[1], other[1]), tuning


def test_full_size_flight_equals_lockstep_rule(pop):
    """BASELINE configs[2]'s swarm (128 agents, 200^3 x 20, moving world): six ticks in one flight against the same rule flown
    lock-step — records and ok flags bit for bit, no failed tick, every agent-tick accounted for."""
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    K, A = 6, 128
    ok_l, rec_l, own_l, cnt_l = _lockstep_lag2(driver, "cfg2", A, K)
    ok_f, rec_f, own_f, last_f, cnt_f, ms = _flight(driver, "cfg2", A, [K])
    assert np.array_equal(ok_f, ok_l)
    for k in range(K):
        assert np.array_equal(rec_f[k], rec_l[k]), f"tick {k}: agents {np.flatnonzero((rec_f[k] != rec_l[k]).any(axis=1))}"
    assert np.array_equal(own_f, own_l) and cnt_f == cnt_l
    per = ms[:, :7].sum(axis=0) / ms[:, 7].sum()
    print("cfg2 flight, mean ms per agent-tick:", dict(zip(pop._abi.FLIGHT_STAT_NAMES, per.round(3))), "ok", int(ok_f.sum()), "of", K * A)


def _poke_queue(delay_s):
    """create and destroy a CU-masked stream (= a new hardware queue: the scheduler unmaps and remaps every queue of the
    process, compute waves are saved and restored) `delay_s` from now, on a thread of its own"""
    import ctypes as C
    import threading
    import time
    path = next(m.split()[-1] for m in open("/proc/self/maps") if "libamdhip64" in m)
    h = C.CDLL(path)
    h.hipExtStreamCreateWithCUMask.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    res = {}

    def run():
        time.sleep(delay_s)
        st = C.c_void_p()
        mask = (C.c_uint32 * 8)(1, 0, 0, 0, 0, 0, 0, 0)
        res["create"] = h.hipExtStreamCreateWithCUMask(C.byref(st), 8, mask)
        res["destroy"] = h.hipStreamDestroy(st) if res["create"] == 0 else -1

    th = threading.Thread(target=run)
    th.start()
    return th, res


def test_full_size_flight_survives_a_queue_save_and_restore_with_identical_records(pop):
    """A run-list change in the middle of a flight (here: this process creates and destroys a masked stream 60 / 150 / 250 ms
    into 60-tick flights; on the round-5 layout the FIRST such flight timed out, tools/diag_flight_preempt.py) must cost a
    flight nothing but time: no error, every agent-tick finished, and the records of the undisturbed flight, bit for bit."""
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    A, n = 128, 60
    calm = _flight(driver, "cfg2", A, [3, n, n])
    sw = driver.SwarmTick("cfg2", A, moving_world=True, prestamp=False, grids=1)
    sw.compute.prepare(0, 3 + 2 * n + 1)
    oks, recs = [], []
    for chunk, delay in ((3, None), (n, 0.06), (n, 0.25)):
        th = _poke_queue(delay) if delay is not None else None
        ok, rec = sw.fly(chunk)
        torch.cuda.synchronize()
        if th is not None:
            th[0].join()
            assert th[1] == {"create": 0, "destroy": 0}, th[1]
        _, hdr = sw.planner.flight_stats()
        assert hdr[pop._abi.FLIGHT_HDR_ERR] == 0 and hdr[pop._abi.FLIGHT_HDR_FINISHED] == A * chunk, hdr.tolist()
        assert hdr[pop._abi.FLIGHT_HDR_LATE_WGS] == 0 and sw.planner.flow_failures() == (0, 0), hdr.tolist()
        oks.append(ok.cpu().numpy().copy())
        recs.append(rec.cpu().numpy().copy())
    own = sw.own.cpu().numpy().copy()
    sw.close()
    assert np.array_equal(np.concatenate(oks), calm[0]) and np.array_equal(np.concatenate(recs), calm[1])
    assert np.array_equal(own, calm[2])


def test_soak_five_flights_of_sixty_after_a_lockstep_swarm_lived_in_the_process(pop):
    """bench.py's sequence: a lock-step swarm (three grids, nine streams) flown and closed, then a fresh
    flight swarm flying 3 + 20 + 5 x 60 full-size ticks — every flight checked when it ends: no error, every agent-tick
    finished, no late workgroup, worst flight within 1.5 x of the best; the ok fraction equals the same rule flown lock-step."""
    import time
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    A, chunks = 128, [3, 20, 60, 60, 60, 60, 60]
    head = driver.SwarmTick("cfg2", A, moving_world=True)
    head.compute.prepare(0, 13)
    for _ in range(12):
        head.step()
    torch.cuda.synchronize()
    assert head.planner.flow_failures() == (0, 0)
    scene = head.scene
    head.close()
    torch.cuda.empty_cache()
    sw = driver.SwarmTick("cfg2", A, moving_world=True, prestamp=False, grids=1, scene=scene)
    sw.compute.prepare(0, sum(chunks) + 1)
    n_ok, per_tick = 0, []
    for n in chunks:
        t0 = time.perf_counter()
        ok, _ = sw.fly(n)
        torch.cuda.synchronize()
        per_tick.append((time.perf_counter() - t0) / n * 1e3)
        _, hdr = sw.planner.flight_stats()
        assert hdr[pop._abi.FLIGHT_HDR_ERR] == 0 and hdr[pop._abi.FLIGHT_HDR_FINISHED] == A * n, (n, hdr.tolist())
        assert hdr[pop._abi.FLIGHT_HDR_LATE_WGS] == 0 and sw.planner.flow_failures() == (0, 0), (n, hdr.tolist())
        n_ok += int(ok.sum().item())
    sw.close()
    torch.cuda.empty_cache()
    sixty = per_tick[2:]
    assert max(sixty) <= 1.5 * min(sixty), per_tick
    ok_l, _, _, _ = _lockstep_lag2(driver, "cfg2", A, sum(chunks), scene=scene, grids=1)
    assert n_ok == int(ok_l.sum()), (n_ok, int(ok_l.sum()))
    print("soak: ms per tick of the seven flights", [round(x, 2) for x in per_tick], "ok fraction", n_ok / (A * sum(chunks)))


def test_flight_through_frames_of_different_sizes(pop, monkeypatch):
    """agents of one flight are on ticks k and k + 1 at once; when those frames hold different numbers of
    256-point blocks, the per-agent crop lists — one buffer for the whole flight — must keep ONE row stride (CloudBlocks::row,
    the context's capacity), not the frame's block count: with the frame's count as the stride an agent's head overwrote the
    list another agent's bits tickets were still reading, and obstacles went missing from a map.  Every frame here drops a
    different number of trailing cloud points (block counts differ by up to 6); the flight must still equal the same rule
    flown lock-step, where one tick runs at a time."""
    scene_mod = importlib.import_module("pred-occ-planner_amd.scene")
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    plain = scene_mod.WorldTimeline.frame
    blocks = set()

    def ragged(self, k):
        f = plain(self, k)
        n = len(f["cloud"]) - 530 * ((k * 7) % 4)
        blocks.add((max(n, 256) + 255) // 256)
        return {"cloud": np.ascontiguousarray(f["cloud"][:max(n, 256)]), "cylinders": f["cylinders"]}

    monkeypatch.setattr(scene_mod.WorldTimeline, "frame", ragged)
    K, A = 9, 6
    ok_l, rec_l, own_l, cnt_l = _lockstep_lag2(driver, "parity", A, K)
    ok_f, rec_f, own_f, last_f, cnt_f, ms = _flight(driver, "parity", A, [K])
    assert len(blocks) >= 3, blocks   # (the frames really differ in their block counts)
    assert np.array_equal(ok_f, ok_l), (ok_f, ok_l)
    for k in range(K):
        assert np.array_equal(rec_f[k], rec_l[k]), f"tick {k}: agents {np.flatnonzero((rec_f[k] != rec_l[k]).any(axis=1))}"
    assert np.array_equal(own_f, own_l) and cnt_f == cnt_l


def test_flight_with_the_references_staleness_equals_the_lockstep_tick(pop):
    """VERDICT r05 missing #5: the reference's drones read records that are at most ONE broadcast old
    (traj_coordinator/src/particles.cpp:179-190); the flight's default rule reads them two ticks old.  With
    `flight_neighbour_lag` = 1 tick k's overlay and isSafeAfterOpt read table ver(k - 1) — an agent still builds the reset, bits
    and marks of its next map while it waits for the swarm's previous tick — and the records must equal the ordinary lock-step
    tick's (sogm_update_world + sogm_replan, the bench's headline rule), bit for bit: parity grid and 128 x 200^3 x 20."""
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    for grid, A, K in (("parity", 6, 10), ("cfg2", 128, 6)):
        ok_l, rec_l, own_l, cnt_l = _lockstep_lag2(driver, grid, A, K, lag=1)
        ok_f, rec_f, own_f, last_f, cnt_f, ms = _flight(driver, grid, A, [K], tuning={"flight_neighbour_lag": 1})
        assert ok_l.sum() > K * A // 3
        assert np.array_equal(ok_f, ok_l), (grid, ok_f.sum(axis=1), ok_l.sum(axis=1))
        for k in range(K):
            assert np.array_equal(rec_f[k], rec_l[k]), f"{grid} tick {k}: agents {np.flatnonzero((rec_f[k] != rec_l[k]).any(axis=1))}"
        assert np.array_equal(own_f, own_l) and cnt_f == cnt_l
        print(grid, "flight with the reference's staleness, mean ms per agent-tick:",
              dict(zip(pop._abi.FLIGHT_STAT_NAMES, (ms[:, :7].sum(axis=0) / ms[:, 7].sum()).round(3))))
