"""GPU: sogm_flight_run under the per-agent FSM (sogm_planner_set_flight_fsm) — every agent-tick of a flight is one
FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233) under the flight's staleness rule: only the
agents that are due replan, EXEC_TRAJ agents check the lapse, isTrajSafe and the goal, a machine that gives up publishes
a hover record.

Held here, byte for byte and tick for tick, against the SAME rule flown lock-step through the per-tick entry points
(sogm_fsm_inputs -> sogm_update_world -> overlay -> sogm_traj_safe -> sogm_planner_set_due -> sogm_replan ->
sogm_fsm_apply): with flight_neighbour_lag = 1 that is SwarmTick.step() itself (step_fsm_device), with the flight's own
rule (the neighbours' records of tick k - 2) the helper _lockstep below, which keeps the last two tables.  Every flight
of this file ends with the assertions of tests/test_flight_gpu.py::_flight: error word 0, no failed tick, every
agent-tick finished, no late workgroup.

The swarm: SwarmTick("parity", 8, moving_world=True), 25 ticks — the figures of
test_fsm_device_gpu.py::test_closed_loop_with_the_machines_on_the_device.  Coverage (an agent-tick that was not due, the
states EXEC_TRAJ and REPLAN, an unsafe verdict, a hover record) is asserted on the LOCK-STEP side's log; for the hover
record a second swarm of 12 ticks runs with replan_max_failures = 0, where the first failed REPLAN gives up.  That swarm
has scene seed 1: with the default seed the parity swarm's first failed REPLAN comes at tick 24 (8 agents; seeds 1 .. 7 and
8, 10, 12 agents were flown LOCK-STEP for 12 and 40 ticks, and seed 1 with 8 agents fails a REPLAN at tick 9, the earliest
of them) — chosen on the lock-step run, before any flight of it was looked at."""
import functools
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A_MAIN, N_MAIN = 8, 25
A_HOVER, N_HOVER, SEED_HOVER = 8, 12, 1
KEYS = ("own", "state", "due", "safe", "reached", "pub", "hover_start", "ok", "new")


def _mods():
    return (importlib.import_module("pred-occ-planner_amd.driver"), importlib.import_module("pred-occ-planner_amd.fsm"),
            importlib.import_module("pred-occ-planner_amd._abi"))


def _swarm(driver, fsm, A, max_failures=None, **kw):
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False, fsm=True, device_fsm=True, **kw)
    if max_failures is not None:   # the helper's own SogmFsmParams (inputs, apply and fly all read sw.fsm_dev.prm)
        sw.fsm_dev.prm = fsm.make_params(driver.TICK_PERIOD, driver.REPLAN_START_TIME, driver.GOAL_TOLERANCE, 1.0,
                                         max_failures)
    return sw


def _tick_row(sw, ok, safe):
    f = sw.fsm_dev
    return {"own": sw.own, "state": f.state, "due": f.due, "safe": safe, "reached": f.reached, "pub": f.pub,
            "hover_start": f.hover_start, "ok": ok, "new": sw.new}


def _stack(rows):
    return {k: np.stack([r[k] for r in rows]) for k in KEYS}


def _host(row):
    return {k: v.cpu().numpy().copy() for k, v in row.items()}


def _lockstep(A, n, lag, max_failures=None, audit=False, **kw):
    """the rule flown lock-step.  lag 1: SwarmTick.step() (step_fsm_device); lag 2: the same entry points with the
    overlay and isSafeAfterOpt of tick k reading ver(k - 2), the last two executed tables kept here"""
    import torch
    driver, fsm, _ = _mods()
    sw = _swarm(driver, fsm, A, max_failures, audit=audit, **kw)
    rows = []
    if lag == 1:
        for _ in range(n):
            ok = sw.step()
            rows.append(_host(_tick_row(sw, ok, sw.last_fsm["safe"])))
    else:
        f, ego = sw.fsm_dev, sw.dev["ego_ids"]
        tables = [torch.zeros_like(sw.all), torch.zeros_like(sw.all)]   # ver(k - 2), ver(k - 1)
        for k in range(n):
            stamp = sw.t0 + k * driver.TICK_PERIOD
            f.inputs(sw.own, sw.goals, stamp, sw.hover, sw.now, sw.t_start, sw.pva, sw.poses)
            sw.map.updateWorld(sw.compute.world(k), sw.poses, sw.now)
            sw.map.addOtherAgents(tables[0], A, ego)
            safe = sw.map.isTrajSafe(sw.own, sw.now, driver.COLLI_CHECK_DURATION)
            sw.planner.set_due(f.due)
            sw.planner.setSwarm(tables[0], A, ego, sw.now)
            sw.planner.replan(sw.pva, sw.goals, sw.t_start, ego, sw.new, sw.ok)
            f.apply(sw.ok, safe, sw.new, ego, sw.own, stamp)
            rows.append(_host(_tick_row(sw, sw.ok, safe)))
            tables = [tables[1], sw.own.clone()]
            sw.tick += 1
    torch.cuda.synchronize()
    assert sw.planner.flow_failures() == (0, 0)
    out = {"log": _stack(rows), "counters": sw.planner.counters(), "audit": sw.audit_report()}
    sw.close()
    return out


def _search_stats(sw, abi):
    import ctypes as C
    lib = abi.lib()
    lib.sogm_debug_planner_buffer.restype = C.c_int
    lib.sogm_debug_planner_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    stats = np.zeros((sw.A_loc, 4), np.int32)   # {nodes, expansions, path nodes, searches} of every agent's last search
    assert lib.sogm_debug_planner_buffer(sw.planner._p, 10, stats.ctypes.data_as(C.c_void_p), stats.nbytes) == 0
    return stats


def _flight(A, chunks, max_failures=None, audit=False, **kw):
    import torch
    driver, fsm, abi = _mods()
    sw = _swarm(driver, fsm, A, max_failures, audit=audit, **kw)
    logs = []
    for n in chunks:
        sw.fly(n)
        torch.cuda.synchronize()
        ms, hdr = sw.planner.flight_stats()
        assert hdr[abi.FLIGHT_HDR_ERR] == 0 and sw.planner.flow_failures() == (0, 0), (hdr.tolist(), sw.planner.flow_failures())
        assert hdr[abi.FLIGHT_HDR_FINISHED] == A * n and (ms[:, 7] == n).all(), (hdr.tolist(), ms[:, 7])
        assert hdr[abi.FLIGHT_HDR_LATE_WGS] == 0, hdr.tolist()
        logs.append(_host({k: sw.flight_fsm_log[k] for k in KEYS}))
    out = {"log": {k: np.concatenate([g[k] for g in logs]) for k in KEYS}, "counters": sw.planner.counters(),
           "state": sw.fsm_dev.state.cpu().numpy().copy(), "own": sw.own.cpu().numpy().copy(),
           "table": sw.all.cpu().numpy().copy(), "stats": _search_stats(sw, abi), "audit": sw.audit_report(),
           "views": (sw.status.cpu().numpy().copy(), sw.fail.cpu().numpy().copy(), sw.traj_start.cpu().numpy().copy()),
           "last_fsm": _host({k: v for k, v in sw.last_fsm.items() if k != "now"})}
    sw.close()
    return out


def _once(run):
    """every shared run is computed once (none of the tests changes what it gets) — and STARTED once: a run that raised
    is not flown again for the next test that shares it, which gets the same exception"""
    box = []

    @functools.wraps(run)
    def shared():
        if not box:
            try:
                box.append((run(), None))
            except BaseException as e:   # (a failed flight must not reach the GPU a second time)
                box.append((None, e))
        out, err = box[0]
        if err is not None:
            raise err
        return out
    return shared


@_once
def lock_lag1():
    return _lockstep(A_MAIN, N_MAIN, 1, audit=True)


@_once
def lock_lag2():
    return _lockstep(A_MAIN, N_MAIN, 2)


@_once
def lock_hover():
    return _lockstep(A_HOVER, N_HOVER, 2, max_failures=0, seed=SEED_HOVER)


@_once
def flight_lag1():
    return _flight(A_MAIN, [N_MAIN], audit=True, tuning={"flight_neighbour_lag": 1})


@_once
def flight_lag2():
    return _flight(A_MAIN, [N_MAIN])


def _same_logs(got, want, what):
    for key in KEYS:
        g, w = got[key], want[key]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        for k in range(g.shape[0]):
            assert g[k].tobytes() == w[k].tobytes(), (what, key, f"tick {k}", "agents",
                                                      np.flatnonzero((g[k] != w[k]).reshape(g.shape[1], -1).any(axis=1)))


def test_the_references_staleness_equals_step_tick_for_tick(pop):
    """flight_neighbour_lag = 1 against SwarmTick.step() flown lock-step: executed records, state records (status, fail,
    traj_start, success), due, safe, reached, pub, hover_start, the masked ok and the replan's output records after every
    tick, and the outcome counters after the run"""
    fl, lk = flight_lag1(), lock_lag1()
    _same_logs(fl["log"], lk["log"], "lag 1")
    assert fl["counters"] == lk["counters"]
    # the driver's views of the state after the flight, and its last_fsm
    status, fail, traj_start = fl["views"]
    last = lk["log"]["state"][-1].view([("traj_start", "<f8"), ("status", "<i4"), ("fail", "<i4"), ("success", "<i4"),
                                        ("r", "<i4")]).reshape(-1)
    assert (status == last["status"]).all() and (fail == last["fail"]).all() and (traj_start == last["traj_start"]).all()
    assert fl["own"].tobytes() == lk["log"]["own"][-1].tobytes() and fl["table"].tobytes() == fl["own"].tobytes()
    for key in ("due", "safe", "reached", "ok", "hover_start"):
        assert fl["last_fsm"][key].tobytes() == lk["log"][key][-1].tobytes(), key
    assert (fl["last_fsm"]["pub_hover"] == (lk["log"]["pub"][-1] == 2)).all()
    assert (fl["last_fsm"]["pub_new"] == (lk["log"]["pub"][-1] == 1)).all()


def test_the_flights_own_rule_equals_the_rule_flown_lockstep(pop):
    """the default lag (ver(k - 2)) against _lockstep(lag = 2)"""
    fl, lk = flight_lag2(), lock_lag2()
    _same_logs(fl["log"], lk["log"], "lag 2")
    assert fl["counters"] == lk["counters"]
    assert fl["state"].tobytes() == lk["log"]["state"][-1].tobytes()


def test_the_runs_cover_the_machine(pop):
    """on the LOCK-STEP logs: an agent-tick that was not due, EXEC_TRAJ and REPLAN, an unsafe verdict — and, in the swarm
    with replan_max_failures = 0, a hover record, which the flight reproduces byte for byte as well"""
    _, _, abi = _mods()
    hover_l = lock_hover()
    n = {"not_due": 0, "unsafe": 0, "hover": 0}
    states = set()
    for run in (lock_lag1(), lock_lag2(), hover_l):
        log = run["log"]
        n["not_due"] += int((log["due"] == 0).sum())
        n["unsafe"] += int((log["safe"] == 0).sum())
        n["hover"] += int((log["pub"] == abi.FSM_PUB_HOVER).sum())
        states |= set(log["state"][:, :, 8:12].copy().view(np.int32).reshape(-1).tolist())
    print("lock-step coverage: not due", n["not_due"], "states", sorted(states), "unsafe", n["unsafe"], "hover", n["hover"])
    assert n["not_due"] > 0 and {1, 2} <= states and n["unsafe"] > 0
    assert int((hover_l["log"]["pub"] == abi.FSM_PUB_HOVER).sum()) > 0
    hover_f = _flight(A_HOVER, [N_HOVER], max_failures=0, seed=SEED_HOVER)
    _same_logs(hover_f["log"], hover_l["log"], "replan_max_failures = 0")
    assert hover_f["counters"] == hover_l["counters"]


def test_counters_move_per_due_agent_tick_and_the_last_ticks_idle_agents_did_not_search(pop):
    """the outcome counters move once per DUE agent-tick of the whole flight; the search statistics are checked for the
    flight's LAST tick only (sogm_debug_planner_buffer keeps each agent's last search): an agent that was not due then has
    the statistics of no search"""
    fl = flight_lag2()
    due = fl["log"]["due"]
    outcome = ("replan_ok", "fail_search", "fail_corridor", "fail_qp", "fail_unsafe")
    assert sum(fl["counters"][k] for k in outcome) == int((due != 0).sum())
    assert 0 < int((due != 0).sum()) < due.size
    idle = np.flatnonzero(due[-1] == 0)
    assert idle.size > 0
    for a in range(A_MAIN):
        if a in idle:
            assert fl["stats"][a].tolist() == [0, 0, 0, 0], (a, fl["stats"][a])
        else:
            assert fl["stats"][a][3] >= 1, (a, fl["stats"][a])


def test_a_flight_under_the_fsm_continues_a_flight(pop):
    one, two = _flight(5, [9]), _flight(5, [1, 3, 5])
    _same_logs(two["log"], one["log"], "chunks")
    assert one["state"].tobytes() == two["state"].tobytes() and one["table"].tobytes() == two["table"].tobytes()
    assert one["own"].tobytes() == two["own"].tobytes()


def test_the_schedule_does_not_change_the_logs(pop):
    base = _flight(6, [6])
    for tuning in ({"flight_spec": 0}, {"flight_urgent": 0},
                   {"flight_qp_units": 2, "flight_search_units": 1, "flight_map_units": 6}):
        other = _flight(6, [6], tuning=tuning)
        _same_logs(other["log"], base["log"], tuning)
        assert other["state"].tobytes() == base["state"].tobytes(), tuning


def test_off_means_off(pop):
    """one planner: the mode registered, a flight, one sogm_replan tick WITH the mode still registered, NULL, then a fresh
    flight and one more sogm_replan tick — the plain flight and both replan ticks equal those of a planner that never saw
    the mode"""
    import torch
    driver, fsm, abi = _mods()
    A, n = 5, 4

    def flight(sw):
        tables = torch.zeros((4, A, abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
        own, hover = torch.zeros_like(sw.own), sw.hover.clone()
        log_r = torch.zeros((n, A, abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
        log_ok = torch.zeros((n, A), dtype=torch.int32, device="cuda")
        worlds = [sw.compute.world(i) for i in range(n)]
        sw.planner.flight(worlds, 0, sw.t0, driver.TICK_PERIOD, driver.REPLAN_START_TIME, sw.goals, sw.dev["ego_ids"],
                          hover, own, tables, log_r, log_ok)
        torch.cuda.synchronize()
        ms, hdr = sw.planner.flight_stats()
        assert hdr[abi.FLIGHT_HDR_ERR] == 0 and hdr[abi.FLIGHT_HDR_FINISHED] == A * n and hdr[abi.FLIGHT_HDR_LATE_WGS] == 0
        assert sw.planner.flow_failures() == (0, 0)
        return [t.cpu().numpy().copy() for t in (log_r, log_ok, own)]

    def replan_tick(sw):
        """one lock-step tick through sogm_replan, from rest"""
        own, hover = torch.zeros_like(sw.own), sw.hover.clone()
        c = sw.compute
        c.tick_inputs(own, sw.t0, hover, sw.now, sw.t_start, sw.pva, sw.poses)
        c.update_map(sw.poses, sw.now, torch.zeros_like(sw.all), A, 0)
        new, ok = torch.zeros_like(sw.own), torch.zeros((A,), dtype=torch.int32, device="cuda")
        sw.planner.setSwarm(None, 0, None, None)
        sw.planner.replan(sw.pva, sw.goals, sw.t_start, sw.dev["ego_ids"], new, ok)
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (new, ok)]

    never = driver.SwarmTick("parity", A, moving_world=True, prestamp=False)
    want = flight(never) + replan_tick(never)
    never.close()
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False)
    f = fsm.FsmState(A, sw.t0 - 2.0, fsm.make_params(driver.TICK_PERIOD, driver.REPLAN_START_TIME, driver.GOAL_TOLERANCE,
                                                     1.0, driver.REPLAN_MAX_FAILURES))
    logs = f.flight_logs(n)
    sw.planner.set_flight_fsm(f.prm, driver.COLLI_CHECK_DURATION, f.state, logs)
    flight(sw)
    assert int((logs["due"] == 0).sum()) > 0            # the mode was on: somebody was spared a replan
    between = replan_tick(sw)                           # the mode still registered: sogm_replan never looks at it
    sw.planner.set_flight_fsm(None)
    sw.planner.counters(reset=True)
    got = flight(sw) + replan_tick(sw)
    sw.close()
    names = ("log_records", "log_ok", "own", "replan records", "replan ok")
    for g, w, name in zip(got, want, names):
        assert g.tobytes() == w.tobytes(), name
    for g, w, name in zip(between, want[3:], names[3:]):
        assert g.tobytes() == w.tobytes(), (name, "with the mode registered")


def test_refusals(pop):
    import ctypes as C
    import torch
    driver, fsm, abi = _mods()
    A = 4
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False)
    lib = abi.lib()
    prm = fsm.make_params()
    bad = abi.SogmFlightFsm(prm, 0.2, None, None, None, None, None, None, None, None)
    assert lib.sogm_planner_set_flight_fsm(sw.planner._p, C.byref(bad)) == abi.SOGM_ERR_INVALID_ARG
    assert b"state_inout" in lib.sogm_last_error()
    state = torch.zeros((A, abi.FSM_STATE_BYTES), dtype=torch.uint8, device="cuda")
    nan = abi.SogmFlightFsm(prm, float("nan"), state.data_ptr(), None, None, None, None, None, None, None)
    assert lib.sogm_planner_set_flight_fsm(sw.planner._p, C.byref(nan)) == abi.SOGM_ERR_INVALID_ARG
    assert b"finite" in lib.sogm_last_error()
    neg = abi.SogmFlightFsm(fsm.make_params(replan_duration=-0.1), 0.2, state.data_ptr(), None, None, None, None, None,
                            None, None)
    assert lib.sogm_planner_set_flight_fsm(sw.planner._p, C.byref(neg)) == abi.SOGM_ERR_INVALID_ARG
    # the mode on, a flight over more rows than the batch has agents
    sw.planner.set_flight_fsm(prm, 0.2, state)
    tables = torch.zeros((4, A + 2, abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    log_r = torch.zeros((1, A, abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device="cuda")
    log_ok = torch.zeros((1, A), dtype=torch.int32, device="cuda")
    with pytest.raises(abi.SogmError) as e:
        sw.planner.flight([sw.compute.world(0)], 0, sw.t0, driver.TICK_PERIOD, driver.REPLAN_START_TIME, sw.goals,
                          sw.dev["ego_ids"], sw.hover, sw.own, tables, log_r, log_ok, n_total=A + 2, agent0=0)
    assert "n_total" in str(e.value)
    sw.planner.set_flight_fsm(None)
    sw.close()
    # the torch machines have no flight
    host = driver.SwarmTick("parity", A, moving_world=True, prestamp=False, fsm=True)
    with pytest.raises(AssertionError):
        host.fly(1)
    host.close()


def test_the_audit_of_a_flight_under_the_fsm_equals_the_lockstep_audit(pop):
    """SwarmTick(..., audit=True).fly() audits the log's executed tables: the same tables as the lock-step run of the
    first test audited tick by tick, so the same report"""
    fl, lk = flight_lag1(), lock_lag1()
    assert fl["audit"] is not None and fl["audit"] == lk["audit"]
    assert fl["audit"]["ticks"] == N_MAIN
