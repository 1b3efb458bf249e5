"""GPU: the flight audit (sogm_swarm_audit, audit.SwarmAudit, SwarmTick(audit=True)) against the numpy restatement of
tests/swarm_audit_reference.py: closed-form cases, a real swarm (lock-step and FSM), incremental and rank-split calls,
the event capacity, flight = lock-step, audit on = audit off for the records, and the full-size swarm."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swarm_audit_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

INT_KEYS = ("min_gap_obstacle", "min_sep_agent", "obstacle_samples", "agent_samples", "n_samples", "has_last")
F_KEYS = ("min_gap", "min_gap_time", "min_sep", "min_sep_time", "goal_time", "first_collision_time", "path_length")


def _mods():
    return (importlib.import_module("pred-occ-planner_amd.audit"), importlib.import_module("pred-occ-planner_amd._abi"),
            importlib.import_module("pred-occ-planner_amd.driver"))


def _cyl_struct(abi, rows7):
    rows7 = np.asarray(rows7, np.float64).reshape(-1, 7)
    arr = (abi.SogmCylinder * len(rows7))()
    for c, (x, y, z, w, h, vx, vy) in zip(arr, rows7):
        c.type, c.x, c.y, c.z, c.w, c.h, c.vx, c.vy, c.qw = 3, x, y, z, w, h, vx, vy, 1.0
    return arr


def _device_audit(tables, prev, fallback, goals, cyl7, t0, first_tick, period, t_obs, agent0=0, n_local=None,
                  splits=None, capacity=4096):
    """audit on the device; splits: tick counts of successive calls (default one call).  Returns (per_agent, events, n)."""
    import torch
    audit, abi, _ = _mods()
    tables = np.asarray(tables, np.uint8)
    n_total = tables.shape[1]
    n_local = n_total - agent0 if n_local is None else n_local
    a = audit.SwarmAudit(n_total, np.asarray(goals)[agent0:agent0 + n_local], fallback, _cyl_struct(abi, cyl7), t_obs,
                         agent0=agent0, n_local=n_local, event_capacity=capacity)
    dev = torch.from_numpy(tables).cuda()
    k = 0
    for n in (splits or [len(tables)]):
        a.add(dev[k:k + n], t0, first_tick + k, period,
              prev_table=torch.from_numpy(np.asarray(prev, np.uint8)).cuda() if (k == 0 and prev is not None) else None)
        k += n
    ev, n, _ = a.event_list()
    return a.per_agent(), ev, n


def _compare(got, ev, n, want, wev, what, exact_events=True):
    for key in INT_KEYS:
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    for key in F_KEYS:
        g, w = got[key], want[key]
        assert np.array_equal(np.isinf(g), np.isinf(w)), (what, key, g, w)
        fin = np.isfinite(w)
        np.testing.assert_allclose(g[fin], w[fin], rtol=0, atol=1e-12, err_msg=f"{what} {key}")
    np.testing.assert_allclose(got["last_pos"], want["last_pos"], rtol=0, atol=1e-12)
    assert n == len(wev), (what, n, len(wev))
    if exact_events:
        kept = [(int(e["agent"]), int(e["other"]), int(e["kind"])) for e in ev]
        assert kept == [(e[1], e[2], e[3]) for e in wev[:len(ev)]], what
        np.testing.assert_allclose(ev["t"], [e[0] for e in wev[:len(ev)]], rtol=0, atol=1e-12)


@pytest.mark.parametrize("case", ref.closed_form_cases(), ids=lambda c: c["name"])
def test_closed_form_cases_on_the_device(pop, case):
    c = case
    want, wev, _ = ref.run_case(c)
    got, ev, n = _device_audit(c["tables"], c["prev_table"], c["fallback"], c["goals"], c["cyl"], c["t0"], c["first_tick"],
                               c["period"], c["t_obstacles"])
    _compare(got, ev, n, want, wev, c["name"])
    ref.check_expect(c, {k: got[k] for k in got.dtype.names}, [(float(e["t"]), 0, 0, 0) for e in ev])


def _swarm_tables(driver, n_ticks, fsm=False, A=8, grid="parity"):
    """a swarm with the audit on: its executed table after every tick, its report and per-agent accumulators"""
    import torch
    sw = driver.SwarmTick(grid, A, moving_world=True, prestamp=False, fsm=fsm, audit=True)
    tabs = []
    for _ in range(n_ticks):
        sw.step()
        tab = sw.own if fsm else sw.records_all()
        tabs.append(tab.cpu().numpy().copy())
    torch.cuda.synchronize()
    rep, acc = sw.audit_report(), sw.auditor.per_agent()
    scene, t0, tl = sw.scene, sw.t0, sw.compute.timeline
    sw.close()
    return np.stack(tabs), rep, acc, scene, t0, tl


def _reference_of(tables, scene, t0, tl):
    cyl = ref.cylinders(tl.cylinders(0))
    want, wev, margins = ref.audit(tables, None, scene["starts"], scene["goals"], cyl, t0, 0, 0.1, 0, tables.shape[1],
                                   t_obstacles=t0)
    return cyl, want, wev, margins


@pytest.mark.parametrize("fsm", [False, True], ids=["lockstep", "fsm"])
def test_real_swarm_equals_the_reference(pop, fsm):
    _, _, driver = _mods()
    tables, rep, acc, scene, t0, tl = _swarm_tables(driver, 40, fsm=fsm)
    cyl, want, wev, margins = _reference_of(tables, scene, t0, tl)
    close = ref.near_threshold(margins)
    print(f"fsm={fsm}: report {dict((k, v) for k, v in rep.items() if k != 'events')}; decisions within 1e-9: {close}")
    assert close == 0, f"{close} decisions within 1e-9 of their threshold"
    got, ev, n = _device_audit(tables, None, scene["starts"], scene["goals"], cyl, t0, 0, 0.1, t0)
    _compare(got, ev, n, want, wev, f"swarm fsm={fsm}")
    # the driver's own audit (one call per tick) gives the same
    assert acc.tobytes() == got.tobytes()
    assert rep["n_events"] == n and rep["ticks"] == 40


def test_incremental_and_rank_split_equal_the_whole_call(pop):
    _, _, driver = _mods()
    tables, _, _, scene, t0, tl = _swarm_tables(driver, 40)
    cyl = ref.cylinders(tl.cylinders(0))
    args = (tables, None, scene["starts"], scene["goals"], cyl, t0, 0, 0.1, t0)
    whole, ev_w, n_w = _device_audit(*args)
    inc, ev_i, n_i = _device_audit(*args, splits=[5] * 8)
    assert whole.tobytes() == inc.tobytes() and ev_w.tobytes() == ev_i.tobytes() and n_w == n_i
    lo, _, _ = _device_audit(*args, agent0=0, n_local=4)
    hi, _, _ = _device_audit(*args, agent0=4, n_local=4)
    assert np.concatenate([lo, hi]).tobytes() == whole.tobytes()


def test_capacity_keeps_the_earliest_events(pop):
    c = [c for c in ref.closed_form_cases() if c["name"] == "head_on"][0]
    _, wev, _ = ref.run_case(c)
    args = (c["tables"], None, c["fallback"], c["goals"], c["cyl"], 0.0, 0, 0.1, 0.0)
    full, ev_f, n_f = _device_audit(*args)
    part, ev_p, n_p = _device_audit(*args, capacity=7)
    assert n_f == n_p == len(wev) == 80 and len(ev_p) == 7
    assert ev_p.tobytes() == ev_f[:7].tobytes()
    assert full.tobytes() == part.tobytes()


def test_flight_audit_equals_the_lockstep_audit(pop):
    import torch
    _, _, driver = _mods()
    K, A = 10, 6
    lk = driver.SwarmTick("parity", A, moving_world=True, prestamp=False, neighbour_lag=2, audit=True)
    for _ in range(K):
        lk.step()
    torch.cuda.synchronize()
    rep_l, acc_l = lk.audit_report(), lk.auditor.per_agent()
    lk.close()
    fl = driver.SwarmTick("parity", A, moving_world=True, prestamp=False, audit=True)
    fl.fly(4)
    fl.fly(6)
    torch.cuda.synchronize()
    rep_f, acc_f = fl.audit_report(), fl.auditor.per_agent()
    fl.close()
    assert acc_f.tobytes() == acc_l.tobytes()
    assert rep_f == rep_l


def test_audit_off_changes_nothing(pop):
    import torch
    _, _, driver = _mods()
    out = []
    for audit in (False, True):
        sw = driver.SwarmTick("parity", 8, moving_world=True, prestamp=False, audit=audit)
        oks, recs = [], []
        for _ in range(20):
            oks.append(sw.step().cpu().numpy())
            recs.append(sw.new.cpu().numpy())
        torch.cuda.synchronize()
        out.append((np.stack(oks), np.stack(recs), sw.records_all().cpu().numpy()))
        sw.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_unsupported_obstacle_types_are_refused(pop):
    audit, abi, _ = _mods()
    arr = _cyl_struct(abi, [[0, 0, 2, 0.5, 4, 0, 0]])
    arr[0].type = 2
    with pytest.raises(ValueError):
        audit.SwarmAudit(1, [[0, 0, 1]], [[0, 0, 1]], arr, 0.0)


def test_full_size_swarm_equals_the_reference(pop):
    _, _, driver = _mods()
    tables, rep, acc, scene, t0, tl = _swarm_tables(driver, 60, A=128, grid="cfg2")
    _, want, wev, margins = _reference_of(tables, scene, t0, tl)
    close = ref.near_threshold(margins)
    print(f"cfg2 60 ticks: {dict((k, v) for k, v in rep.items() if k != 'events')}; decisions within 1e-9: {close}")
    assert close == 0, f"{close} decisions within 1e-9 of their threshold"
    _compare(acc, None, rep["n_events"], want, wev, "cfg2", exact_events=False)
