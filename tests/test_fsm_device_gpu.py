"""The FSM on the device (sogm_fsm_init / sogm_fsm_inputs / sogm_fsm_apply, csrc/sogm_fsm.hip) and the due gate of
sogm_replan (sogm_planner_set_due): the kernels against the independent restatement of FSMCallback
(tests/golden/fsm_independent.json), the inputs kernel against the torch expressions of SwarmTick.step_fsm, masked against
unmasked replans in both forms of sogm_replan, and the closed loop with the machines on the device against step_fsm."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "fsm_independent.json")))
CODE = {"NEW_PLAN": 0, "EXEC_TRAJ": 1, "REPLAN": 2, "GOAL_REACHED": 3}

pytestmark = pytest.mark.gpu


def _mods():
    return (importlib.import_module("pred-occ-planner_amd.driver"), importlib.import_module("pred-occ-planner_amd.fsm"),
            importlib.import_module("pred-occ-planner_amd.planner"), importlib.import_module("pred-occ-planner_amd._abi"))


def _state_array(n):
    return np.zeros(n, dtype=np.dtype([("traj_start", "<f8"), ("status", "<i4"), ("fail", "<i4"), ("success", "<i4"),
                                       ("reserved_", "<i4")]))


def test_fsm_kernels_equal_the_independent_restatement(pop):
    """130 rows (the fixture's 24 agents repeated: two full waves and a partial one of the one-lane-per-agent kernels)
    fed the fixture's ok / safe / reached tick by tick: status, failure count, traj_start_time_, the publication kind
    and the hover start of EVERY tick equal the fixture; what sogm_fsm_inputs says is due follows from the fixture's
    previous state; a hover record is driver.hover_records' bytes, a new record the tick's, anything else untouched."""
    driver, fsm, _, abi = _mods()
    n, agents = 130, FX["agents"]
    rows = [agents[r % len(agents)] for r in range(n)]
    n_ticks = max(len(t) for t in agents)
    assert sum(len(t) for t in agents) == 2879
    dev, g = "cuda", torch.Generator().manual_seed(7)
    f = fsm.FsmState(n, FX["traj_start0"], fsm.make_params(FX["replan_duration"], FX["replan_start_time"], 1.0, 1.0,
                                                           FX["replan_max_failures"]))
    ids = torch.arange(n, dtype=torch.int32, device=dev) + 3
    own = torch.zeros((n, abi.TRAJ_RECORD_BYTES), dtype=torch.uint8, device=dev)
    goals = torch.full((n, 3), 1.0e3, dtype=torch.float64, device=dev)
    hover = torch.cat([torch.randn((n, 3), generator=g, dtype=torch.float64), torch.zeros((n, 6), dtype=torch.float64)],
                      dim=1).to(dev)
    now, t_start = (torch.zeros((n,), dtype=torch.float64, device=dev) for _ in range(2))
    pva = torch.zeros((n, 9), dtype=torch.float64, device=dev)
    poses = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    prev = [(CODE["NEW_PLAN"], FX["traj_start0"])] * n
    seen = set()
    for k in range(n_ticks):
        stamp = agents[0][k][0]
        live = [k < len(t) for t in rows]   # an agent whose sequence ended at GOAL_REACHED stays there
        tick = [t[k] if k < len(t) else [stamp, 0, 1, 0, t[-1][4], t[-1][5], t[-1][6], None] for t in rows]
        assert all(t[0] == stamp for t in tick)
        ok, safe, reached = (torch.tensor([t[c] for t in tick], dtype=torch.int32, device=dev) for c in (1, 2, 3))
        # the tick's "new" records: valid one-piece records, different every tick
        new = driver.hover_records(ids, torch.full((n,), stamp + 0.25, dtype=torch.float64, device=dev),
                                   torch.randn((n, 3), generator=g, dtype=torch.float64).to(dev))
        before = own.clone()
        f.inputs(own, goals, stamp, hover, now, t_start, pva, poses)
        f.apply(ok, safe, new, ids, own, stamp, reached=reached)
        want_hover = driver.hover_records(ids, f.hover_start, f.pos_now).cpu().numpy()
        got_own, new_h, before_h = own.cpu().numpy(), new.cpu().numpy(), before.cpu().numpy()
        st, fl, ts = f.status.cpu().numpy(), f.fail.cpu().numpy(), f.traj_start.cpu().numpy()
        due, pub, hs = f.due.cpu().numpy(), f.pub.cpu().numpy(), f.hover_start.cpu().numpy()
        assert (now.cpu().numpy() == stamp).all()
        for r, (_, _, _, _, status, fails, tstart, p) in enumerate(tick):
            want_due = (1 if prev[r][0] == 0 and (stamp - prev[r][1]) > 1.0 else 0) | (2 if prev[r][0] == 2 else 0)
            assert int(due[r]) == want_due, (k, r)
            assert (int(st[r]), int(fl[r]), float(ts[r])) == (CODE[status], fails, tstart), (k, r)
            if p is None:
                assert pub[r] == abi.FSM_PUB_NONE and got_own[r].tobytes() == before_h[r].tobytes(), (k, r)
            elif p[0] == "new":
                assert pub[r] == abi.FSM_PUB_NEW and got_own[r].tobytes() == new_h[r].tobytes(), (k, r)
            else:
                assert pub[r] == abi.FSM_PUB_HOVER and float(hs[r]) == p[1], (k, r)
                assert got_own[r].tobytes() == want_hover[r].tobytes(), (k, r)
                seen.add("hover")
            if live[r]:
                seen.add(status)
            prev[r] = (CODE[status], tstart)
    assert {"NEW_PLAN", "EXEC_TRAJ", "REPLAN", "GOAL_REACHED", "hover"} <= seen


def test_fsm_inputs_equal_the_torch_path(pop):
    """sogm_fsm_inputs against lines 505-513 and 522 of SwarmTick.step_fsm on own records of three real replan ticks (one
    agent executes nothing) and machines in every state: start states, start times, map centres, the refreshed hover
    and who is due bit for bit; `reached` wherever the distance to the goal is further than 1e-9 from the tolerance."""
    driver, fsm, planner, abi = _mods()
    A = 8
    sw = driver.SwarmTick("parity", A, prestamp=False)
    for _ in range(3):
        sw.step()
    own = sw.own.clone()
    own[5] = 0                                    # n_pieces == 0: hovers
    n_pieces = np.array([r.n_pieces for r in planner.records_from_bytes(own.cpu().numpy())])
    assert (n_pieces[np.arange(A) != 5] > 0).sum() >= 4 and n_pieces[5] == 0
    stamp = sw.t0 + 3 * driver.TICK_PERIOD
    now = torch.full((A,), stamp, dtype=torch.float64, device="cuda")
    hover0 = sw.hover.clone()
    sa = _state_array(A)
    sa["status"] = [0, 0, 1, 2, 3, 2, 1, 0]
    sa["traj_start"] = [stamp - 1.5, stamp - 0.5, stamp - 0.2, stamp - 0.1, stamp - 3.0, stamp, stamp, stamp - 1.0]
    f = fsm.FsmState(A, 0.0, fsm.make_params(driver.TICK_PERIOD, driver.REPLAN_START_TIME, driver.GOAL_TOLERANCE, 1.0,
                                             driver.REPLAN_MAX_FAILURES))
    f.state.copy_(torch.from_numpy(sa.view(np.uint8).reshape(A, abi.FSM_STATE_BYTES)).cuda())
    # ---- the torch path (step_fsm) ----
    status = torch.from_numpy(sa["status"].copy()).cuda()
    traj_start = torch.from_numpy(sa["traj_start"].copy()).cuda()
    due_new, is_rep, t_start = driver.fsm_plan_inputs(status, traj_start, now)
    pva_now, valid_now = planner.traj_eval(own, now)
    pva_now = torch.where(valid_now.bool().unsqueeze(1), pva_now, hover0)
    pva, valid = planner.traj_eval(own, t_start)
    pva = torch.where(valid.bool().unsqueeze(1), pva, hover0).contiguous()
    hover_want = torch.cat([pva_now[:, :3], torch.zeros_like(pva_now[:, 3:])], dim=1)
    # goals: inside the tolerance for three agents (the hovering one among them), the scene's far ones for the rest
    goals = sw.goals.clone()
    off = torch.tensor([[0.3, -0.2, 0.1], [0.9, 0.0, 0.3], [0.0, 0.6, -0.6]], dtype=torch.float64, device="cuda")
    goals[[1, 5, 6]] = pva_now[[1, 5, 6], :3] + off
    dist = (pva_now[:, :3] - goals).norm(dim=1)
    assert ((dist - driver.GOAL_TOLERANCE).abs() > 1e-9).all()          # nobody inside the band: the reference alone
    reached_want = dist < driver.GOAL_TOLERANCE
    assert 0 < int(reached_want.sum()) < A
    # ---- the kernel ----
    hover = hover0.clone()
    o_now, o_ts = (torch.zeros((A,), dtype=torch.float64, device="cuda") for _ in range(2))
    o_pva = torch.zeros((A, 9), dtype=torch.float64, device="cuda")
    o_poses = torch.zeros((A, 3), dtype=torch.float32, device="cuda")
    f.inputs(own, goals, stamp, hover, o_now, o_ts, o_pva, o_poses)
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert same(o_pva, pva) and same(o_ts, t_start) and same(o_now, now)
    assert same(o_poses, pva_now[:, :3].to(torch.float32).contiguous())
    assert same(hover, hover_want) and same(f.pos_now, pva_now[:, :3].contiguous())
    assert torch.equal(f.due != 0, due_new | is_rep)
    assert torch.equal(f.due, due_new.to(torch.int32) + 2 * is_rep.to(torch.int32))
    assert {0, 1, 2} <= set(f.due.cpu().tolist())
    assert torch.equal(f.reached.bool(), reached_want)
    sw.close()


def _due_gate(driver, abi, want_grouped, **swarm_kwargs):
    """one tick's replan three times on identically rebuilt maps: every agent, a mixed mask, nobody.  A publish target is
    set (sogm_planner_set_publish): `own` holds a hover record per agent before every call, `table` is poisoned"""
    import ctypes as C
    A = 8
    sw = driver.SwarmTick("parity", A, **swarm_kwargs)
    # the form under test is the one that runs: overlap mode 1 (the in-place clear) takes the grouped-stream chain,
    # every other mode the dataflow replan (sogm_replan)
    assert (sw.overlap_mode == 1) == want_grouped, sw.overlap_mode
    c, P = sw.compute, sw.planner
    lib = abi.lib()
    lib.sogm_debug_planner_buffer.restype = C.c_int
    lib.sogm_debug_planner_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    stamp = sw.t0
    outcome = ("replan_ok", "fail_search", "fail_corridor", "fail_qp", "fail_unsafe")
    ids = sw.dev["ego_ids"]
    executing = driver.hover_records(ids, torch.full((A,), stamp - 0.3, dtype=torch.float64, device="cuda"),
                                     sw.hover[:, :3].clone())
    res = []
    try:
        for mask in (None, [1, 0, 1, 1, 0, 0, 1, 0], [0] * A):
            hover = sw.hover.clone()
            c.tick_inputs(sw.own, stamp, hover, sw.now, sw.t_start, sw.pva, sw.poses)
            c.update_map(sw.poses, sw.now, sw.all, sw.A_tot, 0)
            due = None if mask is None else torch.tensor(mask, dtype=torch.int32, device="cuda")
            new = torch.full((A, abi.TRAJ_RECORD_BYTES), 0xA5, dtype=torch.uint8, device="cuda")
            ok = torch.full((A,), 7, dtype=torch.int32, device="cuda")
            own = executing.clone()
            table = torch.full((A, abi.TRAJ_RECORD_BYTES), 0x5A, dtype=torch.uint8, device="cuda")
            P.counters(reset=True)
            P.setPublish(own, table)
            P.set_due(due)
            c.replan(sw.pva, sw.goals, sw.t_start, new, ok)
            cnt = P.counters()
            err = P.flow_error()
            stats = np.zeros((A, 4), np.int32)   # the search's {nodes, expansions, path nodes, searches} per agent
            assert lib.sogm_debug_planner_buffer(P._p, 10, stats.ctypes.data_as(C.c_void_p), stats.nbytes) == 0
            res.append({"mask": mask, "new": new.cpu().numpy(), "ok": ok.cpu().numpy(), "own": own.cpu().numpy(),
                        "table": table.cpu().numpy(), "counted": sum(cnt[k] for k in outcome), "err": err, "stats": stats})
    finally:
        P.set_due(None)
        P.setPublish(None, None)
        sw.close()
    return res, executing.cpu().numpy()


@pytest.mark.parametrize("form", ["flow", "grouped"])
def test_replan_plans_only_the_agents_that_are_due(pop, form):
    """sogm_planner_set_due in the dataflow replan and in the grouped-stream form (the in-place clear's, grids=1): the
    records and ok of the due agents are those of the unmasked call bit for bit, the others report ok = 0, an empty
    record and the statistics of no search (0 nodes, 0 expansions, 0 searches); the outcome counters move by exactly
    the number of due agents; a tick in which nobody is due ends without a flow error.  With a publish target set, the
    rows of an agent that is not due are what a failed replan leaves: its own record untouched, the table's row a copy
    of it."""
    driver, _, planner, abi = _mods()
    res, executing = _due_gate(driver, abi, form == "grouped",
                               **({} if form == "flow" else {"overlap_clear": True, "grids": 1}))
    full = res[0]
    A = len(full["ok"])
    assert full["counted"] == A and full["err"] == 0 and set(full["ok"].tolist()) <= {0, 1} and full["ok"].sum() >= 1
    assert (full["stats"][:, 3] >= 1).all() and (full["stats"][:, 0] >= 1).all()   # unmasked: everybody searched
    for r in res:
        mask = r["mask"] if r["mask"] is not None else [1] * A
        assert r["err"] == 0, (form, mask, r["err"])
        assert r["counted"] == sum(mask), (form, mask, r["counted"])
        recs = planner.records_from_bytes(r["new"])
        for a in range(A):
            if mask[a]:
                assert r["ok"][a] == full["ok"][a] and r["new"][a].tobytes() == full["new"][a].tobytes(), (form, mask, a)
                assert (r["stats"][a] == full["stats"][a]).all(), (form, mask, a)
            else:
                assert r["ok"][a] == 0 and recs[a].n_pieces == 0, (form, mask, a)
                assert r["stats"][a].tolist() == [0, 0, 0, 0], (form, mask, a, r["stats"][a])
            # publication: latest wins where the replan succeeded, else the agent goes on executing its record
            want_own = r["new"][a] if (mask[a] and r["ok"][a]) else executing[a]
            assert r["own"][a].tobytes() == want_own.tobytes(), (form, mask, a)
            assert r["table"][a].tobytes() == want_own.tobytes(), (form, mask, a)
    assert any(full["ok"][a] == 1 for a in range(A) if res[1]["mask"][a])      # a due agent of the mixed mask did plan


def test_closed_loop_with_the_machines_on_the_device(pop):
    """25 ticks of SwarmTick("parity", 8, fsm=True) with the torch state machines (step_fsm, which replans everybody and
    discards) and with device_fsm=True (sogm_fsm_inputs -> ... -> replan of the due agents -> sogm_fsm_apply): executed
    records, state, failure counter, traj_start_time_ and the masked ok are bit-identical after every tick."""
    driver, _, _, _ = _mods()
    A, ticks = 8, 25

    def fly(**kw):
        sw = driver.SwarmTick("parity", A, fsm=True, **kw)
        log = []
        for _ in range(ticks):
            ok = sw.step()
            log.append({"own": sw.own.cpu().numpy().copy(), "status": sw.status.cpu().numpy().copy(),
                        "fail": sw.fail.cpu().numpy().copy(), "traj_start": sw.traj_start.cpu().numpy().copy(),
                        "ok": ok.cpu().numpy().copy(),
                        "due": sw.last_fsm["due"].cpu().numpy().copy() if "due" in sw.last_fsm else None})
        sw.close()
        return log

    host, dev = fly(), fly(device_fsm=True)
    for k in range(ticks):
        for key in ("own", "status", "fail", "traj_start", "ok"):
            assert host[k][key].dtype == dev[k][key].dtype and host[k][key].tobytes() == dev[k][key].tobytes(), (k, key)
    assert any((t["due"] == 0).any() for t in dev)                      # somebody was spared a replan
    seen = {int(s) for t in dev for s in t["status"]}
    assert {driver.FSM_EXEC_TRAJ, driver.FSM_REPLAN} <= seen


def test_facade_fsm_on_gpu(tmp_path):
    """sogm_host::Fsm and Planner::setDue (host/sogm_facade.hpp) run from C++: tests/facade_fsm_gpu_test.cpp, compiled
    with hipcc like tests/test_facade_host.py's programs."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "facade_fsm_gpu_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "facade_fsm_gpu_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")], timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "facade fsm ok" in out.stdout
