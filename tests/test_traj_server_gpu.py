"""GPU: the trajectory server (sogm_traj_server_run, sogm_camera_poses, trajserver.TrajServer, SwarmTick(traj_server=...)):
every case of the independent reading (tests/golden/traj_server_independent.json) through the kernel, call-split
invariance, agent indexing, argument validation, the hand-over of commanded camera poses to sogm_render_depth, and the
tick driver's hook, which must change nothing else in a tick."""
import ctypes as C
import importlib
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_render_reference as ref  # noqa: E402
import traj_server_fixture as tsf  # noqa: E402

pytestmark = pytest.mark.gpu
N_LOCAL = 5


def _mods():
    return (importlib.import_module("pred-occ-planner_amd"), importlib.import_module("pred-occ-planner_amd.trajserver"),
            importlib.import_module("pred-occ-planner_amd.driver"))


def _prm(ts, p):
    return ts.make_params(p["replan_threshold"], p["yaw_mode"], (p["yaw_pi"], p["yaw_dot_max"]), p["sample_dt"])


def _tables(rows):
    """numpy records [n_ticks][n] -> device uint8 [n_ticks][n][2064]"""
    import torch
    rows = np.ascontiguousarray(rows)
    return torch.from_numpy(rows.view(np.uint8).reshape(rows.shape + (tsf.REC_BYTES,))).cuda()


def _cmd_rows(cmds):
    return [[c["t_pub"], c["t_sample"], *c["pos"], *c["vel"], *c["acc"], c["yaw"], c["yaw_dot"], c["traj_id"], c["flags"]]
            for c in cmds]


def _live(state, ring):
    return [[ring[(state["head"] + i) & 255][k] for k in ("t", "yaw", "yaw_dot")] for i in range(int(state["size"]))]


# ---- 4. the fixture through the kernel ----
@pytest.mark.parametrize("case", tsf.CASES, ids=[c["name"] for c in tsf.CASES])
def test_fixture_through_the_kernel(case):
    import torch
    _, ts, _ = _mods()
    tab, rcv = tsf.case_tables(case)
    n_ticks = len(tab)
    srv = ts.TrajServer(N_LOCAL, np.tile(case["init_pos"], (N_LOCAL, 1)), case["t_trigger"],
                        init_yaw=np.full(N_LOCAL, case["init_yaw"]), prm=_prm(ts, case["prm"]),
                        receive_delay=case["receive_delay"])
    tables = _tables(np.repeat(tab[:, None], N_LOCAL, axis=1))
    received = None if case["infer"] else torch.from_numpy(np.repeat(rcv[:, None], N_LOCAL, axis=1)).cuda()
    srv.run(tables, case["t0"], case["first_tick"], case["period"], received=received)
    cmds = srv.commands
    st, rings = srv.states()
    assert cmds.shape == (N_LOCAL, n_ticks * case["m"])
    for a in range(N_LOCAL):
        final = {k: st[a][k] for k in ("ts", "te", "duration", "last_yaw", "last_yawdot", "size", "traj_id", "received",
                                       "overflow")}
        tsf.check(case, _cmd_rows(cmds[a]), None, final, _live(st[a], rings[a]))
        assert cmds[a].tobytes() == cmds[0].tobytes() and rings[a].tobytes() == rings[0].tobytes()


# ---- 5 / 6: a swarm of fixture records ----
def _swarm_rows(n, n_ticks):
    """agent a flies the records of fixture case a (mod the curved cases), a new one every second tick"""
    pool = [c for c in tsf.CASES if len(c["records"]) >= 2 and c["t0"] == 10.0]
    rows = np.zeros((n_ticks, n), tsf.REC_DTYPE)
    for a in range(n):
        recs = pool[a % len(pool)]["records"]
        for k in range(n_ticks):
            rows[k, a] = tsf.record_bytes(recs[min((k + a % 2) // 2, len(recs) - 1)], a)
    return rows


def _fly(ts, rows, splits, agent0=0, n_local=None, yaw_mode=1):
    import torch
    n = rows.shape[1]
    n_local = n - agent0 if n_local is None else n_local
    pos = np.stack([np.arange(n), -np.arange(n), np.ones(n)], axis=1).astype(np.float64)[agent0:agent0 + n_local]
    srv = ts.TrajServer(n, pos, 7.0, agent0=agent0, n_local=n_local, init_yaw=np.linspace(-0.01, 0.01, n)[agent0:agent0 + n_local],
                        prm=ts.make_params(0.5, yaw_mode))
    tables, out, k = _tables(rows), [], 0
    for s in splits:
        out.append(srv.run(tables[k:k + s], 10.0, k, 0.1).clone())
        k += s
    torch.cuda.synchronize()
    st, rings = srv.states()
    return torch.cat(out, dim=1).cpu().numpy(), st, rings


def test_call_split_invariance():
    _, ts, _ = _mods()
    rows = _swarm_rows(N_LOCAL, 6)
    one = _fly(ts, rows, [6])
    assert (one[0].view(ts.COMMAND_DTYPE)["flags"] & 1).all()
    for splits in ([1] * 6, [2, 4]):
        got = _fly(ts, rows, splits)
        for g, w, what in zip(got, one, ("commands", "states", "rings")):
            assert g.tobytes() == w.tobytes(), (splits, what)


def test_agent_indexing():
    _, ts, _ = _mods()
    rows = _swarm_rows(65, 3)
    rows[:, 64] = rows[:, 0]
    rows["drone_id"][:, 64] = 64
    cmd, st, rings = _fly(ts, rows, [3])
    # (agent 64's init_pos / init_yaw differ from agent 0's: every command is published, and yaw_mode 0 pushes yaw 0)
    cmd0, st0, rings0 = _fly(ts, rows, [3], yaw_mode=0)
    assert cmd0[64].tobytes() == cmd0[0].tobytes() and rings0[64].tobytes() == rings0[0].tobytes()
    assert cmd0[1].tobytes() != cmd0[0].tobytes()
    part = _fly(ts, rows, [3], agent0=60, n_local=5)
    assert part[0].tobytes() == cmd[60:65].tobytes() and part[1].tobytes() == st[60:65].tobytes()
    assert part[2].tobytes() == rings[60:65].tobytes()
    mid = _fly(ts, rows, [3], agent0=3, n_local=2)
    assert mid[0].tobytes() == cmd[3:5].tobytes()


# ---- 7. argument validation ----
def test_argument_validation():
    import torch
    pop, ts, _ = _mods()
    abi, lib = pop._abi, pop.lib()
    n, n_ticks = 3, 2
    rows = _swarm_rows(n, n_ticks)
    tables = _tables(rows)
    srv = ts.TrajServer(n, np.zeros((n, 3)), 7.0)
    torch.cuda.synchronize()
    state0, queue0 = srv.state.clone(), srv.queue.clone()
    cmd = torch.full((n, n_ticks * 10, abi.POSITION_COMMAND_BYTES), 0xAB, dtype=torch.uint8, device="cuda")
    good = dict(prm=ts.make_params(0.5, 1), state=srv.state.data_ptr(), queue=srv.queue.data_ptr(), tables=tables.data_ptr(),
                prev=None, received=None, n_ticks=n_ticks, n_total=n, agent0=0, n_local=n, t0=10.0, first_tick=0, period=0.1,
                delay=0.0, cmd=cmd.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.sogm_traj_server_run(C.byref(a["prm"]) if a["prm"] is not None else None, a["state"], a["queue"],
                                        a["tables"], a["prev"], a["received"], a["n_ticks"], a["n_total"], a["agent0"],
                                        a["n_local"], a["t0"], a["first_tick"], a["period"], a["delay"], a["cmd"], None)

    bad = [dict(prm=None), dict(state=None), dict(queue=None), dict(tables=None), dict(cmd=None),
           dict(n_ticks=0), dict(n_ticks=65), dict(n_total=0), dict(agent0=-1), dict(n_local=0), dict(agent0=1, n_local=n),
           dict(first_tick=-1), dict(period=0.105), dict(period=0.0), dict(delay=-0.01), dict(delay=0.1),
           dict(t0=float("nan"))]
    for thres in (0.0, -0.5, 1.28, float("nan")):
        bad.append(dict(prm=ts.make_params(thres, 1)))
    bad += [dict(prm=ts.make_params(0.5, 2)), dict(prm=ts.make_params(0.5, -1)), dict(prm=ts.make_params(0.5, 1, sample_dt=0.0)),
            dict(prm=ts.make_params(0.5, 1, (float("inf"), 1.0)))]
    for kw in bad:
        assert call(**kw) == abi.SOGM_ERR_INVALID_ARG, kw
        assert b"sogm_traj_server_run" in lib.sogm_last_error(), kw
    one = torch.zeros((1, 3), dtype=torch.float64, device="cuda")
    assert lib.sogm_traj_server_init(None, srv.queue.data_ptr(), n, 7.0, one.data_ptr(), None, None) == abi.SOGM_ERR_INVALID_ARG
    assert lib.sogm_traj_server_init(srv.state.data_ptr(), srv.queue.data_ptr(), 0, 7.0, one.data_ptr(), None,
                                     None) == abi.SOGM_ERR_INVALID_ARG
    assert lib.sogm_traj_server_init(srv.state.data_ptr(), srv.queue.data_ptr(), n, 7.0, None, None, None) == abi.SOGM_ERR_INVALID_ARG
    c9, c3 = (C.c_double * 9)(*ts.CAM2BODY), (C.c_double * 3)(0.0, 0.0, 0.0)
    pos, rot = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros((n, 9), dtype=torch.float64, device="cuda")
    for args in ((None, n, 1, c9, c3, pos.data_ptr(), rot.data_ptr()), (cmd.data_ptr(), 0, 1, c9, c3, pos.data_ptr(), rot.data_ptr()),
                 (cmd.data_ptr(), n, 0, c9, c3, pos.data_ptr(), rot.data_ptr()), (cmd.data_ptr(), n, 1, None, c3, pos.data_ptr(), rot.data_ptr()),
                 (cmd.data_ptr(), n, 1, c9, c3, None, rot.data_ptr()), (cmd.data_ptr(), n, 1, c9, c3, pos.data_ptr(), None)):
        assert lib.sogm_camera_poses(*args, None) == abi.SOGM_ERR_INVALID_ARG, args
    torch.cuda.synchronize()
    assert bool((cmd == 0xAB).all()) and torch.equal(srv.state, state0) and torch.equal(srv.queue, queue0)
    assert not pos.any() and not rot.any()
    assert call() == abi.SOGM_OK       # and the good call runs
    torch.cuda.synchronize()
    assert not bool((cmd == 0xAB).all())


# ---- 8. camera hand-over ----
def test_camera_poses_feed_the_depth_renderer():
    import torch
    pop, ts, _ = _mods()
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    depth = importlib.import_module("pred-occ-planner_amd.depth")
    rows = np.zeros((2, 2), tsf.REC_DTYPE)
    by_name = {c["name"]: c for c in tsf.CASES}
    for a, name in enumerate(("ends_drains_held_then_reset", "hover_zero_velocity_yaw_held")):
        for k in range(2):
            rows[k, a] = tsf.record_bytes(by_name[name]["records"][k], a)
    srv = ts.TrajServer(2, np.zeros((2, 3)), 7.0, init_yaw=[0.3, 0.7], prm=ts.make_params(0.3, 1))
    srv.run(_tables(rows), 10.0, 0, 0.1)
    pos, rot = srv.camera_poses()
    last = srv.commands[:, -1]
    pos_h, rot_h = pos.cpu().numpy(), rot.cpu().numpy()
    assert abs(last["yaw"][1] - 0.7) < 1e-3 and abs(last["yaw"][0] - 0.3) < 0.02 and (last["flags"] & 1).all()
    for a in range(2):
        p, R = pop.scene.camera_pose(*last["pos"][a], last["yaw"][a])
        assert np.abs(rot_h[a].reshape(3, 3) - R).max() <= 1e-15      # test_detmath's 2 eps on cos (and sin)
        assert np.array_equal(pos_h[a], last["pos"][a])                # zero offset: exact
    off = srv.camera_poses(cam_offset=(0.1, 0.0, -0.05))[0].cpu().numpy()
    for a in range(2):
        c, s = np.cos(last["yaw"][a]), np.sin(last["yaw"][a])
        assert np.abs(off[a] - (last["pos"][a] + [0.1 * c, 0.1 * s, -0.05])).max() <= 1e-15
    # the device poses straight into the renderer: three cylinders ahead of the two agents, a 24 x 32 frame
    rec = np.array([[3, last["pos"][0][0] + 2.0, last["pos"][0][1] + 0.2, 2.0, 0.5, 4.0],
                    [3, last["pos"][1][0] + 1.5, last["pos"][1][1] + 1.4, 2.0, 0.6, 4.0],
                    [3, last["pos"][1][0] + 3.0, last["pos"][0][1] - 0.8, 0.4, 0.7, 0.8]])
    cam = types.SimpleNamespace(fx=19.0, fy=19.0, cx=16.0, cy=12.0, max_depth=5.0, depth_scale=1000.0, ground_z=0.0,
                                rows=24, cols=32, use_ground=1)
    arr = (pop._abi.SogmCylinder * 3)()
    for i, (typ, x, y, z, w, h) in enumerate(rec):
        o = arr[i]
        o.type, o.x, o.y, o.z, o.w, o.h, o.qw = int(typ), x, y, z, w, h, 1.0
    world = sogm.World(np.zeros((0, 3), np.float32), arr, n_cyl=3)
    dcam = depth.make_depth_camera(24, 32, 5.0, 1000.0, 0.0, True, fx=19.0, fy=19.0, cx=16.0, cy=12.0)
    d, cl, _, other = depth.render_depth(world, dcam, pos, rot, True)
    torch.cuda.synchronize()
    want = ref.render_agents(rec, cam, pos_h, rot_h)
    ok, why = ref.same(d.cpu().numpy().view(np.uint16), cl.cpu().numpy(), want[0], want[1])
    assert ok, why
    assert all((w != 0).sum() > 100 for w in want[0]) and len({int(v) for v in want[0][0].ravel()}) > 10


# ---- 9. the tick driver's hook ----
def _run_swarm(driver, mode, server, K=6, A=8):
    """K ticks of the 8-agent parity swarm; mode "fsm": step_fsm_device(), "step": step().  Returns what must not depend on
    the server (records, ok flags, FSM states) and, with the server on, the tables it was fed and its commands per tick."""
    import torch
    fsm = mode == "fsm"
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False, fsm=fsm, device_fsm=fsm, traj_server=server)
    oks, recs, tabs, rcvs, cmds = [], [], [], [], []
    for _ in range(K):
        oks.append(sw.step().cpu().numpy())
        recs.append(sw.new.cpu().numpy())
        tabs.append((sw.own if fsm else sw.records_all()).clone())
        if fsm:
            rcvs.append((sw.last_fsm["pub_new"] | sw.last_fsm["pub_hover"]).to(torch.int32).clone())
        if server:
            cmds.append(sw.server.cmd.clone())
    torch.cuda.synchronize()
    fixed = [np.stack(oks), np.stack(recs), sw.records_all().cpu().numpy(), sw.status.cpu().numpy(), sw.fail.cpu().numpy(),
             sw.traj_start.cpu().numpy()]
    last = sw.commands()
    starts, t0 = sw.scene["starts"][:A].copy(), sw.t0
    sw.close()
    return fixed, torch.stack(tabs), (torch.stack(rcvs) if fsm else None), cmds, last, starts, t0


@pytest.mark.parametrize("mode", ["fsm", "step"])
def test_driver_hook_changes_nothing_and_serves_the_executed_tables(mode):
    import torch
    _, ts, driver = _mods()
    off = _run_swarm(driver, mode, None)
    on = _run_swarm(driver, mode, True)
    assert off[4] is None
    for a, b in zip(off[0], on[0]):
        assert a.tobytes() == b.tobytes()
    fixed, tabs, rcvs, cmds, last, starts, t0 = on
    assert last.tobytes() == cmds[-1].cpu().numpy().tobytes() and last.shape == (8, 10)
    direct = ts.TrajServer(8, starts, t0)
    want = direct.run(tabs, t0, 0, driver.TICK_PERIOD, received=rcvs)
    assert torch.equal(torch.cat(cmds, dim=1), want)
    c = direct.commands
    assert (c["flags"] & 1).mean() > 0.5 and len({int(v) for v in c["traj_id"].ravel()}) > 1


@pytest.mark.parametrize("fsm", [False, True])
def test_driver_hook_in_a_flight(fsm):
    import torch
    pop, ts, driver = _mods()
    out = []
    for server in (None, True):
        sw = driver.SwarmTick("parity", 8, moving_world=True, prestamp=False, fsm=fsm, device_fsm=fsm, traj_server=server)
        ok, recs = sw.fly(4)
        torch.cuda.synchronize()
        out.append((ok.cpu().numpy(), recs.cpu().numpy(), sw.own.cpu().numpy(), sw.status.cpu().numpy()))
        if server:
            got = sw.server.cmd.clone()
            assert sw.commands().shape == (8, 40)
            if fsm:
                tabs, rcv = sw.flight_fsm_log["own"], sw.flight_fsm_log["pub"] != pop._abi.FSM_PUB_NONE
            else:
                tabs, rcv, cur = [], None, torch.zeros_like(recs[0])
                for k in range(4):
                    cur = torch.where(ok[k].bool().unsqueeze(1), recs[k], cur)
                    tabs.append(cur)
                tabs = torch.stack(tabs)
            direct = ts.TrajServer(8, sw.scene["starts"][:8], sw.t0)
            assert torch.equal(direct.run(tabs, sw.t0, 0, driver.TICK_PERIOD, received=rcv), got)
            assert (direct.commands["flags"] & 1).mean() > 0.5
        sw.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
