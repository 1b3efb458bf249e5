"""Side bench of the trajectory server (sogm_traj_server_run), event-timed, ONE JSON line.

128 agents on cfg2: the lock-step tick of the same process with the server off and on (as tools/eval_swarm.py does for the
audit), then the server alone on that swarm's executed tables — as 60 one-tick calls and as one 60-tick call, yaw_mode 0
and 1 (median of --repeat runs after a warm-up, hip events around the calls).  --gap also flies the 8-agent parity swarm
for 40 ticks and counts the command samples whose position differs from the flight audit's rule ("the newest record with
time_start <= t", evaluated at t by sogm_traj_eval) and by how much, in metres and in seconds of flight (|dp| / |v|)."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fly(driver, grid, agents, ticks, server, keep=False):
    """ms per lock-step tick (events around the whole run); with keep, also the executed table of every tick"""
    import torch
    sw = driver.SwarmTick(grid, agents, moving_world=True, traj_server=server)
    sw.compute.prepare(0, ticks)
    tabs = []
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(ticks):
        sw.step()
        if keep:
            tabs.append(sw.records_all().clone())
    end.record()
    torch.cuda.synchronize()
    out = (start.elapsed_time(end) / ticks, torch.stack(tabs) if keep else None, sw.scene["starts"][:agents].copy(), sw.t0,
           sw.server.cmd.clone() if keep and server is not None else None)
    sw.close()
    return out


def alone(ts, driver, tables, starts, t0, yaw_mode, one_call, repeat):
    """device ms per tick of the server alone on `tables`"""
    import torch
    n_ticks, n = int(tables.shape[0]), int(tables.shape[1])
    ms = []
    for r in range(repeat + 1):   # (the first run warms up)
        srv = ts.TrajServer(n, starts, t0, prm=ts.make_params(0.5, yaw_mode))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        if one_call:
            srv.run(tables, t0, 0, driver.TICK_PERIOD)
        else:
            for k in range(n_ticks):
                srv.run(tables[k], t0, k, driver.TICK_PERIOD)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1) / n_ticks)
    return statistics.median(ms)


def gap(ts, driver, planner, ticks=40, agents=8):
    """the server's commands against the audit's sampling rule on the parity swarm"""
    import numpy as np
    import torch
    sw = driver.SwarmTick("parity", agents, moving_world=True, prestamp=False, fsm=True, device_fsm=True,
                          traj_server=ts.make_params(0.5, 0))
    tabs, cmds = [], []
    for _ in range(ticks):
        sw.step()
        tabs.append(sw.own.clone())
        cmds.append(sw.server.cmd.clone())
    torch.cuda.synchronize()
    starts, t0 = torch.from_numpy(sw.scene["starts"][:agents].copy()).cuda(), sw.t0
    cmd = torch.cat(cmds, dim=1).cpu().numpy().view(ts.COMMAND_DTYPE).reshape(agents, ticks * 10)
    tabs = torch.stack(tabs)                                   # [ticks][A][2064]
    prev = torch.cat([torch.zeros_like(tabs[:1]), tabs[:-1]])
    want = np.zeros((agents, ticks * 10, 3))
    for j in range(10):
        t = torch.tensor([[(t0 + k * driver.TICK_PERIOD) + j * 0.01] * agents for k in range(ticks)], dtype=torch.float64,
                         device="cuda")
        pos = starts.unsqueeze(0).expand(ticks, agents, 3).clone()
        for table in (prev, tabs):                            # the newer table wins where its record has started
            flat = table.reshape(ticks * agents, -1).contiguous()
            pva, valid = planner.traj_eval(flat, t.reshape(-1).contiguous())
            hdr = flat[:, :16].cpu().numpy()
            started = torch.from_numpy(hdr[:, 8:16].copy().view(np.float64).reshape(-1)).cuda() <= t.reshape(-1)
            use = (valid.bool() & started).reshape(ticks, agents, 1)
            pos = torch.where(use, pva[:, :3].reshape(ticks, agents, 3), pos)
        want[:, j::10] = pos.permute(1, 0, 2).cpu().numpy()
    sw.close()
    pub = (cmd["flags"] & 1) != 0
    dp = np.linalg.norm(cmd["pos"] - want, axis=2)
    speed = np.linalg.norm(cmd["vel"], axis=2)
    differ = pub & (dp > 1e-9)
    dt = np.where(differ & (speed > 1e-6), dp / np.maximum(speed, 1e-6), 0.0)
    return {"gap_samples": int(pub.sum()), "gap_unpublished": int((~pub).sum()), "gap_differing": int(differ.sum()),
            "gap_max_m": float(dp[pub].max()) if pub.any() else 0.0,
            "gap_mean_m_of_differing": float(dp[differ].mean()) if differ.any() else 0.0,
            "gap_max_s": float(dt.max()), "gap_median_s_of_differing": float(np.median(dt[differ])) if differ.any() else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="cfg2")
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--gap", action="store_true", help="also measure the gap to the audit's sampling rule (parity swarm)")
    args = ap.parse_args()
    assert 1 <= args.ticks <= 64, "one call serves at most 64 ticks"
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    ts = importlib.import_module("pred-occ-planner_amd.trajserver")
    fly(driver, args.grid, args.agents, min(args.ticks, 5), None)   # warm-up
    ms_off = fly(driver, args.grid, args.agents, args.ticks, None)[0]
    ms_on = fly(driver, args.grid, args.agents, args.ticks, ts.make_params(0.5, 1))[0]
    _, tables, starts, t0, _ = fly(driver, args.grid, args.agents, args.ticks, None, keep=True)
    out = {"grid": args.grid, "agents": args.agents, "ticks": args.ticks,
           "ms_per_tick_server_off": round(ms_off, 4), "ms_per_tick_server_on": round(ms_on, 4)}
    for yaw_mode in (0, 1):
        out[f"server_ms_per_tick_one_tick_calls_yaw{yaw_mode}"] = round(alone(ts, driver, tables, starts, t0, yaw_mode, False,
                                                                          args.repeat), 5)
        out[f"server_ms_per_tick_one_call_yaw{yaw_mode}"] = round(alone(ts, driver, tables, starts, t0, yaw_mode, True,
                                                                        args.repeat), 5)
    if args.gap:
        out.update(gap(ts, driver, planner))
    out["timing"] = ("same process: lock-step swarm with the server off, then on (yaw_mode 1); the server alone on that "
                     "swarm's executed tables, hip events around the calls, median of the repeats")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
