"""Diagnostic: what an agent's chain pays behind its LAST corridor segment in the dataflow replan, over the bench tick
(cfg2: 128 agents, 200^3 x 20, 3 warm-up + 20 timed ticks as bench.py flies them).  Per agent and tick, from the device
stamps of the bookkeeping (sogm_debug_corridor_finalize_times: start = the agent's last segment slot is counted, adjacent
pairs done, goal LPs done, copy done) and ts[3] "corridors final" of sogm_debug_flow_times: the whole tail and its split
into pair LPs, goal LPs, copy and publication, as mean / max over the agents and for the tick's critical agent (the one
whose chain ends last: chain_ms.critical_agent of bench.py --full).  Also the pair counters (sogm_debug_corridor_pairs).
A library built with -DSOGM_PAIRS_EAGER=0 gives the "before" column of one source: every pair LP in the bookkeeping.

usage: python tools/diag_pairs.py [timed ticks] [out.json]"""
import ctypes as C, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
pop = importlib.import_module("pred-occ-planner_amd")
driver = importlib.import_module("pred-occ-planner_amd.driver")
A, WARM = 128, 3
ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 20
sw = driver.SwarmTick("cfg2", A, moving_world=True)
sw.compute.prepare(0, WARM + ticks + 1)
lib = pop.lib()
lib.sogm_debug_corridor_finalize_times.restype = C.c_int
lib.sogm_debug_corridor_finalize_times.argtypes = [C.c_void_p, C.c_void_p]
for _ in range(WARM):
    sw.step()
torch.cuda.synchronize()
sw.planner.corridor_pairs()
names = ("tail", "pairs", "goal", "copy", "publish")
rows, crit_rows, tick_end, pieces = [], [], [], []
for k in range(ticks):
    sw.step()
    ts, fin = np.zeros((A, 8), np.int64), np.zeros((A, 4), np.int64)
    lib.sogm_debug_flow_times(sw.planner._p, ts.ctypes.data_as(C.c_void_p))  # synchronises
    lib.sogm_debug_corridor_finalize_times(sw.planner._p, fin.ctypes.data_as(C.c_void_p))
    t0 = ts[:, 7].min() if ts[:, 7].min() > 0 else ts[:, 0].min()
    us = np.stack([ts[:, 3] - fin[:, 0], fin[:, 1] - fin[:, 0], fin[:, 2] - fin[:, 1], fin[:, 3] - fin[:, 2],
                   ts[:, 3] - fin[:, 3]], axis=1) / 100.0  # 100 MHz ticks -> us
    crit = int(np.argmax(ts[:, 6]))
    rows.append(us)
    crit_rows.append(us[crit])
    tick_end.append((ts[:, 6].max() - t0) / 1e5)
cnt = sw.planner.corridor_pairs()
flow = sw.planner.flow_failures()
sw.close()
rows, crit_rows = np.stack(rows), np.stack(crit_rows)  # [ticks, A, 5], [ticks, 5]
out = {"ticks": ticks, "agents": A, "unit": "us", "pair_counters": cnt, "flow_failures": list(flow),
       "chain_end_ms_mean": float(np.mean(tick_end)),
       "mean": dict(zip(names, rows.mean(axis=(0, 1)).round(2).tolist())),
       "max_over_agents_mean_over_ticks": dict(zip(names, rows.max(axis=1).mean(axis=0).round(2).tolist())),
       "max": dict(zip(names, rows.max(axis=(0, 1)).round(2).tolist())),
       "critical_agent_mean": dict(zip(names, crit_rows.mean(axis=0).round(2).tolist())),
       "critical_agent_max": dict(zip(names, crit_rows.max(axis=0).round(2).tolist())),
       "critical_agent_per_tick_tail": crit_rows[:, 0].round(1).tolist(),
       "critical_agent_per_tick_pairs": crit_rows[:, 1].round(1).tolist()}
print(f"behind the last segment, us, {ticks} ticks x {A} agents; pair counters {cnt}; chain end {out['chain_end_ms_mean']:.2f} ms")
print(f"{'':28s}" + "".join(f"{n:>10s}" for n in names))
for key in ("mean", "max_over_agents_mean_over_ticks", "max", "critical_agent_mean", "critical_agent_max"):
    print(f"{key:28s}" + "".join(f"{out[key][n]:10.1f}" for n in names))
print(json.dumps(out))
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(out, f)
