#!/usr/bin/env python
"""Closed-loop FSM tick, host state machines against device state machines: SwarmTick("cfg2", 128, fsm=True) with
device_fsm off (step_fsm: torch expressions, every agent replanned, most results discarded) and on (sogm_fsm_inputs ->
... -> replan of the agents that are due -> sogm_fsm_apply).  Reports ms per tick and the share of agent-ticks that were
due.  A timing tool, not a test: the two variants fly the same scene for the same ticks in processes of their own (each
holds its own hardware queues), interleaved over --repeats so that drift of the box hits both alike.

Timing: ticks are stream-ordered and never synchronise, so a pair of events around a block of ticks measures the device's
time for the block; the first --warmup ticks (NEW_PLAN for everybody, allocator warm-up, first-use stream creation) are
flown before the first event.  One JSON line per variant and repeat, then a summary line.

    python tools/bench_fsm.py --ticks 100 --warmup 20 --repeats 3
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fly(device_fsm, grid, agents, ticks, warmup, block):
    import importlib

    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    sw = driver.SwarmTick(grid, agents, fsm=True, device_fsm=device_fsm)
    kept = []

    def keep():   # this tick's flags, looked at after the timed region (no synchronisation inside a block)
        f = sw.last_fsm
        if "due" in f:   # device machines: the buffers are rewritten by the next tick -> one small copy each
            kept.append((f["due"].clone(), f["ok"].clone()))
        else:            # step_fsm makes fresh tensors every tick: keep them.  Due = it planned: published new, published
            kept.append((f["ok"] | f["pub_hover"] | (f["t_start"] != f["now"]), f["ok"]))   # a hover, or was in REPLAN

    for _ in range(warmup):
        sw.step()
    torch.cuda.synchronize()
    times, k = [], 0
    while k < ticks:
        n = min(block, ticks - k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            sw.step()
            keep()
        e1.record()
        e1.synchronize()
        times.append((e0.elapsed_time(e1), n))
        k += n
    torch.cuda.synchronize()
    n_due = sum(int((d != 0).sum().item()) for d, _ in kept)
    n_ok = sum(int((o != 0).sum().item()) for _, o in kept)
    status = sw.status.cpu().numpy()
    code, fails = sw.planner.flow_failures()
    out = {"variant": "device_fsm" if device_fsm else "host_fsm", "grid": grid, "agents": agents, "ticks": ticks,
           "ms_per_tick": sum(t for t, _ in times) / ticks,
           "ms_per_tick_blocks": [round(t / n, 4) for t, n in times],
           "due_share": n_due / (ticks * agents), "ok_share": n_ok / (ticks * agents),
           "status_counts": [int((status == s).sum()) for s in range(4)], "flow_failures": fails}
    sw.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="cfg2")
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--child", choices=["host", "device"])
    a = ap.parse_args()
    if a.child:
        print(json.dumps(fly(a.child == "device", a.grid, a.agents, a.ticks, a.warmup, a.block)), flush=True)
        return 0
    res = {"host": [], "device": []}
    for _ in range(a.repeats):
        for which in ("host", "device"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--grid", a.grid, "--agents", str(a.agents),
                   "--ticks", str(a.ticks), "--warmup", str(a.warmup), "--block", str(a.block)]
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if run.returncode != 0:   # nothing more is started on the device after a child that failed
                sys.stderr.write(run.stdout + run.stderr)
                return run.returncode or 1
            line = run.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[which].append(json.loads(line))
    med = lambda v: sorted(v)[len(v) // 2]
    h, d = med([r["ms_per_tick"] for r in res["host"]]), med([r["ms_per_tick"] for r in res["device"]])
    print(json.dumps({"summary": "median of repeats", "host_fsm_ms_per_tick": h, "device_fsm_ms_per_tick": d,
                      "speedup": h / d, "due_share_host": med([r["due_share"] for r in res["host"]]),
                      "due_share_device": med([r["due_share"] for r in res["device"]])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
