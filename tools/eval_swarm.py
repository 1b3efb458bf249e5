"""Fly a swarm with the flight audit on and print ONE JSON line: the audit's report (arrivals, collisions of each kind,
minimum separation and gap) and its cost.

    python tools/eval_swarm.py cfg2 128 300 lockstep|fsm|flight|flight_fsm [rings] [--frozen] [--events N]
                               [--link loss=P,delay=A..B,range=R,seed=N[,newest]]
                               [--msg-noise loc=S|X/Y/Z,time=S,track=S,hold=N,seed=N] [--belief]

--link (lockstep only): every agent reads its own table of the swarm, what radio links with that loss, delay (whole ticks),
range (metres) and seed delivered to it (links.LinkModel; include/sogm_abi.h "radio links"); the audit still judges the true
tables.  The line then has a `link` block: the parameters and the link model's counters summed over receivers and ticks.

--msg-noise (lockstep only): what every sender broadcasts carries a localisation bias, a clock offset and a tracking error
(links.parse_noise; include/sogm_abi.h "message noise"); --belief scores every receiver's view against the table the senders
execute after each delivery ("belief audit").  Without --link both fly perfect links.  The line then has a `msg_noise` block
with the spec and a `belief` block: the twelve totals and rms_m = sqrt(sum_q / samples) / 1000.

rings (optional, default 0): that many ring obstacles in the scene (scene.make_scene(n_rings=...)), audited as rings; the
report then also has ring_agents / ring_samples / min_ring_gap, counted from the event list and the per-agent minima.

flight_fsm: the flight with every agent-tick one FSMCallback on the device (sogm_planner_set_flight_fsm) — the closed loop
of `fsm` on the schedule of `flight`.

ms_per_tick: the same swarm flown twice back to back in this process, audit off then audit on (hip events around the
whole run after a warm-up swarm); audit_ms_per_tick: device time of the audit's own launches in the audited run (hip
events around each audit call)."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(driver, args, audit):
    import torch
    flight = args.mode in ("flight", "flight_fsm")
    extra = {}
    if args.msg_noise is not None:
        extra["msg_noise"] = args.msg_noise
    if args.belief:
        extra["belief"] = True
    sw = driver.SwarmTick(args.grid, args.agents, moving_world=not args.frozen, prestamp=False if flight else None,
                          fsm=args.mode in ("fsm", "flight_fsm"), device_fsm=args.mode == "flight_fsm", audit=audit,
                          n_rings=args.rings, link=args.link, **extra)
    sw.compute.prepare(0, args.ticks)
    audit_ms = []
    if audit:   # time every audit call with events of its own on the same stream
        inner = sw.auditor.add

        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            inner(*a, **k)
            e1.record()
            audit_ms.append((e0, e1))
        sw.auditor.add = timed
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    if flight:
        done = 0
        while done < args.ticks:
            n = min(60, args.ticks - done)
            sw.fly(n)
            done += n
    else:
        for _ in range(args.ticks):
            sw.step()
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end) / args.ticks
    rep = sw.audit_report() if audit else None
    if audit and args.rings:
        # the ring column: the records after the cylinders are the rings; per (sample, agent) collisions from the events
        # (complete only when the list was not truncated), the smallest gap among the agents whose nearest obstacle is a ring
        n_cyl = len(sw.scene["cylinders"])
        ev = [e for e in rep["events"] if e[3] == 1 and e[2] >= n_cyl]
        acc = sw.auditor.per_agent()
        near = acc["min_gap_obstacle"] >= n_cyl
        rep.update(rings=args.rings, ring_agents=len({e[1] for e in ev}), ring_samples=len({(e[0], e[1]) for e in ev}),
                   ring_events_complete=not rep["events_truncated"],
                   min_ring_gap_where_nearest=float(acc["min_gap"][near].min()) if near.any() else None)
    a_ms = sum(e0.elapsed_time(e1) for e0, e1 in audit_ms) / args.ticks if audit else None
    if audit and args.link:
        rep["link"] = dict(spec=args.link, **sw.link_counters())
    if audit and args.msg_noise is not None:
        rep["msg_noise"] = dict(spec=args.msg_noise)
    if audit and args.belief:
        rep["belief"] = sw.belief_report()
    sw.close()
    return ms, rep, a_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("grid")
    ap.add_argument("agents", type=int)
    ap.add_argument("ticks", type=int)
    ap.add_argument("mode", choices=("lockstep", "fsm", "flight", "flight_fsm"))
    ap.add_argument("rings", type=int, nargs="?", default=0, help="ring obstacles in the scene (default 0)")
    ap.add_argument("--frozen", action="store_true", help="a frozen world (moving_world=False)")
    ap.add_argument("--events", type=int, default=20, help="events printed (the report counts all)")
    ap.add_argument("--link", default=None, help="loss=P,delay=A..B,range=R,seed=N[,newest] (lockstep only)")
    ap.add_argument("--msg-noise", default=None, help="loc=S|X/Y/Z,time=S,track=S,hold=N,seed=N (lockstep only)")
    ap.add_argument("--belief", action="store_true", help="score every receiver's view against the true table (lockstep only)")
    args = ap.parse_args()
    if (args.link or args.msg_noise is not None or args.belief) and args.mode != "lockstep":
        ap.error("--link, --msg-noise and --belief fly the lock-step tick only")
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    run(driver, argparse.Namespace(**dict(vars(args), ticks=min(args.ticks, 5))), False)   # warm-up
    ms_off, _, _ = run(driver, args, False)
    ms_on, rep, audit_ms = run(driver, args, True)
    ev = rep.pop("events")
    out = {"grid": args.grid, "agents": args.agents, "ticks": args.ticks, "mode": args.mode, "moving_world": not args.frozen,
           **rep, "first_events": ev[:args.events], "ms_per_tick_audit_off": round(ms_off, 4),
           "ms_per_tick_audit_on": round(ms_on, 4), "audit_ms_per_tick": round(audit_ms, 4),
           "timing": "same process, audit off then on, back to back; audit_ms_per_tick = hip events around each audit call"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
