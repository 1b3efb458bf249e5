"""Side bench of the radio-link model (sogm_link_deliver), event-timed, ONE JSON line.

    python tools/bench_link.py [--agents 128] [--calls 400] [--repeat 5] [--grid cfg2] [--ticks 60] [--no-tick]
                               [--noise] [--belief]

1. sogm_link_deliver alone, agents x agents pairs: hip events around --calls consecutive ticks on a table of full records,
   median of --repeat runs after a warm-up, for perfect links, for loss 0.3 / delay 0..2, and for the same with a range (the
   positions are read then).  bytes_per_call_at_most is what the definition moves when every pair applies a row: the table
   into the ring, one row read and one written per pair.
2. The lock-step tick (cfg2, 128 agents, moving world, no pre-stamp, no fused publication) with perfect-link views against
   the same tick on the shared table, the two swarms alternating in this process, --repeat times each.
3. --noise / --belief: sogm_traj_noise (agents rows, loc 0.1 / time 0.05 / track 0.05) and sogm_belief_audit (agents x agents
   pairs, the views of that noise on perfect links, default parameters) alone, timed like the deliver; and the lock-step tick
   on lossy links (loss 0.3, delay 0..2) with the noise, and with the noise and the audit, against the same tick on those
   links alone, the swarms alternating."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REC = 2064


def deliver_alone(links, n, prm, calls, repeat):
    """device microseconds per sogm_link_deliver"""
    import numpy as np
    import torch
    rng = np.random.default_rng(0x5067)
    table = rng.integers(0, 256, (n, REC), dtype=np.uint8)
    table[:, 4:8] = np.frombuffer(np.int32(6).tobytes(), np.uint8)      # n_pieces 6: every row is a message
    table = torch.from_numpy(table).cuda()
    pos = torch.from_numpy(rng.uniform(-20.0, 20.0, (n, 3))).cuda()
    us = []
    for r in range(repeat + 1):   # (the first run warms up)
        model = links.LinkModel(n, 0, n, prm)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(calls):
            model.deliver(k, table, pos)
        e1.record()
        torch.cuda.synchronize()
        if r:
            us.append(1e3 * e0.elapsed_time(e1) / calls)
    return statistics.median(us), min(us), max(us), model.totals()


def launch_alone(call, calls, repeat):
    """device microseconds per call of call(k), k = 0 .. calls - 1"""
    import torch
    us = []
    for r in range(repeat + 1):   # (the first run warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(calls):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        if r:
            us.append(1e3 * e0.elapsed_time(e1) / calls)
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def flying_table(n):
    """n rows of six 0.3 s pieces flying straight lines: what a tick's table looks like"""
    import numpy as np
    import torch
    rec = np.dtype([("drone_id", "i4"), ("n_pieces", "i4"), ("time_start", "f8"), ("duration", "f8", (16,)), ("cpts", "f8", (240,))])
    rng = np.random.default_rng(0x5067)
    t = np.zeros(n, rec)
    t["drone_id"], t["n_pieces"], t["time_start"] = np.arange(n), 6, 10.0
    t["duration"][:, :6] = 0.3
    start, vel = rng.uniform(-20.0, 20.0, (n, 1, 3)), rng.uniform(-1.0, 1.0, (n, 1, 3))
    t["cpts"][:, :90] = (start + vel * (0.075 * np.arange(30))[None, :, None]).reshape(n, 90)
    return torch.from_numpy(t.view(np.uint8).reshape(n, REC).copy()).cuda()


def noise_and_belief_alone(links, n, calls, repeat, noise, with_noise, with_belief):
    import torch
    out = {}
    table = flying_table(n)
    sent, shift = torch.empty_like(table), torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    if with_noise:
        out["traj_noise_us"] = launch_alone(lambda k: links.traj_noise(noise, k, table, sent, shift), calls, repeat)
        out["traj_noise_bytes_per_call"] = 2 * n * REC + n * 32
    if with_belief:
        model = links.LinkModel(n, 0, n)
        model.deliver(0, table, noise=noise)
        t_now = torch.full((n,), 10.05, dtype=torch.float64, device="cuda")
        out["belief_audit_us"] = launch_alone(lambda k: model.audit_belief(table, t_now), calls, repeat)
        out["belief_audit_totals"] = model.belief()
        out["belief_audit_record_bytes_in_reach"] = n * REC + n * n * REC
    return out


def fly(driver, grid, agents, ticks, link, **extra):
    """ms per lock-step tick (events around the whole run)"""
    import torch
    sw = driver.SwarmTick(grid, agents, moving_world=True, prestamp=False, link=link, **extra)
    assert not sw.publish and not sw.prestamp
    sw.compute.prepare(0, ticks)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(ticks):
        sw.step()
    end.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(end) / ticks
    ok = sw.n_ok_total
    sw.close()
    return ms, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, default=128)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--grid", default="cfg2")
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--no-tick", action="store_true", help="the launches alone, not the lock-step ticks")
    ap.add_argument("--noise", action="store_true", help="also sogm_traj_noise alone and the tick with message noise")
    ap.add_argument("--belief", action="store_true", help="also sogm_belief_audit alone and the tick with the belief audit")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_link.py measures on a GPU"
    os.environ["SOGM_PUBLISH"] = "0"   # the twin of a link run: the separate latest-wins merge, no fused publication
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    links = importlib.import_module("pred-occ-planner_amd.links")
    n = args.agents
    out = {"agents": n, "pairs": n * n, "calls": args.calls, "repeat": args.repeat,
           "bytes_per_call_at_most": n * REC + 2 * n * n * REC}
    cases = {"perfect": links.make_params(), "loss03_delay0_2": links.make_params(0x5067, 0.3, 0.0, 0, 2),
             "loss03_delay0_2_range25": links.make_params(0x5067, 0.3, 25.0, 0, 2),
             "loss01_delay0_7": links.make_params(0x5067, 0.1, 0.0, 0, 7)}
    for name, prm in cases.items():
        med, lo, hi, totals = deliver_alone(links, n, prm, args.calls, args.repeat)
        out[f"deliver_us_{name}"] = {"median": round(med, 2), "min": round(lo, 2), "max": round(hi, 2),
                                     "applied_per_call": totals["applied"] / args.calls}
    if not args.no_tick:
        fly(driver, args.grid, n, min(args.ticks, 5), None)   # warm-up
        shared, views = [], []
        for _ in range(args.repeat):
            shared.append(fly(driver, args.grid, n, args.ticks, None)[0])
            views.append(fly(driver, args.grid, n, args.ticks, links.make_params())[0])
        out.update(grid=args.grid, ticks=args.ticks,
                   ms_per_tick_shared_table=[round(v, 4) for v in shared], ms_per_tick_perfect_link_views=[round(v, 4) for v in views],
                   ms_per_tick_shared_table_median=round(statistics.median(shared), 4),
                   ms_per_tick_perfect_link_views_median=round(statistics.median(views), 4))
    if args.noise or args.belief:
        noise = links.make_noise(seed=0x5067, loc=0.1, time=0.05, track=0.05)
        out.update(noise_and_belief_alone(links, n, args.calls, args.repeat, noise, args.noise, args.belief))
        if not args.no_tick:
            lossy = links.make_params(0x5067, 0.3, 0.0, 0, 2)
            variants = {"ms_per_tick_lossy_links": {}}
            if args.noise:
                variants["ms_per_tick_lossy_links_noise"] = {"msg_noise": noise}
            if args.belief:
                variants["ms_per_tick_lossy_links_noise_belief" if args.noise else "ms_per_tick_lossy_links_belief"] = dict(
                    {"msg_noise": noise} if args.noise else {}, belief=True)
            runs = {name: [] for name in variants}
            fly(driver, args.grid, n, min(args.ticks, 5), lossy)   # warm-up
            for _ in range(3):
                for name, extra in variants.items():
                    runs[name].append(fly(driver, args.grid, n, args.ticks, lossy, **extra)[0])
            for name, ms in runs.items():
                out[name] = [round(v, 4) for v in ms]
                out[name + "_median"] = round(statistics.median(ms), 4)
    out["timing"] = ("hip events; deliver: --calls consecutive ticks per run, median / min / max of the repeats after a warm-up "
                     "run; ticks: the two swarms alternate in this process, events around each whole run; --noise / --belief: the two "
                     "launches alone are timed like the deliver (--calls consecutive calls per run), and the lossy-link ticks with "
                     "and without them alternate in this process, three runs each")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
