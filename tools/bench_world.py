"""World frames on the device against the host path they replace (include/sogm_abi.h "world timeline"): cfg2,
128 agents, the bench's scene (make_scene seed 0x5069) through scene.WorldTimeline.  One process; after a warm-up the two
paths alternate and medians over the repeats are reported with their spread (min .. max).

  host path per frame    numpy frame (WorldTimeline.frame), struct fill (cylinders_to_struct), upload (two host-to-device
                         copies), k_block_bounds — a host clock around each part, each ending in a synchronise
  device path per frame  sogm_world_frames between HIP events on the launch stream: as one-tick calls and as ONE 60-tick
                         call; bytes moved from shapes, n_points*(12 + 4 + 12) + n_blocks*16 + n_cyl*192 per frame, over that
                         time, as a share of the HBM peak (8.0 TB/s spec, 6.29 TB/s measured float4 copy).  A single frame of
                         a few MB is LAUNCH-BOUND (its time is mostly the launch): the 60-tick call is the figure that says
                         something about bandwidth
  lock-step ticks        --ticks step() ticks WITHOUT prepare(), host frames against device frames: ms per tick (a host
                         clock around the whole flight, ending in a synchronise) and the device memory held by frames

Prints one JSON line."""
import argparse, importlib, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12


def stat(v, nd=4):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), nd), "min": round(float(v.min()), nd), "max": round(float(v.max()), nd),
            "n": int(len(v))}


def frame_bytes(n_points, n_blocks, n_cyl):
    """what one frame must move: cloud read, owner read, cloud written; bounds written; records read and written"""
    return n_points * (12 + 4 + 12) + n_blocks * 16 + n_cyl * 192


def per_frame(pop, sogm, tl, repeats, batch):
    lib, abi = pop.lib(), pop._abi
    dev = sogm.WorldTimelineDev.from_timeline(tl, pool=batch)
    host = {k: [] for k in ("numpy_frame_ms", "struct_fill_ms", "upload_ms", "block_bounds_ms", "total_ms")}
    one, many = [], []
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    sync = torch.cuda.synchronize
    bounds = torch.empty((dev._slots[0].n_blocks, 4), dtype=torch.float32, device="cuda")
    for r in range(-3, repeats):       # three warm-up rounds of both paths
        k = 7 + r
        # host path
        sync()
        t0 = time.perf_counter()
        f = tl.frame(k)
        t1 = time.perf_counter()
        cyl = pop.scene.cylinders_to_struct(f["cylinders"])
        t2 = time.perf_counter()
        d_cloud, d_cyl = sogm._dev(f["cloud"], np.float32), sogm._dev(cyl)
        sync()
        t3 = time.perf_counter()
        abi.check(lib.sogm_cloud_block_bounds(d_cloud.data_ptr(), len(f["cloud"]), 256, bounds.data_ptr(), sogm._stream()),
                  "sogm_cloud_block_bounds")
        sync()
        t4 = time.perf_counter()
        # device path: a one-tick call, then one call for `batch` ticks
        e = [ev() for _ in range(4)]
        e[0].record()
        dev.frames(k, 1)
        e[1].record()
        e[2].record()
        dev.frames(k, batch)
        e[3].record()
        sync()
        if r >= 0:
            for name, v in zip(host, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                host[name].append(v * 1e3)
            one.append(e[0].elapsed_time(e[1]))
            many.append(e[2].elapsed_time(e[3]) / batch)
    nbytes = frame_bytes(dev.n_points, dev._slots[0].n_blocks, dev.n_cyl)
    rate = lambda ms: nbytes / (ms * 1e-3)  # noqa: E731
    out = {"n_points": dev.n_points, "n_blocks": dev._slots[0].n_blocks, "n_cyl": dev.n_cyl, "frame_bytes_moved": nbytes,
           "frame_bytes_held": dev._slots[0].nbytes(),
           "host_path_per_frame_ms": {k: stat(v) for k, v in host.items()},
           "device_one_tick_call_ms": stat(one), "device_one_tick_call_note": "launch-bound: one small kernel per call",
           f"device_{batch}_tick_call_ms_per_frame": stat(many)}
    m = float(np.median(many))
    out[f"device_{batch}_tick_call_GBps"] = round(rate(m) / 1e9, 1)
    out[f"device_{batch}_tick_call_share_of_hbm_spec"] = round(rate(m) / HBM_SPEC, 3)
    out[f"device_{batch}_tick_call_share_of_hbm_measured_copy"] = round(rate(m) / HBM_MEASURED, 3)
    out["device_one_tick_call_GBps"] = round(rate(float(np.median(one))) / 1e9, 1)
    return out


def lock_step(driver, ticks, device_world, scene):
    sw = driver.SwarmTick("cfg2", 128, moving_world=True, scene=scene, device_world=device_world)
    for _ in range(3):                # code objects, streams, grids: not the frames' cost
        sw.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ticks):
        sw.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / ticks
    c = sw.compute
    held = c._tl_dev.pool_bytes() if device_world else sum(
        t.numel() * t.element_size() for w in c._frames.values() for t in (w.cloud, w.bounds, w.cylinders))
    n_ok = int(sw.ok.sum().item())
    sw.close()
    return ms, held, n_ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=60)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--flights", type=int, default=2, help="lock-step repeats of each path, alternating")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    pop = importlib.import_module("pred-occ-planner_amd")
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    spec = pop.config.make_spec("cfg2")
    scene = pop.scene.make_scene(128, (spec.L // 2) * 0.15, seed=0x5069)
    tl = pop.scene.WorldTimeline(scene, driver.TICK_PERIOD, moving=True)
    out = {"workload": "world frames, cfg2 scene for 128 agents (seed 0x5069), block_points 256", **per_frame(pop, sogm, tl, a.repeats, a.batch)}
    if a.ticks > 0:
        runs = {False: [], True: []}
        for _ in range(a.flights):
            for dw in (False, True):
                runs[dw].append(lock_step(driver, a.ticks, dw, scene))
        for dw, name in ((False, "host_frames"), (True, "device_frames")):
            out[f"lock_step_{name}"] = {"ticks": a.ticks, "ms_per_tick": stat([r[0] for r in runs[dw]], 3),
                                       "frame_bytes_held_at_end": runs[dw][0][1], "ok_last_tick": runs[dw][0][2]}
    print(json.dumps(out))
