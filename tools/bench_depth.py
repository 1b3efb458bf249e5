"""Timing of the depth camera (sogm_render_depth, include/sogm_abi.h "depth camera"): A cameras, 480 x 640, on the cfg2
moving world (make_scene(A, 15 m, 0x5069) through WorldTimeline, one frame per tick), alone and back to back with its two
consumers (sogm_gridmap_update; sogm_filter_point_cloud).  The cameras stand on a 12 m circle and look at its centre, so that
every one is inside the GridMap's 40 x 40 m map.  HIP events on the launch stream around every timed call, all inputs
resident before the first one.  Prints one JSON line.

Three more renders of the same frames say what bounds the kernel: the image alone (the same arithmetic, 2 of the 14 bytes
per pixel), an empty world with the ground (all 14 bytes, next to no arithmetic), and the full render.

--bodies N renders through sogm_render_depth_swarm ("agent bodies") instead: every camera's own carrier (a 0.4 x 0.4 x 0.45
box 0.1 m behind and 0.05 m below the camera, not drawn for it) plus N - cameras bystanders hovering inside the circle
become bodies (N below the number of cameras: only the first N cameras are carried); --bodies 0 is that entry without
bodies, i.e. the cost of carrying the hit codes.  --hit also asks for the hit image (4 more bytes per pixel).

--labels (with --bodies N) also times the labelled filter (sogm_filter_point_cloud_labelled, "ground-truth labels") in the same
run, next to the plain one: the render then always writes the hit image, every body gets a velocity from SplitMix64, and
filter_labelled_ms / render_then_filter_labelled_ms stand beside filter_ms / render_then_filter_ms, with their ratio.

--noise also times the sensor-noise pass (sogm_depth_noise, "sensor noise": sigma 0.002, 0.003, 0.004, 5 % dropout, half the
pixels at 0.15 m edges, nothing below 0.3 m) on the last rendered frame — with the cloud (and the hit image, when the render
gave one), the image alone — and behind the render; noise_GBps_algorithmic counts the bytes the definition moves: 2 + 2 per
pixel, + 12 with the cloud, + 4 + 4 with the hit image."""
import argparse, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch


def candidates(cyl, cam, pos, rot):
    """per camera: the type-3 records k_render_depth's cull keeps (csrc/sogm_depth.hip, restated: it is the same list for
    every workgroup of an agent) — xy distance to the axis <= max_depth * max |d_xy| over the image corners + r"""
    out = []
    xs = [(0.0 - cam.cx) / cam.fx, (cam.cols - 1 - cam.cx) / cam.fx]
    ys = [(0.0 - cam.cy) / cam.fy, (cam.rows - 1 - cam.cy) / cam.fy]
    for p, R in zip(pos, rot.reshape(-1, 3, 3)):
        a = max((R[0, 0] * x + R[0, 1] * y + R[0, 2]) ** 2 + (R[1, 0] * x + R[1, 1] * y + R[1, 2]) ** 2 for x in xs for y in ys)
        far = cam.max_depth * np.sqrt(a) * (1.0 + 1e-6) + 0.5 * cyl[:, 2] * (1.0 + 1e-6)
        out.append(int(((cyl[:, 0] - p[0]) ** 2 + (cyl[:, 1] - p[1]) ** 2 <= far * far).sum()))
    return out


def camera_ring(pop, A):
    """A cameras on a 12 m circle looking roughly at its centre, in GENERAL position: no pose component is a round number.
    The reference's RayCaster (raycast.cpp:242-335; the oracle's and k_gm_paths' walk alike) never reaches its end cell from a
    ray end that lies exactly on a voxel boundary, and the clean frames of an axis-aligned camera at z = 1.0 have such ends
    (ground returns at z = 0.0 exactly: row 330, depth 4300) — a real sensor's pose and noise never do."""
    th = 2.0 * np.pi * np.arange(A) / A + 0.1
    return [pop.scene.camera_pose(12.0 * np.cos(t), 12.0 * np.sin(t), 1.03 + 0.0111 * np.sin(a + 1.0), t + np.pi + 0.05 * np.sin(a))
            for a, t in enumerate(th)]


def swarm_bodies(pop, pos, rot, n_bodies):
    """(body centres [n_bodies, 3], cam_body [A]) of --bodies: carriers first, then bystanders from SplitMix64"""
    A = len(pos)
    ahead = rot.reshape(-1, 3, 3)[:, :, 2]
    carriers = pos - 0.1 * ahead * [1.0, 1.0, 0.0] - [0.0, 0.0, 0.05]
    rng = pop.scene.SplitMix64(0xB0D1)
    extra = [[rng.uniform(-11.0, 11.0), rng.uniform(-11.0, 11.0), rng.uniform(0.5, 2.0)] for _ in range(max(n_bodies - A, 0))]
    bodies = np.concatenate([carriers[:min(n_bodies, A)], np.array(extra, np.float64).reshape(-1, 3)])
    return bodies, np.array([a if a < n_bodies else -1 for a in range(A)], np.int32)


def run(A, steps=30, warmup=5, rings=0, bodies=-1, hit=False, labels=False, noise=False):
    pop = importlib.import_module("pred-occ-planner_amd")
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    gm = importlib.import_module("pred-occ-planner_amd.gridmap")
    depth = importlib.import_module("pred-occ-planner_amd.depth")
    sc = pop.scene.make_scene(A, 15.0, seed=0x5069, n_rings=rings)     # rings = 0: the scene as it always was
    tl = pop.scene.WorldTimeline(sc, 0.1)
    cam = depth.make_depth_camera()
    poses = camera_ring(pop, A)
    pos, rot = np.stack([p for p, _ in poses]), np.stack([R.reshape(9) for _, R in poses])
    pos_d, rot_d = sogm._dev(pos, np.float64), sogm._dev(rot, np.float64)
    n = warmup + steps
    none = np.zeros((0, 3), np.float32)
    if rings:   # --rings N: the same world with N rings, rendered with SOGM_DEPTH_RINGS
        worlds = [sogm.World(none, *tl.records(k)) for k in range(n)]
    else:
        worlds = [sogm.World(none, tl.cylinders(k)) for k in range(n)]
    empty = sogm.World(none, np.zeros((0, 5)))
    g = gm.GridMap(gm.make_gridmap_params(), A)
    m = sogm.SogmMap(pop.config.make_spec("cfg1", map_kind=pop._abi.SOGM_MAP_RISKVOXEL), A)
    n_cand = [candidates(tl.cylinders(k), cam, pos, rot) for k in (warmup, n - 1)]

    def timed(fn):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(steps)]
        for k in range(n):
            e = ev[k - warmup] if k >= warmup else None
            if e: e[0].record()
            fn(k)
            if e: e[1].record()
        torch.cuda.synchronize()
        ms = np.array([e[0].elapsed_time(e[1]) for e in ev])
        return {"mean": round(float(ms.mean()), 4), "min": round(float(ms.min()), 4), "max": round(float(ms.max()), 4)}

    keep = {}
    if bodies >= 0:
        body_h, own_h = swarm_bodies(pop, pos, rot, bodies)
        body_d, own_d = sogm._dev(body_h, np.float64), sogm._dev(own_h, np.int32)
        vrng = pop.scene.SplitMix64(0xB0D2)
        vel_d = sogm._dev(np.array([[vrng.uniform(-1.0, 1.0) for _ in range(3)] for _ in body_h], np.float64).reshape(-1, 3),
                          np.float64)
    hit = hit or labels

    def render(k, want_cloud=True, world=None):
        if bodies >= 0:
            keep["out"] = depth.render_depth_swarm(world or worlds[k], cam, pos_d, rot_d, body_d, own_d, rings=bool(rings),
                                                   want_cloud=want_cloud, want_hit=hit)
            keep["hit"] = keep["out"][4]
            keep["out"] = keep["out"][:4]
        else:
            keep["out"] = depth.render_depth(world or worlds[k], cam, pos_d, rot_d, want_cloud, rings=bool(rings))
        return keep["out"]

    def render_gridmap(k):
        d = render(k, False)[0]
        keep["upd"] = g.update(d, pos_d, rot_d)

    def render_filter(k):
        _, cl, rng, _ = render(k)
        keep["flt"] = m.filterPointCloud(cl, rng, 0.15, 5000)

    t_render = timed(render)
    d16 = keep["out"][0]
    returns = float((d16 != 0).float().mean().item())
    t_image = timed(lambda k: render(k, False))
    t_ground = timed(lambda k: render(k, True, empty))
    t_gridmap = timed(lambda k: keep.__setitem__("upd", g.update(d16, pos_d, rot_d)))
    t_rg = timed(render_gridmap)
    _, cl, rng, _ = render(n - 1)
    hit_last = keep.get("hit")      # the hit image of the frame `cl` is
    t_filter = timed(lambda k: keep.__setitem__("flt", m.filterPointCloud(cl, rng, 0.15, 5000)))
    t_rf = timed(render_filter)
    if labels:
        def filter_labelled(k):
            keep["lab"] = m.filterPointCloudLabelled(cl, hit_last, rng, worlds[n - 1], vel_d, 0.05, 0.15, 5000)

        def render_filter_labelled(k):
            _, cl_k, rng_k, _ = render(k)
            keep["lab"] = m.filterPointCloudLabelled(cl_k, keep["hit"], rng_k, worlds[k], vel_d, 0.05, 0.15, 5000)

        t_fl = timed(filter_labelled)
        t_rfl = timed(render_filter_labelled)
        t_filter_again = timed(lambda k: keep.__setitem__("flt", m.filterPointCloud(cl, rng, 0.15, 5000)))
    if noise:
        nz = [depth.make_depth_noise(0x5067, k, 0, (0.002, 0.003, 0.004), 0.05, 0.15, 0.5, 0.3) for k in range(n)]
        d_last = render(n - 1)[0]
        h_noise = keep.get("hit")

        def render_noise(k):
            d_k = render(k)[0]
            keep["noise"] = depth.add_depth_noise(cam, nz[k], d_k, keep.get("hit"))

        t_noise = timed(lambda k: keep.__setitem__("noise", depth.add_depth_noise(cam, nz[k], d_last, h_noise)))
        noise_counts = keep["noise"][3].sum(dim=0).tolist()
        t_noise_image = timed(lambda k: keep.__setitem__("noise", depth.add_depth_noise(cam, nz[k], d_last, None, want_cloud=False)))
        t_rn = timed(render_noise)
    nbytes = A * cam.rows * cam.cols * 14
    out = {"agents": A, "cylinders": int(len(sc["cylinders"])), "rings": int(rings), "frames_timed": steps,
           "render_ms": t_render, "render_GBps_algorithmic": round(nbytes / (t_render["mean"] * 1e-3) / 1e9, 1),
           "algorithmic_bytes": nbytes, "pixels_with_return": round(returns, 3),
           "candidates_per_workgroup_mean": round(float(np.mean(n_cand)), 2), "candidates_per_workgroup_max": int(np.max(n_cand)),
           "render_image_only_ms": t_image, "render_empty_world_ground_ms": t_ground,
           "gridmap_update_ms": t_gridmap, "render_then_gridmap_ms": t_rg,
           "filter_ms": t_filter, "render_then_filter_ms": t_rf,
           "gridmap_updated": int(keep["upd"].sum().item()), "filtered_points_agent0": int(keep["flt"][1][0].item())}
    if bodies >= 0:
        out.update({"entry": "sogm_render_depth_swarm", "bodies": int(len(body_h)), "hit_image": bool(hit)})
    if labels:
        lab, cnt0 = keep["lab"][2], int(keep["lab"][1][0].item())
        out.update({"filter_labelled_ms": t_fl, "render_then_filter_labelled_ms": t_rfl,
                    "filter_ms_after_labelled": t_filter_again,      # the plain entry once the key array exists
                    "filter_labelled_over_filter": round(t_fl["mean"] / t_filter["mean"], 3),
                    "labelled_points_agent0": int((lab[0, :cnt0, 3] > 0).sum().item()), "filtered_points_labelled_agent0": cnt0})
    if noise:
        nb = A * cam.rows * cam.cols * (16 + (8 if h_noise is not None else 0))
        out.update({"noise_ms": t_noise, "noise_image_only_ms": t_noise_image, "render_then_noise_ms": t_rn,
                    "noise_algorithmic_bytes": nb, "noise_GBps_algorithmic": round(nb / (t_noise["mean"] * 1e-3) / 1e9, 1),
                    "noise_counters": dict(zip(pop._abi.DEPTH_NOISE_COUNTERS, noise_counts))})
    g.close()
    m.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rings", type=int, default=0, help="ring obstacles in the world, drawn (default 0: cylinders only)")
    ap.add_argument("--bodies", type=int, default=-1, help="render through sogm_render_depth_swarm with N bodies (default: "
                    "sogm_render_depth, today's run)")
    ap.add_argument("--hit", action="store_true", help="with --bodies: also ask for the hit image")
    ap.add_argument("--labels", action="store_true", help="with --bodies: also time sogm_filter_point_cloud_labelled on the hit "
                    "image (implies --hit)")
    ap.add_argument("--noise", action="store_true", help="also time the sensor-noise pass (sogm_depth_noise) on the rendered frames")
    a = ap.parse_args()
    assert a.steps >= 20 and torch.cuda.is_available(), "needs a GPU and at least 20 timed frames"
    assert not a.labels or a.bodies >= 0, "--labels needs --bodies N (the hit image comes from sogm_render_depth_swarm)"
    print(json.dumps({"workload": "sogm_render_depth, 480x640 per camera, cfg2 moving world (seed 0x5069), cameras on a 12 m "
                                  "circle; ms per frame: HIP events on the launch stream around each call",
                      "runs": [run(A, a.steps, a.warmup, a.rings, a.bodies, a.hit, a.labels, a.noise) for A in a.agents]}))
