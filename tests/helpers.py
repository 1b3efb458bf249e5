"""Shared test helpers (not collected)."""
import importlib

import numpy as np


def hard_cases(pop, A, seed, field=7.0):
    """Scene whose agents start at random places INSIDE the obstacle field with random velocity
    (so that A* has to route around cylinders and other agents)."""
    sc = pop.scene.make_scene(A, 4.95, seed=seed, moving=True, circle_radius=8.0)
    rng = np.random.default_rng(seed)
    cyl = sc["cylinders"]
    starts = np.zeros((A, 3))
    for a in range(A):
        for _ in range(1000):
            p = rng.uniform(-field, field, 2)
            d = np.hypot(cyl[:, 0] - p[0], cyl[:, 1] - p[1]) - cyl[:, 2] * 0.5
            if d.min() > 0.9 and (a == 0 or np.hypot(*(starts[:a, :2] - p).T).min() > 1.6):
                break
        starts[a] = (p[0], p[1], rng.uniform(0.6, 1.8))
    goals = starts + np.concatenate([rng.uniform(-9, 9, (A, 2)), np.zeros((A, 1))], axis=1)
    goals[:, 2] = 1.0
    vel = rng.uniform(-1.0, 1.0, (A, 3)) * np.array([1, 1, 0.2])
    acc = rng.uniform(-2.0, 2.0, (A, 3)) * np.array([1, 1, 0.2])
    sc["starts"], sc["goals"] = starts, goals
    sc["poses"] = starts.astype(np.float32).copy()
    pva = np.concatenate([starts, vel, acc], axis=1)
    return sc, pva


def pocket_cloud(pose, half_width, depth, back=0.6, step=0.1):
    """Static wall points (no cylinder record: velocity zero) forming a U-shaped pocket that opens towards -x around `pose`:
    a front wall at x = pose.x + depth and two side walls at y = pose.y +- half_width reaching back to x = pose.x - back,
    floor to ceiling.  A search towards +x has to explore the pocket before it backs out: hundreds of expansions
    (tests/golden/make_astar_fixture.py, tests/test_astar_independent.py)."""
    zs = np.arange(0.05, 3.0, step)
    ys = np.arange(-half_width, half_width + 1e-6, step)
    xs = np.arange(-back, depth + 1e-6, step)
    front = np.stack(np.meshgrid([depth], ys, zs, indexing="ij"), -1).reshape(-1, 3)
    left = np.stack(np.meshgrid(xs, [-half_width], zs, indexing="ij"), -1).reshape(-1, 3)
    right = np.stack(np.meshgrid(xs, [half_width], zs, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate([front, left, right]) + np.asarray(pose, np.float64)[None, :] * np.array([1.0, 1.0, 0.0])
    return pts.astype(np.float32)


def oracle_grids(pop, orc, spec, sc, recs):
    cyl = pop.scene.cylinders_to_struct(sc["cylinders"])
    body = pop.scene.received_body_particles()
    out = []
    A = sc["n_agents"]
    for a in range(A):
        g = orc.update_gt(spec, sc["cloud"], cyl, len(sc["cylinders"]), sc["poses"][a])
        if recs is not None:
            orc.project_neighbours(spec, g, recs, A, a, body, sc["poses"][a], sc["stamps"][a])
        out.append(g)
    return out


def approaching_cylinder_scene(pop, gx, cy, vy):
    """One agent at the origin (z = 1), goal `gx` metres ahead, one cylinder beside the goal at (gx, cy) moving
    with velocity (0, vy): slice 0 and the later slices differ around the goal — the situation in which
    FakeRiskHybridAstar's shot check (with time) and RiskHybridAstar's (slice 0) give different return codes."""
    sc = pop.scene.make_scene(1, 4.95, seed=1, n_cyl=0)
    sc["starts"][0] = (0, 0, 1)
    sc["goals"][0] = (gx, 0, 1)
    sc["poses"][0] = (0, 0, 1)
    cyl = np.array([[gx, cy, 0.6, 0.0, vy]])
    sc["cylinders"] = cyl
    zs = np.arange(0, 40) * 0.1
    x, y, w = cyl[0, :3]
    r = w * 0.5
    gxx, gyy = np.meshgrid(np.arange(int(np.floor((x - r) / 0.1)), int(np.ceil((x + r) / 0.1)) + 1) * 0.1,
                           np.arange(int(np.floor((y - r) / 0.1)), int(np.ceil((y + r) / 0.1)) + 1) * 0.1,
                           indexing="ij")
    d = np.hypot(gxx - x, gyy - y)
    m = (d <= r) & (d > r - 0.15)
    sx, sy = gxx[m], gyy[m]
    sc["cloud"] = np.ascontiguousarray(
        np.stack([np.repeat(sx, zs.size), np.repeat(sy, zs.size), np.tile(zs, sx.size)], axis=1), np.float32)
    return sc


class OracleCompute:
    """The CPU oracle standing in for driver.HipCompute (the four kernels calls of a tick), so that the rank-local
    bookkeeping of driver.SwarmTick.step() — tick inputs, map update from the EXCHANGED records, replan, latest-wins
    merge, the all-gather — runs on CPU over gloo (tests/test_driver_gloo.py).  Test infrastructure only."""
    device = "cpu"
    ctx = None

    def __init__(self, pop, orc, spec, scene, lo, hi, timeline=None):
        self.pop, self.orc, self.spec, self.scene, self.lo, self.hi = pop, orc, spec, scene, lo, hi
        self.timeline = timeline  # scene.WorldTimeline: the sensor frame of every tick (None: the frozen scene)
        self.abi = pop._abi
        self.ap, self.pp, self.qs = (pop.config.make_astar_params(), pop.config.make_planner_params(True),
                                     pop.config.make_qp_settings())
        self.cyl = pop.scene.cylinders_to_struct(scene["cylinders"])
        self.body = pop.scene.received_body_particles()
        self.grids, self.swarm, self.pub = [None] * (hi - lo), None, None
        self.overlay_sums = []   # (tick stamp, agent, sum of the SOGM, hash of the occupied cells) per agent-update

    def set_swarm(self, all_records, A_tot, now):
        self.swarm = (all_records, A_tot)

    def set_publish(self, own, next_table):
        self.pub = (own, next_table)

    def _records(self, t):
        n = t.shape[0]
        return (self.abi.SogmTrajRecord * n).from_buffer_copy(t.numpy().tobytes())

    def tick_inputs(self, own, stamp, hover, now, t_start, pva, poses):
        """k_tick_inputs (csrc/sogm_traj.hip) restated: start state = the executed trajectory at stamp + 0.02, or
        the hover state; hover <- position with zero velocity / acceleration."""
        import importlib
        drv = importlib.import_module("pred-occ-planner_amd.driver")
        recs = self._records(own)
        ts = stamp + drv.REPLAN_START_TIME
        for i in range(own.shape[0]):
            r = recs[i]
            if r.n_pieces > 0:
                d = np.array(r.duration[:r.n_pieces])
                c = np.array(r.cpts[:15 * r.n_pieces]).reshape(-1, 3)
                tt = min(max(ts - r.time_start, 0.0), d.sum())
                o = np.concatenate([self.orc.bezier_eval(d, c, tt, k) for k in range(3)])
            else:
                o = hover[i].numpy().copy()
            pva[i] = torch_from(o)
            hover[i, :3] = torch_from(o[:3])
            hover[i, 3:] = 0.0
            poses[i] = torch_from(o[:3].astype(np.float32))
        now.fill_(stamp)
        t_start.fill_(ts)

    def update_map(self, poses, now, all_records, A_tot, tick=0):
        recs = self._records(all_records)
        cloud, cyl = self.scene["cloud"], self.cyl
        if self.timeline is not None:
            f = self.timeline.frame(tick)
            cloud, cyl = f["cloud"], self.pop.scene.cylinders_to_struct(f["cylinders"])
        for i in range(self.hi - self.lo):
            pose = poses[i].numpy()
            g = self.orc.update_gt(self.spec, cloud, cyl, len(self.scene["cylinders"]), pose)
            self.orc.project_neighbours(self.spec, g, recs, A_tot, self.lo + i, self.body, pose, float(now[i]))
            self.grids[i] = g
            self.overlay_sums.append((round(float(now[i]), 6), self.lo + i, float(g.sum()),
                                      int(np.flatnonzero(g.ravel()).sum() % 1000003)))

    def replan(self, pva, goals, t_start, new, ok):
        import torch
        allr = self._records(self.swarm[0]) if self.swarm else None
        for i in range(self.hi - self.lo):
            a = self.lo + i
            pose = pva[i, :3].numpy().astype(np.float32)
            stamp = float(t_start[i]) - 0.02
            okk, rec, _ = self.orc.replan(self.spec, self.ap, self.pp, self.qs, self.grids[i], pose, stamp,
                                          pva[i].numpy(), goals[i].numpy(), float(t_start[i]), a)
            if okk and allr is not None:  # isSafeAfterOpt, the last step of replan() (baseline_fake.cpp:453-460)
                okk = self.orc.safe_after_opt(np.asarray(rec.cpts[:15 * rec.n_pieces]), rec.n_pieces, allr,
                                              self.swarm[1], a, stamp)
            ok[i] = int(bool(okk))
            new[i] = torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.uint8).copy())
        if self.pub is not None and self.pub[0] is not None:  # sogm_planner_set_publish restated
            own, table = self.pub
            own.copy_(new.where(ok.bool().unsqueeze(1), own))
            if table is not None:
                table.copy_(own)

    def merge_latest(self, new, ok, own, all_records):
        """k_merge_latest restated: a successful replan replaces the agent's record, a failed one keeps it; the
        swarm table (single process only) is refreshed in the same pass."""
        sel = ok.bool().unsqueeze(1)
        own.copy_(new.where(sel, own))
        if all_records is not None:
            all_records.copy_(own)

    def close(self):
        pass


def torch_from(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))



def filter_fixture_clouds():
    """camera frame: x right, y down, z forward"""
    out = []
    rng = np.random.default_rng(20260929)
    a = np.stack([rng.uniform(-4, 4, 30000), rng.uniform(-1.2, 1.2, 30000), rng.uniform(0.3, 4.5, 30000)], 1).astype(np.float32)
    out.append(("uniform box", a))
    b = a[:12000].copy()
    b[::531] = np.nan                      # invalid depth pixels
    b[5::977, 2] = np.inf
    out.append(("with non-finite points", b))
    # a wall 3 m ahead sampled like a depth image (dense: many points per leaf) + points beyond every range
    u, v = np.meshgrid(np.linspace(-2.5, 2.5, 260), np.linspace(-1.0, 1.0, 110))
    wall = np.stack([u.ravel(), v.ravel(), np.full(u.size, 3.0) + 0.02 * np.sin(7 * u.ravel())], 1).astype(np.float32)
    far = np.float32([[0.0, 0.0, 9.0], [0.2, 0.1, 9.3], [6.0, 0.0, 1.0], [0.0, -1.6, 2.0]])
    out.append(("wall + out of range", np.concatenate([wall, far])))
    out.append(("empty", np.zeros((0, 3), np.float32)))
    # > 5000 leaves inside the range: the cap
    g = np.stack(np.meshgrid(np.arange(-30, 30), np.arange(-6, 6), np.arange(3, 28), indexing="ij"), -1).reshape(-1, 3)
    out.append(("the cap", (g * 0.15 + 0.07).astype(np.float32)))
    # coordinates exactly on leaf boundaries and exactly on the range
    e = np.float32([[0.15, 0.0, 0.3], [0.3, 0.15, 0.45], [-0.15, -0.15, 0.15], [0.0, 0.0, 4.95], [0.0, 0.0, 4.9499998],
                    [4.95, 0.0, 1.0], [-4.9499998, 0.0, 1.0], [0.0, 1.5, 1.0], [0.0, 1.4999999, 1.0], [0.0, -1.5, 1.0]])
    out.append(("boundaries", e))
    return out


def gridmap_fixture_params():
    """the small test map of tests/test_gridmap.py as a plain dict (inputs of tests/golden/make_gridmap_fixture.py)"""
    return {"resolution": 0.1, "map_size": [12.0, 12.0, 3.0], "local_update_range": [4.0, 4.0, 2.0], "obstacles_inflation": 0.099,
            "fx": 387.0, "fy": 387.0, "cx": 320.0, "cy": 240.0, "depth_filter_maxdist": 5.0, "depth_filter_mindist": 0.2,
            "k_depth_scaling_factor": 1000.0, "p_hit": 0.70, "p_miss": 0.35, "p_min": 0.12, "p_max": 0.97, "p_occ": 0.80,
            "max_ray_length": 4.5, "virtual_ceil_height": 2.5, "ground_height": -0.01, "use_depth_filter": 1,
            "depth_filter_margin": 2, "skip_pixel": 2, "local_map_margin": 5, "rows": 480, "cols": 640}


def gridmap_fixture_frames(n=9):
    """depth images + camera poses of a camera creeping through the small map (frame 0 only arms the depth filter; five hits
    take a cell from unknown to occupied)"""
    pop = importlib.import_module("pred-occ-planner_amd")
    out = []
    for k in range(n):
        img = pop.scene.make_depth_image(k % 2)
        cam, R = pop.scene.camera_pose(-3.0 + 0.02 * k, 0.05 * np.sin(0.4 * k), 1.0 + 0.005 * k, 0.04 * np.sin(0.5 * k))
        out.append((img, cam, R))
    return out



def dsp_fixture_inputs(n_updates=4, seed=7):
    """the injected tables (Gaussian position / velocity noise, rand()) and a synthetic sensor sequence with labels for
    tests/golden/make_dsp_fixture.py and tests/test_dsp_independent.py"""
    pop = importlib.import_module("pred-occ-planner_amd")
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    tables = dsp.make_tables(11, n_gauss=1 << 18, n_rand=1 << 12)
    seq = pop.scene.make_dsp_sequence(seed, n_updates, half=(66 * 0.15 / 2, 66 * 0.15 / 2, 20 * 0.15 / 2))
    return tables, seq



# ---- velocityEstimationThread: the INPUTS of tests/golden/make_velocity_fixture.py and tests/test_velocity_independent.py.
# Scenes are built in WORLD coordinates that are multiples of 1 / 1024 (or searched float by float where a case is deliberately
# exact), seen from an exactly representable sensor position with the identity attitude: world - position is exact in float32 and
# the reference's forward transform gives the intended coordinates back (the generator asserts it).  Nothing here decides
# anything about the expected output.

VEL_POS = (0.0, 0.0, 0.5)
VEL_T0, VEL_DT = 20.0, 0.5


def _vel_rng(seed):
    return importlib.import_module("pred-occ-planner_amd").scene.SplitMix64(seed)


def _vel_q(a):
    return np.round(np.asarray(a, np.float64) * 1024.0) / 1024.0


def _vel_shuffle(seed, n):
    """Fisher-Yates on the project's SplitMix64 (explicit: the stream never changes)."""
    rng = _vel_rng(seed)
    p = list(range(n))
    for i in range(n - 1, 0, -1):
        j = rng.next_u64() % (i + 1)
        p[i], p[j] = p[j], p[i]
    return np.asarray(p, np.int64)


def vel_blob(n, cx, cy, z0=0.25, w=3, step=0.125):
    """n points of a w x w x k lattice (spacing 0.125 < the 0.3 m tolerance: one component), lowest corner (cx, cy, z0)."""
    i = np.arange(n)
    return _vel_q(np.stack([cx + (i % w) * step, cy + ((i // w) % w) * step, z0 + (i // (w * w)) * step], 1))


def vel_ground(n, x0=1.0, y0=-6.0, z=0.0625, cols=40):
    i = np.arange(n)
    return _vel_q(np.stack([x0 + (i % cols) * 0.25, y0 - (i // cols) * 0.25, np.full(n, z)], 1))


def vel_snake(n, x0, y0, z, L=12, step=0.25):
    """n nodes of a path that snakes over a lattice of `step` (rows two lattice steps apart, one node between the row ends):
    consecutive nodes 0.25 m apart, every other pair >= 0.35 m — one component whose graph diameter is n - 1."""
    nodes, x, y, d = [], 0, 0, 1
    while len(nodes) < n:
        nodes.append((x, y))
        at_end = (x == L) if d == 1 else (x == 0)
        if y % 2 == 1:
            y, d = y + 1, -d
        elif at_end:
            y += 1
        else:
            x += d
    nodes = np.asarray(nodes, np.float64)
    return _vel_q(np.stack([x0 + nodes[:, 0] * step, y0 + nodes[:, 1] * step, np.full(n, z)], 1))


def vel_combs(x0, y0, z=0.5):
    """Two combs, tooth between tooth, 0.35 m apart everywhere (> the 0.3 m tolerance): they must stay two components."""
    a, b = [], []
    for i in range(29):
        a.append((0.125 * i, 0.0))
        b.append((0.125 * i, 1.35))
    for t in range(6):
        a += [(0.7 * t, 0.125 * j) for j in range(1, 9)]
    for t in range(5):
        b += [(0.35 + 0.7 * t, 1.35 - 0.125 * j) for j in range(1, 9)]
    out = []
    for c in (a, b):
        c = np.asarray(c, np.float64)
        out.append(_vel_q(np.stack([x0 + c[:, 0], y0 + c[:, 1], np.full(len(c), z)], 1)))
    return out


def _vel_frame(parts, stamp, pos=VEL_POS, shuffle=None, world32=None):
    if world32 is None:
        world = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p in parts])
        world32 = world.astype(np.float32)
        assert np.array_equal(world32.astype(np.float64), world)
    if shuffle is not None:
        world32 = world32[_vel_shuffle(shuffle, len(world32))]
    p32 = np.asarray(pos, np.float32)
    return {"points": np.ascontiguousarray(world32 - p32[None, :], np.float32), "world": world32, "pos": p32,
            "quat": np.float32([1, 0, 0, 0]), "stamp": float(stamp)}


def vel_round_f32(fr):
    """The float32 nearest to a Fraction, ties to even — exactly (no double rounding through float64)."""
    from fractions import Fraction
    c = np.float32(float(fr))
    best = None
    for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        e = abs(Fraction(float(v)) - fr)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        if best is None or e < best[0] or (e == best[0] and even):
            best = (e, np.float32(v))
    return best[1]


def vel_d2_separate(a, b):
    """FLANN's L2 on three floats: diff = a - b, result += diff * diff — every operation rounded to float32."""
    f = np.float32
    s = f(0)
    for i in range(3):
        d = f(f(a[i]) - f(b[i]))
        s = f(s + f(d * d))
    return s


def vel_d2_fused(a, b):
    """The same loop with every `result += diff * diff` contracted into one fma: exact product, one rounding."""
    from fractions import Fraction
    f = np.float32
    s = f(0)
    for i in range(3):
        d = Fraction(float(f(f(a[i]) - f(b[i]))))
        s = vel_round_f32(d * d + Fraction(float(s)))
    return s


def vel_r2():
    t = np.float32(2) * np.float32(0.15)            # setClusterTolerance(2 * voxel_filtered_resolution): a float product
    return np.float32(float(t) * float(t))            # FLANN's radius: (float)(tolerance * tolerance), the product in double


def _vel_two_lines(a, b):
    """Two 5-point lines leaving a towards -x and b towards +x (spacing 0.125, b.x >= a.x): the closest pair between the two
    groups is (a, b), every other cross pair is at least 0.125 m farther apart in x."""
    pts = []
    for p, sg in ((a, -1.0), (b, 1.0)):
        for k in range(5):
            q = np.asarray(p, np.float32).copy()
            q[0] = np.float32(float(q[0]) + sg * 0.125 * k)
            pts.append(q)
    return np.asarray(pts, np.float32)


def vel_strict_3d_pairs(want, anchors):
    """Search, one pair per anchor: points a, b with all three differences non-zero whose separately rounded and fused squared
    distances fall on different sides of r2.  want = +1: separate < r2 <= fused; -1: fused < r2 <= separate."""
    f = np.float32
    r2 = vel_r2()
    rng = _vel_rng(0x3D00 + (want > 0))
    out = []
    for ax, ay in anchors:
        while True:
            a = f([ax + rng.uniform(0, 0.01), ay + rng.uniform(0, 0.01), 0.25 + rng.uniform(0, 0.01)])
            dx, dy = rng.uniform(0.10, 0.19), rng.uniform(0.10, 0.19)
            dz = np.sqrt(float(r2) - dx * dx - dy * dy)
            b0 = f([float(a[0]) + dx, float(a[1]) + dy, float(a[2]) + dz])
            hit = None
            for k in range(-3, 4):
                b = b0.copy()
                for _ in range(abs(k)):
                    b[2] = np.nextafter(b[2], f(np.inf if k > 0 else -np.inf))
                s, u = vel_d2_separate(b, a), vel_d2_fused(b, a)
                if (s < r2 <= u) if want > 0 else (u < r2 <= s):
                    hit = (a, b)
                    break
            if hit:
                out.append(hit)
                break
    return out


def vel_strict_axis_steps():
    """(dx_out, dx_in): 0.3f, whose float32 square IS r2, and the largest float below it whose square is below r2."""
    f = np.float32
    r2 = vel_r2()
    dx_out = f(2) * f(0.15)
    assert f(dx_out * dx_out) == r2
    dx_in = dx_out
    while not f(dx_in * dx_in) < r2:
        dx_in = np.nextafter(dx_in, f(0))
    return dx_out, dx_in


def _vel_swarm(seed, n_frames=4, n_tracks=26, max_alive=20):
    """Tracks that appear, vanish and cross: pairwise distinct sizes, blobs at least 1 m apart in every frame."""
    rng = _vel_rng(seed)
    sizes = [5 + 2 * int(i) for i in _vel_shuffle(seed + 1, n_tracks)]
    tracks = []
    while len(tracks) < n_tracks:
        p = np.array([rng.uniform(0, 11), rng.uniform(-5, 6)])
        v = np.array([rng.uniform(-1.3, 1.3), rng.uniform(-1.3, 1.3)])
        f0 = int(rng.uniform(0, 2.2))
        f1 = n_frames - int(rng.uniform(0, 2.2))
        z0 = 0.25 + 0.125 * int(rng.uniform(0, 4))
        ok = True
        for (q, u, g0, g1, _, _) in tracks:
            for k in range(max(f0, g0), min(f1, g1)):
                if np.hypot(*(p + v * k - q - u * k)) < 1.0:
                    ok = False
        if ok:
            tracks.append((p, v, f0, f1, z0, sizes[len(tracks)]))
    frames = []
    for k in range(n_frames):
        alive = [t for t in tracks if t[2] <= k < t[3]][:max_alive]
        parts = [vel_blob(t[5], *(t[0] + t[1] * k), z0=t[4]) for t in alive] + [vel_ground(7)]
        frames.append(_vel_frame(parts, VEL_T0 + VEL_DT * k, shuffle=seed + 10 + k))
    return frames


def _vel_grid_blobs(n, size, step, cols, k=0, z0=0.25, drift=0.0):
    return [vel_blob(size, (i % cols) * step + drift * k * ((i % 3) - 1), -4.0 + (i // cols) * step + drift * k * ((i % 2) - 0.5) * 2,
                     z0=z0) for i in range(n)]


def velocity_fixture_inputs():
    """The sequences of the second reading of velocityEstimationThread: a list of {branch, frames}, a frame = {points (sensor
    frame, float32), world (intended float32 world coordinates, where the attitude is the identity), pos, quat, stamp}."""
    f = np.float32
    T = lambda k: VEL_T0 + VEL_DT * k
    S = []

    def seq(branch, frames, **kw):
        S.append(dict(branch=branch, frames=frames, **kw))

    B, G = vel_blob, vel_ground
    # ---- clustering
    seq("size_4_dropped_5_kept", [_vel_frame([B(4, 2 + 0.25 * k, 0), B(5, 2, 2 + 0.25 * k), B(9, 3.5 - 0.25 * k, -2), G(6)],
                                             T(k), shuffle=100 + k) for k in range(3)])
    seq("size_200_dynamic_201_static", [_vel_frame([B(200, 2 + 0.25 * k, -2, w=5), B(201, 2, 2 + 0.25 * k, w=5),
                                                    B(10, 4, 0.25 * k), G(10)], T(k), shuffle=110 + k) for k in range(3)])
    seq("centre_above_1p5_static", [_vel_frame([B(18, 2 + 0.25 * k, -1, z0=1.45), B(18, 2 + 0.25 * k, 1, z0=1.40), G(5)],
                                               T(k), shuffle=120 + k) for k in range(3)])
    # the same SENSOR-frame cloud seen from z = 0.4f and from z = 2: (float)0.4 + (-0.25) is exactly (float)0.15 (ground: the
    # test is strict), -0.25 + 2^-26 lands one float above it (not ground).  From z = 2 the sums are multiples of 2^-23, which
    # (float)0.15 is not: the rows there sit on the last such multiple below it and on the first above it.
    row = lambda x0, y, s: np.stack([x0 + 0.125 * np.arange(6), np.full(6, y), np.full(6, s)], 1)
    v015 = float(f(0.15))
    lo2 = np.floor(v015 * 2.0 ** 23) / 2.0 ** 23
    cloud = np.concatenate([
        row(1.0, 0.0, -0.25), row(1.0, 0.125, -0.25 + 2.0 ** -26),             # from 0.4f: on / one float above 0.15f
        row(1.0, 2.0, lo2 - 2.0), row(1.0, 2.125, lo2 + 2.0 ** -23 - 2.0),     # from 2.0: just below / just above
        vel_blob(8, 3.0, 0.0, z0=-0.2) , vel_blob(12, 3.0, 2.0, z0=-1.8)]).astype(f)
    fr = []
    for k, pz in enumerate([f(0.4), f(2.0), f(0.4), f(2.0)]):
        p = cloud[_vel_shuffle(130 + k, len(cloud))]
        fr.append({"points": p, "pos": f([0, 0, pz]), "quat": f([1, 0, 0, 0]), "stamp": T(k)})
    seq("ground_split_on_world_z", fr)
    seq("all_ground", [_vel_frame([B(8, 2, 0), G(6)], T(0), shuffle=140), _vel_frame([G(12)], T(1), shuffle=141),
                       _vel_frame([B(8, 2.25, 0), G(6)], T(2), shuffle=142)])
    seq("no_accepted_cluster", [_vel_frame([B(8, 2, 0), G(6)], T(0), shuffle=150),
                                _vel_frame([B(3, 2, 0), B(4, 3, 1), B(1, 4, 2), B(2, 5, -1), G(6)], T(1), shuffle=151),
                                _vel_frame([B(8, 2.25, 0), G(6)], T(2), shuffle=152)])
    dx_out, dx_in = vel_strict_axis_steps()
    pts = []
    for i in range(6):
        axis, dx = i // 2, (dx_out, dx_in)[i % 2]
        a = f([[0.1875, 2.0 + 2 * i, 0.25], [4.0 + 2 * i, 0.1875, 0.25], [4.0 + 2 * i, 3.0, 0.1875]][axis])   # a + dx < 0.5: exact
        b = a.copy()
        b[axis] = f(a[axis] + dx)
        assert f(b[axis] - a[axis]) == dx
        pts.append(_vel_two_lines(a, b))
    w = np.concatenate(pts + [G(4).astype(f)])
    seq("tolerance_strict_axis", [_vel_frame(None, T(k), shuffle=160 + k, world32=w) for k in range(3)])
    anchors = [(2.0 * (i % 4), 2.0 * (i // 4) - 3.0) for i in range(16)]
    pairs = vel_strict_3d_pairs(+1, anchors[:8]) + vel_strict_3d_pairs(-1, anchors[8:])
    w = [np.concatenate([_vel_two_lines(a, b) for a, b in pairs[8 * h:8 * h + 8]] + [G(4).astype(f)]) for h in range(2)]
    seq("tolerance_strict_3d", [_vel_frame(None, T(k), shuffle=170 + k, world32=w[k % 2]) for k in range(4)],     # one direction per frame
        pairs=[(a.copy(), b.copy()) for a, b in pairs])
    for name in ("ascending", "descending", "shuffled"):
        fr = []
        for k in range(3):
            ch = vel_snake(180, -1.5, -4 + 0.25 * k, 0.5)
            if name == "descending":
                ch = ch[::-1]
            fr.append(_vel_frame([ch, B(12, 3, 3 + 0.25 * k), G(8)], T(k), shuffle=180 + k if name == "shuffled" else None))
        seq("chain_" + name, fr)
    big = lambda k: [B(216, 4 + 1.5 * i, 0.25 * k * (i % 2), w=6) for i in range(10)]
    seq("chain_across_trips", [_vel_frame([vel_snake(180, -1.5, -4 + 0.25 * k, 0.5)] + big(k) + [G(160)], T(k), shuffle=190 + k)
                               for k in range(3)])
    seq("interleaved_combs_stay_two", [_vel_frame(vel_combs(1 + 0.25 * k, -1) + [G(9)], T(k), shuffle=200 + k) for k in range(3)])
    for n in (1024, 1025, 2600):
        nb = int((n * 0.6 - 75) // 216)
        fr = []
        for k in range(3):
            parts = [B(30, 0.25 * k, 4), B(25, 1.5, 4 + 0.25 * k), B(20, 3 - 0.25 * k, 4)]
            parts += [B(216, 1.5 * (i % 4), -4 + 1.5 * (i // 4), w=6) for i in range(nb)]
            parts.append(G(n - 75 - 216 * nb))
            fr.append(_vel_frame(parts, T(k), shuffle=210 + n + k))
        seq("cloud_%d" % n, fr)
    # a general unit quaternion and a moving position: sensor = R(q)^-1 (world - position), computed in float64
    q = np.array([0.8, 0.2, -0.3, 0.4])
    q /= np.linalg.norm(q)
    qw, qx, qy, qz = q
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    fr = []
    for k in range(4):
        pos = np.array([0.3 * k, -0.2 * k, 1.0 + 0.1 * k])
        w = np.concatenate([B(14, 2 + 0.3 * k, 0), B(9, 3, 2 - 0.4 * k), B(22, 4 - 0.2 * k, -2, z0=0.5), B(216, 6, 0, w=6), G(30)])
        w = w[_vel_shuffle(230 + k, len(w))]
        fr.append({"points": ((w - pos) @ R).astype(f), "pos": pos.astype(f), "quat": q.astype(f), "stamp": T(k)})
    seq("rotated_moving_sensor", fr)
    # ---- association
    base = [(10, 2.0, -2.0), (8, 2.0, 0.0), (6, 2.0, 2.0)]
    new = [(20, 4.0, -1.0), (30, 4.0, 1.0)]
    seq("more_new_than_old", [_vel_frame([B(n, x + 0.25 * k, y) for n, x, y in base + new[:k]] + [G(6)], T(k), shuffle=300 + k)
                              for k in range(3)])
    five = [(14, 2.0, -3.0), (12, 2.0, -1.5), (10, 2.0, 0.0), (8, 2.0, 1.5), (6, 2.0, 3.0)]
    keep = [[0, 1, 2, 3, 4], [1, 3, 4], [3, 4]]
    seq("fewer_new_than_old", [_vel_frame([B(*[five[i][0], five[i][1] + 0.25 * k, five[i][2]]) for i in keep[k]] + [G(6)], T(k),
                                          shuffle=310 + k) for k in range(3)])
    na, nb_ = [10, 110, 10], [10, 111, 10]
    seq("point_num_gate_100_in_101_out", [_vel_frame([B(na[k], 2 + 0.25 * k, -2, w=4), B(nb_[k], 2 + 0.25 * k, 2, w=4), G(6)], T(k),
                                                     shuffle=320 + k) for k in range(3)])
    seq("distance_gate_in_and_out", [_vel_frame([B(10, 2 + 1.49 * k, -2), B(8, 2 + 1.51 * k, 2), G(6)], T(k), shuffle=330 + k)
                                     for k in range(3)])
    st = [20.0, 20.2, 20.4, 21.0]
    seq("faster_than_5_is_zeroed_but_matched", [_vel_frame([B(10, 2 + 1.2 * k, -2), B(8, 2 + 0.9 * k, 2), G(6)], st[k],
                                                           shuffle=340 + k) for k in range(4)])
    st = [20.0, 20.5, 20.5 + 5e-6, 21.5]
    seq("dt_too_small", [_vel_frame([B(10, 2 + 0.25 * k, -2), B(8, 2, 2 - 0.25 * k), G(6)], st[k], shuffle=350 + k)
                         for k in range(4)])
    st = [20.0, 30.0, 30.5]
    seq("dt_10_or_more", [_vel_frame([B(10, 2 + 0.25 * k, -2), B(8, 2, 2 - 0.25 * k), G(6)], st[k], shuffle=360 + k)
                          for k in range(3)])
    # two clusters 0.9 m apart, both stepping 0.8 m: the follower lands 0.1 m from where the leader WAS
    seq("greedy_differs_from_optimum", [_vel_frame([B(12, 0.8 * k, -2), B(8, 0.9 + 0.8 * k, -2), B(9, 3, 0.8 * k), B(7, 3, 0.9 + 0.8 * k),
                                                    G(6)], T(k), shuffle=370 + k) for k in range(7)])
    seq("assigned_to_a_gated_pair_is_no_match", [
        _vel_frame([B(10, 2, -2), G(6)], T(0), shuffle=380),
        _vel_frame([B(10, 2, 1), G(6)], T(1), shuffle=381),                       # 1 x 1: the only pairing is gated
        _vel_frame([B(10, 2.25, 1), B(7, 6, 6), G(6)], T(2), shuffle=382),        # 2 x 1
        _vel_frame([B(10, 2.5, 1), B(7, 6, 1), G(6)], T(3), shuffle=383)])        # 2 x 2: one match, one gated pairing
    seq("random_swarm", _vel_swarm(0x5A))
    seq("sixty_four_dynamic", [_vel_frame(_vel_grid_blobs(64, 5, 2.0, 8, k, drift=0.1) + [G(0)], T(k), shuffle=400 + k)
                               for k in range(3)])
    sizes = [5, 5, 5, 5, 6, 6, 6, 7, 7, 7, 9, 9, 12, 12, 12, 12]
    order = _vel_shuffle(410, 16)
    seq("tie_order_up_to_16", [_vel_frame([B(sizes[int(order[i])], (i % 4) * 1.5 + 0.25 * k, -3 + (i // 4) * 1.5) for i in range(16)]
                                          + [G(6)], T(k), shuffle=411 + k) for k in range(3)])
    return S


def vel_canonical_born(born, sizes_dyn, n_ground, sizes_static):
    """A new-born list with the blocks of EQUAL-SIZED clusters sorted by their bytes: for frames with ties among more than 16
    clusters, where the block order is libstdc++'s introsort's (sizes: the clusters' sizes in list order, descending)."""
    born = np.ascontiguousarray(born, np.float32).reshape(-1, 7)
    out, at = [], 0
    for sizes, skip in ((sizes_dyn, n_ground), (sizes_static, 0)):
        i = 0
        while i < len(sizes):
            j = i
            while j < len(sizes) and sizes[j] == sizes[i]:
                j += 1
            blocks = [born[at + k * sizes[i]: at + (k + 1) * sizes[i]] for k in range(j - i)]
            out += sorted(blocks, key=lambda b: b.tobytes())
            at += (j - i) * sizes[i]
            i = j
        out.append(born[at:at + skip])
        at += skip
    assert at == len(born)
    return np.concatenate(out) if out else born


def velocity_capacity_inputs():
    """Clouds AT and one OVER each capacity of k_dsp_velocity (two frames each; (name, frames, max_points of the handle))."""
    T = lambda k: VEL_T0 + VEL_DT * k
    B, G = vel_blob, vel_ground
    dense = lambda n, k: vel_blob(n, 2 + 0.25 * k, 0, w=6, step=0.03125)       # every point within 0.3 m of every other
    lots = lambda n, k, nd, st=1.0: [B(5, (i % 17) * st + 0.25 * k, -8 + (i // 17) * st, z0=0.25 if i < nd else 1.625) for i in range(n)]
    out = []
    for n in (129, 130):
        out.append(("neighbours_%d" % (n - 1), [_vel_frame([dense(n, k), B(8, 4, 2), G(6)], T(k), shuffle=500 + n + k)
                                                for k in range(2)], 1024))
    for n in (256, 257):
        out.append(("clusters_%d" % n, [_vel_frame(lots(n, k, 6), T(k), shuffle=510 + n + k) for k in range(2)], 2048))
    for n in (64, 65):
        out.append(("dynamic_%d" % n, [_vel_frame(lots(n, k, n, 2.0), T(k), shuffle=520 + n + k) for k in range(2)], 4608))
    for n in (32, 33):          # R * C = 1024 = max_points: the cost matrix just fits; 33 x 33 does not
        out.append(("assoc_%dx%d" % (n, n), [_vel_frame(lots(n, k, n, 2.0), T(k), shuffle=540 + n + k) for k in range(2)], 1024))
    for n in (1024, 1030):
        out.append(("points_%d" % n, [_vel_frame([B(30, 2 + 0.25 * k, 0), B(216, 4, 0, w=6), B(40, 2, 3), G(n - 286)], T(k),
                                                 shuffle=530 + n + k) for k in range(2)], 1024))
    return out


# ---- DSPMap::update branch by branch: the INPUTS of tests/golden/make_dsp_cases_fixture.py and tests/test_dsp_cases_independent.py.
# Hand-built particle stores (injected through the state hook), clouds, poses, cursors and small tables on two tiny grids.  The
# sensor sits at the origin with the identity attitude unless a case says otherwise, so positions are sensor-relative and the
# FOV opens along +x (|y| < x tan 43 deg, |z| < x tan 29 deg): everything at x < 0 is outside it and keeps its weight.  dt = 0.25 s
# and a speed of 0.6 m/s carry a particle exactly one 0.15 m cell.  Nothing here decides anything about the expected output.

DSP_CASE_GRIDS = {"g16": (16, 16, 8, 6), "g24": (24, 24, 8, 6)}
DSP_CASE_T0, DSP_CASE_DT = 10.0, 0.25
_F = np.float32


def dsp_case_tables():
    """4096 position / velocity noise values and 512 rand() values: small, so that every cursor can wrap inside one update"""
    rng = _vel_rng(0xD5B1)
    # position noise in whole 64ths of a metre, |n| <= 12/64: a new-born of a point at a cell centre then lies at (24 + 5 m) / 48 of a
    # cell, never closer than 1/48 of a cell to a cell boundary — no float truncation in voxel_index is ever a close call
    pg = np.asarray([(int(rng.next_u64() % 25) - 12) / 64.0 for _ in range(4096)], np.float32)
    vg = np.asarray([rng.uniform(-0.1, 0.1) for _ in range(4096)], np.float32)
    rnd = np.asarray([rng.next_u64() >> 33 for _ in range(512)], np.int64).astype(np.int32)
    return pg, vg, rnd


def _ulp_below(x):
    return np.nextafter(_F(x), _F(0))


class _DspCase:
    def __init__(self, name, grid, seed=1):
        self.name, self.grid = name, grid
        self.NX, self.NY, self.NZ, self.T = DSP_CASE_GRIDS[grid]
        self.V = self.NX * self.NY * self.NZ
        self.res = _F(0.15)
        self.h = [_F(_F(self.res * _F(n)) * _F(0.5)) for n in (self.NX, self.NY, self.NZ)]
        self.store = np.zeros((self.V, 14, 9), np.float32)
        self.rng = _vel_rng(0xCA5E0000 + seed)
        self.last_pos, self.last_stamp, self.cursors = (0.0, 0.0, 0.0), DSP_CASE_T0, (0, 0, 0)
        self.updates = []
        self.allow = []        # what the generator's margin assertions let this case do on purpose
        self.compare = True    # False: only the counters are held (an over-capacity agent)

    def vox(self, ix, iy, iz):
        return (iz * self.NY + iy) * self.NX + ix

    def centre(self, ix, iy, iz, off=(0.0, 0.0, 0.0)):
        return tuple(float(_F((i + 0.5) * 0.15 - float(h) + o)) for i, h, o in zip((ix, iy, iz), self.h, off))

    def weight(self, lo=0.1, hi=0.5):
        return self.rng.uniform(lo, hi)

    def put(self, v, slot, pos, vel=(0.0, 0.0), w=None, flag=1.0):
        assert self.store[v, slot, 0] == 0, (self.name, v, slot)
        self.store[v, slot] = (flag, vel[0], vel[1], 0.0, pos[0], pos[1], pos[2], self.weight() if w is None else w, 0.0)

    def put_at(self, pos, slot=0, **kw):
        """a particle in the voxel its position lies in"""
        self.put(self.vox(*[int((a + float(h)) / 0.15) for a, h in zip(pos, self.h)]), slot, pos, **kw)

    def fill(self, cell, slots, vel=(0.0, 0.0), spread=0.004, **kw):
        """particles in `cell` at the centre plus a small per-slot offset (told apart by position)"""
        for s in slots:
            self.put(self.vox(*cell), s, self.centre(*cell, off=((s - 6.5) * spread, (s % 3 - 1) * spread, 0.0)), vel, **kw)

    def update(self, points=(), labels=None, pos=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), stamp=None):
        pts = np.asarray(points, np.float32).reshape(-1, 3)
        lab = np.zeros((len(pts), 4), np.float32) if labels is None else np.asarray(labels, np.float32).reshape(-1, 4)
        assert len(lab) == len(pts)
        stamp = DSP_CASE_T0 + DSP_CASE_DT * (len(self.updates) + 1) if stamp is None else stamp
        self.updates.append({"points": pts, "labels": lab, "pos": tuple(pos), "quat": tuple(quat), "stamp": float(stamp)})
        return self


def _dsp_dir(az_deg, el_deg, r):
    """a point at range r whose horizontal / vertical plane angles (atan y/x, atan z/x) are az / el degrees"""
    d = np.array([1.0, np.tan(np.radians(az_deg)), np.tan(np.radians(el_deg))])
    return tuple((d / np.linalg.norm(d) * r).tolist())


FAR = [0.0, 0.0, 0.0, 0.0]                     # label of a static point
DYN = [0.3, 0.1, 0.0, 0.55]                    # a matched cluster's label
UNMATCHED = [-10000.0, -10000.0, -10000.0, 0.55]
X, MX, Y, MY = (0.6, 0.0), (-0.6, 0.0), (0.0, 0.6), (0.0, -0.6)      # one cell per update along +x, -x, +y, -y


def _dsp_search_index_equals_size(h, n):
    """the floats below the upper bound h for which (int)((p + h) / res) == n (the axis size): the largest, or None"""
    res, p = _F(0.15), _ulp_below(h)
    for _ in range(64):
        if int(_F(_F(p + h) / res)) == n:
            return float(p)
        p = _ulp_below(p)
    return None


def _dsp_search_zero_dot(normal, x):
    """a float y with fl(fl(x n0) + fl(y n1)) == 0 exactly (z = 0 term adds +0), near -x n0 / n1; or None"""
    n0, n1 = _F(normal[0]), _F(normal[1])
    y = _F(-float(_F(_F(x) * n0)) / float(n1))
    for cand in [y] + [np.nextafter(y, _F(s)) for s in (-10, 10)]:
        if _F(_F(_F(x) * n0) + _F(cand * n1)) == 0:
            return float(cand)
    return None


# every branch of DSPMap::update that DESIGN section 4 (row a6) lists: each is claimed by a case through the reading's own trace, or the
# fixture lists it as unclaimed with the reason
DSP_CASE_LABELS = """stay_in_fov stay_outside_fov mover_into_unswept_voxel mover_into_swept_voxel
arrivals_before_turn_see_departing_occupants lowest_empty_slot_with_holes arrivals_in_key_order_from_three_sources
fifteen_arrivals_one_phase twenty_eight_arrivals_two_phases leaves_through_each_face leaving_slot_frees_at_own_turn
exactly_on_the_bound one_ulp_below_the_upper_bound_x one_ulp_below_the_upper_bound_y one_ulp_below_the_upper_bound_z
pyramid_full_stay pyramid_full_mover on_a_boundary_plane on_the_fov_edge
cascade_1 cascade_2 cascade_3 cascade_at_the_limit cascade_one_over_the_limit
candidate_pool_exactly_2V candidate_pool_one_over
observations_98_in_one_pyramid observations_99_in_one_pyramid observations_100_in_one_pyramid observations_150_in_one_pyramid
observations_across_trip_boundaries observations_in_shuffled_input_order empty_cloud_reuses_born_list
rejected_quaternion rejected_negative_dt rejected_dt_above_10 rejected_jump_above_10m
occluded_particle_keeps_weight max_length_unset neighbourhood_of_4 neighbourhood_of_6 pdf_clamp_low pdf_clamp_high
ck_over_two_lists split_nan split_all_static split_all_dynamic split_mixed_band split_counts_flag_7 split_passes_over_flag_15
labelled_dynamic unmatched_label low_intensity_zero_velocity random_from_particle_16 newborn_outside_the_map
point_outside_the_map position_table_wraps_inside_one_particle velocity_table_wraps rand_table_wraps
newborn_scan_1024_points newborn_scan_1025_points newborn_scan_2100_points addAParticle_into_13_of_14
more_than_14_newborns_into_an_empty_voxel weight_one_float_below_removal weight_exactly_at_removal
no_resampling_below_5 resampling_5 resampling_7 resampling_8 resampling_14 resample_no_empty_slot_adds_weight
resample_copies_into_slots_freed_in_the_pass flag_0_6_processed_by_next_prediction future_outside_for_some_slices
mean_velocity_excludes_newborns mean_velocity_no_old_particles""".split()

# the seed of a case's generic weights where seed 1 left a resampler comparison closer than the generator's 1e-3 margin
DSP_CASE_SEEDS = {"resampling_counts": 2, "addAParticle_into_13_of_14": 2, "cascade_3": 3, "cascade_at_the_limit": 4,
                  "cascade_one_over_the_limit": 3}


def dsp_case_inputs(seeds=None):
    """{grid: [case, ...]}: every case is one agent of its grid's handle; the branches are DSP_CASE_LABELS"""
    seeds = DSP_CASE_SEEDS if seeds is None else seeds
    cases = []

    def new(name, grid="g16"):
        c = _DspCase(name, grid, seed=seeds.get(name, 1))
        cases.append(c)
        return c

    obs_far = [_dsp_dir(20.5, -10.5, 3.0)]       # one observation inside the FOV and outside both maps: C_k > 0, no new-born

    # ---------------- prediction and placement
    c = new("sweep_basics")
    c.put(c.vox(13, 9, 4), 0, c.centre(13, 9, 4))                    # stays, inside the FOV
    c.put(c.vox(2, 8, 4), 0, c.centre(2, 8, 4))                      # stays, outside
    c.put(c.vox(11, 6, 4), 0, c.centre(11, 6, 4), X)                 # to a higher voxel index
    c.put(c.vox(13, 10, 3), 0, c.centre(13, 10, 3), MX)              # to a lower one
    c.update()

    c = new("arrivals_before_turn_see_departing_occupants")
    c.fill((4, 8, 4), range(14), X)
    c.fill((3, 8, 4), (0, 1), X)
    c.fill((4, 9, 4), (0, 1), MY)
    c.update()

    c = new("lowest_empty_slot_with_holes")
    c.fill((4, 4, 4), (0, 1, 3, 4, 7))
    c.fill((3, 4, 4), (2, 5, 9), X)
    c.update()

    c = new("arrivals_in_key_order_from_three_sources")
    c.fill((4, 7, 4), (2, 9), Y)
    c.fill((3, 8, 4), (0, 5), X)
    c.fill((5, 8, 4), (1, 3), MX)
    c.update()

    c = new("fifteen_arrivals_one_phase")
    c.fill((3, 8, 4), range(14), X)
    c.fill((4, 7, 4), (4,), Y)
    c.update()

    c = new("twenty_eight_arrivals_two_phases")
    c.fill((4, 8, 4), range(7), Y)
    c.fill((3, 8, 4), range(14), X)
    c.fill((5, 8, 4), range(14), MX)
    c.update()

    c = new("leaves_through_each_face")
    c.put(c.vox(15, 14, 4), 0, c.centre(15, 14, 4), X)
    c.put(c.vox(0, 9, 5), 0, c.centre(0, 9, 5), MX)
    c.put(c.vox(3, 15, 4), 0, c.centre(3, 15, 4), Y)
    c.put(c.vox(3, 0, 4), 0, c.centre(3, 0, 4), MY)
    c.put(c.vox(2, 5, 7), 0, c.centre(2, 5, 7))                       # leaves through +z when the sensor sinks one cell
    c.put(c.vox(2, 3, 0), 0, c.centre(2, 3, 0))                       # is at iz = 1 after that and leaves through -z when it climbs two
    c.put(c.vox(2, 9, 4), 0, c.centre(2, 9, 4))                       # stays inside throughout
    c.update(pos=(0.0, 0.0, -0.15))
    c.update(pos=(0.0, 0.0, 0.15))

    c = new("slot_of_a_leaving_particle_frees_at_its_turn")
    c.fill((0, 8, 2), range(14))                                      # a full voxel on the -x face; slot 3 leaves the map
    c.store[c.vox(0, 8, 2), 3, 1] = -0.6
    c.fill((0, 7, 2), (0,), Y)                                        # smaller key: finds the slot still taken
    c.fill((1, 8, 2), (0,), MX)                                       # larger key: finds it free
    c.update()

    c = new("exactly_on_the_bound")
    c.allow.append("searched_truncation")      # (the particle one ulp inside the lower bound: (p + h) / res is a denormal-sized 0+)
    px = c.centre(15, 13, 3)
    c.put(c.vox(15, 13, 3), 0, (float(c.h[0]), px[1], px[2]))
    c.put(c.vox(0, 13, 3), 0, (-float(c.h[0]), px[1], px[2]))
    c.put(c.vox(0, 12, 3), 0, (float(np.nextafter(-c.h[0], _F(0))), c.centre(0, 12, 3)[1], px[2]))     # one ulp inside: stays
    c.update()

    c = new("one_ulp_below_the_upper_bound")
    c.allow.append("searched_truncation")
    c.searched = {}
    for ax, (n, cell) in enumerate(((16, (15, 4, 3)), (16, (3, 15, 3)), (8, (3, 4, 7)))):
        p = _dsp_search_index_equals_size(c.h[ax], n)
        c.searched["xyz"[ax]] = p
        if p is not None:
            pos = list(c.centre(*cell))
            pos[ax] = p
            c.put(c.vox(*cell), 0, tuple(pos))
    c.update()

    c = new("pyramid_full_stay")
    base = np.asarray(c.centre(13, 9, 4))
    for s, k in enumerate((1.0, 1.02, 1.04)):
        c.put(c.vox(13, 9, 4), s, tuple((base * k).tolist()))
    c.update()

    c = new("pyramid_full_mover")
    base = np.asarray(c.centre(13, 7, 4))
    for s, k in enumerate((1.0, 1.02)):
        c.put(c.vox(13, 7, 4), s, tuple((base * k).tolist()))
    land = base * 1.04
    c.put(c.vox(14, 7, 4), 0, (land[0] + 0.15, land[1], land[2]), MX)               # lands in the full pyramid: takes slot 2, vanishes
    c.put(c.vox(13, 8, 4), 0, c.centre(13, 8, 4, off=(0.03, 0.0, 0.03)), MY)       # a later arrival takes slot 2 again
    c.update()

    c = new("on_a_boundary_plane")
    c.allow += ["zero_dot", "exact_cell_boundary"]
    c.put(c.vox(11, 8, 4), 0, (0.525, 0.0, 0.075))        # on y = 0
    c.put(c.vox(11, 8, 4), 1, (0.525, 0.075, 0.0))        # on z = 0
    c.put(c.vox(11, 8, 4), 2, (0.525, 0.0, 0.0))          # on the optical axis
    c.update(points=[(3.0, 0.0, 0.25), (3.0, 0.25, 0.0), (3.0, 0.0, 0.0)])

    c = new("on_the_fov_edge")
    c.allow += ["zero_dot"]
    ang = _F(float(_F(1) / _F(180.0)) * 3.14159265358979323846)
    c.searched = {}
    for sign in (-1, 1):
        nrm = (_F(-np.sin(float(_F(sign * 43) * ang))), _F(np.cos(float(_F(sign * 43) * ang))))
        for x in (0.525, 0.53125, 0.5625, 0.59375, 0.515625):
            y = _dsp_search_zero_dot(nrm, x)
            if y is not None:
                break
        c.searched[sign] = None if y is None else (x, y)
        if y is not None:
            z = 0.075
            ix, iy, iz = int((x + 1.2) / 0.15), int((y + 1.2) / 0.15), int((z + 0.6) / 0.15)
            c.put(c.vox(ix, iy, iz), 0, (x, y, z))                                       # exactly on the edge plane: inside
            c.put(c.vox(ix, iy, iz), 1, (x, float(_F(y) * _F(1.001)), z))                 # just outside it
            c.put(c.vox(ix, iy, iz), 2, (x, float(_F(y) * _F(0.999)), z))                 # just inside it
    c.update(points=obs_far)

    # ---------------- the cascade: a pyramid-full vanish frees the only slot of a full voxel, the arrival that takes it fills the
    # next pyramid, whose later particle vanishes ...  The voxels (14, iy, 7) straddle the upper edge of the FOV: their 12-13
    # fillers sit above it (z > x tan 29 deg: never listed), the chain's particles below it, all in the 26-27 deg row of pyramids.
    # Link k's pyramid crosses the face between voxel iy and iy + 1 (y < 0): its near point (x = 0.95) lies in the upper voxel, the
    # same direction at x = 1.04 in the lower one.
    def cascade(c, depth):
        xn, xf = 0.95, 1.04
        near = lambda y: np.array([xn, y, xn * np.tan(np.radians(26.5))])
        for k in range(1, depth + 1):
            iy = 1 + k
            lower = -1.2 + 0.15 * iy
            v, taken = c.vox(14, iy, 7), {13}
            x_k = near(-0.80) if k == 1 else near(0.96 * lower)
            c.put(v, 13, tuple(x_k.tolist()))                                     # X_k: the last slot, vanishes at depth k
            if k == 1:
                for s, f in ((0, 1.005), (1, 1.01)):                               # the two entries that fill pyramid 1 before X_1
                    c.put(v, s, tuple((x_k * f).tolist()))
                    taken.add(s)
            if k < depth:
                far = near(0.96 * (lower + 0.15)) * (xf / xn)                      # the direction of X_k+1, inside this voxel
                s = 2 if k == 1 else 0
                c.put(v, s, tuple((far * 0.995).tolist()))                          # L_k+1: the first entry of pyramid k + 1
                taken.add(s)
                c.put(c.vox(15, iy, 7), 0, (far[0] + 0.15, far[1], far[2]), MX)    # Y_k: arrives after X_k's turn, second entry
            for s in range(14):
                if s not in taken:
                    c.put(v, s, (0.91, c.centre(14, iy, 7)[1] + (s - 6.5) * 0.008, 0.59))
    for depth, name in ((1, "cascade_1"), (2, "cascade_2"), (3, "cascade_3"), (5, "cascade_at_the_limit"), (6, "cascade_one_over_the_limit")):
        c = new(name)
        cascade(c, depth)
        c.compare = depth <= 5       # DSP_ROUNDS = 6 place / pyramid rounds settle a chain of 5 (round r finds the vanish of depth r + 1, the
        c.update()                   # sixth round confirms that nothing changed); a chain of 6 raises counters[10] and is not compared

    # ---------------- the candidate pool: cand_cap = 2 V
    for extra in (0, 1):
        c = new("candidate_pool_2V" if not extra else "candidate_pool_2V_plus_1")
        wts = [0.125, 0.1875, 0.25, 0.3125, 0.375, 0.4375, 0.28125, 0.21875]
        for iz in range(c.NZ):
            for iy in range(c.NY):
                for ix in range(c.NX):
                    for s in range(2):
                        o = 0.03 if s else -0.03
                        c.put(c.vox(ix, iy, iz), s, c.centre(ix, iy, iz, off=(0.0, o, o)), MX if ix % 2 else X,
                              w=wts[(ix + 3 * iy + 5 * iz + 4 * s) % 8])      # neighbours differ; periodic, so the fixture stays small
        if extra:
            c.put(c.vox(2, 3, 4), 2, c.centre(2, 3, 4), X, w=0.25)
            c.compare = False
        c.update()
    c = new("neighbour_of_the_over_full_pool")
    c.fill((4, 8, 4), range(3), X)
    c.fill((12, 8, 4), range(3))
    c.update(points=obs_far)

    # ---------------- observation binning (g24; the points lie outside the map: no new-born particles)
    for n in (98, 99, 100, 150):
        c = new("observations_%d_in_one_pyramid" % n, "g24")
        c.put_at(_dsp_dir(10.5, 5.5, 0.6))
        c.put_at(_dsp_dir(-30.5, -10.5, 0.6))
        # past the cap the LAST point is the longest: max_length comes from all points, the dropped ones included
        c.update(points=[_dsp_dir(10.5, 5.5, 4.0 if n > 99 and k == n - 1 else 2.5 + 0.01 * ((k * 37) % n)) for k in range(n)] +
                 [_dsp_dir(-30.5, -10.5, 2.75)])

    def trip_cloud():
        pts = [_dsp_dir(-40.5 + (k % 82), -25.5 + (k // 82), 3.0) for k in range(600)]
        for j, k in enumerate((255, 256, 257, 511, 512)):
            pts[k] = _dsp_dir(12.5, 26.5, 3.0 + 0.125 * (5 - j))      # one pyramid (above the filler's rows), decreasing length
        return pts
    c = new("observations_across_trip_boundaries", "g24")
    c.put_at(_dsp_dir(12.5, 26.5, 0.5))
    c.update(points=trip_cloud())
    c = new("observations_in_shuffled_input_order", "g24")
    c.put_at(_dsp_dir(12.5, 26.5, 0.5))
    pts = trip_cloud()
    c.update(points=[pts[i] for i in _vel_shuffle(77, len(pts))])

    c = new("empty_cloud_after_a_cloud", "g24")
    c.fill((4, 8, 4), (0, 1))
    pts = [c.centre(5, 5, 3), c.centre(8, 17, 5), c.centre(3, 12, 2)] + obs_far
    c.update(points=pts, labels=[FAR, DYN, UNMATCHED, FAR])
    c.update()

    for name, kw in (("rejected_quaternion", {"quat": (1.002, 0.0, 0.0, 0.0)}), ("rejected_negative_dt", {"stamp": 9.5}),
                     ("rejected_dt_above_10", {"stamp": 20.5}), ("rejected_jump_above_10m", {"pos": (10.5, 0.0, 0.0)})):
        c = new(name, "g24")
        c.fill((4, 8, 4), range(6), X)
        c.fill((16, 13, 4), (0, 2))
        c.store[c.vox(16, 13, 4), 2, 0] = 0.6
        c.update(points=obs_far, **kw)
        c.update(points=obs_far, stamp=10.5)

    # ---------------- mapUpdate
    c = new("occluded_particle_keeps_weight", "g24")
    c.put_at(_dsp_dir(10.5, 5.5, 1.5))
    c.update(points=[_dsp_dir(10.5, 5.5, 0.9)])

    c = new("neighbourhood_of_4_and_6")
    for az, el in ((-42.5, 28.5), (-42.5, 0.5), (10.5, 5.5)):
        c.put_at(_dsp_dir(az, el, 0.8))
    c.update(points=[_dsp_dir(-42.5, 28.5, 3.0), _dsp_dir(-42.5, 0.5, 3.0), _dsp_dir(10.5, 5.5, 3.0)])

    c = new("pdf_clamp_and_ck_over_two_lists")
    for k, (az, el) in enumerate(((10.5, 5.5), (11.5, 5.5), (-30.5, -10.5))):
        c.put_at(_dsp_dir(az, el, 0.8), slot=k)
    # an observation 0.02 m behind the first particle (inside the map: it also breeds), and far ones on both sides of the clamp
    c.update(points=[_dsp_dir(10.5, 5.5, 0.82), _dsp_dir(10.5, 5.5, 3.0), _dsp_dir(-30.5, -10.5, 3.0)])

    # ---------------- new-born (behind the sensor: the old particles there keep their weights)
    c = new("dempster_shafer_split")
    cells = [(2, 3, 2), (2, 6, 2), (2, 9, 2), (2, 12, 2), (5, 3, 5), (5, 7, 5)]
    c.put(c.vox(*cells[1]), 0, c.centre(*cells[1]))                                           # all static
    c.put(c.vox(*cells[1]), 1, c.centre(*cells[1], off=(0.01, 0.0, 0.0)))
    c.put(c.vox(*cells[2]), 0, c.centre(*cells[2], off=(-0.04, -0.04, 0.0)), (0.3, 0.3))      # all dynamic: |v|_1 = 0.6
    c.put(c.vox(*cells[3]), 0, c.centre(*cells[3], off=(-0.02, 0.0, 0.0)), (0.2, 0.0))        # the mixed band ...
    c.put(c.vox(*cells[3]), 1, c.centre(*cells[3]))                                           # ... beside a static one
    c.put(c.vox(cells[4][0] - 1, cells[4][1], cells[4][2]), 0, c.centre(cells[4][0] - 1, cells[4][1], cells[4][2]), X)   # arrives: flag 7
    pts = [c.centre(*cl) for cl in cells[:5]] + [c.centre(*cells[5], off=(0.0002 * k, 0.0, 0.0)) for k in range(3)] + obs_far
    c.update(points=pts, labels=[FAR, DYN, DYN, DYN, DYN] + [FAR, DYN, DYN] + [FAR])      # (cell 5: the first point breeds static new-borns, flag 15, that the next two pass over)

    c = new("class_branches")
    pts = [c.centre(3, 4, 3), c.centre(3, 8, 3), c.centre(3, 12, 3), c.centre(6, 4, 5)] + obs_far
    c.update(points=pts, labels=[DYN, UNMATCHED, [0.3, 0.1, 0.0, 0.005], [-10000.0, 0.0, 0.0, 0.005], FAR])

    c = new("newborn_and_point_outside_the_map")
    c.update(points=[(-1.125, 0.075, 0.075), (-1.5, 0.075, 0.075), (0.075, -1.125, -0.525)] + obs_far, labels=[DYN, DYN, UNMATCHED, FAR])

    c = new("table_cursors_wrap")
    c.cursors = (4096 - 4, 4096 - 2, 512 - 2)
    c.update(points=[c.centre(3, 4, 3), c.centre(3, 8, 3)] + obs_far, labels=[DYN, UNMATCHED, FAR])

    for n in (1024, 1025, 2100):
        c = new("newborn_scan_%d_points" % n, "g24")
        c.cursors = (4000, 4090, 500)
        # Every point breeds (one observation inside the FOV gives the new-born weight 1e-4 / 0.012; nothing is listed, so every weight
        # is plain float arithmetic).  Most points pile into one cell, whose neighbourhood fills from the first of them: every lane of
        # the scan carries draws, few particles survive.  The points at the scan's lane, wave, chunk and trip boundaries have a cell
        # of their own (three cells apart), so their new-borns survive, and carry the table offsets of everything before them.
        own = [k for k in (0, 1, 63, 64, 65, 127, 128, 255, 256, 511, 512, 513, 767, 768, 1023, 1024, 1535, 1536, 2047, 2048, n - 2, n - 1)
               if k < n]
        cells = [(ix, iy, iz) for iz in (2, 5) for iy in range(0, 24, 3) for ix in (1, 4, 7)]      # (iy = 0: some new-borns leave the map)
        spot = {k: cells[(7 * i) % len(cells)] for i, k in enumerate(sorted(set(own)))}
        pts = [c.centre(*spot.get(k, (10, 12, 4))) for k in range(n)]
        pts[2] = obs_far[0]      # the observation is point 2 of the n: outside the map, it breeds nothing and has no rank
        c.update(points=pts, labels=[FAR if k == 2 else (DYN, UNMATCHED, FAR)[k % 3] for k in range(n)])

    c = new("addAParticle_into_13_of_14")
    c.fill((3, 8, 3), [s for s in range(14) if s != 9])
    pg = dsp_case_tables()[0]      # a cursor at which the first two new-borns (six draws) stay within the point's own cell
    c.cursors = (next(k for k in range(4000) if np.all(np.abs(pg[k:k + 6]) <= 4.0 / 64.0)), 0, 0)
    c.update(points=[c.centre(3, 8, 3, off=(0.0002 * k, 0.0, 0.0)) for k in range(3)] + obs_far, labels=[DYN] * 3 + [FAR])

    # ---------------- occupancy and resample (behind the sensor, no cloud: injected weights only)
    c = new("weight_removal_edge")
    c.put(c.vox(3, 8, 3), 0, c.centre(3, 8, 3), w=float(_F(0.001)))
    c.put(c.vox(3, 8, 3), 1, c.centre(3, 8, 3, off=(0.01, 0.0, 0.0)), w=float(_ulp_below(0.001)))
    c.update()

    c = new("resampling_counts")
    for k, n in enumerate((4, 5, 7, 8, 14)):
        c.fill((2 + k, 5, 3), range(n))
    c.update()

    c = new("resample_no_empty_slot_adds_weight")
    c.fill((3, 8, 3), (0,), w=10.0)
    c.fill((3, 8, 3), range(1, 14), w=0.01)
    c.update()

    c = new("resample_copies_and_flag_0_6")
    c.fill((3, 8, 3), range(6), w=0.01)
    c.fill((3, 8, 3), (6,), w=3.0)
    c.fill((3, 8, 3), range(7, 14), w=0.0125)
    c.update()
    c.update()

    c = new("future_status_outside_for_some_slices")
    c.put(c.vox(1, 8, 3), 0, (-1.0, 0.075, -0.075), (-0.3, 0.0))
    c.put(c.vox(3, 1, 3), 0, (-0.7, -1.02, -0.075), (0.0, -0.2))
    c.update()

    out = {g: [c for c in cases if c.grid == g] for g in DSP_CASE_GRIDS}
    return out


def dsp_case_sha256(case):
    """what the fixture records of a case's inputs"""
    import hashlib
    h = hashlib.sha256()
    h.update(case.store.tobytes())
    h.update(np.asarray(case.last_pos + (case.last_stamp,) + tuple(case.cursors), np.float64).tobytes())
    for u in case.updates:
        h.update(u["points"].tobytes() + u["labels"].tobytes())
        h.update(np.asarray(u["pos"] + u["quat"] + (u["stamp"],), np.float64).tobytes())
    return h.hexdigest()
