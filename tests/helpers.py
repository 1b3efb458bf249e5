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
