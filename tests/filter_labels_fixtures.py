"""Hand-built clouds and hit codes for the labelled voxel filter (include/sogm_abi.h "ground-truth labels"): three agents, a
few hundred points each, every case a leaf of its own with a name.  No camera.

Leaves are 0.15 m; a point is written as (leaf index + fraction) * 0.15 with fractions in [0.1, 0.9], far from the leaf's
faces, so that floorf(p * inv_leaf) is the index on any implementation.  Camera frame: x right, y down, z forward; the map
keeps a centroid with |z| < 4.95, |x| < 4.95, |y| < 1.5.  Lane i & 63 of the accumulate kernel takes point i of an agent: runs
are placed by their index in the agent's cloud."""
import numpy as np

LEAF = 0.15
HIT_GROUND, HIT_NONE = -1, -2
# sources: three records (the last of type 2, a ring) and three bodies; codes 0..2 records, 3..5 bodies
REC = np.array([[3, 1.0, 0.0, 2.0, 0.5, 4.0, 0.7, -0.2, 1.0, 0.0, 0.0, 0.0],
                [3, 2.0, 1.0, 2.0, 0.5, 4.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0],          # a static record: no label
                [2, 0.0, 2.0, 1.0, 1.6, 0.1, -0.31, 0.45, 1.0, 0.0, 0.0, 0.0]])       # type 2: its vx, vy count alike
BODY_VEL = np.array([[0.5, 0.1, -0.2], [0.0, 0.0, 0.0], [1e-3, 0.0, 0.0]])             # the last below MIN_SPEED
MIN_SPEED = 0.05
N_CYL = len(REC)
CODE_BEYOND = N_CYL + len(BODY_VEL)


class Cloud:
    """points and codes in order, and per named case the leaf (ix, iy, iz) and the code that must win it"""

    def __init__(self):
        self.xyz, self.code, self.cases = [], [], {}

    def __len__(self):
        return len(self.code)

    def add(self, leaf, frac, code):
        self.xyz.append([np.float32((leaf[k] + frac[k]) * LEAF) for k in range(3)])
        self.code.append(code)

    def add_raw(self, xyz, code):
        self.xyz.append([np.float32(v) for v in xyz])
        self.code.append(code)

    def pad_to_lane(self, lane):
        """points that are not finite, each with a body's code, until the next point is taken by `lane`"""
        while len(self) % 64 != lane:
            self.add_raw([np.nan, 0.05, 0.3], 3)

    def name(self, case, leaf, winner):
        assert case not in self.cases and leaf not in [c[0] for c in self.cases.values()], case
        self.cases[case] = (leaf, winner)

    def arrays(self):
        return np.array(self.xyz, np.float32).reshape(-1, 3), np.array(self.code, np.int32)


def _run(c, leaf, n, winner_at, code_win, code_rest):
    """n consecutive points in one leaf; the point `winner_at` of the run is in front of all others (z fraction 0.15, the
    others' 0.5 .. 0.8)"""
    for k in range(n):
        fz = 0.5 + 0.3 * ((k * 7) % 11) / 11.0
        if k == winner_at:
            c.add(leaf, (0.2 + 0.6 * (k % 5) / 5.0, 0.5, 0.15), code_win)
        else:
            c.add(leaf, (0.2 + 0.6 * (k % 5) / 5.0, 0.5, fz), code_rest)


def agent0():
    c = Cloud()
    c.add((0, 13, 4), (0.5, 0.5, 0.5), 0)                       # camera y = 2.0: body z = -2.0, outside the map
    c.add((0, 13, 4), (0.4, 0.5, 0.5), 0)
    c.name("a leaf dropped by isInRange", (0, 13, 4), 0)
    c.add((0, 0, 10), (0.5, 0.5, 0.5), 0)
    c.name("a leaf with one point", (0, 0, 10), 0)
    c.add((3, 0, 10), (0.5, 0.5, 0.6), 3)
    c.add((3, 0, 10), (0.3, 0.4, 0.4), 2)
    c.add((3, 0, 10), (0.7, 0.4, 0.8), 5)
    c.name("two codes, z decides", (3, 0, 10), 2)
    for code in (1, 4, HIT_GROUND, 4, 0):
        c.add((6, 0, 10), (0.2 + (0.1 * len(c)) % 0.6, 0.5, 0.5), code)
    c.name("equal z, the larger code wins", (6, 0, 10), 4)
    # a NaN point that would win the one-point leaf (smaller z, larger code) if it were not skipped; one per coordinate
    c.add_raw([np.nan, 0.5 * LEAF, 10.1 * LEAF], 5)
    c.add_raw([0.5 * LEAF, np.inf, 10.1 * LEAF], 5)
    c.add_raw([0.5 * LEAF, 0.5 * LEAF, -np.inf], 5)
    c.pad_to_lane(0)
    _run(c, (9, 0, 10), 160, 0, 3, 0)
    c.name("a run of 160 from lane 0, the winner at its first lane", (9, 0, 10), 3)
    _run(c, (12, 0, 10), 160, 31, 2, 4)                           # from lane 32: lane 63 is the run's point 31
    c.name("a run of 160 from lane 32, the winner at the first wave's last lane", (12, 0, 10), 2)
    c.pad_to_lane(0)
    _run(c, (15, 0, 10), 150, 100, 0, 5)
    c.name("a run of 150 from lane 0, the winner in the following wave", (15, 0, 10), 0)
    _run(c, (18, 0, 10), 70, 69, 3, 2)                            # starts mid-wave, ends in the next
    c.name("a run of 70 across two waves, the winner its last point", (18, 0, 10), 3)
    for k in range(5):
        c.add((0, 3, 12), (0.3, 0.5, 0.5 + 0.05 * k), 1)
    for k in range(4):
        c.add((3, 3, 12), (0.3, 0.5, 0.5), HIT_GROUND)
    c.add((0, 3, 12), (0.6, 0.5, 0.3), 3)
    c.add((0, 3, 12), (0.6, 0.5, 0.7), 5)
    c.name("A B A: the same leaf fed by two runs, the winner in the second", (0, 3, 12), 3)
    c.name("A B A: the leaf between", (3, 3, 12), HIT_GROUND)
    for k in range(3):
        c.add((6, 3, 12), (0.3 + 0.1 * k, 0.5, 0.5), HIT_NONE)
    c.name("finite points with SOGM_HIT_NONE only", (6, 3, 12), HIT_NONE)
    c.add((9, 3, 12), (0.3, 0.5, 0.5), HIT_NONE)
    c.add((9, 3, 12), (0.5, 0.5, 0.5), HIT_GROUND)
    c.name("SOGM_HIT_NONE and the ground at equal z", (9, 3, 12), HIT_GROUND)
    c.add((12, 3, 12), (0.5, 0.5, 0.5), CODE_BEYOND)
    c.name("a code at n_cyl + n_bodies", (12, 3, 12), CODE_BEYOND)
    c.add((15, 3, 12), (0.5, 0.5, 0.5), 2 ** 31 - 1)
    c.add((15, 3, 12), (0.5, 0.5, 0.2), -7)
    c.name("codes out of range on both sides, z decides", (15, 3, 12), -7)
    c.add((18, 3, 12), (0.5, 0.5, 0.5), 2)
    c.name("a type-2 record's velocity", (18, 3, 12), 2)
    c.add((21, 3, 12), (0.5, 0.5, 0.5), 4)
    c.add((24, 3, 12), (0.5, 0.5, 0.5), 5)
    c.add((27, 3, 12), (0.5, 0.5, 0.5), 1)
    c.name("a body at rest", (21, 3, 12), 4)
    c.name("a body slower than min_speed", (24, 3, 12), 5)
    c.name("a record at rest", (27, 3, 12), 1)
    # the leaf round z = 0: -0 comes before +0, whatever the codes
    c.add_raw([0.05, 0.05, 0.0], 5)
    c.add_raw([0.06, 0.05, -0.0], HIT_GROUND)
    c.add_raw([0.07, 0.05, 0.0], 3)
    c.name("-0 before +0", (0, 0, 0), HIT_GROUND)
    assert len(c) % 64 != 0
    return c


def agent2(seed=0x1ABE1, n=403):
    """a random cloud: ~170 leaves, z quantised to 1/64 m so that ties between codes happen, a few NaNs"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.3, 0.3, n), np.round(rng.uniform(0.5, 1.4, n) * 64) / 64], axis=1)
    xyz = xyz[np.argsort((xyz[:, 1] * 7).astype(int), kind="stable")].astype(np.float32)     # rows of a picture, roughly
    code = rng.integers(-2, CODE_BEYOND + 2, n).astype(np.int32)
    xyz[::41] = np.nan
    assert n % 64 != 0
    return xyz, code


def clouds():
    """(raw [n, 3], code [n], raw_range [3, 2], per-agent (xyz, code), agent 0's named cases); agent 1 is empty"""
    c0 = agent0()
    a0, a2 = c0.arrays(), agent2()
    empty = (np.zeros((0, 3), np.float32), np.zeros((0,), np.int32))
    per = [a0, empty, a2]
    ends = np.cumsum([len(p[1]) for p in per])
    rng = np.stack([np.concatenate([[0], ends[:-1]]), ends], axis=1).astype(np.int32)
    return (np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per]), rng, per, c0.cases)


def other_codes(code, seed=0x0DD):
    """different codes for the same points: the third call of the labelled / plain / labelled sequence"""
    rng = np.random.default_rng(seed)
    return rng.integers(-2, CODE_BEYOND + 1, len(code)).astype(np.int32)


def leaf_of_output(points):
    """the camera-frame leaf (ix, iy, iz) of body-frame output points (x = z, y = -x, z = -y undone)"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    cam = np.stack([-p[:, 1], -p[:, 2], p[:, 0]], axis=1)
    return [tuple(int(v) for v in r) for r in np.floor(cam * (np.float32(1.0) / np.float32(LEAF))).astype(np.int64)]
