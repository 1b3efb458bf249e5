"""Fixtures of the ring tests (CPU and GPU): records, cameras, rays and poses.  Records are (n, 12) float64 rows
{type, x, y, z, w, h, vx, vy, qw, qx, qy, qz}.  Test infrastructure; not collected by pytest."""
import math
import types

import numpy as np

CAM2BODY = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
Q_TILT = (0.82, 0.21, -0.33, 0.41)
S45 = math.sqrt(0.5)
Q_UPRIGHT = (S45, S45, 0.0, 0.0)      # n = (0, -1, 0), e1 = (1, 0, 0), e2 = (0, 0, 1): the ring stands in the x-z plane


def ring(x, y, z, w, h=0.1, q=(1.0, 0.0, 0.0, 0.0), vx=0.0, vy=0.0, typ=2):
    return [typ, x, y, z, w, h, vx, vy, *q]


def cylinder(x, y, w, z=2.0, h=4.0, vx=0.0, vy=0.0):
    return [3, x, y, z, w, h, vx, vy, 1.0, 0.0, 0.0, 0.0]


def to_struct(abi, rows12):
    rows12 = np.asarray(rows12, np.float64).reshape(-1, 12)
    arr = (abi.SogmCylinder * max(len(rows12), 1))()
    for i, r in enumerate(rows12):
        o = arr[i]
        o.type = int(r[0])
        o.x, o.y, o.z, o.w, o.h, o.vx, o.vy, o.qw, o.qx, o.qy, o.qz = [float(v) for v in r[1:]]
    return arr


def cam(rows, cols, fx, cx, cy, use_ground=True, max_depth=5.0, ground_z=0.0):
    return types.SimpleNamespace(fx=fx, fy=fx, cx=cx, cy=cy, max_depth=max_depth, depth_scale=1000.0, ground_z=ground_z,
                                 rows=rows, cols=cols, use_ground=1 if use_ground else 0)


def quat_matrix(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def pose(x, y, z, yaw, pitch=None):
    """scene.camera_pose: yaw = 0 gives the exact matrix [[0,0,1],[-1,0,0],[0,-1,0]] (d = (1, -xc, -yc)); pitch > 0 turns the
    nose down"""
    c, s = math.cos(yaw), math.sin(yaw)
    body = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    if pitch is not None:
        cp, sp = math.cos(pitch), math.sin(pitch)
        body = body @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    return np.array([x, y, z], np.float64), body @ CAM2BODY


def branch_scene(rows=48, cols=64):
    """Every branch of the ray rule in one world, four cameras.  cy is a whole number: the middle row has yc == 0, and with
    camera 0's exact matrix nd == 0 exactly against the two horizontal rings 2 (|no| = 0.05 <= rho) and 3 (|no| = 0.3 > rho)."""
    rec = [
        ring(3.0, 0.3, 1.2, 1.6, q=Q_TILT),                 # 0 tilted, general position; camera 2 sits in its hole
        ring(2.5, 0.02, 1.0, 1.4, q=Q_UPRIGHT),             # 1 upright, camera 0 0.02 m off its plane (nd small); camera 3 in its tube
        ring(2.0, 1.0, 1.05, 1.0),                          # 2 horizontal, 0.05 above camera 0: nd == 0 inside the slab
        ring(2.2, -0.4, 1.3, 0.8),                          # 3 horizontal, 0.3 above camera 0: nd == 0 outside the slab
        ring(1.5, -2.2, 0.35, 1.2),                         # 4 horizontal and low: seen from above by camera 1 (steep slab)
        ring(-3.0, 0.2, 1.0, 1.6, q=Q_TILT),                # 5 wholly behind camera 0
        ring(9.0, 0.0, 1.0, 1.6, q=Q_UPRIGHT),              # 6 beyond max_depth
        cylinder(3.6, 0.5, 0.5),                            # 7 behind ring 0, in front of ring 8
        ring(4.3, 0.6, 1.1, 1.8, q=(0.7, 0.1, 0.7, 0.1)),   # 8 behind the cylinder
        ring(2.8, 1.9, 0.5, 1.6, q=Q_UPRIGHT),              # 9 upright, reaches 0.4 below the ground plane
        ring(2.0, 0.0, 1.0, 0.15),                          # 10 not a ring: rho >= R
        ring(2.0, 0.0, 1.0, 1.0, q=(0.0, 0.0, 0.0, 0.0)),   # 11 not a ring: zero quaternion
        ring(2.0, 0.0, 1.0, 1.0, typ=7),                    # 12 another type
        cylinder(1.0, 2.5, 0.6, z=0.6, h=1.2),              # 13 a stump
    ]
    poses = [pose(0.0, 0.0, 1.0, 0.0),
             pose(1.0, -2.0, 1.6, -0.4, pitch=1.1),                                    # looks down at ring 4
             pose(3.0, 0.3, 1.2, 2.0),
             pose(2.5 + 0.7, 0.02, 1.0, -2.5)]
    c = cam(rows, cols, 40.0 * cols / 64.0, 31.3 * cols / 64.0, float(rows // 2))
    return (np.array(rec, np.float64), c, np.stack([p for p, _ in poses]), np.stack([R.reshape(9) for _, R in poses]))


class _Rng:
    """SplitMix64 (scene.SplitMix64 restated: the fixtures do not depend on the package)"""

    def __init__(self, seed):
        self.s = seed & 0xFFFFFFFFFFFFFFFF

    def uniform(self, lo=0.0, hi=1.0):
        self.s = (self.s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 31
        return lo + (hi - lo) * ((z >> 11) / float(1 << 53))


def crowd_scene(split=False):
    """300 small rings and 10 cylinders, all within range of one 16 x 16 camera: more ring candidates than the 256-entry
    list.  split: 150 rings, the cylinders, 150 rings."""
    rng = _Rng(0xB1)
    rings = []
    for _ in range(300):
        rho, ang = rng.uniform(0.8, 4.4), rng.uniform(-0.6, 0.6)
        q = [rng.uniform(-1, 1) for _ in range(4)]
        rings.append(ring(rho * math.cos(ang), rho * math.sin(ang), rng.uniform(0.3, 1.8), rng.uniform(0.3, 0.8),
                          h=rng.uniform(0.03, 0.06), q=q))
    cyls = [cylinder(rng.uniform(1.0, 4.5), rng.uniform(-2.0, 2.0), rng.uniform(0.1, 0.3)) for _ in range(10)]
    rec = rings[:150] + cyls + rings[150:] if split else rings + cyls
    p, R = pose(0.0, 0.0, 1.0, 0.05)
    return np.array(rec, np.float64), cam(16, 16, 10.0, 7.4, 7.7), p[None], R.reshape(1, 9)


def accuracy_views():
    """six views of one ring at 60 x 80 (the ring 1.5 .. 4 m away), for the comparison with exact quartic roots"""
    rng = _Rng(0xACC)
    out = []
    for _ in range(6):
        q = [rng.uniform(-1, 1) for _ in range(4)]
        dist, ang, dz = rng.uniform(1.5, 4.0), rng.uniform(-0.3, 0.3), rng.uniform(-0.4, 0.4)
        rec = np.array([ring(dist * math.cos(ang), dist * math.sin(ang), 1.0 + dz, rng.uniform(1.0, 2.0), q=q)])
        p, R = pose(0.0, 0.0, 1.0, rng.uniform(-0.2, 0.2))
        out.append((rec, cam(60, 80, 48.0, 39.3, 29.6, use_ground=False, max_depth=8.0), p, R.reshape(9)))
    return out


def audit_poses(n=300):
    """(record row, body centres [n, 3]) per ring: poses within 0.3 m (sigma) of the circle of a ring with R in [0.5, 1]"""
    rng = _Rng(0xA0D)
    out = []
    for k in range(3):
        q = [rng.uniform(-1, 1) for _ in range(4)]
        row = np.array(ring(rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.8, 1.6), 2.0 * rng.uniform(0.5, 1.0), q=q))
        M = quat_matrix(q)
        a = np.zeros((n // 3, 3))
        for i in range(len(a)):
            th = rng.uniform(0.0, 2.0 * math.pi)
            gauss = [math.sqrt(-2.0 * math.log(max(rng.uniform(), 1e-300))) * math.cos(2.0 * math.pi * rng.uniform())
                     for _ in range(3)]
            a[i] = row[1:4] + 0.5 * row[4] * (math.cos(th) * M[:, 0] + math.sin(th) * M[:, 1]) + 0.3 * np.array(gauss)
        out.append((row, a))
    return out
