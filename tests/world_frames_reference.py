"""Second reading of include/sogm_abi.h "world timeline", written from the header text alone (numpy, no code shared with
csrc/sogm_world.hpp): one frame of the moving world from the tick-0 world.

    frame(cloud0, owner, rows, dt, moving, k, block_points) -> (cloud, bounds, rows)

cloud0 float32 [n, 3], owner int32 [n], rows float64 (n_cyl, 11) = the record's doubles {x, y, z, w, h, vx, vy, qw, qx, qy,
qz} (type and _pad are "every other field": they are copied, records_bytes() puts them back).  numpy evaluates every
operator on its own, so nothing here is contracted."""
import numpy as np

X, Y, VX, VY = 0, 1, 5, 6


def frame(cloud0, owner, rows, dt, moving, k, block_points=256):
    cloud0 = np.ascontiguousarray(cloud0, np.float32).reshape(-1, 3)
    owner = np.asarray(owner, np.int64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(-1, 11)
    n_cyl = len(rows)
    t = np.float64(k) * np.float64(dt)
    if k == 0 or not moving:           # copied bit for bit
        cloud, out_rows = cloud0.copy(), rows.copy()
    else:
        out_rows = rows.copy()
        out_rows[:, X] = rows[:, X] + rows[:, VX] * t
        out_rows[:, Y] = rows[:, Y] + rows[:, VY] * t
        cloud = cloud0.copy()
        owned = np.nonzero((owner >= 0) & (owner < n_cyl))[0]   # every other point is copied; its owner indexes nothing
        c = owner[owned]
        offx = (rows[c, VX] * t).astype(np.float32)              # fp64 product, rounded once
        offy = (rows[c, VY] * t).astype(np.float32)
        cloud[owned, 0] = cloud0[owned, 0] + offx                # fp32 adds, also when the offset is zero
        cloud[owned, 1] = cloud0[owned, 1] + offy
    assert cloud.dtype == np.float32
    return cloud, block_bounds(cloud, block_points), out_rows


def _lowest(v):
    """min of float32 values as fminf folds them: a NaN is passed over, -0 orders below +0, nothing at all gives +inf"""
    v = v[~np.isnan(v)]
    if not len(v):
        return np.float32(np.inf)
    m = v.min()
    if m == 0:
        return np.float32(-0.0) if np.signbit(v[v == 0]).any() else np.float32(0.0)
    return m


def _highest(v):
    return -_lowest(-v)


def block_bounds(cloud, block_points):
    """{xmin, xmax, ymin, ymax} of every block of block_points consecutive points, the tail block included"""
    n = len(cloud)
    nb = -(-n // block_points)
    out = np.zeros((nb, 4), np.float32)
    for b in range(nb):
        blk = cloud[b * block_points:min((b + 1) * block_points, n)]
        out[b] = (_lowest(blk[:, 0]), _highest(blk[:, 0]), _lowest(blk[:, 1]), _highest(blk[:, 1]))
    return out


def records_bytes(rows, types=None, pads=None):
    """(n, 11) rows -> the n 96-byte records {int32 type, int32 _pad, 11 doubles} as uint8 [n * 96]"""
    rows = np.asarray(rows, np.float64).reshape(-1, 11)
    rec = np.zeros((len(rows),), dtype=[("type", "<i4"), ("pad", "<i4"), ("d", "<f8", (11,))])
    rec["type"] = 3 if types is None else types
    rec["pad"] = 0 if pads is None else pads
    rec["d"] = rows
    return rec.view(np.uint8).reshape(-1).copy()


def cylinder_rows(cyl5):
    """scene rows {x, y, w, vx, vy} -> record rows as scene.cylinders_to_struct fills them (z 2, h 4, identity quaternion)"""
    cyl5 = np.asarray(cyl5, np.float64).reshape(-1, 5)
    rows = np.zeros((len(cyl5), 11), np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4] = cyl5[:, 0], cyl5[:, 1], 2.0, cyl5[:, 2], 4.0
    rows[:, 5], rows[:, 6], rows[:, 7] = cyl5[:, 3], cyl5[:, 4], 1.0
    return rows
