"""The depth camera of include/sogm_abi.h ("depth camera") restated in numpy, vectorised over the pixels of one image
and written from the header's text alone: every expression below is the header's, in its order, in fp64 (numpy does not
contract a*b + c).  No culling, no early exits: each cylinder is tried against every pixel.  Test infrastructure."""
import numpy as np


def records(cyl):
    """(n, 5) rows {x, y, w, vx, vy} (scene / WorldTimeline: type 3, z 2, h 4, as scene.cylinders_to_struct makes them) or a
    ctypes SogmCylinder array -> (n, 6) float64 rows {type, x, y, z, w, h}"""
    if isinstance(cyl, np.ndarray) or isinstance(cyl, (list, tuple)):
        c = np.asarray(cyl, np.float64).reshape(-1, 5)
        out = np.empty((len(c), 6))
        out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5] = 3, c[:, 0], c[:, 1], 2.0, c[:, 2], 4.0
        return out
    return np.array([[o.type, o.x, o.y, o.z, o.w, o.h] for o in cyl], np.float64).reshape(-1, 6)


def in_range(rec, cam, pos):
    """the type-3 records that can be seen at all: xy distance from the camera to the axis, minus r, is at most
    max_depth * sqrt(1 + xc_max^2 + yc_max^2) (how far a point with camera z <= max_depth can be); every other type is
    kept (it is counted)"""
    rec = np.asarray(rec, np.float64).reshape(-1, 6)
    xm = max(abs(0.0 - cam.cx), abs(cam.cols - 1 - cam.cx)) / cam.fx
    ym = max(abs(0.0 - cam.cy), abs(cam.rows - 1 - cam.cy)) / cam.fy
    reach = cam.max_depth * np.sqrt(1.0 + xm * xm + ym * ym)
    dist = np.hypot(rec[:, 1] - pos[0], rec[:, 2] - pos[1]) - 0.5 * rec[:, 4]
    return rec[(rec[:, 0] != 3) | (dist <= reach * 1.001)]


def render(rec, cam, pos, rot):
    """One image.  rec (n, 6) rows {type, x, y, z, w, h}, cam: anything with SogmDepthCamera's fields, pos [3], rot [9] or
    [3, 3] row-major camera-to-world.  Returns (depth [rows, cols] uint16, cloud [rows*cols, 3] float32, unsupported)."""
    rec = np.asarray(rec, np.float64).reshape(-1, 6)
    R = np.asarray(rot, np.float64).reshape(3, 3)
    p = np.asarray(pos, np.float64).reshape(3)
    rows, cols = int(cam.rows), int(cam.cols)
    du = np.broadcast_to(np.arange(cols, dtype=np.float64)[None, :] - cam.cx, (rows, cols))
    dv = np.broadcast_to(np.arange(rows, dtype=np.float64)[:, None] - cam.cy, (rows, cols))
    xc, yc = du / cam.fx, dv / cam.fy
    d0, d1, d2 = [(R[i, 0] * xc + R[i, 1] * yc) + R[i, 2] for i in range(3)]
    best = np.full((rows, cols), np.inf)

    def accept(t, ok):
        nonlocal best
        best = np.where(ok & (t < best), t, best)

    unsupported = 0
    a = d0 * d0 + d1 * d1
    with np.errstate(all="ignore"):
        for typ, x, y, z, w, h in rec:
            if typ != 3:
                unsupported += 1
                continue
            r, z0, z1, ox, oy = 0.5 * w, z - 0.5 * h, z + 0.5 * h, p[0] - x, p[1] - y
            b = ox * d0 + oy * d1
            c = (ox * ox + oy * oy) - r * r
            disc = b * b - a * c
            side = (a > 0) & (disc >= 0)
            s = np.sqrt(np.where(side, disc, 0.0))
            for t in ((-b - s) / a, (-b + s) / a):
                zt = p[2] + t * d2
                accept(t, side & (t > 0) & (z0 <= zt) & (zt <= z1))
            for zp in (z0, z1):
                t = (zp - p[2]) / d2
                qx, qy = ox + t * d0, oy + t * d1
                accept(t, (d2 != 0) & (t > 0) & (qx * qx + qy * qy <= r * r))
        if cam.use_ground:
            t = (cam.ground_z - p[2]) / d2
            accept(t, (d2 != 0) & (t > 0))
        hit = np.isfinite(best) & (best <= cam.max_depth)
        d16 = np.where(hit, np.floor(np.where(hit, best, 0.0) * cam.depth_scale + 0.5), 0.0).astype(np.uint16)
    zq = d16.astype(np.float64) / cam.depth_scale
    cloud = np.stack([(du * zq / cam.fx).astype(np.float32), (dv * zq / cam.fy).astype(np.float32), zq.astype(np.float32)],
                     axis=-1)
    cloud[d16 == 0] = np.nan
    return d16, cloud.reshape(-1, 3), unsupported


def render_agents(rec, cam, pos, rot, cull=False):
    """every agent's image: (depth [A, rows, cols] uint16, cloud [A*rows*cols, 3] float32, unsupported [A] int32).
    cull=True tries only in_range()'s records (tests/test_depth_render.py shows that it changes nothing)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    rot = np.asarray(rot, np.float64).reshape(-1, 9)
    out = [render(in_range(rec, cam, pos[a]) if cull else rec, cam, pos[a], rot[a]) for a in range(len(pos))]
    return (np.stack([o[0] for o in out]), np.concatenate([o[1] for o in out], axis=0),
            np.array([o[2] for o in out], np.int32))


def same(depth, cloud, want_depth, want_cloud):
    """the header's equality: equal uint16 images; clouds equal bit for bit where finite, same NaN mask"""
    depth = np.asarray(depth).view(np.uint16).reshape(want_depth.shape)
    if not np.array_equal(depth, want_depth):
        return False, f"{int((depth != want_depth).sum())} of {depth.size} depth pixels differ"
    if cloud is not None:
        cloud = np.asarray(cloud, np.float32).reshape(want_cloud.shape)
        nan, wnan = np.isnan(cloud), np.isnan(want_cloud)
        if not np.array_equal(nan, wnan):
            return False, "cloud NaN masks differ"
        if not np.array_equal(cloud.view(np.int32)[~nan], want_cloud.view(np.int32)[~wnan]):
            return False, "cloud bits differ"
        if not np.array_equal(nan.all(axis=1), depth.reshape(-1) == 0) or (nan.any(axis=1) != nan.all(axis=1)).any():
            return False, "cloud NaN mask is not the image's zero mask"
    return True, ""
