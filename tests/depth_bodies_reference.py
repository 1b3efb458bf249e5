"""The depth camera with agent bodies and the hit index (include/sogm_abi.h "agent bodies") restated in numpy, vectorised
over the pixels of one image and written from the header's text alone: every expression is the header's, in its order, in
fp64.  The rays, the ring's frame and the ring's hit are tests/depth_ring_reference.py's; a cylinder's own t (the smallest
accepted of its two side roots and two caps), the body's slab rule, the composition by (t, code) and the hit image are
written here.  No culling, no early exits.  Test infrastructure; not collected by pytest."""
import numpy as np

import depth_ring_reference as ringref

HIT_GROUND, HIT_NONE = -1, -2
BODY = (0.4, 0.4, 0.45)
UNSET = np.iinfo(np.int32).max


def hmin(x, y):
    """the header's min(x, y): x if x < y, else y"""
    return np.where(x < y, x, y)


def hmax(x, y):
    return np.where(x > y, x, y)


def cylinder_t(row, p, d):
    """the smallest accepted t of one type-3 record per pixel ("depth camera"), +inf where it has none"""
    _, x, y, z, w, h = [np.float64(v) for v in row[:6]]
    d0, d1, d2 = d
    best = np.full(d0.shape, np.inf)
    with np.errstate(all="ignore"):
        r, z0, z1, ox, oy = 0.5 * w, z - 0.5 * h, z + 0.5 * h, p[0] - x, p[1] - y
        a = d0 * d0 + d1 * d1
        b = ox * d0 + oy * d1
        c = (ox * ox + oy * oy) - r * r
        disc = b * b - a * c
        side = (a > 0) & (disc >= 0)
        s = np.sqrt(np.where(side, disc, 0.0))
        for t in ((-b - s) / a, (-b + s) / a):
            zt = p[2] + t * d2
            ok = side & (t > 0) & (z0 <= zt) & (zt <= z1)
            best = np.where(ok & (t < best), t, best)
        for zp in (z0, z1):
            t = (zp - p[2]) / d2
            qx, qy = ox + t * d0, oy + t * d1
            ok = (d2 != 0) & (t > 0) & (qx * qx + qy * qy <= r * r)
            best = np.where(ok & (t < best), t, best)
    return best


def body_hit(centre, size, p, d):
    """(hit, t) of one body per pixel (the centre is finite); an accepted t may be +inf (overflowing quotients)"""
    shape = d[0].shape
    tn, tf = np.full(shape, -np.inf), np.full(shape, np.inf)
    live = np.ones(shape, bool)
    with np.errstate(all="ignore"):
        for i in range(3):
            half = 0.5 * np.float64(size[i])
            lo, hi = np.float64(centre[i]) - half, np.float64(centre[i]) + half
            zero = d[i] == 0
            live &= ~(zero & ~((lo <= p[i]) & (p[i] <= hi)))
            ta, tb = (lo - p[i]) / d[i], (hi - p[i]) / d[i]
            tn = np.where(zero, tn, hmax(tn, hmin(ta, tb)))
            tf = np.where(zero, tf, hmin(tf, hmax(ta, tb)))
        live &= tn <= tf
        live &= (tn > 0) | (tf > 0)
        t = np.where(tn > 0, tn, tf)
    return live, np.where(live, t, np.inf)


def body_t(centre, size, p, d):
    """the accepted t of one body per pixel, +inf where there is none"""
    return body_hit(centre, size, p, d)[1]


def sources(rows12, cam, pos, rot, body_pos, own, size=BODY, rings=False):
    """One camera: ([(code, t per pixel)] for every record and body that is drawn, unsupported).  own: the index of the body
    that carries this camera (any value outside [0, n_bodies): none)."""
    rows12 = np.asarray(rows12, np.float64).reshape(-1, 12)
    body_pos = np.zeros((0, 3)) if body_pos is None else np.asarray(body_pos, np.float64).reshape(-1, 3)
    p = np.asarray(pos, np.float64).reshape(3)
    d, _, _ = ringref.rays(cam, rot)
    out, unsupported = [], 0
    for i, row in enumerate(rows12):
        if row[0] == 3:
            out.append((i, cylinder_t(row, p, d)))
        elif row[0] == 2 and rings and ringref.frame(row) is not None:
            c, R, rho, _, _, n = ringref.frame(row)
            out.append((i, ringref.ray_hit(p, d, c, R, rho, n)[0]))
        else:
            unsupported += 1
    for j, b in enumerate(body_pos):
        if j == own:
            continue
        if not np.isfinite(b).all():
            unsupported += 1
            continue
        out.append((len(rows12) + j, body_t(b, size, p, d)))
    return out, unsupported


def render(rows12, cam, pos, rot, body_pos=None, own=-1, size=BODY, rings=False):
    """One image: (depth [rows, cols] uint16, cloud [rows*cols, 3] float32, unsupported, hit [rows, cols] int32).  The code
    of a pixel is that of the smallest (t, code) pair over records and bodies; the ground wins only with a smaller t."""
    p = np.asarray(pos, np.float64).reshape(3)
    d, du, dv = ringref.rays(cam, rot)
    src, unsupported = sources(rows12, cam, pos, rot, body_pos, own, size, rings)
    best = np.full(d[0].shape, np.inf)
    code = np.full(d[0].shape, UNSET, np.int64)
    for c, t in src:
        better = (t < best) | ((t == best) & (c < code))
        best, code = np.where(better, t, best), np.where(better, c, code)
    with np.errstate(all="ignore"):
        if cam.use_ground:
            t = (cam.ground_z - p[2]) / d[2]
            better = (d[2] != 0) & (t > 0) & (t < best)
            best, code = np.where(better, t, best), np.where(better, HIT_GROUND, code)
        hit = np.isfinite(best) & (best <= cam.max_depth)
        d16 = np.where(hit, np.floor(np.where(hit, best, 0.0) * cam.depth_scale + 0.5), 0.0).astype(np.uint16)
    zq = d16.astype(np.float64) / cam.depth_scale
    cloud = np.stack([(du * zq / cam.fx).astype(np.float32), (dv * zq / cam.fy).astype(np.float32), zq.astype(np.float32)],
                     axis=-1)
    cloud[d16 == 0] = np.nan
    return d16, cloud.reshape(-1, 3), unsupported, np.where(d16 == 0, HIT_NONE, code).astype(np.int32)


def owners(n_agents, cam_body=None):
    return list(range(n_agents)) if cam_body is None else [int(v) for v in cam_body]


def render_agents(rows12, cam, pos, rot, body_pos=None, cam_body=None, size=BODY, rings=False):
    """every camera: (depth [A, rows, cols] uint16, cloud [A*rows*cols, 3] float32, unsupported [A] int32,
    hit [A, rows, cols] int32)"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    rot = np.asarray(rot, np.float64).reshape(-1, 9)
    own = owners(len(pos), cam_body)
    out = [render(rows12, cam, pos[a], rot[a], body_pos, own[a], size, rings) for a in range(len(pos))]
    return (np.stack([o[0] for o in out]), np.concatenate([o[1] for o in out], axis=0),
            np.array([o[2] for o in out], np.int32), np.stack([o[3] for o in out]))


def face_hit(centre, size, p, d):
    """A different algorithm, to judge the rule and not to restate it: each of the six faces on its own — the ray against
    the face's plane, then the point p + t d against the face's rectangle — and the smallest t > 0 of the faces hit."""
    best = np.full(d[0].shape, np.inf)
    c, h = np.asarray(centre, np.float64), 0.5 * np.asarray(size, np.float64)
    with np.errstate(all="ignore"):
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            for plane in (c[i] - h[i], c[i] + h[i]):
                t = (plane - p[i]) / d[i]
                qj, qk = p[j] + t * d[j], p[k] + t * d[k]
                ok = (d[i] != 0) & (t > 0) & (np.abs(qj - c[j]) <= h[j]) & (np.abs(qk - c[k]) <= h[k])
                best = np.where(ok & (t < best), t, best)
    return best
