"""The ray rule of include/sogm_abi.h ("ring obstacles") and the depth camera with SOGM_DEPTH_RINGS restated in numpy,
vectorised over the pixels of one image and written from the header's text alone: every expression is the header's, in its
order, in fp64.  Everything that is not a ring — cylinders, caps, ground, quantisation — is tests/depth_render_reference.py's.
Test infrastructure; not collected by pytest."""
import numpy as np

import depth_render_reference as cylref


def records(cyl):
    """a ctypes SogmCylinder array (or any sequence of such records) -> (n, 12) float64 rows
    {type, x, y, z, w, h, vx, vy, qw, qx, qy, qz}"""
    return np.array([[o.type, o.x, o.y, o.z, o.w, o.h, o.vx, o.vy, o.qw, o.qx, o.qy, o.qz] for o in cyl],
                    np.float64).reshape(-1, 12)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def frame(row):
    """None for "not a ring", else (c [3], R, rho, e1, e2, n)"""
    row = np.asarray(row, np.float64)
    _, x, y, z, w, h, vx, vy, qw, qx, qy, qz = row
    if not np.isfinite(row[1:]).all():
        return None
    R, rho = 0.5 * w, h
    if not R > 0 or not rho > 0 or not rho < R:
        return None
    with np.errstate(all="ignore"):
        qn = np.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    if not np.isfinite(qn) or not qn > 0:
        return None
    w_, x_, y_, z_ = qw / qn, qx / qn, qy / qn, qz / qn
    e1 = np.array([1 - 2 * (y_ * y_ + z_ * z_), 2 * (x_ * y_ + w_ * z_), 2 * (x_ * z_ - w_ * y_)])
    e2 = np.array([2 * (x_ * y_ - w_ * z_), 1 - 2 * (x_ * x_ + z_ * z_), 2 * (y_ * z_ + w_ * x_)])
    n = np.array([2 * (x_ * z_ + w_ * y_), 2 * (y_ * z_ - w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)])
    return np.array([x, y, z]), R, rho, e1, e2, n


def coefficients(p, d, c, R, rho, n):
    """the scalars and the quartic of the rule for rays p + t d (d: three arrays of one shape)"""
    o = p - c
    alpha, beta, gamma = dot(d, d), dot(o, d), dot(o, o)
    no, nd = dot(n, o), dot(n, d)
    RR = R * R
    K = (gamma + RR) - rho * rho
    c4 = alpha * alpha
    c3 = (4 * alpha) * beta
    c2 = ((4 * beta) * beta + (2 * alpha) * K) - (4 * RR) * (alpha - nd * nd)
    c1 = (4 * beta) * K - (8 * RR) * (beta - no * nd)
    c0 = K * K - (4 * RR) * (gamma - no * no)
    return alpha, beta, gamma, no, nd, (c4, c3, c2, c1, c0)


def ray_hit(p, d, c, R, rho, n):
    """t of the ring's hit per ray, +inf where there is none.  Also returns the interval (t0, t1, live) the search ran on."""
    shape = d[0].shape
    alpha, beta, gamma, no, nd, (c4, c3, c2, c1, c0) = coefficients(p, d, c, R, rho, n)

    def f(t):
        return (((c4 * t + c3) * t + c2) * t + c1) * t + c0

    with np.errstate(all="ignore"):
        live = alpha > 0
        S = R + rho
        cs = gamma - S * S
        disc = beta * beta - alpha * cs
        live &= ~(disc < 0)
        s = np.sqrt(np.where(live, disc, 0.0))
        t0 = (-beta - s) / alpha
        t1 = (-beta + s) / alpha
        flat = nd == 0
        live &= ~(flat & ~(np.abs(no) <= rho))
        ta, tb = (-rho - no) / nd, (rho - no) / nd
        lo, hi = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
        t0 = np.where(~flat & (lo > t0), lo, t0)
        t1 = np.where(~flat & (hi < t1), hi, t1)
        t0 = np.where(t0 < 0, 0.0, t0)
        live &= t0 <= t1
        t0, t1 = np.where(live, t0, 0.0), np.where(live, t1, 0.0)
        hit = np.full(shape, np.inf)
        f0 = f(t0)
        inside = live & (f0 <= 0)
        hit = np.where(inside & (t0 > 0), t0, hit)          # t0 == 0: the camera is inside the tube, no return
        todo = live & ~inside
        hs = (t1 - t0) / 32.0
        lo_b, hi_b = t0.copy(), np.zeros(shape)
        found = np.zeros(shape, bool)
        prev = t0
        for i in range(1, 33):
            node = t1 if i == 32 else t0 + float(i) * hs
            first = todo & ~found & (f(node) <= 0)
            lo_b = np.where(first, prev, lo_b)
            hi_b = np.where(first, node, hi_b)
            found |= first
            prev = node
        for _ in range(48):
            m = 0.5 * (lo_b + hi_b)
            neg = f(m) <= 0
            hi_b = np.where(neg, m, hi_b)
            lo_b = np.where(neg, lo_b, m)
        hit = np.where(found, hi_b, hit)
    return hit, (t0, t1, live)


def rays(cam, rot):
    """the camera section's d_0, d_1, d_2 and du, dv per pixel"""
    R = np.asarray(rot, np.float64).reshape(3, 3)
    rows, cols = int(cam.rows), int(cam.cols)
    du = np.broadcast_to(np.arange(cols, dtype=np.float64)[None, :] - cam.cx, (rows, cols))
    dv = np.broadcast_to(np.arange(rows, dtype=np.float64)[:, None] - cam.cy, (rows, cols))
    xc, yc = du / cam.fx, dv / cam.fy
    return [(R[i, 0] * xc + R[i, 1] * yc) + R[i, 2] for i in range(3)], du, dv


def ring_depth(rows12, cam, pos, rot):
    """(t of the nearest ring hit per pixel (+inf none), number of type-2 records that are not rings)"""
    d, _, _ = rays(cam, rot)
    p = np.asarray(pos, np.float64).reshape(3)
    best = np.full(d[0].shape, np.inf)
    invalid = 0
    for row in rows12:
        if row[0] != 2:
            continue
        fr = frame(row)
        if fr is None:
            invalid += 1
            continue
        c, R, rho, _, _, n = fr
        t, _ = ray_hit(p, d, c, R, rho, n)
        best = np.where(t < best, t, best)
    return best, invalid


def render(rows12, cam, pos, rot, rings=True):
    """One image of records (n, 12).  rings=False is depth_render_reference.render itself.  rings=True: the pixel's t* is
    the minimum over everything accepted.  The cylinder reading returns its quantised image, not its t*; quantisation
    floor(t * depth_scale + 0.5) is monotone in t, so the image of the minimum is the minimum of the two images over the
    pixels where either has a return — except where a return quantises to 0 (t < 0.5 / depth_scale), which this reading
    refuses for rings (asserted) and the fixtures keep away from for everything else."""
    rows12 = np.asarray(rows12, np.float64).reshape(-1, 12)
    rec6 = rows12[:, [0, 1, 2, 3, 4, 5]]
    d_cyl, cloud_cyl, unsupported = cylref.render(rec6, cam, pos, rot)
    if not rings:
        return d_cyl, cloud_cyl, unsupported
    t_ring, invalid = ring_depth(rows12, cam, pos, rot)
    unsupported = unsupported - int((rows12[:, 0] == 2).sum()) + invalid
    hit = np.isfinite(t_ring) & (t_ring <= cam.max_depth)
    q = np.floor(np.where(hit, t_ring, 0.0) * cam.depth_scale + 0.5)
    assert not (hit & (q == 0)).any(), "a ring return nearer than half a depth unit"
    d_ring = np.where(hit, q, 0.0).astype(np.uint16)
    both = (d_cyl > 0) & (d_ring > 0)
    d16 = np.where(both, np.minimum(d_cyl, d_ring), np.maximum(d_cyl, d_ring)).astype(np.uint16)
    _, du, dv = rays(cam, rot)
    zq = d16.astype(np.float64) / cam.depth_scale
    cloud = np.stack([(du * zq / cam.fx).astype(np.float32), (dv * zq / cam.fy).astype(np.float32), zq.astype(np.float32)],
                     axis=-1)
    cloud[d16 == 0] = np.nan
    return d16, cloud.reshape(-1, 3), unsupported


def render_agents(rows12, cam, pos, rot, rings=True):
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    rot = np.asarray(rot, np.float64).reshape(-1, 9)
    out = [render(rows12, cam, pos[a], rot[a], rings) for a in range(len(pos))]
    return (np.stack([o[0] for o in out]), np.concatenate([o[1] for o in out], axis=0),
            np.array([o[2] for o in out], np.int32))


def exact_hit(p, d, c, R, rho, n):
    """one ray: the smallest real root t > 0 of the quartic (numpy.roots) at which the ray ENTERS or touches the torus,
    +inf if none; a camera inside the tube (f(0) < 0) gives +inf as the rule does.  Used to judge the rule, not to restate it."""
    dd = [np.float64(v) for v in d]
    _, _, _, _, _, co = coefficients(p, dd, c, R, rho, n)
    if co[4] < 0:
        return np.inf
    r = np.roots(np.array(co, np.float64))
    real = np.sort(r[np.abs(r.imag) < 1e-9 * np.maximum(1.0, np.abs(r.real))].real)
    real = real[real > 0]
    return float(real[0]) if len(real) else np.inf
