"""The depth camera's sensor-noise pass (include/sogm_abi.h "sensor noise") restated in numpy, vectorised over the pixels of
one image and written from the header's text alone: uint64 arithmetic that wraps, fp64 one operation at a time in the
header's order.  No skipped draws, no early exits: every pixel forms every draw and every rule, and masks choose.
Test infrastructure; not collected by pytest."""
from types import SimpleNamespace

import numpy as np

HIT_NONE = -2
COUNTERS = ("returns_in", "drop_uniform", "drop_edge", "below_min", "beyond_max", "returns_out")
U64 = np.uint64


def params(seed=0, frame=0, agent_base=0, sigma=(0.0, 0.0, 0.0), p_drop=0.0, edge_jump=0.0, p_edge=0.0, min_depth=0.0):
    return SimpleNamespace(seed=int(seed), frame=int(frame), agent_base=int(agent_base), sigma0=float(sigma[0]),
                           sigma1=float(sigma[1]), sigma2=float(sigma[2]), p_drop=float(p_drop), edge_jump=float(edge_jump),
                           p_edge=float(p_edge), min_depth=float(min_depth))


def mix(x):
    x = np.asarray(x, U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        return x ^ (x >> U64(31))


def pixel_key(seed, frame, g):
    """h of the pixels with swarm-wide indices g"""
    return mix(mix(mix(U64(seed)) ^ U64(frame)) ^ np.asarray(g, U64))


def draw(h, k):
    with np.errstate(over="ignore"):
        return mix(np.asarray(h, U64) + U64(k))


def uniform(w):
    return (np.asarray(w, U64) >> U64(11)).astype(np.float64) * 2.0 ** -53


def pieces_sum(h):
    S = np.zeros(np.shape(h), np.int64)
    for k in (2, 3, 4):
        w = draw(h, k)
        for j in range(4):
            S = S + ((w >> U64(16 * j)) & U64(0xFFFF)).astype(np.int64)
    return S


def normal(h):
    return (pieces_sum(h).astype(np.float64) - 393210.0) * 2.0 ** -16


def edges(d16, depth_scale, edge_jump):
    """the edge pixels of one INPUT image [rows, cols] (for pixels with a return; the others' value is not used)"""
    d16 = np.asarray(d16, np.uint16)
    rows, cols = d16.shape
    z = d16.astype(np.float64) / depth_scale
    edge = np.zeros((rows, cols), bool)
    for dv in (-1, 0, 1):
        for du in (-1, 0, 1):
            if dv == 0 and du == 0:
                continue
            # the part of the image whose neighbour at (dv, du) exists
            v0, v1, u0, u1 = max(0, -dv), rows - max(0, dv), max(0, -du), cols - max(0, du)
            if v0 >= v1 or u0 >= u1:
                continue
            dn = d16[v0 + dv:v1 + dv, u0 + du:u1 + du]
            zn = z[v0 + dv:v1 + dv, u0 + du:u1 + du]
            edge[v0:v1, u0:u1] |= (dn == 0) | (np.abs(zn - z[v0:v1, u0:u1]) > edge_jump)
    return edge


def noise_image(cam, prm, a, d16):
    """local agent a's image: (d16' [rows, cols] uint16, counts [6] int64, outcome masks)"""
    d16 = np.asarray(d16, np.uint16)
    rows, cols = d16.shape
    assert (rows, cols) == (cam.rows, cam.cols)
    v, u = np.meshgrid(np.arange(rows, dtype=U64), np.arange(cols, dtype=U64), indexing="ij")
    with np.errstate(over="ignore"):
        g = (U64(prm.agent_base + a) * U64(rows) + v) * U64(cols) + u
    h = pixel_key(prm.seed, prm.frame, g)
    ret = d16 != 0
    z = d16.astype(np.float64) / cam.depth_scale
    drop_u = ret & (uniform(draw(h, 0)) < prm.p_drop)
    live = ret & ~drop_u
    if prm.edge_jump > 0:
        drop_e = live & edges(d16, cam.depth_scale, prm.edge_jump) & (uniform(draw(h, 1)) < prm.p_edge)
    else:
        drop_e = np.zeros_like(ret)
    live = live & ~drop_e
    s = (prm.sigma2 * z + prm.sigma1) * z + prm.sigma0
    zn = z + s * normal(h)
    below = live & ~(zn >= prm.min_depth)
    beyond = live & ~below & (zn > cam.max_depth)
    live = live & ~below & ~beyond
    q = np.floor(np.where(live, zn, 0.0) * cam.depth_scale + 0.5)
    zero = live & (q == 0)
    below = below | zero
    live = live & ~zero
    out = np.where(live, q, 0.0).astype(np.uint16)
    counts = np.array([ret.sum(), drop_u.sum(), drop_e.sum(), below.sum(), beyond.sum(), live.sum()], np.int64)
    return out, counts, SimpleNamespace(drop_uniform=drop_u, drop_edge=drop_e, below_min=below, beyond_max=beyond, out=live)


def backproject(cam, d16):
    """"depth camera"'s cloud of one image: [rows*cols, 3] float32, NaN where d16 == 0"""
    d16 = np.asarray(d16, np.uint16)
    v, u = np.meshgrid(np.arange(cam.rows, dtype=np.float64), np.arange(cam.cols, dtype=np.float64), indexing="ij")
    zq = d16.astype(np.float64) / cam.depth_scale
    cloud = np.stack([((u - cam.cx) * zq / cam.fx).astype(np.float32), ((v - cam.cy) * zq / cam.fy).astype(np.float32),
                      zq.astype(np.float32)], axis=-1)
    cloud[d16 == 0] = np.nan
    return cloud.reshape(-1, 3)


def add_noise(cam, prm, depth, hit=None):
    """every local agent: (depth' [A, rows, cols] uint16, cloud [A*rows*cols, 3] float32, hit' [A, rows, cols] int32 or None,
    counts [A, 6] int32)"""
    depth = np.asarray(depth, np.uint16).reshape(-1, cam.rows, cam.cols)
    outs = [noise_image(cam, prm, a, depth[a]) for a in range(len(depth))]
    d = np.stack([o[0] for o in outs])
    cloud = np.concatenate([backproject(cam, x) for x in d], axis=0)
    h = None
    if hit is not None:
        h = np.where(d != 0, np.asarray(hit, np.int32).reshape(d.shape), HIT_NONE).astype(np.int32)
    return d, cloud, h, np.stack([o[1] for o in outs]).astype(np.int32)


def same_cloud(got, want):
    """equal as int32 where finite, the same NaN mask"""
    got, want = np.asarray(got, np.float32).reshape(-1, 3), np.asarray(want, np.float32).reshape(-1, 3)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~wn], want.view(np.int32)[~wn])
