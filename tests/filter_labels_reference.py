"""A numpy reading of include/sogm_abi.h "ground-truth labels" (sogm_filter_point_cloud_labelled), written from the header's
text and not from the kernel: the voxel filter's leaves (leaf index floorf(p * inv_leaf) per axis in fp32, ascending leaf
order, axis swap, isInRange, cap), per leaf the winner among its finite points (smallest camera-frame z by the order-preserving
key of its bits, then the largest code), and the winner's label in fp32.

Two implementations of the same text: `filter_labelled` (sorting, vectorised) and `filter_labelled_loop` (a plain Python loop
over a dict of leaves that compares floats and codes directly, no packed key) — tests hold one to the other.

Centroids: fp32 sums in INPUT order, then one fp32 division per axis.  A device's atomic order differs: they are held to 1e-4,
labels and codes bit for bit."""
import numpy as np

HIT_GROUND, HIT_NONE = -1, -2
KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
f32 = np.float32


# ---- the key --------------------------------------------------------------------------------------------------------------
def f2key(z):
    """the order-preserving unsigned image of fp32 bits: sign set -> ~bits, else bits | 0x80000000"""
    bits = np.ascontiguousarray(z, f32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def pack_key(z, code):
    """high word f2key(z); low word the complement of the unsigned image of the int32 code: the smallest key is 'smallest z,
    then largest code'"""
    image = np.ascontiguousarray(code, np.int32).view(np.uint32) ^ np.uint32(0x80000000)
    return (f2key(z).astype(np.uint64) << np.uint64(32)) | (~image).astype(np.uint64)


def key_code(key):
    low = (np.asarray(key, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return ((~low) ^ np.uint32(0x80000000)).view(np.int32)


# ---- the label ------------------------------------------------------------------------------------------------------------
def label_of(code, rec_vel, body_vel, min_speed):
    """code int32 [n]; rec_vel fp64 [n_cyl, 2] (the records' vx, vy); body_vel fp64 [n_bodies, 3]; -> fp32 [n, 4]"""
    code = np.asarray(code, np.int64).reshape(-1)
    rec_vel = np.asarray(rec_vel, np.float64).reshape(-1, 2)
    body_vel = np.asarray(body_vel if body_vel is not None else [], np.float64).reshape(-1, 3)
    n_cyl, n_bodies = len(rec_vel), len(body_vel)
    v = np.zeros((len(code), 3), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        is_rec = (code >= 0) & (code < n_cyl)
        if is_rec.any():
            v[is_rec, :2] = rec_vel[code[is_rec]].astype(f32)
        is_body = (code >= n_cyl) & (code < n_cyl + n_bodies)
        if is_body.any():
            v[is_body] = body_vel[code[is_body] - n_cyl].astype(f32)
        s2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        m = f32(min_speed)
        on = np.isfinite(v).all(axis=1) & (s2 > m * m)
    out = np.zeros((len(code), 4), f32)
    out[on, :3] = v[on]
    out[on, 3] = f32(1.0)
    return out


# ---- the filter -----------------------------------------------------------------------------------------------------------
def leaf_ijk(raw, leaf):
    inv = f32(1.0) / f32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(np.asarray(raw, f32) * inv).astype(np.int64)


def _too_many(ijk, max_cells):
    div = ijk.max(axis=0) - ijk.min(axis=0) + 1
    return int(div[0]) * int(div[1]) * int(div[2]) > max_cells


def _emit(leaves, rng, cap):
    """leaves: ascending list of (sum xyz fp32 [3], count, code); -> the rows that pass the swap, isInRange and the cap"""
    pts, codes = [], []
    for s, c, code in leaves:
        cx, cy, cz = s[0] / f32(c), s[1] / f32(c), s[2] / f32(c)
        o = (cz, -cx, -cy)
        if all(-r < x < r for x, r in zip(o, rng)):
            pts.append(o)
            codes.append(code)
            if len(pts) >= cap:
                break
    return np.array(pts, f32).reshape(-1, 3), np.array(codes, np.int32)


def filter_labelled(raw, code, leaf, cap, rng, rec_vel, body_vel, min_speed, max_cells=1 << 20):
    """raw fp32 [n, 3] camera frame, code int32 [n], rng = the map's half ranges (rx, ry, rz) as fp32.
    -> (points fp32 [k, 3], labels fp32 [k, 4], codes int32 [k], count); count is -1 (and k = 0) when the cloud's bounding box
    has more than max_cells leaves"""
    raw, code = np.asarray(raw, f32).reshape(-1, 3), np.asarray(code, np.int32).reshape(-1)
    rng = [f32(r) for r in rng]
    fin = np.isfinite(raw).all(axis=1)
    none = (np.zeros((0, 3), f32), np.zeros((0, 4), f32), np.zeros((0,), np.int32))
    if not fin.any():
        return (*none, 0)
    p, c = raw[fin], code[fin]
    ijk = leaf_ijk(p, leaf)
    if _too_many(ijk, max_cells):
        return (*none, -1)
    key = pack_key(p[:, 2], c)
    order = np.lexsort((key, ijk[:, 0], ijk[:, 1], ijk[:, 2]))        # leaf ascending (z index slowest), then the key
    s_ijk = ijk[order]
    first = np.ones(len(order), bool)
    first[1:] = (s_ijk[1:] != s_ijk[:-1]).any(axis=1)
    group = np.cumsum(first) - 1                                       # the leaf's rank, per sorted point
    n_leaf = int(group[-1]) + 1
    win_code = key_code(key[order][first])
    leaf_of_point = np.empty(len(p), np.int64)
    leaf_of_point[order] = group
    sums, cnt = np.zeros((n_leaf, 3), f32), np.zeros(n_leaf, np.int64)
    for k in range(3):
        np.add.at(sums[:, k], leaf_of_point, p[:, k])                  # unbuffered: fp32 adds in input order
    np.add.at(cnt, leaf_of_point, 1)
    pts, codes = _emit([(sums[i], cnt[i], win_code[i]) for i in range(n_leaf)], rng, cap)
    return pts, label_of(codes, rec_vel, body_vel, min_speed), codes, len(pts)


def _before(z1, c1, z2, c2):
    """is the point (z1, c1) a better winner than (z2, c2)?  Floats and ints compared directly."""
    if z1 != z2:
        return z1 < z2
    if z1 == 0.0 and np.signbit(z1) != np.signbit(z2):
        return bool(np.signbit(z1))                                    # -0 before +0
    return c1 > c2


def filter_labelled_loop(raw, code, leaf, cap, rng, rec_vel, body_vel, min_speed, max_cells=1 << 20):
    """the same text as a plain loop over a dict of leaves"""
    raw, code = np.asarray(raw, f32).reshape(-1, 3), np.asarray(code, np.int32).reshape(-1)
    rng = [f32(r) for r in rng]
    inv = f32(1.0) / f32(leaf)
    leaves = {}
    for pnt, c in zip(raw, code):
        if not (np.isfinite(pnt[0]) and np.isfinite(pnt[1]) and np.isfinite(pnt[2])):
            continue
        ix, iy, iz = (int(np.floor(pnt[k] * inv)) for k in range(3))
        cell = leaves.get((iz, iy, ix))
        if cell is None:
            leaves[(iz, iy, ix)] = [np.zeros(3, f32) + pnt, 1, pnt[2], int(c)]      # (a sum that starts at +0: -0 becomes +0)
            continue
        cell[0] = cell[0] + pnt                                        # fp32, input order
        cell[1] += 1
        if _before(pnt[2], int(c), cell[2], cell[3]):
            cell[2], cell[3] = pnt[2], int(c)
    none = (np.zeros((0, 3), f32), np.zeros((0, 4), f32), np.zeros((0,), np.int32))
    if not leaves:
        return (*none, 0)
    idx = np.array(list(leaves.keys()), np.int64)
    if _too_many(idx, max_cells):
        return (*none, -1)
    pts, codes = _emit([(leaves[k][0], leaves[k][1], leaves[k][3]) for k in sorted(leaves)], rng, cap)
    labels = np.concatenate([label_of([c], rec_vel, body_vel, min_speed) for c in codes]).reshape(-1, 4) if len(codes) else none[1]
    return pts, labels, codes, len(pts)


def map_range(spec):
    """the half ranges isInRange tests: (L/2, W/2, H/2) voxels times the resolution, fp32"""
    return [f32(n // 2) * f32(spec.resolution) for n in (spec.L, spec.W, spec.H)]
