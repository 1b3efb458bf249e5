"""The view mask restated in numpy from the text of include/sogm_abi.h "view mask" alone (not from csrc/sogm_viewmask.hpp):
whole arrays, one IEEE fp64 operation per numpy operation, no bit words until the packing.  Plus audit_with_region: the map
audit's six counts on a GIVEN boolean region, from "map audit"'s text (occupied, volume and dilate are
tests/map_audit_reference.py's)."""
import numpy as np

from map_audit_reference import dilate, occupied, volume

OUTSIDE, OFFIMAGE, FREE, SURFACE, HIDDEN = 0, 1, 2, 3, 4
BIT = {OUTSIDE: 1, OFFIMAGE: 2, FREE: 4, SURFACE: 8, HIDDEN: 16}
ALL = 31
CENTRE, SKIPPED = 1, 2


def cell_centres(dims, resolution, offset=None):
    """p_d = (((double)i_d + 0.5) * (double)res - (double)range_d) - off_d; range_d = (float)(N_d / 2) * res in fp32; offset
    None: no subtraction"""
    res = np.float32(resolution)
    out = []
    for d, n in enumerate(dims):
        rng = np.float32(n // 2) * res
        assert rng.dtype == np.float32
        p = (np.arange(n, dtype=np.float64) + 0.5) * np.float64(res) - np.float64(rng)
        out.append(p if offset is None else p - np.float64(offset[d]))
    return out


def classify(dims, resolution, depth, rot, prm, offset=None):
    """int8 [H, W, L]: the class of every cell of one agent.  depth: uint16 [rows, cols]; rot: row-major [9]; prm: dict with fx
    fy cx cy depth_scale near_z far_z tan_h tan_v band"""
    depth = np.asarray(depth, np.uint16)
    rows, cols = depth.shape
    R = np.asarray(rot, np.float64).reshape(3, 3)
    px, py, pz = cell_centres(dims, resolution, offset)
    p0, p1, p2 = px[None, None, :], py[None, :, None], pz[:, None, None]
    f = lambda k: np.float64(prm[k])                                                              # noqa: E731
    with np.errstate(all="ignore"):
        q = [(R[0, j] * p0 + R[1, j] * p1) + R[2, j] * p2 for j in range(3)]
        qx, qy, qz = (np.broadcast_to(v, (dims[2], dims[1], dims[0])) for v in q)
        inside = (qz > f("near_z")) & (qz <= f("far_z")) & (np.abs(qx) <= qz * f("tan_h")) & (np.abs(qy) <= qz * f("tan_v"))
        uf = (qx / qz) * f("fx") + f("cx")
        vf = (qy / qz) * f("fy") + f("cy")
        u, v = np.floor(uf + 0.5), np.floor(vf + 0.5)
        on = (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
        ui = np.where(inside & on, u, 0).astype(np.int64)
        vi = np.where(inside & on, v, 0).astype(np.int64)
        d16 = depth[vi, ui]
        z_hit = d16.astype(np.float64) / f("depth_scale")
        cls = np.full(qz.shape, HIDDEN, np.int8)
        cls[qz <= z_hit + f("band")] = SURFACE
        cls[qz < z_hit - f("band")] = FREE
        cls[d16 == 0] = FREE
        cls[~on] = OFFIMAGE
        cls[~inside] = OUTSIDE
    return cls


def pack(bits):
    """bool [H, W, L] -> uint64 [H, W, ceil(L / 64)]: cell x is bit x % 64 of word x / 64, spare bits clear"""
    H, W, L = bits.shape
    nw = (L + 63) // 64
    pad = np.zeros((H, W, nw * 64), np.uint64)
    pad[:, :, :L] = bits
    weights = np.left_shift(np.uint64(1), np.arange(64, dtype=np.uint64))
    return (pad.reshape(H, W, nw, 64) * weights).sum(axis=3, dtype=np.uint64)


def unpack(words, L):
    """uint64 [..., nw] -> bool [..., L]"""
    words = np.asarray(words).view(np.uint64)
    bits = (words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(*words.shape[:-1], -1)[..., :L].astype(bool)


def view_mask(dims, resolution, depths, rots, prm, classes, offsets=None):
    """(cls int8 [n, H, W, L], words uint64 [n, H, W, nw], counts int32 [n, 8]) for n agents"""
    cls = np.stack([classify(dims, resolution, depths[a], rots[a], prm, None if offsets is None else offsets[a])
                    for a in range(len(depths))])
    sel = np.zeros(cls.shape, bool)
    for c, b in BIT.items():
        if classes & b:
            sel |= cls == c
    counts = np.zeros((len(depths), 8), np.int32)
    for c in range(5):
        counts[:, c] = (cls == c).sum(axis=(1, 2, 3))
    counts[:, 5] = sel.sum(axis=(1, 2, 3))
    return cls, np.stack([pack(s) for s in sel]), counts


def audit_with_region(test_vt, truth_vt, R, dims, thr_test, thr_truth, r=0, box=None, slice_map=None, centre_differs=False):
    """rows int32 [T_test, 8] of one agent in SogmMapAuditRow's order: "map audit"'s counts with region = box & R (bool
    [H, W, L])"""
    vt, vg = volume(test_vt, dims), volume(truth_vt, dims)
    T_test, T_truth = vt.shape[0], vg.shape[0]
    if slice_map is None:
        slice_map = [t if t < min(T_test, T_truth) else -1 for t in range(T_test)]
    R = np.array(R, bool)
    if box is not None:
        lo, hi = box
        inbox = np.zeros_like(R)
        inbox[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
        R &= inbox
    rows = np.zeros((T_test, 8), np.int32)
    for t in range(T_test):
        s = int(slice_map[t])
        rows[t, 6] = s
        if s < 0:
            rows[t, 7] = SKIPPED
            continue
        if centre_differs:
            rows[t, 7] = CENTRE
            continue
        ot, og = occupied(vt[t], thr_test), occupied(vg[s], thr_truth)
        rows[t, :6] = [R.sum(), (ot & R).sum(), (og & R).sum(), (ot & og & R).sum(), (ot & dilate(og, r) & R).sum(),
                       (og & dilate(ot, r) & R).sum()]
    return rows
