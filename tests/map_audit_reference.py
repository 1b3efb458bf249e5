"""The map audit restated in numpy from the text of include/sogm_abi.h "map audit" alone (not from csrc/sogm_mapaudit.hpp):
whole arrays, no bit words, no slabs.  A grid is what SogmMap.download returns: float32 [V, T], v = iz * L * W + iy * L + ix.
Dilation is a maximum over shifted zero-padded copies."""
import numpy as np

FRUSTUM = 1
CENTRE, SKIPPED = 1, 2
FIELDS = ("n_region", "n_test", "n_truth", "n_both", "n_test_near", "n_truth_near", "truth_slice", "status")


def occupied(values, thr):
    """value > thr in fp32, strict; a NaN is not occupied"""
    with np.errstate(invalid="ignore"):
        return np.asarray(values, np.float32) > np.float32(thr)


def volume(grid_vt, dims):
    """[V, T] -> [T, H, W, L]"""
    L, W, H = dims
    return np.moveaxis(np.asarray(grid_vt).reshape(H, W, L, -1), 3, 0)


def centres(dims, resolution):
    """p_d = ((double)i_d + 0.5) * (double)res - (double)range_d, range_d = (float)(N_d / 2) * res in fp32"""
    res = np.float32(resolution)
    out = []
    for n in dims:
        rng = np.float32(n // 2) * res
        assert rng.dtype == np.float32
        out.append((np.arange(n, dtype=np.float64) + 0.5) * np.float64(res) - np.float64(rng))
    return out


def in_view(p0, p1, p2, rot, near_z, far_z, tan_h, tan_v):
    """q_j = (R[0][j] p_0 + R[1][j] p_1) + R[2][j] p_2; rot is row-major [9]"""
    R = np.asarray(rot, np.float64).reshape(3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        q = [(R[0, j] * p0 + R[1, j] * p1) + R[2, j] * p2 for j in range(3)]
        return (q[2] > near_z) & (q[2] <= far_z) & (np.abs(q[0]) <= q[2] * tan_h) & (np.abs(q[1]) <= q[2] * tan_v)


def region(dims, resolution, box=None, frustum=None):
    """bool [H, W, L].  box = (lo [3], hi [3]) or None (also all six zero): the whole grid; frustum = (rot [9], near_z,
    far_z, tan_h, tan_v) or None"""
    L, W, H = dims
    R = np.ones((H, W, L), bool)
    if box is not None and (np.asarray(box[0]) != 0).any() | (np.asarray(box[1]) != 0).any():
        lo, hi = box
        R[:] = False
        R[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    if frustum is not None:
        px, py, pz = centres(dims, resolution)
        R &= in_view(px[None, None, :], py[None, :, None], pz[:, None, None], *frustum)
    return R


def dilate(occ, r):
    """D_r over a bool [H, W, L]: the maximum over every shift of at most r cells per axis of a zero-padded copy"""
    H, W, L = occ.shape
    pad = np.zeros((H + 2 * r, W + 2 * r, L + 2 * r), bool)
    pad[r:r + H, r:r + W, r:r + L] = occ
    out = np.zeros_like(occ)
    for dz in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                out |= pad[dz:dz + H, dy:dy + W, dx:dx + L]
    return out


def audit_agent(test_vt, truth_vt, dims, resolution, thr_test, thr_truth, r=0, box=None, frustum=None, slice_map=None,
                centre_test=None, centre_truth=None):
    """rows int32 [T_test, 8] of one agent, FIELDS' order"""
    vt, vg = volume(test_vt, dims), volume(truth_vt, dims)
    T_test, T_truth = vt.shape[0], vg.shape[0]
    if slice_map is None:
        slice_map = [t if t < min(T_test, T_truth) else -1 for t in range(T_test)]
    differ = (centre_test is not None and
              np.asarray(centre_test, np.float32).tobytes() != np.asarray(centre_truth, np.float32).tobytes())
    R = region(dims, resolution, box, frustum)
    rows = np.zeros((T_test, 8), np.int32)
    for t in range(T_test):
        s = int(slice_map[t])
        rows[t, 6] = s
        if s < 0:
            rows[t, 7] = SKIPPED
            continue
        if differ:
            rows[t, 7] = CENTRE
            continue
        ot, og = occupied(vt[t], thr_test), occupied(vg[s], thr_truth)
        rows[t, :6] = [R.sum(), (ot & R).sum(), (og & R).sum(), (ot & og & R).sum(), (ot & dilate(og, r) & R).sum(),
                       (og & dilate(ot, r) & R).sum()]
    return rows


def audit(tests, truths, dims, resolution, thr_test, thr_truth, r=0, box=None, cam_rot=None, frustum=None, slice_map=None,
          centres_test=None, centres_truth=None):
    """rows [n_agents, T_test, 8]; frustum = (near_z, far_z, tan_h, tan_v) with cam_rot [n, 9]"""
    out = []
    for a in range(len(tests)):
        fr = None if frustum is None else (cam_rot[a], *frustum)
        out.append(audit_agent(tests[a], truths[a], dims, resolution, thr_test, thr_truth, r, box, fr, slice_map,
                               None if centres_test is None else centres_test[a],
                               None if centres_truth is None else centres_truth[a]))
    return np.stack(out)


def brute_force_near(occ_a, occ_b, R, r):
    """|{c in occ_a & R : the smallest Chebyshev distance from c to a cell of occ_b is <= r}| by pairwise distances — a
    different algorithm from dilate()"""
    a = np.argwhere(occ_a & R)
    b = np.argwhere(occ_b)
    if len(a) == 0 or len(b) == 0:
        return 0
    n = 0
    for i in range(0, len(a), 256):
        d = np.abs(a[i:i + 256, None, :] - b[None, :, :]).max(axis=2).min(axis=1)
        n += int((d <= r).sum())
    return n


# ---- the bit rows and the layout, for the host program (tests/mapaudit_rules_host_test.cpp) ------------------------------------
def row_words(L):
    return (L + 63) // 64


def dilate_row_words(words, L, r):
    """an x-row given as 64-bit words (cell x = bit x % 64 of word x / 64) dilated by r: through a bool array"""
    bits = np.zeros(L + 2 * r, bool)
    for x in range(L):
        bits[r + x] = (int(words[x // 64]) >> (x % 64)) & 1
    out = np.zeros(L, bool)
    for d in range(2 * r + 1):
        out |= bits[d:d + L]
    res = [0] * row_words(L)
    for x in np.nonzero(out)[0]:
        res[x // 64] |= 1 << (int(x) % 64)
    return res


LDS_BYTES, LDS_RESERVED, DEFAULT_LAYERS = 160 * 1024, 1024, 4


def layout(L, W, H, r, slab_layers):
    """(row_words, layer_words, halo, layers, slabs, occ_layers, bytes): one region array of `layers` layers, and two
    (r = 0) or four (r > 0) arrays of layers + 2 r layers, 8-byte words, within 160 KB less 1 KB; `layers` is the largest
    count that fits, at most slab_layers (0: 4) and at most H"""
    rw = row_words(L)
    lw = W * rw
    size = lambda s: 8 * lw * (s + (4 if r > 0 else 2) * (s + 2 * r))  # noqa: E731
    want = min(slab_layers if slab_layers > 0 else DEFAULT_LAYERS, H)
    layers = max([s for s in range(1, want + 1) if size(s) <= LDS_BYTES - LDS_RESERVED], default=0)
    slabs = -(-H // layers) if layers else 0
    return rw, lw, r, layers, slabs, layers + 2 * r, size(layers) if layers else 0
