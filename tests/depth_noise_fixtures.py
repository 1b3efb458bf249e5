"""Fixtures of the sensor-noise tests (CPU and GPU): parameter sets, named pixels, the rendered branch scene and the tile-seam
image.  Cameras are ring_fixtures.cam namespaces (depth_scale 1000, max_depth 5), parameters depth_noise_reference.params
namespaces.  Test infrastructure; not collected by pytest."""
import functools

import numpy as np

import body_fixtures as bf
import depth_bodies_reference as bref
import depth_noise_reference as nref
import ring_fixtures as fx

SEED = 0x5067
# every term active: s = 0.004 z^2 + 0.003 z + 0.002 (0.117 m at 5 m), 5 % uniform dropout, half the pixels at a 0.15 m edge,
# nothing below 0.3 m
ACTIVE = dict(sigma=(0.002, 0.003, 0.004), p_drop=0.05, edge_jump=0.15, p_edge=0.5, min_depth=0.3)


def small_cam(rows, cols):
    return fx.cam(rows, cols, 40.0, float(cols // 2), float(rows // 2))


def negative_frame():
    """the first frame at SEED whose draw for pixel g = 0 has n < -0.5: (frame, n)"""
    for frame in range(64):
        n = float(nref.normal(nref.pixel_key(SEED, frame, 0)))
        if n < -0.5:
            return frame, n
    raise AssertionError("no negative draw in 64 frames")


def named_pixels():
    """(name, image [rows, cols], params, (v, u) of the named pixel, the counter it is built to add to) — the camera is
    small_cam of the image's shape"""
    P = nref.params
    nf, n_neg = negative_frame()
    flat = np.full((8, 8), 2000)
    board = np.where(np.add.outer(np.arange(8), np.arange(8)) % 2 == 0, 2000, 0)
    hole = np.full((3, 3), 2000)
    hole[1, 1] = 0
    line = [2000, 2000, 0, 2000, 2000]
    cases = [
        ("returns_out: a noised return", [[2000]], P(SEED, 3, sigma=(0.01, 0, 0)), (0, 0), "returns_out"),
        ("drop_uniform", [[2000]], P(SEED, 3, p_drop=1.0), (0, 0), "drop_uniform"),
        ("drop_edge: an edge through a no-return neighbour", [[2000, 0]], P(SEED, 3, edge_jump=0.1, p_edge=1.0), (0, 0),
         "drop_edge"),
        ("below_min", [[300]], P(SEED, 3, min_depth=0.5), (0, 0), "below_min"),
        ("beyond_max: n = +0.66 at 5 m", [[5000]], P(SEED, 3, sigma=(1.0, 0, 0)), (0, 0), "beyond_max"),
        ("q == 0 with min_depth == 0", [[1]], P(SEED, nf, sigma=(0.00075 / -n_neg, 0, 0)), (0, 0), "below_min"),
        ("zn negative", [[100]], P(SEED, nf, sigma=(1.0, 0, 0)), (0, 0), "below_min"),
        ("p_drop = 0 never drops", flat, P(SEED, 1, p_drop=0.0), (3, 3), "returns_out"),
        ("p_drop = 1 always drops", flat, P(SEED, 1, p_drop=1.0), (3, 3), "drop_uniform"),
        ("p_edge = 0 never drops", board, P(SEED, 1, edge_jump=0.1, p_edge=0.0), (2, 2), "returns_out"),
        ("p_edge = 1 always drops", board, P(SEED, 1, edge_jump=0.1, p_edge=1.0), (2, 2), "drop_edge"),
        ("a jump exactly equal to edge_jump is not an edge", [[2000, 2500]], P(SEED, 2, edge_jump=0.5, p_edge=1.0), (0, 0),
         "returns_out"),
        ("a jump one quantum above edge_jump is an edge", [[2000, 2501]], P(SEED, 2, edge_jump=0.5, p_edge=1.0), (0, 0),
         "drop_edge"),
        ("the same from the far side", [[2000, 2501]], P(SEED, 2, edge_jump=0.5, p_edge=1.0), (0, 1), "drop_edge"),
        ("corners and borders of a flat image are not edges", np.full((3, 3), 2000), P(SEED, 2, edge_jump=0.1, p_edge=1.0),
         (0, 0), "returns_out"),
        ("a corner beside a hole", hole, P(SEED, 2, edge_jump=0.1, p_edge=1.0), (2, 2), "drop_edge"),
        ("a border beside a hole", hole, P(SEED, 2, edge_jump=0.1, p_edge=1.0), (0, 1), "drop_edge"),
        ("1 x 1: no edge pixel", [[2000]], P(SEED, 2, edge_jump=0.1, p_edge=1.0), (0, 0), "returns_out"),
        ("1 x N beside the hole", [line], P(SEED, 2, edge_jump=0.1, p_edge=1.0), (0, 1), "drop_edge"),
        ("1 x N at the end", [line], P(SEED, 2, edge_jump=0.1, p_edge=1.0), (0, 4), "returns_out"),
        ("N x 1 beside the hole", [[d] for d in line], P(SEED, 2, edge_jump=0.1, p_edge=1.0), (3, 0), "drop_edge"),
        ("N x 1 at the end", [[d] for d in line], P(SEED, 2, edge_jump=0.1, p_edge=1.0), (0, 0), "returns_out"),
    ]
    return [(name, np.asarray(img, np.uint16), prm, px, counter) for name, img, prm, px, counter in cases]


@functools.lru_cache(maxsize=None)
def scene_frames(rows, cols, n_cams=4):
    """the branch scene (bodies, a ground, rings, no-return pixels) rendered by the numpy readings:
    (camera, depth [A, rows, cols] uint16, hit [A, rows, cols] int32)"""
    rec, cam, pos, rot, bodies, _ = bf.branch_scene(rows, cols)
    d, _, _, hit = bref.render_agents(rec, cam, pos[:n_cams], rot[:n_cams], bodies, None, rings=True)
    assert (d == 0).any() and (d != 0).any()
    return cam, d, hit


def active_params(frame=3, agent_base=0, seed=SEED):
    return nref.params(seed, frame, agent_base, **ACTIVE)


def seam_image(rows=67, cols=131, seed=0x5EA3):
    """seeded 5 x 7 blocks of constant depth, about one in six no-return; steps between neighbouring blocks of 0.05 m (below
    SEAM_JUMP) and of 0.15 m and more (above it): (image [rows, cols] uint16, edge_jump)"""
    rng = fx._Rng(seed)
    br, bc = -(-rows // 5), -(-cols // 7)
    levels = np.array([0, 1500, 1550, 1700, 1750, 2400], np.uint16)
    blocks = np.array([[levels[min(int(rng.uniform() * 6), 5)] for _ in range(bc)] for _ in range(br)], np.uint16)
    img = np.repeat(np.repeat(blocks, 5, axis=0), 7, axis=1)[:rows, :cols]
    return np.ascontiguousarray(img), 0.1
