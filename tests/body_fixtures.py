"""Fixtures of the agent-body tests (CPU and GPU): worlds, bodies, cameras and rays.  Records are ring_fixtures' (n, 12)
rows, bodies (n, 3) centres.  Test infrastructure; not collected by pytest."""
import math

import numpy as np

import depth_bodies_reference as bref
import depth_ring_reference as ringref
import ring_fixtures as fx

BODY = (0.4, 0.4, 0.45)
HI_TIE = 0.6 + 0.5 * 0.45          # the top face of body 10 (centre z 0.6), in the header's arithmetic


def branch_scene(rows=48, cols=64):
    """Every branch of "agent bodies" in one world, four cameras, cx and cy whole numbers: with camera 0's exact matrix
    (d = (1, -xc, -yc)) the centre column has d_1 == 0 and the middle row d_2 == 0 exactly.
    Returns (records, camera, pos, rot, body_pos, cam_body) — cam_body is the table of the run that gives one; the other run
    passes none (camera a is carried by body a)."""
    rec = [
        fx.cylinder(3.0, 0.5, 0.5),                         # 0 behind body 4
        fx.cylinder(2.5, -0.8, 0.6),                        # 1 hides body 6
        fx.cylinder(1.5, -2.3, 0.6, z=0.0, h=2.0 * HI_TIE),  # 2 a stump whose top cap is z1 = 0 + HI_TIE: body 10's top face
        fx.ring(2.0, 0.5, 1.1, 0.5, h=0.06, q=fx.Q_TILT),   # 3 tilted, round body 4's centre: R 0.25 is outside the box along
                                                            #   its axes and inside it on the diagonals, so it crosses its faces
        fx.ring(2.0, 0.0, 1.0, 0.15),                       # 4 not a ring: rho >= R
        fx.cylinder(2.6, 3.4, 0.5),                         # 5 in camera 3's view
    ]
    poses = [fx.pose(0.0, 0.0, 1.0, 0.0),
             fx.pose(1.0, -2.0, 1.6, -0.4, pitch=1.1),      # looks down at the stump and body 10
             fx.pose(3.0, 0.3, 1.2, 2.0),                   # inside body 5
             fx.pose(4.013, 3.027, 1.31, -2.2)]
    pos = np.stack([p for p, _ in poses])
    rot = np.stack([R.reshape(9) for _, R in poses])
    ahead3 = rot[3].reshape(3, 3)[:, 2]                     # camera 3's optical axis
    bodies = [
        pos[0],                                             # 0 carries camera 0, which sits at its centre
        pos[1] - [0.1, 0.0, 0.05],                          # 1 carries camera 1 0.1 m ahead of and 0.05 above its centre: drawn,
                                                            #   its inner wall would fill the image
        pos[2],                                             # 2 carries camera 2
        pos[3] + 1.1 * ahead3 + [0.0, 0.0, 0.07],           # 3 camera 3's by default; with cam_body[3] = -1 it is IN its view
        [2.0, 0.5, 1.1],                                    # 4 in front of cylinder 0; the centre column misses it (d_1 == 0
                                                            #   outside the slab), the middle row does not (d_2 == 0 inside)
        [3.05, 0.35, 1.25],                                 # 5 camera 2 is inside it: inner wall
        [3.5, -1.12, 1.0],                                  # 6 wholly behind cylinder 1
        [5.05, 3.6, 1.0],                                   # 7 cut by max_depth: its side face runs from t = 4.85 to 5.25
        [1.5, -0.5, 0.225],                                 # 8 stands on the ground: lo_2 == 0.0 == ground_z
        [3.9, 0.1, 1.7],                                    # 9 straddles y = 0: d_1 == 0 inside the slab
        [1.6, -2.2, 0.6],                                   # 10 top face and stump 2's top cap in one plane: the tie
        [np.nan, 0.0, 1.0],                                 # 11 not a body
        [2.0, np.inf, 1.0],                                 # 12 not a body
        pos[3] + 2.0 * ahead3 + [0.3, 0.0, -0.2],           # 13 in camera 3's view in both runs
    ]
    c = fx.cam(rows, cols, 40.0 * cols / 64.0, float(cols // 2), float(rows // 2))
    return (np.array(rec, np.float64), c, pos, rot, np.array([np.asarray(b, np.float64) for b in bodies]),
            np.array([0, 1, 2, -1], np.int32))


def crowd_scene():
    """about 300 of each kind — bodies on a jittered lattice, thin cylinders, small rings — all within reach of one 24 x 32
    camera: more candidates than the 256-entry list in all three lists; rings and cylinders alternate in the world, so the
    flushes of their lists interleave.  Returns (records, camera, pos, rot, body_pos)."""
    rng = fx._Rng(0xB0D1E5)
    rings, cyls, bodies = [], [], []
    for _ in range(300):
        rho, ang = rng.uniform(0.8, 4.4), rng.uniform(-0.6, 0.6)
        q = [rng.uniform(-1, 1) for _ in range(4)]
        rings.append(fx.ring(rho * math.cos(ang), rho * math.sin(ang), rng.uniform(0.3, 1.8), rng.uniform(0.3, 0.8),
                             h=rng.uniform(0.03, 0.06), q=q))
        cyls.append(fx.cylinder(rng.uniform(1.0, 4.4), rng.uniform(-2.0, 2.0), rng.uniform(0.02, 0.08),
                                z=rng.uniform(0.5, 1.5), h=rng.uniform(0.5, 2.0)))
    for i in range(10):
        for j in range(6):
            for k in range(5):
                bodies.append([1.2 + 0.33 * i + rng.uniform(-0.05, 0.05), -1.5 + 0.6 * j + rng.uniform(-0.05, 0.05),
                               0.3 + 0.45 * k + rng.uniform(-0.05, 0.05)])
    rec = [r for pair in zip(rings, cyls) for r in pair]
    p, R = fx.pose(0.0, 0.0, 1.0, 0.05)
    return (np.array(rec, np.float64), fx.cam(24, 32, 20.0, 15.4, 11.7), p[None], R.reshape(1, 9),
            np.array(bodies, np.float64))


def permutation(n, seed):
    """a permutation of range(n) by SplitMix64 (Fisher-Yates)"""
    rng, perm = fx._Rng(seed), list(range(n))
    for i in range(n - 1, 0, -1):
        j = min(int(rng.uniform() * (i + 1)), i)
        perm[i], perm[j] = perm[j], perm[i]
    return np.array(perm)


def accuracy_views():
    """six 60 x 80 views of six bodies each, 1.5 .. 4 m away, for the comparison with the face-by-face algorithm:
    (bodies [6, 3], camera, p, rot)"""
    rng = fx._Rng(0xB0C5)
    out = []
    for _ in range(6):
        bodies = []
        for _ in range(6):
            dist, ang, dz = rng.uniform(1.5, 4.0), rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.4)
            bodies.append([dist * math.cos(ang), dist * math.sin(ang), 1.0 + dz])
        p, R = fx.pose(0.0, 0.0, 1.0, rng.uniform(-0.2, 0.2), pitch=rng.uniform(-0.2, 0.2))
        out.append((np.array(bodies), fx.cam(60, 80, 48.0, 39.3, 29.6, use_ground=False, max_depth=8.0), p, R.reshape(9)))
    return out


def named_rays():
    """(name, centre [3], size [3], p [3], d [3]) — one ray per branch of the slab rule"""
    B, o = list(BODY), [0.0, 0.0, 0.0]
    tiny = 5e-324
    rays = []
    for i in range(3):                                      # the entry face per axis and sign
        for sgn in (1.0, -1.0):
            c, d = [0.03, -0.02, 0.01], [0.011, -0.007, 0.013]
            c[i], d[i] = 2.0 * sgn, sgn
            rays.append((f"entry face axis {i} sign {sgn:+.0f}", c, B, o, d))
    rays += [
        ("d_0 == 0 inside the slab", [0.1, 2.0, 0.0], B, o, [0.0, 1.0, 0.05]),
        ("d_0 == 0 outside the slab", [0.3, 2.0, 0.0], B, o, [0.0, 1.0, 0.05]),
        ("d_1 == -0.0 inside the slab", [2.0, 0.1, 0.0], B, o, [1.0, -0.0, 0.02]),
        ("d_1 == 0 outside the slab", [2.0, -0.25, 0.0], B, o, [1.0, 0.0, 0.02]),
        ("d_2 == 0 on the slab's edge", [2.0, 0.0, 0.225], B, o, [1.0, 0.03, 0.0]),
        ("d_2 == 0 outside the slab", [2.0, 0.0, 0.3], B, o, [1.0, 0.03, 0.0]),
        ("two zero components", [0.1, -0.1, 3.0], B, o, [0.0, 0.0, 1.0]),
        ("camera inside the box: inner wall", [0.05, -0.03, 0.1], B, o, [1.0, 0.2, -0.1]),
        ("camera at the centre", o, B, o, [0.3, 1.0, 0.4]),
        ("box wholly behind", [-2.0, 0.0, 0.0], B, o, [1.0, 0.01, 0.02]),
        ("camera on a face looking out (tn < 0, tf == 0)", [-0.2, 0.0, 0.0], B, o, [1.0, 0.0, 0.0]),
        ("camera on a face looking in (tn == 0)", [0.2, 0.0, 0.0], B, o, [1.0, 0.0, 0.0]),
        # x in [0.75, 1.25], y (and z) in [0.625, 1.125], all dyadic: the ray leaves the x slab at t = 1.25 where it enters y
        ("tn == tf on an edge", [1.0, 0.875, 0.0], [0.5, 0.5, 0.5], o, [1.0, 0.5, 0.0]),
        ("tn == tf on a corner", [1.0, 0.875, 0.875], [0.5, 0.5, 0.5], o, [1.0, 0.5, 0.5]),
        ("just past the edge", [1.0, 0.875, 0.0], [0.5, 0.5, 0.5], o, [1.0, 0.4999999, 0.0]),
        ("overflowing quotients", [1e300, 0.0, 0.0], B, o, [1e-300, 1e-310, 1e-310]),
        ("overflowing quotients, subnormal d", [2.0, 0.1, 0.0], B, o, [1.0, tiny, -tiny]),
        ("overflowing extent", [1.7e308, 0.0, 0.0], [1e308, 0.4, 0.4], o, [1.0, 0.0, 0.0]),
        ("a miss beside the box", [2.0, 1.0, 0.0], B, o, [1.0, 0.1, 0.0]),
    ]
    return [(n, np.array(c, np.float64), np.array(s, np.float64), np.array(p, np.float64), np.array(d, np.float64))
            for n, c, s, p, d in rays]


NO_HIT_NAMES = ("outside", "behind", "looking out", "past", "miss")     # what a ray's name says about its answer
NOT_BODIES = [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [0.0, 0.0, -np.inf], [1e308, -1e308, 5e-324]]   # the last one is a body


def assert_branches(scene, want, cam_body, rings=True, min_body_px=15):
    """scene: branch_scene(); want: the reference's render_agents of it with `cam_body` (None or the table).  Asserts that
    every named branch occurs in the reference images, and that every camera has more than min_body_px body pixels."""
    rec, cam, pos, rot, bodies, _ = scene
    depth, _, unsupported, hit = want
    n = len(rec)
    own = bref.owners(len(pos), cam_body)
    d = [ringref.rays(cam, rot[a])[0] for a in range(len(pos))]

    def alone(j, a):
        return bref.body_t(bodies[j], BODY, pos[a], d[a])

    body_px = [(hit[a] >= n).sum() for a in range(len(pos))]
    assert all(v > min_body_px for v in body_px), body_px
    # not bodies (11, 12) are counted with the undrawn records: 4 always, 3 as well unless it is drawn
    assert (unsupported == (1 if rings else 2) + 2).all(), unsupported
    t4, t_c0 = alone(4, 0), bref.cylinder_t(rec[0], pos[0], d[0])
    assert ((hit[0] == n + 4) & (t4 < t_c0) & np.isfinite(t_c0)).sum() > 5                   # a body in front of a cylinder
    t6 = alone(6, 0)
    assert np.isfinite(t6).sum() > 5 and not (hit[0] == n + 6).any()                         # a body hidden behind one
    assert (hit[0][np.isfinite(t6)] == 1).all()
    t7 = alone(7, 0)
    assert (np.isfinite(t7) & (t7 > cam.max_depth)).sum() > 0 and (hit[0] == n + 7).sum() > 0   # cut by max_depth
    assert (hit[0][np.isfinite(t7) & (t7 > cam.max_depth)] != n + 7).all()
    assert (hit[2] == n + 5).all() and (depth[2] < 500).all() and (depth[2] > 0).all()       # camera 2 inside body 5
    for a in range(3):                                                                       # nobody sees its own body
        assert not (hit[a] == n + a).any()
    own1 = alone(1, 1)
    assert np.isfinite(own1).all() and (own1 < 0.5).all()                                    # (it would fill the image)
    mid_u, mid_v = cam.cols // 2, cam.rows // 2
    assert (d[0][1][:, mid_u] == 0).all() and (d[0][2][mid_v] == 0).all()                    # d_1 == 0, d_2 == 0 exactly
    assert not np.isfinite(t4[:, mid_u]).any() and np.isfinite(t4[mid_v]).any()              # 4: outside in y, inside in z
    t9 = alone(9, 0)
    assert np.isfinite(t9[:, mid_u]).any() and (hit[0][:, mid_u] == n + 9).any()             # 9: inside in y
    assert not np.isfinite(t9[mid_v]).any()                                                  #    outside in z
    assert (hit[0] == n + 8).sum() > 5 and (hit[0] == bref.HIT_GROUND).sum() > 50            # a body standing on the ground
    t10, t_c2 = alone(10, 1), bref.cylinder_t(rec[2], pos[1], d[1])
    tie = np.isfinite(t10) & (t10 == t_c2)
    assert tie.sum() > 5 and (hit[1][tie] == 2).all() and (hit[1] == n + 10).sum() > 5        # the cap-face tie: the record's
    if cam_body is None:
        assert not (hit[3] == n + 3).any() and (hit[3] == n + 13).sum() > min_body_px
    else:
        assert own[3] == -1 and (hit[3] == n + 3).sum() > min_body_px                        # carried by no body: 3 is drawn
    if rings:
        c, R, rho, _, _, nn = ringref.frame(rec[3])
        t_r = ringref.ray_hit(pos[0], d[0], c, R, rho, nn)[0]
        both = np.isfinite(t_r) & np.isfinite(t4)
        assert ((hit[0] == 3) & both).sum() > 10 and ((hit[0] == n + 4) & both).sum() > 10    # a ring crossing a body
    else:
        assert not (hit[0] == 3).any()
