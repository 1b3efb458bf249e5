"""GPU: sogm_depth_noise against the numpy reading of "sensor noise" (tests/depth_noise_reference.py), bit for bit — uint16
images equal, clouds equal as int32 where finite with the same NaN mask, hit images equal, counters equal, guard bytes behind
all four outputs untouched — at tile seams, at the identity, twice, as a shard, refused, with each optional argument left out,
handed to the two perception front ends, and through tools/eval_map.py."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import body_fixtures as bf  # noqa: E402
import depth_noise_fixtures as nf  # noqa: E402
import depth_noise_reference as nref  # noqa: E402
import ring_fixtures as fx  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
TAIL = 16


def _pop():
    return importlib.import_module("pred-occ-planner_amd")


def _mods():
    return (importlib.import_module("pred-occ-planner_amd.sogm"), importlib.import_module("pred-occ-planner_amd.depth"))


def _camera(cam):
    _, depth = _mods()
    return depth.make_depth_camera(cam.rows, cam.cols, cam.max_depth, cam.depth_scale, cam.ground_z, bool(cam.use_ground),
                                   fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy)


def _noise(prm, flags=0x70):
    _, depth = _mods()
    n = depth.make_depth_noise(prm.seed, prm.frame, prm.agent_base, (prm.sigma0, prm.sigma1, prm.sigma2), prm.p_drop,
                               prm.edge_jump, prm.p_edge, prm.min_depth)
    n.flags = flags                                                         # other bits are ignored
    return n


def _gpu(cam, prm, depth_in, hit_in=None, want_cloud=True, want_hit=True, hit_in_place=False, expect=0, override=None):
    """sogm_depth_noise into buffers with GUARD bytes of 0xA5 behind each (and a tail of -7 behind out_counts):
    (depth uint16 [A, rows, cols], cloud float32 [A*rows*cols, 3] or None, hit int32 [A, rows, cols] or None, counts [A, 6]).
    A refusal (expect != 0) must leave every output byte as it was; then the return is sogm_last_error()."""
    import torch
    pop = _pop()
    sogm, _ = _mods()
    depth_in = np.ascontiguousarray(depth_in, np.uint16).reshape(-1, cam.rows, cam.cols)
    A, n = len(depth_in), cam.rows * cam.cols
    in_d = torch.from_numpy(depth_in.view(np.int16)).cuda()
    want_hit = want_hit and hit_in is not None
    d_buf = torch.full((A * n * 2 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    c_buf = torch.full((A * n * 12 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    h_buf = torch.full((A * n * 4 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((A * 6 + TAIL,), -7, dtype=torch.int32, device="cuda")
    in_h = None
    if hit_in is not None:
        if hit_in_place:
            h_buf[:A * n * 4] = torch.from_numpy(np.ascontiguousarray(hit_in, np.int32).reshape(-1).view(np.uint8)).cuda()
            in_h = h_buf
        else:
            in_h = torch.from_numpy(np.ascontiguousarray(hit_in, np.int32).reshape(-1)).cuda()
    before_hit = h_buf.cpu().numpy().copy()
    args = dict(cam=C.byref(_camera(cam)), noise=C.byref(_noise(prm)), n=A, in_depth=in_d.data_ptr(),
                in_hit=in_h.data_ptr() if in_h is not None else None, out_depth=d_buf.data_ptr(),
                cloud=c_buf.data_ptr() if want_cloud else None, out_hit=h_buf.data_ptr() if want_hit else None,
                counts=counts.data_ptr())
    args.update(override or {})
    rc = pop.lib().sogm_depth_noise(args["cam"], args["noise"], args["n"], args["in_depth"], args["in_hit"], args["out_depth"],
                                    args["cloud"], args["out_hit"], args["counts"], sogm._stream())
    err = pop.lib().sogm_last_error()
    torch.cuda.synchronize()
    assert rc == expect, (rc, err)
    d_h, c_h, h_h, n_h = d_buf.cpu().numpy(), c_buf.cpu().numpy(), h_buf.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(in_d.cpu().numpy().view(np.uint16), depth_in), "the input image was written"
    if expect != 0:
        assert (d_h == 0xA5).all() and (c_h == 0xA5).all() and np.array_equal(h_h, before_hit) and (n_h == -7).all(), \
            "outputs written by a refused call"
        return err
    assert (d_h[A * n * 2:] == 0xA5).all() and (n_h[A * 6:] == -7).all(), "guard bytes written"
    assert (c_h[A * n * 12 if want_cloud else 0:] == 0xA5).all(), "guard bytes written behind (or into an unrequested) cloud"
    if want_hit:
        assert (h_h[A * n * 4:] == 0xA5).all(), "guard bytes written behind the hit image"
    else:
        assert np.array_equal(h_h, before_hit), "an unrequested hit image was written"
    if in_h is not None and not hit_in_place:
        assert np.array_equal(in_h.cpu().numpy(), np.asarray(hit_in, np.int32).reshape(-1)), "the input hit image was written"
    return (d_h[:A * n * 2].view(np.uint16).reshape(A, cam.rows, cam.cols),
            c_h[:A * n * 12].view(np.float32).reshape(-1, 3) if want_cloud else None,
            h_h[:A * n * 4].view(np.int32).reshape(A, cam.rows, cam.cols) if want_hit else None, n_h[:A * 6].reshape(A, 6))


def _same(got, want):
    d, cl, hit, counts = got
    print("pixels differing per agent:", [int((d[a] != want[0][a]).sum()) for a in range(len(d))],
          "counts", counts.tolist(), "want", want[3].tolist())
    assert np.array_equal(d, want[0])
    assert np.array_equal(counts, want[3])
    if cl is not None:
        assert nref.same_cloud(cl, want[1])
    if hit is not None:
        assert np.array_equal(hit, want[2])


# ---- 1. every term active, against the reading ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53), (48, 64)])
def test_every_term_active_three_cameras(shape):
    cam, depth, hit = nf.scene_frames(*shape, 3)
    prm = nf.active_params(frame=0)      # a frame whose draws push one of the few returns near 5 m beyond max_depth in both shapes
    want = nref.add_noise(cam, prm, depth, hit)
    assert (want[3].sum(axis=0) > 0).all(), "the scene does not take every branch"
    _same(_gpu(cam, prm, depth, hit), want)


# ---- 2. tile seams ----------------------------------------------------------------------------------------------------------
def test_edges_across_tile_seams():
    img, jump = nf.seam_image()
    assert img.shape == (67, 131)
    cam = nf.small_cam(*img.shape)
    edge = nref.edges(img, cam.depth_scale, jump) & (img != 0)
    keep = (img != 0) & ~edge
    assert edge.any(axis=1).all() and edge.any(axis=0).all() and keep.any(axis=1).all() and keep.any(axis=0).all()
    steps = np.abs(np.diff(img.astype(np.int64), axis=1))[(img[:, 1:] != 0) & (img[:, :-1] != 0)]
    assert ((steps > 0) & (steps < 1000 * jump)).any() and (steps > 1000 * jump).any()          # steps below and above edge_jump
    prm = nref.params(nf.SEED, 5, edge_jump=jump, p_edge=1.0)
    d, _, _, counts = _gpu(cam, prm, img[None])
    assert np.array_equal(d[0] == 0, (img == 0) | edge)                                          # the dropped set is the edge set
    assert np.array_equal(d[0][keep], img[keep])
    assert counts[0].tolist() == [int((img != 0).sum()), 0, int(edge.sum()), 0, 0, int(keep.sum())]
    _same((d, None, None, counts), nref.add_noise(cam, prm, img[None]))


# ---- 3. the identity --------------------------------------------------------------------------------------------------------
def test_all_zero_parameters_are_the_identity_on_a_rendered_frame():
    pop = _pop()
    sogm, depth = _mods()
    rec, cam, pos, rot, bodies, _ = bf.branch_scene(37, 53)
    world = sogm.World(np.zeros((0, 3), np.float32), fx.to_struct(pop._abi, rec), n_cyl=len(rec))
    dcam = _camera(cam)
    d, cl, _, _, hit = depth.render_depth_swarm(world, dcam, pos, rot, bodies, rings=True, want_hit=True)
    d2, cl2, hit2, counts = depth.add_depth_noise(dcam, depth.make_depth_noise(nf.SEED, 9), d, hit)
    assert d2.data_ptr() != d.data_ptr() and hit2.data_ptr() != hit.data_ptr()
    assert d2.cpu().numpy().tobytes() == d.cpu().numpy().tobytes()
    assert hit2.cpu().numpy().tobytes() == hit.cpu().numpy().tobytes()
    assert cl2.cpu().numpy().tobytes() == cl.cpu().numpy().tobytes()
    n = counts.cpu().numpy()
    assert np.array_equal(n[:, 0], (d != 0).sum(dim=(1, 2)).cpu().numpy()) and np.array_equal(n[:, 0], n[:, 5])
    assert (n[:, 1:5] == 0).all() and (n[:, 0] > 0).all()


# ---- 4. twice, and as a shard -----------------------------------------------------------------------------------------------
def test_twice_the_same_bytes_and_a_shard_draws_what_the_swarm_would():
    cam, depth, hit = nf.scene_frames(37, 53, 3)
    full = _gpu(cam, nf.active_params(), depth, hit)
    again = _gpu(cam, nf.active_params(), depth, hit)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))
    part = _gpu(cam, nf.active_params(agent_base=1), depth[1:3], hit[1:3])
    n = cam.rows * cam.cols
    assert np.array_equal(part[0], full[0][1:3]) and np.array_equal(part[2], full[2][1:3]) and np.array_equal(part[3], full[3][1:3])
    assert part[1].tobytes() == full[1][n:3 * n].tobytes()
    other = _gpu(cam, nf.active_params(frame=4), depth, hit)
    assert (other[0] != full[0]).mean() > 0.3


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_rule_and_writes_nothing():
    import torch
    pop = _pop()
    cam, depth, hit = nf.scene_frames(37, 53, 2)
    bad = pop._abi.SOGM_ERR_INVALID_ARG
    P = nf.active_params

    def refused(rule, prm=None, cam_field=None, **override):
        if cam_field:                                   # the buffers keep the scene's size
            c = _camera(cam)
            setattr(c, *cam_field)
            override["cam"] = C.byref(c)
        err = _gpu(cam, prm or P(), depth, hit, expect=bad, override=override)
        assert err.startswith(b"sogm_depth_noise: ") and rule in err, (rule, err)

    for key in ("cam", "noise", "in_depth", "out_depth", "counts"):
        refused(b"null pointer", **{key: None})
    refused(b"n_agents", n=0)
    for field, rule in ((("rows", 0), b">= 1"), (("cols", 0), b">= 1"), (("fx", 0.0), b"positive"), (("fy", -1.0), b"positive"),
                        (("max_depth", 0.0), b"positive"), (("depth_scale", 0.0), b"positive"), (("max_depth", 65.536), b"65535"),
                        (("cx", float("inf")), b"finite"), (("ground_z", float("nan")), b"finite")):
        refused(rule, cam_field=field)
    refused(b"out_hit without in_hit", in_hit=None)
    for field in ("sigma0", "sigma1", "sigma2", "p_drop", "edge_jump", "p_edge", "min_depth"):
        for v in (float("nan"), float("inf")):
            prm = P()
            setattr(prm, field, v)
            refused(b"finite", prm)
    for field in ("sigma0", "sigma1", "sigma2", "edge_jump", "min_depth"):
        prm = P()
        setattr(prm, field, -1e-12)
        refused(b"must be >= 0", prm)
    for field in ("p_drop", "p_edge"):
        for v in (-1e-12, 1.0 + 1e-12):
            prm = P()
            setattr(prm, field, v)
            refused(b"must be in [0, 1]", prm)
    refused(b"agent_base", P(agent_base=-1))
    # in place, and overlapping by one pixel: both buffers inside one allocation
    n = depth.size
    buf = torch.full((3 * n,), 0x5A5A, dtype=torch.int16, device="cuda")
    base = buf.data_ptr()
    for off_in, off_out in ((n, n), (n, 1), (1, n), (n, 2 * n - 1)):
        refused(b"overlaps in_depth", in_depth=base + 2 * off_in, out_depth=base + 2 * off_out)
    assert (buf.cpu().numpy() == 0x5A5A).all()


# ---- 6. optional arguments --------------------------------------------------------------------------------------------------
def test_each_optional_argument_left_out():
    cam, depth, hit = nf.scene_frames(37, 53, 3)
    prm = nf.active_params()
    want = nref.add_noise(cam, prm, depth, hit)
    _same(_gpu(cam, prm, depth, hit, want_cloud=False), want)                     # no cloud
    _same(_gpu(cam, prm, depth, None), want)                                      # no in_hit (and so no out_hit)
    _same(_gpu(cam, prm, depth, hit, want_hit=False), want)                       # in_hit given, out_hit not
    _same(_gpu(cam, prm, depth, None, want_cloud=False), want)                    # the image alone
    _same(_gpu(cam, prm, depth, hit, hit_in_place=True), want)                    # out_hit == in_hit


# ---- 7. hand-over -----------------------------------------------------------------------------------------------------------
def test_noised_frames_go_through_both_front_ends(pop):
    """render_depth_swarm -> add_depth_noise -> filterPointCloudLabelled -> sogm_update_dsp, and the uint16 image ->
    GridMap.update, at a tiny grid; with only dropouts on, the filter keeps no more leaves than without noise (a leaf needs a
    point, and the pass only removes points)"""
    import torch
    sogm, depth = _mods()
    gm = importlib.import_module("pred-occ-planner_amd.gridmap")
    dsp = importlib.import_module("pred-occ-planner_amd.dsp")
    rows, cols, A, cap = 60, 80, 2, 5000
    p = gm.make_gridmap_params(rows, cols)
    p.fx, p.fy, p.cx, p.cy = 387.0 / 8, 387.0 / 8, 320.0 / 8, 240.0 / 8
    p.map_size[:] = [12.0, 12.0, 3.0]
    p.local_update_range[:] = [4.0, 4.0, 2.0]
    p.local_map_margin = 5
    cam = depth.make_depth_camera(rows, cols, fx=p.fx, fy=p.fy, cx=p.cx, cy=p.cy, use_ground=False)
    rec = np.array([fx.cylinder(-1.37, 0.61, 0.5, vx=0.4), fx.cylinder(-0.4, 2.3, 0.6), fx.cylinder(1.9, -1.3, 0.5, vy=-0.3)])
    poses = [pop.scene.camera_pose(-4.013, 0.527, 1.031, 0.03), pop.scene.camera_pose(0.517, -4.021, 1.217, 1.47)]
    pos, rot = np.stack([c for c, _ in poses]), np.stack([R.reshape(9) for _, R in poses])
    yaw = np.array([0.03, 1.47])
    pos_d, rot_d = sogm._dev(pos, np.float64), sogm._dev(rot, np.float64)
    world = sogm.World(np.zeros((0, 3), np.float32), fx.to_struct(pop._abi, rec), n_cyl=len(rec))
    d, cl, rng, _, hit = depth.render_depth_swarm(world, cam, pos_d, rot_d, None, want_hit=True)
    noisy = depth.make_depth_noise(nf.SEED, 0, 0, **nf.ACTIVE)
    drops = depth.make_depth_noise(nf.SEED, 0, 0, p_drop=0.3, edge_jump=0.15, p_edge=0.5)
    dn, cln, hitn, counts = depth.add_depth_noise(cam, noisy, d, hit)
    dd, cld, hitd, counts_d = depth.add_depth_noise(cam, drops, d, hit)
    cn, cd = counts.cpu().numpy(), counts_d.cpu().numpy()
    assert (cn[:, 5] > 0).all() and (cd[:, 1] > 0).all() and (cd[:, 2] > 0).all() and (cd[:, 3:5] == 0).all()
    assert np.array_equal((dd != 0).sum(dim=(1, 2)).cpu().numpy(), cd[:, 5])
    kept = (dd != 0)
    assert torch.equal(dd[kept], d[kept])                                   # dropouts only: what is left is unchanged
    spec = pop.config.make_spec("parity", map_kind=pop._abi.SOGM_MAP_RISKVOXEL)
    m = sogm.SogmMap(spec, A)
    g = dsp.DspMap(m, dsp.make_dsp_params(spec.T), dsp.make_tables(5), max_points=cap)
    _, cnt_clean, _, _ = m.filterPointCloudLabelled(cl, hit, rng, world, None, 0.0, 0.15, cap)
    cnt_clean = cnt_clean.cpu().numpy().copy()
    _, cnt_drop, _, _ = m.filterPointCloudLabelled(cld, hitd, rng, world, None, 0.0, 0.15, cap)
    cnt_drop = cnt_drop.cpu().numpy().copy()
    pts, cnt, lab, _ = m.filterPointCloudLabelled(cln, hitn, rng, world, None, 0.0, 0.15, cap)
    print("filtered points: clean", cnt_clean.tolist(), "dropouts", cnt_drop.tolist(), "noisy", cnt.cpu().numpy().tolist())
    assert (cnt_drop <= cnt_clean).all() and (cnt_drop > 0).all() and (cnt.cpu().numpy() > 0).all()
    assert (lab.view(-1, 4)[:, 3] > 0).any()                                # moving records are still labelled
    base = torch.arange(A, dtype=torch.int32, device="cuda") * cap
    crange = torch.stack([base, base + cnt], dim=1).contiguous()
    quat = sogm._dev(np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], axis=1), np.float32)
    g.update(pts.view(-1, 3), lab.view(-1, 4), crange, sogm._dev(pos.astype(np.float32), np.float32), quat,
             sogm._dev(np.full(A, 1.0), np.float64))
    g.publish()
    grid = gm.GridMap(p, A)
    for _ in range(3):
        upd = grid.update(dn, pos_d, rot_d).cpu().numpy()
    occupied = []
    for a in range(A):
        _, inflated, _, err = grid.download(a)
        assert err[3] == 0, f"device error counters {err}"
        occupied.append(int((inflated > 0).sum()))
    print("gridmap updated:", upd.tolist(), "occupied cells:", occupied)
    assert (upd > 0).all() and all(o > 0 for o in occupied)
    torch.cuda.synchronize()
    grid.close()
    g.close()
    m.close()


# ---- 8. the tool ------------------------------------------------------------------------------------------------------------
TIMED = ("audit_ms_per_call", "audit_ms_all", "audit_TB_per_s", "audit_frac_of_8TB_per_s", "dense_clear_same_run")


def test_eval_map_without_flags_is_the_parents_and_with_full_dropout_sees_nothing():
    """tests/golden/eval_map_tiny.json holds a small configuration ("config": run()'s keywords — the tool's intrinsics are
    those of 480 x 640 frames, so it is small in agents and frames) and the line tools/eval_map.py printed for it before it had
    noise flags ("line"); the keys in TIMED are times and rates and are held only to be there"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        eval_map = importlib.import_module("eval_map")
    finally:
        sys.path.pop(0)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "eval_map_tiny.json")))
    TINY, want = golden["config"], golden["line"]
    assert eval_map.noise_settings(eval_map.parse_args([])) is None
    got = json.loads(json.dumps(eval_map.run(**TINY, noise=None)))
    assert list(got.keys()) == list(want.keys())
    for k in want:
        if k not in TIMED:
            assert got[k] == want[k], k
    assert sum(want["n_test"]) > 0, "the parent's perceived map is empty: the comparison says nothing"
    blind = eval_map.run(**TINY, noise=eval_map.noise_settings(eval_map.parse_args(["--drop", "1"])))
    c = blind["depth_noise"]["counters"]
    assert c["returns_out"] == 0 and c["returns_in"] == c["drop_uniform"] > 0
    assert list(blind.keys()) == list(want.keys()) + ["depth_noise"]
    assert sum(blind["n_test"]) == 0 and blind["n_truth"] == want["n_truth"]                     # an empty perceived map
