"""CPU: the depth camera's numpy restatement (tests/depth_render_reference.py) against anchors worked out by hand, its
independence of culling, and the host side of sogm_render_depth: declared, exported, bound, argument checks first,
no device -> SOGM_ERR_NO_DEVICE, the facade's renderDepth."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_render_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = np.array([[3.0, 3.0, 0.0, 2.0, 1.0, 4.0]])   # {type, x, y, z, w, h}


def _cam(use_ground=1, ground_z=0.0, rows=480, cols=640, fx=387.0, fy=387.0, cx=320.0, cy=240.0):
    return types.SimpleNamespace(fx=fx, fy=fy, cx=cx, cy=cy, max_depth=5.0, depth_scale=1000.0, ground_z=ground_z,
                                 rows=rows, cols=cols, use_ground=use_ground)


def test_level_camera_in_front_with_ground(pop):
    pos, R = pop.scene.camera_pose(0.0, 0.0, 1.0, 0.0)
    d, cloud, other = ref.render(ONE, _cam(1), pos, R)
    assert other == 0 and d.dtype == np.uint16 and d.shape == (480, 640)
    assert d[240, 320] == 2500          # the side, 3 - 0.5 m ahead
    assert d[479, 320] == 1619          # the ground: 1 m below, yc = 239 / 387
    assert np.array_equal(np.nonzero(d[240])[0], np.arange(255, 386))
    # the cloud is the image's back-projection: NaN exactly where there is no return
    c = cloud.reshape(480, 640, 3)
    assert np.array_equal(np.isnan(c).all(axis=2), d == 0) and not np.isnan(c[d != 0]).any()
    assert c[240, 320, 2] == np.float32(2.5) and c[240, 320, 0] == 0 and c[240, 320, 1] == 0
    assert c[479, 320, 1] == np.float32(239.0 * 1.619 / 387.0)


def test_level_camera_in_front_without_ground(pop):
    pos, R = pop.scene.camera_pose(0.0, 0.0, 1.0, 0.0)
    d, _, _ = ref.render(ONE, _cam(0), pos, R)
    assert d[479, 320] == 0 and d[240, 320] == 2500
    assert int((d != 0).sum()) == 51157


def test_looking_down_sees_the_top_cap():
    R = np.array([[0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])   # columns x = (0,-1,0), y = (-1,0,0), z = (0,0,-1)
    d, _, _ = ref.render(ONE, _cam(1), [3.0, 0.0, 6.0], R)
    assert d[240, 320] == 2000 and d[0, 0] == 0     # the ground is 6 m away: out of range


@pytest.mark.parametrize("use_ground", [0, 1])
def test_inside_the_cylinder_sees_its_inner_wall(pop, use_ground):
    pos, R = pop.scene.camera_pose(3.0, 0.0, 1.0, 0.0)
    d, _, _ = ref.render(ONE, _cam(use_ground), pos, R)
    assert d[240, 320] == 500


def test_other_types_are_counted_not_drawn(pop):
    pos, R = pop.scene.camera_pose(0.0, 0.0, 1.0, 0.0)
    cam = _cam(1, rows=60, cols=80, fx=48.375, fy=48.375, cx=40.0, cy=30.0)
    ring = np.array([[2.0, 2.0, 0.0, 1.0, 2.0, 0.1]])
    d0, c0, n0 = ref.render(ONE, cam, pos, R)
    d1, c1, n1 = ref.render(np.concatenate([ONE, ring]), cam, pos, R)
    assert (n0, n1) == (0, 1) and ref.same(d1, c1, d0, c0)[0]


def test_culling_changes_nothing(pop):
    sc = pop.scene.make_scene(4, 4.95, 7)
    rec = ref.records(pop.scene.WorldTimeline(sc).cylinders(10))
    cam = _cam(0, rows=60, cols=80, fx=48.375, fy=48.375, cx=40.0, cy=30.0)
    for a in range(4):
        s, g = sc["starts"][a], sc["goals"][a]
        pos, R = pop.scene.camera_pose(s[0], s[1], 1.0, float(np.arctan2(g[1] - s[1], g[0] - s[0])))
        near = ref.in_range(rec, cam, pos)
        assert 0 < len(near) < len(rec)
        d_all, c_all, _ = ref.render(rec, cam, pos, R)
        d_near, c_near, _ = ref.render(near[::-1], cam, pos, R)      # (and in another order)
        ok, why = ref.same(d_near, c_near, d_all, c_all)
        assert ok, why
        assert int((d_all != 0).sum()) >= 300


def test_struct_is_declared_bound_and_72_bytes(pop):
    assert C.sizeof(pop._abi.SogmDepthCamera) == 72 == pop._abi.DEPTH_CAMERA_BYTES
    assert "sogm_render_depth" in pop._abi.PROTOTYPES
    assert hasattr(C.CDLL(pop._abi.LIB_PATH), "sogm_render_depth")
    txt = open(os.path.join(ROOT, "include", "sogm_abi.h")).read()
    assert "int sogm_render_depth(const SogmWorld *world, const SogmDepthCamera *cam, int n_agents," in txt
    depth = __import__("importlib").import_module("pred-occ-planner_amd.depth")
    cam = depth.make_depth_camera()
    assert (cam.rows, cam.cols, cam.fx, cam.fy, cam.cx, cam.cy) == (480, 640, 387.0, 387.0, 320.0, 240.0)
    assert (cam.max_depth, cam.depth_scale, cam.ground_z, cam.use_ground) == (5.0, 1000.0, 0.0, 1)


def _call(pop, world=True, cam=None, n=2, pos=0x1000, rot=0x2000, depth=0x3000, cloud=0x4000, other=0x5000, n_cyl=1):
    """stand-in addresses: every refusal happens before anything is read"""
    depth_mod = __import__("importlib").import_module("pred-occ-planner_amd.depth")
    w = pop._abi.SogmWorld(None, None, 0x6000 if n_cyl > 0 else None, 0, 0, 256, n_cyl)
    c = cam if cam is not None else depth_mod.make_depth_camera(37, 53)
    return pop.lib().sogm_render_depth(C.byref(w) if world else None, C.byref(c), n, pos, rot, depth, cloud, other, None)


def test_invalid_arguments_are_refused_first(pop):
    depth = __import__("importlib").import_module("pred-occ-planner_amd.depth")
    bad = pop._abi.SOGM_ERR_INVALID_ARG
    assert _call(pop, world=False) == bad
    assert pop.lib().sogm_last_error().startswith(b"sogm_render_depth")
    assert pop.lib().sogm_render_depth(C.byref(pop._abi.SogmWorld()), None, 1, 0x1000, 0x2000, 0x3000, None, 0x5000, None) == bad
    for kw in ({"n": 0}, {"pos": None}, {"rot": None}, {"depth": None}, {"other": None}, {"n_cyl": -1}):
        assert _call(pop, **kw) == bad, kw
    for field, value in (("rows", 0), ("cols", 0), ("fx", 0.0), ("fy", -1.0), ("max_depth", 0.0), ("depth_scale", 0.0),
                         ("fx", float("nan")), ("max_depth", 65.536), ("depth_scale", 13107.2)):
        cam = depth.make_depth_camera(37, 53)
        setattr(cam, field, value)
        assert _call(pop, cam=cam) == bad, (field, value)
    w = pop._abi.SogmWorld(None, None, None, 0, 0, 256, 3)     # cylinders announced, none given
    cam = depth.make_depth_camera(37, 53)
    assert pop.lib().sogm_render_depth(C.byref(w), C.byref(cam), 1, 0x1000, 0x2000, 0x3000, None, 0x5000, None) == bad


def test_valid_call_without_a_gpu_fails_loudly(pop):
    if pop.lib().sogm_device_count() > 0:
        return      # with a device the stand-in addresses would be used: tests/test_depth_render_gpu.py runs real calls
    no_dev = pop._abi.SOGM_ERR_NO_DEVICE
    assert _call(pop) == no_dev
    assert _call(pop, cloud=None, n_cyl=0) == no_dev
    cam = __import__("importlib").import_module("pred-occ-planner_amd.depth").make_depth_camera(37, 53, max_depth=4.0,
                                                                                               depth_scale=16383.75)
    assert _call(pop, cam=cam) == no_dev        # max_depth * depth_scale == 65535 exactly is allowed
    with pytest.raises(pop.SogmError):
        pop._abi.check(no_dev, "sogm_render_depth")


def test_facade_render_depth_compiles_and_refuses(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "depth_facade_host_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "depth_facade_host_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "depth facade host ok" in out.stdout
