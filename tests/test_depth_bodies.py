"""CPU: the host side of sogm_render_depth_swarm (include/sogm_abi.h "agent bodies"): declared, exported, bound, the struct's
size, sogm_render_depth's refusals first and then its own, no device -> SOGM_ERR_NO_DEVICE, the facade's renderDepthSwarm."""
import ctypes as C
import importlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _depth():
    return importlib.import_module("pred-occ-planner_amd.depth")


def test_struct_is_declared_bound_and_48_bytes(pop):
    abi = pop._abi
    assert C.sizeof(abi.SogmDepthBodies) == 48 == abi.DEPTH_BODIES_BYTES
    assert abi.SogmDepthBodies.size.offset == 16 and abi.SogmDepthBodies.n_bodies.offset == 40
    assert (abi.SOGM_HIT_GROUND, abi.SOGM_HIT_NONE) == (-1, -2)
    assert "sogm_render_depth_swarm" in abi.PROTOTYPES and len(abi.PROTOTYPES["sogm_render_depth_swarm"][1]) == 11
    assert hasattr(C.CDLL(abi.LIB_PATH), "sogm_render_depth_swarm")
    txt = open(os.path.join(ROOT, "include", "sogm_abi.h")).read()
    assert "int sogm_render_depth_swarm(const SogmWorld *world, const SogmDepthCamera *cam, const SogmDepthBodies *bodies" in txt
    assert "enum { SOGM_HIT_GROUND = -1, SOGM_HIT_NONE = -2 };" in txt and "} SogmDepthBodies;" in txt
    assert abi.SOGM_ABI_VERSION == 6
    assert callable(_depth().render_depth_swarm)
    ts = importlib.import_module("pred-occ-planner_amd.trajserver")
    assert callable(ts.TrajServer.body_positions)


def _bodies(pop, pos=0x7000, cam_body=None, size=(0.4, 0.4, 0.45), n=5):
    b = pop._abi.SogmDepthBodies()
    b.pos, b.cam_body, b.n_bodies = pos, cam_body, n
    b.size[:] = size
    return b


def _call(pop, world=True, cam=None, bodies="default", n=2, pos=0x1000, rot=0x2000, depth=0x3000, cloud=0x4000, hit=0x8000,
          other=0x5000, n_cyl=1):
    """stand-in addresses: every refusal happens before anything is read"""
    w = pop._abi.SogmWorld(None, None, 0x6000 if n_cyl > 0 else None, 0, 0, 256, n_cyl)
    c = cam if cam is not None else _depth().make_depth_camera(37, 53)
    b = _bodies(pop) if isinstance(bodies, str) else bodies
    return pop.lib().sogm_render_depth_swarm(C.byref(w) if world else None, C.byref(c), C.byref(b) if b is not None else None,
                                             n, pos, rot, depth, cloud, hit, other, None)


def test_invalid_arguments_are_refused_first(pop):
    bad = pop._abi.SOGM_ERR_INVALID_ARG
    # sogm_render_depth's refusals
    assert _call(pop, world=False) == bad
    assert pop.lib().sogm_last_error().startswith(b"sogm_render_depth_swarm")
    assert pop.lib().sogm_render_depth_swarm(C.byref(pop._abi.SogmWorld()), None, None, 1, 0x1000, 0x2000, 0x3000, None, None,
                                             0x5000, None) == bad
    for kw in ({"n": 0}, {"pos": None}, {"rot": None}, {"depth": None}, {"other": None}, {"n_cyl": -1}):
        assert _call(pop, **kw) == bad, kw
    for field, value in (("rows", 0), ("cols", 0), ("fx", 0.0), ("fy", -1.0), ("max_depth", 0.0), ("depth_scale", 0.0),
                         ("fx", float("nan")), ("max_depth", 65.536), ("depth_scale", 13107.2)):
        cam = _depth().make_depth_camera(37, 53)
        setattr(cam, field, value)
        assert _call(pop, cam=cam) == bad, (field, value)
        assert _call(pop, cam=cam, bodies=None) == bad, (field, value)
    w = pop._abi.SogmWorld(None, None, None, 0, 0, 256, 3)     # cylinders announced, none given
    cam = _depth().make_depth_camera(37, 53)
    assert pop.lib().sogm_render_depth_swarm(C.byref(w), C.byref(cam), None, 1, 0x1000, 0x2000, 0x3000, None, None, 0x5000,
                                             None) == bad
    # its own
    assert _call(pop, bodies=_bodies(pop, n=-1)) == bad
    assert pop.lib().sogm_last_error().startswith(b"sogm_render_depth_swarm")
    assert _call(pop, bodies=_bodies(pop, pos=None, n=3)) == bad
    for i in range(3):
        for v in (0.0, -0.4, float("nan"), float("inf")):
            size = [0.4, 0.4, 0.45]
            size[i] = v
            assert _call(pop, bodies=_bodies(pop, size=size)) == bad, (i, v)
            assert _call(pop, bodies=_bodies(pop, size=size, pos=None, n=0)) == bad, (i, v)   # also with no bodies


def test_valid_call_without_a_gpu_fails_loudly(pop):
    if pop.lib().sogm_device_count() > 0:
        return      # with a device the stand-in addresses would be used: tests/test_depth_bodies_gpu.py runs real calls
    no_dev = pop._abi.SOGM_ERR_NO_DEVICE
    assert _call(pop) == no_dev
    assert _call(pop, bodies=None, cloud=None, hit=None, n_cyl=0) == no_dev
    assert _call(pop, bodies=_bodies(pop, pos=None, n=0)) == no_dev
    assert _call(pop, bodies=_bodies(pop, cam_body=0x9000)) == no_dev
    with pytest.raises(pop.SogmError):
        pop._abi.check(no_dev, "sogm_render_depth_swarm")


def test_facade_render_depth_swarm_compiles_and_refuses(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "depth_bodies_facade_host_test")
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pred-occ-planner_amd", "host"),
                           os.path.join(ROOT, "tests", "depth_bodies_facade_host_test.cpp"), "-o", exe,
                           "-L", os.path.join(ROOT, "pred-occ-planner_amd"), "-lsogm_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "pred-occ-planner_amd")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "depth bodies facade host ok" in out.stdout
