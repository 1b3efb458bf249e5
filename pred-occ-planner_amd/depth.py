"""The build's own depth camera (include/sogm_abi.h "depth camera"): every agent's depth frame of a sogm.World's
cylinders and ground plane, rendered on the device (sogm_render_depth) in the layouts the two perception front ends
read — the uint16 image GridMap.update takes and the camera-frame cloud SogmMap.filterPointCloud takes.
render_depth_swarm also draws the other vehicles of a swarm (sogm_render_depth_swarm, "agent bodies") and can say per pixel
what was hit.  No CPU path."""
import ctypes as C

import numpy as np
import torch

from ._abi import SOGM_DEPTH_RINGS, SogmDepthBodies, SogmDepthCamera, check, lib
from .gridmap import make_gridmap_params
from .sogm import _dev, _stream


def make_depth_camera(rows=480, cols=640, max_depth=5.0, depth_scale=1000.0, ground_z=0.0, use_ground=True,
                      fx=None, fy=None, cx=None, cy=None):
    """The intrinsics of make_gridmap_params (fx = fy = 387, cx = 320, cy = 240 at 480 x 640) unless given."""
    p = make_gridmap_params(rows, cols)
    cam = SogmDepthCamera()
    cam.fx, cam.fy = (p.fx if fx is None else fx), (p.fy if fy is None else fy)
    cam.cx, cam.cy = (p.cx if cx is None else cx), (p.cy if cy is None else cy)
    cam.max_depth, cam.depth_scale, cam.ground_z = float(max_depth), float(depth_scale), float(ground_z)
    cam.rows, cam.cols, cam.use_ground = int(rows), int(cols), 1 if use_ground else 0
    return cam


def render_depth(world, cam, cam_pos, cam_rot, want_cloud=True, rings=False):
    """world: sogm.World; cam_pos [A, 3], cam_rot [A, 9] (or [A, 3, 3]) fp64, row-major camera-to-world (scene.camera_pose).
    Returns device tensors (depth [A, rows, cols] int16 storage of the uint16 image, cloud [A*rows*cols, 3] float32 with
    NaN where there is no return — None unless want_cloud —, raw_range [A, 2] int32, unsupported [A] int32: the
    world's records that are not drawn: with rings=False every type other than 3; with rings=True the valid type-2 records
    are drawn as rings (include/sogm_abi.h "ring obstacles") and only what is left is counted).  Stream-ordered, no
    synchronisation."""
    if bool(cam.flags & SOGM_DEPTH_RINGS) != bool(rings):   # the caller's camera is not changed
        cam = SogmDepthCamera.from_buffer_copy(cam)
        cam.flags = (cam.flags | SOGM_DEPTH_RINGS) if rings else (cam.flags & ~SOGM_DEPTH_RINGS)
    dev = world.cylinders.device
    pos = _dev(np.asarray(cam_pos, np.float64) if not isinstance(cam_pos, torch.Tensor) else cam_pos, None, dev)
    rot = _dev(np.asarray(cam_rot, np.float64) if not isinstance(cam_rot, torch.Tensor) else cam_rot, None, dev)
    pos = pos.to(torch.float64).reshape(-1, 3).contiguous()
    rot = rot.to(torch.float64).reshape(-1, 9).contiguous()
    A = int(pos.shape[0])
    assert rot.shape[0] == A, (pos.shape, rot.shape)
    n = cam.rows * cam.cols
    depth = torch.empty((A, cam.rows, cam.cols), dtype=torch.int16, device=dev)
    cloud = torch.empty((A * n, 3), dtype=torch.float32, device=dev) if want_cloud else None
    unsupported = torch.empty((A,), dtype=torch.int32, device=dev)
    check(lib().sogm_render_depth(C.byref(world.c), C.byref(cam), A, pos.data_ptr(), rot.data_ptr(), depth.data_ptr(),
                                  cloud.data_ptr() if want_cloud else None, unsupported.data_ptr(), _stream()),
          "sogm_render_depth")
    begin = torch.arange(A, dtype=torch.int64, device=dev) * n
    raw_range = torch.stack([begin, begin + n], dim=1).to(torch.int32)
    return depth, cloud, raw_range, unsupported


def render_depth_swarm(world, cam, cam_pos, cam_rot, body_pos, cam_body=None, body=(0.4, 0.4, 0.45), rings=False,
                       want_cloud=True, want_hit=False):
    """render_depth with the other vehicles in view (include/sogm_abi.h "agent bodies", sogm_render_depth_swarm): body_pos
    [B, 3] fp64 box centres (TrajServer.body_positions; None or empty: no bodies), cam_body [A] int32 — the body that carries
    each camera and is not drawn for it; None: camera a is carried by body a, a value outside [0, B): by none —, body: the
    box's size, the flight audit's.  Returns render_depth's four and hit [A, rows, cols] int32 (None unless want_hit): per
    pixel the world's record index, n_cyl + the body's index, SOGM_HIT_GROUND or SOGM_HIT_NONE.  unsupported also counts
    the bodies whose centre is not finite.  The caller's camera is not changed.  Stream-ordered, no synchronisation."""
    if bool(cam.flags & SOGM_DEPTH_RINGS) != bool(rings):
        cam = SogmDepthCamera.from_buffer_copy(cam)
        cam.flags = (cam.flags | SOGM_DEPTH_RINGS) if rings else (cam.flags & ~SOGM_DEPTH_RINGS)
    dev = world.cylinders.device
    pos = _dev(np.asarray(cam_pos, np.float64) if not isinstance(cam_pos, torch.Tensor) else cam_pos, None, dev)
    rot = _dev(np.asarray(cam_rot, np.float64) if not isinstance(cam_rot, torch.Tensor) else cam_rot, None, dev)
    pos = pos.to(torch.float64).reshape(-1, 3).contiguous()
    rot = rot.to(torch.float64).reshape(-1, 9).contiguous()
    A = int(pos.shape[0])
    assert rot.shape[0] == A, (pos.shape, rot.shape)
    bodies = SogmDepthBodies()
    bodies.size[:] = [float(v) for v in body]
    bpos = bown = None       # (kept alive until the call is queued; the stream orders their release)
    if body_pos is not None:
        bpos = _dev(np.asarray(body_pos, np.float64) if not isinstance(body_pos, torch.Tensor) else body_pos, None, dev)
        bpos = bpos.to(torch.float64).reshape(-1, 3).contiguous()
        bodies.n_bodies = int(bpos.shape[0])
        bodies.pos = bpos.data_ptr() if bodies.n_bodies else None
    if cam_body is not None:
        bown = _dev(np.asarray(cam_body, np.int32) if not isinstance(cam_body, torch.Tensor) else cam_body, None, dev)
        bown = bown.to(torch.int32).reshape(-1).contiguous()
        assert bown.shape[0] == A, (bown.shape, A)
        bodies.cam_body = bown.data_ptr()
    n = cam.rows * cam.cols
    depth = torch.empty((A, cam.rows, cam.cols), dtype=torch.int16, device=dev)
    cloud = torch.empty((A * n, 3), dtype=torch.float32, device=dev) if want_cloud else None
    hit = torch.empty((A, cam.rows, cam.cols), dtype=torch.int32, device=dev) if want_hit else None
    unsupported = torch.empty((A,), dtype=torch.int32, device=dev)
    check(lib().sogm_render_depth_swarm(C.byref(world.c), C.byref(cam), C.byref(bodies), A, pos.data_ptr(), rot.data_ptr(),
                                        depth.data_ptr(), cloud.data_ptr() if want_cloud else None,
                                        hit.data_ptr() if want_hit else None, unsupported.data_ptr(), _stream()),
          "sogm_render_depth_swarm")
    begin = torch.arange(A, dtype=torch.int64, device=dev) * n
    raw_range = torch.stack([begin, begin + n], dim=1).to(torch.int32)
    return depth, cloud, raw_range, unsupported, hit
