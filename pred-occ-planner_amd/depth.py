"""The build's own depth camera (include/sogm_abi.h "depth camera"): every agent's depth frame of a sogm.World's
cylinders and ground plane, rendered on the device (sogm_render_depth) in the layouts the two perception front ends
read — the uint16 image GridMap.update takes and the camera-frame cloud SogmMap.filterPointCloud takes.  No CPU path."""
import ctypes as C

import numpy as np
import torch

from ._abi import SOGM_DEPTH_RINGS, SogmDepthCamera, check, lib
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
