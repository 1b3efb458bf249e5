"""The build's own depth camera (include/sogm_abi.h "depth camera"): every agent's depth frame of a sogm.World's
cylinders and ground plane, rendered on the device (sogm_render_depth) in the layouts the two perception front ends
read — the uint16 image GridMap.update takes and the camera-frame cloud SogmMap.filterPointCloud takes.
render_depth_swarm also draws the other vehicles of a swarm (sogm_render_depth_swarm, "agent bodies") and can say per pixel
what was hit.  add_depth_noise runs the sensor-noise pass (sogm_depth_noise, "sensor noise") over such frames.  No CPU path."""
import ctypes as C

import numpy as np
import torch

from ._abi import SOGM_DEPTH_RINGS, SogmDepthBodies, SogmDepthCamera, SogmDepthNoise, check, lib
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


def make_depth_noise(seed=0, frame=0, agent_base=0, sigma=(0.0, 0.0, 0.0), p_drop=0.0, edge_jump=0.0, p_edge=0.0, min_depth=0.0):
    """The parameters of include/sogm_abi.h "sensor noise": axial noise s = (sigma[2] z + sigma[1]) z + sigma[0] metres, uniform
    dropout p_drop, dropout p_edge at depth steps above edge_jump metres (0: none), no return below min_depth.  The default is
    the identity.  agent_base: the global index of local agent 0."""
    n = SogmDepthNoise()
    n.seed, n.frame, n.agent_base = int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame) & 0xFFFFFFFFFFFFFFFF, int(agent_base)
    n.sigma0, n.sigma1, n.sigma2 = (float(v) for v in sigma)
    n.p_drop, n.edge_jump, n.p_edge, n.min_depth = float(p_drop), float(edge_jump), float(p_edge), float(min_depth)
    return n


def add_depth_noise(cam, noise, depth, hit=None, want_cloud=True):
    """The noise pass over rendered frames: depth [A, rows, cols] int16 storage of the uint16 image (render_depth's), hit
    [A, rows, cols] int32 or None.  Returns new device tensors (depth in the same storage, cloud [A*rows*cols, 3] float32 with
    NaN where there is no return — None unless want_cloud —, hit with SOGM_HIT_NONE where the return was lost — None without
    hit —, counts [A, 6] int32: _abi.DEPTH_NOISE_COUNTERS).  The caller's tensors are untouched.  Stream-ordered, no
    synchronisation."""
    assert depth.dtype == torch.int16 and depth.is_cuda, (depth.dtype, depth.device)
    depth = depth.reshape(-1, cam.rows, cam.cols).contiguous()
    A, n, dev = int(depth.shape[0]), cam.rows * cam.cols, depth.device
    if hit is not None:
        assert hit.dtype == torch.int32 and hit.numel() == A * n, (hit.dtype, hit.shape)
        hit = hit.reshape(A, cam.rows, cam.cols).contiguous()
    out = torch.empty_like(depth)
    cloud = torch.empty((A * n, 3), dtype=torch.float32, device=dev) if want_cloud else None
    out_hit = torch.empty_like(hit) if hit is not None else None
    counts = torch.empty((A, 6), dtype=torch.int32, device=dev)
    check(lib().sogm_depth_noise(C.byref(cam), C.byref(noise), A, depth.data_ptr(), hit.data_ptr() if hit is not None else None,
                                 out.data_ptr(), cloud.data_ptr() if want_cloud else None,
                                 out_hit.data_ptr() if hit is not None else None, counts.data_ptr(), _stream()),
          "sogm_depth_noise")
    return out, cloud, out_hit, counts
