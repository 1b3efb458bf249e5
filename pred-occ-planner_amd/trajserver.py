"""Trajectory server (include/sogm_abi.h "trajectory server"): the reference's bezier_traj_server on the device — every
agent's look-ahead queue of 100 Hz samples and the position commands (position, velocity, acceleration, yaw, yaw_dot) it
publishes, from the tables the agents execute (sogm_traj_server_run).

TrajServer keeps the states and the rings on the device; run() queues one call per batch of executed tables and never
synchronises; commands / states() read the result back; camera_poses() turns commands into the camera poses
sogm_render_depth takes, on the device, and body_positions() into the box centres sogm_render_depth_swarm takes."""
import ctypes as C
import math

import numpy as np
import torch

from . import _abi
from .sogm import _dev, _stream

SAMPLE_DT = 0.01   # DELTA_T (bezier_traj_server.cpp:34)
# (pi, yaw_dot_max) of the two servers: bezier_traj_server.cpp:35-36 and bezier_traj_server_rotors.cpp:36, :78
YAW_CONSTANTS = {"launched": (3.14159265358979323846, 3.14159265358979323846), "rotors": (3.1415926, 0.05)}
CAM2BODY = (0.0, 0.0, 1.0, -1.0, 0.0, 0.0, 0.0, -1.0, 0.0)   # scene.camera_pose's forward-looking camera

COMMAND_DTYPE = np.dtype([("t_pub", "f8"), ("t_sample", "f8"), ("pos", "f8", (3,)), ("vel", "f8", (3,)),
                          ("acc", "f8", (3,)), ("yaw", "f8"), ("yaw_dot", "f8"), ("traj_id", "i4"), ("flags", "i4")])
POINT_DTYPE = np.dtype([("t", "f8"), ("pos", "f8", (3,)), ("vel", "f8", (3,)), ("acc", "f8", (3,)), ("yaw", "f8"),
                        ("yaw_dot", "f8")])
STATE_DTYPE = np.dtype([("ts", "f8"), ("te", "f8"), ("duration", "f8"), ("last_yaw", "f8"), ("last_yawdot", "f8"),
                        ("init_pos", "f8", (3,)), ("head", "i4"), ("size", "i4"), ("traj_id", "i4"), ("received", "i4"),
                        ("overflow", "i4"), ("reserved_", "i4", (3,)), ("traj", "u1", (_abi.TRAJ_RECORD_BYTES,))])
assert COMMAND_DTYPE.itemsize == _abi.POSITION_COMMAND_BYTES and POINT_DTYPE.itemsize == _abi.TRAJ_POINT_BYTES
assert STATE_DTYPE.itemsize == _abi.TRAJSRV_STATE_BYTES


def make_params(replan_threshold=0.5, yaw_mode=0, constants="launched", sample_dt=SAMPLE_DT):
    """replan_threshold: seconds of trajectory kept queued (the launch files use 0.02, 0.3, 0.5 and 1.2); yaw_mode 0: yaw 0
    is pushed (the launched server), 1: getYaw at every push; constants: "launched" / "rotors" or a (pi, yaw_dot_max) pair"""
    pi, rate = YAW_CONSTANTS[constants] if isinstance(constants, str) else constants
    prm = _abi.SogmTrajServerParams()
    prm.replan_threshold, prm.sample_dt, prm.yaw_pi, prm.yaw_dot_max = float(replan_threshold), float(sample_dt), pi, rate
    prm.yaw_mode = int(yaw_mode)
    return prm


class TrajServer:
    """The servers of rows [agent0, agent0 + n_local) of an n_total swarm, triggered at t_trigger.  init_pos [n_local][3]:
    where an agent stands before its first command; init_yaw [n_local] or None (0)."""

    def __init__(self, n_total, init_pos, t_trigger, agent0=0, n_local=None, init_yaw=None, prm=None, receive_delay=0.0,
                 device="cuda"):
        self.n_total, self.agent0 = int(n_total), int(agent0)
        self.n_local = int(n_local) if n_local is not None else self.n_total - self.agent0
        if not (0 <= self.agent0 and 1 <= self.n_local <= self.n_total - self.agent0):
            raise ValueError("agent0 / n_local out of range")
        self.prm = prm if prm is not None else make_params()
        self.receive_delay = float(receive_delay)
        self.state = torch.empty((self.n_local, _abi.TRAJSRV_STATE_BYTES), dtype=torch.uint8, device=device)
        self.queue = torch.empty((self.n_local, _abi.SOGM_TRAJSRV_QUEUE, _abi.TRAJ_POINT_BYTES), dtype=torch.uint8,
                                 device=device)
        pos = _dev(np.asarray(init_pos, np.float64).reshape(self.n_local, 3), np.float64, device)
        yaw = _dev(np.asarray(init_yaw, np.float64).reshape(self.n_local), np.float64, device) if init_yaw is not None else None
        _abi.check(_abi.lib().sogm_traj_server_init(self.state.data_ptr(), self.queue.data_ptr(), self.n_local,
                                                    float(t_trigger), pos.data_ptr(),
                                                    yaw.data_ptr() if yaw is not None else None, _stream()),
                   "sogm_traj_server_init")
        self.prev = None        # own copy of the last table seen (the next call's prev_table)
        self.next_tick = None
        self.cmd = None         # the last call's commands, uint8 [n_local][n_ticks * m][112]
        self.m = None

    def run(self, tables, t0, first_tick, period, received=None, prev_table=None):
        """Queue n_ticks ticks: the executed tables [n_ticks][n_total] (or one table [n_total]) of ticks first_tick ..,
        stamps t0 + tick * period.  received: int32 [n_ticks][n_local] (which records arrive) or None: a record arrives when
        its time_start differs from the previous table's — prev_table, by default the last table this object saw when the
        ticks continue the previous call's.  Returns the call's commands (device, uint8 [n_local][n_ticks * m][112]); no
        host synchronisation."""
        tables = tables if tables.dim() == 3 else tables.unsqueeze(0)
        tables = tables.contiguous()
        n_ticks = int(tables.shape[0])
        assert tables.shape[1:] == (self.n_total, _abi.TRAJ_RECORD_BYTES), tables.shape
        if prev_table is None and self.prev is not None and self.next_tick == first_tick:
            prev_table = self.prev
        if received is not None:
            received = received.to(torch.int32).reshape(n_ticks, self.n_local).contiguous()
        ratio = float(period) / self.prm.sample_dt if self.prm.sample_dt > 0 else float("nan")
        m = int(round(ratio)) if math.isfinite(ratio) else 0
        cmd = torch.empty((self.n_local, max(n_ticks * m, 1), _abi.POSITION_COMMAND_BYTES), dtype=torch.uint8,
                          device=tables.device)
        rc = _abi.lib().sogm_traj_server_run(
            C.byref(self.prm), self.state.data_ptr(), self.queue.data_ptr(), tables.data_ptr(),
            prev_table.data_ptr() if prev_table is not None else None,
            received.data_ptr() if received is not None else None, n_ticks, self.n_total, self.agent0, self.n_local,
            float(t0), int(first_tick), float(period), self.receive_delay, cmd.data_ptr(), _stream())
        _abi.check(rc, "sogm_traj_server_run")
        # a copy: the caller's buffer may be refilled by the next tick (publish mode alternates two tables)
        if self.prev is None:
            self.prev = torch.empty_like(tables[-1])
        self.prev.copy_(tables[-1])
        self.next_tick = first_tick + n_ticks
        self.cmd, self.m = cmd, m
        return cmd

    @property
    def commands(self):
        """the last call's commands as a numpy structured array [n_local][n_ticks * m] (synchronises)"""
        if self.cmd is None:
            return None
        torch.cuda.current_stream().synchronize()
        return self.cmd.cpu().numpy().view(COMMAND_DTYPE).reshape(self.cmd.shape[0], self.cmd.shape[1]).copy()

    def states(self):
        """(states [n_local], rings [n_local][256]) as numpy structured arrays (synchronises)"""
        torch.cuda.current_stream().synchronize()
        st = self.state.cpu().numpy().view(STATE_DTYPE).reshape(self.n_local).copy()
        rg = self.queue.cpu().numpy().view(POINT_DTYPE).reshape(self.n_local, _abi.SOGM_TRAJSRV_QUEUE).copy()
        return st, rg

    def camera_poses(self, sample=-1, cam2body=CAM2BODY, cam_offset=(0.0, 0.0, 0.0), cmd=None):
        """The camera poses of every agent at command `sample` of the last call (or of `cmd`, uint8 [n][k][112]):
        (pos [n][3], rot [n][9]) fp64 device tensors in sogm_render_depth's layouts.  No host synchronisation."""
        cmd = self.cmd if cmd is None else cmd
        n, k = int(cmd.shape[0]), int(cmd.shape[1])
        first = cmd[:, sample % k]
        pos = torch.empty((n, 3), dtype=torch.float64, device=cmd.device)
        rot = torch.empty((n, 9), dtype=torch.float64, device=cmd.device)
        c2b, off = (C.c_double * 9)(*[float(v) for v in cam2body]), (C.c_double * 3)(*[float(v) for v in cam_offset])
        rc = _abi.lib().sogm_camera_poses(first.data_ptr(), n, k, c2b, off, pos.data_ptr(), rot.data_ptr(), _stream())
        _abi.check(rc, "sogm_camera_poses")
        return pos, rot

    def body_positions(self, sample=-1, cmd=None):
        """The commanded positions of every agent at command `sample` of the last call (or of `cmd`, uint8 [n][k][112]): an
        fp64 device tensor [n][3], the body centres depth.render_depth_swarm takes.  A copy made by torch: no kernel of the
        library's, no host synchronisation."""
        cmd = self.cmd if cmd is None else cmd
        k = int(cmd.shape[1])
        off = COMMAND_DTYPE.fields["pos"][1]
        return cmd[:, sample % k, off:off + 24].contiguous().view(torch.float64)

    def body_velocities(self, sample=-1, cmd=None):
        """The commanded velocities (world axes) of every agent at command `sample`, body_positions' sibling: an fp64 device
        tensor [n][3], the body_vel SogmMap.filterPointCloudLabelled takes.  A copy made by torch: no kernel of the library's,
        no host synchronisation."""
        cmd = self.cmd if cmd is None else cmd
        k = int(cmd.shape[1])
        off = COMMAND_DTYPE.fields["vel"][1]
        return cmd[:, sample % k, off:off + 24].contiguous().view(torch.float64)
