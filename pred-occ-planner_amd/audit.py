"""Flight audit (include/sogm_abi.h "flight audit"): did two drones touch, did one fly through a cylinder, who reached
its goal and when — from the tables the agents execute, sampled at 100 Hz on the device (sogm_swarm_audit).

SwarmAudit keeps the accumulators and the event list on the device; add() queues one audit call per batch of executed
tables and never synchronises; report() / per_agent() read the result back."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from .sogm import _dev, _stream

BODY = (0.4, 0.4, 0.45)   # plan_manager/config/sim_fake.yaml:85-87
SAMPLE_DT = 0.01          # traj_server DELTA_T (bezier_traj_server.cpp:34)
GOAL_TOLERANCE = 1.0      # fsm/goal_tolerance (sim_fake.yaml:5)

_AGENT_DTYPE = np.dtype([("min_gap", "f8"), ("min_gap_time", "f8"), ("min_sep", "f8"), ("min_sep_time", "f8"),
                         ("goal_time", "f8"), ("first_collision_time", "f8"), ("path_length", "f8"),
                         ("last_pos", "f8", (3,)), ("min_gap_obstacle", "i4"), ("min_sep_agent", "i4"),
                         ("obstacle_samples", "i4"), ("agent_samples", "i4"), ("n_samples", "i4"), ("has_last", "i4")])
_EVENT_DTYPE = np.dtype([("t", "f8"), ("agent", "i4"), ("other", "i4"), ("kind", "i4"), ("reserved_", "i4")])
assert _AGENT_DTYPE.itemsize == _abi.AUDIT_AGENT_BYTES and _EVENT_DTYPE.itemsize == _abi.AUDIT_EVENT_BYTES


def cylinder_table(rows, moving=True):
    """(n, 5) rows {x, y, w, vx, vy} (scene / WorldTimeline) -> ctypes SogmCylinder array (type 3, z 2, h 4); a frozen world
    gets zero velocities"""
    from .scene import cylinders_to_struct
    r = np.asarray(rows, np.float64).reshape(-1, 5).copy()
    if not moving:
        r[:, 3:5] = 0.0
    return cylinders_to_struct(r), len(r)


class SwarmAudit:
    """Audits rows [agent0, agent0 + n_local) of an n_total swarm.  goals [n_local][3], fallback_pos [n_total][3] (where an
    agent hovers before its first trajectory), cylinders: (n, 5) rows {x, y, w, vx, vy} at t_obstacles, or a SogmCylinder
    ctypes array (type 3 only; with rings=True also type 2, audited as rings: include/sogm_abi.h "ring obstacles")."""

    def __init__(self, n_total, goals, fallback_pos, cylinders, t_obstacles, agent0=0, n_local=None, moving=True,
                 body=BODY, sample_dt=SAMPLE_DT, goal_tolerance=GOAL_TOLERANCE, event_capacity=4096, device="cuda",
                 rings=False):
        self.n_total, self.agent0 = int(n_total), int(agent0)
        self.n_local = int(n_local) if n_local is not None else self.n_total - self.agent0
        if not (0 <= self.agent0 and 1 <= self.n_local <= self.n_total - self.agent0):
            raise ValueError("agent0 / n_local out of range")
        if isinstance(cylinders, np.ndarray) or isinstance(cylinders, (list, tuple)):
            cyl, n_cyl = cylinder_table(cylinders, moving)
        else:
            cyl, n_cyl = cylinders, len(cylinders)
            if not moving:
                for c in cyl:
                    c.vx = c.vy = 0.0
        bad = [i for i in range(n_cyl) if cyl[i].type != 3 and not (rings and cyl[i].type == 2)]
        if bad:
            raise ValueError(f"SwarmAudit audits cylinders (type 3) only; obstacles {bad[:8]} are of another type"
                             if not rings else
                             f"SwarmAudit(rings=True) audits types 3 and 2 only; obstacles {bad[:8]} are of another type")
        self.n_cyl = n_cyl
        self.cyl = torch.frombuffer(bytearray(bytes(cyl)[:n_cyl * _abi.CYLINDER_BYTES]) or bytearray(_abi.CYLINDER_BYTES),
                                    dtype=torch.uint8).to(device)
        self.goals = _dev(np.asarray(goals, np.float64).reshape(self.n_local, 3), np.float64, device)
        self.fallback = _dev(np.asarray(fallback_pos, np.float64).reshape(self.n_total, 3), np.float64, device)
        self.prm = _abi.SogmAuditParams()
        self.prm.body[:] = [float(b) for b in body]
        self.prm.sample_dt, self.prm.goal_tolerance = float(sample_dt), float(goal_tolerance)
        self.prm.t_obstacles, self.prm.event_capacity = float(t_obstacles), int(event_capacity)
        self.prm.flags = _abi.SOGM_AUDIT_RINGS if rings else 0
        self.acc = torch.empty((self.n_local, _abi.AUDIT_AGENT_BYTES), dtype=torch.uint8, device=device)
        self.events = torch.zeros((max(int(event_capacity), 1), _abi.AUDIT_EVENT_BYTES), dtype=torch.uint8, device=device)
        self.n_events = torch.zeros((1,), dtype=torch.int32, device=device)
        self.prev = None            # own copy of the last table audited (the next call's prev_table)
        self.ticks = 0
        self.next_tick = None
        _abi.check(_abi.lib().sogm_audit_init_agents(self.acc.data_ptr(), self.n_local, _stream()), "sogm_audit_init_agents")

    def add(self, tables, t0, first_tick, period, prev_table=None):
        """Queue the audit of the executed tables [n_ticks][n_total] (or one table [n_total]) of ticks first_tick ..;
        stamps t0 + tick * period.  prev_table: the table before tables[0]; by default the last table this object saw when
        the ticks continue the previous call's.  No host synchronisation."""
        tables = tables if tables.dim() == 3 else tables.unsqueeze(0)
        tables = tables.contiguous()
        n_ticks = int(tables.shape[0])
        assert tables.shape[1:] == (self.n_total, _abi.TRAJ_RECORD_BYTES), tables.shape
        if prev_table is None and self.prev is not None and self.next_tick == first_tick:
            prev_table = self.prev
        rc = _abi.lib().sogm_swarm_audit(
            C.byref(self.prm), tables.data_ptr(), n_ticks, self.n_total,
            prev_table.data_ptr() if prev_table is not None else None, float(t0), int(first_tick), float(period),
            self.agent0, self.n_local, self.fallback.data_ptr(), self.goals.data_ptr(),
            self.cyl.data_ptr() if self.n_cyl else None, self.n_cyl, self.acc.data_ptr(),
            self.events.data_ptr() if self.prm.event_capacity > 0 else None, self.n_events.data_ptr(), _stream())
        _abi.check(rc, "sogm_swarm_audit")
        if n_ticks:
            # a copy: the caller's buffer may be refilled by the next tick (publish mode alternates two tables)
            if self.prev is None:
                self.prev = torch.empty_like(tables[-1])
            self.prev.copy_(tables[-1])
            self.ticks += n_ticks
            self.next_tick = first_tick + n_ticks

    def per_agent(self):
        """the accumulators as a numpy structured array [n_local] (synchronises)"""
        torch.cuda.current_stream().synchronize()
        return self.acc.cpu().numpy().view(_AGENT_DTYPE).reshape(self.n_local).copy()

    def event_list(self):
        """(events as a structured array in order, total colliding samples seen, truncated)"""
        torch.cuda.current_stream().synchronize()
        n = int(self.n_events.item())
        if n < 0:
            raise RuntimeError("sogm_swarm_audit met an obstacle of an unsupported type")
        kept = min(n, self.prm.event_capacity)
        ev = self.events[:kept].cpu().numpy().view(_EVENT_DTYPE).reshape(kept).copy()
        return ev, n, n > kept

    def report(self):
        a = self.per_agent()
        ev, n, trunc = self.event_list()
        arrived = a["goal_time"] >= 0
        clean = (a["agent_samples"] == 0) & (a["obstacle_samples"] == 0)
        i_sep, i_gap = int(np.argmin(a["min_sep"])), int(np.argmin(a["min_gap"]))
        return {
            "agents": self.n_local, "ticks": self.ticks, "samples": int(a["n_samples"][0]),
            "arrived": int(arrived.sum()),
            "mean_goal_time": float(a["goal_time"][arrived].mean()) if arrived.any() else None,
            "max_goal_time": float(a["goal_time"][arrived].max()) if arrived.any() else None,
            "success": int((arrived & clean).sum()),
            "agents_with_agent_collision": int((a["agent_samples"] > 0).sum()),
            "agents_with_obstacle_collision": int((a["obstacle_samples"] > 0).sum()),
            "agent_collision_samples": int(a["agent_samples"].sum()),
            "obstacle_collision_samples": int(a["obstacle_samples"].sum()),
            "min_separation": float(a["min_sep"][i_sep]), "min_separation_time": float(a["min_sep_time"][i_sep]),
            "min_separation_agents": [self.agent0 + i_sep, int(a["min_sep_agent"][i_sep])],
            "min_gap": float(a["min_gap"][i_gap]), "min_gap_time": float(a["min_gap_time"][i_gap]),
            "min_gap_agent": self.agent0 + i_gap, "min_gap_obstacle": int(a["min_gap_obstacle"][i_gap]),
            "mean_path_length": float(a["path_length"].mean()),
            "events": [(float(e["t"]), int(e["agent"]), int(e["other"]), int(e["kind"])) for e in ev],
            "n_events": n, "events_truncated": bool(trunc),
        }
