"""FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233) for a batch of agents on the device: the
per-agent state records and the two launches of a tick behind the C ABI (sogm_fsm_init / sogm_fsm_inputs /
sogm_fsm_apply; the rules are csrc/sogm_fsm.hpp's).  PyTorch only provides the device buffers and the stream."""
import ctypes as C

import torch

from . import _abi
from ._abi import check, lib
from .sogm import _stream


def make_params(replan_duration=0.1, replan_start_time=0.02, goal_tolerance=1.0, new_plan_interval=1.0,
                replan_max_failures=5):
    """fsm/* of sim_fake.yaml:5-10 (and the 1.0 s of NEW_PLAN's time lapse, plan_manager.cpp:112)"""
    return _abi.SogmFsmParams(replan_duration, replan_start_time, goal_tolerance, new_plan_interval,
                              replan_max_failures, 0)


class FsmState:
    """n agents' machines: `state` uint8 [n, 24] (SogmFsmState records) and this tick's device tensors — `due` (bit 0
    NEW_PLAN plans, bit 1 REPLAN), `reached`, `pos_now` [n, 3] from inputs(); `pub` (_abi.FSM_PUB_*) and `hover_start`
    from apply().  Every call is one launch on the current stream."""

    def __init__(self, n, traj_start0, params=None, device="cuda"):
        self.n, self.prm = n, params if params is not None else make_params()
        self.state = torch.zeros((n, _abi.FSM_STATE_BYTES), dtype=torch.uint8, device=device)
        self.due = torch.zeros((n,), dtype=torch.int32, device=device)
        self.reached = torch.zeros((n,), dtype=torch.int32, device=device)
        self.pub = torch.zeros((n,), dtype=torch.int32, device=device)
        self.pos_now = torch.zeros((n, 3), dtype=torch.float64, device=device)
        self.hover_start = torch.zeros((n,), dtype=torch.float64, device=device)
        self.init(traj_start0)

    def init(self, traj_start0):
        check(lib().sogm_fsm_init(self.state.data_ptr(), self.n, float(traj_start0), _stream()), "sogm_fsm_init")

    def inputs(self, own, goals, stamp, hover, now, t_start, pva, poses):
        """the head of the tick: fills due / reached / pos_now and the caller's now, t_start, pva [n, 9], poses [n, 3]
        fp32; refreshes hover [n, 9]"""
        check(lib().sogm_fsm_inputs(C.byref(self.prm), self.state.data_ptr(), own.data_ptr(), goals.data_ptr(), self.n,
                                    float(stamp), hover.data_ptr(), now.data_ptr(), t_start.data_ptr(), pva.data_ptr(),
                                    poses.data_ptr(), self.pos_now.data_ptr(), self.due.data_ptr(),
                                    self.reached.data_ptr(), _stream()), "sogm_fsm_inputs")

    def apply(self, ok, safe, new, drone_ids, own, stamp, reached=None):
        """the state update from the tick's results and the publication into `own` (uint8 [n, 2064]); `reached`
        defaults to what inputs() computed"""
        reached = self.reached if reached is None else reached
        check(lib().sogm_fsm_apply(C.byref(self.prm), self.state.data_ptr(), self.due.data_ptr(), ok.data_ptr(),
                                   safe.data_ptr(), reached.data_ptr(), new.data_ptr(), drone_ids.data_ptr(),
                                   self.pos_now.data_ptr(), own.data_ptr(), self.pub.data_ptr(),
                                   self.hover_start.data_ptr(), self.n, float(stamp), _stream()), "sogm_fsm_apply")

    def flight_logs(self, n_ticks):
        """the per-tick logs of a flight under the FSM (planner.set_flight_fsm): zeroed device tensors [n_ticks, n]"""
        dev = self.state.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        return {"state": z((n_ticks, self.n, _abi.FSM_STATE_BYTES), torch.uint8), "due": z((n_ticks, self.n), torch.int32),
                "safe": z((n_ticks, self.n), torch.int32), "reached": z((n_ticks, self.n), torch.int32),
                "pub": z((n_ticks, self.n), torch.int32), "hover_start": z((n_ticks, self.n), torch.float64),
                "own": z((n_ticks, self.n, _abi.TRAJ_RECORD_BYTES), torch.uint8)}

    # views of the state records (device tensors sharing the records' memory)
    @property
    def traj_start(self):
        return self.state[:, 0:8].view(torch.float64).view(self.n)

    @property
    def status(self):
        return self.state[:, 8:12].view(torch.int32).view(self.n)

    @property
    def fail(self):
        return self.state[:, 12:16].view(torch.int32).view(self.n)

    @property
    def success(self):
        return self.state[:, 16:20].view(torch.int32).view(self.n)
