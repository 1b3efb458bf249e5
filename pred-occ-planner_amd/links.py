"""Radio links (include/sogm_abi.h "radio links"): every receiver's own table of the swarm's trajectories under per-message
delay, loss and radio range (sogm_link_deliver).

LinkModel keeps the ring of sent tables, the views, the held ticks and the counters on the device; deliver() queues one
tick and never synchronises; `views` is the [n_local][n_total] table the *_views entries take; counters() / held_ticks()
read the result back."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from .sogm import _stream

COUNTER_NAMES = _abi.LINK_COUNTER_NAMES


def make_params(seed=0, p_loss=0.0, range=0.0, delay_min=0, delay_max=None, newest_wins=False):
    """All defaults: perfect links.  Delays in whole ticks, 0 <= delay_min <= delay_max <= 7 (delay_max defaults to
    delay_min); range in metres, 0: unlimited; newest_wins: an arrival older than the row held is dropped, where the
    reference's callback lets whatever arrives last overwrite."""
    prm = _abi.SogmLinkParams()
    _abi.check(_abi.lib().sogm_link_default_params(C.byref(prm)), "sogm_link_default_params")
    prm.seed, prm.p_loss, prm.range = int(seed), float(p_loss), float(range)
    prm.delay_min = int(delay_min)
    prm.delay_max = int(delay_min if delay_max is None else delay_max)
    prm.flags = _abi.SOGM_LINK_NEWEST_WINS if newest_wins else 0
    return prm


def parse_params(text):
    """'loss=P,delay=A..B,range=R,seed=N[,newest]' (every part optional; delay=A alone is A..A) -> SogmLinkParams"""
    kw = {}
    for part in filter(None, (p.strip() for p in text.split(","))):
        key, _, val = part.partition("=")
        if key == "newest" and not val:
            kw["newest_wins"] = True
        elif key == "loss":
            kw["p_loss"] = float(val)
        elif key == "range":
            kw["range"] = float(val)
        elif key == "seed":
            kw["seed"] = int(val, 0)
        elif key == "delay":
            lo, _, hi = val.partition("..")
            kw["delay_min"], kw["delay_max"] = int(lo), int(hi or lo)
        else:
            raise ValueError(f"link: unknown part {part!r}")
    return make_params(**kw)


class LinkModel:
    """The links into rows [agent0, agent0 + n_local) of an n_total swarm."""

    def __init__(self, n_total, agent0=0, n_local=None, prm=None, device="cuda"):
        self.n_total, self.agent0 = int(n_total), int(agent0)
        self.n_local = int(n_local) if n_local is not None else self.n_total - self.agent0
        if not (0 <= self.agent0 and 1 <= self.n_local <= self.n_total - self.agent0):
            raise ValueError("agent0 / n_local out of range")
        self.prm = prm if prm is not None else make_params()
        slots = max(int(self.prm.delay_max), 0) + 1
        rec = _abi.TRAJ_RECORD_BYTES
        self.ring_table = torch.empty((slots, self.n_total, rec), dtype=torch.uint8, device=device)
        self.ring_pos = torch.empty((slots, self.n_total, 3), dtype=torch.float64, device=device)
        self.views = torch.empty((self.n_local, self.n_total, rec), dtype=torch.uint8, device=device)
        self.held = torch.empty((self.n_local, self.n_total), dtype=torch.int32, device=device)
        self.counts = torch.empty((self.n_local, _abi.SOGM_LINK_COUNTERS), dtype=torch.int64, device=device)
        self.buffers = _abi.SogmLinkBuffers(self.ring_table.data_ptr(), self.ring_pos.data_ptr(), self.views.data_ptr(),
                                            self.held.data_ptr(), self.counts.data_ptr())
        self.tick0 = self.next_tick = None
        self.reset()

    def reset(self):
        """nothing sent, nothing heard, counters 0; the next deliver() starts a new run of ticks"""
        rc = _abi.lib().sogm_link_init(C.byref(self.prm), self.n_total, self.n_local, C.byref(self.buffers), _stream())
        _abi.check(rc, "sogm_link_init")
        self.tick0 = self.next_tick = None

    def deliver(self, tick, table, pos=None):
        """The delivery at `tick`: table uint8 [n_total][2064] is what every agent executes after the tick, pos fp64
        [n_total][3] where the agents are (needed when range > 0).  Ticks are consecutive from the first one.  Returns
        `views`; no host synchronisation."""
        tick = int(tick)
        if self.next_tick is not None and tick != self.next_tick:
            raise ValueError(f"links: tick {tick} does not follow tick {self.next_tick - 1}")
        if self.tick0 is None:
            self.tick0 = tick
        assert table.shape == (self.n_total, _abi.TRAJ_RECORD_BYTES) and table.dtype == torch.uint8, table.shape
        table = table.contiguous()
        if pos is not None:
            pos = pos.to(torch.float64).reshape(self.n_total, 3).contiguous()
        rc = _abi.lib().sogm_link_deliver(C.byref(self.prm), tick, self.tick0, table.data_ptr(),
                                          pos.data_ptr() if pos is not None else None, self.n_total, self.agent0,
                                          self.n_local, C.byref(self.buffers), _stream())
        _abi.check(rc, "sogm_link_deliver")
        self.next_tick = tick + 1
        return self.views

    def counters(self):
        """int64 [n_local][8] (COUNTER_NAMES), summed over the ticks so far (synchronises)"""
        torch.cuda.current_stream().synchronize()
        return self.counts.cpu().numpy().copy()

    def held_ticks(self):
        """int32 [n_local][n_total]: the send tick of every row held, -1: nothing heard (synchronises)"""
        torch.cuda.current_stream().synchronize()
        return self.held.cpu().numpy().copy()

    def totals(self):
        """{name: sum over the receivers}"""
        return {k: int(v) for k, v in zip(COUNTER_NAMES, self.counters().sum(axis=0))}
