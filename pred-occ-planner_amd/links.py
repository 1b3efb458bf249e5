"""Radio links (include/sogm_abi.h "radio links"): every receiver's own table of the swarm's trajectories under per-message
delay, loss and radio range (sogm_link_deliver).

LinkModel keeps the ring of sent tables, the views, the held ticks and the counters on the device; deliver() queues one
tick and never synchronises; `views` is the [n_local][n_total] table the *_views entries take; counters() / held_ticks()
read the result back.

Message noise ("message noise": sogm_traj_noise) is what a sender broadcasts against what it flies: deliver(noise=...)
sends the table through it first.  The belief audit ("belief audit": sogm_belief_audit) scores the views against the table
the senders execute: audit_belief() / belief()."""
import ctypes as C

import numpy as np
import torch

from . import _abi
from .sogm import _stream

COUNTER_NAMES = _abi.LINK_COUNTER_NAMES
BELIEF_COUNTER_NAMES = _abi.BELIEF_COUNTER_NAMES


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


def make_noise(seed=0, loc=0.0, time=0.0, track=0.0, hold=0):
    """All defaults: no noise.  loc: the localisation bias' sigma in metres, one value or (x, y, z); time: the clock
    offset's in seconds; track: the tracking error's in metres; hold: ticks a localisation bias lasts, 0: the whole run."""
    prm = _abi.SogmTrajNoise()
    _abi.check(_abi.lib().sogm_traj_noise_default_params(C.byref(prm)), "sogm_traj_noise_default_params")
    loc = (loc,) * 3 if np.isscalar(loc) else tuple(loc)
    if len(loc) != 3:
        raise ValueError("noise: loc takes one value or three")
    prm.seed, prm.sigma_time, prm.sigma_track, prm.loc_hold = int(seed), float(time), float(track), int(hold)
    for c in range(3):
        prm.sigma_loc[c] = float(loc[c])
    return prm


def parse_noise(text):
    """'loc=S|X/Y/Z,time=S,track=S,hold=N,seed=N' (every part optional) -> SogmTrajNoise"""
    kw = {}
    for part in filter(None, (p.strip() for p in text.split(","))):
        key, _, val = part.partition("=")
        if key == "loc" and val:
            loc = tuple(float(v) for v in val.split("/"))
            if len(loc) not in (1, 3):
                raise ValueError(f"noise: loc takes one value or x/y/z, not {val!r}")
            kw["loc"] = loc * 3 if len(loc) == 1 else loc
        elif key in ("time", "track") and val:
            kw[key] = float(val)
        elif key == "hold" and val:
            kw["hold"] = int(val)
        elif key == "seed" and val:
            kw["seed"] = int(val, 0)
        else:
            raise ValueError(f"noise: unknown part {part!r}")
    return make_noise(**kw)


def format_noise(prm):
    """the text parse_noise reads back into the same parameters (floats by repr: exact)"""
    return (f"loc={'/'.join(repr(float(v)) for v in prm.sigma_loc)},time={float(prm.sigma_time)!r},"
            f"track={float(prm.sigma_track)!r},hold={int(prm.loc_hold)},seed={int(prm.seed):#x}")


def make_belief_params(dt_sample=None, edges=None, n_samples=None):
    """sogm_belief_default_params (8 samples 0.2 s apart, edges 0.05 0.1 0.2 0.5 1.0 m) with what is given replaced"""
    prm = _abi.SogmBeliefParams()
    _abi.check(_abi.lib().sogm_belief_default_params(C.byref(prm)), "sogm_belief_default_params")
    if dt_sample is not None:
        prm.dt_sample = float(dt_sample)
    if n_samples is not None:
        prm.n_samples = int(n_samples)
    if edges is not None:
        if len(edges) != 5:
            raise ValueError("belief: five edges")
        for i in range(5):
            prm.edges[i] = float(edges[i])
    return prm


def traj_noise(prm, tick, table, out=None, out_shift=None):
    """sogm_traj_noise: the table uint8 [n][2064] as its senders broadcast it at `tick` (out may be table; a new tensor
    when None).  out_shift: fp64 [n][4] for every row's shift x, y, z and tau.  No host synchronisation."""
    assert table.dtype == torch.uint8 and table.dim() == 2 and table.shape[1] == _abi.TRAJ_RECORD_BYTES and table.is_contiguous()
    if out is None:
        out = torch.empty_like(table)
    assert out.shape == table.shape and out.dtype == torch.uint8 and out.is_contiguous()
    if out_shift is not None:
        assert out_shift.shape == (table.shape[0], 4) and out_shift.dtype == torch.float64 and out_shift.is_contiguous()
    rc = _abi.lib().sogm_traj_noise(C.byref(prm), int(tick), table.data_ptr(), table.shape[0], out.data_ptr(),
                                    out_shift.data_ptr() if out_shift is not None else None, _stream())
    _abi.check(rc, "sogm_traj_noise")
    return out


def belief_audit(prm, truth, views, t_now, agent0, counters, out_pair_q=None):
    """sogm_belief_audit: views uint8 [n_local][n_total][2064] against truth uint8 [n_total][2064] at the receivers' times
    t_now fp64 [n_local]; adds into counters int64 [n_local][12].  No host synchronisation."""
    n_local, n_total = views.shape[0], views.shape[1]
    assert truth.shape == (n_total, _abi.TRAJ_RECORD_BYTES) and truth.dtype == torch.uint8 and truth.is_contiguous()
    assert views.shape[2] == _abi.TRAJ_RECORD_BYTES and views.dtype == torch.uint8 and views.is_contiguous()
    assert t_now.shape == (n_local,) and t_now.dtype == torch.float64 and t_now.is_contiguous()
    assert counters.shape == (n_local, _abi.SOGM_BELIEF_COUNTERS) and counters.dtype == torch.int64 and counters.is_contiguous()
    if out_pair_q is not None:
        assert out_pair_q.shape == (n_local, n_total) and out_pair_q.dtype == torch.int64 and out_pair_q.is_contiguous()
    rc = _abi.lib().sogm_belief_audit(C.byref(prm), truth.data_ptr(), views.data_ptr(), t_now.data_ptr(), n_total, int(agent0),
                                      n_local, counters.data_ptr(), out_pair_q.data_ptr() if out_pair_q is not None else None,
                                      _stream())
    _abi.check(rc, "sogm_belief_audit")
    return counters


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
        self.sent = self.sent_shift = self.belief_counts = self.belief_prm = None   # made by the first call that needs them
        self.reset()

    def reset(self):
        """nothing sent, nothing heard, counters 0; the next deliver() starts a new run of ticks"""
        rc = _abi.lib().sogm_link_init(C.byref(self.prm), self.n_total, self.n_local, C.byref(self.buffers), _stream())
        _abi.check(rc, "sogm_link_init")
        self.tick0 = self.next_tick = None
        if self.belief_counts is not None:
            self.belief_counts.zero_()

    def deliver(self, tick, table, pos=None, noise=None):
        """The delivery at `tick`: table uint8 [n_total][2064] is what every agent executes after the tick, pos fp64
        [n_total][3] where the agents are (needed when range > 0).  Ticks are consecutive from the first one.  Returns
        `views`; no host synchronisation.
        noise (a SogmTrajNoise): the table goes through sogm_traj_noise into a buffer of the model's own (`sent`, its
        shifts in `sent_shift`) and that is what the links carry; `table` is not touched and the positions stay the true
        ones."""
        tick = int(tick)
        if self.next_tick is not None and tick != self.next_tick:
            raise ValueError(f"links: tick {tick} does not follow tick {self.next_tick - 1}")
        if self.tick0 is None:
            self.tick0 = tick
        assert table.shape == (self.n_total, _abi.TRAJ_RECORD_BYTES) and table.dtype == torch.uint8, table.shape
        table = table.contiguous()
        if noise is not None:
            if self.sent is None:
                self.sent = torch.empty_like(table)
                self.sent_shift = torch.zeros((self.n_total, 4), dtype=torch.float64, device=table.device)
            table = traj_noise(noise, tick, table, self.sent, self.sent_shift)
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

    def audit_belief(self, truth, t_now, prm=None):
        """Score `views` against truth uint8 [n_total][2064], the table the senders execute, at the receivers' times t_now
        fp64 [n_local] (sogm_belief_audit); every call adds to the belief counters.  prm: a SogmBeliefParams (default:
        make_belief_params(), or the one given before).  No host synchronisation."""
        if prm is not None or self.belief_prm is None:
            self.belief_prm = prm if prm is not None else make_belief_params()
        if self.belief_counts is None:
            self.belief_counts = torch.zeros((self.n_local, _abi.SOGM_BELIEF_COUNTERS), dtype=torch.int64,
                                             device=self.views.device)
        t_now = t_now.to(torch.float64).reshape(self.n_local).contiguous()
        belief_audit(self.belief_prm, truth.contiguous(), self.views, t_now, self.agent0, self.belief_counts)

    def belief_counters(self):
        """int64 [n_local][12] (BELIEF_COUNTER_NAMES), over the audit_belief() calls so far (synchronises)"""
        torch.cuda.current_stream().synchronize()
        if self.belief_counts is None:
            return np.zeros((self.n_local, _abi.SOGM_BELIEF_COUNTERS), np.int64)
        return self.belief_counts.cpu().numpy().copy()

    def belief(self):
        """{name: total over the receivers}: max_q is their maximum, the rest are sums"""
        c = self.belief_counters()
        return {k: int(c[:, i].max() if k == "max_q" else c[:, i].sum()) for i, k in enumerate(BELIEF_COUNTER_NAMES)}
