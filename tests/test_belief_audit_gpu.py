"""GPU: sogm_belief_audit (csrc/sogm_belief.hip) against the plain Python reading of the header
(tests/belief_audit_reference.py), count for count, out_pair_q too: 5 x 5, a shard (agent0 1, n_local 3 of 5) and 130 x 130
(nine workgroups of sixteen senders per receiver, the last with two).

The position evaluation: csrc/sogm_belief.hpp restates traj_eval_relative for host and device.  The host build of that
header equals the reading bit for bit (tests/test_belief_rules_host.py); here sogm_traj_eval's positions equal the reading
bit for bit, on the same records and times the audit samples — so the restatement and sogm_traj_eval agree through the
reading, and the kernel's counts, which are exact functions of those positions, equal the reading's."""
import importlib
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import belief_audit_reference as bref  # noqa: E402
from traj_noise_reference import RECORD  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = (0.05, 0.1, 0.5, 2.5, 4.0)                    # 2.5^2 = 6.25 = 1.5^2 + 2.0^2 exactly
LATER = 1000.0                                        # the start of the parked rows: every sample is clamped to it (s = 0)


@pytest.fixture(scope="module")
def links(pop):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return importlib.import_module("pred-occ-planner_amd.links")


def next_up(x):
    return struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", x))[0] + 1))[0]


def flights(ids, n_pieces, t_start, offset, seed):
    """smooth multi-piece records with unequal dyadic durations, one per entry of `ids` (arrays of equal length)"""
    ids = np.asarray(ids)
    rows = np.zeros(len(ids), RECORD)
    rows["drone_id"], rows["n_pieces"], rows["time_start"] = ids, n_pieces, t_start
    k = np.arange(16)
    rows["duration"] = 0.25 * (1 + (k[None, :] * 5 + ids[:, None] + seed) % 4)
    k = np.arange(80)[None, :]
    j = ids[:, None]
    pts = np.stack([0.3 * k + j, np.sin(0.21 * k + j + seed) * 2.0, 1.0 + 0.1 * np.cos(0.4 * k + seed) + 0 * j], axis=2)
    rows["cpts"] = (pts + np.asarray(offset, np.float64).reshape(-1, 1, 3)).reshape(len(ids), 240)
    return rows


def parked(j, pos):
    row = np.zeros((), RECORD)
    row["drone_id"], row["n_pieces"], row["time_start"] = j, 1, LATER
    row["duration"][0] = 0.5
    row["cpts"][:15] = np.tile(np.array(pos, np.float64), 5)
    return row


def make_case(n_total, agent0, n_local, compare_every=1, on_purpose=False):
    """(truth [n_total], views [n_local][n_total], t_now [n_local]): senders 0 mod 7 fly nothing (phantoms where believed),
    a pair is believed when (a * 7 + j) % compare_every == 0 and (a + 2 * j) % 11 != 0 (else unheard), believed rows are the
    truth moved by a pair's own offset between millimetres and metres, started a little later and cut to fewer pieces"""
    j = np.arange(n_total)
    truth = flights(j, 1 + j % 16, 10.0 + 0.25 * (j % 3), np.zeros((n_total, 3)), 0)
    truth["n_pieces"][j % 7 == 0] = 0
    views = np.zeros((n_local, n_total), RECORD)
    rng = np.random.default_rng(n_total * 100 + agent0)
    for al in range(n_local):
        a = agent0 + al
        size = 10.0 ** rng.uniform(-3.0, 0.7, n_total)
        off = rng.normal(size=(n_total, 3))
        off *= (size / np.linalg.norm(off, axis=1))[:, None]
        views[al] = flights(j, 1 + (j + a) % 16, 10.0 + 0.25 * ((j + a) % 4), off, a % 2)
        believed = ((a * 7 + j) % compare_every == 0) & ((a + 2 * j) % 11 != 0)
        views[al]["n_pieces"][~believed] = 0
    if on_purpose:                                    # receiver 0's d2 of sender 1 is 6.25 exactly, of sender 2 the next double up
        assert agent0 == 0 and n_total >= 5
        truth[1], views[0, 1] = parked(1, (0.0, 0.0, 0.0)), parked(1, (1.5, 2.0, 0.0))
        truth[2], views[0, 2] = parked(2, (0.0, 0.0, 1.0)), parked(2, (2.5, 0.0, 1.0 + 2.0 ** -25))
        views[1:, 1]["n_pieces"] = 0
        views[1:, 2]["n_pieces"] = 0
        nan = flights([3], 4, 10.0, np.zeros((1, 3)), 0)[0]
        nan["cpts"][7] = float("nan")
        views[1, 3] = nan                                                    # a NaN control point: bin 5, q clamped
        views[1, 4] = flights([4], 4, 10.0, [[3000.0, 0.0, 0.0]], 0)[0]      # far enough apart to clamp q
    t_now = 10.0 + 0.1 * np.arange(agent0, agent0 + n_local)                 # inside, and for late rows before the start
    return truth, views, t_now


_cache = {}


def reading(prm, key, truth, views, t_now, n_total, agent0, n_local):
    """the reading's answer, computed once per case; also asserts that no sample sits where a last-bit difference could move
    a count: within 1e-9 relative of an edge (the two built on purpose apart), within 1e-6 of a half-integer in mm^2"""
    if key not in _cache:
        d2s = []
        cnt, pq = bref.audit(prm, truth, views, t_now, n_total, agent0, n_local, on_sample=d2s.append)
        d2 = np.array([d for d in d2s if d == d and d not in (6.25, next_up(6.25))])
        for e in prm.edges:
            assert not (np.abs(d2 - e * e) <= 1e-9 * e * e).any(), e
        mm2 = d2[d2 < 1e6] * 1e6
        assert not (np.abs(mm2 - np.floor(mm2) - 0.5) <= 1e-6).any()
        _cache[key] = (cnt, pq, len(d2s))
    return _cache[key]


def run(links, prm, truth, views, t_now, agent0, calls=1):
    import torch
    n_local, n_total = views.shape
    dt = torch.from_numpy(truth.view(np.uint8).reshape(n_total, 2064).copy()).cuda()
    dv = torch.from_numpy(views.view(np.uint8).reshape(n_local, n_total, 2064).copy()).cuda()
    tn = torch.from_numpy(np.asarray(t_now, np.float64)).cuda()
    counters = torch.zeros((n_local, 12), dtype=torch.int64, device="cuda")
    pair_q = torch.full((n_local, n_total), -7, dtype=torch.int64, device="cuda")
    p = links.make_belief_params(prm.dt_sample, prm.edges, prm.n_samples)
    for _ in range(calls):
        links.belief_audit(p, dt, dv, tn, agent0, counters, pair_q)
    torch.cuda.synchronize()
    assert dt.cpu().numpy().tobytes() == truth.tobytes() and dv.cpu().numpy().tobytes() == views.tobytes()   # only read
    return counters.cpu().numpy(), pair_q.cpu().numpy()


CASES = {"5x5": (5, 0, 5, 1, True, 8), "shard": (5, 1, 3, 1, False, 16), "130x130": (130, 0, 130, 5, False, 3),
         "one sample": (7, 0, 7, 1, False, 1)}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_equals_the_reading(links, name):
    n_total, agent0, n_local, every, on_purpose, n_samples = CASES[name]
    prm = bref.params(0.2, EDGES, n_samples)
    truth, views, t_now = make_case(n_total, agent0, n_local, every, on_purpose)
    want, want_q, n = reading(prm, name, truth, views, t_now, n_total, agent0, n_local)
    got, got_q = run(links, prm, truth, views, t_now, agent0)
    tot = want.sum(axis=0)
    print(name, dict(zip(bref.COUNTERS, tot.tolist())), "samples read", n)
    assert np.array_equal(got, want), (got[:3], want[:3])
    assert np.array_equal(got_q, want_q)
    assert tot[0] > 0 and tot[1] > 0 and tot[3] == tot[0] * n_samples and (tot[4:10] > 0).sum() >= 4
    if n_total >= 7:
        assert tot[2] > 0                                                    # phantoms: senders that fly nothing but are believed
    if on_purpose:
        assert want_q[0, 1] == want_q[0, 2] == 6250000 and want[0][4 + 3] >= 1 and want[0][4 + 4] >= 1   # bins 3 and 4
        assert want_q[1, 3] == want_q[1, 4] == bref.Q_MAX and want[1][11] == bref.Q_MAX
    for al in range(n_local):
        assert want_q[al, agent0 + al] == -1


def test_counters_accumulate_and_runs_repeat(links):
    n_total, agent0, n_local, every, on_purpose, n_samples = CASES["5x5"]
    prm = bref.params(0.2, EDGES, n_samples)
    truth, views, t_now = make_case(n_total, agent0, n_local, every, on_purpose)
    want, want_q, _ = reading(prm, "5x5", truth, views, t_now, n_total, agent0, n_local)
    twice = want * 2
    twice[:, 11] = want[:, 11]                                               # a maximum
    got, got_q = run(links, prm, truth, views, t_now, agent0, calls=2)
    assert np.array_equal(got, twice) and np.array_equal(got_q, want_q)      # out_pair_q is this call's
    again, again_q = run(links, prm, truth, views, t_now, agent0, calls=2)
    assert np.array_equal(again, got) and np.array_equal(again_q, got_q)


def test_traj_eval_positions_equal_the_reading_bit_for_bit(links, pop):
    """sogm_traj_eval against the reading's position on the records and times the audit samples"""
    import torch
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    truth, views, t_now = make_case(5, 0, 5, 1, True)
    rows = np.concatenate([truth, views.reshape(-1), flights(np.arange(3), [1, 16, 17], 10.0, np.zeros((3, 3)), 2)])
    rows = rows[(rows["n_pieces"] > 0) & np.isfinite(rows["cpts"]).all(axis=1)]   # (a NaN's payload is not held to the reading)
    rows["n_pieces"] = np.minimum(rows["n_pieces"], 16)                     # sogm_traj_eval's contract
    times = []
    for r in rows:
        t0, total = float(r["time_start"]), float(np.sum(r["duration"][:int(r["n_pieces"])]))
        times.append([t0 - 1.0, t0, t0 + float(r["duration"][0]), t0 + 0.37, t0 + total, t0 + total + 2.0, 10.3, 11.7])
    times = np.array(times)
    recs = torch.from_numpy(rows.view(np.uint8).reshape(len(rows), 2064).copy()).cuda()
    for s in range(times.shape[1]):
        pva, ok = planner.traj_eval(recs, torch.from_numpy(np.ascontiguousarray(times[:, s])).cuda())
        got = pva.cpu().numpy()[:, :3]
        assert ok.cpu().numpy().all()
        want = np.array([bref.position(r, float(times[i, s])) for i, r in enumerate(rows)])
        assert got.tobytes() == want.tobytes(), s
