"""GPU: the default lock-step tick on four hardware queues.  The dataflow replan runs its corridor stage and the end of every
agent's replan in ONE persistent kernel (k_worker_flow: finishing blocks at the lowest block indices, corridor blocks behind
them), and the context and the planner create a stream when they first launch on it: the default tick — three grids, sparse
reset, no pre-stamp — holds three streams beside the caller's.  Small shapes, nothing timed: the full-size ratio between
four and 32 queues is bench.py's and tests/test_residency_gpu.py's printout.
  * the fused kernel against the grouped-stream path (SOGM_FLOW=0: k_corridor_finalize, k_safe_after_opt, k_pack_records —
    code the fusion does not touch), with the default block counts and with both roles starved so that both loops of the
    kernel run more than one trip;
  * a pre-stamping flight (its gate reads the finishers' ticket word) against the flight that builds every map at the start
    of its tick;
  * the streams held, and the same flight in child processes with GPU_MAX_HW_QUEUES = 4 and 32."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, TICKS = 6, 8
# two finishing blocks for six agents, five corridor blocks for the 96 segment tickets of a tick
STARVED = {"finish_wgs": 2, "corridor_wgs": 5}


def _flight(tuning=None, ticks=TICKS, **kw):
    """ok flags and the record table, tick by tick, of the moving-world swarm"""
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False, tuning=tuning, **kw)
    out = []
    for _ in range(ticks):
        ok = sw.step().cpu().numpy().copy()
        out.append((ok, sw.own.cpu().numpy().copy(), sw.records_all().cpu().numpy().copy()))
    torch.cuda.synchronize()
    info = {"failures": sw.planner.flow_failures(), "pairs": sw.planner.corridor_pairs(), "counters": sw.planner.counters(),
            "streams": sw.planner.streams_held()}
    sw.close()
    return out, info


@pytest.fixture(scope="module")
def grouped(monkeypatch_module):
    """the reference of this module, flown once: the grouped-stream path"""
    monkeypatch_module.setenv("SOGM_FLOW", "0")  # read by sogm_planner_create
    out, info = _flight()
    monkeypatch_module.delenv("SOGM_FLOW")
    # every pair LP ran in k_corridor_finalize: this was not the dataflow replan
    assert info["pairs"]["eager"] == 0 and info["pairs"]["consumed"] == 0, info
    assert sum(int(x[0].sum()) for x in out) >= 2 * TICKS, [x[0].tolist() for x in out]
    return out, info


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.mark.parametrize("tuning", [None, STARVED], ids=["default", "starved"])
def test_worker_kernel_equals_the_grouped_path(pop, grouped, tuning):
    want, want_info = grouped
    got, info = _flight(tuning)
    assert info["failures"] == (0, 0), info
    assert info["pairs"]["eager"] > 0 and info["pairs"]["residue"] == 0, info  # the dataflow replan ran, and cleaned up
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x[0], y[0]), (k, x[0], y[0])   # ok flags
        assert np.array_equal(x[1], y[1]), k                 # the records the agents execute
        assert np.array_equal(x[2], y[2]), k                 # the swarm table
    for key in ("replan_ok", "fail_search", "fail_corridor", "fail_qp", "fail_unsafe"):  # where the replans ended
        assert info["counters"][key] == want_info["counters"][key], (key, info["counters"], want_info["counters"])


@pytest.mark.parametrize("tuning", [None, STARVED], ids=["default", "starved"])
def test_prestamping_flight_equals_the_plain_flight(pop, tuning):
    """as tests/test_pipelining_gpu.py::test_prestamp_flight_equals_the_plain_flight holds the pre-stamp to its lock-step
    rule: ok flags, the start states every tick planned from, records, table and every cell of the final grids"""
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    out = []
    for pre in (True, False):
        sw = driver.SwarmTick("parity", A, grids=3, prestamp=pre, tuning=tuning)
        assert sw.prestamp == pre
        oks, pvas, used = [], [], 0
        for _ in range(TICKS):
            used += int(pre and sw.compute.prestamp_pending())
            oks.append(sw.step().cpu().numpy().copy())
            pvas.append(sw.pva.cpu().numpy().copy())
        torch.cuda.synchronize()
        assert sw.planner.flow_failures() == (0, 0)
        out.append((oks, pvas, sw.records_all().cpu().numpy().copy(), sw.own.cpu().numpy().copy(),
                    [sw.map.download(a) for a in range(A)], used))
        sw.close()
    (oa, pa, ta, wa, ga, ua), (ob, pb, tb, wb, gb, ub) = out
    assert ua >= 5 and ub == 0
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob)) and sum(int(x.sum()) for x in oa) > 0
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert np.array_equal(ta, tb) and np.array_equal(wa, wb)
    assert all(np.array_equal(x, y) for x, y in zip(ga, gb))


def test_streams_are_created_when_first_used(pop):
    import torch
    driver = importlib.import_module("pred-occ-planner_amd.driver")
    sw = driver.SwarmTick("parity", A, moving_world=True, prestamp=False)
    held = [sw.planner.streams_held()]
    assert held[0] == 1, held          # the resets' side stream; the planner's two come with its first dataflow replan
    for _ in range(3):
        sw.step()
        held.append(sw.planner.streams_held())
    assert held[-1] == 3, held         # + the worker stream and the QP stream: with the caller's, four busy streams
    # the dense-clear mode's wide launch has a stream of its own
    sw.map.set_sparse_reset(False)
    for _ in range(2):
        sw.step()
        held.append(sw.planner.streams_held())
    assert held[-1] == 4, held
    sw.map.set_sparse_reset(True)
    for _ in range(2):
        sw.step()
        held.append(sw.planner.streams_held())
    torch.cuda.synchronize()
    assert sw.planner.flow_failures() == (0, 0)
    assert all(b >= a for a, b in zip(held, held[1:])), held   # never smaller than before
    sw.close()
    # a pre-stamp on a stream of its own (the default of a pre-stamping flight) is the other fifth stream
    sw = driver.SwarmTick("parity", A, grids=3, prestamp=True)
    held, used = [sw.planner.streams_held()], 0
    for _ in range(5):
        sw.step()
        used += int(sw.compute.prestamp_pending())
        held.append(sw.planner.streams_held())
    torch.cuda.synchronize()
    assert used >= 1 and held[-1] == 4 and all(b >= a for a, b in zip(held, held[1:])), (used, held)
    sw.close()
    # ... and on the resets' stream (prestamp_stream = 0) it is none
    sw = driver.SwarmTick("parity", A, grids=3, prestamp=True, tuning={"prestamp_stream": 0})
    for _ in range(5):
        sw.step()
    torch.cuda.synchronize()
    assert sw.planner.streams_held() == 3 and sw.planner.flow_failures() == (0, 0)
    sw.close()


_CHILD = r"""
import hashlib, importlib, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.environ["SOGM_REPO"])
driver = importlib.import_module("pred-occ-planner_amd.driver")
sw = driver.SwarmTick("parity", 6, moving_world=True, prestamp=False)
h = hashlib.sha256()
n_ok = 0
for _ in range(8):
    ok = sw.step().cpu().numpy()
    n_ok += int(ok.sum())
    h.update(ok.tobytes())
    h.update(sw.own.cpu().numpy().tobytes())
    h.update(sw.records_all().cpu().numpy().tobytes())
torch.cuda.synchronize()
print("LOCKSTEP " + json.dumps({"digest": h.hexdigest(), "ok": n_ok, "failures": list(sw.planner.flow_failures()),
                                "streams": sw.planner.streams_held(), "queues": os.environ.get("GPU_MAX_HW_QUEUES")}))
sw.close()
"""


@pytest.mark.own_device
def test_four_and_thirty_two_hardware_queues_fly_the_same_records(pop):
    def fly(queues):
        # in the child's environment before its Python starts: the variable is read once, when HIP initialises
        env = dict(os.environ, SOGM_REPO=ROOT, GPU_MAX_HW_QUEUES=queues)
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LOCKSTEP ")]
        assert r.returncode == 0 and lines, (queues, r.stdout[-1500:], r.stderr[-3000:])
        return json.loads(lines[-1][9:])
    four, many = fly("4"), fly("32")
    assert four["queues"] == "4" and many["queues"] == "32"
    for f in (four, many):
        assert f["failures"] == [0, 0] and f["streams"] == 3 and f["ok"] > 0, f
    assert four["digest"] == many["digest"], (four, many)
