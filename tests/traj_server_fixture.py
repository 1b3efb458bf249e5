"""tests/golden/traj_server_independent.json for the tests that hold the trajectory server to it (the host body in
test_traj_server_independent.py, the kernel in test_traj_server_gpu.py): the cases, their records as SogmTrajRecord bytes
and ONE comparison: what must be equal and the
tolerances of what need not be."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "traj_server_independent.json")))
CASES = FX["cases"]
REC_BYTES = 2064
REC_DTYPE = np.dtype([("drone_id", "i4"), ("n_pieces", "i4"), ("time_start", "f8"), ("duration", "f8", (16,)),
                      ("cpts", "f8", (240,))])
assert REC_DTYPE.itemsize == REC_BYTES

# pos / vel / acc: the project's tolerance in test_traj_eval_gpu.py and test_swarm_audit_gpu.py.  yaw: a 1e-12 velocity
# error over the fixture's smallest |v_xy| (>= 1e-3, checked below) turns the heading by at most 1e-9 rad; yaw_dot divides a
# yaw difference by 0.01 (2e-7).
TOL_PVA, TOL_YAW, TOL_YAW_DOT = 1e-12, 1e-9, 2e-7
assert FX["near_threshold"] == 0 and FX["min_vxy"] >= 1e-3


def record_bytes(rec, drone_id=0):
    """a fixture record (or None: no trajectory) as one SogmTrajRecord"""
    r = np.zeros((), REC_DTYPE)
    r["drone_id"] = drone_id
    if rec is not None:
        n = len(rec["duration"])
        r["n_pieces"], r["time_start"] = n, rec["time_start"]
        r["duration"][:n] = rec["duration"]
        r["cpts"][:n * 15] = np.asarray(rec["cpts"], np.float64).reshape(-1)
    return r


def case_tables(case):
    """(tables [n_ticks] of SogmTrajRecord: the latest record, repeated while nothing arrives; received [n_ticks] int32)"""
    rows, last = [], None
    for t in case["ticks"]:
        if t["record"] is not None:
            last = case["records"][t["record"]]
        rows.append(record_bytes(last))
    return np.stack(rows), np.asarray([t["received"] for t in case["ticks"]], np.int32)


def check(case, cmds, sizes, final, queue):
    """cmds: [n][13 doubles + traj_id + flags] rows as the fixture orders them; sizes: the queue size after every event, or
    None (the kernel reports no intermediate sizes); final: dict of the state's scalars; queue: [size][t, yaw, yaw_dot]"""
    name = case["name"]
    want = case["commands"]
    assert len(cmds) == len(want), (name, len(cmds), len(want))
    for i, (g, w) in enumerate(zip(cmds, want)):
        at = (name, i)
        assert g[0] == w[0] and g[1] == w[1], (at, "times", g[:2], w[:2])           # t_pub, t_sample: equal exactly
        assert int(g[13]) == w[13] and int(g[14]) == w[14], (at, "traj_id / flags", g[13:], w[13:])
        err = max(abs(a - b) for a, b in zip(g[2:11], w[2:11]))
        assert err <= TOL_PVA, (at, "pos / vel / acc", err)
        assert abs(g[11] - w[11]) <= TOL_YAW, (at, "yaw", g[11], w[11])
        assert abs(g[12] - w[12]) <= TOL_YAW_DOT, (at, "yaw_dot", g[12], w[12])
    if sizes is not None:
        assert list(sizes) == case["sizes"], (name, "queue sizes")
    f = case["final"]
    for key in ("ts", "te", "duration"):
        assert final[key] == f[key], (name, key, final[key], f[key])
    for key in ("size", "traj_id", "received", "overflow"):
        assert int(final[key]) == f[key], (name, key, final[key], f[key])
    assert abs(final["last_yaw"] - f["last_yaw"]) <= TOL_YAW, (name, "last_yaw")
    assert abs(final["last_yawdot"] - f["last_yawdot"]) <= TOL_YAW_DOT, (name, "last_yawdot")
    assert len(queue) == len(case["queue"]), (name, "live queue")
    for i, (g, w) in enumerate(zip(queue, case["queue"])):
        assert g[0] == w[0], (name, i, "queued sample time", g[0], w[0])
        assert abs(g[1] - w[1]) <= TOL_YAW and abs(g[2] - w[2]) <= TOL_YAW_DOT, (name, i, "queued yaw", g, w)
