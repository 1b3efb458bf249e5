"""GPU: the batched Bezier QP kernels held to the termination contract of tests/qp_contract.py — k_qp through
sogm_bezier_qp_solve / _timed on every case of tests/golden/qp_optimum_independent.json (independent optima and LP
verdicts, tests/golden/make_qp_optimum_fixture.py), with fp64 and with fp32 residuals; the same cases in one mixed launch
against each case alone; the pipeline's own QPs (search -> corridors -> optimize) and those of the dataflow kernel
k_qp_flow (replan()), assembled again in numpy.  No scipy here: numpy, the fixture and the contract only."""
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import pytest

from helpers import hard_cases

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import qp_contract  # noqa: E402
from make_qp_fixture import assemble  # noqa: E402

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(HERE, "golden", "qp_optimum_independent.json")))
CASES = G["cases"]
MP = 16
# residual_fp32 = 1 computes each row's |Ax - z| / E and the norms in fp32: a few roundings of relative 2^-24 on both
# sides of the termination test, so the bound the contract derives may be missed by that much and no more
FP32_SLACK = 1e-6


def _problem(c):
    return assemble(c["start"], c["end"], c["t"], [np.array(p, float) for p in c["polys"]], c["vmax"], c["amax"])


def _planner(pop, A, fp32=0):
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    m = sogm.SogmMap(pop.config.make_spec("parity"), A)
    qs = pop.config.make_qp_settings()
    qs.residual_fp32 = fp32
    P = planner.SogmPlanner(m, pop.config.make_astar_params(), pop.config.make_planner_params(True), qs)
    return sogm, m, P


def _uniform(c, pp):
    """what sogm_bezier_qp_solve assembles: corridor_tau per piece, no end acceleration, the planner's limits"""
    return (all(t == pp.corridor_tau for t in c["t"]) and not np.any(np.array(c["end"])[2])
            and (c["vmax"], c["amax"]) == (pp.opt_max_vel, pp.opt_max_acc))


def _launch(sogm, P, cases, lim=None):
    """one launch, agent a solving cases[a] (agents beyond: no pieces); lim None = sogm_bezier_qp_solve, else the timed
    entry with these limits"""
    A, MF = P.A, P.pp.max_faces
    pva, end, tal = np.zeros((A, 9)), np.zeros((A, 9)), np.zeros((A, MP))
    polys, nf, npoly = np.zeros((A, MP, MF, 4)), np.zeros((A, MP), np.int32), np.zeros(A, np.int32)
    for a, c in enumerate(cases):
        M = c["M"]
        pva[a], end[a], tal[a, :M], npoly[a] = np.reshape(c["start"], 9), np.reshape(c["end"], 9), c["t"], M
        for i, p in enumerate(c["polys"]):
            polys[a, i, :len(p)], nf[a, i] = p, len(p)
    d = lambda x: sogm._dev(np.ascontiguousarray(x), x.dtype)
    if lim is None:
        q = P.optimize(d(pva), d(end[:, :6]), d(polys), d(nf), d(npoly))
    else:
        q = P.optimize_timed(d(pva), d(end), d(tal), d(polys), d(nf), d(npoly), lim[0], lim[1])
    return {k: v.cpu().numpy() for k, v in q.items()}


def _groups(cases, pp):
    """(limits or None for the untimed entry) -> cases"""
    out = {}
    for c in cases:
        key = None if _uniform(c, pp) else (c["vmax"], c["amax"])
        out.setdefault(key, []).append(c)
    return out


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64_residuals", "fp32_residuals"])
def test_every_fixture_case_meets_the_contract(pop, fp32):
    sogm, m, P = _planner(pop, len(CASES), fp32)
    qs = P.qs
    errors, by_status, worst = [], {}, {}
    for lim, group in _groups(CASES, P.pp).items():
        q = _launch(sogm, P, group, lim)
        for a, c in enumerate(group):
            st, it = int(q["status"][a]), int(q["iters"][a])
            Q, A, lb, ub = _problem(c)
            opt = {"x": c["x_star"], "f": c["f_star"], "active": c["active"]} if c["feasible"] else None
            rep = qp_contract.check(Q, A, lb, ub, st, q["cpts"][a], qs.eps_abs, qs.eps_rel, M=c["M"],
                                    t_star=c["t_star"], opt=opt, sanity=G["sanity"],
                                    slack_rel=FP32_SLACK if fp32 else 0.0)
            if rep["errors"]:
                errors.append((c["name"], st, it, rep["errors"]))
            by_status[st] = by_status.get(st, 0) + 1
            w = worst.setdefault(c["path"], {"ratio": 0.0, "dx": 0.0})
            w["ratio"] = max(w["ratio"], rep.get("ratio", 0.0))
            w["dx"] = max(w["dx"], rep.get("dx", 0.0))
    print(f"residual_fp32={fp32}: cases per status {dict(sorted(by_status.items()))}")
    for p, w in sorted(worst.items()):
        print(f"  {p:14s} worst viol/bound {w['ratio']:.3f}  worst |x - x*| {w['dx']:.2e}")
    assert not errors, errors
    P.close()
    m.close()


def test_mixed_launch_is_bit_identical_to_each_case_alone(pop):
    """the kernel picks its path per agent: one launch per limit pair holding every fixture case of that pair twice
    (register-resident beside HBM-scratch, feasible beside infeasible and max-iter), each slot against the same case
    solved in a launch of one agent — status, iteration count and coefficients bit for bit"""
    groups = {}
    for c in CASES:
        groups.setdefault((c["vmax"], c["amax"]), []).append(c)
    n = max(2 * len(g) for g in groups.values())
    sogm, m, P = _planner(pop, n)
    sogm1, m1, P1 = _planner(pop, 1)
    statuses, mixed = set(), 0
    for lim, group in groups.items():
        slots = group + group[::-1]
        q = _launch(sogm, P, slots, lim)
        for a, c in enumerate(slots):
            s = _launch(sogm1, P1, [c], lim)
            assert (q["status"][a], q["iters"][a]) == (s["status"][0], s["iters"][0]), (c["name"], a)
            assert np.array_equal(q["cpts"][a].view(np.uint64), s["cpts"][0].view(np.uint64)), (c["name"], a)
        st = {int(v) for v in q["status"][:len(slots)]}
        statuses |= st
        mixed += len(st) > 1 and len({c["path"] for c in group}) > 1
    print("statuses seen in the mixed launches:", sorted(statuses), "launches mixing paths and statuses:", mixed)
    assert mixed >= 1 and 1 in statuses and statuses & {-3, 3} and statuses & {2, -2}
    P1.close()
    m1.close()
    P.close()
    m.close()


def _setup(pop, A, seed):
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    spec = pop.config.make_spec("parity")
    sc, pva = hard_cases(pop, A, seed)
    recs = pop.scene.straight_records(sc)
    dev = sogm.upload_scene(sc)
    m = sogm.SogmMap(spec, A)
    m.updateMap(dev["cloud"], dev["cloud_range"], dev["cylinders"], dev["n_cyl"], dev["poses"], dev["stamps"])
    m.addOtherAgents(sogm._dev(recs), A, dev["ego_ids"])
    P = planner.SogmPlanner(m, pop.config.make_astar_params(), pop.config.make_planner_params(True),
                            pop.config.make_qp_settings())
    return sogm, sc, pva, dev, m, P


def _pipeline_check(pp, qs, pva, polys, nfaces, npoly, goal, cpts, status):
    """every agent with pieces: its QP assembled in numpy from the corridor outputs (corridor_tau per piece, end
    acceleration 0), the status / violation part of the contract"""
    errors, solved = [], 0
    for a in range(len(npoly)):
        M = int(npoly[a])
        if M <= 0:
            continue
        end = np.zeros((3, 3))
        end[0], end[1] = goal[a, :3], goal[a, 3:6]
        Q, A, lb, ub = assemble(pva[a].reshape(3, 3), end, [pp.corridor_tau] * M,
                                [polys[a, i, :nfaces[a, i]] for i in range(M)], pp.opt_max_vel, pp.opt_max_acc)
        rep = qp_contract.check(Q, A, lb, ub, int(status[a]), cpts[a], qs.eps_abs, qs.eps_rel, M=M)
        if rep["errors"]:
            errors.append((a, int(status[a]), rep["errors"]))
        solved += int(status[a]) in (1, 2)
    return errors, solved


@pytest.mark.parametrize("A,seed", [(8, 17), (12, 99), (6, 5), (10, 23), (16, 41)])
def test_pipeline_qps_meet_the_contract(pop, A, seed):
    sogm, sc, pva, dev, m, P = _setup(pop, A, seed)
    t_start = sc["stamps"] + 0.05
    d_pva, d_ts = sogm._dev(pva, np.float64), sogm._dev(t_start, np.float64)
    s = P.search(d_pva, sogm._dev(sc["goals"], np.float64), d_ts)
    c = P.generateCorridors(d_pva, d_ts, s["route"], s["route_len"])
    q = P.optimize(d_pva, c["goal"], c["polys"], c["nfaces"], c["npoly"])
    cn = {k: v.cpu().numpy() for k, v in c.items()}
    qn = {k: v.cpu().numpy() for k, v in q.items()}
    errors, solved = _pipeline_check(P.pp, P.qs, pva, cn["polys"], cn["nfaces"], cn["npoly"], cn["goal"], qn["cpts"],
                                     qn["status"])
    print(f"A={A} seed={seed}: statuses {qn['status'].tolist()}")
    assert not errors, errors
    assert solved > 0
    P.close()
    m.close()


@pytest.mark.parametrize("A,seed", [(8, 17), (6, 5), (12, 99)])
def test_replan_dataflow_qps_meet_the_contract(pop, A, seed):
    """k_qp_flow: the QP inputs and outputs of the last replan() read back with sogm_debug_planner_buffer"""
    import torch
    sogm, sc, pva, dev, m, P = _setup(pop, A, seed)
    t_start = sc["stamps"] + 0.05
    _, ok_d = P.replan(sogm._dev(pva, np.float64), sogm._dev(sc["goals"], np.float64), sogm._dev(t_start, np.float64),
                       dev["ego_ids"])
    torch.cuda.synchronize()
    ok = ok_d.cpu().numpy()
    lib = pop.lib()
    lib.sogm_debug_planner_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    MF = P.pp.max_faces
    shapes = {0: ((A, MP, MF, 4), np.float64), 1: ((A, MP), np.int32), 2: ((A,), np.int32), 3: ((A, 6), np.float64),
              6: ((A, MP * 15), np.float64), 8: ((A,), np.int32)}
    buf = {}
    for k, (shp, dt) in shapes.items():
        buf[k] = np.zeros(shp, dt)
        assert lib.sogm_debug_planner_buffer(P._p, k, buf[k].ctypes.data_as(C.c_void_p), buf[k].nbytes) == 0, k
    errors, solved = _pipeline_check(P.pp, P.qs, pva, buf[0], buf[1], buf[2], buf[3], buf[6], buf[8])
    print(f"A={A} seed={seed}: flow statuses {buf[8].tolist()} ok {ok.tolist()}")
    assert not errors, errors
    assert solved > 0
    assert all(buf[8][a] in (1, 2) for a in range(A) if ok[a])          # replan accepts status 1 and 2 only
    P.close()
    m.close()
