"""GPU parity: batched Bezier QP (assembly + OSQP-algorithm ADMM) and the full replan chain vs the
CPU oracle.  Trajectory coefficients within 1e-4 (north_star tolerance; observed ~1e-9), same
solver status and iteration count."""
import importlib

import numpy as np
import pytest

from helpers import hard_cases, oracle_grids

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _setup(pop, A, seed, fake=True):
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    spec = pop.config.make_spec("parity")
    sc, pva = hard_cases(pop, A, seed)
    recs = pop.scene.straight_records(sc)
    dev = sogm.upload_scene(sc)
    m = sogm.SogmMap(spec, A)
    m.updateMap(dev["cloud"], dev["cloud_range"], dev["cylinders"], dev["n_cyl"], dev["poses"], dev["stamps"])
    m.addOtherAgents(sogm._dev(recs), A, dev["ego_ids"])
    ap, pp, qs = pop.config.make_astar_params(), pop.config.make_planner_params(fake), pop.config.make_qp_settings()
    P = planner.SogmPlanner(m, ap, pp, qs)
    return sogm, planner, spec, sc, pva, recs, dev, m, ap, pp, qs, P


@pytest.mark.parametrize("A,seed", [(8, 17), (12, 99)])
def test_qp_matches_oracle(pop, orc, A, seed):
    sogm, planner, spec, sc, pva, recs, dev, m, ap, pp, qs, P = _setup(pop, A, seed)
    t_start = sc["stamps"] + 0.05
    d_pva, d_ts = sogm._dev(pva, np.float64), sogm._dev(t_start, np.float64)
    s = P.search(d_pva, sogm._dev(sc["goals"], np.float64), d_ts)
    c = P.generateCorridors(d_pva, d_ts, s["route"], s["route_len"])
    q = P.optimize(d_pva, c["goal"], c["polys"], c["nfaces"], c["npoly"])
    cn = {k: v.cpu().numpy() for k, v in c.items()}
    qn = {k: v.cpu().numpy() for k, v in q.items()}
    worst = 0.0
    for a in range(A):
        M = int(cn["npoly"][a])
        assert M > 0
        goal = np.concatenate([cn["goal"][a], np.zeros(3)])
        st, x, it = orc.qp_solve(pva[a], goal, [pp.corridor_tau] * M, cn["polys"][a], cn["nfaces"][a],
                                 pp.max_faces, pp.opt_max_vel, pp.opt_max_acc, qs)
        assert qn["status"][a] == st and qn["iters"][a] == it, (a, qn["status"][a], st, qn["iters"][a], it)
        got = qn["cpts"][a, :15 * M]
        worst = max(worst, np.abs(got - x).max())
        assert np.allclose(got, x, atol=TOL, rtol=0), f"agent {a}: max diff {np.abs(got - x).max()}"
        assert not qn["cpts"][a, 15 * M:].any()
        # solution quality (reference's own test tolerance 1e-3, test_bezier_opt.cpp:156-185)
        X = got.reshape(-1, 3)
        d = np.full(M, pp.corridor_tau)
        assert np.abs(orc.bezier_eval(d, X, 0.0) - pva[a, :3]).max() < 1e-3 + 1e-3
    print("max |cpts_gpu - cpts_oracle| =", worst)
    P.close()
    m.close()


@pytest.mark.parametrize("A,seed", [(8, 17), (6, 5)])
def test_replan_chain_matches_oracle(pop, orc, A, seed):
    sogm, planner, spec, sc, pva, recs, dev, m, ap, pp, qs, P = _setup(pop, A, seed)
    t_start = sc["stamps"] + 0.05
    rec_d, ok_d = P.replan(sogm._dev(pva, np.float64), sogm._dev(sc["goals"], np.float64),
                           sogm._dev(t_start, np.float64), dev["ego_ids"])
    got = planner.records_from_bytes(rec_d.cpu().numpy())
    ok = ok_d.cpu().numpy()
    grids = oracle_grids(pop, orc, spec, sc, recs)
    n_ok = 0
    for a in range(A):
        w_ok, w, stage = orc.replan(spec, ap, pp, qs, grids[a], sc["poses"][a], sc["stamps"][a], pva[a],
                                    sc["goals"][a], t_start[a], a)
        assert ok[a] == w_ok
        assert got[a].drone_id == a and got[a].n_pieces == w.n_pieces and got[a].time_start == w.time_start
        if w_ok:
            n_ok += 1
            k = w.n_pieces
            assert list(got[a].duration)[:k] == list(w.duration)[:k]
            assert np.allclose(np.array(got[a].cpts[:15 * k]), np.array(w.cpts[:15 * k]), atol=TOL, rtol=0)
    assert n_ok > 0
    P.close()
    m.close()


def _box_chain(M, nf, max_faces, rng, tau_len=0.3):
    """A straight corridor of M overlapping polytopes along +x: the six box faces of segment i plus nf - 6 redundant
    tilted planes that do not cut the box (h.x + d <= 0 inside).  Returns polys [16][max_faces][4], nfaces [16]."""
    polys = np.zeros((16, max_faces, 4))
    nfaces = np.zeros(16, np.int32)
    for i in range(M):
        lo = np.array([i * tau_len - 0.5, -0.6, 0.4]); hi = np.array([(i + 1) * tau_len + 0.5, 0.6, 1.6])
        H = []
        for k in range(3):
            e = np.zeros(3); e[k] = 1.0
            H.append(np.concatenate([e, [-hi[k]]]))
            H.append(np.concatenate([-e, [lo[k]]]))
        c = 0.5 * (lo + hi)
        while len(H) < nf:
            n = rng.normal(size=3); n /= np.linalg.norm(n)
            # support of the box in direction n, pushed out by a margin: redundant but a real row of the QP
            sup = np.sum(np.abs(n) * 0.5 * (hi - lo)) + rng.uniform(0.05, 0.5)
            H.append(np.concatenate([n, [-(n @ c + sup)]]))
        polys[i, :nf] = np.array(H)
        nfaces[i] = nf
    return polys, nfaces


# (pieces, faces per polytope) and the path the solver must take for it, (register-resident iteration, every row array in
# LDS) — what the layout description (csrc/sogm_qp_layout.hpp; on the host: tests/qp_layout_host_test.cpp) gives for the
# shape at the dynamic LDS a planner is granted.  All four combinations occur:
QP_PATH_SHAPES = [
    (12, 6, (0, 1)),   # general iteration (no block factor), rows in LDS
    (8, 30, (0, 0)),   # S = 1200 rows: general iteration, row storage in HBM scratch
    (8, 25, (1, 0)),   # S = 1000: register-resident iteration with the cold row data in HBM scratch
    (5, 40, (1, 0)),   # S = 1000 with few pieces: 149 584 bytes with everything in LDS, just beyond the grant
    (3, 6, (1, 1)),    # the common small case
    (16, 6, (0, 0)),   # the most pieces the ABI takes (n = 240: the set-up's column quads take two trips)
]
assert {p for _, _, p in QP_PATH_SHAPES} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("M,nf,path", QP_PATH_SHAPES, ids=[f"{M}-{nf}" for M, nf, _ in QP_PATH_SHAPES])
def test_qp_solver_paths_match_oracle(pop, orc, M, nf, path):
    import torch
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    A = 3
    spec = pop.config.make_spec("parity")
    m = sogm.SogmMap(spec, A)
    ap, pp, qs = pop.config.make_astar_params(), pop.config.make_planner_params(True), pop.config.make_qp_settings()
    P = planner.SogmPlanner(m, ap, pp, qs)
    rng = np.random.default_rng(1000 * M + nf)
    polys = np.zeros((A, 16, pp.max_faces, 4)); nfaces = np.zeros((A, 16), np.int32)
    pva = np.zeros((A, 9)); goal = np.zeros((A, 6))
    for a in range(A):
        polys[a], nfaces[a] = _box_chain(M, nf, pp.max_faces, rng)
        pva[a, :3] = [0.0, rng.uniform(-0.2, 0.2), 1.0 + rng.uniform(-0.2, 0.2)]
        pva[a, 3:6] = [rng.uniform(0.0, 0.8), 0.0, 0.0]
        goal[a, :3] = [M * 0.3, rng.uniform(-0.2, 0.2), 1.0]
    npoly = np.full(A, M, np.int32)
    dev = lambda x, t: torch.as_tensor(np.ascontiguousarray(x, dtype=t), device="cuda")
    q = P.optimize(dev(pva, np.float64), dev(goal, np.float64), dev(polys, np.float64), dev(nfaces, np.int32),
                   dev(npoly, np.int32))
    qn = {k: v.cpu().numpy() for k, v in q.items()}
    worst = 0.0
    for a in range(A):
        st, x, it = orc.qp_solve(pva[a], np.concatenate([goal[a], np.zeros(3)]), [pp.corridor_tau] * M, polys[a],
                                 nfaces[a], pp.max_faces,
                                 pp.opt_max_vel, pp.opt_max_acc, qs)
        assert qn["status"][a] == st and qn["iters"][a] == it, (a, qn["status"][a], st, qn["iters"][a], it)
        if st in (1, 2):
            got = qn["cpts"][a, :15 * M]
            worst = max(worst, np.abs(got - x).max())
            assert np.allclose(got, x, atol=TOL, rtol=0), f"agent {a}: max diff {np.abs(got - x).max()}"
    print(f"M={M} faces={nf}: statuses {qn['status'].tolist()} iters {qn['iters'].tolist()} max diff {worst:.2e}")
    assert (qn["status"] == 1).any(), "the synthetic corridors are meant to be solvable"
    # every agent's workgroup took the named path, which is also what the layout predicts for its (M, nfaces)
    stats = P.qp_stats()
    for a in range(A):
        lay = P.qp_layout(nfaces[a, :M])
        # the record is this solve's (a record nobody wrote would read path 0, which two of the shapes expect)
        assert stats[a, pop._abi.QP_STAT_ITERS] == qn["iters"][a] > 0 and stats[a, pop._abi.QP_STAT_TOTAL] > 0, (a, stats[a])
        took = int(stats[a, pop._abi.QP_STAT_PATH])
        print(f"  agent {a}: path {took} layout {lay}")
        assert (lay["fast"], lay["rows_in_lds"]) == path, (a, lay)
        assert took == lay["fast"] | lay["rows_in_lds"] << 1, (a, took, lay)
    P.close()
    m.close()


def test_time_allocation_end_state_and_limits_of_bezieropt_setup(pop, orc):
    """BezierOpt::setup in full (sogm_bezier_qp_solve_timed): the reference's own 3-cube fixture with ITS time vector
    (test_bezier_opt.cpp:57-99: t = [2, 4, 2], limits 3 / 3, an end state with velocity), plus per-agent variations —
    other time vectors, a non-zero final acceleration, other limits — against the oracle's assembly + OSQP
    restatement: same status and iteration count, coefficients within 1e-4; and the fixture's solution still meets the
    reference test's own boundary tolerances (:156-185)."""
    import json
    import os
    import torch
    sogm = importlib.import_module("pred-occ-planner_amd.sogm")
    planner = importlib.import_module("pred-occ-planner_amd.planner")
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bezier_opt_fixture.json")))
    t = G["three"]
    A, MP = 6, pop._abi.SOGM_MAX_PIECES
    spec = pop.config.make_spec("parity")
    m = sogm.SogmMap(spec, A)
    pp = pop.config.make_planner_params(True)
    P = planner.SogmPlanner(m, pop.config.make_astar_params(), pp, pop.config.make_qp_settings())
    MF = pp.max_faces
    cubes = np.array(t["cubes"], float)                                    # [3][6][4]
    start, end = np.array(t["start"], float), np.array(t["end"], float)   # rows pos, vel, acc
    cases = []
    for a in range(A):
        tv = np.array(t["t"], float) * [1.0, 0.5, 1.5, 1.0, 0.8, 1.0][a]
        if a == 3:
            tv = np.array([1.5, 3.0, 2.5])
        e = end.copy()
        if a in (2, 4):
            e[2] = [0.3, -0.2, 0.1]                                          # final acceleration
        if a == 5:
            e[1] = [0.0, 0.0, 0.0]
        lim = (3.0, 3.0) if a != 4 else (4.0, 5.0)
        cases.append((tv, e, lim))
    polys = np.zeros((A, MP, MF, 4))
    nf = np.zeros((A, MP), np.int32)
    tal = np.zeros((A, MP))
    for a, (tv, e, lim) in enumerate(cases):
        polys[a, :3, :6] = cubes
        nf[a, :3] = 6
        tal[a, :3] = tv
    # one launch per limit pair (the limits are arguments of the call, not per agent)
    got = {}
    for lim in sorted({c[2] for c in cases}):
        q = P.optimize_timed(sogm._dev(np.tile(start.reshape(1, 9), (A, 1)), np.float64),
                             sogm._dev(np.stack([c[1].reshape(9) for c in cases]), np.float64),
                             sogm._dev(tal, np.float64), sogm._dev(polys, np.float64), sogm._dev(nf),
                             sogm._dev(np.full(A, 3, np.int32)), lim[0], lim[1])
        got[lim] = {k: v.cpu().numpy() for k, v in q.items()}
    n_solved = 0
    for a, (tv, e, lim) in enumerate(cases):
        st, x, it = orc.qp_solve(start, e, tv, polys[a], nf[a], MF, lim[0], lim[1], P.qs)
        g = got[lim]
        assert (g["status"][a], g["iters"][a]) == (st, it), (a, g["status"][a], st, g["iters"][a], it)
        if st in (1, 2):
            n_solved += 1
            assert np.abs(g["cpts"][a, :45] - x).max() <= 1e-4, a
    assert n_solved >= 4 and got[(3.0, 3.0)]["status"][0] in (1, 2)   # (halving the times makes one case infeasible)
    # agent 0 is the reference's fixture itself: its own boundary checks (TestWaypoints, 1e-3)
    X, d = got[(3.0, 3.0)]["cpts"][0, :45].reshape(15, 3), np.array(t["t"], float)
    for der in range(3):
        assert np.abs(orc.bezier_eval(d, X, 0.0, der) - start[der]).max() < t["bc_tol"]
        assert np.abs(orc.bezier_eval(d, X, d.sum(), der) - end[der]).max() < t["bc_tol"]
    P.close()
    m.close()


def test_fp32_residual_mode_keeps_status_and_coefficients(pop, orc):
    """BASELINE configs[4]'s "mixed-precision ADMM residuals" (SogmQpSettings.residual_fp32 = 1): the termination
    checks run in fp32.  Contract (sogm_abi.h): same status as the fp64 solve and coefficients within 1e-4 — a check
    may pass one interval earlier or later, so the iteration count may differ by a multiple of check_termination."""
    sogm, planner, spec, sc, pva, recs, dev, m, ap, pp, qs, P = _setup(pop, 12, 99)
    qs32 = pop.config.make_qp_settings()
    qs32.residual_fp32 = 1
    P32 = planner.SogmPlanner(m, ap, pp, qs32)
    t_start = sc["stamps"] + 0.05
    d_pva, d_ts = sogm._dev(pva, np.float64), sogm._dev(t_start, np.float64)
    s = P.search(d_pva, sogm._dev(sc["goals"], np.float64), d_ts)
    c = P.generateCorridors(d_pva, d_ts, s["route"], s["route_len"])
    q64 = {k: v.cpu().numpy() for k, v in P.optimize(d_pva, c["goal"], c["polys"], c["nfaces"], c["npoly"]).items()}
    q32 = {k: v.cpu().numpy() for k, v in P32.optimize(d_pva, c["goal"], c["polys"], c["nfaces"], c["npoly"]).items()}
    assert np.array_equal(q32["status"], q64["status"])
    d_it = np.abs(q32["iters"] - q64["iters"])
    assert (d_it % qs.check_termination == 0).all() and d_it.max() <= 2 * qs.check_termination, d_it
    ok = np.isin(q64["status"], (1, 2))
    assert ok.sum() >= 8 and np.abs(q32["cpts"][ok] - q64["cpts"][ok]).max() <= TOL
    print("fp32 residuals: iteration differences", d_it.tolist(), "max |dx|", np.abs(q32["cpts"][ok] - q64["cpts"][ok]).max())
    P32.close()
    P.close()
    m.close()
