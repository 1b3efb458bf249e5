"""The Bezier QP's answer against an optimum and a feasibility verdict that do not come from OSQP
(tests/golden/make_qp_optimum_fixture.py -> qp_optimum_independent.json: numpy assembly, HiGHS LP, interior point with
a KKT certificate).  CPU only: the stored certificates re-checked in numpy on matrices assembled again from the stored
inputs, the C++ oracle's assembly on these shapes, and the oracle's OSQP restatement held to the termination contract
of tests/qp_contract.py — which pins the meaning of the answer (feasible within OSQP's tolerance, a true
infeasibility verdict, an objective no better than duality allows), not OSQP's iteration path."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)
import qp_contract  # noqa: E402
from make_qp_fixture import assemble  # noqa: E402

G = json.load(open(os.path.join(HERE, "golden", "qp_optimum_independent.json")))
CASES = G["cases"]
MF = 64
IDS = [c["name"] for c in CASES]


def problem(c):
    return assemble(c["start"], c["end"], c["t"], [np.array(p, float) for p in c["polys"]], c["vmax"], c["amax"])


def padded(c):
    polys = np.zeros((c["M"], MF, 4))
    for i, p in enumerate(c["polys"]):
        polys[i, :len(p)] = np.array(p, float)
    return polys, np.array(c["faces"], np.int32)


def test_fixture_covers_every_path_and_regime():
    """every kernel path with a feasible case whose box rows are active and an infeasible case; near-boundary cases;
    every case says why it exists"""
    assert all(c["why"] for c in CASES)
    paths = ("reg_3x6", "reg_8x6", "reg_cold_8x25", "reg_few_5x40", "gen_lds_12x6", "gen_hbm_8x30", "gen_16x6")
    for p in paths:
        mine = [c for c in CASES if c["path"] == p]
        assert any(c["feasible"] and c["active_box_rows"] > 0 for c in mine), p
        assert any(not c["feasible"] and c["t_star"] >= 1e-2 for c in mine), p
    assert sum(0 < c["t_star"] < 1e-3 for c in CASES) >= 3
    assert {1, 2} <= {c["M"] for c in CASES}
    assert os.path.getsize(os.path.join(HERE, "golden", "qp_optimum_independent.json")) < 500 * 1024


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_stored_optimum_carries_its_kkt_certificate(k):
    c = CASES[k]
    if not c["feasible"]:
        assert c["t_star"] > 0 and "x_star" not in c
        return
    Q, A, lb, ub = problem(c)
    l, u = qp_contract.lower(lb), np.asarray(ub, float)
    x = np.array(c["x_star"])
    act = np.array(c["active"], float)
    rows, lam = act[:, 0].astype(int), act[:, 1]
    Ax = A @ x
    # stationarity
    r = Q @ x + A[rows].T @ lam
    scale = max(1.0, np.abs(Q @ x).max(), (np.abs(A[rows]) * np.abs(lam)[:, None]).max())
    assert np.abs(r).max() <= 1e-9 * scale, np.abs(r).max()
    # primal feasibility
    v, nAx = qp_contract.violation(A, l, u, x)
    assert v.max() <= 1e-9 * max(1.0, nAx)
    # sign on the active side and complementarity: lam > 0 only where the row sits at u, lam < 0 only at a finite l
    up, lo_ = lam > 0, lam < 0
    assert (np.abs(Ax[rows][up] - u[rows][up]) <= 1e-9 * max(1.0, nAx)).all()
    assert np.isfinite(l[rows][lo_]).all()
    assert (np.abs(Ax[rows][lo_] - l[rows][lo_]) <= 1e-9 * max(1.0, nAx)).all()
    assert np.abs(0.5 * x @ Q @ x - c["f_star"]) <= 1e-12 * max(1.0, abs(c["f_star"]))


def test_row_scaling_leaves_the_optimum():
    """every face row (h, h3) scaled by 10^U(-3, 3): the same problem, the same x*"""
    by = {c["name"]: c for c in CASES}
    a, b = by["reg_3x6_tight"], by["reg_3x6_tight_rows_scaled"]
    assert np.abs(np.array(a["x_star"]) - np.array(b["x_star"])).max() <= 1e-8
    assert abs(a["f_star"] - b["f_star"]) <= 1e-10 * abs(a["f_star"])


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_oracle_assembly_equals_the_numpy_assembly(orc, k):
    c = CASES[k]
    polys, nf = padded(c)
    Q, A, l, u = orc.qp_assemble(c["start"], c["end"], c["t"], polys, nf, MF, c["vmax"], c["amax"])
    Qi, Ai, lbi, ubi = problem(c)
    assert A.shape == Ai.shape and np.array_equal(A != 0, Ai != 0)
    assert np.abs(A - Ai).max() <= 1e-13 * max(1.0, np.abs(Ai).max())
    assert np.abs(Q - Qi).max() <= 1e-12 * np.abs(Qi).max()
    assert np.abs(u - ubi).max() <= 1e-13 * max(1.0, np.abs(ubi).max())
    li = qp_contract.lower(lbi)
    fin = np.isfinite(li)
    assert (l[~fin] <= -1e29).all() and np.abs(l[fin] - li[fin]).max() <= 1e-13 * max(1.0, np.abs(li[fin]).max())


_worst = {}


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_oracle_meets_the_contract(pop, orc, k):
    c = CASES[k]
    qs = pop.config.make_qp_settings()
    polys, nf = padded(c)
    st, x, it = orc.qp_solve(c["start"], c["end"], c["t"], polys, nf, MF, c["vmax"], c["amax"], qs)
    Q, A, lb, ub = problem(c)
    opt = {"x": c["x_star"], "f": c["f_star"], "active": c["active"]} if c["feasible"] else None
    rep = qp_contract.check(Q, A, lb, ub, st, x, qs.eps_abs, qs.eps_rel, t_star=c["t_star"], opt=opt,
                            sanity=G["sanity"])
    assert not rep["errors"], (c["name"], st, it, rep)
    for key in ("dx", "df_rel"):
        if key in rep:
            _worst[key] = max(_worst.get(key, 0.0), rep[key])
    print(f"{c['name']}: status {st} iters {it} viol/bound {rep.get('ratio', float('nan')):.3f} "
          f"dx {rep.get('dx', float('nan')):.2e} df_rel {rep.get('df_rel', float('nan')):.2e}; worst so far {_worst}")


def _oracle_solves(pop, orc, pick):
    qs = pop.config.make_qp_settings()
    out = []
    for c in CASES:
        if pick(c):
            polys, nf = padded(c)
            st, x, it = orc.qp_solve(c["start"], c["end"], c["t"], polys, nf, MF, c["vmax"], c["amax"], qs)
            out.append((c, st, x, it, qs))
    return out


def test_wide_infeasibility_is_certified(pop, orc):
    """a corridor whose goal lies 0.3 m outside its last box (t* = 0.15) is certified infeasible, not run to max_iter:
    the contract alone would accept -2, so without this a certificate that never fires (a sign turned round in
    u'(dy)+ + l'(dy)- < -eps ||dy||, or in the projection of dy) would pass"""
    got = _oracle_solves(pop, orc, lambda c: not c["feasible"] and c["t_star"] >= 0.1)
    assert len(got) >= 7
    bad = [(c["name"], st, it) for c, st, x, it, qs in got if st not in (-3, 3)]
    assert not bad, bad


def test_relative_tolerance_is_used(pop, orc):
    """OSQP's status-1 test is eps_abs + eps_rel max(||Ax||, ||z||): on this fixture some answer lands beyond eps_abs
    alone (and within the contract's bound) — a termination test without its eps_rel term would never get there"""
    got = _oracle_solves(pop, orc, lambda c: True)
    beyond = []
    for c, st, x, it, qs in got:
        if st == 1:
            Q, A, lb, ub = problem(c)
            v, nAx = qp_contract.violation(A, qp_contract.lower(lb), np.asarray(ub, float), x)
            if v.max() > qs.eps_abs / (1.0 - qs.eps_rel):
                beyond.append((c["name"], float(v.max())))
    assert beyond, "no status-1 answer uses the eps_rel part of the tolerance"
