"""OSQP's termination contract for the Bezier QP, written once in numpy (fp64) and read by the CPU and the GPU tests
(tests/test_qp_optimum_independent.py, tests/test_qp_optimum_gpu.py).  Not collected by pytest (helper module).

It judges a returned (status, x) by what the answer means, not by how OSQP got there.  Everything is taken from the
independent numpy assembly (tests/golden/make_qp_fixture.py `assemble`), never from the solver:
  viol = || max(Ax - u, l - Ax, 0) ||_inf  over the UNSCALED rows (OSQP's default scaled_termination = 0).
OSQP keeps z in [l, u], so its primal residual ||Ax - z||_inf >= viol, and its test
||Ax - z|| < eps_abs + eps_rel max(||Ax||, ||z||) with ||z|| <= ||Ax|| + ||Ax - z|| gives, with no solver state at all,
  status 1  (solved):             viol <= (eps_abs + eps_rel ||Ax||_inf) / (1 - eps_rel)
  status 2  (solved inaccurate):  the same with both eps x 10 (osqp_solve's epilogue, check_termination(approximate))
  status -3 / 3 (primal infeasible [inaccurate]): the QP really is infeasible, t* > 0, where t* is the optimum of the
            LP  min t  s.t.  l - t <= Ax <= u + t  (viol >= t* for every x, so a "solved" with t* above its bound is
            impossible as well)
  status 1 / 2 with a certified optimum x* (multipliers lam* on its active rows, Q x* + A' lam* = 0):
    weak duality  f(x) >= f* - sum_i |lam*_i| viol_i(x)   (always true: convexity of f, signs of lam*);
    f(x) - f* and ||x - x*||_inf below sanity bounds that are calibrated, not derived (the fixture keeps both the
    bounds and the measured worst values they came from: OSQP at eps 1e-3 may stop decimetres from x*);
  always: the coefficients beyond 15 M are zero."""
import numpy as np

FREE = -1e29   # lower bounds at or below this are -OSQP_INFTY (assemble() writes None)


def lower(lb):
    return np.array([-np.inf if v is None or v <= FREE else float(v) for v in lb])


def violation(A, l, u, x):
    """per-row violation max(Ax - u, l - Ax, 0) and ||Ax||_inf"""
    Ax = A @ x
    return np.maximum(np.maximum(Ax - u, l - Ax), 0.0), float(np.abs(Ax).max())


def viol_bound(nAx, eps_abs, eps_rel, status, slack=0.0):
    """the largest violation a status of 1 (or 2: tolerances x 10) allows, plus `slack` (rounding of the solver's
    residual arithmetic, stated where it is used)"""
    k = 10.0 if status == 2 else 1.0
    ea, er = eps_abs * k, eps_rel * k
    return (ea + er * nAx) / (1.0 - er) + slack


def objective(Q, x):
    return 0.5 * float(x @ Q @ x)


def check(Q, A, lb, ub, status, x, eps_abs, eps_rel, M=None, t_star=None, opt=None, sanity=None, slack_rel=0.0):
    """Apply the contract.  Q, A, lb, ub: the independent assembly (lb may hold None / -1e30 for free sides).  x: the
    returned coefficients (15 M, or the full padded vector with M given: the tail must be zero).  t_star: the LP
    optimum (None: not known, the infeasibility verdict is then not judged).  opt: {"x": x*, "f": f*, "active":
    [[row, lam], ...]} of a certified optimum, or None.  sanity: {"dx": bound, "df_rel": bound}.  slack_rel: rounding
    allowance added to the violation bound, as a multiple of ||Ax||_inf.  Returns a report dict; report["errors"]
    lists every breach (empty = the answer meets the contract)."""
    x = np.asarray(x, np.float64).reshape(-1)
    n = Q.shape[0]
    rep = {"status": int(status), "errors": []}
    if M is not None and x.size > 15 * M:
        tail = np.abs(x[15 * M:]).max()
        rep["tail"] = float(tail)
        if tail != 0.0:
            rep["errors"].append(f"coefficients beyond 15 M = {15 * M} are not zero (max |x| {tail:.3e})")
    x = x[:n]
    l, u = lower(lb), np.asarray(ub, np.float64)
    v, nAx = violation(A, l, u, x)
    rep["viol"], rep["nAx"] = float(v.max()), nAx
    if status in (1, 2):
        if not np.isfinite(x).all():
            rep["errors"].append("non-finite coefficients")
            return rep
        bnd = viol_bound(nAx, eps_abs, eps_rel, status, slack_rel * nAx)
        rep["bound"] = bnd
        rep["ratio"] = rep["viol"] / bnd
        if not rep["viol"] <= bnd:
            rep["errors"].append(f"status {status}: violation {rep['viol']:.3e} > bound {bnd:.3e}")
        if t_star is not None and t_star > bnd:
            rep["errors"].append(f"status {status} on a QP with t* = {t_star:.3e} > bound {bnd:.3e}")
        if opt is not None:
            xs = np.asarray(opt["x"], np.float64)
            f, fs = objective(Q, x), float(opt["f"])
            act = np.asarray(opt["active"], np.float64).reshape(-1, 2)
            rows, lam = act[:, 0].astype(int), act[:, 1]
            # slack of the weak-duality bound: the certificate's own residuals (stationarity r, primal error of x*)
            r = Q @ xs + A[rows].T @ lam
            ax_s = A[rows] @ xs
            tgt = np.where(lam > 0, u[rows], np.where(np.isfinite(l[rows]), l[rows], u[rows]))
            dual_slack = np.abs(r).sum() * np.abs(x - xs).max() + np.abs(lam) @ np.abs(ax_s - tgt) + 1e-12 * abs(fs)
            wd = fs - np.abs(lam) @ v[rows] - dual_slack
            rep["f"], rep["f_star"], rep["weak_dual_lb"] = f, fs, float(wd)
            if not f >= wd:
                rep["errors"].append(f"objective {f:.9e} below the weak-duality bound {wd:.9e} (f* {fs:.9e})")
            rep["dx"] = float(np.abs(x - xs).max())
            rep["df_rel"] = (f - fs) / max(abs(fs), 1e-12)
            if sanity is not None:
                if not rep["dx"] <= sanity["dx"]:
                    rep["errors"].append(f"||x - x*|| = {rep['dx']:.3e} > sanity bound {sanity['dx']:.3e}")
                if not rep["df_rel"] <= sanity["df_rel"]:
                    rep["errors"].append(f"(f - f*) / |f*| = {rep['df_rel']:.3e} > sanity bound {sanity['df_rel']:.3e}")
    elif status in (-3, 3):
        if t_star is not None and not t_star > 0.0:
            rep["errors"].append(f"status {status} (primal infeasible) on a feasible QP (t* = {t_star:.3e})")
    elif status != -2:
        rep["errors"].append(f"status {status} is not an outcome of this solver (1, 2, -2, -3, 3)")
    return rep
