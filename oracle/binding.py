"""ctypes binding of oracle/liboracle.so.  TEST INFRASTRUCTURE ONLY: imported by tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg — never by the product package."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
_abi = importlib.import_module("pred-occ-planner_amd._abi")

LIB_PATH = os.path.join(_HERE, "liboracle.so")


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


_lib = None
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        for name in ("orc_bezier_max_rate", "orc_linprog", "orc_linprog_perm"):
            if hasattr(_lib, name):
                getattr(_lib, name).restype = C.c_double
    return _lib


def dptr(a):
    return a.ctypes.data_as(_dp)


def fptr(a):
    return a.ctypes.data_as(_fp)


def iptr(a):
    return a.ctypes.data_as(_ip)


# ---------------------------------------------------------------- Bernstein
def bezier_eval(durations, cpts, t, derivative=0):
    d = np.ascontiguousarray(durations, np.float64)
    c = np.ascontiguousarray(cpts, np.float64)
    out = np.zeros(3)
    lib().orc_bezier_eval(dptr(d), dptr(c), len(d), C.c_double(t), derivative, dptr(out))
    return out


def piece_eval(cpts, t0, tf, t, derivative=0):
    c = np.ascontiguousarray(cpts, np.float64)
    out = np.zeros(3)
    lib().orc_piece_eval(dptr(c), C.c_double(t0), C.c_double(tf), C.c_double(t), derivative, dptr(out))
    return out


def derivative_ctrl_pts(pts):
    p = np.ascontiguousarray(pts, np.float64)
    out = np.zeros((p.shape[0] - 1, 3))
    lib().orc_derivative_ctrl_pts(dptr(p), p.shape[0], dptr(out))
    return out


def bezier_max_rate(durations, cpts, derivative):
    d = np.ascontiguousarray(durations, np.float64)
    c = np.ascontiguousarray(cpts, np.float64)
    return float(lib().orc_bezier_max_rate(dptr(d), dptr(c), len(d), derivative))


def bernstein_coeff():
    A = np.zeros(25)
    lib().orc_bernstein_coeff(dptr(A))
    return A.reshape(5, 5)


# ---------------------------------------------------------------- map
def ego_particles(size):
    out = np.zeros((512, 3))
    n = lib().orc_ego_particles(C.c_double(size[0]), C.c_double(size[1]), C.c_double(size[2]), dptr(out), 512)
    return out[:n].copy()


def update_gt(spec, cloud, cyl_struct, n_cyl, pose):
    V = spec.L * spec.W * spec.H
    grid = np.zeros((V, spec.T), dtype=np.float32)
    cloud = np.ascontiguousarray(cloud, np.float32)
    pose = np.ascontiguousarray(pose, np.float32)
    lib().orc_update_gt(C.byref(spec), fptr(cloud), cloud.shape[0], cyl_struct, n_cyl, fptr(pose), fptr(grid))
    return grid


def project_neighbours(spec, grid, records, n_rec, ego_id, body, pose, stamp):
    pose = np.ascontiguousarray(pose, np.float32)
    body = np.ascontiguousarray(body, np.float64)
    lib().orc_project_neighbours(C.byref(spec), records, n_rec, int(ego_id), dptr(body), body.shape[0],
                                 fptr(pose), C.c_double(stamp), fptr(grid))
    return grid


_resample_keep = None


def set_resample(rate, n, table):
    """ParticleATC's resample branch for project_neighbours (off: rate 0); `table` float32 standard normals."""
    global _resample_keep
    _resample_keep = np.ascontiguousarray(table, np.float32) if table is not None else None
    lib().orc_set_resample(C.c_float(rate), int(n), fptr(_resample_keep) if _resample_keep is not None else None)


def query_clear(spec, grid, pose, pos, t, t_is_index=False):
    pose = np.ascontiguousarray(pose, np.float32)
    pos = np.ascontiguousarray(pos, np.float64)
    if t_is_index:
        return lib().orc_query_clear_idx(C.byref(spec), fptr(grid), fptr(pose), dptr(pos), int(t))
    return lib().orc_query_clear_time(C.byref(spec), fptr(grid), fptr(pose), dptr(pos), C.c_double(t))


def obstacle_points(spec, grid, pose, stamp, t0, t1, lc, hc, cap=4096):
    pose = np.ascontiguousarray(pose, np.float32)
    lc = np.ascontiguousarray(lc, np.float64)
    hc = np.ascontiguousarray(hc, np.float64)
    out = np.zeros((cap, 3))
    n = lib().orc_obstacle_points(C.byref(spec), fptr(grid), fptr(pose), C.c_double(stamp), C.c_double(t0),
                                  C.c_double(t1), dptr(lc), dptr(hc), dptr(out), cap)
    return out[:min(n, cap)].copy(), n


# ---------------------------------------------------------------- A*
def astar_use_libm(on):
    lib().orc_astar_use_libm(1 if on else 0)


def astar_search(spec, ap, grid, pose, start_pva, goal, t_after_map, corridor_tau=0.3, route_cap=64,
                 trace_cap=20000, mode=0):
    lib().orc_astar_set_mode(mode)
    pose = np.ascontiguousarray(pose, np.float32)
    s = np.ascontiguousarray(start_pva, np.float64).reshape(9)
    g = np.ascontiguousarray(goal, np.float64)
    route = np.zeros((route_cap, 6))
    n = C.c_int(0)
    stats = (C.c_int * 4)()
    trace = np.zeros(trace_cap, np.int32)
    ntr = C.c_int(0)
    ret = lib().orc_astar_search(C.byref(spec), C.byref(ap), fptr(grid), fptr(pose), dptr(s), dptr(g),
                                 C.c_double(t_after_map), C.c_double(corridor_tau), dptr(route), C.byref(n),
                                 route_cap, stats, trace.ctypes.data_as(C.POINTER(C.c_int32)), trace_cap,
                                 C.byref(ntr))
    # route_len: the route's full count; "route" holds its first min(route_len, route_cap) points
    return {"ret": ret, "route": route[:n.value].copy(), "route_len": n.value, "stats": list(stats),
            "trace": trace[:min(ntr.value, trace_cap)].copy(), "trace_len": ntr.value}


def astar_debug_nodes(n):
    """the first n pool nodes of the last astar_search: rows {state[6], input[3], duration, time, g, f, index[3], time_idx,
    parent}"""
    out = np.zeros((n, 18))
    k = lib().orc_astar_debug_nodes(dptr(out), n)
    return out[:k]


# ---------------------------------------------------------------- LP
def linprog(c, A, b):
    c = np.ascontiguousarray(c, np.float64)
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    d = len(c)
    x = np.zeros(d)
    v = lib().orc_linprog(d, dptr(c), dptr(A), dptr(b), A.shape[0], dptr(x))
    return float(v), x


def linprog_perm(c, A, b, perm):
    c = np.ascontiguousarray(c, np.float64)
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    perm = np.ascontiguousarray(perm, np.int32)
    assert sorted(perm.tolist()) == list(range(A.shape[0]))
    x = np.zeros(len(c))
    v = lib().orc_linprog_perm(len(c), dptr(c), dptr(A), dptr(b), A.shape[0], iptr(perm), dptr(x))
    return float(v), x


def lp_set_mode(mode, reset=True):
    lib().orc_lp_set_mode(int(mode))
    if reset:
        lib().orc_lp_rng_reset()


def lp_permutation(n, kind="fixed"):
    p = np.zeros(max(n, 1), np.int32)
    (lib().orc_lp_fixed_permutation if kind == "fixed" else lib().orc_lp_rand_permutation)(n, iptr(p))
    return p[:n]


# ---------------------------------------------------------------- FIRI / corridors
def firi(bd, pc, a, b, iterations=2, max_faces=64, r=None):
    bd = np.ascontiguousarray(bd, np.float64)
    pc = np.ascontiguousarray(pc, np.float64).reshape(-1, 3)
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    hp = np.zeros((max_faces, 4))
    r = np.ones(3) if r is None else np.ascontiguousarray(r, np.float64).copy()
    n = lib().orc_firi(dptr(bd), bd.shape[0], dptr(pc), pc.shape[0], dptr(a), dptr(b), iterations,
                       dptr(hp), max_faces, dptr(r))
    return (hp[:max(n, 0)].copy() if n <= max_faces else hp.copy()), n, r


def lbfgs_set_max_iterations(k):
    """test knob: lbfgs_parameter_t::max_iterations of the MVIE's optimiser (0 = the reference's unlimited default)"""
    lib().orc_lbfgs_set_max_iterations(int(k))


def mvie(hpoly, R, p, r):
    h = np.ascontiguousarray(hpoly, np.float64)
    R = np.ascontiguousarray(R, np.float64).copy()
    p = np.ascontiguousarray(p, np.float64).copy()
    r = np.ascontiguousarray(r, np.float64).copy()
    ok = lib().orc_mvie(dptr(h), h.shape[0], dptr(R), dptr(p), dptr(r))
    return ok, R, p, r


def corridor_generate(spec, pp, grid, pose, stamp, start_pva, t_start, route):
    pose = np.ascontiguousarray(pose, np.float32)
    s = np.ascontiguousarray(start_pva, np.float64).reshape(9)
    route = np.ascontiguousarray(route, np.float64)
    MP = _abi.SOGM_MAX_PIECES
    polys = np.zeros((MP, pp.max_faces, 4))
    nf = np.zeros(MP, np.int32)
    goal = np.zeros(6)
    n = lib().orc_corridor_generate(C.byref(spec), C.byref(pp), fptr(grid), fptr(pose), C.c_double(stamp),
                                    dptr(s), C.c_double(t_start), dptr(route), route.shape[0], dptr(polys),
                                    nf.ctypes.data_as(C.POINTER(C.c_int32)), dptr(goal))
    return {"npoly": n, "polys": polys, "nfaces": nf, "goal": goal}


def corridor_rules(pp, start_pva, route, polys, nfaces, seg_state=None):
    """The corridor rules around FIRI for injected polytopes: polys [16, max_faces, 4] un-shrunk, nfaces [16],
    seg_state [16] or None (-3 marks a segment as over capacity)."""
    s = np.ascontiguousarray(start_pva, np.float64).reshape(9)
    route = np.ascontiguousarray(route, np.float64).reshape(-1, 6)
    MP, MF = _abi.SOGM_MAX_PIECES, pp.max_faces
    polys = np.ascontiguousarray(polys, np.float64).reshape(MP, MF, 4)
    nfaces = np.ascontiguousarray(nfaces, np.int32).reshape(MP)
    st = None if seg_state is None else np.ascontiguousarray(seg_state, np.int32).reshape(MP)
    iptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = {"box": np.zeros((MP, 6)), "shrunk": np.zeros((MP, MF, 4)), "seg_nfaces": np.zeros(MP, np.int32),
           "seg_state": np.zeros(MP, np.int32), "polys": np.zeros((MP, MF, 4)), "nfaces": np.zeros(MP, np.int32),
           "goal": np.zeros(6)}
    cap = np.zeros(2, np.int32)
    out["npoly"] = int(lib().orc_corridor_rules(
        C.byref(pp), dptr(s), dptr(route), route.shape[0], dptr(polys), iptr(nfaces), None if st is None else iptr(st),
        dptr(out["box"]), dptr(out["shrunk"]), iptr(out["seg_nfaces"]), iptr(out["seg_state"]), dptr(out["polys"]),
        iptr(out["nfaces"]), dptr(out["goal"]), iptr(cap)))
    out["corridor_capacity"], out["pieces_capacity"] = int(cap[0]), int(cap[1])
    return out


# ---------------------------------------------------------------- QP
def qp_assemble(start, goal, t_alloc, polys, nfaces, max_faces, vmax, amax, m_cap=8192):
    s = np.ascontiguousarray(start, np.float64).reshape(9)
    g = np.ascontiguousarray(goal, np.float64).reshape(9)
    t = np.ascontiguousarray(t_alloc, np.float64)
    M = len(t)
    n = 15 * M
    polys = np.ascontiguousarray(polys, np.float64)
    nf = np.ascontiguousarray(nfaces, np.int32)
    Q = np.zeros((n, n))
    A = np.zeros((m_cap, n))
    l = np.zeros(m_cap)
    u = np.zeros(m_cap)
    m = lib().orc_qp_assemble(dptr(s), dptr(g), dptr(t), M, dptr(polys), nf.ctypes.data_as(C.POINTER(C.c_int32)),
                              max_faces, C.c_double(vmax), C.c_double(amax), dptr(Q), dptr(A), dptr(l), dptr(u),
                              m_cap)
    A = A.reshape(-1)[:m * n].reshape(m, n).copy()
    return Q, A, l[:m].copy(), u[:m].copy()


def qp_solve(start, goal, t_alloc, polys, nfaces, max_faces, vmax, amax, qs):
    s = np.ascontiguousarray(start, np.float64).reshape(9)
    g = np.ascontiguousarray(goal, np.float64).reshape(9)
    t = np.ascontiguousarray(t_alloc, np.float64)
    M = len(t)
    polys = np.ascontiguousarray(polys, np.float64)
    nf = np.ascontiguousarray(nfaces, np.int32)
    x = np.zeros(15 * M)
    it = C.c_int(0)
    st = lib().orc_qp_solve(dptr(s), dptr(g), dptr(t), M, dptr(polys), nf.ctypes.data_as(C.POINTER(C.c_int32)),
                            max_faces, C.c_double(vmax), C.c_double(amax), C.byref(qs), dptr(x), C.byref(it))
    return st, x, it.value


def osqp_dense(P, q, A, l, u, qs):
    P = np.ascontiguousarray(P, np.float64)
    A = np.ascontiguousarray(A, np.float64)
    q = np.ascontiguousarray(q, np.float64)
    l = np.ascontiguousarray(l, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    n, m = P.shape[0], A.shape[0]
    x = np.zeros(n)
    y = np.zeros(m)
    it = C.c_int(0)
    st = lib().orc_osqp_dense(dptr(P), dptr(q), dptr(A), dptr(l), dptr(u), n, m, C.byref(qs), dptr(x), dptr(y),
                              C.byref(it))
    return st, x, y, it.value


# ---------------------------------------------------------------- full replan
def replan(spec, ap, pp, qs, grid, pose, stamp, start_pva, goal, t_start, drone_id=0):
    pose = np.ascontiguousarray(pose, np.float32)
    s = np.ascontiguousarray(start_pva, np.float64).reshape(9)
    g = np.ascontiguousarray(goal, np.float64)
    rec = _abi.SogmTrajRecord()
    stage = (C.c_int * 1)()
    ok = lib().orc_replan(C.byref(spec), C.byref(ap), C.byref(pp), C.byref(qs), fptr(grid), fptr(pose),
                          C.c_double(stamp), dptr(s), dptr(g), C.c_double(t_start), int(drone_id),
                          C.byref(rec), stage)
    return ok, rec, stage[0]


# ---------------------------------------------------------------- particle-filter SOGM (a6)
class DspOracle:
    """dsp_map::DSPMap restated (oracle/dsp_oracle.cpp), one agent."""

    def __init__(self, spec, params, tables):
        pg, vg, rnd = tables
        L = lib()
        L.orc_dsp_create.restype = C.c_void_p
        self.spec, self.params = spec, params
        self.h = C.c_void_p(L.orc_dsp_create(C.byref(spec), C.byref(params), fptr(pg), fptr(vg), len(pg),
                                             rnd.ctypes.data_as(C.c_void_p), len(rnd)))
        self.V = spec.L * spec.W * spec.H
        self.S = 2 * params.max_particle_num_voxel

    def update(self, points, labels, pos, quat, stamp):
        """labels=None: velocityEstimationThread runs inside the oracle (clustering + association)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        lab = np.ascontiguousarray(labels, np.float32) if labels is not None else None
        return lib().orc_dsp_update(self.h, len(pts), fptr(pts), fptr(lab) if lab is not None else None,
                                    C.c_float(pos[0]), C.c_float(pos[1]),
                                    C.c_float(pos[2]), C.c_double(stamp), C.c_float(quat[0]), C.c_float(quat[1]),
                                    C.c_float(quat[2]), C.c_float(quat[3]))

    def born(self, cap=8192):
        out = np.zeros((cap, 7), np.float32)
        cnt = (C.c_int * 3)()
        n = lib().orc_dsp_born(self.h, fptr(out), cap, cnt)
        return out[:n].copy(), list(cnt)

    def publish(self, threshold, inf_step):
        out = np.zeros((self.V, self.spec.T), np.float32)
        n = lib().orc_dsp_publish(self.h, fptr(out), C.c_float(threshold), inf_step)
        return out, n

    def state(self):
        store = np.zeros((self.V, self.S, 9), np.float32)
        objnum = np.zeros((self.V, 4 + self.spec.T), np.float32)
        counters = np.zeros(16, np.int32)
        lib().orc_dsp_state(self.h, fptr(store), fptr(objnum), counters.ctypes.data_as(C.c_void_p))
        return store, objnum, counters

    def set_state(self, store, last_pos, last_stamp, cursors):
        """orc_dsp_set_state: the meaning of sogm_dsp_upload_state.  Returns 0, or -1 (refused, nothing changed)."""
        st = np.ascontiguousarray(store, np.float32)
        assert st.shape == (self.V, self.S, 9), st.shape
        lp = np.ascontiguousarray(last_pos, np.float32)
        cu = np.ascontiguousarray(cursors, np.int32)
        assert lp.shape == (3,) and cu.shape == (3,)
        return lib().orc_dsp_set_state(self.h, fptr(st), fptr(lp), C.c_double(last_stamp), cu.ctypes.data_as(C.c_void_p))

    def observations(self, NP):
        OM = self.params.obs_max_per_pyramid
        nobs = np.zeros(NP, np.int32)
        pc = np.zeros((NP, OM, 5), np.float32)
        ml = np.zeros(NP, np.float32)
        lib().orc_dsp_observations(self.h, nobs.ctypes.data_as(C.c_void_p), fptr(pc), fptr(ml))
        return nobs, pc, ml

    def close(self):
        if self.h:
            lib().orc_dsp_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- filterPointCloud (a7)
def filter_point_cloud(spec, raw, filter_res=0.15, cap=5000):
    raw = np.ascontiguousarray(raw, np.float32)
    out = np.zeros((cap, 3), np.float32)
    n = lib().orc_filter_point_cloud(C.byref(spec), fptr(raw), len(raw), C.c_float(filter_res), cap, fptr(out))
    return out[:n].copy()


# ---------------------------------------------------------------- isSafeAfterOpt (f3)
def separable(A, B):
    A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64)
    return int(lib().orc_separable(dptr(A), len(A), dptr(B), len(B)))


def safe_after_opt(cpts, M, records, n_records, ego_id, t_now, max_rows=144):
    c = np.ascontiguousarray(cpts, np.float64)
    return int(lib().orc_safe_after_opt(dptr(c), M, records, n_records, ego_id, C.c_double(t_now), max_rows))


# ---------------------------------------------------------------- GridMap depth front end (f1)
class GridMapOracle:
    def __init__(self, params):
        L = lib()
        L.orc_gridmap_create.restype = C.c_void_p
        self.h = C.c_void_p(L.orc_gridmap_create(C.byref(params)))
        nv = np.zeros(3, np.int32)
        L.orc_gridmap_dims(self.h, nv.ctypes.data_as(C.c_void_p))
        self.nv = [int(x) for x in nv]
        self.N = self.nv[0] * self.nv[1] * self.nv[2]

    def update(self, depth, cam, R):
        d = np.ascontiguousarray(depth, np.uint16)
        c = np.ascontiguousarray(cam, np.float64)
        r = np.ascontiguousarray(R, np.float64).reshape(9)
        return int(lib().orc_gridmap_update(self.h, d.ctypes.data_as(C.c_void_p), dptr(c), dptr(r)))

    def force_frame(self, n):
        lib().orc_gridmap_force_frame(self.h, n)

    def state(self):
        occ = np.zeros(self.N, np.float64)
        inf = np.zeros(self.N, np.int8)
        b = np.zeros(6, np.int32)
        lib().orc_gridmap_state(self.h, dptr(occ), inf.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
        return occ, inf, b

    def inflate_occupancy(self, pos):
        p = np.ascontiguousarray(pos, np.float64)
        return int(lib().orc_gridmap_inflate_occupancy(self.h, dptr(p)))

    def close(self):
        if self.h:
            lib().orc_gridmap_destroy(self.h)
            self.h = None


# ---------------------------------------------------------------- isTrajSafe (f2)
def traj_safe(spec, grid, pose, map_stamp, record, t_now, T):
    g = np.ascontiguousarray(grid, np.float32)
    ps = np.ascontiguousarray(pose, np.float32)
    return int(lib().orc_traj_safe(C.byref(spec), fptr(g), fptr(ps), C.c_double(map_stamp), C.byref(record),
                                   C.c_double(t_now), C.c_double(T)))


# ---------------------------------------------------------------- f2: FSM
class OrcFsmState(C.Structure):
    _fields_ = [("status", C.c_int32), ("num_replan_failures", C.c_int32), ("is_success", C.c_int32),
                ("_pad", C.c_int32), ("traj_start_time", C.c_double)]


class OrcFsmConfig(C.Structure):
    _fields_ = [("replan_duration", C.c_double), ("replan_start_time", C.c_double),
                ("replan_max_failures", C.c_int32), ("_pad", C.c_int32)]


class FsmOracle:
    """FiniteStateMachine::FSMCallback for one agent (plan_manager/src/plan_manager.cpp:92-233)."""

    def __init__(self, traj_start_time, replan_duration=0.1, replan_start_time=0.02, replan_max_failures=5):
        self.s = OrcFsmState()
        self.cfg = OrcFsmConfig(replan_duration, replan_start_time, replan_max_failures, 0)
        lib().orc_fsm_init(C.byref(self.s), C.c_double(traj_start_time))

    def tick(self, now, replan_ok, traj_safe, goal_reached):
        """-> None | 'new' | ('hover', start_time)"""
        hs = C.c_double(0.0)
        pub = lib().orc_fsm_tick(C.byref(self.s), C.byref(self.cfg), C.c_double(now), int(replan_ok),
                                 int(traj_safe), int(goal_reached), C.byref(hs))
        return None if pub == 0 else ("new" if pub == 1 else ("hover", hs.value))
