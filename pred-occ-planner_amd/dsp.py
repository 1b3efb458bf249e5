"""Host mirror of dsp_map::DSPMap as owned by RiskVoxel (plan_env/src/risk_voxel.cpp:42-50,237-254),
batched over the agents of a SogmMap.  Forwards to sogm_dsp_* / sogm_update_dsp (include/sogm_abi.h);
no CPU path."""
import ctypes as C

import numpy as np
import torch

from ._abi import (SOGM_DSP_MAX_T, SOGM_VELAUDIT_ACCUMULATE, SOGM_VELAUDIT_ROW, SogmDspParams, SogmVelAuditParams, check,
                   lib)
from .sogm import _stream


def make_dsp_params(T=6):
    """map_parameters.h:5-54 + RiskVoxel::init (risk_voxel.cpp:20-21,42-50)."""
    p = SogmDspParams()
    p.max_particle_num_voxel = 7
    p.half_fov_h, p.half_fov_v, p.angle_resolution = 43, 29, 1
    p.newborn_num = 20
    p.obs_max_per_pyramid = 100
    for t in range(SOGM_DSP_MAX_T):
        p.prediction_times[t] = round(0.3 * (t + 1), 1)  # prediction_future_time {0.3f .. 1.8f}
    p.sigma_observation = 0.05
    p.p_detection = 0.95
    p.kappa = 0.01
    p.newborn_weight = 0.0001
    p.obstacle_thickness = 0.3
    return p


def make_tables(seed, n_gauss=1 << 20, n_rand=1 << 16, p_std=0.05, v_std=0.05):
    """Stand-ins for generateGaussianRandomsVectorZeroCenter (dsp_dynamic.h:1229-1239; N(0, 0.05) after
    setPredictionVariance(0.05, 0.05), risk_voxel.cpp:43) and for rand(): reproducible tables."""
    rng = np.random.default_rng(seed)
    pg = (rng.standard_normal(n_gauss) * p_std).astype(np.float32)
    vg = (rng.standard_normal(n_gauss) * v_std).astype(np.float32)
    rnd = rng.integers(0, 2 ** 31 - 1, size=n_rand, dtype=np.int64).astype(np.int32)
    return pg, vg, rnd


class DspMap:
    def __init__(self, sogm_map, params, tables, max_points=5000):
        self.map = sogm_map
        self.params = params
        pg, vg, rnd = tables
        self._h = C.c_void_p()
        fp = C.POINTER(C.c_float)
        check(lib().sogm_dsp_create(sogm_map.ctx, C.byref(params), pg.ctypes.data_as(fp),
                                    vg.ctypes.data_as(fp), len(pg), rnd.ctypes.data_as(C.c_void_p),
                                    len(rnd), max_points, C.byref(self._h)), "sogm_dsp_create")
        self.max_points = max_points
        self.S = 2 * params.max_particle_num_voxel
        self.NP = (params.half_fov_h * 2 // params.angle_resolution) * (params.half_fov_v * 2 // params.angle_resolution)

    def close(self):
        if self._h:
            torch.cuda.synchronize()
            lib().sogm_dsp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, points, labels, cloud_range, sensor_pos, sensor_quat, stamps, out_ok=None):
        """DSPMap::update for every agent; all arguments are device tensors (see sogm_abi.h).  labels=None runs
        velocityEstimationThread (clustering + association) on the GPU."""
        ok = out_ok if out_ok is not None else torch.zeros(self.map.n_agents, dtype=torch.int32, device=points.device)
        check(lib().sogm_update_dsp(self._h, points.data_ptr(), labels.data_ptr() if labels is not None else None,
                                    cloud_range.data_ptr(),
                                    sensor_pos.data_ptr(), sensor_quat.data_ptr(), stamps.data_ptr(),
                                    ok.data_ptr(), _stream()), "sogm_update_dsp")
        return ok

    def download_born(self, agent):
        """input_cloud_with_velocity of the last update: (rows [n, 7], counters {clusters, dynamic, matched, err})."""
        cap = self.max_points
        born = np.zeros((cap, 7), np.float32)
        n = C.c_int32(0)
        cnt = (C.c_int32 * 4)()
        check(lib().sogm_dsp_download_born(self._h, agent, born.ctypes.data_as(C.c_void_p), cap, C.byref(n), cnt),
              "sogm_dsp_download_born")
        return born[:n.value].copy(), list(cnt)

    def download_born_source(self, agent):
        """The source index of download_born's rows (sogm_dsp_download_born_source): row k of the list came from input point
        src[k] of the agent's range.  The identity after an update with labels."""
        src = np.zeros(self.max_points, np.int32)
        n = C.c_int32(0)
        check(lib().sogm_dsp_download_born_source(self._h, agent, src.ctypes.data_as(C.c_void_p), self.max_points,
                                                  C.byref(n)), "sogm_dsp_download_born_source")
        return src[:n.value].copy()

    def audit_velocity(self, truth_labels, truth_code, cloud_range, n_codes=0, speed_tolerance=0.25, per_code=False,
                       accumulate_into=None):
        """sogm_dsp_velocity_audit (sogm_abi.h "velocity audit") of the last update: device tensors (rows int64 [n_agents, 32],
        per-code table int64 [n_agents, n_codes + 2, 6] or None).  truth_labels [points, 4] and truth_code [points] (or None)
        are in the order of the cloud that update was given, cloud_range is its range.  accumulate_into = (rows, table or None)
        of an earlier call: the counts are added to them and they are returned."""
        A = self.map.n_agents
        prm = SogmVelAuditParams()
        prm.speed_tolerance, prm.n_codes = speed_tolerance, n_codes
        if accumulate_into is not None:
            rows, table = accumulate_into
            prm.flags = SOGM_VELAUDIT_ACCUMULATE
            assert rows.dtype == torch.int64 and rows.is_contiguous() and tuple(rows.shape) == (A, SOGM_VELAUDIT_ROW)
            assert (table is not None) == bool(per_code)
        else:
            rows = torch.empty((A, SOGM_VELAUDIT_ROW), dtype=torch.int64, device=truth_labels.device)
            table = torch.empty((A, n_codes + 2, 6), dtype=torch.int64, device=truth_labels.device) if per_code else None
        if table is not None:
            assert table.dtype == torch.int64 and table.is_contiguous() and tuple(table.shape) == (A, n_codes + 2, 6)
        check(lib().sogm_dsp_velocity_audit(self._h, truth_labels.data_ptr(),
                                            truth_code.data_ptr() if truth_code is not None else None,
                                            cloud_range.data_ptr(), C.byref(prm), rows.data_ptr(),
                                            table.data_ptr() if table is not None else None, _stream()),
              "sogm_dsp_velocity_audit")
        return rows, table

    def publish(self):
        """RiskVoxel::publishMap's map half: future status -> SOGM grid (+ inflate-kernel zeroing)."""
        n = torch.zeros(self.map.n_agents, dtype=torch.int32, device="cuda")
        check(lib().sogm_dsp_publish(self._h, n.data_ptr(), _stream()), "sogm_dsp_publish")
        return n

    def download_state(self, agent):
        V, T = self.map.V, self.map.spec.T
        store = np.zeros((V, self.S, 9), np.float32)
        objnum = np.zeros((V, 4 + T), np.float32)
        counters = np.zeros(16, np.int32)
        check(lib().sogm_dsp_download_state(self._h, agent, store.ctypes.data_as(C.c_void_p),
                                            objnum.ctypes.data_as(C.c_void_p),
                                            counters.ctypes.data_as(C.c_void_p)), "sogm_dsp_download_state")
        return store, objnum, counters

    def upload_state(self, agent, store, last_pos, last_stamp, cursors):
        """Test hook (sogm_dsp_upload_state): a between-updates store [V, 2*max, 9] (flags 0 / 0.6 / 1, vz 0) becomes the
        agent's; last_pos / last_stamp the previous update's pose; cursors = (p_seq, v_seq, rand_seq).  Returns the status
        (SOGM_OK or SOGM_ERR_INVALID_ARG: nothing changed) instead of raising: tests assert both."""
        st = np.ascontiguousarray(store, np.float32)
        assert st.shape == (self.map.V, self.S, 9), st.shape
        lp = np.ascontiguousarray(last_pos, np.float32)
        cu = np.ascontiguousarray(cursors, np.int32)
        assert lp.shape == (3,) and cu.shape == (3,)
        return lib().sogm_dsp_upload_state(self._h, agent, st.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p),
                                           C.c_double(last_stamp), cu.ctypes.data_as(C.c_void_p))

    def download_observations(self, agent):
        OM = self.params.obs_max_per_pyramid
        nobs = np.zeros(self.NP, np.int32)
        pc = np.zeros((self.NP, OM, 5), np.float32)
        ml = np.zeros(self.NP, np.float32)
        check(lib().sogm_dsp_download_observations(self._h, agent, nobs.ctypes.data_as(C.c_void_p),
                                                   pc.ctypes.data_as(C.c_void_p), ml.ctypes.data_as(C.c_void_p)),
              "sogm_dsp_download_observations")
        return nobs, pc, ml


def velocity_scores(rows):
    """What a velocity-audit row (or rows: they are summed) says, as a dict.  `detected` = TRACKED or UNTRACKED: the estimator
    took the point for something that moves.  Ratios with an empty denominator are None."""
    r = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows, np.int64).reshape(-1, SOGM_VELAUDIT_ROW).sum(axis=0)
    conf = r[4:12].reshape(2, 4)                      # [truth still, moving][static, tracked, untracked, dropped]
    moving, still = int(conf[1].sum()), int(conf[0].sum())
    det_moving, det_still = int(conf[1, 1] + conf[1, 2]), int(conf[0, 1] + conf[0, 2])
    scored = int(r[12:18].sum())                      # MOVING x TRACKED rows that are not NaN

    def ratio(a, b):
        return float(a) / float(b) if b else None

    return {
        "n_in": int(r[0]), "n_born": int(r[1]), "moving": moving, "still": still,
        "detection_precision": ratio(det_moving, det_moving + det_still),
        "detection_recall": ratio(det_moving, moving),
        "tracked_share_of_moving": ratio(int(conf[1, 1]), moving),
        "dropped_share": ratio(int(conf[0, 3] + conf[1, 3]), int(r[0])),
        "dropped_share_of_moving": ratio(int(conf[1, 3]), moving),
        "rms_error": (float(r[29]) * 1e-6 / scored) ** 0.5 if scored else None,
        "within_tolerance_share": ratio(int(r[30]), scored),
    }
