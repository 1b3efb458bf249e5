"""ctypes binding of include/sogm_abi.h (the C-ABI drop-in boundary).

The HIP library is REQUIRED: importing this module without ``libsogm_hip.so`` raises — there is no
CPU fallback in the product path.  Plain-data records mirror the C structs field for field.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SOGM_LIB_PATH: another build of the same ABI, for same-box A/B runs of two library versions — tools/micro/ab.sh)
LIB_PATH = os.environ.get("SOGM_LIB_PATH") or os.path.join(_HERE, "libsogm_hip.so")

SOGM_ABI_VERSION = 6  # include/sogm_abi.h; load_library() refuses a library of another version
SOGM_MAX_PIECES = 16
SOGM_MAP_FAKE = 0
SOGM_MAP_RISKBASE = 1
SOGM_MAP_RISKVOXEL = 2
SOGM_STORE_F32, SOGM_STORE_F16 = 0, 1
SOGM_LAYOUT_TILED = 16  # OR-ed into SogmSpec.storage: 2 x 2 x 2 cell tiles
SOGM_DSP_MAX_T = 16

SOGM_OK = 0
SOGM_ERR_INVALID_ARG = -1
SOGM_ERR_NO_DEVICE = -2
SOGM_ERR_HIP = -3
SOGM_ERR_CAPACITY = -4
SOGM_ERR_STATE = -5
SOGM_ERR_COMM = -6
SOGM_COMM_ID_BYTES = 128
PROF_CLEAR, PROF_STAMP, PROF_SPLAT, PROF_ASTAR, PROF_CORRIDOR, PROF_QP, PROF_CLEAR_HEAD, PROF_EXCHANGE, PROF_N = range(9)

COUNTER_NAMES = ("replan_ok", "fail_search", "fail_corridor", "fail_qp", "fail_unsafe", "corridor_capacity",
                 "pieces_capacity", "deconflict_capacity")

# ASTAR_RET (path_searching/include/path_searching/dyn_a_star.h:15)
ASTAR_NO_PATH, ASTAR_INIT_ERR, ASTAR_SEARCH_ERR, ASTAR_REACH_HORIZON, ASTAR_REACH_END, ASTAR_NEAR_END = range(6)


class SogmSpec(C.Structure):
    _fields_ = [("L", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("T", C.c_int32),
                ("resolution", C.c_float), ("time_resolution", C.c_float),
                ("risk_threshold", C.c_float), ("clearance", C.c_float),
                ("ground_height", C.c_float), ("ceiling_height", C.c_float),
                ("risk_threshold_region", C.c_float), ("risk_thres_reg_decay", C.c_float),
                ("risk_thres_vox_decay", C.c_float), ("map_kind", C.c_int32),
                ("storage", C.c_int32)]


class SogmDspParams(C.Structure):
    _fields_ = [("max_particle_num_voxel", C.c_int32), ("half_fov_h", C.c_int32),
                ("half_fov_v", C.c_int32), ("angle_resolution", C.c_int32),
                ("newborn_num", C.c_int32), ("obs_max_per_pyramid", C.c_int32),
                ("prediction_times", C.c_float * SOGM_DSP_MAX_T),
                ("sigma_observation", C.c_float), ("p_detection", C.c_float), ("kappa", C.c_float),
                ("newborn_weight", C.c_float), ("obstacle_thickness", C.c_float)]


class SogmGridMapParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("map_size", C.c_double * 3), ("local_update_range", C.c_double * 3),
                ("obstacles_inflation", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("depth_filter_maxdist", C.c_double), ("depth_filter_mindist", C.c_double),
                ("k_depth_scaling_factor", C.c_double), ("p_hit", C.c_double), ("p_miss", C.c_double),
                ("p_min", C.c_double), ("p_max", C.c_double), ("p_occ", C.c_double), ("max_ray_length", C.c_double),
                ("virtual_ceil_height", C.c_double), ("ground_height", C.c_double),
                ("use_depth_filter", C.c_int32), ("depth_filter_margin", C.c_int32), ("skip_pixel", C.c_int32),
                ("local_map_margin", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32)]


class SogmDepthCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("max_depth", C.c_double), ("depth_scale", C.c_double), ("ground_z", C.c_double),
                ("rows", C.c_int32), ("cols", C.c_int32), ("use_ground", C.c_int32), ("flags", C.c_int32)]


class SogmDepthBodies(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("cam_body", C.c_void_p), ("size", C.c_double * 3),
                ("n_bodies", C.c_int32), ("reserved_", C.c_int32)]


class SogmDepthNoise(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("frame", C.c_uint64), ("agent_base", C.c_int32), ("flags", C.c_int32),
                ("sigma0", C.c_double), ("sigma1", C.c_double), ("sigma2", C.c_double), ("p_drop", C.c_double),
                ("edge_jump", C.c_double), ("p_edge", C.c_double), ("min_depth", C.c_double)]


class SogmLinkParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("p_loss", C.c_double), ("range", C.c_double), ("delay_min", C.c_int32),
                ("delay_max", C.c_int32), ("flags", C.c_int32), ("reserved_", C.c_int32)]


class SogmTrajNoise(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("sigma_loc", C.c_double * 3), ("sigma_time", C.c_double), ("sigma_track", C.c_double),
                ("loc_hold", C.c_int32), ("reserved_", C.c_int32)]


class SogmBeliefParams(C.Structure):
    _fields_ = [("dt_sample", C.c_double), ("edges", C.c_double * 5), ("n_samples", C.c_int32), ("reserved_", C.c_int32)]


class SogmLinkBuffers(C.Structure):
    _fields_ = [("ring_table", C.c_void_p), ("ring_pos", C.c_void_p), ("views", C.c_void_p), ("held_tick", C.c_void_p),
                ("counters", C.c_void_p)]


class SogmCylinder(C.Structure):
    _fields_ = [("type", C.c_int32), ("_pad", C.c_int32)] + [
        (k, C.c_double) for k in ("x", "y", "z", "w", "h", "vx", "vy", "qw", "qx", "qy", "qz")]


class SogmLabelSources(C.Structure):
    _fields_ = [("cylinders", C.c_void_p), ("body_vel", C.c_void_p), ("n_cyl", C.c_int32), ("n_bodies", C.c_int32),
                ("min_speed", C.c_float), ("reserved_", C.c_int32)]


class SogmTrajRecord(C.Structure):
    _fields_ = [("drone_id", C.c_int32), ("n_pieces", C.c_int32), ("time_start", C.c_double),
                ("duration", C.c_double * SOGM_MAX_PIECES),
                ("cpts", C.c_double * (SOGM_MAX_PIECES * 15))]


class SogmAstarParams(C.Structure):
    _fields_ = [("max_tau", C.c_double), ("max_vel", C.c_double), ("max_acc", C.c_double),
                ("w_time", C.c_double), ("horizon", C.c_double), ("lambda_heu", C.c_double),
                ("resolution", C.c_double), ("time_resolution", C.c_double),
                ("allocate_num", C.c_int32), ("check_num", C.c_int32), ("tolerance", C.c_int32),
                ("shot_ignores_time", C.c_int32)]


class SogmPlannerParams(C.Structure):
    _fields_ = [("corridor_tau", C.c_double), ("init_range", C.c_double),
                ("shrink_size", C.c_double), ("opt_max_vel", C.c_double),
                ("opt_max_acc", C.c_double), ("fake_planner", C.c_int32),
                ("firi_iterations", C.c_int32), ("pc_capacity", C.c_int32),
                ("max_faces", C.c_int32)]


class SogmQpSettings(C.Structure):
    _fields_ = [("rho", C.c_double), ("sigma", C.c_double), ("alpha", C.c_double),
                ("eps_abs", C.c_double), ("eps_rel", C.c_double), ("max_iter", C.c_int32),
                ("check_termination", C.c_int32), ("scaling_iters", C.c_int32),
                ("adaptive_rho_interval", C.c_int32), ("residual_fp32", C.c_int32), ("reserved_", C.c_int32)]


class SogmWorld(C.Structure):
    _fields_ = [("cloud_xyz", C.c_void_p), ("block_bounds", C.c_void_p), ("cylinders", C.c_void_p),
                ("n_points", C.c_int32), ("n_blocks", C.c_int32), ("block_points", C.c_int32), ("n_cyl", C.c_int32)]


class SogmWorldTimeline(C.Structure):
    _fields_ = [("cloud0", C.c_void_p), ("owner", C.c_void_p), ("cylinders0", C.c_void_p),
                ("n_points", C.c_int32), ("n_cyl", C.c_int32), ("block_points", C.c_int32), ("moving", C.c_int32),
                ("dt", C.c_double)]


class SogmPrestamp(C.Structure):
    _fields_ = [("cloud_xyz", C.c_void_p), ("cloud_range", C.c_void_p), ("cylinders", C.c_void_p),
                ("n_cyl", C.c_int32), ("reserved_", C.c_int32), ("next_stamp", C.c_double),
                ("replan_start_offset", C.c_double), ("hover_inout", C.c_void_p), ("out_now", C.c_void_p),
                ("out_t_start", C.c_void_p), ("out_pva", C.c_void_p), ("out_poses", C.c_void_p),
                ("world", C.POINTER(SogmWorld))]


class SogmFlight(C.Structure):
    _fields_ = [("n_ticks", C.c_int32), ("first_tick", C.c_int32), ("t0", C.c_double), ("period", C.c_double),
                ("replan_start_offset", C.c_double), ("worlds", C.POINTER(SogmWorld)), ("goals", C.c_void_p),
                ("drone_ids", C.c_void_p), ("hover_inout", C.c_void_p), ("own_inout", C.c_void_p),
                ("tables", C.c_void_p), ("n_total", C.c_int32), ("agent0", C.c_int32), ("log_records", C.c_void_p),
                ("log_ok", C.c_void_p), ("nccl_comm", C.c_void_p)]


class SogmAuditParams(C.Structure):
    _fields_ = [("body", C.c_double * 3), ("sample_dt", C.c_double), ("goal_tolerance", C.c_double),
                ("t_obstacles", C.c_double), ("event_capacity", C.c_int32), ("flags", C.c_int32)]


class SogmAuditAgent(C.Structure):
    _fields_ = [("min_gap", C.c_double), ("min_gap_time", C.c_double), ("min_sep", C.c_double),
                ("min_sep_time", C.c_double), ("goal_time", C.c_double), ("first_collision_time", C.c_double),
                ("path_length", C.c_double), ("last_pos", C.c_double * 3), ("min_gap_obstacle", C.c_int32),
                ("min_sep_agent", C.c_int32), ("obstacle_samples", C.c_int32), ("agent_samples", C.c_int32),
                ("n_samples", C.c_int32), ("has_last", C.c_int32)]


class SogmAuditEvent(C.Structure):
    _fields_ = [("t", C.c_double), ("agent", C.c_int32), ("other", C.c_int32), ("kind", C.c_int32),
                ("reserved_", C.c_int32)]


SOGM_AUDIT_AGENT, SOGM_AUDIT_OBSTACLE = 0, 1
SOGM_DEPTH_RINGS, SOGM_AUDIT_RINGS = 1, 1   # SogmDepthCamera.flags, SogmAuditParams.flags
AUDIT_AGENT_BYTES = C.sizeof(SogmAuditAgent)  # 104
AUDIT_EVENT_BYTES = C.sizeof(SogmAuditEvent)  # 24

# map audit (include/sogm_abi.h "map audit")
SOGM_MAPAUDIT_FRUSTUM = 1
SOGM_MAPAUDIT_CENTRE, SOGM_MAPAUDIT_SKIPPED = 1, 2
SOGM_MAPAUDIT_MAX_T = 32


class SogmMapAuditParams(C.Structure):
    _fields_ = [("thr_test", C.c_float), ("thr_truth", C.c_float), ("tolerance", C.c_int32), ("flags", C.c_int32),
                ("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("slab_layers", C.c_int32), ("reserved_", C.c_int32),
                ("near_z", C.c_double), ("far_z", C.c_double), ("tan_h", C.c_double), ("tan_v", C.c_double),
                ("slice_map", C.c_int32 * SOGM_MAPAUDIT_MAX_T)]


MAPAUDIT_ROW_FIELDS = ("n_region", "n_test", "n_truth", "n_both", "n_test_near", "n_truth_near", "truth_slice", "status")
MAPAUDIT_PARAMS_BYTES = C.sizeof(SogmMapAuditParams)  # 208

# view mask (include/sogm_abi.h "view mask"): the classes, and their bits in SogmViewParams.classes
SOGM_VIEW_OUTSIDE, SOGM_VIEW_OFFIMAGE, SOGM_VIEW_FREE, SOGM_VIEW_SURFACE, SOGM_VIEW_HIDDEN = 0, 1, 2, 3, 4
SOGM_VIEWBIT_OUTSIDE, SOGM_VIEWBIT_OFFIMAGE, SOGM_VIEWBIT_FREE, SOGM_VIEWBIT_SURFACE, SOGM_VIEWBIT_HIDDEN = 1, 2, 4, 8, 16
SOGM_VIEWBIT_ALL = 31
VIEW_CLASS_NAMES = ("outside", "offimage", "free", "surface", "hidden")


class SogmViewParams(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("depth_scale", C.c_double),
                ("max_depth", C.c_double), ("near_z", C.c_double), ("far_z", C.c_double), ("tan_h", C.c_double),
                ("tan_v", C.c_double), ("band", C.c_double), ("rows", C.c_int32), ("cols", C.c_int32), ("classes", C.c_int32),
                ("reserved_", C.c_int32)]


VIEW_PARAMS_BYTES = C.sizeof(SogmViewParams)  # 104

# velocity audit (include/sogm_abi.h "velocity audit"): estimate classes, status bits, the flag, the row's layout
SOGM_VELAUDIT_ROW = 32
SOGM_VEL_STATIC, SOGM_VEL_TRACKED, SOGM_VEL_UNTRACKED, SOGM_VEL_DROPPED = 0, 1, 2, 3
SOGM_VELAUDIT_SKIPPED, SOGM_VELAUDIT_BAD_SOURCE, SOGM_VELAUDIT_CLIPPED = 1, 2, 4
SOGM_VELAUDIT_ACCUMULATE = 1
VEL_ESTIMATE_NAMES = ("static", "tracked", "untracked", "dropped")
VELAUDIT_CODE_COLUMNS = ("static", "tracked", "untracked", "dropped", "n_within", "sum_e2_um")


class SogmVelAuditParams(C.Structure):
    _fields_ = [("speed_tolerance", C.c_float), ("n_codes", C.c_int32), ("flags", C.c_int32), ("reserved_", C.c_int32)]


VELAUDIT_PARAMS_BYTES = C.sizeof(SogmVelAuditParams)  # 16


class SogmFsmParams(C.Structure):
    _fields_ = [("replan_duration", C.c_double), ("replan_start_time", C.c_double), ("goal_tolerance", C.c_double),
                ("new_plan_interval", C.c_double), ("replan_max_failures", C.c_int32), ("reserved_", C.c_int32)]


class SogmFsmState(C.Structure):
    _fields_ = [("traj_start", C.c_double), ("status", C.c_int32), ("fail", C.c_int32), ("success", C.c_int32),
                ("reserved_", C.c_int32)]


class SogmFlightFsm(C.Structure):
    _fields_ = [("prm", SogmFsmParams), ("check_duration", C.c_double), ("state_inout", C.c_void_p),
                ("log_state", C.c_void_p), ("log_due", C.c_void_p), ("log_safe", C.c_void_p), ("log_reached", C.c_void_p),
                ("log_pub", C.c_void_p), ("log_hover_start", C.c_void_p), ("log_own", C.c_void_p)]


FSM_STATE_BYTES = C.sizeof(SogmFsmState)  # 24
FSM_PUB_NONE, FSM_PUB_NEW, FSM_PUB_HOVER = 0, 1, 2  # sogm_fsm_apply's out_pub

# trajectory server (include/sogm_abi.h "trajectory server")
SOGM_TRAJSRV_QUEUE = 256
SOGM_CMD_PUBLISHED, SOGM_CMD_HELD = 1, 2


class SogmTrajServerParams(C.Structure):
    _fields_ = [("replan_threshold", C.c_double), ("sample_dt", C.c_double), ("yaw_pi", C.c_double),
                ("yaw_dot_max", C.c_double), ("yaw_mode", C.c_int32), ("reserved_", C.c_int32)]


class SogmTrajPoint(C.Structure):
    _fields_ = [("t", C.c_double), ("pos", C.c_double * 3), ("vel", C.c_double * 3), ("acc", C.c_double * 3),
                ("yaw", C.c_double), ("yaw_dot", C.c_double)]


class SogmPositionCommand(C.Structure):
    _fields_ = [("t_pub", C.c_double), ("t_sample", C.c_double), ("pos", C.c_double * 3), ("vel", C.c_double * 3),
                ("acc", C.c_double * 3), ("yaw", C.c_double), ("yaw_dot", C.c_double), ("traj_id", C.c_int32),
                ("flags", C.c_int32)]


class SogmTrajServerCore(C.Structure):
    _fields_ = [("ts", C.c_double), ("te", C.c_double), ("duration", C.c_double), ("last_yaw", C.c_double),
                ("last_yawdot", C.c_double), ("init_pos", C.c_double * 3), ("head", C.c_int32), ("size", C.c_int32),
                ("traj_id", C.c_int32), ("received", C.c_int32), ("overflow", C.c_int32), ("reserved_", C.c_int32 * 3)]


FLIGHT_MAX_TICKS = 64
RULES_PARALLEL = 1  # sogm_corridor_rules_batched_flags: SOGM_RULES_PARALLEL
FINISH_WAVE = 1  # sogm_finish_batched: SOGM_FINISH_WAVE
FLIGHT_HDR_ERR, FLIGHT_HDR_FINISHED, FLIGHT_HDR_LATE_WGS = 4, 5, 15  # sogm_flight_stats out_hdr indices
FLIGHT_STAT_NAMES = ("gate_wait", "map", "search", "corridor", "qp", "finish", "chain", "ticks")
TRAJ_RECORD_BYTES = C.sizeof(SogmTrajRecord)  # 2064
CYLINDER_BYTES = C.sizeof(SogmCylinder)  # 96
DEPTH_CAMERA_BYTES = C.sizeof(SogmDepthCamera)  # 72
DEPTH_BODIES_BYTES = C.sizeof(SogmDepthBodies)  # 48
SOGM_HIT_GROUND, SOGM_HIT_NONE = -1, -2   # out_hit of sogm_render_depth_swarm
DEPTH_NOISE_BYTES = C.sizeof(SogmDepthNoise)  # 80
DEPTH_NOISE_COUNTERS = ("returns_in", "drop_uniform", "drop_edge", "below_min", "beyond_max", "returns_out")
LABEL_SOURCES_BYTES = C.sizeof(SogmLabelSources)  # 32
# radio links (include/sogm_abi.h "radio links")
SOGM_LINK_MAX_DELAY, SOGM_LINK_NEWEST_WINS, SOGM_LINK_COUNTERS = 7, 1, 8
LINK_PARAMS_BYTES = C.sizeof(SogmLinkParams)  # 40
LINK_COUNTER_NAMES = ("sent", "out_of_range", "lost", "arrivals", "applied", "stale", "age_sum", "unheard")
# message noise and belief audit (include/sogm_abi.h "message noise", "belief audit")
TRAJ_NOISE_BYTES = C.sizeof(SogmTrajNoise)  # 56
SOGM_BELIEF_COUNTERS, SOGM_BELIEF_MAX_SAMPLES = 12, 16
BELIEF_PARAMS_BYTES = C.sizeof(SogmBeliefParams)  # 56
BELIEF_COUNTER_NAMES = ("compared", "unheard", "phantom", "samples", "bin0", "bin1", "bin2", "bin3", "bin4", "bin5", "sum_q",
                        "max_q")


class SogmTrajServerState(C.Structure):
    _fields_ = [("core", SogmTrajServerCore), ("traj", SogmTrajRecord)]


TRAJ_POINT_BYTES = C.sizeof(SogmTrajPoint)  # 96
POSITION_COMMAND_BYTES = C.sizeof(SogmPositionCommand)  # 112
TRAJSRV_STATE_BYTES = C.sizeof(SogmTrajServerState)  # 96 + 2064

_vp = C.c_void_p
_i = C.c_int

# name -> (restype, argtypes); every symbol include/sogm_abi.h declares
# slots of the per-agent record of sogm_debug_qp_stats (the enum SOGM_QP_STAT_* of sogm_abi_debug.h)
QP_STAT_TOTAL, QP_STAT_SETUP, QP_STAT_REFAC, QP_STAT_N_REFAC, QP_STAT_CHECK, QP_STAT_N_CHECK, QP_STAT_ITERS, QP_STAT_PATH = range(8)
QP_STAT_FACTOR_ASM, QP_STAT_FACTOR_FWD, QP_STAT_FACTOR_BWD, QP_STAT_SHADER_CLOCKS = 8, 9, 10, 11
QP_STAT_CHECK_STAGE, QP_STAT_CHECK_RESID, QP_STAT_SETUP_SPLIT, QP_STAT_N = 12, 13, 14, 16

PROTOTYPES = {
    "sogm_abi_version": (_i, []),
    "sogm_last_error": (C.c_char_p, []),
    "sogm_device_count": (_i, []),
    "sogm_create": (_i, [C.POINTER(SogmSpec), _i, _i, C.POINTER(_vp)]),
    "sogm_destroy": (None, [_vp]),
    "sogm_grid_bytes": (C.c_int64, [_vp]),
    "sogm_grid_ptr": (_vp, [_vp]),
    "sogm_set_sparse_reset": (_i, [_vp, _i, _i]),
    "sogm_sparse_reset_state": (_i, [_vp, _vp]),
    "sogm_grid_history": (_i, [_vp, _vp]),
    "sogm_map_traffic": (_i, [_vp, _vp, _i]),
    "sogm_set_resample": (_i, [_vp, C.c_float, _i, _vp, _i]),
    "sogm_set_tuning": (_i, [_vp, C.c_char_p, C.c_double]),
    "sogm_get_tuning": (_i, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    "sogm_tuning_key": (C.c_char_p, [_i]),
    "sogm_set_body_particles": (_i, [_vp, C.POINTER(C.c_double), _i]),
    "sogm_set_overlap_clear": (_i, [_vp, _i]),
    "sogm_set_profiling": (_i, [_vp, _i]),
    "sogm_set_profiling_slots": (_i, [_vp, _i]),
    "sogm_profile_read": (_i, [_vp, C.POINTER(C.c_double)]),
    "sogm_profile_read_all": (_i, [_vp, _i, C.POINTER(C.c_double), _i, C.POINTER(_i)]),
    "sogm_update_gt": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "sogm_project_neighbours": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sogm_update_gt_swarm": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    "sogm_device_clock": (_i, [_vp, C.POINTER(C.c_int64), _vp]),
    "sogm_tick_clock": (_i, [_vp, C.POINTER(C.c_int64)]),
    "sogm_cloud_block_bounds": (_i, [_vp, _i, _i, _vp, _vp]),
    "sogm_update_world": (_i, [_vp, C.POINTER(SogmWorld), _vp, _vp, _vp, _i, _vp, _vp]),
    "sogm_world_frames": (_i, [C.POINTER(SogmWorldTimeline), _i, _i, C.POINTER(SogmWorld), _vp]),
    "sogm_set_future_risk": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "sogm_download_reference_layout": (_i, [_vp, _i, _vp]),
    "sogm_tick_inputs": (_i, [_vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_merge_latest": (_i, [_vp, _vp, _vp, _vp, _i, _vp]),
    "sogm_fsm_init": (_i, [_vp, _i, C.c_double, _vp]),
    "sogm_fsm_inputs": (_i, [C.POINTER(SogmFsmParams), _vp, _vp, _vp, _i, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                             _vp, _vp]),
    "sogm_fsm_apply": (_i, [C.POINTER(SogmFsmParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i,
                            C.c_double, _vp]),
    "sogm_map_state": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_float), _vp]),
    "sogm_traj_eval": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "sogm_firi_batched": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _i, C.c_double, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sogm_planner_select_agents": (_i, [_vp, _i, _i]),
    "sogm_planner_set_search_mode": (_i, [_vp, _i]),
    "sogm_query_clear": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "sogm_obstacle_points": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "sogm_planner_create": (_i, [_vp, C.POINTER(SogmAstarParams), C.POINTER(SogmPlannerParams),
                                 C.POINTER(SogmQpSettings), C.POINTER(_vp)]),
    "sogm_planner_destroy": (None, [_vp]),
    "sogm_astar_search": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp]),
    "sogm_corridor_generate": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "sogm_bezier_qp_solve": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_bezier_qp_solve_timed": (_i, [_vp, _vp, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_linprog_batched": (_i, [_i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "sogm_corridor_rules_batched": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp]),
    "sogm_corridor_rules_batched_flags": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _vp, _i, _vp]),
    "sogm_finish_batched": (_i, [_vp, C.c_double, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp,
                                 _vp, _vp, _i, _vp]),
    "sogm_debug_corridor_pairs": (_i, [_vp, _vp]),
    "sogm_debug_streams_held": (_i, [_vp]),
    "sogm_debug_qp_stats": (_i, [_vp, _vp]),  # [A][QP_STAT_N] int64
    "sogm_debug_qp_layout": (_i, [_vp, _i, _vp, _vp]),
    "sogm_replan": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_gridmap_create": (_i, [C.POINTER(SogmGridMapParams), _i, _i, C.POINTER(_vp)]),
    "sogm_gridmap_destroy": (None, [_vp]),
    "sogm_gridmap_update": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_gridmap_query_inflate": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "sogm_render_depth": (_i, [C.POINTER(SogmWorld), C.POINTER(SogmDepthCamera), _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_render_depth_swarm": (_i, [C.POINTER(SogmWorld), C.POINTER(SogmDepthCamera), C.POINTER(SogmDepthBodies), _i, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_depth_noise": (_i, [C.POINTER(SogmDepthCamera), C.POINTER(SogmDepthNoise), _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_gridmap_download": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "sogm_gridmap_force_frame": (_i, [_vp, _i]),
    "sogm_traj_safe": (_i, [_vp, _vp, _vp, C.c_double, _vp, _vp]),
    "sogm_safe_after_opt": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "sogm_planner_flow_error": (_i, [_vp]),
    "sogm_planner_flow_failures": (_i, [_vp, _vp]),
    "sogm_planner_set_publish": (_i, [_vp, _vp, _vp]),
    "sogm_planner_set_prestamp": (_i, [_vp, _vp]),
    "sogm_prestamp_pending": (_i, [_vp]),
    "sogm_prestamp_join": (_i, [_vp, _vp]),
    "sogm_update_prestamped": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sogm_planner_counters": (_i, [_vp, C.POINTER(C.c_int64), _i]),
    "sogm_flight_run": (_i, [_vp, C.POINTER(SogmFlight), _vp]),
    "sogm_flight_prepare": (_i, [_vp, _i]),
    "sogm_flight_stats": (_i, [_vp, _vp, _vp]),
    "sogm_planner_set_swarm": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sogm_planner_set_due": (_i, [_vp, _vp]),
    "sogm_planner_set_flight_fsm": (_i, [_vp, C.POINTER(SogmFlightFsm)]),
    "sogm_audit_init_agents": (_i, [_vp, _i, _vp]),
    "sogm_swarm_audit": (_i, [C.POINTER(SogmAuditParams), _vp, _i, _i, _vp, C.c_double, _i, C.c_double, _i, _i, _vp, _vp,
                              _vp, _i, _vp, _vp, _vp, _vp]),
    "sogm_map_audit_default_params": (_i, [_i, _i, C.POINTER(SogmMapAuditParams)]),
    "sogm_map_audit": (_i, [_vp, _vp, C.POINTER(SogmMapAuditParams), _vp, _vp, _vp, _vp]),
    "sogm_view_default_params": (_i, [C.POINTER(SogmDepthCamera), C.POINTER(SogmViewParams)]),
    "sogm_view_mask": (_i, [_vp, C.POINTER(SogmViewParams), _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_map_audit_masked": (_i, [_vp, _vp, C.POINTER(SogmMapAuditParams), _vp, _vp, _vp, _vp]),
    "sogm_traj_server_init": (_i, [_vp, _vp, _i, C.c_double, _vp, _vp, _vp]),
    "sogm_traj_server_run": (_i, [C.POINTER(SogmTrajServerParams), _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, C.c_double, _i,
                                  C.c_double, C.c_double, _vp, _vp]),
    "sogm_camera_poses": (_i, [_vp, _i, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), _vp, _vp, _vp]),
    "sogm_link_default_params": (_i, [C.POINTER(SogmLinkParams)]),
    "sogm_link_init": (_i, [C.POINTER(SogmLinkParams), _i, _i, C.POINTER(SogmLinkBuffers), _vp]),
    "sogm_link_deliver": (_i, [C.POINTER(SogmLinkParams), _i, _i, _vp, _vp, _i, _i, _i, C.POINTER(SogmLinkBuffers), _vp]),
    "sogm_traj_noise_default_params": (_i, [C.POINTER(SogmTrajNoise)]),
    "sogm_traj_noise": (_i, [C.POINTER(SogmTrajNoise), _i, _vp, _i, _vp, _vp, _vp]),
    "sogm_belief_default_params": (_i, [C.POINTER(SogmBeliefParams)]),
    "sogm_belief_audit": (_i, [C.POINTER(SogmBeliefParams), _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "sogm_project_neighbours_views": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sogm_update_world_views": (_i, [_vp, C.POINTER(SogmWorld), _vp, _vp, _vp, _i, _vp, _vp]),
    "sogm_safe_after_opt_views": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "sogm_planner_set_swarm_views": (_i, [_vp, _vp, _i, _vp, _vp]),
    "sogm_traj_allgather": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "sogm_exchange_wait": (_i, [_vp, _vp]),
    "sogm_comm_unique_id": (_i, [C.c_char_p]),
    "sogm_comm_create": (_i, [C.c_char_p, _i, _i, _i, C.POINTER(_vp)]),
    "sogm_comm_destroy": (None, [_vp]),
    "sogm_comm_handle": (_vp, [_vp]),
    "sogm_comm_info": (_i, [_vp, _vp]),
    "sogm_filter_point_cloud": (_i, [_vp, _vp, _vp, C.c_float, _i, _vp, _vp, _vp]),
    "sogm_filter_point_cloud_labelled": (_i, [_vp, _vp, _vp, _vp, C.c_float, _i, C.POINTER(SogmLabelSources), _vp, _vp, _vp,
                                              _vp, _vp]),
    "sogm_filter_reserve": (_i, [_vp, _i]),
    "sogm_dsp_create": (_i, [_vp, C.POINTER(SogmDspParams), _vp, _vp, _i, _vp, _i, _i, C.POINTER(_vp)]),
    "sogm_dsp_destroy": (None, [_vp]),
    "sogm_update_dsp": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sogm_dsp_publish": (_i, [_vp, _vp, _vp]),
    "sogm_dsp_download_state": (_i, [_vp, _i, _vp, _vp, _vp]),
    "sogm_dsp_upload_state": (_i, [_vp, _i, _vp, _vp, C.c_double, _vp]),
    "sogm_dsp_download_born": (_i, [_vp, _i, _vp, _i, _vp, _vp]),
    "sogm_dsp_download_born_source": (_i, [_vp, _i, _vp, _i, _vp]),
    "sogm_dsp_velocity_audit": (_i, [_vp, _vp, _vp, _vp, C.POINTER(SogmVelAuditParams), _vp, _vp, _vp]),
    "sogm_dsp_download_observations": (_i, [_vp, _i, _vp, _vp, _vp]),
}


class SogmError(RuntimeError):
    pass


def load_library(path=LIB_PATH):
    """Load libsogm_hip.so and bind every ABI symbol.  Raises if the extension is missing."""
    if not os.path.exists(path):
        raise SogmError(
            f"HIP extension not built: {path} is missing. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # The hosts above this binding keep device buffers in torch tensors.  torch ships its own
    # libamdhip64; load it first so that the extension binds to the SAME HIP runtime (two runtimes in one
    # process do not see each other's devices or allocations).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    got = lib.sogm_abi_version()
    if got != SOGM_ABI_VERSION:  # buffer sizes of existing entry points changed between versions: never mix them
        raise SogmError(f"{path} implements ABI version {got}, this binding was written against {SOGM_ABI_VERSION}: "
                        "rebuild the extension (python -c 'import __graft_entry__ as g; g.build()')")
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = load_library()
    return _lib


def check(rc, what):
    if rc != SOGM_OK:
        msg = lib().sogm_last_error()
        raise SogmError(f"{what} failed: status {rc} ({msg.decode() if msg else ''})")
