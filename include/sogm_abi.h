/*
 * sogm_abi.h — the extern "C" drop-in boundary of the MI355X-native SOGM replan hot path.
 *
 * The reference (siyuanwu99/pred-occ-planner) has no FFI/plugin layer: plan_manager links the
 * map / search / corridor / optimiser class libraries directly (plan_manager/CMakeLists.txt:15-32)
 * and calls them through shared_ptr members (plan_manager/include/plan_manager/baseline.h:155-158).
 * The drop-in boundary is therefore (i) the C++ facade classes in
 * the headers under pred-occ-planner_amd/host/, which keep the reference method names, and (ii) this C ABI,
 * which those facades (and the Python ctypes host) forward to.  Each entry point cites the
 * reference interface it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / Eigen / ROS types;
 *   - every array argument marked "dev" is a DEVICE pointer (HBM resident), "host" a host pointer;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - all calls are asynchronous on `stream` unless documented otherwise;
 *   - return value: 0 = SOGM_OK, negative = sogm_status error; no exceptions cross the boundary;
 *   - one context per thread (thread-compatible, not thread-safe), like the reference objects;
 *   - there is NO CPU fallback: without a HIP device every compute call returns SOGM_ERR_NO_DEVICE.
 */
#ifndef SOGM_ABI_H
#define SOGM_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* status                                                                                      */
/* ------------------------------------------------------------------------------------------ */
typedef enum sogm_status {
  SOGM_OK              = 0,
  SOGM_ERR_INVALID_ARG = -1,
  SOGM_ERR_NO_DEVICE   = -2, /* no HIP device / HIP runtime error at create time             */
  SOGM_ERR_HIP         = -3, /* a HIP call failed; see sogm_last_error()                     */
  SOGM_ERR_CAPACITY    = -4, /* an output buffer / pool was too small                        */
  SOGM_ERR_STATE       = -5, /* call order violated (e.g. query before any update)           */
  SOGM_ERR_COMM        = -6  /* RCCL could not be loaded / a collective failed; see sogm_last_error() */
} sogm_status;

/* ------------------------------------------------------------------------------------------ */
/* plain-data records                                                                          */
/* ------------------------------------------------------------------------------------------ */

/* Which reference map class the context reproduces. */
enum {
  SOGM_MAP_FAKE      = 0, /* FakeParticleRiskVoxel  plan_env/src/fake_particle_risk_voxel.cpp    */
  SOGM_MAP_RISKBASE  = 1, /* RiskBase               plan_env/src/risk_base.cpp                   */
  SOGM_MAP_RISKVOXEL = 2  /* RiskVoxel (DSP particle map)  plan_env/src/risk_voxel.cpp: queries
                             as RiskBase; the neighbour overlay SETS cells to 1.0
                             (addObstaclesToRiskMap :311-318) instead of adding risk.            */
};

/*
 * Grid + map parameters.  The reference fixes L,W,H,T with macros
 * (plan_env/include/plan_env/map_parameters.h:5-13); here they are runtime values.
 * Field defaults (reference):  66,66,20,6, 0.15, time_resolution 0.2 (map.cpp:30),
 * risk_threshold 0.2 (map.cpp:35), clearance 0.3 (map.cpp:36; sim_fake.yaml:71 -> 0.45),
 * ceiling 2.0 / ground -1.0 (map.cpp:37-38; sim_fake.yaml:68-69 -> 3.0 / -0.01),
 * region threshold 1.2, decays 0.2 (risk_base.cpp:21-23).
 */
enum { SOGM_STORE_F32 = 0, SOGM_STORE_F16 = 1,
       /* OR-ed into SogmSpec.storage: the cells of a slice are kept in 2 x 2 x 2 tiles (L, W, H even) instead of x-fastest
        * rows — same values at the ABI (sogm_download_reference_layout, queries, sogm_set_future_risk convert), about half
        * the 32-byte sectors written by the stamp and zeroed by the sparse reset (obstacle surfaces run along z).
        * sogm_grid_ptr() then points at tiled slices: cell
        * (x, y, z) of slice t at  t V + ((((z>>1) (W>>1) + (y>>1)) (L>>1) + (x>>1)) << 3 | (z&1) << 2 | (y&1) << 1 | (x&1)). */
       SOGM_LAYOUT_TILED = 16 };
typedef struct SogmSpec {
  int32_t L, W, H, T;
  float   resolution;
  float   time_resolution;
  float   risk_threshold;
  float   clearance;
  float   ground_height;
  float   ceiling_height;
  float   risk_threshold_region;
  float   risk_thres_reg_decay;
  float   risk_thres_vox_decay;
  int32_t map_kind; /* SOGM_MAP_FAKE | SOGM_MAP_RISKBASE | SOGM_MAP_RISKVOXEL */
  int32_t storage;  /* SOGM_STORE_F32 (reference: float risk_maps_) | SOGM_STORE_F16 (half the HBM
                       bytes per voxel; marks and neighbour counts up to 2048 stay exact) */
} SogmSpec;

/* Ground-truth obstacle record, field-for-field `struct Cylinder`
 * (plan_env/include/plan_env/fake_particle_risk_voxel.h:31-44). type 3 = cylinder, 2 = ring. */
typedef struct SogmCylinder {
  int32_t type;
  int32_t _pad;
  double  x, y, z, w, h, vx, vy, qw, qx, qy, qz;
} SogmCylinder;

/*
 * One shared trajectory = the payload of traj_utils/msg/BezierTraj.msg:1-9 as stored by
 * ParticleATC::trajectoryCallback (traj_coordinator/src/particles.cpp:131-191) in
 * SwarmParticleTraj (traj_coordinator/include/traj_coordinator/particle.hpp:30-37).
 * Fixed size so that one RCCL all-gather moves the whole swarm's records.
 * n_pieces == 0 means "no trajectory received from this drone".
 * cpts: piece-major, 5 control points per piece, xyz-minor (row k = piece*5 + j).
 */
#define SOGM_MAX_PIECES 16
typedef struct SogmTrajRecord {
  int32_t drone_id;
  int32_t n_pieces;
  double  time_start; /* absolute seconds (traj_msg->start_time) */
  double  duration[SOGM_MAX_PIECES];
  double  cpts[SOGM_MAX_PIECES * 5 * 3];
} SogmTrajRecord;

/* Search parameters = FakeRiskHybridAstar::setParam (path_searching/src/fake_risk_hybrid_a_star.cpp:62-82),
 * values from plan_manager/config/sim_fake.yaml:15-29. */
typedef struct SogmAstarParams {
  double  max_tau;
  double  max_vel;
  double  max_acc;
  double  w_time;
  double  horizon;
  double  lambda_heu;
  double  resolution;      /* search/resolution_astar */
  double  time_resolution; /* search/time_resolution  */
  int32_t allocate_num;
  int32_t check_num;
  int32_t tolerance; /* search/tolerance, default 1 */
  int32_t shot_ignores_time; /* 0 = FakeRiskHybridAstar: the shot trajectory is checked with
                                getClearOcccupancy(coord, time) (fake_risk_hybrid_a_star.cpp:521);
                                1 = RiskHybridAstar: getClearOcccupancy(coord), i.e. slice 0
                                (risk_hybrid_a_star.cpp:514, risk_base.cpp:251-253) — the only difference
                                between the two classes.  sogm_planner_create() sets it from
                                SogmPlannerParams.fake_planner (BaselinePlanner owns a RiskHybridAstar,
                                FakeBaselinePlanner a FakeRiskHybridAstar: baseline.h:155, baseline_fake.h). */
} SogmAstarParams;

/* Planner parameters = BaselineParameters (plan_manager/include/plan_manager/baseline.h:45-94). */
typedef struct SogmPlannerParams {
  double  corridor_tau;
  double  init_range;
  double  shrink_size;
  double  opt_max_vel; /* finite and positive: the QP's velocity / acceleration rows are two-sided boxes; values */
  double  opt_max_acc; /* >= 1e20 ("unbounded") are rejected by sogm_planner_create (SOGM_ERR_INVALID_ARG)      */
  int32_t fake_planner; /* 1 = FakeBaselinePlanner rules (baseline_fake.cpp), 0 = BaselinePlanner */
  int32_t firi_iterations; /* 2 at baseline.cpp:352 */
  int32_t pc_capacity;     /* max obstacle points per corridor box */
  int32_t max_faces;       /* max faces kept per polytope */
} SogmPlannerParams;

/* QP solver settings = OSQP v0.6 defaults as used through IOSQP (traj_opt/include/iosqp.hpp:40-115,
 * traj_opt/src/bezier_optimizer.cpp:269).  adaptive_rho_interval: 0 = fixed rho (one KKT factor
 * for the whole solve); k > 0 = OSQP's adaptive rho evaluated every k iterations (OSQP's
 * wall-clock-derived interval lands on its check_termination multiple, 25, for problems this size).
 * residual_fp32 (BASELINE configs[4], "mixed-precision ADMM residuals"; 0 = off, the default): the termination
 * checks evaluate the residual norms, their normalisations and the workgroup reductions in fp32 (the iteration
 * itself, the rho estimate's inputs and the infeasibility certificate's A'dy stay fp64).  A check near its threshold
 * may then pass one check earlier or later than OSQP's fp64 test: the contract of this mode is "same status,
 * coefficients within 1e-4 of the fp64 solve", not "same iteration count". */
typedef struct SogmQpSettings {
  double  rho;
  double  sigma;
  double  alpha;
  double  eps_abs;
  double  eps_rel;
  int32_t max_iter;
  int32_t check_termination;
  int32_t scaling_iters;
  int32_t adaptive_rho_interval;
  int32_t residual_fp32;
  int32_t reserved_;
} SogmQpSettings;

typedef struct sogm_ctx sogm_ctx;

/* This header is what a plan_manager host binds: contexts, the map updates, the overlay, the queries, search, corridors,
 * QP, replan, the flight, the trajectory exchange, version and errors.  Everything a host does NOT need to fly — tuning
 * knobs, per-kernel profiling, device clocks, traffic counters, parity downloads of internal state, test hooks — is
 * declared in include/sogm_abi_debug.h (same library, same version number). */
/* ------------------------------------------------------------------------------------------ */
/* library                                                                                     */
/* ------------------------------------------------------------------------------------------ */
/* ABI version of this header; bumps on any change of a signature OR of the size of a buffer an entry point writes
 * (version 5: sogm_sparse_reset_state writes out[8] and sogm_profile_read SOGM_PROF_N = 8 doubles, where version 4's
 * first revision wrote 7; SogmWorld / the world-frame update entries / the flight entries were added; version 6: SogmFlight
 * gained nccl_comm, sogm_flight_stats reports hdr[15], the profiling / tuning / debug entries moved to sogm_abi_debug.h).  A host
 * compares sogm_abi_version() with the SOGM_ABI_VERSION it was compiled against before any other call: the Python
 * binding and host/sogm_facade.hpp refuse a library of another version. */
#define SOGM_ABI_VERSION 6
int         sogm_abi_version(void);
/* Text of the last HIP error seen by this thread ("" if none). */
const char *sogm_last_error(void);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int         sogm_device_count(void);

/* ------------------------------------------------------------------------------------------ */
/* map context:  MapBase::init / RiskBase::init / FakeParticleRiskVoxel::init                   */
/*   (plan_env/src/map.cpp:42-105, risk_base.cpp:15-58, fake_particle_risk_voxel.cpp:20-73)    */
/* ------------------------------------------------------------------------------------------ */
/* Allocates the batched SOGM  sogm[n_agents][T][H][W][L]  (fp32 or fp16 per spec->storage, time-major
 * slabs) on `device`. */
int  sogm_create(const SogmSpec *spec, int n_agents, int device, sogm_ctx **out);
void sogm_destroy(sogm_ctx *ctx);
/* Bytes of HBM held by the grid. */
int64_t sogm_grid_bytes(const sogm_ctx *ctx);
/* Device pointer of the grid (layout above; __half elements when storage is SOGM_STORE_F16).  The caller may write
 * through it: the grid's next reset is then the dense clear (see sogm_set_sparse_reset). */
float  *sogm_grid_ptr(sogm_ctx *ctx);

/* Sparse reset of the map.  The reference rebuilds the SOGM from zero at every update
 * (fake_particle_risk_voxel.cpp:107-108, a fill over all V x T cells, then the marks).  The library produces the
 * same cells without touching the ones that are zero already: every mark written by sogm_update_gt[_swarm] /
 * sogm_project_neighbours is logged as the index of its 32-byte sector (one log per agent and per grid of the pool,
 * log_capacity entries per agent: 0 keeps the current value; default V*T/80, at least 2^20, or SOGM_LOG_CAP), and the grid's next reset
 * zeroes exactly the logged sectors.  A grid written by a dense writer (sogm_set_future_risk, sogm_dsp_publish, the
 * caller through sogm_grid_ptr), a freshly allocated one, and an agent whose log overflowed are cleared densely.
 * enable = 0 restores the dense clear everywhere (also: SOGM_SPARSE_RESET=0 in the environment at sogm_create).
 * Synchronises the device; call between ticks. */
int sogm_set_sparse_reset(sogm_ctx *ctx, int enable, int log_capacity);
/* Resample branch of ParticleATC::getParticlesWithRisk (particles.cpp:365-409; swarm/replan_risk_rate and
 * swarm/num_resample, particles.cpp:33-34 — 0.00 in every shipped configuration, which is also the default here).  With
 * a rate > 0 a neighbour's body particle at slice time t is replaced, once replan_risk_rate * (t - time_start) >= 1e-3,
 * by num_resample Gaussian samples weighted exp(-|n|^2 / 2 sigma^2), the weights normalised to num_resample per
 * particle, and the map receives the weights instead of 1.0.  The reference draws the noise from
 * std::default_random_engine(time(NULL)), re-seeded at every call: every call of one wall-clock second replays one
 * sequence.  The host injects that sequence as a table of standard normals (device, float, kept alive by the caller,
 * >= 3 * body particles * num_resample entries): sample i of particle e uses entries 3 (e n + i) + {0, 1, 2} times
 * sigma.  Applies to sogm_project_neighbours / sogm_update_gt_swarm / sogm_update_prestamped on FAKE and RISKBASE maps
 * with fp32 cells (RiskVoxel's overlay does not resample, risk_voxel.cpp:258-339).  Call after
 * sogm_set_body_particles.  rate 0 or num_resample 0 switches it off. */
int sogm_set_resample(sogm_ctx *ctx, float replan_risk_rate, int num_resample, const float *normal_table_dev,
                      int n_table);

/* Body particles of one drone: ParticleATC::initEgoParticles (particles.cpp:62-87).
 * host: xyz[n*3] offsets (fp64).  Every drone of the swarm uses the same set.
 * The overlay places ANOTHER drone's particles, and those reach a ParticleATC through particlesCallback
 * (particles.cpp:89-108) as geometry_msgs/Polygon points — Point32, i.e. float32 coordinates cast back to double.  A host
 * that wants the reference's cells to the last bit passes the offsets as received ((double)(float)x; the Python mirror's
 * scene.received_body_particles does); the library uses what it is given. */
int sogm_set_body_particles(sogm_ctx *ctx, const double *xyz_host, int n);


/*
 * Tick pipelining (mode): 0 = off (every update clears its grid in stream order).
 * 1 = in-place pre-clear in two parts on an internal side stream: a narrow launch clears the head of the grid
 *     as soon as sogm_replan()'s obstacle-point kernels have read the SOGM (it shares the machine with the FIRI
 *     kernels), and a full-width launch clears the rest once the corridor stage is done with global memory (only
 *     the LDS-resident QP runs beside it).  While that pre-clear is pending the map counts as "not
 *     updated": queries return SOGM_ERR_STATE until the next update.
 * 2 = double-buffered: a second grid is allocated (SOGM_ERR_CAPACITY if HBM has no room; the mode is then
 *     unchanged) and sogm_replan() clears it under the WHOLE replan; the next update swaps it in.  The current
 *     map stays valid for queries.  sogm_grid_ptr() changes at every update in this mode.
 * The next sogm_update_gt() / sogm_set_future_risk() / sogm_dsp_publish() waits for the pending clear instead
 * of issuing its own.  Changing the mode while a pre-clear is in flight synchronises the device and drops it.
 */
int sogm_set_overlap_clear(sogm_ctx *ctx, int mode);


/* ------------------------------------------------------------------------------------------ */
/* SOGM update                                                                                 */
/* ------------------------------------------------------------------------------------------ */
/*
 * FakeParticleRiskVoxel::updateMap (fake_particle_risk_voxel.cpp:80-222) without the neighbour
 * overlay, for every agent of the batch:
 *   crop cloud to pose +- range (:88-104), zero the grid (:107-108), mark slice 0 (:111-116),
 *   for each occupied voxel look up the GT velocity (:127-154) and stamp slices 1..T-1 (:155-160).
 * dev  cloud_xyz     [n_points*3] fp32, world frame
 * dev  cloud_range   [n_agents*2] int32 {begin,end} point indices seen by each agent
 * dev  cylinders     [n_cyl]      SogmCylinder          (shared GT state, may be NULL if n_cyl==0)
 * dev  poses         [n_agents*3] fp32  map centre (MapBase::pose_)
 * dev  stamps        [n_agents]   fp64  last_update_time_ (absolute seconds)
 */
int sogm_update_gt(sogm_ctx *ctx, const float *cloud_xyz, const int32_t *cloud_range,
                   const SogmCylinder *cylinders, int n_cyl, const float *poses,
                   const double *stamps, void *stream);

/*
 * One sensor frame of the fake-perception map — what MapBase::cloudCallback (plan_env/src/map.cpp:170-171) and
 * FakeParticleRiskVoxel::groundTruthStateCallback (fake_particle_risk_voxel.cpp:244-264) delivered for ONE update —
 * with the spatial index the device-side crop needs: the cloud in blocks of `block_points` consecutive points and the
 * xy bounds of every block (sogm_cloud_block_bounds computes them; a sensor driver that emits obstacles one after the
 * other gets tight blocks for free).  updateMap's PassThrough crop (fake_particle_risk_voxel.cpp:88-104) then runs on the
 * device, per agent, around the agent's CURRENT map centre: one wave lists the blocks that intersect the window, the
 * stamp walks the list.  All pointers are device pointers; the struct itself is read on the host at call time.
 */
typedef struct SogmWorld {
  const float        *cloud_xyz;    /* dev [n_points*3] fp32, world frame                                         */
  const float        *block_bounds; /* dev [n_blocks*4] {xmin, xmax, ymin, ymax} of points [b*block_points, ...)  */
  const SogmCylinder *cylinders;    /* dev [n_cyl] GT obstacle states of the same instant (NULL if n_cyl == 0)     */
  int32_t             n_points;
  int32_t             n_blocks;     /* ceil(n_points / block_points)                                              */
  int32_t             block_points; /* 64 .. 4096                                                                 */
  int32_t             n_cyl;
} SogmWorld;
/* xy bounds of every block of `block_points` consecutive points of a cloud; dev out_bounds[ceil(n/block_points)*4]. */
int sogm_cloud_block_bounds(const float *cloud_xyz, int n_points, int block_points, float *out_bounds, void *stream);
/*
 * FakeParticleRiskVoxel::updateMap for every agent of the batch from one SogmWorld frame: as sogm_update_gt_swarm, with
 * the crop done on the device around `poses` (no per-agent ranges from the host).  records may be NULL (n_records 0):
 * no overlay.  The maps are identical to sogm_update_gt[_swarm] fed with any superset of each agent's window.
 */
int sogm_update_world(sogm_ctx *ctx, const SogmWorld *world, const float *poses, const double *stamps,
                      const SogmTrajRecord *records, int n_records, const int32_t *ego_ids, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* world timeline: the SogmWorld frames of any range of ticks, written on the device           */
/*   The reference's counterpart is the map_generator dynamic_forest_seq node of its            */
/*   uav_simulator submodule (simulator_fake.launch:41), an empty directory in its tree: like    */
/*   the depth camera this is the build's OWN simulator piece.        */
/*   What is held is the definition below, by two independent implementations                    */
/*   (csrc/sogm_world.hpp + csrc/sogm_world.hip and the numpy restatement                        */
/*   tests/world_frames_reference.py), bit for bit.                                              */
/* ------------------------------------------------------------------------------------------ */
/*
 * The world at tick 0 and how it moves: every obstacle record keeps its constant planar velocity (vx, vy), every
 * cloud point moves with the record that owns it.  Frame i of a call is tick k = first_tick + i and is written
 * through the pointers of frames[i], buffers the caller allocated: cloud_xyz [n_points*3], block_bounds [n_blocks*4],
 * cylinders [n_cyl].
 *
 * The arithmetic, in exactly this order, without contraction (the library is built with -ffp-contract=off):
 *
 *   t = (double)k * dt
 *   k == 0 or moving == 0:  the cloud and the records of tick 0 are copied bit for bit (a -0.0f stays -0.0f)
 *   otherwise, record c:    x = x0 + vx*t;  y = y0 + vy*t   (fp64);  every other field is copied
 *   otherwise, point p with c = owner[p] in [0, n_cyl):
 *                           offx = (float)(vx_c * t)        the product in fp64, then rounded ONCE
 *                           X    = x_p + offx               an fp32 add, performed even when offx is zero
 *                                                           (-0.0f + 0.0f = +0.0f, as numpy gives)
 *                           y likewise; z is copied
 *   a point whose owner is outside [0, n_cyl) is copied; no read ever depends on an out-of-range owner
 *
 *   block_bounds of the written cloud = what sogm_cloud_block_bounds(cloud_xyz, n_points, block_points, ...) gives,
 *   bit for bit, the tail block included (min and max are exact: the order of the reduction is free).
 *   Non-finite points are the caller's problem: they are treated as that entry treats them.
 */
typedef struct SogmWorldTimeline {
  const float        *cloud0;      /* dev [n_points*3] fp32, the cloud at tick 0                                  */
  const int32_t      *owner;       /* dev [n_points]: the record a point moves with; outside [0, n_cyl): static   */
  const SogmCylinder *cylinders0;  /* dev [n_cyl] states at tick 0 (NULL if n_cyl == 0)                           */
  int32_t n_points, n_cyl, block_points /* 64..4096 */, moving /* 0: every frame is tick 0 */;
  double  dt;                      /* seconds per tick */
} SogmWorldTimeline;
/*
 * Writes the frames of ticks first_tick .. first_tick + n_ticks - 1.  Context-free like sogm_render_depth: the current
 * device, stream-ordered, no allocation, no host synchronisation; the structs are read on the host at call time.
 * SOGM_ERR_INVALID_ARG (checked first, as in sogm_render_depth; sogm_last_error() names the rule): a null tl or frames;
 * a null cloud0 or owner with n_points > 0; a null cylinders0 with n_cyl > 0; n_points < 0 or n_cyl < 0; block_points
 * outside 64..4096; dt not finite or not positive; first_tick < 0, n_ticks < 1 or first_tick + n_ticks overflowing int;
 * a frame whose n_points, n_blocks, block_points or n_cyl differs from the timeline's (n_blocks = ceil(n_points /
 * block_points)); a frame with a null buffer it needs (cloud_xyz and block_bounds with n_points > 0, cylinders with
 * n_cyl > 0); a frame buffer equal to one of the timeline's inputs or to another frame's buffer of the same call.
 * SOGM_ERR_NO_DEVICE without a GPU.
 */
int sogm_world_frames(const SogmWorldTimeline *tl, int first_tick, int n_ticks,
                      const SogmWorld *frames /* host [n_ticks]; their device buffers are WRITTEN */, void *stream);

/*
 * Neighbour overlay: RiskBase::addOtherAgents (risk_base.cpp:136-168) ==
 * fake_particle_risk_voxel.cpp:178-218, through ParticleATC::getParticlesWithRisk
 * (particles.cpp:346-422, replan_risk_rate == 0 branch) and addParticlesToRiskMap
 * (risk_base.cpp:199-208).  Uses the poses/stamps of the last update.
 * dev  records  [n_records] SogmTrajRecord  (the swarm's latest trajectories)
 * dev  ego_ids  [n_agents]  int32           drone_id of each batch agent (skipped as "ego")
 */
int sogm_project_neighbours(sogm_ctx *ctx, const SogmTrajRecord *records, int n_records,
                            const int32_t *ego_ids, void *stream);

/*
 * FakeParticleRiskVoxel::updateMap as ONE call: sogm_update_gt followed by the neighbour overlay the reference runs
 * at the end of the same function (plan_env/src/fake_particle_risk_voxel.cpp:175-226; RiskBase / RiskVoxel:
 * risk_base.cpp:71, risk_voxel.cpp:179).  Arguments as sogm_update_gt + sogm_project_neighbours; the resulting maps
 * are identical to the two separate calls.  Needs sogm_set_body_particles().
 */
int sogm_update_gt_swarm(sogm_ctx *ctx, const float *cloud_xyz, const int32_t *cloud_range,
                         const SogmCylinder *cylinders, int n_cyl, const float *poses, const double *stamps,
                         const SogmTrajRecord *records, int n_records, const int32_t *ego_ids, void *stream);

/*
 * RiskBase::futureRiskCallback (risk_base.cpp:60-80): adopt an externally produced SOGM.
 * dev  grid_vt  [n_agents][V][T] fp32 in the REFERENCE layout (voxel-major); transposed into slabs.
 */
int sogm_set_future_risk(sogm_ctx *ctx, const float *grid_vt, const float *poses,
                         const double *stamps, void *stream);


/*
 * RiskBase::getMapTime().toSec() and getMapCenter() of one agent (plan_env/include/plan_env/risk_base.h:70,76;
 * map.h:109-111): the stamp and pose the last update / sogm_set_future_risk adopted.  Host outputs (either may be
 * NULL); waits for `stream`.  SOGM_ERR_STATE before the first update.
 */
int sogm_map_state(sogm_ctx *ctx, int agent, double *out_map_time_host, float *out_center_host /* [3] */,
                   void *stream);

/*
 * Bezier::getPos / getVel / getAcc (traj_utils/include/traj_utils/bernstein.hpp:174-187,
 * traj_utils/src/bernstein.cpp:25-59) for a batch of shared trajectories:
 * out_pva[i] = {pos, vel, acc} of records[i] at absolute time t[i] (clamped to the trajectory's
 * span, as FiniteStateMachine does when it samples the replan start state,
 * plan_manager/src/plan_manager.cpp:169-175).  out_valid[i] = 0 when the record holds no trajectory.
 * dev records[n], dev t[n] fp64, dev out_pva[n*9] fp64, dev out_valid[n] int32.
 */
int sogm_traj_eval(const SogmTrajRecord *records, int n, const double *t, double *out_pva,
                   int32_t *out_valid, void *stream);


/*
 * MapBase::filterPointCloud (plan_env/src/map.cpp:107-132; duplicate risk_mapping_node.cpp:74-99) for
 * every agent: pcl::VoxelGrid centroid filter with leaf `filter_res` (one fp32 centroid per occupied
 * leaf, emitted in ascending leaf index — PCL >= 1.8 applyFilter, third-party), camera->body axis
 * swap (x = z, y = -x, z = -y), isInRange against the map's local range, stop at `cap` points
 * (5000 in the reference).  The output feeds sogm_update_dsp as `points`.
 * dev raw_xyz   [n_total*3] fp32 camera-frame points (non-finite points are skipped)
 * dev raw_range [n_agents*2] int32 {begin,end}
 * dev out_xyz   [n_agents*cap*3] fp32,  dev out_count [n_agents] int32 (-1: the cloud's bounding box
 *               has more leaves than the accumulator array, see sogm_filter_reserve)
 */
int sogm_filter_point_cloud(sogm_ctx *ctx, const float *raw_xyz, const int32_t *raw_range,
                            float filter_res, int cap, float *out_xyz, int32_t *out_count,
                            void *stream);
/* Leaf accumulators per agent (default 2^20 = a 15 m cube at 0.15 m); call before the first filter call. */
int sogm_filter_reserve(sogm_ctx *ctx, int max_cells_per_agent);

/* ------------------------------------------------------------------------------------------ */
/* particle-filter SOGM:  dsp_map::DSPMap  (plan_env/include/plan_env/dsp_dynamic.h)            */
/*   as owned and configured by RiskVoxel (plan_env/src/risk_voxel.cpp:42-50,237-254)          */
/* ------------------------------------------------------------------------------------------ */
/* Compile-time constants of the reference (plan_env/include/plan_env/map_parameters.h:5-54) and
 * the DSPMap settings RiskVoxel::init applies, as runtime values.  The grid (L,W,H,T,resolution)
 * comes from the SogmSpec of the map context; T = PREDICTION_TIMES. */
#define SOGM_DSP_MAX_T 16
typedef struct SogmDspParams {
  int32_t max_particle_num_voxel; /* MAX_PARTICLE_NUM_VOXEL 7; slots per voxel = 2x (:51)        */
  int32_t half_fov_h;             /* 43 deg (:22)                                                */
  int32_t half_fov_v;             /* 29 deg (:24)                                                */
  int32_t angle_resolution;       /* ANGLE_RESOLUTION 1 (:9)                                     */
  int32_t newborn_num;            /* setNewBornParticleNumberofEachPoint(20) risk_voxel.cpp:47   */
  int32_t obs_max_per_pyramid;    /* observation_max_points_num_one_pyramid 100 (:51)            */
  float   prediction_times[SOGM_DSP_MAX_T]; /* prediction_future_time {0.3 .. 1.8} (:19)         */
  float   sigma_observation;      /* map/sigma_observation 0.05 (risk_voxel.cpp:20,45)           */
  float   p_detection;            /* 0.95 (dsp_dynamic.h:135)                                    */
  float   kappa;                  /* 0.01 (:134)                                                 */
  float   newborn_weight;         /* setNewBornParticleWeight(0.0001) risk_voxel.cpp:49          */
  float   obstacle_thickness;     /* obstacle_thickness_for_occlusion 0.3 (map_parameters.h:54)  */
} SogmDspParams;

typedef struct sogm_dsp sogm_dsp;

/*
 * DSPMap::DSPMap + setInitParameters (dsp_dynamic.h:118-163,566-632) for every agent of `map`.
 * The reference fills three 1e7-entry Gaussian tables from a time(0)-seeded engine (:1229-1239)
 * and draws uniforms from rand(); here the tables are inputs so that runs are reproducible:
 * host p_gauss[n_gauss] (position noise, N(0, 0.05)), v_gauss[n_gauss] (velocity noise),
 * rand_tab[n_rand] (values of rand(), 0..RAND_MAX).  The tables are read cyclically.
 * max_points: capacity of one agent's cloud (5000 in MapBase::filterPointCloud, map.cpp:126).
 * Particle store per agent: V x 16 slots x 25 B (SoA) — SOGM_ERR_HIP if it does not fit in HBM.  max_points <= 8192.
 */
int  sogm_dsp_create(sogm_ctx *map, const SogmDspParams *params, const float *p_gauss,
                     const float *v_gauss, int n_gauss, const int32_t *rand_tab, int n_rand,
                     int max_points, sogm_dsp **out);
void sogm_dsp_destroy(sogm_dsp *d);

/*
 * DSPMap::update (dsp_dynamic.h:165-364) for every agent: observation binning into FOV pyramids,
 * mapPrediction (:663), mapUpdate (:750), mapAddNewBornParticlesByObservation (:852),
 * mapOccupancyCalculationAndResample (:993).  Stream-ordered, no host round trip.
 * dev points  [n_total*3] fp32  sensor-frame points, already voxel-filtered (MapBase::filterPointCloud)
 * dev labels  [n_total*4] fp32  {vx, vy, vz, intensity} per point = an externally supplied output of
 *             velocityEstimationThread (new-born particles are then created in the order the points are given),
 *             or NULL: velocityEstimationThread (:1487-1678) runs on the GPU — ground split, Euclidean
 *             clustering (tolerance 2 x 0.15 m, 5..10000 points; PCL's seed / size order), centres, gated
 *             optimal assignment to the previous frame's clusters (Munkres' role), velocity = centre
 *             displacement / dt, and the new-born list in the reference's order [possibly-dynamic clusters]
 *             [ground points][static clusters].  Needs a voxel-filtered cloud (<= 128 neighbours within the
 *             tolerance, <= 256 clusters, <= 64 possibly-dynamic ones; beyond: an error counter, never a hang)
 * dev cloud_range [n_agents*2] int32 {begin,end} points of each agent
 * dev sensor_pos [n_agents*3] fp32, dev sensor_quat [n_agents*4] fp32 (w,x,y,z), dev stamps [n_agents] fp64
 * dev out_ok  [n_agents] int32: DSPMap::update's return value (0 = rejected odometry, :186-203)
 */
int sogm_update_dsp(sogm_dsp *d, const float *points, const float *labels,
                    const int32_t *cloud_range, const float *sensor_pos, const float *sensor_quat,
                    const double *stamps, int32_t *out_ok, void *stream);

/*
 * The map half of RiskVoxel::publishMap (risk_voxel.cpp:138-153): getOccupancyMapWithFutureStatus
 * (dsp_dynamic.h:445-469) into the SOGM grid of the map context (which also adopts the sensor
 * position / stamp of the last update as map pose / map time), clearing the future accumulators,
 * then the zeroing loop over the inflate kernel.  dev out_n_occupied [n_agents] int32 or NULL.
 * Follow with sogm_project_neighbours() for the overlay (risk_voxel.cpp:161-163).
 */
int sogm_dsp_publish(sogm_dsp *d, int32_t *out_n_occupied, void *stream);


/* ------------------------------------------------------------------------------------------ */
/* depth-image front end:  GridMap  (plan_env/src/grid_map.cpp, plan_env/src/raycast.cpp)      */
/*   SURVEY section 8 row f1 — not on the reference's SOGM path today; occupancy grid of its own */
/* ------------------------------------------------------------------------------------------ */
/* grid_map/ parameters (GridMap::initMap, grid_map.cpp:15-63).  The reference ships no YAML for them
 * (defaults are -1): every value is the caller's. */
typedef struct SogmGridMapParams {
  double  resolution;
  double  map_size[3];
  double  local_update_range[3];
  double  obstacles_inflation;
  double  fx, fy, cx, cy;
  double  depth_filter_maxdist, depth_filter_mindist;
  double  k_depth_scaling_factor;
  double  p_hit, p_miss, p_min, p_max, p_occ; /* 0.70 0.35 0.12 0.97 0.80 (:43-47) */
  double  max_ray_length;
  double  virtual_ceil_height, ground_height;
  int32_t use_depth_filter;    /* default true (:35) */
  int32_t depth_filter_margin;
  int32_t skip_pixel;
  int32_t local_map_margin;    /* 1 (:60) */
  int32_t rows, cols;          /* depth image size (480 x 640) */
} SogmGridMapParams;

typedef struct sogm_gridmap sogm_gridmap;

/* GridMap::initMap for n_agents independent maps (log-odds buffer fp64 like the reference). */
int  sogm_gridmap_create(const SogmGridMapParams *params, int n_agents, int device, sogm_gridmap **out);
void sogm_gridmap_destroy(sogm_gridmap *g);
/*
 * depthPoseCallback + updateOccupancyCallback (grid_map.cpp:585-665) for every agent:
 * projectDepthImage (:210-311), raycastProcess (:313-445: 3-D DDA per pixel from the ray end towards the
 * camera with the per-frame ray-end / traversed-voxel de-duplication, hit/miss log-odds fusion),
 * clearAndInflateLocalMap (:469-583).  The de-duplication makes the reference order dependent (a ray
 * stops at the first voxel an EARLIER ray traversed); it is reproduced exactly by iterating
 * "first ray to arrive" to its fixed point.
 * dev depth   [n_agents*rows*cols] uint16 (depth * k_depth_scaling_factor)
 * dev cam_pos [n_agents*3] fp64, dev cam_rot [n_agents*9] fp64 row-major camera-to-world rotation
 * dev out_updated [n_agents] int32 or NULL: 0 when the camera is outside the map (:656-662)
 */
int sogm_gridmap_update(sogm_gridmap *g, const uint16_t *depth, const double *cam_pos,
                        const double *cam_rot, int32_t *out_updated, void *stream);
/* GridMap::getInflateOccupancy (grid_map.h:342-349): dev agent_idx[n], pos[n*3] fp64 -> out[n] int8 {-1,0,1} */
int sogm_gridmap_query_inflate(sogm_gridmap *g, const int32_t *agent_idx, const double *pos, int n,
                               int8_t *out, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* ring obstacles: the second obstacle kind of the ground-truth record (type 2), as the depth     */
/*   camera and the flight audit below take it.  The reference only attributes ring velocities   */
/*   in its map (fake_particle_risk_voxel.cpp:139-150); what a ring IS to a camera or to a body  */
/*   is the build's OWN definition, held by two independent implementations each                 */
/*   (csrc/sogm_ring.hpp; tests/depth_ring_reference.py and tests/audit_ring_reference.py).      */
/* ------------------------------------------------------------------------------------------ */
/*
 * All arithmetic is fp64, in exactly the order written, one IEEE operation at a time (+ - * / sqrt), without contraction:
 * the host and the device give the same bits.  dot(a, b) = (a0*b0 + a1*b1) + a2*b2.
 *
 * Geometry: a SogmCylinder record of type 2 is a solid torus.
 *   centre  c = (x, y, z).  z and the orientation never change; x, y are the record's (depth camera: "of the same
 *           instant") or advance with vx, vy (flight audit).
 *   R   = 0.5*w   major radius (the reference's cyl.w / 2, fake_particle_risk_voxel.cpp:147)
 *   rho = h       tube radius.  This choice is the build's own: scene.add_rings writes h = 0.1, the half width of the
 *                 3 x 3 tube section it puts into the cloud.
 *   frame   qn = sqrt(((qw*qw + qx*qx) + qy*qy) + qz*qz);  w = qw/qn; x = qx/qn; y = qy/qn; z = qz/qn  (these four
 *           letters: the unit quaternion, only in the next three lines)
 *             e1 = ( 1 - 2*(y*y + z*z),  2*(x*y + w*z),      2*(x*z - w*y)     )
 *             e2 = ( 2*(x*y - w*z),      1 - 2*(x*x + z*z),  2*(y*z + w*x)     )
 *             n  = ( 2*(x*z + w*y),      2*(y*z - w*x),      1 - 2*(x*x + y*y) )
 *           the columns of scene._quat_to_matrix; the circle is c + R (cos e1 + sin e2), the reference's plane through
 *           c, c + q(0,1,0), c + q(1,0,0) (:141-143).
 *   not a ring: any of x, y, z, w, h, vx, vy, qw, qx, qy, qz not finite, or not R > 0, or not rho > 0, or not rho < R, or
 *           qn not finite or not > 0.  The camera counts such a record as unsupported and does not draw it; the audit
 *           treats it as it treats an unsupported type.
 *
 * Ray against ring (depth camera; t is the camera's z-depth parameter, the ray is p + t d):
 *   o = p - c;  alpha = dot(d, d);  beta = dot(o, d);  gamma = dot(o, o);  no = dot(n, o);  nd = dot(n, d)
 *   alpha > 0, else no hit.
 *   bounding sphere:  S = R + rho;  cs = gamma - S*S;  disc = beta*beta - alpha*cs;  disc < 0: no hit.
 *                     s = sqrt(disc);  t0 = (-beta - s)/alpha;  t1 = (-beta + s)/alpha
 *   slab |no + t nd| <= rho:  nd == 0: no hit unless |no| <= rho.  Otherwise ta = (-rho - no)/nd;  tb = (rho - no)/nd;
 *                     t0 = max(t0, min(ta, tb));  t1 = min(t1, max(ta, tb))
 *   t0 = max(t0, 0);  no hit unless t0 <= t1.
 *   inside the torus means f(t) < 0,  f(t) = (((c4*t + c3)*t + c2)*t + c1)*t + c0  with
 *     RR = R*R;  K = (gamma + RR) - rho*rho
 *     c4 = alpha*alpha
 *     c3 = (4*alpha)*beta
 *     c2 = ((4*beta)*beta + (2*alpha)*K) - (4*RR)*(alpha - nd*nd)
 *     c1 = (4*beta)*K - (8*RR)*(beta - no*nd)
 *     c0 = K*K - (4*RR)*(gamma - no*no)
 *   f(t0) <= 0 and t0 == 0: the camera is inside the tube and this ring gives the pixel NO return (for a cylinder the
 *     camera sees the inner wall; here it does not).
 *   f(t0) <= 0 and t0 > 0: the hit is t0.
 *   otherwise search: hs = (t1 - t0)/32; node_i = t0 + i*hs for i = 1 .. 31, node_32 = t1.  The first node with
 *     f(node_i) <= 0 brackets the entry: lo = node_(i-1) (node_0 = t0), hi = node_i.  48 times: m = 0.5*(lo + hi);
 *     f(m) <= 0 moves hi to m, otherwise lo to m.  The hit is hi.  No such node: no hit.
 *   The sphere, the slab and the empty interval are part of the rule, not an approximation of it.  A thin near-side
 *   crossing that lies wholly between two nodes is not found: the far side (or nothing) is returned.
 *
 * Body box against ring (flight audit):
 *   table of 64 unit vectors by arc halving: u_0 = (1,0), u_16 = (0,1), u_32 = (-1,0), u_48 = (0,-1); then for
 *     step = 8, 4, 2, 1 every u_i with i an odd multiple of step is mid(u_(i-step), u_(i+step)) (indices mod 64), where
 *     mid(a, b):  sx = a0 + b0;  sy = a1 + b1;  nn = sqrt(sx*sx + sy*sy);  (sx/nn, sy/nn).
 *   box: lo_i = a_i - 0.5*body_i;  hi_i = a_i + 0.5*body_i  (a: the agent's position)
 *   g(u):  P_i = c_i + R*(u0*e1_i + u1*e2_i);  q_i = lo_i if P_i < lo_i, hi_i if P_i > hi_i, else P_i;  dd_i = P_i - q_i;
 *          g = sqrt((dd_0*dd_0 + dd_1*dd_1) + dd_2*dd_2)
 *   the vertex with the smallest g (lowest index on ties) is m, its table neighbours l and r.  Twelve times:
 *     ml = mid(l, m);  mr = mid(m, r);  if g(ml) < g(m) and g(ml) <= g(mr): (l, m, r) = (l, ml, m);
 *     else if g(mr) < g(m): (l, m, r) = (m, mr, r);  else (l, m, r) = (ml, m, mr).
 *   gap = g(m) - rho;  a collision is gap < 0.  Unlike the cylinder's, this gap is three-dimensional: there is no
 *   z-overlap gate, it takes part in min_gap at every sample.
 */
enum { SOGM_DEPTH_RINGS = 1 };   /* SogmDepthCamera.flags */
enum { SOGM_AUDIT_RINGS = 1 };   /* SogmAuditParams.flags */

/* ------------------------------------------------------------------------------------------ */
/* depth camera: the frames the two front ends above see of a SogmWorld                          */
/*   The reference took them from its uav_simulator submodule, an empty directory in its tree:   */
/*   this camera is the build's OWN (SURVEY section 8 d), as the intrinsics of the GridMap       */
/*   parameters are.  There is nothing to be in parity with; what is held is the definition      */
/*   below, by two independent implementations (csrc/sogm_depth.hip and the numpy restatement    */
/*   tests/depth_render_reference.py), bit for bit.                                              */
/* ------------------------------------------------------------------------------------------ */
/*
 * Camera: pin-hole, x right, y down, z forward.  cam_rot is the row-major camera-to-world rotation R
 * (scene.camera_pose; the same array sogm_gridmap_update takes), cam_pos the camera centre p.
 * Obstacles: the SogmCylinder records of a SogmWorld, "of the same instant" — vx, vy are not used.  Geometry as the
 * flight audit's: type 3 is a vertical cylinder of diameter w with its axis at (x, y), z extent [z - h/2, z + h/2],
 * closed by two discs.  Optionally a ground plane z = ground_z.  With SOGM_DEPTH_RINGS set in flags, a type-2 record
 * that is a ring ("ring obstacles" above) is drawn by that section's ray rule: its hit is one more accepted t.  Every
 * other record — another type, a type 2 that is not a ring, every type 2 with the flag clear — is not rendered: it is
 * counted per agent (out_unsupported) and the image is what it would be without it.
 *
 * All arithmetic is fp64, in exactly this order, without contraction (the library is built with -ffp-contract=off).
 * Pixel (row v, column u) of agent a:
 *
 *   xc = (u - cx) / fx;  yc = (v - cy) / fy
 *   d_i = (R[i][0]*xc + R[i][1]*yc) + R[i][2]     i = 0, 1, 2
 *         (z-depth parametrisation: the point p + t d has camera z = t)
 *
 *   per type-3 cylinder:  r = 0.5*w;  z0 = z - 0.5*h;  z1 = z + 0.5*h;  ox = p.x - x;  oy = p.y - y
 *     side:  a = d0*d0 + d1*d1;  if a > 0:  b = ox*d0 + oy*d1;  c = (ox*ox + oy*oy) - r*r;  disc = b*b - a*c
 *            if disc >= 0:  s = sqrt(disc);  t = (-b - s)/a  and  t = (-b + s)/a,
 *            each accepted if t > 0 and z0 <= p.z + t*d2 <= z1
 *     caps:  if d2 != 0, for zp in (z0, z1):  t = (zp - p.z)/d2;  qx = ox + t*d0;  qy = oy + t*d1;
 *            accepted if t > 0 and qx*qx + qy*qy <= r*r
 *   ground:  if use_ground and d2 != 0:  t = (ground_z - p.z)/d2, accepted if t > 0
 *
 *   t*  = the smallest accepted t (a camera inside a cylinder sees its inner wall)
 *   d16 = (uint16) floor(t* * depth_scale + 0.5)  if t* exists and t* <= max_depth, else 0      (0 = no return)
 *   cloud point (camera frame: GridMap::projectDepthImage's back-projection of this image, grid_map.cpp:231-235):
 *     zq = d16 / depth_scale;  ( (float)((u - cx)*zq/fx), (float)((v - cy)*zq/fy), (float)zq );
 *     d16 == 0 -> three quiet NaNs (sogm_filter_point_cloud skips non-finite points: every agent hands over exactly
 *     rows*cols points, raw_range[a] = {a*rows*cols, (a+1)*rows*cols}, no compaction)
 *
 * The result is a minimum over everything accepted (cylinder sides, caps, ground, rings): it depends neither on the
 * records' order nor on any culling of records that cannot be hit within max_depth.
 */
typedef struct SogmDepthCamera {
  double  fx, fy, cx, cy;
  double  max_depth;     /* metres along the optical axis */
  double  depth_scale;   /* k_depth_scaling_factor, 1000 */
  double  ground_z;
  int32_t rows, cols;
  int32_t use_ground;
  int32_t flags;         /* SOGM_DEPTH_RINGS; other bits are ignored */
} SogmDepthCamera;       /* 72 bytes */
/*
 * Renders every agent's frame of `world` (only cylinders / n_cyl are read).  Context-free like sogm_traj_eval: the
 * current device, stream-ordered, no allocation, no host synchronisation.
 * dev cam_pos [n*3] fp64, dev cam_rot [n*9] fp64, dev out_depth [n*rows*cols] uint16 (what sogm_gridmap_update takes),
 * dev out_cloud_xyz [n*rows*cols*3] fp32 or NULL (what sogm_filter_point_cloud takes as raw_xyz),
 * dev out_unsupported [n] int32: the records that are not drawn (above).
 * SOGM_ERR_INVALID_ARG (checked first, as in sogm_create): rows, cols or n_agents < 1, n_cyl < 0, fx, fy, max_depth or
 * depth_scale not positive, max_depth*depth_scale > 65535, intrinsics that are not finite, a null required pointer, an
 * image of more than 2^31 - 1 pixels.  SOGM_ERR_NO_DEVICE without a GPU.
 */
int sogm_render_depth(const SogmWorld *world, const SogmDepthCamera *cam, int n_agents,
                      const double *cam_pos /* dev [n*3] */, const double *cam_rot /* dev [n*9] */,
                      uint16_t *out_depth /* dev [n*rows*cols] */, float *out_cloud_xyz /* dev [n*rows*cols*3] or NULL */,
                      int32_t *out_unsupported /* dev [n]: records that are not drawn */, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* agent bodies: the other vehicles of a swarm as the depth camera sees them, and a per-pixel   */
/*   hit index.  The reference has no camera (above); a vehicle is what the flight audit below   */
/*   already takes it for, the axis-aligned box body[] (0.4 x 0.4 x 0.45, sim_fake.yaml:85-87).  */
/*   The build's OWN definition, held by two independent implementations                         */
/*   (csrc/sogm_body.hpp; tests/depth_bodies_reference.py), bit for bit.                         */
/* ------------------------------------------------------------------------------------------ */
/*
 * All arithmetic is fp64, in exactly the order written, one IEEE operation at a time (+ - * /), without contraction.
 * Here min(x, y) is x if x < y, else y; max(x, y) is x if x > y, else y.
 *
 * Geometry: body j is the axis-aligned box of size size[3] centred at b = body_pos[j]:
 *     half_i = 0.5*size_i;  lo_i = b_i - half_i;  hi_i = b_i + half_i        i = 0, 1, 2
 *   This is the audit's box.  Yaw does not turn it, as it does not in the audit.
 * Not a body: if any of the three coordinates b_i is not finite, the body is not drawn.  It is counted per camera in
 *   out_unsupported, together with the world's undrawn records.
 * Own body: camera a skips body cam_body[a].  It is neither drawn nor counted.  cam_body == NULL means cam_body[a] = a.
 *   A value outside [0, n_bodies) means "this camera is carried by no body" and nothing is skipped.
 * Ray against body: the ray is p + t d, where t is the camera's z-depth parameter and d is as in "depth camera".
 *   Start with tn = -inf, tf = +inf.  For i = 0, 1, 2:
 *     if d_i == 0:  no hit unless lo_i <= p_i && p_i <= hi_i.
 *     otherwise:    ta = (lo_i - p_i)/d_i;  tb = (hi_i - p_i)/d_i;  tn = max(tn, min(ta, tb));  tf = min(tf, max(ta, tb))
 *   No hit unless tn <= tf.
 *   The accepted t is tn if tn > 0.  Otherwise it is tf if tf > 0: a camera inside another vehicle's box sees its inner
 *   wall, as it does a cylinder's.  Otherwise there is no hit.
 * The image stays a minimum over everything accepted — cylinder sides, caps, rings when SOGM_DEPTH_RINGS is set, bodies,
 *   ground.  It still depends on neither order nor culling.  Quantisation and the cloud are unchanged.
 * Hit index (out_hit, int32 per pixel, optional): SOGM_HIT_NONE when d16 == 0.  Otherwise the code of what gave t*:
 *   record i of the world -> i;  body j -> n_cyl + j;  the ground -> SOGM_HIT_GROUND.  Among equal t the winner is the
 *   lowest record index, then the lowest body index, then the ground: the code is that of the smallest (t, code) pair
 *   over records and bodies, and the ground wins only with a strictly smaller t.  It does not depend on the order in which
 *   an implementation visits records and bodies.
 */
enum { SOGM_HIT_GROUND = -1, SOGM_HIT_NONE = -2 };
typedef struct SogmDepthBodies {
  const double  *pos;       /* dev [n_bodies*3] fp64 */
  const int32_t *cam_body;  /* dev [n_agents] or NULL */
  double         size[3];   /* 0.4 0.4 0.45 */
  int32_t        n_bodies, reserved_;
} SogmDepthBodies;          /* 48 bytes */
/*
 * sogm_render_depth with the bodies drawn and, when out_hit is given, the hit index.  bodies == NULL: none (the images are
 * sogm_render_depth's).  Context-free, stream-ordered, no allocation, no host synchronisation, like sogm_render_depth.
 * dev out_hit [n*rows*cols] int32 or NULL; every other array as in sogm_render_depth.
 * SOGM_ERR_INVALID_ARG: sogm_render_depth's refusals, checked first; then n_bodies < 0, n_bodies > 0 with a null pos, a
 * size[i] that is not finite or not > 0.  SOGM_ERR_NO_DEVICE without a GPU.
 */
int sogm_render_depth_swarm(const SogmWorld *world, const SogmDepthCamera *cam, const SogmDepthBodies *bodies /* NULL: none */,
                            int n_agents, const double *cam_pos, const double *cam_rot, uint16_t *out_depth,
                            float *out_cloud_xyz /* or NULL */, int32_t *out_hit /* dev [n*rows*cols] or NULL */,
                            int32_t *out_unsupported, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* sensor noise: a deterministic noise pass over the frames the depth camera leaves on the      */
/*   device — axial noise that grows with range, uniform dropout, dropout at depth edges and a   */
/*   minimum range.  The reference intended depth noise and never shipped it                     */
/*   (grid_map.cpp:160-161, 263-264 are commented out); like the camera this is the build's OWN  */
/*   definition, held by two independent implementations (csrc/sogm_depthnoise.hpp;              */
/*   tests/depth_noise_reference.py), bit for bit.                                               */
/* ------------------------------------------------------------------------------------------ */
/*
 * All fp64 is one IEEE operation at a time (+ - * / floor) in the written order, without contraction.  No transcendentals.
 * Integers are uint64 and wrap.
 *
 * Counter-based draws — no state, no dependence on scheduling or on the branch a pixel takes:
 *   mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *            x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)            (splitmix64's step)
 *   g   = ((uint64)(agent_base + a) * rows + v) * cols + u          (the pixel's index in the whole swarm's frame)
 *   h   = mix( mix( mix(seed) ^ frame ) ^ g )
 *   w_k = mix(h + k)                                    k = 0 .. 4
 *   U(w) = (double)(w >> 11) * 2^-53                                in [0, 1)
 *   S   = sum over k in (2, 3, 4), j in (0, 1, 2, 3) of (w_k >> 16 j) & 0xFFFF          (12 pieces: Irwin-Hall)
 *   n   = ((double)S - 393210.0) * 2^-16                            mean 0, variance 1 - 2^-32, support about +-6
 * Known answers: mix(0) = 0xE220A8397B1DCDAF.  seed 0x5067, frame 3, g 0: h = 0x52E3CB0B7BF29351, S = 436624,
 *   n = 0x1.532cp-1.  Over g = 0 .. 199999 at that seed and frame: mean(n) = -0.0047, var(n) = 0.9972, share of
 *   U(w_0) < 0.05 = 0.0508.
 *
 * Pixel (a, v, u) with input d16 (camera: "depth camera" above):
 *   1. d16 == 0: no return in, no return out; nothing is counted.
 *   2. z = (double)d16 / depth_scale; count returns_in.
 *   3. uniform dropout: if U(w_0) < p_drop, count drop_uniform; no return.
 *   4. edge dropout, only when edge_jump > 0: the pixel is an edge pixel if any of its up to 8 neighbours INSIDE the image
 *      has d16_n == 0 or fabs(z_n - z) > edge_jump (z_n formed like z).  Neighbours outside the image do not exist: a 1 x 1
 *      image has no edge pixel.  An edge pixel with U(w_1) < p_edge counts drop_edge; no return.  Edges are those of the
 *      INPUT image, never of noised neighbours.
 *   5. axial noise: s = (sigma2*z + sigma1)*z + sigma0;  zn = z + s*n
 *   6. range: if !(zn >= min_depth), count below_min; no return.  Else if zn > max_depth, count beyond_max; no return.
 *      Else q = floor(zn*depth_scale + 0.5); q == 0 counts below_min (no return); otherwise d16' = (uint16)q, count
 *      returns_out (max_depth*depth_scale <= 65535 is required of the camera: q fits).
 *   7. cloud point: "depth camera"'s back-projection of d16' (three quiet NaNs for 0).
 *   8. hit: in_hit where d16' != 0, SOGM_HIT_NONE where it is 0.
 * out_counts[a*6 + i], i = 0 .. 5: returns_in, drop_uniform, drop_edge, below_min, beyond_max, returns_out.  Per agent
 *   returns_in == drop_uniform + drop_edge + below_min + beyond_max + returns_out.  The call zeroes them in stream order and
 *   adds integers: they are the same bits from run to run.
 * With every sigma, probability, edge_jump and min_depth 0 the pass is the identity on image, cloud and hit wherever
 *   d16/depth_scale <= max_depth and floor((d16/depth_scale)*depth_scale + 0.5) == d16 — every d16 the camera gives at
 *   depth_scale 1000 and a max_depth that is a whole number of quanta.
 */
typedef struct SogmDepthNoise {
  uint64_t seed;
  uint64_t frame;
  int32_t  agent_base;   /* the global index of local agent 0: a rank's shard draws what the whole swarm would */
  int32_t  flags;        /* reserved; other bits are ignored */
  double   sigma0, sigma1, sigma2;   /* s = (sigma2*z + sigma1)*z + sigma0, metres */
  double   p_drop;       /* [0, 1] */
  double   edge_jump;    /* metres; 0: no edge dropout */
  double   p_edge;       /* [0, 1] */
  double   min_depth;    /* metres */
} SogmDepthNoise;        /* 80 bytes */
/*
 * The pass over n_agents frames of cam's size.  Context-free, stream-ordered, no allocation, no host synchronisation, like
 * sogm_render_depth.  dev in_depth [n*rows*cols] uint16 and in_hit [n*rows*cols] int32 (or NULL) are only read; dev out_depth
 * [n*rows*cols] uint16, out_cloud_xyz [n*rows*cols*3] fp32 or NULL, out_hit [n*rows*cols] int32 or NULL (needs in_hit; may BE
 * in_hit: that path is per pixel), out_counts [n*6] int32.
 * SOGM_ERR_INVALID_ARG (checked first; sogm_last_error() names the rule): sogm_render_depth's camera refusals; a null noise,
 * in_depth, out_depth or out_counts; out_hit without in_hit; a parameter that is not finite; a sigma, edge_jump or min_depth
 * below 0; a probability outside [0, 1]; agent_base < 0; out_depth overlapping in_depth (the 3 x 3 test reads neighbours other
 * workgroups own, so an in-place pass is refused).  SOGM_ERR_NO_DEVICE without a GPU.
 */
int sogm_depth_noise(const SogmDepthCamera *cam, const SogmDepthNoise *noise, int n_agents,
                     const uint16_t *in_depth /* dev [n*rows*cols] */, const int32_t *in_hit /* dev [n*rows*cols] or NULL */,
                     uint16_t *out_depth /* dev [n*rows*cols] */, float *out_cloud_xyz /* dev [n*rows*cols*3] or NULL */,
                     int32_t *out_hit /* dev [n*rows*cols] or NULL */, int32_t *out_counts /* dev [n*6] */, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* ground-truth labels: the hit index carried through the voxel filter, leaf by leaf, into the   */
/*   per-point {vx, vy, vz, intensity} labels sogm_update_dsp takes.  The reference's main mode   */
/*   (FakeParticleRiskVoxel) gives its map ground-truth velocities; this is the same for the      */
/*   perception path: rendered depth -> filtered cloud with exact labels -> particle SOGM.        */
/*   The build's OWN definition, held by two independent implementations                         */
/*   (csrc/sogm_labels.hpp; tests/filter_labels_reference.py), bit for bit.                      */
/* ------------------------------------------------------------------------------------------ */
/*
 * Label arithmetic is fp32, in exactly the order written, one IEEE operation at a time, without contraction.
 *
 * Points: exactly sogm_filter_point_cloud's — the same leaves (leaf index floorf(p * inv_leaf) per axis, fp32), the same
 *   ascending leaf order, the same axis swap, isInRange and cap, the same out_count (-1 included).  Centroids carry that
 *   entry's caveat: the fp32 summation order inside a leaf is unspecified, so they agree to 1e-4, not bit for bit.
 * raw_code[i] is the hit code of raw point i: out_hit of sogm_render_depth_swarm, flattened, in the layout raw_xyz has.
 * Leaf winner: among the FINITE raw points of a leaf (a point with a coordinate that is not finite is skipped with its
 *   code), the winner is the one with the smallest camera-frame z — the front-most surface, the one a sensor would
 *   attribute the leaf to.  z is compared by the order-preserving key of its fp32 bits
 *     key(f) = bits(f) has its sign bit set ? ~bits(f) : bits(f) | 0x80000000        (unsigned compare)
 *   so -0 comes before +0.  Among equal z the LARGEST code wins: a body over a record, a record over the ground, the ground
 *   over SOGM_HIT_NONE.  This is a minimum over a set: it depends on neither point order nor scheduling.
 * Label of the winner's code c:
 *     0 <= c < n_cyl:                     v = ((float)cylinders[c].vx, (float)cylinders[c].vy, 0.0f)     (any record type)
 *     n_cyl <= c < n_cyl + n_bodies:      v_k = (float)body_vel[3*(c - n_cyl) + k]                        k = 0, 1, 2
 *     any other c (SOGM_HIT_GROUND, SOGM_HIT_NONE, out of range):  v = (0, 0, 0)
 *     s2 = (vx*vx + vy*vy) + vz*vz
 *   The label is {vx, vy, vz, 1.0f} if all three components (as fp32) are finite and s2 > min_speed*min_speed; otherwise
 *   {0, 0, 0, 0}.  (The reference draws the intensity uniformly from (0.1, 1) "for visualization"; only "> 0.01" is ever
 *   read: sogm_update_dsp takes a point with intensity > 0.01 as born dynamic with that velocity.)
 *   Velocities are in WORLD axes: sogm_update_dsp copies labels as given, next to points it has itself turned by the sensor's
 *   orientation and moved to the sensor's position (input_cloud_with_velocity) — a label is never rotated.
 * Outputs: out_labels row r of agent a, and out_code[a*cap + r] if given (the winner's code, as it came), belong to point r
 *   of out_xyz.  Rows at and beyond out_count[a] are not written.  Labels and codes are bit-identical from run to run.
 * Memory: a key array of n_agents * max_cells * 8 bytes (sogm_filter_reserve; 1 GiB at 128 agents with the default 2^20
 *   leaves) is allocated on the FIRST labelled call of a context, never by sogm_filter_point_cloud.  Plain and labelled
 *   calls may alternate on one context in any order.
 * SOGM_ERR_INVALID_ARG: sogm_filter_point_cloud's refusals, checked first; then a null raw_code, out_labels or src,
 *   n_cyl < 0, n_cyl > 0 with null cylinders, n_bodies < 0, n_bodies > 0 with null body_vel, min_speed negative or not finite.
 */
typedef struct SogmLabelSources {
  const SogmCylinder *cylinders;   /* dev [n_cyl]: the frame the hit image was rendered from (NULL if n_cyl == 0) */
  const double       *body_vel;    /* dev [n_bodies*3] fp64, world axes (NULL only if n_bodies == 0)               */
  int32_t             n_cyl, n_bodies;
  float               min_speed;   /* >= 0 */
  int32_t             reserved_;
} SogmLabelSources;                /* 32 bytes */
int sogm_filter_point_cloud_labelled(sogm_ctx *ctx, const float *raw_xyz, const int32_t *raw_code,
                                     const int32_t *raw_range, float filter_res, int cap,
                                     const SogmLabelSources *src, float *out_xyz, int32_t *out_count,
                                     float *out_labels /* dev [n_agents*cap*4] */,
                                     int32_t *out_code /* dev [n_agents*cap] or NULL */, void *stream);

/*
 * Tick glue of a batched planner service, each ONE launch (the FSM bookkeeping around replan()):
 * sogm_tick_inputs — the replan start state of every agent: its executing trajectory own_records[a] sampled at
 * stamp + replan_start_offset (FiniteStateMachine, plan_manager/src/plan_manager.cpp:169-175); an agent without a
 * trajectory (n_pieces == 0) starts from hover_inout[a] (odom, :127-133).  hover_inout [n][9] is refreshed to
 * {start position, 0, 0}.  Outputs (dev): out_now [n] = stamp (map stamp and "now" of the deconfliction),
 * out_t_start [n] = stamp + offset, out_pva [n][9], out_poses [n][3] fp32 (the map centres).
 * sogm_merge_latest — latest-wins per drone (traj_coordinator/src/particles.cpp:179-190): own_inout[a] =
 * new_records[a] where ok[a] != 0, else unchanged (a failed replan keeps executing the previous trajectory,
 * plan_manager.cpp:176-196); all_or_null, if given, receives a copy of the merged table (the swarm table of a
 * single-process run; multi-GPU runs use sogm_traj_allgather instead).
 */
int sogm_tick_inputs(const SogmTrajRecord *own_records, int n, double stamp, double replan_start_offset,
                     double *hover_inout, double *out_now, double *out_t_start, double *out_pva, float *out_poses,
                     void *stream);
int sogm_merge_latest(const SogmTrajRecord *new_records, const int32_t *ok, SogmTrajRecord *own_inout,
                      SogmTrajRecord *all_or_null, int n, void *stream);

/*
 * FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233) for a batch of agents, on the device:
 * one state record per agent and two launches per tick around the map update and sogm_replan.  The rules themselves
 * are written once, in csrc/sogm_fsm.hpp (fsm_due / fsm_step; the header compiles on the host too).  Each entry is ONE
 * launch, one lane per agent, stream-ordered, no host synchronisation.
 */
typedef struct SogmFsmParams {
  double  replan_duration;     /* fsm/replan_duration: EXEC_TRAJ asks for a replan after this long (:137-150)       */
  double  replan_start_time;   /* fsm/replan_start_time: REPLAN plans from now + this (:165-175)                    */
  double  goal_tolerance;      /* fsm/goal_tolerance: isGoalReached, |position - goal| < tolerance                  */
  double  new_plan_interval;   /* NEW_PLAN plans when more than this has passed since traj_start (:110-135; 1.0 s)  */
  int32_t replan_max_failures; /* fsm/replan_max_failures: more failures in a row -> hover record, NEW_PLAN (:176-199) */
  int32_t reserved_;
} SogmFsmParams;
typedef struct SogmFsmState { /* 24 bytes */
  double  traj_start; /* traj_start_time_                                             */
  int32_t status;     /* 0 NEW_PLAN, 1 EXEC_TRAJ, 2 REPLAN, 3 GOAL_REACHED            */
  int32_t fail;       /* num_replan_failures_                                         */
  int32_t success;    /* the member is_success_ (written by NEW_PLAN only, :110-135)  */
  int32_t reserved_;
} SogmFsmState;
/* values of sogm_fsm_apply's out_pub */
#define SOGM_FSM_PUB_NONE  0
#define SOGM_FSM_PUB_NEW   1 /* the tick's new record (plan_manager.cpp:364-399)               */
#define SOGM_FSM_PUB_HOVER 2 /* publishEmptyTrajectory's hover record (plan_manager.cpp:404-424) */
/*
 * sogm_fsm_init — dev state [n]: every agent in NEW_PLAN with traj_start = traj_start0, no failures (the machine once
 * INIT and WAIT_TARGET have passed: inputs received, goal set, execution triggered, plan_manager.cpp:96-108).
 * sogm_fsm_inputs — the head of one FSMCallback: which agents plan in this tick and from where.  out_due [n]: bit 0 a
 * NEW_PLAN agent whose new_plan_interval has passed (:110-135), bit 1 a REPLAN agent (:164-175); out_t_start [n] the
 * planning start time (stamp, or stamp + replan_start_time in REPLAN); out_pva [n][9] own_records[a] sampled there and
 * out_pos_now [n][3] sampled at stamp (sogm_traj_eval's arithmetic), an agent without a valid sample takes
 * hover_inout[a] for both (odom, :127-133); hover_inout [n][9] is then refreshed to {position now, 0, 0}; out_now [n] =
 * stamp; out_poses [n][3] fp32 the map centres (position now); out_reached [n] int32 = |position now - goals[a]| <
 * goal_tolerance (isGoalReached).  dev goals [n][3] fp64.
 * sogm_fsm_apply — the rest of the FSMCallback and its publication: the state update from this tick's results (dev int32
 * [n]: due = sogm_fsm_inputs' out_due, ok = sogm_replan's out_ok — looked at only where the agent was due —, safe =
 * sogm_traj_safe's output, reached), then own_inout[a] becomes new_records[a] (out_pub[a] = SOGM_FSM_PUB_NEW), the
 * hover record of publishEmptyTrajectory (:404-424: one 0.5 s piece, five control points at pos_now[a], start time
 * out_hover_start[a]; SOGM_FSM_PUB_HOVER) or stays untouched (SOGM_FSM_PUB_NONE, out_hover_start[a] = 0).
 */
int sogm_fsm_init(SogmFsmState *state, int n, double traj_start0, void *stream);
int sogm_fsm_inputs(const SogmFsmParams *prm, const SogmFsmState *state, const SogmTrajRecord *own_records,
                    const double *goals, int n, double stamp, double *hover_inout, double *out_now, double *out_t_start,
                    double *out_pva, float *out_poses, double *out_pos_now, int32_t *out_due, int32_t *out_reached,
                    void *stream);
int sogm_fsm_apply(const SogmFsmParams *prm, SogmFsmState *state_inout, const int32_t *due, const int32_t *ok,
                   const int32_t *safe, const int32_t *reached, const SogmTrajRecord *new_records,
                   const int32_t *drone_ids, const double *pos_now, SogmTrajRecord *own_inout, int32_t *out_pub,
                   double *out_hover_start, int n, double stamp, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* queries                                                                                     */
/* ------------------------------------------------------------------------------------------ */
/*
 * getClearOcccupancy(pos, double dt)  — fake_particle_risk_voxel.cpp:309-346 / risk_base.cpp:228-260.
 * dev agent_idx[n_q] int32, dev pos_xyz[n_q*3] fp64 (world), dev t[n_q] fp64 (seconds after the map
 * stamp; if t_is_index != 0 the value is an integer slice index, the (pos,int) overload).
 * dev out[n_q] int8: 0 free, 1 occupied, -1 out of bound.
 */
int sogm_query_clear(sogm_ctx *ctx, const int32_t *agent_idx, const double *pos_xyz,
                     const double *t, int t_is_index, int n_q, int8_t *out, void *stream);

/*
 * BaselinePlanner::isTrajSafe(T) (plan_manager/src/baseline.cpp:45-68) for every agent: the executed
 * trajectory records[a] is sampled every 0.1 s from t_now[a] to min(T, duration) and checked with
 * getClearOcccupancy(pos, t + traj_start - map_time).  The trajectory's own time_start is used where the
 * reference reads the planner's traj_start_time_ member (identical after a successful replan).
 * dev records [n_agents], dev t_now [n_agents] fp64, dev out_safe [n_agents] int32 (1 safe).
 */
int sogm_traj_safe(sogm_ctx *ctx, const SogmTrajRecord *records, const double *t_now,
                   double check_duration, int32_t *out_safe, void *stream);

/*
 * getObstaclePoints(points, t_start, t_end, lc, hc) — map.cpp:480-518 (fake map) /
 * risk_base.cpp:295-337 (RiskBase, decayed threshold).  One box per entry, points appended in the
 * reference's z,y,x,slice order.
 * dev agent_idx[n_b], box_lo[n_b*3], box_hi[n_b*3], t0[n_b], t1[n_b] (absolute seconds);
 * dev out_pts[n_b*cap*3] fp64, dev out_counts[n_b] int32 (true count; > cap means truncated).
 */
int sogm_obstacle_points(sogm_ctx *ctx, const int32_t *agent_idx, const double *box_lo,
                         const double *box_hi, const double *t0, const double *t1, int n_b,
                         double *out_pts, int32_t *out_counts, int cap, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* planner context: search + corridors + QP, batched over the same agents as the map            */
/* ------------------------------------------------------------------------------------------ */
typedef struct sogm_planner sogm_planner;

/* FakeBaselinePlanner::init / BaselinePlanner::init (baseline_fake.cpp:18-51, baseline.cpp:15-43).
 * Lifetime: a planner refers to its map context until it is destroyed — destroy planners BEFORE their sogm_ctx
 * (sogm_planner_destroy unregisters the gate / progress words the map's kernels poll and waits for them on the map's
 * device; a C++ host declares the map member before the planner member, as host/sogm_reference_api.hpp does). */
int  sogm_planner_create(sogm_ctx *map, const SogmAstarParams *astar, const SogmPlannerParams *pp,
                         const SogmQpSettings *qp, sogm_planner **out);
void sogm_planner_destroy(sogm_planner *p);

/*
 * FakeRiskHybridAstar::reset + search (fake_risk_hybrid_a_star.cpp:84-426), then
 * getPathWithVel(corridor_tau) (:663-694), for every agent.  The `init=true` search is retried with
 * `init=false` when it returns NO_PATH, as baseline_fake.cpp:284-291 does.
 * dev start_pva [n_agents*9] fp64 rows pos,vel,acc;  dev goal [n_agents*3] fp64;
 * dev t_start   [n_agents]   fp64 absolute trajectory start time (traj_start_time_)
 * dev out_ret   [n_agents]   int32 ASTAR_RET (dyn_a_star.h:15)
 * dev out_route [n_agents*route_cap*6] fp64, dev out_route_len [n_agents] int32
 *   A route longer than its row: out_route_len is the route's FULL count n (0 after NO_PATH), whatever route_cap
 *   (>= 2) is; the agent's row holds the first min(n, route_cap) points counted from the start of the route, so its
 *   first point is the same for every route_cap; points past them are left as they were.  Every consumer of (route,
 *   route_len, route_cap) — sogm_corridor_generate, sogm_corridor_rules_batched, the replan — uses
 *   min(route_len, route_cap) points and reads nothing past the agent's row.
 * dev out_stats [n_agents*4] int32 {use_node_num, iter_num, n_path_nodes, searches_run}
 * dev out_trace [n_agents*trace_cap] int32 or NULL: pool id of every popped node, in order.
 */
int sogm_astar_search(sogm_planner *p, const double *start_pva, const double *goal,
                      const double *t_start, int32_t *out_ret, double *out_route,
                      int32_t *out_route_len, int route_cap, int32_t *out_stats,
                      int32_t *out_trace, int trace_cap, void *stream);

/*
 * Corridor generation for given routes: baseline_fake.cpp:300-412 — per segment local box,
 * getObstaclePoints, firi::firi (sfc_gen/firi.hpp:238-365), ShrinkCorridor, validity LP;
 * adjacent-intersection LPs; goal reachability.  Polytopes are rows h0 x + h1 y + h2 z + h3 <= 0.
 * dev route [n_agents*route_cap*6] fp64, dev route_len [n_agents] int32 as sogm_astar_search writes them: an agent
 *   with route_len > route_cap is treated as one with route_len = route_cap (the points its row holds).
 * dev out_polys  [n_agents*SOGM_MAX_PIECES*max_faces*4] fp64
 * dev out_nfaces [n_agents*SOGM_MAX_PIECES] int32,  dev out_npoly [n_agents] int32
 * dev out_goal   [n_agents*6] fp64 local goal pos,vel
 */
int sogm_corridor_generate(sogm_planner *p, const double *start_pva, const double *t_start,
                           const double *route, const int32_t *route_len, int route_cap,
                           double *out_polys, int32_t *out_nfaces, int32_t *out_npoly,
                           double *out_goal, void *stream);

/*
 * BezierOpt::setup + optimize (traj_opt/src/bezier_optimizer.cpp:27-285) for every agent.
 * dev out_cpts [n_agents*SOGM_MAX_PIECES*15] fp64, dev out_status [n_agents] int32 (OSQP status_val:
 * 1 solved, 2 solved inaccurate (max_iter, tolerances x 10), -2 max iter, -3 primal infeasible, 3 primal infeasible
 * inaccurate, -7 KKT factorisation failed, -100 no pieces), dev out_iters [n_agents] int32.
 * Contract on the unscaled rows, viol = ||max(Ax - u, l - Ax, 0)||_inf: status 1 means viol <= (eps_abs + eps_rel
 * ||Ax||_inf) / (1 - eps_rel), 2 the same with both eps x 10; -3 / 3 only on an infeasible QP (tests/qp_contract.py).
 * replan() accepts status 1 and 2 (as BezierOpt::optimize does): a status-2 trajectory is flown.
 */
int sogm_bezier_qp_solve(sogm_planner *p, const double *start_pva, const double *goal_pv,
                         const double *polys, const int32_t *nfaces, const int32_t *npoly,
                         double *out_cpts, int32_t *out_status, int32_t *out_iters, void *stream);
/*
 * BezierOpt::setup in full (traj_opt/src/bezier_optimizer.cpp:27-54,113-260) + optimize: an arbitrary time
 * allocation t_[i] per piece (continuity rows scaled by 1 / t, 1 / t^2 of either side of a knot :164-165,191-192;
 * velocity / acceleration boxes by t, t^2 :220-246), an end state with velocity AND acceleration (:150-160,205-215)
 * and the caller's limits — replan() itself only ever asks for t_[i] = corridor_tau and a final acceleration of
 * zero (baseline.cpp:411,423), which is what sogm_bezier_qp_solve / sogm_replan assemble.
 * dev end_pva    [n_agents*9]  fp64 rows pos, vel, acc of the end state
 * dev time_alloc [n_agents*SOGM_MAX_PIECES] fp64, entries [0, npoly) used
 * Everything else as sogm_bezier_qp_solve.  (The reference writes pow(t, 2); the kernel multiplies.)
 */
int sogm_bezier_qp_solve_timed(sogm_planner *p, const double *start_pva, const double *end_pva,
                               const double *time_alloc, double max_vel, double max_acc, const double *polys,
                               const int32_t *nfaces, const int32_t *npoly, double *out_cpts,
                               int32_t *out_status, int32_t *out_iters, void *stream);

/*
 * sdlp::linprog<d> (traj_utils/include/traj_utils/sdlp.hpp:709-787) for a batch of independent problems
 *   min c^T x  s.t.  A x <= b,  d = 3 or 4
 * — the LP behind checkCorridorValidity / checkCorridorIntersect / checkGoalReachability
 * (plan_manager/src/baseline_fake.cpp:143-199) and the MVIE's deepest interior point
 * (plan_manager/include/sfc_gen/firi.hpp:150-165), one wave per problem.  Same arithmetic as sdlp's projective
 * Seidel LP; the plane insertion order is a fixed permutation of the row count (sdlp draws it from a
 * process-global std::mt19937_64, :686-705).
 * dev c [n*d], dev A [total_rows*d] row-major, dev b [total_rows], dev row_range [n*2] int32 {begin,end};
 * dev out_x [n*d], dev out_min [n]: the minimum, +inf infeasible, -inf unbounded (out_x then holds a
 * direction, :777-781); NaN when a problem has more than 152 rows (the LDS capacity of one wave's LP).
 */
int sogm_linprog_batched(int d, const double *c, const double *A, const double *b,
                         const int32_t *row_range, int n, double *out_x, double *out_min, void *stream);

/*
 * firi::firi(bd, pc, a, b, hPoly, r, iterations, epsilon) (plan_manager/include/sfc_gen/firi.hpp:238-365) as a
 * standalone call for n independent problems — the same wave-per-problem code the replan runs per path segment,
 * without its box construction, ShrinkCorridor and validity LP.  No context: the current device, scratch is
 * allocated stream-ordered.
 * dev bd [n][n_bd][4] row-major (n_bd <= 32; rows h.x + h3 <= 0), dev pc_xyz packed fp64 points with
 * dev pc_range [n][2] = {first, last+1} into it (at most max_points <= 16384 points per problem),
 * dev a, b [n][3] (the seed segment), dev r [n][3] in/out (ellipsoid radii: the reference's callers pass ones),
 * iterations >= 1 (2 at baseline.cpp:352), epsilon 1e-6 in the reference.
 * dev out_hpoly [n][max_faces][4] (max_faces <= 128), out_nfaces [n], out_status [n]: 1 = firi returned true,
 * 0 = it returned false (a or b outside bd; nothing else written), -3 = over capacity (more than max_points
 * points, or more than max_faces / 128 selected planes: the polytope is truncated).
 */
int sogm_firi_batched(const double *bd, int n_bd, const double *pc_xyz, const int32_t *pc_range, const double *a,
                      const double *b, double *r, int iterations, double epsilon, int n, int max_points,
                      int max_faces, double *out_hpoly, int32_t *out_nfaces, int32_t *out_status, void *stream);

/*
 * Per-object use of the per-stage entries (host/sogm_reference_api.hpp): after select_agents(first, count),
 * sogm_astar_search / sogm_corridor_generate / sogm_bezier_qp_solve / sogm_safe_after_opt process agents
 * [first, first + count) only; every array keeps its full [n_agents] layout and is indexed by the absolute agent.
 * (0, n_agents) restores the default.  sogm_replan always processes every agent.
 * set_search_mode: 0 (default) = the replan's call pattern — search(…, init_search = true, …) and, if that returns
 * NO_PATH, reset() + search(…, false, …) (baseline_fake.cpp:284-291); 1 / 2 = exactly one
 * RiskHybridAstar::search with init_search = true / false (risk_hybrid_a_star.h:103-110).  Adding 4 makes
 * sogm_astar_search read t_start[] as that function's time_start argument (seconds after the map stamp) instead of
 * an absolute time.  Adding 16 selects search(…, dynamic = false, …): the reference's branch reads node times it never
 * writes (risk_hybrid_a_star.cpp:153-158,177,271,324); they are DEFINED as zero here (oracle/astar_oracle.cpp does the
 * same): a spatial search over the SOGM's first tau seconds, t_start ignored.
 */
int sogm_planner_select_agents(sogm_planner *p, int first, int count);

int sogm_planner_set_search_mode(sogm_planner *p, int mode);

/*
 * ParticleATC::isSafeAfterOpt (traj_coordinator/src/particles.cpp:223-283) for every agent: the new
 * trajectory's control points must be linearly separable (separator::Separator::solveModel,
 * utils/separator/src/separator_glpk.cpp:75-190 — a GLPK feasibility LP, solved here with the
 * planner's own LP) from the remaining control points of every other agent's active trajectory.
 * dev cpts [n_agents*SOGM_MAX_PIECES*15] fp64 (sogm_bezier_qp_solve layout), dev npoly [n_agents],
 * dev records [n_records], dev ego_ids [n_agents], dev t_now [n_agents] fp64 ("ros::Time::now()" of the
 * check), dev out_safe [n_agents] int32 (1 safe, 0 collides / LP capacity exceeded; agents with
 * npoly <= 0 report 1).
 */
int sogm_safe_after_opt(sogm_planner *p, const double *cpts, const int32_t *npoly,
                        const SogmTrajRecord *records, int n_records, const int32_t *ego_ids,
                        const double *t_now, int32_t *out_safe, void *stream);
/*
 * Makes sogm_replan() finish like FakeBaselinePlanner::replan does (baseline_fake.cpp:453-460): with
 * a swarm set, a trajectory that fails isSafeAfterOpt against `records` counts as a failed replan.
 * The device pointers are read by later sogm_replan() calls; records == NULL switches the check off.
 */
int sogm_planner_set_swarm(sogm_planner *p, const SogmTrajRecord *records, int n_records,
                           const int32_t *ego_ids, const double *t_now);
/*
 * The reference plans only in NEW_PLAN (once per new_plan_interval) and REPLAN (plan_manager.cpp:110-135,164-175): with a
 * mask set, later sogm_replan() calls plan only the agents with due[a] != 0 (dev int32 [n_agents], read by those calls:
 * sogm_fsm_inputs' out_due).  An agent that is not due ends like a replan whose search found no path — out_ok 0, an
 * empty record, its published record kept — without expanding a node, and moves none of sogm_planner_counters.
 * NULL (the default): every agent plans.  sogm_flight_run does not look at the mask: a flight runs the machines itself,
 * per agent, once they are registered with sogm_planner_set_flight_fsm.
 * The planner keeps the POINTER, not a copy: the mask stays in force for every later sogm_replan() until another call
 * replaces it or passes NULL, each of those calls reads the buffer's contents as they are when its searches run (stream
 * order), and the buffer must stay allocated until they have completed or the mask has been replaced.
 */
int sogm_planner_set_due(sogm_planner *p, const int32_t *due_dev_or_null);

/*
 * Cumulative counters of sogm_replan() since creation / the last reset: where each replan ended (the early
 * returns of baseline_fake.cpp:292,405-419,447,455) and how often a capacity limit that the reference does not
 * have (it grows std::vectors) turned a corridor / a deconfliction check into a failure.  Synchronous.
 * host out[SOGM_CNT_N] int64.
 */
enum {
  SOGM_CNT_REPLAN_OK           = 0, /* replan() returned true                                        */
  SOGM_CNT_FAIL_SEARCH         = 1, /* A* NO_PATH after the retry (:284-295)                         */
  SOGM_CNT_FAIL_CORRIDOR       = 2, /* no usable corridor (:405-419)                                 */
  SOGM_CNT_FAIL_QP             = 3, /* OSQP status not SOLVED / SOLVED_INACCURATE (:447)             */
  SOGM_CNT_FAIL_UNSAFE         = 4, /* isSafeAfterOpt false (:455-460)                               */
  SOGM_CNT_CORRIDOR_CAPACITY   = 5, /* corridor chains cut at a segment that exceeded pc_capacity points,
                                       128 selected planes or max_faces (treated as invalid)         */
  SOGM_CNT_PIECES_CAPACITY     = 6, /* routes longer than SOGM_MAX_PIECES segments (truncated)       */
  SOGM_CNT_DECONFLICT_CAPACITY = 7, /* pairs with more than 144 LP rows (treated as unsafe)          */
  SOGM_CNT_N                   = 8
};
/*
 * Publication inside the replan.  The reference's FSM publishes a successful replan's trajectory and keeps executing
 * the previous one otherwise (plan_manager.cpp:176-199,364-399); every other drone stores what it receives
 * (particles.cpp:131-191).  sogm_merge_latest does that in a launch of its own after sogm_replan; with a table
 * registered here the replan's finishing kernel does it per agent as its chain completes (same stores, overlapped with
 * the other agents' chains — beside the streaming clear a separate store-heavy launch takes 2 ms):
 *   own_records [n_agents]  dev: overwritten with the new record where the replan succeeded (latest wins);
 *   next_table  [n_agents]  dev or NULL: receives every agent's CURRENT record (new, or the one it keeps executing) —
 *                           the swarm table of the NEXT tick for a single-process host (n_total == n_agents), which
 *                           must differ from the table registered with sogm_planner_set_swarm for this replan
 *                           (sogm_replan returns SOGM_ERR_INVALID_ARG when the two are the same table, or when
 *                           own_records overlaps its out_records: the finishing kernel would write what other agents'
 *                           deconfliction reads in the same launch).
 * NULL, NULL switches it off (the default).  Pointers are read by later sogm_replan calls.
 */
int sogm_planner_set_publish(sogm_planner *p, SogmTrajRecord *own_records, SogmTrajRecord *next_table);

/* Pre-stamp.  The tick's critical path is "map update -> chain of the slowest agent", yet an agent's next map centre
 * depends on its own new record only, which is final when its replan finishes.  With a SogmPrestamp registered (and
 * publication on, two or three grids per agent, the sparse reset, the dataflow replan), sogm_replan also builds the NEXT
 * tick's map —
 * sogm_tick_inputs' start states, then FakeParticleRiskVoxel::updateMap's stamp (fake_particle_risk_voxel.cpp:80-170)
 * — agent by agent as their records are published, into the pool's next grid; the next tick then calls
 * sogm_update_prestamped (the grid swap + the neighbour overlay) instead of sogm_tick_inputs + sogm_update_gt_swarm.
 * Same cells, same start states.  ps = NULL switches it off; the arrays stay owned by the caller and must not be the
 * ones the replan in flight reads (start_pva, t_start: double-buffer them).  A replan that could not pre-stamp (no
 * spare grid ready yet: first ticks) leaves sogm_update_prestamped returning SOGM_ERR_STATE: fall back to the two
 * calls.
 * Stream order: a pre-stamping sogm_replan leaves `stream` behind its own outputs (out_records, out_ok), NOT behind the
 * pre-stamp, which goes on for a few hundred microseconds on a stream of the context.  The SogmPrestamp outputs and the
 * pre-stamped grid are complete in stream order behind the next sogm_update_prestamped / sogm_update_* / sogm_replan
 * call on a stream (each joins it), or after a device synchronisation — sogm_update_prestamped launches its overlay
 * under that tail, an agent's additions waiting for that agent's stamp.  Tuning key "splat_overlap" = 0 restores the
 * join inside sogm_replan.
 * Failed ticks: if the pre-stamping replan failed on the device (sogm_planner_flow_failures), its grid is incomplete;
 * sogm_update_prestamped then returns SOGM_ERR_STATE once the failure has reached the host — rebuild the map with
 * sogm_tick_inputs + sogm_update_gt_swarm, which discards the grid and clears the stamp's bitmask. */
typedef struct SogmPrestamp {
  const float        *cloud_xyz;    /* next update's inputs, as for sogm_update_gt (device) */
  const int32_t      *cloud_range;
  const SogmCylinder *cylinders;
  int32_t             n_cyl;
  int32_t             reserved_;
  double              next_stamp;           /* sogm_tick_inputs' stamp of the next tick */
  double              replan_start_offset;
  double             *hover_inout;          /* sogm_tick_inputs' in/out and outputs for the next tick (device) */
  double             *out_now;
  double             *out_t_start;
  double             *out_pva;
  float              *out_poses;            /* the next map centres, [A][3] (may be NULL: the context keeps its own) */
  const SogmWorld    *world;                /* host pointer or NULL.  Non-NULL: the stamp's inputs are this frame, cropped on the
                                               device around each agent's NEXT map centre, and cloud_xyz / cloud_range /
                                               cylinders above are ignored (may be NULL).  CAUSALITY: a pre-stamp runs inside
                                               tick k, so the newest frame a live host can hand it is tick k's — the map tick
                                               k + 1 plans on is then one tick staler than the reference's, which updates from
                                               the cloud that arrived for that update (map.cpp:170-171).  bench.py reports this
                                               as config.map_input_staleness_ticks = 1 and keeps the 0-staleness tick
                                               (sogm_update_world at the start of the tick) as the headline. */
} SogmPrestamp;
int sogm_planner_set_prestamp(sogm_planner *p, const SogmPrestamp *ps);
/* 1 if the last sogm_replan pre-stamped the next grid (no synchronisation: host-side state). */
int sogm_prestamp_pending(const sogm_ctx *ctx);
/* `stream` waits for the end of the last replan's pre-stamp, if nothing has joined it yet (see "Stream order" above):
 * for a host that touches the SogmPrestamp arrays itself — e.g. sogm_tick_inputs on the same hover_inout — before its
 * next sogm_update_* / sogm_replan call.  No-op otherwise. */
int sogm_prestamp_join(sogm_ctx *ctx, void *stream);
/* The update of a pre-stamped tick: adopts the grid, its map centres and stamps, then adds the neighbour overlay
 * (records may be NULL with n_records = 0).  A grid whose pre-stamping replan FAILED is refused (SOGM_ERR_STATE: build the
 * map with sogm_update_gt* / sogm_update_world instead) — decided on two levels: while the pre-stamp is still running the
 * overlay waits per agent on the device and writes nothing once that replan's error word is set (the tick is then
 * reported as failed by sogm_planner_flow_failures); the HOST check (the failure count against its value when the pre-stamp
 * was queued) sees a failure only once the failing replan's report has run, i.e. it is exact after a synchronisation of
 * the stream and best-effort for a host that pipelines ticks without one. */
int sogm_update_prestamped(sogm_ctx *ctx, const SogmTrajRecord *records, int n_records, const int32_t *ego_ids,
                           void *stream);
/*
 * Flight: n_ticks replan ticks of every agent of the batch in ONE call, every agent on its own clock — the reference's
 * drones each run their own FSM and read whatever trajectories arrived last (plan_manager/src/plan_manager.cpp:92-233,
 * traj_coordinator/src/particles.cpp:179-190); a lock-step sogm_replan per tick makes 127 agents wait for the slowest
 * chain of every tick.  RESULTS are fixed by a staleness rule, so a flight is reproducible whatever the schedule:
 *   agent a's tick k  =  FakeParticleRiskVoxel::updateMap from worlds[k] around a's start state of tick k (sampled from
 *   its own record of tick k - 1 at t0 + k * period + replan_start_offset), overlay and isSafeAfterOpt against table
 *   ver(k - 2) — every agent's executed record as of ITS tick k - 2 —, then FakeBaselinePlanner::replan; a may start tick
 *   k as soon as its own tick k - 1 is finished and EVERY agent has finished tick k - 2.
 * (sogm_replan's lock-step tick reads ver(k - 1): the flight's neighbour records are one tick staler, like a record that
 * missed one broadcast period.)  tables is a ring of four versions, ver(j) at tables[(j & 3) * n_total]: on entry ver(first_tick - 1)
 * and ver(first_tick - 2) must hold the swarm's records of those ticks (a fresh flight: the initial table — empty or hover
 * records — in both); on return ver(first_tick + n_ticks - 1) and ver(first_tick + n_ticks - 2) are complete, i.e. a
 * following call with first_tick advanced by n_ticks continues the flight.  Needs the sparse reset (the agent's single grid is
 * reset through its mark log at the start of each of its ticks), body particles, 32-byte aligned agent grids.
 * Several ranks (n_total > n_agents: the batch is rows agent0 .. agent0 + n_agents - 1, the other rows belong to other
 * ranks).  With `nccl_comm` set (an ncclComm_t, e.g. sogm_comm_handle) the exchange runs BEHIND the call, no host step
 * between ticks: for every tick j of the call the library queues, on the context's exchange stream, a one-lane kernel that
 * waits until every LOCAL agent has finished tick j, the in-place ncclAllGather of this rank's rows of ver(j)
 * (tables[(j & 3) * n_total + agent0], n_agents records), and a one-lane kernel that marks ver(j) complete and queues the
 * overlays of tick j + 2 parked at the gate; the gate of tick k's overlay is then "the all-gather of ver(k - 2) has completed
 * here" — the same staleness rule, so the records equal those of one process flying all agents.  Every rank passes the same
 * n_ticks (the collectives are matched one to one); a rank whose flight failed still runs all of its collectives.  The
 * call's last two versions are complete when the exchange stream has drained: `stream` waits for it as for the flight.
 * Without `nccl_comm` a call flies at most TWO ticks — ticks k and k + 1 read ver(k - 2) and ver(k - 1), which the host
 * completes between two calls by all-gathering every rank's rows of the versions the previous call finished
 * (sogm_traj_allgather, in place).  Both forms: tests/test_exchange_gpu.py (two ranks on one GPU, stand-in RCCL).  Four persistent kernels on
 * four streams with disjoint compute-unit masks (tuning keys flight_*_units, 16 CUs per unit); asynchronous: `stream`
 * waits for the flight's end.  SOGM_ERR_STATE if the planner was created without the dataflow path.
 */
typedef struct SogmFlight {
  int32_t          n_ticks;              /* 1 .. 64 */
  int32_t          first_tick;           /* absolute index of this call's first tick (>= 0) */
  double           t0, period;           /* stamp of tick k = t0 + k * period */
  double           replan_start_offset;  /* fsm/replan_start_time */
  const SogmWorld *worlds;               /* host array [n_ticks]: the sensor frame of tick first_tick + i */
  const double    *goals;                /* dev [A][3] */
  const int32_t   *drone_ids;            /* dev [A]  (ego ids of the batch = rows agent0 .. agent0 + A - 1 of the tables) */
  double          *hover_inout;          /* dev [A][9] where an agent without a trajectory hovers (sogm_tick_inputs) */
  SogmTrajRecord  *own_inout;            /* dev [A] the records the agents execute (latest wins) */
  SogmTrajRecord  *tables;               /* dev [4][n_total] */
  int32_t          n_total, agent0;
  SogmTrajRecord  *log_records;          /* dev [n_ticks][A] every tick's sogm_replan-style output record ... */
  int32_t         *log_ok;               /* dev [n_ticks][A] ... and ok flag */
  void            *nccl_comm;            /* several ranks: the communicator of the exchange behind the call (see above); NULL:
                                            one process owns every row, or the host all-gathers between calls of two ticks */
} SogmFlight;
int sogm_flight_run(sogm_planner *p, const SogmFlight *flight, void *stream);
/*
 * The flight under the per-agent FSM (opt-in; without it a flight replans every agent in every tick, as above).  With a
 * SogmFlightFsm registered, agent a's tick k of a later sogm_flight_run is ONE FiniteStateMachine::FSMCallback
 * (plan_manager/src/plan_manager.cpp:92-233) under the flight's staleness rule:
 *   head    sogm_fsm_inputs for the agent, from state_inout[a] and its own record of tick k - 1: who is due, the planning
 *           start time (the stamp, or stamp + prm.replan_start_time in REPLAN — SogmFlight::replan_start_offset is not
 *           used), the start state sampled there, and the position at the stamp: the map centre, the refreshed hover row
 *           and the goal test;
 *   map     as without the mode (every agent, due or not: isTrajSafe needs it);
 *   search  only where the agent is due; an agent that is not due goes the way sogm_planner_set_due describes (no
 *           expansion, statistics 0/0/0/0, corridors / QP / finish see a failed search, no outcome counter moves);
 *   finish  BaselinePlanner::isTrajSafe(check_duration) (baseline.cpp:45-68, sogm_traj_safe's verdict bit for bit) of the
 *           record the agent executes against its complete map of this tick, the replan's finish, then sogm_fsm_apply for
 *           the agent: the state back into state_inout[a], and for SOGM_FSM_PUB_HOVER publishEmptyTrajectory's record
 *           (plan_manager.cpp:404-424) into own_inout[a] and the agent's row of ver(k).
 * log_ok[k][a] is then the replan's ok as the due gate leaves it (0 where the agent was not due) and log_records[k][a] the
 * replan's output record (empty where the agent was not due or its replan failed): a lock-step tick's sogm_replan outputs
 * under sogm_planner_set_due.  No kernel gains a wait: the head's results travel in per-agent arrays beside the start state.
 * The struct is COPIED at the call and its pointers are kept: it is in force for every later sogm_flight_run until another
 * call replaces it or passes NULL (off, the default); sogm_replan never looks at it.  SOGM_ERR_INVALID_ARG (with a
 * sogm_last_error text): state_inout NULL, a parameter that is negative or not finite; sogm_flight_run returns the same
 * while the mode is on and n_total != n_agents (flights of several ranks under the FSM are not supported).
 */
typedef struct SogmFlightFsm {
  SogmFsmParams   prm;
  double          check_duration;   /* isTrajSafe's horizon, fsm/colli_check_duration (0.2) */
  SogmFsmState   *state_inout;      /* dev [A]: in = states before the call's first tick, out = after its last */
  /* per-tick logs of the NEXT flight, dev, each may be NULL; [n_ticks][A] unless noted */
  SogmFsmState   *log_state;        /* state after the tick */
  int32_t        *log_due, *log_safe, *log_reached, *log_pub;
  double         *log_hover_start;
  SogmTrajRecord *log_own;          /* the record the agent executes after the tick (own_inout[a] at its finish) */
} SogmFlightFsm;
int sogm_planner_set_flight_fsm(sogm_planner *p, const SogmFlightFsm *fsm_or_null);
/* Optional: creates the flight's control block and its five streams (four masked ones + the exchange stream), runs an empty
 * kernel on each, so that their hardware queues exist before any flight is in the air, and allocates what the first
 * sogm_flight_run would allocate (crop lists for frames of up to max_cloud_points points, the stamp's scratch) — the first
 * call otherwise synchronises the DEVICE while it grows them.  For a host that flies several planners in ONE process (a
 * second planner's first call would wait for the first planner's flight to end).  Reads the flight_* tuning keys like the
 * first sogm_flight_run would.  Synchronises. */
int sogm_flight_prepare(sogm_planner *p, int max_cloud_points);
/* After a flight (synchronises): host out_ms[A][8] = per-agent sums over the last flight in ms {wait at the tick k - 2 gate,
 * map (reset + stamp + overlay), search (queue + A*), corridors (queue + FIRI), QP (queue + solve), finish, whole chain,
 * ticks completed}; host out_hdr[32] = the flight's control counters ([4] = error code, 0 = none; [5] = agent-ticks
 * finished; [15] = workgroups of the flight's four kernels that were NOT running within 1 ms of their kernel's first workgroup — must be
 * 0: every kernel's compute-unit mask holds the same number of units in every shader engine it touches and a launch has
 * exactly the workgroups that mask holds at once, so nothing waits in a dispatcher that a queue save / restore could start
 * ahead of a restored wave (DESIGN.md 3.1 "Liveness of the flight"); [16..24] = wave time of the map / corridor + finish kernels by activity, in units of 10 us: map workers idle,
 * reset, bits, marks, overlay, heads, light waves idle, corridor segments, finish; [25..31] = descriptor counts). */
int sogm_flight_stats(sogm_planner *p, double *out_ms_host, int32_t *out_hdr_host);
int sogm_planner_counters(sogm_planner *p, int64_t *out_host, int reset);
/* sogm_replan() chains its kernels per agent through device-side ready lists ("dataflow replan");
 * a wait that exceeds 3 s marks the tick as failed instead of hanging the GPU: agents whose chain did not complete
 * report ok = 0 and an empty record (n_pieces = 0) for that tick.  Synchronises the device and returns 0 if the
 * last sogm_replan() completed normally, a positive code if one of its waits timed out, negative = sogm_status.
 * The codes — which kernel waited for what (the same values in sogm_flight_stats out_hdr[4] for a flight, and, as 100 + code,
 * in sogm_planner_flow_failures after a failed flight; enum FlowCode of csrc/sogm_handover.hpp):
 *    1  k_flow_gate: every search workgroup of the replan resident
 *    2  k_worker_flow (corridor blocks / finishing blocks) / k_prestamp_flow: its entry of the ready list (searches done / QPs done / records published)
 *    3  k_qp_flow: its entry of the list of agents whose corridors are final
 *    4  the second search attempt (k_astar, k_flight_search): the first attempt's verdict
 *    6  k_prestamp_flow, k_update_flow, the heads of k_flight_map: a stage counter (the lower tickets of the agent's stamp; the
 *       admission window)
 *    7  k_prestamp_gate: corridors final, QP workgroups and finishing waves resident
 *    8  k_splat_neighbours behind a pre-stamp: the agent's pre-stamp complete
 *   12  k_flight_search / k_flight_qp: its position of the map-ready / corridors-final ring
 *   15  three waiters for a work-queue descriptor: k_flight_light, the workers of k_flight_map on the plain and on the urgent queue
 *   16  two waiters, in different error words: k_astar beside an update flow (replan): the agent's map of this tick; a plain head of
 *       k_flight_map (flight): its turn in the admission order
 *   17  a plain head of k_flight_map: its position of the ring of finished agents */
int sogm_planner_flow_error(sogm_planner *p);
/* The same without synchronising anything: out[0] = code of the most recent failed tick (0 = none ever),
 * out[1] = number of sogm_replan() calls that failed so far, as of the ticks that have COMPLETED on the device
 * (the words live in pinned host memory and are written by the last kernel of each replan).  A tick driver polls
 * this once per tick and stops merging records when the count moves (the reference has no analogue: its replan()
 * cannot time out). */
int sogm_planner_flow_failures(sogm_planner *p, int32_t out[2]);

/*
 * One full FakeBaselinePlanner::replan (baseline_fake.cpp:266-472; isSafeAfterOpt only when a swarm has
 * been set with sogm_planner_set_swarm) for every
 * agent: search -> corridors -> QP, stream-ordered, no host round trip.  On success writes the
 * agent's SogmTrajRecord (time_start = t_start) into out_records; on failure writes n_pieces = 0.
 * dev out_ok [n_agents] int32 (1 = replan() returned true).
 */
int sogm_replan(sogm_planner *p, const double *start_pva, const double *goal,
                const double *t_start, const int32_t *drone_ids, SogmTrajRecord *out_records,
                int32_t *out_ok, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* flight audit: what the swarm flies against the world that is there (the reference took these   */
/*   numbers from its eval_helper submodule, absent from its tree)                                */
/* ------------------------------------------------------------------------------------------ */
/*
 * Semantics (one definition; tests/swarm_audit_reference.py restates it in numpy):
 *   - What an agent flies (traj_server/src/bezier_traj_server.cpp): commands sampled every sample_dt (DELTA_T = 0.01 s,
 *     :34); a new trajectory takes over at its start_time (bezierCallback :283-357); after its end the last point is held
 *     (PubCallback :415+).
 *   - Input: EXECUTED tables.  tables[k][a] is the record agent a executes after tick k (the latest-wins table).
 *   - Samples: tick k of a call has the stamp t_k = t0 + (first_tick + k) * period (the tick driver's own expression) and the
 *     samples t = t_k + j * sample_dt, j = 0 .. m - 1, m = period / sample_dt, which must be a whole number to 1e-9.  Times
 *     are built from integers: auditing ticks in several calls gives the same samples as one call.
 *   - Record: tables[k][a] is evaluated at t if it has n_pieces > 0 and time_start <= t; otherwise tables[k - 1][a] under the
 *     same test (for k = 0 of a call: prev_table, or none if NULL); otherwise the agent is at fallback_pos[a] (where it hovers
 *     before its first trajectory).  Evaluation is sogm_traj_eval's (clamped to [time_start, time_start + total]: the end
 *     point is held).
 *   - Body: an axis-aligned box of size body[] (0.4, 0.4, 0.45: plan_manager/config/sim_fake.yaml:85-87).
 *   - Agent-agent collision at a sample: |dx| < bx && |dy| < by && |dz| < bz (two boxes overlap).  The separation is the
 *     Euclidean distance of the two centres.
 *   - Agent-obstacle collision (SogmCylinder type 3): diameter w, z extent [z - h/2, z + h/2], axis at time t at
 *     (x + vx (t - t_obstacles), y + vy (t - t_obstacles)).  The z extents overlap if |pz - z| < (h + bz) / 2.  The gap is
 *     the xy distance from the axis to the body's xy rectangle minus w / 2 (-w / 2 when the axis is inside the rectangle);
 *     a collision is z overlap and gap < 0.
 *   - Agent-ring (type 2, only with SOGM_AUDIT_RINGS set in flags): the body-box rule of "ring obstacles" with the centre
 *     at time t at (x + vx (t - t_obstacles), y + vy (t - t_obstacles), z).  Its gap takes part in min_gap at every sample
 *     and a collision is gap < 0; `other` / min_gap_obstacle is the record's index in cylinders[], kind stays
 *     SOGM_AUDIT_OBSTACLE.  With the flag clear type 2 is refused like any other type, and so is a type 2 that is not a
 *     ring with the flag set (below).
 *   - Goal: the first sample with |p - goal| < goal_tolerance (1.0: fsm/goal_tolerance, sim_fake.yaml:5).
 *   - Path length: sum of |p(t_i) - p(t_(i-1))| over consecutive samples, carried across calls (last_pos).
 *   - Minima break ties by the earliest sample, then the lowest index.  Events: one per colliding (sample, agent, other or
 *     obstacle), ordered by (tick, sample, agent, kind, other) within a call and appended in call order; when
 *     event_capacity runs out the earliest are kept and *n_events still counts every one (a count -> exclusive scan ->
 *     write, no order-dependent atomic: the output is bit-identical on repeated runs).
 */
typedef struct SogmAuditParams {
  double  body[3];          /* box size, 0.4 0.4 0.45 */
  double  sample_dt;        /* 0.01 */
  double  goal_tolerance;   /* 1.0 */
  double  t_obstacles;      /* the instant cylinders[] describes */
  int32_t event_capacity;   /* entries of events[] (>= 0) */
  int32_t flags;            /* SOGM_AUDIT_RINGS; other bits are ignored */
} SogmAuditParams;

/* One audited agent's accumulator; sogm_audit_init_agents sets +inf minima, -1 times and indices, zero counts. */
typedef struct SogmAuditAgent {
  double  min_gap, min_gap_time;   /* smallest obstacle gap over samples with z overlap (+inf if none) */
  double  min_sep, min_sep_time;   /* smallest centre distance to any other agent (+inf if none) */
  double  goal_time;               /* first arrival, -1 never */
  double  first_collision_time;    /* first sample in collision of either kind, -1 never */
  double  path_length, last_pos[3];
  int32_t min_gap_obstacle, min_sep_agent;
  int32_t obstacle_samples, agent_samples;   /* samples in collision, per kind */
  int32_t n_samples, has_last;
} SogmAuditAgent;

enum { SOGM_AUDIT_AGENT = 0, SOGM_AUDIT_OBSTACLE = 1 };
typedef struct SogmAuditEvent {
  double  t;
  int32_t agent, other, kind, reserved_;   /* kind SOGM_AUDIT_AGENT (other = agent index) | SOGM_AUDIT_OBSTACLE (cylinder) */
} SogmAuditEvent;

/* dev acc [n_local]: the initial accumulator, stream-ordered. */
int sogm_audit_init_agents(SogmAuditAgent *acc, int n_local, void *stream);
/*
 * Audits n_ticks executed tables (rows [agent0, agent0 + n_local) against all n_total rows and the cylinders) and adds the
 * result to acc / events.  Stateless: the current device, the caller's stream, stream-ordered scratch; no streams, events or
 * host synchronisation.
 * dev tables [n_ticks][n_total], dev prev_table [n_total] or NULL (the table before tables[0]), dev fallback_pos [n_total][3],
 * dev goals [n_local][3], dev cylinders [n_cyl] (NULL if n_cyl == 0), dev acc [n_local] in/out, dev events [event_capacity]
 * (NULL if the capacity is 0), dev n_events [1] in/out: every colliding sample seen so far, kept or not.
 * SOGM_ERR_INVALID_ARG (with sogm_last_error text) for null pointers, counts out of range, period / sample_dt not whole.
 * The cylinders are device data the call does not read on the host: a record that is not audited (a type other than 3;
 * with SOGM_AUDIT_RINGS, other than 3 or a type 2 that is a ring) makes the call add nothing and set *n_events = -1, which every later call keeps (the Python binding refuses such obstacles on the host).
 */
int sogm_swarm_audit(const SogmAuditParams *prm, const SogmTrajRecord *tables, int n_ticks, int n_total,
                     const SogmTrajRecord *prev_table, double t0, int first_tick, double period, int agent0, int n_local,
                     const double *fallback_pos, const double *goals, const SogmCylinder *cylinders, int n_cyl,
                     SogmAuditAgent *acc, SogmAuditEvent *events, int32_t *n_events, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* map audit: how far a perceived SOGM is from the ground-truth SOGM, agent by agent and future   */
/*   slice by future slice.  The reference has no such figure: this is the build's OWN            */
/*   instrument, held by two readings (csrc/sogm_mapaudit.hpp + csrc/sogm_mapaudit.hip, and the   */
/*   numpy restatement tests/map_audit_reference.py), count for count.                            */
/* ------------------------------------------------------------------------------------------ */
/*
 * Two contexts, `test` (the map under judgement: e.g. a SOGM_MAP_RISKVOXEL context that sogm_dsp_publish fills) and `truth`
 * (e.g. a SOGM_MAP_FAKE context that sogm_update_world fills), on the same device, with the same n_agents, L, W, H and a
 * resolution equal bit for bit.  T, map_kind and storage (fp32 / fp16 cells, rows / 2 x 2 x 2 tiles) may differ.  A cell is
 * named by its LOGICAL index (ix, iy, iz), 0 <= ix < L, 0 <= iy < W, 0 <= iz < H, whatever the storage.
 *
 * Occupancy.  O(c) = value(c) > thr, where value(c) is the stored cell converted to fp32 (an fp16 cell: the stored half,
 *   converted exactly) and the comparison is fp32 and strict: a value equal to thr is not occupied, a NaN is not occupied.
 *   The test side uses thr_test, the truth side thr_truth.
 *
 * Region R (the same for every slice of an agent).  A cell is in R when box_lo[d] <= i_d < box_hi[d] for d = 0, 1, 2 (all six
 *   zero: the whole grid) and, with SOGM_MAPAUDIT_FRUSTUM set in flags, it passes the frustum test.  All of it fp64, in
 *   exactly this order, without contraction; R is the row-major camera-to-world rotation cam_rot[agent] of "depth camera"
 *   (camera frame: x right, y down, z forward) and the camera sits at the map centre, where sogm_dsp_publish puts it:
 *     p_d = ((double)i_d + 0.5) * (double)resolution - (double)range_d       d = 0, 1, 2
 *           range_0 = (float)(L / 2) * resolution, range_1 = (float)(W / 2) * resolution, range_2 = (float)(H / 2) * resolution
 *           (fp32 products, integer halves: the map's local_update_range)
 *     q_j = (R[0][j]*p_0 + R[1][j]*p_1) + R[2][j]*p_2                         j = 0 (x), 1 (y), 2 (z)
 *     in view iff  q_z > near_z  &&  q_z <= far_z  &&  fabs(q_x) <= q_z*tan_h  &&  fabs(q_y) <= q_z*tan_v
 *   A rotation that is not finite puts no cell in view (every comparison with a NaN is false; far_z is finite).
 *
 * Neighbourhood.  D_r(O)(c) is true when some cell c' of the grid (anywhere in it, not only in R) has O(c') and
 *   max(|ix - ix'|, |iy - iy'|, |iz - iz'|) <= r.  Grid edges do not wrap.  r = tolerance, 0 .. 3.
 *
 * Counts.  Test slice t of agent a is compared with truth slice s = slice_map[t]; out[a * T_test + t] is
 *     n_region      |R|
 *     n_test        |O_test  &  R|
 *     n_truth       |O_truth &  R|
 *     n_both        |O_test  &  O_truth  &  R|
 *     n_test_near   |O_test  &  D_r(O_truth)  &  R|     (test cells with a truth cell within r: the numerator of precision)
 *     n_truth_near  |O_truth &  D_r(O_test)   &  R|     (truth cells with a test cell within r: the numerator of recall)
 *     truth_slice   s
 *     status        0 audited | SOGM_MAPAUDIT_CENTRE | SOGM_MAPAUDIT_SKIPPED
 *   With r = 0 both near counts equal n_both.  Precision (n_test_near / n_test) and recall (n_truth_near / n_truth) are the
 *   caller's divisions.  Rows are overwritten, not accumulated; only integer adds are used, so the output is bit-identical
 *   from run to run.
 *   SOGM_MAPAUDIT_CENTRE: the two maps' centres of this agent (sogm_map_state's) differ in any bit of their three floats:
 *     the cells do not coincide, all six counts of all its rows are zero (truth_slice is still slice_map[t]); other agents are
 *     not affected.
 *   SOGM_MAPAUDIT_SKIPPED: slice_map[t] == -1: all six counts are zero, truth_slice is -1.  (An agent with differing centres
 *     reports SOGM_MAPAUDIT_SKIPPED for such a row.)
 *   out_dt[a] = test stamp - truth stamp (fp64, sogm_map_state's times): reported, not judged.
 */
enum { SOGM_MAPAUDIT_FRUSTUM = 1 };                            /* SogmMapAuditParams.flags; other bits are ignored */
enum { SOGM_MAPAUDIT_CENTRE = 1, SOGM_MAPAUDIT_SKIPPED = 2 };  /* SogmMapAuditRow.status */
#define SOGM_MAPAUDIT_MAX_T 32
typedef struct SogmMapAuditParams {
  float   thr_test, thr_truth;   /* occupancy thresholds, one per side */
  int32_t tolerance;             /* r, 0 .. 3 cells */
  int32_t flags;                 /* SOGM_MAPAUDIT_FRUSTUM */
  int32_t box_lo[3], box_hi[3];  /* logical cells [lo, hi); all six zero: the whole grid */
  int32_t slab_layers;           /* 0: the layout chooses; otherwise an upper bound on the z layers a workgroup holds at a
                                    time.  The rows never depend on it. */
  int32_t reserved_;
  double  near_z, far_z;         /* frustum: finite, 0 <= near_z < far_z */
  double  tan_h, tan_v;          /* frustum: finite, > 0: the tangents of the half angles (0.5 * cols / fx, 0.5 * rows / fy) */
  int32_t slice_map[SOGM_MAPAUDIT_MAX_T];  /* truth slice of test slice t, or -1: skip it; entries at and beyond T_test are
                                              not read */
} SogmMapAuditParams;            /* 208 bytes */
typedef struct SogmMapAuditRow {
  int32_t n_region, n_test, n_truth, n_both, n_test_near, n_truth_near, truth_slice, status;
} SogmMapAuditRow;               /* 32 bytes */

/* thresholds 0, tolerance 0, no flags, the whole grid, slab_layers 0, frustum parameters 0, slice_map = the identity on
 * min(T_test, T_truth) slices and -1 beyond.  SOGM_ERR_INVALID_ARG for a null prm or a T outside 1 .. SOGM_MAPAUDIT_MAX_T. */
int sogm_map_audit_default_params(int T_test, int T_truth, SogmMapAuditParams *out_prm_host);
/*
 * Audits the two contexts' CURRENT maps.  The call joins an update flow still building either map on `stream`, then reads
 * the two grids, map centres and stamps; it writes nothing to either context, allocates nothing, and does not synchronise
 * with the host.  prm is a host record; dev cam_rot [n_agents * 9] fp64 (NULL without SOGM_MAPAUDIT_FRUSTUM), dev out
 * [n_agents][T_test], dev out_dt [n_agents] fp64 or NULL.
 * SOGM_ERR_INVALID_ARG (with sogm_last_error text; checked first, before anything is queued on the device): a null test,
 * truth, prm or out; tolerance outside 0 .. 3; SOGM_MAPAUDIT_FRUSTUM without cam_rot, or with near_z, far_z, tan_h or tan_v
 * not finite, near_z < 0, far_z <= near_z, tan_h <= 0 or tan_v <= 0; a box that is empty or leaves the grid (unless all six
 * are zero); a slice_map entry of a test slice below -1 or at or above T_truth; a T above SOGM_MAPAUDIT_MAX_T on either
 * side; contexts on different devices, with different n_agents, L, W, H or resolution bits; a grid of which not even one z
 * layer fits one compute unit's LDS (W * ceil(L / 64) * 8 bytes * (5 + 8 r), 3 with r = 0, above 159 KB).
 * SOGM_ERR_NO_DEVICE without a GPU (no context exists on such a host: it is what a call gets there once its pointers are
 * not null and prm's own fields have passed).  SOGM_ERR_STATE when either map has never been updated.
 */
int sogm_map_audit(sogm_ctx *test, sogm_ctx *truth, const SogmMapAuditParams *prm,
                   const double *cam_rot /* dev [n_agents*9] or NULL */,
                   SogmMapAuditRow *out /* dev [n_agents][T_test] */, double *out_dt /* dev [n_agents] or NULL */,
                   void *stream);

/* ------------------------------------------------------------------------------------------ */
/* view mask: the cells of an agent's map that its depth image says something about, as a region */
/*   for the map audit.  The build's OWN instrument, like "map audit", held by two readings        */
/*   (csrc/sogm_viewmask.hpp + csrc/sogm_viewmask.hip, and the numpy restatement                   */
/*   tests/view_mask_reference.py), bit for bit.                                                   */
/* ------------------------------------------------------------------------------------------ */
/*
 * Every logical cell (ix, iy, iz) of agent a gets ONE class from the agent's uint16 depth image ("depth camera": what
 * sogm_render_depth[_swarm] leaves on the device).  All arithmetic is fp64, in exactly this order, one IEEE operation at a
 * time, without contraction:
 *
 *   p_d = (((double)i_d + 0.5) * (double)resolution - (double)range_d) - off_d      d = 0, 1, 2
 *         ("map audit"'s cell centre; off = cam_offset[a], the camera centre minus the map centre.  cam_offset == NULL: the
 *         subtraction is not made at all — the camera sits at the map centre, as in "map audit")
 *   q_j = (R[0][j]*p_0 + R[1][j]*p_1) + R[2][j]*p_2                                  j = 0 (x), 1 (y), 2 (z);  R = cam_rot[a]
 *   SOGM_VIEW_OUTSIDE (0)   unless  q_z > near_z && q_z <= far_z && fabs(q_x) <= q_z*tan_h && fabs(q_y) <= q_z*tan_v
 *                           ("map audit"'s frustum test, comparison for comparison)
 *   uf = (q_x / q_z) * fx + cx;   vf = (q_y / q_z) * fy + cy
 *   u  = floor(uf + 0.5);         v  = floor(vf + 0.5)          (doubles.  The nearest pixel centre: pixel u of "depth camera"
 *                                                                looks along xc = (u - cx) / fx)
 *   SOGM_VIEW_OFFIMAGE (1)  unless  u >= 0 && u < cols && v >= 0 && v < rows        (a NaN fails, and lands here)
 *   d16 = depth[(a * rows + (int)v) * cols + (int)u]
 *   SOGM_VIEW_FREE (2)      if d16 == 0                         (no return within max_depth: the ray is free as far as far_z,
 *                                                                which is why far_z <= max_depth is required)
 *   z_hit = (double)d16 / depth_scale                           (the zq of "depth camera")
 *   SOGM_VIEW_FREE (2)      if q_z <  z_hit - band
 *   SOGM_VIEW_SURFACE (3)   else if q_z <= z_hit + band
 *   SOGM_VIEW_HIDDEN (4)    otherwise
 *
 * Known coarseness, on purpose: ONE pixel per cell.  A near cell covers many pixels and a silhouette can cut through it; the
 * class is that of the pixel nearest its centre's projection.  No footprint, no stencil.
 *
 * Mask.  out_mask is [n_agents][H][W][row_words] 64-bit words, row_words = ceil(L / 64); cell ix is bit ix % 64 of word
 * ix / 64 of its row; the spare bits of a row's last word are clear.  A cell's bit is set when bit `class` of prm->classes is
 * set.  This is the layout sogm_map_audit_masked reads.
 * Counts.  out_counts[a][c], c = 0 .. 4: the cells of class c (they sum to L*W*H);  [5]: the bits set in the agent's mask;
 * [6], [7]: zero.  Overwritten by every call, produced by integer adds only: bit-identical from run to run.
 */
enum { SOGM_VIEW_OUTSIDE = 0, SOGM_VIEW_OFFIMAGE = 1, SOGM_VIEW_FREE = 2, SOGM_VIEW_SURFACE = 3, SOGM_VIEW_HIDDEN = 4 };
enum {                            /* SogmViewParams.classes: bit c stands for class c */
  SOGM_VIEWBIT_OUTSIDE = 1, SOGM_VIEWBIT_OFFIMAGE = 2, SOGM_VIEWBIT_FREE = 4, SOGM_VIEWBIT_SURFACE = 8, SOGM_VIEWBIT_HIDDEN = 16,
  SOGM_VIEWBIT_ALL = 31
};
typedef struct SogmViewParams {
  double  fx, fy, cx, cy;        /* the camera's intrinsics */
  double  depth_scale;           /* > 0 */
  double  max_depth;             /* > 0: what a zero pixel speaks for */
  double  near_z, far_z;         /* 0 <= near_z < far_z <= max_depth */
  double  tan_h, tan_v;          /* > 0 */
  double  band;                  /* metres, >= 0: half the thickness of SURFACE along the optical axis */
  int32_t rows, cols;
  int32_t classes;               /* SOGM_VIEWBIT_*, not zero */
  int32_t reserved_;
} SogmViewParams;                /* 104 bytes */

/* The camera's intrinsics, depth_scale, max_depth, rows and cols; near_z = 0, far_z = max_depth, tan_h = 0.5 * cols / fx,
 * tan_v = 0.5 * rows / fy, band = 0, classes = FREE | SURFACE.  SOGM_ERR_INVALID_ARG for a null pointer. */
int sogm_view_default_params(const SogmDepthCamera *cam, SogmViewParams *out_prm_host);
/*
 * Classifies every cell of every agent of `map`'s grid.  The context supplies only the geometry (n_agents, L, W, H,
 * resolution): no map is read or written, and a map that has never been updated is fine.  Stream-ordered, allocates
 * nothing, does not synchronise with the host; depth, cam_rot and cam_offset are only read.
 * SOGM_ERR_INVALID_ARG (with sogm_last_error text; checked first, before anything is queued on the device): a null map, prm,
 * depth, cam_rot or out_mask; rows or cols < 1, or an image of more than 2^31 - 1 pixels; fx, fy, cx, cy, depth_scale,
 * max_depth, band, near_z, far_z, tan_h or tan_v not finite; fx, fy, depth_scale, max_depth, tan_h or tan_v <= 0;
 * near_z < 0; far_z <= near_z; far_z > max_depth; band < 0; classes zero or with a bit above class 4.
 * SOGM_ERR_NO_DEVICE without a GPU (what a call gets there once its pointers are not null and prm has passed).
 */
int sogm_view_mask(sogm_ctx *map, const SogmViewParams *prm, const uint16_t *depth /* dev [n*rows*cols] */,
                   const double *cam_rot /* dev [n*9] */, const double *cam_offset /* dev [n*3] or NULL */,
                   uint64_t *out_mask /* dev [n][H][W][row_words] */, int32_t *out_counts /* dev [n][8] or NULL */,
                   void *stream);
/*
 * sogm_map_audit on a given region: R = box && the cell's bit of `mask` (the layout above; e.g. sogm_view_mask's).
 * Everything else — occupancy, neighbourhood, counts, status, out_dt, refusals, SOGM_ERR_STATE — is sogm_map_audit's.
 * SOGM_MAPAUDIT_FRUSTUM must be clear: with it set the call is SOGM_ERR_INVALID_ARG; near_z, far_z, tan_h and tan_v are
 * not read.  A null mask is SOGM_ERR_INVALID_ARG.  Bits of `mask` beyond a row's L cells are ignored.
 */
int sogm_map_audit_masked(sogm_ctx *test, sogm_ctx *truth, const SogmMapAuditParams *prm,
                          const uint64_t *mask /* dev [n_agents][H][W][row_words] */,
                          SogmMapAuditRow *out /* dev [n_agents][T_test] */, double *out_dt /* dev [n_agents] or NULL */,
                          void *stream);

/* ------------------------------------------------------------------------------------------ */
/* velocity audit: the new-born list of a particle map's last update — what the on-device        */
/*   velocity estimation (sogm_update_dsp with labels == NULL) made of the cloud — scored point   */
/*   by point against truth labels ("ground-truth labels": out_labels and out_code of             */
/*   sogm_filter_point_cloud_labelled, in the same point order).  The build's OWN instrument,      */
/*   like "map audit", held by two readings (csrc/sogm_velaudit.hpp + csrc/sogm_velaudit.hip, and  */
/*   the numpy restatement tests/velocity_audit_reference.py), field for field.                    */
/* ------------------------------------------------------------------------------------------ */
/*
 * All arithmetic is fp32, in exactly this order, one IEEE operation at a time, without contraction.  Every output is an
 * integer and bit-identical from run to run.
 *
 * The list.  sogm_update_dsp leaves per agent the new-born list (rows {x, y, z, vx, vy, vz, intensity}, n_born of them) and,
 *   beside it, the SOURCE INDEX of every row: the index, inside the agent's range of the input cloud, of the point the row
 *   came from.  With labels given the list is the cloud in input order and the index is the identity; with labels == NULL the
 *   estimator reorders the list ([possibly-dynamic clusters][ground][static clusters]) and drops the points of rejected
 *   clusters, and the index says which is which.  (sogm_abi_debug.h: sogm_dsp_download_born_source.)
 * Per agent: n_in = min(cloud_range end - begin, max_points).  truth_labels[(begin + i)*4 ..] and truth_code[begin + i] belong
 *   to input point i, as `labels` do in sogm_update_dsp.
 * Estimate class of input point i — the tests the map itself applies to the list when it creates particles:
 *     DROPPED (3)     no born row names i
 *   and for the born row {.., vx, vy, vz, inten} that names it
 *     STATIC (0)      unless inten > 0.01f
 *     TRACKED (1)     if inten > 0.01f && vx > -100.f
 *     UNTRACKED (2)   otherwise (the -10000 label of a possibly-dynamic cluster without a match: the map gives its
 *                     particles a random velocity)
 * Truth class: MOVING (1) if truth_labels[i].intensity > 0.01f, else STILL (0).
 * Truth velocity: (tvx, tvy) = the label's (vx, vy) if MOVING, else (0, 0).  Only the HORIZONTAL components are scored: the
 *   map reads vx and vy of a label and nothing else.
 * Quantities of a TRACKED row:
 *     ex = vx - tvx;  ey = vy - tvy;  e2 = ex*ex + ey*ey
 *     s_e = vx*vx + vy*vy;  s_t = tvx*tvx + tvy*tvy;  dot = vx*tvx + vy*tvy;  m = s_e*s_t
 *   NaN: a TRACKED row whose e2 or m is NaN counts in the confusion matrix (and in its code's `tracked` column) and in
 *     n_nan, and nowhere else.  Every other TRACKED row is SCORED:
 *   speed bin = the number of T in {0.1f, 0.25f, 0.5f, 1.0f, 2.0f} with e2 > T*T                              (0 .. 5)
 *   direction bin (MOVING rows):  4 if s_e == 0 (an estimate faster than 5 m/s is zeroed, but matched);
 *     else 0 if dot > 0 && dot*dot >= 0.9330127f*m (within 15 degrees);  else 1 if dot > 0 && dot*dot >= 0.5f*m (within 45);
 *     else 2 if dot > 0;  else 3
 *   within = e2 <= tol*tol,  tol = speed_tolerance
 *   e2_um = (int64)(min(e2, 1.0e4f) * 1.0e6f), truncated toward zero
 * Output row per agent, SOGM_VELAUDIT_ROW = 32 int64:
 *     [0] n_in   [1] n_born   [2] status bits   [3] n_nan
 *     [4 .. 11]   confusion [truth: STILL, MOVING][estimate: STATIC, TRACKED, UNTRACKED, DROPPED]  (sums to n_in)
 *     [12 .. 17]  speed bins of the scored MOVING x TRACKED rows
 *     [18 .. 23]  speed bins of the scored STILL x TRACKED rows (spurious velocity)
 *     [24 .. 28]  direction bins of the scored MOVING x TRACKED rows
 *     [29] the sum of e2_um, [30] the number within, both over the scored MOVING x TRACKED rows   [31] 0
 * Status: SOGM_VELAUDIT_SKIPPED — the agent's last update was rejected or never ran, or its range is empty: every count is 0;
 *   SOGM_VELAUDIT_BAD_SOURCE — a born row whose source index is outside [0, n_in), or names a point a row with a smaller
 *   index names already: that row is ignored;  SOGM_VELAUDIT_CLIPPED — the range was longer than max_points.
 * Per-code table (optional; needs truth_code): int64 [n_agents][n_codes + 2][6], row r = {static, tracked, untracked, dropped,
 *   n_within, sum of e2_um}; input point i lands in row c = truth_code[begin + i] if 0 <= c < n_codes, in row n_codes if
 *   c == SOGM_HIT_GROUND, in row n_codes + 1 otherwise.  Here n_within and the sum cover EVERY scored row of the code, moving
 *   or still, against the truth velocity above: which obstacle or body the estimator sees, and which it loses.
 */
#define SOGM_VELAUDIT_ROW 32
enum { SOGM_VEL_STATIC = 0, SOGM_VEL_TRACKED = 1, SOGM_VEL_UNTRACKED = 2, SOGM_VEL_DROPPED = 3 };
enum { SOGM_VELAUDIT_SKIPPED = 1, SOGM_VELAUDIT_BAD_SOURCE = 2, SOGM_VELAUDIT_CLIPPED = 4 }; /* status bits */
enum { SOGM_VELAUDIT_ACCUMULATE = 1 };                                                       /* SogmVelAuditParams.flags */
typedef struct SogmVelAuditParams {
  float   speed_tolerance; /* m/s, finite, >= 0 */
  int32_t n_codes;         /* >= 0, n_codes + 2 <= 1024 */
  int32_t flags;           /* SOGM_VELAUDIT_ACCUMULATE or 0 */
  int32_t reserved_;
} SogmVelAuditParams;      /* 16 bytes */
/*
 * Scores every agent of `d` after a sogm_update_dsp on the same stream (cloud_range: the one that update was given).  Without
 * SOGM_VELAUDIT_ACCUMULATE the outputs are zeroed first and then written; with it every count is ADDED to what out_rows and
 * out_per_code hold and the status is ORed: a run over many frames needs one read-back.
 * Stream-ordered, allocates nothing, does not synchronise with the host, writes nothing to the handle.
 * SOGM_ERR_INVALID_ARG (with sogm_last_error text; checked first, before anything is queued on the device): a null d,
 * truth_labels, cloud_range, prm or out_rows; out_per_code without truth_code; n_codes < 0; n_codes + 2 > 1024 (the table of
 * an agent lives in 48 KB of LDS); speed_tolerance negative or not finite; an undefined flag.
 * SOGM_ERR_NO_DEVICE without a GPU (what a call gets there once its pointers are not null and prm has passed).
 */
int sogm_dsp_velocity_audit(sogm_dsp *d, const float *truth_labels /* dev [points*4] */,
                            const int32_t *truth_code /* dev [points] or NULL */, const int32_t *cloud_range /* dev [n*2] */,
                            const SogmVelAuditParams *prm, int64_t *out_rows /* dev [n][32] */,
                            int64_t *out_per_code /* dev [n][n_codes + 2][6] or NULL */, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* trajectory server: the 100 Hz position commands (with yaw) a vehicle consumes                  */
/*   (traj_server/src/bezier_traj_server.cpp, bezier_traj_server_rotors.cpp)                      */
/* ------------------------------------------------------------------------------------------ */
/*
 * Semantics (one definition: csrc/sogm_trajserver.hpp, compiled for the host and the device;
 * tests/golden/make_traj_server_fixture.py restates it in plain Python).  One server per agent: a state record and a ring
 * of queued samples.  Line numbers are bezier_traj_server.cpp's unless a file is named.
 *   - State after the preamble: odometry received, yaw initialised, triggered at t_trigger (main :527-529,
 *     triggerCallback :361-371): ts = te = t_trigger, duration = 0, last_yaw = init_yaw, last_yawdot = 0, traj_id = 0
 *     (:531), nothing received, empty queue.
 *   - Receiving a trajectory at `now` (bezierCallback :283-355): tns = time_start, duration = the sum of the piece
 *     durations in order (:293-299).
 *       te <= tns (:343): resetTrajQueue (:233-244): the queue is emptied; for (t = 0; t < replan_threshold; t += sample_dt)
 *         a sample at t is pushed (t is that ACCUMULATED sum).
 *       otherwise mergeTrajQueue (:246-277): int k = (now + replan_threshold - tns) / sample_dt, the truncated IEEE
 *         quotient (a quotient outside int's range counts as a k larger than the queue).  k < 0 or k > size (:248 compares
 *         the int with a size_t, so a negative k is "larger"): "next traj starts earlier than current buffer" — nothing
 *         is erased and for (i = 0; i < replan_threshold / sample_dt; i++) a sample at i * sample_dt + (now - tns) is
 *         pushed (:252-261).  Otherwise the last k samples are erased and samples at i * sample_dt, i < k, pushed
 *         (:264-276).
 *     Then traj = the record, ts = tns, te = ts + duration, traj_id += 1 (:351-354).  A sample pushed at trajectory time t
 *     carries the time ts + t with the ts of BEFORE that assignment (pushToTrajQueue :202).
 *   - The timer at `now` (PubCallback :415-485): nothing received or an empty queue publishes nothing (:452-462).  A
 *     queue of one sample is held: that sample with zero velocity and acceleration, yaw = last_yaw, yaw_dot = 0
 *     (:463-468).  Otherwise the front sample is popped and published, then fillTrajQueue (:211-228): tq = now +
 *     replan_threshold; nothing is pushed when tq < ts or when t = tq - ts > duration; otherwise a sample of the current
 *     trajectory at t.
 *   - Yaw.  yaw_mode 0 (the launched bezier_traj_server: the getYaw call of pushToTrajQueue is commented out, :201):
 *     every sample is pushed with yaw = yaw_dot = 0.  yaw_mode 1 (bezier_traj_server_rotors.cpp:212-223): getYaw
 *     (:79-140; rotors :77-140) runs at every push, in push order, on the sample's velocity, and updates last_yaw /
 *     last_yawdot.  PI = yaw_pi and YAW_DOT_MAX_PER_SEC = yaw_dot_max are parameters (3.14159265358979323846 and that
 *     same value per second, :35-36; 3.1415926 and 0.05, rotors :36, :78); MAX_YAW_CHANGE = yaw_dot_max * 0.01 and the
 *     literal 0.01 of yaw_dot = (yaw_temp - last_yaw) / 0.01 stay literals.  dir = v.normalized() is Eigen's: v / |v| when
 *     the squared norm is > 0, v itself otherwise, so dir.norm() > 0.1 fails exactly for a zero velocity (the hover
 *     records), where yaw_temp = last_yaw.  atan2 is sogm_det::atan2 (sogm_detmath.h): host, device and the Python
 *     reading agree bit for bit.
 *   - Times are built from integers as the audit builds them: tick k of a call has the stamp t_k = t0 + (first_tick + k) *
 *     period; the timer fires at t_k + j * sample_dt, j = 0 .. m - 1, m = period / sample_dt whole to 1e-9.  Tick k's
 *     record tables[k][a] is received at t_k + receive_delay (0 <= receive_delay < period), before the timer of the first
 *     instant that is not earlier.  It is received if received[k][i] != 0, or with received == NULL if its time_start
 *     differs from the previous table's record (tables[k - 1][a]; prev_table for k = 0) or that record has no pieces
 *     (or is absent) — in both cases only if it has n_pieces > 0.
 * Deviations, all stated here:
 *   - Evaluation outside [0, duration] (the "earlier" branch and a reset with replan_threshold > duration ask for it) is
 *     sogm_traj_eval's: t clamped to [0, duration].  Bezier::getPos (traj_utils/include/traj_utils/bernstein.hpp:164-177,
 *     src/bernstein.cpp:25-59) extrapolates the first piece's polynomial below 0 and the last piece's above the duration.
 *   - The ring holds SOGM_TRAJSRV_QUEUE samples; replan_threshold / sample_dt <= 127 (replan_threshold in (0, 1.27] at
 *     100 Hz; the launch files use 0.02, 0.3, 0.5, 1.2).  A push into a full ring is dropped (it does not run getYaw) and
 *     sets the sticky `overflow`; the reference's deque grows without bound when "earlier" arrivals repeat.
 *   - Sample times stay doubles (ros::Time::fromSec rounds to nanoseconds, :202); a flagged record without pieces is
 *     ignored (:307-311 would drop is_traj_received_).
 *   - Out of scope: the yaw-alignment preamble (is_init_yaw, :429-450), the tracking error (:399-408), the trigger topic
 *     and the visualiser.
 */
#define SOGM_TRAJSRV_QUEUE 256
typedef struct SogmTrajServerParams {
  double  replan_threshold;   /* seconds of trajectory kept queued, (0, 127 * sample_dt] */
  double  sample_dt;          /* DELTA_T, 0.01 */
  double  yaw_pi, yaw_dot_max;
  int32_t yaw_mode;           /* 0: yaw 0 is pushed; 1: getYaw at every push */
  int32_t reserved_;
} SogmTrajServerParams;       /* 40 bytes */
typedef struct SogmTrajPoint {   /* a queued sample */
  double t, pos[3], vel[3], acc[3], yaw, yaw_dot;
} SogmTrajPoint;              /* 96 bytes */
enum { SOGM_CMD_PUBLISHED = 1, SOGM_CMD_HELD = 2 };
typedef struct SogmPositionCommand {   /* quadrotor_msgs/PositionCommand as publishCmd fills it (:163-187) */
  double  t_pub, t_sample;    /* the timer instant (header.stamp); the popped sample's time */
  double  pos[3], vel[3], acc[3], yaw, yaw_dot;
  int32_t traj_id;
  int32_t flags;              /* SOGM_CMD_PUBLISHED (0: PubCallback returned without publishing: pos = init_pos, the rest
                                 0) | SOGM_CMD_HELD (the queue's last sample, held) */
} SogmPositionCommand;        /* 112 bytes */
typedef struct SogmTrajServerCore {   /* one server's scalars */
  double  ts, te, duration, last_yaw, last_yawdot, init_pos[3];
  int32_t head, size;         /* the queue: ring slots head, head + 1, ... (mod SOGM_TRAJSRV_QUEUE), `size` of them */
  int32_t traj_id, received, overflow, reserved_[3];
} SogmTrajServerCore;         /* 96 bytes */
typedef struct SogmTrajServerState {
  SogmTrajServerCore core;
  SogmTrajRecord     traj;    /* traj_: the trajectory fillTrajQueue samples */
} SogmTrajServerState;        /* 96 + 2064 bytes */

/*
 * The three entries are context-free and stateless like sogm_swarm_audit: the caller's buffers, the caller's stream, no
 * allocation, no host synchronisation.  SOGM_ERR_INVALID_ARG (with sogm_last_error text, checked first) for null pointers,
 * counts out of range (n_ticks 1 .. 64, n_total >= 1, 0 <= agent0, 1 <= n_local <= n_total - agent0, first_tick >= 0),
 * replan_threshold outside (0, 127 * sample_dt], period / sample_dt not whole (1 .. 4096), receive_delay outside
 * [0, period), yaw_mode not 0 or 1, times or yaw constants that are not finite.
 *
 * sogm_traj_server_init: dev state [n], dev queue [n][SOGM_TRAJSRV_QUEUE] (zeroed), dev init_pos [n][3], dev init_yaw [n]
 * or NULL (0).
 * sogm_traj_server_run: n_ticks ticks of agents [agent0, agent0 + n_local): dev state [n_local] in/out, dev queue
 * [n_local][SOGM_TRAJSRV_QUEUE] in/out, dev tables [n_ticks][n_total] (the executed tables the audit takes), dev prev_table
 * [n_total] or NULL, dev received int32 [n_ticks][n_local] or NULL, dev out_cmd [n_local][n_ticks * m].
 * sogm_camera_poses: commands cmd[i * cmd_stride], i < n (any command: an unpublished one stands at init_pos with yaw 0) ->
 * the layouts sogm_render_depth takes: out_rot[i] = Rz(yaw) * cam2body (row-major; Rz from sogm_det::cos / sogm_det::sin, each
 * entry (a * b + c * d) + e * f in column order), out_pos[i] = pos + Rz(yaw) * cam_offset.  cam2body [9] and cam_offset [3]
 * are HOST arrays.  scene.camera_pose is the host expression of the same convention.
 */
int sogm_traj_server_init(SogmTrajServerState *state, SogmTrajPoint *queue, int n, double t_trigger,
                          const double *init_pos /* dev [n][3] */, const double *init_yaw /* dev [n] or NULL */,
                          void *stream);
int sogm_traj_server_run(const SogmTrajServerParams *prm, SogmTrajServerState *state, SogmTrajPoint *queue,
                         const SogmTrajRecord *tables, const SogmTrajRecord *prev_table, const int32_t *received,
                         int n_ticks, int n_total, int agent0, int n_local, double t0, int first_tick, double period,
                         double receive_delay, SogmPositionCommand *out_cmd, void *stream);
int sogm_camera_poses(const SogmPositionCommand *cmd, int n, int cmd_stride, const double *cam2body /* host [9] */,
                      const double *cam_offset /* host [3] */, double *out_pos /* dev [n][3] */,
                      double *out_rot /* dev [n][9] */, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* radio links: every receiver's own table of the swarm's trajectories, under per-message delay,  */
/*   loss and radio range.  The reference is decentralised: each drone keeps a ParticleATC store  */
/*   of the BezierTraj messages that reached it (traj_coordinator/src/particles.cpp:131-191), the */
/*   callback logs each message's delay (:156-157) and whatever arrives last overwrites the entry */
/*   (:184-186).  The link model itself is the build's OWN definition, held by two independent    */
/*   implementations (csrc/sogm_link.hpp; tests/link_model_reference.py), bit for bit.            */
/* ------------------------------------------------------------------------------------------ */
/*
 * Draws are "sensor noise"'s: mix and U as defined there, counter-based, uint64 that wraps; fp64 is one IEEE operation at
 * a time without contraction.
 *
 * Messages.  At tick m sender j broadcasts row j of the table every agent executes after tick m, provided that row has
 *   n_pieces > 0; a row with n_pieces <= 0 is not a message.  Deviation: this happens EVERY tick whether or not the record
 *   changed (a heartbeat), where the reference sends only a new trajectory (plan_manager.cpp:364-399); the heartbeat only
 *   re-sends what a lossless link had already delivered.
 * Message (m, j -> a), a the receiver's global row, a != j:
 *   h = mix( mix( mix(seed) ^ m ) ^ (j * n_total + a) )                                   (all uint64)
 *   u = U(mix(h + 0))
 *   d = delay_min + min( (int)floor( U(mix(h + 1)) * (double)(delay_max - delay_min + 1) ), delay_max - delay_min )
 *   out of range, only when range > 0: with the positions of j and a at tick m, dx, dy, dz their differences,
 *     d2 = (dx*dx + dy*dy) + dz*dz; out of range iff !(d2 <= range*range) — a NaN position is out of range.
 *   lost iff out of range, else iff u < p_loss (the range test comes first).  A message that is not lost arrives at m + d.
 * Known answers: seed 0x5067, n_total 5, p_loss 0.3, delay 0..2: (m 0, j 0, a 1) h = 0xF556F0F326877456,
 *   u = 0x1.570a43181f084p-3, d 0, lost; (7, 4, 0) h = 0xECEED24989F9F5F8, u = 0x1.5e11450a71e6bp-1, d 1, not lost.
 *
 * Delivery at tick k — one call per tick, ticks consecutive from tick0:
 *   1. the table and the positions are stored in slot k % (delay_max + 1) of the caller's ring;
 *   2. for every (local receiver a, sender j != a): of the not-lost messages with tick0 <= m <= k and m + d == k the one
 *      with the largest m wins;
 *   3. with SOGM_LINK_NEWEST_WINS a winner with m < the send tick already held is dropped;
 *   4. otherwise it is copied into views[a_local][j] and held_tick[a_local][j] = m — without the flag an older message
 *      does overwrite a newer one, as `*obs_ptr = traj` does (particles.cpp:184-186);
 *   5. no arrival leaves the view unchanged;
 *   6. views[a_local][a], the receiver's own row, always gets the current row (held_tick = k).
 * counters[a_local][8] int64, added to by every call (integer adds: the same bits from run to run):
 *   0 messages of tick k addressed to the receiver   1 of those, out of range        2 of those, lost by draw
 *   3 arrivals at tick k                             4 arrivals applied (winners copied)
 *   5 winners older than what was held (applied, or dropped under the flag)
 *   6 sum over heard senders of k - held_tick after delivery                        7 senders not heard yet
 * All-zero parameters are perfect links: every view row equals the table's from the first tick on.
 */
#define SOGM_LINK_MAX_DELAY   7
#define SOGM_LINK_NEWEST_WINS 1
#define SOGM_LINK_COUNTERS    8
typedef struct SogmLinkParams {
  uint64_t seed;
  double   p_loss;        /* [0, 1] */
  double   range;         /* metres; 0: unlimited */
  int32_t  delay_min;     /* whole ticks, 0 <= delay_min <= delay_max <= SOGM_LINK_MAX_DELAY */
  int32_t  delay_max;
  int32_t  flags;         /* SOGM_LINK_NEWEST_WINS; other bits are ignored */
  int32_t  reserved_;
} SogmLinkParams;         /* 40 bytes */
typedef struct SogmLinkBuffers {   /* all the caller's, device memory, 16-byte aligned */
  SogmTrajRecord *ring_table;   /* [delay_max + 1][n_total] */
  double         *ring_pos;     /* [delay_max + 1][n_total][3]; may be NULL when range == 0 */
  SogmTrajRecord *views;        /* [n_local][n_total]: what sogm_*_views take */
  int32_t        *held_tick;    /* [n_local][n_total]: the send tick of the row held, -1: nothing heard */
  int64_t        *counters;     /* [n_local][SOGM_LINK_COUNTERS] */
} SogmLinkBuffers;              /* 40 bytes */
/*
 * Context-free, stream-ordered, no allocation, no host synchronisation, like sogm_depth_noise.  sogm_link_init zeroes the
 * ring, the views and the counters and sets every held tick to -1.  sogm_link_deliver is the delivery at `tick`: dev table
 * [n_total] and dev pos [n_total][3] fp64 (or NULL) are only read, and may be reused as soon as the call is queued.
 * SOGM_ERR_INVALID_ARG (checked first; sogm_last_error() names the rule): a null prm, buffers, table or buffer pointer
 * (ring_pos only with range > 0); pos == NULL with range > 0; p_loss outside [0, 1] or not finite; range negative or not
 * finite; delays outside 0 <= delay_min <= delay_max <= SOGM_LINK_MAX_DELAY; n_total < 1, agent0 < 0, n_local outside
 * 1 .. n_total - agent0; tick0 < 0 or tick < tick0; a record buffer that is not 16-byte aligned.  SOGM_ERR_NO_DEVICE
 * without a GPU.
 */
int sogm_link_default_params(SogmLinkParams *out);
int sogm_link_init(const SogmLinkParams *prm, int n_total, int n_local, const SogmLinkBuffers *buffers, void *stream);
int sogm_link_deliver(const SogmLinkParams *prm, int tick, int tick0, const SogmTrajRecord *table /* dev [n_total] */,
                      const double *pos /* dev [n_total][3] or NULL */, int n_total, int agent0, int n_local,
                      const SogmLinkBuffers *buffers, void *stream);
/*
 * The consumers of per-agent tables.  Each is its namesake without `_views` with the same arguments, except that the
 * records are dev views [n_agents][n_records] — SogmLinkBuffers.views of a model with n_local == the context's n_agents —
 * and agent a (the context's a-th) reads views[a * n_records + r] where the namesake reads records[r].  The namesakes'
 * results are unchanged; with every block of `views` equal to one table the results are the namesake's on that table, bit
 * for bit.  sogm_planner_set_swarm_views is honoured by both forms of sogm_replan (the dataflow replan's finishing wave and
 * the grouped path) and undone by sogm_planner_set_swarm; sogm_flight_run reads its own ring of tables as before, and
 * sogm_update_prestamped has no views form.
 */
int sogm_project_neighbours_views(sogm_ctx *ctx, const SogmTrajRecord *views, int n_records, const int32_t *ego_ids,
                                  void *stream);
int sogm_update_world_views(sogm_ctx *ctx, const SogmWorld *world, const float *poses, const double *stamps,
                            const SogmTrajRecord *views, int n_records, const int32_t *ego_ids, void *stream);
int sogm_safe_after_opt_views(sogm_planner *p, const double *cpts, const int32_t *npoly, const SogmTrajRecord *views,
                              int n_records, const int32_t *ego_ids, const double *t_now, int32_t *out_safe, void *stream);
int sogm_planner_set_swarm_views(sogm_planner *p, const SogmTrajRecord *views, int n_records, const int32_t *ego_ids,
                                 const double *t_now);

/* ------------------------------------------------------------------------------------------ */
/* message noise: what a sender broadcasts against what it flies.  The reference's authors run   */
/*   eval_helper/traj_noise_maker between /broadcast_traj and /noisy_broadcast_traj               */
/*   (plan_manager/launch/sim_fkpcp_8_case_{1,2}.launch:169-178: noise/seed, noise/loc/{x,y,z},   */
/*   noise/time_sync, noise/tracking) and point the planner at the noisy topic                    */
/*   (launch/simulator/noisy_drone_fake_perception.xml:39).  eval_helper is an absent submodule:  */
/*   only the parameters are known, so the rule is the build's OWN definition, held by two        */
/*   independent implementations (csrc/sogm_trajnoise.hpp; tests/traj_noise_reference.py), bit    */
/*   for bit.  Only traj_noise_maker's side: the per-drone noisy pose and odometry of noise_maker */
/*   (noisy_drone_fake_perception.xml:100-108) stay out of scope.                                 */
/* ------------------------------------------------------------------------------------------ */
/*
 * mix and N(h) are "sensor noise"'s noise_mix and noise_normal: N is the twelve-piece Irwin-Hall normal, a multiple of
 * 2^-16 with |N| <= 6.  All keys are uint64 and wrap.  Every fp64 expression is one IEEE operation, with no contraction.
 *
 *   key(tag, x, j) = mix( mix( mix( mix(seed) ^ tag ) ^ x ) ^ j ).  Component c draws N(key + 16*c).
 *   Localisation bias of sender j at send tick m: b[c] = sigma_loc[c] * N(key(1, e, j) + 16c), with
 *     e = loc_hold > 0 ? m / loc_hold : 0.
 *   Clock offset of sender j, constant over the run: tau = sigma_time * N(key(2, 0, j)).
 *   Tracking error of message (m, j): e[c] = sigma_track * N(key(3, m, j) + 16c).
 *   shift[c] = b[c] + e[c].
 *   Row j with n_pieces <= 0 is not a message.  It is copied unchanged and its out_shift is four zeros.
 *   Otherwise every coordinate c of the control points k < 5 * min(n_pieces, SOGM_MAX_PIECES) becomes cpts + shift[c], one
 *     add.  It is copied bit for bit when shift[c] == 0.0, so a -0.0 survives zero parameters.
 *   Control points beyond those, drone_id, n_pieces and duration[] are copied.
 *   time_start becomes time_start + tau, and is copied when tau == 0.0.
 *   The same noisy message reaches every receiver, since one node republishes it in the reference.
 *   A receiver's own row in its view is therefore noisy too.  That is harmless: the overlay and both forms of
 *     isSafeAfterOpt skip it by drone_id.
 * Known answers, seed 0x5067:
 *   key(1, 0, 0) = 0x4ACD8EB1A9CFDCC6   N at c = 0, 1, 2: 0x1.469p-2, -0x1.c25p-4, -0x1.a0b6p-1
 *   key(2, 0, 3) = 0xF86E1BF400FF8055   N = -0x1.1598p-1
 *   key(3, 7, 4) = 0x0E12DE2E62B1FC89   N at c = 0, 1, 2: 0x1.d6dep-1, -0x1.34dep+0, 0x1.8a64p-1
 *
 * Context-free, stream-ordered, no allocation, no host synchronisation, like sogm_link_deliver.  `tick` is the send tick m
 * of every row; `out` may be `table` itself (in place) and must not overlap it otherwise.  out_shift (or NULL) receives
 * every row's shift x, y, z and tau.  SOGM_ERR_INVALID_ARG (checked before a device is looked for; sogm_last_error() names
 * the rule): a null prm, table or out; a sigma that is negative or not finite; loc_hold < 0; tick < 0; n_total < 1; a record
 * buffer that is not 16-byte aligned.  SOGM_ERR_NO_DEVICE without a GPU.
 */
typedef struct SogmTrajNoise {
  uint64_t seed;
  double   sigma_loc[3];   /* metres, per axis: the sender's localisation bias */
  double   sigma_time;     /* seconds: the sender's clock offset */
  double   sigma_track;    /* metres, all three axes: tracking error, new with every message */
  int32_t  loc_hold;       /* ticks a localisation bias lasts; 0: the whole run */
  int32_t  reserved_;
} SogmTrajNoise;           /* 56 bytes */

int sogm_traj_noise_default_params(SogmTrajNoise *out);   /* all zero: out == table, byte for byte */
int sogm_traj_noise(const SogmTrajNoise *prm, int tick, const SogmTrajRecord *table /* dev [n_total] */, int n_total,
                    SogmTrajRecord *out /* dev [n_total]; may be table */,
                    double *out_shift /* dev [n_total][4] = shift x, y, z, tau; or NULL */, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* belief audit: what each receiver believes about its neighbours' trajectories (its view,       */
/*   SogmLinkBuffers.views) against what the senders intend (the table they execute).  Like the  */
/*   link model and the message noise it is the build's own definition, held by                  */
/*   csrc/sogm_belief.hpp and tests/belief_audit_reference.py, count for count.                  */
/* ------------------------------------------------------------------------------------------ */
/*
 * For receiver row a = agent0 + a_local and sender row j != a, with T = truth[j] and B = views[a_local][j]:
 *   Both rows empty (n_pieces <= 0): nothing is counted.
 *   T has a trajectory and B has none: unheard (+1).   B has one and T has none: phantom (+1).
 *   Otherwise the pair is compared.  For s = 0 .. n_samples - 1:
 *     t = t_now[a_local] + (double)s * dt_sample.
 *     pT and pB are the positions of T and B at t: sogm_traj_eval's arithmetic (Bezier::getPos), t clamped to the
 *       record's span [time_start, time_start + total]; a record's n_pieces above SOGM_MAX_PIECES counts as
 *       SOGM_MAX_PIECES.
 *     d2 = (dx*dx + dy*dy) + dz*dz.  There is no square root: bins compare d2 <= edges[i] * edges[i].
 *     The sample goes to the first bin that holds it, else to bin 5.  A NaN goes to bin 5.
 *     q = min((int64)floor(d2 * 1e6 + 0.5), 2^40), the squared error in mm^2, clamped.  It is 2^40 for a NaN.
 * counters[a_local][12] int64, the caller zeroes them once and every call adds (integer adds and maxima: the same bits from
 * run to run):
 *   0 compared pairs   1 unheard   2 phantom   3 samples   4 .. 9 the six bins   10 sum of q   11 max q (an integer max)
 * out_pair_q[a_local][j] (or NULL) is the pair's largest q of this call, -1 when the pair is not compared or j == a.
 * Nothing is written to truth or views.
 *
 * Context-free, stream-ordered, no allocation, no host synchronisation.  SOGM_ERR_INVALID_ARG (checked first): a null prm,
 * truth, views, t_now or counters; n_samples outside 1 .. SOGM_BELIEF_MAX_SAMPLES; dt_sample not positive or not finite;
 * edges not strictly ascending, not positive or not finite; n_total < 1, agent0 < 0, n_local outside 1 .. n_total - agent0;
 * a record buffer that is not 16-byte aligned; n_local > 65535.  SOGM_ERR_NO_DEVICE without a GPU.
 */
#define SOGM_BELIEF_COUNTERS    12
#define SOGM_BELIEF_MAX_SAMPLES 16
typedef struct SogmBeliefParams {
  double  dt_sample;     /* seconds between samples (> 0) */
  double  edges[5];      /* metres, strictly ascending, > 0; default 0.05 0.1 0.2 0.5 1.0 */
  int32_t n_samples;     /* 1 .. 16; default 8, dt_sample 0.2 */
  int32_t reserved_;
} SogmBeliefParams;      /* 56 bytes */

int sogm_belief_default_params(SogmBeliefParams *out);
int sogm_belief_audit(const SogmBeliefParams *prm, const SogmTrajRecord *truth /* dev [n_total]: the table the agents execute */,
                      const SogmTrajRecord *views /* dev [n_local][n_total] */, const double *t_now /* dev [n_local] */,
                      int n_total, int agent0, int n_local, int64_t *counters /* dev [n_local][12] */,
                      int64_t *out_pair_q /* dev [n_local][n_total] or NULL */, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* trajectory exchange: the /broadcast_traj topic as ONE RCCL all-gather per replan tick          */
/*   (plan_manager/src/plan_manager.cpp:364-399 publish, traj_coordinator/src/particles.cpp:131-191 receive)  */
/* ------------------------------------------------------------------------------------------ */
/*
 * Agents are sharded over the GPUs of a node, one process per GPU; rank r owns a contiguous block of agents.
 * After sogm_replan() (and the caller's latest-wins merge) every rank contributes the SogmTrajRecord of each of
 * its n_local agents and receives the whole swarm's: all_records[r * n_local + i] = rank r's local_records[i].
 * `nccl_comm` is an ncclComm_t (RCCL; <rccl/rccl.h>) whose ranks all call this with the same n_local.  RCCL is
 * resolved with dlopen("librccl.so.1") the first time it is needed, so a host that already links RCCL (or runs
 * PyTorch-ROCm) shares its instance and may pass a communicator of its own; sogm_comm_* creates one for hosts
 * that do not have RCCL headers.
 * The collective runs on an internal exchange stream: it starts when the work queued on `stream` so far is done
 * and sogm_project_neighbours / sogm_replan (deconfliction) / sogm_safe_after_opt wait for it on their own stream,
 * so the next tick's clear, stamp and trajectory sampling overlap with it.  A host that reads all_records by other
 * means calls sogm_exchange_wait(ctx, its_stream) first.
 * dev local_records [n_local], dev all_records [n_local * n_ranks].
 */
int sogm_traj_allgather(sogm_ctx *ctx, void *nccl_comm, const SogmTrajRecord *local_records, int n_local,
                        SogmTrajRecord *all_records, void *stream);
int sogm_exchange_wait(sogm_ctx *ctx, void *stream);

/* Communicator helpers (thin wrappers of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy).  Rank 0 makes
 * an id and ships its 128 bytes to the other ranks by any out-of-band means (torch.distributed's store, MPI, a
 * file); every rank then calls sogm_comm_create.  sogm_comm_handle returns the ncclComm_t to pass above. */
#define SOGM_COMM_ID_BYTES 128
typedef struct sogm_comm sogm_comm;
int   sogm_comm_unique_id(char *out_id_host /* [SOGM_COMM_ID_BYTES] */);
int   sogm_comm_create(const char *id_host, int rank, int n_ranks, int device, sogm_comm **out);
void  sogm_comm_destroy(sogm_comm *comm);
void *sogm_comm_handle(sogm_comm *comm);
/* what RCCL itself says about the communicator: host out[2] = {ncclCommCount, ncclCommUserRank} (a multi-GPU bench line
 * reports them: a run that silently fell back to fewer ranks cannot print the requested N) */
int   sogm_comm_info(sogm_comm *comm, int32_t *out_host);

#ifdef __cplusplus
}
#endif
#endif /* SOGM_ABI_H */
