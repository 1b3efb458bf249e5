// sogm_facade.hpp — host C++ facade that keeps the reference's class surface and forwards to the
// C ABI (include/sogm_abi.h).  Header-only, C++17, no Eigen / ROS: vectors are std::array<double,3>
// (an Eigen::Vector3d's storage is layout-compatible: pass v.data()).
//
// One facade object is a VIEW of one agent inside a batched context, so that a plan_manager-style
// caller written against
//     map_->getClearOcccupancy(pos, t) / getObstaclePoints(...)      (risk_base.h:84-105)
//     a_star_->search(...) / getPathWithVel(dt)                      (risk_hybrid_a_star.h:96-121)
//     firi::firi(...)                                                (sfc_gen/firi.hpp:238)
//     traj_optimizer_->setup(...) / optimize() / getOptBezier(...)   (bezier_optimizer.hpp:57-88)
// links against this instead (plan_manager/include/plan_manager/baseline.h:155-158 holds exactly
// these four pointers).  The batched entry points are what a multi-agent service calls directly;
// the per-agent methods below stage one agent's arguments through small device buffers and are
// meant for drop-in use and testing, not for throughput.
#pragma once

#include <hip/hip_runtime_api.h>

#include <array>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sogm_abi.h"

namespace sogm_host {

using Vec3 = std::array<double, 3>;
using State6 = std::array<double, 6>;

inline void check(int rc, const char *what) {
  if (rc != SOGM_OK)
    throw std::runtime_error(std::string(what) + " failed: " + std::to_string(rc) + " " + sogm_last_error());
}

// The library must implement the header this host was compiled against: buffer sizes of existing entry points have
// changed between versions (sogm_abi.h, SOGM_ABI_VERSION).  Every facade object checks once at construction.
inline void check_abi() {
  static const int got = sogm_abi_version();
  if (got != SOGM_ABI_VERSION)
    throw std::runtime_error("libsogm_hip.so implements ABI version " + std::to_string(got) + ", this host was built against " +
                             std::to_string(SOGM_ABI_VERSION));
}

template <typename T>
class DevBuf {  // tiny RAII device buffer
 public:
  explicit DevBuf(size_t n = 0) { resize(n); }
  ~DevBuf() { if (p_) (void)hipFree(p_); }
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  void resize(size_t n) {
    if (n <= n_) return;
    if (p_) (void)hipFree(p_);
    if (hipMalloc((void **)&p_, n * sizeof(T)) != hipSuccess) throw std::bad_alloc();
    n_ = n;
  }
  void put(const T *h, size_t n) { resize(n); (void)hipMemcpy(p_, h, n * sizeof(T), hipMemcpyHostToDevice); }
  void get(T *h, size_t n) const { (void)hipMemcpy(h, p_, n * sizeof(T), hipMemcpyDeviceToHost); }
  T *data() { return p_; }

 private:
  T     *p_ = nullptr;
  size_t n_ = 0;
};

// ---- wire formats -----------------------------------------------------------------------
// traj_utils/msg/BezierTraj.msg:1-9 as filled by FiniteStateMachine::publishTrajectory
// (plan_manager/src/plan_manager.cpp:364-399) and read by ParticleATC::trajectoryCallback
// (traj_coordinator/src/particles.cpp:131-191): float32 durations, geometry_msgs/Point control points.
struct BezierTrajMsg {
  int32_t             drone_id = 0, traj_id = 0;
  double              start_time = 0.0, pub_time = 0.0;  // ros::Time::toSec()
  uint8_t             order = 4;
  std::vector<float>  duration;
  std::vector<Vec3>   cpts;
};
// message -> fixed-size record (the all-gather payload).  Returns false when the message does not fit
// (more than SOGM_MAX_PIECES pieces, order != 4 or an inconsistent control-point count).
inline bool recordFromMsg(const BezierTrajMsg &m, SogmTrajRecord &r) {
  const size_t n = m.duration.size();
  if (m.order != 4 || n > SOGM_MAX_PIECES || m.cpts.size() != 5 * n) return false;
  r = SogmTrajRecord{};
  r.drone_id   = m.drone_id;
  r.n_pieces   = (int32_t)n;
  r.time_start = m.start_time;
  for (size_t i = 0; i < n; ++i) r.duration[i] = (double)m.duration[i];  // float32 on the wire
  for (size_t k = 0; k < 5 * n; ++k)
    for (int d = 0; d < 3; ++d) r.cpts[k * 3 + d] = m.cpts[k][d];
  return true;
}
inline BezierTrajMsg msgFromRecord(const SogmTrajRecord &r, int32_t traj_id, double pub_time) {
  BezierTrajMsg m;
  m.drone_id   = r.drone_id;
  m.traj_id    = traj_id;
  m.start_time = r.time_start;
  m.pub_time   = pub_time;
  m.order      = 4;
  for (int i = 0; i < r.n_pieces; ++i) m.duration.push_back((float)r.duration[i]);
  for (int k = 0; k < 5 * r.n_pieces; ++k) m.cpts.push_back({r.cpts[k * 3], r.cpts[k * 3 + 1], r.cpts[k * 3 + 2]});
  return m;
}
// map/future_risk std_msgs/Float32MultiArray (plan_env/src/risk_mapping_node.cpp:129-145, consumer
// risk_base.cpp:60-75): data = [V * stride risk values | pose x, y, z | stamp], layout.dim[0].stride = T.
// Splits one message into the arguments of sogm_set_future_risk (host side; grid returned voxel-major [V][T]).
inline bool splitFutureRiskMsg(const std::vector<float> &data, int V, int T, int stride, std::vector<float> &grid_vt,
                               float pose[3], double &stamp) {
  if (stride < T || data.size() < (size_t)V * stride + 4) return false;
  grid_vt.resize((size_t)V * T);
  for (int i = 0; i < V; ++i)
    for (int j = 0; j < T; ++j) grid_vt[(size_t)i * T + j] = data[(size_t)i * stride + j];
  // pose and time follow the V * PREDICTION_TIMES block (risk_base.cpp:72 reads index V*T + 3)
  const size_t o = (size_t)V * T;
  pose[0] = data[o];
  pose[1] = data[o + 1];
  pose[2] = data[o + 2];
  stamp   = (double)data[o + 3];  // float32 seconds on the wire
  return true;
}
inline std::vector<float> futureRiskMsg(const std::vector<float> &grid_vt, const float pose[3], double stamp) {
  std::vector<float> d(grid_vt);
  d.push_back(pose[0]);
  d.push_back(pose[1]);
  d.push_back(pose[2]);
  d.push_back((float)stamp);
  return d;
}

// ---- RiskMap / SOGM : RiskBase + FakeParticleRiskVoxel surface --------------------------------------
class RiskMap {
 public:
  RiskMap(const SogmSpec &spec, int n_agents, int device = 0) : n_(n_agents), spec_(spec) {
    check_abi();
    check(sogm_create(&spec, n_agents, device, &ctx_), "sogm_create");
  }
  ~RiskMap() { sogm_destroy(ctx_); }
  sogm_ctx *ctx() { return ctx_; }
  int       agents() const { return n_; }

  // ParticleATC::initEgoParticles + setCoordinator (risk_base.h:62-65)
  // (pass the particles as ANOTHER drone's ParticleATC holds them: particlesCallback reads Point32 coordinates —
  //  (double)(float)x — particles.cpp:89-108; the library uses what it is given)
  void setCoordinator(const std::vector<Vec3> &body_particles) {
    check(sogm_set_body_particles(ctx_, body_particles[0].data(), (int)body_particles.size()), "set_body");
  }
  // Tick pipelining (no reference counterpart): 0 off, 1 in-place reset after the replan's last map reader, 2 / 3 a pool of
  // two / three grids (returns false and leaves the mode unchanged if HBM has no room for them)
  bool setTickPipelining(int mode) {
    const int rc = sogm_set_overlap_clear(ctx_, mode);
    if (rc == SOGM_ERR_CAPACITY) return false;
    check(rc, "sogm_set_overlap_clear");
    return true;
  }
  // How updateMap's "fill the map with zeros" (fake_particle_risk_voxel.cpp:107-108) is carried out: by zeroing the
  // logged sectors of the previous build's marks (default) or by the dense clear; same cells either way
  // swarm/replan_risk_rate, swarm/num_resample (particles.cpp:33-34) and the injected standard-normal table that
  // stands in for getParticlesWithRisk's time(NULL)-seeded generator (sogm_set_resample); rate 0 = off (the default)
  void setResample(float replan_risk_rate, int num_resample, const float *normal_table_dev, int n_table) {
    check(sogm_set_resample(ctx_, replan_risk_rate, num_resample, normal_table_dev, n_table), "sogm_set_resample");
  }
#ifdef SOGM_ABI_DEBUG_H
  // a tuning knob of this context (include/sogm_abi_debug.h "Tuning knobs"; there when that header was included first)
  void setTuning(const char *key, double value) { check(sogm_set_tuning(ctx_, key, value), "sogm_set_tuning"); }
#endif
  void setSparseReset(bool on, int log_capacity_per_agent = 0) {
    check(sogm_set_sparse_reset(ctx_, on ? 1 : 0, log_capacity_per_agent), "sogm_set_sparse_reset");
  }
  // SOGM::update — FakeParticleRiskVoxel::updateMap for the whole batch (device pointers)
  void update(const float *cloud_xyz, const int32_t *cloud_range, const SogmCylinder *cyl, int n_cyl,
              const float *poses, const double *stamps, hipStream_t st = nullptr) {
    check(sogm_update_gt(ctx_, cloud_xyz, cloud_range, cyl, n_cyl, poses, stamps, st), "sogm_update_gt");
  }
  // FakeParticleRiskVoxel::updateMap including its closing neighbour overlay (fake_particle_risk_voxel.cpp:175-226)
  void updateWithSwarm(const float *cloud_xyz, const int32_t *cloud_range, const SogmCylinder *cyl, int n_cyl,
                       const float *poses, const double *stamps, const SogmTrajRecord *records, int n_records,
                       const int32_t *ego_ids, hipStream_t st = nullptr) {
    check(sogm_update_gt_swarm(ctx_, cloud_xyz, cloud_range, cyl, n_cyl, poses, stamps, records, n_records, ego_ids, st),
          "sogm_update_gt_swarm");
  }
  // updateMap from one sensor frame (MapBase::cloudCallback -> updateMap with the states groundTruthStateCallback
  // delivered, map.cpp:170-171, fake_particle_risk_voxel.cpp:244-264): the PassThrough crop (:88-104) runs on the device
  // around each agent's map centre.  `bounds`: xy bounds of the cloud's blocks of `block_points` points — blockBounds()
  // computes them on the device, once per frame.  records = nullptr: no overlay.
  static void blockBounds(const float *cloud_xyz, int n_points, int block_points, float *bounds, hipStream_t st = nullptr) {
    check(sogm_cloud_block_bounds(cloud_xyz, n_points, block_points, bounds, st), "sogm_cloud_block_bounds");
  }
  static SogmWorld world(const float *cloud_xyz, int n_points, const float *bounds, int block_points,
                         const SogmCylinder *cyl, int n_cyl) {
    return SogmWorld{cloud_xyz, bounds, cyl, n_points, (n_points + block_points - 1) / block_points, block_points, n_cyl};
  }
  // The frames of ticks first_tick .. first_tick + n_ticks - 1 of a moving world, written on the device from its tick-0
  // state (include/sogm_abi.h "world timeline"): frames[i]'s cloud, block bounds and records are OUTPUTS here.
  static void worldFrames(const SogmWorldTimeline &tl, int first_tick, int n_ticks, const SogmWorld *frames,
                          hipStream_t st = nullptr) {
    check(sogm_world_frames(&tl, first_tick, n_ticks, frames, st), "sogm_world_frames");
  }
  void updateWorld(const SogmWorld &frame, const float *poses, const double *stamps, const SogmTrajRecord *records = nullptr,
                   int n_records = 0, const int32_t *ego_ids = nullptr, hipStream_t st = nullptr) {
    check(sogm_update_world(ctx_, &frame, poses, stamps, records, n_records, ego_ids, st), "sogm_update_world");
  }
  // updateWorld whose closing overlay reads every agent's OWN table: dev views [n_agents][n_records] (Links::views())
  void updateWorldViews(const SogmWorld &frame, const float *poses, const double *stamps, const SogmTrajRecord *views,
                        int n_records, const int32_t *ego_ids, hipStream_t st = nullptr) {
    check(sogm_update_world_views(ctx_, &frame, poses, stamps, views, n_records, ego_ids, st), "sogm_update_world_views");
  }
  // The update of a tick whose map the previous replan pre-stamped (Planner::setPrestamp): grid swap + overlay
  bool prestampPending() const { return sogm_prestamp_pending(ctx_) != 0; }
  void prestampJoin(void *stream = nullptr) { check(sogm_prestamp_join(ctx_, stream), "sogm_prestamp_join"); }
  void updatePrestamped(const SogmTrajRecord *records, int n_records, const int32_t *ego_ids, hipStream_t st = nullptr) {
    check(sogm_update_prestamped(ctx_, records, n_records, ego_ids, st), "sogm_update_prestamped");
  }
  // RiskBase::futureRiskCallback for agent 0 of a 1-agent context: adopt one map/future_risk message.
  // `map_time` is the map stamp to adopt (the ROS header / receive time as a double).  The reference reads the
  // message's trailing float32 field into a dead local (risk_base.cpp:72) and leaves last_update_time_ alone; a
  // float32 epoch time is quantised to ~128 s, so it is only used when no map_time is given (NaN).
  void futureRiskCallback(const std::vector<float> &msg_data, int stride, hipStream_t st = nullptr,
                          double map_time = std::numeric_limits<double>::quiet_NaN()) {
    const SogmSpec sp = spec_;
    const int      V  = sp.L * sp.W * sp.H;
    std::vector<float> grid;
    float  pose[3];
    double stamp = 0.0;
    if (n_ != 1 || !splitFutureRiskMsg(msg_data, V, sp.T, stride, grid, pose, stamp))
      throw std::runtime_error("futureRiskCallback: malformed message");
    if (map_time == map_time) stamp = map_time;
    g_.put(grid.data(), grid.size());
    f_.put(pose, 3);
    t_.put(&stamp, 1);
    check(sogm_set_future_risk(ctx_, g_.data(), f_.data(), t_.data(), st), "sogm_set_future_risk");
  }
  // RiskBase::addOtherAgents
  void addOtherAgents(const SogmTrajRecord *records, int n, const int32_t *ego_ids, hipStream_t st = nullptr) {
    check(sogm_project_neighbours(ctx_, records, n, ego_ids, st), "sogm_project_neighbours");
  }
  // addOtherAgents from every agent's OWN ParticleATC store: dev views [n_agents][n] (Links::views())
  void addOtherAgentsViews(const SogmTrajRecord *views, int n, const int32_t *ego_ids, hipStream_t st = nullptr) {
    check(sogm_project_neighbours_views(ctx_, views, n, ego_ids, st), "sogm_project_neighbours_views");
  }
  // int getClearOcccupancy(const Vector3d& pos, double dt) const  -> 0 free / 1 occupied / -1 out
  int getClearOcccupancy(int agent, const Vec3 &pos, double dt) {
    int32_t a = agent; int8_t r = 0;
    a_.put(&a, 1); p_.put(pos.data(), 3); t_.put(&dt, 1); o_.resize(1);
    check(sogm_query_clear(ctx_, a_.data(), p_.data(), t_.data(), 0, 1, o_.data(), nullptr), "sogm_query_clear");
    o_.get(&r, 1);
    return r;
  }
  int getClearOcccupancy(int agent, const Vec3 &pos, int t_index) {
    int32_t a = agent; int8_t r = 0; double t = t_index;
    a_.put(&a, 1); p_.put(pos.data(), 3); t_.put(&t, 1); o_.resize(1);
    check(sogm_query_clear(ctx_, a_.data(), p_.data(), t_.data(), 1, 1, o_.data(), nullptr), "sogm_query_clear");
    o_.get(&r, 1);
    return r;
  }
  // void getObstaclePoints(std::vector<Vector3d>&, double t0, double t1, const Vector3d& lc, const Vector3d& hc)
  void getObstaclePoints(int agent, std::vector<Vec3> &points, double t0, double t1, const Vec3 &lc,
                         const Vec3 &hc, int cap = 4096) {
    int32_t a = agent, n = 0;
    a_.put(&a, 1); p_.put(lc.data(), 3); q_.put(hc.data(), 3); t_.put(&t0, 1); u_.put(&t1, 1);
    pts_.resize((size_t)cap * 3); cnt_.resize(1);
    check(sogm_obstacle_points(ctx_, a_.data(), p_.data(), q_.data(), t_.data(), u_.data(), 1, pts_.data(),
                               cnt_.data(), cap, nullptr), "sogm_obstacle_points");
    cnt_.get(&n, 1);
    if (n > cap) n = cap;
    std::vector<double> h((size_t)n * 3);
    pts_.get(h.data(), h.size());
    for (int i = 0; i < n; ++i) points.push_back({h[i * 3], h[i * 3 + 1], h[i * 3 + 2]});
  }
  // Map audit (include/sogm_abi.h "map audit"; no reference counterpart): this map — the perceived one — against `truth`,
  // agent by agent and slice by slice.  auditParams() is sogm_map_audit_default_params for the two maps with each spec's
  // risk_threshold as the occupancy thresholds; the caller sets tolerance, box, frustum and slice_map on it.  cam_rot_host:
  // [agents * 9] row-major camera-to-world rotations, needed with SOGM_MAPAUDIT_FRUSTUM only.  Returns the rows
  // [agents][T of this map]; out_dt_host (agents values, optional): this map's stamp minus truth's.  Synchronises `st`.
  SogmMapAuditParams auditParams(const RiskMap &truth) const {
    SogmMapAuditParams prm;
    check(sogm_map_audit_default_params(spec_.T, truth.spec_.T, &prm), "sogm_map_audit_default_params");
    prm.thr_test  = spec_.risk_threshold;
    prm.thr_truth = truth.spec_.risk_threshold;
    return prm;
  }
  std::vector<SogmMapAuditRow> auditAgainst(RiskMap &truth, const SogmMapAuditParams &prm, const double *cam_rot_host = nullptr,
                                            double *out_dt_host = nullptr, hipStream_t st = nullptr) {
    const size_t rows = (size_t)n_ * (size_t)spec_.T;
    audit_rows_.resize(rows);
    u_.resize((size_t)n_);
    if (cam_rot_host) pts_.put(cam_rot_host, (size_t)n_ * 9);
    check(sogm_map_audit(ctx_, truth.ctx_, &prm, cam_rot_host ? pts_.data() : nullptr, audit_rows_.data(), u_.data(), st),
          "sogm_map_audit");
    if (hipStreamSynchronize(st) != hipSuccess) throw std::runtime_error("auditAgainst: hipStreamSynchronize failed");
    std::vector<SogmMapAuditRow> out(rows);
    audit_rows_.get(out.data(), rows);
    if (out_dt_host) u_.get(out_dt_host, (size_t)n_);
    return out;
  }
  // View mask (include/sogm_abi.h "view mask"; no reference counterpart): the cells of every agent's grid that its depth
  // image speaks for.  viewParams() is sogm_view_default_params of the camera the images were rendered with; the caller sets
  // band, classes and the frustum on it.  depth_dev: device [agents * rows * cols] (GridMap::renderDepth's); cam_rot_host
  // [agents * 9]; cam_offset_host [agents * 3], camera centre minus map centre, or nullptr (the camera at the map centre);
  // mask_dev: device [viewMaskWords()] 64-bit words, what auditAgainstMasked reads.  Only this map's geometry is used.
  // Returns the counts [agents][8] (five classes, the mask's bits, two zeros).  Synchronises `st`.
  static SogmViewParams viewParams(const SogmDepthCamera &cam) {
    SogmViewParams prm;
    check(sogm_view_default_params(&cam, &prm), "sogm_view_default_params");
    return prm;
  }
  size_t viewMaskWords() const { return (size_t)n_ * (size_t)spec_.H * (size_t)spec_.W * (size_t)((spec_.L + 63) / 64); }
  std::vector<int32_t> viewMask(const SogmViewParams &prm, const uint16_t *depth_dev, const double *cam_rot_host,
                                const double *cam_offset_host, uint64_t *mask_dev, hipStream_t st = nullptr) {
    pts_.put(cam_rot_host, (size_t)n_ * 9);
    if (cam_offset_host) q_.put(cam_offset_host, (size_t)n_ * 3);
    a_.resize((size_t)n_ * 8);
    check(sogm_view_mask(ctx_, &prm, depth_dev, pts_.data(), cam_offset_host ? q_.data() : nullptr, mask_dev, a_.data(), st),
          "sogm_view_mask");
    if (hipStreamSynchronize(st) != hipSuccess) throw std::runtime_error("viewMask: hipStreamSynchronize failed");
    std::vector<int32_t> counts((size_t)n_ * 8);
    a_.get(counts.data(), counts.size());
    return counts;
  }
  // auditAgainst with the region given as a mask (sogm_map_audit_masked): prm without SOGM_MAPAUDIT_FRUSTUM; the box still cuts.
  std::vector<SogmMapAuditRow> auditAgainstMasked(RiskMap &truth, const SogmMapAuditParams &prm, const uint64_t *mask_dev,
                                                  double *out_dt_host = nullptr, hipStream_t st = nullptr) {
    const size_t rows = (size_t)n_ * (size_t)spec_.T;
    audit_rows_.resize(rows);
    u_.resize((size_t)n_);
    check(sogm_map_audit_masked(ctx_, truth.ctx_, &prm, mask_dev, audit_rows_.data(), u_.data(), st), "sogm_map_audit_masked");
    if (hipStreamSynchronize(st) != hipSuccess) throw std::runtime_error("auditAgainstMasked: hipStreamSynchronize failed");
    std::vector<SogmMapAuditRow> out(rows);
    audit_rows_.get(out.data(), rows);
    if (out_dt_host) u_.get(out_dt_host, (size_t)n_);
    return out;
  }

 private:
  DevBuf<SogmMapAuditRow> audit_rows_;
  sogm_ctx       *ctx_ = nullptr;
  int             n_;
  SogmSpec        spec_;
  DevBuf<float>   g_, f_;
  DevBuf<int32_t> a_, cnt_;
  DevBuf<double>  p_, q_, t_, u_, pts_;
  DevBuf<int8_t>  o_;
};

// One agent's row of the velocity audit (sogm_abi.h "velocity audit"): the SOGM_VELAUDIT_ROW int64 values, by name.
struct VelAuditRow {
  int64_t n_in, n_born, status, n_nan;
  int64_t confusion[2][4];    // [truth: still, moving][estimate: SOGM_VEL_STATIC, _TRACKED, _UNTRACKED, _DROPPED]
  int64_t speed_moving[6];    // speed-error bins of the scored moving x tracked rows
  int64_t speed_still[6];     // ... of the still x tracked rows: spurious velocity
  int64_t direction[5];       // within 15 degrees, within 45, ahead, behind, a zero estimate
  int64_t sum_e2_um, n_within;  // over the scored moving x tracked rows
  int64_t zero_;
  int64_t scored() const { int64_t n = 0; for (int64_t v : speed_moving) n += v; return n; }
  double  rmsError() const { return scored() ? std::sqrt((double)sum_e2_um * 1e-6 / (double)scored()) : 0.0; }
};
static_assert(sizeof(VelAuditRow) == SOGM_VELAUDIT_ROW * sizeof(int64_t), "VelAuditRow names the 32 values of a row");

// ---- DspMap : dsp_map::DSPMap as owned by RiskVoxel (risk_voxel.cpp:42-50,138-153,237-254) ----------
// One instance serves every agent of a RiskMap created with map_kind = SOGM_MAP_RISKVOXEL.
class DspMap {
 public:
  // DSPMap() + setPredictionVariance / setObservationStdDev / setNewBornParticle* (risk_voxel.cpp:42-49);
  // the Gaussian and rand() tables the reference seeds from time(0) are supplied by the caller.
  DspMap(RiskMap &map, const SogmDspParams &p, const std::vector<float> &p_gauss,
         const std::vector<float> &v_gauss, const std::vector<int32_t> &rand_tab, int max_points = 5000)
      : n_(map.agents()) {
    check(sogm_dsp_create(map.ctx(), &p, p_gauss.data(), v_gauss.data(), (int)p_gauss.size(), rand_tab.data(),
                          (int)rand_tab.size(), max_points, &h_), "sogm_dsp_create");
  }
  ~DspMap() { sogm_dsp_destroy(h_); }
  // MapBase::filterPointCloud (map.cpp:107-132) — device pointers, camera-frame cloud in, body-frame out
  static void filterPointCloud(RiskMap &map, const float *raw_xyz, const int32_t *raw_range, float filter_res,
                               float *out_xyz, int32_t *out_count, int cap = 5000, hipStream_t st = nullptr) {
    check(sogm_filter_point_cloud(map.ctx(), raw_xyz, raw_range, filter_res, cap, out_xyz, out_count, st),
          "sogm_filter_point_cloud");
  }
  // The same with ground-truth velocity labels (sogm_abi.h "ground-truth labels"): raw_code is the hit image of
  // GridMap::renderDepthSwarm in raw_xyz's order, src the frame's records and the bodies' world-axes velocities; labels
  // [n cap 4] is what update() below takes, code [n cap] (may be nullptr) the winning hit code of every output point.
  static void filterPointCloudLabelled(RiskMap &map, const float *raw_xyz, const int32_t *raw_code, const int32_t *raw_range,
                                       float filter_res, const SogmLabelSources &src, float *out_xyz, int32_t *out_count,
                                       float *out_labels, int32_t *out_code = nullptr, int cap = 5000,
                                       hipStream_t st = nullptr) {
    check(sogm_filter_point_cloud_labelled(map.ctx(), raw_xyz, raw_code, raw_range, filter_res, cap, &src, out_xyz,
                                           out_count, out_labels, out_code, st), "sogm_filter_point_cloud_labelled");
  }
  // int DSPMap::update(n, 3, pts, px, py, pz, stamp, qw, qx, qy, qz) for the whole batch (device pointers)
  // labels == nullptr: velocityEstimationThread (clustering + association, :1487-1678) runs on the GPU
  void update(const float *points, const float *labels, const int32_t *cloud_range, const float *sensor_pos,
              const float *sensor_quat, const double *stamps, int32_t *out_ok, hipStream_t st = nullptr) {
    check(sogm_update_dsp(h_, points, labels, cloud_range, sensor_pos, sensor_quat, stamps, out_ok, st),
          "sogm_update_dsp");
  }
  // RiskVoxel::publishMap: getOccupancyMapWithFutureStatus -> risk_maps_ (+ RiskMap::addOtherAgents after)
  void publishMap(int32_t *out_n_occupied = nullptr, hipStream_t st = nullptr) {
    check(sogm_dsp_publish(h_, out_n_occupied, st), "sogm_dsp_publish");
  }
  // Velocity audit (sogm_abi.h "velocity audit"; no reference counterpart) of the last update(): its new-born list against
  // truth labels in the order of the cloud that update was given — filterPointCloudLabelled's labels [points 4] and code
  // [points] (or nullptr), device pointers; cloud_range: that update's.  per_code_host: nullptr, or host room for
  // agents x (n_codes + 2) x 6 values.  Returns one row per agent.  Synchronises `st`.
  std::vector<VelAuditRow> auditVelocity(const float *truth_labels, const int32_t *truth_code, const int32_t *cloud_range,
                                         int n_codes = 0, float speed_tolerance = 0.25f, int64_t *per_code_host = nullptr,
                                         hipStream_t st = nullptr) {
    SogmVelAuditParams prm{};
    prm.speed_tolerance = speed_tolerance, prm.n_codes = n_codes;
    const size_t n_tab = per_code_host && n_codes >= 0 ? (size_t)n_ * (size_t)(n_codes + 2) * 6 : 0;
    vel_rows_.resize((size_t)n_ * SOGM_VELAUDIT_ROW);
    if (n_tab) vel_tab_.resize(n_tab);
    check(sogm_dsp_velocity_audit(h_, truth_labels, truth_code, cloud_range, &prm, vel_rows_.data(),
                                  per_code_host ? vel_tab_.data() : nullptr, st), "sogm_dsp_velocity_audit");
    if (hipStreamSynchronize(st) != hipSuccess) throw std::runtime_error("auditVelocity: hipStreamSynchronize failed");
    std::vector<VelAuditRow> out((size_t)n_);
    vel_rows_.get(reinterpret_cast<int64_t *>(out.data()), (size_t)n_ * SOGM_VELAUDIT_ROW);
    if (n_tab) vel_tab_.get(per_code_host, n_tab);
    return out;
  }

 private:
  sogm_dsp *h_ = nullptr;
  int       n_ = 0;
  DevBuf<int64_t> vel_rows_, vel_tab_;
};

// ---- GridMap : depth-image occupancy front end (plan_env/src/grid_map.cpp) ------------------------------
class GridMap {
 public:
  GridMap(const SogmGridMapParams &p, int n_agents, int device = 0) {  // GridMap::initMap
    check_abi();
    check(sogm_gridmap_create(&p, n_agents, device, &h_), "sogm_gridmap_create");
  }
  ~GridMap() { sogm_gridmap_destroy(h_); }
  // depthPoseCallback + updateOccupancyCallback for the whole batch (device pointers)
  void update(const uint16_t *depth, const double *cam_pos, const double *cam_rot, int32_t *out_updated = nullptr,
              hipStream_t st = nullptr) {
    check(sogm_gridmap_update(h_, depth, cam_pos, cam_rot, out_updated, st), "sogm_gridmap_update");
  }
  // The build's own depth camera (sogm_abi.h "depth camera"): every agent's frame of `frame`'s cylinders (RiskMap::world
  // makes the struct), device pointers, in the layouts update() above (depth) and DspMap::filterPointCloud (cloud, may be
  // nullptr; raw_range[a] = {a rows cols, (a + 1) rows cols}) read.  unsupported [n]: records of a type other than 3.
  static void renderDepth(const SogmWorld &frame, const SogmDepthCamera &cam, int n_agents, const double *cam_pos,
                          const double *cam_rot, uint16_t *depth, float *cloud_xyz, int32_t *unsupported,
                          hipStream_t st = nullptr) {
    check(sogm_render_depth(&frame, &cam, n_agents, cam_pos, cam_rot, depth, cloud_xyz, unsupported, st), "sogm_render_depth");
  }
  // The same with the other vehicles drawn (sogm_abi.h "agent bodies"): bodies (nullptr: none) holds the box centres, the
  // body that carries each camera and the box's size; hit [n rows cols] (may be nullptr) gets per pixel the record index,
  // n_cyl + the body's index, SOGM_HIT_GROUND or SOGM_HIT_NONE.  unsupported also counts bodies with a non-finite centre.
  static void renderDepthSwarm(const SogmWorld &frame, const SogmDepthCamera &cam, const SogmDepthBodies *bodies, int n_agents,
                               const double *cam_pos, const double *cam_rot, uint16_t *depth, float *cloud_xyz, int32_t *hit,
                               int32_t *unsupported, hipStream_t st = nullptr) {
    check(sogm_render_depth_swarm(&frame, &cam, bodies, n_agents, cam_pos, cam_rot, depth, cloud_xyz, hit, unsupported, st),
          "sogm_render_depth_swarm");
  }
  // The sensor-noise pass over such frames (sogm_abi.h "sensor noise"): axial noise, uniform and edge dropout and a minimum
  // range, drawn per pixel from (seed, frame, agent_base + agent, v, u) alone.  in_depth / in_hit (may be nullptr) are only
  // read; depth must not overlap in_depth; cloud_xyz and hit may be nullptr, hit may be in_hit; counts [n * 6]: returns_in,
  // drop_uniform, drop_edge, below_min, beyond_max, returns_out per agent.
  static void addDepthNoise(const SogmDepthCamera &cam, const SogmDepthNoise &noise, int n_agents, const uint16_t *in_depth,
                            const int32_t *in_hit, uint16_t *depth, float *cloud_xyz, int32_t *hit, int32_t *counts,
                            hipStream_t st = nullptr) {
    check(sogm_depth_noise(&cam, &noise, n_agents, in_depth, in_hit, depth, cloud_xyz, hit, counts, st), "sogm_depth_noise");
  }
  // int getInflateOccupancy(Eigen::Vector3d pos) for a batch of device-resident queries
  void getInflateOccupancy(const int32_t *agent_idx, const double *pos, int n, int8_t *out, hipStream_t st = nullptr) {
    check(sogm_gridmap_query_inflate(h_, agent_idx, pos, n, out, st), "sogm_gridmap_query_inflate");
  }

 private:
  sogm_gridmap *h_ = nullptr;
};

// ---- planner: search (KinodynamicAstar-style), CorridorGen, PolyTrajOptimizer, replan ---------------
class Planner {
 public:
  Planner(RiskMap &map, const SogmAstarParams &ap, const SogmPlannerParams &pp, const SogmQpSettings &qs)
      : map_(map), pp_(pp) {
    check(sogm_planner_create(map.ctx(), &ap, &pp, &qs, &p_), "sogm_planner_create");
  }
  ~Planner() { sogm_planner_destroy(p_); }
  sogm_planner *handle() { return p_; }

  // ASTAR_RET search(start_p, start_v, start_a, end_p, ...) + getPathWithVel(corridor_tau) — batched
  void search(const double *start_pva, const double *goal, const double *t_start, int32_t *ret, double *route,
              int32_t *route_len, int route_cap, int32_t *stats, hipStream_t st = nullptr) {
    check(sogm_astar_search(p_, start_pva, goal, t_start, ret, route, route_len, route_cap, stats, nullptr, 0, st),
          "sogm_astar_search");
  }
  // CorridorGen: getObstaclePoints + firi::firi + ShrinkCorridor + validity/intersection/goal LPs — batched
  void generateCorridors(const double *start_pva, const double *t_start, const double *route,
                         const int32_t *route_len, int route_cap, double *polys, int32_t *nfaces, int32_t *npoly,
                         double *goal_pv, hipStream_t st = nullptr) {
    check(sogm_corridor_generate(p_, start_pva, t_start, route, route_len, route_cap, polys, nfaces, npoly,
                                 goal_pv, st), "sogm_corridor_generate");
  }
  // PolyTrajOptimizer::optimize == BezierOpt::setup + optimize — batched
  void optimize(const double *start_pva, const double *goal_pv, const double *polys, const int32_t *nfaces,
                const int32_t *npoly, double *cpts, int32_t *status, int32_t *iters, hipStream_t st = nullptr) {
    check(sogm_bezier_qp_solve(p_, start_pva, goal_pv, polys, nfaces, npoly, cpts, status, iters, st),
          "sogm_bezier_qp_solve");
  }
  // Publication and pre-stamp of the tick loop (no reference counterparts: plan_manager.cpp:176-196 / :364-399 keep
  // the latest trajectory per drone on the host; here the replan's finishing kernel does, and — with a pre-stamp
  // registered — the replan also builds the next tick's start states and map, see sogm_abi.h)
  void setPublish(SogmTrajRecord *own_records, SogmTrajRecord *next_table = nullptr) {
    check(sogm_planner_set_publish(p_, own_records, next_table), "sogm_planner_set_publish");
  }
  void setPrestamp(const SogmPrestamp *next_tick) {
    check(sogm_planner_set_prestamp(p_, next_tick), "sogm_planner_set_prestamp");
  }
  // replan() ends with isSafeAfterOpt of every agent against its OWN table: dev views [n_agents][n_records]
  // (Links::views()), ego_ids / t_now dev [n_agents]; read by later replan() calls (sogm_planner_set_swarm_views)
  void setSwarmViews(const SogmTrajRecord *views, int n_records, const int32_t *ego_ids, const double *t_now) {
    check(sogm_planner_set_swarm_views(p_, views, n_records, ego_ids, t_now), "sogm_planner_set_swarm_views");
  }
  // The reference plans only in NEW_PLAN and REPLAN (plan_manager.cpp:110-135,164-175): later replan() calls plan only
  // the agents with due[a] != 0 (dev int32 [n_agents], e.g. Fsm::due()); nullptr = every agent (sogm_planner_set_due)
  void setDue(const int32_t *due_dev_or_null) { check(sogm_planner_set_due(p_, due_dev_or_null), "sogm_planner_set_due"); }
  // Later flight() calls fly under the per-agent FSM: every agent-tick is one FSMCallback, only the agents that are due
  // replan (sogm_planner_set_flight_fsm; the struct is copied, its device pointers — e.g. Fsm::state() — are kept);
  // nullptr = off: every agent replans in every tick.  replan() never looks at it.
  void setFlightFsm(const SogmFlightFsm *fsm_or_null) {
    check(sogm_planner_set_flight_fsm(p_, fsm_or_null), "sogm_planner_set_flight_fsm");
  }
  // n ticks of every agent in one call, every agent on its own clock (the reference's drones each run their own FSM,
  // plan_manager.cpp:92-233): sogm_flight_run, see sogm_abi.h "Flight".  Returns the device's verdict after a
  // synchronisation when `wait` is set: false = a device-side wait timed out (sogm_flight_stats hdr[4]).
  bool flight(const SogmFlight &f, hipStream_t st = nullptr, bool wait = false) {
    check(sogm_flight_run(p_, &f, st), "sogm_flight_run");
    if (!wait) return true;
    int32_t hdr[32];
    check(sogm_flight_stats(p_, nullptr, hdr), "sogm_flight_stats");
    return hdr[4] == 0 && hdr[15] == 0;  // no time-out, and every workgroup of the flight was resident from the start
  }
  // bool BaselinePlanner::replan(t, start_pos, start_vel, start_acc, goal_pos) — batched
  void replan(const double *start_pva, const double *goal, const double *t_start, const int32_t *drone_ids,
              SogmTrajRecord *records, int32_t *ok, hipStream_t st = nullptr) {
    check(sogm_replan(p_, start_pva, goal, t_start, drone_ids, records, ok, st), "sogm_replan");
  }

 private:
  RiskMap          &map_;
  SogmPlannerParams pp_;
  sogm_planner     *p_ = nullptr;
};

// FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233) for n agents: owns the machines' records and
// the tick's per-agent flags on the device.  A tick is inputs() -> map update, sogm_traj_safe ->
// Planner::setDue(due()) + Planner::replan -> apply(); both calls are one launch on the caller's stream.
class Fsm {
 public:
  Fsm(int n, const SogmFsmParams &prm, double traj_start0, hipStream_t st = nullptr) : n_(n), prm_(prm) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    try {
      alloc(&state_, nn * sizeof(SogmFsmState));
      alloc(&due_, nn * sizeof(int32_t));
      alloc(&reached_, nn * sizeof(int32_t));
      alloc(&pub_, nn * sizeof(int32_t));
      alloc(&pos_now_, nn * 3 * sizeof(double));
      alloc(&hover_start_, nn * sizeof(double));
      check(sogm_fsm_init(state_, n_, traj_start0, st), "sogm_fsm_init");
    } catch (...) {
      release();  // (no destructor runs for a constructor that throws)
      throw;
    }
  }
  ~Fsm() { release(); }
  Fsm(const Fsm &)            = delete;
  Fsm &operator=(const Fsm &) = delete;

  // the head of the tick (:110-135, :165-175): who is due and the replan's start states, start times and map centres
  void inputs(const SogmTrajRecord *own_records, const double *goals, double stamp, double *hover_inout, double *out_now,
              double *out_t_start, double *out_pva, float *out_poses, hipStream_t st = nullptr) {
    check(sogm_fsm_inputs(&prm_, state_, own_records, goals, n_, stamp, hover_inout, out_now, out_t_start, out_pva,
                          out_poses, pos_now_, due_, reached_, st), "sogm_fsm_inputs");
  }
  // the state update and the publication into own_inout (the new record, publishEmptyTrajectory's, or nothing)
  void apply(const int32_t *ok, const int32_t *safe, const SogmTrajRecord *new_records, const int32_t *drone_ids,
             SogmTrajRecord *own_inout, double stamp, hipStream_t st = nullptr) {
    check(sogm_fsm_apply(&prm_, state_, due_, ok, safe, reached_, new_records, drone_ids, pos_now_, own_inout, pub_,
                         hover_start_, n_, stamp, st), "sogm_fsm_apply");
  }
  // device arrays [n] of the last inputs() / apply()
  const int32_t *due() const { return due_; }
  SogmFsmState  *state() { return state_; }  // the machines' records, dev [n] (SogmFlightFsm::state_inout for a flight)
  const int32_t *reached() const { return reached_; }
  const int32_t *published() const { return pub_; }  // SOGM_FSM_PUB_*
  const double  *posNow() const { return pos_now_; }  // [n][3]
  const double  *hoverStart() const { return hover_start_; }  // start time of the hover record where published() says HOVER
  // the machines as they stand (synchronises the stream)
  std::vector<SogmFsmState> states(hipStream_t st = nullptr) const {
    std::vector<SogmFsmState> out((size_t)n_);
    if (n_ > 0) {
      if (hipMemcpyAsync(out.data(), state_, out.size() * sizeof(SogmFsmState), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        throw std::runtime_error("sogm_host::Fsm::states: copy failed");
    }
    return out;
  }

 private:
  template <typename T>
  static void alloc(T **p, size_t bytes) {
    if (hipMalloc((void **)p, bytes) != hipSuccess) throw std::runtime_error("sogm_host::Fsm: hipMalloc failed");
  }
  void release() {
    for (void *q : {(void *)state_, (void *)due_, (void *)reached_, (void *)pub_, (void *)pos_now_, (void *)hover_start_})
      if (q) (void)hipFree(q);
  }
  int            n_;
  SogmFsmParams  prm_;
  SogmFsmState  *state_ = nullptr;
  int32_t       *due_ = nullptr, *reached_ = nullptr, *pub_ = nullptr;
  double        *pos_now_ = nullptr, *hover_start_ = nullptr;
};

// Flight audit (sogm_abi.h "flight audit"): owns the accumulators of n_local agents and the event list on the device;
// add() audits a batch of executed tables on the caller's stream (no synchronisation), agents() / events() read them back.
class Audit {
 public:
  Audit(const SogmAuditParams &prm, int n_local, void *stream = nullptr)
      : prm_(prm), n_(n_local), acc_((size_t)(n_local > 0 ? n_local : 1)),
        ev_((size_t)(prm.event_capacity > 0 ? prm.event_capacity : 1)), n_ev_(1) {
    check_abi();
    check(sogm_audit_init_agents(acc_.data(), n_local, stream), "sogm_audit_init_agents");
    (void)hipMemsetAsync(n_ev_.data(), 0, sizeof(int32_t), (hipStream_t)stream);
  }
  // dev tables [n_ticks][n_total], prev_table [n_total] or null, fallback_pos [n_total][3], goals [n_local][3], cylinders [n_cyl]
  void add(const SogmTrajRecord *tables, int n_ticks, int n_total, const SogmTrajRecord *prev_table, double t0, int first_tick,
           double period, int agent0, const double *fallback_pos, const double *goals, const SogmCylinder *cylinders,
           int n_cyl, void *stream = nullptr) {
    check(sogm_swarm_audit(&prm_, tables, n_ticks, n_total, prev_table, t0, first_tick, period, agent0, n_, fallback_pos,
                           goals, cylinders, n_cyl, acc_.data(), prm_.event_capacity > 0 ? ev_.data() : nullptr,
                           n_ev_.data(), stream),
          "sogm_swarm_audit");
  }
  // synchronous read-backs
  std::vector<SogmAuditAgent> agents() {
    std::vector<SogmAuditAgent> out((size_t)n_);
    (void)hipDeviceSynchronize();
    acc_.get(out.data(), out.size());
    return out;
  }
  // the kept events (earliest first) and, in *seen, every colliding sample counted (-1: an unsupported obstacle type)
  std::vector<SogmAuditEvent> events(int32_t *seen = nullptr) {
    int32_t n = 0;
    (void)hipDeviceSynchronize();
    n_ev_.get(&n, 1);
    if (seen) *seen = n;
    const int kept = n < 0 ? 0 : (n < prm_.event_capacity ? n : prm_.event_capacity);
    std::vector<SogmAuditEvent> out((size_t)kept);
    if (kept) ev_.get(out.data(), out.size());
    return out;
  }

 private:
  SogmAuditParams        prm_;
  int                    n_;
  DevBuf<SogmAuditAgent> acc_;
  DevBuf<SogmAuditEvent> ev_;
  DevBuf<int32_t>        n_ev_;
};

// quadrotor_msgs/PositionCommand as publishCmd fills it (traj_server/src/bezier_traj_server.cpp:163-187): the fields a
// host copies into the message it publishes on position_cmd.  header.frame_id is "world", trajectory_flag
// TRAJECTORY_STATUS_READY (1); `publish` is false where PubCallback returned without publishing.
struct PositionCommandFields {
  bool    publish = false;
  double  stamp = 0.0;  // header.stamp (ros::Time::now() of the timer)
  Vec3    position{}, velocity{}, acceleration{};
  double  yaw = 0.0, yaw_dot = 0.0;
  int32_t trajectory_id = 0;
  uint8_t trajectory_flag = 1;
};
inline PositionCommandFields positionCommandFields(const SogmPositionCommand &c) {
  PositionCommandFields f;
  f.publish = (c.flags & SOGM_CMD_PUBLISHED) != 0;
  f.stamp   = c.t_pub;
  for (int d = 0; d < 3; ++d) {
    f.position[d]     = c.pos[d];
    f.velocity[d]     = c.vel[d];
    f.acceleration[d] = c.acc[d];
  }
  f.yaw           = c.yaw;
  f.yaw_dot       = c.yaw_dot;
  f.trajectory_id = c.traj_id;
  return f;
}

// Trajectory server (sogm_abi.h "trajectory server"): owns the states and rings of n_local agents on the device; run()
// serves a batch of executed tables on the caller's stream (no synchronisation) into a command buffer it owns,
// commands() reads the last call's commands back, cameraPoses() hands one command per agent to sogm_render_depth's layouts.
class TrajServer {
 public:
  // dev init_pos [n_local][3], dev init_yaw [n_local] or null
  TrajServer(const SogmTrajServerParams &prm, int n_local, double t_trigger, const double *init_pos, const double *init_yaw,
             void *stream = nullptr)
      : prm_(prm), n_(n_local), state_((size_t)(n_local > 0 ? n_local : 1)),
        queue_((size_t)(n_local > 0 ? n_local : 1) * SOGM_TRAJSRV_QUEUE) {
    check_abi();
    check(sogm_traj_server_init(state_.data(), queue_.data(), n_local, t_trigger, init_pos, init_yaw, stream),
          "sogm_traj_server_init");
  }
  // dev tables [n_ticks][n_total], prev_table [n_total] or null, received int32 [n_ticks][n_local] or null; samples_per_tick
  // = period / sample_dt.  Returns the device commands [n_local][n_ticks * samples_per_tick].
  const SogmPositionCommand *run(const SogmTrajRecord *tables, int n_ticks, int n_total, const SogmTrajRecord *prev_table,
                                 const int32_t *received, double t0, int first_tick, double period, int agent0,
                                 int samples_per_tick, double receive_delay = 0.0, void *stream = nullptr) {
    per_agent_ = n_ticks > 0 && samples_per_tick > 0 ? n_ticks * samples_per_tick : 0;
    cmd_.resize((size_t)(n_ > 0 ? n_ : 1) * (size_t)(per_agent_ > 0 ? per_agent_ : 1));
    check(sogm_traj_server_run(&prm_, state_.data(), queue_.data(), tables, prev_table, received, n_ticks, n_total, agent0,
                               n_, t0, first_tick, period, receive_delay, cmd_.data(), stream),
          "sogm_traj_server_run");
    return cmd_.data();
  }
  int commandsPerAgent() const { return per_agent_; }
  // the camera poses at command `sample` of the last run: dev out_pos [n_local][3], out_rot [n_local][9]
  void cameraPoses(int sample, const double cam2body[9], const double cam_offset[3], double *out_pos, double *out_rot,
                   void *stream = nullptr) {
    if (sample < 0 || sample >= per_agent_) throw std::out_of_range("sogm_host::TrajServer::cameraPoses: no such command");
    check(sogm_camera_poses(cmd_.data() + sample, n_, per_agent_, cam2body, cam_offset, out_pos, out_rot, stream),
          "sogm_camera_poses");
  }
  // synchronous read-backs
  std::vector<SogmPositionCommand> commands() {
    std::vector<SogmPositionCommand> out((size_t)n_ * (size_t)per_agent_);
    (void)hipDeviceSynchronize();
    if (!out.empty()) cmd_.get(out.data(), out.size());
    return out;
  }
  std::vector<SogmTrajServerState> states() {
    std::vector<SogmTrajServerState> out((size_t)n_);
    (void)hipDeviceSynchronize();
    state_.get(out.data(), out.size());
    return out;
  }

 private:
  SogmTrajServerParams         prm_;
  int                          n_, per_agent_ = 0;
  DevBuf<SogmTrajServerState>  state_;
  DevBuf<SogmTrajPoint>        queue_;
  DevBuf<SogmPositionCommand>  cmd_;
};

// Radio links (sogm_abi.h "radio links"): owns the ring of sent tables, the views, the held ticks and the counters of the
// receivers [agent0, agent0 + n_local) of an n_total swarm on the device.  deliver() is one tick on the caller's stream (no
// synchronisation), ticks consecutive from the first; views() is what RiskMap::addOtherAgentsViews / updateWorldViews and
// Planner::setSwarmViews take.
class Links {
 public:
  Links(const SogmLinkParams &prm, int n_total, int agent0, int n_local, void *stream = nullptr)
      : prm_(prm), n_total_(n_total), agent0_(agent0), n_local_(n_local) {
    check_abi();
    const size_t slots = (size_t)(prm.delay_max >= 0 && prm.delay_max <= SOGM_LINK_MAX_DELAY ? prm.delay_max : 0) + 1;
    const size_t nt = (size_t)(n_total > 0 ? n_total : 1), nl = (size_t)(n_local > 0 ? n_local : 1);
    ring_table_.resize(slots * nt);
    ring_pos_.resize(slots * nt * 3);
    views_.resize(nl * nt);
    held_.resize(nl * nt);
    counters_.resize(nl * SOGM_LINK_COUNTERS);
    buf_ = SogmLinkBuffers{ring_table_.data(), ring_pos_.data(), views_.data(), held_.data(), counters_.data()};
    belief_.resize(beliefSize());
    check(sogm_link_init(&prm_, n_total, n_local, &buf_, stream), "sogm_link_init");
    (void)hipMemsetAsync(belief_.data(), 0, beliefSize() * sizeof(int64_t), (hipStream_t)stream);
  }
  static SogmLinkParams defaultParams() {
    SogmLinkParams p;
    check(sogm_link_default_params(&p), "sogm_link_default_params");
    return p;
  }
  // dev table [n_total] (what every agent executes after `tick`), dev pos [n_total][3] or null (needed with a range)
  const SogmTrajRecord *deliver(int tick, const SogmTrajRecord *table, const double *pos, void *stream = nullptr) {
    if (next_ >= 0 && tick != next_) throw std::logic_error("sogm_host::Links::deliver: ticks are consecutive");
    if (next_ < 0) tick0_ = tick;
    if (has_noise_) {
      check(sogm_traj_noise(&noise_, tick, table, n_total_, sent_.data(), sent_shift_.data(), stream), "sogm_traj_noise");
      table = sent_.data();
    }
    check(sogm_link_deliver(&prm_, tick, tick0_, table, pos, n_total_, agent0_, n_local_, &buf_, stream), "sogm_link_deliver");
    next_ = tick + 1;
    return views_.data();
  }
  const SogmTrajRecord *views() { return views_.data(); }
  // Message noise (sogm_abi.h "message noise"): from now on deliver() sends every table through sogm_traj_noise into a
  // buffer of this object's (sent(), its shifts in sentShift()) and the links carry that; the caller's table is not
  // touched and the positions stay the true ones.  All-zero parameters send the table as it is.  setNoise allocates the
  // buffer (call it before the run, not between two ticks in flight).
  static SogmTrajNoise defaultNoise() {
    SogmTrajNoise p;
    check(sogm_traj_noise_default_params(&p), "sogm_traj_noise_default_params");
    return p;
  }
  void setNoise(const SogmTrajNoise &noise) {
    noise_     = noise;
    has_noise_ = true;
    sent_.resize((size_t)(n_total_ > 0 ? n_total_ : 1));
    sent_shift_.resize((size_t)(n_total_ > 0 ? n_total_ : 1) * 4);
  }
  const SogmTrajRecord *sent() { return sent_.data(); }
  const double         *sentShift() { return sent_shift_.data(); }
  // Belief audit (sogm_abi.h "belief audit"): scores views() against dev truth [n_total], the table the senders execute,
  // at the receivers' times dev t_now [n_local]; every call adds to belief() (the counters were allocated and zeroed by the
  // constructor: stream-ordered from the first call, no synchronisation).
  static SogmBeliefParams defaultBeliefParams() {
    SogmBeliefParams p;
    check(sogm_belief_default_params(&p), "sogm_belief_default_params");
    return p;
  }
  void auditBelief(const SogmBeliefParams &prm, const SogmTrajRecord *truth, const double *t_now, void *stream = nullptr) {
    check(sogm_belief_audit(&prm, truth, views_.data(), t_now, n_total_, agent0_, n_local_, belief_.data(), nullptr, stream),
          "sogm_belief_audit");
  }
  // synchronous read-back: [n_local][SOGM_BELIEF_COUNTERS] (all zero before the first auditBelief)
  std::vector<int64_t> belief() {
    std::vector<int64_t> out(beliefSize());
    (void)hipDeviceSynchronize();
    belief_.get(out.data(), out.size());
    return out;
  }
  // synchronous read-backs: counters [n_local][SOGM_LINK_COUNTERS], held ticks [n_local][n_total]
  std::vector<int64_t> counters() {
    std::vector<int64_t> out((size_t)n_local_ * SOGM_LINK_COUNTERS);
    (void)hipDeviceSynchronize();
    counters_.get(out.data(), out.size());
    return out;
  }
  std::vector<int32_t> heldTicks() {
    std::vector<int32_t> out((size_t)n_local_ * (size_t)n_total_);
    (void)hipDeviceSynchronize();
    held_.get(out.data(), out.size());
    return out;
  }

 private:
  SogmLinkParams         prm_;
  int                    n_total_, agent0_, n_local_, tick0_ = 0, next_ = -1;
  DevBuf<SogmTrajRecord> ring_table_, views_;
  DevBuf<double>         ring_pos_;
  DevBuf<int32_t>        held_;
  DevBuf<int64_t>        counters_;
  SogmLinkBuffers        buf_{};
  size_t                 beliefSize() const { return (size_t)(n_local_ > 0 ? n_local_ : 1) * SOGM_BELIEF_COUNTERS; }
  SogmTrajNoise          noise_{};
  bool                   has_noise_ = false;
  DevBuf<SogmTrajRecord> sent_;
  DevBuf<double>         sent_shift_;
  DevBuf<int64_t>        belief_;
};

}  // namespace sogm_host
