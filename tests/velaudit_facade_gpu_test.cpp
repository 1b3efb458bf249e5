// GPU use of host/sogm_facade.hpp's DspMap::auditVelocity: two frames of a 27-point cluster stepping 0.25 m in 0.5 s along x, a
// 4-point cluster (rejected by the clustering: its points vanish from the new-born list) and six ground points, fed to
// DspMap::update with labels == nullptr; the audit against hand-written truth labels and codes.  The second agent's range is
// empty.  Prints "velocity audit facade ok".
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_facade.hpp"

using namespace sogm_host;

#define REQUIRE(cond)                                                 \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("REQUIRE failed: %s (line %d)\n", #cond, __LINE__); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

int main() {
  static_assert(sizeof(SogmVelAuditParams) == 16 && SOGM_VELAUDIT_ROW == 32, "layout");
  static_assert(offsetof(VelAuditRow, confusion) == 4 * 8 && offsetof(VelAuditRow, speed_still) == 18 * 8 &&
                    offsetof(VelAuditRow, direction) == 24 * 8 && offsetof(VelAuditRow, sum_e2_um) == 29 * 8, "row fields");
  if (sogm_device_count() < 1) {
    std::puts("no device");
    return 77;
  }
  SogmSpec spec{};
  spec.L = 66; spec.W = 66; spec.H = 20; spec.T = 6;
  spec.resolution = 0.15f; spec.time_resolution = 0.2f; spec.risk_threshold = 0.2f; spec.clearance = 0.45f;
  spec.ground_height = -0.01f; spec.ceiling_height = 3.0f; spec.risk_threshold_region = 1.2f;
  spec.risk_thres_reg_decay = 0.2f; spec.risk_thres_vox_decay = 0.2f;
  spec.map_kind = SOGM_MAP_RISKVOXEL; spec.storage = SOGM_STORE_F32;
  const int A = 2, cap = 64;
  RiskMap map(spec, A);
  SogmDspParams dp{};
  dp.max_particle_num_voxel = 7; dp.half_fov_h = 43; dp.half_fov_v = 29; dp.angle_resolution = 1; dp.newborn_num = 20;
  dp.obs_max_per_pyramid = 100;
  for (int t = 0; t < SOGM_DSP_MAX_T; ++t) dp.prediction_times[t] = 0.3f * (float)(t + 1);
  dp.sigma_observation = 0.05f; dp.p_detection = 0.95f; dp.kappa = 0.01f; dp.newborn_weight = 0.0001f; dp.obstacle_thickness = 0.3f;
  std::vector<float>   pg(4096), vg(4096);
  std::vector<int32_t> rnd(1024);
  unsigned             lcg = 12345u;
  for (size_t i = 0; i < pg.size(); ++i) {
    lcg   = lcg * 1664525u + 1013904223u;
    pg[i] = ((float)(lcg >> 8) / 16777216.f - 0.5f) * 0.1f;
    lcg   = lcg * 1664525u + 1013904223u;
    vg[i] = ((float)(lcg >> 8) / 16777216.f - 0.5f) * 0.1f;
  }
  for (auto &r : rnd) {
    lcg = lcg * 1664525u + 1013904223u;
    r   = (int32_t)(lcg >> 1);
  }
  DspMap dsp(map, dp, pg, vg, rnd, cap);

  const float sensor[3] = {0.f, 0.f, 0.5f};
  std::vector<float>   truth;  // per input point {vx, vy, vz, intensity}
  std::vector<int32_t> code;
  int                  n_pts = 0;
  auto cloud_at = [&](float x0, bool fill_truth) {
    std::vector<float> c;
    auto put = [&](float x, float y, float z, float tvx, float tvy, float inten, int cd) {  // world -> sensor frame
      c.push_back(x - sensor[0]), c.push_back(y - sensor[1]), c.push_back(z - sensor[2]);
      if (fill_truth) {
        truth.insert(truth.end(), {tvx, tvy, 0.f, inten});
        code.push_back(cd);
      }
    };
    for (int i = 0; i < 6; ++i) put(1.f + 0.25f * i, -3.f, 0.0625f, 0.f, 0.f, 0.f, SOGM_HIT_GROUND);
    for (int i = 0; i < 27; ++i) put(x0 + 0.125f * (i % 3), 0.125f * ((i / 3) % 3), 0.25f + 0.125f * (i / 9), 0.5f, 0.f, 1.f, 0);
    for (int i = 0; i < 4; ++i) put(4.f + 0.125f * i, 2.f, 0.25f, 0.f, 0.5f, 1.f, 1);
    return c;
  };
  DevBuf<float>   d_pts, d_pos, d_quat, d_truth;
  DevBuf<int32_t> d_range, d_ok, d_code;
  DevBuf<double>  d_stamps;
  const float pos[6] = {sensor[0], sensor[1], sensor[2], 5.f, 5.f, 0.5f}, quat[8] = {1, 0, 0, 0, 1, 0, 0, 0};
  d_pos.put(pos, 6), d_quat.put(quat, 8), d_ok.resize(A);
  for (int k = 0; k < 2; ++k) {
    const std::vector<float> c = cloud_at(2.f + 0.25f * k, k == 1);
    n_pts                      = (int)c.size() / 3;
    const int32_t range[4]     = {0, n_pts, n_pts, n_pts};
    const double  stamps[2]    = {20.0 + 0.5 * k, 20.0 + 0.5 * k};
    d_pts.put(c.data(), c.size()), d_range.put(range, 4), d_stamps.put(stamps, 2);
    dsp.update(d_pts.data(), nullptr, d_range.data(), d_pos.data(), d_quat.data(), d_stamps.data(), d_ok.data());
  }
  int32_t ok[2] = {0, 0};
  REQUIRE(hipDeviceSynchronize() == hipSuccess);
  d_ok.get(ok, 2);
  REQUIRE(ok[0] == 1 && ok[1] == 1 && n_pts == 37);
  d_truth.put(truth.data(), truth.size()), d_code.put(code.data(), code.size());
  std::vector<int64_t> tab((size_t)A * 4 * 6, -1);
  const auto rows = dsp.auditVelocity(d_truth.data(), d_code.data(), d_range.data(), 2, 0.25f, tab.data());
  REQUIRE(rows.size() == 2);
  const VelAuditRow &r = rows[0];
  REQUIRE(r.n_in == 37 && r.n_born == 33 && r.status == 0 && r.n_nan == 0);
  REQUIRE(r.confusion[0][SOGM_VEL_STATIC] == 6 && r.confusion[1][SOGM_VEL_TRACKED] == 27 && r.confusion[1][SOGM_VEL_DROPPED] == 4);
  int64_t sum = 0;
  for (int t = 0; t < 2; ++t)
    for (int e = 0; e < 4; ++e) sum += r.confusion[t][e];
  REQUIRE(sum == 37);
  REQUIRE(r.speed_moving[0] == 27 && r.direction[0] == 27 && r.n_within == 27 && r.scored() == 27 && r.rmsError() < 1e-3);
  REQUIRE(r.sum_e2_um == 0 && r.zero_ == 0);  // an error of ~1e-7 m/s squared is below one micro-unit
  // per code: record 0 tracked, record 1 dropped, the ground static, nothing else
  REQUIRE(tab[0 * 6 + 1] == 27 && tab[0 * 6 + 4] == 27 && tab[1 * 6 + 3] == 4 && tab[2 * 6 + 0] == 6);
  int64_t cells = 0;
  for (int row = 0; row < 4; ++row)
    for (int e = 0; e < 4; ++e) cells += tab[row * 6 + e];
  REQUIRE(cells == 37);
  // the second agent's range is empty: SKIPPED and zeros
  REQUIRE(rows[1].status == SOGM_VELAUDIT_SKIPPED && rows[1].n_in == 0 && rows[1].n_born == 0);
  for (int i = 0; i < 24; ++i) REQUIRE(tab[24 + i] == 0);
  // without codes and a table
  const auto again = dsp.auditVelocity(d_truth.data(), nullptr, d_range.data());
  REQUIRE(std::memcmp(again.data(), rows.data(), sizeof(VelAuditRow) * 2) == 0);
  // a refusal reaches the caller as an exception that names the entry
  bool threw = false;
  try {
    (void)dsp.auditVelocity(d_truth.data(), nullptr, d_range.data(), 0, -1.0f);
  } catch (const std::exception &e) {
    threw = std::strstr(e.what(), "sogm_dsp_velocity_audit") != nullptr;
  }
  REQUIRE(threw);
  std::puts("velocity audit facade ok");
  return 0;
}
