// sogm_host::Fsm and Planner::setDue (pred-occ-planner_amd/host/sogm_facade.hpp) on a GPU: twelve closed-loop ticks of two
// agents around one pillar — Fsm::inputs -> map update -> sogm_traj_safe -> setDue + replan -> Fsm::apply — with the same
// rules (csrc/sogm_fsm.hpp) run on the host beside them from the tick's downloaded flags: states, due bits, publication
// kinds and hover start times must agree tick by tick, an agent that is not due reports ok = 0 and keeps its record, a
// published plan is the tick's new record.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pred-occ-planner_amd/csrc/sogm_fsm.hpp"
#include "sogm_facade.hpp"

using namespace sogm_host;

#define REQUIRE(cond)                                               \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("REQUIRE failed: %s (line %d)\n", #cond, __LINE__); \
      return 1;                                                     \
    }                                                               \
  } while (0)

int main() {
  if (sogm_device_count() < 1) {
    std::puts("no device");
    return 77;
  }
  SogmSpec spec{};
  spec.L = 66; spec.W = 66; spec.H = 20; spec.T = 6;
  spec.resolution = 0.15f; spec.time_resolution = 0.2f; spec.risk_threshold = 0.2f; spec.clearance = 0.45f;
  spec.ground_height = -0.01f; spec.ceiling_height = 3.0f; spec.risk_threshold_region = 1.2f;
  spec.risk_thres_reg_decay = 0.2f; spec.risk_thres_vox_decay = 0.2f;
  spec.map_kind = SOGM_MAP_FAKE; spec.storage = SOGM_STORE_F32;
  const int A = 2;
  RiskMap map(spec, A);
  std::vector<Vec3> body;
  for (double x = -0.2; x <= 0.2; x += 0.15)
    for (double y = -0.2; y <= 0.2; y += 0.15)
      for (double z = -0.225; z <= 0.225; z += 0.15) body.push_back({x, y, z});
  map.setCoordinator(body);
  std::vector<float> cloud;
  for (int k = 0; k < 48; ++k)
    for (int iz = 0; iz < 30; ++iz) {
      cloud.push_back(0.4f * std::cos(k * 0.1309f));
      cloud.push_back(0.4f * std::sin(k * 0.1309f));
      cloud.push_back(0.1f * iz);
    }
  const int n_pts = (int)cloud.size() / 3;
  SogmCylinder cyl{};
  cyl.type = 3; cyl.x = 0; cyl.y = 0; cyl.z = 1.5; cyl.w = 0.8; cyl.h = 3.0; cyl.qw = 1.0;
  const int32_t range[4] = {0, n_pts, 0, n_pts};
  DevBuf<float> d_cloud; DevBuf<int32_t> d_range; DevBuf<SogmCylinder> d_cyl;
  d_cloud.put(cloud.data(), cloud.size()); d_range.put(range, 4); d_cyl.put(&cyl, 1);
  SogmAstarParams ap{}; ap.max_tau = 2.0; ap.max_vel = 2.0; ap.max_acc = 6.0; ap.w_time = 5.0; ap.horizon = 5.0;
  ap.lambda_heu = 5.0; ap.resolution = 0.15; ap.time_resolution = 0.3; ap.allocate_num = 10000; ap.check_num = 1;
  ap.tolerance = 1;
  SogmPlannerParams pp{}; pp.corridor_tau = 0.3; pp.init_range = 1.2; pp.shrink_size = 0.2; pp.opt_max_vel = 3.0;
  pp.opt_max_acc = 6.0; pp.fake_planner = 1; pp.firi_iterations = 2; pp.pc_capacity = 16384; pp.max_faces = 64;
  SogmQpSettings qs{}; qs.rho = 0.1; qs.sigma = 1e-6; qs.alpha = 1.6; qs.eps_abs = 1e-3; qs.eps_rel = 1e-3;
  qs.max_iter = 4000; qs.check_termination = 25; qs.scaling_iters = 10; qs.adaptive_rho_interval = 25;
  Planner planner(map, ap, pp, qs);

  const double  t0 = 100.0;
  SogmFsmParams prm{0.1, 0.02, 1.0, 1.0, 5, 0};
  Fsm           fsm(A, prm, t0 - 2.0);
  const double  hover0[18] = {-3, 0.1, 1, 0, 0, 0, 0, 0, 0, 3, -0.1, 1, 0, 0, 0, 0, 0, 0};
  const double  goal[6]    = {3, 0.1, 1, -3, -0.1, 1};
  const int32_t ids[2]     = {0, 1};
  DevBuf<double> d_hover, d_goal, d_now(A), d_t(A), d_pva(A * 9);
  DevBuf<float>  d_poses(A * 3);
  DevBuf<int32_t> d_ids, d_ok(A), d_safe(A);
  DevBuf<SogmTrajRecord> d_own(A), d_new(A);
  std::vector<SogmTrajRecord> zero(A);
  std::memset(zero.data(), 0, sizeof(SogmTrajRecord) * A);
  d_hover.put(hover0, 18); d_goal.put(goal, 6); d_ids.put(ids, 2); d_own.put(zero.data(), A);

  std::vector<SogmFsmState> mirror(A, SogmFsmState{t0 - 2.0, sogm::FSM_NEW_PLAN, 0, 0, 0});
  int n_spared = 0, n_new = 0;
  for (int k = 0; k < 12; ++k) {
    const double stamp = t0 + 0.1 * k;
    SogmTrajRecord before[2], after[2], fresh[2];
    d_own.get(before, A);
    fsm.inputs(d_own.data(), d_goal.data(), stamp, d_hover.data(), d_now.data(), d_t.data(), d_pva.data(), d_poses.data());
    map.update(d_cloud.data(), d_range.data(), d_cyl.data(), 1, d_poses.data(), d_now.data());
    REQUIRE(sogm_traj_safe(map.ctx(), d_own.data(), d_now.data(), 0.2, d_safe.data(), nullptr) == SOGM_OK);
    planner.setDue(fsm.due());
    planner.replan(d_pva.data(), d_goal.data(), d_t.data(), d_ids.data(), d_new.data(), d_ok.data());
    fsm.apply(d_ok.data(), d_safe.data(), d_new.data(), d_ids.data(), d_own.data(), stamp);
    const std::vector<SogmFsmState> got = fsm.states();
    int32_t due[2], ok[2], safe[2], reached[2], pub[2];
    double  hs[2], tst[2];
    REQUIRE(hipMemcpy(due, fsm.due(), sizeof(due), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(reached, fsm.reached(), sizeof(reached), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(pub, fsm.published(), sizeof(pub), hipMemcpyDeviceToHost) == hipSuccess);
    REQUIRE(hipMemcpy(hs, fsm.hoverStart(), sizeof(hs), hipMemcpyDeviceToHost) == hipSuccess);
    d_ok.get(ok, A); d_safe.get(safe, A); d_t.get(tst, A); d_own.get(after, A); d_new.get(fresh, A);
    for (int a = 0; a < A; ++a) {
      const sogm::FsmDue wd = sogm::fsm_due(mirror[a], stamp, prm);
      REQUIRE(due[a] == wd.bits && tst[a] == wd.t_start);
      if (!due[a]) {
        REQUIRE(ok[a] == 0 && fresh[a].n_pieces == 0);  // not planned
        ++n_spared;
      }
      const sogm::FsmPub wp = sogm::fsm_step(mirror[a], wd.bits, ok[a] != 0, safe[a] != 0, reached[a] != 0, stamp, prm);
      REQUIRE(got[a].status == mirror[a].status && got[a].fail == mirror[a].fail && got[a].success == mirror[a].success &&
              got[a].traj_start == mirror[a].traj_start);
      REQUIRE(pub[a] == wp.kind && hs[a] == wp.hover_start);
      if (pub[a] == SOGM_FSM_PUB_NEW) {
        REQUIRE(std::memcmp(&after[a], &fresh[a], sizeof(SogmTrajRecord)) == 0 && after[a].n_pieces > 0 &&
                after[a].time_start == wd.t_start);
        ++n_new;
      } else if (pub[a] == SOGM_FSM_PUB_HOVER) {
        REQUIRE(after[a].n_pieces == 1 && after[a].duration[0] == 0.5 && after[a].time_start == hs[a] &&
                after[a].drone_id == ids[a]);
      } else {
        REQUIRE(std::memcmp(&after[a], &before[a], sizeof(SogmTrajRecord)) == 0);
      }
    }
  }
  REQUIRE(n_new >= 2 && n_spared >= 2);  // both agents planned, and somebody was spared a replan
  planner.setDue(nullptr);
  std::puts("facade fsm ok");
  return 0;
}
