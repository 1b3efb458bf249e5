// Compiles against host/sogm_facade.hpp's TrajServer and positionCommandFields.  On the host: the message fields of a
// command, and the trajectory server's argument handling — refused arguments give SOGM_ERR_INVALID_ARG with a
// sogm_last_error text before anything is read, a well-formed call without a GPU is SOGM_ERR_NO_DEVICE.  With a GPU the
// facade flies one agent over a hover record for two ticks and hands its last command to sogm_camera_poses.
// Prints "trajserver facade host ok".
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sogm_facade.hpp"

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);  \
      ++fails;                                                 \
    }                                                          \
  } while (0)

int main() {
  static_assert(sizeof(SogmTrajServerParams) == 40 && sizeof(SogmTrajPoint) == 96 && sizeof(SogmPositionCommand) == 112 &&
                    sizeof(SogmTrajServerState) == 96 + sizeof(SogmTrajRecord),
                "layout");
  SogmPositionCommand c{};
  c.t_pub = 12.5, c.pos[0] = 1, c.pos[1] = 2, c.pos[2] = 3, c.vel[1] = -4, c.acc[2] = 5, c.yaw = 0.25, c.yaw_dot = -0.5;
  c.traj_id = 7, c.flags = SOGM_CMD_PUBLISHED;
  const sogm_host::PositionCommandFields f = sogm_host::positionCommandFields(c);
  EXPECT(f.publish && f.stamp == 12.5 && f.position[2] == 3 && f.velocity[1] == -4 && f.acceleration[2] == 5);
  EXPECT(f.yaw == 0.25 && f.yaw_dot == -0.5 && f.trajectory_id == 7 && f.trajectory_flag == 1);
  c.flags = 0;
  EXPECT(!sogm_host::positionCommandFields(c).publish);

  SogmTrajServerParams prm{0.5, 0.01, 3.14159265358979323846, 3.14159265358979323846, 1, 0};
  // stand-in addresses: every refusal below happens before anything is read
  auto *st  = reinterpret_cast<SogmTrajServerState *>(0x1000);
  auto *q   = reinterpret_cast<SogmTrajPoint *>(0x2000);
  auto *tab = reinterpret_cast<const SogmTrajRecord *>(0x3000);
  auto *cmd = reinterpret_cast<SogmPositionCommand *>(0x4000);
  auto *dp  = reinterpret_cast<double *>(0x5000);
  EXPECT(sogm_traj_server_run(nullptr, st, q, tab, nullptr, nullptr, 1, 1, 0, 1, 0.0, 0, 0.1, 0.0, cmd, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_traj_server_run") != nullptr);
  EXPECT(sogm_traj_server_run(&prm, st, q, tab, nullptr, nullptr, 65, 1, 0, 1, 0.0, 0, 0.1, 0.0, cmd, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_traj_server_run(&prm, st, q, tab, nullptr, nullptr, 1, 4, 2, 3, 0.0, 0, 0.1, 0.0, cmd, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_traj_server_run(&prm, st, q, tab, nullptr, nullptr, 1, 1, 0, 1, 0.0, 0, 0.105, 0.0, cmd, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  SogmTrajServerParams wide = prm;
  wide.replan_threshold = 1.28;
  EXPECT(sogm_traj_server_run(&wide, st, q, tab, nullptr, nullptr, 1, 1, 0, 1, 0.0, 0, 0.1, 0.0, cmd, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  SogmTrajServerParams mode = prm;
  mode.yaw_mode = 2;
  EXPECT(sogm_traj_server_run(&mode, st, q, tab, nullptr, nullptr, 1, 1, 0, 1, 0.0, 0, 0.1, 0.0, cmd, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_traj_server_init(st, q, 0, 0.0, dp, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  const double c2b[9] = {0, 0, 1, -1, 0, 0, 0, -1, 0}, off[3] = {0, 0, 0};
  EXPECT(sogm_camera_poses(cmd, 1, 0, c2b, off, dp, dp, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_camera_poses") != nullptr);
  if (sogm_device_count() == 0) {
    EXPECT(sogm_traj_server_run(&prm, st, q, tab, nullptr, nullptr, 1, 1, 0, 1, 0.0, 0, 0.1, 0.0, cmd, nullptr) ==
           SOGM_ERR_NO_DEVICE);
    EXPECT(sogm_traj_server_init(st, q, 1, 0.0, dp, nullptr, nullptr) == SOGM_ERR_NO_DEVICE);
    EXPECT(sogm_camera_poses(cmd, 1, 1, c2b, off, dp, dp, nullptr) == SOGM_ERR_NO_DEVICE);
  } else {
    // one agent hovering at (1, 2, 1.5) from t = 10: reset on arrival (50 samples), one more push at t = duration, then 19 pops
    SogmTrajRecord rec{};
    rec.n_pieces = 1, rec.time_start = 10.0, rec.duration[0] = 0.5;
    for (int k = 0; k < 5; ++k) rec.cpts[k * 3] = 1.0, rec.cpts[k * 3 + 1] = 2.0, rec.cpts[k * 3 + 2] = 1.5;
    const SogmTrajRecord two[2] = {rec, rec};
    const double         start[3] = {0.0, 0.0, 0.0}, yaw0 = 0.25;
    sogm_host::DevBuf<SogmTrajRecord> tables;
    sogm_host::DevBuf<double>         pos0, yaw, cam_pos(3), cam_rot(9);
    tables.put(two, 2);
    pos0.put(start, 3);
    yaw.put(&yaw0, 1);
    sogm_host::TrajServer srv(prm, 1, 7.0, pos0.data(), yaw.data());
    srv.run(tables.data(), 2, 1, nullptr, nullptr, 10.0, 0, 0.1, 0, 10);
    EXPECT(srv.commandsPerAgent() == 20);
    srv.cameraPoses(19, c2b, off, cam_pos.data(), cam_rot.data());
    const std::vector<SogmPositionCommand> got = srv.commands();
    EXPECT(got.size() == 20);
    for (const SogmPositionCommand &g : got) {
      EXPECT(g.flags == SOGM_CMD_PUBLISHED && g.traj_id == 1 && g.pos[0] == 1.0 && g.pos[1] == 2.0 && g.pos[2] == 1.5);
      EXPECT(g.yaw == 0.25 && g.yaw_dot == 0.0);   // zero velocity: the heading is held
    }
    EXPECT(got[19].t_pub == (10.0 + 1 * 0.1) + 9 * 0.01 && got[3].t_sample == 7.0 + (0.01 + 0.01 + 0.01));
    // (a reset stamps its samples with the start time of BEFORE the arrival, pushToTrajQueue :202: the trigger's 7.0)
    const std::vector<SogmTrajServerState> s = srv.states();
    EXPECT(s[0].core.traj_id == 1 && s[0].core.size == 31 && s[0].core.overflow == 0 && s[0].traj.n_pieces == 1);
    double p[3], r[9];
    cam_pos.get(p, 3);
    cam_rot.get(r, 9);
    EXPECT(p[0] == 1.0 && p[1] == 2.0 && p[2] == 1.5);
    EXPECT(std::fabs(r[2] - std::cos(0.25)) < 1e-15 && std::fabs(r[5] - std::sin(0.25)) < 1e-15 && r[7] == -1.0);
  }
  if (fails) return 1;
  std::printf("trajserver facade host ok\n");
  return 0;
}
