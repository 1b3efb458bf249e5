// The trajectory server's serial bodies (csrc/sogm_trajserver.hpp: trajsrv_receive / trajsrv_timer) on the host, with a plain
// C++ evaluator.  Reads one case on stdin (tests/test_traj_server_independent.py writes it from
// tests/golden/traj_server_independent.json), drives the callbacks as sogm_traj_server_run orders them and prints every
// command, the queue size after every event, the final state and the live queue, doubles with 17 significant digits.
//   P replan_threshold sample_dt yaw_pi yaw_dot_max yaw_mode
//   I t_trigger init_yaw x y z
//   T t0 first_tick period receive_delay n_ticks m
//   per tick:  N   |   R n_pieces time_start duration[n_pieces] cpts[n_pieces * 15]
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_trajserver.hpp"

// Bezier::getPos / getVel / getAcc at a trajectory time clamped to [0, total] (sogm_traj_eval's arithmetic)
static bool eval_record(const SogmTrajRecord &r, double tt, double *out) {
  double total = 0;
  for (int k = 0; k < r.n_pieces; ++k) total += r.duration[k];
  tt = tt < 0 ? 0 : (tt > total ? total : tt);
  int    piece = r.n_pieces - 1;
  double rem   = tt;
  for (int k = 0; k < r.n_pieces; ++k) {
    rem -= r.duration[k];
    if (rem < 0) {
      piece = k;
      break;
    }
  }
  double t0 = 0;
  for (int k = 0; k < piece; ++k) t0 += r.duration[k];
  const double tf = t0 + r.duration[piece], dur = tf - t0, s = (tt - t0) / dur;
  const double A[5][5] = {{1, -4, 6, -4, 1}, {0, 4, -12, 12, -4}, {0, 0, 6, -12, 6}, {0, 0, 0, 4, -4}, {0, 0, 0, 0, 1}};
  const double S0[5] = {1, s, s * s, s * s * s, (s * s) * (s * s)};
  const double S1[5] = {0, 1, 2 * s, 3 * (s * s), 4 * (s * s * s)};
  const double S2[5] = {0, 0, 2, 6 * s, 12 * (s * s)};
  const double *c    = r.cpts + piece * 15;
  for (int d = 0; d < 3; ++d) {
    double p = 0, v = 0, a = 0;
    for (int j = 0; j < 5; ++j) {
      double b = 0;
      for (int q = 0; q < 5; ++q) b += c[q * 3 + d] * A[q][j];
      p += b * S0[j];
      v += b * S1[j];
      a += b * S2[j];
    }
    out[d]     = p;
    out[3 + d] = v / dur;
    out[6 + d] = a / (dur * dur);
  }
  return true;
}

static void print_cmd(const SogmPositionCommand &c, int size) {
  std::printf("C %.17g %.17g", c.t_pub, c.t_sample);
  for (int d = 0; d < 3; ++d) std::printf(" %.17g", c.pos[d]);
  for (int d = 0; d < 3; ++d) std::printf(" %.17g", c.vel[d]);
  for (int d = 0; d < 3; ++d) std::printf(" %.17g", c.acc[d]);
  std::printf(" %.17g %.17g %d %d %d\n", c.yaw, c.yaw_dot, c.traj_id, c.flags, size);
}

int main() {
  SogmTrajServerParams prm{};
  double               t_trigger, init_yaw, t0, period, receive_delay;
  int                  first_tick, n_ticks, m;
  std::vector<SogmTrajServerState> state(1);   // heap: the sanitizers watch its bounds
  std::vector<SogmTrajPoint>       ring(SOGM_TRAJSRV_QUEUE);
  std::memset(state.data(), 0, sizeof(SogmTrajServerState));
  std::memset(ring.data(), 0, sizeof(SogmTrajPoint) * SOGM_TRAJSRV_QUEUE);
  SogmTrajServerState &s = state[0];
  if (std::scanf(" P %lf %lf %lf %lf %d", &prm.replan_threshold, &prm.sample_dt, &prm.yaw_pi, &prm.yaw_dot_max,
                 &prm.yaw_mode) != 5)
    return 2;
  if (std::scanf(" I %lf %lf %lf %lf %lf", &t_trigger, &init_yaw, &s.core.init_pos[0], &s.core.init_pos[1],
                 &s.core.init_pos[2]) != 5)
    return 2;
  if (std::scanf(" T %lf %d %lf %lf %d %d", &t0, &first_tick, &period, &receive_delay, &n_ticks, &m) != 6) return 2;
  s.core.ts = s.core.te = t_trigger;
  s.core.last_yaw       = init_yaw;
  std::vector<SogmTrajRecord> recv(1);
  SogmTrajRecord &rec = recv[0];
  for (int k = 0; k < n_ticks; ++k) {
    char kind;
    if (std::scanf(" %c", &kind) != 1) return 2;
    bool rcv = false;
    if (kind == 'R') {
      std::memset(&rec, 0, sizeof(rec));
      if (std::scanf("%d %lf", &rec.n_pieces, &rec.time_start) != 2 || rec.n_pieces < 1 || rec.n_pieces > SOGM_MAX_PIECES)
        return 2;
      for (int i = 0; i < rec.n_pieces; ++i)
        if (std::scanf("%lf", &rec.duration[i]) != 1) return 2;
      for (int i = 0; i < rec.n_pieces * 15; ++i)
        if (std::scanf("%lf", &rec.cpts[i]) != 1) return 2;
      rcv = true;
    }
    const double t_k = t0 + (double)(first_tick + k) * period, t_rcv = t_k + receive_delay;
    int          j_rcv = 0;
    while (j_rcv < m && t_k + (double)j_rcv * prm.sample_dt < t_rcv) ++j_rcv;
    for (int j = 0; j <= m; ++j) {
      if (j == j_rcv && rcv) {
        sogm::trajsrv_receive(prm, s, ring.data(), rec, t_rcv, eval_record);
        std::printf("E %d\n", s.core.size);
      }
      if (j < m) {
        SogmPositionCommand cmd;
        sogm::trajsrv_timer(prm, s, ring.data(), t_k + (double)j * prm.sample_dt, eval_record, cmd);
        print_cmd(cmd, s.core.size);
      }
    }
  }
  const SogmTrajServerCore &c = s.core;
  std::printf("S %.17g %.17g %.17g %.17g %.17g %d %d %d %d\n", c.ts, c.te, c.duration, c.last_yaw, c.last_yawdot, c.size,
              c.traj_id, c.received, c.overflow);
  for (int i = 0; i < c.size; ++i) {
    const SogmTrajPoint &p = ring[(c.head + i) & sogm::TRAJSRV_MASK];
    std::printf("Q %.17g %.17g %.17g\n", p.t, p.yaw, p.yaw_dot);
  }
  return 0;
}
