// The per-agent bodies of csrc/sogm_fsm.hpp that the stand-alone FSM kernels and the flight under the FSM
// (sogm_planner_set_flight_fsm) share — fsm_inputs_agent (the head of a tick) and fsm_hover_record (publishEmptyTrajectory's
// record) — on the host, no GPU: ONE agent flown through them by tick lines read from standard input.
// tests/test_flight_fsm_host.py feeds it the agents of tests/golden/fsm_independent.json and compares every printed line.
//   usage: flight_fsm_host_test traj_start0 replan_duration replan_start_time replan_max_failures
//          flight_fsm_host_test layout          (prints sizeof / offsetof of SogmFlightFsm and SOGM_ABI_VERSION)
//   in:    now ok safe reached                  (one tick per line; ok = what replan() would return)
//   out:   due t_start reached | status fail traj_start pub [hover_start] | n_pieces time_start x y z
// The agent's records here are one-piece records whose control points coincide (a hover record, or a "new" record at a
// point of its own), for which Bezier::getPos is that point at any time: the evaluator handed to fsm_inputs_agent says so
// and the device's traj_eval_record is not needed.  Exit codes 3.. name the check that failed.
#include "sogm_fsm.hpp"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool eval_point_record(const SogmTrajRecord &r, double, double *o) {
  for (int k = 0; k < 9; ++k) o[k] = 0.0;
  if (r.n_pieces <= 0) return false;
  for (int k = 0; k < 3; ++k) o[k] = r.cpts[k];
  return true;
}

int main(int argc, char **argv) {
  if (argc == 2 && std::strcmp(argv[1], "layout") == 0) {
    std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(SogmFlightFsm), offsetof(SogmFlightFsm, prm),
                offsetof(SogmFlightFsm, check_duration), offsetof(SogmFlightFsm, state_inout),
                offsetof(SogmFlightFsm, log_state), offsetof(SogmFlightFsm, log_due), offsetof(SogmFlightFsm, log_safe),
                offsetof(SogmFlightFsm, log_reached), offsetof(SogmFlightFsm, log_pub),
                offsetof(SogmFlightFsm, log_hover_start), offsetof(SogmFlightFsm, log_own), SOGM_ABI_VERSION);
    return 0;
  }
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s traj_start0 replan_duration replan_start_time replan_max_failures | layout\n", argv[0]);
    return 2;
  }
  SogmFsmParams prm{};
  prm.replan_duration     = std::atof(argv[2]);
  prm.replan_start_time   = std::atof(argv[3]);
  prm.goal_tolerance      = 1.0;
  prm.new_plan_interval   = 1.0;
  prm.replan_max_failures = std::atoi(argv[4]);
  // two agents' arrays; the one under test is row 1 (the functions index their outputs by the agent)
  constexpr int A = 2, a = 1;
  SogmFsmState  s{std::atof(argv[1]), sogm::FSM_NEW_PLAN, 0, 0, 0};
  static SogmTrajRecord own{};  // executes nothing yet
  double  hover[A * 9] = {0}, now_o[A] = {0}, t_start[A] = {0}, pva[A * 9] = {0}, pos_now[A * 3] = {0};
  float   poses[A * 3] = {0};
  int32_t due[A] = {-1, -1}, reached_o[A] = {-1, -1};
  hover[a * 9 + 0] = 1.25, hover[a * 9 + 1] = -2.5, hover[a * 9 + 2] = 0.75;
  hover[a * 9 + 4] = 9.0;  // (a stale velocity: the refreshed row has none)
  static const char *const names[4] = {"NEW_PLAN", "EXEC_TRAJ", "REPLAN", "GOAL_REACHED"};
  double now;
  int    ok, safe, reached, tick = 0;
  while (std::scanf("%lf %d %d %d", &now, &ok, &safe, &reached) == 4) {
    ++tick;
    double hov[9], where[3];
    for (int k = 0; k < 9; ++k) hov[k] = hover[a * 9 + k];
    for (int k = 0; k < 3; ++k) where[k] = own.n_pieces > 0 ? own.cpts[k] : hov[k];
    // a goal inside the tolerance exactly when the fixture says the agent has arrived
    const double goal[3] = {where[0] + (reached ? 0.6 : 7.0), where[1] - (reached ? 0.6 : 3.0), where[2]};
    sogm::fsm_inputs_agent(prm, s, own, hov, goal, a, now, hover, now_o, t_start, pva, poses, pos_now, due, reached_o,
                           eval_point_record);
    if (due[0] != -1 || reached_o[0] != -1 || now_o[0] != 0.0 || hover[0] != 0.0) return 3;  // row 0 is not this agent's
    if (now_o[a] != now || reached_o[a] != reached) return 4;
    for (int k = 0; k < 3; ++k) {
      if (pos_now[a * 3 + k] != where[k] || pva[a * 9 + k] != where[k] || hover[a * 9 + k] != where[k]) return 5;
      if (poses[a * 3 + k] != (float)where[k] || hover[a * 9 + 3 + k] != 0.0 || hover[a * 9 + 6 + k] != 0.0) return 6;
    }
    const sogm::FsmDue d = sogm::fsm_due(s, now, prm);
    if (due[a] != d.bits || t_start[a] != d.t_start) return 7;
    const sogm::FsmPub pub = sogm::fsm_step(s, due[a], ok != 0, safe != 0, reached != 0, now, prm);
    if (pub.kind == SOGM_FSM_PUB_NEW) {  // the tick's new record: a point of its own, from the planning start time
      const double p[3] = {where[0] + 0.25, where[1] + 0.125 * tick, where[2]};
      sogm::fsm_hover_record(own, 7, p, t_start[a], 0, 1);
    } else if (pub.kind == SOGM_FSM_PUB_HOVER) {
      // as 64 lanes would write it: every lane its share, in any order
      std::memset(&own, 0xA5, sizeof(own));
      for (int lane = 63; lane >= 0; --lane) sogm::fsm_hover_record(own, 7, &pos_now[a * 3], pub.hover_start, lane, 64);
      if (own.drone_id != 7 || own.n_pieces != 1 || own.time_start != pub.hover_start || own.duration[0] != 0.5) return 8;
      for (int i = 1; i < SOGM_MAX_PIECES; ++i)
        if (own.duration[i] != 0.0) return 9;
      for (int i = 0; i < SOGM_MAX_PIECES * 15; ++i)
        if (own.cpts[i] != (i < 15 ? pos_now[a * 3 + i % 3] : 0.0)) return 10;
    }
    std::printf("%d %.17g %d | ", due[a], t_start[a], reached_o[a]);
    if (pub.kind == SOGM_FSM_PUB_HOVER)
      std::printf("%s %d %.17g hover %.17g", names[s.status], s.fail, s.traj_start, pub.hover_start);
    else
      std::printf("%s %d %.17g %s", names[s.status], s.fail, s.traj_start, pub.kind == SOGM_FSM_PUB_NEW ? "new" : "none");
    std::printf(" | %d %.17g %.17g %.17g %.17g\n", own.n_pieces, own.time_start, own.cpts[0], own.cpts[1], own.cpts[2]);
  }
  return 0;
}
