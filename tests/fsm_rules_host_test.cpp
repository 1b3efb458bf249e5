// The FSM rules of csrc/sogm_fsm.hpp (fsm_due / fsm_step) on the host, no GPU: one agent's machine driven by tick lines
// read from standard input — tests/test_fsm_rules_host.py feeds it the agents of tests/golden/fsm_independent.json and
// compares every printed line.
//   usage: fsm_rules_host_test traj_start0 replan_duration replan_start_time replan_max_failures
//   in:    now ok safe reached                            (one tick per line; ok = what replan() would return)
//   out:   status fail traj_start pub [hover_start]       (after the tick; doubles as %.17g; pub none | new | hover)
#include "sogm_fsm.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv) {
  if (argc != 5) {
    std::fprintf(stderr, "usage: %s traj_start0 replan_duration replan_start_time replan_max_failures\n", argv[0]);
    return 2;
  }
  static_assert(sizeof(SogmFsmState) == 24, "SogmFsmState is 24 bytes");
  SogmFsmParams prm{};
  prm.replan_duration     = std::atof(argv[2]);
  prm.replan_start_time   = std::atof(argv[3]);
  prm.goal_tolerance      = 1.0;
  prm.new_plan_interval   = 1.0;
  prm.replan_max_failures = std::atoi(argv[4]);
  SogmFsmState s{std::atof(argv[1]), sogm::FSM_NEW_PLAN, 0, 0, 0};
  static const char *const names[4] = {"NEW_PLAN", "EXEC_TRAJ", "REPLAN", "GOAL_REACHED"};
  double now;
  int    ok, safe, reached;
  while (std::scanf("%lf %d %d %d", &now, &ok, &safe, &reached) == 4) {
    const sogm::FsmDue due = sogm::fsm_due(s, now, prm);
    // the planning start time is the state's own rule: now, or now + replan_start_time in REPLAN
    if (due.t_start != ((due.bits & sogm::FSM_DUE_REPLAN) ? now + prm.replan_start_time : now)) return 3;
    const sogm::FsmPub pub = sogm::fsm_step(s, due.bits, ok != 0, safe != 0, reached != 0, now, prm);
    if (s.status < 0 || s.status > 3) return 4;
    if (pub.kind == SOGM_FSM_PUB_HOVER)
      std::printf("%s %d %.17g hover %.17g\n", names[s.status], s.fail, s.traj_start, pub.hover_start);
    else
      std::printf("%s %d %.17g %s\n", names[s.status], s.fail, s.traj_start, pub.kind == SOGM_FSM_PUB_NEW ? "new" : "none");
  }
  return 0;
}
