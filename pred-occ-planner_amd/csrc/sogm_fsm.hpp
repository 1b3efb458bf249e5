// sogm_fsm.hpp — FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233), the rules of one tick of one
// agent, written ONCE for the host and the device: fsm_due (who plans in this tick, from which time) and fsm_step (the state
// update and what is published).  The kernels behind sogm_fsm_inputs / sogm_fsm_apply call them per agent; the host
// compiles them too (tests/fsm_rules_host_test.cpp).  Plain fp64 compares and single additions / subtractions: nothing a
// contraction could change.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_FSM_HD __host__ __device__
#else
#define SOGM_FSM_HD
#endif

#include "../../include/sogm_abi.h"

namespace sogm {

// FSM_STATUS as the tick driver numbers it (driver.py FSM_*); INIT and WAIT_TARGET are behind an agent that flies
enum : int32_t { FSM_NEW_PLAN = 0, FSM_EXEC_TRAJ = 1, FSM_REPLAN = 2, FSM_GOAL_REACHED = 3 };
enum : int32_t { FSM_DUE_NEW = 1, FSM_DUE_REPLAN = 2 };  // bits of FsmDue::bits

struct FsmDue {
  int32_t bits;     // FSM_DUE_NEW | FSM_DUE_REPLAN; 0: the agent does not plan in this tick
  double  t_start;  // the planning start time: now, or now + replan_start_time in REPLAN (:169-171)
};
struct FsmPub {
  int32_t kind;         // SOGM_FSM_PUB_NONE / _NEW / _HOVER
  double  hover_start;  // start time of the hover record (traj_start_time_ at publishEmptyTrajectory's call, :411); 0 otherwise
};

// Which states plan (:110-135, :164-175): NEW_PLAN once more than new_plan_interval has passed since traj_start (strict,
// checkTimeLapse), REPLAN always.
SOGM_FSM_HD inline FsmDue fsm_due(const SogmFsmState &s, double now, const SogmFsmParams &prm) {
  FsmDue     d;
  const bool is_rep = s.status == FSM_REPLAN;
  d.bits = 0;
  if (s.status == FSM_NEW_PLAN && (now - s.traj_start) > prm.new_plan_interval) d.bits |= FSM_DUE_NEW;
  if (is_rep) d.bits |= FSM_DUE_REPLAN;
  d.t_start = is_rep ? now + prm.replan_start_time : now;
  return d;
}

// One FSMCallback given the tick's results.  `due`: fsm_due's bits of this tick; `ok`: replan() returned true — it counts
// only where the agent was due (the reference does not call replan() otherwise); `safe` (isTrajSafe) and `reached`
// (isGoalReached) are consulted in EXEC_TRAJ only.  The blocks run in driver.fsm_apply's order — NEW_PLAN, REPLAN,
// EXEC_TRAJ — and each is chosen by the state the agent ENTERED the tick with, like the switch.
SOGM_FSM_HD inline FsmPub fsm_step(SogmFsmState &s, int32_t due, bool ok, bool safe, bool reached, double now,
                                   const SogmFsmParams &prm) {
  FsmPub        pub{SOGM_FSM_PUB_NONE, 0.0};
  const int32_t entered = s.status;
  ok = ok && due != 0;
  if (entered == FSM_NEW_PLAN) {  // :110-135
    if (due & FSM_DUE_NEW) {
      s.traj_start    = now;
      s.success       = ok ? 1 : 0;
      pub.kind        = ok ? SOGM_FSM_PUB_NEW : SOGM_FSM_PUB_HOVER;
      pub.hover_start = ok ? 0.0 : s.traj_start;
    }
    if (s.success) s.status = FSM_EXEC_TRAJ;  // the MEMBER is_success_, which REPLAN never writes
  } else if (entered == FSM_REPLAN) {  // :164-199
    const double t_rep = now + prm.replan_start_time;
    s.traj_start       = t_rep;
    if (ok) {
      s.fail   = 0;
      pub.kind = SOGM_FSM_PUB_NEW;
      s.status = FSM_EXEC_TRAJ;
    } else {
      s.fail += 1;
      if (s.fail > prm.replan_max_failures) {  // tested after the increment
        s.status        = FSM_NEW_PLAN;
        pub.kind        = SOGM_FSM_PUB_HOVER;  // published first, with traj_start_time_ = now + replan_start_time ...
        pub.hover_start = t_rep;
        s.traj_start    = now - 1.0;  // ... then "force new plan immediately" (:194; the reference's literal)
      }
    }
  } else if (entered == FSM_EXEC_TRAJ) {  // :137-162
    if ((now - s.traj_start) > prm.replan_duration || !safe) s.status = FSM_REPLAN;
    if (reached) s.status = FSM_GOAL_REACHED;  // tested last: a reached goal wins over the lapse
  }
  return pub;
}

}  // namespace sogm
