// sogm_fsm.hpp — FiniteStateMachine::FSMCallback (plan_manager/src/plan_manager.cpp:92-233), the rules of one tick of one
// agent, written ONCE for the host and the device: fsm_due (who plans in this tick, from which time) and fsm_step (the state
// update and what is published).  The kernels behind sogm_fsm_inputs / sogm_fsm_apply call them per agent; the host
// compiles them too (tests/fsm_rules_host_test.cpp).  Plain fp64 compares and single additions / subtractions: nothing a
// contraction could change.
// Below the rules, the per-agent bodies around them — fsm_inputs_agent (the head of a tick) and fsm_hover_record
// (publishEmptyTrajectory's record) — which the stand-alone kernels of sogm_fsm.hip and the flight's kernels
// (sogm_planner_set_flight_fsm: the head of k_flight_map, the finish of k_flight_light) both call; the host compiles these
// too (tests/flight_fsm_host_test.cpp).
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_FSM_HD __host__ __device__
#else
#define SOGM_FSM_HD
#endif

#include "../../include/sogm_abi.h"
#include "../../include/sogm_detmath.h"

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

// The head of one FSMCallback for one agent (k_fsm_inputs' lane, the admitting wave of a flight under the FSM mode): who
// plans and from when (fsm_due), the own record sampled at the stamp (where the agent is: map centre, hover point, goal
// test) and at the planning start time (the replan's start state, :169-175); an agent that executes nothing stands where it
// hovers (odom, :127-133).  `hov` is a COPY of the agent's hover row (the row itself is refreshed here); `eval(rec, t, out9)`
// is sogm_device.hpp's traj_eval_record on the device (a host caller brings its own reading of Bezier::getPos / Vel / Acc).
template <class Eval>
SOGM_FSM_HD inline void fsm_inputs_agent(const SogmFsmParams &prm, const SogmFsmState &s, const SogmTrajRecord &rec,
                                         const double *hov, const double *goal, int a, double stamp, double *hover,
                                         double *now, double *t_start, double *pva, float *poses, double *pos_now,
                                         int32_t *due, int32_t *reached, Eval eval) {
  const FsmDue d = fsm_due(s, stamp, prm);
  double       pn[9], o[9];
  if (!eval(rec, stamp, pn))
    for (int k = 0; k < 9; ++k) pn[k] = hov[k];
  if (!eval(rec, d.t_start, o))
    for (int k = 0; k < 9; ++k) o[k] = hov[k];
  for (int k = 0; k < 9; ++k) pva[a * 9 + k] = o[k];
  for (int k = 0; k < 3; ++k) {
    hover[a * 9 + k]     = pn[k];
    hover[a * 9 + 3 + k] = 0.0;
    hover[a * 9 + 6 + k] = 0.0;
    poses[a * 3 + k]     = (float)pn[k];
    pos_now[a * 3 + k]   = pn[k];
  }
  now[a]     = stamp;
  t_start[a] = d.t_start;
  due[a]     = d.bits;
  // isGoalReached: |position - goal| < goal_tolerance
  const double dx = pn[0] - goal[0], dy = pn[1] - goal[1], dz = pn[2] - goal[2];
  reached[a] = sogm_det::sqrt_rn((dx * dx + dy * dy) + dz * dz) < prm.goal_tolerance ? 1 : 0;
}

// publishEmptyTrajectory's record (plan_manager.cpp:404-424): one 0.5 s piece whose five control points sit at the agent's
// position `p`, start time `start`.  Lane `lane` of `n_lanes` writes its share of the words (a host caller: 0 of 1).
SOGM_FSM_HD inline void fsm_hover_record(SogmTrajRecord &r, int32_t drone_id, const double *p, double start, int lane,
                                         int n_lanes) {
  for (int i = lane; i < SOGM_MAX_PIECES; i += n_lanes) r.duration[i] = i == 0 ? 0.5 : 0.0;
  for (int i = lane; i < SOGM_MAX_PIECES * 15; i += n_lanes) r.cpts[i] = i < 15 ? p[i % 3] : 0.0;
  if (lane == 0) {
    r.drone_id   = drone_id;
    r.n_pieces   = 1;
    r.time_start = start;
  }
}

}  // namespace sogm
