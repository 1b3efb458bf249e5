// sogm_flight_light.hpp — the flight's worker kernel (sogm_flight_run; host side in sogm_flight.hip, the hand-overs in
// sogm_handover.hpp): k_flight_light, one-wave workgroups over one queue of corridor-segment and finish descriptors, with the
// per-agent FSM's two hooks around the finish, and launch_flight_light.  A corridor descriptor is corridor_slot
// (sogm_corridor.hpp), a finish descriptor finish_agent + finish_count (sogm_finish.hpp); what is written here is the queue,
// the FSM hooks and the tick's accounting.
//
// A kernel and its launcher in a header: this file is included by sogm_corridor.hip and by nothing else, i.e. compiled in the
// corridor stage's translation unit.  The compiler specialises corridor_slot and the bodies under it for the set of callers
// it sees in a unit before it inlines them; as a unit of its own, with k_flight_light their only caller, this kernel came out
// with another instruction schedule and register allocation all through its corridor branch (profiles/EXPERIMENTS.md).
#pragma once
#include <hip/hip_runtime.h>

#include "sogm_corridor.hpp"
#include "sogm_finish.hpp"
#include "sogm_fsm.hpp"

namespace sogm {

// The finish of a flight under the per-agent FSM (sogm_planner_set_flight_fsm), one wave, in two halves around finish_agent.
// Before it (finish_agent overwrites own[a]): BaselinePlanner::isTrajSafe of the record the agent executes against its
// complete map of this tick — traj_safe_agent, a lane per sample of the accumulated time sequence, the verdict is the AND.
__device__ inline int flight_fsm_traj_safe(const MapView &m, const FlightFsmDev &u, const FinishArgs &f, int a, int lane) {
  const int mine = traj_safe_agent(m, a, f.pub_own[a], f.swarm_now[a], u.check_duration, lane, 64);
  return __ballot(mine == 0) == 0ull ? 1 : 0;
}
// Behind it: sogm_fsm_apply for the agent — fsm_step on lane 0, the state back into the caller's record, the hover record
// (publishEmptyTrajectory) into own[a] and the agent's row of ver(k); SOGM_FSM_PUB_NEW needs nothing: due && ok publishes in
// both planning states and finish_agent has published — and the tick's row of the logs.
__device__ inline void flight_fsm_apply(const FlightFsmDev &u, const FinishArgs &f, int a, size_t row, bool ok, int safe,
                                        int lane) {
  const double stamp = f.swarm_now[a];
  int          kind  = 0;
  double       start = 0.0;
  if (lane == 0) {
    SogmFsmState  s       = u.state[a];
    const int32_t due     = u.due[a], reached = u.reached[a];
    const FsmPub  pub     = fsm_step(s, due, ok, safe != 0, reached != 0, stamp, u.prm);
    u.state[a]            = s;
    kind                  = pub.kind;
    start                 = pub.hover_start;
    if (u.log_state) u.log_state[row] = s;
    if (u.log_due) u.log_due[row] = due;
    if (u.log_safe) u.log_safe[row] = safe;
    if (u.log_reached) u.log_reached[row] = reached;
    if (u.log_pub) u.log_pub[row] = pub.kind;
    if (u.log_hover_start) u.log_hover_start[row] = pub.hover_start;
  }
  kind  = __shfl(kind, 0, 64);
  start = __shfl(start, 0, 64);
  if (kind == SOGM_FSM_PUB_HOVER) {  // (wave-uniform)
    const double p[3] = {u.pos_now[a * 3], u.pos_now[a * 3 + 1], u.pos_now[a * 3 + 2]};
    fsm_hover_record(f.pub_own[a], f.drone_ids[a], p, start, lane, 64);
    if (f.pub_table) fsm_hover_record(f.pub_table[a], f.drone_ids[a], p, start, lane, 64);
  }
  if (u.log_own) {  // what the agent executes after the tick: own[a] as this wave's lanes have just left it
    __threadfence();
    copy_record(u.log_own + row, f.pub_own + a, lane);
  }
}

// Flight kernel L (sogm_flight_run): role-less one-wave workgroups over the corridor + finish work queue.  A wave takes a
// ticket (one atomicAdd), waits for the descriptor at that position and does what it says.  WK_CORRIDOR: one of the 16
// segment slots of an agent whose search is done, as in k_worker_flow; the wave that completes the agent's last slot
// finalises its corridors and queues the QP.  WK_FINISH: finish_agent against table ver(k - 2), the record into ver(k) and
// the flight log, then the tick's accounting and the agent's next map head.  17 descriptors per (agent, tick).
__global__ __launch_bounds__(64) void k_flight_light(MapView m, SogmPlannerParams pp, CorridorWorkspace ws, FlightCtl fl,
                                                     FlightLightDev d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int      lane  = threadIdx.x;
  // ONE FIFO of 17 descriptors per agent-tick (16 corridor segments + the finish); a worker whose ticket lies beyond the
  // flight's last descriptor leaves at once.  (Tried at the end of round 5 and taken back: a second, priority queue for the
  // finishes — 50 us of work that end an agent's tick; in the FIFO they wait 0.1-0.2 ms behind corridor segments — which
  // every worker looked at first and whose descriptor count per queue is not known in advance, so that the idle workers
  // stayed resident until the call's end.  Single-process flights: records identical, finish 0.2 -> 0.05 ms per agent-tick,
  // tick 6.99 -> 6.83 ms.  The two-rank flight of tests/test_exchange_gpu.py (two-tick calls): from the second call on two
  // corridor segments per call stayed unprocessed for 3 s — with every exit rule tried (finished count, epoch word, both
  // queues' known totals), with the queue's head / tail never reset, and NOT with all but 64 of the idle workers leaving
  // early.  Unexplained; profiles/EXPERIMENTS.md.)
  const unsigned total = (unsigned)fl.n_agents * (unsigned)fl.n_ticks * (SOGM_MAX_PIECES + 1);
  int           *err   = &fl.hdr[FL_ERR];
  fl_wg_started(fl, 2);
  long long      c1_prev = 0;
  int            kind_prev = 0;
  for (;;) {
    const unsigned t = (unsigned)flow_ticket(&fl.hdr[FL_LW_HEAD]);
    if (t >= total) break;
    const long long c0   = wall_clock64();
    const int       desc = wq_take(fl.lw, t, err);
    if (desc < 0) break;
    __threadfence();
    const long long c1 = wall_clock64();
    if (lane == 0) {  // wave time by activity (sogm_flight_stats)
      if (c1_prev) {
        atomicAdd(&fl.prof[kind_prev == WK_FINISH ? 8 : 7], (unsigned long long)(c0 - c1_prev));
        atomicAdd(&fl.prof[kind_prev == WK_FINISH ? 15 : 14], 1ull);
      }
      atomicAdd(&fl.prof[6], (unsigned long long)(c1 - c0));
    }
    const int kind = wk_kind(desc), a = wk_agent(desc);
    c1_prev   = c1;
    kind_prev = kind;
    if (kind == WK_FINISH) {
      const int k  = fl.tick_of[a];
      const int kl = k - fl.first_tick;
      FinishArgs f = d.fin;
      f.swarm      = d.tables ? d.tables + (size_t)((k - fl.lag) & 3) * d.n_total : nullptr;
      f.swarm_stride = 0;  // the flight's tables are shared: no per-agent views
      f.pub_table  = d.tables ? d.tables + (size_t)(k & 3) * d.n_total + d.agent0 : nullptr;
      f.out        = d.log_records + (size_t)kl * fl.n_agents;
      f.out_ok     = d.log_ok + (size_t)kl * fl.n_agents;
      // the FSM mode (d.fsm.state set): isTrajSafe in front of finish_agent, the state update and the hover record behind it
      int traj_safe = 1;
      if (d.fsm.state) traj_safe = flight_fsm_traj_safe(m, d.fsm, f, a, lane);
      const int code = finish_agent(f, a, LpLds::carve(smem), lane);
      if (d.fsm.state) flight_fsm_apply(d.fsm, f, a, (size_t)kl * fl.n_agents + a, (code & 2) != 0, traj_safe, lane);
      __syncthreads();
      __threadfence();  // the record (own, ver(k), log) is out before the tick counts as finished
      if (lane == 0) {
        const long long now = wall_clock64();
        long long      *ts  = fl.ts + (size_t)a * FL_TS, *acc = fl.acc + (size_t)a * 8;
        ts[6]               = now;
        acc[0] += ts[14] - ts[10];                       // gate wait: the overlay parked behind the finished marks
        acc[1] += (ts[11] - ts[7]) - (ts[14] - ts[10]);  // map: from the head's publication to the complete map, less that
        acc[2] += ts[1] - ts[11];                      // search queue + A*
        acc[3] += ts[3] - ts[1];                       // corridor queue + corridors
        acc[4] += ts[5] - ts[3];                       // QP queue + QP
        acc[5] += now - ts[5];                         // finish queue + finish
        acc[6] += now - ts[7];                         // the whole chain
        acc[7] += 1;
        if (fl.ts_log) {
          long long *lg = fl.ts_log + ((size_t)kl * fl.n_agents + a) * FL_TS;
          for (int q = 0; q < FL_TS; ++q) lg[q] = ts[q];
        }
        finish_count(f, a, (code & 1) != 0);
        // The gate of the staleness rule — tick j reads table ver(j - 2), so every agent must have finished tick j - 2 — sits
        // in FRONT OF THE OVERLAY, the only phase of a map that reads the table (k_flight_map): an agent goes on to its next
        // map head at once and builds reset / bits / marks while it waits; the overlay of a map that reaches the gate early
        // is PARKED there, not queued, and the finish that completes the awaited tick queues the parked overlays.  (First
        // version: the whole head parked at the gate.  A gate then released a burst of 20-60 heads into the admission order
        // and the map workers at once, and the laggards arriving just then — the very agents the next gate waits for —
        // queued behind it: parked + admission + map 1.9 ms per tick of the flight's critical path.)
        const int A_      = fl.n_agents;
        const int done_kl = __hip_atomic_fetch_add(&fl.tick_done[kl], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1;
        if (atomicAdd(&fl.hdr[FL_FINISHED], 1) + 1 == A_ * fl.n_ticks)  // the call's last agent-tick: the map kernel's waves may go
          __hip_atomic_store(&fl.hdr[FL_END], fl.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (kl + 1 < fl.n_ticks) {  // the agent's next tick: its map head, now
          fl.tick_of[a] = k + 1;
          ts[7]         = now;
          // one of the last finishers of its tick: its next map goes through the urgent lane
          const bool urgent = fl.n_urgent > 0 && done_kl > A_ - fl.n_urgent;
          fl.urgent[a]      = urgent ? 1 : 0;
          fl_publish(urgent ? fl.u_ring : fl.m_ring, fl.ring_mask, &fl.hdr[urgent ? FL_U_READY : FL_M_READY], a);
        }
        // tick k is complete: the overlays of tick k + 2 parked so far may go.  (Several ranks with the exchange behind the
        // call: the gate is the all-gather of ver(k), and the kernel behind that collective releases them — k_flight_xsignal.)
        if (done_kl == A_ && kl + fl.lag < fl.n_ticks && !fl.xready) fl_gate_release(fl, kl + fl.lag);
      }
      continue;
    }
    // ---- WK_CORRIDOR: segment slot `seg` of agent a ----
    const int seg = wk_sub(desc);
    if (seg == 0 && lane == 0) fl.ts[a * FL_TS + 2] = wall_clock64();
    // diagnostics (sogm_debug_corridor_stats, tools/soak_flight.py): when this slot's descriptor was taken, its obstacle points
    // were out, its segment was done, and on which compute unit (HW_ID | XCC_ID << 32)
    long long *sdbg = ws.seg_dbg + ((size_t)a * SOGM_MAX_PIECES + seg) * 16;
    if (lane == 0) {
      sdbg[12] = c1;
      sdbg[13] = 0;
      sdbg[14] = 0;
      sdbg[15] = (long long)(unsigned)__builtin_amdgcn_s_getreg(63492) | ((long long)(unsigned)__builtin_amdgcn_s_getreg(63508) << 32);
    }
    if (corridor_slot(m, pp, ws, d.cor, a, seg, smem, fl.seg_done, true, sdbg)) {
      if (lane == 0) {
        fl.ts[a * FL_TS + 3] = wall_clock64();
        fl_publish(fl.q_ring, fl.ring_mask, &fl.hdr[FL_Q_READY], a);
      }
    }
    __syncthreads();
  }
}

hipError_t launch_flight_light(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws, const FlightCtl &fl,
                               const FlightLightDev &d, int n_workgroups, hipStream_t st) {
  hipLaunchKernelGGL(k_flight_light, dim3(n_workgroups), dim3(64), SegmentLds<6>::bytes(pp.pc_capacity), st, m, pp, ws, fl, d);
  return hipGetLastError();
}

}  // namespace sogm
