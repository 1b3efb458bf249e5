// sogm_fsm.hip — FiniteStateMachine::FSMCallback on the device (plan_manager/src/plan_manager.cpp:92-233): the per-agent
// state records and the two launches of a tick, sogm_fsm_inputs in front of the map update and sogm_fsm_apply behind
// sogm_replan.  The rules are sogm_fsm.hpp's (fsm_due / fsm_step); here are their inputs, the publication and the entries.
#include <hip/hip_runtime.h>

#include "sogm_device.hpp"
#include "sogm_fsm.hpp"

using namespace sogm;

static_assert(sizeof(SogmFsmState) == 24, "SogmFsmState is 24 bytes (sogm_abi.h)");
static_assert(sizeof(SogmFsmParams) == 40, "SogmFsmParams (sogm_abi.h)");
static_assert(sizeof(SogmTrajRecord) == 8 * (2 + SOGM_MAX_PIECES + SOGM_MAX_PIECES * 15) && sizeof(SogmTrajRecord) % 16 == 0,
              "a record is {id, pieces}, time_start, duration[], cpts[]: 8-byte words, copied 16 bytes per lane");

__global__ __launch_bounds__(64) void k_fsm_init(SogmFsmState *__restrict__ state, int n, double traj_start0) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  state[a] = SogmFsmState{traj_start0, FSM_NEW_PLAN, 0, 0, 0};
}

// The head of the tick, one lane per agent: who plans and from when (fsm_due), the own record sampled at the stamp (where
// the agent is: map centre, hover point, goal test) and at the planning start time (the replan's start state, :169-175);
// an agent that executes nothing stands where it hovers (odom, :127-133).
__global__ __launch_bounds__(64) void k_fsm_inputs(SogmFsmParams prm, const SogmFsmState *__restrict__ state,
                                                   const SogmTrajRecord *__restrict__ own, const double *__restrict__ goals,
                                                   int n, double stamp, double *__restrict__ hover, double *__restrict__ now,
                                                   double *__restrict__ t_start, double *__restrict__ pva,
                                                   float *__restrict__ poses, double *__restrict__ pos_now,
                                                   int32_t *__restrict__ due, int32_t *__restrict__ reached) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  double hov[9];
  for (int k = 0; k < 9; ++k) hov[k] = hover[a * 9 + k];
  fsm_inputs_agent(prm, state[a], own[a], hov, goals + a * 3, a, stamp, hover, now, t_start, pva, poses, pos_now, due, reached,
                   [](const SogmTrajRecord &r, double t, double *o) { return traj_eval_record(r, t, o); });
}

// The rest of the tick, one wave per agent: lane 0 runs fsm_step, then the wave publishes — the tick's new record
// (plan_manager.cpp:364-399), or publishEmptyTrajectory's (:404-424: one 0.5 s piece whose five control points sit at the
// agent's position), or nothing: the agent goes on executing own[a].
__global__ __launch_bounds__(64) void k_fsm_apply(SogmFsmParams prm, SogmFsmState *__restrict__ state,
                                                  const int32_t *__restrict__ due, const int32_t *__restrict__ ok,
                                                  const int32_t *__restrict__ safe, const int32_t *__restrict__ reached,
                                                  const SogmTrajRecord *__restrict__ fresh,
                                                  const int32_t *__restrict__ drone_ids, const double *__restrict__ pos_now,
                                                  SogmTrajRecord *__restrict__ own, int32_t *__restrict__ out_pub,
                                                  double *__restrict__ out_hover_start, int n, double stamp) {
  const int a = blockIdx.x, lane = threadIdx.x;
  if (a >= n) return;
  __shared__ int    s_kind;
  __shared__ double s_start;
  if (lane == 0) {
    SogmFsmState s   = state[a];
    const FsmPub pub = fsm_step(s, due[a], ok[a] != 0, safe[a] != 0, reached[a] != 0, stamp, prm);
    state[a]           = s;
    out_pub[a]         = pub.kind;
    out_hover_start[a] = pub.hover_start;
    s_kind             = pub.kind;
    s_start            = pub.hover_start;
  }
  __syncthreads();
  const int kind = s_kind;  // (wave-uniform)
  if (kind == SOGM_FSM_PUB_NEW) {
    copy_record(own + a, fresh + a, lane);
  } else if (kind == SOGM_FSM_PUB_HOVER) {
    const double p[3] = {pos_now[a * 3], pos_now[a * 3 + 1], pos_now[a * 3 + 2]};
    fsm_hover_record(own[a], drone_ids[a], p, s_start, lane, 64);
  }
}

extern "C" {

int sogm_fsm_init(SogmFsmState *state, int n, double traj_start0, void *stream) {
  if (!state || n < 0) return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  hipLaunchKernelGGL(k_fsm_init, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, n, traj_start0);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_fsm_inputs(const SogmFsmParams *prm, const SogmFsmState *state, const SogmTrajRecord *own_records,
                    const double *goals, int n, double stamp, double *hover_inout, double *out_now, double *out_t_start,
                    double *out_pva, float *out_poses, double *out_pos_now, int32_t *out_due, int32_t *out_reached,
                    void *stream) {
  if (!prm || !state || !own_records || !goals || !hover_inout || !out_now || !out_t_start || !out_pva || !out_poses ||
      !out_pos_now || !out_due || !out_reached || n < 0)
    return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  hipLaunchKernelGGL(k_fsm_inputs, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, *prm, state, own_records, goals,
                     n, stamp, hover_inout, out_now, out_t_start, out_pva, out_poses, out_pos_now, out_due, out_reached);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_fsm_apply(const SogmFsmParams *prm, SogmFsmState *state_inout, const int32_t *due, const int32_t *ok,
                   const int32_t *safe, const int32_t *reached, const SogmTrajRecord *new_records,
                   const int32_t *drone_ids, const double *pos_now, SogmTrajRecord *own_inout, int32_t *out_pub,
                   double *out_hover_start, int n, double stamp, void *stream) {
  if (!prm || !state_inout || !due || !ok || !safe || !reached || !new_records || !drone_ids || !pos_now || !own_inout ||
      !out_pub || !out_hover_start || n < 0)
    return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  hipLaunchKernelGGL(k_fsm_apply, dim3(n), dim3(64), 0, (hipStream_t)stream, *prm, state_inout, due, ok, safe, reached,
                     new_records, drone_ids, pos_now, own_inout, out_pub, out_hover_start, n, stamp);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

}  // extern "C"
