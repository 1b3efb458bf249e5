// sogm_traj.hip — the trajectory-record kernels that need no context (the tick driver's glue around a replan):
//   k_traj_eval      Bezier pos / vel / acc of a record at an absolute time.   bernstein.cpp:25-59
//   k_tick_inputs    start of a tick: every agent's replan start state.        plan_manager.cpp:127-133,169-175
//   k_merge_latest   end of a tick: latest-wins per drone.                     particles.cpp:179-190
#include <hip/hip_runtime.h>

#include "sogm_planner.hpp"  // TickInputsIO, tick_inputs_agent, stage_record_hover

namespace sogm {

__global__ __launch_bounds__(64) void k_traj_eval(const SogmTrajRecord *__restrict__ rec, int n,
                                                  const double *__restrict__ t,
                                                  double *__restrict__ out, int32_t *__restrict__ ok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double o[9];
  ok[i] = traj_eval_record(rec[i], t[i], o) ? 1 : 0;
  for (int k = 0; k < 9; ++k) out[i * 9 + k] = o[k];
}

// Start of a replan tick for n agents in one launch (the tick driver's glue): the replan start state of every agent
// from the trajectory it is executing — FiniteStateMachine samples traj_ at the planned start time
// (plan_manager/src/plan_manager.cpp:169-175), an agent without a trajectory starts from where it hovers
// (odom, :127-133) — plus the stamps the map update and the replan take.
// One wave per agent: the 2064-byte record is fetched with ONE coalesced batch of loads into LDS (a lane walking
// n_pieces -> durations -> control points through global memory needs four dependent round trips, which the tail
// of the streaming clear beside this kernel stretches to a millisecond each), lane 0 evaluates it there.
__global__ __launch_bounds__(64) void k_tick_inputs(const SogmTrajRecord *__restrict__ own, int n, double stamp,
                                                    double start_offset, double *__restrict__ hover,
                                                    double *__restrict__ now, double *__restrict__ t_start,
                                                    double *__restrict__ pva, float *__restrict__ poses) {
  __shared__ __attribute__((aligned(16))) SogmTrajRecord s_rec;
  __shared__ double                                      s_hov[9];
  const int i = blockIdx.x;
  if (i >= n) return;
  const TickInputsIO io{.own = own, .hover = hover, .now = now, .t_start = t_start, .pva = pva, .start_offset = start_offset};
  stage_record_hover(&s_rec, s_hov, io.own, io.hover, i, threadIdx.x);
  if (threadIdx.x != 0) return;
  tick_inputs_agent(s_rec, s_hov, i, stamp, io, poses);
}

// End of a tick: latest-wins per drone (particles.cpp:179-190) — a successful replan replaces the agent's record,
// a failed one keeps the trajectory being executed (plan_manager.cpp:176-196); `all` (optional) is the swarm table of
// a single-process run, refreshed in the same pass.  One lane per 16 bytes of a record.
__global__ __launch_bounds__(256) void k_merge_latest(const SogmTrajRecord *__restrict__ fresh,
                                                      const int32_t *__restrict__ ok, SogmTrajRecord *__restrict__ own,
                                                      SogmTrajRecord *__restrict__ all, int n) {
  constexpr int W = (int)(sizeof(SogmTrajRecord) / 16);
  static_assert(sizeof(SogmTrajRecord) % 16 == 0, "record size");
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long long)n * W) return;
  const int a = (int)(gid / W), w = (int)(gid % W);
  // all three loads are issued together: this kernel often runs beside the tail of the streaming clear, where a
  // dependent global round trip costs a millisecond
  const int   good = ok[a];
  const uint4 vf = reinterpret_cast<const uint4 *>(fresh + a)[w], vo = reinterpret_cast<const uint4 *>(own + a)[w];
  const uint4 v  = good ? vf : vo;
  if (good) reinterpret_cast<uint4 *>(own + a)[w] = v;
  if (all) reinterpret_cast<uint4 *>(all + a)[w] = v;
}

}  // namespace sogm

using namespace sogm;

extern "C" {

int sogm_traj_eval(const SogmTrajRecord *records, int n, const double *t, double *out_pva,
                   int32_t *out_valid, void *stream) {
  if (!records || !t || !out_pva || !out_valid || n < 0) return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  hipLaunchKernelGGL(k_traj_eval, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, records, n,
                     t, out_pva, out_valid);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_tick_inputs(const SogmTrajRecord *own_records, int n, double stamp, double replan_start_offset,
                     double *hover_inout, double *out_now, double *out_t_start, double *out_pva, float *out_poses,
                     void *stream) {
  if (!own_records || !hover_inout || !out_now || !out_t_start || !out_pva || !out_poses || n < 0)
    return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  hipLaunchKernelGGL(k_tick_inputs, dim3(n), dim3(64), 0, (hipStream_t)stream, own_records, n, stamp,
                     replan_start_offset, hover_inout, out_now, out_t_start, out_pva, out_poses);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_merge_latest(const SogmTrajRecord *new_records, const int32_t *ok, SogmTrajRecord *own_inout,
                      SogmTrajRecord *all_or_null, int n, void *stream) {
  if (!new_records || !ok || !own_inout || n < 0) return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  const long long lanes = (long long)n * (long long)(sizeof(SogmTrajRecord) / 16);
  hipLaunchKernelGGL(k_merge_latest, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     new_records, ok, own_inout, all_or_null, n);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

}  // extern "C"
