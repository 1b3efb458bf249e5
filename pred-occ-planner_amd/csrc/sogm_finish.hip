// sogm_finish.hip — the end of a replan in all its forms: isSafeAfterOpt and the record / outcome count of every agent.
// Grouped path (sogm_replan, pipelining mode 1, and the per-stage entry sogm_safe_after_opt): k_fill_i32 + k_safe_after_opt
// (launch_deconflict), then k_pack_records.  Dataflow replan: the finishing blocks of k_worker_flow (sogm_corridor.hip), which
// do both per agent as its QP finishes.  The flight's finish is the WK_FINISH branch of k_flight_light (sogm_flight_light.hpp).  All of them
// share the device bodies and the outcome rule of sogm_finish.hpp.
// Test hook (sogm_finish_batched, include/sogm_abi_debug.h): both forms on a FinishArgs the caller injects — the grouped
// launchers as they are, or k_finish_wave, finish_agent + finish_count per agent without the dataflow's hand-over control.
#include <hip/hip_runtime.h>

#include "sogm_finish.hpp"

namespace sogm {

// grouped path: one workgroup per (other agent's record, ego agent), see deconflict_pair_unsafe
__global__ __launch_bounds__(64) void k_safe_after_opt(const double *__restrict__ cpts,
                                                       const int32_t *__restrict__ npoly,
                                                       const SogmTrajRecord *__restrict__ rec, int n_rec,
                                                       const int32_t *__restrict__ ego_ids,
                                                       const double *__restrict__ t_now,
                                                       int32_t *__restrict__ out_safe, int agent0,
                                                       unsigned long long *counters, int rec_stride) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int a = blockIdx.y + agent0, i = blockIdx.x;
  // (rec_stride 0: one table; n_rec: agent a's own view, rec[a][.])
  if (deconflict_pair_unsafe(cpts + (size_t)a * SOGM_MAX_PIECES * 15, npoly[a], rec[(size_t)a * rec_stride + i], ego_ids[a], t_now[a],
                             LpLds::carve(s_dyn), counters) &&
      threadIdx.x == 0)
    out_safe[a] = 0;  // every writer writes 0
}

__global__ void k_fill_i32(int32_t *p, int n, int32_t v, int agent0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[agent0 + i] = v;
}

// The finishing wave alone (sogm_finish_batched with SOGM_FINISH_WAVE): one one-wave workgroup per agent runs what
// k_worker_flow and k_flight_light inline for an agent, with no ticket, ready list or hand-over around it.
__global__ __launch_bounds__(64) void k_finish_wave(FinishArgs f) {
  extern __shared__ __attribute__((aligned(16))) double s_dyn[];
  const int a = blockIdx.x, lane = threadIdx.x;
  const int code = finish_agent(f, a, LpLds::carve(s_dyn), lane);
  if (lane == 0) finish_count(f, a, (code & 1) != 0);
}

// The grouped path's end of a replan, behind launch_qp and (with a swarm) launch_deconflict, one thread per agent: the count
// of where it ended and the BezierTraj record of a successful replan (plan_manager/src/plan_manager.cpp:364-399 publishes
// duration[] and cpts[]); n_pieces = 0 marks "replan() returned false".
__global__ void k_pack_records(int A, FinishArgs f, int agent0) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x + agent0;
  if (a >= A) return;
  const int  npoly = f.npoly[a];
  const bool safe  = f.swarm ? f.out_safe[a] != 0 : true;  // (launch_deconflict ran in front of this kernel only with a swarm)
  // isSafeAfterOpt false -> replan() returns false (baseline_fake.cpp:455-460)
  const int  outcome = replan_outcome(f.ret[a], npoly, f.status[a], safe);
  const bool good    = outcome == SOGM_CNT_REPLAN_OK;
  // (an agent sogm_planner_set_due's mask left out was not asked to plan: it is not counted)
  if (f.counters && !(f.due && f.due[a] == 0)) atomicAdd(&f.counters[outcome], 1ull);
  SogmTrajRecord &r = f.out[a];
  r.drone_id        = f.drone_ids[a];
  r.time_start      = f.t_start[a];
  r.n_pieces        = good ? npoly : 0;
  for (int i = 0; i < SOGM_MAX_PIECES; ++i) r.duration[i] = (good && i < npoly) ? f.corridor_tau : 0.0;
  for (int i = 0; i < SOGM_MAX_PIECES * 15; ++i)
    r.cpts[i] = (good && i < npoly * 15) ? f.cpts[(size_t)a * SOGM_MAX_PIECES * 15 + i] : 0.0;
  f.out_ok[a] = good ? 1 : 0;
  if (f.pub_own) {  // publication, as the dataflow replan's finishers do it (sogm_planner_set_publish)
    if (good) f.pub_own[a] = r;
    if (f.pub_table) f.pub_table[a] = f.pub_own[a];
  }
}

hipError_t launch_deconflict(int n_agents, const double *cpts, const int32_t *npoly, const SogmTrajRecord *rec,
                             int n_rec, const int32_t *ego_ids, const double *t_now, int32_t *out_safe,
                             hipStream_t st, int agent0, unsigned long long *counters, int rec_stride) {
  hipLaunchKernelGGL(k_fill_i32, dim3((n_agents + 63) / 64), dim3(64), 0, st, out_safe, n_agents, 1, agent0);
  if (n_rec > 0)
    hipLaunchKernelGGL(k_safe_after_opt, dim3(n_rec, n_agents), dim3(64), LpLds::bytes(), st, cpts, npoly, rec, n_rec,
                       ego_ids, t_now, out_safe, agent0, counters, rec_stride);
  return hipGetLastError();
}

hipError_t launch_pack_records(int n_agents, const FinishArgs &f, hipStream_t st, int agent0) {
  hipLaunchKernelGGL(k_pack_records, dim3((n_agents + 63) / 64), dim3(64), 0, st, agent0 + n_agents, f, agent0);
  return hipGetLastError();
}

}  // namespace sogm

extern "C" int sogm_finish_batched(sogm_planner *counters_of, double corridor_tau, const int32_t *ret, const int32_t *npoly,
                                   const int32_t *status, const double *cpts, const SogmTrajRecord *swarm, int n_swarm,
                                   const int32_t *swarm_ego, const double *swarm_now, const double *t_start,
                                   const int32_t *drone_ids, const int32_t *due, int n, SogmTrajRecord *out, int32_t *out_ok,
                                   int32_t *out_safe, SogmTrajRecord *pub_own, SogmTrajRecord *pub_table, int flags,
                                   void *stream) {
  if ((flags & ~SOGM_FINISH_WAVE) || n < 0 || n > (1 << 20) || n_swarm < 0 ||
      (n > 0 && (!ret || !npoly || !status || !cpts || !t_start || !drone_ids || !out || !out_ok || !out_safe)) ||
      (n > 0 && swarm && (!swarm_ego || !swarm_now)))
    return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  if (!swarm) n_swarm = 0;
  hipStream_t            st = (hipStream_t)stream;
  const sogm::FinishArgs f{.corridor_tau = corridor_tau, .ret = ret, .npoly = npoly, .status = status, .cpts = cpts,
                           .swarm = swarm, .n_swarm = n_swarm, .swarm_ego = swarm_ego, .swarm_now = swarm_now,
                           .t_start = t_start, .drone_ids = drone_ids, .out = out, .out_ok = out_ok, .out_safe = out_safe,
                           .counters = counters_of ? counters_of->cw.counters : nullptr, .pub_own = pub_own,
                           .pub_table = pub_table, .due = due};
  if (flags & SOGM_FINISH_WAVE) {
    hipLaunchKernelGGL(sogm::k_finish_wave, dim3(n), dim3(64), sogm::LpLds::bytes(), st, f);
    return launched("sogm_finish_batched k_finish_wave", hipGetLastError());
  }
  if (swarm)
    if (int rc = launched("sogm_finish_batched launch_deconflict",
                          sogm::launch_deconflict(n, cpts, npoly, swarm, n_swarm, swarm_ego, swarm_now, out_safe, st, 0,
                                                  f.counters)))
      return rc;
  return launched("sogm_finish_batched launch_pack_records", sogm::launch_pack_records(n, f, st, 0));
}
