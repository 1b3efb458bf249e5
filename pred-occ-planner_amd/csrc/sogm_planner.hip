// sogm_planner.hip — planner context and host side of the planner entry points: the per-stage calls (search,
// corridors, QP, deconfliction) and sogm_replan in its two forms — the dataflow replan (replan_flow: five launches,
// persistent corridor / QP / finish kernels chained per agent through ready lists) and the grouped-stream chain
// (replan_impl) — with the flow's one-lane glue kernels (k_flow_gate, k_flow_reset, k_flow_report).  The stages' kernels are
// in their own units: sogm_astar.hip, sogm_corridor.hip, sogm_qp.hip, and the end of a replan (isSafeAfterOpt, records,
// outcome counters) in sogm_finish.hip.  The flight (sogm_flight_run) is in sogm_flight.hip.  SOGM_ERR_STATE from an entry point means a call-order error (no map update before planning).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "sogm_planner.hpp"
#include "sogm_qp_layout.hpp"

using namespace sogm;

// Per-piece min-jerk cost  QM = p2j^T [[I/3, I/6],[I/6, I/3]] p2j  with p2j = a2j v2a p2v
// (traj_opt/src/bezier_optimizer.cpp:64-111; N = 4, DIM = 3).  Host-side, once per planner.
static void min_jerk_block(double *QM /*15x15*/) {
  // derivative-of-control-points operators act per dimension: rows (i,d), cols (j,d)
  auto diff = [](int rows, double scale, double *out, int cols) {
    for (int i = 0; i < rows * cols; ++i) out[i] = 0.0;
    for (int i = 0; i < rows / 3; ++i)
      for (int d = 0; d < 3; ++d) {
        out[(i * 3 + d) * cols + i * 3 + d]       = -scale;
        out[(i * 3 + d) * cols + (i + 1) * 3 + d] = scale;
      }
  };
  double p2v[12 * 15], v2a[9 * 12], a2j[6 * 9], p2a[9 * 15], p2j[6 * 15], W[6 * 6], T[6 * 15];
  diff(12, 4, p2v, 15);
  diff(9, 3, v2a, 12);
  diff(6, 2, a2j, 9);
  auto mul = [](const double *A, const double *B, double *C, int r, int k, int c) {
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < c; ++j) {
        double s = 0;
        for (int q = 0; q < k; ++q) s += A[i * k + q] * B[q * c + j];
        C[i * c + j] = s;
      }
  };
  mul(v2a, p2v, p2a, 9, 12, 15);
  mul(a2j, p2a, p2j, 6, 9, 15);
  for (int i = 0; i < 36; ++i) W[i] = 0.0;
  for (int d = 0; d < 3; ++d) {
    W[d * 6 + d]           = 1.0 / 3;
    W[d * 6 + 3 + d]       = 1.0 / 6;
    W[(3 + d) * 6 + d]     = 1.0 / 6;
    W[(3 + d) * 6 + 3 + d] = 1.0 / 3;
  }
  mul(W, p2j, T, 6, 6, 15);
  for (int i = 0; i < 15; ++i)
    for (int j = 0; j < 15; ++j) {
      double s = 0;
      for (int q = 0; q < 6; ++q) s += p2j[q * 15 + i] * T[q * 15 + j];
      QM[i * 15 + j] = s;
    }
}

namespace sogm {
// residency gate of the dataflow replan: returns when every A* workgroup has started (see k_astar)
__global__ void k_flow_gate(FlowCtl fc, int expected) {
  if (threadIdx.x != 0) return;
  wait_at_least<WaitResidencyGate, false>(&fc.hdr[FLOW_ERR], &fc.hdr[FLOW_A_RESIDENT], expected);
}

hipError_t launch_flow_gate(const FlowCtl &fc, int expected, hipStream_t st) {
  hipLaunchKernelGGL(k_flow_gate, dim3(1), dim3(64), 0, st, fc, expected);
  return hipGetLastError();
}
}  // namespace sogm

// End of a dataflow replan (one lane, on the caller's stream after the fan-in): a wait of this tick timed out ->
// remember the code and count the tick in pinned host memory, so the host can see failed ticks without a device
// synchronisation (sogm_planner_flow_failures).
__global__ void k_flow_report(const int *__restrict__ hdr, int *__restrict__ host_words, int *__restrict__ epoch_word,
                              long long *__restrict__ tick_clock) {
  if (tick_clock) tick_clock[1] = wall_clock64();  // the tick's last kernel (sogm_tick_clock)
  // the replan is over: the wide launch of the side-stream clear retires (sogm_ctx::clear_epoch_word), so that the
  // one-wave glue kernels between two replans (latest-wins merge, tick inputs, the stamp) find the memory pipeline
  // responsive; the narrow launch goes on
  if (epoch_word) *epoch_word = 0;
  const int e = hdr[FLOW_ERR];
  if (e != 0) {
    host_words[0] = e;
    host_words[1] = host_words[1] + 1;
  }
}

extern "C" {

// Everything sogm_planner_create acquires, all or nothing (Resources::Setup): an error return leaves nothing allocated.
static int planner_acquire(sogm_planner *p) {
  sogm_ctx                *map = p->map;
  const SogmPlannerParams *pp  = &p->pp;
  const int                A   = map->n_agents;
  sogm::Resources::Setup   setup(p->res);
  // two pools / hash tables per agent: the replan's second search attempt runs speculatively beside the first
  SOGM_HIP_CHECK(p->res.device(&p->aw.pool, p->aw.pool_stride * A * 2));
  SOGM_HIP_CHECK(p->res.device(&p->aw.hkeys, 8 * (size_t)p->aw.hash_cap * A * 2));
  SOGM_HIP_CHECK(p->res.device(&p->aw.verdict, sizeof(int) * A));
  SOGM_HIP_CHECK(p->res.device(&p->aw.dbg, sizeof(long long) * 8 * A, true));
  SOGM_HIP_CHECK(p->res.device(&p->d_ret, sizeof(int32_t) * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_route_len, sizeof(int32_t) * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_stats, sizeof(int32_t) * 4 * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_route, sizeof(double) * 6 * p->route_cap * A));
  const size_t slots = (size_t)A * SOGM_MAX_PIECES, cap = (size_t)pp->pc_capacity;
  SOGM_HIP_CHECK(p->res.device(&p->cw.pc, sizeof(double) * slots * cap * 3));
  SOGM_HIP_CHECK(p->res.device(&p->cw.fpc, sizeof(double) * slots * cap * 3));
  SOGM_HIP_CHECK(p->res.device(&p->cw.tang, sizeof(double) * slots * cap * 4));
  SOGM_HIP_CHECK(p->res.device(&p->cw.distr, sizeof(double) * slots * cap));
  SOGM_HIP_CHECK(p->res.device(&p->cw.polys, sizeof(double) * slots * pp->max_faces * 4));
  SOGM_HIP_CHECK(p->res.device(&p->cw.seg_nfaces, sizeof(int32_t) * slots));
  SOGM_HIP_CHECK(p->res.device(&p->cw.seg_state, sizeof(int32_t) * slots));
  SOGM_HIP_CHECK(p->res.device(&p->cw.seg_npts, sizeof(int32_t) * slots));
  // (slots no segment ever ran in are read by sogm_debug_corridor_stats as well: zero, not whatever the allocation held)
  SOGM_HIP_CHECK(p->res.device(&p->cw.seg_dbg, sizeof(long long) * 16 * slots, true));
  SOGM_HIP_CHECK(p->res.device(&p->cw.counters, sizeof(unsigned long long) * SOGM_CNT_N, true));
  // eager adjacent-pair LPs: ready words and verdict rows in one block (one reset range), their counters, the bookkeeping's stamps
  SOGM_HIP_CHECK(p->res.device(&p->cw.seg_ready, sizeof(int32_t) * sogm::corridor_pair_words(A), true));
  p->cw.pair_ok = reinterpret_cast<int32_t *>(p->cw.seg_ready) + A;
  SOGM_HIP_CHECK(p->res.device(&p->cw.pair_cnt, sizeof(unsigned long long) * 4, true));
  SOGM_HIP_CHECK(p->res.device(&p->cw.fin_dbg, sizeof(long long) * 4 * (size_t)A, true));
  // QP row storage fallback (rows normally live in LDS)
  p->qw.scratch_stride = qp_scratch_bytes_per_agent(pp->max_faces);
  p->qw.dyn_lds_bytes  = qp_kernel_setup();  // 160 KiB/CU minus the QP kernels' static LDS, granted on this device
  SOGM_HIP_CHECK(p->res.device(&p->qw.scratch, p->qw.scratch_stride * (size_t)A));
  SOGM_HIP_CHECK(p->res.device(&p->qw.k1_scratch, qp_k1_scratch_bytes_per_agent() * (size_t)A));
  SOGM_HIP_CHECK(p->res.device(&p->qw.dbg, sizeof(long long) * SOGM_QP_STAT_N * (size_t)A, true));
  SOGM_HIP_CHECK(p->res.device(&p->d_polys, sizeof(double) * slots * pp->max_faces * 4));
  SOGM_HIP_CHECK(p->res.device(&p->d_goal, sizeof(double) * 6 * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_cpts, sizeof(double) * slots * 15));
  SOGM_HIP_CHECK(p->res.device(&p->d_nfaces, sizeof(int32_t) * slots));
  SOGM_HIP_CHECK(p->res.device(&p->d_npoly, sizeof(int32_t) * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_status, sizeof(int32_t) * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_iters, sizeof(int32_t) * A));
  SOGM_HIP_CHECK(p->res.device(&p->d_safe, sizeof(int32_t) * A));
  // (the group streams themselves are created by the grouped path's first replan: the dataflow path never uses them,
  // and every stream is a hardware queue the process holds — INTEGRATION.md section 2 on sharing a GPU)
  for (int g = 0; g < p->n_groups; ++g) {
    SOGM_HIP_CHECK(p->res.event(&p->ev_corr[g]));
    SOGM_HIP_CHECK(p->res.event(&p->ev_pts[g]));
    SOGM_HIP_CHECK(p->res.event(&p->ev_done[g]));
  }
  SOGM_HIP_CHECK(p->res.event(&p->ev_in));
  // dataflow replan: control block and events.  Its two streams are created by the first dataflow replan (flow_streams):
  // with the caller's stream and the context's `side` the default tick keeps four streams busy — ROCm's default number of
  // hardware queues — and holds no others (the pre-stamp's own stream and the dense clear's wide part make a fifth)
  SOGM_HIP_CHECK(p->res.device(&p->d_flow, sizeof(int) * FlowBlock::words(A), true));
  FlowBlock::carve(p->d_flow, A, &p->fc);
  SOGM_HIP_CHECK(p->res.event(&p->ev_pdone));
  // [A][8] chain stamps, then [A][4] pre-stamp stamps (record seen, cull done, bits done, marks done)
  SOGM_HIP_CHECK(p->res.device(&p->d_flow_ts, sizeof(long long) * 12 * (size_t)A, true));
  p->fc.ts = p->d_flow_ts;
  SOGM_HIP_CHECK(p->res.event(&p->ev_records));
  SOGM_HIP_CHECK(p->res.event(&p->ev_wdone));
  SOGM_HIP_CHECK(p->res.event(&p->ev_qdone));
  SOGM_HIP_CHECK(p->res.event(&p->ev_gate));
  SOGM_HIP_CHECK(p->res.device(&p->d_epoch, sizeof(int), true));
  SOGM_HIP_CHECK(p->res.pinned(&p->h_flow_fail, sizeof(int) * 2, hipHostMallocMapped));
  p->h_flow_fail[0] = p->h_flow_fail[1] = 0;
  // (the memsets above are null-stream operations: complete before any kernel on the planner's non-blocking streams)
  SOGM_HIP_CHECK(hipStreamSynchronize(nullptr));
  return setup.done();
}

int sogm_planner_create(sogm_ctx *map, const SogmAstarParams *astar, const SogmPlannerParams *pp,
                        const SogmQpSettings *qp, sogm_planner **out) {
  if (!map || !astar || !pp || !qp || !out) return SOGM_ERR_INVALID_ARG;
  // The QP's register-resident path assumes every velocity / acceleration row is two-sided (rho = rho_cur or 1000 rho_cur):
  // "unbounded" limits (OSQP_INFTY-like values) would give those rows RHO_MIN and a K that does not match
  if (!(pp->opt_max_vel > 0 && pp->opt_max_vel < 1e20) || !(pp->opt_max_acc > 0 && pp->opt_max_acc < 1e20))
    return SOGM_ERR_INVALID_ARG;
  if (astar->allocate_num < 2 || astar->allocate_num > astar_pool_max() || astar->check_num < 1 || !(astar->resolution > 0) ||
      !(astar->time_resolution > 0))
    return SOGM_ERR_INVALID_ARG;
  if (pp->max_faces < 6 || pp->max_faces > 64 || pp->pc_capacity < 1 || pp->pc_capacity > 16384 || pp->firi_iterations < 1)
    return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(map->device));
  sogm_planner *p = new (std::nothrow) sogm_planner();  // (value-initialised: every field without an initialiser is zero)
  if (!p) return SOGM_ERR_INVALID_ARG;
  p->map = map;
  p->ap  = *astar;
  p->pp  = *pp;
  // BaselinePlanner searches with RiskHybridAstar, FakeBaselinePlanner with FakeRiskHybridAstar: the classes
  // differ in the shot check only (risk_hybrid_a_star.cpp:514 vs fake_risk_hybrid_a_star.cpp:521)
  p->ap.shot_ignores_time = pp->fake_planner ? 0 : 1;
  p->qs  = *qp;
  const int A = map->n_agents;
  int       hc = 1;
  while (hc < 2 * astar->allocate_num) hc <<= 1;
  p->aw.hash_cap    = hc;
  p->aw.pool_stride = astar_node_bytes() * (size_t)astar->allocate_num;
  p->route_cap      = 64;
  min_jerk_block(p->qc.QM);
  // Streams beyond the number of hardware queues (ROCm default GPU_MAX_HW_QUEUES = 4) share a queue
  // and serialise, so the default is 2 groups; the Python driver raises both (GPU_MAX_HW_QUEUES = 32 before HIP
  // initialises, sogm_set_tuning "groups" = 8 before it creates the planner).
  {
    int ng = map->tune_i(SOGM_TUNE_GROUPS);
    if (ng < 1) ng = 1;
    if (ng > SOGM_MAX_GROUPS) ng = SOGM_MAX_GROUPS;
    p->n_groups = A < ng ? A : ng;
  }
  p->sel_first   = 0;
  p->sel_count   = A;
  p->search_mode = 0;
  {
    p->spec_astar = map->tune_i(SOGM_TUNE_SPEC_ASTAR) != 0;
    // the second attempts wait on the first ones: only when every workgroup of both is resident at once
    if (p->spec_astar && 2 * A > sogm::astar_resident_workgroups(map->device)) p->spec_astar = 0;
  }
  {
    const char *ef = getenv("SOGM_FLOW");  // (one of the library's three environment switches)
    p->flow        = ef ? atoi(ef) != 0 : 1;
  }
  if (int rc = planner_acquire(p)) {
    delete p;
    return rc;
  }
  if (p->flow) {  // the map's pooled clear follows this planner's "corridors final" counter (sogm_device.hpp)
    map->clear_gate        = p->fc.hdr + FLOW_Q_READY_N;
    map->clear_gate_err    = p->fc.hdr + FLOW_ERR;
    map->clear_gate_target = A;
    {  // tuning aid: open the wide clear at a fraction of A
      const double f = map->tune[SOGM_TUNE_CLEAR_GATE_FRAC];
      if (f > 0.0 && f < 1.0) map->clear_gate_target = (int)(f * A + 0.5) < 1 ? 1 : (int)(f * A + 0.5);
    }
    map->clear_epoch_word  = p->d_epoch;
  }
  *out = p;
  return SOGM_OK;
}
void sogm_planner_destroy(sogm_planner *p) {
  if (!p) return;
  // (the planner's map must still exist: sogm_abi.h "destroy planners before their sogm_ctx")
  if (p->map) (void)hipSetDevice(p->map->device);
  if (p->map && p->map->ps_fail_host == p->h_flow_fail) p->map->ps_fail_host = nullptr;
  if (p->map && p->map->pdone_pending && p->map->ev_pdone == p->ev_pdone) {
    (void)hipDeviceSynchronize();  // a pre-stamp nobody joined: its event and progress words go away with this planner
    p->map->pdone_pending = 0;
    p->map->ps_stage = p->map->ps_err = nullptr;
  }
  if (p->map && p->d_epoch && p->map->clear_epoch_word == p->d_epoch) {
    (void)hipDeviceSynchronize();  // a gate kernel may still be polling this planner's words
    p->map->clear_gate = p->map->clear_gate_err = p->map->clear_epoch_word = nullptr;
  }
  p->res.release_all();
  delete p;
}

int sogm_astar_search(sogm_planner *p, const double *start_pva, const double *goal,
                      const double *t_start, int32_t *out_ret, double *out_route,
                      int32_t *out_route_len, int route_cap, int32_t *out_stats,
                      int32_t *out_trace, int trace_cap, void *stream) {
  if (!p || !start_pva || !goal || !t_start || !out_ret || !out_route || !out_route_len ||
      !out_stats || route_cap < 2)
    return SOGM_ERR_INVALID_ARG;
  if (!p->map->updated) return SOGM_ERR_STATE;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc0 = sogm::join_update(p->map, st)) return rc0;
  const sogm::SearchIO io{.start_pva = start_pva, .goal = goal, .t_start = t_start, .out_ret = out_ret,
                          .out_route = out_route, .out_route_len = out_route_len, .route_cap = route_cap,
                          .out_stats = out_stats};
  prof_begin(p->map, SOGM_PROF_ASTAR, st);
  const hipError_t e = launch_astar(view_of(p->map), p->ap, p->pp.corridor_tau, astar_ws(p), p->sel_count, io, out_trace,
                                    out_trace ? trace_cap : 0, st, p->sel_first, nullptr, p->search_mode);
  prof_end(p->map, SOGM_PROF_ASTAR, st);
  return launched("k_astar", e);
}
int sogm_corridor_generate(sogm_planner *p, const double *start_pva, const double *t_start,
                           const double *route, const int32_t *route_len, int route_cap,
                           double *out_polys, int32_t *out_nfaces, int32_t *out_npoly,
                           double *out_goal, void *stream) {
  if (!p || !start_pva || !t_start || !route || !route_len || !out_polys || !out_nfaces ||
      !out_npoly || !out_goal || route_cap < 2)
    return SOGM_ERR_INVALID_ARG;
  if (!p->map->updated) return SOGM_ERR_STATE;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc0 = sogm::join_update(p->map, st)) return rc0;
  const sogm::CorridorIO io{.start_pva = start_pva, .t_start = t_start, .route = route, .route_len = route_len,
                            .route_cap = route_cap, .out_polys = out_polys, .out_nfaces = out_nfaces,
                            .out_npoly = out_npoly, .out_goal = out_goal};
  prof_begin(p->map, SOGM_PROF_CORRIDOR, st);
  const hipError_t e = launch_corridor(view_of(p->map), p->pp, p->cw, p->sel_count, io, st, p->sel_first);
  prof_end(p->map, SOGM_PROF_CORRIDOR, st);
  return launched("k_corridor", e);
}
// diagnostics (tools/ only): per-agent A* phase ticks
int sogm_debug_astar_stats(sogm_planner *p, long long *out_host) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->aw.dbg, sizeof(long long) * 8 * (size_t)p->map->n_agents,
                           hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics (tools/ only): raw 128-byte node records of one agent's last search through sogm_astar_search (the
// replan's speculative second attempt keeps its nodes in the second half of the pool)
int sogm_debug_astar_nodes(sogm_planner *p, int agent, void *out_host, int n) {
  if (!p || !out_host || agent < 0 || agent >= p->map->n_agents || n < 0) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->aw.pool + (size_t)agent * p->aw.pool_stride, (size_t)n * sogm::astar_node_bytes(),
                           hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics: per-agent clock split of the last QP solve (QpWorkspace::dbg), [A][SOGM_QP_STAT_N]
int sogm_debug_qp_stats(sogm_planner *p, long long *out_host) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->qw.dbg, sizeof(long long) * SOGM_QP_STAT_N * (size_t)p->map->n_agents,
                           hipMemcpyDeviceToHost));
  return SOGM_OK;
}
// diagnostics: the QP kernels' memory plan for one problem as the host's description (sogm_qp_layout.hpp) gives it; no GPU work
int sogm_debug_qp_layout(sogm_planner *p, int n_pieces, const int32_t *nfaces_host, long long *out8) {
  if (!p || !nfaces_host || !out8 || n_pieces < 1 || n_pieces > SOGM_MAX_PIECES) return SOGM_ERR_INVALID_ARG;
  int faces = 0;
  for (int i = 0; i < n_pieces; ++i) {
    if (nfaces_host[i] < 0 || nfaces_host[i] > p->pp.max_faces) return SOGM_ERR_INVALID_ARG;
    faces += nfaces_host[i];
  }
  const sogm::QpLayout L(sogm::QpShape(n_pieces, faces), (size_t)p->qw.dyn_lds_bytes);
  const long long      out[8] = {L.fast, L.rows_in_lds, p->qw.dyn_lds_bytes, (long long)L.lds_bytes(), (long long)L.scratch_bytes(),
                                 L.fast && L.rows_in_lds, L.sh.G, L.sh.S};
  std::memcpy(out8, out, sizeof(out));
  return SOGM_OK;
}

// diagnostics (tools/ only): copy the per-segment corridor counters to the host
int sogm_debug_corridor_stats(sogm_planner *p, long long *out_host) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->cw.seg_dbg,
                           sizeof(long long) * 16 * (size_t)p->map->n_agents * SOGM_MAX_PIECES,
                           hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics: the adjacent-pair LPs' counters since the last call and what is set in the ready words / verdict rows now
int sogm_debug_corridor_pairs(sogm_planner *p, unsigned long long *out4) {
  if (!p || !out4) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out4, p->cw.pair_cnt, sizeof(unsigned long long) * 4, hipMemcpyDeviceToHost));
  SOGM_HIP_CHECK(hipMemset(p->cw.pair_cnt, 0, sizeof(unsigned long long) * 4));
  std::vector<uint32_t> words(sogm::corridor_pair_words(p->map->n_agents));
  SOGM_HIP_CHECK(hipMemcpy(words.data(), p->cw.seg_ready, sizeof(uint32_t) * words.size(), hipMemcpyDeviceToHost));
  for (const uint32_t w : words) out4[3] |= w;
  return SOGM_OK;
}
// diagnostics (tools/ only): [A][4] wall_clock64 of every agent's last bookkeeping in the dataflow replan or the flight
// (CorridorWorkspace::fin_dbg: start, adjacent pairs done, goal LPs done, copy done)
int sogm_debug_corridor_finalize_times(sogm_planner *p, long long *out_host) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->cw.fin_dbg, sizeof(long long) * 4 * (size_t)p->map->n_agents, hipMemcpyDeviceToHost));
  return SOGM_OK;
}

int sogm_bezier_qp_solve(sogm_planner *p, const double *start_pva, const double *goal_pv,
                         const double *polys, const int32_t *nfaces, const int32_t *npoly,
                         double *out_cpts, int32_t *out_status, int32_t *out_iters, void *stream) {
  if (!p || !start_pva || !goal_pv || !polys || !nfaces || !npoly || !out_cpts || !out_status ||
      !out_iters)
    return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  hipStream_t st = (hipStream_t)stream;
  const sogm::QpIO io{.start_pva = start_pva, .goal_pv = goal_pv, .polys = polys, .nfaces = nfaces, .npoly = npoly,
                      .out_cpts = out_cpts, .out_status = out_status, .out_iters = out_iters};
  prof_begin(p->map, SOGM_PROF_QP, st);
  sogm::QpWorkspace qw0 = p->qw;
  qw0.ablate            = p->map->tune_i(SOGM_TUNE_QP_ABLATE);
  const hipError_t e    = launch_qp(p->pp, p->qs, qw0, p->qc, p->sel_count, io, st, p->sel_first);
  prof_end(p->map, SOGM_PROF_QP, st);
  return launched("k_qp", e);
}
int sogm_bezier_qp_solve_timed(sogm_planner *p, const double *start_pva, const double *end_pva,
                               const double *time_alloc, double max_vel, double max_acc, const double *polys,
                               const int32_t *nfaces, const int32_t *npoly, double *out_cpts, int32_t *out_status,
                               int32_t *out_iters, void *stream) {
  if (!p || !start_pva || !end_pva || !time_alloc || !polys || !nfaces || !npoly || !out_cpts || !out_status ||
      !out_iters || !(max_vel > 0 && max_vel < 1e20) || !(max_acc > 0 && max_acc < 1e20))
    return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  hipStream_t       st = (hipStream_t)stream;
  SogmPlannerParams pp = p->pp;
  pp.opt_max_vel       = max_vel;
  pp.opt_max_acc       = max_acc;
  sogm::QpWorkspace qw = p->qw;
  qw.t_alloc           = time_alloc;
  qw.goal_stride       = 9;
  const sogm::QpIO io{.start_pva = start_pva, .goal_pv = end_pva, .polys = polys, .nfaces = nfaces, .npoly = npoly,
                      .out_cpts = out_cpts, .out_status = out_status, .out_iters = out_iters};
  prof_begin(p->map, SOGM_PROF_QP, st);
  const hipError_t e = launch_qp(pp, p->qs, qw, p->qc, p->sel_count, io, st, p->sel_first);
  prof_end(p->map, SOGM_PROF_QP, st);
  return launched("k_qp", e);
}
static int safe_after_opt(sogm_planner *p, const double *cpts, const int32_t *npoly, const SogmTrajRecord *records,
                          int n_records, const int32_t *ego_ids, const double *t_now, int32_t *out_safe, bool per_agent,
                          void *stream) {
  if (!p || !cpts || !npoly || !ego_ids || !t_now || !out_safe || n_records < 0 || (n_records > 0 && !records))
    return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  if (int rc = sogm::join_exchange(p->map, (hipStream_t)stream)) return rc;
  return launched("sogm_safe_after_opt", sogm::launch_deconflict(p->sel_count, cpts, npoly, records, n_records, ego_ids,
                                                                t_now, out_safe, (hipStream_t)stream, p->sel_first, nullptr,
                                                                per_agent ? n_records : 0));
}
int sogm_safe_after_opt(sogm_planner *p, const double *cpts, const int32_t *npoly,
                        const SogmTrajRecord *records, int n_records, const int32_t *ego_ids,
                        const double *t_now, int32_t *out_safe, void *stream) {
  return safe_after_opt(p, cpts, npoly, records, n_records, ego_ids, t_now, out_safe, false, stream);
}
int sogm_safe_after_opt_views(sogm_planner *p, const double *cpts, const int32_t *npoly, const SogmTrajRecord *views,
                              int n_records, const int32_t *ego_ids, const double *t_now, int32_t *out_safe, void *stream) {
  return safe_after_opt(p, cpts, npoly, views, n_records, ego_ids, t_now, out_safe, true, stream);
}

int sogm_planner_select_agents(sogm_planner *p, int first, int count) {
  if (!p || first < 0 || count < 1 || first + count > p->map->n_agents) return SOGM_ERR_INVALID_ARG;
  p->sel_first = first;
  p->sel_count = count;
  return SOGM_OK;
}
int sogm_planner_set_search_mode(sogm_planner *p, int mode) {
  if (!p || mode < 0 || (mode & ~(3 | 4 | 16)) != 0 || (mode & 3) == 3) return SOGM_ERR_INVALID_ARG;
  p->search_mode = mode;
  return SOGM_OK;
}

// diagnostics (tools/ only): the dataflow control block, copied on a private stream while the tick's kernels run
int sogm_debug_flow_peek(sogm_planner *p, int *out_host, int n) {
  if (!p || !out_host || n < 0) return SOGM_ERR_INVALID_ARG;
  if (!p->peek) SOGM_HIP_CHECK(p->res.stream(&p->peek));
  hipStream_t peek = p->peek;
  const int nf = FlowBlock(p->map->n_agents).gen;  // (everything in front of the generation word)
  SOGM_HIP_CHECK(hipMemcpyAsync(out_host, p->d_flow, sizeof(int) * (size_t)(n < nf ? n : nf), hipMemcpyDeviceToHost, peek));
  if (n > nf)  // followed by d_safe (progress markers in debug builds)
    SOGM_HIP_CHECK(hipMemcpyAsync(out_host + nf, p->d_safe, sizeof(int) * (size_t)(n - nf), hipMemcpyDeviceToHost, peek));
  SOGM_HIP_CHECK(hipStreamSynchronize(peek));
  return SOGM_OK;
}

// diagnostics: streams the context's and the planner's Resources hold now (host-side count, no HIP call)
int sogm_debug_streams_held(sogm_planner *p) {
  if (!p || !p->map) return SOGM_ERR_INVALID_ARG;
  return p->map->res.streams_held() + p->res.streams_held();
}

// diagnostics (tools/ only): per-agent stage timestamps of the last dataflow replan, [A][8] ticks of 10 ns
int sogm_debug_flow_times(sogm_planner *p, long long *out_host) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->d_flow_ts, sizeof(long long) * 8 * (size_t)p->map->n_agents, hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics (tools/ only): the internal stage outputs of the last sogm_replan, copied to the host.  which: 0 polytopes
// [A][16][max_faces][4] f64, 1 faces per polytope [A][16] i32, 2 polytopes per agent [A] i32, 3 local goal [A][6] f64,
// 4 route [A][route_cap][6] f64, 5 route length [A] i32, 6 control points [A][16 * 15] f64, 7 QP iterations [A] i32,
// 8 QP status [A] i32, 9 search return codes [A] i32, 10 search stats [A][4] i32
int sogm_debug_planner_buffer(sogm_planner *p, int which, void *out_host, size_t bytes) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  const size_t A = (size_t)p->map->n_agents, slots = A * SOGM_MAX_PIECES;
  const void  *src[11] = {p->d_polys, p->d_nfaces, p->d_npoly, p->d_goal, p->d_route, p->d_route_len, p->d_cpts, p->d_iters,
                          p->d_status, p->d_ret, p->d_stats};
  const size_t len[11] = {sizeof(double) * slots * p->pp.max_faces * 4, sizeof(int32_t) * slots, sizeof(int32_t) * A,
                          sizeof(double) * 6 * A, sizeof(double) * 6 * p->route_cap * A, sizeof(int32_t) * A,
                          sizeof(double) * slots * 15, sizeof(int32_t) * A, sizeof(int32_t) * A, sizeof(int32_t) * A,
                          sizeof(int32_t) * 4 * A};
  if (which < 0 || which > 10 || bytes > len[which]) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, src[which], bytes, hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics (tools/ only): per-agent stamps of the last pre-stamp, [A][4] ticks of 10 ns: the agent's record seen by its
// first ticket, cylinders culled, last bits ticket done, last marks ticket done
int sogm_debug_prestamp_times(sogm_planner *p, long long *out_host) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->d_flow_ts + 8 * (size_t)p->map->n_agents, sizeof(long long) * 4 * (size_t)p->map->n_agents,
                           hipMemcpyDeviceToHost));
  return SOGM_OK;
}

int sogm_planner_flow_error(sogm_planner *p) {
  if (!p) return SOGM_ERR_INVALID_ARG;
  int hdr[FLOW_HDR];
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(hdr, p->d_flow, sizeof(hdr), hipMemcpyDeviceToHost));
  return hdr[FLOW_ERR];
}

int sogm_planner_flow_failures(sogm_planner *p, int32_t out[2]) {
  if (!p || !out) return SOGM_ERR_INVALID_ARG;
  volatile int *h = p->h_flow_fail;
  out[0]          = h ? h[0] : 0;
  out[1]          = h ? h[1] : 0;
  return SOGM_OK;
}

int sogm_planner_counters(sogm_planner *p, int64_t *out_host, int reset) {
  if (!p || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->cw.counters, sizeof(int64_t) * SOGM_CNT_N, hipMemcpyDeviceToHost));
  if (reset) SOGM_HIP_CHECK(hipMemset(p->cw.counters, 0, sizeof(int64_t) * SOGM_CNT_N));
  return SOGM_OK;
}

int sogm_planner_set_publish(sogm_planner *p, SogmTrajRecord *own_records, SogmTrajRecord *next_table) {
  if (!p || (next_table && !own_records)) return SOGM_ERR_INVALID_ARG;
  p->pub_own   = own_records;
  p->pub_table = next_table;
  return SOGM_OK;
}

int sogm_planner_set_prestamp(sogm_planner *p, const SogmPrestamp *ps) {
  if (!p) return SOGM_ERR_INVALID_ARG;
  if (!ps) {
    p->ps_on = 0;
    return SOGM_OK;
  }
  if (!ps->hover_inout || !ps->out_now || !ps->out_t_start || !ps->out_pva) return SOGM_ERR_INVALID_ARG;
  const SogmWorld *w = ps->world;
  if (w) {
    if (!w->cloud_xyz || !w->block_bounds || w->n_points < 0 || w->block_points < 64 || w->block_points > 4096 ||
        w->n_blocks != (w->n_points + w->block_points - 1) / w->block_points || w->n_cyl < 0 || (w->n_cyl > 0 && !w->cylinders))
      return SOGM_ERR_INVALID_ARG;
  } else if (!ps->cloud_xyz || !ps->cloud_range || ps->n_cyl < 0 || (ps->n_cyl > 0 && !ps->cylinders)) {
    return SOGM_ERR_INVALID_ARG;
  }
  p->ps = sogm::PrestampDev{
      .frame      = {.cloud       = w ? w->cloud_xyz : ps->cloud_xyz,
                     .cloud_range = w ? nullptr : ps->cloud_range,
                     .cb          = {},  // (a world's: per replan, replan_flow)
                     .cyl         = w ? w->cylinders : ps->cylinders,
                     .n_cyl       = w ? w->n_cyl : ps->n_cyl},
      .tick       = {.own = nullptr, .hover = ps->hover_inout, .now = ps->out_now, .t_start = ps->out_t_start,
                     .pva = ps->out_pva, .start_offset = ps->replan_start_offset},
      .stamp      = ps->next_stamp,
      .poses_host = ps->out_poses};
  p->ps_world_on = w ? 1 : 0;
  if (w) {
    p->ps_world = *w;
    // the crop lists grow HERE if this frame holds more blocks than any before it (world_blocks then drains the device and
    // re-allocates): between two calls of the tick, never inside sogm_replan with the tick's persistent kernels queued
    sogm::CloudBlocks sized{};
    if (int rc = sogm::world_blocks(p->map, w, &sized)) return rc;
  }
  p->ps_on = 1;
  return SOGM_OK;
}

int sogm_planner_set_due(sogm_planner *p, const int32_t *due_dev_or_null) {
  if (!p) return SOGM_ERR_INVALID_ARG;
  p->due = due_dev_or_null;
  return SOGM_OK;
}

int sogm_planner_set_flight_fsm(sogm_planner *p, const SogmFlightFsm *fsm) {
  if (!p) return SOGM_ERR_INVALID_ARG;
  if (!fsm) {
    p->fl_fsm_on = 0;
    p->fl_fsm    = SogmFlightFsm{};
    return SOGM_OK;
  }
  if (!fsm->state_inout) {
    sogm::set_error_text("sogm_planner_set_flight_fsm: state_inout is NULL");
    return SOGM_ERR_INVALID_ARG;
  }
  const double v[5] = {fsm->prm.replan_duration, fsm->prm.replan_start_time, fsm->prm.goal_tolerance,
                       fsm->prm.new_plan_interval, fsm->check_duration};
  for (double x : v)
    if (!std::isfinite(x) || x < 0.0) {
      sogm::set_error_text("sogm_planner_set_flight_fsm: the parameters must be finite and not negative");
      return SOGM_ERR_INVALID_ARG;
    }
  if (fsm->prm.replan_max_failures < 0) {
    sogm::set_error_text("sogm_planner_set_flight_fsm: replan_max_failures must not be negative");
    return SOGM_ERR_INVALID_ARG;
  }
  p->fl_fsm    = *fsm;
  p->fl_fsm_on = 1;
  return SOGM_OK;
}

int sogm_planner_set_swarm(sogm_planner *p, const SogmTrajRecord *records, int n_records,
                           const int32_t *ego_ids, const double *t_now) {
  if (!p || n_records < 0 || (records && (!ego_ids || !t_now))) return SOGM_ERR_INVALID_ARG;
  p->swarm        = records;
  p->n_swarm      = records ? n_records : 0;
  p->swarm_stride = 0;
  p->swarm_ego    = ego_ids;
  p->swarm_now    = t_now;
  return SOGM_OK;
}

int sogm_planner_set_swarm_views(sogm_planner *p, const SogmTrajRecord *views, int n_records, const int32_t *ego_ids,
                                 const double *t_now) {
  if (int rc = sogm_planner_set_swarm(p, views, n_records, ego_ids, t_now)) return rc;
  p->swarm_stride = p->n_swarm;  // agent a checks against views[a][.]
  return SOGM_OK;
}

// The dataflow replan: a handful of launches for the whole tick.  k_astar (one workgroup per agent) publishes agents as their
// searches finish; k_worker_flow (corridor blocks and finishing blocks) and k_qp_flow are persistent and chain per agent
// through ready lists in HBM, so a slow search / corridor / QP only delays its own agent's chain.  k_flow_gate makes the
// waiting kernels dispatch only after every search is resident (they could otherwise fill the CUs and starve it).
// Streams: the caller's (k_astar), the worker stream (k_flow_reset -> k_flow_gate -> k_worker_flow -> k_flow_report), the QP
// stream (behind ev_gate) and the context's `side` (the gate and sparse reset of the grid the update swapped out) — four
// busy streams for ROCm's default of four hardware queues.  Streams that share a queue run one after the other, and a
// persistent kernel that waits holds back whatever is queued behind it.  The pre-stamp on a stream of its own and the
// dense-clear mode's wide launch are a fifth busy stream: those variants want five queues to run at full speed.
// The dataflow replan's control block and outputs back to their start values: counters / seg_done 0, ready lists -1,
// verdicts 0, ok 0, records empty.
// epoch_word (dense clear's gate, sogm_device.hpp): this replan's epoch, written by the block that reset the counters
// and after them.
// ONE workgroup, on the corridor stream, launched before the searches and run under the map update (it only touches the
// planner's own words): when everything is back to its start value the generation word gets this replan's number — the
// search workgroups wait for it in their prologue (no event between the update's last kernel and k_astar on the caller's
// stream: the record's marker cost 55 us there) and zero their agent's ok / record themselves.
// pairs: the corridors' ready words and pair verdicts (CorridorWorkspace::seg_ready, one block with pair_ok) — the waves that
// finalise an agent zero its own, a drained or timed-out tick leaves bits behind.
__global__ __launch_bounds__(1024) void k_flow_reset(int *hdr, int n_hdr, int *ready, int n_ready, int *verdict,
                                                     int n_verdict, unsigned *pairs, int n_pairs, int *epoch_word, int epoch,
                                                     int *gen_word, int gen) {
  const int i0 = (int)threadIdx.x, step = (int)blockDim.x;
  for (int i = i0; i < n_hdr; i += step) hdr[i] = 0;
  for (int i = i0; i < n_ready; i += step) ready[i] = -1;
  for (int i = i0; i < n_pairs; i += step) pairs[i] = 0u;
  if (verdict)
    for (int i = i0; i < n_verdict; i += step) verdict[i] = 0;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    if (epoch_word) __hip_atomic_store(epoch_word, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(gen_word, gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// order[rank] = agent, rank = the number of agents whose chain of this tick (search start -> finished) was longer (ties:
// lower index first); by == 0: identity
__global__ void k_update_rank(const long long *__restrict__ ts, int *__restrict__ order, int n, int by) {
  for (int a = threadIdx.x; a < n; a += blockDim.x) {
    if (!by) {
      order[a] = a;
      continue;
    }
    const long long da = ts[a * 8 + 6] - ts[a * 8 + 0];
    int             r  = 0;
    for (int b = 0; b < n; ++b) {
      const long long db = ts[b * 8 + 6] - ts[b * 8 + 0];
      r += (db > da || (db == da && b < a)) ? 1 : 0;
    }
    order[r] = a;
  }
}

// One sogm_replan through the dataflow path: the caller's arguments and what the steps below (each called once, in this
// order, by replan_flow) hand on.
struct FlowCall {
  const double   *start_pva, *goal, *t_start;
  const int32_t  *drone_ids;
  SogmTrajRecord *out_records;
  int32_t        *out_ok;
  hipStream_t     main;
  bool            spec;      // the second search attempts run beside the first
  int            *gen_word;  // the reset's generation word
  int             n_cu, wg_q, wg_f;
  bool            prestamp;  // this replan stamps the next tick's map ...
  hipStream_t     pst;       // ... on this stream (the tick's report follows it there)
};

// 0. the planner's two streams, at the first dataflow replan (a planner that only ever runs the grouped path holds none)
static int flow_streams(sogm_planner *p) {
  if (p->wstream && p->qstream) return SOGM_OK;
  sogm::Resources::Setup setup(p->res);
  SOGM_HIP_CHECK(p->res.stream(&p->wstream));
  SOGM_HIP_CHECK(p->res.stream(&p->qstream));
  return setup.done();
}
// 1. reset the control block in stream order: counters and seg_done to 0, ready lists to -1
// (one launch instead of five memset nodes: each cost a dispatch gap on the tick's critical path)
// The finishing blocks write ok / the record of every agent whose chain completes; an agent whose chain does NOT (a wait
// timed out, FLOW_ERR) must report ok = 0 and an empty record, not the previous tick's
static int flow_reset(sogm_planner *p, FlowCall &call) {
  sogm_ctx         *c    = p->map;
  const hipStream_t main = call.main, sC = p->wstream;
  const int         A    = c->n_agents;
  const bool        spec = call.spec;
  // The reset on the worker stream: behind the previous replan's report (that stream's last kernel: below) and, in the
  // pre-stamping variant, behind the pre-stamp's end; the waiting kernels of THIS replan follow it on the same stream or
  // behind ev_gate.  The readers of the swarm table on those streams wait for an all-gather in flight themselves.
  SOGM_HIP_CHECK(hipStreamWaitEvent(sC, p->ev_pdone, 0));  // (never recorded, or long complete, without a pre-stamp: no wait)
  if (c->pool.current_prestamped()) {
    // a grid adopted by sogm_update_prestamped: its overlay (on the caller's stream) waits per agent on the control
    // block's stage words — the reset must not run under it.  An event on the caller's stream, as before (this variant pays
    // the marker in front of its searches)
    SOGM_HIP_CHECK(hipEventRecord(p->ev_gate, main));
    SOGM_HIP_CHECK(hipStreamWaitEvent(sC, p->ev_gate, 0));
  }
  const FlowBlock fb(A);
  int *gen_word = p->d_flow + fb.gen;
  ++p->reset_epoch;
  hipLaunchKernelGGL(k_flow_reset, dim3(1), dim3(1024), 0, sC, p->d_flow, fb.zero_words(), p->d_flow + fb.fill_first(),
                     fb.fill_words(), spec ? p->aw.verdict : nullptr, A, p->cw.seg_ready, (int)sogm::corridor_pair_words(A),
                     c->overlap >= 2 && c->clear_gate ? c->clear_epoch_word : nullptr,
                     c->overlap >= 2 && c->clear_gate ? sogm::next_clear_epoch(c) : 0, gen_word, p->reset_epoch);
  SOGM_HIP_CHECK(hipGetLastError());
  call.gen_word = gen_word;
  return SOGM_OK;
}
// Whether this replan pre-stamps: known before the worker kernel is launched, whose finishers publish to p_ready only then.
// (only with the sparse reset: the pre-stamp runs behind the target grid's reset on the side stream, and with
//  SOGM_SPARSE_RESET=0 a dense clear fills that stream for the whole tick.  On the first ticks of a flight — and
//  after a dense writer — queue_spare_clears has queued dense clears even in sparse mode: the pre-stamp, the
//  report and ev_pdone then sit behind them, the next sogm_update_prestamped overlay waits per agent for as long
//  (tests/test_pipelining_gpu.py::test_overlay_under_the_prestamp_tail_at_full_size flies exactly that).)
// The target is the front of the ready queue as queue_spare_clears leaves it at the end of flow_launch_chain: a grid that
// is ready now, or the first dirty spare, whose reset that call queues.
static bool flow_prestamps(const sogm_planner *p) {
  const sogm_ctx *c = p->map;
  return p->ps_on && c->sparse && c->overlap >= 2 && (c->pool.front_ready() >= 0 || c->pool.first_dirty() >= 0) && p->pub_own &&
         c->clear_gate;
}
// 2. the searches on the caller's stream, then the residency gate and the worker kernel on the worker stream, the QP kernel
// on its own
// (the searches run on the caller's stream: they are the first kernel of the chain, and a hop to another stream
//  costs an event round trip on the critical path)
static int flow_launch_chain(sogm_planner *p, FlowCall &call) {
  sogm_ctx         *c    = p->map;
  const hipStream_t main = call.main, sA = main, sC = p->wstream, sQ = p->qstream;
  const int         A    = c->n_agents;
  const MapView     mv   = view_of(c);
  const bool        spec = call.spec;
  int              *gen_word = call.gen_word;
  const double     *start_pva = call.start_pva, *goal = call.goal, *t_start = call.t_start;
  SogmTrajRecord   *out_records = call.out_records;
  int32_t          *out_ok      = call.out_ok;
  if (c->exchange_pending) {
    SOGM_HIP_CHECK(hipStreamWaitEvent(sC, c->ev_xdone, 0));
    SOGM_HIP_CHECK(hipStreamWaitEvent(sQ, c->ev_xdone, 0));
  }
  prof_begin(c, SOGM_PROF_ASTAR, sA);
  // an update flow still building this tick's maps (sogm_update_world with update_flow): the searches are launched beside
  // it and every search workgroup waits for ITS agent's map; the caller's stream joins the flow's end at the fan-in
  sogm::FlowCtl fca = p->fc;
  fca.map_ready = c->update_pending ? c->d_map_ready : nullptr;
  fca.map_epoch = c->map_epoch;
  fca.reset_gen   = gen_word;
  fca.reset_epoch = p->reset_epoch;
  fca.out_ok      = out_ok;
  fca.out_records = reinterpret_cast<int *>(out_records);
  fca.rec_words   = (int)(sizeof(SogmTrajRecord) / sizeof(int));
  if (int rc = launched("sogm_replan: k_astar",
                        launch_astar(mv, p->ap, p->pp.corridor_tau, astar_ws(p), A, search_io(p, start_pva, goal, t_start),
                                     nullptr, 0, sA, 0, &fca, spec ? 8 : 0)))
    return rc;
  prof_end(c, SOGM_PROF_ASTAR, sA);
  // "the searches are launched" for the side-stream work that starts from here (spare grids' clears, the pre-stamp):
  // recorded BEHIND k_astar — in front of it the record's marker held the searches back by 55 us
  SOGM_HIP_CHECK(hipEventRecord(p->ev_in, main));
  if (int rc = launched("sogm_replan: k_flow_gate", sogm::launch_flow_gate(p->fc, spec ? 2 * A : A, sC))) return rc;
  SOGM_HIP_CHECK(hipEventRecord(p->ev_gate, sC));
  SOGM_HIP_CHECK(hipStreamWaitEvent(sQ, p->ev_gate, 0));
  // persistent workgroups: one wave each for the corridor items (4 per CU fit), half of the CUs' worth of QP
  // workgroups (each takes a whole CU's LDS while it runs; with fewer, agents queue for a solver — measured: 64 / 96
  // / 128 / 160 workgroups -> 6.3 / 6.9 / 7.5 / 7.4 k replans/s), a handful of finishing waves
  // (finish_wgs / corridor_wgs: tuning aids; tests starve a role with them so that its loop runs more than one trip)
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  int wg_c = 4 * n_cu;
  if (c->tune_i(SOGM_TUNE_CORRIDOR_WGS) > 0) wg_c = c->tune_i(SOGM_TUNE_CORRIDOR_WGS);
  if (wg_c > A * SOGM_MAX_PIECES) wg_c = A * SOGM_MAX_PIECES;
  int wg_q = n_cu / 2;
  if (c->tune_i(SOGM_TUNE_QP_WGS) > 0) wg_q = c->tune_i(SOGM_TUNE_QP_WGS);  // tuning aid
  if (wg_q > A) wg_q = A;
  if (wg_q < 1) wg_q = 1;
  int wg_f = 64;
  if (c->tune_i(SOGM_TUNE_FINISH_WGS) > 0) wg_f = c->tune_i(SOGM_TUNE_FINISH_WGS);
  if (wg_f > A) wg_f = A;
  call.n_cu = n_cu, call.wg_q = wg_q, call.wg_f = wg_f;
  // the worker kernel: the finishers (lowest block indices: dispatched first) and the corridor stage in one launch
  call.prestamp     = flow_prestamps(p);
  sogm::FlowCtl fcw = p->fc;
  if (!call.prestamp) fcw.p_ready = nullptr;
  prof_begin(c, SOGM_PROF_CORRIDOR, sC);
  if (int rc = launched("sogm_replan: k_worker_flow",
                        sogm::launch_worker_flow(mv, p->pp, p->cw, fcw, A, wg_f, wg_c, corridor_io(p, start_pva, t_start),
                                                 finish_args(p, t_start, call.drone_ids, out_records, out_ok), sC)))
    return rc;
  prof_end(c, SOGM_PROF_CORRIDOR, sC);
  // every record is published behind the worker kernel (sogm_traj_allgather starts from here: flow_fan_in)
  SOGM_HIP_CHECK(hipEventRecord(p->ev_records, sC));
  // (a QP workgroup takes a whole CU — registers and LDS — from the moment it is resident, and the first corridors are
  //  final long after an update flow has ended: the QP kernel is dispatched behind the flow's end, not beside it)
  if (c->update_pending) SOGM_HIP_CHECK(hipStreamWaitEvent(sQ, c->ev_udone, 0));
  prof_begin(c, SOGM_PROF_QP, sQ);
  if (int rc = launched("sogm_replan: k_qp_flow",
                        sogm::launch_qp_flow(p->pp, p->qs, p->qw, p->qc, p->fc, A, wg_q, qp_io(p, start_pva), sQ)))
    return rc;
  prof_end(c, SOGM_PROF_QP, sQ);
  // (queued AFTER the searches / corridor / QP launches: its gate waits for the corridor stage, and when streams share a
  //  hardware queue a launch behind a waiting gate waits with it — a QP kernel started 5 ms late costs the tick 5 ms)
  c->gate_open_valid = 0;
  c->gate_frac_valid = 0;
  {
    const double f      = c->tune[SOGM_TUNE_PRESTAMP_GATE_FRAC];
    c->gate_frac_agents = f > 0.0 && f < 1.0 ? ((int)(f * A + 0.5) < 1 ? 1 : (int)(f * A + 0.5)) : 0;
  }
  if (c->overlap >= 2) {
    // the side-stream clear of the grid this tick's update swapped out: narrow, with a wide second launch that joins
    // once every agent's corridors are final (FLOW_Q_READY_N == A, registered as the gate at planner creation) —
    // announce this replan's epoch now that the counters are reset
    int rc = sogm::queue_spare_clears(c, p->ev_in);  // grids still dirty (first ticks, pool changes)
    if (rc) return rc;
  }
  return SOGM_OK;
}
// 3. the pre-stamp's arguments from sogm_planner_set_prestamp's and the tuning: no HIP call (tgt and frame.cb: flow_prestamp)
static sogm::PrestampDev prestamp_args(const sogm_planner *p) {
  const sogm_ctx   *c = p->map;
  const int         A = c->n_agents;
  sogm::PrestampDev d = p->ps;
  d.tick.own = p->pub_own;
  d.n_agents = A;
  {
    const double f = c->tune[SOGM_TUNE_PRESTAMP_GATE_FRAC];
    d.gate_agents  = f >= 1.0 ? A : f <= 0.0 ? 0 : (int)(f * A + 0.5);
  }
  // tickets per agent (tuning aids): too few and the last agents' stamps trail the replan, too many and the
  // hand-overs cost more than the work (bits + marks 16+16 / 32+64 / 64+64 / 128+256 tickets: 13.1 / 12.1 / 12.2 /
  // 14.1 ms per tick, 13.0 without the pre-stamp); finer tickets for the last agents to be published (none / 8 / 16
  // late agents: 12.06 / 11.85 / 11.98 ms per tick)
  const int nb = c->tune_i(SOGM_TUNE_PRESTAMP_BITS) > 0 ? c->tune_i(SOGM_TUNE_PRESTAMP_BITS) : 32;
  const int nm = c->tune_i(SOGM_TUNE_PRESTAMP_MARKS) > 0 ? c->tune_i(SOGM_TUNE_PRESTAMP_MARKS) : 64;
  d.n_bits       = nb;
  d.n_marks      = nm;
  d.n_late       = c->tune_i(SOGM_TUNE_PRESTAMP_LATE_AGENTS) < 0 ? 0 : c->tune_i(SOGM_TUNE_PRESTAMP_LATE_AGENTS);
  d.n_bits_late  = c->tune_i(SOGM_TUNE_PRESTAMP_LATE_BITS) > 0 ? c->tune_i(SOGM_TUNE_PRESTAMP_LATE_BITS) : nb;
  d.n_marks_late = c->tune_i(SOGM_TUNE_PRESTAMP_LATE_MARKS) > 0 ? c->tune_i(SOGM_TUNE_PRESTAMP_LATE_MARKS) : nm;
  return d;
}
// 4. pre-stamp (sogm_planner_set_prestamp): the next tick's map, agent by agent as their records are published, into
// the pool's next grid — behind the gate that keeps store streams away from the searches and point scans, and
// behind that grid's reset
static int flow_prestamp(sogm_planner *p, FlowCall &call) {
  sogm_ctx *c = p->map;
  const int A = c->n_agents;
  c->pool.clear_prestamp_target();
  // the pre-stamp's stream (why it has one of its own: below; created by the first replan that pre-stamps on it — it is the
  // tick's fifth busy stream, and a replan that does not pre-stamp holds no place in the pool of hardware queues for it);
  // the tick's report follows it there
  const bool own_stream = c->tune_i(SOGM_TUNE_PRESTAMP_STREAM) != 0 && call.prestamp;
  if (own_stream && !c->pstream) {
    sogm::Resources::Setup setup(c->res);
    SOGM_HIP_CHECK(c->res.stream(&c->pstream));
    setup.done();
  }
  const hipStream_t pst = own_stream ? c->pstream : c->side;
  call.pst = pst;
  if (call.prestamp) {
    const int nxt = c->pool.front_ready();  // (>= 0: flow_prestamps saw a ready or a dirty spare, and the dirty ones are queued by now)
    sogm::PrestampDev d = prestamp_args(p);
    if (int rc = sogm::map_target(c, nxt, true, nullptr, &d.tgt)) return rc;
    if (p->ps_world_on)  // the frame's blocks + the context's crop lists (built by each agent's first ticket)
      if (int rc = sogm::world_blocks(c, &p->ps_world, &d.frame.cb)) return rc;
    // The pre-stamp's target grid was reset by an EARLIER replan when the pool holds three grids (the front of the ready
    // queue), yet on the resets' stream the launch would also sit behind THIS replan's reset — which is held back until
    // every agent's corridors are final and then takes a millisecond: traces showed the pre-stamp starting at 5.6 ms
    // of the tick, working off a backlog of ~100 published agents on the CUs the QP workgroups leave free, and ending
    // 1-2.5 ms after the last QP in half of the ticks — the tick's end.  It runs on a stream of its own, ordered
    // behind its target's reset (and log restart) by that grid's event and behind "every agent's corridors are final"
    // by an event recorded after a gate kernel on the resets' stream: reset and pre-stamp then run side by side.  The
    // pre-stamp's gate is "prestamp_gate_frac of the agents' corridors are final" (default 0.9): waiting for ALL of them
    // makes 127 agents' stamps wait for one late search — seen as ticks ending 1.5-2.9 ms after their slowest chain — while
    // the few agents still searching or scanning points pay little for the stores beside them (same box: burst 9.07 ->
    // 8.81 ms, 300 sustained ticks 10.3 -> 11.3 k replans/s; 0.5 starts too early and loses late in a flight).  The gate
    // with the lower target is a kernel on the resets' stream — which spins for the full gate anyway — followed by an
    // event; a first version put a spinning gate at the head of THIS stream, one more spinner for shared or
    // oversubscribed hardware queues to stall on.  (prestamp_stream = 0: round 3's placement on the resets' stream.)
    SOGM_HIP_CHECK(hipStreamWaitEvent(pst, p->ev_in, 0));
    if (own_stream) {
      SOGM_HIP_CHECK(hipStreamWaitEvent(pst, c->pool.cleared_event(nxt), 0));
      if (c->gate_frac_valid && d.gate_agents < A)
        SOGM_HIP_CHECK(hipStreamWaitEvent(pst, c->ev_gate_frac, 0));
      else if (c->gate_open_valid && d.gate_agents >= A)
        SOGM_HIP_CHECK(hipStreamWaitEvent(pst, c->ev_gate_open, 0));
    }
    int wg_p = 8 * call.n_cu;  // one-wave workgroups (512 / 1024 / 2048+: 14.0 / 12.3 / 12.1 ms per tick)
    if (c->tune_i(SOGM_TUNE_PRESTAMP_WGS) > 0) wg_p = c->tune_i(SOGM_TUNE_PRESTAMP_WGS);
    if (int rc = launched("sogm_replan: k_prestamp_flow",
                          sogm::launch_prestamp_flow(c->geom, p->fc, d, wg_p, call.wg_q, call.wg_f < A ? call.wg_f : A, pst)))
      return rc;
    c->pool.set_prestamp_target(nxt);
    c->n_stamps++;
    c->ps_fail_host = p->h_flow_fail;  // sogm_update_prestamped refuses the grid if this replan turns out to have failed
    c->ps_fail_seen = p->h_flow_fail ? p->h_flow_fail[1] : 0;
  }
  return SOGM_OK;
}
// 5. fan-in.  Without a pre-stamp the tick's report runs on the worker stream behind the worker and QP kernels, so that
// the NEXT replan's reset — same stream — is ordered behind it without an event on the caller's stream
static int flow_fan_in(sogm_planner *p, const FlowCall &call) {
  sogm_ctx         *c    = p->map;
  const hipStream_t main = call.main, sC = p->wstream, sQ = p->qstream, pst = call.pst;
  const int         A    = c->n_agents;
  const int         retire     = c->tune_i(SOGM_TUNE_CLEAR_RETIRE_AT_END);  // measured: tick -2 %, but the clear 14.5 -> 15.5 ms; off
  auto report = [&](hipStream_t st) {
    hipLaunchKernelGGL(k_flow_report, dim3(1), dim3(1), 0, st, (const int *)p->d_flow, p->h_flow_fail,
                       retire ? p->d_epoch : (int *)nullptr, c->h_tick_clock);
    return hipGetLastError();
  };
  const bool report_on_sc = !c->pool.prestamp_pending();
  SOGM_HIP_CHECK(hipEventRecord(p->ev_qdone, sQ));
  if (report_on_sc) {
    SOGM_HIP_CHECK(hipStreamWaitEvent(sC, p->ev_qdone, 0));
    SOGM_HIP_CHECK(report(sC));
  }
  SOGM_HIP_CHECK(hipEventRecord(p->ev_wdone, sC));
  SOGM_HIP_CHECK(hipStreamWaitEvent(main, p->ev_wdone, 0));
  SOGM_HIP_CHECK(hipStreamWaitEvent(main, p->ev_qdone, 0));
  if (int rc = sogm::join_update(c, main)) return rc;  // (complete long ago: every search waited for its agent's map)
  if (c->d_update_order && c->tune_i(SOGM_TUNE_UPDATE_FLOW) != 0) {
    // the next update flow takes the agents in the order of this tick's chain lengths, longest first (a schedule only)
    hipLaunchKernelGGL(k_update_rank, dim3(1), dim3(256), 0, main, (const long long *)p->fc.ts, c->d_update_order, A,
                       c->tune_i(SOGM_TUNE_UPDATE_ORDER));
    SOGM_HIP_CHECK(hipGetLastError());
  }
  bool reported = report_on_sc;
  if (c->pool.prestamp_pending()) {
    // the tick's report behind the pre-stamp on ITS stream (the last kernel of the tick to end), so that the caller's
    // stream goes from the fan-in straight to the next tick's first kernel instead of through one more launch
    SOGM_HIP_CHECK(hipStreamWaitEvent(pst, p->ev_wdone, 0));
    SOGM_HIP_CHECK(hipStreamWaitEvent(pst, p->ev_qdone, 0));
    SOGM_HIP_CHECK(report(pst));
    SOGM_HIP_CHECK(hipEventRecord(p->ev_pdone, pst));
    const int defer = c->tune_i(SOGM_TUNE_SPLAT_OVERLAP) != 0;  // 0: the caller's stream waits for the pre-stamp's end here
    if (defer) {
      // the caller's stream goes on behind the fan-in: the next update's overlay waits per agent (sogm_update_prestamped),
      // everything else joins the pre-stamp's end when it is called (sogm::join_prestamp)
      c->ev_pdone      = p->ev_pdone;
      c->pdone_pending = 1;
      c->ps_stage      = p->fc.stage;
      c->ps_err        = &p->fc.hdr[FLOW_ERR];
    } else {
      SOGM_HIP_CHECK(hipStreamWaitEvent(main, p->ev_pdone, 0));
    }
    reported = true;
  }
  // the exchange of the records this replan publishes may start when the worker kernel — its finishers — is done
  // (sogm_traj_allgather): the event recorded behind that kernel and in front of the report
  c->records_final_valid = 0;
  if (p->pub_own) {
    c->ev_records_final    = p->ev_records;
    c->records_final_ptr   = p->pub_own;
    c->records_final_valid = 1;
  }
  if (!reported) SOGM_HIP_CHECK(report(main));
  return SOGM_OK;
}

static int replan_flow(sogm_planner *p, const double *start_pva, const double *goal, const double *t_start,
                       const int32_t *drone_ids, SogmTrajRecord *out_records, int32_t *out_ok, void *stream) {
  FlowCall call{.start_pva = start_pva, .goal = goal, .t_start = t_start, .drone_ids = drone_ids, .out_records = out_records,
                .out_ok = out_ok, .main = (hipStream_t)stream, .spec = p->spec_astar != 0};
  if (p->swarm)
    if (int rc = sogm::join_exchange(p->map, call.main)) return rc;
  if (int rc = flow_streams(p)) return rc;
  if (int rc = flow_reset(p, call)) return rc;
  if (int rc = flow_launch_chain(p, call)) return rc;
  if (int rc = flow_prestamp(p, call)) return rc;
  return flow_fan_in(p, call);
}

static int replan_impl(sogm_planner *p, const double *start_pva, const double *goal,
                       const double *t_start, const int32_t *drone_ids, SogmTrajRecord *out_records,
                       int32_t *out_ok, void *stream) {
  sogm_ctx   *c    = p->map;
  hipStream_t main = (hipStream_t)stream;
  const int   A = c->n_agents, G = p->n_groups;
  const MapView mv = view_of(c);
  if (int rc = sogm::join_update(c, main)) return rc;
  for (int g = 0; g < G; ++g)
    if (!p->gstream[g]) SOGM_HIP_CHECK(p->res.stream(&p->gstream[g]));
  // the swarm's records (deconfliction) may come from an all-gather still in flight on the exchange stream
  if (p->swarm)
    if (int rc = sogm::join_exchange(c, main)) return rc;
  // fan out: every group stream starts when the caller's stream has produced the inputs
  SOGM_HIP_CHECK(hipEventRecord(p->ev_in, main));
  if (c->overlap >= 2) {
    // double / triple-buffered SOGM: the spare grid this tick's update swapped out is cleared on the side stream
    // under this whole replan (its last readers, the previous tick's corridor kernels, are ordered before ev_in).
    // Mode 2: it is the NEXT update's grid (deadline: the next stamp).  Mode 3: the next update takes the grid
    // cleared during the PREVIOUS replan, so every clear has a whole tick of slack.
    int rc = sogm::queue_spare_clears(c, p->ev_in);
    if (rc) return rc;
  }
  for (int g = 0; g < G; ++g) {
    const int a0 = (int)((long long)A * g / G), a1 = (int)((long long)A * (g + 1) / G), n = a1 - a0;
    if (n <= 0) continue;
    hipStream_t st = p->gstream[g];
    SOGM_HIP_CHECK(hipStreamWaitEvent(st, p->ev_in, 0));
    hipError_t e = launch_astar(mv, p->ap, p->pp.corridor_tau, astar_ws(p), n, search_io(p, start_pva, goal, t_start),
                                nullptr, 0, st, a0);
    if (e == hipSuccess) e = launch_corridor(mv, p->pp, p->cw, n, corridor_io(p, start_pva, t_start), st, a0, p->ev_pts[g]);
    if (int rc = launched("sogm_replan launch", e)) return rc;
    SOGM_HIP_CHECK(hipEventRecord(p->ev_corr[g], st));
  }
  if (c->overlap == 1) {
    // Single grid, cleared in place for the next update in two parts on the side stream.  Head: a narrow launch
    // as soon as every group's obstacle-point kernel — the tick's last reader of the SOGM — is done; it shares the
    // machine with the FIRI kernels (about what they take to run: ~28 GB).  Rest: a full-width launch once every
    // group's corridor stage has finished with global memory (a full-width clear starves every concurrent load;
    // k_qp only touches LDS).
    const size_t total = sogm::clear_vec4_total(c);
    size_t       head  = (size_t)28e9 / 16;
    if (head > total / 2) head = total / 2;
    for (int g = 0; g < G; ++g) SOGM_HIP_CHECK(hipStreamWaitEvent(c->side, p->ev_pts[g], 0));
    const int slot = c->pool.current();
    if (c->pool.loggable(slot)) {
      // sparse reset: the logged sectors only, as soon as the SOGM's last readers are done
      int rc = sogm::reset_slot(c, c->side, slot, c->d_grid, true);
      if (rc) return rc;
    } else {
      int rc = sogm::launch_clear(c, c->side, c->d_grid, true, 1, head);
      if (rc) return rc;
      for (int g = 0; g < G; ++g) SOGM_HIP_CHECK(hipStreamWaitEvent(c->side, p->ev_corr[g], 0));
      rc = sogm::launch_clear(c, c->side, c->d_grid, false, 2, head);
      if (rc) return rc;
    }
    SOGM_HIP_CHECK(hipEventRecord(c->ev_cleared, c->side));
    c->pool.cleared_in_place();
    c->updated = 0;
  }
  for (int g = 0; g < G; ++g) {
    const int a0 = (int)((long long)A * g / G), a1 = (int)((long long)A * (g + 1) / G), n = a1 - a0;
    if (n <= 0) continue;
    hipStream_t st = p->gstream[g];
    if (int rc = launched("sogm_replan launch_qp", launch_qp(p->pp, p->qs, p->qw, p->qc, n, qp_io(p, start_pva), st, a0)))
      return rc;
    if (p->swarm)
      if (int rc = launched("sogm_replan launch_deconflict",
                            sogm::launch_deconflict(n, p->d_cpts, p->d_npoly, p->swarm, p->n_swarm, p->swarm_ego,
                                                    p->swarm_now, p->d_safe, st, a0, p->cw.counters, p->swarm_stride)))
        return rc;
    SOGM_HIP_CHECK(sogm::launch_pack_records(n, finish_args(p, t_start, drone_ids, out_records, out_ok), st, a0));
    SOGM_HIP_CHECK(hipEventRecord(p->ev_done[g], st));
    SOGM_HIP_CHECK(hipStreamWaitEvent(main, p->ev_done[g], 0));  // fan in
  }
  return SOGM_OK;
}


int sogm_replan(sogm_planner *p, const double *start_pva, const double *goal,
                const double *t_start, const int32_t *drone_ids, SogmTrajRecord *out_records,
                int32_t *out_ok, void *stream) {
  if (!p || !start_pva || !goal || !t_start || !drone_ids || !out_records || !out_ok)
    return SOGM_ERR_INVALID_ARG;
  if (!p->map->updated) return SOGM_ERR_STATE;
  sogm_ctx *c = p->map;
  // publication (sogm_planner_set_publish): the finishing kernel writes every agent's record into next_table while
  // other agents' deconfliction still reads the swarm table, and into own_records while out_records is written
  if (p->pub_table && p->swarm) {  // byte ranges, not pointers: a rank's slice INSIDE the all-records buffer overlaps too
    const char *a0 = (const char *)p->pub_table, *a1 = a0 + sizeof(SogmTrajRecord) * (size_t)c->n_agents;
    // (the extent of the one table, or of the agents' views [n_agents][n_swarm])
    const char *b0 = (const char *)p->swarm;
    const char *b1 = b0 + sizeof(SogmTrajRecord) * (size_t)p->n_swarm * (size_t)(p->swarm_stride ? c->n_agents : 1);
    if (a0 < b1 && b0 < a1) {
      sogm::set_error_text("sogm_replan: sogm_planner_set_publish's next_table overlaps the table given to sogm_planner_set_swarm");
      return SOGM_ERR_INVALID_ARG;
    }
  }
  if (p->pub_own) {
    const char *a0 = (const char *)p->pub_own, *a1 = a0 + sizeof(SogmTrajRecord) * (size_t)c->n_agents;
    const char *b0 = (const char *)out_records, *b1 = b0 + sizeof(SogmTrajRecord) * (size_t)c->n_agents;
    if (a0 < b1 && b0 < a1) {
      sogm::set_error_text("sogm_replan: out_records overlaps sogm_planner_set_publish's own_records");
      return SOGM_ERR_INVALID_ARG;
    }
  }
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  // the in-place pre-clear (mode 1) needs the grouped path's "last reader of the SOGM" events
  const bool use_flow = p->flow && c->overlap != 1;
  if (int jr = sogm::join_prestamp(c, (hipStream_t)stream)) return jr;  // a pre-stamp nobody has waited for yet
  const int  rc = use_flow ? replan_flow(p, start_pva, goal, t_start, drone_ids, out_records, out_ok, stream)
                           : replan_impl(p, start_pva, goal, t_start, drone_ids, out_records, out_ok, stream);
  if (rc != SOGM_OK) {
    // A launch failed half-way: group / side streams may hold work the caller's stream was never joined to, and
    // a pre-clear may or may not have been issued.  Drain everything and forget the pre-clear (the next update
    // clears its grid itself); an in-place clear (mode 1) may already have eaten part of the map.
    (void)hipDeviceSynchronize();
    if (c->pool.precleared() && c->overlap == 1) c->updated = 0;
    if (c->overlap < 2) c->pool.forget_preclear();  // modes 2 / 3: clears already queued stay valid (events recorded)
  }
  return rc;
}
}
