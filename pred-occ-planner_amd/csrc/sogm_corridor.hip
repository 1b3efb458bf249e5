// sogm_corridor.hip — batched safe-corridor generation (FIRI polytopes) on the SOGM, gfx950.
//
// Reference: the corridor stage of FakeBaselinePlanner::replan / BaselinePlanner::replan
// (plan_manager/src/baseline_fake.cpp:300-414, baseline.cpp:296-403) =
//   getObstaclePoints (plan_env/src/map.cpp:480-518 / risk_base.cpp:295-337)
//   firi::firi + maxVolInsEllipsoid + costMVIE (plan_manager/include/sfc_gen/firi.hpp:44-365)
//   lbfgs::lbfgs_optimize + Lewis-Overton line search (plan_manager/include/sfc_gen/lbfgs.hpp)
//   sdlp::linprog<3|4> (traj_utils/include/traj_utils/sdlp.hpp) — the projective Seidel LP, whole-wave
//   ShrinkCorridor / checkCorridorValidity / checkCorridorIntersect / checkGoalReachability.
//
// Mapping to CDNA4: one 64-lane wave per (agent, path segment) — 7 segments x 128 agents = 896 independent
// problems fill the 256 CUs (4 waves per CU, 39.8 KB LDS each).  Inside a wave the point-cloud work is lane-parallel
// (obstacle-point extraction with an order-preserving wave scan, ellipsoid-frame transform, tangent planes, the
// greedy plane selection with a wave arg-min that breaks ties by index exactly like the reference's sequential scan);
// the LPs are solved by the whole wave (sdlp's projective algorithm, see linprog_wave), the MVIE cost is evaluated one
// face per lane and summed in the reference's order, the 9-variable L-BFGS and the 3x3 Jacobi run replicated /
// on lane 0 with their working set in LDS.  The per-agent bookkeeping (first invalid corridor, adjacent
// intersections, goal projection) is done by the wave that finishes an agent's last segment (dataflow replan) or by
// a second small kernel (grouped path).  All fp64, operation order identical to the CPU oracle — which follows the
// reference's (-ffp-contract=off, include/sogm_detmath.h for log) — so polytopes match bit for bit.
// No dense contraction -> no MFMA.
//
// This file is the corridor stage: its kernels, their launchers and the C entry points of the stage and its test hooks.
// The device bodies the kernels inline are in sogm_corridor.hpp (points, FIRI segment, bookkeeping, the segment slot), the
// ellipsoid optimiser in sogm_mvie.hpp, the wave LP and the LDS layouts in sogm_lp.hpp.  The flight's worker kernel, which
// runs the same segment slot, is written in sogm_flight_light.hpp and compiled here.  How a replan ends (isSafeAfterOpt,
// records, counters) is sogm_finish.hpp / sogm_finish.hip; the dataflow replan's finishing role runs in this file's worker
// kernel (k_worker_flow).
#include <hip/hip_runtime.h>

#include "sogm_corridor.hpp"
#include "sogm_finish.hpp"

namespace sogm {

// Kernel P (corridor_points_body): obstacle points of one (segment, agent), four waves
__global__ __launch_bounds__(256) void k_corridor_points(MapView m, SogmPlannerParams pp, CorridorWorkspace ws,
                                                        const double *__restrict__ start_pva,
                                                        const double *__restrict__ t_start,
                                                        const double *__restrict__ route,
                                                        const int32_t *__restrict__ route_len, int route_cap,
                                                        int agent0) {
  const CorridorIO io{.start_pva = start_pva, .t_start = t_start, .route = route, .route_len = route_len,
                      .route_cap = route_cap};
  corridor_points_body<4>(m, pp, ws, io, blockIdx.y + agent0, blockIdx.x);
}

// Kernel A (corridor_segment_body): one workgroup per (segment, agent); k_firi_direct is its standalone firi::firi form
__global__ __launch_bounds__(64) void k_corridor_segment(
    MapView m, SogmPlannerParams pp, CorridorWorkspace ws, const double *__restrict__ start_pva,
    const double *__restrict__ t_start, const double *__restrict__ route,
    const int32_t *__restrict__ route_len, int route_cap, int agent0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const CorridorIO io{.start_pva = start_pva, .t_start = t_start, .route = route, .route_len = route_len,
                      .route_cap = route_cap};
  corridor_segment_body<6, false>(m, pp, ws, io, blockIdx.y + agent0, blockIdx.x, smem, FiriDirect{});
}

__global__ __launch_bounds__(64) void k_firi_direct(MapView m, SogmPlannerParams pp, CorridorWorkspace ws,
                                                    FiriDirect fd) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  corridor_segment_body<FIRI_DIRECT_BD_MAX, true>(m, pp, ws, CorridorIO{}, blockIdx.x, 0, smem, fd);
}

// Kernel B (corridor_finalize_body): per agent bookkeeping, one wave per agent
__global__ __launch_bounds__(64) void k_corridor_finalize(
    SogmPlannerParams pp, CorridorWorkspace ws, const double *__restrict__ start_pva,
    const double *__restrict__ route, const int32_t *__restrict__ route_len, int route_cap,
    double *__restrict__ out_polys, int32_t *__restrict__ out_nfaces,
    int32_t *__restrict__ out_npoly, double *__restrict__ out_goal, int agent0) {
  const CorridorIO io{.start_pva = start_pva, .route = route, .route_len = route_len, .route_cap = route_cap,
                      .out_polys = out_polys, .out_nfaces = out_nfaces, .out_npoly = out_npoly, .out_goal = out_goal};
  extern __shared__ __attribute__((aligned(16))) char smem[];
  corridor_finalize_body(pp, ws, io, blockIdx.x + agent0, LpLds::carve(smem));
}

// Test hook (sogm_corridor_rules_batched): the rules around FIRI for polytopes the caller injects, one wave per problem.
// The wave lays a CorridorWorkspace view over the caller's arrays, then per segment runs segment_box, shrink_corridor and
// corridorValidW as corridor_segment_body does after FIRI, and ends in corridor_finalize_body: the replan's device code,
// with the caller's polytopes where FIRI's would be.
struct CorridorRules {
  const SogmPlannerParams *pp;         // [n]
  const double            *polys_in;   // [n][SOGM_MAX_PIECES][max_faces][4] un-shrunk
  const int32_t           *nfaces_in;  // [n][SOGM_MAX_PIECES]
  const int32_t           *state_in;   // [n][SOGM_MAX_PIECES] or null; -3 = "capacity exceeded" in this segment
  double                  *out_box;    // [n][SOGM_MAX_PIECES][6] llc, lhc
};
// segment `seg` of problem `prob`: box, shrink, own validity, with the caller's polytope where FIRI's would be (whole wave)
__device__ __forceinline__ void rules_segment(const CorridorRules &cr, const SogmPlannerParams &pp, const CorridorWorkspace &ws,
                                              const CorridorIO &io, int prob, int seg, char *smem) {
  double *base = (double *)smem, *s_poly = base + RulesLds::poly, *s_box = base + RulesLds::box, *s_w = base + RulesLds::w;
  const LpScratch sc{base + LpLds::work, base + LpLds::rows, (int *)(smem + RulesLds::perm)};
  const int lane = threadIdx.x, MF = pp.max_faces;
  const int slot = prob * SOGM_MAX_PIECES + seg;
  if (seg >= io.points(prob) - 1) {
    if (lane == 0) {
      ws.seg_state[slot]  = -2;  // no such segment
      ws.seg_nfaces[slot] = 0;
      for (int k = 0; k < 6; ++k) cr.out_box[slot * 6 + k] = 0.0;
    }
    return;
  }
  int nf = cr.nfaces_in[slot];
  nf     = nf < 0 ? 0 : (nf > MF ? MF : nf);
  if (lane == 0) segment_box(pp, io.start_pva + prob * 9, io.route + (size_t)prob * io.route_cap * 6, seg, s_box, s_w);
  for (int i = lane; i < nf * 4; i += 64) s_poly[i] = cr.polys_in[(size_t)slot * MF * 4 + i];
  wave_lds_sync();
  shrink_corridor(pp, s_w, s_poly, nf);
  wave_lds_sync();
  const bool valid = corridorValidW(s_poly, nf, nullptr, 0, sc);
  double    *out   = ws.polys + (size_t)slot * MF * 4;
  for (int i = lane; i < nf * 4; i += 64) out[i] = s_poly[i];
  if (lane == 0) {
    for (int k = 0; k < 6; ++k) cr.out_box[slot * 6 + k] = s_box[k];
    ws.seg_nfaces[slot] = nf;
    ws.seg_state[slot]  = cr.state_in && cr.state_in[slot] == -3 ? -3 : (valid ? 1 : 0);
  }
  wave_lds_sync();
}
__global__ __launch_bounds__(64) void k_corridor_rules(CorridorRules cr, CorridorWorkspace ws, CorridorIO io) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double         *base = (double *)smem;
  const LpScratch sc{base + LpLds::work, base + LpLds::rows, (int *)(smem + RulesLds::perm)};
  const int               prob = blockIdx.x;
  const SogmPlannerParams pp   = cr.pp[prob];
  for (int seg = 0; seg < SOGM_MAX_PIECES; ++seg) rules_segment(cr, pp, ws, io, prob, seg, smem);
  __threadfence_block();  // the bookkeeping reads every lane's polytope rows back from memory
  __syncthreads();
  corridor_finalize_body(pp, ws, io, prob, sc);
}

// The rules hook in the replan's parallel form (sogm_corridor_rules_batched_flags, SOGM_RULES_PARALLEL): SOGM_MAX_PIECES one-wave
// workgroups per problem, each its segment as k_corridor_rules does it, then corridor_slot's second half — corridor_slot
// with the caller's polytopes where FIRI's would be.  seg_done: [n] zeroes.
__global__ __launch_bounds__(64) void k_corridor_rules_slots(CorridorRules cr, CorridorWorkspace ws, CorridorIO io, int *seg_done) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int               prob = blockIdx.x / SOGM_MAX_PIECES, seg = blockIdx.x % SOGM_MAX_PIECES;
  const SogmPlannerParams pp   = cr.pp[prob];
  rules_segment(cr, pp, ws, io, prob, seg, smem);
  __syncthreads();
  corridor_slot_done(pp, ws, io, prob, seg, seg < io.points(prob) - 1, smem, seg_done, false);
}
// what the parallel hook left set in its ready words and verdict rows (nothing, if its finalising waves cleaned up)
__global__ void k_pairs_residue(const unsigned *words, int n, unsigned long long *pair_cnt) {
  unsigned v = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) v |= words[i];
  if (v) atomicOr(&pair_cnt[3], (unsigned long long)v);
}

// =================================================================================================
// Dataflow kernel W (sogm_replan, pipelining modes 0 / 2 / 3): ONE persistent launch of one-wave workgroups for the
// corridor stage and for the end of every agent's replan, the role given by the block index (the flight's k_flight_light
// is the same fusion over one queue; both are compiled in this unit, sogm_flight_light.hpp says why).  One launch, one
// stream: with the caller's stream, the QP kernel's and the resets' the tick keeps four streams busy, ROCm's default number
// of hardware queues.
// Blocks [0, wg_f) finish: a wave takes the agent whose QP finished ticket-th, runs finish_agent (what k_safe_after_opt +
// k_pack_records do in the grouped path) and hands the agent to the pre-stamp.  The lowest indices are dispatched first:
// the finishers are resident from the start, and each draws its first FLOW_F_TICKET as it starts — k_prestamp_gate
// reads that word as "finishing waves resident".
// The other blocks are the corridor stage.  A wave takes tickets; ticket k is segment k % 16 of the (k / 16)-th agent
// whose A* search has finished (k_astar publishes agents in completion order), so an agent's corridors start the moment
// ITS search is done — not when the slowest search of a group is.  The wave extracts the segment's obstacle points itself,
// runs FIRI / MVIE / shrink / validity, and the wave that completes an agent's last segment does the per-agent
// bookkeeping (adjacent intersections, goal projection) and publishes the agent to the QP kernel's ready list.
// Waiting is a bounded spin (s_sleep polling of one word); a timeout raises FlowCtl::err and every kernel of the
// tick drains.  Dynamic LDS: the segment layout's, of which the finishers use the prefix LpLds (sogm_lp.hpp).
// =================================================================================================
__global__ __launch_bounds__(64) void k_worker_flow(MapView m, SogmPlannerParams pp, CorridorWorkspace ws, FlowCtl fc,
                                                    CorridorIO io, FinishArgs f, int n_agents, int wg_f) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x < wg_f) {  // ---- finishing role ----
    for (;;) {
      const int k = flow_ticket(&fc.hdr[FLOW_F_TICKET]);
      if (k >= n_agents) break;
      const int a = flow_wait_slot(fc.f_ready + k, &fc.hdr[FLOW_ERR]);
      if (a < 0) break;
      __threadfence();
      const int  code = finish_agent(f, a, LpLds::carve(smem), lane);
      const bool safe = (code & 1) != 0;
      if (fc.p_ready) {  // the agent's record is final: hand it to the pre-stamp
        __threadfence();
        if (lane == 0) publish_next(fc.p_ready, &fc.hdr[FLOW_P_READY_N], a);
      }
      if (lane == 0) {
        fc.ts[a * 8 + 6] = wall_clock64();
        finish_count(f, a, safe);
      }
    }
    return;
  }
  // ---- corridor role ----
  const int total = n_agents * SOGM_MAX_PIECES;
  for (;;) {
    const int k = flow_ticket(&fc.hdr[FLOW_C_TICKET]);
    if (k >= total) break;
    const int agent = flow_wait_slot(fc.a_ready + k / SOGM_MAX_PIECES, &fc.hdr[FLOW_ERR]);
    if (agent < 0) break;  // timed out / another kernel failed: drain
    __threadfence();        // the search's outputs (route, route_len) were published before the ready slot
    const int seg = k % SOGM_MAX_PIECES;
    if (seg == 0 && lane == 0) fc.ts[agent * 8 + 2] = wall_clock64();
    if (corridor_slot(m, pp, ws, io, agent, seg, smem, fc.seg_done, false, nullptr)) {
      if (lane == 0) fc.ts[agent * 8 + 3] = wall_clock64();
      __threadfence();
      if (lane == 0) publish_next(fc.q_ready, &fc.hdr[FLOW_Q_READY_N], agent);
    }
    __syncthreads();
  }
}

hipError_t launch_worker_flow(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws, const FlowCtl &fc,
                              int n_agents, int n_finish, int n_corridor, const CorridorIO &io, const FinishArgs &f,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_worker_flow, dim3(n_finish + n_corridor), dim3(64), SegmentLds<6>::bytes(pp.pc_capacity), st, m, pp,
                     ws, fc, io, f, n_agents, n_finish);
  return hipGetLastError();
}

hipError_t launch_corridor(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws, int n_agents,
                           const CorridorIO &io, hipStream_t st, int agent0, hipEvent_t ev_map_read) {
  hipLaunchKernelGGL(k_corridor_points, dim3(SOGM_MAX_PIECES, n_agents), dim3(256), 0, st, m, pp, ws, io.start_pva,
                     io.t_start, io.route, io.route_len, io.route_cap, agent0);
  hipError_t e = hipGetLastError();
  // nothing after this point reads the SOGM
  if (e == hipSuccess && ev_map_read) e = hipEventRecord(ev_map_read, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_corridor_segment, dim3(SOGM_MAX_PIECES, n_agents), dim3(64),
                     SegmentLds<6>::bytes(pp.pc_capacity), st, m, pp, ws, io.start_pva, io.t_start, io.route,
                     io.route_len, io.route_cap, agent0);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(k_corridor_finalize, dim3(n_agents), dim3(64), LpLds::bytes(), st, pp, ws, io.start_pva, io.route,
                     io.route_len, io.route_cap, io.out_polys, io.out_nfaces, io.out_npoly, io.out_goal, agent0);
  return hipGetLastError();
}

}  // namespace sogm

// k_flight_light, the other caller of corridor_slot, is compiled in this unit (why: the head of that file)
#include "sogm_flight_light.hpp"

extern "C" int sogm_firi_batched(const double *bd, int n_bd, const double *pc_xyz, const int32_t *pc_range,
                                 const double *a, const double *b, double *r, int iterations, double epsilon, int n,
                                 int max_points, int max_faces, double *out_hpoly, int32_t *out_nfaces,
                                 int32_t *out_status, void *stream) {
  if (n < 0 || n_bd < 1 || n_bd > FIRI_DIRECT_BD_MAX || iterations < 1 || max_points < 1 || max_points > 16384 ||
      max_faces < 1 || max_faces > FIRI_MAX_H ||
      (n > 0 && (!bd || !pc_range || !a || !b || !r || !out_hpoly || !out_nfaces || !out_status)))
    return SOGM_ERR_INVALID_ARG;
  if (n == 0) return SOGM_OK;
  hipStream_t st = (hipStream_t)stream;
  // per-problem scratch (ellipsoid-frame points, tangent planes, distances, debug words): stream-ordered
  const size_t per = sizeof(double) * 8 * (size_t)max_points + sizeof(long long) * 16;
  char        *scratch = nullptr;
  SOGM_HIP_CHECK(hipMallocAsync((void **)&scratch, per * (size_t)n, st));
  sogm::CorridorWorkspace ws{};
  ws.fpc     = (double *)scratch;
  ws.tang    = ws.fpc + (size_t)n * max_points * 3;
  ws.distr   = ws.tang + (size_t)n * max_points * 4;
  ws.seg_dbg = (long long *)(ws.distr + (size_t)n * max_points);
  SogmPlannerParams pp{};
  pp.pc_capacity = max_points;
  sogm::FiriDirect fd{bd, n_bd, pc_xyz, pc_range, a, b, r, iterations, out_hpoly, out_nfaces, out_status,
                      max_faces, 0, epsilon};
  hipLaunchKernelGGL(sogm::k_firi_direct, dim3(n), dim3(64), sogm::SegmentLds<FIRI_DIRECT_BD_MAX>::bytes(max_points), st, sogm::MapView{},
                     pp, ws, fd);
  const hipError_t e = hipGetLastError();
  (void)hipFreeAsync(scratch, st);
  SOGM_HIP_CHECK(e);
  return SOGM_OK;
}

extern "C" int sogm_corridor_rules_batched(sogm_planner *counters_of, const SogmPlannerParams *pp_host,
                                           const double *start_pva, const double *route, const int32_t *route_len,
                                           int route_cap, const double *polys, const int32_t *nfaces,
                                           const int32_t *seg_state, int n, int max_faces, double *out_box,
                                           double *out_shrunk, int32_t *out_seg_nfaces, int32_t *out_seg_state,
                                           double *out_polys, int32_t *out_nfaces, int32_t *out_npoly,
                                           double *out_goal, void *stream) {
  return sogm_corridor_rules_batched_flags(counters_of, pp_host, start_pva, route, route_len, route_cap, polys, nfaces, seg_state,
                                           n, max_faces, out_box, out_shrunk, out_seg_nfaces, out_seg_state, out_polys,
                                           out_nfaces, out_npoly, out_goal, 0, stream);
}

extern "C" int sogm_corridor_rules_batched_flags(sogm_planner *counters_of, const SogmPlannerParams *pp_host,
                                                 const double *start_pva, const double *route, const int32_t *route_len,
                                                 int route_cap, const double *polys, const int32_t *nfaces,
                                                 const int32_t *seg_state, int n, int max_faces, double *out_box,
                                                 double *out_shrunk, int32_t *out_seg_nfaces, int32_t *out_seg_state,
                                                 double *out_polys, int32_t *out_nfaces, int32_t *out_npoly,
                                                 double *out_goal, int flags, void *stream) {
  // route_cap > SOGM_MAX_PIECES: the rules read way-points 0 .. SOGM_MAX_PIECES at most, whatever route_len says
  if ((flags & ~SOGM_RULES_PARALLEL) || ((flags & SOGM_RULES_PARALLEL) && n > (1 << 20)) ||
      n < 0 || max_faces < 1 || max_faces > RULES_MAX_FACES || route_cap <= SOGM_MAX_PIECES ||
      (n > 0 && (!pp_host || !start_pva || !route || !route_len || !polys || !nfaces || !out_box || !out_shrunk ||
                 !out_seg_nfaces || !out_seg_state || !out_polys || !out_nfaces || !out_npoly || !out_goal)))
    return SOGM_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (pp_host[i].max_faces != max_faces) return SOGM_ERR_INVALID_ARG;  // one stride for the whole batch
  if (n == 0) return SOGM_OK;
  hipStream_t        st   = (hipStream_t)stream;
  SogmPlannerParams *d_pp = nullptr;
  SOGM_HIP_CHECK(hipMallocAsync((void **)&d_pp, sizeof(SogmPlannerParams) * (size_t)n, st));
  hipError_t e = hipMemcpyAsync(d_pp, pp_host, sizeof(SogmPlannerParams) * (size_t)n, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // pp_host is the caller's pageable memory
  // the parallel form's control words, zeroed: seg_done [n] | seg_ready [n] | pair_ok [n][SOGM_MAX_PIECES]
  int         *d_ctl = nullptr;
  const size_t n_ctl = (size_t)n + sogm::corridor_pair_words(n);
  if (e == hipSuccess && (flags & SOGM_RULES_PARALLEL)) {
    e = hipMallocAsync((void **)&d_ctl, sizeof(int) * n_ctl, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_ctl, 0, sizeof(int) * n_ctl, st);
  }
  if (e == hipSuccess) {
    sogm::CorridorWorkspace ws{};
    ws.polys      = out_shrunk;
    ws.seg_nfaces = out_seg_nfaces;
    ws.seg_state  = out_seg_state;
    ws.counters   = counters_of ? counters_of->cw.counters : nullptr;
    const sogm::CorridorIO    io{.start_pva = start_pva, .route = route, .route_len = route_len, .route_cap = route_cap,
                                 .out_polys = out_polys, .out_nfaces = out_nfaces, .out_npoly = out_npoly,
                                 .out_goal = out_goal};
    const sogm::CorridorRules cr{d_pp, polys, nfaces, seg_state, out_box};
    if (flags & SOGM_RULES_PARALLEL) {
      ws.seg_ready = reinterpret_cast<unsigned *>(d_ctl + n);
      ws.pair_ok   = d_ctl + 2 * (size_t)n;
      ws.pair_cnt  = counters_of ? counters_of->cw.pair_cnt : nullptr;
      hipLaunchKernelGGL(sogm::k_corridor_rules_slots, dim3(n * SOGM_MAX_PIECES), dim3(64), sogm::RulesLds::bytes(), st, cr, ws,
                         io, d_ctl);
      if (ws.pair_cnt)
        hipLaunchKernelGGL(sogm::k_pairs_residue, dim3(1), dim3(256), 0, st, ws.seg_ready, (int)sogm::corridor_pair_words(n),
                           ws.pair_cnt);
    } else {
      hipLaunchKernelGGL(sogm::k_corridor_rules, dim3(n), dim3(64), sogm::RulesLds::bytes(), st, cr, ws, io);
    }
    e = hipGetLastError();
  }
  if (d_ctl) (void)hipFreeAsync(d_ctl, st);
  (void)hipFreeAsync(d_pp, st);
  SOGM_HIP_CHECK(e);
  return SOGM_OK;
}

// debug aid (not part of include/sogm_abi.h): resident workgroups per CU of the segment kernel
extern "C" int sogm_debug_corridor_occupancy(int pc_capacity) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)sogm::k_corridor_segment, 64,
                                                   sogm::SegmentLds<6>::bytes(pc_capacity)) != hipSuccess)
    return -1;
  return n;
}

#ifdef SOGM_PROFILE_MVIE
extern "C" int sogm_debug_mvie_prof(unsigned long long *out2) {
  if (hipMemcpyFromSymbol(out2, HIP_SYMBOL(sogm::g_mvie_prof), 16) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out2 + 2, HIP_SYMBOL(sogm::g_lbfgs_prof), 40) != hipSuccess) return -1;
  unsigned long long z[5] = {0, 0, 0, 0, 0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(sogm::g_mvie_prof), z, 16);
  (void)hipMemcpyToSymbol(HIP_SYMBOL(sogm::g_lbfgs_prof), z, 40);
  return 0;
}
#endif
