// sogm_flight.hip — host side of the flight (sogm_flight_run, described in sogm_handover.hpp / sogm_abi.h): its set-up, the call
// itself as its steps, sogm_flight_prepare, the dumps and the statistics, and the small kernels that reset, seed and report.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <new>

#include "sogm_flight_layout.hpp"
#include "sogm_planner.hpp"

using namespace sogm;

// ---------------------------------------------------------------------------------------------------------------
// sogm_flight_run (the flight is described in sogm_planner.hpp / sogm_abi.h)
// ---------------------------------------------------------------------------------------------------------------
// control block back to its start values: header / rings / counters 0, every agent's first map item published in agent
// order, tick_of = first_tick, verdicts 0 (their tags are absolute tick numbers), the flight's log cleared (an agent-tick
// that does not complete reports ok = 0 and an empty record)
// pairs: the corridors' ready words and pair verdicts (CorridorWorkspace::seg_ready, one block with pair_ok), which an aborted
// flight or a drained replan may have left set
__global__ __launch_bounds__(256) void k_flight_reset(FlightCtl fl, int n_words, int *verdict, long long *acc, int *log_words,
                                                      long long n_log_words, unsigned *pairs, int n_pairs) {
  const long long i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x, step = (long long)gridDim.x * blockDim.x;
  // header, rings, plain queues, tick_done, tick_of, seg_done, stage: one block (FlightBlock::reset_words).  NOT the head / tail words of the urgent
  // queue: its consumers decide "a descriptor is there" by LOADING tail and head (every other hand-over of the flight is a
  // read-modify-write or a generation-tagged slot), so the queue runs on over the planner's life instead of restarting
  // with every call: positions only grow (modulo 2^32; a slot's generation tag follows its position), and a value a
  // consumer reads late can only be LOWER than the true one — it then looks again — never claim a descriptor that
  // does not exist yet.
  for (long long i = i0; i < n_words; i += step)
    if (i != FL_UW_TAIL && i != FL_UW_HEAD) fl.hdr[i] = 0;
  if (i0 == 0) fl.hdr[FL_UW_HEAD] = fl.hdr[FL_UW_TAIL];  // (descriptors an aborted call left behind are skipped)
  for (long long i = i0; i < n_log_words; i += step) log_words[i] = 0;
  for (long long i = i0; i < fl.n_agents; i += step) verdict[i] = 0;
  for (long long i = i0; i < n_pairs; i += step) pairs[i] = 0u;
  for (long long i = i0; i < 8ll * fl.n_agents; i += step) acc[i] = 0;
  for (long long i = i0; i < 16; i += step) fl.prof[i] = 0ull;
  for (long long i = i0; i < 8 * FL_WG_LOG; i += step) fl.wg_start[i] = 0;
}
__global__ __launch_bounds__(256) void k_flight_seed(FlightCtl fl) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < fl.n_agents) {
    fl.tick_of[a] = fl.first_tick;
    fl.m_ring[a]  = ring_encode(a, fl.ring_mask + 1, a);               // position a, generation 1: every agent's first head, in agent order
    fl.ts[(size_t)a * FL_TS + 7] = wall_clock64();  // the head's publication
  }
  if (a == 0) fl.hdr[FL_M_READY] = fl.n_agents;
  for (int i = a; i < FlightBlock::parked_words(fl.n_agents); i += (int)(gridDim.x * blockDim.x)) fl.parked[i] = -1;
}
// the exchange behind a multi-rank flight (sogm_flight_run with SogmFlight::nccl_comm), on the exchange stream, per tick i of the
// call: k_flight_xwait -> ncclAllGather(rows of ver(first_tick + i)) -> k_flight_xsignal
__global__ void k_flight_xwait(FlightCtl fl, int i) {  // every local agent has finished tick i: its rows of the version are final
  if (threadIdx.x != 0) return;
  // (no limit of its own: every wait INSIDE the flight is bounded and sets the error word, which ends this one — the
  //  collective behind it still runs, its peers are waiting in theirs)
  wait_at_least<WaitUntimed, false>(&fl.hdr[FL_ERR], &fl.tick_done[i], fl.n_agents);
}
__global__ void k_flight_xsignal(FlightCtl fl, int i) {  // every rank's rows of ver(first_tick + i) are here
  if (threadIdx.x != 0) return;
  __threadfence();
  __hip_atomic_store(&fl.xready[i], fl.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  if (i + fl.lag < fl.n_ticks) fl_gate_release(fl, i + fl.lag);
}
__global__ void k_flight_report(const int *__restrict__ hdr, int *__restrict__ host_words) {
  const int e = hdr[FL_ERR];
  if (e != 0) {
    host_words[0] = 100 + e;
    host_words[1] = host_words[1] + 1;
  }
}

static int flight_setup(sogm_planner *p) {
  sogm_ctx *c = p->map;
  const int A = c->n_agents;
  if (p->d_fl) return SOGM_OK;
  if (A >= (1 << 16)) return SOGM_ERR_INVALID_ARG;
  // the four streams' compute units and the launches' sizes (flight_partition), in front of the first allocation: a split
  // that cannot be flown leaves d_fl null, and a later call with repaired tuning sets up
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  const bool      masks = c->tune_i(SOGM_TUNE_FLIGHT_MASKS) != 0;
  const int       n_se = c->tune_i(SOGM_TUNE_FLIGHT_ENGINES), se0 = c->tune_i(SOGM_TUNE_FLIGHT_ENGINE_FIRST);
  const int       units[3] = {c->tune_i(SOGM_TUNE_FLIGHT_QP_UNITS), c->tune_i(SOGM_TUNE_FLIGHT_SEARCH_UNITS),
                              c->tune_i(SOGM_TUNE_FLIGHT_MAP_UNITS)};
  FlightPartition part;
  switch (flight_partition(n_cu, n_se, se0, c->tune_i(SOGM_TUNE_FLIGHT_EXCHANGE_UNITS), units[0], units[1], units[2], masks,
                           c->tune_i(SOGM_TUNE_FLIGHT_LIGHT_PER_CU), c->tune_i(SOGM_TUNE_FLIGHT_MAP_PER_CU), &part)) {
    case FLIGHT_PARTITION_OK: break;
    case FLIGHT_PARTITION_NO_REST:
      sogm::set_error_text("sogm_flight_run: flight_qp_units + flight_search_units + flight_map_units must leave a unit for the corridor kernel");
      return SOGM_ERR_INVALID_ARG;
    case FLIGHT_PARTITION_UNPLACEABLE: {
      char text[256];
      std::snprintf(text, sizeof(text), "sogm_flight_run: flight_qp_units = %d, flight_search_units = %d, flight_map_units = %d is a split "
                    "that cannot be placed on %d shader engines (every kernel needs the same share of each engine it touches)",
                    units[0], units[1], units[2], se0 + n_se > 4 ? 4 - se0 : n_se);
      sogm::set_error_text(text);
      return SOGM_ERR_INVALID_ARG;
    }
  }
  sogm::Resources::Setup setup(p->res);
  SOGM_HIP_CHECK(p->res.device(&p->d_fl, sizeof(int) * FlightBlock::words(A), true));  // (once: the urgent / priority queues start empty at position 0)
  FlightBlock::carve(p->d_fl, A, &p->fl, &p->fl_xready);
  p->fl.n_agents  = A;
  SOGM_HIP_CHECK(p->res.device(&p->fl.ts, sizeof(long long) * FL_TS * (size_t)A, true));
  SOGM_HIP_CHECK(p->res.device(&p->fl.acc, sizeof(long long) * 8 * (size_t)A, true));
  SOGM_HIP_CHECK(p->res.device(&p->fl.ts_log, sizeof(long long) * FL_TS * (size_t)A * FLIGHT_MAX_TICKS));
  SOGM_HIP_CHECK(p->res.device(&p->fl.wg_start, sizeof(long long) * 8 * FL_WG_LOG));
  SOGM_HIP_CHECK(p->res.device(&p->fl.prof, sizeof(unsigned long long) * 16, true));
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_worlds, sizeof(FlightWorld) * FLIGHT_MAX_TICKS));
  SOGM_HIP_CHECK(p->res.pinned(&p->h_fl_worlds, sizeof(FlightWorld) * FLIGHT_MAX_TICKS, hipHostMallocDefault));
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_pva, sizeof(double) * 9 * (size_t)A));
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_tstart, sizeof(double) * (size_t)A));
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_now, sizeof(double) * (size_t)A));
  // the head's hand-over arrays of the FSM mode (sogm_planner_set_flight_fsm)
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_due, sizeof(int32_t) * (size_t)A));
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_reached, sizeof(int32_t) * (size_t)A));
  SOGM_HIP_CHECK(p->res.device(&p->d_fl_posnow, sizeof(double) * 3 * (size_t)A));
  for (int k = 0; k < 4; ++k) {
    if (masks)
      SOGM_HIP_CHECK(p->res.stream_masked(&p->fl_stream[k], (uint32_t)((n_cu + 31) / 32), part.mask[k]));
    else
      SOGM_HIP_CHECK(p->res.stream(&p->fl_stream[k]));
    SOGM_HIP_CHECK(p->res.event(&p->fl_ev_done[k]));
    p->fl_cus[k] = part.cus[k];
    p->fl_wgs[k] = part.wgs[k];
  }
  SOGM_HIP_CHECK(p->res.event(&p->fl_ev_in));
  SOGM_HIP_CHECK(hipStreamSynchronize(nullptr));
  return setup.done();
}

#ifdef SOGM_FLIGHT_TRACE
#include <chrono>
#define FL_TRACE(what) std::fprintf(stderr, "FLTRACE %p %s %.3f ms\n", (void *)p, what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count())
#else
#define FL_TRACE(what) (void)0
#endif
// The steps of sogm_flight_run, each called once and in this order.
// 1. the arguments and the planner's state; *xchg: the exchange runs behind the call (k_flight_xwait / xsignal)
static int flight_check_call(const sogm_planner *p, const SogmFlight *f, bool *xchg_out, int *lag_out) {
  if (!p || !f || f->n_ticks < 1 || f->n_ticks > FLIGHT_MAX_TICKS || f->first_tick < 0 || !f->worlds || !f->goals ||
      !f->drone_ids || !f->hover_inout || !f->own_inout || !f->tables || !f->log_records || !f->log_ok || !(f->period > 0))
    return SOGM_ERR_INVALID_ARG;
  sogm_ctx *c = p->map;
  const int A = c->n_agents;
  if (f->n_total < A || f->agent0 < 0 || f->agent0 + A > f->n_total) return SOGM_ERR_INVALID_ARG;
  if (p->fl_fsm_on && f->n_total != A) {
    sogm::set_error_text("sogm_flight_run: under sogm_planner_set_flight_fsm a flight has n_total == n_agents (one process owns every row)");
    return SOGM_ERR_INVALID_ARG;
  }
  const bool xchg = f->n_total != A && f->nccl_comm != nullptr;  // the exchange runs behind the call (k_flight_xwait / xsignal)
  const int lag = c->tune_i(SOGM_TUNE_FLIGHT_NEIGHBOUR_LAG) == 1 ? 1 : 2;
  if (f->n_total != A && !xchg && f->n_ticks > lag) {
    // several ranks, no communicator: the rows of the OTHER ranks' agents in ver(k - 2) must be complete before tick k starts,
    // and only the host can put them there (an all-gather of the finished versions between two calls): two ticks per call
    sogm::set_error_text("sogm_flight_run: with n_total > n_agents (other ranks' rows in the tables) and no nccl_comm a call flies at most two ticks");
    return SOGM_ERR_INVALID_ARG;
  }
  if (!p->flow || !c->sparse || !c->d_body || c->n_body <= 0) return SOGM_ERR_STATE;
  *xchg_out = xchg;
  *lag_out  = lag;
  return SOGM_OK;
}
// 2. what the tuning asks of the work queues and the grid's geometry of the kernels' 32-byte accesses
static int flight_check_capacity(const sogm_ctx *c, size_t *agent_bytes_out) {
  const int A = c->n_agents;
  {  // the work queues hold the descriptors of two ticks at most (an agent is at most one tick ahead of the slowest)
    const long long per_tick = (long long)A * (1 + c->tune_i(SOGM_TUNE_FLIGHT_RESET) + c->tune_i(SOGM_TUNE_FLIGHT_BITS) +
                                               c->tune_i(SOGM_TUNE_FLIGHT_MARKS) + c->tune_i(SOGM_TUNE_FLIGHT_SPLAT));
    if (2 * per_tick > FL_WQ_SLOTS || 2ll * A * (SOGM_MAX_PIECES + 1) > FL_WQ_SLOTS) {
      sogm::set_error_text("sogm_flight_run: agents x tickets per tick exceed the work queue (lower flight_marks / flight_bits)");
      return SOGM_ERR_CAPACITY;
    }
  }
  const size_t agent_bytes = (size_t)c->spec.T * (size_t)c->geom.V * c->cell_bytes();
  if (agent_bytes % 32 != 0 || (reinterpret_cast<uintptr_t>(c->d_grid) & 31) != 0) {
    sogm::set_error_text("sogm_flight_run: agent grids must be 32-byte aligned (V * T * cell bytes a multiple of 32)");
    return SOGM_ERR_INVALID_ARG;
  }
  *agent_bytes_out = agent_bytes;
  return SOGM_OK;
}
// 3. the call's frames into the pinned staging array, crop lists for the largest of them, and the grid the flight builds into
static int flight_stage_frames(sogm_planner *p, const SogmFlight *f, hipStream_t main, sogm::FlightMapDev &md) {
  sogm_ctx *c = p->map;
  int max_blocks = 0;
  for (int i = 0; i < f->n_ticks; ++i) {
    const SogmWorld &w = f->worlds[i];
    if (!w.cloud_xyz || !w.block_bounds || w.n_points < 0 || w.block_points < 64 || w.block_points > 4096 ||
        w.n_blocks != (w.n_points + w.block_points - 1) / w.block_points || w.n_cyl < 0 || (w.n_cyl > 0 && !w.cylinders))
      return SOGM_ERR_INVALID_ARG;
    if (w.n_blocks > max_blocks) max_blocks = w.n_blocks;
    p->h_fl_worlds[i] = FlightWorld{w.cloud_xyz, w.block_bounds, w.cylinders, w.n_points, w.n_blocks, w.block_points, w.n_cyl};
  }
  {
    SogmWorld big = f->worlds[0];  // (only its block count sizes the lists)
    big.n_blocks  = max_blocks;
    big.n_points  = max_blocks * big.block_points;
    if (int rc = sogm::world_blocks(c, &big, &md.cb)) return rc;
    md.cb.n_blocks = max_blocks;  // (per frame in the kernel; the lists' row length is md.cb.row = the context's capacity)
  }
  // the agent's single grid of the flight is the context's current one; it must be covered by its mark log
  // (a pooled tick path may have left a spare grid queued: nothing to adopt here)
  const int slot = c->pool.current();
  if (!c->pool.loggable(slot)) {
    if (int rc = sogm::launch_clear(c, main, c->d_grid, false)) return rc;  // dense, once; restarts the log
    if (!c->pool.loggable(slot)) {
      sogm::set_error_text("sogm_flight_run: the current grid has no mark log (sogm_set_sparse_reset)");
      return SOGM_ERR_STATE;
    }
  }
  return sogm::map_target(c, slot, false, nullptr, &md.tgt);
}
// 4. the control block's per-call fields and the map role's arguments from the call and the tuning: no HIP call
static void flight_args(const sogm_planner *p, const SogmFlight *f, bool xchg, int lag, size_t agent_bytes, FlightCtl &fl,
                        sogm::FlightMapDev &md) {
  const sogm_ctx *c = p->map;
  const int       A = c->n_agents;
  fl             = p->fl;
  fl.xready      = xchg ? p->fl_xready : nullptr;
  fl.lag         = lag;
  fl.n_ticks     = f->n_ticks;
  fl.first_tick  = f->first_tick;
  md.worlds      = p->d_fl_worlds;
  md.ov          = {.rec = nullptr, .n_rec = 0, .ego_ids = f->drone_ids, .body = c->d_body, .n_body = c->n_body};
  md.tables      = f->tables;
  md.n_total     = f->n_total;
  md.tick        = {.own = f->own_inout, .hover = f->hover_inout, .now = p->d_fl_now, .t_start = p->d_fl_tstart,
                    .pva = p->d_fl_pva, .start_offset = f->replan_start_offset};
  md.t0          = f->t0;
  md.period      = f->period;
  md.n_reset     = c->tune_i(SOGM_TUNE_FLIGHT_RESET);
  md.n_bits      = c->tune_i(SOGM_TUNE_FLIGHT_BITS);
  md.n_marks     = c->tune_i(SOGM_TUNE_FLIGHT_MARKS);
  md.n_splat     = c->tune_i(SOGM_TUNE_FLIGHT_SPLAT);
  md.n_head_wgs  = c->tune_i(SOGM_TUNE_FLIGHT_HEADS) < p->fl_wgs[3] / 2 ? c->tune_i(SOGM_TUNE_FLIGHT_HEADS)
                                                                        : (p->fl_wgs[3] / 2 > 0 ? p->fl_wgs[3] / 2 : 1);
  // the urgent lane (sogm_planner.hpp): a few heads and a share of the workers, none with flight_urgent = 0
  fl.n_urgent    = c->tune_i(SOGM_TUNE_FLIGHT_URGENT) < A ? c->tune_i(SOGM_TUNE_FLIGHT_URGENT) : A - 1;
  if (fl.n_urgent < 0) fl.n_urgent = 0;
  md.n_uhead_wgs = 0;
  md.n_uwork_wgs = 0;
  {
    const int fine = c->tune_i(SOGM_TUNE_FLIGHT_URGENT_FINE);
    auto      cut  = [fine](int n, int hi) { return n * fine < hi ? n * fine : hi; };
    md.un_reset = cut(md.n_reset, 256);
    md.un_bits  = cut(md.n_bits, 256) > 2 * md.n_bits ? 2 * md.n_bits : cut(md.n_bits, 256);  // (bits tickets are short already)
    md.un_marks = cut(md.n_marks, 256);
    md.un_splat = cut(md.n_splat, 64);
  }
  fl.gate_pace_ticks = (int)(c->tune[SOGM_TUNE_FLIGHT_GATE_PACE_US] * 100.0);
  fl.epoch    = p->fl_epoch;
  fl.n_splat  = md.n_splat;
  fl.un_splat = md.un_splat;
  if (fl.n_urgent > 0) {
    const int workers = p->fl_wgs[3] - md.n_head_wgs;
    md.n_uhead_wgs = md.n_head_wgs >= 8 ? 4 : md.n_head_wgs / 2;
    md.n_uwork_wgs = c->tune_i(SOGM_TUNE_FLIGHT_URGENT_WAVES) < workers ? c->tune_i(SOGM_TUNE_FLIGHT_URGENT_WAVES) : workers;
    if (md.n_uhead_wgs < 1 || md.n_uwork_wgs < 1) fl.n_urgent = 0, md.n_uhead_wgs = 0, md.n_uwork_wgs = 0;
  }
  md.n_admit     = c->tune_i(SOGM_TUNE_FLIGHT_ADMIT);
  md.pace_ticks  = (int)(c->tune[SOGM_TUNE_FLIGHT_PACE_US] * 100.0);
  md.agent_bytes = agent_bytes;
  md.reset_stat  = c->d_reset_stat;
  // the per-agent FSM (sogm_planner_set_flight_fsm); all null: off
  sogm::FlightFsmDev fd{};
  if (p->fl_fsm_on) {
    const SogmFlightFsm &u = p->fl_fsm;
    fd = sogm::FlightFsmDev{.prm = u.prm, .check_duration = u.check_duration, .state = u.state_inout, .goals = f->goals,
                            .due = p->d_fl_due, .reached = p->d_fl_reached, .pos_now = p->d_fl_posnow,
                            .log_state = u.log_state, .log_due = u.log_due, .log_safe = u.log_safe,
                            .log_reached = u.log_reached, .log_pub = u.log_pub, .log_hover_start = u.log_hover_start,
                            .log_own = u.log_own};
  }
  md.fsm = fd;
}
// 5. frames + control block, in stream order on the caller's stream; the four streams wait for them
static int flight_reset_and_seed(sogm_planner *p, const SogmFlight *f, const FlightCtl &fl, hipStream_t main) {
  const int A = p->map->n_agents;
  SOGM_HIP_CHECK(hipMemcpyAsync(p->d_fl_worlds, p->h_fl_worlds, sizeof(FlightWorld) * (size_t)f->n_ticks, hipMemcpyHostToDevice, main));
  const int       n_words = FlightBlock::reset_words(A);  // (the parked lists: k_flight_seed)
  const long long n_log  = (long long)f->n_ticks * A * (long long)(sizeof(SogmTrajRecord) / sizeof(int));
  hipLaunchKernelGGL(k_flight_reset, dim3(256), dim3(256), 0, main, fl, n_words, p->aw.verdict, p->fl.acc,
                     reinterpret_cast<int *>(f->log_records), n_log, p->cw.seg_ready, (int)corridor_pair_words(A));
  SOGM_HIP_CHECK(hipGetLastError());
  SOGM_HIP_CHECK(hipMemsetAsync(f->log_ok, 0, sizeof(int32_t) * (size_t)f->n_ticks * A, main));
  hipLaunchKernelGGL(k_flight_seed, dim3((A + 255) / 256), dim3(256), 0, main, fl);
  SOGM_HIP_CHECK(hipGetLastError());
  SOGM_HIP_CHECK(hipEventRecord(p->fl_ev_in, main));
  for (int k = 0; k < 4; ++k) SOGM_HIP_CHECK(hipStreamWaitEvent(p->fl_stream[k], p->fl_ev_in, 0));
  FL_TRACE("waits queued");
  return SOGM_OK;
}
// 6. the four launches.  QP first, then search (each wants whole CUs), then the one-wave kernels: with masks the order is immaterial
static int flight_launch(sogm_planner *p, const SogmFlight *f, const FlightCtl &fl, const sogm::FlightMapDev &md) {
  sogm_ctx                 *c  = p->map;
  const MapView             mv = view_of(c);
  const sogm::FlightFsmDev &fd = md.fsm;
  const int spec = c->tune_i(SOGM_TUNE_FLIGHT_SPEC) != 0 ? 1 : 0;
  hipError_t e = sogm::launch_flight_qp(p->pp, p->qs, p->qw, p->qc, fl, p->fl_wgs[0], qp_io(p, p->d_fl_pva), p->fl_stream[0]);
  if (e == hipSuccess) {
    sogm::SearchIO sio = search_io(p, p->d_fl_pva, f->goals, p->d_fl_tstart);
    sio.due            = fd.state ? fd.due : nullptr;  // (never sogm_planner_set_due's mask)
    e = sogm::launch_flight_search(mv, p->ap, p->pp.corridor_tau, astar_ws(p), fl, p->fl_wgs[1], sio, spec, p->fl_stream[1]);
  }
  if (int rc = launched("sogm_flight_run: launch", e)) {
    (void)hipDeviceSynchronize();
    return rc;
  }
  FL_TRACE("qp + search launched");
  sogm::FlightLightDev ld{};
  ld.cor = corridor_io(p, p->d_fl_pva, p->d_fl_tstart);
  // (the flight's swarm is its ring of tables: the kernel sets swarm / pub_table / out / out_ok per tick, null here)
  ld.fin = sogm::FinishArgs{.corridor_tau = p->pp.corridor_tau, .ret = p->d_ret, .npoly = p->d_npoly,
                            .status = p->d_status, .cpts = p->d_cpts, .n_swarm = f->n_total, .swarm_ego = f->drone_ids,
                            .swarm_now = p->d_fl_now, .t_start = p->d_fl_tstart, .drone_ids = f->drone_ids,
                            .out_safe = p->d_safe, .counters = p->cw.counters, .pub_own = f->own_inout,
                            .due = fd.state ? fd.due : nullptr};
  ld.fsm         = fd;
  ld.tables      = f->tables;
  ld.n_total     = f->n_total;
  ld.agent0      = f->agent0;
  ld.log_records = f->log_records;
  ld.log_ok      = f->log_ok;
  e = sogm::launch_flight_light(mv, p->pp, p->cw, fl, ld, p->fl_wgs[2], p->fl_stream[2]);
  if (e == hipSuccess) e = sogm::launch_flight_map(c->geom, fl, md, p->fl_wgs[3], p->fl_stream[3]);
  if (int rc = launched("sogm_flight_run: launch", e)) {
    (void)hipDeviceSynchronize();
    return rc;
  }
  FL_TRACE("light + map launched");
  return SOGM_OK;
}
// 7. (several ranks with a communicator)
static int flight_exchange(sogm_planner *p, const SogmFlight *f, const FlightCtl &fl, hipStream_t main) {
  sogm_ctx *c = p->map;
  const int A = c->n_agents;
  // The exchange behind the call: per tick [wait: every local agent has finished it] -> in-place all-gather of this rank's
  // rows of its table version -> [mark the version complete, queue the overlays parked at its gate], all queued now, on the
  // context's exchange stream, behind the control block's reset.  Every rank queues the same n_ticks collectives; a rank
  // whose flight fails still runs them (the waiting kernel gives up on the error word), so no peer hangs in a collective.
  hipStream_t xs = nullptr;
  if (int rc = sogm::exchange_stream(c, &xs)) return rc;
  SOGM_HIP_CHECK(hipStreamWaitEvent(xs, p->fl_ev_in, 0));
  int rc_x = SOGM_OK;
  for (int i = 0; i < f->n_ticks; ++i) {
    const int       k   = f->first_tick + i;
    SogmTrajRecord *tab = f->tables + (size_t)(k & 3) * f->n_total;
    hipLaunchKernelGGL(k_flight_xwait, dim3(1), dim3(64), 0, xs, fl, i);
    if (rc_x == SOGM_OK)  // (after a failed collective the remaining ones are not attempted: the communicator is broken)
      rc_x = sogm::exchange_allgather_raw(c, f->nccl_comm, tab + f->agent0, tab, sizeof(SogmTrajRecord) * (size_t)A);
    hipLaunchKernelGGL(k_flight_xsignal, dim3(1), dim3(64), 0, xs, fl, i);
    if (i == 0) FL_TRACE("first collective queued");
  }
  FL_TRACE("collectives queued");
  SOGM_HIP_CHECK(hipGetLastError());
  if (int rc = sogm::exchange_mark_pending(c)) return rc;
  if (int rc = sogm::join_exchange(c, main)) return rc;  // the call's last versions are complete when `stream` goes on
  if (rc_x != SOGM_OK) {
    (void)hipDeviceSynchronize();
    return rc_x;
  }
  return SOGM_OK;
}
// 8. fan-in: the caller's stream goes on behind the four kernels and the flight's report
static int flight_fan_in(sogm_planner *p, const SogmFlight *f, hipStream_t main) {
  sogm_ctx *c = p->map;
  for (int k = 0; k < 4; ++k) {
    SOGM_HIP_CHECK(hipEventRecord(p->fl_ev_done[k], p->fl_stream[k]));
    SOGM_HIP_CHECK(hipStreamWaitEvent(main, p->fl_ev_done[k], 0));
  }
  hipLaunchKernelGGL(k_flight_report, dim3(1), dim3(1), 0, main, (const int *)p->fl.hdr, p->h_flow_fail);
  SOGM_HIP_CHECK(hipGetLastError());
  c->updated             = 1;
  c->pool.current_rebuilt();
  c->records_final_valid = 0;
  c->n_stamps += f->n_ticks;
  return SOGM_OK;
}

extern "C" {
int sogm_flight_run(sogm_planner *p, const SogmFlight *f, void *stream) {
  bool xchg = false;
  int  lag  = 2;
  if (int rc = flight_check_call(p, f, &xchg, &lag)) return rc;
  sogm_ctx *c = p->map;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t main = (hipStream_t)stream;
  if (int rc = sogm::join_update(c, main)) return rc;
  if (int rc = sogm::join_prestamp(c, main)) return rc;
  if (int rc = sogm::join_exchange(c, main)) return rc;
  if (int rc = flight_setup(p)) return rc;
  size_t agent_bytes = 0;
  if (int rc = flight_check_capacity(c, &agent_bytes)) return rc;
  sogm::FlightMapDev md{};
  if (int rc = flight_stage_frames(p, f, main, md)) return rc;
  p->fl_epoch = p->fl_epoch >= 0x7ffffff0 ? 1 : p->fl_epoch + 1;  // (never 0: the zeroed word)
  FlightCtl fl;
  flight_args(p, f, xchg, lag, agent_bytes, fl, md);
  if (int rc = flight_reset_and_seed(p, f, fl, main)) return rc;
  if (int rc = flight_launch(p, f, fl, md)) return rc;
  if (xchg)
    if (int rc = flight_exchange(p, f, fl, main)) return rc;
  return flight_fan_in(p, f, main);
}

}  // extern "C"
__global__ void k_flight_touch(int *word) {
  if (threadIdx.x == 0 && word) atomicAdd(word, 0);
}
extern "C" {
// Creates what the first sogm_flight_run would create — control block, the four masked streams, the exchange stream — and
// runs one empty kernel on each, so that their hardware queues EXIST before any flight is in the air, and allocates what the
// first sogm_flight_run would allocate (crop lists for frames of up to max_cloud_points points, the stamp's scratch): that
// first call otherwise synchronises the DEVICE while it grows them.  A host that flies several planners in one process (two
// ranks on one device: tests) calls this for each of them before the first flight — the second rank's first call would
// otherwise wait for the first rank's flight to end, which waits for the second rank's rows.  Optional otherwise.  Synchronises.
int sogm_flight_prepare(sogm_planner *p, int max_cloud_points) {
  if (!p || max_cloud_points < 0) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  if (int rc = flight_setup(p)) return rc;
  {  // everything a first sogm_flight_run would allocate — and synchronise the DEVICE for: the per-agent crop lists for
     // frames of up to max_cloud_points points (blocks of 256), the stamp's scratch
    SogmWorld big{};
    big.block_points = 256;
    big.n_points     = max_cloud_points;
    big.n_blocks     = (max_cloud_points + 255) / 256;
    sogm::CloudBlocks cb{};
    if (int rc = sogm::world_blocks(p->map, &big, &cb)) return rc;
    if (p->map->sparse) {
      // the stamp's scratch, the current grid's mark log (its creation ends with a null-stream memset and synchronisation,
      // which waits for every BLOCKING stream of the process — masked streams are — i.e. for another planner's flight) and the
      // one dense clear that puts the grid under its log
      sogm_ctx       *c = p->map;
      sogm::MapTarget tgt{};
      if (int rc = sogm::map_target(c, c->pool.current(), false, nullptr, &tgt)) return rc;
      if (!c->pool.loggable(c->pool.current()))
        if (int rc = sogm::launch_clear(c, nullptr, c->d_grid, false)) return rc;
    }
  }
  hipStream_t xs = nullptr;
  if (int rc = sogm::exchange_stream(p->map, &xs)) return rc;
  for (int k = 0; k < 4; ++k) hipLaunchKernelGGL(k_flight_touch, dim3(1), dim3(64), 0, p->fl_stream[k], (int *)nullptr);
  hipLaunchKernelGGL(k_flight_touch, dim3(1), dim3(64), 0, xs, (int *)nullptr);
  SOGM_HIP_CHECK(hipGetLastError());
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  return SOGM_OK;
}

// diagnostics (tools/ only): every agent-tick's stamps of the last flight, [n_ticks][A][FL_TS] ticks of 10 ns
int sogm_debug_flight_times(sogm_planner *p, long long *out_host, int n_ticks) {
  if (!p || !p->d_fl || !out_host || n_ticks < 1 || n_ticks > FLIGHT_MAX_TICKS) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->fl.ts_log, sizeof(long long) * FL_TS * (size_t)p->map->n_agents * n_ticks, hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics (tools/ only): the control block of the last flight as it stands — out_words = [FL_COUNTERS header counters]
// [FLIGHT_MAX_TICKS tick_done][FLIGHT_MAX_TICKS parked_n][A tick_of][A seg_done][A stage][A urgent], out_ts = [A][FL_TS]
// stamps of every agent's current tick.  What a stalled flight looked like when it was aborted.
int sogm_debug_flight_dump(sogm_planner *p, int32_t *out_words, int cap_words, long long *out_ts) {
  if (!p || !p->d_fl || !out_words) return SOGM_ERR_INVALID_ARG;
  const int A = p->map->n_agents;
  // the dump's own order, whatever FlightBlock's is: each part through its carved pointer
  const struct { const int *src; int n; } part[] = {{p->fl.tick_done, FLIGHT_MAX_TICKS}, {p->fl.parked_n, FLIGHT_MAX_TICKS},
                                                    {p->fl.tick_of, A}, {p->fl.seg_done, A}, {p->fl.stage, A}, {p->fl.urgent, A}};
  int need = FL_COUNTERS;
  for (const auto &s : part) need += s.n;
  if (cap_words < need) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  for (int i = 0; i < FL_COUNTERS; ++i)
    SOGM_HIP_CHECK(hipMemcpy(out_words + i, p->fl.hdr + (size_t)i * FL_STRIDE, sizeof(int), hipMemcpyDeviceToHost));
  int32_t *o = out_words + FL_COUNTERS;
  for (const auto &s : part) {
    SOGM_HIP_CHECK(hipMemcpy(o, s.src, sizeof(int) * (size_t)s.n, hipMemcpyDeviceToHost));
    o += s.n;
  }
  if (out_ts) SOGM_HIP_CHECK(hipMemcpy(out_ts, p->fl.ts, sizeof(long long) * FL_TS * (size_t)A, hipMemcpyDeviceToHost));
  return SOGM_OK;
}

// diagnostics (tools/, tests/): when every workgroup of the last flight's four kernels started — out_host [8][4096]: [0..3] wall-clock
// ticks (100 MHz; 0 = the workgroup never ran), [4..7] where it started (HW_ID | XCC_ID << 32), out_wgs_host[4] the launched counts (QP, search, corridor + finish, map)
int sogm_debug_flight_wg_starts(sogm_planner *p, long long *out_host, int32_t *out_wgs_host) {
  if (!p || !p->d_fl || !out_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  SOGM_HIP_CHECK(hipMemcpy(out_host, p->fl.wg_start, sizeof(long long) * 8 * FL_WG_LOG, hipMemcpyDeviceToHost));
  if (out_wgs_host)
    for (int k = 0; k < 4; ++k) out_wgs_host[k] = p->fl_wgs[k];
  return SOGM_OK;
}

int sogm_flight_stats(sogm_planner *p, double *out_ms, int32_t *out_hdr) {
  if (!p || !p->d_fl) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(p->map->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  const int A = p->map->n_agents;
  if (out_ms) {
    long long *tmp = new (std::nothrow) long long[8 * (size_t)A];
    if (!tmp) return SOGM_ERR_INVALID_ARG;
    const hipError_t e = hipMemcpy(tmp, p->fl.acc, sizeof(long long) * 8 * (size_t)A, hipMemcpyDeviceToHost);
    for (int i = 0; i < 8 * A; ++i) out_ms[i] = (i % 8) == 7 ? (double)tmp[i] : (double)tmp[i] / 1.0e5;  // 100 MHz -> ms
    delete[] tmp;
    SOGM_HIP_CHECK(e);
  }
  if (out_hdr) {  // the counters, compacted (the device keeps them FL_STRIDE words apart)
    int *tmp = new (std::nothrow) int[FL_HDR];
    if (!tmp) return SOGM_ERR_INVALID_ARG;
    const hipError_t e = hipMemcpy(tmp, p->fl.hdr, sizeof(int) * FL_HDR, hipMemcpyDeviceToHost);
    for (int i = 0; i < 32; ++i) out_hdr[i] = i < 15 ? tmp[(size_t)i * FL_STRIDE] : 0;  // (the urgent lane's four: not reported)
    delete[] tmp;
    SOGM_HIP_CHECK(e);
    {  // [15]: workgroups of the four kernels that were NOT resident from the start (first instruction > 1 ms after the
       // flight's first workgroup): must be 0 — the liveness argument (flight_layout) and tests/test_flight_gpu.py hold it
      long long *ws = new (std::nothrow) long long[4 * FL_WG_LOG];
      if (!ws) return SOGM_ERR_INVALID_ARG;
      const hipError_t e2 = hipMemcpy(ws, p->fl.wg_start, sizeof(long long) * 4 * FL_WG_LOG, hipMemcpyDeviceToHost);
      int late = 0;
      for (int k = 0; k < 4; ++k) {  // per kernel: against ITS first workgroup (the four launches may start a millisecond apart)
        long long first = 0;
        for (int b = 0; b < p->fl_wgs[k] && b < FL_WG_LOG; ++b) {
          const long long v = ws[(size_t)k * FL_WG_LOG + b];
          if (v > 0 && (first == 0 || v < first)) first = v;
        }
        for (int b = 0; b < p->fl_wgs[k] && b < FL_WG_LOG; ++b) {
          const long long v = ws[(size_t)k * FL_WG_LOG + b];
          if (v == 0 || v - first > 100000) ++late;
        }
      }
      delete[] ws;
      SOGM_HIP_CHECK(e2);
      out_hdr[15] = late;
    }
    unsigned long long prof[16];  // [16..31]: wave time by activity in units of 10 us (0-8), descriptor counts (9-15)
    SOGM_HIP_CHECK(hipMemcpy(prof, p->fl.prof, sizeof(prof), hipMemcpyDeviceToHost));
    for (int i = 0; i < 16; ++i) out_hdr[16 + i] = (int32_t)(i < 9 ? prof[i] / 1000ull : prof[i]);
  }
  return SOGM_OK;
}
}  // extern "C"
