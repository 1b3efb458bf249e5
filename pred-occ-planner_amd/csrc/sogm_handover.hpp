// sogm_handover.hpp — device-side hand-overs between the persistent kernels: the control blocks, their
// layouts (FlowBlock, UpdateBlock, FlightBlock: what is carved where, what a call resets), the tag arithmetic of their slots, the failure
// codes, ONE bounded wait and ONE publish.  The layouts, the arithmetic and the codes compile on the host too
// (tests/planner_blocks_host_test.cpp, tests/handover_host_test.cpp); everything that runs on the device sits behind __HIPCC__.
#pragma once

#include <cstddef>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

namespace sogm {

// Device-side control block of the dataflow replan (one per planner, reset at the start of every sogm_replan):
// kernels of one tick hand agents to each other through ready lists instead of stream order.
//   hdr[FLOW_*] counters; seg_done[A] finished segment slots per agent; a_ready[A] agents in A* completion order;
//   q_ready[A] agents in corridor completion order (entries are -1 until published).
//   f_ready[A] agents in QP completion order; p_ready[A] agents whose record is published (the finishing blocks of k_worker_flow done), the
//   pre-stamp's input; stage[A] per-agent progress counter of the pre-stamp (0 at the start of a replan).
enum { FLOW_A_RESIDENT = 0, FLOW_A_READY_N = 1, FLOW_C_TICKET = 2, FLOW_Q_READY_N = 3, FLOW_Q_TICKET = 4,
       FLOW_ERR = 5, FLOW_F_READY_N = 6, FLOW_F_TICKET = 7, FLOW_P_READY_N = 8, FLOW_P_TICKET = 9,
       FLOW_Q_RESIDENT = 10 /* QP workgroups that have started */, FLOW_HDR = 11 };
#define FLOW_PS_DONE (1 << 20)  // stage[agent] once the agent's pre-stamp is complete (its last marks ticket sets it)
#define FLOW_TIMEOUT_TICKS 300000000LL  // 3 s of the 100 MHz wall clock: a stuck tick fails instead of hanging
// One polling interval of the waiting loops of the dataflow replan.  A poll is a device-scope load that goes to the
// memory side (the L2s are per XCD) while the SOGM clear streams beside it; the stages waited for take hundreds of
// microseconds, so the waiting waves look every ~14 us (SOGM_POLL_PAUSES x s_sleep 127 = 4 x 3.4 us).
#ifndef SOGM_POLL_PAUSES
#define SOGM_POLL_PAUSES 4
#endif
struct FlowCtl {
  int *hdr;       // [FLOW_HDR]
  int *seg_done;  // [A]
  int *a_ready;   // [A]
  int *q_ready;   // [A]
  int *f_ready;   // [A] agents in QP completion order
  long long *ts;  // [A][8] wall_clock64 stamps (100 MHz): 0 A* start, 1 A* done, 2 first corridor item taken,
                  //        3 corridors final, 4 QP start, 5 QP done, 6 finished, 7 A* workgroup resident
                  //        (diagnostics, always written)
  int *p_ready;   // [A] agents in publication order (null: nobody consumes it)
  int *stage;     // [A]
  const int *map_ready;  // [A] update flow: the agent's map is complete when this holds map_epoch (null: it is already)
  int        map_epoch;
  // the control block's reset runs on the corridor stream, early (under the map update); the searches wait for its
  // generation word in their prologue and zero their agent's outputs there (k_astar; null: nothing to wait for)
  const int *reset_gen;
  int        reset_epoch;
  int32_t   *out_ok;       // [A] this replan's outputs, zeroed per agent by its first search workgroup
  int       *out_records;  // [A][rec_words]
  int        rec_words;
};
// The block's layout (sogm_planner::d_flow), word offsets from its base, the only place that knows it:
//   hdr[FLOW_HDR] | seg_done[A] | stage[A] | a_ready[A] | q_ready[A] | f_ready[A] | p_ready[A] | gen
// Tests and tools read peeked words by these offsets (sogm_debug_flow_peek copies the block in front of `gen`).
struct FlowBlock {
  int seg_done, stage, a_ready, q_ready, f_ready, p_ready;
  int gen;  // the reset's generation word (FlowCtl::reset_gen), the block's last
  constexpr explicit FlowBlock(int A)
      : seg_done(FLOW_HDR), stage(seg_done + A), a_ready(stage + A), q_ready(a_ready + A), f_ready(q_ready + A),
        p_ready(f_ready + A), gen(p_ready + A) {}
  // what k_flow_reset puts back per replan: header, seg_done and stage to 0, the four ready lists to -1
  constexpr int zero_words() const { return a_ready; }  // [0, zero_words)
  constexpr int fill_first() const { return a_ready; }  // [fill_first, fill_first + fill_words)
  constexpr int fill_words() const { return gen - a_ready; }
  static constexpr size_t words(int A) { return (size_t)FlowBlock(A).gen + 1; }
  static void carve(int *base, int A, FlowCtl *fc) {
    const FlowBlock b(A);
    fc->hdr      = base;
    fc->seg_done = base + b.seg_done;
    fc->stage    = base + b.stage;
    fc->a_ready  = base + b.a_ready;
    fc->q_ready  = base + b.q_ready;
    fc->f_ready  = base + b.f_ready;
    fc->p_ready  = base + b.p_ready;
  }
};
// The update flow's control block (sogm_ctx::d_update_ctl; k_update_flow, csrc/sogm_map.hip), word offsets from its base, the
// only place that knows it.  Thousands of waves claim tickets, bump and poll these words — in one 128-byte line that line's
// memory channel is the bottleneck, as the flight's header showed —, so every word has a line of its own:
//   ticket | (unused) | error at word 1024 | (unused) | from word 2048 one progress counter per agent, 32 words apart
// Zeroed as a whole in front of every update flow.
struct UpdateBlock {
  static constexpr int    ticket() { return 0; }
  static constexpr int    err() { return 1024; }
  static constexpr int    stage(int agent) { return 2048 + 32 * agent; }
  static constexpr size_t words(int A) { return (size_t)stage(A); }  // the last agent's line is whole
  // base + stage(agent) for the kernel: the constant part first, so that it is folded into one address in front of the ticket
  // loop and a ticket adds its agent's 32 words to it
  static constexpr int *stage_word(int *base, int agent) { return base + stage(0) + (stage(1) - stage(0)) * agent; }
};
// ---------------------------------------------------------------------------------------------------------------
// Flight (sogm_flight_run): n_ticks replan ticks of every agent in ONE set of launches, every agent on its own clock.
// The reference's drones replan asynchronously, each reading whatever trajectories arrived last
// (plan_manager/src/plan_manager.cpp:92-233, traj_coordinator/src/particles.cpp:179-190).  Here the RESULTS are
// fixed by a staleness rule — agent a's tick k reads its own record of tick k - 1 and the neighbours' records as of
// their tick k - 2 (table ver(k - 2)), and may start once every agent has finished tick k - 2 — and the SCHEDULE is free:
// an agent whose chain is done goes straight on to its next tick while a straggler still solves its QP.
// Four persistent kernels, each on a stream with its own compute units (a CU-masked stream; every mask balanced over
// the shader engines it touches and every launch exactly as large as its mask holds — flight_partition in sogm_flight_layout.hpp: all
// workgroups resident from the first microsecond, which is also what lets a flight survive the hardware scheduler's queue
// save / restore; no residency gates, no dispatch-order assumptions, four hardware queues):
//   k_flight_map     a few admitting waves + role-less one-wave workgroups over ONE work queue of ready map work (a descriptor
//                    is pushed when its prerequisites are complete, so no worker sits waiting on another).  The admitting
//                    waves take agents in the order their previous tick finished and let `flight_admit` maps be under
//                    construction at once: agents leave the map stage one after the other and stay spread over the stages
//                    — a swarm whose agents all share every stage equally moves in step, and then every kernel's compute
//                    units idle while another kernel's are busy.  Head (start state from the own record, cull of
//                    cylinders and cloud blocks of the tick's SogmWorld frame) -> sparse reset of the agent's grid through its
//                    mark log + occupancy bits -> marks -> [gate: every agent has finished tick k - 2] -> neighbour overlay
//                    (the only phase that reads table ver(k - 2)) -> s_ring
//   k_flight_search  one workgroup per (agent, attempt) ticket: hybrid A* (both attempts side by side) -> 16 corridor descriptors
//   k_flight_light   role-less one-wave workgroups over ONE work queue: corridor segments (-> q_ring) and finish items
//                    (deconfliction, record, publication, tick accounting, the agent's next map head descriptor)
//   k_flight_qp      one workgroup per CU: the Bezier QP -> a finish descriptor
// Hand-over to the search and QP kernels: rings in HBM indexed by a monotonic position; a slot holds
// ((position / R + 1) << 16) | agent, so a reader with ticket t takes its item when the slot's generation is t / R + 1
// (R >= 2 A: an agent has one item in flight).  To the one-wave kernels: work queues (below).
// Per-agent buffers (start state, route, polytopes, control points, grid, mark log) are single: an agent's chain is
// strictly sequential.  Swarm tables: a ring of four versions, ver(j) at slot j & 3.
// Every counter of the header sits 4 KiB from the next: idle waves poll words of it, and with all of them in one 128-byte
// line ~900 polling waves saturated that line's memory channel — every claim of every kernel queued behind the polls.
#define FL_STRIDE 1024
enum { FL_S_READY = 0 * FL_STRIDE, FL_S_TICKET = 1 * FL_STRIDE, FL_Q_READY = 2 * FL_STRIDE, FL_Q_TICKET = 3 * FL_STRIDE,
       FL_ERR = 4 * FL_STRIDE, FL_FINISHED = 5 * FL_STRIDE /* agent-ticks finished */,
       FL_MW_TAIL = 6 * FL_STRIDE, FL_MW_HEAD = 7 * FL_STRIDE,   // work queue of the map kernel: descriptors pushed / tickets taken
       FL_LW_TAIL = 8 * FL_STRIDE, FL_LW_HEAD = 9 * FL_STRIDE,   // work queue of the corridor + finish kernel
       FL_M_READY = 10 * FL_STRIDE, FL_M_TICKET = 11 * FL_STRIDE,  // map heads: agents whose previous tick is finished / admitted
       FL_MAPS_DONE = 12 * FL_STRIDE,                               // maps completed (admission control)
       FL_ADMITTED = 13 * FL_STRIDE,                                // heads admitted so far (they are admitted in ticket order)
       FL_PACE_CLOCK = 14 * FL_STRIDE,                              // (two words) wall clock of the last admission
       FL_U_READY = 15 * FL_STRIDE, FL_U_TICKET = 16 * FL_STRIDE,   // urgent lane (below): heads published / taken
       FL_UW_TAIL = 17 * FL_STRIDE, FL_UW_HEAD = 18 * FL_STRIDE,    // urgent lane: map descriptors pushed / tickets taken
       FL_END = 19 * FL_STRIDE,                                     // the epoch of the call whose last agent-tick is finished
       FL_COUNTERS = 20, FL_HDR = 20 * FL_STRIDE };
// The urgent lane of the map kernel.  The flight's rate is the rate of its SLOWEST agent's own chain (tools/diag_flight.py:
// the critical path follows one agent with long corridors / QPs for many ticks in a row), and that agent — always behind,
// never gated — queued like everybody else: behind a burst of leaders the gate had just released (up to 1.3 ms in the
// in-order admission, 0.4 ms for a free head wave) and then shared the map workers with ~24 other maps (1.0 ms for a map
// that takes 0.3 by itself).  The leaders have slack by definition, the laggards have none: an agent that finishes tick k
// among the last `flight_urgent` of the swarm builds the map of its tick k + 1 through a lane of its own — `u_ring` ->
// urgent heads (no admission order, no pace, no window) -> work queue `uw`, which the workers look at before they take
// plain work and while they wait for it, in finer tickets.  The cells, records and logs do not depend on the schedule
// (the staleness rule fixes every input).
// Work queues (map kernel, corridor + finish kernel): ONE FIFO of ready work per kernel.  A producer reserves positions with
// one atomicAdd on the tail and stores a descriptor per position, tagged with the position's generation; a consumer takes a
// ticket with one atomicAdd on the head and waits for ITS position (idle waves therefore poll distinct words).  Every
// published descriptor is taken by the lowest waiting ticket, whatever its kind: no wave ever waits for work that depends
// on work nobody is free to do.  (Two earlier forms: all tickets of an item handed out in order and waiting for each
// other — 512 waves / 61 tickets = 8 maps in flight; a compare-and-swap claim per phase queue — hundreds of waves
// retrying on one counter, the map stage took 5-28 ms per agent and got SLOWER with more waves or tickets.)
// descriptor: kind << 28 | sub << 16 | agent
enum { WK_MAP_HEAD = 0, WK_MAP_RESET = 1, WK_MAP_BITS = 2, WK_MAP_MARKS = 3, WK_MAP_SPLAT = 4, WK_CORRIDOR = 5, WK_FINISH = 6 };
#define FL_TS 16            // stamps per agent-tick (FlightCtl::ts)
#define FL_WQ_SLOTS 131072  // per queue (a tick of 128 agents pushes 8-25 k map descriptors; at most two ticks are in flight)
#define FLIGHT_MAX_TICKS 64
struct FlightCtl {
  int *hdr;                                         // [FL_HDR]
  int *s_ring, *q_ring, *m_ring, *u_ring;           // [ring_mask + 1] each: maps ready for the search, corridors final for the QP,
                                                    // agents whose previous tick is finished (map heads; u_ring: the urgent ones)
  unsigned long long *mw, *lw, *uw;                 // [FL_WQ_SLOTS] work queues of the map / the corridor + finish kernel / the
                                                    // map kernel's urgent lane
  int  ring_mask;
  int *urgent;      // [A] 1: the agent's current tick goes through the urgent lane
  int  n_urgent;    // an agent among the last n_urgent finishers of a tick is urgent in its next one (0: no urgent lane)
  int  n_splat, un_splat;  // overlay tickets of a map in the plain / the urgent lane (the finish that opens a gate queues them)
  int  epoch;              // this call's number (never 0, never repeated while the planner lives): the waves whose work has
                           // no known count leave when hdr[FL_END] holds it — a word the call's last finish stores, compared for
                           // EQUALITY, so that a value left by an earlier call can end nothing (the counters are zeroed by a
                           // kernel before the flight's kernels start, but a poll is a load, and "FINISHED >= all" would
                           // hold for the previous call's final count)
  int  gate_pace_ticks;    // 100 MHz ticks between two overlays that a gate releases (they reach the search and the corridors
                           // one after the other instead of as a burst)
  int *tick_done;   // [FLIGHT_MAX_TICKS] agents that have finished tick first_tick + i
  int *parked_n;    // [FLIGHT_MAX_TICKS] maps of tick first_tick + i whose overlay is parked at the gate "tick i - 2 is complete" ...
  int *parked;      // [FLIGHT_MAX_TICKS][A] ... the agents (-1 empty, -2 released)
  int *xready;      // [FLIGHT_MAX_TICKS] several ranks with the exchange behind the call (SogmFlight::nccl_comm): == epoch once the
                    // all-gather of table ver(first_tick + i) — every rank's rows — has completed here; null: one process owns
                    // every row.  The gate of tick k's overlay is then xready[k - 2] instead of tick_done[k - 2] (which the
                    // collective itself waited for), and the parked overlays are released by the kernel behind the collective
                    // on the exchange stream (k_flight_xsignal) instead of by the finish that completes the tick.
  int *tick_of;     // [A] the tick the agent is in (absolute index)
  int *seg_done;    // [A] cumulative corridor segment slots finished
  int *stage;       // [A] cumulative map tickets finished
  long long *ts;    // [A][FL_TS] stamps of the agent's current tick: 0 A* start, 1 A* done, 2 first corridor item, 3 corridors
                    //         final, 4 QP start, 5 QP done, 6 finished, 7 map item published, 8 map head start, 9 gate passed, 10 marks done, 11 map ready,
                    //         12 head done (reset / bits tickets queued), 13 grid reset and bits set (marks tickets queued),
                    //         14 overlay tickets queued (the gate "tick k - 2 is complete" lies between 10 and 14)
  long long *acc;   // [A][8] sums over the flight (100 MHz ticks): gate wait, map, search queue + A*, corridors, QP queue + QP,
                    //        finish, whole chain, ticks completed
  long long *ts_log;         // [FLIGHT_MAX_TICKS][A][FL_TS] every agent-tick's stamps (sogm_debug_flight_times)
  unsigned long long *prof;  // [16] wave time (100 MHz ticks) by activity, summed over the flight: 0 map workers idle (waiting
                             //      for a descriptor), 1 reset, 2 bits, 3 marks, 4 overlay, 5 heads (incl. their waits),
                             //      6 light waves idle, 7 corridor segments, 8 finish; 9.. descriptor counts of 1-4, 7, 8
  long long *wg_start;       // [8][FL_WG_LOG] ([4..7]: where, HW_ID | XCC_ID << 32) wall clock at which workgroup b of kernel k (0 QP, 1 search, 2 corridor + finish, 3 map)
                             //      executed its first instruction in this call (0: never) — the residency evidence of
                             //      sogm_debug_flight_wg_starts: a workgroup that starts late was NOT resident from the start
  int  n_agents, n_ticks, first_tick;
  int  lag;         // tick k reads the neighbours' records of tick k - lag: 2 (the flight's rule: the most overlap) or 1 (the
                    // reference's staleness — a record one broadcast old, particles.cpp:179-190; tuning key flight_neighbour_lag)
};
// The block's layout (sogm_planner::d_fl), word offsets from its base, the only place that knows it:
//   hdr[FL_HDR] | s_ring | q_ring | m_ring | u_ring (ring(A) each) | mw | lw (2 FL_WQ_SLOTS each) | tick_done | parked_n |
//   xready (FLIGHT_MAX_TICKS each) | tick_of | seg_done | stage | urgent (A each) | parked[FLIGHT_MAX_TICKS][A] | uw (2 FL_WQ_SLOTS)
// Every call zeroes the words in front of `parked` (k_flight_reset; k_flight_seed fills the parked lists); the urgent queue
// lies behind them because its slots and its head / tail words run on over the planner's life (k_flight_reset).
struct FlightBlock {
  int ring;  // slots of each ring: the smallest power of two >= 2 A
  int s_ring, q_ring, m_ring, u_ring, mw, lw, tick_done, parked_n, xready, tick_of, seg_done, stage, urgent, parked, uw;
  int end;   // == words(A)
  static constexpr int ring_of(int A) {
    int r = 1;
    while (r < 2 * A) r <<= 1;
    return r;
  }
  constexpr explicit FlightBlock(int A)
      : ring(ring_of(A)), s_ring(FL_HDR), q_ring(s_ring + ring), m_ring(q_ring + ring), u_ring(m_ring + ring),
        mw(u_ring + ring), lw(mw + 2 * FL_WQ_SLOTS), tick_done(lw + 2 * FL_WQ_SLOTS), parked_n(tick_done + FLIGHT_MAX_TICKS),
        xready(parked_n + FLIGHT_MAX_TICKS), tick_of(xready + FLIGHT_MAX_TICKS), seg_done(tick_of + A), stage(seg_done + A),
        urgent(stage + A), parked(urgent + A), uw(parked + parked_words(A)), end(uw + 2 * FL_WQ_SLOTS) {}
  // the 64-bit queues start on 8 bytes: every term in front of them is even (a ring holds >= 2 slots, A >= 1)
  static_assert(FL_HDR % 2 == 0 && FLIGHT_MAX_TICKS % 2 == 0, "mw, lw and uw must start on even word offsets");
  static constexpr int    parked_words(int A) { return FLIGHT_MAX_TICKS * A; }
  static constexpr int    reset_words(int A) { return FlightBlock(A).parked; }
  static constexpr size_t words(int A) { return (size_t)FlightBlock(A).end; }
  static void carve(int *base, int A, FlightCtl *fl, int **xready_out) {
    const FlightBlock b(A);
    fl->hdr       = base;
    fl->s_ring    = base + b.s_ring;
    fl->q_ring    = base + b.q_ring;
    fl->m_ring    = base + b.m_ring;
    fl->u_ring    = base + b.u_ring;
    fl->mw        = reinterpret_cast<unsigned long long *>(base + b.mw);
    fl->lw        = reinterpret_cast<unsigned long long *>(base + b.lw);
    fl->uw        = reinterpret_cast<unsigned long long *>(base + b.uw);
    fl->ring_mask = b.ring - 1;
    fl->tick_done = base + b.tick_done;
    fl->parked_n  = base + b.parked_n;
    *xready_out   = base + b.xready;  // (FlightCtl::xready is set per call: null without the exchange behind it)
    fl->tick_of   = base + b.tick_of;
    fl->seg_done  = base + b.seg_done;
    fl->stage     = base + b.stage;
    fl->urgent    = base + b.urgent;
    fl->parked    = base + b.parked;
  }
};

// ---------------------------------------------------------------------------------------------------------------
// Tag arithmetic (host and device): the only place where the shifts and masks of the slots appear.
// Ring slot of size R (a power of two >= 2 A): generation << 16 | agent; the generation of position pos is pos / R + 1, so the
// all-zero word a reset leaves matches no position.
constexpr int RING_MAX_AGENTS = 1 << 16;  // agent < 65536 (flight_setup refuses more)
constexpr int ring_want(int pos, int R) { return pos / R + 1; }
constexpr int ring_encode(int pos, int R, int agent) { return (ring_want(pos, R) << 16) | agent; }
constexpr int ring_generation(int tag) { return tag >> 16; }
constexpr int ring_agent(int tag) { return tag & 0xFFFF; }
// a ring takes one item per agent and tick (positions < n_ticks * A) and R >= 2 A: the generation stays far below 2^15, the
// tag positive
constexpr int RING_MAX_GENERATION = FLIGHT_MAX_TICKS / 2 + 1;
static_assert(RING_MAX_GENERATION < (1 << 15), "ring tags must stay positive over a whole flight");
// Work-queue slot: generation << 32 | descriptor; the generation of position pos is pos / FL_WQ_SLOTS + 1 (never 0).
constexpr unsigned           wq_slot(unsigned pos) { return pos % FL_WQ_SLOTS; }
constexpr unsigned           wq_want(unsigned pos) { return pos / FL_WQ_SLOTS + 1u; }
constexpr unsigned long long wq_encode(unsigned pos, unsigned desc) { return ((unsigned long long)wq_want(pos) << 32) | desc; }
constexpr unsigned           wq_generation(unsigned long long tag) { return (unsigned)(tag >> 32); }
constexpr unsigned           wq_desc(unsigned long long tag) { return (unsigned)tag; }
// Descriptor: kind << 28 | sub << 16 | agent.  The consumers return it as an int whose negative values mean "no descriptor",
// so the kind stays below 8.
constexpr int WK_MAX_AGENTS = 1 << 16;  // agent < 65536
constexpr int WK_MAX_SUB    = 1 << 12;  // sub < 4096 (tickets of one phase of one map; corridor segment slots)
static_assert(WK_FINISH < 8, "a descriptor must stay non-negative as an int");
static_assert(WK_MAX_AGENTS == RING_MAX_AGENTS, "rings and descriptors carry the same agents");
constexpr unsigned wk_pack(int kind, int sub, int agent) { return ((unsigned)kind << 28) | ((unsigned)sub << 16) | (unsigned)agent; }
constexpr int      wk_kind(int desc) { return desc >> 28; }
constexpr int      wk_sub(int desc) { return (desc >> 16) & 0xFFF; }
constexpr int      wk_agent(int desc) { return desc & 0xFFFF; }
constexpr unsigned wk_advance_sub(unsigned desc0, int i) { return desc0 + ((unsigned)i << 16); }  // wq_push: sub + i < WK_MAX_SUB

// ---------------------------------------------------------------------------------------------------------------
// Failure codes: what a waiter whose 3 s ran out stores in its control block's error word.  sogm_planner_flow_error and
// sogm_planner_flow_failures return the code of a replan (FlowCtl::hdr[FLOW_ERR]), sogm_flight_stats hdr[4] that of a flight
// (FlightCtl::hdr[FL_ERR]; sogm_planner_flow_failures reports it as 100 + code), sogm_debug_update_flow out[3] that of an
// update flow.  Two values name more than one waiter.  (The same table: DESIGN.md, include/sogm_abi.h, INTEGRATION.md.)
enum FlowCode : int {
  FLOW_CODE_NONE           = 0,   // nothing is raised (k_astar's wait for the reset generation: the finishing kernel's own limit fails the tick)
  FLOW_CODE_RESIDENCY_GATE = 1,   // replan, k_flow_gate: every search workgroup resident (hdr[FLOW_A_RESIDENT])
  FLOW_CODE_READY_SLOT     = 2,   // replan, flow_wait_slot: k_worker_flow: its corridor blocks for a_ready, its finishing blocks for f_ready, k_prestamp_flow for p_ready
  FLOW_CODE_QP_ITEM        = 3,   // replan, k_qp_flow: its q_ready slot
  FLOW_CODE_VERDICT        = 4,   // replan and flight, the second search attempt (k_astar, k_flight_search): the first one's verdict
  FLOW_CODE_STAGE_COUNT    = 6,   // flow_wait_count: a stage counter — k_prestamp_flow and k_update_flow (the lower tickets of the agent's
                                  // stamp), k_flight_map's heads (hdr[FL_MAPS_DONE], the admission window)
  FLOW_CODE_PRESTAMP_GATE  = 7,   // replan, k_prestamp_gate: corridors final, QP workgroups and finishing waves resident
  FLOW_CODE_OVERLAY_STAMP  = 8,   // update behind a pre-stamp, k_splat_neighbours: the agent's stamp complete (stage >= FLOW_PS_DONE)
  FLOW_CODE_RING_ITEM      = 12,  // flight, fl_wait_item: k_flight_search for s_ring, k_flight_qp for q_ring
  FLOW_CODE_WORK_QUEUE     = 15,  // flight, THREE waiters for a work-queue descriptor: wq_take (k_flight_light), wq_take2 and
                                  // wq_take_end (k_flight_map's workers: plain queue, urgent queue)
  FLOW_CODE_MAP_READY      = 16,  // replan beside an update flow, k_astar: the agent's map (FlowCtl::map_ready) ...
  FLOW_CODE_ADMISSION      = 16,  // ... and, in the flight's own error word, k_flight_map's head: its turn (hdr[FL_ADMITTED])
  FLOW_CODE_HEAD_ITEM      = 17,  // flight, fl_wait_item_end: k_flight_map's plain heads for m_ring
};

#ifdef __HIPCC__
__device__ inline void flow_pause() {
#pragma unroll
  for (int i = 0; i < SOGM_POLL_PAUSES; ++i) __builtin_amdgcn_s_sleep(127);
}
__device__ inline int flow_ticket(int *counter) {  // one ticket per wave, uniform
  int k = 0;
  if ((threadIdx.x & 63) == 0) k = atomicAdd(counter, 1);
  return __builtin_amdgcn_readfirstlane(k);
}

// ---------------------------------------------------------------------------------------------------------------
// The bounded wait.  A consumer polls its word with relaxed agent-scope loads (an sc1 load), takes ONE acquire fence once the
// value is there (an acquire per poll would invalidate the CU's L1 every microsecond), gives up when the error word is set,
// and raises its code after FLOW_TIMEOUT_TICKS.  (Deliberately not here: k_clear_gate of sogm_clear.hip, a launch gate with a
// limit of 0.5 s whose running out OPENS it.)
// A policy is a type: what differs between the waiting sites, fixed at compile time.  A site derives from WaitPolicy and
// overrides by name.
struct WaitPolicy {
  static constexpr int  code     = FLOW_CODE_NONE;  // FlowCode raised when the limit runs out
  static constexpr int  sleep    = 0;      // one nap: s_sleep of 8, 32 or 127; 0: flow_pause()
  static constexpr bool timed    = true;   // false: no limit of its own (it ends through the error word, which the timed waiters set)
  static constexpr bool watch    = true;   // false: the error word is not looked at (as k_flow_gate, the verdict and the reset
                                           // generation never did)
  static constexpr bool growing  = false;  // the i-th nap is min(i, cap) + 1 naps long — an idle wave polls less and less
  static constexpr int  end_mask = 0;      // the end word and ...
  static constexpr int  err_mask = 0;      // ... the error word are looked at after every nap whose number & mask == 0
};
struct WaitResidencyGate : WaitPolicy { static constexpr int code = FLOW_CODE_RESIDENCY_GATE; static constexpr int sleep = 8; static constexpr bool watch = false; };  // k_flow_gate
struct WaitReadySlot : WaitPolicy { static constexpr int code = FLOW_CODE_READY_SLOT; };
struct WaitQpItem : WaitPolicy { static constexpr int code = FLOW_CODE_QP_ITEM; };
struct WaitVerdict : WaitPolicy { static constexpr int code = FLOW_CODE_VERDICT; static constexpr bool watch = false; };
struct WaitResetGeneration : WaitPolicy { static constexpr int sleep = 32; static constexpr bool watch = false; };  // k_astar's prologue: silent
struct WaitStageCount : WaitPolicy { static constexpr int code = FLOW_CODE_STAGE_COUNT; };
struct WaitPrestampGate : WaitPolicy { static constexpr int code = FLOW_CODE_PRESTAMP_GATE; };
struct WaitMapReady : WaitPolicy { static constexpr int code = FLOW_CODE_MAP_READY; static constexpr int sleep = 32; };  // (~1 us: on the tick's critical path)
struct WaitAdmission : WaitPolicy { static constexpr int code = FLOW_CODE_ADMISSION; static constexpr int sleep = 8; };
struct WaitUntimed : WaitPolicy { static constexpr bool timed = false; };  // k_flight_xwait: ends through the error word only
struct WaitRingItem : WaitPolicy { static constexpr int code = FLOW_CODE_RING_ITEM; };
struct WaitHeadItem : WaitPolicy { static constexpr int code = FLOW_CODE_HEAD_ITEM; };
struct WaitUrgentHeadItem : WaitPolicy { static constexpr int sleep = 127; static constexpr bool timed = false; };  // the few urgent heads poll every 3.4 us
// a worker without a descriptor: naps of 14 us ... 110 us (cap 7), the end word after every second
struct WaitWorkQueue : WaitPolicy { static constexpr int code = FLOW_CODE_WORK_QUEUE; static constexpr bool growing = true; static constexpr int end_mask = 1; };
// 3.4 us naps — the urgent lane exists for latency, and few waves poll it — the end and error words after every eighth
struct WaitUrgentWorkQueue : WaitPolicy { static constexpr int sleep = 127; static constexpr bool timed = false; static constexpr int end_mask = 7; static constexpr int err_mask = 7; };
// WAVE: called by all lanes of a wave with uniform arguments — every value that steers a branch goes through readfirstlane, so
// that the compiler sees a scalar condition — and the wave's first lane raises the code.  Otherwise: one lane.
template <bool WAVE>
__device__ __forceinline__ int flow_peek(const int *p) {
  const int v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return WAVE ? __builtin_amdgcn_readfirstlane(v) : v;
}
template <class P>
__device__ __forceinline__ void wait_nap(int naps, int cap) {
  const int extra = !P::growing ? 0 : naps < cap ? naps : cap;
  for (int i = 0; i <= extra; ++i) {
    if (P::sleep == 0) flow_pause();
    else __builtin_amdgcn_s_sleep(P::sleep);
  }
}
// after the naps-th nap: 0 = poll again, -2 = the end word holds `epoch` (null: none), -1 = failed (err null: nothing is raised)
template <class P, bool WAVE>
__device__ __forceinline__ int wait_exit(int naps, long long t0, int *err, const int *end_word, int epoch) {
  if (end_word && (naps & P::end_mask) == 0 && flow_peek<WAVE>(end_word) == epoch) return -2;
  if (P::watch && (naps & P::err_mask) == 0 && flow_peek<WAVE>(err) != 0) return -1;
  if (P::timed && wall_clock64() - t0 > FLOW_TIMEOUT_TICKS) {
    if (P::code != FLOW_CODE_NONE && err && (!WAVE || (threadIdx.x & 63) == 0)) atomicExch(err, (int)P::code);
    return -1;
  }
  return 0;
}
// 0 once arrived() holds (it loads through flow_peek<WAVE> and keeps what it saw), or wait_exit's verdict
template <class P, bool WAVE, class Arrived>
__device__ __forceinline__ int bounded_wait(int *err, Arrived arrived, const int *end_word = nullptr, int epoch = 0, int cap = 7) {
  const long long t0 = wall_clock64();
  for (int naps = 0;;) {
    if (arrived()) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      return 0;
    }
    wait_nap<P>(naps++, cap);
    if (const int r = wait_exit<P, WAVE>(naps, t0, err, end_word, epoch)) return r;
  }
}
// the common slot test: *p >= target (a counter; an entry of a ready list with target 0).  The value seen (never negative), or -1
template <class P, bool WAVE>
__device__ __forceinline__ int wait_at_least(int *err, const int *p, int target) {
  int v = 0;
  return bounded_wait<P, WAVE>(err, [&] { return (v = flow_peek<WAVE>(p)) >= target; }) ? -1 : v;
}

// The per-lane form, for a wave whose lanes wait for DIFFERENT words (the overlay behind a pre-stamp, k_splat_neighbours: every
// lane waits for the stage word of its own item's agent).  The loop diverges, so it is written for that: the exits set a flag,
// the lanes meet behind the loop and the ones that succeeded fence there once.  true = *p >= target.
__device__ __forceinline__ bool lane_wait_at_least(const int *p, int target, int *err, int code) {
  const long long t0 = wall_clock64();
  bool            ok = false;
  for (;;) {
    if (flow_peek<false>(p) >= target) {
      ok = true;
      break;
    }
    if (flow_peek<false>(err) != 0) break;
    if (wall_clock64() - t0 > FLOW_TIMEOUT_TICKS) {
      atomicExch(err, code);
      break;
    }
    flow_pause();
  }
  if (ok) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  return ok;
}

// ---- the publish: the item's data is written; ONE lane ----
__device__ inline void publish_next(int *list, int *counter, int value) {  // the next entry of a ready list
  __threadfence();
  const int r = atomicAdd(counter, 1);
  __hip_atomic_store(list + r, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void fl_publish(int *ring, int mask, int *ready_n, int agent) {  // the next position of a ring
  __threadfence();
  const int r = atomicAdd(ready_n, 1);
  __hip_atomic_store(ring + (r & mask), ring_encode(r, mask + 1, agent), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// work queue, producer side (ONE lane): `count` descriptors desc0, desc0 + (1 << 16), ... (consecutive `sub` fields)
__device__ inline void wq_push(unsigned long long *wq, int *tail, unsigned desc0, int count) {
  __threadfence();
  const unsigned base = (unsigned)atomicAdd(tail, count);
  for (int i = 0; i < count; ++i) {
    const unsigned pos = base + (unsigned)i;
    __hip_atomic_store(wq + wq_slot(pos), wq_encode(pos, wk_advance_sub(desc0, i)), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the wave-uniform waiters of the ready lists, rings and work queues ----
// the entry of a ready list (>= 0), or -1: the tick failed
__device__ __forceinline__ int flow_wait_slot(int *slot, int *err) { return wait_at_least<WaitReadySlot, true>(err, slot, 0); }
__device__ __forceinline__ int flow_wait_count(int *p, int target, int *err) {  // 0 once *p >= target, or -1
  return wait_at_least<WaitStageCount, true>(err, p, target) < 0 ? -1 : 0;
}
// the agent at ring position `pos` (-1 = the flight failed).  With an end word, for the map kernel's lanes, whose item counts
// are not known in advance (an agent-tick goes through the plain or the urgent lane): -2 once the call's last agent-tick
// is finished (hdr[FL_END] == epoch).
template <class P>
__device__ __forceinline__ int fl_wait_ring(const int *ring, int mask, int pos, int *err, const int *end_word, int epoch) {
  const int want = ring_want(pos, mask + 1);
  int       v    = 0;
  const int r    = bounded_wait<P, true>(
      err, [&] { return ring_generation(v = flow_peek<true>(ring + (pos & mask))) == want; }, end_word, epoch);
  return r ? r : ring_agent(v);
}
__device__ __forceinline__ int fl_wait_item(const int *ring, int mask, int pos, int *err) {
  return fl_wait_ring<WaitRingItem>(ring, mask, pos, err, nullptr, 0);
}
// `timed` = false: the urgent lane may see no item for a whole flight; a stalled flight ends through the other waiters' limits
// and `err`
__device__ __forceinline__ int fl_wait_item_end(const int *ring, int mask, int pos, int *err, const int *end_word, int epoch,
                                                bool timed) {
  return timed ? fl_wait_ring<WaitHeadItem>(ring, mask, pos, err, end_word, epoch)
               : fl_wait_ring<WaitUrgentHeadItem>(ring, mask, pos, err, end_word, epoch);
}
// work queue, consumer side: is the descriptor of position `pos` there?
__device__ __forceinline__ bool wq_arrived(const unsigned long long *wq, unsigned pos, unsigned want, int &desc) {
  const unsigned long long v = __hip_atomic_load(wq + wq_slot(pos), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (__builtin_amdgcn_readfirstlane(wq_generation(v)) != want) return false;
  desc = (int)__builtin_amdgcn_readfirstlane(wq_desc(v));
  return true;
}
template <class P>
__device__ __forceinline__ int wq_wait(const unsigned long long *wq, unsigned pos, int *err, const int *end_word, int epoch) {
  const unsigned want = wq_want(pos);
  int            desc = 0;
  const int      r    = bounded_wait<P, true>(err, [&] { return wq_arrived(wq, pos, want, desc); }, end_word, epoch);
  return r ? r : desc;
}
// the descriptor at position `pos` (-1 = the flight failed)
__device__ __forceinline__ int wq_take(const unsigned long long *wq, unsigned pos, int *err) {
  return wq_wait<WaitWorkQueue>(wq, pos, err, nullptr, 0);
}
// the same with the end-of-flight exit (see fl_wait_item_end): -2 = every agent-tick is finished
__device__ __forceinline__ int wq_take_end(const unsigned long long *wq, unsigned pos, int *err, const int *end_word, int epoch,
                                           bool timed) {
  return timed ? wq_wait<WaitWorkQueue>(wq, pos, err, end_word, epoch) : wq_wait<WaitUrgentWorkQueue>(wq, pos, err, end_word, epoch);
}
// A worker of a kernel with a plain FIFO and a priority queue.  It holds a ticket of the plain queue, as wq_take's callers do,
// and looks at the priority queue first — before it takes its plain descriptor and while it waits for it — claiming a
// priority descriptor that is THERE with a compare-and-swap on that queue's head (never a ticket for one that is not: a
// worker must not be lost to the plain queue waiting for priority work; one try per look, so the waves do not spin on the
// counter).  Returns the descriptor (>= 0; `prio` says from which queue), -2 once every agent-tick of the flight is finished
// (the queues' item counts are not known in advance), -1 if the flight failed.  Wave-uniform.  The loop is bounded_wait's with
// the look at the priority queue in front of the slot test (naps of WaitWorkQueue, cap `max_naps`).
struct WqWorker {
  bool     have_plain = false;
  unsigned plain_t    = 0;
  int      seen_ph    = 0;
};
__device__ __forceinline__ int wq_take2(const unsigned long long *plain, int *plain_head, const unsigned long long *prioq,
                                        int *prio_tail, int *prio_head, WqWorker &w, bool look, int max_naps, int *err,
                                        const int *end_word, int epoch, bool &prio) {
  const long long t0 = wall_clock64();
  prio               = false;
  for (int naps = 0;;) {
    if (look) {
      const int pt = flow_peek<true>(prio_tail);
      if (pt - w.seen_ph > 0) {
        const int h = flow_peek<true>(prio_head);
        w.seen_ph   = h;
        if (pt - h > 0) {
          int got = 0;
          if ((threadIdx.x & 63) == 0) {
            int e = h;
            got   = __hip_atomic_compare_exchange_strong(prio_head, &e, h + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT) ? 1 : 0;
          }
          if (__builtin_amdgcn_readfirstlane(got)) {  // position h is reserved by its producer: the descriptor is there or about to be
            prio = true;
            return wq_take_end(prioq, (unsigned)h, err, end_word, epoch, false);
          }
        }
      }
    }
    if (!w.have_plain) {
      w.plain_t    = (unsigned)flow_ticket(plain_head);
      w.have_plain = true;
    }
    int desc;
    if (wq_arrived(plain, w.plain_t, wq_want(w.plain_t), desc)) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      w.have_plain = false;
      return desc;
    }
    wait_nap<WaitWorkQueue>(naps++, max_naps);
    if (const int r = wait_exit<WaitWorkQueue, true>(naps, t0, err, end_word, epoch)) return r;
  }
}

// ---- the gate of the staleness rule in front of tick kl's overlay (kl relative to first_tick): is table ver(kl - lag) complete? ----
__device__ inline bool fl_gate_open(const FlightCtl &fl, int kl) {
  if (kl < fl.lag) return true;  // (versions of an earlier call: complete before this call's kernels started)
  if (fl.xready) return __hip_atomic_load(&fl.xready[kl - fl.lag], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == fl.epoch;
  return __hip_atomic_load(&fl.tick_done[kl - fl.lag], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= fl.n_agents;
}
// table ver(kl - 2) has just become complete: queue the overlays of tick kl that were parked at the gate so far (ONE lane;
// the parking side re-checks the gate after it has written its slot: list + compare-and-swap on both sides)
__device__ inline void fl_gate_release(const FlightCtl &fl, int kl) {
  const int A_ = fl.n_agents;
  __threadfence();
  int      *lst = fl.parked + (size_t)kl * A_;
  const int n   = __hip_atomic_load(&fl.parked_n[kl], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
  for (int i = 0; i < n && i < A_; ++i) {
    const int v = __hip_atomic_load(&lst[i], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if (v >= 0 && atomicCAS(&lst[i], v, -2) == v) {
      const bool u = fl.urgent[v] != 0;
      if (fl.gate_pace_ticks > 0 && i > 0) {
        const long long p0 = wall_clock64();
        while (wall_clock64() - p0 < fl.gate_pace_ticks) __builtin_amdgcn_s_sleep(32);
      }
      fl.ts[(size_t)v * FL_TS + 14] = wall_clock64();
      wq_push(u ? fl.uw : fl.mw, &fl.hdr[u ? FL_UW_TAIL : FL_MW_TAIL], wk_pack(WK_MAP_SPLAT, 0, v), u ? fl.un_splat : fl.n_splat);
    }
  }
}
#endif

}  // namespace sogm
