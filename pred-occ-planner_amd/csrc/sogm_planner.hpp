// sogm_planner.hpp — planner context + stage launchers shared by the planner translation units.
#pragma once

#include "sogm_device.hpp"
#include "sogm_handover.hpp"

namespace sogm {

// Per-agent A* scratch in HBM (L2-resident while a search runs).
struct AstarWorkspace {
  char  *pool;         // [A][pool_stride] bytes, Node records
  size_t pool_stride;  // bytes per agent
  void  *hkeys;        // [A][hash_cap] 64-bit slots {x, y, z, t, node id}
  int    hash_cap;     // power of two >= 2 * allocate_num
  long long *dbg;      // [A][8] per-phase wall_clock64 ticks (diagnostics)
  // speculative second attempt (dataflow replan): a second set of pools / hash tables ([A..2A)) and the verdict of
  // the first attempt per agent (0 pending, 1 found a path, 2 NO_PATH); null = not available
  int *verdict;
};
int astar_pool_max();

// Per-(agent, segment) corridor scratch in HBM.
struct CorridorWorkspace {
  double  *pc;          // [A*P][cap][3] obstacle points
  double  *fpc;         // [A*P][cap][3] points in the ellipsoid frame
  double  *tang;        // [A*P][cap][4] tangent planes
  double  *distr;       // [A*P][cap]
  double  *polys;       // [A*P][max_faces][4] shrunk polytopes
  int32_t *seg_nfaces;  // [A*P]
  int32_t *seg_state;   // [A*P] 1 valid, 0 invalid, -2 no segment, -3 capacity exceeded
  int32_t *seg_npts;    // [A*P]
  long long *seg_dbg;   // [A*P][16] diagnostics: counts and wall_clock64 ticks (100 MHz) per phase
  unsigned long long *counters;  // [SOGM_CNT_N] cumulative outcome / capacity counters (sogm_planner_counters)
  // Adjacent-pair LPs run as their segments finish (corridor_slot); all null: every pair LP runs in the bookkeeping.
  // seg_ready and pair_ok are ONE allocation (pair_ok = seg_ready + A): zero at creation, zeroed by the wave that finalises
  // the agent, by k_flow_reset per replan and by k_flight_reset per flight (a drained tick leaves bits behind).
  unsigned *seg_ready;           // [A] bit i: segment i's polytope, seg_nfaces and seg_state are stored and fenced
  int32_t  *pair_ok;             // [A*P] pair (i, i + 1): 0 not evaluated, 1 the polytopes intersect, 2 they do not
  unsigned long long *pair_cnt;  // [4] sogm_debug_corridor_pairs: pair LPs run eagerly, run in the bookkeeping behind a verdict
                                 //     of 0, pairs consumed from a verdict, words the parallel rules hook left set
  long long *fin_dbg;            // [A][4] wall_clock64 of the agent's last bookkeeping in the dataflow replan or the flight:
                                 //     start, pair loop done, goal LPs done, copy done (diagnostics, always written)
};
// words of the seg_ready + pair_ok allocation
constexpr size_t corridor_pair_words(int A) { return (size_t)A * (1 + SOGM_MAX_PIECES); }

// The flight (sogm_flight_run): its control block FlightCtl and the hand-overs between its kernels are in sogm_handover.hpp.
static_assert(SOGM_MAX_PIECES <= WK_MAX_SUB, "a search pushes one corridor descriptor per segment slot, sub = the slot");
struct FlightWorld {  // one SogmWorld frame as the kernels read it
  const float        *cloud, *bounds;
  const SogmCylinder *cyl;
  int                 n_points, n_blocks, block_points, n_cyl;
};
// workgroups per kernel in FlightCtl::wg_start (tests/test_lifecycle_gpu.py reads the line below: the number ends it)
#define FL_WG_LOG 4096
#ifdef __HIPCC__
// residency evidence (diagnostics, no hand-over): when and where this workgroup executed its first instruction
__device__ inline void fl_wg_started(const FlightCtl &fl, int kernel) {
  if (threadIdx.x == 0 && fl.wg_start && blockIdx.x < FL_WG_LOG) {
    fl.wg_start[(size_t)kernel * FL_WG_LOG + blockIdx.x] = wall_clock64();
    // where: HW_ID (wave / SIMD / CU / SH / SE) | XCC_ID << 32
    fl.wg_start[(size_t)(4 + kernel) * FL_WG_LOG + blockIdx.x] =
        (long long)(unsigned)__builtin_amdgcn_s_getreg(63492) | ((long long)(unsigned)__builtin_amdgcn_s_getreg(63508) << 32);
  }
}
#endif
// The flight under the per-agent FSM (sogm_planner_set_flight_fsm; state == null: off, the flight as it is without it).
// What the head of an agent's tick hands to its search and its finish travels in the per-agent arrays due / reached /
// pos_now, like pva and t_start: written by the head in front of its wq_push, read behind the acquire the reader
// performs anyway.  Only the agent's own chain touches state[a]: the head reads it, the finish writes it.
struct FlightFsmDev {
  SogmFsmParams   prm;
  double          check_duration;  // isTrajSafe's horizon
  SogmFsmState   *state;           // [A] the caller's records
  const double   *goals;           // [A][3]
  int32_t        *due, *reached;   // [A] fsm_due's bits / isGoalReached of the agent's current tick
  double         *pos_now;         // [A][3] where the agent is at its current tick's stamp
  // the call's logs, each may be null; row of tick first_tick + i at [i][A]
  SogmFsmState   *log_state;
  int32_t        *log_due, *log_safe, *log_reached, *log_pub;
  double         *log_hover_start;
  SogmTrajRecord *log_own;
};
// The map stage's buffers, one struct per concern: the four builders of an agent's map (the lock-step kernels, k_update_flow,
// k_prestamp_flow, k_flight_map) hand the same structs to the same ticket bodies (csrc/sogm_map.hip).
struct MapTarget {  // where a map is built (host: sogm::map_target)
  void     *grid;    // all agents' cells
  unsigned *bits;    // [A][words] occupancy bits of slice 0 between the bits and the marks pass
  int       words;
  void     *cand;    // [A][SOGM_MAX_CYL_LDS] CylCand
  int      *n_cand;  // [A]
  MarkLog   lg;
  float    *poses;   // [A][3] map centres / [A] stamps of these maps (the queries read them)
  double   *stamps;
};
struct MapFrame {  // one sensor frame as the kernels read it
  const float        *cloud;
  const int32_t      *cloud_range;  // per-agent {begin, end} (null with cb.bounds set)
  CloudBlocks         cb;           // SogmWorld frame: blocks + the context's crop lists (bounds null = the ranges above)
  const SogmCylinder *cyl;
  int                 n_cyl;
};
struct OverlayIO {  // the neighbours' records an overlay adds
  const SogmTrajRecord *rec;
  int                   n_rec;
  int                   stride;  // 0: one table for every agent; n_rec: agent a reads rec[a * stride + r] (its own view)
  const int32_t        *ego_ids;
  const double         *body;
  int                   n_body;
};
struct TickInputsIO {  // sogm_tick_inputs' arguments: the executed records in, a tick's start states out
  const SogmTrajRecord *own;
  double               *hover, *now, *t_start, *pva;
  double                start_offset;
};
// One agent's tick inputs (plan_manager.cpp:169-175): the start state sampled from its executing trajectory at
// stamp + start_offset, or where it hovers; the map centre of the tick is that position.
// (k_tick_inputs in csrc/sogm_traj.hip, and the heads of k_prestamp_flow and k_flight_map in csrc/sogm_map.hip)
__device__ inline void tick_inputs_agent(const SogmTrajRecord &rec, const double *hov, int i, double stamp,
                                         const TickInputsIO &io, float *__restrict__ poses) {
  const double ts = stamp + io.start_offset;
  double       o[9];
  if (!traj_eval_record(rec, ts, o))
    for (int k = 0; k < 9; ++k) o[k] = hov[k];
  for (int k = 0; k < 9; ++k) io.pva[i * 9 + k] = o[k];
  for (int k = 0; k < 3; ++k) {
    io.hover[i * 9 + k]     = o[k];
    io.hover[i * 9 + 3 + k] = 0.0;
    io.hover[i * 9 + 6 + k] = 0.0;
    poses[i * 3 + k]        = (float)o[k];
  }
  io.now[i]     = stamp;
  io.t_start[i] = ts;
}
// The agent's executed record and hover row into the workgroup's LDS (one wave), visible to every lane on return.
__device__ __forceinline__ void stage_record_hover(SogmTrajRecord *s_rec, double *s_hov, const SogmTrajRecord *own,
                                                   const double *hover, int agent, int lane) {
  copy_record(s_rec, own + agent, lane);
  if (lane < 9) s_hov[lane] = hover[agent * 9 + lane];
  __syncthreads();
}
// the map role's arguments (csrc/sogm_map.hip, k_flight_map)
struct FlightMapDev {
  MapTarget             tgt;           // the context's current grid, centres and stamps
  const FlightWorld    *worlds;        // dev [n_ticks]
  CloudBlocks           cb;            // crop lists (bounds / counts per frame come from worlds[k])
  OverlayIO             ov;            // rec / n_rec are set per tick from the two fields below
  const SogmTrajRecord *tables;        // [4][n_total] ring of swarm tables
  int                   n_total;
  TickInputsIO          tick;          // own: executed records (latest wins)
  double                t0, period;
  int                   n_reset, n_bits, n_marks, n_splat;  // one-wave tickets per agent and tick
  int                   un_reset, un_bits, un_marks, un_splat;  // ... of a map in the urgent lane
  int                   n_head_wgs;    // workgroups 0 .. n_head_wgs - 1 of the launch admit agents (heads), the rest work off the queue
  int                   n_uhead_wgs;   // the first n_uhead_wgs of the heads serve the urgent ring
  int                   n_uwork_wgs;   // the first n_uwork_wgs of the workers look at the urgent queue first
  int                   n_admit;       // agents whose map may be under construction at once
  int                   pace_ticks;    // 100 MHz ticks between two admissions (0 = as fast as the heads run)
  size_t                agent_bytes;
  unsigned long long   *reset_stat;    // the context's reset statistics (sogm_sparse_reset_state / sogm_map_traffic), or null
  FlightFsmDev          fsm;           // the head of a tick under the FSM mode (fsm.state null: tick_inputs_agent, as before)
};
hipError_t launch_flight_map(const GridGeom &g, const FlightCtl &fl, const FlightMapDev &d, int n_workgroups, hipStream_t st);

// A stage's device buffers, one struct per stage: the grouped, dataflow and flight variants of a stage take the same
// struct from the launcher down to the device body (the map stage's four: MapTarget / MapFrame / OverlayIO / TickInputsIO
// above).  Field order = the kernels' argument order.  Every launch_* returns
// the first error it saw: hipGetLastError() clears the error as it reads it, the caller cannot ask again.
struct SearchIO {  // search: start state, goal and start time in, return code / route / statistics out
  const double *start_pva, *goal, *t_start;
  int32_t      *out_ret;
  double       *out_route;
  int32_t      *out_route_len;
  int           route_cap;
  int32_t      *out_stats;
  // who searches (null: every agent).  launch_astar: sogm_planner_set_due's mask, sogm_replan's searches.
  // launch_flight_search: the due bits the head of the agent's tick wrote under sogm_planner_set_flight_fsm — never
  // sogm_planner_set_due's mask, which a flight does not look at.
  const int32_t *due;
};
struct CorridorIO {  // corridors: the search's route in, polytopes and the local goal out
  const double  *start_pva, *t_start, *route;
  const int32_t *route_len;
  int            route_cap;
  double        *out_polys;
  int32_t       *out_nfaces, *out_npoly;
  double        *out_goal;
  // way-points in the agent's row: route_len is the route's full count, the row keeps route_cap of them (sogm_abi.h)
  __device__ __forceinline__ int points(int agent) const {
    const int n = route_len[agent];
    return n < route_cap ? n : route_cap;
  }
};
struct QpIO {  // QP: the corridors' polytopes and goal in, control points / status / iterations out
  const double  *start_pva, *goal_pv, *polys;
  const int32_t *nfaces, *npoly;
  double        *out_cpts;
  int32_t       *out_status, *out_iters;
};
// `__restrict__` lives on the `__global__` parameters of the per-stage entries' kernels (k_astar, k_flight_search,
// k_qp, k_corridor_points / _segment / _finalize) and of the map stage's lock-step kernels (k_cull_cylinders, k_stamp_bits /
// _blocks, k_stamp_marks / _cached, k_splat_neighbours; k_tick_inputs in csrc/sogm_traj.hip), which fill the struct in their first lines: a struct
// member cannot carry it.
// what finish_agent (csrc/sogm_finish.hpp) and k_pack_records (csrc/sogm_finish.hip) read and write for one agent
struct FinishArgs {
  double                corridor_tau;
  const int32_t        *ret, *npoly, *status;
  const double         *cpts;
  const SogmTrajRecord *swarm;
  int                   n_swarm;
  int                   swarm_stride;  // 0: one table for every agent; n_swarm: agent a reads swarm[a * swarm_stride + i]
  const int32_t        *swarm_ego;
  const double         *swarm_now, *t_start;
  const int32_t        *drone_ids;
  SogmTrajRecord       *out;
  int32_t              *out_ok, *out_safe;
  unsigned long long   *counters;
  SogmTrajRecord       *pub_own, *pub_table;
  const int32_t        *due;  // sogm_planner_set_due's mask (null: every agent was asked to plan): who is counted
};
// the light roles' arguments (k_flight_light): corridor stage buffers + the finishing role's
struct FlightLightDev {
  CorridorIO      cor;
  FinishArgs      fin;          // swarm / pub_table / out / out_ok are set per tick from the fields below
  SogmTrajRecord *tables;       // [4][n_total] ring of swarm tables (null: no deconfliction, no table)
  int             n_total, agent0;
  SogmTrajRecord *log_records;  // [n_ticks][A]
  int32_t        *log_ok;       // [n_ticks][A]
  FlightFsmDev    fsm;          // the finish under the FSM mode (fsm.state null: off)
};
struct CorridorWorkspace;
hipError_t launch_flight_light(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws, const FlightCtl &fl,
                               const FlightLightDev &d, int n_workgroups, hipStream_t st);
struct AstarWorkspace;
hipError_t launch_flight_search(const MapView &m, const SogmAstarParams &ap, double corridor_tau, const AstarWorkspace &wsp,
                                const FlightCtl &fl, int n_workgroups, const SearchIO &io, int spec, hipStream_t st);
struct QpWorkspace;
struct QpConst;
hipError_t launch_flight_qp(const SogmPlannerParams &pp, const SogmQpSettings &qs, const QpWorkspace &ws, const QpConst &qc,
                            const FlightCtl &fl, int n_workgroups, const QpIO &io, hipStream_t st);

// Arguments of the pre-stamp kernel (csrc/sogm_map.hip, k_prestamp_flow): the next tick's update inputs, the grid and
// mark log it builds into, and where the next tick's start states go.
struct PrestampDev {
  MapTarget    tgt;          // the pool's next grid and the context's NEXT poses / stamps (swapped in by sogm_update_prestamped)
  MapFrame     frame;
  TickInputsIO tick;         // own: the records the replan publishes into; the outputs are the next tick's
  double       stamp;
  float       *poses_host;   // the caller's copy of the next map centres (optional)
  int          n_agents;
  int          n_bits, n_marks;  // one-wave tickets per agent for the two passes of the stamp
  int          n_late, n_bits_late, n_marks_late;  // ... and for the last n_late agents to be published
  int          gate_agents;  // agents whose corridors must be final before the pre-stamp starts (tuning key prestamp_gate_frac)
};
// n_qp / n_finish: the QP workgroups and finishing waves of this replan — the pre-stamp's waves are not dispatched before
// all of them are resident (they wait for what those produce, and a QP workgroup needs a whole CU)
hipError_t launch_prestamp_flow(const GridGeom &g, const FlowCtl &fc, const PrestampDev &ps, int n_workgroups, int n_qp,
                                int n_finish, hipStream_t st);

// ParticleATC::isSafeAfterOpt for agents [agent0, agent0 + n_agents): out_safe[a] = 1 / 0
hipError_t launch_deconflict(int n_agents, const double *cpts, const int32_t *npoly, const SogmTrajRecord *rec,
                             int n_rec, const int32_t *ego_ids, const double *t_now, int32_t *out_safe,
                             hipStream_t st, int agent0, unsigned long long *counters = nullptr, int rec_stride = 0);
// the grouped path's records, ok flags and outcome counts for agents [agent0, agent0 + n_agents) (k_pack_records)
hipError_t launch_pack_records(int n_agents, const FinishArgs &f, hipStream_t st, int agent0);
hipError_t launch_corridor(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws, int n_agents,
                           const CorridorIO &io, hipStream_t st, int agent0 = 0, hipEvent_t ev_map_read = nullptr);

// dataflow replan launchers (persistent kernels; see k_worker_flow / k_qp_flow).  The worker kernel: n_finish finishing
// blocks at the lowest block indices, then n_corridor corridor blocks
hipError_t launch_flow_gate(const FlowCtl &fc, int expected, hipStream_t st);
hipError_t launch_worker_flow(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws, const FlowCtl &fc,
                              int n_agents, int n_finish, int n_corridor, const CorridorIO &io, const FinishArgs &f,
                              hipStream_t st);

// Per-agent QP row storage in HBM, used only when a problem's rows do not fit in LDS (what lives where: sogm_qp_layout.hpp,
// which also sizes both buffers: qp_scratch_bytes_per_agent(max_faces), qp_k1_scratch_bytes_per_agent()).
struct QpWorkspace {
  char  *scratch;         // [A][scratch_stride]
  size_t scratch_stride;  // bytes per agent (rows at M = SOGM_MAX_PIECES, max_faces faces)
  int    dyn_lds_bytes;   // dynamic LDS per workgroup of k_qp
  double *k1_scratch;     // [A][120 * 18] band of A^T diag(rho / rho_cur) A when it does not fit in LDS beside the rows
  // BezierOpt::setup in full (sogm_bezier_qp_solve_timed): per-piece time allocation [A][SOGM_MAX_PIECES] and an
  // end state with acceleration (goal rows of 9 doubles instead of 6).  nullptr / 6: every piece = corridor_tau,
  // final acceleration 0 — what replan() asks for (baseline.cpp:411,423).
  const double *t_alloc;
  int           goal_stride;
  // diagnostics (tools/): [A][SOGM_QP_STAT_N] the clocks of the agent's last solve, slots SOGM_QP_STAT_* (sogm_abi_debug.h);
  // always written (a handful of clock reads per 25 iterations)
  long long    *dbg;
  int           ablate;  // phase ablation mask of the staged k_qp launch (profiling builds only; tuning key qp_ablate)
};
// Lets the three QP kernels use the CU's LDS beyond the default limit on the current device and returns the dynamic
// LDS a workgroup of them may ask for (QpWorkspace::dyn_lds_bytes): once per planner, before its first launch.
int    qp_kernel_setup();
struct QpConst {
  double QM[225];  // per-piece min-jerk cost block (bezier_optimizer.cpp:96-111)
};
int astar_resident_workgroups(int device);
hipError_t launch_qp(const SogmPlannerParams &pp, const SogmQpSettings &qs, const QpWorkspace &ws, const QpConst &qc,
                     int n_agents, const QpIO &io, hipStream_t st, int agent0 = 0);
hipError_t launch_qp_flow(const SogmPlannerParams &pp, const SogmQpSettings &qs, const QpWorkspace &ws, const QpConst &qc,
                          const FlowCtl &fc, int n_agents, int n_workgroups, const QpIO &io, hipStream_t st);

size_t astar_node_bytes();
// out_trace / trace_cap: the expansion trace of sogm_astar_search (null / 0 everywhere else)
hipError_t launch_astar(const MapView &m, const SogmAstarParams &ap, double corridor_tau, const AstarWorkspace &wsp,
                        int n_agents, const SearchIO &io, int32_t *out_trace, int trace_cap, hipStream_t st,
                        int agent0 = 0, const FlowCtl *fc = nullptr, int search_mode = 0);

}  // namespace sogm

#define SOGM_MAX_GROUPS 64

struct sogm_planner {
  sogm::Resources      res;  // owns every buffer, stream and event below (sogm_resources.hpp)
  sogm_ctx            *map;
  SogmAstarParams      ap;
  SogmPlannerParams    pp;
  SogmQpSettings       qs;
  sogm::AstarWorkspace aw;
  sogm::CorridorWorkspace cw;
  sogm::QpWorkspace qw;
  sogm::QpConst qc;
  // internal buffers used by sogm_replan (device)
  int32_t *d_ret, *d_route_len, *d_stats;
  double  *d_route;
  int      route_cap;
  double  *d_polys, *d_goal, *d_cpts;
  int32_t *d_nfaces, *d_npoly, *d_status, *d_iters;
  // post-optimisation deconfliction (ParticleATC::isSafeAfterOpt); off while swarm == nullptr
  int32_t              *d_safe;
  const SogmTrajRecord *swarm;
  int                   n_swarm;
  int                   swarm_stride;  // 0: sogm_planner_set_swarm's one table; n_swarm: _set_swarm_views' [A][n_swarm]
  const int32_t        *swarm_ego;
  const double         *swarm_now;
  // publication inside the replan (sogm_planner_set_publish): the host's own-record table and the next swarm table
  SogmTrajRecord       *pub_own, *pub_table;
  // the agents sogm_replan plans (sogm_planner_set_due): dev [A], != 0 = due; null = all
  const int32_t        *due;
  // agent groups: sogm_replan runs each group's search -> corridors -> QP chain on its own stream,
  // so one slow agent (a long A* search, an infeasible QP) only delays its own group
  int         n_groups;
  hipStream_t gstream[SOGM_MAX_GROUPS];
  hipEvent_t  ev_in, ev_corr[SOGM_MAX_GROUPS], ev_done[SOGM_MAX_GROUPS];
  hipEvent_t  ev_pts[SOGM_MAX_GROUPS];  // after a group's obstacle-point kernel: its last read of the SOGM
  // dataflow replan (persistent kernels chained per agent through device-side ready lists)
  int            flow;        // 1 = use it (pipelining modes other than the in-place pre-clear)
  int           *d_flow;      // the control block (layout: sogm::FlowBlock)
  long long     *d_flow_ts;   // [A][8]
  sogm::FlowCtl  fc;
  // its two streams, created by the first dataflow replan (the searches run on the caller's stream): the worker stream —
  // reset, residency gate, k_worker_flow, report — and the QP kernel's
  hipStream_t    wstream, qstream;
  hipEvent_t     ev_pdone;
  sogm::PrestampDev ps;       // the host's part of the pre-stamp arguments
  int            ps_on;
  int            ps_world_on;  // the pre-stamp's inputs are a SogmWorld frame (copied at sogm_planner_set_prestamp)
  SogmWorld      ps_world;
  hipEvent_t     ev_gate;
  hipEvent_t     ev_records;  // behind the worker kernel, in front of the report: every record is published (the context's ev_records_final)
  hipEvent_t     ev_wdone, ev_qdone;  // the fan-in: the worker stream's end (with the report, when it runs there), the QP kernel's end
  int           *d_epoch;      // device word: the clear epoch of the replan in flight (sogm_ctx::clear_epoch_word)
  int            reset_epoch;  // generation of the control block's reset (k_flow_reset writes it into the block's word FlowBlock::gen)
  int           *h_flow_fail;  // pinned, device-visible: {last FLOW_ERR code, ticks that failed} (k_flow_report)
  // per-object use of the per-stage entries (sogm_planner_select_agents / _set_search_mode)
  int sel_first, sel_count;  // agents the per-stage entries process; (0, A) by default
  int search_mode;           // 0 the replan's two-call pattern, 1 / 2 one search with init_search true / false
  int spec_astar;            // dataflow replan: run the second search attempt speculatively beside the first
  hipStream_t peek;          // sogm_debug_flow_peek's private stream (created on first use)
  // flight (sogm_flight_run): control block, per-agent tick inputs, frames, masked streams (all created on first use)
  sogm::FlightCtl     fl;
  int                *d_fl;          // the control block (layout: sogm::FlightBlock)
  sogm::FlightWorld  *d_fl_worlds, *h_fl_worlds;  // [FLIGHT_MAX_TICKS] device / pinned staging
  double             *d_fl_pva, *d_fl_tstart, *d_fl_now;
  hipStream_t         fl_stream[4];  // QP, search, corridor + finish, map
  hipEvent_t          fl_ev_in, fl_ev_done[4];
  int                 fl_cus[4];     // compute units of each stream's mask
  int                 fl_wgs[4];     // workgroups of each kernel
  int                 fl_epoch = 0;  // number of the last sogm_flight_run call (FlightCtl::epoch)
  int                *fl_xready = nullptr;  // [FLIGHT_MAX_TICKS] FlightCtl::xready of a multi-rank flight
  // sogm_planner_set_flight_fsm: the caller's struct (fl_fsm_on: registered) and the head's hand-over arrays (flight_setup)
  int                 fl_fsm_on = 0;
  SogmFlightFsm       fl_fsm{};
  int32_t            *d_fl_due = nullptr, *d_fl_reached = nullptr;
  double             *d_fl_posnow = nullptr;
};

// The search's per-phase clock statistics (sogm_debug_astar_stats, tools/diag_astar.py) are collected while the map's
// profiling is on: five s_memrealtime reads per expansion are not free.
inline sogm::AstarWorkspace astar_ws(const sogm_planner *p) {
  sogm::AstarWorkspace w = p->aw;
  if (!((p->map->profiling >> SOGM_PROF_ASTAR) & 1)) w.dbg = nullptr;
  return w;
}

// A launcher's error under the caller's label.  The launchers hand over what hipGetLastError() gave them: it clears the
// error as it reads it, so a second call here would report "no error".
inline int launched(const char *what, hipError_t e) {
  if (e == hipSuccess) return SOGM_OK;
  sogm::set_error(what, e);
  return SOGM_ERR_HIP;
}

// The stages' buffers of a replan or a flight: the planner's own between the stages, the caller's at both ends.
inline sogm::SearchIO search_io(const sogm_planner *p, const double *start_pva, const double *goal, const double *t_start) {
  return sogm::SearchIO{.start_pva = start_pva, .goal = goal, .t_start = t_start, .out_ret = p->d_ret,
                        .out_route = p->d_route, .out_route_len = p->d_route_len, .route_cap = p->route_cap,
                        .out_stats = p->d_stats, .due = p->due};
}
inline sogm::CorridorIO corridor_io(const sogm_planner *p, const double *start_pva, const double *t_start) {
  return sogm::CorridorIO{.start_pva = start_pva, .t_start = t_start, .route = p->d_route,
                          .route_len = p->d_route_len, .route_cap = p->route_cap, .out_polys = p->d_polys,
                          .out_nfaces = p->d_nfaces, .out_npoly = p->d_npoly, .out_goal = p->d_goal};
}
inline sogm::QpIO qp_io(const sogm_planner *p, const double *start_pva) {
  return sogm::QpIO{.start_pva = start_pva, .goal_pv = p->d_goal, .polys = p->d_polys, .nfaces = p->d_nfaces,
                    .npoly = p->d_npoly, .out_cpts = p->d_cpts, .out_status = p->d_status, .out_iters = p->d_iters};
}
// a replan's: swarm and publication as sogm_planner_set_swarm / _set_publish left them (the flight fills its own)
inline sogm::FinishArgs finish_args(const sogm_planner *p, const double *t_start, const int32_t *drone_ids,
                                    SogmTrajRecord *out, int32_t *out_ok) {
  return sogm::FinishArgs{.corridor_tau = p->pp.corridor_tau, .ret = p->d_ret, .npoly = p->d_npoly,
                          .status = p->d_status, .cpts = p->d_cpts, .swarm = p->swarm, .n_swarm = p->n_swarm,
                          .swarm_stride = p->swarm_stride, .swarm_ego = p->swarm_ego, .swarm_now = p->swarm_now, .t_start = t_start,
                          .drone_ids = drone_ids, .out = out, .out_ok = out_ok, .out_safe = p->d_safe,
                          .counters = p->cw.counters, .pub_own = p->pub_own, .pub_table = p->pub_table,
                          .due = p->due};
}
