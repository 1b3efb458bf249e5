/* sogm_abi_debug.h — the part of libsogm_hip.so's C ABI that a plan_manager host does not need to fly: tuning knobs,
 * per-kernel profiling, device clocks, traffic counters, parity downloads of internal state and test hooks.  Used by
 * bench.py, tools/ and tests/ (the Python binding declares both headers' symbols; tests/test_abi_symbols.py checks both
 * against the library).  Same library, same SOGM_ABI_VERSION as include/sogm_abi.h, which it includes.
 * host/sogm_facade.hpp includes only sogm_abi.h; its setTuning() exists when this header was included first. */
#ifndef SOGM_ABI_DEBUG_H
#define SOGM_ABI_DEBUG_H
#include "sogm_abi.h"
#ifdef __cplusplus
extern "C" {
#endif

/* host out[8]: {enabled, log capacity per agent, 1 if the current grid is covered by its log, largest per-agent
 * entry count of the current grid's log (above the capacity: that agent's next reset is dense), entries of all
 * agents together (saturating), sparse resets launched since the previous call, mean entries read per such
 * launch, mean KiB zeroed per such launch (the stores the reset kernel issued, counted on the device)}.
 * Synchronises. */
int sogm_sparse_reset_state(sogm_ctx *ctx, int32_t *out_host);

/* Tuning knobs.  Every internal width and switch of the library has a default chosen on MI355X; a host that wants
 * another value sets it per context — nothing is read from the environment (the library's only environment switches are
 * SOGM_SPARSE_RESET, SOGM_FLOW and SOGM_RCCL_LIB).  Keys (defaults in parentheses):
 *   read by sogm_planner_create (set them before):  "groups" (2) agent groups of the grouped-stream replan,
 *     "spec_astar" (1) speculative second search, "clear_gate_frac" (1.0);
 *   read at every call:  "qp_wgs" (0 = half the CUs) persistent QP workgroups, "finish_wgs" (0 = min(agents, 64)) finishing and "corridor_wgs" (0 = min(4 per CU, one per segment slot)) corridor blocks of the dataflow replan's worker kernel, "stamp_wgs" (256), "stamp_bits_wgs" (0 = stamp_wgs), "stamp_cached" (0), "stamp_lds_log" (1), "stamp_lds_kb" (0), "splat_wgs" (256),
 *     "splat_overlap" (1), "reset_wgs" (32), "reset_lanes" (0 = auto: 2 under the replan, 4 alone), "reset_unroll"
 *     (0 = auto: 1 / 8), "reset_late" (1), "prestamp_bits" (32), "prestamp_marks" (64), "prestamp_wgs" (0 = 8 per CU), "prestamp_stream" (1), "prestamp_gate_frac" (0.9: the pre-stamp of the next map starts when that share of the agents' corridors is final — an event recorded behind a gate kernel on the resets' stream; 1.0: when all are),
 *     "prestamp_late_agents" (8), "prestamp_late_bits" (128), "prestamp_late_marks" (256), and the dense clear's
 *     "clear_wgs" (0 = auto), "clear_throttle" (0), "clear_nt" (1), "clear_wide_wgs" (256; 0 = fixed width),
 *     "clear_wide_bound" (0), "clear_head_gb" (1e9), "clear_early" (0), "clear_retire_at_end" (0); "qp_ablate" (0;
 *     profiling builds only);
 *   sogm_flight_run (read at its first call: the masked streams are created once):  "flight_qp_units" (4),
 *     "flight_search_units" (2), "flight_map_units" (4) — compute units in units of 16 for the QP / search / map kernels,
 *     the corridor + finish kernel takes the rest —, "flight_masks" (1; 0 = unmasked streams), "flight_spec" (1: both
 *     search attempts side by side), and per (agent, tick) one-wave tickets "flight_reset" (8), "flight_bits" (16),
 *     "flight_marks" (32), "flight_splat" (4); "flight_admit" (48) agents whose map may be under construction at once, "flight_pace_us" (20; 40 until round 6) microseconds between two
 *     admissions to the map stage (agents then reach every stage at a steady rate; 0 = unpaced), "flight_heads" (32)
 *     admitting waves of the map kernel; "flight_urgent" (8): an agent among the last n finishers of a tick — the agents the
 *     swarm waits for at the next gate — builds the map of its next tick through a lane of its own (four of the heads, no
 *     admission order / pace / window; a work queue of its own that the first "flight_urgent_waves" (4096 = all) map workers
 *     look at before they take plain work and while they wait for it; its maps are cut into "flight_urgent_fine" (4) times
 *     more tickets; 0 = no such lane); "flight_gate_pace_us" (20; 40 until round 6): the staleness rule's gate — tick k reads the neighbours'
 *     records of tick k - 2 — sits in front of a map's overlay, the only phase that reads them: an agent builds the rest of its
 *     next map while it waits, and the finish that opens a gate queues the waiting overlays this many microseconds apart;
 *     "flight_neighbour_lag" (2): tick k's overlay and isSafeAfterOpt read the neighbours' records of tick k - lag.  2 is the
 *     flight's rule (an agent runs up to two ticks ahead of the slowest); 1 is the REFERENCE's staleness — a record is at most
 *     one broadcast period old (particles.cpp:179-190), what the lock-step tick reads — with less overlap: an agent's overlay
 *     waits until every agent has finished the previous tick.  This key DOES change records (it selects the rule);
 *     "flight_engines" (4), "flight_engine_first" (0): the shader engines (of every XCD) the flight's kernels share — a flight on
 *     half of them leaves the other half to a second flight on the same device (two ranks as two threads: tests) —,
 *     "flight_exchange_units" (0): units given to NO kernel, room for a collective's own kernels beside a multi-rank flight
 *     (the Python driver sets 1 when torch.distributed runs over more than one rank: untested on hardware);
 *     "flight_light_per_cu" (4), "flight_map_per_cu" (8): one-wave workgroups of the corridor + finish / the map kernel per
 *     compute unit of their partition (what a unit holds at once; fewer leaves slack).  Whatever the unit counts, every
 *     kernel's mask gets the same number of units in every shader engine it touches and a launch exactly the workgroups
 *     that mask holds at once (sogm_flight_stats hdr[15] counts workgroups that were not resident from the start: 0).
 *     None of these keys but flight_neighbour_lag changes a cell or a record.
 *   sogm_update_world, experimental (measured, not adopted: profiles/EXPERIMENTS.md round 5):  "update_flow" (0; 1 = the
 *     maps are built agent by agent on a stream of the context's own — one persistent launch over one-wave tickets, per
 *     agent occupancy bits -> marks -> overlay, agents in the order of their previous chain's length — and sogm_replan's
 *     searches start per agent as their map completes; every other reader of the grid joins the flow's end by itself;
 *     identical cells and records), with "update_bits" (16), "update_marks" (64), "update_splat" (40) tickets per agent,
 *     "update_wgs" (0 = 16 per CU), "update_chunk" (1) tickets per claim, "update_cached" (0), "update_order" (1).
 * Not thread-safe against calls on the same context (like every other call).  Unknown key: SOGM_ERR_INVALID_ARG.
 * sogm_tuning_key(i) enumerates the keys (NULL past the last). */
int         sogm_set_tuning(sogm_ctx *ctx, const char *key, double value);
int         sogm_get_tuning(const sogm_ctx *ctx, const char *key, double *out_value_host);
const char *sogm_tuning_key(int index);

/* What the map kernels moved since the last reset of these counters (device-side counts, for the roofline figures of
 * bench.py); host out[6]: {resets through the mark logs, log entries those resets read, bytes they zeroed, stamps
 * launched (sogm_update_gt* and pre-stamps), marks (cells set to 1) the stamps wrote, log entries the stamps
 * appended}.  Counted while the sparse reset is on.  reset != 0 zeroes the counters.  Synchronises. */
int sogm_map_traffic(sogm_ctx *ctx, int64_t *out_host, int reset);

/* How the CURRENT grid (the one queries and planning read) came to be; host out[4]: {pool slot, resets of that slot
 * through its mark log since the pool was built, dense clears of that slot (fake_particle_risk_voxel.cpp:107-108's
 * fill), 1 if the grid was built by the previous sogm_replan's pre-stamp and adopted by sogm_update_prestamped}.
 * Host-side launch counts; does not synchronise.  (Parity tests use it to assert which path built the map.) */
int sogm_grid_history(sogm_ctx *ctx, int32_t *out_host);

/* Per-kernel timing with HIP events recorded on the caller's stream around each launch (used by
 * bench.py for the roofline figure).  Slots: */
enum {
  SOGM_PROF_CLEAR = 0, /* the grid's reset: k_reset_sectors (sparse) or k_clear_slabs / k_clear_chunks (dense) */
  SOGM_PROF_STAMP = 1, /* k_cull_cylinders + k_stamp_bits + k_stamp_marks    */
  SOGM_PROF_SPLAT = 2, /* k_splat_neighbours                                 */
  SOGM_PROF_ASTAR = 3,
  SOGM_PROF_CORRIDOR = 4,
  SOGM_PROF_QP = 5,
  SOGM_PROF_CLEAR_HEAD = 6, /* single-grid pipelining: the narrow first part of a two-part clear (slot 0 = the rest) */
  SOGM_PROF_EXCHANGE = 7, /* sogm_traj_allgather: the ncclAllGather on the exchange stream */
  SOGM_PROF_N = 8
};
int sogm_set_profiling(sogm_ctx *ctx, int enable);
/* The same for a choice of slots (bit k of slot_mask = slot k; 0 = off): every timed launch costs two event records on
 * its stream, which a tick's critical path notices — bench.py times only the rated kernel inside its timed region. */
int sogm_set_profiling_slots(sogm_ctx *ctx, int slot_mask);
/* Synchronises the device, then writes the duration (ms) of the LAST launch of each slot
 * (negative if that slot has not run since profiling was enabled).  host out_ms[SOGM_PROF_N]. */
int sogm_profile_read(sogm_ctx *ctx, double *out_ms_host);
/* Every launch of a slot since sogm_set_profiling(ctx, 1) keeps its own event pair (the last 1024 are kept), so a
 * whole timed region can be measured launch by launch with no synchronisation inside it.  Synchronises the
 * device, then writes the durations (ms, oldest first) of the last min(cap, 1024, launches) launches of `slot`
 * to host out_ms[cap] and their number to *out_n. */
int sogm_profile_read_all(sogm_ctx *ctx, int slot, double *out_ms_host, int cap, int *out_n);

/* Where a tick's wall time goes (bench.py's sustained.slowest_tick).  sogm_device_clock runs a one-lane kernel on `stream`
 * that reads the device's 100 MHz wall clock, synchronises the stream and returns the value: a host that brackets the call with
 * its own clock learns the offset between the two clocks to within the synchronisation's return latency (also arms the
 * stamps below).  sogm_tick_clock: host out[2] = that clock at the start of the last map update's first kernel and in the
 * last sogm_replan's closing kernel (pinned memory, no synchronisation: read them after one). */
int sogm_device_clock(sogm_ctx *ctx, int64_t *out_ticks_host, void *stream);
int sogm_tick_clock(sogm_ctx *ctx, int64_t *out2_host);

/* Copy agent `a`'s grid to host in the reference layout risk_maps_[V][T] (map.h:52). Synchronous. */
int sogm_download_reference_layout(sogm_ctx *ctx, int agent, float *out_vt_host);

/* Parity I/O (synchronous): agent's particle store in the reference layout
 * voxels_with_particle[V][2*max][9] (slot 8, the update time, is written as 0) and
 * voxels_objects_number[V][4+T]; counters[16]: {voxel_full, pyramid_full, moved_out, candidates,
 * p_seq, v_seq, rand_seq, slots_per_voxel, slots_per_pyramid, n_pyramids, unconverged_rounds,
 * pool_overflow, ...}.  Any pointer may be NULL. */
int sogm_dsp_download_state(sogm_dsp *d, int agent, float *store_host, float *objnum_host,
                            int32_t *counters_host);
/* Test hook, the inverse of sogm_dsp_download_state (synchronous): makes store_host [V][2*max][9] (reference layout) agent
 * `agent`'s particle store as it stands BETWEEN two updates, so that a test can start from a hand-built store.  Rules:
 *   - every slot's flag (entry 0) is exactly 0, 0.6f or 1.0f (empty / a resampler's copy / a particle: what
 *     mapOccupancyCalculationAndResample leaves) and a non-empty slot's vz (entry 3) is 0; entry 8 (the update time) is
 *     ignored; entries 1, 2 and 4-7 of an empty slot are stored as given (nothing reads them), its entry 3 is not kept
 *     (the device stores no vz): sogm_dsp_download_state gives 0 for every slot's entries 3 and 8;
 *   - last_pos3_host / last_stamp become the pose and stamp of the "previous update" (the next sogm_update_dsp is not a first
 *     call: its deltas are taken against them); cursors3_host = {p_seq, v_seq, rand_seq}, each within its table;
 *   - the agent's voxels_objects_number (weight sums, mean velocities, future status) is zeroed, its debug and error
 *     counters (counters 0-3 and 10-12 of sogm_dsp_download_state) are cleared, and the velocity estimation forgets its
 *     previous frame's clusters (its sticky error code stays).  The observation tables and the new-born list of the last
 *     update stay as they are.
 * Anything else — a NULL pointer, an agent out of range, another flag value, a NaN flag, vz != 0 on a non-empty slot, a
 * cursor outside its table — returns SOGM_ERR_INVALID_ARG and changes nothing.  Other agents are never touched. */
int sogm_dsp_upload_state(sogm_dsp *d, int agent, const float *store_host, const float *last_pos3_host, double last_stamp,
                          const int32_t *cursors3_host);
/* input_cloud_with_velocity of the last update (the new-born list, rows {x,y,z,vx,vy,vz,intensity}, at most `cap`
 * rows), its length, and counters4 = {clusters, possibly dynamic, matched, error code of the velocity estimation}.
 * The error code is 0 or the capacity that was exceeded: 2 = a point with more than 128 neighbours within the cluster
 * tolerance (neighbours dropped), 3 = more than 256 accepted clusters (the rest dropped), 4 = more than 64 possibly-dynamic
 * clusters (the rest treated as static), 5 = new x previous possibly-dynamic clusters > max_points (no association in that
 * frame).  The update itself still returns SOGM_OK and the other agents of the batch are unaffected.  The code is STICKY:
 * a later frame within the capacities does not clear it (the latest non-zero code stays until the handle is destroyed).
 * A cloud longer than max_points is clamped to its first max_points points and counted in counters[12] of
 * sogm_dsp_download_state (once per clamped update), not here. */
int sogm_dsp_download_born(sogm_dsp *d, int agent, float *born_host, int cap, int32_t *n_born, int32_t *counters4);
/* The source index of that list (sogm_abi.h "velocity audit"; synchronous like the call above): out_host[k], k < min(n_born,
 * cap), is the index inside the agent's range of the input cloud of the point row k of the list came from.  The identity after
 * an update with labels; after one without, the order the velocity estimation gave the list, the points of rejected clusters
 * missing.  Rows at and beyond n_born are not meaningful. */
int sogm_dsp_download_born_source(sogm_dsp *d, int agent, int32_t *out_host, int cap, int32_t *n_born);
/* Observation tables of the last update: nobs[n_pyramids], pc[n_pyramids*obs_max*5], maxlen[n_pyramids] */
int sogm_dsp_download_observations(sogm_dsp *d, int agent, int32_t *nobs_host, float *pc_host,
                                   float *maxlen_host);

/* Parity I/O (synchronous): occupancy_buffer_ [nx*ny*nz] fp64, occupancy_buffer_inflate_ int8,
 * bounds[6] = local_bound_min, local_bound_max, counters[4] = {rays, active rays, rounds used, errors}. */
int sogm_gridmap_download(sogm_gridmap *g, int agent, double *occupancy_host, int8_t *inflate_host,
                          int32_t *bounds_host, int32_t *counters_host);
/* Test hook: sets raycast_num_ (the de-duplication flags are chars and stop matching after frame 127). */
int sogm_gridmap_force_frame(sogm_gridmap *g, int raycast_num);

/* Test hook: the corridor rules around FIRI (the per-segment box, ShrinkCorridor, checkCorridorValidity and the `break`,
 * the adjacent-intersection scan, the goal scan; baseline.cpp:300-403 / baseline_fake.cpp:300-414) for n independent
 * problems whose polytopes the caller injects where FIRI's would be — the replan's own device code, one wave per
 * problem.  pp_host[n] is HOST memory (fake_planner, shrink_size, init_range and max_faces are read; every max_faces
 * must equal `max_faces` <= 64, the stride of all polytope arrays); every other pointer is device memory:
 * start_pva [n][9], route [n][route_cap][6] with route_cap > SOGM_MAX_PIECES, route_len [n], polys
 * [n][SOGM_MAX_PIECES][max_faces][4] un-shrunk rows h.x + h3 <= 0, nfaces [n][SOGM_MAX_PIECES], seg_state
 * [n][SOGM_MAX_PIECES] or NULL (-3 marks a segment "capacity exceeded", anything else leaves the verdict to the rules).
 * Outputs: out_box [n][SOGM_MAX_PIECES][6] (llc, lhc), out_shrunk (as polys), out_seg_nfaces, out_seg_state
 * [n][SOGM_MAX_PIECES] (1 valid, 0 invalid, -2 no such segment, -3 capacity) and sogm_corridor_generate's out_polys
 * [n][SOGM_MAX_PIECES][max_faces][4], out_nfaces [n][SOGM_MAX_PIECES], out_npoly [n], out_goal [n][6].
 * counters_of (may be NULL): the planner whose corridor_capacity / pieces_capacity counters the bookkeeping raises.
 * Asynchronous on `stream` but for the copy of pp_host. */
int sogm_corridor_rules_batched(sogm_planner *counters_of, const SogmPlannerParams *pp_host, const double *start_pva,
                                const double *route, const int32_t *route_len, int route_cap, const double *polys,
                                const int32_t *nfaces, const int32_t *seg_state, int n, int max_faces, double *out_box,
                                double *out_shrunk, int32_t *out_seg_nfaces, int32_t *out_seg_state, double *out_polys,
                                int32_t *out_nfaces, int32_t *out_npoly, double *out_goal, void *stream);
/* The same hook with flags.  SOGM_RULES_PARALLEL: the dataflow replan's form — SOGM_MAX_PIECES one-wave workgroups per
 * problem, one per segment slot; the wave that finishes the later of two neighbouring segments solves their
 * adjacent-intersection LP at once, the one that completes the problem's last slot does the bookkeeping from those
 * verdicts.  Every output is the sequential form's, byte for byte.  counters_of then also takes the pair counters
 * (sogm_debug_corridor_pairs).  flags = 0: sogm_corridor_rules_batched. */
#define SOGM_RULES_PARALLEL 1
int sogm_corridor_rules_batched_flags(sogm_planner *counters_of, const SogmPlannerParams *pp_host, const double *start_pva,
                                      const double *route, const int32_t *route_len, int route_cap, const double *polys,
                                      const int32_t *nfaces, const int32_t *seg_state, int n, int max_faces,
                                      double *out_box, double *out_shrunk, int32_t *out_seg_nfaces, int32_t *out_seg_state,
                                      double *out_polys, int32_t *out_nfaces, int32_t *out_npoly, double *out_goal,
                                      int flags, void *stream);

/* Test hook: the end of a replan — ParticleATC::isSafeAfterOpt against a swarm table, the outcome count, the SogmTrajRecord and
 * its publication — for n independent agents whose search / corridor / QP results the caller injects, in either of the two
 * forms the library has (csrc/sogm_finish.hip).  flags = 0: the grouped form, one wave per (record, agent) pair and the
 * records packed behind it (sogm_replan in pipelining mode 1, sogm_safe_after_opt).  SOGM_FINISH_WAVE: the finishing wave,
 * one wave per agent — the device body the dataflow sogm_replan and sogm_flight_run inline, without their hand-over
 * control: one lane per record pre-tests 64 records at a time, the pairs left over take the LP in record order, the first
 * unsafe one ends the check, and an agent that was not solved skips it (its out_safe is 1 there).
 * Device memory: ret, npoly (<= SOGM_MAX_PIECES), status [n] (the search's return, the corridor count, the QP's status:
 * 1 / 2 = solved), cpts [n][SOGM_MAX_PIECES * 15], swarm [n_swarm] (NULL: no check, n_swarm is taken as 0; every n_pieces
 * <= SOGM_MAX_PIECES) with swarm_ego, swarm_now [n], t_start, drone_ids [n], due [n] or NULL (an agent with due 0 is not
 * counted).  Outputs: out [n], out_ok [n], out_safe [n] (the grouped form writes it only when a swarm is given, and for
 * unsolved agents too; the two forms agree on it for solved agents); pub_own [n] and pub_table [n], each or NULL, are read and
 * written as sogm_planner_set_publish describes (with pub_own NULL nothing is published).  counters_of (may be NULL):
 * the planner whose outcome and deconflict_capacity counters are raised.  Asynchronous on `stream`. */
#define SOGM_FINISH_WAVE 1
int sogm_finish_batched(sogm_planner *counters_of, double corridor_tau, const int32_t *ret, const int32_t *npoly,
                        const int32_t *status, const double *cpts, const SogmTrajRecord *swarm, int n_swarm,
                        const int32_t *swarm_ego, const double *swarm_now, const double *t_start, const int32_t *drone_ids,
                        const int32_t *due, int n, SogmTrajRecord *out, int32_t *out_ok, int32_t *out_safe,
                        SogmTrajRecord *pub_own, SogmTrajRecord *pub_table, int flags, void *stream);

/* Diagnostics: the adjacent-pair LPs of the corridor bookkeeping (dataflow replan, flight, parallel rules hook).  out4, since
 * the last call: [0] pair LPs solved by a segment's wave as its neighbour was done, [1] pair LPs solved inside the
 * bookkeeping because no verdict was there, [2] pairs the bookkeeping took from a verdict, [3] the OR of every ready word
 * and verdict of the planner now and of what a parallel rules hook left set (0: every finalising wave cleaned up).
 * Synchronises the device. */
int sogm_debug_corridor_pairs(sogm_planner *p, unsigned long long *out4);

/* Diagnostics: the number of HIP streams the planner and its map context hold now (the return value; negative: an SOGM_ERR_*
 * code).  Every stream takes a place in the runtime's pool of hardware queues, so streams are
 * created by the first call that launches on them: 1 after sogm_create (the resets' side stream), 3 once a dataflow
 * sogm_replan has run (+ its worker and QP streams; the searches run on the caller's stream), one more each for a pre-stamp on
 * a stream of its own, the dense-clear mode's wide launch, the grouped path's group streams, the update flow, the trajectory
 * exchange, a flight's four masked streams and sogm_debug_flow_peek.  Host-side count, no HIP call. */
int sogm_debug_streams_held(sogm_planner *p);

/* Diagnostics: every agent's last QP solve as its workgroup clocked it, host out[n_agents][SOGM_QP_STAT_N].  Times are
 * ticks of the device's 100 MHz wall clock unless said otherwise.  Synchronises the device. */
enum {
  SOGM_QP_STAT_TOTAL = 0,      /* the whole solve */
  SOGM_QP_STAT_SETUP = 1,      /* assembly, scaling, first factorisation */
  SOGM_QP_STAT_REFAC = 2,      /* later refactorisations ... */
  SOGM_QP_STAT_N_REFAC = 3,    /* ... and their count */
  SOGM_QP_STAT_CHECK = 4,      /* termination checks: residual passes, tests, certificates ... */
  SOGM_QP_STAT_N_CHECK = 5,    /* ... and their count */
  SOGM_QP_STAT_ITERS = 6,      /* iterations run */
  SOGM_QP_STAT_PATH = 7,       /* bit 0: register-resident iteration, bit 1: every row array in LDS (sogm_debug_qp_layout) */
  SOGM_QP_STAT_FACTOR_ASM = 8, /* the factorisations, summed: block assembly | forward sweep | backward rows + K^-1 registers */
  SOGM_QP_STAT_FACTOR_FWD = 9,
  SOGM_QP_STAT_FACTOR_BWD = 10,
  SOGM_QP_STAT_SHADER_CLOCKS = 11, /* the span of slot 0 in shader clocks */
  SOGM_QP_STAT_CHECK_STAGE = 12,   /* of slot 4: staging the row state for the check | the residual pass */
  SOGM_QP_STAT_CHECK_RESID = 13,
  SOGM_QP_STAT_SETUP_SPLIT = 14, /* three 20-bit fields of ticks since the start: assembly + CSC done | Ruiz scaling done |
                                    rho + K1 done (slot 1 minus the third: the first factorisation and the load of the row state) */
  SOGM_QP_STAT_N = 16
};
int sogm_debug_qp_stats(sogm_planner *p, long long *out_host);
/* What the QP kernels are expected to do with a problem of n_pieces polytopes with nfaces_host[n_pieces] faces: the host's
 * description of their memory plan (csrc/sogm_qp_layout.hpp, which also sizes the planner's QP scratch) evaluated with the
 * dynamic LDS this planner was granted.  The kernels compute their plan themselves, from the same constants and byte
 * totals; tests/test_qp_gpu.py holds the path they report (SOGM_QP_STAT_PATH) to this one.  host out8: {register-resident iteration, every row array in LDS (the two bits of
 * SOGM_QP_STAT_PATH), dynamic LDS granted, dynamic LDS used, bytes of the agent's HBM scratch used, K1 in LDS,
 * general rows, safety rows}.  No GPU work. */
int sogm_debug_qp_layout(sogm_planner *p, int n_pieces, const int32_t *nfaces_host, long long *out8);

#ifdef __cplusplus
}
#endif
#endif /* SOGM_ABI_DEBUG_H */
