// sogm_finish.hpp — how a replan ends.  The outcome rule is plain C++ for host and device (tests/finish_rules_host_test.cpp
// builds it with the host compiler); behind __HIPCC__ the device bodies the finishing kernels inline: isSafeAfterOpt for one
// pair, its one-lane-per-record prefilter, and what the finishing role does for one agent (the finishing blocks of sogm_corridor.hip's k_worker_flow,
// sogm_flight_light.hpp's k_flight_light).
#pragma once
#include "sogm_lp.hpp"

namespace sogm {

// where replan() ended (baseline_fake.cpp: :292 no path, :405-419 corridors, :447 QP, :455 unsafe): a SOGM_CNT_* index.
// replan_outcome_of takes the QP's status as a callable and reads it only behind a search and corridors — the device's
// wave-per-agent bodies have always loaded it there, and the code the compiler makes of the finishing blocks of k_worker_flow and k_flight_light
// follows these loads (profiles/EXPERIMENTS.md); replan_outcome is the same rule over plain values.
template <class Status>
LDS_HD inline int replan_outcome_of(int ret, int npoly, Status status, bool safe) {
  if (ret == 0) return SOGM_CNT_FAIL_SEARCH;
  if (npoly <= 0) return SOGM_CNT_FAIL_CORRIDOR;
  const int st = status();
  if (!(st == 1 || st == 2)) return SOGM_CNT_FAIL_QP;
  if (!safe) return SOGM_CNT_FAIL_UNSAFE;
  return SOGM_CNT_REPLAN_OK;
}
LDS_HD inline int replan_outcome(int ret, int npoly, int status, bool safe) {
  return replan_outcome_of(ret, npoly, [=] { return status; }, safe);
}
// "solved": everything in front of isSafeAfterOpt went well, i.e. replan_outcome_of(.., safe = true) is SOGM_CNT_REPLAN_OK;
// a replan is good when it is solved and safe.  Written as the conjunction because finish_agent branches on it in front of
// the swarm check (tests/finish_rules_host_test.cpp holds the two to each other over its whole table).
template <class Status>
LDS_HD inline bool replan_solved(int ret, int npoly, Status status) {
  return ret != 0 && npoly > 0 && (status() == 1 || status() == 2);
}

}  // namespace sogm

#ifdef __HIPCC__
#include "sogm_planner.hpp"

namespace sogm {

// ------------------------------------------------------------------------------------------------
// ParticleATC::isSafeAfterOpt (traj_coordinator/src/particles.cpp:223-283): one workgroup per
// (other agent's record, ego agent).  Set A = the new trajectory's control points, set B = the record's
// control points from the piece that contains t_now onwards; separable iff the feasibility LP
// n.a + d >= 1, n.b + d <= -1 (utils/separator/src/separator_glpk.cpp:75-190, zero objective) has a
// solution — solved with the same sdlp LP as the corridor checks, the four variables boxed at +-1e4 (8 extra
// rows): the projective LP reports a feasible point at infinity (two crossing segments: the plane through both)
// as "-inf", GLPK's affine model calls that infeasible; with the box the result is finite or +inf.
// ------------------------------------------------------------------------------------------------
// One (new trajectory of agent a, record r) pair, executed by one wave: true = NOT separable (unsafe).
// ca: the agent's 5 M control points; sc: the wave's LP scratch in LDS.
__device__ __forceinline__ bool deconflict_pair_unsafe(const double *ca, int M, const SogmTrajRecord &r, int ego_id,
                                                       double now, const LpScratch &sc, unsigned long long *counters) {
  if (M <= 0) return false;  // nothing optimised for this agent
  if (r.n_pieces <= 0 || r.drone_id == ego_id) return false;
  double time_end = r.time_start;
  for (int k = 0; k < r.n_pieces; ++k) time_end += r.duration[k];
  if (!(r.time_start < now && now < time_end)) return false;
  double t     = now - r.time_start;  // Bezier::locatePiece (bernstein.hpp:164-172)
  int    piece = r.n_pieces - 1;
  for (int k = 0; k < r.n_pieces; ++k) {
    t -= r.duration[k];
    if (t < 0) {
      piece = k;
      break;
    }
  }
  const int nA = 5 * M, nB = (r.n_pieces - piece) * 5;
  if (nA + nB > DECONFLICT_MAX_ROWS) {  // LP capacity: treated as "not separable" (oracle does the same)
    if ((threadIdx.x & 63) == 0 && counters) atomicAdd(&counters[SOGM_CNT_DECONFLICT_CAPACITY], 1ull);
    return true;
  }
  double       *A = sc.A(), *b = sc.b();
  const double *cb = r.cpts + piece * 15;
  // Disjoint bounding boxes are separated by an axis-aligned plane (the LP is feasible): most pairs of
  // a swarm end here without touching the LP.  64-lane min/max over the two point sets.
  {
    double lo[6], hi[6];
    for (int k = 0; k < 6; ++k) {
      lo[k] = INFINITY;
      hi[k] = -INFINITY;
    }
    for (int q = threadIdx.x; q < nA; q += 64)
      for (int k = 0; k < 3; ++k) {
        lo[k] = fmin(lo[k], ca[q * 3 + k]);
        hi[k] = fmax(hi[k], ca[q * 3 + k]);
      }
    for (int q = threadIdx.x; q < nB; q += 64)
      for (int k = 0; k < 3; ++k) {
        lo[3 + k] = fmin(lo[3 + k], cb[q * 3 + k]);
        hi[3 + k] = fmax(hi[3 + k], cb[q * 3 + k]);
      }
    bool apart = false;
    for (int k = 0; k < 6; ++k)
      for (int d = 32; d >= 1; d >>= 1) {
        lo[k] = fmin(lo[k], __shfl_xor(lo[k], d, 64));
        hi[k] = fmax(hi[k], __shfl_xor(hi[k], d, 64));
      }
    for (int k = 0; k < 3; ++k) apart = apart || hi[k] < lo[3 + k] || hi[3 + k] < lo[k];
    if (apart) return false;  // wave-uniform
    // more candidate normals (face / body diagonals, the line between the box centres), same list and
    // order as oracle/deconflict_oracle.cpp: disjoint projections = separable, no LP needed
    double dirs[11][3] = {{1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1}, {0, 1, 1}, {0, 1, -1},
                          {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}, {0, 0, 0}};
    for (int k = 0; k < 3; ++k) dirs[10][k] = 0.5 * (lo[3 + k] + hi[3 + k]) - 0.5 * (lo[k] + hi[k]);
#pragma unroll
    for (int q = 0; q < 11; ++q) {  // unrolled: the normals are immediates, not a scratch-memory table
      const double n0 = dirs[q][0], n1 = dirs[q][1], n2 = dirs[q][2];
      double loA = INFINITY, hiA = -INFINITY, loB = INFINITY, hiB = -INFINITY;
      for (int i = threadIdx.x; i < nA; i += 64) {
        const double v = (n0 * ca[i * 3] + n1 * ca[i * 3 + 1]) + n2 * ca[i * 3 + 2];
        loA = fmin(loA, v);
        hiA = fmax(hiA, v);
      }
      for (int i = threadIdx.x; i < nB; i += 64) {
        const double v = (n0 * cb[i * 3] + n1 * cb[i * 3 + 1]) + n2 * cb[i * 3 + 2];
        loB = fmin(loB, v);
        hiB = fmax(hiB, v);
      }
      for (int d = 32; d >= 1; d >>= 1) {
        loA = fmin(loA, __shfl_xor(loA, d, 64));
        hiA = fmax(hiA, __shfl_xor(hiA, d, 64));
        loB = fmin(loB, __shfl_xor(loB, d, 64));
        hiB = fmax(hiB, __shfl_xor(hiB, d, 64));
      }
      if (hiA < loB || hiB < loA) return false;  // wave-uniform
    }
  }
  for (int q = threadIdx.x; q < nA + nB; q += 64) {
    if (q < nA) {
      A[q * 4 + 0] = -ca[q * 3 + 0];
      A[q * 4 + 1] = -ca[q * 3 + 1];
      A[q * 4 + 2] = -ca[q * 3 + 2];
      A[q * 4 + 3] = -1.0;
    } else {
      const int e  = q - nA;
      A[q * 4 + 0] = cb[e * 3 + 0];
      A[q * 4 + 1] = cb[e * 3 + 1];
      A[q * 4 + 2] = cb[e * 3 + 2];
      A[q * 4 + 3] = 1.0;
    }
    b[q] = -1.0;
  }
  if (threadIdx.x < 8) {  // x_k <= 1e4, -x_k <= 1e4
    const int q = nA + nB + threadIdx.x, k = threadIdx.x >> 1;
    for (int j = 0; j < 4; ++j) A[q * 4 + j] = j == k ? ((threadIdx.x & 1) ? -1.0 : 1.0) : 0.0;
    b[q] = 1.0e4;
  }
  wave_lds_sync();
  const double c[4] = {0, 0, 0, 0};
  double       x[4];
  const double v = linprog_wave<4>(c, nA + nB + 8, A, b, x, sc.work, sc.perm);  // the whole wave solves the LP
  wave_lds_sync();
  return v == INFINITY || v == -INFINITY;
}

// The cheap part of deconflict_pair_unsafe with ONE LANE PER RECORD (the dataflow replan's finishing kernel: the
// wave-per-pair form above walks the swarm table record by record, two dependent global round trips each, and
// those round trips are the first thing a streaming clear beside it stretches).  Same decisions bit for bit: the
// activity tests, the bounding boxes and the 11 candidate-normal projections are minima / maxima of the same
// products, whatever the order.  sA: the agent's nA control points (LDS), boxA lo[3] hi[3], prA[q][2] = (lo, hi) of
// A's projection on the ten fixed normals.  Returns true when the pair still needs the full test (the LP, or the
// capacity rule), i.e. whenever deconflict_pair_unsafe would not return false before its LP assembly.
__device__ inline bool deconflict_prefilter(const double *sA, int nA, const double *boxA, const double (*prA)[2],
                                            const SogmTrajRecord &r, int ego_id, double now) {
  const int np = r.n_pieces;
  if (np <= 0 || r.drone_id == ego_id) return false;
  const double ts = r.time_start;
  double       time_end = ts;
  for (int k = 0; k < np; ++k) time_end += r.duration[k];
  if (!(ts < now && now < time_end)) return false;
  double t     = now - ts;
  int    piece = np - 1;
  for (int k = 0; k < np; ++k) {
    t -= r.duration[k];
    if (t < 0) {
      piece = k;
      break;
    }
  }
  const int nB = (np - piece) * 5;
  if (nA + nB > DECONFLICT_MAX_ROWS) return true;  // the capacity rule (and its counter) live in the full test
  const double *cb = r.cpts + piece * 15;
  const double  dirs[10][3] = {{1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1}, {0, 1, 1},
                               {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  double plo[10], phi[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    plo[q] = INFINITY;
    phi[q] = -INFINITY;
  }
#pragma unroll 4
  for (int i = 0; i < nB; ++i) {
    const double x = cb[i * 3], y = cb[i * 3 + 1], z = cb[i * 3 + 2];
    lo[0] = fmin(lo[0], x);
    hi[0] = fmax(hi[0], x);
    lo[1] = fmin(lo[1], y);
    hi[1] = fmax(hi[1], y);
    lo[2] = fmin(lo[2], z);
    hi[2] = fmax(hi[2], z);
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      const double v = (dirs[q][0] * x + dirs[q][1] * y) + dirs[q][2] * z;
      plo[q]         = fmin(plo[q], v);
      phi[q]         = fmax(phi[q], v);
    }
  }
  for (int k = 0; k < 3; ++k)
    if (boxA[3 + k] < lo[k] || hi[k] < boxA[k]) return false;  // disjoint bounding boxes
#pragma unroll
  for (int q = 0; q < 10; ++q)
    if (prA[q][1] < plo[q] || phi[q] < prA[q][0]) return false;
  // the line between the box centres
  double n[3];
  for (int k = 0; k < 3; ++k) n[k] = 0.5 * (lo[k] + hi[k]) - 0.5 * (boxA[k] + boxA[3 + k]);
  double loA = INFINITY, hiA = -INFINITY, loB = INFINITY, hiB = -INFINITY;
  for (int i = 0; i < nA; ++i) {
    const double v = (n[0] * sA[i * 3] + n[1] * sA[i * 3 + 1]) + n[2] * sA[i * 3 + 2];
    loA            = fmin(loA, v);
    hiA            = fmax(hiA, v);
  }
  for (int i = 0; i < nB; ++i) {
    const double v = (n[0] * cb[i * 3] + n[1] * cb[i * 3 + 1]) + n[2] * cb[i * 3 + 2];
    loB            = fmin(loB, v);
    hiB            = fmax(hiB, v);
  }
  if (hiA < loB || hiB < loA) return false;
  return true;
}

// What the finishing role does for one agent (one wave): ParticleATC::isSafeAfterOpt against every record of the swarm
// (when a swarm is set), then the agent's SogmTrajRecord / ok flag and the publication — shared by the finishing blocks of k_worker_flow
// (sogm_replan) and k_flight_light (sogm_flight_run).  Returns bit 0 = safe, bit 1 = replan() returned true.
__device__ __forceinline__ int finish_agent(const FinishArgs &f, int a, const LpScratch &sc, int lane) {
  const int M    = f.npoly[a];
  int       safe = 1;
  const int32_t *st = f.status + a;  // (captured as the word's address: the form whose code is the earlier chain's)
  const bool solved = replan_solved(f.ret[a], M, [st] { return *st; });
  if (f.swarm && solved) {  // unsolved agents fail anyway: the check cannot change their outcome
    const double *ca  = f.cpts + (size_t)a * SOGM_MAX_PIECES * 15;
    const int     ego = f.swarm_ego[a];
    const double  now = f.swarm_now[a];
    const int     nA  = 5 * M;
    const SogmTrajRecord *swarm = f.swarm + (size_t)a * f.swarm_stride;  // the one table, or the agent's own view of it
    // set A once per agent: its points in LDS (the LP scratch is idle until a pair needs the LP), its box and
    // its projections on the ten fixed normals as wave-uniform values
    double *sA = sc.work;
    double  boxA[6], prA[10][2];
    auto stage_A = [&]() {
      for (int q = lane; q < nA * 3; q += 64) sA[q] = ca[q];
      wave_lds_sync();
    };
    stage_A();
    {
      const double dirs[10][3] = {{1, 1, 0}, {1, -1, 0}, {1, 0, 1}, {1, 0, -1}, {0, 1, 1},
                                  {0, 1, -1}, {1, 1, 1}, {1, 1, -1}, {1, -1, 1}, {1, -1, -1}};
      double lo[13], hi[13];
#pragma unroll
      for (int k = 0; k < 13; ++k) {
        lo[k] = INFINITY;
        hi[k] = -INFINITY;
      }
      for (int q = lane; q < nA; q += 64) {
        const double x = sA[q * 3], y = sA[q * 3 + 1], z = sA[q * 3 + 2];
        lo[0] = fmin(lo[0], x);
        hi[0] = fmax(hi[0], x);
        lo[1] = fmin(lo[1], y);
        hi[1] = fmax(hi[1], y);
        lo[2] = fmin(lo[2], z);
        hi[2] = fmax(hi[2], z);
#pragma unroll
        for (int k = 0; k < 10; ++k) {
          const double v = (dirs[k][0] * x + dirs[k][1] * y) + dirs[k][2] * z;
          lo[3 + k]      = fmin(lo[3 + k], v);
          hi[3 + k]      = fmax(hi[3 + k], v);
        }
      }
#pragma unroll
      for (int k = 0; k < 13; ++k)
        for (int d = 32; d >= 1; d >>= 1) {
          lo[k] = fmin(lo[k], __shfl_xor(lo[k], d, 64));
          hi[k] = fmax(hi[k], __shfl_xor(hi[k], d, 64));
        }
      for (int k = 0; k < 3; ++k) {
        boxA[k]     = lo[k];
        boxA[3 + k] = hi[k];
      }
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        prA[k][0] = lo[3 + k];
        prA[k][1] = hi[3 + k];
      }
    }
    // one lane per record decides whether the pair needs the full test; the few that do go through it one at a
    // time, in record order (first unsafe pair ends the check, as the sequential loop did)
    for (int i0 = 0; i0 < f.n_swarm && safe; i0 += 64) {
      const int  i    = i0 + lane;
      const bool need = i < f.n_swarm && deconflict_prefilter(sA, nA, boxA, prA, swarm[i], ego, now);
      unsigned long long m = __ballot(need);
      bool               lp_ran = false;
      while (m != 0 && safe) {
        const int j = __builtin_ctzll(m);
        m &= m - 1;
        if (deconflict_pair_unsafe(ca, M, swarm[i0 + j], ego, now, sc, f.counters)) safe = 0;
        lp_ran = true;
      }
      if (lp_ran && safe && i0 + 64 < f.n_swarm) stage_A();  // the LP used the scratch that held set A
    }
  }
#ifdef SOGM_FLOW_DEBUG
  if (lane == 0) f.out_safe[a] = 101;
#else
  if (lane == 0 && f.out_safe) f.out_safe[a] = safe;
#endif
  // BezierTraj record (plan_manager.cpp:364-399); n_pieces = 0 marks "replan() returned false".
  // Publication (sogm_planner_set_publish): a successful replan's record also goes — in the same stores — into
  // the host's own table (latest wins; a failed replan keeps executing the previous trajectory, :176-196) and the
  // agent's current record into the next tick's swarm table, HERE, where the stores overlap with the other agents'
  // chains, instead of in a store-heavy kernel after the replan (beside the streaming clear that kernel took 2 ms).
  const bool      good = solved && safe != 0;  // replan_outcome is SOGM_CNT_REPLAN_OK
  SogmTrajRecord *dst[3] = {f.out + a, (good && f.pub_own) ? f.pub_own + a : nullptr,
                            (good && f.pub_own && f.pub_table) ? f.pub_table + a : nullptr};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    SogmTrajRecord *r = dst[k];
    if (!r) continue;  // wave-uniform
    for (int i = lane; i < SOGM_MAX_PIECES; i += 64) r->duration[i] = (good && i < M) ? f.corridor_tau : 0.0;
    for (int i = lane; i < SOGM_MAX_PIECES * 15; i += 64)
      r->cpts[i] = (good && i < M * 15) ? f.cpts[(size_t)a * SOGM_MAX_PIECES * 15 + i] : 0.0;
    if (lane == 0) {
      r->drone_id   = f.drone_ids[a];
      r->time_start = f.t_start[a];
      r->n_pieces   = good ? M : 0;
    }
  }
  if (!good && f.pub_own && f.pub_table)  // the table still lists the trajectory the agent goes on executing
    copy_record(f.pub_table + a, f.pub_own + a, lane);
  if (lane == 0) f.out_ok[a] = good ? 1 : 0;
  return (safe ? 1 : 0) | (good ? 2 : 0);
}

// counts where this replan ended (replan_outcome); one lane
__device__ __forceinline__ void finish_count(const FinishArgs &f, int a, bool safe) {
  if (!f.counters) return;
  if (f.due && f.due[a] == 0) return;  // left out by sogm_planner_set_due's mask: not a replan that was asked for
  const int M = f.npoly[a];
  atomicAdd(&f.counters[replan_outcome_of(f.ret[a], M, [&] { return f.status[a]; }, safe)], 1ull);
}

}  // namespace sogm
#endif
