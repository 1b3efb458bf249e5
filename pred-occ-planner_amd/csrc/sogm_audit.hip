// Flight audit (include/sogm_abi.h "flight audit"): the positions the agents fly, sampled at 100 Hz from the executed
// tables, against each other and against the moving cylinders.  Five launches, stream-ordered, no host round trip:
//   k_audit_pos     one wave per (agent, tick): the tick's record and the one before it staged in LDS, lanes evaluate the
//                   tick's samples -> pos [samples][n_total][3]
//   k_audit_sample  one lane per (sample, audited agent), 64 agents of one sample per workgroup: every other agent's position
//                   (64 x 64 tiles in LDS), then the cylinders (chunks of 64 in LDS) -> per (sample, agent) minima + counts;
//                   the same kernel again in its writing form puts the events at their scanned offsets
//   k_audit_scan    one workgroup: exclusive scan of the per-(sample, agent) event counts (their order IS the event order)
//   k_audit_fold    one lane per audited agent walks the samples in order and updates its accumulator
// With SOGM_AUDIT_RINGS k_audit_sample runs in its RINGS form: the same lane per (sample, agent) walks the same chunks of
// records in index order — which IS the event order and the tie rule of min_gap — and takes sogm_ring.hpp's ring_box_gap
// for a type-2 record where it takes the cylinder's gap for every other; the chunk's ring frames are staged in LDS by the
// lanes that load the records, the 64 unit vectors are built in LDS once per workgroup.
#include "sogm_device.hpp"
#include "sogm_ring.hpp"

#include <cmath>
#include <cstdio>

namespace sogm {
namespace {

constexpr int AUDIT_WG = 64;

struct AuditDims {
  double t0, period, sample_dt, t_obs;
  double bx, by, bz, goal_tol;
  int    first_tick, m, n_ticks, n_total, agent0, n_local, n_cyl, capacity;
};

// a record of a chunk as the ring form stages it
struct AuditRing {
  RingBody body;
  int      is_ring, valid;
};
template <bool RINGS>
struct AuditRingLds {
  static constexpr int N = RINGS ? AUDIT_WG : 1;
};

// sample s of the call (tick s / m, sample s % m of that tick): times built from integers
__device__ inline double sample_time(const AuditDims &d, int s) {
  const int k = s / d.m, j = s - k * d.m;
  return (d.t0 + (double)(d.first_tick + k) * d.period) + (double)j * d.sample_dt;
}

__device__ inline double norm3(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

__global__ __launch_bounds__(AUDIT_WG) void k_audit_pos(AuditDims d, const SogmTrajRecord *__restrict__ tables,
                                                        const SogmTrajRecord *__restrict__ prev_table,
                                                        const double *__restrict__ fallback, double *__restrict__ pos) {
  __shared__ __attribute__((aligned(16))) SogmTrajRecord s_rec[2];   // [0] tick k's record, [1] the one before
  const int a = blockIdx.x, k = blockIdx.y;
  const SogmTrajRecord *prev = k > 0 ? tables + (size_t)(k - 1) * d.n_total + a : (prev_table ? prev_table + a : nullptr);
  copy_record(&s_rec[0], tables + (size_t)k * d.n_total + a, threadIdx.x, AUDIT_WG);
  if (prev) {
    copy_record(&s_rec[1], prev, threadIdx.x, AUDIT_WG);
  } else if (threadIdx.x == 0) {
    s_rec[1].n_pieces = 0;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < d.m; j += AUDIT_WG) {
    const int    s = k * d.m + j;
    const double t = sample_time(d, s);
    double       o[9] = {fallback[a * 3], fallback[a * 3 + 1], fallback[a * 3 + 2]};
    for (int r = 0; r < 2; ++r) {
      const SogmTrajRecord &rec = s_rec[r];
      if (rec.n_pieces > 0 && rec.time_start <= t) {
        traj_eval_record(rec, t, o);
        break;
      }
    }
    double *p = pos + ((size_t)s * d.n_total + a) * 3;
    p[0] = o[0];
    p[1] = o[1];
    p[2] = o[2];
  }
}

// per (sample, audited agent)
struct AuditCell {
  double min_sep, min_gap;
  int    sep_idx, gap_idx, n_agent, n_obs;
};

// WRITE = false: minima and counts into cells / counts; WRITE = true: the events at base + offs[cell] (capacity permitting)
template <bool WRITE, bool RINGS>
__global__ __launch_bounds__(AUDIT_WG) void k_audit_sample(AuditDims d, const double *__restrict__ pos,
                                                           const SogmCylinder *__restrict__ cyl,
                                                           AuditCell *__restrict__ cells, int32_t *__restrict__ counts,
                                                           const long long *__restrict__ offs,
                                                           const long long *__restrict__ base,
                                                           SogmAuditEvent *__restrict__ events) {
  __shared__ double s_p[AUDIT_WG][3];
  __shared__ double s_c[AUDIT_WG][5];   // x, y (at the sample's time), z, w, h: per chunk of cylinders
  __shared__ AuditRing s_r[AuditRingLds<RINGS>::N];          // the chunk's type-2 records
  __shared__ double    s_tab[AuditRingLds<RINGS>::N][2];     // the 64 unit vectors
  if (RINGS) {  // level by level: entry i needs its two neighbours of the coarser level (AUDIT_WG == RING_TABLE lanes)
    static_assert(!RINGS || AUDIT_WG == RING_TABLE, "one lane per table entry");
    const int i = threadIdx.x;
    if ((i & 15) == 0) ring_table_axis(s_tab, i);
    for (int step = 8; step >= 1; step >>= 1) {
      __syncthreads();
      if ((i & (2 * step - 1)) == step) ring_table_level(s_tab, i, step);
    }
    __syncthreads();
  }
  const int  s = blockIdx.y, i = blockIdx.x * AUDIT_WG + threadIdx.x;
  const bool live = i < d.n_local;
  const int  cell = s * d.n_local + i;
  long long  at   = 0;
  if (WRITE) {
    const bool any = live && counts[cell] > 0 && *base >= 0;
    if (!__syncthreads_or(any)) return;
    if (live) at = *base + offs[cell];
  }
  const double t  = sample_time(d, s);
  const int    me = d.agent0 + i;
  double       px = 0, py = 0, pz = 0;
  if (live) {
    const double *p = pos + ((size_t)s * d.n_total + me) * 3;
    px = p[0];
    py = p[1];
    pz = p[2];
  }
  AuditCell c{INFINITY, INFINITY, -1, -1, 0, 0};
  for (int j0 = 0; j0 < d.n_total; j0 += AUDIT_WG) {
    __syncthreads();
    const int jj = j0 + threadIdx.x;
    if (jj < d.n_total)
      for (int q = 0; q < 3; ++q) s_p[threadIdx.x][q] = pos[((size_t)s * d.n_total + jj) * 3 + q];
    __syncthreads();
    const int nj = min(AUDIT_WG, d.n_total - j0);
    if (!live) continue;
    for (int u = 0; u < nj; ++u) {
      const int j = j0 + u;
      if (j == me) continue;
      const double dx = px - s_p[u][0], dy = py - s_p[u][1], dz = pz - s_p[u][2];
      const double sep = norm3(dx, dy, dz);
      if (sep < c.min_sep) {
        c.min_sep = sep;
        c.sep_idx = j;
      }
      if (fabs(dx) < d.bx && fabs(dy) < d.by && fabs(dz) < d.bz) {
        if (WRITE && at < d.capacity) events[at] = SogmAuditEvent{t, me, j, SOGM_AUDIT_AGENT, 0};
        ++at;
        ++c.n_agent;
      }
    }
  }
  const double dt = t - d.t_obs;
  for (int c0 = 0; c0 < d.n_cyl; c0 += AUDIT_WG) {
    __syncthreads();
    const int cc = c0 + threadIdx.x;
    if (cc < d.n_cyl) {
      const SogmCylinder &o = cyl[cc];
      s_c[threadIdx.x][0]   = o.x + o.vx * dt;
      s_c[threadIdx.x][1]   = o.y + o.vy * dt;
      s_c[threadIdx.x][2]   = o.z;
      s_c[threadIdx.x][3]   = o.w;
      s_c[threadIdx.x][4]   = o.h;
      if (RINGS) {
        AuditRing &q = s_r[threadIdx.x];
        RingFrame  f;
        q.is_ring = o.type == 2;
        q.valid   = q.is_ring && ring_frame(o, f);
        if (q.valid) {
          q.body.c[0] = s_c[threadIdx.x][0], q.body.c[1] = s_c[threadIdx.x][1], q.body.c[2] = o.z;
          q.body.R = f.R, q.body.rho = f.rho;
          for (int e = 0; e < 3; ++e) q.body.e1[e] = f.e1[e], q.body.e2[e] = f.e2[e];
        }
      }
    }
    __syncthreads();
    const int nc = min(AUDIT_WG, d.n_cyl - c0);
    if (!live) continue;
    for (int u = 0; u < nc; ++u) {
      double gap;
      if (RINGS && s_r[u].is_ring) {
        if (!s_r[u].valid) continue;   // not a ring: k_audit_scan refuses the call
        const double a[3] = {px, py, pz}, body[3] = {d.bx, d.by, d.bz};
        gap = ring_box_gap(s_r[u].body, a, body, s_tab);
      } else {
        if (!(fabs(pz - s_c[u][2]) < (s_c[u][4] + d.bz) * 0.5)) continue;   // no z overlap
        const double ex = fmax(fabs(s_c[u][0] - px) - d.bx * 0.5, 0.0);
        const double ey = fmax(fabs(s_c[u][1] - py) - d.by * 0.5, 0.0);
        gap             = sqrt(ex * ex + ey * ey) - s_c[u][3] * 0.5;
      }
      if (gap < c.min_gap) {
        c.min_gap = gap;
        c.gap_idx = c0 + u;
      }
      if (gap < 0.0) {
        if (WRITE && at < d.capacity) events[at] = SogmAuditEvent{t, me, c0 + u, SOGM_AUDIT_OBSTACLE, 0};
        ++at;
        ++c.n_obs;
      }
    }
  }
  if (!WRITE && live) {
    cells[cell]  = c;
    counts[cell] = c.n_agent + c.n_obs;
  }
}

// one workgroup of 1024 lanes: offs = exclusive scan of counts; *n_events += total (saturating); a record that is not
// audited (a type other than 3; with `rings`, other than 3 or a type 2 that is a ring) poisons *n_events (-1).  base_out = *n_events before this call (-1: poisoned, nothing is written or folded).
__global__ __launch_bounds__(1024) void k_audit_scan(const int32_t *__restrict__ counts, long long n,
                                                     const SogmCylinder *__restrict__ cyl, int n_cyl, int rings,
                                                     long long *__restrict__ offs, long long *__restrict__ base_out,
                                                     int32_t *__restrict__ n_events) {
  __shared__ long long s_sum[1024];
  __shared__ int       s_bad;
  const int       tid   = threadIdx.x;
  const long long chunk = (n + 1023) / 1024, lo = min(n, chunk * tid), hi = min(n, lo + chunk);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int c = tid; c < n_cyl; c += 1024)
    if (cyl[c].type != 3) {
      RingFrame f;
      if (!(rings && cyl[c].type == 2 && ring_frame(cyl[c], f))) s_bad = 1;
    }
  long long sum = 0;
  for (long long q = lo; q < hi; ++q) sum += counts[q];
  s_sum[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {   // inclusive Hillis-Steele scan of the 1024 chunk sums
    const long long v = tid >= off ? s_sum[tid - off] : 0;
    __syncthreads();
    s_sum[tid] += v;
    __syncthreads();
  }
  long long run = s_sum[tid] - sum;
  for (long long q = lo; q < hi; ++q) {
    offs[q] = run;
    run += counts[q];
  }
  if (tid == 0) {
    const long long prev = *n_events;
    if (prev < 0 || s_bad) {
      *base_out = -1;
      *n_events = -1;
    } else {
      *base_out         = prev;
      const long long t = prev + s_sum[1023];
      *n_events         = (int32_t)(t > 2147483647LL ? 2147483647LL : t);
    }
  }
}

__global__ __launch_bounds__(AUDIT_WG) void k_audit_fold(AuditDims d, const double *__restrict__ pos,
                                                         const AuditCell *__restrict__ cells,
                                                         const double *__restrict__ goals,
                                                         const long long *__restrict__ base,
                                                         SogmAuditAgent *__restrict__ acc) {
  const int i = blockIdx.x * AUDIT_WG + threadIdx.x;
  if (i >= d.n_local || *base < 0) return;
  SogmAuditAgent a  = acc[i];
  const int      me = d.agent0 + i;
  const double   gx = goals[i * 3], gy = goals[i * 3 + 1], gz = goals[i * 3 + 2];
  const int      ns = d.n_ticks * d.m;
  for (int s = 0; s < ns; ++s) {
    const double     t = sample_time(d, s);
    const AuditCell &c = cells[s * d.n_local + i];
    const double    *p = pos + ((size_t)s * d.n_total + me) * 3;
    if (c.min_sep < a.min_sep) {
      a.min_sep       = c.min_sep;
      a.min_sep_time  = t;
      a.min_sep_agent = c.sep_idx;
    }
    if (c.min_gap < a.min_gap) {
      a.min_gap          = c.min_gap;
      a.min_gap_time     = t;
      a.min_gap_obstacle = c.gap_idx;
    }
    a.agent_samples += c.n_agent > 0;
    a.obstacle_samples += c.n_obs > 0;
    if ((c.n_agent > 0 || c.n_obs > 0) && a.first_collision_time < 0) a.first_collision_time = t;
    if (a.goal_time < 0 && norm3(p[0] - gx, p[1] - gy, p[2] - gz) < d.goal_tol) a.goal_time = t;
    if (a.has_last) a.path_length += norm3(p[0] - a.last_pos[0], p[1] - a.last_pos[1], p[2] - a.last_pos[2]);
    a.last_pos[0] = p[0];
    a.last_pos[1] = p[1];
    a.last_pos[2] = p[2];
    a.has_last    = 1;
  }
  a.n_samples += ns;
  acc[i] = a;
}

__global__ __launch_bounds__(AUDIT_WG) void k_audit_init(SogmAuditAgent *__restrict__ acc, int n) {
  const int i = blockIdx.x * AUDIT_WG + threadIdx.x;
  if (i >= n) return;
  SogmAuditAgent a{};
  a.min_gap = a.min_sep = INFINITY;
  a.min_gap_time = a.min_sep_time = a.goal_time = a.first_collision_time = -1.0;
  a.min_gap_obstacle = a.min_sep_agent = -1;
  acc[i] = a;
}

int audit_refuse(const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "sogm_swarm_audit: %s", what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

int audit_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error_text("flight audit: no HIP device");
    return SOGM_ERR_NO_DEVICE;
  }
  return SOGM_OK;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_audit_init_agents(SogmAuditAgent *acc, int n_local, void *stream) {
  if (!acc || n_local < 0) {
    sogm::set_error_text("sogm_audit_init_agents: null accumulator or negative count");
    return SOGM_ERR_INVALID_ARG;
  }
  if (n_local == 0) return SOGM_OK;
  if (int rc = sogm::audit_device()) return rc;
  hipLaunchKernelGGL(sogm::k_audit_init, dim3((n_local + sogm::AUDIT_WG - 1) / sogm::AUDIT_WG), dim3(sogm::AUDIT_WG), 0,
                     (hipStream_t)stream, acc, n_local);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

extern "C" int sogm_swarm_audit(const SogmAuditParams *prm, const SogmTrajRecord *tables, int n_ticks, int n_total,
                                const SogmTrajRecord *prev_table, double t0, int first_tick, double period, int agent0,
                                int n_local, const double *fallback_pos, const double *goals,
                                const SogmCylinder *cylinders, int n_cyl, SogmAuditAgent *acc, SogmAuditEvent *events,
                                int32_t *n_events, void *stream) {
  using namespace sogm;
  if (!prm || !tables || !fallback_pos || !goals || !acc || !n_events) return audit_refuse("null pointer");
  if (n_ticks < 0 || n_total < 1 || n_cyl < 0 || first_tick < 0 || prm->event_capacity < 0)
    return audit_refuse("negative count (or n_total < 1)");
  if (agent0 < 0 || n_local < 1 || n_local > n_total - agent0) return audit_refuse("agent0 / n_local out of range");
  if (n_cyl > 0 && !cylinders) return audit_refuse("null cylinders with n_cyl > 0");
  if (prm->event_capacity > 0 && !events) return audit_refuse("null events with event_capacity > 0");
  if (!(prm->sample_dt > 0) || !(period > 0) || !(prm->body[0] > 0) || !(prm->body[1] > 0) || !(prm->body[2] > 0) ||
      !(prm->goal_tolerance >= 0) || !std::isfinite(t0) || !std::isfinite(prm->t_obstacles))
    return audit_refuse("sample_dt, period and body must be positive, goal_tolerance >= 0, times finite");
  const double ratio = period / prm->sample_dt, m = std::nearbyint(ratio);
  if (!(std::fabs(ratio - m) <= 1e-9) || m < 1 || m > 4096) return audit_refuse("period / sample_dt is not a whole number (1 .. 4096)");
  const long long cells = (long long)n_ticks * (long long)m * n_local;
  if ((long long)n_ticks * (long long)m > 65535 || (long long)n_ticks * (long long)m * n_total > (1LL << 28))
    return audit_refuse("too many samples in one call (n_ticks * period / sample_dt <= 65535)");
  if (int rc = audit_device()) return rc;
  if (n_ticks == 0) return SOGM_OK;
  AuditDims d{};
  d.t0 = t0, d.period = period, d.sample_dt = prm->sample_dt, d.t_obs = prm->t_obstacles;
  d.bx = prm->body[0], d.by = prm->body[1], d.bz = prm->body[2], d.goal_tol = prm->goal_tolerance;
  d.first_tick = first_tick, d.m = (int)m, d.n_ticks = n_ticks, d.n_total = n_total, d.agent0 = agent0;
  d.n_local = n_local, d.n_cyl = n_cyl, d.capacity = prm->event_capacity;
  const int    ns = n_ticks * d.m;
  hipStream_t  st = (hipStream_t)stream;
  // scratch: positions, cells, counts, offsets, base
  const size_t b_pos = sizeof(double) * 3 * (size_t)ns * n_total, b_cell = sizeof(AuditCell) * (size_t)cells;
  const size_t b_cnt = ((sizeof(int32_t) * (size_t)cells + 15) / 16) * 16, b_off = sizeof(long long) * (size_t)cells;
  char        *scratch = nullptr;
  SOGM_HIP_CHECK(hipMallocAsync((void **)&scratch, b_pos + b_cell + b_cnt + b_off + 16, st));
  double    *pos   = (double *)scratch;
  AuditCell *cell  = (AuditCell *)(scratch + b_pos);
  int32_t   *cnt   = (int32_t *)(scratch + b_pos + b_cell);
  long long *offs  = (long long *)(scratch + b_pos + b_cell + b_cnt);
  long long *base  = offs + cells;
  const dim3 g_smp((n_local + AUDIT_WG - 1) / AUDIT_WG, ns);
  hipLaunchKernelGGL(k_audit_pos, dim3(n_total, n_ticks), dim3(AUDIT_WG), 0, st, d, tables, prev_table, fallback_pos, pos);
  const int  rings = prm->flags & SOGM_AUDIT_RINGS;
  if (rings)
    hipLaunchKernelGGL((k_audit_sample<false, true>), g_smp, dim3(AUDIT_WG), 0, st, d, pos, cylinders, cell, cnt, nullptr,
                       nullptr, nullptr);
  else
    hipLaunchKernelGGL((k_audit_sample<false, false>), g_smp, dim3(AUDIT_WG), 0, st, d, pos, cylinders, cell, cnt, nullptr,
                       nullptr, nullptr);
  hipLaunchKernelGGL(k_audit_scan, dim3(1), dim3(1024), 0, st, cnt, cells, cylinders, n_cyl, rings, offs, base, n_events);
  if (d.capacity > 0) {
    if (rings)
      hipLaunchKernelGGL((k_audit_sample<true, true>), g_smp, dim3(AUDIT_WG), 0, st, d, pos, cylinders, cell, cnt, offs, base,
                         events);
    else
      hipLaunchKernelGGL((k_audit_sample<true, false>), g_smp, dim3(AUDIT_WG), 0, st, d, pos, cylinders, cell, cnt, offs, base,
                         events);
  }
  hipLaunchKernelGGL(k_audit_fold, dim3((n_local + AUDIT_WG - 1) / AUDIT_WG), dim3(AUDIT_WG), 0, st, d, pos, cell, goals,
                     base, acc);
  const hipError_t e = hipGetLastError();
  (void)hipFreeAsync(scratch, st);
  SOGM_HIP_CHECK(e);
  return SOGM_OK;
}
