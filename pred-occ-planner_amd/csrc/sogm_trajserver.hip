// Trajectory server (include/sogm_abi.h "trajectory server"; the rules are sogm_trajserver.hpp's): every agent's look-ahead
// queue of 100 Hz samples and the position commands it publishes, from the executed tables.  Three kernels, stream-ordered:
//   k_traj_server_init  one wave per agent: zeroes the state and the ring, sets the state after the preamble
//   k_traj_server       one wave per agent for all ticks of the call: ring, current and arriving record staged in LDS.  The
//                       bookkeeping (sizes, head and tail, which pushes happen, k) depends on times only and every lane runs
//                       it, uniformly, on its own copy of the scalars; the Bezier evaluations it asks for run one per lane
//                       and land in the ring at their push slots; getYaw then walks the pushed samples in push order.
//   k_camera_poses      one lane per command: Rz(yaw) * cam2body and the camera centre
// No waiting on other workgroups, no atomics; every loop is bounded by a validated argument or by SOGM_TRAJSRV_QUEUE and
// every ring index is masked (TRAJSRV_MASK).
#include "sogm_device.hpp"
#include "sogm_trajserver.hpp"

#include <cmath>
#include <cstdio>

namespace sogm {
namespace {

constexpr int TS_WG = 64;
constexpr int RING_BYTES = (int)sizeof(SogmTrajPoint) * SOGM_TRAJSRV_QUEUE;
static_assert(RING_BYTES % 16 == 0 && sizeof(SogmTrajServerState) % 16 == 0 && sizeof(SogmTrajServerCore) % 16 == 0,
              "rings and states are copied in 16-byte pieces");

struct TrajSrvDims {
  double t0, period, receive_delay;
  int    first_tick, m, n_ticks, n_total, agent0, n_local;
};
struct CameraMount {
  double cam2body[9], offset[3];
};

__device__ __forceinline__ void copy16(void *dst, const void *src, int bytes, int lane) {
  const uint4 *s = reinterpret_cast<const uint4 *>(src);
  uint4       *d = reinterpret_cast<uint4 *>(dst);
  for (int w = lane; w < bytes / 16; w += TS_WG) d[w] = s[w];
}

// bezierCallback for the wave's agent: trajsrv_receive with the evaluations dealt to the lanes
__device__ inline void receive_wave(const SogmTrajServerParams &prm, TrajSrvCore &c, SogmTrajPoint *ring,
                                    const SogmTrajRecord &rec, double now, int lane) {
  const double      tns = rec.time_start, duration = trajsrv_duration(rec);
  const TrajSrvPlan p   = trajsrv_receive_plan(prm, c, now, tns);
  int               first;
  const int         adm = trajsrv_reserve(c, p.n_push, &first);
  __syncthreads();  // the lanes' reads of the samples they published are behind them
  for (int q = lane; q < adm; q += TS_WG) {
    const double t = trajsrv_push_time(prm, p, q);
    double       o[9];
    traj_eval_relative(rec, t, o);
    trajsrv_point(ring[(first + q) & TRAJSRV_MASK], c.ts + t, o);
  }
  __syncthreads();
  trajsrv_yaw_pass(prm, c, ring, first, adm, lane == 0);
  __syncthreads();
  trajsrv_receive_done(c, tns, duration);
}

// PubCallback at the instants t_k + j * sample_dt, j0 <= j < j1 (no record arrives between them), 64 instants per trip: the
// bookkeeping of the trip's instants in order (lane u keeps instant u's), the samples published from what was queued before
// the trip are read, the pushes are evaluated one per lane and stored, getYaw walks them, the samples published from the
// trip's own pushes are read (a short queue: replan_threshold 0.02 keeps two samples), the commands are written.
__device__ inline void timers_wave(const SogmTrajServerParams &prm, TrajSrvCore &c, SogmTrajPoint *ring,
                                   const SogmTrajRecord &traj, double t_k, int j0, int j1, SogmPositionCommand *out,
                                   int lane) {
  for (int b = j0; b < j1; b += TS_WG) {
    const int    n = min(TS_WG, j1 - b);
    TrajSrvTimer mine{0, -1, -1, 0.0};
    bool         mine_old = false;
    int          old_left = c.size, first_push = 0, n_pushed = 0;
    for (int u = 0; u < n; ++u) {
      const TrajSrvTimer tp  = trajsrv_timer_plan(prm, c, t_k + (double)(b + u) * prm.sample_dt);
      const bool         old = old_left > 0;
      if ((tp.flags & SOGM_CMD_PUBLISHED) && !(tp.flags & SOGM_CMD_HELD) && old) --old_left;
      if (tp.push_slot >= 0) {
        if (n_pushed == 0) first_push = tp.push_slot;  // (one pop, one push: the trip's pushes are consecutive slots)
        ++n_pushed;
      }
      if (u == lane) {
        mine     = tp;
        mine_old = old;
      }
    }
    const bool    pub = (mine.flags & SOGM_CMD_PUBLISHED) != 0;
    SogmTrajPoint p{};
    if (pub && mine_old) p = ring[mine.src & TRAJSRV_MASK];
    __syncthreads();
    if (mine.push_slot >= 0) {
      double o[9];
      traj_eval_relative(traj, mine.t_sample, o);
      trajsrv_point(ring[mine.push_slot & TRAJSRV_MASK], c.ts + mine.t_sample, o);
    }
    __syncthreads();
    trajsrv_yaw_pass(prm, c, ring, first_push, n_pushed, lane == 0);
    __syncthreads();
    if (pub && !mine_old) p = ring[mine.src & TRAJSRV_MASK];
    if (lane < n) {
      SogmPositionCommand cmd;
      trajsrv_command(cmd, c, mine, p, t_k + (double)(b + lane) * prm.sample_dt);  // (a held sample: last_yaw as the pushes left it)
      out[b + lane] = cmd;
    }
  }
}

__global__ __launch_bounds__(TS_WG) void k_traj_server(SogmTrajServerParams prm, TrajSrvDims d,
                                                       SogmTrajServerState *__restrict__ state,
                                                       SogmTrajPoint *__restrict__ queue,
                                                       const SogmTrajRecord *__restrict__ tables,
                                                       const SogmTrajRecord *__restrict__ prev_table,
                                                       const int32_t *__restrict__ received,
                                                       SogmPositionCommand *__restrict__ out_cmd) {
  __shared__ __attribute__((aligned(16))) SogmTrajPoint  s_ring[SOGM_TRAJSRV_QUEUE];
  __shared__ __attribute__((aligned(16))) SogmTrajRecord s_rec[2];  // [cur] traj_, [cur ^ 1] the arriving record
  const int i = blockIdx.x, lane = threadIdx.x, a = d.agent0 + i;
  if (i >= d.n_local) return;
  SogmTrajServerState *st = state + i;
  SogmTrajPoint       *q  = queue + (size_t)i * SOGM_TRAJSRV_QUEUE;
  copy16(s_ring, q, RING_BYTES, lane);
  copy_record(&s_rec[0], &st->traj, lane, TS_WG);
  TrajSrvCore c   = st->core;
  int         cur = 0;
  __syncthreads();
  for (int k = 0; k < d.n_ticks; ++k) {
    const double          t_k = d.t0 + (double)(d.first_tick + k) * d.period;
    const SogmTrajRecord *rk  = tables + (size_t)k * d.n_total + a;
    const int             np  = rk->n_pieces;
    bool                  rcv;
    if (received) {
      rcv = received[(size_t)k * d.n_local + i] != 0;
    } else {
      const SogmTrajRecord *pv = k > 0 ? rk - d.n_total : (prev_table ? prev_table + a : nullptr);
      rcv = !pv || pv->n_pieces <= 0 || pv->time_start != rk->time_start;
    }
    rcv = rcv && np > 0 && np <= SOGM_MAX_PIECES;
    // the arrival comes before the timer of the first instant that is not earlier
    const double t_rcv = t_k + d.receive_delay;
    int          j_rcv = 0;
    while (j_rcv < d.m && t_k + (double)j_rcv * prm.sample_dt < t_rcv) ++j_rcv;
    SogmPositionCommand *out = out_cmd + ((size_t)i * d.n_ticks + k) * d.m;
    timers_wave(prm, c, s_ring, s_rec[cur], t_k, 0, j_rcv, out, lane);
    if (rcv) {
      __syncthreads();  // (the record being replaced: its readers are done)
      copy_record(&s_rec[cur ^ 1], rk, lane, TS_WG);
      __syncthreads();
      receive_wave(prm, c, s_ring, s_rec[cur ^ 1], t_rcv, lane);
      cur ^= 1;
    }
    timers_wave(prm, c, s_ring, s_rec[cur], t_k, j_rcv, d.m, out, lane);
  }
  __syncthreads();
  copy16(q, s_ring, RING_BYTES, lane);
  copy_record(&st->traj, &s_rec[cur], lane, TS_WG);
  if (lane == 0) st->core = c;
}

__global__ __launch_bounds__(TS_WG) void k_traj_server_init(SogmTrajServerState *__restrict__ state,
                                                            SogmTrajPoint *__restrict__ queue, int n, double t_trigger,
                                                            const double *__restrict__ init_pos,
                                                            const double *__restrict__ init_yaw) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  const uint4 zero = make_uint4(0, 0, 0, 0);
  uint4      *s = reinterpret_cast<uint4 *>(state + i), *r = reinterpret_cast<uint4 *>(queue + (size_t)i * SOGM_TRAJSRV_QUEUE);
  for (int w = lane; w < (int)(sizeof(SogmTrajServerState) / 16); w += TS_WG) s[w] = zero;
  for (int w = lane; w < RING_BYTES / 16; w += TS_WG) r[w] = zero;
  __syncthreads();
  if (lane == 0) {  // main :527-531 with the trigger behind it
    SogmTrajServerCore c{};
    c.ts = c.te = t_trigger;
    c.last_yaw = init_yaw ? init_yaw[i] : 0.0;
    for (int k = 0; k < 3; ++k) c.init_pos[k] = init_pos[i * 3 + k];
    state[i].core = c;
  }
}

__global__ __launch_bounds__(TS_WG) void k_camera_poses(const SogmPositionCommand *__restrict__ cmd, int n, int stride,
                                                        CameraMount mnt, double *__restrict__ out_pos,
                                                        double *__restrict__ out_rot) {
  const int i = blockIdx.x * TS_WG + threadIdx.x;
  if (i >= n) return;
  const SogmPositionCommand &m = cmd[(size_t)i * stride];
  const double c = sogm_det::cos(m.yaw), s = sogm_det::sin(m.yaw);
  const double rz[3][3] = {{c, -s, 0.0}, {s, c, 0.0}, {0.0, 0.0, 1.0}};
  for (int r = 0; r < 3; ++r) {
    for (int j = 0; j < 3; ++j)
      out_rot[(size_t)i * 9 + r * 3 + j] =
          (rz[r][0] * mnt.cam2body[j] + rz[r][1] * mnt.cam2body[3 + j]) + rz[r][2] * mnt.cam2body[6 + j];
    out_pos[(size_t)i * 3 + r] = m.pos[r] + ((rz[r][0] * mnt.offset[0] + rz[r][1] * mnt.offset[1]) + rz[r][2] * mnt.offset[2]);
  }
}

int trajsrv_refuse(const char *entry, const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

int trajsrv_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_error_text("trajectory server: no HIP device");
    return SOGM_ERR_NO_DEVICE;
  }
  return SOGM_OK;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_traj_server_init(SogmTrajServerState *state, SogmTrajPoint *queue, int n, double t_trigger,
                                     const double *init_pos, const double *init_yaw, void *stream) {
  using namespace sogm;
  if (!state || !queue || !init_pos) return trajsrv_refuse("sogm_traj_server_init", "null pointer");
  if (n < 1) return trajsrv_refuse("sogm_traj_server_init", "n < 1");
  if (!std::isfinite(t_trigger)) return trajsrv_refuse("sogm_traj_server_init", "t_trigger is not finite");
  if (int rc = trajsrv_device()) return rc;
  hipLaunchKernelGGL(k_traj_server_init, dim3(n), dim3(TS_WG), 0, (hipStream_t)stream, state, queue, n, t_trigger, init_pos,
                     init_yaw);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

extern "C" int sogm_traj_server_run(const SogmTrajServerParams *prm, SogmTrajServerState *state, SogmTrajPoint *queue,
                                    const SogmTrajRecord *tables, const SogmTrajRecord *prev_table, const int32_t *received,
                                    int n_ticks, int n_total, int agent0, int n_local, double t0, int first_tick,
                                    double period, double receive_delay, SogmPositionCommand *out_cmd, void *stream) {
  using namespace sogm;
  const char *me = "sogm_traj_server_run";
  if (!prm || !state || !queue || !tables || !out_cmd) return trajsrv_refuse(me, "null pointer");
  if (n_ticks < 1 || n_ticks > 64) return trajsrv_refuse(me, "n_ticks out of range (1 .. 64)");
  if (n_total < 1 || first_tick < 0) return trajsrv_refuse(me, "n_total < 1 or first_tick < 0");
  if (agent0 < 0 || n_local < 1 || n_local > n_total - agent0) return trajsrv_refuse(me, "agent0 / n_local out of range");
  if (prm->yaw_mode != 0 && prm->yaw_mode != 1) return trajsrv_refuse(me, "yaw_mode is not 0 or 1");
  if (!(prm->sample_dt > 0) || !(period > 0) || !std::isfinite(prm->sample_dt) || !std::isfinite(period) ||
      !std::isfinite(t0) || !std::isfinite(prm->yaw_pi) || !std::isfinite(prm->yaw_dot_max))
    return trajsrv_refuse(me, "sample_dt and period must be positive, times and yaw constants finite");
  if (!(prm->replan_threshold > 0) || !(prm->replan_threshold / prm->sample_dt <= 127.0 + 1e-9))
    return trajsrv_refuse(me, "replan_threshold outside (0, 127 * sample_dt]");
  const double ratio = period / prm->sample_dt, m = std::nearbyint(ratio);
  if (!(std::fabs(ratio - m) <= 1e-9) || m < 1 || m > 4096)
    return trajsrv_refuse(me, "period / sample_dt is not a whole number (1 .. 4096)");
  if (!(receive_delay >= 0) || !(receive_delay < period)) return trajsrv_refuse(me, "receive_delay outside [0, period)");
  if (int rc = trajsrv_device()) return rc;
  TrajSrvDims d{};
  d.t0 = t0, d.period = period, d.receive_delay = receive_delay;
  d.first_tick = first_tick, d.m = (int)m, d.n_ticks = n_ticks, d.n_total = n_total, d.agent0 = agent0, d.n_local = n_local;
  hipLaunchKernelGGL(k_traj_server, dim3(n_local), dim3(TS_WG), 0, (hipStream_t)stream, *prm, d, state, queue, tables,
                     prev_table, received, out_cmd);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

extern "C" int sogm_camera_poses(const SogmPositionCommand *cmd, int n, int cmd_stride, const double *cam2body,
                                 const double *cam_offset, double *out_pos, double *out_rot, void *stream) {
  using namespace sogm;
  const char *me = "sogm_camera_poses";
  if (!cmd || !cam2body || !cam_offset || !out_pos || !out_rot) return trajsrv_refuse(me, "null pointer");
  if (n < 1 || cmd_stride < 1) return trajsrv_refuse(me, "n < 1 or cmd_stride < 1");
  CameraMount mnt;
  for (int k = 0; k < 9; ++k) mnt.cam2body[k] = cam2body[k];
  for (int k = 0; k < 3; ++k) mnt.offset[k] = cam_offset[k];
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(k < 9 ? mnt.cam2body[k] : mnt.offset[k - 9])) return trajsrv_refuse(me, "mount is not finite");
  if (int rc = trajsrv_device()) return rc;
  hipLaunchKernelGGL(k_camera_poses, dim3((n + TS_WG - 1) / TS_WG), dim3(TS_WG), 0, (hipStream_t)stream, cmd, n, cmd_stride,
                     mnt, out_pos, out_rot);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
