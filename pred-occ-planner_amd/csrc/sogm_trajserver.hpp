// sogm_trajserver.hpp — the reference's bezier_traj_server (traj_server/src/bezier_traj_server.cpp; getYaw at every push as
// bezier_traj_server_rotors.cpp:212-223 does), the rules of one agent's server written ONCE for the host and the device
// (include/sogm_abi.h "trajectory server" is the definition, with the deviations).  Line numbers are bezier_traj_server.cpp's.
//   the rules      trajsrv_receive_plan / trajsrv_push_time / trajsrv_receive_done (bezierCallback :283-355, resetTrajQueue
//                  :233-244, mergeTrajQueue :246-277), trajsrv_timer_plan (PubCallback :415-485, fillTrajQueue :211-228),
//                  trajsrv_get_yaw (getYaw :79-140), trajsrv_reserve / trajsrv_yaw_pass (pushToTrajQueue on a bounded ring)
//   the bodies     trajsrv_receive and trajsrv_timer: one callback each, serial, the evaluator a functor eval(rec, t, out9)
//                  with t RELATIVE to the record's start (a host caller brings its own reading of Bezier::getPos / Vel / Acc,
//                  clamped to [0, duration]).  The kernel of sogm_trajserver.hip calls the same rules, runs the evaluations
//                  they ask for one per lane and must give what these bodies give.
// Bookkeeping depends on times only: plain fp64 compares, single operations and the expressions the reference writes.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_TS_HD __host__ __device__
#else
#define SOGM_TS_HD
#endif

#include "../../include/sogm_abi.h"
#include "../../include/sogm_detmath.h"

namespace sogm {

constexpr int TRAJSRV_MASK = SOGM_TRAJSRV_QUEUE - 1;
static_assert((SOGM_TRAJSRV_QUEUE & TRAJSRV_MASK) == 0, "ring indices are masked");

// the scalar part of a server: what the rules read and write
using TrajSrvCore = SogmTrajServerCore;
static_assert(sizeof(TrajSrvCore) == 96 && sizeof(SogmTrajServerState) == 96 + sizeof(SogmTrajRecord), "state layout");
static_assert(sizeof(SogmTrajPoint) == 96 && sizeof(SogmPositionCommand) == 112, "sample / command layout");

enum : int32_t { TRAJSRV_RESET = 0, TRAJSRV_MERGE = 1, TRAJSRV_EARLY = 2 };
struct TrajSrvPlan {
  int32_t kind;    // which branch of bezierCallback
  int32_t n_push;  // samples it pushes (before the ring's bound)
  double  base;    // EARLY: now - tns, added to i * sample_dt
};
struct TrajSrvTimer {
  int32_t flags;      // SOGM_CMD_*
  int32_t src;        // ring slot of the published sample (flags & SOGM_CMD_PUBLISHED)
  int32_t push_slot;  // ring slot fillTrajQueue pushes to, -1: nothing is pushed
  double  t_sample;   // where: trajectory time t = tq - ts
};

// :293-299
SOGM_TS_HD inline double trajsrv_duration(const SogmTrajRecord &r) {
  double d = 0.0;
  for (int i = 0; i < r.n_pieces && i < SOGM_MAX_PIECES; ++i) d += r.duration[i];
  return d;
}

// bezierCallback's choice of branch and what it erases (:337-349 with the preamble behind it, :233-236, :246-264)
SOGM_TS_HD inline TrajSrvPlan trajsrv_receive_plan(const SogmTrajServerParams &prm, TrajSrvCore &c, double now, double tns) {
  TrajSrvPlan p{TRAJSRV_RESET, 0, 0.0};
  if (c.te <= tns) {  // the current trajectory is finished
    c.head = c.size = 0;
    for (double t = 0; t < prm.replan_threshold && p.n_push < SOGM_TRAJSRV_QUEUE; t += prm.sample_dt) ++p.n_push;
    return p;
  }
  const double q = (now + prm.replan_threshold - tns) / prm.sample_dt;
  const bool   fits = q > -2147483648.0 && q < 2147483648.0;
  const int    k    = fits ? (int)q : -1;
  if (k < 0 || k > c.size) {  // "Next traj starts earlier than current buffer!"
    p.kind = TRAJSRV_EARLY;
    p.base = now - tns;
    for (int i = 0; i < prm.replan_threshold / prm.sample_dt && i < SOGM_TRAJSRV_QUEUE; i++) ++p.n_push;
    return p;
  }
  p.kind = TRAJSRV_MERGE;
  c.size -= k;
  p.n_push = k;
  return p;
}

// trajectory time of the plan's push i
SOGM_TS_HD inline double trajsrv_push_time(const SogmTrajServerParams &prm, const TrajSrvPlan &p, int i) {
  if (p.kind == TRAJSRV_RESET) {  // t += DELTA_T, accumulated (:236)
    double t = 0;
    for (int n = 0; n < i && n < SOGM_TRAJSRV_QUEUE; ++n) t += prm.sample_dt;
    return t;
  }
  const double t = i * prm.sample_dt;
  return p.kind == TRAJSRV_EARLY ? t + p.base : t;  // :254, :269
}

// :351-354
SOGM_TS_HD inline void trajsrv_receive_done(TrajSrvCore &c, double tns, double duration) {
  c.duration = duration;
  c.ts       = tns;
  c.te       = c.ts + c.duration;
  c.traj_id += 1;
  c.received = 1;
}

// room for n pushes at the tail: how many are admitted (the rest are dropped: overflow) and the first one's slot
SOGM_TS_HD inline int trajsrv_reserve(TrajSrvCore &c, int n, int *first_slot) {
  const int room = SOGM_TRAJSRV_QUEUE - c.size, adm = n < room ? n : room;
  if (adm < n) c.overflow = 1;
  *first_slot = (c.head + c.size) & TRAJSRV_MASK;
  c.size += adm;
  return adm;
}

// pushToTrajQueue's sample (:194-205) before its yaw
SOGM_TS_HD inline void trajsrv_point(SogmTrajPoint &p, double t_abs, const double *pva) {
  p.t = t_abs;
  for (int d = 0; d < 3; ++d) {
    p.pos[d] = pva[d];
    p.vel[d] = pva[3 + d];
    p.acc[d] = pva[6 + d];
  }
  p.yaw = p.yaw_dot = 0.0;
}

// getYaw (:79-140)
SOGM_TS_HD inline void trajsrv_get_yaw(const SogmTrajServerParams &prm, TrajSrvCore &c, const double *v, double &yaw,
                                       double &yaw_dot) {
  const double PI = prm.yaw_pi, RATE = prm.yaw_dot_max, MAX_YAW_CHANGE = prm.yaw_dot_max * 0.01;
  yaw     = 0;
  yaw_dot = 0;
  // Eigen's normalized(): v / |v| when the squared norm is positive, v otherwise
  double       dir[3] = {v[0], v[1], v[2]};
  const double z      = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (z > 0) {
    const double n = sogm_det::sqrt_rn(z);
    for (int d = 0; d < 3; ++d) dir[d] = v[d] / n;
  }
  const double norm     = sogm_det::sqrt_rn((dir[0] * dir[0] + dir[1] * dir[1]) + dir[2] * dir[2]);
  const double yaw_temp = norm > 0.1 ? sogm_det::atan2(dir[1], dir[0]) : c.last_yaw;
  const double last     = c.last_yaw;
  if (yaw_temp - last > PI) {
    if (yaw_temp - last - 2 * PI < -MAX_YAW_CHANGE) {
      yaw = last - MAX_YAW_CHANGE;
      if (yaw < -PI) yaw += 2 * PI;
      yaw_dot = -RATE;
    } else {
      yaw = yaw_temp;
      if (yaw - last > PI)
        yaw_dot = -RATE;
      else
        yaw_dot = (yaw_temp - last) / 0.01;
    }
  } else if (yaw_temp - last < -PI) {
    if (yaw_temp - last + 2 * PI > MAX_YAW_CHANGE) {
      yaw = last + MAX_YAW_CHANGE;
      if (yaw > PI) yaw -= 2 * PI;
      yaw_dot = RATE;
    } else {
      yaw = yaw_temp;
      if (yaw - last < -PI)
        yaw_dot = RATE;
      else
        yaw_dot = (yaw_temp - last) / 0.01;
    }
  } else {
    if (yaw_temp - last < -MAX_YAW_CHANGE) {
      yaw = last - MAX_YAW_CHANGE;
      if (yaw < -PI) yaw += 2 * PI;
      yaw_dot = -RATE;
    } else if (yaw_temp - last > MAX_YAW_CHANGE) {
      yaw = last + MAX_YAW_CHANGE;
      if (yaw > PI) yaw -= 2 * PI;
      yaw_dot = RATE;
    } else {
      yaw = yaw_temp;
      if (yaw - last > PI)
        yaw_dot = -RATE;
      else if (yaw - last < -PI)
        yaw_dot = RATE;
      else
        yaw_dot = (yaw_temp - last) / 0.01;
    }
  }
  if (sogm_det::fabs_(yaw - last) <= MAX_YAW_CHANGE) yaw = 0.5 * last + 0.5 * yaw;  // "nieve LPF"
  yaw_dot       = 0.5 * c.last_yawdot + 0.5 * yaw_dot;
  c.last_yaw    = yaw;
  c.last_yawdot = yaw_dot;
}

// yaw_mode 1: getYaw over the n samples just pushed at slots first, first + 1, ... in that order.  `write` says whether this
// caller stores the result (every lane of the kernel's wave runs the recurrence, one of them stores).
SOGM_TS_HD inline void trajsrv_yaw_pass(const SogmTrajServerParams &prm, TrajSrvCore &c, SogmTrajPoint *ring, int first,
                                        int n, bool write) {
  if (prm.yaw_mode != 1) return;
  for (int i = 0; i < n && i < SOGM_TRAJSRV_QUEUE; ++i) {
    SogmTrajPoint &p = ring[(first + i) & TRAJSRV_MASK];
    const double   v[3] = {p.vel[0], p.vel[1], p.vel[2]};
    double         yaw, yaw_dot;
    trajsrv_get_yaw(prm, c, v, yaw, yaw_dot);
    if (write) {
      p.yaw     = yaw;
      p.yaw_dot = yaw_dot;
    }
  }
}

// PubCallback's bookkeeping at `now` (:452-473) with fillTrajQueue's (:211-221): pops, and says what is published and pushed
SOGM_TS_HD inline TrajSrvTimer trajsrv_timer_plan(const SogmTrajServerParams &prm, TrajSrvCore &c, double now) {
  TrajSrvTimer tp{0, -1, -1, 0.0};
  if (!c.received || c.size == 0) return tp;
  tp.src = c.head & TRAJSRV_MASK;
  if (c.size == 1) {
    tp.flags = SOGM_CMD_PUBLISHED | SOGM_CMD_HELD;
    return tp;
  }
  tp.flags = SOGM_CMD_PUBLISHED;
  c.head   = (c.head + 1) & TRAJSRV_MASK;
  c.size -= 1;
  const double tq = now + prm.replan_threshold;
  if (tq < c.ts) return tp;  // "Invalid start time, too late!"
  const double t = tq - c.ts;
  if (t > c.duration) return tp;
  tp.t_sample = t;
  (void)trajsrv_reserve(c, 1, &tp.push_slot);  // (a sample was popped: there is room)
  return tp;
}

// publishCmd's message (:163-187) from the sample the timer chose
SOGM_TS_HD inline void trajsrv_command(SogmPositionCommand &cmd, const TrajSrvCore &c, const TrajSrvTimer &tp,
                                       const SogmTrajPoint &p, double now) {
  const bool pub = (tp.flags & SOGM_CMD_PUBLISHED) != 0, held = (tp.flags & SOGM_CMD_HELD) != 0;
  cmd.t_pub    = now;
  cmd.t_sample = pub ? p.t : 0.0;
  for (int d = 0; d < 3; ++d) {
    cmd.pos[d] = pub ? p.pos[d] : c.init_pos[d];
    cmd.vel[d] = pub && !held ? p.vel[d] : 0.0;
    cmd.acc[d] = pub && !held ? p.acc[d] : 0.0;
  }
  cmd.yaw     = !pub ? 0.0 : (held ? c.last_yaw : p.yaw);
  cmd.yaw_dot = pub && !held ? p.yaw_dot : 0.0;
  cmd.traj_id = pub ? c.traj_id : 0;
  cmd.flags   = tp.flags;
}

// ---- the serial bodies ----

// bezierCallback: `rec` (n_pieces > 0) arrives at `now`
template <class Eval>
inline void trajsrv_receive(const SogmTrajServerParams &prm, SogmTrajServerState &s, SogmTrajPoint *ring,
                            const SogmTrajRecord &rec, double now, Eval eval) {
  TrajSrvCore      &c   = s.core;
  const double      tns = rec.time_start, duration = trajsrv_duration(rec);
  const TrajSrvPlan p   = trajsrv_receive_plan(prm, c, now, tns);
  int               first;
  const int         adm = trajsrv_reserve(c, p.n_push, &first);
  for (int i = 0; i < adm; ++i) {
    const double t = trajsrv_push_time(prm, p, i);
    double       o[9];
    eval(rec, t, o);
    trajsrv_point(ring[(first + i) & TRAJSRV_MASK], c.ts + t, o);
  }
  trajsrv_yaw_pass(prm, c, ring, first, adm, true);
  s.traj = rec;
  trajsrv_receive_done(c, tns, duration);
}

// PubCallback at `now`
template <class Eval>
inline void trajsrv_timer(const SogmTrajServerParams &prm, SogmTrajServerState &s, SogmTrajPoint *ring, double now,
                          Eval eval, SogmPositionCommand &cmd) {
  TrajSrvCore       &c  = s.core;
  const TrajSrvTimer tp = trajsrv_timer_plan(prm, c, now);
  SogmTrajPoint      p{};
  if (tp.flags & SOGM_CMD_PUBLISHED) p = ring[tp.src];  // before the push: a full ring pushes into the popped slot
  if (tp.push_slot >= 0) {
    double o[9];
    eval(s.traj, tp.t_sample, o);
    trajsrv_point(ring[tp.push_slot], c.ts + tp.t_sample, o);
    trajsrv_yaw_pass(prm, c, ring, tp.push_slot, 1, true);
  }
  trajsrv_command(cmd, c, tp, p, now);
}

}  // namespace sogm
