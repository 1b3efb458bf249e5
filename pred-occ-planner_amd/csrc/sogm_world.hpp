// sogm_world.hpp — the moving world's timeline (include/sogm_abi.h "world timeline" is the definition), the rules written
// ONCE for the host and the device:
//   world_tick_time / world_still     t = (double)k * dt, and when a frame is tick 0's bit for bit
//   world_record_at                   a record's state at a tick
//   world_owned / world_offset / world_moved
//                                     whether a point moves with a record, the record's displacement rounded once to fp32,
//                                     the fp32 add
//   world_point_at                    a point's position at a tick, from the pieces above
// The kernel of sogm_world.hip calls these bodies (one coordinate at a time: its lanes hold four consecutive floats of the
// cloud, which straddle points); a host program compiles them as well (tests/world_frames_host_test.cpp).  Every
// expression is a single IEEE operation or a conversion: with -ffp-contract=off host and device give the same bits.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_WORLD_HD __host__ __device__
#else
#define SOGM_WORLD_HD
#endif

#include "../../include/sogm_abi.h"

namespace sogm {

static_assert(sizeof(SogmCylinder) == 96, "record layout");

SOGM_WORLD_HD inline double world_tick_time(int k, double dt) { return (double)k * dt; }

// the frame is the world of tick 0, copied: no add is performed (a -0.0f stays -0.0f)
SOGM_WORLD_HD inline bool world_still(int k, int moving) { return k == 0 || moving == 0; }

// a record's state at time t: x and y advance in fp64, every other field is copied
SOGM_WORLD_HD inline SogmCylinder world_record_at(const SogmCylinder &c0, bool still, double t) {
  SogmCylinder c;  // (field by field: the device keeps the record in registers)
  c.type = c0.type;
  c._pad = c0._pad;
  c.x    = still ? c0.x : c0.x + c0.vx * t;
  c.y    = still ? c0.y : c0.y + c0.vy * t;
  c.z = c0.z, c.w = c0.w, c.h = c0.h, c.vx = c0.vx, c.vy = c0.vy;
  c.qw = c0.qw, c.qx = c0.qx, c.qy = c0.qy, c.qz = c0.qz;
  return c;
}

// a point moves with record `owner` only if that record exists; nothing is read through any other owner
SOGM_WORLD_HD inline bool world_owned(int32_t owner, int n_cyl) { return owner >= 0 && owner < n_cyl; }

// a record's displacement along one axis: the product in fp64, rounded once
SOGM_WORLD_HD inline float world_offset(double v, double t) { return (float)(v * t); }

// the fp32 add, performed even when off is zero (-0.0f + 0.0f = +0.0f)
SOGM_WORLD_HD inline float world_moved(float x0, float off) { return x0 + off; }

// coordinate `comp` (0 x, 1 y, 2 z) of a point at time t
SOGM_WORLD_HD inline float world_coord_at(float v0, int comp, int32_t owner, const SogmCylinder *cyl0, int n_cyl, bool still,
                                          double t) {
  if (still || comp == 2 || !world_owned(owner, n_cyl)) return v0;
  return world_moved(v0, world_offset(comp == 0 ? cyl0[owner].vx : cyl0[owner].vy, t));
}

SOGM_WORLD_HD inline void world_point_at(const float *p0, int32_t owner, const SogmCylinder *cyl0, int n_cyl, bool still,
                                         double t, float *out) {
  for (int comp = 0; comp < 3; ++comp) out[comp] = world_coord_at(p0[comp], comp, owner, cyl0, n_cyl, still, t);
}

}  // namespace sogm
