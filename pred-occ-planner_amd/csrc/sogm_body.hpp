// sogm_body.hpp — agent bodies in the depth camera (include/sogm_abi.h "agent bodies" is the definition), the rule written
// ONCE for the host and the device:
//   body_valid                     "not a body": a centre coordinate that is not finite
//   body_prepare / body_ray_hit    the ray p + t d against the axis-aligned box: three slabs, then tn, else tf
// k_render_depth<., true> of sogm_depth.hip calls these bodies; a host program compiles them as well
// (tests/body_rules_host_test.cpp).  Every expression is a single IEEE operation (+ - * /, comparisons): with
// -ffp-contract=off host and device give the same bits.
#pragma once

#include <cmath>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_BODY_HD __host__ __device__
#else
#define SOGM_BODY_HD
#endif

#include "../../include/sogm_abi.h"

namespace sogm {

// what a pixel needs of one (camera, body) pair: a_i = lo_i - p_i, b_i = hi_i - p_i and the body's index
struct BodyCand {
  double  a[3], b[3];
  int32_t idx, pad_;
};

SOGM_BODY_HD inline bool body_finite(double v) { return v - v == 0.0; }  // false for +-inf and NaN

SOGM_BODY_HD inline bool body_valid(const double *c) { return body_finite(c[0]) && body_finite(c[1]) && body_finite(c[2]); }

SOGM_BODY_HD inline BodyCand body_prepare(const double *c, const double *size, const double *p, int32_t idx) {
  BodyCand q;
  for (int i = 0; i < 3; ++i) {
    const double half = 0.5 * size[i];
    const double lo = c[i] - half, hi = c[i] + half;
    q.a[i] = lo - p[i];
    q.b[i] = hi - p[i];
  }
  q.idx  = idx;
  q.pad_ = 0;
  return q;
}

// The body's accepted t along p + t d, or false.
// The header's test for d_i == 0 is lo_i <= p_i && p_i <= hi_i; here it reads a_i <= 0 && 0 <= b_i.  They are the same
// decision: a rounded difference x - y has the sign of the exact one and is zero only when x == y (fp64 keeps subnormals),
// and a NaN or an inf - inf makes both forms false.
// The early return after an axis is not a shortcut of the rule's answer: once tn > tf (neither a NaN) a later axis either
// brings a NaN into tn or tf, and the rule's own "no hit unless tn <= tf" refuses, or leaves tn no smaller and tf no larger.
SOGM_BODY_HD inline bool body_ray_hit(const BodyCand &q, const double *d, double &t_hit) {
  double tn = -INFINITY, tf = INFINITY;
  for (int i = 0; i < 3; ++i) {
    if (d[i] == 0.0) {
      if (!(q.a[i] <= 0.0 && 0.0 <= q.b[i])) return false;
    } else {
      const double ta = q.a[i] / d[i], tb = q.b[i] / d[i];
      const double lo = ta < tb ? ta : tb, hi = ta > tb ? ta : tb;
      tn = tn > lo ? tn : lo;
      tf = tf < hi ? tf : hi;
      if (tn > tf) return false;
    }
  }
  if (!(tn <= tf)) return false;
  if (tn > 0.0) {
    t_hit = tn;
    return true;
  }
  if (tf > 0.0) {
    t_hit = tf;
    return true;
  }
  return false;
}

}  // namespace sogm
