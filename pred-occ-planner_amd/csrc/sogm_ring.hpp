// sogm_ring.hpp — ring obstacles (include/sogm_abi.h "ring obstacles" is the definition), the rules written ONCE for the
// host and the device:
//   ring_frame                      validity, R, rho and the three columns e1, e2, n of the normalised quaternion's matrix
//   ring_ray_prepare / ring_ray_hit the depth camera's ray against the solid torus: bounding-sphere chord, slab, t >= 0,
//                                   then 32 nodes and 48 bisection steps on the quartic
//   ring_arc_mid / ring_table_fill  the 64 unit vectors made by arc halving
//   ring_box_gap                    the flight audit's distance from the ring's circle to the body box, minus rho
// The kernels of sogm_depth.hip and sogm_audit.hip call these bodies; a host program compiles them as well
// (tests/ring_rules_host_test.cpp).  Every expression is a single IEEE operation (+ - * / sqrt, comparisons): with
// -ffp-contract=off host and device give the same bits.
#pragma once

#include <cmath>
#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_RING_HD __host__ __device__
#else
#define SOGM_RING_HD
#endif

#include "../../include/sogm_abi.h"

namespace sogm {

constexpr int RING_TABLE   = 64;  // unit vectors of the table
constexpr int RING_NODES   = 32;  // sub-intervals of the ray search
constexpr int RING_BISECT  = 48;  // bisection steps of the ray search
constexpr int RING_HALVING = 12;  // halving steps of the box gap

struct RingFrame {
  double R, rho;                   // major radius 0.5 * w, tube radius h
  double e1[3], e2[3], n[3];       // columns 0, 1, 2 of the matrix of q / |q|: the circle lies in span(e1, e2)
};

SOGM_RING_HD inline bool ring_finite(double v) { return v - v == 0.0; }  // false for +-inf and NaN

// "not a ring" (false) or the ring's frame
SOGM_RING_HD inline bool ring_frame(const SogmCylinder &c, RingFrame &f) {
  if (!(ring_finite(c.x) && ring_finite(c.y) && ring_finite(c.z) && ring_finite(c.w) && ring_finite(c.h) &&
        ring_finite(c.vx) && ring_finite(c.vy) && ring_finite(c.qw) && ring_finite(c.qx) && ring_finite(c.qy) &&
        ring_finite(c.qz)))
    return false;
  f.R   = 0.5 * c.w;
  f.rho = c.h;
  if (!(f.R > 0.0) || !(f.rho > 0.0) || !(f.rho < f.R)) return false;
  const double qn = sqrt(((c.qw * c.qw + c.qx * c.qx) + c.qy * c.qy) + c.qz * c.qz);
  if (!(qn > 0.0) || !ring_finite(qn)) return false;
  const double w = c.qw / qn, x = c.qx / qn, y = c.qy / qn, z = c.qz / qn;
  f.e1[0] = 1.0 - 2.0 * (y * y + z * z);
  f.e1[1] = 2.0 * (x * y + w * z);
  f.e1[2] = 2.0 * (x * z - w * y);
  f.e2[0] = 2.0 * (x * y - w * z);
  f.e2[1] = 1.0 - 2.0 * (x * x + z * z);
  f.e2[2] = 2.0 * (y * z + w * x);
  f.n[0]  = 2.0 * (x * z + w * y);
  f.n[1]  = 2.0 * (y * z - w * x);
  f.n[2]  = 1.0 - 2.0 * (x * x + y * y);
  return true;
}

SOGM_RING_HD inline double ring_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ---- ray against ring ----------------------------------------------------------------------------------------------
// what a pixel needs of one (camera, ring) pair: o = p - c, the normal, R, rho, and the two products without d
struct RingCand {
  double o[3], n[3], R, rho, gamma, no;
};

SOGM_RING_HD inline RingCand ring_ray_prepare(const RingFrame &f, const double *c, const double *p) {
  RingCand q;
  for (int i = 0; i < 3; ++i) {
    q.o[i] = p[i] - c[i];
    q.n[i] = f.n[i];
  }
  q.R     = f.R;
  q.rho   = f.rho;
  q.gamma = ring_dot(q.o, q.o);
  q.no    = ring_dot(q.n, q.o);
  return q;
}

struct RingQuartic {
  double c4, c3, c2, c1, c0;
};

SOGM_RING_HD inline double ring_f(const RingQuartic &k, double t) {
  return (((k.c4 * t + k.c3) * t + k.c2) * t + k.c1) * t + k.c0;
}

// The ring's hit along p + t d, or false.  t_stop: a caller that only wants hits below t_stop (the pixel's best so far,
// the camera's range) gets false as soon as the interval's start shows that the hit cannot be below it; pass +inf for the
// definition's own answer.
SOGM_RING_HD inline bool ring_ray_hit(const RingCand &q, const double *d, double t_stop, double &t_hit) {
  const double alpha = ring_dot(d, d);
  if (!(alpha > 0.0)) return false;
  const double beta = ring_dot(q.o, d);
  // bounding sphere of radius R + rho
  const double S    = q.R + q.rho;
  const double cs   = q.gamma - S * S;
  const double disc = beta * beta - alpha * cs;
  if (disc < 0.0) return false;
  const double s  = sqrt(disc);
  double       t0 = (-beta - s) / alpha;
  double       t1 = (-beta + s) / alpha;
  // slab |no + t nd| <= rho
  const double nd = ring_dot(q.n, d);
  if (nd == 0.0) {
    if (!(fabs(q.no) <= q.rho)) return false;
  } else {
    const double ta = (-q.rho - q.no) / nd, tb = (q.rho - q.no) / nd;
    const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
    if (lo > t0) t0 = lo;
    if (hi < t1) t1 = hi;
  }
  if (t0 < 0.0) t0 = 0.0;
  if (!(t0 <= t1)) return false;
  if (!(t0 < t_stop)) return false;  // (not part of the definition: every hit is >= t0)
  const double RR   = q.R * q.R;
  const double K    = (q.gamma + RR) - q.rho * q.rho;
  const double nd2  = nd * nd;
  const double nond = q.no * nd;
  const double no2  = q.no * q.no;
  RingQuartic  k;
  k.c4 = alpha * alpha;
  k.c3 = (4.0 * alpha) * beta;
  k.c2 = ((4.0 * beta) * beta + (2.0 * alpha) * K) - (4.0 * RR) * (alpha - nd2);
  k.c1 = (4.0 * beta) * K - (8.0 * RR) * (beta - nond);
  k.c0 = K * K - (4.0 * RR) * (q.gamma - no2);
  if (ring_f(k, t0) <= 0.0) {
    if (t0 == 0.0) return false;  // the camera is inside the tube: no return from this ring
    t_hit = t0;
    return true;
  }
  const double h  = (t1 - t0) / (double)RING_NODES;
  double       lo = t0;
  for (int i = 1; i <= RING_NODES; ++i) {
    const double node = i == RING_NODES ? t1 : t0 + (double)i * h;
    if (ring_f(k, node) <= 0.0) {
      double hi = node;
      for (int b = 0; b < RING_BISECT; ++b) {
        const double m = 0.5 * (lo + hi);
        if (ring_f(k, m) <= 0.0)
          hi = m;
        else
          lo = m;
      }
      t_hit = hi;
      return true;
    }
    lo = node;
  }
  return false;
}

// ---- body box against ring -------------------------------------------------------------------------------------------
// the unit vector half way along the arc from a to b (neighbours: never antipodal)
SOGM_RING_HD inline void ring_arc_mid(const double *a, const double *b, double *out) {
  const double sx = a[0] + b[0], sy = a[1] + b[1];
  const double nn = sqrt(sx * sx + sy * sy);
  out[0] = sx / nn;
  out[1] = sy / nn;
}

// entry i of the table needs entries i - step and i + step (mod 64), step = the lowest set bit of i; multiples of 16 are
// the four axes.  ring_table_level(tab, i, step) fills entry i once the entries of the coarser levels are there.
SOGM_RING_HD inline void ring_table_axis(double (*tab)[2], int i) {
  const int k = i / 16;
  tab[i][0] = k == 0 ? 1.0 : (k == 2 ? -1.0 : 0.0);
  tab[i][1] = k == 1 ? 1.0 : (k == 3 ? -1.0 : 0.0);
}
SOGM_RING_HD inline void ring_table_level(double (*tab)[2], int i, int step) {
  ring_arc_mid(tab[(i - step) & (RING_TABLE - 1)], tab[(i + step) & (RING_TABLE - 1)], tab[i]);
}
SOGM_RING_HD inline void ring_table_fill(double (*tab)[2]) {
  for (int i = 0; i < RING_TABLE; i += 16) ring_table_axis(tab, i);
  for (int step = 8; step >= 1; step >>= 1)
    for (int i = step; i < RING_TABLE; i += 2 * step) ring_table_level(tab, i, step);
}

// what a (sample, agent) pair needs of one ring: the centre at the sample's time, R, rho, e1, e2
struct RingBody {
  double c[3], R, rho, e1[3], e2[3];
};

// g(u): distance of the circle point c + R (u0 e1 + u1 e2) to the box [lo, hi]
SOGM_RING_HD inline double ring_point_gap(const RingBody &r, const double *lo, const double *hi, const double *u) {
  double dd[3];
  for (int i = 0; i < 3; ++i) {
    const double P = r.c[i] + r.R * (u[0] * r.e1[i] + u[1] * r.e2[i]);
    const double q = P < lo[i] ? lo[i] : (P > hi[i] ? hi[i] : P);
    dd[i]          = P - q;
  }
  return sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]);
}

// gap = g(m) - rho after the vertex search and twelve halving steps; a = the body's centre, body = its size
SOGM_RING_HD inline double ring_box_gap(const RingBody &r, const double *a, const double *body, const double (*tab)[2]) {
  double lo[3], hi[3];
  for (int i = 0; i < 3; ++i) {
    const double hb = 0.5 * body[i];
    lo[i] = a[i] - hb;
    hi[i] = a[i] + hb;
  }
  int    best = 0;
  double gm   = ring_point_gap(r, lo, hi, tab[0]);
  for (int k = 1; k < RING_TABLE; ++k) {
    const double g = ring_point_gap(r, lo, hi, tab[k]);
    if (g < gm) {
      gm   = g;
      best = k;
    }
  }
  const int il = (best + RING_TABLE - 1) & (RING_TABLE - 1), ir = (best + 1) & (RING_TABLE - 1);
  double    ul[2] = {tab[il][0], tab[il][1]}, um[2] = {tab[best][0], tab[best][1]}, ur[2] = {tab[ir][0], tab[ir][1]};
  for (int s = 0; s < RING_HALVING; ++s) {
    double ml[2], mr[2];
    ring_arc_mid(ul, um, ml);
    ring_arc_mid(um, ur, mr);
    const double gl = ring_point_gap(r, lo, hi, ml), gr = ring_point_gap(r, lo, hi, mr);
    if (gl < gm && gl <= gr) {
      ur[0] = um[0], ur[1] = um[1];
      um[0] = ml[0], um[1] = ml[1];
      gm    = gl;
    } else if (gr < gm) {
      ul[0] = um[0], ul[1] = um[1];
      um[0] = mr[0], um[1] = mr[1];
      gm    = gr;
    } else {
      ul[0] = ml[0], ul[1] = ml[1];
      ur[0] = mr[0], ur[1] = mr[1];
    }
  }
  return gm - r.rho;
}

}  // namespace sogm
