// Depth camera (include/sogm_abi.h "depth camera"): every agent's depth image and camera-frame cloud of a SogmWorld's
// cylinders (+ ground plane), rendered where sogm_gridmap_update and sogm_filter_point_cloud read them.  One launch:
//   k_render_depth  a workgroup of 256 lanes owns 256 groups of 8 consecutive pixels of one agent (a band of rows).  It
//                   first culls the world's cylinders against the camera's range — 256 per trip, one per lane, survivors
//                   compacted into an LDS list with 64-wide ballots; a list that would overflow is rendered and emptied
//                   first, so no cylinder is ever dropped — then every lane walks the list for its 8 pixels and keeps the
//                   smallest accepted t of each, and stores 16 B of depth and 6 x 16 B of cloud (scalar stores for row
//                   tails and for pieces that are not 16-byte aligned).
// k_render_depth<true> (SOGM_DEPTH_RINGS) also draws the valid type-2 records ("ring obstacles"): they take the same
// cull-and-compact trip into a second LDS list beside the cylinders' (both are rendered and emptied when either would
// overflow) and every lane runs sogm_ring.hpp's ring_ray_hit for its pixels.  k_render_depth<false> is the kernel without
// any of that.
// k_render_depth<., true> (sogm_render_depth_swarm) also draws the other vehicles ("agent bodies"): after the records, the
// bodies take the same trip, 256 per trip, into a third LDS list (all three are rendered and emptied when any would
// overflow), every lane runs sogm_body.hpp's body_ray_hit for its pixels, and each pixel carries the code of what gave its
// t so far: the smallest (t, code) pair, so that neither the order of the lists nor a flush decides a tie.  The
// <., false> forms carry none of that.
// The header's arithmetic is evaluated as written (fp64, -ffp-contract=off).  What is NOT evaluated is skipped only where
// the header's own expressions cannot yield an accepted t <= max_depth; each skip says why next to it.
#include "sogm_device.hpp"
#include "sogm_body.hpp"
#include "sogm_ring.hpp"

#include <cmath>
#include <cstdio>

namespace sogm {
namespace {

constexpr int DEPTH_WG  = 256;  // lanes per workgroup = cylinders culled per trip
constexpr int DEPTH_PX  = 8;    // consecutive pixels of a row per lane
constexpr int DEPTH_CAP = 256;  // candidates in LDS; >= DEPTH_WG so that one trip's survivors always fit an empty list

// what a pixel needs of one (camera, cylinder) pair: the header's ox, oy, c = (ox*ox + oy*oy) - r*r, r*r, z0, z1
struct DepthCand {
  double ox, oy, c, rr, z0, z1;
};

struct DepthArgs {
  SogmDepthCamera     cam;
  const SogmCylinder *cyl;
  const double       *pos, *rot;
  uint16_t           *depth;
  float              *cloud;
  int32_t            *unsupported;
  int                 n_cyl;
  int                 groups_per_row;    // ceil(cols / 8)
  int                 groups_per_agent;  // rows * groups_per_row
  int                 wgs_per_agent;     // ceil(groups_per_agent / 256)
};

// what only the BODIES forms take
struct BodyArgs {
  const double  *pos;       // [n_bodies * 3]
  const int32_t *cam_body;  // [n_agents] or null
  int32_t       *hit;       // [n_agents * rows * cols] or null
  double         size[3];
  double         half_norm;  // |half|
  int            n_bodies;
};
template <bool BODIES>
struct DepthArgsT : DepthArgs {};
template <>
struct DepthArgsT<true> : DepthArgs {
  BodyArgs b;
};

struct Ray {
  double d0, d1, d2, a;  // direction and a = d0*d0 + d1*d1
};

// LDS of the ring instantiation (the other one gets a single entry it never touches)
template <bool RINGS>
struct RingList {
  static constexpr int CAP = RINGS ? DEPTH_CAP : 1;
};

// LDS of the body instantiations: the third list and the record index of every entry of the other two
template <bool BODIES>
struct BodyList {
  static constexpr int CAP = BODIES ? DEPTH_CAP : 1;
};

constexpr int HIT_UNSET = 0x7FFFFFFF;  // above every code: the first accepted t of a pixel takes it over

__device__ inline void keep_min(double t, double &best) {
  if (t < best) best = t;
}

// the smallest (t, code) pair.  (A t of +inf may leave a code next to best = +inf: such a pixel has no return and its
// code is never read.)
__device__ inline void keep_min_code(double t, int code, double &best, int &best_code) {
  if (t < best || (t == best && code < best_code)) {
    best      = t;
    best_code = code;
  }
}

// one cylinder against one ray; t_reach = max_depth (1 + 1e-9)
__device__ inline void hit_cylinder(const DepthCand &q, const Ray &r, double pz, double t_reach, double &best) {
  if (r.a > 0) {
    const double b = q.ox * r.d0 + q.oy * r.d1;
    // Camera outside the cylinder (c > 0) and the ray's xy projection leaving the axis (b > 0): |q(t)|^2 - r^2 =
    // a t^2 + 2 b t + c > c for every t > 0, so no cap is hit (the margin on c covers the rounding of qx, qy: 1e-14 of
    // ox^2 + oy^2 = c + r^2), and a c >= 0 gives disc <= b b, s <= b, both roots <= 0: no side either.
    if (b > 1e-100 && q.c > 1e-9 * q.rr) return;
    const double disc = b * b - r.a * q.c;
    if (disc >= 0) {
      const double s = sqrt(disc);
      // (-b - s) / a <= (-b + s) / a (a > 0, s >= 0, division is monotone): the far root is needed only when the near one
      // is not accepted
      double t = (-b - s) / r.a;
      double z = pz + t * r.d2;
      if (!(t > 0 && q.z0 <= z && z <= q.z1)) {
        t = (-b + s) / r.a;
        z = pz + t * r.d2;
      }
      if (t > 0 && q.z0 <= z && z <= q.z1) keep_min(t, best);
    } else if (disc < -1e-9 * (b * b + r.a * (q.c + 2.0 * q.rr))) {
      // min over t of |q(t)|^2 - r^2 is -disc / a: with disc this far below zero (rounding is 1e-15 of the same terms) the
      // ray's xy projection stays outside the circle and no cap is hit
      return;
    }
  }
  if (r.d2 != 0) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const double num = (e ? q.z1 : q.z0) - pz;
      // num / d2 > 0 needs both of one sign (IEEE division gives the exact sign); beyond t_reach the quotient is above
      // max_depth and cannot be the image's t*
      if (num == 0 || (num > 0) != (r.d2 > 0) || fabs(num) > fabs(r.d2) * t_reach) continue;
      const double t  = num / r.d2;
      const double qx = q.ox + t * r.d0, qy = q.oy + t * r.d1;
      if (t > 0 && qx * qx + qy * qy <= q.rr) keep_min(t, best);
    }
  }
}

__device__ inline Ray make_ray(const double *R, double xc, double yc) {
  Ray r;
  r.d0 = (R[0] * xc + R[1] * yc) + R[2];
  r.d1 = (R[3] * xc + R[4] * yc) + R[5];
  r.d2 = (R[6] * xc + R[7] * yc) + R[8];
  r.a  = r.d0 * r.d0 + r.d1 * r.d1;
  return r;
}

template <bool RINGS, bool BODIES>
__global__ __launch_bounds__(DEPTH_WG) void k_render_depth(DepthArgsT<BODIES> g) {
  __shared__ DepthCand s_list[DEPTH_CAP];
  __shared__ RingCand  s_ring[RingList<RINGS>::CAP];
  __shared__ BodyCand  s_body[BodyList<BODIES>::CAP];
  __shared__ int       s_list_idx[BodyList<BODIES>::CAP];
  __shared__ int       s_ring_idx[BodyList<(BODIES && RINGS)>::CAP];
  __shared__ int       s_wave_n[DEPTH_WG / 64];
  __shared__ int       s_wave_r[DEPTH_WG / 64];
  __shared__ int       s_unsupported;

  const SogmDepthCamera &cam = g.cam;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int agent = blockIdx.x / g.wgs_per_agent, wg = blockIdx.x - agent * g.wgs_per_agent;
  const int grp   = wg * DEPTH_WG + tid;
  const bool live = grp < g.groups_per_agent;
  const int v = live ? grp / g.groups_per_row : 0, u0 = live ? (grp - v * g.groups_per_row) * DEPTH_PX : 0;
  const int npx = live ? min(DEPTH_PX, cam.cols - u0) : 0;

  double R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = g.rot[(size_t)agent * 9 + i];
  const double px = g.pos[(size_t)agent * 3], py = g.pos[(size_t)agent * 3 + 1], pz = g.pos[(size_t)agent * 3 + 2];
  const double yc = ((double)v - cam.cy) / cam.fy;
  const double t_reach = cam.max_depth * (1.0 + 1e-9);

  // How far from the camera, in xy, a point with t <= max_depth can be: t |d_xy|, and |d_xy|^2 is convex in (xc, yc), so
  // its maximum over the image is at a corner.  1e-6: rounding, and the caps' and t_reach's own margins.
  double reach;
  {
    const double x_lo = (0.0 - cam.cx) / cam.fx, x_hi = ((double)(cam.cols - 1) - cam.cx) / cam.fx;
    const double y_lo = (0.0 - cam.cy) / cam.fy, y_hi = ((double)(cam.rows - 1) - cam.cy) / cam.fy;
    const double a_max = fmax(fmax(make_ray(R, x_lo, y_lo).a, make_ray(R, x_hi, y_lo).a),
                              fmax(make_ray(R, x_lo, y_hi).a, make_ray(R, x_hi, y_hi).a));
    reach = cam.max_depth * sqrt(a_max) * (1.0 + 1e-6);
  }
  // The same in three dimensions, for the rings: a point with t <= max_depth is t |d| from the camera, and |d|^2 = a + d2^2
  // is convex in (xc, yc) as well.
  double reach3 = 0;
  if (RINGS || BODIES) {
    const double x_lo = (0.0 - cam.cx) / cam.fx, x_hi = ((double)(cam.cols - 1) - cam.cx) / cam.fx;
    const double y_lo = (0.0 - cam.cy) / cam.fy, y_hi = ((double)(cam.rows - 1) - cam.cy) / cam.fy;
    double       m = 0;
    for (int e = 0; e < 4; ++e) {
      const Ray r = make_ray(R, e & 1 ? x_hi : x_lo, e & 2 ? y_hi : y_lo);
      m           = fmax(m, r.a + r.d2 * r.d2);
    }
    reach3 = cam.max_depth * sqrt(m) * (1.0 + 1e-6);
  }

  double best[DEPTH_PX];
#pragma unroll
  for (int k = 0; k < DEPTH_PX; ++k) best[k] = INFINITY;
  int code[BODIES ? DEPTH_PX : 1];  // BODIES: what gave best[k]
  if constexpr (BODIES) {
#pragma unroll
    for (int k = 0; k < DEPTH_PX; ++k) code[k] = HIT_UNSET;
  }

  // every live lane: its pixels against the first n entries of the list
  auto render_list = [&](int n, int n_ring, int n_body) {
    if (n == 0 && n_ring == 0 && n_body == 0) return;
#pragma unroll
    for (int k = 0; k < DEPTH_PX; ++k) {
      if (k >= npx) continue;
      const Ray r = make_ray(R, ((double)(u0 + k) - cam.cx) / cam.fx, yc);
      double    t = best[k];
      if constexpr (!BODIES) {
        for (int j = 0; j < n; ++j) hit_cylinder(s_list[j], r, pz, t_reach, t);
        if (RINGS) {
          const double d[3] = {r.d0, r.d1, r.d2};
          for (int j = 0; j < n_ring; ++j) {
            // a hit that is not below the pixel's t so far, or beyond the camera's range, cannot change the image
            double th;
            if (ring_ray_hit(s_ring[j], d, fmin(t, t_reach), th)) keep_min(th, t);
          }
        }
      } else {
        int          c    = code[k];
        const double d[3] = {r.d0, r.d1, r.d2};
        for (int j = 0; j < n; ++j) {
          double tc = INFINITY;  // this cylinder's own smallest accepted t
          hit_cylinder(s_list[j], r, pz, t_reach, tc);
          keep_min_code(tc, s_list_idx[j], t, c);
        }
        if (RINGS) {
          for (int j = 0; j < n_ring; ++j) {
            // A ring's hit is >= the start t0 of its interval, and ring_ray_hit gives up when t0 >= t_stop.  A hit EQUAL
            // to the pixel's t so far can still change the code, so t_stop is the next double above t (t > 0: t + t 2^-52
            // rounds to more than t; +inf stays): what is given up is above t, or beyond the camera's range.
            double th;
            if (ring_ray_hit(s_ring[j], d, fmin(t * (1.0 + 0x1p-52), t_reach), th)) keep_min_code(th, s_ring_idx[j], t, c);
          }
        }
        for (int j = 0; j < n_body; ++j) {
          // the rule as written; its only skips are body_ray_hit's own (argued there)
          double tb;
          if (body_ray_hit(s_body[j], d, tb)) keep_min_code(tb, g.n_cyl + s_body[j].idx, t, c);
        }
        code[k] = c;
      }
      best[k] = t;
    }
  };

  if (tid == 0) s_unsupported = 0;
  int n_list = 0, n_ring = 0, n_body = 0, n_other = 0;
  for (int c0 = 0; c0 < g.n_cyl; c0 += DEPTH_WG) {
    const int i    = c0 + tid;
    bool      keep = false, keep_ring = false;
    DepthCand q{};
    RingCand  qr{};
    if (i < g.n_cyl) {
      const SogmCylinder &o = g.cyl[i];
      if (RINGS && o.type == 2) {
        RingFrame f;
        if (!ring_frame(o, f)) {
          ++n_other;  // not a ring: counted, not drawn
        } else {
          const double c[3] = {o.x, o.y, o.z}, p[3] = {px, py, pz};
          qr = ring_ray_prepare(f, c, p);
          // a hit point lies within R + rho of the centre (the bounding sphere the rule starts from) and within `reach3`
          // of the camera; 1e-6 as for the cylinders
          const double far = reach3 + (f.R + f.rho) * (1.0 + 1e-6);
          keep_ring        = qr.gamma <= far * far;
        }
      } else if (o.type != 3) {
        ++n_other;
      } else {
        const double r = 0.5 * o.w;
        q.z0 = o.z - 0.5 * o.h;
        q.z1 = o.z + 0.5 * o.h;
        q.ox = px - o.x;
        q.oy = py - o.y;
        const double oo = q.ox * q.ox + q.oy * q.oy;
        q.rr = r * r;
        q.c  = oo - q.rr;
        // a hit point lies within r of the axis (1e-6: the caps' rounded test) and within `reach` of the camera
        const double far = reach + fabs(r) * (1.0 + 1e-6);
        keep = oo <= far * far;
      }
    }
    const unsigned long long mask = __ballot(keep);
    const unsigned long long mask_r = RINGS ? __ballot(keep_ring) : 0ull;
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    if (RINGS && lane == 0) s_wave_r[wave] = __popcll(mask_r);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < DEPTH_WG / 64; ++w) {
      before += w < wave ? s_wave_n[w] : 0;
      total += s_wave_n[w];
    }
    int before_r = 0, total_r = 0;
    if (RINGS) {
#pragma unroll
      for (int w = 0; w < DEPTH_WG / 64; ++w) {
        before_r += w < wave ? s_wave_r[w] : 0;
        total_r += s_wave_r[w];
      }
    }
    // (uniform) render what is listed, start empty lists: a trip's survivors, total + total_r <= DEPTH_WG, fit either
    if (n_list + total > DEPTH_CAP || (RINGS && n_ring + total_r > DEPTH_CAP)) {
      render_list(n_list, n_ring, 0);
      n_list = n_ring = 0;
      __syncthreads();
    }
    if (keep) s_list[n_list + before + __popcll(mask & ((1ull << lane) - 1ull))] = q;
    if constexpr (BODIES) {
      if (keep) s_list_idx[n_list + before + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
    n_list += total;
    if (RINGS) {
      if (keep_ring) s_ring[n_ring + before_r + __popcll(mask_r & ((1ull << lane) - 1ull))] = qr;
      if constexpr (BODIES) {
        if (keep_ring) s_ring_idx[n_ring + before_r + __popcll(mask_r & ((1ull << lane) - 1ull))] = i;
      }
      n_ring += total_r;
    }
    __syncthreads();
  }
  if constexpr (BODIES) {
    // the bodies' trip: the same cull and compaction, into the third list (the counts of the waves reuse s_wave_n: the
    // last barrier of the records' loop lies behind every read of it)
    const BodyArgs &bd  = g.b;
    int             own = bd.cam_body ? bd.cam_body[agent] : agent;  // outside [0, n_bodies): matches no j
    for (int c0 = 0; c0 < bd.n_bodies; c0 += DEPTH_WG) {
      const int j    = c0 + tid;
      bool      keep = false;
      BodyCand  q{};
      if (j < bd.n_bodies && j != own) {
        const double c[3] = {bd.pos[(size_t)j * 3], bd.pos[(size_t)j * 3 + 1], bd.pos[(size_t)j * 3 + 2]};
        if (!body_valid(c)) {
          ++n_other;  // not a body: counted, not drawn
        } else {
          const double p[3] = {px, py, pz};
          q                 = body_prepare(c, bd.size, p, j);
          // a hit point lies within |half| of the centre and within `reach3` of the camera; 1e-6 as for the cylinders
          const double ex = c[0] - px, ey = c[1] - py, ez = c[2] - pz;
          const double far = reach3 + bd.half_norm * (1.0 + 1e-6);
          keep             = (ex * ex + ey * ey) + ez * ez <= far * far;
        }
      }
      const unsigned long long mask = __ballot(keep);
      if (lane == 0) s_wave_n[wave] = __popcll(mask);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < DEPTH_WG / 64; ++w) {
        before += w < wave ? s_wave_n[w] : 0;
        total += s_wave_n[w];
      }
      // (uniform) a trip's survivors, total <= DEPTH_WG, fit an empty list
      if (n_body + total > DEPTH_CAP) {
        render_list(n_list, n_ring, n_body);
        n_list = n_ring = n_body = 0;
        __syncthreads();
      }
      if (keep) s_body[n_body + before + __popcll(mask & ((1ull << lane) - 1ull))] = q;
      n_body += total;
      __syncthreads();
    }
  }
  render_list(n_list, n_ring, n_body);

  if (wg == 0) {  // one workgroup per agent reports the records of another type
    if (n_other) atomicAdd(&s_unsupported, n_other);
    __syncthreads();
    if (tid == 0) g.unsupported[agent] = s_unsupported;
  }
  if (!live) return;

  // ground, quantisation, back-projection
  uint16_t d16[DEPTH_PX];
  float    xyz[DEPTH_PX * 3];
  int      hit[BODIES ? DEPTH_PX : 1];
  const double gnum = cam.ground_z - pz;
#pragma unroll
  for (int k = 0; k < DEPTH_PX; ++k) {
    d16[k]         = 0;
    xyz[k * 3]     = xyz[k * 3 + 1] = xyz[k * 3 + 2] = __uint_as_float(0x7FC00000u);
    if constexpr (BODIES) hit[k] = SOGM_HIT_NONE;
    if (k >= npx) continue;
    const double du = (double)(u0 + k) - cam.cx;
    double       t  = best[k];
    if (cam.use_ground) {
      const double d2 = (R[6] * (du / cam.fx) + R[7] * yc) + R[8];
      // (gnum / d2 > 0 needs both of one sign)
      if (d2 != 0 && gnum != 0 && (gnum > 0) == (d2 > 0)) {
        const double tg = gnum / d2;
        if constexpr (BODIES) {
          if (tg > 0 && tg < t) {  // the ground wins only with a strictly smaller t
            t       = tg;
            code[k] = SOGM_HIT_GROUND;
          }
        } else {
          if (tg > 0) keep_min(tg, t);
        }
      }
    }
    if (t <= cam.max_depth) d16[k] = (uint16_t)floor(t * cam.depth_scale + 0.5);
    if constexpr (BODIES) {
      if (d16[k]) hit[k] = code[k];
    }
    if (d16[k]) {
      const double zq = (double)d16[k] / cam.depth_scale;
      xyz[k * 3]      = (float)(du * zq / cam.fx);
      xyz[k * 3 + 1]  = (float)(((double)v - cam.cy) * zq / cam.fy);
      xyz[k * 3 + 2]  = (float)zq;
    }
  }

  const size_t pix = ((size_t)agent * cam.rows + v) * (size_t)cam.cols + u0;
  uint16_t    *dp  = g.depth + pix;
  if (npx == DEPTH_PX && ((uintptr_t)dp & 15) == 0) {
    uint4 w;
    w.x = d16[0] | ((unsigned)d16[1] << 16);
    w.y = d16[2] | ((unsigned)d16[3] << 16);
    w.z = d16[4] | ((unsigned)d16[5] << 16);
    w.w = d16[6] | ((unsigned)d16[7] << 16);
    *reinterpret_cast<uint4 *>(dp) = w;
  } else {
#pragma unroll
    for (int k = 0; k < DEPTH_PX; ++k)
      if (k < npx) dp[k] = d16[k];
  }
  if (g.cloud) {
    float *cp = g.cloud + pix * 3;
    if (npx == DEPTH_PX && ((uintptr_t)cp & 15) == 0) {
#pragma unroll
      for (int k = 0; k < DEPTH_PX * 3; k += 4) {
        vfloat4 w = {xyz[k], xyz[k + 1], xyz[k + 2], xyz[k + 3]};
        *reinterpret_cast<vfloat4 *>(cp + k) = w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < DEPTH_PX * 3; ++k)
        if (k < npx * 3) cp[k] = xyz[k];
    }
  }
  if constexpr (BODIES) {
    if (g.b.hit) {
      int32_t *hp = g.b.hit + pix;
      if (npx == DEPTH_PX && ((uintptr_t)hp & 15) == 0) {
#pragma unroll
        for (int k = 0; k < DEPTH_PX; k += 4) {
          int4 w = {hit[k], hit[k + 1], hit[k + 2], hit[k + 3]};
          *reinterpret_cast<int4 *>(hp + k) = w;
        }
      } else {
#pragma unroll
        for (int k = 0; k < DEPTH_PX; ++k)
          if (k < npx) hp[k] = hit[k];
      }
    }
  }
}

int depth_refuse(const char *what, const char *entry = "sogm_render_depth") {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

// the refusals of both entries, then the launch geometry; SOGM_OK or the code to return
int depth_prepare(const char *entry, const SogmWorld *world, const SogmDepthCamera *cam, const SogmDepthBodies *bodies,
                  int n_agents, const double *cam_pos, const double *cam_rot, uint16_t *out_depth, float *out_cloud_xyz,
                  int32_t *out_unsupported, DepthArgs &g, long long &wgs) {
  if (!world || !cam || !cam_pos || !cam_rot || !out_depth || !out_unsupported) return depth_refuse("null pointer", entry);
  if (cam->rows < 1 || cam->cols < 1 || n_agents < 1) return depth_refuse("rows, cols and n_agents must be >= 1", entry);
  if (world->n_cyl < 0 || (world->n_cyl > 0 && !world->cylinders))
    return depth_refuse("n_cyl < 0, or null cylinders with n_cyl > 0", entry);
  if (!(cam->fx > 0) || !(cam->fy > 0) || !(cam->max_depth > 0) || !(cam->depth_scale > 0))
    return depth_refuse("fx, fy, max_depth and depth_scale must be positive", entry);
  if (!(cam->max_depth * cam->depth_scale <= 65535.0)) return depth_refuse("max_depth * depth_scale exceeds 65535", entry);
  if (!std::isfinite(cam->cx) || !std::isfinite(cam->cy) || !std::isfinite(cam->fx) || !std::isfinite(cam->fy) ||
      (cam->use_ground && !std::isfinite(cam->ground_z)))
    return depth_refuse("intrinsics and ground_z must be finite", entry);
  g                = DepthArgs{};
  g.cam            = *cam;
  g.groups_per_row = (cam->cols + DEPTH_PX - 1) / DEPTH_PX;
  const long long groups = (long long)cam->rows * g.groups_per_row;
  wgs                    = (groups + DEPTH_WG - 1) / DEPTH_WG;
  if ((long long)cam->rows * cam->cols > 2147483647LL || wgs * n_agents > 2147483647LL)
    return depth_refuse("image or batch too large for one launch", entry);
  if (bodies) {
    if (bodies->n_bodies < 0 || (bodies->n_bodies > 0 && !bodies->pos))
      return depth_refuse("n_bodies < 0, or null pos with n_bodies > 0", entry);
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(bodies->size[i]) || !(bodies->size[i] > 0)) return depth_refuse("size must be finite and positive", entry);
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    char buf[96];
    std::snprintf(buf, sizeof(buf), "%s: no HIP device", entry);
    set_error_text(buf);
    return SOGM_ERR_NO_DEVICE;
  }
  g.groups_per_agent = (int)groups;
  g.wgs_per_agent    = (int)wgs;
  g.cyl              = world->cylinders;
  g.n_cyl            = world->n_cyl;
  g.pos              = cam_pos;
  g.rot              = cam_rot;
  g.depth            = out_depth;
  g.cloud            = out_cloud_xyz;
  g.unsupported      = out_unsupported;
  return SOGM_OK;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_render_depth(const SogmWorld *world, const SogmDepthCamera *cam, int n_agents, const double *cam_pos,
                                 const double *cam_rot, uint16_t *out_depth, float *out_cloud_xyz,
                                 int32_t *out_unsupported, void *stream) {
  using namespace sogm;
  DepthArgsT<false> g{};
  long long         wgs = 0;
  const int rc = depth_prepare("sogm_render_depth", world, cam, nullptr, n_agents, cam_pos, cam_rot, out_depth, out_cloud_xyz,
                               out_unsupported, g, wgs);
  if (rc != SOGM_OK) return rc;
  if (cam->flags & SOGM_DEPTH_RINGS)
    hipLaunchKernelGGL((k_render_depth<true, false>), dim3((unsigned)(wgs * n_agents)), dim3(DEPTH_WG), 0, (hipStream_t)stream, g);
  else
    hipLaunchKernelGGL((k_render_depth<false, false>), dim3((unsigned)(wgs * n_agents)), dim3(DEPTH_WG), 0, (hipStream_t)stream, g);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

extern "C" int sogm_render_depth_swarm(const SogmWorld *world, const SogmDepthCamera *cam, const SogmDepthBodies *bodies,
                                       int n_agents, const double *cam_pos, const double *cam_rot, uint16_t *out_depth,
                                       float *out_cloud_xyz, int32_t *out_hit, int32_t *out_unsupported, void *stream) {
  using namespace sogm;
  DepthArgsT<true> g{};
  long long        wgs = 0;
  const int rc = depth_prepare("sogm_render_depth_swarm", world, cam, bodies, n_agents, cam_pos, cam_rot, out_depth,
                               out_cloud_xyz, out_unsupported, g, wgs);
  if (rc != SOGM_OK) return rc;
  g.b.hit = out_hit;
  for (int i = 0; i < 3; ++i) g.b.size[i] = 1.0;  // (no bodies: never read)
  if (bodies && bodies->n_bodies > 0) {
    g.b.pos      = bodies->pos;
    g.b.cam_body = bodies->cam_body;
    g.b.n_bodies = bodies->n_bodies;
    double hh    = 0;
    for (int i = 0; i < 3; ++i) {
      g.b.size[i] = bodies->size[i];
      hh += (0.5 * bodies->size[i]) * (0.5 * bodies->size[i]);
    }
    g.b.half_norm = std::sqrt(hh);
  }
  if (cam->flags & SOGM_DEPTH_RINGS)
    hipLaunchKernelGGL((k_render_depth<true, true>), dim3((unsigned)(wgs * n_agents)), dim3(DEPTH_WG), 0, (hipStream_t)stream, g);
  else
    hipLaunchKernelGGL((k_render_depth<false, true>), dim3((unsigned)(wgs * n_agents)), dim3(DEPTH_WG), 0, (hipStream_t)stream, g);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
