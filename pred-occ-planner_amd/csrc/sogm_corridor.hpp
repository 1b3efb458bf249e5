// sogm_corridor.hpp — what a corridor segment slot is made of, device only: the LP-based corridor checks, the obstacle
// points of a segment, the FIRI segment body (its ellipsoid step is sogm_mvie.hpp, its LPs sogm_lp.hpp), the per-agent
// bookkeeping and the slot that strings them together.  Inlined by the corridor stage's kernels (sogm_corridor.hip) and
// by the flight's worker kernel (sogm_flight_light.hip); the build has no relocatable device code, so each of the two
// units carries its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../../include/sogm_detmath.h"
#include "sogm_lp.hpp"
#include "sogm_mvie.hpp"
#include "sogm_planner.hpp"

namespace sogm {
namespace {

__device__ inline double dot3(const double *a, const double *b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// checkCorridorValidity (baseline.cpp:191-204; poly rows h0 x + h1 y + h2 z + h3 <= 0) and
// checkGoalReachability (baseline.cpp:143-182), executed by the whole wave (linprog_wave)
__device__ bool corridorValidW(const double *polyA, int mA, const double *polyB, int mB, const LpScratch &sc) {
  const int    lane = threadIdx.x & 63;
  const double c[3] = {0, 0, 0};
  double       x[3];
  double      *A = sc.A(), *b = sc.b();
  for (int i = lane; i < mA + mB; i += 64) {
    const double *h = i < mA ? polyA + i * 4 : polyB + (i - mA) * 4;
    A[i * 3 + 0]    = h[0];
    A[i * 3 + 1]    = h[1];
    A[i * 3 + 2]    = h[2];
    b[i]            = -h[3];
  }
  wave_lds_sync();
  const double v = linprog_wave<3>(c, mA + mB, A, b, x, sc.work, sc.perm);
  wave_lds_sync();
  return !(v == INFINITY || v == -INFINITY);
}
__device__ bool goalReachableW(const double *poly, int m, const double *start, double *goal, const LpScratch &sc) {
  const int lane = threadIdx.x & 63;
  if (m <= 0) return true;
  double mx = -INFINITY;
  for (int i = 0; i < m; ++i) {
    const double *h = poly + i * 4;
    const double  v = dot3(h, goal) + h[3] * 1.0;
    mx              = v > mx ? v : mx;
  }
  if (mx <= 0) return true;
  double *A = sc.A(), *b = sc.b();
  for (int i = lane; i < m; i += 64) {
    const double *h = poly + i * 4;
    A[i * 3 + 0]    = h[0];
    A[i * 3 + 1]    = h[1];
    A[i * 3 + 2]    = h[2];
    b[i]            = -h[3];
  }
  wave_lds_sync();
  double c[3] = {-goal[0] + start[0], -goal[1] + start[1], -goal[2] + start[2]};
  double gmax[3], gmin[3];
  linprog_wave<3>(c, m, A, b, gmax, sc.work, sc.perm);
  wave_lds_sync();
  for (int j = 0; j < 3; ++j) c[j] = goal[j] - start[j];
  linprog_wave<3>(c, m, A, b, gmin, sc.work, sc.perm);
  wave_lds_sync();
  for (int j = 0; j < 3; ++j) goal[j] = 0.5 * (gmax[j] + gmin[j]);
  return false;
}

// wave arg-min of (value, index): smaller value wins, ties -> smaller index
__device__ inline void wave_argmin(double &v, int &idx) {
  for (int d = 32; d >= 1; d >>= 1) {
    const double ov = __shfl_xor(v, d, 64);
    const int    oi = __shfl_xor(idx, d, 64);
    if (ov < v || (ov == v && oi < idx)) {
      v   = ov;
      idx = oi;
    }
  }
}

// Local box of segment `seg` (baseline.cpp:300-324): box[0..2] = llc, box[3..5] = lhc, w[0..5] = the two waypoints
__device__ inline void segment_box(const SogmPlannerParams &pp, const double *sp, const double *rt, int seg,
                                   double *box, double *w) {
  double w0[3], w1[3];
  for (int k = 0; k < 3; ++k) {
    w0[k] = rt[seg * 6 + k];
    w1[k] = rt[(seg + 1) * 6 + k];
  }
  if (w0[2] < 0) w0[2] = 0.1;  // baseline.cpp:314
  if (w1[2] < 0) w1[2] = 0.1;
  double lower[3]  = {-4 + sp[0], -4 + sp[1], -1 + sp[2]};
  double higher[3] = {4 + sp[0], 4 + sp[1], 1 + sp[2]};
  if (lower[2] < 0) lower[2] = 0;
  if (higher[2] > 4) higher[2] = 4;
  for (int k = 0; k < 3; ++k) {
    const double mxw = w0[k] > w1[k] ? w0[k] : w1[k];
    const double mnw = w0[k] < w1[k] ? w0[k] : w1[k];
    const double hi  = mxw + pp.init_range;
    const double lo  = mnw - pp.init_range;
    box[3 + k]       = hi < higher[k] ? hi : higher[k];  // lhc
    box[k]           = lo > lower[k] ? lo : lower[k];    // llc
    w[k]             = w0[k];
    w[3 + k]         = w1[k];
  }
}

// ShrinkCorridor(hPoly, path) (baseline.cpp:206-213; baseline_fake.cpp:211-223 keeps the faces that look along the
// path or along z): whole wave, one face per lane; w = the segment's two waypoints, poly = its nf planes (LDS).  The
// caller synchronises the wave before it reads poly again.
__device__ inline void shrink_corridor(const SogmPlannerParams &pp, const double *w, double *poly, int nf) {
  const int    lane    = threadIdx.x & 63;
  const double path[3] = {w[3] - w[0], w[4] - w[1], w[5] - w[2]};
  for (int f = lane; f < nf; f += 64) {
    double      *h   = poly + f * 4;
    const double nrm = sogm_det::sqrt_rn(dot3(h, h));
    if (pp.fake_planner) {
      const double pn = sogm_det::sqrt_rn(dot3(path, path));
      if (dot3(h, path) / nrm / pn > 0.8) continue;
      if (dabs(h[2]) / nrm > 0.8) continue;
    }
    h[3] += nrm * pp.shrink_size;
  }
}

}  // namespace

// =================================================================================================
// Kernel P: obstacle points of one (segment, agent) — map.cpp:480-518 / risk_base.cpp:295-337.
// The only corridor stage that reads the SOGM: once it has run the grid may be cleared for the next update.
// Four waves; a lane takes four consecutive cells of the box scan per step (4 x slices loads in flight per lane,
// 1024 cells per workgroup step), and an order-preserving wave scan + cross-wave offsets keep the reference's
// point order (x fastest, then y, z; a cell's time slices in ascending order).
// =================================================================================================
// NW = waves of the calling workgroup (4: k_corridor_points; 1: the dataflow kernel, where the segment's own wave
// extracts its points).  Same cells, same order, same output for either.
template <int NW>
__device__ __forceinline__ void corridor_points_body(const MapView &m, const SogmPlannerParams &pp,
                                                     const CorridorWorkspace &ws, const CorridorIO &io, int agent,
                                                     int seg) {
  const int tid   = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl    = io.points(agent);
  const int slot  = agent * SOGM_MAX_PIECES + seg;
  if (seg >= rl - 1 || seg >= SOGM_MAX_PIECES) return;
  __shared__ double s_box[6], s_w[6];
  __shared__ int    s_wtot[4];
  const GridGeom &g    = m.g;
  const float    *pose = m.poses + agent * 3;
  const int       cap  = pp.pc_capacity;
  double         *pc   = ws.pc + (size_t)slot * cap * 3;
  if (tid == 0) segment_box(pp, io.start_pva + agent * 9, io.route + (size_t)agent * io.route_cap * 6, seg, s_box, s_w);
  __syncthreads();
  int N = 0;
  {
    const double stamp = m.stamps[agent];
    const double tr    = (double)g.dt;
    const double t1    = io.t_start[agent] + seg * pp.corridor_tau;
    const double t2    = io.t_start[agent] + (seg + 1) * pp.corridor_tau;
    int          js    = (int)floor((t1 - stamp) / tr);
    int          je    = (int)ceil((t2 - stamp) / tr);
    js                 = js < 0 ? 0 : js;
    js                 = js > g.T ? g.T : js;
    je                 = je > g.T ? g.T : je;
    je                 = je < 0 ? 0 : je;
    if (je > g.T - 1) je = g.T - 1;
    int lx = (int)((s_box[0] - pose[0] + g.rx) / g.res);
    int ly = (int)((s_box[1] - pose[1] + g.ry) / g.res);
    int lz = (int)((s_box[2] - pose[2] + g.rz) / g.res);
    int hx = (int)((s_box[3] - pose[0] + g.rx) / g.res);
    int hy = (int)((s_box[4] - pose[1] + g.ry) / g.res);
    int hz = (int)((s_box[5] - pose[2] + g.rz) / g.res);
    hx     = min(hx, g.L - 1);
    hy     = min(hy, g.W - 1);
    hz     = min(hz, g.H - 1);
    lx     = max(lx, 0);
    ly     = max(ly, 0);
    lz     = max(lz, 0);
    const int nx = hx - lx + 1, ny = hy - ly + 1, nz = hz - lz + 1;
    if (nx > 0 && ny > 0 && nz > 0 && js <= je) {
      const int   cells = nx * ny * nz;
      const void *grid0 = m.slab(agent, 0);
      int         base  = 0;
      for (int c0 = 0; c0 < cells; c0 += 256 * NW) {
        int      cnt[4], vi[4];
        unsigned mask[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = c0 + 4 * tid + q;
          cnt[q]      = 0;
          mask[q]     = 0;
          vi[q]       = 0;
          if (c < cells) {
            const int x = lx + c % nx;
            const int y = ly + (c / nx) % ny;
            const int z = lz + c / (nx * ny);
            vi[q]       = x + y * g.L + z * g.L * g.W;
            const int pi = g.phys(x, y, z);
            for (int j = js; j <= je; ++j) {
              const float thr = g.map_kind == SOGM_MAP_FAKE ? g.risk_threshold
                                                             : g.risk_threshold - g.decay_voxel * (float)j;
              if (cell_ld(grid0, (size_t)j * g.V + pi, g.half) > thr) {
                ++cnt[q];
                mask[q] |= 1u << (j - js);
              }
            }
          }
        }
        const int mine = cnt[0] + cnt[1] + cnt[2] + cnt[3];
        int       incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
          const int up = __shfl_up(incl, d, 64);
          if (lane >= d) incl += up;
        }
        if (lane == 63) s_wtot[wave] = incl;
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const int t = s_wtot[w];
          woff += w < wave ? t : 0;
          total += t;
        }
        __syncthreads();  // s_wtot is rewritten by the next step
        int off = base + woff + incl - mine;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (cnt[q]) {
            float fx, fy, fz;
            g.corner_of(vi[q], pose, fx, fy, fz);
            for (int j = 0; j < 32 && (mask[q] >> j); ++j)
              if ((mask[q] >> j) & 1u) {
                if (off < cap) {
                  pc[off * 3 + 0] = (double)fx;
                  pc[off * 3 + 1] = (double)fy;
                  pc[off * 3 + 2] = (double)fz;
                }
                ++off;
              }
          }
        base += total;
      }
      N = base;
    }
  }
  if (tid == 0) ws.seg_npts[slot] = N;
}

// =================================================================================================
// Kernel A: one workgroup per (segment, agent)
// =================================================================================================
// MB = capacity of the boundary block (6 in the replan path: getInitCorridor's box), DIRECT = the standalone
// firi::firi entry (sogm_firi_batched): bd / points / a / b / r come from the caller instead of the route and the
// map, and the polytope is returned as firi leaves it (no ShrinkCorridor, no validity LP).
struct FiriDirect {
  const double  *bd;        // [n][n_bd][4]
  int            n_bd;
  const double  *pc;        // packed xyz
  const int32_t *pc_range;  // [n][2]
  const double  *a, *b;     // [n][3]
  double        *r;         // [n][3] in / out
  int            iterations;
  double        *hpoly;     // [n][max_faces][4]
  int32_t       *nfaces;    // [n]
  int32_t       *status;    // [n] 1 ok, 0 a or b outside bd (firi returns false), -3 over capacity
  int            max_faces;
  int            first;     // problem index of slot 0 in this launch
  double         epsilon;
};

template <int MB, bool DIRECT>
__device__ __forceinline__ void corridor_segment_body(const MapView &m, const SogmPlannerParams &pp,
                                                      const CorridorWorkspace &ws, const CorridorIO &io, int agent,
                                                      int seg, char *smem, const FiriDirect &fd) {
  const int lane  = threadIdx.x;
  const int slot  = DIRECT ? agent : agent * SOGM_MAX_PIECES + seg;
  if constexpr (!DIRECT) {
    const int rl = io.points(agent);
    if (seg >= rl - 1 || seg >= SOGM_MAX_PIECES) {
      if (lane == 0) ws.seg_state[slot] = -2;  // no such segment
      return;
    }
  }
  using L = SegmentLds<MB>;
  double *base = (double *)smem, *s_fH = base + L::fH, *s_poly = base + L::poly, *s_small = base + L::small;
  // "point not yet covered" flags of the greedy selection: one BIT per obstacle point, 64 per word — the 64 lanes of
  // a trip of the point loops share one word, which lane 0 rewrites from a ballot (no atomics, 2 KiB for 16 k points)
  unsigned long long *s_fw  = (unsigned long long *)(base + L::flags);
  int                *s_int = (int *)(smem + L::ints(pp.pc_capacity));  // 16 ints
  const LpScratch     sc{base + LpLds::work, base + LpLds::rows, (int *)(smem + L::perm(pp.pc_capacity))};
  double *s_fwd = s_small + L::fwd, *s_fa = s_small + L::fa, *s_fb = s_small + L::fb, *s_p = s_small + L::p;
  double *s_fh = s_small + L::fh, *s_bd = s_small + L::bd, *s_fB = s_small + L::fB, *s_fD = s_small + L::fD;
  double *s_dD = s_small + L::dD, *s_box = s_small + L::box, *s_w = s_small + L::w;

  const double   *rt    = DIRECT ? nullptr : io.route + (size_t)agent * io.route_cap * 6;
  const double   *sp    = DIRECT ? nullptr : io.start_pva + agent * 9;
  const int       cap   = pp.pc_capacity;
  const int       prob  = DIRECT ? fd.first + slot : 0;
  const double   *pc    = DIRECT ? fd.pc + (size_t)fd.pc_range[prob * 2] * 3 : ws.pc + (size_t)slot * cap * 3;
  double         *fpc   = ws.fpc + (size_t)slot * cap * 3;
  double         *tang  = ws.tang + (size_t)slot * cap * 4;
  double         *distR = ws.distr + (size_t)slot * cap;

  long long *dbg = ws.seg_dbg + (size_t)slot * 16;
  const long long tk0 = wall_clock64();
  const int M = DIRECT ? fd.n_bd : 6;
  if (lane == 0) {
    for (int k = 0; k < 12; ++k) dbg[k] = 0;  // (12-15: the flight's own stamps of this slot, k_flight_light)
    if constexpr (DIRECT) {
      for (int i = 0; i < 4 * M; ++i) s_bd[i] = fd.bd[(size_t)prob * M * 4 + i];
      for (int k = 0; k < 3; ++k) {
        s_w[k]     = fd.a[prob * 3 + k];
        s_w[3 + k] = fd.b[prob * 3 + k];
      }
    } else {
      segment_box(pp, sp, rt, seg, s_box, s_w);
      // getInitCorridor (baseline.cpp:127-141) with the local box
      for (int i = 0; i < 24; ++i) s_bd[i] = 0;
      for (int k = 0; k < 3; ++k) {
        s_bd[k * 4 + k]       = 1.0;
        s_bd[(k + 3) * 4 + k] = -1.0;
        s_bd[k * 4 + 3]       = -s_box[3 + k];
        s_bd[(k + 3) * 4 + 3] = s_box[k];
      }
    }
  }
  __syncthreads();

  // obstacle points: written by k_corridor_points (the only stage of the corridor generation that reads the SOGM)
  int N = DIRECT ? fd.pc_range[prob * 2 + 1] - fd.pc_range[prob * 2] : ws.seg_npts[slot];
  int overflow = 0;
  if (N > cap) {
    N        = cap;
    overflow = 1;
  }
  __syncthreads();

  if (lane == 0) {
    dbg[0] = N;
    dbg[5] = wall_clock64() - tk0;
  }
  // ---------------- firi::firi (firi.hpp:238-365) ----------------
  const double epsilon = DIRECT ? fd.epsilon : 1.0e-6;
  int          nH      = 0;
  const int    n_iter  = DIRECT ? fd.iterations : pp.firi_iterations;
  bool         seed_ok = true;
  if (lane == 0) {
    int ok = 1;
    for (int i = 0; i < M; ++i) {
      const double *h = s_bd + i * 4;
      if (dot3(h, s_w) + h[3] > 0.0 || dot3(h, s_w + 3) + h[3] > 0.0) ok = 0;
    }
    s_int[0] = ok;
  }
  __syncthreads();
  seed_ok = s_int[0] != 0;

  if (seed_ok) {
    // lane-0 private ellipsoid state (R, p, r)
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    double p[3]    = {0.5 * (s_w[0] + s_w[3]), 0.5 * (s_w[1] + s_w[4]), 0.5 * (s_w[2] + s_w[5])};
    double r[3]    = {1, 1, 1};
    if constexpr (DIRECT)
      for (int k = 0; k < 3; ++k) r[k] = fd.r[prob * 3 + k];
    for (int loop = 0; loop < n_iter; ++loop) {
      if (lane == 0) {
        double forward[3][3], backward[3][3];
        for (int k = 0; k < 3; ++k)
          for (int j = 0; j < 3; ++j) {
            forward[k][j]    = (1.0 / r[k]) * R[j][k];
            backward[k][j]   = R[k][j] * r[j];
            s_fwd[k * 3 + j] = forward[k][j];
          }
        for (int i = 0; i < M; ++i) {
          const double *h = s_bd + i * 4;
          for (int j = 0; j < 3; ++j)
            s_fB[i * 3 + j] =
                (h[0] * backward[0][j] + h[1] * backward[1][j]) + h[2] * backward[2][j];
          s_fD[i] = h[3] + dot3(h, p);
        }
        const double da[3] = {s_w[0] - p[0], s_w[1] - p[1], s_w[2] - p[2]};
        const double db[3] = {s_w[3] - p[0], s_w[4] - p[1], s_w[5] - p[2]};
        for (int k = 0; k < 3; ++k) {
          s_fa[k] = dot3(forward[k], da);
          s_fb[k] = dot3(forward[k], db);
          s_p[k]  = p[k];
        }
        for (int i = 0; i < M; ++i) {
          const double *fb = s_fB + i * 3;
          s_dD[i]          = dabs(s_fD[i]) / sogm_det::sqrt_rn(dot3(fb, fb));
        }
      }
      __syncthreads();
      // per-point: ellipsoid frame, tangent plane with the a/b fix-ups (firi.hpp:274-305)
      double lmin = INFINITY;
      int    lidx = 0x7fffffff;
      {
        double fwd[9], fa[3], fb[3], pp3[3];
        for (int k = 0; k < 9; ++k) fwd[k] = s_fwd[k];
        for (int k = 0; k < 3; ++k) {
          fa[k]  = s_fa[k];
          fb[k]  = s_fb[k];
          pp3[k] = s_p[k];
        }
        for (int i = lane; i < N; i += 64) {
          const double d[3] = {pc[i * 3] - pp3[0], pc[i * 3 + 1] - pp3[1], pc[i * 3 + 2] - pp3[2]};
          double       q[3];
          for (int k = 0; k < 3; ++k) q[k] = dot3(fwd + k * 3, d);
          double t[4];
          double dr = sogm_det::sqrt_rn(dot3(q, q));
          t[3]      = -dr;
          for (int k = 0; k < 3; ++k) t[k] = q[k] / dr;
          if (dot3(t, fa) + t[3] > epsilon) {
            const double delta[3] = {q[0] - fa[0], q[1] - fa[1], q[2] - fa[2]};
            const double s        = dot3(delta, fa) / dot3(delta, delta);
            for (int k = 0; k < 3; ++k) t[k] = fa[k] - s * delta[k];
            dr   = sogm_det::sqrt_rn(dot3(t, t));
            t[3] = -dr;
            for (int k = 0; k < 3; ++k) t[k] /= dr;
          }
          if (dot3(t, fb) + t[3] > epsilon) {
            const double delta[3] = {q[0] - fb[0], q[1] - fb[1], q[2] - fb[2]};
            const double s        = dot3(delta, fb) / dot3(delta, delta);
            for (int k = 0; k < 3; ++k) t[k] = fb[k] - s * delta[k];
            dr   = sogm_det::sqrt_rn(dot3(t, t));
            t[3] = -dr;
            for (int k = 0; k < 3; ++k) t[k] /= dr;
          }
          if (dot3(t, fa) + t[3] > epsilon) {
            const double u[3] = {fa[0] - q[0], fa[1] - q[1], fa[2] - q[2]};
            const double v[3] = {fb[0] - q[0], fb[1] - q[1], fb[2] - q[2]};
            double       n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                                 u[0] * v[1] - u[1] * v[0]};
            const double nn   = sogm_det::sqrt_rn(dot3(n, n));
            if (nn > 0)
              for (int k = 0; k < 3; ++k) n[k] /= nn;
            for (int k = 0; k < 3; ++k) t[k] = n[k];
            t[3]            = -dot3(t, fa);
            const double sg = t[3] > 0.0 ? -1.0 : 1.0;
            for (int k = 0; k < 4; ++k) t[k] *= sg;
          }
          for (int k = 0; k < 3; ++k) fpc[i * 3 + k] = q[k];
          for (int k = 0; k < 4; ++k) tang[i * 4 + k] = t[k];
          distR[i]  = dr;
          {  // every point starts uncovered: the active lanes of this trip are exactly the points i < N of its word
            const unsigned long long act = __ballot(1);
            if (lane == 0) s_fw[i >> 6] = act;
          }
          if (dr < lmin) {
            lmin = dr;
            lidx = i;
          }
        }
      }
      wave_argmin(lmin, lidx);
      // greedy plane selection (firi.hpp:307-349)
      double minSqrR = lmin;
      int    pcMinId = lidx == 0x7fffffff ? 0 : lidx;
      double minSqrD = INFINITY;
      int    bdMinId = 0;
      unsigned bdFlags = M >= 32 ? 0xffffffffu : (1u << M) - 1u;
      for (int j = 0; j < M; ++j)
        if (s_dD[j] < minSqrD) {
          minSqrD = s_dD[j];
          bdMinId = j;
        }
      nH             = 0;
      bool completed = false;
      for (int i = 0; !completed && i < (M + N); ++i) {
        __syncthreads();
        if (lane == 0) {
          double *fh = s_fH + (nH < FIRI_MAX_H ? nH : FIRI_MAX_H - 1) * 4;
          if (minSqrD < minSqrR) {
            for (int k = 0; k < 3; ++k) fh[k] = s_fB[bdMinId * 3 + k];
            fh[3] = s_fD[bdMinId];
          } else {
            for (int k = 0; k < 4; ++k) fh[k] = tang[pcMinId * 4 + k];
            s_fw[pcMinId >> 6] &= ~(1ull << (pcMinId & 63));
          }
          for (int k = 0; k < 4; ++k) s_fh[k] = fh[k];
        }
        if (minSqrD < minSqrR) bdFlags &= ~(1u << bdMinId);  // uniform across lanes
        __syncthreads();
        completed = true;
        minSqrD   = INFINITY;
        for (int j = 0; j < M; ++j)
          if (bdFlags & (1u << j)) {
            completed = false;
            if (minSqrD > s_dD[j]) {
              bdMinId = j;
              minSqrD = s_dD[j];
            }
          }
        const double fh0 = s_fh[0], fh1 = s_fh[1], fh2 = s_fh[2], fh3 = s_fh[3];
        double       lm = INFINITY;
        int          li = 0x7fffffff;
        int          open = 0;
        for (int j = lane; j < N; j += 64) {
          const unsigned long long word = s_fw[j >> 6];  // uniform over the trip's lanes
          bool                     covered = false;
          if ((word >> lane) & 1ull) {
            const double *q = fpc + j * 3;
            if (((fh0 * q[0] + fh1 * q[1]) + fh2 * q[2]) + fh3 > -epsilon) {
              covered = true;
            } else {
              open = 1;
              if (lm > distR[j]) {
                lm = distR[j];
                li = j;
              }
            }
          }
          const unsigned long long clr = __ballot(covered);
          if (clr != 0ull && lane == 0) s_fw[j >> 6] = word & ~clr;
        }
        wave_argmin(lm, li);
        if (__any(open)) completed = false;
        minSqrR = lm;
        pcMinId = li == 0x7fffffff ? 0 : li;
        ++nH;
      }
      __syncthreads();
      if (nH > FIRI_MAX_H) {
        nH       = FIRI_MAX_H;
        overflow = 1;
      }
      // hPoly = forwardH * forward, offset back by p (firi.hpp:351-355)
      for (int i = lane; i < nH; i += 64) {
        const double *fh = s_fH + i * 4;
        double        h[4];
        for (int j = 0; j < 3; ++j)
          h[j] = (fh[0] * s_fwd[0 * 3 + j] + fh[1] * s_fwd[1 * 3 + j]) + fh[2] * s_fwd[2 * 3 + j];
        h[3] = fh[3] - dot3(h, s_p);
        for (int k = 0; k < 4; ++k) s_poly[i * 4 + k] = h[k];
      }
      __syncthreads();
      if (lane == 0) {
        dbg[1 + (loop > 0)] = nH;
        dbg[6 + 2 * (loop > 0)] = wall_clock64() - tk0;
      }
      if (loop == n_iter - 1) break;
      {
        const int       mm  = nH < LP_MAX_ROWS - 9 ? nH : LP_MAX_ROWS - 9;
        const long long tm0 = wall_clock64();
        maxVolInsEllipsoid(s_poly, mm, R, p, r, sc, base + L::lm, base + L::handoff, dbg);
        if (lane == 0) dbg[7] = wall_clock64() - tm0;
      }
      __syncthreads();
    }
    if constexpr (DIRECT)
      if (lane == 0)
        for (int k = 0; k < 3; ++k) fd.r[prob * 3 + k] = r[k];
  }

  if constexpr (DIRECT) {
    int nf = seed_ok ? nH : 0;
    if (nf > fd.max_faces) {
      nf       = fd.max_faces;
      overflow = 1;
    }
    double *out = fd.hpoly + (size_t)prob * fd.max_faces * 4;
    for (int i = lane; i < nf * 4; i += 64) out[i] = s_poly[i];
    if (lane == 0) {
      fd.nfaces[prob] = nf;
      fd.status[prob] = overflow ? -3 : (seed_ok ? 1 : 0);
    }
    return;
  }
  // ---------------- ShrinkCorridor + checkCorridorValidity ----------------
  int nf = seed_ok ? nH : 0;
  if (nf > pp.max_faces) {
    nf       = pp.max_faces;
    overflow = 1;
  }
  shrink_corridor(pp, s_w, s_poly, nf);
  wave_lds_sync();
  const bool valid = corridorValidW(s_poly, nf, nullptr, 0, sc);  // whole wave
  {
    double *out = ws.polys + (size_t)slot * pp.max_faces * 4;
    for (int i = lane; i < nf * 4; i += 64) out[i] = s_poly[i];
  }
  if (lane == 0) {
    ws.seg_nfaces[slot] = nf;
    ws.seg_state[slot]  = overflow ? -3 : (valid ? 1 : 0);
    ws.seg_npts[slot]   = N;
    dbg[10]             = wall_clock64() - tk0;
  }
}

// =================================================================================================
// Kernel B: per agent bookkeeping (baseline_fake.cpp:364-414 / baseline.cpp:362-403)
// =================================================================================================
// PAIRS (the dataflow replan, the flight, the parallel rules hook): pair_row is the agent's row of CorridorWorkspace::pair_ok
// or null — a verdict the segments' waves left there (corridor_pairs_eager) replaces the pair's LP; 0, or a null row, runs the
// LP in place — and stamps the agent's row of CorridorWorkspace::fin_dbg or null.  Without PAIRS (k_corridor_finalize,
// k_corridor_rules) neither exists in the code: these kernels compile to what they were.
template <bool PAIRS = false>
__device__ __forceinline__ void corridor_finalize_body(const SogmPlannerParams &pp, const CorridorWorkspace &ws,
                                                       const CorridorIO &io, int agent, const LpScratch &sc,
                                                       const int32_t *pair_row = nullptr, long long *stamps = nullptr) {
  // The sequential bookkeeping below is executed by all 64 lanes with identical data (uniform control flow);
  // the LPs inside are solved by the whole wave, outputs are written by lane 0 / copied lane-parallel.
  const bool    w0    = threadIdx.x == 0;
  const int     MF    = pp.max_faces;
  const double *polys = ws.polys + (size_t)agent * SOGM_MAX_PIECES * MF * 4;
  const int    *nfs   = ws.seg_nfaces + agent * SOGM_MAX_PIECES;
  const int    *state = ws.seg_state + agent * SOGM_MAX_PIECES;
  const double *rt    = io.route + (size_t)agent * io.route_cap * 6;
  const double *sp    = io.start_pva + agent * 9;
  const int     rl    = io.points(agent);
  int           npoly = 0;
  if constexpr (PAIRS)
    if (stamps && w0) stamps[0] = stamps[1] = stamps[2] = stamps[3] = wall_clock64();
  if (w0) {
    for (int i = 0; i < SOGM_MAX_PIECES; ++i) io.out_nfaces[agent * SOGM_MAX_PIECES + i] = 0;
    for (int i = 0; i < 6; ++i) io.out_goal[agent * 6 + i] = 0;
    io.out_npoly[agent] = 0;
  }
  if (!pp.fake_planner && rl < 2) return;
  if (rl < 1) return;
  // corridors are kept up to the first invalid one (the loop `break`s, baseline.cpp:355-358)
  for (int i = 0; i < rl - 1 && i < SOGM_MAX_PIECES; ++i) {
    if (state[i] != 1) {
      // a corridor that hit a capacity the reference does not have (pc_capacity points, 128 selected planes,
      // max_faces) counts as invalid: make that visible
      if (state[i] == -3 && w0 && ws.counters) atomicAdd(&ws.counters[SOGM_CNT_CORRIDOR_CAPACITY], 1ull);
      break;
    }
    ++npoly;
  }
  // (the route's full count: a route cut by its row AND by the 16 pieces is counted as before)
  if (npoly == SOGM_MAX_PIECES && io.route_len[agent] - 1 > SOGM_MAX_PIECES && w0 && ws.counters)
    atomicAdd(&ws.counters[SOGM_CNT_PIECES_CAPACITY], 1ull);  // route longer than 16 pieces: truncated
  if (npoly == 0) return;
  if constexpr (!PAIRS) {
    for (int i = 0; i + 1 < npoly; ++i) {
      if (!corridorValidW(polys + (size_t)i * MF * 4, nfs[i], polys + (size_t)(i + 1) * MF * 4,
                          nfs[i + 1], sc)) {
        if (i < 2) return;
        npoly = pp.fake_planner ? i + 1 : i;
        break;
      }
    }
  } else {
    // the same scan with the verdicts the segments' waves left: 1 / 2 replace the pair's LP, 0 (or no row) runs it here
    int n_late = 0, n_used = 0;
    for (int i = 0; i + 1 < npoly; ++i) {
      const int v = pair_row ? pair_row[i] : 0;
      ++(v ? n_used : n_late);
      if (v == 2 || (v == 0 && !corridorValidW(polys + (size_t)i * MF * 4, nfs[i], polys + (size_t)(i + 1) * MF * 4,
                                               nfs[i + 1], sc))) {
        npoly = i < 2 ? 0 : pp.fake_planner ? i + 1 : i;  // (i < 2: no corridors — the exit below takes it)
        break;
      }
    }
    if (w0) {
      if (pair_row && ws.pair_cnt && n_late) atomicAdd(&ws.pair_cnt[1], (unsigned long long)n_late);
      if (pair_row && ws.pair_cnt && n_used) atomicAdd(&ws.pair_cnt[2], (unsigned long long)n_used);
      if (stamps) stamps[1] = stamps[2] = stamps[3] = wall_clock64();
    }
  }
  if (pp.fake_planner ? npoly == 0 : npoly <= 1) return;
  double gpos[3], gvel[3];
  int    gi = npoly - 1;
  for (int k = 0; k < 3; ++k) {
    gpos[k] = rt[gi * 6 + k];
    gvel[k] = rt[gi * 6 + 3 + k];
  }
  bool do_scan = true;
  if (!pp.fake_planner)
    do_scan = !goalReachableW(polys + (size_t)(npoly - 1) * MF * 4, nfs[npoly - 1], sp, gpos, sc);
  if (do_scan) {
    for (int it = npoly - 1; it != 0; --it) {
      if (goalReachableW(polys + (size_t)it * MF * 4, nfs[it], sp, gpos, sc)) {
        npoly         = it + 1;
        const int idx = npoly - 1;
        for (int k = 0; k < 3; ++k) {
          gpos[k] = rt[idx * 6 + k];
          gvel[k] = rt[idx * 6 + 3 + k];
        }
        break;
      }
    }
  }
  if constexpr (PAIRS)
    if (stamps && w0) stamps[2] = stamps[3] = wall_clock64();
  for (int i = 0; i < npoly; ++i) {
    if (w0) io.out_nfaces[agent * SOGM_MAX_PIECES + i] = nfs[i];
    const double *src = polys + (size_t)i * MF * 4;
    double       *dst = io.out_polys + ((size_t)agent * SOGM_MAX_PIECES + i) * MF * 4;
    for (int k = threadIdx.x; k < nfs[i] * 4; k += 64) dst[k] = src[k];
  }
  if (w0) {
    for (int k = 0; k < 3; ++k) {
      io.out_goal[agent * 6 + k]     = gpos[k];
      io.out_goal[agent * 6 + 3 + k] = gvel[k];
    }
    io.out_npoly[agent] = npoly;
    if constexpr (PAIRS)
      if (stamps) stamps[3] = wall_clock64();
  }
}

// One segment slot of an agent, run by a one-wave workgroup of k_worker_flow or k_flight_light: its obstacle points, its
// polytope, its completion counted in seg_done[agent] and — if that made it the agent's last slot (`cumulative`: the counter
// runs on over the flight's ticks) — the per-agent bookkeeping, with the LP view laid over the segment layout's head
// (SegmentLds).  True if this wave finalised the agent: publishing it is the caller's.  stamps: the flight's (null: none).
//
// The adjacent-pair LPs of the bookkeeping, corridorValidW(poly_i, poly_i+1), depend on their two polytopes only, so the wave
// that finishes the LATER of two neighbouring segments solves the pair's LP at once, in its own LDS (free between two
// segments), instead of leaving all M - 1 of them to the finalising wave behind the agent's slowest segment.  Who is later is
// decided by one fetch-or on the agent's ready word: of two neighbours exactly one sees the other's bit, so every pair with two
// valid states is evaluated exactly once, and before either segment's completion is counted in seg_done — when the last
// ticket is drawn every verdict is visible.  The verdict is a pure function of the two polytopes (linprog_wave orders its
// rows by a fixed permutation of the row count and keeps no call history); the bookkeeping consumes the same booleans in
// the same order.  Nothing waits: no spin, no new row in the liveness table of DESIGN 3.1.
// SOGM_PAIRS_EAGER=0 (a profiling build) leaves every pair LP to the bookkeeping, for before / after stamps of one source.
#ifndef SOGM_PAIRS_EAGER
#define SOGM_PAIRS_EAGER 1
#endif
// called by the whole wave behind the fence that makes segment `seg` (a real one: seg < points - 1) visible
__device__ __forceinline__ void corridor_pairs_eager(const SogmPlannerParams &pp, const CorridorWorkspace &ws, int agent,
                                                     int seg, const LpScratch &sc) {
  unsigned old = 0;
  if (threadIdx.x == 0) old = __hip_atomic_fetch_or(&ws.seg_ready[agent], 1u << seg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = __builtin_amdgcn_readfirstlane(old);
  if (!(old & ((1u << seg) >> 1 | 2u << seg))) return;  // neither neighbour is done: the pairs are theirs
  __threadfence();  // the neighbours' polytopes, face counts and states (the fence the finalising wave takes behind its ticket)
  const int     MF    = pp.max_faces;
  const double *polys = ws.polys + (size_t)agent * SOGM_MAX_PIECES * MF * 4;
  const int    *nfs   = ws.seg_nfaces + agent * SOGM_MAX_PIECES;
  const int    *state = ws.seg_state + agent * SOGM_MAX_PIECES;
  if (state[seg] == 1) {
    for (int lo = seg - 1; lo <= seg; ++lo) {  // pair (lo, lo + 1): the lower segment is polyA, as in the bookkeeping
      const int other = lo == seg ? seg + 1 : lo;
      if (other < 0 || other >= SOGM_MAX_PIECES || !((old >> other) & 1u) || state[other] != 1) continue;
      const bool meet = corridorValidW(polys + (size_t)lo * MF * 4, nfs[lo], polys + (size_t)(lo + 1) * MF * 4, nfs[lo + 1], sc);
      if (threadIdx.x == 0) {
        ws.pair_ok[agent * SOGM_MAX_PIECES + lo] = meet ? 1 : 2;
        if (ws.pair_cnt) atomicAdd(&ws.pair_cnt[0], 1ull);
      }
    }
  }
  __threadfence();  // the verdicts are visible before this segment's completion is counted
}

// the slot's second half, behind the segment itself (k_corridor_rules_slots shares it): pairs, ticket, bookkeeping
__device__ __forceinline__ bool corridor_slot_done(const SogmPlannerParams &pp, const CorridorWorkspace &ws, const CorridorIO &io,
                                                   int agent, int seg, bool real, char *smem, int *seg_done, bool cumulative) {
  __threadfence();  // this segment's polytope is visible before its completion is counted
  const bool eager = SOGM_PAIRS_EAGER && ws.seg_ready;
  if (eager && real) corridor_pairs_eager(pp, ws, agent, seg, LpLds::carve(smem));
  const int done = flow_ticket(&seg_done[agent]);
  if ((cumulative ? done & (SOGM_MAX_PIECES - 1) : done) != SOGM_MAX_PIECES - 1) return false;
  __threadfence();  // the other segments' polytopes and verdicts (their completions were counted before ours)
  corridor_finalize_body<true>(pp, ws, io, agent, LpLds::carve(smem), eager ? ws.pair_ok + agent * SOGM_MAX_PIECES : nullptr,
                               ws.fin_dbg ? ws.fin_dbg + agent * 4 : nullptr);
  // Back to zero for the agent's next tick, in front of the caller's publication.  Every other slot of this agent has drawn
  // its seg_done ticket, which lies behind its fetch-or and its verdicts: nobody touches the word or the row any more.  In the
  // flight the agent's next tick reaches a segment only through this publication (q_ring -> QP -> finish -> map head -> map
  // -> search -> corridor descriptors), so its first fetch-or finds the zeroes.
  if (eager) {
    if (threadIdx.x < SOGM_MAX_PIECES) ws.pair_ok[agent * SOGM_MAX_PIECES + threadIdx.x] = 0;
    if (threadIdx.x == 0) ws.seg_ready[agent] = 0u;
  }
  __syncthreads();
  return true;
}
__device__ __forceinline__ bool corridor_slot(const MapView &m, const SogmPlannerParams &pp, const CorridorWorkspace &ws,
                                              const CorridorIO &io, int agent, int seg, char *smem, int *seg_done,
                                              bool cumulative, long long *stamps) {
  const bool real = seg < io.points(agent) - 1;
  if (real) {
    corridor_points_body<1>(m, pp, ws, io, agent, seg);
    __threadfence_block();
    __syncthreads();
  }
  if (stamps && threadIdx.x == 0) stamps[13] = wall_clock64();
  corridor_segment_body<6, false>(m, pp, ws, io, agent, seg, smem, FiriDirect{});
  __syncthreads();
  if (stamps && threadIdx.x == 0) stamps[14] = wall_clock64();
  return corridor_slot_done(pp, ws, io, agent, seg, real, smem, seg_done, cumulative);
}

}  // namespace sogm
