// sogm_map.hip — building an agent's SOGM on gfx950 (MI355X), behind include/sogm_abi.h.  (The library's root is
// sogm_context.hip, the readers of a finished map sogm_query.hip, the record kernels sogm_traj.hip, the kernels that zero a
// grid, the mark logs and the pool of grids sogm_clear.hip.)
//
// An agent's map is built by one of four builders out of the same steps, each step written once as a ticket body:
//   cull_ticket      candidate cylinders around the map centre + the agent's crop of a SogmWorld cloud.
//   bits_ticket      per cloud point: crop, voxel index, one atomic OR into the occupancy bitmask of slice 0.
//                                                               fake_particle_risk_voxel.cpp:88-114
//   marks_ticket     per occupied voxel: slice-0 mark, GT velocity of the first matching record, T - 1 advected marks,
//                    mark log.                                  fake_particle_risk_voxel.cpp:114-170
//   overlay_ticket   per (record, slice): Bezier sample (fp64) + body particles, float atomic add, mark log.
//                                                               risk_base.cpp:136-168,199-208
// (all HBM-bound integer / fp32 work — no MFMA anywhere on this path).  The builders:
//   the lock-step kernels   k_cull_cylinders, k_stamp_bits / _blocks, k_stamp_marks / _cached, k_splat_neighbours: one launch
//                           per step over the whole swarm (sogm_update_gt / _gt_swarm / _world, sogm_project_neighbours)
//   k_update_flow           one persistent launch, agent by agent (tuning key update_flow)
//   k_prestamp_flow         the NEXT tick's map inside this tick's dataflow replan (sogm_update_prestamped adopts it)
//   k_flight_map            the map role of sogm_flight_run
// Behind them the host side: map_target / world_blocks, the lock-step update as named steps, the update entries.
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "sogm_device.hpp"
#include "sogm_fsm.hpp"
#include "sogm_planner.hpp"  // FlowCtl: the pre-stamp consumes the dataflow replan's list of finished agents

namespace sogm {

// ------------------------------------------------------------------------------------------------
// stamp: cloud -> slice 0, GT velocity -> slices 1..T-1
// ------------------------------------------------------------------------------------------------
#define SOGM_MAX_CYL_LDS 1024

// Ring obstacle test (fake_particle_risk_voxel.cpp:137-149): the voxel corner pt lies within 2 voxels of the
// ring's plane and of its circle of diameter w.  Eigen's operation sequence in fp32 (as oracle/map_oracle.cpp):
// q * v = _transformVector (uv = q.vec x v; uv += uv; v + w uv + q.vec x uv), Hyperplane::Through(p0, p1, p2)
// (normal = (p2 - p0) x (p1 - p0), normalised; offset = -p0.normal), projection, absDistance.
__device__ inline void cross3f(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline void quat_rotate_f(float qw, const float qv[3], const float v[3], float o[3]) {
  float uv[3], w2[3];
  cross3f(qv, v, uv);
  for (int k = 0; k < 3; ++k) uv[k] += uv[k];
  cross3f(qv, uv, w2);
  for (int k = 0; k < 3; ++k) o[k] = (v[k] + qw * uv[k]) + w2[k];
}
__device__ __noinline__ bool ring_contains(const SogmCylinder &cy, float px, float py, float pz, float res) {
  const float qw = (float)cy.qw, qv[3] = {(float)cy.qx, (float)cy.qy, (float)cy.qz};
  const float c0[3] = {(float)cy.x, (float)cy.y, (float)cy.z};
  const float ey[3] = {0, 1, 0}, ex[3] = {1, 0, 0};
  float       ry[3], rx[3], v0[3], v1[3], n[3];
  quat_rotate_f(qw, qv, ey, ry);
  quat_rotate_f(qw, qv, ex, rx);
  for (int k = 0; k < 3; ++k) {
    const float p1 = c0[k] + ry[k], p2 = c0[k] + rx[k];
    v0[k] = p2 - c0[k];
    v1[k] = p1 - c0[k];
  }
  cross3f(v0, v1, n);
  const float nn = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  for (int k = 0; k < 3; ++k) n[k] /= nn;
  const float off = -((c0[0] * n[0] + c0[1] * n[1]) + c0[2] * n[2]);
  const float sd  = ((n[0] * px + n[1] * py) + n[2] * pz) + off;
  const float b0 = px - sd * n[0], b1 = py - sd * n[1], b2 = pz - sd * n[2];
  const float e0 = c0[0] - b0, e1 = c0[1] - b1, e2 = c0[2] - b2;
  const float dist = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
  return fabs(cy.w / 2 - (double)dist) < (double)(2 * res) && fabsf(sd) < 2 * res;
}

// Candidate cylinders of an agent: those that can touch its window, in their original order (the reference takes
// the FIRST record containing the voxel, :127-154).  A voxel corner lies inside the window, so a record further than
// range + res + reach from the map centre along x or y can never match; culling keeps the per-point loop independent
// of the size of the global obstacle field (tens of candidates instead of thousands).  One wave per agent, no LDS.
struct CylCand {
  float  x, y, vx, vy;
  double wlim;  // w + clearance (fp64, as the reference compares)
  int    type, orig;
};
static_assert(sizeof(CylCand) == 32, "CylCand is copied in 16-byte pieces");
// candidates a pre-stamp wave keeps in LDS (16 KiB; the bench scene keeps ~280 of its 555 cylinders per agent, the rest
// of a longer list is read from global memory as before)
constexpr int PRESTAMP_CAND_LDS = 512;
// (The kernel also files the update's poses and stamps into the context's arrays — the later kernels of the update
//  and the queries read those —, which saves two copy nodes in front of it.)
__device__ __forceinline__ void cull_agent(const GridGeom &g, const SogmCylinder *__restrict__ cyl, int n_cyl,
                                           float q0, float q1, CylCand *__restrict__ out, int *__restrict__ n_out,
                                           int lane) {
  int kept = 0;
  for (int c0 = 0; c0 < n_cyl; c0 += 64) {
    const int c    = c0 + lane;
    bool      keep = false;
    double    wl   = 0.0;
    if (c < n_cyl) {
      wl = cyl[c].w + (double)g.clearance;
      // reach of a record around its centre: a cylinder matches within w + clearance; a ring (type 2) within
      // w/2 + 2 res of its axis point and 2 res of its plane, i.e. at most w/2 + 4 res from the centre
      const double reach = cyl[c].type == 2 ? 0.5 * cyl[c].w + 4.0 * (double)g.res : wl;
      const double lim_x = (double)g.rx + (double)g.res + reach + 0.5, lim_y = (double)g.ry + (double)g.res + reach + 0.5;
      keep = fabs((double)(float)cyl[c].x - (double)q0) <= lim_x && fabs((double)(float)cyl[c].y - (double)q1) <= lim_y;
    }
    const unsigned long long m   = __ballot(keep);
    const int                off = kept + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && off < SOGM_MAX_CYL_LDS)
      out[off] = CylCand{(float)cyl[c].x, (float)cyl[c].y, (float)cyl[c].vx, (float)cyl[c].vy, wl, cyl[c].type, c};
    kept += __popcll(m);
  }
  if (lane == 0) *n_out = kept;  // > SOGM_MAX_CYL_LDS: the stamp falls back to the full list
}
__device__ __forceinline__ void cull_blocks_agent(const GridGeom &g, const CloudBlocks &cb, int agent, float q0, float q1,
                                                  int lane);
// ---- The ticket bodies.  An agent's map is built by four builders — the lock-step kernels below, k_update_flow,
// k_prestamp_flow and k_flight_map — out of the same steps: cull, bits, marks, overlay.  Each step is written once, takes the
// map stage's structs (sogm_planner.hpp) and is the one place that unpacks them into the `__restrict__` parameters of the
// loops; every builder that runs the step calls its body, which is why all four mark the same cells.
// Cull (one wave): the agent's candidate cylinders around the map centre (q0, q1) and its crop of a SogmWorld cloud.
__device__ __forceinline__ void cull_ticket(const GridGeom &g, const MapFrame &f, const MapTarget &t, int agent, float q0,
                                            float q1, int lane) {
  cull_agent(g, f.cyl, f.n_cyl, q0, q1, (CylCand *)t.cand + (size_t)agent * SOGM_MAX_CYL_LDS, t.n_cand + agent, lane);
  if (f.cb.bounds) cull_blocks_agent(g, f.cb, agent, q0, q1, lane);
}
__global__ __launch_bounds__(64) void k_cull_cylinders(GridGeom g, const SogmCylinder *__restrict__ cyl, int n_cyl,
                                                       const float *__restrict__ poses, CylCand *__restrict__ cand,
                                                       int *__restrict__ n_cand, const double *__restrict__ stamps_in,
                                                       float *__restrict__ poses_out, double *__restrict__ stamps_out,
                                                       CloudBlocks cb, long long *__restrict__ tick_clock) {
  const MapFrame  f{.cb = cb, .cyl = cyl, .n_cyl = n_cyl};
  const MapTarget t{.cand = cand, .n_cand = n_cand};
  const int       agent = blockIdx.x, lane = threadIdx.x;
  if (tick_clock && agent == 0 && lane == 0) tick_clock[0] = wall_clock64();  // the update's first kernel is running
  const float  q0 = poses[agent * 3], q1 = poses[agent * 3 + 1];
  if (lane < 3) poses_out[agent * 3 + lane] = poses[agent * 3 + lane];
  if (lane == 3) stamps_out[agent] = stamps_in[agent];
  cull_ticket(g, f, t, agent, q0, q1, lane);
}

// The stamp in two passes (one-wave workgroups, no LDS; the candidates come from k_cull_cylinders through L1 / the
// scalar cache).  The cloud arrives z-fastest (an obstacle generator walks x, y, z), i.e. consecutive points are a
// whole z-layer apart in the grid, and the T - 1 future marks of a voxel sit a slice (V cells) apart: stamped point
// by point, every 4-byte mark dirtied a sector of its own (rocprof WRITE_SIZE 8.8 x the marked bytes, r02).  Now
//   k_stamp_bits   per (agent, cloud point): crop, voxel index, ONE fire-and-forget atomic OR into the agent's
//                  occupancy bitmask of slice 0 (V bits: on-chip traffic; duplicates — the 0.10 m cloud lattice is
//                  finer than the 0.15 m voxels — cost nothing more);
//   k_stamp_marks  per (agent, 64 mask words): lanes take the set bits of a non-zero word — 32 x-consecutive
//                  voxels — so the slice-0 mark and the T - 1 future marks of neighbouring voxels leave the wave as
//                  stores to neighbouring addresses of one slice (a few 64-byte lines per instruction instead of one
//                  line per mark); the velocity lookup runs once per occupied voxel as before; consumed words are
//                  zeroed for the next update.
// The set of marked cells is the one the per-point form produced (marks are idempotent, the lookup depends on the
// voxel only).
// one cloud point of the bits pass: PassThrough limits (fake_particle_risk_voxel.cpp:88-104, fp32), voxel index, one OR
struct CropBox {
  float lox, hix, loy, hiy, loz, hiz, p0, p1, p2;
  __device__ __forceinline__ CropBox(const GridGeom &g, float q0, float q1, float q2)
      : lox(q0 - g.rx), hix(q0 + g.rx), loy(q1 - g.ry), hiy(q1 + g.ry), loz(q2 - g.rz), hiz(q2 + g.rz), p0(q0), p1(q1), p2(q2) {}
};
// the bit a cloud point sets (the slice's storage order), -1 if the point sets none
__device__ __forceinline__ int stamp_bit_of(const GridGeom &g, const CropBox &b, float px, float py, float pz) {
  if (!(px >= b.lox && px <= b.hix && py >= b.loy && py <= b.hiy && pz >= b.loz && pz <= b.hiz)) return -1;
  const float x = px - b.p0, y = py - b.p1, z = pz - b.p2;
  if (!g.in_range(x, y, z)) return -1;
  const int v = g.voxel_of(x, y, z);
  if (v >= g.V) return -1;  // (the reference's out-of-array index, see stamp_bits_point)
  return g.phys_of(v);
}
__device__ __forceinline__ void stamp_bits_point(const GridGeom &g, const CropBox &b, float px, float py, float pz,
                                                 unsigned *__restrict__ mask) {
  if (!(px >= b.lox && px <= b.hix && py >= b.loy && py <= b.hiy && pz >= b.loz && pz <= b.hiz)) return;
  const float x = px - b.p0, y = py - b.p1, z = pz - b.p2;
  if (!g.in_range(x, y, z)) return;
  const int v = g.voxel_of(x, y, z);
  // Reference UB (map.h:169-174): a coordinate one ulp below +range rounds up to range in "x + r" and to the full
  // count in the fp32 division, so the index component equals the axis size; for z (or y on the top layer) the
  // voxel index is >= V and the reference writes outside risk_maps_.  Such marks are dropped, here and in the
  // oracle (x / y overflows inside the array wrap into the next row / layer exactly as the reference's do).
  if (v >= g.V) return;
  const int p = g.phys_of(v);  // the mask is kept in the slice's storage order: neighbouring bits share a sector
  __hip_atomic_fetch_or(mask + (p >> 5), 1u << (p & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// points first, first + stride, ... of [begin, end) (lane included in `first`)
__device__ __forceinline__ void stamp_bits_range(const GridGeom &g, const float *__restrict__ cloud, int first, int end,
                                                 int stride, float p0, float p1, float p2, unsigned *__restrict__ mask) {
  const CropBox box(g, p0, p1, p2);
  // four points per trip: their twelve loads are in flight together (one point per trip was a dependent HBM / L2 round
  // trip each, ~2.3 us per point and lane inside the tick; the marks are idempotent ORs, their order is free)
  int i = first;
  for (; (long long)i + 3ll * stride < end; i += 4 * stride) {
    float px[4], py[4], pz[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t q = (size_t)(i + u * stride) * 3;
      px[u] = cloud[q];
      py[u] = cloud[q + 1];
      pz[u] = cloud[q + 2];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) stamp_bits_point(g, box, px[u], py[u], pz[u], mask);
  }
  for (; i < end; i += stride) stamp_bits_point(g, box, cloud[(size_t)i * 3], cloud[(size_t)i * 3 + 1], cloud[(size_t)i * 3 + 2], mask);
}

// ---- the crop of updateMap on the device (SogmWorld): the cloud comes in blocks of `block_points` consecutive points
// with their xy bounds (sogm_cloud_block_bounds); an agent's crop is the ascending list of the blocks whose bounds
// intersect its window, built once per agent-update by one wave (cull_blocks_agent), and the bits pass walks that list.
// The PassThrough test per point is unchanged, so the set of marked voxels is the one a scan of the whole cloud gives.
__device__ __forceinline__ void cull_blocks_agent(const GridGeom &g, const CloudBlocks &cb, int agent, float q0, float q1,
                                                  int lane) {
  const float lox = q0 - g.rx, hix = q0 + g.rx, loy = q1 - g.ry, hiy = q1 + g.ry;
  int        *out = cb.list + (size_t)agent * cb.row;
  int         kept = 0;
  for (int b0 = 0; b0 < cb.n_blocks; b0 += 64) {
    const int b    = b0 + lane;
    bool      keep = false;
    if (b < cb.n_blocks) {
      const float4 bb = reinterpret_cast<const float4 *>(cb.bounds)[b];  // {xmin, xmax, ymin, ymax}
      keep            = !(bb.y < lox || bb.x > hix || bb.w < loy || bb.z > hiy);
    }
    const unsigned long long m = __ballot(keep);
    if (keep) out[kept + __popcll(m & ((1ull << lane) - 1ull))] = b;
    kept += __popcll(m);
  }
  if (lane == 0) cb.n_list[agent] = kept;
}
// 64 points of a wave: ONE atomic OR per distinct mask word.  The ORs are device-scope atomics that execute at the memory
// side — their count is what the bits pass costs (a predecessor-lane de-duplication alone: 448 -> 318 us per tick) — and
// the points of a block are neighbours (consecutive along z, 0.10 m apart in 0.15 m voxels, columns side by side), so a
// wave's 64 points fall into a handful of words (a word = four 2 x 2 x 2 tiles along x).  Leader loop: the first lane
// still to do names its word, the lanes with that word OR their bits together, the leader issues the atomic.
__device__ __forceinline__ void stamp_bits_wave(const GridGeom &g, const CropBox &box, float px, float py, float pz,
                                                unsigned *__restrict__ mask, int lane) {
  const int          p   = stamp_bit_of(g, box, px, py, pz);
  const int          w   = p >= 0 ? p >> 5 : -1;
  const unsigned     bit = p >= 0 ? 1u << (p & 31) : 0u;
  unsigned long long todo = __ballot(p >= 0);
  while (todo) {  // uniform
    const int                leader = __builtin_ctzll(todo);
    const int                wv     = __shfl(w, leader, 64);
    const bool               mine   = w == wv;
    const unsigned long long m      = __ballot(mine);
    unsigned                 b      = mine ? bit : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) b |= (unsigned)__shfl_xor((int)b, d, 64);
    if (lane == leader) __hip_atomic_fetch_or(mask + wv, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    todo &= ~m;
  }
}
// ... and for the 256 points a wave has in flight (four per lane): the columns of a block lie side by side, 0.10 m apart,
// so their bits share words across the four sets as well
// (called by ALL 64 lanes — the wave OR reads lane 63 —; `valid` bit u = the lane's point u exists)
__device__ __forceinline__ void stamp_bits_wave4(const GridGeom &g, const CropBox &box, const float (&px)[4],
                                                 const float (&py)[4], const float (&pz)[4], unsigned *__restrict__ mask,
                                                 int lane, unsigned valid) {
  int                w[4];
  unsigned           bit[4];
  unsigned long long todo[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int p = ((valid >> u) & 1u) ? stamp_bit_of(g, box, px[u], py[u], pz[u]) : -1;
    w[u]        = p >= 0 ? p >> 5 : -1;
    bit[u]      = p >= 0 ? 1u << (p & 31) : 0u;
    todo[u]     = __ballot(p >= 0);
  }
  for (;;) {  // uniform
    int wv;
    if (todo[0]) wv = __shfl(w[0], __builtin_ctzll(todo[0]), 64);
    else if (todo[1]) wv = __shfl(w[1], __builtin_ctzll(todo[1]), 64);
    else if (todo[2]) wv = __shfl(w[2], __builtin_ctzll(todo[2]), 64);
    else if (todo[3]) wv = __shfl(w[3], __builtin_ctzll(todo[3]), 64);
    else break;
    unsigned b = 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool mine = w[u] == wv;
      b |= mine ? bit[u] : 0u;
      todo[u] &= ~__ballot(mine);
    }
    // OR over the wave with DPP (row_shr 1, 2, 4, 8: lane 15 of every row holds its row; row_bcast 15 / 31: lane 63 holds
    // the wave) — seven instructions instead of six ds_bpermute round trips with their address arithmetic: the bits pass
    // is bound by instruction issue (80 % of the slots), and this loop is most of it
    int x = (int)b;
    x |= __builtin_amdgcn_update_dpp(0, x, 0x111 /* row_shr:1 */, 0xF, 0xF, true);
    x |= __builtin_amdgcn_update_dpp(0, x, 0x112 /* row_shr:2 */, 0xF, 0xF, true);
    x |= __builtin_amdgcn_update_dpp(0, x, 0x114 /* row_shr:4 */, 0xF, 0xF, true);
    x |= __builtin_amdgcn_update_dpp(0, x, 0x118 /* row_shr:8 */, 0xF, 0xF, true);
    x |= __builtin_amdgcn_update_dpp(0, x, 0x142 /* row_bcast:15 */, 0xA, 0xF, true);
    x |= __builtin_amdgcn_update_dpp(0, x, 0x143 /* row_bcast:31 */, 0xC, 0xF, true);
    b = (unsigned)__builtin_amdgcn_readlane(x, 63);
    if (lane == 0) __hip_atomic_fetch_or(mask + wv, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// listed blocks first, first + stride, ... of the agent (one wave per call; a block's points are taken 64 at a time)
// WAVE_DEDUPE: the word-level de-duplication over the 256 points in flight (k_stamp_bits_blocks: 32768 short-lived waves
// hide its ~10 us of dependent cross-lane steps per block, and the atomics' count is that kernel's cost); the persistent
// kernels, where a ticket walks dozens of blocks one after the other, only drop the bit of the predecessor lane (one DPP
// move: with the leader loop the flight's bits stage took 775 instead of 146 wave-ms per tick)
template <bool WAVE_DEDUPE = false>
__device__ __forceinline__ void stamp_bits_blocks(const GridGeom &g, const float *__restrict__ cloud, const CloudBlocks &cb,
                                                  int agent, int first, int stride, float p0, float p1, float p2,
                                                  unsigned *__restrict__ mask, int lane) {
  const CropBox box(g, p0, p1, p2);
  const int    *list = cb.list + (size_t)agent * cb.row;
  const int     n    = cb.n_list[agent];
  for (int i = first; i < n; i += stride) {  // uniform
    const int b   = list[i];
    const int beg = b * cb.block_points;
    const int end = beg + cb.block_points < cb.n_points ? beg + cb.block_points : cb.n_points;
    if constexpr (WAVE_DEDUPE) {
      for (int jb = beg; jb < end; jb += 256) {  // uniform trips of 256 points: every lane takes part in the wave OR
        float    px[4], py[4], pz[4];
        unsigned valid = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = jb + lane + u * 64;
          valid |= (idx < end ? 1u : 0u) << u;
          const size_t q = (size_t)(idx < end ? idx : end - 1) * 3;
          px[u] = cloud[q];
          py[u] = cloud[q + 1];
          pz[u] = cloud[q + 2];
        }
        stamp_bits_wave4(g, box, px, py, pz, mask, lane, valid);
      }
      continue;
    }
    int       j   = beg + lane;
    for (; j + 192 < end; j += 256) {  // four points of this lane in flight
      float px[4], py[4], pz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t q = (size_t)(j + u * 64) * 3;
        px[u] = cloud[q];
        py[u] = cloud[q + 1];
        pz[u] = cloud[q + 2];
      }
      // consecutive points of a block are neighbours along z, 0.10 m apart in 0.15 m voxels: a lane whose bit is its
      // predecessor's leaves the OR to it (the ORs are device-scope atomics that execute at the memory side: their count
      // is what the pass costs)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p    = stamp_bit_of(g, box, px[u], py[u], pz[u]);
        const int prev = __builtin_amdgcn_update_dpp(-2, p, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
        if (p >= 0 && prev != p)
          __hip_atomic_fetch_or(mask + (p >> 5), 1u << (p & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    for (; j < end; j += 64) stamp_bits_point(g, box, cloud[(size_t)j * 3], cloud[(size_t)j * 3 + 1], cloud[(size_t)j * 3 + 2], mask);
  }
}
// Bits ticket `sub` of the agent's `n_sub` (one wave each): the listed blocks of a SogmWorld frame, or the agent's range of
// the caller's cloud.
template <bool WAVE_DEDUPE = false>
__device__ __forceinline__ void bits_ticket(const GridGeom &g, const MapFrame &f, const MapTarget &t, int agent, int sub,
                                            int n_sub, int lane) {
  const float *pose = t.poses + agent * 3;
  unsigned    *mask = t.bits + (size_t)agent * t.words;
  if (f.cb.bounds) {
    stamp_bits_blocks<WAVE_DEDUPE>(g, f.cloud, f.cb, agent, sub, n_sub, pose[0], pose[1], pose[2], mask, lane);
  } else {
    const int begin = f.cloud_range[agent * 2], end = f.cloud_range[agent * 2 + 1];
    stamp_bits_range(g, f.cloud, begin + sub * 64 + lane, end, n_sub * 64, pose[0], pose[1], pose[2], mask);
  }
}
__global__ __launch_bounds__(64) void k_stamp_bits(GridGeom g, const float *__restrict__ cloud,
                                                   const int32_t *__restrict__ cloud_range,
                                                   const float *__restrict__ poses, unsigned *__restrict__ bits,
                                                   int words_per_agent, int agent0) {
  const MapFrame  f{.cloud = cloud, .cloud_range = cloud_range, .cb = {}};
  const MapTarget t{.bits = bits, .words = words_per_agent, .poses = const_cast<float *>(poses)};
  bits_ticket(g, f, t, (int)blockIdx.y + agent0, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(64) void k_stamp_bits_blocks(GridGeom g, const float *__restrict__ cloud, CloudBlocks cb,
                                                          const float *__restrict__ poses, unsigned *__restrict__ bits,
                                                          int words_per_agent) {
  const MapFrame  f{.cloud = cloud, .cb = cb};
  const MapTarget t{.bits = bits, .words = words_per_agent, .poses = const_cast<float *>(poses)};
  bits_ticket<true>(g, f, t, (int)blockIdx.y, (int)blockIdx.x, (int)gridDim.x, (int)threadIdx.x);
}
// xy bounds of every block of `block_points` consecutive points (sogm_cloud_block_bounds): one wave per block
__global__ __launch_bounds__(64) void k_block_bounds(const float *__restrict__ cloud, int n_points, int block_points,
                                                     float *__restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int beg = b * block_points, end = beg + block_points < n_points ? beg + block_points : n_points;
  float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
  for (int j = beg + lane; j < end; j += 64) {
    const float x = cloud[(size_t)j * 3], y = cloud[(size_t)j * 3 + 1];
    xlo = fminf(xlo, x);
    xhi = fmaxf(xhi, x);
    ylo = fminf(ylo, y);
    yhi = fmaxf(yhi, y);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    xlo = fminf(xlo, __shfl_xor(xlo, d, 64));
    xhi = fmaxf(xhi, __shfl_xor(xhi, d, 64));
    ylo = fminf(ylo, __shfl_xor(ylo, d, 64));
    yhi = fmaxf(yhi, __shfl_xor(yhi, d, 64));
  }
  if (lane == 0) reinterpret_cast<float4 *>(out)[b] = make_float4(xlo, xhi, ylo, yhi);
}

// Profiling build only (make EXTRA=-DSOGM_PROFILE_PRESTAMP, tools/diag_prestamp.py): 100 MHz ticks the pre-stamp's waves
// spend [0] waiting for a published agent, [1] waiting for the agent's cull / bits pass, [2] in the cull, [3] in the bits
// pass, [4] in the marks pass, of which [5] the candidate walk and [6] the slice loops; [7] tickets, [8] chunks of 64 voxels
#ifdef SOGM_PROFILE_PRESTAMP
__device__ unsigned long long g_ps_prof[12];
#define PS_CLK() wall_clock64()
#define PS_ADD(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_ps_prof[i], (unsigned long long)(v)); } while (0)
#else
#define PS_CLK() 0ll
#define PS_ADD(i, v) do { } while (0)
#endif
// CACHED: the slice loop keeps a group's sectors in registers between its store pass and its log pass (fewer
// instructions: the persistent kernels, whose occupancy is two waves per SIMD anyway); otherwise it recomputes them in a
// second pass (fewer registers: k_stamp_marks, whose scattered stores want every wave the CU can hold — 1.61 ms against
// 1.76 for the cached form on the full machine).
template <bool CACHED>
__device__ __forceinline__ void stamp_marks_trips(const GridGeom &g, void *__restrict__ grid,
                                                  unsigned *__restrict__ bits, int words_per_agent,
                                                  const SogmCylinder *__restrict__ cyl, int n_cyl,
                                                  const float *__restrict__ poses,
                                                  const CylCand *__restrict__ cand_all,
                                                  const int *__restrict__ n_cand, int agent, const MarkLog &lg,
                                                  int w_first, int w_stride, CylCand *cand_lds = nullptr,
                                                  int cand_lds_cap = 0, unsigned *lds_secs = nullptr) {
  const int      kept   = n_cand[agent];
  const bool     culled = kept <= SOGM_MAX_CYL_LDS;
  const int      n_lds  = culled ? kept : 0;
  const int      n_loop = culled ? kept : n_cyl;
  const CylCand *cand   = cand_all + (size_t)agent * SOGM_MAX_CYL_LDS;
  const float   *pose   = poses + agent * 3;
  const float    p0 = pose[0], p1 = pose[1], p2 = pose[2];
  char          *base = reinterpret_cast<char *>(grid) + (size_t)agent * g.T * (size_t)g.V * (g.half ? 2 : 4);
  unsigned      *mask = bits + (size_t)agent * words_per_agent;
  const int      lane = threadIdx.x;
  unsigned n_marks = 0, n_logged = 0;  // this lane's marks, the wave's log entries (statistics: two atomics per call)
  // One-wave workgroups of the dataflow pre-stamp stage the head of the agent's candidate list in LDS at their first
  // occupied trip (16-byte pieces, coalesced): the walk below reads every candidate for every chunk of 64 voxels, and
  // from global memory each batch of four cost a ~0.7 us L2 round trip in the tick — 51 us per chunk, three quarters of
  // the pre-stamp's wave time (tools/diag_prestamp.py) and what the tick's end waited for in half of the ticks.
  int n_staged = 0;
  bool staged  = cand_lds == nullptr;
  // a trip covers 256 mask words (8192 voxels): every lane loads four, the set bits of the whole trip are numbered
  // by a wave scan of the pop counts, and lane t of chunk b takes set bit b + t — dense lanes whatever the
  // occupancy pattern, and neighbouring lanes still hold neighbouring voxels (words_per_agent is padded to 256)
  for (int w0 = w_first; w0 < words_per_agent; w0 += w_stride) {
    uint4 *wp = reinterpret_cast<uint4 *>(mask + w0) + lane;
    uint4  w4 = *wp;
    if ((w4.x | w4.y | w4.z | w4.w) != 0u) *wp = make_uint4(0u, 0u, 0u, 0u);  // consumed: clean for the next update
    const int c0 = __popc(w4.x), c1 = c0 + __popc(w4.y), c2 = c1 + __popc(w4.z), cnt = c2 + __popc(w4.w);
    int       inc = cnt;  // inclusive prefix sum over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(inc, d, 64);
      if (lane >= d) inc += o;
    }
    const int excl  = inc - cnt;
    const int total = __shfl(inc, 63, 64);
    if (total > 0 && !staged) {  // uniform
      n_staged            = n_lds < cand_lds_cap ? n_lds : cand_lds_cap;
      const uint4 *src    = reinterpret_cast<const uint4 *>(cand);
      uint4       *dst    = reinterpret_cast<uint4 *>(cand_lds);
      const int    pieces = n_staged * (int)(sizeof(CylCand) / 16);
      for (int q = lane; q < pieces; q += 64) dst[q] = src[q];
      __syncthreads();  // (one wave: the LDS writes above are visible to the reads of the walk)
      staged = true;
    }
    for (int b0 = 0; b0 < total; b0 += 64) {  // uniform
      const int  i      = b0 + lane;
      const bool active = i < total;
      // owner lane: the last one whose exclusive prefix is <= i (binary search with lane reads; lanes with no set
      // bit share their successor's prefix and lose the comparison)
      int lo = 0, hi = 63;
#pragma unroll
      for (int it = 0; it < 6; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        const int em  = __shfl(excl, mid, 64);
        if (em <= i) lo = mid; else hi = mid - 1;
      }
      const int      own = lo;
      const int      r   = i - __shfl(excl, own, 64);  // rank of the bit among the owner's 128
      const unsigned q0 = (unsigned)__shfl((int)w4.x, own, 64), q1 = (unsigned)__shfl((int)w4.y, own, 64);
      const unsigned q2 = (unsigned)__shfl((int)w4.z, own, 64), q3 = (unsigned)__shfl((int)w4.w, own, 64);
      const int      k0 = __shfl(c0, own, 64), k1 = __shfl(c1, own, 64), k2 = __shfl(c2, own, 64);
      // Every lane of the wave goes through the slice loops (the mark log's offsets come from ballots): lanes without a
      // voxel carry v = 0 and write nothing.
      const int esh = g.half ? 4 : 3;  // cells per 32-byte sector, as a shift
      int       v   = 0;
      if (active) {
        const int sel = r < k0 ? 0 : r < k1 ? 1 : r < k2 ? 2 : 3;
        unsigned  wv  = sel == 0 ? q0 : sel == 1 ? q1 : sel == 2 ? q2 : q3;
        int       rr  = r - (sel == 0 ? 0 : sel == 1 ? k0 : sel == 2 ? k1 : k2);
        while (rr-- > 0) wv &= wv - 1;  // drop the lower set bits
        v = (w0 + own * 4 + sel) * 32 + __builtin_ctz(wv);
      }
      // slice 0 (:114), then the occupied voxel's future marks (:121-170): GT velocity of the first matching record
      if (active) {
        cell_st(base, (size_t)v, 1.0F, g.half);
        ++n_marks;
      }
      float cx, cy, cz;
      g.corner_of(g.logical_of(v), pose, cx, cy, cz);  // (v is the cell's position in the slice's storage order)
      float vx = 0.f, vy = 0.f;
      // GT velocity of the FIRST record containing the voxel (:127-154).  The walk is wave-uniform — every lane visits
      // the candidates in order until all lanes have their match — and takes the candidates four at a time: their loads
      // do not depend on the tests, so four are in flight instead of one (the walk stopped at each lane's own match
      // before: one dependent L1 round trip per candidate, ~30 us per chunk of 64 voxels with the bench scene's ~280
      // candidates, which is what an agent's pre-stamp — and the tick's tail behind the last QP — waited for).
      bool found = !active;
      [[maybe_unused]] const long long ps_w0 = PS_CLK();
      // The ordered walk only has to VISIT the candidates that can contain a voxel of this chunk.  The chunk's 64 voxels
      // are neighbouring set bits (one obstacle's cross-section, usually): their xy bounding box is tested against 64
      // candidates at a time, one per lane (a cylinder whose axis is farther from the box than its radius + 1 cm cannot
      // pass the test below for any voxel in it; rings are always visited), and the walk takes the surviving candidates
      // in list order — the first match per voxel is the one the full walk finds.  ~280 visits per chunk become a
      // handful (pre-stamp wave, list in LDS: 25 -> 5 us per chunk with the bench scene).  `cl`: the culled list, in
      // LDS (pre-stamp waves) or in global memory (k_stamp_marks: one coalesced load per 64 candidates).
      auto walk_filtered = [&](const auto *cl) __attribute__((always_inline)) {
        float xlo = active ? cx : INFINITY, xhi = active ? cx : -INFINITY;
        float ylo = active ? cy : INFINITY, yhi = active ? cy : -INFINITY;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
          xlo = fminf(xlo, __shfl_xor(xlo, d, 64));
          xhi = fmaxf(xhi, __shfl_xor(xhi, d, 64));
          ylo = fminf(ylo, __shfl_xor(ylo, d, 64));
          yhi = fmaxf(yhi, __shfl_xor(yhi, d, 64));
        }
        bool done = false;
        for (int c0 = 0; c0 < n_loop && !done; c0 += 64) {  // uniform
          bool maybe = false;
          if (c0 + lane < n_loop) {
            const CylCand cc = cl[c0 + lane];
            if (cc.type == 3) {
              const float ex = fmaxf(fmaxf(xlo - cc.x, cc.x - xhi), 0.0F), ey = fmaxf(fmaxf(ylo - cc.y, cc.y - yhi), 0.0F);
              maybe          = (double)sqrtf(ex * ex + ey * ey) <= cc.wlim + 0.01;
            } else {
              maybe = cc.type == 2;
            }
          }
          unsigned long long m = __ballot(maybe);
          while (m) {  // uniform
            const int c = c0 + __builtin_ctzll(m);
            m &= m - 1;
            const CylCand cc = cl[c];
            if (!found) {
              bool hit = false;
              if (cc.type == 2) {  // ring (:137-149)
                hit = ring_contains(cyl[cc.orig], cx, cy, cz, g.res);
              } else if (cc.type == 3) {
                const float dx = cx - cc.x, dy = cy - cc.y, dz = cz - cz;
                const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
                hit = (double)dist <= cc.wlim;
              }
              if (hit) {
                vx    = cc.vx;
                vy    = cc.vy;
                found = true;
              }
            }
            if (__builtin_amdgcn_readfirstlane((int)(__ballot(!found) == 0ull))) {
              done = true;
              break;
            }
          }
        }
      };
      if (cand_lds != nullptr && n_staged == n_loop) {
        walk_filtered(cand_lds);
      } else if (culled) {
        walk_filtered(cand);
      } else {
        for (int c0 = 0; c0 < n_loop; c0 += 4) {  // uniform
          if (__builtin_amdgcn_readfirstlane((int)(__ballot(!found) == 0ull))) break;
          int    type[4], orig[4];
          float  ox[4], oy[4], wx[4], wy[4];
          double wlim[4];
  #pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int c = c0 + u < n_loop ? c0 + u : n_loop - 1;  // (clamped: the test below skips it)
            if (c < n_lds) {
              const CylCand cc = c < n_staged ? cand_lds[c] : cand[c];
              type[u] = cc.type;
              orig[u] = cc.orig;
              ox[u]   = cc.x;
              oy[u]   = cc.y;
              wx[u]   = cc.vx;
              wy[u]   = cc.vy;
              wlim[u] = cc.wlim;
            } else {
              type[u] = cyl[c].type;
              orig[u] = c;
              ox[u]   = (float)cyl[c].x;
              oy[u]   = (float)cyl[c].y;
              wx[u]   = (float)cyl[c].vx;
              wy[u]   = (float)cyl[c].vy;
              wlim[u] = cyl[c].w + (double)g.clearance;
            }
          }
  #pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (found || c0 + u >= n_loop) continue;
            bool hit = false;
            if (type[u] == 2) {  // ring (:137-149)
              hit = ring_contains(cyl[orig[u]], cx, cy, cz, g.res);
            } else if (type[u] == 3) {  // (unknown type: the reference prints a warning and goes on, :150-152)
              const float dx = cx - ox[u], dy = cy - oy[u], dz = cz - cz;
              const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
              hit = (double)dist <= wlim[u];
            }
            if (hit) {
              vx    = wx[u];
              vy    = wy[u];
              found = true;
            }
          }
        }
      }
      [[maybe_unused]] const long long ps_w1 = PS_CLK();
      PS_ADD(5, ps_w1 - ps_w0);
      PS_ADD(8, 1);
      // the cell of slice k this voxel marks (g.V: none — outside the grid, or the reference's out-of-bounds index)
      // (the z velocity is zero — (cz + (0.0F * dt) * k) - p2 is the same number for every k — so the z part of the range
      //  test and the z index are the voxel's own, computed once: one division and four comparisons less per mark)
      const float fzc = (cz + 0.0F) - p2;
      const bool  zin = fzc > -g.rz && fzc < g.rz;
      const int   izc = (int)g.div_res(fzc + g.rz);
      auto future_cell = [&](int k) -> int {
        const float fx = (cx + (vx * g.dt) * (float)k) - p0;
        const float fy = (cy + (vy * g.dt) * (float)k) - p1;
        return zin && fx > -g.rx && fx < g.rx && fy > -g.ry && fy < g.ry ? g.cell_of_xy(fx, fy, izc) : g.V;
      };
      // Mark log (sparse reset).  The lanes of a trip hold neighbouring voxels of the slice's storage order, so the marks of
      // neighbouring lanes fall into the same 32-byte sector most of the time, in slice 0 and — same velocity — in every
      // later slice: a lane logs its sector only when no lane just below it holds the same one (rows: the lower neighbour;
      // tiles: the lanes 1, 2 and 4 below — a moving obstacle's future cells straddle two tiles in alternation), and
      // marks outside the grid log nothing.  One pass per group of eight slices: the marks are stored, the group's sectors and
      // keep bits stay in registers, one atomic reserves the group's entries, then the sectors are written.  (Until round 5 a
      // second pass recomputed every future cell — three IEEE divisions each — and every keep ballot: the stamp is bound by
      // instruction issue, not by its stores.)
      const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
      // (the lanes below through DPP — v_mov_b32_dpp, no LDS round trip like __shfl_up: a lane with no source keeps the
      //  sentinel.  wave_shr:1 crosses the rows of 16; row_shr:2 / :4 do not, so a row's first lanes keep a duplicate.)
      auto keep_of = [&](unsigned sector, bool in) -> unsigned long long {
        constexpr int NONE = (int)0xFFFFFFFDu;
        bool dup = (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x138 /* wave_shr:1 */, 0xF, 0xF, false) == sector;
        if (g.tile) {
          dup = dup || (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x112 /* row_shr:2 */, 0xF, 0xF, false) == sector;
          dup = dup || (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x114 /* row_shr:4 */, 0xF, 0xF, false) == sector;
#ifdef SOGM_LOOKBACK_FULL
          dup = dup || (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x113 /* row_shr:3 */, 0xF, 0xF, false) == sector;
          dup = dup || (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x115 /* row_shr:5 */, 0xF, 0xF, false) == sector;
          dup = dup || (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x116 /* row_shr:6 */, 0xF, 0xF, false) == sector;
          dup = dup || (unsigned)__builtin_amdgcn_update_dpp(NONE, (int)sector, 0x117 /* row_shr:7 */, 0xF, 0xF, false) == sector;
#endif
        }
        return __ballot(active && in && !dup);
      };
      // slices in groups of SG: a group's sectors and keep bits stay in registers between the store pass and the log pass
      // (a cache of all T slices cost 40 registers and halved the occupancy of the waves that call this)
      if constexpr (CACHED) {
      constexpr int SG = 8;
      unsigned     *lent = lg.entries ? lg.entries + (size_t)agent * lg.cap : nullptr;
      // the log pass of group i runs after the store pass of group i + 1: the reservation's atomic has a group's worth of
      // work to come back in
      unsigned p_secs[SG], p_keep = 0, p_off = 0;
      int      p_n = 0;  // slices of the pending group (0: none)
      auto     flush = [&]() __attribute__((always_inline)) {
        unsigned off = (unsigned)__shfl((int)p_off, 0, 64);
#pragma unroll
        for (int q = 0; q < SG; ++q)
          if (q < p_n) {  // uniform
            const bool               mine = ((p_keep >> q) & 1u) != 0;
            const unsigned long long m    = __ballot(mine);
            const unsigned           li   = off + (unsigned)__popcll(m & lt);
            if (mine && li < (unsigned)lg.cap) lent[li] = p_secs[q];
            off += (unsigned)__popcll(m);
          }
      };
      for (int k0 = 0; k0 < g.T; k0 += SG) {  // uniform
        unsigned secs[SG];
        unsigned keepbits = 0, run = 0;
#pragma unroll
        for (int q = 0; q < SG; ++q) {
          const int k = k0 + q;
          secs[q]     = 0xFFFFFFFFu;
          if (k < g.T) {  // uniform
            const int    fv = k == 0 ? v : future_cell(k);
            const bool   in = k == 0 ? true : fv < g.V;
            const size_t ci = (size_t)k * g.V + (in ? fv : 0);
            if (k != 0 && active && in) {  // (slice 0 was stored above)
              cell_st(base, ci, 1.0F, g.half);
              ++n_marks;
            }
            if (lent) {
              secs[q]                    = in ? (unsigned)(ci >> esh) : 0xFFFFFFFFu;
              const unsigned long long m = keep_of(secs[q], in);
              keepbits |= (unsigned)((m >> lane) & 1ull) << q;
              run += (unsigned)__popcll(m);
            }
          }
        }
        if (lent) {
          unsigned off = 0;
          if (lane == 0 && run) off = atomicAdd(lg.n + agent, run);  // (consumed one group later)
          n_logged += run;
          if (p_n) flush();
#pragma unroll
          for (int q = 0; q < SG; ++q) p_secs[q] = secs[q];
          p_keep = keepbits;
          p_off  = off;
          p_n    = g.T - k0 < SG ? g.T - k0 : SG;
        }
      }
      if (lent && p_n) flush();
      } else {
        unsigned *lent = lg.entries ? lg.entries + (size_t)agent * lg.cap : nullptr;
        unsigned  pref = 0, run = 0;
        // lds_secs ([T][64] words of the wave's LDS; k_stamp_marks): the store pass leaves every slice's sector there — or
        // NOT_KEPT for a lane that does not log it — and the log pass reads it back instead of recomputing the future cell
        // and the keep ballot (half of the slice loops' instructions: the kernel is bound by instruction issue)
        constexpr unsigned NOT_KEPT = 0xFFFFFFFEu;
        {
          const unsigned long long m = keep_of((unsigned)v >> esh, true);
          run                        = (unsigned)__popcll(m);
          if (lds_secs) lds_secs[lane] = ((m >> lane) & 1ull) ? (unsigned)v >> esh : NOT_KEPT;
        }
        for (int k = 1; k < g.T; ++k) {
          const int    fv = future_cell(k);
          const bool   in = fv < g.V;
          const size_t ci = (size_t)k * g.V + (in ? fv : 0);
          if (active && in) {
            cell_st(base, ci, 1.0F, g.half);
            ++n_marks;
          }
          if (lent) {
            const unsigned long long m = keep_of(in ? (unsigned)(ci >> esh) : 0xFFFFFFFFu, in);
            if (lane == (k & 63)) pref = run;
            run += (unsigned)__popcll(m);
            if (lds_secs) lds_secs[k * 64 + lane] = ((m >> lane) & 1ull) ? (unsigned)(ci >> esh) : NOT_KEPT;
          }
        }
        if (lent && g.T <= 64) {
          unsigned lbase = 0;
          if (lane == 0) lbase = atomicAdd(lg.n + agent, run);
          lbase          = (unsigned)__shfl((int)lbase, 0, 64);
          n_logged += run;
          if (lds_secs) {
            for (int k = 0; k < g.T; ++k) {
              const unsigned           sec  = lds_secs[k * 64 + lane];  // (this lane's own word: no cross-lane hazard)
              const bool               mine = sec != NOT_KEPT;
              const unsigned long long m    = __ballot(mine);
              const unsigned           li   = lbase + (unsigned)__shfl((int)pref, k, 64) + (unsigned)__popcll(m & lt);
              if (mine && li < (unsigned)lg.cap) lent[li] = sec;
            }
          } else
          for (int k = 0; k < g.T; ++k) {
            const int                fv  = k == 0 ? v : future_cell(k);
            const bool               in  = fv < g.V;
            const unsigned           sec = in ? (unsigned)(((size_t)k * g.V + fv) >> esh) : 0xFFFFFFFFu;
            const unsigned long long m   = keep_of(sec, in);
            const unsigned           li  = lbase + (unsigned)__shfl((int)pref, k, 64) + (unsigned)__popcll(m & lt);
            if (((m >> lane) & 1ull) && li < (unsigned)lg.cap) lent[li] = sec;
          }
        } else if (lent && lane == 0) {
          // (T > 64: no log — the agent's next reset is the dense one.  A saturating mark: an add per trip could carry the
          //  unsigned counter past 2^32 and back under `cap`, and the next sparse reset would trust an empty log)
          atomicMax(lg.n + agent, (unsigned)lg.cap + 1u);
        }
      }
      PS_ADD(6, PS_CLK() - ps_w1);
    }
  }
  if (lg.stat) {
    for (int d = 32; d >= 1; d >>= 1) n_marks += (unsigned)__shfl_xor((int)n_marks, d, 64);
    if (lane == 0 && n_marks) {
      atomicAdd(lg.stat, (unsigned long long)n_marks);
      atomicAdd(lg.stat + 1, (unsigned long long)n_logged);
    }
  }
}
// Marks ticket `sub` of the agent's `n_sub` (one wave each; a trip is 256 mask words).  cand_lds: the wave's LDS candidate
// cache, free again for the next ticket's staging when this returns; lds_secs: k_stamp_marks' sector cache.
template <bool CACHED>
__device__ __forceinline__ void marks_ticket(const GridGeom &g, const MapFrame &f, const MapTarget &t, int agent, int sub,
                                             int n_sub, CylCand *cand_lds = nullptr, int cand_lds_cap = 0,
                                             unsigned *lds_secs = nullptr) {
  stamp_marks_trips<CACHED>(g, t.grid, t.bits, t.words, f.cyl, f.n_cyl, t.poses, (const CylCand *)t.cand, t.n_cand, agent, t.lg,
                            sub * 256, n_sub * 256, cand_lds, cand_lds_cap, lds_secs);
  if (cand_lds) __syncthreads();
}

__global__ __launch_bounds__(64) void k_stamp_marks(GridGeom g, void *__restrict__ grid,
                                                    unsigned *__restrict__ bits, int words_per_agent,
                                                    const SogmCylinder *__restrict__ cyl, int n_cyl,
                                                    const float *__restrict__ poses,
                                                    const CylCand *__restrict__ cand_all,
                                                    const int *__restrict__ n_cand, int agent0, MarkLog lg, int lds_log) {
  extern __shared__ unsigned s_marks_secs[];  // [T][64] when the launch provides it (lds_log != 0)
  const MapFrame  f{.cyl = cyl, .n_cyl = n_cyl};
  const MapTarget t{.grid = grid, .bits = bits, .words = words_per_agent, .cand = const_cast<CylCand *>(cand_all),
                    .n_cand = const_cast<int *>(n_cand), .lg = lg, .poses = const_cast<float *>(poses)};
  marks_ticket<false>(g, f, t, (int)blockIdx.y + agent0, (int)blockIdx.x, (int)gridDim.x, nullptr, 0,
                      lds_log ? s_marks_secs : nullptr);
}
// (the register-cached single-pass form of the slice loops: tuning key stamp_cached)
__global__ __launch_bounds__(64) void k_stamp_marks_cached(GridGeom g, void *__restrict__ grid,
                                                           unsigned *__restrict__ bits, int words_per_agent,
                                                           const SogmCylinder *__restrict__ cyl, int n_cyl,
                                                           const float *__restrict__ poses,
                                                           const CylCand *__restrict__ cand_all,
                                                           const int *__restrict__ n_cand, int agent0, MarkLog lg) {
  const MapFrame  f{.cyl = cyl, .n_cyl = n_cyl};
  const MapTarget t{.grid = grid, .bits = bits, .words = words_per_agent, .cand = const_cast<CylCand *>(cand_all),
                    .n_cand = const_cast<int *>(n_cand), .lg = lg, .poses = const_cast<float *>(poses)};
  marks_ticket<true>(g, f, t, (int)blockIdx.y + agent0, (int)blockIdx.x, (int)gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// neighbour overlay
// ------------------------------------------------------------------------------------------------
// Mark-log reservation of `count` entries for every lane active at the call (count uniform): one atomic per agent
// present among those lanes — a wave of the overlay holds one or two agents — instead of one per lane (2540 lanes
// per agent hammering one counter cost the overlay 0.8 ms).
__device__ inline unsigned log_reserve(const MarkLog &lg, int agent, unsigned count) {
  const int                lane = (int)(threadIdx.x & 63);
  const unsigned long long lt   = lane ? (~0ull >> (64 - lane)) : 0ull;
  unsigned long long       todo = __ballot(1);
  unsigned                 base = 0;
  while (todo) {  // uniform over the active lanes
    const int                leader = __ffsll((long long)todo) - 1;
    const int                la     = __shfl(agent, leader, 64);
    const unsigned long long grp    = __ballot(agent == la) & todo;
    unsigned                 b      = 0;
    if (lane == leader) b = atomicAdd(lg.n + la, count * (unsigned)__popcll(grp));
    b = (unsigned)__shfl((int)b, leader, 64);
    if (agent == la) base = b + count * (unsigned)__popcll(grp & lt);
    todo &= ~grp;
  }
  return base;
}

// One lane per (agent, record, slice).  The reference's is_swarm_traj_valid chain
// (risk_base.cpp:154-159) collapses to: record contributes at slice t  iff
//     time_start < t_abs(0)  and  t_abs(s) < time_end for every s <= t
// and t_abs is increasing, i.e.  time_start < t_abs(0) && t_abs(t) < time_end.
// one (agent, record, slice) item of the overlay
__device__ inline void splat_item(const GridGeom &g, void *__restrict__ grid, const SogmTrajRecord &R, int agent,
                                  int t, const int32_t *__restrict__ ego_ids, const float *__restrict__ poses,
                                  const double *__restrict__ stamps, const double *__restrict__ body, int n_body,
                                  const MarkLog &lg) {
  // mark log (sparse reset): a lane that writes reserves n_body entries (or one) and fills them with the sectors of
  // its cells, ~0 for a particle outside the grid
  const int    esh   = g.half ? 4 : 3;
  const size_t tslab = (size_t)t * g.V;
  unsigned    *lent  = lg.entries ? lg.entries + (size_t)agent * lg.cap : nullptr;
  if (R.n_pieces <= 0 || R.drone_id == ego_ids[agent]) return;
  double time_end = R.time_start;
  for (int k = 0; k < R.n_pieces; ++k) time_end += R.duration[k];
  const double stamp = stamps[agent];
  const double t0    = stamp + (double)(g.dt * (float)0);
  const double tt    = stamp + (double)(g.dt * (float)t);
  if (g.map_kind == SOGM_MAP_RISKVOXEL) {
    // RiskVoxel::addOtherAgents (risk_voxel.cpp:258-288) calls getWaypoints (particles.cpp:316-344)
    // directly and SETS cells (:311-318).  The record is visited at slice t iff every earlier slice
    // returned true (running or not yet started); on the slice where it has ended its last point is
    // stamped once, without body particles.
    for (int s_ = 0; s_ < t; ++s_) {
      const double ts = stamp + (double)(g.dt * (float)s_);
      if (!((R.time_start < ts && time_end > ts) || R.time_start > ts)) return;
    }
    const float *pose = poses + agent * 3;
    const double q0 = (double)pose[0], q1 = (double)pose[1], q2 = (double)pose[2];
    char        *slab = reinterpret_cast<char *>(grid) + ((size_t)agent * g.T + t) * (size_t)g.V * (g.half ? 2 : 4);
    double       p[3];
    if (R.time_start < tt && time_end > tt) {
      bezier_pos(R, tt - R.time_start, p);
      const unsigned lb = lent ? log_reserve(lg, agent, (unsigned)n_body) : 0u;
      for (int e = 0; e < n_body; ++e) {
        const float fx = (float)((p[0] + body[e * 3 + 0]) - q0);
        const float fy = (float)((p[1] + body[e * 3 + 1]) - q1);
        const float fz = (float)((p[2] + body[e * 3 + 2]) - q2);
        const int   vl = g.in_range(fx, fy, fz) ? g.voxel_of(fx, fy, fz) : g.V;
        const bool  in = vl < g.V;  // (index >= V: the reference's out-of-bounds case, see k_stamp_bits)
        const int   vx = in ? g.phys_of(vl) : g.V;
        if (in) cell_st(slab, vx, 1.0F, g.half);
        if (lent && lb + (unsigned)e < (unsigned)lg.cap) lent[lb + e] = in ? (unsigned)((tslab + vx) >> esh) : 0xFFFFFFFFu;
      }
    } else if (time_end < tt) {
      double dur = 0.0;
      for (int k = 0; k < R.n_pieces; ++k) dur += R.duration[k];
      bezier_pos(R, dur, p);
      const float fx = (float)(p[0] - q0), fy = (float)(p[1] - q1), fz = (float)(p[2] - q2);
      const int vl = g.in_range(fx, fy, fz) ? g.voxel_of(fx, fy, fz) : g.V;
      const int vx = vl < g.V ? g.phys_of(vl) : g.V;
      if (vx < g.V) {
        cell_st(slab, vx, 1.0F, g.half);
        if (lent) {
          const unsigned lb = atomicAdd(lg.n + agent, 1u);
          if (lb < (unsigned)lg.cap) lent[lb] = (unsigned)((tslab + vx) >> esh);
        }
      }
    }
    return;
  }
  if (!(R.time_start < t0 && time_end > t0)) return;  // chain broken at slice 0
  if (!(R.time_start < tt && time_end > tt)) return;

  double p[3];
  bezier_pos(R, tt - R.time_start, p);
  const float *pose = poses + agent * 3;
  const double q0 = (double)pose[0], q1 = (double)pose[1], q2 = (double)pose[2];
  char        *slab = reinterpret_cast<char *>(grid) + ((size_t)agent * g.T + t) * (size_t)g.V * (g.half ? 2 : 4);
  // getParticlesWithRisk (particles.cpp:365-409): pos_stddev = replan_risk_rate * (t - time_start) in float; below 1e-3
  // (every shipped configuration: the rate is 0) each body particle counts 1.0; otherwise each is replaced by
  // num_resample Gaussian samples whose weights are normalised to num_resample per particle.
  const float sd = g.rs_rate * (float)(tt - R.time_start);
  if (g.rs_n > 0 && g.rs_z != nullptr && !(sd < 1e-3F)) {
    // The reference draws from std::default_random_engine(time(NULL)) — re-seeded at every call, so every call within
    // one second sees the same sequence: the injected table plays that sequence, entry 3 (e n + i) + d for sample i of
    // particle e, axis d (sogm_set_resample).  Weights: float arithmetic in the reference's order; exp through
    // sogm_det::expf_neg on both sides.  (RiskBase::addOtherAgents indexes ONE risks vector, cleared by every
    // getParticlesWithRisk call, with the particles of ALL agents — an out-of-bounds read once two agents contribute;
    // here and in the oracle a particle adds its own weight, the evident intent.)
    const int      n  = g.rs_n;
    const unsigned lb = lent ? log_reserve(lg, agent, (unsigned)(n_body * n)) : 0u;
    for (int e = 0; e < n_body; ++e) {
      const double w0 = p[0] + body[e * 3 + 0], w1 = p[1] + body[e * 3 + 1], w2 = p[2] + body[e * 3 + 2];
      const float *z  = g.rs_z + 3 * e * n;
      float        sum = 0.0F;  // std::accumulate(risk_buf.begin(), risk_buf.end(), 0.0f)
      for (int i = 0; i < n; ++i) {
        const float nx = z[3 * i] * sd, ny = z[3 * i + 1] * sd, nz = z[3 * i + 2] * sd;
        sum += sogm_det::expf_neg((-0.5F * ((nx * nx + ny * ny) + nz * nz)) / (sd * sd));
      }
      for (int i = 0; i < n; ++i) {
        const float nx = z[3 * i] * sd, ny = z[3 * i + 1] * sd, nz = z[3 * i + 2] * sd;
        const float rk = (sogm_det::expf_neg((-0.5F * ((nx * nx + ny * ny) + nz * nz)) / (sd * sd)) * (float)n) / sum;
        const float fx = (float)((w0 + (double)nx) - q0);
        const float fy = (float)((w1 + (double)ny) - q1);
        const float fz = (float)((w2 + (double)nz) - q2);
        const int   vl = g.in_range(fx, fy, fz) ? g.voxel_of(fx, fy, fz) : g.V;
        const bool  in = vl < g.V;
        const int   vx = in ? g.phys_of(vl) : g.V;
        const unsigned li = lb + (unsigned)(e * n + i);
        if (lent && li < (unsigned)lg.cap) lent[li] = in ? (unsigned)((tslab + vx) >> esh) : 0xFFFFFFFFu;
        if (in) cell_add(slab, vx, rk, g.half);  // (fractional weights: the sum depends on the order in the last bits)
      }
    }
    return;
  }
  // a neighbour farther outside the map than its body reaches marks nothing: no log entries, no 36 range tests (most
  // (agent, record) pairs of a swarm spread over many map widths; 1 cm of slack covers the fp32 rounding of the test below)
  if (fabs(p[0] - q0) > (double)g.rx + (double)g.body_ext[0] + 0.01 || fabs(p[1] - q1) > (double)g.ry + (double)g.body_ext[1] + 0.01 ||
      fabs(p[2] - q2) > (double)g.rz + (double)g.body_ext[2] + 0.01)
    return;
  const unsigned lb = lent ? log_reserve(lg, agent, (unsigned)n_body) : 0u;
  for (int e = 0; e < n_body; ++e) {
    const float fx = (float)((p[0] + body[e * 3 + 0]) - q0);
    const float fy = (float)((p[1] + body[e * 3 + 1]) - q1);
    const float fz = (float)((p[2] + body[e * 3 + 2]) - q2);
    const int   vl = g.in_range(fx, fy, fz) ? g.voxel_of(fx, fy, fz) : g.V;
    const bool  in = vl < g.V;
    const int   vx = in ? g.phys_of(vl) : g.V;
    if (lent && lb + (unsigned)e < (unsigned)lg.cap) lent[lb + e] = in ? (unsigned)((tslab + vx) >> esh) : 0xFFFFFFFFu;
    if (!in) continue;
    // += 1.0f per body particle; sums of 1.0 are exact in fp32 (and in fp16 up to 2048), so the order
    // is immaterial
    cell_add(slab, vx, 1.0F, g.half);
  }
}
// Overlay: record r at slice `slice` into the agent's map, and ticket `sub` of the agent's `n_sub` (one wave each) over the
// n_rec * T items of a table — the one table every agent reads (o.stride 0) or the agent's own view of it (o.stride n_rec).
__device__ __forceinline__ void overlay_item(const GridGeom &g, const OverlayIO &o, const MapTarget &t, int agent, int r,
                                             int slice) {
  splat_item(g, t.grid, o.rec[(size_t)agent * o.stride + r], agent, slice, o.ego_ids, t.poses, t.stamps, o.body, o.n_body, t.lg);
}
__device__ __forceinline__ void overlay_ticket(const GridGeom &g, const OverlayIO &o, const MapTarget &t, int agent, int sub,
                                               int n_sub, int lane) {
  const int n = o.n_rec * g.T;
  for (int i = sub * 64 + lane; i < n; i += n_sub * 64) overlay_item(g, o, t, agent, i / g.T, i % g.T);
}
__global__ __launch_bounds__(256) void k_splat_neighbours(
    GridGeom g, void *__restrict__ grid, const SogmTrajRecord *__restrict__ rec, int n_rec, int rec_stride,
    const int32_t *__restrict__ ego_ids, const float *__restrict__ poses,
    const double *__restrict__ stamps, const double *__restrict__ body, int n_body, int n_agents, int agent0,
    MarkLog lg, const int *wait_stage, int *wait_err) {
  const OverlayIO o{.rec = rec, .n_rec = n_rec, .stride = rec_stride, .ego_ids = ego_ids, .body = body, .n_body = n_body};
  const MapTarget tgt{.grid = grid, .lg = lg, .poses = const_cast<float *>(poses), .stamps = const_cast<double *>(stamps)};
  const long long total  = (long long)n_agents * n_rec * g.T;
  const long long stride = (long long)gridDim.x * blockDim.x;  // (one item per lane unless the launch is narrower)
  for (long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += stride) {
    const int t     = (int)(gid % g.T);
    const int r     = (int)((gid / g.T) % n_rec);
    const int agent = agent0 + (int)(gid / ((long long)g.T * n_rec));
    if (wait_stage) {
      // launched under the tail of the pre-stamp that builds this grid (sogm_update_prestamped): an agent's overlay
      // starts when ITS stamp is complete — stores of 1.0 first, the overlay's additions after them, as in the serial
      // order.  The launch is narrow (the waiting lanes must leave room for the pre-stamp's own waves: a full-size
      // grid of pollers starved a pre-stamp that was not resident yet until the timeouts fired).  Bounded: a
      // pre-stamp that failed has set the error word (the tick is reported as failed); nothing is written then, and an
      // overlay whose own wait runs out sets it: the tick is reported as failed (the report runs behind the pre-stamp), not
      // silently left without its overlay.  Every lane waits for the word of its own item's agent.
      if (!lane_wait_at_least(wait_stage + agent, FLOW_PS_DONE, wait_err, FLOW_CODE_OVERLAY_STAMP)) return;
    }
    overlay_item(g, o, tgt, agent, r, t);
  }
}

// ------------------------------------------------------------------------------------------------
// Pre-stamp: the NEXT tick's map built inside this tick's replan (dataflow replan only).
// The tick's critical path was "stamp (1.8 ms, nothing else running) -> chain of the slowest agent"; but an agent's
// next map centre only depends on its OWN new record, which is final the moment a finishing block of k_worker_flow publishes it.  This
// persistent kernel (launched behind the gate that holds stores back until every agent's corridors are final)
// takes agents in publication order and, for each: samples the start state of the next tick (k_tick_inputs' rule),
// culls the cylinders, sets the occupancy bits and writes the marks + log entries into the pool's next grid — split
// into ps.n_bits + ps.n_marks one-wave tickets per agent (64 + 64 by default) handed out in order (a ticket only ever waits for lower ones, so
// any number of resident waves makes progress).  The next update then only adopts the grid and adds the overlay
// (sogm_update_prestamped).  The lock-step kernels' ticket bodies (stage_record_hover, cull_ticket, bits_ticket,
// marks_ticket): same cells.
// ------------------------------------------------------------------------------------------------
// Launch gate of the pre-stamp (one lane, on its stream in front of it): every agent's corridors final — store streams
// stay away from the searches and point scans — AND every QP workgroup and finishing wave of this replan resident:
// the pre-stamp's waves wait for what those produce, and a QP workgroup that is not placed yet (its launch can sit
// behind another kernel when streams share a hardware queue) needs a whole CU, which thousands of small waiting
// waves would never leave it.  Bounded like every wait of the tick: on a timeout the tick fails, the waves drain.
__global__ void k_prestamp_gate(int *hdr, int n_agents, int n_qp, int n_finish) {
  if (threadIdx.x != 0) return;
  bounded_wait<WaitPrestampGate, false>(&hdr[FLOW_ERR], [&] {
    return flow_peek<false>(&hdr[FLOW_Q_READY_N]) >= n_agents && flow_peek<false>(&hdr[FLOW_Q_RESIDENT]) >= n_qp &&
           flow_peek<false>(&hdr[FLOW_F_TICKET]) >= n_finish;
  });
}
__global__ __launch_bounds__(64) void k_prestamp_flow(GridGeom g, FlowCtl fc, PrestampDev ps) {
  __shared__ __attribute__((aligned(16))) SogmTrajRecord s_rec;
  __shared__ double                                      s_hov[9];
  __shared__ __attribute__((aligned(16))) CylCand        s_cand[PRESTAMP_CAND_LDS];
  const int lane  = threadIdx.x;
  // the last agents to be published get finer tickets: nobody is left to share the waves with, and their stamps are
  // what trails the replan
  const int n_early = ps.n_agents > ps.n_late ? ps.n_agents - ps.n_late : 0;
  const int per_e = ps.n_bits + ps.n_marks, per_l = ps.n_bits_late + ps.n_marks_late;
  const int total = n_early * per_e + (ps.n_agents - n_early) * per_l;
  for (;;) {
    const int t = flow_ticket(&fc.hdr[FLOW_P_TICKET]);
    if (t >= total) break;
    [[maybe_unused]] const long long ps_t0 = PS_CLK();
    PS_ADD(7, 1);
    const bool late = t >= n_early * per_e;
    const int  tl   = late ? t - n_early * per_e : t;
    const int  per  = late ? per_l : per_e;
    const int  n_bits = late ? ps.n_bits_late : ps.n_bits, n_marks = late ? ps.n_marks_late : ps.n_marks;
    const int agent = flow_wait_slot(fc.p_ready + (late ? n_early : 0) + tl / per, &fc.hdr[FLOW_ERR]);
    if (agent < 0) break;
    PS_ADD(0, PS_CLK() - ps_t0);
    __threadfence();  // the agent's own record was published before its slot
    const int  s   = tl % per;
    long long *pts = fc.ts + 8 * (size_t)ps.n_agents + 4 * (size_t)agent;  // diagnostics (sogm_debug_prestamp_times)
    if (s == 0) {
      [[maybe_unused]] const long long ps_c0 = PS_CLK();
      if (lane == 0) pts[0] = wall_clock64();
      // next tick's inputs of this agent (k_tick_inputs), then its candidate cylinders around the new centre
      stage_record_hover(&s_rec, s_hov, ps.tick.own, ps.tick.hover, agent, lane);
      if (lane == 0) {
        tick_inputs_agent(s_rec, s_hov, agent, ps.stamp, ps.tick, ps.tgt.poses);
        ps.tgt.stamps[agent] = ps.stamp;
        if (ps.poses_host)
          for (int k = 0; k < 3; ++k) ps.poses_host[agent * 3 + k] = ps.tgt.poses[agent * 3 + k];
      }
      __threadfence();
      __syncthreads();
      cull_ticket(g, ps.frame, ps.tgt, agent, ps.tgt.poses[agent * 3], ps.tgt.poses[agent * 3 + 1], lane);
      __threadfence();
      if (lane == 0) {
        pts[1] = wall_clock64();
        atomicAdd(&fc.stage[agent], 1);
      }
      PS_ADD(2, PS_CLK() - ps_c0);
    }
    [[maybe_unused]] const long long ps_t1 = PS_CLK();
    if (s < n_bits) {
      if (flow_wait_count(&fc.stage[agent], 1, &fc.hdr[FLOW_ERR])) break;
      [[maybe_unused]] const long long ps_t2 = PS_CLK();
      PS_ADD(1, ps_t2 - ps_t1);
      bits_ticket(g, ps.frame, ps.tgt, agent, s, n_bits, lane);
      __threadfence();
      PS_ADD(3, PS_CLK() - ps_t2);
      if (lane == 0 && atomicAdd(&fc.stage[agent], 1) + 1 == 1 + n_bits) pts[2] = wall_clock64();
    } else {
      if (flow_wait_count(&fc.stage[agent], 1 + n_bits, &fc.hdr[FLOW_ERR])) break;
      [[maybe_unused]] const long long ps_t2 = PS_CLK();
      PS_ADD(1, ps_t2 - ps_t1);
      marks_ticket<true>(g, ps.frame, ps.tgt, agent, s - n_bits, n_marks, s_cand, PRESTAMP_CAND_LDS);
      // the agent's last marks ticket to finish declares its grid complete (the next update's overlay waits for it)
      __threadfence();
      PS_ADD(4, PS_CLK() - ps_t2);
      if (lane == 0 && atomicAdd(&fc.stage[agent], 1) + 1 == 1 + n_bits + n_marks) {
        pts[3] = wall_clock64();
        __hip_atomic_store(&fc.stage[agent], FLOW_PS_DONE, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
#ifdef SOGM_PROFILE_PRESTAMP
}  // namespace sogm
extern "C" int sogm_debug_prestamp_prof(unsigned long long *out12_host, int reset) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (out12_host && hipMemcpyFromSymbol(out12_host, HIP_SYMBOL(sogm::g_ps_prof), sizeof(unsigned long long) * 12) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[12] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(sogm::g_ps_prof), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
namespace sogm {
#endif
// ------------------------------------------------------------------------------------------------
// Flight kernel M (sogm_flight_run; the flight is described in sogm_planner.hpp): an agent's map of its next tick, built
// the moment the agent's previous tick is finished.  Per (agent, tick) 1 + n_reset + n_bits + n_marks + n_splat one-wave
// tickets in four phases; every phase is a queue of its own and a wave claims — never blocking — a ticket of the LATEST
// phase that has one (a first version handed all tickets of an item out in order and let them wait for each other: 512
// waves / 61 tickets = 8 items in flight, the swarm's maps took 17 ms per tick).  Only the head may wait: for the swarm's
// tick k - 2.
//   head    gate "every agent has finished tick k - 2" (the staleness rule's other half: table ver(k - 2) is complete);
//           start state / map centre / stamp of tick k from the agent's executed record (k_tick_inputs' rule);
//           candidate cylinders and cloud blocks of frame k around the new centre
//   reset   the agent's grid back to zero through its mark log (k_reset_sectors' 2-lanes-per-sector form; an overflowed
//           log: the whole grid), then the log restarts
//   bits    occupancy bits of slice 0 from the listed cloud blocks
//   marks   slice 0 + T - 1 future marks per occupied voxel, logged
//   splat   the neighbours' records of table ver(k - 2), logged -> the agent goes to the search queue
// The per-tick kernels' ticket bodies (stage_record_hover, cull_ticket, bits_ticket, marks_ticket, overlay_ticket): same cells.
// ------------------------------------------------------------------------------------------------
// frame k of the flight as the ticket bodies read it: the tick's world record + the context's crop lists
__device__ __forceinline__ MapFrame flight_frame(const FlightMapDev &d, int kl) {
  const FlightWorld &w = d.worlds[kl];
  MapFrame f{.cloud = w.cloud, .cloud_range = nullptr, .cb = d.cb, .cyl = w.cyl, .n_cyl = w.n_cyl};
  f.cb.bounds       = w.bounds;
  f.cb.n_blocks     = w.n_blocks;
  f.cb.block_points = w.block_points;
  f.cb.n_points     = w.n_points;
  return f;
}
__device__ __forceinline__ void flight_reset_ticket(char *__restrict__ base, size_t agent_bytes, const unsigned *__restrict__ e,
                                                    unsigned n, int cap, int first, int stride, int lane,
                                                    unsigned long long *__restrict__ stat) {
  const vfloat4 z = {0.f, 0.f, 0.f, 0.f};
  if (n > (unsigned)cap) {  // overflowed log: this ticket's share of the whole grid (agent_bytes is a multiple of 32)
    const size_t nv = agent_bytes / 16;
    for (size_t i = (size_t)first * 64 + lane; i < nv; i += (size_t)stride * 64)
      __builtin_nontemporal_store(z, reinterpret_cast<vfloat4 *>(base) + i);
    return;
  }
  const int part = lane & 1, pair = lane >> 1;
  unsigned  n_lines = 0;
  // 32 entries per trip, two lanes each; EIGHT trips' entry loads are issued together (a trip by itself is one dependent
  // load -> store pair: ~1 us per trip, 1.05 ms per ticket of 40 k entries in the first flights)
  constexpr int U = 8;
  const size_t  step = (size_t)stride * 32;
  for (size_t i0 = (size_t)first * 32; i0 < n; i0 += U * step) {
    unsigned sct[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t i = i0 + u * step + pair;
      sct[u]         = i < n ? e[i] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned prev = __shfl_up(sct[u], 2);
      if (sct[u] == 0xFFFFFFFFu || (pair > 0 && prev == sct[u])) continue;
      const size_t off = (size_t)sct[u] * 32 + 16 * part;
      if (off + 16 <= agent_bytes) *reinterpret_cast<vfloat4 *>(base + off) = z;
      if (part == 0) ++n_lines;
    }
  }
  if (stat) {
    for (int d = 32; d >= 1; d >>= 1) n_lines += (unsigned)__shfl_xor((int)n_lines, d, 64);
    if (lane == 0 && n_lines) atomicAdd(stat + 2, (unsigned long long)n_lines * 32ull);
  }
}
__global__ __launch_bounds__(64) void k_flight_map(GridGeom g, FlightCtl fl, FlightMapDev d, unsigned long long *reset_stat) {
  __shared__ __attribute__((aligned(16))) SogmTrajRecord s_rec;
  __shared__ double                                      s_hov[9];
  __shared__ __attribute__((aligned(16))) CylCand        s_cand[PRESTAMP_CAND_LDS];
  const int lane = threadIdx.x;
  const int A    = fl.n_agents;
  // (the urgent lane cuts a map into finer tickets: a map's latency is the sum of its phases' longest tickets — 0.25 reset +
  //  0.3 marks + 0.17 overlay ms with the plain lane's counts even on idle workers — and the urgent lane exists for latency)
  int      *err = &fl.hdr[FL_ERR];
  fl_wg_started(fl, 3);
  // (every lane of this kernel ends when the call's last finish has stored the call's epoch in hdr[FL_END])
  if ((int)blockIdx.x < d.n_head_wgs) {
    // ---- admitting waves: heads, in the order the agents' previous ticks finished; the first n_uhead_wgs serve the
    // urgent ring: no admission order, no pace, no window (the gate is open for an agent that is behind) ----
    const bool urgent = (int)blockIdx.x < d.n_uhead_wgs;
    const int  n_r = urgent ? d.un_reset : d.n_reset, n_b = urgent ? d.un_bits : d.n_bits;
    unsigned long long *const wq      = urgent ? fl.uw : fl.mw;
    int *const                wq_tail = &fl.hdr[urgent ? FL_UW_TAIL : FL_MW_TAIL];
    for (;;) {
      const int t     = flow_ticket(&fl.hdr[urgent ? FL_U_TICKET : FL_M_TICKET]);
      const int agent = fl_wait_item_end(urgent ? fl.u_ring : fl.m_ring, fl.ring_mask, t, err, &fl.hdr[FL_END], fl.epoch, !urgent);
      if (agent < 0) break;
      __threadfence();
      const int      k = fl.tick_of[agent], kl = k - fl.first_tick;
      const MapFrame frame = flight_frame(d, kl);
      long long     *ts = fl.ts + (size_t)agent * FL_TS;
      if (lane == 0) ts[8] = wall_clock64();
      // admission, in ticket order: at most n_admit maps under construction, and no faster than one agent per pace_ticks
      // — agents then leave the map stage (and reach every later stage) at a steady rate instead of in a burst, which is
      // what lets kernels with FIXED compute units all be busy at once: a swarm that moves in step serves one stage at a
      // time and the tick becomes the SUM of the stages' times (measured: 12.9 ms = 5.6 map + 3.7 corridors + 3.4 QP).
      // my turn: a tight poll — a handful of waves wait here, and the hand-over from head to head is the admission rate
      if (!urgent && wait_at_least<WaitAdmission, true>(err, &fl.hdr[FL_ADMITTED], t) < 0) break;
      if (!urgent && flow_wait_count(&fl.hdr[FL_MAPS_DONE], t - d.n_admit + 1, err)) break;
      if (!urgent && lane == 0) {
        long long *pc = reinterpret_cast<long long *>(&fl.hdr[FL_PACE_CLOCK]);
        while (wall_clock64() - *pc < d.pace_ticks) __builtin_amdgcn_s_sleep(16);
        *pc = wall_clock64();
        __hip_atomic_store(&fl.hdr[FL_ADMITTED], t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (lane == 0) ts[9] = wall_clock64();
      stage_record_hover(&s_rec, s_hov, d.tick.own, d.tick.hover, agent, lane);
      const double stamp = d.t0 + k * d.period;
      if (lane == 0) {
        if (d.fsm.state)  // the head of one FSMCallback (sogm_planner_set_flight_fsm): k_fsm_inputs' body for this agent
          fsm_inputs_agent(d.fsm.prm, d.fsm.state[agent], s_rec, s_hov, d.fsm.goals + agent * 3, agent, stamp, d.tick.hover,
                           d.tick.now, d.tick.t_start, d.tick.pva, d.tgt.poses, d.fsm.pos_now, d.fsm.due, d.fsm.reached,
                           [](const SogmTrajRecord &r, double t, double *o) { return traj_eval_record(r, t, o); });
        else
          tick_inputs_agent(s_rec, s_hov, agent, stamp, d.tick, d.tgt.poses);
        d.tgt.stamps[agent] = stamp;
      }
      __threadfence();
      __syncthreads();
      cull_ticket(g, frame, d.tgt, agent, d.tgt.poses[agent * 3], d.tgt.poses[agent * 3 + 1], lane);
      __threadfence();
      if (lane == 0) {  // the agent's grid may be reset and its occupancy bits set (neither touches what the other writes)
        ts[12] = wall_clock64();
        atomicExch(&fl.stage[agent], 1);  // (the agent's previous map is complete: nobody else touches the counter now)
        wq_push(wq, wq_tail, wk_pack(WK_MAP_RESET, 0, agent), n_r);
        wq_push(wq, wq_tail, wk_pack(WK_MAP_BITS, 0, agent), n_b);
      }
      __syncthreads();
    }
    return;
  }
  // ---- workers.  Every worker holds a ticket of the plain queue, as before; the first n_uwork_wgs of them look at the urgent
  // queue first — before they take a plain descriptor and while they wait for one — and claim an urgent descriptor that is
  // THERE with a compare-and-swap on the queue's head (never a ticket for one that is not: a worker must not be lost to the
  // plain lane waiting for urgent work; the claim is tried once per look, so the waves do not spin on the counter).  A
  // first version gave the urgent lane 128 workers of its own: they idled most of the time, which a flight whose map
  // kernel is the bottleneck paid for (300^3 x 30: 11.5 -> 13.7 ms per tick).  A map stays in the lane its head put it in:
  // the next phase's descriptors go into the queue the finished one came from. ----
  const bool ulane = (int)blockIdx.x - d.n_head_wgs < d.n_uwork_wgs;
  WqWorker   ww;
  long long c1_prev = 0;
  int       kind_prev = 0;
  for (;;) {
    const long long c0     = wall_clock64();
    bool            urgent = false;
    // (a worker that also serves the urgent lane naps 14 ... 28 us between two looks, the others up to 110)
    const int desc = wq_take2(fl.mw, &fl.hdr[FL_MW_HEAD], fl.uw, &fl.hdr[FL_UW_TAIL], &fl.hdr[FL_UW_HEAD], ww, ulane, ulane ? 1 : 7,
                              err, &fl.hdr[FL_END], fl.epoch, urgent);
    if (desc < 0) break;
    const int n_r = urgent ? d.un_reset : d.n_reset, n_b = urgent ? d.un_bits : d.n_bits;
    const int n_m = urgent ? d.un_marks : d.n_marks, n_s = urgent ? d.un_splat : d.n_splat;
    const int S   = 1 + n_r + n_b + n_m + n_s;  // stage counts per (agent, tick); the agent's stage counter restarts at its head
    unsigned long long *const wq      = urgent ? fl.uw : fl.mw;
    int *const                wq_tail = &fl.hdr[urgent ? FL_UW_TAIL : FL_MW_TAIL];
    __threadfence();
    const long long c1 = wall_clock64();
    if (lane == 0 && c1_prev) {
      atomicAdd(&fl.prof[kind_prev], (unsigned long long)(c0 - c1_prev));  // the previous descriptor's work
      atomicAdd(&fl.prof[8 + kind_prev], 1ull);
    }
    if (lane == 0) atomicAdd(&fl.prof[0], (unsigned long long)(c1 - c0));
    const int          kind = wk_kind(desc), sub = wk_sub(desc), agent = wk_agent(desc);
    c1_prev   = c1;
    kind_prev = kind;
    const int      k = fl.tick_of[agent], kl = k - fl.first_tick;
    const MapFrame frame = flight_frame(d, kl);
    const MarkLog &lg = d.tgt.lg;
    long long     *ts  = fl.ts + (size_t)agent * FL_TS;
    if (kind == WK_MAP_RESET || kind == WK_MAP_BITS) {
      if (kind == WK_MAP_RESET) {
        const unsigned n = lg.n[agent];
        if (sub == 0 && lane == 0 && reset_stat) {
          atomicAdd(reset_stat, (unsigned long long)(n > (unsigned)lg.cap ? (unsigned)lg.cap : n));
          if (agent == 0) atomicAdd(reset_stat + 1, 1ull);
        }
        flight_reset_ticket(reinterpret_cast<char *>(d.tgt.grid) + (size_t)agent * d.agent_bytes, d.agent_bytes,
                            lg.entries + (size_t)agent * lg.cap, n, lg.cap, sub, n_r, lane, reset_stat);
      } else {
        bits_ticket(g, frame, d.tgt, agent, sub, n_b, lane);
      }
      __threadfence();
      if (lane == 0 && atomicAdd(&fl.stage[agent], 1) + 1 == 1 + n_r + n_b) {
        // the grid is clean and the bits are set: the log restarts, then the marks may append
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        lg.n[agent] = 0u;
        ts[13]      = wall_clock64();
        wq_push(wq, wq_tail, wk_pack(WK_MAP_MARKS, 0, agent), n_m);
      }
    } else if (kind == WK_MAP_MARKS) {
      marks_ticket<true>(g, frame, d.tgt, agent, sub, n_m, s_cand, PRESTAMP_CAND_LDS);
      __threadfence();
      if (lane == 0 && atomicAdd(&fl.stage[agent], 1) + 1 == 1 + n_r + n_b + n_m) {
        const long long now = wall_clock64();
        ts[10] = now;
        if (!urgent) atomicAdd(&fl.hdr[FL_MAPS_DONE], 1);  // one more agent may be admitted (a map at the gate holds no worker)
        // the gate of the staleness rule: the overlay reads table ver(k - 2) — every agent must have finished tick k - 2.
        // Early: the overlay is parked, and the finish that completes that tick queues it (k_flight_light).
        const bool open = fl_gate_open(fl, kl);
        if (open) {
          ts[14] = now;
          wq_push(wq, wq_tail, wk_pack(WK_MAP_SPLAT, 0, agent), n_s);
        } else {
          int      *lst  = fl.parked + (size_t)kl * A;
          const int slot = atomicAdd(&fl.parked_n[kl], 1);
          __hip_atomic_store(&lst[slot], agent, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          __threadfence();
          // (the releaser may have scanned the list before this slot was written)
          if (fl_gate_open(fl, kl) && atomicCAS(&lst[slot], agent, -2) == agent) {
            ts[14] = wall_clock64();
            wq_push(wq, wq_tail, wk_pack(WK_MAP_SPLAT, 0, agent), n_s);
          }
        }
      }
    } else {  // WK_MAP_SPLAT: the neighbours' records of table ver(k - 2)
      if (d.tables && d.n_total > 0) {
        OverlayIO ov = d.ov;
        ov.rec       = d.tables + (size_t)((k - fl.lag) & 3) * d.n_total;
        ov.n_rec     = d.n_total;
        ov.stride    = 0;  // the flight's tables are shared: no per-agent views
        overlay_ticket(g, ov, d.tgt, agent, sub, n_s, lane);
      }
      __threadfence();
      if (lane == 0 && atomicAdd(&fl.stage[agent], 1) + 1 == S) {  // the agent's map of tick k is complete
        ts[11] = wall_clock64();
        fl_publish(fl.s_ring, fl.ring_mask, &fl.hdr[FL_S_READY], agent);
      }
    }
  }
}
hipError_t launch_flight_map(const GridGeom &g, const FlightCtl &fl, const FlightMapDev &d, int n_workgroups, hipStream_t st) {
  hipLaunchKernelGGL(k_flight_map, dim3(n_workgroups), dim3(64), 0, st, g, fl, d, d.reset_stat);
  return hipGetLastError();
}

hipError_t launch_prestamp_flow(const GridGeom &g, const FlowCtl &fc, const PrestampDev &ps, int n_workgroups, int n_qp,
                                int n_finish, hipStream_t st) {
  hipLaunchKernelGGL(k_prestamp_gate, dim3(1), dim3(64), 0, st, fc.hdr, ps.gate_agents, n_qp, n_finish);
  hipLaunchKernelGGL(k_prestamp_flow, dim3(n_workgroups), dim3(64), 0, st, g, fc, ps);
  return hipGetLastError();
}

// row length of the stamp's occupancy bitmask (one row per agent): k_stamp_marks reads 256 words per trip
static int stamp_bits_words(const GridGeom &g) { return (((g.V + 31) / 32) + 255) & ~255; }
int map_target(sogm_ctx *c, int slot, bool next_poses, hipStream_t st, MapTarget *out) {
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  const size_t A = (size_t)c->n_agents;
  const int    words = stamp_bits_words(c->geom);
  if (next_poses && !c->d_poses_next) {
    Resources::Setup setup(c->res);
    SOGM_HIP_CHECK(c->res.device(&c->d_poses_next, sizeof(float) * 3 * A));
    SOGM_HIP_CHECK(c->res.device(&c->d_stamps_next, sizeof(double) * A));
    setup.done();
  }
  if (!c->d_cand) {
    Resources::Setup setup(c->res);
    SOGM_HIP_CHECK(c->res.device(&c->d_cand, sizeof(CylCand) * SOGM_MAX_CYL_LDS * A));
    SOGM_HIP_CHECK(c->res.device(&c->d_ncand, sizeof(int) * A));
    SOGM_HIP_CHECK(c->res.device(&c->d_stamp_bits, sizeof(unsigned) * (size_t)words * A));
    SOGM_HIP_CHECK(hipMemsetAsync(c->d_stamp_bits, 0, sizeof(unsigned) * (size_t)words * A, st));
    setup.done();
  }
  *out = MapTarget{.grid = (void *)c->pool.grid_of(slot), .bits = c->d_stamp_bits, .words = words, .cand = c->d_cand,
                   .n_cand = c->d_ncand, .lg = mark_log(c, slot), .poses = next_poses ? c->d_poses_next : c->d_poses,
                   .stamps = next_poses ? c->d_stamps_next : c->d_stamps};
  return SOGM_OK;
}

// Growing stalls the host for as long as the device needs to drain (hipDeviceSynchronize + hipFree + hipMalloc): callers
// reach it before they launch anything of their tick — sogm_update_world / sogm_update_gt_swarm at their top,
// sogm_planner_set_prestamp (so that sogm_replan's own call below never grows), sogm_flight_run before its first launch.
int world_blocks(sogm_ctx *c, const SogmWorld *w, CloudBlocks *out) {
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (w->n_blocks > c->blk_cap || !c->d_blk_n) {  // (also the first frame of all, even an empty one: the counts exist)
    // (grown between ticks only: a frame with more blocks than any before; the old lists may still be read by a
    //  pre-stamp in flight, so everything drains first)
    SOGM_HIP_CHECK(hipDeviceSynchronize());
    c->res.release(&c->d_blk_list);
    c->blk_cap = 0;
    Resources::Setup setup(c->res);
    const int cap = (w->n_blocks + 1023) & ~1023;
    SOGM_HIP_CHECK(c->res.device(&c->d_blk_list, sizeof(int) * (size_t)cap * (size_t)c->n_agents));
    if (!c->d_blk_n) SOGM_HIP_CHECK(c->res.device(&c->d_blk_n, sizeof(int) * (size_t)c->n_agents));
    setup.done();
    c->blk_cap = cap;
  }
  // (rows of blk_cap entries whatever the frame holds: a row never exceeds n_blocks <= blk_cap)
  *out = CloudBlocks{w->block_bounds, w->n_blocks, w->block_points, w->n_points, c->d_blk_list, c->d_blk_n, c->blk_cap};
  return SOGM_OK;
}

// ---- update flow (tuning key update_flow): the maps of a lock-step tick agent by agent ----
// One persistent launch of one-wave workgroups over tickets; an agent's tickets are consecutive (bits, marks, overlay) and
// agents are taken in `order` (the previous tick's longest chains first), so the first agents' maps are complete after the
// latency of ONE ticket chain instead of after four kernels over the whole swarm; the agent's last ticket stores the
// epoch into map_ready[agent] (release), which sogm_replan's search workgroups wait for.  A ticket only ever waits for
// tickets of its own agent, all of which are held by resident or earlier waves: no residency assumption beyond one agent's
// worth of waves.  The four kernels' ticket bodies (bits_ticket, marks_ticket, overlay_ticket): same cells, same log
// (tests/test_update_flow_gpu.py).
struct UpdateFlowDev {
  MapTarget             tgt;      // poses / stamps: the context's copies (filed by k_cull_cylinders, the launch before)
  MapFrame              frame;
  OverlayIO             ov;
  int                   n_agents, n_bits, n_marks, n_splat;
  int                  *ctl;      // ticket, error and per-agent progress words (layout: UpdateBlock, sogm_handover.hpp)
  int                   chunk;    // consecutive tickets per claim
  long long            *ts;       // [A][4] wall clock: first ticket claimed, bits complete, marks complete, map ready (diagnostics)
  int                  *map_ready;
  int                   epoch;
  const int            *order;
};
// (no LDS: the replan's corridor workgroups, resident beside this kernel and waiting for routes, hold every CU's LDS)
template <bool CACHED>
__global__ __launch_bounds__(64) void k_update_flow(GridGeom g, UpdateFlowDev u) {
  const int lane  = threadIdx.x;
  const int per   = u.n_bits + u.n_marks + u.n_splat;
  const int total = u.n_agents * per;
  int      *err   = u.ctl + UpdateBlock::err();
  for (;;) {
    int t0 = 0;
    if (lane == 0) t0 = atomicAdd(&u.ctl[UpdateBlock::ticket()], u.chunk);  // a chunk of consecutive tickets per claim
    t0 = __builtin_amdgcn_readfirstlane(t0);
    if (t0 >= total) break;
    for (int t = t0; t < t0 + u.chunk && t < total; ++t) {
      const int agent = u.order[t / per];
      const int s     = t % per;
      int      *stage = UpdateBlock::stage_word(u.ctl, agent);
      bool      last  = false;
      if (s == 0 && lane == 0) u.ts[agent * 4] = wall_clock64();
      if (s < u.n_bits) {
        bits_ticket(g, u.frame, u.tgt, agent, s, u.n_bits, lane);
        __threadfence();
        if (lane == 0 && atomicAdd(stage, 1) + 1 == u.n_bits) u.ts[agent * 4 + 1] = wall_clock64();
      } else if (s < u.n_bits + u.n_marks) {
        if (flow_wait_count(stage, u.n_bits, err)) return;
        marks_ticket<CACHED>(g, u.frame, u.tgt, agent, s - u.n_bits, u.n_marks);
        __threadfence();
        if (lane == 0) {
          const int n = atomicAdd(stage, 1) + 1;
          last        = n == per;
          if (n == u.n_bits + u.n_marks) u.ts[agent * 4 + 2] = wall_clock64();
        }
      } else {
        if (flow_wait_count(stage, u.n_bits + u.n_marks, err)) return;  // stores of 1.0 first, the additions after them
        overlay_ticket(g, u.ov, u.tgt, agent, s - u.n_bits - u.n_marks, u.n_splat, lane);
        __threadfence();
        if (lane == 0) last = atomicAdd(stage, 1) + 1 == per;
      }
      if (last) {
        u.ts[agent * 4 + 3] = wall_clock64();
        __hip_atomic_store(&u.map_ready[agent], u.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
__global__ void k_iota(int *p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}
// stream, events and words of the update flow (first use)
static int update_flow_setup(sogm_ctx *c) {
  if (c->ustream) return SOGM_OK;
  Resources::Setup setup(c->res);
  const int A = c->n_agents;
  SOGM_HIP_CHECK(c->res.stream(&c->ustream));
  SOGM_HIP_CHECK(c->res.event(&c->ev_uin));
  SOGM_HIP_CHECK(c->res.event(&c->ev_udone));
  SOGM_HIP_CHECK(c->res.device(&c->d_map_ready, sizeof(int) * A, true));
  SOGM_HIP_CHECK(c->res.device(&c->d_update_ctl, sizeof(int) * UpdateBlock::words(A)));
  SOGM_HIP_CHECK(c->res.device(&c->d_update_order, sizeof(int) * A));
  SOGM_HIP_CHECK(c->res.device(&c->d_update_ts, sizeof(long long) * 4 * A, true));
  hipLaunchKernelGGL(k_iota, dim3((A + 255) / 256), dim3(256), 0, nullptr, c->d_update_order, A);
  SOGM_HIP_CHECK(hipGetLastError());
  SOGM_HIP_CHECK(hipStreamSynchronize(nullptr));  // (null-stream work is not ordered with the non-blocking streams)
  return setup.done();
}

// ------------------------------------------------------------------------------------------------
// The lock-step update's host side (sogm_update_gt / _gt_swarm / _world): one function per step, in launch order.
// ------------------------------------------------------------------------------------------------
// The crop lists of a SogmWorld frame (they may grow, which drains the device: before anything of this tick is launched), then
// the caller's stream behind whatever still builds or feeds what this update touches.
static int update_joins(sogm_ctx *c, hipStream_t st, const SogmWorld *world, bool records, CloudBlocks *cb) {
  if (world)
    if (int rc = world_blocks(c, world, cb)) return rc;
  if (int rc = join_update(c, st)) return rc;    // an update flow of the previous tick nobody joined
  if (int rc = join_prestamp(c, st)) return rc;  // a pre-stamp of the last replan may still be running
  if (records)
    if (int rc = join_exchange(c, st)) return rc;  // records may come from an all-gather in flight
  return SOGM_OK;
}
// The grid this update builds into, zero on `st`: the pool's pre-cleared one, or the current one cleared here.
static int take_grid(sogm_ctx *c, hipStream_t st) {
  // A grid the previous replan pre-stamped is not what this call builds (other inputs): it is the front of the ready
  // queue, i.e. the grid adopted below — its marks are in its log, so it is reset again before the stamp.
  const int stale = c->pool.discard_prestamp();
  c->records_final_valid = 0;
  if (c->pool.precleared()) {
    // the grid was already cleared on the side stream during the previous tick
    if (int rc = adopt_preclear(c, st)) return rc;
    if (stale >= 0 && c->pool.current() == stale)
      if (int rc = reset_slot(c, st, stale, c->d_grid, false)) return rc;
    if (stale >= 0 && c->d_stamp_bits) {
      // a pre-stamp that was cut short (a failed tick) may have left occupancy bits behind — only consumed words are
      // zeroed — and they are relative to ITS map centres: start this stamp from a clean mask
      const size_t words = (size_t)stamp_bits_words(c->geom) * (size_t)c->n_agents;
      SOGM_HIP_CHECK(hipMemsetAsync(c->d_stamp_bits, 0, sizeof(unsigned) * words, st));
    }
    return SOGM_OK;
  }
  if (int rc = reset_slot(c, st, c->pool.current(), c->d_grid, false)) return rc;
  // tuning-aid mode: the pool's spare grids (dirty at the start, no readers) are cleared from here on as well,
  // so that a run of updates alone exercises the pooled clear (tools/diag_clear_pmc.py)
  if (c->overlap >= 2 && c->pool.first_dirty() >= 0 && c->clear_gate && c->tune_i(SOGM_TUNE_CLEAR_EARLY))
    return queue_spare_clears_ahead(c, st);
  return SOGM_OK;
}
// Candidate cylinders (and cloud blocks of a SogmWorld frame) per agent; the kernel also files the update's poses and stamps
// into the target's arrays, where the later kernels of the update and the queries read them.
static void launch_cull(sogm_ctx *c, hipStream_t st, const MapFrame &f, const MapTarget &tgt, const float *poses,
                        const double *stamps) {
  hipLaunchKernelGGL(k_cull_cylinders, dim3(c->n_agents), dim3(64), 0, st, c->geom, f.cyl, f.n_cyl, poses, (CylCand *)tgt.cand,
                     tgt.n_cand, stamps, tgt.poses, tgt.stamps, f.cb, c->h_tick_clock);
}
// The maps agent by agent on the flow's stream, behind the cull on `st`; the caller's stream goes on (sogm_replan's searches
// wait per agent, everything else joins the flow's end: join_update).  Closes the stamp's profiling pair on the flow's stream.
static int launch_update_flow(sogm_ctx *c, hipStream_t st, const MapFrame &f, const MapTarget &tgt, const OverlayIO *ov) {
  if (int rc = update_flow_setup(c)) return rc;
  const int           A = c->n_agents;
  const UpdateFlowDev u{.tgt       = tgt,
                        .frame     = f,
                        .ov        = ov ? *ov : OverlayIO{},
                        .n_agents  = A,
                        .n_bits    = c->tune_i(SOGM_TUNE_UPDATE_BITS),
                        .n_marks   = c->tune_i(SOGM_TUNE_UPDATE_MARKS),
                        .n_splat   = ov && ov->n_rec > 0 ? c->tune_i(SOGM_TUNE_UPDATE_SPLAT) : 0,
                        .ctl       = c->d_update_ctl,
                        .chunk     = c->tune_i(SOGM_TUNE_UPDATE_CHUNK) > 0 ? c->tune_i(SOGM_TUNE_UPDATE_CHUNK) : 1,
                        .ts        = c->d_update_ts,
                        .map_ready = c->d_map_ready,
                        .epoch     = ++c->map_epoch,
                        .order     = c->d_update_order};
  int n_cu = 256;
  (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  int       wgs   = c->tune_i(SOGM_TUNE_UPDATE_WGS) > 0 ? c->tune_i(SOGM_TUNE_UPDATE_WGS) : 16 * n_cu;
  const int total = A * (u.n_bits + u.n_marks + u.n_splat);
  if (wgs > total) wgs = total;
  SOGM_HIP_CHECK(hipEventRecord(c->ev_uin, st));
  SOGM_HIP_CHECK(hipStreamWaitEvent(c->ustream, c->ev_uin, 0));
  SOGM_HIP_CHECK(hipMemsetAsync(c->d_update_ctl, 0, sizeof(int) * UpdateBlock::words(A), c->ustream));
  if (c->tune_i(SOGM_TUNE_UPDATE_CACHED))
    hipLaunchKernelGGL(k_update_flow<true>, dim3(wgs), dim3(64), 0, c->ustream, c->geom, u);
  else
    hipLaunchKernelGGL(k_update_flow<false>, dim3(wgs), dim3(64), 0, c->ustream, c->geom, u);
  SOGM_HIP_CHECK(hipGetLastError());
  prof_end(c, SOGM_PROF_STAMP, c->ustream);
  SOGM_HIP_CHECK(hipEventRecord(c->ev_udone, c->ustream));
  c->update_pending = 1;
  return SOGM_OK;
}
// The lock-step stamp: one-wave workgroups stride over each agent's listed blocks or cloud range and set the occupancy bits,
// then over its mask words and write the marks.
static void launch_stamp(sogm_ctx *c, hipStream_t st, const MapFrame &f, const MapTarget &tgt) {
  const int A         = c->n_agents;
  const int stamp_wgs = c->tune_i(SOGM_TUNE_STAMP_WGS) > 0 ? c->tune_i(SOGM_TUNE_STAMP_WGS) : 256;  // one-wave workgroups per agent
  const int bits_wgs  = c->tune_i(SOGM_TUNE_STAMP_BITS_WGS) > 0 ? c->tune_i(SOGM_TUNE_STAMP_BITS_WGS) : stamp_wgs;
  if (f.cb.bounds)
    hipLaunchKernelGGL(k_stamp_bits_blocks, dim3(bits_wgs, A), dim3(64), 0, st, c->geom, f.cloud, f.cb, tgt.poses, tgt.bits,
                       tgt.words);
  else
    hipLaunchKernelGGL(k_stamp_bits, dim3(bits_wgs, A), dim3(64), 0, st, c->geom, f.cloud, f.cloud_range, tgt.poses, tgt.bits,
                       tgt.words, 0);
  // (dynamic LDS the kernel does not use bounds its waves per CU: the marks' scattered stores merge worse in L2 the more
  //  waves interleave theirs — tuning key stamp_lds_kb, 160 / kb workgroups per CU)
  const size_t marks_lds = (size_t)c->tune_i(SOGM_TUNE_STAMP_LDS_KB) * 1024;
  if (c->tune_i(SOGM_TUNE_STAMP_CACHED)) {
    hipLaunchKernelGGL(k_stamp_marks_cached, dim3(stamp_wgs, A), dim3(64), marks_lds, st, c->geom, tgt.grid, tgt.bits,
                       tgt.words, f.cyl, f.n_cyl, tgt.poses, (const CylCand *)tgt.cand, (const int *)tgt.n_cand, 0, tgt.lg);
  } else {
    // the log pass's sector cache: T x 64 words of LDS per (one-wave) workgroup, in front of the tuning aid's padding
    const int    lds_log = tgt.lg.entries && c->spec.T <= 64 && c->tune_i(SOGM_TUNE_STAMP_LDS_LOG) ? 1 : 0;
    const size_t lds     = marks_lds + (lds_log ? sizeof(unsigned) * 64 * (size_t)c->spec.T : 0);
    hipLaunchKernelGGL(k_stamp_marks, dim3(stamp_wgs, A), dim3(64), lds, st, c->geom, tgt.grid, tgt.bits, tgt.words, f.cyl,
                       f.n_cyl, tgt.poses, (const CylCand *)tgt.cand, (const int *)tgt.n_cand, 0, tgt.lg, lds_log);
  }
}
// The neighbours' records of `ov` into the CURRENT grid of every agent: one lane per (agent, record, slice) item, unless
// max_workgroups > 0 narrows the launch (its lanes then stride over the items).  wait_stage / wait_err (or null): the launch
// runs under the tail of the pre-stamp that builds this grid, and every lane waits for its agent's completion word
// (k_splat_neighbours).  The caller has joined whatever writes the grid or the records.
static int launch_overlay(sogm_ctx *c, hipStream_t st, const OverlayIO &ov, const int *wait_stage, int *wait_err,
                          int max_workgroups) {
  const long long total = (long long)c->n_agents * ov.n_rec * c->spec.T;
  long long       nblk  = (total + 255) / 256;
  if (max_workgroups > 0 && nblk > max_workgroups) nblk = max_workgroups;
  prof_begin(c, SOGM_PROF_SPLAT, st);
  hipLaunchKernelGGL(k_splat_neighbours, dim3((unsigned)nblk), dim3(256), 0, st, c->geom, (void *)c->d_grid, ov.rec, ov.n_rec,
                     ov.stride, ov.ego_ids, c->d_poses, c->d_stamps, ov.body, ov.n_body, c->n_agents, 0, mark_log(c, c->pool.current()),
                     wait_stage, wait_err);
  prof_end(c, SOGM_PROF_SPLAT, st);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
// per_agent: `records` is [n_agents][n_records], agent a's own view of the swarm (include/sogm_abi.h "radio links")
static OverlayIO overlay_io(const sogm_ctx *c, const SogmTrajRecord *records, int n_records, const int32_t *ego_ids,
                            bool per_agent = false) {
  return OverlayIO{.rec = records, .n_rec = n_records, .stride = per_agent ? n_records : 0, .ego_ids = ego_ids,
                   .body = c->d_body, .n_body = c->n_body};
}

// updateMap for every agent; with `ov` the neighbour overlay follows in the same call.  `world` (or null): the frame is a
// SogmWorld's — its crop lists are the context's (frame.cb is filled here) and the tuning key update_flow applies.
static int update_maps(sogm_ctx *c, hipStream_t st, MapFrame frame, const SogmWorld *world, const float *poses,
                       const double *stamps, const OverlayIO *ov) {
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = update_joins(c, st, world, ov != nullptr, &frame.cb)) return rc;
  if (int rc = take_grid(c, st)) return rc;
  MapTarget tgt{};
  if (int rc = map_target(c, c->pool.current(), false, st, &tgt)) return rc;
  c->n_stamps++;
  prof_begin(c, SOGM_PROF_STAMP, st);
  launch_cull(c, st, frame, tgt, poses, stamps);
  if (world && c->tune_i(SOGM_TUNE_UPDATE_FLOW) != 0) {
    if (int rc = launch_update_flow(c, st, frame, tgt, ov)) return rc;
  } else {
    launch_stamp(c, st, frame, tgt);
    prof_end(c, SOGM_PROF_STAMP, st);
    SOGM_HIP_CHECK(hipGetLastError());
    if (ov && ov->n_rec > 0)
      if (int rc = launch_overlay(c, st, *ov, nullptr, nullptr, 0)) return rc;
  }
  c->updated = 1;
  return SOGM_OK;
}

}  // namespace sogm

using namespace sogm;

extern "C" {

int sogm_update_gt(sogm_ctx *c, const float *cloud_xyz, const int32_t *cloud_range,
                   const SogmCylinder *cylinders, int n_cyl, const float *poses,
                   const double *stamps, void *stream) {
  if (!c || !cloud_xyz || !cloud_range || !poses || !stamps || n_cyl < 0 ||
      (n_cyl > 0 && !cylinders))
    return SOGM_ERR_INVALID_ARG;
  const MapFrame frame{.cloud = cloud_xyz, .cloud_range = cloud_range, .cb = {}, .cyl = cylinders, .n_cyl = n_cyl};
  return update_maps(c, (hipStream_t)stream, frame, nullptr, poses, stamps, nullptr);
}

int sogm_update_gt_swarm(sogm_ctx *c, const float *cloud_xyz, const int32_t *cloud_range,
                         const SogmCylinder *cylinders, int n_cyl, const float *poses, const double *stamps,
                         const SogmTrajRecord *records, int n_records, const int32_t *ego_ids, void *stream) {
  if (!c || !cloud_xyz || !cloud_range || !poses || !stamps || n_cyl < 0 || (n_cyl > 0 && !cylinders) ||
      n_records < 0 || (n_records > 0 && !records) || !ego_ids)
    return SOGM_ERR_INVALID_ARG;
  if (!c->d_body || c->n_body <= 0) return SOGM_ERR_STATE;
  const MapFrame  frame{.cloud = cloud_xyz, .cloud_range = cloud_range, .cb = {}, .cyl = cylinders, .n_cyl = n_cyl};
  const OverlayIO ov = overlay_io(c, records, n_records, ego_ids);
  return update_maps(c, (hipStream_t)stream, frame, nullptr, poses, stamps, &ov);
}

// sogm_update_world / _views: `records` is the one table [n_records], or per_agent the agents' views [n_agents][n_records]
static int update_world(sogm_ctx *c, const SogmWorld *w, const float *poses, const double *stamps,
                        const SogmTrajRecord *records, int n_records, const int32_t *ego_ids, bool per_agent, void *stream) {
  if (!c || !w || !poses || !stamps || !w->cloud_xyz || !w->block_bounds || w->n_points < 0 || w->block_points < 64 ||
      w->block_points > 4096 || w->n_blocks != (w->n_points + w->block_points - 1) / w->block_points || w->n_cyl < 0 ||
      (w->n_cyl > 0 && !w->cylinders) || n_records < 0 || (n_records > 0 && (!records || !ego_ids)))
    return SOGM_ERR_INVALID_ARG;
  if (n_records > 0 && (!c->d_body || c->n_body <= 0)) return SOGM_ERR_STATE;
  // (cb: the context's crop lists, sized for this frame inside the update)
  const MapFrame  frame{.cloud = w->cloud_xyz, .cloud_range = nullptr, .cb = {}, .cyl = w->cylinders, .n_cyl = w->n_cyl};
  const OverlayIO ov = overlay_io(c, records, n_records, ego_ids, per_agent);
  return update_maps(c, (hipStream_t)stream, frame, w, poses, stamps, n_records > 0 ? &ov : nullptr);
}
int sogm_update_world(sogm_ctx *c, const SogmWorld *w, const float *poses, const double *stamps,
                      const SogmTrajRecord *records, int n_records, const int32_t *ego_ids, void *stream) {
  return update_world(c, w, poses, stamps, records, n_records, ego_ids, false, stream);
}
int sogm_update_world_views(sogm_ctx *c, const SogmWorld *w, const float *poses, const double *stamps,
                            const SogmTrajRecord *views, int n_records, const int32_t *ego_ids, void *stream) {
  return update_world(c, w, poses, stamps, views, n_records, ego_ids, true, stream);
}

int sogm_update_prestamped(sogm_ctx *c, const SogmTrajRecord *records, int n_records, const int32_t *ego_ids,
                           void *stream) {
  if (!c || n_records < 0 || (n_records > 0 && (!records || !ego_ids))) return SOGM_ERR_INVALID_ARG;
  if (!c->pool.front_is_prestamped()) {
    sogm::set_error_text("sogm_update_prestamped: the previous sogm_replan did not pre-stamp the next grid");
    return SOGM_ERR_STATE;
  }
  if (n_records > 0 && (!c->d_body || c->n_body <= 0)) return SOGM_ERR_STATE;
  if (c->ps_fail_host && c->ps_fail_host[1] != c->ps_fail_seen) {
    sogm::set_error_text("sogm_update_prestamped: the replan that pre-stamped this grid failed on the device "
                         "(sogm_planner_flow_failures); build the map with sogm_update_gt[_swarm] instead");
    return SOGM_ERR_STATE;
  }
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = sogm::join_update(c, st)) return rc;
  if (n_records > 0)
    if (int rc = sogm::join_exchange(c, st)) return rc;  // records may come from an all-gather in flight
  if (int rc = sogm::adopt_preclear(c, st, false)) return rc;  // the pre-stamped grid becomes the current one
  c->records_final_valid = 0;
  std::swap(c->d_poses, c->d_poses_next);                // its map centres and stamps with it
  std::swap(c->d_stamps, c->d_stamps_next);
  c->pool.adopted_prestamped();
  if (n_records > 0) {
    // The replan that pre-stamped this grid left the caller's stream behind its fan-in, not behind the pre-stamp's
    // end: the overlay is launched now, narrow, and waits per agent for the stamp's completion word — it runs under the
    // pre-stamp's tail (the last agents' stamps, the report) instead of after it.
    // (a pre-stamp that has ended already — a host that synchronises every tick — needs no waiting: full width)
    if (c->pdone_pending && hipEventQuery(c->ev_pdone) == hipSuccess)
      if (int rc = sogm::join_prestamp(c, st)) return rc;
    (void)hipGetLastError();  // (hipErrorNotReady is not an error here)
    const int *stage = c->pdone_pending ? c->ps_stage : nullptr;
    // workgroups of the waiting launch (128 / 256 / 512 / 2048: 11.22 / 11.25 / 11.31 / 11.26 ms per tick)
    const int cap = c->tune_i(SOGM_TUNE_SPLAT_WGS) > 0 ? c->tune_i(SOGM_TUNE_SPLAT_WGS) : 256;
    if (int rc = launch_overlay(c, st, overlay_io(c, records, n_records, ego_ids), stage, c->ps_err, stage ? cap : 0)) return rc;
  }
  if (int rc = sogm::join_prestamp(c, st)) return rc;  // whatever follows is behind the pre-stamp's end
  if (int rc = sogm::retire_wide_clear(c, st)) return rc;
  c->updated = 1;
  return SOGM_OK;
}

static int project_neighbours(sogm_ctx *c, const SogmTrajRecord *records, int n_records, const int32_t *ego_ids,
                              bool per_agent, void *stream) {
  if (!c || n_records < 0 || (n_records > 0 && !records) || !ego_ids) return SOGM_ERR_INVALID_ARG;
  if (!c->updated) return SOGM_ERR_STATE;
  if (!c->d_body || c->n_body <= 0) return SOGM_ERR_STATE;
  if (n_records == 0) return SOGM_OK;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = sogm::join_update(c, (hipStream_t)stream)) return rc;
  if (int rc = sogm::join_exchange(c, (hipStream_t)stream)) return rc;  // records may come from an all-gather in flight
  return launch_overlay(c, (hipStream_t)stream, overlay_io(c, records, n_records, ego_ids, per_agent), nullptr, nullptr, 0);
}
int sogm_project_neighbours(sogm_ctx *c, const SogmTrajRecord *records, int n_records,
                            const int32_t *ego_ids, void *stream) {
  return project_neighbours(c, records, n_records, ego_ids, false, stream);
}
int sogm_project_neighbours_views(sogm_ctx *c, const SogmTrajRecord *views, int n_records, const int32_t *ego_ids,
                                  void *stream) {
  return project_neighbours(c, views, n_records, ego_ids, true, stream);
}

int sogm_cloud_block_bounds(const float *cloud_xyz, int n_points, int block_points, float *out_bounds, void *stream) {
  if (!cloud_xyz || !out_bounds || n_points < 0 || block_points < 64 || block_points > 4096) return SOGM_ERR_INVALID_ARG;
  const int nb = (n_points + block_points - 1) / block_points;
  if (nb == 0) return SOGM_OK;
  hipLaunchKernelGGL(k_block_bounds, dim3(nb), dim3(64), 0, (hipStream_t)stream, cloud_xyz, n_points, block_points, out_bounds);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_prestamp_pending(const sogm_ctx *c) { return c && c->pool.prestamp_pending() ? 1 : 0; }
int sogm_prestamp_join(sogm_ctx *c, void *stream) {
  if (!c) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  return sogm::join_prestamp(c, (hipStream_t)stream);
}

// diagnostics (tools/ only): the update flow's control words after a device synchronisation —
// out = {epoch, pending, ticket, error, ...ctl[2..7], stage[A], map_ready[A]}
int sogm_debug_update_flow(sogm_ctx *c, int32_t *out, int cap) {
  if (!c || !out || cap < 10 + 2 * c->n_agents) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  (void)hipDeviceSynchronize();
  const int A = c->n_agents;
  out[0]      = c->map_epoch;
  out[1]      = c->update_pending;
  if (!c->d_update_ctl) return SOGM_ERR_STATE;
  {
    std::vector<int> w(UpdateBlock::words(A));
    SOGM_HIP_CHECK(hipMemcpy(w.data(), c->d_update_ctl, sizeof(int) * w.size(), hipMemcpyDeviceToHost));
    out[2] = w[UpdateBlock::ticket()];
    out[3] = w[UpdateBlock::err()];
    for (int a = 0; a < A; ++a) out[10 + a] = w[(size_t)UpdateBlock::stage(a)];
  }
  SOGM_HIP_CHECK(hipMemcpy(out + 10 + A, c->d_map_ready, sizeof(int) * A, hipMemcpyDeviceToHost));
  return SOGM_OK;
}
// ... and its per-agent stamps [A][4] (100 MHz wall clock) + the order it took the agents in [A]
int sogm_debug_update_flow_times(sogm_ctx *c, int64_t *out_ts, int32_t *out_order) {
  if (!c || !out_ts || !out_order || !c->d_update_ts) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  (void)hipDeviceSynchronize();
  SOGM_HIP_CHECK(hipMemcpy(out_ts, c->d_update_ts, sizeof(long long) * 4 * c->n_agents, hipMemcpyDeviceToHost));
  SOGM_HIP_CHECK(hipMemcpy(out_order, c->d_update_order, sizeof(int) * c->n_agents, hipMemcpyDeviceToHost));
  return SOGM_OK;
}

}  // extern "C"
