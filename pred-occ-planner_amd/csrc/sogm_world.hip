// World timeline (include/sogm_abi.h "world timeline"): the SogmWorld frames of a range of ticks — moved cloud, block bounds,
// obstacle records — written from the tick-0 world.  The rules are sogm_world.hpp's; this file is the launch:
//   k_world_frames  grid (x, tick).  The first cloud_wgs workgroups of a tick own whole blocks of block_points points,
//                   blocks_per_wg consecutive blocks each (about 2048 points).  Per block the 256 lanes read the block's
//                   floats once as 16-byte pieces — a piece's four floats straddle points: float F has component F % 3 of
//                   point F / 3 — with the (at most two) owners a piece needs, store the moved piece, and keep the xy
//                   bounds of what they stored; the bounds are reduced with wave shuffles, then across the four waves
//                   through LDS (two sets of slots, taken in turn: one barrier per block), no atomics.  Floats before the
//                   block's first 16-byte boundary and after its last whole piece (a block starts at float 3*b*block_points,
//                   off a boundary whenever that is no multiple of 4 or the buffers are not aligned; the cloud ends where
//                   n_points*3 does) go one float per lane; so does the whole block when the input and the output are not
//                   equally aligned.  The remaining workgroups of the tick write its records, one per lane.
// No workgroup waits for another; every loop is bounded by a validated argument.  The frames' pointers travel in the kernel
// arguments (no staging buffer, no allocation): WORLD_FRAMES ticks per launch, longer calls take further launches.
#include "sogm_device.hpp"
#include "sogm_world.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

namespace sogm {
namespace {

constexpr int WORLD_WG        = 256;   // lanes per workgroup
constexpr int WORLD_WG_POINTS = 2048;  // a workgroup's share of a frame: max(1, 2048 / block_points) blocks
constexpr int WORLD_FRAMES    = 128;   // ticks per launch (3 pointers each: the argument block stays under 4 KiB)

struct WorldFrameOut {
  float        *cloud, *bounds;
  SogmCylinder *cyl;
};
struct WorldArgs {
  const float        *cloud0;
  const int32_t      *owner;
  const SogmCylinder *cyl0;
  int                 n_points, n_cyl, block_points, moving;
  int                 n_blocks, blocks_per_wg, cloud_wgs, first_tick;
  double              dt;
  WorldFrameOut       out[WORLD_FRAMES];
};
static_assert(sizeof(WorldArgs) <= 4096, "kernel arguments");

struct XyBounds {
  float xlo, xhi, ylo, yhi;
};
// (fminf / fmaxf as k_block_bounds takes them: a NaN is passed over)
// (selects, not branches on comp: the four values stay in registers; min with +inf / max with -inf changes nothing)
__device__ inline void bounds_take(XyBounds &b, int comp, float v) {
  b.xlo = fminf(b.xlo, comp == 0 ? v : INFINITY);
  b.xhi = fmaxf(b.xhi, comp == 0 ? v : -INFINITY);
  b.ylo = fminf(b.ylo, comp == 1 ? v : INFINITY);
  b.yhi = fmaxf(b.yhi, comp == 1 ? v : -INFINITY);
}

__global__ __launch_bounds__(WORLD_WG) void k_world_frames(WorldArgs g) {
  __shared__ float s_red[2][WORLD_WG / 64][4];

  const int    tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int    k     = g.first_tick + (int)blockIdx.y;
  const bool   still = world_still(k, g.moving);
  const double t     = world_tick_time(k, g.dt);
  const WorldFrameOut o = g.out[blockIdx.y];

  if ((int)blockIdx.x >= g.cloud_wgs) {  // the tick's records
    const int i = ((int)blockIdx.x - g.cloud_wgs) * WORLD_WG + tid;
    if (i < g.n_cyl) o.cyl[i] = world_record_at(g.cyl0[i], still, t);
    return;
  }

  const float *__restrict__ in  = g.cloud0;
  float *__restrict__       out = o.cloud;
  // float index F is on a 16-byte boundary of both buffers when (F + mis) % 4 == 0 — if they are equally misaligned
  const unsigned mis  = (unsigned)((uintptr_t)in >> 2) & 3u;
  const bool     wide = mis == ((unsigned)((uintptr_t)out >> 2) & 3u);

  // one float of the cloud: component F % 3 of point F / 3
  auto one = [&](long long F, XyBounds &bb) {
    const long long p    = F / 3;
    const int       comp = (int)(F - p * 3);
    const int32_t   ow   = (still || comp == 2) ? -1 : g.owner[p];
    const float     r    = world_coord_at(in[F], comp, ow, g.cyl0, g.n_cyl, still, t);
    bounds_take(bb, comp, r);
    out[F] = r;
  };

  for (int i = 0; i < g.blocks_per_wg; ++i) {
    const int b = (int)blockIdx.x * g.blocks_per_wg + i;
    if (b >= g.n_blocks) break;  // (uniform)
    const long long beg = (long long)b * g.block_points;
    const long long end = beg + g.block_points < g.n_points ? beg + g.block_points : g.n_points;
    const long long f0 = beg * 3, f1 = end * 3;
    // [f0, a0) one float per lane, [a0, a0 + 4 nq) 16-byte pieces, [a0 + 4 nq, f1) one float per lane
    long long a0 = f1, nq = 0;
    if (wide) {
      a0 = f0 + ((4 - (int)((f0 + mis) & 3)) & 3);
      if (a0 > f1) a0 = f1;
      nq = (f1 - a0) >> 2;
    }
    XyBounds bb{INFINITY, -INFINITY, INFINITY, -INFINITY};

    for (long long F = f0 + tid; F < a0; F += WORLD_WG) one(F, bb);
    for (long long q = tid; q < nq; q += WORLD_WG) {
      const long long F  = a0 + 4 * q;
      const long long p0 = F / 3;
      const int       c0 = (int)(F - p0 * 3);
      const vfloat4   v  = *reinterpret_cast<const vfloat4 *>(in + F);
      // the piece holds components c0.. of point p0 and then 0.. of point p0 + 1 (its last float is that point's: p0 + 1 < end);
      // p0's owner is needed for its x or y only
      int32_t ow0 = -1, ow1 = -1;
      if (!still) {
        if (c0 <= 1) ow0 = g.owner[p0];
        ow1 = g.owner[p0 + 1];
      }
      vfloat4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int cj = c0 + j, comp = cj >= 3 ? cj - 3 : cj;
        w[j] = world_coord_at(v[j], comp, cj >= 3 ? ow1 : ow0, g.cyl0, g.n_cyl, still, t);
        bounds_take(bb, comp, w[j]);
      }
      *reinterpret_cast<vfloat4 *>(out + F) = w;
    }
    for (long long F = a0 + 4 * nq + tid; F < f1; F += WORLD_WG) one(F, bb);

#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      bb.xlo = fminf(bb.xlo, __shfl_xor(bb.xlo, d, 64));
      bb.xhi = fmaxf(bb.xhi, __shfl_xor(bb.xhi, d, 64));
      bb.ylo = fminf(bb.ylo, __shfl_xor(bb.ylo, d, 64));
      bb.yhi = fmaxf(bb.yhi, __shfl_xor(bb.yhi, d, 64));
    }
    // slots i & 1: lane 0 of the workgroup reads block i's while the waves may already write block i + 1's; block i + 2's are
    // written behind block i + 1's barrier, which lane 0 reaches after this read
    float(*red)[4] = s_red[i & 1];
    if (lane == 0) {
      red[wave][0] = bb.xlo;
      red[wave][1] = bb.xhi;
      red[wave][2] = bb.ylo;
      red[wave][3] = bb.yhi;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < WORLD_WG / 64; ++w) {
        bb.xlo = fminf(bb.xlo, red[w][0]);
        bb.xhi = fmaxf(bb.xhi, red[w][1]);
        bb.ylo = fminf(bb.ylo, red[w][2]);
        bb.yhi = fmaxf(bb.yhi, red[w][3]);
      }
      float *ob = o.bounds + (size_t)b * 4;
      ob[0] = bb.xlo;
      ob[1] = bb.xhi;
      ob[2] = bb.ylo;
      ob[3] = bb.yhi;
    }
  }
}

int world_refuse(const char *what, int frame = -1) {
  char buf[256];
  if (frame >= 0)
    std::snprintf(buf, sizeof(buf), "sogm_world_frames: frame %d: %s", frame, what);
  else
    std::snprintf(buf, sizeof(buf), "sogm_world_frames: %s", what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_world_frames(const SogmWorldTimeline *tl, int first_tick, int n_ticks, const SogmWorld *frames,
                                 void *stream) {
  using namespace sogm;
  if (!tl || !frames) return world_refuse("null tl or frames");
  if (tl->n_points < 0 || tl->n_cyl < 0) return world_refuse("n_points < 0 or n_cyl < 0");
  if (tl->n_points > 0 && (!tl->cloud0 || !tl->owner)) return world_refuse("null cloud0 or owner with n_points > 0");
  if (tl->n_cyl > 0 && !tl->cylinders0) return world_refuse("null cylinders0 with n_cyl > 0");
  if (tl->block_points < 64 || tl->block_points > 4096) return world_refuse("block_points outside 64..4096");
  if (!std::isfinite(tl->dt) || !(tl->dt > 0)) return world_refuse("dt must be finite and positive");
  if (first_tick < 0 || n_ticks < 1) return world_refuse("first_tick < 0 or n_ticks < 1");
  if ((long long)first_tick + n_ticks > 2147483647LL) return world_refuse("first_tick + n_ticks overflows int");
  const int n_blocks = (int)(((long long)tl->n_points + tl->block_points - 1) / tl->block_points);
  std::vector<const void *> written;
  written.reserve((size_t)n_ticks * 3);
  for (int i = 0; i < n_ticks; ++i) {
    const SogmWorld &w = frames[i];
    if (w.n_points != tl->n_points || w.n_blocks != n_blocks || w.block_points != tl->block_points || w.n_cyl != tl->n_cyl)
      return world_refuse("n_points, n_blocks, block_points or n_cyl differs from the timeline's", i);
    if (tl->n_points > 0 && (!w.cloud_xyz || !w.block_bounds)) return world_refuse("null cloud_xyz or block_bounds", i);
    if (tl->n_cyl > 0 && !w.cylinders) return world_refuse("null cylinders", i);
    if (tl->n_points > 0) {
      written.push_back(w.cloud_xyz);
      written.push_back(w.block_bounds);
    }
    if (tl->n_cyl > 0) written.push_back(w.cylinders);
  }
  std::sort(written.begin(), written.end());
  if (std::adjacent_find(written.begin(), written.end()) != written.end())
    return world_refuse("two frame buffers of the call are the same buffer");
  for (const void *in : {(const void *)tl->cloud0, (const void *)tl->owner, (const void *)tl->cylinders0})
    if (in && std::binary_search(written.begin(), written.end(), in))
      return world_refuse("a frame buffer is one of the timeline's inputs");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    set_error_text("sogm_world_frames: no HIP device");
    return SOGM_ERR_NO_DEVICE;
  }
  WorldArgs g{};
  g.cloud0        = tl->cloud0;
  g.owner         = tl->owner;
  g.cyl0          = tl->cylinders0;
  g.n_points      = tl->n_points;
  g.n_cyl         = tl->n_cyl;
  g.block_points  = tl->block_points;
  g.moving        = tl->moving;
  g.dt            = tl->dt;
  g.n_blocks      = n_blocks;
  g.blocks_per_wg = std::max(1, WORLD_WG_POINTS / tl->block_points);
  g.cloud_wgs     = (n_blocks + g.blocks_per_wg - 1) / g.blocks_per_wg;
  const int wgs   = g.cloud_wgs + (tl->n_cyl + WORLD_WG - 1) / WORLD_WG;
  if (wgs == 0) return SOGM_OK;  // an empty world
  for (int i0 = 0; i0 < n_ticks; i0 += WORLD_FRAMES) {
    const int n  = std::min(WORLD_FRAMES, n_ticks - i0);
    g.first_tick = first_tick + i0;
    for (int i = 0; i < n; ++i) {
      const SogmWorld &w = frames[i0 + i];
      g.out[i] = WorldFrameOut{const_cast<float *>(w.cloud_xyz), const_cast<float *>(w.block_bounds),
                               const_cast<SogmCylinder *>(w.cylinders)};
    }
    hipLaunchKernelGGL(k_world_frames, dim3((unsigned)wgs, (unsigned)n), dim3(WORLD_WG), 0, (hipStream_t)stream, g);
    SOGM_HIP_CHECK(hipGetLastError());
  }
  return SOGM_OK;
}
