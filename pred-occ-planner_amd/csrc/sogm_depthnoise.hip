// Sensor-noise pass over rendered depth frames (include/sogm_abi.h "sensor noise"; the per-pixel rule is
// sogm_depthnoise.hpp's, shared with the host).  One launch behind a stream-ordered clear of the counters:
//   k_depth_noise   a workgroup of 256 lanes owns a tile of NOISE_TH x NOISE_TW = 16 x 64 pixels of one agent.  It loads the
//                   tile and a one-pixel halo of in_depth into LDS — 32-bit words, two pixels per lane and load, wherever the
//                   word lies wholly inside the image buffer; single pixels at the buffer's two ends — and then wave w takes
//                   the tile's rows w, w + 4, ...: one pixel per lane, the 3 x 3 test from LDS, so that a wave's stores are
//                   one contiguous run each: 128 B of image, 768 B of cloud, 256 B of hit.
//                   The six counters: a ballot per outcome and row, summed by lane 0 of each wave, one LDS add per wave and
//                   counter, one global integer add per workgroup and counter (none for a zero).
// Halo pixels outside the image are never read from LDS: noise_is_edge skips them by their coordinates.
#include "sogm_device.hpp"
#include "sogm_depthnoise.hpp"

#include <cmath>
#include <cstdio>

namespace sogm {
namespace {

constexpr int NOISE_WG    = 256;
constexpr int NOISE_TW    = 64;                // tile width: one wave per row
constexpr int NOISE_TH    = 16;                // tile height: four rows per wave
constexpr int NOISE_LW    = NOISE_TW + 2;      // with the halo
constexpr int NOISE_LH    = NOISE_TH + 2;
constexpr int NOISE_PITCH = NOISE_LW + 2;      // 68 uint16: rows start on 8-byte boundaries
constexpr int NOISE_WORDS = NOISE_LW / 2 + 1;  // 32-bit words that can cover a halo row of 66 pixels at either parity

struct NoiseArgs {
  SogmDepthCamera cam;
  SogmDepthNoise  prm;
  const uint16_t *in_depth;
  const int32_t  *in_hit;
  uint16_t       *out_depth;
  float          *out_cloud;
  int32_t        *out_hit;
  int32_t        *out_counts;
  uint64_t        frame_key;  // mix(mix(seed) ^ frame)
  long long       n_px;       // n_agents * rows * cols: the image buffer's length
  int             tiles_x, tiles_per_agent;
};

__global__ __launch_bounds__(NOISE_WG) void k_depth_noise(NoiseArgs g) {
  __shared__ uint16_t s_px[NOISE_LH * NOISE_PITCH];
  __shared__ int      s_cnt[6];

  const SogmDepthCamera &cam = g.cam;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int agent = blockIdx.x / g.tiles_per_agent, tile = blockIdx.x - agent * g.tiles_per_agent;
  const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
  const int v0 = ty * NOISE_TH, u0 = tx * NOISE_TW;
  if (tid < 6) s_cnt[tid] = 0;

  // the tile and its halo: LDS (r, c) is pixel (v0 - 1 + r, u0 - 1 + c).  Words are those of the ADDRESS: pixel e of the
  // buffer sits in word (e + odd) >> 1, where odd says that the buffer starts in the upper half of a word.
  const int       odd  = (int)(((uintptr_t)g.in_depth >> 1) & 1);
  const uint32_t *base = reinterpret_cast<const uint32_t *>(g.in_depth - odd);
  const int       c_lo = max(u0 - 1, 0), c_hi = min(u0 + NOISE_TW, cam.cols - 1);  // the columns that exist
  for (int i = tid; i < NOISE_LH * NOISE_WORDS; i += NOISE_WG) {
    const int r = i / NOISE_WORDS, k = i - r * NOISE_WORDS;
    const int v = v0 - 1 + r;
    if (v < 0 || v >= cam.rows) continue;
    const long long row = ((long long)agent * cam.rows + v) * (long long)cam.cols;  // the row's first pixel in the buffer
    const long long w   = ((row + c_lo + odd) >> 1) + k;                              // this lane's word
    const long long e0  = 2 * w - odd;                                                // its lower pixel
    if (e0 > row + c_hi) continue;
    if (e0 >= 0 && e0 + 1 < g.n_px) {
      const uint32_t two = base[w];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long long c = e0 + j - row;
        if (c >= c_lo && c <= c_hi) s_px[r * NOISE_PITCH + (int)(c - (u0 - 1))] = (uint16_t)(two >> (16 * j));
      }
    } else {  // a word that reaches past either end of the buffer: its pixels one by one
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long long e = e0 + j, c = e - row;
        if (e >= 0 && e < g.n_px && c >= c_lo && c <= c_hi) s_px[r * NOISE_PITCH + (int)(c - (u0 - 1))] = g.in_depth[e];
      }
    }
  }
  __syncthreads();

  const int u    = u0 + lane;
  int       n[6] = {0, 0, 0, 0, 0, 0};  // lane 0's sums over the wave's rows
  for (int r = wave; r < NOISE_TH; r += NOISE_WG / 64) {
    const int v = v0 + r;
    if (v >= cam.rows) break;  // (uniform in the wave)
    const bool live = u < cam.cols;
    int        outcome = NOISE_NO_INPUT;
    if (live) {
      const uint16_t d16 = s_px[(r + 1) * NOISE_PITCH + lane + 1];
      const uint64_t h   = noise_pixel_key(g.frame_key, noise_pixel_index(g.prm.agent_base, agent, cam.rows, cam.cols, v, u));
      auto fetch = [&](int vn, int un) { return s_px[(vn - (v0 - 1)) * NOISE_PITCH + (un - (u0 - 1))]; };
      auto edge  = [&]() { return noise_is_edge(fetch, v, u, cam.rows, cam.cols, d16, cam.depth_scale, g.prm.edge_jump); };
      uint16_t out;
      outcome = noise_pixel(cam, g.prm, h, d16, edge, out);
      const size_t pix = ((size_t)agent * cam.rows + v) * (size_t)cam.cols + u;
      g.out_depth[pix] = out;
      if (g.out_cloud) {
        float xyz[3];
        noise_backproject(cam, v, u, out, xyz);
        float *cp = g.out_cloud + pix * 3;
        cp[0]     = xyz[0];
        cp[1]     = xyz[1];
        cp[2]     = xyz[2];
      }
      if (g.out_hit) g.out_hit[pix] = out ? g.in_hit[pix] : SOGM_HIT_NONE;
    }
#pragma unroll
    for (int k = 1; k <= 5; ++k) n[k] += __popcll(__ballot(outcome == k));
  }
  if (lane == 0) {
    n[0] = n[1] + n[2] + n[3] + n[4] + n[5];  // returns_in: every pixel with a return has exactly one outcome
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (n[k]) atomicAdd(&s_cnt[k], n[k]);
  }
  __syncthreads();
  if (tid < 6 && s_cnt[tid]) atomicAdd(&g.out_counts[(size_t)agent * 6 + tid], s_cnt[tid]);
}

int noise_refuse(const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "sogm_depth_noise: %s", what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_depth_noise(const SogmDepthCamera *cam, const SogmDepthNoise *noise, int n_agents, const uint16_t *in_depth,
                                const int32_t *in_hit, uint16_t *out_depth, float *out_cloud_xyz, int32_t *out_hit,
                                int32_t *out_counts, void *stream) {
  using namespace sogm;
  if (!cam || !noise || !in_depth || !out_depth || !out_counts) return noise_refuse("null pointer");
  // the camera refusals of sogm_render_depth
  if (cam->rows < 1 || cam->cols < 1 || n_agents < 1) return noise_refuse("rows, cols and n_agents must be >= 1");
  if (!(cam->fx > 0) || !(cam->fy > 0) || !(cam->max_depth > 0) || !(cam->depth_scale > 0))
    return noise_refuse("fx, fy, max_depth and depth_scale must be positive");
  if (!(cam->max_depth * cam->depth_scale <= 65535.0)) return noise_refuse("max_depth * depth_scale exceeds 65535");
  if (!std::isfinite(cam->cx) || !std::isfinite(cam->cy) || !std::isfinite(cam->fx) || !std::isfinite(cam->fy) ||
      (cam->use_ground && !std::isfinite(cam->ground_z)))
    return noise_refuse("intrinsics and ground_z must be finite");
  const long long tiles_x = (cam->cols + NOISE_TW - 1) / NOISE_TW, tiles_y = (cam->rows + NOISE_TH - 1) / NOISE_TH;
  if ((long long)cam->rows * cam->cols > 2147483647LL || tiles_x * tiles_y * n_agents > 2147483647LL)
    return noise_refuse("image or batch too large for one launch");
  if (out_hit && !in_hit) return noise_refuse("out_hit without in_hit");
  const double prm[7] = {noise->sigma0, noise->sigma1, noise->sigma2, noise->p_drop, noise->edge_jump, noise->p_edge,
                         noise->min_depth};
  for (double x : prm)
    if (!std::isfinite(x)) return noise_refuse("parameters must be finite");
  if (noise->sigma0 < 0 || noise->sigma1 < 0 || noise->sigma2 < 0 || noise->edge_jump < 0 || noise->min_depth < 0)
    return noise_refuse("sigma0, sigma1, sigma2, edge_jump and min_depth must be >= 0");
  if (noise->p_drop < 0 || noise->p_drop > 1 || noise->p_edge < 0 || noise->p_edge > 1)
    return noise_refuse("p_drop and p_edge must be in [0, 1]");
  if (noise->agent_base < 0) return noise_refuse("agent_base must be >= 0");
  const long long n_px = (long long)n_agents * cam->rows * cam->cols;
  {
    const uintptr_t a = (uintptr_t)in_depth, b = (uintptr_t)out_depth, len = (uintptr_t)n_px * 2;
    if (a < b + len && b < a + len) return noise_refuse("out_depth overlaps in_depth (the pass is not in place)");
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    set_error_text("sogm_depth_noise: no HIP device");
    return SOGM_ERR_NO_DEVICE;
  }
  NoiseArgs g{};
  g.cam             = *cam;
  g.prm             = *noise;
  g.in_depth        = in_depth;
  g.in_hit          = in_hit;
  g.out_depth       = out_depth;
  g.out_cloud       = out_cloud_xyz;
  g.out_hit         = out_hit;
  g.out_counts      = out_counts;
  g.frame_key       = noise_frame_key(noise->seed, noise->frame);
  g.n_px            = n_px;
  g.tiles_x         = (int)tiles_x;
  g.tiles_per_agent = (int)(tiles_x * tiles_y);
  hipStream_t st = (hipStream_t)stream;
  SOGM_HIP_CHECK(hipMemsetAsync(out_counts, 0, (size_t)n_agents * 6 * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_depth_noise, dim3((unsigned)(tiles_x * tiles_y * n_agents)), dim3(NOISE_WG), 0, st, g);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
