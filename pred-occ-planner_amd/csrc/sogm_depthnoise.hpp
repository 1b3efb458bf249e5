// sogm_depthnoise.hpp — the depth camera's sensor-noise pass (include/sogm_abi.h "sensor noise" is the definition), the
// per-pixel rule written ONCE for the host and the device:
//   noise_mix                      splitmix64's step
//   noise_frame_key / noise_pixel_key   h = mix(mix(mix(seed) ^ frame) ^ g) in two halves (the first is per call)
//   noise_draw / noise_uniform / noise_normal   w_k = mix(h + k), U(w), the twelve-piece Irwin-Hall n
//   noise_is_edge                  the 3 x 3 test on the INPUT image, through a fetch(v, u) the caller gives
//   noise_pixel                    steps 1-6: the outgoing d16 and which counter the pixel adds to
//   noise_backproject              step 7: the camera's cloud point of a d16
// k_depth_noise of sogm_depthnoise.hip calls these bodies; a host program compiles them as well
// (tests/depth_noise_rules_host_test.cpp).  Every fp64 expression is a single IEEE operation: with -ffp-contract=off host and
// device give the same bits.  Known answers: noise_mix(0) = 0xE220A8397B1DCDAF; seed 0x5067, frame 3, g 0:
// h = 0x52E3CB0B7BF29351, S = 436624, n = 0x1.532cp-1.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_NOISE_HD __host__ __device__
#else
#define SOGM_NOISE_HD
#endif

#include "../../include/sogm_abi.h"

namespace sogm {

// what a pixel adds to: its index into out_counts[a*6 + .] besides returns_in (0), which every pixel with a return adds to
enum NoiseOutcome {
  NOISE_NO_INPUT     = -1,  // d16 == 0: nothing is counted
  NOISE_DROP_UNIFORM = 1,
  NOISE_DROP_EDGE    = 2,
  NOISE_BELOW_MIN    = 3,
  NOISE_BEYOND_MAX   = 4,
  NOISE_RETURN       = 5,
};

SOGM_NOISE_HD inline uint64_t noise_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

SOGM_NOISE_HD inline uint64_t noise_frame_key(uint64_t seed, uint64_t frame) { return noise_mix(noise_mix(seed) ^ frame); }

// g: the pixel's index in the whole swarm's frame
SOGM_NOISE_HD inline uint64_t noise_pixel_index(int32_t agent_base, int a, int rows, int cols, int v, int u) {
  return ((uint64_t)((int64_t)agent_base + (int64_t)a) * (uint64_t)rows + (uint64_t)v) * (uint64_t)cols + (uint64_t)u;
}

SOGM_NOISE_HD inline uint64_t noise_pixel_key(uint64_t frame_key, uint64_t g) { return noise_mix(frame_key ^ g); }

SOGM_NOISE_HD inline uint64_t noise_draw(uint64_t h, int k) { return noise_mix(h + (uint64_t)k); }

SOGM_NOISE_HD inline double noise_uniform(uint64_t w) { return (double)(w >> 11) * 0x1p-53; }

// S: the twelve 16-bit pieces of w_2, w_3, w_4
SOGM_NOISE_HD inline uint32_t noise_sum(uint64_t h) {
  uint32_t S = 0;
  for (int k = 2; k <= 4; ++k) {
    const uint64_t w = noise_draw(h, k);
    for (int j = 0; j < 4; ++j) S += (uint32_t)((w >> (16 * j)) & 0xFFFFull);
  }
  return S;
}

SOGM_NOISE_HD inline double noise_normal(uint64_t h) { return ((double)noise_sum(h) - 393210.0) * 0x1p-16; }

// Step 4's test of pixel (v, u), whose input is d16 != 0: any neighbour inside the image with no return, or with
// fabs(z_n - z) > edge_jump.  fetch(vn, un) is the INPUT image's pixel.  (A neighbour with the pixel's own d16 has z_n == z:
// its quotient is not formed.)
template <class Fetch>
SOGM_NOISE_HD inline bool noise_is_edge(Fetch fetch, int v, int u, int rows, int cols, uint16_t d16, double depth_scale,
                                        double edge_jump) {
  const double z = (double)d16 / depth_scale;
  for (int dv = -1; dv <= 1; ++dv) {
    const int vn = v + dv;
    if (vn < 0 || vn >= rows) continue;
    for (int du = -1; du <= 1; ++du) {
      const int un = u + du;
      if (un < 0 || un >= cols || (dv == 0 && du == 0)) continue;
      const uint16_t dn = fetch(vn, un);
      if (dn == 0) return true;
      if (dn == d16) continue;
      const double zn = (double)dn / depth_scale;
      const double df = zn - z;
      if ((df < 0 ? -df : df) > edge_jump) return true;
    }
  }
  return false;
}

// Steps 1-6 of pixel (v, u) with key h.  edge() is asked only for a pixel that has a return, survived the uniform dropout
// and whose answer matters (edge_jump > 0); the draws are indexed, so what is not drawn changes nothing.
template <class Edge>
SOGM_NOISE_HD inline int noise_pixel(const SogmDepthCamera &cam, const SogmDepthNoise &prm, uint64_t h, uint16_t d16, Edge edge,
                                     uint16_t &out) {
  out = 0;
  if (d16 == 0) return NOISE_NO_INPUT;
  const double z = (double)d16 / cam.depth_scale;
  if (noise_uniform(noise_draw(h, 0)) < prm.p_drop) return NOISE_DROP_UNIFORM;
  if (prm.edge_jump > 0 && edge() && noise_uniform(noise_draw(h, 1)) < prm.p_edge) return NOISE_DROP_EDGE;
  const double s1 = prm.sigma2 * z;
  const double s2 = s1 + prm.sigma1;
  const double s3 = s2 * z;
  const double s  = s3 + prm.sigma0;
  const double sn = s * noise_normal(h);
  const double zn = z + sn;
  if (!(zn >= prm.min_depth)) return NOISE_BELOW_MIN;
  if (zn > cam.max_depth) return NOISE_BEYOND_MAX;
  const double zs = zn * cam.depth_scale;
  const double q  = __builtin_floor(zs + 0.5);
  if (q == 0) return NOISE_BELOW_MIN;
  out = (uint16_t)q;  // max_depth * depth_scale <= 65535: q fits
  return NOISE_RETURN;
}

// "depth camera"'s cloud point of d16 at pixel (v, u): three quiet NaNs for 0
SOGM_NOISE_HD inline void noise_backproject(const SogmDepthCamera &cam, int v, int u, uint16_t d16, float xyz[3]) {
  if (d16 == 0) {
    const uint32_t qnan = 0x7FC00000u;
    for (int i = 0; i < 3; ++i) __builtin_memcpy(&xyz[i], &qnan, 4);
    return;
  }
  const double zq = (double)d16 / cam.depth_scale;
  const double du = (double)u - cam.cx;
  const double dv = (double)v - cam.cy;
  const double xz = du * zq;
  const double yz = dv * zq;
  xyz[0] = (float)(xz / cam.fx);
  xyz[1] = (float)(yz / cam.fy);
  xyz[2] = (float)zq;
}

}  // namespace sogm
