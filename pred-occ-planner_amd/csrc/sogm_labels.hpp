// sogm_labels.hpp — ground-truth velocity labels through the voxel filter (include/sogm_abi.h "ground-truth labels" is the
// definition), the rule written ONCE for the host and the device:
//   f2key                          the order-preserving unsigned image of an fp32's bits (the filter's bounding box uses it too)
//   label_key / label_key_code     the 64-bit key of a raw point {f2key(z), ~image(code)} and the code back from a key
//   label_of                       the label {vx, vy, vz, intensity} of a hit code
// k_filter_accumulate<true> / k_filter_emit<true> of sogm_filter.hip call these bodies; a host program compiles them as well
// (tests/label_rules_host_test.cpp).  Every fp32 expression is a single IEEE operation: with -ffp-contract=off host and device
// give the same bits.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_LABEL_HD __host__ __device__
#else
#define SOGM_LABEL_HD
#endif

#include "../../include/sogm_abi.h"

namespace sogm {

SOGM_LABEL_HD inline unsigned f2key(float f) {
  unsigned u;
  __builtin_memcpy(&u, &f, sizeof u);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// "No point yet" of a leaf.  No finite point makes it: a high word of all ones would be f2key of the bits 0x7fffffff, a NaN.
constexpr unsigned long long LABEL_KEY_EMPTY = ~0ull;

// The smallest key of a leaf is "smallest z (-0 before +0), then LARGEST code": the low word falls as the code rises.
SOGM_LABEL_HD inline unsigned long long label_key(float z, int32_t code) {
  const unsigned image = (unsigned)code ^ 0x80000000u;  // int32 order -> unsigned order
  return ((unsigned long long)f2key(z) << 32) | (unsigned long long)(~image);
}

SOGM_LABEL_HD inline int32_t label_key_code(unsigned long long key) {
  return (int32_t)(~(unsigned)key ^ 0x80000000u);
}

SOGM_LABEL_HD inline bool label_finite(float v) { return v - v == 0.0f; }  // false for +-inf and NaN

// out = {vx, vy, vz, 1} of what code `c` names if that moves faster than min_speed, else {0, 0, 0, 0}
SOGM_LABEL_HD inline void label_of(int32_t c, const SogmLabelSources &s, float out[4]) {
  float v[3] = {0.0f, 0.0f, 0.0f};
  const long long k = (long long)c - (long long)s.n_cyl;
  if (c >= 0 && k < 0) {
    v[0] = (float)s.cylinders[c].vx;
    v[1] = (float)s.cylinders[c].vy;
  } else if (k >= 0 && k < (long long)s.n_bodies) {
    for (int i = 0; i < 3; ++i) v[i] = (float)s.body_vel[(size_t)k * 3 + (size_t)i];
  }
  const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  const float xy = xx + yy;
  const float s2 = xy + zz;
  const float m2 = s.min_speed * s.min_speed;
  const bool  on = label_finite(v[0]) && label_finite(v[1]) && label_finite(v[2]) && s2 > m2;
  out[0] = on ? v[0] : 0.0f;
  out[1] = on ? v[1] : 0.0f;
  out[2] = on ? v[2] : 0.0f;
  out[3] = on ? 1.0f : 0.0f;
}

}  // namespace sogm
