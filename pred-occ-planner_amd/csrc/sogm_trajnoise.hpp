// sogm_trajnoise.hpp — the message noise (include/sogm_abi.h "message noise" is the definition), the rules written ONCE for
// the host and the device:
//   trajnoise_key / trajnoise_draw   key(tag, x, j) = mix(mix(mix(mix(seed) ^ tag) ^ x) ^ j), component c draws N(key + 16c)
//   trajnoise_term                   one of a message's seven terms sigma * N: b[0..2], tau, e[0..2]
//   trajnoise_shift                  shift x, y, z = b + e and tau of message (m, j)
//   trajnoise_noised                 how many of a record's cpts doubles carry noise
//   trajnoise_word                   what one 8-byte word of the record becomes
//   trajnoise_record                 a whole record (the host's loop over the words)
//   trajnoise_refuse                 the refusals of sogm_traj_noise, as the rule's text (NULL: accepted)
// k_traj_noise of sogm_trajnoise.hip evaluates trajnoise_term in seven lanes, shares the terms and calls trajnoise_word for the
// two words of every 16-byte piece; a host program calls trajnoise_record (tests/traj_noise_rules_host_test.cpp).  The
// draws are sogm_depthnoise.hpp's noise_mix / noise_normal.  Every fp64 expression is a single IEEE operation: with
// -ffp-contract=off host and device give the same bits.  Known answers, seed 0x5067: key(1, 0, 0) = 0x4ACD8EB1A9CFDCC6,
// N at c = 0, 1, 2: 0x1.469p-2, -0x1.c25p-4, -0x1.a0b6p-1; key(2, 0, 3) = 0xF86E1BF400FF8055, N = -0x1.1598p-1;
// key(3, 7, 4) = 0x0E12DE2E62B1FC89, N: 0x1.d6dep-1, -0x1.34dep+0, 0x1.8a64p-1.
#pragma once

#include "sogm_depthnoise.hpp"

namespace sogm {

constexpr uint64_t TRAJNOISE_LOC = 1, TRAJNOISE_TIME = 2, TRAJNOISE_TRACK = 3;  // the tags
constexpr int      TRAJNOISE_TERMS = 7;                                         // b[0..2], tau, e[0..2]
constexpr int      TRAJ_WORDS      = (int)(sizeof(SogmTrajRecord) / 8);         // 258: ids, time_start, 16 durations, 240 cpts
constexpr int      TRAJ_WORD_TIME  = 1, TRAJ_WORD_CPTS = 2 + SOGM_MAX_PIECES;
static_assert(sizeof(SogmTrajRecord) == 8 * (2 + SOGM_MAX_PIECES + SOGM_MAX_PIECES * 15), "a record is 258 words");

SOGM_NOISE_HD inline uint64_t trajnoise_key(uint64_t seed, uint64_t tag, uint64_t x, uint64_t j) {
  return noise_mix(noise_mix(noise_mix(noise_mix(seed) ^ tag) ^ x) ^ j);
}

SOGM_NOISE_HD inline double trajnoise_draw(uint64_t key, int c) { return noise_normal(key + 16ull * (uint64_t)c); }

SOGM_NOISE_HD inline int trajnoise_epoch(const SogmTrajNoise &prm, int m) { return prm.loc_hold > 0 ? m / prm.loc_hold : 0; }

// term i of message (m, j): 0 .. 2 the localisation bias b[i], 3 the clock offset tau, 4 .. 6 the tracking error e[i - 4]
SOGM_NOISE_HD inline double trajnoise_term(const SogmTrajNoise &prm, int m, int j, int i) {
  const uint64_t jj = (uint64_t)(int64_t)j;
  if (i < 3) return prm.sigma_loc[i] * trajnoise_draw(trajnoise_key(prm.seed, TRAJNOISE_LOC, (uint64_t)trajnoise_epoch(prm, m), jj), i);
  if (i == 3) return prm.sigma_time * trajnoise_draw(trajnoise_key(prm.seed, TRAJNOISE_TIME, 0, jj), 0);
  return prm.sigma_track * trajnoise_draw(trajnoise_key(prm.seed, TRAJNOISE_TRACK, (uint64_t)(int64_t)m, jj), i - 4);
}

// shift[0..2] = b + e, shift[3] = tau
SOGM_NOISE_HD inline void trajnoise_shift(const SogmTrajNoise &prm, int m, int j, double shift[4]) {
  for (int c = 0; c < 3; ++c) {
    const double b = trajnoise_term(prm, m, j, c), e = trajnoise_term(prm, m, j, 4 + c);
    shift[c] = b + e;
  }
  shift[3] = trajnoise_term(prm, m, j, 3);
}

// the doubles of cpts that carry noise: 15 per piece of the trajectory (0: the row is not a message)
SOGM_NOISE_HD inline int trajnoise_noised(int n_pieces) {
  return n_pieces <= 0 ? 0 : 15 * (n_pieces < SOGM_MAX_PIECES ? n_pieces : SOGM_MAX_PIECES);
}

// word q (0 .. 257) of a message: time_start takes tau, cpts double i < noised takes shift[i % 3]; everything else, and
// any word whose shift == 0.0, keeps its bits
SOGM_NOISE_HD inline uint64_t trajnoise_word(int q, uint64_t bits, int noised, const double shift[4]) {
  double s;
  if (q == TRAJ_WORD_TIME && noised > 0)
    s = shift[3];
  else if (q >= TRAJ_WORD_CPTS && q - TRAJ_WORD_CPTS < noised) {
    const int c = (q - TRAJ_WORD_CPTS) % 3;  // (selects, not an indexed read: the shift stays in registers on the device)
    s           = c == 0 ? shift[0] : c == 1 ? shift[1] : shift[2];
  } else
    return bits;
  if (s == 0.0) return bits;
  double v;
  __builtin_memcpy(&v, &bits, 8);
  v = v + s;
  __builtin_memcpy(&bits, &v, 8);
  return bits;
}

// row j of the table sent at tick m; out may be the row itself.  shift4 (or null): the row's out_shift
inline void trajnoise_record(const SogmTrajNoise &prm, int m, int j, const SogmTrajRecord *in, SogmTrajRecord *out,
                             double *shift4) {
  const int noised   = trajnoise_noised(in->n_pieces);
  double    shift[4] = {0.0, 0.0, 0.0, 0.0};
  if (noised > 0) trajnoise_shift(prm, m, j, shift);
  for (int q = 0; q < TRAJ_WORDS; ++q) {
    uint64_t w;
    __builtin_memcpy(&w, reinterpret_cast<const char *>(in) + 8 * q, 8);
    w = trajnoise_word(q, w, noised, shift);
    __builtin_memcpy(reinterpret_cast<char *>(out) + 8 * q, &w, 8);
  }
  if (shift4)
    for (int i = 0; i < 4; ++i) shift4[i] = shift[i];
}

// isfinite without <cmath>: x - x is 0 exactly for a finite x
SOGM_NOISE_HD inline bool trajnoise_bad_sigma(double x) { return !(x - x == 0.0) || x < 0; }

SOGM_NOISE_HD inline const char *trajnoise_refuse_params(const SogmTrajNoise *prm) {
  if (!prm) return "null parameters";
  for (int c = 0; c < 3; ++c)
    if (trajnoise_bad_sigma(prm->sigma_loc[c])) return "sigma_loc must be finite and >= 0";
  if (trajnoise_bad_sigma(prm->sigma_time)) return "sigma_time must be finite and >= 0";
  if (trajnoise_bad_sigma(prm->sigma_track)) return "sigma_track must be finite and >= 0";
  if (prm->loc_hold < 0) return "loc_hold must be >= 0";
  return nullptr;
}

SOGM_NOISE_HD inline const char *trajnoise_refuse(const SogmTrajNoise *prm, int tick, const void *table, int n_total,
                                                  const void *out) {
  if (const char *why = trajnoise_refuse_params(prm)) return why;
  if (!table || !out) return "null table";
  if (tick < 0) return "tick must be >= 0";
  if (n_total < 1) return "n_total must be >= 1";
  if (((uintptr_t)table & 15) != 0 || ((uintptr_t)out & 15) != 0) return "record buffers must be 16-byte aligned";
  return nullptr;
}

}  // namespace sogm
