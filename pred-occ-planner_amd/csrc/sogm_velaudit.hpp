// sogm_velaudit.hpp — the rules of the velocity audit (include/sogm_abi.h "velocity audit" is the definition), written ONCE
// for the host and the device:
//   velaudit_estimate   the class of a new-born row: STATIC, TRACKED or UNTRACKED — the tests k_dsp_newborn applies to the list
//   velaudit_score      what one born row adds against its point's truth label: the confusion cell, NaN, the speed and
//                       direction bins, the clamped squared error in micro-units, the tolerance count
//   velaudit_code_row   the row of the per-code table a hit code lands in
//   velaudit_add        one scored point into an output row (and a per-code table): what a sequential reader does; the kernel
//                       adds the same fields through ballots and LDS
//   velaudit_agent      the whole rule for one agent, sequentially (the host's form; tests/velaudit_rules_host_test.cpp)
// k_vel_audit of sogm_velaudit.hip calls velaudit_score and velaudit_code_row.  Every fp32 expression is one IEEE operation at
// a time in the definition's order: with -ffp-contract=off host and device give the same bits.
// Only the HORIZONTAL velocity is scored: k_dsp_newborn reads vx and vy of a label and nothing else.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_VELAUDIT_HD __host__ __device__
#else
#define SOGM_VELAUDIT_HD
#endif

namespace sogm {

enum : int { VEL_EST_STATIC = 0, VEL_EST_TRACKED = 1, VEL_EST_UNTRACKED = 2, VEL_EST_DROPPED = 3 };
enum : int { VEL_TRUTH_STILL = 0, VEL_TRUTH_MOVING = 1 };
enum : int { VELAUDIT_SKIPPED = 1, VELAUDIT_BAD_SOURCE = 2, VELAUDIT_CLIPPED = 4 };
// the output row (SOGM_VELAUDIT_ROW int64 values)
enum : int {
  VELROW_N_IN = 0, VELROW_N_BORN = 1, VELROW_STATUS = 2, VELROW_N_NAN = 3, VELROW_CONFUSION = 4, VELROW_SPEED_MOVING = 12,
  VELROW_SPEED_STILL = 18, VELROW_DIRECTION = 24, VELROW_SUM_E2_UM = 29, VELROW_N_WITHIN = 30, VELROW_N = 32
};
constexpr int VELCODE_COLS = 6;  // per-code row: {static, tracked, untracked, dropped, n_within, sum_e2_um}

struct VelScore {
  int       est, truth;  // VEL_EST_*, VEL_TRUTH_*
  bool      scored;      // TRACKED and neither e2 nor m is NaN: the row counts beyond the confusion matrix
  bool      nan;         // TRACKED and e2 or m is NaN
  int       speed_bin;   // 0 .. 5 (scored rows)
  int       dir_bin;     // 0 .. 4 (scored MOVING rows)
  bool      within;      // e2 <= tol*tol (scored rows)
  long long e2_um;       // (int64)(min(e2, 1e4f) * 1e6f) (scored rows)
};

SOGM_VELAUDIT_HD inline int velaudit_estimate(float vx, float inten) {
  if (!(inten > 0.01f)) return VEL_EST_STATIC;
  return vx > -100.f ? VEL_EST_TRACKED : VEL_EST_UNTRACKED;  // the -10000 label of an unmatched possibly-dynamic cluster
}

SOGM_VELAUDIT_HD inline int velaudit_truth(float t_inten) { return t_inten > 0.01f ? VEL_TRUTH_MOVING : VEL_TRUTH_STILL; }

// est4 = {vx, vy, vz, intensity} of the born row, truth4 the same of the point's truth label
SOGM_VELAUDIT_HD inline VelScore velaudit_score(const float *est4, const float *truth4, float tol) {
  VelScore s{};
  const float vx = est4[0], vy = est4[1];
  s.est   = velaudit_estimate(vx, est4[3]);
  s.truth = velaudit_truth(truth4[3]);
  if (s.est != VEL_EST_TRACKED) return s;
  const float tvx = s.truth == VEL_TRUTH_MOVING ? truth4[0] : 0.f, tvy = s.truth == VEL_TRUTH_MOVING ? truth4[1] : 0.f;
  const float ex = vx - tvx, ey = vy - tvy;
  const float e2  = ex * ex + ey * ey;
  const float s_e = vx * vx + vy * vy, s_t = tvx * tvx + tvy * tvy;
  const float dot = vx * tvx + vy * tvy;
  const float m   = s_e * s_t;
  if (e2 != e2 || m != m) {
    s.nan = true;
    return s;
  }
  s.scored = true;
  const float T[5] = {0.1f, 0.25f, 0.5f, 1.0f, 2.0f};
  for (int k = 0; k < 5; ++k) s.speed_bin += e2 > T[k] * T[k] ? 1 : 0;
  const float d2 = dot * dot;
  if (s_e == 0.f)
    s.dir_bin = 4;  // faster than 5 m/s: zeroed but matched
  else if (dot > 0.f && d2 >= 0.9330127f * m)
    s.dir_bin = 0;  // within 15 degrees
  else if (dot > 0.f && d2 >= 0.5f * m)
    s.dir_bin = 1;  // within 45 degrees
  else if (dot > 0.f)
    s.dir_bin = 2;
  else
    s.dir_bin = 3;
  s.within = e2 <= tol * tol;
  const float clamped = e2 < 1.0e4f ? e2 : 1.0e4f;
  s.e2_um = (long long)(clamped * 1.0e6f);
  return s;
}

// rows 0 .. n_codes - 1: the codes themselves; n_codes: SOGM_HIT_GROUND (-1); n_codes + 1: anything else
SOGM_VELAUDIT_HD inline int velaudit_code_row(int code, int n_codes) {
  if (code >= 0 && code < n_codes) return code;
  return code == -1 ? n_codes : n_codes + 1;
}

// one scored point into a row (and, with `per_code`, into row `code_row` of the agent's table)
SOGM_VELAUDIT_HD inline void velaudit_add(const VelScore &s, long long *row, long long *per_code, int code_row) {
  row[VELROW_CONFUSION + s.truth * 4 + s.est] += 1;
  if (per_code) per_code[code_row * VELCODE_COLS + s.est] += 1;
  if (s.nan) row[VELROW_N_NAN] += 1;
  if (!s.scored) return;
  if (per_code) {
    per_code[code_row * VELCODE_COLS + 4] += s.within ? 1 : 0;
    per_code[code_row * VELCODE_COLS + 5] += s.e2_um;
  }
  if (s.truth == VEL_TRUTH_MOVING) {
    row[VELROW_SPEED_MOVING + s.speed_bin] += 1;
    row[VELROW_DIRECTION + s.dir_bin] += 1;
    row[VELROW_SUM_E2_UM] += s.e2_um;
    row[VELROW_N_WITHIN] += s.within ? 1 : 0;
  } else {
    row[VELROW_SPEED_STILL + s.speed_bin] += 1;
  }
}

// One agent, sequentially.  born [n_born][7], src [n_born], truth labels [n_in][4] and codes [n_in] (or null) of THIS agent;
// range_len = range end - begin; seen: max_points bits of scratch, zeroed here.  Adds into row[32] / per_code (the caller
// zeroes them for a plain call) and ORs the status.  Of several rows that name one point the one with the smallest k counts.
SOGM_VELAUDIT_HD inline void velaudit_agent(bool ok, long long range_len, int max_points, int n_born, const float *born,
                                            const int32_t *src, const float *truth, const int32_t *code, int n_codes,
                                            float tol, uint32_t *seen, long long *row, long long *per_code) {
  long long n_in = range_len < (long long)max_points ? range_len : (long long)max_points;
  if (!ok || n_in <= 0) {
    row[VELROW_STATUS] |= VELAUDIT_SKIPPED;
    return;
  }
  if (range_len > (long long)max_points) row[VELROW_STATUS] |= VELAUDIT_CLIPPED;
  if (n_born < 0) n_born = 0;
  if (n_born > max_points) n_born = max_points;
  row[VELROW_N_IN] += n_in;
  row[VELROW_N_BORN] += n_born;
  for (int w = 0; w < (max_points + 31) / 32; ++w) seen[w] = 0;
  for (int k = 0; k < n_born; ++k) {
    const int i = src[k];
    if (i < 0 || (long long)i >= n_in || ((seen[i >> 5] >> (i & 31)) & 1u)) {
      row[VELROW_STATUS] |= VELAUDIT_BAD_SOURCE;
      continue;
    }
    seen[i >> 5] |= 1u << (i & 31);
    const VelScore s = velaudit_score(born + (size_t)k * 7 + 3, truth + (size_t)i * 4, tol);
    velaudit_add(s, row, per_code, per_code ? velaudit_code_row(code[i], n_codes) : 0);
  }
  for (int i = 0; i < (int)n_in; ++i) {
    if ((seen[i >> 5] >> (i & 31)) & 1u) continue;
    VelScore s{};
    s.est   = VEL_EST_DROPPED;
    s.truth = velaudit_truth(truth[(size_t)i * 4 + 3]);
    velaudit_add(s, row, per_code, per_code ? velaudit_code_row(code[i], n_codes) : 0);
  }
}

}  // namespace sogm
