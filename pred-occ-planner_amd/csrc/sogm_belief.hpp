// sogm_belief.hpp — the belief audit (include/sogm_abi.h "belief audit" is the definition), the rules written ONCE for the
// host and the device:
//   belief_position    a record's position at an absolute time: traj_eval_relative's arithmetic (sogm_device.hpp), restated
//                      here in its order of operations so that a host compiler reads it too
//   belief_class       what a pair (truth row, believed row) is: nothing, compared, unheard, phantom
//   belief_sample      one compared sample: its bin and its q
//   belief_pair        a whole pair (the host's loop over the samples): what it adds to the twelve counters, its largest q
//   belief_refuse      the refusals of sogm_belief_audit, as the rule's text (NULL: accepted)
// k_belief_audit of sogm_belief.hip evaluates belief_sample in one lane per sample; a host program calls belief_pair
// (tests/belief_rules_host_test.cpp).  Every fp64 expression is a single IEEE operation: with -ffp-contract=off host and
// device give the same bits.
#pragma once

#include "sogm_depthnoise.hpp"

namespace sogm {

constexpr long long BELIEF_Q_MAX = 1ll << 40;
enum BeliefClass { BELIEF_NONE = 0, BELIEF_COMPARED = 1, BELIEF_UNHEARD = 2, BELIEF_PHANTOM = 3 };
enum BeliefCounter { BELIEF_CNT_COMPARED = 0, BELIEF_CNT_UNHEARD = 1, BELIEF_CNT_PHANTOM = 2, BELIEF_CNT_SAMPLES = 3,
                     BELIEF_CNT_BIN0 = 4, BELIEF_CNT_SUM_Q = 10, BELIEF_CNT_MAX_Q = 11 };

// Bezier::getPos of a record at t_abs, clamped to [time_start, time_start + total]; false (and zeros) for an empty record.
// n_pieces above SOGM_MAX_PIECES counts as SOGM_MAX_PIECES (no read past the arrays).
SOGM_NOISE_HD inline bool belief_position(const SogmTrajRecord &r, double t_abs, double p[3]) {
  const int n = r.n_pieces < SOGM_MAX_PIECES ? r.n_pieces : SOGM_MAX_PIECES;
  if (n <= 0) {
    p[0] = p[1] = p[2] = 0.0;
    return false;
  }
  double tt    = t_abs - r.time_start;
  double total = 0;
  for (int k = 0; k < n; ++k) total += r.duration[k];
  tt = tt < 0 ? 0 : (tt > total ? total : tt);
  int    piece = n - 1;
  double rem   = tt;
  for (int k = 0; k < n; ++k) {
    rem -= r.duration[k];
    if (rem < 0) {
      piece = k;
      break;
    }
  }
  double t0 = 0;
  for (int k = 0; k < piece; ++k) t0 += r.duration[k];
  const double tf = t0 + r.duration[piece], dur = tf - t0, s = (tt - t0) / dur;
  const double A[5][5] = {{1, -4, 6, -4, 1}, {0, 4, -12, 12, -4}, {0, 0, 6, -12, 6}, {0, 0, 0, 4, -4}, {0, 0, 0, 0, 1}};
  const double S0[5]   = {1, s, s * s, s * s * s, (s * s) * (s * s)};
  const double *c      = r.cpts + piece * 15;
  for (int d = 0; d < 3; ++d) {
    double pos = 0;
    for (int j = 0; j < 5; ++j) {
      double b = 0;
      for (int q = 0; q < 5; ++q) b += c[q * 3 + d] * A[q][j];
      pos += b * S0[j];
    }
    p[d] = pos;
  }
  return true;
}

SOGM_NOISE_HD inline int belief_class(int truth_pieces, int believed_pieces) {
  const bool t = truth_pieces > 0, b = believed_pieces > 0;
  return t && b ? BELIEF_COMPARED : t ? BELIEF_UNHEARD : b ? BELIEF_PHANTOM : BELIEF_NONE;
}

// sample s of a compared pair as receiver time t_now sees it: its bin 0 .. 5 and its q
SOGM_NOISE_HD inline void belief_sample(const SogmBeliefParams &prm, const SogmTrajRecord &T, const SogmTrajRecord &B, double t_now,
                                        int s, int *bin, long long *q) {
  const double ts = (double)s * prm.dt_sample;
  const double t  = t_now + ts;
  double       pT[3], pB[3];
  belief_position(T, t, pT);
  belief_position(B, t, pB);
  const double dx = pB[0] - pT[0], dy = pB[1] - pT[1], dz = pB[2] - pT[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double xy = xx + yy;
  const double d2 = xy + zz;
  int          b  = 5;
  for (int i = 4; i >= 0; --i) {
    const double e2 = prm.edges[i] * prm.edges[i];
    if (d2 <= e2) b = i;  // (the edges ascend: the last hit walking down is the first bin that holds it; a NaN hits none)
  }
  const double m = d2 * 1e6;
  const double y = m + 0.5;
  const double f = __builtin_floor(y);
  *bin = b;
  *q   = f < (double)BELIEF_Q_MAX ? (long long)f : BELIEF_Q_MAX;  // a NaN and +inf compare false
}

// what pair (T, B) adds: add[0 .. 10] are sums, add[11] is the pair's maximum; pair_q is -1 when it is not compared
SOGM_NOISE_HD inline void belief_pair(const SogmBeliefParams &prm, const SogmTrajRecord &T, const SogmTrajRecord &B, double t_now,
                                      long long add[SOGM_BELIEF_COUNTERS], long long *pair_q) {
  for (int i = 0; i < SOGM_BELIEF_COUNTERS; ++i) add[i] = 0;
  *pair_q       = -1;
  const int cls = belief_class(T.n_pieces, B.n_pieces);
  if (cls == BELIEF_UNHEARD) add[BELIEF_CNT_UNHEARD] = 1;
  if (cls == BELIEF_PHANTOM) add[BELIEF_CNT_PHANTOM] = 1;
  if (cls != BELIEF_COMPARED) return;
  add[BELIEF_CNT_COMPARED] = 1;
  long long worst          = 0;
  for (int s = 0; s < prm.n_samples; ++s) {
    int       bin;
    long long q;
    belief_sample(prm, T, B, t_now, s, &bin, &q);
    add[BELIEF_CNT_SAMPLES] += 1;
    add[BELIEF_CNT_BIN0 + bin] += 1;
    add[BELIEF_CNT_SUM_Q] += q;
    worst = q > worst ? q : worst;
  }
  add[BELIEF_CNT_MAX_Q] = worst;
  *pair_q               = worst;
}

SOGM_NOISE_HD inline bool belief_finite(double x) { return x - x == 0.0; }

SOGM_NOISE_HD inline const char *belief_refuse_params(const SogmBeliefParams *prm) {
  if (!prm) return "null parameters";
  if (prm->n_samples < 1 || prm->n_samples > SOGM_BELIEF_MAX_SAMPLES) return "n_samples must be in 1 .. SOGM_BELIEF_MAX_SAMPLES";
  if (!belief_finite(prm->dt_sample) || !(prm->dt_sample > 0)) return "dt_sample must be finite and > 0";
  for (int i = 0; i < 5; ++i)
    if (!belief_finite(prm->edges[i]) || !(prm->edges[i] > (i ? prm->edges[i - 1] : 0.0)))
      return "edges must be finite, > 0 and strictly ascending";
  return nullptr;
}

SOGM_NOISE_HD inline const char *belief_refuse(const SogmBeliefParams *prm, const void *truth, const void *views, const void *t_now,
                                               int n_total, int agent0, int n_local, const void *counters) {
  if (const char *why = belief_refuse_params(prm)) return why;
  if (!truth || !views || !t_now || !counters) return "null buffer";
  if (n_total < 1 || agent0 < 0 || n_local < 1 || n_local > n_total - agent0)
    return "n_total >= 1, 0 <= agent0 and 1 <= n_local <= n_total - agent0";
  if (((uintptr_t)truth & 15) != 0 || ((uintptr_t)views & 15) != 0) return "record buffers must be 16-byte aligned";
  if (n_local > 65535) return "n_local exceeds one launch (65535)";
  return nullptr;
}

}  // namespace sogm
