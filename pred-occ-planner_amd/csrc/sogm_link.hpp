// sogm_link.hpp — the radio-link model (include/sogm_abi.h "radio links" is the definition), the rules written ONCE for the
// host and the device:
//   link_tick_key / link_key       h = mix(mix(mix(seed) ^ m) ^ (j * n_total + a)) in two halves
//   link_delay / link_out_of_range the delay draw, the fp64 range test
//   link_candidate                 the fate of message (k - l, j -> a) as seen at tick k: does it exist, is it out of range,
//                                  lost, and does it arrive now
//   link_resolve                   the winner among a pair's arrivals and what it does to the held row
//   link_pair_counts               what the pair adds to the receiver's eight counters
//   link_refuse_params / link_refuse_call   the refusals of the three entries, as the rule's text (NULL: accepted)
// k_link_deliver of sogm_link.hip evaluates link_candidate in eight lanes and ballots; a host program walks the same
// candidates in a loop (tests/link_rules_host_test.cpp).  The draws are sogm_depthnoise.hpp's noise_mix / noise_uniform.
// Every fp64 expression is a single IEEE operation: with -ffp-contract=off host and device give the same bits.
#pragma once

#include "sogm_depthnoise.hpp"

namespace sogm {

constexpr int LINK_LANES = SOGM_LINK_MAX_DELAY + 1;  // candidate send ticks k, k - 1, ..., k - 7

SOGM_NOISE_HD inline uint64_t link_tick_key(uint64_t seed, int m) { return noise_mix(noise_mix(seed) ^ (uint64_t)(int64_t)m); }

SOGM_NOISE_HD inline uint64_t link_key(uint64_t tick_key, int j, int a, int n_total) {
  return noise_mix(tick_key ^ ((uint64_t)j * (uint64_t)n_total + (uint64_t)a));
}

SOGM_NOISE_HD inline int link_delay(const SogmLinkParams &prm, uint64_t h) {
  const int    span = prm.delay_max - prm.delay_min + 1;
  const double x    = noise_uniform(noise_mix(h + 1)) * (double)span;
  const int    i    = (int)__builtin_floor(x);
  return prm.delay_min + (i < span - 1 ? i : span - 1);
}

// pj, pa: the positions of sender and receiver at the send tick (not read when range == 0)
SOGM_NOISE_HD inline bool link_out_of_range(double range, const double *pj, const double *pa) {
  if (!(range > 0)) return false;
  const double dx = pj[0] - pa[0], dy = pj[1] - pa[1], dz = pj[2] - pa[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const double s  = xx + yy;
  const double d2 = s + zz;
  const double r2 = range * range;
  return !(d2 <= r2);
}

inline SOGM_NOISE_HD int link_slot(int tick, int delay_max) { return tick % (delay_max + 1); }

struct LinkCandidate {
  bool exists, far, lost, arrives;
};

// Message (m = k - l, j -> a), l = 0 .. LINK_LANES - 1, as tick k sees it.  n_pieces and the positions are those stored for
// tick m; fetch_n() and fetch_pos(pj, pa) are asked only for a tick that is in the ring (l <= delay_max, m >= tick0) and
// for l == 0.
template <class FetchN, class FetchPos>
SOGM_NOISE_HD inline LinkCandidate link_candidate(const SogmLinkParams &prm, int n_total, int k, int l, int tick0, int j, int a,
                                                  FetchN fetch_n, FetchPos fetch_pos) {
  LinkCandidate c{false, false, false, false};
  const int m = k - l;
  if (l > prm.delay_max || m < tick0) return c;
  if (fetch_n() <= 0) return c;
  c.exists = true;
  if (prm.range > 0) {
    double pj[3], pa[3];
    fetch_pos(pj, pa);
    c.far = link_out_of_range(prm.range, pj, pa);
  }
  const uint64_t h = link_key(link_tick_key(prm.seed, m), j, a, n_total);
  if (!c.far) c.lost = noise_uniform(noise_mix(h)) < prm.p_loss;
  c.arrives = !c.far && !c.lost && link_delay(prm, h) == l;
  return c;
}

struct LinkVerdict {
  int  m;      // the winner's send tick (-1: nothing arrived)
  bool stale;  // it is older than what was held
  bool apply;  // it is copied into the view
};

// arrivals: bit l is set when message (k - l) arrives at k.  The lowest bit is the largest m.
SOGM_NOISE_HD inline LinkVerdict link_resolve(const SogmLinkParams &prm, int k, unsigned arrivals, int held) {
  LinkVerdict v{-1, false, false};
  if (!arrivals) return v;
  v.m     = k - __builtin_ctz(arrivals);
  v.stale = v.m < held;
  v.apply = !(v.stale && (prm.flags & SOGM_LINK_NEWEST_WINS));
  return v;
}

// what pair (a, j != a) adds at tick k: now is candidate l == 0, held_after the held tick after delivery
SOGM_NOISE_HD inline void link_pair_counts(const LinkCandidate &now, unsigned arrivals, const LinkVerdict &v, int k,
                                           int held_after, long long add[SOGM_LINK_COUNTERS]) {
  add[0] = now.exists ? 1 : 0;
  add[1] = now.far ? 1 : 0;
  add[2] = now.lost ? 1 : 0;
  add[3] = __builtin_popcount(arrivals);
  add[4] = v.apply ? 1 : 0;
  add[5] = v.stale ? 1 : 0;
  add[6] = held_after >= 0 ? (long long)k - held_after : 0;
  add[7] = held_after >= 0 ? 0 : 1;
}

// isfinite without <cmath>: x - x is 0 exactly for a finite x
SOGM_NOISE_HD inline bool link_finite(double x) { return x - x == 0.0; }

SOGM_NOISE_HD inline const char *link_refuse_params(const SogmLinkParams *prm) {
  if (!prm) return "null parameters";
  if (!link_finite(prm->p_loss) || prm->p_loss < 0 || prm->p_loss > 1) return "p_loss must be in [0, 1]";
  if (!link_finite(prm->range) || prm->range < 0) return "range must be finite and >= 0";
  if (prm->delay_min < 0 || prm->delay_max < prm->delay_min || prm->delay_max > SOGM_LINK_MAX_DELAY)
    return "delays must satisfy 0 <= delay_min <= delay_max <= SOGM_LINK_MAX_DELAY";
  return nullptr;
}

SOGM_NOISE_HD inline bool link_misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

SOGM_NOISE_HD inline const char *link_refuse_buffers(const SogmLinkParams *prm, int n_total, int n_local,
                                                     const SogmLinkBuffers *b) {
  if (const char *why = link_refuse_params(prm)) return why;
  if (n_total < 1 || n_local < 1 || n_local > n_total) return "n_total >= 1 and 1 <= n_local <= n_total";
  if (!b || !b->ring_table || !b->views || !b->held_tick || !b->counters) return "null buffer";
  if (prm->range > 0 && !b->ring_pos) return "range > 0 without ring_pos";
  if (link_misaligned(b->ring_table) || link_misaligned(b->views)) return "record buffers must be 16-byte aligned";
  return nullptr;
}

SOGM_NOISE_HD inline const char *link_refuse_call(const SogmLinkParams *prm, int tick, int tick0, const void *table,
                                                  const void *pos, int n_total, int agent0, int n_local,
                                                  const SogmLinkBuffers *b) {
  if (const char *why = link_refuse_buffers(prm, n_total, n_local, b)) return why;
  if (!table) return "null table";
  if (prm->range > 0 && !pos) return "range > 0 without positions";
  if (agent0 < 0 || n_local > n_total - agent0) return "0 <= agent0 and n_local <= n_total - agent0";
  if (tick0 < 0 || tick < tick0) return "0 <= tick0 <= tick";
  if (link_misaligned(table)) return "record buffers must be 16-byte aligned";
  return nullptr;
}

}  // namespace sogm
