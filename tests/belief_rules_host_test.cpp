// The rules of csrc/sogm_belief.hpp compiled for the host (no HIP): reads cases, prints every result.  Numbers are hex uint64
// (doubles as their bits) unless marked dec.
//   P <prm>                                             -> P <refused 0|1>
//   E <t bits> <258 words of a record>                  -> E <valid 0|1> <x y z as bits>
//   B <prm> <t_now bits> <258 words of T> <258 of B>    -> B <12 counters dec> <pair_q dec>
// <prm> = <dt_sample bits> <5 edges bits> <n_samples dec>
// tests/test_belief_rules_host.py holds the output to tests/belief_audit_reference.py, and runs this program once more under
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "sogm_belief.hpp"

static double from_bits(uint64_t u) {
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}
static uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}
static bool read_u64(FILE *f, uint64_t *out, int n) {
  for (int i = 0; i < n; ++i)
    if (std::fscanf(f, "%" SCNx64, &out[i]) != 1) return false;
  return true;
}
static bool read_prm(FILE *f, SogmBeliefParams *prm) {
  uint64_t u[6];
  if (!read_u64(f, u, 6) || std::fscanf(f, "%d", &prm->n_samples) != 1) return false;
  prm->dt_sample = from_bits(u[0]);
  for (int i = 0; i < 5; ++i) prm->edges[i] = from_bits(u[1 + i]);
  prm->reserved_ = 0;
  return true;
}
static bool read_record(FILE *f, SogmTrajRecord *r) {
  uint64_t w[sizeof(SogmTrajRecord) / 8];
  if (!read_u64(f, w, (int)(sizeof(SogmTrajRecord) / 8))) return false;
  std::memcpy(r, w, sizeof(*r));
  return true;
}

int main(int argc, char **argv) {
  static_assert(sizeof(SogmBeliefParams) == 56 && sizeof(SogmTrajRecord) == 2064 && SOGM_BELIEF_COUNTERS == 12, "layout");
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    SogmBeliefParams prm{};
    if (tag[0] == 'P') {
      if (!read_prm(f, &prm)) return 3;
      std::printf("P %d\n", sogm::belief_refuse_params(&prm) ? 1 : 0);
    } else if (tag[0] == 'E') {
      uint64_t                   t;
      alignas(16) SogmTrajRecord r;
      if (!read_u64(f, &t, 1) || !read_record(f, &r)) return 3;
      double     p[3];
      const bool ok = sogm::belief_position(r, from_bits(t), p);
      std::printf("E %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", ok ? 1 : 0, bits(p[0]), bits(p[1]), bits(p[2]));
    } else if (tag[0] == 'B') {
      uint64_t                   t;
      alignas(16) SogmTrajRecord T, B;
      if (!read_prm(f, &prm) || sogm::belief_refuse_params(&prm) || !read_u64(f, &t, 1) || !read_record(f, &T) ||
          !read_record(f, &B))
        return 3;
      long long add[SOGM_BELIEF_COUNTERS], pair_q;
      sogm::belief_pair(prm, T, B, from_bits(t), add, &pair_q);
      std::printf("B");
      for (int i = 0; i < SOGM_BELIEF_COUNTERS; ++i) std::printf(" %lld", add[i]);
      std::printf(" %lld\n", pair_q);
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
