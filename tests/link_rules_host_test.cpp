// The rules of csrc/sogm_link.hpp compiled for the host (no HIP): reads cases, prints every result.
//   M <u64 x>                                              -> M <mix(x)>
//   K <u64 seed> <m j a n_total dec> <p_loss bits> <delay_min delay_max dec>
//                                                          -> K <h> <u bits> <d dec> <lost 0|1>
//   G <range bits> <pj: 3 x bits> <pa: 3 x bits>           -> G <out of range 0|1>
//   P <p_loss bits> <range bits> <delay_min delay_max dec> -> P <refused 0|1>
//   S <u64 seed> <p_loss bits> <range bits> <delay_min delay_max flags dec> <n_total agent0 n_local tick0 n_ticks dec>
//     <with_pos 0|1>, then per tick n_total x <n_pieces dec> and, with_pos, n_total x 3 x <bits>
//                                                          -> per tick and local receiver: per sender
//                                                             V <tick> <a> <j> <held tick> <arrival mask hex>, then
//                                                             C <tick> <a> <8 counters decimal>
// A view row is named by its held tick: the row is the sender's row of that tick's table.  The walk over a pair's eight
// candidates is the kernel's, with a loop where the kernel has lanes and a ballot.
// tests/test_link_rules_host.py holds the output to tests/link_model_reference.py, and runs this program once more under
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_link.hpp"

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
static bool read_doubles(FILE *f, double *out, int n) {
  for (int i = 0; i < n; ++i) {
    uint64_t u;
    if (!read_u64(f, &u, 1)) return false;
    out[i] = from_bits(u);
  }
  return true;
}

static int run_swarm(FILE *f) {
  SogmLinkParams prm{};
  double         pr[2];
  int            n_total, agent0, n_local, tick0, n_ticks, with_pos;
  if (!read_u64(f, &prm.seed, 1) || !read_doubles(f, pr, 2) ||
      std::fscanf(f, "%d %d %d", &prm.delay_min, &prm.delay_max, &prm.flags) != 3 ||
      std::fscanf(f, "%d %d %d %d %d %d", &n_total, &agent0, &n_local, &tick0, &n_ticks, &with_pos) != 6)
    return 3;
  prm.p_loss = pr[0], prm.range = pr[1];
  if (sogm::link_refuse_params(&prm) || n_total < 1 || agent0 < 0 || n_local < 1 || n_local > n_total - agent0 || tick0 < 0 ||
      n_ticks < 1 || (prm.range > 0 && !with_pos))
    return 3;
  const int              slots = prm.delay_max + 1;
  std::vector<int>       ring_n((size_t)slots * n_total, 0);
  std::vector<double>    ring_pos((size_t)slots * n_total * 3, 0.0);
  std::vector<int>       held((size_t)n_local * n_total, -1);
  std::vector<long long> counters((size_t)n_local * SOGM_LINK_COUNTERS, 0);
  for (int k = tick0; k < tick0 + n_ticks; ++k) {
    const size_t now = (size_t)sogm::link_slot(k, prm.delay_max) * n_total;
    for (int j = 0; j < n_total; ++j)
      if (std::fscanf(f, "%d", &ring_n[now + j]) != 1) return 3;
    if (with_pos && !read_doubles(f, &ring_pos[now * 3], n_total * 3)) return 3;
    for (int al = 0; al < n_local; ++al) {
      const int a = agent0 + al;
      for (int j = 0; j < n_total; ++j) {
        const size_t pair = (size_t)al * n_total + j;
        if (j == a) {
          held[pair] = k;
          continue;
        }
        unsigned            arrivals = 0;
        sogm::LinkCandidate first{false, false, false, false};
        for (int l = 0; l < sogm::LINK_LANES; ++l) {
          const size_t row       = (size_t)sogm::link_slot(k - l < 0 ? 0 : k - l, prm.delay_max) * n_total;
          auto         fetch_n   = [&]() { return ring_n[row + j]; };
          auto         fetch_pos = [&](double pj[3], double pa[3]) {
            for (int i = 0; i < 3; ++i) pj[i] = ring_pos[(row + j) * 3 + i], pa[i] = ring_pos[(row + a) * 3 + i];
          };
          const sogm::LinkCandidate c = sogm::link_candidate(prm, n_total, k, l, tick0, j, a, fetch_n, fetch_pos);
          if (l == 0) first = c;
          if (c.arrives) arrivals |= 1u << l;
        }
        const sogm::LinkVerdict v = sogm::link_resolve(prm, k, arrivals, held[pair]);
        if (v.apply) held[pair] = v.m;
        long long add[SOGM_LINK_COUNTERS];
        sogm::link_pair_counts(first, arrivals, v, k, held[pair], add);
        for (int i = 0; i < SOGM_LINK_COUNTERS; ++i) counters[(size_t)al * SOGM_LINK_COUNTERS + i] += add[i];
        std::printf("V %d %d %d %d %x\n", k, a, j, held[pair], arrivals);
      }
      std::printf("C %d %d", k, a);
      for (int i = 0; i < SOGM_LINK_COUNTERS; ++i) std::printf(" %lld", counters[(size_t)al * SOGM_LINK_COUNTERS + i]);
      std::printf("\n");
    }
  }
  return 0;
}

int main(int argc, char **argv) {
  static_assert(sizeof(SogmLinkParams) == 40 && sizeof(SogmLinkBuffers) == 5 * sizeof(void *), "layout");
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    if (tag[0] == 'M') {
      uint64_t x;
      if (!read_u64(f, &x, 1)) return 3;
      std::printf("M %016" PRIx64 "\n", sogm::noise_mix(x));
    } else if (tag[0] == 'K') {
      SogmLinkParams prm{};
      int            m, j, a, n_total;
      if (!read_u64(f, &prm.seed, 1) || std::fscanf(f, "%d %d %d %d", &m, &j, &a, &n_total) != 4 ||
          !read_doubles(f, &prm.p_loss, 1) || std::fscanf(f, "%d %d", &prm.delay_min, &prm.delay_max) != 2 ||
          sogm::link_refuse_params(&prm))
        return 3;
      const uint64_t h = sogm::link_key(sogm::link_tick_key(prm.seed, m), j, a, n_total);
      const double   u = sogm::noise_uniform(sogm::noise_mix(h));
      std::printf("K %016" PRIx64 " %016" PRIx64 " %d %d\n", h, bits(u), sogm::link_delay(prm, h), u < prm.p_loss ? 1 : 0);
    } else if (tag[0] == 'G') {
      double x[7];
      if (!read_doubles(f, x, 7)) return 3;
      std::printf("G %d\n", sogm::link_out_of_range(x[0], x + 1, x + 4) ? 1 : 0);
    } else if (tag[0] == 'P') {
      SogmLinkParams prm{};
      double         x[2];
      if (!read_doubles(f, x, 2) || std::fscanf(f, "%d %d", &prm.delay_min, &prm.delay_max) != 2) return 3;
      prm.p_loss = x[0], prm.range = x[1];
      std::printf("P %d\n", sogm::link_refuse_params(&prm) ? 1 : 0);
    } else if (tag[0] == 'S') {
      const int rc = run_swarm(f);
      if (rc) return rc;
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
