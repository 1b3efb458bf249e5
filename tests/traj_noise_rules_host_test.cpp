// The rules of csrc/sogm_trajnoise.hpp compiled for the host (no HIP): reads cases, prints every result.  Numbers are hex
// uint64 (doubles as their bits) unless marked dec.
//   M <x>                                            -> M <mix(x)>
//   K <seed> <tag> <x> <j>                           -> K <key> <N at c = 0, 1, 2 as bits>
//   H <prm> <m dec> <j dec>                          -> H <shift x, y, z, tau as bits>
//   P <prm>                                          -> P <refused 0|1>
//   R <prm> <m dec> <j dec> <258 words of the row>   -> R <258 words of the noisy row> <shift x, y, z, tau as bits>
//   I ...as R...                                     -> the same, computed in place (out == in)
// <prm> = <seed> <sigma_loc x y z bits> <sigma_time bits> <sigma_track bits> <loc_hold dec>
// tests/test_traj_noise_rules_host.py holds the output to tests/traj_noise_reference.py, and runs this program once more
// under -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "sogm_trajnoise.hpp"

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
static bool read_prm(FILE *f, SogmTrajNoise *prm) {
  uint64_t u[6];
  if (!read_u64(f, u, 6) || std::fscanf(f, "%d", &prm->loc_hold) != 1) return false;
  prm->seed = u[0];
  for (int c = 0; c < 3; ++c) prm->sigma_loc[c] = from_bits(u[1 + c]);
  prm->sigma_time = from_bits(u[4]), prm->sigma_track = from_bits(u[5]);
  prm->reserved_ = 0;
  return true;
}

int main(int argc, char **argv) {
  static_assert(sizeof(SogmTrajNoise) == 56 && sizeof(SogmTrajRecord) == 2064 && sogm::TRAJ_WORDS == 258, "layout");
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    SogmTrajNoise prm{};
    if (tag[0] == 'M') {
      uint64_t x;
      if (!read_u64(f, &x, 1)) return 3;
      std::printf("M %016" PRIx64 "\n", sogm::noise_mix(x));
    } else if (tag[0] == 'K') {
      uint64_t x[4];
      if (!read_u64(f, x, 4)) return 3;
      const uint64_t k = sogm::trajnoise_key(x[0], x[1], x[2], x[3]);
      std::printf("K %016" PRIx64, k);
      for (int c = 0; c < 3; ++c) std::printf(" %016" PRIx64, bits(sogm::trajnoise_draw(k, c)));
      std::printf("\n");
    } else if (tag[0] == 'H') {
      int m, j;
      if (!read_prm(f, &prm) || std::fscanf(f, "%d %d", &m, &j) != 2 || sogm::trajnoise_refuse_params(&prm)) return 3;
      double s[4];
      sogm::trajnoise_shift(prm, m, j, s);
      std::printf("H %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(s[0]), bits(s[1]), bits(s[2]), bits(s[3]));
    } else if (tag[0] == 'P') {
      if (!read_prm(f, &prm)) return 3;
      std::printf("P %d\n", sogm::trajnoise_refuse_params(&prm) ? 1 : 0);
    } else if (tag[0] == 'R' || tag[0] == 'I') {
      int m, j;
      if (!read_prm(f, &prm) || std::fscanf(f, "%d %d", &m, &j) != 2 || sogm::trajnoise_refuse_params(&prm)) return 3;
      alignas(16) SogmTrajRecord in, out;
      uint64_t                   w[sogm::TRAJ_WORDS];
      if (!read_u64(f, w, sogm::TRAJ_WORDS)) return 3;
      std::memcpy(&in, w, sizeof(in));
      double s[4];
      if (sogm::trajnoise_refuse(&prm, m, &in, 1, &out)) return 3;
      if (tag[0] == 'I') {
        sogm::trajnoise_record(prm, m, j, &in, &in, s);
        std::memcpy(w, &in, sizeof(in));
      } else {
        sogm::trajnoise_record(prm, m, j, &in, &out, s);
        std::memcpy(w, &out, sizeof(out));
      }
      std::printf("%c", tag[0]);
      for (int q = 0; q < sogm::TRAJ_WORDS; ++q) std::printf(" %" PRIx64, w[q]);
      for (int i = 0; i < 4; ++i) std::printf(" %016" PRIx64, bits(s[i]));
      std::printf("\n");
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
