// The bodies of csrc/sogm_body.hpp compiled for the host (no HIP): reads cases, prints every result as hex bits.
//   V <3 x u64: centre>                                          -> V <valid>
//   B <3 x u64: centre> <3 x u64: size> <p[3]> <d[3]>            -> B <hit> <t>
// tests/test_depth_bodies_host.py holds the output to the numpy reading bit for bit, and runs this program once more under
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "sogm_body.hpp"

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

static bool read_doubles(FILE *f, double *out, int n) {
  for (int i = 0; i < n; ++i) {
    uint64_t u;
    if (std::fscanf(f, "%" SCNx64, &u) != 1) return false;
    out[i] = from_bits(u);
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    double c[3], size[3], p[3], d[3];
    if (tag[0] == 'V') {
      if (!read_doubles(f, c, 3)) return 3;
      std::printf("V %d\n", sogm::body_valid(c) ? 1 : 0);
    } else if (tag[0] == 'B') {
      if (!read_doubles(f, c, 3) || !read_doubles(f, size, 3) || !read_doubles(f, p, 3) || !read_doubles(f, d, 3)) return 3;
      if (!sogm::body_valid(c)) return 4;
      const sogm::BodyCand q = sogm::body_prepare(c, size, p, 7);
      if (q.idx != 7) return 4;
      double     t   = 0.0;
      const bool hit = sogm::body_ray_hit(q, d, t);
      std::printf("B %d %016" PRIx64 "\n", hit ? 1 : 0, bits(hit ? t : 0.0));
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
