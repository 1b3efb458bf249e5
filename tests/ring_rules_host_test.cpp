// The bodies of csrc/sogm_ring.hpp compiled for the host (no HIP): reads cases, prints every result as hex bits.
//   F <type> <11 x u64: x y z w h vx vy qw qx qy qz>            -> F <valid> [R rho e1[3] e2[3] n[3]]
//   R <type> <11 x u64> <p[3]> <d[3]>                           -> R <hit> <t>
//   T                                                            -> T <128 x u64>
//   G <type> <11 x u64> <a[3]> <body[3]>                        -> G <gap>
// tests/test_ring_rules_host.py holds the output to the numpy readings bit for bit, and runs this program once more under
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "sogm_ring.hpp"

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

static bool read_record(FILE *f, SogmCylinder &c) {
  int    type;
  double v[11];
  if (std::fscanf(f, "%d", &type) != 1 || !read_doubles(f, v, 11)) return false;
  c      = SogmCylinder{};
  c.type = type;
  c.x = v[0], c.y = v[1], c.z = v[2], c.w = v[3], c.h = v[4], c.vx = v[5], c.vy = v[6];
  c.qw = v[7], c.qx = v[8], c.qy = v[9], c.qz = v[10];
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<double> tab_store(sogm::RING_TABLE * 2);
  double(*tab)[2] = reinterpret_cast<double(*)[2]>(tab_store.data());
  sogm::ring_table_fill(tab);
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    SogmCylinder    c;
    sogm::RingFrame fr;
    if (tag[0] == 'T') {
      std::printf("T");
      for (int i = 0; i < sogm::RING_TABLE; ++i) std::printf(" %016" PRIx64 " %016" PRIx64, bits(tab[i][0]), bits(tab[i][1]));
      std::printf("\n");
    } else if (tag[0] == 'F') {
      if (!read_record(f, c)) return 3;
      if (!sogm::ring_frame(c, fr)) {
        std::printf("F 0\n");
        continue;
      }
      std::printf("F 1 %016" PRIx64 " %016" PRIx64, bits(fr.R), bits(fr.rho));
      for (int i = 0; i < 3; ++i) std::printf(" %016" PRIx64, bits(fr.e1[i]));
      for (int i = 0; i < 3; ++i) std::printf(" %016" PRIx64, bits(fr.e2[i]));
      for (int i = 0; i < 3; ++i) std::printf(" %016" PRIx64, bits(fr.n[i]));
      std::printf("\n");
    } else if (tag[0] == 'R') {
      double p[3], d[3];
      if (!read_record(f, c) || !read_doubles(f, p, 3) || !read_doubles(f, d, 3)) return 3;
      if (!sogm::ring_frame(c, fr)) return 4;
      const double         centre[3] = {c.x, c.y, c.z};
      const sogm::RingCand q = sogm::ring_ray_prepare(fr, centre, p);
      double               t   = 0.0;
      const bool           hit = sogm::ring_ray_hit(q, d, std::numeric_limits<double>::infinity(), t);
      std::printf("R %d %016" PRIx64 "\n", hit ? 1 : 0, bits(hit ? t : 0.0));
    } else if (tag[0] == 'G') {
      double a[3], body[3];
      if (!read_record(f, c) || !read_doubles(f, a, 3) || !read_doubles(f, body, 3)) return 3;
      if (!sogm::ring_frame(c, fr)) return 4;
      sogm::RingBody r;
      r.c[0] = c.x, r.c[1] = c.y, r.c[2] = c.z, r.R = fr.R, r.rho = fr.rho;
      for (int i = 0; i < 3; ++i) r.e1[i] = fr.e1[i], r.e2[i] = fr.e2[i];
      std::printf("G %016" PRIx64 "\n", bits(sogm::ring_box_gap(r, a, body, tab)));
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
