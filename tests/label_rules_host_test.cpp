// The rules of csrc/sogm_labels.hpp compiled for the host (no HIP): reads cases, prints every result as hex bits.
//   K <u32: bits of z> <code>                                    -> K <u64 key> <code decoded from the key>
//   W <n> n x (<u32: bits of z> <code>)                          -> W <u64: the smallest key> <its code>
//   S <u32: bits of min_speed> <n_cyl> <n_bodies> n_cyl x (<u64 vx> <u64 vy>) n_bodies x (3 x u64)   -> S <n_cyl> <n_bodies>
//   L <code>                                                     -> L <4 x u32: the label under the last S>
// tests/test_filter_labels_host.py holds the output to the numpy reading (tests/filter_labels_reference.py) bit for bit, and
// runs this program once more under -fsanitize=address,undefined.  The tables of S are heap arrays of exactly n_cyl records
// and 3 n_bodies doubles: a label that read beyond them would be reported there.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_labels.hpp"

template <class T, class U>
static T cast_bits(U u) {
  static_assert(sizeof(T) == sizeof(U), "same size");
  T t;
  std::memcpy(&t, &u, sizeof t);
  return t;
}

static bool read_point(FILE *f, float &z, int32_t &code) {
  uint32_t u;
  if (std::fscanf(f, "%" SCNx32 " %" SCNd32, &u, &code) != 2) return false;
  z = cast_bits<float>(u);
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<SogmCylinder> cyl;
  std::vector<double>       vel;
  SogmLabelSources          src;
  std::memset(&src, 0, sizeof src);
  static_assert(sizeof(SogmLabelSources) == 32, "SogmLabelSources is 32 bytes");
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    if (tag[0] == 'K') {
      float   z;
      int32_t code;
      if (!read_point(f, z, code)) return 3;
      const unsigned long long key = sogm::label_key(z, code);
      if (key == sogm::LABEL_KEY_EMPTY) return 4;  // (the cases are finite points)
      std::printf("K %016llx %" PRId32 "\n", key, sogm::label_key_code(key));
    } else if (tag[0] == 'W') {
      int n = 0;
      if (std::fscanf(f, "%d", &n) != 1 || n < 1) return 3;
      unsigned long long best = sogm::LABEL_KEY_EMPTY;
      for (int i = 0; i < n; ++i) {
        float   z;
        int32_t code;
        if (!read_point(f, z, code)) return 3;
        const unsigned long long key = sogm::label_key(z, code);
        best                         = key < best ? key : best;
      }
      std::printf("W %016llx %" PRId32 "\n", best, sogm::label_key_code(best));
    } else if (tag[0] == 'S') {
      uint32_t m;
      int      n_cyl = 0, n_bodies = 0;
      if (std::fscanf(f, "%" SCNx32 " %d %d", &m, &n_cyl, &n_bodies) != 3 || n_cyl < 0 || n_bodies < 0) return 3;
      cyl.assign((size_t)n_cyl, SogmCylinder{});
      cyl.shrink_to_fit();
      vel.assign((size_t)n_bodies * 3, 0.0);
      vel.shrink_to_fit();
      for (int i = 0; i < n_cyl; ++i) {
        uint64_t a, b;
        if (std::fscanf(f, "%" SCNx64 " %" SCNx64, &a, &b) != 2) return 3;
        cyl[(size_t)i].type = 3;
        cyl[(size_t)i].vx   = cast_bits<double>(a);
        cyl[(size_t)i].vy   = cast_bits<double>(b);
      }
      for (size_t i = 0; i < vel.size(); ++i) {
        uint64_t a;
        if (std::fscanf(f, "%" SCNx64, &a) != 1) return 3;
        vel[i] = cast_bits<double>(a);
      }
      src.cylinders = n_cyl ? cyl.data() : nullptr;
      src.body_vel  = n_bodies ? vel.data() : nullptr;
      src.n_cyl     = n_cyl;
      src.n_bodies  = n_bodies;
      src.min_speed = cast_bits<float>(m);
      std::printf("S %d %d\n", n_cyl, n_bodies);
    } else if (tag[0] == 'L') {
      int32_t code;
      if (std::fscanf(f, "%" SCNd32, &code) != 1) return 3;
      float l[4];
      sogm::label_of(code, src, l);
      std::printf("L %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", cast_bits<uint32_t>(l[0]),
                  cast_bits<uint32_t>(l[1]), cast_bits<uint32_t>(l[2]), cast_bits<uint32_t>(l[3]));
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
