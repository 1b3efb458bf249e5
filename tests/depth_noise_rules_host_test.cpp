// The bodies of csrc/sogm_depthnoise.hpp compiled for the host (no HIP): reads cases, prints every result as hex bits.
//   M <u64 x>                                         -> M <mix(x)>
//   K <u64 seed> <u64 frame> <u64 g>                  -> K <h> <S decimal> <n bits>
//   R <u64 seed> <u64 frame> <u64 g0> <count dec>     -> count lines  R <U(w_0) bits> <U(w_1) bits> <n bits>
//   I <fx fy cx cy max_depth depth_scale: 6 x u64 bits> <rows cols dec> <seed frame: u64> <agent_base dec>
//     <sigma0 sigma1 sigma2 p_drop edge_jump p_edge min_depth: 7 x u64 bits> <n_agents dec> <with_hit 0|1>
//     then n_agents*rows*cols pixels: <d16 hex> [<hit as u32 hex>]
//                                                     -> per agent  C <6 counters decimal>, then per pixel
//                                                        P <d16' hex> <x y z as u32 bits> [<hit' as u32 hex>]
// tests/test_depth_noise_host.py holds the output to the numpy reading bit for bit, and runs this program once more under
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_depthnoise.hpp"

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
static uint32_t bits32(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
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

static int run_image(FILE *f) {
  SogmDepthCamera cam{};
  SogmDepthNoise  prm{};
  double          c[6], p[7];
  uint64_t        sf[2];
  int             n_agents = 0, with_hit = 0;
  if (!read_doubles(f, c, 6) || std::fscanf(f, "%d %d", &cam.rows, &cam.cols) != 2 || !read_u64(f, sf, 2) ||
      std::fscanf(f, "%d", &prm.agent_base) != 1 || !read_doubles(f, p, 7) || std::fscanf(f, "%d %d", &n_agents, &with_hit) != 2)
    return 3;
  cam.fx = c[0], cam.fy = c[1], cam.cx = c[2], cam.cy = c[3], cam.max_depth = c[4], cam.depth_scale = c[5];
  prm.seed = sf[0], prm.frame = sf[1];
  prm.sigma0 = p[0], prm.sigma1 = p[1], prm.sigma2 = p[2], prm.p_drop = p[3], prm.edge_jump = p[4], prm.p_edge = p[5];
  prm.min_depth = p[6];
  if (cam.rows < 1 || cam.cols < 1 || n_agents < 1) return 3;
  const size_t          n = (size_t)cam.rows * (size_t)cam.cols;
  std::vector<uint16_t> in(n * (size_t)n_agents);
  std::vector<int32_t>  hit(with_hit ? in.size() : 0);
  for (size_t i = 0; i < in.size(); ++i) {
    unsigned d = 0, h = 0;
    if (std::fscanf(f, "%x", &d) != 1 || d > 0xFFFFu) return 3;
    if (with_hit && std::fscanf(f, "%x", &h) != 1) return 3;
    in[i] = (uint16_t)d;
    if (with_hit) hit[i] = (int32_t)h;
  }
  const uint64_t fk = sogm::noise_frame_key(prm.seed, prm.frame);
  for (int a = 0; a < n_agents; ++a) {
    const uint16_t       *img = in.data() + (size_t)a * n;
    std::vector<uint16_t> out(n);
    long long             cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int v = 0; v < cam.rows; ++v)
      for (int u = 0; u < cam.cols; ++u) {
        const uint16_t d16   = img[(size_t)v * cam.cols + u];
        const uint64_t h     = sogm::noise_pixel_key(fk, sogm::noise_pixel_index(prm.agent_base, a, cam.rows, cam.cols, v, u));
        auto           fetch = [&](int vn, int un) { return img[(size_t)vn * cam.cols + un]; };
        auto           edge  = [&]() {
          return sogm::noise_is_edge(fetch, v, u, cam.rows, cam.cols, d16, cam.depth_scale, prm.edge_jump);
        };
        const int outcome = sogm::noise_pixel(cam, prm, h, d16, edge, out[(size_t)v * cam.cols + u]);
        if (outcome != sogm::NOISE_NO_INPUT) {
          ++cnt[0];
          ++cnt[outcome];
        }
      }
    std::printf("C %lld %lld %lld %lld %lld %lld\n", cnt[0], cnt[1], cnt[2], cnt[3], cnt[4], cnt[5]);
    for (int v = 0; v < cam.rows; ++v)
      for (int u = 0; u < cam.cols; ++u) {
        const size_t i = (size_t)v * cam.cols + u;
        float        xyz[3];
        sogm::noise_backproject(cam, v, u, out[i], xyz);
        std::printf("P %04x %08x %08x %08x", (unsigned)out[i], bits32(xyz[0]), bits32(xyz[1]), bits32(xyz[2]));
        if (with_hit) std::printf(" %08x", (unsigned)(out[i] ? hit[(size_t)a * n + i] : (int32_t)SOGM_HIT_NONE));
        std::printf("\n");
      }
  }
  return 0;
}

int main(int argc, char **argv) {
  static_assert(sizeof(SogmDepthNoise) == 80, "layout");
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  char tag[8];
  while (std::fscanf(f, "%7s", tag) == 1) {
    uint64_t x[3];
    if (tag[0] == 'M') {
      if (!read_u64(f, x, 1)) return 3;
      std::printf("M %016" PRIx64 "\n", sogm::noise_mix(x[0]));
    } else if (tag[0] == 'K') {
      if (!read_u64(f, x, 3)) return 3;
      const uint64_t h = sogm::noise_pixel_key(sogm::noise_frame_key(x[0], x[1]), x[2]);
      std::printf("K %016" PRIx64 " %u %016" PRIx64 "\n", h, (unsigned)sogm::noise_sum(h), bits(sogm::noise_normal(h)));
    } else if (tag[0] == 'R') {
      long long count = 0;
      if (!read_u64(f, x, 3) || std::fscanf(f, "%lld", &count) != 1 || count < 0) return 3;
      const uint64_t fk = sogm::noise_frame_key(x[0], x[1]);
      for (long long i = 0; i < count; ++i) {
        const uint64_t h = sogm::noise_pixel_key(fk, x[2] + (uint64_t)i);
        std::printf("R %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(sogm::noise_uniform(sogm::noise_draw(h, 0))),
                    bits(sogm::noise_uniform(sogm::noise_draw(h, 1))), bits(sogm::noise_normal(h)));
      }
    } else if (tag[0] == 'I') {
      const int rc = run_image(f);
      if (rc) return rc;
    } else {
      return 5;
    }
  }
  std::fclose(f);
  return 0;
}
