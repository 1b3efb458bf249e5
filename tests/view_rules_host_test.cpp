// Host build of csrc/sogm_viewmask.hpp (the body k_view_mask calls): reads cases from a file (or stdin), prints two lines per
// case.  One case per line:
//   V L W H  res rx ry rz (fp32 bits)  R[9] (fp64 bits)  has_off off[3] (fp64 bits)
//     fx fy cx cy depth_scale near far tan_h tan_v band (fp64 bits)  rows cols classes  depth[rows * cols] (hex)
//   -> "C" + one digit per cell, the class, cells in [z][y][x] order
//   -> "W" + the mask's words [z][y][word] (hex) + "N" + the five class counts and the mask's bits
// tests/test_view_mask_host.py holds the output to the numpy reading (tests/view_mask_reference.py) character by character.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sogm_viewmask.hpp"

static double f64(const std::string &h) {
  const uint64_t u = std::stoull(h, nullptr, 16);
  double         d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}
static float f32(const std::string &h) {
  const uint32_t u = (uint32_t)std::stoul(h, nullptr, 16);
  float          f;
  std::memcpy(&f, &u, sizeof f);
  return f;
}

static int run(std::istream &in) {
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string        tag, h;
    ss >> tag;
    if (tag.empty()) continue;
    if (tag != "V") return 5;
    int L, W, H;
    ss >> L >> W >> H;
    float g[4];
    for (float &x : g) ss >> h, x = f32(h);
    sogm::AuditFrustum f;
    for (double &x : f.R) ss >> h, x = f64(h);
    int    has_off;
    double off[3];
    ss >> has_off;
    for (double &x : off) ss >> h, x = f64(h);
    sogm::ViewCamera c;
    ss >> h, c.fx = f64(h);
    ss >> h, c.fy = f64(h);
    ss >> h, c.cx = f64(h);
    ss >> h, c.cy = f64(h);
    ss >> h, c.depth_scale = f64(h);
    ss >> h, f.near_z = f64(h);
    ss >> h, f.far_z = f64(h);
    ss >> h, f.tan_h = f64(h);
    ss >> h, f.tan_v = f64(h);
    ss >> h, c.band = f64(h);
    int classes;
    ss >> c.rows >> c.cols >> classes;
    if (!ss || L < 1 || W < 1 || H < 1 || c.rows < 1 || c.cols < 1) return 4;
    std::vector<uint16_t> depth((size_t)c.rows * c.cols);
    for (auto &d : depth) {
      if (!(ss >> h)) return 6;
      d = (uint16_t)std::stoul(h, nullptr, 16);
    }
    const int             nw = sogm::audit_row_words(L);
    std::vector<uint64_t> words((size_t)sogm::view_mask_words(L, W, H), 0);
    long long             n[6] = {0, 0, 0, 0, 0, 0};
    std::string           cls;
    for (int z = 0; z < H; ++z)
      for (int y = 0; y < W; ++y)
        for (int x = 0; x < L; ++x) {
          const int k = sogm::view_class(f, c, depth.data(), sogm::view_centre(x, g[0], g[1], has_off != 0, off[0]),
                                         sogm::view_centre(y, g[0], g[2], has_off != 0, off[1]),
                                         sogm::view_centre(z, g[0], g[3], has_off != 0, off[2]));
          cls.push_back((char)('0' + k));
          n[k]++;
          if ((classes >> k) & 1) {
            words[((size_t)z * W + y) * nw + (x >> 6)] |= (uint64_t)1 << (x & 63);
            n[5]++;
          }
        }
    for (int w = 0; w < nw; ++w)  // the layout's own statement of the spare bits
      for (size_t row = 0; row < (size_t)W * H; ++row)
        if (words[row * nw + w] & ~sogm::audit_row_mask(L, w)) return 7;
    std::printf("C %s\nW", cls.c_str());
    for (uint64_t w : words) std::printf(" %016" PRIx64, w);
    std::printf(" N %lld %lld %lld %lld %lld %lld\n", n[0], n[1], n[2], n[3], n[4], n[5]);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return run(std::cin);
  std::ifstream in(argv[1]);
  if (!in) return 3;
  return run(in);
}
