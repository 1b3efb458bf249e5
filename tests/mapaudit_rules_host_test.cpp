// Host build of csrc/sogm_mapaudit.hpp (the bodies k_map_audit calls): reads cases from a file, prints one answer per line.
//   D L r n w[n]                         -> "D" + the row's n words dilated by r (hex)
//   O value thr                          (fp32 bits, hex) -> "O 0|1"
//   F R[9] near far tan_h tan_v (fp64 bits) res rx ry rz (fp32 bits) ix iy iz
//                                        -> "F 0|1" + the three centre coordinates (fp64 bits)
//   Y L W H r slab_layers                -> "Y row_words layer_words halo layers slabs occ_layers bytes" and the offsets' order
// tests/test_map_audit_host.py holds the output to the numpy reading (tests/map_audit_reference.py) line by line.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sogm_mapaudit.hpp"

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
static uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  return u;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 3;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string        tag;
    ss >> tag;
    if (tag == "D") {
      int L, r, n;
      ss >> L >> r >> n;
      if (n != sogm::audit_row_words(L)) return 4;
      std::vector<uint64_t> src((size_t)n), dst((size_t)n);
      for (auto &w : src) {
        std::string h;
        ss >> h;
        w = std::stoull(h, nullptr, 16);
      }
      sogm::audit_dilate_row(src.data(), dst.data(), L, r);
      std::printf("D");
      for (uint64_t w : dst) std::printf(" %016" PRIx64, w);
      std::printf("\n");
    } else if (tag == "O") {
      std::string v, t;
      ss >> v >> t;
      std::printf("O %d\n", sogm::audit_occupied(f32(v), f32(t)) ? 1 : 0);
    } else if (tag == "F") {
      sogm::AuditFrustum f;
      std::string        h;
      for (double &x : f.R) {
        ss >> h;
        x = f64(h);
      }
      ss >> h, f.near_z = f64(h);
      ss >> h, f.far_z = f64(h);
      ss >> h, f.tan_h = f64(h);
      ss >> h, f.tan_v = f64(h);
      float g[4];
      for (float &x : g) {
        ss >> h;
        x = f32(h);
      }
      int i[3];
      ss >> i[0] >> i[1] >> i[2];
      const double p0 = sogm::audit_centre(i[0], g[0], g[1]), p1 = sogm::audit_centre(i[1], g[0], g[2]),
                   p2 = sogm::audit_centre(i[2], g[0], g[3]);
      std::printf("F %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", sogm::audit_in_view(f, p0, p1, p2) ? 1 : 0, bits(p0),
                  bits(p1), bits(p2));
    } else if (tag == "Y") {
      int L, W, H, r, slab;
      ss >> L >> W >> H >> r >> slab;
      const sogm::AuditLayout a = sogm::audit_layout(L, W, H, r, slab);
      // the arrays follow each other without overlap, inside `bytes` (r = 0: the dilated rows are the rows)
      const int occ = a.occ_layers * a.layer_words;
      bool      ok  = a.region_off == 0 && a.occ_off[0] == a.layers * a.layer_words && a.occ_off[1] == a.occ_off[0] + occ;
      if (r > 0)
        ok = ok && a.xy_off[0] == a.occ_off[1] + occ && a.xy_off[1] == a.xy_off[0] + occ && (a.xy_off[1] + occ) * 8 == a.bytes;
      else
        ok = ok && a.xy_off[0] == a.occ_off[0] && a.xy_off[1] == a.occ_off[1] && (a.occ_off[1] + occ) * 8 == a.bytes;
      if (a.layers == 0) ok = a.bytes == 0 && a.slabs == 0;
      std::printf("Y %d %d %d %d %d %d %d %s\n", a.row_words, a.layer_words, a.halo, a.layers, a.slabs, a.occ_layers, a.bytes,
                  ok ? "carved" : "OVERLAP");
    } else if (!tag.empty()) {
      return 5;
    }
  }
  return 0;
}
