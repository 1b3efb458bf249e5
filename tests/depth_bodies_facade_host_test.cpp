// Compiles against host/sogm_facade.hpp's GridMap::renderDepthSwarm and checks sogm_render_depth_swarm's argument
// handling on the host: sogm_render_depth's refusals first, then the bodies'; a well-formed call without a GPU is
// SOGM_ERR_NO_DEVICE, which the facade throws.  Prints "depth bodies facade host ok".
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sogm_facade.hpp"

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);  \
      ++fails;                                                 \
    }                                                          \
  } while (0)

int main() {
  static_assert(sizeof(SogmDepthBodies) == 48, "layout");
  static_assert(SOGM_HIT_GROUND == -1 && SOGM_HIT_NONE == -2, "codes");
  SogmDepthCamera cam{387.0, 387.0, 320.0, 240.0, 5.0, 1000.0, 0.0, 480, 640, 1, 0};
  // stand-in addresses: every refusal below happens before anything is read
  auto *cyl = reinterpret_cast<const SogmCylinder *>(0x1000);
  auto *dp  = reinterpret_cast<const double *>(0x2000);
  auto *img = reinterpret_cast<uint16_t *>(0x3000);
  auto *pts = reinterpret_cast<float *>(0x4000);
  auto *cnt = reinterpret_cast<int32_t *>(0x5000);
  auto *hit = reinterpret_cast<int32_t *>(0x6000);
  const SogmWorld w = sogm_host::RiskMap::world(nullptr, 0, nullptr, 256, cyl, 3);
  SogmDepthBodies b{dp, nullptr, {0.4, 0.4, 0.45}, 8, 0};
  EXPECT(sogm_render_depth_swarm(nullptr, &cam, &b, 1, dp, dp, img, pts, hit, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_render_depth_swarm") != nullptr);
  EXPECT(sogm_render_depth_swarm(&w, &cam, &b, 0, dp, dp, img, pts, hit, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_render_depth_swarm(&w, &cam, &b, 1, dp, dp, nullptr, pts, hit, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  SogmDepthBodies bad = b;
  bad.n_bodies = -1;
  EXPECT(sogm_render_depth_swarm(&w, &cam, &bad, 1, dp, dp, img, pts, hit, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  bad     = b;
  bad.pos = nullptr;
  EXPECT(sogm_render_depth_swarm(&w, &cam, &bad, 1, dp, dp, img, pts, hit, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  bad         = b;
  bad.size[2] = 0.0;
  EXPECT(sogm_render_depth_swarm(&w, &cam, &bad, 1, dp, dp, img, pts, hit, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  bad.size[2] = INFINITY;
  bool threw  = false;
  try {
    sogm_host::GridMap::renderDepthSwarm(w, cam, &bad, 1, dp, dp, img, nullptr, nullptr, cnt);
  } catch (const std::exception &e) {
    threw = std::strstr(e.what(), "sogm_render_depth_swarm") != nullptr;
  }
  EXPECT(threw);
  if (sogm_device_count() == 0) {
    EXPECT(sogm_render_depth_swarm(&w, &cam, &b, 1, dp, dp, img, pts, hit, cnt, nullptr) == SOGM_ERR_NO_DEVICE);
    EXPECT(sogm_render_depth_swarm(&w, &cam, nullptr, 1, dp, dp, img, nullptr, nullptr, cnt, nullptr) == SOGM_ERR_NO_DEVICE);
    threw = false;
    try {
      sogm_host::GridMap::renderDepthSwarm(w, cam, &b, 4, dp, dp, img, nullptr, hit, cnt);   // (no cloud)
    } catch (const std::exception &e) {
      threw = std::strstr(e.what(), "-2") != nullptr;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("depth bodies facade host ok\n");
  return 0;
}
