// Compiles against host/sogm_facade.hpp's GridMap::renderDepth and checks sogm_render_depth's argument handling on the
// host: refused arguments give SOGM_ERR_INVALID_ARG with a sogm_last_error text before anything is read; a well-formed call
// without a GPU is SOGM_ERR_NO_DEVICE, which the facade throws.  Prints "depth facade host ok".
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
  static_assert(sizeof(SogmDepthCamera) == 72, "layout");
  SogmDepthCamera cam{387.0, 387.0, 320.0, 240.0, 5.0, 1000.0, 0.0, 480, 640, 1, 0};
  // stand-in addresses: every refusal below happens before anything is read
  auto *cyl = reinterpret_cast<const SogmCylinder *>(0x1000);
  auto *dp  = reinterpret_cast<const double *>(0x2000);
  auto *img = reinterpret_cast<uint16_t *>(0x3000);
  auto *pts = reinterpret_cast<float *>(0x4000);
  auto *cnt = reinterpret_cast<int32_t *>(0x5000);
  const SogmWorld w = sogm_host::RiskMap::world(nullptr, 0, nullptr, 256, cyl, 3);
  EXPECT(sogm_render_depth(nullptr, &cam, 1, dp, dp, img, pts, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_render_depth") != nullptr);
  EXPECT(sogm_render_depth(&w, &cam, 0, dp, dp, img, pts, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_render_depth(&w, &cam, 1, dp, dp, nullptr, pts, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  SogmDepthCamera far = cam;
  far.max_depth = 70.0;   // 70 000 does not fit the uint16 image
  EXPECT(sogm_render_depth(&w, &far, 1, dp, dp, img, pts, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  bool threw = false;
  try {
    sogm_host::GridMap::renderDepth(w, far, 1, dp, dp, img, nullptr, cnt);
  } catch (const std::exception &e) {
    threw = std::strstr(e.what(), "sogm_render_depth") != nullptr;
  }
  EXPECT(threw);
  if (sogm_device_count() == 0) {
    EXPECT(sogm_render_depth(&w, &cam, 1, dp, dp, img, pts, cnt, nullptr) == SOGM_ERR_NO_DEVICE);
    threw = false;
    try {
      sogm_host::GridMap::renderDepth(w, cam, 4, dp, dp, img, nullptr, cnt);   // (no cloud)
    } catch (const std::exception &e) {
      threw = std::strstr(e.what(), "-2") != nullptr;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("depth facade host ok\n");
  return 0;
}
