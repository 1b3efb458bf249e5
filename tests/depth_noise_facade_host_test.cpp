// Compiles against host/sogm_facade.hpp's GridMap::addDepthNoise and checks sogm_depth_noise's argument handling on the
// host: every refusal with the rule sogm_last_error() names; a well-formed call without a GPU is SOGM_ERR_NO_DEVICE, which
// the facade throws.  Prints "depth noise facade host ok".
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

// stand-in addresses: every refusal below happens before anything is read
static auto *in  = reinterpret_cast<const uint16_t *>(0x100000);
static auto *out = reinterpret_cast<uint16_t *>(0x900000);
static auto *pts = reinterpret_cast<float *>(0x4000000);
static auto *hin = reinterpret_cast<int32_t *>(0x8000000);
static auto *cnt = reinterpret_cast<int32_t *>(0x5000);

static bool refused(const SogmDepthCamera &cam, const SogmDepthNoise &n, const char *rule) {
  const int rc = sogm_depth_noise(&cam, &n, 1, in, hin, out, pts, hin, cnt, nullptr);
  return rc == SOGM_ERR_INVALID_ARG && std::strstr(sogm_last_error(), "sogm_depth_noise") && std::strstr(sogm_last_error(), rule);
}

int main() {
  static_assert(sizeof(SogmDepthNoise) == 80, "layout");
  const SogmDepthCamera cam{387.0, 387.0, 320.0, 240.0, 5.0, 1000.0, 0.0, 480, 640, 1, 0};
  const SogmDepthNoise  ok{0x5067, 3, 0, 0, 0.002, 0.003, 0.004, 0.05, 0.15, 0.5, 0.3};
  // null pointers
  EXPECT(sogm_depth_noise(nullptr, &ok, 1, in, hin, out, pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_depth_noise: null pointer") != nullptr);
  EXPECT(sogm_depth_noise(&cam, nullptr, 1, in, hin, out, pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_depth_noise(&cam, &ok, 1, nullptr, hin, out, pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_depth_noise(&cam, &ok, 1, in, hin, nullptr, pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_depth_noise(&cam, &ok, 1, in, hin, out, pts, hin, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_depth_noise(&cam, &ok, 0, in, hin, out, pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  // the camera's
  SogmDepthCamera far = cam;
  far.max_depth       = 70.0;
  EXPECT(refused(far, ok, "65535"));
  far       = cam;
  far.rows  = 0;
  EXPECT(refused(far, ok, "rows"));
  far    = cam;
  far.fx = 0.0;
  EXPECT(refused(far, ok, "positive"));
  far    = cam;
  far.cx = NAN;
  EXPECT(refused(far, ok, "finite"));
  // out_hit without in_hit
  EXPECT(sogm_depth_noise(&cam, &ok, 1, in, nullptr, out, pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "out_hit without in_hit") != nullptr);
  // the parameters
  SogmDepthNoise bad = ok;
  bad.sigma1         = INFINITY;
  EXPECT(refused(cam, bad, "finite"));
  bad           = ok;
  bad.min_depth = NAN;
  EXPECT(refused(cam, bad, "finite"));
  bad        = ok;
  bad.sigma2 = -1e-9;
  EXPECT(refused(cam, bad, ">= 0"));
  bad           = ok;
  bad.edge_jump = -0.1;
  EXPECT(refused(cam, bad, ">= 0"));
  bad           = ok;
  bad.min_depth = -0.1;
  EXPECT(refused(cam, bad, ">= 0"));
  bad        = ok;
  bad.p_drop = 1.5;
  EXPECT(refused(cam, bad, "[0, 1]"));
  bad        = ok;
  bad.p_edge = -0.5;
  EXPECT(refused(cam, bad, "[0, 1]"));
  bad            = ok;
  bad.agent_base = -1;
  EXPECT(refused(cam, bad, "agent_base"));
  // in place, and overlapping by one pixel at either end
  const size_t n = 480 * 640;
  EXPECT(sogm_depth_noise(&cam, &ok, 1, in, hin, const_cast<uint16_t *>(in), pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "overlaps") != nullptr);
  EXPECT(sogm_depth_noise(&cam, &ok, 1, in, hin, const_cast<uint16_t *>(in) + (n - 1), pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_depth_noise(&cam, &ok, 1, in + (n - 1), hin, const_cast<uint16_t *>(in), pts, hin, cnt, nullptr) == SOGM_ERR_INVALID_ARG);
  bool threw = false;
  try {
    sogm_host::GridMap::addDepthNoise(cam, bad, 1, in, nullptr, out, nullptr, nullptr, cnt);
  } catch (const std::exception &e) {
    threw = std::strstr(e.what(), "sogm_depth_noise") != nullptr;
  }
  EXPECT(threw);
  if (sogm_device_count() == 0) {
    EXPECT(sogm_depth_noise(&cam, &ok, 1, in, hin, out, pts, hin, cnt, nullptr) == SOGM_ERR_NO_DEVICE);
    // adjacent buffers, no cloud, no hit, the identity's parameters, flags that are ignored
    SogmDepthNoise zero{};
    zero.flags = 0x70;
    EXPECT(sogm_depth_noise(&cam, &zero, 1, in, nullptr, const_cast<uint16_t *>(in) + n, nullptr, nullptr, cnt, nullptr) ==
           SOGM_ERR_NO_DEVICE);
    threw = false;
    try {
      sogm_host::GridMap::addDepthNoise(cam, ok, 4, in, hin, out, nullptr, hin, cnt);
    } catch (const std::exception &e) {
      threw = std::strstr(e.what(), "-2") != nullptr;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("depth noise facade host ok\n");
  return 0;
}
