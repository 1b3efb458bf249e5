// Compiles against host/sogm_facade.hpp's Links, RiskMap::addOtherAgentsViews / updateWorldViews and Planner::setSwarmViews.
// Without a GPU: the default parameters are perfect links, a bad parameter set is refused with the rule's text, and Links
// cannot be built (it throws).  With one: three receivers on perfect links get every tick's table, a uniform delay of one
// tick hands them the table of the tick before, and ticks out of order are refused.  Prints "links facade ok".
#include <cstdio>
#include <cstring>
#include <vector>

#include "sogm_facade.hpp"

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);  \
      ++fails;                                                 \
    }                                                          \
  } while (0)

// the signatures the facade forwards to (never called here: a context needs a scene)
using ViewsOverlay = void (sogm_host::RiskMap::*)(const SogmTrajRecord *, int, const int32_t *, hipStream_t);
using ViewsUpdate  = void (sogm_host::RiskMap::*)(const SogmWorld &, const float *, const double *, const SogmTrajRecord *, int,
                                                  const int32_t *, hipStream_t);
using ViewsSwarm   = void (sogm_host::Planner::*)(const SogmTrajRecord *, int, const int32_t *, const double *);
static ViewsOverlay f_overlay = &sogm_host::RiskMap::addOtherAgentsViews;
static ViewsUpdate  f_update  = &sogm_host::RiskMap::updateWorldViews;
static ViewsSwarm   f_swarm   = &sogm_host::Planner::setSwarmViews;

static std::vector<SogmTrajRecord> table_of(int n, int tick) {
  std::vector<SogmTrajRecord> t((size_t)n);
  for (int j = 0; j < n; ++j) {
    std::memset(&t[j], 0, sizeof(SogmTrajRecord));
    t[j].drone_id   = j;
    t[j].n_pieces   = 1 + j;
    t[j].time_start = 0.1 * tick;
    for (int i = 0; i < SOGM_MAX_PIECES * 15; ++i) t[j].cpts[i] = tick * 1000.0 + j * 10.0 + i * 1e-3;
  }
  return t;
}

int main() {
  static_assert(sizeof(SogmLinkParams) == 40 && sizeof(SogmLinkBuffers) == 40, "layout");
  EXPECT(f_overlay && f_update && f_swarm);
  const SogmLinkParams perfect = sogm_host::Links::defaultParams();
  const SogmLinkParams zero{};
  EXPECT(std::memcmp(&perfect, &zero, sizeof(zero)) == 0);
  SogmLinkParams bad = perfect;
  bad.delay_max      = SOGM_LINK_MAX_DELAY + 1;
  bool threw         = false;
  try {
    sogm_host::Links l(bad, 3, 0, 3);
  } catch (const std::exception &e) {
    threw = true;
  }
  EXPECT(threw);
  const SogmLinkBuffers fake{reinterpret_cast<SogmTrajRecord *>(0x1000), nullptr, reinterpret_cast<SogmTrajRecord *>(0x1000),
                             reinterpret_cast<int32_t *>(0x1000), reinterpret_cast<int64_t *>(0x1000)};
  EXPECT(sogm_link_init(&bad, 3, 3, &fake, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_link_init") && std::strstr(sogm_last_error(), "SOGM_LINK_MAX_DELAY"));
  if (sogm_device_count() == 0) {
    EXPECT(sogm_link_init(&perfect, 3, 3, &fake, nullptr) == SOGM_ERR_NO_DEVICE);
    threw = false;
    try {
      sogm_host::Links l(perfect, 3, 0, 3);
    } catch (const std::exception &e) {
      threw = true;
    }
    EXPECT(threw);
  } else {
    const int                       n = 3;
    sogm_host::DevBuf<SogmTrajRecord> dev((size_t)n);
    std::vector<SogmTrajRecord>     got((size_t)n * n);
    {
      sogm_host::Links l(perfect, n, 0, n);
      for (int k = 0; k < 3; ++k) {
        const auto t = table_of(n, k);
        dev.put(t.data(), t.size());
        const SogmTrajRecord *views = l.deliver(k, dev.data(), nullptr);
        EXPECT(views == l.views());
        (void)hipDeviceSynchronize();
        (void)hipMemcpy(got.data(), views, got.size() * sizeof(SogmTrajRecord), hipMemcpyDeviceToHost);
        for (int a = 0; a < n; ++a) EXPECT(std::memcmp(&got[(size_t)a * n], t.data(), sizeof(SogmTrajRecord) * n) == 0);
      }
      const auto c = l.counters();
      EXPECT(c.size() == (size_t)n * SOGM_LINK_COUNTERS && c[0] == 3 * (n - 1) && c[3] == 3 * (n - 1) && c[4] == 3 * (n - 1));
      EXPECT(c[1] == 0 && c[2] == 0 && c[5] == 0 && c[6] == 0 && c[7] == 0);
      threw = false;
      try {
        l.deliver(5, dev.data(), nullptr);
      } catch (const std::logic_error &) {
        threw = true;
      }
      EXPECT(threw);
    }
    {
      SogmLinkParams late = perfect;
      late.delay_min = late.delay_max = 1;
      sogm_host::Links l(late, n, 0, n);
      for (int k = 0; k < 3; ++k) {
        const auto t = table_of(n, k);
        dev.put(t.data(), t.size());
        l.deliver(k, dev.data(), nullptr);
      }
      (void)hipDeviceSynchronize();
      (void)hipMemcpy(got.data(), l.views(), got.size() * sizeof(SogmTrajRecord), hipMemcpyDeviceToHost);
      const auto now = table_of(n, 2), before = table_of(n, 1);
      for (int a = 0; a < n; ++a)
        for (int j = 0; j < n; ++j)
          EXPECT(std::memcmp(&got[(size_t)a * n + j], j == a ? &now[j] : &before[j], sizeof(SogmTrajRecord)) == 0);
      const auto h = l.heldTicks();
      EXPECT(h[0] == 2 && h[1] == 1 && h[2] == 1);
    }
  }
  if (fails) return 1;
  std::printf("links facade ok\n");
  return 0;
}
