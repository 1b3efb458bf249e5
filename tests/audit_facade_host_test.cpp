// Compiles against host/sogm_facade.hpp's Audit wrapper and checks the audit entry points' argument handling on the host:
// refused arguments give SOGM_ERR_INVALID_ARG with a sogm_last_error text; a well-formed call without a GPU returns an
// error code (no crash).  Prints "audit facade host ok".
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
  static_assert(sizeof(SogmAuditAgent) == 104 && sizeof(SogmAuditEvent) == 24 && sizeof(SogmAuditParams) == 56, "layout");
  SogmAuditParams prm{{0.4, 0.4, 0.45}, 0.01, 1.0, 0.0, 16, 0};
  // stand-in addresses: every refusal below happens before anything is read
  auto *tab = reinterpret_cast<const SogmTrajRecord *>(0x1000);
  auto *dp  = reinterpret_cast<const double *>(0x2000);
  auto *cyl = reinterpret_cast<const SogmCylinder *>(0x3000);
  auto *acc = reinterpret_cast<SogmAuditAgent *>(0x4000);
  auto *ev  = reinterpret_cast<SogmAuditEvent *>(0x5000);
  auto *nev = reinterpret_cast<int32_t *>(0x6000);
  EXPECT(sogm_swarm_audit(nullptr, tab, 1, 4, nullptr, 0, 0, 0.1, 0, 4, dp, dp, cyl, 1, acc, ev, nev, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(std::strlen(sogm_last_error()) > 0);
  EXPECT(sogm_swarm_audit(&prm, tab, 1, 4, nullptr, 0, 0, 0.1, 2, 3, dp, dp, cyl, 1, acc, ev, nev, nullptr) ==
         SOGM_ERR_INVALID_ARG);   // rows past n_total
  EXPECT(sogm_swarm_audit(&prm, tab, -1, 4, nullptr, 0, 0, 0.1, 0, 4, dp, dp, cyl, 1, acc, ev, nev, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_swarm_audit(&prm, tab, 1, 4, nullptr, 0, 0, 0.105, 0, 4, dp, dp, cyl, 1, acc, ev, nev, nullptr) ==
         SOGM_ERR_INVALID_ARG);   // 10.5 samples per tick
  EXPECT(std::strstr(sogm_last_error(), "whole") != nullptr);
  EXPECT(sogm_swarm_audit(&prm, tab, 1, 4, nullptr, 0, 0, 0.1, 0, 4, dp, dp, nullptr, 1, acc, ev, nev, nullptr) ==
         SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_audit_init_agents(nullptr, 4, nullptr) == SOGM_ERR_INVALID_ARG);
  if (sogm_device_count() == 0) {
    EXPECT(sogm_swarm_audit(&prm, tab, 1, 4, nullptr, 0, 0, 0.1, 0, 4, dp, dp, cyl, 1, acc, ev, nev, nullptr) < 0);
    EXPECT(sogm_audit_init_agents(acc, 4, nullptr) < 0);
    bool threw = false;
    try {
      sogm_host::Audit a(prm, 4);
    } catch (const std::exception &) {
      threw = true;
    }
    EXPECT(threw);
  }
  if (fails) return 1;
  std::printf("audit facade host ok\n");
  return 0;
}
