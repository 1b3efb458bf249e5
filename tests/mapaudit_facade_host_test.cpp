// Compiles against host/sogm_facade.hpp's RiskMap::auditParams / auditAgainst and checks sogm_map_audit's argument handling
// on the host: null pointers and prm's own fields are refused before anything else; a well-formed call without a GPU is
// SOGM_ERR_NO_DEVICE.  With a GPU the facade audits two one-agent maps adopted from map/future_risk messages.
// Prints "map audit facade host ok".
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
  static_assert(sizeof(SogmMapAuditParams) == 208, "layout");
  static_assert(sizeof(SogmMapAuditRow) == 32, "layout");
  static_assert(SOGM_MAPAUDIT_CENTRE == 1 && SOGM_MAPAUDIT_SKIPPED == 2 && SOGM_MAPAUDIT_FRUSTUM == 1, "codes");
  SogmMapAuditParams prm;
  EXPECT(sogm_map_audit_default_params(6, 4, &prm) == SOGM_OK);
  EXPECT(prm.slice_map[3] == 3 && prm.slice_map[4] == -1 && prm.slice_map[31] == -1 && prm.tolerance == 0 && prm.flags == 0);
  EXPECT(sogm_map_audit_default_params(6, 4, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_map_audit_default_params(33, 4, &prm) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_map_audit_default_params(6, 6, &prm) == SOGM_OK);
  // stand-in addresses: every refusal below happens before anything is read
  auto *ctx = reinterpret_cast<sogm_ctx *>(0x1000);
  auto *rot = reinterpret_cast<const double *>(0x2000);
  auto *out = reinterpret_cast<SogmMapAuditRow *>(0x3000);
  EXPECT(sogm_map_audit(nullptr, ctx, &prm, nullptr, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_map_audit") != nullptr);
  EXPECT(sogm_map_audit(ctx, nullptr, &prm, nullptr, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_map_audit(ctx, ctx, nullptr, nullptr, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(sogm_map_audit(ctx, ctx, &prm, nullptr, nullptr, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  SogmMapAuditParams bad = prm;
  bad.tolerance = 4;
  EXPECT(sogm_map_audit(ctx, ctx, &bad, nullptr, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  bad       = prm;
  bad.flags = SOGM_MAPAUDIT_FRUSTUM;
  bad.far_z = 5.0, bad.tan_h = 1.0, bad.tan_v = 1.0;
  EXPECT(sogm_map_audit(ctx, ctx, &bad, nullptr, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);   // no cam_rot
  bad.tan_v = NAN;
  EXPECT(sogm_map_audit(ctx, ctx, &bad, rot, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  bad.tan_v = 1.0, bad.far_z = 0.0;
  EXPECT(sogm_map_audit(ctx, ctx, &bad, rot, out, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  SogmSpec spec{6, 4, 2, 2, 0.15f, 0.2f, 0.2f, 0.45f, -0.01f, 3.0f, 1.2f, 0.2f, 0.2f, SOGM_MAP_RISKBASE, SOGM_STORE_F32};
  if (sogm_device_count() == 0) {
    EXPECT(sogm_map_audit(ctx, ctx, &prm, nullptr, out, nullptr, nullptr) == SOGM_ERR_NO_DEVICE);
    bool threw = false;
    try {
      sogm_host::RiskMap m(spec, 1);   // no context without a device: the facade's methods are compiled, not run
      sogm_host::RiskMap t(spec, 1);
      (void)m.auditAgainst(t, m.auditParams(t));
    } catch (const std::exception &e) {
      threw = std::strstr(e.what(), "sogm_create") != nullptr;
    }
    EXPECT(threw);
  } else {
    sogm_host::RiskMap m(spec, 1), t(spec, 1);
    SogmSpec           half = spec;
    half.storage            = SOGM_STORE_F16 | SOGM_LAYOUT_TILED;
    half.T                  = 1;
    sogm_host::RiskMap h(half, 1);
    const float        pose[3] = {1.0f, 2.0f, 0.5f};
    std::vector<float> gm(48 * 2, 0.0f), gt(48 * 2, 0.0f), gh(48, 0.0f);
    gm[0 * 2 + 0] = 1.0f, gt[0 * 2 + 0] = 1.0f;   // cell 0, slice 0: both
    gm[7 * 2 + 1] = 1.0f, gt[8 * 2 + 1] = 1.0f;   // slice 1: neighbours in x
    gh[7]         = 1.0f;
    m.futureRiskCallback(sogm_host::futureRiskMsg(gm, pose, 3.5), 2);
    t.futureRiskCallback(sogm_host::futureRiskMsg(gt, pose, 3.25), 2);
    h.futureRiskCallback(sogm_host::futureRiskMsg(gh, pose, 3.0), 1);
    SogmMapAuditParams p = m.auditParams(t);
    EXPECT(p.thr_test == 0.2f && p.thr_truth == 0.2f && p.slice_map[1] == 1 && p.slice_map[2] == -1);
    p.tolerance = 1;
    double dt   = 0.0;
    auto   rows = m.auditAgainst(t, p, nullptr, &dt);
    EXPECT(rows.size() == 2 && dt == 0.25);
    EXPECT(rows[0].n_region == 48 && rows[0].n_test == 1 && rows[0].n_both == 1 && rows[0].status == 0);
    EXPECT(rows[1].n_both == 0 && rows[1].n_test_near == 1 && rows[1].n_truth_near == 1 && rows[1].truth_slice == 1);
    p          = m.auditParams(h);   // T_truth 1: slice 1 is skipped
    rows       = m.auditAgainst(h, p);
    EXPECT(rows[0].n_both == 0 && rows[0].n_truth == 1 && rows[1].status == SOGM_MAPAUDIT_SKIPPED && rows[1].truth_slice == -1);
    p.slice_map[1] = 0;
    p.flags        = SOGM_MAPAUDIT_FRUSTUM;
    p.far_z = 9.0, p.tan_h = 50.0, p.tan_v = 50.0;
    const double R[9] = {0, 0, 1, -1, 0, 0, 0, -1, 0};   // a camera looking along +x sees the cells with p_0 > 0: x = 3, 4, 5
    rows = m.auditAgainst(h, p, R);
    EXPECT(rows[1].n_region == 24 && rows[1].n_both == 0 && rows[1].n_test == 0 && rows[1].n_truth == 0);
  }
  if (fails) return 1;
  std::printf("map audit facade host ok\n");
  return 0;
}
