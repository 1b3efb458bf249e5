// Compiles against host/sogm_facade.hpp's RiskMap::viewParams / viewMask / auditAgainstMasked and checks the argument handling
// of sogm_view_mask and sogm_map_audit_masked on the host: null pointers and prm's own fields are refused before anything
// else; a well-formed call without a GPU is SOGM_ERR_NO_DEVICE.  With a GPU the facade masks a one-agent 6 x 4 x 2 map from a
// 4 x 4 depth image and audits two maps on that mask.  Prints "view mask facade ok".
#include <cmath>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

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
  static_assert(sizeof(SogmViewParams) == 104, "layout");
  static_assert(SOGM_VIEW_OUTSIDE == 0 && SOGM_VIEW_HIDDEN == 4 && SOGM_VIEWBIT_FREE == 4 && SOGM_VIEWBIT_ALL == 31, "codes");
  SogmDepthCamera cam{};
  cam.fx = 2.0, cam.fy = 2.0, cam.cx = 1.5, cam.cy = 1.5, cam.max_depth = 2.0, cam.depth_scale = 1000.0;
  cam.rows = 4, cam.cols = 4;
  SogmViewParams prm = sogm_host::RiskMap::viewParams(cam);
  EXPECT(prm.near_z == 0.0 && prm.far_z == 2.0 && prm.tan_h == 1.0 && prm.tan_v == 1.0 && prm.band == 0.0);
  EXPECT(prm.classes == (SOGM_VIEWBIT_FREE | SOGM_VIEWBIT_SURFACE) && prm.rows == 4 && prm.cols == 4);
  EXPECT(sogm_view_default_params(nullptr, &prm) == SOGM_ERR_INVALID_ARG);
  // stand-in addresses: every refusal below happens before anything is read
  auto *ctx  = reinterpret_cast<sogm_ctx *>(0x1000);
  auto *img  = reinterpret_cast<const uint16_t *>(0x2000);
  auto *rot  = reinterpret_cast<const double *>(0x3000);
  auto *mask = reinterpret_cast<uint64_t *>(0x4000);
  auto *rows = reinterpret_cast<SogmMapAuditRow *>(0x5000);
  EXPECT(sogm_view_mask(nullptr, &prm, img, rot, nullptr, mask, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  EXPECT(std::strstr(sogm_last_error(), "sogm_view_mask") != nullptr);
  EXPECT(sogm_view_mask(ctx, &prm, img, rot, nullptr, nullptr, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  SogmViewParams bad = prm;
  bad.far_z          = 2.5;   // beyond max_depth
  EXPECT(sogm_view_mask(ctx, &bad, img, rot, nullptr, mask, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  bad = prm, bad.band = -1.0;
  EXPECT(sogm_view_mask(ctx, &bad, img, rot, nullptr, mask, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  bad = prm, bad.classes = 32;
  EXPECT(sogm_view_mask(ctx, &bad, img, rot, nullptr, mask, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  SogmMapAuditParams ap;
  EXPECT(sogm_map_audit_default_params(2, 2, &ap) == SOGM_OK);
  EXPECT(sogm_map_audit_masked(ctx, ctx, &ap, nullptr, rows, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  ap.flags = SOGM_MAPAUDIT_FRUSTUM;
  EXPECT(sogm_map_audit_masked(ctx, ctx, &ap, mask, rows, nullptr, nullptr) == SOGM_ERR_INVALID_ARG);
  ap.flags = 0;
  SogmSpec spec{6, 4, 2, 2, 0.15f, 0.2f, 0.2f, 0.45f, -0.01f, 3.0f, 1.2f, 0.2f, 0.2f, SOGM_MAP_RISKBASE, SOGM_STORE_F32};
  if (sogm_device_count() == 0) {
    EXPECT(sogm_view_mask(ctx, &prm, img, rot, nullptr, mask, nullptr, nullptr) == SOGM_ERR_NO_DEVICE);
    EXPECT(sogm_map_audit_masked(ctx, ctx, &ap, mask, rows, nullptr, nullptr) == SOGM_ERR_NO_DEVICE);
    bool threw = false;
    try {
      sogm_host::RiskMap m(spec, 1);   // no context without a device: the facade's methods are compiled, not run
      sogm_host::RiskMap t(spec, 1);
      (void)m.viewMask(prm, img, nullptr, nullptr, mask);
      (void)m.auditAgainstMasked(t, m.auditParams(t), mask);
    } catch (const std::exception &e) {
      threw = std::strstr(e.what(), "sogm_create") != nullptr;
    }
    EXPECT(threw);
  } else {
    sogm_host::RiskMap m(spec, 1), t(spec, 1);
    const float        pose[3] = {1.0f, 2.0f, 0.5f};
    std::vector<float> gm(48 * 2, 1.0f), gt(48 * 2, 1.0f);   // every cell occupied on both sides: the counts are the region
    m.futureRiskCallback(sogm_host::futureRiskMsg(gm, pose, 3.5), 2);
    t.futureRiskCallback(sogm_host::futureRiskMsg(gt, pose, 3.25), 2);
    uint16_t       host_img[16];
    for (auto &d : host_img) d = 300;                        // a wall 0.3 m ahead
    uint16_t *d_img  = nullptr;
    uint64_t *d_mask = nullptr;
    EXPECT(m.viewMaskWords() == 8);
    EXPECT(hipMalloc(&d_img, sizeof host_img) == hipSuccess && hipMalloc(&d_mask, m.viewMaskWords() * 8) == hipSuccess);
    EXPECT(hipMemcpy(d_img, host_img, sizeof host_img, hipMemcpyHostToDevice) == hipSuccess);
    const double R[9] = {0, 0, 1, -1, 0, 0, 0, -1, 0};       // looking along +x: only the cells with p_0 > 0 (x = 3, 4, 5)
    auto counts = m.viewMask(prm, d_img, R, nullptr, d_mask);
    EXPECT(counts.size() == 8 && counts[0] + counts[1] + counts[2] + counts[3] + counts[4] == 48 && counts[0] >= 24);
    EXPECT(counts[5] == counts[2] + counts[3] && counts[2] > 0 && counts[4] > 0 && counts[6] == 0 && counts[7] == 0);
    SogmMapAuditParams p = m.auditParams(t);
    double dt = 0.0;
    auto   got = m.auditAgainstMasked(t, p, d_mask, &dt);
    EXPECT(got.size() == 2 && dt == 0.25 && got[0].status == 0 && got[1].truth_slice == 1);
    EXPECT(got[0].n_region == counts[5] && got[0].n_test == counts[5] && got[1].n_both == counts[5]);
    // every class but OUTSIDE: the frustum audit's region
    SogmViewParams all = prm;
    all.classes        = SOGM_VIEWBIT_ALL & ~SOGM_VIEWBIT_OUTSIDE;
    counts             = m.viewMask(all, d_img, R, nullptr, d_mask);
    got                = m.auditAgainstMasked(t, p, d_mask);
    SogmMapAuditParams fr = p;
    fr.flags = SOGM_MAPAUDIT_FRUSTUM, fr.near_z = all.near_z, fr.far_z = all.far_z, fr.tan_h = all.tan_h, fr.tan_v = all.tan_v;
    auto want = m.auditAgainst(t, fr, R);
    EXPECT(want[0].n_region == 48 - counts[0] && std::memcmp(got.data(), want.data(), sizeof(SogmMapAuditRow) * 2) == 0);
    // an offset that puts the camera 0.3 m behind the map centre: more of the grid is ahead of it
    const double off[3] = {-0.3, 0.0, 0.0};
    auto shifted = m.viewMask(all, d_img, R, off, d_mask);
    EXPECT(shifted[0] < counts[0]);
    (void)hipFree(d_img);
    (void)hipFree(d_mask);
  }
  if (fails) return 1;
  std::printf("view mask facade ok\n");
  return 0;
}
