// sogm_viewmask.hpp — the rules of the view mask (include/sogm_abi.h "view mask" is the definition), written ONCE for the
// host and the device:
//   view_class        the class of one logical cell against one agent's depth image: OUTSIDE the frustum, OFFIMAGE, FREE,
//                     SURFACE or HIDDEN
//   view_mask_words   the 64-bit words of a mask [agent][z][y][word]: cell x is bit x % 64 of word x / 64 (audit_row_words),
//                     the spare bits of a row's last word clear (audit_row_mask) — the layout of k_map_audit's region[]
// k_view_mask of sogm_viewmask.hip calls view_class; a host program compiles it as well (tests/view_rules_host_test.cpp).
// Every fp64 expression is written in the definition's order: with -ffp-contract=off host and device give the same bits.
// Known coarseness, on purpose: ONE pixel per cell, the one nearest the projection of the cell's centre.  A near cell covers
// many pixels and a silhouette can cut through it; the class is that of the centre's pixel alone.
#pragma once

#include "sogm_mapaudit.hpp"

#define SOGM_VIEWMASK_HD SOGM_MAPAUDIT_HD

namespace sogm {

enum : int { VIEW_OUTSIDE = 0, VIEW_OFFIMAGE = 1, VIEW_FREE = 2, VIEW_SURFACE = 3, VIEW_HIDDEN = 4, VIEW_N_CLASSES = 5 };

struct ViewCamera {
  double fx, fy, cx, cy;
  double depth_scale;
  double band;  // metres, finite, >= 0
  int    rows, cols;
};

// p_d = audit_centre(i_d) - off_d; without a cam_offset (has_off false) there is no subtraction at all, not one of 0.0
SOGM_VIEWMASK_HD inline double view_centre(int i, float res, float range, bool has_off, double off) {
  const double p = audit_centre(i, res, range);
  return has_off ? p - off : p;
}

// depth: ONE agent's image [rows * cols]; p0, p1, p2 from view_centre
SOGM_VIEWMASK_HD inline int view_class(const AuditFrustum &f, const ViewCamera &c, const uint16_t *depth, double p0, double p1,
                                       double p2) {
  double qx, qy, qz;
  audit_to_camera(f, p0, p1, p2, qx, qy, qz);
  if (!audit_in_frustum(f, qx, qy, qz)) return VIEW_OUTSIDE;
  const double uf = (qx / qz) * c.fx + c.cx, vf = (qy / qz) * c.fy + c.cy;
  const double u = __builtin_floor(uf + 0.5), v = __builtin_floor(vf + 0.5);
  if (!(u >= 0 && u < (double)c.cols && v >= 0 && v < (double)c.rows)) return VIEW_OFFIMAGE;  // (a NaN lands here)
  const uint16_t d16 = depth[(int)v * c.cols + (int)u];
  if (d16 == 0) return VIEW_FREE;  // no return within max_depth
  const double z_hit = (double)d16 / c.depth_scale;
  if (qz < z_hit - c.band) return VIEW_FREE;
  if (qz <= z_hit + c.band) return VIEW_SURFACE;
  return VIEW_HIDDEN;
}

SOGM_VIEWMASK_HD inline long long view_mask_words(int L, int W, int H) { return (long long)audit_row_words(L) * W * H; }

}  // namespace sogm
