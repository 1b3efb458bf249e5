// sogm_mapaudit.hpp — the rules of the map audit (include/sogm_abi.h "map audit" is the definition), written ONCE for the
// host and the device:
//   audit_occupied                 the occupancy test of one cell value
//   audit_centre / audit_in_view   the centre of a logical cell in the map frame and the frustum test (its two halves,
//                                  audit_to_camera and audit_in_frustum, are also what sogm_viewmask.hpp is built on)
//   audit_row_words / audit_row_mask / audit_dilate_word / audit_dilate_row
//                                  an x-row of L cells as ceil(L / 64) 64-bit words (cell x is bit x % 64 of word x / 64) and
//                                  its dilation by r cells: shifts and ORs with carries between neighbouring words, the spare
//                                  bits of the last word kept clear
//   audit_layout                   words per layer, layers per workgroup trip, halo and LDS bytes from L, W, H, r and
//                                  slab_layers: k_map_audit carves its LDS with it and sogm_map_audit sizes the launch with it
// k_map_audit of sogm_mapaudit.hip calls these bodies; a host program compiles them as well
// (tests/mapaudit_rules_host_test.cpp).  Every fp64 expression is written in the definition's order: with -ffp-contract=off
// host and device give the same bits.
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SOGM_MAPAUDIT_HD __host__ __device__
#else
#define SOGM_MAPAUDIT_HD
#endif

namespace sogm {

// O(c) = value > thr: fp32, strict; false for a NaN on either side
SOGM_MAPAUDIT_HD inline bool audit_occupied(float value, float thr) { return value > thr; }

// p_d = ((double)i_d + 0.5) * (double)res - (double)range_d
SOGM_MAPAUDIT_HD inline double audit_centre(int i, float res, float range) {
  return ((double)i + 0.5) * (double)res - (double)range;
}

struct AuditFrustum {
  double R[9];  // row-major camera-to-world rotation
  double near_z, far_z, tan_h, tan_v;
};

// q_j = (R[0][j] p_0 + R[1][j] p_1) + R[2][j] p_2;  in view iff q_z > near_z && q_z <= far_z && |q_x| <= q_z tan_h &&
// |q_y| <= q_z tan_v.  A non-finite R makes a non-finite q, and every comparison with a NaN is false; an infinite q_z fails
// q_z <= far_z (far_z is finite).
// The two halves are one body for audit_in_view and for view_class of sogm_viewmask.hpp ("view mask" uses the same q and the
// same four comparisons).
SOGM_MAPAUDIT_HD inline void audit_to_camera(const AuditFrustum &f, double p0, double p1, double p2, double &qx, double &qy,
                                             double &qz) {
  qx = (f.R[0] * p0 + f.R[3] * p1) + f.R[6] * p2;
  qy = (f.R[1] * p0 + f.R[4] * p1) + f.R[7] * p2;
  qz = (f.R[2] * p0 + f.R[5] * p1) + f.R[8] * p2;
}
SOGM_MAPAUDIT_HD inline bool audit_in_frustum(const AuditFrustum &f, double qx, double qy, double qz) {
  return qz > f.near_z && qz <= f.far_z && __builtin_fabs(qx) <= qz * f.tan_h && __builtin_fabs(qy) <= qz * f.tan_v;
}
SOGM_MAPAUDIT_HD inline bool audit_in_view(const AuditFrustum &f, double p0, double p1, double p2) {
  double qx, qy, qz;
  audit_to_camera(f, p0, p1, p2, qx, qy, qz);
  return audit_in_frustum(f, qx, qy, qz);
}

// ---- bit rows -------------------------------------------------------------------------------------------------------------
SOGM_MAPAUDIT_HD inline int audit_row_words(int L) { return (L + 63) >> 6; }

// the bits of word w that stand for cells of a row of L cells
SOGM_MAPAUDIT_HD inline uint64_t audit_row_mask(int L, int w) {
  const int left = L - (w << 6);
  return left >= 64 ? ~(uint64_t)0 : (left <= 0 ? (uint64_t)0 : (((uint64_t)1 << left) - 1));
}

// Word `cur` of a row dilated by r (0 .. 3) cells in x; prev / next are its neighbours in the row (0 beyond the row's ends:
// rows do not wrap).  The caller masks the result with audit_row_mask.
SOGM_MAPAUDIT_HD inline uint64_t audit_dilate_word(uint64_t prev, uint64_t cur, uint64_t next, int r) {
  uint64_t out = cur;
  for (int k = 1; k <= r; ++k) {
    out |= (cur << k) | (prev >> (64 - k));  // a cell k to the left reaches here
    out |= (cur >> k) | (next << (64 - k));  // a cell k to the right
  }
  return out;
}

// a whole row: out[w] for w < audit_row_words(L); in and out do not overlap
SOGM_MAPAUDIT_HD inline void audit_dilate_row(const uint64_t *in, uint64_t *out, int L, int r) {
  const int nw = audit_row_words(L);
  for (int w = 0; w < nw; ++w) {
    const uint64_t prev = w > 0 ? in[w - 1] : 0, next = w + 1 < nw ? in[w + 1] : 0;
    out[w] = audit_dilate_word(prev, in[w], next, r) & audit_row_mask(L, w);
  }
}

// ---- layout ---------------------------------------------------------------------------------------------------------------
constexpr int AUDIT_LDS_BYTES     = 160 * 1024;  // of a gfx950 compute unit
constexpr int AUDIT_LDS_RESERVED  = 1024;        // the kernel's static LDS (the workgroup reduction)
constexpr int AUDIT_DEFAULT_LAYERS = 4;          // slab_layers == 0.  Measured at 16 x 100^3 x 15: more, smaller
                                                 // workgroups hide the loads' latency better than fewer halo re-reads pay back;
                                                 // even, so that a slab of a tiled map is whole tiles

// One workgroup trip handles z layers [z0, z0 + layers) of an agent and holds, as 64-bit words [layer][y][word of the row]:
//   region  [layers]               the region's bits (built once per trip, every slice reads them)
//   occ     [2][layers + 2 halo]   the occupancy bits of the test and the truth slice, layers z0 - halo .. z0 + layers + halo
//                                  (a layer outside the grid stays clear: edges do not wrap)
//   xy      [2][layers + 2 halo]   the same rows dilated in x and y — only when halo > 0
struct AuditLayout {
  int row_words;    // words per x-row
  int layer_words;  // words per z layer: W * row_words
  int halo;         // = r
  int layers;       // z layers per trip (0: even one layer does not fit, the entry refuses the grid)
  int slabs;        // trips per agent: ceil(H / layers)
  int occ_layers;   // layers + 2 * halo
  int region_off, occ_off[2], xy_off[2];  // word offsets into the dynamic LDS
  int bytes;        // dynamic LDS of the launch
};

SOGM_MAPAUDIT_HD inline int audit_layout_bytes(int layer_words, int layers, int r) {
  const long long words = (long long)layer_words * ((long long)layers + (long long)(r > 0 ? 4 : 2) * (layers + 2 * r));
  return words * 8 > 0x7fffffffLL ? 0x7fffffff : (int)(words * 8);
}

SOGM_MAPAUDIT_HD inline AuditLayout audit_layout(int L, int W, int H, int r, int slab_layers) {
  AuditLayout a;
  a.row_words   = audit_row_words(L);
  a.layer_words = W * a.row_words;
  a.halo        = r;
  const int budget = AUDIT_LDS_BYTES - AUDIT_LDS_RESERVED;
  int       want   = slab_layers > 0 ? slab_layers : AUDIT_DEFAULT_LAYERS;
  if (want > H) want = H;
  int layers = 0;
  for (int s = 1; s <= want; ++s) {  // the largest count up to `want` that fits (bytes grow with s)
    if (audit_layout_bytes(a.layer_words, s, r) > budget) break;
    layers = s;
  }
  a.layers     = layers;
  a.slabs      = layers > 0 ? (H + layers - 1) / layers : 0;
  a.occ_layers = layers + 2 * r;
  const int occ = a.occ_layers * a.layer_words;
  a.region_off  = 0;
  a.occ_off[0]  = layers * a.layer_words;
  a.occ_off[1]  = a.occ_off[0] + occ;
  a.xy_off[0]   = r > 0 ? a.occ_off[1] + occ : a.occ_off[0];  // (r == 0: the dilated rows ARE the rows)
  a.xy_off[1]   = r > 0 ? a.xy_off[0] + occ : a.occ_off[1];
  a.bytes       = layers > 0 ? audit_layout_bytes(a.layer_words, layers, r) : 0;
  return a;
}

}  // namespace sogm
