// sogm_dsp.hpp — what the particle map (sogm_dsp.hip, sogm_dsp_velocity.hip, sogm_dsp_state.hip) is made of: the flag codes
// and capacities, the per-agent scalars, the device view DspDev with ONE table of its per-agent arrays (member, elements per
// agent, initial fill) and the per-agent bases the kernels address them by, and the two rules of the ordered first-fit.
// That much is plain C++ (tests/dsp_rules_host_test.cpp builds it with the host compiler); behind __HIPCC__ follow the
// handle, the small device helpers the kernels share and the entry points one unit offers the others.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/sogm_abi.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DSP_HD __host__ __device__
#else
#define DSP_HD
#endif

namespace sogm {

enum : uint8_t { F_EMPTY = 0, F_VALID = 1, F_RESAMP = 2, F_MOVED = 3, F_NEW = 4, F_DEPART = 5, F_KILLED = 6 };
#define DSP_SLOTS 16   // storage slots per voxel (>= SAFE_PARTICLE_NUM_VOXEL)
#define DSP_ROUNDS 6   // place/pyramid fixed-point rounds issued per update

#define VEL_MAX_CLUSTERS 256  // accepted clusters per frame (more: error counter)
#define VEL_MAX_DYN 64        // possibly-dynamic clusters per frame taking part in the association
#define VEL_ADJ_CAP 128       // neighbours within the cluster tolerance kept per point
#define VEL_MAX_POINTS 8192   // k_dsp_velocity stages 8 points per thread in registers

struct DspAgent {  // per-agent scalars (device)
  float  last_p[3];
  int    first;
  double last_t;
  float  cur[3];
  float  update_time;
  float  quat[4];
  float  odom[4];  // -dx, -dy, -dz, dt
  int    pseq, vseq, rseq;
  int    ok;
  int    n_born, n_obs, valid_points;
  float  enb;  // expected_new_born_objects
  float  w_new;
  int    cand_cnt, born_cnt;
  int    changed[DSP_ROUNDS];
  int    dbg_voxel_full, dbg_pyr_full, dbg_out;
  int    err_unconverged, err_pool, err_points;
  int    n_occupied;
  // velocity estimation (velocityEstimationThread): previous frame's possibly-dynamic clusters and counters
  int    vel_n_last;
  int    vel_clusters, vel_dynamic, vel_matched, vel_err;
  float  vel_last[VEL_MAX_DYN][5];  // centre x, y, z, intensity, point_num (as float)
};

struct DspDev {
  int   A, V, S, L, W, H, T, NP, nph, npv, SP, OM, cand_cap, max_pts, nb, maxp, n_gauss, n_rand;
  float res, hx, hy, hz, sigma, Pd, kappa, w_nb, thick;
  float pred_t[SOGM_DSP_MAX_T];
  DspAgent *ag;
  uint8_t  *flag;  // [A][V][16]
  float    *f[6];  // vx vy px py pz w : [A][V][16]
  float    *fut;   // [A][T][V]
  float    *occ;   // [A][4][V]
  float    *pc;    // [A][NP][OM][5]
  int      *nobs;  // [A][NP]
  int      *maxlen;  // [A][NP] float bits (>= 0) or -1
  int      *obs_list;  // [A][max_pts] pi*OM + seq of every stored observation
  float    *bp_h, *bp_v;  // [A][(nph+1)*3], [A][(npv+1)*3]
  float    *born;  // [A][max_pts][7]
  int      *born_src;  // [A][max_pts] input index of every row of `born` (the velocity audit's link; rows >= n_born: stale)
  unsigned short *vel_adj;  // [A][max_pts][VEL_ADJ_CAP] neighbour lists of the clustering (velocity estimation)
  int            *vel_deg;  // [A][max_pts]
  // candidates of the prediction step (movers + in-FOV stays)
  int     *c_key, *c_dest, *c_pyr, *c_assign, *c_vnext, *c_pnext;  // [A][cand_cap]
  uint8_t *c_kill;                                                 // [A][cand_cap]
  float   *c_pay;                                                  // [A][cand_cap][6]
  int     *vhead;  // [A][V]
  int     *phead;  // [A][NP]
  int     *pyr_list, *pyr_n;  // [A][NP][SP] loc, [A][NP]
  int     *pyr_key, *pyr_id;  // [A][NP][SP] selection scratch (sweep key, candidate id)
  // new-born scratch
  int   *b_valid, *b_nstatic, *b_vi;  // [A][max_pts]
  float *b_c;                          // [A][max_pts][3]
  int8_t *b_cls;                       // [A][max_pts*nb]
  int   *b_dest, *b_vnext;             // [A][max_pts*nb]
  float *b_pay;                        // [A][max_pts*nb][5] px py pz vx vy
  const float *pg, *vg, *pdf, *bp_ori_h, *bp_ori_v;
  const int   *rnd, *nbr;

  // Per-agent bases, in ELEMENTS of the unit named (a slot, a pyramid, a candidate, ...); an array with several values per
  // unit multiplies the base by its count.  Each multiplies and adds left to right as written here: the kernels' addressing
  // follows this arithmetic.
  DSP_HD size_t slot_base(int a) const { return (size_t)a * V * DSP_SLOTS; }               // flag, f[k]
  DSP_HD size_t slot_base(int a, int v) const { return ((size_t)a * V + v) * DSP_SLOTS; }  // first slot of voxel v
  DSP_HD size_t voxel_base(int a) const { return (size_t)a * V; }                          // vhead
  DSP_HD size_t pyr_base(int a) const { return (size_t)a * NP; }                           // nobs, maxlen, phead, pyr_n; x SP: pyr_list, pyr_key, pyr_id
  DSP_HD size_t obs_base(int a) const { return (size_t)a * NP * OM; }                      // x 5: pc
  DSP_HD size_t bph_base(int a) const { return (size_t)a * (nph + 1); }                    // x 3: bp_h
  DSP_HD size_t bpv_base(int a) const { return (size_t)a * (npv + 1); }                    // x 3: bp_v
  DSP_HD size_t cand_base(int a) const { return (size_t)a * cand_cap; }                    // c_*; x 6: c_pay
  DSP_HD size_t point_base(int a) const { return (size_t)a * max_pts; }                    // obs_list, born_src, vel_deg, b_valid, b_nstatic, b_vi; x 7 born, x 3 b_c, x VEL_ADJ_CAP vel_adj
  DSP_HD size_t newborn_base(int a) const { return (size_t)a * max_pts * nb; }             // b_cls, b_dest, b_vnext; x 5: b_pay
  DSP_HD size_t fut_base(int a) const { return (size_t)a * T * V; }                        // fut: T planes of V
  DSP_HD size_t occ_base(int a) const { return (size_t)a * 4 * V; }                        // occ: weight, vx, vy, vz planes of V
};

// The table: every per-agent array of DspDev once — f(member, elements per agent, initial fill).  sogm_dsp_create allocates
// A times the count and fills by walking it; the constant tables (pg, vg, rnd, pdf, bp_ori_*, nbr) have no per-agent stride
// and are not part of it.
enum DspFill { DSP_FILL_NONE, DSP_FILL_ZERO, DSP_FILL_FF };
template <class F>
inline void dsp_for_each_buffer(DspDev &d, F &&f) {
  const size_t V = d.V, VS = V * DSP_SLOTS, NP = d.NP, MP = d.max_pts, NB = d.nb, CC = d.cand_cap;
  f(d.ag, (size_t)1, DSP_FILL_NONE);  // (set by sogm_dsp_create itself: first = 1, unit quaternion)
  f(d.flag, VS, DSP_FILL_ZERO);
  for (int k = 0; k < 6; ++k) f(d.f[k], VS, DSP_FILL_ZERO);
  f(d.fut, d.T * V, DSP_FILL_ZERO);
  f(d.occ, 4 * V, DSP_FILL_ZERO);
  f(d.pc, NP * d.OM * 5, DSP_FILL_ZERO);
  f(d.nobs, NP, DSP_FILL_ZERO);
  f(d.maxlen, NP, DSP_FILL_FF);
  f(d.obs_list, MP, DSP_FILL_NONE);
  f(d.bp_h, (size_t)(d.nph + 1) * 3, DSP_FILL_NONE);
  f(d.bp_v, (size_t)(d.npv + 1) * 3, DSP_FILL_NONE);
  f(d.born, MP * 7, DSP_FILL_NONE);
  f(d.born_src, MP, DSP_FILL_NONE);
  f(d.vel_adj, MP * VEL_ADJ_CAP, DSP_FILL_NONE);
  f(d.vel_deg, MP, DSP_FILL_NONE);
  f(d.c_key, CC, DSP_FILL_NONE);
  f(d.c_dest, CC, DSP_FILL_NONE);
  f(d.c_pyr, CC, DSP_FILL_NONE);
  f(d.c_assign, CC, DSP_FILL_NONE);
  f(d.c_vnext, CC, DSP_FILL_NONE);
  f(d.c_pnext, CC, DSP_FILL_NONE);
  f(d.c_kill, CC, DSP_FILL_NONE);
  f(d.c_pay, CC * 6, DSP_FILL_NONE);
  f(d.vhead, V, DSP_FILL_NONE);
  f(d.phead, NP, DSP_FILL_NONE);
  f(d.pyr_list, NP * d.SP, DSP_FILL_NONE);
  f(d.pyr_n, NP, DSP_FILL_ZERO);
  f(d.pyr_key, NP * d.SP, DSP_FILL_NONE);
  f(d.pyr_id, NP * d.SP, DSP_FILL_NONE);
  f(d.b_valid, MP, DSP_FILL_NONE);
  f(d.b_nstatic, MP, DSP_FILL_NONE);
  f(d.b_vi, MP, DSP_FILL_NONE);
  f(d.b_c, MP * 3, DSP_FILL_NONE);
  f(d.b_cls, MP * NB, DSP_FILL_NONE);
  f(d.b_dest, MP * NB, DSP_FILL_NONE);
  f(d.b_vnext, MP * NB, DSP_FILL_NONE);
  f(d.b_pay, MP * NB * 5, DSP_FILL_NONE);
}

// The scalar fields of DspDev from the map's spec and the parameters (every pointer stays as it is).  false: the parameters
// leave no room in a pyramid's list (SAFE_PARTICLE_NUM_PYRAMID < 1).
inline bool dsp_set_shape(DspDev &d, int n_agents, const SogmSpec &sp, const SogmDspParams &P, int max_points, int n_gauss,
                          int n_rand) {
  const int ar = P.angle_resolution;
  d.A   = n_agents;
  d.L   = sp.L;
  d.W   = sp.W;
  d.H   = sp.H;
  d.T   = sp.T;
  d.V   = sp.L * sp.W * sp.H;
  d.S   = P.max_particle_num_voxel * 2;
  d.nph = P.half_fov_h * 2 / ar;
  d.npv = P.half_fov_v * 2 / ar;
  d.NP  = d.nph * d.npv;
  d.SP  = (int)(d.V * P.max_particle_num_voxel + 1e5) / (360 * 180 / ar / ar) * 2;  // SAFE_PARTICLE_NUM_PYRAMID
  if (d.SP < 1) return false;
  d.OM       = P.obs_max_per_pyramid;
  d.cand_cap = 2 * d.V;
  d.max_pts  = max_points;
  d.nb       = P.newborn_num;
  d.maxp     = P.max_particle_num_voxel;
  d.n_gauss  = n_gauss;
  d.n_rand   = n_rand;
  d.res      = sp.resolution;
  d.hx       = (d.res * (float)sp.L) * 0.5f;  // map_length_x_half (:572)
  d.hy       = (d.res * (float)sp.W) * 0.5f;
  d.hz       = (d.res * (float)sp.H) * 0.5f;
  d.sigma    = P.sigma_observation;
  d.Pd       = P.p_detection;
  d.kappa    = P.kappa;
  d.w_nb     = P.newborn_weight;
  d.thick    = P.obstacle_thickness;
  for (int t = 0; t < SOGM_DSP_MAX_T; ++t) d.pred_t[t] = P.prediction_times[t];
  return true;
}

// ---- the ordered first-fit's two rules --------------------------------------------------------------------------------
// Keep the `cap` smallest keys seen so far in K[0, n), sorted ascending, each with its id in I (I == nullptr: keys only).
DSP_HD inline void keep_smallest(int *K, int *I, int &n, int cap, int key, int id) {
  if (n == cap && key > K[cap - 1]) return;
  int j = n < cap ? n : cap - 1;
  while (j > 0 && K[j - 1] > key) {
    K[j] = K[j - 1];
    if (I) I[j] = I[j - 1];
    --j;
  }
  K[j] = key;
  if (I) I[j] = id;
  if (n < cap) n = n + 1;
}
// The lowest slot of `all` (a mask of the voxel's slots) that `occ` leaves empty, or -1.
DSP_HD inline int lowest_free(unsigned occ, unsigned all) {
  const unsigned fr = ~occ & all;
  if (!fr) return -1;
#ifdef __HIP_DEVICE_COMPILE__
  return __ffs(fr) - 1;
#else
  return __builtin_ctz(fr);
#endif
}

}  // namespace sogm

#ifdef __HIPCC__
#include "sogm_device.hpp"

struct sogm_dsp {
  sogm_ctx           *map;
  sogm::DspDev        d;
  SogmDspParams       P;
  sogm::Resources     res;  // owns every buffer of `d`
};

namespace sogm {

// ---- entry points between the units (no relocatable device code: a kernel is launched by the unit that defines it) ----
// sogm_dsp_velocity.hip: the velocity estimation of one update on `st` (a SOGM_* code), and whether a handle of
// `max_points` can launch it on `device` at all: 1 yes, 0 no, < 0 a SOGM_ERR_* code.
int launch_dsp_velocity(const DspDev &d, const int32_t *range, float vres, hipStream_t st);
int velocity_lds_fits(int max_points, int device);
// sogm_dsp.hip: k_dsp_observe and k_dsp_newborn may ask for the dynamic LDS this handle needs
void reserve_update_lds(const DspDev &d);

// hipFuncAttributeMaxDynamicSharedMemorySize is per function, not per handle: raise it whenever a handle asks for more than
// any before (one "largest request so far" per kernel)
template <auto Kernel>
inline hipError_t raise_dynamic_lds(size_t bytes) {
  static size_t largest = 0;
  if (bytes <= largest) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) largest = bytes;
  return e;
}

// ---- small device helpers (arithmetic mirrors the reference, see oracle/dsp_oracle.cpp) ---------
__device__ inline void qmul(const float a[4], const float b[4], float o[4]) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
// rotateVectorByQuaternion dsp_dynamic.h:1391-1411
__device__ inline void rotate_q(const float *v, const float *q, float *o) {
  float vq[4] = {0.f, v[0], v[1], v[2]}, t[4], r[4];
  float n2    = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  float inv[4] = {q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2};
  qmul(q, vq, t);
  qmul(t, inv, r);
  o[0] = r[1];
  o[1] = r[2];
  o[2] = r[3];
}
__device__ inline float dot3(float x, float y, float z, const float *n) { return x * n[0] + y * n[1] + z * n[2]; }

// ifInPyramidsArea + findPointPyramid{Horizontal,Vertical}Index (:1413-1474): pyramid index or -1
__device__ inline int pyramid_of(const float *bh, const float *bv, int nph, int npv, float x, float y, float z) {
  if (!(dot3(x, y, z, bh) >= 0.f && dot3(x, y, z, bh + nph * 3) <= 0.f && dot3(x, y, z, bv) <= 0.f &&
        dot3(x, y, z, bv + npv * 3) >= 0.f))
    return -1;
  int h = -1, v = -1;
  if (fabsf(x) + fabsf(y) + fabsf(z) < 1e-12f) {
    // degenerate lengths: the products last*t of the reference's scan may underflow — replay it literally
    float last = 1.f;
    for (int i = 0; i < nph; i++) {
      float t = dot3(x, y, z, bh + (i + 1) * 3);
      if (last * t <= 0.f) {
        h = i;
        break;
      }
      last = t;
    }
    last = -1.f;
    for (int j = 0; j < npv; j++) {
      float t = dot3(x, y, z, bv + (j + 1) * 3);
      if (last * t <= 0.f) {
        v = j;
        break;
      }
      last = t;
    }
  } else {
    // The reference scans the boundary planes for the first sign change.  Inside the FOV the dot
    // products are positive (h) / negative (v) up to the point's pyramid and change sign once (planes
    // are 1 degree apart, far more than fp32 rounding), so the first index with t <= 0 (h) / t >= 0 (v)
    // is found by bisection with the same fp32 dot products: ~13 instead of ~70 plane tests.
    int lo = 0, hi = nph - 1;  // predicate true at nph-1 (ifInPyramidsArea: dot with plane nph <= 0)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (dot3(x, y, z, bh + (mid + 1) * 3) <= 0.f)
        hi = mid;
      else
        lo = mid + 1;
    }
    h  = lo;
    lo = 0;
    hi = npv - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (dot3(x, y, z, bv + (mid + 1) * 3) >= 0.f)
        hi = mid;
      else
        lo = mid + 1;
    }
    v = lo;
  }
  if (h < 0 || v < 0) return -1;  // "should not happen" in the reference (:1449,1471)
  return h * npv + v;
}
// getParticleVoxelsIndex (:1152-1166)
__device__ inline int voxel_index(const DspDev &d, float px, float py, float pz) {
  if (px >= d.hx || px <= -d.hx || py >= d.hy || py <= -d.hy || pz >= d.hz || pz <= -d.hz) return -1;
  int x = (int)((px + d.hx) / d.res);
  int y = (int)((py + d.hy) / d.res);
  int z = (int)((pz + d.hz) / d.res);
  int index = z * d.W * d.L + y * d.L + x;
  if (index < 0 || index >= d.V) return -1;
  return index;
}
// queryNormalPDF (:1380-1389)
__device__ inline float query_pdf(const float *pdf, float x, float mu, float sigma) {
  float c = (x - mu) / sigma;
  if (c > 9.9f)
    c = 9.9f;
  else if (c < -9.9f)
    c = -9.9f;
  return pdf[(int)(c * 1000 + 10000)];
}

}  // namespace sogm
#endif  // __HIPCC__
#undef DSP_HD
