// Map audit (include/sogm_abi.h "map audit"; the rules: sogm_mapaudit.hpp): the cells where a perceived SOGM and the
// ground-truth SOGM agree, strictly and within r cells, per agent and test slice.  Two launches, stream-ordered:
//   k_map_audit_rows   one lane per (agent, test slice): the row zeroed, its truth_slice and status; out_dt
//   k_map_audit        one workgroup per (agent, slab of z layers), looping over the test slices:
//     once per slab    the region's bits (box, frustum in fp64) by 64-wide ballots, one wave per word, into LDS; or, in
//                      sogm_map_audit_masked's instantiation, copied from a given mask of the same layout and ANDed with the box
//     per slice        both maps' cells of layers z0 - r .. z1 + r streamed with 16-byte loads over the slab's CONTIGUOUS
//                      physical range (rows: whole layers; tiles: whole pairs of layers), whatever the cell type; a lane
//                      decodes its chunk's first cell once (GridGeom's rows or tiles), walks the 4 or 8 cells and ORs the
//                      bits of each row word it touches into LDS — a 16-byte load hands a lane CONSECUTIVE cells, which a
//                      ballot would interleave across four or eight words; the chunks at the range's unaligned ends go
//                      through cell_ld cell by cell
//                      x and y dilation on the words (audit_dilate_word, then an OR of rows), z as an OR of layers while
//                      counting; popcounts of ANDs, reduced by wave (shuffles), then by workgroup (LDS), then ONE integer
//                      atomicAdd per count and workgroup into the row
// Integer adds only: the rows do not depend on the order the workgroups finish in, nor on slab_layers.
#include "sogm_device.hpp"
#include "sogm_mapaudit.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

namespace sogm {
namespace {

constexpr int MAPAUDIT_WG     = 512;
constexpr int MAPAUDIT_UNROLL = 4;  // 16-byte loads a lane has in flight per map
constexpr int N_COUNTS        = 6;  // n_region .. n_truth_near, SogmMapAuditRow's first fields in order

struct MapAuditArgs {
  float       thr[2];
  int         r, frustum;
  int         lo[3], hi[3];
  int         T_test;
  int         slice_map[SOGM_MAPAUDIT_MAX_T];
  double      near_z, far_z, tan_h, tan_v;
  AuditLayout lay;
};
static_assert(AUDIT_LDS_RESERVED >= (int)(sizeof(int) * 2 * N_COUNTS), "the static LDS of k_map_audit");
static_assert(sizeof(SogmMapAuditRow) == 8 * sizeof(int32_t), "a row is eight counters");

__device__ inline bool centres_differ(const MapView &a, const MapView &b, int agent) {
  bool d = false;
  for (int k = 0; k < 3; ++k) d = d || __float_as_uint(a.poses[agent * 3 + k]) != __float_as_uint(b.poses[agent * 3 + k]);
  return d;
}

__global__ __launch_bounds__(64) void k_map_audit_rows(MapView test, MapView truth, MapAuditArgs p,
                                                       SogmMapAuditRow *__restrict__ out, double *__restrict__ out_dt) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= test.n_agents * p.T_test) return;
  const int a = i / p.T_test, t = i - a * p.T_test;
  SogmMapAuditRow row{};
  row.truth_slice = p.slice_map[t];
  row.status      = row.truth_slice < 0 ? SOGM_MAPAUDIT_SKIPPED : (centres_differ(test, truth, a) ? SOGM_MAPAUDIT_CENTRE : 0);
  out[i] = row;
  if (t == 0 && out_dt) out_dt[a] = test.stamps[a] - truth.stamps[a];
}

// sum over the wave, valid in lane 0
__device__ inline int wave_sum(int v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// The cells of one chunk as floats.  Fully unrolled by the callers: compile-time indices only, no scratch.
__device__ inline float chunk_cell(const uint4 &q, int j, int half) {
  const unsigned w[4] = {q.x, q.y, q.z, q.w};
  if (!half) return __uint_as_float(w[j & 3]);
  return __half2float(__ushort_as_half((unsigned short)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu)));
}

// Occupancy bits of layers [zlo, zlo + lay.occ_layers) of one slice into occ (zeroed by the caller; layers outside the
// grid stay clear).  The workgroup streams the physical range that holds layers [max(zlo, 0), min(zhi, H)) in 16-byte
// chunks, chunk c0 + k * MAPAUDIT_WG + lane for k < MAPAUDIT_UNROLL per trip: issue() starts a trip's loads, consume()
// turns them into bits.
struct BitStream {
  const GridGeom     &g;
  const void         *slab;
  float               thr;
  unsigned long long *occ;
  int                 zlo, zb;           // the first layer of occ; one past the last layer wanted
  int                 p0, p1;            // first and one-past-last physical cell of the range
  int                 sh, per;           // bytes per cell (log2), cells per 16-byte chunk
  int                 head, nchunks;     // cells before p0 in the aligned chunk that holds it; chunks in all
  uintptr_t           a0;                // that chunk's address

  __device__ BitStream(const GridGeom &geom, const void *s, float t, unsigned long long *o, int zlo_, int zhi)
      : g(geom), slab(s), thr(t), occ(o), zlo(zlo_), zb(min(zhi, geom.H)) {
    const int za = max(zlo, 0), LW = g.L * g.W;
    p0 = g.tile ? (za >> 1) * 2 * LW : za * LW;
    p1 = g.tile ? ((zb + 1) >> 1) * 2 * LW : zb * LW;
    sh = g.half ? 1 : 2, per = 16 >> sh;
    const uintptr_t base = reinterpret_cast<uintptr_t>(slab) + ((uintptr_t)p0 << sh);
    a0      = base & ~(uintptr_t)15;
    head    = (int)((base - a0) >> sh);
    nchunks = (p1 - p0 + head + per - 1) / per;
  }
  // chunk c's first cell (may lie before p0) and whether all of it lies inside the range
  __device__ int  first(int c) const { return p0 - head + c * per; }
  __device__ bool full(int c) const { return c < nchunks && first(c) >= p0 && first(c) + per <= p1; }

  // the 16-byte loads of this lane's chunks c0 + k * MAPAUDIT_WG + lane: issued, not waited for
  __device__ void issue(int c0, uint4 (&q)[MAPAUDIT_UNROLL]) const {
#pragma unroll
    for (int k = 0; k < MAPAUDIT_UNROLL; ++k) {
      const int c = c0 + k * MAPAUDIT_WG + (int)threadIdx.x;
      q[k]        = make_uint4(0, 0, 0, 0);
      if (full(c)) q[k] = *reinterpret_cast<const uint4 *>(a0 + (uintptr_t)c * 16);
    }
  }
  __device__ void consume(const AuditLayout &lay, int c0, const uint4 (&q)[MAPAUDIT_UNROLL]) const;
};

__device__ inline void BitStream::consume(const AuditLayout &lay, int c0, const uint4 (&q)[MAPAUDIT_UNROLL]) const {
  const int LW = g.L * g.W, lt = g.L >> 1, wt = g.W >> 1;
#pragma unroll
  for (int k = 0; k < MAPAUDIT_UNROLL; ++k) {
    const int c = c0 + k * MAPAUDIT_WG + (int)threadIdx.x;
    if (c >= nchunks) continue;
    const int  cs     = first(c);
    const bool whole  = full(c);
    const int  j0 = max(p0 - cs, 0), j1 = min(p1 - cs, per);       // the chunk's cells inside the range
    unsigned   bits = 0;                                           // bit j: cell cs + j is occupied
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= per) break;
      float v;
      if (whole)
        v = chunk_cell(q[k], j, g.half);
      else
        v = (j >= j0 && j < j1) ? cell_ld(slab, (size_t)(cs + j), g.half) : NAN;  // (a NaN is not occupied)
      bits |= audit_occupied(v, thr) ? 1u << j : 0u;
    }
    if (!bits) continue;
    // decode the first cell once, then walk
    int x, y, z, tx = 0, ty = 0, tz = 0;
    const int pf = cs + j0;
    if (!g.tile) {
      z = pf / LW;
      const int rem = pf - z * LW;
      y = rem / g.L;
      x = rem - y * g.L;
    } else {
      const int t = pf >> 3;
      tz = t / (lt * wt);
      const int rem = t - tz * lt * wt;
      ty = rem / lt;
      tx = rem - ty * lt;
      x = y = z = 0;
    }
    int                word = -1;
    unsigned long long acc  = 0;
    for (int j = j0; j < j1; ++j) {
      const int p = cs + j;
      if (g.tile) {
        if (j > j0 && (p & 7) == 0 && ++tx == lt) {  // the next tile (only a chunk that is not tile-aligned gets here)
          tx = 0;
          if (++ty == wt) ty = 0, ++tz;
        }
        x = (tx << 1) | (p & 1), y = (ty << 1) | ((p >> 1) & 1), z = (tz << 1) | ((p >> 2) & 1);
      }
      const int zl = z - zlo;
      if (((bits >> j) & 1) && zl >= 0 && zl < lay.occ_layers && z < zb) {
        const int w = (zl * g.W + y) * lay.row_words + (x >> 6);
        if (w != word) {
          if (word >= 0) atomicOr(occ + word, acc);
          word = w, acc = 0;
        }
        acc |= 1ull << (x & 63);
      }
      if (!g.tile && ++x == g.L) {
        x = 0;
        if (++y == g.W) y = 0, ++z;
      }
    }
    if (word >= 0) atomicOr(occ + word, acc);
  }
}

// MASKED: the region's second source (sogm_map_audit_masked) — a mask in region[]'s own [layer][y][word] layout, ANDed with
// the box.  The frustum instantiation <false> is the kernel as it was; `mask` is not read there.
template <bool MASKED>
__global__ __launch_bounds__(MAPAUDIT_WG) void k_map_audit(MapView test, MapView truth, MapAuditArgs p,
                                                           const double *__restrict__ cam_rot,
                                                           SogmMapAuditRow *__restrict__ out,
                                                           const unsigned long long *__restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
  __shared__ int s_cnt[N_COUNTS];
  const AuditLayout &lay = p.lay;
  const GridGeom    &g   = test.g;
  const int a = blockIdx.y, z0 = blockIdx.x * lay.layers, nz = min(lay.layers, g.H - z0);
  if (centres_differ(test, truth, a)) return;  // (uniform: the rows kernel has said so)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lw = lay.layer_words, r = p.r;
  unsigned long long *region = lds + lay.region_off;
  if (tid < N_COUNTS) s_cnt[tid] = 0;

  int n_reg = 0;
  if constexpr (MASKED) {
    // ---- the region's bits from the mask: the slab's words are contiguous, a lane per word; the box as bits of the word ----
    const unsigned long long *src = mask + ((size_t)a * g.H + z0) * (size_t)lw;
    for (int i = tid; i < nz * lw; i += MAPAUDIT_WG) {
      const int zl = i / lw, rem = i - zl * lw, y = rem / lay.row_words, w = rem - y * lay.row_words, z = z0 + zl;
      const bool               in  = y >= p.lo[1] && y < p.hi[1] && z >= p.lo[2] && z < p.hi[2];
      const unsigned long long box = in ? audit_row_mask(p.hi[0], w) & ~audit_row_mask(p.lo[0], w) : 0ull;  // (hi[0] <= L)
      const unsigned long long m   = src[i] & box;
      region[i] = m;
      n_reg += __popcll(m);
    }
    n_reg = wave_sum(n_reg);  // (valid in lane 0, which is the lane that adds it below)
  } else {
    // ---- the region's bits, once per slab: one wave per word, one lane per cell ----
    AuditFrustum f{};
    if (p.frustum) {
      for (int k = 0; k < 9; ++k) f.R[k] = cam_rot[a * 9 + k];
      f.near_z = p.near_z, f.far_z = p.far_z, f.tan_h = p.tan_h, f.tan_v = p.tan_v;
    }
    for (int i = wave; i < nz * lw; i += MAPAUDIT_WG / 64) {
      const int zl = i / lw, rem = i - zl * lw, y = rem / lay.row_words, w = rem - y * lay.row_words;
      const int x = (w << 6) + lane, z = z0 + zl;
      bool      in = x < g.L && x >= p.lo[0] && x < p.hi[0] && y >= p.lo[1] && y < p.hi[1] && z >= p.lo[2] && z < p.hi[2];
      if (in && p.frustum)
        in = audit_in_view(f, audit_centre(x, g.res, g.rx), audit_centre(y, g.res, g.ry), audit_centre(z, g.res, g.rz));
      const unsigned long long m = __ballot(in);
      if (lane == 0) {
        region[i] = m;
        n_reg += __popcll(m);
      }
    }
  }
  __syncthreads();
  if (lane == 0 && n_reg) atomicAdd(&s_cnt[0], n_reg);
  __syncthreads();
  const int n_region = s_cnt[0];
  __syncthreads();
  if (tid == 0) s_cnt[0] = 0;

  unsigned long long *occ_t = lds + lay.occ_off[0], *occ_g = lds + lay.occ_off[1];
  unsigned long long *xy_t = lds + lay.xy_off[0], *xy_g = lds + lay.xy_off[1];
  const int           occ_words = lay.occ_layers * lw;
  for (int t = 0; t < p.T_test; ++t) {
    const int s = p.slice_map[t];
    if (s < 0) continue;
    __syncthreads();  // the previous slice's counting has read the bits
    for (int i = tid; i < 2 * occ_words; i += MAPAUDIT_WG) occ_t[i] = 0;  // (occ_g follows occ_t)
    __syncthreads();
    {
      // both maps' loads of a trip are in flight before either is looked at: 2 x MAPAUDIT_UNROLL x 16 bytes per lane
      const BitStream st(test.g, test.slab(a, t), p.thr[0], occ_t, z0 - r, z0 + nz + r);
      const BitStream sg(truth.g, truth.slab(a, s), p.thr[1], occ_g, z0 - r, z0 + nz + r);
      for (int c0 = 0; c0 < max(st.nchunks, sg.nchunks); c0 += MAPAUDIT_WG * MAPAUDIT_UNROLL) {
        uint4 qt[MAPAUDIT_UNROLL], qg[MAPAUDIT_UNROLL];
        st.issue(c0, qt);
        sg.issue(c0, qg);
        st.consume(lay, c0, qt);
        sg.consume(lay, c0, qg);
      }
    }
    __syncthreads();
    if (r > 0) {
      // x and y: xy[z][y][w] = OR over |dy| <= r of the x-dilated word w of row y + dy (rows outside the grid: nothing)
      for (int i = tid; i < 2 * occ_words; i += MAPAUDIT_WG) {
        const int m = i >= occ_words ? 1 : 0, e = i - m * occ_words;
        const int zl = e / lw, rem = e - zl * lw, y = rem / lay.row_words, w = rem - y * lay.row_words;
        const unsigned long long *src = (m ? occ_g : occ_t) + zl * lw;
        unsigned long long        acc = 0;
        for (int yy = max(y - r, 0); yy <= min(y + r, g.W - 1); ++yy) {
          const unsigned long long *row = src + yy * lay.row_words;
          acc |= audit_dilate_word(w > 0 ? row[w - 1] : 0, row[w], w + 1 < lay.row_words ? row[w + 1] : 0, r);
        }
        (m ? xy_g : xy_t)[e] = acc & audit_row_mask(g.L, w);
      }
      __syncthreads();
    }
    int c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
    for (int i = tid; i < nz * lw; i += MAPAUDIT_WG) {
      const unsigned long long R = region[i];
      if (!R) continue;
      const int                zl = i / lw, rem = i - zl * lw;
      const int                at = (zl + r) * lw + rem;  // layer z0 + zl of the occupancy arrays
      const unsigned long long ot = occ_t[at] & R, og = occ_g[at] & R;
      unsigned long long       dt = 0, dg = 0;            // D_r of the test and of the truth bits
      for (int dz = -r; dz <= r; ++dz) {
        dt |= xy_t[at + dz * lw];
        dg |= xy_g[at + dz * lw];
      }
      c1 += __popcll(ot);
      c2 += __popcll(og);
      c3 += __popcll(ot & og);
      c4 += __popcll(ot & dg);
      c5 += __popcll(og & dt);
    }
    c1 = wave_sum(c1), c2 = wave_sum(c2), c3 = wave_sum(c3), c4 = wave_sum(c4), c5 = wave_sum(c5);
    if (lane == 0) {
      if (c1) atomicAdd(&s_cnt[1], c1);
      if (c2) atomicAdd(&s_cnt[2], c2);
      if (c3) atomicAdd(&s_cnt[3], c3);
      if (c4) atomicAdd(&s_cnt[4], c4);
      if (c5) atomicAdd(&s_cnt[5], c5);
    }
    __syncthreads();
    if (tid < N_COUNTS) {
      const int v = tid == 0 ? n_region : s_cnt[tid];
      if (v) atomicAdd(reinterpret_cast<int *>(out + (size_t)a * p.T_test + t) + tid, v);
      s_cnt[tid] = 0;
    }
  }
}

int refuse(const char *what, const char *entry = "sogm_map_audit") {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_map_audit_default_params(int T_test, int T_truth, SogmMapAuditParams *out) {
  if (!out || T_test < 1 || T_truth < 1 || T_test > SOGM_MAPAUDIT_MAX_T || T_truth > SOGM_MAPAUDIT_MAX_T) {
    sogm::set_error_text("sogm_map_audit_default_params: null prm or T outside 1 .. 32");
    return SOGM_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  for (int t = 0; t < SOGM_MAPAUDIT_MAX_T; ++t) out->slice_map[t] = t < T_test && t < T_truth ? t : -1;
  return SOGM_OK;
}

namespace sogm {
namespace {
// the body of both entries: MASKED takes the region from `mask` (and the box), the other from the box and the frustum
template <bool MASKED>
int map_audit_entry(sogm_ctx *test, sogm_ctx *truth, const SogmMapAuditParams *prm, const double *cam_rot,
                    const uint64_t *mask, SogmMapAuditRow *out, double *out_dt, void *stream) {
  const char *entry = MASKED ? "sogm_map_audit_masked" : "sogm_map_audit";
  const auto  refuse = [entry](const char *what) { return sogm::refuse(what, entry); };
  if (!test || !truth || !prm || !out || (MASKED && !mask)) return refuse("null pointer");
  if (prm->tolerance < 0 || prm->tolerance > 3) return refuse("tolerance outside 0 .. 3");
  const bool frustum = (prm->flags & SOGM_MAPAUDIT_FRUSTUM) != 0;
  if (MASKED && frustum) return refuse("SOGM_MAPAUDIT_FRUSTUM is set: the mask is the region");
  if (frustum) {
    if (!cam_rot) return refuse("SOGM_MAPAUDIT_FRUSTUM without cam_rot");
    if (!std::isfinite(prm->near_z) || !std::isfinite(prm->far_z) || !std::isfinite(prm->tan_h) || !std::isfinite(prm->tan_v))
      return refuse("near_z, far_z, tan_h and tan_v must be finite");
    if (prm->near_z < 0 || !(prm->far_z > prm->near_z) || !(prm->tan_h > 0) || !(prm->tan_v > 0))
      return refuse("near_z >= 0, far_z > near_z, tan_h > 0 and tan_v > 0 are required");
  }
  {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
      set_error_text(MASKED ? "sogm_map_audit_masked: no HIP device" : "sogm_map_audit: no HIP device");
      return SOGM_ERR_NO_DEVICE;
    }
  }
  const SogmSpec &a = test->spec, &b = truth->spec;
  if (test->device != truth->device) return refuse("the two contexts are on different devices");
  if (test->n_agents != truth->n_agents) return refuse("the two contexts have different n_agents");
  if (a.L != b.L || a.W != b.W || a.H != b.H || std::memcmp(&a.resolution, &b.resolution, sizeof(float)) != 0)
    return refuse("the two contexts have different L, W, H or resolution");
  if (a.T > SOGM_MAPAUDIT_MAX_T || b.T > SOGM_MAPAUDIT_MAX_T) return refuse("T above 32");
  MapAuditArgs p{};
  bool         whole = true;
  for (int d = 0; d < 3; ++d) whole = whole && prm->box_lo[d] == 0 && prm->box_hi[d] == 0;
  const int dims[3] = {a.L, a.W, a.H};
  for (int d = 0; d < 3; ++d) {
    p.lo[d] = whole ? 0 : prm->box_lo[d];
    p.hi[d] = whole ? dims[d] : prm->box_hi[d];
    if (p.lo[d] < 0 || p.hi[d] > dims[d] || p.lo[d] >= p.hi[d]) return refuse("the box is empty or leaves the grid");
  }
  for (int t = 0; t < a.T; ++t) {
    if (prm->slice_map[t] < -1 || prm->slice_map[t] >= b.T) return refuse("a slice_map entry below -1 or at or above T_truth");
    p.slice_map[t] = prm->slice_map[t];
  }
  p.lay = audit_layout(a.L, a.W, a.H, prm->tolerance, prm->slab_layers);
  if (p.lay.layers < 1) return refuse("one z layer of the grid does not fit a compute unit's LDS");
  if (!test->updated || !truth->updated) {
    set_error_text(MASKED ? "sogm_map_audit_masked: a map has never been updated" : "sogm_map_audit: a map has never been updated");
    return SOGM_ERR_STATE;
  }
  p.thr[0] = prm->thr_test, p.thr[1] = prm->thr_truth;
  p.r = prm->tolerance, p.frustum = frustum ? 1 : 0, p.T_test = a.T;
  p.near_z = prm->near_z, p.far_z = prm->far_z, p.tan_h = prm->tan_h, p.tan_v = prm->tan_v;

  SOGM_HIP_CHECK(hipSetDevice(test->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = join_update(test, st)) return rc;
  if (int rc = join_update(truth, st)) return rc;
  const MapView vt = view_of(test), vg = view_of(truth);
  const int     rows = test->n_agents * a.T;
  hipLaunchKernelGGL(k_map_audit_rows, dim3((rows + 63) / 64), dim3(64), 0, st, vt, vg, p, out, out_dt);
  // (more dynamic LDS than the 64 KB a launch gets by default: the attribute is a host-side setting of the function)
  SOGM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_map_audit<MASKED>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, AUDIT_LDS_BYTES - AUDIT_LDS_RESERVED));
  hipLaunchKernelGGL(k_map_audit<MASKED>, dim3(p.lay.slabs, test->n_agents), dim3(MAPAUDIT_WG), (size_t)p.lay.bytes, st, vt, vg,
                     p, cam_rot, out, reinterpret_cast<const unsigned long long *>(mask));
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
}  // namespace
}  // namespace sogm

extern "C" int sogm_map_audit(sogm_ctx *test, sogm_ctx *truth, const SogmMapAuditParams *prm, const double *cam_rot,
                              SogmMapAuditRow *out, double *out_dt, void *stream) {
  return sogm::map_audit_entry<false>(test, truth, prm, cam_rot, nullptr, out, out_dt, stream);
}

extern "C" int sogm_map_audit_masked(sogm_ctx *test, sogm_ctx *truth, const SogmMapAuditParams *prm, const uint64_t *mask,
                                     SogmMapAuditRow *out, double *out_dt, void *stream) {
  return sogm::map_audit_entry<true>(test, truth, prm, nullptr, mask, out, out_dt, stream);
}
