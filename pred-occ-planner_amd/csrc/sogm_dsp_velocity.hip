// sogm_dsp_velocity.hip — velocityEstimationThread (dsp_dynamic.h:1487-1678) of the particle map for gfx950: k_dsp_velocity
// and its launcher (sogm_update_dsp with labels == NULL, sogm_dsp.hip).
//
// One workgroup per agent (see oracle/dsp_oracle.cpp::velocityEstimation for the restated third-party pieces):
//   ground split -> Euclidean clustering of the non-ground points (connected components under "squared distance
//   < tolerance^2": neighbour lists by brute force over the LDS-resident cloud, min-label propagation with pointer
//   jumping; a component's label = its smallest index = PCL's seed) -> clusters ordered like
//   std::sort(rbegin, rend, size <) (libstdc++'s introsort restated, ties included) -> centres summed in ascending
//   index order -> gated association with the previous frame's clusters (optimal assignment, same scan order as
//   the oracle) -> input_cloud_with_velocity rewritten in the reference's order:
//   [possibly-dynamic clusters][ground points][static clusters].  Points of rejected (small) clusters vanish.
// The kernel is the list of these steps; what a single lane does of them is plain C++ in sogm_dsp_velocity.hpp.
#include <hip/hip_runtime.h>

#include "sogm_dsp_velocity.hpp"

namespace sogm {
namespace {

constexpr int VEL_THREADS = 1024;
constexpr int VEL_TRIPS   = VEL_MAX_POINTS / VEL_THREADS;  // points a thread stages in registers
constexpr int NO_POINT    = 0x7fffffff;                    // cidx of a staging slot past the cloud
constexpr int NO_CLUSTER  = 0xFFFF;                        // label of a point in no accepted cluster

// the kernel's static LDS (the arrays first: each starts on a 16-byte boundary, as separate __shared__ arrays would, so
// that an Item or a row of v moves in one LDS access)
struct alignas(16) VelShared {
  int       scan[VEL_THREADS];
  vel::Item item[VEL_MAX_CLUSTERS];
  int       root[VEL_MAX_CLUSTERS], size[VEL_MAX_CLUSTERS], off[VEL_MAX_CLUSTERS], dynseq[VEL_MAX_CLUSTERS];
  float     cx[VEL_MAX_CLUSTERS], cy[VEL_MAX_CLUSTERS], cz[VEL_MAX_CLUSTERS];
  float     v[VEL_MAX_DYN][4];  // vx vy vz intensity of the possibly-dynamic clusters
  int       base_ng, base_g, changed, nc, err, total_dyn, n_static;
};

// 2. neighbour lists: FLANN L2_Simple squared distance, strictly below (float)(tolerance^2)
__device__ __forceinline__ void neighbour_lists(VelShared &sh, const vel::Lds &l, int m, float vres, unsigned short *adj, int *deg) {
  const double tol = (double)(2 * vres);
  const float  r2  = (float)(tol * tol);
  for (int i = threadIdx.x; i < m; i += VEL_THREADS) {
    const float ax = l.sx[i], ay = l.sy[i], az = l.sz[i];
    int         c  = 0;
    for (int j = 0; j < m; ++j) {
      float df = ax - l.sx[j], d2 = 0.f;
      d2 += df * df;
      df = ay - l.sy[j];
      d2 += df * df;
      df = az - l.sz[j];
      d2 += df * df;
      if (d2 < r2 && j != i) {
        if (c < VEL_ADJ_CAP) adj[(size_t)i * VEL_ADJ_CAP + c] = (unsigned short)j;
        ++c;
      }
    }
    if (c > VEL_ADJ_CAP) {
      sh.err = 2;  // denser than a voxel-filtered cloud: neighbours were dropped
      c      = VEL_ADJ_CAP;
    }
    deg[i]   = c;
    l.lab[i] = i;
  }
}

// 3. connected components: min-label propagation + pointer jumping to the fixed point
__device__ __forceinline__ void connected_components(VelShared &sh, int *lab, int m, const unsigned short *adj, const int *deg) {
  const int tid = threadIdx.x;
  for (int round = 0; round < 4096; ++round) {
    if (tid == 0) sh.changed = 0;
    __syncthreads();
    for (int i = tid; i < m; i += VEL_THREADS) {
      int mn = lab[i];
      const int dg = deg[i];
      for (int q = 0; q < dg; ++q) {
        const int l = lab[adj[(size_t)i * VEL_ADJ_CAP + q]];
        mn          = l < mn ? l : mn;
      }
      if (mn < lab[i]) {
        atomicMin(&lab[lab[i]], mn);  // hook the old root as well
        atomicMin(&lab[i], mn);
        sh.changed = 1;
      }
    }
    __syncthreads();
    for (int i = tid; i < m; i += VEL_THREADS) {
      int l = lab[i];
      while (lab[l] < l) l = lab[l];
      lab[i] = l;
    }
    __syncthreads();
    if (!sh.changed) break;
    __syncthreads();
  }
}

// 4. sizes per root; one lane then accepts the clusters in seed (= root index) order
__device__ __forceinline__ void sizes_and_accepted_clusters(VelShared &sh, const vel::Lds &l, int m) {
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += VEL_THREADS) l.aux[i] = 0;
  __syncthreads();
  for (int i = tid; i < m; i += VEL_THREADS) atomicAdd(&l.aux[l.lab[i]], 1);
  __syncthreads();
  if (tid != 0) return;
  int nc = 0;
  for (int i = 0; i < m; ++i)
    if (l.lab[i] == i && l.aux[i] >= vel::MIN_CLUSTER_SIZE && l.aux[i] <= vel::MAX_CLUSTER_SIZE) {
      if (nc < VEL_MAX_CLUSTERS) {
        sh.root[nc] = i;
        sh.size[nc] = l.aux[i];
      }
      ++nc;
    }
  if (nc > VEL_MAX_CLUSTERS) {
    sh.err = 3;
    nc     = VEL_MAX_CLUSTERS;
  }
  sh.nc = nc;
}

// 5. the same lane orders them as EuclideanClusterExtraction::extract does — std::sort(clusters.rbegin(), clusters.rend(),
//    size <): cluster slot c (extraction order) = item[nc - 1 - c] — then every point finds its slot through its root.
//    Returns the number of clusters.
__device__ __forceinline__ int extraction_order_and_slots(VelShared &sh, const vel::Lds &l, int m) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    const int nc = sh.nc;
    for (int k = 0; k < nc; ++k) {  // the reversed sequence
      sh.item[k].size = sh.size[nc - 1 - k];
      sh.item[k].id   = nc - 1 - k;
    }
    vel::std_sort(sh.item, nc);
  }
  __syncthreads();
  const int nc = sh.nc;
  for (int i = tid; i < m; i += VEL_THREADS) l.aux[i] = -1;
  __syncthreads();
  for (int c = tid; c < nc; c += VEL_THREADS) l.aux[sh.root[sh.item[nc - 1 - c].id]] = c;  // slot of a root
  __syncthreads();
  for (int i = tid; i < m; i += VEL_THREADS) {
    const int sl = l.aux[l.lab[i]];  // lab[i] is the point's root; aux[root] the cluster's slot (or -1)
    l.lab[i]     = sl >= 0 ? sl : NO_CLUSTER;
  }
  return nc;
}

// 6. centres (sums in ascending index order, :1533-1542) and rank of every point inside its cluster
__device__ __forceinline__ void centres_and_ranks(VelShared &sh, const vel::Lds &l, int m, int nc) {
  for (int c = threadIdx.x; c < nc; c += VEL_THREADS) {
    float cx = 0.f, cy = 0.f, cz = 0.f;
    int   cnt = 0;
    for (int i = 0; i < m; ++i)
      if (l.lab[i] == c) {
        cx += l.sx[i];
        cy += l.sy[i];
        cz += l.sz[i];
        l.aux[i] = cnt;
        ++cnt;
      }
    sh.cx[c]   = cx / (float)cnt;
    sh.cy[c]   = cy / (float)cnt;
    sh.cz[c]   = cz / (float)cnt;
    sh.size[c] = cnt;  // now in extraction order
  }
}

// 7. (one lane) possibly-dynamic split, association with the previous frame, output offsets, the agent's counters
__device__ __forceinline__ void split_and_associate(VelShared &sh, const vel::Lds &l, DspAgent &s, int nc, int n_ground, int max_pts) {
  const vel::Clusters cl = {nc, sh.size, sh.cx, sh.cy, sh.cz};
  const int nd = vel::dynamic_split(cl, n_ground, sh.dynseq, sh.off, sh.v, &sh.total_dyn, &sh.n_static, &sh.err);
  // cost / gate matrices live in the (now free) coordinate arrays of the dynamic LDS: max_pts floats each;
  // dt = delt_t_from_last_observation (:213)
  const int matched = vel::associate(cl, sh.dynseq, nd, s.vel_last, s.vel_n_last, s.odom[3], l.sx, l.sy, max_pts, sh.v, &sh.err);
  s.vel_n_last   = vel::hand_over(cl, sh.dynseq, sh.v, s.vel_last);
  s.vel_clusters = nc;
  s.vel_dynamic  = nd;
  s.vel_matched  = matched;
  if (sh.err) s.vel_err = sh.err;
  s.n_born = sh.total_dyn + n_ground + sh.n_static;
}

// 8. input_cloud_with_velocity in the reference's order (every thread writes the points it read)
__device__ __forceinline__ void write_born(const VelShared &sh, const vel::Lds &l, float *born, int *born_src, int trips,
                                           const float (&px)[VEL_TRIPS][3], const int (&cidx)[VEL_TRIPS]) {
#pragma unroll
  for (int t = 0; t < VEL_TRIPS; ++t) {
    if (t >= trips) break;
    const int ci = cidx[t];
    if (ci == NO_POINT) continue;
    int   pos;
    float lv[4] = {0.f, 0.f, 0.f, 0.f};
    if (ci < 0) {
      pos = sh.total_dyn + (-ci - 1);
    } else {
      const int c = l.lab[ci];
      if (c == NO_CLUSTER) continue;  // no accepted cluster: the point is dropped
      pos = sh.off[c] + l.aux[ci];
      if (sh.dynseq[c] >= 0)
        for (int j = 0; j < 4; ++j) lv[j] = sh.v[sh.dynseq[c]][j];
    }
    float *o = born + (size_t)pos * 7;
    o[0]     = px[t][0];
    o[1]     = px[t][1];
    o[2]     = px[t][2];
    for (int j = 0; j < 4; ++j) o[3 + j] = lv[j];
    born_src[pos] = t * VEL_THREADS + threadIdx.x;  // the input index of px[t]
  }
}

}  // namespace

__global__ __launch_bounds__(1024) void k_dsp_velocity(DspDev d, const int32_t *__restrict__ range, float vres) {
  extern __shared__ __attribute__((aligned(16))) float s_vel[];
  __shared__ VelShared sh;
  const int a   = blockIdx.x;
  DspAgent &s   = d.ag[a];
  const int tid = threadIdx.x;
  if (!s.ok) return;
  int n = range[a * 2 + 1] - range[a * 2];
  if (n > d.max_pts) n = d.max_pts;
  if (n <= 0) return;  // :1488 — input_cloud_with_velocity and the previous clusters stay as they are
  const vel::Lds l(s_vel, d.max_pts);
  float *born = d.born + d.point_base(a) * 7;
  if (tid == 0) {
    sh.base_ng = 0;
    sh.base_g  = 0;
    sh.err     = 0;
  }
  __syncthreads();
  // (max_points <= VEL_MAX_POINTS is checked by sogm_dsp_create: the register staging holds VEL_TRIPS points per thread)
  float px[VEL_TRIPS][3];
  int   cidx[VEL_TRIPS];
  const int trips = (n + VEL_THREADS - 1) / VEL_THREADS;
  // 1. ground split (:1497-1507), order-preserving compaction of both lists; a thread keeps its points' data:
  //    cidx >= 0: index in the non-ground list; < 0: -(ground rank) - 1.  (Not a function of its own: behind any call
  //    boundary — function, per-trip function, lambda — the kernel takes 107 VGPRs instead of 93, profiles/EXPERIMENTS.md.)
#pragma unroll
  for (int t = 0; t < VEL_TRIPS; ++t) {
    if (t >= trips) break;
    const int k = t * VEL_THREADS + tid;
    float x = 0.f, y = 0.f, z = 0.f;
    bool  in = k < n, ng = false;
    if (in) {
      x  = born[(size_t)k * 7];
      y  = born[(size_t)k * 7 + 1];
      z  = born[(size_t)k * 7 + 2];
      ng = z > vres;
    }
    // two exclusive scans over the workgroup (non-ground and ground flags)
    const unsigned long long bn = __ballot(in && ng), bg = __ballot(in && !ng);
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    if (lane == 0) {
      sh.scan[wave]      = __popcll(bn);
      sh.scan[16 + wave] = __popcll(bg);
    }
    __syncthreads();
    int on = 0, og = 0, tn = 0, tg = 0;
    for (int w = 0; w < 16; ++w) {
      on += w < wave ? sh.scan[w] : 0;
      og += w < wave ? sh.scan[16 + w] : 0;
      tn += sh.scan[w];
      tg += sh.scan[16 + w];
    }
    const int rn = sh.base_ng + on + __popcll(bn & lt), rg = sh.base_g + og + __popcll(bg & lt);
    px[t][0] = x;
    px[t][1] = y;
    px[t][2] = z;
    cidx[t]  = !in ? NO_POINT : (ng ? rn : -rg - 1);
    if (in && ng) {
      l.sx[rn] = x;
      l.sy[rn] = y;
      l.sz[rn] = z;
    }
    __syncthreads();
    if (tid == 0) {
      sh.base_ng += tn;
      sh.base_g += tg;
    }
    __syncthreads();
  }
  const int m = sh.base_ng, n_ground = sh.base_g;
  unsigned short *adj = d.vel_adj + d.point_base(a) * VEL_ADJ_CAP;
  int            *deg = d.vel_deg + d.point_base(a);
  neighbour_lists(sh, l, m, vres, adj, deg);
  __syncthreads();
  connected_components(sh, l.lab, m, adj, deg);
  sizes_and_accepted_clusters(sh, l, m);
  const int nc = extraction_order_and_slots(sh, l, m);
  __syncthreads();
  centres_and_ranks(sh, l, m, nc);
  __syncthreads();
  if (tid == 0) split_and_associate(sh, l, s, nc, n_ground, d.max_pts);
  __syncthreads();
  write_born(sh, l, born, d.born_src + d.point_base(a), trips, px, cidx);
}

int launch_dsp_velocity(const DspDev &d, const int32_t *range, float vres, hipStream_t st) {
  const size_t lds = vel::Lds::bytes(d.max_pts);  // (checked against the device limit in sogm_dsp_create)
  SOGM_HIP_CHECK(raise_dynamic_lds<k_dsp_velocity>(lds));
  hipLaunchKernelGGL(k_dsp_velocity, dim3((unsigned)d.A), dim3(VEL_THREADS), lds, st, d, range, vres);
  return SOGM_OK;
}

// k_dsp_velocity keeps the cloud in LDS: its dynamic LDS on top of its static arrays must fit the workgroup limit of THIS
// device (160 KiB on gfx950: max_points <= ~7.4 k)
int velocity_lds_fits(int max_points, int device) {
  hipFuncAttributes fa;
  int               lds_max = 0;
  SOGM_HIP_CHECK(hipFuncGetAttributes(&fa, (const void *)k_dsp_velocity));
  SOGM_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  return vel::Lds::bytes(max_points) + fa.sharedSizeBytes <= (size_t)lds_max ? 1 : 0;
}

}  // namespace sogm
