// sogm_query.hip — readers of a finished map (every entry joins an update flow still building it first):
//   k_query_clear        batched getClearOcccupancy.            fake_particle_risk_voxel.cpp:309-346
//   k_obstacle_points    one workgroup per corridor box, order-preserving block-scan compaction.
//                                                               map.cpp:480-518 / risk_base.cpp:295-337
//   k_traj_safe          BaselinePlanner::isTrajSafe per agent. baseline.cpp:45-68
//   k_slabs_to_vt / k_vt_to_slabs   layout converters for parity I/O and futureRiskCallback.
#include <hip/hip_runtime.h>

#include "sogm_device.hpp"

namespace sogm {

__global__ __launch_bounds__(256) void k_query_clear(MapView m, const int32_t *__restrict__ agent,
                                                     const double *__restrict__ pos,
                                                     const double *__restrict__ t, int t_is_index,
                                                     int n, int8_t *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int a = agent[i];
  int       r;
  if (t_is_index) {
    r = query_clear_idx(m, a, pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2], (int)t[i]);
  } else {
    r = query_clear_time(m, a, pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2], t[i]);
  }
  out[i] = (int8_t)r;
}

// Order-preserving extraction.  Cells of the box are visited in the reference's z,y,x order, 256
// cells per trip; each lane counts the slices of its cell that exceed the threshold, a block-wide
// exclusive scan turns counts into output offsets, so the emitted sequence is exactly the
// reference's (FIRI's greedy selection breaks ties by point order).
__global__ __launch_bounds__(256) void k_obstacle_points(
    MapView m, const int32_t *__restrict__ agent_idx, const double *__restrict__ box_lo,
    const double *__restrict__ box_hi, const double *__restrict__ t0v,
    const double *__restrict__ t1v, double *__restrict__ out_pts, int32_t *__restrict__ out_cnt,
    int cap) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const GridGeom &g     = m.g;
  const int       b     = blockIdx.x;
  const int       agent = agent_idx[b];
  const float    *pose  = m.poses + agent * 3;
  const double    stamp = m.stamps[agent];
  const double    tr    = (double)g.dt;
  int             js    = (int)floor((t0v[b] - stamp) / tr);
  int             je    = (int)ceil((t1v[b] - stamp) / tr);
  js                    = js < 0 ? 0 : js;
  js                    = js > g.T ? g.T : js;
  je                    = je > g.T ? g.T : je;
  je                    = je < 0 ? 0 : je;
  if (je > g.T - 1) je = g.T - 1;  // slices >= T do not exist (reference reads one past the end)
  int lx = (int)((box_lo[b * 3 + 0] - pose[0] + g.rx) / g.res);
  int ly = (int)((box_lo[b * 3 + 1] - pose[1] + g.ry) / g.res);
  int lz = (int)((box_lo[b * 3 + 2] - pose[2] + g.rz) / g.res);
  int hx = (int)((box_hi[b * 3 + 0] - pose[0] + g.rx) / g.res);
  int hy = (int)((box_hi[b * 3 + 1] - pose[1] + g.ry) / g.res);
  int hz = (int)((box_hi[b * 3 + 2] - pose[2] + g.rz) / g.res);
  hx     = min(hx, g.L - 1);
  hy     = min(hy, g.W - 1);
  hz     = min(hz, g.H - 1);
  lx     = max(lx, 0);
  ly     = max(ly, 0);
  lz     = max(lz, 0);
  const int nx = hx - lx + 1, ny = hy - ly + 1, nz = hz - lz + 1;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  if (nx <= 0 || ny <= 0 || nz <= 0 || js > je) {
    if (threadIdx.x == 0) out_cnt[b] = 0;
    return;
  }
  const int    cells = nx * ny * nz;
  const void  *grid0 = m.slab(agent, 0);
  double      *outp  = out_pts + (size_t)b * cap * 3;
  const int    lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (int c0 = 0; c0 < cells; c0 += blockDim.x) {
    const int c    = c0 + threadIdx.x;
    int       cnt  = 0;
    unsigned  mask = 0;  // bit j-js set when slice j exceeds
    int       vi   = 0;
    if (c < cells) {
      const int x = lx + c % nx;
      const int y = ly + (c / nx) % ny;
      const int z = lz + c / (nx * ny);
      vi          = x + y * g.L + z * g.L * g.W;
      const int pi = g.phys(x, y, z);
      for (int j = js; j <= je; ++j) {
        const float thr =
            g.map_kind == SOGM_MAP_FAKE ? g.risk_threshold : g.risk_threshold - g.decay_voxel * (float)j;
        if (cell_ld(grid0, (size_t)j * g.V + pi, g.half) > thr) {
          ++cnt;
          mask |= 1u << (j - js);
        }
      }
    }
    // wave-level inclusive scan (64 lanes), then 4-wave combine through LDS
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int wave_off = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
      const int v = s_wave[w];
      if (w < wave) wave_off += v;
      total += v;
    }
    const int base = s_base;
    int       off  = base + wave_off + incl - cnt;
    if (cnt) {
      float fx, fy, fz;
      g.corner_of(vi, pose, fx, fy, fz);
      for (int j = 0; j < 32 && (mask >> j); ++j) {
        if ((mask >> j) & 1u) {
          if (off < cap) {
            outp[off * 3 + 0] = (double)fx;
            outp[off * 3 + 1] = (double)fy;
            outp[off * 3 + 2] = (double)fz;
          }
          ++off;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) s_base = base + total;
    __syncthreads();
  }
  if (threadIdx.x == 0) out_cnt[b] = s_base;
}

// ------------------------------------------------------------------------------------------------
// layout converters ([T][V] slabs <-> reference [V][T])
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_slabs_to_vt(const void *__restrict__ slabs, GridGeom g, float *__restrict__ vt) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= g.V) return;
  const int p = g.phys_of(v);
  for (int t = 0; t < g.T; ++t) vt[(size_t)v * g.T + t] = cell_ld(slabs, (size_t)t * g.V + p, g.half);
}
__global__ __launch_bounds__(256) void k_vt_to_slabs(const float *__restrict__ vt, GridGeom g, void *__restrict__ slabs) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= g.V) return;
  const int p = g.phys_of(v);
  for (int t = 0; t < g.T; ++t) cell_st(slabs, (size_t)t * g.V + p, vt[(size_t)v * g.T + t], g.half);
}

// BaselinePlanner::isTrajSafe (plan_manager/src/baseline.cpp:45-68): sample the executed trajectory every
// 0.1 s from "now" up to min(T, duration) and query the SOGM at the sample's time after the map stamp.
__global__ __launch_bounds__(64) void k_traj_safe(MapView m, const SogmTrajRecord *__restrict__ rec,
                                                  const double *__restrict__ t_now, double T,
                                                  int32_t *__restrict__ out) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= m.n_agents) return;
  out[a] = traj_safe_agent(m, a, rec[a], t_now[a], T, 0, 1);
}

}  // namespace sogm

using namespace sogm;

extern "C" {

int sogm_query_clear(sogm_ctx *c, const int32_t *agent_idx, const double *pos_xyz, const double *t,
                     int t_is_index, int n_q, int8_t *out, void *stream) {
  if (!c || !agent_idx || !pos_xyz || !t || !out || n_q < 0) return SOGM_ERR_INVALID_ARG;
  if (!c->updated) return SOGM_ERR_STATE;
  if (n_q == 0) return SOGM_OK;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = sogm::join_update(c, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(k_query_clear, dim3((n_q + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     view_of(c), agent_idx, pos_xyz, t, t_is_index, n_q, out);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_obstacle_points(sogm_ctx *c, const int32_t *agent_idx, const double *box_lo,
                         const double *box_hi, const double *t0, const double *t1, int n_b,
                         double *out_pts, int32_t *out_counts, int cap, void *stream) {
  if (!c || !agent_idx || !box_lo || !box_hi || !t0 || !t1 || !out_pts || !out_counts ||
      n_b < 0 || cap <= 0)
    return SOGM_ERR_INVALID_ARG;
  if (!c->updated) return SOGM_ERR_STATE;
  if (n_b == 0) return SOGM_OK;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = sogm::join_update(c, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(k_obstacle_points, dim3(n_b), dim3(256), 0, (hipStream_t)stream, view_of(c),
                     agent_idx, box_lo, box_hi, t0, t1, out_pts, out_counts, cap);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_traj_safe(sogm_ctx *c, const SogmTrajRecord *records, const double *t_now, double check_duration,
                   int32_t *out_safe, void *stream) {
  if (!c || !records || !t_now || !out_safe) return SOGM_ERR_INVALID_ARG;
  if (!c->updated) return SOGM_ERR_STATE;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = sogm::join_update(c, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(k_traj_safe, dim3((c->n_agents + 63) / 64), dim3(64), 0, (hipStream_t)stream, view_of(c),
                     records, t_now, check_duration, out_safe);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_set_future_risk(sogm_ctx *c, const float *grid_vt, const float *poses,
                         const double *stamps, void *stream) {
  if (!c || !grid_vt || !poses || !stamps) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = sogm::join_update(c, st)) return rc;
  SOGM_HIP_CHECK(hipMemcpyAsync(c->d_poses, poses, sizeof(float) * 3 * c->n_agents,
                                hipMemcpyDeviceToDevice, st));
  SOGM_HIP_CHECK(hipMemcpyAsync(c->d_stamps, stamps, sizeof(double) * c->n_agents,
                                hipMemcpyDeviceToDevice, st));
  if (c->pool.precleared()) {
    int rc = sogm::adopt_preclear(c, st);
    if (rc) return rc;
  }
  const int    V = c->geom.V, T = c->spec.T;
  const size_t per = (size_t)V * T;
  c->pool.dense_write_current();  // every cell is written: the next reset of this grid is the dense clear
  for (int a = 0; a < c->n_agents; ++a) {
    hipLaunchKernelGGL(k_vt_to_slabs, dim3((V + 255) / 256), dim3(256), 0, st, grid_vt + a * per, c->geom,
                       (void *)((char *)c->d_grid + a * per * c->cell_bytes()));
  }
  SOGM_HIP_CHECK(hipGetLastError());
  c->updated = 1;
  return SOGM_OK;
}

int sogm_download_reference_layout(sogm_ctx *c, int agent, float *out) {
  if (!c || !out || agent < 0 || agent >= c->n_agents) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  const int    V = c->geom.V, T = c->spec.T;
  const size_t per = (size_t)V * T;
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_slabs_to_vt, dim3((V + 255) / 256), dim3(256), 0, 0,
                     (const void *)((const char *)c->d_grid + (size_t)agent * per * c->cell_bytes()), c->geom,
                     c->d_scratch_vt);
  SOGM_HIP_CHECK(hipGetLastError());
  SOGM_HIP_CHECK(hipMemcpy(out, c->d_scratch_vt, per * sizeof(float), hipMemcpyDeviceToHost));
  return SOGM_OK;
}

int sogm_map_state(sogm_ctx *c, int agent, double *out_time, float *out_center, void *stream) {
  if (!c || agent < 0 || agent >= c->n_agents || (!out_time && !out_center)) return SOGM_ERR_INVALID_ARG;
  if (!c->updated) return SOGM_ERR_STATE;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (out_time)
    SOGM_HIP_CHECK(hipMemcpyAsync(out_time, c->d_stamps + agent, sizeof(double), hipMemcpyDeviceToHost, st));
  if (out_center)
    SOGM_HIP_CHECK(hipMemcpyAsync(out_center, c->d_poses + 3 * agent, 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  SOGM_HIP_CHECK(hipStreamSynchronize(st));
  return SOGM_OK;
}

}  // extern "C"
