// sogm_dsp.hip — batched particle-filter SOGM (dsp_map::DSPMap, plan_env/include/plan_env/dsp_dynamic.h)
// for gfx950, behind sogm_dsp_* / sogm_update_dsp in include/sogm_abi.h.
//
// The reference sweeps the voxels sequentially and lets every particle take the first empty slot of
// its destination voxel / FOV pyramid at the moment it is processed.  That order dependence is the
// only coupling between particles, so it is reproduced exactly WITHOUT a sequential sweep:
//
//   * every particle's new state is a pure function of its old state (LIMIT_MOVEMENT_IN_XY_PLANE
//     keeps vz == 0, so the velocity-noise branches of mapPrediction/moveParticle never draw:
//     |vx*vy*vz| < 1e-6 always) -> one thread per slot (k_dsp_predict);
//   * the sweep order is the key  src_voxel*16 + src_slot.  For a destination voxel B the events in
//     time order are: arrivals with key < B*16 (B still holds all of its own particles), B's own
//     departures, arrivals with key > B*16.  Arrivals are linked into a per-voxel list; one thread
//     per voxel keeps the <= S smallest keys of either phase and replays "lowest empty slot"
//     (k_dsp_place).  Only S arrivals per phase can ever be placed, so the selection is exact;
//   * pyramid lists hold the first SP (=20) placed particles in key order (k_dsp_pyramids); a later
//     one vanishes (moveParticle returns -2), which frees its slot for later arrivals — resolved by
//     iterating place/pyramids to the fixed point (monotone; rounds after convergence exit at once);
//   * new-born particles: Gaussian-table offsets are closed-form prefix sums over (point, particle)
//     order (k_dsp_newborn, block scan), slots again by ordered first-fit (k_dsp_place_born).
//
// Data layout (HBM, per agent): particle store as SoA with 16 slots per voxel —
//   flag u8 [V][16] (one 16-B load tells whether a voxel holds anything) and six fp32 planes
//   vx, vy, px, py, pz, w [V][16] (one 64-B line per voxel and field, touched only where occupied);
//   future-occupancy accumulators fut[T][V] in the SOGM's own time-major layout, so that publishing
//   is a straight copy.  vz and the per-particle update time are not stored (always 0 / never read).
// Everything is HBM/latency-bound gather-scatter work; no MFMA.
#include <hip/hip_runtime.h>

#include "sogm_dsp.hpp"

namespace sogm {

// ---- update: begin ------------------------------------------------------------------------------
// DSPMap::update :176-229: odometry checks, deltas, boundary-plane rotation.
__global__ void k_dsp_begin(DspDev d, const float *__restrict__ pos, const float *__restrict__ quat,
                            const double *__restrict__ stamps, int32_t *__restrict__ out_ok) {
  const int a  = blockIdx.x;
  DspAgent &s  = d.ag[a];
  __shared__ int s_ok;
  if (threadIdx.x == 0) {
    const float  px = pos[a * 3], py = pos[a * 3 + 1], pz = pos[a * 3 + 2];
    const float  qw = quat[a * 4], qx = quat[a * 4 + 1], qy = quat[a * 4 + 2], qz = quat[a * 4 + 3];
    const double t  = stamps[a];
    if (s.first) {
      s.last_p[0] = px;
      s.last_p[1] = py;
      s.last_p[2] = pz;
      s.last_t    = t;
      s.first     = 0;
    }
    int ok = 1;
    if (fabsf(qw) > 1.001f || fabsf(qx) > 1.001f || fabsf(qy) > 1.001f || fabsf(qz) > 1.001f) ok = 0;
    const float dx = px - s.last_p[0], dy = py - s.last_p[1], dz = pz - s.last_p[2];
    const float dt = (float)(t - s.last_t);
    if (ok && (fabsf(dx) > 10.f || fabsf(dy) > 10.f || fabsf(dz) > 10.f || dt < 0.f || dt > 10.f)) ok = 0;
    if (ok) {
      s.cur[0] = s.last_p[0] = px;
      s.cur[1] = s.last_p[1] = py;
      s.cur[2] = s.last_p[2] = pz;
      s.last_t  = t;
      s.quat[0] = qw;
      s.quat[1] = qx;
      s.quat[2] = qy;
      s.quat[3] = qz;
      s.odom[0] = -dx;
      s.odom[1] = -dy;
      s.odom[2] = -dz;
      s.odom[3] = dt;
      s.update_time += dt;
      s.cand_cnt = 0;
      s.born_cnt = 0;
      s.n_obs    = 0;
      for (int r = 0; r < DSP_ROUNDS; ++r) s.changed[r] = 0;
    }
    s.ok = ok;
    if (out_ok) out_ok[a] = ok;
    s_ok = ok;
  }
  __syncthreads();
  if (!s_ok) return;
  const float q[4] = {quat[a * 4], quat[a * 4 + 1], quat[a * 4 + 2], quat[a * 4 + 3]};
  for (int i = threadIdx.x; i < d.nph + 1; i += blockDim.x)
    rotate_q(d.bp_ori_h + i * 3, q, d.bp_h + (d.bph_base(a) + i) * 3);
  for (int i = threadIdx.x; i < d.npv + 1; i += blockDim.x)
    rotate_q(d.bp_ori_v + i * 3, q, d.bp_v + (d.bpv_base(a) + i) * 3);
}

// ---- update: observation binning (:231-297) -------------------------------------------------------
// One workgroup per agent walks the cloud in input order, 256 points per trip; the slot of a point
// inside its pyramid is (points of earlier trips) + (earlier lanes of this trip in the same pyramid).
__global__ __launch_bounds__(256) void k_dsp_observe(DspDev d, const float *__restrict__ pts,
                                                     const float *__restrict__ labels,
                                                     const int32_t *__restrict__ range) {
  extern __shared__ int s_dyn[];
  const int a = blockIdx.x;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  int *s_cnt = s_dyn;          // [NP]
  int *s_max = s_dyn + d.NP;   // [NP] float bits
  __shared__ int   s_pi[256];
  __shared__ float s_bh[181 * 3], s_bv[181 * 3];
  __shared__ int   s_valid, s_nobs;
  for (int i = threadIdx.x; i < d.NP; i += 256) {
    s_cnt[i] = 0;
    s_max[i] = -1;
  }
  for (int i = threadIdx.x; i < (d.nph + 1) * 3; i += 256) s_bh[i] = d.bp_h[d.bph_base(a) * 3 + i];
  for (int i = threadIdx.x; i < (d.npv + 1) * 3; i += 256) s_bv[i] = d.bp_v[d.bpv_base(a) * 3 + i];
  if (threadIdx.x == 0) {
    s_valid = 0;
    s_nobs  = 0;
  }
  __syncthreads();
  const int begin = range[a * 2];
  int       n     = range[a * 2 + 1] - begin;
  if (n > d.max_pts) {
    n = d.max_pts;
    if (threadIdx.x == 0) s.err_points += 1;
  }
  const float q[4] = {s.quat[0], s.quat[1], s.quat[2], s.quat[3]};
  const float c0 = s.cur[0], c1 = s.cur[1], c2 = s.cur[2];
  float      *born = d.born + d.point_base(a) * 7;
  float      *pc   = d.pc + d.obs_base(a) * 5;
  for (int base = 0; base < n; base += 256) {
    const int k  = base + threadIdx.x;
    int       pi = -1;
    float     r[3] = {0.f, 0.f, 0.f};
    if (k < n) {
      rotate_q(pts + (size_t)(begin + k) * 3, q, r);
      // input_cloud_with_velocity (:1494-1500,1651-1660): rotated + current_position, labels as given
      born[(size_t)k * 7 + 0] = r[0] + c0;
      born[(size_t)k * 7 + 1] = r[1] + c1;
      born[(size_t)k * 7 + 2] = r[2] + c2;
      d.born_src[d.point_base(a) + k] = k;  // (k_dsp_velocity rewrites it with the list)
      for (int j = 0; j < 4; ++j)  // labels == NULL: k_dsp_velocity fills (and reorders) the list afterwards
        born[(size_t)k * 7 + 3 + j] = labels ? labels[(size_t)(begin + k) * 4 + j] : 0.f;
      pi = pyramid_of(s_bh, s_bv, d.nph, d.npv, r[0], r[1], r[2]);
    }
    s_pi[threadIdx.x] = pi;
    __syncthreads();
    if (pi >= 0) {
      int rank = 0;
      for (int j = 0; j < (int)threadIdx.x; ++j) rank += (s_pi[j] == pi);
      const int seq = s_cnt[pi] + rank;  // s_cnt is only advanced after the barrier below
      const float len = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      if (seq < d.OM - 1) {  // slot OM-1 is overwritten by every later point and never read (:287-290)
        float *o = pc + ((size_t)pi * d.OM + seq) * 5;
        o[0]     = r[0];
        o[1]     = r[1];
        o[2]     = r[2];
        o[3]     = 0.f;
        o[4]     = len;
        d.obs_list[d.point_base(a) + atomicAdd(&s_nobs, 1)] = pi * d.OM + seq;
      }
      atomicMax(&s_max[pi], __float_as_int(len));
      atomicAdd(&s_valid, 1);
    }
    __syncthreads();
    if (pi >= 0) atomicAdd(&s_cnt[pi], 1);
    __syncthreads();
  }
  for (int i = threadIdx.x; i < d.NP; i += 256) {
    const int c                  = s_cnt[i];
    d.nobs[d.pyr_base(a) + i]   = c >= d.OM ? d.OM - 1 : c;
    d.maxlen[d.pyr_base(a) + i] = s_max[i];
  }
  if (threadIdx.x == 0) {
    s.valid_points = s_valid;
    s.n_obs        = s_nobs;
    s.enb          = d.w_nb * (float)s_valid * (float)d.nb;  // :299-300
    if (n > 0) s.n_born = n;  // velocityEstimationThread returns early on an empty cloud (:1488)
  }
}

// ---- update: prediction (:663-748, moveParticle :1295-1372) ------------------------------------------
// One thread per voxel: a single 16-B load of the slot flags rejects empty voxels (the vast majority);
// occupied slots are then processed independently of each other.
__global__ __launch_bounds__(256) void k_dsp_predict(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  __shared__ float s_bh[181 * 3], s_bv[181 * 3];
  for (int i = threadIdx.x; i < (d.nph + 1) * 3; i += 256) s_bh[i] = d.bp_h[d.bph_base(a) * 3 + i];
  for (int i = threadIdx.x; i < (d.npv + 1) * 3; i += 256) s_bv[i] = d.bp_v[d.bpv_base(a) * 3 + i];
  __syncthreads();
  const int    v   = blockIdx.x * 256 + threadIdx.x;
  const size_t at0 = d.slot_base(a, v < d.V ? v : 0);
  uint4        f4  = {0u, 0u, 0u, 0u};
  if (v < d.V) f4 = *reinterpret_cast<const uint4 *>(d.flag + at0);
  if (!__any((f4.x | f4.y | f4.z | f4.w) != 0u)) return;  // wave-uniform: whole wave of empty voxels
  const unsigned w4[4] = {f4.x, f4.y, f4.z, f4.w};
  const float    ox = s.odom[0], oy = s.odom[1], oz = s.odom[2], dt = s.odom[3];
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // Compact the wave's occupied (voxel, slot) pairs into LDS, then process them 64 at a time: one round
  // of memory latency per 64 particles instead of one per slot index.
  __shared__ unsigned short s_list[4][64 * DSP_SLOTS];
  int n_act = 0;
#pragma unroll
  for (int p = 0; p < DSP_SLOTS; ++p) {
    const uint8_t            c   = (uint8_t)((w4[p >> 2] >> ((p & 3) * 8)) & 0xffu);
    const bool               act = (c == F_VALID || c == F_RESAMP);
    const unsigned long long m   = __ballot(act);
    if (act) s_list[wave][n_act + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)(lane * DSP_SLOTS + p);
    n_act += __popcll(m);
  }
  __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // LDS is in-order per wave; keep the compiler honest
  const int v0 = v - lane;
  for (int base = 0; base < n_act; base += 64) {
    const bool act = base + lane < n_act;
    const int  e   = act ? s_list[wave][base + lane] : 0;
    const int  vv = v0 + (e >> 4), p = e & (DSP_SLOTS - 1);
    const size_t at  = d.slot_base(a, act ? vv : 0) + p;
    const int    gid = vv * DSP_SLOTS + p;
    float        vx = 0.f, vy = 0.f, px = 0.f, py = 0.f, pz = 0.f;
    int          nv = -1, pyr = -1;
    bool         need = false;
    if (act) {
      vx = d.f[0][at];
      vy = d.f[1][at];
      px = d.f[2][at];
      py = d.f[3][at];
      pz = d.f[4][at];
      px += dt * vx + ox;
      py += dt * vy + oy;
      pz += dt * 0.f + oz;
      d.f[2][at] = px;
      d.f[3][at] = py;
      d.f[4][at] = pz;
      nv = voxel_index(d, px, py, pz);
      if (nv < 0) {  // moved out (:738-741): the slot frees up at this particle's own turn in the sweep
        d.flag[at] = F_DEPART;
        atomicAdd(&s.dbg_out, 1);
      } else {
        pyr = pyramid_of(s_bh, s_bv, d.nph, d.npv, px, py, pz);
        if (nv == vv) {
          d.flag[at] = F_VALID;
          need       = pyr >= 0;
        } else {
          d.flag[at] = F_DEPART;
          need       = true;
        }
      }
    }
    // one counter bump per wave instead of one same-address atomic per particle
    const unsigned long long m = __ballot(need);
    if (!m) continue;
    int base_c = 0;
    if (lane == __ffsll((long long)m) - 1) base_c = atomicAdd(&s.cand_cnt, __popcll(m));
    base_c = __shfl(base_c, __ffsll((long long)m) - 1);
    if (!need) continue;
    const int c_i = base_c + __popcll(m & ((1ull << lane) - 1ull));
    if (c_i >= d.cand_cap) {
      atomicAdd(&s.err_pool, 1);
      if (nv != vv) d.flag[at] = F_EMPTY;
      continue;
    }
    const size_t ci = d.cand_base(a) + c_i;
    d.c_key[ci]    = gid;
    d.c_dest[ci]   = nv;
    d.c_pyr[ci]    = pyr;
    d.c_kill[ci]   = 0;
    if (nv == vv) {
      d.c_assign[ci] = p;   // stay: slot known
      d.c_vnext[ci]  = -2;  // marks "stay"
    } else {
      d.c_assign[ci] = -1;
      float *pay     = d.c_pay + ci * 6;
      pay[0]         = vx;
      pay[1]         = vy;
      pay[2]         = px;
      pay[3]         = py;
      pay[4]         = pz;
      pay[5]         = d.f[5][at];
      d.c_vnext[ci]  = atomicExch(&d.vhead[d.voxel_base(a) + nv], c_i);
    }
    if (pyr >= 0) d.c_pnext[ci] = atomicExch(&d.phead[d.pyr_base(a) + pyr], c_i);
  }
}

// ---- update: ordered first-fit of arrivals, one thread per destination voxel ---------------------
__global__ __launch_bounds__(64) void k_dsp_place(DspDev d, int round) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  if (round > 0 && s.changed[round - 1] == 0) return;
  const int B = blockIdx.x * 64 + threadIdx.x;
  if (B >= d.V) return;
  int head = d.vhead[d.voxel_base(a) + B];
  if (head < 0) return;
  __shared__ int s_key[64][2 * DSP_SLOTS], s_id[64][2 * DSP_SLOTS];
  int *kb = s_key[threadIdx.x], *ib = s_id[threadIdx.x];  // [0,S): before, [16,16+S): after
  int  nb_ = 0, na_ = 0;
  const int    S = d.S, lo = B * DSP_SLOTS;
  const size_t cb = d.cand_base(a);
  for (int m = head; m >= 0; m = d.c_vnext[cb + m]) {
    d.c_assign[cb + m] = -1;
    if (d.c_kill[cb + m]) continue;
    const int key = d.c_key[cb + m];
    int *K, *I, *N;
    if (key < lo) {
      K = kb;
      I = ib;
      N = &nb_;
    } else {
      K = kb + DSP_SLOTS;
      I = ib + DSP_SLOTS;
      N = &na_;
    }
    keep_smallest(K, I, *N, S, key, m);
  }
  // occupancy of B before its own turn: everything non-empty (incl. departing / vanishing stays)
  const uint8_t *fl = d.flag + d.slot_base(a, B);
  unsigned occ = 0, leaving = 0;
  for (int p = 0; p < S; ++p) {
    const uint8_t c = fl[p];
    if (c != F_EMPTY) occ |= 1u << p;
    if (c == F_DEPART || c == F_KILLED) leaving |= 1u << p;
  }
  const unsigned all = (1u << S) - 1u;
  for (int i = 0; i < nb_; ++i) {  // arrivals before B's own turn
    const int sl = lowest_free(occ, all);
    if (sl < 0) break;
    occ |= 1u << sl;
    d.c_assign[cb + ib[i]] = sl;
  }
  occ &= ~leaving;  // B's own turn
  for (int i = 0; i < na_; ++i) {  // arrivals after it
    const int sl = lowest_free(occ, all);
    if (sl < 0) break;
    occ |= 1u << sl;
    d.c_assign[cb + ib[DSP_SLOTS + i]] = sl;
  }
}

// ---- update: pyramid lists = first SP placed particles in sweep order, one thread per pyramid -----
__global__ __launch_bounds__(64) void k_dsp_pyramids(DspDev d, int round) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  if (round > 0 && s.changed[round - 1] == 0) return;
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= d.NP) return;
  const int head = d.phead[d.pyr_base(a) + q];
  int      *out  = d.pyr_list + (d.pyr_base(a) + q) * d.SP;
  if (head < 0) {
    d.pyr_n[d.pyr_base(a) + q] = 0;
    return;
  }
  // selection scratch in HBM/L2: SAFE_PARTICLE_NUM_PYRAMID grows with the grid (20 at 66x66x20, 218 at
  // 100^3) while a pyramid rarely holds more than a handful of particles
  int *K = d.pyr_key + (d.pyr_base(a) + q) * d.SP, *I = d.pyr_id + (d.pyr_base(a) + q) * d.SP;
  int  n = 0, placed = 0;
  const int    SP = d.SP;
  const size_t cb = d.cand_base(a);
  for (int m = head; m >= 0; m = d.c_pnext[cb + m]) {
    if (d.c_kill[cb + m] || d.c_assign[cb + m] < 0) continue;
    ++placed;
    keep_smallest(K, I, n, SP, d.c_key[cb + m], m);
  }
  for (int i = 0; i < n; ++i) out[i] = d.c_dest[cb + I[i]] * DSP_SLOTS + d.c_assign[cb + I[i]];
  d.pyr_n[d.pyr_base(a) + q] = n;
  if (placed > SP) {  // the rest found the list full: they vanish (moveParticle -> -2)
    const int last = K[SP - 1];
    int       newly = 0;
    for (int m = head; m >= 0; m = d.c_pnext[cb + m]) {
      if (d.c_kill[cb + m] || d.c_assign[cb + m] < 0) continue;
      if (d.c_key[cb + m] > last) {
        d.c_kill[cb + m] = 1;
        if (d.c_vnext[cb + m] == -2)  // a stay: its slot frees up at its own turn
          d.flag[d.slot_base(a) + d.c_key[cb + m]] = F_KILLED;
        ++newly;
      }
    }
    if (newly) atomicAdd(&s.changed[round], newly);
  }
}

// ---- update: commit ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dsp_commit_slots(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v == 0 && s.changed[DSP_ROUNDS - 1] != 0) s.err_unconverged += 1;
  if (v >= d.V) return;
  const size_t at0 = d.slot_base(a, v);
  const uint4  f4  = *reinterpret_cast<const uint4 *>(d.flag + at0);
  // bytes >= 5 are the transient codes F_DEPART / F_KILLED: (b + 3) & 8 is set exactly for 5, 6 (codes <= 6)
  const unsigned w4[4] = {f4.x, f4.y, f4.z, f4.w};
  unsigned       any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) any |= (w4[k] + 0x03030303u) & 0x08080808u;
  if (!any) return;
#pragma unroll
  for (int p = 0; p < DSP_SLOTS; ++p) {
    const uint8_t c = (uint8_t)((w4[p >> 2] >> ((p & 3) * 8)) & 0xffu);
    if (c == F_DEPART) d.flag[at0 + p] = F_EMPTY;
    if (c == F_KILLED) {
      d.flag[at0 + p] = F_EMPTY;
      atomicAdd(&s.dbg_pyr_full, 1);
    }
  }
}
__global__ __launch_bounds__(256) void k_dsp_commit_movers(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int n = s.cand_cnt < d.cand_cap ? s.cand_cnt : d.cand_cap;
  if (m >= n) return;
  const size_t ci = d.cand_base(a) + m;
  if (d.c_vnext[ci] == -2) return;  // stays live in place
  if (d.c_kill[ci]) {
    atomicAdd(&s.dbg_pyr_full, 1);
    return;
  }
  const int sl = d.c_assign[ci];
  if (sl < 0) {
    atomicAdd(&s.dbg_voxel_full, 1);
    return;
  }
  const size_t at  = d.slot_base(a, d.c_dest[ci]) + sl;
  const float *pay = d.c_pay + ci * 6;
  d.flag[at]       = F_MOVED;
  for (int k = 0; k < 6; ++k) d.f[k][at] = pay[k];
}

// ---- update: mapUpdate (:750-849) --------------------------------------------------------------------
// C_k + kappa per stored observation: neighbour pyramids in table order, list entries in sweep order.
__global__ __launch_bounds__(256) void k_dsp_ck(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= s.n_obs) return;
  const int    e  = d.obs_list[d.point_base(a) + k];
  const int    pi = e / d.OM;
  float       *o  = d.pc + (d.obs_base(a) + e) * 5;
  const float  ox = o[0], oy = o[1], oz = o[2];
  float        ck = 0.f;
  const int   *nb = d.nbr + pi * 10;
  const size_t sb = d.slot_base(a);
  float        sig = d.sigma;
  for (int n = 0; n < nb[0]; ++n) {
    const int  q  = nb[n + 1];
    const int  cn = d.pyr_n[d.pyr_base(a) + q];
    const int *li = d.pyr_list + (d.pyr_base(a) + q) * d.SP;
    for (int i = 0; i < cn; ++i) {
      const size_t at = sb + li[i];
      const float  gk = query_pdf(d.pdf, d.f[2][at], ox, sig) * query_pdf(d.pdf, d.f[3][at], oy, sig) *
                       query_pdf(d.pdf, d.f[4][at], oz, sig);
      ck += d.Pd * d.f[5][at] * gk;
    }
  }
  ck += (s.enb + d.kappa);
  o[3] = ck;
}
// weight update of every particle listed in a pyramid
__global__ __launch_bounds__(256) void k_dsp_weight(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= d.NP * d.SP) return;
  const int i = gid / d.SP, q = gid % d.SP;
  if (q >= d.pyr_n[d.pyr_base(a) + i]) return;
  const size_t at = d.slot_base(a) + d.pyr_list[(d.pyr_base(a) + i) * d.SP + q];
  const float  px = d.f[2][at], py = d.f[3][at], pz = d.f[4][at];
  const float  len = sqrtf(px * px + py * py + pz * pz);
  const int    mb  = d.maxlen[d.pyr_base(a) + i];
  const float  ml  = mb < 0 ? -1.f : __int_as_float(mb);
  if (ml > 0.f && len > ml + d.thick) return;  // occluded
  const int   *nb = d.nbr + i * 10;
  const float *pc = d.pc + d.obs_base(a) * 5;
  float        sum = 0.f, sig = d.sigma;
  for (int n = 0; n < nb[0]; ++n) {
    const int ni = nb[n + 1];
    const int cn = d.nobs[d.pyr_base(a) + ni];
    for (int z = 0; z < cn; ++z) {
      const float *o  = pc + ((size_t)ni * d.OM + z) * 5;
      const float  gk = query_pdf(d.pdf, px, o[0], sig) * query_pdf(d.pdf, py, o[1], sig) *
                       query_pdf(d.pdf, pz, o[2], sig);
      sum += d.Pd * gk / o[3];
    }
  }
  d.f[5][at] *= ((1 - d.Pd) + sum);
}

// ---- update: new-born particles (:852-990) --------------------------------------------------------------
__device__ inline int block_scan_excl(int v, int *s_tmp, int *total) {  // blockDim = 1024
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int       x    = v;
  for (int o = 1; o < 64; o <<= 1) {
    int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_tmp[w] = x;
  __syncthreads();
  if (w == 0) {
    int t = lane < 16 ? s_tmp[lane] : 0;
    for (int o = 1; o < 16; o <<= 1) {
      int y = __shfl_up(t, o);
      if (lane >= o) t += y;
    }
    if (lane < 16) s_tmp[lane] = t;
  }
  __syncthreads();
  const int base = w ? s_tmp[w - 1] : 0;
  if (total) *total = s_tmp[15];
  __syncthreads();
  return base + x - v;
}

__global__ __launch_bounds__(1024) void k_dsp_newborn(DspDev d) {
  extern __shared__ float s_inv[];  // [max_pts] 1/C_k in (pyramid, j) order
  __shared__ int   s_tmp[16];
  __shared__ float s_wnew;
  const int a = blockIdx.x;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int tid = threadIdx.x;
  // normalisation coefficient: sequential fp32 sum in (pyramid, j) order (:854-860)
  {
    const int per = (d.NP + 1023) / 1024;
    int       cnt = 0;
    for (int i = tid * per; i < (tid + 1) * per && i < d.NP; ++i) cnt += d.nobs[d.pyr_base(a) + i];
    int       tot;
    int       off = block_scan_excl(cnt, s_tmp, &tot);
    const float *pc = d.pc + d.obs_base(a) * 5;
    for (int i = tid * per; i < (tid + 1) * per && i < d.NP; ++i) {
      const int c = d.nobs[d.pyr_base(a) + i];
      for (int j = 0; j < c; ++j) s_inv[off++] = 1.f / pc[((size_t)i * d.OM + j) * 5 + 3];
    }
    __syncthreads();
    if (tid == 0) {
      float norm = 0.f;
      for (int i = 0; i < tot; ++i) norm += s_inv[i];
      s_wnew  = d.w_nb * norm;
      s.w_new = s_wnew;
    }
    __syncthreads();
  }
  const int n = s.n_born, nb = d.nb;
  const int min_static = (int)((float)nb * 0.15f), model_gen = (int)((float)nb * 0.8f);
  const float *born = d.born + d.point_base(a) * 7;
  int   *b_valid = d.b_valid + d.point_base(a), *b_nst = d.b_nstatic + d.point_base(a);
  float *b_c = d.b_c + d.point_base(a) * 3;
  const size_t sb = d.slot_base(a);
  // per point: voxel, Dempster-Shafer split (:880-925)
  for (int k = tid; k < n; k += 1024) {
    const float cx = born[k * 7] - s.cur[0], cy = born[k * 7 + 1] - s.cur[1], cz = born[k * 7 + 2] - s.cur[2];
    b_c[k * 3] = cx;
    b_c[k * 3 + 1] = cy;
    b_c[k * 3 + 2] = cz;
    const int vi = voxel_index(d, cx, cy, cz);
    int       ns = 0;
    if (vi >= 0) {
      float ws = 0.f, wd = 0.f, wsd = 0.f;
      for (int kk = 0; kk < d.S; ++kk) {
        const size_t  at = sb + (size_t)vi * DSP_SLOTS + kk;
        const uint8_t c  = d.flag[at];
        if (c == F_VALID || c == F_MOVED) {
          const float va = fabsf(d.f[0][at]) + fabsf(d.f[1][at]) + fabsf(0.f);
          const float w  = d.f[5][at];
          if (va < 0.1f)
            ws += w;
          else if (va < 0.5f)
            wsd += w;
          else
            wd += w;
        }
      }
      const float tot = ws + wd + wsd;
      const float m_s = ws / tot, m_d = wd / tot, m_sd = wsd / tot;
      const float p_s = (m_s + m_s + m_sd) * 0.5f, p_d = (m_d + m_d + m_sd) * 0.5f;
      const float psn = p_s / (p_s + p_d);
      const float fs  = (float)model_gen * psn;
      ns              = (fs == fs) ? (int)fs : min_static;
      ns              = ns > min_static ? ns : min_static;
    }
    b_valid[k] = vi >= 0;
    b_nst[k]   = ns;
  }
  __syncthreads();
  // rank of each valid point (position-noise draws happen only for valid points)
  int n_valid;
  {
    const int per = (n + 1023) / 1024;
    int       cnt = 0;
    for (int k = tid * per; k < (tid + 1) * per && k < n; ++k) cnt += b_valid[k];
    int off = block_scan_excl(cnt, s_tmp, &n_valid);
    for (int k = tid * per; k < (tid + 1) * per && k < n; ++k) {
      const int v = b_valid[k];
      b_valid[k]  = v ? off : -1;  // becomes the rank
      off += v;
    }
  }
  __syncthreads();
  // per particle: position, class; counts of velocity / rand draws
  const int total = n * nb;
  const int per   = (total + 1023) / 1024;
  int8_t   *b_cls = d.b_cls + d.newborn_base(a);
  int      *b_dest = d.b_dest + d.newborn_base(a);
  float    *b_pay  = d.b_pay + d.newborn_base(a) * 5;
  int       cv = 0, cr = 0;
  for (int j = tid * per; j < (tid + 1) * per && j < total; ++j) {
    const int k = j / nb, p = j % nb;
    int8_t    cls = -1;
    const int rk  = b_valid[k];
    if (rk >= 0) {
      long long g0 = (long long)s.pseq + ((long long)rk * nb + p) * 3;
      const float qx = b_c[k * 3] + d.pg[(g0 + 0) % d.n_gauss];
      const float qy = b_c[k * 3 + 1] + d.pg[(g0 + 1) % d.n_gauss];
      const float qz = b_c[k * 3 + 2] + d.pg[(g0 + 2) % d.n_gauss];
      const int   qi = voxel_index(d, qx, qy, qz);
      if (qi >= 0) {
        const float nx = born[k * 7 + 3], inten = born[k * 7 + 6];
        if (p < b_nst[k])
          cls = 0;
        else if (nx > -100.f && p < model_gen)
          cls = inten > 0.01f ? 1 : 0;
        else
          cls = inten > 0.01f ? 2 : 0;
        b_dest[j]        = qi;
        b_pay[j * 5 + 0] = qx;
        b_pay[j * 5 + 1] = qy;
        b_pay[j * 5 + 2] = qz;
      }
    }
    b_cls[j] = cls;
    cv += cls == 1;
    cr += cls == 2;
  }
  int tv, tr;
  int ov = block_scan_excl(cv, s_tmp, &tv);
  int orr = block_scan_excl(cr, s_tmp, &tr);
  for (int j = tid * per; j < (tid + 1) * per && j < total; ++j) {
    const int8_t cls = b_cls[j];
    if (cls < 0) continue;
    const int k = j / nb;
    float     vx = 0.f, vy = 0.f;
    if (cls == 1) {  // estimated velocity + 4 sigma noise (:944-948); the vz draw is consumed
      const long long g = (long long)s.vseq + (long long)ov * 3;
      vx = born[k * 7 + 3] + 4 * d.vg[(g + 0) % d.n_gauss];
      vy = born[k * 7 + 4] + 4 * d.vg[(g + 1) % d.n_gauss];
      ++ov;
    } else if (cls == 2) {  // generateRandomFloat(-1.5, 1.5) x2, (-0.5, 0.5) consumed (:956-958,1682)
      const long long g = (long long)s.rseq + (long long)orr * 3;
      const float den = (float)((float)2147483647 / (1.5f - -1.5f));
      vx = -1.5f + (float)d.rnd[(g + 0) % d.n_rand] / den;
      vy = -1.5f + (float)d.rnd[(g + 1) % d.n_rand] / den;
      ++orr;
    }
    b_pay[j * 5 + 3] = vx;
    b_pay[j * 5 + 4] = vy;
    d.b_vnext[d.newborn_base(a) + j] = atomicExch(&d.vhead[d.voxel_base(a) + b_dest[j]], j);
  }
  __syncthreads();
  if (tid == 0) {
    s.pseq     = (int)(((long long)s.pseq + (long long)n_valid * nb * 3) % d.n_gauss);
    s.vseq     = (int)(((long long)s.vseq + (long long)tv * 3) % d.n_gauss);
    s.rseq     = (int)(((long long)s.rseq + (long long)tr * 3) % d.n_rand);
    s.born_cnt = total;
  }
}

// addAParticle in (point, particle) order (:1271-1290): one thread per destination voxel
__global__ __launch_bounds__(64) void k_dsp_place_born(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int B = blockIdx.x * 64 + threadIdx.x;
  if (B >= d.V) return;
  const int head = d.vhead[d.voxel_base(a) + B];
  if (head < 0) return;
  __shared__ int s_key[64][DSP_SLOTS];
  int *K = s_key[threadIdx.x];
  int  n = 0;
  const int    S = d.S;
  const size_t bb = d.newborn_base(a);
  for (int m = head; m >= 0; m = d.b_vnext[bb + m]) {
    keep_smallest(K, nullptr, n, S, m, m);
  }
  uint8_t *fl  = d.flag + d.slot_base(a, B);
  unsigned occ = 0;
  for (int p = 0; p < S; ++p)
    if (fl[p] != F_EMPTY) occ |= 1u << p;
  const unsigned all = (1u << S) - 1u;
  const float    w   = s.w_new;
  for (int i = 0; i < n; ++i) {
    const int sl = lowest_free(occ, all);
    if (sl < 0) break;
    occ |= 1u << sl;
    const size_t at  = d.slot_base(a, B) + sl;
    const float *pay = d.b_pay + (bb + K[i]) * 5;
    d.flag[at]       = F_NEW;
    d.f[0][at]       = pay[3];
    d.f[1][at]       = pay[4];
    d.f[2][at]       = pay[0];
    d.f[3][at]       = pay[1];
    d.f[4][at]       = pay[2];
    d.f[5][at]       = w;
  }
}

// ---- update: occupancy + resampling, one thread per voxel (:993-1130) -----------------------------------
__global__ __launch_bounds__(256) void k_dsp_occupancy(DspDev d) {
  const int a = blockIdx.y;
  DspAgent &s = d.ag[a];
  if (!s.ok) return;
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= d.V) return;
  const size_t at0 = d.slot_base(a, v);
  float       *occ = d.occ + d.occ_base(a);
  const uint4  f4  = *reinterpret_cast<const uint4 *>(d.flag + at0);
  if ((f4.x | f4.y | f4.z | f4.w) == 0u) {
    occ[v] = occ[d.V + v] = occ[2 * d.V + v] = occ[3 * d.V + v] = 0.f;
    return;
  }
  const int S = d.S;
  float     wsum = 0.f, vxs = 0.f, vys = 0.f, vzs = 0.f;
  int       n = 0, n_old = 0;
  unsigned  valid = 0;
  float    *fut = d.fut + d.fut_base(a);
  for (int p = 0; p < S; ++p) {
    const uint8_t c = d.flag[at0 + p];
    if (c == F_EMPTY) continue;
    const float w = d.f[5][at0 + p];
    if ((double)w < 1e-3) {
      d.flag[at0 + p] = F_EMPTY;
      continue;
    }
    if (c != F_NEW) {
      ++n_old;
      const float vx = d.f[0][at0 + p], vy = d.f[1][at0 + p];
      const float px = d.f[2][at0 + p], py = d.f[3][at0 + p], pz = d.f[4][at0 + p];
      vxs += vx;
      vys += vy;
      vzs += 0.f;
      for (int t = 0; t < d.T; ++t) {
        const float pt = d.pred_t[t];
        const int   pi = voxel_index(d, px + vx * pt, py + vy * pt, pz + 0.f * pt);
        if (pi >= 0) atomicAdd(&fut[(size_t)t * d.V + pi], w);
      }
    }
    d.flag[at0 + p] = F_VALID;
    valid |= 1u << p;
    ++n;
    wsum += w;
  }
  occ[v] = wsum;
  if (n_old > 0) {
    occ[d.V + v]     = vxs / (float)n_old;
    occ[2 * d.V + v] = vys / (float)n_old;
    occ[3 * d.V + v] = vzs / (float)n_old;
  } else {
    occ[d.V + v] = occ[2 * d.V + v] = occ[3 * d.V + v] = 0.f;
  }
  if (n < 5) return;
  const int   n_after = n > d.maxp ? d.maxp : n;
  const float w_after = wsum / (float)n_after;
  float       acc_ori = 0.f, acc_new = w_after * 0.5f;
  unsigned    used = valid;  // non-empty slots (copies included)
  for (int p = 0; p < S; ++p) {
    if (!((valid >> p) & 1u)) continue;
    float w = d.f[5][at0 + p];
    acc_ori += w;
    if (acc_ori > acc_new) {
      w = w_after;
      acc_new += w_after;
      int full = 0, p_i = 0;
      while (acc_ori > acc_new) {
        int found = 0;
        if (!full) {
          for (; p_i < S; ++p_i) {
            if (!((used >> p_i) & 1u)) {
              d.flag[at0 + p_i] = F_RESAMP;
              for (int k = 0; k < 5; ++k) d.f[k][at0 + p_i] = d.f[k][at0 + p];
              d.f[5][at0 + p_i] = w;
              used |= 1u << p_i;
              found = 1;
              break;
            }
          }
        }
        if (!found) {
          w += w_after;
          full = 1;
        }
        acc_new += w_after;
      }
      d.f[5][at0 + p] = w;
    } else {
      d.flag[at0 + p] = F_EMPTY;
      used &= ~(1u << p);
    }
  }
}

// ---- publish (:445-469 + risk_voxel.cpp:141-153) ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_dsp_publish(DspDev d, void *__restrict__ grid, GridGeom gg, float thr,
                                                     float *__restrict__ poses, double *__restrict__ stamps) {
  const int half = gg.half;
  const int a = blockIdx.y;
  const int v = blockIdx.x * 256 + threadIdx.x;
  DspAgent &s = d.ag[a];
  if (v == 0) {
    poses[a * 3]     = s.cur[0];
    poses[a * 3 + 1] = s.cur[1];
    poses[a * 3 + 2] = s.cur[2];
    stamps[a]        = s.last_t;
  }
  if (v >= d.V) return;
  float *fut = d.fut + d.fut_base(a);
  char  *g   = reinterpret_cast<char *>(grid) + d.fut_base(a) * (half ? 2 : 4);
  const int pv = gg.phys_of(v);  // (rows: v itself, the straight copy; tiles: the cell's place in the slice)
  for (int t = 0; t < d.T; ++t) {
    cell_st(g, (size_t)t * d.V + pv, fut[(size_t)t * d.V + v], half);
    fut[(size_t)t * d.V + v] = 0.f;
  }
  if (d.occ[d.occ_base(a) + v] > thr) atomicAdd(&s.n_occupied, 1);
}
__global__ void k_dsp_publish_ego(DspDev d, void *__restrict__ grid, GridGeom gg, int inf_step,
                                  int32_t *__restrict__ out_n) {
  const int half = gg.half;
  const int a = blockIdx.x;
  const int w = 2 * inf_step + 1;
  char     *g = reinterpret_cast<char *>(grid) + d.fut_base(a) * (half ? 2 : 4);
  for (int k = threadIdx.x; k < w * w * w; k += blockDim.x) {
    const int x = k / (w * w) - inf_step, y = (k / w) % w - inf_step, z = k % w - inf_step;
    const int idx = z * d.L * d.W + y * d.L + x;  // getVoxelIndex(Vector3i) of the OFFSET (map.h:176)
    if (idx < 0 || idx >= d.V) continue;          // negative index = UB in the reference: skipped
    for (int t = 0; t < 3 && t < d.T; ++t) cell_st(g, (size_t)t * d.V + gg.phys_of(idx), 0.f, half);
  }
  if (threadIdx.x == 0) {
    if (out_n) out_n[a] = d.ag[a].n_occupied;
    d.ag[a].n_occupied = 0;
  }
}

}  // namespace sogm

using namespace sogm;

// k_dsp_observe keeps per-pyramid counters, k_dsp_newborn the 1/C_k list in dynamic LDS
static size_t observe_lds(const DspDev &d) { return 2 * (size_t)d.NP * sizeof(int); }
static size_t newborn_lds(const DspDev &d) { return (size_t)d.max_pts * sizeof(float); }
void sogm::reserve_update_lds(const DspDev &d) {
  (void)raise_dynamic_lds<k_dsp_observe>(observe_lds(d));
  (void)raise_dynamic_lds<k_dsp_newborn>(newborn_lds(d));
}

namespace {
// launch grids of one update: (x, agent) with one thread per x, or one workgroup per agent
struct UpdateGrids {
  unsigned A;
  explicit UpdateGrids(const DspDev &d) : A((unsigned)d.A) {}
  dim3 per(size_t n, unsigned block) const { return dim3((unsigned)((n + block - 1) / block), A); }
  dim3 agents() const { return dim3(A); }
};
}  // namespace

extern "C" {

int sogm_update_dsp(sogm_dsp *h, const float *points, const float *labels, const int32_t *cloud_range,
                    const float *sensor_pos, const float *sensor_quat, const double *stamps,
                    int32_t *out_ok, void *stream) {
  if (!h || !points || !cloud_range || !sensor_pos || !sensor_quat || !stamps) return SOGM_ERR_INVALID_ARG;
  DspDev     &d  = h->d;
  hipStream_t st = (hipStream_t)stream;
  SOGM_HIP_CHECK(hipSetDevice(h->map->device));
  const UpdateGrids g(d);
  const size_t      A = d.A, V = d.V;
  // odometry, observations, the new-born list
  hipLaunchKernelGGL(k_dsp_begin, g.agents(), dim3(128), 0, st, d, sensor_pos, sensor_quat, stamps, out_ok);
  SOGM_HIP_CHECK(hipMemsetAsync(d.vhead, 0xFF, A * V * sizeof(int), st));
  SOGM_HIP_CHECK(hipMemsetAsync(d.phead, 0xFF, A * d.NP * sizeof(int), st));
  hipLaunchKernelGGL(k_dsp_observe, g.agents(), dim3(256), observe_lds(d), st, d, points, labels, cloud_range);
  if (!labels)  // velocityEstimationThread (:305): labels and point order of the new-born list are computed here
    if (int rc = launch_dsp_velocity(d, cloud_range, 0.15f, st)) return rc;
  // prediction: move, then the ordered first-fit to its fixed point, then commit
  hipLaunchKernelGGL(k_dsp_predict, g.per(V, 256), dim3(256), 0, st, d);
  for (int r = 0; r < DSP_ROUNDS; ++r) {
    hipLaunchKernelGGL(k_dsp_place, g.per(V, 64), dim3(64), 0, st, d, r);
    hipLaunchKernelGGL(k_dsp_pyramids, g.per(d.NP, 64), dim3(64), 0, st, d, r);
  }
  hipLaunchKernelGGL(k_dsp_commit_slots, g.per(V, 256), dim3(256), 0, st, d);
  hipLaunchKernelGGL(k_dsp_commit_movers, g.per(d.cand_cap, 256), dim3(256), 0, st, d);
  // weights
  hipLaunchKernelGGL(k_dsp_ck, g.per(d.max_pts, 256), dim3(256), 0, st, d);
  hipLaunchKernelGGL(k_dsp_weight, g.per(d.NP * d.SP, 256), dim3(256), 0, st, d);
  // new-born particles, occupancy and resampling
  SOGM_HIP_CHECK(hipMemsetAsync(d.vhead, 0xFF, A * V * sizeof(int), st));
  hipLaunchKernelGGL(k_dsp_newborn, g.agents(), dim3(1024), newborn_lds(d), st, d);
  hipLaunchKernelGGL(k_dsp_place_born, g.per(V, 64), dim3(64), 0, st, d);
  hipLaunchKernelGGL(k_dsp_occupancy, g.per(V, 256), dim3(256), 0, st, d);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int sogm_dsp_publish(sogm_dsp *h, int32_t *out_n_occupied, void *stream) {
  if (!h) return SOGM_ERR_INVALID_ARG;
  DspDev     &d  = h->d;
  sogm_ctx   *c  = h->map;
  hipStream_t st = (hipStream_t)stream;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (int rc = sogm::join_update(c, st)) return rc;
  if (c->pool.precleared()) {  // a pending side-stream clear must not race the copy
    int rc = sogm::adopt_preclear(c, st);
    if (rc) return rc;
  }
  c->pool.dense_write_current();  // every cell is written: the next reset of this grid is the dense clear
  hipLaunchKernelGGL(k_dsp_publish, dim3((unsigned)((d.V + 255) / 256), (unsigned)d.A), dim3(256), 0, st, d,
                     (void *)c->d_grid, c->geom, c->geom.risk_threshold, c->d_poses, c->d_stamps);
  hipLaunchKernelGGL(k_dsp_publish_ego, dim3((unsigned)d.A), dim3(128), 0, st, d, (void *)c->d_grid, c->geom, c->geom.inf_step,
                     out_n_occupied);
  SOGM_HIP_CHECK(hipGetLastError());
  c->updated = 1;
  return SOGM_OK;
}

}  // extern "C"
