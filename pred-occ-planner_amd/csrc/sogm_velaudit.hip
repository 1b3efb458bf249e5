// Velocity audit (include/sogm_abi.h "velocity audit"; the rules: sogm_velaudit.hpp): the new-born list of a particle map's
// last update — input_cloud_with_velocity, what velocityEstimationThread or the caller's labels made of the cloud — scored
// point by point against truth labels in the order of the INPUT cloud, through the list's source index (born_src).
// Two launches, stream-ordered:
//   k_vel_audit_zero   one lane per int64: out_rows and out_per_code zeroed (not with SOGM_VELAUDIT_ACCUMULATE)
//   k_vel_audit        one 256-lane workgroup per agent.
//     pass 0  born_src[k] marked in an LDS bitmap of max_points bits (atomicOr).  An index outside [0, n_in) or a bit that
//             was already set is BAD_SOURCE; a point named twice is also marked in a second bitmap.
//     pass 1  over the born rows: velaudit_score against the truth label of point born_src[k].  A row whose point is in the
//             second bitmap looks for a smaller k with the same index (the error path: the smallest k counts, whatever the
//             order the lanes ran in).
//     pass 2  over the input points whose bit is clear: DROPPED.
//     Every field of the row is a predicate: one __ballot and __popcll per field and trip, summed in uniform registers per
//     wave; sum_e2_um is a 64-bit sum per lane, reduced across the wave by shuffles.  Then one 64-bit integer LDS add per
//     wave and field, then one plain 8-byte store per field by one lane (one integer add with ACCUMULATE: the workgroup owns
//     the agent's row).  The per-code table lives in dynamic LDS (64-bit integer atomics; the ground's row — thousands of
//     consecutive points share it — is summed across the wave by ballots first); its non-zero entries are added to the output.
// All LDS is dynamic and carved in multiples of 16 bytes (the 64-bit atomics need their 8-byte alignment).  Integer adds only:
// nothing depends on the order lanes, waves or workgroups run in.
#include "sogm_device.hpp"
#include "sogm_velaudit.hpp"

#include <cmath>
#include <cstdio>

namespace sogm {
namespace {

constexpr int VA_WG         = 256;
constexpr int VA_MAX_POINTS = 8192;                // sogm_dsp_create's limit
constexpr int VA_WORDS      = VA_MAX_POINTS / 32;  // one bitmap
constexpr int VA_MAX_CODE_ROWS = 1024;
// dynamic LDS: [row: 32 x u64][seen: VA_WORDS x u32][dup: VA_WORDS x u32][flags: 4 x u32][table: code_rows x 6 x u64]
constexpr int VA_OFF_SEEN  = VELROW_N * 8;
constexpr int VA_OFF_DUP   = VA_OFF_SEEN + VA_WORDS * 4;
constexpr int VA_OFF_FLAGS = VA_OFF_DUP + VA_WORDS * 4;
constexpr int VA_OFF_TABLE = VA_OFF_FLAGS + 16;
static_assert(VA_OFF_TABLE % 16 == 0, "the table's 64-bit atomics start 16-byte aligned");

struct VelAuditArgs {
  const float   *born;      // [A][max_pts][7]
  const int32_t *born_src;  // [A][max_pts]
  const int32_t *ok, *n_born;  // the agents' scalars, `stride` ints apart
  int            stride;
  int            max_pts, n_codes, accumulate;
  float          tol;
};

__global__ __launch_bounds__(64) void k_vel_audit_zero(long long *__restrict__ rows, long long n_rows,
                                                       long long *__restrict__ per_code, long long n_per_code) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i < n_rows) rows[i] = 0;
  if (per_code && i < n_per_code) per_code[i] = 0;
}

__device__ inline long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(VA_WG) void k_vel_audit(VelAuditArgs p, const float *__restrict__ truth,
                                                     const int32_t *__restrict__ code, const int32_t *__restrict__ range,
                                                     long long *__restrict__ out_rows, long long *__restrict__ out_per_code) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_va[];
  unsigned long long *s_row   = reinterpret_cast<unsigned long long *>(s_va);
  unsigned           *s_seen  = reinterpret_cast<unsigned *>(s_va + VA_OFF_SEEN);
  unsigned           *s_dup   = reinterpret_cast<unsigned *>(s_va + VA_OFF_DUP);
  unsigned           *s_flags = reinterpret_cast<unsigned *>(s_va + VA_OFF_FLAGS);  // [0]: status bits, [1]: a point named twice
  unsigned long long *s_tab   = reinterpret_cast<unsigned long long *>(s_va + VA_OFF_TABLE);
  const int a = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const bool per_code = out_per_code != nullptr;
  const int  code_rows = p.n_codes + 2;
  long long *row_out = out_rows + (size_t)a * VELROW_N;
  long long *tab_out = per_code ? out_per_code + (size_t)a * code_rows * VELCODE_COLS : nullptr;

  const int       begin = range[a * 2];
  const long long len   = (long long)range[a * 2 + 1] - (long long)begin;
  const int       n_in  = (int)(len < (long long)p.max_pts ? len : (long long)p.max_pts);
  if (!p.ok[(size_t)a * p.stride] || n_in <= 0) {  // (uniform) rejected, never run, or an empty cloud: zeros
    if (tid == 0) row_out[VELROW_STATUS] = (p.accumulate ? row_out[VELROW_STATUS] : 0) | VELAUDIT_SKIPPED;
    return;
  }
  int n_born = p.n_born[(size_t)a * p.stride];
  n_born     = n_born < 0 ? 0 : (n_born > p.max_pts ? p.max_pts : n_born);

  for (int i = tid; i < VELROW_N; i += VA_WG) s_row[i] = 0;
  for (int i = tid; i < VA_WORDS; i += VA_WG) {
    s_seen[i] = 0;
    s_dup[i]  = 0;
  }
  if (tid < 4) s_flags[tid] = 0;
  if (per_code)
    for (int i = tid; i < code_rows * VELCODE_COLS; i += VA_WG) s_tab[i] = 0;
  __syncthreads();

  const float   *born = p.born + (size_t)a * p.max_pts * 7;
  const int32_t *src  = p.born_src + (size_t)a * p.max_pts;
  const float   *tl   = truth + (size_t)begin * 4;
  const int32_t *tc   = per_code ? code + begin : nullptr;

  // ---- pass 0: which input point every born row names
  for (int k = tid; k < n_born; k += VA_WG) {
    const int i = src[k];
    if (i < 0 || i >= n_in) {
      s_flags[0] = VELAUDIT_BAD_SOURCE;
    } else if (atomicOr(&s_seen[i >> 5], 1u << (i & 31)) & (1u << (i & 31))) {
      atomicOr(&s_dup[i >> 5], 1u << (i & 31));
      s_flags[0] = VELAUDIT_BAD_SOURCE;
      s_flags[1] = 1;
    }
  }
  __syncthreads();
  const bool any_dup = s_flags[1] != 0;

  int       cnt[VELROW_N];  // uniform over the wave: sums of popcounts of ballots; field f of the row (3 .. 28, 30)
  long long sum_um = 0;     // per lane
#pragma unroll
  for (int f = 0; f < VELROW_N; ++f) cnt[f] = 0;
  const int ground_row = p.n_codes;

  // ---- pass 1 (born rows, est from the row) and pass 2 (unnamed input points, DROPPED): one loop body, two ranges
#pragma unroll 1
  for (int pass = 1; pass <= 2; ++pass) {
    const int n = pass == 1 ? n_born : n_in;
    for (int base = 0; base < n; base += VA_WG) {  // (uniform trip count: the ballots below see whole waves)
      const int k = base + tid;
      unsigned  bits = 0;  // bit f: this lane's point counts in field f of the row
      VelScore  s{};
      int       crow = -1;
      if (k < n) {
        int  i    = k;
        bool live = true;
        if (pass == 1) {
          i    = src[k];
          live = i >= 0 && i < n_in;
          if (live && any_dup && ((s_dup[i >> 5] >> (i & 31)) & 1u))
            for (int j = 0; j < k && live; ++j) live = src[j] != i;  // the smallest k that names the point counts
        } else {
          live = !((s_seen[i >> 5] >> (i & 31)) & 1u);
        }
        if (live) {
          const float *t = tl + (size_t)i * 4;
          const float  t4[4] = {t[0], t[1], t[2], t[3]};
          if (pass == 1) {
            const float *r = born + (size_t)k * 7;
            const float  e4[4] = {r[3], r[4], r[5], r[6]};
            s = velaudit_score(e4, t4, p.tol);
          } else {
            s.est   = VEL_EST_DROPPED;
            s.truth = velaudit_truth(t4[3]);
          }
          bits = 1u << (VELROW_CONFUSION + s.truth * 4 + s.est);
          if (s.nan) bits |= 1u << VELROW_N_NAN;
          if (s.scored) {
            if (s.truth == VEL_TRUTH_MOVING) {
              bits |= 1u << (VELROW_SPEED_MOVING + s.speed_bin) | 1u << (VELROW_DIRECTION + s.dir_bin);
              if (s.within) bits |= 1u << VELROW_N_WITHIN;
              sum_um += s.e2_um;
            } else {
              bits |= 1u << (VELROW_SPEED_STILL + s.speed_bin);
            }
          }
          if (per_code) crow = velaudit_code_row(tc[i], p.n_codes);
        }
      }
#pragma unroll
      for (int f = VELROW_N_NAN; f <= VELROW_N_WITHIN; ++f)
        if (f != VELROW_SUM_E2_UM) cnt[f] += __popcll(__ballot((bits >> f) & 1u));
      if (per_code) {
        // the ground's row: one LDS add per class and wave
        const bool g = crow == ground_row;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = __popcll(__ballot(g && s.est == e));
          if (lane == 0 && c) atomicAdd(&s_tab[ground_row * VELCODE_COLS + e], (unsigned long long)c);
        }
        if (crow >= 0 && !g) atomicAdd(&s_tab[crow * VELCODE_COLS + s.est], 1ull);
        if (crow >= 0 && s.scored) {  // (a scored ground point is rare: the estimator labels the ground static)
          if (s.within) atomicAdd(&s_tab[crow * VELCODE_COLS + 4], 1ull);
          if (s.e2_um) atomicAdd(&s_tab[crow * VELCODE_COLS + 5], (unsigned long long)s.e2_um);
        }
      }
    }
  }
  sum_um = wave_sum(sum_um);
  if (lane == 0) {
#pragma unroll
    for (int f = VELROW_N_NAN; f <= VELROW_N_WITHIN; ++f)
      if (f != VELROW_SUM_E2_UM && cnt[f]) atomicAdd(&s_row[f], (unsigned long long)cnt[f]);
    if (sum_um) atomicAdd(&s_row[VELROW_SUM_E2_UM], (unsigned long long)sum_um);
  }
  __syncthreads();
  if (tid < VELROW_N) {
    long long v = (long long)s_row[tid];
    if (tid == VELROW_N_IN) v = n_in;
    if (tid == VELROW_N_BORN) v = n_born;
    if (tid == VELROW_STATUS) {
      v = (long long)s_flags[0] | (len > (long long)p.max_pts ? VELAUDIT_CLIPPED : 0);
      row_out[tid] = p.accumulate ? (row_out[tid] | v) : v;
    } else {
      row_out[tid] = p.accumulate ? row_out[tid] + v : v;
    }
  }
  if (per_code)
    for (int i = tid; i < code_rows * VELCODE_COLS; i += VA_WG)
      if (s_tab[i]) tab_out[i] += (long long)s_tab[i];  // (zeroed by k_vel_audit_zero without ACCUMULATE)
}

int velaudit_refuse(const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "sogm_dsp_velocity_audit: %s", what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_dsp_velocity_audit(sogm_dsp *d, const float *truth_labels, const int32_t *truth_code,
                                       const int32_t *cloud_range, const SogmVelAuditParams *prm, int64_t *out_rows,
                                       int64_t *out_per_code, void *stream) {
  using namespace sogm;
  if (!d || !truth_labels || !cloud_range || !prm || !out_rows) return velaudit_refuse("null pointer");
  if (out_per_code && !truth_code) return velaudit_refuse("out_per_code needs truth_code");
  if (prm->n_codes < 0) return velaudit_refuse("n_codes must be >= 0");
  if (prm->n_codes + 2 > VA_MAX_CODE_ROWS) return velaudit_refuse("n_codes + 2 must be <= 1024 (the per-code table lives in LDS)");
  if (!std::isfinite(prm->speed_tolerance) || prm->speed_tolerance < 0.f)
    return velaudit_refuse("speed_tolerance must be finite and >= 0");
  if (prm->flags & ~SOGM_VELAUDIT_ACCUMULATE) return velaudit_refuse("flags has a bit that is not defined");
  {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
      set_error_text("sogm_dsp_velocity_audit: no HIP device");
      return SOGM_ERR_NO_DEVICE;
    }
  }
  DspBornView v;
  if (dsp_born_view(d, &v) != SOGM_OK || v.max_pts > VA_MAX_POINTS) return velaudit_refuse("not a particle map handle");
  SOGM_HIP_CHECK(hipSetDevice(v.device));
  hipStream_t  st = (hipStream_t)stream;
  VelAuditArgs p{};
  p.born = v.born, p.born_src = v.born_src, p.ok = v.ok, p.n_born = v.n_born, p.stride = v.stride;
  p.max_pts = v.max_pts, p.n_codes = prm->n_codes, p.accumulate = (prm->flags & SOGM_VELAUDIT_ACCUMULATE) ? 1 : 0;
  p.tol = prm->speed_tolerance;
  const long long n_rows = (long long)v.n_agents * VELROW_N;
  const long long n_tab  = out_per_code ? (long long)v.n_agents * (prm->n_codes + 2) * VELCODE_COLS : 0;
  if (!p.accumulate) {
    const long long n = n_rows > n_tab ? n_rows : n_tab;
    hipLaunchKernelGGL(k_vel_audit_zero, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (long long *)out_rows, n_rows,
                       (long long *)out_per_code, n_tab);
  }
  const size_t lds = (size_t)VA_OFF_TABLE + (out_per_code ? (size_t)(prm->n_codes + 2) * VELCODE_COLS * 8 : 0);
  hipLaunchKernelGGL(k_vel_audit, dim3((unsigned)v.n_agents), dim3(VA_WG), lds, st, p, truth_labels,
                     out_per_code ? truth_code : nullptr, cloud_range, (long long *)out_rows, (long long *)out_per_code);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
