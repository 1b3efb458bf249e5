// sogm_context.hip — the library's root behind include/sogm_abi.h: the thread's error text, the ABI version, a context's
// life (sogm_create / sogm_destroy, its grid's size and pointer), the tuning table, the resample table and the body
// particles, the profiling rings' readers, the device clock, and two diagnostics (sogm_debug_div_check,
// sogm_debug_copy_grid).  Host code, except the one-line kernels of the clock and of the division check.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "sogm_device.hpp"

namespace sogm {

static thread_local char g_err[512] = {0};
void set_error(const char *what, hipError_t e) {
  std::snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
}
void set_error_text(const char *text) { std::snprintf(g_err, sizeof(g_err), "%s", text); }

}  // namespace sogm

using namespace sogm;

// every float whose bit pattern lies in [bits_lo, bits_hi) and its negative: GridGeom::div_res against the IEEE division
__global__ __launch_bounds__(256) void k_div_check(sogm::GridGeom g, unsigned bits_lo, unsigned bits_hi, unsigned long long *out) {
  const unsigned long long n    = (unsigned long long)(bits_hi - bits_lo);
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  unsigned                 bad = 0, first = 0xFFFFFFFFu;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const unsigned b = bits_lo + (unsigned)i;
    const float    a = __uint_as_float(b);
    const float    q = g.div_res(a), t = a / g.res, qn = g.div_res(-a), tn = (-a) / g.res;
    if (__float_as_uint(q) != __float_as_uint(t) || __float_as_uint(qn) != __float_as_uint(tn)) {
      ++bad;
      if (b < first) first = b;
    }
  }
  if (bad) {
    atomicAdd(out, (unsigned long long)bad);
    atomicMin(out + 1, (unsigned long long)first);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out[2] = (unsigned long long)g.fast_div;
}
// sogm_device_clock: the 100 MHz wall clock, read on the device
__global__ void k_device_clock(long long *out) { *out = wall_clock64(); }

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int sogm_abi_version(void) { return SOGM_ABI_VERSION; }
const char *sogm_last_error(void) { return sogm::g_err; }

int sogm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sogm_create(const SogmSpec *spec, int n_agents, int device, sogm_ctx **out) {
  if (!spec || !out || n_agents <= 0) return SOGM_ERR_INVALID_ARG;
  if (spec->L <= 0 || spec->W <= 0 || spec->H <= 0 || spec->T <= 0 || spec->T > 32 ||
      !(spec->resolution > 0.f) || !(spec->time_resolution > 0.f))
    return SOGM_ERR_INVALID_ARG;
  if (spec->map_kind != SOGM_MAP_FAKE && spec->map_kind != SOGM_MAP_RISKBASE &&
      spec->map_kind != SOGM_MAP_RISKVOXEL)
    return SOGM_ERR_INVALID_ARG;
  if ((spec->storage & ~(1 | SOGM_LAYOUT_TILED)) != 0) return SOGM_ERR_INVALID_ARG;
  if ((spec->storage & SOGM_LAYOUT_TILED) && ((spec->L | spec->W | spec->H) & 1)) return SOGM_ERR_INVALID_ARG;  // whole tiles
  // one time slice is addressed with 32-bit byte offsets (window_sum_hits) and V is an int
  if ((unsigned long long)spec->L * spec->W * spec->H >= (1ull << 30)) {
    sogm::set_error_text("sogm_create: L * W * H must stay below 2^30 cells per time slice");
    return SOGM_ERR_INVALID_ARG;
  }
  *out = nullptr;
  if (sogm_device_count() <= device || device < 0) {
    std::snprintf(sogm::g_err, sizeof(sogm::g_err), "no HIP device %d", device);
    return SOGM_ERR_NO_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) return SOGM_ERR_NO_DEVICE;
  sogm_ctx *c = new (std::nothrow) sogm_ctx();  // (value-initialised: every field is zero)
  if (!c) return SOGM_ERR_INVALID_ARG;
  c->spec          = *spec;
  c->geom          = make_geom(*spec);
  c->n_agents      = n_agents;
  c->device        = device;
  {
#define X(id, name, dflt, lo, hi) c->tune[SOGM_TUNE_##id] = (double)(dflt);
    SOGM_TUNING_TABLE(X)
#undef X
    const char *e = getenv("SOGM_SPARSE_RESET");  // (one of the library's three environment switches)
    c->sparse     = e ? atoi(e) != 0 : 1;
    // default capacity per agent: one entry per 80 cells, at least 2^20 (the bench scenes log ~0.3 M entries per
    // agent and tick at 200^3 x 20); sogm_set_sparse_reset changes it
    const long long dflt = (long long)spec->L * spec->W * spec->H * spec->T / 80;
    c->log_cap    = (int)(dflt < (1 << 20) ? (1 << 20) : (dflt > (1 << 26) ? (1 << 26) : dflt));
  }
  const size_t n   = (size_t)n_agents * spec->T * (size_t)c->geom.V;
  hipError_t   e   = c->res.device(&c->pool.slot[0].grid, (n * c->cell_bytes() + 15) & ~(size_t)15);
  sogm::sync_grid(c);
  if (e == hipSuccess) e = c->res.device(&c->d_poses, sizeof(float) * 3 * n_agents, true);
  if (e == hipSuccess) e = c->res.device(&c->d_stamps, sizeof(double) * n_agents, true);
  if (e == hipSuccess) e = c->res.device(&c->d_scratch_vt, sizeof(float) * (size_t)c->geom.V * spec->T);
  if (e == hipSuccess) e = c->res.device(&c->clear_cursor, 2 * sizeof(unsigned long long), true);
  // (side2 and pstream are created by the first launch that uses them — a dense clear's wide part, a pre-stamp with a
  // stream of its own: every stream takes a place in the runtime's pool of hardware queues)
  if (e == hipSuccess) e = c->res.stream(&c->side);
  if (e == hipSuccess) e = c->res.event(&c->ev_side2_go);
  if (e == hipSuccess) e = c->res.event(&c->ev_side2_done);
  if (e == hipSuccess) e = c->res.event(&c->ev_grid_free);
  if (e == hipSuccess) e = c->res.event(&c->ev_cleared);
  if (e == hipSuccess) e = c->res.event(&c->ev_gate_open);
  if (e == hipSuccess) e = c->res.event(&c->ev_gate_frac);
  // the memsets above are null-stream operations, which the non-blocking streams every later call uses do not wait for
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) {
    sogm::set_error("sogm_create", e);
    sogm_destroy(c);
    return SOGM_ERR_HIP;
  }
  *out = c;
  return SOGM_OK;
}

void sogm_destroy(sogm_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->res.release_all();
  delete c;
}

int64_t sogm_grid_bytes(const sogm_ctx *c) {
  return c ? (int64_t)c->n_agents * c->spec.T * (int64_t)c->geom.V * (int64_t)c->cell_bytes() : 0;
}
float *sogm_grid_ptr(sogm_ctx *c) {
  if (!c) return nullptr;
  if (c->update_pending) {  // an update flow still building this grid: the pointer is handed out complete
    (void)hipStreamSynchronize(c->ustream);
    c->update_pending = 0;
  }
  c->pool.dense_write_current();  // the caller may write cells the mark log does not see
  return c->d_grid;
}

static const char *const k_tune_names[SOGM_TUNE_N] = {
#define X(id, name, dflt, lo, hi) name,
    SOGM_TUNING_TABLE(X)
#undef X
};
static const double k_tune_range[SOGM_TUNE_N][2] = {
#define X(id, name, dflt, lo, hi) {(double)(lo), (double)(hi)},
    SOGM_TUNING_TABLE(X)
#undef X
};
static int tune_index(const char *key) {
  if (!key) return -1;
  for (int i = 0; i < SOGM_TUNE_N; ++i)
    if (std::strcmp(key, k_tune_names[i]) == 0) return i;
  return -1;
}
int sogm_set_tuning(sogm_ctx *c, const char *key, double value) {
  const int i = tune_index(key);
  if (!c) return SOGM_ERR_INVALID_ARG;
  if (i < 0) {
    char buf[160];
    std::snprintf(buf, sizeof(buf), "sogm_set_tuning: unknown key '%s'", key ? key : "(null)");
    sogm::set_error_text(buf);
    return SOGM_ERR_INVALID_ARG;
  }
  // the values end up as launch dimensions and ticket counts: NaN, infinities and anything outside the key's range
  // (SOGM_TUNING_TABLE) are refused here rather than cast to int later
  if (!(value >= k_tune_range[i][0] && value <= k_tune_range[i][1])) {
    char buf[200];
    std::snprintf(buf, sizeof(buf), "sogm_set_tuning: '%s' = %g is outside [%g, %g]", key, value, k_tune_range[i][0],
                  k_tune_range[i][1]);
    sogm::set_error_text(buf);
    return SOGM_ERR_INVALID_ARG;
  }
  c->tune[i] = value;
  return SOGM_OK;
}
int sogm_get_tuning(const sogm_ctx *c, const char *key, double *out) {
  const int i = tune_index(key);
  if (!c || !out || i < 0) return SOGM_ERR_INVALID_ARG;
  *out = c->tune[i];
  return SOGM_OK;
}
const char *sogm_tuning_key(int index) { return index >= 0 && index < SOGM_TUNE_N ? k_tune_names[index] : nullptr; }

int sogm_set_resample(sogm_ctx *c, float replan_risk_rate, int num_resample, const float *normal_table_dev, int n_table) {
  if (!c || !(replan_risk_rate >= 0.0f) || num_resample < 0 || n_table < 0) return SOGM_ERR_INVALID_ARG;
  const bool on = replan_risk_rate > 0.0f && num_resample > 0;
  if (on) {
    if (!normal_table_dev || c->n_body <= 0 || n_table < 3 * c->n_body * num_resample) {
      sogm::set_error_text("sogm_set_resample: the table must hold 3 * body particles * num_resample standard normals "
                           "(call sogm_set_body_particles first)");
      return SOGM_ERR_INVALID_ARG;
    }
    if (c->geom.half) {
      sogm::set_error_text("sogm_set_resample: fractional weights need SOGM_STORE_F32 cells");
      return SOGM_ERR_INVALID_ARG;
    }
  }
  c->geom.rs_rate = on ? replan_risk_rate : 0.0f;
  c->geom.rs_n    = on ? num_resample : 0;
  c->geom.rs_z    = on ? normal_table_dev : nullptr;
  c->geom.rs_nz   = on ? n_table : 0;
  return SOGM_OK;
}

int sogm_set_body_particles(sogm_ctx *c, const double *xyz, int n) {
  if (!c || !xyz || n <= 0) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  c->res.release(&c->d_body);
  SOGM_HIP_CHECK(c->res.device(&c->d_body, sizeof(double) * 3 * n));
  SOGM_HIP_CHECK(hipMemcpy(c->d_body, xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice));
  c->n_body = n;
  for (int k = 0; k < 3; ++k) {
    double m = 0.0;
    for (int e = 0; e < n; ++e) m = std::fabs(xyz[e * 3 + k]) > m ? std::fabs(xyz[e * 3 + k]) : m;
    c->geom.body_ext[k] = (float)m;
  }
  return SOGM_OK;
}

int sogm_set_profiling(sogm_ctx *c, int enable) {
  return sogm_set_profiling_slots(c, enable ? (1 << SOGM_PROF_N) - 1 : 0);
}

int sogm_set_profiling_slots(sogm_ctx *c, int slot_mask) {
  if (!c || slot_mask < 0 || slot_mask >= (1 << SOGM_PROF_N)) return SOGM_ERR_INVALID_ARG;
  c->profiling = slot_mask;
  for (int k = 0; k < SOGM_PROF_N; ++k) c->ring_n[k] = 0;
  return SOGM_OK;
}

int sogm_profile_read(sogm_ctx *c, double *out_ms) {
  if (!c || !out_ms) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  for (int k = 0; k < SOGM_PROF_N; ++k) {
    out_ms[k] = -1.0;
    if (c->ring_n[k] <= 0 || c->ring[k].empty()) continue;
    hipEvent_t *p  = c->ring[k].data() + 2 * ((c->ring_n[k] - 1) % SOGM_PROF_RING);
    float       ms = 0.f;
    if (hipEventElapsedTime(&ms, p[0], p[1]) == hipSuccess) out_ms[k] = (double)ms;
  }
  return SOGM_OK;
}

int sogm_profile_read_all(sogm_ctx *c, int slot, double *out_ms, int cap, int *out_n) {
  if (!c || !out_ms || !out_n || slot < 0 || slot >= SOGM_PROF_N || cap < 0) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  long long n = c->ring_n[slot];
  if (n > SOGM_PROF_RING) n = SOGM_PROF_RING;
  if (n > cap) n = cap;
  *out_n = 0;
  if (c->ring[slot].empty()) return SOGM_OK;
  for (long long i = c->ring_n[slot] - n; i < c->ring_n[slot]; ++i) {  // oldest kept launch first
    hipEvent_t *p  = c->ring[slot].data() + 2 * (i % SOGM_PROF_RING);
    float       ms = 0.f;
    if (hipEventElapsedTime(&ms, p[0], p[1]) != hipSuccess) ms = -1.f;
    out_ms[(*out_n)++] = (double)ms;
  }
  return SOGM_OK;
}

int sogm_device_clock(sogm_ctx *c, int64_t *out_ticks, void *stream) {
  if (!c || !out_ticks) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (!c->h_tick_clock) {
    SOGM_HIP_CHECK(c->res.pinned(&c->h_tick_clock, sizeof(long long) * 4, hipHostMallocMapped));
    for (int i = 0; i < 4; ++i) c->h_tick_clock[i] = 0;
  }
  hipLaunchKernelGGL(k_device_clock, dim3(1), dim3(1), 0, (hipStream_t)stream, c->h_tick_clock + 2);
  SOGM_HIP_CHECK(hipGetLastError());
  SOGM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *out_ticks = (int64_t) * (volatile long long *)(c->h_tick_clock + 2);
  return SOGM_OK;
}
int sogm_tick_clock(sogm_ctx *c, int64_t *out2) {
  if (!c || !out2) return SOGM_ERR_INVALID_ARG;
  volatile long long *h = c->h_tick_clock;
  out2[0] = h ? (int64_t)h[0] : 0;
  out2[1] = h ? (int64_t)h[1] : 0;
  return SOGM_OK;
}

// diagnostics (tests/ only): GridGeom::div_res — the three-instruction fp32 division the stamp and the search use — against
// the IEEE division, on the device, for EVERY float in [lo, hi) and its negative.  out3_host = {mismatches, bit pattern of the
// first one (2^64 - 1 if none), whether the context uses the fast sequence at all (its resolution is 0.15f)}
int sogm_debug_div_check(sogm_ctx *c, float lo, float hi, unsigned long long *out3_host) {
  if (!c || !out3_host || !(lo > 0.0f) || !(hi > lo)) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  unsigned long long *d = nullptr;
  SOGM_HIP_CHECK(hipMalloc((void **)&d, 3 * sizeof(unsigned long long)));
  const unsigned long long init[3] = {0ull, ~0ull, 0ull};
  SOGM_HIP_CHECK(hipMemcpy(d, init, sizeof(init), hipMemcpyHostToDevice));
  unsigned bl, bh;
  std::memcpy(&bl, &lo, 4);
  std::memcpy(&bh, &hi, 4);
  hipLaunchKernelGGL(k_div_check, dim3(4096), dim3(256), 0, nullptr, c->geom, bl, bh, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out3_host, d, sizeof(init), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  SOGM_HIP_CHECK(e);
  return SOGM_OK;
}

// diagnostics (tools/ only): one agent's CURRENT grid ([T][V] cells, device layout) copied to a device buffer in stream
// order — no device synchronisation, no effect on the mark logs (unlike sogm_grid_ptr)
int sogm_debug_copy_grid(sogm_ctx *c, int agent, void *dst_dev, void *stream) {
  if (!c || !dst_dev || agent < 0 || agent >= c->n_agents) return SOGM_ERR_INVALID_ARG;
  const size_t bytes = (size_t)c->spec.T * (size_t)c->geom.V * c->cell_bytes();
  if (int rc = sogm::join_update(c, (hipStream_t)stream)) return rc;
  SOGM_HIP_CHECK(hipMemcpyAsync(dst_dev, (const char *)c->d_grid + (size_t)agent * bytes, bytes, hipMemcpyDeviceToDevice,
                                (hipStream_t)stream));
  return SOGM_OK;
}

}  // extern "C"
