// sogm_dsp_state.hip — the particle map's handle on the host: create and destroy, the state up- and downloads of the tests
// and tools, and the velocity audit's view of the handle.  No kernel lives here; the update and the publishing are
// sogm_dsp.hip, the velocity estimation sogm_dsp_velocity.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "sogm_dsp.hpp"

using namespace sogm;

// (sogm_device.hpp) the handle's arrays as sogm_velaudit.hip reads them: nothing of the handle is written through this view
int sogm::dsp_born_view(const sogm_dsp *h, DspBornView *out) {
  if (!h || !out) return SOGM_ERR_INVALID_ARG;
  static_assert(sizeof(DspAgent) % sizeof(int32_t) == 0, "the agents' scalars are strided in ints");
  out->born     = h->d.born;
  out->born_src = h->d.born_src;
  out->ok       = &h->d.ag->ok;
  out->n_born   = &h->d.ag->n_born;
  out->stride   = (int)(sizeof(DspAgent) / sizeof(int32_t));
  out->n_agents = h->d.A;
  out->max_pts  = h->d.max_pts;
  out->device   = h->map->device;
  return SOGM_OK;
}

namespace {
template <typename T>
int dupload(sogm_dsp *h, const T **out, const T *src, size_t n) {
  if (h->res.array(const_cast<T **>(out), n) != hipSuccess) return -1;
  return hipMemcpy(const_cast<T *>(*out), src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess ? -1 : 0;
}

// host-side constant tables (setInitParameters :566-632) — set-up, evaluated once with libm.
// Boundary-plane normals of the FOV pyramids: `n` planes, `half` of them either side of the axis, `arr` radians apart.
std::vector<float> boundary_planes(int n, int half, float arr, bool vertical) {
  std::vector<float> b(n * 3);
  for (int i = -half; i <= half; i++) {
    if (vertical) {
      b[(i + half) * 3 + 0] = sinf((float)i * arr);
      b[(i + half) * 3 + 1] = 0.f;
      b[(i + half) * 3 + 2] = cosf((float)i * arr);
    } else {
      b[(i + half) * 3 + 0] = -sinf((float)i * arr);
      b[(i + half) * 3 + 1] = cosf((float)i * arr);
      b[(i + half) * 3 + 2] = 0.f;
    }
  }
  return b;
}
// Neighbour table: per pyramid its count and up to nine pyramids (itself included) of the 3 x 3 around it, in scan order.
std::vector<int> neighbour_table(int nph, int npv) {
  std::vector<int> nbr((size_t)nph * npv * 10, 0);
  for (int i = 0; i < nph * npv; i++) {
    int h0 = i / npv, v0 = i % npv, n = 0;
    for (int x = -1; x <= 1; ++x)
      for (int y = -1; y <= 1; ++y) {
        int hh = h0 + x, vv = v0 + y;
        if (hh >= 0 && hh < nph && vv >= 0 && vv < npv) nbr[i * 10 + 1 + n++] = hh * npv + vv;
      }
    nbr[i * 10] = n;
  }
  return nbr;
}
// Gaussian PDF lookup (calculateNormalPDFBuffer :1373-1378)
std::vector<float> pdf_table() {
  std::vector<float> pdf(20000);
  for (int i = 0; i < 20000; ++i) {
    float value = (float)(i - 10000) * 0.001f;
    pdf[i]      = (1.f / (sqrtf(2.f * 1.57079632679489661923f))) * expf(-powf(value, 2) / (2));
  }
  return pdf;
}

// The external store row of one slot (sogm_dsp_download_state / sogm_dsp_upload_state), 9 floats:
//   flag value, vx, vy, vz = 0, px, py, pz, w, time = 0
constexpr int   ROW       = 9;
constexpr int   ROW_OF[6] = {1, 2, 4, 5, 6, 7};                           // where vx vy px py pz w of a slot sit in its row
constexpr float FLAG_VALUE[7] = {0.f, 1.f, 0.6f, 7.f, 15.f, 0.f, 0.f};  // by flag code; the transient codes read as empty
void slot_to_row(uint8_t flag, const float f[6], float *o) {
  o[0] = FLAG_VALUE[flag < 7 ? flag : 0];
  o[3] = 0.f;
  o[8] = 0.f;
  for (int k = 0; k < 6; ++k) o[ROW_OF[k]] = f[k];
}
// false: not a row of a between-updates store — a flag value that is not exactly that of F_EMPTY, F_VALID or F_RESAMP (a NaN
// compares unequal to all three), or a live slot with vz != 0
bool row_to_slot(const float *o, uint8_t *flag, float f[6]) {
  uint8_t c = F_EMPTY;
  while (c <= F_RESAMP && !(o[0] == FLAG_VALUE[c])) ++c;
  if (c > F_RESAMP) return false;
  if (c != F_EMPTY && !(o[3] == 0.f)) return false;
  *flag = c;
  for (int k = 0; k < 6; ++k) f[k] = o[ROW_OF[k]];
  return true;
}

// the entry checks of every download / upload, then the device quiet
int quiesce(sogm_dsp *h) {
  SOGM_HIP_CHECK(hipSetDevice(h->map->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  return SOGM_OK;
}
int read_agent(const sogm_dsp *h, int agent, DspAgent *s) {
  SOGM_HIP_CHECK(hipMemcpy(s, h->d.ag + agent, sizeof(*s), hipMemcpyDeviceToHost));
  return SOGM_OK;
}
}  // namespace

extern "C" {

void sogm_dsp_destroy(sogm_dsp *h) {
  if (!h) return;
  (void)hipSetDevice(h->map->device);
  h->res.release_all();
  delete h;
}

int sogm_dsp_create(sogm_ctx *map, const SogmDspParams *P, const float *p_gauss, const float *v_gauss,
                    int n_gauss, const int32_t *rand_tab, int n_rand, int max_points, sogm_dsp **out) {
  if (!map || !P || !out || !p_gauss || !v_gauss || !rand_tab || n_gauss <= 0 || n_rand <= 0 ||
      max_points <= 0 || max_points > VEL_MAX_POINTS)
    return SOGM_ERR_INVALID_ARG;
  const SogmSpec &sp = map->spec;
  const int       S  = P->max_particle_num_voxel * 2;
  const int       ar = P->angle_resolution;
  if (S > DSP_SLOTS || S < 1 || ar < 1 || sp.T > SOGM_DSP_MAX_T || P->newborn_num < 1 ||
      P->obs_max_per_pyramid < 2 || P->half_fov_h * 2 / ar > 180 || P->half_fov_v * 2 / ar > 180)
    return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(map->device));
  // checked here instead of failing every later sogm_update_dsp(labels = NULL) launch
  const int fits = velocity_lds_fits(max_points, map->device);
  if (fits < 0) return fits;
  if (!fits) {
    set_error("sogm_dsp_create: max_points needs more LDS than a workgroup can have (k_dsp_velocity)", hipErrorInvalidValue);
    return SOGM_ERR_CAPACITY;
  }
  sogm_dsp *h = new (std::nothrow) sogm_dsp();  // (value-initialised: `d` is zero)
  if (!h) return SOGM_ERR_HIP;
  h->map    = map;
  h->P      = *P;
  DspDev &d = h->d;
  if (!dsp_set_shape(d, map->n_agents, sp, *P, max_points, n_gauss, n_rand)) {
    delete h;
    return SOGM_ERR_INVALID_ARG;
  }
  const float              arr = (float)ar / 180.f * 3.14159265358979323846f;
  const std::vector<float> bh = boundary_planes(d.nph + 1, P->half_fov_h / ar, arr, false),
                           bv = boundary_planes(d.npv + 1, P->half_fov_v / ar, arr, true);
  const std::vector<float> pdf = pdf_table();
  const std::vector<int>   nbr = neighbour_table(d.nph, d.npv);
  const size_t             A   = d.A;
  int                      bad = 0;
  dsp_for_each_buffer(d, [&](auto *&p, size_t per_agent, DspFill) { bad |= h->res.array(&p, A * per_agent); });
  bad |= dupload(h, &d.pg, p_gauss, (size_t)n_gauss);
  bad |= dupload(h, &d.vg, v_gauss, (size_t)n_gauss);
  bad |= dupload(h, &d.rnd, (const int *)rand_tab, (size_t)n_rand);
  bad |= dupload(h, &d.pdf, pdf.data(), pdf.size());
  bad |= dupload(h, &d.bp_ori_h, bh.data(), bh.size());
  bad |= dupload(h, &d.bp_ori_v, bv.data(), bv.size());
  bad |= dupload(h, &d.nbr, nbr.data(), nbr.size());
  if (bad) {
    set_error("sogm_dsp_create: hipMalloc", hipGetLastError());
    sogm_dsp_destroy(h);
    return SOGM_ERR_HIP;
  }
  std::vector<DspAgent> ag(A);
  std::memset(ag.data(), 0, A * sizeof(DspAgent));
  for (auto &x : ag) {
    x.first   = 1;
    x.quat[0] = 1.f;
  }
  hipError_t e = hipMemcpy(d.ag, ag.data(), A * sizeof(DspAgent), hipMemcpyHostToDevice);
  dsp_for_each_buffer(d, [&](auto *&p, size_t per_agent, DspFill fill) {
    if (e == hipSuccess && fill != DSP_FILL_NONE) e = hipMemset(p, fill == DSP_FILL_FF ? 0xFF : 0, A * per_agent * sizeof(*p));
  });
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // null-stream memsets: complete before the first update on another stream
  if (e != hipSuccess) {
    set_error("sogm_dsp_create: init", e);
    sogm_dsp_destroy(h);
    return SOGM_ERR_HIP;
  }
  reserve_update_lds(d);
  *out = h;
  return SOGM_OK;
}

int sogm_dsp_download_state(sogm_dsp *h, int agent, float *store, float *objnum, int32_t *counters) {
  if (!h || agent < 0 || agent >= h->d.A) return SOGM_ERR_INVALID_ARG;
  DspDev &d = h->d;
  if (int rc = quiesce(h)) return rc;
  const size_t V = d.V, VS = V * DSP_SLOTS;
  if (store) {
    std::vector<uint8_t> fl(VS);
    std::vector<float>   f[6];
    SOGM_HIP_CHECK(hipMemcpy(fl.data(), d.flag + d.slot_base(agent), VS, hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; ++k) {
      f[k].resize(VS);
      SOGM_HIP_CHECK(hipMemcpy(f[k].data(), d.f[k] + d.slot_base(agent), VS * sizeof(float), hipMemcpyDeviceToHost));
    }
    for (size_t v = 0; v < V; ++v)
      for (int p = 0; p < d.S; ++p) {
        const size_t at   = v * DSP_SLOTS + p;
        const float  s[6] = {f[0][at], f[1][at], f[2][at], f[3][at], f[4][at], f[5][at]};
        slot_to_row(fl[at], s, store + (v * d.S + p) * ROW);
      }
  }
  if (objnum) {
    std::vector<float> occ(4 * V), fut((size_t)d.T * V);
    SOGM_HIP_CHECK(hipMemcpy(occ.data(), d.occ + d.occ_base(agent), occ.size() * sizeof(float), hipMemcpyDeviceToHost));
    SOGM_HIP_CHECK(hipMemcpy(fut.data(), d.fut + d.fut_base(agent), fut.size() * sizeof(float), hipMemcpyDeviceToHost));
    const int OD = 4 + d.T;
    for (size_t v = 0; v < V; ++v) {
      for (int k = 0; k < 4; ++k) objnum[v * OD + k] = occ[k * V + v];
      for (int t = 0; t < d.T; ++t) objnum[v * OD + 4 + t] = fut[(size_t)t * V + v];
    }
  }
  if (counters) {
    DspAgent s;
    if (int rc = read_agent(h, agent, &s)) return rc;
    std::memset(counters, 0, 16 * sizeof(int32_t));
    counters[0]  = s.dbg_voxel_full;
    counters[1]  = s.dbg_pyr_full;
    counters[2]  = s.dbg_out;
    counters[3]  = s.cand_cnt;
    counters[4]  = s.pseq;
    counters[5]  = s.vseq;
    counters[6]  = s.rseq;
    counters[7]  = d.S;
    counters[8]  = d.SP;
    counters[9]  = d.NP;
    counters[10] = s.err_unconverged;
    counters[11] = s.err_pool;
    counters[12] = s.err_points;
    counters[13] = s.valid_points;
    counters[14] = s.n_obs;
    counters[15] = s.ok;
  }
  return SOGM_OK;
}

// Test hook (sogm_abi_debug.h): the inverse of sogm_dsp_download_state for a between-updates store.  Validated on the
// host before anything is written; plain copies, no kernel.
int sogm_dsp_upload_state(sogm_dsp *h, int agent, const float *store, const float *last_pos3, double last_stamp,
                          const int32_t *cursors3) {
  if (!h || agent < 0 || agent >= h->d.A || !store || !last_pos3 || !cursors3) return SOGM_ERR_INVALID_ARG;
  DspDev &d = h->d;
  if (cursors3[0] < 0 || cursors3[0] >= d.n_gauss || cursors3[1] < 0 || cursors3[1] >= d.n_gauss || cursors3[2] < 0 ||
      cursors3[2] >= d.n_rand)
    return SOGM_ERR_INVALID_ARG;
  const size_t V = d.V, VS = V * DSP_SLOTS;
  std::vector<uint8_t> fl(VS, (uint8_t)F_EMPTY);
  std::vector<float>   f[6];
  for (int k = 0; k < 6; ++k) f[k].assign(VS, 0.f);
  for (size_t v = 0; v < V; ++v)
    for (int p = 0; p < d.S; ++p) {
      const size_t at = v * DSP_SLOTS + p;
      float        s[6];
      if (!row_to_slot(store + (v * d.S + p) * ROW, &fl[at], s)) return SOGM_ERR_INVALID_ARG;
      for (int k = 0; k < 6; ++k) f[k][at] = s[k];
    }
  if (int rc = quiesce(h)) return rc;
  DspAgent s;
  if (int rc = read_agent(h, agent, &s)) return rc;
  SOGM_HIP_CHECK(hipMemcpy(d.flag + d.slot_base(agent), fl.data(), VS, hipMemcpyHostToDevice));
  for (int k = 0; k < 6; ++k)
    SOGM_HIP_CHECK(hipMemcpy(d.f[k] + d.slot_base(agent), f[k].data(), VS * sizeof(float), hipMemcpyHostToDevice));
  SOGM_HIP_CHECK(hipMemset(d.occ + d.occ_base(agent), 0, 4 * V * sizeof(float)));
  SOGM_HIP_CHECK(hipMemset(d.fut + d.fut_base(agent), 0, (size_t)d.T * V * sizeof(float)));
  for (int k = 0; k < 3; ++k) s.last_p[k] = last_pos3[k];
  s.last_t = last_stamp;
  s.first  = 0;
  s.pseq   = cursors3[0];
  s.vseq   = cursors3[1];
  s.rseq   = cursors3[2];
  s.cand_cnt = 0;
  s.dbg_voxel_full = s.dbg_pyr_full = s.dbg_out = 0;
  s.err_unconverged = s.err_pool = s.err_points = 0;
  s.vel_n_last = 0;
  SOGM_HIP_CHECK(hipMemcpy(d.ag + agent, &s, sizeof(s), hipMemcpyHostToDevice));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  return SOGM_OK;
}

int sogm_dsp_download_observations(sogm_dsp *h, int agent, int32_t *nobs, float *pc, float *maxlen) {
  if (!h || agent < 0 || agent >= h->d.A) return SOGM_ERR_INVALID_ARG;
  DspDev &d = h->d;
  if (int rc = quiesce(h)) return rc;
  const size_t NP = d.NP;
  if (nobs) SOGM_HIP_CHECK(hipMemcpy(nobs, d.nobs + d.pyr_base(agent), NP * sizeof(int), hipMemcpyDeviceToHost));
  if (pc)
    SOGM_HIP_CHECK(hipMemcpy(pc, d.pc + d.obs_base(agent) * 5, NP * d.OM * 5 * sizeof(float), hipMemcpyDeviceToHost));
  if (maxlen) {
    std::vector<int> b(NP);
    SOGM_HIP_CHECK(hipMemcpy(b.data(), d.maxlen + d.pyr_base(agent), NP * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < NP; ++i) {
      float f;
      std::memcpy(&f, &b[i], 4);
      maxlen[i] = b[i] < 0 ? -1.f : f;
    }
  }
  return SOGM_OK;
}

// Parity I/O (synchronous): input_cloud_with_velocity of the last update — rows {x, y, z, vx, vy, vz, intensity} in
// the order new-born particles are created — and counters {clusters, possibly dynamic, matched, error code}.
int sogm_dsp_download_born(sogm_dsp *h, int agent, float *born_host, int cap, int32_t *n_born, int32_t *counters4) {
  if (!h || agent < 0 || agent >= h->d.A || cap < 0) return SOGM_ERR_INVALID_ARG;
  DspDev &d = h->d;
  if (int rc = quiesce(h)) return rc;
  DspAgent ag;
  if (int rc = read_agent(h, agent, &ag)) return rc;
  if (n_born) *n_born = ag.n_born;
  if (counters4) {
    counters4[0] = ag.vel_clusters;
    counters4[1] = ag.vel_dynamic;
    counters4[2] = ag.vel_matched;
    counters4[3] = ag.vel_err;
  }
  if (born_host) {
    const size_t n = (size_t)(ag.n_born < cap ? ag.n_born : cap);
    SOGM_HIP_CHECK(hipMemcpy(born_host, d.born + d.point_base(agent) * 7, n * 7 * sizeof(float), hipMemcpyDeviceToHost));
  }
  return SOGM_OK;
}

// The source index of that list (sogm_abi_debug.h): born_src rows 0 .. n_born - 1.
int sogm_dsp_download_born_source(sogm_dsp *h, int agent, int32_t *out, int cap, int32_t *n_born) {
  if (!h || agent < 0 || agent >= h->d.A || cap < 0) return SOGM_ERR_INVALID_ARG;
  DspDev &d = h->d;
  if (int rc = quiesce(h)) return rc;
  DspAgent ag;
  if (int rc = read_agent(h, agent, &ag)) return rc;
  if (n_born) *n_born = ag.n_born;
  if (out) {
    const size_t n = (size_t)(ag.n_born < cap ? ag.n_born : cap);
    SOGM_HIP_CHECK(hipMemcpy(out, d.born_src + d.point_base(agent), n * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  return SOGM_OK;
}

}  // extern "C"
