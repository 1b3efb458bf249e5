// Host test of what the particle map is made of (csrc/sogm_dsp.hpp), compiled with the host compiler: the two rules of the
// ordered first-fit — keep_smallest against "sort everything, take the first cap", lowest_free over every occupancy of a
// small voxel — and the buffer table against the per-agent accessors the kernels address the arrays by.
#include "sogm_dsp.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static int id_of(int key) { return key * 7 + 3; }

// one stream of distinct keys through keep_smallest, against the sorted stream's first `cap`
static int keep_smallest_stream(const std::vector<int> &keys, int cap, bool with_ids) {
  std::vector<int> K(cap, -1), I(cap, -1);  // heap: the sanitizers watch the bounds
  int              n = 0;
  for (int key : keys) keep_smallest(K.data(), with_ids ? I.data() : nullptr, n, cap, key, id_of(key));
  std::vector<int> want(keys);
  std::sort(want.begin(), want.end());
  if ((int)want.size() > cap) want.resize(cap);
  EXPECT(n == (int)want.size());
  for (int i = 0; i < n; ++i) {
    EXPECT(K[i] == want[i]);
    EXPECT(I[i] == (with_ids ? id_of(want[i]) : -1));
  }
  for (int i = n; i < cap; ++i) EXPECT(K[i] == -1 && I[i] == -1);  // nothing past the kept keys is touched
  return 0;
}
static int keep_smallest_cases() {
  std::mt19937 rng(20240607u);
  for (int cap : {1, 2, 16, 20})
    for (int len = 0; len <= 3 * cap; ++len)
      for (int order = 0; order < 3; ++order) {
        std::vector<int> keys(len);
        for (int i = 0; i < len; ++i) keys[i] = 5 + 3 * i;  // distinct, as sweep keys are
        if (order == 1) std::reverse(keys.begin(), keys.end());
        if (order == 2) std::shuffle(keys.begin(), keys.end(), rng);
        for (bool with_ids : {true, false})
          if (keep_smallest_stream(keys, cap, with_ids)) return 1;
      }
  return 0;
}

static int lowest_free_cases() {
  for (unsigned occ = 0; occ < 16u; ++occ) {  // every occupancy of a 4-slot voxel
    int want = -1;
    for (int p = 3; p >= 0; --p)
      if (!((occ >> p) & 1u)) want = p;
    EXPECT(lowest_free(occ, 0xFu) == want);
  }
  const unsigned all16 = (1u << 16) - 1u;  // S = 16
  EXPECT(lowest_free(0u, all16) == 0);
  for (int p = 0; p < 16; ++p) EXPECT(lowest_free(1u << p, all16) == (p == 0 ? 1 : 0));
  EXPECT(lowest_free(all16 & ~(1u << 15), all16) == 15);
  EXPECT(lowest_free(all16, all16) == -1);
  return 0;
}

// DspDev of (A, V = L^3, NP = nph * npv, max_pts, nb), filled by the function sogm_dsp_create uses
static bool shape(DspDev &d, int A, int L, int half_h, int half_v, int max_pts, int nb) {
  SogmSpec      sp{};
  SogmDspParams P{};
  sp.L = sp.W = sp.H = L;
  sp.T           = 6;
  sp.resolution  = 0.15f;
  P.angle_resolution       = 1;
  P.half_fov_h             = half_h;
  P.half_fov_v             = half_v;
  P.max_particle_num_voxel = 8;
  P.obs_max_per_pyramid    = 10;
  P.newborn_num            = nb;
  return dsp_set_shape(d, A, sp, P, max_pts, 1000, 1000);
}

static int buffer_table(int A, int V, int NP, int max_pts, int nb, int L, int half_h, int half_v) {
  DspDev d{};
  EXPECT(shape(d, A, L, half_h, half_v, max_pts, nb));
  EXPECT(d.A == A && d.V == V && d.NP == NP && d.max_pts == max_pts && d.nb == nb && d.SP >= 1);
  std::map<const void *, size_t> count;  // the member's address in `d` -> its elements per agent
  dsp_for_each_buffer(d, [&](auto *&p, size_t per_agent, DspFill) { count[(const void *)&p] = per_agent; });
  std::set<const void *> seen;
  // `base(a)` x `per` is where agent a's part of `member` starts: a times the table's count, and the last agent's part ends
  // at the allocated total
  auto holds = [&](const void *member, auto base, size_t per) {
    if (!count.count(member) || !seen.insert(member).second) return false;
    const size_t c = count[member];
    for (int a = 0; a < A; ++a)
      if (base(a) * per != (size_t)a * c) return false;
    return base(A - 1) * per + c == (size_t)A * c;
  };
  auto slot = [&](int a) { return d.slot_base(a); };
  auto vox  = [&](int a) { return d.voxel_base(a); };
  auto pyr  = [&](int a) { return d.pyr_base(a); };
  auto obs  = [&](int a) { return d.obs_base(a); };
  auto bph  = [&](int a) { return d.bph_base(a); };
  auto bpv  = [&](int a) { return d.bpv_base(a); };
  auto cand = [&](int a) { return d.cand_base(a); };
  auto pt   = [&](int a) { return d.point_base(a); };
  auto nbn  = [&](int a) { return d.newborn_base(a); };
  auto fut  = [&](int a) { return d.fut_base(a); };
  auto occ  = [&](int a) { return d.occ_base(a); };
  auto one  = [&](int a) { return (size_t)a; };
  EXPECT(holds(&d.ag, one, 1));
  EXPECT(holds(&d.flag, slot, 1));
  for (int k = 0; k < 6; ++k) EXPECT(holds(&d.f[k], slot, 1));
  EXPECT(holds(&d.vhead, vox, 1));
  EXPECT(holds(&d.nobs, pyr, 1) && holds(&d.maxlen, pyr, 1) && holds(&d.phead, pyr, 1) && holds(&d.pyr_n, pyr, 1));
  EXPECT(holds(&d.pyr_list, pyr, d.SP) && holds(&d.pyr_key, pyr, d.SP) && holds(&d.pyr_id, pyr, d.SP));
  EXPECT(holds(&d.pc, obs, 5));
  EXPECT(holds(&d.bp_h, bph, 3) && holds(&d.bp_v, bpv, 3));
  EXPECT(holds(&d.c_key, cand, 1) && holds(&d.c_dest, cand, 1) && holds(&d.c_pyr, cand, 1) && holds(&d.c_assign, cand, 1));
  EXPECT(holds(&d.c_vnext, cand, 1) && holds(&d.c_pnext, cand, 1) && holds(&d.c_kill, cand, 1) && holds(&d.c_pay, cand, 6));
  EXPECT(holds(&d.obs_list, pt, 1) && holds(&d.born_src, pt, 1) && holds(&d.vel_deg, pt, 1));
  EXPECT(holds(&d.b_valid, pt, 1) && holds(&d.b_nstatic, pt, 1) && holds(&d.b_vi, pt, 1));
  EXPECT(holds(&d.born, pt, 7) && holds(&d.b_c, pt, 3) && holds(&d.vel_adj, pt, VEL_ADJ_CAP));
  EXPECT(holds(&d.b_cls, nbn, 1) && holds(&d.b_dest, nbn, 1) && holds(&d.b_vnext, nbn, 1) && holds(&d.b_pay, nbn, 5));
  EXPECT(holds(&d.fut, fut, 1) && holds(&d.occ, occ, 1));
  EXPECT(seen.size() == count.size());  // no array of the table without an accessor
  // a voxel's slots inside its agent's
  for (int a = 0; a < A; ++a)
    for (int v : {0, 1, V - 1}) EXPECT(d.slot_base(a, v) == d.slot_base(a) + (size_t)v * DSP_SLOTS);
  EXPECT(d.slot_base(A - 1, V - 1) + DSP_SLOTS == (size_t)A * count[&d.flag]);
  return 0;
}

int main() {
  if (keep_smallest_cases()) return 1;
  if (lowest_free_cases()) return 1;
  if (buffer_table(1, 8, 4, 16, 2, /*L*/ 2, /*half fov*/ 1, 1)) return 1;
  if (buffer_table(3, 1000, 60, 64, 20, /*L*/ 10, /*half fov*/ 5, 3)) return 1;
  std::printf("dsp rules host ok\n");
  return 0;
}
