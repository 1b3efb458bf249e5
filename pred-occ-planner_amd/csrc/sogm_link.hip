// Radio links (include/sogm_abi.h "radio links"; the rules are sogm_link.hpp's, shared with the host).  A delivery is two
// stream-ordered copies of the tick's table and positions into the ring, then one launch:
//   k_link_deliver   a workgroup of 256 lanes owns LINK_PAIRS = 4 senders of one receiver, one wave per (receiver, sender)
//                    pair.  Lanes 0 .. 7 evaluate the candidate send ticks k, k - 1, ..., k - 7 (link_candidate: 4 bytes of the
//                    ring's row, six doubles when there is a range, three mixes); a ballot of the arrivals and link_resolve
//                    pick the winner; all 64 lanes copy its 2064-byte record in 16-byte pieces (copy_record).  The wave whose
//                    sender is the receiver copies the current row.  The eight counters: lane 0 of each wave adds the pair's
//                    non-zero terms into LDS, one global integer add per workgroup and counter (none for a zero).
// Every ring index is tick % (delay_max + 1) of a tick in [tick0, k], k - tick <= delay_max: the slot still holds that
// tick.  No waiting on other workgroups; a wave writes only its own pair's view row and held tick.
#include "sogm_device.hpp"
#include "sogm_link.hpp"

#include <cstdio>

namespace sogm {
namespace {

constexpr int LINK_WG    = 256;
constexpr int LINK_PAIRS = LINK_WG / 64;
static_assert(sizeof(SogmTrajRecord) % 16 == 0, "records are copied in 16-byte pieces");
static_assert(sizeof(SogmLinkParams) == 40 && sizeof(SogmLinkBuffers) == 40, "include/sogm_abi.h states the sizes");

struct LinkArgs {
  SogmLinkParams  prm;
  SogmLinkBuffers b;
  int             k, tick0, n_total, agent0;
};

__global__ __launch_bounds__(LINK_WG) void k_link_deliver(LinkArgs g) {
  __shared__ unsigned long long s_cnt[SOGM_LINK_COUNTERS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int al = blockIdx.y, a = g.agent0 + al, N = g.n_total;
  const int j = blockIdx.x * LINK_PAIRS + wave;
  if (tid < SOGM_LINK_COUNTERS) s_cnt[tid] = 0;
  __syncthreads();

  if (j < N) {  // (uniform in the wave)
    const size_t    pair = (size_t)al * N + j;
    SogmTrajRecord *view = g.b.views + pair;
    if (j == a) {
      copy_record(view, g.b.ring_table + (size_t)link_slot(g.k, g.prm.delay_max) * N + a, lane);
      if (lane == 0) g.b.held_tick[pair] = g.k;
    } else {
      LinkCandidate c{false, false, false, false};
      if (lane < LINK_LANES) {
        const size_t row = (size_t)link_slot(g.k - lane < 0 ? 0 : g.k - lane, g.prm.delay_max) * N;  // read only for m >= tick0
        auto fetch_n   = [&]() { return g.b.ring_table[row + j].n_pieces; };
        auto fetch_pos = [&](double pj[3], double pa[3]) {
          for (int i = 0; i < 3; ++i) {
            pj[i] = g.b.ring_pos[(row + j) * 3 + i];
            pa[i] = g.b.ring_pos[(row + a) * 3 + i];
          }
        };
        c = link_candidate(g.prm, N, g.k, lane, g.tick0, j, a, fetch_n, fetch_pos);
      }
      const unsigned    arrivals = (unsigned)__ballot(c.arrives);  // bits 0 .. 7
      const int         held     = g.b.held_tick[pair];
      const LinkVerdict v        = link_resolve(g.prm, g.k, arrivals, held);
      if (v.apply) copy_record(view, g.b.ring_table + (size_t)link_slot(v.m, g.prm.delay_max) * N + j, lane);
      if (lane == 0) {
        const int held_after = v.apply ? v.m : held;
        if (v.apply) g.b.held_tick[pair] = v.m;
        long long add[SOGM_LINK_COUNTERS];
        link_pair_counts(c, arrivals, v, g.k, held_after, add);
#pragma unroll
        for (int i = 0; i < SOGM_LINK_COUNTERS; ++i)
          if (add[i]) atomicAdd(&s_cnt[i], (unsigned long long)add[i]);
      }
    }
  }
  __syncthreads();
  if (tid < SOGM_LINK_COUNTERS && s_cnt[tid])
    atomicAdd(reinterpret_cast<unsigned long long *>(g.b.counters) + (size_t)al * SOGM_LINK_COUNTERS + tid, s_cnt[tid]);
}

int link_refuse(const char *entry, const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

int link_no_device(const char *entry) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0) return SOGM_OK;
  char buf[96];
  std::snprintf(buf, sizeof(buf), "%s: no HIP device", entry);
  set_error_text(buf);
  return SOGM_ERR_NO_DEVICE;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_link_default_params(SogmLinkParams *out) {
  using namespace sogm;
  if (!out) return link_refuse("sogm_link_default_params", "null pointer");
  *out = SogmLinkParams{};  // perfect links
  return SOGM_OK;
}

extern "C" int sogm_link_init(const SogmLinkParams *prm, int n_total, int n_local, const SogmLinkBuffers *b, void *stream) {
  using namespace sogm;
  if (const char *why = link_refuse_buffers(prm, n_total, n_local, b)) return link_refuse("sogm_link_init", why);
  if (const int rc = link_no_device("sogm_link_init")) return rc;
  hipStream_t  st    = (hipStream_t)stream;
  const size_t slots = (size_t)prm->delay_max + 1, pairs = (size_t)n_local * n_total;
  SOGM_HIP_CHECK(hipMemsetAsync(b->ring_table, 0, slots * n_total * sizeof(SogmTrajRecord), st));
  if (b->ring_pos) SOGM_HIP_CHECK(hipMemsetAsync(b->ring_pos, 0, slots * n_total * 3 * sizeof(double), st));
  SOGM_HIP_CHECK(hipMemsetAsync(b->views, 0, pairs * sizeof(SogmTrajRecord), st));
  SOGM_HIP_CHECK(hipMemsetAsync(b->held_tick, 0xFF, pairs * sizeof(int32_t), st));  // -1
  SOGM_HIP_CHECK(hipMemsetAsync(b->counters, 0, (size_t)n_local * SOGM_LINK_COUNTERS * sizeof(int64_t), st));
  return SOGM_OK;
}

extern "C" int sogm_link_deliver(const SogmLinkParams *prm, int tick, int tick0, const SogmTrajRecord *table, const double *pos,
                                 int n_total, int agent0, int n_local, const SogmLinkBuffers *b, void *stream) {
  using namespace sogm;
  if (const char *why = link_refuse_call(prm, tick, tick0, table, pos, n_total, agent0, n_local, b))
    return link_refuse("sogm_link_deliver", why);
  if (n_local > 65535) return link_refuse("sogm_link_deliver", "n_local exceeds one launch (65535)");
  if (const int rc = link_no_device("sogm_link_deliver")) return rc;
  hipStream_t  st   = (hipStream_t)stream;
  const size_t slot = (size_t)link_slot(tick, prm->delay_max);
  SOGM_HIP_CHECK(hipMemcpyAsync(b->ring_table + slot * n_total, table, (size_t)n_total * sizeof(SogmTrajRecord),
                                hipMemcpyDeviceToDevice, st));
  if (prm->range > 0)
    SOGM_HIP_CHECK(hipMemcpyAsync(b->ring_pos + slot * n_total * 3, pos, (size_t)n_total * 3 * sizeof(double),
                                  hipMemcpyDeviceToDevice, st));
  LinkArgs g{};
  g.prm     = *prm;
  g.b       = *b;
  g.k       = tick;
  g.tick0   = tick0;
  g.n_total = n_total;
  g.agent0  = agent0;
  hipLaunchKernelGGL(k_link_deliver, dim3((unsigned)((n_total + LINK_PAIRS - 1) / LINK_PAIRS), (unsigned)n_local),
                     dim3(LINK_WG), 0, st, g);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
