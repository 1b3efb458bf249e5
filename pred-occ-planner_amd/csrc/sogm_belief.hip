// Belief audit (include/sogm_abi.h "belief audit"; the rules are sogm_belief.hpp's, shared with the host).  One launch:
//   k_belief_audit   a workgroup of 256 lanes owns BELIEF_PAIRS = 16 senders of one receiver (blockIdx.y), 16 lanes per
//                    (receiver, sender) pair, one lane per sample (belief_sample).  A lane reads what its sample needs of the
//                    two records straight from global memory — n_pieces, time_start, the durations, the fifteen control
//                    point coordinates of one piece — so the views are not streamed.  Sums and maxima are integer atomics
//                    in LDS: the receiver's twelve counters and the sixteen pairs' largest q; then one global atomic per
//                    workgroup and non-zero counter, and one plain store per pair of out_pair_q.
// Integer adds and maxima commute: the same bits from run to run.  Nothing is written to truth or views.
#include "sogm_device.hpp"
#include "sogm_belief.hpp"

#include <cstdio>

namespace sogm {
namespace {

constexpr int BELIEF_WG    = 256;
constexpr int BELIEF_LANES = SOGM_BELIEF_MAX_SAMPLES;  // lanes per pair
constexpr int BELIEF_PAIRS = BELIEF_WG / BELIEF_LANES;
static_assert(sizeof(SogmBeliefParams) == 56, "include/sogm_abi.h states the size");

struct BeliefArgs {
  SogmBeliefParams      prm;
  const SogmTrajRecord *truth, *views;
  const double         *t_now;
  unsigned long long   *counters;
  long long            *out_pair_q;
  int                   n_total, agent0;
};

__global__ __launch_bounds__(BELIEF_WG) void k_belief_audit(BeliefArgs g) {
  __shared__ unsigned long long s_cnt[SOGM_BELIEF_COUNTERS];
  __shared__ long long          s_pair[BELIEF_PAIRS];

  const int tid = threadIdx.x, s = tid % BELIEF_LANES, slot = tid / BELIEF_LANES;
  const int al = blockIdx.y, a = g.agent0 + al, N = g.n_total;
  const int j = blockIdx.x * BELIEF_PAIRS + slot;
  if (tid < SOGM_BELIEF_COUNTERS) s_cnt[tid] = 0;
  if (tid < BELIEF_PAIRS) s_pair[tid] = -1;
  __syncthreads();

  if (j < N && j != a) {
    const SogmTrajRecord &T = g.truth[j], &B = g.views[(size_t)al * N + j];
    const int             cls = belief_class(T.n_pieces, B.n_pieces);
    if (s == 0 && cls != BELIEF_NONE)
      atomicAdd(&s_cnt[cls == BELIEF_COMPARED ? BELIEF_CNT_COMPARED : cls == BELIEF_UNHEARD ? BELIEF_CNT_UNHEARD : BELIEF_CNT_PHANTOM],
                1ull);
    if (cls == BELIEF_COMPARED && s < g.prm.n_samples) {
      int       bin;
      long long q;
      belief_sample(g.prm, T, B, g.t_now[al], s, &bin, &q);
      atomicAdd(&s_cnt[BELIEF_CNT_SAMPLES], 1ull);
      atomicAdd(&s_cnt[BELIEF_CNT_BIN0 + bin], 1ull);
      if (q) atomicAdd(&s_cnt[BELIEF_CNT_SUM_Q], (unsigned long long)q);
      atomicMax(&s_pair[slot], q);
    }
  }
  __syncthreads();
  if (tid < BELIEF_PAIRS) {
    const int jj = blockIdx.x * BELIEF_PAIRS + tid;
    if (jj < N) {
      const long long worst = s_pair[tid];
      if (worst > 0) atomicMax(&s_cnt[BELIEF_CNT_MAX_Q], (unsigned long long)worst);
      if (g.out_pair_q) g.out_pair_q[(size_t)al * N + jj] = worst;
    }
  }
  __syncthreads();
  if (tid < SOGM_BELIEF_COUNTERS && s_cnt[tid]) {
    unsigned long long *dst = g.counters + (size_t)al * SOGM_BELIEF_COUNTERS + tid;
    if (tid == BELIEF_CNT_MAX_Q)
      atomicMax(dst, s_cnt[tid]);
    else
      atomicAdd(dst, s_cnt[tid]);
  }
}

int belief_refused(const char *entry, const char *what) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s: %s", entry, what);
  set_error_text(buf);
  return SOGM_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace sogm

extern "C" int sogm_belief_default_params(SogmBeliefParams *out) {
  using namespace sogm;
  if (!out) return belief_refused("sogm_belief_default_params", "null pointer");
  *out           = SogmBeliefParams{};
  out->dt_sample = 0.2;
  out->n_samples = 8;
  const double edges[5] = {0.05, 0.1, 0.2, 0.5, 1.0};
  for (int i = 0; i < 5; ++i) out->edges[i] = edges[i];
  return SOGM_OK;
}

extern "C" int sogm_belief_audit(const SogmBeliefParams *prm, const SogmTrajRecord *truth, const SogmTrajRecord *views,
                                 const double *t_now, int n_total, int agent0, int n_local, int64_t *counters,
                                 int64_t *out_pair_q, void *stream) {
  using namespace sogm;
  if (const char *why = belief_refuse(prm, truth, views, t_now, n_total, agent0, n_local, counters))
    return belief_refused("sogm_belief_audit", why);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
    set_error_text("sogm_belief_audit: no HIP device");
    return SOGM_ERR_NO_DEVICE;
  }
  BeliefArgs g{};
  g.prm        = *prm;
  g.truth      = truth;
  g.views      = views;
  g.t_now      = t_now;
  g.counters   = reinterpret_cast<unsigned long long *>(counters);
  g.out_pair_q = reinterpret_cast<long long *>(out_pair_q);
  g.n_total    = n_total;
  g.agent0     = agent0;
  hipLaunchKernelGGL(k_belief_audit, dim3((unsigned)((n_total - 1) / BELIEF_PAIRS + 1), (unsigned)n_local), dim3(BELIEF_WG), 0,
                     (hipStream_t)stream, g);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}
