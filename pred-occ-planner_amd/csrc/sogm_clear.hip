// sogm_clear.hip — everything that zeroes a SOGM grid, and the pool of grids it is done for (sogm_gridpool.hpp): the
// dense clear (k_clear_slabs / k_clear_chunks: the voxel-update roofline kernel, B = V*T*4 bytes per agent-update), the
// sparse reset through the mark logs (k_reset_sectors), the spares' side-stream pre-clears and their adoption by the next
// update, and the ABI entries that only concern the pool and its logs.
#include <hip/hip_runtime.h>

#include <vector>

#include "sogm_device.hpp"

namespace sogm {

// ------------------------------------------------------------------------------------------------
// clear
// ------------------------------------------------------------------------------------------------
// Pure streaming store.  One float4 (16 B) per lane per iteration -> 1 KiB per wave-instruction,
// fully coalesced; 4 independent stores in flight per lane per trip.  The grid is sized to
// ~8 workgroups per CU and strides over the buffer.
template <bool NT>
__device__ inline void clear_store(vfloat4 *p) {
  const vfloat4 z = {0.f, 0.f, 0.f, 0.f};
  if (NT)
    __builtin_nontemporal_store(z, p);
  else
    *p = z;
}
template <bool NT>
__global__ __launch_bounds__(256) void k_clear_slabs(vfloat4 *__restrict__ p, size_t n_vec4,
                                                     float *__restrict__ tail, int n_tail, int throttle) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t       i      = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n_vec4; i += 4 * stride) {
    clear_store<NT>(p + i);
    clear_store<NT>(p + i + stride);
    clear_store<NT>(p + i + 2 * stride);
    clear_store<NT>(p + i + 3 * stride);
    // tuning aid: bound the stores a wave keeps in flight (vmcnt <= 4 / 8 / 12)
    if (throttle == 4) __builtin_amdgcn_s_waitcnt(0x0F74);
    else if (throttle == 8) __builtin_amdgcn_s_waitcnt(0x0F78);
    else if (throttle == 12) __builtin_amdgcn_s_waitcnt(0x0F7C);
    else if (throttle == 1) __builtin_amdgcn_s_waitcnt(0x0F70);
  }
  for (; i < n_vec4; i += stride) clear_store<NT>(p + i);
  if (blockIdx.x == 0 && (int)threadIdx.x < n_tail) tail[threadIdx.x] = 0.f;
}

// The same stream of stores with a width that follows the tick (side-stream clear of the dataflow replan).  The
// grid is cut into 4 MiB chunks handed out by an atomic cursor shared by TWO launches: a narrow one (64 workgroups,
// <= 4 stores in flight per wave: what the latency-bound planner kernels tolerate beside them) that starts with the
// tick, and a wide, unbounded one on a second stream behind k_clear_gate, which returns once *gate >= gate_target —
// every agent's corridors are final, what is left of the tick iterates in LDS (QP) — or the tick failed, or no
// chunk is left.  (Gating at launch granularity matters: workgroups that merely SLEEP on a CU hold a wave slot per
// SIMD, and a QP workgroup — 2 x 256 registers per SIMD — cannot be placed beside them.)  A workgroup asks for its
// next chunk before it stores the current one, so the cursor's round trip hides under the stores.
#define CLEAR_CHUNK_V4 (size_t)(4u << 20 >> 4)  // 16-byte elements per chunk
__global__ void k_clear_gate(const unsigned long long *__restrict__ cursor, size_t nchunks,
                             const int *__restrict__ gate, const int *__restrict__ gate_err, int gate_target,
                             const int *__restrict__ epoch_word, int epoch) {
  if (threadIdx.x != 0) return;
  // bounded like every device-side wait of the tick (0.5 s of the 100 MHz clock): opening the wide launch early is
  // harmless, a gate that never returns is not (e.g. under a profiler that serialises kernels and runs this one
  // before the narrow launch it watches)
  const long long t0 = wall_clock64();
  for (;;) {
    if (wall_clock64() - t0 > 50000000LL) break;
    if (__hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= nchunks) break;
    // the replan this clear runs under writes `epoch` after resetting its counters; a later epoch = it is over
    const int e = __hip_atomic_load(epoch_word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if (e != 0 && e - epoch > 0) break;
    if (e == epoch && (__hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= gate_target ||
                       __hip_atomic_load(gate_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0))
      break;
#pragma unroll
    for (int i = 0; i < 4; ++i) __builtin_amdgcn_s_sleep(127);  // ~14 us between polls
  }
}
__global__ void k_set_word(int *p, int v) { *p = v; }
// (the mark log's counters are zeroed by a kernel, not a memset node: measured with four hardware queues, a 24-byte
//  hipMemsetAsync ran AFTER work another stream had ordered behind an event recorded after it)
__global__ void k_zero_words(unsigned *p, int n) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) p[i] = 0u;
}

// Sparse reset: zero the 32-byte sectors named by an agent's mark log (duplicates and ~0 place-holders included; the
// sector of a logged cell holds nothing but marks of the same log or zeros).  An overflowed log (n > cap) makes the
// agent's workgroups zero its whole grid instead.  Launched (blocks, A); the counts are reset by a kernel behind it.
// LANES adjacent lanes zero one entry with one 16-byte store each, so an entry is ONE write request of 16*LANES bytes
// at the L2 instead of two of 16; LANES = 4 zeroes the aligned 64-byte pair of sectors (everything
// non-zero in a tracked grid is in the log, so the neighbour sector holds marks of the same log or zeros as well).  An
// entry equal to the one before it in the wave is skipped: neighbouring marks of a stamp row log the same sector.
// Measured alone on 80.6 M entries (cfg2, 128 agents): one lane per entry with two stores 1.10 ms; 2 lanes 0.91;
// 4 lanes 0.87; 4 lanes x 8 entries per trip 0.745; 8 lanes (128-byte lines) 1.08-1.2.  reset_slot picks per use.
template <int LANES, int UNROLL>
__global__ __launch_bounds__(256) void k_reset_sectors(char *__restrict__ grid, size_t agent_bytes,
                                                       const unsigned *__restrict__ entries,
                                                       const unsigned *__restrict__ counts, int cap,
                                                       unsigned long long *__restrict__ stat) {
  const int      agent = blockIdx.y;
  const unsigned n     = counts[agent];
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // statistics for sogm_sparse_reset_state: entries read, launches
    atomicAdd(stat, (unsigned long long)(n > (unsigned)cap ? (unsigned)cap : n));
    if (agent == 0) atomicAdd(stat + 1, 1ull);
  }
  char          *base  = grid + (size_t)agent * agent_bytes;
  const vfloat4  z     = {0.f, 0.f, 0.f, 0.f};
  const size_t   tid   = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
  if (n > (unsigned)cap) {
    // dense fall-back for this agent: 16-byte stores over the aligned body, bytes at the two ends
    char  *lo = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(base) + 15) & ~(uintptr_t)15);
    char  *hi = reinterpret_cast<char *>(reinterpret_cast<uintptr_t>(base + agent_bytes) & ~(uintptr_t)15);
    if (hi < lo) hi = lo = base + agent_bytes;
    const size_t nv = (size_t)(hi - lo) / 16;
    for (size_t i = tid; i < nv; i += nthr) __builtin_nontemporal_store(z, reinterpret_cast<vfloat4 *>(lo) + i);
    if (tid == 0) {
      for (char *q = base; q < lo && q < base + agent_bytes; ++q) *q = 0;
      for (char *q = hi; q < base + agent_bytes; ++q) *q = 0;
    }
    return;
  }
  const unsigned *e       = entries + (size_t)agent * cap;
  unsigned        n_lines = 0;  // lines this lane group zeroed (counted on the group's first lane)
  const int       part    = (int)(threadIdx.x % LANES);
  const bool      first   = (threadIdx.x & 63) < LANES;  // the wave's first entry has no predecessor to compare with
  const bool      aligned = (reinterpret_cast<uintptr_t>(base) & (16 * LANES - 1)) == 0;
  // UNROLL entries per trip, their loads issued together (a trip is otherwise one dependent load -> store pair)
  const size_t  stride = nthr / LANES;
  for (size_t i0 = tid / LANES; i0 < n; i0 += UNROLL * stride) {
    unsigned sct[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) sct[u] = i0 + u * stride < n ? e[i0 + u * stride] : 0xFFFFFFFFu;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const unsigned id   = LANES == 4 ? sct[u] >> 1 : sct[u];  // the 16*LANES-byte line this entry zeroes
      const unsigned prev = __shfl_up(id, LANES);               // (lanes below an active lane are active: smaller i0)
      if (sct[u] == 0xFFFFFFFFu || (!first && prev == id)) continue;
      if (part == 0) ++n_lines;
      const size_t off = (size_t)id * (16 * LANES) + 16 * part;
      if (aligned) {
        if (off + 16 <= agent_bytes) *reinterpret_cast<vfloat4 *>(base + off) = z;
        else if (off < agent_bytes)  // a short last sector
          for (size_t b = off; b + 2 <= agent_bytes; b += 2) *reinterpret_cast<unsigned short *>(base + b) = 0;
      } else if (part == 0) {  // odd grid sizes: the agent's base is only cell-aligned
        const size_t o32 = (size_t)sct[u] * 32;
        const size_t end = o32 + 32 <= agent_bytes ? o32 + 32 : agent_bytes;
        for (size_t b = o32; b + 2 <= end; b += 2) *reinterpret_cast<unsigned short *>(base + b) = 0;
      }
    }
  }
  // statistics: the 16 * LANES-byte lines zeroed (what the launch wrote), one atomic per wave
  for (int d = 32; d >= 1; d >>= 1) n_lines += (unsigned)__shfl_xor((int)n_lines, d, 64);
  if ((threadIdx.x & 63) == 0 && n_lines) atomicAdd(stat + 2, (unsigned long long)n_lines * (unsigned)(16 * LANES));
}
template <bool POLITE>
__global__ __launch_bounds__(256) void k_clear_chunks(vfloat4 *__restrict__ p, size_t n_vec4,
                                                      float *__restrict__ tail, int n_tail,
                                                      unsigned long long *__restrict__ cursor,
                                                      unsigned long long *__restrict__ next_cursor,
                                                      const int *__restrict__ epoch_word, int epoch, int bound) {
  __shared__ unsigned long long s_next;
  // two cursors take turns: the narrow launch of a clear zeroes the one the NEXT clear will use (the clear that used
  // it last is complete — both of its launches are ordered before this one on the side stream); no memset node
  if (POLITE && blockIdx.x == 0 && threadIdx.x == 0) *next_cursor = 0ull;
  const size_t nchunks = (n_vec4 + CLEAR_CHUNK_V4 - 1) / CLEAR_CHUNK_V4;
  // the wide launch only streams while the replan it was opened for is in flight (*epoch_word == epoch): once the
  // next update starts (word reset) its workgroups take no further chunk and the narrow launch finishes alone
  auto take = [&]() -> unsigned long long {
    if (!POLITE && __hip_atomic_load(epoch_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) return ~0ull;
    return atomicAdd(cursor, 1ull);
  };
  if (threadIdx.x == 0) s_next = take();
  __syncthreads();
  unsigned long long cur = s_next;
  while (cur < nchunks) {
    __syncthreads();  // everybody holds `cur`
    unsigned long long nxt = 0;
    if (threadIdx.x == 0) nxt = take();  // in flight under the stores below
    const size_t b = (size_t)cur * CLEAR_CHUNK_V4;
    const size_t e = b + CLEAR_CHUNK_V4 < n_vec4 ? b + CLEAR_CHUNK_V4 : n_vec4;
    size_t       i = b + threadIdx.x;
    for (; i + 768 < e; i += 1024) {
      clear_store<true>(p + i);
      clear_store<true>(p + i + 256);
      clear_store<true>(p + i + 512);
      clear_store<true>(p + i + 768);
      if (POLITE) __builtin_amdgcn_s_waitcnt(0x0F75);  // vmcnt <= 5: four stores (+ the cursor's atomic on lane 0)
      else if (bound == 8) __builtin_amdgcn_s_waitcnt(0x0F78);
      else if (bound == 12) __builtin_amdgcn_s_waitcnt(0x0F7C);
      else if (bound == 16) __builtin_amdgcn_s_waitcnt(0x4F70);
      else if (bound == 24) __builtin_amdgcn_s_waitcnt(0x4F78);
      else if (bound == 32) __builtin_amdgcn_s_waitcnt(0x8F70);
    }
    for (; i < e; i += 256) clear_store<true>(p + i);
    if (threadIdx.x == 0) s_next = nxt;
    __syncthreads();
    cur = s_next;
  }
  if (POLITE && blockIdx.x == 0 && (int)threadIdx.x < n_tail) tail[threadIdx.x] = 0.f;
}

static int launch_clear_impl(sogm_ctx *c, hipStream_t st, float *grid, bool polite, int part, size_t split);
// ---- sparse reset: logs per pool slot --------------------------------------------------------------------
// the log of a slot, allocated on first use; {nullptr, ...} when the feature is off or there is no room for it (the
// slot then stays untracked and is cleared densely)
MarkLog mark_log(sogm_ctx *c, int slot) {
  MarkLog none{nullptr, nullptr, 0, nullptr};
  if (!c->sparse || slot < 0) return none;
  GridSlot &g = c->pool.slot[slot];
  if (!g.log) {
    Resources::Setup setup(c->res);
    // (The counters' first zeroing is COMPLETE when this returns: the memset is a null-stream operation, which the
    //  library's non-blocking streams do not wait for — with a second context busy on the device it was seen to run
    //  after the first stamp had appended its entries, i.e. it threw them away, and the slot's first reset through
    //  its log left that stamp's marks in the grid.  Only the null stream is synchronised: persistent kernels of a
    //  replan in flight on other streams are not waited for.)
    if (c->res.device(&g.log, sizeof(unsigned) * (size_t)c->log_cap * c->n_agents) != hipSuccess ||
        c->res.device(&g.log_n, sizeof(unsigned) * (size_t)c->n_agents, true) != hipSuccess ||
        (!c->d_reset_stat && c->res.device(&c->d_reset_stat, 8 * sizeof(unsigned long long), true) != hipSuccess) ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
      (void)hipGetLastError();
      c->sparse = 0;  // no room: dense clears from here on
      c->pool.untrack_all();
      return none;
    }
    setup.done();
    g.tracked = 0;  // what the grid holds now was written without a log
  }
  return MarkLog{g.log, g.log_n, c->log_cap, c->d_reset_stat ? c->d_reset_stat + 4 : nullptr};
}
static size_t agent_grid_bytes(const sogm_ctx *c) { return (size_t)c->spec.T * (size_t)c->geom.V * c->cell_bytes(); }

int reset_slot(sogm_ctx *c, hipStream_t st, int slot, float *grid, bool polite) {
  if (c->pool.loggable(slot)) {
    const MarkLog lg = mark_log(c, slot);
    const int wgs = c->tune_i(SOGM_TUNE_RESET_WGS) > 0 ? c->tune_i(SOGM_TUNE_RESET_WGS) : 32;  // workgroups per agent
    // under the replan (polite: beside the QP stage, few CUs free) two lanes and 32-byte lines are faster - 1.05 ms
    // against 1.17 for the 64-byte lines, half the write traffic; with the machine to itself (reset in the update's
    // own stream) four lanes x eight entries per trip - 0.75 ms against 0.91.  Both switches are tuning aids.
    const int lanes_env = c->tune_i(SOGM_TUNE_RESET_LANES), unroll_env = c->tune_i(SOGM_TUNE_RESET_UNROLL);
    const int lanes  = lanes_env == 2 || lanes_env == 4 ? lanes_env : polite ? 2 : 4;
    const int unroll = unroll_env == 1 || unroll_env == 8 ? unroll_env : polite ? 1 : 8;
    prof_begin(c, SOGM_PROF_CLEAR, st);
    auto *kern = lanes == 4 ? (unroll == 1 ? k_reset_sectors<4, 1> : k_reset_sectors<4, 8>)
                            : (unroll == 1 ? k_reset_sectors<2, 1> : k_reset_sectors<2, 8>);
    hipLaunchKernelGGL(kern, dim3(wgs, c->n_agents), dim3(256), 0, st, reinterpret_cast<char *>(grid),
                       agent_grid_bytes(c), lg.entries, lg.n, lg.cap, c->d_reset_stat);
    prof_end(c, SOGM_PROF_CLEAR, st);
    SOGM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_zero_words, dim3((c->n_agents + 255) / 256), dim3(256), 0, st, lg.n, c->n_agents);
    SOGM_HIP_CHECK(hipGetLastError());
    c->pool.slot[slot].n_sparse++;
    return SOGM_OK;
  }
  return launch_clear(c, st, grid, polite);  // (a complete dense clear restarts the slot's log, see launch_clear)
}

// a new tick: wide clear workgroups opened for the replan that just ended retire (the stamp, the searches and the
// corridor stage want the memory pipeline responsive), the narrow launch goes on.  (Only when a dense clear was
// queued since the last update: sparse resets have no wide launch.)  Behind the side stream's work of that replan: its
// gate kernels compare the word with their epoch.
int retire_wide_clear(sogm_ctx *c, hipStream_t st) {
  if (c->overlap >= 2 && c->clear_gate && c->wide_clear_pending) {
    hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, st, c->clear_epoch_word, 0);
    SOGM_HIP_CHECK(hipGetLastError());
    c->wide_clear_pending = 0;
  }
  return SOGM_OK;
}

int adopt_preclear(sogm_ctx *c, hipStream_t st, bool join) {
  if (join)  // (sogm_update_prestamped joins behind its overlay instead, and retires the wide clear there)
    if (int rc = join_prestamp(c, st)) return rc;
  if (!c->pool.precleared()) return SOGM_OK;
  if (c->overlap >= 2) {
    const int nxt = c->pool.adopt_front();
    sync_grid(c);
    SOGM_HIP_CHECK(hipStreamWaitEvent(st, c->pool.slot[nxt].cleared, 0));
    const int early = c->tune_i(SOGM_TUNE_CLEAR_EARLY);
    if (join)
      if (int rc = retire_wide_clear(c, st)) return rc;
    if (c->clear_gate && early) {
      // tuning aid (clear_early = 1): queue the clear of the swapped-out grid NOW, under the stamp — its readers,
      // the previous replan's kernels, are complete on `st` in stream order — for the replan that will announce
      // epoch clear_epoch + 1.  Measured: the stamp beside it takes twice as long (1.4 -> 3.1 ms) and the first
      // ticks of a flight lose 5 %; later ticks gain 3 %.  Off by default.
      return queue_spare_clears_ahead(c, st);
    }
    return SOGM_OK;
  }
  SOGM_HIP_CHECK(hipStreamWaitEvent(st, c->ev_cleared, 0));
  c->pool.forget_preclear();
  return SOGM_OK;
}

// modes 2 / 3: queue the clear of every dirty spare grid on the side stream once `after` has fired (every reader
// of those grids is ordered before it); sogm_replan calls this right after its fan-out event
int queue_spare_clears(sogm_ctx *c, hipEvent_t after) {
  if (c->overlap < 2 || c->pool.first_dirty() < 0) return SOGM_OK;
  SOGM_HIP_CHECK(hipStreamWaitEvent(c->side, after, 0));
  // The clear shares the machine with the whole replan, as ONE narrow launch by default.  clear_head_gb (a
  // tuning aid) splits it into a narrow head of that many GB and a full-width rest: measured with the dataflow
  // replan (profiles/r02_*), a wide rest shortens the clear (15.9 -> 14.3 ms) but costs the planner kernels more
  // than it saves (tick 18.2 -> 19.3 ms), because per-agent chaining spreads the global-memory phases (searches,
  // point scans, FIRI set-up of late agents) over the whole tick.
  const double head_gb = c->tune[SOGM_TUNE_CLEAR_HEAD_GB] >= 0 ? c->tune[SOGM_TUNE_CLEAR_HEAD_GB] : 1.0e9;
  const size_t total = clear_vec4_total(c);
  size_t       head  = (size_t)(head_gb * 1e9 / 16.0);
  if (head > total) head = total;
  for (int g; (g = c->pool.first_dirty()) >= 0;) {
    float *grid = c->pool.slot[g].grid;
    int    rc   = SOGM_OK;
    if (c->pool.loggable(g)) {
      // The reset is held back until every agent's corridors are final (the gate the dense clear's wide launch
      // uses): beside the searches and the corridor stage's point scans its 3 GB of scattered stores cost the
      // chain 0.8 ms (tick 13.8 -> 12.9 ms); under the QP stage, which lives in LDS, they cost nothing and the
      // reset itself takes 1.3 instead of 2.4 ms.  reset_late = 0: start it with the replan.
      const int late = c->tune_i(SOGM_TUNE_RESET_LATE);
      if (late && c->clear_gate) {
        if (c->gate_frac_agents > 0 && c->gate_frac_agents < c->clear_gate_target && !c->gate_frac_valid) {
          // the pre-stamp may start when this share of the agents' corridors is final (tuning key prestamp_gate_frac):
          // the same gate kernel with a lower target, on THIS stream (which spins for the full gate anyway), and an
          // event for the pre-stamp's stream — no spinning kernel at the head of a second stream
          hipLaunchKernelGGL(k_clear_gate, dim3(1), dim3(64), 0, c->side, c->clear_cursor, ~(size_t)0, c->clear_gate,
                             c->clear_gate_err, c->gate_frac_agents, c->clear_epoch_word, c->clear_epoch);
          SOGM_HIP_CHECK(hipGetLastError());
          SOGM_HIP_CHECK(hipEventRecord(c->ev_gate_frac, c->side));
          c->gate_frac_valid = 1;
        }
        hipLaunchKernelGGL(k_clear_gate, dim3(1), dim3(64), 0, c->side, c->clear_cursor, ~(size_t)0, c->clear_gate,
                           c->clear_gate_err, c->clear_gate_target, c->clear_epoch_word, c->clear_epoch);
        SOGM_HIP_CHECK(hipGetLastError());
        // "every agent's corridors are final" as an EVENT for the pre-stamp's stream (sogm_replan): no second gate kernel
        // spinning at the head of a stream (with shared or oversubscribed hardware queues every spinner is a hazard)
        SOGM_HIP_CHECK(hipEventRecord(c->ev_gate_open, c->side));
        c->gate_open_valid = 1;
      }
      rc = reset_slot(c, c->side, g, grid, true);  // the logged sectors only: a fraction of a millisecond
    } else if (head == 0) {
      rc = launch_clear(c, c->side, grid, false);
    } else if (head >= total) {
      rc = launch_clear(c, c->side, grid, true);
    } else {
      rc = launch_clear(c, c->side, grid, true, 1, head);
      if (!rc) rc = launch_clear(c, c->side, grid, false, 2, head);
    }
    if (rc) return rc;
    SOGM_HIP_CHECK(hipEventRecord(c->pool.slot[g].cleared, c->side));
    c->pool.queue_ready(g);
  }
  return SOGM_OK;
}

// polite = the clear shares the machine with latency-bound kernels that read global memory (double-buffered
// mode): a full-width clear (2048 persistent workgroups, unbounded stores in flight) starves every other
// kernel's loads for its whole duration; 64 workgroups with <= 4 stores in flight per wave still stream at
// ~5.7 TB/s and leave the memory pipeline responsive.  SOGM_CLEAR_WGS / SOGM_CLEAR_THROTTLE / SOGM_CLEAR_NT
// override the choice (tuning aids: clear_wgs / clear_throttle / clear_nt).
// ... behind what `st` holds now, for the replan that will announce epoch clear_epoch + 1 (tuning aid clear_early)
int queue_spare_clears_ahead(sogm_ctx *c, hipStream_t st) {
  c->clear_epoch_ahead = 1;
  SOGM_HIP_CHECK(hipEventRecord(c->ev_grid_free, st));
  const int rc         = queue_spare_clears(c, c->ev_grid_free);
  c->clear_epoch_ahead = 0;
  return rc;
}
size_t clear_vec4_total(const sogm_ctx *c) {
  return (size_t)c->n_agents * c->spec.T * (size_t)c->geom.V * c->cell_bytes() / 4 / 4;
}
// part: 0 = the whole grid, 1 = the first `split` 16-byte elements, 2 = everything from `split` on
int launch_clear(sogm_ctx *c, hipStream_t st, float *grid, bool polite, int part, size_t split) {
  if (!grid) grid = c->d_grid;
  const int rc = launch_clear_impl(c, st, grid, polite, part, split);
  if (rc == SOGM_OK && part != 1) {
    // this launch completes a dense clear of the slot: behind it (stream order) the slot's mark log starts empty and
    // covers every non-zero cell again
    const int     slot = c->pool.slot_of(grid);
    const MarkLog lg   = mark_log(c, slot);
    if (slot >= 0) c->pool.slot[slot].n_dense++;
    if (lg.entries) {
      hipLaunchKernelGGL(k_zero_words, dim3((c->n_agents + 255) / 256), dim3(256), 0, st, lg.n, c->n_agents);
      c->pool.slot[slot].tracked = hipGetLastError() == hipSuccess ? 1 : 0;
    }
  }
  return rc;
}
static int launch_clear_impl(sogm_ctx *c, hipStream_t st, float *grid, bool polite, int part, size_t split) {
  // the clear is a byte stream: n = number of 4-byte words of the grid (fp16 grids: 2 cells per word)
  // (rounded up: an odd number of fp16 cells ends in half a word; allocations are padded to 16 B)
  const size_t n     = ((size_t)c->n_agents * c->spec.T * (size_t)c->geom.V * c->cell_bytes() + 3) / 4;
  const size_t nall  = n / 4;
  const size_t first = part == 2 ? split : 0;
  const size_t nv4   = part == 1 ? split : nall - first;
  const int    tail  = part == 1 ? 0 : (int)(n - nall * 4);
  const int    slot  = part == 1 ? SOGM_PROF_CLEAR_HEAD : SOGM_PROF_CLEAR;
  size_t       want  = (nv4 + 255) / 256;
  const int env_wgs = c->tune_i(SOGM_TUNE_CLEAR_WGS) > 0 ? c->tune_i(SOGM_TUNE_CLEAR_WGS) : 0;
  const int env_throttle = c->tune_i(SOGM_TUNE_CLEAR_THROTTLE), nt = c->tune_i(SOGM_TUNE_CLEAR_NT) != 0;
  const size_t max_wgs  = env_wgs ? (size_t)env_wgs : (polite ? (c->clear_gate && part == 0 ? 80 : 64) : 2048);
  const int    throttle = env_wgs ? env_throttle : (polite ? 4 : 0);
  const int    nblk     = (int)(want < 1 ? 1 : (want > max_wgs ? max_wgs : want));
  // clear_wide_wgs = 0 switches the adaptive width off; clear_wide_bound: stores in flight per wave of the wide launch
  const int wide_wgs = c->tune_i(SOGM_TUNE_CLEAR_WIDE_WGS), wide_bound = c->tune_i(SOGM_TUNE_CLEAR_WIDE_BOUND);
  // The wide part belongs to the dense-clear mode, where a whole grid is cleared under every replan.  With the sparse reset on,
  // a dense clear happens once per grid (first use) or behind a dense writer: it stays one narrow launch on `st`, and the
  // context holds no stream for a second one.
  if (polite && part == 0 && c->clear_gate && c->clear_cursor && !c->sparse && wide_wgs > 0 && nt) {
    if (!c->side2) {  // the wide part's stream, at its first launch
      Resources::Setup setup(c->res);
      SOGM_HIP_CHECK(c->res.stream(&c->side2));
      setup.done();
    }
    const size_t        nchunks = (nall + CLEAR_CHUNK_V4 - 1) / CLEAR_CHUNK_V4;
    unsigned long long *cur = c->clear_cursor + (c->clear_seq & 1), *nxt = c->clear_cursor + ((c->clear_seq + 1) & 1);
    ++c->clear_seq;
    SOGM_HIP_CHECK(hipEventRecord(c->ev_side2_go, st));
    SOGM_HIP_CHECK(hipStreamWaitEvent(c->side2, c->ev_side2_go, 0));
    prof_begin(c, slot, st);
    const int epoch = c->clear_epoch + c->clear_epoch_ahead;
    c->wide_clear_pending = 1;
    hipLaunchKernelGGL(k_clear_chunks<true>, dim3(nblk), dim3(256), 0, st, (vfloat4 *)grid, nall, grid + nall * 4,
                       tail, cur, nxt, c->clear_epoch_word, epoch, 0);
    hipLaunchKernelGGL(k_clear_gate, dim3(1), dim3(64), 0, c->side2, cur, nchunks, c->clear_gate,
                       c->clear_gate_err, c->clear_gate_target, c->clear_epoch_word, epoch);
    hipLaunchKernelGGL(k_clear_chunks<false>, dim3(wide_wgs), dim3(256), 0, c->side2, (vfloat4 *)grid, nall,
                       grid + nall * 4, 0, cur, nxt, c->clear_epoch_word, epoch, wide_bound);
    SOGM_HIP_CHECK(hipEventRecord(c->ev_side2_done, c->side2));
    SOGM_HIP_CHECK(hipStreamWaitEvent(st, c->ev_side2_done, 0));  // the clear is complete when both launches are
    prof_end(c, slot, st);
    SOGM_HIP_CHECK(hipGetLastError());
    return SOGM_OK;
  }
  prof_begin(c, slot, st);
  if (nt)
    hipLaunchKernelGGL(k_clear_slabs<true>, dim3(nblk), dim3(256), 0, st, (vfloat4 *)grid + first, nv4,
                       grid + nall * 4, tail, throttle);
  else
    hipLaunchKernelGGL(k_clear_slabs<false>, dim3(nblk), dim3(256), 0, st, (vfloat4 *)grid + first, nv4,
                       grid + nall * 4, tail, throttle);
  prof_end(c, slot, st);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

int next_clear_epoch(sogm_ctx *c) {
  if (++c->clear_epoch <= 0) c->clear_epoch = 1;  // 0 = "no replan in flight"
  return c->clear_epoch;
}
int announce_clear_epoch(sogm_ctx *c, hipStream_t st) {
  next_clear_epoch(c);
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, st, c->clear_epoch_word, c->clear_epoch);
  SOGM_HIP_CHECK(hipGetLastError());
  return SOGM_OK;
}

}  // namespace sogm

using namespace sogm;

// diagnostics (bench.py, tools/): how many DISTINCT 32-byte sectors the current grid's mark log names.  The log holds one entry
// per mark the wave-local lookback could not merge (sogm_map.hip, stamp_marks_trips) — marks of different waves in one sector
// are logged once each, the reset zeroes such a sector more than once and the stores merge in the L2 — so "4 B x entries +
// 32 B x entries" over-counts what HBM moves; 4 B x entries + 32 B x DISTINCT sectors is the honest denominator.  A
// test-and-set over a throw-away bitmap (one bit per sector and agent), outside any timed region: a returning atomic per
// entry at 25-30 G/s would cost the stamp more than the duplicates cost the reset.
__global__ __launch_bounds__(256) void k_log_distinct(sogm::MarkLog lg, int n_agents, unsigned *bitmap, size_t words_per_agent,
                                                      unsigned long long *out) {
  const int agent = blockIdx.y;
  if (agent >= n_agents) return;
  const unsigned  n = lg.n[agent] > (unsigned)lg.cap ? (unsigned)lg.cap : lg.n[agent];
  const unsigned *e = lg.entries + (size_t)agent * lg.cap;
  unsigned       *bm = bitmap + (size_t)agent * words_per_agent;
  unsigned long long ent = 0, dis = 0, near8 = 0, near63 = 0, near1k = 0;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const unsigned sec = e[i];
    if (sec == 0xFFFFFFFFu || (size_t)(sec >> 5) >= words_per_agent) continue;
    ++ent;
    const unsigned bit = 1u << (sec & 31);
    if (!(atomicOr(bm + (sec >> 5), bit) & bit)) ++dis;
    // where the duplicates sit: an equal entry among the previous 8 / 63 / 1023 positions of the log (a wave appends its
    // entries as one block: "within 63" ~ what a wave-wide de-duplication could remove, "within 1023" a workgroup-wide one)
    bool d8 = false, d63 = false, d1k = false;
    for (unsigned b = 1; b <= 1023 && b <= i; ++b)
      if (e[i - b] == sec) {
        d1k = true;
        if (b <= 63) d63 = true;
        if (b <= 8) d8 = true;
        break;
      }
    near8 += d8, near63 += d63, near1k += d1k;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    ent += __shfl_xor(ent, d, 64);
    dis += __shfl_xor(dis, d, 64);
    near8 += __shfl_xor(near8, d, 64);
    near63 += __shfl_xor(near63, d, 64);
    near1k += __shfl_xor(near1k, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && ent) {
    atomicAdd(out, ent);
    atomicAdd(out + 1, dis);
    atomicAdd(out + 3, near8);
    atomicAdd(out + 4, near63);
    atomicAdd(out + 5, near1k);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && lg.n[agent] > (unsigned)lg.cap) atomicAdd(out + 2, 1ull);
}

extern "C" {

int sogm_set_overlap_clear(sogm_ctx *c, int mode) {
  if (!c || mode < 0 || mode > 3) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  if (c->update_pending) {
    (void)hipDeviceSynchronize();
    c->update_pending = 0;
  }
  if (c->pool.precleared() || c->pool.n_slots() > 1) {
    // pre-clears may be in flight: let them finish and forget them (the next update clears its grid itself)
    (void)hipDeviceSynchronize();
  }
  // the current grid stays the current grid (slot 0 from here on); spares are added / released around it
  const sogm::GridPool::Change ch = c->pool.rebuild(mode >= 2 ? mode : 1);
  for (int i = ch.release_to; i-- > ch.release_from;) c->res.release(&c->pool.slot[i].grid);
  const size_t bytes = ((size_t)sogm_grid_bytes(c) + 15) & ~(size_t)15;
  {
    sogm::Resources::Setup setup(c->res);  // all or nothing: the mode is unchanged when a spare or an event cannot be had
    hipError_t e = hipSuccess;
    bool       grid = false;
    for (int i = ch.acquire_from; i < ch.acquire_to && e == hipSuccess; ++i)
      grid = (e = c->res.device(&c->pool.slot[i].grid, bytes)) != hipSuccess;
    for (int i = 0; i < ch.acquire_to && e == hipSuccess; ++i)  // every slot takes the spare role in turn
      if (!c->pool.slot[i].cleared) e = c->res.event(&c->pool.slot[i].cleared);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      sogm::set_error(grid ? "sogm_set_overlap_clear: no room for the spare grid(s)" : "sogm_set_overlap_clear: event", e);
      return grid ? SOGM_ERR_CAPACITY : SOGM_ERR_HIP;
    }
    setup.done();
    c->pool.acquired(ch);
  }
  c->overlap = mode;
  return SOGM_OK;
}

int sogm_set_sparse_reset(sogm_ctx *c, int enable, int log_capacity) {
  if (!c || log_capacity < 0) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());  // resets / writers in flight use the logs
  for (sogm::GridSlot &g : c->pool.slot) {
    c->res.release(&g.log);
    c->res.release(&g.log_n);
  }
  c->pool.untrack_all();  // contents unknown to the (new) logs: each slot's next reset is dense
  c->sparse = enable ? 1 : 0;
  if (log_capacity > 0) c->log_cap = log_capacity;
  return SOGM_OK;
}

int sogm_sparse_reset_state(sogm_ctx *c, int32_t *out) {
  if (!c || !out) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  const sogm::GridSlot &cur = c->pool.slot[c->pool.current()];
  auto clamp31 = [](unsigned long long v) { return (int32_t)(v > 0x7FFFFFFFull ? 0x7FFFFFFFull : v); };
  out[0] = c->sparse;
  out[1] = c->log_cap;
  out[2] = cur.tracked;
  out[3] = 0;  // largest per-agent entry count of the current grid's log
  out[4] = 0;  // entries of all agents (what the grid's next reset reads; capped at the capacity per agent)
  if (c->sparse && cur.log_n) {
    std::vector<unsigned> n((size_t)c->n_agents);
    SOGM_HIP_CHECK(hipMemcpy(n.data(), cur.log_n, sizeof(unsigned) * n.size(), hipMemcpyDeviceToHost));
    unsigned           mx  = 0;
    unsigned long long tot = 0;
    for (unsigned v : n) {
      mx = v > mx ? v : mx;
      tot += v > (unsigned)c->log_cap ? (unsigned)c->log_cap : v;
    }
    out[3] = clamp31(mx);
    out[4] = clamp31(tot);
  }
  out[5] = out[6] = out[7] = 0;  // sparse resets since the previous call: launches, entries read and KiB zeroed per launch (means)
  if (c->d_reset_stat) {
    unsigned long long st[4] = {0, 0, 0, 0};
    SOGM_HIP_CHECK(hipMemcpy(st, c->d_reset_stat, sizeof(st), hipMemcpyDeviceToHost));
    SOGM_HIP_CHECK(hipMemset(c->d_reset_stat, 0, sizeof(st)));  // (the reset's counters only: the stamp's stay)
    out[5] = clamp31(st[1]);
    out[6] = clamp31(st[1] ? st[0] / st[1] : 0);
    out[7] = clamp31(st[1] ? st[2] / st[1] / 1024 : 0);
  }
  return SOGM_OK;
}

int sogm_grid_history(sogm_ctx *c, int32_t *out) {
  if (!c || !out) return SOGM_ERR_INVALID_ARG;
  const int slot = c->pool.current();
  out[0] = slot;
  out[1] = c->pool.slot[slot].n_sparse;
  out[2] = c->pool.slot[slot].n_dense;
  out[3] = c->pool.current_prestamped();
  return SOGM_OK;
}

int sogm_map_traffic(sogm_ctx *c, int64_t *out, int reset) {
  if (!c || !out) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c->d_reset_stat) SOGM_HIP_CHECK(hipMemcpy(st, c->d_reset_stat, sizeof(st), hipMemcpyDeviceToHost));
  out[0] = (int64_t)st[1];  // resets through the mark logs
  out[1] = (int64_t)st[0];  // log entries they read
  out[2] = (int64_t)st[2];  // bytes they zeroed
  out[3] = (int64_t)c->n_stamps;
  out[4] = (int64_t)st[4];  // marks (cells set to 1) the stamps wrote
  out[5] = (int64_t)st[5];  // log entries the stamps appended
  if (reset) {
    if (c->d_reset_stat) SOGM_HIP_CHECK(hipMemset(c->d_reset_stat, 0, sizeof(st)));
    c->n_stamps = 0;
  }
  return SOGM_OK;
}

// host out[6] = {valid entries of the current grid's mark logs (all agents), distinct sectors among them, agents whose log
// overflowed (their reset is dense: not counted), entries with an equal entry among the previous 8 / 63 / 1023 log positions}.
// Synchronises; allocates and frees V T / 64 bytes per agent.
int sogm_debug_log_distinct(sogm_ctx *c, unsigned long long *out3_host) {
  if (!c || !out3_host) return SOGM_ERR_INVALID_ARG;
  SOGM_HIP_CHECK(hipSetDevice(c->device));
  SOGM_HIP_CHECK(hipDeviceSynchronize());
  const int slot = c->pool.current();
  for (int i = 0; i < 6; ++i) out3_host[i] = 0;
  if (!c->pool.loggable(slot)) return SOGM_ERR_STATE;
  const sogm::MarkLog lg = sogm::mark_log(c, slot);
  const size_t cells_per_sector = 32 / c->cell_bytes();
  const size_t sectors = ((size_t)c->spec.T * (size_t)c->geom.V + cells_per_sector - 1) / cells_per_sector;
  const size_t words   = (sectors + 31) / 32;
  unsigned           *bm = nullptr;
  unsigned long long *d  = nullptr;
  SOGM_HIP_CHECK(hipMalloc((void **)&bm, sizeof(unsigned) * words * (size_t)c->n_agents));
  hipError_t e = hipMalloc((void **)&d, 6 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(bm, 0, sizeof(unsigned) * words * (size_t)c->n_agents);
  if (e == hipSuccess) e = hipMemset(d, 0, 6 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_log_distinct, dim3(64, c->n_agents), dim3(256), 0, nullptr, lg, c->n_agents, bm, words, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out3_host, d, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(bm);
  if (d) (void)hipFree(d);
  SOGM_HIP_CHECK(e);
  return SOGM_OK;
}

}  // extern "C"
