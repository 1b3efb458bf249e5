// The pool of 1 to 3 SOGM grids a context rotates through, as one value (host-only bookkeeping: HIP supplies the handle
// types, nothing here calls it).  Allocation, events, streams and launches are sogm_clear.hip's, through sogm_ctx::res;
// every other file uses the operations, never the fields.
// Tick pipelining (sogm_set_overlap_clear): modes 0 / 1 keep one grid, modes 2 / 3 a pool of 2 / 3.  Every slot is in
// exactly one place: it is the current grid, or in `ready` — spares whose reset has been queued on the side stream (FIFO;
// the next update adopts the front one after waiting for its event) — or in `dirty` — spares that still hold an old map
// (the next sogm_replan queues their reset).  Mode 1 resets the one grid in place behind ev_cleared.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace sogm {
// Everything that belongs to one grid, so that reordering slots is one std::swap.
// Sparse reset: the reference rebuilds the map from zero at every update (fake_particle_risk_voxel.cpp:107-108: a fill
// over all V x T cells); here every mark written into a grid since its last reset is logged as the index of its 32-byte
// sector (per agent), and the reset zeroes exactly those sectors — the cells of the rebuilt map are the same, the 640 MB
// per agent of zero stores are not issued.  A log that overflows makes the reset kernel zero that agent's whole grid.
struct GridSlot {
  float     *grid;     // [A][T][V] cells (fp32, or __half when geom.half)
  hipEvent_t cleared;  // recorded on the side stream behind the slot's queued reset
  unsigned  *log;      // [A][log_cap] sectors marked since the slot's last reset, lazy (mark_log)
  unsigned  *log_n;    // [A] entries appended since then (beyond log_cap: overflow)
  int        tracked;  // every non-zero cell is covered by the log (false after dense writers — sogm_set_future_risk,
                       // sogm_dsp_publish, sogm_grid_ptr — and for a fresh allocation: the next reset is the dense clear)
  int n_sparse, n_dense;  // since the pool was (re)built: resets through the log, dense clears (host-side launch counts;
                          // sogm_grid_history: a parity test asserts that its grid went through k_reset_sectors)
};

struct GridPool {
  GridSlot slot[3] = {};
  int      n = 1, cur = 0;  // slots in use (sogm_create files its grid as slot 0), the current one
  int      ready[2] = {}, n_ready = 0;
  int      dirty[2] = {}, n_dirty = 0;
  int      preclear       = 0;   // the next update finds a (being-)cleared grid: mode 1 in place, modes 2 / 3 n_ready > 0
  int      prestamp_slot  = -1;  // the slot a replan is building the next tick's map into (sogm_planner_set_prestamp)
  int      cur_prestamped = 0;   // the CURRENT grid was built by a replan's pre-stamp (sogm_grid_history; sogm_replan
                                 // orders its reset behind such a grid's overlay)

  int        n_slots() const { return n; }
  int        current() const { return cur; }
  float     *grid() const { return slot[cur].grid; }
  float     *grid_of(int s) const { return slot[s].grid; }
  hipEvent_t cleared_event(int s) const { return slot[s].cleared; }
  int        slot_of(const float *g) const {  // -1: not a grid of this pool
    for (int i = 0; i < n; ++i)
      if (slot[i].grid == g) return i;
    return -1;
  }
  // the slot can be reset through its log (tracked is only ever set on a slot that has a log, and untrack_all()
  // accompanies every switch-off of the sparse reset)
  bool loggable(int s) const { return slot[s].tracked && slot[s].log; }
  // a dense writer touched the current grid: its log no longer covers it, and it is not the pre-stamp's work any more
  void dense_write_current() { slot[cur].tracked = cur_prestamped = 0; }
  void untrack_all() { slot[0].tracked = slot[1].tracked = slot[2].tracked = 0; }

  bool precleared() const { return preclear != 0; }
  void cleared_in_place() { preclear = 1; }  // mode 1
  void forget_preclear() { preclear = 0; }   // modes 0 / 1: adopted, or given up after a failed replan
  int  front_ready() const { return n_ready ? ready[0] : -1; }
  int  first_dirty() const { return n_dirty ? dirty[0] : -1; }
  // a dirty spare's reset has been queued (its event recorded): it joins the back of `ready`
  void queue_ready(int s) {
    int k = 0;
    for (int i = 0; i < n_dirty; ++i)
      if (dirty[i] != s) dirty[k++] = dirty[i];
    n_dirty          = k;
    ready[n_ready++] = s;
    preclear         = 1;
  }
  // rotate: the front of `ready` becomes the current grid, the old current grid is dirty
  int adopt_front() {
    const int nxt = ready[0];
    for (int i = 1; i < n_ready; ++i) ready[i - 1] = ready[i];
    n_ready--;
    dirty[n_dirty++] = cur;
    cur              = nxt;
    preclear         = n_ready > 0;
    return nxt;
  }

  // pre-stamp: sogm_update_prestamped adopts the target while it still is the front of `ready`; any other update takes
  // it back as stale (-1: none) and, if that is the grid it adopts, resets it
  void set_prestamp_target(int s) { prestamp_slot = s; }
  void clear_prestamp_target() { prestamp_slot = -1; }
  bool prestamp_pending() const { return prestamp_slot >= 0; }
  bool front_is_prestamped() const { return prestamp_slot >= 0 && front_ready() == prestamp_slot && preclear; }
  int  discard_prestamp() { return cur_prestamped = 0, std::exchange(prestamp_slot, -1); }
  bool current_prestamped() const { return cur_prestamped != 0; }
  void adopted_prestamped() { prestamp_slot = -1, cur_prestamped = 1; }  // behind adopt_front() of the target
  void current_rebuilt() { cur_prestamped = 0; }  // in place, by something that is no pre-stamp (sogm_flight_run)

  // sogm_set_overlap_clear's bookkeeping.  rebuild(want) moves the current grid (with everything of its slot) to slot 0
  // and drops the slots beyond `want`: the caller releases the grids of slots [release_from, release_to), acquires
  // grids for [acquire_from, acquire_to) and an event for every slot below acquire_to that has none, then calls
  // acquired() if all of it succeeded.  Either way ready is empty, dirty is every spare — they hold garbage until a
  // replan clears them — and the spares are untracked with zeroed history; without acquired() that describes the pool
  // as it was (less the released slots).
  struct Change {
    int release_from, release_to, acquire_from, acquire_to;
  };
  Change rebuild(int want) {
    if (cur != 0) std::swap(slot[0], slot[cur]);
    const Change ch{want < n ? want : n, n, want < n ? want : n, want};
    for (int i = 1; i < 3; ++i) slot[i].tracked = slot[i].n_sparse = slot[i].n_dense = 0;
    prestamp_slot = -1;  // (a pre-stamped spare is dirty like the others)
    list_spares(ch.release_from);
    return ch;
  }
  void acquired(const Change &ch) { list_spares(ch.acquire_to); }
  void list_spares(int n_now) {
    n   = n_now;
    cur = n_ready = n_dirty = preclear = 0;
    for (int i = 1; i < n; ++i) dirty[n_dirty++] = i;
  }
};
}  // namespace sogm
