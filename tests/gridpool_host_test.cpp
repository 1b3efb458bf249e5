// Host test of csrc/sogm_gridpool.hpp: the pool's bookkeeping compiled with the host compiler against nothing (the
// header calls no HIP entry point; grids, logs and events are made-up handle values).  Scripted sequences, with the
// pool's invariants checked after every step.
#include "sogm_gridpool.hpp"

#include <cstdint>
#include <cstdio>
#include <deque>

using sogm::GridPool;
using sogm::GridSlot;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// every field of a slot carries the same id
static void tag(GridSlot &s, int id) {
  s.grid    = (float *)(uintptr_t)(0x10000 * id);
  s.cleared = (hipEvent_t)(uintptr_t)(0x10000 * id + 0x100);
  s.log     = (unsigned *)(uintptr_t)(0x10000 * id + 0x200);
  s.log_n   = (unsigned *)(uintptr_t)(0x10000 * id + 0x300);
  s.tracked = s.n_sparse = s.n_dense = id;
}
static bool tagged(const GridSlot &s, int id) {
  GridSlot t{};
  tag(t, id);
  return s.grid == t.grid && s.cleared == t.cleared && s.log == t.log && s.log_n == t.log_n && s.tracked == id &&
         s.n_sparse == id && s.n_dense == id;
}
static int id_of(const GridSlot &s) { return (int)((uintptr_t)s.grid / 0x10000); }

// {current} + ready + dirty is a partition of 0..n-1; with two grids or more, precleared <=> ready is not empty
static int check(const GridPool &p) {
  int seen[3] = {0, 0, 0};
  const int n = p.n_slots();
  EXPECT(n >= 1 && n <= 3);
  EXPECT(p.current() >= 0 && p.current() < n);
  seen[p.current()]++;
  EXPECT(p.n_ready >= 0 && p.n_dirty >= 0 && p.n_ready + p.n_dirty == n - 1);
  for (int i = 0; i < p.n_ready; ++i) {
    EXPECT(p.ready[i] >= 0 && p.ready[i] < n);
    seen[p.ready[i]]++;
  }
  for (int i = 0; i < p.n_dirty; ++i) {
    EXPECT(p.dirty[i] >= 0 && p.dirty[i] < n);
    seen[p.dirty[i]]++;
  }
  for (int i = 0; i < n; ++i) EXPECT(seen[i] == 1);
  EXPECT(p.front_ready() == (p.n_ready ? p.ready[0] : -1));
  EXPECT(p.first_dirty() == (p.n_dirty ? p.dirty[0] : -1));
  if (n >= 2) EXPECT(p.precleared() == (p.n_ready > 0));
  EXPECT(p.grid() == p.slot[p.current()].grid && p.slot_of(p.grid()) == p.current());
  return 0;
}
#define STEP(stmt) \
  do {             \
    stmt;          \
    if (check(p)) return 1; \
  } while (0)

static int next_id = 1;
// what sogm_set_overlap_clear does around rebuild(): release, acquire (or fail to), report
static int resize(GridPool &p, int want, bool acquire_ok) {
  const GridPool::Change ch = p.rebuild(want);
  EXPECT(ch.release_from <= ch.release_to && ch.acquire_from <= ch.acquire_to && ch.acquire_to == want);
  EXPECT(ch.release_from == ch.release_to || ch.acquire_from == ch.acquire_to);  // never both
  for (int i = ch.release_from; i < ch.release_to; ++i) p.slot[i].grid = nullptr;
  if (check(p)) return 1;
  if (!acquire_ok) return 0;
  for (int i = ch.acquire_from; i < ch.acquire_to; ++i) {
    p.slot[i] = GridSlot{};
    p.slot[i].grid = (float *)(uintptr_t)(0x10000 * next_id++);
  }
  for (int i = 0; i < ch.acquire_to; ++i)
    if (!p.slot[i].cleared) p.slot[i].cleared = (hipEvent_t)(uintptr_t)(0x10000 * next_id++ + 0x100);
  p.acquired(ch);
  return check(p);
}
static int fresh(GridPool &p, int n) {  // as sogm_create leaves it, then n grids, every slot tagged
  p = GridPool();
  EXPECT(p.n_slots() == 1 && p.current() == 0 && !p.precleared() && !p.prestamp_pending() && p.front_ready() < 0);
  tag(p.slot[0], next_id++);
  if (check(p)) return 1;
  if (resize(p, n, true)) return 1;
  for (int i = 1; i < n; ++i) tag(p.slot[i], next_id++);
  EXPECT(p.n_slots() == n);
  return check(p);
}
static int tick(GridPool &p) {  // a replan queues every dirty spare's reset, the next update adopts the front
  for (int g; (g = p.first_dirty()) >= 0;) STEP(p.queue_ready(g));
  STEP(p.adopt_front());
  return 0;
}
// after a rebuild: ready empty, dirty = every spare in order, spares untracked with zeroed history
static int spares_fresh(const GridPool &p) {
  EXPECT(p.current() == 0 && p.n_ready == 0 && !p.precleared() && !p.prestamp_pending());
  EXPECT(p.n_dirty == p.n_slots() - 1);
  for (int i = 1; i < p.n_slots(); ++i) EXPECT(p.dirty[i - 1] == i);
  for (int i = 1; i < 3; ++i) EXPECT(!p.slot[i].tracked && !p.slot[i].n_sparse && !p.slot[i].n_dense && !p.loggable(i));
  return 0;
}

int main() {
  GridPool p;
  // 2. adoption is FIFO over 10 ticks with 2 and with 3 grids
  for (int n = 2; n <= 3; ++n) {
    if (fresh(p, n)) return 1;
    std::deque<int> queued;
    for (int k = 0; k < 10; ++k) {
      for (int g; (g = p.first_dirty()) >= 0;) {
        queued.push_back(g);
        STEP(p.queue_ready(g));
        EXPECT(p.precleared());
      }
      EXPECT(p.front_ready() == queued.front());
      const int    old  = p.current();
      const float *want = p.slot[queued.front()].grid;
      int          got  = -1;
      STEP(got = p.adopt_front());
      EXPECT(got == queued.front() && p.current() == got && p.grid() == want);
      queued.pop_front();
      EXPECT(p.n_dirty >= 1 && p.dirty[p.n_dirty - 1] == old);  // the old current grid is dirty
      EXPECT(p.precleared() == !queued.empty());
    }
    EXPECT(n == 2 ? queued.empty() : queued.size() == 1);  // three grids: every reset has a tick of slack
  }
  // 3. rebuild keeps the per-grid state with the current grid, from every current slot, shrinking and growing
  for (int from = 1; from <= 3; ++from)
    for (int cur = 0; cur < from; ++cur)
      for (int want = 1; want <= 3; ++want)
        for (int ok = 0; ok <= 1; ++ok) {
          if (fresh(p, from)) return 1;
          for (int k = 0; k < 6 && p.current() != cur; ++k)
            if (tick(p)) return 1;
          EXPECT(p.current() == cur);
          const int    id   = id_of(p.slot[cur]);
          const float *grid = p.grid();
          EXPECT(tagged(p.slot[cur], id));
          if (from >= 2) {  // something queued and a pre-stamp target: both are forgotten
            for (int g; (g = p.first_dirty()) >= 0;) STEP(p.queue_ready(g));
            STEP(p.set_prestamp_target(p.front_ready()));
          }
          if (resize(p, want, ok != 0)) return 1;
          EXPECT(p.grid() == grid && tagged(p.slot[0], id));  // its own grid, logs, event, tracked and history
          if (spares_fresh(p)) return 1;
          // told that the acquisition failed, the pool is the old one (less what a shrink released)
          EXPECT(p.n_slots() == (ok || want < from ? want : from));
          for (int i = 0; i < p.n_slots(); ++i) EXPECT(p.slot[i].grid != nullptr);
          if (p.n_slots() >= 2) {  // and it goes on rotating
            if (tick(p)) return 1;
            EXPECT(p.current() == 1);
          }
        }
  // 4. dense writers
  if (fresh(p, 3)) return 1;
  if (tick(p)) return 1;
  EXPECT(p.current() == 1 && p.loggable(0) && p.loggable(1) && p.loggable(2));
  STEP(p.adopted_prestamped());
  EXPECT(p.current_prestamped());
  STEP(p.dense_write_current());
  EXPECT(!p.loggable(1) && !p.slot[1].tracked && p.loggable(0) && p.loggable(2) && !p.current_prestamped());
  EXPECT(p.slot[1].log != nullptr);  // (the log stays; the next dense clear restarts it)
  STEP(p.untrack_all());
  EXPECT(!p.loggable(0) && !p.loggable(1) && !p.loggable(2));
  p.slot[0].tracked = 1;
  p.slot[0].log     = nullptr;
  EXPECT(!p.loggable(0));  // tracked without a log is not loggable
  // 5. the pre-stamp target
  for (int n = 2; n <= 3; ++n) {
    // adopted by sogm_update_prestamped while it is the front of ready
    if (fresh(p, n)) return 1;
    EXPECT(!p.front_is_prestamped());
    for (int g; (g = p.first_dirty()) >= 0;) STEP(p.queue_ready(g));
    const int target = p.front_ready();
    STEP(p.set_prestamp_target(target));
    EXPECT(p.prestamp_pending() && p.front_is_prestamped());
    STEP(p.adopt_front());
    STEP(p.adopted_prestamped());
    EXPECT(p.current() == target && p.current_prestamped() && !p.prestamp_pending() && !p.front_is_prestamped());
    // a plain update takes the target back: it is stale, it is the grid adopted next, and the caller resets it
    if (tick(p)) return 1;
    for (int g; (g = p.first_dirty()) >= 0;) STEP(p.queue_ready(g));
    const int t2 = p.front_ready();
    STEP(p.set_prestamp_target(t2));
    int stale = -1;
    STEP(stale = p.discard_prestamp());
    EXPECT(stale == t2 && !p.prestamp_pending() && !p.front_is_prestamped() && !p.current_prestamped());
    STEP(p.adopt_front());
    EXPECT(p.current() == stale);
    EXPECT(p.discard_prestamp() == -1);
    // adopted by somebody else (a dense writer's adopt): no longer the front, so not adoptable as pre-stamped
    for (int g; (g = p.first_dirty()) >= 0;) STEP(p.queue_ready(g));
    STEP(p.set_prestamp_target(p.front_ready()));
    STEP(p.adopt_front());
    EXPECT(!p.front_is_prestamped());
    // a replan that does not pre-stamp clears the target
    STEP(p.clear_prestamp_target());
    EXPECT(!p.prestamp_pending());
  }
  // mode 1: the in-place pre-clear is a flag of the single grid
  if (fresh(p, 1)) return 1;
  EXPECT(!p.precleared() && p.first_dirty() < 0 && p.front_ready() < 0);
  STEP(p.cleared_in_place());
  EXPECT(p.precleared());
  STEP(p.forget_preclear());
  EXPECT(!p.precleared());
  EXPECT(p.slot_of((const float *)(uintptr_t)0x8) == -1);
  std::printf("gridpool host ok\n");
  return 0;
}
