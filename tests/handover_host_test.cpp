// Host test of csrc/sogm_handover.hpp: the tag arithmetic of the rings, work queues and descriptors and the values of the
// failure codes, compiled with the host compiler (the device-side parts of the header sit behind __HIPCC__).
#include "sogm_handover.hpp"

#include <cstdio>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static bool ring_match(int tag, int pos, int R) { return ring_generation(tag) == ring_want(pos, R); }
static bool wq_match(unsigned long long tag, unsigned pos) { return wq_generation(tag) == wq_want(pos); }

static int rings() {
  const int sizes[] = {2, 4, 256}, agents[] = {0, 1, 65535};
  for (int R : sizes)
    for (int pos = 0; pos <= 4 * R; ++pos) {
      EXPECT(!ring_match(0, pos, R));  // the word a reset leaves
      for (int agent : agents) {
        const int tag = ring_encode(pos, R, agent);
        EXPECT(ring_agent(tag) == agent);
        EXPECT(ring_match(tag, pos, R));
        EXPECT(!ring_match(tag, pos + R, R));
        if (pos >= R) EXPECT(!ring_match(tag, pos - R, R));
        EXPECT(tag > 0);
      }
    }
  // the largest position of a flight: one item per agent and tick, 65535 agents, the smallest ring flight_setup makes for
  // them (the power of two >= 2 A)
  const int A = RING_MAX_AGENTS - 1, R = 2 * RING_MAX_AGENTS, last = FLIGHT_MAX_TICKS * A - 1;
  EXPECT(R >= 2 * A && (R & (R - 1)) == 0 && R / 2 < 2 * A);
  EXPECT(ring_encode(last, R, A) > 0 && ring_agent(ring_encode(last, R, A)) == A && ring_match(ring_encode(last, R, A), last, R));
  EXPECT(ring_want(last, R) <= RING_MAX_GENERATION);
  return 0;
}

static int queues() {
  const unsigned S = FL_WQ_SLOTS, positions[] = {0u, S - 1u, S, 3u * S + 5u, 0xFFFFFFFFu}, descs[] = {0u, 1u, 0x6FFFFFFFu};
  for (unsigned pos : positions) {
    EXPECT(!wq_match(0ull, pos));
    EXPECT(wq_slot(pos) < S && (pos - wq_slot(pos)) % S == 0);
    for (unsigned desc : descs) {
      const unsigned long long tag = wq_encode(pos, desc);
      EXPECT(wq_desc(tag) == desc);
      EXPECT(wq_match(tag, pos));
      if (pos <= 0xFFFFFFFFu - S) EXPECT(!wq_match(tag, pos + S));
      if (pos >= S) EXPECT(!wq_match(tag, pos - S));
      EXPECT(tag != 0ull);
    }
  }
  return 0;
}

static int descriptors() {
  const int subs[] = {0, 1, WK_MAX_SUB - 1}, agents[] = {0, WK_MAX_AGENTS - 1};
  EXPECT(WK_MAX_SUB == 4096 && WK_MAX_AGENTS == 65536);
  for (int kind = WK_MAP_HEAD; kind <= WK_FINISH; ++kind)
    for (int sub : subs)
      for (int agent : agents) {
        const unsigned d = wk_pack(kind, sub, agent);
        EXPECT((int)d >= 0);  // the consumers return it as an int; negative values mean "no descriptor"
        EXPECT(wk_kind((int)d) == kind && wk_sub((int)d) == sub && wk_agent((int)d) == agent);
        // wq_push's consecutive descriptors: the sub field advances, the kind and the agent stay
        for (int i = 0; i < WK_MAX_SUB - sub; ++i) {
          const int e = (int)wk_advance_sub(d, i);
          EXPECT(wk_kind(e) == kind && wk_sub(e) == sub + i && wk_agent(e) == agent);
        }
      }
  return 0;
}

// the values of the commit before the codes had names
static int codes() {
  EXPECT(FLOW_CODE_NONE == 0);
  EXPECT(FLOW_CODE_RESIDENCY_GATE == 1);
  EXPECT(FLOW_CODE_READY_SLOT == 2);
  EXPECT(FLOW_CODE_QP_ITEM == 3);
  EXPECT(FLOW_CODE_VERDICT == 4);
  EXPECT(FLOW_CODE_STAGE_COUNT == 6);
  EXPECT(FLOW_CODE_PRESTAMP_GATE == 7);
  EXPECT(FLOW_CODE_OVERLAY_STAMP == 8);
  EXPECT(FLOW_CODE_RING_ITEM == 12);
  EXPECT(FLOW_CODE_WORK_QUEUE == 15);
  EXPECT(FLOW_CODE_MAP_READY == 16);
  EXPECT(FLOW_CODE_ADMISSION == 16);
  EXPECT(FLOW_CODE_HEAD_ITEM == 17);
  EXPECT(FLOW_TIMEOUT_TICKS == 300000000LL);  // 3 s at 100 MHz
  return 0;
}

int main() {
  if (rings() || queues() || descriptors() || codes()) return 1;
  std::printf("handover host ok\n");
  return 0;
}
