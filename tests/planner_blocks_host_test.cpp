// Host test of the device-side control blocks' layouts (csrc/sogm_handover.hpp: FlowBlock, FlightBlock, UpdateBlock), compiled with the
// host compiler: the regions in offset order without gap or overlap, carve() handing out exactly those offsets, the ranges a
// call resets, the 8-byte alignment of the 64-bit work queues, and the offsets tests and tools read peeked words by as literals;
// the update flow's block: every word on a 128-byte line of its own.
#include "sogm_handover.hpp"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

struct Region {
  long        off, words;
  const void *carved;  // what carve() handed out for it (null: nothing is carved for it)
};
// in offset order from 0: contiguous, no overlap, the last one ends at or before `total`; carve() agrees with the offsets
static int tiled(const Region *r, int n, const int *base, size_t total) {
  long at = 0;
  for (int i = 0; i < n; ++i) {
    EXPECT(r[i].off == at && r[i].words > 0);
    EXPECT(r[i].carved == nullptr || r[i].carved == (const void *)(base + r[i].off));
    at = r[i].off + r[i].words;
  }
  EXPECT((size_t)at <= total);
  return 0;
}

static int flow_block(int A, const int *base) {
  const FlowBlock b(A);
  FlowCtl         fc{};
  FlowBlock::carve(const_cast<int *>(base), A, &fc);
  const Region r[] = {{0, FLOW_HDR, fc.hdr},        {b.seg_done, A, fc.seg_done}, {b.stage, A, fc.stage},
                      {b.a_ready, A, fc.a_ready},   {b.q_ready, A, fc.q_ready},   {b.f_ready, A, fc.f_ready},
                      {b.p_ready, A, fc.p_ready},   {b.gen, 1, nullptr}};
  if (tiled(r, 8, base, FlowBlock::words(A))) return 1;
  // the order tools read by: hdr | seg_done | stage | a_ready | q_ready | f_ready | p_ready | gen
  EXPECT(b.seg_done == FLOW_HDR && b.stage == FLOW_HDR + A && b.a_ready == FLOW_HDR + 2 * A && b.q_ready == FLOW_HDR + 3 * A);
  EXPECT(b.f_ready == FLOW_HDR + 4 * A && b.p_ready == FLOW_HDR + 5 * A);
  // zeroed [0, FLOW_HDR + 2A), -1 over [FLOW_HDR + 2A, FLOW_HDR + 6A), the generation word at FLOW_HDR + 6A
  EXPECT(b.zero_words() == FLOW_HDR + 2 * A);
  EXPECT(b.fill_first() == FLOW_HDR + 2 * A && b.fill_first() + b.fill_words() == FLOW_HDR + 6 * A);
  EXPECT(b.gen == FLOW_HDR + 6 * A && FlowBlock::words(A) == (size_t)FLOW_HDR + 6 * (size_t)A + 1);
  return 0;
}

static int flight_block(int A, const int *base) {
  const FlightBlock b(A);
  FlightCtl         fl{};
  int              *xready = nullptr;
  FlightBlock::carve(const_cast<int *>(base), A, &fl, &xready);
  EXPECT(b.ring >= 2 * A && b.ring / 2 < 2 * A && (b.ring & (b.ring - 1)) == 0 && fl.ring_mask == b.ring - 1);
  const long   Q   = 2 * FL_WQ_SLOTS, T = FLIGHT_MAX_TICKS;
  const Region r[] = {{0, FL_HDR, fl.hdr},
                      {b.s_ring, b.ring, fl.s_ring},   {b.q_ring, b.ring, fl.q_ring},     {b.m_ring, b.ring, fl.m_ring},
                      {b.u_ring, b.ring, fl.u_ring},   {b.mw, Q, fl.mw},                  {b.lw, Q, fl.lw},
                      {b.tick_done, T, fl.tick_done},  {b.parked_n, T, fl.parked_n},      {b.xready, T, xready},
                      {b.tick_of, A, fl.tick_of},      {b.seg_done, A, fl.seg_done},      {b.stage, A, fl.stage},
                      {b.urgent, A, fl.urgent},        {b.parked, T * A, fl.parked},      {b.uw, Q, fl.uw}};
  if (tiled(r, 16, base, FlightBlock::words(A))) return 1;
  EXPECT((size_t)b.uw + Q <= FlightBlock::words(A) && (size_t)b.end == FlightBlock::words(A));
  EXPECT(FlightBlock::parked_words(A) == T * A);
  EXPECT(b.mw % 2 == 0 && b.lw % 2 == 0 && b.uw % 2 == 0);
  // a call zeroes exactly what lies in front of `parked`: xready is inside, the urgent queue is not
  EXPECT(FlightBlock::reset_words(A) == b.parked);
  EXPECT(b.xready + T <= FlightBlock::reset_words(A) && FlightBlock::reset_words(A) < b.uw);
  return 0;
}

// The update flow's block (the base is 128-byte aligned: a device allocation): the ticket, the error word and every agent's
// progress word lie on distinct 128-byte lines inside words(A), at the offsets tools read them by.
static int update_block(int A, int *base) {
  EXPECT(UpdateBlock::words(A) == 2048 + 32 * (size_t)A);
  EXPECT(UpdateBlock::ticket() == 0 && UpdateBlock::err() == 1024);
  std::vector<long> lines = {UpdateBlock::ticket() * 4L / 128, UpdateBlock::err() * 4L / 128};
  for (int a = 0; a < A; ++a) {
    EXPECT(UpdateBlock::stage(a) == 2048 + 32 * a);
    EXPECT(UpdateBlock::stage_word(base, a) == base + UpdateBlock::stage(a));
    lines.push_back(UpdateBlock::stage(a) * 4L / 128);
  }
  std::sort(lines.begin(), lines.end());
  EXPECT(std::adjacent_find(lines.begin(), lines.end()) == lines.end());
  EXPECT(UpdateBlock::stage(A - 1) >= 0 && (size_t)UpdateBlock::stage(A - 1) < UpdateBlock::words(A));
  EXPECT((size_t)UpdateBlock::err() < UpdateBlock::words(A) && (size_t)(lines.back() + 1) * 32 <= UpdateBlock::words(A));
  return 0;
}

int main() {
  const int sizes[] = {1, 2, 3, 127, 128, 129, 1000, 65535};
  std::vector<int> mem(FlightBlock::words(65535));  // (carve only computes addresses: one buffer for every size of both blocks)
  for (int A : sizes) {
    if (flow_block(A, mem.data())) return 1;
    if (flight_block(A, mem.data())) return 1;
  }
  for (int A : {1, 2, 128})
    if (update_block(A, mem.data())) return 1;
  EXPECT(FlowBlock::words(128) == 780 && FlowBlock::words(1) == 18);
  EXPECT(FlightBlock::ring_of(1) == 2 && FlightBlock::ring_of(3) == 8 && FlightBlock::ring_of(128) == 256 &&
         FlightBlock::ring_of(129) == 512);
  const FlightBlock b(128);
  EXPECT(b.s_ring == 20480 && b.mw == 21504 && b.lw == 283648 && b.tick_done == 545792 && b.tick_of == 545984);
  EXPECT(b.parked == 546496 && FlightBlock::reset_words(128) == 546496 && b.uw == 554688 && b.uw + 2 * FL_WQ_SLOTS == 816832);
  std::printf("planner blocks host ok\n");
  return 0;
}
