// Host test of the LDS layouts of the corridor translation unit (csrc/sogm_lp.hpp), compiled with the host compiler (the
// header's device-side parts sit behind __HIPCC__): the byte totals the launchers passed before the layouts had one
// description, the regions in order without gap or overlap, the LP view a wave uses between two segments, and the bound that
// keeps four workgroups on a compute unit.
#include "sogm_lp.hpp"

#include <cstdio>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

struct Region {
  size_t off, bytes;  // byte offset in the layout; the bytes its users need (the kernels' own loop bounds)
  bool   f64;
};
// in offset order: contiguous, no overlap, the last one ends at `total`; doubles start on 8 bytes
static int tiled(const Region *r, int n, size_t total) {
  size_t at = 0;
  for (int i = 0; i < n; ++i) {
    EXPECT(r[i].off == at);
    EXPECT(!r[i].f64 || r[i].off % 8 == 0);
    EXPECT(r[i].off % 4 == 0 && r[i].bytes > 0);
    at = r[i].off + r[i].bytes;
  }
  EXPECT(at == total);
  return 0;
}
static size_t d(int doubles) { return 8 * (size_t)doubles; }

static int lp_wave() {
  EXPECT(LpLds::bytes() == 23868);  // 8 (2142 + 765) + 4 * 153
  const Region r[] = {{d(LpLds::work), d(14 * 153), true}, {d(LpLds::rows), d(153 * 5), true}, {LpLds::perm, 4 * 153, false}};
  if (tiled(r, 3, LpLds::bytes())) return 1;
  // the view: A in front of b inside rows, perm directly behind the rows
  static double base[LpLds::bytes() / 8 + 1];
  LpScratch sc = LpLds::carve(base);
  EXPECT(sc.work == base && sc.rows == base + 2142 && sc.A() == sc.rows && sc.b() == sc.rows + 153 * 4);
  EXPECT((char *)sc.perm == (char *)(sc.rows + 153 * 5) && (char *)sc.perm == (char *)base + LpLds::perm);
  return 0;
}

template <int MB>
static int segment(size_t fixed_bytes) {
  using L = SegmentLds<MB>;
  const int caps[] = {1, 63, 64, 65, 4096, 16384};
  for (int cap : caps) {
    const size_t words = ((size_t)cap + 63) / 64;
    EXPECT(L::bytes(cap) == fixed_bytes + 8 * words);
    const int    small = MB == 6 ? 96 : 34 + 9 * MB;  // 96 at MB = 6: 88 used, 8 spare
    const Region r[]   = {{d(LpLds::work), d(14 * 153), true}, {d(LpLds::rows), d(153 * 5), true},
                          {d(L::lm), d(2 * 18 * 9), true},     {d(L::handoff), d(16), true},
                          {d(L::keep), d(36), true},           {d(L::fH), d(128 * 4), true},
                          {d(L::poly), d(128 * 4), true},      {d(L::small), d(small), true},
                          {d(L::flags), 8 * words, true},      {L::perm(cap), 4 * 153, false},
                          {L::ints(cap), 4 * 16, false}};
    if (tiled(r, 11, L::bytes(cap))) return 1;
    EXPECT(L::flag_words(cap) == (int)words && 64 * words >= (size_t)cap);
  }
  // the small state: fields in order, each as long as its loops write, inside the block
  const int f[] = {L::fwd, L::fa, L::fb, L::p, L::fh, L::bd, L::fB, L::fD, L::dD, L::box, L::w, 34 + 9 * MB};
  const int n[] = {9, 3, 3, 3, 4, 4 * MB, 3 * MB, MB, MB, 6, 6};
  EXPECT(f[0] == 0);
  for (int i = 0; i < 11; ++i) EXPECT(f[i + 1] == f[i] + n[i]);
  EXPECT(f[11] <= L::small_n && L::flags == L::small + L::small_n);
  // the LP view between two segments lies in [rows end, fH start): the head of lm
  EXPECT(LpLds::perm >= d(LpLds::rows + 153 * 5) && LpLds::perm == d(L::lm) && LpLds::bytes() <= d(L::fH));
  EXPECT(L::bytes(16384) <= 40960);  // four workgroups per compute unit
  return 0;
}

static int rules() {
  EXPECT(RulesLds::bytes() == 26012);  // 8 (2907 + 268) + 612
  const Region r[] = {{d(LpLds::work), d(14 * 153), true}, {d(LpLds::rows), d(153 * 5), true}, {d(RulesLds::poly), d(64 * 4), true},
                      {d(RulesLds::box), d(6), true},      {d(RulesLds::w), d(6), true},       {RulesLds::perm, 4 * 153, false}};
  return tiled(r, 6, RulesLds::bytes());
}

int main() {
  if (lp_wave() || segment<6>(35900) || segment<FIRI_DIRECT_BD_MAX>(37708) || rules()) return 1;
  EXPECT(SegmentLds<6>::bytes(16384) == 37948 && SegmentLds<32>::bytes(16384) == 39756);
  std::printf("corridor lds host ok\n");
  return 0;
}
