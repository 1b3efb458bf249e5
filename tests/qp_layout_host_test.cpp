// Host test of the QP solver's memory plan (csrc/sogm_qp_layout.hpp), compiled with the host compiler: the regions of
// every (fast, rows_in_lds) combination in offset order without gap or overlap (the layout's offsets: the kernel's own
// pointers are held to it only through the path it reports, tests/test_qp_gpu.py); the byte totals and path choices the solver's formulas gave before they had one description (computed from
// those formulas for M pieces of f faces each); every term of `fast` at its edge.
#include "sogm_qp_layout.hpp"

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

static const size_t DYN = 145408;  // 160 KiB minus about 18 KiB of static LDS, rounded down to 256

struct Region {
  size_t off, bytes;
};
// in offset order: contiguous, no overlap, every start on 8 bytes (every region starts with doubles), the last ends at `total`
static int tiled(const std::vector<Region> &r, size_t total) {
  size_t at = 0;
  for (const Region &x : r) {
    EXPECT(x.off == at && x.off % 8 == 0 && x.bytes > 0);
    at += x.bytes;
  }
  EXPECT(at == total);
  return 0;
}
// the row arrays as the solver indexes them, written out here a second time (the header's table is under test): bytes of the
// hot arrays, of the cold doubles, of the cold ints with the cidx allowance of QP_ELL ints per general row, and the 64 B tail
static size_t hot_of(size_t G, size_t S) { return 8 * (S * 3 + S + G); }
static size_t cold_doubles_of(size_t G, size_t S) { return 8 * (G * 6 + 8 * G + 5 * S); }
static size_t cold_ints_of(size_t G, size_t S) { return 4 * (G * 6 + S + G * 6); }

// M pieces of f faces each at DYN: the expected path, every region in its buffer
static int tiling(int M, int f, bool want_fast, bool want_in_lds) {
  const QpShape  sh(M, M * f);
  const QpLayout L(sh, DYN);
  EXPECT(L.fast == want_fast && L.rows_in_lds == want_in_lds);
  const size_t G = sh.G, S = sh.S, blk = (size_t)M * 225 * 8, band = (size_t)sh.n * 18 * 8;
  const size_t hot = hot_of(G, S), cold = cold_doubles_of(G, S) + cold_ints_of(G, S) + 64, pad = (16 - (hot + cold) % 16) % 16;
  EXPECT(rows_hot_bytes(sh.G, sh.S) == hot && rows_cold_bytes(sh.G, sh.S) == cold && rows_bytes(sh.G, sh.S) == hot + cold);
  EXPECT(cold_doubles_of(G, S) % 8 == 0 && cold_ints_of(G, S) % 4 == 0);  // doubles on 8 bytes, the ints behind them on 4
  const size_t stride = qp_scratch_bytes_per_agent(f);
  EXPECT(L.lds_bytes() <= DYN && L.scratch_bytes() <= stride && L.k1_scratch_bytes() <= qp_k1_scratch_bytes_per_agent());
  std::vector<Region> in_lds, in_scr;
  if (L.fast) {
    in_lds = {{L.P, blk}, {L.Dv, blk}, {L.V, blk}, {L.Z, blk}, {L.hot, hot}};
    // the check's staging: from Dv on, inside [Dv, Z end), ending at or before the hot rows
    const size_t stage_end = L.check + 8 * L.check_doubles();
    EXPECT(L.check == L.Dv && stage_end <= L.Z + blk && L.Z + blk == L.hot);
    EXPECT(L.check_doubles() == G + S + 320 && L.block_area_doubles() == 3 * blk / 8);
  } else {
    in_lds = {{L.Kb, band}, {L.P, blk}};
    if (L.rows_in_lds) in_lds.push_back({L.hot, hot});
  }
  if (L.rows_in_lds) {
    in_lds.push_back({L.cold, cold + pad});
    if (L.fast) in_lds.push_back({L.k1, band});
    EXPECT(L.scratch_bytes() == 0 && L.k1_scratch_bytes() == 0);
  } else {
    in_scr = {{L.scr_hot, hot}, {L.scr_cold, cold}};  // (the hot part is left unused while the hot rows are in LDS)
    EXPECT(L.k1_scratch_bytes() == (L.fast ? band : 0));
    if (tiled(in_scr, L.scratch_bytes())) return 1;
  }
  return tiled(in_lds, L.lds_bytes());
}

// the values the solver's formulas gave before this header: G, S, hot and cold bytes, the rows' offset in LDS, K1 bytes
static int pinned(int M, int f, int G, int S, size_t hot, size_t cold, size_t head_general, size_t head_fast, size_t k1) {
  const QpShape  sh(M, M * f);
  const QpLayout L(sh, DYN);
  EXPECT(sh.M == M && sh.n == 15 * M && sh.R1 == 3 * (M + 1) && sh.R3 == 3 * sh.R1 && sh.R4 == sh.R3 + 12 * M);
  EXPECT(sh.G == G && sh.S == S && rows_hot_bytes(sh.G, sh.S) == hot && rows_cold_bytes(sh.G, sh.S) == cold);
  EXPECT(L.fast == (head_fast != 0) && L.hot == (L.fast ? head_fast : head_general) && L.cold == L.hot + hot);
  if (L.fast) EXPECT(L.band_bytes() == k1 && L.P == 0 && L.check == L.Dv && L.Dv == head_fast / 4);
  return 0;
}

static int path(int M, int f, size_t dyn, bool fast, bool in_lds) {
  const QpLayout L(QpShape(M, M * f), dyn);
  EXPECT(L.fast == fast && L.rows_in_lds == in_lds);
  return 0;
}

static bool fast_of(QpShape sh, size_t dyn = DYN) { return QpLayout(sh, dyn).fast; }
static QpShape with_rows(int M, int S) {  // a shape with S safety rows, S not a multiple of 5 included
  QpShape sh(M, 0);
  sh.S = S;
  return sh;
}

static int edges() {
  QpShape sh(8, 48);  // G = 249
  EXPECT(fast_of(sh));
  sh.G = 256;
  EXPECT(fast_of(sh));
  sh.G = 257;
  EXPECT(!fast_of(sh));
  QpShape m9(9, 54);
  m9.G = 256;  // (a real shape of 9 pieces has 279 general rows: the term for M on its own)
  EXPECT(!fast_of(m9));
  m9.M = 8;
  EXPECT(fast_of(m9));
  EXPECT(fast_of(with_rows(8, 1024)) && !fast_of(with_rows(8, 1025)));
  // the check's staging area exactly fills the block area: 39 + 316 + 320 == 675
  EXPECT(QpLayout(with_rows(1, 316), DYN).check_doubles() == QpLayout(with_rows(1, 316), DYN).block_area_doubles());
  EXPECT(fast_of(with_rows(1, 316)) && !fast_of(with_rows(1, 317)));
  // blocks + hot rows exactly fill the dynamic LDS: 8 x 25 needs 57 600 + 33 992
  EXPECT(fast_of(QpShape(8, 200), 91592) && !fast_of(QpShape(8, 200), 91591));
  EXPECT(!QpLayout(QpShape(8, 200), 91592).rows_in_lds && QpLayout(QpShape(8, 200), 91592).lds_bytes() == 91592);
  // all rows in LDS exactly: 3 x 6 needs 21 600 + 23 536 + 6 480
  EXPECT(QpLayout(QpShape(3, 18), 51616).rows_in_lds && !QpLayout(QpShape(3, 18), 51615).rows_in_lds);
  return 0;
}

int main() {
  if (tiling(12, 6, false, true) || tiling(8, 30, false, false) || tiling(8, 25, true, false) || tiling(3, 6, true, true) ||
      tiling(5, 40, true, false) || tiling(16, 6, false, false) || tiling(1, 6, true, true))
    return 1;
  if (pinned(12, 6, 369, 360, 14472, 74944, 47520, 0, 0) || pinned(8, 30, 249, 1200, 40392, 92704, 31680, 0, 0) ||
      pinned(8, 25, 249, 1000, 33992, 83904, 0, 57600, 17280) || pinned(5, 40, 159, 1000, 33272, 69504, 0, 36000, 10800) ||
      pinned(3, 6, 99, 90, 3672, 19864, 0, 21600, 6480) || pinned(16, 6, 489, 480, 19272, 99424, 63360, 0, 0) ||
      pinned(1, 6, 39, 30, 1272, 7624, 0, 7200, 2160))
    return 1;
  EXPECT(qp_scratch_bytes_per_agent(64) == 471552 && qp_k1_scratch_bytes_per_agent() == 17280);
  // 5 x 40 needs 36 000 + 102 784 + 10 800 = 149 584 bytes for everything in LDS: out at all three
  EXPECT(QpLayout(QpShape(5, 200), 149584).rows_in_lds && !QpLayout(QpShape(5, 200), 149583).rows_in_lds);
  for (size_t dyn : {(size_t)145408, (size_t)147456, (size_t)149504})
    if (path(12, 6, dyn, false, true) || path(8, 30, dyn, false, false) || path(8, 25, dyn, true, false) ||
        path(5, 40, dyn, true, false) || path(3, 6, dyn, true, true) || path(16, 6, dyn, false, false))
      return 1;
  if (edges()) return 1;
  std::printf("qp layout host ok\n");
  return 0;
}
