// Host test of the flight's compute-unit partition (csrc/sogm_flight_layout.hpp), compiled with the host compiler: which unit
// a compute unit belongs to, the grids flight_layout places for six configurations (literals: what the function returned
// before it had a header of its own), the balance property the flight's liveness rests on, the masks and launch sizes
// flight_partition derives from a grid, and the splits it refuses.
#include "sogm_flight_layout.hpp"

#include <cstdio>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

struct Case {
  int want[4];  // QP, search, rest (corridor + finish), map
  int n_se, se0, reserved;
  int grid[4][4];  // rows: shader engine 0..3
  int resident[4];
};
static const Case cases[] = {
    {{4, 2, 6, 4}, 4, 0, 0, {{0, 0, 0, 0}, {3, 3, 3, 3}, {1, 2, 2, 2}, {1, 2, 2, 2}}, {4, 2, 6, 4}},
    {{3, 1, 6, 6}, 4, 0, 0, {{0, 0, 0, 1}, {3, 3, 2, 2}, {3, 3, 2, 2}, {3, 3, 2, 2}}, {3, 1, 6, 6}},
    {{2, 1, 7, 6}, 4, 0, 0, {{0, 0, 3, 3}, {3, 3, 2, 2}, {3, 3, 2, 2}, {1, 2, 2, 2}}, {2, 1, 6, 6}},  // the rest is cut: 6 of 7
    {{2, 2, 2, 2}, 2, 0, 0, {{0, 0, 3, 3}, {1, 1, 2, 2}, {-2, -2, -2, -2}, {-2, -2, -2, -2}}, {2, 2, 2, 2}},
    {{2, 2, 2, 2}, 2, 2, 0, {{-2, -2, -2, -2}, {-2, -2, -2, -2}, {0, 0, 3, 3}, {1, 1, 2, 2}}, {2, 2, 2, 2}},
    {{4, 2, 6, 3}, 4, 0, 1, {{0, 0, 0, 0}, {3, 3, 3, 1}, {1, 2, 2, 2}, {2, 2, 2, -3}}, {4, 2, 6, 3}},
};
static const int n_cases = (int)(sizeof(cases) / sizeof(cases[0]));

static int popcount(const uint32_t *mask) {
  int n = 0;
  for (int w = 0; w < 16; ++w) n += __builtin_popcount(mask[w]);
  return n;
}

static int unit_of() {
  int per_unit[16] = {0};
  for (int i = 0; i < 256; ++i) {
    const int u = flight_unit_of(i);
    EXPECT(u >= 0 && u < 16);
    ++per_unit[u];
  }
  for (int u = 0; u < 16; ++u) EXPECT(per_unit[u] == 16);
  return 0;
}

static int layout(const Case &c) {
  const FlightLayout L = flight_layout(c.want, c.se0, c.n_se, c.reserved);
  for (int se = 0; se < 4; ++se)
    for (int r = 0; r < 4; ++r) EXPECT(L.grid[se][r] == c.grid[se][r]);
  for (int k = 0; k < 4; ++k) {
    EXPECT(L.resident_units[k] == c.resident[k]);
    // the property: the dispatcher's rotation stops at the smallest engine share, so a kernel whose launch is to be resident
    // as a whole holds the SAME number of units in every engine it touches.  QP, search and map are placed that way or not
    // at all; the rest takes what is left and is balanced exactly when nothing of it is cut (resident == wanted).
    int units = 0, touched = 0, lo = 5, hi = 0;
    for (int se = 0; se < 4; ++se) {
      int n = 0;
      for (int r = 0; r < 4; ++r) n += L.grid[se][r] == k;
      if (n == 0) continue;
      units += n, ++touched;
      if (n < lo) lo = n;
      if (n > hi) hi = n;
    }
    EXPECT(units == c.want[k] && L.resident_units[k] == touched * lo);
    if (k != 2 || L.resident_units[k] == c.want[k]) EXPECT(lo == hi);
    else EXPECT(lo < hi);
  }
  return 0;
}

// n_cu = 256, masks on, flight_light_per_cu = 4, flight_map_per_cu = 8
static int partition(const Case &c) {
  FlightPartition P;
  EXPECT(flight_partition(256, c.n_se, c.se0, c.reserved, c.want[0], c.want[1], c.want[3], true, 4, 8, &P) == FLIGHT_PARTITION_OK);
  uint32_t all[16] = {0};
  for (int k = 0; k < 4; ++k) {
    EXPECT(P.layout.resident_units[k] == c.resident[k]);
    EXPECT(popcount(P.mask[k]) == 16 * c.want[k]);
    EXPECT(P.cus[k] == 16 * c.resident[k]);
    for (int w = 0; w < 16; ++w) {
      EXPECT((all[w] & P.mask[k][w]) == 0);  // disjoint
      all[w] |= P.mask[k][w];
    }
  }
  // with the reserved units (and the engines that are not the flight's) the masks cover every compute unit
  for (int i = 0; i < 512; ++i) {
    const int  un     = flight_unit_of(i);
    const bool masked = (all[i / 32] >> (i % 32)) & 1;
    EXPECT(masked == (i < 256 && c.grid[un / 4][un % 4] >= 0));
  }
  EXPECT(popcount(all) + 16 * c.reserved + 64 * (4 - c.n_se) == 256);
  EXPECT(P.wgs[0] == P.cus[0] && P.wgs[1] == P.cus[1] && P.wgs[2] == 4 * P.cus[2] && P.wgs[3] == 8 * P.cus[3]);
  // masks off: every compute unit counts, the layout is the same
  FlightPartition Q;
  EXPECT(flight_partition(256, c.n_se, c.se0, c.reserved, c.want[0], c.want[1], c.want[3], false, 4, 8, &Q) == FLIGHT_PARTITION_OK);
  for (int k = 0; k < 4; ++k) EXPECT(Q.cus[k] == 16 * c.want[k]);
  return 0;
}

int main() {
  if (unit_of()) return 1;
  for (int i = 0; i < n_cases; ++i) {
    if (layout(cases[i])) return 1;
    if (partition(cases[i])) return 1;
  }
  FlightPartition P;
  EXPECT(flight_partition(256, 4, 0, 0, 2, 1, 6, true, 4, 8, &P) == FLIGHT_PARTITION_OK);  // {2,1,7,6}
  EXPECT(P.cus[0] == 32 && P.cus[1] == 16 && P.cus[2] == 96 && P.cus[3] == 96);
  // an engine count beyond the device's last engine is cut, as flight_setup always did
  EXPECT(flight_partition(256, 4, 2, 0, 2, 2, 2, true, 4, 8, &P) == FLIGHT_PARTITION_OK && P.layout.grid[2][0] == 0 &&
         P.layout.grid[0][0] == -2);
  // {5,2,5,4}: no balanced place for QP, search and map — before, a stream with an empty mask and a launch of no workgroups
  const int bad[4] = {5, 2, 5, 4};
  const FlightLayout L = flight_layout(bad);
  EXPECT(L.resident_units[0] == 0 && L.resident_units[1] == 0 && L.resident_units[2] == 16 && L.resident_units[3] == 0);
  EXPECT(flight_partition(256, 4, 0, 0, 5, 2, 4, true, 4, 8, &P) == FLIGHT_PARTITION_UNPLACEABLE);
  EXPECT(flight_partition(256, 4, 0, 0, 5, 2, 4, false, 4, 8, &P) == FLIGHT_PARTITION_UNPLACEABLE);
  EXPECT(flight_partition(256, 4, 0, 0, 6, 6, 4, true, 4, 8, &P) == FLIGHT_PARTITION_NO_REST);
  std::printf("flight layout host ok\n");
  return 0;
}
