// sogm_flight_layout.hpp — which compute units each of the flight's four kernels gets: pure integer code, host-compilable
// (tests/flight_layout_host_test.cpp).  The liveness argument of the flight rests on it.
#pragma once

#include <cstdint>
#include <cstring>

namespace sogm {

// the 16-CU unit of a mask bit: two CUs per XCD whether bit i names XCD i / 32 or XCD i % 8 (tools/micro/cumask.hip).
// unit = 4 * shader engine + r: the compute units of one shader engine (of every XCD) whose index is congruent r mod 4.
inline int flight_unit_of(int i) { return ((i / 8) % 4) * 4 + ((i / 32 + i % 8) % 4); }

// Which units each of the four kernels gets.  The workgroup dispatcher hands the workgroups of a launch to the shader
// engines of its compute-unit mask in strict ROTATION: when one engine's units are full the dispatch stops, whatever room the
// other engines have (measured, tools/diag_flight_residency.py: a mask with four units in one engine and eight in another
// held 16 + 16 one-wave workgroups per XCD, not 16 + 32 — 120 of the round-5 corridor kernel's 384 workgroups sat in the
// dispatcher for the whole flight).  A workgroup that is not running is harmless until the hardware scheduler saves and
// restores the process's queues (any queue created or destroyed on the device, by any process, does that): the waiting
// workgroups then start in the slots the save freed, one per XCD ahead of the restored waves, and the wave that lost its slot
// stays saved until somebody leaves — the 3-second stalls of round 5.  So: every kernel's mask holds the SAME number of units
// in every shader engine it touches, and a launch has exactly as many workgroups as that mask holds at once
// (engines x smallest engine share): every workgroup is resident from the first microsecond, nothing waits in a dispatcher.
// grid[se][r] = kernel that owns unit 4 se + r (-1 free).  Kernels 0, 1, 3 (QP, search, map) are placed by a small search —
// fewest engines first — such that the rest (kernel 2, corridor + finish) is balanced too; if no such layout exists the most
// balanced one is kept and the launch is cut to what is resident.
struct FlightLayout {
  int grid[4][4];
  int resident_units[4];  // engines touched x smallest share, in units
};
inline int layout_rest_score(const int grid[4][4]) {  // units of the rest that are resident under the rotation
  int touched = 0, smallest = 5;
  for (int se = 0; se < 4; ++se) {
    int n = 0;
    for (int r = 0; r < 4; ++r) n += grid[se][r] == -1;
    if (n > 0) {
      ++touched;
      if (n < smallest) smallest = n;
    }
  }
  return touched ? touched * smallest : 0;
}
inline void layout_search(int grid[4][4], const int want[4], const int order[3], int depth, int rest_units, int *best_score,
                          int best[4][4]) {
  if (depth == 3) {
    const int sc = layout_rest_score(grid);
    if (sc > *best_score) {
      *best_score = sc;
      std::memcpy(best, grid, sizeof(int) * 16);
    }
    return;
  }
  const int k = order[depth], u = want[k];
  for (int n_se = 1; n_se <= 4 && *best_score < rest_units; ++n_se) {
    if (u % n_se != 0 || u / n_se > 4) continue;
    const int per = u / n_se;
    for (int set = 1; set < 16 && *best_score < rest_units; ++set) {
      if (__builtin_popcount((unsigned)set) != n_se) continue;
      int  saved[4][4];
      bool ok = true;
      std::memcpy(saved, grid, sizeof(saved));
      for (int se = 0; se < 4 && ok; ++se) {
        if (!((set >> se) & 1)) continue;
        int got = 0;
        for (int r = 0; r < 4 && got < per; ++r)
          if (grid[se][r] == -1) grid[se][r] = k, ++got;
        ok = got == per;
      }
      if (ok) layout_search(grid, want, order, depth + 1, rest_units, best_score, best);
      std::memcpy(grid, saved, sizeof(saved));
    }
  }
}
// engines [se0, se0 + n_se) are the flight's (the others belong to nobody here: -2); `reserved` units of them stay free of any
// kernel (-3), taken from the highest engine's highest classes first
inline FlightLayout flight_layout(const int want[4], int se0 = 0, int n_se = 4, int reserved = 0) {
  FlightLayout L;
  int          grid[4][4], best_score = -1;
  for (int i = 0; i < 16; ++i) (&grid[0][0])[i] = -1, (&L.grid[0][0])[i] = -1;
  for (int se = 0; se < 4; ++se)
    if (se < se0 || se >= se0 + n_se)
      for (int r = 0; r < 4; ++r) grid[se][r] = -2;
  for (int se = se0 + n_se - 1, left = reserved; se >= se0 && left > 0; --se)
    for (int r = 3; r >= 0 && left > 0; --r)
      if (grid[se][r] == -1) grid[se][r] = -3, --left;
  std::memcpy(L.grid, grid, sizeof(grid));
  const int order[3] = {0, 3, 1};  // QP and map (whole engines when they can have them), then the search
  layout_search(grid, want, order, 0, want[2], &best_score, L.grid);
  for (int i = 0; i < 16; ++i)
    if ((&L.grid[0][0])[i] == -1) (&L.grid[0][0])[i] = 2;
  for (int k = 0; k < 4; ++k) {
    int touched = 0, smallest = 5;
    for (int se = 0; se < 4; ++se) {
      int n = 0;
      for (int r = 0; r < 4; ++r) n += L.grid[se][r] == k;
      if (n > 0) {
        ++touched;
        if (n < smallest) smallest = n;
      }
    }
    L.resident_units[k] = touched ? touched * smallest : 0;
  }
  return L;
}

// The four streams' compute units and the four launches' sizes: QP, search, map take qp / search / map units of 16 CUs,
// corridor + finish the rest of the flight's engines; workgroups = what the partition holds at once (every workgroup of a
// flight kernel is resident from the start: nothing waits for a workgroup that is not running).
struct FlightPartition {
  FlightLayout layout;
  uint32_t     mask[4][16];  // the CU mask of each kernel's stream (QP, search, corridor + finish, map)
  int          cus[4];       // compute units that hold workgroups from the start
  int          wgs[4];       // workgroups of each launch
};
enum FlightPartitionError {
  FLIGHT_PARTITION_OK = 0,
  FLIGHT_PARTITION_NO_REST,      // the three unit counts leave no unit for the corridor kernel
  FLIGHT_PARTITION_UNPLACEABLE,  // no layout gives QP, search and map the same share in every engine they touch
};
inline FlightPartitionError flight_partition(int n_cu, int n_se, int se0, int reserved, int qp_units, int search_units,
                                             int map_units, bool masks, int light_per_cu, int map_per_cu, FlightPartition *out) {
  if (se0 + n_se > 4) n_se = 4 - se0;
  const int units_total = 4 * n_se - reserved;
  int       u[4]        = {qp_units, search_units, 0, map_units};
  u[2] = units_total - u[0] - u[1] - u[3];
  if (u[2] < 1) return FLIGHT_PARTITION_NO_REST;
  const FlightLayout L = flight_layout(u, se0, n_se, reserved);
  // (layout_search places a kernel whole or not at all: a stream without a compute unit and a launch of no workgroups)
  if (L.resident_units[0] < 1 || L.resident_units[1] < 1 || L.resident_units[3] < 1) return FLIGHT_PARTITION_UNPLACEABLE;
  out->layout = L;
  for (int k = 0; k < 4; ++k) {
    uint32_t *mask = out->mask[k];
    int       cus  = 0;
    for (int w = 0; w < 16; ++w) mask[w] = 0;
    for (int i = 0; i < n_cu && i < 512; ++i) {
      const int un = flight_unit_of(i);
      if (L.grid[un / 4][un % 4] == k) {
        mask[i / 32] |= 1u << (i % 32);
        ++cus;
      }
    }
    // compute units that hold workgroups from the start: the dispatcher's rotation over the mask's shader engines stops at
    // the smallest engine share (flight_layout balances the shares; an unbalanced rest is cut here)
    out->cus[k] = masks ? cus * L.resident_units[k] / (u[k] > 0 ? u[k] : 1) : cus;
  }
  out->wgs[0] = out->cus[0];                 // one QP workgroup per CU (a whole CU's LDS and registers)
  out->wgs[1] = out->cus[1];                 // one search workgroup per CU (124 KB of LDS)
  out->wgs[2] = light_per_cu * out->cus[2];  // corridor / finish waves: 39.8 KB of LDS, one per SIMD
  out->wgs[3] = map_per_cu * out->cus[3];    // map waves: two per SIMD
  return FLIGHT_PARTITION_OK;
}

}  // namespace sogm
