// Host test of the velocity estimation's single-lane rules (csrc/sogm_dsp_velocity.hpp), compiled with the host compiler
// against libstdc++: the restated std::sort and its heap-sort fallback against the library's, tie order included; the
// minimum-cost assignment against brute force on matrices with a unique optimum; the gates and the velocity clamp; the
// possibly-dynamic split with its offsets against literals; the kernel's dynamic-LDS layout.
#include "sogm_dsp_velocity.hpp"

#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <vector>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// ---- the sort ---------------------------------------------------------------------------------------------------------
static bool by_size(const vel::Item &a, const vel::Item &b) { return a.size < b.size; }

static int sort_cases() {
  std::mt19937 rng(1487u);
  for (int n : {0, 1, 2, 15, 16, 17, 33, 100, 256})
    for (int kind = 0; kind < 3; ++kind) {
      std::vector<vel::Item> in(n);
      for (int i = 0; i < n; ++i) {
        in[i].id   = i;
        in[i].size = kind == 0 ? 7 : kind == 1 ? 5 + (int)(rng() % 6u) : 1000 - i;  // equal | many ties | decreasing
      }
      {
        std::vector<vel::Item> got(in), want(in);
        vel::std_sort(got.data(), n);
        std::sort(want.begin(), want.end(), by_size);
        for (int i = 0; i < n; ++i) EXPECT(got[i].id == want[i].id && got[i].size == want[i].size);
      }
      {
        std::vector<vel::Item> got(in), want(in);
        vel::heap_sort(got.data(), n);
        std::partial_sort(want.begin(), want.end(), want.end(), by_size);
        for (int i = 0; i < n; ++i) EXPECT(got[i].id == want[i].id && got[i].size == want[i].size);
      }
    }
  return 0;
}

// ---- the assignment ---------------------------------------------------------------------------------------------------
// cheapest injection of the smaller side into the larger by brute force: match[r] = c or -1
static void brute_force(const std::vector<float> &cost, int R, int C, std::vector<int> &match) {
  const bool       tr = R > C;
  const int        NR = tr ? C : R, NC = tr ? R : C;
  std::vector<int> pick(NR), used(NC, 0), best;
  float            best_sum = 0.f;
  auto at = [&](int i, int j) { return tr ? cost[j * C + i] : cost[i * C + j]; };
  auto rec = [&](auto &&self, int i, float sum) -> void {
    if (i == NR) {
      if (best.empty() || sum < best_sum) {
        best     = pick;
        best_sum = sum;
      }
      return;
    }
    for (int j = 0; j < NC; ++j)
      if (!used[j]) {
        used[j] = 1;
        pick[i] = j;
        self(self, i + 1, sum + at(i, j));
        used[j] = 0;
      }
  };
  rec(rec, 0, 0.f);
  match.assign(R, -1);
  for (int i = 0; i < NR; ++i) {
    if (tr)
      match[best[i]] = i;
    else
      match[i] = best[i];
  }
}

static int assignment_cases() {
  const int shapes[7][2] = {{1, 1}, {1, 4}, {4, 1}, {2, 3}, {3, 4}, {4, 3}, {4, 4}};
  for (const auto &sh : shapes)
    for (unsigned seed = 1; seed <= 3; ++seed) {
      const int        R = sh[0], C = sh[1];
      std::vector<int> perm(R * C);
      std::iota(perm.begin(), perm.end(), 0);
      std::mt19937 rng(seed * 7919u + (unsigned)(R * 16 + C));
      std::shuffle(perm.begin(), perm.end(), rng);
      std::vector<float> cost(R * C);
      float              total = 0.f;
      for (int k = 0; k < R * C; ++k) {
        cost[k] = (float)(1u << perm[k]);  // powers of two: distinct subsets have distinct sums, the optimum is unique
        total += cost[k];
      }
      EXPECT(total < 65536.f);  // every value and every sum is exact in fp32
      std::vector<int> want;
      brute_force(cost, R, C, want);
      vel::Assignment as;
      vel::assign(cost.data(), R, C, &as);
      EXPECT(as.ncols == (R > C ? R : C) && as.tr == (R > C));
      std::vector<int> got(R, -1);
      int              pairs = 0;
      for (int j = 1; j <= as.ncols; ++j) {
        int r, c;
        if (!as.pair(j, &r, &c)) continue;
        EXPECT(r >= 0 && r < R && c >= 0 && c < C && got[r] == -1);
        got[r] = c;
        ++pairs;
      }
      EXPECT(pairs == (R < C ? R : C));
      EXPECT(got == want);
    }
  return 0;
}

// ---- gates and clamp: two new clusters against two old ones -----------------------------------------------------------
static int association_cases() {
  const int            size[2] = {20, 30};
  const float          cz[2]   = {0.5f, 0.5f};
  const int            dynseq[2] = {0, 1};
  std::vector<float>   cost(16), gate(16);
  for (int kind = 0; kind < 2; ++kind) {
    // kind 0: every old cluster is >= distance_gate away from every new one, or differs by more than point_num_gate points
    // kind 1: cluster 0 moved 1 m in 0.1 s (10 m/s > maximum_velocity), cluster 1 has no partner within the gates
    const float          cx[2] = {0.f, 10.f}, cy[2] = {0.f, 0.f};
    const vel::Clusters  cl = {2, size, cx, cy, cz};
    float last[VEL_MAX_DYN][5] = {};
    if (kind == 0) {
      const float l0[5] = {0.f, 1.5f, 0.5f, 0.8f, 20.f}, l1[5] = {10.f, 0.f, 0.5f, 0.9f, 131.f};  // at the gate; 101 points off
      std::copy(l0, l0 + 5, last[0]);
      std::copy(l1, l1 + 5, last[1]);
    } else {
      const float l0[5] = {1.f, 0.f, 0.5f, 0.8f, 25.f}, l1[5] = {50.f, 0.f, 0.5f, 0.9f, 30.f};
      std::copy(l0, l0 + 5, last[0]);
      std::copy(l1, l1 + 5, last[1]);
    }
    float v[VEL_MAX_DYN][4];
    int   ds[2], off[2], total_dyn = -1, n_static = -1, err = 0;
    const int nd = vel::dynamic_split(cl, 0, ds, off, v, &total_dyn, &n_static, &err);
    EXPECT(nd == 2 && ds[0] == 0 && ds[1] == 1 && err == 0);
    const int matched = vel::associate(cl, dynseq, nd, last, 2, 0.1f, cost.data(), gate.data(), (int)cost.size(), v, &err);
    EXPECT(err == 0);
    if (kind == 0) {
      EXPECT(matched == 0);
      for (int r = 0; r < 2; ++r) EXPECT(v[r][0] == -10000.f && v[r][1] == -10000.f && v[r][2] == -10000.f && v[r][3] == 0.55f);
    } else {
      EXPECT(matched == 1);
      EXPECT(v[0][0] == 0.f && v[0][1] == 0.f && v[0][2] == 0.f && v[0][3] == 0.8f);  // too fast: zero, and it counts
      EXPECT(v[1][0] == -10000.f && v[1][1] == -10000.f && v[1][2] == -10000.f && v[1][3] == 0.55f);
    }
    // more pairs than the matrices hold: error 5, nothing matched; a dt outside (1e-5, 10): nothing matched, no error
    EXPECT(vel::associate(cl, dynseq, nd, last, 2, 0.1f, cost.data(), gate.data(), 3, v, &err) == 0 && err == 5);
    err = 0;
    EXPECT(vel::associate(cl, dynseq, nd, last, 2, 10.f, cost.data(), gate.data(), 16, v, &err) == 0 && err == 0);
    EXPECT(vel::associate(cl, dynseq, nd, last, 2, 0.00001f, cost.data(), gate.data(), 16, v, &err) == 0 && err == 0);
  }
  return 0;
}

// ---- the dynamic split ------------------------------------------------------------------------------------------------
static int split_case() {
  // small and low | too many points | AT the point bound | too high | AT the height bound | both
  const int   size[6] = {10, 201, 200, 8, 7, 300};
  const float cz[6]   = {0.5f, 0.5f, 1.0f, 1.6f, 1.5f, 2.0f};
  const float cx[6] = {}, cy[6] = {};
  const vel::Clusters cl = {6, size, cx, cy, cz};
  int   dynseq[6], off[6], total_dyn = -1, n_static = -1, err = 0;
  float v[VEL_MAX_DYN][4];
  const int nd = vel::dynamic_split(cl, /*n_ground*/ 11, dynseq, off, v, &total_dyn, &n_static, &err);
  const int want_seq[6] = {0, -1, 1, -1, 2, -1};
  const int want_off[6] = {0, 228, 10, 429, 210, 437};
  EXPECT(nd == 3 && err == 0 && total_dyn == 217 && n_static == 509);
  for (int c = 0; c < 6; ++c) EXPECT(dynseq[c] == want_seq[c] && off[c] == want_off[c]);
  for (int r = 0; r < 3; ++r) EXPECT(v[r][0] == -10000.f && v[r][1] == -10000.f && v[r][2] == -10000.f && v[r][3] == 0.55f);
  // the hand-over keeps the possibly-dynamic ones, in order, with their intensity
  float last[VEL_MAX_DYN][5] = {};
  v[1][3] = 0.7f;
  EXPECT(vel::hand_over(cl, dynseq, v, last) == 3);
  EXPECT(last[0][4] == 10.f && last[1][4] == 200.f && last[2][4] == 7.f);
  EXPECT(last[0][2] == 0.5f && last[1][2] == 1.0f && last[2][2] == 1.5f);
  EXPECT(last[0][3] == 0.55f && last[1][3] == 0.7f && last[2][3] == 0.55f);
  return 0;
}

// ---- the LDS layout ---------------------------------------------------------------------------------------------------
static int lds_layout() {
  for (int mp : {1, 16, 7400, 8192}) {
    const size_t bytes = vel::Lds::bytes(mp);
    EXPECT(bytes == (size_t)20 * mp);  // 12 B of coordinates, a label and a scratch word per point
    std::vector<float> mem(bytes / sizeof(float));
    const vel::Lds     l(mem.data(), mp);
    const char        *at[6] = {(const char *)l.sx, (const char *)l.sy, (const char *)l.sz, (const char *)l.lab,
                                (const char *)l.aux, (const char *)mem.data() + bytes};
    EXPECT(at[0] == (const char *)mem.data());
    for (int k = 0; k < 5; ++k) EXPECT(at[k + 1] - at[k] == (long)mp * 4);  // disjoint, ordered, ending at bytes(max_pts)
  }
  return 0;
}

int main() {
  if (sort_cases()) return 1;
  if (assignment_cases()) return 1;
  if (association_cases()) return 1;
  if (split_case()) return 1;
  if (lds_layout()) return 1;
  std::printf("dsp velocity rules host ok\n");
  return 0;
}
