// Host test of the rule "where did this replan end" (csrc/sogm_finish.hpp: replan_outcome, replan_outcome_of, replan_solved),
// compiled with the host compiler (the header's device bodies sit behind __HIPCC__).  The expected index of every combination
// is written out below by hand from the precedence — no path, no corridor, QP not solved, unsafe, else ok — and the five
// SOGM_CNT_* values appear as the literals 0-4: renumbering the enum fails this test.
#include "sogm_finish.hpp"

#include <cstdio>

using namespace sogm;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static const int kRet[3]    = {0, 1, 3};
static const int kNpoly[4]  = {-1, 0, 1, 16};
static const int kStatus[6] = {-100, -7, 0, 1, 2, 3};
// want[ret][npoly][status][safe], safe = {false, true}.  0 ok, 1 no path, 2 no corridor, 3 QP, 4 unsafe.
static const int want[3][4][6][2] = {
    // ret = 0: the search found no path, whatever the later stages' words hold
    {{{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}},    // npoly -1
     {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}},    // npoly 0
     {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}},    // npoly 1
     {{1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}}},   // npoly 16
    // ret = 1
    {{{2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}},    // npoly -1: no corridor
     {{2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}},    // npoly 0
     {{3, 3}, {3, 3}, {3, 3}, {4, 0}, {4, 0}, {3, 3}},    // npoly 1: status -100 -7 0 | 1 2 | 3
     {{3, 3}, {3, 3}, {3, 3}, {4, 0}, {4, 0}, {3, 3}}},   // npoly 16
    // ret = 3: any non-zero return of the search counts as a path
    {{{2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}},
     {{2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}, {2, 2}},
     {{3, 3}, {3, 3}, {3, 3}, {4, 0}, {4, 0}, {3, 3}},
     {{3, 3}, {3, 3}, {3, 3}, {4, 0}, {4, 0}, {3, 3}}},
};

int main() {
  EXPECT(SOGM_CNT_REPLAN_OK == 0 && SOGM_CNT_FAIL_SEARCH == 1 && SOGM_CNT_FAIL_CORRIDOR == 2 && SOGM_CNT_FAIL_QP == 3 &&
         SOGM_CNT_FAIL_UNSAFE == 4);
  int n = 0;
  for (int r = 0; r < 3; ++r)
    for (int p = 0; p < 4; ++p)
      for (int s = 0; s < 6; ++s)
        for (int safe = 0; safe < 2; ++safe, ++n) {
          const int ret = kRet[r], npoly = kNpoly[p], status = kStatus[s], w = want[r][p][s][safe];
          EXPECT(replan_outcome(ret, npoly, status, safe != 0) == w);
          // the form the device bodies call: the same index, and the status is read only behind a search and corridors
          int       reads = 0;
          const int lazy  = replan_outcome_of(ret, npoly, [&] { ++reads; return status; }, safe != 0);
          EXPECT(lazy == w);
          EXPECT(reads == ((ret != 0 && npoly > 0) ? 1 : 0));
          // "solved" is the outcome with safe = true being ok; "good" is the outcome being ok
          const bool solved = replan_solved(ret, npoly, [&] { return status; });
          EXPECT(solved == (want[r][p][s][1] == 0));
          EXPECT((solved && safe != 0) == (w == 0));
        }
  EXPECT(n == 144);
  std::printf("finish rules host ok\n");
  return 0;
}
