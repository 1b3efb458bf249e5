// sogm_qp_layout.hpp — the memory plan of one agent's QP solve (sogm_qp.hip), described ONCE: which iteration runs, what
// sits where in the workgroup's dynamic LDS and in the agent's HBM scratch, and what aliases what.  The planner sizes the
// scratch buffers from it, sogm_debug_qp_layout evaluates it on the host, tests/qp_layout_host_test.cpp reads it with the host
// compiler.  qp_solve_agent takes struct Rows, the byte totals and every constant of the path choice from here; the ORDER of
// the row arrays (carve_rows) and the pointers of its prologue are still its own (why: the note above carve_rows in
// sogm_qp.hip), so no carve is offered here; tests/test_qp_gpu.py holds the path each solve reports to QpLayout's.
//
// Dynamic LDS, general iteration:            Kb [n][18] K band / Cholesky factor | P [M][225] scaled cost blocks | rows
// Dynamic LDS, register-resident iteration:  P | Dv | V | Z  ([M][225] each) | hot rows | cold rows | K1 [n][18]
//   K is block tridiagonal in 15 x 15 piece blocks (the profile of the continuity rows) and its inverse is built block by
//   block (factor()): Dv the diagonal blocks of K, then inv(D_i); V the blocks K(i, i-1), then V_i; Z one block row of
//   K^-1; K1 the band of A^T diag(rho / rho_cur) A.
//   Aliasing: Dv | V | Z are dead between two factorisations; the termination check stages c_sy [S] | c_gy [G] (every
//   row's y) | c_red [32][10] (its partial reductions) there, from Dv on.  `fast` requires that this fits.
// The rows: the "hot" arrays are the only row data the register-resident iteration touches and live in LDS whenever it
// runs; the "cold" rest and K1 sit in LDS when everything fits and in HBM otherwise — the agent's scratch, laid out
// hot | cold (the hot part stays unused while the hot rows are in LDS), and the agent's K1 scratch.  The general
// iteration keeps all rows together, in LDS or in the scratch.
#pragma once
#include <cstddef>
#include "../../include/sogm_abi.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define QP_HD __host__ __device__ __forceinline__  // (a layout held in memory would cost a kernel its registers)
#define QP_HDI __host__ __device__ inline
#else
#define QP_HD inline
#define QP_HDI inline
#endif

namespace sogm {

constexpr int QP_BW  = 17;  // half bandwidth of K
constexpr int QP_ELL = 6;   // non-zeros of a general row

// The sizes of one problem: M pieces, `faces` corridor faces over all of them.
struct QpShape {
  int M, n;        // pieces, variables (15 per piece)
  int R1, R3, R4;  // general rows: [0, R3) continuity in three kinds of R1, [R3, R4) velocity boxes, [R4, G) acceleration boxes
  int G, S;        // general rows 9 (M + 1) + 21 M; safety rows, 5 per face
  QP_HD QpShape(int pieces, int faces)
      : M(pieces), n(15 * pieces), R1(3 * (pieces + 1)), R3(9 * (pieces + 1)), R4(R3 + 12 * pieces), G(R4 + 9 * pieces),
        S(5 * faces) {}
};

// The row arrays, in storage order: X(name, rows in {G, S}, elements per row, element type, hot).
//   general rows [0, G);  safety rows [0, S): s = off_i + 5 * face + k, columns i * 15 + k * 3 + {0, 1, 2}
#define QP_ROW_ARRAYS(X)                                                                                      \
  X(sval, S, 3, double, true)       /* the face normal */                                                     \
  X(sw, S, 1, double, true)         /* rho z - y: refreshed by the row update, read by the next A^T product */ \
  X(gw, G, 1, double, true)         /* the same of the general rows */                                        \
  X(gval, G, QP_ELL, double, false) /* ELL values */                                                          \
  X(gl, G, 1, double, false)                                                                                  \
  X(gu, G, 1, double, false)                                                                                  \
  X(grho, G, 1, double, false)                                                                                \
  X(gE, G, 1, double, false)                                                                                  \
  X(gz, G, 1, double, false)                                                                                  \
  X(gy, G, 1, double, false)                                                                                  \
  X(gdy, G, 1, double, false)                                                                                 \
  X(grinv, G, 1, double, false) /* 1 / rho (OSQP rho_inv_vec) */                                              \
  X(su, S, 1, double, false)                                                                                  \
  X(sE, S, 1, double, false)                                                                                  \
  X(sz, S, 1, double, false)                                                                                  \
  X(sy, S, 1, double, false)                                                                                  \
  X(sdy, S, 1, double, false)                                                                                 \
  X(gcol, G, QP_ELL, int, false) /* ELL columns, -1 = no entry */                                             \
  X(sc0, S, 1, int, false)       /* first column of the row's control point */                                \
  X(cidx, G, QP_ELL, int, false) /* CSC entries over general rows: row * 8 + slot, row-sorted inside a column */

struct Rows {
#define X(name, rows, per, T, hot) T *name;
  QP_ROW_ARRAYS(X)
#undef X
};

// bytes that one general (`of` = 'G') or one safety ('S') row takes in the hot or in the cold arrays
constexpr size_t row_bytes(char of, bool want_hot) {
  constexpr char G = 'G', S = 'S';
  size_t         b = 0;
#define X(name, rows, per, T, hot) \
  if (rows == of && hot == want_hot) b += per * sizeof(T);
  QP_ROW_ARRAYS(X)
#undef X
  return b;
}
static_assert(row_bytes('S', true) % sizeof(double) == 0 && row_bytes('G', true) % sizeof(double) == 0, "the hot arrays hold doubles");
// Byte totals of G general and S safety rows; qp_solve_agent places the cold rows, and the planner sizes the scratch, with
// these.  (Plain inline, and hot counted in doubles: the kernel's code depends on the shape of this arithmetic.)
QP_HDI size_t rows_hot_bytes(int G, int S) {
  return ((size_t)S * (row_bytes('S', true) / sizeof(double)) + G * (row_bytes('G', true) / sizeof(double))) * sizeof(double);
}
QP_HDI size_t rows_cold_bytes(int G, int S) {  // (+ a tail nobody reads)
  return (size_t)G * row_bytes('G', false) + (size_t)S * row_bytes('S', false) + 64;
}
QP_HDI size_t rows_bytes(int G, int S) { return rows_hot_bytes(G, S) + rows_cold_bytes(G, S); }

constexpr int QP_FAST_MAX_PIECES = 8;  // the block form of the factor: rows of K^-1 in registers, 30 entries per lane
constexpr int QP_FAST_MAX_G = 256;     // one general row per lane of waves 0-3
constexpr int QP_FAST_MAX_S = 1024;    // four safety rows per lane of waves 4-7
constexpr int QP_CHECK_RED = 32 * 10;  // c_red: ten partial results of each of the workgroup's 32 sixteen-lane rows

struct QpLayout {
  QpShape sh;
  bool    fast;         // the register-resident iteration runs
  bool    rows_in_lds;  // every row array (and, if fast, K1) is in LDS; else the cold rows — all rows if !fast — and K1 are in HBM
  // byte offsets in dynamic LDS.  Kb only if !fast; Dv, V, Z, check only if fast; cold and k1 only if rows_in_lds, hot also if fast
  size_t Kb, P, Dv, V, Z, hot, cold, k1, check;
  // byte offsets in the agent's scratch (if !rows_in_lds; hot only if also !fast); K1 starts the agent's K1 scratch
  size_t scr_hot, scr_cold;

  QP_HD size_t block_bytes() const { return (size_t)sh.M * 225 * sizeof(double); }
  QP_HD size_t band_bytes() const { return (size_t)sh.n * (QP_BW + 1) * sizeof(double); }
  // the check's staging area against what it lies over
  QP_HD size_t check_doubles() const { return (size_t)(sh.G + sh.S) + QP_CHECK_RED; }
  QP_HD size_t block_area_doubles() const { return (size_t)sh.M * (225 * 3); }
  QP_HD size_t blocks_end() const { return 4 * block_bytes(); }  // P | Dv | V | Z: where the hot rows start if fast

  QP_HD QpLayout(const QpShape &shape, size_t dyn_lds_bytes) : sh(shape) {
    const size_t hot_b = rows_hot_bytes(sh.G, sh.S), rows_al = (rows_bytes(sh.G, sh.S) + 15) & ~(size_t)15;
    fast = sh.M <= QP_FAST_MAX_PIECES && sh.G <= QP_FAST_MAX_G && sh.S <= QP_FAST_MAX_S &&
           check_doubles() <= block_area_doubles() && blocks_end() + hot_b <= dyn_lds_bytes;
    Kb          = 0;
    P           = fast ? 0 : band_bytes();
    Dv          = block_bytes();  // (the four that exist only if fast: no select on `fast` in what the iteration addresses)
    V           = 2 * block_bytes();
    Z           = 3 * block_bytes();
    check       = Dv;
    hot         = fast ? blocks_end() : band_bytes() + block_bytes();
    cold        = hot + hot_b;
    k1          = hot + rows_al;
    rows_in_lds = k1 + (fast ? band_bytes() : 0) <= dyn_lds_bytes;
    scr_hot     = 0;
    scr_cold    = hot_b;
  }
  // bytes in use
  QP_HD size_t lds_bytes() const { return rows_in_lds ? k1 + (fast ? band_bytes() : 0) : fast ? cold : hot; }
  QP_HD size_t scratch_bytes() const { return rows_in_lds ? 0 : scr_cold + rows_cold_bytes(sh.G, sh.S); }
  QP_HD size_t k1_scratch_bytes() const { return fast && !rows_in_lds ? band_bytes() : 0; }
};

// HBM scratch of one agent: the largest problem the ABI takes with every row in scratch; K1 of the largest fast problem
inline size_t qp_scratch_bytes_per_agent(int max_faces) {
  return (QpLayout(QpShape(SOGM_MAX_PIECES, max_faces * SOGM_MAX_PIECES), 0).scratch_bytes() + 255) & ~(size_t)255;
}
inline size_t qp_k1_scratch_bytes_per_agent() { return QpLayout(QpShape(QP_FAST_MAX_PIECES, 0), 0).band_bytes(); }

#undef QP_HD
#undef QP_HDI

}  // namespace sogm
