// sogm_lp.hpp (included by sogm_corridor.hpp, sogm_finish.hpp and sogm_lp.hip) — the wave LP (sdlp's projective Seidel LP) and the dynamic LDS of the
// kernels that run it, each layout described ONCE: the kernels carve their pointers from it, the launchers take their byte
// count from it, tests/corridor_lds_host_test.cpp reads it with the host compiler (the device's code sits behind __HIPCC__).
#pragma once
#include <cstddef>
#include "../../include/sogm_abi.h"
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include "../../include/sogm_detmath.h"
#define LDS_HD __host__ __device__
#else
#define LDS_HD
#endif

namespace sogm {

#define LP_MAX_ROWS 153  // planes of one LP incl. sdlp's plane 0; keeps the segment kernel at 4 workgroups per CU (LDS <= 40 KB)
#define LP_WORK_DOUBLES (14 * LP_MAX_ROWS)  // planes of the four recursion levels: (5 + 4 + 3 + 2) per row
#define FIRI_MAX_H 128  // planes selected before truncation to max_faces
#define FIRI_DIRECT_BD_MAX 32  // boundary planes of sogm_firi_batched
#define RULES_MAX_FACES 64  // faces per polytope of sogm_corridor_rules_batched
#define DECONFLICT_MAX_ROWS (LP_MAX_ROWS - 9)  // 144 point rows, + 8 box rows + sdlp's plane 0
constexpr int PLANNER_MAX_FACES = 64;  // sogm_planner_create refuses a larger max_faces

// The LP wave's scratch as linprog_wave's callers hold it.  `work` is idle between two LPs: costMVIE parks its face terms
// there (10 per face), finish_agent the agent's control points (set A).
struct LpScratch {
  double *work;  // LP_WORK_DOUBLES
  double *rows;  // LP_MAX_ROWS * 5: the caller's constraints, A in front of b
  int    *perm;  // LP_MAX_ROWS: the insertion order
  LDS_HD double *A() const { return rows; }                    // [rows][D], D <= 4
  LDS_HD double *b() const { return rows + LP_MAX_ROWS * 4; }  // [rows]
};
// LDS of a wave that only solves LPs (k_corridor_finalize, k_safe_after_opt, the finishing blocks of k_worker_flow, k_linprog): work, rows, perm
struct LpLds {
  static constexpr int    work = 0, rows = work + LP_WORK_DOUBLES, end = rows + LP_MAX_ROWS * 5;  // in doubles
  static constexpr size_t perm = sizeof(double) * end;                                             // in bytes, as bytes()
  static constexpr size_t bytes() { return perm + sizeof(int) * LP_MAX_ROWS; }
  static LDS_HD LpScratch carve(void *smem) { return {(double *)smem + work, (double *)smem + rows, (int *)((char *)smem + perm)}; }
};
// LDS of a corridor segment's wave; MB = capacity of the boundary block (6: k_corridor_segment / _flow, k_flight_light; 32:
// k_firi_direct).  The LP's work and rows, then in doubles: lm (L-BFGS history), maxVolInsEllipsoid's hand-off words, alpha / ys,
// fH, poly, the small shared state, the flag words (one bit per obstacle point); then, at bytes that depend on pc_capacity, the
// LP's perm and 16 ints.  BETWEEN two segments k_worker_flow and k_flight_light lay LpLds over the same bytes (finalise,
// finish): its perm is then the head of lm, which only a running segment uses (asserted below).
template <int MB>
constexpr int firi_small_doubles() { return 34 + 9 * MB; }
template <int MB>
struct SegmentLds {
  enum : int {
    lm = LpLds::end, handoff = lm + 2 * 18 * 9, keep = handoff + 16, fH = keep + 36, poly = fH + FIRI_MAX_H * 4,
    small = poly + FIRI_MAX_H * 4,
    // the small state, from `small`: forward 9, fwd_a 3, fwd_b 3, p 3, the current plane 4, bd 4 MB, forwardB 3 MB, forwardD MB,
    // distDs MB, box (llc, lhc) 6, w (w0, w1 = a, b) 6
    fwd = 0, fa = 9, fb = 12, p = 15, fh = 18, bd = 22, fB = bd + 4 * MB, fD = fB + 3 * MB, dD = fD + MB, box = dD + MB, w = box + 6,
    small_n = MB == 6 ? 96 : w + 6,  // MB == 6: 88 used, 8 spare (the byte count every build so far has launched with)
    flags = small + small_n
  };
  static_assert(w + 6 == firi_small_doubles<MB>() && w + 6 <= small_n, "the small state's fields fill its block");
  static constexpr int    flag_words(int pc_capacity) { return (pc_capacity + 63) / 64; }
  static constexpr size_t perm(int pc_capacity) { return 8 * ((size_t)flags + (size_t)flag_words(pc_capacity)); }
  static constexpr size_t ints(int pc_capacity) { return perm(pc_capacity) + sizeof(int) * LP_MAX_ROWS; }
  static constexpr size_t bytes(int pc_capacity) { return ints(pc_capacity) + sizeof(int) * 16; }
};
// LDS of the rules hook (k_corridor_rules): the LP's work and rows, the segment's polytope, box and way-points, then perm
struct RulesLds {
  static constexpr int    poly = LpLds::end, box = poly + RULES_MAX_FACES * 4, w = box + 6;
  static constexpr size_t perm = sizeof(double) * (w + 6);
  static constexpr size_t bytes() { return perm + sizeof(int) * LP_MAX_ROWS; }
};
static_assert(LP_MAX_ROWS <= 193, "lp_move_to_front rotates three positions per lane");
static_assert(DECONFLICT_MAX_ROWS + 9 <= LP_MAX_ROWS, "deconfliction: point rows + 8 box rows + plane 0");
static_assert(2 * RULES_MAX_FACES + 1 <= LP_MAX_ROWS && 2 * PLANNER_MAX_FACES + 1 <= LP_MAX_ROWS, "two joined polytopes + plane 0");
static_assert(5 * SOGM_MAX_PIECES * 3 <= LP_WORK_DOUBLES, "finish_agent parks set A in the LP work area");
static_assert(10 * (LP_MAX_ROWS - 9) <= LP_WORK_DOUBLES, "costMVIE parks ten terms per face there");
static_assert(LpLds::perm % 8 == 0 && RulesLds::perm % 8 == 0, "doubles start on 8 bytes (all other offsets count doubles)");
static_assert(LpLds::bytes() <= sizeof(double) * SegmentLds<6>::fH, "the LP view between two segments ends inside lm");
static_assert(SegmentLds<6>::bytes(16384) <= 40960 && SegmentLds<FIRI_DIRECT_BD_MAX>::bytes(16384) <= 40960, "four workgroups per CU");


#ifdef __HIPCC__
namespace {

__device__ inline double dabs(double x) { return x < 0 ? -x : x; }

__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------
// sdlp::linprog<d> (traj_utils/include/traj_utils/sdlp.hpp:709-787) executed by a whole wave.
//
// Hohmeyer's projective Seidel LP: planes carry d+1 homogeneous coefficients, plane 0 is "x_d >= 0", the
// objective is n.x / d.x; a violated plane recurses into the problem on that plane with the coordinate of its
// largest coefficient eliminated (linfracprog<d>, :526-662), the 1-D problem is a wedge on the projective line
// (wedge / lp_base_case, :260-446).  All 64 lanes call with identical arguments; the arithmetic and every
// decision are those of the sequential code (same operation order as oracle/lp_oracle.cpp, bit for bit):
//   * sdlp's doubly linked list (next/prev, shared by all recursion levels) is the array ord[position] ->
//     plane; move_to_front (:132-150) of the plane at position q rotates ord[1..q] by one, and "continue with
//     the successor of the returned plane" is position q + 1 in either of its branches;
//   * opt does not change between two violated planes, so "the next violated plane in list order" is found 64
//     positions at a time with a ballot (first set bit = the sequential scan's hit); the same holds for the
//     wedge, whose state (cw, ccw) only changes at an "offensive" plane;
//   * the planes in front of the violated one are projected one per lane (:604-618);
//   * objective vectors and optima live in registers (compile-time indices, select chains for imax).
// Deviation from the reference (documented in DESIGN.md): the insertion order is a fixed LCG Fisher-Yates
// permutation of the row count instead of sdlp's process-global mt19937_64 (call-history dependent).
// ---------------------------------------------------------------------------------------------
#define SDLP_EPS 1.0e-12
enum { SDLP_MINIMUM = 0, SDLP_INFEASIBLE = 1, SDLP_UNBOUNDED = 2, SDLP_AMBIGUOUS = 3 };

// lp_no_con<d> (:97-129) incl. unit<d> (:76-94)
template <int D>
__device__ __forceinline__ int lp_no_con(const double (&nv)[D + 1], const double (&dv)[D + 1],
                                         double (&opt)[D + 1]) {
  double n_dot_d = 0.0, d_dot_d = 0.0;
#pragma unroll
  for (int i = 0; i <= D; ++i) {
    n_dot_d += nv[i] * dv[i];
    d_dot_d += dv[i] * dv[i];
  }
  if (d_dot_d < SDLP_EPS * SDLP_EPS) {
    n_dot_d = 0.0;
    d_dot_d = 1.0;
  }
#pragma unroll
  for (int i = 0; i <= D; ++i) opt[i] = -nv[i] + dv[i] * n_dot_d / d_dot_d;
  double mag = 0.0;
#pragma unroll
  for (int i = 0; i <= D; ++i) mag += opt[i] * opt[i];
  if (mag < (D + 1) * SDLP_EPS * SDLP_EPS) {
    opt[D] = 1.0;
    return SDLP_AMBIGUOUS;
  }
  mag = 1.0 / sogm_det::sqrt_rn(mag);
#pragma unroll
  for (int i = 0; i <= D; ++i) opt[i] *= mag;
  return SDLP_MINIMUM;
}

// move_to_front (:132-150) on the position array: the plane at position q goes to position 1
__device__ __forceinline__ void lp_move_to_front(int *ord, int q) {
  if (q > 1) {  // q == 0: plane 0; q == 1: already next[0]
    const int lane = threadIdx.x & 63;
    const int iq   = ord[q];
    const int r0 = 1 + lane, r1 = 65 + lane, r2 = 129 + lane;  // LP_MAX_ROWS <= 193 positions
    const int v0 = r0 < q ? ord[r0] : 0;
    const int v1 = r1 < q ? ord[r1] : 0;
    const int v2 = r2 < q ? ord[r2] : 0;
    wave_lds_sync();
    if (r0 < q) ord[r0 + 1] = v0;
    if (r1 < q) ord[r1 + 1] = v1;
    if (r2 < q) ord[r2 + 1] = v2;
    if (lane == 0) ord[1] = iq;
    wave_lds_sync();
  }
}

__device__ __forceinline__ double dot2(const double a[2], const double b[2]) { return a[0] * b[0] + a[1] * b[1]; }
__device__ __forceinline__ double cross2(const double a[2], const double b[2]) { return a[0] * b[1] - a[1] * b[0]; }
// unit2 (:61-73); b may alias a
__device__ __forceinline__ bool unit2(const double a[2], double b[2]) {
  const double a0 = a[0], a1 = a[1];
  const double mag = sogm_det::sqrt_rn(a0 * a0 + a1 * a1);
  if (mag < 2.0 * SDLP_EPS) return true;
  b[0] = a0 / mag;
  b[1] = a1 / mag;
  return false;
}

// lp_min_lin_rat (:152-258)
__device__ __forceinline__ void lp_min_lin_rat(bool degen, const double cw[2], const double ccw[2],
                                               const double nv[2], const double dv[2], double opt[2]) {
  const double d_cw = dot2(cw, dv), d_ccw = dot2(ccw, dv);
  const double n_cw = dot2(cw, nv), n_ccw = dot2(ccw, nv);
  bool take_cw;
  if (degen) {
    take_cw = n_cw / d_cw < n_ccw / d_ccw;
  } else if (dabs(d_cw) > 2.0 * SDLP_EPS && dabs(d_ccw) > 2.0 * SDLP_EPS) {
    if (d_cw * d_ccw > 0.0) {
      take_cw = n_cw / d_cw < n_ccw / d_ccw;
    } else {
      if (d_cw > 0.0) {
        opt[0] = -dv[1];
        opt[1] = dv[0];
      } else {
        opt[0] = dv[1];
        opt[1] = -dv[0];
      }
      return;
    }
  } else if (dabs(d_cw) > 2.0 * SDLP_EPS) {
    take_cw = n_ccw * d_cw > 0.0;
  } else if (dabs(d_ccw) > 2.0 * SDLP_EPS) {
    take_cw = !(n_cw * d_ccw > 2.0 * SDLP_EPS);
  } else {
    take_cw = cross2(dv, nv) > 0.0;
  }
  opt[0] = take_cw ? cw[0] : ccw[0];
  opt[1] = take_cw ? cw[1] : ccw[1];
}

// first position in [p, count) whose lane predicate holds (-1 if none); pred(r) is evaluated one position per lane
template <class F>
__device__ __forceinline__ int lp_first(int p, int count, F pred) {
  const int lane = threadIdx.x & 63;
  for (int base = p; base < count; base += 64) {
    const int                r  = base + lane;
    const bool               ok = r < count ? pred(r) : false;
    const unsigned long long mk = __ballot(ok);
    if (mk) return base + __ffsll((long long)mk) - 1;
  }
  return -1;
}

template <int D>
struct Lfp {
  // halves: LDS, stride D+1, indexed by plane; the list is ord[0..count).  work: planes of the lower levels.
  __device__ __forceinline__ static int solve(const double *halves, int count, const double (&nv_in)[D + 1],
                              const double (&dv_in)[D + 1], double (&opt)[D + 1], double *work, int *ord) {
    const int lane = threadIdx.x & 63;
    // the objective by value: a select between two entries of the CALLER's array would be folded into an
    // indexed load before inlining and demote that array to scratch memory
    double nv[D + 1], dv[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) {
      nv[j] = nv_in[j];
      dv[j] = dv_in[j];
    }
    double    val  = 0.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) val += dv[j] * dv[j];
    const bool d_vec_zero = val < (D + 1) * SDLP_EPS * SDLP_EPS;
    int        status     = lp_no_con<D>(nv, dv, opt);
    if (count <= 0) return status;
    double *new_halves = work;  // [LP_MAX_ROWS][D]
    int     p          = 0;
    while (p < count) {
      const int q = lp_first(p, count, [&](int r) {
        const double *pl = halves + ord[r] * (D + 1);
        double        v  = 0.0;
#pragma unroll
        for (int j = 0; j <= D; ++j) v += opt[j] * pl[j];
        return v < -(D + 1) * SDLP_EPS;
      });
      if (q < 0) break;
      const int     i  = ord[q];
      const double *pi = halves + i * (D + 1);
      double        pv[D + 1];
#pragma unroll
      for (int j = 0; j <= D; ++j) pv[j] = pi[j];
      int    imax = 0;  // findimax (:449-464); the imax-th entries of the plane and of both objective vectors
      double rmax = dabs(pv[0]), pmax = pv[0], nmax = nv[0], dmax = dv[0];  // ride along (no indexed access)
#pragma unroll
      for (int j = 1; j <= D; ++j) {
        const double ab = dabs(pv[j]);
        if (ab > rmax) {
          imax = j;
          rmax = ab;
          pmax = pv[j];
          nmax = nv[j];
          dmax = dv[j];
        }
      }
      if (i != 0) {  // project the planes in front of i (:604-618), one per lane
        const double fac = 1.0 / pmax;
        for (int r = lane; r < q; r += 64) {
          const int     j    = ord[r];
          const double *old  = halves + j * (D + 1);
          const double  crit = old[imax] * fac;
          double       *np   = new_halves + j * D;
#pragma unroll
          for (int l = 0; l < D; ++l) {
            const int k = l < imax ? l : l + 1;
            np[l]       = old[k] - (l < imax ? pv[l] : pv[l + 1]) * crit;
          }
        }
      }
      wave_lds_sync();
      double nn[D], nd[D];
      if (d_vec_zero) {  // vector_down (:485-507)
        double ve = 0.0, ee = 0.0;
#pragma unroll
        for (int j = 0; j <= D; ++j) {
          ve += nv[j] * pv[j];
          ee += pv[j] * pv[j];
        }
        const double fac = ve / ee;
#pragma unroll
        for (int l = 0; l < D; ++l) {
          nn[l] = (l < imax ? nv[l] : nv[l + 1]) - (l < imax ? pv[l] : pv[l + 1]) * fac;
          nd[l] = 0.0;
        }
      } else {  // plane_down (:509-524) for numerator and denominator
        const double critn = nmax / pmax;
        const double critd = dmax / pmax;
#pragma unroll
        for (int l = 0; l < D; ++l) {
          const double e = l < imax ? pv[l] : pv[l + 1];
          nn[l]          = (l < imax ? nv[l] : nv[l + 1]) - e * critn;
          nd[l]          = (l < imax ? dv[l] : dv[l + 1]) - e * critd;
        }
      }
      double nopt[D];
      status = Lfp<D - 1>::solve(new_halves, q, nn, nd, nopt, work + LP_MAX_ROWS * D, ord);
      if (status == SDLP_INFEASIBLE) return status;
      // vector_up (:466-483) then the inline unit (:641-651)
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j <= D; ++j) {
        const double lo = nopt[j < D ? j : 0];       // low_vector[j]     (used when j < imax)
        const double hi = nopt[j > 0 ? j - 1 : 0];   // low_vector[j - 1] (used when j > imax)
        const double v  = j < imax ? lo : hi;
        const double na = acc - pv[j] * v;
        acc             = j != imax ? na : acc;
        opt[j]          = v;
      }
      acc /= pmax;
#pragma unroll
      for (int j = 0; j <= D; ++j) opt[j] = j == imax ? acc : opt[j];
      double mag = 0.0;
#pragma unroll
      for (int j = 0; j <= D; ++j) mag += opt[j] * opt[j];
      mag = 1.0 / sogm_det::sqrt_rn(mag);
#pragma unroll
      for (int j = 0; j <= D; ++j) opt[j] *= mag;
      lp_move_to_front(ord, q);
      p = q + 1;
    }
    return status;
  }
};

// linfracprog<1> (:664-684) = lp_base_case (:378-446) over wedge (:260-375); halves stride 2
template <>
struct Lfp<1> {
  __device__ __forceinline__ static int solve(const double *halves, int count, const double (&nv)[2], const double (&dv)[2],
                              double (&opt)[2], double *, int *ord) {
    if (count <= 0) return lp_no_con<1>(nv, dv, opt);
    const double e2 = 2.0 * SDLP_EPS;
    double       cw[2], ccw[2];
    bool         degen = false;
    {  // the first plane of the list that is not (numerically) zero spans the initial half circle
      const int q0 = lp_first(0, count, [&](int r) {
        const double *h = halves + 2 * ord[r];
        return !(sogm_det::sqrt_rn(h[0] * h[0] + h[1] * h[1]) < e2);
      });
      if (q0 < 0) return lp_no_con<1>(nv, dv, opt);  // wedge: UNBOUNDED
      const double *h = halves + 2 * ord[q0];
      unit2(h, ccw);
      cw[0]  = ccw[1];
      cw[1]  = -ccw[0];
      ccw[0] = -cw[0];
      ccw[1] = -cw[1];
    }
    int p = 0;
    while (p < count) {
      const int q = lp_first(p, count, [&](int r) {
        const double *h    = halves + 2 * ord[r];
        const double  d_cw = dot2(cw, h), d_ccw = dot2(ccw, h);
        if (d_ccw >= e2) return d_cw <= -e2;
        if (d_cw >= e2) return d_ccw <= -e2;
        if (d_ccw <= -e2 && d_cw <= -e2) return true;
        return d_cw <= -e2 || d_ccw <= -e2 || cross2(cw, h) < 0.0;
      });
      if (q < 0) break;
      const double h[2]  = {halves[2 * ord[q]], halves[2 * ord[q] + 1]};
      const double d_cw = dot2(cw, h), d_ccw = dot2(ccw, h);
      if (d_ccw >= e2) {
        cw[0] = h[1];
        cw[1] = -h[0];
        unit2(cw, cw);
      } else if (d_cw >= e2) {
        ccw[0] = -h[1];
        ccw[1] = h[0];
        unit2(ccw, ccw);
      } else if (d_ccw <= -e2 && d_cw <= -e2) {
        return SDLP_INFEASIBLE;
      } else {
        if (d_cw <= -e2)
          unit2(ccw, cw);
        else if (d_ccw <= -e2)
          unit2(cw, ccw);
        degen = true;
      }
      lp_move_to_front(ord, q);
      p = q + 1;
      if (degen) break;
    }
    if (degen) {
      while (p < count) {
        const int q = lp_first(p, count, [&](int r) {
          const double *h = halves + 2 * ord[r];
          return dot2(cw, h) < -e2 || dot2(ccw, h) < -e2;
        });
        if (q < 0) break;
        const double h[2] = {halves[2 * ord[q]], halves[2 * ord[q] + 1]};
        const double d_cw = dot2(cw, h), d_ccw = dot2(ccw, h);
        if (d_cw < -e2) {
          if (d_ccw < -e2) return SDLP_INFEASIBLE;
          cw[0] = ccw[0];
          cw[1] = ccw[1];
        } else {
          ccw[0] = cw[0];
          ccw[1] = cw[1];
        }
        p = q + 1;
      }
    }
    // lp_base_case (:403-445)
    if (dabs(cross2(nv, dv)) < 2.0 * SDLP_EPS * SDLP_EPS) {
      if (dot2(nv, nv) < 2.0 * SDLP_EPS * SDLP_EPS || dot2(dv, dv) > 2.0 * SDLP_EPS * SDLP_EPS) {
        opt[0] = cw[0];
        opt[1] = cw[1];
        return SDLP_AMBIGUOUS;
      }
      if (!degen && cross2(cw, nv) <= 0.0 && cross2(nv, ccw) <= 0.0) {
        opt[0] = -nv[0];
        opt[1] = -nv[1];
      } else if (dot2(nv, cw) > dot2(nv, ccw)) {
        opt[0] = ccw[0];
        opt[1] = ccw[1];
      } else {
        opt[0] = cw[0];
        opt[1] = cw[1];
      }
      return SDLP_MINIMUM;
    }
    lp_min_lin_rat(degen, cw, ccw, nv, dv, opt);
    return SDLP_MINIMUM;
  }
};

// linprog<D> (:709-787): min c^T x s.t. A[i][0..D) x <= rhs[i]  (A row-major, stride D, in LDS).
// work: LP_WORK_DOUBLES doubles (LDS), ord: LP_MAX_ROWS ints (LDS); rows < LP_MAX_ROWS.
// Returns +inf infeasible, -inf unbounded / optimum at infinity, else the minimum.  Whole wave.
template <int D>
__device__ __forceinline__ double linprog_wave(const double *c, int rows, const double *A, const double *rhsv,
                                               double *x, double *work, int *ord) {
  const int lane = threadIdx.x & 63;
  for (int j = 0; j < D; ++j) x[j] = 0.0;
  if (rows <= 0) {
    double mx = 0;
    for (int j = 0; j < D; ++j) mx = dabs(c[j]) > mx ? dabs(c[j]) : mx;
    return mx > 0.0 ? -INFINITY : 0.0;
  }
  const int m      = rows + 1;
  double   *halves = work;  // [LP_MAX_ROWS][D + 1]
  if (lane == 0) {
    ord[0] = 0;
    for (int i = 0; i < rows; ++i) ord[1 + i] = i + 1;
    unsigned long long s = 0x9E3779B97F4A7C15ULL;  // the fixed insertion order (oracle: fixed_permutation)
    for (int i = rows - 1; i > 0; --i) {
      s           = s * 6364136223846793005ULL + 1442695040888963407ULL;
      const int j = (int)((s >> 33) % (unsigned long long)(i + 1));
      const int t = ord[1 + i];
      ord[1 + i]  = ord[1 + j];
      ord[1 + j]  = t;
    }
    for (int j = 0; j < D; ++j) halves[j] = 0.0;
    halves[D] = 1.0;
  }
  for (int i = 1 + lane; i < m; i += 64) {  // halves.col(i) = (-A_i, b_i) normalised (:737-740)
    const double *src = A + (i - 1) * D;
    double        h[D + 1];
#pragma unroll
    for (int j = 0; j < D; ++j) h[j] = -src[j];
    h[D]      = rhsv[i - 1];
    double nn = 0.0;
#pragma unroll
    for (int j = 0; j <= D; ++j) nn += h[j] * h[j];
    nn          = sogm_det::sqrt_rn(nn);
    double *dst = halves + i * (D + 1);
#pragma unroll
    for (int j = 0; j <= D; ++j) dst[j] = nn > 0.0 ? h[j] / nn : h[j];
  }
  wave_lds_sync();
  double nv[D + 1], dv[D + 1], opt[D + 1];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    nv[j] = c[j];
    dv[j] = 0.0;
  }
  nv[D] = 0.0;
  dv[D] = 1.0;
  const int status = Lfp<D>::solve(halves, m, nv, dv, opt, work + LP_MAX_ROWS * (D + 1), ord);
  double    minimum = INFINITY;
  if (status != SDLP_INFEASIBLE) {
    if (opt[D] != 0.0 && status != SDLP_UNBOUNDED) {
      minimum = 0.0;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        x[j] = opt[j] / opt[D];
        minimum += c[j] * x[j];
      }
    }
    if (opt[D] == 0.0 || status == SDLP_UNBOUNDED) {
#pragma unroll
      for (int j = 0; j < D; ++j) x[j] = opt[j];
      minimum = -INFINITY;
    }
  }
  return minimum;
}

}  // namespace
#endif
}  // namespace sogm
