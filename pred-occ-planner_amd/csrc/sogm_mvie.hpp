// sogm_mvie.hpp — the corridor optimiser, device only: the maximum-volume inscribed ellipsoid of a polytope
// (firi::maxVolInsEllipsoid + costMVIE, plan_manager/include/sfc_gen/firi.hpp:44-365) with its 9-variable L-BFGS and
// Lewis-Overton line search (sfc_gen/lbfgs.hpp) and the 3x3 Jacobi eigen-solver, executed by one wave.  Included by
// sogm_corridor.hpp, whose corridor_segment_body is the only caller; nothing here knows about maps, routes or agents.
// SOGM_PROFILE_MVIE builds: the timer words below exist once per translation unit that includes this header.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "../../include/sogm_detmath.h"

namespace sogm {
namespace {

// ---------------------------------------------------------------------------------------------
// MVIE (firi.hpp:44-236) — lane 0 only
// ---------------------------------------------------------------------------------------------
__device__ inline bool smoothedL1(double mu, double x, double &f, double &df) {
  if (x < 0.0) return false;
  if (x > mu) {
    f  = x - 0.5 * mu;
    df = 1.0;
    return true;
  }
  const double xdmu = x / mu, sqrxdmu = xdmu * xdmu, mumxd2 = mu - 0.5 * x;
  f  = mumxd2 * sqrxdmu * xdmu;
  df = sqrxdmu * ((-0.5) * xdmu + 3.0 * mumxd2 / mu);
  return true;
}

struct MvieData {
  int    M;
  double smoothEps, penaltyWt;
  // this lane's faces (lane and lane + 64); a face beyond M is flagged off
  double a0[3], a1[3];
  bool   on0, on1;
};

#ifdef SOGM_PROFILE_MVIE
__device__ unsigned long long g_mvie_prof[2];  // profiling build only: ticks (100 MHz) and calls of costMVIE
__device__ unsigned long long g_lbfgs_prof[5];  // line-search ticks, direction-update ticks, iterations, history entries, ticks of the two loops alone
#endif
__device__ inline double lane_f64(double v, int l) {  // value of lane l (l wave-uniform)
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo     = __builtin_amdgcn_readlane(lo, l);
  hi     = __builtin_amdgcn_readlane(hi, l);
  return __hiloint2double(hi, lo);
}
// N independent IEEE fp64 divisions x[i] / y[i], stage by stage: the instruction sequence the compiler expands "x / y" to
// (v_div_scale of the denominator and of the numerator, v_rcp, two Newton steps on the reciprocal, the quotient, its
// residual, v_div_fmas, v_div_fixup — LLVM's LowerFDIV64), so every quotient has the bits of the plain division; written
// out because the expansion passes its scale flag through VCC, which makes the compiler emit N divisions as N chains of
// thirteen dependent instructions one after the other — on a wave that is alone on its SIMD and issues in order, N times
// ~110 cycles.  Stage-wise the chains overlap (the flags live in ordinary scalar registers until their v_div_fmas).
template <int N>
__device__ __forceinline__ void div_n(const double (&x)[N], const double (&y)[N], double (&q)[N]) {
  double s0[N], s1[N], r[N], e[N], m[N];
  bool   fl[N], unused;
#pragma unroll
  for (int i = 0; i < N; ++i) s0[i] = __builtin_amdgcn_div_scale(x[i], y[i], false, &unused);  // the denominator, scaled
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = __builtin_amdgcn_rcp(s0[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) s1[i] = __builtin_amdgcn_div_scale(x[i], y[i], true, &fl[i]);  // the numerator, scaled
#pragma unroll
  for (int i = 0; i < N; ++i) e[i] = __builtin_fma(-s0[i], r[i], 1.0);
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = __builtin_fma(r[i], e[i], r[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) e[i] = __builtin_fma(-s0[i], r[i], 1.0);
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = __builtin_fma(r[i], e[i], r[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = s1[i] * r[i];
#pragma unroll
  for (int i = 0; i < N; ++i) e[i] = __builtin_fma(-s0[i], m[i], s1[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) q[i] = __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(e[i], r[i], m[i], fl[i]), y[i], x[i]);
}

// one face's terms of cost and gradient (firi.hpp:105-122); false when smoothedL1 rejects the face.  The face's five
// divisions — A L / ||A L|| and the two of smoothedL1's cubic branch (firi.hpp's x / mu and 3 (mu - x / 2) / mu, evaluated
// whether or not the branch is the lane's: some lane of the wave takes it) — go through div_n together.
__device__ inline bool mvie_face(const double a[3], const double L[3][3], const double *p,
                                 double smoothEps, double t[10]) {
  double AL[3];
  for (int j = 0; j < 3; ++j) AL[j] = (a[0] * L[0][j] + a[1] * L[1][j]) + a[2] * L[2][j];
  const double normAL = sogm_det::sqrt_rn((AL[0] * AL[0] + AL[1] * AL[1]) + AL[2] * AL[2]);
  const double Ap     = (a[0] * p[0] + a[1] * p[1]) + a[2] * p[2];
  const double viola  = (normAL + Ap) - 1.0;
  const double mu = smoothEps, mumxd2 = mu - 0.5 * viola;
  const double nx[5] = {AL[0], AL[1], AL[2], viola, 3.0 * mumxd2}, ny[5] = {normAL, normAL, normAL, mu, mu};
  double       qd[5];
  div_n<5>(nx, ny, qd);
  const double adj[3] = {qd[0], qd[1], qd[2]};
  double       c, dc;
  // smoothedL1(mu, viola, c, dc) with its two quotients taken from above
  if (viola < 0.0) return false;
  if (viola > mu) {
    c  = viola - 0.5 * mu;
    dc = 1.0;
  } else {
    const double xdmu = qd[3], sqrxdmu = xdmu * xdmu;
    c  = mumxd2 * sqrxdmu * xdmu;
    dc = sqrxdmu * ((-0.5) * xdmu + qd[4]);
  }
  t[0]                = c;
  const double vec[3] = {dc * a[0], dc * a[1], dc * a[2]};
  for (int j = 0; j < 3; ++j) t[1 + j] = vec[j];
  for (int j = 0; j < 3; ++j) t[4 + j] = adj[j] * vec[j];
  t[7] = adj[0] * vec[1];
  t[8] = adj[1] * vec[2];
  t[9] = adj[0] * vec[2];
  return true;
}

// costMVIE (firi.hpp:74-140), evaluated by the whole wave: one face per lane (two when M > 64).  The ten sums
// over faces (cost, gdp, gdrtd, gdcde) are accumulated IN THE REFERENCE'S ORDER — one running sum per quantity,
// faces in index order, only the faces smoothedL1 accepts (:111-122): the accepted faces' terms are compacted in
// face order into LDS (`terms`, >= 10 * M doubles: the LP work area, idle during the L-BFGS), lanes 0..9 each
// run one of the ten chains (usually a handful of dependent adds: few faces touch the ellipsoid), the totals are
// broadcast.  Every lane returns the same cost and gradient, bit-identical to the sequential loop.
__device__ __forceinline__ double costMVIE(const MvieData &D, const double *x, double *g, double *terms) {
  const int     lane = threadIdx.x & 63;
  const double *p = x, *rtd = x + 3, *cde = x + 6;
  double       *gdp = g, *gdrtd = g + 3, *gdcde = g + 6;
  double L[3][3];
  L[0][0] = rtd[0] * rtd[0] + DBL_EPSILON;
  L[0][1] = 0.0;
  L[0][2] = 0.0;
  L[1][0] = cde[0];
  L[1][1] = rtd[1] * rtd[1] + DBL_EPSILON;
  L[1][2] = 0.0;
  L[2][0] = cde[2];
  L[2][1] = cde[1];
  L[2][2] = rtd[2] * rtd[2] + DBL_EPSILON;
  // log and reciprocal of the three diagonal entries (the barrier term, used at the end): one entry per lane (lanes
  // 0..2; the others repeat entry 0) instead of three chains one after the other on the single wave of a SIMD, and
  // issued here, where the face terms' own dependent chains leave issue slots free; same functions, same inputs
  const double Ld = lane == 1 ? L[1][1] : (lane == 2 ? L[2][2] : L[0][0]);
  const double lg = sogm_det::log(Ld), rc = 1.0 / Ld;
  double t0[10], t1[10];
  bool   a0 = false, a1 = false;
  if (D.on0) a0 = mvie_face(D.a0, L, p, D.smoothEps, t0);
  if (D.on1) a1 = mvie_face(D.a1, L, p, D.smoothEps, t1);
  const unsigned long long m0 = __ballot(a0), m1 = D.M > 64 ? __ballot(a1) : 0ull;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int                n0 = __popcll(m0), n = n0 + __popcll(m1);
  if (a0) {
    double *dst = terms + __popcll(m0 & below) * 10;
#pragma unroll
    for (int k = 0; k < 10; ++k) dst[k] = t0[k];
  }
  if (a1) {
    double *dst = terms + (n0 + __popcll(m1 & below)) * 10;
#pragma unroll
    for (int k = 0; k < 10; ++k) dst[k] = t1[k];
  }
  wave_lds_sync();
  double sum = 0.0;
  if (lane < 10) {
    // the running sum in face order, its LDS reads four at a time (read one, wait, add one was a chain of LDS latencies
    // as long as the number of faces the ellipsoid touches); a row beyond n re-reads row n - 1 and is not added
    const double *src = terms + lane;
    for (int r = 0; r < n; r += 4) {
      double t4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t4[u] = src[(r + u < n ? r + u : n - 1) * 10];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double t = sum + t4[u];
        sum            = r + u < n ? t : sum;
      }
    }
  }
  wave_lds_sync();  // the next evaluation overwrites `terms`
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = lane_f64(sum, k);
  double cost = acc[0];
  for (int j = 0; j < 3; ++j) {
    gdp[j]   = acc[1 + j];
    gdrtd[j] = acc[4 + j];
    gdcde[j] = acc[7 + j];
  }
  cost *= D.penaltyWt;
  for (int j = 0; j < 3; ++j) {
    gdp[j] *= D.penaltyWt;
    gdrtd[j] *= D.penaltyWt;
    gdcde[j] *= D.penaltyWt;
  }
  cost -= lane_f64(lg, 0) + lane_f64(lg, 1) + lane_f64(lg, 2);
  gdrtd[0] -= lane_f64(rc, 0);
  gdrtd[1] -= lane_f64(rc, 1);
  gdrtd[2] -= lane_f64(rc, 2);
  gdrtd[0] *= 2.0 * rtd[0];
  gdrtd[1] *= 2.0 * rtd[1];
  gdrtd[2] *= 2.0 * rtd[2];
  return cost;
}

__device__ inline double dotn9(const double *a, const double *b) {
  double s = 0;
  for (int i = 0; i < 9; ++i) s += a[i] * b[i];
  return s;
}
__device__ inline double ninf9(const double *v) {
  // (max |v_i| from +0: v_max_f64 with the |x| operand modifier gives the value of "dabs(v[i]) > mx ? dabs(v[i]) : mx" for
  //  every finite input — a compare, a sign flip and four selects per element otherwise, twice per L-BFGS iteration on
  //  a wave that issues in order)
  double mx = 0;
  for (int i = 0; i < 9; ++i) mx = __builtin_fmax(mx, __builtin_fabs(v[i]));
  return mx;
}

#ifdef SOGM_PROFILE_MVIE
#define MVIE_PROF_ARG , long long *prof
#define MVIE_PROF_PASS , prof
#else
#define MVIE_PROF_ARG
#define MVIE_PROF_PASS
#endif
__device__ __forceinline__ int lineSearchLO(const MvieData &D, double *x, double &f, double *g, double &stp,
                            const double *s, const double *xp, const double *gp, double stpmin,
                            double stpmax, double *terms MVIE_PROF_ARG) {
  const double f_dec = 1.0e-4, s_curv = 0.9, machine_prec = 1.0e-16;
  const int    max_linesearch = 64;
  int          count = 0;
  bool         brackt = false, touched = false;
  double       mu = 0.0, nu = stpmax;
  if (!(stp > 0.0)) return -1;
  const double dginit = dotn9(gp, s);
  if (0.0 < dginit) return -2;
  const double finit = f, dgtest = f_dec * dginit, dstest = s_curv * dginit;
  while (true) {
    for (int i = 0; i < 9; ++i) x[i] = xp[i] + stp * s[i];
#ifdef SOGM_PROFILE_MVIE
    const long long tc0 = wall_clock64();
#endif
    f = costMVIE(D, x, g, terms);
#ifdef SOGM_PROFILE_MVIE
    prof[0] += wall_clock64() - tc0;
    prof[1] += 1;
#endif
    ++count;
    if (f != f || f == INFINITY || f == -INFINITY) return -3;
    if (f > finit + stp * dgtest) {
      nu     = stp;
      brackt = true;
    } else {
      if (dotn9(g, s) < dstest)
        mu = stp;
      else
        return count;
    }
    if (max_linesearch <= count) return -4;
    if (brackt && (nu - mu) < machine_prec * nu) return -5;
    if (brackt)
      stp = 0.5 * (mu + nu);
    else
      stp *= 2.0;
    if (stp < stpmin) return -6;
    if (stp > stpmax) {
      if (touched) return -7;
      touched = true;
      stp     = stpmax;
    }
  }
}

// L-BFGS (lbfgs.hpp lbfgs_optimize with the parameters of firi.hpp:191-199), executed replicated
// by every lane of the wave (uniform control flow; only costMVIE is lane-parallel).  Everything that
// is indexed dynamically lives in LDS with lane 0 as the single writer, so nothing spills to scratch:
//   lm = SegmentLds's `lm`: s history [18][9], then y history [18][9]
#define LBFGS_FENCE()                                        \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   \
    __builtin_amdgcn_wave_barrier();                         \
  } while (0)
__device__ __forceinline__ int lbfgsMVIE(const MvieData &D, double *x, double *lm, double *terms, int *n_iter,
                                         int *n_eval) {
  const int    n = 9, m = 18, past = 3;
  const double g_epsilon = 0.0, delta = 1.0e-7, min_step = 1.0e-32, max_step = 1.0e+20,
               cautious = 1.0e-6;
  double       xp[9], g[9], gp[9], d[9];
  double       pf0 = 0, pf1 = 0, pf2 = 0;  // pf[k % 3]
  const int    lane   = threadIdx.x & 63;
  const bool   writer = lane == 0;
  // s / y history in LDS (lane 0 writes an entry per iteration); the per-entry scalars y.s and alpha live in lane j
  // of two registers: written with a lane compare, read back with readlane, so the two-loop recursion contains no
  // LDS store and its history reads can be issued ahead of the dependent dot product / division / update.
  // (Also tried: the whole history in lane registers — 9.1 vs 8.7 us per iteration, 36 more AGPRs; prefetching the
  // next entry's vector one entry ahead — 9.3 us; a Markstein-corrected multiply by the stored reciprocal of y.s in
  // place of the division — 8.6 us: the compiler already starts the divisor's part of the division early.)
  double      *lm_s = lm, *lm_y = lm + m * n;
  double       ys_keep = 0.0, al_keep = 0.0;
#ifdef SOGM_PROFILE_MVIE
  long long prof[7] = {0, 0, 0, 0, 0, 0, 0};
#endif
  if (writer)
    for (int i = 0; i < 2 * m * n; ++i) lm[i] = 0;
  LBFGS_FENCE();
  double fx = costMVIE(D, x, g, terms);
  pf0       = fx;
  for (int i = 0; i < n; ++i) d[i] = -g[i];
  int          ret;
  // (g_epsilon is 0 here (firi.hpp:193): "||g||inf / max(1, ||x||inf) < 0" cannot hold — the quotient of a non-negative
  //  number and one >= 1 is non-negative or NaN — so with the constant the two norms and the division fold away;
  //  written so that a positive g_epsilon would bring the test back)
  auto grad_small = [&]() __attribute__((always_inline)) -> bool {
    if (!(g_epsilon > 0.0)) return false;
    const double xn = ninf9(x);
    return ninf9(g) / (1.0 > xn ? 1.0 : xn) < g_epsilon;
  };
  if (grad_small()) {
    ret = 0;
  } else {
    double step = 1.0 / sogm_det::sqrt_rn(dotn9(d, d));
    int    k = 1, end = 0, bound = 0;
    while (true) {
      for (int i = 0; i < n; ++i) {
        xp[i] = x[i];
        gp[i] = g[i];
      }
#ifdef SOGM_PROFILE_MVIE
      const long long tl0 = wall_clock64();
#endif
      const int ls = lineSearchLO(D, x, fx, g, step, d, xp, gp, min_step, max_step, terms MVIE_PROF_PASS);
#ifdef SOGM_PROFILE_MVIE
      prof[2] += wall_clock64() - tl0;
      prof[4] += 1;
      const long long tr0 = wall_clock64();
#endif
      *n_iter += 1;
      *n_eval += ls > 0 ? ls : 0;
      if (ls < 0) {
        for (int i = 0; i < n; ++i) {
          x[i] = xp[i];
          g[i] = gp[i];
        }
        ret = ls;
        break;
      }
      if (grad_small()) {
        ret = 0;
        break;
      }
      const int km = k % past;
      if (past <= k) {
        const double afx  = dabs(fx);
        const double pfk  = km == 0 ? pf0 : (km == 1 ? pf1 : pf2);
        const double rate = dabs(pfk - fx) / (1.0 > afx ? 1.0 : afx);
        if (rate < delta) {
          ret = 1;
          break;
        }
      }
      if (km == 0) pf0 = fx;
      else if (km == 1) pf1 = fx;
      else pf2 = fx;
      ++k;
      double  sv[9], yv[9];
      for (int i = 0; i < n; ++i) {
        sv[i] = x[i] - xp[i];
        yv[i] = g[i] - gp[i];
      }
      const double ys = dotn9(yv, sv);
      const double yy = dotn9(yv, yv);
      if (writer) {
        double *se = lm_s + end * n, *ye = lm_y + end * n;
        for (int i = 0; i < n; ++i) {
          se[i] = sv[i];
          ye[i] = yv[i];
        }
      }
      if (lane == end) ys_keep = ys;  // lm_ys[end]
      LBFGS_FENCE();
      for (int i = 0; i < n; ++i) d[i] = -g[i];
      const double cau = dotn9(sv, sv) * sogm_det::sqrt_rn(dotn9(gp, gp)) * cautious;
      // every lane holds the same values: make the bookkeeping provably wave-uniform (scalar branches, and
      // readlane needs a scalar lane index)
      if (__builtin_amdgcn_readfirstlane((int)(ys > cau))) {
#ifdef SOGM_PROFILE_MVIE
        const long long tw0 = wall_clock64();
#endif
        ++bound;
        bound = m < bound ? m : bound;
        end   = end + 1 == m ? 0 : end + 1;
        int j = end;
        // The two-loop recursion with d spread over the lanes: lane (row r, i) — i = lane & 15 < 9, every 16-lane DPP row
        // alike — holds d[i] and reads ITS element of s_j and y_j (two LDS reads per entry instead of eighteen); the nine
        // products of a dot product are one instruction, the update two, and the sum is taken in dotn9's order,
        // ((0 + p0) + p1) + ... + p8, by nine dependent v_fmac_f64_dpp with row_newbcast:k (acc += lane k's product x 1.0:
        // the product by one is exact, so each is the plain addition, rounded once) — every lane ends with the same sum.
        // 85 -> ~40 instructions per entry for a wave that is alone on its SIMD and issues in order; same operations on
        // the same values as the replicated form (polytopes stay bit-identical to the oracle's).
        const int ql  = (lane & 15) < n ? (lane & 15) : 0;
        double    dl  = d[0];
#pragma unroll
        for (int q = 1; q < n; ++q) dl = ql == q ? d[q] : dl;
        double one = 1.0;
        asm volatile("" : "+v"(one));
#define LBFGS_BC(K) "v_fmac_f64_dpp %0, %1, %2 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n\t"
        auto ordered_sum = [&](double p) __attribute__((always_inline)) -> double {
          double acc = 0.0;
          asm volatile("s_nop 1\n\t"  // (a VGPR written by the VALU needs two wait states before a DPP read)
                       LBFGS_BC(0) LBFGS_BC(1) LBFGS_BC(2) LBFGS_BC(3) LBFGS_BC(4) LBFGS_BC(5) LBFGS_BC(6) LBFGS_BC(7)
                       LBFGS_BC(8)
                       : "+v"(acc)
                       : "v"(p), "v"(one));
          return acc;
        };
#undef LBFGS_BC
        // (the next entry's two elements are read while the current entry's chain — product, ordered sum, division, update —
        //  runs: the address does not depend on it, and read at the top of its own trip the LDS latency stood in front of
        //  every entry.  The read past the last entry of a loop is of a valid slot and unused.)
        int    jn = j == 0 ? m - 1 : j - 1;
        double ns = lm_s[jn * n + ql], ny = lm_y[jn * n + ql];
        double hsq = 0.0, hyq = 0.0;
        for (int i = 0; i < bound; ++i) {
          j   = jn;
          hsq = ns;
          hyq = ny;
          jn  = j == 0 ? m - 1 : j - 1;
          ns  = lm_s[jn * n + ql];
          ny  = lm_y[jn * n + ql];
          const double alpha = ordered_sum(hsq * dl) / lane_f64(ys_keep, j);
          if (lane == j) al_keep = alpha;  // lm_alpha[j]
          dl += (-alpha) * hyq;
        }
        dl *= ys / yy;
        jn = j;  // the second loop starts at the entry the first one ended with: its elements are still in hsq / hyq
        ns = hsq;
        ny = hyq;
        for (int i = 0; i < bound; ++i) {
          j   = jn;
          hsq = ns;
          hyq = ny;
          jn  = j + 1 == m ? 0 : j + 1;
          ns  = lm_s[jn * n + ql];
          ny  = lm_y[jn * n + ql];
          const double beta = ordered_sum(hyq * dl) / lane_f64(ys_keep, j);
          const double al   = lane_f64(al_keep, j);
          dl += (al - beta) * hsq;
        }
#pragma unroll
        for (int q = 0; q < n; ++q) d[q] = lane_f64(dl, q);
#ifdef SOGM_PROFILE_MVIE
        prof[6] += wall_clock64() - tw0;
#endif
      }
      step = 1.0;
#ifdef SOGM_PROFILE_MVIE
      prof[3] += wall_clock64() - tr0;
      prof[5] += bound;
#endif
    }
  }
#ifdef SOGM_PROFILE_MVIE
  if (writer) {
    atomicAdd(&g_mvie_prof[0], (unsigned long long)prof[0]);
    atomicAdd(&g_mvie_prof[1], (unsigned long long)prof[1]);
    atomicAdd(&g_lbfgs_prof[0], (unsigned long long)prof[2]);
    atomicAdd(&g_lbfgs_prof[1], (unsigned long long)prof[3]);
    atomicAdd(&g_lbfgs_prof[2], (unsigned long long)prof[4]);
    atomicAdd(&g_lbfgs_prof[3], (unsigned long long)prof[5]);
    atomicAdd(&g_lbfgs_prof[4], (unsigned long long)prof[6]);
  }
#endif
  return ret;
}

__device__ void jacobiEig3(double S[3][3], double V[3][3], double w[3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = dabs(S[0][1]) + dabs(S[0][2]) + dabs(S[1][2]);
    const double dia = dabs(S[0][0]) + dabs(S[1][1]) + dabs(S[2][2]);
    if (off <= 1e-300 || off <= 1e-17 * dia) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (S[p][q] == 0.0) continue;
        const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
        const double t =
            (theta >= 0 ? 1.0 : -1.0) / (dabs(theta) + sogm_det::sqrt_rn(theta * theta + 1.0));
        const double c = 1.0 / sogm_det::sqrt_rn(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {
          const double skp = S[k][p], skq = S[k][q];
          S[k][p] = c * skp - s * skq;
          S[k][q] = s * skp + c * skq;
        }
        for (int k = 0; k < 3; ++k) {
          const double spk = S[p][k], sqk = S[q][k];
          S[p][k] = c * spk - s * sqk;
          S[q][k] = s * spk + c * sqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 3; ++i) w[i] = S[i][i];
}

// maxVolInsEllipsoid (firi.hpp:146-236); hPoly: M x 4 in LDS.  Called by the WHOLE wave: the
// deepest-point LP and the final 3x3 SVD run on lane 0, the L-BFGS runs replicated on all lanes
// with the cost evaluated one face per lane.  R, p, r are meaningful on lane 0 only.
__device__ __forceinline__ bool maxVolInsEllipsoid(const double *hPoly, int M, double R[3][3], double p[3],
                                   double r[3], const LpScratch &sc, double *lm, double *sh, long long *dbg) {
  const int lane = threadIdx.x & 63;
  double   *Alp = sc.A(), *blp = sc.b();  // M x 4 (normalised rows, then the MVIE's A), M; lm, sh: SegmentLds's lm and handoff
  // deepest interior point: rows one per lane, LP solved by the whole wave
  for (int i = lane; i < M; i += 64) {
    const double *h  = hPoly + i * 4;
    const double  hn = sogm_det::sqrt_rn((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]);
    for (int j = 0; j < 3; ++j) Alp[i * 4 + j] = h[j] / hn;
    Alp[i * 4 + 3] = 1.0;
    blp[i]         = -h[3] / hn;
  }
  wave_lds_sync();
  const double clp[4] = {0, 0, 0, -1.0};
  double       xlp[4];
  const double maxdepth = -linprog_wave<4>(clp, M, Alp, blp, xlp, sc.work, sc.perm);
  wave_lds_sync();
  if (lane == 0) {
    const bool   ok = !(!(maxdepth > 0.0) || maxdepth == INFINITY || maxdepth == -INFINITY);
    sh[12]          = ok ? 1.0 : 0.0;
    if (ok) {
      const double interior[3] = {xlp[0], xlp[1], xlp[2]};
      // A = Alp / (blp - Alp interior), overwriting Alp's first three columns (stride 4)
      for (int i = 0; i < M; ++i) {
        double      *a   = Alp + i * 4;
        const double den = blp[i] - ((a[0] * interior[0] + a[1] * interior[1]) + a[2] * interior[2]);
        for (int j = 0; j < 3; ++j) a[j] = a[j] / den;
      }
      double Q[3][3], L[3][3];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          Q[i][j] = (R[i][0] * (r[0] * r[0]) * R[j][0] + R[i][1] * (r[1] * r[1]) * R[j][1]) +
                    R[i][2] * (r[2] * r[2]) * R[j][2];
      // chol3d (firi.hpp:44-55)
      L[0][0] = sogm_det::sqrt_rn(Q[0][0]);
      L[1][0] = 0.5 * (Q[0][1] + Q[1][0]) / L[0][0];
      L[1][1] = sogm_det::sqrt_rn(Q[1][1] - L[1][0] * L[1][0]);
      L[2][0] = 0.5 * (Q[0][2] + Q[2][0]) / L[0][0];
      L[2][1] = (0.5 * (Q[1][2] + Q[2][1]) - L[2][0] * L[1][0]) / L[1][1];
      L[2][2] = sogm_det::sqrt_rn(Q[2][2] - L[2][0] * L[2][0] - L[2][1] * L[2][1]);
      for (int j = 0; j < 3; ++j) sh[j] = p[j] - interior[j];
      sh[3] = sogm_det::sqrt_rn(L[0][0]);
      sh[4] = sogm_det::sqrt_rn(L[1][1]);
      sh[5] = sogm_det::sqrt_rn(L[2][2]);
      sh[6] = L[1][0];
      sh[7] = L[2][1];
      sh[8] = L[2][0];
      for (int j = 0; j < 3; ++j) sh[9 + j] = interior[j];
    }
  }
  __syncthreads();
  if (sh[12] == 0.0) {
    __syncthreads();
    return false;
  }
  MvieData D;
  D.M         = M;
  D.smoothEps = 1.0e-2;
  D.penaltyWt = 1.0e+3;
  D.on0       = lane < M;
  D.on1       = lane + 64 < M;
  for (int j = 0; j < 3; ++j) {
    D.a0[j] = D.on0 ? Alp[lane * 4 + j] : 0.0;
    D.a1[j] = D.on1 ? Alp[(lane + 64) * 4 + j] : 0.0;
  }
  double x[9];
  for (int j = 0; j < 9; ++j) x[j] = sh[j];
  const double interior[3] = {sh[9], sh[10], sh[11]};
  __syncthreads();
  int             n_it = 0, n_ev = 0;
  const long long tl0 = wall_clock64();
#ifdef SOGM_PROFILE_MVIE
  const long long tcl0 = clock64();
#endif
  const int       ret = lbfgsMVIE(D, x, lm, sc.work, &n_it, &n_ev);  // LP work area: idle by now
  if (dbg && lane == 0) {
    dbg[3] = n_it;
    dbg[4] = n_ev;
    dbg[9] = wall_clock64() - tl0;
#ifdef SOGM_PROFILE_MVIE
    dbg[11] = clock64() - tcl0;  // shader-clock cycles of the same interval: dbg[11] / dbg[9] x 100 MHz = shader clock
#endif
  }
  if (lane == 0) {
    double L[3][3];
    for (int j = 0; j < 3; ++j) p[j] = x[j] + interior[j];
    L[0][0] = x[3] * x[3];
    L[0][1] = 0.0;
    L[0][2] = 0.0;
    L[1][0] = x[6];
    L[1][1] = x[4] * x[4];
    L[1][2] = 0.0;
    L[2][0] = x[8];
    L[2][1] = x[7];
    L[2][2] = x[5] * x[5];
    double S[3][3], V[3][3], w[3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j)
        S[i][j] = (L[i][0] * L[j][0] + L[i][1] * L[j][1]) + L[i][2] * L[j][2];
    jacobiEig3(S, V, w);
    int ord[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2 - a; ++b)
        if (w[ord[b]] < w[ord[b + 1]]) {
          const int t = ord[b];
          ord[b]      = ord[b + 1];
          ord[b + 1]  = t;
        }
    double U[3][3], Sg[3];
    for (int c = 0; c < 3; ++c) {
      Sg[c] = sogm_det::sqrt_rn(w[ord[c]] > 0 ? w[ord[c]] : 0.0);
      for (int k = 0; k < 3; ++k) U[k][c] = V[k][ord[c]];
    }
    const double det = U[0][0] * (U[1][1] * U[2][2] - U[1][2] * U[2][1]) -
                       U[0][1] * (U[1][0] * U[2][2] - U[1][2] * U[2][0]) +
                       U[0][2] * (U[1][0] * U[2][1] - U[1][1] * U[2][0]);
    if (det < 0.0) {
      for (int k = 0; k < 3; ++k) {
        R[k][0] = U[k][1];
        R[k][1] = U[k][0];
        R[k][2] = U[k][2];
      }
      r[0] = Sg[1];
      r[1] = Sg[0];
      r[2] = Sg[2];
    } else {
      for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) R[k][c] = U[k][c];
      r[0] = Sg[0];
      r[1] = Sg[1];
      r[2] = Sg[2];
    }
  }
  __syncthreads();
  return ret >= 0;
}

}  // namespace
}  // namespace sogm
