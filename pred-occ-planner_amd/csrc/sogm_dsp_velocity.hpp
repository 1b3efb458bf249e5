// sogm_dsp_velocity.hpp — the rules of the velocity estimation (velocityEstimationThread, dsp_dynamic.h:1487-1678) that one
// lane of k_dsp_velocity (sogm_dsp_velocity.hip) runs, as plain C++ for host and device: the reference's constants, the
// kernel's dynamic-LDS layout, libstdc++'s std::sort restated (the ORDER OF TIES under that unstable sort is what the
// cluster order depends on), the possibly-dynamic split with the output offsets, and the gated association with the
// previous frame's clusters.  tests/dsp_velocity_rules_host_test.cpp builds it with the host compiler.
#pragma once
#include <cmath>
#include <cstddef>

#include "sogm_dsp.hpp"
#ifdef __HIPCC__
#define VEL_HD __host__ __device__
#else
#define VEL_HD
#endif

namespace sogm {
namespace vel {

// The reference's constants, values and types as it compares them.
constexpr int    MIN_CLUSTER_SIZE = 5, MAX_CLUSTER_SIZE = 10000;  // EuclideanClusterExtraction (:1517-1518)
constexpr int    DYNAMIC_CLUSTER_MAX_POINT_NUM     = 200;
constexpr double DYNAMIC_CLUSTER_MAX_CENTER_HEIGHT = 1.5;      // (a double: the fp32 centre height is promoted to compare)
constexpr float  DISTANCE_GATE                     = 1.5f;     // (:1563-1565)
constexpr int    POINT_NUM_GATE                    = 100;
constexpr float  MAXIMUM_VELOCITY                  = 5.f;
constexpr float  UNMATCHED_VELOCITY                = -10000.f;  // "no estimate": new-born particles draw a random velocity
constexpr float  DEFAULT_INTENSITY                 = 0.55f;
constexpr double DT_MIN = 0.00001, DT_MAX = 10.0;               // (:1575, compared in double)

// The kernel's dynamic LDS: the non-ground points' coordinates compacted in input order, a label and a scratch word per
// point.  After the clustering the coordinate arrays are free and hold the association's cost and gate matrices.
struct Lds {
  float *sx, *sy, *sz;
  int   *lab;  // component label (-> cluster slot later)
  int   *aux;  // sizes per root, then rank of a point inside its cluster
  VEL_HD Lds(void *base, int max_pts)
      : sx((float *)base), sy(sx + max_pts), sz(sy + max_pts), lab((int *)(sz + max_pts)), aux(lab + max_pts) {}
  VEL_HD static size_t bytes(int max_pts) { return (size_t)max_pts * (3 * sizeof(float) + 2 * sizeof(int)); }
};

// ---- std::sort(first, last, size <) of libstdc++ ---------------------------------------------------------------------
struct Item {
  int size, id;
};
VEL_HD inline bool less_(const Item &a, const Item &b) { return a.size < b.size; }
VEL_HD inline void swap_(Item &a, Item &b) {
  const Item t = a;
  a            = b;
  b            = t;
}
// libstdc++ <bits/stl_heap.h> __adjust_heap / __push_heap with comp = less_
VEL_HD inline void adjust_heap(Item *f, int hole, int len, Item value) {
  const int top = hole;
  int       child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (less_(f[child], f[child - 1])) child--;
    f[hole] = f[child];
    hole    = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child   = 2 * (child + 1);
    f[hole] = f[child - 1];
    hole    = child - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && less_(f[parent], value)) {
    f[hole] = f[parent];
    hole    = parent;
    parent  = (hole - 1) / 2;
  }
  f[hole] = value;
}
VEL_HD inline void heap_sort(Item *f, int n) {  // __partial_sort(first, last, last): make_heap + sort_heap
  if (n >= 2)
    for (int parent = (n - 2) / 2;; --parent) {
      adjust_heap(f, parent, n, f[parent]);
      if (parent == 0) break;
    }
  for (int last = n; last > 1; --last) {
    const Item v = f[last - 1];
    f[last - 1]  = f[0];
    adjust_heap(f, 0, last - 1, v);
  }
}
VEL_HD inline void unguarded_linear_insert(Item *f, int last) {
  const Item val = f[last];
  int        next = last - 1;
  while (less_(val, f[next])) {
    f[last] = f[next];
    last    = next;
    --next;
  }
  f[last] = val;
}
VEL_HD inline void insertion_sort(Item *f, int first, int last) {
  if (first == last) return;
  for (int i = first + 1; i != last; ++i) {
    if (less_(f[i], f[first])) {
      const Item val = f[i];
      for (int k = i; k > first; --k) f[k] = f[k - 1];
      f[first] = val;
    } else {
      unguarded_linear_insert(f, i);
    }
  }
}
// std::sort(first, last, less_) of libstdc++ (<bits/stl_algo.h>: __introsort_loop + __final_insertion_sort)
VEL_HD inline void std_sort(Item *f, int n) {
  if (n <= 0) return;
  int depth = 0;
  for (int t = n; t > 1; t >>= 1) ++depth;  // __lg(n)
  depth *= 2;
  // explicit stack for the recursion on the right part
  int st_first[40], st_last[40], st_depth[40], sp = 0;
  int first = 0, last = n, dl = depth;
  for (;;) {
    while (last - first > 16) {
      if (dl == 0) {
        heap_sort(f + first, last - first);
        break;
      }
      --dl;
      // __unguarded_partition_pivot
      const int mid = first + (last - first) / 2;
      {  // __move_median_to_first(first, first + 1, mid, last - 1)
        const int a = first + 1, b = mid, c = last - 1;
        if (less_(f[a], f[b])) {
          if (less_(f[b], f[c])) swap_(f[first], f[b]);
          else if (less_(f[a], f[c])) swap_(f[first], f[c]);
          else swap_(f[first], f[a]);
        } else if (less_(f[a], f[c])) swap_(f[first], f[a]);
        else if (less_(f[b], f[c])) swap_(f[first], f[c]);
        else swap_(f[first], f[b]);
      }
      int lo = first + 1, hi = last;
      for (;;) {  // __unguarded_partition(first + 1, last, first)
        while (less_(f[lo], f[first])) ++lo;
        --hi;
        while (less_(f[first], f[hi])) --hi;
        if (!(lo < hi)) break;
        swap_(f[lo], f[hi]);
        ++lo;
      }
      // recurse on [lo, last), continue with [first, lo)
      st_first[sp] = lo;
      st_last[sp]  = last;
      st_depth[sp] = dl;
      ++sp;
      last = lo;
    }
    if (sp == 0) break;
    --sp;
    first = st_first[sp];
    last  = st_last[sp];
    dl    = st_depth[sp];
  }
  if (n > 16) {  // __final_insertion_sort
    insertion_sort(f, 0, 16);
    for (int i = 16; i < n; ++i) unguarded_linear_insert(f, i);
  } else {
    insertion_sort(f, 0, n);
  }
}

// ---- the accepted clusters of a frame, in extraction order ------------------------------------------------------------
struct Clusters {
  int          nc;
  const int   *size;
  const float *cx, *cy, *cz;  // centres
};

// Possibly-dynamic split (:1544-1560) and the output offsets of input_cloud_with_velocity, which the reference orders
// [possibly-dynamic clusters][ground points][static clusters].  dynseq[c]: the cluster's row among the possibly-dynamic
// ones, or -1 (static, or past VEL_MAX_DYN: *err = 4); off[c]: where its points start; v[row]: "no estimate".
// Returns the number of possibly-dynamic clusters.
VEL_HD inline int dynamic_split(const Clusters &cl, int n_ground, int *dynseq, int *off, float (*v)[4], int *total_dyn,
                                int *n_static, int *err) {
  int nd = 0, o = 0;
  for (int c = 0; c < cl.nc; ++c) {
    const bool stat = cl.size[c] > DYNAMIC_CLUSTER_MAX_POINT_NUM || cl.cz[c] > DYNAMIC_CLUSTER_MAX_CENTER_HEIGHT;
    if (!stat && nd >= VEL_MAX_DYN) *err = 4;
    dynseq[c] = (!stat && nd < VEL_MAX_DYN) ? nd : -1;
    if (dynseq[c] >= 0) {
      off[c] = o;
      o += cl.size[c];
      v[nd][0] = UNMATCHED_VELOCITY;
      v[nd][1] = UNMATCHED_VELOCITY;
      v[nd][2] = UNMATCHED_VELOCITY;
      v[nd][3] = DEFAULT_INTENSITY;
      ++nd;
    }
  }
  *total_dyn = o;
  o += n_ground;
  for (int c = 0; c < cl.nc; ++c)
    if (dynseq[c] < 0) {
      off[c] = o;
      o += cl.size[c];
    }
  *n_static = o - *total_dyn - n_ground;
  return nd;
}

// Cost and gate of (new possibly-dynamic cluster r = cluster rows[r], old cluster c) (:1577-1597), R x C row-major.
VEL_HD inline void fill_cost_gate(const Clusters &cl, const int *rows, int R, const float (*last)[5], int C, float *cost,
                                  float *gate) {
  for (int r = 0; r < R; ++r)
    for (int c = 0; c < C; ++c) {
      const int   k  = rows[r];
      const float ex = cl.cx[k] - last[c][0], ey = cl.cy[k] - last[c][1], ez = cl.cz[k] - last[c][2];
      const float dist = sqrtf(ex * ex + ey * ey + ez * ez);
      const int   dn   = cl.size[k] - (int)last[c][4];
      if ((dn < 0 ? -dn : dn) > POINT_NUM_GATE || dist >= DISTANCE_GATE) {
        gate[r * C + c] = 0.f;
        cost[r * C + c] = DISTANCE_GATE * 5000.f;
      } else {
        gate[r * C + c] = 1.f;
        cost[r * C + c] = dist / DISTANCE_GATE * 1000.f;
      }
    }
}

// Minimum-cost assignment of an R x C cost matrix, potentials form, rows <= cols (transposed view otherwise), in the
// oracle's scan order.  pair(j, ..) reads the match of the view's column j = 1 .. ncols.
struct Assignment {
  int  pj[VEL_MAX_DYN + 1];  // the view's row (1-based) assigned to the view's column j, 0: none
  int  ncols;
  bool tr;
  VEL_HD bool pair(int j, int *r, int *c) const {  // new cluster r <-> old cluster c
    if (pj[j] <= 0) return false;
    *r = tr ? j - 1 : pj[j] - 1;
    *c = tr ? pj[j] - 1 : j - 1;
    return true;
  }
};
VEL_HD inline void assign(const float *cost, int R, int C, Assignment *out) {  // R, C <= VEL_MAX_DYN
  const bool  tr = R > C;
  const int   NR = tr ? C : R, NCc = tr ? R : C;
  const float INF = 3.0e38f;
  float u[VEL_MAX_DYN + 1], v[VEL_MAX_DYN + 1], minv[VEL_MAX_DYN + 1];
  int  *pj = out->pj, way[VEL_MAX_DYN + 1];
  bool  used[VEL_MAX_DYN + 1];
  for (int j = 0; j <= NCc; ++j) {
    v[j]  = 0.f;
    pj[j] = 0;
    way[j] = 0;
  }
  for (int i = 0; i <= NR; ++i) u[i] = 0.f;
  auto at = [&](int i, int j) { return tr ? cost[j * C + i] : cost[i * C + j]; };  // (row i, col j) of the NR x NCc view
  for (int i = 1; i <= NR; ++i) {
    pj[0]  = i;
    int j0 = 0;
    for (int j = 0; j <= NCc; ++j) {
      minv[j] = INF;
      used[j] = false;
    }
    do {
      used[j0]     = true;
      const int i0 = pj[j0];
      float     delta = INF;
      int       j1 = 0;
      for (int j = 1; j <= NCc; ++j)
        if (!used[j]) {
          const float cur = at(i0 - 1, j - 1) - u[i0] - v[j];
          if (cur < minv[j]) {
            minv[j] = cur;
            way[j]  = j0;
          }
          if (minv[j] < delta) {
            delta = minv[j];
            j1    = j;
          }
        }
      for (int j = 0; j <= NCc; ++j)
        if (used[j]) {
          u[pj[j]] += delta;
          v[j] -= delta;
        } else {
          minv[j] -= delta;
        }
      j0 = j1;
    } while (pj[j0] != 0);
    do {
      const int j1 = way[j0];
      pj[j0]       = pj[j1];
      j0           = j1;
    } while (j0);
  }
  out->ncols = NCc;
  out->tr    = tr;
}

// Velocity and intensity of every matched pair whose gate is open (:1603-1622); a pair faster than maximum_velocity
// reports zero and still counts.  Returns the number of matches.
VEL_HD inline int read_out(const Assignment &as, const float *gate, const Clusters &cl, const int *rows,
                           const float (*last)[5], int C, float dt, float (*v)[4]) {
  int matched = 0;
  for (int j = 1; j <= as.ncols; ++j) {
    int r, c;
    if (!as.pair(j, &r, &c)) continue;
    if (!(gate[r * C + c] > 0.01f)) continue;
    const int k = rows[r];
    float vx = (cl.cx[k] - last[c][0]) / dt, vy = (cl.cy[k] - last[c][1]) / dt, vz = (cl.cz[k] - last[c][2]) / dt;
    const float vv = sqrtf(vx * vx + vy * vy + vz * vz);
    if (vv > MAXIMUM_VELOCITY) vx = vy = vz = 0.f;
    v[r][0] = vx;
    v[r][1] = vy;
    v[r][2] = vz;
    v[r][3] = last[c][3];
    ++matched;
  }
  return matched;
}

// The association (:1562-1622) of this frame's R possibly-dynamic clusters with the C of the previous frame, dt apart.
// cost and gate: `cap` floats each (more pairs than that: *err = 5 and nothing is matched).  Returns the matches.
VEL_HD inline int associate(const Clusters &cl, const int *dynseq, int R, const float (*last)[5], int C, float dt,
                            float *cost, float *gate, int cap, float (*v)[4], int *err) {
  if (R * C > cap) *err = 5;
  if (!(R > 0 && C > 0 && R * C <= cap && dt > DT_MIN && dt < DT_MAX)) return 0;
  int rows[VEL_MAX_DYN];
  {
    int k = 0;
    for (int c = 0; c < cl.nc; ++c)
      if (dynseq[c] >= 0) rows[k++] = c;
  }
  fill_cost_gate(cl, rows, R, last, C, cost, gate);
  Assignment as;
  assign(cost, R, C, &as);
  return read_out(as, gate, cl, rows, last, C, dt, v);
}

// clusters_feature_vector_dynamic_last = clusters_feature_vector_dynamic (:1665).  Returns how many were handed over.
VEL_HD inline int hand_over(const Clusters &cl, const int *dynseq, const float (*v)[4], float (*last)[5]) {
  int k = 0;
  for (int c = 0; c < cl.nc; ++c)
    if (dynseq[c] >= 0) {
      last[k][0] = cl.cx[c];
      last[k][1] = cl.cy[c];
      last[k][2] = cl.cz[c];
      last[k][3] = v[k][3];
      last[k][4] = (float)cl.size[c];
      ++k;
    }
  return k;
}

}  // namespace vel
}  // namespace sogm
#undef VEL_HD
