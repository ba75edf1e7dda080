// sdm_walk.h — the walk of a segment through the map's cells, shared by the three kernels that walk one: k_query_segments
// (queries.hip), k_view_rays (views.hip) and k_query_forecast_segments (forecast.hip).  Only those three units include it.
//
// One lane per segment, a 3-D DDA in batches of SEG_K cells.
// The cells a segment visits follow from its end points alone; only "stop here" depends on the map.  So the DDA walks
// SEG_K cells ahead, the SEG_K loads are issued together, and then their results are tested: one memory round trip per
// SEG_K cells instead of one per cell (a 100-cell segment taken cell by cell would wait ~100 x 900 cycles).  Every load
// of a batch feeds the stop mask unconditionally, so none of them can be sunk behind an earlier cell's test.
// The DDA runs in double: crossing parameters t = (plane - u_a) * (1 / (u_b - u_a)) are computed fresh from the end
// points for every plane (no accumulated increments), so a cell sequence differs from the exact one only where two crossings lie
// within rounding of each other.
//
// The state is scalars per axis, never arrays, and no conditional operator ever has two of its members as operands: such
// an operator selects an address and the whole state lands in scratch memory (tests/test_isa_hygiene.py has the case).
#pragma once
#include "sdm_layer.h"

namespace sdm {

constexpr int SEG_K = 8;
enum : int { SEG_CELL = 0, SEG_OUT = 1, SEG_END = 2 };  // a cell of the map; the cell outside it the segment leaves into; nothing

struct SegAxis {
  int c, step, n;     // the current cell's coordinate; -1, 0, +1: the way the segment goes; the map's cells
  double A, inv, tn;  // u_a; 1 / (u_b - u_a), 0 where the segment is parallel to the planes; the t of the next plane
};
struct SegWalk {
  SegAxis x, y, z;
  double t_cur;  // the t at which the current cell was entered
  int kind;      // of the current cell
};
// what the set-up finds of a (finite) segment: a lies inside the map; the segment has no point in it (parallel to a slab
// that a lies outside of); the range of t inside all three slabs
struct SegClip {
  bool inside, empty;
  double t_in, t_out;
  __device__ __forceinline__ bool enters() const { return !empty && t_in <= 1.0 && t_out > 0.0 && t_in < t_out; }
};

__device__ __forceinline__ void seg_axis_begin(SegAxis &s, SegClip &cl, float ua, float ub, int n) {
  s.c = 0;
  s.n = n;
  s.A = (double)ua;
  const double D = (double)ub - s.A;
  cl.inside = cl.inside && ua >= 0.f && ua < (float)n;
  if (D == 0.0) {
    cl.empty = cl.empty || !(ua >= 0.f && ua < (float)n);
    s.inv = 0.0;
  } else {
    s.inv = 1.0 / D;
    const double t0 = (0.0 - s.A) * s.inv, t1 = ((double)n - s.A) * s.inv;
    cl.t_in = fmax(cl.t_in, fmin(t0, t1));
    cl.t_out = fmin(cl.t_out, fmax(t0, t1));
  }
  s.step = D > 0.0 ? 1 : (D < 0.0 ? -1 : 0);
}

// the set-up of a segment whose map-index end points ua, ub are finite: the slab clip in double; the walk has no cell yet
__device__ __forceinline__ SegClip seg_begin(SegWalk &w, const Dims &d, const float (&ua)[3], const float (&ub)[3]) {
  SegClip cl = {true, false, -INFINITY, INFINITY};
  w.t_cur = 0.0;
  w.kind = SEG_END;
  seg_axis_begin(w.x, cl, ua[0], ub[0], (int)d.NX);
  seg_axis_begin(w.y, cl, ua[1], ub[1], (int)d.NY);
  seg_axis_begin(w.z, cl, ua[2], ub[2], (int)d.NZ);
  return cl;
}
// the first cell is a's (a lies inside the map)
__device__ __forceinline__ void seg_enter_inside(SegWalk &w, const float (&ua)[3]) {
  w.kind = SEG_CELL;
  w.x.c = (int)floorf(ua[0]);
  w.y.c = (int)floorf(ua[1]);
  w.z.c = (int)floorf(ua[2]);
}
// clipped: the walk starts where the segment enters the map (rounding at the face is clamped back into the map)
__device__ __forceinline__ void seg_enter_clipped(SegWalk &w, const SegClip &cl, const float (&ub)[3]) {
  w.kind = SEG_CELL;
  w.t_cur = fmax(cl.t_in, 0.0);
  w.x.c = min(max((int)floor(w.x.A + w.t_cur * ((double)ub[0] - w.x.A)), 0), w.x.n - 1);
  w.y.c = min(max((int)floor(w.y.A + w.t_cur * ((double)ub[1] - w.y.A)), 0), w.y.n - 1);
  w.z.c = min(max((int)floor(w.z.A + w.t_cur * ((double)ub[2] - w.z.A)), 0), w.z.n - 1);
}
__device__ __forceinline__ void seg_axis_plane(SegAxis &s) {
  s.tn = s.step == 0 ? INFINITY : ((double)(s.c + (s.step > 0)) - s.A) * s.inv;
}
// the next plane of every axis from the first cell: ends the set-up
__device__ __forceinline__ void seg_planes(SegWalk &w) {
  seg_axis_plane(w.x);
  seg_axis_plane(w.y);
  seg_axis_plane(w.z);
}

// one of three by the axis; by value, so that nothing ever selects between two addresses
template <typename T>
__device__ __forceinline__ T seg_pick(int ax, T x, T y, T z) {
  return ax == 0 ? x : ax == 1 ? y : z;
}
__device__ __forceinline__ void seg_cross(SegAxis &s, bool here, int cn, double tn) {
  if (here) {
    s.c = cn;
    s.tn = tn;
  }
}
// From the current cell to the next: `cell` is cell_of(x, y, z) of the current one (INVALID_INDEX where it is none of the
// map's).  Returns the t at which the current cell is left (1 where the segment ends in it).  The crossed axis' values are
// picked first and the next plane computed once: three computations, one per axis, with their results picked cost the
// walking kernels 12 to 15 registers.
template <typename CellOf>
__device__ __forceinline__ double seg_advance(SegWalk &w, uint32_t &cell, const CellOf &cell_of) {
  double t_out = 1.0;
  cell = INVALID_INDEX;
  if (w.kind == SEG_CELL) {
    cell = cell_of(w.x.c, w.y.c, w.z.c);
    int ax = 0;  // the plane crossed next: x before y before z at equal t
    double tm = w.x.tn;
    if (w.y.tn < tm) { ax = 1; tm = w.y.tn; }
    if (w.z.tn < tm) { ax = 2; tm = w.z.tn; }
    if (tm > 1.0) {
      w.kind = SEG_END;
    } else {
      const int step = seg_pick(ax, w.x.step, w.y.step, w.z.step);
      const int cn = seg_pick(ax, w.x.c, w.y.c, w.z.c) + step;
      const double tn = ((double)(cn + (step > 0)) - seg_pick(ax, w.x.A, w.y.A, w.z.A)) * seg_pick(ax, w.x.inv, w.y.inv, w.z.inv);
      const bool out = cn < 0 || cn >= seg_pick(ax, w.x.n, w.y.n, w.z.n);
      seg_cross(w.x, ax == 0, cn, tn);
      seg_cross(w.y, ax == 1, cn, tn);
      seg_cross(w.z, ax == 2, cn, tn);
      w.t_cur = tm;
      t_out = tm;
      if (out) w.kind = SEG_OUT;
    }
  } else {
    w.kind = SEG_END;  // (after the cell outside the map there is nothing: the map is convex)
  }
  return t_out;
}

}  // namespace sdm
