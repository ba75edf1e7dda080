// ground.hip — the ground layer: a height map, a costmap and footprint checks of the map block (gfx950; include/sdm.h,
// "ground layer").
//
// A column is the line of cells along the up axis over one cell (i, j) of the other two axes u < v; the grid is N_u x N_v,
// column word i + j * N_u.  Heights count from the bottom: h = idx for up_sign +1, N - 1 - idx for -1.  The build is three
// launches on the map's stream:
//   k_ground_x     up axis x: one wave per column (a contiguous x line, loaded whole before anything else).  The solid /
//                  not-passable / support-candidate / unknown masks of a 64-cell chunk are ballots, so the level, the top
//                  and the headroom are bit operations on scalars; "the first cell above that is not passable" is carried
//                  across the chunks as k_esdf_x carries its nearest obstacle.
//   k_ground_walk  up axis y or z: one lane per column, the lanes of a wave on adjacent x, so every height step is one
//                  coalesced row; one walk from the top downward that carries the passable cells directly above, the
//                  loads of GW_U rows issued together.
//   k_ground_rows  one wave per row of the grid: the step bit (4-neighbours' levels), the lethal bit, the class byte, the
//                  row's counts (ballot + popcount; the getter adds the rows up on the host) and the row pass of the 2-D
//                  distance transform: the distance along the row to its nearest lethal column, 16 bits (the lethal mask
//                  of the row sits in scalar registers).
//   k_ground_cols  one lane per column and row p: d2 = the smallest g(q)^2 + (p - q)^2 over the rows q, every q tried.
//                  The lanes of a wave sit on adjacent columns, so a step is one coalesced 128-byte row that the block's
//                  other waves find in the L1.  A lower envelope per grid column (Felzenszwalb-Huttenlocher, as
//                  k_esdf_env) was built first and measured: N_u / 64 workgroups of one wave each, 4 on a 256 x 256 grid,
//                  each a serial chain of 2 N_v steps through LDS - 153 us of a 260 us build.  N_v^2 steps
//                  per column over every SIMD take a tenth of that (13 us).
// Everything is integer: g < 2^9, so g^2 + (p - q)^2 < 2^19.
// The queries read the layer's own arrays only, never State: the layer answers for the frame it was built from.
#include "sdm_layer.h"
#include "sdm_map.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_ground_cell) == 8 && sizeof(sdm_ground_result) == 32, "sdm.h layout");
static_assert(sizeof(sdm_footprint) == 24 && sizeof(sdm_footprint_result) == 32, "sdm.h layout");
static_assert(sizeof(sdm_ground_options) == 60 && sizeof(sdm_ground_info) == 104, "sdm.h layout");

namespace sdm {

namespace {

constexpr int GX_TPB = 256;     // k_ground_x, k_ground_rows: four lines per workgroup
constexpr int G_CHUNKS = 8;     // an axis has at most 512 = 8 x 64 cells
constexpr int GW_TPB = 256;     // k_ground_walk
constexpr int GW_U = 32;        // ... rows loaded together (16 measured 84 us at 256^3: DESIGN.md 5i)
constexpr int GC_TPB = 256;     // k_ground_cols
constexpr int GC_U = 4;         // ... rows loaded together (an axis has at least 4 cells, and a power of two)
constexpr uint32_t NO_ROW = 0xffffu;  // "no lethal column on this row", as a row distance
constexpr int G_NONE = 1 << 20; // "no lethal column on this row", as a position
constexpr int GQ_TPB = 256;
constexpr uint32_t NO_LEVEL = 0xffffu;
constexpr uint32_t ALL_FLAGS = SDM_GROUND_UNKNOWN_PASSABLE | SDM_GROUND_IGNORE_MOVABLE | SDM_GROUND_NONE_IS_LETHAL;
constexpr LayerName GROUND = {"the ground layer", "ground layer", "sdm_ground_update", false};
// the info counters of one row of the grid on the device: [row][M_WORDS]
enum { M_GROUND = 0, M_OBSTACLE, M_NONE, M_STEP, M_LETHAL, M_LEVEL_MIN, M_LEVEL_MAX, M_PAD, M_WORDS };

// What the kernels know of a build (by value): the orientation, the grid and the options.
struct Grid {
  int a, sign;          // up axis, +1 / -1
  int au, av;           // the grid's axes, au < av
  uint32_t NA, NU, NV;  // cells along the up axis; the grid
  int u_n;              // log2 NU
  int h_lo, h_hi, clearance, max_step;
  uint32_t flags;
  uint32_t labels[8];
};

// the classes of a cell's second result word: bit 0 solid, bit 1 not passable, bit 2 support candidate, bit 3 unknown
__device__ __forceinline__ uint32_t cell_class(const Grid &g, uint32_t w1, int max_movable) {
  const int occ = occ_of(w1);
  const uint32_t track = w1 & 0xffffu, label = (w1 >> 16) & 0xffu;
  const bool movable = track >= 1u && (int)track <= max_movable;
  const bool solid = occ >= 1 && !((g.flags & SDM_GROUND_IGNORE_MOVABLE) && movable);
  const bool passable = occ == 0 || (occ >= 1 && !solid) || ((g.flags & SDM_GROUND_UNKNOWN_PASSABLE) && occ == -1);
  const bool cand = solid && !movable && ((g.labels[label >> 5] >> (label & 31u)) & 1u);
  return (solid ? 1u : 0u) | (passable ? 0u : 2u) | (cand ? 4u : 0u) | (occ == -1 ? 8u : 0u);
}

__device__ __forceinline__ uint2 pack_cell(uint32_t level, uint32_t top, uint32_t label, uint32_t headroom, uint32_t n_unknown) {
  const uint32_t cls = level != NO_LEVEL ? 1u : (top != NO_LEVEL ? 2u : 0u);  // (k_ground_rows adds the step and lethal bits)
  return make_uint2(level | (top << 16), label | (cls << 8) | (min(headroom, 255u) << 16) | (min(n_unknown, 255u) << 24));
}

// position of the highest set bit of the chunks' masks, -1 if none
__device__ __forceinline__ int highest_bit(const unsigned long long *m) {
  int at = -1;
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c)
    if (m[c]) at = c * 64 + 63 - __builtin_clzll(m[c]);
  return at;
}

// ---- columns along x -----------------------------------------------------------------------------------------------
// Column (y, z) is line y + z * NY, which is its column word (u = y, v = z).  Lane l of chunk c holds height c * 64 + l.
__global__ __launch_bounds__(GX_TPB) void k_ground_x(Dims d, Frame f, Grid g, const uint2 *__restrict__ res, uint2 *__restrict__ cells) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t line = blockIdx.x * (GX_TPB / 64) + (threadIdx.x >> 6);
  if (line >= d.NY * d.NZ) return;  // (whole waves: no barrier below)
  const uint32_t y = line & (d.NY - 1), z = line >> d.y_n;
  const uint32_t ry = axis_correct((int)y + f.eq[1], d.NY), rz = axis_correct((int)z + f.eq[2], d.NZ);
  const int N = (int)d.NX;
  const uint32_t nc = (d.NX + 63u) >> 6;
  uint32_t w[G_CHUNKS];
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c) {  // every load of the line first
    const int h = c * 64 + (int)lane;
    w[c] = 0u;
    if ((uint32_t)c < nc && h < N) {
      const int x = g.sign > 0 ? h : N - 1 - h;
      w[c] = res[ring_to_voxel(d, axis_correct(x + f.eq[0], d.NX), ry, rz)].y;
    }
  }
  // the masks, in height order; what lies above the map is passable and nothing else
  unsigned long long solid[G_CHUNKS], blocked[G_CHUNKS];
  bool cand[G_CHUNKS];
  uint32_t n_unknown = 0;
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c) {
    solid[c] = blocked[c] = 0ull;
    cand[c] = false;
    if ((uint32_t)c >= nc) continue;  // (uniform: a line of 256 cells pays for four chunks)
    const int h = c * 64 + (int)lane;
    const bool in = h < N, band = in && h >= g.h_lo && h <= g.h_hi;
    const uint32_t k = in ? cell_class(g, w[c], d.max_movable) : 0u;
    solid[c] = __ballot(band && (k & 1u));
    blocked[c] = __ballot((k & 2u) != 0u);
    cand[c] = band && (k & 4u);
    n_unknown += (uint32_t)__builtin_popcountll(__ballot(band && (k & 8u)));
  }
  // first blocked cell above each height (N: none up to the map's top, and above it everything is passable)
  int after = N;
  unsigned long long support[G_CHUNKS];
  const unsigned long long above = ~1ull << lane;  // bits > lane
#pragma unroll
  for (int c = G_CHUNKS - 1; c >= 0; --c) {
    support[c] = 0ull;
    if ((uint32_t)c >= nc) continue;
    const int h = c * 64 + (int)lane;
    const unsigned long long bm = blocked[c] & above;
    const int stop = bm ? c * 64 + __builtin_ctzll(bm) : after;
    support[c] = __ballot(cand[c] && (stop == N || stop - h - 1 >= g.clearance));
    if (blocked[c]) after = c * 64 + __builtin_ctzll(blocked[c]);
  }
  const int level = highest_bit(support), top = highest_bit(solid);
  uint32_t label = 0u, headroom = 0u;
  if (level >= 0) {  // (uniform)
    const int lc = level >> 6, ll = level & 63;
    uint32_t wl = 0u;
    int stop = N;
#pragma unroll
    for (int c = G_CHUNKS - 1; c >= 0; --c) {
      if (c == lc) wl = w[c];
      const unsigned long long bm = c == lc ? blocked[c] & (~1ull << ll) : (c > lc ? blocked[c] : 0ull);
      if (bm) stop = c * 64 + __builtin_ctzll(bm);
    }
    label = ((uint32_t)__shfl((int)wl, ll, 64) >> 16) & 0xffu;
    headroom = (uint32_t)(stop - level - 1);
  }
  if (lane == 0) cells[line] = pack_cell(level >= 0 ? (uint32_t)level : NO_LEVEL, top >= 0 ? (uint32_t)top : NO_LEVEL, label, headroom, n_unknown);
}

// ---- columns along y or z ------------------------------------------------------------------------------------------
// AX = 1: column (x, z) runs along y, word x + z * NX.  AX = 2: column (x, y) runs along z, word x + y * NX.
template <int AX>
__global__ __launch_bounds__(GW_TPB) void k_ground_walk(Dims d, Frame f, Grid g, const uint2 *__restrict__ res, uint2 *__restrict__ cells) {
  const uint32_t col = blockIdx.x * GW_TPB + threadIdx.x;
  if (col >= g.NU * g.NV) return;
  const uint32_t x = col & (d.NX - 1), o = col >> d.x_n;  // o: z for AX = 1, y for AX = 2
  const uint32_t rx = axis_correct((int)x + f.eq[0], d.NX);
  const uint32_t ro = AX == 1 ? axis_correct((int)o + f.eq[2], d.NZ) : axis_correct((int)o + f.eq[1], d.NY);
  const int N = (int)g.NA;
  // a cell more than 255 above the band's top decides nothing: the clearance is at most 255 and the headroom saturates there
  const int h_start = min(N - 1, g.h_hi + 255);
  bool open = h_start == N - 1;  // every cell above the current one, up to the map's top, is passable
  int run = 0;                   // passable cells directly above the current one (counted from h_start down)
  uint32_t level = NO_LEVEL, top = NO_LEVEL, label = 0u, headroom = 0u, n_unknown = 0u;
  for (int h0 = h_start; h0 >= g.h_lo; h0 -= GW_U) {
    uint32_t w[GW_U];
#pragma unroll
    for (int j = 0; j < GW_U; ++j) {
      const int h = h0 - j;
      w[j] = 0u;
      if (h >= g.h_lo) {
        const uint32_t r = axis_correct((g.sign > 0 ? h : N - 1 - h) + f.eq[AX], g.NA);
        w[j] = res[AX == 1 ? ring_to_voxel(d, rx, r, ro) : ring_to_voxel(d, rx, ro, r)].y;
      }
    }
#pragma unroll
    for (int j = 0; j < GW_U; ++j) {
      const int h = h0 - j;
      if (h < g.h_lo) continue;  // (below the band: only the last group has such rows)
      const uint32_t k = cell_class(g, w[j], d.max_movable);
      if (h <= g.h_hi) {
        if ((k & 1u) && top == NO_LEVEL) top = (uint32_t)h;
        if ((k & 4u) && level == NO_LEVEL && (open || run >= g.clearance)) {
          level = (uint32_t)h;
          label = (w[j] >> 16) & 0xffu;
          headroom = (uint32_t)run;
        }
        n_unknown += (k >> 3) & 1u;
      }
      if (k & 2u) {
        run = 0;
        open = false;
      } else {
        ++run;
      }
    }
  }
  cells[col] = pack_cell(level, top, label, headroom, n_unknown);
}

// ---- step, lethal, the counts; the distance transform's row pass -----------------------------------------------------
// One wave per row j.  A neighbour's level is read from the cell's first half-word, which no launch but the column pass
// writes; this pass stores the class byte alone.  No atomics: a row's counts go to the row's own words.
__global__ __launch_bounds__(GX_TPB) void k_ground_rows(Grid g, sdm_ground_cell *__restrict__ cells, uint16_t *__restrict__ rowd,
                                                        uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * (GX_TPB / 64) + (threadIdx.x >> 6);
  if (j >= g.NV) return;  // (whole waves: no barrier below)
  const uint32_t nc = (g.NU + 63u) >> 6;
  const size_t row = (size_t)j << g.u_n;
  const uint16_t *level_of = reinterpret_cast<const uint16_t *>(cells);  // [col * 4]
  uint32_t lv[G_CHUNKS], nb[G_CHUNKS][4], cls[G_CHUNKS];
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c) {  // every load of the row first
    const uint32_t i = (uint32_t)c * 64u + lane;
    lv[c] = NO_LEVEL, cls[c] = 0u;
    nb[c][0] = nb[c][1] = nb[c][2] = nb[c][3] = NO_LEVEL;
    if ((uint32_t)c < nc && i < g.NU) {
      lv[c] = level_of[(row + i) * 4];
      cls[c] = cells[row + i].cls;
      if (i > 0) nb[c][0] = level_of[(row + i - 1) * 4];
      if (i + 1 < g.NU) nb[c][1] = level_of[(row + i + 1) * 4];
      if (j > 0) nb[c][2] = level_of[(row - g.NU + i) * 4];
      if (j + 1 < g.NV) nb[c][3] = level_of[(row + g.NU + i) * 4];
    }
  }
  unsigned long long m[G_CHUNKS];
  uint32_t n[5] = {0u, 0u, 0u, 0u, 0u}, lo = NO_LEVEL, hi = 0u;
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c) {
    m[c] = 0ull;
    if ((uint32_t)c >= nc) continue;  // (uniform)
    const uint32_t i = (uint32_t)c * 64u + lane;
    const bool in = i < g.NU;
    const uint32_t k = cls[c] & 3u;
    bool step = false;
    if (in && k == 1u) {
#pragma unroll
      for (int q = 0; q < 4; ++q) step = step || (nb[c][q] != NO_LEVEL && lv[c] > nb[c][q] + (uint32_t)g.max_step);
      lo = min(lo, lv[c]);
      hi = max(hi, lv[c]);
    }
    const bool lethal = in && (k == 2u || step || (k == 0u && (g.flags & SDM_GROUND_NONE_IS_LETHAL)));
    if (in) cells[row + i].cls = (uint8_t)(k | (step ? 4u : 0u) | (lethal ? 8u : 0u));
    m[c] = __ballot(lethal);
    n[M_GROUND] += (uint32_t)__builtin_popcountll(__ballot(in && k == 1u));
    n[M_OBSTACLE] += (uint32_t)__builtin_popcountll(__ballot(in && k == 2u));
    n[M_NONE] += (uint32_t)__builtin_popcountll(__ballot(in && k == 0u));
    n[M_STEP] += (uint32_t)__builtin_popcountll(__ballot(step));
    n[M_LETHAL] += (uint32_t)__builtin_popcountll(m[c]);
  }
  lo = wave_min(lo), hi = wave_max(hi);
  if (lane < M_WORDS) {  // one 32-byte store of the row's words
    uint32_t v = lane == M_LEVEL_MIN ? lo : (lane == M_LEVEL_MAX ? hi : 0u);
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if ((int)lane == q) v = n[q];
    meta[j * M_WORDS + lane] = v;
  }
  // nearest lethal column at or left of each column, then at or right of it (k_esdf_x's pass)
  int left[G_CHUNKS], right[G_CHUNKS];
  int before = -G_NONE, after = G_NONE;
  const unsigned long long upto = (2ull << lane) - 1ull, from = ~0ull << lane;  // bits <= lane, bits >= lane
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c) {
    const unsigned long long lm = m[c] & upto;
    left[c] = lm ? c * 64 + 63 - __builtin_clzll(lm) : before;
    if (m[c]) before = c * 64 + 63 - __builtin_clzll(m[c]);
  }
#pragma unroll
  for (int c = G_CHUNKS - 1; c >= 0; --c) {
    const unsigned long long rm = m[c] & from;
    right[c] = rm ? c * 64 + __builtin_ctzll(rm) : after;
    if (m[c]) after = c * 64 + __builtin_ctzll(m[c]);
  }
#pragma unroll
  for (int c = 0; c < G_CHUNKS; ++c) {
    const int i = c * 64 + (int)lane;
    if ((uint32_t)c < nc && i < (int)g.NU) {
      const int near = min(i - left[c], right[c] - i);  // (>= G_NONE - 511 where there is none)
      rowd[row + i] = near < G_NONE / 2 ? (uint16_t)near : (uint16_t)NO_ROW;
    }
  }
}

// ---- the distance transform's column pass ------------------------------------------------------------------------------
// Thread t answers column word t = i + p * N_u.
__global__ __launch_bounds__(GC_TPB) void k_ground_cols(Grid g, const uint16_t *__restrict__ rowd, uint32_t *__restrict__ d2) {
  const uint32_t t = blockIdx.x * GC_TPB + threadIdx.x;
  if (t >= g.NU * g.NV) return;
  const uint32_t i = t & (g.NU - 1u);
  const int p = (int)(t >> g.u_n);
  uint32_t best = INVALID_INDEX;
  for (uint32_t q0 = 0; q0 < g.NV; q0 += GC_U) {  // (N_v is a multiple of GC_U)
    uint32_t r[GC_U];
#pragma unroll
    for (int k = 0; k < GC_U; ++k) r[k] = rowd[i + ((size_t)(q0 + k) << g.u_n)];
#pragma unroll
    for (int k = 0; k < GC_U; ++k) {
      const int dq = p - (int)(q0 + k);
      const uint32_t v = r[k] * r[k] + (uint32_t)(dq * dq);
      if (r[k] != NO_ROW) best = min(best, v);
    }
  }
  d2[t] = best;
}

// ---- the point query: one lane per point ---------------------------------------------------------------------------
__device__ __forceinline__ sdm_ground_cell unpack_cell(uint2 c) {
  sdm_ground_cell r;
  __builtin_memcpy(&r, &c, 8);
  return r;
}

__global__ __launch_bounds__(GQ_TPB) void k_query_ground(Dims d, Frame f, Grid g, const float *__restrict__ xyz, uint32_t n,
                                                         const uint2 *__restrict__ cells, const uint32_t *__restrict__ d2,
                                                         sdm_ground_result *__restrict__ out) {
  const uint32_t p = blockIdx.x * GQ_TPB + threadIdx.x;
  if (p >= n) return;
  const float pos[3] = {xyz[3 * (size_t)p], xyz[3 * (size_t)p + 1], xyz[3 * (size_t)p + 2]};
  int cell[3];
  float u[3];
  const bool ok = point_coords(d, f, pos, cell, u);
  sdm_ground_result r;
  r.col = INVALID_INDEX;
  r.d2 = INVALID_INDEX;
  r.surface = 0.f;
  r.above = INT32_MIN;
  r.cell = unpack_cell(make_uint2(NO_LEVEL | (NO_LEVEL << 16), 0u));
  r.dist = -1.f;
  r.status = 3u;
  if (ok) {
    // (the axes are picked by selects, not by indexing with a runtime value: the arrays stay in registers)
    const int ia = g.a == 0 ? cell[0] : (g.a == 1 ? cell[1] : cell[2]);
    const int iu = g.au == 0 ? cell[0] : cell[1], iv = g.av == 1 ? cell[1] : cell[2];
    const uint32_t col = (uint32_t)iu + ((uint32_t)iv << g.u_n);
    r.col = col;
    r.cell = unpack_cell(cells[col]);
    r.d2 = d2[col];
    r.status = 0u;
    if (r.d2 != INVALID_INDEX) r.dist = sqrtf((float)r.d2) * d.voxel_size;
    if (r.cell.level != NO_LEVEL) {
      const int level = (int)r.cell.level;
      const int h = g.sign > 0 ? ia : (int)g.NA - 1 - ia;
      r.above = h - level;
      const int k = g.sign > 0 ? level + 1 : (int)g.NA - 1 - level;  // the index of the level cell's upper face
      const float ca = g.a == 0 ? f.center[0] : (g.a == 1 ? f.center[1] : f.center[2]);
      const float pa = g.a == 0 ? d.pmin[0] : (g.a == 1 ? d.pmin[1] : d.pmin[2]);
      r.surface = (ca + pa) + (float)k * d.voxel_size;
    }
  }
  out[p] = r;
}

// ---- the footprint query: one wave per footprint ---------------------------------------------------------------------
// The wave walks a rectangle of columns that holds every column the rule can cover, 64 columns a step.  With
// |dir|^2 >= 1/2 a covered centre lies within sqrt(2) * (half_len + half_wid) of the footprint's centre; the rectangle
// takes 1.5 times that sum, two columns more and a few float32 steps of the coordinates' magnitude.  Any other dir - the
// rule does not ask for a unit vector - gets the whole grid.
__global__ __launch_bounds__(GQ_TPB) void k_query_footprints(Dims d, Frame f, Grid g, const sdm_footprint *__restrict__ fps, uint32_t n,
                                                             const uint2 *__restrict__ cells, const uint32_t *__restrict__ d2,
                                                             sdm_footprint_result *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * (GQ_TPB / 64) + (threadIdx.x >> 6);
  if (p >= n) return;  // (whole waves)
  const sdm_footprint fp = fps[p];
  const float size = d.voxel_size;
  const float ou = (g.au == 0 ? f.center[0] : f.center[1]) + (g.au == 0 ? d.pmin[0] : d.pmin[1]);
  const float ov = (g.av == 1 ? f.center[1] : f.center[2]) + (g.av == 1 ? d.pmin[1] : d.pmin[2]);
  const float reach = fp.half_len + fp.half_wid;
  const bool finite = isfinite(fp.center_u) && isfinite(fp.center_v) && isfinite(fp.dir_u) && isfinite(fp.dir_v) && isfinite(fp.half_len) &&
                      isfinite(fp.half_wid);
  int i0 = 0, i1 = -1, j0 = 0, j1 = -1;  // [i0, i1] x [j0, j1], empty
  if (finite && !(reach > 64.f * size)) {
    i1 = (int)g.NU - 1, j1 = (int)g.NV - 1;
    if (fp.dir_u * fp.dir_u + fp.dir_v * fp.dir_v >= 0.5f) {
      const float r = 1.5f * reach * d.recip + 2.f;
      const float eu = (fabsf(fp.center_u) + fabsf(ou) + (float)g.NU * size) * (d.recip * 0x1p-20f);
      const float ev = (fabsf(fp.center_v) + fabsf(ov) + (float)g.NV * size) * (d.recip * 0x1p-20f);
      const float cu = (fp.center_u - ou) * d.recip, cv = (fp.center_v - ov) * d.recip;
      // (clamped as floats: no cast of a value far outside the grid)
      i0 = (int)fminf(fmaxf(floorf(cu - r - eu), 0.f), (float)g.NU);
      i1 = (int)fminf(fmaxf(ceilf(cu + r + eu), -1.f), (float)(g.NU - 1));
      j0 = (int)fminf(fmaxf(floorf(cv - r - ev), 0.f), (float)g.NV);
      j1 = (int)fminf(fmaxf(ceilf(cv + r + ev), -1.f), (float)(g.NV - 1));
    }
  }
  uint32_t n_cols = 0, n_lethal = 0, n_none = 0, n_ground = 0;
  uint32_t lv_min = NO_LEVEL, lv_max = 0u, min_d2 = INVALID_INDEX, first = INVALID_INDEX;
  if (i1 >= i0 && j1 >= j0) {  // (uniform)
    const uint32_t wu = (uint32_t)(i1 - i0 + 1), total = wu * (uint32_t)(j1 - j0 + 1);
    for (uint32_t base = 0; base < total; base += 64u) {
      const uint32_t k = base + lane;
      bool covered = false;
      uint32_t col = 0u;
      if (k < total) {
        const uint32_t jj = k / wu;
        const int i = i0 + (int)(k - jj * wu), j = j0 + (int)jj;
        col = (uint32_t)i + ((uint32_t)j << g.u_n);
        const float pu = ou + ((float)i + 0.5f) * size, pv = ov + ((float)j + 0.5f) * size;
        const float du = pu - fp.center_u, dv = pv - fp.center_v;
        covered = fabsf(du * fp.dir_u + dv * fp.dir_v) <= fp.half_len && fabsf(dv * fp.dir_u - du * fp.dir_v) <= fp.half_wid;
      }
      uint32_t cls = 0u, level = NO_LEVEL;
      if (covered) {
        const uint2 c = cells[col];
        cls = (c.y >> 8) & 0xffu;
        level = c.x & 0xffffu;
        min_d2 = min(min_d2, d2[col]);
        if (cls & 8u) first = min(first, col);
        if ((cls & 3u) == 1u) {
          lv_min = min(lv_min, level);
          lv_max = max(lv_max, level);
        }
      }
      n_cols += (uint32_t)__builtin_popcountll(__ballot(covered));
      n_lethal += (uint32_t)__builtin_popcountll(__ballot(covered && (cls & 8u)));
      n_none += (uint32_t)__builtin_popcountll(__ballot(covered && (cls & 3u) == 0u));
      n_ground += (uint32_t)__builtin_popcountll(__ballot(covered && (cls & 3u) == 1u));
    }
  }
  lv_min = wave_min(lv_min), lv_max = wave_max(lv_max), min_d2 = wave_min(min_d2), first = wave_min(first);
  if (lane == 0) {
    sdm_footprint_result r;
    r.n_cols = n_cols, r.n_lethal = n_lethal, r.n_none = n_none, r.n_ground = n_ground;
    r.level_min = (uint16_t)lv_min;
    r.level_max = (uint16_t)(n_ground ? lv_max : NO_LEVEL);
    r.min_d2 = min_d2;
    r.first_lethal = first;
    r.pad = 0u;
    out[p] = r;
  }
}

Grid grid_of(const Dims &d, const sdm_ground_options &o) {
  Grid g{};
  const uint32_t N[3] = {d.NX, d.NY, d.NZ};
  const int bits[3] = {d.x_n, d.y_n, d.z_n};
  g.a = o.up_axis, g.sign = o.up_sign;
  g.au = g.a == 0 ? 1 : 0, g.av = g.a == 2 ? 1 : 2;
  g.NA = N[g.a], g.NU = N[g.au], g.NV = N[g.av];
  g.u_n = bits[g.au];
  g.h_lo = o.h_lo, g.h_hi = o.h_hi, g.clearance = (int)o.clearance, g.max_step = (int)o.max_step;
  g.flags = o.flags;
  for (int k = 0; k < 8; ++k) g.labels[k] = o.support_labels[k];
  return g;
}

hipError_t launch_ground_build(const Dims &d, const Frame &f, const Grid &g, const State &st, GroundLayer &L, hipStream_t s) {
  const uint2 *res = reinterpret_cast<const uint2 *>(st.res);
  uint2 *cells = reinterpret_cast<uint2 *>(L.cells);
  const uint32_t n_cols = g.NU * g.NV;
  if (g.a == 0)
    hipLaunchKernelGGL(k_ground_x, dim3((n_cols + GX_TPB / 64 - 1) / (GX_TPB / 64)), dim3(GX_TPB), 0, s, d, f, g, res, cells);
  else if (g.a == 1)
    hipLaunchKernelGGL(k_ground_walk<1>, dim3((n_cols + GW_TPB - 1) / GW_TPB), dim3(GW_TPB), 0, s, d, f, g, res, cells);
  else
    hipLaunchKernelGGL(k_ground_walk<2>, dim3((n_cols + GW_TPB - 1) / GW_TPB), dim3(GW_TPB), 0, s, d, f, g, res, cells);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ground_rows, dim3((g.NV + GX_TPB / 64 - 1) / (GX_TPB / 64)), dim3(GX_TPB), 0, s, g, L.cells, L.rowd, L.meta);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ground_cols, dim3((n_cols + GC_TPB - 1) / GC_TPB), dim3(GC_TPB), 0, s, g, (const uint16_t *)L.rowd, L.d2);
  return hipGetLastError();
}


}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
// The build reads the result array in stream order and takes the host Frame of the last issued frame by value, as the
// other layers do; the Frame and the options are kept with the layer, so that the getter and the queries answer for them.
extern "C" {

sdm_status sdm_ground_update(sdm_map *m, const sdm_ground_options *o) {
  const char *what = "sdm_ground_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->up_axis < 0 || o->up_axis > 2 || (o->up_sign != 1 && o->up_sign != -1)) return LAYER_REFUSE(what, "up_axis not in 0..2 or up_sign not +1 / -1");
  const int32_t NA = (int32_t)(o->up_axis == 0 ? m->d.NX : (o->up_axis == 1 ? m->d.NY : m->d.NZ));
  if (o->h_lo < 0 || o->h_lo > o->h_hi || o->h_hi >= NA) return LAYER_REFUSE(what, "the band needs 0 <= h_lo <= h_hi < N along the up axis");
  if (o->clearance > 255u || o->max_step > 65535u) return LAYER_REFUSE(what, "clearance > 255 or max_step > 65535");
  SDM_TRY(layer_check(m, what, nullptr, GROUND));
  HIP_TRY(hipSetDevice(m->device));
  GroundLayer &L = m->ground;
  const size_t cap = (size_t)std::max({m->d.NX * m->d.NY, m->d.NX * m->d.NZ, m->d.NY * m->d.NZ});  // whatever the orientation
  if (!L.cells) SDM_TRY(alloc_tracked(m, &L.cells, cap));
  if (!L.d2) SDM_TRY(alloc_tracked(m, &L.d2, cap));
  if (!L.rowd) SDM_TRY(alloc_tracked(m, &L.rowd, cap));
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, (size_t)M_WORDS * std::max({m->d.NX, m->d.NY, m->d.NZ})));  // a row's counters, for the longest axis
  const Frame f = m->f;
  HIP_TRY(launch_ground_build(m->d, f, grid_of(m->d, *o), m->st, L, m->stream));
  L.opt = *o;
  L.built(f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_ground(sdm_map *m, sdm_ground_cell *cells, uint32_t *d2, sdm_ground_info *info, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_get_ground", &m->ground, GROUND));
  HIP_TRY(hipSetDevice(m->device));
  const GroundLayer &L = m->ground;
  const Grid g = grid_of(m->d, L.opt);
  const size_t n_cols = (size_t)g.NU * g.NV;
  std::vector<uint32_t> rows(info ? (size_t)M_WORDS * g.NV : 0);
  if (cells) HIP_TRY(hipMemcpyAsync(cells, L.cells, n_cols * sizeof(sdm_ground_cell), hipMemcpyDeviceToHost, m->stream));
  if (d2) HIP_TRY(hipMemcpyAsync(d2, L.d2, n_cols * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (info) HIP_TRY(hipMemcpyAsync(rows.data(), L.meta, rows.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (info) {
    uint32_t meta[M_WORDS] = {0u, 0u, 0u, 0u, 0u, NO_LEVEL, 0u, 0u};  // the rows' counters added up
    for (uint32_t j = 0; j < g.NV; ++j) {
      const uint32_t *r = &rows[(size_t)j * M_WORDS];
      for (int q = 0; q < 5; ++q) meta[q] += r[q];
      meta[M_LEVEL_MIN] = std::min(meta[M_LEVEL_MIN], r[M_LEVEL_MIN]);
      meta[M_LEVEL_MAX] = std::max(meta[M_LEVEL_MAX], r[M_LEVEL_MAX]);
    }
    info->n_u = g.NU, info->n_v = g.NV;
    info->axis_u = (uint32_t)g.au, info->axis_v = (uint32_t)g.av;
    info->n_ground = meta[M_GROUND], info->n_obstacle = meta[M_OBSTACLE], info->n_none = meta[M_NONE];
    info->n_step = meta[M_STEP], info->n_lethal = meta[M_LETHAL];
    info->level_min = meta[M_GROUND] ? meta[M_LEVEL_MIN] : NO_LEVEL;
    info->level_max = meta[M_GROUND] ? meta[M_LEVEL_MAX] : NO_LEVEL;
    info->options = L.opt;
  }
  layer_origin(m, L, origin);
  return SDM_OK;
}

sdm_status sdm_query_ground(sdm_map *m, const float *xyz, int64_t n, sdm_ground_result *out, uint32_t flags) {
  SDM_TRY(query_check(m, xyz, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_ground"));
  SDM_TRY(layer_check(m, "sdm_query_ground", &m->ground, GROUND));
  const GroundLayer &L = m->ground;
  const Frame f = L.f;
  const Grid g = grid_of(m->d, L.opt);
  const uint2 *cells = reinterpret_cast<const uint2 *>(L.cells);
  const uint32_t *d2 = L.d2;
  return run_query(m, xyz, 12, out, sizeof(sdm_ground_result), nullptr, 0, n, flags,
                   [m, f, g, cells, d2](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_ground, dim3((c + GQ_TPB - 1) / GQ_TPB), dim3(GQ_TPB), 0, s, m->d, f, g,
                                        static_cast<const float *>(in), c, cells, d2, static_cast<sdm_ground_result *>(o));
                   });
}

sdm_status sdm_query_footprints(sdm_map *m, const sdm_footprint *fp, int64_t n, sdm_footprint_result *out, uint32_t flags) {
  SDM_TRY(query_check(m, fp, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_footprints"));
  SDM_TRY(layer_check(m, "sdm_query_footprints", &m->ground, GROUND));
  const GroundLayer &L = m->ground;
  const Frame f = L.f;
  const Grid g = grid_of(m->d, L.opt);
  const uint2 *cells = reinterpret_cast<const uint2 *>(L.cells);
  const uint32_t *d2 = L.d2;
  return run_query(m, fp, sizeof(sdm_footprint), out, sizeof(sdm_footprint_result), nullptr, 0, n, flags,
                   [m, f, g, cells, d2](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_footprints, dim3((c + GQ_TPB / 64 - 1) / (GQ_TPB / 64)), dim3(GQ_TPB), 0, s, m->d, f, g,
                                        static_cast<const sdm_footprint *>(in), c, cells, d2, static_cast<sdm_footprint_result *>(o));
                   });
}

}  // extern "C"
