// sdm_layer.h — device helpers of the derived map layers (queries.hip, esdf.hip, instances.hip, frontiers.hip, views.hip,
// reach.hip, forecast.hip, ground.hip, mesh.hip, world.hip, world_io.hip, world_snapshot.hip, world_reach.hip, world_frontiers.hip, world_esdf.hip, world_ground.hip, world_ground_reach.hip, world_rays.hip, world_mesh.hip, world_match.hip, world_objects.hip, world_changes.hip): how they read a result word, go from a global position to a map-index
// coordinate and to a cell, between a cell word and its (x, y, z), and from a map-index cell to its storage index; how a
// wave loads the results of chunks of 64 cells in map-index order; a neighbour's bit in a 64-cell mask word; the rank of a
// lane's bit; reductions over the 64 lanes of a wave.  Only those twenty-two units include it (the three that walk segments
// through the block through sdm_walk.h): the frame pipeline's units see sdm_internal.h alone.
#pragma once
#include "sdm_internal.h"

namespace sdm {

typedef unsigned long long u64;

constexpr uint32_t RES_UNKNOWN_W1 = 0xff000000u;  // second word of an "unobserved" result: track 0, label 0, occ -1
constexpr uint32_t RES_UNKNOWN_W0 = 0xbf800000u;  // wsum -1.f

// occ of the second word of a result: -1 unobserved, 0 free, >= 1 an obstacle
__device__ __forceinline__ int8_t occ_of(uint32_t w1) { return (int8_t)(w1 >> 24); }

// map-index coordinate of one axis: the float32 expression of global_pos_to_voxel, without its cast
__device__ __forceinline__ float map_u(const Dims &d, const Frame &f, int a, float p) { return ((p - f.center[a]) - d.pmin[a]) * d.recip; }

// storage index of in-map cell (ix, iy, iz): the ring correction of global_pos_to_voxel
__device__ __forceinline__ uint32_t cell_voxel(const Dims &d, const Frame &f, int ix, int iy, int iz) {
  return ring_to_voxel(d, axis_correct(ix + f.eq[0], d.NX), axis_correct(iy + f.eq[1], d.NY), axis_correct(iz + f.eq[2], d.NZ));
}

// the cell word of in-map cell (x, y, z), and back
__device__ __forceinline__ uint32_t cell_word(const Dims &d, int x, int y, int z) {
  return (uint32_t)x | ((uint32_t)y << d.x_n) | ((uint32_t)z << (d.x_n + d.y_n));
}
template <typename T>
__device__ __forceinline__ void cell_xyz(const Dims &d, uint32_t c, T &x, T &y, T &z) {
  x = (T)(c & (d.NX - 1)), y = (T)((c >> d.x_n) & (d.NY - 1)), z = (T)(c >> (d.x_n + d.y_n));
}
// ... for the kernels that carry the axes' bit counts and no Dims
template <typename T>
__device__ __forceinline__ void cell_xyz(int x_n, int y_n, uint32_t c, T &x, T &y, T &z) {
  x = (T)(c & ((1u << x_n) - 1u)), y = (T)((c >> x_n) & ((1u << y_n) - 1u)), z = (T)(c >> (x_n + y_n));
}
// storage index of the cell of word c
__device__ __forceinline__ uint32_t word_voxel(const Dims &d, const Frame &f, uint32_t c) {
  uint32_t x, y, z;
  cell_xyz(d, c, x, y, z);
  return cell_voxel(d, f, (int)x, (int)y, (int)z);
}

// The cell of a global position, the one rule of every query by point: it lies in the map where every axis' map_u is in
// [0, N) (NaN and +-inf fail it).  u: the coordinates, cell: their floors - from the first axis that fails on 0.5 and 0 (no
// cast of a value outside the map).
__device__ __forceinline__ bool point_coords(const Dims &d, const Frame &f, const float (&p)[3], int (&cell)[3], float (&u)[3]) {
  const int N[3] = {(int)d.NX, (int)d.NY, (int)d.NZ};
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float v = map_u(d, f, a, p[a]);
    ok = ok && v >= 0.f && v < (float)N[a];
    u[a] = ok ? v : 0.5f;
    cell[a] = (int)floorf(u[a]);
  }
  return ok;
}
// ... as a cell word; INVALID_INDEX outside the map
__device__ __forceinline__ uint32_t point_cell(const Dims &d, const Frame &f, const float (&p)[3]) {
  int cell[3];
  float u[3];
  return point_coords(d, f, p, cell, u) ? cell_word(d, cell[0], cell[1], cell[2]) : INVALID_INDEX;
}

// The classify prologue: a wave takes U chunks of 64 cells from chunk0 on, a lane per cell in map-index order, and issues
// every load of the results' second word first (V is a multiple of 64: a chunk inside the map is whole; one beyond it -
// chunk >= nw, wave-uniform - reads as unobserved).
template <int U>
__device__ __forceinline__ void load_w1(const Dims &d, const Frame &f, const uint2 *__restrict__ res, uint32_t chunk0, uint32_t nw, uint32_t lane,
                                        uint32_t (&w)[U]) {
  const uint32_t xy_n = (uint32_t)(d.x_n + d.y_n), x_mask = d.NX - 1, y_mask = d.NY - 1;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t chunk = chunk0 + (uint32_t)u;
    w[u] = RES_UNKNOWN_W1;
    if (chunk < nw) {
      const uint32_t c = (chunk << 6) + lane;
      const uint32_t x = c & x_mask, y = (c >> d.x_n) & y_mask, z = c >> xy_n;
      w[u] = res[cell_voxel(d, f, (int)x, (int)y, (int)z)].y;
    }
  }
}

// ---- 64-cell mask words: word wi holds cells 64 wi .. 64 wi + 63 in map-index order -----------------------------------
// the low `width` bits of every `period` bits (powers of two, width <= period <= 64)
__device__ __forceinline__ u64 rep_mask(uint32_t period, uint32_t width) {
  u64 m = width >= 64u ? ~0ull : (1ull << width) - 1ull;
  for (uint32_t p = period; p < 64u; p <<= 1) m |= m << p;
  return m;
}

// the bits b of the word that begins at cell c0 (a multiple of 64) whose coordinate ((c0 + b) >> s) & (2^nb - 1) is t
__device__ __forceinline__ u64 coord_is(uint32_t c0, int s, int nb, uint32_t t) {
  const uint32_t N = 1u << nb;
  if (s >= 6) return ((c0 >> s) & (N - 1u)) == t ? ~0ull : 0ull;          // the whole word has one coordinate
  if (s + nb <= 6) return rep_mask(1u << (s + nb), 1u << s) << (t << s);  // the word holds every coordinate, 64 >> (s + nb) times
  const uint32_t k = t - ((c0 >> s) & (N - 1u));                          // the word holds 64 >> s coordinates from its first
  if (k >= (64u >> s)) return 0ull;
  return ((1ull << (1u << s)) - 1ull) << (k << s);
}

// bit b: the bit of cell c0 + b - 2^s (down) / c0 + b + 2^s (up) in mask; cells beyond the ends of the mask read 0
__device__ __forceinline__ u64 bits_down(const u64 *__restrict__ mask, uint32_t wi, int s) {
  if (s >= 6) {
    const uint32_t k = 1u << (s - 6);
    return wi >= k ? mask[wi - k] : 0ull;
  }
  const uint32_t D = 1u << s;
  return (mask[wi] << D) | (wi > 0u ? mask[wi - 1u] >> (64u - D) : 0ull);
}
__device__ __forceinline__ u64 bits_up(const u64 *__restrict__ mask, uint32_t wi, uint32_t nw, int s) {
  if (s >= 6) {
    const uint32_t k = 1u << (s - 6);
    return wi + k < nw ? mask[wi + k] : 0ull;
  }
  const uint32_t D = 1u << s;
  return (mask[wi] >> D) | (wi + 1u < nw ? mask[wi + 1u] << (64u - D) : 0ull);
}

// how many bits of mask lie below bit b: the rank of b's cell among the set ones of its word
__device__ __forceinline__ uint32_t lane_rank(u64 mask, uint32_t b) { return (uint32_t)__popcll(mask & ((1ull << b) - 1ull)); }

// ---- over the 64 lanes of a wave --------------------------------------------------------------------------------------
// sum / smallest / largest of v, in every lane
template <typename Op>
__device__ __forceinline__ uint32_t wave_all(uint32_t v, Op op) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = op(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return min(a, b); }); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s, 64);
    v += ((u64)hi << 32) | lo;
  }
  return v;
}

}  // namespace sdm
