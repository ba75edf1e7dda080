// sdm_layer.h — device helpers of the derived map layers (queries.hip, esdf.hip, instances.hip, frontiers.hip, views.hip,
// reach.hip, forecast.hip, ground.hip, mesh.hip): how they read a result word, go from a global position to a map-index coordinate and from a map-index cell
// to its storage index, and reduce a value over the 64 lanes of a wave.  Only those nine units include it: the frame
// pipeline's units see sdm_internal.h alone.
#pragma once
#include "sdm_internal.h"

namespace sdm {

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

// sum / smallest / largest of v over the 64 lanes of the wave, in every lane
template <typename Op>
__device__ __forceinline__ uint32_t wave_all(uint32_t v, Op op) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = op(v, (uint32_t)__shfl_xor((int)v, s, 64));
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return min(a, b); }); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_all(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }

}  // namespace sdm
