// sdm_world.h — what the units of the world archive share (world.hip: the update, the getters and the queries;
// world_io.hip: import and retain; world_reach.hip: the travel-cost field over the bricks; world_frontiers.hip:
// the frontiers of the bricks; world_esdf.hip: the truncated distance field of the bricks; world_ground.hip: the height map
// and costmap over the bricks; world_ground_reach.hip: the 2-D travel-cost field over that costmap): the hash table's key, hash,
// lookup and insertion, which cells write, the header-word layout, the indices of the counters, an update's geometry and
// its closing kernel, and the three host helpers of world.hip that the other units call.  Everything but those three
// helpers has internal linkage: each unit compiles its own copy.
#pragma once
#include "sdm_layer.h"
#include "sdm_map.h"

namespace sdm {

// world.hip: the first update or import after creation or sdm_world_clear fixes the capacity (max_bricks 0: the default);
// later another non-zero capacity is refused while the archive holds bricks (waits) and exchanges the buffers while not
sdm_status world_capacity(sdm_map *m, const char *what, int64_t max_bricks);
// world.hip: waits; the archive's counters (M_WORDS words)
sdm_status world_counters(sdm_map *m, uint32_t *meta);
// world.hip: the pool slots in brick order, n_bricks of them (device memory, good until the archive next changes); sorted
// at the first call after a change, like sdm_get_world_bricks, which shares the order
sdm_status world_order(sdm_map *m, const uint32_t **order);

namespace {

constexpr int WTPB = 256, WWAVES = WTPB / 64;
constexpr uint32_t NONE = 0xffffffffu;
constexpr u64 EMPTY_KEY = ~0ull;
constexpr uint32_t HDR_WORDS = 5;  // sdm_world_brick as words: bx | by << 16, bz | n_occupied << 16, n_free | pad << 16, first_stamp, last_stamp
constexpr uint32_t ALL_FLAGS = SDM_WORLD_STATIC_ONLY | SDM_WORLD_OBSERVED_ONLY;
constexpr int64_t MAX_BRICKS_LIMIT = (int64_t)1 << 21;  // 512 words each: the pool's word index stays in 32 bits
enum { M_N_BRICKS = 0, M_CREATED, M_DROPPED, M_OOR, M_DROPPED_TOTAL /* u64: two words */, M_WORDS = 8 };

constexpr LayerName WORLD = {"the world archive", "archive", "sdm_world_update", false};

struct WGeo {       // an update's geometry, by value
  int g0[3];        // world cell of map-index cell (0, 0, 0)
  int b0[3], nb[3]; // the candidates: bricks b0 .. b0 + nb - 1 per axis
  uint32_t nc;      // nb[0] * nb[1] * nb[2]
  uint32_t nc_max;  // what the candidate arrays and the scan are sized for
  uint32_t flags, gts, max_bricks, hmask;
  int max_movable;
};

__device__ __forceinline__ bool brick_in_range(int bx, int by, int bz) {
  return bx >= -32768 && bx <= 32767 && by >= -32768 && by <= 32767 && bz >= -32768 && bz <= 32767;
}
__device__ __forceinline__ u64 brick_key(int bx, int by, int bz) {
  return (u64)(uint32_t)(bx + 32768) | ((u64)(uint32_t)(by + 32768) << 16) | ((u64)(uint32_t)(bz + 32768) << 32);
}
__device__ __forceinline__ uint32_t key_hash(u64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}
// the pool slot of a key, NONE if the archive has no such brick (the table is never more than half full)
__device__ __forceinline__ uint32_t world_find(const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask, u64 key) {
  uint32_t h = key_hash(key) & hmask;
  for (uint32_t i = 0; i <= hmask; ++i) {
    const u64 k = keys[h];
    if (k == key) return vals[h];
    if (k == EMPTY_KEY) return NONE;
    h = (h + 1u) & hmask;
  }
  return NONE;
}
__device__ __forceinline__ void world_insert(u64 *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t hmask, u64 key, uint32_t slot) {
  uint32_t h = key_hash(key) & hmask;
  for (uint32_t i = 0; i <= hmask; ++i) {
    if (atomicCAS(keys + h, EMPTY_KEY, key) == EMPTY_KEY) {
      vals[h] = slot;  // (read by later launches only)
      return;
    }
    h = (h + 1u) & hmask;
  }
}

__device__ __forceinline__ bool cell_writes(uint32_t w1, uint32_t flags, int max_movable) {
  const int occ = occ_of(w1);
  const uint32_t track = w1 & 0xffffu;
  const bool movable = track >= 1u && (int)track <= max_movable;
  return occ >= 0 && !((flags & SDM_WORLD_STATIC_ONLY) && occ >= 1 && movable) && !((flags & SDM_WORLD_OBSERVED_ONLY) && occ == 2);
}

__global__ __launch_bounds__(64) void k_world_finish(WGeo g, const uint32_t *__restrict__ rank, uint32_t *__restrict__ meta) {
  if (threadIdx.x != 0u) return;
  const uint32_t n = meta[M_N_BRICKS], wanted = rank[g.nc_max], room = g.max_bricks - n;
  const uint32_t created = wanted < room ? wanted : room;
  meta[M_N_BRICKS] = n + created;
  meta[M_CREATED] = created;
  u64 *total = reinterpret_cast<u64 *>(meta + M_DROPPED_TOTAL);
  *total += meta[M_DROPPED];
}

}  // namespace

}  // namespace sdm
