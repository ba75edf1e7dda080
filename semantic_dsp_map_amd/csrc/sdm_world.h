// sdm_world.h — what the units of the world archive share (world.hip: the update, the getters and the queries;
// world_io.hip: import and retain; world_snapshot.hip: the kernels and host helpers the builds over the archive share;
// world_reach.hip: the travel-cost field over the bricks; world_frontiers.hip: the frontiers of the bricks; world_esdf.hip:
// the truncated distance field of the bricks; world_ground.hip: the height map and costmap over the bricks;
// world_ground_reach.hip: the 2-D travel-cost field over that costmap; world_rays.hip: segments and views through the
// bricks; world_mesh.hip: the faces and welded vertices of the bricks' surface; world_match.hip: foreign bricks scored
// against the archive under a window of whole-cell offsets; world_objects.hip: the connected same-key components of the
// bricks' occupied cells): the hash table's key, hash, lookup and
// insertion, which cells write, the header-word layout, the indices of the counters, an update's geometry, how an entry of
// a query becomes a world cell, the packing of brick coordinates and tile keys, the host scaffold of a snapshot build and
// of the two route planners, and the host entry points of world.hip and world_snapshot.hip that the other units call.  No kernel lives here: everything in the unnamed namespace has internal
// linkage and each unit compiles its own copy, so a kernel here would land in every object.
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
// world.hip: the kernel that closes an update or an import - n_bricks, created_last, dropped_total from *wanted, the number
// of bricks that asked for room
hipError_t launch_world_finish(const uint32_t *wanted, uint32_t max_bricks, uint32_t *meta, hipStream_t s);
// world_io.hip: the import's source table over n source headers - every key once, the lowest source index with these
// coordinates beside it; the caller hands in smask + 1 slots (a power of two >= 2 n) of keys and indices, all ones
hipError_t launch_world_sources(const uint32_t *src_hdr, uint32_t n, uint32_t smask, unsigned long long *skeys, uint32_t *svals, hipStream_t s);

struct BrickBox {  // the bricks lo .. hi per axis; use 0: every brick
  int lo[3], hi[3];
  uint32_t use;
};
// world_snapshot.hip: rank = the exclusive scan of flag over items + 1 entries (scan: layer_scan_scratch's); the entry behind
// the last item, the number of flags set, goes through the page-locked word `landing` into *n.  Waits, once.
sdm_status snapshot_rank(sdm_map *m, const uint32_t *flag, uint32_t *rank, size_t items, uint32_t *scan, void *landing, uint32_t *n);
// world_snapshot.hip: flag[j] = the j-th archived brick of the brick order lies in the box, then snapshot_rank over them
sdm_status snapshot_flag_bricks(sdm_map *m, const uint32_t *order, uint32_t n_arch, const BrickBox &box, uint32_t *flag, uint32_t *rank,
                                uint32_t *scan, void *landing, uint32_t *n);
// world_snapshot.hip: a flagged brick writes its coordinates at its rank (< n), its pool slot into slot_of (may be null) and
// inserts key -> rank into the caller's table
hipError_t launch_snapshot_index(const sdm_map *m, const uint32_t *order, const uint32_t *flag, const uint32_t *rank, uint32_t n_arch, uint32_t n,
                                 uint32_t *coord, uint32_t *slot_of, unsigned long long *keys, uint32_t *vals, uint32_t hmask);
// world_snapshot.hip: the activity bits of n items become a list (and are cleared); *count grows by its length
hipError_t launch_snapshot_list(uint32_t *act, uint32_t *list, uint32_t *count, uint32_t n, hipStream_t s);

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

// ---- an entry of a query, the packing of coordinates ----------------------------------------------------------------------
// the world cell of a coordinate: floorf(p * recip); false (and 0) for a non-finite one or a brick out of range
__device__ __forceinline__ bool world_cell_of(float p, float recip, int &g) {
  const float v = floorf(p * recip);
  const bool ok = v >= -262144.f && v < 262144.f;  // (NaN fails; the cast sees values in range only)
  g = ok ? (int)v : 0;
  return ok;
}
// entry i as a world cell: the cell given, or the cell of a point by the archive's rule.  False where its brick is out of
// range or the point is not finite; g is then (0, 0, 0) for a point and the entry itself for a cell.
__device__ __forceinline__ bool entry_cell(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t i, float recip, int (&g)[3]) {
  if (cells) {
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = cells[3 * (size_t)i + a];
    return brick_in_range(g[0] >> 3, g[1] >> 3, g[2] >> 3);
  }
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = world_cell_of(xyz[3 * (size_t)i + a], recip, g[a]) && ok;
  if (!ok) g[0] = g[1] = g[2] = 0;
  return ok;
}
// a brick's coordinates from the first two words of its header, or from a coordinate pair (the same words, the counts cut off)
__device__ __forceinline__ void brick_of(uint32_t h0, uint32_t h1, int &bx, int &by, int &bz) {
  bx = (int16_t)(h0 & 0xffffu), by = (int16_t)(h0 >> 16), bz = (int16_t)(h1 & 0xffffu);
}
__device__ __forceinline__ void coord_of(const uint32_t *__restrict__ coord, uint32_t r, int &bx, int &by, int &bz) {
  brick_of(coord[2 * (size_t)r], coord[2 * (size_t)r + 1], bx, by, bz);
}
// the brick offset (-1, 0, 1) of coordinate c in -1 .. 8 of the brick's own cells 0 .. 7
__device__ __forceinline__ int brick_off(int c) { return c < 0 ? -1 : c > 7 ? 1 : 0; }
// a tile (bu, bv) of the world ground layer: its key, 32 bits, and back
__device__ __forceinline__ u64 tile_key(int bu, int bv) { return (u64)(uint32_t)(bu + 32768) | ((u64)(uint32_t)(bv + 32768) << 16); }
__device__ __forceinline__ bool tile_in_range(int bu, int bv) { return bu >= -32768 && bu <= 32767 && bv >= -32768 && bv <= 32767; }
__host__ __device__ __forceinline__ void tile_of(uint32_t key, int &bu, int &bv) { bu = (int)(key & 0xffffu) - 32768, bv = (int)(key >> 16) - 32768; }

// ---- the host scaffold --------------------------------------------------------------------------------------------------
// the slots of a table that is at most half full with `items` keys
inline uint32_t table_slots(size_t items) {
  uint32_t slots = 2;
  while (slots < 2 * items) slots <<= 1;
  return slots;
}
// the getters: coordinate pairs / tile keys as int16 triples / pairs
inline void unpack_coords(const std::vector<uint32_t> &pairs, int16_t *coords) {
  for (size_t i = 0; i < pairs.size() / 2; ++i) {
    coords[3 * i] = (int16_t)(pairs[2 * i] & 0xffffu);
    coords[3 * i + 1] = (int16_t)(pairs[2 * i] >> 16);
    coords[3 * i + 2] = (int16_t)(pairs[2 * i + 1] & 0xffffu);
  }
}
inline void unpack_tiles(const std::vector<uint32_t> &keys, int16_t *coords) {
  for (size_t i = 0; i < keys.size(); ++i) {
    int bu, bv;
    tile_of(keys[i], bu, bv);
    coords[2 * i] = (int16_t)bu, coords[2 * i + 1] = (int16_t)bv;
  }
}

// The prelude of a build over the bricks of a box (reach, frontiers, esdf): the archive's counters (waits), and if it holds
// bricks their order, the layers' scan scratch for a scan of scan_len entries, the caller's flag and rank arrays for n_arch + 1
// entries - buffers(n_arch, &flag, &rank), which may wait or allocate - the box flags and their ranks (snapshot_flag_bricks).
struct SnapshotBricks {
  uint32_t n_arch = 0, n = 0;  // archived bricks, bricks of the field
  const uint32_t *order = nullptr;
  uint32_t *flag = nullptr, *rank = nullptr, *scan = nullptr;
};
template <class Buffers>
sdm_status snapshot_bricks(sdm_map *m, const BrickBox &box, size_t scan_len, void *landing, Buffers buffers, SnapshotBricks *b) {
  uint32_t wmeta[M_WORDS];
  SDM_TRY(world_counters(m, wmeta));
  if (!(b->n_arch = wmeta[M_N_BRICKS])) return SDM_OK;
  SDM_TRY(world_order(m, &b->order));
  SDM_TRY(layer_scan_scratch(m, scan_len, &b->scan));
  SDM_TRY(buffers(b->n_arch, &b->flag, &b->rank));
  return snapshot_flag_bricks(m, b->order, b->n_arch, box, b->flag, b->rank, b->scan, landing, &b->n);
}

// The rounds of a route planner's relaxation: `batch` rounds - launch_round(grid, round) - between two looks at the
// counters (`words` of them, d_meta to h_meta); h_cnt: the two counts of listed items, round r's in h_cnt[r & 1].  An empty
// round ends it: nothing was lowered in the one before it, nothing ever will be.  grid_of(last): the grid for rounds that
// follow one of `last` items (0: the first).
template <class GridOf, class Round>
sdm_status relax_rounds(sdm_map *m, const char *what, uint32_t batch, uint64_t cap, const uint32_t *d_meta, uint32_t *h_meta, size_t words,
                        const uint32_t *h_cnt, const char *not_converged, GridOf grid_of, Round launch_round) {
  uint64_t round = 0;
  uint32_t grid = grid_of(0u);
  for (;;) {
    for (uint32_t k = 0; k < batch; ++k, ++round) HIP_TRY(launch_round(grid, (uint32_t)round));
    HIP_TRY(hipMemcpyAsync(h_meta, d_meta, words * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const uint32_t last = h_cnt[(round - 1) & 1u];
    if (last == 0u) return SDM_OK;
    if (round >= cap) {
      set_error(what, __FILE__, __LINE__, not_converged);
      return SDM_ERR_NOT_CONVERGED;
    }
    grid = grid_of(last);
  }
}

// the checks of the queries whose entries are points or cells, against the layer they read
template <class Layer>
sdm_status goal_query_check(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, const void *out, uint32_t flags, const char *what,
                            Layer sdm_map::*layer, const LayerName &name) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if ((xyz != nullptr) == (cells != nullptr)) return LAYER_REFUSE(what, "exactly one of xyz and cells must be given");
  SDM_TRY(query_check(m, xyz ? (const void *)xyz : (const void *)cells, n, out, flags, SDM_QUERY_ON_DEVICE, what));
  return layer_check(m, what, &(m->*layer), name);
}

// The paths of a route planner, after goal_query_check: launch(points, cells, count, len_cap, stride, rows, lens) enqueues
// one chunk of goals on m->stream (exactly one of points and cells is given); field_cells: the cells of the field, which no
// path has more of.
template <class Launch>
sdm_status goal_paths(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, int32_t max_len, int32_t *cells_out, int32_t *len_out,
                      uint32_t flags, const char *what, size_t field_cells, Launch launch) {
  if (max_len < 0 || (max_len > 0 && !cells_out)) return LAYER_REFUSE(what, "max_len < 0, or no cells_out for max_len > 0");
  if (n == 0) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  const unsigned char *in = xyz ? reinterpret_cast<const unsigned char *>(xyz) : reinterpret_cast<const unsigned char *>(cells);
  auto chunk_of = [&](const void *src, uint32_t c, uint32_t len_cap, size_t stride, void *rows, void *lens) {
    launch(xyz ? static_cast<const float *>(src) : nullptr, xyz ? nullptr : static_cast<const int32_t *>(src), c, len_cap, stride,
           static_cast<int32_t *>(rows), static_cast<int32_t *>(lens));
  };
  if (flags & SDM_QUERY_ON_DEVICE)  // (run_query's chunks: a row of the caller's is max_len cells of three words)
    return run_query(m, in, 12, len_out, 4, cells_out, (size_t)max_len * 12, n, flags, [&](const void *src, void *lens, void *rows, uint32_t c, hipStream_t) {
      chunk_of(src, c, (uint32_t)max_len, (size_t)max_len, rows, lens);
    });
  constexpr size_t CHUNK = (size_t)1 << 20;
  // host mode: through the queries' staging area, in chunks of whole rows; a staged row holds what a path can be long, and
  // only the cells a path has are copied into the caller's row
  const size_t row = std::min<size_t>((size_t)max_len, std::max<size_t>(field_cells, 1));
  const size_t chunk = std::min<size_t>((size_t)n, std::max<size_t>(1, std::min(CHUNK, ((size_t)16 << 20) / std::max<size_t>(row * 12, 1))));
  return run_staged(
      m, (size_t)n, chunk, nullptr, 0, {{StageCol::IN, const_cast<unsigned char *>(in), 12}, {StageCol::OUT, len_out, 4}, {StageCol::OUT_RAW, nullptr, row * 12}},
      [&](const unsigned char *, unsigned char *const *col, size_t c) -> sdm_status {
        chunk_of(col[0], (uint32_t)c, (uint32_t)row, row, col[2], col[1]);
        HIP_TRY(hipGetLastError());
        return SDM_OK;
      },
      [&](const unsigned char *const *col, size_t off, size_t c) {
        const int32_t *lens = reinterpret_cast<const int32_t *>(col[1]);
        for (size_t i = 0; i < c; ++i) {
          const size_t take = std::min<size_t>((size_t)lens[i], row);
          if (take) memcpy(cells_out + (off + i) * (size_t)max_len * 3, col[2] + i * row * 12, take * 12);
        }
      });
}

}  // namespace

}  // namespace sdm
