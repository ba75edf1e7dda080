// sdm_world.h — what the units of the world archive share (world.hip: the update, the getters and the queries;
// world_io.hip: import and retain; world_snapshot.hip: the kernels and host helpers the builds over the archive share;
// world_reach.hip: the travel-cost field over the bricks; world_frontiers.hip: the frontiers of the bricks; world_esdf.hip:
// the truncated distance field of the bricks; world_ground.hip: the height map and costmap over the bricks;
// world_ground_reach.hip: the 2-D travel-cost field over that costmap; world_rays.hip: segments and views through the
// bricks; world_mesh.hip: the faces and welded vertices of the bricks' surface; world_match.hip: foreign bricks scored
// against the archive under a window of whole-cell offsets; world_objects.hip: the connected same-key components of the
// bricks' occupied cells; world_changes.hip: the block's results against the archived bricks it overlaps, and the connected
// regions of what changed): the hash table's key, hash, lookup and
// insertion, which cells write, the header-word layout, the indices of the counters, an update's geometry, how an entry of
// a query becomes a world cell, the packing of brick coordinates and tile keys; the inline device code the layers share
//  - the 3 x 3 x 3 offset tables, a wave's loads of a brick, list indices, the 64-bit layer words and the
// lateral shifts inside them, the min-linking union-find with the seam body, the two ends of the brick-local labelling
// over it and the keyed sweep between them (5y); the host scaffold of a snapshot build (its buffers' one way to grow included) and of the two route planners, and
// the host entry points of world.hip and world_snapshot.hip that the other units call.  No kernel lives here: everything
// in the unnamed namespace has internal linkage and each unit compiles its own copy, so a kernel here would land in every
// object.
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
// world_snapshot.hip: nbr[27 r + k] = the rank in the caller's table of the brick at offset k (off_d) from brick r of the n of
// `coord`, NONE where the table has none or the offset leaves the int16 range; nbr[27 r + 13] = r
hipError_t launch_snapshot_neighbours(const uint32_t *coord, const unsigned long long *keys, const uint32_t *vals, uint32_t hmask, uint32_t n,
                                      uint32_t *nbr, hipStream_t s);
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

// ---- the 3 x 3 x 3 offsets: k = 13 + dx + 3 dy + 9 dz, a cell's neighbours and a brick's alike --------------------------
constexpr int off_d(int k, int a) { return a == 0 ? k % 3 - 1 : a == 1 ? (k / 3) % 3 - 1 : k / 9 - 1; }
constexpr int nb_bit(int dx, int dy, int dz) { return (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); }
constexpr int FACE_K[6] = {12, 14, 10, 16, 4, 22};  // the six faces: x-, x+, y-, y+, z-, z+
// the place of offset k among the six faces, -1 for an edge, a corner and the cell itself
constexpr int face_of(int k) {
  for (int f = 0; f < 6; ++f)
    if (FACE_K[f] == k) return f;
  return -1;
}
constexpr bool is_face(int k) { return face_of(k) >= 0; }
constexpr uint32_t face_moves() {
  uint32_t m = 0;
  for (int f = 0; f < 6; ++f) m |= 1u << FACE_K[f];
  return m;
}
constexpr uint32_t FACE_MOVES = face_moves();  // bit k: offset k is a face
constexpr bool offsets_agree() {
  uint32_t faces = 0;
  for (int k = 0; k < 27; ++k) {
    if (nb_bit(off_d(k, 0), off_d(k, 1), off_d(k, 2)) != k || is_face(k) != (face_of(k) >= 0)) return false;
    if (is_face(k) != (off_d(k, 0) * off_d(k, 0) + off_d(k, 1) * off_d(k, 1) + off_d(k, 2) * off_d(k, 2) == 1)) return false;
    faces |= is_face(k) ? 1u << k : 0u;
  }
  for (int f = 0; f < 6; ++f)  // (the order of the six: the axis, then the sign)
    if (off_d(FACE_K[f], f >> 1) != ((f & 1) ? 1 : -1)) return false;
  return faces == FACE_MOVES;
}
static_assert(offsets_agree(), "off_d, nb_bit, face_of, is_face and FACE_MOVES are one table");

// ---- a brick's cells, list indices ---------------------------------------------------------------------------------------
// "a wave per brick, a lane per (cx, cy)": the lane's cell of each of the eight layers of the brick at pool slot `slot`,
// every load issued before anything uses one
__device__ __forceinline__ void load_brick(const uint32_t *__restrict__ cells, uint32_t slot, uint32_t lane, uint32_t (&w)[8]) {
  const uint32_t *__restrict__ src = cells + (size_t)slot * 512u + lane;
#pragma unroll
  for (int l = 0; l < 8; ++l) w[l] = src[l * 64];
}
// the list index of bit b of word wi: the word's first index (the exclusive scan of the popcounts) + the set bits below b
__device__ __forceinline__ uint32_t list_index(const u64 *__restrict__ words, const uint32_t *__restrict__ pre, size_t wi, uint32_t b) {
  return pre[wi] + lane_rank(words[wi], b);
}
// the world cell of lane (cx + 8 cy) of layer z of brick (bx, by, bz), at list index `at`
__device__ __forceinline__ void store_world_cell(int32_t *__restrict__ xyz, uint32_t at, int bx, int by, int bz, uint32_t lane, int z) {
  xyz[3 * (size_t)at] = bx * 8 + (int)(lane & 7u);
  xyz[3 * (size_t)at + 1] = by * 8 + (int)(lane >> 3);
  xyz[3 * (size_t)at + 2] = bz * 8 + z;
}

// ---- 64-bit layer words: bit cx + 8 cy -----------------------------------------------------------------------------------
constexpr u64 COL0 = 0x0101010101010101ull, COL7 = 0x8080808080808080ull, ROW0 = 0xffull, ROW7 = 0xffull << 56;
// what the cells of a layer (own) see across lateral face DIR (x-, x+, y-, y+), nbr_word being the same layer of the brick
// beyond that face: a shift inside the word, the wrapping column masked out and the neighbour's column shifted in, or the
// neighbour's row.  What an absent brick reads, and where a brick's words lie, is the caller's.
template <int DIR>
__device__ __forceinline__ u64 across_lateral(u64 own, u64 nbr_word) {
  static_assert(DIR >= 0 && DIR < 4, "the four lateral faces");
  if (DIR == 0) return ((own << 1) & ~COL0) | ((nbr_word >> 7) & COL0);  // cx - 1: the bit below; column 0 looks at the neighbour's column 7
  if (DIR == 1) return ((own >> 1) & ~COL7) | ((nbr_word << 7) & COL7);
  if (DIR == 2) return (own << 8) | (nbr_word >> 56);                    // cy - 1: the row below; row 0 looks at the neighbour's row 7
  return (own >> 8) | (nbr_word << 56);
}

// ---- labels: the min-linking union-find over list indices, and what the two labelled layers do with it -------------------
// parent[a] <= a; a root is its own parent, and a component's root ends up as its smallest index whatever order the unions
// arrive in.  Within the launch that unites, every read of parent[] is a relaxed agent-scope atomic load or an atomic's
// return value: the L2s of the XCDs are not coherent for plain loads, and a plain load might also be kept in a register
// across the loop.  Relaxed is enough: nothing but parent[] itself is published through it, and the next launch reads with
// plain loads.  Lock-free: no thread waits for another; a failed link hands the loop a strictly smaller root.
__device__ __forceinline__ uint32_t parent_of(uint32_t *__restrict__ parent, uint32_t a) {
  return __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t lower_parent(uint32_t *__restrict__ parent, uint32_t a, uint32_t v) {  // -> what it was
  return __hip_atomic_fetch_min(parent + a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the root of a, halving the path on the way (a parent is only ever lowered to an ancestor: still the same component;
// every step goes to a strictly smaller index: at most n_cells steps)
__device__ __forceinline__ uint32_t find_root(uint32_t *__restrict__ parent, uint32_t a) {
  for (;;) {
    const uint32_t p = parent_of(parent, a);
    if (p >= a) return a;  // (p == a: a root; never above)
    const uint32_t gp = parent_of(parent, p);
    if (gp >= p) return p;
    lower_parent(parent, a, gp);
    a = gp;
  }
}
__device__ __forceinline__ void unite(uint32_t *__restrict__ parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = lower_parent(parent, hi, lo);
    if (old == hi) return;  // hi was still a root and now hangs below lo
    a = old;                // somebody linked hi below `old` (< hi) first: old and lo remain to be united
    b = lo;
  }
}

constexpr uint32_t NO_LABEL = 0xffffu;  // the local labelling: the cell is not listed
// The opening of a brick's local labelling: the eight words of brick r and, per layer, the lane's start label - its own
// cell word z * 64 + lane, NO_LABEL for a cell that is not listed.  False (wave-uniform) for a brick without a listed cell.
__device__ __forceinline__ bool local_labels(const u64 *__restrict__ words, uint32_t r, uint32_t lane, u64 (&m)[8], uint32_t (&v)[8]) {
#pragma unroll
  for (int z = 0; z < 8; ++z) m[z] = words[(size_t)r * 8u + z];
  if (!(m[0] | m[1] | m[2] | m[3] | m[4] | m[5] | m[6] | m[7])) return false;
#pragma unroll
  for (int z = 0; z < 8; ++z) v[z] = ((m[z] >> lane) & 1ull) ? (uint32_t)z * 64u + lane : NO_LABEL;
  return true;
}
// ... and its end: v[z] is the smallest cell word of the local component of the lane's cell of layer z; parent[] of the cell
// becomes the list index of that cell - one root per local component, no LDS, no global atomic
__device__ __forceinline__ void store_local_roots(const uint32_t (&v)[8], const u64 (&m)[8], const u64 *__restrict__ words,
                                                  const uint32_t *__restrict__ pre, uint32_t r, uint32_t lane, uint32_t n_cells,
                                                  uint32_t *__restrict__ parent) {
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    if (v[z] == NO_LABEL) continue;
    const uint32_t lz = v[z] >> 6, lb = v[z] & 63u;  // the local root: a cell word <= this cell's
    const uint32_t at = pre[(size_t)r * 8u + z] + lane_rank(m[z], lane);  // (list_index, on the word the lane holds since the opening)
    const uint32_t root = list_index(words, pre, (size_t)r * 8u + lz, lb);
    if (at < n_cells) parent[at] = root;
  }
}
// ... and what lies between the two, for the layers whose cells join under a key (world_objects.hip: label, or label and
// track; world_changes.hip: the class, or class and label pair).  A wave per brick, a lane per (cx, cy): k[z] is the key of the
// lane's cell of layer z, NO_KEY for a cell that is not listed (a key has 24 bits at most), v[z] its label from local_labels.
constexpr uint32_t NO_KEY = 0xffffffffu;
// a, or the neighbour's label t if it is smaller and bit `bit` of eq allows it (an equal key: both cells are listed, t is a
// label); the bit, spread over the word, turns a forbidden t into all ones
__device__ __forceinline__ uint32_t take_label(uint32_t a, uint32_t t, uint32_t eq, int bit) {
  return min(a, t | ~(uint32_t)((int)(eq << (31 - bit)) >> 31));
}
// The keys never change, so who may join whom is settled ONCE, then labels are swept until a sweep changes nothing (at most
// 512 sweeps): explicit comparisons against every neighbour, no separable minimum.  No LDS, no global memory.
template <bool FACE>
__device__ __forceinline__ void sweep_local_labels(const uint32_t (&k)[8], uint32_t (&v)[8], uint32_t lane) {
  uint32_t eq[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) eq[z] = 0u;
  const int cx = (int)(lane & 7u), cy = (int)(lane >> 3);
  // who may join whom: bit nb_bit(dx, dy, dz) of eq[c] - that neighbour of cell c lies in the brick, is listed and
  // carries c's key.  The lane of a neighbour beyond the brick's border is the lane itself, and its key reads NO_KEY.  The
  // in-layer directions are a loop that stays a loop (i: dx = i % 3 - 1, dy = i / 3 - 1; for 6-connectivity the four
  // lateral ones, the column's own z neighbours apart): unrolled, the 208 tests of a sweep, which no sweep changes, would
  // be hoisted out of the sweeps and held in registers.
#pragma unroll 1
  for (int i = 0; i < (FACE ? 4 : 9); ++i) {
    const int d = FACE ? 2 * i + 1 : i, dx = d % 3 - 1, dy = d / 3 - 1;
    const bool inside = cx + dx >= 0 && cx + dx <= 7 && cy + dy >= 0 && cy + dy <= 7;
    const int from = inside ? (int)lane + dx + 8 * dy : (int)lane;
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      const uint32_t got = (uint32_t)__shfl((int)k[z], from, 64), nk = inside ? got : NO_KEY;
#pragma unroll
      for (int dz = FACE ? 0 : -1; dz <= (FACE ? 0 : 1); ++dz) {
        const int c = z - dz;  // the cell whose neighbour at (dx, dy, dz) is this one
        if (c < 0 || c > 7) continue;
        eq[c] |= (k[c] != NO_KEY && nk == k[c] ? 1u : 0u) << (d + 9 * (dz + 1));
      }
    }
  }
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    if (FACE && z > 0) eq[z] |= (k[z] != NO_KEY && k[z - 1] == k[z] ? 1u : 0u) << nb_bit(0, 0, -1);
    if (FACE && z < 7) eq[z] |= (k[z] != NO_KEY && k[z + 1] == k[z] ? 1u : 0u) << nb_bit(0, 0, 1);
    eq[z] &= ~(1u << nb_bit(0, 0, 0));  // (the cell itself)
  }
  for (int sweep = 0; sweep < 512; ++sweep) {  // a label falls by at least one cell of its component a sweep
    uint32_t a[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) a[z] = v[z];
#pragma unroll 1
    for (int i = 0; i < (FACE ? 4 : 9); ++i) {
      const int d = FACE ? 2 * i + 1 : i, dx = d % 3 - 1, dy = d / 3 - 1;
      const bool inside = cx + dx >= 0 && cx + dx <= 7 && cy + dy >= 0 && cy + dy <= 7;
      const int from = inside ? (int)lane + dx + 8 * dy : (int)lane;
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        const uint32_t t = (uint32_t)__shfl((int)v[z], from, 64);
#pragma unroll
        for (int dz = FACE ? 0 : -1; dz <= (FACE ? 0 : 1); ++dz) {
          const int c = z - dz;
          if (c < 0 || c > 7) continue;
          a[c] = take_label(a[c], t, eq[c], d + 9 * (dz + 1));
        }
      }
    }
    if (FACE) {
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        if (z > 0) a[z] = take_label(a[z], v[z - 1], eq[z], nb_bit(0, 0, -1));
        if (z < 7) a[z] = take_label(a[z], v[z + 1], eq[z], nb_bit(0, 0, 1));
      }
    }
    bool changed = false;
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      changed = changed || a[z] != v[z];
      v[z] = a[z];
    }
    if (!__ballot(changed)) break;
  }
}
// The seams, a wave per word and a lane per cell: the cell `lane` of layer lz of brick r (of n), if it is listed and lies on
// the brick's shell, looks at its 26 (FACE: 6) neighbours that lie in a field brick of lower rank and unites with those that
// are listed and carry its key.  nbr: the 27 ranks round every brick, NONE for none.  key_of_cell(list index): "the same key"
// is the predicate under which two listed cells join - an equivalence whatever the caller passes, as a union-find needs it,
// and the cell's own key is fetched once, before the first neighbour; a constant key joins every listed pair.
template <bool FACE, class Key>
__device__ __forceinline__ void seam_unions(const uint32_t *__restrict__ nbr, const u64 *__restrict__ words, const uint32_t *__restrict__ pre,
                                            uint32_t r, int lz, uint32_t lane, uint32_t n, uint32_t n_cells, uint32_t *__restrict__ parent,
                                            Key key_of_cell) {
  if (r >= n) return;  // (wave-uniform)
  const u64 mw = words[(size_t)r * 8u + (uint32_t)lz];
  const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
  const bool shell = lx == 0 || lx == 7 || ly == 0 || ly == 7 || lz == 0 || lz == 7;
  if (!((mw >> lane) & 1ull) || !shell) return;
  const uint32_t at = list_index(words, pre, (size_t)r * 8u + (uint32_t)lz, lane);
  if (at >= n_cells) return;  // (never)
  const auto key = key_of_cell(at);
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    if (k == 13 || (FACE && !is_face(k))) continue;
    const int x = lx + off_d(k, 0), y = ly + off_d(k, 1), z = lz + off_d(k, 2);
    const int ox = brick_off(x), oy = brick_off(y), oz = brick_off(z);
    if (ox == 0 && oy == 0 && oz == 0) continue;  // inside the brick: the local labelling has united them
    const uint32_t nr = nbr[(size_t)r * 27u + (uint32_t)(13 + ox + 3 * oy + 9 * oz)];
    if (nr >= r) continue;  // absent, outside the field, or later in cell order: that cell unites with this one
    const uint32_t wi = nr * 8u + (uint32_t)(z & 7), b = (uint32_t)((x & 7) + 8 * (y & 7));
    const u64 nw = words[wi];
    if (!((nw >> b) & 1ull)) continue;
    const uint32_t other = list_index(words, pre, wi, b);
    if (other < n_cells && key_of_cell(other) == key) unite(parent, at, other);
  }
}

// ---- the host scaffold --------------------------------------------------------------------------------------------------
// the slots of a table that is at most half full with `items` keys
inline uint32_t table_slots(size_t items) {
  uint32_t slots = 2;
  while (slots < 2 * items) slots <<= 1;
  return slots;
}
// The one way a snapshot's buffers grow.  A set of buffers shares a capacity, *cap; while need <= *cap nothing happens.
// Otherwise every buffer listed is released, *cap is 0, every buffer is allocated - in the order listed - at the size the
// caller states for the new capacity `to`, and only then *cap = to: an allocation that fails leaves *cap == 0 and the next
// build starts over.  The caller rounds `to` (256 bricks or tiles, the route planners' too; 1024 objects; 4096 cells, faces
// and vertices; frontiers' pool slots not at all) and writes every buffer's elements out, where a reader checks them against
// the BYTES_PER_* constants of sdm.h.  The stream is idle when this is called, or there were no buffers before.  then():
// what else has to succeed before the capacity counts - it runs only when the buffers grew, after the last allocation.  A
// set with a second capacity (the mesh's cap_slots) sets it there; to have it 0 while the first is, the caller zeroes it
// before the call under this function's own test, need > *cap - the one thing a caller has to know of the inside.
struct GrowBuf {
  void **p;
  size_t bytes;
};
template <typename T>
GrowBuf buf(T **p, size_t n) { return {(void **)p, std::max<size_t>(n, 1) * sizeof(T)}; }  // (alloc_tracked's size)
template <class Then>
sdm_status grow_buffers(sdm_map *m, size_t need, size_t to, size_t *cap, std::initializer_list<GrowBuf> bufs, Then then) {
  if (need <= *cap) return SDM_OK;
  for (const GrowBuf &b : bufs) map_release(m, b.p);
  *cap = 0;
  for (const GrowBuf &b : bufs) SDM_TRY(map_alloc(m, b.p, b.bytes, false));
  SDM_TRY(then());
  *cap = to;
  return SDM_OK;
}
inline sdm_status grow_buffers(sdm_map *m, size_t need, size_t to, size_t *cap, std::initializer_list<GrowBuf> bufs) {
  return grow_buffers(m, need, to, cap, bufs, [] { return SDM_OK; });
}
inline size_t round_up(size_t n, size_t to) { return (n + to - 1) & ~(to - 1); }  // (to: a power of two)

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
