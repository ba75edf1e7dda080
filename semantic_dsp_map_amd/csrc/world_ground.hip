// world_ground.hip — the world ground layer: a height map, a costmap and a truncated distance to the nearest lethal column
// over the bricks of the world archive, for a robot that stands on the ground at a place the block has long left (gfx950;
// include/sdm.h, "world ground layer").  The cell rules are ground.hip's, the host scaffold is world_esdf.hip's.
//
// A tile is the 8 x 8 columns over one (bu, bv) of the two axes that are not the up axis; it exists where the archive has a
// brick whose heights meet the read window h_lo .. h_hi + clearance.  The build is a snapshot: the tiles' keys, a hash
// table of its own from tile key to rank, 64 cells, 64 distances and one lethal word per tile; no pool slot is kept.
//   k_wg_claim     a thread per archived brick in brick order: a brick whose heights meet the window (and whose tile lies in
//               the box) claims its tile key in the layer's table; the one thread whose compare-and-swap found the slot
//               empty flags the brick.  So every tile is flagged exactly once, whatever the arrival order, and the sort
//               below sees each tile once instead of once per brick of its column.
//   snapshot_rank  (world_snapshot.hip) ranks the flags; the entry behind the last brick ends as the number of tiles.
//   k_wg_keys      a thread per archived brick: a flagged one writes its tile key at its rank.
//   radix_sort_pairs 32 bits   the keys, bu + 32768 | (bv + 32768) << 16, ascending: tile order (bv, bu).
//   k_wg_tiles     a thread per tile: the key at its rank, and the rank beside the key in the table.
//   k_wg_columns<A>   a wave per tile, a lane per column, the read window from the top down, brick by brick: one wave-uniform
//               lookup in the archive's table per brick, the brick's eight cells of every column loaded before any is
//               looked at (up axis z: eight rows of 64 consecutive words; y: eight rows of eight 32-byte runs; x: the
//               column's own 32 bytes, two 16-byte loads), the run of passable cells above carried in a register.  An
//               absent brick costs the lookup and no load: its cells are unknown all alike.
//   k_wg_cost      a wave per tile: the step bit (the four neighbours' levels, across the tile's sides through the table),
//               the lethal bit, the class byte, the tile's lethal word (a ballot) and the counts.
//   k_wg_dist<H>   a wave per tile: the lethal words of the (2 H + 1)^2 tiles round it to LDS (H = 1 up to R = 8, 2 beyond),
//               an absent tile as zeros, or ones under ABSENT_IS_LETHAL; per row within R the nearest set bit on either
//               side of each of the tile's eight columns (a mask and __clzll, a shift and __ffsll: k_we_build's x pass),
//               then per column the windowed minimum over the rows.  Integer, truncated at R^2, one 2-byte store a column.
//   k_query_world_ground       a lane per point: its cell, one table lookup, two loads; five 8-byte stores.
//   k_query_world_footprints   a wave per footprint: the tiles of a rectangle that holds every column the rule can cover,
//               a lane per column of the tile, one wave-uniform lookup per tile that has a covered column.
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_ground_options) == 80 && sizeof(sdm_world_ground_info) == 136 && sizeof(sdm_world_ground_result) == 40 &&
                  sizeof(sdm_world_footprint_result) == 40 && sizeof(sdm_ground_cell) == 8 && sizeof(sdm_footprint) == 24,
              "sdm.h layout");
static_assert(offsetof(sdm_world_ground_options, tmin) == 32 && offsetof(sdm_world_ground_options, support_labels) == 48 &&
                  offsetof(sdm_world_ground_info, n_ground) == 16 && offsetof(sdm_world_ground_info, options) == 56 &&
                  offsetof(sdm_world_ground_result, cell) == 20 && offsetof(sdm_world_ground_result, dist) == 28 &&
                  offsetof(sdm_world_footprint_result, level_min) == 20 && offsetof(sdm_world_footprint_result, first_lethal) == 28,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;  // the kernels of a thread or a wave per item
constexpr int DT = 64;   // k_wg_dist: one wave
constexpr uint32_t ALL_WG_FLAGS = SDM_WORLD_GROUND_UNKNOWN_PASSABLE | SDM_WORLD_GROUND_IGNORE_MOVABLE | SDM_WORLD_GROUND_NONE_IS_LETHAL |
                                  SDM_WORLD_GROUND_ABSENT_IS_LETHAL | SDM_WORLD_GROUND_BOX;
constexpr uint32_t NO_LEVEL = 0xffffu;
constexpr int CELL_MIN = -262144, CELL_MAX = 262143;  // the world cells of the brick range
// the build's counters, 64 bits each, in G_SPREAD copies - a wave adds to copy (tile & (G_SPREAD - 1)), the getter combines
// them (tens of thousands of atomics on one address take milliseconds).  G_LMIN holds the largest
// 0xffff - level and G_LMAX the largest level + 1, so that zero is "none" for both.  The landing area has one word more,
// for the count the build waits for.
enum { G_GROUND = 0, G_OBSTACLE, G_NONE, G_STEP, G_LETHAL, G_LMIN, G_LMAX, G_PAD, G_ROW, G_SPREAD = 64, G_WORDS = G_ROW * G_SPREAD };

constexpr size_t ARCH_BYTES = 4 + 4 + 2 * (8 + 4);                 // flag, rank, two hash slots
constexpr size_t TILE_BYTES = 64 * 8 + 64 * 2 + 8 + 4 + 4 * 4;     // cells, d2, lethal word, key, the sort's four words
static_assert(ARCH_BYTES == SDM_WORLD_GROUND_BYTES_PER_ARCHIVED_BRICK && TILE_BYTES == SDM_WORLD_GROUND_BYTES_PER_TILE, "sdm.h states the bytes");

// What the kernels know of a build (by value).  Heights are relative to h_lo from here on: rel = h - h_lo, the band is
// 0 .. span, the read window 0 .. rel_top.  Height brick hb_lo + k holds rel 8 k - lo_off .. 8 k - lo_off + 7.
struct Band {
  int a, sign, au, av;
  int h_lo, hb_lo, n_hb, lo_off;  // n_hb height bricks meet the window
  int span, rel_top, clearance, max_step;
  uint32_t flags;
  uint32_t labels[8];
  int tlo[2], thi[2];
  uint32_t use_box;
};

template <int H>
struct DistShape {
  static constexpr int W = 2 * H + 1, S = 8 * W;
  static constexpr size_t LDS = (size_t)W * W * 8 + (size_t)S * 8;
};
static_assert(DistShape<1>::LDS == 72 + 192 && DistShape<2>::LDS == 200 + 320, "DESIGN.md 5q states the bytes");

// the brick's coordinates as (up, u, v)
__device__ __forceinline__ void brick_auv(const Band &b, const uint32_t *__restrict__ hdr, uint32_t slot, int &ba, int &bu, int &bv) {
  int c[3];
  brick_of(hdr[(size_t)slot * HDR_WORDS], hdr[(size_t)slot * HDR_WORDS + 1], c[0], c[1], c[2]);
  ba = b.a == 0 ? c[0] : (b.a == 1 ? c[1] : c[2]);
  bu = b.au == 0 ? c[0] : c[1];
  bv = b.av == 1 ? c[1] : c[2];
}

// ---- the tile set ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wg_claim(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr, uint32_t n_arch, Band b,
                                                 u64 *__restrict__ keys, uint32_t hmask, uint32_t *__restrict__ flag) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j > n_arch) return;
  uint32_t first = 0u;
  if (j < n_arch) {  // (the entry behind the last brick: the scan leaves the number of flags there)
    int ba, bu, bv;
    brick_auv(b, hdr, order[j], ba, bu, bv);
    const int hb = b.sign > 0 ? ba : -1 - ba;
    bool in = hb >= b.hb_lo && hb - b.hb_lo < b.n_hb;
    if (b.use_box) in = in && bu >= b.tlo[0] && bu <= b.thi[0] && bv >= b.tlo[1] && bv <= b.thi[1];
    if (in) {
      const u64 key = tile_key(bu, bv);
      uint32_t h = key_hash(key) & hmask;
      for (uint32_t i = 0; i <= hmask; ++i) {  // (the table is at most half full)
        const u64 was = atomicCAS(keys + h, EMPTY_KEY, key);
        if (was == EMPTY_KEY) first = 1u;
        if (was == EMPTY_KEY || was == key) break;
        h = (h + 1u) & hmask;
      }
    }
  }
  flag[j] = first;
}

__global__ __launch_bounds__(QT) void k_wg_keys(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ flag,
                                                const uint32_t *__restrict__ rank, uint32_t n_arch, uint32_t n, Band b, uint32_t *__restrict__ key_out,
                                                uint32_t *__restrict__ val_out) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j >= n_arch || !flag[j]) return;
  const uint32_t r = rank[j];
  if (r >= n) return;  // (never: the scan's total is n)
  int ba, bu, bv;
  brick_auv(b, hdr, order[j], ba, bu, bv);
  key_out[r] = (uint32_t)tile_key(bu, bv);
  val_out[r] = j;
}

__global__ __launch_bounds__(QT) void k_wg_tiles(const uint32_t *__restrict__ sorted, uint32_t n, const u64 *__restrict__ keys, uint32_t *__restrict__ vals,
                                                 uint32_t hmask, uint32_t *__restrict__ coord) {
  const uint32_t r = blockIdx.x * QT + threadIdx.x;
  if (r >= n) return;
  const uint32_t k32 = sorted[r];
  coord[r] = k32;
  const u64 key = (u64)k32;
  uint32_t h = key_hash(key) & hmask;
  for (uint32_t i = 0; i <= hmask; ++i) {  // (the key is there: k_wg_claim put it)
    const u64 k = keys[h];
    if (k == key) {
      vals[h] = r;
      return;
    }
    if (k == EMPTY_KEY) return;
    h = (h + 1u) & hmask;
  }
}

// ---- the columns -------------------------------------------------------------------------------------------------------
// the classes of an archived word: bit 0 solid, bit 1 not passable, bit 2 support candidate, bit 3 unknown (ground.hip's)
__device__ __forceinline__ uint32_t cell_class(const Band &g, uint32_t w1, int max_movable) {
  const int occ = occ_of(w1);
  const uint32_t track = w1 & 0xffffu, label = (w1 >> 16) & 0xffu;
  const bool movable = track >= 1u && (int)track <= max_movable;
  const bool solid = occ >= 1 && !((g.flags & SDM_WORLD_GROUND_IGNORE_MOVABLE) && movable);
  const bool passable = occ == 0 || (occ >= 1 && !solid) || ((g.flags & SDM_WORLD_GROUND_UNKNOWN_PASSABLE) && occ == -1);
  const bool cand = solid && !movable && ((g.labels[label >> 5] >> (label & 31u)) & 1u);
  return (solid ? 1u : 0u) | (passable ? 0u : 2u) | (cand ? 4u : 0u) | (occ == -1 ? 8u : 0u);
}

// A = the up axis.  Lane cu | cv << 3 holds column (cu, cv) of the tile.
template <int A>
__global__ __launch_bounds__(QT) void k_wg_columns(const uint32_t *__restrict__ coord, uint32_t n_tiles, const u64 *__restrict__ akeys,
                                                   const uint32_t *__restrict__ avals, uint32_t ahmask, uint32_t n_arch,
                                                   const uint32_t *__restrict__ acells, Band b, int max_movable, uint2 *__restrict__ cells) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (t >= n_tiles) return;  // (wave-uniform)
  int bu, bv;
  tile_of(coord[t], bu, bv);
  const uint32_t cu = lane & 7u, cv = lane >> 3;
  // the word of the column's cell c along the up axis: x | y << 3 | z << 6
  const uint32_t off = A == 2 ? lane : (A == 1 ? cu | (cv << 6) : lane << 3);
  constexpr uint32_t STRIDE = A == 2 ? 64u : (A == 1 ? 8u : 1u);
  int run = 0;  // passable cells directly above the current one, inside the window
  uint32_t level = NO_LEVEL, top = NO_LEVEL, label = 0u, headroom = 0u, n_unknown = 0u;
  for (int k = b.n_hb - 1; k >= 0; --k) {
    const int hb = b.hb_lo + k, ba = b.sign > 0 ? hb : -1 - hb;
    const int rel0 = 8 * k - b.lo_off;  // of the brick's lowest cell
    uint32_t slot = NONE;
    if (ba >= -32768 && ba <= 32767) {  // (a coordinate beyond would alias another brick's key)
      const u64 bk = A == 0 ? brick_key(ba, bu, bv) : (A == 1 ? brick_key(bu, ba, bv) : brick_key(bu, bv, ba));
      slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)world_find(akeys, avals, ahmask, bk));
      if (slot >= n_arch) slot = NONE;
    }
    if (slot == NONE) {  // eight unknown cells, those inside the window (uniform)
      const int lo = max(0, -rel0), hi = min(7, b.rel_top - rel0), hi_band = min(7, b.span - rel0);
      n_unknown += (uint32_t)max(0, hi_band - lo + 1);
      run = (b.flags & SDM_WORLD_GROUND_UNKNOWN_PASSABLE) ? run + max(0, hi - lo + 1) : 0;
      continue;
    }
    const uint32_t *__restrict__ src = acells + (size_t)slot * 512u + off;
    uint32_t w[8];  // by height inside the brick
    if (A == 0) {
      const uint4 q0 = *reinterpret_cast<const uint4 *>(src), q1 = *reinterpret_cast<const uint4 *>(src + 4);
      const uint32_t c[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
      for (int l = 0; l < 8; ++l) w[l] = b.sign > 0 ? c[l] : c[7 - l];
    } else {
      uint32_t c[8];
#pragma unroll
      for (int l = 0; l < 8; ++l) c[l] = src[(uint32_t)l * STRIDE];
#pragma unroll
      for (int l = 0; l < 8; ++l) w[l] = b.sign > 0 ? c[l] : c[7 - l];
    }
#pragma unroll
    for (int l = 7; l >= 0; --l) {
      const int rel = rel0 + l;
      if (rel < 0 || rel > b.rel_top) continue;  // (uniform: outside the window)
      const uint32_t c = cell_class(b, w[l], max_movable);
      if (rel <= b.span) {
        if ((c & 1u) && top == NO_LEVEL) top = (uint32_t)rel;
        if ((c & 4u) && level == NO_LEVEL && run >= b.clearance) {
          level = (uint32_t)rel;
          label = (w[l] >> 16) & 0xffu;
          headroom = (uint32_t)run;
        }
        n_unknown += (c >> 3) & 1u;
      }
      run = (c & 2u) ? 0 : run + 1;
    }
  }
  const uint32_t cls = level != NO_LEVEL ? 1u : (top != NO_LEVEL ? 2u : 0u);  // (k_wg_cost adds the step and lethal bits)
  cells[(size_t)t * 64u + lane] = make_uint2(level | (top << 16), label | (cls << 8) | (min(headroom, 255u) << 16) | (min(n_unknown, 255u) << 24));
}

// ---- step, lethal, the counts ----------------------------------------------------------------------------------------
// A neighbour's level is read from the cell's first half-word, which no launch but k_wg_columns writes; this one stores the
// class byte alone.
__global__ __launch_bounds__(QT) void k_wg_cost(const uint32_t *__restrict__ coord, uint32_t n_tiles, const u64 *__restrict__ keys,
                                                const uint32_t *__restrict__ vals, uint32_t hmask, Band b, sdm_ground_cell *__restrict__ cells,
                                                u64 *__restrict__ lethal_out, u64 *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (t >= n_tiles) return;  // (wave-uniform)
  int bu, bv;
  tile_of(coord[t], bu, bv);
  uint32_t nt[4];  // the tiles at u - 1, u + 1, v - 1, v + 1
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int tu = bu + (q == 0 ? -1 : (q == 1 ? 1 : 0)), tv = bv + (q == 2 ? -1 : (q == 3 ? 1 : 0));
    uint32_t r = NONE;
    if (tile_in_range(tu, tv)) r = (uint32_t)__builtin_amdgcn_readfirstlane((int)world_find(keys, vals, hmask, tile_key(tu, tv)));
    nt[q] = r < n_tiles ? r : NONE;
  }
  const uint16_t *level_of = reinterpret_cast<const uint16_t *>(cells);  // [column * 4]
  const size_t at = (size_t)t * 64u + lane;
  const uint32_t cu = lane & 7u, cv = lane >> 3;
  const uint32_t lv = level_of[at * 4], k = cells[at].cls & 3u;
  uint32_t nb[4];
  nb[0] = cu > 0u ? level_of[(at - 1) * 4] : (nt[0] != NONE ? level_of[((size_t)nt[0] * 64u + (7u | (cv << 3))) * 4] : NO_LEVEL);
  nb[1] = cu < 7u ? level_of[(at + 1) * 4] : (nt[1] != NONE ? level_of[((size_t)nt[1] * 64u + (cv << 3)) * 4] : NO_LEVEL);
  nb[2] = cv > 0u ? level_of[(at - 8) * 4] : (nt[2] != NONE ? level_of[((size_t)nt[2] * 64u + (cu | (7u << 3))) * 4] : NO_LEVEL);
  nb[3] = cv < 7u ? level_of[(at + 8) * 4] : (nt[3] != NONE ? level_of[((size_t)nt[3] * 64u + cu) * 4] : NO_LEVEL);
  bool step = false;
  if (k == 1u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) step = step || (nb[q] != NO_LEVEL && lv > nb[q] + (uint32_t)b.max_step);
  }
  const bool lethal = k == 2u || step || (k == 0u && (b.flags & SDM_WORLD_GROUND_NONE_IS_LETHAL));
  cells[at].cls = (uint8_t)(k | (step ? 4u : 0u) | (lethal ? 8u : 0u));
  const u64 lm = __ballot(lethal);
  const uint32_t n[5] = {(uint32_t)__popcll(__ballot(k == 1u)), (uint32_t)__popcll(__ballot(k == 2u)), (uint32_t)__popcll(__ballot(k == 0u)),
                         (uint32_t)__popcll(__ballot(step)), (uint32_t)__popcll(lm)};
  const uint32_t lo = wave_max(k == 1u ? 0xffffu - lv : 0u), hi = wave_max(k == 1u ? lv + 1u : 0u);
  if (lane == 0) lethal_out[t] = lm;
  u64 *mine = meta + (size_t)(t & (uint32_t)(G_SPREAD - 1)) * G_ROW;
  if (lane < 5u) {
    uint32_t v = 0u;
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if ((int)lane == q) v = n[q];
    if (v) atomicAdd(mine + lane, (u64)v);
  } else if (lane == (uint32_t)G_LMIN) {
    if (lo) atomicMax(mine + G_LMIN, (u64)lo);
  } else if (lane == (uint32_t)G_LMAX) {
    if (hi) atomicMax(mine + G_LMAX, (u64)hi);
  }
}

// ---- the distance ------------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(DT) void k_wg_dist(const uint32_t *__restrict__ coord, const u64 *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                uint32_t hmask, uint32_t n_tiles, const u64 *__restrict__ lethal, int R, u64 absent_reads,
                                                uint16_t *__restrict__ d2) {
  constexpr int W = DistShape<H>::W, S = DistShape<H>::S;
  __shared__ u64 s_let[W * W];  // [tile v][tile u]: the lethal word of that tile, bit cu | cv << 3
  __shared__ u64 s_x[S];        // [row]: eight bytes, the distance along the row to the nearest lethal column, 255: none within R
  const int tid = (int)threadIdx.x;
  const uint32_t t = blockIdx.x;
  if (tid < W * W) {
    const uint32_t key = coord[t];
    const int tu = (int)(key & 0xffffu) - 32768 + tid % W - H, tv = (int)(key >> 16) - 32768 + tid / W - H;
    const uint32_t r = tile_in_range(tu, tv) ? world_find(keys, vals, hmask, tile_key(tu, tv)) : NONE;
    s_let[tid] = r < n_tiles ? lethal[r] : absent_reads;
  }
  __syncthreads();
  const int T = 8 + 2 * R, base = 8 * H - R, R2 = R * R;  // the rows within R of the tile: base .. base + T - 1 (T <= 40 < DT)
  if (tid < T) {
    const int y = base + tid, tvi = y >> 3, sh = 8 * (y & 7);
    u64 row = 0ull;  // the row across the W tiles: bit 8 * tile + cu (a tile's word wraps every eight columns)
#pragma unroll
    for (int tui = 0; tui < W; ++tui) row |= ((s_let[tvi * W + tui] >> sh) & 0xffull) << (8 * tui);
    u64 out = 0ull;
#pragma unroll
    for (int cx = 0; cx < 8; ++cx) {
      const int p = 8 * H + cx;
      const u64 below = row & ((2ull << p) - 1ull), above = row >> p;  // both hold the column itself
      const int dl = below ? p - (63 - __clzll((long long)below)) : 64, dr = above ? __ffsll((long long)above) - 1 : 64;
      const int dx = min(dl, dr);
      out |= (u64)(uint32_t)(dx <= R ? dx : 255) << (8 * cx);
    }
    s_x[y] = out;
  }
  __syncthreads();
  const int cx = tid & 7, y = 8 * H + (tid >> 3);
  int best = 0xffff;
  for (int k = -R; k <= R; ++k) {
    const int dx = (int)((s_x[y + k] >> (8 * cx)) & 0xffull);
    const int v = dx * dx + k * k;  // (255: above every R^2)
    if (v <= R2) best = min(best, v);
  }
  d2[(size_t)t * 64u + (uint32_t)tid] = (uint16_t)best;
}

// ---- the queries -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_query_world_ground(const float *__restrict__ xyz, const int32_t *__restrict__ in_cells, uint32_t n, float recip,
                                                           float voxel_size, Band b, int R, const u64 *__restrict__ keys,
                                                           const uint32_t *__restrict__ vals, uint32_t hmask, uint32_t n_tiles,
                                                           const uint2 *__restrict__ cells, const uint16_t *__restrict__ d2, uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n) return;
  int g[3];
  const bool ok = entry_cell(xyz, in_cells, i, recip, g);
  // (the axes are picked by selects, not by indexing with a runtime value: the array stays in registers)
  const int ga = b.a == 0 ? g[0] : (b.a == 1 ? g[1] : g[2]);
  const int iu = ok ? (b.au == 0 ? g[0] : g[1]) : 0, iv = ok ? (b.av == 1 ? g[1] : g[2]) : 0;
  const uint32_t r = ok ? world_find(keys, vals, hmask, tile_key(iu >> 3, iv >> 3)) : NONE;
  uint2 cell = make_uint2(NO_LEVEL | (NO_LEVEL << 16), 0u);
  uint32_t dd = 0xffffffffu, status = 3u;
  float surface = 0.f, dist = -1.f;
  int above = INT32_MIN;
  if (r < n_tiles) {
    const size_t at = (size_t)r * 64u + (uint32_t)((iu & 7) | ((iv & 7) << 3));
    cell = cells[at];
    const uint32_t v = d2[at];
    status = 0u;
    if (v == 0xffffu) {
      dd = SDM_WORLD_GROUND_FAR;
      dist = sqrtf((float)(R * R + 1)) * voxel_size;  // a lower bound
    } else {
      dd = v;
      dist = sqrtf((float)v) * voxel_size;
    }
    const uint32_t level = cell.x & 0xffffu;
    if (level != NO_LEVEL) {
      const int hl = b.h_lo + (int)level, hp = b.sign > 0 ? ga : -1 - ga;
      above = hp - hl;
      const int k = b.sign > 0 ? hl + 1 : -1 - hl;  // the world coordinate of the level cell's upper face
      surface = (float)k * voxel_size;
    }
  }
  uint2 *__restrict__ o = out + 5 * (size_t)i;
  o[0] = make_uint2((uint32_t)iu, (uint32_t)iv);
  o[1] = make_uint2(dd, __float_as_uint(surface));
  o[2] = make_uint2((uint32_t)above, cell.x);
  o[3] = make_uint2(cell.y, __float_as_uint(dist));
  o[4] = make_uint2(status, 0u);
}

__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s, 64);
    const u64 o = ((u64)hi << 32) | lo;
    v = o < v ? o : v;
  }
  return v;
}

// One wave per footprint.  With |dir|^2 >= 1/2 a covered centre lies within sqrt(2) * (half_len + half_wid) of the
// footprint's centre; the rectangle takes 1.5 times that sum, two columns more and a few float32 steps of the centre's
// magnitude, cut to the columns of the brick range, and the wave tests every column of every tile that meets it.
__global__ __launch_bounds__(QT) void k_query_world_footprints(const sdm_footprint *__restrict__ fps, uint32_t n, float recip, float size,
                                                               const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                               uint32_t n_tiles, const uint2 *__restrict__ cells, const uint16_t *__restrict__ d2,
                                                               uint2 *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (p >= n) return;  // (whole waves)
  const sdm_footprint fp = fps[p];
  const float reach = fp.half_len + fp.half_wid;
  const bool finite = isfinite(fp.center_u) && isfinite(fp.center_v) && isfinite(fp.dir_u) && isfinite(fp.dir_v) && isfinite(fp.half_len) &&
                      isfinite(fp.half_wid);
  int i0 = 0, i1 = -1, j0 = 0, j1 = -1;  // [i0, i1] x [j0, j1], empty
  if (finite && !(reach > 64.f * size) && fp.dir_u * fp.dir_u + fp.dir_v * fp.dir_v >= 0.5f) {
    const float r = 1.5f * reach * recip + 2.f;
    const float cu = fp.center_u * recip, cv = fp.center_v * recip;
    const float eu = fabsf(cu) * 0x1p-20f, ev = fabsf(cv) * 0x1p-20f;
    // (clamped as floats: no cast of a value far outside the range)
    i0 = (int)fminf(fmaxf(floorf(cu - r - eu), (float)CELL_MIN), (float)CELL_MAX + 1.f);
    i1 = (int)fminf(fmaxf(ceilf(cu + r + eu), (float)CELL_MIN - 1.f), (float)CELL_MAX);
    j0 = (int)fminf(fmaxf(floorf(cv - r - ev), (float)CELL_MIN), (float)CELL_MAX + 1.f);
    j1 = (int)fminf(fmaxf(ceilf(cv + r + ev), (float)CELL_MIN - 1.f), (float)CELL_MAX);
  }
  uint32_t n_cols = 0, n_lethal = 0, n_none = 0, n_ground = 0, n_absent = 0;
  uint32_t lv_min = NO_LEVEL, lv_max = 0u, min_d2 = 0xffffffffu;
  u64 first = ~0ull;
  if (i1 >= i0 && j1 >= j0) {  // (uniform)
    const int cu = (int)(lane & 7u), cv = (int)(lane >> 3);
    for (int tv = j0 >> 3; tv <= (j1 >> 3); ++tv)
      for (int tu = i0 >> 3; tu <= (i1 >> 3); ++tu) {
        const int i = tu * 8 + cu, j = tv * 8 + cv;
        const float pu = ((float)i + 0.5f) * size, pv = ((float)j + 0.5f) * size;
        const float du = pu - fp.center_u, dv = pv - fp.center_v;
        const bool covered = fabsf(du * fp.dir_u + dv * fp.dir_v) <= fp.half_len && fabsf(dv * fp.dir_u - du * fp.dir_v) <= fp.half_wid;
        const u64 cm = __ballot(covered);
        if (!cm) continue;  // (uniform)
        const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)world_find(keys, vals, hmask, tile_key(tu, tv)));
        if (r >= n_tiles) {
          n_absent += (uint32_t)__popcll(cm);
          continue;
        }
        uint32_t cls = 0u;
        if (covered) {
          const size_t at = (size_t)r * 64u + lane;
          const uint2 c = cells[at];
          const uint32_t v = d2[at];
          cls = (c.y >> 8) & 0xffu;
          min_d2 = min(min_d2, v == 0xffffu ? (uint32_t)SDM_WORLD_GROUND_FAR : v);
          if (cls & 8u) first = min(first, ((u64)(uint32_t)(j - CELL_MIN) << 32) | (uint32_t)(i - CELL_MIN));
          if ((cls & 3u) == 1u) {
            lv_min = min(lv_min, c.x & 0xffffu);
            lv_max = max(lv_max, c.x & 0xffffu);
          }
        }
        n_cols += (uint32_t)__popcll(cm);
        n_lethal += (uint32_t)__popcll(__ballot(covered && (cls & 8u)));
        n_none += (uint32_t)__popcll(__ballot(covered && (cls & 3u) == 0u));
        n_ground += (uint32_t)__popcll(__ballot(covered && (cls & 3u) == 1u));
      }
  }
  lv_min = wave_min(lv_min), lv_max = wave_max(lv_max), min_d2 = wave_min(min_d2), first = wave_min64(first);
  if (lane == 0) {
    const int fu = n_lethal ? (int)(uint32_t)(first & 0xffffffffull) + CELL_MIN : 0, fv = n_lethal ? (int)(uint32_t)(first >> 32) + CELL_MIN : 0;
    uint2 *__restrict__ o = out + 5 * (size_t)p;
    o[0] = make_uint2(n_cols, n_lethal);
    o[1] = make_uint2(n_none, n_ground);
    o[2] = make_uint2(n_absent, (lv_min & 0xffffu) | ((n_ground ? lv_max : NO_LEVEL) << 16));
    o[3] = make_uint2(min_d2, (uint32_t)fu);
    o[4] = make_uint2((uint32_t)fv, 0u);
  }
}

// a length whose scan scratch holds `elems` words: the sort's histogram lies behind its scan's scratch, in the part of the
// layers' shared scratch that needs no initialising (sdm_internal.h)
size_t scan_length_for(size_t elems) { return std::max<size_t>(elems, 1032 + 513) * 2048 - (size_t)1032 * 2048; }

// the buffers for n_arch archived bricks / for `tiles` tiles (the stream is idle when either is called)
sdm_status grow_arch(sdm_map *m, size_t n_arch) {
  WorldGroundLayer &L = m->wground;
  const size_t cap = round_up(n_arch + 1, 256);
  return grow_buffers(m, n_arch + 1, cap, &L.cap_arch,
                      {buf(&L.flag, cap), buf(&L.rank, cap), buf(&L.keys, table_slots(cap)), buf(&L.vals, table_slots(cap))});
}

sdm_status grow_tiles(sdm_map *m, size_t tiles) {  // (no tile: still buffers to hand out)
  WorldGroundLayer &L = m->wground;
  const size_t need = std::max<size_t>(tiles, 1), cap = round_up(need, 256);
  return grow_buffers(m, need, cap, &L.cap_tiles,
                      {buf(&L.coord, cap), buf(&L.cells, cap * 64), buf(&L.d2, cap * 64), buf(&L.lethal, cap), buf(&L.sortbuf, cap * 4)});
}

Band band_of(const sdm_world_ground_options &o) {
  Band b{};
  b.a = o.up_axis, b.sign = o.up_sign;
  b.au = b.a == 0 ? 1 : 0, b.av = b.a == 2 ? 1 : 2;
  b.h_lo = o.h_lo;
  b.span = (int)((int64_t)o.h_hi - o.h_lo);
  b.clearance = (int)o.clearance, b.max_step = (int)o.max_step;
  b.rel_top = b.span + b.clearance;
  b.hb_lo = o.h_lo >> 3;
  b.lo_off = o.h_lo & 7;
  b.n_hb = (b.lo_off + b.rel_top) / 8 + 1;
  b.flags = o.flags;
  for (int k = 0; k < 8; ++k) b.labels[k] = o.support_labels[k];
  b.use_box = (o.flags & SDM_WORLD_GROUND_BOX) ? 1u : 0u;
  for (int k = 0; k < 2; ++k) b.tlo[k] = o.tmin[k], b.thi[k] = o.tmax[k];
  return b;
}

// the tiles in order, the columns, the costmap and the distances of a build of n tiles
hipError_t launch_wg_build(const sdm_map *m, const uint32_t *order, uint32_t n_arch, uint32_t n, const Band &b, int R, uint32_t *scratch) {
  const WorldGroundLayer &L = m->wground;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  hipError_t e;
  if ((e = hipMemsetAsync(L.meta, 0, G_WORDS * sizeof(u64), s)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  uint32_t *buf[4] = {L.sortbuf, L.sortbuf + L.cap_tiles, L.sortbuf + 2 * L.cap_tiles, L.sortbuf + 3 * L.cap_tiles};  // keys a, vals a, keys b, vals b
  LAYER_LAUNCH(k_wg_keys, (n_arch + QT - 1) / QT, QT, s, order, W.hdr, L.flag, L.rank, n_arch, n, b, buf[0], buf[1]);
  const int w = radix_sort_pairs(buf[0], buf[1], buf[2], buf[3], n, 32, scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t waves = (n + QT / 64 - 1) / (QT / 64);
  LAYER_LAUNCH(k_wg_tiles, (n + QT - 1) / QT, QT, s, buf[2 * w], n, L.keys, L.vals, L.hmask, L.coord);
  uint2 *cells = reinterpret_cast<uint2 *>(L.cells);
  if (b.a == 0)
    LAYER_LAUNCH(k_wg_columns<0>, waves, QT, s, L.coord, n, W.keys, W.vals, W.hmask, n_arch, W.cells, b, m->d.max_movable, cells);
  else if (b.a == 1)
    LAYER_LAUNCH(k_wg_columns<1>, waves, QT, s, L.coord, n, W.keys, W.vals, W.hmask, n_arch, W.cells, b, m->d.max_movable, cells);
  else
    LAYER_LAUNCH(k_wg_columns<2>, waves, QT, s, L.coord, n, W.keys, W.vals, W.hmask, n_arch, W.cells, b, m->d.max_movable, cells);
  LAYER_LAUNCH(k_wg_cost, waves, QT, s, L.coord, n, L.keys, L.vals, L.hmask, b, L.cells, L.lethal, L.meta);
  const u64 absent_reads = (b.flags & SDM_WORLD_GROUND_ABSENT_IS_LETHAL) ? ~0ull : 0ull;
  if (R <= 8)
    LAYER_LAUNCH(k_wg_dist<1>, n, DT, s, L.coord, L.keys, L.vals, L.hmask, n, L.lethal, R, absent_reads, L.d2);
  else
    LAYER_LAUNCH(k_wg_dist<2>, n, DT, s, L.coord, L.keys, L.vals, L.hmask, n, L.lethal, R, absent_reads, L.d2);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_GROUND = {"the world ground layer", "world ground layer", "sdm_world_ground_update", false};
}  // namespace

extern "C" {

sdm_status sdm_world_ground_update(sdm_map *m, const sdm_world_ground_options *o) {
  const char *what = "sdm_world_ground_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WG_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->up_axis < 0 || o->up_axis > 2 || (o->up_sign != 1 && o->up_sign != -1)) return LAYER_REFUSE(what, "up_axis not in 0..2 or up_sign not +1 / -1");
  if (o->h_lo > o->h_hi || (int64_t)o->h_hi - o->h_lo >= (int64_t)SDM_WORLD_GROUND_MAX_SPAN)
    return LAYER_REFUSE(what, "the band needs h_lo <= h_hi <= h_lo + 4095");
  if (o->clearance > 255u || o->max_step > 65535u) return LAYER_REFUSE(what, "clearance > 255 or max_step > 65535");
  if (o->radius < 1u || o->radius > (uint32_t)SDM_WORLD_GROUND_MAX_RADIUS) return LAYER_REFUSE(what, "radius 0 or > 16");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldGroundLayer &L = m->wground;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, G_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, G_WORDS + 1, true));
  const Band b = band_of(*o);
  uint32_t wmeta[M_WORDS];
  SDM_TRY(world_counters(m, wmeta));  // (waits: the last build, if any, has run)
  const uint32_t n_arch = wmeta[M_N_BRICKS];
  const uint32_t *order = nullptr;
  uint32_t *scan = nullptr;
  uint32_t n = 0;
  SDM_TRY(grow_arch(m, n_arch));
  L.hmask = table_slots(L.cap_arch) - 1;
  HIP_TRY(hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s));
  if (n_arch) {
    SDM_TRY(world_order(m, &order));
    SDM_TRY(layer_scan_scratch(m, std::max<size_t>((size_t)m->world.max_bricks + 1, scan_length_for(sort_scratch_elems(m->world.max_bricks))), &scan));
    hipLaunchKernelGGL(k_wg_claim, dim3(n_arch / QT + 1), dim3(QT), 0, s, order, m->world.hdr, n_arch, b, L.keys, L.hmask, L.flag);
    HIP_TRY(hipGetLastError());
    SDM_TRY(snapshot_rank(m, L.flag, L.rank, n_arch, scan, L.h_meta + G_WORDS, &n));
  }
  SDM_TRY(grow_tiles(m, n));
  L.n = n;
  HIP_TRY(launch_wg_build(m, order, n_arch, n, b, (int)o->radius, scan));
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, G_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));  // (the getter waits for them)
  L.opt = *o;
  L.stamp = m->world.f.gts;
  L.built(m->world.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_ground(sdm_map *m, int16_t *coords, sdm_ground_cell *cells, uint16_t *d2, int64_t first, int64_t cap, int64_t *n_out,
                                sdm_world_ground_info *info) {
  const char *what = "sdm_get_world_ground";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wground, WORLD_GROUND));
  HIP_TRY(hipSetDevice(m->device));
  const WorldGroundLayer &L = m->wground;
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>((int64_t)L.n - first, cap), 0);
  std::vector<uint32_t> keys(coords ? take : 0);
  if (take && coords) HIP_TRY(hipMemcpyAsync(keys.data(), L.coord + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (take && cells)
    HIP_TRY(hipMemcpyAsync(cells, L.cells + (size_t)first * 64, take * 64 * sizeof(sdm_ground_cell), hipMemcpyDeviceToHost, m->stream));
  if (take && d2) HIP_TRY(hipMemcpyAsync(d2, L.d2 + (size_t)first * 64, take * 64 * sizeof(uint16_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  unpack_tiles(keys, coords);
  *n_out = (int64_t)L.n;
  if (info) {
    const u64 *h = L.h_meta;  // (the stream has drained: the build's copy has landed)
    int64_t sum[5] = {0, 0, 0, 0, 0};
    u64 lo = 0, hi = 0;
    for (int k = 0; k < G_SPREAD; ++k) {
      for (int q = 0; q < 5; ++q) sum[q] += (int64_t)h[k * G_ROW + q];
      lo = std::max(lo, h[k * G_ROW + G_LMIN]);
      hi = std::max(hi, h[k * G_ROW + G_LMAX]);
    }
    info->n_tiles = L.n;
    info->level_min = hi ? (uint32_t)(0xffffu - lo) : NO_LEVEL;
    info->level_max = hi ? (uint32_t)(hi - 1) : NO_LEVEL;
    info->stamp = L.stamp;
    info->n_ground = sum[G_GROUND], info->n_obstacle = sum[G_OBSTACLE], info->n_none = sum[G_NONE];
    info->n_step = sum[G_STEP], info->n_lethal = sum[G_LETHAL];
    info->options = L.opt;
  }
  return SDM_OK;
}

sdm_status sdm_query_world_ground(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_ground_result *out, uint32_t flags) {
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, "sdm_query_world_ground", &sdm_map::wground, WORLD_GROUND));
  const WorldGroundLayer L = m->wground;
  const Band b = band_of(L.opt);
  const float recip = m->d.recip, voxel_size = m->d.voxel_size;
  const bool points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, 12, out, sizeof(sdm_world_ground_result), nullptr, 0, n, flags,
                   [L, b, recip, voxel_size, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_world_ground, dim3((c + QT - 1) / QT), dim3(QT), 0, s, points ? static_cast<const float *>(in) : nullptr,
                                        points ? nullptr : static_cast<const int32_t *>(in), c, recip, voxel_size, b, (int)L.opt.radius, L.keys, L.vals,
                                        L.hmask, L.n, reinterpret_cast<const uint2 *>(L.cells), L.d2, static_cast<uint2 *>(o));
                   });
}

sdm_status sdm_query_world_footprints(sdm_map *m, const sdm_footprint *fp, int64_t n, sdm_world_footprint_result *out, uint32_t flags) {
  const char *what = "sdm_query_world_footprints";
  SDM_TRY(query_check(m, fp, n, out, flags, SDM_QUERY_ON_DEVICE, what));
  SDM_TRY(layer_check(m, what, &m->wground, WORLD_GROUND));
  const WorldGroundLayer L = m->wground;
  const float recip = m->d.recip, voxel_size = m->d.voxel_size;
  return run_query(m, fp, sizeof(sdm_footprint), out, sizeof(sdm_world_footprint_result), nullptr, 0, n, flags,
                   [L, recip, voxel_size](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_world_footprints, dim3((c + QT / 64 - 1) / (QT / 64)), dim3(QT), 0, s,
                                        static_cast<const sdm_footprint *>(in), c, recip, voxel_size, L.keys, L.vals, L.hmask, L.n,
                                        reinterpret_cast<const uint2 *>(L.cells), L.d2, static_cast<uint2 *>(o));
                   });
}

}  // extern "C"
