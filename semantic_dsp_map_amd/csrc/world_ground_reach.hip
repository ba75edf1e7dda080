// world_ground_reach.hip — world ground reach: a 2-D travel-cost field over the costmap of the world ground layer - the
// cheapest way on the ground from a set of start columns to every traversable column the layer holds, the cost at a goal
// and the path itself, in world cells (gfx950; include/sdm.h, "world ground reach").
//
// A tile is the world ground layer's: 8 x 8 columns, one wave, a lane per column.  The build is a snapshot: it keeps the
// tiles' keys in the ground layer's order (their rank), a hash table of its own from tile key to rank, per tile the ranks
// of the eight tiles round it, the traversable word, the penalty word, 64 levels and 64 costs, and reads nothing of the
// ground layer afterwards.  cost[] is the fixed point of the relaxation, so it is the same whatever order the device
// relaxes in.
//   k_wgr_flag        a thread per tile of the ground layer: 1 if it lies in the box (or there is none).
//   snapshot_rank     (world_snapshot.hip) ranks the flags; the entry behind the last tile ends as the number of tiles.
//   k_wgr_index       a thread per ground tile: a tile of the field writes its key at its rank and inserts key -> rank
//               (a compare-and-swap on the key: every key by one thread).
//   k_wgr_neighbours  a thread per (tile, one of 8): one lookup, the rank or NONE; the range test before every lookup.
//   k_wgr_classify    a wave per ground tile, a lane per column: the cell's class byte and the stored distance give the
//               traversable and the penalty bit, two ballots write the tile's two words, the level leaves as a half-word
//               and 0xffffffff goes into the cost.
//   k_wgr_seed        a thread per start: cost 0 by atomicMin - the thread that lowers it counts the start - and the
//               activity bit of the tile and of its present neighbours.
//   launch_snapshot_list / k_wgr_relax   a round: the activity bits become a list (world_snapshot.hip's k_ws_list); ONE
//               WAVE per listed tile holds the tile's 64 costs in a register a lane, takes the 36 columns of the halo through the neighbour ranks (an absent tile reads
//               not traversable, 0xffffffff) into registers of the lanes on the tile's rim, works out each lane's allowed
//               moves once and sweeps - eight cross-lane reads of the neighbours' costs a sweep, no LDS, no barrier -
//               until a ballot says that nothing fell; it stores what it lowered and wakes every side and corner
//               neighbour whose halo holds a lowered column.  No kernel waits for another workgroup; the host issues
//               eight rounds between two looks at the count and caps them at 64 x n_tiles + 8.
//   k_wgr_reduce      traversable columns, reached columns, the largest cost.
//   k_query_world_ground_reach   a lane per goal: its column, one lookup, the ranks of the tiles round it, then the nine
//               costs, mask words and levels issued together; the result leaves in three 8-byte stores.
//   k_world_ground_reach_paths   a lane per goal, one descent step per two round trips to memory (ranks, then columns).
// The moves and the sweep share nothing with world_reach.hip or reach.hip (DESIGN.md 5r says why).
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_ground_reach_options) == 48 && sizeof(sdm_world_ground_reach_info) == 80 &&
                  sizeof(sdm_world_ground_reach_result) == 24,
              "sdm.h layout");
static_assert(offsetof(sdm_world_ground_reach_options, tmin) == 24 && offsetof(sdm_world_ground_reach_options, pad) == 40 &&
                  offsetof(sdm_world_ground_reach_info, options) == 32 && offsetof(sdm_world_ground_reach_result, col) == 8 &&
                  offsetof(sdm_world_ground_reach_result, level) == 16 && offsetof(sdm_world_ground_reach_result, next) == 18 &&
                  offsetof(sdm_world_ground_reach_result, status) == 19 && offsetof(sdm_world_ground_reach_result, pad) == 20,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;  // the kernels of a thread or a wave per item
constexpr int RT = 256;  // k_wgr_relax: four waves, a tile each; they share the workgroup only to fill the CU
constexpr uint32_t RR_GRID = 1024;
constexpr uint32_t NO_COST = 0xffffffffu, NO_LEVEL = 0xffffu;
constexpr uint32_t ALL_WGR_FLAGS = SDM_WORLD_GROUND_REACH_FACE_CONNECTED | SDM_WORLD_GROUND_REACH_BOX;
// the build's counters: the first four are sdm_world_ground_reach_info's; the rounds that had a tile to relax; the tiles
// relaxed in all rounds; the two counts of listed tiles, round r's in R_CNT + (r & 1)
enum { R_STARTS = 0, R_TRAV, R_REACHED, R_MAXCOST, R_ROUNDS, R_TILES, R_CNT, R_WORDS = 8 };

// cost, traversable word, penalty word, levels, neighbour ranks, key, two hash slots, list word
constexpr size_t TILE_BYTES = 64 * 4 + 8 + 8 + 64 * 2 + 8 * 4 + 4 + 2 * (8 + 4) + 4;
static_assert(TILE_BYTES == SDM_WORLD_GROUND_REACH_BYTES_PER_TILE, "sdm.h states the bytes");

struct TileBox {
  int lo[2], hi[2];
  uint32_t use;
};

// What the kernels know of the ground build the field stands on (by value): the up axis, its sign, the two plane axes in
// ascending order and the height that level 0 stands for.
struct Plane {
  int a, sign, au, av, h_lo;
};

// ---- moves: k = (dv + 1) * 3 + (du + 1), 4 is "no move" ------------------------------------------------------------------
constexpr int move_du(int k) { return k % 3 - 1; }
constexpr int move_dv(int k) { return k / 3 - 1; }
constexpr bool move_diagonal(int k) { return move_du(k) != 0 && move_dv(k) != 0; }
constexpr uint32_t move_weight(int k) { return move_diagonal(k) ? 14u : 10u; }
template <bool FACE>
constexpr bool move_used(int k) {
  return k != 4 && !(FACE && move_diagonal(k));
}
static_assert(move_weight(1) == 10 && move_weight(0) == 14 && move_du(5) == 1 && move_dv(7) == 1 && !move_used<true>(8) && move_used<false>(8), "moves");

// the tile offset (-1, 0, 1) of coordinate c in -1 .. 8 of the tile's own columns 0 .. 7
__device__ __forceinline__ int tile_off(int c) { return c < 0 ? -1 : c > 7 ? 1 : 0; }
// where tile r keeps the rank of its neighbour k (k != 4)
__device__ __forceinline__ size_t nbr_at(uint32_t r, int k) { return (size_t)r * 8u + (uint32_t)(k < 4 ? k : k - 1); }

// May a robot on a column of level l0 make move k?  tl[q]: the column at offset q of the 3 x 3 round it, level | traversable
// << 16; the column itself is traversable.  All 2 or 4 columns of the move traversable, their levels within max_climb.
template <int K>
__device__ __forceinline__ bool move_allowed(uint32_t l0, const uint32_t (&tl)[9], uint32_t max_climb) {
  const uint32_t t = tl[K];
  if (!move_diagonal(K)) return (t >> 16) && max(l0, t & 0xffffu) - min(l0, t & 0xffffu) <= max_climb;
  const uint32_t h = tl[4 + move_du(K)], v = tl[4 + 3 * move_dv(K)];
  const uint32_t hi = max(max(l0, t & 0xffffu), max(h & 0xffffu, v & 0xffffu)), lo = min(min(l0, t & 0xffffu), min(h & 0xffffu, v & 0xffffu));
  return (t >> 16) && (h >> 16) && (v >> 16) && hi - lo <= max_climb;
}

// ---- the index ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wgr_flag(const uint32_t *__restrict__ gcoord, uint32_t n_g, TileBox box, uint32_t *__restrict__ flag) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j > n_g) return;
  uint32_t in = 0u;
  if (j < n_g) {  // (the entry behind the last tile: the scan leaves the number of flags there)
    int bu, bv;
    tile_of(gcoord[j], bu, bv);
    in = !box.use || (bu >= box.lo[0] && bu <= box.hi[0] && bv >= box.lo[1] && bv <= box.hi[1]) ? 1u : 0u;
  }
  flag[j] = in;
}

__global__ __launch_bounds__(QT) void k_wgr_index(const uint32_t *__restrict__ gcoord, const uint32_t *__restrict__ flag,
                                                  const uint32_t *__restrict__ rank, uint32_t n_g, uint32_t n, uint32_t *__restrict__ coord,
                                                  u64 *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t hmask) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j >= n_g || !flag[j]) return;
  const uint32_t r = rank[j];
  if (r >= n) return;  // (never: the scan's total is n)
  const uint32_t key = gcoord[j];
  coord[r] = key;
  world_insert(keys, vals, hmask, (u64)key, r);
}

__global__ __launch_bounds__(QT) void k_wgr_neighbours(const uint32_t *__restrict__ coord, const u64 *__restrict__ keys,
                                                       const uint32_t *__restrict__ vals, uint32_t hmask, uint32_t n, uint32_t *__restrict__ nbr) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n * 8u) return;
  const uint32_t r = i >> 3, q = i & 7u, k = q < 4u ? q : q + 1u;
  int tu, tv;
  tile_of(coord[r], tu, tv);
  tu += (int)(k % 3u) - 1, tv += (int)(k / 3u) - 1;
  // (a coordinate of 32768 would alias another tile's key)
  const uint32_t found = tile_in_range(tu, tv) ? world_find(keys, vals, hmask, tile_key(tu, tv)) : NONE;
  nbr[i] = found < n ? found : NONE;
}

// ---- the classes -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wgr_classify(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n_g, uint32_t n,
                                                     const uint2 *__restrict__ gcells, const uint16_t *__restrict__ gd2, uint32_t min_d2,
                                                     uint32_t soft_d2, u64 *__restrict__ trav, u64 *__restrict__ pen,
                                                     uint16_t *__restrict__ level, uint32_t *__restrict__ cost) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (j >= n_g || !flag[j]) return;  // (wave-uniform)
  const uint32_t r = rank[j];
  if (r >= n) return;
  const uint2 c = gcells[(size_t)j * 64u + lane];
  const uint32_t v = gd2[(size_t)j * 64u + lane];
  const uint32_t cls = (c.y >> 8) & 0xffu;
  const bool tr = (cls & 3u) == 1u && !(cls & 8u) && (v == SDM_WORLD_GROUND_NONE || v >= min_d2);
  const u64 tm = __ballot(tr), pm = __ballot(v != SDM_WORLD_GROUND_NONE && v < soft_d2);
  if (lane == 0) {
    trav[r] = tm;
    pen[r] = pm;
  }
  level[(size_t)r * 64u + lane] = (uint16_t)(c.x & 0xffffu);
  cost[(size_t)r * 64u + lane] = NO_COST;
}

// ---- goals and starts --------------------------------------------------------------------------------------------------
// entry i (sdm_world.h's entry_cell: the rule of sdm_query_world_ground, all three coordinates) as a column (i_u, j_v):
// (0, 0) where the entry is not usable
__device__ __forceinline__ bool entry_column(const Plane &p, const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t i, float recip,
                                             int &iu, int &iv) {
  int g[3];
  const bool ok = entry_cell(xyz, cells, i, recip, g);
  // (the axes are picked by selects, not by indexing with a runtime value: the array stays in registers)
  iu = ok ? (p.au == 0 ? g[0] : g[1]) : 0;
  iv = ok ? (p.av == 1 ? g[1] : g[2]) : 0;
  return ok;
}

__global__ __launch_bounds__(QT) void k_wgr_seed(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n_starts, float recip,
                                                 Plane p, const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                 uint32_t n, const uint32_t *__restrict__ nbr, const u64 *__restrict__ trav,
                                                 uint32_t *__restrict__ cost, uint32_t *__restrict__ act, uint32_t *__restrict__ meta) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n_starts) return;
  int iu, iv;
  if (!entry_column(p, xyz, cells, i, recip, iu, iv)) return;
  const uint32_t r = world_find(keys, vals, hmask, tile_key(iu >> 3, iv >> 3));
  if (r >= n) return;
  const uint32_t w = (uint32_t)((iu & 7) | ((iv & 7) << 3));
  if (!((trav[r] >> w) & 1ull)) return;
  if (atomicMin(cost + (size_t)r * 64u + w, 0u) != 0u) atomicAdd(meta + R_STARTS, 1u);
  atomicOr(act + (r >> 5), 1u << (r & 31u));
  for (int k = 0; k < 9; ++k) {  // its neighbours: a start on a tile's rim is news for their halos
    if (k == 4) continue;
    const uint32_t nr = nbr[nbr_at(r, k)];
    if (nr != NONE) atomicOr(act + (nr >> 5), 1u << (nr & 31u));
  }
}

// ---- a round: the list of active tiles, then their relaxation --------------------------------------------------------
// One wave per listed tile; lane cu | cv << 3 holds column (cu, cv).  The costs of the tile live in `cur`, one a lane; a
// neighbour inside the tile is read across the lanes, one outside it from fix[], which only the lanes on the rim need and
// which does not change during the sweep: a neighbour tile's cost read here may be stale by this round's lowerings, but
// costs only fall, and whoever lowers a column of this tile's halo wakes this tile for the next round.
template <bool FACE>
__global__ __launch_bounds__(RT) void k_wgr_relax(uint32_t *__restrict__ cost, const u64 *__restrict__ trav, const u64 *__restrict__ pen,
                                                  const uint16_t *__restrict__ level, const uint32_t *__restrict__ nbr,
                                                  const uint32_t *__restrict__ list, uint32_t *__restrict__ act, uint32_t *__restrict__ meta,
                                                  uint32_t n, uint32_t penalty, uint32_t max_climb, uint32_t limit, uint32_t round) {
  const uint32_t count = min(meta[R_CNT + (round & 1u)], n);
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the next round's count: nobody reads or adds to it in this launch)
    meta[R_CNT + ((round + 1u) & 1u)] = 0u;
    if (count) {
      meta[R_ROUNDS] += 1u;
      meta[R_TILES] += count;
    }
  }
  const uint32_t *__restrict__ trav32 = reinterpret_cast<const uint32_t *>(trav);  // the same words as halves
  const uint32_t lane = threadIdx.x & 63u;
  const int cu = (int)(lane & 7u), cv = (int)(lane >> 3);
  for (uint32_t t = blockIdx.x * (RT / 64) + (threadIdx.x >> 6); t < count; t += gridDim.x * (RT / 64)) {  // (wave-uniform)
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[t]);
    if (b >= n) continue;  // (never)
    const u64 tw = trav[b];
    if (!tw) continue;  // nothing of this tile can be reached
    uint32_t nb[9];     // (uniform)
#pragma unroll
    for (int k = 0; k < 9; ++k) nb[k] = k == 4 ? b : nbr[nbr_at(b, k)];
    const uint32_t own = b * 64u + lane;  // (< 2^27: the field has at most 2^21 tiles)
    const uint32_t was = cost[own];
    const uint32_t my_t = (uint32_t)((tw >> lane) & 1ull), my_l = level[own];
    const uint32_t step_pen = ((pen[b] >> lane) & 1ull) ? penalty : 0u;
    // the 3 x 3 round the column, every load first and none of them conditional: a column of the tile itself is read like
    // one of the halo, a column of an absent tile reads a word of this tile that is thrown away
    uint32_t hc[9], hl[9], hw[9], out_m = 0u, gone_m = 0u;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      hc[k] = NO_COST, hl[k] = NO_LEVEL, hw[k] = 0u;
      if (!move_used<false>(k)) continue;  // (the corners too under FACE: no move reads them, the compiler drops them)
      const int x = cu + move_du(k), y = cv + move_dv(k), ox = tile_off(x), oy = tile_off(y);
      // the tile the column lies in: this one, the one across a side or the one across the corner
      const uint32_t nr = ox != 0 ? (oy != 0 ? nb[k] : nb[4 + move_du(k)]) : (oy != 0 ? nb[4 + 3 * move_dv(k)] : b);
      const uint32_t w = (uint32_t)((x & 7) | ((y & 7) << 3)), from = nr != NONE ? nr : b;
      out_m |= (ox != 0 || oy != 0 ? 1u : 0u) << k;
      gone_m |= (nr == NONE ? 1u : 0u) << k;
      hc[k] = cost[from * 64u + w];
      hl[k] = level[from * 64u + w];
      hw[k] = (trav32[from * 2u + (w >> 5)] >> (w & 31u)) & 1u;
    }
    uint32_t tl[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) tl[k] = (gone_m >> k) & 1u ? NO_LEVEL : hl[k] | (hw[k] << 16);  // (an absent tile: not traversable)
    // the moves this column may make: levels and masks do not change during a build
    uint32_t al = 0u;
    if (my_t) {
      if (move_used<FACE>(0) && move_allowed<0>(my_l, tl, max_climb)) al |= 1u << 0;
      if (move_used<FACE>(1) && move_allowed<1>(my_l, tl, max_climb)) al |= 1u << 1;
      if (move_used<FACE>(2) && move_allowed<2>(my_l, tl, max_climb)) al |= 1u << 2;
      if (move_used<FACE>(3) && move_allowed<3>(my_l, tl, max_climb)) al |= 1u << 3;
      if (move_used<FACE>(5) && move_allowed<5>(my_l, tl, max_climb)) al |= 1u << 5;
      if (move_used<FACE>(6) && move_allowed<6>(my_l, tl, max_climb)) al |= 1u << 6;
      if (move_used<FACE>(7) && move_allowed<7>(my_l, tl, max_climb)) al |= 1u << 7;
      if (move_used<FACE>(8) && move_allowed<8>(my_l, tl, max_climb)) al |= 1u << 8;
    }
    // per move, once: keep - all ones where the neighbour is a lane of this wave and the move is allowed; fix - NO_COST where
    // the move is not allowed, the halo's cost where the neighbour lies outside the tile, 0 otherwise.  A neighbour's cost
    // is then (cost across the lanes & keep) | fix: arithmetic, not a condition; NO_COST plus a weight saturates and stays
    // above the limit.
    uint32_t keep[9], fix[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const bool ok = (al >> k) & 1u, outside = (out_m >> k) & 1u;
      keep[k] = ok && !outside ? ~0u : 0u;
      fix[k] = !ok ? NO_COST : outside ? hc[k] : 0u;
    }
    // sweep until nothing falls: every lane reads its neighbours' costs of the sweep before, then all lower together
    uint32_t cur = was;
    bool fell;
    do {
      uint32_t best = cur;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        if (!move_used<FACE>(k)) continue;
        const uint32_t in = (uint32_t)__shfl((int)cur, (int)((lane + (uint32_t)(move_du(k) + 8 * move_dv(k))) & 63u), 64);
        const uint32_t via = __builtin_elementwise_add_sat((in & keep[k]) | fix[k], move_weight(k) + step_pen);
        best = min(best, via > limit ? NO_COST : via);
      }
      fell = best < cur;
      cur = best;
    } while (__ballot(fell) != 0ull);
    // what was lowered goes to memory, and to the neighbour tiles whose halo holds it goes the word to run
    const bool lowered = cur < was;
    if (lowered) cost[own] = cur;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      if (!move_used<FACE>(k)) continue;  // (face moves never read a corner of the halo)
      const bool seen = lowered && (move_du(k) < 0 ? cu == 0 : move_du(k) > 0 ? cu == 7 : true) &&
                        (move_dv(k) < 0 ? cv == 0 : move_dv(k) > 0 ? cv == 7 : true);
      if (__ballot(seen) != 0ull && lane == 0 && nb[k] != NONE) atomicOr(act + (nb[k] >> 5), 1u << (nb[k] & 31u));
    }
  }
}

// ---- the info block ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wgr_reduce(const uint32_t *__restrict__ cost, const u64 *__restrict__ trav, uint32_t n,
                                                   uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n_trav = 0, n_reached = 0, top = 0;
  for (uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6); r < n; r += gridDim.x * (QT / 64)) {  // (wave-uniform)
    const uint32_t v = cost[((size_t)r << 6) + lane];
    n_trav += (uint32_t)__popcll(trav[r]);
    n_reached += (uint32_t)__popcll(__ballot(v != NO_COST));
    if (v != NO_COST) top = max(top, v);
  }
  top = wave_max(top);
  if (lane == 0) {
    if (n_trav) atomicAdd(meta + R_TRAV, n_trav);
    if (n_reached) atomicAdd(meta + R_REACHED, n_reached);
    if (top) atomicMax(meta + R_MAXCOST, top);
  }
}

// ---- queries ----------------------------------------------------------------------------------------------------------
// the first descent step from column (cu, cv) of tile r, a traversable column of level l0 and cost `cost_c`: the smallest
// allowed move k with cost(c + o) + w(o) + pen(c) == cost_c, the neighbour's tile, cost and level; 255 if there is none.
// Two round trips: the ranks of the tiles the nine columns lie in, then their costs, mask words and levels, each issued
// together.  trav32: the traversable words as halves.
template <bool FACE>
__device__ __forceinline__ void descent_step(const uint32_t *__restrict__ cost, const uint32_t *__restrict__ trav32, const uint16_t *__restrict__ level,
                                             const uint32_t *__restrict__ nbr, uint32_t r, int cu, int cv, uint32_t l0, uint32_t cost_c,
                                             uint32_t step_pen, uint32_t max_climb, uint32_t &next, uint32_t &next_tile, uint32_t &next_cost,
                                             uint32_t &next_level) {
  uint32_t nr[9], cw[9], tw[9], lw[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    nr[k] = NONE;
    if (!move_used<false>(k)) continue;
    const int q = 4 + tile_off(cu + move_du(k)) + 3 * tile_off(cv + move_dv(k));
    nr[k] = q == 4 ? r : nbr[nbr_at(r, q)];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    cw[k] = NO_COST, tw[k] = 0u, lw[k] = NO_LEVEL;
    if (nr[k] != NONE) {  // (no tile: no cost, not traversable)
      const uint32_t w = (uint32_t)(((cu + move_du(k)) & 7) | (((cv + move_dv(k)) & 7) << 3));
      cw[k] = cost[(size_t)nr[k] * 64u + w];
      tw[k] = trav32[(size_t)nr[k] * 2u + (w >> 5)];
      lw[k] = level[(size_t)nr[k] * 64u + w];
    }
  }
  uint32_t tl[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const uint32_t w = (uint32_t)(((cu + move_du(k)) & 7) | (((cv + move_dv(k)) & 7) << 3));
    tl[k] = lw[k] | (((tw[k] >> (w & 31u)) & 1u) << 16);  // (no tile: the word is 0)
  }
  const bool ok[9] = {move_used<FACE>(0) && move_allowed<0>(l0, tl, max_climb), move_used<FACE>(1) && move_allowed<1>(l0, tl, max_climb),
                      move_used<FACE>(2) && move_allowed<2>(l0, tl, max_climb), move_used<FACE>(3) && move_allowed<3>(l0, tl, max_climb),
                      false,
                      move_used<FACE>(5) && move_allowed<5>(l0, tl, max_climb), move_used<FACE>(6) && move_allowed<6>(l0, tl, max_climb),
                      move_used<FACE>(7) && move_allowed<7>(l0, tl, max_climb), move_used<FACE>(8) && move_allowed<8>(l0, tl, max_climb)};
  next = 255u;
  next_tile = NONE;
  next_cost = NO_COST;
  next_level = NO_LEVEL;
#pragma unroll
  for (int k = 8; k >= 0; --k) {  // (descending, so the smallest k is the last to overwrite)
    if (!move_used<FACE>(k)) continue;
    // (the sum saturates at NO_COST, which no cost of a reached column is)
    if (ok[k] && cw[k] != NO_COST && __builtin_elementwise_add_sat(cw[k], move_weight(k) + step_pen) == cost_c) {
      next = (uint32_t)k;
      next_cost = cw[k];
      next_tile = nr[k];
      next_level = lw[k];
    }
  }
}

template <bool FACE>
__global__ __launch_bounds__(QT) void k_query_world_ground_reach(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n_goals,
                                                                 float recip, float voxel_size, Plane p, const u64 *__restrict__ keys,
                                                                 const uint32_t *__restrict__ vals, uint32_t hmask, uint32_t n,
                                                                 const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ trav32,
                                                                 const uint32_t *__restrict__ pen32, const uint16_t *__restrict__ level,
                                                                 const uint32_t *__restrict__ cost, uint32_t penalty, uint32_t max_climb,
                                                                 uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n_goals) return;
  int iu, iv;
  const bool ok = entry_column(p, xyz, cells, i, recip, iu, iv);
  const uint32_t r = ok ? world_find(keys, vals, hmask, tile_key(iu >> 3, iv >> 3)) : NONE;
  uint32_t c = NO_COST, next = 255u, status = 3u, lv = NO_LEVEL;
  if (r < n) {
    const int cu = iu & 7, cv = iv & 7;
    const uint32_t w = (uint32_t)(cu | (cv << 3));
    const uint32_t v = cost[(size_t)r * 64u + w];
    const bool tr = (trav32[(size_t)r * 2u + (w >> 5)] >> (w & 31u)) & 1u;
    lv = level[(size_t)r * 64u + w];
    status = !tr ? 2u : v == NO_COST ? 1u : 0u;
    if (status == 0u) {
      c = v;
      next = 4u;
      if (v != 0u) {
        const uint32_t step_pen = ((pen32[(size_t)r * 2u + (w >> 5)] >> (w & 31u)) & 1u) ? penalty : 0u;
        uint32_t nt, nc, nl;
        descent_step<FACE>(cost, trav32, level, nbr, r, cu, cv, lv, v, step_pen, max_climb, next, nt, nc, nl);
      }
    }
  }
  const float metres = c == NO_COST ? -1.f : (float)c * (voxel_size * 0.1f);
  uint2 *__restrict__ o = out + 3 * (size_t)i;
  o[0] = make_uint2(c, __float_as_uint(metres));
  o[1] = make_uint2((uint32_t)iu, (uint32_t)iv);
  o[2] = make_uint2(lv | (next << 16) | (status << 24), 0u);  // level, next, status; pad = 0
}

template <bool FACE>
__global__ __launch_bounds__(QT) void k_world_ground_reach_paths(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n_goals,
                                                                 float recip, Plane p, const u64 *__restrict__ keys,
                                                                 const uint32_t *__restrict__ vals, uint32_t hmask, uint32_t n,
                                                                 const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ trav32,
                                                                 const uint32_t *__restrict__ pen32, const uint16_t *__restrict__ level,
                                                                 const uint32_t *__restrict__ cost, uint32_t penalty, uint32_t max_climb,
                                                                 uint32_t max_len, size_t stride, int32_t *__restrict__ cells_out,
                                                                 int32_t *__restrict__ len_out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n_goals) return;
  int iu, iv;
  const bool ok = entry_column(p, xyz, cells, i, recip, iu, iv);
  uint32_t r = ok ? world_find(keys, vals, hmask, tile_key(iu >> 3, iv >> 3)) : NONE;
  uint32_t len = 0;
  if (r < n) {
    const uint32_t w0 = (uint32_t)((iu & 7) | ((iv & 7) << 3));
    uint32_t v = cost[(size_t)r * 64u + w0];  // (a column with a cost is traversable)
    uint32_t lv = level[(size_t)r * 64u + w0];
    if (v != NO_COST) {
      const uint32_t longest = v / 10u + 1u;  // every move weighs at least 10: the loop ends whatever the field holds
      int32_t *row = cells_out + (size_t)i * stride * 3u;
      for (;;) {
        if (len < max_len) {
          // the cell the robot's base stands in: the column on the plane, height h_lo + level + 1 on the up axis
          const int h = p.h_lo + (int)lv + 1, ga = p.sign > 0 ? h : -1 - h;
          row[3 * (size_t)len] = p.a == 0 ? ga : iu;
          row[3 * (size_t)len + 1] = p.a == 1 ? ga : (p.a == 0 ? iu : iv);
          row[3 * (size_t)len + 2] = p.a == 2 ? ga : iv;
        }
        ++len;
        if (v == 0u || len >= longest) break;
        const uint32_t w = (uint32_t)((iu & 7) | ((iv & 7) << 3));
        const uint32_t step_pen = ((pen32[(size_t)r * 2u + (w >> 5)] >> (w & 31u)) & 1u) ? penalty : 0u;
        uint32_t next, nt, nc, nl;
        descent_step<FACE>(cost, trav32, level, nbr, r, iu & 7, iv & 7, lv, v, step_pen, max_climb, next, nt, nc, nl);
        if (next == 255u) break;
        iu += (int)(next % 3u) - 1, iv += (int)(next / 3u) - 1;
        r = nt, v = nc, lv = nl;
      }
    }
  }
  len_out[i] = (int32_t)len;
}

constexpr uint32_t REACH_BATCH = 8;  // rounds issued between two looks at the count

// the buffers for `tiles` tiles (the stream is idle if there were buffers before)
sdm_status reach_alloc(sdm_map *m, size_t need) {  // (no tile: still a table to look up in)
  WorldGroundReachLayer &L = m->wgreach;
  need = std::max<size_t>(need, 1);
  const size_t tiles = round_up(need, 256), slots = table_slots(tiles);
  return grow_buffers(m, need, tiles, &L.cap,
                      {buf(&L.cost, tiles * 64), buf(&L.trav, tiles), buf(&L.pen, tiles), buf(&L.level, tiles * 64), buf(&L.nbr, tiles * 8),
                       buf(&L.coord, tiles), buf(&L.keys, slots), buf(&L.vals, slots), buf(&L.act, (tiles + 31) / 32), buf(&L.list, tiles)});
}

Plane plane_of(const sdm_world_ground_options &g) {
  Plane p{};
  p.a = g.up_axis, p.sign = g.up_sign;
  p.au = p.a == 0 ? 1 : 0, p.av = p.a == 2 ? 1 : 2;
  p.h_lo = g.h_lo;
  return p;
}

// the index, the neighbour ranks, the classes and the seeds of a build of n tiles out of the ground layer's n_g
hipError_t launch_prepare(const sdm_map *m, const sdm_world_ground_reach_options &o, const uint32_t *flag, const uint32_t *rank, uint32_t n_g,
                          uint32_t n, const float *d_xyz, const int32_t *d_cells, uint32_t n_starts) {
  const WorldGroundReachLayer &L = m->wgreach;
  const WorldGroundLayer &G = m->wground;
  hipStream_t s = m->stream;
  hipError_t e;
  if ((e = hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(L.meta, 0, R_WORDS * sizeof(uint32_t), s)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  if ((e = hipMemsetAsync(L.act, 0, (((size_t)n + 31) / 32) * sizeof(uint32_t), s)) != hipSuccess) return e;
  LAYER_LAUNCH(k_wgr_index, (n_g + QT - 1) / QT, QT, s, G.coord, flag, rank, n_g, n, L.coord, L.keys, L.vals, L.hmask);
  LAYER_LAUNCH(k_wgr_neighbours, (n * 8u + QT - 1) / QT, QT, s, L.coord, L.keys, L.vals, L.hmask, n, L.nbr);
  LAYER_LAUNCH(k_wgr_classify, (n_g + QT / 64 - 1) / (QT / 64), QT, s, flag, rank, n_g, n, reinterpret_cast<const uint2 *>(G.cells), G.d2, o.min_d2,
               o.soft_d2, L.trav, L.pen, L.level, L.cost);
  if (n_starts)
    LAYER_LAUNCH(k_wgr_seed, (n_starts + QT - 1) / QT, QT, s, d_xyz, d_cells, n_starts, m->d.recip, plane_of(G.opt), L.keys, L.vals, L.hmask, n, L.nbr,
                 L.trav, L.cost, L.act, L.meta);
  return hipSuccess;
}

hipError_t launch_round(const WorldGroundReachLayer &L, const sdm_world_ground_reach_options &o, uint32_t limit, uint32_t grid, uint32_t round,
                        hipStream_t s) {
  hipError_t e;
  if ((e = launch_snapshot_list(L.act, L.list, L.meta + R_CNT + (round & 1u), L.n, s)) != hipSuccess) return e;
  if (o.flags & SDM_WORLD_GROUND_REACH_FACE_CONNECTED)
    LAYER_LAUNCH(k_wgr_relax<true>, grid, RT, s, L.cost, L.trav, L.pen, L.level, L.nbr, L.list, L.act, L.meta, L.n, o.penalty, o.max_climb, limit,
                 round);
  else
    LAYER_LAUNCH(k_wgr_relax<false>, grid, RT, s, L.cost, L.trav, L.pen, L.level, L.nbr, L.list, L.act, L.meta, L.n, o.penalty, o.max_climb, limit,
                 round);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_GROUND = {"the world ground layer", "world ground layer", "sdm_world_ground_update", false};
constexpr LayerName WORLD_GROUND_REACH = {"world ground reach", "world ground reach field", "sdm_world_ground_reach_update", false};
}  // namespace

extern "C" {

sdm_status sdm_world_ground_reach_update(sdm_map *m, const sdm_world_ground_reach_options *o, const float *start_xyz, const int32_t *start_cells,
                                         int64_t n_starts) {
  const char *what = "sdm_world_ground_reach_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WGR_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->pad[0] != 0 || o->pad[1] != 0) return LAYER_REFUSE(what, "a non-zero pad");
  if (o->penalty > 65535u || o->max_climb > 65535u) return LAYER_REFUSE(what, "penalty > 65535 or max_climb > 65535");
  if (n_starts < 0 || n_starts > 0x7fffffff || (start_xyz != nullptr) == (start_cells != nullptr))
    return LAYER_REFUSE(what, "n_starts < 0 or >= 2^31, or not exactly one of start_xyz and start_cells");
  SDM_TRY(layer_check(m, what, &m->wground, WORLD_GROUND));
  const WorldGroundLayer &G = m->wground;
  const uint32_t d2_top = G.opt.radius * G.opt.radius + 1u;
  if (o->min_d2 > d2_top || o->soft_d2 > d2_top) return LAYER_REFUSE(what, "min_d2 or soft_d2 above R^2 + 1 of the ground build");
  HIP_TRY(hipSetDevice(m->device));
  WorldGroundReachLayer &L = m->wgreach;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, R_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, R_WORDS, true));
  TileBox box{};
  bool none = false;  // an empty box: a field of no tiles
  if (o->flags & SDM_WORLD_GROUND_REACH_BOX) {
    box.use = 1u;
    for (int a = 0; a < 2; ++a) {
      box.lo[a] = o->tmin[a], box.hi[a] = o->tmax[a];
      none = none || o->tmax[a] < o->tmin[a];
    }
  }
  // the tiles of the field: the ground layer's in its order, those of the box ranked
  const uint32_t n_g = none ? 0u : G.n;
  DevTemps tmp;
  uint32_t *flag = nullptr, *rank = nullptr;
  uint32_t n = 0;
  if (n_g) {
    uint32_t *scan = nullptr;
    SDM_TRY(layer_scan_scratch(m, std::max<size_t>(m->world.max_bricks, n_g) + 1, &scan));
    HIP_TRY(tmp.alloc(&flag, (size_t)n_g + 1));
    HIP_TRY(tmp.alloc(&rank, (size_t)n_g + 1));
    hipLaunchKernelGGL(k_wgr_flag, dim3(n_g / QT + 1), dim3(QT), 0, s, G.coord, n_g, box, flag);
    HIP_TRY(hipGetLastError());
    SDM_TRY(snapshot_rank(m, flag, rank, n_g, scan, L.h_meta, &n));
    n = std::min(n, n_g);
  }
  SDM_TRY(reach_alloc(m, n));
  L.n = n;
  L.hmask = table_slots(n) - 1;
  unsigned char *d_starts = nullptr;
  if (n_starts > 0) {
    HIP_TRY(tmp.alloc(&d_starts, (size_t)n_starts * 12));
    HIP_TRY(hipMemcpyAsync(d_starts, start_xyz ? (const void *)start_xyz : (const void *)start_cells, (size_t)n_starts * 12, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(launch_prepare(m, *o, flag, rank, n_g, n, start_xyz ? reinterpret_cast<const float *>(d_starts) : nullptr,
                         start_xyz ? nullptr : reinterpret_cast<const int32_t *>(d_starts), (uint32_t)n_starts));
  // rounds of plain launches; the count of the last round issued says whether anything is still moving
  const uint32_t limit = o->max_cost ? o->max_cost : NO_COST - 1u;
  if (n) {
    SDM_TRY(relax_rounds(
        m, what, REACH_BATCH, 64ull * n + REACH_BATCH, L.meta, L.h_meta, R_WORDS, L.h_meta + R_CNT,
        "the relaxation has not come to rest after 64 x n_tiles + 8 rounds",
        [n](uint32_t last) {  // (a wave a tile)
          return std::min<uint32_t>((n + RT / 64 - 1) / (RT / 64), std::max<uint32_t>((last + RT / 64 - 1) / (RT / 64), 64u));
        },
        [&](uint32_t grid, uint32_t round) { return launch_round(L, *o, limit, grid, round, s); }));
    hipLaunchKernelGGL(k_wgr_reduce, dim3(std::min<uint32_t>(RR_GRID, (n + QT / 64 - 1) / (QT / 64))), dim3(QT), 0, s, L.cost, L.trav, n, L.meta);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, R_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (the build's temporaries go when this returns)
  L.opt = *o;
  L.ground = G.opt;
  L.stamp = G.stamp;
  L.built(G.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_ground_reach(sdm_map *m, int16_t *coords, uint32_t *cost, int64_t first, int64_t cap, int64_t *n_out,
                                      sdm_world_ground_reach_info *info) {
  const char *what = "sdm_get_world_ground_reach";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wgreach, WORLD_GROUND_REACH));
  HIP_TRY(hipSetDevice(m->device));
  const WorldGroundReachLayer &L = m->wgreach;
  *n_out = (int64_t)L.n;
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>((int64_t)L.n - first, cap), 0);
  std::vector<uint32_t> keys(coords ? take : 0);
  if (take && coords) HIP_TRY(hipMemcpyAsync(keys.data(), L.coord + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (take && cost) HIP_TRY(hipMemcpyAsync(cost, L.cost + 64 * (size_t)first, 64 * take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  unpack_tiles(keys, coords);
  if (info) {
    const uint32_t *h = L.h_meta;  // (the build waited for them)
    info->n_tiles = L.n;
    info->n_starts_used = h[R_STARTS];
    info->n_traversable = h[R_TRAV];
    info->n_reached = h[R_REACHED];
    info->max_cost_reached = h[R_MAXCOST];
    info->rounds = h[R_ROUNDS];
    info->stamp = L.stamp;
    info->pad = 0;
    info->options = L.opt;
  }
  return SDM_OK;
}

sdm_status sdm_query_world_ground_reach(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_ground_reach_result *out,
                                        uint32_t flags) {
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, "sdm_query_world_ground_reach", &sdm_map::wgreach, WORLD_GROUND_REACH));
  const WorldGroundReachLayer L = m->wgreach;
  const Plane p = plane_of(L.ground);
  const float recip = m->d.recip, voxel_size = m->d.voxel_size;
  const bool face = (L.flags & SDM_WORLD_GROUND_REACH_FACE_CONNECTED) != 0, points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, 12, out, sizeof(sdm_world_ground_reach_result), nullptr, 0, n, flags,
                   [L, p, recip, voxel_size, face, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     const float *q = points ? static_cast<const float *>(in) : nullptr;
                     const int32_t *w = points ? nullptr : static_cast<const int32_t *>(in);
                     const uint32_t *trav32 = reinterpret_cast<const uint32_t *>(L.trav), *pen32 = reinterpret_cast<const uint32_t *>(L.pen);
                     const dim3 grid((c + QT - 1) / QT), tpb(QT);
                     if (face)
                       hipLaunchKernelGGL(k_query_world_ground_reach<true>, grid, tpb, 0, s, q, w, c, recip, voxel_size, p, L.keys, L.vals, L.hmask, L.n,
                                          L.nbr, trav32, pen32, L.level, L.cost, L.opt.penalty, L.opt.max_climb, static_cast<uint2 *>(o));
                     else
                       hipLaunchKernelGGL(k_query_world_ground_reach<false>, grid, tpb, 0, s, q, w, c, recip, voxel_size, p, L.keys, L.vals, L.hmask, L.n,
                                          L.nbr, trav32, pen32, L.level, L.cost, L.opt.penalty, L.opt.max_climb, static_cast<uint2 *>(o));
                   });
}

sdm_status sdm_world_ground_reach_paths(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, int32_t max_len, int32_t *cells_out,
                                        int32_t *len_out, uint32_t flags) {
  const char *what = "sdm_world_ground_reach_paths";
  SDM_TRY(goal_query_check(m, xyz, cells, n, len_out, flags, what, &sdm_map::wgreach, WORLD_GROUND_REACH));
  const WorldGroundReachLayer L = m->wgreach;
  const Plane p = plane_of(L.ground);
  const float recip = m->d.recip;
  const bool face = (L.flags & SDM_WORLD_GROUND_REACH_FACE_CONNECTED) != 0;
  return goal_paths(m, xyz, cells, n, max_len, cells_out, len_out, flags, what, (size_t)L.n * 64,
                    [&](const float *q, const int32_t *w, uint32_t c, uint32_t len_cap, size_t stride, int32_t *rows, int32_t *lens) {
                      const uint32_t *trav32 = reinterpret_cast<const uint32_t *>(L.trav), *pen32 = reinterpret_cast<const uint32_t *>(L.pen);
                      const dim3 grid((c + QT - 1) / QT), tpb(QT);
                      if (face)
                        hipLaunchKernelGGL(k_world_ground_reach_paths<true>, grid, tpb, 0, m->stream, q, w, c, recip, p, L.keys, L.vals, L.hmask, L.n, L.nbr,
                                           trav32, pen32, L.level, L.cost, L.opt.penalty, L.opt.max_climb, len_cap, stride, rows, lens);
                      else
                        hipLaunchKernelGGL(k_world_ground_reach_paths<false>, grid, tpb, 0, m->stream, q, w, c, recip, p, L.keys, L.vals, L.hmask, L.n, L.nbr,
                                           trav32, pen32, L.level, L.cost, L.opt.penalty, L.opt.max_climb, len_cap, stride, rows, lens);
                    });
}

sdm_status sdm_debug_world_ground_reach_tiles(sdm_map *m, int64_t *tiles_out) {
  if (!m || !tiles_out) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_debug_world_ground_reach_tiles", &m->wgreach, WORLD_GROUND_REACH));
  *tiles_out = (int64_t)m->wgreach.h_meta[R_TILES];
  return SDM_OK;
}

}  // extern "C"
