// world_reach.hip — world reach: the travel-cost field of reach.hip over the bricks of the world archive instead of the
// map block - the cheapest path from a set of start cells to every traversable cell the archive remembers, the cost at
// a goal and the path itself, in world cells (gfx950; include/sdm.h, "world reach").
//
// A tile of reach.hip becomes a brick of 8 x 8 x 8 cells, "the neighbour tile" becomes "the brick a table names".  The
// build is a snapshot: it keeps the bricks' coordinates in brick order (their rank), a hash table of its own from key to
// rank, per brick the ranks of the 27 bricks round it, the traversable (and obstacle) masks and the costs, and reads
// nothing of the archive afterwards - no pool slot outlives the build.  cost[] is the fixed point of reach.hip's
// relaxation, so it is the same whatever order the device relaxes in.
//   snapshot_bricks, launch_snapshot_index   world_snapshot.hip's: the bricks of the box flagged and ranked, their
//               coordinates and pool slots (a temporary of the build) at their rank, key -> rank in the field's own table.
//   launch_snapshot_neighbours   world_snapshot.hip's k_ws_neighbours: a thread per (brick, one of 27): one lookup, the rank
//               or NONE; brick_in_range before every lookup.
//   k_wr_classify    a wave per brick, a lane per (cx, cy), the eight layers' loads first: ballots write the traversable
//               and the obstacle mask, 8 x 64 bits each, and 0xffffffff goes into the 512 costs.
//   k_wr_inflate     (inflate > 0) a thread per (brick, layer): clears from the traversable word the dilation of the
//               obstacle words of the layers and bricks round it - shifts inside a 64-bit word for x and y, the word
//               index for z, the neighbour ranks for the bricks.  It reads obstacle words and writes traversable ones.
//   k_wr_seed        a thread per start: cost 0 by atomicMin - the thread that lowers it counts the start - and the
//               activity bit of the brick and of its present neighbours.
//   launch_snapshot_list / k_wr_relax   a round, exactly reach.hip's: the activity bits become a list (world_snapshot.hip's
//               k_ws_list), a workgroup per listed brick loads 10^3 costs and traversable bits through the neighbour ranks (an absent brick reads not traversable,
//               0xffffffff), relaxes in LDS until a sweep lowers nothing, stores what it lowered and wakes every face,
//               edge and corner neighbour whose halo holds a lowered cell.  No kernel waits for another workgroup; the
//               host issues eight rounds between two looks at the count and caps them at 512 x n_bricks.
//   k_wr_reduce      traversable cells, reached cells, the largest cost.
//   k_query_world_reach   a lane per goal: its cell, one lookup, then the ranks and the 27 costs and traversable words
//               round the goal issued together; the result leaves in three 8-byte stores.
//   k_world_reach_paths   a lane per goal, one descent step per two round trips to memory (ranks, then costs).
// The move masks and the sweep are this unit's own copy of reach.hip's (DESIGN.md 5m says why); the 27 offsets and the face
// moves under them are sdm_world.h's, the world layers' one table (5w).
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_reach_options) == 40 && sizeof(sdm_world_reach_info) == 40 && sizeof(sdm_world_reach_result) == 24, "sdm.h layout");
static_assert(offsetof(sdm_world_reach_options, bmin) == 16 && offsetof(sdm_world_reach_result, cell) == 8 &&
                  offsetof(sdm_world_reach_result, next) == 20 && offsetof(sdm_world_reach_result, pad) == 22,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;                               // the kernels of a thread or a wave per item
constexpr int RT = 256;                               // k_wr_relax: two cells of the brick and four of the region a thread
constexpr int RX = 10, RXY = RX * RX, RC = RXY * RX;  // the brick and its one-cell halo
constexpr int KR = (RC + RT - 1) / RT, KT = 512 / RT;
constexpr uint32_t RR_GRID = 1024;
constexpr uint32_t NO_COST = 0xffffffffu;
constexpr uint32_t ALL_REACH_FLAGS =
    SDM_WORLD_REACH_FACE_CONNECTED | SDM_WORLD_REACH_THROUGH_UNKNOWN | SDM_WORLD_REACH_IGNORE_MOVABLE | SDM_WORLD_REACH_BOX;
// the build's counters: the first four are sdm_world_reach_info's; the bricks relaxed in all rounds; the two counts of
// listed bricks, round r's in R_CNT + (r & 1)
enum { R_STARTS = 0, R_TRAV, R_REACHED, R_MAXCOST, R_ROUNDS, R_BRICKS, R_CNT, R_WORDS = 8 };

// ---- moves (reach.hip's; move n goes by off_d(n, .), the face moves are FACE_MOVES: sdm_world.h) -----------------------
constexpr uint32_t move_weight(int n) {
  const int k = (off_d(n, 0) != 0) + (off_d(n, 1) != 0) + (off_d(n, 2) != 0);
  return k == 1 ? 10u : k == 2 ? 14u : 17u;
}
constexpr uint32_t move_needs(int n) {
  uint32_t m = 0;
  for (int k = 0; k < 8; ++k) {
    const int sx = (k & 1) ? off_d(n, 0) : 0, sy = (k & 2) ? off_d(n, 1) : 0, sz = (k & 4) ? off_d(n, 2) : 0;
    m |= 1u << ((sz + 1) * 9 + (sy + 1) * 3 + (sx + 1));
  }
  return m;
}
static_assert(move_weight(12) == 10 && move_weight(0) == 17 && move_weight(1) == 14 && move_needs(14) == ((1u << 13) | (1u << 14)), "moves");

template <bool FACE>
__device__ __forceinline__ uint32_t allowed_moves(uint32_t nb) {
  uint32_t al = 0;
#pragma unroll
  for (int n = 0; n < 27; ++n) {
    if (n == 13 || (FACE && !((FACE_MOVES >> n) & 1u))) continue;
    if ((nb & move_needs(n)) == move_needs(n)) al |= 1u << n;
  }
  return al;
}

// cell (cx, cy, cz) of a brick: its cost word, and its bit in the halves of the traversable mask
__device__ __forceinline__ uint32_t cost_at(uint32_t r, int cx, int cy, int cz) { return r * 512u + (uint32_t)(cz * 64 + cy * 8 + cx); }
__device__ __forceinline__ uint32_t trav_word(uint32_t r, int cy, int cz) { return (r * 8u + (uint32_t)cz) * 2u + (uint32_t)(cy >> 2); }
__device__ __forceinline__ uint32_t trav_bit(int cx, int cy) { return (uint32_t)((cy & 3) * 8 + cx); }

// ---- the classes -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wr_classify(const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ cells, uint32_t n,
                                                    uint32_t through_unknown, uint32_t ignore_movable, int max_movable, u64 *__restrict__ trav,
                                                    u64 *__restrict__ obst, uint32_t *__restrict__ cost) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform)
  uint32_t w[8];
  load_brick(cells, slot_of[r], lane, w);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    int occ = occ_of(w[l]);
    const uint32_t track = w[l] & 0xffffu;
    if (ignore_movable && occ >= 1 && track >= 1u && (int)track <= max_movable) occ = 0;
    const u64 tm = __ballot(occ == 0 || (through_unknown && occ == -1)), om = __ballot(occ >= 1);
    if (lane == 0) {
      trav[(size_t)r * 8u + l] = tm;
      obst[(size_t)r * 8u + l] = om;
    }
    cost[(size_t)r * 512u + (uint32_t)l * 64u + lane] = NO_COST;
  }
}

// 64-bit layer words: bit cx + 8 cy.  The columns cx < t / cx >= 8 - t of every row:
__device__ __forceinline__ u64 cols_below(int t) { return 0x0101010101010101ull * ((1ull << t) - 1ull); }
__device__ __forceinline__ u64 cols_from(int t) { return 0x0101010101010101ull * (0xffull & ~((1ull << t) - 1ull)); }
// the cells of the middle word within R cells in x of an obstacle of the words left of it, itself and right of it
template <int R>
__device__ __forceinline__ u64 dilate_x(u64 left, u64 mid, u64 right) {
  u64 o = mid;
#pragma unroll
  for (int t = 1; t <= R; ++t) {
    o |= ((mid << t) & ~cols_below(t)) | ((mid >> t) & ~cols_from(8 - t));
    o |= ((left >> (8 - t)) & cols_below(t)) | ((right << (8 - t)) & cols_from(8 - t));
  }
  return o;
}

template <int R>
__global__ __launch_bounds__(QT) void k_wr_inflate(const uint32_t *__restrict__ nbr, const u64 *__restrict__ obst, u64 *__restrict__ trav,
                                                   uint32_t n) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n * 8u) return;
  const uint32_t r = i >> 3;
  const int z = (int)(i & 7u);
  u64 near = 0ull;
#pragma unroll
  for (int dz = -R; dz <= R; ++dz) {
    const int zz = z + dz, oz = brick_off(zz), lz = zz & 7;
    u64 row[3];
#pragma unroll
    for (int oy = -1; oy <= 1; ++oy) {
      const uint32_t *__restrict__ k = nbr + (size_t)r * 27u + (uint32_t)(13 + 9 * oz + 3 * oy);
      const uint32_t a = k[-1], b = k[0], c = k[1];
      const u64 wa = a != NONE ? obst[(size_t)a * 8u + lz] : 0ull, wb = b != NONE ? obst[(size_t)b * 8u + lz] : 0ull,
                wc = c != NONE ? obst[(size_t)c * 8u + lz] : 0ull;
      row[oy + 1] = dilate_x<R>(wa, wb, wc);
    }
    u64 o = row[1];
#pragma unroll
    for (int t = 1; t <= R; ++t) o |= (row[1] << (8 * t)) | (row[1] >> (8 * t)) | (row[0] >> (64 - 8 * t)) | (row[2] << (64 - 8 * t));
    near |= o;
  }
  trav[i] &= ~near;
}

// ---- goals and starts --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wr_seed(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n_starts, float recip,
                                                const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ trav, uint32_t *__restrict__ cost,
                                                uint32_t *__restrict__ act, uint32_t *__restrict__ meta) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n_starts) return;
  int g[3];
  if (!entry_cell(xyz, cells, i, recip, g)) return;
  const uint32_t r = world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3));
  if (r == NONE) return;
  const int cx = g[0] & 7, cy = g[1] & 7, cz = g[2] & 7;
  if (!((trav[trav_word(r, cy, cz)] >> trav_bit(cx, cy)) & 1u)) return;
  if (atomicMin(cost + cost_at(r, cx, cy, cz), 0u) != 0u) atomicAdd(meta + R_STARTS, 1u);
  for (int k = 0; k < 27; ++k) {  // the brick and its neighbours: a start on a brick's border is news for their halos
    const uint32_t nr = nbr[(size_t)r * 27u + k];
    if (nr != NONE) atomicOr(act + (nr >> 5), 1u << (nr & 31u));
  }
}

// ---- a round: the list of active bricks, then their relaxation -------------------------------------------------------
template <bool FACE>
__global__ __launch_bounds__(RT) void k_wr_relax(uint32_t *__restrict__ cost, const uint32_t *__restrict__ trav, const uint32_t *__restrict__ nbr,
                                                 const uint32_t *__restrict__ list, uint32_t *__restrict__ act, uint32_t *__restrict__ meta,
                                                 uint32_t limit, uint32_t round) {
  __shared__ uint32_t s_cost[RC];
  __shared__ uint8_t s_trav[RC];
  __shared__ uint32_t s_nbr[27];
  __shared__ uint32_t s_wake;
  const uint32_t count = meta[R_CNT + (round & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the next round's count: nobody reads or adds to it in this launch)
    meta[R_CNT + ((round + 1u) & 1u)] = 0u;
    if (count) {
      meta[R_ROUNDS] += 1u;
      meta[R_BRICKS] += count;
    }
  }
  const int tid = (int)threadIdx.x;
  for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {  // (count is the same for every thread: the barriers are whole)
    const uint32_t b = list[t];
    if (tid < 27) s_nbr[tid] = nbr[(size_t)b * 27u + tid];
    if (tid == 0) s_wake = 0u;
    __syncthreads();
    // the brick and its halo through the neighbour ranks: every load first
    uint32_t lc[KR], lw[KR], ls[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = tid + k * RT;
      lc[k] = NO_COST;
      lw[k] = 0u;
      ls[k] = 0u;
      if (i < RC) {
        const int rx = i % RX - 1, q = i / RX, ry = q % RX - 1, rz = q / RX - 1;
        const uint32_t nr = s_nbr[13 + brick_off(rx) + 3 * brick_off(ry) + 9 * brick_off(rz)];
        if (nr != NONE) {  // (an absent brick: not traversable, no cost)
          const int cx = rx & 7, cy = ry & 7, cz = rz & 7;
          lc[k] = cost[cost_at(nr, cx, cy, cz)];
          lw[k] = trav[trav_word(nr, cy, cz)];
          ls[k] = trav_bit(cx, cy);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = tid + k * RT;
      if (i < RC) {
        s_cost[i] = lc[k];
        s_trav[i] = (uint8_t)((lw[k] >> ls[k]) & 1u);
      }
    }
    __syncthreads();
    int ri[KT];
    uint32_t al[KT], cur[KT], was[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int i = tid + k * RT;
      ri[k] = ((i & 7) + 1) + (((i >> 3) & 7) + 1) * RX + ((i >> 6) + 1) * RXY;
      uint32_t nb = 0u;
#pragma unroll
      for (int n = 0; n < 27; ++n) nb |= (uint32_t)s_trav[ri[k] + off_d(n, 0) + off_d(n, 1) * RX + off_d(n, 2) * RXY] << n;
      al[k] = allowed_moves<FACE>(nb);
      cur[k] = was[k] = s_cost[ri[k]];
    }
    // relax until a whole sweep lowers nothing (a cell read while its owner lowers it gives the old or the new value:
    // both are real path weights, and the sweep that ends the loop has read values that nobody wrote)
    bool changed;
    do {
      changed = false;
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        uint32_t best = cur[k];
#pragma unroll
        for (int n = 0; n < 27; ++n) {
          if (n == 13 || (FACE && !((FACE_MOVES >> n) & 1u))) continue;
          // arithmetic, not a condition: a move that is not allowed makes its neighbour NO_COST, and NO_COST plus a
          // weight saturates and stays above the limit
          const uint32_t v = s_cost[ri[k] + off_d(n, 0) + off_d(n, 1) * RX + off_d(n, 2) * RXY] | (((al[k] >> n) & 1u) - 1u);
          const uint32_t via = __builtin_elementwise_add_sat(v, move_weight(n));
          best = min(best, via > limit ? NO_COST : via);
        }
        if (best < cur[k]) {
          cur[k] = best;
          s_cost[ri[k]] = best;
          changed = true;
        }
      }
    } while (__syncthreads_or(changed));
    // what was lowered goes to memory, and to the neighbour bricks whose halo holds it goes the word to run
    uint32_t wake = 0u;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (cur[k] < was[k]) {
        const int i = tid + k * RT;
        const int lx = i & 7, ly = (i >> 3) & 7, lz = i >> 6;
        cost[b * 512u + (uint32_t)i] = cur[k];
        const uint32_t ax = 2u | (lx == 0 ? 1u : 0u) | (lx == 7 ? 4u : 0u);  // bit d + 1: the brick at offset d sees the cell
        const uint32_t ay = 2u | (ly == 0 ? 1u : 0u) | (ly == 7 ? 4u : 0u);
        const uint32_t az = 2u | (lz == 0 ? 1u : 0u) | (lz == 7 ? 4u : 0u);
#pragma unroll
        for (int n = 0; n < 27; ++n) {
          if (n == 13 || (FACE && !((FACE_MOVES >> n) & 1u))) continue;  // (face moves never read an edge or corner halo)
          wake |= ((ax >> (off_d(n, 0) + 1)) & (ay >> (off_d(n, 1) + 1)) & (az >> (off_d(n, 2) + 1)) & 1u) << n;
        }
      }
    }
    if (wake) atomicOr(&s_wake, wake);
    __syncthreads();
    if (tid < 27 && ((s_wake >> tid) & 1u)) {
      const uint32_t nr = s_nbr[tid];
      if (nr != NONE) atomicOr(act + (nr >> 5), 1u << (nr & 31u));
    }
    __syncthreads();  // (s_wake, s_nbr and the region are the next brick's from here on)
  }
}

// ---- the info block ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wr_reduce(const uint32_t *__restrict__ cost, const u64 *__restrict__ trav, uint32_t nw,
                                                  uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n_trav = 0, n_reached = 0, top = 0;
  for (uint32_t chunk = blockIdx.x * (QT / 64) + (threadIdx.x >> 6); chunk < nw; chunk += gridDim.x * (QT / 64)) {  // (wave-uniform)
    const uint32_t v = cost[((size_t)chunk << 6) + lane];
    n_trav += (uint32_t)__popcll(trav[chunk]);
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
// the first descent step from cell (lx, ly, lz) of brick b with cost `cost_c`: the smallest allowed move n with
// cost(c + o) + w(o) == cost_c, the neighbour's brick and cost; 255 if there is none.  Two round trips: the ranks of the
// bricks the 27 cells lie in, then their costs and mask words, each issued together.
template <bool FACE>
__device__ __forceinline__ void descent_step(const uint32_t *__restrict__ cost, const uint32_t *__restrict__ trav, const uint32_t *__restrict__ nbr,
                                             uint32_t b, int lx, int ly, int lz, uint32_t cost_c, uint32_t &next, uint32_t &next_brick,
                                             uint32_t &next_cost) {
  uint32_t nr[27], cw[27], tw[27];
#pragma unroll
  for (int n = 0; n < 27; ++n) {
    nr[n] = NONE;
    if (FACE && n != 13 && !((FACE_MOVES >> n) & 1u)) continue;
    const int x = lx + off_d(n, 0), y = ly + off_d(n, 1), z = lz + off_d(n, 2);
    nr[n] = nbr[(size_t)b * 27u + (uint32_t)(13 + brick_off(x) + 3 * brick_off(y) + 9 * brick_off(z))];
  }
#pragma unroll
  for (int n = 0; n < 27; ++n) {
    cw[n] = NO_COST;
    tw[n] = 0u;
    if (nr[n] != NONE) {  // (no brick: no cost, not traversable)
      const int cx = (lx + off_d(n, 0)) & 7, cy = (ly + off_d(n, 1)) & 7, cz = (lz + off_d(n, 2)) & 7;
      cw[n] = cost[cost_at(nr[n], cx, cy, cz)];
      tw[n] = trav[trav_word(nr[n], cy, cz)];
    }
  }
  uint32_t nb = 0u;
#pragma unroll
  for (int n = 0; n < 27; ++n) nb |= ((tw[n] >> trav_bit((lx + off_d(n, 0)) & 7, (ly + off_d(n, 1)) & 7)) & 1u) << n;  // (no brick: the word is 0)
  const uint32_t al = allowed_moves<FACE>(nb);
  next = 255u;
  next_brick = NONE;
  next_cost = NO_COST;
#pragma unroll
  for (int n = 26; n >= 0; --n) {  // (descending, so the smallest n is the last to overwrite)
    if (n == 13 || (FACE && !((FACE_MOVES >> n) & 1u))) continue;
    if (((al >> n) & 1u) && cw[n] != NO_COST && cw[n] + move_weight(n) == cost_c) {
      next = (uint32_t)n;
      next_cost = cw[n];
      next_brick = nr[n];
    }
  }
}

template <bool FACE>
__global__ __launch_bounds__(QT) void k_query_world_reach(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n, float recip,
                                                          float voxel_size, const u64 *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                          uint32_t hmask, const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ trav,
                                                          const uint32_t *__restrict__ cost, uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n) return;
  int g[3];
  const bool ok = entry_cell(xyz, cells, i, recip, g);
  const uint32_t b = ok ? world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3)) : NONE;
  uint32_t c = NO_COST, next = 255u, status = 3u;
  if (b != NONE) {
    const int lx = g[0] & 7, ly = g[1] & 7, lz = g[2] & 7;
    const uint32_t v = cost[cost_at(b, lx, ly, lz)];
    const bool tr = (trav[trav_word(b, ly, lz)] >> trav_bit(lx, ly)) & 1u;
    status = !tr ? 2u : v == NO_COST ? 1u : 0u;
    if (status == 0u) {
      c = v;
      next = 13u;
      if (v != 0u) {
        uint32_t nb, nv;
        descent_step<FACE>(cost, trav, nbr, b, lx, ly, lz, v, next, nb, nv);
      }
    }
  }
  const float metres = c == NO_COST ? -1.f : (float)c * (voxel_size * 0.1f);
  uint2 *__restrict__ o = out + 3 * (size_t)i;
  o[0] = make_uint2(c, __float_as_uint(metres));
  o[1] = make_uint2((uint32_t)g[0], (uint32_t)g[1]);
  o[2] = make_uint2((uint32_t)g[2], next | (status << 8));  // next, status, pad = 0
}

template <bool FACE>
__global__ __launch_bounds__(QT) void k_world_reach_paths(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n, float recip,
                                                          const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                          const uint32_t *__restrict__ nbr, const uint32_t *__restrict__ trav,
                                                          const uint32_t *__restrict__ cost, uint32_t max_len, size_t stride,
                                                          int32_t *__restrict__ cells_out, int32_t *__restrict__ len_out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n) return;
  int g[3];
  const bool ok = entry_cell(xyz, cells, i, recip, g);
  uint32_t b = ok ? world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3)) : NONE;
  uint32_t len = 0;
  if (b != NONE) {
    uint32_t v = cost[cost_at(b, g[0] & 7, g[1] & 7, g[2] & 7)];  // (a cell with a cost is traversable)
    if (v != NO_COST) {
      const uint32_t longest = v / 10u + 1u;  // every move weighs at least 10: the loop ends whatever the field holds
      int32_t *row = cells_out + (size_t)i * stride * 3u;
      for (;;) {
        if (len < max_len) {
          row[3 * (size_t)len] = g[0];
          row[3 * (size_t)len + 1] = g[1];
          row[3 * (size_t)len + 2] = g[2];
        }
        ++len;
        if (v == 0u || len >= longest) break;
        uint32_t next, nb, nv;
        descent_step<FACE>(cost, trav, nbr, b, g[0] & 7, g[1] & 7, g[2] & 7, v, next, nb, nv);
        if (next == 255u) break;
        g[0] += (int)(next % 3u) - 1, g[1] += (int)((next / 3u) % 3u) - 1, g[2] += (int)(next / 9u) - 1;
        b = nb;
        v = nv;
      }
    }
  }
  len_out[i] = (int32_t)len;
}

constexpr uint32_t REACH_BATCH = 8;  // rounds issued between two looks at the count

// the buffers for `bricks` bricks (the stream is idle if there were buffers before)
sdm_status reach_alloc(sdm_map *m, size_t need) {  // (no brick: still a table to look up in)
  WorldReachLayer &L = m->wreach;
  need = std::max<size_t>(need, 1);
  const size_t bricks = round_up(need, 256), slots = table_slots(bricks);
  return grow_buffers(m, need, bricks, &L.cap,
                      {buf(&L.cost, bricks * 512), buf(&L.trav, bricks * 8), buf(&L.obst, bricks * 8), buf(&L.nbr, bricks * 27), buf(&L.coord, bricks * 2),
                       buf(&L.keys, slots), buf(&L.vals, slots), buf(&L.act, (bricks + 31) / 32), buf(&L.list, bricks)});
}

// the index, the neighbour ranks, the classes and the seeds of a build of n bricks
hipError_t launch_reach_prepare(const sdm_map *m, const sdm_world_reach_options &o, const uint32_t *order, const uint32_t *flag,
                                const uint32_t *rank, uint32_t *slot_of, uint32_t n_arch, uint32_t n, const float *d_xyz, const int32_t *d_cells,
                                uint32_t n_starts) {
  const WorldReachLayer &L = m->wreach;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  hipError_t e;
  if ((e = hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(L.meta, 0, R_WORDS * sizeof(uint32_t), s)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  if ((e = hipMemsetAsync(L.act, 0, (((size_t)n + 31) / 32) * sizeof(uint32_t), s)) != hipSuccess) return e;
  if ((e = launch_snapshot_index(m, order, flag, rank, n_arch, n, L.coord, slot_of, L.keys, L.vals, L.hmask)) != hipSuccess) return e;
  if ((e = launch_snapshot_neighbours(L.coord, L.keys, L.vals, L.hmask, n, L.nbr, s)) != hipSuccess) return e;
  LAYER_LAUNCH(k_wr_classify, (n + QT / 64 - 1) / (QT / 64), QT, s, slot_of, W.cells, n, (o.flags & SDM_WORLD_REACH_THROUGH_UNKNOWN) ? 1u : 0u,
               (o.flags & SDM_WORLD_REACH_IGNORE_MOVABLE) ? 1u : 0u, m->d.max_movable, L.trav, L.obst, L.cost);
  if (o.inflate == 1) LAYER_LAUNCH(k_wr_inflate<1>, (n * 8u + QT - 1) / QT, QT, s, L.nbr, L.obst, L.trav, n);
  if (o.inflate == 2) LAYER_LAUNCH(k_wr_inflate<2>, (n * 8u + QT - 1) / QT, QT, s, L.nbr, L.obst, L.trav, n);
  if (n_starts)
    LAYER_LAUNCH(k_wr_seed, (n_starts + QT - 1) / QT, QT, s, d_xyz, d_cells, n_starts, m->d.recip, L.keys, L.vals, L.hmask, L.nbr,
                 reinterpret_cast<const uint32_t *>(L.trav), L.cost, L.act, L.meta);
  return hipSuccess;
}

hipError_t launch_reach_round(const WorldReachLayer &L, bool face, uint32_t limit, uint32_t grid, uint32_t round, hipStream_t s) {
  hipError_t e;
  if ((e = launch_snapshot_list(L.act, L.list, L.meta + R_CNT + (round & 1u), L.n, s)) != hipSuccess) return e;
  const uint32_t *trav = reinterpret_cast<const uint32_t *>(L.trav);
  if (face)
    LAYER_LAUNCH(k_wr_relax<true>, grid, RT, s, L.cost, trav, L.nbr, L.list, L.act, L.meta, limit, round);
  else
    LAYER_LAUNCH(k_wr_relax<false>, grid, RT, s, L.cost, trav, L.nbr, L.list, L.act, L.meta, limit, round);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_REACH = {"world reach", "world reach field", "sdm_world_reach_update", false};
}  // namespace

extern "C" {

sdm_status sdm_world_reach_update(sdm_map *m, const sdm_world_reach_options *o, const float *start_xyz, const int32_t *start_cells,
                                  int64_t n_starts) {
  const char *what = "sdm_world_reach_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_REACH_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->inflate > 2 || o->pad != 0) return LAYER_REFUSE(what, "inflate > 2 or a non-zero pad");
  BrickBox box{};
  if (o->flags & SDM_WORLD_REACH_BOX) {
    box.use = 1u;
    for (int a = 0; a < 3; ++a) {
      if (o->bmax[a] < o->bmin[a]) return LAYER_REFUSE(what, "bmax < bmin");
      box.lo[a] = o->bmin[a], box.hi[a] = o->bmax[a];
    }
  }
  if (n_starts < 0 || n_starts > 0x7fffffff || (start_xyz != nullptr) == (start_cells != nullptr))
    return LAYER_REFUSE(what, "n_starts < 0 or >= 2^31, or not exactly one of start_xyz and start_cells");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldReachLayer &L = m->wreach;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, R_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, R_WORDS, true));
  // the bricks of the field: the archive's in brick order, those of the box ranked
  DevTemps tmp;
  SnapshotBricks b;
  SDM_TRY(snapshot_bricks(m, box, (size_t)m->world.max_bricks + 1, L.h_meta, [&](uint32_t n_arch, uint32_t **flag, uint32_t **rank) -> sdm_status {
    HIP_TRY(tmp.alloc(flag, (size_t)n_arch + 1));
    HIP_TRY(tmp.alloc(rank, (size_t)n_arch + 1));
    return SDM_OK;
  }, &b));
  const uint32_t n = b.n;
  uint32_t *slot_of = nullptr;
  SDM_TRY(reach_alloc(m, n));
  L.n = n;
  L.hmask = table_slots(n) - 1;
  unsigned char *d_starts = nullptr;
  if (n_starts > 0) {
    HIP_TRY(tmp.alloc(&d_starts, (size_t)n_starts * 12));
    HIP_TRY(hipMemcpyAsync(d_starts, start_xyz ? (const void *)start_xyz : (const void *)start_cells, (size_t)n_starts * 12, hipMemcpyHostToDevice, s));
  }
  if (n) HIP_TRY(tmp.alloc(&slot_of, n));
  HIP_TRY(launch_reach_prepare(m, *o, b.order, b.flag, b.rank, slot_of, b.n_arch, n, start_xyz ? reinterpret_cast<const float *>(d_starts) : nullptr,
                               start_xyz ? nullptr : reinterpret_cast<const int32_t *>(d_starts), (uint32_t)n_starts));
  // rounds of plain launches; the count of the last round issued says whether anything is still moving
  const bool face = (o->flags & SDM_WORLD_REACH_FACE_CONNECTED) != 0;
  const uint32_t limit = o->max_cost ? o->max_cost : NO_COST - 1u;
  if (n) {
    SDM_TRY(relax_rounds(
        m, what, REACH_BATCH, 512ull * n + REACH_BATCH, L.meta, L.h_meta, R_WORDS, L.h_meta + R_CNT,
        "the relaxation has not come to rest after 512 x n_bricks rounds",
        [n](uint32_t last) { return std::min<uint32_t>(n, std::max<uint32_t>(2u * last, 64u)); },
        [&](uint32_t grid, uint32_t round) { return launch_reach_round(L, face, limit, grid, round, s); }));
    hipLaunchKernelGGL(k_wr_reduce, dim3(std::min<uint32_t>(RR_GRID, (n * 8u + QT / 64 - 1) / (QT / 64))), dim3(QT), 0, s, L.cost, L.trav, n * 8u,
                       L.meta);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, R_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (the build's temporaries go when this returns)
  L.inflate = o->inflate;
  L.max_cost = o->max_cost;
  L.stamp = m->world.f.gts;
  L.built(m->world.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_reach(sdm_map *m, int16_t *coords, uint32_t *cost, int64_t first, int64_t cap, int64_t *n_out, sdm_world_reach_info *info) {
  const char *what = "sdm_get_world_reach";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wreach, WORLD_REACH));
  HIP_TRY(hipSetDevice(m->device));
  const WorldReachLayer &L = m->wreach;
  *n_out = (int64_t)L.n;
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>((int64_t)L.n - first, cap), 0);
  std::vector<uint32_t> pairs(coords ? 2 * take : 0);
  if (take && coords) HIP_TRY(hipMemcpyAsync(pairs.data(), L.coord + 2 * (size_t)first, 2 * take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (take && cost) HIP_TRY(hipMemcpyAsync(cost, L.cost + 512 * (size_t)first, 512 * take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  unpack_coords(pairs, coords);
  if (info) {
    const uint32_t *h = L.h_meta;  // (the build waited for them)
    info->n_bricks = L.n;
    info->n_starts_used = h[R_STARTS];
    info->n_traversable = h[R_TRAV];
    info->n_reached = h[R_REACHED];
    info->max_cost_reached = h[R_MAXCOST];
    info->rounds = h[R_ROUNDS];
    info->flags = L.flags;
    info->inflate = L.inflate;
    info->max_cost = L.max_cost;
    info->stamp = L.stamp;
  }
  return SDM_OK;
}

sdm_status sdm_query_world_reach(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_reach_result *out, uint32_t flags) {
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, "sdm_query_world_reach", &sdm_map::wreach, WORLD_REACH));
  const WorldReachLayer L = m->wreach;
  const float recip = m->d.recip, voxel_size = m->d.voxel_size;
  const bool face = (L.flags & SDM_WORLD_REACH_FACE_CONNECTED) != 0, points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, 12, out, sizeof(sdm_world_reach_result), nullptr, 0, n, flags,
                   [L, recip, voxel_size, face, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     const float *p = points ? static_cast<const float *>(in) : nullptr;
                     const int32_t *w = points ? nullptr : static_cast<const int32_t *>(in);
                     const uint32_t *trav = reinterpret_cast<const uint32_t *>(L.trav);
                     const dim3 grid((c + QT - 1) / QT), tpb(QT);
                     if (face)
                       hipLaunchKernelGGL(k_query_world_reach<true>, grid, tpb, 0, s, p, w, c, recip, voxel_size, L.keys, L.vals, L.hmask, L.nbr, trav,
                                          L.cost, static_cast<uint2 *>(o));
                     else
                       hipLaunchKernelGGL(k_query_world_reach<false>, grid, tpb, 0, s, p, w, c, recip, voxel_size, L.keys, L.vals, L.hmask, L.nbr, trav,
                                          L.cost, static_cast<uint2 *>(o));
                   });
}

sdm_status sdm_world_reach_paths(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, int32_t max_len, int32_t *cells_out,
                                 int32_t *len_out, uint32_t flags) {
  const char *what = "sdm_world_reach_paths";
  SDM_TRY(goal_query_check(m, xyz, cells, n, len_out, flags, what, &sdm_map::wreach, WORLD_REACH));
  const WorldReachLayer L = m->wreach;
  const float recip = m->d.recip;
  const bool face = (L.flags & SDM_WORLD_REACH_FACE_CONNECTED) != 0;
  return goal_paths(m, xyz, cells, n, max_len, cells_out, len_out, flags, what, (size_t)L.n * 512,
                    [&](const float *p, const int32_t *w, uint32_t c, uint32_t len_cap, size_t stride, int32_t *rows, int32_t *lens) {
                      const uint32_t *trav = reinterpret_cast<const uint32_t *>(L.trav);
                      const dim3 grid((c + QT - 1) / QT), tpb(QT);
                      if (face)
                        hipLaunchKernelGGL(k_world_reach_paths<true>, grid, tpb, 0, m->stream, p, w, c, recip, L.keys, L.vals, L.hmask, L.nbr, trav,
                                           L.cost, len_cap, stride, rows, lens);
                      else
                        hipLaunchKernelGGL(k_world_reach_paths<false>, grid, tpb, 0, m->stream, p, w, c, recip, L.keys, L.vals, L.hmask, L.nbr, trav,
                                           L.cost, len_cap, stride, rows, lens);
                    });
}

sdm_status sdm_debug_world_reach_bricks(sdm_map *m, int64_t *bricks_out) {
  if (!m || !bricks_out) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_debug_world_reach_bricks", &m->wreach, WORLD_REACH));
  *bricks_out = (int64_t)m->wreach.h_meta[R_BRICKS];
  return SDM_OK;
}

}  // extern "C"
