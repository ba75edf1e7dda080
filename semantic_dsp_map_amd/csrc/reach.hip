// reach.hip — the travel-cost field: the cheapest path from a set of start cells to every traversable cell of the map
// block, the cost at a goal and the path itself (gfx950; include/sdm.h, "travel cost").
//
// A snapshot of one frame in map-index cells, like the distance field, the instance table and the frontiers.  cost[] is
// the unique fixed point of  cost(c) = min(cost(c), cost(c + o) + w(o))  over the allowed moves, from cost = 0 at the
// starts and 0xffffffff elsewhere; every value ever stored is the weight of a real path, values only ever decrease, and
// the build ends when nothing can be lowered any more - so the field is the same whatever order the device relaxes in.
//   k_reach_classify  a wave per chunk of 64 cells in map-index order (RC_U chunks a wave, all loads first): reads the
//               results through the ring correction - or, with a clearance, the distance field's snapshot and site,
//               which are in map-index order already - and writes one word of the traversable mask from a ballot and
//               0xffffffff into the 64 costs.
//   k_reach_seed      a thread per start: its cell (a point's by the distance query's rule), cost 0 by atomicMin - the
//               thread that lowers it counts the start -, and the activity bit of the cell's tile and its 26 neighbours.
//   k_reach_list      a thread per word of the tiles' activity mask: takes the word (and leaves zero) and appends its
//               tiles to the round's list.  The list's order changes from run to run; the result cannot.
//   k_reach_relax     a workgroup per listed tile of up to 8 x 8 x 8 cells (clipped on 4-cell axes): loads the tile and
//               a one-cell halo of costs and traversable bits into LDS (at most 1000 words and 1000 bytes), gives every
//               cell the mask of its allowed moves from the 27 bits around it, relaxes inside LDS behind barriers
//               until a whole sweep changes nothing, stores the cells it lowered - only a tile's owner ever writes a
//               cell - and sets, with an atomic OR, the activity bit of every face, edge or corner neighbour tile whose
//               halo holds a cell it lowered.  A neighbour that read such a halo word stale in this round is thereby
//               simply run again in the next: data crosses workgroups only across kernel boundaries, no kernel waits
//               for another workgroup, and the host loop (which reads the last round's count every few rounds) carries
//               a hard cap of V rounds.
//   k_reach_reduce    counts the traversable and the reached cells and takes the largest cost.
//   k_query_reach     a lane per goal: the 27 costs and mask words round the goal's cell are issued together; status,
//               cost, metres and the first descent step.
//   k_reach_paths     a lane per goal: one descent step per round trip to memory, the loads of a step issued together.
//               The chain is as long as the path and each step depends on the one before: it is bound by latency.
#include "sdm_layer.h"
#include "sdm_map.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_reach_info) == 32 && sizeof(sdm_reach_result) == 16, "sdm.h layout");
static_assert(offsetof(sdm_reach_result, next) == 12 && offsetof(sdm_reach_result, pad) == 14, "sdm.h layout");

namespace sdm {

namespace {

constexpr int RC_TPB = 256, RC_WAVES = RC_TPB / 64;
constexpr int RC_U = 8;             // chunks (mask words) a wave takes
constexpr int RT_TPB = 256;         // k_reach_relax: up to two cells of the tile and four of the halo region a thread
constexpr int RT_REGION = 1000;     // (8 + 2)^3
constexpr int RQ_TPB = 256;
constexpr uint32_t RR_GRID = 1024;  // k_reach_reduce strides over the chunks
constexpr uint32_t NO_COST = 0xffffffffu;
// the build's counters: the first four are sdm_reach_info's; the tiles relaxed in all rounds; the two counts of listed
// tiles, round r's in M_CNT + (r & 1)
enum { M_STARTS = 0, M_TRAV, M_REACHED, M_MAXCOST, M_ROUNDS, M_TILES, M_CNT, META_WORDS = 8 };

struct Reach {  // everything a build or a query touches
  uint32_t *cost;  // [V]
  uint32_t *trav;  // [V / 32]: bit c & 31 of word c >> 5
  uint32_t *act;   // [(n_tiles + 31) / 32]
  uint32_t *list;  // [n_tiles]
  uint32_t *meta;  // [META_WORDS]
  int x_n, y_n, z_n;
  int tx_n, ty_n, tz_n;  // the tile: 2^tx_n x 2^ty_n x 2^tz_n cells
  uint32_t n_tiles;
  uint32_t limit;        // costs above it are not stored (max_cost, or the largest cost there is)
};

// ---- moves -----------------------------------------------------------------------------------------------------------
constexpr int move_d(int n, int a) { return a == 0 ? n % 3 - 1 : a == 1 ? (n / 3) % 3 - 1 : n / 9 - 1; }
constexpr uint32_t move_weight(int n) {
  const int k = (move_d(n, 0) != 0) + (move_d(n, 1) != 0) + (move_d(n, 2) != 0);
  return k == 1 ? 10u : k == 2 ? 14u : 17u;
}
// the cells c + s, s_a in {0, o_a}, as bits of the 27 cells round c (numbered like the moves)
constexpr uint32_t move_needs(int n) {
  uint32_t m = 0;
  for (int k = 0; k < 8; ++k) {
    const int sx = (k & 1) ? move_d(n, 0) : 0, sy = (k & 2) ? move_d(n, 1) : 0, sz = (k & 4) ? move_d(n, 2) : 0;
    m |= 1u << ((sz + 1) * 9 + (sy + 1) * 3 + (sx + 1));
  }
  return m;
}
constexpr uint32_t FACE_MOVES = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22);
static_assert(move_weight(12) == 10 && move_weight(0) == 17 && move_weight(1) == 14 && move_needs(14) == ((1u << 13) | (1u << 14)), "moves");
static_assert(SDM_REACH_COST_PER_CELL == 10, "sdm.h");

// the allowed moves of a cell from the traversable bits of the 27 cells round it (cells outside the map: 0)
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

// ---- classify --------------------------------------------------------------------------------------------------------
template <bool FIELD>
__global__ __launch_bounds__(RC_TPB) void k_reach_classify(Dims d, Frame f, const uint2 *__restrict__ res, const uint32_t *__restrict__ snap,
                                                           const uint32_t *__restrict__ site, uint32_t min_d2, uint32_t through_unknown,
                                                           u64 *__restrict__ trav, uint32_t *__restrict__ cost, uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * RC_WAVES + (threadIdx.x >> 6)) * RC_U;
  uint32_t w[RC_U], s[RC_U];
  if (FIELD) {
#pragma unroll
    for (int u = 0; u < RC_U; ++u) {  // every load first, like load_w1's: the field's words are in map-index order already
      const uint32_t chunk = first + (uint32_t)u;
      w[u] = RES_UNKNOWN_W1;
      s[u] = INVALID_INDEX;
      if (chunk < nw) {
        w[u] = snap[(chunk << 6) + lane];
        s[u] = site[(chunk << 6) + lane];
      }
    }
  } else {
    load_w1(d, f, res, first, nw, lane, w);
  }
#pragma unroll
  for (int u = 0; u < RC_U; ++u) {
    const uint32_t chunk = first + (uint32_t)u;
    if (chunk >= nw) break;  // (wave-uniform)
    const uint32_t c = (chunk << 6) + lane;
    const int occ = occ_of(w[u]);
    bool ok = occ == 0 || (through_unknown && occ == -1);
    if (FIELD && s[u] != INVALID_INDEX) {  // (no site: no obstacle anywhere, d2 = 0xffffffff passes)
      int x, y, z, sx, sy, sz;
      cell_xyz(d, c, x, y, z);
      cell_xyz(d, s[u], sx, sy, sz);
      const int dx = x - sx, dy = y - sy, dz = z - sz;
      ok = ok && (uint32_t)(dx * dx + dy * dy + dz * dz) >= min_d2;
    }
    const u64 tm = __ballot(ok);
    if (lane == 0) trav[chunk] = tm;
    cost[c] = NO_COST;
  }
}

// ---- goals and starts ------------------------------------------------------------------------------------------------
// entry i as a cell word: a cell word itself, or the cell of a point (point_cell); INVALID_INDEX outside the map and for
// non-finite points
__device__ __forceinline__ uint32_t entry_cell(const Dims &d, const Frame &f, const float *__restrict__ xyz, const uint32_t *__restrict__ cells,
                                               uint32_t i) {
  if (cells) {
    const uint32_t c = cells[i];
    return c < d.V ? c : INVALID_INDEX;
  }
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  return point_cell(d, f, p);
}

__device__ __forceinline__ bool is_traversable(const Reach &g, uint32_t c) { return (g.trav[c >> 5] >> (c & 31u)) & 1u; }

__global__ __launch_bounds__(RQ_TPB) void k_reach_seed(Dims d, Frame f, Reach g, const float *__restrict__ xyz, const uint32_t *__restrict__ cells,
                                                       uint32_t n) {
  const uint32_t i = blockIdx.x * RQ_TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = entry_cell(d, f, xyz, cells, i);
  if (c == INVALID_INDEX || !is_traversable(g, c)) return;
  if (atomicMin(g.cost + c, 0u) != 0u) atomicAdd(g.meta + M_STARTS, 1u);
  int x, y, z;
  cell_xyz(d, c, x, y, z);
  const int t[3] = {x >> g.tx_n, y >> g.ty_n, z >> g.tz_n};
  const int nt[3] = {1 << (g.x_n - g.tx_n), 1 << (g.y_n - g.ty_n), 1 << (g.z_n - g.tz_n)};
  for (int k = 0; k < 27; ++k) {  // the tile and its neighbours: a start on a tile's border is news for their halos
    const int a = t[0] + move_d(k, 0), b = t[1] + move_d(k, 1), e = t[2] + move_d(k, 2);
    if ((uint32_t)a >= (uint32_t)nt[0] || (uint32_t)b >= (uint32_t)nt[1] || (uint32_t)e >= (uint32_t)nt[2]) continue;
    const uint32_t tile = (uint32_t)a | ((uint32_t)b << (g.x_n - g.tx_n)) | ((uint32_t)e << (g.x_n - g.tx_n + g.y_n - g.ty_n));
    atomicOr(g.act + (tile >> 5), 1u << (tile & 31u));
  }
}

// ---- a round: the list of active tiles, then their relaxation ---------------------------------------------------------
__global__ __launch_bounds__(RQ_TPB) void k_reach_list(Reach g, uint32_t round) {
  const uint32_t i = blockIdx.x * RQ_TPB + threadIdx.x;
  if (i >= (g.n_tiles + 31u) / 32u) return;
  uint32_t w = g.act[i];
  if (!w) return;
  g.act[i] = 0u;
  uint32_t at = atomicAdd(g.meta + M_CNT + (round & 1u), (uint32_t)__popc(w));  // (<= n_tiles in all: a tile has one bit)
  while (w) {
    g.list[at++] = i * 32u + (uint32_t)__builtin_ctz(w);
    w &= w - 1u;
  }
}

// The tile's extents are template arguments (2^TXN x 2^TYN x 2^TZN cells, 4 or 8 an axis): every offset into the region
// is then a constant of the instruction, and the sweep is straight-line code - it reads all its neighbours and selects,
// so no move costs a branch.
template <bool FACE, int TXN, int TYN, int TZN>
__global__ __launch_bounds__(RT_TPB) void k_reach_relax(Reach g, uint32_t round) {
  constexpr int TX = 1 << TXN, TY = 1 << TYN, TZ = 1 << TZN;
  constexpr int RX = TX + 2, RY = TY + 2, RZ = TZ + 2, RXY = RX * RY, RC = RXY * RZ;
  constexpr int TC = TX * TY * TZ;
  constexpr int KR = (RC + RT_TPB - 1) / RT_TPB, KT = (TC + RT_TPB - 1) / RT_TPB;  // cells of the region / of the tile a thread
  static_assert(RC <= RT_REGION && KR <= 4 && KT <= 2, "the tile");
  __shared__ uint32_t s_cost[RC];
  __shared__ uint8_t s_trav[RC];
  __shared__ uint32_t s_wake;
  const uint32_t count = g.meta[M_CNT + (round & 1u)];
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // (the next round's count: nobody reads or adds to it in this launch)
    g.meta[M_CNT + ((round + 1u) & 1u)] = 0u;
    if (count) {
      g.meta[M_ROUNDS] += 1u;
      g.meta[M_TILES] += count;
    }
  }
  const int tid = (int)threadIdx.x;
  const int NX = 1 << g.x_n, NY = 1 << g.y_n, NZ = 1 << g.z_n, xy_n = g.x_n + g.y_n;
  const int ntx_n = g.x_n - TXN, nty_n = g.y_n - TYN, ntz_n = g.z_n - TZN;
  const uint32_t limit = g.limit;
  for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {  // (count is the same for every thread: the barriers are whole)
    const uint32_t tile = g.list[t];
    const int tix = (int)(tile & ((1u << ntx_n) - 1u)), tiy = (int)((tile >> ntx_n) & ((1u << nty_n) - 1u)), tiz = (int)(tile >> (ntx_n + nty_n));
    const int x0 = tix << TXN, y0 = tiy << TYN, z0 = tiz << TZN;
    if (tid == 0) s_wake = 0u;
    // the tile and its halo: every load first
    uint32_t lc[KR], lw[KR], ls[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = tid + k * RT_TPB;
      lc[k] = NO_COST;
      lw[k] = 0u;
      ls[k] = 0u;
      if (i < RC) {
        const int rx = i % RX, r = i / RX, ry = r % RY, rz = r / RY;
        const int gx = x0 + rx - 1, gy = y0 + ry - 1, gz = z0 + rz - 1;
        if ((uint32_t)gx < (uint32_t)NX && (uint32_t)gy < (uint32_t)NY && (uint32_t)gz < (uint32_t)NZ) {
          const uint32_t c = (uint32_t)gx | ((uint32_t)gy << g.x_n) | ((uint32_t)gz << xy_n);
          lc[k] = g.cost[c];
          lw[k] = g.trav[c >> 5];
          ls[k] = c & 31u;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = tid + k * RT_TPB;
      if (i < RC) {
        s_cost[i] = lc[k];
        s_trav[i] = (uint8_t)((lw[k] >> ls[k]) & 1u);
      }
    }
    __syncthreads();
    // this thread's cells: their place in the region, their allowed moves, their cost.  A thread past the tile's cells
    // (tiles of fewer than RT_TPB cells) takes cell 0's place with no allowed move: it reads and never writes.
    int ri[KT];
    uint32_t al[KT], cur[KT], was[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int i = tid + k * RT_TPB;
      const bool mine = i < TC;
      const int j = mine ? i : 0;
      ri[k] = ((j & (TX - 1)) + 1) + (((j >> TXN) & (TY - 1)) + 1) * RX + ((j >> (TXN + TYN)) + 1) * RXY;
      uint32_t nb = 0u;
#pragma unroll
      for (int n = 0; n < 27; ++n) nb |= (uint32_t)s_trav[ri[k] + move_d(n, 0) + move_d(n, 1) * RX + move_d(n, 2) * RXY] << n;
      al[k] = mine ? allowed_moves<FACE>(nb) : 0u;
      cur[k] = was[k] = mine ? s_cost[ri[k]] : NO_COST;
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
          // arithmetic, not a condition (26 lane masks would not fit the scalar registers): a move that is not allowed
          // makes its neighbour NO_COST, and NO_COST plus a weight saturates and stays above the limit
          const uint32_t v = s_cost[ri[k] + move_d(n, 0) + move_d(n, 1) * RX + move_d(n, 2) * RXY] | (((al[k] >> n) & 1u) - 1u);
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
    // what was lowered goes to memory, and to the neighbour tiles whose halo holds it goes the word to run
    uint32_t wake = 0u;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (cur[k] < was[k]) {  // (never for a thread past the tile: both are NO_COST there)
        const int i = tid + k * RT_TPB;
        const int lx = i & (TX - 1), ly = (i >> TXN) & (TY - 1), lz = i >> (TXN + TYN);
        g.cost[(uint32_t)(x0 + lx) | ((uint32_t)(y0 + ly) << g.x_n) | ((uint32_t)(z0 + lz) << xy_n)] = cur[k];
        const uint32_t ax = 2u | (lx == 0 ? 1u : 0u) | (lx == TX - 1 ? 4u : 0u);  // bit d + 1: the tile at offset d sees the cell
        const uint32_t ay = 2u | (ly == 0 ? 1u : 0u) | (ly == TY - 1 ? 4u : 0u);
        const uint32_t az = 2u | (lz == 0 ? 1u : 0u) | (lz == TZ - 1 ? 4u : 0u);
#pragma unroll
        for (int n = 0; n < 27; ++n) {
          if (n == 13 || (FACE && !((FACE_MOVES >> n) & 1u))) continue;  // (face moves never read an edge or corner halo)
          wake |= ((ax >> (move_d(n, 0) + 1)) & (ay >> (move_d(n, 1) + 1)) & (az >> (move_d(n, 2) + 1)) & 1u) << n;
        }
      }
    }
    if (wake) atomicOr(&s_wake, wake);
    __syncthreads();
    if (tid < 27 && ((s_wake >> tid) & 1u)) {
      const int a = tix + tid % 3 - 1, b = tiy + (tid / 3) % 3 - 1, e = tiz + tid / 9 - 1;
      if ((uint32_t)a < (1u << ntx_n) && (uint32_t)b < (1u << nty_n) && (uint32_t)e < (1u << ntz_n)) {
        const uint32_t nt = (uint32_t)a | ((uint32_t)b << ntx_n) | ((uint32_t)e << (ntx_n + nty_n));
        atomicOr(g.act + (nt >> 5), 1u << (nt & 31u));
      }
    }
    __syncthreads();  // (s_wake and the region are the next tile's from here on)
  }
}

// the relaxation for a connectivity and a tile: [face][tx_n - 2][ty_n - 2][tz_n - 2]
typedef void (*relax_fn)(Reach, uint32_t);
#define SDM_RELAX_ROW(F) \
  {{{k_reach_relax<F, 2, 2, 2>, k_reach_relax<F, 2, 2, 3>}, {k_reach_relax<F, 2, 3, 2>, k_reach_relax<F, 2, 3, 3>}}, \
   {{k_reach_relax<F, 3, 2, 2>, k_reach_relax<F, 3, 2, 3>}, {k_reach_relax<F, 3, 3, 2>, k_reach_relax<F, 3, 3, 3>}}}
const relax_fn RELAX[2][2][2][2] = {SDM_RELAX_ROW(false), SDM_RELAX_ROW(true)};
#undef SDM_RELAX_ROW

// ---- the info block ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RC_TPB) void k_reach_reduce(Reach g, uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n_trav = 0, n_reached = 0, top = 0;
  for (uint32_t chunk = blockIdx.x * RC_WAVES + (threadIdx.x >> 6); chunk < nw; chunk += gridDim.x * RC_WAVES) {  // (wave-uniform)
    const uint32_t v = g.cost[(chunk << 6) + lane];
    const u64 tm = reinterpret_cast<const u64 *>(g.trav)[chunk];
    n_trav += (uint32_t)__popcll(tm);
    n_reached += (uint32_t)__popcll(__ballot(v != NO_COST));
    if (v != NO_COST) top = max(top, v);
  }
  top = wave_max(top);
  if (lane == 0) {
    if (n_trav) atomicAdd(g.meta + M_TRAV, n_trav);
    if (n_reached) atomicAdd(g.meta + M_REACHED, n_reached);
    if (top) atomicMax(g.meta + M_MAXCOST, top);
  }
}

// ---- queries ----------------------------------------------------------------------------------------------------------
// the first descent step from cell (x, y, z) with cost `cost_c`: the smallest allowed move n with cost(c + o) + w(o) ==
// cost_c, the neighbour's cell word and cost; 255 if there is none.  The 27 costs and mask words are issued together.
template <bool FACE>
__device__ __forceinline__ void descent_step(const Reach &g, int x, int y, int z, uint32_t cost_c, uint32_t &next, uint32_t &next_cell,
                                             uint32_t &next_cost) {
  const int NX = 1 << g.x_n, NY = 1 << g.y_n, NZ = 1 << g.z_n, xy_n = g.x_n + g.y_n;
  uint32_t cw[27], tw[27];
#pragma unroll
  for (int n = 0; n < 27; ++n) {
    cw[n] = NO_COST;
    tw[n] = 0u;
    if (FACE && n != 13 && !((FACE_MOVES >> n) & 1u)) continue;
    const int nx = x + move_d(n, 0), ny = y + move_d(n, 1), nz = z + move_d(n, 2);
    if ((uint32_t)nx < (uint32_t)NX && (uint32_t)ny < (uint32_t)NY && (uint32_t)nz < (uint32_t)NZ) {
      const uint32_t c = (uint32_t)nx | ((uint32_t)ny << g.x_n) | ((uint32_t)nz << xy_n);
      cw[n] = g.cost[c];
      tw[n] = g.trav[c >> 5];
    }
  }
  uint32_t nb = 0u;
#pragma unroll
  for (int n = 0; n < 27; ++n) {
    const uint32_t c = (uint32_t)(x + move_d(n, 0)) | ((uint32_t)(y + move_d(n, 1)) << g.x_n) | ((uint32_t)(z + move_d(n, 2)) << xy_n);
    nb |= ((tw[n] >> (c & 31u)) & 1u) << n;  // (outside the map the word is 0)
  }
  const uint32_t al = allowed_moves<FACE>(nb);
  next = 255u;
  next_cell = INVALID_INDEX;
  next_cost = NO_COST;
#pragma unroll
  for (int n = 26; n >= 0; --n) {  // (descending, so the smallest n is the last to overwrite)
    if (n == 13 || (FACE && !((FACE_MOVES >> n) & 1u))) continue;
    if (((al >> n) & 1u) && cw[n] != NO_COST && cw[n] + move_weight(n) == cost_c) {
      next = (uint32_t)n;
      next_cost = cw[n];
      next_cell = (uint32_t)(x + move_d(n, 0)) | ((uint32_t)(y + move_d(n, 1)) << g.x_n) | ((uint32_t)(z + move_d(n, 2)) << xy_n);
    }
  }
}

template <bool FACE>
__global__ __launch_bounds__(RQ_TPB) void k_query_reach(Dims d, Frame f, Reach g, const float *__restrict__ xyz, const uint32_t *__restrict__ cells,
                                                        uint32_t n, sdm_reach_result *__restrict__ out) {
  const uint32_t i = blockIdx.x * RQ_TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = entry_cell(d, f, xyz, cells, i);
  uint32_t cost = NO_COST, next = 255u, status = 3u;
  if (c != INVALID_INDEX) {
    const uint32_t v = g.cost[c];
    const bool tr = is_traversable(g, c);
    status = !tr ? 2u : v == NO_COST ? 1u : 0u;
    if (status == 0u) {
      cost = v;
      next = 13u;
      if (v != 0u) {
        uint32_t nc, nv;
        int x, y, z;
        cell_xyz(d, c, x, y, z);
        descent_step<FACE>(g, x, y, z, v, next, nc, nv);
      }
    }
  }
  const float metres = cost == NO_COST ? -1.f : (float)cost * (d.voxel_size * 0.1f);
  uint4 o;
  o.x = cost;
  o.y = __float_as_uint(metres);
  o.z = c;
  o.w = next | (status << 8);  // next, status, pad = 0
  reinterpret_cast<uint4 *>(out)[i] = o;
}

template <bool FACE>
__global__ __launch_bounds__(RQ_TPB) void k_reach_paths(Dims d, Frame f, Reach g, const float *__restrict__ xyz, const uint32_t *__restrict__ cells,
                                                        uint32_t n, uint32_t max_len, size_t stride, uint32_t *__restrict__ cells_out,
                                                        int32_t *__restrict__ len_out) {
  const uint32_t i = blockIdx.x * RQ_TPB + threadIdx.x;
  if (i >= n) return;
  uint32_t c = entry_cell(d, f, xyz, cells, i);
  uint32_t len = 0;
  if (c != INVALID_INDEX) {
    uint32_t v = g.cost[c];  // (a cell with a cost is traversable)
    if (v != NO_COST) {
      const uint32_t longest = v / 10u + 1u;  // every move weighs at least 10: the loop ends whatever the field holds
      uint32_t *row = cells_out + (size_t)i * stride;
      for (;;) {
        if (len < max_len) row[len] = c;
        ++len;
        if (v == 0u || len >= longest) break;
        uint32_t next, nc, nv;
        int x, y, z;
        cell_xyz(d, c, x, y, z);
        descent_step<FACE>(g, x, y, z, v, next, nc, nv);
        if (next == 255u) break;
        c = nc;
        v = nv;
      }
    }
  }
  len_out[i] = (int32_t)len;
}

Reach reach_of(const sdm_map *m, uint32_t max_cost) {
  const Dims &d = m->d;
  Reach g;
  g.cost = m->reach.cost;
  g.trav = m->reach.trav;
  g.act = m->reach.act;
  g.list = m->reach.list;
  g.meta = m->reach.meta;
  g.x_n = d.x_n, g.y_n = d.y_n, g.z_n = d.z_n;
  g.tx_n = std::min(d.x_n, 3), g.ty_n = std::min(d.y_n, 3), g.tz_n = std::min(d.z_n, 3);
  g.n_tiles = d.V >> (g.tx_n + g.ty_n + g.tz_n);
  g.limit = max_cost ? max_cost : NO_COST - 1u;
  return g;
}

constexpr uint32_t REACH_BATCH = 8;  // rounds issued between two looks at the count (SDM_REACH_BATCH overrides: tools/probes/reach_probe.py)

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName REACH = {"the travel cost", "travel-cost field", "sdm_reach_update", false};

// the checks the two goal queries share
sdm_status goal_query_check(sdm_map *m, const float *xyz, const uint32_t *cells, int64_t n, const void *out, uint32_t flags, const char *what) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if ((xyz != nullptr) == (cells != nullptr)) {
    set_error(what, __FILE__, __LINE__, "exactly one of xyz and cells must be given");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(query_check(m, xyz ? (const void *)xyz : (const void *)cells, n, out, flags, SDM_QUERY_ON_DEVICE, what));
  return layer_check(m, what, &m->reach, REACH);
}
}  // namespace

extern "C" {

sdm_status sdm_reach_update(sdm_map *m, const float *start_xyz, const uint32_t *start_cells, int64_t n_starts, uint32_t min_d2,
                            uint32_t max_cost, uint32_t flags) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (flags & ~(SDM_REACH_FACE_CONNECTED | SDM_REACH_THROUGH_UNKNOWN)) {
    set_error("sdm_reach_update", __FILE__, __LINE__, "unknown flag bits");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  if (n_starts < 0 || n_starts > 0x7fffffff || (start_xyz != nullptr) == (start_cells != nullptr)) {
    set_error("sdm_reach_update", __FILE__, __LINE__, "n_starts < 0 or >= 2^31, or not exactly one of start_xyz and start_cells");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_reach_update", nullptr, REACH));
  if (min_d2 > 0 && !m->esdf.valid) {
    set_error("sdm_reach_update", __FILE__, __LINE__, "min_d2 > 0 needs the distance field: call sdm_esdf_update first");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(m->device));
  const Dims &d = m->d;
  const uint32_t nw = d.V >> 6;
  if (!m->reach.cost) SDM_TRY(alloc_tracked(m, &m->reach.cost, d.V));
  if (!m->reach.trav) SDM_TRY(alloc_tracked(m, &m->reach.trav, (size_t)nw * 2));
  if (!m->reach.meta) SDM_TRY(alloc_tracked(m, &m->reach.meta, META_WORDS));
  if (!m->reach.h_meta) SDM_TRY(alloc_tracked(m, &m->reach.h_meta, META_WORDS, true));
  const uint32_t n_tiles = d.V >> (std::min(d.x_n, 3) + std::min(d.y_n, 3) + std::min(d.z_n, 3)), act_words = (n_tiles + 31u) / 32u;
  if (!m->reach.act) SDM_TRY(alloc_tracked(m, &m->reach.act, act_words));
  if (!m->reach.list) SDM_TRY(alloc_tracked(m, &m->reach.list, n_tiles));
  const Reach g = reach_of(m, max_cost);
  m->reach.valid = false;  // (until this build is complete)
  hipStream_t s = m->stream;
  const bool field = min_d2 > 0;
  const Frame f = field ? m->esdf.f : m->f;
  HIP_TRY(hipMemsetAsync(g.meta, 0, META_WORDS * sizeof(uint32_t), s));
  HIP_TRY(hipMemsetAsync(g.act, 0, (size_t)act_words * sizeof(uint32_t), s));
  const uint32_t by_word = (nw + RC_WAVES * RC_U - 1) / (RC_WAVES * RC_U);
  const uint32_t through = (flags & SDM_REACH_THROUGH_UNKNOWN) ? 1u : 0u;
  if (field)
    hipLaunchKernelGGL(k_reach_classify<true>, dim3(by_word), dim3(RC_TPB), 0, s, d, f, (const uint2 *)nullptr, m->esdf.snap, m->esdf.site,
                       min_d2, through, reinterpret_cast<u64 *>(g.trav), g.cost, nw);
  else
    hipLaunchKernelGGL(k_reach_classify<false>, dim3(by_word), dim3(RC_TPB), 0, s, d, f, reinterpret_cast<const uint2 *>(m->st.res),
                       (const uint32_t *)nullptr, (const uint32_t *)nullptr, 0u, through, reinterpret_cast<u64 *>(g.trav), g.cost, nw);
  HIP_TRY(hipGetLastError());
  DevTemps tmp;
  if (n_starts > 0) {
    unsigned char *d_starts = nullptr;
    const size_t bytes = (size_t)n_starts * (start_xyz ? 12 : 4);
    HIP_TRY(tmp.alloc(&d_starts, bytes));
    HIP_TRY(hipMemcpyAsync(d_starts, start_xyz ? (const void *)start_xyz : (const void *)start_cells, bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_reach_seed, dim3(((uint32_t)n_starts + RQ_TPB - 1) / RQ_TPB), dim3(RQ_TPB), 0, s, d, f, g,
                       start_xyz ? reinterpret_cast<const float *>(d_starts) : nullptr,
                       start_xyz ? nullptr : reinterpret_cast<const uint32_t *>(d_starts), (uint32_t)n_starts);
    HIP_TRY(hipGetLastError());
  }
  // rounds of plain launches; the count of the last round issued says whether anything is still moving
  const char *env = getenv("SDM_REACH_BATCH");
  const uint32_t batch = env && atoi(env) > 0 ? (uint32_t)atoi(env) : REACH_BATCH;
  const relax_fn relax = RELAX[(flags & SDM_REACH_FACE_CONNECTED) ? 1 : 0][g.tx_n - 2][g.ty_n - 2][g.tz_n - 2];  // (axes have 4 cells or more)
  const uint64_t cap = (uint64_t)d.V + batch;
  uint64_t round = 0;
  uint32_t grid = std::min<uint32_t>(g.n_tiles, 64u);
  for (;;) {
    for (uint32_t k = 0; k < batch; ++k, ++round) {
      hipLaunchKernelGGL(k_reach_list, dim3((act_words + RQ_TPB - 1) / RQ_TPB), dim3(RQ_TPB), 0, s, g, (uint32_t)round);
      hipLaunchKernelGGL(relax, dim3(grid), dim3(RT_TPB), 0, s, g, (uint32_t)round);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(m->reach.h_meta, g.meta, META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t last = m->reach.h_meta[M_CNT + ((round - 1) & 1u)];
    if (last == 0u) break;  // an empty round: nothing was lowered in the one before it, nothing ever will be
    if (round >= cap) {
      set_error("sdm_reach_update", __FILE__, __LINE__, "the relaxation has not come to rest after V rounds");
      return SDM_ERR_NOT_CONVERGED;
    }
    grid = std::min<uint32_t>(g.n_tiles, std::max<uint32_t>(2u * last, 64u));
  }
  hipLaunchKernelGGL(k_reach_reduce, dim3(std::min<uint32_t>(RR_GRID, (nw + RC_WAVES - 1) / RC_WAVES)), dim3(RC_TPB), 0, s, g, nw);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(m->reach.h_meta, g.meta, META_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  m->reach.min_d2 = min_d2;
  m->reach.max_cost = max_cost;
  m->reach.built(f, flags);
  return SDM_OK;
}

sdm_status sdm_get_reach(sdm_map *m, uint32_t *cost, sdm_reach_info *info, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_get_reach", &m->reach, REACH));
  HIP_TRY(hipSetDevice(m->device));
  if (cost) HIP_TRY(hipMemcpyAsync(cost, m->reach.cost, (size_t)m->d.V * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (info) {
    const uint32_t *h = m->reach.h_meta;  // (the build waited for them)
    info->n_starts_used = h[M_STARTS];
    info->n_traversable = h[M_TRAV];
    info->n_reached = h[M_REACHED];
    info->max_cost_reached = h[M_MAXCOST];
    info->rounds = h[M_ROUNDS];
    info->flags = m->reach.flags;
    info->min_d2 = m->reach.min_d2;
    info->max_cost = m->reach.max_cost;
  }
  layer_origin(m, m->reach, origin);
  return SDM_OK;
}

sdm_status sdm_query_reach(sdm_map *m, const float *xyz, const uint32_t *cells, int64_t n, sdm_reach_result *out, uint32_t flags) {
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, "sdm_query_reach"));
  const Frame f = m->reach.f;
  const Reach g = reach_of(m, m->reach.max_cost);
  const bool face = (m->reach.flags & SDM_REACH_FACE_CONNECTED) != 0, points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, points ? 12 : 4, out, sizeof(sdm_reach_result), nullptr, 0, n, flags,
                   [m, f, g, face, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     const float *p = points ? static_cast<const float *>(in) : nullptr;
                     const uint32_t *w = points ? nullptr : static_cast<const uint32_t *>(in);
                     const dim3 grid((c + RQ_TPB - 1) / RQ_TPB), tpb(RQ_TPB);
                     if (face)
                       hipLaunchKernelGGL(k_query_reach<true>, grid, tpb, 0, s, m->d, f, g, p, w, c, static_cast<sdm_reach_result *>(o));
                     else
                       hipLaunchKernelGGL(k_query_reach<false>, grid, tpb, 0, s, m->d, f, g, p, w, c, static_cast<sdm_reach_result *>(o));
                   });
}

sdm_status sdm_reach_paths(sdm_map *m, const float *xyz, const uint32_t *cells, int64_t n, int32_t max_len, uint32_t *cells_out,
                           int32_t *len_out, uint32_t flags) {
  SDM_TRY(goal_query_check(m, xyz, cells, n, len_out, flags, "sdm_reach_paths"));
  if (max_len < 0 || (max_len > 0 && !cells_out)) {
    set_error("sdm_reach_paths", __FILE__, __LINE__, "max_len < 0, or no cells_out for max_len > 0");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  const Frame f = m->reach.f;
  const Reach g = reach_of(m, m->reach.max_cost);
  const bool face = (m->reach.flags & SDM_REACH_FACE_CONNECTED) != 0;
  const size_t in_elem = xyz ? 12 : 4;
  const unsigned char *in = xyz ? reinterpret_cast<const unsigned char *>(xyz) : reinterpret_cast<const unsigned char *>(cells);
  auto launch = [&](const void *src, uint32_t c, uint32_t len_cap, size_t stride, uint32_t *rows, int32_t *lens) {
    const float *p = xyz ? static_cast<const float *>(src) : nullptr;
    const uint32_t *w = xyz ? nullptr : static_cast<const uint32_t *>(src);
    const dim3 grid((c + RQ_TPB - 1) / RQ_TPB), tpb(RQ_TPB);
    if (face)
      hipLaunchKernelGGL(k_reach_paths<true>, grid, tpb, 0, m->stream, m->d, f, g, p, w, c, len_cap, stride, rows, lens);
    else
      hipLaunchKernelGGL(k_reach_paths<false>, grid, tpb, 0, m->stream, m->d, f, g, p, w, c, len_cap, stride, rows, lens);
  };
  if (flags & SDM_QUERY_ON_DEVICE)  // (run_query's chunks: a row of the caller's is max_len cells)
    return run_query(m, in, in_elem, len_out, 4, cells_out, (size_t)max_len * 4, n, flags, [&](const void *src, void *lens, void *rows, uint32_t c, hipStream_t) {
      launch(src, c, (uint32_t)max_len, (size_t)max_len, static_cast<uint32_t *>(rows), static_cast<int32_t *>(lens));
    });
  constexpr size_t CHUNK = (size_t)1 << 20;
  // host mode: through the queries' staging area, in chunks of whole rows; a staged row holds what a path can be long (no
  // path has more cells than the map), and only the cells a path has are copied into the caller's row
  const size_t row = std::min<size_t>((size_t)max_len, m->d.V);
  const size_t chunk = std::min<size_t>((size_t)n, std::max<size_t>(1, std::min(CHUNK, ((size_t)16 << 20) / std::max<size_t>(row * 4, 1))));
  return run_staged(
      m, (size_t)n, chunk, nullptr, 0,
      {{StageCol::IN, const_cast<unsigned char *>(in), in_elem}, {StageCol::OUT, len_out, 4}, {StageCol::OUT_RAW, nullptr, row * 4}},
      [&](const unsigned char *, unsigned char *const *col, size_t c) -> sdm_status {
        launch(col[0], (uint32_t)c, (uint32_t)row, row, reinterpret_cast<uint32_t *>(col[2]), reinterpret_cast<int32_t *>(col[1]));
        HIP_TRY(hipGetLastError());
        return SDM_OK;
      },
      [&](const unsigned char *const *col, size_t off, size_t c) {
        const int32_t *lens = reinterpret_cast<const int32_t *>(col[1]);
        for (size_t i = 0; i < c; ++i) {
          const size_t take = std::min<size_t>((size_t)lens[i], row);
          if (take) memcpy(cells_out + (off + i) * (size_t)max_len, col[2] + i * row * 4, take * 4);
        }
      });
}

sdm_status sdm_debug_reach_tiles(sdm_map *m, int64_t *tiles_out) {
  if (!m || !tiles_out) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_debug_reach_tiles", &m->reach, REACH));
  *tiles_out = (int64_t)m->reach.h_meta[M_TILES];
  return SDM_OK;
}

}  // extern "C"
