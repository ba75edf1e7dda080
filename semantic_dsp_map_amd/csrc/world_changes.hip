// world_changes.hip — world changes: what the block sees against what the archive remembers, cell by cell; the cells that
// changed as a list, joined into connected regions of one key (the class, or class and label pair) across brick borders, a
// table of the regions with counts, boxes and first moments, per-label counters and a query from a point or a cell to its
// change (gfx950; include/sdm.h, "world changes").
//
// A brick is 8 x 8 x 8 cells, a layer of it one 64-bit word (bit cx + 8 cy).  The two sides meet at the world cell
// g = moved_steps + i - (N >> 1), sdm_world_update's own geometry, and the candidates are that update's: the bricks the
// block overlaps in (bz, by, bx) order.  The build is a snapshot: what it leaves are the field's coordinates, a hash table of
// its own from brick key to rank, the listed words with their prefix and class planes, the lists and the table; it writes
// nothing of the map or the archive.  Everything it accumulates is an integer sum, minimum, maximum or OR, and a region's
// root is its smallest list index whatever order the unions arrive in: two builds give the same bytes.
//   k_wc_mark        a wave per candidate brick, a lane per (cx, cy), the eight z layers' loads of the results' second word
//               issued first; lane 0 makes the one lookup in the archive's table and reads the header's stamp, the eight
//               archived words come in through load_brick (an absent brick loads nothing: it reads unknown).  Both sides
//               are classified in registers by one function (cell_writes under the layer's flags); per layer ballots give
//               the listed word and two bit planes of the class, and the eleven counters are popcounts of ballots, summed
//               three to a scalar register, that lanes 0 .. 10 add to copy (candidate & 63) of each.  A flag per candidate
//               with a listed cell.
//   snapshot_rank    world_snapshot.hip's: ranks the flags - the build's first wait.
//   k_wc_index       a thread per candidate: a flagged one writes its coordinates and pool slot at its rank, inserts
//               key -> rank into the layer's table and moves its listed words, their popcounts and the class planes there.
//   launch_snapshot_neighbours   world_snapshot.hip's k_ws_neighbours, as it is.
//   exclusive_scan_u32 over the 8 n + 1 popcounts: every word's first list index and the cell count - the second wait.
//   k_wc_compact     a wave per field brick: reads again the block's and the archive's words of that brick only (changes
//               are sparse) and writes world cell, now, before, class and key at the list index.
//   k_wc_label_local a wave per field brick: sdm_world.h's local_labels, sweep_local_labels - the sweep world_objects.hip
//               runs, one copy - and store_local_roots, the keys read from the per-cell key array.
//   k_wc_seams       sdm_world.h's seam_unions, the key read from the per-cell key array.
//   k_wc_roots + exclusive_scan_u32   the root of every cell, the roots ranked and counted - the third wait.
//   k_wc_accumulate, k_wc_flags + exclusive_scan_u32, k_wc_table, k_wc_assign   as in world_objects.hip without second
//               moments; the per-label counters are reduced per workgroup in LDS before the atomics.
//   k_query_world_changes   a thread per entry, as k_query_world_objects, with the class from the two planes.
// No kernel uses LDS but k_wc_assign, none scratch; every buffer is a __restrict__ argument.  This unit includes no code of
// a frame unit.  The candidate walk and the block's brick load restate world.hip's (its unnamed namespace; that unit is not
// edited for this layer).
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_changes_options) == 64 && sizeof(sdm_world_change_region) == 112 && sizeof(sdm_world_changes_info) == 128 &&
                  sizeof(sdm_world_change_result) == 24,
              "sdm.h layout");
static_assert(offsetof(sdm_world_changes_options, max_cells) == 8 && offsetof(sdm_world_changes_options, labels) == 16 &&
                  offsetof(sdm_world_changes_options, classes) == 48 && offsetof(sdm_world_changes_options, pad) == 56 &&
                  offsetof(sdm_world_change_region, cls) == 8 && offsetof(sdm_world_change_region, first_cell) == 12 &&
                  offsetof(sdm_world_change_region, cell_sum) == 48 && offsetof(sdm_world_change_region, box_min) == 72 &&
                  offsetof(sdm_world_change_region, pad) == 108 && offsetof(sdm_world_changes_info, n_candidates) == 88 &&
                  offsetof(sdm_world_changes_info, n_cells) == 96 && offsetof(sdm_world_changes_info, n_regions) == 104 &&
                  offsetof(sdm_world_changes_info, stamp) == 124 && offsetof(sdm_world_change_result, region) == 12,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;             // the kernels of a thread or a wave per item
constexpr uint32_t WC_GRID = 4096;  // the largest grid of the kernels over cells: they stride
constexpr uint32_t ALL_WC_FLAGS = SDM_WORLD_CHANGES_FACE_CONNECTED | SDM_WORLD_CHANGES_BY_LABEL | SDM_WORLD_CHANGES_STATIC_ONLY |
                                  SDM_WORLD_CHANGES_OBSERVED_ONLY | SDM_WORLD_CHANGES_OLDER;
constexpr uint32_t ALL_CLASSES = (1u << SDM_WORLD_CHANGE_APPEARED) | (1u << SDM_WORLD_CHANGE_VANISHED) | (1u << SDM_WORLD_CHANGE_RELABELLED);
// the eleven counters in the order of sdm_world_changes_info
enum { C_APPEARED = 0, C_VANISHED, C_RELABELLED, C_SAME_OCC, C_SAME_FREE, C_NEW_OCC, C_NEW_FREE, C_REMEMBERED, C_KNOWN_NOW, C_KNOWN_BEFORE,
       C_OUTSIDE, N_COUNTERS };
// the build's counters, 64 bits each: every counter in G_SPREAD copies (a wave adds to copy candidate & 63, the getter sums
// them), the regions listed, per label the appeared, vanished and relabelled cells
enum { G_SPREAD = 64, G_COUNT = 0, G_LISTED = N_COUNTERS * G_SPREAD, G_LAB = G_LISTED + 1, G_WORDS = G_LAB + 3 * 256 };
static_assert(N_COUNTERS == 11 && offsetof(sdm_world_changes_info, n_outside) == 8 * C_OUTSIDE, "the info record's counters");

struct WcAcc {  // per region; all zero = no cell yet.  nmin / max: the largest ~code / code, code = coordinate ^ 2^31
  u64 sum[3];
  uint32_t n, nmin[3], max[3], mixed;
};
struct WcRule {  // how a side is classified and which cells are listed, by value
  uint32_t labels[8];
  uint32_t wflags;  // the archive's flags that stand for the layer's (cell_writes)
  uint32_t classes, older, max_last_stamp, by_label;
  int max_movable;
};
static_assert(sizeof(WcAcc) == 56, "bytes per region in sdm.h");
constexpr size_t CAND_BYTES = 4 + 4 + 4 + 3 * 8 * 8;                                        // flag, rank, slot; listed words, two planes
constexpr size_t BRICK_BYTES = 8 + 4 + 27 * 4 + 8 * 8 + 8 * 4 + 2 * 8 * 8 + 2 * (8 + 4);    // coord, slot, nbr, listed words, prefix, planes, two hash slots
constexpr size_t CELL_BYTES = 12 + 4 + 4 + 4 + 1 + 3 * 4;                                   // xyz, now, before, key, class; parent, root, idx
constexpr size_t REGION_BYTES = sizeof(WcAcc) + sizeof(sdm_world_change_region) + 4 + 4;    // first, lidx
static_assert(CAND_BYTES == SDM_WORLD_CHANGES_BYTES_PER_CANDIDATE && BRICK_BYTES == SDM_WORLD_CHANGES_BYTES_PER_BRICK &&
                  CELL_BYTES == SDM_WORLD_CHANGES_BYTES_PER_CELL && REGION_BYTES == SDM_WORLD_CHANGES_BYTES_PER_REGION &&
                  (2 * G_WORDS + 1) * 8 == 23576,
              "sdm.h states the bytes");

// ---- the block over the bricks: world.hip's candidate walk and brick load ------------------------------------------------
__device__ __forceinline__ void candidate_brick(const WGeo &g, uint32_t c, int &bx, int &by, int &bz) {
  const uint32_t nx = (uint32_t)g.nb[0], ny = (uint32_t)g.nb[1];
  const uint32_t t = c / nx;
  bx = g.b0[0] + (int)(c - t * nx);
  by = g.b0[1] + (int)(t % ny);
  bz = g.b0[2] + (int)(t / ny);
}
// the block's words of brick (bx, by, bz), a lane per (cx, cy), layer cz in w[cz]: every load issued first; a cell of the
// brick outside the block reads as unobserved, and bit cz of `outside` says so
__device__ __forceinline__ void load_block_brick(const Dims &d, const Frame &f, const uint2 *__restrict__ res, const WGeo &g, int bx, int by, int bz,
                                                 uint32_t lane, uint32_t (&w)[8], uint32_t &outside) {
  const int ix = bx * 8 + (int)(lane & 7u) - g.g0[0], iy = by * 8 + (int)(lane >> 3) - g.g0[1], iz0 = bz * 8 - g.g0[2];
  const bool in_xy = (uint32_t)ix < d.NX && (uint32_t)iy < d.NY;
  outside = 0u;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int iz = iz0 + l;
    w[l] = RES_UNKNOWN_W1;
    if (in_xy && (uint32_t)iz < d.NZ) w[l] = res[cell_voxel(d, f, ix, iy, iz)].y;
    else outside |= 1u << l;
  }
}

// ---- classes ------------------------------------------------------------------------------------------------------------
// 0 UNKNOWN, 1 FREE, 2 OCCUPIED: the class of a side's word, the block's and the archive's alike
__device__ __forceinline__ uint32_t side_class(uint32_t w, const WcRule &q) {
  return cell_writes(w, q.wflags, q.max_movable) ? (occ_of(w) >= 1 ? 2u : 1u) : 0u;
}
__device__ __forceinline__ bool admitted(uint32_t label, const WcRule &q) {
  uint32_t mw = 0u;  // (a chain of selects: an index into the by-value words would put them into scratch)
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) mw = (label >> 5) == i ? q.labels[i] : mw;
  return (mw >> (label & 31u)) & 1u;
}
// the labels of a changed cell's two sides as label_now << 8 | label_before << 16, a side that is not occupied reading 0
__device__ __forceinline__ uint32_t label_pair(uint32_t now, uint32_t before, uint32_t cls) {
  const uint32_t ln = cls != SDM_WORLD_CHANGE_VANISHED ? (now >> 16) & 0xffu : 0u, lb = cls != SDM_WORLD_CHANGE_APPEARED ? (before >> 16) & 0xffu : 0u;
  return (ln << 8) | (lb << 16);
}

// ---- the comparison -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wc_mark(Dims d, Frame f, const uint2 *__restrict__ res, WGeo g, const u64 *__restrict__ keys,
                                                const uint32_t *__restrict__ vals, const uint32_t *__restrict__ hdr,
                                                const uint32_t *__restrict__ cells, WcRule q, uint32_t *__restrict__ flag,
                                                uint32_t *__restrict__ cslot, u64 *__restrict__ lw, u64 *__restrict__ p0, u64 *__restrict__ p1,
                                                u64 *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (c == 0u && lane == 0u) flag[g.nc] = 0u;  // the entry behind the last candidate: the scan's total
  if (c >= g.nc) return;                       // (wave-uniform)
  int bx, by, bz;
  candidate_brick(g, c, bx, by, bz);
  uint32_t w[8], a[8], outside;
  load_block_brick(d, f, res, g, bx, by, bz, lane, w, outside);
  uint32_t slot = NONE;
  if (lane == 0u && brick_in_range(bx, by, bz)) {
    slot = world_find(keys, vals, g.hmask, brick_key(bx, by, bz));
    if (slot >= g.max_bricks) slot = NONE;  // (never but for NONE itself)
    if (slot != NONE && q.older && hdr[(size_t)slot * HDR_WORDS + 4] > q.max_last_stamp) slot = NONE;
  }
  slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
  if (slot != NONE) {  // (wave-uniform)
    load_brick(cells, slot, lane, a);
  } else {
#pragma unroll
    for (int l = 0; l < 8; ++l) a[l] = RES_UNKNOWN_W1;
  }
  // every count is a popcount of a ballot, wave-uniform; a brick has 512 cells, so a count fits ten bits and three of them a
  // scalar register (eleven running sums of their own, beside the kernel's arguments by value, spill scalar registers)
  uint32_t pk[(N_COUNTERS + 2) / 3] = {};
  const auto count = [&](uint32_t k, bool is) {
    pk[k / 3u] += (uint32_t)__popcll(__ballot(is)) << (10u * (k % 3u));
    asm volatile("" : "+s"(pk[k / 3u]));  // the sum is due here: left alone, all 88 popcounts sink to the kernel's end and their lane masks spill
  };
  u64 any = 0ull;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const uint32_t sn = side_class(w[l], q), sb = side_class(a[l], q);
    const uint32_t ln = (w[l] >> 16) & 0xffu, lb = (a[l] >> 16) & 0xffu;
    const uint32_t cls = sn == 2u && sb == 1u ? SDM_WORLD_CHANGE_APPEARED
                         : sn == 1u && sb == 2u ? SDM_WORLD_CHANGE_VANISHED
                         : sn == 2u && sb == 2u && ln != lb ? SDM_WORLD_CHANGE_RELABELLED : 0u;
    const bool listed = cls != 0u && ((q.classes >> cls) & 1u) &&
                        ((cls != SDM_WORLD_CHANGE_VANISHED && admitted(ln, q)) || (cls != SDM_WORLD_CHANGE_APPEARED && admitted(lb, q)));
    const u64 lm = __ballot(listed), m0 = __ballot(listed && (cls & 1u)), m1 = __ballot(listed && (cls & 2u));
    any |= lm;
    if (lane == 0u) {
      lw[(size_t)c * 8u + l] = lm;
      p0[(size_t)c * 8u + l] = m0;
      p1[(size_t)c * 8u + l] = m1;
    }
    count(C_APPEARED, cls == SDM_WORLD_CHANGE_APPEARED);
    count(C_VANISHED, cls == SDM_WORLD_CHANGE_VANISHED);
    count(C_RELABELLED, cls == SDM_WORLD_CHANGE_RELABELLED);
    count(C_SAME_OCC, sn == 2u && sb == 2u && ln == lb);
    count(C_SAME_FREE, sn == 1u && sb == 1u);
    count(C_NEW_OCC, sn == 2u && sb == 0u);
    count(C_NEW_FREE, sn == 1u && sb == 0u);
    count(C_REMEMBERED, sn == 0u && sb != 0u);
    count(C_KNOWN_NOW, sn != 0u);
    count(C_KNOWN_BEFORE, sb != 0u);
    count(C_OUTSIDE, (outside >> l) & 1u);
  }
  if (lane == 0u) {
    flag[c] = any ? 1u : 0u;
    cslot[c] = slot;
  }
  uint32_t mine = 0u;  // lane k adds counter k (a chain of selects: the counts are wave-uniform)
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)N_COUNTERS; ++k) mine = lane == k ? (pk[k / 3u] >> (10u * (k % 3u))) & 0x3ffu : mine;
  if (lane < (uint32_t)N_COUNTERS && mine) atomicAdd(meta + G_COUNT + lane * G_SPREAD + (c & (uint32_t)(G_SPREAD - 1)), (u64)mine);
}

// ---- the field ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wc_index(WGeo g, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank,
                                                 const uint32_t *__restrict__ cslot, const u64 *__restrict__ lw, const u64 *__restrict__ p0,
                                                 const u64 *__restrict__ p1, uint32_t n, uint32_t *__restrict__ coord, uint32_t *__restrict__ slot_of,
                                                 u64 *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t hmask, u64 *__restrict__ cw,
                                                 uint32_t *__restrict__ pre, u64 *__restrict__ c0, u64 *__restrict__ c1) {
  const uint32_t c = blockIdx.x * QT + threadIdx.x;
  if (c == 0u) cw[(size_t)n * 8u] = 0ull, pre[(size_t)n * 8u] = 0u;  // the entry behind the last word: the scan's total
  if (c >= g.nc || !flag[c]) return;
  const uint32_t r = rank[c];
  if (r >= n) return;  // (never: n is the scan's total)
  int bx, by, bz;
  candidate_brick(g, c, bx, by, bz);  // (in range: a listed cell has a known archive side)
  coord[2 * (size_t)r] = ((uint32_t)bx & 0xffffu) | (((uint32_t)by & 0xffffu) << 16);
  coord[2 * (size_t)r + 1] = (uint32_t)bz & 0xffffu;
  slot_of[r] = cslot[c];
  world_insert(keys, vals, hmask, brick_key(bx, by, bz), r);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const u64 m = lw[(size_t)c * 8u + l];
    cw[(size_t)r * 8u + l] = m;
    pre[(size_t)r * 8u + l] = (uint32_t)__popcll(m);
    c0[(size_t)r * 8u + l] = p0[(size_t)c * 8u + l];
    c1[(size_t)r * 8u + l] = p1[(size_t)c * 8u + l];
  }
}

// ---- the cell list -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wc_compact(Dims d, Frame f, const uint2 *__restrict__ res, WGeo g, const uint32_t *__restrict__ coord,
                                                   const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ cells,
                                                   const u64 *__restrict__ cw, const uint32_t *__restrict__ pre, const u64 *__restrict__ c0,
                                                   const u64 *__restrict__ c1, uint32_t n, uint32_t n_cells, uint32_t by_label,
                                                   int32_t *__restrict__ xyz, uint32_t *__restrict__ now, uint32_t *__restrict__ before,
                                                   uint8_t *__restrict__ cls_of, uint32_t *__restrict__ key) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform)
  const uint32_t slot = slot_of[r];
  if (slot >= g.max_bricks) return;  // (never: a brick of the field has an archived brick)
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
  uint32_t w[8], a[8], outside;
  load_block_brick(d, f, res, g, bx, by, bz, lane, w, outside);
  load_brick(cells, slot, lane, a);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const size_t wi = (size_t)r * 8u + l;
    const u64 cm = cw[wi];
    if (!((cm >> lane) & 1ull)) continue;
    const uint32_t at = list_index(cw, pre, wi, lane);
    if (at >= n_cells) continue;  // (never: the scan's total is n_cells)
    const uint32_t cls = (uint32_t)((c0[wi] >> lane) & 1ull) | ((uint32_t)((c1[wi] >> lane) & 1ull) << 1);
    store_world_cell(xyz, at, bx, by, bz, lane, l);
    now[at] = w[l];
    before[at] = a[l];
    cls_of[at] = (uint8_t)cls;
    key[at] = by_label ? cls | label_pair(w[l], a[l], cls) : cls;
  }
}

// ---- labels, inside a brick and across the seams ------------------------------------------------------------------------
template <bool FACE>
__global__ __launch_bounds__(QT) void k_wc_label_local(const u64 *__restrict__ cw, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ key,
                                                       uint32_t n, uint32_t n_cells, uint32_t *__restrict__ parent) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform: nothing below waits for another wave)
  u64 cm[8];
  uint32_t k[8], v[8];
  if (!local_labels(cw, r, lane, cm, v)) return;
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    k[z] = NO_KEY;
    if (v[z] != NO_LABEL) {  // (a start label: the cell is listed)
      const uint32_t at = pre[(size_t)r * 8u + z] + lane_rank(cm[z], lane);
      if (at < n_cells) k[z] = key[at];
    }
  }
  sweep_local_labels<FACE>(k, v, lane);
  store_local_roots(v, cm, cw, pre, r, lane, n_cells, parent);
}

template <bool FACE>
__global__ __launch_bounds__(QT) void k_wc_seams(const uint32_t *__restrict__ nbr, const u64 *__restrict__ cw, const uint32_t *__restrict__ pre,
                                                 const uint32_t *__restrict__ key, uint32_t n, uint32_t n_cells, uint32_t *__restrict__ parent) {
  const uint32_t i = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  seam_unions<FACE>(nbr, cw, pre, i >> 3, (int)(i & 7u), threadIdx.x & 63u, n, n_cells, parent, [=](uint32_t c) { return key[c]; });
}

// ---- roots -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wc_roots(const uint32_t *__restrict__ parent, uint32_t n_cells, uint32_t *__restrict__ root,
                                                 uint32_t *__restrict__ idx) {
  for (uint32_t c = blockIdx.x * QT + threadIdx.x; c <= n_cells; c += gridDim.x * QT) {  // (n_cells + 1 entries: the scan's total)
    uint32_t a = c;
    if (c < n_cells) {
      uint32_t p;
      while ((p = parent[a]) < a) a = p;  // (the labelling launches are over: plain loads; strictly downwards)
      root[c] = a;
    }
    idx[c] = c < n_cells && a == c ? 1u : 0u;
  }
}

// ---- accumulators ------------------------------------------------------------------------------------------------------
constexpr int RA_SUMS = 4;  // x y z (signed), n
constexpr int RA_MAX = 6;   // ~code x y z, code x y z
constexpr int RA_FEW = 4;   // up to this many lanes of a wave send a root's cells themselves

__device__ __forceinline__ void send_root(WcAcc *__restrict__ a, const uint32_t (&s)[RA_SUMS], const uint32_t (&mx)[RA_MAX], uint32_t mixed) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (s[i]) atomicAdd(&a->sum[i], (u64)(long long)(int)s[i]);  // (two's complement: the sum is signed)
  atomicAdd(&a->n, s[3]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    atomicMax(&a->nmin[i], mx[i]);
    atomicMax(&a->max[i], mx[3 + i]);
  }
  if (mixed) atomicOr(&a->mixed, 1u);
}

__global__ __launch_bounds__(QT) void k_wc_accumulate(const uint32_t *__restrict__ root, const uint32_t *__restrict__ idx,
                                                      const int32_t *__restrict__ xyz, const uint32_t *__restrict__ now,
                                                      const uint32_t *__restrict__ before, const uint8_t *__restrict__ cls_of, uint32_t n_cells,
                                                      uint32_t n_roots, uint32_t *__restrict__ first, WcAcc *__restrict__ acc) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rounds = (n_cells + gridDim.x * QT - 1) / (gridDim.x * QT);
  for (uint32_t t = 0; t < rounds; ++t) {  // (whole waves: the ballots below see every lane)
    const uint32_t c = (t * gridDim.x + blockIdx.x) * QT + threadIdx.x;
    bool alive = c < n_cells;
    uint32_t o = 0u, s[RA_SUMS] = {}, mx[RA_MAX] = {}, mixed = 0u;
    if (alive) {
      const uint32_t rt = root[c];
      o = idx[rt];  // the root's rank: the region's accumulator
      alive = o < n_roots;  // (always)
      if (rt == c && alive) first[o] = c;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int g = xyz[3 * (size_t)c + i];
        const uint32_t code = (uint32_t)g ^ 0x80000000u;
        s[i] = (uint32_t)g, mx[i] = ~code, mx[3 + i] = code;
      }
      s[3] = 1u;
      mixed = label_pair(now[c], before[c], cls_of[c]) != label_pair(now[rt], before[rt], cls_of[rt]) ? 1u : 0u;
    }
    // per distinct region of the wave one reduction across its lanes and one set of atomics
    for (int turn = 0; turn < 64; ++turn) {
      const u64 todo = __ballot(alive);
      if (!todo) break;
      const uint32_t head = (uint32_t)__builtin_amdgcn_readlane((int)o, __builtin_ctzll(todo));
      const bool mine = alive && o == head;
      alive = alive && !mine;
      if (__popcll(__ballot(mine)) <= RA_FEW) {  // (wave-uniform)
        if (mine) send_root(acc + head, s, mx, mixed);
        continue;
      }
      uint32_t vs[RA_SUMS], vm[RA_MAX], vo = mine ? mixed : 0u;
#pragma unroll
      for (int i = 0; i < RA_SUMS; ++i) vs[i] = wave_sum(mine ? s[i] : 0u);  // (64 coordinates below 2^18 in size: no overflow)
#pragma unroll
      for (int i = 0; i < RA_MAX; ++i) vm[i] = wave_max(mine ? mx[i] : 0u);
      vo = wave_max(vo);
      if (lane == 0) send_root(acc + head, vs, vm, vo);
    }
  }
}

// ---- the table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wc_flags(const WcAcc *__restrict__ acc, uint32_t n_roots, uint32_t min_cells, uint32_t *__restrict__ lidx) {
  const uint32_t o = blockIdx.x * QT + threadIdx.x;
  if (o <= n_roots) lidx[o] = o < n_roots && acc[o].n >= min_cells ? 1u : 0u;  // (n_roots + 1 entries: the scan's total)
}

__global__ __launch_bounds__(QT) void k_wc_table(const uint32_t *__restrict__ first, const uint32_t *__restrict__ lidx,
                                                 const int32_t *__restrict__ xyz, const uint32_t *__restrict__ now,
                                                 const uint32_t *__restrict__ before, const uint8_t *__restrict__ cls_of, uint32_t n_roots,
                                                 float voxel_size, WcAcc *__restrict__ acc, sdm_world_change_region *__restrict__ table,
                                                 u64 *__restrict__ meta) {
  const uint32_t o = blockIdx.x * QT + threadIdx.x;
  if (o == 0u) meta[G_LISTED] = lidx[n_roots];
  if (o >= n_roots) return;
  const WcAcc a = acc[o];
  acc[o] = WcAcc{};
  const uint32_t j = lidx[o];
  if (lidx[o + 1u] == j) return;  // the region's flag: below min_cells
  const uint32_t c = first[o], cls = cls_of[c], pair = label_pair(now[c], before[c], cls);
  sdm_world_change_region e;
  e.first_index = c;
  e.n_cells = a.n;
  e.cls = (uint8_t)cls;
  e.label_now = (uint8_t)((pair >> 8) & 0xffu);
  e.label_before = (uint8_t)((pair >> 16) & 0xffu);
  e.mixed = a.mixed ? 1 : 0;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    const int lo = (int)(~a.nmin[ax] ^ 0x80000000u), hi = (int)(a.max[ax] ^ 0x80000000u);
    const long long sum = (long long)a.sum[ax];
    e.first_cell[ax] = xyz[3 * (size_t)c + ax];
    e.cell_min[ax] = lo;
    e.cell_max[ax] = hi;
    e.cell_sum[ax] = sum;
    e.box_min[ax] = (float)lo * voxel_size;
    e.box_max[ax] = (float)(hi + 1) * voxel_size;
    e.centroid[ax] = (float)(((double)sum / (double)a.n + 0.5) * (double)voxel_size);
  }
  e.pad = 0u;
  table[j] = e;
}

__global__ __launch_bounds__(QT) void k_wc_assign(const uint32_t *__restrict__ root, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ lidx,
                                                  const uint32_t *__restrict__ now, const uint32_t *__restrict__ before,
                                                  const uint8_t *__restrict__ cls_of, uint32_t n_cells, uint32_t n_roots, uint32_t *__restrict__ region,
                                                  u64 *__restrict__ meta) {
  __shared__ uint32_t s_lab[3 * 256];
#pragma unroll
  for (int k = 0; k < 3; ++k) s_lab[k * 256 + threadIdx.x] = 0u;  // (QT == 256)
  __syncthreads();
  for (uint32_t c = blockIdx.x * QT + threadIdx.x; c < n_cells; c += gridDim.x * QT) {
    const uint32_t rt = root[c], o = idx[rt];
    uint32_t j = SDM_WORLD_CHANGE_UNLISTED;
    if (o < n_roots) {  // (always)
      const uint32_t at = lidx[o];
      if (lidx[o + 1u] != at) j = at;
    }
    region[c] = j;
    const uint32_t cls = cls_of[c];
    if (cls >= 1u && cls <= 3u) {  // (always) a vanished cell under the archive's label, the others under the block's
      const uint32_t label = ((cls == SDM_WORLD_CHANGE_VANISHED ? before[c] : now[c]) >> 16) & 0xffu;
      atomicAdd(&s_lab[(cls - 1u) * 256u + label], 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const uint32_t v = s_lab[k * 256 + threadIdx.x];
    if (v) atomicAdd(meta + G_LAB + k * 256 + threadIdx.x, (u64)v);
  }
}
static_assert(QT == 256, "k_wc_assign: a thread per label");

// ---- the query ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_query_world_changes(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n, float recip,
                                                            const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                            uint32_t n_bricks, const u64 *__restrict__ cw, const uint32_t *__restrict__ pre,
                                                            const u64 *__restrict__ c0, const u64 *__restrict__ c1,
                                                            const uint32_t *__restrict__ region, uint32_t n_cells, uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n) return;
  int g[3];
  const bool ok = entry_cell(xyz, cells, i, recip, g);
  const uint32_t r = ok ? world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3)) : NONE;
  uint32_t reg = SDM_WORLD_CHANGE_NONE, index = SDM_WORLD_CHANGE_NONE, cls = SDM_WORLD_CHANGE_NONE;
  if (r < n_bricks) {  // (NONE: in no brick of the field)
    const uint32_t wi = r * 8u + (uint32_t)(g[2] & 7), b = (uint32_t)((g[0] & 7) | ((g[1] & 7) << 3));
    const u64 cm = cw[wi];
    if ((cm >> b) & 1ull) {
      const uint32_t at = list_index(cw, pre, wi, b);
      if (at < n_cells) {
        index = at, reg = region[at];
        cls = (uint32_t)((c0[wi] >> b) & 1ull) | ((uint32_t)((c1[wi] >> b) & 1ull) << 1);
      }
    }
  }
  uint2 *__restrict__ o = out + 3 * (size_t)i;
  o[0] = make_uint2((uint32_t)g[0], (uint32_t)g[1]);
  o[1] = make_uint2((uint32_t)g[2], reg);
  o[2] = make_uint2(index, cls);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
uint32_t candidates_max(const Dims &d) { return (((d.NX + 7) >> 3) + 1) * (((d.NY + 7) >> 3) + 1) * (((d.NZ + 7) >> 3) + 1); }

// sdm_world_update's geometry (world.hip's geo_of), the layer's flags standing for the archive's
WGeo geo_of(const sdm_map *m) {
  const Dims &d = m->d;
  const WorldLayer &W = m->world;
  const int N[3] = {(int)d.NX, (int)d.NY, (int)d.NZ};
  WGeo g;
  for (int a = 0; a < 3; ++a) {
    g.g0[a] = m->moved_steps[a] - (N[a] >> 1);
    g.b0[a] = g.g0[a] >> 3;
    g.nb[a] = ((g.g0[a] + N[a] - 1) >> 3) - g.b0[a] + 1;
  }
  g.nc = (uint32_t)(g.nb[0] * g.nb[1] * g.nb[2]);
  g.nc_max = candidates_max(d);
  g.flags = 0u;
  g.gts = m->f.gts;
  g.max_bricks = W.max_bricks;
  g.hmask = W.hmask;
  g.max_movable = d.max_movable;
  return g;
}

// the buffers for `cand` candidates / `bricks` bricks of the field / `cells` cells / `regions` regions (the stream is idle
// if there were buffers before)
sdm_status grow_cand(sdm_map *m, size_t cand) {
  WorldChangesLayer &L = m->wchg;
  const size_t cap = round_up(cand + 1, 256);
  return grow_buffers(m, cand + 1, cap, &L.cap_cand,
                      {buf(&L.flag, cap), buf(&L.rank, cap), buf(&L.cslot, cap), buf(&L.lw_c, cap * 8), buf(&L.p0_c, cap * 8), buf(&L.p1_c, cap * 8)});
}

sdm_status grow_bricks(sdm_map *m, size_t bricks) {  // (no brick: still a table to look up in)
  WorldChangesLayer &L = m->wchg;
  const size_t need = std::max<size_t>(bricks, 1), cap = round_up(need, 256);
  return grow_buffers(m, need, cap, &L.cap_bricks,
                      {buf(&L.coord, cap * 2), buf(&L.slot_of, cap), buf(&L.nbr, cap * 27), buf(&L.cw, cap * 8 + 1), buf(&L.pre, cap * 8 + 1),
                       buf(&L.c0, cap * 8), buf(&L.c1, cap * 8), buf(&L.keys, table_slots(cap)), buf(&L.vals, table_slots(cap))});
}

sdm_status grow_cells(sdm_map *m, size_t cells) {
  WorldChangesLayer &L = m->wchg;
  const size_t cap = round_up(cells, 4096);
  return grow_buffers(m, cells, cap, &L.cap_cells,
                      {buf(&L.xyz, cap * 3), buf(&L.now, cap), buf(&L.before, cap), buf(&L.key, cap), buf(&L.cls, cap), buf(&L.parent, cap),
                       buf(&L.root, cap), buf(&L.idx, cap + 1)});
}

sdm_status grow_regions(sdm_map *m, size_t regions) {
  WorldChangesLayer &L = m->wchg;
  const size_t cap = round_up(regions, 1024);
  return grow_buffers(m, regions, cap, &L.cap_regions,
                      {buf(&L.acc, cap * sizeof(WcAcc)), buf(&L.first, cap), buf(&L.lidx, cap + 1), buf(&L.table, cap)}, [&]() -> sdm_status {
                        HIP_TRY(hipMemsetAsync(L.acc, 0, cap * sizeof(WcAcc), m->stream));  // empty; every build leaves them empty again
                        return SDM_OK;
                      });
}

WcRule rule_of(const sdm_map *m, const sdm_world_changes_options *o) {
  WcRule q{};
  for (int i = 0; i < 8; ++i) q.labels[i] = o->labels[i];
  q.wflags = ((o->flags & SDM_WORLD_CHANGES_STATIC_ONLY) ? SDM_WORLD_STATIC_ONLY : 0u) |
             ((o->flags & SDM_WORLD_CHANGES_OBSERVED_ONLY) ? SDM_WORLD_OBSERVED_ONLY : 0u);
  q.classes = o->classes;
  q.older = (o->flags & SDM_WORLD_CHANGES_OLDER) ? 1u : 0u;
  q.max_last_stamp = o->max_last_stamp;
  q.by_label = (o->flags & SDM_WORLD_CHANGES_BY_LABEL) ? 1u : 0u;
  q.max_movable = m->d.max_movable;
  return q;
}

// the field: its coordinates, the layer's table, the neighbours, the listed words with their counts and planes
hipError_t launch_wc_field(const sdm_map *m, const WGeo &g, uint32_t n) {
  const WorldChangesLayer &L = m->wchg;
  hipStream_t s = m->stream;
  hipError_t e;
  if ((e = hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  LAYER_LAUNCH(k_wc_index, (g.nc + QT - 1) / QT, QT, s, g, L.flag, L.rank, L.cslot, L.lw_c, L.p0_c, L.p1_c, n, L.coord, L.slot_of, L.keys, L.vals,
               L.hmask, L.cw, L.pre, L.c0, L.c1);
  return launch_snapshot_neighbours(L.coord, L.keys, L.vals, L.hmask, n, L.nbr, s);
}

// from the cell list to the root flags
hipError_t launch_wc_labels(const sdm_map *m, const Frame &f, const WGeo &g, uint32_t n, uint32_t n_cells, bool face, uint32_t by_label) {
  const WorldChangesLayer &L = m->wchg;
  hipStream_t s = m->stream;
  const uint32_t by_word = (n * 8u + QT / 64 - 1) / (QT / 64), by_brick = (n + QT / 64 - 1) / (QT / 64);
  const uint32_t by_cell = std::min<uint32_t>(n_cells / QT + 1, WC_GRID);
  LAYER_LAUNCH(k_wc_compact, by_brick, QT, s, m->d, f, reinterpret_cast<const uint2 *>(m->st.res), g, L.coord, L.slot_of, m->world.cells, L.cw, L.pre,
               L.c0, L.c1, n, n_cells, by_label, L.xyz, L.now, L.before, L.cls, L.key);
  if (face) {
    LAYER_LAUNCH(k_wc_label_local<true>, by_brick, QT, s, L.cw, L.pre, L.key, n, n_cells, L.parent);
    LAYER_LAUNCH(k_wc_seams<true>, by_word, QT, s, L.nbr, L.cw, L.pre, L.key, n, n_cells, L.parent);
  } else {
    LAYER_LAUNCH(k_wc_label_local<false>, by_brick, QT, s, L.cw, L.pre, L.key, n, n_cells, L.parent);
    LAYER_LAUNCH(k_wc_seams<false>, by_word, QT, s, L.nbr, L.cw, L.pre, L.key, n, n_cells, L.parent);
  }
  LAYER_LAUNCH(k_wc_roots, by_cell, QT, s, L.parent, n_cells, L.root, L.idx);
  return hipSuccess;
}

// from the ranked roots to the table, the cells' region indices and the per-label counters
hipError_t launch_wc_table(const sdm_map *m, uint32_t n_cells, uint32_t n_roots, uint32_t min_cells, uint32_t *scan) {
  const WorldChangesLayer &L = m->wchg;
  hipStream_t s = m->stream;
  const uint32_t by_cell = std::min<uint32_t>(n_cells / QT + 1, WC_GRID), by_region = n_roots / QT + 1;
  hipError_t e;
  LAYER_LAUNCH(k_wc_accumulate, by_cell, QT, s, L.root, L.idx, L.xyz, L.now, L.before, L.cls, n_cells, n_roots, L.first, reinterpret_cast<WcAcc *>(L.acc));
  LAYER_LAUNCH(k_wc_flags, by_region, QT, s, reinterpret_cast<const WcAcc *>(L.acc), n_roots, min_cells, L.lidx);
  exclusive_scan_u32(L.lidx, L.lidx, (size_t)n_roots + 1, scan, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wc_table, by_region, QT, s, L.first, L.lidx, L.xyz, L.now, L.before, L.cls, n_roots, m->d.voxel_size, reinterpret_cast<WcAcc *>(L.acc),
               L.table, L.meta);
  LAYER_LAUNCH(k_wc_assign, by_cell, QT, s, L.root, L.idx, L.lidx, L.now, L.before, L.cls, n_cells, n_roots, L.parent, L.meta);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_CHANGES = {"the world changes", "world changes", "sdm_world_changes_update", true};

void fill_info(const WorldChangesLayer &L, sdm_world_changes_info *info) {
  const u64 *h = L.h_meta;  // (the build waited for them)
  uint64_t *counter = &info->n_appeared;
  for (int k = 0; k < N_COUNTERS; ++k) {
    counter[k] = 0;
    for (int j = 0; j < G_SPREAD; ++j) counter[k] += (uint64_t)h[G_COUNT + k * G_SPREAD + j];
  }
  info->n_candidates = L.n_candidates;
  info->n_bricks = L.n;
  info->n_cells = L.n_cells;
  info->n_regions = (uint32_t)h[G_LISTED];
  info->n_regions_total = L.n_roots;
  info->flags = L.flags;
  info->min_cells = L.min_cells;
  info->frame_stamp = L.frame_stamp;
  info->stamp = L.stamp;
}

sdm_status refuse_over(const WorldChangesLayer &L, const char *what) {
  char msg[200];
  std::snprintf(msg, sizeof(msg), "%lld listed world cells, max_cells is %lld: call sdm_world_changes_update with a larger max_cells (or 0)",
                (long long)L.n_cells, (long long)L.max_cells);
  set_error(what, __FILE__, __LINE__, msg);
  return SDM_ERR_CAPACITY;
}
}  // namespace

extern "C" {

sdm_status sdm_world_changes_update(sdm_map *m, const sdm_world_changes_options *o) {
  const char *what = "sdm_world_changes_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WC_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->classes & ~ALL_CLASSES) return LAYER_REFUSE(what, "unknown class bits");
  if (o->pad[0] || o->pad[1]) return LAYER_REFUSE(what, "non-zero pad");
  if (o->max_cells < 0) return LAYER_REFUSE(what, "max_cells < 0");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldChangesLayer &L = m->wchg;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, G_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, G_WORDS + 1, true));
  const Frame f = m->f;
  const WGeo g = geo_of(m);
  const WcRule rule = rule_of(m, o);
  const uint2 *res = reinterpret_cast<const uint2 *>(m->st.res);
  if (g.nc_max + 1 > L.cap_cand && L.cap_cand) HIP_TRY(hipStreamSynchronize(s));  // (never: a map has one largest candidate count)
  SDM_TRY(grow_cand(m, g.nc_max));
  uint32_t *scan = nullptr;
  SDM_TRY(layer_scan_scratch(m, (size_t)g.nc_max * 8 + 1, &scan));
  HIP_TRY(hipMemsetAsync(L.meta, 0, G_WORDS * sizeof(u64), s));
  // the comparison: counters, listed words, the flags of the candidates with a listed cell - and how many those are
  hipLaunchKernelGGL(k_wc_mark, dim3((g.nc + QT / 64 - 1) / (QT / 64)), dim3(QT), 0, s, m->d, f, res, g, m->world.keys, m->world.vals, m->world.hdr,
                     m->world.cells, rule, L.flag, L.cslot, L.lw_c, L.p0_c, L.p1_c, L.meta);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, G_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
  uint32_t n = 0;
  SDM_TRY(snapshot_rank(m, L.flag, L.rank, g.nc, scan, L.h_meta + G_WORDS, &n));
  SDM_TRY(grow_bricks(m, n));
  L.hmask = table_slots(n) - 1;
  HIP_TRY(launch_wc_field(m, g, n));
  if (n) {
    exclusive_scan_u32(L.pre, L.pre, (size_t)n * 8 + 1, scan, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.h_meta + G_WORDS, L.pre + (size_t)n * 8, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  const uint32_t n_cells = n ? (uint32_t)L.h_meta[G_WORDS] : 0u;
  L.n = n;
  L.n_candidates = g.nc;
  L.n_cells = (int64_t)n_cells;
  L.n_roots = 0;
  L.max_cells = o->max_cells;
  L.min_cells = o->min_cells;
  L.frame_stamp = f.gts;
  L.stamp = m->world.f.gts;
  L.over = o->max_cells > 0 && (int64_t)n_cells > o->max_cells;
  if (L.over) {  // nothing is written past the cap, nothing is truncated: the getters say so too
    L.built(f, o->flags);
    return refuse_over(L, what);
  }
  if (n_cells) {
    SDM_TRY(grow_cells(m, n_cells));
    SDM_TRY(layer_scan_scratch(m, std::max<size_t>((size_t)g.nc_max * 8, n_cells) + 1, &scan));
    HIP_TRY(launch_wc_labels(m, f, g, n, n_cells, (o->flags & SDM_WORLD_CHANGES_FACE_CONNECTED) != 0, rule.by_label));
    exclusive_scan_u32(L.idx, L.idx, (size_t)n_cells + 1, scan, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.h_meta + G_WORDS, L.idx + (size_t)n_cells, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t n_roots = (uint32_t)L.h_meta[G_WORDS];  // the regions in all: they size accumulators and table
    SDM_TRY(grow_regions(m, n_roots));
    HIP_TRY(launch_wc_table(m, n_cells, n_roots, (uint32_t)std::max<int32_t>(o->min_cells, 1), scan));
    HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, G_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    L.n_roots = n_roots;
  }
  L.built(f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_changes(sdm_map *m, sdm_world_change_region *out, int32_t cap, int32_t *n_out, sdm_world_changes_info *info) {
  const char *what = "sdm_get_world_changes";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out || (cap > 0 && !out)) return LAYER_REFUSE(what, "cap < 0, no n_out, or no regions for cap > 0");
  SDM_TRY(layer_check(m, what, &m->wchg, WORLD_CHANGES));
  const WorldChangesLayer &L = m->wchg;
  if (info) fill_info(L, info);
  if (L.over) return refuse_over(L, what);
  const uint32_t n = (uint32_t)L.h_meta[G_LISTED];
  const size_t take = std::min<size_t>(n, (size_t)cap);
  if (take) {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(out, L.table, take * sizeof(sdm_world_change_region), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  *n_out = (int32_t)n;
  return SDM_OK;
}

sdm_status sdm_get_world_change_cells(sdm_map *m, int32_t *cell_xyz, uint32_t *now, uint32_t *before, uint8_t *cls, uint32_t *region, int64_t first,
                                      int64_t cap, int64_t *n_out) {
  const char *what = "sdm_get_world_change_cells";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wchg, WORLD_CHANGES));
  const WorldChangesLayer &L = m->wchg;
  *n_out = L.n_cells;
  if (L.over) return refuse_over(L, what);
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>(L.n_cells - first, cap), 0);
  if (take && (cell_xyz || now || before || cls || region)) {
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    if (cell_xyz) HIP_TRY(hipMemcpyAsync(cell_xyz, L.xyz + 3 * (size_t)first, take * 12, hipMemcpyDeviceToHost, s));
    if (now) HIP_TRY(hipMemcpyAsync(now, L.now + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (before) HIP_TRY(hipMemcpyAsync(before, L.before + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (cls) HIP_TRY(hipMemcpyAsync(cls, L.cls + (size_t)first, take, hipMemcpyDeviceToHost, s));
    if (region) HIP_TRY(hipMemcpyAsync(region, L.parent + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return SDM_OK;
}

sdm_status sdm_get_world_change_labels(sdm_map *m, uint64_t appeared[256], uint64_t vanished[256], uint64_t relabelled[256]) {
  const char *what = "sdm_get_world_change_labels";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, what, &m->wchg, WORLD_CHANGES));
  const WorldChangesLayer &L = m->wchg;
  if (L.over) return refuse_over(L, what);
  const u64 *h = L.h_meta;  // (the build waited for them)
  uint64_t *out[3] = {appeared, vanished, relabelled};
  for (int k = 0; k < 3; ++k)
    if (out[k])
      for (int l = 0; l < 256; ++l) out[k][l] = (uint64_t)h[G_LAB + k * 256 + l];
  return SDM_OK;
}

sdm_status sdm_query_world_changes(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_change_result *out, uint32_t flags) {
  const char *what = "sdm_query_world_changes";
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, what, &sdm_map::wchg, WORLD_CHANGES));
  const WorldChangesLayer L = m->wchg;
  if (L.over) return refuse_over(L, what);
  const float recip = m->d.recip;
  const bool points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, 12, out, sizeof(sdm_world_change_result), nullptr, 0, n, flags,
                   [L, recip, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_world_changes, dim3((c + QT - 1) / QT), dim3(QT), 0, s, points ? static_cast<const float *>(in) : nullptr,
                                        points ? nullptr : static_cast<const int32_t *>(in), c, recip, L.keys, L.vals, L.hmask, L.n, L.cw, L.pre, L.c0,
                                        L.c1, L.parent, (uint32_t)L.n_cells, static_cast<uint2 *>(o));
                   });
}

}  // extern "C"
