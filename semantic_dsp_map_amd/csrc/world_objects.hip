// world_objects.hip — world objects: the connected components of occupied archived cells that carry the same key (the
// label, or label and track), across brick borders, a table of them with counts, boxes and first and second moments, per-label
// counters and a query from a point or a cell to its object (gfx950; include/sdm.h, "world objects").
//
// A brick is 8 x 8 x 8 cells, a layer of it one 64-bit word (bit cx + 8 cy).  The build is a snapshot: what it leaves are the
// field's coordinates, a hash table of its own from brick key to rank, the counted words with their prefix, the lists and the
// table; no pool slot.  Everything it accumulates is an integer sum, minimum, maximum or OR, and a component's root is its
// smallest list index whatever order the unions arrive in: two builds give the same bytes.
//   snapshot_bricks, launch_snapshot_index   world_snapshot.hip's: the bricks of the box flagged and ranked, their
//               coordinates and pool slots at their rank, key -> rank in the layer's table.
//   launch_snapshot_neighbours   world_snapshot.hip's k_ws_neighbours: a thread per (brick of the field, one of 27): one
//               lookup in the layer's table, the neighbour's rank or NONE.  brick_in_range before every lookup.
//   k_wo_classify    a wave per field brick, a lane per (cx, cy), the eight layers' loads first: a ballot a layer writes the
//               counted word (occ >= 1, the flags, the label mask) and its popcount, a second one counts occ == 2.
//               exclusive_scan_u32 over the 8 n + 1 popcounts gives every word's first list index and the cell count.
//   k_wo_compact     a wave per field brick: world cell and archived word at prefix + popcount of the lower bits.
//   k_wo_label_local a wave per brick, a lane per (cx, cy), the eight keys and eight labels of its column in registers.  The
//               keys never change, so who may join whom is settled ONCE: per cell a mask of its 26 (6) neighbours inside the
//               brick that are counted and carry an equal key - the z neighbours from the lane's own registers, the others
//               by lane shuffles of the keys, 8 (4) directions x 8 layers.  A sweep then shuffles labels only, 64 (32)
//               shuffles, and a cell takes a neighbour's label where its mask allows: explicit comparisons against every
//               neighbour, no separable minimum - that would carry a label through a cell of another key, or, masked per
//               stage, miss two cells that touch only at an edge or a corner.  A lane at the brick's border names itself as
//               the source and masks the result: bit 7 + 8 cy and bit 8 (cy + 1) never meet.  Until a sweep changes
//               nothing (at most 512 sweeps).  parent[] of a cell becomes the list index of its local component's smallest
//               cell: no LDS, no global atomic.
//   k_wo_seams       a wave per word, a lane per cell: a counted cell on the brick's shell looks at its 26 (6) neighbours
//               that lie in a field brick of lower rank and unites with those that are counted and carry an equal key:
//               sdm_world.h's seam_unions over its min-linking union-find, which world_frontiers.hip runs with one key for
//               all.  Every read of parent[] in this launch is an agent-scope atomic load or an atomic's return value.
//               Lock-free: a failed link hands the loop a strictly smaller root.
//   k_wo_roots       a thread per cell: follows parent[] to the root (plain loads: a later launch), writes root[] and the
//               root flag; exclusive_scan_u32 over n + 1 flags ranks the roots and counts them - the build's third wait,
//               after which accumulators and table are sized by objects, not by cells.
//   k_wo_accumulate  a thread per cell: adds the cell to its root's accumulator - counts, signed sums, the six products of
//               d = cell - first cell, the box as maxima of order-preserving codes, mixed_tracks as an OR - after a
//               reduction across the lanes of the wave that share a root.
//   k_wo_flags + exclusive_scan_u32   1 per object with n_cells >= min_cells, scanned over objects + 1 entries.
//   k_wo_table       a thread per object: a listed one writes its table entry; every one stores zeros back into its
//               accumulator, so the next build starts from empty accumulators.
//   k_wo_assign      a thread per cell: its object index; the per-label counters - cells, and objects from the roots -
//               reduced per workgroup in LDS before the atomics.
//   k_query_world_objects   a thread per entry: its cell, the layer's own table -> rank, the bit of the counted word,
//               index = prefix + popcount of the lower bits, object[index]; three 8-byte stores.
// The build waits three times: for the number of bricks of the field, for the number of cells, for the number of objects.
// This unit includes no code of a frame unit and defines every kernel it launches but those of world_snapshot.hip; the
// opening and the end of the local labelling, the seam body, the union-find, the offset tables and the brick loads are
// sdm_world.h's, shared with world_frontiers.hip; the keyed sweep between the two ends is sdm_world.h's
// sweep_local_labels, shared with world_changes.hip (5y; 5v says why it differs from the frontiers').
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_objects_options) == 72 && sizeof(sdm_world_object) == 168 && sizeof(sdm_world_objects_info) == 40 &&
                  sizeof(sdm_world_object_result) == 24,
              "sdm.h layout");
static_assert(offsetof(sdm_world_objects_options, max_cells) == 8 && offsetof(sdm_world_objects_options, labels) == 16 &&
                  offsetof(sdm_world_objects_options, bmin) == 48 && offsetof(sdm_world_object, track) == 12 &&
                  offsetof(sdm_world_object, first_cell) == 16 && offsetof(sdm_world_object, cell_sum) == 56 &&
                  offsetof(sdm_world_object, cell_sq) == 80 && offsetof(sdm_world_object, box_min) == 128 && offsetof(sdm_world_object, pad1) == 164 &&
                  offsetof(sdm_world_objects_info, n_cells) == 16 && offsetof(sdm_world_objects_info, min_cells) == 32 &&
                  offsetof(sdm_world_object_result, object) == 12,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;             // the kernels of a thread or a wave per item
constexpr uint32_t WO_GRID = 4096;  // the largest grid of the kernels over cells: they stride
constexpr uint32_t ALL_WO_FLAGS = SDM_WORLD_OBJECTS_FACE_CONNECTED | SDM_WORLD_OBJECTS_BOX | SDM_WORLD_OBJECTS_BY_TRACK |
                                  SDM_WORLD_OBJECTS_STATIC_ONLY | SDM_WORLD_OBJECTS_MOVABLE_ONLY | SDM_WORLD_OBJECTS_OBSERVED_ONLY;
// the build's counters, 64 bits each: the guessed cells in G_SPREAD copies (a wave adds to copy rank & 63, the getter sums
// them), the objects listed, per label the cells, per label the objects (32 bits each, two a word)
enum { G_GUESSED = 0, G_SPREAD = 64, G_LISTED = G_SPREAD, G_LAB_CELLS, G_LAB_OBJS = G_LAB_CELLS + 256, G_WORDS = G_LAB_OBJS + 128 };

struct WoAcc {  // per object; all zero = no cell yet.  nmin / max: the largest ~code / code, code = coordinate ^ 2^31
  u64 sum[3], sq[6];
  uint32_t n, guessed, nmin[3], max[3], mixed, pad;
};
struct WoRule {  // which cells count, by value
  uint32_t labels[8];
  uint32_t static_only, movable_only, observed_only, by_track;
  int max_movable;
};
static_assert(sizeof(WoAcc) == 112, "bytes per object in sdm.h");
constexpr size_t ARCH_BYTES = 4 + 4;                                            // flag, rank
constexpr size_t BRICK_BYTES = 8 + 4 + 27 * 4 + 8 * 8 + 8 * 4 + 2 * (8 + 4);    // coord, slot, nbr, counted words, prefix, two hash slots
constexpr size_t CELL_BYTES = 12 + 4 + 3 * 4 + 0;                               // xyz, word; parent, root, idx
constexpr size_t OBJECT_BYTES = sizeof(WoAcc) + sizeof(sdm_world_object) + 4 + 4;  // first, lidx
static_assert(ARCH_BYTES == SDM_WORLD_OBJECTS_BYTES_PER_ARCHIVED_BRICK && BRICK_BYTES == SDM_WORLD_OBJECTS_BYTES_PER_BRICK &&
                  CELL_BYTES == SDM_WORLD_OBJECTS_BYTES_PER_CELL && OBJECT_BYTES == SDM_WORLD_OBJECTS_BYTES_PER_OBJECT &&
                  (2 * G_WORDS + 1) * 8 == 7192,
              "sdm.h states the bytes");

__device__ __forceinline__ uint32_t key_of(uint32_t w, uint32_t by_track) { return by_track ? (w & 0xffffffu) : ((w >> 16) & 0xffu); }

__device__ __forceinline__ bool counts(uint32_t w, const WoRule &q) {
  const int occ = occ_of(w);
  const uint32_t track = w & 0xffffu, label = (w >> 16) & 0xffu;
  const bool movable = track >= 1u && (int)track <= q.max_movable;
  uint32_t mw = 0u;  // (a chain of selects: an index into the by-value words would put them into scratch)
#pragma unroll
  for (uint32_t i = 0; i < 8u; ++i) mw = (label >> 5) == i ? q.labels[i] : mw;
  return occ >= 1 && ((mw >> (label & 31u)) & 1u) && !(q.static_only && movable) && !(q.movable_only && !movable) &&
         !(q.observed_only && occ == 2);
}

// ---- counted words -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wo_classify(const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ cells, uint32_t n,
                                                    uint32_t max_bricks, WoRule rule, u64 *__restrict__ cw, uint32_t *__restrict__ cnt,
                                                    u64 *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform)
  if (r == 0u && lane == 0u) cw[(size_t)n * 8u] = 0ull, cnt[(size_t)n * 8u] = 0u;  // the entry behind the last word: the scan's total
  const uint32_t slot = slot_of[r];
  if (slot >= max_bricks) return;  // (never: the pool has max_bricks slots; wave-uniform)
  uint32_t w[8];
  load_brick(cells, slot, lane, w);
  uint32_t guessed = 0u;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const bool c = counts(w[l], rule);
    const u64 cm = __ballot(c), gm = __ballot(c && occ_of(w[l]) == 2);
    guessed += (uint32_t)__popcll(gm);
    if (lane == 0) {
      cw[(size_t)r * 8u + l] = cm;
      cnt[(size_t)r * 8u + l] = (uint32_t)__popcll(cm);
    }
  }
  if (lane == 0 && guessed) atomicAdd(meta + G_GUESSED + (r & (uint32_t)(G_SPREAD - 1)), (u64)guessed);
}

// ---- the cell list -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wo_compact(const uint32_t *__restrict__ coord, const uint32_t *__restrict__ slot_of,
                                                   const uint32_t *__restrict__ cells, const u64 *__restrict__ cw, const uint32_t *__restrict__ pre,
                                                   uint32_t n, uint32_t max_bricks, uint32_t n_cells, int32_t *__restrict__ xyz,
                                                   uint32_t *__restrict__ word) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform)
  const uint32_t slot = slot_of[r];
  if (slot >= max_bricks) return;  // (never)
  uint32_t w[8];
  load_brick(cells, slot, lane, w);
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const u64 cm = cw[(size_t)r * 8u + l];
    if (!((cm >> lane) & 1ull)) continue;
    const uint32_t at = list_index(cw, pre, (size_t)r * 8u + l, lane);
    if (at >= n_cells) continue;  // (never: the scan's total is n_cells)
    store_world_cell(xyz, at, bx, by, bz, lane, l);
    word[at] = w[l];
  }
}

// ---- labels, inside a brick --------------------------------------------------------------------------------------------
template <bool FACE>
__global__ __launch_bounds__(QT) void k_wo_label_local(const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ cells,
                                                       const u64 *__restrict__ cw, const uint32_t *__restrict__ pre, uint32_t n, uint32_t max_bricks,
                                                       uint32_t n_cells, uint32_t by_track, uint32_t *__restrict__ parent) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform: nothing below waits for another wave)
  u64 cm[8];
  uint32_t k[8], v[8];
  if (!local_labels(cw, r, lane, cm, v)) return;
  const uint32_t slot = slot_of[r];
  if (slot >= max_bricks) return;  // (never)
  load_brick(cells, slot, lane, k);
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    k[z] = v[z] != NO_LABEL ? key_of(k[z], by_track) : NO_KEY;  // (a start label: the cell is counted)
  }
  sweep_local_labels<FACE>(k, v, lane);
  store_local_roots(v, cm, cw, pre, r, lane, n_cells, parent);
}

// ---- labels, across the seams -------------------------------------------------------------------------------------------
template <bool FACE>
__global__ __launch_bounds__(QT) void k_wo_seams(const uint32_t *__restrict__ nbr, const u64 *__restrict__ cw, const uint32_t *__restrict__ pre,
                                                 const uint32_t *__restrict__ word, uint32_t n, uint32_t n_cells, uint32_t by_track,
                                                 uint32_t *__restrict__ parent) {
  const uint32_t i = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  seam_unions<FACE>(nbr, cw, pre, i >> 3, (int)(i & 7u), threadIdx.x & 63u, n, n_cells, parent,
                    [=](uint32_t c) { return key_of(word[c], by_track); });
}

// ---- roots -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wo_roots(const uint32_t *__restrict__ parent, uint32_t n_cells, uint32_t *__restrict__ root,
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
constexpr int OA_SUMS = 5;  // x y z (signed), n, guessed
constexpr int OA_MAX = 6;   // ~code x y z, code x y z
constexpr int OA_FEW = 4;   // up to this many lanes of a wave send a root's cells themselves

__device__ __forceinline__ void send_root(WoAcc *__restrict__ a, const uint32_t (&s)[OA_SUMS], const u64 (&q)[6], const uint32_t (&mx)[OA_MAX],
                                          uint32_t mixed) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (s[i]) atomicAdd(&a->sum[i], (u64)(long long)(int)s[i]);  // (two's complement: the sum is signed)
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (q[i]) atomicAdd(&a->sq[i], q[i]);
  atomicAdd(&a->n, s[3]);
  if (s[4]) atomicAdd(&a->guessed, s[4]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    atomicMax(&a->nmin[i], mx[i]);
    atomicMax(&a->max[i], mx[3 + i]);
  }
  if (mixed) atomicOr(&a->mixed, 1u);
}

__global__ __launch_bounds__(QT) void k_wo_accumulate(const uint32_t *__restrict__ root, const uint32_t *__restrict__ idx,
                                                      const int32_t *__restrict__ xyz, const uint32_t *__restrict__ word, uint32_t n_cells,
                                                      uint32_t n_roots, uint32_t *__restrict__ first, WoAcc *__restrict__ acc) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rounds = (n_cells + gridDim.x * QT - 1) / (gridDim.x * QT);
  for (uint32_t t = 0; t < rounds; ++t) {  // (whole waves: the ballots below see every lane)
    const uint32_t c = (t * gridDim.x + blockIdx.x) * QT + threadIdx.x;
    bool alive = c < n_cells;
    uint32_t o = 0u, s[OA_SUMS] = {}, mx[OA_MAX] = {}, mixed = 0u;
    u64 q[6] = {};
    if (alive) {
      const uint32_t rt = root[c];
      o = idx[rt];  // the root's rank: the object's accumulator
      alive = o < n_roots;  // (always)
      if (rt == c && alive) first[o] = c;
      long long d[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int g = xyz[3 * (size_t)c + i];
        const uint32_t code = (uint32_t)g ^ 0x80000000u;
        s[i] = (uint32_t)g, mx[i] = ~code, mx[3 + i] = code;
        d[i] = (long long)g - (long long)xyz[3 * (size_t)rt + i];
      }
      const uint32_t w = word[c];
      s[3] = 1u, s[4] = occ_of(w) == 2 ? 1u : 0u;
      mixed = ((w ^ word[rt]) & 0xffffu) ? 1u : 0u;
      q[0] = (u64)(d[0] * d[0]), q[1] = (u64)(d[1] * d[1]), q[2] = (u64)(d[2] * d[2]);
      q[3] = (u64)(d[0] * d[1]), q[4] = (u64)(d[0] * d[2]), q[5] = (u64)(d[1] * d[2]);
    }
    // per distinct object of the wave one reduction across its lanes and one set of atomics
    for (int turn = 0; turn < 64; ++turn) {
      const u64 todo = __ballot(alive);
      if (!todo) break;
      const uint32_t head = (uint32_t)__builtin_amdgcn_readlane((int)o, __builtin_ctzll(todo));
      const bool mine = alive && o == head;
      alive = alive && !mine;
      if (__popcll(__ballot(mine)) <= OA_FEW) {  // (wave-uniform)
        if (mine) send_root(acc + head, s, q, mx, mixed);
        continue;
      }
      uint32_t vs[OA_SUMS], vm[OA_MAX], vo = mine ? mixed : 0u;
      u64 vq[6];
#pragma unroll
      for (int i = 0; i < OA_SUMS; ++i) vs[i] = mine ? s[i] : 0u;
#pragma unroll
      for (int i = 0; i < OA_MAX; ++i) vm[i] = mine ? mx[i] : 0u;
#pragma unroll
      for (int i = 0; i < 6; ++i) vq[i] = wave_sum64(mine ? q[i] : 0ull);
#pragma unroll
      for (int i = 0; i < OA_SUMS; ++i) vs[i] = wave_sum(vs[i]);  // (64 coordinates below 2^18 in size: no overflow)
#pragma unroll
      for (int i = 0; i < OA_MAX; ++i) vm[i] = wave_max(vm[i]);
      vo = wave_max(vo);
      if (lane == 0) send_root(acc + head, vs, vq, vm, vo);
    }
  }
}

// ---- the table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wo_flags(const WoAcc *__restrict__ acc, uint32_t n_roots, uint32_t min_cells, uint32_t *__restrict__ lidx) {
  const uint32_t o = blockIdx.x * QT + threadIdx.x;
  if (o <= n_roots) lidx[o] = o < n_roots && acc[o].n >= min_cells ? 1u : 0u;  // (n_roots + 1 entries: the scan's total)
}

__global__ __launch_bounds__(QT) void k_wo_table(const uint32_t *__restrict__ first, const uint32_t *__restrict__ lidx,
                                                 const int32_t *__restrict__ xyz, const uint32_t *__restrict__ word, uint32_t n_roots,
                                                 float voxel_size, WoAcc *__restrict__ acc, sdm_world_object *__restrict__ table,
                                                 u64 *__restrict__ meta) {
  const uint32_t o = blockIdx.x * QT + threadIdx.x;
  if (o == 0u) meta[G_LISTED] = lidx[n_roots];
  if (o >= n_roots) return;
  const WoAcc a = acc[o];
  acc[o] = WoAcc{};
  const uint32_t j = lidx[o];
  if (lidx[o + 1u] == j) return;  // the object's flag: below min_cells
  const uint32_t c = first[o], w = word[c];
  sdm_world_object e;
  e.first_index = c;
  e.n_cells = a.n;
  e.n_guessed = a.guessed;
  e.track = (uint16_t)(w & 0xffffu);
  e.label = (uint8_t)((w >> 16) & 0xffu);
  e.mixed_tracks = a.mixed ? 1 : 0;
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
#pragma unroll
  for (int i = 0; i < 6; ++i) e.cell_sq[i] = (long long)a.sq[i];
  e.pad0 = 0u;
  e.pad1 = 0u;
  table[j] = e;
}

__global__ __launch_bounds__(QT) void k_wo_assign(const uint32_t *__restrict__ root, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ lidx,
                                                  const uint32_t *__restrict__ word, uint32_t n_cells, uint32_t n_roots, uint32_t *__restrict__ object,
                                                  u64 *__restrict__ meta) {
  __shared__ uint32_t s_cells[256], s_objs[256];
  s_cells[threadIdx.x] = 0u, s_objs[threadIdx.x] = 0u;  // (QT == 256)
  __syncthreads();
  for (uint32_t c = blockIdx.x * QT + threadIdx.x; c < n_cells; c += gridDim.x * QT) {
    const uint32_t rt = root[c], o = idx[rt];
    uint32_t j = SDM_WORLD_OBJECT_UNLISTED;
    if (o < n_roots) {  // (always)
      const uint32_t at = lidx[o];
      if (lidx[o + 1u] != at) j = at;
    }
    object[c] = j;
    const uint32_t label = (word[c] >> 16) & 0xffu;
    atomicAdd(&s_cells[label], 1u);
    if (rt == c) atomicAdd(&s_objs[label], 1u);
  }
  __syncthreads();
  const uint32_t nc = s_cells[threadIdx.x], no = s_objs[threadIdx.x];
  if (nc) atomicAdd(meta + G_LAB_CELLS + threadIdx.x, (u64)nc);
  if (no) atomicAdd(reinterpret_cast<uint32_t *>(meta + G_LAB_OBJS) + threadIdx.x, no);
}
static_assert(QT == 256, "k_wo_assign: a thread per label");

// ---- the query ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_query_world_objects(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n, float recip,
                                                            const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                            uint32_t n_bricks, const u64 *__restrict__ cw, const uint32_t *__restrict__ pre,
                                                            const uint32_t *__restrict__ object, uint32_t n_cells, uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n) return;
  int g[3];
  const bool ok = entry_cell(xyz, cells, i, recip, g);
  const uint32_t r = ok ? world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3)) : NONE;
  uint32_t obj = SDM_WORLD_OBJECT_NONE, index = SDM_WORLD_OBJECT_NONE;
  if (r < n_bricks) {  // (NONE: in no brick of the field)
    const uint32_t wi = r * 8u + (uint32_t)(g[2] & 7), b = (uint32_t)((g[0] & 7) | ((g[1] & 7) << 3));
    const u64 cm = cw[wi];
    if ((cm >> b) & 1ull) {
      const uint32_t at = list_index(cw, pre, wi, b);
      if (at < n_cells) index = at, obj = object[at];
    }
  }
  uint2 *__restrict__ o = out + 3 * (size_t)i;
  o[0] = make_uint2((uint32_t)g[0], (uint32_t)g[1]);
  o[1] = make_uint2((uint32_t)g[2], obj);
  o[2] = make_uint2(index, 0u);
}

// the buffers for n_arch archived bricks / `bricks` bricks of the field / `cells` cells / `objects` objects (the stream is
// idle if there were buffers before)
sdm_status grow_arch(sdm_map *m, size_t n_arch) {
  WorldObjectsLayer &L = m->wobj;
  const size_t cap = round_up(n_arch + 1, 256);
  return grow_buffers(m, n_arch + 1, cap, &L.cap_arch, {buf(&L.flag, cap), buf(&L.rank, cap)});
}

sdm_status grow_bricks(sdm_map *m, size_t bricks) {  // (no brick: still a table to look up in)
  WorldObjectsLayer &L = m->wobj;
  const size_t need = std::max<size_t>(bricks, 1), cap = round_up(need, 256);
  return grow_buffers(m, need, cap, &L.cap_bricks,
                      {buf(&L.coord, cap * 2), buf(&L.slot_of, cap), buf(&L.nbr, cap * 27), buf(&L.cw, cap * 8 + 1), buf(&L.pre, cap * 8 + 1),
                       buf(&L.keys, table_slots(cap)), buf(&L.vals, table_slots(cap))});
}

sdm_status grow_cells(sdm_map *m, size_t cells) {
  WorldObjectsLayer &L = m->wobj;
  const size_t cap = round_up(cells, 4096);
  return grow_buffers(m, cells, cap, &L.cap_cells,
                      {buf(&L.xyz, cap * 3), buf(&L.word, cap), buf(&L.parent, cap), buf(&L.root, cap), buf(&L.idx, cap + 1)});
}

sdm_status grow_objects(sdm_map *m, size_t objects) {
  WorldObjectsLayer &L = m->wobj;
  const size_t cap = round_up(objects, 1024);
  return grow_buffers(m, objects, cap, &L.cap_objects,
                      {buf(&L.acc, cap * sizeof(WoAcc)), buf(&L.first, cap), buf(&L.lidx, cap + 1), buf(&L.table, cap)}, [&]() -> sdm_status {
                        HIP_TRY(hipMemsetAsync(L.acc, 0, cap * sizeof(WoAcc), m->stream));  // empty; every build leaves them empty again
                        return SDM_OK;
                      });
}

WoRule rule_of(const sdm_map *m, const sdm_world_objects_options *o) {
  WoRule q{};
  for (int i = 0; i < 8; ++i) q.labels[i] = o->labels[i];
  q.static_only = (o->flags & SDM_WORLD_OBJECTS_STATIC_ONLY) ? 1u : 0u;
  q.movable_only = (o->flags & SDM_WORLD_OBJECTS_MOVABLE_ONLY) ? 1u : 0u;
  q.observed_only = (o->flags & SDM_WORLD_OBJECTS_OBSERVED_ONLY) ? 1u : 0u;
  q.by_track = (o->flags & SDM_WORLD_OBJECTS_BY_TRACK) ? 1u : 0u;
  q.max_movable = m->d.max_movable;
  return q;
}

// the index, the neighbours, the counted words and their counts
hipError_t launch_wo_words(const sdm_map *m, const uint32_t *order, uint32_t n_arch, uint32_t n, const WoRule &rule) {
  const WorldObjectsLayer &L = m->wobj;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  hipError_t e;
  if ((e = hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  if ((e = launch_snapshot_index(m, order, L.flag, L.rank, n_arch, n, L.coord, L.slot_of, L.keys, L.vals, L.hmask)) != hipSuccess) return e;
  if ((e = launch_snapshot_neighbours(L.coord, L.keys, L.vals, L.hmask, n, L.nbr, s)) != hipSuccess) return e;
  LAYER_LAUNCH(k_wo_classify, (n + QT / 64 - 1) / (QT / 64), QT, s, L.slot_of, W.cells, n, W.max_bricks, rule, L.cw, L.pre, L.meta);
  return hipSuccess;
}

// from the cell list to the root flags
hipError_t launch_wo_labels(const sdm_map *m, uint32_t n, uint32_t n_cells, bool face, uint32_t by_track) {
  const WorldObjectsLayer &L = m->wobj;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  const uint32_t by_word = (n * 8u + QT / 64 - 1) / (QT / 64), by_brick = (n + QT / 64 - 1) / (QT / 64);
  const uint32_t by_cell = std::min<uint32_t>(n_cells / QT + 1, WO_GRID);
  LAYER_LAUNCH(k_wo_compact, by_brick, QT, s, L.coord, L.slot_of, W.cells, L.cw, L.pre, n, W.max_bricks, n_cells, L.xyz, L.word);
  if (face) {
    LAYER_LAUNCH(k_wo_label_local<true>, by_brick, QT, s, L.slot_of, W.cells, L.cw, L.pre, n, W.max_bricks, n_cells, by_track, L.parent);
    LAYER_LAUNCH(k_wo_seams<true>, by_word, QT, s, L.nbr, L.cw, L.pre, L.word, n, n_cells, by_track, L.parent);
  } else {
    LAYER_LAUNCH(k_wo_label_local<false>, by_brick, QT, s, L.slot_of, W.cells, L.cw, L.pre, n, W.max_bricks, n_cells, by_track, L.parent);
    LAYER_LAUNCH(k_wo_seams<false>, by_word, QT, s, L.nbr, L.cw, L.pre, L.word, n, n_cells, by_track, L.parent);
  }
  LAYER_LAUNCH(k_wo_roots, by_cell, QT, s, L.parent, n_cells, L.root, L.idx);
  return hipSuccess;
}

// from the ranked roots to the table, the cells' object indices and the per-label counters
hipError_t launch_wo_table(const sdm_map *m, uint32_t n_cells, uint32_t n_roots, uint32_t min_cells, uint32_t *scan) {
  const WorldObjectsLayer &L = m->wobj;
  hipStream_t s = m->stream;
  const uint32_t by_cell = std::min<uint32_t>(n_cells / QT + 1, WO_GRID), by_object = n_roots / QT + 1;
  hipError_t e;
  LAYER_LAUNCH(k_wo_accumulate, by_cell, QT, s, L.root, L.idx, L.xyz, L.word, n_cells, n_roots, L.first, reinterpret_cast<WoAcc *>(L.acc));
  LAYER_LAUNCH(k_wo_flags, by_object, QT, s, reinterpret_cast<const WoAcc *>(L.acc), n_roots, min_cells, L.lidx);
  exclusive_scan_u32(L.lidx, L.lidx, (size_t)n_roots + 1, scan, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wo_table, by_object, QT, s, L.first, L.lidx, L.xyz, L.word, n_roots, m->d.voxel_size, reinterpret_cast<WoAcc *>(L.acc), L.table, L.meta);
  LAYER_LAUNCH(k_wo_assign, by_cell, QT, s, L.root, L.idx, L.lidx, L.word, n_cells, n_roots, L.parent, L.meta);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_OBJECTS = {"the world objects", "world objects", "sdm_world_objects_update", true};

void fill_info(const WorldObjectsLayer &L, sdm_world_objects_info *info) {
  const u64 *h = L.h_meta;  // (the build waited for them)
  info->n_bricks = L.n;
  info->n_objects = (uint32_t)h[G_LISTED];
  info->n_objects_total = L.n_roots;
  info->flags = L.flags;
  info->n_cells = L.n_cells;
  info->n_guessed = 0;
  for (int k = 0; k < G_SPREAD; ++k) info->n_guessed += (int64_t)h[G_GUESSED + k];
  info->min_cells = L.min_cells;
  info->stamp = L.stamp;
}

sdm_status refuse_over(const WorldObjectsLayer &L, const char *what) {
  char msg[200];
  std::snprintf(msg, sizeof(msg), "%lld counted world cells, max_cells is %lld: call sdm_world_objects_update with a larger max_cells (or 0)",
                (long long)L.n_cells, (long long)L.max_cells);
  set_error(what, __FILE__, __LINE__, msg);
  return SDM_ERR_CAPACITY;
}
}  // namespace

extern "C" {

sdm_status sdm_world_objects_update(sdm_map *m, const sdm_world_objects_options *o) {
  const char *what = "sdm_world_objects_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WO_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if ((o->flags & SDM_WORLD_OBJECTS_STATIC_ONLY) && (o->flags & SDM_WORLD_OBJECTS_MOVABLE_ONLY))
    return LAYER_REFUSE(what, "STATIC_ONLY and MOVABLE_ONLY together: no cell could count");
  if (o->max_cells < 0) return LAYER_REFUSE(what, "max_cells < 0");
  BrickBox box{};
  if (o->flags & SDM_WORLD_OBJECTS_BOX) {  // (bmax < bmin: an empty box, a field of no bricks)
    box.use = 1u;
    for (int a = 0; a < 3; ++a) box.lo[a] = o->bmin[a], box.hi[a] = o->bmax[a];
  }
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldObjectsLayer &L = m->wobj;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, G_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, G_WORDS + 1, true));
  HIP_TRY(hipMemsetAsync(L.meta, 0, G_WORDS * sizeof(u64), s));
  // the bricks of the field: the archive's in brick order, those of the box ranked
  SnapshotBricks b;
  SDM_TRY(snapshot_bricks(m, box, (size_t)m->world.max_bricks * 8 + 1, L.h_meta + G_WORDS, [&](uint32_t n_arch, uint32_t **flag, uint32_t **rank) -> sdm_status {
    HIP_TRY(hipStreamSynchronize(s));
    SDM_TRY(grow_arch(m, n_arch));
    *flag = L.flag, *rank = L.rank;
    return SDM_OK;
  }, &b));
  const uint32_t n = b.n;
  uint32_t *scan = b.scan;
  HIP_TRY(hipStreamSynchronize(s));
  SDM_TRY(grow_bricks(m, n));
  L.hmask = table_slots(n) - 1;
  // the counted words, and how many cells they hold
  const WoRule rule = rule_of(m, o);
  HIP_TRY(launch_wo_words(m, b.order, b.n_arch, n, rule));
  if (n) {
    exclusive_scan_u32(L.pre, L.pre, (size_t)n * 8 + 1, scan, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.h_meta + G_WORDS, L.pre + (size_t)n * 8, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, G_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint32_t n_cells = n ? (uint32_t)L.h_meta[G_WORDS] : 0u;
  L.n = n;
  L.n_cells = (int64_t)n_cells;
  L.n_roots = 0;
  L.max_cells = o->max_cells;
  L.min_cells = o->min_cells;
  L.stamp = m->world.f.gts;
  L.over = o->max_cells > 0 && (int64_t)n_cells > o->max_cells;
  if (L.over) {  // nothing is written past the cap, nothing is truncated: the getters say so too
    L.built(m->world.f, o->flags);
    return refuse_over(L, what);
  }
  if (n_cells) {
    SDM_TRY(grow_cells(m, n_cells));
    SDM_TRY(layer_scan_scratch(m, std::max<size_t>((size_t)m->world.max_bricks * 8, n_cells) + 1, &scan));
    HIP_TRY(launch_wo_labels(m, n, n_cells, (o->flags & SDM_WORLD_OBJECTS_FACE_CONNECTED) != 0, rule.by_track));
    exclusive_scan_u32(L.idx, L.idx, (size_t)n_cells + 1, scan, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.h_meta + G_WORDS, L.idx + (size_t)n_cells, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t n_roots = (uint32_t)L.h_meta[G_WORDS];  // the objects in all: they size accumulators and table
    SDM_TRY(grow_objects(m, n_roots));
    HIP_TRY(launch_wo_table(m, n_cells, n_roots, (uint32_t)std::max<int32_t>(o->min_cells, 1), scan));
    HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, G_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    L.n_roots = n_roots;
  }
  L.built(m->world.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_objects(sdm_map *m, sdm_world_object *out, int32_t cap, int32_t *n_out, sdm_world_objects_info *info) {
  const char *what = "sdm_get_world_objects";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out || (cap > 0 && !out)) return LAYER_REFUSE(what, "cap < 0, no n_out, or no out for cap > 0");
  SDM_TRY(layer_check(m, what, &m->wobj, WORLD_OBJECTS));
  const WorldObjectsLayer &L = m->wobj;
  if (info) fill_info(L, info);
  if (L.over) return refuse_over(L, what);
  const uint32_t n = (uint32_t)L.h_meta[G_LISTED];
  const size_t take = std::min<size_t>(n, (size_t)cap);
  if (take) {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(out, L.table, take * sizeof(sdm_world_object), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  *n_out = (int32_t)n;
  return SDM_OK;
}

sdm_status sdm_get_world_object_cells(sdm_map *m, int32_t *cell_xyz, uint32_t *object, uint32_t *words, int64_t first, int64_t cap,
                                      int64_t *n_out) {
  const char *what = "sdm_get_world_object_cells";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wobj, WORLD_OBJECTS));
  const WorldObjectsLayer &L = m->wobj;
  *n_out = L.n_cells;
  if (L.over) return refuse_over(L, what);
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>(L.n_cells - first, cap), 0);
  if (take && (cell_xyz || object || words)) {
    HIP_TRY(hipSetDevice(m->device));
    if (cell_xyz) HIP_TRY(hipMemcpyAsync(cell_xyz, L.xyz + 3 * (size_t)first, take * 12, hipMemcpyDeviceToHost, m->stream));
    if (object) HIP_TRY(hipMemcpyAsync(object, L.parent + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    if (words) HIP_TRY(hipMemcpyAsync(words, L.word + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return SDM_OK;
}

sdm_status sdm_get_world_object_labels(sdm_map *m, uint64_t cells[256], uint32_t objects[256]) {
  const char *what = "sdm_get_world_object_labels";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, what, &m->wobj, WORLD_OBJECTS));
  const WorldObjectsLayer &L = m->wobj;
  if (L.over) return refuse_over(L, what);
  const u64 *h = L.h_meta;  // (the build waited for them)
  if (cells)
    for (int l = 0; l < 256; ++l) cells[l] = (uint64_t)h[G_LAB_CELLS + l];
  if (objects) memcpy(objects, h + G_LAB_OBJS, 256 * sizeof(uint32_t));
  return SDM_OK;
}

sdm_status sdm_query_world_objects(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_object_result *out, uint32_t flags) {
  const char *what = "sdm_query_world_objects";
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, what, &sdm_map::wobj, WORLD_OBJECTS));
  const WorldObjectsLayer L = m->wobj;
  if (L.over) return refuse_over(L, what);
  const float recip = m->d.recip;
  const bool points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, 12, out, sizeof(sdm_world_object_result), nullptr, 0, n, flags,
                   [L, recip, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_world_objects, dim3((c + QT - 1) / QT), dim3(QT), 0, s, points ? static_cast<const float *>(in) : nullptr,
                                        points ? nullptr : static_cast<const int32_t *>(in), c, recip, L.keys, L.vals, L.hmask, L.n, L.cw, L.pre,
                                        L.parent, (uint32_t)L.n_cells, static_cast<uint2 *>(o));
                   });
}

}  // extern "C"
