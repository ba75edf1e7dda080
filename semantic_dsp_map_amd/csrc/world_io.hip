// world_io.hip — the world archive's way back in and its trim (gfx950; include/sdm.h, "world archive": sdm_world_import,
// sdm_world_retain).  The table, the pool, the capacity rule and the closing kernel are world.hip's (sdm_world.h).
//
// An import merges n foreign bricks - headers and 512 words each, as sdm_get_world_bricks returns them - under a cell
// offset: q = offset >> 3 and r = offset & 7 per axis.  A source brick s touches the destination bricks s + q + e, e in
// {0, 1} on the axes with r != 0; cell c of destination brick d comes from cell (c - r) & 7 of source brick
// d - q - (c < r), so up to 8 sources meet in one destination.
//   k_wio_src_insert  a thread per source: its key into a transient table (CAS), its index beside it (atomicMin): of
//                 sources with the same coordinates the lowest index stays, whatever the arrival order.
//   k_wio_owners      a thread per pair (s, e) of a source that stayed: the pair owns its destination iff no source exists
//                 at d - q - e' for a combination e' before e - so every distinct destination is flagged exactly once.
//   exclusive_scan_u32, k_wio_compact   the owners, compacted, with the low sort key (bx, by) of their destination.
//   radix_sort_pairs 32 bits, k_wio_key_hi, radix_sort_pairs 16 bits   ... into brick order, like the pool's own order.
//   k_wio_mark        a wave per destination, a lane per (cx, cy), eight layers: lanes 0 .. 7 look the 8 sources up, every
//                 load of the incoming words is issued first; counts the cells that write, looks the resident brick up,
//                 flags "needs creating".  Lookups only.
//   exclusive_scan_u32   ranks the flags.
//   k_wio_merge       a wave per destination with a writing cell: room by rank exactly as in k_world_merge; a fresh brick
//                 is written whole, an archived one has its written cells replaced; counts by ballot, stamps min / max over
//                 the sources that wrote.
//   launch_world_finish   world.hip's closing kernel: n_bricks, created_last, dropped_total.
// The atomics are the CAS, the atomicMin and counters: all commute.  Every probe loop ends after one round of its table.
//
// A retain flags the bricks to keep, ranks them, packs them into a transient copy, empties the table, and copies them back
// to the front of the pool in their previous relative order, reinserting every key (moving inside the pool would let one
// wave overwrite what another has not read yet).
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_import_options) == 24 && offsetof(sdm_world_import_options, cell_offset) == 4 &&
                  offsetof(sdm_world_import_options, max_bricks) == 16 && sizeof(sdm_world_retain_options) == 32 &&
                  offsetof(sdm_world_retain_options, bmax) == 12 && offsetof(sdm_world_retain_options, min_last_stamp) == 24,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr uint32_t IMPORT_FLAGS = ALL_FLAGS | SDM_WORLD_IMPORT_FILL | SDM_WORLD_IMPORT_ON_DEVICE;
constexpr int64_t MAX_SOURCES = (int64_t)1 << 21;
constexpr int MAX_OFFSET = 1 << 19;

struct IoGeo {       // an import's geometry, by value
  int q[3], r[3];    // cell_offset >> 3, cell_offset & 7
  uint32_t n;        // source bricks
  uint32_t ne;       // destinations per source: 2^(axes with r != 0)
  uint32_t cap;      // n * ne: what the candidate arrays, the scans and the sorts are sized for
  uint32_t smask;    // the source table's slots - 1
  uint32_t flags, max_bricks, hmask;
  int max_movable;
};

__device__ __forceinline__ void source_brick(const uint32_t *__restrict__ src_hdr, uint32_t i, int (&s)[3]) {
  const uint32_t h0 = src_hdr[(size_t)i * HDR_WORDS], h1 = src_hdr[(size_t)i * HDR_WORDS + 1];
  s[0] = (int16_t)(h0 & 0xffffu), s[1] = (int16_t)(h0 >> 16), s[2] = (int16_t)(h1 & 0xffffu);
}
// the k-th combination e: bit b of k goes to the b-th axis with r != 0
__device__ __forceinline__ void combination(const IoGeo &g, uint32_t k, int (&e)[3]) {
  uint32_t b = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e[a] = 0;
    if (g.r[a]) e[a] = (int)((k >> b++) & 1u);
  }
}
// the destination brick of pair t = source * ne + combination
__device__ __forceinline__ void pair_brick(const IoGeo &g, const uint32_t *__restrict__ src_hdr, uint32_t t, int (&d)[3]) {
  const uint32_t i = t / g.ne;
  int s[3], e[3];
  source_brick(src_hdr, i, s);
  combination(g, t - i * g.ne, e);
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = s[a] + g.q[a] + e[a];
}

// ---- the import ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WTPB) void k_wio_src_insert(IoGeo g, const uint32_t *__restrict__ src_hdr, u64 *__restrict__ skeys,
                                                         uint32_t *__restrict__ svals) {
  const uint32_t i = blockIdx.x * WTPB + threadIdx.x;
  if (i >= g.n) return;
  int s[3];
  source_brick(src_hdr, i, s);
  const u64 key = brick_key(s[0], s[1], s[2]);
  uint32_t h = key_hash(key) & g.smask;
  for (uint32_t t = 0; t <= g.smask; ++t) {
    const u64 old = atomicCAS(skeys + h, EMPTY_KEY, key);
    if (old == EMPTY_KEY || old == key) {
      atomicMin(svals + h, i);  // (the slots start at all ones)
      return;
    }
    h = (h + 1u) & g.smask;
  }
}

__global__ __launch_bounds__(WTPB) void k_wio_owners(IoGeo g, const uint32_t *__restrict__ src_hdr, const u64 *__restrict__ skeys,
                                                     const uint32_t *__restrict__ svals, uint32_t *__restrict__ own) {
  const uint32_t t = blockIdx.x * WTPB + threadIdx.x;
  if (t > g.cap) return;
  if (t == g.cap) {
    own[t] = 0u;  // the scan's extra entry: the number of destinations lands there
    return;
  }
  const uint32_t i = t / g.ne, k = t - i * g.ne;
  int s[3], e[3];
  source_brick(src_hdr, i, s);
  combination(g, k, e);
  bool mine = world_find(skeys, svals, g.smask, brick_key(s[0], s[1], s[2])) == i;  // (a later source of the same brick is ignored)
  for (uint32_t k2 = 0; mine && k2 < k; ++k2) {
    int e2[3];
    combination(g, k2, e2);
    const int x = s[0] + e[0] - e2[0], y = s[1] + e[1] - e2[1], z = s[2] + e[2] - e2[2];
    if (brick_in_range(x, y, z) && world_find(skeys, svals, g.smask, brick_key(x, y, z)) != NONE) mine = false;
  }
  own[t] = mine ? 1u : 0u;
}

// a destination beyond the coordinate range is never created: its place in the order does not matter
__global__ __launch_bounds__(WTPB) void k_wio_compact(IoGeo g, const uint32_t *__restrict__ src_hdr, const uint32_t *__restrict__ own,
                                                      const uint32_t *__restrict__ pos, uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  const uint32_t t = blockIdx.x * WTPB + threadIdx.x;
  if (t >= g.cap || !own[t]) return;
  int d[3];
  pair_brick(g, src_hdr, t, d);
  const uint32_t j = pos[t];
  key[j] = brick_in_range(d[0], d[1], d[2]) ? (uint32_t)(d[0] + 32768) | ((uint32_t)(d[1] + 32768) << 16) : 0u;
  val[j] = t;
}
// the second pass's keys: bz + 32768 of the destinations in the order the first pass left
__global__ __launch_bounds__(WTPB) void k_wio_key_hi(IoGeo g, const uint32_t *__restrict__ src_hdr, const uint32_t *__restrict__ count,
                                                     uint32_t *__restrict__ key, const uint32_t *__restrict__ val) {
  const uint32_t j = blockIdx.x * WTPB + threadIdx.x;
  if (j >= g.cap || j >= count[0]) return;
  int d[3];
  pair_brick(g, src_hdr, val[j], d);
  key[j] = brick_in_range(d[0], d[1], d[2]) ? (uint32_t)(d[2] + 32768) : 0u;
}

// What arrives in destination brick d, a lane per (cx, cy), layer cz in w[cz], every load issued first: lanes 0 .. 7 look
// up the source d - q - e' of e' = (lane & 1, lane >> 1 & 1, lane >> 2) - `src`, NONE where there is none -, a cell takes
// the word of the source its own e' = (c < r) names (which[cz]), unknown where that source is missing.
__device__ __forceinline__ void load_incoming(const IoGeo &g, const int (&d)[3], uint32_t lane, const u64 *__restrict__ skeys,
                                              const uint32_t *__restrict__ svals, const uint32_t *__restrict__ src_cells, uint32_t &src,
                                              uint32_t (&w)[8], uint32_t (&which)[8]) {
  src = NONE;
  if (lane < 8u) {
    const int e[3] = {(int)(lane & 1u), (int)((lane >> 1) & 1u), (int)(lane >> 2)};
    const int x = d[0] - g.q[0] - e[0], y = d[1] - g.q[1] - e[1], z = d[2] - g.q[2] - e[2];
    const bool used = (!e[0] || g.r[0]) && (!e[1] || g.r[1]) && (!e[2] || g.r[2]);
    if (used && brick_in_range(x, y, z)) src = world_find(skeys, svals, g.smask, brick_key(x, y, z));
  }
  const int cx = (int)(lane & 7u), cy = (int)(lane >> 3);
  const uint32_t exy = (cx < g.r[0] ? 1u : 0u) | (cy < g.r[1] ? 2u : 0u);
  const uint32_t s_lo = (uint32_t)__shfl((int)src, (int)exy, 64), s_hi = (uint32_t)__shfl((int)src, (int)(exy | 4u), 64);
  const uint32_t cxy = (uint32_t)((cx - g.r[0]) & 7) | ((uint32_t)((cy - g.r[1]) & 7) << 3);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const bool up = l < g.r[2];
    const uint32_t from = up ? s_hi : s_lo;
    which[l] = exy | (up ? 4u : 0u);
    w[l] = RES_UNKNOWN_W1;
    if (from != NONE) w[l] = src_cells[(size_t)from * 512u + (cxy | ((uint32_t)((l - g.r[2]) & 7) << 6))];
  }
}
__device__ __forceinline__ bool incoming_writes(const IoGeo &g, uint32_t w, uint32_t old) {
  return cell_writes(w, g.flags, g.max_movable) && (!(g.flags & SDM_WORLD_IMPORT_FILL) || occ_of(old) < 0);
}

__global__ __launch_bounds__(WTPB) void k_wio_mark(IoGeo g, const uint32_t *__restrict__ src_hdr, const uint32_t *__restrict__ src_cells,
                                                   const u64 *__restrict__ skeys, const uint32_t *__restrict__ svals,
                                                   const uint32_t *__restrict__ count, const uint32_t *__restrict__ cand,
                                                   const u64 *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                   const uint32_t *__restrict__ cells, uint32_t *__restrict__ need, uint32_t *__restrict__ cslot,
                                                   uint32_t *__restrict__ cnw, uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (j >= g.cap || j >= count[0]) return;  // (wave-uniform; need[] beyond the count was zeroed by the host)
  int d[3];
  pair_brick(g, src_hdr, cand[j], d);
  const bool in_range = brick_in_range(d[0], d[1], d[2]);
  const uint32_t slot = in_range ? world_find(keys, vals, g.hmask, brick_key(d[0], d[1], d[2])) : NONE;  // (one address per wave)
  uint32_t src, w[8], which[8], old[8];
  load_incoming(g, d, lane, skeys, svals, src_cells, src, w, which);
  const bool look = (g.flags & SDM_WORLD_IMPORT_FILL) && slot != NONE;
#pragma unroll
  for (int l = 0; l < 8; ++l) old[l] = look ? cells[(size_t)slot * 512u + (uint32_t)l * 64u + lane] : RES_UNKNOWN_W1;
  uint32_t nw = 0;
#pragma unroll
  for (int l = 0; l < 8; ++l) nw += (uint32_t)__popcll(__ballot(incoming_writes(g, w[l], old[l])));
  if (lane != 0u) return;
  uint32_t create = 0u;
  if (nw) {
    if (in_range) {
      create = slot == NONE ? 1u : 0u;
    } else {
      nw = 0u;  // never created: its cells write nothing
      atomicAdd(meta + M_OOR, 1u);
    }
  }
  need[j] = create;
  cslot[j] = slot;
  cnw[j] = nw;
}

__global__ __launch_bounds__(WTPB) void k_wio_merge(IoGeo g, const uint32_t *__restrict__ src_hdr, const uint32_t *__restrict__ src_cells,
                                                    const u64 *__restrict__ skeys, const uint32_t *__restrict__ svals,
                                                    const uint32_t *__restrict__ count, const uint32_t *__restrict__ cand, u64 *__restrict__ keys,
                                                    uint32_t *__restrict__ vals, const uint32_t *__restrict__ need,
                                                    const uint32_t *__restrict__ rank, const uint32_t *__restrict__ cslot,
                                                    const uint32_t *__restrict__ cnw, uint32_t *__restrict__ cells, uint32_t *__restrict__ hdr,
                                                    uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (j >= g.cap || j >= count[0]) return;  // (wave-uniform, like every return below)
  const uint32_t nw = cnw[j];
  if (!nw) return;
  const bool fresh = need[j] != 0u;
  const uint32_t slot = fresh ? meta[M_N_BRICKS] + rank[j] : cslot[j];
  if (slot >= g.max_bricks) {  // a new brick without room: its cells are dropped
    if (lane == 0u) atomicAdd(meta + M_DROPPED, nw);
    return;
  }
  int d[3];
  pair_brick(g, src_hdr, cand[j], d);
  uint32_t src, w[8], which[8], old[8];
  load_incoming(g, d, lane, skeys, svals, src_cells, src, w, which);
  uint32_t *__restrict__ mine = cells + (size_t)slot * 512u + lane;
#pragma unroll
  for (int l = 0; l < 8; ++l) old[l] = fresh ? RES_UNKNOWN_W1 : mine[l * 64];
  uint32_t n_occ = 0, n_free = 0, wrote = 0;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const bool wr = incoming_writes(g, w[l], old[l]);
    const uint32_t v = wr ? w[l] : old[l];
    if (wr || fresh) mine[l * 64] = v;
    if (wr) wrote |= 1u << which[l];
    const int occ = occ_of(v);
    n_occ += (uint32_t)__popcll(__ballot(occ >= 1));
    n_free += (uint32_t)__popcll(__ballot(occ == 0));
  }
  // the sources that wrote here: their stamps sit with lanes 0 .. 7
  wrote = wave_all(wrote, [](uint32_t a, uint32_t b) { return a | b; });
  const bool gave = lane < 8u && src != NONE && ((wrote >> lane) & 1u);
  uint32_t first = 0xffffffffu, last = 0u;
  if (gave) first = src_hdr[(size_t)src * HDR_WORDS + 3], last = src_hdr[(size_t)src * HDR_WORDS + 4];
  first = wave_min(first), last = wave_max(last);
  if (lane != 0u) return;
  if (fresh) world_insert(keys, vals, g.hmask, brick_key(d[0], d[1], d[2]), slot);
  uint32_t *__restrict__ h = hdr + (size_t)slot * HDR_WORDS;
  if (!fresh) first = min(first, h[3]), last = max(last, h[4]);
  h[0] = ((uint32_t)d[0] & 0xffffu) | (((uint32_t)d[1] & 0xffffu) << 16);
  h[1] = ((uint32_t)d[2] & 0xffffu) | (n_occ << 16);
  h[2] = n_free;
  h[3] = first;
  h[4] = last;
}

// ---- the retain ---------------------------------------------------------------------------------------------------
struct KeepBox {
  int lo[3], hi[3];
  uint32_t min_last;
};
__global__ __launch_bounds__(WTPB) void k_wio_keep(KeepBox b, uint32_t n, const uint32_t *__restrict__ hdr, uint32_t *__restrict__ keep) {
  const uint32_t i = blockIdx.x * WTPB + threadIdx.x;
  if (i > n) return;
  uint32_t k = 0u;
  if (i < n) {  // (entry n: the scan's extra one, where the number of kept bricks lands)
    int s[3];
    source_brick(hdr, i, s);
    k = s[0] >= b.lo[0] && s[0] <= b.hi[0] && s[1] >= b.lo[1] && s[1] <= b.hi[1] && s[2] >= b.lo[2] && s[2] <= b.hi[2] &&
                hdr[(size_t)i * HDR_WORDS + 4] >= b.min_last
            ? 1u
            : 0u;
  }
  keep[i] = k;
}
// a wave per brick: header and cells of `from` brick a to `to` brick b
__device__ __forceinline__ void copy_brick(const uint32_t *__restrict__ from_hdr, const uint32_t *__restrict__ from_cells, uint32_t a,
                                           uint32_t *__restrict__ to_hdr, uint32_t *__restrict__ to_cells, uint32_t b, uint32_t lane) {
  uint32_t w[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) w[l] = from_cells[(size_t)a * 512u + (uint32_t)l * 64u + lane];
  if (lane < HDR_WORDS) to_hdr[(size_t)b * HDR_WORDS + lane] = from_hdr[(size_t)a * HDR_WORDS + lane];
#pragma unroll
  for (int l = 0; l < 8; ++l) to_cells[(size_t)b * 512u + (uint32_t)l * 64u + lane] = w[l];
}
__global__ __launch_bounds__(WTPB) void k_wio_pack(uint32_t n, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                                                   const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ cells,
                                                   uint32_t *__restrict__ t_hdr, uint32_t *__restrict__ t_cells) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (i >= n || !keep[i]) return;
  copy_brick(hdr, cells, i, t_hdr, t_cells, pos[i], lane);
}
// ... back to the front of the pool (the table was emptied before this launch); n_bricks becomes the kept count
__global__ __launch_bounds__(WTPB) void k_wio_unpack(uint32_t n, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ t_hdr,
                                                     const uint32_t *__restrict__ t_cells, uint32_t *__restrict__ hdr, uint32_t *__restrict__ cells,
                                                     u64 *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t hmask, uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  const uint32_t k = kept[0];
  if (j == 0u && lane == 0u) meta[M_N_BRICKS] = k;
  if (j >= n || j >= k) return;
  copy_brick(t_hdr, t_cells, j, hdr, cells, j, lane);
  if (lane != 0u) return;
  int s[3];
  source_brick(t_hdr, j, s);
  world_insert(keys, vals, hmask, brick_key(s[0], s[1], s[2]), j);
}

// ---- host ------------------------------------------------------------------------------------------------------------
// the import's work arrays inside WorldLayer::io, in words
struct IoLayout {
  size_t skeys, svals, own, pos, sortbuf, need, rank, cslot, cnw, sort, total;
  IoLayout(size_t slots, size_t cap) {
    size_t at = 0;
    auto take = [&at](size_t words) {
      const size_t here = at;
      at += (words + 1) & ~(size_t)1;  // (the 64-bit keys come first; everything stays 8-byte aligned)
      return here;
    };
    skeys = take(2 * slots), svals = take(slots);
    own = take(cap + 1), pos = take(cap + 1), sortbuf = take(4 * cap);
    need = take(cap + 1), rank = take(cap + 1), cslot = take(cap), cnw = take(cap);
    sort = take(sort_scratch_elems(cap));
    total = at;
  }
};

hipError_t launch_world_import(const IoGeo &g, const IoLayout &at, const WorldLayer &L, const uint32_t *src_hdr, const uint32_t *src_cells,
                               uint32_t *scan_scratch, hipStream_t s) {
  uint32_t *io = L.io;
  u64 *skeys = reinterpret_cast<u64 *>(io + at.skeys);
  uint32_t *svals = io + at.svals, *own = io + at.own, *pos = io + at.pos, *need = io + at.need, *rank = io + at.rank, *cslot = io + at.cslot,
           *cnw = io + at.cnw, *sort = io + at.sort;
  const uint32_t *count = pos + g.cap;
  uint32_t *buf[4] = {io + at.sortbuf, io + at.sortbuf + g.cap, io + at.sortbuf + 2 * (size_t)g.cap, io + at.sortbuf + 3 * (size_t)g.cap};
  const uint32_t slots = g.smask + 1u, per_thread = (g.cap + WTPB - 1) / WTPB, per_wave = (g.cap + WWAVES - 1) / WWAVES;
  hipError_t e;
  if ((e = hipMemsetAsync(io + at.skeys, 0xff, 3 * (size_t)slots * sizeof(uint32_t), s)) != hipSuccess) return e;  // keys and the indices beside them
  if ((e = hipMemsetAsync(need, 0, ((size_t)g.cap + 1) * sizeof(uint32_t), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(sort, 0, scan_scratch_elems(1) * sizeof(uint32_t), s)) != hipSuccess) return e;  // the part a sort wants zeroed
  if ((e = hipMemsetAsync(L.meta + M_CREATED, 0, 3 * sizeof(uint32_t), s)) != hipSuccess) return e;  // created, dropped, out of range: of this import
  LAYER_LAUNCH(k_wio_src_insert, (g.n + WTPB - 1) / WTPB, WTPB, s, g, src_hdr, skeys, svals);
  LAYER_LAUNCH(k_wio_owners, g.cap / WTPB + 1, WTPB, s, g, src_hdr, skeys, svals, own);
  exclusive_scan_u32(own, pos, (size_t)g.cap + 1, scan_scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wio_compact, per_thread, WTPB, s, g, src_hdr, own, pos, buf[0], buf[1]);
  const int w1 = radix_sort_pairs(buf[0], buf[1], buf[2], buf[3], g.cap, 32, sort, s, count);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t *ka = buf[2 * w1], *va = buf[2 * w1 + 1], *kb = buf[2 * (1 - w1)], *vb = buf[2 * (1 - w1) + 1];
  LAYER_LAUNCH(k_wio_key_hi, per_thread, WTPB, s, g, src_hdr, count, ka, va);
  const int w2 = radix_sort_pairs(ka, va, kb, vb, g.cap, 16, sort, s, count);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t *cand = w2 ? vb : va;
  LAYER_LAUNCH(k_wio_mark, per_wave, WTPB, s, g, src_hdr, src_cells, skeys, svals, count, cand, L.keys, L.vals, L.cells, need, cslot, cnw, L.meta);
  exclusive_scan_u32(need, rank, (size_t)g.cap + 1, scan_scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wio_merge, per_wave, WTPB, s, g, src_hdr, src_cells, skeys, svals, count, cand, L.keys, L.vals, need, rank, cslot, cnw, L.cells,
               L.hdr, L.meta);
  return launch_world_finish(rank + g.cap, g.max_bricks, L.meta, s);
}

}  // namespace

// the source table alone, for world_match.hip (sdm_world.h)
hipError_t launch_world_sources(const uint32_t *src_hdr, uint32_t n, uint32_t smask, unsigned long long *skeys, uint32_t *svals, hipStream_t s) {
  IoGeo g{};
  g.n = n;
  g.smask = smask;
  LAYER_LAUNCH(k_wio_src_insert, (n + WTPB - 1) / WTPB, WTPB, s, g, src_hdr, skeys, svals);
  return hipSuccess;
}

}  // namespace sdm

extern "C" {

sdm_status sdm_world_import(sdm_map *m, const sdm_world_import_options *o, const sdm_world_brick *bricks, const uint32_t *cells, int64_t n) {
  const char *what = "sdm_world_import";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~IMPORT_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (n < 0 || n > MAX_SOURCES) return LAYER_REFUSE(what, "n negative or above 2^21");
  if (n > 0 && (!bricks || !cells)) return LAYER_REFUSE(what, "no bricks or no cells");
  for (int a = 0; a < 3; ++a)
    if (o->cell_offset[a] > MAX_OFFSET || o->cell_offset[a] < -MAX_OFFSET) return LAYER_REFUSE(what, "a cell_offset beyond +-2^19");
  if (o->max_bricks < 0 || o->max_bricks > MAX_BRICKS_LIMIT) return LAYER_REFUSE(what, "max_bricks negative or above 2^21");
  SDM_TRY(layer_check(m, what, nullptr, WORLD));
  if (!n) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  WorldLayer &L = m->world;
  SDM_TRY(world_capacity(m, what, o->max_bricks));
  const bool on_device = (o->flags & SDM_WORLD_IMPORT_ON_DEVICE) != 0;
  IoGeo g;
  g.n = (uint32_t)n;
  g.ne = 1;
  for (int a = 0; a < 3; ++a) {
    g.q[a] = o->cell_offset[a] >> 3;
    g.r[a] = o->cell_offset[a] & 7;
    if (g.r[a]) g.ne *= 2;
  }
  g.cap = g.n * g.ne;
  uint32_t slots = 2;
  while (slots < 2 * g.n) slots <<= 1;
  g.smask = slots - 1;
  g.flags = o->flags & (ALL_FLAGS | SDM_WORLD_IMPORT_FILL);
  g.max_bricks = L.max_bricks;
  g.hmask = L.hmask;
  g.max_movable = m->d.max_movable;
  const IoLayout at(slots, g.cap);
  if (at.total > L.io_elems) SDM_TRY(regrow(m, &L.io, &L.io_elems, at.total, L.io ? m->stream : nullptr));
  uint32_t *scan = nullptr;
  SDM_TRY(layer_scan_scratch(m, (size_t)g.cap + 1, &scan));
  DevTemps tmp;
  const uint32_t *src_hdr = reinterpret_cast<const uint32_t *>(bricks), *src_cells = cells;
  if (!on_device) {
    uint32_t *d_hdr = nullptr, *d_cells = nullptr;
    HIP_TRY(tmp.alloc(&d_hdr, (size_t)n * HDR_WORDS));
    HIP_TRY(tmp.alloc(&d_cells, (size_t)n * 512));
    HIP_TRY(hipMemcpyAsync(d_hdr, bricks, (size_t)n * sizeof(sdm_world_brick), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(d_cells, cells, (size_t)n * 512 * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    src_hdr = d_hdr, src_cells = d_cells;
  }
  HIP_TRY(launch_world_import(g, at, L, src_hdr, src_cells, scan, m->stream));
  L.sorted = false;
  if (!L.n_updates) L.f = Frame{}, L.flags = 0;  // flags and stamp of the info describe the last update: there was none
  L.valid = true;
  if (!on_device) {  // the sources' copies and the work arrays go before the call returns
    HIP_TRY(hipStreamSynchronize(m->stream));
    release(m, &L.io);
    L.io_elems = 0;
  }
  return SDM_OK;
}

sdm_status sdm_world_retain(sdm_map *m, const sdm_world_retain_options *o, int64_t *n_removed) {
  const char *what = "sdm_world_retain";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags) return LAYER_REFUSE(what, "unknown flag bits");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldLayer &L = m->world;
  uint32_t meta[M_WORDS];
  SDM_TRY(world_counters(m, meta));
  const uint32_t n = meta[M_N_BRICKS];
  if (n_removed) *n_removed = 0;
  if (!n) return SDM_OK;
  KeepBox b;
  for (int a = 0; a < 3; ++a) b.lo[a] = o->bmin[a], b.hi[a] = o->bmax[a];
  b.min_last = o->min_last_stamp;
  uint32_t *scan = nullptr;
  SDM_TRY(layer_scan_scratch(m, (size_t)n + 1, &scan));
  DevTemps tmp;
  uint32_t *keep = nullptr, *pos = nullptr, *t_hdr = nullptr, *t_cells = nullptr;
  HIP_TRY(tmp.alloc(&keep, (size_t)n + 1));
  HIP_TRY(tmp.alloc(&pos, (size_t)n + 1));
  HIP_TRY(tmp.alloc(&t_hdr, (size_t)n * HDR_WORDS));
  HIP_TRY(tmp.alloc(&t_cells, (size_t)n * 512));
  hipStream_t s = m->stream;
  const unsigned per_wave = (n + WWAVES - 1) / WWAVES;
  hipLaunchKernelGGL(k_wio_keep, dim3(n / WTPB + 1), dim3(WTPB), 0, s, b, n, L.hdr, keep);
  HIP_TRY(hipGetLastError());
  exclusive_scan_u32(keep, pos, (size_t)n + 1, scan, s);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_wio_pack, dim3(per_wave), dim3(WTPB), 0, s, n, keep, pos, L.hdr, L.cells, t_hdr, t_cells);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s));
  hipLaunchKernelGGL(k_wio_unpack, dim3(per_wave), dim3(WTPB), 0, s, n, pos + n, t_hdr, t_cells, L.hdr, L.cells, L.keys, L.vals, L.hmask, L.meta);
  HIP_TRY(hipGetLastError());
  uint32_t kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, pos + n, sizeof(kept), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  L.sorted = false;
  if (n_removed) *n_removed = (int64_t)n - (int64_t)kept;
  return SDM_OK;
}

}  // extern "C"
