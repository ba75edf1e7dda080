// world.hip — the world archive: a world-fixed, sparse store of result words that outlives the ring's shifts (gfx950;
// include/sdm.h, "world archive").
//
// World cell of map-index cell i on axis a: g = moved_steps + i - (N >> 1); brick b = g >> 3 (arithmetic), 8 x 8 x 8 cells,
// cell word (g & 7) per axis as cx | cy << 3 | cz << 6.  The store is a pool of `max_bricks` bricks - 512 words and a
// 20-byte header each, handed out in the order the bricks are created - behind an open-addressing hash table of 64-bit
// keys ((bx + 32768) | (by + 32768) << 16 | (bz + 32768) << 32; all ones = empty) with the pool slot beside each key.
// An update:
//   k_world_mark    a wave per candidate brick - the bricks the block overlaps, ascending in (bz, by, bx) -, a lane per
//               (cx, cy), the eight z layers' loads of the results' second word issued first: counts the cells that
//               write, looks the key up (lane 0; a candidate without a writing cell is not looked up) and flags the
//               candidates that need creating.  Lookups only.
//   exclusive_scan_u32   ranks the flags; the entry behind the last candidate ends as their number.
//   k_world_merge   a wave per candidate with a writing cell: a new brick of rank r takes pool slot n_bricks + r if that is
//               below max_bricks (lane 0 inserts the key: every key by exactly one thread, the CAS only arbitrates hash
//               slots) and is written whole, an archived one is read, the writing cells replaced, its counts taken
//               again.  Insertions only; n_bricks is read, not written.
//   k_world_finish  one thread: n_bricks, created_last, dropped_total.
// Which bricks get room depends on the scan alone, so everything is reproducible bit for bit.  The pool is in creation
// order; the getters that promise brick order sort the pool slots by two passes of the stable radix sort (low word
// (bx, by), then bz), lazily at the first such getter after an update.
// The table's key, hash, lookup and insertion, cell_writes, the header words and the counters' indices are in sdm_world.h;
// world_io.hip (import and retain) closes with k_world_finish too, through launch_world_finish.
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_options) == 16 && sizeof(sdm_world_brick) == 20 && sizeof(sdm_world_cell) == 8 && sizeof(sdm_world_info) == 80,
              "sdm.h layout");
static_assert(offsetof(sdm_world_options, max_bricks) == 8 && offsetof(sdm_world_info, dropped_total) == 24 &&
                  offsetof(sdm_world_info, bmin) == 48 && offsetof(sdm_world_info, flags) == 72 && offsetof(sdm_world_brick, first_stamp) == 12,
              "sdm.h layout");
static_assert(SDM_WORLD_BYTES_PER_BRICK == 512 * 4 + 20 + 2 * (8 + 4) + 4 * 4 + 4, "sdm.h states the bytes per brick of capacity");

namespace sdm {

namespace {

__device__ __forceinline__ void candidate_brick(const WGeo &g, uint32_t c, int &bx, int &by, int &bz) {
  const uint32_t nx = (uint32_t)g.nb[0], ny = (uint32_t)g.nb[1];
  const uint32_t t = c / nx;
  bx = g.b0[0] + (int)(c - t * nx);
  by = g.b0[1] + (int)(t % ny);
  bz = g.b0[2] + (int)(t / ny);
}

// the block's words of brick (bx, by, bz), a lane per (cx, cy), layer cz in w[cz]: every load issued first; a cell of the
// brick outside the block reads as unobserved (it writes nothing)
__device__ __forceinline__ void load_brick(const Dims &d, const Frame &f, const uint2 *__restrict__ res, const WGeo &g, int bx, int by, int bz,
                                           uint32_t lane, uint32_t (&w)[8]) {
  const int ix = bx * 8 + (int)(lane & 7u) - g.g0[0], iy = by * 8 + (int)(lane >> 3) - g.g0[1], iz0 = bz * 8 - g.g0[2];
  const bool in_xy = (uint32_t)ix < d.NX && (uint32_t)iy < d.NY;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int iz = iz0 + l;
    w[l] = RES_UNKNOWN_W1;
    if (in_xy && (uint32_t)iz < d.NZ) w[l] = res[cell_voxel(d, f, ix, iy, iz)].y;
  }
}

// ---- the update -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WTPB) void k_world_mark(Dims d, Frame f, const uint2 *__restrict__ res, WGeo g, const u64 *__restrict__ keys,
                                                     const uint32_t *__restrict__ vals, uint32_t *__restrict__ need,
                                                     uint32_t *__restrict__ cslot, uint32_t *__restrict__ cnw, uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (c == 0u && lane == 0u) need[g.nc_max] = 0u;  // the scan's extra entry: the number of new bricks lands there
  if (c >= g.nc) {                                 // (wave-uniform) the scan has one length per map
    if (c < g.nc_max && lane == 0u) need[c] = 0u;
    return;
  }
  int bx, by, bz;
  candidate_brick(g, c, bx, by, bz);
  uint32_t w[8];
  load_brick(d, f, res, g, bx, by, bz, lane, w);
  uint32_t nw = 0;
#pragma unroll
  for (int l = 0; l < 8; ++l) nw += (uint32_t)__popcll(__ballot(cell_writes(w[l], g.flags, g.max_movable)));
  if (lane != 0u) return;
  uint32_t slot = NONE, create = 0u;
  if (nw) {
    if (brick_in_range(bx, by, bz)) {
      slot = world_find(keys, vals, g.hmask, brick_key(bx, by, bz));
      create = slot == NONE ? 1u : 0u;
    } else {
      nw = 0u;  // never created: its cells write nothing
      atomicAdd(meta + M_OOR, 1u);
    }
  }
  need[c] = create;
  cslot[c] = slot;
  cnw[c] = nw;
}

__global__ __launch_bounds__(WTPB) void k_world_merge(Dims d, Frame f, const uint2 *__restrict__ res, WGeo g, u64 *__restrict__ keys,
                                                      uint32_t *__restrict__ vals, const uint32_t *__restrict__ need,
                                                      const uint32_t *__restrict__ rank, const uint32_t *__restrict__ cslot,
                                                      const uint32_t *__restrict__ cnw, uint32_t *__restrict__ cells,
                                                      uint32_t *__restrict__ hdr, uint32_t *__restrict__ meta) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (c >= g.nc) return;  // (wave-uniform, like every return below)
  const uint32_t nw = cnw[c];
  if (!nw) return;
  const bool fresh = need[c] != 0u;
  const uint32_t slot = fresh ? meta[M_N_BRICKS] + rank[c] : cslot[c];
  if (slot >= g.max_bricks) {  // a new brick without room: its cells are dropped
    if (lane == 0u) atomicAdd(meta + M_DROPPED, nw);
    return;
  }
  int bx, by, bz;
  candidate_brick(g, c, bx, by, bz);
  uint32_t w[8], old[8];
  load_brick(d, f, res, g, bx, by, bz, lane, w);
  uint32_t *__restrict__ mine = cells + (size_t)slot * 512u + lane;
#pragma unroll
  for (int l = 0; l < 8; ++l) old[l] = fresh ? RES_UNKNOWN_W1 : mine[l * 64];
  uint32_t n_occ = 0, n_free = 0;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const bool wr = cell_writes(w[l], g.flags, g.max_movable);
    const uint32_t v = wr ? w[l] : old[l];
    if (wr || fresh) mine[l * 64] = v;
    const int occ = occ_of(v);
    n_occ += (uint32_t)__popcll(__ballot(occ >= 1));
    n_free += (uint32_t)__popcll(__ballot(occ == 0));
  }
  if (lane != 0u) return;
  if (fresh) world_insert(keys, vals, g.hmask, brick_key(bx, by, bz), slot);
  uint32_t *__restrict__ h = hdr + (size_t)slot * HDR_WORDS;
  h[0] = ((uint32_t)bx & 0xffffu) | (((uint32_t)by & 0xffffu) << 16);
  h[1] = ((uint32_t)bz & 0xffffu) | (n_occ << 16);
  h[2] = n_free;
  if (fresh) h[3] = g.gts;
  h[4] = g.gts;
}

__global__ __launch_bounds__(64) void k_world_finish(const uint32_t *__restrict__ wanted_at, uint32_t max_bricks, uint32_t *__restrict__ meta) {
  if (threadIdx.x != 0u) return;
  const uint32_t n = meta[M_N_BRICKS], wanted = *wanted_at, room = max_bricks - n;
  const uint32_t created = wanted < room ? wanted : room;
  meta[M_N_BRICKS] = n + created;
  meta[M_CREATED] = created;
  u64 *total = reinterpret_cast<u64 *>(meta + M_DROPPED_TOTAL);
  *total += meta[M_DROPPED];
}

// ---- brick order ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WTPB) void k_world_order_lo(const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ meta, uint32_t cap,
                                                          uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  const uint32_t i = blockIdx.x * WTPB + threadIdx.x;
  if (i >= cap) return;
  const uint32_t n = meta[M_N_BRICKS];
  key[i] = i < n ? hdr[(size_t)i * HDR_WORDS] ^ 0x80008000u : 0u;  // (bx + 32768) | (by + 32768) << 16
  val[i] = i;
}
// the second pass's keys: bz + 32768 of the bricks in the order the first pass left
__global__ __launch_bounds__(WTPB) void k_world_order_hi(const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ meta, uint32_t cap,
                                                           uint32_t *__restrict__ key, const uint32_t *__restrict__ val) {
  const uint32_t i = blockIdx.x * WTPB + threadIdx.x;
  if (i >= cap) return;
  const uint32_t n = meta[M_N_BRICKS];
  key[i] = i < n ? (hdr[(size_t)val[i] * HDR_WORDS + 1] & 0xffffu) ^ 0x8000u : 0u;
}

// ---- the getters ----------------------------------------------------------------------------------------------------
// a wave per brick first + j of the order: header and, if asked for, cells into the call's staging lists
__global__ __launch_bounds__(WTPB) void k_world_gather(const uint32_t *__restrict__ order, uint32_t first, uint32_t take,
                                                       const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ cells,
                                                       uint32_t *__restrict__ out_hdr, uint32_t *__restrict__ out_cells) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (j >= take) return;
  const uint32_t src = order[first + j];
  if (lane < HDR_WORDS) out_hdr[(size_t)j * HDR_WORDS + lane] = hdr[(size_t)src * HDR_WORDS + lane];
  if (out_cells) {
    uint32_t w[8];
#pragma unroll
    for (int l = 0; l < 8; ++l) w[l] = cells[(size_t)src * 512u + (uint32_t)l * 64u + lane];
#pragma unroll
    for (int l = 0; l < 8; ++l) out_cells[(size_t)j * 512u + (uint32_t)l * 64u + lane] = w[l];
  }
}

// cnt[j] = the occupied cells of the j-th brick of the order, 0 from n_bricks on (cap + 1 entries: the scan's total)
__global__ __launch_bounds__(WTPB) void k_world_occ_count(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr,
                                                          const uint32_t *__restrict__ meta, uint32_t cap, uint32_t *__restrict__ cnt) {
  const uint32_t j = blockIdx.x * WTPB + threadIdx.x;
  if (j > cap) return;
  cnt[j] = j < meta[M_N_BRICKS] ? hdr[(size_t)order[j] * HDR_WORDS + 1] >> 16 : 0u;
}

// a wave per brick of the order: its cells with occ >= 1 as sdm_point, ascending in cell word, from the brick's prefix on;
// nothing at or beyond `cap`
__global__ __launch_bounds__(WTPB) void k_world_occ_emit(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr,
                                                         const uint32_t *__restrict__ cells, const uint32_t *__restrict__ pre,
                                                         const uint32_t *__restrict__ meta, uint32_t max_bricks, float voxel_size,
                                                         uint4 *__restrict__ out, uint32_t cap) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * WWAVES + (threadIdx.x >> 6);
  if (j >= max_bricks || j >= meta[M_N_BRICKS]) return;
  const uint32_t src = order[j];
  uint32_t base = pre[j];
  const uint32_t h0 = hdr[(size_t)src * HDR_WORDS], h1 = hdr[(size_t)src * HDR_WORDS + 1];
  if (!(h1 >> 16) || base >= cap) return;
  const int bx = (int16_t)(h0 & 0xffffu), by = (int16_t)(h0 >> 16), bz = (int16_t)(h1 & 0xffffu);
  uint32_t w[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) w[l] = cells[(size_t)src * 512u + (uint32_t)l * 64u + lane];
  const float x = (float)(bx * 8 + (int)(lane & 7u)) * voxel_size, y = (float)(by * 8 + (int)(lane >> 3)) * voxel_size;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const bool occ = occ_of(w[l]) >= 1;
    const u64 m = __ballot(occ);
    const uint32_t r = base + lane_rank(m, lane);
    if (occ && r < cap) out[r] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint((float)(bz * 8 + l) * voxel_size), w[l]);
    base += (uint32_t)__popcll(m);
  }
}

__global__ __launch_bounds__(WTPB) void k_world_query(float recip, const float *__restrict__ xyz, uint32_t n, const u64 *__restrict__ keys,
                                                      const uint32_t *__restrict__ vals, const uint32_t *__restrict__ hdr,
                                                      const uint32_t *__restrict__ cells, uint32_t hmask, uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * WTPB + threadIdx.x;
  if (i >= n) return;
  int g[3];
  uint2 r = make_uint2(RES_UNKNOWN_W1, 0u);
  if (entry_cell(xyz, nullptr, i, recip, g)) {
    const uint32_t slot = world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3));
    if (slot != NONE) {
      r.x = cells[(size_t)slot * 512u + (uint32_t)((g[0] & 7) | ((g[1] & 7) << 3) | ((g[2] & 7) << 6))];
      r.y = hdr[(size_t)slot * HDR_WORDS + 4];
    }
  }
  out[i] = r;
}

struct WBox {
  int lo[3];
  uint32_t size[3];
};
// words [off, off + count) of the dense grid of a box of world cells, x fastest
__global__ __launch_bounds__(WTPB) void k_world_region(WBox b, uint32_t off, uint32_t count, const u64 *__restrict__ keys,
                                                       const uint32_t *__restrict__ vals, const uint32_t *__restrict__ cells, uint32_t hmask,
                                                       uint32_t *__restrict__ out) {
  const uint32_t i = blockIdx.x * WTPB + threadIdx.x;
  if (i >= count) return;
  const uint32_t k = off + i, t = k / b.size[0];
  const long long gx = (long long)b.lo[0] + (k - t * b.size[0]), gy = (long long)b.lo[1] + t % b.size[1], gz = (long long)b.lo[2] + t / b.size[1];
  const long long bx = gx >> 3, by = gy >> 3, bz = gz >> 3;
  uint32_t w = RES_UNKNOWN_W1;
  if (bx >= -32768 && bx <= 32767 && by >= -32768 && by <= 32767 && bz >= -32768 && bz <= 32767) {
    const uint32_t slot = world_find(keys, vals, hmask, brick_key((int)bx, (int)by, (int)bz));
    if (slot != NONE) w = cells[(size_t)slot * 512u + (uint32_t)((gx & 7) | ((gy & 7) << 3) | ((gz & 7) << 6))];
  }
  out[i] = w;
}

// ---- host ------------------------------------------------------------------------------------------------------------
uint32_t candidates_max(const Dims &d) { return (((d.NX + 7) >> 3) + 1) * (((d.NY + 7) >> 3) + 1) * (((d.NZ + 7) >> 3) + 1); }
int64_t default_bricks(const Dims &d) {
  int64_t want = std::max<int64_t>(2 * (int64_t)(d.NX / 8 + 1) * (d.NY / 8 + 1) * (d.NZ / 8 + 1), 4096), p = 1;
  while (p < want) p <<= 1;
  return p;
}

void world_release(sdm_map *m) {
  WorldLayer &L = m->world;
  release(m, &L.keys), release(m, &L.vals), release(m, &L.cells), release(m, &L.hdr), release(m, &L.cand), release(m, &L.meta);
  release(m, &L.sort), release(m, &L.sortbuf), release(m, &L.cnt);
  L.max_bricks = 0;
}

// the buffers for `bricks` bricks, empty (the stream is idle if there were buffers before)
sdm_status world_alloc(sdm_map *m, uint32_t bricks) {
  WorldLayer &L = m->world;
  world_release(m);
  const uint32_t slots = table_slots(bricks);
  const size_t nc_max = candidates_max(m->d);
  SDM_TRY(alloc_tracked(m, &L.keys, slots));
  SDM_TRY(alloc_tracked(m, &L.vals, slots));
  SDM_TRY(alloc_tracked(m, &L.cells, (size_t)bricks * 512));
  SDM_TRY(alloc_tracked(m, &L.hdr, (size_t)bricks * HDR_WORDS));
  SDM_TRY(alloc_tracked(m, &L.cand, 4 * nc_max + 2));
  SDM_TRY(alloc_tracked(m, &L.meta, (size_t)M_WORDS));
  SDM_TRY(alloc_tracked(m, &L.sort, sort_scratch_elems(bricks)));
  SDM_TRY(alloc_tracked(m, &L.sortbuf, 4 * (size_t)bricks));
  SDM_TRY(alloc_tracked(m, &L.cnt, (size_t)bricks + 1));
  HIP_TRY(hipMemsetAsync(L.keys, 0xff, (size_t)slots * sizeof(u64), m->stream));
  HIP_TRY(hipMemsetAsync(L.meta, 0, M_WORDS * sizeof(uint32_t), m->stream));
  HIP_TRY(hipMemsetAsync(L.sort, 0, sort_scratch_elems(bricks) * sizeof(uint32_t), m->stream));
  L.max_bricks = bricks;
  L.hmask = slots - 1;
  return SDM_OK;
}

WGeo geo_of(const sdm_map *m, uint32_t flags) {
  const Dims &d = m->d;
  const WorldLayer &L = m->world;
  const int N[3] = {(int)d.NX, (int)d.NY, (int)d.NZ};
  WGeo g;
  for (int a = 0; a < 3; ++a) {
    g.g0[a] = m->moved_steps[a] - (N[a] >> 1);
    g.b0[a] = g.g0[a] >> 3;
    g.nb[a] = ((g.g0[a] + N[a] - 1) >> 3) - g.b0[a] + 1;
  }
  g.nc = (uint32_t)(g.nb[0] * g.nb[1] * g.nb[2]);
  g.nc_max = candidates_max(d);
  g.flags = flags;
  g.gts = m->f.gts;
  g.max_bricks = L.max_bricks;
  g.hmask = L.hmask;
  g.max_movable = d.max_movable;
  return g;
}

hipError_t launch_world_update(const Dims &d, const Frame &f, const State &st, const WGeo &g, const WorldLayer &L, uint32_t *scan_scratch,
                               hipStream_t s) {
  const uint2 *res = reinterpret_cast<const uint2 *>(st.res);
  uint32_t *need = L.cand, *rank = need + g.nc_max + 1, *cslot = rank + g.nc_max + 1, *cnw = cslot + g.nc_max;
  hipError_t e;
  if ((e = hipMemsetAsync(L.meta + M_CREATED, 0, 3 * sizeof(uint32_t), s)) != hipSuccess) return e;  // created, dropped, out of range: of this update
  LAYER_LAUNCH(k_world_mark, (g.nc_max + WWAVES - 1) / WWAVES, WTPB, s, d, f, res, g, L.keys, L.vals, need, cslot, cnw, L.meta);
  exclusive_scan_u32(need, rank, (size_t)g.nc_max + 1, scan_scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_world_merge, (g.nc + WWAVES - 1) / WWAVES, WTPB, s, d, f, res, g, L.keys, L.vals, need, rank, cslot, cnw, L.cells, L.hdr, L.meta);
  return launch_world_finish(rank + g.nc_max, g.max_bricks, L.meta, s);
}

// the pool slots in brick order (WorldLayer::order), once per update
hipError_t launch_world_sort(WorldLayer &L, hipStream_t s) {
  const uint32_t cap = L.max_bricks, grid = (cap + WTPB - 1) / WTPB;
  uint32_t *buf[4] = {L.sortbuf, L.sortbuf + cap, L.sortbuf + 2 * (size_t)cap, L.sortbuf + 3 * (size_t)cap};  // keys a, vals a, keys b, vals b
  LAYER_LAUNCH(k_world_order_lo, grid, WTPB, s, L.hdr, L.meta, cap, buf[0], buf[1]);
  const int w1 = radix_sort_pairs(buf[0], buf[1], buf[2], buf[3], cap, 32, L.sort, s, L.meta + M_N_BRICKS);
  hipError_t e;
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t *ka = buf[2 * w1], *va = buf[2 * w1 + 1], *kb = buf[2 * (1 - w1)], *vb = buf[2 * (1 - w1) + 1];
  LAYER_LAUNCH(k_world_order_hi, grid, WTPB, s, L.hdr, L.meta, cap, ka, va);
  const int w2 = radix_sort_pairs(ka, va, kb, vb, cap, 16, L.sort, s, L.meta + M_N_BRICKS);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  L.order = w2 ? vb : va;
  L.sorted = true;
  return hipSuccess;
}

// the layers' shared scratch, for the longer of the update's scan and the getter's
sdm_status world_scan_scratch(sdm_map *m, uint32_t **scratch) {
  return layer_scan_scratch(m, std::max<size_t>(candidates_max(m->d), m->world.max_bricks) + 1, scratch);
}

// waits; the archive's counters
sdm_status world_meta(sdm_map *m, uint32_t (&meta)[M_WORDS]) {
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(meta, m->world.meta, sizeof(meta), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

sdm_status world_sorted(sdm_map *m) {
  if (!m->world.sorted) HIP_TRY(launch_world_sort(m->world, m->stream));
  return SDM_OK;
}

}  // namespace

hipError_t launch_world_finish(const uint32_t *wanted, uint32_t max_bricks, uint32_t *meta, hipStream_t s) {
  LAYER_LAUNCH(k_world_finish, 1, 64, s, wanted, max_bricks, meta);
  return hipSuccess;
}

sdm_status world_counters(sdm_map *m, uint32_t *meta) {
  uint32_t got[M_WORDS];
  SDM_TRY(world_meta(m, got));
  std::memcpy(meta, got, sizeof(got));
  return SDM_OK;
}

sdm_status world_order(sdm_map *m, const uint32_t **order) {
  SDM_TRY(world_sorted(m));
  *order = m->world.order;
  return SDM_OK;
}

sdm_status world_capacity(sdm_map *m, const char *what, int64_t max_bricks) {
  WorldLayer &L = m->world;
  if (!L.capacity_set) {  // the first update after creation or sdm_world_clear sets the capacity
    const uint32_t want = (uint32_t)(max_bricks ? max_bricks : default_bricks(m->d));
    if (want != L.max_bricks) {
      if (L.max_bricks) HIP_TRY(hipStreamSynchronize(m->stream));
      SDM_TRY(world_alloc(m, want));
    }
    L.capacity_set = true;
  } else if (max_bricks && (uint32_t)max_bricks != L.max_bricks) {
    uint32_t meta[M_WORDS];
    SDM_TRY(world_meta(m, meta));
    if (meta[M_N_BRICKS]) return LAYER_REFUSE(what, "another max_bricks while the archive holds bricks: call sdm_world_clear first");
    SDM_TRY(world_alloc(m, (uint32_t)max_bricks));
  }
  return SDM_OK;
}

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
extern "C" {

sdm_status sdm_world_update(sdm_map *m, const sdm_world_options *o) {
  const char *what = "sdm_world_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->max_bricks < 0 || o->max_bricks > MAX_BRICKS_LIMIT) return LAYER_REFUSE(what, "max_bricks negative or above 2^21");
  SDM_TRY(layer_check(m, what, nullptr, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldLayer &L = m->world;
  SDM_TRY(world_capacity(m, what, o->max_bricks));
  uint32_t *scan = nullptr;
  SDM_TRY(world_scan_scratch(m, &scan));
  const Frame f = m->f;
  HIP_TRY(launch_world_update(m->d, f, m->st, geo_of(m, o->flags), L, scan, m->stream));
  for (int a = 0; a < 3; ++a) L.steps[a] = m->moved_steps[a];
  L.n_updates++;
  L.sorted = false;
  L.built(f, o->flags);
  return SDM_OK;
}

sdm_status sdm_world_clear(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_world_clear", nullptr, WORLD));
  WorldLayer &L = m->world;
  if (L.max_bricks) {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), m->stream));
    HIP_TRY(hipMemsetAsync(L.meta, 0, M_WORDS * sizeof(uint32_t), m->stream));
  }
  L.capacity_set = false;
  L.valid = false;
  L.sorted = false;
  L.n_updates = 0;
  return SDM_OK;
}

sdm_status sdm_get_world_info(sdm_map *m, sdm_world_info *info) {
  const char *what = "sdm_get_world_info";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!info) return LAYER_REFUSE(what, "no info");
  SDM_TRY(layer_check(m, what, nullptr, WORLD));
  WorldLayer &L = m->world;
  sdm_world_info out;
  std::memset(&out, 0, sizeof(out));
  for (int a = 0; a < 3; ++a) out.bmax[a] = -1;
  if (L.valid) {
    uint32_t meta[M_WORDS];
    SDM_TRY(world_meta(m, meta));
    const uint32_t n = meta[M_N_BRICKS];
    std::vector<sdm_world_brick> hdr(n);
    if (n) {
      HIP_TRY(hipMemcpyAsync(hdr.data(), L.hdr, (size_t)n * sizeof(sdm_world_brick), hipMemcpyDeviceToHost, m->stream));
      HIP_TRY(hipStreamSynchronize(m->stream));
    }
    out.n_bricks = n;
    out.max_bricks = L.max_bricks;
    out.n_updates = L.n_updates;
    out.created_last = meta[M_CREATED];
    out.dropped_last = meta[M_DROPPED];
    out.out_of_range_last = meta[M_OOR];
    std::memcpy(&out.dropped_total, meta + M_DROPPED_TOTAL, sizeof(uint64_t));
    for (uint32_t i = 0; i < n; ++i) {
      const int16_t b[3] = {hdr[i].bx, hdr[i].by, hdr[i].bz};
      out.n_occupied += hdr[i].n_occupied;
      out.n_free += hdr[i].n_free;
      for (int a = 0; a < 3; ++a) {
        out.bmin[a] = i ? std::min<int32_t>(out.bmin[a], b[a]) : b[a];
        out.bmax[a] = i ? std::max<int32_t>(out.bmax[a], b[a]) : b[a];
      }
    }
    out.flags = L.flags;
    out.stamp = L.f.gts;
  }
  *info = out;
  return SDM_OK;
}

sdm_status sdm_get_world_bricks(sdm_map *m, sdm_world_brick *bricks, uint32_t *cells, int64_t first, int64_t cap, int64_t *n_out) {
  const char *what = "sdm_get_world_bricks";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  WorldLayer &L = m->world;
  uint32_t meta[M_WORDS];
  SDM_TRY(world_meta(m, meta));
  const int64_t n = meta[M_N_BRICKS];
  *n_out = n;
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>(n - first, cap), 0);
  if (!take || (!bricks && !cells)) return SDM_OK;
  SDM_TRY(world_sorted(m));
  DevTemps tmp;
  uint32_t *d_hdr = nullptr, *d_cells = nullptr;
  HIP_TRY(tmp.alloc(&d_hdr, take * HDR_WORDS));
  if (cells) HIP_TRY(tmp.alloc(&d_cells, take * 512));
  hipLaunchKernelGGL(k_world_gather, dim3((unsigned)((take + WWAVES - 1) / WWAVES)), dim3(WTPB), 0, m->stream, L.order, (uint32_t)first,
                     (uint32_t)take, L.hdr, L.cells, d_hdr, d_cells);
  HIP_TRY(hipGetLastError());
  if (bricks) HIP_TRY(hipMemcpyAsync(bricks, d_hdr, take * sizeof(sdm_world_brick), hipMemcpyDeviceToHost, m->stream));
  if (cells) HIP_TRY(hipMemcpyAsync(cells, d_cells, take * 512 * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

sdm_status sdm_get_world_occupied(sdm_map *m, sdm_point *out, int64_t cap, int64_t *n_out, uint32_t flags) {
  const char *what = "sdm_get_world_occupied";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out) return LAYER_REFUSE(what, "cap < 0 or no n_out");
  if (flags & ~SDM_QUERY_ON_DEVICE) return LAYER_REFUSE(what, "unknown flag bits");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldLayer &L = m->world;
  SDM_TRY(world_sorted(m));
  const uint32_t bricks = L.max_bricks;
  uint32_t *scan = nullptr;
  SDM_TRY(world_scan_scratch(m, &scan));
  hipLaunchKernelGGL(k_world_occ_count, dim3(bricks / WTPB + 1), dim3(WTPB), 0, m->stream, L.order, L.hdr, L.meta, bricks, L.cnt);
  HIP_TRY(hipGetLastError());
  exclusive_scan_u32(L.cnt, L.cnt, (size_t)bricks + 1, scan, m->stream);
  HIP_TRY(hipGetLastError());
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, L.cnt + bricks, sizeof(total), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  *n_out = (int64_t)total;
  const size_t take = (size_t)std::min<int64_t>((int64_t)total, cap);
  if (!take || !out) return SDM_OK;
  DevTemps tmp;
  sdm_point *d_out = out;
  if (!(flags & SDM_QUERY_ON_DEVICE)) HIP_TRY(tmp.alloc(&d_out, take));
  hipLaunchKernelGGL(k_world_occ_emit, dim3((bricks + WWAVES - 1) / WWAVES), dim3(WTPB), 0, m->stream, L.order, L.hdr, L.cells, L.cnt, L.meta, bricks,
                     m->d.voxel_size, reinterpret_cast<uint4 *>(d_out), (uint32_t)take);
  HIP_TRY(hipGetLastError());
  if (!(flags & SDM_QUERY_ON_DEVICE)) {
    HIP_TRY(hipMemcpyAsync(out, d_out, take * sizeof(sdm_point), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return SDM_OK;
}

sdm_status sdm_query_world_points(sdm_map *m, const float *xyz, int64_t n, sdm_world_cell *out, uint32_t flags) {
  const char *what = "sdm_query_world_points";
  SDM_TRY(query_check(m, xyz, n, out, flags, SDM_QUERY_ON_DEVICE, what));
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  const WorldLayer L = m->world;
  const float recip = m->d.recip;
  return run_query(m, xyz, 12, out, sizeof(sdm_world_cell), nullptr, 0, n, flags, [L, recip](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
    hipLaunchKernelGGL(k_world_query, dim3((c + WTPB - 1) / WTPB), dim3(WTPB), 0, s, recip, static_cast<const float *>(in), c, L.keys, L.vals, L.hdr,
                       L.cells, L.hmask, static_cast<uint2 *>(o));
  });
}

sdm_status sdm_get_world_region(sdm_map *m, const int32_t cell_min[3], const int32_t size[3], uint32_t *words, uint32_t flags) {
  const char *what = "sdm_get_world_region";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!cell_min || !size || !words) return LAYER_REFUSE(what, "a null pointer");
  if (flags & ~SDM_QUERY_ON_DEVICE) return LAYER_REFUSE(what, "unknown flag bits");
  if (size[0] <= 0 || size[1] <= 0 || size[2] <= 0 || (int64_t)size[0] * size[1] > ((int64_t)1 << 28) ||
      (int64_t)size[0] * size[1] * size[2] > ((int64_t)1 << 28))
    return LAYER_REFUSE(what, "sizes must be > 0 with a product of at most 2^28");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  const WorldLayer L = m->world;
  WBox b;
  for (int a = 0; a < 3; ++a) b.lo[a] = cell_min[a], b.size[a] = (uint32_t)size[a];
  const size_t total = (size_t)size[0] * size[1] * size[2], chunk = std::min(total, (size_t)1 << 22);
  hipStream_t s = m->stream;
  auto launch = [&](size_t off, size_t count, uint32_t *dst) {
    hipLaunchKernelGGL(k_world_region, dim3((unsigned)((count + WTPB - 1) / WTPB)), dim3(WTPB), 0, s, b, (uint32_t)off, (uint32_t)count, L.keys, L.vals,
                       L.cells, L.hmask, dst);
  };
  if (flags & SDM_QUERY_ON_DEVICE) {
    for (size_t off = 0; off < total; off += chunk) {
      launch(off, std::min(chunk, total - off), words + off);
      HIP_TRY(hipGetLastError());
    }
    return SDM_OK;
  }
  size_t off = 0;  // (run_staged takes the chunks in order)
  return run_staged(m, total, chunk, nullptr, 0, {{StageCol::OUT, words, sizeof(uint32_t)}},
                    [&](const unsigned char *, unsigned char *const *col, size_t c) -> sdm_status {
                      launch(off, c, reinterpret_cast<uint32_t *>(col[0]));
                      HIP_TRY(hipGetLastError());
                      off += c;
                      return SDM_OK;
                    });
}

}  // extern "C"
