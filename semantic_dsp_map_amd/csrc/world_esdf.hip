// world_esdf.hip — the world distance field: a truncated Euclidean distance field over the bricks of the world archive -
// for every cell of a field brick the squared distance, in world cells, to the nearest archived obstacle and the offset to
// it, exact up to a radius R <= 16 cells and "far" beyond (gfx950; include/sdm.h, "world distance field").
//
// Truncation makes the field brick-local: with R <= 8 H everything a brick needs lies in the (2 H + 1)^3 bricks round it,
// as obstacle BITS 1.7 KB (H = 1) or 8 KB (H = 2).  So one workgroup per brick does in LDS what esdf.hip needs three global
// passes for, and the only global traffic of the build is the neighbour lookups, the obstacle words and one packed store a
// cell.  The build is a snapshot: coordinates, a hash table of its own from brick key to rank and the field; no pool slot.
//   snapshot_bricks, launch_snapshot_index   world_snapshot.hip's: the bricks of the box flagged and ranked, their
//               coordinates at their rank, key -> rank in the layer's table.
//   k_we_classify    a wave per archived brick - all of them: a box reads across its sides -, a lane per (cx, cy), the
//               eight layers' loads first, then a ballot a layer: the eight obstacle words (bit cx + 8 cy), 64 B, at the
//               brick's pool slot, where the archive's own hash table leads.
//   k_we_build<H>    a workgroup per field brick.  (2 H + 1)^3 threads look the neighbour bricks up (brick_in_range before
//               every lookup), their obstacle words go to LDS, an absent brick as zeros, or ones under UNKNOWN_IS_OBSTACLE.
//               x pass: a thread per row (y, z) of the halo within R of the brick: the row's 8 (2 H + 1) <= 40 bits in
//               one register, per column of the brick the nearest set bit below (a mask and __clzll) and above (a shift
//               and __ffsll), the lower on a tie: eight signed bytes, one 8-byte LDS store.  y pass: per (cx, cy, z) the
//               windowed minimum of dx^2 + dy^2 over y - R .. y + R, ascending, replaced only by a strictly smaller sum.
//               z pass: per cell the same over z - R .. z + R; one packed store a cell.  A candidate whose partial sum
//               exceeds R^2 is dropped at once.  No global intermediate, no atomics but the two info counters after a
//               ballot, no workgroup waits for another.
//   k_query_world_distance   a lane per point: its cell, one table lookup, one load; the result leaves in four 8-byte stores.
// The packed field word: d2 in bits 0 .. 9 (0x3ff: none within R), dx + 32, dy + 32, dz + 32 in 6 bits each from bit 10.
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_esdf_options) == 32 && sizeof(sdm_world_esdf_info) == 32 && sizeof(sdm_world_distance_result) == 32, "sdm.h layout");
static_assert(offsetof(sdm_world_esdf_options, bmin) == 8 && offsetof(sdm_world_esdf_options, bmax) == 20 &&
                  offsetof(sdm_world_esdf_info, stamp) == 12 && offsetof(sdm_world_esdf_info, n_obstacle_cells) == 16 &&
                  offsetof(sdm_world_esdf_info, n_near_cells) == 24 && offsetof(sdm_world_distance_result, nearest) == 12 &&
                  offsetof(sdm_world_distance_result, d2) == 24 && offsetof(sdm_world_distance_result, distance) == 28,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;  // the kernels of a thread or a wave per item
constexpr int BT = 256;  // k_we_build
constexpr uint32_t ALL_WE_FLAGS = SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE | SDM_WORLD_ESDF_STATIC_ONLY | SDM_WORLD_ESDF_BOX;
constexpr uint32_t PACK_NONE = 0x3ffu | (32u << 10) | (32u << 16) | (32u << 22);
constexpr int NO_DX = -128;           // x pass: no obstacle within R in this row
constexpr uint32_t NO_D2 = 0xffffu;   // y pass: no obstacle within R in this column of the layer
// the build's counters, 64 bits each, in E_SPREAD copies - a workgroup adds to copy (brick & (E_SPREAD - 1)), the getter
// sums them: tens of thousands of atomics on one address take milliseconds.  The landing area has one word
// more, for the count the build waits for.
enum { E_OBST = 0, E_NEAR, E_PAIR, E_SPREAD = 64, E_WORDS = E_PAIR * E_SPREAD };

constexpr size_t ARCH_BYTES = 4 + 4 + 8 * 8;            // flag, rank, obstacle words
constexpr size_t BRICK_BYTES = 512 * 4 + 8 + 2 * (8 + 4);  // field, coordinates, two hash slots
static_assert(ARCH_BYTES == SDM_WORLD_ESDF_BYTES_PER_ARCHIVED_BRICK && BRICK_BYTES == SDM_WORLD_ESDF_BYTES_PER_BRICK, "sdm.h states the bytes");

// what k_we_build<H> keeps in LDS: the obstacle words, the x pass' bytes, the y pass' words, the neighbours' slots (a
// multiple of four words: the other arrays stay aligned wherever the compiler puts them), the waves' two counts
template <int H>
struct BuildShape {
  static constexpr int W = 2 * H + 1, S = 8 * W, NB = W * W * W, NB2 = (NB + 3) & ~3;
  static constexpr size_t LDS = (size_t)S * W * W * 8 + (size_t)S * S * 8 + (size_t)S * 64 * 4 + (size_t)NB2 * 4 + (BT / 64) * 2 * 4;
};
static_assert(BuildShape<1>::LDS == 1728 + 4608 + 6144 + 112 + 32 && BuildShape<2>::LDS == 8000 + 12800 + 10240 + 512 + 32,
              "DESIGN.md 5o states the bytes");

// ---- the obstacle words --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_we_classify(const uint32_t *__restrict__ order, const uint32_t *__restrict__ cells, uint32_t n_arch,
                                                    uint32_t unknown_too, uint32_t static_only, int max_movable, u64 *__restrict__ obst) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (j >= n_arch) return;  // (wave-uniform)
  const uint32_t slot = order[j];
  if (slot >= n_arch) return;  // (never: the pool is dense, n_arch slots are in use; wave-uniform)
  uint32_t w[8];
  load_brick(cells, slot, lane, w);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int occ = occ_of(w[l]);
    const uint32_t track = w[l] & 0xffffu;
    const bool movable = track >= 1u && (int)track <= max_movable;
    const u64 om = __ballot((occ >= 1 && !(static_only && movable)) || (unknown_too && occ == -1));
    if (lane == 0) obst[(size_t)slot * 8u + l] = om;
  }
}

// ---- the build -----------------------------------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(BT) void k_we_build(const uint32_t *__restrict__ coord, const u64 *__restrict__ akeys, const uint32_t *__restrict__ avals,
                                                 uint32_t ahmask, const u64 *__restrict__ obst, uint32_t n_arch, int R, u64 absent_reads,
                                                 uint32_t *__restrict__ field, u64 *__restrict__ meta) {
  constexpr int W = BuildShape<H>::W, S = BuildShape<H>::S, NB = BuildShape<H>::NB;
  __shared__ u64 s_obs[S * W * W];       // [z][brick y][brick x]: the layer word of that brick
  __shared__ u64 s_x[S * S];             // [z][y]: eight signed bytes, dx of the nearest obstacle per column of the brick
  __shared__ uint32_t s_y[S * 64];       // [z][cy][cx]: d2 | dx << 16 | dy << 24
  __shared__ uint32_t s_slot[BuildShape<H>::NB2];
  __shared__ uint32_t s_count[BT / 64][2];  // per wave: obstacle cells, cells within R
  const int tid = (int)threadIdx.x;
  const uint32_t r = blockIdx.x;
  if (tid < NB) {
    int bx, by, bz;
    coord_of(coord, r, bx, by, bz);
    bx += tid % W - H, by += (tid / W) % W - H, bz += tid / (W * W) - H;
    // (a coordinate of 32768 would alias another brick's key)
    const uint32_t slot = brick_in_range(bx, by, bz) ? world_find(akeys, avals, ahmask, brick_key(bx, by, bz)) : NONE;
    s_slot[tid] = slot < n_arch ? slot : NONE;
  }
  __syncthreads();
  for (int i = tid; i < NB * 8; i += BT) {
    const int t = i >> 3, l = i & 7;
    const uint32_t slot = s_slot[t];
    const int bxi = t % W, byi = (t / W) % W, bzi = t / (W * W);
    s_obs[((bzi * 8 + l) * W + byi) * W + bxi] = slot != NONE ? obst[(size_t)slot * 8u + (uint32_t)l] : absent_reads;
  }
  __syncthreads();
  // the rows and layers within R of the brick: base .. base + T - 1 of the halo's 0 .. S - 1 (R <= 8 H: base >= 0)
  const int T = 8 + 2 * R, base = 8 * H - R, R2 = R * R;
  // ---- x: the nearest obstacle of the row on either side of every column of the brick
  for (int i = tid; i < T * T; i += BT) {
    const int z = base + i / T, y = base + i % T;
    const int byi = y >> 3, sh = 8 * (y & 7);
    u64 row = 0ull;
#pragma unroll
    for (int bxi = 0; bxi < W; ++bxi) row |= ((s_obs[(z * W + byi) * W + bxi] >> sh) & 0xffull) << (8 * bxi);
    u64 out = 0ull;
#pragma unroll
    for (int cx = 0; cx < 8; ++cx) {
      const int p = 8 * H + cx;
      const u64 below = row & ((2ull << p) - 1ull), above = row >> p;  // both hold the cell itself
      const int dl = below ? p - (63 - __clzll((long long)below)) : 64, dr = above ? __ffsll((long long)above) - 1 : 64;
      const int dx = dl <= dr ? (dl <= R ? -dl : NO_DX) : (dr <= R ? dr : NO_DX);  // (a tie: the smaller x)
      out |= (u64)(uint32_t)(dx & 0xff) << (8 * cx);
    }
    s_x[z * S + y] = out;
  }
  __syncthreads();
  // ---- y: per (cx, cy) of the brick and layer z, ascending y', replaced only by a strictly smaller sum
  const int8_t *__restrict__ xb = reinterpret_cast<const int8_t *>(s_x);
  for (int e = tid; e < T * 64; e += BT) {
    const int z = base + (e >> 6), cx = e & 7, y = 8 * H + ((e >> 3) & 7);
    int best = (int)NO_D2, bdx = 0, bdy = 0;
    for (int k = -R; k <= R; ++k) {
      const int dx = xb[(z * S + y + k) * 8 + cx];
      const int v = dx * dx + k * k;  // (NO_DX: 16384, above every R^2)
      if (v <= R2 && v < best) best = v, bdx = dx, bdy = k;
    }
    s_y[z * 64 + (e & 63)] = (uint32_t)best | ((uint32_t)(bdx & 0xff) << 16) | ((uint32_t)(bdy & 0xff) << 24);
  }
  __syncthreads();
  // ---- z: per cell, ascending z'; one packed store
  uint32_t n_obst = 0u, n_near = 0u;
  for (int c = tid; c < 512; c += BT) {  // (whole waves: the ballots see every lane)
    const int z = 8 * H + (c >> 6);
    int best = (int)NO_D2, bdx = 0, bdy = 0, bdz = 0;
    for (int k = -R; k <= R; ++k) {
      const uint32_t w = s_y[(z + k) * 64 + (c & 63)];
      const int v = (int)(w & 0xffffu) + k * k;  // (NO_D2: above every R^2)
      if (v <= R2 && v < best) best = v, bdx = (int8_t)(w >> 16), bdy = (int8_t)(w >> 24), bdz = k;
    }
    const bool near = best != (int)NO_D2;
    field[(size_t)r * 512u + (uint32_t)c] =
        near ? (uint32_t)best | ((uint32_t)(bdx + 32) << 10) | ((uint32_t)(bdy + 32) << 16) | ((uint32_t)(bdz + 32) << 22) : PACK_NONE;
    n_near += (uint32_t)__popcll(__ballot(near));
    n_obst += (uint32_t)__popcll(__ballot(best == 0));
  }
  if ((tid & 63) == 0) s_count[tid >> 6][0] = n_obst, s_count[tid >> 6][1] = n_near;
  __syncthreads();
  if (tid < 2) {  // the brick's two counts: one atomic each, on the copy this brick adds to
    uint32_t sum = 0u;
#pragma unroll
    for (int w = 0; w < BT / 64; ++w) sum += s_count[w][tid];
    if (sum) atomicAdd(meta + (size_t)(r & (uint32_t)(E_SPREAD - 1)) * E_PAIR + (uint32_t)tid, (u64)sum);
  }
}

// ---- the query ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_query_world_distance(const float *__restrict__ xyz, const int32_t *__restrict__ cells, uint32_t n, float recip,
                                                             float voxel_size, const u64 *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                             uint32_t hmask, uint32_t n_bricks, const uint32_t *__restrict__ field, uint32_t far_d2,
                                                             uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n) return;
  int g[3];
  const bool ok = entry_cell(xyz, cells, i, recip, g);
  const uint32_t r = ok ? world_find(keys, vals, hmask, brick_key(g[0] >> 3, g[1] >> 3, g[2] >> 3)) : NONE;
  uint32_t d2 = 0xffffffffu;
  int q[3] = {g[0], g[1], g[2]};
  float metres = -1.f;
  if (r < n_bricks) {  // (NONE: in no brick of the field)
    const uint32_t w = field[(size_t)r * 512u + (uint32_t)((g[0] & 7) | ((g[1] & 7) << 3) | ((g[2] & 7) << 6))];
    if ((w & 0x3ffu) == 0x3ffu) {
      d2 = SDM_WORLD_ESDF_FAR;
      metres = sqrtf((float)far_d2) * voxel_size;  // a lower bound: R^2 + 1
    } else {
      d2 = w & 0x3ffu;
      q[0] += (int)((w >> 10) & 63u) - 32, q[1] += (int)((w >> 16) & 63u) - 32, q[2] += (int)((w >> 22) & 63u) - 32;
      metres = sqrtf((float)d2) * voxel_size;
    }
  }
  uint2 *__restrict__ o = out + 4 * (size_t)i;
  o[0] = make_uint2((uint32_t)g[0], (uint32_t)g[1]);
  o[1] = make_uint2((uint32_t)g[2], (uint32_t)q[0]);
  o[2] = make_uint2((uint32_t)q[1], (uint32_t)q[2]);
  o[3] = make_uint2(d2, __float_as_uint(metres));
}

// the buffers for n_arch archived bricks / for `bricks` bricks of the field (the stream is idle when either is called)
sdm_status grow_arch(sdm_map *m, size_t n_arch) {
  WorldEsdfLayer &L = m->wesdf;
  const size_t cap = round_up(n_arch + 1, 256);
  return grow_buffers(m, n_arch + 1, cap, &L.cap_arch, {buf(&L.flag, cap), buf(&L.rank, cap), buf(&L.obst, cap * 8)});
}

sdm_status grow_bricks(sdm_map *m, size_t bricks) {  // (no brick: still a table to look up in)
  WorldEsdfLayer &L = m->wesdf;
  const size_t need = std::max<size_t>(bricks, 1), cap = round_up(need, 256);
  return grow_buffers(m, need, cap, &L.cap_bricks,
                      {buf(&L.coord, cap * 2), buf(&L.field, cap * 512), buf(&L.keys, table_slots(cap)), buf(&L.vals, table_slots(cap))});
}

// the index, the obstacle words and the field of a build of n bricks
hipError_t launch_we_build(const sdm_map *m, const uint32_t *order, uint32_t n_arch, uint32_t n, uint32_t flags, int R) {
  const WorldEsdfLayer &L = m->wesdf;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  hipError_t e;
  if ((e = hipMemsetAsync(L.keys, 0xff, ((size_t)L.hmask + 1) * sizeof(u64), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(L.meta, 0, E_WORDS * sizeof(u64), s)) != hipSuccess) return e;
  if (!n) return hipSuccess;
  const uint32_t unknown_too = (flags & SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE) ? 1u : 0u;
  if ((e = launch_snapshot_index(m, order, L.flag, L.rank, n_arch, n, L.coord, nullptr, L.keys, L.vals, L.hmask)) != hipSuccess) return e;
  LAYER_LAUNCH(k_we_classify, (n_arch + QT / 64 - 1) / (QT / 64), QT, s, order, W.cells, n_arch, unknown_too,
               (flags & SDM_WORLD_ESDF_STATIC_ONLY) ? 1u : 0u, m->d.max_movable, L.obst);
  const u64 absent_reads = unknown_too ? ~0ull : 0ull;
  if (R <= 8)
    LAYER_LAUNCH(k_we_build<1>, n, BT, s, L.coord, W.keys, W.vals, W.hmask, L.obst, n_arch, R, absent_reads, L.field, L.meta);
  else
    LAYER_LAUNCH(k_we_build<2>, n, BT, s, L.coord, W.keys, W.vals, W.hmask, L.obst, n_arch, R, absent_reads, L.field, L.meta);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_ESDF = {"the world distance field", "world distance field", "sdm_world_esdf_update", false};
constexpr size_t GET_CHUNK = 4096;  // bricks a getter unpacks at a time: 8 MB of packed words
}  // namespace

extern "C" {

sdm_status sdm_world_esdf_update(sdm_map *m, const sdm_world_esdf_options *o) {
  const char *what = "sdm_world_esdf_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WE_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->radius < 1u || o->radius > (uint32_t)SDM_WORLD_ESDF_MAX_RADIUS) return LAYER_REFUSE(what, "radius 0 or > 16");
  BrickBox box{};
  if (o->flags & SDM_WORLD_ESDF_BOX) {  // (bmax < bmin: an empty box, a field of no bricks)
    box.use = 1u;
    for (int a = 0; a < 3; ++a) box.lo[a] = o->bmin[a], box.hi[a] = o->bmax[a];
  }
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldEsdfLayer &L = m->wesdf;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, E_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, E_WORDS + 1, true));
  // the bricks of the field: the archive's in brick order, those of the box ranked
  SnapshotBricks b;
  SDM_TRY(snapshot_bricks(m, box, (size_t)m->world.max_bricks + 1, L.h_meta + E_WORDS, [&](uint32_t n_arch, uint32_t **flag, uint32_t **rank) -> sdm_status {
    HIP_TRY(hipStreamSynchronize(s));
    SDM_TRY(grow_arch(m, n_arch));
    *flag = L.flag, *rank = L.rank;
    return SDM_OK;
  }, &b));
  SDM_TRY(grow_bricks(m, b.n));
  L.n = b.n;
  L.hmask = table_slots(b.n) - 1;
  HIP_TRY(launch_we_build(m, b.order, b.n_arch, b.n, o->flags, (int)o->radius));
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, E_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));  // (the getter waits for them)
  L.radius = o->radius;
  L.stamp = m->world.f.gts;
  L.built(m->world.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_esdf(sdm_map *m, int16_t *coords, uint16_t *d2, int8_t *offset, int64_t first, int64_t cap, int64_t *n_out,
                              sdm_world_esdf_info *info) {
  const char *what = "sdm_get_world_esdf";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wesdf, WORLD_ESDF));
  HIP_TRY(hipSetDevice(m->device));
  const WorldEsdfLayer &L = m->wesdf;
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>((int64_t)L.n - first, cap), 0);
  std::vector<uint32_t> pairs(coords ? 2 * take : 0);
  if (take && coords) HIP_TRY(hipMemcpyAsync(pairs.data(), L.coord + 2 * (size_t)first, 2 * take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  unpack_coords(pairs, coords);
  if (take && (d2 || offset)) {  // the packed words, unpacked on the host a chunk of bricks at a time
    std::vector<uint32_t> words(std::min(take, GET_CHUNK) * 512);
    for (size_t at = 0; at < take; at += GET_CHUNK) {
      const size_t c = std::min(GET_CHUNK, take - at);
      HIP_TRY(hipMemcpyAsync(words.data(), L.field + ((size_t)first + at) * 512, c * 512 * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
      HIP_TRY(hipStreamSynchronize(m->stream));
      for (size_t k = 0; k < c * 512; ++k) {
        const uint32_t w = words[k], v = w & 0x3ffu;
        const size_t to = at * 512 + k;
        if (d2) d2[to] = v == 0x3ffu ? (uint16_t)SDM_WORLD_ESDF_NONE : (uint16_t)v;
        if (offset) {
          offset[3 * to] = (int8_t)((int)((w >> 10) & 63u) - 32);
          offset[3 * to + 1] = (int8_t)((int)((w >> 16) & 63u) - 32);
          offset[3 * to + 2] = (int8_t)((int)((w >> 22) & 63u) - 32);
        }
      }
    }
  }
  *n_out = (int64_t)L.n;
  if (info) {
    const u64 *h = L.h_meta;  // (the stream has drained: the build's copy has landed)
    info->n_bricks = L.n;
    info->flags = L.flags;
    info->radius = L.radius;
    info->stamp = L.stamp;
    info->n_obstacle_cells = info->n_near_cells = 0;
    for (int k = 0; k < E_SPREAD; ++k) {
      info->n_obstacle_cells += (int64_t)h[k * E_PAIR + E_OBST];
      info->n_near_cells += (int64_t)h[k * E_PAIR + E_NEAR];
    }
  }
  return SDM_OK;
}

sdm_status sdm_query_world_distance(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_distance_result *out, uint32_t flags) {
  SDM_TRY(goal_query_check(m, xyz, cells, n, out, flags, "sdm_query_world_distance", &sdm_map::wesdf, WORLD_ESDF));
  const WorldEsdfLayer L = m->wesdf;
  const float recip = m->d.recip, voxel_size = m->d.voxel_size;
  const uint32_t far_d2 = L.radius * L.radius + 1u;
  const bool points = xyz != nullptr;
  return run_query(m, points ? (const void *)xyz : (const void *)cells, 12, out, sizeof(sdm_world_distance_result), nullptr, 0, n, flags,
                   [L, recip, voxel_size, far_d2, points](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_world_distance, dim3((c + QT - 1) / QT), dim3(QT), 0, s, points ? static_cast<const float *>(in) : nullptr,
                                        points ? nullptr : static_cast<const int32_t *>(in), c, recip, voxel_size, L.keys, L.vals, L.hmask, L.n, L.field,
                                        far_d2, static_cast<uint2 *>(o));
                   });
}

}  // extern "C"
