// world_rays.hip — world rays: segments and views walked through the bricks of the world archive (gfx950; include/sdm.h,
// "world rays"): sdm_query_world_segments, the archive's counterpart of sdm_query_segments, and sdm_query_world_views, the
// archive's counterpart of sdm_query_views.  Both read the archive live, in stream order, and write only the caller's
// outputs and - the views - a pool of bitmasks of this layer's own, which every call leaves zeroed.
//
// One lane per segment or ray, a 3-D DDA in double through the UNBOUNDED lattice of world cells, in batches of RAY_K
// cells.  As in sdm_walk.h (which this unit does not include: its users' registers are pinned) the cells a ray visits follow
// from its end points alone, so a batch is walked ahead in arithmetic and looked up afterwards.  In the archive a cell is a
// chain of three dependent loads - the hash table's key, the pool slot beside it, the word - so a batch's lookups go
// stage by stage: all first-probe keys and, at the same index, the slots beside them, then all words; two memory round
// trips per RAY_K cells, and no cell's lookup waits for an earlier cell's test.  Every load is unconditional (a cell with
// nothing to load reads entry 0).
// A ray stays in a brick for 8 to 14 cells: a cell whose brick is the previous cell's takes that cell's slot (or NONE) by a
// select, within a batch and - carry_code, carry_slot - across batches, and loads no key.  A first probe that finds
// another brick's key (the table is at most half full) gets a second probe, the batch's together again; what is still
// unresolved takes world_find's loop for that cell: slower, correct.
// The eight words stay in registers: every lane gathers its own 4-byte words, nothing is shared between lanes, and a trip
// through LDS would only add to the latency the batch exists to hide.
// A cell travels as one 64-bit code, (x + 2^19) | (y + 2^19) << 20 | (z + 2^19) << 40: brick key, in-range test, cell word
// and same-brick test are shifts and masks of it.  The walker's state is scalars per axis, never arrays, and no conditional
// operator has two of its members as operands (sdm_walk.h says why).
//   k_world_segments    a lane per segment; the hit's stamp is one header load after the walk.
//   k_world_view_rays   a lane per ray, a block row per view in flight (blockIdx.y = its mask in the pool).  The walk ends
//               at the blocking cell, at b, or where it would leave the window of 2 reach + 1 cells round the view's cell.
//               Marking as in views.hip: the cells to mark follow from the stop mask before any atomic; returned fetch_or
//               atomics of agent scope, all of a batch issued together; a cell counts where the bit was clear; wave sums,
//               then one set of adds per wave.
// The masks are cleared by a memset of the batch's masks, not by a second walk: a second walk would pay the lookups
// of every batch again, while the memset streams at most 64 MiB.
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_segment_hit) == 32 && offsetof(sdm_world_segment_hit, cells) == 4 && offsetof(sdm_world_segment_hit, cell) == 8 &&
                  offsetof(sdm_world_segment_hit, track) == 20 && offsetof(sdm_world_segment_hit, occ) == 23 &&
                  offsetof(sdm_world_segment_hit, unknown) == 24 && offsetof(sdm_world_segment_hit, stamp) == 28,
              "sdm.h layout");
static_assert(sizeof(sdm_view) == 32 && sizeof(sdm_view_gain) == 40, "sdm.h layouts");

namespace sdm {

namespace {

constexpr int RT = 256;
// three waves per SIMD, at most 168 vector registers: what a batch keeps in flight does not fit the 128 of four
#define RAY_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(3, 3)))
constexpr int RAY_K = 8;                 // cells per batch (SEG_K of sdm_walk.h)
constexpr int CELL_BIAS = 1 << 19;       // a world cell is in [-2^18, 2^18) per axis; one step beyond still fits 20 bits
constexpr u64 SUB_MASK = 7ull | (7ull << 20) | (7ull << 40);  // the cell inside its brick
constexpr u64 NO_CODE = ~0ull;           // in no brick of any cell's
constexpr float CELL_LO = -262144.f, CELL_HI = 262144.f;  // floorf(u) of a cell whose brick is in the int16 range: [LO, HI)
constexpr uint32_t ALL_SEG_FLAGS = SDM_QUERY_ON_DEVICE | SDM_QUERY_UNKNOWN_BLOCKS | SDM_WORLD_RAYS_IGNORE_MOVABLE;
constexpr uint32_t ALL_VIEW_FLAGS = SDM_QUERY_ON_DEVICE | SDM_WORLD_RAYS_IGNORE_MOVABLE;

// the archive as the kernels read it, by value
struct Arch {
  const u64 *keys;
  const uint32_t *vals, *cells, *hdr;
  uint32_t hmask, max_bricks;
};

// ---- the walk ------------------------------------------------------------------------------------------------------
struct RayAxis {
  int c;              // the current cell's coordinate
  int c0;             // the view's cell: the middle of the window (views only)
  double A, inv, tn;  // u_a; 1 / (u_b - u_a), 0 where the ray is parallel to the planes; the t of the next plane
};
// -1, 0, +1: the way the ray goes - the sign of inv, not kept in a register of its own
__device__ __forceinline__ int ray_step(double inv) { return (inv > 0.0) - (inv < 0.0); }
struct RayWalk {
  RayAxis x, y, z;
  bool live;     // there is a current cell
};

__device__ __forceinline__ void ray_axis_begin(RayAxis &s, float ua, float ub) {
  s.c = (int)floorf(ua);  // (the caller has checked the range)
  s.c0 = s.c;
  s.A = (double)ua;
  const double D = (double)ub - s.A;
  s.inv = D == 0.0 ? 0.0 : 1.0 / D;
  s.tn = D == 0.0 ? INFINITY : ((double)(s.c + (D > 0.0)) - s.A) * s.inv;
}
__device__ __forceinline__ void ray_begin(RayWalk &w, const float (&ua)[3], const float (&ub)[3]) {
  ray_axis_begin(w.x, ua[0], ub[0]);
  ray_axis_begin(w.y, ua[1], ub[1]);
  ray_axis_begin(w.z, ua[2], ub[2]);
  w.live = true;
}

// one of three by the axis; by value, so that nothing ever selects between two addresses
template <typename T>
__device__ __forceinline__ T ray_pick(int ax, T x, T y, T z) {
  return ax == 0 ? x : ax == 1 ? y : z;
}
__device__ __forceinline__ void ray_cross(RayAxis &s, bool here, int cn, double tn) {
  if (here) {
    s.c = cn;
    s.tn = tn;
  }
}
// entry i of a table of fewer than 2^32 bytes: the base stays in scalar registers, the lane carries a 32-bit byte offset -
// half the address registers of a batch's 24 loads in flight
template <typename T>
__device__ __forceinline__ T load_at(const T *__restrict__ base, uint32_t i) {
  return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + (uint32_t)(i * (uint32_t)sizeof(T)));
}
__device__ __forceinline__ u64 cell_code(int x, int y, int z) {
  return (u64)(uint32_t)(x + CELL_BIAS) | ((u64)(uint32_t)(y + CELL_BIAS) << 20) | ((u64)(uint32_t)(z + CELL_BIAS) << 40);
}
__device__ __forceinline__ int code_x(u64 c) { return (int)((uint32_t)c & 0xfffffu) - CELL_BIAS; }
__device__ __forceinline__ int code_y(u64 c) { return (int)((uint32_t)(c >> 20) & 0xfffffu) - CELL_BIAS; }
__device__ __forceinline__ int code_z(u64 c) { return (int)((uint32_t)(c >> 40) & 0xfffffu) - CELL_BIAS; }
// the brick coordinate + 65536 of every axis: in the int16 range iff in [32768, 98304)
__device__ __forceinline__ bool code_in_range(u64 c) {
  const uint32_t kx = ((uint32_t)c & 0xfffffu) >> 3, ky = ((uint32_t)(c >> 20) & 0xfffffu) >> 3, kz = ((uint32_t)(c >> 40) & 0xfffffu) >> 3;
  return kx - 32768u < 65536u && ky - 32768u < 65536u && kz - 32768u < 65536u;
}
// brick_key of the cell's brick (of a cell in range)
__device__ __forceinline__ u64 code_key(u64 c) {
  const uint32_t kx = ((uint32_t)c & 0xfffffu) >> 3, ky = ((uint32_t)(c >> 20) & 0xfffffu) >> 3, kz = ((uint32_t)(c >> 40) & 0xfffffu) >> 3;
  return (u64)((kx - 32768u) & 0xffffu) | ((u64)((ky - 32768u) & 0xffffu) << 16) | ((u64)((kz - 32768u) & 0xffffu) << 32);
}
__device__ __forceinline__ uint32_t code_word(u64 c) {
  return ((uint32_t)c & 7u) | (((uint32_t)(c >> 20) & 7u) << 3) | (((uint32_t)(c >> 40) & 7u) << 6);
}

// From the current cell to the next: `code` becomes the current cell's (left alone where there is none).  Crossing
// parameters are computed fresh from the end points; x steps before y before z at equal t.  WINDOW: a step that would leave
// the window ends the walk instead.  No branch: every lane of a wave runs the same RAY_K steps of a batch.
template <bool WINDOW>
__device__ __forceinline__ void ray_advance(RayWalk &w, u64 &code, int reach) {
  const bool go = w.live;
  const u64 here = cell_code(w.x.c, w.y.c, w.z.c);
  if (go) code = here;
  int ax = 0;
  double tm = w.x.tn;
  if (w.y.tn < tm) { ax = 1; tm = w.y.tn; }
  if (w.z.tn < tm) { ax = 2; tm = w.z.tn; }
  const bool on = go && !(tm > 1.0);  // (otherwise the ray ends in this cell)
  const double inv = ray_pick(ax, w.x.inv, w.y.inv, w.z.inv);
  const int step = ray_step(inv);
  const int cn = ray_pick(ax, w.x.c, w.y.c, w.z.c) + step;
  const double tn = ((double)(cn + (step > 0)) - ray_pick(ax, w.x.A, w.y.A, w.z.A)) * inv;
  bool out = false;
  if (WINDOW) out = (uint32_t)(cn - ray_pick(ax, w.x.c0, w.y.c0, w.z.c0) + reach) > 2u * (uint32_t)reach;
  ray_cross(w.x, on && ax == 0, cn, tn);
  ray_cross(w.y, on && ax == 1, cn, tn);
  ray_cross(w.z, on && ax == 2, cn, tn);
  w.live = on && !out;
}

// The t at which the walk entered cell (x, y, z): the largest crossing parameter of the planes it came in through, one per
// axis that has left the first cell's coordinate - the very expression, on the very operands, that gave the walk its tn
// for that plane, so this is bit for bit the t of the crossing; 0 in the first cell.  (The crossings' t never decrease: the
// expression is monotone in the plane.)  It spares a batch the RAY_K entry parameters it would carry for one hit.
__device__ __forceinline__ double ray_axis_entry(const RayAxis &s, int c) {
  if (c == (int)floor(s.A)) return 0.0;
  return ((double)(c + (s.inv < 0.0)) - s.A) * s.inv;
}
__device__ __forceinline__ float ray_entry_t(const RayWalk &w, u64 code) {
  return (float)fmax(fmax(ray_axis_entry(w.x, code_x(code)), ray_axis_entry(w.y, code_y(code))), ray_axis_entry(w.z, code_z(code)));
}

// The next RAY_K cells and their words.  Returns the mask of the batch's entries that are cells (a prefix of it); per
// entry the cell's code, its word's index in the pool (slot * 512 + cell word; NONE: the
// archive has no such brick, or the brick lies beyond the int16 range) and its word (the unknown word there).  carry_code /
// carry_slot: the last cell of the batch before and its brick's slot, NO_CODE before the first.
// The slot beside a first-probe key is loaded WITH the key, not behind it - both addresses follow from the hash alone -,
// so a batch is two memory round trips: keys and slots, then words.
template <bool WINDOW>
__device__ __forceinline__ uint32_t ray_batch(RayWalk &w, int reach, const Arch &A, u64 &carry_code, uint32_t &carry_slot, u64 (&code)[RAY_K],
                                              uint32_t (&at)[RAY_K], uint32_t (&word)[RAY_K]) {
  uint32_t live = 0u;
  u64 prev = carry_code;
#pragma unroll
  for (int k = 0; k < RAY_K; ++k) {  // arithmetic only
    live |= (uint32_t)w.live << k;
    code[k] = prev;  // (an entry that is no cell repeats the last cell)
    ray_advance<WINDOW>(w, code[k], reach);
    prev = code[k];
  }
  // stage 1: the first-probe key, and the slot beside it, of every cell that enters a brick (the others read entry 0)
  uint32_t v1[RAY_K], fresh = 0u, inr = 0u;
  u64 k1[RAY_K];
  prev = carry_code;
#pragma unroll
  for (int k = 0; k < RAY_K; ++k) {
    const uint32_t in = code_in_range(code[k]) ? 1u : 0u;  // (brick_in_range, before every lookup)
    const uint32_t f = ((live >> k) & 1u) & in & (((code[k] ^ prev) & ~SUB_MASK) != 0ull ? 1u : 0u);
    inr |= in << k;
    fresh |= f << k;
    const uint32_t h = (key_hash(code_key(code[k])) & A.hmask) & (0u - f);
    k1[k] = load_at(A.keys, h);
    v1[k] = load_at(A.vals, h);
    prev = code[k];
  }
  uint32_t collided = 0u;
#pragma unroll
  for (int k = 0; k < RAY_K; ++k) {
    const uint32_t f = (fresh >> k) & 1u, match = f & (k1[k] == code_key(code[k]) ? 1u : 0u);
    collided |= (f & (match ^ 1u) & (k1[k] != EMPTY_KEY ? 1u : 0u)) << k;
    v1[k] |= match - 1u;  // (NONE without a match)
  }
  if (collided) {  // another brick's key at the first probe: the second probes, together again, in two halves of the batch
#pragma unroll
    for (int k0 = 0; k0 < RAY_K; k0 += RAY_K / 2) {
      u64 k2[RAY_K / 2];
      uint32_t v2[RAY_K / 2];
#pragma unroll
      for (int j = 0; j < RAY_K / 2; ++j) {
        const uint32_t h = ((key_hash(code_key(code[k0 + j])) + 1u) & A.hmask) & (0u - ((collided >> (k0 + j)) & 1u));
        k2[j] = load_at(A.keys, h);
        v2[j] = load_at(A.vals, h);
      }
#pragma unroll
      for (int j = 0; j < RAY_K / 2; ++j) {
        const int k = k0 + j;
        const uint32_t c = (collided >> k) & 1u, match = c & (k2[j] == code_key(code[k]) ? 1u : 0u), empty = c & (k2[j] == EMPTY_KEY ? 1u : 0u);
        const uint32_t mm = 0u - match;
        v1[k] = (v2[j] & mm) | (v1[k] & ~mm);
        collided &= ~((match | empty) << k);
      }
    }
  }
  while (collided) {  // ... and whatever is left walks the probe sequence, one such cell at a time
    const int kk = __builtin_ctz(collided);
    collided &= collided - 1u;
    u64 key = 0ull;
#pragma unroll
    for (int k = 0; k < RAY_K; ++k)  // (selected by compile-time index: no register array indexed at run time)
      if (k == kk) key = code_key(code[k]);
    const uint32_t found = world_find(A.keys, A.vals, A.hmask, key);
#pragma unroll
    for (int k = 0; k < RAY_K; ++k)
      if (k == kk) v1[k] = found;
  }
  // stage 2: the words; a cell in the previous cell's brick has that cell's slot
  uint32_t s = carry_slot;
#pragma unroll
  for (int k = 0; k < RAY_K; ++k) {
    const uint32_t fm = 0u - ((fresh >> k) & 1u);
    const uint32_t p = v1[k] < A.max_bricks ? v1[k] : NONE;
    s = (p & fm) | (s & ~fm);
    s |= ((inr >> k) & 1u) - 1u;  // (NONE beyond the int16 range)
    const uint32_t have = 0u - (((live >> k) & 1u) & (s != NONE ? 1u : 0u));
    at[k] = (s * 512u + code_word(code[k])) | ~have;
    const uint32_t v = load_at(A.cells, at[k] & have);
    word[k] = (v & have) | (RES_UNKNOWN_W1 & ~have);
  }
  carry_code = code[RAY_K - 1];
  carry_slot = s;
  return live;
}

// what a batch's words say: bit k set where cell k blocks / reads unknown
__device__ __forceinline__ void ray_classes(const uint32_t (&word)[RAY_K], uint32_t live, uint32_t unknown_blocks, uint32_t ignore_movable,
                                            int max_movable, uint32_t &blocked, uint32_t &unk) {
  blocked = unk = 0u;
#pragma unroll
  for (int k = 0; k < RAY_K; ++k) {
    const int occ = occ_of(word[k]);
    const uint32_t track = word[k] & 0xffffu;
    const bool movable = track >= 1u && (int)track <= max_movable;
    const bool b = (occ >= 1 && !(ignore_movable && movable)) || (unknown_blocks && occ == -1);
    blocked |= (uint32_t)(b && ((live >> k) & 1u)) << k;
    unk |= (uint32_t)(occ == -1 && ((live >> k) & 1u)) << k;
  }
}

// one result, in four 8-byte stores
__device__ __forceinline__ void store_hit(uint2 *__restrict__ o, float t, int cells, bool hit, u64 code, uint32_t word, uint32_t unknown, uint32_t stamp) {
  o[0] = make_uint2(__float_as_uint(t), (uint32_t)cells);
  o[1] = make_uint2(hit ? (uint32_t)code_x(code) : 0u, hit ? (uint32_t)code_y(code) : 0u);
  o[2] = make_uint2(hit ? (uint32_t)code_z(code) : 0u, word);
  o[3] = make_uint2(unknown, stamp);
}

// ---- segments ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) RAY_WAVES_ATTR void k_world_segments(const float *__restrict__ ab, uint32_t n, float recip, Arch A, uint32_t unknown_blocks,
                                                       uint32_t ignore_movable, int max_movable, uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * RT + threadIdx.x;
  if (i >= n) return;
  float ua[3], ub[3];
  bool valid = true;
  int span = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ua[a] = ab[6 * (size_t)i + a] * recip;
    ub[a] = ab[6 * (size_t)i + 3 + a] * recip;
    const float fa = floorf(ua[a]), fb = floorf(ub[a]);
    const bool in = fa >= CELL_LO && fa < CELL_HI && fb >= CELL_LO && fb < CELL_HI;  // (NaN and inf fail; the casts see values in range only)
    const int d = in ? (int)fb - (int)fa : 0;
    span += d < 0 ? -d : d;
    valid = valid && in;
  }
  const bool too_long = valid && span > SDM_WORLD_SEGMENT_MAX_CELLS;
  float hit_t = -1.f;
  int cells = too_long ? -1 : 0;
  bool hit = false;
  u64 hit_code = 0ull;
  uint32_t hit_w = RES_UNKNOWN_W1, hit_at = NONE, unknown = 0u;
  RayWalk w;
  w.live = false;
  if (!valid) {
    if (unknown_blocks) hit_t = 0.f;
  } else if (!too_long) {
    ray_begin(w, ua, ub);
  }
  u64 carry_code = NO_CODE;
  uint32_t carry_slot = NONE;
  while (w.live) {
    u64 code[RAY_K];
    uint32_t at[RAY_K], word[RAY_K], blocked, unk;
    const uint32_t live = ray_batch<false>(w, 0, A, carry_code, carry_slot, code, at, word);
    ray_classes(word, live, unknown_blocks, ignore_movable, max_movable, blocked, unk);
    const uint32_t stop = blocked | (~live & ((1u << RAY_K) - 1u));
    const int first = stop ? __builtin_ctz(stop) : RAY_K;
    const bool h = stop && ((blocked >> first) & 1u);
    const int nm = first + (h ? 1 : 0);  // cells of this batch the segment visits, the blocking one included
    cells += nm;
    unknown += (uint32_t)__popc(unk & ((1u << nm) - 1u));
    if (!stop) continue;
    if (h) {
      hit = true;
#pragma unroll
      for (int k = 0; k < RAY_K; ++k)  // (selected by compile-time index: no register array indexed at run time)
        if (k == first) {
          hit_code = code[k];
          hit_w = word[k];
          hit_at = at[k];
        }
    }
    break;
  }
  if (hit) hit_t = ray_entry_t(w, hit_code);
  const uint32_t stamp = hit && hit_at != NONE ? A.hdr[(size_t)(hit_at >> 9) * HDR_WORDS + 4] : 0u;
  store_hit(out + 4 * (size_t)i, hit_t, cells, hit, hit_code, hit_w, unknown, stamp);
}

// ---- views -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT) RAY_WAVES_ATTR void k_world_view_rays(const sdm_view *__restrict__ views, const float *__restrict__ dirs, uint32_t n_rays,
                                                        float recip, int reach, Arch A, uint32_t ignore_movable, int max_movable,
                                                        uint32_t *__restrict__ pool, uint32_t mask_words, sdm_view_gain *__restrict__ gain,
                                                        uint2 *__restrict__ rays_out) {
  const uint32_t r = blockIdx.x * RT + threadIdx.x;
  const uint32_t v = blockIdx.y;
  const bool lane = r < n_rays;
  uint32_t *__restrict__ mask = pool + (size_t)v * mask_words;
  // the ray: a = pos, b = pos + range * (R(q) d), float32, one operation at a time (sdm.h pins the order)
  const float px = views[v].pos[0], py = views[v].pos[1], pz = views[v].pos[2];
  const float qw = views[v].q[0], qx = views[v].q[1], qy = views[v].q[2], qz = views[v].q[3];
  const float range = views[v].range;
  float dx = 0.f, dy = 0.f, dz = 0.f;
  if (lane) {
    dx = dirs[3 * (size_t)r];
    dy = dirs[3 * (size_t)r + 1];
    dz = dirs[3 * (size_t)r + 2];
  }
  bool view_ok = isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(qw) && isfinite(qx) && isfinite(qy) && isfinite(qz) && isfinite(range);
  const float R[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qw * qz), 2.f * (qx * qz + qw * qy),
                      2.f * (qx * qy + qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qw * qx),
                      2.f * (qx * qz - qw * qy), 2.f * (qy * qz + qw * qx), 1.f - 2.f * (qx * qx + qy * qy)};
  const float pa[3] = {px, py, pz};
  float ua[3], ub[3];
  bool ray_ok = lane && isfinite(dx) && isfinite(dy) && isfinite(dz);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float rd = (R[3 * a] * dx + R[3 * a + 1] * dy) + R[3 * a + 2] * dz;
    const float pb = range > 0.f ? pa[a] + range * rd : pa[a];  // (range <= 0: the zero-length segment, the cell of a)
    ua[a] = pa[a] * recip;
    ub[a] = pb * recip;
    const float fa = floorf(ua[a]);
    // the window's bricks lie in the int16 range (NaN and inf fail; the cast sees values in range only)
    view_ok = view_ok && fa - (float)reach >= CELL_LO && fa + (float)reach < CELL_HI;
    ray_ok = ray_ok && isfinite(ub[a]);
  }
  float hit_t = -1.f;
  int cells = 0;
  bool hit = false;
  u64 hit_code = 0ull;
  uint32_t hit_w = RES_UNKNOWN_W1, hit_at = NONE;
  uint32_t n_unk = 0u, n_free = 0u, n_occ = 0u, r_unk = 0u;
  RayWalk w;
  w.live = false;
  w.x.c0 = w.y.c0 = w.z.c0 = 0;
  if (view_ok && ray_ok) ray_begin(w, ua, ub);
  const uint32_t S = 2u * (uint32_t)reach + 1u;
  u64 carry_code = NO_CODE;
  uint32_t carry_slot = NONE;
  while (w.live) {
    u64 code[RAY_K];
    uint32_t at[RAY_K], word[RAY_K], blocked, unk;
    const uint32_t live = ray_batch<true>(w, reach, A, carry_code, carry_slot, code, at, word);
    ray_classes(word, live, 0u, ignore_movable, max_movable, blocked, unk);
    const uint32_t stop = blocked | (~live & ((1u << RAY_K) - 1u));
    const int first = stop ? __builtin_ctz(stop) : RAY_K;
    const bool h = stop && ((blocked >> first) & 1u);
    const int nm = first + (h ? 1 : 0);  // cells of this batch the ray visits: all in the window, the last one may block
    uint32_t old[RAY_K], sh[2] = {0u, 0u};  // (the bits' places in their words, a byte each)
#pragma unroll
    for (int k = 0; k < RAY_K; ++k) {  // up to RAY_K returned atomics in flight
      const uint32_t bit = ((uint32_t)(code_z(code[k]) - w.z.c0 + reach) * S + (uint32_t)(code_y(code[k]) - w.y.c0 + reach)) * S +
                           (uint32_t)(code_x(code[k]) - w.x.c0 + reach);
      sh[k >> 2] |= (bit & 31u) << (8 * (k & 3));
      old[k] = 0xffffffffu;
      if (k < nm && (bit >> 5) < mask_words)  // (never beyond: the walk ends before it leaves the window)
        old[k] = __hip_atomic_fetch_or(mask + (bit >> 5), 1u << (bit & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint32_t fresh = 0u;
#pragma unroll
    for (int k = 0; k < RAY_K; ++k) fresh |= (uint32_t)(k < nm && !((old[k] >> ((sh[k >> 2] >> (8 * (k & 3))) & 31u)) & 1u)) << k;
    const uint32_t visited = (1u << nm) - 1u;
    n_occ += (uint32_t)__popc(fresh & blocked);
    n_unk += (uint32_t)__popc(fresh & unk & ~blocked);
    n_free += (uint32_t)__popc(fresh & ~unk & ~blocked);
    r_unk += (uint32_t)__popc(unk & visited);
    cells += nm;
    if (!stop) continue;
    if (h) {
      hit = true;
#pragma unroll
      for (int k = 0; k < RAY_K; ++k)  // (selected by compile-time index: no register array indexed at run time)
        if (k == first) {
          hit_code = code[k];
          hit_w = word[k];
          hit_at = at[k];
        }
    }
    break;
  }
  if (hit) hit_t = ray_entry_t(w, hit_code);
  if (lane && rays_out) {
    const uint32_t stamp = hit && hit_at != NONE ? A.hdr[(size_t)(hit_at >> 9) * HDR_WORDS + 4] : 0u;
    store_hit(rays_out + 4 * ((size_t)v * n_rays + r), hit_t, cells, hit, hit_code, hit_w, r_unk, stamp);
  }
  // the wave's sums (lanes past the last ray carry zeros), one set of adds per wave that has anything
  const uint32_t s_unk = wave_sum(n_unk), s_free = wave_sum(n_free), s_occ = wave_sum(n_occ);
  const uint32_t s_hit = wave_sum((uint32_t)hit), s_in = wave_sum((uint32_t)(cells > 0));
  const uint32_t s_cells = wave_sum((uint32_t)cells), s_runk = wave_sum(r_unk);
  if ((threadIdx.x & 63u) == 0 && s_cells) {
    sdm_view_gain *g = gain + v;
    if (s_unk) atomicAdd(&g->n_unknown, s_unk);
    if (s_free) atomicAdd(&g->n_free, s_free);
    if (s_occ) atomicAdd(&g->n_occupied, s_occ);
    if (s_hit) atomicAdd(&g->rays_hit, s_hit);
    atomicAdd(&g->rays_in_map, s_in);
    atomicAdd(reinterpret_cast<unsigned long long *>(&g->ray_cells), (unsigned long long)s_cells);
    if (s_runk) atomicAdd(reinterpret_cast<unsigned long long *>(&g->ray_unknown), (unsigned long long)s_runk);
  }
}

constexpr size_t RAYS_POOL_BYTES = (size_t)64 << 20;  // what the pool may take: at least three masks at the largest reach
constexpr uint32_t RAYS_POOL_MASKS = 256;
constexpr size_t RAYS_CHUNK_RAYS = (size_t)1 << 20;   // host mode: rays per staged chunk (whole views; at least one)

Arch arch_of(const sdm_map *m) {
  const WorldLayer &W = m->world;
  return Arch{W.keys, W.vals, W.cells, W.hdr, W.hmask, W.max_bricks};
}

// `n` views from device memory, in batches of as many as the pool may hold masks (or the test hook allows)
sdm_status world_views_enqueue(sdm_map *m, const sdm_view *views, const float *dirs, uint32_t n_rays, size_t n, int reach, sdm_view_gain *out,
                               sdm_world_segment_hit *rays_out, uint32_t flags) {
  WorldRaysPool &P = m->wrays;
  const size_t S = 2 * (size_t)reach + 1;
  const uint32_t mask_words = (uint32_t)((S * S * S + 31) / 32);
  const size_t mask_bytes = (size_t)mask_words * 4;
  const uint32_t masks = (uint32_t)std::min<size_t>(RAYS_POOL_MASKS, RAYS_POOL_BYTES / mask_bytes);
  const uint32_t B = (uint32_t)std::min<size_t>(P.batch > 0 ? std::min<uint32_t>(masks, (uint32_t)P.batch) : masks, n);
  if ((size_t)B * mask_words > P.words) {  // (the old pool goes once the calls that use it have run; it was all zero)
    SDM_TRY(regrow(m, &P.pool, &P.words, (size_t)B * mask_words, P.pool ? m->stream : nullptr));
    HIP_TRY(hipMemsetAsync(P.pool, 0, P.words * 4, m->stream));  // zero; every call leaves it zero again
  }
  const Arch A = arch_of(m);
  const uint32_t ignore_movable = (flags & SDM_WORLD_RAYS_IGNORE_MOVABLE) ? 1u : 0u;
  HIP_TRY(hipMemsetAsync(out, 0, n * sizeof(sdm_view_gain), m->stream));
  for (size_t v0 = 0; v0 < n; v0 += B) {
    const uint32_t nb = (uint32_t)std::min<size_t>(B, n - v0);
    const dim3 grid((n_rays + RT - 1) / RT, nb);
    hipLaunchKernelGGL(k_world_view_rays, grid, dim3(RT), 0, m->stream, views + v0, dirs, n_rays, m->d.recip, reach, A, ignore_movable,
                       m->d.max_movable, P.pool, mask_words, out + v0, rays_out ? reinterpret_cast<uint2 *>(rays_out + v0 * n_rays) : nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(P.pool, 0, (size_t)nb * mask_bytes, m->stream));
  }
  return SDM_OK;
}

}  // namespace

}  // namespace sdm

extern "C" {

sdm_status sdm_query_world_segments(sdm_map *m, const float *ab, int64_t n, sdm_world_segment_hit *out, uint32_t flags) {
  const char *what = "sdm_query_world_segments";
  SDM_TRY(query_check(m, ab, n, out, flags, ALL_SEG_FLAGS, what));
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  const Arch A = arch_of(m);
  const float recip = m->d.recip;
  const int max_movable = m->d.max_movable;
  const uint32_t unknown_blocks = (flags & SDM_QUERY_UNKNOWN_BLOCKS) ? 1u : 0u, ignore_movable = (flags & SDM_WORLD_RAYS_IGNORE_MOVABLE) ? 1u : 0u;
  return run_query(m, ab, 24, out, sizeof(sdm_world_segment_hit), nullptr, 0, n, flags,
                   [A, recip, max_movable, unknown_blocks, ignore_movable](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_world_segments, dim3((c + RT - 1) / RT), dim3(RT), 0, s, static_cast<const float *>(in), c, recip, A,
                                        unknown_blocks, ignore_movable, max_movable, static_cast<uint2 *>(o));
                   });
}

sdm_status sdm_query_world_views(sdm_map *m, const sdm_view *views, int64_t n_views, const float *dirs, int32_t n_rays, int32_t reach_cells,
                                 sdm_view_gain *out, sdm_world_segment_hit *rays_out, uint32_t flags) {
  const char *what = "sdm_query_world_views";
  SDM_TRY(query_check(m, views, n_views, out, flags, ALL_VIEW_FLAGS, what));
  if (!dirs || n_rays < 1 || n_rays > SDM_VIEW_MAX_RAYS || n_views > (((int64_t)1 << 31) - 1) / n_rays)
    return LAYER_REFUSE(what, "null ray table, n_rays outside 1 .. 65536, or n_views * n_rays >= 2^31");
  if (reach_cells < 1 || reach_cells > SDM_WORLD_VIEW_MAX_REACH) return LAYER_REFUSE(what, "reach_cells outside 1 .. 255");
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  if (n_views == 0) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  const size_t n = (size_t)n_views, nr = (size_t)n_rays;
  if (flags & SDM_QUERY_ON_DEVICE) return world_views_enqueue(m, views, dirs, (uint32_t)n_rays, n, reach_cells, out, rays_out, flags);
  // host mode: the ray table goes up once, the views in chunks of whole views through the queries' staging area
  return run_staged(m, n, std::min(n, std::max<size_t>(1, RAYS_CHUNK_RAYS / nr)), dirs, nr * 12,
                    {{StageCol::IN, const_cast<sdm_view *>(views), sizeof(sdm_view)},
                     {StageCol::OUT, out, sizeof(sdm_view_gain)},
                     {StageCol::OUT, rays_out, rays_out ? nr * sizeof(sdm_world_segment_hit) : 0}},
                    [&](const unsigned char *pre, unsigned char *const *col, size_t c) {
                      return world_views_enqueue(m, reinterpret_cast<const sdm_view *>(col[0]), reinterpret_cast<const float *>(pre), (uint32_t)n_rays,
                                                 c, reach_cells, reinterpret_cast<sdm_view_gain *>(col[1]),
                                                 reinterpret_cast<sdm_world_segment_hit *>(col[2]), flags);
                    });
}

sdm_status sdm_debug_world_view_batch(sdm_map *m, int32_t max_views_in_flight) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->wrays.batch = max_views_in_flight > 0 ? max_views_in_flight : 0;
  return SDM_OK;
}

}  // extern "C"
