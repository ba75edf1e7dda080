// world_match.hip — foreign bricks scored against the world archive under every whole-cell offset of a small window
// (gfx950; include/sdm.h, "world match": sdm_world_match).  The table and the pool are world.hip's, the source table is
// world_io.hip's (sdm_world.h); the archive is read live on the map's stream and never written.
//
// A candidate offset is centre + d, |d[a]| <= r[a].  For source brick b the destinations under all candidates lie in a
// window of E = 8 + 2 r cells per axis from world cell 8 b + centre - r: at most 24^3 cells over at most 4 x 4 x 4 archive
// bricks, and (centre - r) & 7, where the window begins inside its first brick, is the same for every source brick.
//   launch_world_sources   world_io.hip's source table: key -> the lowest source index with these coordinates.
//   k_wmt_score    a workgroup per run of source bricks and per 256 candidates.  Per source brick that stayed in the
//                  table: its 512 words become an occupied and a free plane by ballot (eight 64-bit z-layers each) and a
//                  list of its occupied cells with their label bytes, by layer; a brick without a counted cell ends
//                  there.  Threads 0 .. 63 look the window's archive bricks up (one world_find each); a window over no
//                  brick ends there.  The window's words are loaded once - a lane per cell, 8, 16 or 32 lanes per row
//                  along x - and classified: an occupied and a free row word by ballot, the label bytes beside them, all
//                  in LDS.  A candidate's four class counts are popcounts of a source layer AND the eight rows its shift
//                  selects; n_same goes over the listed occupied cells, one row word and one label byte per cell.  With
//                  256 candidates a thread has one; a workgroup with C < 256 gives each P = 256 / C threads, which share
//                  its layers and, from P = 16 on, a layer's listed cells.  The sums stay in registers over the run;
//                  shared candidates meet in LDS, then one atomicAdd per candidate and count.
//   k_wmt_reduce   one workgroup: offsets and counts into the caller's records, the best candidate under the tie rule,
//                  the runner-up, the totals.
// The atomics are the source table's CAS and atomicMin and uint32 adds: all commute.  No floating point anywhere.
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_match_options) == 56 && offsetof(sdm_world_match_options, radius) == 16 &&
                  offsetof(sdm_world_match_options, w_oo) == 28 && offsetof(sdm_world_match_options, pad) == 48 &&
                  sizeof(sdm_world_match_score) == 32 && offsetof(sdm_world_match_score, n_same) == 28 &&
                  sizeof(sdm_world_match_result) == 56 && offsetof(sdm_world_match_result, best_score) == 16 &&
                  offsetof(sdm_world_match_result, best) == 32 && offsetof(sdm_world_match_result, pad) == 48,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr uint32_t MATCH_FLAGS = ALL_FLAGS | SDM_WORLD_MATCH_ON_DEVICE;
constexpr int64_t MAX_SOURCES = (int64_t)1 << 21;
constexpr int MAX_OFFSET = 1 << 19;
constexpr int MT = 256;                              // threads of a workgroup: the candidates of one
constexpr int WIN = 8 + 2 * SDM_WORLD_MATCH_MAX_RADIUS;  // 24: the window's cells per axis at most, and the stride of its rows
constexpr int FILL_U = 4;                            // window words a thread has in flight
constexpr uint32_t MAX_RUNS = 1536;                  // workgroups along the sources at most
enum { T_SOURCES = 0, T_OCC, T_FREE, T_WORDS = 4 };  // the totals

struct MatchGeo {      // a match's geometry, by value
  int c[3], r[3];      // the centre offset, the radius
  int nd[3];           // 2 r + 1: candidates per axis
  int E[3];            // 8 + 2 r: the window's cells per axis
  int res[3];          // (c - r) & 7: where the window begins inside its first archive brick
  int nbk[3];          // the archive bricks the window spans per axis, 1 .. 4
  uint32_t xlg;        // 3, 4 or 5: a row of the window takes 2^xlg lanes, the least that hold E[0]
  uint32_t inv_ey;     // ceil(2^16 / E[1]): row / E[1] == row * inv_ey >> 16 for every row a step can name (< 2730: at most 576 + 128)
  int w[5];            // the weights of n_oo, n_same, n_of, n_fo, n_ff
  uint32_t ncand, n, run;  // candidates, source bricks, source bricks per workgroup
  uint32_t smask, hmask, flags;
  int max_movable;
};

// candidate k as the shift (d + r) per axis
__device__ __forceinline__ void candidate(const MatchGeo &g, uint32_t k, int (&sh)[3]) {
  const uint32_t nx = (uint32_t)g.nd[0], ny = (uint32_t)g.nd[1];
  const uint32_t t = k / nx;
  sh[0] = (int)(k - t * nx);
  sh[2] = (int)(t / ny);
  sh[1] = (int)(t - (uint32_t)sh[2] * ny);
}
// 0 unknown, 1 free, 2 occupied: the class of a word on either side
__device__ __forceinline__ uint32_t word_class(uint32_t w, uint32_t flags, int max_movable) {
  if (!cell_writes(w, flags, max_movable)) return 0u;
  return occ_of(w) >= 1 ? 2u : 1u;
}

// (six waves a SIMD, six workgroups a CU: at most 80 VGPRs; MAX_RUNS is what 256 CUs then hold at once)
#define MATCH_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(6, 8)))
__global__ __launch_bounds__(MT) MATCH_WAVES_ATTR void k_wmt_score(MatchGeo g, const uint32_t *__restrict__ src_hdr,
                                                                   const uint32_t *__restrict__ src_cells, const u64 *__restrict__ skeys,
                                                                   const uint32_t *__restrict__ svals, const u64 *__restrict__ keys,
                                                                   const uint32_t *__restrict__ vals, const uint32_t *__restrict__ cells,
                                                                   uint32_t *__restrict__ acc, uint32_t *__restrict__ totals) {
  __shared__ uint32_t s_wocc[WIN * WIN], s_wfree[WIN * WIN];  // the window's rows along x, [z][y]
  __shared__ uint8_t s_wlab[WIN * WIN * WIN];                 // its label bytes, [z][y][x]
  __shared__ u64 s_socc[8], s_sfree[8];                       // the source brick's planes, a z-layer each
  __shared__ uint16_t s_ent[512];                             // its occupied cells by layer: cx | cy << 3 | label << 8
  __shared__ uint32_t s_slot[64];                             // the pool slots of the window's archive bricks
  __shared__ uint32_t s_any;                                  // one of them exists

  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  // A workgroup of fewer than 256 candidates gives each of them P threads: they share its source layers (lp of L) and, from
  // P = 16 on, the listed cells of a layer (ep of EP); every thread's sums are partial sums of its candidate's.
  const uint32_t C = min((uint32_t)MT, g.ncand - blockIdx.y * MT), P = MT / C;
  const uint32_t L = min(P, 8u), EP = max(P >> 3, 1u);
  const uint32_t part = tid / C, k = blockIdx.y * MT + (tid - part * C);
  const uint32_t ep = part / L, lp = part - ep * L;
  const bool valid = ep < EP;
  int sh[3];
  candidate(g, k, sh);
  uint32_t n_oo = 0, n_of = 0, n_fo = 0, n_ff = 0, n_same = 0;
  uint32_t t_src = 0, t_occ = 0, t_free = 0;
  const int nrows = g.E[2] * g.E[1];
  const uint32_t xmask = (1u << g.xlg) - 1u, rowbits = 0xffffffffu >> (32u - (1u << g.xlg));
  const int fill_steps = ((nrows << g.xlg) + MT * FILL_U - 1) / (MT * FILL_U);
  const uint32_t first = blockIdx.x * g.run, last = min(first + g.run, g.n);
  for (uint32_t i = first; i < last; ++i) {
    int s[3];
    brick_of(src_hdr[(size_t)i * HDR_WORDS], src_hdr[(size_t)i * HDR_WORDS + 1], s[0], s[1], s[2]);
    const uint32_t w0 = src_cells[(size_t)i * 512u + tid], w1 = src_cells[(size_t)i * 512u + 256u + tid];  // (in flight beside the lookup)
    if (world_find(skeys, svals, g.smask, brick_key(s[0], s[1], s[2])) != i) continue;  // (uniform) a later source of the same brick
    // ---- the source brick: two planes and the list of its occupied cells
    const uint32_t c0 = word_class(w0, g.flags, g.max_movable), c1 = word_class(w1, g.flags, g.max_movable);
    const u64 bo0 = __ballot(c0 == 2u), bf0 = __ballot(c0 == 1u), bo1 = __ballot(c1 == 2u), bf1 = __ballot(c1 == 1u);
    if (lane == 0u) {
      s_socc[wave] = bo0, s_sfree[wave] = bf0, s_socc[wave + 4u] = bo1, s_sfree[wave + 4u] = bf1;
      t_occ += (uint32_t)(__popcll(bo0) + __popcll(bo1)), t_free += (uint32_t)(__popcll(bf0) + __popcll(bf1));
    }
    if (c0 == 2u) s_ent[wave * 64u + lane_rank(bo0, lane)] = (uint16_t)(lane | ((w0 >> 8) & 0xff00u));
    if (c1 == 2u) s_ent[(wave + 4u) * 64u + lane_rank(bo1, lane)] = (uint16_t)(lane | ((w1 >> 8) & 0xff00u));
    if (tid == 0u) s_any = 0u, ++t_src;
    __syncthreads();
    u64 any = 0ull;
#pragma unroll
    for (int l = 0; l < 8; ++l) any |= s_socc[l] | s_sfree[l];
    if (!any) {  // (uniform, like every early end below) no counted cell
      __syncthreads();
      continue;
    }
    // ---- the archive bricks under the window
    if (tid < 64u) {
      const int kb[3] = {(int)(tid & 3u), (int)((tid >> 2) & 3u), (int)(tid >> 4)};
      uint32_t slot = NONE;
      if (kb[0] < g.nbk[0] && kb[1] < g.nbk[1] && kb[2] < g.nbk[2]) {
        int b[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) b[a] = ((8 * s[a] + g.c[a] - g.r[a]) >> 3) + kb[a];
        if (brick_in_range(b[0], b[1], b[2])) slot = world_find(keys, vals, g.hmask, brick_key(b[0], b[1], b[2]));
      }
      s_slot[tid] = slot;
      if (slot != NONE) s_any = 1u;
    }
    __syncthreads();
    if (!s_any) {  // nothing archived near this brick: every pair has an unknown side
      __syncthreads();
      continue;
    }
    // ---- the window: 8, 16 or 32 lanes per row (xlg), every load of a step issued first
    for (int step = 0; step < fill_steps; ++step) {
      uint32_t w[FILL_U];
      const int x = (int)(tid & xmask);
#pragma unroll
      for (int u = 0; u < FILL_U; ++u) {
        const int row = (int)(((uint32_t)(step * FILL_U + u) * MT + tid) >> g.xlg), z = (int)(((uint32_t)row * g.inv_ey) >> 16), y = row - z * g.E[1];
        w[u] = RES_UNKNOWN_W1;
        if (row < nrows && x < g.E[0]) {
          const int ax = g.res[0] + x, ay = g.res[1] + y, az = g.res[2] + z;  // (< 32: four bricks per axis)
          const uint32_t slot = s_slot[(ax >> 3) | ((ay >> 3) << 2) | ((az >> 3) << 4)];
          if (slot != NONE) w[u] = cells[(size_t)slot * 512u + (uint32_t)((ax & 7) | ((ay & 7) << 3) | ((az & 7) << 6))];
        }
      }
#pragma unroll
      for (int u = 0; u < FILL_U; ++u) {
        const int row = (int)(((uint32_t)(step * FILL_U + u) * MT + tid) >> g.xlg), z = (int)(((uint32_t)row * g.inv_ey) >> 16), y = row - z * g.E[1];
        const uint32_t cls = word_class(w[u], g.flags, g.max_movable);  // (a lane beyond the row holds the unknown word)
        const u64 bo = __ballot(cls == 2u), bf = __ballot(cls == 1u);
        if (row < nrows) {
          if (x < g.E[0]) s_wlab[(z * WIN + y) * WIN + x] = (uint8_t)(w[u] >> 16);
          if (x == 0) {
            const uint32_t from = lane & ~xmask;  // the row's first lane
            s_wocc[z * WIN + y] = (uint32_t)(bo >> from) & rowbits, s_wfree[z * WIN + y] = (uint32_t)(bf >> from) & rowbits;
          }
        }
      }
    }
    __syncthreads();
    // ---- this thread's candidate
    if (valid) {
#pragma unroll 1
      for (int cz = (int)lp; cz < 8; cz += (int)L) {
        const u64 so = s_socc[cz], sf = s_sfree[cz];
        if (!(so | sf)) continue;
        const int at = (cz + sh[2]) * WIN + sh[1];
        if (ep == 0u) {  // the layer of the window under this shift, from the eight rows it selects
          u64 wo = 0ull, wf = 0ull;
#pragma unroll
          for (int cy = 0; cy < 8; ++cy) {
            wo |= (u64)((s_wocc[at + cy] >> sh[0]) & 0xffu) << (8 * cy);
            wf |= (u64)((s_wfree[at + cy] >> sh[0]) & 0xffu) << (8 * cy);
          }
          n_oo += (uint32_t)__popcll(so & wo), n_of += (uint32_t)__popcll(so & wf);
          n_fo += (uint32_t)__popcll(sf & wo), n_ff += (uint32_t)__popcll(sf & wf);
        }
        const int cnt = __popcll(so);
        for (int j = (int)ep; j < cnt; j += (int)EP) {
          const uint32_t e = s_ent[cz * 64 + j];
          const int wx = (int)(e & 7u) + sh[0], wy = at + (int)((e >> 3) & 7u);
          n_same += ((s_wocc[wy] >> wx) & 1u) & (uint32_t)(s_wlab[wy * WIN + wx] == (uint8_t)(e >> 8));
        }
      }
    }
    __syncthreads();
  }
  if (P > 1u) {  // (uniform) the threads of a candidate meet in LDS - the window's rows are free now: C <= 128 -, one of them flushes
    const uint32_t kc = tid - part * C;
    if (part == 0u) s_wocc[4u * kc] = s_wocc[4u * kc + 1u] = s_wocc[4u * kc + 2u] = s_wocc[4u * kc + 3u] = s_wfree[kc] = 0u;
    __syncthreads();
    if (valid) {
      if (n_oo) atomicAdd(&s_wocc[4u * kc], n_oo);
      if (n_of) atomicAdd(&s_wocc[4u * kc + 1u], n_of);
      if (n_fo) atomicAdd(&s_wocc[4u * kc + 2u], n_fo);
      if (n_ff) atomicAdd(&s_wocc[4u * kc + 3u], n_ff);
      if (n_same) atomicAdd(&s_wfree[kc], n_same);
    }
    __syncthreads();
    n_oo = s_wocc[4u * kc], n_of = s_wocc[4u * kc + 1u], n_fo = s_wocc[4u * kc + 2u], n_ff = s_wocc[4u * kc + 3u], n_same = s_wfree[kc];
  }
  if (part == 0u) {
    uint32_t *__restrict__ mine = acc + 5 * (size_t)k;
    if (n_oo) atomicAdd(mine, n_oo);
    if (n_of) atomicAdd(mine + 1, n_of);
    if (n_fo) atomicAdd(mine + 2, n_fo);
    if (n_ff) atomicAdd(mine + 3, n_ff);
    if (n_same) atomicAdd(mine + 4, n_same);
  }
  if (blockIdx.y == 0u && lane == 0u) {  // the sources' totals, once
    if (t_src) atomicAdd(totals + T_SOURCES, t_src);
    if (t_occ) atomicAdd(totals + T_OCC, t_occ);
    if (t_free) atomicAdd(totals + T_FREE, t_free);
  }
}

// is candidate (score a, squared distance da, index ka) better than (b, db, kb)?
__device__ __forceinline__ bool better(long long a, uint32_t da, uint32_t ka, long long b, uint32_t db, uint32_t kb) {
  return a != b ? a > b : da != db ? da < db : ka < kb;
}
__device__ __forceinline__ long long score_of(const MatchGeo &g, const uint32_t *__restrict__ a) {
  return (long long)g.w[0] * a[0] + (long long)g.w[1] * a[4] + (long long)g.w[2] * a[1] + (long long)g.w[3] * a[2] + (long long)g.w[4] * a[3];
}

__global__ __launch_bounds__(MT) void k_wmt_reduce(MatchGeo g, const uint32_t *__restrict__ acc, const uint32_t *__restrict__ totals,
                                                   sdm_world_match_score *__restrict__ scores, sdm_world_match_result *__restrict__ result) {
  __shared__ long long s_score[MT];
  __shared__ uint32_t s_d2[MT], s_k[MT];
  const uint32_t tid = threadIdx.x;
  long long best = 0;
  uint32_t best_d2 = 0xffffffffu, best_k = NONE;  // (NONE: no candidate yet)
  for (uint32_t k = tid; k < g.ncand; k += MT) {
    int sh[3];
    candidate(g, k, sh);
    const uint32_t *__restrict__ a = acc + 5 * (size_t)k;
    const long long sc = score_of(g, a);
    const int d[3] = {sh[0] - g.r[0], sh[1] - g.r[1], sh[2] - g.r[2]};
    const uint32_t d2 = (uint32_t)(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (scores) {
      sdm_world_match_score *__restrict__ o = scores + k;
      o->offset[0] = g.c[0] + d[0], o->offset[1] = g.c[1] + d[1], o->offset[2] = g.c[2] + d[2];
      o->n_oo = a[0], o->n_of = a[1], o->n_fo = a[2], o->n_ff = a[3], o->n_same = a[4];
    }
    if (best_k == NONE || better(sc, d2, k, best, best_d2, best_k)) best = sc, best_d2 = d2, best_k = k;
  }
  s_score[tid] = best, s_d2[tid] = best_d2, s_k[tid] = best_k;
  __syncthreads();
  for (uint32_t step = MT / 2; step >= 1u; step >>= 1) {
    if (tid < step && s_k[tid + step] != NONE &&
        (s_k[tid] == NONE || better(s_score[tid + step], s_d2[tid + step], s_k[tid + step], s_score[tid], s_d2[tid], s_k[tid])))
      s_score[tid] = s_score[tid + step], s_d2[tid] = s_d2[tid + step], s_k[tid] = s_k[tid + step];
    __syncthreads();
  }
  const uint32_t bk = s_k[0];  // (there is always the centre)
  const long long bs = s_score[0];
  int bsh[3];
  candidate(g, bk, bsh);
  __syncthreads();
  long long ru = INT64_MIN;
  for (uint32_t k = tid; k < g.ncand; k += MT) {
    int sh[3];
    candidate(g, k, sh);
    const int cheb = max(max(abs(sh[0] - bsh[0]), abs(sh[1] - bsh[1])), abs(sh[2] - bsh[2]));
    if (cheb >= 2) ru = max(ru, score_of(g, acc + 5 * (size_t)k));
  }
  s_score[tid] = ru;
  __syncthreads();
  for (uint32_t step = MT / 2; step >= 1u; step >>= 1) {
    if (tid < step) s_score[tid] = max(s_score[tid], s_score[tid + step]);
    __syncthreads();
  }
  if (tid != 0u) return;
  result->n_candidates = g.ncand, result->n_sources = totals[T_SOURCES];
  result->src_occupied = totals[T_OCC], result->src_free = totals[T_FREE];
  result->best_score = bs, result->runner_up = s_score[0];
  result->best = (int32_t)bk;
#pragma unroll
  for (int a = 0; a < 3; ++a) result->best_offset[a] = g.c[a] + bsh[a] - g.r[a];
  result->pad[0] = result->pad[1] = 0u;
}

// the work arrays inside WorldMatchPool::work, in words: the 64-bit keys first
struct MatchLayout {
  size_t skeys, svals, acc, totals, total;
  MatchLayout(size_t slots, size_t ncand) {
    skeys = 0, svals = 2 * slots, acc = 3 * slots, totals = acc + 5 * ncand, total = totals + T_WORDS;
  }
};

hipError_t launch_world_match(const MatchGeo &g, const MatchLayout &at, const sdm_map *m, uint32_t *work, const uint32_t *src_hdr,
                              const uint32_t *src_cells, sdm_world_match_score *scores, sdm_world_match_result *result, hipStream_t s) {
  const WorldLayer &L = m->world;
  u64 *skeys = reinterpret_cast<u64 *>(work + at.skeys);
  uint32_t *svals = work + at.svals, *acc = work + at.acc, *totals = work + at.totals;
  hipError_t e;
  if ((e = hipMemsetAsync(acc, 0, (at.total - at.acc) * sizeof(uint32_t), s)) != hipSuccess) return e;  // the counts and the totals
  if (g.n) {
    if ((e = hipMemsetAsync(work, 0xff, at.acc * sizeof(uint32_t), s)) != hipSuccess) return e;  // keys and the indices beside them
    if ((e = launch_world_sources(src_hdr, g.n, g.smask, skeys, svals, s)) != hipSuccess) return e;
    const dim3 grid((g.n + g.run - 1) / g.run, (g.ncand + MT - 1) / MT);
    LAYER_LAUNCH(k_wmt_score, grid, MT, s, g, src_hdr, src_cells, skeys, svals, L.keys, L.vals, L.cells, acc, totals);
  }
  LAYER_LAUNCH(k_wmt_reduce, 1, MT, s, g, acc, totals, scores, result);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

extern "C" {

sdm_status sdm_world_match(sdm_map *m, const sdm_world_match_options *o, const sdm_world_brick *bricks, const uint32_t *cells, int64_t n,
                           sdm_world_match_score *scores, sdm_world_match_result *result) {
  const char *what = "sdm_world_match";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o || !result) return LAYER_REFUSE(what, "no options or no result");
  if (o->flags & ~MATCH_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->pad[0] || o->pad[1]) return LAYER_REFUSE(what, "pad not 0");
  if (n < 0 || n > MAX_SOURCES) return LAYER_REFUSE(what, "n negative or above 2^21");
  if (n > 0 && (!bricks || !cells)) return LAYER_REFUSE(what, "no bricks or no cells");
  for (int a = 0; a < 3; ++a) {
    if (o->radius[a] < 0 || o->radius[a] > SDM_WORLD_MATCH_MAX_RADIUS) return LAYER_REFUSE(what, "a radius outside 0 .. 8");
    if (o->cell_offset[a] > MAX_OFFSET || o->cell_offset[a] < -MAX_OFFSET) return LAYER_REFUSE(what, "a cell_offset beyond +-2^19");
  }
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  const WorldLayer &L = m->world;
  WorldMatchPool &P = m->wmatch;
  const bool on_device = (o->flags & SDM_WORLD_MATCH_ON_DEVICE) != 0;
  MatchGeo g;
  g.ncand = 1;
  for (int a = 0; a < 3; ++a) {
    g.c[a] = o->cell_offset[a], g.r[a] = o->radius[a];
    g.nd[a] = 2 * g.r[a] + 1, g.E[a] = 8 + 2 * g.r[a];
    g.res[a] = (g.c[a] - g.r[a]) & 7;
    g.nbk[a] = ((g.res[a] + g.E[a] - 1) >> 3) + 1;
    g.ncand *= (uint32_t)g.nd[a];
  }
  g.xlg = g.E[0] <= 8 ? 3u : g.E[0] <= 16 ? 4u : 5u;
  g.inv_ey = (65536u + (uint32_t)g.E[1] - 1u) / (uint32_t)g.E[1];
  g.w[0] = o->w_oo, g.w[1] = o->w_same, g.w[2] = o->w_of, g.w[3] = o->w_fo, g.w[4] = o->w_ff;
  g.n = (uint32_t)n;
  g.run = std::max<uint32_t>(1u, (g.n + MAX_RUNS - 1) / MAX_RUNS);
  const uint32_t slots = table_slots((size_t)n);
  g.smask = slots - 1;
  g.hmask = L.hmask;
  g.flags = o->flags & ALL_FLAGS;
  g.max_movable = m->d.max_movable;
  const MatchLayout at(slots, g.ncand);
  if (at.total > P.words) SDM_TRY(regrow(m, &P.work, &P.words, at.total, P.work ? m->stream : nullptr));
  if (on_device) {
    HIP_TRY(launch_world_match(g, at, m, P.work, reinterpret_cast<const uint32_t *>(bricks), cells, scores, result, m->stream));
    return SDM_OK;
  }
  DevTemps tmp;
  uint32_t *d_hdr = nullptr, *d_cells = nullptr;
  sdm_world_match_score *d_scores = nullptr;
  sdm_world_match_result *d_result = nullptr;
  HIP_TRY(tmp.alloc(&d_result, 1));
  if (scores) HIP_TRY(tmp.alloc(&d_scores, g.ncand));
  if (n) {
    HIP_TRY(tmp.alloc(&d_hdr, (size_t)n * HDR_WORDS));
    HIP_TRY(tmp.alloc(&d_cells, (size_t)n * 512));
    HIP_TRY(hipMemcpyAsync(d_hdr, bricks, (size_t)n * sizeof(sdm_world_brick), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(d_cells, cells, (size_t)n * 512 * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
  }
  HIP_TRY(launch_world_match(g, at, m, P.work, d_hdr, d_cells, d_scores, d_result, m->stream));
  if (scores) HIP_TRY(hipMemcpyAsync(scores, d_scores, (size_t)g.ncand * sizeof(sdm_world_match_score), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipMemcpyAsync(result, d_result, sizeof(sdm_world_match_result), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // the sources' copies, the results and the work arrays go before the call returns
  release(m, &P.work);
  P.words = 0;
  return SDM_OK;
}

}  // extern "C"
