// frontiers.hip — the map's frontiers: the free cells that border never-observed space, their connected clusters and a
// table of them (gfx950; include/sdm.h, "frontiers").
//
// A snapshot of one frame in map-index cells, like the distance field and the instance table.  Only the first kernel reads
// State::res; everything after it works on two bitmasks of V / 8 bytes each and on the compacted list of frontier cells.
//   k_frontier_classify   a wave per chunk of 64 cells in map-index order (FC_U chunks a wave, all loads first): reads the
//               results through the ring correction and writes one word of the `free` (occ == 0) and one of the `unknown`
//               (occ == -1) mask from two ballots.
//   k_frontier_mask       a thread per 64-bit word: free & (the unknown bits of the six face neighbours).  A neighbour
//               2^s cells away is a shift by 2^s bits with the carry from the adjacent word (s < 6) or the word 2^(s-6)
//               words away; the cells that have no such neighbour inside the map - line, plane and map ends - are masked
//               out by coord_is(), so x rows of 4..32 cells that share a word never see each other's ends and the map is
//               no torus.  Writes the frontier word and its popcount; exclusive_scan_u32 turns the popcounts into the
//               rank of every word's first frontier cell.
//   k_frontier_compact    a wave per word, a lane per cell: rank = the word's prefix + the popcount of the lower bits =
//               the cell's index in the ascending cell list.  Writes cell, unknown_faces and parent[rank] = the rank of
//               the first cell of the cell's run of frontier cells along x inside the word (itself where it stands
//               alone): such a run is one tree of depth one before the labelling begins.  The scan's total is the
//               number of frontier cells n; n > capacity: the build stops here (every later kernel sees zero cells),
//               the getters report SDM_ERR_CAPACITY with the true n.
//   k_frontier_label      a thread per rank: looks up the 13 (26-connectivity) or 3 (6-connectivity) neighbours that
//               precede the cell in cell order in the frontier mask and unites with those that are set.  Union-find with
//               min-linking: a root only ever gets a smaller parent (atomicMin), so the root of a component ends up its
//               smallest rank = its smallest cell word, in whatever order the unions arrive.  Every read of parent[] in
//               this launch is an agent-scope atomic load or an atomic's return value (the L2s of the XCDs are not
//               coherent for plain loads).  Lock-free: no thread waits for another; a failed link hands the loop a
//               strictly smaller root.
//   k_frontier_accumulate a thread per rank: follows parent[] to the root (plain loads: a later launch), writes root[rank]
//               and adds the cell to the root's accumulator - count, face sum, box (minima as maxima of the complement;
//               the smallest z is the first cell's), three 64-bit sums - with integer atomics, after a reduction across
//               the lanes of the wave that share a root; a wave takes 16 chunks of 64 ranks in a row and carries the
//               totals of the last root from chunk to chunk, so a large cluster sends one set per 1024 cells.
//   k_frontier_flags + exclusive_scan_u32   1 per root with n_cells >= min_cells, scanned over n + 1 entries: idx[root] =
//               the cluster's place in the table (ascending first_cell), idx[n] = the number of clusters.
//   k_frontier_table      a thread per rank: writes the cell's cluster index (over parent[], which is done with); a root
//               writes its sdm_frontier_cluster and stores zeros back into its accumulator, so the next build starts from
//               empty accumulators.
// The number of cells is only known on the device, and sdm_frontiers_update does not wait: the kernels over cells run on a
// fixed grid and stride over the n they read from meta[].
#include "sdm_layer.h"
#include "sdm_map.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_frontier_cluster) == 96, "sdm.h layout");
static_assert(offsetof(sdm_frontier_cluster, cell_sum) == 32 && offsetof(sdm_frontier_cluster, box_min) == 56 &&
                  offsetof(sdm_frontier_cluster, pad1) == 92,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int FC_TPB = 256, FC_WAVES = FC_TPB / 64;
constexpr int FC_U = 8;            // chunks (words) a wave takes
constexpr int FR_TPB = 256;        // the kernels over ranks
constexpr uint32_t FR_GRID = 4096; // ... and their largest grid: they stride over the cells
enum { META_N = 0, META_N_USED, META_N_SCAN, META_N_CLUSTERS, META_WORDS };  // true count; 0 if over capacity; that + 1

struct FAcc {  // per root; all zero = no cell yet
  u64 sum[3];
  uint32_t n, faces, nminx, nminy, maxx, maxy, maxz, pad;
};
static_assert(sizeof(FAcc) == 56, "bytes per cell in sdm.h");

struct Front {  // everything a build touches (sdm_map::front: bits, cells, meta)
  u64 *free_m, *unk_m, *front_m;  // [nw]
  uint32_t *pre;                  // [nw]: popcounts, then their exclusive scan
  FAcc *acc;                      // [cap]
  sdm_frontier_cluster *table;    // [cap]
  uint32_t *cell, *parent, *root; // [cap]; parent ends as the per-cell cluster index
  uint32_t *idx;                  // [cap + 1]
  uint8_t *faces;                 // [cap]
  uint32_t *meta;                 // [META_WORDS]
  uint32_t nw, cap;
  int x_n, y_n, z_n;
};
constexpr size_t CELL_BYTES = sizeof(FAcc) + sizeof(sdm_frontier_cluster) + 4 * 4 + 1;  // 169
static_assert(CELL_BYTES == SDM_FRONTIERS_BYTES_PER_CELL, "sdm.h states the bytes per cell");

size_t cells_bytes(size_t cap) { return CELL_BYTES * cap + 8; }  // (+ idx[cap], and the faces rounded up)

// ---- classify ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_TPB) void k_frontier_classify(Dims d, Frame f, const uint2 *__restrict__ res, u64 *__restrict__ free_m,
                                                              u64 *__restrict__ unk_m, uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * FC_WAVES + (threadIdx.x >> 6)) * FC_U;
  uint32_t w[FC_U];
  load_w1(d, f, res, first, nw, lane, w);
#pragma unroll
  for (int u = 0; u < FC_U; ++u) {
    const uint32_t chunk = first + (uint32_t)u;
    if (chunk >= nw) break;  // (wave-uniform)
    const int occ = occ_of(w[u]);
    const u64 fm = __ballot(occ == 0), um = __ballot(occ == -1);
    if (lane == 0) {
      free_m[chunk] = fm;
      unk_m[chunk] = um;
    }
  }
}

// ---- the frontier mask ---------------------------------------------------------------------------------------------
// per face (x-, x+, y-, y+, z-, z+): the cells of word wi whose neighbour across it lies inside the map and is unknown
__device__ __forceinline__ void unknown_faces(const Front &g, uint32_t wi, u64 (&m)[6]) {
  const uint32_t c0 = wi << 6;
  const int s[3] = {0, g.x_n, g.x_n + g.y_n}, nb[3] = {g.x_n, g.y_n, g.z_n};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m[2 * a] = bits_down(g.unk_m, wi, s[a]) & ~coord_is(c0, s[a], nb[a], 0u);
    m[2 * a + 1] = bits_up(g.unk_m, wi, g.nw, s[a]) & ~coord_is(c0, s[a], nb[a], (1u << nb[a]) - 1u);
  }
}

__global__ __launch_bounds__(FR_TPB) void k_frontier_mask(Front g) {
  const uint32_t wi = blockIdx.x * FR_TPB + threadIdx.x;
  if (wi >= g.nw) return;
  u64 m[6];
  unknown_faces(g, wi, m);
  const u64 fr = g.free_m[wi] & (m[0] | m[1] | m[2] | m[3] | m[4] | m[5]);
  g.front_m[wi] = fr;
  g.pre[wi] = (uint32_t)__popcll(fr);
}

// ---- the cell list -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_TPB) void k_frontier_compact(Front g) {
  const uint32_t total = g.pre[g.nw - 1u] + (uint32_t)__popcll(g.front_m[g.nw - 1u]);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint32_t used = total <= g.cap ? total : 0u;
    g.meta[META_N] = total;
    g.meta[META_N_USED] = used;
    g.meta[META_N_SCAN] = used + 1u;
  }
  if (total > g.cap) return;  // nothing is written past the capacity, nothing is truncated
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * FC_WAVES + (threadIdx.x >> 6)) * FC_U;
  for (int u = 0; u < FC_U; ++u) {
    const uint32_t wi = first + (uint32_t)u;
    if (wi >= g.nw) break;  // (wave-uniform, like the next test)
    const u64 fr = g.front_m[wi];
    if (!fr) continue;
    u64 m[6];
    unknown_faces(g, wi, m);
    // where a run of frontier cells along x begins inside this word: after a cell that is none, at a line's first cell
    const u64 begins = fr & (~(fr << 1) | coord_is(wi << 6, 0, g.x_n, 0u));
    if ((fr >> lane) & 1ull) {
      const uint32_t base = g.pre[wi];
      const uint32_t r = base + lane_rank(fr, lane);  // < total <= cap
      const uint32_t first = 63u - (uint32_t)__builtin_clzll(begins & ((2ull << lane) - 1ull));  // of this cell's run (<= lane)
      uint32_t n = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) n += (uint32_t)((m[i] >> lane) & 1ull);
      g.cell[r] = (wi << 6) | lane;
      g.parent[r] = base + lane_rank(fr, first);  // the run is one tree already, its first cell the root
      g.faces[r] = (uint8_t)n;
    }
  }
}

// ---- labels --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t parent_of(uint32_t *parent, uint32_t a) {
  return __hip_atomic_load(parent + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t lower_parent(uint32_t *parent, uint32_t a, uint32_t v) {  // -> what it was
  return __hip_atomic_fetch_min(parent + a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a, halving the path on the way (a parent is only ever lowered to an ancestor: still the same component)
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t a) {
  for (;;) {
    const uint32_t p = parent_of(parent, a);
    if (p == a) return a;
    const uint32_t gp = parent_of(parent, p);
    if (gp == p) return p;
    lower_parent(parent, a, gp);
    a = gp;
  }
}

__device__ __forceinline__ void unite(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = lower_parent(parent, hi, lo);
    if (old == hi) return;  // hi was still a root and now hangs below lo
    a = old;                // somebody linked hi below `old` (< hi) first: old and lo remain to be united
    b = lo;
  }
}

template <bool FACE>
__global__ __launch_bounds__(FR_TPB) void k_frontier_label(Front g) {
  const uint32_t n = g.meta[META_N_USED];
  const uint32_t N[3] = {1u << g.x_n, 1u << g.y_n, 1u << g.z_n};
  const int xy_n = g.x_n + g.y_n;
  for (uint32_t r = blockIdx.x * FR_TPB + threadIdx.x; r < n; r += gridDim.x * FR_TPB) {
    const uint32_t c = g.cell[r];
    int x, y, z;
    cell_xyz(g.x_n, g.y_n, c, x, y, z);
#pragma unroll
    for (int k = 0; k < 13; ++k) {  // the neighbours before the cell in cell order: (dz, dy, dx) < (0, 0, 0)
      const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
      if (FACE && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
      if (k == 12 && (c & 63u) != 0u) continue;  // x - 1 in the same word: k_frontier_compact has linked the run
      const uint32_t nx = (uint32_t)(x + dx), ny = (uint32_t)(y + dy), nz = (uint32_t)(z + dz);
      if (nx >= N[0] || ny >= N[1] || nz >= N[2]) continue;
      const uint32_t cn = nx | (ny << g.x_n) | (nz << xy_n), wi = cn >> 6, b = cn & 63u;
      const u64 fw = g.front_m[wi];
      if (!((fw >> b) & 1ull)) continue;
      unite(g.parent, r, g.pre[wi] + lane_rank(fw, b));
    }
  }
}

// ---- accumulators --------------------------------------------------------------------------------------------------
constexpr int FA_VALUES = 10;  // sums: x y z, n, faces; maxima: ~x, ~y, x, y, z
constexpr int FA_SUMS = 5;
constexpr int FA_FEW = 4;      // up to this many lanes of a wave send a root's cells themselves
constexpr int FA_RUN = 16;     // chunks of 64 ranks a wave takes in a row

__device__ __forceinline__ void send_root(FAcc *a, const uint32_t (&v)[FA_VALUES]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (v[i]) atomicAdd(&a->sum[i], (u64)v[i]);
  atomicAdd(&a->n, v[3]);
  atomicAdd(&a->faces, v[4]);
  atomicMax(&a->nminx, v[5]);
  atomicMax(&a->nminy, v[6]);
  atomicMax(&a->maxx, v[7]);
  atomicMax(&a->maxy, v[8]);
  atomicMax(&a->maxz, v[9]);
}

__global__ __launch_bounds__(FR_TPB) void k_frontier_accumulate(Front g) {
  const uint32_t n = g.meta[META_N_USED];
  const uint32_t lane = threadIdx.x & 63u;
  // a wave takes FA_RUN consecutive chunks of 64 ranks and carries the totals of the root it reduced last (wave-uniform
  // values) from chunk to chunk: a large cluster's cells are long runs of ranks, and its accumulator sees one set of
  // atomics per change of root instead of one per chunk
  uint32_t carry_root = INVALID_INDEX, carry[FA_VALUES] = {};
  const uint32_t wave_first = (blockIdx.x * (FR_TPB / 64) + (threadIdx.x >> 6)) * (FA_RUN * 64u);
  for (uint32_t base = wave_first; base < n; base += gridDim.x * (FR_TPB / 64) * (FA_RUN * 64u)) {  // (wave-uniform)
    for (uint32_t chunk = 0; chunk < (uint32_t)FA_RUN && base + chunk * 64u < n; ++chunk) {
      const uint32_t r = base + chunk * 64u + lane;
      bool alive = r < n;
      uint32_t rt = 0u, own[FA_VALUES] = {};
      if (alive) {
        uint32_t a = r, p;
        while ((p = g.parent[a]) != a) a = p;  // (the labelling launch is over: plain loads)
        rt = a;
        g.root[r] = rt;
        const uint32_t c = g.cell[r];
        uint32_t x, y, z;
        cell_xyz(g.x_n, g.y_n, c, x, y, z);
        own[0] = x, own[1] = y, own[2] = z, own[3] = 1u, own[4] = g.faces[r];
        own[5] = ~x, own[6] = ~y, own[7] = x, own[8] = y, own[9] = z;
      }
      // per distinct root of the wave one reduction across its lanes and one set of atomics
      for (;;) {
        const u64 todo = __ballot(alive);
        if (!todo) break;
        const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)rt, __builtin_ctzll(todo));
        const bool mine = alive && rt == t;
        alive = alive && !mine;
        const u64 mm = __ballot(mine);
        if (__popcll(mm) <= FA_FEW) {  // (wave-uniform)
          if (mine) send_root(g.acc + t, own);
          continue;
        }
        uint32_t v[FA_VALUES];
#pragma unroll
        for (int i = 0; i < FA_VALUES; ++i) v[i] = mine ? own[i] : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
          for (int i = 0; i < FA_SUMS; ++i) v[i] += (uint32_t)__shfl_xor((int)v[i], o, 64);
#pragma unroll
          for (int i = FA_SUMS; i < FA_VALUES; ++i) v[i] = max(v[i], (uint32_t)__shfl_xor((int)v[i], o, 64));
        }
        if (t == carry_root) {
#pragma unroll
          for (int i = 0; i < FA_SUMS; ++i) carry[i] += v[i];
#pragma unroll
          for (int i = FA_SUMS; i < FA_VALUES; ++i) carry[i] = max(carry[i], v[i]);
        } else {
          if (carry_root != INVALID_INDEX && lane == 0) send_root(g.acc + carry_root, carry);
          carry_root = t;
#pragma unroll
          for (int i = 0; i < FA_VALUES; ++i) carry[i] = v[i];
        }
      }
    }
  }
  if (carry_root != INVALID_INDEX && lane == 0) send_root(g.acc + carry_root, carry);
}

// ---- the table -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FR_TPB) void k_frontier_flags(Front g, uint32_t min_cells) {
  const uint32_t n = g.meta[META_N_USED];
  for (uint32_t r = blockIdx.x * FR_TPB + threadIdx.x; r <= n; r += gridDim.x * FR_TPB)  // idx[n]: the scan's total lands there
    g.idx[r] = (r < n && g.root[r] == r && g.acc[r].n >= min_cells) ? 1u : 0u;
}

__global__ __launch_bounds__(FR_TPB) void k_frontier_table(Dims d, Frame f, Front g) {
  const uint32_t n = g.meta[META_N_USED];
  if (blockIdx.x == 0 && threadIdx.x == 0) g.meta[META_N_CLUSTERS] = g.idx[n];
  const int xy_n = g.x_n + g.y_n;
  for (uint32_t r = blockIdx.x * FR_TPB + threadIdx.x; r < n; r += gridDim.x * FR_TPB) {
    const uint32_t rt = g.root[r];
    const uint32_t j = g.idx[rt];
    const bool listed = g.idx[rt + 1u] != j;  // the root's flag
    g.parent[r] = listed ? j : INVALID_INDEX;
    if (rt != r) continue;
    const FAcc a = g.acc[r];
    g.acc[r] = FAcc{};
    if (!listed) continue;
    const uint32_t c = g.cell[r];
    sdm_frontier_cluster e;
    e.first_cell = c;
    e.n_cells = a.n;
    e.n_unknown_faces = a.faces;
    e.first_index = r;
    const uint32_t cmin[3] = {~a.nminx, ~a.nminy, c >> xy_n}, cmax[3] = {a.maxx, a.maxy, a.maxz};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      e.cell_min[ax] = (uint16_t)cmin[ax];
      e.cell_max[ax] = (uint16_t)cmax[ax];
      e.cell_sum[ax] = a.sum[ax];
      const float origin = f.center[ax] + d.pmin[ax];
      e.box_min[ax] = origin + (float)cmin[ax] * d.voxel_size;
      e.box_max[ax] = origin + (float)(cmax[ax] + 1u) * d.voxel_size;
      e.centroid[ax] = (float)((double)origin + ((double)a.sum[ax] / (double)a.n + 0.5) * (double)d.voxel_size);
    }
    e.pad0 = 0u;
    e.pad1 = 0u;
    g.table[j] = e;
  }
}

Front front_of(const sdm_map *m) {
  const Dims &d = m->d;
  Front g;
  g.nw = d.V >> 6;
  g.cap = (uint32_t)m->front.cap;
  g.x_n = d.x_n, g.y_n = d.y_n, g.z_n = d.z_n;
  g.free_m = reinterpret_cast<u64 *>(m->front.bits);
  g.unk_m = g.free_m + g.nw;
  g.front_m = g.unk_m + g.nw;
  g.pre = reinterpret_cast<uint32_t *>(g.front_m + g.nw);
  const size_t alloc = m->front.alloc;  // the arrays are laid out for the cells allocated, of which cap are in use
  unsigned char *p = m->front.cells;
  g.acc = reinterpret_cast<FAcc *>(p);
  p += alloc * sizeof(FAcc);
  g.table = reinterpret_cast<sdm_frontier_cluster *>(p);
  p += alloc * sizeof(sdm_frontier_cluster);
  g.cell = reinterpret_cast<uint32_t *>(p);
  g.parent = g.cell + alloc;
  g.root = g.parent + alloc;
  g.idx = g.root + alloc;
  g.faces = reinterpret_cast<uint8_t *>(g.idx + alloc + 1);
  g.meta = m->front.meta;
  return g;
}

hipError_t launch_frontiers_build(const Dims &d, const Frame &f, const State &st, const Front &g, uint32_t flags, uint32_t min_cells,
                                  uint32_t *scan_scratch, hipStream_t s) {
  const uint32_t by_word = (g.nw + FC_WAVES * FC_U - 1) / (FC_WAVES * FC_U);
  const uint32_t by_rank = std::min<uint32_t>((g.cap + FR_TPB) / FR_TPB, FR_GRID);  // (>= 1: rank n of k_frontier_flags too)
  hipError_t e;
  LAYER_LAUNCH(k_frontier_classify, by_word, FC_TPB, s, d, f, reinterpret_cast<const uint2 *>(st.res), g.free_m, g.unk_m, g.nw);
  LAYER_LAUNCH(k_frontier_mask, (g.nw + FR_TPB - 1) / FR_TPB, FR_TPB, s, g);
  exclusive_scan_u32(g.pre, g.pre, g.nw, scan_scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_frontier_compact, by_word, FC_TPB, s, g);
  if (flags & SDM_FRONTIERS_FACE_CONNECTED) {
    LAYER_LAUNCH(k_frontier_label<true>, by_rank, FR_TPB, s, g);
  } else {
    LAYER_LAUNCH(k_frontier_label<false>, by_rank, FR_TPB, s, g);
  }
  LAYER_LAUNCH(k_frontier_accumulate, by_rank, FR_TPB, s, g);
  LAYER_LAUNCH(k_frontier_flags, by_rank, FR_TPB, s, g, min_cells);
  exclusive_scan_u32(g.idx, g.idx, (size_t)g.cap + 1, scan_scratch, s, g.meta + META_N_SCAN);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_frontier_table, by_rank, FR_TPB, s, d, f, g);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
// Like the distance field and the instance table, the build reads the result array in stream order and takes the host
// Frame of the last issued frame by value; the Frame stays with the table (sdm_get_frontier_clusters' origin).
namespace {
constexpr LayerName FRONTIERS = {"the frontiers", "frontiers", "sdm_frontiers_update", true};

// waits; the build's counters (META_*)
sdm_status frontiers_meta(sdm_map *m, const char *what, uint32_t (&meta)[META_WORDS], bool *over) {
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(meta, m->front.meta, sizeof(meta), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  *over = (int64_t)meta[META_N] > m->front.cap;
  if (*over) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%u frontier cells, the cell list holds %lld: call sdm_frontiers_update with a larger max_cells",
                  meta[META_N], (long long)m->front.cap);
    set_error(what, __FILE__, __LINE__, msg);
  }
  return SDM_OK;
}
}  // namespace
extern "C" {

sdm_status sdm_frontiers_update(sdm_map *m, uint32_t flags, int32_t min_cells, int64_t max_cells) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (flags & ~SDM_FRONTIERS_FACE_CONNECTED) {
    set_error("sdm_frontiers_update", __FILE__, __LINE__, "unknown flag bits");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  if (max_cells < 0) {
    set_error("sdm_frontiers_update", __FILE__, __LINE__, "max_cells < 0");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_frontiers_update", nullptr, FRONTIERS));
  HIP_TRY(hipSetDevice(m->device));
  const Dims &d = m->d;
  const size_t nw = d.V >> 6;
  const size_t cap = max_cells == 0 ? std::max<size_t>(d.V / 16, 1) : (size_t)std::min<int64_t>(max_cells, (int64_t)d.V);
  if (!m->front.bits) SDM_TRY(alloc_tracked(m, &m->front.bits, nw * (3 * 8 + 4)));
  if (!m->front.meta) SDM_TRY(alloc_tracked(m, &m->front.meta, META_WORDS));
  uint32_t *scan = nullptr;
  SDM_TRY(layer_scan_scratch(m, (size_t)d.V + 1, &scan));
  if (cap > m->front.alloc) {  // a longer cell list: the old one goes once the builds that use it have run
    size_t bytes = 0;
    m->front.alloc = 0;  // (cells; there is no list while it is replaced)
    SDM_TRY(regrow(m, &m->front.cells, &bytes, cells_bytes(cap), m->front.cells ? m->stream : nullptr));
    m->front.alloc = cap;
    HIP_TRY(hipMemsetAsync(m->front.cells, 0, cap * sizeof(FAcc), m->stream));  // empty; every build leaves them empty again
  }
  m->front.cap = (int64_t)cap;
  const Frame f = m->f;
  HIP_TRY(launch_frontiers_build(d, f, m->st, front_of(m), flags, (uint32_t)std::max<int32_t>(min_cells, 1), scan, m->stream));
  m->front.built(f, flags);
  return SDM_OK;
}

sdm_status sdm_get_frontier_clusters(sdm_map *m, sdm_frontier_cluster *out, int32_t cap, int32_t *n_out, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out || (cap > 0 && !out)) {
    set_error("sdm_get_frontier_clusters", __FILE__, __LINE__, "cap < 0, no n_out, or no out for cap > 0");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_get_frontier_clusters", &m->front, FRONTIERS));
  uint32_t meta[META_WORDS];
  bool over = false;
  SDM_TRY(frontiers_meta(m, "sdm_get_frontier_clusters", meta, &over));
  if (over) return SDM_ERR_CAPACITY;
  const uint32_t n = meta[META_N_CLUSTERS];
  const size_t take = std::min<size_t>(n, (size_t)cap);
  if (take) {
    HIP_TRY(hipMemcpyAsync(out, front_of(m).table, take * sizeof(sdm_frontier_cluster), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  *n_out = (int32_t)n;
  layer_origin(m, m->front, origin);
  return SDM_OK;
}

sdm_status sdm_get_frontier_cells(sdm_map *m, uint32_t *cell, uint32_t *cluster, uint8_t *unknown_faces, int64_t cap, int64_t *n_out) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out) {
    set_error("sdm_get_frontier_cells", __FILE__, __LINE__, "cap < 0 or no n_out");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_get_frontier_cells", &m->front, FRONTIERS));
  uint32_t meta[META_WORDS];
  bool over = false;
  SDM_TRY(frontiers_meta(m, "sdm_get_frontier_cells", meta, &over));
  *n_out = (int64_t)meta[META_N];
  if (over) return SDM_ERR_CAPACITY;
  const size_t take = (size_t)std::min<int64_t>((int64_t)meta[META_N], cap);
  if (take && (cell || cluster || unknown_faces)) {
    const Front g = front_of(m);
    if (cell) HIP_TRY(hipMemcpyAsync(cell, g.cell, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    if (cluster) HIP_TRY(hipMemcpyAsync(cluster, g.parent, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    if (unknown_faces) HIP_TRY(hipMemcpyAsync(unknown_faces, g.faces, take, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return SDM_OK;
}

}  // extern "C"
