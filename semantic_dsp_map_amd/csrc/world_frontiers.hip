// world_frontiers.hip — world frontiers: the frontiers of frontiers.hip over the bricks of the world archive instead of
// the map block - the free cells of the archive that border never-observed space, their connected clusters across brick
// borders and a table of them, in world cells (gfx950; include/sdm.h, "world frontiers").
//
// A tile is a brick of 8 x 8 x 8 cells, a layer of it one 64-bit word (bit cx + 8 cy), "the neighbour tile" the brick the
// archive's own hash table names.  The build is a snapshot: what it leaves are lists (cells, unknown faces, cluster
// indices, the table, the counters), no pool slot.  Everything it accumulates is an integer sum, minimum or maximum, and a
// component's root is its smallest rank whatever order the unions arrive in: two builds give the same bytes.
//   snapshot_bricks  world_snapshot.hip's: the bricks of the box flagged and ranked, the number of bricks of the field.
//   k_wf_index       a thread per archived brick: its place in brick order goes to where its pool slot says (the
//               key-to-brick map of the build: the archive's hash table gives the slot), a brick of the field writes its
//               coordinates and its place at its rank.
//   k_wf_classify    a wave per archived brick, a lane per (cx, cy), the eight layers' loads first: ballots write the
//               `free` (occ == 0) and the `unknown` (occ == -1) mask, 8 x 64 bits each.  Every archived brick, not only
//               the field's: a box reads its neighbours' words like any other.
//   k_wf_neighbours  a thread per (brick of the field, one of 27): one lookup; the neighbour's rank in the field or NONE,
//               and for the six face neighbours the place in brick order (NONE: absent).  brick_in_range before every
//               lookup.
//   k_wf_mask        a thread per (brick, layer): free & (unknown at x-1 | x+1 | y-1 | y+1 | z-1 | z+1) by shifts inside
//               the word - x by one bit, the wrapping column masked out and the neighbour brick's column shifted in, y
//               by eight bits with the neighbour brick's row, z the word above or below or the neighbour brick's.  An
//               absent brick reads all ones, or all zeros with INSIDE_BRICKS.  Writes the frontier word and its
//               popcount, adds the unknown faces and those towards absent bricks; exclusive_scan_u32 over the popcounts
//               gives every word's first cell index and, behind the last word, the number of cells.
//   k_wf_compact     a wave per word, a lane per cell: world cell and unknown_faces at prefix + popcount of the lower bits.
//   k_wf_label_local a wave per brick, a lane per (cx, cy), eight labels in registers: every frontier cell starts as its
//               own cell word and takes the smallest label of its 26 (6) neighbours inside the brick - the z neighbours
//               from the lane's own registers, x and y by lane shuffles, for 26 as a separable 3 x 3 x 3 minimum - until
//               a sweep changes nothing (at most 512 sweeps).  parent[] of a cell becomes the global index of its local
//               component's smallest cell: one root per local component, no LDS, no global atomic.
//   k_wf_seams       a wave per word, a lane per cell: a frontier cell on the brick's shell looks at its 26 (6) neighbours
//               that lie in a field brick of lower rank and unites with those that are frontier cells: sdm_world.h's
//               seam_unions over its min-linking union-find (frontiers.hip's scheme; world_objects.hip runs the same body
//               with a key comparison).  Every read of parent[] in this launch is an agent-scope atomic load or an
//               atomic's return value (the L2s of the XCDs are not coherent for plain loads).  Lock-free: no thread
//               waits for another; a failed link hands the loop a strictly smaller root.
//   k_wf_accumulate  a thread per cell: follows parent[] to the root (plain loads: a later launch), writes root[] and adds
//               the cell to the root's accumulator - count, faces, signed sums, the box as maxima of order-preserving
//               codes - after a reduction across the lanes of the wave that share a root.
//   k_wf_flags + exclusive_scan_u32   1 per root with n_cells >= min_cells, scanned over n + 1 entries; counts the roots.
//   k_wf_table       a thread per cell: its cluster index (over parent[]); a root writes its table entry and stores zeros
//               back into its accumulator, so the next build starts from empty accumulators.
// The build waits twice: for the number of bricks of the field, then for the number of cells, and sizes its buffers from
// them.  This unit shares no code with frontiers.hip (DESIGN.md 5n says why); it includes none of a frame unit.  With
// world_objects.hip it shares, through sdm_world.h, the union-find, the seam body and the two ends of the local labelling;
// with every world layer the offset tables, the brick loads and the lateral shifts of a layer word (5w).
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_frontiers_options) == 40 && sizeof(sdm_world_frontier_cluster) == 120 && sizeof(sdm_world_frontiers_info) == 48,
              "sdm.h layout");
static_assert(offsetof(sdm_world_frontiers_options, max_cells) == 8 && offsetof(sdm_world_frontiers_options, bmin) == 16 &&
                  offsetof(sdm_world_frontier_cluster, first_cell) == 16 && offsetof(sdm_world_frontier_cluster, cell_sum) == 56 &&
                  offsetof(sdm_world_frontier_cluster, box_min) == 80 && offsetof(sdm_world_frontier_cluster, pad2) == 116 &&
                  offsetof(sdm_world_frontiers_info, n_cells) == 16 && offsetof(sdm_world_frontiers_info, min_cells) == 40,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;             // the kernels of a thread or a wave per item
constexpr uint32_t WF_GRID = 4096;  // the largest grid of the kernels over cells: they stride
constexpr uint32_t ALL_WF_FLAGS = SDM_WORLD_FRONTIERS_FACE_CONNECTED | SDM_WORLD_FRONTIERS_BOX | SDM_WORLD_FRONTIERS_INSIDE_BRICKS;
// the build's counters, 64 bits each: unknown faces, those towards absent bricks, roots, clusters listed
enum { F_FACES = 0, F_ABSENT, F_ROOTS, F_LISTED, F_WORDS };

struct WfAcc {  // per root; all zero = no cell yet.  nmin / max: the largest ~code / code, code = coordinate ^ 2^31
  u64 sum[3];
  uint32_t n, faces, nmin[3], max[3];
};
static_assert(sizeof(WfAcc) == 56, "bytes per cell in sdm.h");
constexpr size_t CELL_BYTES = sizeof(WfAcc) + sizeof(sdm_world_frontier_cluster) + 12 + 3 * 4 + 1;  // xyz; parent, root, idx; faces
constexpr size_t BRICK_BYTES = 8 + 4 + 27 * 4 + 6 * 4 + 8 * 8 + 8 * 4;                                // coord, place, nbr, face places, front, pre
constexpr size_t ARCH_BYTES = 4 + 4 + 2 * 8 * 8;                                                     // flag, rank, free and unknown words
static_assert(CELL_BYTES == SDM_WORLD_FRONTIERS_BYTES_PER_CELL && BRICK_BYTES == SDM_WORLD_FRONTIERS_BYTES_PER_BRICK &&
                  ARCH_BYTES == SDM_WORLD_FRONTIERS_BYTES_PER_ARCHIVED_BRICK,
              "sdm.h states the bytes");

// ---- the index ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wf_index(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr,
                                                 const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n_arch,
                                                 uint32_t max_bricks, uint32_t *__restrict__ place_of_slot, uint32_t *__restrict__ coord,
                                                 uint32_t *__restrict__ place) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j >= n_arch) return;
  const uint32_t slot = order[j];
  if (slot >= max_bricks) return;  // (never: the pool has max_bricks slots)
  place_of_slot[slot] = j;
  if (!flag[j]) return;
  const uint32_t r = rank[j];
  coord[2 * (size_t)r] = hdr[(size_t)slot * HDR_WORDS];
  coord[2 * (size_t)r + 1] = hdr[(size_t)slot * HDR_WORDS + 1] & 0xffffu;
  place[r] = j;
}

__global__ __launch_bounds__(QT) void k_wf_classify(const uint32_t *__restrict__ order, const uint32_t *__restrict__ cells, uint32_t n_arch,
                                                    u64 *__restrict__ free_m, u64 *__restrict__ unk_m) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t j = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (j >= n_arch) return;  // (wave-uniform)
  uint32_t w[8];
  load_brick(cells, order[j], lane, w);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int occ = occ_of(w[l]);
    const u64 fm = __ballot(occ == 0), um = __ballot(occ == -1);
    if (lane == 0) {
      free_m[(size_t)j * 8u + l] = fm;
      unk_m[(size_t)j * 8u + l] = um;
    }
  }
}

__global__ __launch_bounds__(QT) void k_wf_neighbours(const uint32_t *__restrict__ coord, const u64 *__restrict__ keys,
                                                      const uint32_t *__restrict__ vals, uint32_t hmask,
                                                      const uint32_t *__restrict__ place_of_slot, uint32_t max_bricks,
                                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n_arch,
                                                      uint32_t n, uint32_t *__restrict__ nbr, uint32_t *__restrict__ face_place) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n * 27u) return;
  const uint32_t r = i / 27u, k = i - r * 27u;
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
  bx += off_d((int)k, 0), by += off_d((int)k, 1), bz += off_d((int)k, 2);
  // (a coordinate of 32768 would alias another brick's key)
  const uint32_t slot = brick_in_range(bx, by, bz) ? world_find(keys, vals, hmask, brick_key(bx, by, bz)) : NONE;
  uint32_t j = slot < max_bricks ? place_of_slot[slot] : NONE;
  if (j >= n_arch) j = NONE;
  nbr[i] = j != NONE && flag[j] ? rank[j] : NONE;
  const int f = face_of((int)k);
  if (f >= 0) face_place[(size_t)r * 6u + (uint32_t)f] = j;
}

// ---- the frontier mask -----------------------------------------------------------------------------------------------
// Layer z of the brick of the field with rank r: its place in brick order, per face (x-, x+, y-, y+, z-, z+) the cells
// whose neighbour across it reads unknown, and which of the six neighbour bricks are absent (bit f).
__device__ __forceinline__ void face_masks(const uint32_t *__restrict__ place, const uint32_t *__restrict__ face_place,
                                           const u64 *__restrict__ unk_m, uint32_t r, int z, u64 absent_reads, uint32_t &j, u64 (&m)[6],
                                           uint32_t &absent) {
  j = place[r];
  uint32_t fj[6];
#pragma unroll
  for (int f = 0; f < 6; ++f) fj[f] = face_place[(size_t)r * 6u + f];
  const u64 own = unk_m[(size_t)j * 8u + z];
  u64 w[6];
#pragma unroll
  for (int f = 0; f < 4; ++f) w[f] = fj[f] != NONE ? unk_m[(size_t)fj[f] * 8u + z] : absent_reads;
  w[4] = z > 0 ? unk_m[(size_t)j * 8u + (z - 1)] : fj[4] != NONE ? unk_m[(size_t)fj[4] * 8u + 7u] : absent_reads;
  w[5] = z < 7 ? unk_m[(size_t)j * 8u + (z + 1)] : fj[5] != NONE ? unk_m[(size_t)fj[5] * 8u] : absent_reads;
  m[0] = across_lateral<0>(own, w[0]);
  m[1] = across_lateral<1>(own, w[1]);
  m[2] = across_lateral<2>(own, w[2]);
  m[3] = across_lateral<3>(own, w[3]);
  m[4] = w[4];
  m[5] = w[5];
  absent = 0u;
#pragma unroll
  for (int f = 0; f < 6; ++f) absent |= (fj[f] == NONE ? 1u : 0u) << f;
  if (z > 0) absent &= ~16u;  // (the layer below is the brick's own)
  if (z < 7) absent &= ~32u;
}

__global__ __launch_bounds__(QT) void k_wf_mask(const uint32_t *__restrict__ place, const uint32_t *__restrict__ face_place,
                                                const u64 *__restrict__ free_m, const u64 *__restrict__ unk_m, uint32_t n, u64 absent_reads,
                                                u64 *__restrict__ front, uint32_t *__restrict__ cnt, u64 *__restrict__ meta) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  uint32_t faces = 0u, towards_absent = 0u;
  if (i < n * 8u) {
    const uint32_t r = i >> 3;
    u64 m[6];
    uint32_t j, absent;
    face_masks(place, face_place, unk_m, r, (int)(i & 7u), absent_reads, j, m, absent);
    const u64 fr = free_m[(size_t)j * 8u + (i & 7u)];
    const u64 border[6] = {COL0, COL7, ROW0, ROW7, ~0ull, ~0ull};
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      faces += (uint32_t)__popcll(fr & m[f]);
      if ((absent >> f) & 1u) towards_absent += (uint32_t)__popcll(fr & m[f] & border[f]);
    }
    const u64 fw = fr & (m[0] | m[1] | m[2] | m[3] | m[4] | m[5]);
    front[i] = fw;
    cnt[i] = (uint32_t)__popcll(fw);
  } else if (i == n * 8u) {  // (the entry behind the last word: the scan leaves the number of cells there)
    front[i] = 0ull;
    cnt[i] = 0u;
  }
  faces = wave_sum(faces);  // (every lane of the wave is here)
  towards_absent = wave_sum(towards_absent);
  if ((threadIdx.x & 63u) == 0u) {
    if (faces) atomicAdd(meta + F_FACES, (u64)faces);
    if (towards_absent) atomicAdd(meta + F_ABSENT, (u64)towards_absent);
  }
}

// ---- the cell list -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wf_compact(const uint32_t *__restrict__ coord, const uint32_t *__restrict__ place,
                                                   const uint32_t *__restrict__ face_place, const u64 *__restrict__ unk_m,
                                                   const u64 *__restrict__ front, const uint32_t *__restrict__ pre, uint32_t n, u64 absent_reads,
                                                   uint32_t n_cells, int32_t *__restrict__ xyz, uint8_t *__restrict__ faces) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (i >= n * 8u) return;  // (wave-uniform, like the next test)
  const u64 fw = front[i];
  if (!fw) return;
  const uint32_t r = i >> 3;
  const int z = (int)(i & 7u);
  u64 m[6];
  uint32_t j, absent;
  face_masks(place, face_place, unk_m, r, z, absent_reads, j, m, absent);
  if (!((fw >> lane) & 1ull)) return;
  const uint32_t at = list_index(front, pre, i, lane);
  if (at >= n_cells) return;  // (never: the scan's total is n_cells)
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
  uint32_t nf = 0;
#pragma unroll
  for (int f = 0; f < 6; ++f) nf += (uint32_t)((m[f] >> lane) & 1ull);
  store_world_cell(xyz, at, bx, by, bz, lane, z);
  faces[at] = (uint8_t)nf;
}

// ---- labels, inside a brick --------------------------------------------------------------------------------------------
template <bool FACE>
__global__ __launch_bounds__(QT) void k_wf_label_local(const u64 *__restrict__ front, const uint32_t *__restrict__ pre, uint32_t n,
                                                       uint32_t n_cells, uint32_t *__restrict__ parent) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (r >= n) return;  // (wave-uniform: nothing below waits for another wave)
  u64 fw[8];
  uint32_t v[8];
  if (!local_labels(front, r, lane, fw, v)) return;
  const int cx = (int)(lane & 7u), cy = (int)(lane >> 3);
  // the lanes of the four lateral neighbours; at the brick's border the lane itself, which changes no minimum
  const int lx0 = cx > 0 ? (int)lane - 1 : (int)lane, lx1 = cx < 7 ? (int)lane + 1 : (int)lane;
  const int ly0 = cy > 0 ? (int)lane - 8 : (int)lane, ly1 = cy < 7 ? (int)lane + 8 : (int)lane;
  for (int sweep = 0; sweep < 512; ++sweep) {  // a label falls by at least one cell of its component a sweep
    uint32_t nv[8];
    bool changed = false;
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      uint32_t a = v[z];
      if (z > 0) a = min(a, v[z - 1]);
      if (z < 7) a = min(a, v[z + 1]);
      if (FACE) {
        a = min(a, min((uint32_t)__shfl((int)v[z], lx0, 64), (uint32_t)__shfl((int)v[z], lx1, 64)));
        a = min(a, min((uint32_t)__shfl((int)v[z], ly0, 64), (uint32_t)__shfl((int)v[z], ly1, 64)));
      } else {  // the smallest of 3 x 3 x 3: along z, then x, then y
        a = min(a, min((uint32_t)__shfl((int)a, lx0, 64), (uint32_t)__shfl((int)a, lx1, 64)));
        a = min(a, min((uint32_t)__shfl((int)a, ly0, 64), (uint32_t)__shfl((int)a, ly1, 64)));
      }
      nv[z] = v[z] == NO_LABEL ? NO_LABEL : a;  // (a cell that is no frontier cell carries nothing)
      changed = changed || nv[z] != v[z];
    }
#pragma unroll
    for (int z = 0; z < 8; ++z) v[z] = nv[z];
    if (!__ballot(changed)) break;
  }
  store_local_roots(v, fw, front, pre, r, lane, n_cells, parent);
}

// ---- labels, across the seams -------------------------------------------------------------------------------------------
template <bool FACE>
__global__ __launch_bounds__(QT) void k_wf_seams(const uint32_t *__restrict__ nbr, const u64 *__restrict__ front, const uint32_t *__restrict__ pre,
                                                 uint32_t n, uint32_t n_cells, uint32_t *__restrict__ parent) {
  const uint32_t i = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  seam_unions<FACE>(nbr, front, pre, i >> 3, (int)(i & 7u), threadIdx.x & 63u, n, n_cells, parent, [](uint32_t) { return 0u; });  // (one key: every frontier cell joins every other)
}

// ---- accumulators ------------------------------------------------------------------------------------------------------
constexpr int FA_VALUES = 11;  // sums: x y z (signed), n, faces; maxima: ~code x y z, code x y z
constexpr int FA_SUMS = 5;
constexpr int FA_FEW = 4;      // up to this many lanes of a wave send a root's cells themselves

__device__ __forceinline__ void send_root(WfAcc *__restrict__ a, const uint32_t (&v)[FA_VALUES]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (v[i]) atomicAdd(&a->sum[i], (u64)(long long)(int)v[i]);  // (two's complement: the sum is signed)
  atomicAdd(&a->n, v[3]);
  atomicAdd(&a->faces, v[4]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    atomicMax(&a->nmin[i], v[5 + i]);
    atomicMax(&a->max[i], v[8 + i]);
  }
}

__global__ __launch_bounds__(QT) void k_wf_accumulate(const uint32_t *__restrict__ parent, const int32_t *__restrict__ xyz,
                                                      const uint8_t *__restrict__ faces, uint32_t n_cells, uint32_t *__restrict__ root,
                                                      WfAcc *__restrict__ acc) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rounds = (n_cells + gridDim.x * QT - 1) / (gridDim.x * QT);
  for (uint32_t t = 0; t < rounds; ++t) {  // (whole waves: the ballots below see every lane)
    const uint32_t c = (t * gridDim.x + blockIdx.x) * QT + threadIdx.x;
    bool alive = c < n_cells;
    uint32_t rt = 0u, own[FA_VALUES] = {};
    if (alive) {
      uint32_t a = c, p;
      while ((p = parent[a]) < a) a = p;  // (the labelling launches are over: plain loads; strictly downwards)
      rt = a;
      root[c] = rt;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const uint32_t w = (uint32_t)xyz[3 * (size_t)c + i], code = w ^ 0x80000000u;
        own[i] = w, own[5 + i] = ~code, own[8 + i] = code;
      }
      own[3] = 1u, own[4] = faces[c];
    }
    // per distinct root of the wave one reduction across its lanes and one set of atomics
    for (int turn = 0; turn < 64; ++turn) {
      const u64 todo = __ballot(alive);
      if (!todo) break;
      const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)rt, __builtin_ctzll(todo));
      const bool mine = alive && rt == first;
      alive = alive && !mine;
      if (__popcll(__ballot(mine)) <= FA_FEW) {  // (wave-uniform)
        if (mine) send_root(acc + first, own);
        continue;
      }
      uint32_t v[FA_VALUES];
#pragma unroll
      for (int i = 0; i < FA_VALUES; ++i) v[i] = mine ? own[i] : 0u;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
        for (int i = 0; i < FA_SUMS; ++i) v[i] += (uint32_t)__shfl_xor((int)v[i], o, 64);  // (64 coordinates below 2^19: no overflow)
#pragma unroll
        for (int i = FA_SUMS; i < FA_VALUES; ++i) v[i] = max(v[i], (uint32_t)__shfl_xor((int)v[i], o, 64));
      }
      if (lane == 0) send_root(acc + first, v);
    }
  }
}

// ---- the table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wf_flags(const uint32_t *__restrict__ root, const WfAcc *__restrict__ acc, uint32_t n_cells,
                                                 uint32_t min_cells, uint32_t *__restrict__ idx, u64 *__restrict__ meta) {
  const uint32_t rounds = (n_cells + gridDim.x * QT) / (gridDim.x * QT);  // (n_cells + 1 entries: the scan's total lands in the last)
  for (uint32_t t = 0; t < rounds; ++t) {
    const uint32_t c = (t * gridDim.x + blockIdx.x) * QT + threadIdx.x;
    const bool is_root = c < n_cells && root[c] == c;
    if (c <= n_cells) idx[c] = is_root && acc[c].n >= min_cells ? 1u : 0u;
    const u64 roots = __ballot(is_root);
    if ((threadIdx.x & 63u) == 0u && roots) atomicAdd(meta + F_ROOTS, (u64)__popcll(roots));
  }
}

__global__ __launch_bounds__(QT) void k_wf_table(const uint32_t *__restrict__ root, const uint32_t *__restrict__ idx, const int32_t *__restrict__ xyz,
                                                 uint32_t n_cells, float voxel_size, uint32_t *__restrict__ cluster, WfAcc *__restrict__ acc,
                                                 sdm_world_frontier_cluster *__restrict__ table, u64 *__restrict__ meta) {
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[F_LISTED] = idx[n_cells];
  for (uint32_t c = blockIdx.x * QT + threadIdx.x; c < n_cells; c += gridDim.x * QT) {
    const uint32_t rt = root[c];
    const uint32_t j = idx[rt];
    const bool listed = idx[rt + 1u] != j;  // the root's flag
    cluster[c] = listed ? j : NONE;
    if (rt != c) continue;
    const WfAcc a = acc[c];
    acc[c] = WfAcc{};
    if (!listed) continue;
    sdm_world_frontier_cluster e;
    e.first_index = c;
    e.n_cells = a.n;
    e.n_unknown_faces = a.faces;
    e.pad0 = 0u;
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
    e.pad1 = 0u;
    e.pad2 = 0u;
    table[j] = e;
  }
}

// the buffers for n_arch archived bricks and `slots` pool slots / for `bricks` bricks of the field / for `cells` cells (the
// stream is idle if there were buffers before)
sdm_status grow_arch(sdm_map *m, size_t n_arch, size_t slots) {
  WorldFrontiersLayer &L = m->wfront;
  const size_t cap = round_up(n_arch + 1, 256);
  SDM_TRY(grow_buffers(m, n_arch + 1, cap, &L.cap_arch, {buf(&L.flag, cap), buf(&L.rank, cap), buf(&L.free_m, cap * 8), buf(&L.unk_m, cap * 8)}));
  return grow_buffers(m, slots, slots, &L.cap_slots, {buf(&L.place_of_slot, slots)});
}

sdm_status grow_bricks(sdm_map *m, size_t bricks) {
  WorldFrontiersLayer &L = m->wfront;
  const size_t cap = round_up(bricks, 256);
  return grow_buffers(m, bricks, cap, &L.cap_bricks,
                      {buf(&L.coord, cap * 2), buf(&L.place, cap), buf(&L.nbr, cap * 27), buf(&L.face_place, cap * 6), buf(&L.front, cap * 8 + 1),
                       buf(&L.pre, cap * 8 + 1)});
}

sdm_status grow_cells(sdm_map *m, size_t cells) {
  WorldFrontiersLayer &L = m->wfront;
  const size_t cap = round_up(cells, 4096);
  return grow_buffers(m, cells, cap, &L.cap_cells,
                      {buf(&L.acc, cap * sizeof(WfAcc)), buf(&L.table, cap), buf(&L.xyz, cap * 3), buf(&L.parent, cap), buf(&L.root, cap),
                       buf(&L.idx, cap + 1), buf(&L.faces, cap)},
                      [&]() -> sdm_status {
                        HIP_TRY(hipMemsetAsync(L.acc, 0, cap * sizeof(WfAcc), m->stream));  // empty; every build leaves them empty again
                        return SDM_OK;
                      });
}

// up to the frontier words and their counts
hipError_t launch_wf_words(const sdm_map *m, const uint32_t *order, uint32_t n_arch, uint32_t n, u64 absent_reads) {
  const WorldFrontiersLayer &L = m->wfront;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  if (!n) return hipSuccess;
  hipError_t e;
  if ((e = hipMemsetAsync(L.place_of_slot, 0xff, (size_t)W.max_bricks * sizeof(uint32_t), s)) != hipSuccess) return e;
  LAYER_LAUNCH(k_wf_index, (n_arch + QT - 1) / QT, QT, s, order, W.hdr, L.flag, L.rank, n_arch, W.max_bricks, L.place_of_slot, L.coord, L.place);
  LAYER_LAUNCH(k_wf_classify, (n_arch + QT / 64 - 1) / (QT / 64), QT, s, order, W.cells, n_arch, L.free_m, L.unk_m);
  LAYER_LAUNCH(k_wf_neighbours, (n * 27u + QT - 1) / QT, QT, s, L.coord, W.keys, W.vals, W.hmask, L.place_of_slot, W.max_bricks, L.flag, L.rank, n_arch,
               n, L.nbr, L.face_place);
  LAYER_LAUNCH(k_wf_mask, (n * 8u) / QT + 1, QT, s, L.place, L.face_place, L.free_m, L.unk_m, n, absent_reads, L.front, L.pre, L.meta);
  return hipSuccess;
}

// from the cell list to the table
hipError_t launch_wf_cells(const sdm_map *m, uint32_t n, uint32_t n_cells, u64 absent_reads, bool face, uint32_t min_cells, uint32_t *scan) {
  const WorldFrontiersLayer &L = m->wfront;
  hipStream_t s = m->stream;
  const uint32_t by_word = (n * 8u + QT / 64 - 1) / (QT / 64), by_brick = (n + QT / 64 - 1) / (QT / 64);
  const uint32_t by_cell = std::min<uint32_t>(n_cells / QT + 1, WF_GRID);
  hipError_t e;
  LAYER_LAUNCH(k_wf_compact, by_word, QT, s, L.coord, L.place, L.face_place, L.unk_m, L.front, L.pre, n, absent_reads, n_cells, L.xyz, L.faces);
  if (face) {
    LAYER_LAUNCH(k_wf_label_local<true>, by_brick, QT, s, L.front, L.pre, n, n_cells, L.parent);
    LAYER_LAUNCH(k_wf_seams<true>, by_word, QT, s, L.nbr, L.front, L.pre, n, n_cells, L.parent);
  } else {
    LAYER_LAUNCH(k_wf_label_local<false>, by_brick, QT, s, L.front, L.pre, n, n_cells, L.parent);
    LAYER_LAUNCH(k_wf_seams<false>, by_word, QT, s, L.nbr, L.front, L.pre, n, n_cells, L.parent);
  }
  LAYER_LAUNCH(k_wf_accumulate, by_cell, QT, s, L.parent, L.xyz, L.faces, n_cells, L.root, reinterpret_cast<WfAcc *>(L.acc));
  LAYER_LAUNCH(k_wf_flags, by_cell, QT, s, L.root, reinterpret_cast<const WfAcc *>(L.acc), n_cells, min_cells, L.idx, L.meta);
  exclusive_scan_u32(L.idx, L.idx, (size_t)n_cells + 1, scan, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wf_table, by_cell, QT, s, L.root, L.idx, L.xyz, n_cells, m->d.voxel_size, L.parent, reinterpret_cast<WfAcc *>(L.acc), L.table, L.meta);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_FRONTIERS = {"the world frontiers", "world frontiers", "sdm_world_frontiers_update", true};

void fill_info(const WorldFrontiersLayer &L, sdm_world_frontiers_info *info) {
  const u64 *h = L.h_meta;  // (the build waited for them)
  info->n_bricks = L.n;
  info->n_clusters = (uint32_t)h[F_LISTED];
  info->n_clusters_total = (uint32_t)h[F_ROOTS];
  info->flags = L.flags;
  info->n_cells = L.n_cells;
  info->n_unknown_faces = (int64_t)h[F_FACES];
  info->n_absent_faces = (int64_t)h[F_ABSENT];
  info->min_cells = L.min_cells;
  info->stamp = L.stamp;
}

sdm_status refuse_over(const WorldFrontiersLayer &L, const char *what) {
  char msg[200];
  std::snprintf(msg, sizeof(msg), "%lld world frontier cells, max_cells is %lld: call sdm_world_frontiers_update with a larger max_cells (or 0)",
                (long long)L.n_cells, (long long)L.max_cells);
  set_error(what, __FILE__, __LINE__, msg);
  return SDM_ERR_CAPACITY;
}
}  // namespace

extern "C" {

sdm_status sdm_world_frontiers_update(sdm_map *m, const sdm_world_frontiers_options *o) {
  const char *what = "sdm_world_frontiers_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WF_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if (o->max_cells < 0) return LAYER_REFUSE(what, "max_cells < 0");
  BrickBox box{};
  if (o->flags & SDM_WORLD_FRONTIERS_BOX) {  // (bmax < bmin: an empty box, a field of no bricks)
    box.use = 1u;
    for (int a = 0; a < 3; ++a) box.lo[a] = o->bmin[a], box.hi[a] = o->bmax[a];
  }
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldFrontiersLayer &L = m->wfront;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, F_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, F_WORDS + 1, true));
  HIP_TRY(hipMemsetAsync(L.meta, 0, F_WORDS * sizeof(u64), s));
  // the bricks of the field: the archive's in brick order, those of the box ranked
  SnapshotBricks b;
  SDM_TRY(snapshot_bricks(m, box, (size_t)m->world.max_bricks * 8 + 1, L.h_meta + F_WORDS, [&](uint32_t n_arch, uint32_t **flag, uint32_t **rank) -> sdm_status {
    SDM_TRY(grow_arch(m, n_arch, m->world.max_bricks));
    *flag = L.flag, *rank = L.rank;
    return SDM_OK;
  }, &b));
  const uint32_t n = b.n;
  uint32_t *scan = b.scan;
  // the frontier words, and how many cells they hold
  const u64 absent_reads = (o->flags & SDM_WORLD_FRONTIERS_INSIDE_BRICKS) ? 0ull : ~0ull;
  uint32_t n_cells = 0;
  if (n) {
    SDM_TRY(grow_bricks(m, n));
    HIP_TRY(launch_wf_words(m, b.order, b.n_arch, n, absent_reads));
    exclusive_scan_u32(L.pre, L.pre, (size_t)n * 8 + 1, scan, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L.h_meta + F_WORDS, L.pre + (size_t)n * 8, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, F_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (n) n_cells = (uint32_t)L.h_meta[F_WORDS] & 0xffffffffu;
  L.n = n;
  L.n_cells = (int64_t)n_cells;
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
    HIP_TRY(launch_wf_cells(m, n, n_cells, absent_reads, (o->flags & SDM_WORLD_FRONTIERS_FACE_CONNECTED) != 0,
                            (uint32_t)std::max<int32_t>(o->min_cells, 1), scan));
    HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, F_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  L.built(m->world.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_frontier_clusters(sdm_map *m, sdm_world_frontier_cluster *out, int32_t cap, int32_t *n_out,
                                           sdm_world_frontiers_info *info) {
  const char *what = "sdm_get_world_frontier_clusters";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out || (cap > 0 && !out)) return LAYER_REFUSE(what, "cap < 0, no n_out, or no out for cap > 0");
  SDM_TRY(layer_check(m, what, &m->wfront, WORLD_FRONTIERS));
  const WorldFrontiersLayer &L = m->wfront;
  if (info) fill_info(L, info);
  if (L.over) return refuse_over(L, what);
  const uint32_t n = (uint32_t)L.h_meta[F_LISTED];
  const size_t take = std::min<size_t>(n, (size_t)cap);
  if (take) {
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(out, L.table, take * sizeof(sdm_world_frontier_cluster), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  *n_out = (int32_t)n;
  return SDM_OK;
}

sdm_status sdm_get_world_frontier_cells(sdm_map *m, int32_t *cell_xyz, uint32_t *cluster, uint8_t *unknown_faces, int64_t first, int64_t cap,
                                        int64_t *n_out) {
  const char *what = "sdm_get_world_frontier_cells";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wfront, WORLD_FRONTIERS));
  const WorldFrontiersLayer &L = m->wfront;
  *n_out = L.n_cells;
  if (L.over) return refuse_over(L, what);
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>(L.n_cells - first, cap), 0);
  if (take && (cell_xyz || cluster || unknown_faces)) {
    HIP_TRY(hipSetDevice(m->device));
    if (cell_xyz) HIP_TRY(hipMemcpyAsync(cell_xyz, L.xyz + 3 * (size_t)first, take * 12, hipMemcpyDeviceToHost, m->stream));
    if (cluster) HIP_TRY(hipMemcpyAsync(cluster, L.parent + (size_t)first, take * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    if (unknown_faces) HIP_TRY(hipMemcpyAsync(unknown_faces, L.faces + (size_t)first, take, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return SDM_OK;
}

}  // extern "C"
