// world_mesh.hip — the world mesh: the surface mesh of mesh.hip over the bricks of the world archive instead of the map
// block - one unit quad per face between a solid cell and a neighbour that is not solid, and the world lattice corners
// those faces use as vertices, welded across brick seams (gfx950; include/sdm.h, "world mesh").
//
// A slice is one z layer of a brick, a 64-bit word (bit cx + 8 cy); a vertex brick is a brick that owns a corner of the
// mesh (corner >> 3 per axis: the closed 9 x 9 x 9 corner set of a brick splits over the up to eight bricks b + {0,1}^3),
// whether the archive has it or not.  The build is a snapshot: what it leaves are the field's coordinates and three lists,
// no pool slot.  Everything it accumulates is an integer sum or an OR, and the vertex bricks are sorted by key: two builds
// give the same bytes whatever order the atomics arrive in.
//   snapshot_bricks  world_snapshot.hip's: the bricks of the box flagged and ranked, the number of bricks of the field.
//   k_wm_classify    a wave per archived brick, a lane per (cx, cy), the eight slices' loads first: three ballots a slice
//               write the `solid` (the options' rule), the `unknown` (occ == -1) and the `occupied` (occ >= 1, solid or
//               not) words at the brick's pool slot.  Every archived brick, not only the field's: a box reads its
//               neighbours' words like any other.
//   k_wm_neighbours  a thread per (archived brick in brick order, one of 8): a brick of the field looks one of its six face
//               neighbours up in the archive's table (brick_in_range first) and keeps the pool slot or NONE; the seventh
//               thread writes the brick's coordinates and pool slot at its rank.
//   k_wm_faces       a thread per (brick of the field, slice): the six face words solid & ~(the neighbour's solid bits) by
//               shifts inside the word - x by one bit with the wrapping column masked out and the neighbour brick's column
//               shifted in, y by eight bits with the neighbour brick's row, z the slice above or below or the neighbour
//               brick's - and from the other two masks the kinds; an absent brick reads zeros and makes kind 2.  Stores
//               the slice's face count, leaves the wave's counts for the info in a row of its own (no atomics on shared
//               counters: DESIGN.md 5i, and 5t for what they cost here) and marks the corners: the corner (dx, dy, dz) of a cell is used when the cell has its x face on side dx, its y
//               face on side dy or its z face on side dz; per dz the 9 x 9 corner plane splits into a word, a column, a row
//               and a bit for the four owners (ox, oy), each claimed in the vertex bricks' table (atomicCAS on the 51-bit
//               key, 17 bits an axis: an owner coordinate may be 32768) and ORed into that slot's level z + dz.
//   exclusive_scan_u32   over the slices' face counts and one zero: every slice's first face and, in the last entry, the
//               number of faces.
//   k_wm_vflag + exclusive_scan_u32   a thread per table slot: 1 for a claimed slot, and per wave the corner bits of its
//               claimed slots; the scan gives every claimed slot its place in the list and counts the vertex bricks.
//   k_wm_sums        16 workgroups add the waves' rows of k_wm_faces and k_wm_vflag up into the 64-bit counters and put the
//               two scans' totals beside them.  The build waits for the counters: faces, vertex bricks, vertices.
//   k_wm_vkeys, radix_sort_pairs 27 bits, k_wm_vkeys_hi, radix_sort_pairs 24 bits   the claimed slots in brick order of their
//               keys (bz, by, bx): listed in table order with the keys' low 27 bits, sorted, the high 24 bits fetched in that
//               order, sorted again (stable) - six 9-bit digits in all.
//   (k_wm_clear, before all of them: a thread per table slot empties its key and its 512 corner bits.)
//   k_wm_vrank       a thread per (vertex brick, level): the popcount of the level's word, and the rank back into the table.
//   exclusive_scan_u32   over the levels' popcounts: the first vertex of every level of every vertex brick.
//   k_wm_owners      a thread per (brick of the field, one of 8 owners): one lookup in the vertex bricks' table; the slot
//               and the rank, or NONE for an owner no corner of the brick belongs to.
//   k_wm_emit        a thread per (brick of the field, slice), mesh.hip's mapping (DESIGN.md 5j measured a wave per word
//               ten times slower on scattered surfaces; 5t says what it is here): builds the face words again, loads the
//               slice's up to eight (corner word, prefix) pairs - four owners, levels z and z + 1 - before it uses any, and
//               walks the cells that have a face in ascending order: the cell's archived word, the ids of its eight corners
//               (prefix + popcount of the lower bits, the owner picked by selects, not by an index), a 12-byte record and
//               four vertex ids per direction.
//   k_wm_vertices    a wave per vertex brick, a lane per corner of a level: the corner list, ascending in (owner, local word).
// The build waits three times: for the archive's counters, for the number of bricks of the field, and for the numbers of
// faces, vertex bricks and vertices.  It includes nothing of mesh.hip or of a frame unit.
#include "sdm_world.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_world_mesh_options) == 80 && sizeof(sdm_world_mesh_face) == 12 && sizeof(sdm_world_mesh_info) == 200, "sdm.h layout");
static_assert(offsetof(sdm_world_mesh_options, bmin) == 40 && offsetof(sdm_world_mesh_options, max_faces) == 64 &&
                  offsetof(sdm_world_mesh_face, cell) == 4 && offsetof(sdm_world_mesh_face, dir) == 6 && offsetof(sdm_world_mesh_face, track) == 8 &&
                  offsetof(sdm_world_mesh_face, occ) == 11 && offsetof(sdm_world_mesh_info, n_faces) == 8 &&
                  offsetof(sdm_world_mesh_info, faces_by_dir) == 32 && offsetof(sdm_world_mesh_info, stamp) == 112 &&
                  offsetof(sdm_world_mesh_info, options) == 120,
              "sdm.h layout");

namespace sdm {

namespace {

constexpr int QT = 256;
constexpr uint32_t ALL_WM_FLAGS = SDM_WORLD_MESH_STATIC_ONLY | SDM_WORLD_MESH_MOVABLE_ONLY | SDM_WORLD_MESH_OBSERVED_ONLY |
                                  SDM_WORLD_MESH_SKIP_UNKNOWN_FACES | SDM_WORLD_MESH_SKIP_ABSENT_FACES | SDM_WORLD_MESH_BOX;
// the build's counters, 64 bits each: solid cells, faces by direction, faces by kind; vertex bricks, vertices, faces
enum { C_SOLID = 0, C_DIR = 1, C_KIND = 7, C_COUNTS = 11, C_VB = 11, C_VERTS = 12, C_FACES = 13, C_WORDS = 16 };
constexpr int SUM_BLOCKS = 16;   // workgroups of k_wm_sums
constexpr uint32_t KEY_LO_BITS = 27;  // a vertex brick's key is sorted as 27 + 24 bits: three 9-bit digits each

constexpr size_t ARCH_BYTES = 4 + 4 + 3 * 8 * 8;              // flag, rank, solid, unknown and occupied words
constexpr size_t BRICK_BYTES = 8 + 4 + 6 * 4 + 2 * 8 * 4 + 8 * 4;  // coord, slot, nbr, owners' slot and rank, pre (and 44 B of counts per 8)
constexpr size_t SLOT_BYTES = 8 + 4 + 4 + 8 * 8;              // key, rank, place in the list, corner bits (and 4 B of counts per 64)
constexpr size_t VB_BYTES = 4 * 4 + 8 * 4;                    // the sort's buffers, the levels' prefix
static_assert(ARCH_BYTES == SDM_WORLD_MESH_BYTES_PER_ARCHIVED_BRICK && BRICK_BYTES == SDM_WORLD_MESH_BYTES_PER_BRICK &&
                  SLOT_BYTES == SDM_WORLD_MESH_BYTES_PER_VERTEX_SLOT && VB_BYTES == SDM_WORLD_MESH_BYTES_PER_VERTEX_BRICK &&
                  sizeof(sdm_world_mesh_face) + 16 == SDM_WORLD_MESH_BYTES_PER_FACE && SDM_WORLD_MESH_BYTES_PER_VERTEX == 12,
              "sdm.h states the bytes");

struct Rule {  // what makes a cell solid, by value
  uint32_t flags;
  int track, max_movable;
  uint32_t labels[8];
};

__device__ __forceinline__ bool is_solid(const Rule &g, uint32_t w1) {
  const int occ = occ_of(w1);
  const uint32_t track = w1 & 0xffffu, label = (w1 >> 16) & 0xffu;
  const bool movable = track >= 1u && (int)track <= g.max_movable;
  uint32_t lw = 0u;  // (selects, not an index: the mask stays in scalar registers)
#pragma unroll
  for (uint32_t k = 0; k < 8u; ++k) lw = (label >> 5) == k ? g.labels[k] : lw;
  bool s = (g.flags & SDM_WORLD_MESH_OBSERVED_ONLY) ? occ == 1 : occ >= 1;
  s = s && ((lw >> (label & 31u)) & 1u);
  s = s && (g.track < 0 || (int)track == g.track);
  s = s && !((g.flags & SDM_WORLD_MESH_STATIC_ONLY) && movable) && !((g.flags & SDM_WORLD_MESH_MOVABLE_ONLY) && !movable);
  return s;
}

// a vertex brick's key: 17 bits an axis (-32768 .. 32768), z highest - ascending keys are brick order
__device__ __forceinline__ u64 vkey(int bx, int by, int bz) {
  return (u64)(uint32_t)(bx + 32768) | ((u64)(uint32_t)(by + 32768) << 17) | ((u64)(uint32_t)(bz + 32768) << 34);
}
// the table slot of a key, claimed if nobody has it yet (the table is never more than half full); NONE: never
__device__ __forceinline__ uint32_t vclaim(u64 *__restrict__ keys, uint32_t hmask, u64 key) {
  uint32_t h = key_hash(key) & hmask;
  for (uint32_t i = 0; i <= hmask; ++i) {
    const u64 was = atomicCAS(keys + h, EMPTY_KEY, key);
    if (was == EMPTY_KEY || was == key) return h;
    h = (h + 1u) & hmask;
  }
  return NONE;
}
__device__ __forceinline__ uint32_t vfind(const u64 *__restrict__ keys, uint32_t hmask, u64 key) {
  uint32_t h = key_hash(key) & hmask;
  for (uint32_t i = 0; i <= hmask; ++i) {
    const u64 k = keys[h];
    if (k == key) return h;
    if (k == EMPTY_KEY) return NONE;
    h = (h + 1u) & hmask;
  }
  return NONE;
}

// ---- classify, neighbours ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wm_classify(const uint32_t *__restrict__ cells, uint32_t n_arch, Rule g, u64 *__restrict__ solid_m,
                                                    u64 *__restrict__ unk_m, u64 *__restrict__ occ_m) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t slot = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);  // (the pool is dense: n_arch slots are in use)
  if (slot >= n_arch) return;                                          // (wave-uniform)
  uint32_t w[8];
  load_brick(cells, slot, lane, w);
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    const int occ = occ_of(w[l]);
    const u64 um = __ballot(occ == -1), om = __ballot(occ >= 1);
    const u64 sm = om ? __ballot(is_solid(g, w[l])) : 0ull;  // (uniform)
    if (lane == 0) {
      solid_m[(size_t)slot * 8u + l] = sm;
      unk_m[(size_t)slot * 8u + l] = um;
      occ_m[(size_t)slot * 8u + l] = om;
    }
  }
}

__global__ __launch_bounds__(QT) void k_wm_neighbours(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr,
                                                      const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n_arch, uint32_t n,
                                                      const u64 *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t hmask,
                                                      uint32_t *__restrict__ coord, uint32_t *__restrict__ slot_of, uint32_t *__restrict__ nbr) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  const uint32_t j = i >> 3, f = i & 7u;
  if (j >= n_arch || f == 7u || !flag[j]) return;
  const uint32_t r = rank[j];
  if (r >= n) return;  // (never: the scan's total is n)
  const uint32_t slot = order[j];
  const uint32_t h0 = hdr[(size_t)slot * HDR_WORDS], h1 = hdr[(size_t)slot * HDR_WORDS + 1] & 0xffffu;
  if (f == 6u) {
    coord[2 * (size_t)r] = h0;
    coord[2 * (size_t)r + 1] = h1;
    slot_of[r] = slot < n_arch ? slot : NONE;  // (always a slot)
    return;
  }
  int b[3];
  brick_of(h0, h1, b[0], b[1], b[2]);
  b[f >> 1] += (f & 1u) ? 1 : -1;
  // (a coordinate of 32768 would alias another brick's key)
  const uint32_t s = brick_in_range(b[0], b[1], b[2]) ? world_find(keys, vals, hmask, brick_key(b[0], b[1], b[2])) : NONE;
  nbr[(size_t)r * 6u + f] = s < n_arch ? s : NONE;
}

// ---- the face words --------------------------------------------------------------------------------------------------
// what the cells of slice z of the brick at `slot` see across face `dir` in mask M (own: the slice's own word); the cells
// of an absent brick read 0
template <int DIR>
__device__ __forceinline__ u64 across(const u64 *__restrict__ M, uint32_t slot, const uint32_t (&nb)[6], int z, u64 own) {
  if constexpr (DIR < 4) return across_lateral<DIR>(own, nb[DIR] != NONE ? M[(size_t)nb[DIR] * 8u + (uint32_t)z] : 0ull);
  if (DIR == 4) return z > 0 ? M[(size_t)slot * 8u + (uint32_t)(z - 1)] : nb[4] != NONE ? M[(size_t)nb[4] * 8u + 7u] : 0ull;
  return z < 7 ? M[(size_t)slot * 8u + (uint32_t)(z + 1)] : nb[5] != NONE ? M[(size_t)nb[5] * 8u] : 0ull;
}

struct Masks {
  const u64 *solid_m, *unk_m, *occ_m;
};

template <int DIR>
__device__ __forceinline__ void face_dir(const Masks &k, uint32_t slot, const uint32_t (&nb)[6], int z, uint32_t flags, u64 solid, u64 unk, u64 occ,
                                         u64 &f, u64 &k1, u64 &k2, u64 &k3) {
  constexpr u64 border = DIR == 0 ? COL0 : DIR == 1 ? COL7 : DIR == 2 ? ROW0 : DIR == 3 ? ROW7 : ~0ull;
  u64 face = solid & ~across<DIR>(k.solid_m, slot, nb, z, solid);
  f = k1 = k2 = k3 = 0ull;
  if (!face) return;
  const bool at_seam = DIR < 4 || (DIR == 4 ? z == 0 : z == 7);
  k2 = at_seam && nb[DIR] == NONE ? face & border : 0ull;
  k1 = face & across<DIR>(k.unk_m, slot, nb, z, unk);
  k3 = face & across<DIR>(k.occ_m, slot, nb, z, occ);  // (not solid, or it were no face)
  if (flags & SDM_WORLD_MESH_SKIP_UNKNOWN_FACES) face &= ~k1, k1 = 0ull;
  if (flags & SDM_WORLD_MESH_SKIP_ABSENT_FACES) face &= ~k2, k2 = 0ull;
  f = face;
}

// Per direction (x-, x+, y-, y+, z-, z+) of slice z of the brick at `slot`, whose solid cells are `solid`: f = the cells that
// have a face there under the skip flags, and of those k1 / k2 / k3 the faces of kind 1, 2, 3 (the rest are of kind 0).
__device__ __forceinline__ void face_masks(const Masks &k, uint32_t slot, const uint32_t (&nb)[6], int z, uint32_t flags, u64 solid, u64 (&f)[6],
                                           u64 (&k1)[6], u64 (&k2)[6], u64 (&k3)[6]) {
  const u64 unk = k.unk_m[(size_t)slot * 8u + (uint32_t)z], occ = k.occ_m[(size_t)slot * 8u + (uint32_t)z];
  face_dir<0>(k, slot, nb, z, flags, solid, unk, occ, f[0], k1[0], k2[0], k3[0]);
  face_dir<1>(k, slot, nb, z, flags, solid, unk, occ, f[1], k1[1], k2[1], k3[1]);
  face_dir<2>(k, slot, nb, z, flags, solid, unk, occ, f[2], k1[2], k2[2], k3[2]);
  face_dir<3>(k, slot, nb, z, flags, solid, unk, occ, f[3], k1[3], k2[3], k3[3]);
  face_dir<4>(k, slot, nb, z, flags, solid, unk, occ, f[4], k1[4], k2[4], k3[4]);
  face_dir<5>(k, slot, nb, z, flags, solid, unk, occ, f[5], k1[5], k2[5], k3[5]);
}

__global__ __launch_bounds__(QT) void k_wm_faces(const uint32_t *__restrict__ coord, const uint32_t *__restrict__ slot_of,
                                                 const uint32_t *__restrict__ nbr, Masks k, uint32_t n, uint32_t flags, uint32_t *__restrict__ cnt,
                                                 u64 *__restrict__ vkeys, u64 *__restrict__ vmask, uint32_t vhmask, uint32_t *__restrict__ rows) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  const bool in = i < n * 8u;
  const uint32_t r = i >> 3;
  const int z = (int)(i & 7u);
  const uint32_t slot = in ? slot_of[r] : NONE;
  const u64 solid = slot != NONE ? k.solid_m[(size_t)slot * 8u + (uint32_t)z] : 0ull;
  u64 f[6] = {}, k1[6] = {}, k2[6] = {}, k3[6] = {};
  if (solid) {
    uint32_t nb[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) nb[d] = nbr[(size_t)r * 6u + d];
    face_masks(k, slot, nb, z, flags, solid, f, k1, k2, k3);
  }
  uint32_t st[C_COUNTS] = {};
  st[C_SOLID] = (uint32_t)__popcll(solid);
  uint32_t nf = 0;
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    const uint32_t c = (uint32_t)__popcll(f[d]);
    nf += c;
    st[C_DIR + d] = c;
    st[C_KIND + 0] += (uint32_t)__popcll(f[d] & ~(k1[d] | k2[d] | k3[d]));
    st[C_KIND + 1] += (uint32_t)__popcll(k1[d]);
    st[C_KIND + 2] += (uint32_t)__popcll(k2[d]);
    st[C_KIND + 3] += (uint32_t)__popcll(k3[d]);
  }
  if (i <= n * 8u) cnt[i] = nf;  // (the entry behind the last slice is 0: the scan leaves the number of faces there)
  // the wave's row of counts: every lane is here.  No atomics on shared counters: k_wm_sums adds the rows up
  const bool any_solid = __ballot(solid != 0ull) != 0ull;
  if (any_solid) {
#pragma unroll
    for (int q = 0; q < C_COUNTS; ++q) st[q] = wave_sum(st[q]);
  }
  const uint32_t lane = threadIdx.x & 63u;
  if (lane < (uint32_t)C_COUNTS && (i >> 6) <= (n * 8u) >> 6) {
    uint32_t v = 0u;
#pragma unroll
    for (int q = 0; q < C_COUNTS; ++q)
      if ((int)lane == q) v = st[q];
    rows[(size_t)(i >> 6) * C_COUNTS + lane] = any_solid ? v : 0u;
  }
  if (!nf) return;
  // the corners: per dz the plane z + dz takes, of the cells that use their corner (dx, dy, dz), bit (cx + dx, cy + dy) -
  // 9 x 9 bits, which fall to the owners (ox, oy) as a word, a column, a row and a bit
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
#pragma unroll
  for (int dz = 0; dz < 2; ++dz) {
    const u64 fz = f[4 + dz];
    const u64 u00 = f[0] | f[2] | fz, u10 = f[1] | f[2] | fz, u01 = f[0] | f[3] | fz, u11 = f[1] | f[3] | fz;
    const u64 a10 = (u10 & ~COL7) << 1, a11 = (u11 & ~COL7) << 1;  // dx = 1 inside the brick: one column up
    const u64 part[4] = {u00 | a10 | (u01 << 8) | (a11 << 8), ((u10 & COL7) >> 7) | (((u11 & COL7) >> 7) << 8), (u01 >> 56) | (a11 >> 56), u11 >> 63};
    const int zc = z + dz;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!part[q]) continue;
      const uint32_t h = vclaim(vkeys, vhmask, vkey(bx + (q & 1), by + (q >> 1), bz + (zc >> 3)));
      if (h != NONE) atomicOr(vmask + (size_t)h * 8u + (uint32_t)(zc & 7), part[q]);  // (always a slot)
    }
  }
}

// ---- the vertex bricks in order -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QT) void k_wm_clear(u64 *__restrict__ vkeys, u64 *__restrict__ vmask, uint32_t slots) {
  const uint32_t h = blockIdx.x * QT + threadIdx.x;
  if (h >= slots) return;
  vkeys[h] = EMPTY_KEY;
  ulonglong2 *__restrict__ row = reinterpret_cast<ulonglong2 *>(vmask + (size_t)h * 8u);  // (64 bytes a slot, 64-byte aligned)
#pragma unroll
  for (int k = 0; k < 4; ++k) row[k] = make_ulonglong2(0ull, 0ull);
}

// a thread per table slot: 1 for a claimed one (the entry behind the last slot is 0: the scan leaves the number of vertex
// bricks there), and per wave the number of corner bits of its claimed slots
__global__ __launch_bounds__(QT) void k_wm_vflag(const u64 *__restrict__ vkeys, const u64 *__restrict__ vmask, uint32_t slots,
                                                 uint32_t *__restrict__ vflag, uint32_t *__restrict__ vrows) {
  const uint32_t h = blockIdx.x * QT + threadIdx.x;  // (slots is a multiple of 64 or 2 .. 32: the waves' rows are whole)
  const bool claimed = h < slots && vkeys[h] != EMPTY_KEY;
  uint32_t pc = 0;
  if (claimed) {
#pragma unroll
    for (int l = 0; l < 8; ++l) pc += (uint32_t)__popcll(vmask[(size_t)h * 8u + l]);
  }
  if (h <= slots) vflag[h] = claimed ? 1u : 0u;
  if (__ballot(claimed)) pc = wave_sum(pc);  // (uniform)
  if ((threadIdx.x & 63u) == 0u && h < slots) vrows[h >> 6] = pc;
}

// SUM_BLOCKS workgroups add the rows of k_wm_faces' waves and of k_wm_vflag's up into the counters, a reduction a wave and
// then a few hundred 64-bit atomics in all; the first thread adds the two totals the scans left
__global__ __launch_bounds__(QT) void k_wm_sums(const uint32_t *__restrict__ rows, uint32_t n_rows, const uint32_t *__restrict__ vrows, uint32_t n_vrows,
                                                const uint32_t *__restrict__ n_faces, const uint32_t *__restrict__ n_vb, u64 *__restrict__ meta) {
  const uint32_t t = blockIdx.x * QT + threadIdx.x, T = gridDim.x * QT;
  u64 wide[C_COUNTS] = {}, wide_verts = 0ull;
  for (uint32_t r = t; r < n_rows; r += T) {
#pragma unroll
    for (int q = 0; q < C_COUNTS; ++q) wide[q] += rows[(size_t)r * C_COUNTS + q];
  }
  for (uint32_t r = t; r < n_vrows; r += T) wide_verts += vrows[r];
#pragma unroll
  for (int q = 0; q < C_COUNTS; ++q) {
    const u64 v = wave_sum64(wide[q]);
    if ((threadIdx.x & 63u) == 0u && v) atomicAdd(meta + q, v);
  }
  const u64 v = wave_sum64(wide_verts);
  if ((threadIdx.x & 63u) == 0u && v) atomicAdd(meta + C_VERTS, v);
  if (t == 0u) {
    meta[C_FACES] = *n_faces;
    meta[C_VB] = *n_vb;
  }
}

__global__ __launch_bounds__(QT) void k_wm_vkeys(const u64 *__restrict__ vkeys, const uint32_t *__restrict__ vscan, uint32_t slots, uint32_t n_vb,
                                                 uint32_t *__restrict__ key_lo, uint32_t *__restrict__ val) {
  const uint32_t h = blockIdx.x * QT + threadIdx.x;
  if (h >= slots) return;
  const u64 key = vkeys[h];
  if (key == EMPTY_KEY) return;
  const uint32_t at = vscan[h];  // the claimed slots in table order; the sort makes it brick order
  if (at >= n_vb) return;        // (never: the scan's total is n_vb)
  key_lo[at] = (uint32_t)(key & ((1ull << KEY_LO_BITS) - 1ull));
  val[at] = h;
}

__global__ __launch_bounds__(QT) void k_wm_vkeys_hi(const u64 *__restrict__ vkeys, uint32_t slots, uint32_t n_vb, const uint32_t *__restrict__ val,
                                                    uint32_t *__restrict__ key_hi) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n_vb) return;
  const uint32_t h = val[i];
  key_hi[i] = h < slots ? (uint32_t)(vkeys[h] >> KEY_LO_BITS) : 0u;  // (always a slot; 24 bits)
}

__global__ __launch_bounds__(QT) void k_wm_vrank(const uint32_t *__restrict__ sorted, const u64 *__restrict__ vmask, uint32_t slots, uint32_t n_vb,
                                                 uint32_t *__restrict__ vvals, uint32_t *__restrict__ vcnt) {
  const uint32_t t = blockIdx.x * QT + threadIdx.x;
  if (t > n_vb * 8u) return;
  if (t == n_vb * 8u) {  // (the entry behind the last level: the scan leaves the number of vertices there)
    vcnt[t] = 0u;
    return;
  }
  const uint32_t i = t >> 3, l = t & 7u, h = sorted[i];
  if (h >= slots) {  // (never)
    vcnt[t] = 0u;
    return;
  }
  vcnt[t] = (uint32_t)__popcll(vmask[(size_t)h * 8u + l]);
  if (l == 0u) vvals[h] = i;
}

__global__ __launch_bounds__(QT) void k_wm_owners(const uint32_t *__restrict__ coord, uint32_t n, const u64 *__restrict__ vkeys,
                                                  const uint32_t *__restrict__ vvals, uint32_t vhmask, uint32_t n_vb, uint32_t *__restrict__ own_h,
                                                  uint32_t *__restrict__ own_i) {
  const uint32_t t = blockIdx.x * QT + threadIdx.x;
  if (t >= n * 8u) return;
  const uint32_t r = t >> 3, o = t & 7u;
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
  const uint32_t h = vfind(vkeys, vhmask, vkey(bx + (int)(o & 1u), by + (int)((o >> 1) & 1u), bz + (int)(o >> 2)));
  const uint32_t i = h != NONE ? vvals[h] : NONE;
  own_h[t] = i < n_vb ? h : NONE;
  own_i[t] = i < n_vb ? i : NONE;
}

// ---- the lists -----------------------------------------------------------------------------------------------------
// the corners q0..q3 of the quad of direction dir as offsets from the cell, bit a of an entry = the offset along axis a:
// counter-clockwise seen from outside, q0 the smallest corner (sdm.h's table, "surface mesh")
__device__ __forceinline__ uint32_t quad_corner(int dir, int q) {
  constexpr uint8_t Q[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};
  return Q[dir][q];
}

__global__ __launch_bounds__(QT) void k_wm_emit(const uint32_t *__restrict__ slot_of, const uint32_t *__restrict__ nbr, Masks k, uint32_t n,
                                                uint32_t flags, const uint32_t *__restrict__ pre, const uint32_t *__restrict__ cells,
                                                const uint32_t *__restrict__ own_h, const uint32_t *__restrict__ own_i, const u64 *__restrict__ vmask,
                                                const uint32_t *__restrict__ vpre, uint32_t n_faces, uint32_t *__restrict__ faces,
                                                uint32_t *__restrict__ quads) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n * 8u) return;
  const uint32_t r = i >> 3;
  const int z = (int)(i & 7u);
  const uint32_t slot = slot_of[r];
  if (slot == NONE) return;  // (never)
  const u64 solid = k.solid_m[(size_t)slot * 8u + (uint32_t)z];
  if (!solid) return;
  uint32_t nb[6];
#pragma unroll
  for (int d = 0; d < 6; ++d) nb[d] = nbr[(size_t)r * 6u + d];
  u64 f[6], k1[6], k2[6], k3[6];
  face_masks(k, slot, nb, z, flags, solid, f, k1, k2, k3);
  u64 todo = f[0] | f[1] | f[2] | f[3] | f[4] | f[5];  // the cells with a face, taken in ascending order
  if (!todo) return;
  // the corner words and prefixes of the slice's owners: (ox, oy) at levels z and z + 1, every load issued before the first
  // is used; an owner no corner of the brick belongs to gives numbers nobody reads
  u64 m[2][4];
  uint32_t p[2][4];
  {
    uint32_t oh[2][4], oi[2][4];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t o = (uint32_t)q + 4u * (uint32_t)((z + dz) >> 3);
        oh[dz][q] = own_h[(size_t)r * 8u + o];
        oi[dz][q] = own_i[(size_t)r * 8u + o];
      }
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t l = (uint32_t)((z + dz) & 7);
        const bool ok = oh[dz][q] != NONE;
        m[dz][q] = ok ? vmask[(size_t)oh[dz][q] * 8u + l] : 0ull;
        p[dz][q] = ok ? vpre[(size_t)oi[dz][q] * 8u + l] : 0u;
      }
  }
  const uint32_t *__restrict__ src = cells + (size_t)slot * 512u + (uint32_t)z * 64u;
  uint32_t at = pre[i];  // the rank of the slice's first face; its faces stay below n_faces
  while (todo) {
    const uint32_t b = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    const uint32_t w1 = src[b];  // track | label << 16 | occ << 24: the record's third word
    const uint32_t x = b & 7u, y = b >> 3;
    uint32_t id[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const uint32_t X = x + ((uint32_t)o & 1u), Y = y + (((uint32_t)o >> 1) & 1u);
      const uint32_t q = (X >> 3) | ((Y >> 3) << 1), bit = (X & 7u) | ((Y & 7u) << 3);
      const int dz = o >> 2;
      const u64 mm = q == 0u ? m[dz][0] : q == 1u ? m[dz][1] : q == 2u ? m[dz][2] : m[dz][3];
      const uint32_t pp = q == 0u ? p[dz][0] : q == 1u ? p[dz][1] : q == 2u ? p[dz][2] : p[dz][3];
      id[o] = pp + lane_rank(mm, bit);
    }
#pragma unroll
    for (int dir = 0; dir < 6; ++dir) {
      if (!((f[dir] >> b) & 1ull)) continue;
      const uint32_t kind = ((k1[dir] >> b) & 1ull) ? 1u : (((k2[dir] >> b) & 1ull) ? 2u : (((k3[dir] >> b) & 1ull) ? 3u : 0u));
      if (at < n_faces) {  // (always: the scan's total is n_faces)
        uint32_t *face = faces + 3 * (size_t)at;
        face[0] = r;
        face[1] = ((uint32_t)z * 64u + b) | ((uint32_t)dir << 16) | (kind << 24);
        face[2] = w1;
        *reinterpret_cast<uint4 *>(quads + 4 * (size_t)at) =
            make_uint4(id[quad_corner(dir, 0)], id[quad_corner(dir, 1)], id[quad_corner(dir, 2)], id[quad_corner(dir, 3)]);
      }
      ++at;
    }
  }
}

__global__ __launch_bounds__(QT) void k_wm_vertices(const uint32_t *__restrict__ sorted, const u64 *__restrict__ vkeys, const u64 *__restrict__ vmask,
                                                    const uint32_t *__restrict__ vpre, uint32_t slots, uint32_t n_vb, uint32_t n_verts,
                                                    int32_t *__restrict__ corners) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * (QT / 64) + (threadIdx.x >> 6);
  if (i >= n_vb) return;  // (wave-uniform)
  const uint32_t h = sorted[i];
  if (h >= slots) return;  // (never)
  const u64 key = vkeys[h];
  u64 mw[8];
  uint32_t pr[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) {  // every load first
    mw[l] = vmask[(size_t)h * 8u + l];
    pr[l] = vpre[(size_t)i * 8u + l];
  }
  const int gx = ((int)(key & 0x1ffffu) - 32768) * 8 + (int)(lane & 7u), gy = ((int)((key >> 17) & 0x1ffffu) - 32768) * 8 + (int)(lane >> 3);
  const int gz0 = ((int)((key >> 34) & 0x1ffffu) - 32768) * 8;
#pragma unroll
  for (int l = 0; l < 8; ++l) {
    if (!((mw[l] >> lane) & 1ull)) continue;
    const uint32_t v = pr[l] + lane_rank(mw[l], lane);
    if (v >= n_verts) continue;  // (never: the scan's total is n_verts)
    corners[3 * (size_t)v] = gx;
    corners[3 * (size_t)v + 1] = gy;
    corners[3 * (size_t)v + 2] = gz0 + l;
  }
}

// a scan length whose scratch holds `elems` words (scan_scratch_elems: the fixed region and a word a tile of 2048 beyond 512)
size_t scan_length_for(size_t elems) { return std::max<size_t>(elems, 1032 + 513) * 2048 - (size_t)1032 * 2048; }

// the buffers for n_arch archived bricks / `bricks` bricks of the field / vb vertex bricks / the two lists (the stream is
// idle when any of them is called)
sdm_status grow_arch(sdm_map *m, size_t n_arch) {
  WorldMeshLayer &L = m->wmesh;
  const size_t cap = round_up(n_arch + 1, 256);
  return grow_buffers(m, n_arch + 1, cap, &L.cap_arch,
                      {buf(&L.flag, cap), buf(&L.rank, cap), buf(&L.solid_m, cap * 8), buf(&L.unk_m, cap * 8), buf(&L.occ_m, cap * 8)});
}

sdm_status grow_bricks(sdm_map *m, size_t bricks) {
  WorldMeshLayer &L = m->wmesh;
  const size_t cap = round_up(bricks, 256), slots = table_slots(8 * cap);
  if (bricks > L.cap_bricks) L.cap_slots = 0;  // (grow_buffers' own test: the two capacities fall and rise together)
  return grow_buffers(m, bricks, cap, &L.cap_bricks,
                      {buf(&L.coord, cap * 2), buf(&L.slot_of, cap), buf(&L.nbr, cap * 6), buf(&L.own_h, cap * 8), buf(&L.own_i, cap * 8),
                       buf(&L.pre, cap * 8 + 1), buf(&L.vkeys, slots), buf(&L.vvals, slots), buf(&L.vmask, slots * 8), buf(&L.vflag, slots + 1),
                       buf(&L.rows, (cap / 8 + 1) * C_COUNTS), buf(&L.vrows, slots / 64 + 1)},
                      [&]() -> sdm_status {
                        L.cap_slots = slots;
                        return SDM_OK;
                      });
}

sdm_status grow_lists(sdm_map *m, size_t vb, size_t n_faces, size_t n_verts) {
  WorldMeshLayer &L = m->wmesh;
  const size_t cap_vb = round_up(vb, 256), cap_f = round_up(n_faces, 4096), cap_v = round_up(n_verts, 4096);
  SDM_TRY(grow_buffers(m, vb, cap_vb, &L.cap_vb, {buf(&L.sortbuf, cap_vb * 4), buf(&L.vpre, cap_vb * 8 + 1)}));
  SDM_TRY(grow_buffers(m, n_faces, cap_f, &L.cap_f, {buf(&L.faces, cap_f * 3), buf(&L.quads, cap_f * 4)}));
  return grow_buffers(m, n_verts, cap_v, &L.cap_v, {buf(&L.corners, cap_v * 3)});
}

Masks masks_of(const WorldMeshLayer &L) { return Masks{L.solid_m, L.unk_m, L.occ_m}; }

// up to the counts the build waits for: the face words' counts scanned, the corners marked and counted
hipError_t launch_wm_count(const sdm_map *m, const uint32_t *order, uint32_t n_arch, uint32_t n, const Rule &g, uint32_t *scan) {
  const WorldMeshLayer &L = m->wmesh;
  const WorldLayer &W = m->world;
  hipStream_t s = m->stream;
  const uint32_t slots = (uint32_t)L.cap_slots;
  hipError_t e;
  LAYER_LAUNCH(k_wm_clear, (slots + QT - 1) / QT, QT, s, L.vkeys, L.vmask, slots);  // no vertex brick, no corner of the build before
  LAYER_LAUNCH(k_wm_classify, (n_arch + QT / 64 - 1) / (QT / 64), QT, s, W.cells, n_arch, g, L.solid_m, L.unk_m, L.occ_m);
  LAYER_LAUNCH(k_wm_neighbours, (n_arch * 8u + QT - 1) / QT, QT, s, order, W.hdr, L.flag, L.rank, n_arch, n, W.keys, W.vals, W.hmask, L.coord, L.slot_of,
               L.nbr);
  LAYER_LAUNCH(k_wm_faces, (n * 8u) / QT + 1, QT, s, L.coord, L.slot_of, L.nbr, masks_of(L), n, g.flags, L.pre, L.vkeys, L.vmask, slots - 1, L.rows);
  exclusive_scan_u32(L.pre, L.pre, (size_t)n * 8 + 1, scan, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wm_vflag, slots / QT + 1, QT, s, L.vkeys, L.vmask, slots, L.vflag, L.vrows);
  exclusive_scan_u32(L.vflag, L.vflag, (size_t)slots + 1, scan, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wm_sums, SUM_BLOCKS, QT, s, L.rows, ((n * 8u) >> 6) + 1u, L.vrows, slots / 64u, L.pre + (size_t)n * 8, L.vflag + slots, L.meta);
  return hipSuccess;
}

// the vertex bricks in order, then the three lists
hipError_t launch_wm_lists(const sdm_map *m, uint32_t n, uint32_t n_vb, uint32_t n_faces, uint32_t n_verts, uint32_t flags, uint32_t *scratch) {
  const WorldMeshLayer &L = m->wmesh;
  hipStream_t s = m->stream;
  const uint32_t slots = (uint32_t)L.cap_slots;
  hipError_t e;
  uint32_t *buf[4] = {L.sortbuf, L.sortbuf + L.cap_vb, L.sortbuf + 2 * L.cap_vb, L.sortbuf + 3 * L.cap_vb};  // keys a, vals a, keys b, vals b
  LAYER_LAUNCH(k_wm_vkeys, (slots + QT - 1) / QT, QT, s, L.vkeys, L.vflag, slots, n_vb, buf[0], buf[1]);
  const int w1 = radix_sort_pairs(buf[0], buf[1], buf[2], buf[3], n_vb, (int)KEY_LO_BITS, scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t *ka = buf[2 * w1], *va = buf[2 * w1 + 1], *kb = buf[2 * (1 - w1)], *vb = buf[2 * (1 - w1) + 1];
  LAYER_LAUNCH(k_wm_vkeys_hi, (n_vb + QT - 1) / QT, QT, s, L.vkeys, slots, n_vb, va, ka);
  const int w2 = radix_sort_pairs(ka, va, kb, vb, n_vb, 51 - (int)KEY_LO_BITS, scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const uint32_t *sorted = w2 ? vb : va;
  LAYER_LAUNCH(k_wm_vrank, (n_vb * 8u) / QT + 1, QT, s, sorted, L.vmask, slots, n_vb, L.vvals, L.vpre);
  exclusive_scan_u32(L.vpre, L.vpre, (size_t)n_vb * 8 + 1, scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_wm_owners, (n * 8u + QT - 1) / QT, QT, s, L.coord, n, L.vkeys, L.vvals, slots - 1, n_vb, L.own_h, L.own_i);
  LAYER_LAUNCH(k_wm_emit, (n * 8u + QT - 1) / QT, QT, s, L.slot_of, L.nbr, masks_of(L), n, flags, L.pre, m->world.cells, L.own_h, L.own_i, L.vmask, L.vpre,
               n_faces, L.faces, L.quads);
  LAYER_LAUNCH(k_wm_vertices, (n_vb + QT / 64 - 1) / (QT / 64), QT, s, sorted, L.vkeys, L.vmask, L.vpre, slots, n_vb, n_verts, L.corners);
  return hipSuccess;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
namespace {
constexpr LayerName WORLD_MESH = {"the world mesh", "world mesh", "sdm_world_mesh_update", false};

sdm_status refuse_over(const WorldMeshLayer &L, const char *what) {
  char msg[240];
  std::snprintf(msg, sizeof(msg), "%lld faces and %lld vertices, max_faces is %lld and max_vertices %lld: call sdm_world_mesh_update with larger caps (or 0)",
                (long long)L.n_faces, (long long)L.n_vertices, (long long)L.opt.max_faces, (long long)L.opt.max_vertices);
  set_error(what, __FILE__, __LINE__, msg);
  return SDM_ERR_CAPACITY;
}
}  // namespace

extern "C" {

sdm_status sdm_world_mesh_update(sdm_map *m, const sdm_world_mesh_options *o) {
  const char *what = "sdm_world_mesh_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_WM_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if ((o->flags & SDM_WORLD_MESH_STATIC_ONLY) && (o->flags & SDM_WORLD_MESH_MOVABLE_ONLY)) return LAYER_REFUSE(what, "both STATIC_ONLY and MOVABLE_ONLY");
  if (o->track < -1 || o->track > 65535) return LAYER_REFUSE(what, "track not in -1..65535");
  if (o->max_faces < 0 || o->max_vertices < 0) return LAYER_REFUSE(what, "a negative cap");
  BrickBox box{};
  if (o->flags & SDM_WORLD_MESH_BOX) {  // (bmax < bmin: an empty box, a field of no bricks)
    box.use = 1u;
    for (int a = 0; a < 3; ++a) box.lo[a] = o->bmin[a], box.hi[a] = o->bmax[a];
  }
  SDM_TRY(layer_check(m, what, &m->world, WORLD));
  HIP_TRY(hipSetDevice(m->device));
  WorldMeshLayer &L = m->wmesh;
  hipStream_t s = m->stream;
  L.valid = false;  // (until this build is complete)
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, C_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, C_WORDS + 1, true));
  HIP_TRY(hipMemsetAsync(L.meta, 0, C_WORDS * sizeof(u64), s));
  Rule g{};
  g.flags = o->flags, g.track = o->track, g.max_movable = m->d.max_movable;
  for (int k = 0; k < 8; ++k) g.labels[k] = o->labels[k];
  // the bricks of the field: the archive's in brick order, those of the box ranked.  The longest scan of the build is the
  // one over the levels of the vertex bricks, of which a brick has at most eight; the sort's scratch is the scan's too
  const size_t most_vb = 8 * (size_t)m->world.max_bricks;
  SnapshotBricks b;
  SDM_TRY(snapshot_bricks(m, box, std::max<size_t>(most_vb * 8 + 1, scan_length_for(sort_scratch_elems(most_vb))), L.h_meta + C_WORDS,
                          [&](uint32_t n_arch, uint32_t **flag, uint32_t **rank) -> sdm_status {
                            SDM_TRY(grow_arch(m, n_arch));
                            *flag = L.flag, *rank = L.rank;
                            return SDM_OK;
                          },
                          &b));
  const uint32_t n = b.n;
  if (n) {
    SDM_TRY(grow_bricks(m, n));
    HIP_TRY(launch_wm_count(m, b.order, b.n_arch, n, g, b.scan));
  }
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, C_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // the third wait: the counts size the lists
  const uint32_t n_faces = (uint32_t)L.h_meta[C_FACES], n_vb = (uint32_t)L.h_meta[C_VB], n_verts = (uint32_t)L.h_meta[C_VERTS];
  L.n = n;
  L.n_vb = n_vb;
  L.n_faces = (int64_t)n_faces;
  L.n_vertices = (int64_t)n_verts;
  for (int q = 0; q < C_COUNTS; ++q) L.counts[q] = (int64_t)L.h_meta[q];
  L.opt = *o;
  L.stamp = m->world.f.gts;
  L.over = (o->max_faces > 0 && L.n_faces > o->max_faces) || (o->max_vertices > 0 && L.n_vertices > o->max_vertices);
  if (L.over) {  // nothing is written past a cap, nothing is truncated: the getters say so too
    L.built(m->world.f, o->flags);
    return refuse_over(L, what);
  }
  if (n_faces) {
    SDM_TRY(grow_lists(m, n_vb, n_faces, n_verts));
    HIP_TRY(launch_wm_lists(m, n, n_vb, n_faces, n_verts, o->flags, b.scan));
  }
  L.built(m->world.f, o->flags);
  return SDM_OK;
}

sdm_status sdm_get_world_mesh_info(sdm_map *m, sdm_world_mesh_info *info) {
  const char *what = "sdm_get_world_mesh_info";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!info) return LAYER_REFUSE(what, "no info");
  SDM_TRY(layer_check(m, what, &m->wmesh, WORLD_MESH));
  const WorldMeshLayer &L = m->wmesh;  // (the build waited for every count)
  info->n_bricks = L.n;
  info->n_vertex_bricks = L.n_vb;
  info->n_faces = L.n_faces;
  info->n_vertices = L.n_vertices;
  info->n_solid = L.counts[C_SOLID];
  for (int q = 0; q < 6; ++q) info->faces_by_dir[q] = L.counts[C_DIR + q];
  for (int q = 0; q < 4; ++q) info->faces_by_kind[q] = L.counts[C_KIND + q];
  info->stamp = L.stamp;
  info->pad = 0u;
  info->options = L.opt;
  return SDM_OK;
}

sdm_status sdm_get_world_mesh_faces(sdm_map *m, int16_t *coords, sdm_world_mesh_face *faces, uint32_t *quads, int64_t first, int64_t cap,
                                    int64_t *n_out) {
  const char *what = "sdm_get_world_mesh_faces";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wmesh, WORLD_MESH));
  const WorldMeshLayer &L = m->wmesh;
  *n_out = L.n_faces;
  if (L.over) return refuse_over(L, what);
  HIP_TRY(hipSetDevice(m->device));
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>(L.n_faces - first, cap), 0);
  std::vector<uint32_t> pairs(coords && first == 0 ? 2 * (size_t)L.n : 0);
  if (!pairs.empty()) HIP_TRY(hipMemcpyAsync(pairs.data(), L.coord, pairs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (take && faces) HIP_TRY(hipMemcpyAsync(faces, L.faces + 3 * (size_t)first, take * sizeof(sdm_world_mesh_face), hipMemcpyDeviceToHost, m->stream));
  if (take && quads) HIP_TRY(hipMemcpyAsync(quads, L.quads + 4 * (size_t)first, take * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  unpack_coords(pairs, coords);
  return SDM_OK;
}

sdm_status sdm_get_world_mesh_vertices(sdm_map *m, int32_t *corners, float *xyz, int64_t first, int64_t cap, int64_t *n_out) {
  const char *what = "sdm_get_world_mesh_vertices";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (first < 0 || cap < 0 || !n_out) return LAYER_REFUSE(what, "first < 0, cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->wmesh, WORLD_MESH));
  const WorldMeshLayer &L = m->wmesh;
  *n_out = L.n_vertices;
  if (L.over) return refuse_over(L, what);
  const size_t take = (size_t)std::max<int64_t>(std::min<int64_t>(L.n_vertices - first, cap), 0);
  if (take && (corners || xyz)) {
    HIP_TRY(hipSetDevice(m->device));
    std::vector<int32_t> own;
    if (!corners) {
      own.resize(3 * take);
      corners = own.data();
    }
    HIP_TRY(hipMemcpyAsync(corners, L.corners + 3 * (size_t)first, take * 12, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (xyz) {
      const float size = m->d.voxel_size;
      for (size_t k = 0; k < 3 * take; ++k) xyz[k] = (float)corners[k] * size;  // (one float32 multiply: the archive's rule)
    }
  }
  return SDM_OK;
}

sdm_status sdm_world_mesh_device(sdm_map *m, const sdm_world_mesh_face **faces, const uint32_t **quads, const int32_t **corners) {
  const char *what = "sdm_world_mesh_device";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, what, &m->wmesh, WORLD_MESH));
  const WorldMeshLayer &L = m->wmesh;
  if (L.over) return refuse_over(L, what);
  if (faces) *faces = reinterpret_cast<const sdm_world_mesh_face *>(L.faces);
  if (quads) *quads = L.quads;
  if (corners) *corners = L.corners;
  return SDM_OK;
}

}  // extern "C"
