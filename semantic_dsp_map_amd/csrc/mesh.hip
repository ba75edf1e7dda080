// mesh.hip — the surface mesh of the map block: one unit quad per face between a solid cell and a neighbour that is not
// solid, the lattice corners those faces use as welded vertices (gfx950; include/sdm.h, "surface mesh").
//
// A snapshot of one frame in map-index cells, like the frontiers.  Only the first and the emitting kernel read State::res;
// everything between them works on three bitmasks of V / 8 bytes each and one over the (NX+1)(NY+1)(NZ+1) corners.
//   k_mesh_classify  a wave per chunk of 64 cells in map-index order (MC_U chunks a wave, all loads first): reads the
//               results' second word through the ring correction and writes one word each of the `solid` (the options'
//               rule), the `unknown` (occ == -1) and the `occupied` (occ >= 1, solid or not) mask from three ballots.
//   k_mesh_faces     a thread per 64-bit word: the six face masks solid & ~(the solid bits of the face neighbour).  A
//               neighbour 2^s cells away is a shift by 2^s bits with the carry from the adjacent word (s < 6) or the word
//               2^(s-6) words away; line, plane and map ends are masked by coord_is(), so x rows of 4..32 cells that share
//               a word never see each other and the map is no torus: a cell on the map's end has a face of kind 2 there.
//               The other two masks give the kinds 1 and 3; the skip flags drop kinds 1 and 2.  Stores the word's face
//               count and marks the corners its faces use: the corner (dx, dy, dz) of a cell is used when the cell has its
//               x face on side dx, its y face on side dy or its z face on side dz, which for the 64 cells of the word are
//               three ORs; the bits of one x row go into the corner mask, whose rows are NX + 1 bits and never word-
//               aligned, with at most two 64-bit atomic ORs per row and (dy, dz).  ORs commute: the mask does not depend
//               on who arrives first.  Every wave also leaves the counts of its 64 words - solid cells, faces by direction
//               and by kind, all popcounts - in a row of its own.
//   k_mesh_corner_count   a thread per corner word: its popcount.
//   exclusive_scan_u32 x 2   over the words' face counts and the corner words' popcounts, each with one entry more than
//               there are words (a zero), so that the last entry ends as the total.
//   k_mesh_emit      a thread per cell word: builds the face masks again and walks the word's cells that have a face in
//               ascending order - per cell the ranks of its eight corners looked up at once (rank of a corner = its
//               word's prefix + the popcount of the lower bits), then a face record and four vertex ids per direction,
//               ranks counted up from the word's prefix: (cell, dir) order.  A wave per word with a lane per cell was
//               built first and measured: on a map whose obstacles are scattered nearly every word holds a solid cell or
//               two, so 262,144 waves at 256^3 each walked a chain of four dependent loads for one or two busy lanes -
//               459 us with eight words a wave, 381 us with one, of a 554 / 473 us build.  More faces or
//               vertices than the lists hold: nothing is written, the getters report SDM_ERR_CAPACITY with the true
//               counts.
//   k_mesh_vertices  a wave per corner word (MV_U words a wave, all loads first), a lane per corner: the sdm_mesh_vertex
//               list, ascending in corner word.
//   k_mesh_stats     MS_ROWS workgroups add the waves' rows up into MS_ROWS rows, which the getter adds up on the host: no
//               atomics on shared counters.  The faces of a build over capacity count as not emitted.
// The corner mask is zeroed at the start of every build.  The counts are only known on the device and sdm_mesh_update
// does not wait: every kernel runs on a grid fixed by the map, and the two over the lists read the totals behind the
// scans.
#include "sdm_layer.h"
#include "sdm_map.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_mesh_options) == 56 && sizeof(sdm_mesh_face) == 12 && sizeof(sdm_mesh_vertex) == 8 && sizeof(sdm_mesh_info) == 112,
              "sdm.h layout");
static_assert(offsetof(sdm_mesh_options, max_faces) == 40 && offsetof(sdm_mesh_info, options) == 56 && offsetof(sdm_mesh_face, dir) == 8,
              "sdm.h layout");
static_assert(sizeof(sdm_mesh_face) + 4 * sizeof(uint32_t) == SDM_MESH_BYTES_PER_FACE, "sdm.h states the bytes per face");
static_assert(sizeof(sdm_mesh_vertex) == SDM_MESH_BYTES_PER_VERTEX, "sdm.h states the bytes per vertex");

namespace sdm {

namespace {

constexpr int MC_TPB = 256, MC_WAVES = MC_TPB / 64;
constexpr int MC_U = 8;        // chunks (words) a wave of k_mesh_classify takes
constexpr int MV_U = 4;        // corner words a wave of k_mesh_vertices takes
constexpr int MF_TPB = 256;    // the kernels of one thread per word
constexpr int MS_ROWS = 64;    // rows of counts the getter adds up
enum { META_N_FACES = 0, META_N_VERTICES, META_OVER, META_PAD, META_WORDS };
enum { ST_SOLID = 0, ST_DIR = 1, ST_KIND = 7, ST_WORDS = 11 };  // a row of counts: solid cells, faces by dir, faces by kind
constexpr uint32_t ALL_FLAGS = SDM_MESH_STATIC_ONLY | SDM_MESH_MOVABLE_ONLY | SDM_MESH_OBSERVED_ONLY | SDM_MESH_SKIP_UNKNOWN_FACES |
                               SDM_MESH_SKIP_BORDER_FACES;
constexpr size_t WORD_BYTES = 3 * sizeof(u64) + sizeof(uint32_t);   // per 64 cells: three masks and the face prefix
constexpr size_t CORNER_WORD_BYTES = sizeof(u64) + sizeof(uint32_t);  // per 64 corners: the mask and its prefix
static_assert(WORD_BYTES == SDM_MESH_BYTES_PER_WORD && CORNER_WORD_BYTES == SDM_MESH_BYTES_PER_CORNER_WORD, "sdm.h states the bytes");

struct Mesh {  // everything a build touches, by value
  u64 *solid_m, *unk_m, *occ_m;  // [nw]
  uint32_t *pre_f;               // [nw + 1]: face counts, then their exclusive scan; [nw] the total
  u64 *corner_m;                 // [ncw]
  uint32_t *pre_c;               // [ncw + 1]: likewise over the corner words
  uint32_t *faces;               // [cap_f] sdm_mesh_face as three words
  uint32_t *quads;               // [cap_f][4]
  sdm_mesh_vertex *verts;        // [cap_v]
  uint32_t *meta;                // [META_WORDS + MS_ROWS * ST_WORDS]
  uint32_t *wave_stats;          // [n_rows][ST_WORDS]: a row of counts per wave of k_mesh_faces, 64 words each
  uint32_t nw, ncw, n_rows, cap_f, cap_v;
  int x_n, y_n, z_n;
  uint32_t flags;
  int track, max_movable;
  uint32_t labels[8];
};

__device__ __forceinline__ bool is_solid(const Mesh &g, uint32_t w1) {
  const int occ = occ_of(w1);
  const uint32_t track = w1 & 0xffffu, label = (w1 >> 16) & 0xffu;
  const bool movable = track >= 1u && (int)track <= g.max_movable;
  uint32_t lw = 0u;  // (selects, not an index: the mask stays in scalar registers)
#pragma unroll
  for (uint32_t k = 0; k < 8u; ++k) lw = (label >> 5) == k ? g.labels[k] : lw;
  bool s = (g.flags & SDM_MESH_OBSERVED_ONLY) ? occ == 1 : occ >= 1;
  s = s && ((lw >> (label & 31u)) & 1u);
  s = s && (g.track < 0 || (int)track == g.track);
  s = s && !((g.flags & SDM_MESH_STATIC_ONLY) && movable) && !((g.flags & SDM_MESH_MOVABLE_ONLY) && !movable);
  return s;
}

// ---- classify ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_TPB) void k_mesh_classify(Dims d, Frame f, const uint2 *__restrict__ res, Mesh g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * MC_WAVES + (threadIdx.x >> 6)) * MC_U;
  uint32_t w[MC_U];
  load_w1(d, f, res, first, g.nw, lane, w);
#pragma unroll
  for (int u = 0; u < MC_U; ++u) {
    const uint32_t chunk = first + (uint32_t)u;
    if (chunk >= g.nw) break;  // (wave-uniform)
    const int occ = occ_of(w[u]);
    const u64 um = __ballot(occ == -1), om = __ballot(occ >= 1);
    const u64 sm = om ? __ballot(is_solid(g, w[u])) : 0ull;  // (uniform: most chunks of a map hold no obstacle)
    if (lane == 0) {
      g.solid_m[chunk] = sm;
      g.unk_m[chunk] = um;
      g.occ_m[chunk] = om;
    }
  }
}

// ---- the face masks ------------------------------------------------------------------------------------------------
// Per direction (x-, x+, y-, y+, z-, z+) of word wi, whose solid cells are `solid`: f = the cells that have a face there
// under the skip flags, and of those k1 / k2 / k3 the faces of kind 1, 2, 3 (the rest are of kind 0).
__device__ __forceinline__ void face_masks(const Mesh &g, uint32_t wi, u64 solid, u64 (&f)[6], u64 (&k1)[6], u64 (&k2)[6], u64 (&k3)[6]) {
  const uint32_t c0 = wi << 6;
  const int s[3] = {0, g.x_n, g.x_n + g.y_n}, nb[3] = {g.x_n, g.y_n, g.z_n};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int up = 0; up < 2; ++up) {
      const int dir = 2 * a + up;
      const u64 edge = coord_is(c0, s[a], nb[a], up ? (1u << nb[a]) - 1u : 0u);  // no neighbour inside the map
      const u64 ns = (up ? bits_up(g.solid_m, wi, g.nw, s[a]) : bits_down(g.solid_m, wi, s[a])) & ~edge;
      u64 face = solid & ~ns;
      f[dir] = k1[dir] = k2[dir] = k3[dir] = 0ull;
      if (!face) continue;
      const u64 nu = (up ? bits_up(g.unk_m, wi, g.nw, s[a]) : bits_down(g.unk_m, wi, s[a])) & ~edge;
      const u64 no = (up ? bits_up(g.occ_m, wi, g.nw, s[a]) : bits_down(g.occ_m, wi, s[a])) & ~edge;
      k1[dir] = face & nu;
      k2[dir] = face & edge;
      k3[dir] = face & no;  // (not solid, or it were no face)
      if (g.flags & SDM_MESH_SKIP_UNKNOWN_FACES) face &= ~k1[dir], k1[dir] = 0ull;
      if (g.flags & SDM_MESH_SKIP_BORDER_FACES) face &= ~k2[dir], k2[dir] = 0ull;
      f[dir] = face;
    }
  }
}

__global__ __launch_bounds__(MF_TPB) void k_mesh_faces(Mesh g) {
  const uint32_t wi = blockIdx.x * MF_TPB + threadIdx.x;  // (nw is a multiple of 64 or 1..63 words of one wave: the waves' rows are whole)
  const bool in = wi < g.nw;
  if (wi == 0u) g.pre_f[g.nw] = 0u;  // the scan's extra entry: the total lands there
  const u64 solid = in ? g.solid_m[wi] : 0ull;
  u64 f[6] = {}, k1[6] = {}, k2[6] = {}, k3[6] = {};
  if (solid) face_masks(g, wi, solid, f, k1, k2, k3);
  uint32_t st[ST_WORDS] = {};
  st[ST_SOLID] = (uint32_t)__popcll(solid);
  uint32_t n = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const uint32_t c = (uint32_t)__popcll(f[i]);
    n += c;
    st[ST_DIR + i] = c;
    st[ST_KIND + 0] += (uint32_t)__popcll(f[i] & ~(k1[i] | k2[i] | k3[i]));
    st[ST_KIND + 1] += (uint32_t)__popcll(k1[i]);
    st[ST_KIND + 2] += (uint32_t)__popcll(k2[i]);
    st[ST_KIND + 3] += (uint32_t)__popcll(k3[i]);
  }
  if (in) g.pre_f[wi] = n;
  // the wave's row of counts: every lane is here
  const uint32_t lane = threadIdx.x & 63u;
  const bool any_solid = __ballot(solid != 0ull) != 0ull;
  if (any_solid) {
#pragma unroll
    for (int q = 0; q < ST_WORDS; ++q) st[q] = wave_sum(st[q]);
  }
  if (lane < ST_WORDS && (wi >> 6) < g.n_rows) {
    uint32_t v = 0u;
#pragma unroll
    for (int q = 0; q < ST_WORDS; ++q)
      if ((int)lane == q) v = st[q];
    g.wave_stats[(size_t)(wi >> 6) * ST_WORDS + lane] = any_solid ? v : 0u;
  }
  if (!n) return;
  // the corners: per (dy, dz) the corner row y + dy, z + dz takes, of every x row of the word, bits x (dx = 0) and x + 1
  const uint32_t NX = 1u << g.x_n, NY = 1u << g.y_n;
  const uint32_t L = NX < 64u ? NX : 64u;            // cells of one x row inside the word
  const u64 row_mask = L == 64u ? ~0ull : (1ull << L) - 1ull;
  const uint32_t c0 = wi << 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t dy = (uint32_t)q & 1u, dz = (uint32_t)q >> 1;
    const u64 yz = f[2 + (q & 1)] | f[4 + (q >> 1)];
    const u64 u0 = f[0] | yz, u1 = f[1] | yz;
    if (!(u0 | u1)) continue;
    for (uint32_t r = 0; r < 64u; r += L) {
      const u64 r0 = (u0 >> r) & row_mask, r1 = (u1 >> r) & row_mask;
      if (!(r0 | r1)) continue;
      const uint32_t c = c0 + r;
      uint32_t x, y, z;
      cell_xyz(g.x_n, g.y_n, c, x, y, z);
      const uint32_t o = x + (NX + 1u) * ((y + dy) + (NY + 1u) * (z + dz));  // the corner word of the row's first corner
      const u64 lo = r0 | (r1 << 1), hi = r1 >> 63;                          // L + 1 <= 65 bits from corner o on
      const uint32_t sh = o & 63u, w = o >> 6;
      const u64 w0 = lo << sh, w1 = (sh ? lo >> (64u - sh) : 0ull) | (hi << sh);
      // every bit set stands for a corner of the map: a word that gets one lies inside the mask
      if (w0) atomicOr(g.corner_m + w, w0);
      if (w1) atomicOr(g.corner_m + w + 1u, w1);
    }
  }
}

__global__ __launch_bounds__(MF_TPB) void k_mesh_corner_count(Mesh g) {
  const uint32_t w = blockIdx.x * MF_TPB + threadIdx.x;
  if (w >= g.ncw) return;
  if (w == 0u) g.pre_c[g.ncw] = 0u;
  g.pre_c[w] = (uint32_t)__popcll(g.corner_m[w]);
}

// ---- the lists -----------------------------------------------------------------------------------------------------
// the corners q0..q3 of the quad of direction dir as offsets from the cell, bit a of an entry = the offset along axis a:
// counter-clockwise seen from outside, q0 the smallest corner word (sdm.h's table)
__device__ __forceinline__ uint32_t quad_corner(int dir, int q) {
  constexpr uint8_t Q[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};
  return Q[dir][q];
}

__global__ __launch_bounds__(MF_TPB) void k_mesh_emit(Dims d, Frame fr, const uint2 *__restrict__ res, Mesh g) {
  const uint32_t n_faces = g.pre_f[g.nw], n_verts = g.pre_c[g.ncw];
  const bool over = n_faces > g.cap_f || n_verts > g.cap_v;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    g.meta[META_N_FACES] = n_faces;
    g.meta[META_N_VERTICES] = n_verts;
    g.meta[META_OVER] = over ? 1u : 0u;
    g.meta[META_PAD] = 0u;
  }
  if (over) return;  // nothing is written past a capacity, nothing is truncated
  const uint32_t wi = blockIdx.x * MF_TPB + threadIdx.x;
  if (wi >= g.nw) return;
  const u64 solid = g.solid_m[wi];
  if (!solid) return;
  const uint32_t NX = 1u << g.x_n, NY = 1u << g.y_n;
  u64 f[6], k1[6], k2[6], k3[6];
  face_masks(g, wi, solid, f, k1, k2, k3);
  u64 todo = f[0] | f[1] | f[2] | f[3] | f[4] | f[5];  // the cells with a face, taken in ascending order
  uint32_t r = g.pre_f[wi];                            // the rank of the word's first face; the word's faces stay below n_faces <= cap_f
  while (todo) {
    const uint32_t b = (uint32_t)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    const uint32_t c = (wi << 6) | b;
    uint32_t x, y, z;
    cell_xyz(g.x_n, g.y_n, c, x, y, z);
    const uint32_t w1 = res[cell_voxel(d, fr, (int)x, (int)y, (int)z)].y;  // track | label << 16 | occ << 24: the record's second word
    // the ranks of the cell's eight corners, every load issued before the first is used; a corner no face of the build
    // uses gets a number nobody reads
    uint32_t id[8];
    {
      u64 cm[8];
      uint32_t pre[8], bit[8];
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const uint32_t cw = (x + ((uint32_t)o & 1u)) + (NX + 1u) * ((y + (((uint32_t)o >> 1) & 1u)) + (NY + 1u) * (z + ((uint32_t)o >> 2)));
        cm[o] = g.corner_m[cw >> 6];
        pre[o] = g.pre_c[cw >> 6];
        bit[o] = cw & 63u;
      }
#pragma unroll
      for (int o = 0; o < 8; ++o) id[o] = pre[o] + lane_rank(cm[o], bit[o]);
    }
#pragma unroll
    for (int dir = 0; dir < 6; ++dir) {
      if (!((f[dir] >> b) & 1ull)) continue;
      const uint32_t kind = ((k1[dir] >> b) & 1ull) ? 1u : (((k2[dir] >> b) & 1ull) ? 2u : (((k3[dir] >> b) & 1ull) ? 3u : 0u));
      uint32_t *face = g.faces + 3 * (size_t)r;
      face[0] = c;
      face[1] = w1;
      face[2] = (uint32_t)dir | (kind << 8);
      *reinterpret_cast<uint4 *>(g.quads + 4 * (size_t)r) =
          make_uint4(id[quad_corner(dir, 0)], id[quad_corner(dir, 1)], id[quad_corner(dir, 2)], id[quad_corner(dir, 3)]);
      ++r;
    }
  }
}

__global__ __launch_bounds__(MC_TPB) void k_mesh_vertices(Mesh g) {
  const uint32_t n_faces = g.pre_f[g.nw], n_verts = g.pre_c[g.ncw];
  if (n_faces > g.cap_f || n_verts > g.cap_v) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t first = (blockIdx.x * MC_WAVES + (threadIdx.x >> 6)) * MV_U;
  const uint32_t RX = (1u << g.x_n) + 1u, RY = (1u << g.y_n) + 1u;
  u64 cm[MV_U];
  uint32_t pre[MV_U];
#pragma unroll
  for (int u = 0; u < MV_U; ++u) {  // every load first
    const uint32_t w = first + (uint32_t)u;
    cm[u] = w < g.ncw ? g.corner_m[w] : 0ull;
    pre[u] = w < g.ncw ? g.pre_c[w] : 0u;
  }
#pragma unroll
  for (int u = 0; u < MV_U; ++u) {
    if (!((cm[u] >> lane) & 1ull)) continue;
    const uint32_t r = pre[u] + lane_rank(cm[u], lane);  // < n_verts <= cap_v
    const uint32_t cw = ((first + (uint32_t)u) << 6) | lane, t = cw / RX;
    sdm_mesh_vertex v;
    v.i = (uint16_t)(cw - t * RX);
    v.j = (uint16_t)(t % RY);
    v.k = (uint16_t)(t / RY);
    v.pad = 0u;
    g.verts[r] = v;
  }
}

// workgroup b (one wave) adds the rows b, b + MS_ROWS, ... of k_mesh_faces' waves up into row b of meta; a build over
// capacity has emitted no face
__global__ __launch_bounds__(64) void k_mesh_stats(Mesh g) {
  const uint32_t lane = threadIdx.x;
  const bool over = g.pre_f[g.nw] > g.cap_f || g.pre_c[g.ncw] > g.cap_v;
  uint32_t st[ST_WORDS] = {};
  for (uint32_t row = blockIdx.x + MS_ROWS * lane; row < g.n_rows; row += MS_ROWS * 64u) {
#pragma unroll
    for (int q = 0; q < ST_WORDS; ++q) st[q] += g.wave_stats[(size_t)row * ST_WORDS + q];
  }
  if (over) {
#pragma unroll
    for (int q = ST_DIR; q < ST_WORDS; ++q) st[q] = 0u;
  }
#pragma unroll
  for (int q = 0; q < ST_WORDS; ++q) st[q] = wave_sum(st[q]);
  if (lane < ST_WORDS) {
    uint32_t v = 0u;
#pragma unroll
    for (int q = 0; q < ST_WORDS; ++q)
      if ((int)lane == q) v = st[q];
    g.meta[META_WORDS + blockIdx.x * ST_WORDS + lane] = v;
  }
}

size_t corner_count(const Dims &d) { return (size_t)(d.NX + 1) * (d.NY + 1) * (d.NZ + 1); }

Mesh mesh_of(const sdm_map *m, const sdm_mesh_options &o) {
  const Dims &d = m->d;
  const MeshLayer &L = m->mesh;
  Mesh g;
  g.nw = d.V >> 6;
  g.ncw = (uint32_t)((corner_count(d) + 63) / 64);
  g.n_rows = (g.nw + 63) / 64;
  g.solid_m = reinterpret_cast<u64 *>(L.bits);
  g.unk_m = g.solid_m + g.nw;
  g.occ_m = g.unk_m + g.nw;
  g.corner_m = g.occ_m + g.nw;
  g.pre_f = reinterpret_cast<uint32_t *>(g.corner_m + g.ncw);
  g.pre_c = g.pre_f + g.nw + 1;
  g.faces = reinterpret_cast<uint32_t *>(L.faces);
  g.quads = L.quads;
  g.verts = L.verts;
  g.meta = L.meta;
  g.wave_stats = L.stats;
  g.cap_f = (uint32_t)o.max_faces;
  g.cap_v = (uint32_t)o.max_vertices;
  g.x_n = d.x_n, g.y_n = d.y_n, g.z_n = d.z_n;
  g.flags = o.flags;
  g.track = o.track;
  g.max_movable = d.max_movable;
  for (int k = 0; k < 8; ++k) g.labels[k] = o.labels[k];
  return g;
}

hipError_t launch_mesh_build(const Dims &d, const Frame &f, const State &st, const Mesh &g, uint32_t *scan_scratch, hipStream_t s) {
  const uint2 *res = reinterpret_cast<const uint2 *>(st.res);
  const uint32_t classify_waves = (g.nw + MC_U - 1) / MC_U, corner_waves = (g.ncw + MV_U - 1) / MV_U;
  hipError_t e;
  if ((e = hipMemsetAsync(g.corner_m, 0, (size_t)g.ncw * sizeof(u64), s)) != hipSuccess) return e;  // no corner of the build before
  LAYER_LAUNCH(k_mesh_classify, (classify_waves + MC_WAVES - 1) / MC_WAVES, MC_TPB, s, d, f, res, g);
  LAYER_LAUNCH(k_mesh_faces, (g.nw + MF_TPB - 1) / MF_TPB, MF_TPB, s, g);
  LAYER_LAUNCH(k_mesh_corner_count, (g.ncw + MF_TPB - 1) / MF_TPB, MF_TPB, s, g);
  exclusive_scan_u32(g.pre_f, g.pre_f, (size_t)g.nw + 1, scan_scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  exclusive_scan_u32(g.pre_c, g.pre_c, (size_t)g.ncw + 1, scan_scratch, s);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  LAYER_LAUNCH(k_mesh_emit, (g.nw + MF_TPB - 1) / MF_TPB, MF_TPB, s, d, f, res, g);
  LAYER_LAUNCH(k_mesh_vertices, (corner_waves + MC_WAVES - 1) / MC_WAVES, MC_TPB, s, g);
  LAYER_LAUNCH(k_mesh_stats, MS_ROWS, 64, s, g);
  return hipSuccess;
}

constexpr LayerName MESH = {"the mesh", "mesh", "sdm_mesh_update", false};

// waits; the build's counters and the rows of counts added up
sdm_status mesh_meta(sdm_map *m, const char *what, uint32_t (&meta)[META_WORDS], uint32_t (&st)[ST_WORDS], bool report) {
  uint32_t all[META_WORDS + MS_ROWS * ST_WORDS];
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(all, m->mesh.meta, sizeof(all), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int q = 0; q < META_WORDS; ++q) meta[q] = all[q];
  for (int q = 0; q < ST_WORDS; ++q) st[q] = 0u;
  for (int r = 0; r < MS_ROWS; ++r)
    for (int q = 0; q < ST_WORDS; ++q) st[q] += all[META_WORDS + r * ST_WORDS + q];
  if (meta[META_OVER] && report) {
    char msg[200];
    std::snprintf(msg, sizeof(msg), "%u faces and %u vertices, the lists hold %lld and %lld: call sdm_mesh_update with larger capacities",
                  meta[META_N_FACES], meta[META_N_VERTICES], (long long)m->mesh.opt.max_faces, (long long)m->mesh.opt.max_vertices);
    set_error(what, __FILE__, __LINE__, msg);
  }
  return SDM_OK;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
// Like the other layers, the build reads the result array in stream order and takes the host Frame of the last issued
// frame by value; the Frame and the options (capacities resolved) stay with the layer.
extern "C" {

sdm_status sdm_mesh_update(sdm_map *m, const sdm_mesh_options *o) {
  const char *what = "sdm_mesh_update";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!o) return LAYER_REFUSE(what, "no options");
  if (o->flags & ~ALL_FLAGS) return LAYER_REFUSE(what, "unknown flag bits");
  if ((o->flags & SDM_MESH_STATIC_ONLY) && (o->flags & SDM_MESH_MOVABLE_ONLY)) return LAYER_REFUSE(what, "both STATIC_ONLY and MOVABLE_ONLY");
  if (o->track < -1 || o->track > 65535) return LAYER_REFUSE(what, "track not in -1..65535");
  if (o->max_faces < 0 || o->max_vertices < 0) return LAYER_REFUSE(what, "a negative capacity");
  SDM_TRY(layer_check(m, what, nullptr, MESH));
  HIP_TRY(hipSetDevice(m->device));
  const Dims &d = m->d;
  MeshLayer &L = m->mesh;
  const size_t nw = d.V >> 6, ncw = (corner_count(d) + 63) / 64, n_rows = (nw + 63) / 64;
  sdm_mesh_options opt = *o;
  opt.max_faces = o->max_faces == 0 ? (int64_t)std::max<size_t>(d.V / 8, 1) : std::min<int64_t>(o->max_faces, 6 * (int64_t)d.V);
  // (a cell that stands alone has 8 vertices to its 6 faces, a flat surface about one per face)
  opt.max_vertices = std::min<int64_t>(o->max_vertices == 0 ? opt.max_faces + opt.max_faces / 2 : o->max_vertices, (int64_t)corner_count(d));
  if (!L.bits) SDM_TRY(alloc_tracked(m, &L.bits, nw * WORD_BYTES + ncw * CORNER_WORD_BYTES + 2 * sizeof(uint32_t)));
  if (!L.meta) {
    SDM_TRY(alloc_tracked(m, &L.meta, (size_t)META_WORDS + MS_ROWS * ST_WORDS));
    SDM_TRY(alloc_tracked(m, &L.stats, n_rows * ST_WORDS));
  }
  uint32_t *scan = nullptr;
  SDM_TRY(layer_scan_scratch(m, std::max(nw, ncw) + 1, &scan));
  if ((size_t)opt.max_faces > L.alloc_f) {  // longer lists: the old ones go once the builds that use them have run
    size_t n = 0;
    L.alloc_f = 0;
    SDM_TRY(regrow(m, &L.faces, &n, (size_t)opt.max_faces, L.faces ? m->stream : nullptr));
    SDM_TRY(regrow(m, &L.quads, &n, 4 * (size_t)opt.max_faces));
    L.alloc_f = (size_t)opt.max_faces;
  }
  if ((size_t)opt.max_vertices > L.alloc_v) {
    L.alloc_v = 0;
    SDM_TRY(regrow(m, &L.verts, &L.alloc_v, (size_t)opt.max_vertices, L.verts ? m->stream : nullptr));
  }
  const Frame f = m->f;
  HIP_TRY(launch_mesh_build(d, f, m->st, mesh_of(m, opt), scan, m->stream));
  L.opt = opt;
  L.built(f, opt.flags);
  return SDM_OK;
}

sdm_status sdm_get_mesh_info(sdm_map *m, sdm_mesh_info *info, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_get_mesh_info", &m->mesh, MESH));
  if (info) {
    uint32_t meta[META_WORDS], st[ST_WORDS];
    SDM_TRY(mesh_meta(m, "sdm_get_mesh_info", meta, st, false));
    info->n_faces = meta[META_N_FACES];
    info->n_vertices = meta[META_N_VERTICES];
    info->n_solid = st[ST_SOLID];
    for (int q = 0; q < 6; ++q) info->faces_by_dir[q] = st[ST_DIR + q];
    for (int q = 0; q < 4; ++q) info->faces_by_kind[q] = st[ST_KIND + q];
    info->pad = 0u;
    info->options = m->mesh.opt;
  }
  layer_origin(m, m->mesh, origin);
  return SDM_OK;
}

sdm_status sdm_get_mesh_faces(sdm_map *m, sdm_mesh_face *faces, uint32_t *quads, int64_t cap, int64_t *n_out) {
  const char *what = "sdm_get_mesh_faces";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out) return LAYER_REFUSE(what, "cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->mesh, MESH));
  uint32_t meta[META_WORDS], st[ST_WORDS];
  SDM_TRY(mesh_meta(m, what, meta, st, true));
  *n_out = (int64_t)meta[META_N_FACES];
  if (meta[META_OVER]) return SDM_ERR_CAPACITY;
  const size_t take = (size_t)std::min<int64_t>((int64_t)meta[META_N_FACES], cap);
  if (take && (faces || quads)) {
    if (faces) HIP_TRY(hipMemcpyAsync(faces, m->mesh.faces, take * sizeof(sdm_mesh_face), hipMemcpyDeviceToHost, m->stream));
    if (quads) HIP_TRY(hipMemcpyAsync(quads, m->mesh.quads, take * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return SDM_OK;
}

sdm_status sdm_get_mesh_vertices(sdm_map *m, sdm_mesh_vertex *corners, float *xyz, int64_t cap, int64_t *n_out) {
  const char *what = "sdm_get_mesh_vertices";
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out) return LAYER_REFUSE(what, "cap < 0 or no n_out");
  SDM_TRY(layer_check(m, what, &m->mesh, MESH));
  uint32_t meta[META_WORDS], st[ST_WORDS];
  SDM_TRY(mesh_meta(m, what, meta, st, true));
  *n_out = (int64_t)meta[META_N_VERTICES];
  if (meta[META_OVER]) return SDM_ERR_CAPACITY;
  const size_t take = (size_t)std::min<int64_t>((int64_t)meta[META_N_VERTICES], cap);
  if (take && (corners || xyz)) {
    std::vector<sdm_mesh_vertex> own;
    if (!corners) {
      own.resize(take);
      corners = own.data();
    }
    HIP_TRY(hipMemcpyAsync(corners, m->mesh.verts, take * sizeof(sdm_mesh_vertex), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (xyz) {
      float origin[3];
      layer_origin(m, m->mesh, origin);
      const float size = m->d.voxel_size;
      for (size_t v = 0; v < take; ++v) {
        const uint16_t c[3] = {corners[v].i, corners[v].j, corners[v].k};
        for (int a = 0; a < 3; ++a) {
          const float step = (float)c[a] * size;  // (one IEEE operation at a time)
          xyz[3 * v + a] = origin[a] + step;
        }
      }
    }
  }
  return SDM_OK;
}

sdm_status sdm_mesh_device(sdm_map *m, const sdm_mesh_face **faces, const uint32_t **quads, const sdm_mesh_vertex **corners) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_mesh_device", &m->mesh, MESH));
  if (faces) *faces = m->mesh.faces;
  if (quads) *quads = m->mesh.quads;
  if (corners) *corners = m->mesh.verts;
  return SDM_OK;
}

}  // extern "C"
