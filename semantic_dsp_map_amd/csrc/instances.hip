// instances.hip — the map's instance table: per winning track id its counted cells, box, first cell, label and moments
// (gfx950; include/sdm.h, "instance table").
//
// One streaming pass over State::res in map-index order and one small kernel behind it.  Everything accumulated is an
// integer sum or an integer maximum, so the table does not depend on the order in which cells arrive:
//   sums      n_cells, n_guessed (u32); sum of x y z, of xx yy zz xy xz yz (u64)
//   maxima    every minimum as the maximum of its complement (~min x y z, ~min label, ~(first_cell << 8 | label)), the
//             maxima themselves (x y z, label) and wsum through an order-preserving integer image of the float
// so an accumulator that is all zero is "no cell yet", and emptying one is storing zeros.
//   k_instances_accumulate  <= IA_GRID workgroups of 16 waves, each a contiguous run of chunks of 64 cells; a wave loads
//               the IA_U chunks of its next step before it works on the current ones.  A chunk without a counted cell is
//               one ballot.  Where an x row holds whole chunks (x_n >= 6) a step of the workgroup (4096 cells) is whole
//               rows, and a wave takes its IA_U chunks of a step from IA_U rows at the same x: a lane walks down ONE x
//               column of the map, and y and z are wave-uniform.  The lane keeps that column's cells of its current
//               track in registers (LaneAcc, 16 words; a cell costs some twenty VALU operations with scalar operands
//               and nothing crosses lanes); x enters only when the registers are turned into sums.  A
//               lane that meets another track sends what it holds to the workgroup's LDS table - IA_SLOTS accumulators
//               keyed by track, open addressing - and starts over.  At the end of its run the wave reduces what its
//               lanes still hold, per distinct track, with shuffles and sends one set of values per track (up to IA_FEW lanes
//               send theirs themselves).
//               Rows shorter than a wave (x_n < 6: small maps only) take the plain way: every counted lane sends its
//               own cell to the LDS table.
//               Then the workgroup sends each used slot to the global accumulators, one set of atomics per
//               (workgroup, track), and sets the track's bit.  The global accumulators are field-major (field f of track t
//               at [f][t]): one or two tracks own most cells of a real map and every workgroup flushes them; field-major,
//               the 21 values of a track sit on 21 cache lines that each see one atomic per workgroup.
//               A track that finds the LDS table full goes to the global accumulators directly (correct, slower).
//   k_instances_finalize    one workgroup: scans the 65536 track bits (8 KB), gives every set bit its rank (ascending
//               track id), and one thread per instance reads its accumulators, writes the sdm_instance and stores zeros
//               back, so the next build starts from empty accumulators.  Also moves the 256 label counters.
#include "sdm_layer.h"
#include "sdm_map.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_instance) == 144, "sdm.h layout");
static_assert(offsetof(sdm_instance, cell_sum) == 32 && offsetof(sdm_instance, box_min) == 104 && offsetof(sdm_instance, pad) == 140, "sdm.h layout");

namespace sdm {

namespace {

constexpr int IA_TPB = 1024, IA_WAVES = IA_TPB / 64;
constexpr int IA_U = 4;          // chunks a wave loads together
constexpr int IA_GRID = 256;     // workgroups at most: every one of them flushes the map's dominant tracks
constexpr int IA_SLOTS = 64;     // LDS accumulators per workgroup
constexpr int IA_FEW = 4;        // at the end of a run: up to this many lanes of a wave send a track's cells themselves
constexpr uint32_t N_TRACKS = 65536;
constexpr LayerName INSTANCES = {"the instance table", "instance table", "sdm_instances_update", false};
static_assert((IA_WAVES * IA_U * 64) % 512 == 0, "a step of a workgroup is whole x rows (x_n <= 9)");
// fields of an accumulator: A64 64-bit ones (0..8 sums, 9 the first-cell maximum), A32 32-bit ones (0..1 sums, 2..10 maxima)
constexpr int A64 = 10, A32 = 11;
enum { S_X = 0, S_Y, S_Z, S_XX, S_YY, S_ZZ, S_XY, S_XZ, S_YZ, M_FIRST };
enum { C_N = 0, C_GUESSED, M_NMINX, M_NMINY, M_NMINZ, M_MAXX, M_MAXY, M_MAXZ, M_NLMIN, M_LMAX, M_WSUM };
constexpr size_t ACC64_WORDS = (size_t)A64 * N_TRACKS, ACC32_WORDS = (size_t)A32 * N_TRACKS;
constexpr size_t ACC_BYTES = ACC64_WORDS * 8 + ACC32_WORDS * 4 + (N_TRACKS / 32) * 4 + 256 * 4;

struct Acc {  // the global accumulators (one allocation, sdm_map::inst.acc)
  unsigned long long *a64;  // [A64][N_TRACKS]
  uint32_t *a32;            // [A32][N_TRACKS]
  uint32_t *bits;           // [N_TRACKS / 32]: tracks with cells
  uint32_t *labels;         // [256]
};

// what a lane holds of one x column and one track (k_instances_accumulate, x_n >= 6); all zero = nothing.  A lane sees at
// most 512 cells in a run, so 32 bits hold every sum.
struct LaneAcc {
  uint32_t t, n, ng, sy, sz, syy, szz, syz, nminy, maxy, nminz, maxz;
  uint32_t nfirst;  // max of ~(row << 8 | label), row = cell word >> x_n
  uint32_t nlmin, lmax, wmax;
};

__device__ __forceinline__ bool counted_cell(uint32_t w1, uint32_t flags, int max_movable) {
  const int occ = (int8_t)(w1 >> 24);  // (not occ_of: the kernels' registers stay as they were)
  const int track = (int)(w1 & 0xffffu);
  if (occ < 1) return false;
  if ((flags & SDM_INSTANCES_OBSERVED_ONLY) && occ != 1) return false;
  if ((flags & SDM_INSTANCES_MOVABLE_ONLY) && !(track >= 1 && track <= max_movable)) return false;
  return true;
}

// order-preserving image of a float: a < b as floats  <=>  image(a) < image(b) as unsigned
__device__ __forceinline__ uint32_t float_image(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ uint32_t float_image_inv(uint32_t im) { return (im & 0x80000000u) ? (im & 0x7fffffffu) : ~im; }

// the slot of track t in the workgroup's table (claimed if new); -1: the table is full
__device__ __forceinline__ int find_slot(uint32_t *keys, uint32_t t) {
  const uint32_t h = (t * 2654435761u) >> 26;
  for (int p = 0; p < IA_SLOTS; ++p) {
    const uint32_t s = (h + (uint32_t)p) & (IA_SLOTS - 1);
    uint32_t k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == 0u) {
      k = atomicCAS(keys + s, 0u, t + 1u);
      if (k == 0u) k = t + 1u;
    }
    if (k == t + 1u) return (int)s;
  }
  return -1;
}

// lane l < 21 adds / maximises its value: lanes 0..9 the 64-bit fields, 10..20 the 32-bit ones.  stride: words between fields.
template <typename P64, typename P32>
__device__ __forceinline__ void send_lanes(uint32_t lane, P64 p64, P32 p32, size_t stride, unsigned long long v64, uint32_t v32) {
  if (lane < (uint32_t)M_FIRST) {
    if (v64) atomicAdd(p64 + lane * stride, v64);
  } else if (lane == (uint32_t)M_FIRST) {
    atomicMax(p64 + lane * stride, v64);
  } else if (lane < (uint32_t)(A64 + M_NMINX)) {
    if (v32) atomicAdd(p32 + (lane - A64) * stride, v32);
  } else if (lane < (uint32_t)(A64 + A32)) {
    atomicMax(p32 + (lane - A64) * stride, v32);
  }
}

// all 21 values from one lane
template <typename P64, typename P32>
__device__ __forceinline__ void send_all(P64 p64, P32 p32, size_t stride, const unsigned long long (&a)[A64], const uint32_t (&b)[A32]) {
#pragma unroll
  for (int i = 0; i < M_FIRST; ++i)
    if (a[i]) atomicAdd(p64 + i * stride, a[i]);
  atomicMax(p64 + M_FIRST * stride, a[M_FIRST]);
#pragma unroll
  for (int i = 0; i < M_NMINX; ++i)
    if (b[i]) atomicAdd(p32 + i * stride, b[i]);
#pragma unroll
  for (int i = M_NMINX; i < A32; ++i) atomicMax(p32 + i * stride, b[i]);
}

// ... to track t's slot of the workgroup's table, or, if the table is full, to the global accumulators
__device__ __forceinline__ void send_track(unsigned long long *tab, uint32_t *keys, const Acc &g, uint32_t t, const unsigned long long (&a)[A64],
                                           const uint32_t (&b)[A32]) {
  const int slot = find_slot(keys, t);
  if (slot >= 0) {
    send_all(tab + slot * 16, reinterpret_cast<uint32_t *>(tab + slot * 16 + A64), 1, a, b);
  } else {
    send_all(g.a64 + t, g.a32 + t, N_TRACKS, a, b);
    atomicOr(g.bits + (t >> 5), 1u << (t & 31u));
  }
}

// what a lane holds of column x as the 21 accumulator values (s.n > 0)
__device__ __forceinline__ void lane_values(const LaneAcc &s, uint32_t x, int x_n, unsigned long long (&a)[A64], uint32_t (&b)[A32]) {
  const unsigned long long n = s.n, X = x;
  a[S_X] = n * X;
  a[S_Y] = s.sy;
  a[S_Z] = s.sz;
  a[S_XX] = n * X * X;
  a[S_YY] = s.syy;
  a[S_ZZ] = s.szz;
  a[S_XY] = X * s.sy;
  a[S_XZ] = X * s.sz;
  a[S_YZ] = s.syz;
  const uint32_t key = ~s.nfirst;
  a[M_FIRST] = ~((((((unsigned long long)(key >> 8)) << x_n) | X) << 8) | (key & 0xffu));
  b[C_N] = s.n;
  b[C_GUESSED] = s.ng;
  b[M_NMINX] = ~x;
  b[M_NMINY] = s.nminy;
  b[M_NMINZ] = s.nminz;
  b[M_MAXX] = x;
  b[M_MAXY] = s.maxy;
  b[M_MAXZ] = s.maxz;
  b[M_NLMIN] = s.nlmin;
  b[M_LMAX] = s.lmax;
  b[M_WSUM] = s.wmax;
}

template <bool WIDE>
__global__ __launch_bounds__(IA_TPB) void k_instances_accumulate(Dims d, Frame f, const uint2 *__restrict__ res, uint32_t flags,
                                                                uint32_t n_chunks, uint32_t steps, Acc g) {
  __shared__ unsigned long long tab[IA_SLOTS * 16];  // 128 bytes a slot: A64 64-bit fields, then A32 32-bit ones
  __shared__ uint32_t keys[IA_SLOTS];                // track + 1, 0 = free
  __shared__ uint32_t lab[256];
  for (uint32_t i = threadIdx.x; i < IA_SLOTS * 16; i += IA_TPB) tab[i] = 0ull;
  if (threadIdx.x < IA_SLOTS) keys[threadIdx.x] = 0u;
  if (threadIdx.x < 256) lab[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t xy_n = (uint32_t)(d.x_n + d.y_n);
  // Chunk u of this wave in step `step`.  A step of the workgroup is 64 consecutive chunks.  x_n >= 6: whole x rows, of
  // which the wave takes IA_U at the same x (so its lanes stay in their columns); else the wave's IA_U chunks in a row.
  const uint32_t cpr_n = WIDE ? (uint32_t)d.x_n - 6u : 0u;  // log2 chunks per x row
  auto chunk_of = [&](uint32_t step, int u) {
    const uint32_t base = (blockIdx.x * steps + step) * (IA_WAVES * IA_U);
    if (WIDE) return base + ((((wave >> cpr_n) * IA_U + (uint32_t)u) << cpr_n) | (wave & ((1u << cpr_n) - 1u)));
    return base + wave * IA_U + (uint32_t)u;
  };

  // the result words of the IA_U chunks of step `step` of this wave; 0 (free, not counted) beyond the map
  auto load = [&](uint32_t step, uint2 (&w)[IA_U]) {
#pragma unroll
    for (int u = 0; u < IA_U; ++u) {
      const uint32_t chunk = chunk_of(step, u);
      w[u] = make_uint2(0u, 0u);
      if (chunk >= n_chunks) continue;
      const uint32_t c0 = chunk << 6;
      if (WIDE) {
        const uint32_t x = (c0 & (d.NX - 1)) + lane, y = (c0 >> d.x_n) & (d.NY - 1), z = c0 >> xy_n;
        const uint32_t ry = axis_correct((int)y + f.eq[1], d.NY), rz = axis_correct((int)z + f.eq[2], d.NZ);
        w[u] = res[ring_to_voxel(d, axis_correct((int)x + f.eq[0], d.NX), ry, rz)];
      } else {
        const uint32_t c = c0 + lane;
        if (c < d.V) {
          w[u] = res[word_voxel(d, f, c)];
        }
      }
    }
  };

  LaneAcc s = {};
  const uint32_t column = ((wave & ((1u << cpr_n) - 1u)) << 6) + lane;  // the x of this lane's cells, in every step

  auto work = [&](uint32_t c0, const uint2 &w) {
    const uint32_t track = w.y & 0xffffu, label = (w.y >> 16) & 0xffu;
    const bool counted = counted_cell(w.y, flags, d.max_movable);
    if (!__ballot(counted)) return;
    if (!counted) return;
    const uint32_t guessed = occ_of(w.y) == 2 ? 1u : 0u;
    const uint32_t wim = float_image(w.x);
    atomicAdd(lab + label, 1u);
    if (WIDE) {
      if (s.n && s.t != track) {  // another track in this column: what the lane holds goes to the table
        unsigned long long a[A64];
        uint32_t b[A32];
        lane_values(s, column, d.x_n, a, b);
        send_track(tab, keys, g, s.t, a, b);
        s = LaneAcc{};
      }
      const uint32_t row = c0 >> d.x_n, y = row & (d.NY - 1), z = c0 >> xy_n;  // (wave-uniform)
      s.t = track;
      s.n += 1u;
      s.ng += guessed;
      s.sy += y;
      s.sz += z;
      s.syy += y * y;
      s.szz += z * z;
      s.syz += y * z;
      s.nminy = max(s.nminy, ~y);
      s.maxy = max(s.maxy, y);
      s.nminz = max(s.nminz, ~z);
      s.maxz = max(s.maxz, z);
      s.nfirst = max(s.nfirst, ~((row << 8) | label));
      s.nlmin = max(s.nlmin, ~label);
      s.lmax = max(s.lmax, label);
      s.wmax = max(s.wmax, wim);
    } else {
      const uint32_t c = c0 + lane;
      unsigned long long x, y, z;
      cell_xyz(d, c, x, y, z);
      const unsigned long long a[A64] = {x, y, z, x * x, y * y, z * z, x * y, x * z, y * z, ~(((unsigned long long)c << 8) | label)};
      const uint32_t b[A32] = {1u, guessed, ~(uint32_t)x, ~(uint32_t)y, ~(uint32_t)z, (uint32_t)x, (uint32_t)y, (uint32_t)z, ~label, label, wim};
      send_track(tab, keys, g, track, a, b);
    }
  };

  uint2 cur[IA_U], nxt[IA_U];
  load(0, cur);
  for (uint32_t step = 0; step < steps; ++step) {
#pragma unroll
    for (int u = 0; u < IA_U; ++u) nxt[u] = make_uint2(0u, 0u);
    if (step + 1 < steps) load(step + 1, nxt);  // the next step's loads are out before this step's work
#pragma unroll
    for (int u = 0; u < IA_U; ++u) work(chunk_of(step, u) << 6, cur[u]);
#pragma unroll
    for (int u = 0; u < IA_U; ++u) cur[u] = nxt[u];
  }
  if (WIDE) {
    // what the lanes still hold: per distinct track one reduction across the wave (every lane ends with the totals),
    // one lane sends them; a track that only a few lanes hold is sent by those lanes themselves
    bool alive = s.n != 0u;
    for (;;) {
      const unsigned long long m = __ballot(alive);
      if (!m) break;
      const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)s.t, __builtin_ctzll(m));
      const bool mine = alive && s.t == t;
      alive = alive && !mine;
      unsigned long long A[A64] = {};
      uint32_t B[A32] = {};
      if (mine) lane_values(s, column, d.x_n, A, B);
      const bool few = __popcll(__ballot(mine)) <= IA_FEW;  // (wave-uniform)
#pragma unroll
      for (int o = 32; o >= 1 && !few; o >>= 1) {
#pragma unroll
        for (int i = 0; i < M_FIRST; ++i) A[i] += __shfl_xor(A[i], o, 64);
        A[M_FIRST] = max(A[M_FIRST], (unsigned long long)__shfl_xor(A[M_FIRST], o, 64));
#pragma unroll
        for (int i = 0; i < M_NMINX; ++i) B[i] += (uint32_t)__shfl_xor((int)B[i], o, 64);
#pragma unroll
        for (int i = M_NMINX; i < A32; ++i) B[i] = max(B[i], (uint32_t)__shfl_xor((int)B[i], o, 64));
      }
      if (few ? mine : lane == 0) send_track(tab, keys, g, t, A, B);
    }
  }
  __syncthreads();
  // the workgroup's table goes to the global accumulators: a wave per slot, a lane per field
  for (uint32_t slot = wave; slot < IA_SLOTS; slot += IA_WAVES) {
    const uint32_t k = keys[slot];
    if (k == 0u) continue;
    const uint32_t t = k - 1u;
    const unsigned long long v64 = lane < (uint32_t)A64 ? tab[slot * 16 + lane] : 0ull;
    const uint32_t v32 = (lane >= (uint32_t)A64 && lane < (uint32_t)(A64 + A32)) ? reinterpret_cast<const uint32_t *>(tab + slot * 16 + A64)[lane - A64] : 0u;
    send_lanes(lane, g.a64 + t, g.a32 + t, N_TRACKS, v64, v32);
    if (lane == 63) atomicOr(g.bits + (t >> 5), 1u << (t & 31u));
  }
  if (threadIdx.x < 256 && lab[threadIdx.x]) atomicAdd(g.labels + threadIdx.x, lab[threadIdx.x]);
}

// ---- the table ---------------------------------------------------------------------------------------------------------
constexpr int IF_TPB = 1024;  // a thread per 64 track bits

__global__ __launch_bounds__(IF_TPB) void k_instances_finalize(Dims d, Frame f, Acc g, sdm_instance *__restrict__ out,
                                                              uint32_t *__restrict__ meta) {
  __shared__ uint32_t pre[IF_TPB];
  __shared__ unsigned long long words[IF_TPB];
  const uint32_t tid = threadIdx.x;
  const unsigned long long w = (unsigned long long)g.bits[2 * tid] | ((unsigned long long)g.bits[2 * tid + 1] << 32);
  words[tid] = w;
  const uint32_t cnt = (uint32_t)__popcll(w);
  pre[tid] = cnt;
  __syncthreads();
  for (uint32_t o = 1; o < IF_TPB; o <<= 1) {  // inclusive scan
    const uint32_t v = tid >= o ? pre[tid - o] : 0u;
    __syncthreads();
    pre[tid] += v;
    __syncthreads();
  }
  const uint32_t total = pre[IF_TPB - 1];
  if (w) {
    g.bits[2 * tid] = 0u;
    g.bits[2 * tid + 1] = 0u;
  }
  if (tid < 256) {
    meta[1 + tid] = g.labels[tid];
    g.labels[tid] = 0u;
  }
  if (tid == 0) meta[0] = total;
  for (uint32_t j = tid; j < total; j += IF_TPB) {
    // the thread whose 64 bits hold the j-th instance: the first one whose inclusive count exceeds j
    uint32_t lo = 0, hi = IF_TPB - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (pre[mid] > j) hi = mid; else lo = mid + 1;
    }
    const unsigned long long ww = words[lo];
    const uint32_t before = pre[lo] - (uint32_t)__popcll(ww);
    const uint32_t t = lo * 64u + (uint32_t)nth_set_bit(ww, j - before);
    unsigned long long a[A64];
    uint32_t b[A32];
#pragma unroll
    for (int i = 0; i < A64; ++i) a[i] = g.a64[(size_t)i * N_TRACKS + t];
#pragma unroll
    for (int i = 0; i < A32; ++i) b[i] = g.a32[(size_t)i * N_TRACKS + t];
#pragma unroll
    for (int i = 0; i < A64; ++i) g.a64[(size_t)i * N_TRACKS + t] = 0ull;
#pragma unroll
    for (int i = 0; i < A32; ++i) g.a32[(size_t)i * N_TRACKS + t] = 0u;
    sdm_instance e;
    const unsigned long long first = ~a[M_FIRST];
    e.track = (uint16_t)t;
    e.label = (uint8_t)(first & 0xffu);
    e.mixed_labels = (~b[M_NLMIN] & 0xffu) != b[M_LMAX] ? 1 : 0;
    e.n_cells = b[C_N];
    e.n_guessed = b[C_GUESSED];
    e.first_cell = (uint32_t)(first >> 8);
    e.wsum_max = __uint_as_float(float_image_inv(b[M_WSUM]));
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      const uint32_t cmin = ~b[M_NMINX + ax], cmax = b[M_MAXX + ax];
      e.cell_min[ax] = (uint16_t)cmin;
      e.cell_max[ax] = (uint16_t)cmax;
      e.cell_sum[ax] = a[S_X + ax];
      const float origin = f.center[ax] + d.pmin[ax];
      e.box_min[ax] = origin + (float)cmin * d.voxel_size;
      e.box_max[ax] = origin + (float)(cmax + 1u) * d.voxel_size;
      e.centroid[ax] = (float)((double)origin + ((double)a[S_X + ax] / (double)b[C_N] + 0.5) * (double)d.voxel_size);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) e.cell_sq[i] = a[S_XX + i];
    e.pad = 0u;
    out[j] = e;
  }
}

Acc acc_of(unsigned char *p) {
  Acc g;
  g.a64 = reinterpret_cast<unsigned long long *>(p);
  g.a32 = reinterpret_cast<uint32_t *>(p + ACC64_WORDS * 8);
  g.bits = g.a32 + ACC32_WORDS;
  g.labels = g.bits + N_TRACKS / 32;
  return g;
}

hipError_t launch_instances_build(const Dims &d, const Frame &f, const State &st, uint32_t flags, unsigned char *acc, sdm_instance *out,
                                  uint32_t *meta, hipStream_t s) {
  const Acc g = acc_of(acc);
  const uint32_t n_chunks = (d.V + 63u) >> 6;
  const uint32_t per_step = IA_WAVES * IA_U;  // chunks a workgroup takes in one step
  const uint32_t all_steps = (n_chunks + per_step - 1) / per_step;
  const uint32_t steps = (all_steps + IA_GRID - 1) / IA_GRID;  // per workgroup: a contiguous run of the map
  const uint32_t grid = (all_steps + steps - 1) / steps;
  const uint2 *res = reinterpret_cast<const uint2 *>(st.res);
  if (d.x_n >= 6)
    hipLaunchKernelGGL(k_instances_accumulate<true>, dim3(grid), dim3(IA_TPB), 0, s, d, f, res, flags, n_chunks, steps, g);
  else
    hipLaunchKernelGGL(k_instances_accumulate<false>, dim3(grid), dim3(IA_TPB), 0, s, d, f, res, flags, n_chunks, steps, g);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_instances_finalize, dim3(1), dim3(IF_TPB), 0, s, d, f, g, out, meta);
  return hipGetLastError();
}

}  // namespace

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
// Like the distance field, the build reads the result array in stream order and takes the host Frame of the last issued
// frame by value; the Frame stays with the table (sdm_get_instances' origin).
extern "C" {

sdm_status sdm_instances_update(sdm_map *m, uint32_t flags) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (flags & ~(SDM_INSTANCES_MOVABLE_ONLY | SDM_INSTANCES_OBSERVED_ONLY)) {
    set_error("sdm_instances_update", __FILE__, __LINE__, "unknown flag bits");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_instances_update", nullptr, INSTANCES));
  HIP_TRY(hipSetDevice(m->device));
  if (!m->inst.acc) {
    SDM_TRY(alloc_tracked(m, &m->inst.acc, ACC_BYTES));
    HIP_TRY(hipMemsetAsync(m->inst.acc, 0, ACC_BYTES, m->stream));  // empty; every build leaves them empty again
  }
  if (!m->inst.out) SDM_TRY(alloc_tracked(m, &m->inst.out, N_TRACKS));
  if (!m->inst.meta) SDM_TRY(alloc_tracked(m, &m->inst.meta, 257));
  const Frame f = m->f;
  HIP_TRY(launch_instances_build(m->d, f, m->st, flags, m->inst.acc, m->inst.out, m->inst.meta, m->stream));
  m->inst.built(f, flags);
  return SDM_OK;
}

sdm_status sdm_get_instances(sdm_map *m, sdm_instance *out, int32_t cap, int32_t *n_out, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out || (cap > 0 && !out)) {
    set_error("sdm_get_instances", __FILE__, __LINE__, "cap < 0, no n_out, or no out for cap > 0");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_get_instances", &m->inst, INSTANCES));
  HIP_TRY(hipSetDevice(m->device));
  uint32_t n = 0;
  HIP_TRY(hipMemcpyAsync(&n, m->inst.meta, sizeof(n), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  const size_t take = std::min<size_t>(n, (size_t)cap);
  if (take) {
    HIP_TRY(hipMemcpyAsync(out, m->inst.out, take * sizeof(sdm_instance), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  *n_out = (int32_t)n;
  layer_origin(m, m->inst, origin);
  return SDM_OK;
}

sdm_status sdm_get_label_cells(sdm_map *m, uint32_t out[256]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!out) {
    set_error("sdm_get_label_cells", __FILE__, __LINE__, "no out");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_get_label_cells", &m->inst, INSTANCES));
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(out, m->inst.meta + 1, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

}  // extern "C"
