// world_snapshot.hip — the kernels and host helpers the builds over the world archive share (gfx950).  A
// build is a snapshot: it flags the items of its field, ranks the flags, waits once for their number and indexes the field
// by rank; the two route planners then turn activity bits into a list a round.
//   k_ws_flag    a thread per archived brick in brick order: 1 if it lies in the box (or there is none); the entry behind
//             the last brick is 0, where the scan leaves the number of flags.
//   exclusive_scan_u32   ranks the flags (snapshot_rank: every build's, whatever kernel wrote its flags).
//   k_ws_index   a thread per archived brick: a flagged one writes its coordinates at its rank, its pool slot beside them if
//             the caller keeps it, and inserts key -> rank into the caller's table (every key by one thread, like
//             world_insert).
//   k_ws_neighbours  a thread per (brick of the field, one of 27): one lookup in the caller's own table, the neighbour's rank
//             or NONE (anything >= n); brick_in_range before every lookup.  World reach's and world objects' (DESIGN.md 5w).
//   k_ws_list    a thread per word of activity bits: clears it and appends its items to the list, counted where the caller
//             says.
#include "sdm_world.h"

namespace sdm {

namespace {

constexpr int QT = 256;

__global__ __launch_bounds__(QT) void k_ws_flag(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr, uint32_t n_arch, BrickBox box,
                                                uint32_t *__restrict__ flag) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j > n_arch) return;
  uint32_t in = 0u;
  if (j < n_arch) {  // (the entry behind the last brick: the scan leaves the number of flags there)
    const uint32_t slot = order[j];
    int b[3];
    brick_of(hdr[(size_t)slot * HDR_WORDS], hdr[(size_t)slot * HDR_WORDS + 1], b[0], b[1], b[2]);
    in = 1u;
    if (box.use)
      for (int a = 0; a < 3; ++a) in = in && b[a] >= box.lo[a] && b[a] <= box.hi[a] ? 1u : 0u;
  }
  flag[j] = in;
}

__global__ __launch_bounds__(QT) void k_ws_index(const uint32_t *__restrict__ order, const uint32_t *__restrict__ hdr,
                                                 const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint32_t n_arch, uint32_t n,
                                                 uint32_t *__restrict__ coord, uint32_t *__restrict__ slot_of, u64 *__restrict__ keys,
                                                 uint32_t *__restrict__ vals, uint32_t hmask) {
  const uint32_t j = blockIdx.x * QT + threadIdx.x;
  if (j >= n_arch || !flag[j]) return;
  const uint32_t slot = order[j], r = rank[j];
  if (r >= n) return;  // (never: the scan's total is n)
  const uint32_t h0 = hdr[(size_t)slot * HDR_WORDS], h1 = hdr[(size_t)slot * HDR_WORDS + 1] & 0xffffu;
  coord[2 * (size_t)r] = h0;
  coord[2 * (size_t)r + 1] = h1;
  if (slot_of) slot_of[r] = slot;
  int bx, by, bz;
  brick_of(h0, h1, bx, by, bz);
  world_insert(keys, vals, hmask, brick_key(bx, by, bz), r);
}

__global__ __launch_bounds__(QT) void k_ws_neighbours(const uint32_t *__restrict__ coord, const u64 *__restrict__ keys,
                                                      const uint32_t *__restrict__ vals, uint32_t hmask, uint32_t n, uint32_t *__restrict__ nbr) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= n * 27u) return;
  const uint32_t r = i / 27u, k = i - r * 27u;
  int bx, by, bz;
  coord_of(coord, r, bx, by, bz);
  bx += off_d((int)k, 0), by += off_d((int)k, 1), bz += off_d((int)k, 2);
  // (a coordinate of 32768 would alias another brick's key; k == 13 finds the brick's own rank, which k_ws_index inserted)
  const uint32_t nr = brick_in_range(bx, by, bz) ? world_find(keys, vals, hmask, brick_key(bx, by, bz)) : NONE;
  nbr[i] = nr < n ? nr : NONE;
}

__global__ __launch_bounds__(QT) void k_ws_list(uint32_t *__restrict__ act, uint32_t *__restrict__ list, uint32_t *__restrict__ count, uint32_t n) {
  const uint32_t i = blockIdx.x * QT + threadIdx.x;
  if (i >= (n + 31u) / 32u) return;
  uint32_t w = act[i];
  if (!w) return;
  act[i] = 0u;
  uint32_t at = atomicAdd(count, (uint32_t)__popc(w));  // (<= n in all: an item has one bit)
  while (w) {
    const uint32_t t = i * 32u + (uint32_t)__builtin_ctz(w);
    if (at < n && t < n) list[at] = t;  // (always: the bits beyond n are never set)
    ++at;
    w &= w - 1u;
  }
}

}  // namespace

sdm_status snapshot_rank(sdm_map *m, const uint32_t *flag, uint32_t *rank, size_t items, uint32_t *scan, void *landing, uint32_t *n) {
  exclusive_scan_u32(flag, rank, items + 1, scan, m->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(landing, rank + items, sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));  // the one wait: the count sizes the buffers
  std::memcpy(n, landing, sizeof(uint32_t));
  return SDM_OK;
}

sdm_status snapshot_flag_bricks(sdm_map *m, const uint32_t *order, uint32_t n_arch, const BrickBox &box, uint32_t *flag, uint32_t *rank,
                                uint32_t *scan, void *landing, uint32_t *n) {
  hipLaunchKernelGGL(k_ws_flag, dim3(n_arch / QT + 1), dim3(QT), 0, m->stream, order, m->world.hdr, n_arch, box, flag);
  HIP_TRY(hipGetLastError());
  return snapshot_rank(m, flag, rank, n_arch, scan, landing, n);
}

hipError_t launch_snapshot_index(const sdm_map *m, const uint32_t *order, const uint32_t *flag, const uint32_t *rank, uint32_t n_arch, uint32_t n,
                                 uint32_t *coord, uint32_t *slot_of, u64 *keys, uint32_t *vals, uint32_t hmask) {
  LAYER_LAUNCH(k_ws_index, (n_arch + QT - 1) / QT, QT, m->stream, order, m->world.hdr, flag, rank, n_arch, n, coord, slot_of, keys, vals, hmask);
  return hipSuccess;
}

hipError_t launch_snapshot_neighbours(const uint32_t *coord, const u64 *keys, const uint32_t *vals, uint32_t hmask, uint32_t n, uint32_t *nbr,
                                      hipStream_t s) {
  LAYER_LAUNCH(k_ws_neighbours, (n * 27u + QT - 1) / QT, QT, s, coord, keys, vals, hmask, n, nbr);
  return hipSuccess;
}

hipError_t launch_snapshot_list(uint32_t *act, uint32_t *list, uint32_t *count, uint32_t n, hipStream_t s) {
  LAYER_LAUNCH(k_ws_list, ((n + 31u) / 32u + QT - 1) / QT, QT, s, act, list, count, n);
  return hipSuccess;
}

}  // namespace sdm
