// exchange.hip — multi-GPU: what a Z-slab sharded frame exchanges with the other shards, through RCCL or through
// peer-mapped memory (hipIpc), and sdm_update_sharded, the frame that does its exchanges itself.
#include <rccl/rccl.h>

#include <chrono>
#include <cstdlib>
#include <thread>

#include "sdm_map.h"

namespace {

// ---- exchanges of a sharded frame through peer-mapped memory ------------------------------------------------------
// xGMI is point to point: a shard can write into a peer's HBM directly, and what a sharded frame exchanges is small (a row
// of 64 counts, a few KB of records, 230 KB of partial sums per peer).  A collective library pays a launch, a handshake and
// a proxy round for each of them - 5-7 us with ONE rank on this part, 20 us for the count row on its side stream, and the
// frame has three to four on its critical path.  Here an exchange is one launch of `world` workgroups: workgroup p copies
// this shard's piece for shard p into p's arena (plain stores over the fabric), makes them visible (system-scope fence),
// raises this shard's flag in p's arena to the exchange's sequence number, and waits until p's flag in its OWN arena
// carries that number - then p's piece for this shard has landed.  The kernels behind it on the stream read what arrived.
// No host call but the launch, nothing to hand-shake: the lock step of the frames orders the buffers' reuse (a peer can
// only be one exchange ahead, and every arena region is written by one exchange kind only).
// The wait is bounded (SDM_COMM_TIMEOUT_MS): a shard that is missing leaves an error word, not a hung GPU.
constexpr int IPC_MAX_SHARDS = 16;
constexpr uint32_t IPC_FLAG_STRIDE = 128;  // bytes between two flags: a line each
enum { IPC_COUNTS = 0, IPC_HALO = 1, IPC_CK_PARTS = 2, IPC_CK_FULL = 3, IPC_KINDS = 4 };
constexpr size_t IPC_OFF_ERR = (size_t)IPC_KINDS * IPC_MAX_SHARDS * IPC_FLAG_STRIDE;
constexpr size_t IPC_OFF_DATA = IPC_OFF_ERR + 256;
struct IpcXchg {
  unsigned char *arena[IPC_MAX_SHARDS];
  int world, rank;
  uint32_t kind, seq;
  const unsigned char *src;  // the piece for shard p: src + p * src_stride
  size_t src_stride;
  size_t dst_off, dst_stride;  // it lands at p's arena + dst_off + rank * dst_stride
  uint32_t piece_bytes;        // a multiple of 4
  uint32_t halo_cap;           // != 0: the piece is an export segment - its header and the records it counts travel, not its capacity
  int copy_own;                // the piece for this shard itself is copied too (all-gather kinds)
  unsigned long long timeout_ticks;  // of the 100 MHz wall clock
  // != nullptr: what arrived from shard p is copied on into ordinary device memory, local + p * dst_stride.  The arena is
  // fine-grained memory - peers write it while this GPU reads it, so it is not cached - and a kernel that reads a piece
  // many times (the count rows in k_move_apply) wants it cached.
  unsigned char *local;
};
__device__ __forceinline__ void ipc_copy(unsigned char *dst, const unsigned char *src, uint32_t n, uint32_t t, uint32_t nt) {
  if (((uintptr_t)src | (uintptr_t)dst) % 16 == 0) {
    const uint4 *s16 = reinterpret_cast<const uint4 *>(src);
    uint4 *d16 = reinterpret_cast<uint4 *>(dst);
    for (uint32_t i = t; i < n / 16; i += nt) d16[i] = s16[i];
    for (uint32_t i = (n / 16) * 4 + t; i < n / 4; i += nt) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
  } else {
    for (uint32_t i = t; i < n / 4; i += nt) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
  }
}
// wait until *flag has reached seq (a peer's release store); false: timed out
__device__ __forceinline__ bool ipc_wait(const uint32_t *flag, uint32_t seq, unsigned long long timeout_ticks) {
  const unsigned long long t0 = wall_clock64();
  for (;;) {
    const uint32_t v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
    if ((int32_t)(v - seq) >= 0) return true;
    if (wall_clock64() - t0 > timeout_ticks) return false;
    __builtin_amdgcn_s_sleep(32);
  }
}
__device__ __forceinline__ uint32_t *ipc_flag(unsigned char *arena, uint32_t kind, int shard) {
  return reinterpret_cast<uint32_t *>(arena + ((size_t)kind * IPC_MAX_SHARDS + shard) * IPC_FLAG_STRIDE);
}
__global__ __launch_bounds__(1024) void k_ipc_exchange(const IpcXchg a) {
  const int p = blockIdx.x;
  const unsigned char *src = a.src + (size_t)p * a.src_stride;
  unsigned char *dst = a.arena[p] + a.dst_off + (size_t)a.rank * a.dst_stride;
  uint32_t n = a.piece_bytes;
  if (a.halo_cap) {
    uint32_t c = *reinterpret_cast<const uint32_t *>(src);
    c = c < a.halo_cap ? c : a.halo_cap;
    n = sdm::HALO_HEADER_BYTES + c * sdm::HALO_RECORD_BYTES;
  }
  if (dst != src && (p != a.rank || a.copy_own)) ipc_copy(dst, src, n, threadIdx.x, blockDim.x);
  // The workgroup's stores are ordered before the flag by the barrier and ONE system-scope release (thread 0's store below).
  // (A __threadfence_system() in every thread is a write-back of the whole L2 per wave: the first version of k_ipc_ck spent
  // 40 of its 49 us in them.)
  __syncthreads();
  __shared__ int ok;
  if (threadIdx.x == 0) {
    __hip_atomic_store(ipc_flag(a.arena[p], a.kind, a.rank), a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    ok = ipc_wait(ipc_flag(a.arena[a.rank], a.kind, p), a.seq, a.timeout_ticks) ? 1 : 0;
    if (!ok) *reinterpret_cast<uint32_t *>(a.arena[a.rank] + IPC_OFF_ERR) = a.kind + 1u;
  }
  __syncthreads();
  if (a.local && ok)
    ipc_copy(a.local + (size_t)p * a.dst_stride, a.arena[a.rank] + a.dst_off + (size_t)p * a.dst_stride, a.piece_bytes, threadIdx.x, blockDim.x);
}

// The whole exchange of the partial ck images in ONE launch (chunk-owner reduction): the parts of every
// shard's chunk go to its owner, the owner adds them in slab order - the float sums a single map split into the same slabs
// forms - and the summed chunk goes to every shard.  With a collective library that is all-to-all, a kernel, all-gather:
// three launches and two hand-shakes on the frame's critical path.  Here: `world` x split workgroups,
//   A  workgroup (p, q) writes share q of this shard's part of chunk p into p's arena; the last of p's workgroups raises the flag;
//   B  it waits for p's flag in the own arena; a barrier over the launch's workgroups: all parts of the own chunk are here;
//   C  the own chunk is summed (every workgroup a stretch of it) and written into every peer's arena and the local image;
//      barrier; the flags of the second round go up;
//   D  workgroup (p, q) waits for p's second flag and copies share q of p's summed chunk from the arena (uncached) into
//      the local image (ordinary device memory), which the weight update reads.
// The launch's workgroups are resident together (64 of them), so the barrier is an atomic counter.
struct IpcCk {
  int split;           // workgroups per peer: 64 / world of them, at least 4 (one shard alone sums the whole image: 64 workgroups)
  unsigned char *arena[IPC_MAX_SHARDS];
  int world, rank;
  uint32_t seq;        // of kind IPC_CK_PARTS; the second round's flags are kind IPC_CK_FULL with the same number
  uint32_t chunk;      // floats per chunk
  size_t off_stage, off_full;
  const float *part;   // this shard's partial image, world chunks
  float *local_full;   // the summed image, world chunks (ordinary device memory)
  uint32_t *sync;      // [0..15] arrivals per peer (round A), [16] / [17] barrier counters (never reset: they count launches)
  unsigned long long timeout_ticks;
};
__device__ __forceinline__ void ipc_grid_barrier(uint32_t *counter, uint32_t target, unsigned long long timeout_ticks, bool system_release) {
  __syncthreads();
  if (threadIdx.x == 0) {
    if (system_release) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // the workgroup's stores into the peers' arenas, before anybody raises a flag
    __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = wall_clock64();
    while ((int32_t)(__hip_atomic_load(counter, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
      if (wall_clock64() - t0 > timeout_ticks) break;
      __builtin_amdgcn_s_sleep(8);
    }
  }
  __syncthreads();
}
__global__ __launch_bounds__(1024) void k_ipc_ck(const IpcCk a) {
  const int SPLIT = a.split;
  const int p = blockIdx.x / SPLIT, q = blockIdx.x % SPLIT;
  const uint32_t nb = gridDim.x, C = a.chunk;
  const uint32_t share = (C / SPLIT + 3) / 4 * 4;  // floats per share (whole 16-byte pieces; the last share takes the rest)
  const uint32_t s0 = q * share < C ? q * share : C, s1 = (q + 1 == SPLIT || (q + 1) * share > C) ? C : (q + 1) * share;
  unsigned char *mine = a.arena[a.rank];
  __shared__ int ok;
  // ---- A: this shard's part of chunk p -> shard p
  if (p != a.rank)
    ipc_copy(a.arena[p] + a.off_stage + ((size_t)a.rank * C + s0) * 4, reinterpret_cast<const unsigned char *>(a.part + (size_t)p * C + s0),
             (s1 - s0) * 4, threadIdx.x, blockDim.x);
  __syncthreads();
  if (threadIdx.x == 0) {
    ok = 1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (system scope: this workgroup's share, before the arrival count and the flag)
    const uint32_t arrived = __hip_atomic_fetch_add(a.sync + p, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived % (uint32_t)SPLIT == (uint32_t)SPLIT - 1u)  // the last of p's workgroups: every share is on its way
      __hip_atomic_store(ipc_flag(a.arena[p], IPC_CK_PARTS, a.rank), a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    // ---- B: shard p's part of the own chunk
    if (!ipc_wait(ipc_flag(mine, IPC_CK_PARTS, p), a.seq, a.timeout_ticks)) {
      *reinterpret_cast<uint32_t *>(mine + IPC_OFF_ERR) = IPC_CK_PARTS + 1u;
      ok = 0;
    }
  }
  ipc_grid_barrier(a.sync + 16, a.seq * nb, a.timeout_ticks, false);
  // ---- C: the own chunk, summed in slab order, to everybody
  {
    const float *stage = reinterpret_cast<const float *>(mine + a.off_stage);
    const float *own = a.part + (size_t)a.rank * C;
    float *lf = a.local_full + (size_t)a.rank * C;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < C; i += nb * blockDim.x) {
      float ck = 0.f;
      for (int g = 0; g < a.world; ++g) ck += g == a.rank ? own[i] : stage[(size_t)g * C + i];
      lf[i] = ck;
      for (int g = 0; g < a.world; ++g)
        if (g != a.rank) reinterpret_cast<float *>(a.arena[g] + a.off_full)[(size_t)a.rank * C + i] = ck;
    }
  }
  ipc_grid_barrier(a.sync + 17, a.seq * nb, a.timeout_ticks, true);
  if (threadIdx.x == 0) {
    if (q == 0) __hip_atomic_store(ipc_flag(a.arena[p], IPC_CK_FULL, a.rank), a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    // ---- D: shard p's summed chunk
    if (!ipc_wait(ipc_flag(mine, IPC_CK_FULL, p), a.seq, a.timeout_ticks)) {
      *reinterpret_cast<uint32_t *>(mine + IPC_OFF_ERR) = IPC_CK_FULL + 1u;
      ok = 0;
    }
  }
  __syncthreads();
  if (p != a.rank && ok)
    ipc_copy(reinterpret_cast<unsigned char *>(a.local_full + (size_t)p * C + s0), mine + a.off_full + ((size_t)p * C + s0) * 4, (s1 - s0) * 4,
             threadIdx.x, blockDim.x);
}

}  // namespace

extern "C" {

// ---- multi-GPU: RCCL over xGMI, one process per GPU ---------------------------------------------
// The reference is one process and one thread; these collectives are new.  Rendezvous (handing the
// 128-byte id of rank 0 to the other ranks) is the caller's business (bench.py uses torch.distributed/gloo for it).
sdm_status sdm_comm_unique_id(uint8_t out[128]) {
  if (!out) return SDM_ERR_INVALID_ARGUMENT;
  static_assert(NCCL_UNIQUE_ID_BYTES == 128, "id size");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(out, id.internal, 128);
  return SDM_OK;
}

// what sdm_comm_init and sdm_ipc_create end in: the HIP events around every collective (sdm_comm_timing), the time limit,
// the set-up work done, the frame pointed at the exchange buffers
static sdm_status exchange_ready(sdm_map *m) {
  for (hipEvent_t &e : m->ev_comm)
    if (!e) SDM_TRY(new_event(m, &e, hipEventDefault));
  const char *t = getenv("SDM_COMM_TIMEOUT_MS");
  if (t && atoi(t) > 0) m->comm_timeout_ms = atoi(t);
  HIP_TRY(hipStreamSynchronize(m->stream));
  return sdm_set_halo_buffers(m, m->d_counts_local, m->d_counts_all, m->d_halo_send, m->d_halo_recv, (int32_t)m->halo_cap_own);
}

static sdm_status comm_init(sdm_map *m, const uint8_t id_bytes[128], int32_t halo_cap_records) {
  HIP_TRY(hipSetDevice(m->device));
  const int world = m->cfg.shard_count, rank = m->cfg.shard_rank;
  ncclUniqueId id;
  memcpy(id.internal, id_bytes, 128);
  NCCL_TRY(ncclCommInitRank(&m->comm, world, id, rank));
  m->halo_cap_own = halo_cap_records > 0 ? (uint32_t)halo_cap_records : (uint32_t)SDM_HALO_DEFAULT_CAP;
  const size_t hb = halo_segment_bytes(m->halo_cap_own) * (size_t)world;
  const size_t ck_elems = (size_t)m->ck_chunk * world;
  SDM_TRY(alloc_tracked(m, &m->d_counts_all, (size_t)world * HALO_OBJ));
  SDM_TRY(alloc_tracked(m, &m->d_halo_send, hb));
  SDM_TRY(alloc_tracked(m, &m->d_halo_recv, hb));
  SDM_TRY(alloc_tracked(m, &m->d_ck_stage, ck_elems));
  SDM_TRY(alloc_tracked(m, &m->d_ck_full, ck_elems));
  HIP_TRY(hipMemsetAsync(m->d_halo_send, 0, hb, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_halo_recv, 0, hb, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_stage, 0, ck_elems * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_full, 0, ck_elems * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_part, 0, ck_elems * 4, m->stream));
  // how the partial ck images are combined (sdm_update_sharded; both give the slab-ordered float sums the oracle's
  // `ck_slabs` forms): SDM_CK_EXCHANGE=allgather for the one-collective variant, sdm_comm_set_options at run time
  const char *e = getenv("SDM_CK_EXCHANGE");
  if (e && !strcmp(e, "allgather")) m->ck_exchange = 1;
  SDM_TRY(alloc_tracked(m, &m->d_ck_all, ck_elems * (size_t)world));
  HIP_TRY(hipMemsetAsync(m->d_ck_all, 0, ck_elems * (size_t)world * 4, m->stream));
  return exchange_ready(m);
}

sdm_status sdm_comm_init(sdm_map *m, const uint8_t id_bytes[128], int32_t halo_cap_records) {
  if (!m || !id_bytes || halo_cap_records < 0 || m->comm) return SDM_ERR_INVALID_ARGUMENT;
  const sdm_status rc = comm_init(m, id_bytes, halo_cap_records);
  if (rc != SDM_OK) exchange_teardown(m);  // (all of it or none)
  return rc;
}

// The exchanges without RCCL.  sdm_ipc_create allocates this shard's receive arena (fine-grained device memory where the
// runtime hands out an IPC handle for it: peers write into it while this GPU's kernels poll its flags; SDM_IPC_ALLOC=coarse
// forces plain device memory) and returns its hipIpc handle; the caller hands the handles of all shards round (64 bytes
// each, any transport) and sdm_ipc_connect maps the peers' arenas.  sdm_update_sharded then uses them.
static sdm_status ipc_create(sdm_map *m, int32_t halo_cap_records, uint8_t handle_out[64]) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "the handle travels as 64 bytes");
  HIP_TRY(hipSetDevice(m->device));
  const int world = m->cfg.shard_count;
  if (world > IPC_MAX_SHARDS) {
    set_error("sdm_ipc_create", __FILE__, __LINE__, "more than 16 shards");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  m->halo_cap_own = halo_cap_records > 0 ? (uint32_t)halo_cap_records : (uint32_t)SDM_HALO_DEFAULT_CAP;
  const size_t seg = halo_segment_bytes(m->halo_cap_own);
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  m->ipc_off_counts = IPC_OFF_DATA;
  m->ipc_off_halo = up(m->ipc_off_counts + (size_t)world * HALO_OBJ * 4);
  m->ipc_off_stage = up(m->ipc_off_halo + (size_t)world * seg);
  m->ipc_off_full = up(m->ipc_off_stage + (size_t)world * m->ck_chunk * 4);
  m->ipc_bytes = up(m->ipc_off_full + (size_t)world * m->ck_chunk * 4);
  const char *mode = getenv("SDM_IPC_ALLOC");
  void *p = nullptr;
  hipIpcMemHandle_t h;
  bool have = false;
  if (!(mode && !strcmp(mode, "coarse"))) {
    if (hipExtMallocWithFlags(&p, m->ipc_bytes, hipDeviceMallocFinegrained) == hipSuccess) {
      if (hipIpcGetMemHandle(&h, p) == hipSuccess) {
        have = true;
        m->ipc_fine_grained = 1;
      } else {
        (void)hipFree(p);
        p = nullptr;
      }
    }
    (void)hipGetLastError();
  }
  if (!have) HIP_TRY(hipMalloc(&p, m->ipc_bytes));
  m->ipc_arena = (unsigned char *)p;  // (the map's from here on: exchange_teardown frees it)
  if (!have) HIP_TRY(hipIpcGetMemHandle(&h, p));
  if (getenv("SDM_IPC_VERBOSE"))
    fprintf(stderr, "sdm_ipc_create: shard %d of %d, arena %zu bytes, %s device memory\n", m->cfg.shard_rank, world, m->ipc_bytes,
            m->ipc_fine_grained ? "fine-grained" : "coarse-grained");
  HIP_TRY(hipMemsetAsync(p, 0, m->ipc_bytes, m->stream));
  // the frame's exchange buffers are regions of the arena; the export segments stay local (pushed by the exchange kernel)
  SDM_TRY(alloc_tracked(m, &m->d_counts_all_local, (size_t)world * HALO_OBJ));
  SDM_TRY(alloc_tracked(m, &m->d_ck_full_local, (size_t)world * m->ck_chunk));
  SDM_TRY(alloc_tracked(m, &m->d_ipc_sync, 32));
  HIP_TRY(hipMemsetAsync(m->d_counts_all_local, 0, (size_t)world * HALO_OBJ * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_full_local, 0, (size_t)world * m->ck_chunk * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ipc_sync, 0, 32 * 4, m->stream));
  m->d_counts_all = m->d_counts_all_local;  // (k_move_apply reads the rows from there: the exchange copies them on)
  m->d_halo_recv = m->ipc_arena + m->ipc_off_halo;
  m->d_ck_stage = (float *)(m->ipc_arena + m->ipc_off_stage);
  m->d_ck_full = (float *)(m->ipc_arena + m->ipc_off_full);
  SDM_TRY(alloc_tracked(m, &m->d_halo_send, seg * (size_t)world));
  HIP_TRY(hipMemsetAsync(m->d_halo_send, 0, seg * (size_t)world, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_part, 0, (size_t)m->ck_chunk * world * 4, m->stream));
  memcpy(handle_out, &h, 64);
  return exchange_ready(m);
}
sdm_status sdm_ipc_create(sdm_map *m, int32_t halo_cap_records, uint8_t handle_out[64]) {
  if (!m || !handle_out || halo_cap_records < 0 || m->comm || m->ipc_arena) return SDM_ERR_INVALID_ARGUMENT;
  const sdm_status rc = ipc_create(m, halo_cap_records, handle_out);
  if (rc != SDM_OK) exchange_teardown(m);  // (all of it or none)
  return rc;
}

sdm_status sdm_ipc_connect(sdm_map *m, const uint8_t *handles_all) {
  if (!m || !handles_all || !m->ipc_arena || m->ipc) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  const int world = m->cfg.shard_count, rank = m->cfg.shard_rank;
  for (int p = 0; p < world; ++p) {
    if (p == rank) {
      m->ipc_peer[p] = m->ipc_arena;
      continue;
    }
    hipIpcMemHandle_t h;
    memcpy(&h, handles_all + (size_t)p * 64, 64);
    HIP_TRY(hipIpcOpenMemHandle(&m->ipc_peer[p], h, hipIpcMemLazyEnablePeerAccess));
  }
  m->ipc = true;
  return SDM_OK;
}

sdm_status sdm_comm_set_options(sdm_map *m, int32_t ck_exchange, int32_t timeout_ms) {
  if (m && m->ipc && ck_exchange < 0 && timeout_ms > 0) {
    m->comm_timeout_ms = timeout_ms;
    return SDM_OK;
  }
  if (!m || !m->comm || ck_exchange < -1 || ck_exchange > 1) return SDM_ERR_INVALID_ARGUMENT;
  if (ck_exchange >= 0) m->ck_exchange = ck_exchange;
  if (timeout_ms > 0) m->comm_timeout_ms = timeout_ms;
  return SDM_OK;
}

sdm_status sdm_ck_chunk_elems(sdm_map *m, int64_t *chunk_out) {
  if (!m || !chunk_out) return SDM_ERR_INVALID_ARGUMENT;
  *chunk_out = m->ck_chunk;
  return SDM_OK;
}

// Step between the two ck exchanges: stage = shard_count parts of chunk floats (part s = shard s's partial sums for the
// pixels this shard owns), summed in slab order into this shard's chunk of full (shard_count x chunk floats).
sdm_status sdm_ck_reduce(sdm_map *m, const float *stage_dev, float *full_dev) {
  if (!m || !stage_dev || !full_dev) return SDM_ERR_INVALID_ARGUMENT;
  if (stage_done(m->stop_after, SDM_STAGE_VISIBILITY)) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  launch_ck_reduce_chunk(stage_dev, nullptr, full_dev, m->ck_chunk, m->cfg.shard_count, m->cfg.shard_rank, m->stream);
  return SDM_OK;
}

sdm_status sdm_comm_timing(sdm_map *m, int32_t on) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->comm_timing = on != 0;
  for (bool &b : m->comm_timed) b = false;
  return SDM_OK;
}

// GPU time of the four collectives of the last sdm_update_sharded frame, microseconds (0 for one the frame did not
// issue): [0] member counts (all-gather, beside the previous frame's sweep), [1] slab-crossing copies (all-to-all),
// [2] partial ck chunks to their owners (all-to-all), [3] summed chunks (all-gather).  Waits for the frame.
sdm_status sdm_get_comm_times(sdm_map *m, double out_us[4]) {
  if (!m || !out_us || (!m->comm && !m->ipc)) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  if (m->s_moves) HIP_TRY(hipStreamSynchronize(m->s_moves));
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int k = 0; k < 4; ++k) {
    out_us[k] = 0.0;
    if (!m->comm_timed[k]) continue;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m->ev_comm[2 * k], m->ev_comm[2 * k + 1]));
    out_us[k] = (double)ms * 1e3;
  }
  return SDM_OK;
}

}  // extern "C"

namespace sdm {
// one exchange through the peers' arenas (k_ipc_exchange): kind, where this shard's pieces lie, where they land
static sdm_status ipc_exchange(sdm_map *m, uint32_t kind, const void *src, size_t src_stride, size_t dst_off, size_t dst_stride, size_t piece_bytes,
                        uint32_t halo_cap, bool copy_own, hipStream_t s, void *local = nullptr) {
  IpcXchg a;
  memset(&a, 0, sizeof(a));
  const int world = m->cfg.shard_count;
  for (int p = 0; p < world; ++p) a.arena[p] = (unsigned char *)m->ipc_peer[p];
  a.world = world;
  a.rank = m->cfg.shard_rank;
  a.kind = kind;
  a.seq = ++m->ipc_seq[kind];
  a.src = (const unsigned char *)src;
  a.src_stride = src_stride;
  a.dst_off = dst_off;
  a.dst_stride = dst_stride;
  a.piece_bytes = (uint32_t)piece_bytes;
  a.halo_cap = halo_cap;
  a.copy_own = copy_own ? 1 : 0;
  a.local = (unsigned char *)local;
  a.timeout_ticks = (unsigned long long)m->comm_timeout_ms * 100000ull;
  hipLaunchKernelGGL(k_ipc_exchange, dim3((unsigned)world), dim3(1024), 0, s, a);
  HIP_TRY(hipGetLastError());
  return SDM_OK;
}
// the count rows of all shards (all-gather), on stream s
sdm_status exchange_counts(sdm_map *m, hipStream_t s) {
  if (m->ipc)
    return ipc_exchange(m, IPC_COUNTS, m->d_counts_local, 0, m->ipc_off_counts, HALO_OBJ * sizeof(int32_t), HALO_OBJ * sizeof(int32_t), 0, true, s,
                        m->d_counts_all_local);
  NCCL_TRY(ncclAllGather(m->d_counts_local, m->d_counts_all, HALO_OBJ, ncclInt32, m->comm, s));
  return SDM_OK;
}
// ncclSend / ncclRecv of one equally sized piece per peer (all-to-all).  This rank's own piece stays where it is: nobody
// imports a shard's export segment to itself, and the chunk reduction reads its own part from the partial image (until
// round 6 it was a device copy on the frame's critical path, 5 us each).
static sdm_status all_to_all(sdm_map *m, const void *send, void *recv, size_t piece_bytes, hipStream_t s) {
  const int world = m->cfg.shard_count, rank = m->cfg.shard_rank;
  if (world == 1) return SDM_OK;
  NCCL_TRY(ncclGroupStart());
  for (int peer = 0; peer < world; ++peer) {
    if (peer == rank) continue;
    NCCL_TRY(ncclSend((const char *)send + (size_t)peer * piece_bytes, piece_bytes, ncclUint8, peer, m->comm, s));
    NCCL_TRY(ncclRecv((char *)recv + (size_t)peer * piece_bytes, piece_bytes, ncclUint8, peer, m->comm, s));
  }
  NCCL_TRY(ncclGroupEnd());
  return SDM_OK;
}
// (m->stream is idle) the error word of this shard's arena: an exchange that gave up waiting for a peer left its kind there
sdm_status exchange_check(sdm_map *m) {
  if (!m->ipc) return SDM_OK;
  uint32_t err = 0;
  HIP_TRY(hipMemcpyAsync(&err, m->ipc_arena + IPC_OFF_ERR, 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (err) {
    static const char *const kind[] = {"member counts", "export segments", "partial ck chunks", "summed ck chunks"};
    char buf[160];
    snprintf(buf, sizeof(buf), "an exchange through the peers' arenas (%s) did not complete in time: a shard is missing or out of step",
             kind[(err - 1) & 3]);
    set_error("sdm_update_sharded", __FILE__, __LINE__, buf);
    return SDM_ERR_COMM;
  }
  return SDM_OK;
}

// A sharded frame ends in collectives that only finish when every shard has issued its own: a shard that died or fell
// out of step leaves the others waiting for ever.  The wait is therefore bounded (SDM_COMM_TIMEOUT_MS, 30 s): past it
// the communicator is aborted - which releases the stream - and the caller gets SDM_ERR_COMM instead of a hang.
sdm_status exchange_wait(sdm_map *m) {
  const auto t0 = std::chrono::steady_clock::now();
  for (hipStream_t st : {m->s_moves, m->s_frustum, m->s_birth, m->stream}) {
    if (!st) continue;
    for (;;) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) HIP_TRY(q);
      ncclResult_t async = ncclSuccess;
      const bool failed = ncclCommGetAsyncError(m->comm, &async) == ncclSuccess && async != ncclSuccess && async != ncclInProgress;
      if (failed || std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > m->comm_timeout_ms) {
        (void)ncclCommAbort(m->comm);
        m->comm = nullptr;
        set_error("sdm_synchronize", __FILE__, __LINE__,
                  failed ? ncclGetErrorString(async) : "a collective of the sharded frame did not finish in time (a peer is missing?): communicator aborted");
        return SDM_ERR_COMM;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
  }
  return SDM_OK;
}

// Back to a map without exchanges: the communicator, the peers' mappings, the arena (the receive buffers are regions of
// it) and the exchange buffers.  Shared by sdm_destroy and by an sdm_comm_init / sdm_ipc_create that fails half-way.
void exchange_teardown(sdm_map *m) {
  if (m->comm) (void)ncclCommDestroy(m->comm);
  m->comm = nullptr;
  for (int p = 0; p < IPC_MAX_SHARDS; ++p) {
    if (m->ipc_peer[p] && m->ipc_peer[p] != m->ipc_arena) (void)hipIpcCloseMemHandle(m->ipc_peer[p]);
    m->ipc_peer[p] = nullptr;
  }
  if (m->ipc_arena) {
    (void)hipFree(m->ipc_arena);
    m->ipc_arena = nullptr;
    m->d_counts_all = nullptr;  // (= d_counts_all_local, released below)
    m->d_halo_recv = nullptr;
    m->d_ck_stage = m->d_ck_full = nullptr;
  }
  m->ipc = false;
  for (void **p : {(void **)&m->d_counts_all, (void **)&m->d_halo_send, (void **)&m->d_halo_recv, (void **)&m->d_ck_stage, (void **)&m->d_ck_full,
                   (void **)&m->d_ck_all, (void **)&m->d_counts_all_local, (void **)&m->d_ck_full_local, (void **)&m->d_ipc_sync})
    map_release(m, p);
  (void)sdm_set_halo_buffers(m, nullptr, nullptr, nullptr, nullptr, 0);
}

namespace {
struct CommTimer {
  sdm_map *m;
  int k;
  hipStream_t s;
  CommTimer(sdm_map *m_, int k_, hipStream_t s_) : m(m_), k(k_), s(s_) {
    if (m->comm_timing) (void)hipEventRecord(m->ev_comm[2 * k], s);
  }
  ~CommTimer() {
    if (m->comm_timing) {
      (void)hipEventRecord(m->ev_comm[2 * k + 1], s);
      m->comm_timed[k] = true;
    }
  }
};
}  // namespace

}  // namespace sdm

extern "C" {

// One frame of a sharded map with all exchanges done here, everything stream-ordered (no host synchronisation):
//   start   -> all-gather of the member counts (64 ints per shard; on the member-count stream, i.e. beside the previous
//              frame's sweep - frame_enqueue_start issues it)
//   moves   -> all-to-all of the export segments (slab-crossing copies go to the shard that owns their target voxel)
//   predict -> all-to-all of the partial ck image's chunks to their owners, slab-ordered sum there, all-gather of the
//              summed chunks
//   finish
// Received per shard and frame: (G-1) x [256 B + 16 B + cap x 36 B + 2 x 4 x H*W/G B].
sdm_status sdm_update_sharded(sdm_map *m, const float *depth, const sdm_labeled_point *cloud, const float cam_pos[3],
                              const float cam_q[4], const sdm_object_move *moves, int32_t n_moves,
                              const int32_t *remove_tracks, int32_t n_remove, uint32_t flags) {
  if (!m || (!m->comm && !m->ipc)) return SDM_ERR_INVALID_ARGUMENT;
  const int world = m->cfg.shard_count, rank = m->cfg.shard_rank;
  for (bool &b : m->comm_timed) b = false;
  m->sharded_frame = true;
  sdm_status rc = sdm_frame_start(m, depth, cloud, cam_pos, cam_q, moves, n_moves, remove_tracks, n_remove, flags, 0);
  m->sharded_frame = false;
  if (rc != SDM_OK) return rc;
  rc = sdm_frame_moves(m);
  if (rc != SDM_OK) return rc;
  while (m->mv_batch_ready) {  // the further batches of a long object list: counts all-gathered on the main stream, batch applied
    if ((rc = exchange_counts(m, m->stream)) != SDM_OK) return rc;
    if ((rc = sdm_frame_moves(m)) != SDM_OK) return rc;
  }
  if (n_moves > 0) {
    CommTimer t(m, 1, m->stream);
    const size_t seg = halo_segment_bytes(m->halo_cap_own);
    rc = m->ipc ? ipc_exchange(m, IPC_HALO, m->d_halo_send, seg, m->ipc_off_halo, seg, seg, m->halo_cap_own, false, m->stream)
                : all_to_all(m, m->d_halo_send, m->d_halo_recv, seg, m->stream);
    if (rc != SDM_OK) return rc;
  }
  const float *part = nullptr;
  rc = sdm_frame_predict(m, &part);
  if (rc != SDM_OK) return rc;
  if (m->ck_exchange == 1 && !m->ipc) {
    // ONE collective: every shard gets every shard's whole partial image ((G - 1) x H*W floats received instead of
    // 2 (G - 1) / G x H*W) and adds the G of them itself, in slab order (k_ck_finish) - the same float sums, one
    // latency-bound RCCL launch less on the frame's critical path.  Which of the two wins at 8 ranks is a question for the
    // first 8-GPU run: `collectives_us` in bench.py's line reports whichever ran.
    const size_t padded = (size_t)m->ck_chunk * world;
    {
      CommTimer t(m, 2, m->stream);
      NCCL_TRY(ncclAllGather(part, m->d_ck_all, padded, ncclFloat32, m->comm, m->stream));
    }
    m->ck_part_stride = padded;
    return sdm_update_finish(m, m->d_ck_all, world, flags, 0);
  }
  if (m->ipc) {  // parts to their owners, slab-ordered sum, summed chunks to everybody: one launch (k_ipc_ck)
    {
      CommTimer t(m, 2, m->stream);
      IpcCk a;
      memset(&a, 0, sizeof(a));
      for (int p = 0; p < world; ++p) a.arena[p] = (unsigned char *)m->ipc_peer[p];
      a.world = world;
      a.rank = rank;
      a.seq = ++m->ipc_seq[IPC_CK_PARTS];
      a.chunk = m->ck_chunk;
      a.split = std::max(4, 64 / world);
      a.off_stage = m->ipc_off_stage;
      a.off_full = m->ipc_off_full;
      a.part = part;
      a.local_full = m->d_ck_full_local;
      a.sync = m->d_ipc_sync;
      a.timeout_ticks = (unsigned long long)m->comm_timeout_ms * 100000ull;
      hipLaunchKernelGGL(k_ipc_ck, dim3((unsigned)(world * a.split)), dim3(1024), 0, m->stream, a);
      HIP_TRY(hipGetLastError());
    }
    return sdm_update_finish(m, m->d_ck_full_local, 1, flags, 0);
  }
  {
    CommTimer t(m, 2, m->stream);
    if ((rc = all_to_all(m, part, m->d_ck_stage, (size_t)m->ck_chunk * 4, m->stream)) != SDM_OK) return rc;
  }
  launch_ck_reduce_chunk(m->d_ck_stage, part, m->d_ck_full, m->ck_chunk, world, rank, m->stream);
  {
    CommTimer t(m, 3, m->stream);
    NCCL_TRY(ncclAllGather(m->d_ck_full + (size_t)rank * m->ck_chunk, m->d_ck_full, m->ck_chunk, ncclFloat32, m->comm, m->stream));
  }
  return sdm_update_finish(m, m->d_ck_full, 1, flags, 0);
}

}  // extern "C"
