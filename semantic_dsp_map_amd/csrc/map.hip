// map.hip — host side of libsdm_hip: the map object behind the C ABI (include/sdm.h).
//
// Host work per frame is O(axis length): the ego-centre ring shift of the reference moves no particle
// data, it only stamps the slabs that were recycled (mc_ring/operations.h:68-96, 1111-1191); everything
// else is enqueued on one HIP stream with no host synchronisation inside a frame.
#include <rccl/rccl.h>
#include <rocrand/rocrand.h>
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "sdm_internal.h"
#include "sdm_scratch.h"

#pragma clang fp contract(off)

namespace {

thread_local std::string g_last_error;

// Kernel arguments in device memory instead of host-coherent memory: the frame is a chain of ~50 short launches, each with
// 0.5-3.4 KB of arguments the command processor fetches before the kernel can start; with the default (host memory, read
// over PCIe) that fetch sits in every gap between dependent launches.  Measured on MI355X / ROCm 7.2, C3 benchmark frames:
// 0.319-0.332 ms without, 0.300-0.302 ms with.  The HIP runtime reads the variable when it initialises (first HIP call of
// the process), so it is set when this library is loaded - unless the user has set it, or HIP is already up (then
// nothing changes).
//
// (Not set here: GPU_MAX_HW_QUEUES.  32 hardware queues seemed to cure the two "modes" of the frame time on one box and
// did nothing on another; stream creation took twice as long and a pytest process that had created and destroyed ~120
// maps aborted inside the runtime.  The modes were the host's NUMA node: bind_host_thread_to below.)
// (Priority 101: before the constructors that register this library's kernels with the runtime - they are what brings
// the runtime up when nothing else in the process has, and run at the default priority.)
__attribute__((constructor(101))) void sdm_runtime_defaults() {
  setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
}

// How a plain frame is issued.  Measured on MI355X / ROCm 7.2 (host time inside sdm_update per frame; GPU time per
// benchmark frame, frames back to back, several runs):
//   launches  launch by launch, three side streams, events between them     105-160 us   0.312-0.325 ms, steady
//   pieces    five chain graphs - frustum chain, birth-candidate chain, three sections of the main stream - launched on
//             the streams of the launch-by-launch frame with the same events between them (hipGraphLaunch of a CHAIN
//             of kernel nodes costs the host 5 us whatever its length; the events the rest)
//                                                                            45-95 us     0.335-0.364 ms
//   branched  one graph with the two side chains as branches: a graph with forks and joins is submitted piecewise by
//             the runtime, with synchronisation between the pieces             78-100 us    0.305-0.345 ms
//   chain     ONE chain of all 40 kernels, nothing overlaps                   5-7 us       0.397-0.406 ms, steady
// The graphs' GPU times scatter from run to run on the same box; launch by launch is the steadiest and on average the
// fastest on the GPU, and costs the host the most.  So the default goes by the host: launches while the host issues a
// frame in well under a frame's GPU time, pieces on a host 2-4.5 x slower than this one, the chain beyond that (where
// even the pieces' dozen calls would take longer than the chain needs on the GPU).  The host's speed is measured when
// the map is created: the time to issue 50 launches - a frame's worth - of an empty kernel (this host: 34-40 us; the
// frame's real launches, with their arguments and events, take it 105-160 us).
enum { GRAPH_PIECES = 0, GRAPH_BRANCHED = 1, GRAPH_CHAIN = 2 };
// (Round 6: 75 -> 110 us.  The line was drawn when a frame took 0.31 ms on the GPU and the five graphs 0.34; at 0.206 ms
// launch by launch the graphs' frame is 0.26 ms, and a host that measures 76 us - the round's final profile box did, the
// pool's usual 56-73 us - still issues a frame in 0.15 ms, ahead of the GPU.  Launch by launch stops paying where the host
// needs longer than the graphs' frame: about twice the burst figure, 130 us.)
constexpr double GRAPH_PIECES_US = 110.0, GRAPH_CHAIN_US = 170.0;
constexpr int LAUNCHES_PER_FRAME = 50;

__global__ void k_noop() {}
// Do two streams of a map run side by side?  k_spin holds its stream for `ticks` of the 100 MHz wall clock and leaves the
// clock at its start and end; k_stamp, launched right behind it on another stream, leaves the clock when it runs.
__global__ void k_spin(unsigned long long ticks, unsigned long long *out) {
  const unsigned long long t0 = wall_clock64();
  out[0] = t0;
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  out[1] = wall_clock64();
}
__global__ void k_stamp(unsigned long long *out) { *out = wall_clock64(); }

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

void set_error(const char *what, const char *file, int line, const char *detail) {
  char buf[512];
  snprintf(buf, sizeof(buf), "%s (%s:%d): %s", what, file, line, detail ? detail : "");
  g_last_error = buf;
}

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      set_error(#expr, __FILE__, __LINE__, hipGetErrorString(e_));           \
      return SDM_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)

template <typename T>
hipError_t dev_alloc(T **p, size_t n) {
  return hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T));
}

}  // namespace

using namespace sdm;

struct sdm_map {
  sdm_config cfg{};
  sdm_params prm{};
  Dims d{};
  Frame f{};
  Filter flt{};
  BirthOrder bo{};
  State st{};
  Scratch sc{};
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  // side streams: the frustum reach set (pose only) and the birth candidates + sort (input cloud only) do not depend
  // on the map state, so they run next to the object-move chain and join the main stream through events
  hipStream_t s_frustum = nullptr, s_birth = nullptr, s_moves = nullptr;
  // ev_state: the particles of the last frame are final (after its births, before its sweep); the next frame's
  // member count of the moving objects starts there, next to the sweep
  hipEvent_t ev_state = nullptr, ev_counts = nullptr;
  hipEvent_t ev_vis = nullptr;      // the frame's visibility pass (and binning) has been issued up to here
  bool vis_event_valid = false;
  bool mv_pending = false;          // a member count has run whose k_move_apply has not (it resets the totals)
  bool state_event_valid = false;
  hipEvent_t ev_begin = nullptr, ev_frustum = nullptr, ev_birth = nullptr;
  int birth_which = 0;
  float *ck_user = nullptr;
  bool fused_ck = false;  // single-GPU sdm_update: pass 1 writes ck+kappa directly
  const float *ck_raw_last = nullptr;  // the last frame's summed ck image when pass 2 formed ck + kappa itself (sdm_get_ck_kappa finishes it on demand)
  int32_t stop_after = 0;
  uint32_t frame_flags = 0;
  int n_moves = 0, n_remove = 0;
  // object lists longer than the frame block holds (MAX_MOVE_OBJECTS / MAX_REMOVE_TRACKS): the whole lists, worked off in
  // batches by sdm_frame_moves / sdm_frame_predict (whole maps, launch by launch)
  std::vector<sdm_object_move> moves_all;
  std::vector<int32_t> removes_all;
  size_t mv_batch_next = 0;     // first object of the next batch of a long object list (0: none left)
  bool mv_batch_ready = false;  // Z-slab shard: that batch's member count is issued, its counts await their exchange
  uint32_t mv_seq = 0;            // frames with moving objects so far (FrameArgs::mv_seq)
  uint32_t *d_track_bits = nullptr;  // sdm_tracks_with_particles: one bit per track id
  int32_t *d_counts_local = nullptr;
  // native RCCL path (sdm_comm_init): communicator + exchange buffers owned by the map
  ncclComm_t comm = nullptr;
  // the exchanges of a sharded frame WITHOUT RCCL (sdm_ipc_create / sdm_ipc_connect): every shard owns one receive arena -
  // flags, gathered count rows, import segments, ck parts and summed ck chunks - that its peers have mapped through hipIpc;
  // an exchange is one small kernel that writes this shard's pieces into the peers' arenas, raises a flag per peer and
  // waits for the peers' flags in its own (k_ipc_exchange)
  bool ipc = false;
  unsigned char *ipc_arena = nullptr;
  void *ipc_peer[16] = {};  // [shard]: that shard's arena as this process sees it ([own rank] = ipc_arena)
  uint32_t ipc_seq[4] = {0, 0, 0, 0};  // exchanges issued so far, per kind: the value the flags of the next one carry
  size_t ipc_off_counts = 0, ipc_off_halo = 0, ipc_off_stage = 0, ipc_off_full = 0, ipc_bytes = 0;
  int ipc_fine_grained = 0;
  float *d_ck_full_local = nullptr;      // the summed ck image in ordinary device memory (k_ipc_ck writes it, the weight update reads it)
  int32_t *d_counts_all_local = nullptr; // the gathered count rows, likewise
  uint32_t *d_ipc_sync = nullptr;        // k_ipc_ck's arrival and barrier counters
  int32_t *d_counts_all = nullptr;
  unsigned char *d_halo_send = nullptr, *d_halo_recv = nullptr;
  float *d_ck_stage = nullptr, *d_ck_full = nullptr;  // chunk-owner exchange of the partial ck images (sdm_update_sharded)
  uint32_t halo_cap_own = 0;
  size_t ck_part_stride = 0;     // floats between the partial images handed to the next sdm_update_finish (0 = H*W)
  int ck_exchange = 0;           // 0 chunk-owner reduction (all-to-all + sum + all-gather), 1 one all-gather of the whole partial images
  float *d_ck_all = nullptr;     // ck_exchange 1: shard_count padded partial images
  int comm_timeout_ms = 30000;   // sdm_synchronize gives a sharded frame this long before it aborts the communicator
  uint32_t ck_chunk = 0;  // pixels per shard of the chunk-owner exchange: ceil(H*W / shard_count), a multiple of 64
  // HIP events around every collective of the last sharded frame (sdm_comm_timing): [2k], [2k+1] bracket collective k
  hipEvent_t ev_comm[8]{};
  bool comm_timing = false, comm_timed[4]{};
  bool sharded_frame = false;  // inside sdm_update_sharded
  int32_t *counts_local_user = nullptr;
  const int32_t *counts_all_user = nullptr;
  int device = 0;

  // host ring-buffer state (mc_ring/buffer.h:97-120)
  std::vector<uint32_t> stamps_x, stamps_y, stamps_z;
  int moved_steps[3]{}, eq_steps[3]{};
  float map_center[3]{}, ego_center[3]{}, last_pos[3]{};
  uint32_t global_time_stamp = 0;
  float forgetting_function[5]{};
  bool forgetting_initialized = false;
  float cam_R[9]{}, cam_p[3]{};
  // this frame's scalars (sdm_scratch.h): host copy, the two device blocks and the event that says "the side chains'
  // block is written"
  FrameArgs fa{};
  FrameArgs *d_fa[3]{};        // [0] read by the main-stream kernels, [1] by the frustum chain that runs ahead of the frame, [2] by the member-count chain
  FrameBeginLaunch fb{};       // arguments of k_frame_begin (the frame block travels with it)
  hipEvent_t ev_fa = nullptr;
  const float *cur_depth = nullptr;            // the inputs the last frame read (sdm_get_labeled_cloud)
  const sdm_labeled_point *cur_cloud = nullptr;
  // The launch sequence of a plain frame (sdm_update, device-resident inputs, one GPU) does not depend on the frame:
  // it is captured once into a hipGraph and replayed with one kernel-node parameter update (the frame block) per frame.
  // graph_mode (SDM_GRAPH): 0 never, 1 the branched graph, 3 the chain, 4 the pieces, 2 (default): by the host's speed
  // at issuing launches, measured at creation - launch by launch, the pieces (GRAPH_PIECES_US) or the chain (GRAPH_CHAIN_US).
  int graph_mode = 2;
  bool use_graph = false;
  int graph_shape = 0;             // GRAPH_PIECES / GRAPH_BRANCHED / GRAPH_CHAIN
  hipGraphExec_t piece[5] = {};    // GRAPH_PIECES: frustum chain, birth chain, main stream part 1 / 2 / 3
  double enqueue_us = 0.0;  // measured at creation: host time to issue a frame's worth of launches
  double t_prepare_us = 0, t_setparams_us = 0, t_launch_us = 0, t_direct_us = 0;  // SDM_HOST_TIMING: host time per step of sdm_update
  bool host_timing = false;
  bool capturing = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  hipGraphNode_t graph_set_node = nullptr;
  Filter graph_flt{};          // the filter parameters baked into the captured launches
  hipEvent_t cap_begin = nullptr, cap_frustum = nullptr, cap_birth = nullptr;
  uint64_t n_graph_frames = 0, n_direct_frames = 0;
  int restamped[3]{};        // slabs re-stamped by the last frame's ring shift, per axis
  bool stamps_dirty = true;  // device copy of the stamp arrays needs a full upload
  bool sweep_all = true;     // the next occupancy sweep evaluates every voxel that holds something, changed or not
  // A non-incremental sweep hands the sparse voxels of its tiles to a launch of their own (State::occ_list) - or, where
  // that launch would only cost its 4 us, evaluates them in its first launch: every such sweep leaves word of which it
  // should have been (State::occ_shard: few tiles listed anything = surfaces, lists pay; none or most did, they do not),
  // and the host picks the word up at its next wait (sweep_mode_latch).  Either way every voxel gets the same result.
  bool sweep_lists = true;
  // ... and whether its first launch found anything to do: on a map whose every group of 512 voxels is dense it does not
  // (State::grp_hint), and the next non-incremental sweep is one launch (launch_occupancy, OCC_SKIP_SCAN).
  bool sweep_skip_scan = false;
  bool sweep_skip_allowed = true;  // SDM_SWEEP_SKIP_SCAN=0: always both launches (A/B)
  bool sweep_rec_pending = false;
  int sweep_lists_forced = -1;  // sdm_debug_sweep_lists
  uint32_t sweep_epoch = 1;  // the number the next sweep looks for in State::tile_dirty (mark_tile): advanced by every sweep issued

  // owned device buffers for inputs
  float *d_depth = nullptr;
  sdm_labeled_point *d_cloud = nullptr;
  float *d_ck_part = nullptr;
  // N1 inputs: static mask, label->instance table, object masks (grown on demand)
  // sdm_update_raw: two sets of device-side inputs, filled alternately on a copy stream, so that the upload (and
  // BOOST-mode reduction) of a frame runs beside the previous frame's kernels
  struct RawInputs {
    float *depth = nullptr;
    uint8_t *static_mask = nullptr, *obj_masks = nullptr;
    uint16_t *label_to_inst = nullptr;
    uint16_t label_host[256];  // what label_to_inst holds (the table rarely changes: it is uploaded when it does)
    bool label_valid = false;
    double *bbox = nullptr;  // ZED2: per-object boxes
    int obj_masks_cap = 0;
    hipEvent_t ev_free = nullptr;  // the frame that read this set has been issued up to its end
  } raw[2];
  int raw_next = 0;
  hipStream_t s_copy = nullptr;
  hipEvent_t ev_copy = nullptr;
  unsigned char *d_src_stage = nullptr;  // BOOST mode: one input image at the sensor's size
  size_t src_stage_bytes = 0;
  unsigned long long *d_u64 = nullptr;
  EmitScratch emit;  // compaction of the result lists (getters)
  // page-locked landing area of the getters: [0] the list's length, from byte 16 on the points
  unsigned char *h_emit = nullptr;
  size_t h_emit_bytes = 0;
  uint32_t *h_track_bits = nullptr;  // page-locked landing area of sdm_tracks_with_particles
  size_t emit_guess = 1024;  // points fetched together with the length (the last list's length and a margin)
  sdm_point *d_points = nullptr;
  size_t points_cap = 0;
  // host-mode staging of the batched queries (sdm_query_*): one chunk's inputs and outputs, on the device and page-locked;
  // grown on demand, used by nothing else (a query between two frames changes nothing the next frame reads)
  unsigned char *d_query = nullptr, *h_query = nullptr;
  size_t query_bytes = 0;
  // the distance field (sdm_esdf_update, esdf.hip): site and snapshot word per cell in map-index order, allocated by the
  // first build; the Frame of the frame it was built from (its map center and ring offsets); no frame reads any of it
  uint32_t *d_esdf_site = nullptr, *d_esdf_snap = nullptr;
  Frame esdf_f{};
  bool esdf_valid = false;
  sdm_point_xyzrgb *d_points_rgb = nullptr;
  size_t points_rgb_cap = 0;
  ColourTables *d_colours = nullptr;
  bool colours_set = false;
  int nb_alloc = 0;
  size_t sort_cap = 0;
  int noise_n = 0;
  int force_generic_flood = 0;

  bool profiling = false;
  hipEvent_t ev[9]{};
  bool ev_valid = false;
  bool stage_ran[9]{};
  sdm_stats last_stats{};
  std::vector<void *> allocs;
};

namespace {

template <typename T>
sdm_status alloc_tracked(sdm_map *m, T **p, size_t n) {
  HIP_TRY(dev_alloc(p, n));
  m->allocs.push_back((void *)*p);
  return SDM_OK;
}

// GaussianRandomCalculator::calculateGaussianTable, PDF part (utils/basic_algorithms.h:405-407, 456-460):
// entry i = (1/sqrt(2*(pi/2))) * expf(-x^2/2), x = (i-10000)*0.001.  The quirky normaliser is the reference's.
// The map's streams beyond the three every frame uses (main, frustum chain, birth-candidate chain) are created when they
// are first needed - the member-count stream by Z-slab shards, the copy stream by sdm_update_raw with host inputs - and
// the library stays off the null stream: the runtime hands out at most GPU_MAX_HW_QUEUES (4) hardware queues and lets
// further streams share them.  (Measured while looking for the "later maps of a process are slower" of round 3: neither
// this nor keeping the streams of a destroyed map for the next one changed a later map's frame time - that was the
// launch-mode policy, see sdm_create - but a map that uses three queues instead of six leaves the others to its host.)
hipError_t new_stream(int, hipStream_t *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
void retire_stream(int, hipStream_t s) {
  if (!s) return;
  (void)hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
}
hipError_t lazy_stream(int device, hipStream_t *s) {
  if (*s) return hipSuccess;
  return new_stream(device, s);
}

void build_pdf_table(std::vector<float> &pdf) {
  pdf.resize(PDF_NUM);
  const float pi_2 = 1.5707964f;  // M_PI_2f32
  for (int i = 0; i < PDF_NUM; ++i) {
    float value = (float)(i - PDF_NUM / 2) * 0.001f;
    pdf[i] = (1.f / (sqrtf(2.f * pi_2))) * expf(-powf(value, 2) / (2));
  }
}

// getForgettingFactor (utils/basic_algorithms.h:32-48): table frozen at first use.
void refresh_filter(sdm_map *m) {
  Filter &flt = m->flt;
  const sdm_params &p = m->prm;
  if (!m->forgetting_initialized) {
    for (int i = 0; i < 5; ++i) m->forgetting_function[i] = (float)pow(2.5, -i / p.forgetting_rate);
  }
  for (int c = 0; c < 8; ++c)
    flt.forget[c] = (c < p.max_forget_count && c < 5) ? m->forgetting_function[c] : 0.f;
  flt.p_detect = p.detection_probability;
  flt.noise_number = p.noise_number;
  flt.occ_threshold = p.occupancy_threshold;
  flt.id_transition = p.id_transition_probability;
  flt.independent = p.if_use_independent_filter ? 1 : 0;
  flt.consider_depth_noise = p.if_consider_depth_noise ? 1 : 0;
  // births per valid pixel: the noise flavour makes nb copies, the plain flavour one (semantic_dsp_map.h:789-795)
  flt.nb = p.if_consider_depth_noise ? std::max(p.nb_ptc_num_per_point, 0) : 1;
  flt.use_rng = (p.if_consider_depth_noise && p.nb_ptc_num_per_point != 1) ? 1 : 0;  // :1183-1188
  flt.noise_n = m->noise_n;
}

void build_birth_order(sdm_map *m) {
  const int W = m->d.W, H = m->d.H;
  int off = 0;
  for (int p = 0; p < 9; ++p) {
    int rs = p / 3, cs = p % 3;
    int rows = rs < H ? (H - rs + 2) / 3 : 0;
    int cols = cs < W ? (W - cs + 2) / 3 : 0;
    m->bo.off[p] = off;
    m->bo.cols[p] = cols > 0 ? cols : 1;
    off += rows * cols;
  }
  m->bo.off[9] = off;
}

sdm_status ensure_birth_buffers(sdm_map *m) {
  const size_t hw = (size_t)m->d.W * m->d.H;
  const int nb = std::max(m->flt.nb, 1);
  if (nb <= m->nb_alloc) return SDM_OK;
  size_t need = hw * nb;
  auto re = [&](auto **p, size_t n) -> hipError_t {
    if (*p) (void)hipFree(*p);
    return dev_alloc(p, n);
  };
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(re(&m->sc.bkey_a, need));
  HIP_TRY(re(&m->sc.bval_a, need));
  HIP_TRY(re(&m->sc.bkey_b, need));
  HIP_TRY(re(&m->sc.bval_b, need));
  HIP_TRY(re(&m->sc.bpos, hw * nb));
  HIP_TRY(re(&m->sc.sort_scratch, sort_scratch_elems(need)));
  HIP_TRY(hipMemsetAsync(m->sc.sort_scratch, 0, sort_scratch_elems(need) * 4, m->stream));  // the one-launch scan's words start at zero
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->nb_alloc = nb;
  m->sort_cap = need;
  return SDM_OK;
}

// updateRingbufferIndexParams (mc_ring/operations.h:1111-1191) + getEquivalentSteps* (:1196-1230)
void update_ring_index_params(sdm_map *m) {
  const Dims &d = m->d;
  int steps[3];
  for (int a = 0; a < 3; ++a) steps[a] = static_cast<int>(m->ego_center[a] * d.recip);
  for (int a = 0; a < 3; ++a) m->map_center[a] = static_cast<float>(steps[a]) * d.voxel_size;
  const uint32_t N[3] = {d.NX, d.NY, d.NZ};
  std::vector<uint32_t> *st[3] = {&m->stamps_x, &m->stamps_y, &m->stamps_z};
  for (int a = 0; a < 3; ++a) {
    const int new_moved = steps[a] - m->moved_steps[a];
    const int n = (int)N[a];
    auto stamp = [&](uint32_t idx) {
      (*st[a])[idx] = m->global_time_stamp;
      m->restamped[a]++;
      StampUpdates &su = m->fa.su;
      if (su.n < MAX_STAMP_UPDATES) su.entry[su.n++] = (uint16_t)((a << 12) | idx);
      else m->stamps_dirty = true;  // too many for the kernel-argument list: fall back to a full upload
    };
    if (new_moved > 0) {
      for (int i = 0; i < new_moved; ++i) stamp(axis_correct(i + m->eq_steps[a], N[a]));
    } else if (new_moved < 0) {
      for (int i = 0; i < -new_moved; ++i) stamp(axis_correct(n - 1 - i + m->eq_steps[a], N[a]));
    }
  }
  for (int a = 0; a < 3; ++a) {
    m->moved_steps[a] = steps[a];
    const int n = (int)N[a];
    const int o = steps[a];
    m->eq_steps[a] = o > 0 ? o % n : (o < 0 ? -(-o % n) : 0);
  }
}

// updateEgoCenterPos (mc_ring/operations.h:68-96): jumps larger than a quarter of the smallest axis are split.
// PINNED: norm = sqrt((x*x + y*y) + z*z), normalized() divides by it when it is > 0.
void update_ego_center(sdm_map *m, const float pos[3]) {
  const Dims &d = m->d;
  const float mx = (1 << (d.x_n - 2)) * d.voxel_size;
  const float my = (1 << (d.y_n - 2)) * d.voxel_size;
  const float mz = (1 << (d.z_n - 2)) * d.voxel_size;
  const float max_once = std::min(std::min(mx, my), mz);
  float mv[3] = {pos[0] - m->last_pos[0], pos[1] - m->last_pos[1], pos[2] - m->last_pos[2]};
  const float sq = (mv[0] * mv[0] + mv[1] * mv[1]) + mv[2] * mv[2];
  float dist = sqrtf(sq);
  float unit[3] = {mv[0], mv[1], mv[2]};
  if (sq > 0.f)
    for (int a = 0; a < 3; ++a) unit[a] = mv[a] / dist;
  float new_pos[3] = {m->last_pos[0], m->last_pos[1], m->last_pos[2]};
  while (dist > max_once) {
    for (int a = 0; a < 3; ++a) new_pos[a] = new_pos[a] + unit[a] * max_once;
    for (int a = 0; a < 3; ++a) m->ego_center[a] = new_pos[a];
    update_ring_index_params(m);
    for (int a = 0; a < 3; ++a) mv[a] = pos[a] - new_pos[a];
    dist = sqrtf((mv[0] * mv[0] + mv[1] * mv[1]) + mv[2] * mv[2]);
  }
  for (int a = 0; a < 3; ++a) m->ego_center[a] = pos[a];
  update_ring_index_params(m);
  for (int a = 0; a < 3; ++a) m->last_pos[a] = pos[a];
}

// Extrinsic = inverse of [R(q) | p] (semantic_dsp_map.h:744-747).  PINNED: Eigen's toRotationMatrix
// formula in float, and the rigid inverse [R^T | -(R^T p)] (Eigen's general 4x4 inverse is version-dependent).
void compute_extrinsic(sdm_map *m, const float pos[3], const float q[4]) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  float *R = m->cam_R;
  R[0] = 1.f - (tyy + tzz);
  R[1] = txy - twz;
  R[2] = txz + twy;
  R[3] = txy + twz;
  R[4] = 1.f - (txx + tzz);
  R[5] = tyz - twx;
  R[6] = txz - twy;
  R[7] = tyz + twx;
  R[8] = 1.f - (txx + tyy);
  for (int a = 0; a < 3; ++a) m->cam_p[a] = pos[a];
  float *E = m->f.E;
  for (int r = 0; r < 3; ++r) {
    const float a = R[0 * 3 + r], b = R[1 * 3 + r], c = R[2 * 3 + r];
    E[r * 4 + 0] = a;
    E[r * 4 + 1] = b;
    E[r * 4 + 2] = c;
    E[r * 4 + 3] = -((a * pos[0] + b * pos[1]) + c * pos[2]);
  }
  E[12] = E[13] = E[14] = 0.f;
  E[15] = 1.f;
}

// Conservative map-index bounding box of the view frustum (the BFS of operations.h:1327-1456 never leaves it)
// and the BFS start vertex (operations.h:1312-1321).
void compute_frustum_box(sdm_map *m) {
  const Dims &d = m->d;
  Frame &f = m->f;
  double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
  const double zs[2] = {d.dmin, d.dmax};
  for (int zi = 0; zi < 2; ++zi)
    for (int sx = -1; sx <= 1; sx += 2)
      for (int sy = -1; sy <= 1; sy += 2) {
        // slightly inflated so that float rounding in the device-side test cannot escape the box
        double c[3] = {sx * zs[zi] * d.tanx * 1.001, sy * zs[zi] * d.tany * 1.001, zs[zi] * (zi ? 1.001 : 0.999)};
        for (int a = 0; a < 3; ++a) {
          double g = (double)m->cam_R[a * 3 + 0] * c[0] + (double)m->cam_R[a * 3 + 1] * c[1] +
                     (double)m->cam_R[a * 3 + 2] * c[2] + (double)m->cam_p[a];
          double idx = (g - (double)m->map_center[a] - (double)d.pmin[a]) / (double)d.voxel_size;
          lo[a] = std::min(lo[a], idx);
          hi[a] = std::max(hi[a], idx);
        }
      }
  const int N[3] = {(int)d.NX, (int)d.NY, (int)d.NZ};
  for (int a = 0; a < 3; ++a) {
    long l = (long)std::floor(lo[a]) - 2, h = (long)std::ceil(hi[a]) + 2;
    f.bb0[a] = (int)std::min<long>(std::max<long>(l, 0), N[a]);
    f.bb1[a] = (int)std::min<long>(std::max<long>(h, 0), N[a]);
  }
  // start vertex: the point 1 m in front of the camera, p + R*(0,0,1)
  const float sg[3] = {m->cam_R[2] + m->cam_p[0], m->cam_R[5] + m->cam_p[1], m->cam_R[8] + m->cam_p[2]};
  f.start_ok = 1;
  for (int a = 0; a < 3; ++a) {
    const float sm = sg[a] - m->map_center[a];
    const int v = static_cast<int>((sm + d.pmax[a]) * d.recip);
    f.start_v[a] = v;
    if (v < 0 || v > N[a]) f.start_ok = 0;
    // keep the start vertex inside the box so that the flood sees it
    if (f.start_ok) {
      f.bb0[a] = std::min(f.bb0[a], std::max(v - 1, 0));
      f.bb1[a] = std::max(f.bb1[a], std::min(v + 1, N[a]));
    }
  }
}

void sync_frame_scalars(sdm_map *m) {
  for (int a = 0; a < 3; ++a) {
    m->f.eq[a] = m->eq_steps[a];
    m->f.center[a] = m->map_center[a];
  }
  m->f.gts = m->global_time_stamp;
  m->f.epoch = m->sweep_epoch;
}

sdm_status upload_stamps(sdm_map *m) {
  m->stamps_dirty = false;
  HIP_TRY(hipMemcpyAsync(m->st.stamps_x, m->stamps_x.data(), m->d.NX * 4, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipMemcpyAsync(m->st.stamps_y, m->stamps_y.data(), m->d.NY * 4, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipMemcpyAsync(m->st.stamps_z, m->stamps_z.data(), m->d.NZ * 4, hipMemcpyHostToDevice, m->stream));
  return SDM_OK;
}

void host_initialize(sdm_map *m) {
  std::fill(m->stamps_x.begin(), m->stamps_x.end(), 0u);
  std::fill(m->stamps_y.begin(), m->stamps_y.end(), 0u);
  std::fill(m->stamps_z.begin(), m->stamps_z.end(), 0u);
  m->global_time_stamp = 0;
}

int sweep_mode(const sdm_map *m) { return (m->sweep_lists ? OCC_LISTS : 0) | (m->sweep_skip_scan ? OCC_SKIP_SCAN : 0); }

// (m->stream is idle) what the last non-incremental sweep recommends for the next
sdm_status sweep_mode_latch(sdm_map *m) {
  if (!m->sweep_rec_pending) return SDM_OK;
  uint32_t rec[4] = {0, 0, 0, 0};  // word (two halves), aux[0], aux[1]
  static_assert(offsetof(State::OccListShard, aux) == 8, "the sweep's words to the host are one 16-byte read");
  HIP_TRY(hipMemcpyAsync(rec, &m->st.occ_shard[OCC_LIST_SHARDS].word, 16, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (rec[0] == 1) m->sweep_lists = false;
  if (rec[0] == 2) m->sweep_lists = true;
  if (m->sweep_lists_forced >= 0) m->sweep_lists = m->sweep_lists_forced != 0;
  if (rec[3] == 1) m->sweep_skip_scan = false;
  if (rec[3] == 2) m->sweep_skip_scan = m->sweep_skip_allowed;
  m->sweep_rec_pending = false;
  return SDM_OK;
}

sdm_status check_counters(sdm_map *m, Counters *out) {
  Counters c;
  HIP_TRY(hipStreamSynchronize(m->s_frustum));
  HIP_TRY(hipStreamSynchronize(m->s_birth));
  uint32_t al[2] = {0, 0};  // length and sticky overflow word of the table of older set memberships (State::alias)
  HIP_TRY(hipMemcpyAsync(&c, m->sc.cnt, sizeof(Counters), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipMemcpyAsync(al, m->st.alias, 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  {
    const sdm_status rc = sweep_mode_latch(m);
    if (rc != SDM_OK) return rc;
  }
  if (out) *out = c;
  if (m->ipc) {
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
  }
  if (al[1] != 0 || al[0] > m->st.alias_cap) {
    // sticky (include/sdm.h): once entries were dropped the owner sets are incomplete, and every later frame - also one
    // with removals or births only, which never looks at Counters::overflow's move-list bit - works on incomplete sets
    set_error("capacity", __FILE__, __LINE__, "the table of older owner-set memberships overflowed (more than 8192 particle slots that sit in two "
              "moving objects' sets at once): the owner sets are incomplete until sdm_clear / sdm_load_state");
    return SDM_ERR_CAPACITY;
  }
  if (c.overflow && c.n_halo_dropped > 0) {
    char buf[200];
    snprintf(buf, sizeof(buf), "export segments overflowed: %u slab-crossing copies beyond %u per destination shard were dropped "
             "(raise halo_cap)", c.n_halo_dropped, m->sc.halo_cap);
    set_error("capacity", __FILE__, __LINE__, buf);
    return SDM_ERR_CAPACITY;
  }
  if (c.overflow && c.n_moved > m->sc.cap_move) {
    char buf[160];
    snprintf(buf, sizeof(buf), "moved-copy list overflowed: %u particles of moving objects in one frame, more than %u", c.n_moved,
             m->sc.cap_move);
    set_error("capacity", __FILE__, __LINE__, buf);
    return SDM_ERR_CAPACITY;
  }
  if (c.overflow) {
    set_error("capacity", __FILE__, __LINE__, "visible-particle or move list overflowed: more visible particles than sdm_config.max_visible, more in ONE image row than "
              "max(2 max_visible / height, 2 width slots) - raise max_visible -, or more than 2^20 in one pixel's bin");
    return SDM_ERR_CAPACITY;
  }
  if (c.vis_flood_rounds >= 256 && !c.vis_flood_complex) {
    set_error("flood", __FILE__, __LINE__, "frustum flood fill did not converge");
    return SDM_ERR_NOT_CONVERGED;
  }
  return SDM_OK;
}

}  // namespace

// ======================================================================================= C ABI
extern "C" {

const char *sdm_last_error(void) { return g_last_error.c_str(); }
const char *sdm_version(void) { return "libsdm_hip 0.1 (gfx950)"; }

// The host thread that issues a map's frames belongs on the NUMA node the GPU hangs off.  A frame is a chain of ~50
// dependent launches; the command processor fetches every packet and signals every completion through host memory that
// the runtime allocates where the calling thread runs.  Measured on a two-socket MI355X box (bench.py, 8 processes each):
// pinned to the GPU's node 0.264-0.267 ms per C3 frame (7 of 8; one 0.293), pinned to the other node 0.290-0.297 ms
// (8 of 8), not pinned one or the other - every gap between two dependent kernels is 2-4 us longer from the far socket
// (tools/probes/crossframe.py).  This was the "two modes" of rounds 2 and 3.
// sdm_bind_host_thread moves the CALLING thread (and the threads it starts later) onto the device's node, within the
// CPUs the process is allowed to use; sdm_create calls it unless SDM_NUMA_BIND=0.  Returns the node, -1 if there is
// nothing to do (one node, no sysfs entry, no allowed CPU on that node).
// the calling thread onto NUMA node `node`, within the CPUs the process may use; returns the node, -1: nothing to do
static int bind_to_node(int node) {
  if (node < 0) return -1;
  char path[128];
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  char list[1024] = {0};
  const bool got = fgets(list, sizeof(list), f) != nullptr;
  fclose(f);
  if (!got) return -1;
  // The CPUs the process was allowed BEFORE the first bind: a later bind for a GPU on the other socket (a second map on
  // another device, SdmMap(device=k) after the load-time bind for device 0) chooses among those, not among what an
  // earlier bind narrowed the thread down to - which would leave it nothing to choose from.
  static std::mutex mu;
  static cpu_set_t original;
  static bool have_original = false;
  cpu_set_t allowed, want;
  CPU_ZERO(&want);
  {
    std::lock_guard<std::mutex> g(mu);
    if (!have_original) {
      CPU_ZERO(&original);
      if (sched_getaffinity(0, sizeof(original), &original) != 0) return -1;
      have_original = true;
    }
    allowed = original;
  }
  cpu_set_t current;
  CPU_ZERO(&current);
  if (sched_getaffinity(0, sizeof(current), &current) != 0) return -1;
  int n_want = 0;
  char *save = nullptr;
  for (char *tok = strtok_r(list, ",\n", &save); tok; tok = strtok_r(nullptr, ",\n", &save)) {  // "0-63,128-191"
    int a = 0, b = 0;
    const int k = sscanf(tok, "%d-%d", &a, &b);
    if (k < 1) continue;
    if (k == 1) b = a;
    for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (CPU_ISSET(c, &allowed)) {
        CPU_SET(c, &want);
        ++n_want;
      }
  }
  if (n_want == 0) return -1;  // nothing allowed on that node
  const bool one_node = n_want == CPU_COUNT(&allowed);  // every CPU the process may use is on that node: nothing to choose
  if (!CPU_EQUAL(&want, &current) && sched_setaffinity(0, sizeof(want), &want) != 0) return -1;
  return one_node ? -1 : node;
}
static int numa_node_of_pci(const char *bus_lower) {
  char path[128];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus_lower);
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node;
}
// with the runtime up: HIP knows the device's PCI address
static int bind_host_thread_to(int device) {
  char bus[32] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  for (char *c = bus; *c; ++c) *c = (char)tolower(*c);
  return bind_to_node(numa_node_of_pci(bus));
}
// WITHOUT the runtime (so that its first allocations already land on the right node): HIP device `device` is the
// device-th GPU of the KFD topology (/sys/class/kfd/kfd/topology/nodes/<i>/properties: simd_count > 0, readable only
// for the GPUs this process may open) after ROCR_VISIBLE_DEVICES and HIP_VISIBLE_DEVICES, lists of indices.  Returns
// the NUMA node, -2 if this cannot tell (other forms of the variables, no topology).
static int numa_node_without_runtime(int device) {
  struct Gpu { int domain, location; };
  std::vector<Gpu> gpus;
  for (int i = 0; i < 256; ++i) {
    char path[128];
    snprintf(path, sizeof(path), "/sys/class/kfd/kfd/topology/nodes/%d/properties", i);
    FILE *f = fopen(path, "r");
    if (!f) {
      snprintf(path, sizeof(path), "/sys/class/kfd/kfd/topology/nodes/%d", i);
      if (access(path, F_OK) != 0) break;  // past the last node
      continue;                            // a node this process may not read
    }
    char key[64];
    unsigned long long val = 0;
    long long simd = 0, domain = 0, location = -1;
    while (fscanf(f, "%63s %llu", key, &val) == 2) {
      if (!strcmp(key, "simd_count")) simd = (long long)val;
      else if (!strcmp(key, "domain")) domain = (long long)val;
      else if (!strcmp(key, "location_id")) location = (long long)val;
    }
    fclose(f);
    if (simd > 0 && location >= 0) gpus.push_back({(int)domain, (int)location});
  }
  if (gpus.empty()) return -2;
  for (const char *var : {"ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"}) {
    const char *e = getenv(var);
    if (!e || !*e) continue;
    if (!strcmp(var, "CUDA_VISIBLE_DEVICES") && getenv("HIP_VISIBLE_DEVICES")) continue;  // HIP's own variable wins
    std::vector<Gpu> keep;
    const char *c = e;
    while (*c) {
      if (*c < '0' || *c > '9') return -2;  // a UUID or anything else: cannot tell
      char *end = nullptr;
      const long k = strtol(c, &end, 10);
      if (k < 0 || k >= (long)gpus.size()) break;  // the runtime stops at the first index out of range
      keep.push_back(gpus[(size_t)k]);
      c = end;
      if (*c == ',') ++c;
      else if (*c) return -2;
    }
    gpus.swap(keep);
  }
  if (device < 0 || device >= (int)gpus.size()) return -2;
  char bus[32];
  const int loc = gpus[(size_t)device].location;
  snprintf(bus, sizeof(bus), "%04x:%02x:%02x.%x", gpus[(size_t)device].domain, (loc >> 8) & 0xff, (loc >> 3) & 0x1f, loc & 7);
  const int node = numa_node_of_pci(bus);
  return node < 0 ? -2 : node;
}

int32_t sdm_host_numa_node_early(int32_t device) { return numa_node_without_runtime(device); }

int32_t sdm_bind_host_thread(int32_t device) {
  const char *e = getenv("SDM_NUMA_BIND");
  if (e && e[0] == '0') return -1;
  const int early = numa_node_without_runtime(device);  // no HIP call: the runtime may still be down after this
  if (early >= -1) return bind_to_node(early);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return -1;
  return bind_host_thread_to(device);
}

sdm_status sdm_create(const sdm_config *cfg, sdm_map **out) {
  if (!cfg || !out) return SDM_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  // runSystemChecking (mc_ring/operations.h:54-64)
  if (cfg->x_n + cfg->y_n + cfg->z_n + cfg->p_n > 31 || cfg->x_n < 2 || cfg->y_n < 2 || cfg->z_n < 2 || cfg->p_n < 1 ||
      cfg->p_n > 4 || cfg->x_n > 9 || cfg->y_n > 9 || cfg->z_n > 9 || cfg->width <= 0 || cfg->height <= 0 || !(cfg->voxel_size > 0.f) ||
      cfg->window_half < 0 || cfg->window_half > 7) {
    set_error("sdm_create", __FILE__, __LINE__, "invalid configuration");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  int shard_count = cfg->shard_count > 0 ? cfg->shard_count : 1;
  if (cfg->shard_rank < 0 || cfg->shard_rank >= shard_count || ((1u << cfg->z_n) % (uint32_t)shard_count) != 0) {
    set_error("sdm_create", __FILE__, __LINE__, "invalid shard rank/count (count must divide the z axis)");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
    set_error("sdm_create", __FILE__, __LINE__, "no HIP device / bad device ordinal: libsdm_hip has no CPU path");
    return SDM_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(cfg->device));
  {
    const char *e = getenv("SDM_NUMA_BIND");
    if (!(e && e[0] == '0')) (void)bind_host_thread_to(cfg->device);  // before the streams (their queues) exist
  }
  sdm_map *m = new sdm_map();
  m->cfg = *cfg;
  m->cfg.shard_count = shard_count;
  m->device = cfg->device;
  Dims &d = m->d;
  d.x_n = cfg->x_n;
  d.y_n = cfg->y_n;
  d.z_n = cfg->z_n;
  d.p_n = cfg->p_n;
  d.NX = 1u << d.x_n;
  d.NY = 1u << d.y_n;
  d.NZ = 1u << d.z_n;
  d.S = 1u << d.p_n;
  d.V = d.NX * d.NY * d.NZ;
  d.rz_count = d.NZ / shard_count;
  d.rz_begin = d.rz_count * cfg->shard_rank;
  d.v_count = d.V / shard_count;
  d.v_begin = d.v_count * cfg->shard_rank;
  d.voxel_size = cfg->voxel_size;
  d.recip = 1.f / cfg->voxel_size;  // voxel_size_recip, operations.h:743
  d.pmax[0] = (d.NX >> 1) * cfg->voxel_size;  // operations.h:735-741
  d.pmax[1] = (d.NY >> 1) * cfg->voxel_size;
  d.pmax[2] = (d.NZ >> 1) * cfg->voxel_size;
  for (int a = 0; a < 3; ++a) d.pmin[a] = -d.pmax[a];
  d.W = cfg->width;
  d.H = cfg->height;
  d.fx = cfg->fx;
  d.fy = cfg->fy;
  d.cx = cfg->cx;
  d.cy = cfg->cy;
  d.dmin = cfg->depth_min;
  d.dmax = cfg->depth_max;
  d.tanx = (float)tan(atan2(cfg->width / 2.0, (double)cfg->fx));   // operations.h:1249-1250
  d.tany = (float)tan(atan2(cfg->height / 2.0, (double)cfg->fy));
  d.occl_coeff = 0.1f + 1.f;  // g_depth_error_stddev_at_one_meter + 1.f (settings.h:150, operations.h:1387)
  d.window_half = cfg->window_half;
  d.max_movable = cfg->max_movable_track;
  m->stamps_x.assign(d.NX, 0);
  m->stamps_y.assign(d.NY, 0);
  m->stamps_z.assign(d.NZ, 0);
  // defaults of the SemanticDSPMap constructor (semantic_dsp_map.h:25-42)
  m->prm.detection_probability = 0.95f;
  m->prm.noise_number = 0.1f;
  m->prm.nb_ptc_num_per_point = 3;
  m->prm.occupancy_threshold = 0.2f;
  m->prm.max_obersevation_lost_time = 5;
  m->prm.forgetting_rate = 1.0f;
  m->prm.max_forget_count = 5;
  m->prm.match_score_threshold = 0.3f;
  m->prm.id_transition_probability = 0.1f;
  m->prm.if_consider_depth_noise = 0;
  m->prm.if_use_independent_filter = 0;
  m->prm.depth_noise_first_order = 0.f;
  m->prm.depth_noise_zero_order = 0.1f;

  // (the main stream first: in a process's first map it is the first stream the runtime creates)
  HIP_TRY(new_stream(cfg->device, &m->own_stream));
  m->stream = m->own_stream;
  HIP_TRY(new_stream(cfg->device, &m->s_frustum));
  HIP_TRY(new_stream(cfg->device, &m->s_birth));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_state, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_counts, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_begin, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_frustum, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_birth, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_fa, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->ev_vis, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->cap_begin, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->cap_frustum, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&m->cap_birth, hipEventDisableTiming));
  const size_t n_slots = (size_t)d.v_count * d.S;
  const size_t hw = (size_t)d.W * d.H;
  sdm_status rc;
#define A(ptr, n) \
  if ((rc = alloc_tracked(m, &(ptr), (n))) != SDM_OK) return rc;
  A(m->st.pos4, n_slots);
  A(m->st.forget, n_slots);
  HIP_TRY(hipMemsetAsync(m->st.forget, 0, n_slots, m->stream));
  // one record per voxel: w | ts | track | label (sdm_internal.h); one chunk of 64 records of padding behind the last, so
  // that the sweep's chunk-wide loads need no clamp at the end of the map (k_occupancy_dense)
  A(m->st.rec, rec_array_bytes(d.v_count, d.S));
  // stamps and flags: whole 512-voxel groups plus one chunk - the sweep's chunk-wide loads need no clamp at the end of the
  // map, and a wave of k_occupancy_dense on its fused path loads a whole group's (maps of 64, 128 or 256 voxels are less)
  const size_t v_groups = ((size_t)d.v_count + 511) / 512 * 512;
  A(m->st.vts, v_groups + 64);
  A(m->st.vflag, v_groups + 64);
  m->st.tile_stride = (uint32_t)tile_mark_bytes(d);
  A(m->st.tile_dirty, 2 * (size_t)m->st.tile_stride);
  A(m->st.occ_need, ((size_t)d.v_count + 63) / 64 + 32);
  A(m->st.occ_list, occ_list_tiles(d.v_count) * OCC_LIST_CAP);
  A(m->st.occ_list_n, occ_list_tiles(d.v_count) + 64);
  m->st.occ_unit_cap = (uint32_t)((occ_list_tiles(d.v_count) + OCC_LIST_SHARDS - 1) / OCC_LIST_SHARDS * (OCC_LIST_CAP / OCC_LIST_UNIT));
  A(m->st.occ_unit, (size_t)OCC_LIST_SHARDS * m->st.occ_unit_cap);
  A(m->st.occ_shard, OCC_LIST_SHARDS + 1);
  HIP_TRY(hipMemsetAsync(m->st.occ_shard, 0, (OCC_LIST_SHARDS + 1) * sizeof(State::OccListShard), m->stream));
  A(m->st.grp_hint, grp_hint_bytes(d.v_count));
  HIP_TRY(hipMemsetAsync(m->st.grp_hint, 0, grp_hint_bytes(d.v_count), m->stream));
  A(m->st.owner, n_slots);
  A(m->st.owner_flag, owner_flag_bytes(n_slots));
  A(m->st.owner_flag2, owner_flag2_bytes(n_slots));
  A(m->st.alias, 2 + 2 * ALIAS_CAP);
  m->st.alias_cap = ALIAS_CAP;
  HIP_TRY(hipMemsetAsync(m->st.alias, 0, 8, m->stream));
  A(m->st.alias_filter, ALIAS_FILTER_WORDS);
  HIP_TRY(hipMemsetAsync(m->st.alias_filter, 0, ALIAS_FILTER_WORDS * 4, m->stream));
  A(m->st.res, d.v_count);
  A(m->st.stamps_x, d.NX);
  A(m->st.stamps_y, d.NY);
  A(m->st.stamps_z, d.NZ);
  A(m->st.pdf, PDF_NUM);
  m->noise_n = 1000000;  // GAUSSIAN_RANDOM_NUM, basic_algorithms.h:377
  A(m->st.noise, m->noise_n);
  HIP_TRY(hipMemsetAsync(m->st.noise, 0, (size_t)m->noise_n * 4, m->stream));
  {
    std::vector<float> pdf;
    build_pdf_table(pdf);
    HIP_TRY(hipMemcpyAsync(m->st.pdf, pdf.data(), PDF_NUM * 4, hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));  // (the host table goes out of scope)
  }
  Scratch &sc = m->sc;
  sc.wpl = (int)((d.NX + 1 + 63) / 64);
  const size_t n_words = (size_t)(d.NZ + 1) * (d.NY + 1) * sc.wpl;
  A(sc.vmask, n_words);
  A(sc.reach, n_words);
  sc.wy = (int)((d.NY + 1 + 63) / 64);
  const size_t n_line_words = (size_t)(d.NZ + 1) * sc.wy;
  A(sc.line_ne, n_line_words);
  A(sc.line_ey, n_line_words);
  A(sc.line_ez, n_line_words);
  A(sc.line_reach, n_line_words);
  A(m->d_depth, hw);
  A(m->d_cloud, hw);
  if (d.W >= (1 << ROW_COL_BITS)) {
    set_error("sdm_create", __FILE__, __LINE__, "image width above 4095 (the row kernel of the pixel bins holds one image row in LDS)");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  A(sc.bin_count, hw + 1 + (size_t)d.H * ROW_SUBS * ROW_CNT_STRIDE);
  A(sc.row_win, hw);
  sc.row_cnt = sc.bin_count + hw + 1;
  A(sc.bin_start, (size_t)d.H * (d.W + 1));
  // per-shard capacity is cap_vis / VIS_SHARDS; small maps get head-room for one block's worth of slots per shard
  size_t cap_vis = cfg->max_visible > 0 ? (size_t)cfg->max_visible
                                        : std::min<size_t>(n_slots + (size_t)VIS_SHARDS * 256 * d.S, (size_t)16 << 20);
  cap_vis = (cap_vis + VIS_SHARDS - 1) / VIS_SHARDS * VIS_SHARDS;
  cap_vis = std::min<size_t>(cap_vis, 0xffffff00u);
  sc.cap_vis = (uint32_t)cap_vis;
  // A row's lists hold 2 x its share of the capacity (particles crowd into the image rows the ground and the objects are
  // in) and at least two particles per slot and pixel of the row - or, when the user's max_visible is below that, ALL of
  // the capacity: one crowded row must not void a frame whose particles fit max_visible.  A sub-list holds an eighth of
  // that plus a quarter (k_visibility spreads a row's particles over its sub-lists by lane: evenly, not exactly).
  {
    const size_t row_total = std::min<size_t>(cap_vis, std::max<size_t>(2 * cap_vis / (size_t)d.H, (size_t)2 * d.W * d.S));
    sc.row_cap = (uint32_t)std::max<size_t>(64, (row_total + row_total / 4) / ROW_SUBS + 64);
  }
  A(sc.row_list, (size_t)d.H * ROW_SUBS * sc.row_cap);
  A(sc.bin_idx, cap_vis);
  A(sc.vpix, cap_vis);
  A(sc.vp4, cap_vis);
  A(sc.vtf, cap_vis);
  A(sc.pix4, hw);
  A(sc.pixt, hw);
  A(sc.ck_kappa, hw);
  // pixels reach the heavy list from blocks of TPB consecutive pixels (k_ck_classify), shard = block & 63
  sc.cap_heavy = (uint32_t)(((hw + 255) / 256 + VIS_SHARDS - 1) / VIS_SHARDS * 256);
  A(sc.ck_heavy, (size_t)sc.cap_heavy * VIS_SHARDS);
  A(sc.ck_class, hw);
  m->ck_chunk = (uint32_t)(((hw + shard_count - 1) / shard_count + 63) / 64 * 64);
  A(m->d_ck_part, (size_t)m->ck_chunk * shard_count);  // H*W floats, padded to shard_count whole chunks
  for (auto &r : m->raw) {
    A(r.depth, hw);
    A(r.static_mask, hw);
    A(r.label_to_inst, 256);
    A(r.bbox, 6 * MAX_CLOUD_OBJECTS);
    HIP_TRY(hipEventCreateWithFlags(&r.ev_free, hipEventDisableTiming));
  }
  HIP_TRY(hipEventCreateWithFlags(&m->ev_copy, hipEventDisableTiming));
  A(sc.b_valid, hw + 1);
  A(sc.b_rank, hw + 1);
  // moved particles per frame (objects hold <= ~1e5).  A copy's rank is global - it counts the members of every shard
  // (k_move_apply) - and indexes mv_copy / mv_next on every shard, so the capacity follows the whole map, not the slab
  sc.cap_move = (uint32_t)std::min<size_t>((size_t)d.V * d.S, (size_t)1 << 18);
  A(m->d_counts_local, HALO_OBJ);
  const size_t mv_cnt_n = move_count_elems();
  A(sc.mv_cnt, mv_cnt_n);
  A(sc.mv_list, 8192);
  A(sc.mv_nlist, 4);
  HIP_TRY(hipMemsetAsync(sc.mv_nlist, 0, 4 * sizeof(uint32_t), m->stream));
  A(sc.mv_nmem, 8192);
  A(sc.mv_mem, move_member_elems(n_slots));
  A(sc.mv_tot, move_total_elems());
  HIP_TRY(hipMemsetAsync(sc.mv_tot, 0, move_total_elems() * sizeof(uint32_t), m->stream));
  A(m->d_track_bits, 2048);
  A(sc.mv_copy, sc.cap_move);
  A(sc.track_to_obj, 65536);
  HIP_TRY(hipMemsetAsync(sc.track_to_obj, 0xFF, 65536, m->stream));
  // one scratch buffer per scan call site: the one-launch scan keeps its (self-clearing) words there, which start at zero
  size_t scan_need = scan_scratch_elems(hw + 1);
  A(sc.scan_scratch, scan_need + 16);
  A(sc.scan_scratch_b, scan_scratch_elems(hw + 1) + 16);
  HIP_TRY(hipMemsetAsync(sc.scan_scratch, 0, (scan_need + 16) * 4, m->stream));
  HIP_TRY(hipMemsetAsync(sc.scan_scratch_b, 0, (scan_scratch_elems(hw + 1) + 16) * 4, m->stream));
  A(sc.mv_row, (size_t)d.v_count * MV_ROW);  // (64 bytes per voxel: 1.07 GB at 256^3 - the part has 288 GB)
  HIP_TRY(hipMemsetAsync(sc.mv_row, 0xff, (size_t)d.v_count * MV_ROW * sizeof(uint32_t), m->stream));  // idle: counters and chain heads all ones; the replay leaves them that way
  A(sc.mv_next, sc.cap_move);
  A(sc.cnt, 1);
  A(sc.cur, 1);
  HIP_TRY(hipMemsetAsync(sc.cnt, 0, sizeof(Counters), m->stream));
  HIP_TRY(hipMemsetAsync(sc.cur, 0, sizeof(Cursors), m->stream));
  A(m->d_fa[0], 1);
  A(m->d_fa[1], 1);
  A(m->d_fa[2], 1);
  for (FrameArgs *p : m->d_fa) HIP_TRY(hipMemsetAsync(p, 0, sizeof(FrameArgs), m->stream));
  m->sc.fa = m->d_fa[0];
  m->sc.fa_side = m->d_fa[1];
  m->sc.fa_moves = m->d_fa[2];
  A(m->d_u64, 1);
  A(m->emit.mask, emit_mask_bytes(d));
  A(m->emit.blk_cnt, emit_block_elems(d));
  A(m->emit.total, 4);
#undef A
  m->cur_depth = m->d_depth;
  m->cur_cloud = m->d_cloud;
  {
    const char *e = getenv("SDM_GRAPH");
    if (e && e[0] >= '0' && e[0] <= '4') m->graph_mode = e[0] - '0';
    m->use_graph = m->graph_mode != 0;
    m->graph_shape = m->graph_mode == 1 ? GRAPH_BRANCHED : (m->graph_mode == 3 ? GRAPH_CHAIN : GRAPH_PIECES);
    if (const char *k = getenv("SDM_SWEEP_SKIP_SCAN")) m->sweep_skip_allowed = atoi(k) != 0;
    m->host_timing = getenv("SDM_HOST_TIMING") != nullptr;  // debugging aid: per-step host time of sdm_update on stderr at destroy
  }
  {
    // the line flood keeps its bitmaps in LDS, sized by the map ((NZ+1) x wy x 32 bytes: 148 KB at 512^3 - fits gfx950's
    // 160 KB): where the device offers less than that, every frame takes the generic flood (exact as well)
    int lds_max = 0;
    if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeSharedMemPerBlockOptin, cfg->device) != hipSuccess || lds_max <= 0)
      (void)hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device);
    (void)hipGetLastError();
    if ((size_t)(d.NZ + 1) * sc.wy * 32 > (size_t)std::min(lds_max, 152 * 1024)) m->force_generic_flood = 1;
  }
  refresh_filter(m);
  build_birth_order(m);
  if ((rc = ensure_birth_buffers(m)) != SDM_OK) return rc;
  for (int i = 0; i < 9; ++i) HIP_TRY(hipEventCreate(&m->ev[i]));
  m->ev_valid = true;
  // RingBufferOperations::initialize (operations.h:726-767)
  host_initialize(m);
  launch_clear(d, m->st, m->stream, true);
  if ((rc = upload_stamps(m)) != SDM_OK) return rc;
  HIP_TRY(hipStreamSynchronize(m->stream));
  {
    // how fast does this host issue launches?  (median of five bursts of 16 empty kernels: one burst is noisy, and the
    // answer decides how every frame of this map is issued)
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(1), 0, m->stream);
    HIP_TRY(hipStreamSynchronize(m->stream));
    double burst[5];
    for (int rep = 0; rep < 5; ++rep) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < 16; ++i) hipLaunchKernelGGL(k_noop, dim3(1), dim3(1), 0, m->stream);
      burst[rep] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      HIP_TRY(hipStreamSynchronize(m->stream));
    }
    std::sort(burst, burst + 5);
    // The host's speed is a property of the host, not of this map: the fastest burst any map of the process has seen
    // counts.  (Round 3 took each map's own median: the second and later maps of a process measured 84-122 us where the
    // first had measured 56-73 us - a process that holds more state issues the same sixteen launches slower, or is
    // interrupted more often - crossed the 75 us line and were replayed from the five graphs, whose frame takes 22 us
    // longer on the GPU: the "later maps of a process are slower" of round 3.)
    static std::mutex best_mu;
    static double best_seen = 0.0;
    double best = burst[0];
    {
      std::lock_guard<std::mutex> g(best_mu);
      if (best_seen == 0.0 || best < best_seen) best_seen = best;
      best = best_seen;
    }
    m->enqueue_us = best / 16.0 * LAUNCHES_PER_FRAME;
    if (m->graph_mode == 2) {
      m->use_graph = m->enqueue_us > GRAPH_PIECES_US;
      m->graph_shape = m->enqueue_us > GRAPH_CHAIN_US ? GRAPH_CHAIN : GRAPH_PIECES;
    }
  }
  *out = m;
  return SDM_OK;
}

sdm_status sdm_destroy(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (m->host_timing) {
    const double ng = m->n_graph_frames ? (double)m->n_graph_frames : 1.0, nd = m->n_direct_frames ? (double)m->n_direct_frames : 1.0;
    fprintf(stderr, "sdm host timing: prepare+inputs %.1f us/frame; graph frames %llu: set-params %.1f us, hipGraphLaunch %.1f us; direct frames %llu: %.1f us\n",
            m->t_prepare_us / (ng + nd - ((m->n_graph_frames && m->n_direct_frames) ? 0.0 : 1.0)), (unsigned long long)m->n_graph_frames,
            m->t_setparams_us / ng, m->t_launch_us / ng, (unsigned long long)m->n_direct_frames, m->t_direct_us / nd);
  }
  (void)hipSetDevice(m->device);
  (void)hipStreamSynchronize(m->stream);
  for (void *p : m->allocs) (void)hipFree(p);
  if (m->d_points_rgb) (void)hipFree(m->d_points_rgb);
  if (m->d_colours) (void)hipFree(m->d_colours);
  if (m->h_emit) (void)hipHostFree(m->h_emit);
  if (m->h_track_bits) (void)hipHostFree(m->h_track_bits);
  if (m->h_query) (void)hipHostFree(m->h_query);
  if (m->d_query) (void)hipFree(m->d_query);
  if (m->d_esdf_site) (void)hipFree(m->d_esdf_site);
  if (m->d_esdf_snap) (void)hipFree(m->d_esdf_snap);
  void *extra[] = {m->sc.bkey_a, m->sc.bval_a, m->sc.bkey_b, m->sc.bval_b, m->sc.bpos, m->sc.sort_scratch, m->d_points, m->raw[0].obj_masks, m->raw[1].obj_masks, m->d_src_stage};
  for (void *p : extra)
    if (p) (void)hipFree(p);
  if (m->comm) (void)ncclCommDestroy(m->comm);
  if (m->ipc_arena) {  // (the exchange buffers are regions of the arena)
    for (int p = 0; p < m->cfg.shard_count && p < 16; ++p)
      if (m->ipc_peer[p] && m->ipc_peer[p] != m->ipc_arena) (void)hipIpcCloseMemHandle(m->ipc_peer[p]);
    (void)hipFree(m->ipc_arena);
    for (void *p : {(void *)m->d_halo_send, (void *)m->d_counts_all_local, (void *)m->d_ck_full_local, (void *)m->d_ipc_sync})
      if (p) (void)hipFree(p);
  } else {
    void *comm_bufs[] = {m->d_counts_all, m->d_halo_send, m->d_halo_recv, m->d_ck_stage, m->d_ck_full, m->d_ck_all};
    for (void *p : comm_bufs)
      if (p) (void)hipFree(p);
  }
  for (hipEvent_t e : m->ev_comm)
    if (e) (void)hipEventDestroy(e);
  if (m->ev_valid)
    for (int i = 0; i < 9; ++i) (void)hipEventDestroy(m->ev[i]);
  if (m->s_frustum) (void)hipStreamSynchronize(m->s_frustum);
  if (m->s_birth) (void)hipStreamSynchronize(m->s_birth);
  if (m->s_moves) (void)hipStreamSynchronize(m->s_moves);
  if (m->s_copy) (void)hipStreamSynchronize(m->s_copy);
  for (auto &r : m->raw)
    if (r.ev_free) (void)hipEventDestroy(r.ev_free);
  if (m->ev_copy) (void)hipEventDestroy(m->ev_copy);
  retire_stream(m->device, m->s_copy);
  if (m->ev_state) (void)hipEventDestroy(m->ev_state);
  if (m->ev_counts) (void)hipEventDestroy(m->ev_counts);
  retire_stream(m->device, m->s_moves);
  if (m->ev_begin) (void)hipEventDestroy(m->ev_begin);
  if (m->ev_frustum) (void)hipEventDestroy(m->ev_frustum);
  if (m->ev_birth) (void)hipEventDestroy(m->ev_birth);
  if (m->graph_exec) (void)hipGraphExecDestroy(m->graph_exec);
  for (hipGraphExec_t &g : m->piece)
    if (g) (void)hipGraphExecDestroy(g);
  if (m->graph) (void)hipGraphDestroy(m->graph);
  for (hipEvent_t e : {m->ev_fa, m->ev_vis, m->cap_begin, m->cap_frustum, m->cap_birth})
    if (e) (void)hipEventDestroy(e);
  // (in the order they are taken: the next map's main stream is this map's main stream)
  retire_stream(m->device, m->own_stream);
  retire_stream(m->device, m->s_frustum);
  retire_stream(m->device, m->s_birth);
  delete m;
  return SDM_OK;
}

// SemanticDSPMap::clear (semantic_dsp_map.h:74-81): ring buffer + stamps + global time stamp + object sets;
// the movement of the ring buffer is retained (operations.h:683).
sdm_status sdm_clear(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  m->state_event_valid = false;
  m->vis_event_valid = false;
  m->sweep_all = true;
  m->sweep_skip_scan = false;  // (the groups' hints go with the map; what an unlatched sweep said about them is void)
  m->sweep_rec_pending = false;
  host_initialize(m);
  launch_clear(m->d, m->st, m->stream, false);
  return upload_stamps(m);
}

sdm_status sdm_set_params(sdm_map *m, const sdm_params *p) {
  if (!m || !p) return SDM_ERR_INVALID_ARGUMENT;
  if (p->nb_ptc_num_per_point < 0 || p->nb_ptc_num_per_point > 64) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  m->prm = *p;
  m->sweep_all = true;  // the occupancy threshold may have changed: no stored result is safe
  refresh_filter(m);
  return ensure_birth_buffers(m);
}

sdm_status sdm_generate_noise_table(sdm_map *m, uint64_t seed, int32_t n, float stddev) {
  if (!m || n <= 0 || n > m->noise_n || (n & 1)) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  rocrand_generator gen;
  if (rocrand_create_generator(&gen, ROCRAND_RNG_PSEUDO_PHILOX4_32_10) != ROCRAND_STATUS_SUCCESS) {
    set_error("rocrand_create_generator", __FILE__, __LINE__, "failed");
    return SDM_ERR_HIP;
  }
  rocrand_status rs = rocrand_set_seed(gen, seed);
  if (rs == ROCRAND_STATUS_SUCCESS) rs = rocrand_set_stream(gen, m->stream);
  if (rs == ROCRAND_STATUS_SUCCESS) rs = rocrand_generate_normal(gen, m->st.noise, (size_t)n, 0.0f, stddev);
  (void)hipStreamSynchronize(m->stream);
  rocrand_destroy_generator(gen);
  if (rs != ROCRAND_STATUS_SUCCESS) {
    set_error("rocrand_generate_normal", __FILE__, __LINE__, "failed");
    return SDM_ERR_HIP;
  }
  m->flt.noise_n = n;
  return SDM_OK;
}

sdm_status sdm_upload_noise_table(sdm_map *m, const float *table, int32_t n) {
  if (!m || !table || n <= 0 || n > m->noise_n) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(m->st.noise, table, (size_t)n * 4, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->flt.noise_n = n;
  return SDM_OK;
}

sdm_status sdm_download_noise_table(sdm_map *m, float *table, int32_t n) {
  if (!m || !table || n <= 0 || n > m->noise_n) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(table, m->st.noise, (size_t)n * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

sdm_status sdm_download_pdf_table(sdm_map *m, float *table, int32_t n) {
  if (!m || !table || n <= 0 || n > PDF_NUM) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(table, m->st.pdf, (size_t)n * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

// ---- the frame ---------------------------------------------------------------------------------
// The first half of subObjectLevelUpdate (semantic_dsp_map.h:576-764) in three steps, cut where a Z-slab sharded map
// needs data from the other shards:
//   sdm_frame_start    ego shift; every moving object's local members are collected, per-object counts published
//                      [exchange 1: all-gather of the count rows, HALO_OBJ ints per shard]
//   sdm_frame_moves    global ranks, transform + noise, originals deleted, slab-crossing copies exported
//                      [exchange 2: all-gather of the export buffers]
//   sdm_frame_predict  import, ordered re-insertion, removals, visibility/binning, this shard's partial ck image
//                      [exchange 3: all-gather of the partial ck images]  -> sdm_update_finish
// sdm_update_begin = the three steps back to back (single shard, or a frame without object moves).
//
// Every step is "host arithmetic, then launches".  The host arithmetic of a whole frame sits in frame_host_prepare and
// ends in one FrameArgs block; the launches read their frame scalars from the device copy of that block, so their
// arguments, grids and order are the same every frame.  sdm_update uses that to replay the whole frame as a hipGraph.
namespace {

inline bool stage_done(int32_t stop_after, int stage) { return stop_after != 0 && stop_after <= stage; }
inline void stage_mark(sdm_map *m, int stage) {
  if (m->profiling && !m->capturing) {
    (void)hipEventRecord(m->ev[stage], m->stream);
    m->stage_ran[stage] = true;
  }
}

// P1 on the host: global_time_stamp += 1 (semantic_dsp_map.h:173), ego-centre ring shift (:584-585), extrinsic (:744-747),
// frustum box; the frame block is complete afterwards except for the input pointers.
sdm_status frame_host_prepare(sdm_map *m, const float cam_pos[3], const float cam_q[4], const sdm_object_move *moves, int32_t n_moves,
                              const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after) {
  // Lists longer than the frame block holds are worked off in batches (sdm_frame_moves, sdm_frame_predict).  On a Z-slab
  // shard every batch's per-object member counts are exchanged with the other shards before the batch is applied
  // (sdm_frame_moves / sdm_frame_moves_pending; sdm_update_sharded does it itself).  Only a frame that is being captured
  // into a graph cannot take them - and sdm_update never captures one with long lists.
  if ((n_moves > MAX_MOVE_OBJECTS || n_remove > MAX_REMOVE_TRACKS) && m->capturing) {
    set_error("sdm_update", __FILE__, __LINE__, "object lists beyond one frame block inside a graph capture");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  m->moves_all.clear();
  m->removes_all.clear();
  m->mv_batch_next = n_moves > MAX_MOVE_OBJECTS ? (size_t)MAX_MOVE_OBJECTS : 0;
  m->mv_batch_ready = false;
  if (n_moves > MAX_MOVE_OBJECTS) m->moves_all.assign(moves, moves + n_moves);
  if (n_remove > MAX_REMOVE_TRACKS) m->removes_all.assign(remove_tracks, remove_tracks + n_remove);
  m->stop_after = stop_after;
  m->frame_flags = flags;
  for (int i = 0; i < 9; ++i) m->stage_ran[i] = false;
  m->global_time_stamp += 1;
  FrameArgs &fa = m->fa;
  fa.su.n = 0;
  fa.su.value = m->global_time_stamp;
  m->restamped[0] = m->restamped[1] = m->restamped[2] = 0;
  update_ego_center(m, cam_pos);
  sync_frame_scalars(m);
  if (m->stamps_dirty) {
    m->sweep_all = true;  // stamps replaced wholesale (below): every stored result may be stale
    fa.su.n = 0;
  }
  refresh_filter(m);
  m->forgetting_initialized = true;  // the reference freezes its forgetting table at the first update
  compute_extrinsic(m, cam_pos, cam_q);
  compute_frustum_box(m);
  fa.f = m->f;
  // P2 / P3 inputs: the objects the object layer decided to move (semantic_dsp_map.h:588-693) and to wipe (:702-736)
  memset(&fa.ms, 0, sizeof(fa.ms));
  const int n_first = n_moves < MAX_MOVE_OBJECTS ? n_moves : MAX_MOVE_OBJECTS;  // (the first batch rides in the frame's first kernel)
  fa.ms.n = n_first;
  for (int k = 0; k < n_first; ++k) {
    fa.ms.track[k] = (uint16_t)moves[k].track_id;
    memcpy(fa.ms.T[k], moves[k].T, 12 * sizeof(float));
  }
  fa.n_obj = n_first;
  fa.mv_batch = 0;
  // (the parity of the per-object totals the member count adds up and k_move_apply reads and resets: it advances with
  // every frame in which the two run)
  if (n_moves > 0 && !stage_done(stop_after, 1)) m->mv_seq++;
  fa.mv_seq = m->mv_seq;
  fa.n_remove = n_remove < MAX_REMOVE_TRACKS ? n_remove : MAX_REMOVE_TRACKS;
  for (int k = 0; k < fa.n_remove; ++k) fa.remove[k] = (uint16_t)remove_tracks[k];
  fa.force_generic = m->force_generic_flood;
  m->n_moves = n_moves;
  m->n_remove = n_remove;
  return SDM_OK;
}

sdm_status exchange_counts(sdm_map *m, hipStream_t s);  // (the all-gather of the member-count rows: RCCL or the peers' arenas, below)
// launches of sdm_frame_start: the frame block goes to the device, the chains that depend on nothing but it start
sdm_status frame_enqueue_start(sdm_map *m) {
  hipStream_t s = m->stream;
  const Dims &d = m->d;
  const int32_t stop_after = m->stop_after;
  const bool whole = d.v_count == d.V;  // not a Z-slab shard
  stage_mark(m, 0);
  if (m->stamps_dirty) {
    sdm_status rc = upload_stamps(m);
    if (rc != SDM_OK) return rc;
  }
  m->cur_depth = m->fa.depth;
  m->cur_cloud = m->fa.cloud;
  if (m->capturing) {
    // inside a graph a frame starts when the previous one is through: the first node writes both blocks, the member
    // count stays on the main stream (a detour over another queue costs more than its kernels)
    m->fb.set(d, m->st, m->sc, m->fa, true, whole);
    launch_frame_begin(m->fb, s);
    HIP_TRY(hipEventRecord(m->cap_begin, s));
    HIP_TRY(hipStreamWaitEvent(m->s_frustum, m->cap_begin, 0));
    HIP_TRY(hipStreamWaitEvent(m->s_birth, m->cap_begin, 0));
  } else {
    // The frustum reach set and the member count of the moving objects depend on the pose / the owner sets only,
    // which were final when the previous frame's births were done (ev_state): they get their own copy of the frame
    // block there and start - next to the previous frame's sweep when frames are issued back to back.
    // (recorded only where somebody waits for it: a marker between two launches of the main stream costs 2-3 us of the
    // frame - tools/probes/timers_frame_gaps.py - and a whole map's plain frames need none after the first)
    const bool side_chain_now = m->n_moves > 0 && (!whole || ((m->comm || m->ipc) && m->sharded_frame));
    if (!m->state_event_valid && (!m->vis_event_valid || side_chain_now)) {
      HIP_TRY(hipEventRecord(m->ev_state, s));
      m->state_event_valid = true;
    }
    // (the frustum chain reads the pose only; its bitmaps and flood flags are last read by the previous frame's
    // k_visibility: it starts behind THAT, a hundred microseconds before the births are done, and is off the path that
    // leads from one frame's sweep to the next frame's visibility pass)
    HIP_TRY(hipStreamWaitEvent(m->s_frustum, m->vis_event_valid ? m->ev_vis : m->ev_state, 0));
    launch_set_frame(m->d_fa[1], m->fa, m->s_frustum);
    HIP_TRY(hipEventRecord(m->ev_fa, m->s_frustum));
    if (whole && m->mv_pending) HIP_TRY(hipMemsetAsync(m->sc.mv_tot, 0, move_total_elems() * sizeof(uint32_t), s));
    m->fb.set(d, m->st, m->sc, m->fa, false, whole);
    // (ev_begin - the birth-candidate chain starts behind this kernel - rides on the launch itself, its packet's completion
    // signal, instead of a marker packet behind it: frame_begin -> k_move_apply 6.4 -> 3 us)
    launch_frame_begin(m->fb, s, !stage_done(stop_after, 5) ? m->ev_begin : nullptr);
    if (whole && m->n_moves > 0) m->mv_pending = true;
  }
  stage_mark(m, 1);
  if (stage_done(stop_after, 1)) return SDM_OK;

  // P2 (first part): collect the moving objects' particles (semantic_dsp_map.h:588-693); kernels of a frame without
  // moving objects return at once
  // (launch by launch the host knows that a frame has no moving objects / removals and skips those launches; inside a
  // graph they are always there and return at once)
  // (a whole map counts in k_frame_begin; a shard in a chain of its own, whose counts the all-gather below picks up)
  const bool side_chain = !m->capturing && m->n_moves > 0 && (!whole || ((m->comm || m->ipc) && m->sharded_frame));
  if (m->capturing) {
    if (!whole) launch_moves_count(d, m->st, m->sc, m->d_counts_local, s);
  } else if (side_chain) {
    // (its own copy of the frame block travels with its first kernel: nothing of another stream in front of the chain but
    // the previous frame's births)
    HIP_TRY(lazy_stream(m->device, &m->s_moves));
    HIP_TRY(hipStreamWaitEvent(m->s_moves, m->ev_state, 0));
    if (!whole) {
      if (m->mv_pending) HIP_TRY(hipMemsetAsync(m->sc.mv_tot, 0, move_total_elems() * sizeof(uint32_t), m->s_moves));
      launch_moves_count(d, m->st, m->sc, m->counts_local_user ? m->counts_local_user : m->d_counts_local, m->s_moves, &m->fa);
      m->mv_pending = true;
    }
    if ((m->comm || m->ipc) && m->sharded_frame) {
      // exchange 1 of a sharded frame rides the member-count stream: it runs beside the previous frame's sweep.  (Every
      // use of the communicator is ordered by events: this one behind the previous frame's births, the next one - the
      // export all-to-all on the main stream - behind ev_counts.)
      if (m->comm_timing) HIP_TRY(hipEventRecord(m->ev_comm[0], m->s_moves));
      {
        const sdm_status rc_ = exchange_counts(m, m->s_moves);
        if (rc_ != SDM_OK) return rc_;
      }
      if (m->comm_timing) {
        HIP_TRY(hipEventRecord(m->ev_comm[1], m->s_moves));
        m->comm_timed[0] = true;
      }
    }
    HIP_TRY(hipEventRecord(m->ev_counts, m->s_moves));
  }
  if (!stage_done(stop_after, 3)) {
    launch_frustum(d, m->sc, m->s_frustum);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(m->capturing ? m->cap_frustum : m->ev_frustum, m->s_frustum));
  } else if (!m->capturing) {
    // (parity debugging, stop_after <= 3) nothing else joins the side block's k_set_frame back: the next frame's first
    // kernel, which may write that block from the main stream, has to come after it
    HIP_TRY(hipStreamWaitEvent(s, m->ev_fa, 0));
  }
  if (!stage_done(stop_after, 5)) {
    // the birth candidates read this frame's cloud and the birth cursor: after this frame's k_frame_begin
    if (!m->capturing) HIP_TRY(hipStreamWaitEvent(m->s_birth, m->ev_begin, 0));  // (recorded by k_frame_begin's launch)
    m->birth_which = launch_birth_prepare(d, m->flt, m->bo, m->st, m->sc, m->s_birth);
    HIP_TRY(hipEventRecord(m->capturing ? m->cap_birth : m->ev_birth, m->s_birth));
  }
  if (side_chain) HIP_TRY(hipStreamWaitEvent(s, m->ev_counts, 0));  // join: the main stream picks the counts up
  m->state_event_valid = false;  // set again when this frame's births are done
  m->vis_event_valid = false;    // ... and when its visibility pass has been issued
  return SDM_OK;
}

sdm_status check_frame_args(sdm_map *m, const float *depth, const sdm_labeled_point *cloud, const float cam_pos[3], const float cam_q[4],
                            const sdm_object_move *moves, int32_t n_moves, const int32_t *remove_tracks, int32_t n_remove) {
  if (!m || !depth || !cloud || !cam_pos || !cam_q || n_moves < 0 || n_remove < 0 || (n_moves && !moves) || (n_remove && !remove_tracks)) {
    set_error("sdm_update", __FILE__, __LINE__, "null pointer or negative count");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  return SDM_OK;
}

// this frame's inputs -> device pointers in the frame block
sdm_status stage_inputs(sdm_map *m, const float *depth, const sdm_labeled_point *cloud, uint32_t flags) {
  const size_t hw = (size_t)m->d.W * m->d.H;
  if (flags & SDM_INPUT_ON_DEVICE) {
    m->fa.depth = depth;
    m->fa.cloud = cloud;
  } else {
    HIP_TRY(hipMemcpyAsync(m->d_depth, depth, hw * sizeof(float), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(m->d_cloud, cloud, hw * sizeof(sdm_labeled_point), hipMemcpyHostToDevice, m->stream));
    m->fa.depth = m->d_depth;
    m->fa.cloud = m->d_cloud;
  }
  return SDM_OK;
}

}  // namespace

sdm_status sdm_frame_start(sdm_map *m, const float *depth, const sdm_labeled_point *cloud, const float cam_pos[3],
                           const float cam_q[4], const sdm_object_move *moves, int32_t n_moves,
                           const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after) {
  sdm_status rc = check_frame_args(m, depth, cloud, cam_pos, cam_q, moves, n_moves, remove_tracks, n_remove);
  if (rc != SDM_OK) return rc;
  HIP_TRY(hipSetDevice(m->device));
  if ((rc = frame_host_prepare(m, cam_pos, cam_q, moves, n_moves, remove_tracks, n_remove, flags, stop_after)) != SDM_OK) return rc;
  if ((rc = stage_inputs(m, depth, cloud, flags)) != SDM_OK) return rc;
  m->n_direct_frames++;
  return frame_enqueue_start(m);
}

sdm_status sdm_frame_moves(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (stage_done(m->stop_after, SDM_STAGE_EGO)) return SDM_OK;
  if (!m->capturing) HIP_TRY(hipSetDevice(m->device));
  const int world = m->cfg.shard_count, rank = m->cfg.shard_rank;
  // without gathered counts (single shard, or the caller skipped exchange 1) the local counts are the global ones
  const int32_t *counts_all = m->counts_all_user;
  int w = world, r = rank;
  if (!counts_all) {
    counts_all = m->counts_local_user ? m->counts_local_user : m->d_counts_local;
    w = 1;
    r = 0;
  }
  if (m->capturing || m->n_moves > 0) {
    // (first call of the frame: the first batch, counted by sdm_frame_start; a later call on a shard: the batch the call
    // before prepared, whose counts the caller has exchanged meanwhile)
    launch_moves_transform(m->d, m->flt, m->st, m->sc, counts_all, w, r, m->stream);
    m->mv_pending = false;  // k_move_apply has reset the totals the next member count adds to
    m->mv_batch_ready = false;
    // the rest of a long object list, MAX_MOVE_OBJECTS at a time: the block's list is replaced (one launch that is also
    // the batch's member count), then its members are copied out and invalidated.  The reference takes ALL objects'
    // particles out before it re-inserts any (operations.h:321-362): so does this - k_move_replay comes after the last
    // batch - and the ranks, i.e. the noise draws and the insertion order, run on from batch to batch.
    const bool shard = m->d.v_count != m->d.V;
    while (m->mv_batch_next && m->mv_batch_next < m->moves_all.size()) {
      const size_t k0 = m->mv_batch_next;
      const int nb = (int)std::min<size_t>(MAX_MOVE_OBJECTS, m->moves_all.size() - k0);
      FrameArgs &fa = m->fa;
      memset(&fa.ms, 0, sizeof(fa.ms));
      fa.ms.n = nb;
      for (int k = 0; k < nb; ++k) {
        fa.ms.track[k] = (uint16_t)m->moves_all[k0 + k].track_id;
        memcpy(fa.ms.T[k], m->moves_all[k0 + k].T, 12 * sizeof(float));
      }
      fa.n_obj = nb;
      fa.mv_seq = ++m->mv_seq;
      fa.mv_batch += 1;
      m->mv_batch_next = k0 + MAX_MOVE_OBJECTS;
      launch_moves_batch(m->d, m->st, m->sc, fa, m->counts_local_user ? m->counts_local_user : m->d_counts_local, m->stream);
      if (shard) {
        // the batch's counts are published: the caller exchanges them (all-gather, like the first batch's) and calls again
        m->mv_batch_ready = true;
        return SDM_OK;
      }
      launch_moves_transform(m->d, m->flt, m->st, m->sc, counts_all, w, r, m->stream);
    }
    m->mv_batch_next = 0;
  }
  return SDM_OK;
}

sdm_status sdm_frame_moves_pending(sdm_map *m, int32_t *pending) {
  if (!m || !pending) return SDM_ERR_INVALID_ARGUMENT;
  *pending = m->mv_batch_ready ? 1 : 0;
  return SDM_OK;
}

sdm_status sdm_frame_predict(sdm_map *m, const float **ck_part_dev) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (m->mv_batch_ready) {
    set_error("sdm_frame_predict", __FILE__, __LINE__, "a batch of the frame's object list is still waiting for its counts: sdm_frame_moves_pending");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  const int stop_after = m->stop_after;
  if (stage_done(stop_after, SDM_STAGE_EGO)) return SDM_OK;
  if (!m->capturing) HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const Dims &d = m->d;
  // P2 (second part): re-insert the moved copies in the reference's order (operations.h:351-361)
  if (m->capturing || m->n_moves > 0)
    launch_moves_finish(d, m->flt, m->st, m->sc, m->counts_all_user ? m->cfg.shard_count : 1, m->cfg.shard_rank, s);
  stage_mark(m, 2);
  if (stage_done(stop_after, 2)) return SDM_OK;

  // P3: removals (semantic_dsp_map.h:702-736)
  if (m->capturing || m->n_remove > 0) launch_remove(d, m->st, m->sc, s);
  for (size_t k0 = MAX_REMOVE_TRACKS; k0 < m->removes_all.size(); k0 += MAX_REMOVE_TRACKS) {  // the rest of a long removal list
    FrameArgs &fa = m->fa;
    fa.n_remove = (int)std::min<size_t>(MAX_REMOVE_TRACKS, m->removes_all.size() - k0);
    for (int k = 0; k < fa.n_remove; ++k) fa.remove[k] = (uint16_t)m->removes_all[k0 + k];
    launch_set_frame(m->d_fa[0], fa, s);
    launch_remove(d, m->st, m->sc, s);
  }
  stage_mark(m, 3);
  if (stage_done(stop_after, 3)) return SDM_OK;

  // U1: visibility + binning (semantic_dsp_map.h:749); join the frustum stream first
  HIP_TRY(hipStreamWaitEvent(s, m->capturing ? m->cap_frustum : m->ev_frustum, 0));
  float *ck_dst = m->ck_user ? m->ck_user : m->d_ck_part;
  // (ev_vis: the next frame's frustum chain may overwrite what k_visibility read - recorded by that launch's own completion,
  // not by a marker behind the binning launches that follow it)
  launch_visibility(d, m->flt, m->st, m->sc, ck_dst, m->fused_ck ? 1 : 0, s, m->capturing ? nullptr : m->ev_vis);
  if (!m->capturing) m->vis_event_valid = true;
  stage_mark(m, 4);
  if (stage_done(stop_after, 4)) return SDM_OK;

  // U2 pass 1: this shard's ck partial sums
  launch_ck(d, m->flt, m->st, m->sc, ck_dst, m->fused_ck ? 1 : 0, s);
  if (ck_part_dev) *ck_part_dev = ck_dst;
  return SDM_OK;
}

sdm_status sdm_update_begin(sdm_map *m, const float *depth, const sdm_labeled_point *cloud, const float cam_pos[3],
                            const float cam_q[4], const sdm_object_move *moves, int32_t n_moves,
                            const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after,
                            const float **ck_part_dev) {
  sdm_status rc = sdm_frame_start(m, depth, cloud, cam_pos, cam_q, moves, n_moves, remove_tracks, n_remove, flags, stop_after);
  if (rc != SDM_OK) return rc;
  // no exchange between the steps: moved particles that leave this shard's slab are dropped (exact for one shard)
  const int32_t *keep_all = m->counts_all_user;
  m->counts_all_user = nullptr;
  rc = sdm_frame_moves(m);
  while (rc == SDM_OK && m->mv_batch_ready) rc = sdm_frame_moves(m);  // (a shard on its own: its local counts are all there is)
  if (rc == SDM_OK) rc = sdm_frame_predict(m, ck_part_dev);
  m->counts_all_user = keep_all;
  return rc;
}

// buffers of the two move exchanges (all device pointers, caller-owned):
//   counts_local  HALO_OBJ int32 written by sdm_frame_start      counts_all  shard_count x HALO_OBJ, gathered
//   send          shard_count segments of (16-byte header + cap_records x 36 B), written by sdm_frame_moves: segment d
//                 holds the copies whose target voxel lies in shard d's slab
//   recv_all      shard_count such segments, segment s = what shard s addressed to this one (all-to-all), read by
//                 sdm_frame_predict
sdm_status sdm_set_halo_buffers(sdm_map *m, int32_t *counts_local, const int32_t *counts_all, void *send, const void *recv_all,
                                int32_t cap_records) {
  if (!m || cap_records < 0) return SDM_ERR_INVALID_ARGUMENT;
  m->counts_local_user = counts_local;
  m->counts_all_user = counts_all;
  m->sc.halo_send = (unsigned char *)send;
  m->sc.halo_recv = (const unsigned char *)recv_all;
  m->sc.halo_cap = (uint32_t)cap_records;
  m->sc.halo_world = (uint32_t)m->cfg.shard_count;
  return SDM_OK;
}

// Second half: ck_kappa from the per-shard partial images (n_parts consecutive H*W images, slab order),
// weight update, births/resampling, occupancy sweep.
sdm_status sdm_update_finish(sdm_map *m, const float *ck_parts_dev, int32_t n_parts, uint32_t flags, int32_t stop_after) {
  if (!m || n_parts < 1) return SDM_ERR_INVALID_ARGUMENT;
  if (stage_done(stop_after, SDM_STAGE_VISIBILITY)) return SDM_OK;
  if (!m->capturing) HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const Dims &d = m->d;
  const float *own = m->ck_user ? m->ck_user : m->d_ck_part;
  // One image that is summed already (the chunk-owner exchange of a sharded map, or this shard's own image): pass 2 forms
  // ck + kappa itself from it (k_weight's ck_raw; the pixels' other operands were written by k_ck_classify) - no per-pixel
  // launch between the exchange and the weight update.  Several whole images (the one-collective exchange): k_ck_finish adds
  // them in slab order.
  const float *ck_raw = nullptr;
  if (!m->fused_ck) {
    if (!ck_parts_dev || n_parts == 1) ck_raw = ck_parts_dev ? ck_parts_dev : own;
    else launch_ck_finish(d, m->flt, m->sc, ck_parts_dev, n_parts, m->ck_part_stride, s);
  }
  m->ck_raw_last = ck_raw;
  m->ck_part_stride = 0;
  launch_weight(d, m->flt, m->st, m->sc, s, ck_raw);
  stage_mark(m, 5);
  if (stage_done(stop_after, 5)) return SDM_OK;
  HIP_TRY(hipStreamWaitEvent(s, m->capturing ? m->cap_birth : m->ev_birth, 0));  // join the birth-candidate stream
  launch_birth_replay(d, m->flt, m->st, m->sc, m->birth_which, m->global_time_stamp > 65535u, s);
  if (!m->capturing) {
    // ev_state: the particles are final here.  The member-count chain of a shard / a sharded frame starts behind it; a
    // whole map's plain frames have nobody waiting (frame_enqueue_start records it where it is needed after all)
    if (d.v_count != d.V || m->comm || m->ipc) {
      HIP_TRY(hipEventRecord(m->ev_state, s));
      m->state_event_valid = true;
    } else {
      m->state_event_valid = false;
    }
  }
  stage_mark(m, 6);
  if (stage_done(stop_after, 6)) return SDM_OK;
  if (!(flags & SDM_SKIP_OCCUPANCY)) {
    // (under capture nothing runs: the frame the graph is then launched for advances the epoch)
    launch_occupancy(d, m->flt, m->st, m->sc.cnt, m->sweep_all ? 1 : 0, m->sc.fa, next_epoch(m->f.epoch), s, sweep_mode(m));
    if (m->sweep_all) m->sweep_rec_pending = true;
    m->sweep_all = false;
    if (!m->capturing) m->sweep_epoch = next_epoch(m->f.epoch);
  }
  stage_mark(m, 7);
  return SDM_OK;
}

namespace {

// The frame as a graph: captured from the very launches above, instantiated once, replayed with the frame block as the
// one parameter that changes.  Two shapes.  Branched: the frustum chain and the birth-candidate chain keep their side
// streams and become branches.  Chain: their launches are issued on the main stream for the capture.  hipGraphLaunch of
// a chain of 40 kernel nodes costs the host 5 us, of the branched graph 78 us (ROCm 7.2: a graph with forks and joins is
// submitted piecewise, with synchronisation between the pieces) - against 105 us for issuing the launches one by one.
sdm_status graph_capture(sdm_map *m) {
  if (m->graph_exec) (void)hipGraphExecDestroy(m->graph_exec);
  if (m->graph) (void)hipGraphDestroy(m->graph);
  m->graph_exec = nullptr;
  m->graph = nullptr;
  m->graph_set_node = nullptr;
  // nothing of an earlier frame may still be running on the side streams when they join the capture
  HIP_TRY(hipStreamSynchronize(m->s_frustum));
  if (m->s_moves) HIP_TRY(hipStreamSynchronize(m->s_moves));
  HIP_TRY(hipStreamSynchronize(m->s_birth));
  m->sc.fa = m->d_fa[0];
  m->sc.fa_side = m->d_fa[1];
  m->capturing = true;
  hipStream_t side[3] = {m->s_frustum, m->s_birth, m->s_moves};
  // (under capture the member count of the moving objects is issued on the main stream, frame_enqueue_start)
  if (m->graph_shape == GRAPH_CHAIN) m->s_frustum = m->s_birth = m->stream;
  hipError_t e = hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal);
  sdm_status rc = SDM_OK;
  if (e == hipSuccess) {
    rc = frame_enqueue_start(m);
    if (rc == SDM_OK) rc = sdm_frame_moves(m);
    if (rc == SDM_OK) rc = sdm_frame_predict(m, nullptr);
    if (rc == SDM_OK) rc = sdm_update_finish(m, nullptr, 1, m->frame_flags, 0);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(m->stream, &g);
    m->graph = g;
  }
  m->s_frustum = side[0];
  m->s_birth = side[1];
  m->s_moves = side[2];
  m->capturing = false;
  if (e != hipSuccess || rc != SDM_OK || !m->graph) {
    set_error("hipStreamCapture", __FILE__, __LINE__, e != hipSuccess ? hipGetErrorString(e) : "frame enqueue failed under capture");
    (void)hipGetLastError();
    return rc != SDM_OK ? rc : SDM_ERR_HIP;
  }
  size_t n_nodes = 0;
  HIP_TRY(hipGraphGetNodes(m->graph, nullptr, &n_nodes));
  std::vector<hipGraphNode_t> nodes(n_nodes);
  HIP_TRY(hipGraphGetNodes(m->graph, nodes.data(), &n_nodes));
  for (hipGraphNode_t nd : nodes) {
    hipGraphNodeType t;
    if (hipGraphNodeGetType(nd, &t) != hipSuccess || t != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams kp;
    if (hipGraphKernelNodeGetParams(nd, &kp) == hipSuccess && kp.func == FrameBeginLaunch::kernel()) m->graph_set_node = nd;
  }
  if (!m->graph_set_node) {
    set_error("graph_capture", __FILE__, __LINE__, "frame-block node not found in the captured graph");
    return SDM_ERR_HIP;
  }
  HIP_TRY(hipGraphInstantiate(&m->graph_exec, m->graph, nullptr, nullptr, 0));
  m->graph_flt = m->flt;
  return SDM_OK;
}

sdm_status graph_launch(sdm_map *m) {
  m->fb.set(m->d, m->st, m->sc, m->fa, true, m->d.v_count == m->d.V);
  hipKernelNodeParams kp;
  memset(&kp, 0, sizeof(kp));
  kp.func = const_cast<void *>(FrameBeginLaunch::kernel());
  kp.gridDim = dim3(FrameBeginLaunch::GRID);
  kp.blockDim = dim3(FrameBeginLaunch::BLOCK);
  kp.sharedMemBytes = 0;
  kp.kernelParams = m->fb.argv;
  kp.extra = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipGraphExecKernelNodeSetParams(m->graph_exec, m->graph_set_node, &kp));
  const auto t1 = std::chrono::steady_clock::now();
  HIP_TRY(hipGraphLaunch(m->graph_exec, m->stream));
  if (m->host_timing) {
    m->t_setparams_us += std::chrono::duration<double, std::micro>(t1 - t0).count();
    m->t_launch_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
  }
  m->cur_depth = m->fa.depth;
  m->cur_cloud = m->fa.cloud;
  m->state_event_valid = false;  // ev_state was not recorded: the next plain frame forks from its own start
  m->vis_event_valid = false;
  m->sweep_all = false;
  m->sweep_epoch = next_epoch(m->f.epoch);
  m->n_graph_frames++;
  return SDM_OK;
}

// GRAPH_PIECES: the frame's kernels as five chain graphs.  Which kernels, in which order, on which stream and behind
// which event is exactly what frame_enqueue_start / sdm_frame_moves / sdm_frame_predict / sdm_update_finish issue for a
// plain frame (the member count of the moving objects on the main stream, as under capture); only k_frame_begin, whose
// argument is the frame block, is launched directly.  (A version that mirrors the launch-by-launch frame completely -
// member count as a sixth graph on its own stream, frustum and count chains started behind the previous frame's births -
// was measured: 0.34-0.35 instead of 0.36 ms on the GPU, but 115 instead of 60 us on the host.)
sdm_status pieces_capture(sdm_map *m) {
  for (hipGraphExec_t &g : m->piece) {
    if (g) (void)hipGraphExecDestroy(g);
    g = nullptr;
  }
  HIP_TRY(hipStreamSynchronize(m->s_frustum));
  if (m->s_moves) HIP_TRY(hipStreamSynchronize(m->s_moves));
  HIP_TRY(hipStreamSynchronize(m->s_birth));
  m->sc.fa = m->d_fa[0];
  m->sc.fa_side = m->d_fa[1];
  const Dims &d = m->d;
  auto capture = [&](hipStream_t st, int which, auto &&body) -> sdm_status {
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    body(st);
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(st, &g);
    if (e != hipSuccess || !g) {
      set_error("hipStreamEndCapture", __FILE__, __LINE__, e != hipSuccess ? hipGetErrorString(e) : "no graph");
      (void)hipGetLastError();
      return SDM_ERR_HIP;
    }
    e = hipGraphInstantiate(&m->piece[which], g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) {
      set_error("hipGraphInstantiate", __FILE__, __LINE__, hipGetErrorString(e));
      return SDM_ERR_HIP;
    }
    return SDM_OK;
  };
  // (every launch is issued, also those a launch-by-launch frame skips when the host knows there is nothing to move or
  // remove: the kernels check on the device and return)
  sdm_status rc = capture(m->s_frustum, 0, [&](hipStream_t st) { launch_frustum(d, m->sc, st); });
  if (rc == SDM_OK)
    rc = capture(m->s_birth, 1, [&](hipStream_t st) { m->birth_which = launch_birth_prepare(d, m->flt, m->bo, m->st, m->sc, st); });
  if (rc == SDM_OK)
    rc = capture(m->stream, 2, [&](hipStream_t st) {
      if (d.v_count != d.V) launch_moves_count(d, m->st, m->sc, m->d_counts_local, st);  // (a whole map counts in k_frame_begin)
      launch_moves_transform(d, m->flt, m->st, m->sc, m->d_counts_local, 1, 0, st);
      launch_moves_finish(d, m->flt, m->st, m->sc, 1, m->cfg.shard_rank, st);
      launch_remove(d, m->st, m->sc, st);
    });
  if (rc == SDM_OK)
    rc = capture(m->stream, 3, [&](hipStream_t st) {
      launch_visibility(d, m->flt, m->st, m->sc, m->d_ck_part, 1, st);
      launch_ck(d, m->flt, m->st, m->sc, m->d_ck_part, 1, st);
      launch_weight(d, m->flt, m->st, m->sc, st);
    });
  if (rc == SDM_OK)
    rc = capture(m->stream, 4, [&](hipStream_t st) {
      launch_birth_replay(d, m->flt, m->st, m->sc, m->birth_which, false, st);
      launch_occupancy(d, m->flt, m->st, m->sc.cnt, 0, m->sc.fa, 0, st);
    });
  m->graph_flt = m->flt;
  return rc;
}

sdm_status pieces_launch(sdm_map *m) {
  hipStream_t s = m->stream;
  const auto t0 = std::chrono::steady_clock::now();
  m->fb.set(m->d, m->st, m->sc, m->fa, true, m->d.v_count == m->d.V);  // k_frame_begin writes both copies of the frame block
  launch_frame_begin(m->fb, s);
  HIP_TRY(hipEventRecord(m->ev_begin, s));
  HIP_TRY(hipStreamWaitEvent(m->s_frustum, m->ev_begin, 0));
  HIP_TRY(hipGraphLaunch(m->piece[0], m->s_frustum));
  HIP_TRY(hipEventRecord(m->ev_frustum, m->s_frustum));
  HIP_TRY(hipStreamWaitEvent(m->s_birth, m->ev_begin, 0));
  HIP_TRY(hipGraphLaunch(m->piece[1], m->s_birth));
  HIP_TRY(hipEventRecord(m->ev_birth, m->s_birth));
  HIP_TRY(hipGraphLaunch(m->piece[2], s));
  HIP_TRY(hipStreamWaitEvent(s, m->ev_frustum, 0));
  HIP_TRY(hipGraphLaunch(m->piece[3], s));
  HIP_TRY(hipStreamWaitEvent(s, m->ev_birth, 0));
  HIP_TRY(hipGraphLaunch(m->piece[4], s));
  if (m->host_timing) m->t_launch_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  m->cur_depth = m->fa.depth;
  m->cur_cloud = m->fa.cloud;
  m->state_event_valid = false;
  m->vis_event_valid = false;
  m->sweep_all = false;
  m->sweep_epoch = next_epoch(m->f.epoch);
  m->n_graph_frames++;
  return SDM_OK;
}

}  // namespace

// Development aid (tools/probes/modes.py): a 60 us spin on the main stream, a stamp right behind it on side stream
// `which` (0 frustum, 1 birth candidates, 2 member count).  out_us[0] = stamp - spin start, out_us[1] = spin length.
extern "C" sdm_status sdm_debug_overlap(sdm_map *m, int32_t which, double out_us[2]) {
  if (!m || which < 0 || which > 2 || !out_us) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  unsigned long long *d = nullptr, h[3] = {0, 0, 0};
  HIP_TRY(hipMalloc(&d, sizeof(h)));
  if (which == 2) HIP_TRY(lazy_stream(m->device, &m->s_moves));
  hipStream_t side = which == 0 ? m->s_frustum : (which == 1 ? m->s_birth : m->s_moves);
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipStreamSynchronize(side));
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, m->stream, 6000ull, d);
  hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, side, d + 2);
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipStreamSynchronize(side));
  HIP_TRY(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  out_us[0] = ((double)h[2] - (double)h[0]) / 100.0;
  out_us[1] = ((double)h[1] - (double)h[0]) / 100.0;
  return SDM_OK;
}

sdm_status sdm_set_issue_mode(sdm_map *m, int32_t mode) {
  if (!m || mode < 0 || mode > 4) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  const bool use = mode == 2 ? m->enqueue_us > GRAPH_PIECES_US : mode != 0;
  const int shape = mode == 1 ? GRAPH_BRANCHED
                    : mode == 3 ? GRAPH_CHAIN
                    : mode == 2 ? (m->enqueue_us > GRAPH_CHAIN_US ? GRAPH_CHAIN : GRAPH_PIECES)
                                : GRAPH_PIECES;
  if (shape != m->graph_shape) {
    // the branched graph and the chain share one executable: whatever was captured for the old shape goes
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (m->graph_exec) (void)hipGraphExecDestroy(m->graph_exec);
    if (m->graph) (void)hipGraphDestroy(m->graph);
    m->graph_exec = nullptr;
    m->graph = nullptr;
    m->graph_set_node = nullptr;
    for (hipGraphExec_t &g : m->piece) {
      if (g) (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
  }
  m->graph_mode = mode;
  m->use_graph = use;
  m->graph_shape = shape;
  return SDM_OK;
}

sdm_status sdm_update(sdm_map *m, const float *depth, const sdm_labeled_point *cloud, const float cam_pos[3],
                      const float cam_q[4], const sdm_object_move *moves, int32_t n_moves, const int32_t *remove_tracks,
                      int32_t n_remove, uint32_t flags, int32_t stop_after) {
  sdm_status rc = check_frame_args(m, depth, cloud, cam_pos, cam_q, moves, n_moves, remove_tracks, n_remove);
  if (rc != SDM_OK) return rc;
  HIP_TRY(hipSetDevice(m->device));
  m->fused_ck = true;
  const auto tp0 = std::chrono::steady_clock::now();
  rc = frame_host_prepare(m, cam_pos, cam_q, moves, n_moves, remove_tracks, n_remove, flags, stop_after);
  if (rc == SDM_OK) rc = stage_inputs(m, depth, cloud, flags);
  if (m->host_timing) m->t_prepare_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tp0).count();
  if (rc != SDM_OK) {
    m->fused_ck = false;
    return rc;
  }
  // A plain frame - whole map on this GPU, every stage, incremental sweep, nobody timing stages or owning the stream -
  // is replayed from the graph; everything else takes the launches one by one.
  const bool would_be_plain = stop_after == 0 && (flags & ~(uint32_t)SDM_INPUT_ON_DEVICE) == 0 && !m->profiling &&
                              m->cfg.shard_count == 1 && !m->comm && !m->ck_user && !m->counts_local_user &&
                              m->stream == m->own_stream && !m->sweep_all && !m->stamps_dirty &&
                              n_moves <= MAX_MOVE_OBJECTS && n_remove <= MAX_REMOVE_TRACKS &&  // (longer lists: batches, launch by launch)
                              m->global_time_stamp <= 65535u;  // (beyond: the literal birth replay, not in the captured graphs)
  const bool plain = m->use_graph && would_be_plain;
  if (plain) {
    const bool pieces = m->graph_shape == GRAPH_PIECES;
    bool have = pieces ? m->piece[4] != nullptr : m->graph_exec != nullptr;
    if (have && memcmp(&m->graph_flt, &m->flt, sizeof(Filter)) != 0) have = false;  // sdm_set_params / a new noise table since
    if (!have) {
      const auto tc = std::chrono::steady_clock::now();
      rc = pieces ? pieces_capture(m) : graph_capture(m);
      if (m->host_timing)
        fprintf(stderr, "sdm host timing: graph capture + instantiate %.0f us (%s)\n",
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tc).count(),
                pieces ? "pieces" : (m->graph_shape == GRAPH_CHAIN ? "chain" : "branched"));
    }
    bool direct = false;
    if (rc != SDM_OK) {
      // the capture failed: nothing of this frame has been enqueued yet, so it takes the plain launches (as every later
      // frame does)
      m->use_graph = false;
      direct = true;
      rc = SDM_OK;
    } else {
      rc = pieces ? pieces_launch(m) : graph_launch(m);
      if (rc != SDM_OK) {
        // a launch failed in mid-frame: the host's ring state has moved on, the device may not have got this frame's slab
        // stamps - the next frame uploads them wholesale and sweeps every voxel
        m->use_graph = false;
        m->stamps_dirty = true;
        m->sweep_all = true;
      }
    }
    if (direct) {
      m->n_direct_frames++;
      rc = frame_enqueue_start(m);
      if (rc == SDM_OK) rc = sdm_frame_moves(m);
      if (rc == SDM_OK) rc = sdm_frame_predict(m, nullptr);
      if (rc == SDM_OK) rc = sdm_update_finish(m, nullptr, 1, flags, stop_after);
    }
  } else {
    m->n_direct_frames++;
    const auto t0 = std::chrono::steady_clock::now();
    rc = frame_enqueue_start(m);
    if (rc == SDM_OK) rc = sdm_frame_moves(m);
    if (rc == SDM_OK) rc = sdm_frame_predict(m, nullptr);
    if (rc == SDM_OK) rc = sdm_update_finish(m, nullptr, 1, flags, stop_after);
    if (m->host_timing) m->t_direct_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  }
  m->fused_ck = false;
  return rc;
}

// SURVEY.md row N1 on the device: masks + depth -> LabeledPoint image, then the usual frame on device-resident inputs.
sdm_status sdm_update_raw(sdm_map *m, const float *depth, const uint8_t *static_mask, const uint16_t label_to_static_instance[256],
                          const sdm_instance_mask *objects, int32_t n_objects, const double cam_pos[3], const double cam_q[4],
                          const sdm_object_move *moves, int32_t n_moves, const int32_t *remove_tracks, int32_t n_remove,
                          uint32_t flags, int32_t stop_after) {
  return sdm_update_raw_ex(m, depth, static_mask, label_to_static_instance, objects, n_objects, cam_pos, cam_q, moves, n_moves,
                           remove_tracks, n_remove, flags, stop_after, nullptr);
}

sdm_status sdm_update_raw_ex(sdm_map *m, const float *depth, const uint8_t *static_mask,
                             const uint16_t label_to_static_instance[256], const sdm_instance_mask *objects, int32_t n_objects,
                             const double cam_pos[3], const double cam_q[4], const sdm_object_move *moves, int32_t n_moves,
                             const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after,
                             const sdm_raw_options *opt) {
  if (!m || !depth || !cam_pos || !cam_q || n_objects < 0 || n_objects > MAX_CLOUD_OBJECTS || (n_objects && !objects) ||
      (static_mask && !label_to_static_instance))
    return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const Dims &d = m->d;
  const size_t hw = (size_t)d.W * d.H;
  const bool on_dev = (flags & SDM_INPUT_ON_DEVICE) != 0;
  const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // BOOST mode: the inputs arrive at the sensor's size and are reduced with manualResize first
  const bool resize = opt && opt->src_width > 0;
  size_t src_hw = hw;
  if (resize) {
    if (opt->src_height <= 0 || !(opt->rescale > 0.f) || (int)((float)opt->src_height * opt->rescale) != d.H ||
        (int)((float)opt->src_width * opt->rescale) != d.W) {
      set_error("sdm_update_raw_ex", __FILE__, __LINE__, "int(src size * rescale) must equal the configured image size");
      return SDM_ERR_INVALID_ARGUMENT;
    }
    src_hw = (size_t)opt->src_width * opt->src_height;
    if (!on_dev && src_hw * 4 > m->src_stage_bytes) {
      HIP_TRY(hipStreamSynchronize(s));
      if (m->d_src_stage) HIP_TRY(hipFree(m->d_src_stage));
      m->d_src_stage = nullptr;
      HIP_TRY(dev_alloc(&m->d_src_stage, src_hw * 4));
      m->src_stage_bytes = src_hw * 4;
    }
  }
  // this frame's input set; the copy stream may fill it as soon as the frame that last read it is through
  sdm_map::RawInputs &in = m->raw[m->raw_next];
  m->raw_next ^= 1;
  HIP_TRY(lazy_stream(m->device, &m->s_copy));
  hipStream_t sc_ = m->s_copy;
  HIP_TRY(hipStreamWaitEvent(sc_, in.ev_free, 0));
  // one input image -> its device buffer of the configured size
  auto stage_in = [&](const void *src, void *dst, int elem) -> sdm_status {
    if (!resize) {
      HIP_TRY(hipMemcpyAsync(dst, src, hw * elem, kind, sc_));
      return SDM_OK;
    }
    const void *src_dev = src;
    if (!on_dev) {
      HIP_TRY(hipMemcpyAsync(m->d_src_stage, src, src_hw * elem, hipMemcpyHostToDevice, sc_));
      src_dev = m->d_src_stage;
    }
    launch_manual_resize(d, src_dev, dst, opt->src_width, opt->src_height, opt->rescale, elem, sc_);
    return SDM_OK;
  };
  if (n_objects > in.obj_masks_cap) {
    HIP_TRY(hipStreamSynchronize(sc_));
    if (in.obj_masks) HIP_TRY(hipFree(in.obj_masks));
    in.obj_masks = nullptr;
    HIP_TRY(dev_alloc(&in.obj_masks, hw * n_objects));
    in.obj_masks_cap = n_objects;
  }
  // (every argument is looked at before the first copy is queued, and every exit behind the first copy goes through the
  // epilogue below that waits for the copy stream: the caller's buffers are its own again when this returns, also when it
  // returns an error - the adapter rewrites its page-locked depth and mask buffers in place for the next update())
  for (int k = 0; k < n_objects; ++k)
    if (!objects[k].mask) {
      set_error("sdm_update_raw_ex", __FILE__, __LINE__, "objects[k].mask is null");
      return SDM_ERR_INVALID_ARGUMENT;
    }
  auto queue_and_run = [&]() -> sdm_status {
  sdm_status rc;
  const float *depth_dev = depth;
  if (!on_dev || resize) {
    if ((rc = stage_in(depth, in.depth, 4)) != SDM_OK) return rc;
    depth_dev = in.depth;
  }
  if (static_mask) {
    if ((rc = stage_in(static_mask, in.static_mask, 1)) != SDM_OK) return rc;
    if (!in.label_valid || memcmp(in.label_host, label_to_static_instance, 512) != 0) {
      memcpy(in.label_host, label_to_static_instance, 512);
      HIP_TRY(hipMemcpyAsync(in.label_to_inst, in.label_host, 512, hipMemcpyHostToDevice, sc_));
      in.label_valid = true;
    }
  }
  CloudArgsHost a;
  memset(&a, 0, sizeof(a));
  // masks that lie back to back in the caller's memory (the adapter's do) go up as one transfer
  bool masks_contiguous = !resize && n_objects > 1;
  for (int k = 0; k < n_objects; ++k) {
    if (k && objects[k].mask != objects[k - 1].mask + hw) masks_contiguous = false;
    a.track[k] = objects[k].track_id;
    a.label[k] = objects[k].label_id;
  }
  if (masks_contiguous) {
    HIP_TRY(hipMemcpyAsync(in.obj_masks, objects[0].mask, hw * (size_t)n_objects, kind, sc_));
  } else {
    for (int k = 0; k < n_objects; ++k)
      if ((rc = stage_in(objects[k].mask, in.obj_masks + hw * k, 1)) != SDM_OK) return rc;
  }
  a.sky_instance = opt ? opt->sky_instance : -1;
  a.has_bbox = opt && opt->object_bbox && n_objects > 0 ? 1 : 0;
  if (a.has_bbox) HIP_TRY(hipMemcpyAsync(in.bbox, opt->object_bbox, sizeof(double) * 6 * n_objects, hipMemcpyHostToDevice, sc_));
  HIP_TRY(hipEventRecord(m->ev_copy, sc_));
  HIP_TRY(hipStreamWaitEvent(s, m->ev_copy, 0));
  // Eigen's Quaternion::toRotationMatrix in double (pointcloud_tools.h:107-110)
  {
    const double w = cam_q[0], x = cam_q[1], y = cam_q[2], z = cam_q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    a.R[0] = 1.0 - (tyy + tzz);
    a.R[1] = txy - twz;
    a.R[2] = txz + twy;
    a.R[3] = txy + twz;
    a.R[4] = 1.0 - (txx + tzz);
    a.R[5] = tyz - twx;
    a.R[6] = txz - twy;
    a.R[7] = tyz + twx;
    a.R[8] = 1.0 - (txx + tyy);
  }
  for (int k = 0; k < 3; ++k) a.t[k] = cam_pos[k];
  a.ifx = 1.0 / (double)d.fx;
  a.icx = -(double)d.cx / (double)d.fx;
  a.ify = 1.0 / (double)d.fy;
  a.icy = -(double)d.cy / (double)d.fy;
  a.dmin = (double)d.dmin;
  a.dmax = (double)d.dmax;
  a.sigma0 = m->prm.depth_noise_zero_order;
  a.sigma1 = m->prm.depth_noise_first_order;
  a.consider_depth_noise = m->prm.if_consider_depth_noise ? 1 : 0;
  a.consider_instance = (flags & SDM_NO_INSTANCES) ? 0 : 1;
  a.n_objects = n_objects;
  a.has_static = static_mask ? 1 : 0;
  launch_labeled_cloud(d, a, depth_dev, in.static_mask, in.label_to_inst, in.obj_masks, in.bbox, m->d_cloud, s);
  const float posf[3] = {(float)cam_pos[0], (float)cam_pos[1], (float)cam_pos[2]};       // semantic_dsp_map.h:584
  const float qf[4] = {(float)cam_q[0], (float)cam_q[1], (float)cam_q[2], (float)cam_q[3]};  // :745
  return sdm_update(m, depth_dev, m->d_cloud, posf, qf, moves, n_moves, remove_tracks, n_remove, flags | SDM_INPUT_ON_DEVICE,
                    stop_after);
  };
  sdm_status rc = queue_and_run();
  (void)hipEventRecord(in.ev_free, s);
  // host buffers belong to the caller again when this returns (nothing is retained): wait for the copies, which ran
  // while the frame's launches were issued above
  if (!on_dev) {
    const hipError_t ce = hipStreamSynchronize(sc_);
    if (ce != hipSuccess && rc == SDM_OK) {
      set_error("hipStreamSynchronize(copy stream)", __FILE__, __LINE__, hipGetErrorString(ce));
      rc = SDM_ERR_HIP;
    }
  }
  return rc;
}

sdm_status sdm_get_labeled_cloud(sdm_map *m, sdm_labeled_point *out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(out, m->cur_cloud, (size_t)m->d.W * m->d.H * sizeof(sdm_labeled_point), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

sdm_status sdm_synchronize(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  if (m->comm) {
    // A sharded frame ends in collectives that only finish when every shard has issued its own: a shard that died or fell
    // out of step leaves the others waiting for ever.  The wait is therefore bounded (SDM_COMM_TIMEOUT_MS, 30 s): past it
    // the communicator is aborted - which releases the stream - and the caller gets SDM_ERR_COMM instead of a hang.
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
  } else {
    HIP_TRY(hipStreamSynchronize(m->s_frustum));
    HIP_TRY(hipStreamSynchronize(m->s_birth));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  return check_counters(m, nullptr);
}

sdm_status sdm_set_stream(sdm_map *m, void *hip_stream) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->stream = hip_stream ? (hipStream_t)hip_stream : m->own_stream;
  return SDM_OK;
}

sdm_status sdm_set_ck_buffer(sdm_map *m, float *dev_buffer) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->ck_user = dev_buffer;
  return SDM_OK;
}

sdm_status sdm_stream(sdm_map *m, void **stream_out) {
  if (!m || !stream_out) return SDM_ERR_INVALID_ARGUMENT;
  *stream_out = (void *)m->stream;
  return SDM_OK;
}

// ---- multi-GPU: RCCL over xGMI, one process per GPU ---------------------------------------------
// The reference is one process and one thread; these collectives are new.  Rendezvous (handing the
// 128-byte id of rank 0 to the other ranks) is the caller's business (bench.py uses torch.distributed/gloo for it).
#define NCCL_TRY(expr)                                                       \
  do {                                                                       \
    ncclResult_t r_ = (expr);                                                \
    if (r_ != ncclSuccess) {                                                 \
      set_error(#expr, __FILE__, __LINE__, ncclGetErrorString(r_));          \
      return SDM_ERR_COMM;                                                   \
    }                                                                        \
  } while (0)

sdm_status sdm_comm_unique_id(uint8_t out[128]) {
  if (!out) return SDM_ERR_INVALID_ARGUMENT;
  static_assert(NCCL_UNIQUE_ID_BYTES == 128, "id size");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(out, id.internal, 128);
  return SDM_OK;
}

sdm_status sdm_comm_init(sdm_map *m, const uint8_t id_bytes[128], int32_t halo_cap_records) {
  if (!m || !id_bytes || halo_cap_records < 0 || m->comm) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  const int world = m->cfg.shard_count, rank = m->cfg.shard_rank;
  ncclUniqueId id;
  memcpy(id.internal, id_bytes, 128);
  NCCL_TRY(ncclCommInitRank(&m->comm, world, id, rank));
  m->halo_cap_own = halo_cap_records > 0 ? (uint32_t)halo_cap_records : (uint32_t)SDM_HALO_DEFAULT_CAP;
  const size_t hb = halo_segment_bytes(m->halo_cap_own) * (size_t)world;
  const size_t ck_elems = (size_t)m->ck_chunk * world;
  HIP_TRY(dev_alloc(&m->d_counts_all, (size_t)world * HALO_OBJ));
  HIP_TRY(dev_alloc(&m->d_halo_send, hb));
  HIP_TRY(dev_alloc(&m->d_halo_recv, hb));
  HIP_TRY(dev_alloc(&m->d_ck_stage, ck_elems));
  HIP_TRY(dev_alloc(&m->d_ck_full, ck_elems));
  HIP_TRY(hipMemsetAsync(m->d_halo_send, 0, hb, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_halo_recv, 0, hb, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_stage, 0, ck_elems * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_full, 0, ck_elems * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_part, 0, ck_elems * 4, m->stream));
  for (hipEvent_t &e : m->ev_comm) HIP_TRY(hipEventCreate(&e));
  {
    // how the partial ck images are combined (sdm_update_sharded; both give the slab-ordered float sums the oracle's
    // `ck_slabs` forms): SDM_CK_EXCHANGE=allgather for the one-collective variant, sdm_comm_set_options at run time
    const char *e = getenv("SDM_CK_EXCHANGE");
    if (e && !strcmp(e, "allgather")) m->ck_exchange = 1;
    const char *t = getenv("SDM_COMM_TIMEOUT_MS");
    if (t && atoi(t) > 0) m->comm_timeout_ms = atoi(t);
  }
  HIP_TRY(dev_alloc(&m->d_ck_all, ck_elems * (size_t)world));
  HIP_TRY(hipMemsetAsync(m->d_ck_all, 0, ck_elems * (size_t)world * 4, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return sdm_set_halo_buffers(m, m->d_counts_local, m->d_counts_all, m->d_halo_send, m->d_halo_recv, (int32_t)m->halo_cap_own);
}

// The exchanges without RCCL.  sdm_ipc_create allocates this shard's receive arena (fine-grained device memory where the
// runtime hands out an IPC handle for it: peers write into it while this GPU's kernels poll its flags; SDM_IPC_ALLOC=coarse
// forces plain device memory) and returns its hipIpc handle; the caller hands the handles of all shards round (64 bytes
// each, any transport) and sdm_ipc_connect maps the peers' arenas.  sdm_update_sharded then uses them.
sdm_status sdm_ipc_create(sdm_map *m, int32_t halo_cap_records, uint8_t handle_out[64]) {
  if (!m || !handle_out || halo_cap_records < 0 || m->comm || m->ipc_arena) return SDM_ERR_INVALID_ARGUMENT;
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
  if (!have) {
    HIP_TRY(hipMalloc(&p, m->ipc_bytes));
    HIP_TRY(hipIpcGetMemHandle(&h, p));
  }
  m->ipc_arena = (unsigned char *)p;
  if (getenv("SDM_IPC_VERBOSE"))
    fprintf(stderr, "sdm_ipc_create: shard %d of %d, arena %zu bytes, %s device memory\n", m->cfg.shard_rank, world, m->ipc_bytes,
            m->ipc_fine_grained ? "fine-grained" : "coarse-grained");
  HIP_TRY(hipMemsetAsync(p, 0, m->ipc_bytes, m->stream));
  // the frame's exchange buffers are regions of the arena; the export segments stay local (pushed by the exchange kernel)
  HIP_TRY(dev_alloc(&m->d_counts_all_local, (size_t)world * HALO_OBJ));
  HIP_TRY(dev_alloc(&m->d_ck_full_local, (size_t)world * m->ck_chunk));
  HIP_TRY(dev_alloc(&m->d_ipc_sync, 32));
  HIP_TRY(hipMemsetAsync(m->d_counts_all_local, 0, (size_t)world * HALO_OBJ * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_full_local, 0, (size_t)world * m->ck_chunk * 4, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ipc_sync, 0, 32 * 4, m->stream));
  m->d_counts_all = m->d_counts_all_local;  // (k_move_apply reads the rows from there: the exchange copies them on)
  m->d_halo_recv = m->ipc_arena + m->ipc_off_halo;
  m->d_ck_stage = (float *)(m->ipc_arena + m->ipc_off_stage);
  m->d_ck_full = (float *)(m->ipc_arena + m->ipc_off_full);
  HIP_TRY(dev_alloc(&m->d_halo_send, seg * (size_t)world));
  HIP_TRY(hipMemsetAsync(m->d_halo_send, 0, seg * (size_t)world, m->stream));
  HIP_TRY(hipMemsetAsync(m->d_ck_part, 0, (size_t)m->ck_chunk * world * 4, m->stream));
  for (hipEvent_t &e : m->ev_comm) HIP_TRY(hipEventCreate(&e));
  {
    const char *t = getenv("SDM_COMM_TIMEOUT_MS");
    if (t && atoi(t) > 0) m->comm_timeout_ms = atoi(t);
  }
  HIP_TRY(hipStreamSynchronize(m->stream));
  memcpy(handle_out, &h, 64);
  return sdm_set_halo_buffers(m, m->d_counts_local, m->d_counts_all, m->d_halo_send, m->d_halo_recv, (int32_t)m->halo_cap_own);
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

namespace {
// one exchange through the peers' arenas (k_ipc_exchange): kind, where this shard's pieces lie, where they land
sdm_status ipc_exchange(sdm_map *m, uint32_t kind, const void *src, size_t src_stride, size_t dst_off, size_t dst_stride, size_t piece_bytes,
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
sdm_status all_to_all(sdm_map *m, const void *send, void *recv, size_t piece_bytes, hipStream_t s) {
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

// ---- plain device buffers for callers that keep their frames resident in HBM (SDM_INPUT_ON_DEVICE) ----
sdm_status sdm_device_alloc(sdm_map *m, size_t bytes, void **out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return SDM_OK;
}
sdm_status sdm_device_free(sdm_map *m, void *p) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipFree(p));
  return SDM_OK;
}
sdm_status sdm_device_upload(sdm_map *m, void *dst_dev, const void *src_host, size_t bytes) {
  if (!m || !dst_dev || !src_host) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}
sdm_status sdm_device_download(sdm_map *m, void *dst_host, const void *src_dev, size_t bytes) {
  if (!m || !dst_host || !src_dev) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}
sdm_status sdm_device_synchronize(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipDeviceSynchronize());
  return SDM_OK;
}

// ---- results ----------------------------------------------------------------------------------
sdm_status sdm_get_voxels(sdm_map *m, sdm_voxel_result *out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(out, m->st.res, (size_t)m->d.v_count * sizeof(sdm_voxel_result), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

// A result list comes back in one round trip when its length can be guessed: the length and the first `emit_guess`
// points are copied to page-locked memory behind the kernels, one wait, and only a list that outgrew the guess needs a
// second copy.  (The length first, then the points: two waits, 30 us each way, and a pageable destination.)
constexpr size_t EMIT_STAGE_MAX = (size_t)64 << 20;
static sdm_status fetch_points(sdm_map *m, const void *d_points_v, void *out_v, size_t elem, size_t cap, size_t *n_out) {
  const unsigned char *d_points = static_cast<const unsigned char *>(d_points_v);
  unsigned char *out = static_cast<unsigned char *>(out_v);
  size_t guess = std::min(cap, m->emit_guess);
  if (16 + guess * elem > EMIT_STAGE_MAX) guess = (EMIT_STAGE_MAX - 16) / elem;
  const size_t need = 16 + guess * elem;
  if (need > m->h_emit_bytes) {  // (page-locking memory takes a third of a millisecond: grown in big steps)
    const size_t grown = std::min(EMIT_STAGE_MAX, std::max(need * 2, (size_t)1 << 20));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (m->h_emit) HIP_TRY(hipHostFree(m->h_emit));
    m->h_emit = nullptr;
    m->h_emit_bytes = 0;
    HIP_TRY(hipHostMalloc((void **)&m->h_emit, grown, hipHostMallocDefault));
    m->h_emit_bytes = grown;
  }
  HIP_TRY(hipMemcpyAsync(m->h_emit, m->emit.total, 4, hipMemcpyDeviceToHost, m->stream));
  if (guess) HIP_TRY(hipMemcpyAsync(m->h_emit + 16, d_points, guess * elem, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  uint32_t total = 0;
  memcpy(&total, m->h_emit, 4);
  *n_out = total;
  const size_t ncopy = std::min<size_t>(total, cap), first = std::min(ncopy, guess);
  if (first) memcpy(out, m->h_emit + 16, first * elem);
  if (ncopy > first) {
    HIP_TRY(hipMemcpyAsync(out + first * elem, d_points + first * elem, (ncopy - first) * elem, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
  }
  m->emit_guess = (size_t)total + total / 4 + 1024;
  return SDM_OK;
}

static sdm_status get_points(sdm_map *m, sdm_point *out, size_t cap, size_t *n_out, int flags, int want_free) {
  if (!m || !n_out || (cap && !out)) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  if (cap > m->points_cap) {
    if (m->d_points) HIP_TRY(hipFree(m->d_points));
    m->d_points = nullptr;
    HIP_TRY(dev_alloc(&m->d_points, cap));
    m->points_cap = cap;
  }
  // visualize_with_zero_center: subtract the camera position (semantic_dsp_map.h:1263-1271)
  float sub[3] = {0.f, 0.f, 0.f};
  if (flags & SDM_POINTS_ZERO_CENTER)
    for (int a = 0; a < 3; ++a) sub[a] = m->cam_p[a];
  uint32_t cap32 = (uint32_t)std::min<size_t>(cap, 0xffffffffu);
  launch_emit_points(m->d, m->f, m->st, m->emit, m->d_points, cap32, want_free, sub, (flags & SDM_POINTS_MARK_FOV) ? 1 : 0, m->stream);
  return fetch_points(m, m->d_points, out, sizeof(sdm_point), cap, n_out);
}
sdm_status sdm_get_occupied(sdm_map *m, sdm_point *out, size_t cap, size_t *n_out, int32_t flags) {
  return get_points(m, out, cap, n_out, flags, 0);
}
sdm_status sdm_get_freespace(sdm_map *m, sdm_point *out, size_t cap, size_t *n_out, int32_t flags) {
  return get_points(m, out, cap, n_out, flags, 1);
}
// ---- N2: coloured, packed lists
sdm_status sdm_set_colours(sdm_map *m, const sdm_colour_config *c) {
  if (!m || !c) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  ColourTables t;
  memset(&t, 0, sizeof(t));
  t.cfg = *c;
  // RGB2HSV_b's tables (OpenCV imgproc color_hsv: hsv_shift 12): cvRound = round half to even
  for (int i = 1; i < 256; ++i) {
    t.sdiv[i] = (int32_t)nearbyint((double)(255 << 12) / (1.0 * i));
    t.hdiv180[i] = (int32_t)nearbyint((double)(180 << 12) / (6.0 * i));
  }
  if (!m->d_colours) HIP_TRY(dev_alloc(&m->d_colours, 1));
  HIP_TRY(hipMemcpyAsync(m->d_colours, &t, sizeof(t), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->colours_set = true;
  return SDM_OK;
}

static sdm_status get_points_rgb(sdm_map *m, sdm_point_xyzrgb *out, size_t cap, size_t *n_out, int flags, int want_free) {
  if (!m || !n_out || (cap && !out)) return SDM_ERR_INVALID_ARGUMENT;
  if (!m->colours_set) {
    set_error("sdm_get_occupied_rgb", __FILE__, __LINE__, "call sdm_set_colours first");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  HIP_TRY(hipSetDevice(m->device));
  if (cap > m->points_rgb_cap) {
    if (m->d_points_rgb) HIP_TRY(hipFree(m->d_points_rgb));
    m->d_points_rgb = nullptr;
    HIP_TRY(dev_alloc(&m->d_points_rgb, cap));
    m->points_rgb_cap = cap;
  }
  float sub[3] = {0.f, 0.f, 0.f};
  if (flags & SDM_POINTS_ZERO_CENTER)
    for (int a = 0; a < 3; ++a) sub[a] = m->cam_p[a];
  uint32_t cap32 = (uint32_t)std::min<size_t>(cap, 0xffffffffu);
  launch_emit_points_rgb(m->d, m->f, m->st, m->d_colours, m->emit, m->d_points_rgb, cap32, want_free, sub, m->stream);
  return fetch_points(m, m->d_points_rgb, out, sizeof(sdm_point_xyzrgb), cap, n_out);
}
sdm_status sdm_get_occupied_rgb(sdm_map *m, sdm_point_xyzrgb *out, size_t cap, size_t *n_out, int32_t flags) {
  return get_points_rgb(m, out, cap, n_out, flags, 0);
}
sdm_status sdm_get_freespace_rgb(sdm_map *m, sdm_point_xyzrgb *out, size_t cap, size_t *n_out, int32_t flags) {
  return get_points_rgb(m, out, cap, n_out, flags, 1);
}

sdm_status sdm_voxels_device_ptr(sdm_map *m, const sdm_voxel_result **out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  *out = m->st.res;
  return SDM_OK;
}

// ---- batched map queries (queries.hip) ----------------------------------------------------------------------------
// Host mode works through the queries in chunks of QUERY_CHUNK: inputs copied to the map's page-locked staging area and
// up, the kernel, the outputs down, one wait per chunk.  Device mode launches per chunk too (the kernels count in 32 bits)
// and does not wait.  Either way the kernels read the result array in stream order and the host Frame of the last issued
// frame, taken by value at the call.
}  // extern "C"
namespace {
constexpr size_t QUERY_CHUNK = (size_t)1 << 20;
size_t query_align(size_t b) { return (b + 255) & ~(size_t)255; }

sdm_status query_check(sdm_map *m, const void *in, int64_t n, const void *out, uint32_t flags, uint32_t allowed, const char *what) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (!in || !out || n < 0 || (flags & ~allowed)) {
    set_error(what, __FILE__, __LINE__, "null pointer, negative count or unknown flag bits");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  if (m->cfg.shard_count > 1) {
    set_error(what, __FILE__, __LINE__, "queries on a Z-slab shard (shard_count > 1) are not supported: query a whole map");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  return SDM_OK;
}

// launch(in, out, out2, count, stream) enqueues one chunk; out2 (may be null) is a second output array
template <typename Launch>
sdm_status run_query(sdm_map *m, const void *in_v, size_t in_elem, void *out_v, size_t out_elem, void *out2_v, size_t out2_elem,
                            int64_t n, uint32_t flags, Launch launch) {
  if (n == 0) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  const unsigned char *in = static_cast<const unsigned char *>(in_v);
  unsigned char *out = static_cast<unsigned char *>(out_v), *out2 = static_cast<unsigned char *>(out2_v);
  if (!out2) out2_elem = 0;
  if (flags & SDM_QUERY_ON_DEVICE) {
    for (size_t off = 0; off < (size_t)n; off += QUERY_CHUNK) {
      const uint32_t c = (uint32_t)std::min(QUERY_CHUNK, (size_t)n - off);
      launch(in + off * in_elem, out + off * out_elem, out2 ? out2 + off * out2_elem : nullptr, c, m->stream);
      HIP_TRY(hipGetLastError());
    }
    return SDM_OK;
  }
  const size_t chunk = std::min(QUERY_CHUNK, (size_t)n);
  const size_t o_out = query_align(chunk * in_elem), o_out2 = o_out + query_align(chunk * out_elem);
  const size_t need = o_out2 + query_align(chunk * out2_elem);
  if (need > m->query_bytes) {
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (m->h_query) HIP_TRY(hipHostFree(m->h_query));
    if (m->d_query) HIP_TRY(hipFree(m->d_query));
    m->h_query = nullptr;
    m->d_query = nullptr;
    m->query_bytes = 0;
    const size_t grown = std::max(need, (size_t)1 << 20);
    HIP_TRY(hipHostMalloc((void **)&m->h_query, grown, hipHostMallocDefault));
    HIP_TRY(hipMalloc((void **)&m->d_query, grown));
    m->query_bytes = grown;
  }
  for (size_t off = 0; off < (size_t)n; off += chunk) {
    const size_t c = std::min(chunk, (size_t)n - off);
    memcpy(m->h_query, in + off * in_elem, c * in_elem);
    HIP_TRY(hipMemcpyAsync(m->d_query, m->h_query, c * in_elem, hipMemcpyHostToDevice, m->stream));
    launch(m->d_query, m->d_query + o_out, out2 ? m->d_query + o_out2 : nullptr, (uint32_t)c, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(m->h_query + o_out, m->d_query + o_out, c * out_elem, hipMemcpyDeviceToHost, m->stream));
    if (out2) HIP_TRY(hipMemcpyAsync(m->h_query + o_out2, m->d_query + o_out2, c * out2_elem, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    memcpy(out + off * out_elem, m->h_query + o_out, c * out_elem);
    if (out2) memcpy(out2 + off * out2_elem, m->h_query + o_out2, c * out2_elem);
  }
  return SDM_OK;
}
}  // namespace
extern "C" {

sdm_status sdm_query_points(sdm_map *m, const float *xyz, int64_t n, sdm_voxel_result *out, uint32_t *voxel_out, uint32_t flags) {
  const sdm_status e = query_check(m, xyz, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_points");
  if (e != SDM_OK) return e;
  const Frame f = m->f;
  return run_query(m, xyz, 12, out, sizeof(sdm_voxel_result), voxel_out, 4, n, flags,
                   [m, f](const void *in, void *o, void *o2, uint32_t c, hipStream_t s) {
                     launch_query_points(m->d, f, m->st, static_cast<const float *>(in), c, static_cast<sdm_voxel_result *>(o),
                                         static_cast<uint32_t *>(o2), s);
                   });
}

sdm_status sdm_query_segments(sdm_map *m, const float *ab, int64_t n, sdm_segment_hit *out, uint32_t flags) {
  const sdm_status e = query_check(m, ab, n, out, flags, SDM_QUERY_ON_DEVICE | SDM_QUERY_UNKNOWN_BLOCKS, "sdm_query_segments");
  if (e != SDM_OK) return e;
  const Frame f = m->f;
  const int unknown_blocks = (flags & SDM_QUERY_UNKNOWN_BLOCKS) ? 1 : 0;
  return run_query(m, ab, 24, out, sizeof(sdm_segment_hit), nullptr, 0, n, flags,
                   [m, f, unknown_blocks](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     launch_query_segments(m->d, f, m->st, static_cast<const float *>(in), c, static_cast<sdm_segment_hit *>(o),
                                           unknown_blocks, s);
                   });
}

sdm_status sdm_query_boxes(sdm_map *m, const float *boxes, int64_t n, sdm_box_result *out, uint32_t flags) {
  const sdm_status e = query_check(m, boxes, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_boxes");
  if (e != SDM_OK) return e;
  const Frame f = m->f;
  return run_query(m, boxes, 24, out, sizeof(sdm_box_result), nullptr, 0, n, flags,
                   [m, f](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     launch_query_boxes(m->d, f, m->st, static_cast<const float *>(in), c, static_cast<sdm_box_result *>(o), s);
                   });
}

// ---- distance field (esdf.hip) -------------------------------------------------------------------------------------
// The build reads the result array in stream order and takes the host Frame of the last issued frame by value, as the
// queries do; the Frame is kept with the field, so that the distance query and sdm_get_esdf answer for that frame.
}  // extern "C"
namespace {
sdm_status esdf_check(sdm_map *m, const char *what, bool need_field) {
  if (m->cfg.shard_count > 1) {
    set_error(what, __FILE__, __LINE__, "the distance field of a Z-slab shard (shard_count > 1) is not supported: build it on a whole map");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  if (need_field && !m->esdf_valid) {
    set_error(what, __FILE__, __LINE__, "no distance field: call sdm_esdf_update first");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  return SDM_OK;
}
}  // namespace
extern "C" {

sdm_status sdm_esdf_update(sdm_map *m, uint32_t flags) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (flags & ~(SDM_ESDF_UNKNOWN_IS_OBSTACLE | SDM_ESDF_STATIC_ONLY)) {
    set_error("sdm_esdf_update", __FILE__, __LINE__, "unknown flag bits");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  const sdm_status e = esdf_check(m, "sdm_esdf_update", false);
  if (e != SDM_OK) return e;
  HIP_TRY(hipSetDevice(m->device));
  const size_t bytes = (size_t)m->d.V * sizeof(uint32_t);
  if (!m->d_esdf_site) HIP_TRY(hipMalloc((void **)&m->d_esdf_site, bytes));
  if (!m->d_esdf_snap) HIP_TRY(hipMalloc((void **)&m->d_esdf_snap, bytes));
  const Frame f = m->f;
  HIP_TRY(launch_esdf_build(m->d, f, m->st, flags, m->d_esdf_site, m->d_esdf_snap, m->stream));
  m->esdf_f = f;
  m->esdf_valid = true;
  return SDM_OK;
}

sdm_status sdm_get_esdf(sdm_map *m, uint32_t *d2, uint32_t *site, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  const sdm_status e = esdf_check(m, "sdm_get_esdf", true);
  if (e != SDM_OK) return e;
  HIP_TRY(hipSetDevice(m->device));
  const Dims &d = m->d;
  std::vector<uint32_t> own;
  uint32_t *s = site;
  if (d2 && !s) {
    own.resize(d.V);
    s = own.data();
  }
  if (s) HIP_TRY(hipMemcpyAsync(s, m->d_esdf_site, (size_t)d.V * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (d2) {
    for (uint32_t c = 0; c < d.V; ++c) {
      const uint32_t v = s[c];
      if (v == INVALID_INDEX) {
        d2[c] = INVALID_INDEX;
        continue;
      }
      const int dx = (int)(c & (d.NX - 1)) - (int)(v & (d.NX - 1));
      const int dy = (int)((c >> d.x_n) & (d.NY - 1)) - (int)((v >> d.x_n) & (d.NY - 1));
      const int dz = (int)(c >> (d.x_n + d.y_n)) - (int)(v >> (d.x_n + d.y_n));
      d2[c] = (uint32_t)(dx * dx + dy * dy + dz * dz);
    }
  }
  if (origin)
    for (int a = 0; a < 3; ++a) origin[a] = m->esdf_f.center[a] + d.pmin[a];
  return SDM_OK;
}

sdm_status sdm_query_distance(sdm_map *m, const float *xyz, int64_t n, sdm_distance_result *out, uint32_t flags) {
  sdm_status e = query_check(m, xyz, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_distance");
  if (e != SDM_OK) return e;
  e = esdf_check(m, "sdm_query_distance", true);
  if (e != SDM_OK) return e;
  const Frame f = m->esdf_f;
  const uint32_t *site = m->d_esdf_site, *snap = m->d_esdf_snap;
  return run_query(m, xyz, 12, out, sizeof(sdm_distance_result), nullptr, 0, n, flags,
                   [m, f, site, snap](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     launch_query_distance(m->d, f, site, snap, static_cast<const float *>(in), c, static_cast<sdm_distance_result *>(o), s);
                   });
}

sdm_status sdm_object_particle_count(sdm_map *m, int32_t track_id, int64_t *count) {
  if (!m || !count || track_id < 0 || track_id > 65535) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  launch_count_owner(m->d, m->st, (uint16_t)track_id, m->d_u64, m->stream);
  unsigned long long c = 0;
  HIP_TRY(hipMemcpyAsync(&c, m->d_u64, 8, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  *count = (int64_t)c;
  return SDM_OK;
}

sdm_status sdm_tracks_with_particles(sdm_map *m, int32_t *out, int32_t cap, int32_t *n_out) {
  if (!m || !n_out || cap < 0 || (cap > 0 && !out)) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  launch_tracks_with_particles(m->d, m->st, m->d_track_bits, m->stream);
  if (!m->h_track_bits) HIP_TRY(hipHostMalloc((void **)&m->h_track_bits, 2048 * sizeof(uint32_t), hipHostMallocDefault));
  uint32_t *bits = m->h_track_bits;
  HIP_TRY(hipMemcpyAsync(bits, m->d_track_bits, 2048 * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  int32_t n = 0;
  bits[2047] &= 0x7fffffffu;  // (65535 = "no owner")
  for (uint32_t w = 0; w < 2048u; ++w)
    for (uint32_t b = bits[w]; b; b &= b - 1u) {
      if (n < cap) out[n] = (int32_t)(w * 32u + (uint32_t)__builtin_ctz(b));
      ++n;
    }
  *n_out = n;
  return SDM_OK;
}

// ---- introspection ------------------------------------------------------------------------------
sdm_status sdm_get_stats(sdm_map *m, sdm_stats *out, int32_t count_live) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  Counters c;
  sdm_status rc = check_counters(m, &c);
  memset(out, 0, sizeof(*out));
  out->n_visible = c.n_vis;
  out->n_birth_attempts = c.n_birth_attempts;
  out->n_birth_success = c.n_birth_success;
  out->n_resampled_voxels = c.n_resampled;
  for (uint32_t k = 0; k < VIS_SHARDS; ++k) {
    out->n_birth_success += c.shard[k].birth;
    out->n_resampled_voxels += c.shard[k].resample;
  }
  out->n_moved = c.n_moved;
  out->n_move_reinserted = c.n_move_reinserted;
  for (uint32_t k = 0; k < VIS_SHARDS; ++k) out->n_frustum_voxels += c.shard[k].fv;
  out->bfs_start_in_frustum = c.vis_start_in_frustum;
  for (uint32_t k = 0; k < VIS_SHARDS; ++k) {
    out->sweep_live_voxels += c.shard[k].sweep;
    out->sweep_tiles += c.shard[k].sweep_tiles;
  }
  out->flood_rounds = c.vis_flood_rounds;
  for (int a = 0; a < 3; ++a) out->restamped_slabs[a] = m->restamped[a];
  out->graph_frames = (int64_t)m->n_graph_frames;
  out->direct_frames = (int64_t)m->n_direct_frames;
  out->host_enqueue_us = m->enqueue_us;
  out->halo_dropped = c.n_halo_dropped;
  {
    uint32_t al[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(al, m->st.alias, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    out->alias_entries = al[0] < m->st.alias_cap ? al[0] : m->st.alias_cap;
    out->alias_overflowed = (al[0] > m->st.alias_cap || al[1] != 0) ? 1 : 0;
  }
  if (m->profiling) {
    int prev = 0;
    for (int sidx = 1; sidx <= 7; ++sidx) {
      if (!m->stage_ran[sidx]) continue;
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, m->ev[prev], m->ev[sidx]) == hipSuccess) out->stage_ms[sidx] = ms;
      prev = sidx;
    }
  }
  if (count_live) {
    launch_count_live(m->d, m->st, m->d_u64, m->stream);
    unsigned long long n = 0;
    HIP_TRY(hipMemcpyAsync(&n, m->d_u64, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    out->live_particles = (int64_t)(n & ((1ull << 36) - 1));
    out->live_voxels = (int64_t)(n >> 36);
    size_t nocc = 0;
    // occupied voxel count from the result array
    launch_emit_count(m->d, m->st, m->emit, 0, m->stream);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, m->emit.total, 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    nocc = total;
    out->n_occupied = (int64_t)nocc;
  }
  return rc;
}

sdm_status sdm_debug_force_generic_flood(sdm_map *m, int32_t on) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->force_generic_flood = on ? 1 : 0;
  return SDM_OK;
}

sdm_status sdm_set_profiling(sdm_map *m, int32_t on) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->profiling = on != 0;
  return SDM_OK;
}

sdm_status sdm_get_ring_state(sdm_map *m, sdm_ring_state *o) {
  if (!m || !o) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  Cursors c;
  HIP_TRY(hipMemcpyAsync(&c, m->sc.cur, sizeof(c), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  o->global_time_stamp = m->global_time_stamp;
  for (int a = 0; a < 3; ++a) {
    o->moved_steps[a] = m->moved_steps[a];
    o->eq_steps[a] = m->eq_steps[a];
    o->map_center[a] = m->map_center[a];
    o->last_pos[a] = m->last_pos[a];
  }
  o->birth_cursor = c.birth_cursor;
  o->move_cursor = c.move_cursor;
  return SDM_OK;
}

sdm_status sdm_set_ring_state(sdm_map *m, const sdm_ring_state *o) {
  if (m) m->sweep_all = true;
  if (!m || !o) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  m->global_time_stamp = o->global_time_stamp;
  for (int a = 0; a < 3; ++a) {
    m->moved_steps[a] = o->moved_steps[a];
    m->eq_steps[a] = o->eq_steps[a];
    m->map_center[a] = o->map_center[a];
    m->last_pos[a] = o->last_pos[a];
  }
  Cursors c{o->birth_cursor, o->move_cursor};
  HIP_TRY(hipMemcpyAsync(m->sc.cur, &c, sizeof(c), hipMemcpyHostToDevice, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  sync_frame_scalars(m);
  return SDM_OK;
}

sdm_status sdm_get_stamps(sdm_map *m, uint32_t *sx, uint32_t *sy, uint32_t *sz) {
  if (!m || !sx || !sy || !sz) return SDM_ERR_INVALID_ARGUMENT;
  memcpy(sx, m->stamps_x.data(), m->d.NX * 4);
  memcpy(sy, m->stamps_y.data(), m->d.NY * 4);
  memcpy(sz, m->stamps_z.data(), m->d.NZ * 4);
  return SDM_OK;
}
sdm_status sdm_set_stamps(sdm_map *m, const uint32_t *sx, const uint32_t *sy, const uint32_t *sz) {
  if (m) m->sweep_all = true;
  if (!m || !sx || !sy || !sz) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  memcpy(m->stamps_x.data(), sx, m->d.NX * 4);
  memcpy(m->stamps_y.data(), sy, m->d.NY * 4);
  memcpy(m->stamps_z.data(), sz, m->d.NZ * 4);
  sdm_status rc = upload_stamps(m);
  if (rc != SDM_OK) return rc;
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}

sdm_status sdm_dump_state(sdm_map *m, float *px, float *py, float *pz, float *w, uint16_t *ts, uint16_t *track,
                          uint8_t *label, uint8_t *status, uint8_t *forget, uint16_t *owner) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t n = (size_t)m->d.v_count * m->d.S;
  if (px || py || pz || forget) {
    float *tx, *ty, *tz;
    uint8_t *tf;
    HIP_TRY(dev_alloc(&tx, n));
    HIP_TRY(dev_alloc(&ty, n));
    HIP_TRY(dev_alloc(&tz, n));
    HIP_TRY(dev_alloc(&tf, n));
    launch_unpack_pos4(m->st.pos4, m->st.forget, tx, ty, tz, tf, n, s);
    if (px) HIP_TRY(hipMemcpyAsync(px, tx, n * 4, hipMemcpyDeviceToHost, s));
    if (py) HIP_TRY(hipMemcpyAsync(py, ty, n * 4, hipMemcpyDeviceToHost, s));
    if (pz) HIP_TRY(hipMemcpyAsync(pz, tz, n * 4, hipMemcpyDeviceToHost, s));
    if (forget) HIP_TRY(hipMemcpyAsync(forget, tf, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(tx);
    (void)hipFree(ty);
    (void)hipFree(tz);
    (void)hipFree(tf);
  }
  if (w || ts || track || label || status) {  // record fields -> the reference's slot order, through dense temporaries
    float *tw;
    uint16_t *tts, *ttr;
    uint8_t *tl, *tst;
    HIP_TRY(dev_alloc(&tw, n));
    HIP_TRY(dev_alloc(&tts, n));
    HIP_TRY(dev_alloc(&ttr, n));
    HIP_TRY(dev_alloc(&tl, n));
    HIP_TRY(dev_alloc(&tst, n));
    launch_rec_unpack(m->d, m->st, tw, tts, ttr, tl, tst, s);
    if (status) HIP_TRY(hipMemcpyAsync(status, tst, n, hipMemcpyDeviceToHost, s));
    if (w) HIP_TRY(hipMemcpyAsync(w, tw, n * 4, hipMemcpyDeviceToHost, s));
    if (ts) HIP_TRY(hipMemcpyAsync(ts, tts, n * 2, hipMemcpyDeviceToHost, s));
    if (track) HIP_TRY(hipMemcpyAsync(track, ttr, n * 2, hipMemcpyDeviceToHost, s));
    if (label) HIP_TRY(hipMemcpyAsync(label, tl, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(tw);
    (void)hipFree(tts);
    (void)hipFree(ttr);
    (void)hipFree(tl);
    (void)hipFree(tst);
  }
  if (owner) HIP_TRY(hipMemcpyAsync(owner, m->st.owner, n * 2, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (owner) {
    // one owner per slot in the exported array: a slot that sits in several sets (State::alias) reports the largest
    // track id, which is what walking the reference's sets in ascending track order leaves behind
    std::vector<uint32_t> al(2 + 2 * ALIAS_CAP);
    HIP_TRY(hipMemcpyAsync(al.data(), m->st.alias, al.size() * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    const uint32_t na = std::min<uint32_t>(al[0], m->st.alias_cap);
    for (uint32_t k = 0; k < na; ++k) {
      const uint32_t idx = al[2 + 2 * k], trk = al[3 + 2 * k];
      if (trk == OWNER_NONE || idx >= n) continue;
      if (owner[idx] == OWNER_NONE || owner[idx] < trk) owner[idx] = (uint16_t)trk;
    }
  }
  return SDM_OK;
}

sdm_status sdm_load_state(sdm_map *m, const float *px, const float *py, const float *pz, const float *w,
                          const uint16_t *ts, const uint16_t *track, const uint8_t *label, const uint8_t *status,
                          const uint8_t *forget, const uint16_t *owner) {
  if (!m || !px || !py || !pz || !w || !ts || !track || !label || !status || !forget) return SDM_ERR_INVALID_ARGUMENT;
  m->sweep_all = true;
  m->state_event_valid = false;
  HIP_TRY(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  const size_t n = (size_t)m->d.v_count * m->d.S;
  // (which tiles are dense is not known of a state that comes from outside: the first sweep classifies everything)
  HIP_TRY(hipMemsetAsync(m->st.grp_hint, 0, grp_hint_bytes(m->d.v_count), s));
  m->sweep_skip_scan = false;
  m->sweep_rec_pending = false;
  float *tx, *ty, *tz;
  uint8_t *tf;
  HIP_TRY(dev_alloc(&tx, n));
  HIP_TRY(dev_alloc(&ty, n));
  HIP_TRY(dev_alloc(&tz, n));
  HIP_TRY(dev_alloc(&tf, n));
  HIP_TRY(hipMemcpyAsync(tx, px, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ty, py, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(tz, pz, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(tf, forget, n, hipMemcpyHostToDevice, s));
  launch_pack_pos4(m->st.pos4, m->st.forget, tx, ty, tz, tf, n, s);
  {
    float *tw;
    uint16_t *tts, *ttr;
    uint8_t *tl, *tst;
    HIP_TRY(dev_alloc(&tw, n));
    HIP_TRY(dev_alloc(&tts, n));
    HIP_TRY(dev_alloc(&ttr, n));
    HIP_TRY(dev_alloc(&tl, n));
    HIP_TRY(dev_alloc(&tst, n));
    HIP_TRY(hipMemcpyAsync(tst, status, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tw, w, n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tts, ts, n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ttr, track, n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tl, label, n, hipMemcpyHostToDevice, s));
    launch_rec_pack(m->d, m->st, tw, tts, ttr, tl, tst, s);
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(tw);
    (void)hipFree(tts);
    (void)hipFree(ttr);
    (void)hipFree(tl);
    (void)hipFree(tst);
  }
  if (owner) HIP_TRY(hipMemcpyAsync(m->st.owner, owner, n * 2, hipMemcpyHostToDevice, s));
  else HIP_TRY(hipMemsetAsync(m->st.owner, 0xFF, n * 2, s));
  launch_owner_flags(m->d, m->st, s);
  HIP_TRY(hipMemsetAsync(m->st.alias, 0, 8, s));  // the imported owner array is all there is to the sets
  HIP_TRY(hipMemsetAsync(m->st.alias_filter, 0, ALIAS_FILTER_WORDS * 4, s));
  launch_vflag_from_records(m->d, m->st, s);  // "something here" flags from the status rows (the voxel stamps came with slot 0 of the stamp rows)
  HIP_TRY(hipStreamSynchronize(s));
  (void)hipFree(tx);
  (void)hipFree(ty);
  (void)hipFree(tz);
  (void)hipFree(tf);
  return SDM_OK;
}

sdm_status sdm_get_ck_kappa(sdm_map *m, float *out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  if (m->ck_raw_last) launch_ck_finish(m->d, m->flt, m->sc, m->ck_raw_last, 1, 0, m->stream);  // (debug read-out of a sharded frame)
  HIP_TRY(hipMemcpyAsync(out, m->sc.ck_kappa, (size_t)m->d.W * m->d.H * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}
sdm_status sdm_get_bin_counts(sdm_map *m, uint32_t *out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(out, m->sc.bin_count, (size_t)m->d.W * m->d.H * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}
sdm_status sdm_get_bins(sdm_map *m, uint32_t *out, int64_t cap, int64_t *n_out) {
  if (!m || !n_out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  Counters c;
  HIP_TRY(hipMemcpyAsync(&c, m->sc.cnt, sizeof(c), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  *n_out = c.n_vis;
  const int64_t n_vis = std::min<int64_t>(c.n_vis, m->sc.cap_vis);
  if (n_vis > 0 && out && cap > 0) {
    // pixel-major order (the order of the reference's bins): the rows' blocks lie in the device array in the order their
    // workgroups reserved them, so the rows are put in image order here
    const int W = m->d.W, H = m->d.H;
    std::vector<uint32_t> idx((size_t)n_vis), bs((size_t)H * (W + 1));
    HIP_TRY(hipMemcpyAsync(idx.data(), m->sc.bin_idx, idx.size() * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemcpyAsync(bs.data(), m->sc.bin_start, bs.size() * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    int64_t at = 0;
    for (int r = 0; r < H && at < cap; ++r) {
      const uint32_t a = bs[(size_t)r * (W + 1)], b = bs[(size_t)r * (W + 1) + W];
      for (uint32_t k = a; k < b && at < cap && k < (uint32_t)n_vis; ++k) out[at++] = idx[k];
    }
  }
  return SDM_OK;
}
sdm_status sdm_get_extrinsic(sdm_map *m, float *out16) {
  if (!m || !out16) return SDM_ERR_INVALID_ARGUMENT;
  memcpy(out16, m->f.E, 64);
  return SDM_OK;
}

// Roofline helper for bench.py: the occupancy sweep alone, `iters` launches on the map's stream,
// bracketed by HIP events on that stream.
sdm_status sdm_time_occupancy_sweep(sdm_map *m, int32_t iters, float *avg_ms) {
  if (!m || !avg_ms || iters <= 0) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  hipEvent_t a, b;
  HIP_TRY(hipEventCreate(&a));
  HIP_TRY(hipEventCreate(&b));
  // (what these sweeps have to see again, the next frame's sweep has to see: marked with its epoch)
  // (warm-up, and the launch whose word decides how the timed ones run: all_dirty - the full evaluation every time)
  launch_occupancy(m->d, m->flt, m->st, m->sc.cnt, 1, m->sc.fa, m->sweep_epoch, m->stream, sweep_mode(m));
  m->sweep_rec_pending = true;
  HIP_TRY(hipStreamSynchronize(m->stream));
  {
    const sdm_status rc = sweep_mode_latch(m);
    if (rc != SDM_OK) return rc;
  }
  const int mode = sweep_mode(m);
  HIP_TRY(hipEventRecord(a, m->stream));
  for (int i = 0; i < iters; ++i) launch_occupancy(m->d, m->flt, m->st, m->sc.cnt, 1, m->sc.fa, m->sweep_epoch, m->stream, mode);
  HIP_TRY(hipEventRecord(b, m->stream));
  HIP_TRY(hipEventSynchronize(b));
  m->sweep_rec_pending = true;
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, a, b));
  *avg_ms = ms / iters;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return SDM_OK;
}

// Bench hook: overwrite the map with the dense case (every slot live, every voxel observed).
sdm_status sdm_debug_fill_dense_ex(sdm_map *m, int32_t mode) {
  if (!m || mode < 0 || mode > 1) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  launch_fill_dense(m->d, m->st, m->global_time_stamp ? m->global_time_stamp : 1u, mode, m->stream);
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
}
sdm_status sdm_debug_fill_dense(sdm_map *m) { return sdm_debug_fill_dense_ex(m, 0); }
sdm_status sdm_debug_sweep_lists(sdm_map *m, int32_t mode) {
  if (!m || mode < -1 || mode > 1) return SDM_ERR_INVALID_ARGUMENT;
  m->sweep_lists_forced = mode;
  if (mode >= 0) m->sweep_lists = mode != 0;
  return SDM_OK;
}
sdm_status sdm_debug_sweep_mode(sdm_map *m, int32_t *mode_out) {
  if (!m || !mode_out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipStreamSynchronize(m->stream));
  const sdm_status rc = sweep_mode_latch(m);
  if (rc != SDM_OK) return rc;
  *mode_out = sweep_mode(m);
  return SDM_OK;
}
sdm_status sdm_debug_alias_cap(sdm_map *m, int32_t cap) {
  if (!m || cap < 1 || (uint32_t)cap > ALIAS_CAP) return SDM_ERR_INVALID_ARGUMENT;
  if (m->n_graph_frames || m->n_direct_frames) return SDM_ERR_INVALID_ARGUMENT;  // (captured graphs hold the State by value)
  m->st.alias_cap = (uint32_t)cap;
  return SDM_OK;
}
sdm_status sdm_debug_hinted_groups(sdm_map *m, int64_t *n_out) {
  if (!m || !n_out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  std::vector<uint8_t> h(grp_hint_bytes(m->d.v_count));
  HIP_TRY(hipMemcpyAsync(h.data(), m->st.grp_hint, h.size(), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  int64_t n = 0;
  for (uint8_t b : h) n += b != 0;
  *n_out = n;
  return SDM_OK;
}

#ifdef SDM_AB_TIMERS
extern "C++" {
namespace sdm {
void debug_timers(unsigned long long *out32, int reset);
void debug_timers_moves(unsigned long long *out, int reset);
}
}
sdm_status sdm_debug_timers(sdm_map *m, unsigned long long *out32, int reset) {
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipDeviceSynchronize());
  sdm::debug_timers(out32, reset);
  sdm::debug_timers_moves(out32 + 6 * 8192 * 4, reset);
  return SDM_OK;
}
#endif

// Page-locked host memory for the buffers handed to sdm_update / sdm_update_raw: uploads from it run at PCIe speed
// and beside the kernels of the previous frame.
sdm_status sdm_host_alloc(size_t bytes, void **out) {
  if (!out || !bytes) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return SDM_OK;
}
sdm_status sdm_host_free(void *p) {
  if (p) HIP_TRY(hipHostFree(p));
  return SDM_OK;
}

// ---- unit-test hooks for the primitives -------------------------------------------------------
sdm_status sdm_test_scan(const uint32_t *in, uint32_t *out, int64_t n) {
  if (!in || !out || n <= 0) return SDM_ERR_INVALID_ARGUMENT;
  uint32_t *din, *dout, *scr;
  HIP_TRY(dev_alloc(&din, (size_t)n));
  HIP_TRY(dev_alloc(&dout, (size_t)n));
  HIP_TRY(dev_alloc(&scr, scan_scratch_elems((size_t)n) + 16));
  HIP_TRY(hipMemset(scr, 0, (scan_scratch_elems((size_t)n) + 16) * 4));
  HIP_TRY(hipMemcpy(din, in, (size_t)n * 4, hipMemcpyHostToDevice));
  exclusive_scan_u32(din, dout, (size_t)n, scr, nullptr);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
  (void)hipFree(din);
  (void)hipFree(dout);
  (void)hipFree(scr);
  return SDM_OK;
}

sdm_status sdm_test_sort_pairs(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                               int64_t n, int32_t nbits) {
  if (!keys_in || !vals_in || !keys_out || !vals_out || n <= 0 || nbits <= 0 || nbits > 32) return SDM_ERR_INVALID_ARGUMENT;
  uint32_t *ka, *va, *kb, *vb, *scr;
  HIP_TRY(dev_alloc(&ka, (size_t)n));
  HIP_TRY(dev_alloc(&va, (size_t)n));
  HIP_TRY(dev_alloc(&kb, (size_t)n));
  HIP_TRY(dev_alloc(&vb, (size_t)n));
  HIP_TRY(dev_alloc(&scr, sort_scratch_elems((size_t)n) + 16));
  HIP_TRY(hipMemset(scr, 0, (sort_scratch_elems((size_t)n) + 16) * 4));
  HIP_TRY(hipMemcpy(ka, keys_in, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(va, vals_in, (size_t)n * 4, hipMemcpyHostToDevice));
  int which = radix_sort_pairs(ka, va, kb, vb, (size_t)n, nbits, scr, nullptr);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(keys_out, which ? kb : ka, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(vals_out, which ? vb : va, (size_t)n * 4, hipMemcpyDeviceToHost));
  (void)hipFree(ka);
  (void)hipFree(va);
  (void)hipFree(kb);
  (void)hipFree(vb);
  (void)hipFree(scr);
  return SDM_OK;
}

}  // extern "C"
