// sdm_map.h — private to the host units of libsdm_hip (not installed): the map object behind the C ABI (include/sdm.h) -
// the frame pipeline's state flat in sdm_map, the state of every derived layer in a struct of its own -, the error macros,
// who owns what a map allocates, and the host helpers that more than one unit uses: the frame's, and the layers' (their
// one check, their one refusal, their one origin, their one checked launch, the one staging path of the host-mode batched
// calls).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "sdm_internal.h"
#include "sdm_scratch.h"

typedef struct ncclComm *ncclComm_t;  // (rccl.h's own declaration: only exchange.hip includes that header)

namespace sdm {
// the thread's last error (sdm_last_error): "what (file:line): detail"
void set_error(const char *what, const char *file, int line, const char *detail);
}  // namespace sdm

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      sdm::set_error(#expr, __FILE__, __LINE__, hipGetErrorString(e_));      \
      return SDM_ERR_HIP;                                                    \
    }                                                                        \
  } while (0)
#define NCCL_TRY(expr)                                                       \
  do {                                                                       \
    ncclResult_t r_ = (expr);                                                \
    if (r_ != ncclSuccess) {                                                 \
      sdm::set_error(#expr, __FILE__, __LINE__, ncclGetErrorString(r_));     \
      return SDM_ERR_COMM;                                                   \
    }                                                                        \
  } while (0)
#define SDM_TRY(expr) do { const sdm_status rc_ = (expr); if (rc_ != SDM_OK) return rc_; } while (0)
// the layers' refusal of an argument: the thread's error names the place, the value is the status to return
#define LAYER_REFUSE(what, why) (sdm::set_error(what, __FILE__, __LINE__, why), SDM_ERR_INVALID_ARGUMENT)
// a launch of a layer's build, inside a function that returns hipError_t: returns the launch's error, if any
#define LAYER_LAUNCH(kernel, grid, tpb, stream, ...)                             \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(tpb), 0, stream, __VA_ARGS__);   \
    const hipError_t e_ = hipGetLastError();                                     \
    if (e_ != hipSuccess) return e_;                                             \
  } while (0)

using namespace sdm;

// ---- the derived map layers ---------------------------------------------------------------------------------------------
// Built beside the frame pipeline and touched by their own units only (reach.hip also reads the distance field); no frame
// reads any of it.  Their buffers are the map's like any other (alloc_tracked / regrow, freed by sdm_destroy), allocated
// by the first build or call.  What every layer with a build keeps: the Frame it was built from (map center, ring
// offsets), the build's flags, and whether there is a build at all.
struct Derived {
  Frame f{};
  uint32_t flags = 0;
  bool valid = false;
  void built(const Frame &from, uint32_t with) { f = from, flags = with, valid = true; }  // the layer answers for this build from here on
};
// host-mode staging of the batched calls (run_staged, queries.hip): the preamble and one chunk's inputs and outputs, on
// the device and page-locked; grown on demand, both together: `bytes` is non-zero only while both exist
struct QueryStage {
  unsigned char *d = nullptr, *h = nullptr;
  size_t bytes = 0;
};
// the distance field (esdf.hip): site and snapshot word per cell in map-index order
struct EsdfLayer : Derived {
  uint32_t *site = nullptr, *snap = nullptr;
};
// the instance table (instances.hip): the accumulators (empty between builds), the table of the last build, its count
// ([0]) and label counters ([1..256])
struct InstLayer : Derived {
  unsigned char *acc = nullptr;
  sdm_instance *out = nullptr;
  uint32_t *meta = nullptr;
};
// the frontiers (frontiers.hip): the free / unknown / frontier bitmasks and the words' prefix; the per-cell arrays,
// accumulators (empty between builds) and cluster table, laid out for `alloc` cells of which `cap` are in use and grown
// by a build that asks for more; the build's counters (its scans use the layers' shared scratch, layer_scan_scratch)
struct FrontLayer : Derived {
  unsigned char *bits = nullptr, *cells = nullptr;
  uint32_t *meta = nullptr;
  size_t alloc = 0;
  int64_t cap = 0;
};
// view scoring (views.hip): a pool of `masks` bitmasks of V / 8 bytes, one per view in flight, zero between calls; batch:
// sdm_debug_view_batch's bound on the views in flight (0: as many as the pool has masks); clear_rewalk: a batch's masks
// are cleared by walking its rays again instead of zeroing them whole
struct ViewPool {
  uint32_t *pool = nullptr;
  uint32_t masks = 0;
  int32_t batch = 0;
  bool clear_rewalk = false;
};
// the travel-cost field (reach.hip): the cost per cell and the traversable bitmask in map-index order, the tiles' activity
// bitmask and the list of a round's active tiles, the build's counters (and their page-locked landing area), its arguments
struct ReachLayer : Derived {
  uint32_t *cost = nullptr, *trav = nullptr, *act = nullptr, *list = nullptr;
  uint32_t *meta = nullptr, *h_meta = nullptr;
  uint32_t min_d2 = 0, max_cost = 0;
};
// the forecast (forecast.hip): the two field words per cell in map-index order; the build's table - the motions' track
// set, the per-track stamp offsets, the stamps - on the device and in two page-locked copies that builds fill in turn, each
// with the event that says its last upload has left it; the build's counters (and their page-locked landing area); the cell list's word
// popcounts (their scan uses the layers' shared scratch); what the last build was given
struct ForecastLayer : Derived {
  uint32_t *mask = nullptr, *first = nullptr;
  uint32_t *table = nullptr, *h_table[2] = {nullptr, nullptr};
  hipEvent_t ev_table[2] = {nullptr, nullptr};
  int table_next = 0;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  uint32_t *pre = nullptr;
  float t[16] = {};
  uint32_t n_motions = 0, n_horizons = 0, n_stamps = 0;
};

// the ground layer (ground.hip): a cell, a squared distance and the distance transform's row distance per column of the
// grid, laid out for the largest of the three grids; the build's counters, eight words per row of the grid; the build's
// options (its flags are Derived's)
struct GroundLayer : Derived {
  sdm_ground_cell *cells = nullptr;
  uint32_t *d2 = nullptr, *meta = nullptr;
  uint16_t *rowd = nullptr;
  sdm_ground_options opt{};
};

// the surface mesh (mesh.hip): the solid / unknown / occupied masks, the corner mask and the two prefixes in one block; the
// face records, their vertex ids and the vertex list, laid out for alloc_f faces and alloc_v vertices and grown by a build
// that asks for more; the build's counters and rows of counts, the rows every wave of the emitting kernel leaves; the
// build's options with the capacities resolved (its flags are Derived's).  Its scans use the layers' shared scratch.
struct MeshLayer : Derived {
  unsigned char *bits = nullptr;
  sdm_mesh_face *faces = nullptr;
  uint32_t *quads = nullptr;
  sdm_mesh_vertex *verts = nullptr;
  uint32_t *meta = nullptr, *stats = nullptr;
  size_t alloc_f = 0, alloc_v = 0;
  sdm_mesh_options opt{};
};

// the world archive (world.hip): the hash table (64-bit keys, the pool slot beside each), the pool of bricks - 512 words
// and a header of five words each, in creation order -, the candidates' arrays of an update (flag, rank, slot, writing
// cells), the counters, a sort scratch of its own (its scans use the layers' shared scratch), the
// sort's four buffers and the per-brick counts of the occupied list; order: the pool slots in brick order (inside
// sortbuf) while `sorted`.  Derived's frame and flags are the last update's, steps the moved_steps it was built from;
// capacity_set: an update or import since creation or sdm_world_clear has fixed max_bricks.  io: the work arrays of an
// import (world_io.hip), io_elems words: grown on demand, kept by an import in device mode, released by one in host mode.
struct WorldLayer : Derived {
  uint32_t *io = nullptr;
  size_t io_elems = 0;
  int steps[3] = {0, 0, 0};
  unsigned long long *keys = nullptr;
  uint32_t *vals = nullptr, *cells = nullptr, *hdr = nullptr, *cand = nullptr, *meta = nullptr;
  uint32_t *sort = nullptr, *sortbuf = nullptr, *cnt = nullptr;
  const uint32_t *order = nullptr;
  uint32_t max_bricks = 0, hmask = 0, n_updates = 0;
  bool capacity_set = false, sorted = false;
};

// world reach (world_reach.hip): a snapshot of the archive's bricks as a travel-cost field, laid out for `cap` bricks of
// which n are in use and grown by a build that needs more: per brick of rank r its coordinates (two words), the ranks of
// the 27 bricks round it, the traversable and the obstacle mask (8 x 64 bits each) and 512 costs; the hash table from
// brick key to rank (hmask + 1 slots in use); the bricks' activity bitmask and the list of a round's active bricks; the
// build's counters (and their page-locked landing area), its arguments and the archive's stamp.  No pool slot is kept.
struct WorldReachLayer : Derived {
  uint32_t *cost = nullptr, *nbr = nullptr, *coord = nullptr, *vals = nullptr, *act = nullptr, *list = nullptr;
  unsigned long long *trav = nullptr, *obst = nullptr, *keys = nullptr;
  uint32_t *meta = nullptr, *h_meta = nullptr;
  size_t cap = 0;
  uint32_t n = 0, hmask = 0, inflate = 0, max_cost = 0, stamp = 0;
};

// world frontiers (world_frontiers.hip): a snapshot of the archive's frontier cells and their clusters.  Per archived brick
// (cap_arch) the box flag, the rank in the field and the free and unknown words; per pool slot (cap_slots) the brick's place
// in brick order; per brick of the field (cap_bricks) its coordinates, its place in brick order, the ranks of the 27 bricks
// round it, the places of the six face neighbours, the frontier words and their prefix - all of them the build's own, read
// by nobody once it returns.  Per cell (cap_cells) the world cell, parent (the cluster index in the end), root, the
// scanned flags, unknown_faces, the accumulators (empty between builds) and the table.  The build's counters (and their
// page-locked landing area, whose last word takes a count the build waits for), its arguments, the archive's stamp; over:
// the build found more cells than max_cells and wrote no list.  Every buffer is grown by the build that needs more.
struct WorldFrontiersLayer : Derived {
  uint32_t *flag = nullptr, *rank = nullptr, *place_of_slot = nullptr;
  unsigned long long *free_m = nullptr, *unk_m = nullptr, *front = nullptr;
  uint32_t *coord = nullptr, *place = nullptr, *nbr = nullptr, *face_place = nullptr, *pre = nullptr;
  int32_t *xyz = nullptr;
  uint32_t *parent = nullptr, *root = nullptr, *idx = nullptr;
  uint8_t *faces = nullptr;
  unsigned char *acc = nullptr;
  sdm_world_frontier_cluster *table = nullptr;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  size_t cap_arch = 0, cap_slots = 0, cap_bricks = 0, cap_cells = 0;
  uint32_t n = 0, stamp = 0;
  int32_t min_cells = 0;
  int64_t n_cells = 0, max_cells = 0;
  bool over = false;
};

// the world distance field (world_esdf.hip): a snapshot of the archive's bricks as a truncated distance field.  Per
// archived brick (cap_arch) the box flag, the rank in the field and the eight obstacle words, indexed by pool slot - the
// build's own, read by nobody once it has run; per brick of the field (cap_bricks) its coordinates and 512 packed field
// words, and the hash table from brick key to rank (hmask + 1 slots in use).  The two info counters (and their page-locked
// landing area, whose last word takes the count the build waits for), the build's radius, the archive's stamp.
struct WorldEsdfLayer : Derived {
  uint32_t *flag = nullptr, *rank = nullptr, *coord = nullptr, *vals = nullptr, *field = nullptr;
  unsigned long long *obst = nullptr, *keys = nullptr;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  size_t cap_arch = 0, cap_bricks = 0;
  uint32_t n = 0, hmask = 0, radius = 0, stamp = 0;
};

// the world ground layer (world_ground.hip): a snapshot of the archive's bricks as a height map and costmap in tiles of
// 8 x 8 columns.  Per archived brick (cap_arch) the flag of the one brick that claimed its tile and its rank - the build's
// own - and the hash table from tile key to rank (hmask + 1 slots in use: it is filled before the tiles are counted); per
// tile (cap_tiles) its key, 64 cells, 64 squared distances, the lethal word and the sort's four words.  The info counters
// (and their page-locked landing area, whose last word takes the count the build waits for), the build's options (its
// flags are Derived's), the archive's stamp.  No pool slot is kept.
struct WorldGroundLayer : Derived {
  uint32_t *flag = nullptr, *rank = nullptr, *vals = nullptr, *coord = nullptr, *sortbuf = nullptr;
  unsigned long long *keys = nullptr, *lethal = nullptr;
  sdm_ground_cell *cells = nullptr;
  uint16_t *d2 = nullptr;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  size_t cap_arch = 0, cap_tiles = 0;
  uint32_t n = 0, hmask = 0, stamp = 0;
  sdm_world_ground_options opt{};
};

// world ground reach (world_ground_reach.hip): a snapshot of the world ground layer's costmap as a 2-D travel-cost field,
// laid out for `cap` tiles of which n are in use and grown by a build that needs more: per tile of rank r its key, the
// ranks of the eight tiles round it, the traversable and the penalty word, 64 levels and 64 costs; the hash table from tile
// key to rank (hmask + 1 slots in use); the tiles' activity bitmask and the list of a round's active tiles; the build's
// counters (and their page-locked landing area), its options (its flags are Derived's), the options of the ground build it
// stands on and the archive's stamp that build carried.  Nothing of the ground layer is kept.
struct WorldGroundReachLayer : Derived {
  uint32_t *cost = nullptr, *nbr = nullptr, *coord = nullptr, *vals = nullptr, *act = nullptr, *list = nullptr;
  unsigned long long *trav = nullptr, *pen = nullptr, *keys = nullptr;
  uint16_t *level = nullptr;
  uint32_t *meta = nullptr, *h_meta = nullptr;
  size_t cap = 0;
  uint32_t n = 0, hmask = 0, stamp = 0;
  sdm_world_ground_reach_options opt{};
  sdm_world_ground_options ground{};
};

// world rays (world_rays.hip): the views' pool of bitmasks, `words` words, one mask of (2 reach + 1)^3 bits per view in
// flight, grown on demand up to 64 MiB and zero between calls; batch: sdm_debug_world_view_batch's bound on the views in
// flight (0: as many as the pool may hold masks)
struct WorldRaysPool {
  uint32_t *pool = nullptr;
  size_t words = 0;
  int32_t batch = 0;
};

// world match (world_match.hip): the work arrays of a match, `words` words - the transient source table (64-bit keys, the
// lowest source index beside each), five counts per candidate and the totals -, grown on demand, kept by a match in device
// mode and released by one in host mode
struct WorldMatchPool {
  uint32_t *work = nullptr;
  size_t words = 0;
};

// the world mesh (world_mesh.hip): a snapshot of the archive's surface as faces and welded vertices.  Per archived brick
// (cap_arch) the box flag, the rank in the field and the solid, unknown and occupied words, indexed by pool slot; per brick
// of the field (cap_bricks) its coordinates, its pool slot, the pool slots of the six face neighbours, table slot and rank
// of its corners' eight owner bricks and the prefix of its slices' face counts, and a row of counts per 64 slices; the vertex
// bricks' hash table (cap_slots: key, rank, the scanned claim flag, 512 corner bits a slot, a count per 64 slots) and per
// vertex brick (cap_vb) the sort's four words and the prefix of its levels' corner counts - all of them the build's own,
// read by nobody once it has run, the coordinates apart.  The lists: 12-byte
// face records and four vertex ids per face (cap_f), an int32 triple per vertex (cap_v).  The build's counters (and their
// page-locked landing area, whose last word takes a count the build waits for), the counts it waited for, its options
// (its flags are Derived's), the archive's stamp; over: the build found more than a cap allows and wrote no list.
struct WorldMeshLayer : Derived {
  uint32_t *flag = nullptr, *rank = nullptr;
  unsigned long long *solid_m = nullptr, *unk_m = nullptr, *occ_m = nullptr;
  uint32_t *coord = nullptr, *slot_of = nullptr, *nbr = nullptr, *own_h = nullptr, *own_i = nullptr, *pre = nullptr;
  unsigned long long *vkeys = nullptr, *vmask = nullptr;
  uint32_t *vvals = nullptr, *vflag = nullptr, *rows = nullptr, *vrows = nullptr, *sortbuf = nullptr, *vpre = nullptr;
  uint32_t *faces = nullptr, *quads = nullptr;
  int32_t *corners = nullptr;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  size_t cap_arch = 0, cap_bricks = 0, cap_slots = 0, cap_vb = 0, cap_f = 0, cap_v = 0;
  uint32_t n = 0, n_vb = 0, stamp = 0;
  int64_t n_faces = 0, n_vertices = 0;
  int64_t counts[11] = {};  // solid cells, faces by direction, faces by kind
  sdm_world_mesh_options opt{};
  bool over = false;
};

// world objects (world_objects.hip): a snapshot of the archive's occupied cells as connected same-key components.  Per
// archived brick (cap_arch) the box flag and the rank in the field - the build's own; per brick of the field (cap_bricks)
// its coordinates, its pool slot and the ranks of the 27 bricks round it (the build's own), the eight counted words and
// their prefix, and the hash table from brick key to rank (hmask + 1 slots in use) - what the query reads.  Per counted
// cell (cap_cells) the world cell, the archived word, parent (the object index in the end), root and the scanned root
// flags; per object (cap_objects) the accumulator (empty between builds), the index of its first cell, the scanned
// listing flags and the table.  The build's counters and per-label counters (and their page-locked landing area, whose
// last word takes a count the build waits for), its arguments, the archive's stamp; over: the build found more cells than
// max_cells and wrote no list.  Every buffer is grown by the build that needs more.
struct WorldObjectsLayer : Derived {
  uint32_t *flag = nullptr, *rank = nullptr;
  uint32_t *coord = nullptr, *slot_of = nullptr, *nbr = nullptr, *pre = nullptr, *vals = nullptr;
  unsigned long long *cw = nullptr, *keys = nullptr;
  int32_t *xyz = nullptr;
  uint32_t *word = nullptr, *parent = nullptr, *root = nullptr, *idx = nullptr;
  unsigned char *acc = nullptr;
  uint32_t *first = nullptr, *lidx = nullptr;
  sdm_world_object *table = nullptr;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  size_t cap_arch = 0, cap_bricks = 0, cap_cells = 0, cap_objects = 0;
  uint32_t n = 0, hmask = 0, n_roots = 0, stamp = 0;
  int32_t min_cells = 0;
  int64_t n_cells = 0, max_cells = 0;
  bool over = false;
};

// world changes (world_changes.hip): a snapshot of where the block and the archive disagree.  Per candidate brick of the
// block (cap_cand, the map's largest candidate count) the flag "has a listed cell", its rank in the field, the archive's pool
// slot and the eight listed words with the two bit planes of the class - the build's own; per brick of the field
// (cap_bricks) its coordinates, the pool slot and the ranks of the 27 bricks round it (the build's own), the listed words,
// their prefix and the class planes, and the hash table from brick key to rank (hmask + 1 slots in use) - what the query
// reads.  Per listed cell (cap_cells) the world cell, the block's and the archive's word, the key, the class, parent (the
// region index in the end), root and the scanned root flags; per region (cap_regions) the accumulator (empty between
// builds), the index of its first cell, the scanned listing flags and the table.  The build's counters and per-label
// counters (and their page-locked landing area, whose last word takes a count the build waits for), its arguments, the
// frame's and the archive's stamp; over: the build found more cells than max_cells and wrote no list.  Every buffer is
// grown by the build that needs more.
struct WorldChangesLayer : Derived {
  uint32_t *flag = nullptr, *rank = nullptr, *cslot = nullptr;
  unsigned long long *lw_c = nullptr, *p0_c = nullptr, *p1_c = nullptr;
  uint32_t *coord = nullptr, *slot_of = nullptr, *nbr = nullptr, *pre = nullptr, *vals = nullptr;
  unsigned long long *cw = nullptr, *c0 = nullptr, *c1 = nullptr, *keys = nullptr;
  int32_t *xyz = nullptr;
  uint32_t *now = nullptr, *before = nullptr, *key = nullptr, *parent = nullptr, *root = nullptr, *idx = nullptr;
  uint8_t *cls = nullptr;
  unsigned char *acc = nullptr;
  uint32_t *first = nullptr, *lidx = nullptr;
  sdm_world_change_region *table = nullptr;
  unsigned long long *meta = nullptr, *h_meta = nullptr;
  size_t cap_cand = 0, cap_bricks = 0, cap_cells = 0, cap_regions = 0;
  uint32_t n = 0, hmask = 0, n_roots = 0, n_candidates = 0, stamp = 0, frame_stamp = 0;
  int32_t min_cells = 0;
  int64_t n_cells = 0, max_cells = 0;
  bool over = false;
};

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
    size_t obj_masks_cap = 0;  // bytes
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
  // the derived layers (Derived and the structs behind it, above): nothing of the frame reads or writes them
  QueryStage stage;
  EsdfLayer esdf;
  InstLayer inst;
  FrontLayer front;
  ViewPool views;
  ReachLayer reach;
  ForecastLayer forecast;
  GroundLayer ground;
  MeshLayer mesh;
  WorldLayer world;
  WorldReachLayer wreach;
  WorldFrontiersLayer wfront;
  WorldEsdfLayer wesdf;
  WorldGroundLayer wground;
  WorldGroundReachLayer wgreach;
  WorldRaysPool wrays;
  WorldMatchPool wmatch;
  WorldMeshLayer wmesh;
  WorldObjectsLayer wobj;
  WorldChangesLayer wchg;
  // the scan scratch the layers share (layer_scan_scratch): they all enqueue on `stream` only, so their scans are ordered
  uint32_t *layer_scan = nullptr;
  size_t layer_scan_elems = 0;  // its capacity in uint32
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
  bool stage_ran[9]{};
  // What the map owns, released by sdm_destroy: device memory, page-locked host memory, events (alloc_tracked, regrow,
  // new_event below).  The kernels take the raw pointers by value (State / Scratch), so the fields above stay raw; a field
  // that is null is simply not allocated yet.  Streams, graph executables, the communicator and the peers' arena mappings
  // are not in these lists: the order in which they go matters (sdm_destroy, drop_graphs, exchange_teardown).
  std::vector<void *> allocs, pinned;
  std::vector<hipEvent_t> events;
};

namespace sdm {

// ---- who owns what (lifecycle.hip) -----------------------------------------------------------------------------------
sdm_status map_alloc(sdm_map *m, void **p, size_t bytes, bool pinned);  // *p: fresh memory, registered with the map
void map_release(sdm_map *m, void **p);                                 // *p (registered, or null) is freed and cleared
sdm_status new_event(sdm_map *m, hipEvent_t *e, unsigned flags);        // created and registered
template <typename T>
sdm_status alloc_tracked(sdm_map *m, T **p, size_t n, bool pinned = false) {
  return map_alloc(m, (void **)p, std::max<size_t>(n, 1) * sizeof(T), pinned);
}
template <typename T>
void release(sdm_map *m, T **p) {
  map_release(m, (void **)p);
}
// A buffer that grows on demand: the old one goes - once `quiet`, a stream that may still be using it, has drained - and
// one of n elements comes; *cap is what the caller compares its need with (0 while there is no buffer).
template <typename T>
sdm_status regrow(sdm_map *m, T **p, size_t *cap, size_t n, hipStream_t quiet = nullptr, bool pinned = false) {
  if (quiet) HIP_TRY(hipStreamSynchronize(quiet));
  *cap = 0;
  release(m, p);
  SDM_TRY(alloc_tracked(m, p, n, pinned));
  *cap = n;
  return SDM_OK;
}
// device temporaries of one call: freed on every exit from it
struct DevTemps {
  std::vector<void *> v;
  template <typename T>
  hipError_t alloc(T **p, size_t n) {
    const hipError_t e = hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) v.push_back((void *)*p);
    return e;
  }
  ~DevTemps() { for (void *p : v) (void)hipFree(p); }
};

// ---- host helpers shared between the units ---------------------------------------------------------------------------
inline bool stage_done(int32_t stop_after, int stage) { return stop_after != 0 && stop_after <= stage; }
// lifecycle.hip
enum { GRAPH_PIECES = 0, GRAPH_BRANCHED = 1, GRAPH_CHAIN = 2 };  // sdm_map::graph_shape
void issue_mode_for(const sdm_map *m, int mode, bool *use_graph, int *shape);  // SDM_GRAPH / sdm_set_issue_mode -> how frames are issued
hipError_t lazy_stream(int device, hipStream_t *s);
void refresh_filter(sdm_map *m);
void update_ego_center(sdm_map *m, const float pos[3]);
void compute_extrinsic(sdm_map *m, const float pos[3], const float q[4]);
void compute_frustum_box(sdm_map *m);
void sync_frame_scalars(sdm_map *m);
sdm_status upload_stamps(sdm_map *m);
int sweep_mode(const sdm_map *m);
sdm_status sweep_mode_latch(sdm_map *m);
sdm_status check_counters(sdm_map *m, Counters *out);
// affinity.cpp
int bind_host_thread_to(int device);
// frame.hip
void drop_graphs(sdm_map *m);  // whatever was captured goes (the caller has made sure that none of it is running)
// exchange.hip
sdm_status exchange_counts(sdm_map *m, hipStream_t s);  // the all-gather of the member-count rows: RCCL or the peers' arenas
sdm_status exchange_check(sdm_map *m);                  // (m->stream is idle) did an exchange through the arenas time out?
sdm_status exchange_wait(sdm_map *m);                   // sdm_synchronize with a communicator: a bounded wait for the map's streams
void exchange_teardown(sdm_map *m);                     // communicator, arena, peer mappings, exchange buffers: back to "none"
// ---- the derived layers' shared host side (queries.hip) ---------------------------------------------------------------
sdm_status query_check(sdm_map *m, const void *in, int64_t n, const void *out, uint32_t flags, uint32_t allowed, const char *what);
// How a layer's two refusals name it: "<the_layer> of a Z-slab shard ... is / are not supported: build it / them on a
// whole map" and "no <build>: call <update> first".
struct LayerName {
  const char *the_layer, *build, *update;
  bool plural;
};
// The scratch of every scan a layer runs on m->stream: at least scan_scratch_elems(longest) words that honour the scan's
// contract (sdm_internal.h).  Allocated and zeroed at first use; regrown, once the stream has drained, and zeroed again
// only when a caller asks for a longer one - so a layer passes the longest scan it can ever run on this map.
sdm_status layer_scan_scratch(sdm_map *m, size_t longest, uint32_t **scratch);
// The check of every entry point of a layer: no Z-slab shards, and - `need` given - that layer must hold a build.
sdm_status layer_check(sdm_map *m, const char *what, const Derived *need, const LayerName &name);
// the global position of the min corner of cell (0, 0, 0) of the frame layer `l` was built from (origin may be null)
void layer_origin(const sdm_map *m, const Derived &l, float origin[3]);
// Host mode works through `n` items in chunks, through the map's staging area (sdm_map::stage): `pre` goes up once (the
// views' ray table); per chunk every input column is copied up, launch(pre, col, count) enqueues the items on m->stream
// (device addresses; col[k] null: no such column), every output column is fetched, and after one wait copied out -
// then copy_out(col, off, count), if given, sees the fetched columns of items [off, off + count).
struct StageCol {
  enum Kind { IN, OUT, OUT_RAW } kind;  // OUT_RAW: fetched like OUT, left to copy_out
  void *host;                           // the caller's array (IN: only read)
  size_t elem;                          // bytes per item; 0: the call has no such column
};
using StageLaunch = std::function<sdm_status(const unsigned char *pre, unsigned char *const *col, size_t count)>;
using StageCopyOut = std::function<void(const unsigned char *const *col, size_t off, size_t count)>;
sdm_status run_staged(sdm_map *m, size_t n, size_t chunk, const void *pre, size_t pre_bytes, const std::vector<StageCol> &cols,
                      const StageLaunch &launch, const StageCopyOut &copy_out = nullptr);
// The calls of one input and one or two outputs per item, host or device mode, in chunks of 2^20:
// launch(in, out, out2, count, stream) enqueues one chunk; out2 (may be null) is a second output array
using QueryLaunch = std::function<void(const void *, void *, void *, uint32_t, hipStream_t)>;
sdm_status run_query(sdm_map *m, const void *in_v, size_t in_elem, void *out_v, size_t out_elem, void *out2_v, size_t out2_elem, int64_t n,
                     uint32_t flags, const QueryLaunch &launch);

}  // namespace sdm
