/*
 * sdm.h — C ABI of libsdm_hip: the MI355X-native particle-grid update of
 * tud-amr/semantic_dsp_map (hot path only).
 *
 * The library replaces the private sub-object level of the reference's
 * SemanticDSPMap class; each entry point cites the reference interface it stands
 * in for (paths relative to the reference's include/).  The header-only adapter
 * include/semantic_dsp_map.h puts the reference's own class and method
 * signatures back on top of these calls.
 *
 * Conventions: plain C, caller owns every pointer, nothing is retained after a
 * call returns, no exceptions cross the boundary, every function returns an
 * sdm_status (0 = ok).  One map per handle (the reference allows one per
 * process: its map is a set of header-defined globals, mc_ring/buffer.h:86-120).
 * Calls on one handle must come from one thread at a time (the reference is
 * single-threaded, src/mapping.cpp:156).
 */
#ifndef SDM_H_
#define SDM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdm_map sdm_map;

typedef enum {
  SDM_OK = 0,
  SDM_ERR_INVALID_ARGUMENT = 1, /* bad config / null pointer / size mismatch          */
  SDM_ERR_NO_DEVICE = 2,        /* no HIP device, or the requested ordinal is missing */
  SDM_ERR_HIP = 3,              /* a HIP runtime call failed (sdm_last_error has text)  */
  SDM_ERR_CAPACITY = 4,         /* a per-frame work list overflowed its capacity      */
  SDM_ERR_NOT_CONVERGED = 5,    /* frustum flood fill needed more rounds than budgeted */
  SDM_ERR_COMM = 6              /* multi-GPU exchange failed                           */
} sdm_status;

/* Compile-time constants of the reference (settings/settings.h:18-150:
 * C_VOXEL_NUM_AXIS_*_N, C_MAX_PARTICLE_NUM_PER_VOXEL_N, C_VOXEL_SIZE, g_camera_*,
 * g_image_*, g_depth_range_*, BOOST_MODE window) as run-time configuration. */
typedef struct {
  int32_t x_n, y_n, z_n;      /* log2 voxels per axis (x_n+y_n+z_n+p_n <= 31, operations.h:54-58) */
  int32_t p_n;                /* log2 slots per voxel, 1..4; slot 0 is the time particle         */
  float voxel_size;           /* metres                                                           */
  float fx, fy, cx, cy;       /* pinhole intrinsics                                               */
  int32_t width, height;      /* image size                                                       */
  float depth_min, depth_max; /* metres                                                           */
  int32_t window_half;        /* SMC-PHD neighbour half-size: 5, or 3 in BOOST mode (semantic_dsp_map.h:964-970) */
  int32_t max_movable_track;  /* g_max_movable_object_instance_id (utils/data_base.h:196)         */
  int32_t device;             /* HIP device ordinal                                               */
  int32_t shard_rank;         /* Z-slab sharding: this process owns ring-z slab shard_rank of shard_count */
  int32_t shard_count;        /* 1 = whole map on one GPU                                         */
  int64_t max_visible;        /* capacity of the per-frame visible-particle list, 0 = default     */
} sdm_config;

/* SemanticDSPMap::setMapParameters / setMapOptions / setDepthNoiseModelParameters
 * (semantic_dsp_map.h:101-125, 161-166).  Field spelling follows the reference. */
typedef struct {
  float detection_probability;
  float noise_number;
  int32_t nb_ptc_num_per_point;
  float occupancy_threshold;
  int32_t max_obersevation_lost_time;
  float forgetting_rate;
  int32_t max_forget_count;
  float match_score_threshold;
  float id_transition_probability;
  int32_t if_consider_depth_noise;
  int32_t if_use_independent_filter;
  float depth_noise_first_order;
  float depth_noise_zero_order;
} sdm_params;

/* LabeledPoint (utils/data_base.h:78-92): position in the global frame, sigma,
 * track id, label id, validity.  20 bytes, same field order. */
typedef struct {
  float x, y, z;
  float sigma;
  uint16_t track_id;
  uint8_t label_id;
  uint8_t is_valid;
} sdm_labeled_point;

/* One rigid-body motion handed down by the object layer: the track id and
 * rigidbody_tmatrix_vec[0] cast to float (semantic_dsp_map.h:673-679), row-major. */
typedef struct {
  int32_t track_id;
  float T[16];
} sdm_object_move;

/* Per-voxel result of determineIfVoxelOccupied (mc_ring/operations.h:623-639),
 * indexed by storage voxel index.  8 bytes. */
typedef struct {
  float wsum;     /* weight sum, -1 = unknown voxel                       */
  uint16_t track; /* winning track id (0 if none)                          */
  uint8_t label;  /* its label id                                          */
  int8_t occ;     /* -1 unknown, 0 free, 1 occupied, 2 guessed occupied    */
} sdm_voxel_result;

/* One emitted voxel of getOccupancyResult (semantic_dsp_map.h:1239-1383): min-corner
 * position (global frame, or camera-centred) and the raw semantics; colouring stays
 * in the adapter. 16 bytes. */
typedef struct {
  float x, y, z;
  uint16_t track;
  uint8_t label;
  int8_t occ;
} sdm_point;

/* What one block of kernel arguments holds of the object lists.  Every entry point takes lists of ANY length (whole maps:
 * round 5; Z-slab shards: round 6): they are worked off in batches of this size inside the frame - every object's
 * particles are taken out before any is re-inserted and the noise draws run on across the batches, like
 * moveParticlesInSetsByTransformations does it (mc_ring/operations.h:321-362); a frame with longer lists is issued launch
 * by launch, not from the captured graph.  On a Z-slab shard every batch's per-object member counts are exchanged before
 * the batch is applied: sdm_update_sharded does that itself, the split entry points through sdm_frame_moves_pending. */
#define SDM_MAX_MOVES 48
#define SDM_MAX_REMOVALS 128

/* sdm_update flags */
#define SDM_INPUT_ON_DEVICE 0x1u /* depth / cloud are device pointers already resident in HBM */
#define SDM_SKIP_OCCUPANCY 0x2u  /* do not run the occupancy sweep (debug)                     */
#define SDM_NO_INSTANCES 0x4u    /* sdm_update_raw: ignore the object masks (g_consider_instance == false, settings.h:49) */

/* stage ids (also indices of sdm_stats.stage_ms): the reference's own stage timers,
 * semantic_dsp_map.h:916-921 */
enum {
  SDM_STAGE_ALL = 0,
  SDM_STAGE_EGO = 1,
  SDM_STAGE_MOVE = 2,
  SDM_STAGE_REMOVE = 3,
  SDM_STAGE_VISIBILITY = 4,
  SDM_STAGE_WEIGHT = 5,
  SDM_STAGE_BIRTH = 6,
  SDM_STAGE_OCCUPANCY = 7
};

typedef struct {
  uint32_t global_time_stamp;
  int32_t moved_steps[3];
  int32_t eq_steps[3];
  float map_center[3];
  float last_pos[3];
  int32_t birth_cursor;
  int32_t move_cursor;
} sdm_ring_state;

typedef struct {
  int64_t live_particles;   /* filled by sdm_get_stats(…, count_live=1) only */
  int64_t n_visible;
  int64_t n_birth_attempts;
  int64_t n_birth_success;
  int64_t n_resampled_voxels;
  int64_t n_moved;          /* particles of moving objects the last update copied, over the whole map (every shard). At most
                               min(slots of the whole map, 2^18) per frame, whatever shard_count is; more: SDM_ERR_CAPACITY */
  int64_t n_move_reinserted;
  int64_t n_frustum_voxels;
  int64_t n_occupied;
  int64_t flood_rounds;
  int64_t bfs_start_in_frustum;
  int64_t live_voxels;      /* observed voxels holding a live slot (count_live=1) */
  int64_t sweep_live_voxels; /* voxels the last occupancy sweep evaluated in full: the ones written to since the sweep before */
  int64_t sweep_tiles;      /* 2048-voxel tiles the last occupancy sweep looked into (something in them was written or stamped) */
  double stage_ms[8];       /* GPU time per stage of the last update when profiling is on */
  int64_t restamped_slabs[3]; /* slabs the last update's ring shift re-stamped, per axis (x, y, z) */
  int64_t graph_frames;     /* frames replayed from the captured hipGraph so far ...                       */
  int64_t direct_frames;    /* ... and frames issued launch by launch                                      */
  double host_enqueue_us;   /* host time to issue 50 empty kernel launches (a frame's worth), measured at sdm_create */
  int64_t halo_dropped;     /* sharded maps: slab-crossing copies of the last update beyond the export capacity towards their
                               destination shard (dropped; SDM_ERR_CAPACITY at the next sdm_synchronize) */
  int64_t alias_entries;    /* indices that sit in a second owner set besides their latest one (the reference's sets are real
                               sets, object_layer.h:20-52), as of now - deleted entries included until the next frame's
                               garbage collection */
  int64_t alias_overflowed; /* 1 = that table has overflowed (65536 entries) since the last sdm_clear / sdm_load_state: the
                               sets are incomplete, SDM_ERR_CAPACITY is reported at every synchronisation from then on */
} sdm_stats;

/* ---- host placement.  A frame is a chain of ~50 dependent launches; the command processor fetches every packet and
 * signals every completion through host memory the HIP runtime allocates where the calling thread runs.  From the
 * socket the GPU does not hang off, every gap between two dependent kernels is 2-4 us longer (C3 frame: 0.292 against
 * 0.265 ms).  sdm_bind_host_thread moves the CALLING thread (and the threads it starts afterwards) onto the NUMA node
 * of `device`, within the CPUs the process may use, and returns that node (-1: nothing to do - one node, no sysfs entry,
 * no allowed CPU there).  Best called first thing in the process, before any other HIP call: it finds the node in sysfs
 * (KFD topology) without touching the runtime, so that the runtime's first allocations land on the right node too; only
 * when sysfs cannot tell does it ask HIP for the device's PCI address.
 * sdm_create calls it for its device unless SDM_NUMA_BIND=0 is set in the environment. */
int32_t sdm_bind_host_thread(int32_t device);
/* The NUMA node of HIP device `device` found WITHOUT the HIP runtime (KFD topology in sysfs + the *_VISIBLE_DEVICES index
 * lists), which is what sdm_bind_host_thread tries first: -2 if that cannot tell (it then asks HIP, i.e. brings the runtime
 * up before the thread is moved). */
int32_t sdm_host_numa_node_early(int32_t device);

/* ---- life cycle: SemanticDSPMap() / ~SemanticDSPMap() / clear() (semantic_dsp_map.h:25-81),
 * RingBufferOperations::initialize / clear (mc_ring/operations.h:684-767) */
sdm_status sdm_create(const sdm_config *cfg, sdm_map **out);
sdm_status sdm_destroy(sdm_map *m);
sdm_status sdm_clear(sdm_map *m);

/* ---- setters (semantic_dsp_map.h:101-166) */
sdm_status sdm_set_params(sdm_map *m, const sdm_params *p);

/* ---- Gaussian noise table, GaussianRandomCalculator::calculateGaussianTable
 * (utils/basic_algorithms.h:394-402): n floats ~ N(0, stddev^2).  Either generated on
 * the device with rocRAND (Philox4x32-10) or uploaded by the caller. */
sdm_status sdm_generate_noise_table(sdm_map *m, uint64_t seed, int32_t n, float stddev);
sdm_status sdm_upload_noise_table(sdm_map *m, const float *table, int32_t n);
sdm_status sdm_download_noise_table(sdm_map *m, float *table, int32_t n);
/* standard_gaussian_pdf (basic_algorithms.h:405-407), 20000 floats, for cross-checks */
sdm_status sdm_download_pdf_table(sdm_map *m, float *table, int32_t n);

/* ---- the hot path: one call of SemanticDSPMap::subObjectLevelUpdate
 * (semantic_dsp_map.h:576-955) preceded by global_time_stamp += 1 (:173).
 *   depth          H*W float32 metres (cv::Mat CV_32FC1, src/mapping.cpp:180)
 *   cloud          H*W labeled points (output of generateLabeledPointCloud, :227)
 *   cam_pos,cam_q  camera pose in the global frame, q = (w,x,y,z), already cast to float (:584, :745-746)
 *   moves          objects the object layer decided to move this frame (:593-693), caller's order
 *   remove_tracks  lost / floating objects to wipe (:702-736)
 *   stop_after     SDM_STAGE_ALL, or a stage id to stop after (parity debugging)
 * Asynchronous: returns after enqueueing; results are fetched with the getters below.
 * How the frame's ~50 kernels are issued follows the host's speed at issuing launches, measured in sdm_create
 * (sdm_stats.host_enqueue_us): launch by launch on a fast host, replayed from hipGraphs on a slow one.  The environment
 * variable SDM_GRAPH forces one way (0 launch by launch, 4 five chain graphs, 3 one chain graph, 1 one branched graph;
 * read when the map is created), and so does sdm_set_issue_mode at any time between frames; the results are
 * bit-identical. */
#define SDM_ISSUE_LAUNCHES 0   /* launch by launch */
#define SDM_ISSUE_BRANCHED 1   /* one hipGraph, frustum and birth chains as branches */
#define SDM_ISSUE_AUTO 2       /* by the host's measured speed (the default) */
#define SDM_ISSUE_CHAIN 3      /* one hipGraph, a chain of kernel nodes */
#define SDM_ISSUE_PIECES 4     /* five chain hipGraphs on the frame's streams */
/* mode: one of SDM_ISSUE_*.  Graphs captured for another mode are dropped; the next plain frame captures anew. */
sdm_status sdm_set_issue_mode(sdm_map *m, int32_t mode);
sdm_status sdm_update(sdm_map *m, const float *depth, const sdm_labeled_point *cloud,
                      const float cam_pos[3], const float cam_q[4],
                      const sdm_object_move *moves, int32_t n_moves,
                      const int32_t *remove_tracks, int32_t n_remove,
                      uint32_t flags, int32_t stop_after);

/* ---- the step right before the path, PointCloudTools::generateLabeledPointCloud
 * (utils/pointcloud_tools.h:88-310, general non-BOOST / non-ZED2 path), on the device.  Instead of the 20-byte
 * LabeledPoint image the caller hands over what the reference's update() receives: the depth image, the "static" MONO8
 * mask (pixel value + 1 = label id, :137-138; NULL = every pixel Background/65535, :147-156) and one MONO8 mask per
 * movable object (> 0 = object, later entries override earlier ones, :163-213), plus the camera pose in double
 * (the reference back-projects in double and casts to float, :243-249, 298-300).
 * label_to_static_instance[256]: instance id of a static label id (g_label_to_instance_id_map_default), 65535 for
 * label ids without one.  Every mask is H*W bytes, host memory (or device memory with SDM_INPUT_ON_DEVICE). */
typedef struct {
  int32_t track_id;    /* <= max_movable_track */
  int32_t label_id;    /* g_label_id_map_default[label] */
  const uint8_t *mask; /* H*W, > 0 = object */
} sdm_instance_mask;
sdm_status sdm_update_raw(sdm_map *m, const float *depth, const uint8_t *static_mask,
                          const uint16_t label_to_static_instance[256],
                          const sdm_instance_mask *objects, int32_t n_objects,
                          const double cam_pos[3], const double cam_q[4],
                          const sdm_object_move *moves, int32_t n_moves,
                          const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after);
/* Preset-specific parts of generateLabeledPointCloud:
 *  - BOOST mode (settings.h:26, 137-143): depth and masks arrive at src_width x src_height and are reduced by `rescale`
 *    with the reference's nearest-neighbour manualResize (pointcloud_tools.h:1104-1133); int(src * rescale) must equal
 *    the configured width / height.  src_width = 0: inputs already have the configured size.
 *  - ZED2 (SETTING 3): pixels whose track id is sky_instance are invalid (:236-242); object_bbox (n_objects x 6
 *    doubles: min x, max x, min y, max y, min z, max z of the object's current key points +- 1 m, global frame,
 *    :174-196) turns points of a movable instance that lie outside their object's box into Background (:254-272).
 *    An id below max_movable_track that no object carries - it can only come out of label_to_static_instance - has
 *    the all-zero box, as in the reference, also in a frame without objects: hand a non-NULL object_bbox with
 *    n_objects == 0 to keep the filter on there (it is not read).
 *    sky_instance < 0 / object_bbox NULL: off.
 * The label of a pixel with a movable id (<= max_movable_track) is the label_id of the LAST object with that track_id,
 * whether or not that object's mask covers the pixel (track_to_label_id_map, :168, :281); 0 if no object has the id. */
typedef struct {
  int32_t src_width, src_height;
  float rescale;
  int32_t sky_instance;
  const double *object_bbox;
} sdm_raw_options;
sdm_status sdm_update_raw_ex(sdm_map *m, const float *depth, const uint8_t *static_mask,
                             const uint16_t label_to_static_instance[256],
                             const sdm_instance_mask *objects, int32_t n_objects,
                             const double cam_pos[3], const double cam_q[4],
                             const sdm_object_move *moves, int32_t n_moves,
                             const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after,
                             const sdm_raw_options *opt);
/* the LabeledPoint image sdm_update_raw generated for the last frame (H*W entries), for cross-checks */
sdm_status sdm_get_labeled_cloud(sdm_map *m, sdm_labeled_point *out);

/* The same frame split at its one cross-shard dependency: sdm_update_begin runs the
 * prediction, visibility/binning and this shard's partial ck image (pass 1 of updateParticles,
 * semantic_dsp_map.h:973-1037) and hands back its device pointer; the partial images of all Z-slab shards are summed
 * IN SLAB ORDER (see sdm_ck_reduce for the exchange that does it with 2 (G-1)/G images of traffic) and the result goes
 * to sdm_update_finish, which forms ck+kappa, updates the weights and runs births, resampling and the occupancy sweep.
 * sdm_update_finish accepts either n_parts whole partial images in slab order (it adds them itself) or, with
 * n_parts = 1, the image already summed.  sdm_update == begin + finish with the shard's own image. */
sdm_status sdm_update_begin(sdm_map *m, const float *depth, const sdm_labeled_point *cloud,
                            const float cam_pos[3], const float cam_q[4],
                            const sdm_object_move *moves, int32_t n_moves,
                            const int32_t *remove_tracks, int32_t n_remove,
                            uint32_t flags, int32_t stop_after, const float **ck_part_dev);
sdm_status sdm_update_finish(sdm_map *m, const float *ck_parts_dev, int32_t n_parts, uint32_t flags,
                             int32_t stop_after);
/* sdm_update_begin itself in three steps, for sharded maps whose moving objects cross slab borders
 * (moveParticlesInSetsByTransformations, mc_ring/operations.h:321-362, needs the other shards twice):
 *   sdm_frame_start   -> all-gather of the per-object member counts (SDM_HALO_OBJ int32 per shard)
 *   sdm_frame_moves   -> all-to-all of the export segments: a copy whose target voxel lies in another slab goes to
 *                        the shard that owns that slab, and to nobody else
 *   sdm_frame_predict -> chunk-owner exchange of the partial ck images (below) -> sdm_update_finish
 * The exchange buffers are device memory owned by the caller and registered once with sdm_set_halo_buffers:
 *   counts_local  SDM_HALO_OBJ int32                      counts_all  shard_count x SDM_HALO_OBJ int32 (gathered)
 *   send, recv    shard_count segments of SDM_HALO_HEADER_BYTES + cap_records x SDM_HALO_RECORD_BYTES each; segment d of
 *                 send is addressed to shard d, segment s of recv is what shard s addressed to this one.
 * cap_records is the capacity PER DESTINATION; more slab-crossing copies towards one shard in one frame than that is a
 * capacity error (SDM_ERR_CAPACITY at the next sdm_synchronize; the copies beyond it are dropped like copies whose
 * target voxel is full, mc_ring/operations.h:357). */
#define SDM_HALO_OBJ 64
#define SDM_HALO_RECORD_BYTES 36
#define SDM_HALO_HEADER_BYTES 16
#define SDM_HALO_DEFAULT_CAP 4096
sdm_status sdm_frame_start(sdm_map *m, const float *depth, const sdm_labeled_point *cloud,
                           const float cam_pos[3], const float cam_q[4],
                           const sdm_object_move *moves, int32_t n_moves,
                           const int32_t *remove_tracks, int32_t n_remove, uint32_t flags, int32_t stop_after);
sdm_status sdm_frame_moves(sdm_map *m);
/* More than SDM_MAX_MOVES moving objects on a Z-slab shard: sdm_frame_moves applies ONE batch and, if objects are left,
 * issues the next batch's member count and publishes its per-object counts in counts_local; *pending = 1 then says: gather
 * the count rows once more (the same all-gather as behind sdm_frame_start) and call sdm_frame_moves again.  The export
 * segments collect the copies of all batches; they are exchanged once, when nothing is pending any more. */
sdm_status sdm_frame_moves_pending(sdm_map *m, int32_t *pending);
sdm_status sdm_frame_predict(sdm_map *m, const float **ck_part_dev);
sdm_status sdm_set_halo_buffers(sdm_map *m, int32_t *counts_local, const int32_t *counts_all, void *send,
                                const void *recv_all, int32_t cap_records);
/* the HIP stream (hipStream_t) all work of this map is enqueued on; sdm_set_stream moves the map onto a
 * caller-owned stream (e.g. the one RCCL collectives are issued on, so that no host sync is needed between
 * sdm_update_begin, the all-gather and sdm_update_finish); NULL restores the map's own stream. */
sdm_status sdm_stream(sdm_map *m, void **stream_out);
sdm_status sdm_set_stream(sdm_map *m, void *hip_stream);
/* caller-provided device buffer that sdm_update_begin writes this shard's partial ck image to (H*W floats; for the
 * chunk-owner exchange shard_count x sdm_ck_chunk_elems floats, the image padded to whole chunks); NULL restores the
 * internal buffer. */
sdm_status sdm_set_ck_buffer(sdm_map *m, float *dev_buffer);
/* Chunk-owner exchange of the partial ck images: the image is cut into shard_count chunks of `chunk` pixels
 * (sdm_ck_chunk_elems: ceil(H*W / shard_count) rounded up to 64), shard r owns chunk r.
 *   1. all-to-all: chunk d of every shard's partial image goes to shard d  -> stage (shard_count x chunk floats, part s
 *      from shard s)
 *   2. sdm_ck_reduce: the owner adds the parts in slab order (the float sums a single map split into the same slabs
 *      forms, oracle `ck_slabs`) into chunk `shard_rank` of full (shard_count x chunk floats)
 *   3. all-gather of the summed chunks (in place on full)               -> sdm_update_finish(m, full, 1, ...)
 * 2 (G-1)/G images received per shard instead of the G-1 whole images of a plain all-gather. */
sdm_status sdm_ck_chunk_elems(sdm_map *m, int64_t *chunk_out);
sdm_status sdm_ck_reduce(sdm_map *m, const float *stage_dev, float *full_dev);

/* ---- native multi-GPU path: RCCL over xGMI, one process per GPU.  Rank 0 draws an id, the caller hands it to
 * every rank (any out-of-band channel), every rank calls sdm_comm_init on its shard map (collective), then
 * sdm_update_sharded runs whole frames: the exchanges above are issued on the map's streams, nothing waits on the host. */
sdm_status sdm_comm_unique_id(uint8_t out[128]);
/* halo_cap_records: capacity per destination shard of the export segments, 0 = SDM_HALO_DEFAULT_CAP */
sdm_status sdm_comm_init(sdm_map *m, const uint8_t id[128], int32_t halo_cap_records);
/* The same exchanges WITHOUT RCCL, through peer-mapped memory (xGMI is point to point: a shard writes its pieces straight
 * into the peers' HBM and raises a flag; one small kernel per exchange, no collective launch, no host call but that).
 * sdm_ipc_create allocates this shard's receive arena and returns its hipIpc handle (64 bytes); the caller gathers the
 * handles of all shards - any transport, the order is the shard order - and sdm_ipc_connect maps the peers' arenas.
 * sdm_update_sharded then runs on them (sdm_comm_init is not needed; a map uses one or the other).  A shard that is missing
 * or out of step: SDM_ERR_COMM at the next sdm_synchronize, after SDM_COMM_TIMEOUT_MS (sdm_comm_set_options(m, -1, ms)). */
sdm_status sdm_ipc_create(sdm_map *m, int32_t halo_cap_records, uint8_t handle_out[64]);
sdm_status sdm_ipc_connect(sdm_map *m, const uint8_t *handles_all);
/* How sdm_update_sharded combines the shards' partial ck images, and how long sdm_synchronize waits for a sharded frame.
 * ck_exchange: 0 = chunk-owner reduction (all-to-all of the chunks to their owners, slab-ordered sum there, all-gather of the
 * summed chunks: 2 (G-1)/G images received, two collectives on the critical path; the default), 1 = ONE all-gather of the
 * whole partial images and the slab-ordered sum on every shard (G-1 images received, one collective), -1 = leave as it is
 * (environment: SDM_CK_EXCHANGE=allgather).  Both form the same float sums.  All shards must choose alike.
 * timeout_ms > 0: bound of sdm_synchronize's wait (default 30000, SDM_COMM_TIMEOUT_MS): beyond it - a peer died or fell out
 * of step - the communicator is aborted and SDM_ERR_COMM returned instead of hanging. */
sdm_status sdm_comm_set_options(sdm_map *m, int32_t ck_exchange, int32_t timeout_ms);
sdm_status sdm_update_sharded(sdm_map *m, const float *depth, const sdm_labeled_point *cloud,
                              const float cam_pos[3], const float cam_q[4],
                              const sdm_object_move *moves, int32_t n_moves,
                              const int32_t *remove_tracks, int32_t n_remove, uint32_t flags);
/* HIP events around the four collectives of sdm_update_sharded frames; sdm_get_comm_times waits for the last frame and
 * returns their GPU times in microseconds: [0] member counts (all-gather), [1] slab-crossing copies (all-to-all),
 * [2] partial ck chunks to their owners (all-to-all), [3] summed ck chunks (all-gather); 0 for one the frame did not
 * issue.  The time of a collective includes waiting for the slowest shard to arrive at it. */
sdm_status sdm_comm_timing(sdm_map *m, int32_t on);
sdm_status sdm_get_comm_times(sdm_map *m, double out_us[4]);

/* ---- plain device buffers (for frames kept resident in HBM, see SDM_INPUT_ON_DEVICE) */
/* page-locked host memory for input buffers (uploads then run at PCIe speed, beside the previous frame's kernels) */
sdm_status sdm_host_alloc(size_t bytes, void **out);
sdm_status sdm_host_free(void *p);
sdm_status sdm_device_alloc(sdm_map *m, size_t bytes, void **out);
sdm_status sdm_device_free(sdm_map *m, void *p);
sdm_status sdm_device_upload(sdm_map *m, void *dst_dev, const void *src_host, size_t bytes);
sdm_status sdm_device_download(sdm_map *m, void *dst_host, const void *src_dev, size_t bytes);
sdm_status sdm_device_synchronize(sdm_map *m);

/* Wait for all enqueued work of this map; surfaces deferred device-side errors. */
sdm_status sdm_synchronize(sdm_map *m);

/* ---- results (getOccupancyResult, semantic_dsp_map.h:1239-1383) */
/* all voxels in storage order; out has 2^(x_n+y_n+z_n) entries (this shard's slab if sharded) */
sdm_status sdm_get_voxels(sdm_map *m, sdm_voxel_result *out);
/* compacted list of voxels with occ > 0 (occupied) or occ == 0 (free) in increasing storage index.
 * flags: SDM_POINTS_ZERO_CENTER subtracts the camera position (visualize_with_zero_center_, semantic_dsp_map.h:1263-1271);
 * SDM_POINTS_MARK_FOV adds SDM_OCC_OUT_OF_FOV to sdm_point.occ of voxels whose global position fails
 * checkIfPointInFrustum against the last frame's extrinsic (the test that selects the HSV dimming,
 * semantic_dsp_map.h:1339-1342). */
#define SDM_POINTS_ZERO_CENTER 0x1
#define SDM_POINTS_MARK_FOV 0x2
#define SDM_OCC_OUT_OF_FOV 0x40
sdm_status sdm_get_occupied(sdm_map *m, sdm_point *out, size_t cap, size_t *n_out, int32_t flags);
sdm_status sdm_get_freespace(sdm_map *m, sdm_point *out, size_t cap, size_t *n_out, int32_t flags);
/* ---- the same lists coloured and packed on the device, ready for the ROS message.
 * getOccupancyResult's colour rules (semantic_dsp_map.h:1274-1351): Background voxels by height through the jet map
 * (:50-63, :1277-1294), static instances (track id > max_movable_track, or every label when colour_by_label is set:
 * SETTING == 0) by their label colour (utils/data_base.h:216-232), movable ones (160, perm[track & 255], perm[label])
 * or, in evaluation format, (label, track >> 8, track & 255); guessed-occupied voxels white; free space green; outside
 * the evaluation format every colour then takes OpenCV's 8-bit RGB -> HSV -> RGB round trip with V x 0.7 for voxels
 * outside the camera frustum (:1333-1351; restated from OpenCV 4.x, see oracle/colour.py).
 * One point = pcl::PointXYZRGB's 32 bytes: x, y, z, 1.0f, then b, g, r, a = 255, then 12 bytes of padding. */
typedef struct {
  float x, y, z, one;
  uint8_t b, g, r, a;
  uint32_t pad[3];
} sdm_point_xyzrgb;
typedef struct {
  uint8_t label_bgr[256][3]; /* g_label_color_map_default, BGR like cv::Vec3b                       */
  uint8_t perm[256];         /* color_map_int_256_ (semantic_dsp_map.h:45-48)                         */
  int32_t background_label;  /* g_label_id_map_default["Background"]                                */
  int32_t colour_by_label;   /* SETTING == 0 (:1296-1302)                                            */
  int32_t jet_axis;          /* 0: jet index from -z + 2 (default), 1: from y + 2 (SETTING == 3)       */
  int32_t evaluation_format; /* if_out_evaluation_format_ (:130-134)                                 */
} sdm_colour_config;
sdm_status sdm_set_colours(sdm_map *m, const sdm_colour_config *c);
/* flags: SDM_POINTS_ZERO_CENTER as above (the frustum test always uses the uncentred position) */
sdm_status sdm_get_occupied_rgb(sdm_map *m, sdm_point_xyzrgb *out, size_t cap, size_t *n_out, int32_t flags);
sdm_status sdm_get_freespace_rgb(sdm_map *m, sdm_point_xyzrgb *out, size_t cap, size_t *n_out, int32_t flags);
/* device pointer to the per-voxel result array (valid until the next update) */
sdm_status sdm_voxels_device_ptr(sdm_map *m, const sdm_voxel_result **out);

/* ---- batched map queries (new; the reference has none: its map only fed the RViz cloud) ----
 * What a planner asks of the map - is this point, this path segment, this footprint free? - answered on the GPU from
 * the array sdm_get_voxels returns, read in stream order on the map's stream: the results of the last frame enqueued
 * before the call.  The caller never sees the storage layout (ring buffer, row-major storage index) and never holds a
 * pointer that goes stale.  Queries never modify map state, and use no scratch a frame uses.  Positions are in the
 * global frame.
 *
 * Flags: SDM_QUERY_ON_DEVICE - every input and output pointer is a device pointer; the call enqueues the kernel on the
 * map's stream (sdm_stream) and returns without waiting: the results are there after sdm_synchronize, or in stream
 * order.  The caller must have finished writing the inputs before the map's stream reaches the query (e.g. by writing
 * them on that stream, or synchronising its own stream first).  Without it, inputs and outputs are host memory: the
 * call copies the inputs up (in chunks, through a staging area the map grows on demand), runs the kernel, copies the
 * outputs down and waits.  SDM_QUERY_UNKNOWN_BLOCKS is for segments only.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map / input / output, n < 0, unknown flag bits, or a Z-slab shard
 * (shard_count > 1: routing queries to the slab owners is not implemented).  n == 0 is OK and launches nothing.
 *
 * Map-index coordinates of a position p: u = ((p - map_center) - map_p_min) / voxel_size, per axis, as the float32
 * expression the map itself uses ((p - center) - pmin) * (1 / voxel_size).  Cell (i, j, k) of the map is the box
 * [i, i+1) x [j, j+1) x [k, k+1) of u, inside the map for 0 <= i < NX etc. */
#define SDM_QUERY_ON_DEVICE 0x1u      /* inputs and outputs are device pointers; enqueued on the map's stream, no host wait */
#define SDM_QUERY_UNKNOWN_BLOCKS 0x2u /* segments: unknown voxels (occ == -1) and space outside the map block */

/* Points: out[i] = sdm_get_voxels()[voxel], bit for bit, where voxel is exactly the storage index the map would give a
 * particle at xyz[3i..3i+2] (operations.h:849-883 with the last frame's map center and ring offsets, including the
 * PINNED cast that accepts u in (-1, 0) as cell 0).  A point outside the map, or with a non-finite coordinate, gets
 * {wsum -1, track 0, label 0, occ -1} and voxel 0xffffffff.  voxel_out (n entries) may be NULL. */
sdm_status sdm_query_points(sdm_map *m, const float *xyz, int64_t n, sdm_voxel_result *out, uint32_t *voxel_out,
                            uint32_t flags);

/* Segments a -> b (ab[6i..6i+5] = ax ay az bx by bz) are traversed through the lattice of map cells in ascending t,
 * u(t) = u(a) + t (u(b) - u(a)), t in [0, 1], visiting the cells floor(u(t)) (a 3-D DDA, Amanatides-Woo); where two planes
 * are crossed at the same t, x steps before y before z.  NOTE: segments use floor, points the map's truncation - the
 * two differ only inside the one-voxel sliver below each lower map face (u in (-1, 0)), which is outside the map here.
 * A cell blocks if occ >= 1, or, with SDM_QUERY_UNKNOWN_BLOCKS, if occ == -1 or it lies outside the map.  Without the
 * flag, cells outside the map are skipped: the segment is clipped to the map first, so its cost is bounded by NX+NY+NZ
 * cells however long it is.  A zero-length segment is the cell of a.  A non-finite coordinate gives no hit and
 * cells = 0; with SDM_QUERY_UNKNOWN_BLOCKS it is a hit at t = 0 on voxel 0xffffffff. */
typedef struct {  /* 16 bytes */
  float t;        /* where the segment enters its first blocking cell, as a fraction of a->b in [0,1]; 0 if a lies in it;
                     -1 = nothing blocks */
  uint32_t voxel; /* storage index of that cell; 0xffffffff = outside the map, or no hit */
  int32_t cells;  /* in-map cells visited up to and including the hit (all of them if no hit) */
  uint16_t track; /* result of the blocking cell, as sdm_get_voxels holds it (0 / 0 / -1 if outside or no hit) */
  uint8_t label;
  int8_t occ;
} sdm_segment_hit;
sdm_status sdm_query_segments(sdm_map *m, const float *ab, int64_t n, sdm_segment_hit *out, uint32_t flags);

/* Boxes (boxes[6i..6i+5] = min x y z, max x y z): per axis the cells floor(u(min)) .. floor(u(max)) inclusive, intersected
 * with [0, N), counted by class.  A box with min > max on any axis, or with a non-finite coordinate, counts nothing
 * (all zero, first_occupied 0xffffffff, clipped 0). */
typedef struct {          /* 20 bytes; only cells inside the map are counted */
  int32_t n_occupied;     /* occ >= 1 */
  int32_t n_free;         /* occ == 0 */
  int32_t n_unknown;      /* occ == -1 */
  uint32_t first_occupied; /* smallest storage index among the occupied cells, 0xffffffff if none */
  int32_t clipped;        /* 1 if the box reaches outside the map */
} sdm_box_result;
sdm_status sdm_query_boxes(sdm_map *m, const float *boxes, int64_t n, sdm_box_result *out, uint32_t flags);

/* ---- Euclidean distance field (ESDF) of the map block, and distance queries on it ----
 * sdm_esdf_update enqueues, on the map's stream, an exact Euclidean distance transform of the result array of the last
 * frame enqueued before the call, and returns without waiting.  The field is a snapshot: it answers for that frame -
 * its map center and ring offsets are kept with it - until the next sdm_esdf_update, whatever frames, sdm_clear,
 * sdm_load_state or sdm_set_ring_state come in between.
 * Obstacles: cells with occ >= 1 (occupied or guessed occupied, as segments block); with SDM_ESDF_UNKNOWN_IS_OBSTACLE
 * also occ == -1; with SDM_ESDF_STATIC_ONLY no cell whose winning track is movable (1 <= track <= max_movable_track;
 * track 0 is static).  The map is a block, not a torus: the ring's wrap point is not a neighbour relation, and the
 * space outside the map is never an obstacle, under any flag (unlike SDM_QUERY_UNKNOWN_BLOCKS for segments).
 * Metric: between cell centres in map-index cells (cell (i, j, k) as above).  Per cell the field holds site, the
 * map-index cell i | j << x_n | k << (x_n + y_n) of a nearest obstacle (any one where several are equally near), and
 * d2 = |cell - site|^2, its exact squared distance in cells.  A field without any obstacle holds 0xffffffff in both.
 * Memory: 8 bytes per voxel of device memory (4 B site, 4 B snapshot of each cell's result word track / label / occ),
 * allocated at the first sdm_esdf_update and freed by sdm_destroy: 134 MB at 256^3, 1.07 GB at 512^3.  The build uses no
 * scratch of the frames'.
 * Errors: SDM_ERR_INVALID_ARGUMENT for unknown flag bits, a Z-slab shard (shard_count > 1), and sdm_get_esdf or
 * sdm_query_distance before any sdm_esdf_update. */
#define SDM_ESDF_UNKNOWN_IS_OBSTACLE 0x1u
#define SDM_ESDF_STATIC_ONLY 0x2u
sdm_status sdm_esdf_update(sdm_map *m, uint32_t flags);
/* Host copies of the field in map-index order (x fastest, then y, then z), NX*NY*NZ entries each; any of the three may
 * be NULL; waits.  origin = the global position of the min corner of cell (0,0,0) of the snapshot, center + pmin in
 * float32. */
sdm_status sdm_get_esdf(sdm_map *m, uint32_t *d2, uint32_t *site, float origin[3]);
/* Distance of points xyz[3i..3i+2] (global frame) from the field's obstacles.  A point's cell is floor(u) per axis (as
 * for segments and boxes), u taken with the snapshot's map center.  The distance is the trilinear interpolation of
 * D(c) = sqrtf((float)d2(c)) * voxel_size between cell centres: per axis s = u - 0.5, i0 = floor(s), t = s - i0, corners
 * clamp(i0, 0, N-1) and clamp(i0 + 1, 0, N-1) - so it is constant beyond the outermost cell centres, with gradient 0
 * along that axis.  No answer (a point outside the map, a non-finite coordinate, a field without obstacles): d2
 * 0xffffffff, distance -1, gradient 0, nearest NaN, track / label / occ 0 / 0 / -1.  Flags: SDM_QUERY_ON_DEVICE, as for
 * the queries above; n == 0 launches nothing. */
typedef struct {      /* 36 bytes */
  float distance;     /* metres: the interpolated D; -1 = no answer */
  float gradient[3];  /* d distance / d position of that interpolant, per metre; 0 where no answer */
  float nearest[3];   /* centre of the nearest obstacle of the point's cell, global frame:
                         (center + pmin) + ((float)site + 0.5f) * voxel_size; NaN where no answer */
  uint32_t d2;        /* of the point's cell; 0xffffffff = no answer */
  uint16_t track;     /* snapshot result of that nearest obstacle cell */
  uint8_t label;
  int8_t occ;         /* 1 or 2, or -1 when unknown cells count as obstacles */
} sdm_distance_result;
sdm_status sdm_query_distance(sdm_map *m, const float *xyz, int64_t n, sdm_distance_result *out, uint32_t flags);

/* ---- instance table: the map by object - per winning track id its cells, box and moments ----
 * sdm_instances_update enqueues, on the map's stream, one pass over the result array of the last frame enqueued before
 * the call and returns without waiting.  Like the distance field the table is a snapshot: it keeps that frame's map
 * center and answers for it until the next sdm_instances_update, whatever frames, sdm_clear, sdm_load_state or
 * sdm_set_ring_state come in between.  Nothing of the map's state is modified and no scratch of the frames' is used.
 * Counted cells: occ >= 1 (occupied or guessed occupied, as segments block and as the field's obstacles); with
 * SDM_INSTANCES_MOVABLE_ONLY only cells whose winning track is movable (1 <= track <= max_movable_track), with
 * SDM_INSTANCES_OBSERVED_ONLY only occ == 1.  An instance is the set of counted cells with one winning track id; track 0
 * is an instance like any other unless SDM_INSTANCES_MOVABLE_ONLY is set.  Tracks without a counted cell have no entry.
 * Cells are map-index cells (cell (i, j, k) of the query block above), not storage indices: the ring's wrap point never
 * splits a box.  Every accumulated field is an integer sum, minimum or maximum (wsum_max: a float maximum), so the
 * table is bitwise the same from run to run.  The float triples follow from the integer fields by the formulas below,
 * one IEEE operation at a time: box_* in float32, centroid in double and rounded once; origin = center + pmin in
 * float32, what sdm_get_esdf returns.
 * Memory: 17.6 MB of device memory (8.1 MB of accumulators for the 65536 track ids and the 256 label counters, 9.4 MB
 * for the table itself), allocated by the first sdm_instances_update and freed by sdm_destroy.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, unknown flag bits, cap < 0, a NULL n_out (or a NULL out with
 * cap > 0), a Z-slab shard (shard_count > 1), and either getter before any sdm_instances_update. */
#define SDM_INSTANCES_MOVABLE_ONLY  0x1u  /* count only cells with 1 <= track <= max_movable_track */
#define SDM_INSTANCES_OBSERVED_ONLY 0x2u  /* count only occ == 1 (leave out guessed-occupied cells, occ == 2) */
typedef struct {            /* 144 bytes, every field naturally aligned */
  uint16_t track;           /* the instance: the winning track id of its cells */
  uint8_t  label;           /* label of first_cell */
  uint8_t  mixed_labels;    /* 1 if the counted cells do not all carry the same label */
  uint32_t n_cells;         /* counted cells of this track (> 0: absent tracks have no entry) */
  uint32_t n_guessed;       /* of them, cells with occ == 2 */
  uint32_t first_cell;      /* smallest map-index cell word i | j << x_n | k << (x_n + y_n) among them */
  uint16_t cell_min[3];     /* axis-aligned box in map-index cells, inclusive, x y z */
  uint16_t cell_max[3];
  float    wsum_max;        /* largest sdm_voxel_result.wsum among them (float comparison) */
  uint64_t cell_sum[3];     /* sum of i, of j, of k */
  uint64_t cell_sq[6];      /* sum of ii, jj, kk, ij, ik, jk */
  float    box_min[3];      /* global frame, metres: origin + (float)cell_min * voxel_size */
  float    box_max[3];      /* origin + (float)(cell_max + 1) * voxel_size */
  float    centroid[3];     /* (float)((double)origin + ((double)cell_sum / (double)n_cells + 0.5) * (double)voxel_size) */
  uint32_t pad;             /* 0 */
} sdm_instance;
sdm_status sdm_instances_update(sdm_map *m, uint32_t flags);
/* Waits; writes at most `cap` entries in ascending track id and sets *n_out to how many there are (it may exceed cap,
 * as with sdm_tracks_with_particles; nothing beyond min(cap, *n_out) entries is written).  out may be NULL with cap 0;
 * origin (the global position of the min corner of cell (0,0,0) of the snapshot) may be NULL. */
sdm_status sdm_get_instances(sdm_map *m, sdm_instance *out, int32_t cap, int32_t *n_out, float origin[3]);
/* Counted cells per label id, under the flags of the last sdm_instances_update (how much "Road", how much "Car").  Waits. */
sdm_status sdm_get_label_cells(sdm_map *m, uint32_t out[256]);

/* ---- frontiers: where known free space borders never-observed space, in connected clusters ----
 * sdm_frontiers_update enqueues, on the map's stream, a build from the result array of the last frame enqueued before
 * the call and returns without waiting.  Like the distance field and the instance table the result is a snapshot: it
 * keeps that frame's map center and ring offsets and answers for it until the next sdm_frontiers_update, whatever
 * frames, sdm_clear, sdm_load_state or sdm_set_ring_state come in between.  Nothing of the map's state is modified and no
 * scratch of the frames', the field's or the table's is used.
 * Frontier cell: a map-index cell (cell (i, j, k) of the query block above) with occ == 0 of whose six face neighbours
 * at least one lies inside the map and has occ == -1.  The space outside the map is never unknown here (as it is never
 * an obstacle for the distance field), neighbours are taken in map-index space - the ring's wrap point is not a
 * neighbour relation, the map is not a torus - and unknown_faces of a cell is how many of the six are unknown (1..6).
 * Cluster: a connected component of frontier cells under 26-connectivity (face, edge or corner), under 6-connectivity
 * with SDM_FRONTIERS_FACE_CONNECTED.  Its identity is first_cell, the smallest map-index cell word
 * i | j << x_n | k << (x_n + y_n) among its cells; the table ascends in first_cell.  min_cells <= 1 keeps every cluster;
 * a larger value leaves the clusters with fewer cells out of the table - their cells stay in the cell list, with
 * cluster == 0xffffffff.
 * Everything accumulated is an integer sum, minimum or maximum, and a cluster's label is its smallest cell: tables and
 * lists are bitwise the same from run to run.  The float triples follow from the integer fields by sdm_instance's
 * formulas, one IEEE operation at a time: box_* in float32, centroid in double and rounded once, origin = center + pmin
 * in float32.
 * max_cells is the capacity of the cell list, 0 = V / 16 cells (V = NX*NY*NZ; at most V).  Memory: V * 7 / 16 bytes for
 * the bitmasks and their prefix, and SDM_FRONTIERS_BYTES_PER_CELL = 169 bytes of device memory per cell of capacity
 * (56 B accumulator, 96 B table entry - every cell may be a cluster of its own -, 16 B cell / cluster / root / rank words,
 * 1 B unknown_faces): 7.3 MB + 177 MB at 256^3 with the default capacity.  Allocated at the first sdm_frontiers_update,
 * grown by one that asks for more cells, freed by sdm_destroy.  A frame with more frontier cells than the capacity:
 * both getters return SDM_ERR_CAPACITY and sdm_get_frontier_cells still sets *n_out to the true count; nothing is
 * written out of bounds and nothing is truncated; an update with max_cells >= that count then succeeds.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, unknown flag bits, cap < 0 or max_cells < 0, a NULL n_out (or a NULL
 * out with cap > 0), a Z-slab shard (shard_count > 1), and either getter before any sdm_frontiers_update. */
#define SDM_FRONTIERS_FACE_CONNECTED 0x1u  /* clusters under 6-connectivity instead of 26-connectivity */
#define SDM_FRONTIERS_BYTES_PER_CELL 169
typedef struct {              /* 96 bytes, every field naturally aligned */
  uint32_t first_cell;        /* the cluster: the smallest map-index cell word among its cells */
  uint32_t n_cells;
  uint32_t n_unknown_faces;   /* sum of unknown_faces over its cells */
  uint32_t first_index;       /* position of first_cell in the cell list (the cluster's first entry there) */
  uint16_t cell_min[3];       /* axis-aligned box in map-index cells, inclusive, x y z */
  uint16_t cell_max[3];
  uint32_t pad0;              /* 0 */
  uint64_t cell_sum[3];       /* sum of i, of j, of k */
  float    box_min[3];        /* global frame, metres: origin + (float)cell_min * voxel_size */
  float    box_max[3];        /* origin + (float)(cell_max + 1) * voxel_size */
  float    centroid[3];       /* (float)((double)origin + ((double)cell_sum / (double)n_cells + 0.5) * (double)voxel_size) */
  uint32_t pad1;              /* 0 */
} sdm_frontier_cluster;
sdm_status sdm_frontiers_update(sdm_map *m, uint32_t flags, int32_t min_cells, int64_t max_cells);
/* Waits; writes at most `cap` entries in ascending first_cell and sets *n_out to how many there are (it may exceed cap,
 * as with sdm_get_instances; nothing beyond min(cap, *n_out) entries is written).  out may be NULL with cap 0; origin
 * (the global position of the min corner of cell (0,0,0) of the snapshot) may be NULL. */
sdm_status sdm_get_frontier_clusters(sdm_map *m, sdm_frontier_cluster *out, int32_t cap, int32_t *n_out, float origin[3]);
/* Waits; the frontier cells in ascending map-index cell word, at most `cap` of them: per cell its word, the index of its
 * cluster in the table (0xffffffff: a cluster below min_cells) and unknown_faces.  Any of the three arrays may be NULL.
 * *n_out = how many cells there are (it may exceed cap). */
sdm_status sdm_get_frontier_cells(sdm_map *m, uint32_t *cell, uint32_t *cluster, uint8_t *unknown_faces,
                                  int64_t cap, int64_t *n_out);

/* ---- view scoring: how much unknown space would a camera at this pose see? (next-best-view exploration) ----
 * A view is a camera pose and a range.  Its rays are a table the caller passes once per call: `dirs` holds n_rays
 * camera-frame vectors, three floats each, NOT normalised - (x/z, y/z, 1) gives a ray whose end lies at planar depth
 * `range`, as depth_max is meant.  Ray r of view v is the segment from a = pos to b = pos + range * (R(q) d_r), computed
 * in float32 one IEEE operation at a time (no contraction), in this order: with q = (w, x, y, z), used as given,
 *   R = | 1 - 2 (y y + z z)   2 (x y - w z)       2 (x z + w y)     |
 *       | 2 (x y + w z)       1 - 2 (x x + z z)   2 (y z - w x)     |
 *       | 2 (x z - w y)       2 (y z + w x)       1 - 2 (x x + y y) |
 * (R d)_i = (R_i0 d_0 + R_i1 d_1) + R_i2 d_2, then b_i = pos_i + range * (R d)_i.  range <= 0 is not an error: b = a, the
 * zero-length segment, the cell of a.  The segment is walked exactly as sdm_query_segments walks it without
 * SDM_QUERY_UNKNOWN_BLOCKS: clipped to the map, only cells with occ >= 1 block, unknown cells are passed through and
 * counted, space outside the map is nothing, x steps before y before z at equal t.  rays_out[v * n_rays + r] is bit for
 * bit what sdm_query_segments returns for (a, b); ray_unknown_out[v * n_rays + r] is the number of cells with occ == -1
 * among that ray's `cells`.  Either may be NULL.  A non-finite pos, q or range gives an all-zero gain and "no hit" rays
 * with cells = 0; a non-finite d_r does for that ray only.
 * Distinct counts: a cell counts once per view, however many of its rays visit it - the rays of a camera share their
 * cells near the origin, and a sum over rays would count a nearby cell hundreds of times.  The blocking cell of a ray
 * counts towards n_occupied, every cell before it towards n_unknown or n_free by its occ.  All counters and sums are
 * integers: the result is bitwise the same from run to run whatever order the rays finish in.
 * Like the other queries: reads the results of the last frame enqueued before the call, in stream order on the map's
 * stream; never modifies map state; uses no scratch of the frames', the field's, the table's or the frontiers'.  With
 * SDM_QUERY_ON_DEVICE all five pointers are device pointers and the call returns without waiting; without it inputs and
 * outputs are host memory, staged in chunks of whole views, and the call waits.  n_views == 0 launches nothing.
 * Memory: one bitmask of V / 8 bytes (V = NX*NY*NZ) per view in flight, in a pool of min(256, max(1, 64 MiB / (V / 8)))
 * masks - 64 MiB at 256^3 (32 views in flight) and at 512^3 (4), 256 * V / 8 bytes on maps of up to 2^21 cells -
 * allocated at the first sdm_query_views, freed by sdm_destroy and all zero whenever a call's work has completed.  A call
 * with more views than masks works through them in batches.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, views, dirs or out, n_views < 0, n_rays < 1 or > SDM_VIEW_MAX_RAYS,
 * n_views * n_rays >= 2^31, unknown flag bits (only SDM_QUERY_ON_DEVICE is known), or a Z-slab shard (shard_count > 1). */
#define SDM_VIEW_MAX_RAYS 65536
typedef struct {   /* 32 bytes */
  float pos[3];    /* camera position, global frame */
  float q[4];      /* camera orientation (w, x, y, z), as sdm_update's cam_q; used as given, not normalised */
  float range;     /* metres; scales the ray table */
} sdm_view;
typedef struct {          /* 40 bytes, every field naturally aligned */
  uint32_t n_unknown;     /* DISTINCT in-map cells with occ == -1 that at least one ray of the view visits */
  uint32_t n_free;        /* distinct visited cells with occ == 0 */
  uint32_t n_occupied;    /* distinct cells with occ >= 1 in which at least one ray ends */
  uint32_t rays_hit;      /* rays that end in a blocking cell */
  uint32_t rays_in_map;   /* rays that visit at least one in-map cell */
  uint32_t pad;           /* 0 */
  uint64_t ray_cells;     /* sum over the rays of cells visited (= sum of sdm_segment_hit.cells) */
  uint64_t ray_unknown;   /* sum over the rays of visited cells with occ == -1 (not distinct) */
} sdm_view_gain;
sdm_status sdm_query_views(sdm_map *m, const sdm_view *views, int64_t n_views, const float *dirs, int32_t n_rays,
                           sdm_view_gain *out, sdm_segment_hit *rays_out, int32_t *ray_unknown_out, uint32_t flags);

/* ---- travel cost: how far is it from the robot to a cell, and by which cells? (the denominator of a view's utility) ----
 * sdm_reach_update builds, on the map's stream, a shortest-path field over the traversable cells of the map block from a
 * set of start cells.  Unlike the other builds IT WAITS: it returns when the field is complete - how much work there is
 * depends on the map's topology, the host decides when the relaxation is done, and no kernel ever waits for another
 * workgroup.  Like them the result is a snapshot that keeps its frame's map center and ring offsets and answers for it
 * until the next sdm_reach_update; nothing of the map's state is modified and no scratch of the frames', the distance
 * field's, the instance table's, the frontiers' or view scoring's is used.
 * Cells are map-index cells (i, j, k), cell word i | j << x_n | k << (x_n + y_n), as for the field, the table and the
 * frontiers.  The ring's wrap point is not a neighbour relation, the map is a block and no torus, and nothing outside
 * the map is traversable.
 * Traversable cell: occ == 0; with SDM_REACH_THROUGH_UNKNOWN also occ == -1; occ >= 1 never.
 * Clearance: min_d2 is a squared clearance in cells.  min_d2 == 0: the classes come from the result array of the last
 * frame enqueued before the call.  min_d2 > 0: the build reads the distance field's snapshot instead - the snapshot
 * word for the class, the site for d2 - and a cell must also have d2 >= min_d2 (a field without obstacles has
 * d2 = 0xffffffff, which passes); the reach field then inherits that field's frame, not the current one; without an
 * sdm_esdf_update before it the call is SDM_ERR_INVALID_ARGUMENT.  The field's own flags (UNKNOWN_IS_OBSTACLE,
 * STATIC_ONLY) are the caller's choice and change nothing in this rule.
 * Moves: the offsets o = (dx, dy, dz) in {-1, 0, 1}^3 without 0, numbered n = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); 13 is
 * the centre and unused.  With SDM_REACH_FACE_CONNECTED only the six face moves exist.  A move c -> c + o is allowed
 * when every cell c + s with s_a in {0, o_a} per axis - 2, 4 or 8 cells - lies inside the map and is traversable: no
 * diagonal squeezes between two blocked cells, and the rule is symmetric.  A move weighs 10, 14 or 17 for one, two or
 * three non-zero components (SDM_REACH_COST_PER_CELL = 10).
 * Field: cost(c), uint32, is the smallest weight sum over the paths of allowed moves from any start cell to c; a start
 * cell has cost 0; 0xffffffff = unreachable or not traversable.  With max_cost > 0 the cells whose true cost exceeds
 * max_cost read 0xffffffff (a truncated search, still exact); max_cost == 0: no limit.  The largest possible cost is
 * below 17 * V (< 2^32 at 512^3).  The field is the unique fixed point of a min-plus relaxation over integers: it is
 * bitwise the same whatever order the device relaxes in.
 * Starts: n_starts host entries, as points (start_xyz, three floats each, the cell of floor(u) per axis as for the
 * distance query) or as cell words (start_cells); exactly one of the two pointers is non-NULL, also with n_starts == 0.
 * Entries outside the map, non-finite ones and ones on cells that are not traversable are
 * ignored; duplicates are fine; no usable start is no error: every cell is unreachable.
 * Path descent: from a cell with 0 < cost < 0xffffffff the next cell is c + o for the smallest move number n whose move
 * is allowed and has cost(c + o) + w(o) == cost(c) (one exists by construction; the allowed test is needed: a neighbour
 * can satisfy the equation across a forbidden diagonal).  A path is the cell words from the goal to a start, both
 * included; its length is at most cost / 10 + 1.
 * sdm_query_reach / sdm_reach_paths answer for the field of the last build; goals are points (xyz) or cell words (cells),
 * exactly one of the two non-NULL; SDM_QUERY_ON_DEVICE as for the other queries (device pointers, enqueued, no wait),
 * host mode through the queries' staging area.  len_out[g] is the true length of goal g's path, 0 where there is none;
 * it may exceed max_len: only the first min(len, max_len) cells, counted from the goal, are written to row g of
 * cells_out (n rows of max_len words), the rest of the row is left untouched.
 * Memory: 4 B per voxel of cost, V / 8 bytes of traversable mask, and the activity bookkeeping of the relaxation - one
 * bit and one list word per tile of up to 8 x 8 x 8 cells (V / 512 tiles on maps without 4-cell axes): 64 MiB + 2 MiB +
 * 132 KiB at 256^3.  Allocated at the first sdm_reach_update, freed by sdm_destroy.
 * The build issues its rounds eight at a time between two looks at the count of active tiles; the environment variable
 * SDM_REACH_BATCH=k (k >= 1, read at every build) makes it k, for tools/probes/reach_probe.py.  The field does not depend on it.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, no or both start / goal pointers, unknown flag bits, negative counts,
 * max_len < 0, a NULL output, a Z-slab shard (shard_count > 1), min_d2 > 0 without a distance field, and the getter or a
 * query before any sdm_reach_update.  SDM_ERR_NOT_CONVERGED if the relaxation has not come to rest after V rounds: a
 * defect, never a result. */
#define SDM_REACH_FACE_CONNECTED  0x1u  /* the six face moves only */
#define SDM_REACH_THROUGH_UNKNOWN 0x2u  /* cells with occ == -1 are traversable too */
#define SDM_REACH_COST_PER_CELL   10
typedef struct {            /* 32 bytes */
  uint32_t n_starts_used;   /* distinct start cells that were traversable */
  uint32_t n_traversable, n_reached, max_cost_reached;
  uint32_t rounds;          /* relaxation rounds the build took (diagnostic; not part of the bitwise contract) */
  uint32_t flags, min_d2, max_cost;
} sdm_reach_info;
typedef struct {            /* 16 bytes */
  uint32_t cost;            /* 0xffffffff: no path */
  float    metres;          /* (float)cost * (voxel_size * 0.1f), float32, no contraction; -1 where cost is 0xffffffff */
  uint32_t cell;            /* the goal's cell word; 0xffffffff outside the map / non-finite */
  uint8_t  next;            /* move number of the first descent step; 13 at a start; 255 where no path */
  uint8_t  status;          /* 0 reached, 1 traversable but unreachable (or beyond max_cost), 2 not traversable, 3 outside / non-finite */
  uint16_t pad;             /* 0 */
} sdm_reach_result;
sdm_status sdm_reach_update(sdm_map *m, const float *start_xyz, const uint32_t *start_cells, int64_t n_starts,
                            uint32_t min_d2, uint32_t max_cost, uint32_t flags);
/* Waits; cost in map-index order, x fastest (V words); either of cost and info may be NULL, and so may origin (the global
 * position of the min corner of cell (0,0,0) of the snapshot). */
sdm_status sdm_get_reach(sdm_map *m, uint32_t *cost, sdm_reach_info *info, float origin[3]);
sdm_status sdm_query_reach(sdm_map *m, const float *xyz, const uint32_t *cells, int64_t n, sdm_reach_result *out, uint32_t flags);
sdm_status sdm_reach_paths(sdm_map *m, const float *xyz, const uint32_t *cells, int64_t n, int32_t max_len,
                           uint32_t *cells_out, int32_t *len_out, uint32_t flags);

/* ---- forecast: where will the moving objects be while the robot drives the path it planned? ----
 * sdm_forecast_update enqueues, on the map's stream, the future occupancy of the moving objects of the last frame enqueued
 * before the call, and returns without waiting.  Like the other layers the result is a snapshot: it keeps that frame's
 * map center and ring offsets and answers for it until the next sdm_forecast_update, whatever frames, sdm_clear or
 * sdm_load_state come in between; nothing of the map's state is modified and no scratch of the frames' or of another
 * layer is used.  Cells are map-index cells, cell word i | j << x_n | k << (x_n + y_n).  The map is a block, no torus:
 * what moves out of the block is dropped and counted.  Only integer OR / MIN / ADD atomics build the field: it is
 * bitwise the same from run to run.
 * Motions: per moving track one velocity in metres per second in the global frame, translation only (what the object
 * layer estimates: sdm_object_info.translation_velocity).  n_motions == 0 is allowed: the field then holds only the
 * classes.  Horizons: n_horizons times t[0] < t[1] < ... in seconds, all finite and > 0, 1 <= n_horizons <=
 * SDM_FORECAST_MAX_HORIZONS.  The caller chooses horizons that cover the times it will ask about: a time past the last
 * horizon is answered with the last one.
 * Shift: all cells of a track move by one integer cell vector per horizon,
 *   s[k][a] = clamp(nearbyint(((double)v[a] * (double)t[k]) / (double)voxel_size), -1024, 1024)
 * - two IEEE double operations, ties to even, voxel_size the float32 of the configuration.  Cell centres all shift by the
 * same vector, so this is the translation rounded to cells: it leaves no holes.
 * Stamps: motions x horizons are expanded into a list of (track, horizon k, dx, dy, dz), ascending track, then horizon,
 * then j.  Without flags one stamp s[k] per track and horizon.  With SDM_FORECAST_SWEPT horizon k covers the whole interval
 * (t[k-1], t[k]]: with p = s[k-1] (s[-1] = 0), q = s[k], D = q - p, J = max_a |D_a| the stamps are
 *   p_a + sgn(D_a) * ((2 * j * |D_a| + J) / (2 * J))   (integer division),  j = 1 .. J;   J == 0: the single stamp q.
 * More than SDM_FORECAST_MAX_STAMPS stamps in one build: SDM_ERR_CAPACITY, decided on the host before anything is enqueued
 * (a limit on the input, not a capacity to guess).  sdm_forecast_stamps is that expansion on its own: host code, no map,
 * no device; *n_out is the true number of stamps and may exceed cap (nothing is written beyond cap); it checks what the
 * build checks except the track's upper bound, and answers SDM_ERR_CAPACITY above SDM_FORECAST_MAX_STAMPS.
 * Field, per map-index cell (x fastest), two uint32:
 *   mask   bits 0..15: bit k is set when some source cell plus a horizon-k stamp of its track lands here;
 *          bits 16..17: the class now - 0 unknown (occ == -1), 1 free (occ == 0), 2 an obstacle that stays (occ >= 1, winning
 *          track not among the motions), 3 source (occ >= 1, winning track among the motions; guessed-occupied cells, occ == 2,
 *          count like occ == 1, as for segments and the distance field); all other bits 0.
 *   first  the minimum over all landings of k << 16 | track: the earliest horizon at which anything arrives and, among
 *          equals, the smallest track id; 0xffffffff where nothing lands.
 * State of a cell at horizon k, in this priority: 1 stays (class 2); 2 predicted (bit k set); 3 vacated (class 3, bit k
 * clear); 0 free (class 1); -1 unknown.  Horizon of a time T: the smallest k with T <= t[k]; the last one beyond.
 * The build does not wait for the device: its table goes up from one of two page-locked copies that builds use in turn, so
 * a build waits at most until the upload of the build before the last one has left its copy (stream order: whatever was
 * enqueued before that upload).
 * Memory: 8 bytes per voxel of device memory (4 B mask, 4 B first), and less than 1 MB for the motion table and the
 * stamps (twice that page-locked), allocated at the first sdm_forecast_update and freed by sdm_destroy: 134 MB at 256^3, 1.07 GB at 512^3;
 * sdm_get_forecast_cells adds V / 16 bytes at its first call.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, a Z-slab shard (shard_count > 1), unknown flag bits, n_motions < 0 (or
 * motions NULL with n_motions > 0), a duplicate track, track 0 or a track above max_movable_track, a non-finite velocity,
 * pad != 0, n_horizons out of range, horizons not finite, not > 0 or not strictly ascending, and a getter or query
 * before any sdm_forecast_update. */
#define SDM_FORECAST_SWEPT 0x1u          /* sdm_forecast_update: horizon k covers (t[k-1], t[k]], not the instant t[k] */
#define SDM_FORECAST_VACATED_BLOCKS 0x4u /* sdm_query_forecast_segments: source cells block although their object leaves */
#define SDM_FORECAST_MAX_HORIZONS 16
#define SDM_FORECAST_MAX_STAMPS 65536
typedef struct {   /* 16 bytes */
  uint16_t track;  /* 1 .. max_movable_track */
  uint16_t pad;    /* 0 */
  float v[3];      /* metres per second, global frame */
} sdm_motion;
typedef struct {   /* 12 bytes */
  uint16_t track;
  uint8_t horizon;
  uint8_t pad;     /* 0 */
  int16_t d[3];    /* cells */
  int16_t pad2;    /* 0 */
} sdm_forecast_stamp;
typedef struct {   /* 40 bytes */
  uint32_t n_motions, n_horizons, n_stamps, flags;
  uint32_t n_sources;   /* cells of class 3 */
  uint32_t n_marked;    /* cells with any horizon bit */
  uint64_t n_marks_in;  /* (source cell, stamp) pairs that land inside the block */
  uint64_t n_marks_out; /* ... and outside: dropped */
} sdm_forecast_info;
typedef struct {         /* 8 bytes */
  int8_t state;          /* at `horizon`: -1 unknown, 0 free, 1 stays, 2 predicted, 3 vacated */
  uint8_t horizon;       /* of the query's time; 0xff outside the map / non-finite */
  uint16_t track;        /* of `first`; 0 where nothing lands */
  uint16_t mask;         /* the cell's horizon bits */
  uint8_t first_horizon; /* of `first`; 0xff where nothing lands */
  uint8_t pad;           /* 0 */
} sdm_forecast_result;
typedef struct {    /* 16 bytes */
  float t;          /* where the segment enters its first blocking cell, as a fraction of a->b; -1 = nothing blocks */
  uint32_t cell;    /* map-index word of that cell; 0xffffffff = none / outside the map */
  int32_t cells;    /* in-map cells visited up to and including the hit (all of them if no hit) */
  uint16_t track;   /* state 2: of the cell's `first`; else 0 */
  int8_t state;     /* of the blocking cell: 1 stays, 2 predicted, 3 vacated, -1 unknown / outside; 0 = nothing blocks */
  uint8_t horizon;  /* state 2: the lowest horizon bit set within the cell's time range; else 0xff */
} sdm_forecast_hit;
sdm_status sdm_forecast_stamps(float voxel_size, const sdm_motion *motions, int32_t n_motions, const float *horizons,
                               int32_t n_horizons, uint32_t flags, sdm_forecast_stamp *out, int64_t cap, int64_t *n_out);
sdm_status sdm_forecast_update(sdm_map *m, const sdm_motion *motions, int32_t n_motions, const float *horizons,
                               int32_t n_horizons, uint32_t flags);
/* Waits; mask and first in map-index order, x fastest (V words each); any of the four pointers may be NULL (origin: the
 * global position of the min corner of cell (0,0,0) of the snapshot). */
sdm_status sdm_get_forecast(sdm_map *m, uint32_t *mask, uint32_t *first, sdm_forecast_info *info, float origin[3]);
/* Waits; the cells with any horizon bit in ascending cell word, with their two field words, for visualisation.  *n_out is
 * their number (info.n_marked) and may exceed cap; nothing is written beyond cap; any of the three arrays may be NULL. */
sdm_status sdm_get_forecast_cells(sdm_map *m, uint32_t *cell, uint32_t *mask, uint32_t *first, int64_t cap, int64_t *n_out);
/* Points in space and time, xyzt[4i..4i+3] = x y z T (global frame, seconds from the snapshot): the cell is floor(u) per
 * axis with the snapshot's frame, the state that of the table above at the horizon of T.  A point outside the map or a
 * non-finite value: state -1, horizon 0xff, track 0, mask 0, first_horizon 0xff.  Flags: SDM_QUERY_ON_DEVICE, as for the
 * other queries; n == 0 launches nothing.  Device mode: xyzt must be aligned to 16 bytes and out to 8 (the kernel moves
 * whole items; what sdm_device_alloc returns is, an array that begins at an odd item offset inside it may not be). */
sdm_status sdm_query_forecast(sdm_map *m, const float *xyzt, int64_t n, sdm_forecast_result *out, uint32_t flags);
/* Space-time segments seg[8i..8i+7] = ax ay az ta bx by bz tb, ta <= tb: the first blocking cell on the way.  The walk is
 * sdm_query_segments' (same cells, same order, same t, clipped to the map).  A cell entered at tau_in and left at tau_out
 * (the next cell's tau_in, 1 for the last cell) is occupied during T(tau_in) .. T(tau_out), T(tau) = (double)ta + tau *
 * ((double)tb - (double)ta).  It blocks when its class is 2 (state 1); when any horizon bit between the horizons of
 * those two times, inclusive, is set (state 2); with SDM_QUERY_UNKNOWN_BLOCKS when its class is 0 and none of those bits is
 * set, or it lies outside the map (state -1); with SDM_FORECAST_VACATED_BLOCKS when its class is 3 (state 3, if none of
 * those bits is set).  ta > tb or any non-finite value is handled like a non-finite coordinate in sdm_query_segments: no
 * hit and cells = 0, or with SDM_QUERY_UNKNOWN_BLOCKS a hit at t = 0 on cell 0xffffffff.  With no motions and no flags
 * t, cells and the hit cell are sdm_query_segments'.  Flags: SDM_QUERY_ON_DEVICE, SDM_QUERY_UNKNOWN_BLOCKS,
 * SDM_FORECAST_VACATED_BLOCKS.  Device mode: out must be aligned to 16 bytes (an item is stored whole), seg to 4. */
sdm_status sdm_query_forecast_segments(sdm_map *m, const float *seg, int64_t n, sdm_forecast_hit *out, uint32_t flags);

/* ---- ground layer: where is the surface I stand on, which columns can I not enter, does my body fit here? ----
 * sdm_ground_update enqueues, on the map's stream, a 2-D view of the last frame enqueued before the call - a height map, a
 * costmap and its distance transform - and returns without waiting.  Like the other layers the result is a snapshot: it
 * keeps that frame's map center and ring offsets and answers for it until the next sdm_ground_update, whatever frames,
 * sdm_clear, sdm_load_state or sdm_set_ring_state come in between; nothing of the map's state is modified and no scratch
 * of the frames' or of another layer is used.  Everything is integer and bitwise reproducible; all options are in cells.
 * Up axis: up_axis a in {0, 1, 2}, up_sign +1 or -1 (a camera-style frame with the ground at +y is (1, -1); z-up poses are
 * (2, +1)).  The height of map-index cell idx_a is h = idx_a for sign +1 and N_a - 1 - idx_a for sign -1.
 * Columns: the other two axes in ascending order are u and v; the grid is N_u x N_v, column word col = i_u + j_v * N_u.
 * A column is the N_a cells over one grid cell.  The ring's wrap point is no neighbour relation; the grid is a block.
 * Cell classes, from the second word of the result (track, label, occ):
 *   solid     occ >= 1 (guessed-occupied counts); with SDM_GROUND_IGNORE_MOVABLE an occ >= 1 cell whose track is movable
 *             (1 <= track <= max_movable_track) is not solid and is passable instead.
 *   passable  occ == 0; with SDM_GROUND_UNKNOWN_PASSABLE also occ == -1.  A height outside the map (h >= N_a) is passable.
 *   support at h: the cell is solid, its track is not movable, bit `label` of support_labels is set (bit l of word l / 32),
 *             and the cells h + 1 .. h + clearance of the column are all passable.  Those are read as they are, also
 *             above h_hi: the band limits where supports are looked for, not the headroom test.
 * Per column (sdm_ground_cell): level = the highest support h in [h_lo, h_hi], 0xffff if none; top = the highest solid h
 * in the band, 0xffff if none; label = the level cell's label, 0 if none; headroom = the consecutive passable cells
 * directly above level up to the map's top, saturating at 255, 0 if no level; n_unknown = the occ == -1 cells in the band,
 * saturating at 255.
 * Class byte cls = class | step << 2 | lethal << 3.  class: 1 ground (a level), 2 obstacle (no level, a top), 0 none.
 * step: the column P has a level and some 4-neighbour Q inside the grid has one with level(P) > level(Q) + max_step - only
 * the higher side is marked: one can drive up to a kerb.  lethal: class 2, or step, or with SDM_GROUND_NONE_IS_LETHAL class 0.
 * Distance: d2[col], uint32, the exact squared Euclidean distance in columns to the nearest lethal column; 0 on one,
 * 0xffffffff everywhere when there is none.
 * sdm_query_ground: the point's cell is floor(u) per axis, as for the distance query.  Outside the map or non-finite:
 * col 0xffffffff, d2 0xffffffff, surface 0, above INT32_MIN, cell {0xffff, 0xffff, 0, 0, 0, 0}, dist -1, status 3.
 * sdm_query_footprints: a footprint is a rectangle on the grid's plane: its centre in global metres along u and v, its
 * heading as a unit vector (dir_u, dir_v) the caller supplies - neither side takes a sine -, half its length along the
 * heading and half its width.  Column (i, j) is covered when, in float32 without contraction,
 *   pu = origin[u] + ((float)i + 0.5f) * voxel_size, pv likewise; du = pu - center_u, dv = pv - center_v;
 *   |du * dir_u + dv * dir_v| <= half_len  and  |dv * dir_u - du * dir_v| <= half_wid.
 * The answer is as if every column of the grid were tested; nothing outside the grid is counted.  A non-finite field, or
 * half_len + half_wid > 64 * voxel_size (float32), gives the answer of a footprint that covers nothing: the counts 0,
 * level_min = level_max = 0xffff, min_d2 = first_lethal = 0xffffffff.
 * Both queries answer for the last build and take SDM_QUERY_ON_DEVICE as the other queries do (device pointers, enqueued,
 * no wait; items are 4-byte aligned); host mode goes through the queries' staging area.
 * Memory: 14 B per column (8 B cell, 4 B d2, 2 B of the distance transform's row pass) for the largest of the three
 * grids, 917 KB at 256^2, and 32 B of counters per row of the grid; allocated at the first sdm_ground_update, freed by
 * sdm_destroy.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map or NULL options, unknown flag bits, up_axis not in 0..2, up_sign not
 * +1 / -1, a band that is not 0 <= h_lo <= h_hi < N_a, clearance > 255, max_step > 65535, a Z-slab shard (shard_count > 1),
 * a NULL input or output or a negative count of a query, and the getter or a query before any sdm_ground_update. */
#define SDM_GROUND_UNKNOWN_PASSABLE 0x1u /* occ == -1 cells are passable */
#define SDM_GROUND_IGNORE_MOVABLE   0x2u /* occ >= 1 cells of a movable track are passable, not solid */
#define SDM_GROUND_NONE_IS_LETHAL   0x4u /* columns of class 0 are lethal */
typedef struct {              /* 60 bytes */
  int32_t up_axis, up_sign;
  int32_t h_lo, h_hi;         /* the band, heights in cells */
  uint32_t clearance;         /* 0..255 cells */
  uint32_t max_step;          /* 0..65535 cells */
  uint32_t support_labels[8]; /* bit l of the 256: label l may carry the robot */
  uint32_t flags;
} sdm_ground_options;
typedef struct {       /* 8 bytes */
  uint16_t level, top; /* heights; 0xffff = none */
  uint8_t label;
  uint8_t cls;         /* class | step << 2 | lethal << 3 */
  uint8_t headroom, n_unknown;
} sdm_ground_cell;
typedef struct {       /* 104 bytes */
  uint32_t n_u, n_v, axis_u, axis_v;
  uint32_t n_ground, n_obstacle, n_none, n_step, n_lethal; /* columns */
  uint32_t level_min, level_max;                           /* over the ground columns; 0xffff if there is none */
  sdm_ground_options options;                              /* the build's, echoed */
} sdm_ground_info;
typedef struct {        /* 32 bytes */
  uint32_t col;         /* the point's column word; 0xffffffff outside the map / non-finite */
  uint32_t d2;
  float surface;        /* global coordinate along the up axis of the level cell's upper face: origin[a] + (float)k * voxel_size,
                           k = idx_a + 1 for sign +1, idx_a for sign -1; float32, no contraction; 0 where there is no level */
  int32_t above;        /* h(point) - level; INT32_MIN where there is no level */
  sdm_ground_cell cell;
  float dist;           /* sqrtf((float)d2) * voxel_size, as the distance field's D; -1 when d2 is 0xffffffff */
  uint32_t status;      /* 0 inside, 3 outside / non-finite */
} sdm_ground_result;
typedef struct {        /* 24 bytes */
  float center_u, center_v, dir_u, dir_v, half_len, half_wid;
} sdm_footprint;
typedef struct {        /* 32 bytes */
  uint32_t n_cols, n_lethal, n_none, n_ground; /* covered columns: all, lethal, of class 0, of class 1 */
  uint16_t level_min, level_max;               /* over the covered ground columns; 0xffff if none */
  uint32_t min_d2;                             /* over the covered columns; 0xffffffff if none (or no lethal column at all) */
  uint32_t first_lethal;                       /* the smallest covered lethal column word; 0xffffffff if none */
  uint32_t pad;                                /* 0 */
} sdm_footprint_result;
sdm_status sdm_ground_update(sdm_map *m, const sdm_ground_options *options);
/* Waits; cells and d2 in column-word order (N_u * N_v items each); any of the four pointers may be NULL (origin: the
 * global position of the min corner of cell (0,0,0) of the snapshot). */
sdm_status sdm_get_ground(sdm_map *m, sdm_ground_cell *cells, uint32_t *d2, sdm_ground_info *info, float origin[3]);
sdm_status sdm_query_ground(sdm_map *m, const float *xyz, int64_t n, sdm_ground_result *out, uint32_t flags);
sdm_status sdm_query_footprints(sdm_map *m, const sdm_footprint *fp, int64_t n, sdm_footprint_result *out, uint32_t flags);

/* ---- surface mesh: what does the map look like - to a person, a simulator, a renderer? ----
 * sdm_mesh_update enqueues, on the map's stream, a face mesh of the last frame enqueued before the call and returns
 * without waiting.  Like the other layers the result is a snapshot: it keeps that frame's map center and ring offsets
 * until the next sdm_mesh_update, whatever frames, sdm_clear, sdm_load_state or sdm_set_ring_state come in between;
 * nothing of the map's state is modified and no scratch of the frames' or of another layer is used.  Everything is
 * integer and bitwise reproducible.
 * Cells are map-index cells (i, j, k), cell word i | j << x_n | k << (x_n + y_n).  The map is a block, not a torus: the
 * ring's wrap point is no neighbour relation.
 * Solid cell, from the second word of its result (track, label, occ): occ >= 1 (occ == 1 with SDM_MESH_OBSERVED_ONLY), bit
 * `label` of `labels` set (bit l of word l / 32), track == options.track unless that is -1, and the static / movable flag
 * admits the track (movable: 1 <= track <= max_movable_track).
 * Face: a solid cell and a direction whose face neighbour is not solid or lies outside the map.  kind: what is behind it -
 * 0 a free cell (occ == 0), 1 an unknown cell (occ == -1), 2 nothing, the map ends there, 3 a cell with occ >= 1 that is
 * not solid under these options.  SDM_MESH_SKIP_UNKNOWN_FACES and SDM_MESH_SKIP_BORDER_FACES leave kinds 1 and 2 out.
 * Faces ascend in (cell word, dir).
 * Vertices: the lattice corners (i, j, k) in 0..NX, 0..NY, 0..NZ used by at least one emitted face, each once, ascending in
 * corner word i + (NX + 1) * (j + (NY + 1) * k).
 * Quads: quads[4f .. 4f+3] are the indices into the vertex list of face f's corners q0..q3, counter-clockwise seen from
 * outside; as offsets from the cell's (i, j, k):
 *   dir 0 (-x): 0,0,0  0,0,1  0,1,1  0,1,0      dir 1 (+x): 1,0,0  1,1,0  1,1,1  1,0,1
 *   dir 2 (-y): 0,0,0  1,0,0  1,0,1  0,0,1      dir 3 (+y): 0,1,0  0,1,1  1,1,1  1,1,0
 *   dir 4 (-z): 0,0,0  0,1,0  1,1,0  1,0,0      dir 5 (+z): 0,0,1  1,0,1  1,1,1  0,1,1
 * (q1 - q0) x (q3 - q0) is the outward unit normal, q0 is the quad's smallest corner word, the triangles are (q0, q1, q2)
 * and (q0, q2, q3).  With no skip flag the mesh is closed: every lattice edge carries 2 or 4 faces.
 * Positions: xyz[3v + a] = origin[a] + (float)corner_a * voxel_size in float32, one IEEE operation at a time; origin is
 * the global position of the min corner of cell (0,0,0) of the snapshot.
 * Capacity: max_faces 0 = max(V / 8, 1) faces (V = NX*NY*NZ; at most 6 V), max_vertices 0 = one and a half times the face
 * capacity, rounded down (at most the number of corners; a cell that stands alone has 8 vertices to its 6 faces).  The counts are known on the device only and the update does not wait: a build with more faces
 * or more vertices than either list holds writes no list entry; sdm_get_mesh_faces and sdm_get_mesh_vertices then return
 * SDM_ERR_CAPACITY and still set *n_out to the true count, sdm_get_mesh_info returns SDM_OK with the true n_faces,
 * n_vertices and n_solid (faces_by_dir and faces_by_kind count the faces emitted: zeros); nothing is written out of bounds
 * and nothing is truncated; an update that asks for enough then succeeds.
 * Memory: SDM_MESH_BYTES_PER_WORD = 28 bytes per 64 cells (three bitmasks and the faces' prefix: V * 7 / 16 bytes),
 * SDM_MESH_BYTES_PER_CORNER_WORD = 12 bytes per 64 lattice corners (the corner mask and its prefix),
 * SDM_MESH_BYTES_PER_FACE = 28 bytes per face of capacity (12 B record, 16 B vertex ids), SDM_MESH_BYTES_PER_VERTEX = 8
 * bytes per vertex of capacity, and 44 bytes of counters per 4096 cells: 10.7 MB + 83.9 MB at 256^3 with the default
 * capacities.  Allocated at the first sdm_mesh_update, grown by one that asks for more, freed by sdm_destroy.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map or NULL options, unknown flag bits, both SDM_MESH_STATIC_ONLY and
 * SDM_MESH_MOVABLE_ONLY, track < -1 or > 65535, a negative capacity, cap < 0, a NULL n_out, a Z-slab shard (shard_count >
 * 1), and a getter or sdm_mesh_device before any sdm_mesh_update. */
#define SDM_MESH_STATIC_ONLY        0x01u  /* a cell whose winning track is movable (1 <= track <= max_movable_track) is not solid */
#define SDM_MESH_MOVABLE_ONLY       0x02u  /* only such cells are solid (both bits: SDM_ERR_INVALID_ARGUMENT) */
#define SDM_MESH_OBSERVED_ONLY      0x04u  /* occ == 2 (guessed occupied) is not solid */
#define SDM_MESH_SKIP_UNKNOWN_FACES 0x08u  /* faces of kind 1 are left out: only surfaces seen from known space */
#define SDM_MESH_SKIP_BORDER_FACES  0x10u  /* faces of kind 2 are left out: the mesh is open where the map ends */
#define SDM_MESH_BYTES_PER_WORD 28
#define SDM_MESH_BYTES_PER_CORNER_WORD 12
#define SDM_MESH_BYTES_PER_FACE 28
#define SDM_MESH_BYTES_PER_VERTEX 8
typedef struct {          /* 56 bytes, every field naturally aligned */
  uint32_t flags;
  int32_t  track;         /* -1: any; 0..65535: only cells whose winning track is this one (one object's surface) */
  uint32_t labels[8];     /* bit l of the 256 (binding.label_mask): cells of label l may be solid */
  int64_t  max_faces;     /* capacity of the face list; 0 = max(V / 8, 1); at most 6 V */
  int64_t  max_vertices;  /* capacity of the vertex list; 0 = 3 / 2 of the face capacity; at most the number of corners */
} sdm_mesh_options;
typedef struct {          /* 12 bytes */
  uint32_t cell;          /* the solid cell's word */
  uint16_t track; uint8_t label; int8_t occ;   /* its result, as sdm_get_voxels holds it */
  uint8_t  dir;           /* 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z: the outward normal */
  uint8_t  kind;          /* the neighbour behind the face: 0 free (occ == 0), 1 unknown (occ == -1), 2 outside the map,
                             3 an occ >= 1 cell that is not solid under these options */
  uint16_t pad;           /* 0 */
} sdm_mesh_face;
typedef struct {          /* 8 bytes */
  uint16_t i, j, k, pad;  /* a lattice corner, 0..NX, 0..NY, 0..NZ; pad 0 */
} sdm_mesh_vertex;
typedef struct {          /* 112 bytes, every field naturally aligned */
  uint32_t n_faces, n_vertices, n_solid;       /* true counts, also when over capacity */
  uint32_t faces_by_dir[6], faces_by_kind[4];  /* of the faces emitted */
  uint32_t pad;                                /* 0: the options begin at a multiple of 8 bytes */
  sdm_mesh_options options;                    /* echoed, capacities resolved */
} sdm_mesh_info;
sdm_status sdm_mesh_update(sdm_map *m, const sdm_mesh_options *options);
/* Waits.  info and origin may each be NULL. */
sdm_status sdm_get_mesh_info(sdm_map *m, sdm_mesh_info *info, float origin[3]);
/* Wait; write at most cap entries and set *n_out to the true count.  faces, quads (4 per face), corners and xyz (3 per
 * vertex) may each be NULL. */
sdm_status sdm_get_mesh_faces(sdm_map *m, sdm_mesh_face *faces, uint32_t *quads, int64_t cap, int64_t *n_out);
sdm_status sdm_get_mesh_vertices(sdm_map *m, sdm_mesh_vertex *corners, float *xyz, int64_t cap, int64_t *n_out);
/* Device pointers to the three lists of the last build, for a renderer: valid until the next sdm_mesh_update or
 * sdm_destroy, to be read in stream order on sdm_stream (the counts: sdm_get_mesh_info).  Each may be NULL. */
sdm_status sdm_mesh_device(sdm_map *m, const sdm_mesh_face **faces, const uint32_t **quads, const sdm_mesh_vertex **corners);

/* ---- world archive: what did the map know about a place the block has left? ----
 * Every layer above answers for the block the ring buffer covers; a slab that leaves it is re-stamped and reads unknown
 * from then on.  The world archive is a world-fixed, sparse store of result words that outlives the ring's shifts.
 * sdm_world_update enqueues, on the map's stream, the merge of the result array of the last frame enqueued before the
 * call into the archive and returns without waiting; nothing of the map's state is modified and no scratch of the frames'
 * or of another layer is used.  Everything is integer and bitwise reproducible, including which bricks get room.
 * Geometry.  World cell of map-index cell i on axis a, in the frame the update reads: g = moved_steps[a] + i - (N[a] >> 1)
 * (exact: map_center = moved_steps * voxel_size, pmin = -(N >> 1) * voxel_size).  Brick: 8 x 8 x 8 world cells, b = g >> 3
 * as an arithmetic shift (floor); the cell inside it c = g & 7, cell word cx | cy << 3 | cz << 6.  Brick coordinates are
 * int16 per axis (+-26 km at 0.1 m voxels); a brick outside that range is never created: per update such candidate
 * bricks with a writing cell are counted in out_of_range_last.  Brick order: ascending in (bz, by, bx), signed.
 * World cell of a global position: floorf(p * recip) per axis, one float32 multiply by the map's own recip (1 /
 * voxel_size in float32).  This rule and the map's own cell rule ((p - center) - pmin) * recip can differ inside a rounding
 * sliver at a cell's faces (as a point of sdm_query_points and a segment through it can): query cell centres where that
 * matters.  Global position of a world cell's min corner: (float)g * voxel_size, one float32 multiply per axis.
 * The store holds at most max_bricks bricks, fixed by the first update after creation or after sdm_world_clear: 0 means
 * max(2 * (NX / 8 + 1) * (NY / 8 + 1) * (NZ / 8 + 1), 4096) rounded up to a power of two; at most 2^21.  A later update
 * that asks for a different non-zero capacity while the archive holds bricks is refused (that update waits for the
 * stream; while the archive holds none the buffers are exchanged).  Per brick: 512 words, unknown (0xff000000) until
 * written, and the header below.
 * Which cells write: a block cell writes iff its occ >= 0, except that with SDM_WORLD_STATIC_ONLY a cell with occ >= 1
 * whose track is movable (1 <= track <= max_movable_track) and with SDM_WORLD_OBSERVED_ONLY a cell with occ == 2 write
 * nothing.  A writing cell stores its result word (track | label << 16 | occ << 24) verbatim into its world cell: the
 * latest observation wins.  A cell that does not write leaves the archive as it was: an unknown slab that has just
 * entered the block erases nothing.
 * A brick is created iff it is not in the archive and at least one of its cells writes in this update.  The candidate
 * bricks the block overlaps are taken in brick order and those to create ranked: a new brick of rank r gets room iff
 * n_bricks + r < max_bricks.  The others are not created; their writing cells are dropped for this update and counted
 * (cells) in dropped_last and dropped_total, and a later update may create them once there is room.  n_occupied and n_free
 * of every brick with a writing cell are counted again, last_stamp is set there.
 * sdm_world_clear empties the archive and keeps the buffers; the calls that need an update are refused again until the
 * next one.  sdm_clear, sdm_load_state and sdm_set_ring_state leave the archive alone: later updates trust moved_steps
 * as it then stands, so a caller that sets another ring state and means another world clears the archive itself.
 * Memory: SDM_WORLD_BYTES_PER_BRICK = 2112 bytes per brick of capacity (2048 B of words, 20 B header, 24 B for its two
 * hash slots, 20 B of the brick order's sort buffers and counts), 16 bytes per candidate brick ((ceil(N / 8) + 1) per
 * axis) and the scratch of one scan and one sort: 277 MB at 256^3 with the default capacity of 131072 bricks.
 * Allocated at the first sdm_world_update, freed by sdm_destroy.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options, info or other required pointer, unknown flag bits, a
 * negative capacity, count, first or cap, max_bricks above 2^21, a NULL n_out, a Z-slab shard (shard_count > 1), and -
 * sdm_get_world_info and sdm_world_clear apart - a call before any sdm_world_update. */
#define SDM_WORLD_STATIC_ONLY   0x01u  /* a cell with occ >= 1 whose winning track is movable writes nothing */
#define SDM_WORLD_OBSERVED_ONLY 0x02u  /* a cell with occ == 2 (guessed occupied) writes nothing */
#define SDM_WORLD_BYTES_PER_BRICK 2112
typedef struct {          /* 16 bytes, every field naturally aligned */
  uint32_t flags;
  uint32_t pad;           /* 0 */
  int64_t  max_bricks;    /* capacity of the store; 0: the default, or what it already is */
} sdm_world_options;
typedef struct {          /* 20 bytes */
  int16_t  bx, by, bz;    /* world brick coordinate */
  uint16_t n_occupied;    /* cells with occ >= 1 now */
  uint16_t n_free;        /* cells with occ == 0 now (unknown: 512 - both) */
  uint16_t pad;           /* 0 */
  uint32_t first_stamp;   /* global_time_stamp of the update that created it */
  uint32_t last_stamp;    /* ... of the last update in which one of its cells was written */
} sdm_world_brick;
typedef struct {          /* 8 bytes */
  uint16_t track; uint8_t label; int8_t occ;   /* the world cell's word; 0, 0, -1 where the archive has no brick */
  uint32_t stamp;         /* its brick's last_stamp; 0 where there is none */
} sdm_world_cell;
typedef struct {          /* 80 bytes, every field naturally aligned */
  uint32_t n_bricks, max_bricks, n_updates;    /* n_updates: since creation or sdm_world_clear */
  uint32_t created_last;                       /* bricks the last update created */
  uint32_t dropped_last;                       /* writing cells of bricks the last update had no room for */
  uint32_t out_of_range_last;                  /* candidate bricks of the last update beyond the int16 range */
  uint64_t dropped_total, n_occupied, n_free;  /* dropped_last summed over the updates; the headers' counts summed */
  int32_t  bmin[3], bmax[3];                   /* inclusive brick bounds; 0 and -1 when empty */
  uint32_t flags, stamp;                       /* of the last update */
} sdm_world_info;
sdm_status sdm_world_update(sdm_map *m, const sdm_world_options *options);
sdm_status sdm_world_clear(sdm_map *m);
/* Waits.  SDM_OK with zeros (bmax -1) before any update and after sdm_world_clear. */
sdm_status sdm_get_world_info(sdm_map *m, sdm_world_info *info);
/* Waits.  Headers and - cells not NULL - 512 words per brick, in brick order from the first-th brick on, at most cap of
 * them; *n_out = the archive's brick count.  bricks and cells may each be NULL.  The pool is kept in creation order: the
 * first call of this or of sdm_get_world_occupied after an update sorts it (two passes of the radix sort). */
sdm_status sdm_get_world_bricks(sdm_map *m, sdm_world_brick *bricks, uint32_t *cells, int64_t first, int64_t cap, int64_t *n_out);
/* Every archived cell with occ >= 1 as sdm_point (the min corner as above, track, label, occ), ascending in (brick order,
 * cell word): the world-wide counterpart of sdm_get_occupied.  *n_out is the true count, nothing is written beyond cap.
 * Waits for the count also with SDM_QUERY_ON_DEVICE, with which out is a device pointer filled in stream order. */
sdm_status sdm_get_world_occupied(sdm_map *m, sdm_point *out, int64_t cap, int64_t *n_out, uint32_t flags);
/* Per point the world cell's word and its brick's last_stamp; {0, 0, -1, 0} for a cell of no brick, a non-finite
 * coordinate or a brick out of range.  SDM_QUERY_ON_DEVICE as for sdm_query_points; host mode through the queries'
 * staging area.  n == 0 launches nothing. */
sdm_status sdm_query_world_points(sdm_map *m, const float *xyz, int64_t n, sdm_world_cell *out, uint32_t flags);
/* The dense word grid of the box of world cells cell_min .. cell_min + size - 1, x fastest; cells of no brick hold the
 * unknown word 0xff000000.  Sizes > 0 with a product of at most 2^28.  With SDM_QUERY_ON_DEVICE words is a device pointer
 * and the call does not wait; without it, it goes through the queries' staging area and waits. */
sdm_status sdm_get_world_region(sdm_map *m, const int32_t cell_min[3], const int32_t size[3], uint32_t *words, uint32_t flags);
/* ---- world archive, the way back in: sdm_world_import merges n foreign bricks - what sdm_get_world_bricks of this or of
 * another map returned, kept in a file or not - into the archive under a whole-cell offset; sdm_world_retain trims it.
 * Both are integer and bitwise reproducible like the update, and leave the map's own state alone.
 * Source.  n bricks in any order, cells 512 words per brick in cell-word order.  Of a source header bx, by, bz, first_stamp
 * and last_stamp are read; n_occupied, n_free and pad are ignored, counts are always taken again.  Of several source
 * bricks with the same coordinates the one with the lowest array index is used and the others are ignored entirely; in no
 * other way does the result depend on the order of the array.
 * Geometry.  Source world cell g = 8 * b + c per axis, destination world cell g + cell_offset, destination brick >> 3
 * (arithmetic).  An offset that is no multiple of 8 spreads one source brick over up to 8 destination bricks, and lets one
 * destination brick receive from up to 8 sources.  |cell_offset[a]| <= 2^19.  A destination brick outside the int16 range
 * is never created; such bricks with a writing cell are counted in out_of_range_last.
 * Which cells write: an incoming word writes iff its occ >= 0 and it passes SDM_WORLD_STATIC_ONLY / SDM_WORLD_OBSERVED_ONLY
 * exactly as a block cell does (movable: 1 <= track <= the map's max_movable_track); with SDM_WORLD_IMPORT_FILL the
 * destination cell must also read unknown (no brick there, or occ < 0).  A writing cell stores the word verbatim, a cell
 * that does not write leaves the archive as it is.
 * Creation and capacity: the update's rule.  The distinct destination bricks with at least one writing cell that are not
 * archived are taken in brick order and ranked; one of rank r is created iff n_bricks + r < max_bricks; the writing cells
 * of the others are counted in dropped_last and dropped_total.  created_last, dropped_last and out_of_range_last of
 * sdm_world_info are those of the last update or import; n_updates, flags and stamp keep describing the last
 * sdm_world_update (0 if there was none).
 * Stamps.  The contributors of a destination brick are the source bricks with at least one writing cell in it.  A created
 * brick gets first_stamp = min and last_stamp = max over its contributors' (unsigned), so a round trip into an empty
 * archive reproduces every header byte; an archived brick with a written cell gets min(its own, theirs) and max(its own,
 * theirs); a brick with no written cell is not touched at all.
 * Lifecycle.  Like an update, the first import after creation or sdm_world_clear fixes the capacity (the same default, the
 * same refusal of another non-zero capacity while bricks are held, the same 2^21), and after an import the calls that need
 * an update are served.  n == 0 returns SDM_OK and changes nothing.  Without SDM_WORLD_IMPORT_ON_DEVICE (the import's own
 * bit: SDM_QUERY_ON_DEVICE has the value of SDM_WORLD_STATIC_ONLY and cannot share a word with it) bricks and cells are host
 * pointers, uploaded whole (one import is one ranking), the call waits and frees its device temporaries - the sources'
 * copies, 2068 bytes per brick, and the work arrays - before it returns.  With it they are device pointers read in
 * stream order on the map's stream and the call does not wait; the work arrays (up to 48 bytes per source brick and 40 per
 * destination it can touch: 1, 2, 4 or 8 by the offset's residues) then stay with the map, and a call that needs larger
 * ones than the last waits for the stream once.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map or options, NULL bricks or cells with n > 0, n < 0 or n > 2^21, unknown
 * flag bits, an offset beyond +-2^19, a capacity as refused by sdm_world_update, a Z-slab shard. */
#define SDM_WORLD_IMPORT_FILL 0x10u   /* an incoming cell writes only where the archive's cell reads unknown */
#define SDM_WORLD_IMPORT_ON_DEVICE 0x20u   /* bricks and cells are device pointers; enqueued on the map's stream, no host wait */
typedef struct {            /* 24 bytes, every field naturally aligned */
  uint32_t flags;           /* SDM_WORLD_STATIC_ONLY | SDM_WORLD_OBSERVED_ONLY | SDM_WORLD_IMPORT_FILL | SDM_WORLD_IMPORT_ON_DEVICE */
  int32_t  cell_offset[3];  /* destination world cell = source world cell + cell_offset */
  int64_t  max_bricks;      /* as in sdm_world_options */
} sdm_world_import_options;
sdm_status sdm_world_import(sdm_map *m, const sdm_world_import_options *o, const sdm_world_brick *bricks, const uint32_t *cells, int64_t n);
/* Keeps exactly the bricks inside the inclusive brick box whose last_stamp >= min_last_stamp (a plain unsigned compare)
 * and removes the others; bmax < bmin on an axis is an empty box, which removes everything.  Waits; *n_removed (may be
 * NULL) = the bricks removed.  Kept bricks keep every header and cell byte; afterwards the archive behaves in every
 * observable way like one that only ever held them: lookups, getters, and the capacity rule of later updates and imports
 * with the new n_bricks.  The pool stays dense and in its previous relative order (through a transient copy of the bricks
 * held, freed before the call returns); the hash table is rebuilt.  Unlike sdm_world_clear an empty box keeps capacity,
 * n_updates and the archive itself; dropped_total and the *_last counters are unchanged.  Errors:
 * SDM_ERR_INVALID_ARGUMENT for a NULL map or options, flags != 0, a Z-slab shard, a call before any update or import. */
typedef struct {            /* 32 bytes, every field naturally aligned */
  int32_t  bmin[3], bmax[3];   /* inclusive brick box; bmax < bmin on an axis: an empty box */
  uint32_t min_last_stamp;     /* plain unsigned compare */
  uint32_t flags;              /* 0 */
} sdm_world_retain_options;
sdm_status sdm_world_retain(sdm_map *m, const sdm_world_retain_options *o, int64_t *n_removed);
/* ---- world match: under which whole-cell offset do foreign bricks fit the archive?  sdm_world_match scores every offset
 * of a small window - the 3-D, integer form of a correlative scan matcher - and names the best by a fixed rule: the step
 * in front of sdm_world_import, whose cell_offset it finds.  It reads the archive and writes nothing to it; it is integer
 * and bitwise reproducible like every call of the archive.
 * Sources: exactly as for sdm_world_import - n headers and 512 words each, in any order; of a header only bx, by, bz are
 * read; of several source bricks with the same coordinates the one with the lowest array index is used and the others are
 * ignored entirely.
 * Which source cells count: a cell counts iff its word would write in an import under the same SDM_WORLD_STATIC_ONLY /
 * SDM_WORLD_OBSERVED_ONLY (occ >= 0, movable: 1 <= track <= the map's max_movable_track), so a score predicts what that
 * import would write.  A counted cell with occ >= 1 is OCCUPIED, one with occ == 0 is FREE.
 * Archive cells: the archive's cell at source world cell + candidate offset is classed by the same rule.  It is UNKNOWN
 * where the archive has no brick, the brick lies outside the int16 range, occ < 0 or the word does not pass the flags;
 * otherwise occupied or free by its occ.  A pair with an unknown side counts nowhere.  n_oo, n_of, n_fo, n_ff: the pairs by
 * source class / archive class; n_same: those of n_oo whose label bytes (bits 16 .. 23 of the words) are equal.
 * Candidates: the offsets cell_offset + d, |d[a]| <= radius[a] (0 .. SDM_WORLD_MATCH_MAX_RADIUS per axis), in the order
 * k = ((dz + rz) * (2 ry + 1) + (dy + ry)) * (2 rx + 1) + (dx + rx).  score = w_oo * n_oo + w_same * n_same + w_of * n_of +
 * w_fo * n_fo + w_ff * n_ff in int64.  best: the highest score; ties go to the smallest dx^2 + dy^2 + dz^2, then to the
 * smallest k.  runner_up: the best score among the candidates at Chebyshev distance >= 2 from best, INT64_MIN if there is
 * none - how far the peak stands above everything that is not its own shoulder.  n == 0 is SDM_OK: every count is 0, so
 * the rule picks the centre.
 * The archive is read LIVE, in stream order on the map's stream, as the last sdm_world_update, sdm_world_import or
 * sdm_world_retain before the call left it.  Nothing of the archive, of a snapshot layer or of the map's state changes.
 * Without SDM_WORLD_MATCH_ON_DEVICE every pointer is a host pointer: the sources are uploaded whole, the call waits and
 * frees its device temporaries - the sources' copies, 2068 bytes per brick, the results and the work arrays - before it
 * returns.  With it bricks, cells, scores and result are device pointers, the call enqueues on the map's stream and does
 * not wait (best and runner-up are reduced on the device); the work arrays (at most 48 bytes per source brick, 20 per
 * candidate) then stay with the map until sdm_destroy, and a call that needs larger ones than the last waits for the
 * stream once.  scores may be NULL; otherwise it takes n_candidates records in candidate order.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or result, NULL bricks or cells with n > 0, n < 0 or n > 2^21,
 * unknown flag bits or a non-zero pad, a radius outside 0 .. 8, an offset beyond +-2^19, a Z-slab shard, and a call before
 * any sdm_world_update / sdm_world_import or after sdm_world_clear. */
#define SDM_WORLD_MATCH_ON_DEVICE 0x20u   /* same value and meaning as SDM_WORLD_IMPORT_ON_DEVICE */
#define SDM_WORLD_MATCH_MAX_RADIUS 8
typedef struct {            /* 56 bytes, every field naturally aligned */
  uint32_t flags;           /* SDM_WORLD_STATIC_ONLY | SDM_WORLD_OBSERVED_ONLY | SDM_WORLD_MATCH_ON_DEVICE */
  int32_t  cell_offset[3];  /* the centre candidate, as sdm_world_import_options.cell_offset; |.| <= 2^19 */
  int32_t  radius[3];       /* 0 .. 8 per axis: candidates centre + d, |d[a]| <= radius[a] */
  int32_t  w_oo, w_same, w_of, w_fo, w_ff;   /* signed weights of the five counts */
  uint32_t pad[2];          /* 0 */
} sdm_world_match_options;
typedef struct {            /* 32 bytes */
  int32_t  offset[3];       /* the candidate itself (centre + d) */
  uint32_t n_oo, n_of, n_fo, n_ff;   /* source class / archive class: occupied-occupied, occupied-free, free-occupied, free-free */
  uint32_t n_same;          /* those of n_oo whose label bytes are equal */
} sdm_world_match_score;
typedef struct {            /* 56 bytes: 48 of fields and the pad, every field naturally aligned */
  uint32_t n_candidates, n_sources;  /* (2rx+1)(2ry+1)(2rz+1); distinct source coordinates */
  uint32_t src_occupied, src_free;   /* counted source cells by class */
  int64_t  best_score, runner_up;    /* runner_up: the best score among candidates at Chebyshev distance >= 2 from best; INT64_MIN if none */
  int32_t  best, best_offset[3];     /* candidate index and its offset */
  uint32_t pad[2];                   /* written as 0 */
} sdm_world_match_result;
sdm_status sdm_world_match(sdm_map *m, const sdm_world_match_options *o, const sdm_world_brick *bricks, const uint32_t *cells,
                           int64_t n, sdm_world_match_score *scores /* may be NULL */, sdm_world_match_result *result);

/* ---- world objects: what things does the map remember out there, where is each of them, and how large? ----
 * sdm_world_objects_update builds, on the map's stream, the connected components of occupied archived cells that carry the
 * same label, across brick borders, and a table of them.  Track ids are not stable between sessions and static cells share
 * one id per label, so on the archive an object is a component, not a track (sdm_instances_update is the block's table).
 * Like sdm_world_frontiers_update IT WAITS: for the number of bricks of the field, for the number of counted cells and for
 * the number of objects, and sizes its buffers from them.  Cells are world cells (int32 per axis, brick = cell >> 3).  The
 * archive is what the layer reads: call sdm_world_update first for what is still in the block.
 * Field: the archived bricks at the time of the build; with SDM_WORLD_OBJECTS_BOX those inside the inclusive brick box
 * bmin .. bmax (bmax < bmin on an axis: no brick, which is no error).  Bricks are ranked in brick order - ascending in
 * (bz, by, bx), signed, the order of sdm_get_world_bricks.
 * Counted cell: a cell of a field brick with occ >= 1 whose label l has bit l & 31 of labels[l >> 5] set (all zero: no cell
 * counts, which is no error).  SDM_WORLD_OBJECTS_STATIC_ONLY: a cell on a movable track (1 <= track <= max_movable_track)
 * does not count; SDM_WORLD_OBJECTS_MOVABLE_ONLY: only such cells count (both: SDM_ERR_INVALID_ARGUMENT);
 * SDM_WORLD_OBJECTS_OBSERVED_ONLY: occ == 2 does not count.
 * Key: the label byte of a counted cell; with SDM_WORLD_OBJECTS_BY_TRACK the low 24 bits of its word, label and track.
 * Object: a connected component of counted cells of the field with EQUAL KEYS, in world cells across brick borders,
 * 26-connected, or 6-connected with SDM_WORLD_OBJECTS_FACE_CONNECTED.  Only a counted cell of a field brick joins: a box
 * cuts objects at its sides, a brick beyond the int16 range is absent.  Two cells of one key that touch only at an edge or
 * a corner are joined under 26-connectivity whatever lies between them; a cell of another key carries nothing across.
 * Cell list: the counted cells, ascending in (brick rank, cell word cx | cy << 3 | cz << 6).  An object's identity is the
 * index of its first cell in that list; the table ascends in first_index.  min_cells <= 1 lists every object; a larger
 * value leaves smaller ones out of the table, their cells stay in the list with object SDM_WORLD_OBJECT_UNLISTED.
 * Table entry: track and label are the first cell's; mixed_tracks is 1 if not every cell carries that track (always 0 with
 * BY_TRACK); n_guessed counts occ == 2.  cell_sum: signed sums of the world cells.  cell_sq: the sums of dx dx, dy dy, dz dz,
 * dx dy, dx dz, dy dz with d = cell - first_cell, two's-complement adds modulo 2^64: they cannot wrap while n_cells x E^2 <
 * 2^63, E the largest |d| on any axis - so for every object that stays within 46340 cells of its first cell, and for every
 * object of up to 2^25 cells anywhere (cells lie in +-2^18, so E < 2^19).  Float fields, one IEEE operation at a time, no
 * contraction: box_min = (float)cell_min * voxel_size, box_max = (float)(cell_max + 1) * voxel_size, centroid =
 * (float)(((double)cell_sum / (double)n_cells + 0.5) * (double)voxel_size).  Everything accumulated is an integer sum,
 * minimum, maximum or OR and an object's identity is its smallest cell index: two builds give the same bytes.
 * The build is a SNAPSHOT: it owns the field's coordinates, a hash table of its own from brick to rank, the counted words
 * with their prefix, the lists and the table, holds no pool slot once it returns, and answers the same bytes after any
 * later sdm_world_update, sdm_world_import, sdm_world_retain or sdm_world_clear, until the next sdm_world_objects_update.
 * Nothing of the archive or of the map's state is modified.
 * max_cells > 0 caps the cell-proportional buffers: with more counted cells than that the build writes no list and returns
 * SDM_ERR_CAPACITY; sdm_get_world_objects then still fills info (n_cells and n_guessed are the true counts, the object
 * counts are 0), sdm_get_world_object_cells still sets *n_out to the true count, and they, sdm_get_world_object_labels and
 * sdm_query_world_objects return SDM_ERR_CAPACITY until a build with room.  max_cells == 0: no cap.
 * sdm_get_world_objects: the first min(n, cap) table entries, *n_out = n, the objects listed; info may be NULL.
 * sdm_get_world_object_cells: rows first .. first + cap - 1 of the cell list - cell_xyz three int32 a cell, object the index
 * into the table (SDM_WORLD_OBJECT_UNLISTED: below min_cells), words the archived word - each array may be NULL; *n_out =
 * the cells in all.  sdm_get_world_object_labels: per label the counted cells and the objects in all (those below min_cells
 * included); either array may be NULL.
 * sdm_query_world_objects answers for the last build, for points (three floats each; world cell = floorf(p * recip) per
 * axis) or world cells (three int32 each); exactly one of the two pointers is non-NULL, also with n == 0.  `cell` is as in
 * sdm_query_world_distance: (0, 0, 0) for a point that is non-finite or beyond the brick range, a cell given is echoed as
 * given.  object: the table index; SDM_WORLD_OBJECT_UNLISTED for a counted cell of an object below min_cells;
 * SDM_WORLD_OBJECT_NONE where the cell is no counted cell of the field, the point is not finite, or point or cell are out of
 * range.  index: the cell's place in the cell list, SDM_WORLD_OBJECT_NONE if it has none.  SDM_QUERY_ON_DEVICE as for the
 * other queries (device pointers, enqueued, no wait; out 8-byte aligned), host mode through the queries' staging area.
 * Memory, allocated at the first build, grown by a build that needs more, freed by sdm_destroy:
 *   SDM_WORLD_OBJECTS_BYTES_PER_ARCHIVED_BRICK x (archived bricks + 1, in steps of 256)
 * + SDM_WORLD_OBJECTS_BYTES_PER_BRICK x (bricks of the field, in steps of 256) + 12
 * + SDM_WORLD_OBJECTS_BYTES_PER_CELL x (counted cells, in steps of 4096) + 4
 * + SDM_WORLD_OBJECTS_BYTES_PER_OBJECT x (objects in all, in steps of 1024) + 4
 * + 7192 (the counters, the per-label counters and their landing area).
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or output (n_out, out), unknown flag bits, STATIC_ONLY together
 * with MOVABLE_ONLY, negative max_cells, counts, cap or first, a NULL out with cap > 0, none or both of xyz and cells, a
 * Z-slab shard (shard_count > 1), a build before the archive has had an update or import, and a getter or the query before
 * any build. */
#define SDM_WORLD_OBJECTS_FACE_CONNECTED 0x01u  /* objects under 6- instead of 26-connectivity */
#define SDM_WORLD_OBJECTS_BOX            0x02u  /* the field is the bricks inside bmin .. bmax (inclusive brick box) */
#define SDM_WORLD_OBJECTS_BY_TRACK       0x04u  /* the key is label and track, not the label alone */
#define SDM_WORLD_OBJECTS_STATIC_ONLY    0x08u  /* cells on movable tracks do not count */
#define SDM_WORLD_OBJECTS_MOVABLE_ONLY   0x10u  /* only cells on movable tracks count */
#define SDM_WORLD_OBJECTS_OBSERVED_ONLY  0x20u  /* occ == 2 does not count */
#define SDM_WORLD_OBJECT_UNLISTED 0xfffffffeu   /* a counted cell of an object below min_cells */
#define SDM_WORLD_OBJECT_NONE     0xffffffffu   /* no counted cell of the field */
#define SDM_WORLD_OBJECTS_BYTES_PER_ARCHIVED_BRICK 8  /* box flag, rank */
#define SDM_WORLD_OBJECTS_BYTES_PER_BRICK 240   /* coordinates, pool slot, 27 neighbours, counted words and prefix, two hash slots */
#define SDM_WORLD_OBJECTS_BYTES_PER_CELL  28    /* world cell, word, object, root, scan */
#define SDM_WORLD_OBJECTS_BYTES_PER_OBJECT 288  /* table entry 168, accumulator 112, first cell's index, scan */
typedef struct {            /* 72 bytes, every field naturally aligned */
  uint32_t flags;
  int32_t  min_cells;       /* <= 1: every object is listed */
  int64_t  max_cells;       /* 0: no cap */
  uint32_t labels[8];       /* bit l & 31 of word l >> 5 admits label l */
  int32_t  bmin[3], bmax[3];/* inclusive brick box, read only with SDM_WORLD_OBJECTS_BOX */
} sdm_world_objects_options;
typedef struct {            /* 168 bytes, every field naturally aligned */
  uint32_t first_index;     /* of the object's first cell in the cell list: its identity */
  uint32_t n_cells;
  uint32_t n_guessed;       /* those with occ == 2 */
  uint16_t track;           /* of the first cell */
  uint8_t  label;           /* of the first cell, and of every other */
  uint8_t  mixed_tracks;    /* 1: not every cell carries `track` */
  int32_t  first_cell[3];   /* world cell of the first cell */
  int32_t  cell_min[3], cell_max[3]; /* inclusive */
  uint32_t pad0;            /* 0 */
  int64_t  cell_sum[3];     /* signed */
  int64_t  cell_sq[6];      /* xx yy zz xy xz yz of d = cell - first_cell, modulo 2^64 */
  float    box_min[3], box_max[3], centroid[3];
  uint32_t pad1;            /* 0 */
} sdm_world_object;
typedef struct {            /* 40 bytes, every field naturally aligned */
  uint32_t n_bricks;        /* bricks of the field */
  uint32_t n_objects;       /* objects listed: the table's length */
  uint32_t n_objects_total; /* objects in all, those below min_cells included */
  uint32_t flags;
  int64_t  n_cells;         /* counted cells */
  int64_t  n_guessed;       /* those with occ == 2 */
  int32_t  min_cells;       /* as given */
  uint32_t stamp;           /* the archive's stamp at the build: sdm_world_info.stamp */
} sdm_world_objects_info;
typedef struct {            /* 24 bytes */
  int32_t  cell[3];         /* the world cell asked about */
  uint32_t object;          /* table index, SDM_WORLD_OBJECT_UNLISTED or SDM_WORLD_OBJECT_NONE */
  uint32_t index;           /* place in the cell list; SDM_WORLD_OBJECT_NONE if none */
  uint32_t pad;             /* 0 */
} sdm_world_object_result;
sdm_status sdm_world_objects_update(sdm_map *m, const sdm_world_objects_options *o);
sdm_status sdm_get_world_objects(sdm_map *m, sdm_world_object *out, int32_t cap, int32_t *n_out, sdm_world_objects_info *info);
sdm_status sdm_get_world_object_cells(sdm_map *m, int32_t *cell_xyz, uint32_t *object, uint32_t *words, int64_t first,
                                      int64_t cap, int64_t *n_out);
sdm_status sdm_get_world_object_labels(sdm_map *m, uint64_t cells[256], uint32_t objects[256]);
sdm_status sdm_query_world_objects(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n,
                                   sdm_world_object_result *out, uint32_t flags);

/* ---- world changes: is the place the block has come back to still as the archive remembers it? ----
 * sdm_world_changes_update compares, on the map's stream, what the block sees with what the archive remembers, cell by
 * cell, lists the cells that changed, joins them into regions and makes a table of those.  The intended use is one call
 * between a frame and its archiving: sdm_update -> sdm_world_changes_update -> sdm_world_update (which then overwrites the
 * difference this call has found).  Like sdm_world_objects_update IT WAITS, three times: for the bricks of the field, for
 * the listed cells and for the regions, and sizes its buffers from them.  Cells are world cells (int32 per axis, brick =
 * cell >> 3).
 * What is compared: the block side is the result array of the last frame enqueued before the call; the archive side is the
 * archive as the last sdm_world_update, sdm_world_import or sdm_world_retain left it, read live in stream order.  The two
 * sides meet at the same world cell, g = moved_steps + i - (N >> 1) per axis: sdm_world_update's own geometry.
 * Field candidates: the bricks the block overlaps, at most ceil(N / 8) + 1 per axis, in brick order - ascending in
 * (bz, by, bx) -, the candidates of sdm_world_update.  Cells of such a brick that lie outside the block read unknown on the
 * block side.
 * Class of a side: a word is OCCUPIED (occ >= 1) or FREE (occ == 0) iff it would write under the archive's own rule with
 * this layer's flags in place of the archive's: occ >= 0; with SDM_WORLD_CHANGES_STATIC_ONLY no movable track on an occupied
 * cell (1 <= track <= max_movable_track); with SDM_WORLD_CHANGES_OBSERVED_ONLY no occ == 2.  Everything else is UNKNOWN.
 * Both sides go through the same rule.  The archive side is also UNKNOWN where the archive has no brick, where the brick is
 * beyond the int16 range, and - with SDM_WORLD_CHANGES_OLDER - where the brick's last_stamp > max_last_stamp (a plain
 * unsigned compare, like sdm_world_retain's min_last_stamp).
 * Class of a cell, block / archive:  O / F  SDM_WORLD_CHANGE_APPEARED (1);  F / O  SDM_WORLD_CHANGE_VANISHED (2);  O / O with
 * different label bytes  SDM_WORLD_CHANGE_RELABELLED (3);  O / O with equal label bytes counts as n_same_occupied;  F / F
 * n_same_free;  O / U  n_new_occupied;  F / U  n_new_free;  U / O and U / F  n_remembered;  U / U nothing.  The three
 * change classes count as n_appeared, n_vanished, n_relabelled.  Three more close the sums: n_known_now and n_known_before,
 * the cells of either side that are not UNKNOWN (n_known_now = the three changes + the two same + the two new;
 * n_known_before = the three changes + the two same + n_remembered), and n_outside, the cells of the candidates that lie
 * outside the block.  Every counter is a true count over all candidates, before any mask.
 * Listed cell: a changed cell whose class has its bit set in `classes` (bit 1, 2 or 3) and one of whose occupied sides'
 * labels l is admitted by `labels` (bit l & 31 of labels[l >> 5], the rule of the world objects): the block's label for
 * APPEARED, the archive's for VANISHED, either for RELABELLED.  All-zero masks list nothing, which is no error.
 * Field: the candidates with at least one listed cell, ranked in brick order.
 * Cell list: the listed cells, ascending in (brick rank, cell word cx | cy << 3 | cz << 6); per cell the world cell, the
 * block's word `now`, the archive's word `before`, the class and the region index.
 * Region: a connected component of listed cells with EQUAL KEYS, in world cells across brick borders, 26-connected, or
 * 6-connected with SDM_WORLD_CHANGES_FACE_CONNECTED.  The key is the class; with SDM_WORLD_CHANGES_BY_LABEL it is
 * class | label_now << 8 | label_before << 16, a side's label being 0 when that side is not occupied.  As with the world
 * objects two cells of one key that touch only at an edge or a corner are joined under 26-connectivity whatever lies
 * between them, and a cell of another key carries nothing across.  A region's identity is the list index of its first
 * cell; the table ascends in first_index.  min_cells <= 1 lists every region; a larger value leaves smaller regions out of
 * the table, their cells stay in the list with region SDM_WORLD_CHANGE_UNLISTED: the debounce for the flicker at occupancy
 * borders.
 * Table entry: cls, label_now and label_before are the first cell's (a side's label 0 when it is not occupied); mixed is 1
 * if not every cell has that label pair (always 0 with BY_LABEL).  cell_sum: signed sums of the world cells.  Float fields,
 * one IEEE operation at a time, no contraction: box_min = (float)cell_min * voxel_size, box_max = (float)(cell_max + 1) *
 * voxel_size, centroid = (float)(((double)cell_sum / (double)n_cells + 0.5) * (double)voxel_size).  Everything accumulated
 * is an integer sum, minimum, maximum or OR and a region's identity is its smallest cell index: two builds give the same
 * bytes.
 * The build is a SNAPSHOT: it owns the field's coordinates, a hash table of its own from brick to rank, the listed words
 * with their prefix, the lists and the table, and answers the same bytes after any later frame, sdm_world_update,
 * sdm_world_import, sdm_world_retain or sdm_world_clear, until the next sdm_world_changes_update.  Nothing of the map or of
 * the archive is modified.
 * max_cells > 0 caps the cell-proportional buffers: with more listed cells than that the build writes no list and returns
 * SDM_ERR_CAPACITY; sdm_get_world_changes then still fills info (the eleven counters, n_candidates, n_bricks and n_cells
 * are the true counts, the region counts are 0), sdm_get_world_change_cells still sets *n_out to the true count, and they,
 * sdm_get_world_change_labels and sdm_query_world_changes return SDM_ERR_CAPACITY until a build with room.  max_cells == 0:
 * no cap.
 * sdm_get_world_changes: the first min(n, cap) table entries, *n_out = n, the regions listed; info may be NULL.
 * sdm_get_world_change_cells: rows first .. first + cap - 1 of the cell list - cell_xyz three int32 a cell, now and before
 * the two words, cls the class (one byte), region the index into the table (SDM_WORLD_CHANGE_UNLISTED: below min_cells);
 * every array may be NULL; *n_out = the cells in all.  sdm_get_world_change_labels: listed cells per label - an appeared or
 * relabelled cell under the block's label, a vanished cell under the archive's; each array may be NULL.
 * sdm_query_world_changes answers for the last build, for points (three floats each; world cell = floorf(p * recip) per
 * axis) or world cells (three int32 each) under the protocol of sdm_query_world_objects: exactly one of the two pointers is
 * non-NULL, also with n == 0; `cell` is (0, 0, 0) for a point that is non-finite or beyond the brick range, a cell given is
 * echoed as given.  region: the table index, SDM_WORLD_CHANGE_UNLISTED for a listed cell of a region below min_cells,
 * SDM_WORLD_CHANGE_NONE where the cell is no listed cell; index: its place in the cell list or SDM_WORLD_CHANGE_NONE; cls:
 * its class, SDM_WORLD_CHANGE_NONE if it has none.  SDM_QUERY_ON_DEVICE as for the other queries.
 * Memory, allocated at the first build, grown by a build that needs more, freed by sdm_destroy:
 *   SDM_WORLD_CHANGES_BYTES_PER_CANDIDATE x (the map's largest candidate count + 1, in steps of 256)
 * + SDM_WORLD_CHANGES_BYTES_PER_BRICK x (bricks of the field, in steps of 256) + 12, which counts two hash slots a brick: the
 *   table has the power of two at or above twice that stepped count, so up to 12 more bytes for each of up to two more slots a brick
 * + SDM_WORLD_CHANGES_BYTES_PER_CELL x (listed cells, in steps of 4096) + 4
 * + SDM_WORLD_CHANGES_BYTES_PER_REGION x (regions in all, in steps of 1024) + 4
 * + 23576 (the counters in 64 spread copies, the per-label counters and their landing area).
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or output (n_out, out), unknown flag or class bits, non-zero
 * pads, negative max_cells, counts, cap or first, a NULL out with cap > 0, none or both of xyz and cells, a Z-slab shard
 * (shard_count > 1), a build before the archive has had an update or import, and a getter or the query before any build.
 * An archive that holds no brick the block overlaps is no error: everything known then counts as new. */
#define SDM_WORLD_CHANGES_FACE_CONNECTED 0x01u  /* regions under 6- instead of 26-connectivity */
#define SDM_WORLD_CHANGES_BY_LABEL       0x02u  /* the key is class and label pair, not the class alone */
#define SDM_WORLD_CHANGES_STATIC_ONLY    0x04u  /* an occupied cell on a movable track reads unknown, on either side */
#define SDM_WORLD_CHANGES_OBSERVED_ONLY  0x08u  /* occ == 2 reads unknown, on either side */
#define SDM_WORLD_CHANGES_OLDER          0x10u  /* a brick with last_stamp > max_last_stamp reads unknown */
#define SDM_WORLD_CHANGE_APPEARED   1u          /* occupied now, free before */
#define SDM_WORLD_CHANGE_VANISHED   2u          /* free now, occupied before */
#define SDM_WORLD_CHANGE_RELABELLED 3u          /* occupied on both sides, the label bytes differ */
#define SDM_WORLD_CHANGE_UNLISTED 0xfffffffeu   /* a listed cell of a region below min_cells */
#define SDM_WORLD_CHANGE_NONE     0xffffffffu   /* no listed cell */
#define SDM_WORLD_CHANGES_BYTES_PER_CANDIDATE 204  /* flag, rank, pool slot, listed words and two class planes */
#define SDM_WORLD_CHANGES_BYTES_PER_BRICK 368   /* coordinates, pool slot, 27 neighbours, listed words, prefix, two class planes, two hash slots */
#define SDM_WORLD_CHANGES_BYTES_PER_CELL  37    /* world cell, now, before, key, class, region, root, scan */
#define SDM_WORLD_CHANGES_BYTES_PER_REGION 176  /* table entry 112, accumulator 56, first cell's index, scan */
typedef struct {            /* 64 bytes, every field naturally aligned */
  uint32_t flags;
  int32_t  min_cells;       /* <= 1: every region is listed */
  int64_t  max_cells;       /* 0: no cap */
  uint32_t labels[8];       /* bit l & 31 of word l >> 5 admits label l */
  uint32_t classes;         /* bit c admits class c: 0x2 appeared, 0x4 vanished, 0x8 relabelled */
  uint32_t max_last_stamp;  /* read only with SDM_WORLD_CHANGES_OLDER */
  uint32_t pad[2];          /* 0 */
} sdm_world_changes_options;
typedef struct {            /* 112 bytes, every field naturally aligned */
  uint32_t first_index;     /* of the region's first cell in the cell list: its identity */
  uint32_t n_cells;
  uint8_t  cls;             /* of the first cell, and of every other */
  uint8_t  label_now;       /* of the first cell; 0 where the block side is not occupied */
  uint8_t  label_before;    /* of the first cell; 0 where the archive side is not occupied */
  uint8_t  mixed;           /* 1: not every cell carries that label pair */
  int32_t  first_cell[3];   /* world cell of the first cell */
  int32_t  cell_min[3], cell_max[3]; /* inclusive */
  int64_t  cell_sum[3];     /* signed */
  float    box_min[3], box_max[3], centroid[3];
  uint32_t pad;             /* 0 */
} sdm_world_change_region;
typedef struct {            /* 128 bytes, every field naturally aligned */
  uint64_t n_appeared, n_vanished, n_relabelled;  /* the three change classes, before any mask */
  uint64_t n_same_occupied, n_same_free;          /* O / O with equal labels, F / F */
  uint64_t n_new_occupied, n_new_free;            /* O / U, F / U */
  uint64_t n_remembered;                          /* U / O and U / F */
  uint64_t n_known_now, n_known_before;           /* cells of the block side / of the archive side that are not UNKNOWN */
  uint64_t n_outside;                             /* cells of the candidates that lie outside the block */
  uint32_t n_candidates;    /* bricks the block overlaps */
  uint32_t n_bricks;        /* bricks of the field */
  int64_t  n_cells;         /* listed cells */
  uint32_t n_regions;       /* regions listed: the table's length */
  uint32_t n_regions_total; /* regions in all, those below min_cells included */
  uint32_t flags;
  int32_t  min_cells;       /* as given */
  uint32_t frame_stamp;     /* the frame's global_time_stamp */
  uint32_t stamp;           /* the archive's stamp at the build: sdm_world_info.stamp */
} sdm_world_changes_info;
typedef struct {            /* 24 bytes */
  int32_t  cell[3];         /* the world cell asked about */
  uint32_t region;          /* table index, SDM_WORLD_CHANGE_UNLISTED or SDM_WORLD_CHANGE_NONE */
  uint32_t index;           /* place in the cell list; SDM_WORLD_CHANGE_NONE if none */
  uint32_t cls;             /* the class; SDM_WORLD_CHANGE_NONE if none */
} sdm_world_change_result;
sdm_status sdm_world_changes_update(sdm_map *m, const sdm_world_changes_options *o);
sdm_status sdm_get_world_changes(sdm_map *m, sdm_world_change_region *regions, int32_t cap, int32_t *n_out, sdm_world_changes_info *info);
sdm_status sdm_get_world_change_cells(sdm_map *m, int32_t *cell_xyz, uint32_t *now, uint32_t *before, uint8_t *cls, uint32_t *region,
                                      int64_t first, int64_t cap, int64_t *n_out);
sdm_status sdm_get_world_change_labels(sdm_map *m, uint64_t appeared[256], uint64_t vanished[256], uint64_t relabelled[256]);
sdm_status sdm_query_world_changes(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n,
                                   sdm_world_change_result *out, uint32_t flags);

/* ---- world reach: how far is it, through everything the map remembers, to a place the block has left? ----
 * sdm_world_reach_update builds, on the map's stream, the travel-cost field of sdm_reach_update over the bricks of the
 * world archive instead of the map block, from a set of start cells.  Like sdm_reach_update IT WAITS: the host decides
 * when the relaxation is at rest, and no kernel ever waits for another workgroup.  Cells are world cells (int32 per
 * axis): world cell of a point = floorf(p * recip) per axis, the archive's rule; brick = cell >> 3 (arithmetic).
 * The field is the set of archived bricks at the time of the build; with SDM_WORLD_REACH_BOX those inside the inclusive
 * brick box bmin .. bmax, and a brick outside it is as if absent.  Bricks are ranked in brick order - ascending in
 * (bz, by, bx), signed, the order of sdm_get_world_bricks: without a box row r of sdm_get_world_reach belongs to row r of
 * sdm_get_world_bricks taken at the same moment.  A cell of no brick of the field is never traversable under any flag:
 * that bounds the search.  A neighbour brick whose coordinate would leave the int16 range is absent.
 * The build is a SNAPSHOT: it owns its copy of the bricks' coordinates, a hash table of its own from brick to rank, the
 * neighbour ranks, the masks and the costs, and answers the same bytes after any later sdm_world_update,
 * sdm_world_import, sdm_world_retain or sdm_world_clear, until the next sdm_world_reach_update.  Nothing of the archive
 * or of the map's state is modified.
 * Cell class, from the archived word: traversable iff occ == 0; with SDM_WORLD_REACH_THROUGH_UNKNOWN also occ == -1 inside
 * a brick of the field; with SDM_WORLD_REACH_IGNORE_MOVABLE a cell with occ >= 1 and 1 <= track <= max_movable_track counts
 * as occ == 0 and is no obstacle.  An obstacle is a cell with occ >= 1 after that rule.
 * Inflation: with inflate = r (1 or 2) a cell is traversable only if no obstacle cell lies within Chebyshev distance r of
 * it.  Cells of no brick and unknown cells are no obstacles; the obstacles of absent bricks - with a box, of bricks outside
 * it - do not exist.
 * Moves, weights, field and descent are word for word those of sdm_reach_update: the 26 offsets numbered
 * (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), six with SDM_WORLD_REACH_FACE_CONNECTED; a move c -> c + o is allowed iff all 2,
 * 4 or 8 cells c + s, s_a in {0, o_a}, are traversable cells of the field; weights 10 / 14 / 17; the descent takes the
 * smallest allowed move number with cost(c + o) + w(o) == cost(c).  Everything is integer and bitwise reproducible.
 * Budget: 17 x 512 x 2^21 does not fit 32 bits, so the effective budget is max_cost if that is non-zero and 0xfffffffe
 * otherwise; a cell whose true cost exceeds it reads 0xffffffff, additions saturate, and the truncated field is still
 * exact because every prefix of a cheapest path lies within the budget.
 * Starts and goals: points (three floats each) or world cells (three int32 each); exactly one of the two pointers is
 * non-NULL, also with a count of 0.  A start on a cell that is not traversable, in no brick of the field, non-finite or
 * beyond the brick range is ignored; duplicates are fine; no usable start is no error: every cell then reads unreachable.
 * sdm_get_world_reach waits: coords takes three int16 (bx, by, bz) and cost 512 words (cell word cx | cy << 3 | cz << 6;
 * 0xffffffff: unreachable or not traversable) per brick of rows first .. first + cap - 1 of the field; *n_out = the bricks
 * of the field; coords, cost and info may each be NULL.
 * sdm_query_world_reach / sdm_world_reach_paths answer for the last build; SDM_QUERY_ON_DEVICE as for the other queries
 * (device pointers, enqueued, no wait; out 8-byte aligned), host mode through the queries' staging area.  Row g of
 * cells_out (n rows of max_len * 3 int32) takes the world cells of goal g's path from the goal to a start, both included;
 * len_out[g] is its true length, 0 where there is none, and may exceed max_len: only the first min(len, max_len) cells
 * are written, the rest of the row is left untouched, in host mode too.
 * Memory, per brick of the field (in steps of 256 bricks): 2048 B of cost, 64 B of traversable and 64 B of obstacle mask,
 * 108 B of neighbour ranks, 8 B of coordinates, its two hash slots (24 B), 4 B of list and a bit of activity: about 2320 B.
 * Allocated at the first build, grown by a build of more bricks, freed by sdm_destroy.  A build also holds 12 B per
 * archived brick (flags, ranks, pool slots) until it returns.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or output (n_out, out, len_out; cells_out with max_len > 0),
 * none or both start / goal pointers, unknown flag bits, inflate > 2, a non-zero pad, bmax < bmin with the box flag,
 * negative counts, first, cap or max_len, a Z-slab shard (shard_count > 1), a build before the archive has had an update
 * or import, and the getter or a query before any build.  SDM_ERR_NOT_CONVERGED if the relaxation has not come to rest
 * after 512 x n_bricks rounds: a defect, never a result. */
#define SDM_WORLD_REACH_FACE_CONNECTED  0x01u  /* the six face moves only */
#define SDM_WORLD_REACH_THROUGH_UNKNOWN 0x02u  /* cells with occ == -1 inside a brick of the field are traversable too */
#define SDM_WORLD_REACH_IGNORE_MOVABLE  0x04u  /* occupied cells on movable tracks count as free */
#define SDM_WORLD_REACH_BOX             0x08u  /* the field is the bricks inside bmin .. bmax */
typedef struct {            /* 40 bytes, every field naturally aligned */
  uint32_t flags;
  uint32_t inflate;         /* 0, 1 or 2 cells */
  uint32_t max_cost;        /* 0: no budget */
  uint32_t pad;             /* 0 */
  int32_t  bmin[3], bmax[3];/* inclusive brick box, read only with SDM_WORLD_REACH_BOX */
} sdm_world_reach_options;
typedef struct {            /* 40 bytes */
  uint32_t n_bricks;        /* bricks in the field */
  uint32_t n_starts_used;   /* distinct start cells that were traversable */
  uint32_t n_traversable, n_reached, max_cost_reached;
  uint32_t rounds;          /* relaxation rounds the build took (diagnostic; not part of the bitwise contract) */
  uint32_t flags, inflate, max_cost;
  uint32_t stamp;           /* the archive's stamp at the build: sdm_world_info.stamp */
} sdm_world_reach_info;
typedef struct {            /* 24 bytes */
  uint32_t cost;            /* 0xffffffff: no path */
  float    metres;          /* (float)cost * (voxel_size * 0.1f), float32, no contraction; -1 where no path */
  int32_t  cell[3];         /* the goal's world cell; (0, 0, 0) for a point that is non-finite or beyond the brick range */
  uint8_t  next;            /* move number of the first descent step; 13 at a start; 255 where no path */
  uint8_t  status;          /* 0 reached, 1 traversable but unreachable (or beyond the budget), 2 in a brick of the field but
                               not traversable, 3 in no brick of the field / non-finite / out of range */
  uint16_t pad;             /* 0 */
} sdm_world_reach_result;
sdm_status sdm_world_reach_update(sdm_map *m, const sdm_world_reach_options *o, const float *start_xyz, const int32_t *start_cells,
                                  int64_t n_starts);
sdm_status sdm_get_world_reach(sdm_map *m, int16_t *coords, uint32_t *cost, int64_t first, int64_t cap, int64_t *n_out,
                               sdm_world_reach_info *info);
sdm_status sdm_query_world_reach(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, sdm_world_reach_result *out, uint32_t flags);
sdm_status sdm_world_reach_paths(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, int32_t max_len, int32_t *cells_out,
                                 int32_t *len_out, uint32_t flags);

/* ---- world frontiers: where, beyond the block, is it worth going? ----
 * sdm_world_frontiers_update builds, on the map's stream, the frontiers of sdm_frontiers_update over the bricks of the
 * world archive instead of the map block: the free cells that border never-observed space, their connected clusters
 * across brick borders and a table of them.  Like sdm_world_reach_update IT WAITS: it reads the number of bricks of the
 * field and then the number of frontier cells, and sizes its buffers from them.  Cells are world cells (int32 per axis,
 * brick = cell >> 3), the archive's origin is the world's, as in sdm_query_world_points.  The archive is what the layer
 * reads: frontiers that mix the live block and the archive do not exist - call sdm_world_update first.
 * Field: the archived bricks at the time of the build; with SDM_WORLD_FRONTIERS_BOX those inside the inclusive brick box
 * bmin .. bmax (bmax < bmin on an axis: no brick, which is no error).  Bricks are ranked in brick order - ascending in
 * (bz, by, bx), signed, the order of sdm_get_world_bricks.
 * Frontier cell: a cell of a field brick whose archived word has occ == 0 and at least one of whose six face neighbours
 * reads unknown; unknown_faces counts those neighbours (1 .. 6).  A neighbour reads unknown if its archived word has
 * occ == -1, and also if it lies in no archived brick - the world is unbounded, an absent brick was never observed -
 * unless SDM_WORLD_FRONTIERS_INSIDE_BRICKS is given.  The neighbour's word is read from the whole archive, not only from
 * the field: a box makes no false frontier along its sides.  A neighbour brick beyond the int16 range is absent.
 * Cell order: the cell list ascends in (brick rank, cell word cx | cy << 3 | cz << 6).
 * Cluster: a connected component of frontier cells of the field, in world cells across brick borders, 26-connected, or
 * 6-connected with SDM_WORLD_FRONTIERS_FACE_CONNECTED.  Its identity is its first cell in the list; the table ascends in
 * first_index.  min_cells <= 1 keeps every cluster; a larger value leaves smaller clusters out of the table, their cells
 * stay in the list with cluster 0xffffffff.
 * Float fields of a cluster, one IEEE operation at a time, no contraction: box_min = (float)cell_min * voxel_size,
 * box_max = (float)(cell_max + 1) * voxel_size, centroid = (float)(((double)cell_sum / (double)n_cells + 0.5) *
 * (double)voxel_size).  Everything accumulated is an integer sum, minimum or maximum and a cluster's identity is its
 * smallest cell index: two builds give the same bytes.
 * The build is a SNAPSHOT: the getters return the same bytes after any later sdm_world_update, sdm_world_import,
 * sdm_world_retain or sdm_world_clear, until the next sdm_world_frontiers_update.  It holds lists, no pool slot, once it
 * returns.  Nothing of the archive or of the map's state is modified.
 * max_cells > 0 caps the cell-proportional buffers: with more frontier cells than that the build writes no list and
 * returns SDM_ERR_CAPACITY; sdm_get_world_frontier_clusters then still fills info (n_cells is the true count, the cluster
 * counts are 0) and sdm_get_world_frontier_cells still sets *n_out to the true count, and both return SDM_ERR_CAPACITY
 * until a build with room.  max_cells == 0: no cap.
 * sdm_get_world_frontier_clusters: the first min(n, cap) table entries, *n_out = n, the clusters listed; info may be NULL.
 * sdm_get_world_frontier_cells: rows first .. first + cap - 1 of the cell list - cell_xyz three int32 a cell, cluster the
 * index into the table (0xffffffff: below min_cells), unknown_faces - each array may be NULL; *n_out = the cells in all.
 * Memory, allocated at the first build, grown by a build that needs more, freed by sdm_destroy:
 *   SDM_WORLD_FRONTIERS_BYTES_PER_ARCHIVED_BRICK x (archived bricks + 1, in steps of 256) + 4 x max_bricks
 * + SDM_WORLD_FRONTIERS_BYTES_PER_BRICK x (bricks of the field, in steps of 256) + 12
 * + SDM_WORLD_FRONTIERS_BYTES_PER_CELL x (frontier cells, in steps of 4096) + 4.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map or options, unknown flag bits, negative max_cells, cap or first, a NULL
 * n_out, a NULL out with cap > 0, a Z-slab shard (shard_count > 1), a build before the archive has had an update or
 * import, and a getter before any build. */
#define SDM_WORLD_FRONTIERS_FACE_CONNECTED 0x1u  /* clusters under 6- instead of 26-connectivity */
#define SDM_WORLD_FRONTIERS_BOX            0x2u  /* the field is the bricks inside bmin .. bmax (inclusive brick box) */
#define SDM_WORLD_FRONTIERS_INSIDE_BRICKS  0x4u  /* a neighbour in no archived brick is NOT unknown */
#define SDM_WORLD_FRONTIERS_BYTES_PER_ARCHIVED_BRICK 136  /* box flag, rank, the free and the unknown words */
#define SDM_WORLD_FRONTIERS_BYTES_PER_BRICK 240  /* coordinates, place, 27 + 6 neighbours, frontier words and their prefix */
#define SDM_WORLD_FRONTIERS_BYTES_PER_CELL  201  /* world cell, cluster, root, scan, unknown_faces, accumulator, table entry */
typedef struct {            /* 40 bytes, every field naturally aligned */
  uint32_t flags;
  int32_t  min_cells;       /* <= 1: every cluster is listed */
  int64_t  max_cells;       /* 0: no cap */
  int32_t  bmin[3], bmax[3];/* inclusive brick box, read only with SDM_WORLD_FRONTIERS_BOX */
} sdm_world_frontiers_options;
typedef struct {            /* 120 bytes, every field naturally aligned */
  uint32_t first_index;     /* of the cluster's first cell in the cell list: its identity */
  uint32_t n_cells;
  uint32_t n_unknown_faces; /* the sum of its cells' unknown_faces */
  uint32_t pad0;            /* 0 */
  int32_t  first_cell[3];   /* world cell of the first cell */
  int32_t  cell_min[3], cell_max[3]; /* inclusive */
  uint32_t pad1;            /* 0 */
  int64_t  cell_sum[3];     /* signed */
  float    box_min[3], box_max[3], centroid[3];
  uint32_t pad2;            /* 0 */
} sdm_world_frontier_cluster;
typedef struct {            /* 48 bytes, every field naturally aligned */
  uint32_t n_bricks;        /* bricks of the field */
  uint32_t n_clusters;      /* clusters listed: the table's length */
  uint32_t n_clusters_total;/* clusters in all, those below min_cells included */
  uint32_t flags;
  int64_t  n_cells;         /* frontier cells */
  int64_t  n_unknown_faces; /* the sum of unknown_faces over the cells */
  int64_t  n_absent_faces;  /* how many of those faces look into bricks the archive does not have */
  int32_t  min_cells;       /* as given */
  uint32_t stamp;           /* the archive's stamp at the build: sdm_world_info.stamp */
} sdm_world_frontiers_info;
sdm_status sdm_world_frontiers_update(sdm_map *m, const sdm_world_frontiers_options *o);
sdm_status sdm_get_world_frontier_clusters(sdm_map *m, sdm_world_frontier_cluster *out, int32_t cap, int32_t *n_out,
                                           sdm_world_frontiers_info *info);
sdm_status sdm_get_world_frontier_cells(sdm_map *m, int32_t *cell_xyz, uint32_t *cluster, uint8_t *unknown_faces,
                                        int64_t first, int64_t cap, int64_t *n_out);

/* ---- world distance field: how close is a remembered place to an obstacle? ----
 * sdm_world_esdf_update builds, on the map's stream, a TRUNCATED Euclidean distance field over the bricks of the world
 * archive: for every cell of a field brick the squared distance, in world cells, to the nearest archived obstacle cell and
 * the offset to it, exact up to `radius` cells (1 .. SDM_WORLD_ESDF_MAX_RADIUS) and "far" beyond.  IT WAITS ONCE, for the
 * number of bricks of the field, which sizes the buffers; the field itself is enqueued and the getter waits for it.  Cells
 * are world cells (int32 per axis, brick = cell >> 3), the archive's origin is the world's.
 * Obstacles: an archived cell with occ >= 1; with SDM_WORLD_ESDF_STATIC_ONLY a cell on a movable track (1 <= track <=
 * max_movable_track) is none - the rule of SDM_WORLD_REACH_IGNORE_MOVABLE; with SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE every
 * cell with occ == -1 is one too, and so is EVERY CELL OF A BRICK THE ARCHIVE DOES NOT HAVE (a brick beyond the int16 range
 * is absent).  Obstacles come from the whole archive, not only from the field: a box hides no wall behind its side.
 * Field: the archived bricks at the time of the build; with SDM_WORLD_ESDF_BOX those inside the inclusive brick box
 * bmin .. bmax (bmax < bmin on an axis: no brick, which is no error).  Bricks are ranked in brick order - ascending in
 * (bz, by, bx), signed: without a box row r of sdm_get_world_esdf is row r of sdm_get_world_bricks taken at the same moment.
 * Values, for a cell c of a field brick and R = radius: d2(c) = min over obstacle cells q of |c - q|^2.  If d2(c) <= R^2 the
 * field holds it and offset = q - c of the nearest obstacle; among equally near obstacles the one with the SMALLEST WORLD
 * CELL IN (z, y, x) ORDER wins, so the whole field is defined bit for bit.  An obstacle cell reads 0 / (0, 0, 0).
 * Otherwise d2 = SDM_WORLD_ESDF_NONE and offset (0, 0, 0).
 * The build is a SNAPSHOT: it owns the bricks' coordinates, a hash table of its own from brick to rank and the field, holds
 * no pool slot, and answers the same bytes after any later sdm_world_update, sdm_world_import, sdm_world_retain or
 * sdm_world_clear, until the next sdm_world_esdf_update.  Nothing of the archive or of the map's state is modified.
 * sdm_get_world_esdf waits: per brick of rows first .. first + cap - 1 coords takes three int16 (bx, by, bz), d2 512 uint16
 * (cell word cx | cy << 3 | cz << 6) and offset 512 x 3 int8 (dx, dy, dz); each array and info may be NULL; *n_out = the
 * bricks of the field.  info: n_obstacle_cells counts the field cells that are obstacles, n_near_cells those with
 * d2 <= R^2, the obstacle cells included.
 * sdm_query_world_distance answers for the last build, for points (three floats each; world cell = floorf(p * recip) per
 * axis, the archive's rule) or world cells (three int32 each); exactly one of the two pointers is non-NULL, also with
 * n == 0.  `cell` is as sdm_world_reach_result.cell: (0, 0, 0) for a point that is non-finite or beyond the brick range, a
 * cell given is echoed as given.  A cell in no brick of the field, a non-finite point or one out of range: d2 0xffffffff,
 * distance -1, nearest = cell.  A field cell beyond the radius: d2 SDM_WORLD_ESDF_FAR, nearest = cell, distance =
 * sqrtf((float)(R * R + 1)) * voxel_size, a LOWER BOUND.  Otherwise d2, nearest = cell + offset, distance =
 * sqrtf((float)d2) * voxel_size - float32, one IEEE operation at a time, no contraction.  SDM_QUERY_ON_DEVICE as for the
 * other queries (device pointers, enqueued, no wait; out 8-byte aligned), host mode through the queries' staging area.
 * Memory, allocated at the first build, grown by a build that needs more, freed by sdm_destroy:
 *   SDM_WORLD_ESDF_BYTES_PER_ARCHIVED_BRICK x (archived bricks + 1, in steps of 256)
 * + SDM_WORLD_ESDF_BYTES_PER_BRICK x (bricks of the field, in steps of 256) + 2056 (the counters and their landing area).
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or output (n_out, out), unknown flag bits, radius 0 or > 16,
 * negative counts, first or cap, none or both of xyz and cells, a Z-slab shard (shard_count > 1), a build before the
 * archive has had an update or import, and the getter or the query before any build. */
#define SDM_WORLD_ESDF_UNKNOWN_IS_OBSTACLE 0x1u  /* occ == -1 and every cell of a brick the archive does not have */
#define SDM_WORLD_ESDF_STATIC_ONLY         0x2u  /* occupied cells on movable tracks are no obstacles */
#define SDM_WORLD_ESDF_BOX                 0x4u  /* the field is the bricks inside bmin .. bmax (inclusive brick box) */
#define SDM_WORLD_ESDF_MAX_RADIUS 16
#define SDM_WORLD_ESDF_NONE 0xffffu              /* in the getter's d2: no obstacle within the radius */
#define SDM_WORLD_ESDF_FAR  0xfffffffeu          /* in a query's d2: a field cell with no obstacle within the radius */
#define SDM_WORLD_ESDF_BYTES_PER_ARCHIVED_BRICK 72  /* box flag, rank, the eight obstacle words */
#define SDM_WORLD_ESDF_BYTES_PER_BRICK 2080      /* 512 packed field words, coordinates, two hash slots */
typedef struct {            /* 32 bytes, every field naturally aligned */
  uint32_t flags;
  uint32_t radius;          /* 1 .. SDM_WORLD_ESDF_MAX_RADIUS cells */
  int32_t  bmin[3], bmax[3];/* inclusive brick box, read only with SDM_WORLD_ESDF_BOX */
} sdm_world_esdf_options;
typedef struct {            /* 32 bytes, every field naturally aligned */
  uint32_t n_bricks;        /* bricks of the field */
  uint32_t flags, radius;   /* as given */
  uint32_t stamp;           /* the archive's stamp at the build: sdm_world_info.stamp */
  int64_t  n_obstacle_cells;/* field cells that are obstacles (d2 == 0) */
  int64_t  n_near_cells;    /* field cells with d2 <= radius^2, the obstacle cells included */
} sdm_world_esdf_info;
typedef struct {            /* 32 bytes */
  int32_t  cell[3];         /* the world cell asked about */
  int32_t  nearest[3];      /* world cell of the nearest obstacle; = cell where there is none within reach */
  uint32_t d2;              /* squared distance in cells; SDM_WORLD_ESDF_FAR; 0xffffffff: in no brick of the field */
  float    distance;        /* metres; the lower bound for FAR; -1 in no brick of the field */
} sdm_world_distance_result;
sdm_status sdm_world_esdf_update(sdm_map *m, const sdm_world_esdf_options *o);
sdm_status sdm_get_world_esdf(sdm_map *m, int16_t *coords, uint16_t *d2, int8_t *offset, int64_t first, int64_t cap,
                              int64_t *n_out, sdm_world_esdf_info *info);
sdm_status sdm_query_world_distance(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n,
                                    sdm_world_distance_result *out, uint32_t flags);

/* ---- world ground layer: is there floor under that remembered place, a kerb on the way, room for the robot's body? ----
 * sdm_world_ground_update builds, on the map's stream, the ground layer of the block (sdm_ground_update) over the bricks of
 * the world archive: a height map, a costmap and the truncated squared distance to the nearest lethal column, in tiles of
 * 8 x 8 columns.  IT WAITS ONCE, for the number of tiles, which sizes the buffers; the rest is enqueued and the getter waits
 * for it.  Cells are world cells (int32 per axis, brick = cell >> 3); everything is integer and bitwise reproducible.
 * Up axis and heights: up_axis a in {0, 1, 2}, up_sign +1 or -1 as in sdm_ground_options.  The height of a world cell with
 * coordinate g on axis a is h = g for sign +1 and h = -1 - g for sign -1, so height brick h >> 3 is brick g >> 3 or
 * -1 - (g >> 3): bricks stay aligned.  The other two axes in ascending order are u and v; a column is (i_u, j_v).
 * Band: h_lo <= h_hi, signed world heights, h_hi - h_lo <= SDM_WORLD_GROUND_MAX_SPAN - 1; clearance 0 .. 255, max_step
 * 0 .. 65535.  The READ WINDOW is h_lo .. h_hi + clearance: no cell above or below it is read, whatever it holds.
 * Tiles: a tile is the 8 x 8 columns over one (bu, bv) = (i_u >> 3, j_v >> 3).  A tile exists iff, at the time of the build,
 * the archive holds at least one brick over (bu, bv) whose heights meet the read window - and, with SDM_WORLD_GROUND_BOX,
 * tmin[0] <= bu <= tmax[0] and tmin[1] <= bv <= tmax[1] (tmax < tmin: no tile, which is no error).  Tiles are ranked
 * ascending in (bv, bu), signed; a column's word inside its tile is cu | cv << 3.
 * Cell classes, from an archived word (track, label, occ), exactly the block's:
 *   solid     occ >= 1; with SDM_WORLD_GROUND_IGNORE_MOVABLE an occ >= 1 cell whose track is movable (1 <= track <=
 *             max_movable_track) is not solid and is passable instead.
 *   passable  occ == 0; with SDM_WORLD_GROUND_UNKNOWN_PASSABLE also occ == -1.
 *   support at h: the cell is solid, its track is not movable, bit `label` of support_labels is set (bit l of word l / 32),
 *             and the cells h + 1 .. h + clearance are all passable (they lie inside the read window).
 *   A cell of a brick the archive does not have, or of a brick beyond the int16 range, reads unknown (occ == -1).
 * Per column (sdm_ground_cell; level and top are heights RELATIVE TO h_lo, 0xffff = none): level = the highest support in
 * [h_lo, h_hi]; top = the highest solid cell in the band; label = the level cell's label, 0 if none; headroom = the
 * consecutive passable cells directly above the level INSIDE THE READ WINDOW, saturating at 255, 0 if no level - so it is
 * >= clearance wherever there is a level, and a cell above h_hi + clearance never ends it; n_unknown = the unknown cells in
 * the band, absent bricks included, saturating at 255.
 * Class byte cls = class | step << 2 | lethal << 3, as the block's.  class: 1 ground (a level), 2 obstacle (no level, a top),
 * 0 none.  step: the column P has a level and a 4-neighbour column Q of some tile of the layer has one with
 * level(P) > level(Q) + max_step; only the higher side is marked; Q may lie across a tile's side; a neighbour in no tile
 * gives no relation.  lethal: class 2, or step, or with SDM_WORLD_GROUND_NONE_IS_LETHAL class 0.
 * Distance: radius R in 1 .. SDM_WORLD_GROUND_MAX_RADIUS.  Per column, d2 = the squared distance in columns to the nearest
 * lethal column of any tile of the layer, stored exactly if d2 <= R^2 and as SDM_WORLD_GROUND_NONE otherwise.  With
 * SDM_WORLD_GROUND_ABSENT_IS_LETHAL every column of no tile is lethal too: the archive's edge, for a cautious planner.  A box
 * cuts the layer - columns outside it are columns of no tile, for the step as for the distance -, so a caller who wants the
 * distance exact at the box's side GROWS THE BOX BY TWO TILES (R <= 16 columns) and ignores the rim.  No offset is stored.
 * The build is a SNAPSHOT: it owns the tiles' coordinates, a hash table of its own from tile to rank, the cells and the
 * distances, holds no pool slot, and answers the same bytes after any later sdm_world_update, sdm_world_import,
 * sdm_world_retain or sdm_world_clear, until the next sdm_world_ground_update.  Nothing of the archive or of the map's state
 * is modified; the sort and the scan run on the layers' shared scratch.
 * sdm_get_world_ground waits: per tile of rows first .. first + cap - 1 coords takes two int16 (bu, bv), cells 64
 * sdm_ground_cell and d2 64 uint16, both in column-word order; each array and info may be NULL; *n_out = the tiles of the
 * layer.  info: the counts are columns of tiles; level_min / level_max are relative, over the ground columns, 0xffff if
 * there is none; stamp is the archive's at the build (sdm_world_info.stamp); the options are the build's.
 * sdm_query_world_ground answers for the last build, for points (three floats each; world cell = floorf(p * recip) per axis,
 * the archive's rule) or world cells (three int32 each); exactly one of the two pointers is non-NULL, also with n == 0.
 * An entry that is non-finite or beyond the brick range: col (0, 0), d2 0xffffffff, surface 0, above INT32_MIN, cell
 * {0xffff, 0xffff, 0, 0, 0, 0}, dist -1, status 3.  A column of no tile: the same with col = the column.  In a tile:
 * status 0, the column's cell; d2 as stored, or SDM_WORLD_GROUND_FAR beyond R; dist = sqrtf((float)d2) * voxel_size, and for
 * FAR sqrtf((float)(R * R + 1)) * voxel_size, a LOWER BOUND; with a level, above = h(entry) - (h_lo + level) and surface =
 * (float)k * voxel_size, k the world coordinate of the level cell's upper face: g + 1 for sign +1, g for sign -1 (the
 * world's origin is the archive's).  Float32, one IEEE operation at a time, no contraction.
 * sdm_query_world_footprints takes the block's sdm_footprint - centre in global metres along u and v, heading (dir_u, dir_v)
 * a unit vector the caller supplies, half length and half width - and the block's rule: world column (i, j) is covered when
 *   pu = ((float)i + 0.5f) * voxel_size, pv likewise; du = pu - center_u, dv = pv - center_v;
 *   |du * dir_u + dv * dir_v| <= half_len  and  |dv * dir_u - du * dir_v| <= half_wid      (float32, no contraction).
 * The answer is as if every column of the plane - the columns of the brick range, -262144 .. 262143 per axis - were tested.
 * A non-finite field, half_len + half_wid > 64 * voxel_size (float32), or a heading with dir_u^2 + dir_v^2 < 0.5 (float32:
 * the plane has no sides that would bound what such a rule covers) gives the answer of a footprint that covers nothing:
 * the counts 0, level_min = level_max = 0xffff, min_d2 0xffffffff, first_lethal (0, 0).
 * Both queries take SDM_QUERY_ON_DEVICE as the other queries do (device pointers, enqueued, no wait; out 8-byte aligned,
 * inputs 4-byte aligned); host mode goes through the queries' staging area.
 * Memory, allocated at the first build, grown by a build that needs more, freed by sdm_destroy:
 *   SDM_WORLD_GROUND_BYTES_PER_ARCHIVED_BRICK x (archived bricks + 1, in steps of 256; the table's slots a power of two)
 * + SDM_WORLD_GROUND_BYTES_PER_TILE x (tiles, in steps of 256) + 8200 (the counters and their landing area).
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or output (n_out, out), unknown flag bits, up_axis not in 0..2,
 * up_sign not +1 / -1, h_lo > h_hi or a span above SDM_WORLD_GROUND_MAX_SPAN, clearance > 255, max_step > 65535, radius 0 or
 * > 16, negative counts, first or cap, none or both of xyz and cells, a NULL input of a query, a Z-slab shard
 * (shard_count > 1), a build before the archive has had an update or import, and the getter or a query before any build. */
#define SDM_WORLD_GROUND_UNKNOWN_PASSABLE 0x1u   /* occ == -1 cells, absent bricks included, are passable */
#define SDM_WORLD_GROUND_IGNORE_MOVABLE   0x2u   /* occ >= 1 cells of a movable track are passable, not solid */
#define SDM_WORLD_GROUND_NONE_IS_LETHAL   0x4u   /* columns of class 0 are lethal */
#define SDM_WORLD_GROUND_ABSENT_IS_LETHAL 0x8u   /* for the distance, every column of no tile is lethal */
#define SDM_WORLD_GROUND_BOX              0x10u  /* the layer is the tiles inside tmin .. tmax (inclusive tile box) */
#define SDM_WORLD_GROUND_MAX_SPAN 4096           /* cells of the band, h_hi - h_lo + 1, at most */
#define SDM_WORLD_GROUND_MAX_RADIUS 16
#define SDM_WORLD_GROUND_NONE 0xffffu            /* in the getter's d2: no lethal column within the radius */
#define SDM_WORLD_GROUND_FAR  0xfffffffeu        /* in a query's d2: a column of a tile with no lethal column within the radius */
#define SDM_WORLD_GROUND_BYTES_PER_ARCHIVED_BRICK 32  /* claim flag, rank, two hash slots */
#define SDM_WORLD_GROUND_BYTES_PER_TILE 668      /* 64 cells, 64 d2, the lethal word, the key, the sort's four words */
typedef struct {              /* 80 bytes, every field naturally aligned */
  uint32_t flags;
  int32_t  up_axis, up_sign;
  int32_t  h_lo, h_hi;        /* the band, world heights in cells */
  uint32_t clearance;         /* 0..255 cells */
  uint32_t max_step;          /* 0..65535 cells */
  uint32_t radius;            /* 1 .. SDM_WORLD_GROUND_MAX_RADIUS columns */
  int32_t  tmin[2], tmax[2];  /* inclusive tile box (bu, bv), read only with SDM_WORLD_GROUND_BOX */
  uint32_t support_labels[8]; /* bit l of the 256: label l may carry the robot */
} sdm_world_ground_options;
typedef struct {              /* 136 bytes, every field naturally aligned */
  uint32_t n_tiles;
  uint32_t level_min, level_max;  /* relative to h_lo, over the ground columns; 0xffff if there is none */
  uint32_t stamp;             /* the archive's stamp at the build: sdm_world_info.stamp */
  int64_t  n_ground, n_obstacle, n_none, n_step, n_lethal; /* columns of tiles */
  sdm_world_ground_options options;                        /* the build's, echoed */
} sdm_world_ground_info;
typedef struct {              /* 40 bytes */
  int32_t  col[2];            /* the entry's column (i_u, j_v); (0, 0) if non-finite or beyond the brick range */
  uint32_t d2;                /* squared distance in columns; SDM_WORLD_GROUND_FAR; 0xffffffff: in no tile */
  float    surface;           /* world coordinate along the up axis of the level cell's upper face; 0 where there is no level */
  int32_t  above;             /* h(entry) - (h_lo + level); INT32_MIN where there is no level */
  sdm_ground_cell cell;
  float    dist;              /* metres; the lower bound for FAR; -1 in no tile */
  uint32_t status;            /* 0 in a tile, 3 otherwise */
  uint32_t pad;               /* 0 */
} sdm_world_ground_result;
typedef struct {              /* 40 bytes */
  uint32_t n_cols, n_lethal, n_none, n_ground; /* covered columns of tiles: all, lethal, of class 0, of class 1 */
  uint32_t n_absent;          /* covered columns of no tile, in none of the other counts */
  uint16_t level_min, level_max;               /* relative, over the covered ground columns; 0xffff if none */
  uint32_t min_d2;            /* over the covered columns of tiles, FAR as SDM_WORLD_GROUND_FAR; 0xffffffff if n_cols == 0 */
  int32_t  first_lethal[2];   /* (i_u, j_v) of the smallest covered lethal column in (v, u) order; (0, 0) with n_lethal == 0 */
  uint32_t pad;               /* 0 */
} sdm_world_footprint_result;
sdm_status sdm_world_ground_update(sdm_map *m, const sdm_world_ground_options *o);
sdm_status sdm_get_world_ground(sdm_map *m, int16_t *coords, sdm_ground_cell *cells, uint16_t *d2, int64_t first, int64_t cap,
                                int64_t *n_out, sdm_world_ground_info *info);
sdm_status sdm_query_world_ground(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n,
                                  sdm_world_ground_result *out, uint32_t flags);
sdm_status sdm_query_world_footprints(sdm_map *m, const sdm_footprint *fp, int64_t n,
                                      sdm_world_footprint_result *out, uint32_t flags);

/* ---- world ground reach: how does a robot on wheels get from here to that remembered place, and how far is it? ----
 * sdm_world_ground_reach_update builds, on the map's stream, a 2-D travel-cost field over the costmap of the world ground
 * layer: the cheapest way ON THE GROUND from a set of start columns to every traversable column.  Like
 * sdm_world_reach_update IT WAITS: the host decides when the relaxation is at rest, and no kernel ever waits for another
 * workgroup.  Everything is integer and bitwise reproducible except `metres`.
 * Source: the field is built from the last sdm_world_ground_update of the same map; columns, tiles, up axis, h_lo and R are
 * that build's.  The tiles of the field are the ground layer's; with SDM_WORLD_GROUND_REACH_BOX only those with
 * tmin[0] <= bu <= tmax[0] and tmin[1] <= bv <= tmax[1] (tmax < tmin: a field of no tiles, which is no error).  Tiles are
 * ranked ascending in (bv, bu), the ground layer's order: without a box row r of sdm_get_world_ground_reach belongs to row
 * r of sdm_get_world_ground.
 * The build is a SNAPSHOT: it owns its copy of the tiles' coordinates, a hash table of its own from tile to rank, the eight
 * neighbour ranks per tile, the masks, the levels and the costs, and answers the same bytes after any later
 * sdm_world_ground_update, sdm_world_update, sdm_world_import, sdm_world_retain or sdm_world_clear, until the next
 * sdm_world_ground_reach_update.  Nothing of the ground layer, the archive or the map's state is modified; the scan runs on
 * the layers' shared scratch.
 * Traversable: a column is traversable iff it lies in a tile of the field, its class is 1 (it has a level), its lethal bit
 * is clear, and its stored d2 is SDM_WORLD_GROUND_NONE or >= min_d2.  min_d2 and soft_d2 range over 0 .. R^2 + 1 (beyond
 * that the truncated distance cannot answer); min_d2 = R^2 + 1 means "only columns with nothing lethal within R".  A column
 * of no tile of the field is never traversable: that bounds the search.
 * Penalty: pen(Q) = penalty (0 .. 65535) if Q's stored d2 is not SDM_WORLD_GROUND_NONE and < soft_d2, otherwise 0.
 * Moves: the eight offsets (du, dv) numbered (dv + 1) * 3 + (du + 1), 4 is "no move"; four with
 * SDM_WORLD_GROUND_REACH_FACE_CONNECTED.  The tile across a side or a corner is the one the table finds; a neighbour tile
 * whose coordinate would leave the int16 range is absent.  A move P -> P + o is allowed iff all 2 or 4 columns P + s,
 * s_a in {0, o_a}, are traversable columns of the field (no squeezing through a diagonal) and the largest minus the smallest
 * of their levels is <= max_climb (0 .. 65535 cells).  The rule is symmetric.
 * Cost: weights 10 for a straight move, 14 for a diagonal one; cost(start) = 0; cost(Q) = the minimum over the allowed moves
 * P -> Q of cost(P) + w + pen(Q).  The effective budget is max_cost if that is non-zero and 0xfffffffe otherwise; a column
 * whose true cost exceeds it reads 0xffffffff, additions saturate, and the truncated field is still exact because every
 * prefix of a cheapest path lies within the budget.
 * Descent: from column c, the smallest allowed move number o with cost(c + o) + w(o) + pen(c) == cost(c).
 * Starts and goals: points (three floats each; world cell = floorf(p * recip) per axis, the archive's rule) or world cells
 * (three int32 each), as for sdm_query_world_ground; exactly one of the two pointers is non-NULL, also with a count of 0.
 * Only the column counts: the VALUE of the coordinate along the up axis is ignored, so first_cell of a world frontier
 * cluster goes in as it is (an entry with any of its three coordinates non-finite or beyond the brick range is not usable,
 * the rule of sdm_query_world_ground).  A start that is not traversable, in no tile of the field, non-finite or out of range
 * is ignored; duplicates are fine; no usable start is no error: every column then reads unreachable.
 * sdm_get_world_ground_reach waits: per tile of rows first .. first + cap - 1 coords takes two int16 (bu, bv) and cost 64
 * words in column-word order (cu | cv << 3; 0xffffffff: unreachable or not traversable); *n_out = the tiles of the field;
 * coords, cost and info may each be NULL.
 * sdm_query_world_ground_reach / sdm_world_ground_reach_paths answer for the last build; SDM_QUERY_ON_DEVICE as for the
 * other queries (device pointers, enqueued, no wait; out 8-byte aligned), host mode through the queries' staging area.  A
 * result's level is the column's as the ground build stored it (0xffff: none, or status 3).  Row g of cells_out (n rows of
 * max_len * 3 int32) takes WORLD CELLS (x, y, z) of goal g's path from the goal to a start, both included: on the two plane
 * axes the column, on the up axis the cell the robot's base stands in, height h = h_lo + level + 1, which is coordinate
 * g = h for up_sign +1 and g = -1 - h for up_sign -1 - so a path feeds sdm_query_world_segments, sdm_query_world_distance
 * and sdm_query_world_ground as it is.  len_out[g] is its true length, 0 where there is none, and may exceed max_len: only
 * the first min(len, max_len) cells are written, the rest of the row is left untouched, in host mode too.
 * Memory: SDM_WORLD_GROUND_REACH_BYTES_PER_TILE x (tiles of the field, in steps of 256; the table's slots a power of two)
 * and a bit of activity per tile, + 64 (the counters and their landing area).  Allocated at the first build, grown by a
 * build of more tiles, freed by sdm_destroy.  A build also holds 8 B per tile of the ground layer (flags, ranks) until it
 * returns.
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options or output (n_out, out, len_out; cells_out with max_len > 0),
 * none or both start / goal pointers, unknown flag bits, a non-zero pad, penalty or max_climb > 65535, min_d2 or soft_d2
 * > R^2 + 1, negative counts, first, cap or max_len, a Z-slab shard (shard_count > 1), a build before any
 * sdm_world_ground_update, and the getter or a query before any build.  SDM_ERR_NOT_CONVERGED if the relaxation has not come
 * to rest after 64 x n_tiles + 8 rounds: a defect, never a result. */
#define SDM_WORLD_GROUND_REACH_FACE_CONNECTED 0x1u  /* the four straight moves only */
#define SDM_WORLD_GROUND_REACH_BOX            0x2u  /* the field is the ground layer's tiles inside tmin .. tmax */
#define SDM_WORLD_GROUND_REACH_BYTES_PER_TILE 464   /* 64 costs, the traversable and the penalty word, 64 levels, eight
                                                       neighbour ranks, the key, two hash slots, the list word */
typedef struct {              /* 48 bytes, every field naturally aligned */
  uint32_t flags;
  uint32_t min_d2;            /* 0 .. R^2 + 1: a column whose stored d2 is below it is not traversable */
  uint32_t soft_d2;           /* 0 .. R^2 + 1: a column whose stored d2 is below it costs `penalty` more to enter */
  uint32_t penalty;           /* 0 .. 65535 */
  uint32_t max_climb;         /* 0 .. 65535 cells */
  uint32_t max_cost;          /* 0: no budget */
  int32_t  tmin[2], tmax[2];  /* inclusive tile box (bu, bv), read only with SDM_WORLD_GROUND_REACH_BOX */
  uint32_t pad[2];            /* 0 */
} sdm_world_ground_reach_options;
typedef struct {              /* 80 bytes: options at offset 32 */
  uint32_t n_tiles;           /* tiles in the field */
  uint32_t n_starts_used;     /* distinct start columns that were traversable */
  uint32_t n_traversable, n_reached, max_cost_reached;
  uint32_t rounds;            /* relaxation rounds the build took (diagnostic; not part of the bitwise contract) */
  uint32_t stamp;             /* the archive's stamp the ground build carried: sdm_world_ground_info.stamp */
  uint32_t pad;               /* 0 */
  sdm_world_ground_reach_options options;  /* the build's, echoed */
} sdm_world_ground_reach_info;
typedef struct {              /* 24 bytes: col at 8, level at 16, next at 18, status at 19, pad at 20 */
  uint32_t cost;              /* 0xffffffff: no path */
  float    metres;            /* (float)cost * (voxel_size * 0.1f), float32, no contraction; -1 where no path */
  int32_t  col[2];            /* the entry's column (i_u, j_v); (0, 0) if non-finite or beyond the brick range */
  uint16_t level;             /* relative to the ground build's h_lo; 0xffff if none */
  uint8_t  next;              /* move number of the first descent step; 4 at a start; 255 where no path */
  uint8_t  status;            /* 0 reached, 1 traversable but unreached (or beyond the budget), 2 a column of a tile of the
                                 field but not traversable, 3 in no tile of the field / non-finite / out of range */
  uint32_t pad;               /* 0 */
} sdm_world_ground_reach_result;
sdm_status sdm_world_ground_reach_update(sdm_map *m, const sdm_world_ground_reach_options *o, const float *start_xyz,
                                         const int32_t *start_cells, int64_t n_starts);
sdm_status sdm_get_world_ground_reach(sdm_map *m, int16_t *coords, uint32_t *cost, int64_t first, int64_t cap, int64_t *n_out,
                                      sdm_world_ground_reach_info *info);
sdm_status sdm_query_world_ground_reach(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n,
                                        sdm_world_ground_reach_result *out, uint32_t flags);
sdm_status sdm_world_ground_reach_paths(sdm_map *m, const float *xyz, const int32_t *cells, int64_t n, int32_t max_len,
                                        int32_t *cells_out, int32_t *len_out, uint32_t flags);

/* ---- world rays: is this straight leg free, and what would a camera at that remembered place see? ----
 * sdm_query_world_segments and sdm_query_world_views are the archive's counterparts of sdm_query_segments and
 * sdm_query_views: the same walks, through the bricks of the world archive instead of the block.  Both read the archive
 * LIVE, in stream order on the map's stream: they see it as the last sdm_world_update, sdm_world_import, sdm_world_retain
 * or sdm_world_clear enqueued before them left it, take no snapshot, and write only the caller's outputs and - the views - a
 * pool of bitmasks of their own.  Positions are in the global frame.  World-index coordinate of a position p: u = p * recip
 * per axis, the archive's own float32 rule; world cell floor(u); brick = cell >> 3; a brick beyond the int16 range is absent
 * and never looked up.  Everything but t is an integer: the answers are bitwise reproducible.
 * Cell classes: occupied - the archived word has occ >= 1; free - occ == 0; unknown - occ == -1 OR THE CELL LIES IN A BRICK
 * THE ARCHIVE DOES NOT HAVE.  With SDM_WORLD_RAYS_IGNORE_MOVABLE an occupied cell on a movable track (1 <= track <=
 * max_movable_track) counts as free - the rule of SDM_WORLD_REACH_IGNORE_MOVABLE.
 *
 * Segments a -> b (ab[6i..6i+5] = ax ay az bx by bz) are traversed in ascending t, u(t) = u(a) + t (u(b) - u(a)), t in
 * [0, 1], as sdm_query_segments traverses them: a 3-D DDA in double, every crossing parameter computed fresh from the end
 * points as (plane - u_a) * (1 / (u_b - u_a)), a plane crossed while its t <= 1, x before y before z at equal t; a
 * zero-length segment is the cell of a.  The lattice is the unbounded lattice of world cells: nothing is clipped.  Occupied
 * cells block; with SDM_QUERY_UNKNOWN_BLOCKS unknown cells block too, those of absent bricks included.
 * Two rules keep the cost finite.  INVALID: an end point with a non-finite u, or whose cell lies in a brick beyond the int16
 * range (floor(u) outside [-262144, 262144)): no hit, cells = 0, unknown = 0; with SDM_QUERY_UNKNOWN_BLOCKS a hit at t = 0
 * with occ -1, cell (0, 0, 0), cells = 0.  TOO LONG: a valid segment with 1 + sum over the axes of |floor(u_b) - floor(u_a)|
 * > SDM_WORLD_SEGMENT_MAX_CELLS (8192: 819 m at 0.1 m voxels, a second of a lane's time): t = -1, cells = -1, nothing is
 * walked, under any flag.  (The walk itself may visit one cell more per axis: a plane at exactly t = 1, approached from
 * above, is still crossed - as in sdm_query_segments.)
 *
 * Views: sdm_view, sdm_view_gain and the ray table are sdm_query_views': ray r of view v is the segment from a = pos to
 * b = pos + range * (R(q) d_r) in the float32 order given there; range <= 0 is the zero-length segment.  Where the block
 * query is bounded by the block, this one is bounded by a window the caller states: with c0 the cell of pos, the world cells
 * with |c_i - c0_i| <= reach_cells per axis, 1 <= reach_cells <= SDM_WORLD_VIEW_MAX_REACH - a host integer, so that device
 * mode never reads a view to size anything.  A ray is walked as a world segment without SDM_QUERY_UNKNOWN_BLOCKS and ends at
 * its blocking cell, at b, or where its next step would leave the window (at most 3 reach_cells + 1 cells: the 8192 rule
 * does not apply).  The blocking cell counts towards n_occupied, every cell before it towards n_unknown or n_free by its
 * class - cells of absent bricks are unknown: they are the gain -, each cell ONCE per view however many rays visit it;
 * rays_hit counts the rays that end in a blocking cell, rays_in_map those walked (>= 1 cell), ray_cells and ray_unknown are
 * the sums over the rays.  A view is invalid - an all-zero gain, rays with t = -1 and cells = 0 - when pos, q or range is
 * non-finite or the window reaches beyond the int16 brick range; a non-finite d_r or u(b) does that for its ray only.
 * rays_out (may be NULL) holds one sdm_world_segment_hit per (view, ray) at [v * n_rays + r]: bit for bit what
 * sdm_query_world_segments returns for (a, b) under the same SDM_WORLD_RAYS_IGNORE_MOVABLE whenever every cell of that
 * segment lies in the window and the segment is not too long; otherwise the clipped walk's.
 * Memory: one bit per window cell and view in flight, S^3 bits with S = 2 reach_cells + 1 (bit ((z - z0) S + (y - y0)) S +
 * (x - x0)), in a pool of this layer's own of at most 64 MiB, grown on demand (a call that grows it waits for the stream
 * once), freed by sdm_destroy and all zero whenever a call's work has completed (each batch's masks are zeroed by a memset
 * behind it).  min(256, 64 MiB / mask bytes) views are in flight, at least 3 (the mask of reach 255 takes 16.7 MB); a call
 * with more views works in batches.  Host mode is staged in chunks of whole views, like sdm_query_views.
 * SDM_QUERY_ON_DEVICE as for the other queries (device pointers, enqueued, no wait; outputs 8-byte aligned).
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, input or out, n < 0, unknown flag bits (the views refuse
 * SDM_QUERY_UNKNOWN_BLOCKS), a NULL ray table, n_rays < 1 or > SDM_VIEW_MAX_RAYS, n_views * n_rays >= 2^31, reach_cells out of
 * range, a Z-slab shard (shard_count > 1), and a call before any sdm_world_update / sdm_world_import or after
 * sdm_world_clear.  n == 0 launches nothing. */
#define SDM_WORLD_RAYS_IGNORE_MOVABLE 0x10u   /* occupied cells on movable tracks count as free */
#define SDM_WORLD_SEGMENT_MAX_CELLS 8192      /* a segment of more world cells is "too long" and not walked */
#define SDM_WORLD_VIEW_MAX_REACH 255          /* the largest reach_cells: a window of 511^3 cells */
typedef struct {          /* 32 bytes */
  float    t;             /* as sdm_segment_hit.t; -1: nothing blocks */
  int32_t  cells;         /* world cells visited up to and including the hit; 0: invalid; -1: too long */
  int32_t  cell[3];       /* world cell of the hit; (0, 0, 0) without one */
  uint16_t track; uint8_t label; int8_t occ;  /* the hit cell's word; 0 / 0 / -1 without a hit or for an absent brick */
  int32_t  unknown;       /* visited cells that are unknown, the hit included if it is one */
  uint32_t stamp;         /* last_stamp of the hit cell's brick; 0 without one */
} sdm_world_segment_hit;
sdm_status sdm_query_world_segments(sdm_map *m, const float *ab, int64_t n, sdm_world_segment_hit *out, uint32_t flags);
sdm_status sdm_query_world_views(sdm_map *m, const sdm_view *views, int64_t n_views, const float *dirs, int32_t n_rays,
                                 int32_t reach_cells, sdm_view_gain *out, sdm_world_segment_hit *rays_out, uint32_t flags);

/* ---- world mesh: what does everything the map remembers look like - to a person, a simulator, a renderer? ----
 * sdm_world_mesh_update builds, on the map's stream, the face mesh of sdm_mesh_update over the bricks of the world archive
 * instead of the map block: one unit quad per face between a solid cell and a neighbour that is not solid, and the world
 * lattice corners those faces use as welded vertices.  IT WAITS THREE TIMES: for the archive's counters, for the number of
 * bricks of the field, and for the numbers of faces, vertex bricks and vertices together, and sizes its buffers from them;
 * the lists themselves are enqueued and the getters wait for them.  Cells are world cells (int32 per axis, brick =
 * cell >> 3), the archive's origin is the world's.  Everything is integer and bitwise reproducible.  The archive is what
 * the layer reads: a mesh that mixes the live block and the archive does not exist - call sdm_world_update first.
 * Field: the archived bricks at the time of the build; with SDM_WORLD_MESH_BOX those inside the inclusive brick box
 * bmin .. bmax (bmax < bmin on an axis: no brick, which is no error).  Bricks are ranked in brick order - ascending in
 * (bz, by, bx), signed: without a box rank r is row r of sdm_get_world_bricks taken at the same moment, as in
 * sdm_get_world_esdf.
 * Solid cell: a cell of a field brick whose archived word (track, label, occ) has occ >= 1 (occ == 1 with
 * SDM_WORLD_MESH_OBSERVED_ONLY), bit `label` of `labels` set (bit l of word l / 32), track == options.track unless that
 * is -1, and a track the static / movable flag admits (movable: 1 <= track <= max_movable_track) - sdm_mesh_update's rule.
 * Face: a solid cell of the field and a direction whose face neighbour is not solid by the same rule.  The neighbour's word
 * is read from the WHOLE ARCHIVE, not from the field, so the meshes of disjoint boxes tile: no face stands between two
 * solid cells on either side of a box wall.  kind: what is behind the face - 0 a free cell (occ == 0), 1 a cell with
 * occ == -1 in an archived brick, 2 a cell in no archived brick (a brick beyond the int16 range is absent), 3 a cell with
 * occ >= 1 that is not solid under these options.  SDM_WORLD_MESH_SKIP_UNKNOWN_FACES and SDM_WORLD_MESH_SKIP_ABSENT_FACES
 * leave kinds 1 and 2 out.  Faces ascend in (brick rank, cell word cx | cy << 3 | cz << 6, dir).
 * dir, the corners q0..q3 of a face as offsets from its cell, the winding and the triangles are sdm_mesh_update's table:
 * (q1 - q0) x (q3 - q0) is the outward unit normal and q0 is the quad's smallest corner in (z, y, x).
 * Vertices: the world lattice corners used by at least one emitted face, each once, welded across brick seams.  Corner
 * (gx, gy, gz), an int32 triple, is the min corner of world cell (gx, gy, gz).  Its owner brick is corner >> 3 per axis, its
 * local word (gx & 7) | (gy & 7) << 3 | (gz & 7) << 6; the list ascends in (owner brick in brick order, local word).  The
 * owner brick need be neither in the field nor in the archive - the +x face of a cell with cx == 7 uses corners of brick
 * bx + 1 - and may be 32768 on an axis.  quads[4f .. 4f+3] index the vertex list.
 * xyz[3v + a] = (float)corner_a * voxel_size, one float32 multiply: the archive's rule for a cell's min corner.
 * The build is a SNAPSHOT: the getters return the same bytes after any later sdm_world_update, sdm_world_import,
 * sdm_world_retain or sdm_world_clear, until the next sdm_world_mesh_update.  It holds lists, no pool slot, once it returns.
 * Nothing of the archive or of the map's state is modified.
 * max_faces / max_vertices > 0 cap the two lists: with more faces or more vertices than that the build writes no list and
 * returns SDM_ERR_CAPACITY; sdm_get_world_mesh_info then still gives the true counts (faces_by_dir and faces_by_kind
 * included: they count the faces of the build, listed or not), the two list getters still set *n_out to the true count,
 * and they and sdm_world_mesh_device return SDM_ERR_CAPACITY until a build with room.  0: no cap.
 * sdm_get_world_mesh_faces: rows first .. first + cap - 1 of the face list into faces and quads (4 per face); *n_out = the
 * faces in all.  coords takes the field bricks' (bx, by, bz), three int16 for each of the info's n_bricks bricks - row r for
 * brick rank r, which is what sdm_world_mesh_face.brick indexes - and is written whole by a call with first == 0, whatever
 * cap is, and not at all by a call with first > 0: cap counts faces only.  sdm_get_world_mesh_vertices: rows first ..
 * first + cap - 1 of the vertex list into corners (three int32) and xyz (three floats); *n_out = the vertices in all.  Every
 * array may be NULL.  Both wait.
 * sdm_world_mesh_device: device pointers to the three lists of the last build, for a renderer: valid until the next
 * sdm_world_mesh_update or sdm_destroy, to be read in stream order on sdm_stream (the counts: sdm_get_world_mesh_info).
 * Each may be NULL.
 * Memory, allocated at the first build, grown by a build that needs more, freed by sdm_destroy:
 *   SDM_WORLD_MESH_BYTES_PER_ARCHIVED_BRICK x (archived bricks + 1, in steps of 256)
 * + (SDM_WORLD_MESH_BYTES_PER_BRICK + 5.5) x (bricks of the field, in steps of 256; 5.5: 44 bytes of counts per 8 bricks)
 * + (SDM_WORLD_MESH_BYTES_PER_VERTEX_SLOT + 1 / 16) x (the power of two >= 16 x that number: a brick's corners have at most
 *   eight owner bricks and the table of them is at most half full; 1 / 16: a count per 64 slots)
 * + SDM_WORLD_MESH_BYTES_PER_VERTEX_BRICK x (vertex bricks, in steps of 256)
 * + SDM_WORLD_MESH_BYTES_PER_FACE x (faces, in steps of 4096) + SDM_WORLD_MESH_BYTES_PER_VERTEX x (vertices, in steps of
 *   4096) + 264 (the counters and their landing area).
 * Errors: SDM_ERR_INVALID_ARGUMENT for a NULL map, options, info or n_out, unknown flag bits, both
 * SDM_WORLD_MESH_STATIC_ONLY and SDM_WORLD_MESH_MOVABLE_ONLY, track < -1 or > 65535, a negative max_faces, max_vertices,
 * first or cap, a Z-slab shard (shard_count > 1), a build before the archive has had an update or import, and a getter or
 * sdm_world_mesh_device before any build. */
#define SDM_WORLD_MESH_STATIC_ONLY         0x01u  /* a cell whose winning track is movable is not solid */
#define SDM_WORLD_MESH_MOVABLE_ONLY        0x02u  /* only such cells are solid (both bits: SDM_ERR_INVALID_ARGUMENT) */
#define SDM_WORLD_MESH_OBSERVED_ONLY       0x04u  /* occ == 2 (guessed occupied) is not solid */
#define SDM_WORLD_MESH_SKIP_UNKNOWN_FACES  0x08u  /* faces of kind 1 are left out */
#define SDM_WORLD_MESH_SKIP_ABSENT_FACES   0x10u  /* faces of kind 2 are left out: the mesh is open where the archive ends */
#define SDM_WORLD_MESH_BOX                 0x20u  /* the field is the bricks inside bmin .. bmax (inclusive brick box) */
#define SDM_WORLD_MESH_BYTES_PER_ARCHIVED_BRICK 200  /* box flag, rank, the solid, unknown and occupied words */
#define SDM_WORLD_MESH_BYTES_PER_BRICK 132   /* coordinates, pool slot, six neighbours, eight owners twice, the slices' prefix */
#define SDM_WORLD_MESH_BYTES_PER_VERTEX_SLOT 80   /* key, rank, place in the list, the 512 corner bits */
#define SDM_WORLD_MESH_BYTES_PER_VERTEX_BRICK 48  /* the sort's four words, the eight levels' prefix */
#define SDM_WORLD_MESH_BYTES_PER_FACE 28     /* 12 B record, 16 B vertex ids */
#define SDM_WORLD_MESH_BYTES_PER_VERTEX 12   /* the corner */
typedef struct {          /* 80 bytes, every field naturally aligned */
  uint32_t flags;
  int32_t  track;         /* -1: any; 0..65535: only cells whose winning track is this one */
  uint32_t labels[8];     /* bit l of the 256 (binding.label_mask): cells of label l may be solid */
  int32_t  bmin[3], bmax[3];  /* inclusive brick box, read only with SDM_WORLD_MESH_BOX */
  int64_t  max_faces;     /* 0: no cap */
  int64_t  max_vertices;  /* 0: no cap */
} sdm_world_mesh_options;
typedef struct {          /* 12 bytes */
  uint32_t brick;         /* rank of the cell's brick in the field: row of the faces getter's coords */
  uint16_t cell;          /* cx | cy << 3 | cz << 6 */
  uint8_t  dir;           /* 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z: the outward normal */
  uint8_t  kind;          /* behind the face: 0 free, 1 unknown, 2 no archived brick, 3 occ >= 1 but not solid */
  uint16_t track; uint8_t label; int8_t occ;   /* the solid cell's archived word */
} sdm_world_mesh_face;
typedef struct {          /* 200 bytes, every field naturally aligned */
  uint32_t n_bricks;        /* bricks of the field */
  uint32_t n_vertex_bricks; /* bricks that own at least one vertex */
  int64_t  n_faces, n_vertices, n_solid;       /* true counts, also when over a cap; n_solid: solid cells of the field */
  int64_t  faces_by_dir[6], faces_by_kind[4];  /* of the faces of the build */
  uint32_t stamp;           /* the archive's stamp at the build: sdm_world_info.stamp */
  uint32_t pad;             /* 0 */
  sdm_world_mesh_options options;              /* echoed as given */
} sdm_world_mesh_info;
sdm_status sdm_world_mesh_update(sdm_map *m, const sdm_world_mesh_options *o);
sdm_status sdm_get_world_mesh_info(sdm_map *m, sdm_world_mesh_info *info);
sdm_status sdm_get_world_mesh_faces(sdm_map *m, int16_t *coords, sdm_world_mesh_face *faces, uint32_t *quads,
                                    int64_t first, int64_t cap, int64_t *n_out);
sdm_status sdm_get_world_mesh_vertices(sdm_map *m, int32_t *corners, float *xyz, int64_t first, int64_t cap, int64_t *n_out);
sdm_status sdm_world_mesh_device(sdm_map *m, const sdm_world_mesh_face **faces, const uint32_t **quads, const int32_t **corners);

/* ---- owner sets of the object layer: ObjectParticleHashMap (object_layer.h:20-52) */
sdm_status sdm_object_particle_count(sdm_map *m, int32_t track_id, int64_t *count);
/* The keys of ObjectParticleHashMap::indices_map whose sets are not empty: every track id that owns at least one slot of
 * this map (this shard), ascending, at most `cap` of them; *n_out = how many there are.  What the reference's floating-object
 * check iterates over (semantic_dsp_map.h:712-736: an owner set without a tracked object is wiped): an object layer on the
 * C ABI lists these, drops the ids it tracks, and passes the rest to sdm_update as remove_tracks.  Synchronises the map's
 * stream. */
sdm_status sdm_tracks_with_particles(sdm_map *m, int32_t *out, int32_t cap, int32_t *n_out);

/* ---- introspection / checkpoint (tests, fixtures; SURVEY.md §5 checkpoint row) */
sdm_status sdm_get_stats(sdm_map *m, sdm_stats *out, int32_t count_live);
sdm_status sdm_set_profiling(sdm_map *m, int32_t on);
/* test hook: always run the generic 3-D frustum flood instead of the line-graph flood (both are exact) */
sdm_status sdm_debug_force_generic_flood(sdm_map *m, int32_t on);
sdm_status sdm_get_ring_state(sdm_map *m, sdm_ring_state *out);
sdm_status sdm_set_ring_state(sdm_map *m, const sdm_ring_state *in);
sdm_status sdm_get_stamps(sdm_map *m, uint32_t *sx, uint32_t *sy, uint32_t *sz);
sdm_status sdm_set_stamps(sdm_map *m, const uint32_t *sx, const uint32_t *sy, const uint32_t *sz);
/* SoA dump/load of every slot of this shard (V*S entries per array; NULL = skip on dump) */
sdm_status sdm_dump_state(sdm_map *m, float *px, float *py, float *pz, float *w, uint16_t *ts,
                          uint16_t *track, uint8_t *label, uint8_t *status, uint8_t *forget,
                          uint16_t *owner);
sdm_status sdm_load_state(sdm_map *m, const float *px, const float *py, const float *pz,
                          const float *w, const uint16_t *ts, const uint16_t *track,
                          const uint8_t *label, const uint8_t *status, const uint8_t *forget,
                          const uint16_t *owner);
/* diagnostics of the last update: ck+kappa image, per-pixel bin counts, extrinsic */
sdm_status sdm_get_ck_kappa(sdm_map *m, float *out);
sdm_status sdm_get_bin_counts(sdm_map *m, uint32_t *out);
sdm_status sdm_get_bins(sdm_map *m, uint32_t *out, int64_t cap, int64_t *n_out);
sdm_status sdm_get_extrinsic(sdm_map *m, float *out16);

/* ---- timing of single kernels for bench.py's roofline line: runs the occupancy sweep
 * `iters` times on the map's stream bracketed by HIP events, returns average ms per launch. */
sdm_status sdm_time_occupancy_sweep(sdm_map *m, int32_t iters, float *avg_ms);
/* bench hook: overwrite the map with the dense case of SURVEY.md 8(d) (every slot live, every voxel observed) */
sdm_status sdm_debug_fill_dense(sdm_map *m);
/* mode 0 (= sdm_debug_fill_dense): every slot draws one of eight track ids - four to five different ones per voxel, the
 * worst case for the track vote; mode 1: every voxel draws one (a voxel of a real map holds particles of one surface),
 * one voxel in 16 two */
sdm_status sdm_debug_fill_dense_ex(sdm_map *m, int32_t mode);
/* Test hook: how many groups of 512 voxels carry the non-incremental sweep's "every chunk was dense" hint right now, i.e.
 * will be skipped by its classification launch and classified by the evaluating launch itself next time
 * (tests/test_sweep_dense_gpu.py makes sure its repeated sweeps do take that path). */
sdm_status sdm_debug_hinted_groups(sdm_map *m, int64_t *n_out);
/* Test hook.  A non-incremental sweep evaluates the voxels of its sparse chunks either in its first launch or through
 * per-tile lists and a launch of their own; the library picks per sweep from what the sweep before found (speed only:
 * the results are the same).  mode 1 / 0: always / never the lists; -1: the library picks again. */
sdm_status sdm_debug_sweep_lists(sdm_map *m, int32_t mode);
/* Test hook: how the next non-incremental sweep would be issued, from what the last one reported (waits for the map's
 * stream).  Bit 0: the sparse voxels go through per-tile lists; bit 1: every group of 512 voxels was dense, the
 * classification launch is left out and the evaluation launch takes every group (one launch instead of two; the
 * environment variable SDM_SWEEP_SKIP_SCAN=0 keeps both).  Either way every voxel gets the same result. */
sdm_status sdm_debug_sweep_mode(sdm_map *m, int32_t *mode_out);
/* Test hook.  The table of older owner-set memberships (sdm_stats.alias_entries) takes 65536 entries; `cap` (1..65536)
 * makes it report its overflow earlier, so that a test can reach it on a small map.  Call before the map's first frame. */
sdm_status sdm_debug_alias_cap(sdm_map *m, int32_t cap);
/* Diagnostic (tools/probes/reach_probe.py): the tiles relaxed by the last sdm_reach_update, summed over its rounds. */
sdm_status sdm_debug_reach_tiles(sdm_map *m, int64_t *tiles_out);
/* Diagnostic (tools/probes/world_reach_probe.py): the bricks relaxed by the last sdm_world_reach_update, summed over its rounds. */
sdm_status sdm_debug_world_reach_bricks(sdm_map *m, int64_t *bricks_out);
/* Diagnostic (tools/probes/world_ground_reach_probe.py): the tiles relaxed by the last sdm_world_ground_reach_update, summed over its rounds. */
sdm_status sdm_debug_world_ground_reach_tiles(sdm_map *m, int64_t *tiles_out);
/* Test hook.  sdm_query_views keeps at most max_views_in_flight views in flight (never more than its pool has masks);
 * <= 0: the library's choice.  A test on a small map can so force a call to take several batches. */
sdm_status sdm_debug_view_batch(sdm_map *m, int32_t max_views_in_flight);
/* Test hook.  The same for sdm_query_world_views and its pool. */
sdm_status sdm_debug_world_view_batch(sdm_map *m, int32_t max_views_in_flight);

/* ---- device-side unit tests of the hand-written primitives (tests/test_primitives_gpu.py) */
sdm_status sdm_test_scan(const uint32_t *in, uint32_t *out, int64_t n);
sdm_status sdm_test_sort_pairs(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                               uint32_t *vals_out, int64_t n, int32_t nbits);
/* The same two primitives through their whole contract (csrc/sdm_internal.h): a SEQUENCE of n_calls calls issued back to
 * back on one stream, without a host synchronisation between them, on ONE scratch buffer that is sized for the longest
 * capacity of the sequence with no slack, zeroed once before the first call and followed by SDM_TEST_GUARD_WORDS words
 * of a canary.  Call i works on `capacity[i]` words, slice i of the concatenated arrays (sum of the capacities long).
 * Without SDM_TEST_COUNT_ON_DEVICE its length is count[i] (<= capacity[i]); with it the call is launched at the
 * capacity and count[i] (any value) is read on the device.  *guard_ok = every guard word survived.  scratch_out, if not
 * null, receives the scratch as the last call left it: sdm_test_scratch_elems words for the longest capacity.
 *
 * sdm_test_scan_seq: `out` is uploaded before the calls and downloaded after them, so the caller sees what the scan left
 * alone.  With SDM_TEST_IN_PLACE the scan runs with out == in on a copy of `in`, and `out` receives that buffer.
 *
 * sdm_test_sort_pairs_seq: keys_in / vals_in are uploaded as the first pair of buffers, keys_out / vals_out as the
 * second; which[i] is what radix_sort_pairs returned for call i (0 = first pair, 1 = second), and slice i of keys_out /
 * vals_out receives the whole slice of THAT pair.  Keys must be < 2^nbits[i]. */
#define SDM_TEST_IN_PLACE 1u
#define SDM_TEST_COUNT_ON_DEVICE 2u
#define SDM_TEST_GUARD_WORDS 64
sdm_status sdm_test_scratch_elems(int32_t sort, int64_t n, int64_t *elems);
sdm_status sdm_test_scan_seq(int32_t n_calls, const int64_t *capacity, const int64_t *count, uint32_t flags,
                             const uint32_t *in, uint32_t *out, int32_t *guard_ok, uint32_t *scratch_out);
sdm_status sdm_test_sort_pairs_seq(int32_t n_calls, const int64_t *capacity, const int64_t *count, const int32_t *nbits,
                                   uint32_t flags, const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                                   uint32_t *vals_out, int32_t *which, int32_t *guard_ok, uint32_t *scratch_out);

const char *sdm_last_error(void);
const char *sdm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SDM_H_ */
