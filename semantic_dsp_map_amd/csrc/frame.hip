// frame.hip — one frame of a map: its host preparation, its launches (start / moves / predict / finish), the three graph
// shapes a plain frame is replayed from, sdm_update and the raw-input path in front of it, sdm_synchronize.
#include <chrono>

#include "sdm_map.h"

#pragma clang fp contract(off)

void sdm::drop_graphs(sdm_map *m) {
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

// launches of sdm_frame_start: the frame block goes to the device, the chains that depend on nothing but it start
sdm_status frame_enqueue_start(sdm_map *m) {
  hipStream_t s = m->stream;
  const Dims &d = m->d;
  const int32_t stop_after = m->stop_after;
  const bool whole = d.v_count == d.V;  // not a Z-slab shard
  stage_mark(m, 0);
  if (m->stamps_dirty) SDM_TRY(upload_stamps(m));
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
      SDM_TRY(exchange_counts(m, m->s_moves));
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

extern "C" {

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

// the launch-by-launch frame of sdm_update (the frame block is prepared, the inputs are staged): issued directly, or
// into a capture
sdm_status issue_frame(sdm_map *m, uint32_t flags, int32_t stop_after) {
  sdm_status rc = frame_enqueue_start(m);
  if (rc == SDM_OK) rc = sdm_frame_moves(m);
  if (rc == SDM_OK) rc = sdm_frame_predict(m, nullptr);
  if (rc == SDM_OK) rc = sdm_update_finish(m, nullptr, 1, flags, stop_after);
  return rc;
}

// before a capture: the old graphs go; nothing of an earlier frame may still be running on the side streams when they join
sdm_status capture_prepare(sdm_map *m) {
  drop_graphs(m);
  HIP_TRY(hipStreamSynchronize(m->s_frustum));
  if (m->s_moves) HIP_TRY(hipStreamSynchronize(m->s_moves));
  HIP_TRY(hipStreamSynchronize(m->s_birth));
  m->sc.fa = m->d_fa[0];
  m->sc.fa_side = m->d_fa[1];
  return SDM_OK;
}

// The frame as a graph: captured from the very launches above, instantiated once, replayed with the frame block as the
// one parameter that changes.  Two shapes.  Branched: the frustum chain and the birth-candidate chain keep their side
// streams and become branches.  Chain: their launches are issued on the main stream for the capture.  hipGraphLaunch of
// a chain of 40 kernel nodes costs the host 5 us, of the branched graph 78 us (ROCm 7.2: a graph with forks and joins is
// submitted piecewise, with synchronisation between the pieces) - against 105 us for issuing the launches one by one.
sdm_status graph_capture(sdm_map *m) {
  SDM_TRY(capture_prepare(m));
  m->capturing = true;
  hipStream_t side[3] = {m->s_frustum, m->s_birth, m->s_moves};
  // (under capture the member count of the moving objects is issued on the main stream, frame_enqueue_start)
  if (m->graph_shape == GRAPH_CHAIN) m->s_frustum = m->s_birth = m->stream;
  hipError_t e = hipStreamBeginCapture(m->stream, hipStreamCaptureModeThreadLocal);
  sdm_status rc = SDM_OK;
  if (e == hipSuccess) {
    rc = issue_frame(m, m->frame_flags, 0);
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
  return SDM_OK;
}

// GRAPH_PIECES: the frame's kernels as five chain graphs.  Which kernels, in which order, on which stream and behind
// which event is exactly what frame_enqueue_start / sdm_frame_moves / sdm_frame_predict / sdm_update_finish issue for a
// plain frame (the member count of the moving objects on the main stream, as under capture); only k_frame_begin, whose
// argument is the frame block, is launched directly.  (A version that mirrors the launch-by-launch frame completely -
// member count as a sixth graph on its own stream, frustum and count chains started behind the previous frame's births -
// was measured: 0.34-0.35 instead of 0.36 ms on the GPU, but 115 instead of 60 us on the host.)
sdm_status pieces_capture(sdm_map *m) {
  SDM_TRY(capture_prepare(m));
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
  return SDM_OK;
}

}  // namespace

sdm_status sdm_set_issue_mode(sdm_map *m, int32_t mode) {
  if (!m || mode < 0 || mode > 4) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  bool use;
  int shape;
  issue_mode_for(m, mode, &use, &shape);
  if (shape != m->graph_shape) {
    // the branched graph and the chain share one executable: whatever was captured for the old shape goes
    HIP_TRY(hipStreamSynchronize(m->stream));
    drop_graphs(m);
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
      } else {
        m->cur_depth = m->fa.depth;
        m->cur_cloud = m->fa.cloud;
        m->state_event_valid = false;  // ev_state was not recorded: the next plain frame forks from its own start
        m->vis_event_valid = false;
        m->sweep_all = false;
        m->sweep_epoch = next_epoch(m->f.epoch);
        m->n_graph_frames++;
      }
    }
    if (direct) {
      m->n_direct_frames++;
      rc = issue_frame(m, flags, stop_after);
    }
  } else {
    m->n_direct_frames++;
    const auto t0 = std::chrono::steady_clock::now();
    rc = issue_frame(m, flags, stop_after);
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
    if (!on_dev && src_hw * 4 > m->src_stage_bytes) SDM_TRY(regrow(m, &m->d_src_stage, &m->src_stage_bytes, src_hw * 4, s));
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
  if (hw * n_objects > in.obj_masks_cap) SDM_TRY(regrow(m, &in.obj_masks, &in.obj_masks_cap, hw * n_objects, sc_));
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
  // (a frame without objects keeps the filter: a movable id out of the static table has the all-zero box there too)
  a.has_bbox = opt && opt->object_bbox ? 1 : 0;
  if (a.has_bbox && n_objects > 0)
    HIP_TRY(hipMemcpyAsync(in.bbox, opt->object_bbox, sizeof(double) * 6 * n_objects, hipMemcpyHostToDevice, sc_));
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

sdm_status sdm_synchronize(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  if (m->comm) {
    SDM_TRY(exchange_wait(m));
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

}  // extern "C"
