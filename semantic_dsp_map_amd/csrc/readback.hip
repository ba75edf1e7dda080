// readback.hip — what a caller reads back from a map (voxels, point lists, statistics, ring state, the whole particle
// state and its way back in) and the plain device / page-locked buffers handed to callers.
#include <cmath>

#include "sdm_map.h"

extern "C" {

sdm_status sdm_get_labeled_cloud(sdm_map *m, sdm_labeled_point *out) {
  if (!m || !out) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(out, m->cur_cloud, (size_t)m->d.W * m->d.H * sizeof(sdm_labeled_point), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return SDM_OK;
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
    SDM_TRY(regrow(m, &m->h_emit, &m->h_emit_bytes, grown, m->stream, true));
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
  if (cap > m->points_cap) SDM_TRY(regrow(m, &m->d_points, &m->points_cap, cap));
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
  if (!m->d_colours) SDM_TRY(alloc_tracked(m, &m->d_colours, 1));
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
  if (cap > m->points_rgb_cap) SDM_TRY(regrow(m, &m->d_points_rgb, &m->points_rgb_cap, cap));
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
  if (!m->h_track_bits) SDM_TRY(alloc_tracked(m, &m->h_track_bits, 2048, true));
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
  SDM_TRY(upload_stamps(m));
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
    DevTemps tmp;
    float *tx, *ty, *tz;
    uint8_t *tf;
    HIP_TRY(tmp.alloc(&tx, n));
    HIP_TRY(tmp.alloc(&ty, n));
    HIP_TRY(tmp.alloc(&tz, n));
    HIP_TRY(tmp.alloc(&tf, n));
    launch_unpack_pos4(m->st.pos4, m->st.forget, tx, ty, tz, tf, n, s);
    if (px) HIP_TRY(hipMemcpyAsync(px, tx, n * 4, hipMemcpyDeviceToHost, s));
    if (py) HIP_TRY(hipMemcpyAsync(py, ty, n * 4, hipMemcpyDeviceToHost, s));
    if (pz) HIP_TRY(hipMemcpyAsync(pz, tz, n * 4, hipMemcpyDeviceToHost, s));
    if (forget) HIP_TRY(hipMemcpyAsync(forget, tf, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (w || ts || track || label || status) {  // record fields -> the reference's slot order, through dense temporaries
    DevTemps tmp;
    float *tw;
    uint16_t *tts, *ttr;
    uint8_t *tl, *tst;
    HIP_TRY(tmp.alloc(&tw, n));
    HIP_TRY(tmp.alloc(&tts, n));
    HIP_TRY(tmp.alloc(&ttr, n));
    HIP_TRY(tmp.alloc(&tl, n));
    HIP_TRY(tmp.alloc(&tst, n));
    launch_rec_unpack(m->d, m->st, tw, tts, ttr, tl, tst, s);
    if (status) HIP_TRY(hipMemcpyAsync(status, tst, n, hipMemcpyDeviceToHost, s));
    if (w) HIP_TRY(hipMemcpyAsync(w, tw, n * 4, hipMemcpyDeviceToHost, s));
    if (ts) HIP_TRY(hipMemcpyAsync(ts, tts, n * 2, hipMemcpyDeviceToHost, s));
    if (track) HIP_TRY(hipMemcpyAsync(track, ttr, n * 2, hipMemcpyDeviceToHost, s));
    if (label) HIP_TRY(hipMemcpyAsync(label, tl, n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
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
  DevTemps tmp;
  float *tx, *ty, *tz;
  uint8_t *tf;
  HIP_TRY(tmp.alloc(&tx, n));
  HIP_TRY(tmp.alloc(&ty, n));
  HIP_TRY(tmp.alloc(&tz, n));
  HIP_TRY(tmp.alloc(&tf, n));
  HIP_TRY(hipMemcpyAsync(tx, px, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(ty, py, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(tz, pz, n * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(tf, forget, n, hipMemcpyHostToDevice, s));
  launch_pack_pos4(m->st.pos4, m->st.forget, tx, ty, tz, tf, n, s);
  {
    float *tw;
    uint16_t *tts, *ttr;
    uint8_t *tl, *tst;
    HIP_TRY(tmp.alloc(&tw, n));
    HIP_TRY(tmp.alloc(&tts, n));
    HIP_TRY(tmp.alloc(&ttr, n));
    HIP_TRY(tmp.alloc(&tl, n));
    HIP_TRY(tmp.alloc(&tst, n));
    HIP_TRY(hipMemcpyAsync(tst, status, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tw, w, n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tts, ts, n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ttr, track, n * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tl, label, n, hipMemcpyHostToDevice, s));
    launch_rec_pack(m->d, m->st, tw, tts, ttr, tl, tst, s);
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (owner) HIP_TRY(hipMemcpyAsync(m->st.owner, owner, n * 2, hipMemcpyHostToDevice, s));
  else HIP_TRY(hipMemsetAsync(m->st.owner, 0xFF, n * 2, s));
  launch_owner_flags(m->d, m->st, s);
  HIP_TRY(hipMemsetAsync(m->st.alias, 0, 8, s));  // the imported owner array is all there is to the sets
  HIP_TRY(hipMemsetAsync(m->st.alias_filter, 0, ALIAS_FILTER_WORDS * 4, s));
  launch_vflag_from_records(m->d, m->st, s);  // "something here" flags from the status rows (the voxel stamps came with slot 0 of the stamp rows)
  HIP_TRY(hipStreamSynchronize(s));
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

}  // extern "C"
