// queries.hip — batched map queries (gfx950): points, segments, boxes (include/sdm.h, "batched map queries").
//
// All three read the result array of the occupancy sweep (State::res, 8 B per voxel, indexed by storage index) and
// nothing else of the map; they write only the caller's outputs.  The grid geometry (Dims) and the ring state of the
// last issued frame (Frame: map center, ring offsets) come by value, so a query enqueued between two frames answers for
// the frame before it whatever the host does next.  Segments and boxes only need the second word of a result (track,
// label, occ): they gather 4 bytes per cell.
#include "sdm_map.h"
#include "sdm_walk.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_segment_hit) == 16 && sizeof(sdm_box_result) == 20 && sizeof(sdm_voxel_result) == 8, "sdm.h layouts");

namespace sdm {

namespace {

constexpr int QTPB = 256;
// ---- points: one lane per query, one 8-byte gather -----------------------------------------------------------------
__global__ __launch_bounds__(QTPB) void k_query_points(Dims d, Frame f, const float *__restrict__ xyz, uint32_t n,
                                                       const uint2 *__restrict__ res, uint2 *__restrict__ out,
                                                       uint32_t *__restrict__ voxel_out) {
  const uint32_t i = blockIdx.x * QTPB + threadIdx.x;
  if (i >= n) return;
  const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
  uint32_t rx, ry, rz;
  const uint32_t v = global_pos_to_voxel(d, f, px, py, pz, rx, ry, rz);  // (NaN / inf fail its range test: outside)
  const uint2 r = v != INVALID_INDEX ? res[v] : make_uint2(RES_UNKNOWN_W0, RES_UNKNOWN_W1);
  out[i] = r;
  if (voxel_out) voxel_out[i] = v;
}

// ---- segments: one lane per segment, the walk of sdm_walk.h ---------------------------------------------------------
__global__ __launch_bounds__(QTPB) void k_query_segments(Dims d, Frame f, const float *__restrict__ ab, uint32_t n,
                                                         const uint2 *__restrict__ res, sdm_segment_hit *__restrict__ out,
                                                         int unknown_blocks) {
  const uint32_t i = blockIdx.x * QTPB + threadIdx.x;
  if (i >= n) return;
  float ua[3], ub[3];
  bool finite = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ua[a] = map_u(d, f, a, ab[6 * (size_t)i + a]);
    ub[a] = map_u(d, f, a, ab[6 * (size_t)i + 3 + a]);
    finite = finite && isfinite(ua[a]) && isfinite(ub[a]);
  }
  float hit_t = -1.f;
  uint32_t hit_v = INVALID_INDEX, hit_w = RES_UNKNOWN_W1;
  int cells = 0;
  SegWalk sw;
  sw.kind = SEG_END;
  if (!finite) {
    if (unknown_blocks) hit_t = 0.f;
  } else {
    const SegClip cl = seg_begin(sw, d, ua, ub);
    if (cl.inside) {
      seg_enter_inside(sw, ua);
    } else if (unknown_blocks) {
      hit_t = 0.f;  // a lies outside the map, which blocks
    } else if (cl.enters()) {
      seg_enter_clipped(sw, cl, ub);
    }
    seg_planes(sw);
  }
  while (sw.kind != SEG_END) {
    uint32_t vox[SEG_K], w[SEG_K];
    float tin[SEG_K];
    int kd[SEG_K];
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) {  // the next SEG_K cells: arithmetic only
      kd[k] = sw.kind;
      tin[k] = (float)sw.t_cur;
      seg_advance(sw, vox[k], [&](int x, int y, int z) { return cell_voxel(d, f, x, y, z); });
    }
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) w[k] = res[kd[k] == SEG_CELL ? vox[k] : 0u].y;  // SEG_K independent loads
    uint32_t stop = 0;
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) {
      const int8_t o = occ_of(w[k]);
      const bool blocks = o >= 1 || (unknown_blocks && o == -1);
      stop |= (uint32_t)(kd[k] != SEG_CELL || blocks) << k;
    }
    if (!stop) {
      cells += SEG_K;
      continue;
    }
    const int first = __builtin_ctz(stop);
    int fk = SEG_END;
    float ft = 0.f;
    uint32_t fv = INVALID_INDEX, fw = RES_UNKNOWN_W1;
#pragma unroll
    for (int k = 0; k < SEG_K; ++k)  // (selected by compile-time index: no register array indexed at run time)
      if (k == first) {
        fk = kd[k];
        ft = tin[k];
        fv = vox[k];
        fw = w[k];
      }
    cells += first + (fk == SEG_CELL ? 1 : 0);
    if (fk == SEG_CELL) {
      hit_t = ft;
      hit_v = fv;
      hit_w = fw;
    } else if (fk == SEG_OUT && unknown_blocks) {
      hit_t = ft;
    }
    break;
  }
  sdm_segment_hit h;
  h.t = hit_t;
  h.voxel = hit_v;
  h.cells = cells;
  __builtin_memcpy(&h.track, &hit_w, 4);
  uint4 v;
  __builtin_memcpy(&v, &h, 16);
  reinterpret_cast<uint4 *>(out)[i] = v;
}

// ---- boxes: one wave per box, lanes along x ------------------------------------------------------------------------
// The box's cells are numbered x fastest, so consecutive lanes read consecutive cells of an x row (contiguous in storage
// except where the ring wraps), and a narrow footprint still keeps all 64 lanes busy.  Each lane takes BOX_U cells per
// round, loads first.  Counts are wave-wide ballots (popcount in scalar registers), first_occupied a min over the wave.
constexpr int BOX_U = 4;

__global__ __launch_bounds__(QTPB) void k_query_boxes(Dims d, Frame f, const float *__restrict__ boxes, uint32_t n,
                                                      const uint2 *__restrict__ res, sdm_box_result *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = blockIdx.x * (QTPB / 64) + (threadIdx.x >> 6);
  if (b >= n) return;
  const int N[3] = {(int)d.NX, (int)d.NY, (int)d.NZ};
  int lo[3], w[3];
  bool valid = true, clipped = false, empty = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float pl = boxes[6 * (size_t)b + a], ph = boxes[6 * (size_t)b + 3 + a];
    valid = valid && isfinite(pl) && isfinite(ph) && pl <= ph;
    const float fl = floorf(map_u(d, f, a, pl)), fh = floorf(map_u(d, f, a, ph));
    clipped = clipped || fl < 0.f || fh >= (float)N[a];
    // (clamped in float - a coordinate far outside may overflow u to +-inf -: the casts see values inside the map only)
    const int l = (int)fmaxf(fl, 0.f), h = (int)fminf(fh, (float)(N[a] - 1));
    lo[a] = l;
    w[a] = h - l + 1;
    empty = empty || !(fl <= (float)(N[a] - 1) && fh >= 0.f);
  }
  uint32_t n_occ = 0, n_free = 0, n_unk = 0, first = INVALID_INDEX;
  if (valid && !empty) {
    const uint32_t wx = (uint32_t)w[0], wxy = wx * (uint32_t)w[1], total = wxy * (uint32_t)w[2];
    for (uint32_t base = 0; base < total; base += 64u * BOX_U) {
      uint32_t vox[BOX_U], r[BOX_U];
      bool in[BOX_U];
#pragma unroll
      for (int u = 0; u < BOX_U; ++u) {
        const uint32_t k = base + (uint32_t)u * 64u + lane;
        in[u] = k < total;
        const uint32_t z = k / wxy, rem = k - z * wxy, y = rem / wx, x = rem - y * wx;
        vox[u] = in[u] ? cell_voxel(d, f, lo[0] + (int)x, lo[1] + (int)y, lo[2] + (int)z) : 0u;
      }
#pragma unroll
      for (int u = 0; u < BOX_U; ++u) r[u] = res[vox[u]].y;
#pragma unroll
      for (int u = 0; u < BOX_U; ++u) {
        const int8_t o = occ_of(r[u]);
        const bool occ = in[u] && o >= 1;
        n_occ += (uint32_t)__popcll(__ballot(occ));
        n_free += (uint32_t)__popcll(__ballot(in[u] && o == 0));
        n_unk += (uint32_t)__popcll(__ballot(in[u] && o == -1));
        if (occ) first = min(first, vox[u]);
      }
    }
    first = wave_min(first);
  }
  if (lane == 0) {
    sdm_box_result o;
    o.n_occupied = (int32_t)n_occ;
    o.n_free = (int32_t)n_free;
    o.n_unknown = (int32_t)n_unk;
    o.first_occupied = first;
    o.clipped = valid && clipped ? 1 : 0;
    out[b] = o;
  }
}

}  // namespace

void launch_query_points(const Dims &d, const Frame &f, const State &st, const float *xyz, uint32_t n, sdm_voxel_result *out,
                         uint32_t *voxel_out, hipStream_t s) {
  hipLaunchKernelGGL(k_query_points, dim3((n + QTPB - 1) / QTPB), dim3(QTPB), 0, s, d, f, xyz, n,
                     reinterpret_cast<const uint2 *>(st.res), reinterpret_cast<uint2 *>(out), voxel_out);
}

void launch_query_segments(const Dims &d, const Frame &f, const State &st, const float *ab, uint32_t n, sdm_segment_hit *out,
                           int unknown_blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_query_segments, dim3((n + QTPB - 1) / QTPB), dim3(QTPB), 0, s, d, f, ab, n,
                     reinterpret_cast<const uint2 *>(st.res), out, unknown_blocks);
}

void launch_query_boxes(const Dims &d, const Frame &f, const State &st, const float *boxes, uint32_t n, sdm_box_result *out,
                        hipStream_t s) {
  constexpr uint32_t per_block = QTPB / 64;
  hipLaunchKernelGGL(k_query_boxes, dim3((n + per_block - 1) / per_block), dim3(QTPB), 0, s, d, f, boxes, n,
                     reinterpret_cast<const uint2 *>(st.res), out);
}

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
// Host mode works through the queries in chunks of QUERY_CHUNK: inputs copied to the map's page-locked staging area and
// up, the kernel, the outputs down, one wait per chunk (run_staged: every host-mode batched call goes through it).  Device
// mode launches per chunk too (the kernels count in 32 bits) and does not wait.  Either way the kernels read the result
// array in stream order and the host Frame of the last issued frame, taken by value at the call.
namespace sdm {

namespace {
constexpr size_t QUERY_CHUNK = (size_t)1 << 20;
}  // namespace

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

sdm_status layer_check(sdm_map *m, const char *what, const Derived *need, const LayerName &name) {
  char msg[160];
  if (m->cfg.shard_count > 1) {
    std::snprintf(msg, sizeof(msg), "%s of a Z-slab shard (shard_count > 1) %s not supported: build %s on a whole map", name.the_layer,
                  name.plural ? "are" : "is", name.plural ? "them" : "it");
  } else if (need && !need->valid) {
    std::snprintf(msg, sizeof(msg), "no %s: call %s first", name.build, name.update);
  } else {
    return SDM_OK;
  }
  set_error(what, __FILE__, __LINE__, msg);
  return SDM_ERR_INVALID_ARGUMENT;
}

sdm_status layer_scan_scratch(sdm_map *m, size_t longest, uint32_t **scratch) {
  const size_t elems = scan_scratch_elems(longest);
  if (elems > m->layer_scan_elems) {  // (the old one goes once the scans that use it have run)
    SDM_TRY(regrow(m, &m->layer_scan, &m->layer_scan_elems, elems, m->layer_scan ? m->stream : nullptr));
    HIP_TRY(hipMemsetAsync(m->layer_scan, 0, elems * sizeof(uint32_t), m->stream));  // (the scans leave its fixed region zeroed)
  }
  *scratch = m->layer_scan;
  return SDM_OK;
}

void layer_origin(const sdm_map *m, const Derived &l, float origin[3]) {
  if (origin)
    for (int a = 0; a < 3; ++a) origin[a] = l.f.center[a] + m->d.pmin[a];
}

// The staging area holds the preamble and one chunk of every column, each at a multiple of 256 bytes, in the order given.
sdm_status run_staged(sdm_map *m, size_t n, size_t chunk, const void *pre, size_t pre_bytes, const std::vector<StageCol> &cols,
                      const StageLaunch &launch, const StageCopyOut &copy_out) {
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t k_n = cols.size();
  std::vector<size_t> at(k_n);
  size_t need = align(pre_bytes);
  for (size_t k = 0; k < k_n; ++k) {
    at[k] = need;
    need += align(chunk * cols[k].elem);
  }
  QueryStage &st = m->stage;
  if (need > st.bytes) {  // both buffers grow together; the pinned one goes once the stream that may use it has drained
    const size_t grown = std::max(need, (size_t)1 << 20);
    size_t cap = 0;
    st.bytes = 0;  // (non-zero only while both are there)
    SDM_TRY(regrow(m, &st.h, &cap, grown, m->stream, true));
    SDM_TRY(regrow(m, &st.d, &cap, grown));
    st.bytes = grown;
  }
  std::vector<unsigned char *> dev(k_n), host(k_n);
  for (size_t k = 0; k < k_n; ++k) {
    dev[k] = cols[k].elem ? st.d + at[k] : nullptr;
    host[k] = cols[k].elem ? st.h + at[k] : nullptr;
  }
  if (pre_bytes) {
    memcpy(st.h, pre, pre_bytes);
    HIP_TRY(hipMemcpyAsync(st.d, st.h, pre_bytes, hipMemcpyHostToDevice, m->stream));
  }
  for (size_t off = 0; off < n; off += chunk) {
    const size_t c = std::min(chunk, n - off);
    for (size_t k = 0; k < k_n; ++k) {
      if (cols[k].kind != StageCol::IN || !cols[k].elem) continue;
      memcpy(host[k], static_cast<const unsigned char *>(cols[k].host) + off * cols[k].elem, c * cols[k].elem);
      HIP_TRY(hipMemcpyAsync(dev[k], host[k], c * cols[k].elem, hipMemcpyHostToDevice, m->stream));
    }
    SDM_TRY(launch(st.d, dev.data(), c));
    for (size_t k = 0; k < k_n; ++k)
      if (cols[k].kind != StageCol::IN && cols[k].elem)
        HIP_TRY(hipMemcpyAsync(host[k], dev[k], c * cols[k].elem, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (size_t k = 0; k < k_n; ++k)
      if (cols[k].kind == StageCol::OUT && cols[k].elem) memcpy(static_cast<unsigned char *>(cols[k].host) + off * cols[k].elem, host[k], c * cols[k].elem);
    if (copy_out) copy_out(host.data(), off, c);
  }
  return SDM_OK;
}

sdm_status run_query(sdm_map *m, const void *in_v, size_t in_elem, void *out_v, size_t out_elem, void *out2_v, size_t out2_elem, int64_t n,
                     uint32_t flags, const QueryLaunch &launch) {
  if (n == 0) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  if (!out2_v) out2_elem = 0;
  if (flags & SDM_QUERY_ON_DEVICE) {
    const unsigned char *in = static_cast<const unsigned char *>(in_v);
    unsigned char *out = static_cast<unsigned char *>(out_v), *out2 = static_cast<unsigned char *>(out2_v);
    for (size_t off = 0; off < (size_t)n; off += QUERY_CHUNK) {
      const uint32_t c = (uint32_t)std::min(QUERY_CHUNK, (size_t)n - off);
      launch(in + off * in_elem, out + off * out_elem, out2 ? out2 + off * out2_elem : nullptr, c, m->stream);
      HIP_TRY(hipGetLastError());
    }
    return SDM_OK;
  }
  return run_staged(m, (size_t)n, std::min(QUERY_CHUNK, (size_t)n), nullptr, 0,
                    {{StageCol::IN, const_cast<void *>(in_v), in_elem}, {StageCol::OUT, out_v, out_elem}, {StageCol::OUT, out2_v, out2_elem}},
                    [&](const unsigned char *, unsigned char *const *col, size_t c) -> sdm_status {
                      launch(col[0], col[1], col[2], (uint32_t)c, m->stream);
                      HIP_TRY(hipGetLastError());
                      return SDM_OK;
                    });
}
}  // namespace sdm

extern "C" {

sdm_status sdm_query_points(sdm_map *m, const float *xyz, int64_t n, sdm_voxel_result *out, uint32_t *voxel_out, uint32_t flags) {
  SDM_TRY(query_check(m, xyz, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_points"));
  const Frame f = m->f;
  return run_query(m, xyz, 12, out, sizeof(sdm_voxel_result), voxel_out, 4, n, flags,
                   [m, f](const void *in, void *o, void *o2, uint32_t c, hipStream_t s) {
                     launch_query_points(m->d, f, m->st, static_cast<const float *>(in), c, static_cast<sdm_voxel_result *>(o),
                                         static_cast<uint32_t *>(o2), s);
                   });
}

sdm_status sdm_query_segments(sdm_map *m, const float *ab, int64_t n, sdm_segment_hit *out, uint32_t flags) {
  SDM_TRY(query_check(m, ab, n, out, flags, SDM_QUERY_ON_DEVICE | SDM_QUERY_UNKNOWN_BLOCKS, "sdm_query_segments"));
  const Frame f = m->f;
  const int unknown_blocks = (flags & SDM_QUERY_UNKNOWN_BLOCKS) ? 1 : 0;
  return run_query(m, ab, 24, out, sizeof(sdm_segment_hit), nullptr, 0, n, flags,
                   [m, f, unknown_blocks](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     launch_query_segments(m->d, f, m->st, static_cast<const float *>(in), c, static_cast<sdm_segment_hit *>(o),
                                           unknown_blocks, s);
                   });
}

sdm_status sdm_query_boxes(sdm_map *m, const float *boxes, int64_t n, sdm_box_result *out, uint32_t flags) {
  SDM_TRY(query_check(m, boxes, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_boxes"));
  const Frame f = m->f;
  return run_query(m, boxes, 24, out, sizeof(sdm_box_result), nullptr, 0, n, flags,
                   [m, f](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     launch_query_boxes(m->d, f, m->st, static_cast<const float *>(in), c, static_cast<sdm_box_result *>(o), s);
                   });
}

}  // extern "C"
