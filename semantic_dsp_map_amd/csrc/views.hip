// views.hip — view scoring for next-best-view exploration (gfx950): sdm_query_views (include/sdm.h, "view scoring").
//
// A view is a camera pose and a range; its rays are the caller's table of camera-frame directions.  Every ray is the
// segment sdm_query_segments would walk (clipped to the map, occ >= 1 blocks, unknown cells passed through), and per view
// the kernel counts the DISTINCT cells its rays visit, by class.  Like the other queries it reads the result array of the
// occupancy sweep (State::res) in stream order and the Frame of the last issued frame by value, and writes only the
// caller's outputs - and a pool of bitmasks of its own, one bit per voxel and view in flight, which every call leaves
// zeroed.
//
// The walk is k_query_segments' (sdm_walk.h has it and says why it goes SEG_K cells ahead); tests/test_views_gpu.py holds
// the two kernels together ray by ray, bit by bit.
#include <cstdlib>

#include "sdm_map.h"
#include "sdm_walk.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_view) == 32 && sizeof(sdm_view_gain) == 40 && sizeof(sdm_segment_hit) == 16, "sdm.h layouts");

namespace sdm {

namespace {

constexpr int VTPB = 256;
enum : int { VIEW_MARK = 0, VIEW_CLEAR = 1 };

// One lane per ray, a block row per view (blockIdx.y = the view within the batch = its mask in the pool).
// VIEW_MARK: a lane sets the bits of the cells of a batch with returned atomics, all issued together; where the bit was
// clear it is the first of the view to visit that cell and counts it by its class.  The atomics carry agent scope: the
// workgroups of a view sit on different XCDs, whose L2s do not see each other's plain writes, while a returned atomic is
// executed at the memory side.  Cells behind the blocking one are not marked: the number of cells to mark follows from the
// stop mask, before any atomic.  Counts are summed over the wave, then one set of atomic adds per wave goes to the view.
// VIEW_CLEAR: the same walk stores zero words over the cells the first pass marked (the alternative to zeroing the whole
// masks; DESIGN.md 5f has both measured).
template <int MODE>
__global__ __launch_bounds__(VTPB) void k_view_rays(Dims d, Frame f, const sdm_view *__restrict__ views, const float *__restrict__ dirs,
                                                    uint32_t n_rays, const uint2 *__restrict__ res, uint32_t *__restrict__ pool,
                                                    uint32_t mask_words, sdm_view_gain *__restrict__ gain,
                                                    sdm_segment_hit *__restrict__ rays_out, int32_t *__restrict__ unk_out) {
  const uint32_t r = blockIdx.x * VTPB + threadIdx.x;
  const uint32_t v = blockIdx.y;
  const bool live = r < n_rays;
  uint32_t *__restrict__ mask = pool + (size_t)v * mask_words;
  // the ray: a = pos, b = pos + range * (R(q) d), float32, one operation at a time (sdm.h pins the order)
  const float px = views[v].pos[0], py = views[v].pos[1], pz = views[v].pos[2];
  const float qw = views[v].q[0], qx = views[v].q[1], qy = views[v].q[2], qz = views[v].q[3];
  const float range = views[v].range;
  float dx = 0.f, dy = 0.f, dz = 0.f;
  if (live) {
    dx = dirs[3 * (size_t)r];
    dy = dirs[3 * (size_t)r + 1];
    dz = dirs[3 * (size_t)r + 2];
  }
  const bool given = live && isfinite(px) && isfinite(py) && isfinite(pz) && isfinite(qw) && isfinite(qx) && isfinite(qy) && isfinite(qz) &&
                     isfinite(range) && isfinite(dx) && isfinite(dy) && isfinite(dz);
  const float R[9] = {1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qw * qz), 2.f * (qx * qz + qw * qy),
                      2.f * (qx * qy + qw * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qw * qx),
                      2.f * (qx * qz - qw * qy), 2.f * (qy * qz + qw * qx), 1.f - 2.f * (qx * qx + qy * qy)};
  const float pa[3] = {px, py, pz};
  float ua[3], ub[3];
  bool finite = given;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float rd = (R[3 * a] * dx + R[3 * a + 1] * dy) + R[3 * a + 2] * dz;
    const float pb = range > 0.f ? pa[a] + range * rd : pa[a];  // (range <= 0: the zero-length segment, the cell of a)
    ua[a] = map_u(d, f, a, pa[a]);
    ub[a] = map_u(d, f, a, pb);
    finite = finite && isfinite(ua[a]) && isfinite(ub[a]);
  }
  float hit_t = -1.f;
  uint32_t hit_v = INVALID_INDEX, hit_w = RES_UNKNOWN_W1;
  int cells = 0;
  uint32_t n_unk = 0, n_free = 0, n_occ = 0, r_unk = 0;
  SegWalk sw;
  sw.kind = SEG_END;
  if (finite) {
    const SegClip cl = seg_begin(sw, d, ua, ub);
    if (cl.inside) {
      seg_enter_inside(sw, ua);
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
    uint32_t blocked = 0, ended = 0;
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) {
      blocked |= (uint32_t)(kd[k] == SEG_CELL && occ_of(w[k]) >= 1) << k;
      ended |= (uint32_t)(kd[k] != SEG_CELL) << k;
    }
    const uint32_t stop = blocked | ended;
    const int first = stop ? __builtin_ctz(stop) : SEG_K;
    const bool hit = stop && ((blocked >> first) & 1u);
    const int nm = first + (hit ? 1 : 0);  // cells of this batch the ray visits: all in the map, the last one may block
    if (MODE == VIEW_MARK) {
      uint32_t old[SEG_K];
#pragma unroll
      for (int k = 0; k < SEG_K; ++k) {  // up to SEG_K returned atomics in flight
        old[k] = 0xffffffffu;
        if (k < nm) old[k] = __hip_atomic_fetch_or(mask + (vox[k] >> 5), 1u << (vox[k] & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int k = 0; k < SEG_K; ++k) {
        const int8_t o = occ_of(w[k]);
        const bool visited = k < nm, fresh = visited && !((old[k] >> (vox[k] & 31u)) & 1u);
        n_unk += (uint32_t)(fresh && o == -1);
        n_free += (uint32_t)(fresh && o == 0);
        n_occ += (uint32_t)(fresh && o >= 1);
        r_unk += (uint32_t)(visited && o == -1);
      }
    } else {
#pragma unroll
      for (int k = 0; k < SEG_K; ++k)
        if (k < nm) mask[vox[k] >> 5] = 0u;
    }
    cells += nm;
    if (!stop) continue;
    if (hit) {
#pragma unroll
      for (int k = 0; k < SEG_K; ++k)  // (selected by compile-time index: no register array indexed at run time)
        if (k == first) {
          hit_t = tin[k];
          hit_v = vox[k];
          hit_w = w[k];
        }
    }
    break;
  }
  if (MODE == VIEW_CLEAR) return;
  if (live) {
    const size_t i = (size_t)v * n_rays + r;
    if (rays_out) {
      sdm_segment_hit h;
      h.t = hit_t;
      h.voxel = hit_v;
      h.cells = cells;
      __builtin_memcpy(&h.track, &hit_w, 4);
      uint4 o;
      __builtin_memcpy(&o, &h, 16);
      reinterpret_cast<uint4 *>(rays_out)[i] = o;
    }
    if (unk_out) unk_out[i] = (int32_t)r_unk;
  }
  // the wave's sums (lanes past the last ray carry zeros), one set of adds per wave that has anything
  const uint32_t s_unk = wave_sum(n_unk), s_free = wave_sum(n_free), s_occ = wave_sum(n_occ);
  const uint32_t s_hit = wave_sum((uint32_t)(hit_v != INVALID_INDEX)), s_in = wave_sum((uint32_t)(cells > 0));
  const uint32_t s_cells = wave_sum((uint32_t)cells), s_runk = wave_sum(r_unk);
  if ((threadIdx.x & 63u) == 0 && s_cells) {
    sdm_view_gain *g = gain + v;
    if (s_unk) atomicAdd(&g->n_unknown, s_unk);
    if (s_free) atomicAdd(&g->n_free, s_free);
    if (s_occ) atomicAdd(&g->n_occupied, s_occ);
    if (s_hit) atomicAdd(&g->rays_hit, s_hit);
    atomicAdd(&g->rays_in_map, s_in);
    atomicAdd(reinterpret_cast<unsigned long long *>(&g->ray_cells), (unsigned long long)s_cells);
    if (s_runk) atomicAdd(reinterpret_cast<unsigned long long *>(&g->ray_unknown), (unsigned long long)s_runk);
  }
}

constexpr size_t VIEW_POOL_BYTES = (size_t)64 << 20;  // what the pool may take; at least one mask, at most VIEW_POOL_MASKS
constexpr uint32_t VIEW_POOL_MASKS = 256;
constexpr size_t VIEW_CHUNK_RAYS = (size_t)1 << 20;   // host mode: rays per staged chunk (whole views; at least one)

// `n` views from device memory, in batches of as many as the pool has masks (or the test hook allows)
sdm_status views_enqueue(sdm_map *m, const Frame &f, const sdm_view *views, const float *dirs, uint32_t n_rays, size_t n, sdm_view_gain *out,
                         sdm_segment_hit *rays_out, int32_t *unk_out) {
  const uint32_t mask_words = m->d.V / 32u;
  if (!m->views.pool) {
    const size_t mask_bytes = (size_t)mask_words * 4;
    m->views.masks = (uint32_t)std::min<size_t>(VIEW_POOL_MASKS, std::max<size_t>(1, VIEW_POOL_BYTES / mask_bytes));
    SDM_TRY(alloc_tracked(m, &m->views.pool, (size_t)m->views.masks * mask_words));
    HIP_TRY(hipMemsetAsync(m->views.pool, 0, (size_t)m->views.masks * mask_bytes, m->stream));  // zero; every call leaves it zero again
  }
  const char *e = getenv("SDM_VIEW_CLEAR");  // A/B (tools/probes/views_probe.py): "rewalk" or "memset", looked up per call
  const bool rewalk = e ? strcmp(e, "rewalk") == 0 : m->views.clear_rewalk;
  const uint32_t B = m->views.batch > 0 ? std::min<uint32_t>(m->views.masks, (uint32_t)m->views.batch) : m->views.masks;
  const uint2 *res = reinterpret_cast<const uint2 *>(m->st.res);
  HIP_TRY(hipMemsetAsync(out, 0, n * sizeof(sdm_view_gain), m->stream));
  for (size_t v0 = 0; v0 < n; v0 += B) {
    const uint32_t nb = (uint32_t)std::min<size_t>(B, n - v0);
    const dim3 grid((n_rays + VTPB - 1) / VTPB, nb);
    sdm_segment_hit *ro = rays_out ? rays_out + v0 * n_rays : nullptr;
    int32_t *uo = unk_out ? unk_out + v0 * n_rays : nullptr;
    hipLaunchKernelGGL(k_view_rays<VIEW_MARK>, grid, dim3(VTPB), 0, m->stream, m->d, f, views + v0, dirs, n_rays, res, m->views.pool, mask_words,
                       out + v0, ro, uo);
    HIP_TRY(hipGetLastError());
    if (rewalk) {
      hipLaunchKernelGGL(k_view_rays<VIEW_CLEAR>, grid, dim3(VTPB), 0, m->stream, m->d, f, views + v0, dirs, n_rays, res, m->views.pool,
                         mask_words, (sdm_view_gain *)nullptr, (sdm_segment_hit *)nullptr, (int32_t *)nullptr);
      HIP_TRY(hipGetLastError());
    } else {
      HIP_TRY(hipMemsetAsync(m->views.pool, 0, (size_t)nb * mask_words * 4, m->stream));
    }
  }
  return SDM_OK;
}

}  // namespace

}  // namespace sdm

extern "C" {

sdm_status sdm_query_views(sdm_map *m, const sdm_view *views, int64_t n_views, const float *dirs, int32_t n_rays, sdm_view_gain *out,
                           sdm_segment_hit *rays_out, int32_t *ray_unknown_out, uint32_t flags) {
  SDM_TRY(query_check(m, views, n_views, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_views"));
  if (!dirs || n_rays < 1 || n_rays > SDM_VIEW_MAX_RAYS || n_views > (((int64_t)1 << 31) - 1) / n_rays) {
    set_error("sdm_query_views", __FILE__, __LINE__, "null ray table, n_rays outside 1 .. 65536, or n_views * n_rays >= 2^31");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  if (n_views == 0) return SDM_OK;
  HIP_TRY(hipSetDevice(m->device));
  const Frame f = m->f;
  const size_t n = (size_t)n_views, nr = (size_t)n_rays;
  if (flags & SDM_QUERY_ON_DEVICE) return views_enqueue(m, f, views, dirs, (uint32_t)n_rays, n, out, rays_out, ray_unknown_out);
  // host mode: the ray table goes up once, the views in chunks of whole views through the queries' staging area
  return run_staged(m, n, std::min(n, std::max<size_t>(1, VIEW_CHUNK_RAYS / nr)), dirs, nr * 12,
                    {{StageCol::IN, const_cast<sdm_view *>(views), sizeof(sdm_view)},
                     {StageCol::OUT, out, sizeof(sdm_view_gain)},
                     {StageCol::OUT, rays_out, rays_out ? nr * sizeof(sdm_segment_hit) : 0},
                     {StageCol::OUT, ray_unknown_out, ray_unknown_out ? nr * 4 : 0}},
                    [&](const unsigned char *pre, unsigned char *const *col, size_t c) {
                      return views_enqueue(m, f, reinterpret_cast<const sdm_view *>(col[0]), reinterpret_cast<const float *>(pre), (uint32_t)n_rays,
                                           c, reinterpret_cast<sdm_view_gain *>(col[1]), reinterpret_cast<sdm_segment_hit *>(col[2]),
                                           reinterpret_cast<int32_t *>(col[3]));
                    });
}

sdm_status sdm_debug_view_batch(sdm_map *m, int32_t max_views_in_flight) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->views.batch = max_views_in_flight > 0 ? max_views_in_flight : 0;
  return SDM_OK;
}

}  // extern "C"
