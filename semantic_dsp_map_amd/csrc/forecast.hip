// forecast.hip — the forecast: where the moving objects of the map will be at a few horizons, from one translation
// velocity per track, and the point-time and space-time segment queries on it (gfx950; include/sdm.h, "forecast").
//
// A snapshot of one frame in map-index cells, like the distance field, the instance table, the frontiers and the travel
// cost.  The host turns motions x horizons into stamps - integer cell shifts (expand(): pure host code, also exported
// on its own as sdm_forecast_stamps) - and the device moves every source cell by every stamp of its track.
//   k_forecast_classify  a wave per chunk of 64 cells in map-index order (FC_U chunks a wave, all loads first): reads
//               the results through the ring correction, looks the winning track up in the motions' 65536-bit set (8 KB,
//               through L2) and writes mask = class << 16 and first = 0xffffffff for every cell - no memset - and counts
//               the sources, one atomic a wave.
//   k_forecast_scatter   after it, at a kernel boundary: a wave per chunk of mask words; takes the class-3 cells by
//               ballot, re-reads their track and walks the track's stamps (found through the per-track offsets) in lock
//               step: lanes are consecutive source cells, so one stamp's atomicOr(mask) / atomicMin(first) land on adjacent
//               words.  The class bits of a mask word never change in this launch, so reading them beside the atomics of
//               other waves is no race.  Landings outside the block are dropped; both kinds are counted, one 64-bit
//               atomic each a wave.  There is no list of the sources (it would need a capacity): a wave's work is its
//               sources times their stamps, which under SWEPT is uneven for a fast object.
//   k_forecast_reduce    counts the cells with any horizon bit.
//   k_query_forecast     a lane per point and time.
//   k_query_forecast_segments   a lane per segment: k_query_segments' walk (sdm_walk.h), reading mask words in map-index
//               order instead of results, plus per cell the times at which it is entered and left and the horizon bits
//               between them.
//   k_forecast_cells_count / exclusive_scan_u32 / k_forecast_cells_write   the list of marked cells in ascending cell
//               word: word popcounts, their scan, a write pass (as the frontiers compact theirs).
// Only integer OR / MIN / ADD atomics: the field is bitwise the same from run to run.
#include <cmath>

#include "sdm_map.h"
#include "sdm_walk.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_motion) == 16 && sizeof(sdm_forecast_stamp) == 12 && sizeof(sdm_forecast_info) == 40, "sdm.h layouts");
static_assert(sizeof(sdm_forecast_result) == 8 && sizeof(sdm_forecast_hit) == 16, "sdm.h layouts");
static_assert(SDM_FORECAST_MAX_HORIZONS == 16, "the horizon bits are the low half of a mask word");

namespace sdm {

namespace {

constexpr int FC_TPB = 256, FC_WAVES = FC_TPB / 64;
constexpr int FC_U = 8;             // chunks of 64 cells a wave takes
constexpr int FQ_TPB = 256;
constexpr uint32_t FR_GRID = 1024;  // k_forecast_reduce strides over the chunks
constexpr uint32_t NOTHING = 0xffffffffu;
constexpr int SHIFT_MAX = 1024;     // a stamp's components lie in [-SHIFT_MAX, SHIFT_MAX]
constexpr uint32_t SET_WORDS = 65536 / 32;
enum { M_SOURCES = 0, M_MARKED, M_IN, M_OUT, META_WORDS };

// The build's table, one array of words: the track set, off[0 .. max_track + 1] (track t's stamps are off[t] .. off[t + 1]),
// the stamps as two words each: dx + 1024 | (dy + 1024) << 12 | horizon << 24, dz + 1024.
struct Table {
  const uint32_t *set, *off;
  const uint2 *stamps;
};

struct Field {  // what a query reads
  const uint32_t *mask, *first;
  float t[SDM_FORECAST_MAX_HORIZONS];  // +inf beyond n_h
  int n_h;
};

// ---- classify --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_TPB) void k_forecast_classify(Dims d, Frame f, const uint2 *__restrict__ res, const uint32_t *__restrict__ set,
                                                              uint32_t *__restrict__ mask, uint32_t *__restrict__ first, u64 *__restrict__ meta,
                                                              uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t chunk0 = (blockIdx.x * FC_WAVES + (threadIdx.x >> 6)) * FC_U;
  uint32_t w[FC_U];
  load_w1(d, f, res, chunk0, nw, lane, w);
  uint32_t in_set[FC_U];
#pragma unroll
  for (int u = 0; u < FC_U; ++u) in_set[u] = set[(w[u] & 0xffffu) >> 5];  // (any track has a word: the set holds all 65536)
  uint32_t n_src = 0;
#pragma unroll
  for (int u = 0; u < FC_U; ++u) {
    const uint32_t chunk = chunk0 + (uint32_t)u;
    if (chunk >= nw) break;  // (wave-uniform)
    const uint32_t c = (chunk << 6) + lane;
    const int occ = occ_of(w[u]);
    const bool moves = (in_set[u] >> (w[u] & 31u)) & 1u;
    const uint32_t cls = occ == -1 ? 0u : occ == 0 ? 1u : moves ? 3u : 2u;
    n_src += (uint32_t)__popcll(__ballot(cls == 3u));
    mask[c] = cls << 16;
    first[c] = NOTHING;
  }
  if (lane == 0 && n_src) atomicAdd(meta + M_SOURCES, (u64)n_src);
}

// ---- scatter ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_TPB) void k_forecast_scatter(Dims d, Frame f, const uint2 *__restrict__ res, Table tb, uint32_t *mask,
                                                             uint32_t *first, u64 *__restrict__ meta, uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t chunk0 = (blockIdx.x * FC_WAVES + (threadIdx.x >> 6)) * FC_U;
  uint32_t mw[FC_U];
#pragma unroll
  for (int u = 0; u < FC_U; ++u) {
    const uint32_t chunk = chunk0 + (uint32_t)u;
    mw[u] = chunk < nw ? mask[(chunk << 6) + lane] : 0u;
  }
  u64 n_in = 0, n_all = 0;
#pragma unroll
  for (int u = 0; u < FC_U; ++u) {
    const bool src = ((mw[u] >> 16) & 3u) == 3u;
    if (!__ballot(src)) continue;  // (wave-uniform; chunks beyond the map read 0)
    const uint32_t c = ((chunk0 + (uint32_t)u) << 6) + lane;
    int x, y, z;
    cell_xyz(d, c, x, y, z);
    uint32_t track = 0, beg = 0, cnt = 0;
    if (src) {
      track = res[cell_voxel(d, f, x, y, z)].y & 0xffffu;  // (in the set, so 1 <= track <= max_track: off[track + 1] exists)
      beg = tb.off[track];
      cnt = tb.off[track + 1u] - beg;
    }
    n_all += cnt;
    const uint32_t longest = wave_max(cnt);
    for (uint32_t j = 0; j < longest; ++j) {  // (wave-uniform bound: the lanes of one object go through its stamps together)
      if (j >= cnt) continue;
      const uint2 st = tb.stamps[beg + j];
      const int tx = x + (int)(st.x & 0xfffu) - SHIFT_MAX, ty = y + (int)((st.x >> 12) & 0xfffu) - SHIFT_MAX, tz = z + (int)st.y - SHIFT_MAX;
      const uint32_t k = st.x >> 24;
      if ((uint32_t)tx < d.NX && (uint32_t)ty < d.NY && (uint32_t)tz < d.NZ) {
        const uint32_t t = cell_word(d, tx, ty, tz);  // < V
        atomicOr(mask + t, 1u << k);
        atomicMin(first + t, (k << 16) | track);
        ++n_in;
      }
    }
  }
  n_in = wave_sum64(n_in);
  n_all = wave_sum64(n_all);
  if (lane == 0) {
    if (n_in) atomicAdd(meta + M_IN, n_in);
    if (n_all - n_in) atomicAdd(meta + M_OUT, n_all - n_in);
  }
}

// ---- the info block ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_TPB) void k_forecast_reduce(const uint32_t *__restrict__ mask, u64 *__restrict__ meta, uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n = 0;
  for (uint32_t chunk = blockIdx.x * FC_WAVES + (threadIdx.x >> 6); chunk < nw; chunk += gridDim.x * FC_WAVES)  // (wave-uniform)
    n += (uint32_t)__popcll(__ballot((mask[(chunk << 6) + lane] & 0xffffu) != 0u));
  if (lane == 0 && n) atomicAdd(meta + M_MARKED, (u64)n);
}

// ---- the cell list ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FC_TPB) void k_forecast_cells_count(const uint32_t *__restrict__ mask, uint32_t *__restrict__ pre, uint32_t nw) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t chunk = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
  if (chunk >= nw) return;  // (wave-uniform)
  const u64 m = __ballot((mask[(chunk << 6) + lane] & 0xffffu) != 0u);
  if (lane == 0) pre[chunk] = (uint32_t)__popcll(m);
}

__global__ __launch_bounds__(FC_TPB) void k_forecast_cells_write(const uint32_t *__restrict__ mask, const uint32_t *__restrict__ first,
                                                                 const uint32_t *__restrict__ pre, uint32_t nw, uint32_t take,
                                                                 uint32_t *__restrict__ cell_out, uint32_t *__restrict__ mask_out,
                                                                 uint32_t *__restrict__ first_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t chunk = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
  if (chunk >= nw) return;  // (wave-uniform)
  const uint32_t c = (chunk << 6) + lane;
  const uint32_t mw = mask[c];
  const bool marked = (mw & 0xffffu) != 0u;
  const u64 m = __ballot(marked);
  if (!marked) return;
  const uint32_t r = pre[chunk] + lane_rank(m, lane);
  if (r >= take) return;  // nothing is written beyond the caller's capacity
  if (cell_out) cell_out[r] = c;
  if (mask_out) mask_out[r] = mw;
  if (first_out) first_out[r] = first[c];
}

// ---- queries ----------------------------------------------------------------------------------------------------------
// the horizon of time T: the smallest k with T <= t[k], the last one beyond (t[k] = +inf for k >= n_h)
__device__ __forceinline__ uint32_t horizon_of(const Field &g, double T) {
  int k = 0;
#pragma unroll
  for (int j = 0; j < SDM_FORECAST_MAX_HORIZONS; ++j) k += (double)g.t[j] < T ? 1 : 0;
  return (uint32_t)min(k, g.n_h - 1);
}

__global__ __launch_bounds__(FQ_TPB) void k_query_forecast(Dims d, Frame f, Field g, const float *__restrict__ xyzt, uint32_t n,
                                                           uint2 *__restrict__ out) {
  const uint32_t i = blockIdx.x * FQ_TPB + threadIdx.x;
  if (i >= n) return;
  const float4 p = reinterpret_cast<const float4 *>(xyzt)[i];
  const float pos[3] = {p.x, p.y, p.z};
  const uint32_t c = point_cell(d, f, pos);
  uint2 o = make_uint2(0xff00u | 0xffu, 0x00ff0000u);  // state -1, horizon 0xff; track 0; mask 0, first_horizon 0xff, pad 0
  if (isfinite(p.w) && c != INVALID_INDEX) {
    const uint32_t mw = g.mask[c], fw = g.first[c];
    const uint32_t k = horizon_of(g, (double)p.w);
    const uint32_t cls = (mw >> 16) & 3u;
    const int state = cls == 2u ? 1 : ((mw >> k) & 1u) ? 2 : cls == 3u ? 3 : cls == 1u ? 0 : -1;
    const uint32_t track = fw == NOTHING ? 0u : fw & 0xffffu, fh = fw == NOTHING ? 0xffu : (fw >> 16) & 0xffu;
    o.x = ((uint32_t)state & 0xffu) | (k << 8) | (track << 16);
    o.y = (mw & 0xffffu) | (fh << 16);
  }
  out[i] = o;
}

__global__ __launch_bounds__(FQ_TPB) void k_query_forecast_segments(Dims d, Frame f, Field g, const float *__restrict__ seg, uint32_t n,
                                                                    sdm_forecast_hit *__restrict__ out, int unknown_blocks, int vacated_blocks) {
  const uint32_t i = blockIdx.x * FQ_TPB + threadIdx.x;
  if (i >= n) return;
  float ua[3], ub[3];
  const float ta = seg[8 * (size_t)i + 3], tb = seg[8 * (size_t)i + 7];
  bool finite = isfinite(ta) && isfinite(tb) && ta <= tb;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ua[a] = map_u(d, f, a, seg[8 * (size_t)i + a]);
    ub[a] = map_u(d, f, a, seg[8 * (size_t)i + 4 + a]);
    finite = finite && isfinite(ua[a]) && isfinite(ub[a]);
  }
  const double T0 = (double)ta, dT = (double)tb - (double)ta;
  float hit_t = -1.f;
  uint32_t hit_c = NOTHING, hit_track = 0u, hit_h = 0xffu;
  int hit_state = 0;
  int cells = 0;
  SegWalk sw;
  sw.kind = SEG_END;
  if (!finite) {
    if (unknown_blocks) hit_t = 0.f, hit_state = -1;
  } else {
    const SegClip cl = seg_begin(sw, d, ua, ub);
    if (cl.inside) {
      seg_enter_inside(sw, ua);
    } else if (unknown_blocks) {
      hit_t = 0.f, hit_state = -1;  // a lies outside the map, which blocks
    } else if (cl.enters()) {
      seg_enter_clipped(sw, cl, ub);
    }
    seg_planes(sw);
  }
  while (sw.kind != SEG_END) {
    uint32_t word[SEG_K], w[SEG_K], range[SEG_K];
    float tin[SEG_K];
    int kd[SEG_K];
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) {  // the next SEG_K cells: arithmetic only
      kd[k] = sw.kind;
      tin[k] = (float)sw.t_cur;
      const double tau_in = sw.t_cur;
      const double tau_out = seg_advance(sw, word[k], [&](int x, int y, int z) { return cell_word(d, x, y, z); });
      // the horizon bits of the time the cell is occupied (lo <= hi: T is monotonic in tau)
      const uint32_t lo = horizon_of(g, T0 + tau_in * dT), hi = horizon_of(g, T0 + tau_out * dT);
      range[k] = (2u << hi) - (1u << lo);
    }
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) w[k] = g.mask[kd[k] == SEG_CELL ? word[k] : 0u];  // SEG_K independent loads
    uint32_t stop = 0;
#pragma unroll
    for (int k = 0; k < SEG_K; ++k) {
      const uint32_t cls = (w[k] >> 16) & 3u;
      const bool blocks = cls == 2u || (w[k] & range[k]) != 0u || (unknown_blocks && cls == 0u) || (vacated_blocks && cls == 3u);
      stop |= (uint32_t)(kd[k] != SEG_CELL || blocks) << k;
    }
    if (!stop) {
      cells += SEG_K;
      continue;
    }
    const int first = __builtin_ctz(stop);
    int fk = SEG_END;
    float ft = 0.f;
    uint32_t fc = NOTHING, fw = 0u, fr = 0u;
#pragma unroll
    for (int k = 0; k < SEG_K; ++k)  // (selected by compile-time index: no register array indexed at run time)
      if (k == first) {
        fk = kd[k];
        ft = tin[k];
        fc = word[k];
        fw = w[k];
        fr = range[k];
      }
    cells += first + (fk == SEG_CELL ? 1 : 0);
    if (fk == SEG_CELL) {
      const uint32_t cls = (fw >> 16) & 3u, bits = fw & fr;
      hit_t = ft;
      hit_c = fc;
      hit_state = cls == 2u ? 1 : bits ? 2 : cls == 3u ? 3 : -1;
      if (hit_state == 2) {
        hit_h = (uint32_t)__builtin_ctz(bits);
        hit_track = g.first[fc] & 0xffffu;
      }
    } else if (fk == SEG_OUT && unknown_blocks) {
      hit_t = ft;
      hit_state = -1;
    }
    break;
  }
  uint4 v;
  v.x = __float_as_uint(hit_t);
  v.y = hit_c;
  v.z = (uint32_t)cells;
  v.w = hit_track | (((uint32_t)hit_state & 0xffu) << 16) | (hit_h << 24);
  reinterpret_cast<uint4 *>(out)[i] = v;
}

}  // namespace

}  // namespace sdm

// ---- the host side: the stamps, and the entry points behind include/sdm.h ------------------------------------------
namespace {
constexpr LayerName FORECAST = {"the forecast", "forecast", "sdm_forecast_update", false};

// The checks of the motions and horizons and their expansion into stamps (sdm.h): emit(track, horizon, d) sees the first
// `limit` stamps in order, *n_out is how many there are.  max_track < 0: no upper bound on the tracks (no map to ask).
template <typename Emit>
sdm_status expand(const char *what, float voxel_size, const sdm_motion *motions, int32_t n_motions, const float *horizons, int32_t n_horizons,
                  uint32_t flags, int max_track, int64_t limit, int64_t *n_out, const Emit &emit) {
  if (flags & ~SDM_FORECAST_SWEPT) return LAYER_REFUSE(what, "unknown flag bits");
  if (!(voxel_size > 0.f) || !std::isfinite(voxel_size)) return LAYER_REFUSE(what, "voxel_size is not a positive number");
  if (n_motions < 0 || (n_motions > 0 && !motions)) return LAYER_REFUSE(what, "n_motions < 0, or no motions");
  if (n_horizons < 1 || n_horizons > SDM_FORECAST_MAX_HORIZONS || !horizons)
    return LAYER_REFUSE(what, "n_horizons outside 1 .. SDM_FORECAST_MAX_HORIZONS, or no horizons");
  for (int k = 0; k < n_horizons; ++k)
    if (!std::isfinite(horizons[k]) || !(horizons[k] > 0.f) || (k > 0 && !(horizons[k] > horizons[k - 1])))
      return LAYER_REFUSE(what, "horizons must be finite, > 0 and strictly ascending");
  std::vector<int32_t> order((size_t)n_motions);
  for (int32_t i = 0; i < n_motions; ++i) {
    const sdm_motion &mo = motions[i];
    if (mo.track == 0 || (max_track >= 0 && (int)mo.track > max_track)) return LAYER_REFUSE(what, "track 0 or a track above max_movable_track");
    if (mo.pad != 0) return LAYER_REFUSE(what, "sdm_motion.pad != 0");
    if (!std::isfinite(mo.v[0]) || !std::isfinite(mo.v[1]) || !std::isfinite(mo.v[2])) return LAYER_REFUSE(what, "a velocity is not finite");
    order[(size_t)i] = i;
  }
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return motions[a].track < motions[b].track; });
  for (int32_t i = 1; i < n_motions; ++i)
    if (motions[order[(size_t)i]].track == motions[order[(size_t)i - 1]].track) return LAYER_REFUSE(what, "a track appears twice");
  const bool swept = (flags & SDM_FORECAST_SWEPT) != 0;
  int64_t n = 0;
  for (int32_t i = 0; i < n_motions; ++i) {
    const sdm_motion &mo = motions[order[(size_t)i]];
    int p[3] = {0, 0, 0};
    for (int k = 0; k < n_horizons; ++k) {
      int q[3];
      for (int a = 0; a < 3; ++a) {
        const double s = std::nearbyint(((double)mo.v[a] * (double)horizons[k]) / (double)voxel_size);  // (ties to even)
        q[a] = (int)std::min(std::max(s, -1024.0), 1024.0);
      }
      const int D[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
      const int J = swept ? std::max(std::abs(D[0]), std::max(std::abs(D[1]), std::abs(D[2]))) : 0;
      if (J == 0) {
        if (n < limit) emit(mo.track, k, q);
        ++n;
      } else if (n >= limit) {
        n += J;
      } else {
        for (int j = 1; j <= J; ++j, ++n) {
          if (n >= limit) continue;
          int e[3];
          for (int a = 0; a < 3; ++a) e[a] = p[a] + (D[a] > 0 ? 1 : D[a] < 0 ? -1 : 0) * ((2 * j * std::abs(D[a]) + J) / (2 * J));
          emit(mo.track, k, e);
        }
      }
      for (int a = 0; a < 3; ++a) p[a] = q[a];
    }
  }
  *n_out = n;
  if (n > SDM_FORECAST_MAX_STAMPS) {
    char msg[160];
    std::snprintf(msg, sizeof(msg), "%lld stamps, one build takes %d: fewer motions or horizons, or a build without SDM_FORECAST_SWEPT", (long long)n,
                  SDM_FORECAST_MAX_STAMPS);
    set_error(what, __FILE__, __LINE__, msg);
    return SDM_ERR_CAPACITY;
  }
  return SDM_OK;
}

// words of the build's table: the set, the offsets of tracks 0 .. max_track + 1, the stamps
struct TableLayout {
  size_t off, stamps, total;
};
TableLayout table_layout(uint32_t max_track) {
  TableLayout l;
  l.off = SET_WORDS;
  l.stamps = (l.off + max_track + 2u + 1u) & ~(size_t)1;  // (8-byte aligned)
  l.total = l.stamps + 2 * (size_t)SDM_FORECAST_MAX_STAMPS;
  return l;
}
uint32_t max_track_of(const sdm_map *m) { return (uint32_t)std::min(std::max(m->cfg.max_movable_track, 0), 65535); }

Field field_of(const sdm_map *m) {
  Field g;
  g.mask = m->forecast.mask;
  g.first = m->forecast.first;
  g.n_h = (int)m->forecast.n_horizons;
  for (int k = 0; k < SDM_FORECAST_MAX_HORIZONS; ++k) g.t[k] = k < g.n_h ? m->forecast.t[k] : INFINITY;
  return g;
}
}  // namespace

extern "C" {

sdm_status sdm_forecast_stamps(float voxel_size, const sdm_motion *motions, int32_t n_motions, const float *horizons, int32_t n_horizons,
                               uint32_t flags, sdm_forecast_stamp *out, int64_t cap, int64_t *n_out) {
  if (!n_out || cap < 0 || (cap > 0 && !out)) return LAYER_REFUSE("sdm_forecast_stamps", "no n_out, cap < 0, or no out for cap > 0");
  int64_t at = 0;
  return expand("sdm_forecast_stamps", voxel_size, motions, n_motions, horizons, n_horizons, flags, -1, cap, n_out,
                [&](uint16_t track, int k, const int (&e)[3]) {
                  sdm_forecast_stamp s;
                  s.track = track;
                  s.horizon = (uint8_t)k;
                  s.pad = 0;
                  for (int a = 0; a < 3; ++a) s.d[a] = (int16_t)e[a];
                  s.pad2 = 0;
                  out[at++] = s;
                });
}

sdm_status sdm_forecast_update(sdm_map *m, const sdm_motion *motions, int32_t n_motions, const float *horizons, int32_t n_horizons,
                               uint32_t flags) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_forecast_update", nullptr, FORECAST));
  // the stamps, before anything is enqueued: a refusal leaves the last build as it is
  const uint32_t max_track = max_track_of(m);
  const TableLayout l = table_layout(max_track);
  std::vector<uint32_t> per_track((size_t)max_track + 2, 0u);
  std::vector<uint2> stamps;
  std::vector<uint16_t> tracks;
  int64_t n_stamps = 0;
  SDM_TRY(expand("sdm_forecast_update", m->d.voxel_size, motions, n_motions, horizons, n_horizons, flags, (int)max_track, SDM_FORECAST_MAX_STAMPS,
                 &n_stamps, [&](uint16_t track, int k, const int (&e)[3]) {
                   if (tracks.empty() || tracks.back() != track) tracks.push_back(track);
                   ++per_track[track];
                   stamps.push_back(make_uint2((uint32_t)(e[0] + SHIFT_MAX) | ((uint32_t)(e[1] + SHIFT_MAX) << 12) | ((uint32_t)k << 24),
                                               (uint32_t)(e[2] + SHIFT_MAX)));
                 }));
  HIP_TRY(hipSetDevice(m->device));
  const Dims &d = m->d;
  ForecastLayer &L = m->forecast;
  if (!L.mask) SDM_TRY(alloc_tracked(m, &L.mask, d.V));
  if (!L.first) SDM_TRY(alloc_tracked(m, &L.first, d.V));
  if (!L.table) SDM_TRY(alloc_tracked(m, &L.table, l.total));
  const int side = L.table_next;  // builds fill the two page-locked copies in turn
  L.table_next ^= 1;
  if (!L.h_table[side]) SDM_TRY(alloc_tracked(m, &L.h_table[side], l.total, true));
  if (!L.meta) SDM_TRY(alloc_tracked(m, &L.meta, META_WORDS));
  if (!L.h_meta) SDM_TRY(alloc_tracked(m, &L.h_meta, META_WORDS, true));
  if (!L.ev_table[side])
    SDM_TRY(new_event(m, &L.ev_table[side], hipEventDisableTiming));
  else
    HIP_TRY(hipEventSynchronize(L.ev_table[side]));  // the upload of the build before the last has left this copy: no wait in the steady state
  L.valid = false;  // (until this build is enqueued whole)
  uint32_t *h = L.h_table[side];
  memset(h, 0, SET_WORDS * sizeof(uint32_t));
  for (uint16_t t : tracks) h[t >> 5] |= 1u << (t & 31u);
  uint32_t at = 0;
  for (uint32_t t = 0; t <= max_track + 1u; ++t) {
    h[l.off + t] = at;
    at += per_track[t];
  }
  if (!stamps.empty()) memcpy(h + l.stamps, stamps.data(), stamps.size() * sizeof(uint2));
  hipStream_t s = m->stream;
  HIP_TRY(hipMemcpyAsync(L.table, h, (l.stamps + 2 * stamps.size()) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(L.ev_table[side], s));
  HIP_TRY(hipMemsetAsync(L.meta, 0, META_WORDS * sizeof(u64), s));
  const Frame f = m->f;
  const uint32_t nw = d.V >> 6;
  const uint32_t by_word = (nw + FC_WAVES * FC_U - 1) / (FC_WAVES * FC_U);
  const uint2 *res = reinterpret_cast<const uint2 *>(m->st.res);
  hipLaunchKernelGGL(k_forecast_classify, dim3(by_word), dim3(FC_TPB), 0, s, d, f, res, (const uint32_t *)L.table, L.mask, L.first, L.meta, nw);
  HIP_TRY(hipGetLastError());
  if (!stamps.empty()) {
    Table tb;
    tb.set = L.table;
    tb.off = L.table + l.off;
    tb.stamps = reinterpret_cast<const uint2 *>(L.table + l.stamps);
    hipLaunchKernelGGL(k_forecast_scatter, dim3(by_word), dim3(FC_TPB), 0, s, d, f, res, tb, L.mask, L.first, L.meta, nw);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_forecast_reduce, dim3(std::min<uint32_t>(FR_GRID, (nw + FC_WAVES - 1) / FC_WAVES)), dim3(FC_TPB), 0, s,
                       (const uint32_t *)L.mask, L.meta, nw);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(L.h_meta, L.meta, META_WORDS * sizeof(u64), hipMemcpyDeviceToHost, s));
  for (int k = 0; k < SDM_FORECAST_MAX_HORIZONS; ++k) L.t[k] = k < n_horizons ? horizons[k] : 0.f;
  L.n_motions = (uint32_t)n_motions;
  L.n_horizons = (uint32_t)n_horizons;
  L.n_stamps = (uint32_t)n_stamps;
  L.built(f, flags);
  return SDM_OK;
}

sdm_status sdm_get_forecast(sdm_map *m, uint32_t *mask, uint32_t *first, sdm_forecast_info *info, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_get_forecast", &m->forecast, FORECAST));
  HIP_TRY(hipSetDevice(m->device));
  const ForecastLayer &L = m->forecast;
  if (mask) HIP_TRY(hipMemcpyAsync(mask, L.mask, (size_t)m->d.V * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  if (first) HIP_TRY(hipMemcpyAsync(first, L.first, (size_t)m->d.V * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (info) {
    const u64 *h = L.h_meta;  // (the last build's: its copy has landed)
    info->n_motions = L.n_motions;
    info->n_horizons = L.n_horizons;
    info->n_stamps = L.n_stamps;
    info->flags = L.flags;
    info->n_sources = (uint32_t)h[M_SOURCES];
    info->n_marked = (uint32_t)h[M_MARKED];
    info->n_marks_in = h[M_IN];
    info->n_marks_out = h[M_OUT];
  }
  layer_origin(m, L, origin);
  return SDM_OK;
}

sdm_status sdm_get_forecast_cells(sdm_map *m, uint32_t *cell, uint32_t *mask, uint32_t *first, int64_t cap, int64_t *n_out) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (cap < 0 || !n_out) return LAYER_REFUSE("sdm_get_forecast_cells", "cap < 0 or no n_out");
  SDM_TRY(layer_check(m, "sdm_get_forecast_cells", &m->forecast, FORECAST));
  HIP_TRY(hipSetDevice(m->device));
  ForecastLayer &L = m->forecast;
  hipStream_t s = m->stream;
  HIP_TRY(hipStreamSynchronize(s));
  const u64 n = L.h_meta[M_MARKED];
  *n_out = (int64_t)n;
  const size_t take = (size_t)std::min<u64>(n, (u64)cap);
  if (!take || !(cell || mask || first)) return SDM_OK;
  const uint32_t nw = m->d.V >> 6;
  if (!L.pre) SDM_TRY(alloc_tracked(m, &L.pre, nw));
  uint32_t *scan = nullptr;
  SDM_TRY(layer_scan_scratch(m, nw, &scan));
  DevTemps tmp;
  uint32_t *d_out[3] = {nullptr, nullptr, nullptr};
  uint32_t *const host[3] = {cell, mask, first};
  for (int k = 0; k < 3; ++k)
    if (host[k]) HIP_TRY(tmp.alloc(&d_out[k], take));
  const uint32_t by_chunk = (nw + FC_WAVES - 1) / FC_WAVES;
  hipLaunchKernelGGL(k_forecast_cells_count, dim3(by_chunk), dim3(FC_TPB), 0, s, (const uint32_t *)L.mask, L.pre, nw);
  HIP_TRY(hipGetLastError());
  exclusive_scan_u32(L.pre, L.pre, nw, scan, s);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_forecast_cells_write, dim3(by_chunk), dim3(FC_TPB), 0, s, (const uint32_t *)L.mask, (const uint32_t *)L.first,
                     (const uint32_t *)L.pre, nw, (uint32_t)take, d_out[0], d_out[1], d_out[2]);
  HIP_TRY(hipGetLastError());
  for (int k = 0; k < 3; ++k)
    if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], d_out[k], take * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SDM_OK;
}

sdm_status sdm_query_forecast(sdm_map *m, const float *xyzt, int64_t n, sdm_forecast_result *out, uint32_t flags) {
  SDM_TRY(query_check(m, xyzt, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_forecast"));
  SDM_TRY(layer_check(m, "sdm_query_forecast", &m->forecast, FORECAST));
  const Frame f = m->forecast.f;
  const Field g = field_of(m);
  return run_query(m, xyzt, 16, out, sizeof(sdm_forecast_result), nullptr, 0, n, flags,
                   [m, f, g](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_forecast, dim3((c + FQ_TPB - 1) / FQ_TPB), dim3(FQ_TPB), 0, s, m->d, f, g,
                                        static_cast<const float *>(in), c, static_cast<uint2 *>(o));
                   });
}

sdm_status sdm_query_forecast_segments(sdm_map *m, const float *seg, int64_t n, sdm_forecast_hit *out, uint32_t flags) {
  SDM_TRY(query_check(m, seg, n, out, flags, SDM_QUERY_ON_DEVICE | SDM_QUERY_UNKNOWN_BLOCKS | SDM_FORECAST_VACATED_BLOCKS,
                      "sdm_query_forecast_segments"));
  SDM_TRY(layer_check(m, "sdm_query_forecast_segments", &m->forecast, FORECAST));
  const Frame f = m->forecast.f;
  const Field g = field_of(m);
  const int unknown_blocks = (flags & SDM_QUERY_UNKNOWN_BLOCKS) ? 1 : 0, vacated_blocks = (flags & SDM_FORECAST_VACATED_BLOCKS) ? 1 : 0;
  return run_query(m, seg, 32, out, sizeof(sdm_forecast_hit), nullptr, 0, n, flags,
                   [m, f, g, unknown_blocks, vacated_blocks](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     hipLaunchKernelGGL(k_query_forecast_segments, dim3((c + FQ_TPB - 1) / FQ_TPB), dim3(FQ_TPB), 0, s, m->d, f, g,
                                        static_cast<const float *>(in), c, static_cast<sdm_forecast_hit *>(o), unknown_blocks, vacated_blocks);
                   });
}

}  // extern "C"
