// lifecycle.hip — host side of libsdm_hip: a map is created, configured and destroyed here; what it owns is released
// here; the host arithmetic of a frame (ring shift, extrinsic, frustum box) and the launch-mode policy live here.
//
// Host work per frame is O(axis length): the ego-centre ring shift of the reference moves no particle
// data, it only stamps the slabs that were recycled (mc_ring/operations.h:68-96, 1111-1191); everything
// else is enqueued on one HIP stream with no host synchronisation inside a frame.
#include <rocrand/rocrand.h>

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "sdm_map.h"

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
// (Round 6: 75 -> 110 us.  The line was drawn when a frame took 0.31 ms on the GPU and the five graphs 0.34; at 0.206 ms
// launch by launch the graphs' frame is 0.26 ms, and a host that measures 76 us - the round's final profile box did, the
// pool's usual 56-73 us - still issues a frame in 0.15 ms, ahead of the GPU.  Launch by launch stops paying where the host
// needs longer than the graphs' frame: about twice the burst figure, 130 us.)
constexpr double GRAPH_PIECES_US = 110.0, GRAPH_CHAIN_US = 170.0;
constexpr int LAUNCHES_PER_FRAME = 50;

__global__ void k_noop() {}

}  // namespace

namespace sdm {

void set_error(const char *what, const char *file, int line, const char *detail) {
  char buf[512];
  snprintf(buf, sizeof(buf), "%s (%s:%d): %s", what, file, line, detail ? detail : "");
  g_last_error = buf;
}

sdm_status map_alloc(sdm_map *m, void **p, size_t bytes, bool pinned) {
  *p = nullptr;
  HIP_TRY(pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes));
  (pinned ? m->pinned : m->allocs).push_back(*p);
  return SDM_OK;
}
void map_release(sdm_map *m, void **p) {
  for (auto *list : {&m->allocs, &m->pinned}) {
    const auto at = std::find(list->begin(), list->end(), *p);
    if (!*p || at == list->end()) continue;
    list->erase(at);
    (void)(list == &m->pinned ? hipHostFree(*p) : hipFree(*p));
  }
  *p = nullptr;
}
sdm_status new_event(sdm_map *m, hipEvent_t *e, unsigned flags) {
  HIP_TRY(hipEventCreateWithFlags(e, flags));
  m->events.push_back(*e);
  return SDM_OK;
}

// mode (SDM_GRAPH, sdm_set_issue_mode): 0 launch by launch, 1 the branched graph, 3 the chain, 4 the pieces, 2 by the host's
// speed at issuing launches as measured at creation (the table above)
void issue_mode_for(const sdm_map *m, int mode, bool *use_graph, int *shape) {
  *use_graph = mode == 2 ? m->enqueue_us > GRAPH_PIECES_US : mode != 0;
  *shape = mode == 1 ? GRAPH_BRANCHED
           : mode == 3 ? GRAPH_CHAIN
           : mode == 2 ? (m->enqueue_us > GRAPH_CHAIN_US ? GRAPH_CHAIN : GRAPH_PIECES)
                       : GRAPH_PIECES;
}

// The map's streams beyond the three every frame uses (main, frustum chain, birth-candidate chain) are created when they
// are first needed - the member-count stream by Z-slab shards, the copy stream by sdm_update_raw with host inputs - and
// the library stays off the null stream: the runtime hands out at most GPU_MAX_HW_QUEUES (4) hardware queues and lets
// further streams share them.  (Measured while looking for the "later maps of a process are slower" of round 3: neither
// this nor keeping the streams of a destroyed map for the next one changed a later map's frame time - that was the
// launch-mode policy, see sdm_create - but a map that uses three queues instead of six leaves the others to its host.)
static hipError_t new_stream(int, hipStream_t *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
static void retire_stream(int, hipStream_t s) {
  if (!s) return;
  (void)hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
}
hipError_t lazy_stream(int device, hipStream_t *s) {
  if (*s) return hipSuccess;
  return new_stream(device, s);
}

// GaussianRandomCalculator::calculateGaussianTable, PDF part (utils/basic_algorithms.h:405-407, 456-460):
// entry i = (1/sqrt(2*(pi/2))) * expf(-x^2/2), x = (i-10000)*0.001.  The quirky normaliser is the reference's.
static void build_pdf_table(std::vector<float> &pdf) {
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

static void build_birth_order(sdm_map *m) {
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

// All six or none: the new set is complete before the old one goes, so a failure leaves the map with the buffers (and
// nb_alloc) it had.
static sdm_status ensure_birth_buffers(sdm_map *m) {
  const size_t hw = (size_t)m->d.W * m->d.H;
  const int nb = std::max(m->flt.nb, 1);
  if (nb <= m->nb_alloc) return SDM_OK;
  const size_t need = hw * nb;
  Scratch &sc = m->sc;
  void **const old[6] = {(void **)&sc.bkey_a, (void **)&sc.bval_a, (void **)&sc.bkey_b, (void **)&sc.bval_b, (void **)&sc.bpos, (void **)&sc.sort_scratch};
  const size_t bytes[6] = {need * 4, need * 4, need * 4, need * 4, need * sizeof(*sc.bpos), sort_scratch_elems(need) * 4};
  void *fresh[6] = {};
  sdm_status rc = SDM_OK;
  HIP_TRY(hipStreamSynchronize(m->stream));
  for (int i = 0; i < 6 && rc == SDM_OK; ++i) rc = map_alloc(m, &fresh[i], bytes[i], false);
  for (int i = 0; i < 6; ++i) {
    map_release(m, rc == SDM_OK ? old[i] : &fresh[i]);
    if (rc == SDM_OK) *old[i] = fresh[i];
  }
  SDM_TRY(rc);
  HIP_TRY(hipMemsetAsync(sc.sort_scratch, 0, sort_scratch_elems(need) * 4, m->stream));  // the one-launch scan's words start at zero
  HIP_TRY(hipStreamSynchronize(m->stream));
  m->nb_alloc = nb;
  m->sort_cap = need;
  return SDM_OK;
}

// updateRingbufferIndexParams (mc_ring/operations.h:1111-1191) + getEquivalentSteps* (:1196-1230)
static void update_ring_index_params(sdm_map *m) {
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

static void host_initialize(sdm_map *m) {
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
  SDM_TRY(sweep_mode_latch(m));
  if (out) *out = c;
  SDM_TRY(exchange_check(m));
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

}  // namespace sdm

extern "C" {

const char *sdm_last_error(void) { return g_last_error.c_str(); }
const char *sdm_version(void) { return "libsdm_hip 0.1 (gfx950)"; }

// everything of sdm_create behind the argument checks; a failure leaves a partly built map that sdm_destroy takes
static sdm_status map_init(sdm_map *m, const sdm_config *cfg, int shard_count) {
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
  for (hipStream_t *s : {&m->own_stream, &m->s_frustum, &m->s_birth}) HIP_TRY(new_stream(cfg->device, s));
  m->stream = m->own_stream;
  for (hipEvent_t *e : {&m->ev_state, &m->ev_counts, &m->ev_begin, &m->ev_frustum, &m->ev_birth, &m->ev_fa, &m->ev_vis, &m->cap_begin,
                        &m->cap_frustum, &m->cap_birth, &m->ev_copy, &m->raw[0].ev_free, &m->raw[1].ev_free})
    SDM_TRY(new_event(m, e, hipEventDisableTiming));
  const size_t n_slots = (size_t)d.v_count * d.S;
  const size_t hw = (size_t)d.W * d.H;
#define A(ptr, n) SDM_TRY(alloc_tracked(m, &(ptr), (n)))
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
  }
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
  A(sc.scan_scratch, scan_need);
  A(sc.scan_scratch_b, scan_need);
  HIP_TRY(hipMemsetAsync(sc.scan_scratch, 0, scan_need * 4, m->stream));
  HIP_TRY(hipMemsetAsync(sc.scan_scratch_b, 0, scan_need * 4, m->stream));
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
  SDM_TRY(ensure_birth_buffers(m));
  for (hipEvent_t &e : m->ev) SDM_TRY(new_event(m, &e, hipEventDefault));
  // RingBufferOperations::initialize (operations.h:726-767)
  host_initialize(m);
  launch_clear(d, m->st, m->stream, true);
  SDM_TRY(upload_stamps(m));
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
    issue_mode_for(m, m->graph_mode, &m->use_graph, &m->graph_shape);
  }
  return SDM_OK;
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
  if (cfg->width >= (1 << ROW_COL_BITS)) {
    set_error("sdm_create", __FILE__, __LINE__, "image width above 4095 (the row kernel of the pixel bins holds one image row in LDS)");
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
  const sdm_status rc = map_init(m, cfg, shard_count);
  if (rc == SDM_OK) *out = m;
  else (void)sdm_destroy(m);  // (the one way out of a create that failed behind this line)
  return rc;
}

sdm_status sdm_destroy(sdm_map *m) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (m->host_timing) {
    const double ng = m->n_graph_frames ? (double)m->n_graph_frames : 1.0, nd = m->n_direct_frames ? (double)m->n_direct_frames : 1.0;
    fprintf(stderr, "sdm host timing: prepare+inputs %.1f us/frame; graph frames %llu: set-params %.1f us, hipGraphLaunch %.1f us; direct frames %llu: %.1f us\n",
            m->t_prepare_us / (ng + nd - ((m->n_graph_frames && m->n_direct_frames) ? 0.0 : 1.0)), (unsigned long long)m->n_graph_frames,
            m->t_setparams_us / ng, m->t_launch_us / ng, (unsigned long long)m->n_direct_frames, m->t_direct_us / nd);
  }
  // (also a map that sdm_create gave up on half-way: whatever it did not get to is null or not in the lists)
  (void)hipSetDevice(m->device);
  for (hipStream_t st : {m->stream, m->s_frustum, m->s_birth, m->s_moves, m->s_copy})
    if (st) (void)hipStreamSynchronize(st);
  exchange_teardown(m);
  drop_graphs(m);
  for (hipEvent_t e : m->events) (void)hipEventDestroy(e);
  for (void *p : m->allocs) (void)hipFree(p);
  for (void *p : m->pinned) (void)hipHostFree(p);
  retire_stream(m->device, m->s_copy);
  retire_stream(m->device, m->s_moves);
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
  const sdm_params before = m->prm;
  m->prm = *p;
  m->sweep_all = true;  // the occupancy threshold may have changed: no stored result is safe
  refresh_filter(m);
  const sdm_status rc = ensure_birth_buffers(m);
  if (rc != SDM_OK) {  // (no room for the births the new parameters ask for: the map keeps the old ones)
    m->prm = before;
    refresh_filter(m);
  }
  return rc;
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

}  // extern "C"
