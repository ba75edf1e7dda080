// debug.hip — development aids and test hooks behind the C ABI: sdm_debug_*, the sweep timer for bench.py's roofline,
// sdm_test_* for the primitives.
#include "sdm_map.h"

namespace {

// Do two streams of a map run side by side?  k_spin holds its stream for `ticks` of the 100 MHz wall clock and leaves the
// clock at its start and end; k_stamp, launched right behind it on another stream, leaves the clock when it runs.
__global__ void k_spin(unsigned long long ticks, unsigned long long *out) {
  const unsigned long long t0 = wall_clock64();
  out[0] = t0;
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
  out[1] = wall_clock64();
}
__global__ void k_stamp(unsigned long long *out) { *out = wall_clock64(); }

}  // namespace

extern "C" {

// Development aid (tools/probes/modes.py): a 60 us spin on the main stream, a stamp right behind it on side stream
// `which` (0 frustum, 1 birth candidates, 2 member count).  out_us[0] = stamp - spin start, out_us[1] = spin length.
sdm_status sdm_debug_overlap(sdm_map *m, int32_t which, double out_us[2]) {
  if (!m || which < 0 || which > 2 || !out_us) return SDM_ERR_INVALID_ARGUMENT;
  HIP_TRY(hipSetDevice(m->device));
  unsigned long long *d = nullptr, h[3] = {0, 0, 0};
  DevTemps tmp;
  HIP_TRY(tmp.alloc(&d, 3));
  if (which == 2) HIP_TRY(lazy_stream(m->device, &m->s_moves));
  hipStream_t side = which == 0 ? m->s_frustum : (which == 1 ? m->s_birth : m->s_moves);
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipStreamSynchronize(side));
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, m->stream, 6000ull, d);
  hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, side, d + 2);
  HIP_TRY(hipStreamSynchronize(m->stream));
  HIP_TRY(hipStreamSynchronize(side));
  HIP_TRY(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  out_us[0] = ((double)h[2] - (double)h[0]) / 100.0;
  out_us[1] = ((double)h[1] - (double)h[0]) / 100.0;
  return SDM_OK;
}

sdm_status sdm_debug_force_generic_flood(sdm_map *m, int32_t on) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  m->force_generic_flood = on ? 1 : 0;
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
  SDM_TRY(sweep_mode_latch(m));
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
  SDM_TRY(sweep_mode_latch(m));
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

// ---- unit-test hooks for the primitives -------------------------------------------------------
sdm_status sdm_test_scan(const uint32_t *in, uint32_t *out, int64_t n) {
  if (!in || !out || n <= 0) return SDM_ERR_INVALID_ARGUMENT;
  uint32_t *din, *dout, *scr;
  DevTemps tmp;
  HIP_TRY(tmp.alloc(&din, (size_t)n));
  HIP_TRY(tmp.alloc(&dout, (size_t)n));
  HIP_TRY(tmp.alloc(&scr, scan_scratch_elems((size_t)n)));
  HIP_TRY(hipMemset(scr, 0, scan_scratch_elems((size_t)n) * 4));
  HIP_TRY(hipMemcpy(din, in, (size_t)n * 4, hipMemcpyHostToDevice));
  exclusive_scan_u32(din, dout, (size_t)n, scr, nullptr);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
  return SDM_OK;
}

sdm_status sdm_test_sort_pairs(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out, uint32_t *vals_out,
                               int64_t n, int32_t nbits) {
  if (!keys_in || !vals_in || !keys_out || !vals_out || n <= 0 || nbits <= 0 || nbits > 32) return SDM_ERR_INVALID_ARGUMENT;
  uint32_t *ka, *va, *kb, *vb, *scr;
  DevTemps tmp;
  HIP_TRY(tmp.alloc(&ka, (size_t)n));
  HIP_TRY(tmp.alloc(&va, (size_t)n));
  HIP_TRY(tmp.alloc(&kb, (size_t)n));
  HIP_TRY(tmp.alloc(&vb, (size_t)n));
  HIP_TRY(tmp.alloc(&scr, sort_scratch_elems((size_t)n)));
  HIP_TRY(hipMemset(scr, 0, sort_scratch_elems((size_t)n) * 4));
  HIP_TRY(hipMemcpy(ka, keys_in, (size_t)n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(va, vals_in, (size_t)n * 4, hipMemcpyHostToDevice));
  int which = radix_sort_pairs(ka, va, kb, vb, (size_t)n, nbits, scr, nullptr);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(keys_out, which ? kb : ka, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(vals_out, which ? vb : va, (size_t)n * 4, hipMemcpyDeviceToHost));
  return SDM_OK;
}

// ---- the same two through their whole contract (sdm.h): a sequence of calls on one scratch without slack --------------
}  // extern "C"
namespace {

constexpr uint32_t SEQ_CANARY = 0xC0FFEE5Au;
constexpr size_t SEQ_MAX_WORDS = (size_t)1 << 28;  // all slices of one array together: 1 GiB

// the slices of a sequence: capacities > 0; counts <= capacity unless they are read on the device, where any uint32 goes
bool seq_layout(int32_t n_calls, const int64_t *capacity, const int64_t *count, bool on_device, std::vector<size_t> *first,
                size_t *total, size_t *longest) {
  if (n_calls <= 0 || !capacity || !count) return false;
  *total = *longest = 0;
  first->clear();
  for (int32_t i = 0; i < n_calls; ++i) {
    if (capacity[i] <= 0 || (size_t)capacity[i] > SEQ_MAX_WORDS || count[i] < 0 || count[i] > 0xffffffffll) return false;
    if (!on_device && count[i] > capacity[i]) return false;
    first->push_back(*total);
    *total += (size_t)capacity[i];
    *longest = std::max(*longest, (size_t)capacity[i]);
  }
  return *total <= SEQ_MAX_WORDS;
}

// the scratch of a sequence: exactly n words, zero, and SDM_TEST_GUARD_WORDS of the canary right behind them
hipError_t seq_scratch(DevTemps &tmp, size_t n, uint32_t **scr) {
  std::vector<uint32_t> h(n + SDM_TEST_GUARD_WORDS, 0u);
  std::fill(h.begin() + n, h.end(), SEQ_CANARY);
  hipError_t e = tmp.alloc(scr, h.size());
  if (e == hipSuccess) e = hipMemcpy(*scr, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  return e;
}
hipError_t seq_scratch_read(const uint32_t *scr, size_t n, int32_t *guard_ok, uint32_t *scratch_out) {
  uint32_t g[SDM_TEST_GUARD_WORDS];
  hipError_t e = hipMemcpy(g, scr + n, sizeof(g), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  *guard_ok = 1;
  for (uint32_t w : g)
    if (w != SEQ_CANARY) *guard_ok = 0;
  if (scratch_out) e = hipMemcpy(scratch_out, scr, n * 4, hipMemcpyDeviceToHost);
  return e;
}
hipError_t seq_counts(DevTemps &tmp, int32_t n_calls, const int64_t *count, uint32_t **dcount) {
  std::vector<uint32_t> h(n_calls);
  for (int32_t i = 0; i < n_calls; ++i) h[i] = (uint32_t)count[i];
  hipError_t e = tmp.alloc(dcount, h.size());
  if (e == hipSuccess) e = hipMemcpy(*dcount, h.data(), h.size() * 4, hipMemcpyHostToDevice);
  return e;
}

}  // namespace
extern "C" {

sdm_status sdm_test_scratch_elems(int32_t sort, int64_t n, int64_t *elems) {
  if (n <= 0 || !elems) return SDM_ERR_INVALID_ARGUMENT;
  *elems = (int64_t)(sort ? sort_scratch_elems((size_t)n) : scan_scratch_elems((size_t)n));
  return SDM_OK;
}

sdm_status sdm_test_scan_seq(int32_t n_calls, const int64_t *capacity, const int64_t *count, uint32_t flags, const uint32_t *in,
                             uint32_t *out, int32_t *guard_ok, uint32_t *scratch_out) {
  if (!in || !out || !guard_ok || (flags & ~(SDM_TEST_IN_PLACE | SDM_TEST_COUNT_ON_DEVICE))) return SDM_ERR_INVALID_ARGUMENT;
  const bool on_device = flags & SDM_TEST_COUNT_ON_DEVICE, in_place = flags & SDM_TEST_IN_PLACE;
  std::vector<size_t> first;
  size_t total, longest;
  if (!seq_layout(n_calls, capacity, count, on_device, &first, &total, &longest)) return SDM_ERR_INVALID_ARGUMENT;
  const size_t scr_n = scan_scratch_elems(longest);
  uint32_t *din, *dout, *scr, *dcount;
  DevTemps tmp;
  HIP_TRY(tmp.alloc(&din, total));
  HIP_TRY(hipMemcpy(din, in, total * 4, hipMemcpyHostToDevice));
  if (in_place) {
    dout = din;
  } else {
    HIP_TRY(tmp.alloc(&dout, total));
    HIP_TRY(hipMemcpy(dout, out, total * 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(seq_scratch(tmp, scr_n, &scr));
  HIP_TRY(seq_counts(tmp, n_calls, count, &dcount));
  for (int32_t i = 0; i < n_calls; ++i)
    exclusive_scan_u32(din + first[i], dout + first[i], on_device ? (size_t)capacity[i] : (size_t)count[i], scr, nullptr,
                       on_device ? dcount + i : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, dout, total * 4, hipMemcpyDeviceToHost));
  HIP_TRY(seq_scratch_read(scr, scr_n, guard_ok, scratch_out));
  return SDM_OK;
}

sdm_status sdm_test_sort_pairs_seq(int32_t n_calls, const int64_t *capacity, const int64_t *count, const int32_t *nbits,
                                   uint32_t flags, const uint32_t *keys_in, const uint32_t *vals_in, uint32_t *keys_out,
                                   uint32_t *vals_out, int32_t *which, int32_t *guard_ok, uint32_t *scratch_out) {
  if (!nbits || !keys_in || !vals_in || !keys_out || !vals_out || !which || !guard_ok || (flags & ~SDM_TEST_COUNT_ON_DEVICE))
    return SDM_ERR_INVALID_ARGUMENT;
  const bool on_device = flags & SDM_TEST_COUNT_ON_DEVICE;
  std::vector<size_t> first;
  size_t total, longest;
  if (!seq_layout(n_calls, capacity, count, on_device, &first, &total, &longest)) return SDM_ERR_INVALID_ARGUMENT;
  for (int32_t i = 0; i < n_calls; ++i)
    if (nbits[i] <= 0 || nbits[i] > 32) return SDM_ERR_INVALID_ARGUMENT;
  const size_t scr_n = sort_scratch_elems(longest);
  uint32_t *ka, *va, *kb, *vb, *scr, *dcount;
  DevTemps tmp;
  HIP_TRY(tmp.alloc(&ka, total));
  HIP_TRY(tmp.alloc(&va, total));
  HIP_TRY(tmp.alloc(&kb, total));
  HIP_TRY(tmp.alloc(&vb, total));
  HIP_TRY(hipMemcpy(ka, keys_in, total * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(va, vals_in, total * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(kb, keys_out, total * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(vb, vals_out, total * 4, hipMemcpyHostToDevice));
  HIP_TRY(seq_scratch(tmp, scr_n, &scr));
  HIP_TRY(seq_counts(tmp, n_calls, count, &dcount));
  for (int32_t i = 0; i < n_calls; ++i)
    which[i] = radix_sort_pairs(ka + first[i], va + first[i], kb + first[i], vb + first[i],
                                on_device ? (size_t)capacity[i] : (size_t)count[i], nbits[i], scr, nullptr,
                                on_device ? dcount + i : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  for (int32_t i = 0; i < n_calls; ++i) {
    HIP_TRY(hipMemcpy(keys_out + first[i], (which[i] ? kb : ka) + first[i], (size_t)capacity[i] * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(vals_out + first[i], (which[i] ? vb : va) + first[i], (size_t)capacity[i] * 4, hipMemcpyDeviceToHost));
  }
  HIP_TRY(seq_scratch_read(scr, scr_n, guard_ok, scratch_out));
  return SDM_OK;
}

}  // extern "C"
