// esdf.hip — the map's Euclidean distance field and its distance query (gfx950; include/sdm.h, "batched map queries").
//
// The field is an exact squared Euclidean distance transform over the whole map block, in cells, built by three 1-D
// passes over lines of one axis each, in place on one array: site[c] = the map-index cell (x | y << x_n | z << (x_n+y_n))
// of a nearest obstacle of cell c, INVALID_INDEX if the field has none.  d2 is never stored: it is |c - site[c]|^2.
//   k_esdf_x    one wave per x line: reads the line's results through the ring correction (so everything after it is in
//               map-index order and the ring's wrap point is not a neighbour relation), writes the snapshot word of every
//               cell and the nearest obstacle on the line (ballots: the line's obstacle mask sits in scalar registers).
//   k_esdf_env  one lane per y (or z) line, the lanes of a wave on adjacent x, so each step of a line is one coalesced
//               row: the lower envelope of the parabolas f(q) + (p - q)^2 (Felzenszwalb-Huttenlocher), f(q) = the
//               squared distance of cell q to its site across the axes already done.  A lane's stack of envelope
//               vertices lives in LDS, lane-interleaved; a vertex is one word (its position and the two site
//               coordinates f depends on), so f is recomputed exactly and the winner's site is carried along without
//               touching memory again: the line is read once, then written once.
// All breakpoint tests are integer cross-multiplications: f + q^2 < 2^20 + 2^18 and positions < 2^9, so every product
// fits in 31 bits.
// The distance query reads the field and the snapshot only, never State: the field answers for the frame it was built
// from until the next build.
#include "sdm_layer.h"
#include "sdm_map.h"

#pragma clang fp contract(off)

static_assert(sizeof(sdm_distance_result) == 36, "sdm.h layout");

namespace sdm {

namespace {

constexpr int EX_TPB = 256;      // k_esdf_x: four lines per workgroup
constexpr int EX_CHUNKS = 8;     // NX <= 512 = 8 x 64
constexpr int ENV_U = 32;        // k_esdf_env: rows loaded together (8 measured the same: DESIGN.md 5c)
constexpr int ENV_NONE = 1 << 20;
constexpr int QTPB = 256;
constexpr LayerName ESDF = {"the distance field", "distance field", "sdm_esdf_update", false};

__device__ __forceinline__ bool esdf_obstacle(uint32_t w1, uint32_t flags, int max_movable) {
  const int occ = (int8_t)(w1 >> 24);  // (not occ_of: the kernels' registers stay as they were)
  const int track = (int)(w1 & 0xffffu);
  const bool obst = occ >= 1 || ((flags & SDM_ESDF_UNKNOWN_IS_OBSTACLE) && occ == -1);
  const bool movable = (flags & SDM_ESDF_STATIC_ONLY) && track >= 1 && track <= max_movable;
  return obst && !movable;
}

// ---- pass x --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EX_TPB) void k_esdf_x(Dims d, Frame f, const uint2 *__restrict__ res, uint32_t *__restrict__ site,
                                                   uint32_t *__restrict__ snap, uint32_t flags) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t line = blockIdx.x * (EX_TPB / 64) + (threadIdx.x >> 6);
  if (line >= d.NY * d.NZ) return;  // (whole waves: no barrier below)
  const uint32_t y = line & (d.NY - 1), z = line >> d.y_n;
  const uint32_t ry = axis_correct((int)y + f.eq[1], d.NY), rz = axis_correct((int)z + f.eq[2], d.NZ);
  const uint32_t nc = (d.NX + 63u) >> 6;
  const size_t row = (size_t)line << d.x_n;
  uint32_t w[EX_CHUNKS];
#pragma unroll
  for (int c = 0; c < EX_CHUNKS; ++c) {  // every load of the line first
    const uint32_t x = (uint32_t)c * 64u + lane;
    w[c] = 0u;
    if ((uint32_t)c < nc && x < d.NX) w[c] = res[ring_to_voxel(d, axis_correct((int)x + f.eq[0], d.NX), ry, rz)].y;
  }
  unsigned long long m[EX_CHUNKS];
#pragma unroll
  for (int c = 0; c < EX_CHUNKS; ++c) {
    const uint32_t x = (uint32_t)c * 64u + lane;
    const bool in = (uint32_t)c < nc && x < d.NX;
    m[c] = __ballot(in && esdf_obstacle(w[c], flags, d.max_movable));
    if (in) snap[row + x] = w[c];
  }
  // nearest obstacle at or left of each cell (a running "last one before this chunk"), then at or right of it
  int left[EX_CHUNKS], right[EX_CHUNKS];
  int before = -ENV_NONE, after = ENV_NONE;
  const unsigned long long upto = (2ull << lane) - 1ull, from = ~0ull << lane;  // bits <= lane, bits >= lane
#pragma unroll
  for (int c = 0; c < EX_CHUNKS; ++c) {
    const unsigned long long lm = m[c] & upto;
    left[c] = lm ? c * 64 + 63 - __builtin_clzll(lm) : before;
    if (m[c]) before = c * 64 + 63 - __builtin_clzll(m[c]);
  }
#pragma unroll
  for (int c = EX_CHUNKS - 1; c >= 0; --c) {
    const unsigned long long rm = m[c] & from;
    right[c] = rm ? c * 64 + __builtin_ctzll(rm) : after;
    if (m[c]) after = c * 64 + __builtin_ctzll(m[c]);
  }
  const uint32_t yz = (y << d.x_n) | (z << (d.x_n + d.y_n));
#pragma unroll
  for (int c = 0; c < EX_CHUNKS; ++c) {
    const int x = c * 64 + (int)lane;
    if ((uint32_t)c < nc && x < (int)d.NX) {
      const int dl = x - left[c], dr = right[c] - x;  // (>= ENV_NONE - 511 where there is none)
      const int sx = dl <= dr ? left[c] : right[c];
      site[row + x] = min(dl, dr) < ENV_NONE / 2 ? ((uint32_t)sx | yz) : INVALID_INDEX;
    }
  }
}

// ---- passes y and z ------------------------------------------------------------------------------------------------
// Line (x, c) of axis AX: AX = 1 runs along y at z = c, AX = 2 along z at y = c.  A vertex word holds q | sx << 9 |
// o << 18, o the site coordinate on the line's other axis (z for AX = 1 - always c there -, y for AX = 2).
template <int AX>
__device__ __forceinline__ int env_f(uint32_t e, int x, int c) {
  const int dx = x - (int)((e >> 9) & 511u), dc = c - (int)(e >> 18);
  return dx * dx + dc * dc;
}

template <int AX>
__global__ __launch_bounds__(64) void k_esdf_env(Dims d, uint32_t *__restrict__ site) {
  extern __shared__ uint32_t env[];  // [vertex][lane]
  const uint32_t lane = threadIdx.x;
  const uint32_t N = AX == 1 ? d.NY : d.NZ, other = AX == 1 ? d.NZ : d.NY;
  const uint32_t g = blockIdx.x * 64u + lane;
  if (g >= d.NX * other) return;  // (no barrier below)
  const int x = (int)(g & (d.NX - 1)), c = (int)(g >> d.x_n);
  const size_t stride = AX == 1 ? (size_t)d.NX : (size_t)d.NX * d.NY;
  const size_t base = (size_t)x + (AX == 1 ? ((size_t)c << (d.x_n + d.y_n)) : ((size_t)c << d.x_n));
  const uint32_t xmask = d.NX - 1, ymask = d.NY - 1;
  // build the envelope, q ascending; the bottom vertex is never popped (its breakpoint is -infinity)
  int cnt = 0, top_q = 0, top_F = 0;
  for (uint32_t q0 = 0; q0 < N; q0 += ENV_U) {
    uint32_t s[ENV_U];
#pragma unroll
    for (int j = 0; j < ENV_U; ++j) s[j] = q0 + j < N ? site[base + (size_t)(q0 + j) * stride] : INVALID_INDEX;
#pragma unroll
    for (int j = 0; j < ENV_U; ++j) {
      if (s[j] == INVALID_INDEX) continue;
      const int q = (int)q0 + j;
      const uint32_t sx = s[j] & xmask, so = AX == 1 ? (s[j] >> (d.x_n + d.y_n)) : ((s[j] >> d.x_n) & ymask);
      const uint32_t e = (uint32_t)q | (sx << 9) | (so << 18);
      const int Fq = env_f<AX>(e, x, c) + q * q;
      while (cnt >= 2) {
        // pop the top v (below it u) if the parabola of q overtakes v's no later than v overtakes u:
        // (Fq - Fv) / 2(q - v) <= (Fv - Fu) / 2(v - u), with q > v > u
        const uint32_t eu = env[(cnt - 2) * 64 + lane];
        const int qu = (int)(eu & 511u), Fu = env_f<AX>(eu, x, c) + qu * qu;
        if ((Fq - top_F) * (top_q - qu) > (top_F - Fu) * (q - top_q)) break;
        --cnt;
        top_q = qu;
        top_F = Fu;
      }
      env[cnt * 64 + lane] = e;
      ++cnt;
      top_q = q;
      top_F = Fq;
    }
  }
  // read it off, q ascending: the next vertex takes over where its parabola is no higher
  uint32_t cur = cnt ? env[lane] : 0u, nxt = cnt > 1 ? env[64 + lane] : 0u;
  int k = 0;
  for (uint32_t q = 0; q < N; ++q) {
    uint32_t out = INVALID_INDEX;
    if (cnt) {
      while (k + 1 < cnt) {
        const int qc = (int)(cur & 511u), qn = (int)(nxt & 511u);
        const int vc = env_f<AX>(cur, x, c) + ((int)q - qc) * ((int)q - qc);
        const int vn = env_f<AX>(nxt, x, c) + ((int)q - qn) * ((int)q - qn);
        if (vn > vc) break;
        ++k;
        cur = nxt;
        nxt = k + 1 < cnt ? env[(k + 1) * 64 + lane] : 0u;
      }
      const uint32_t vq = cur & 511u, vx = (cur >> 9) & 511u, vo = cur >> 18;
      out = AX == 1 ? (vx | (vq << d.x_n) | ((uint32_t)c << (d.x_n + d.y_n))) : (vx | (vo << d.x_n) | (vq << (d.x_n + d.y_n)));
    }
    site[base + (size_t)q * stride] = out;
  }
}

// ---- the distance query: one lane per point ------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cell_d2(const Dims &d, int cx, int cy, int cz, uint32_t s) {
  int sx, sy, sz;
  cell_xyz(d, s, sx, sy, sz);
  const int dx = cx - sx, dy = cy - sy, dz = cz - sz;
  return (uint32_t)(dx * dx + dy * dy + dz * dz);
}

__global__ __launch_bounds__(QTPB) void k_query_distance(Dims d, Frame f, const float *__restrict__ xyz, uint32_t n,
                                                         const uint32_t *__restrict__ site, const uint32_t *__restrict__ snap,
                                                         sdm_distance_result *__restrict__ out) {
  const uint32_t i = blockIdx.x * QTPB + threadIdx.x;
  if (i >= n) return;
  const int N[3] = {(int)d.NX, (int)d.NY, (int)d.NZ};
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  float uu[3], t[3];
  int cell[3], c0[3], c1[3];
  const bool ok = point_coords(d, f, p, cell, uu);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float s = uu[a] - 0.5f, i0 = floorf(s);
    t[a] = s - i0;
    c0[a] = min(max((int)i0, 0), N[a] - 1);
    c1[a] = min(max((int)i0 + 1, 0), N[a] - 1);
  }
  auto lin = [&](int x, int y, int z) { return cell_word(d, x, y, z); };
  // the point's cell and the eight corners: nine independent loads (corners differing in x are mostly adjacent words)
  uint32_t sc = INVALID_INDEX, sk[8];
  if (ok) {
    sc = site[lin(cell[0], cell[1], cell[2])];
#pragma unroll
    for (int k = 0; k < 8; ++k) sk[k] = site[lin(k & 1 ? c1[0] : c0[0], k & 2 ? c1[1] : c0[1], k & 4 ? c1[2] : c0[2])];
  }
  sdm_distance_result r;
  if (!ok || sc == INVALID_INDEX) {
    r.distance = -1.f;
    r.gradient[0] = r.gradient[1] = r.gradient[2] = 0.f;
    r.nearest[0] = r.nearest[1] = r.nearest[2] = __builtin_nanf("");
    r.d2 = INVALID_INDEX;
    const uint32_t w = RES_UNKNOWN_W1;
    __builtin_memcpy(&r.track, &w, 4);
  } else {
    const uint32_t w = snap[sc];  // (issued before the arithmetic that does not need it)
    float D[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      D[k] = sqrtf((float)cell_d2(d, k & 1 ? c1[0] : c0[0], k & 2 ? c1[1] : c0[1], k & 4 ? c1[2] : c0[2], sk[k])) * d.voxel_size;
    const float wx[2] = {1.f - t[0], t[0]}, wy[2] = {1.f - t[1], t[1]}, wz[2] = {1.f - t[2], t[2]};
    float v = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
      v += (wx[bx] * wy[by] * wz[bz]) * D[k];
      gx += ((bx ? 1.f : -1.f) * wy[by] * wz[bz]) * D[k];
      gy += ((by ? 1.f : -1.f) * wx[bx] * wz[bz]) * D[k];
      gz += ((bz ? 1.f : -1.f) * wx[bx] * wy[by]) * D[k];
    }
    r.distance = v;
    r.gradient[0] = gx * d.recip;
    r.gradient[1] = gy * d.recip;
    r.gradient[2] = gz * d.recip;
    uint32_t s3[3];
    cell_xyz(d, sc, s3[0], s3[1], s3[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) r.nearest[a] = (f.center[a] + d.pmin[a]) + ((float)s3[a] + 0.5f) * d.voxel_size;
    r.d2 = cell_d2(d, cell[0], cell[1], cell[2], sc);
    __builtin_memcpy(&r.track, &w, 4);
  }
  out[i] = r;
}

}  // namespace

hipError_t launch_esdf_build(const Dims &d, const Frame &f, const State &st, uint32_t flags, uint32_t *site, uint32_t *snap,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_esdf_x, dim3((d.NY * d.NZ + EX_TPB / 64 - 1) / (EX_TPB / 64)), dim3(EX_TPB), 0, s, d, f,
                     reinterpret_cast<const uint2 *>(st.res), site, snap, flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t lds_y = (size_t)d.NY * 64 * 4, lds_z = (size_t)d.NZ * 64 * 4;  // a vertex per cell of the line, worst case
  if (lds_y > 65536) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_esdf_env<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_y);
    if (e != hipSuccess) return e;
  }
  if (lds_z > 65536) {
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_esdf_env<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_z);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_esdf_env<1>, dim3((d.NX * d.NZ + 63) / 64), dim3(64), lds_y, s, d, site);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_esdf_env<2>, dim3((d.NX * d.NY + 63) / 64), dim3(64), lds_z, s, d, site);
  return hipGetLastError();
}

void launch_query_distance(const Dims &d, const Frame &f, const uint32_t *site, const uint32_t *snap, const float *xyz, uint32_t n,
                           sdm_distance_result *out, hipStream_t s) {
  hipLaunchKernelGGL(k_query_distance, dim3((n + QTPB - 1) / QTPB), dim3(QTPB), 0, s, d, f, xyz, n, site, snap, out);
}

}  // namespace sdm

// ---- the host side: the entry points behind include/sdm.h ---------------------------------------------------------
// The build reads the result array in stream order and takes the host Frame of the last issued frame by value, as the
// queries do; the Frame is kept with the field, so that the distance query and sdm_get_esdf answer for that frame.
extern "C" {

sdm_status sdm_esdf_update(sdm_map *m, uint32_t flags) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  if (flags & ~(SDM_ESDF_UNKNOWN_IS_OBSTACLE | SDM_ESDF_STATIC_ONLY)) {
    set_error("sdm_esdf_update", __FILE__, __LINE__, "unknown flag bits");
    return SDM_ERR_INVALID_ARGUMENT;
  }
  SDM_TRY(layer_check(m, "sdm_esdf_update", nullptr, ESDF));
  HIP_TRY(hipSetDevice(m->device));
  if (!m->esdf.site) SDM_TRY(alloc_tracked(m, &m->esdf.site, m->d.V));
  if (!m->esdf.snap) SDM_TRY(alloc_tracked(m, &m->esdf.snap, m->d.V));
  const Frame f = m->f;
  HIP_TRY(launch_esdf_build(m->d, f, m->st, flags, m->esdf.site, m->esdf.snap, m->stream));
  m->esdf.built(f, flags);
  return SDM_OK;
}

sdm_status sdm_get_esdf(sdm_map *m, uint32_t *d2, uint32_t *site, float origin[3]) {
  if (!m) return SDM_ERR_INVALID_ARGUMENT;
  SDM_TRY(layer_check(m, "sdm_get_esdf", &m->esdf, ESDF));
  HIP_TRY(hipSetDevice(m->device));
  const Dims &d = m->d;
  std::vector<uint32_t> own;
  uint32_t *s = site;
  if (d2 && !s) {
    own.resize(d.V);
    s = own.data();
  }
  if (s) HIP_TRY(hipMemcpyAsync(s, m->esdf.site, (size_t)d.V * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
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
  layer_origin(m, m->esdf, origin);
  return SDM_OK;
}

sdm_status sdm_query_distance(sdm_map *m, const float *xyz, int64_t n, sdm_distance_result *out, uint32_t flags) {
  SDM_TRY(query_check(m, xyz, n, out, flags, SDM_QUERY_ON_DEVICE, "sdm_query_distance"));
  SDM_TRY(layer_check(m, "sdm_query_distance", &m->esdf, ESDF));
  const Frame f = m->esdf.f;
  const uint32_t *site = m->esdf.site, *snap = m->esdf.snap;
  return run_query(m, xyz, 12, out, sizeof(sdm_distance_result), nullptr, 0, n, flags,
                   [m, f, site, snap](const void *in, void *o, void *, uint32_t c, hipStream_t s) {
                     launch_query_distance(m->d, f, site, snap, static_cast<const float *>(in), c, static_cast<sdm_distance_result *>(o), s);
                   });
}

}  // extern "C"
