// Measurement probe (not part of the library): the brick-local labelling of the world objects (csrc/world_objects.hip,
// k_wo_label_local) two ways over the same bricks - REG, the library's scheme restated here: one wave a brick, eight keys and
// labels of a column in registers, neighbours by lane shuffles against a mask of equal-key neighbours settled once; LDS: one
// workgroup of 512 threads a brick, a thread per cell, labels in LDS, two barriers a sweep.  Three fills: three labels at
// 30 % density, a full brick of one label, the serpentine of tests/world_objects_cases.py (143 cells in a row).  Prints per
// fill and connectivity both times (HIP events, the median of 5) and whether the two label arrays are equal.
//   hipcc --offload-arch=gfx950 -O3 -Wno-unused-result -o world_objects_label_probe world_objects_label_probe.hip
//   timeout -k 10 120 ./world_objects_label_probe [bricks]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr uint32_t NO_KEY = 0xffffffffu, NO_LABEL = 0xffffu;

__device__ __forceinline__ uint32_t take_label(uint32_t a, uint32_t t, uint32_t eq, int bit) {
  return min(a, t | ~(uint32_t)((int)(eq << (31 - bit)) >> 31));
}

template <bool FACE>
__global__ __launch_bounds__(256) void k_reg(const uint32_t *__restrict__ keys, uint32_t n, uint16_t *__restrict__ out, uint32_t *__restrict__ sweeps) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= n) return;
  const uint32_t *__restrict__ src = keys + (size_t)r * 512u + lane;
  uint32_t k[8], v[8], eq[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) k[z] = src[z * 64];
#pragma unroll
  for (int z = 0; z < 8; ++z) v[z] = k[z] != NO_KEY ? (uint32_t)z * 64u + lane : NO_LABEL, eq[z] = 0u;
  const int cx = (int)(lane & 7u), cy = (int)(lane >> 3);
#pragma unroll 1
  for (int i = 0; i < (FACE ? 4 : 9); ++i) {
    const int d = FACE ? 2 * i + 1 : i, dx = d % 3 - 1, dy = d / 3 - 1;
    const bool inside = cx + dx >= 0 && cx + dx <= 7 && cy + dy >= 0 && cy + dy <= 7;
    const int from = inside ? (int)lane + dx + 8 * dy : (int)lane;
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      const uint32_t got = (uint32_t)__shfl((int)k[z], from, 64), nk = inside ? got : NO_KEY;
#pragma unroll
      for (int dz = FACE ? 0 : -1; dz <= (FACE ? 0 : 1); ++dz) {
        const int c = z - dz;
        if (c < 0 || c > 7) continue;
        eq[c] |= (k[c] != NO_KEY && nk == k[c] ? 1u : 0u) << (d + 9 * (dz + 1));
      }
    }
  }
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    if (FACE && z > 0) eq[z] |= (k[z] != NO_KEY && k[z - 1] == k[z] ? 1u : 0u) << 4;
    if (FACE && z < 7) eq[z] |= (k[z] != NO_KEY && k[z + 1] == k[z] ? 1u : 0u) << 22;
    eq[z] &= ~(1u << 13);
  }
  int sweep = 0;
  for (; sweep < 512; ++sweep) {
    uint32_t a[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) a[z] = v[z];
#pragma unroll 1
    for (int i = 0; i < (FACE ? 4 : 9); ++i) {
      const int d = FACE ? 2 * i + 1 : i, dx = d % 3 - 1, dy = d / 3 - 1;
      const bool inside = cx + dx >= 0 && cx + dx <= 7 && cy + dy >= 0 && cy + dy <= 7;
      const int from = inside ? (int)lane + dx + 8 * dy : (int)lane;
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        const uint32_t t = (uint32_t)__shfl((int)v[z], from, 64);
#pragma unroll
        for (int dz = FACE ? 0 : -1; dz <= (FACE ? 0 : 1); ++dz) {
          const int c = z - dz;
          if (c < 0 || c > 7) continue;
          a[c] = take_label(a[c], t, eq[c], d + 9 * (dz + 1));
        }
      }
    }
    if (FACE) {
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        if (z > 0) a[z] = take_label(a[z], v[z - 1], eq[z], 4);
        if (z < 7) a[z] = take_label(a[z], v[z + 1], eq[z], 22);
      }
    }
    bool changed = false;
#pragma unroll
    for (int z = 0; z < 8; ++z) changed = changed || a[z] != v[z], v[z] = a[z];
    if (!__ballot(changed)) break;
  }
#pragma unroll
  for (int z = 0; z < 8; ++z) out[(size_t)r * 512u + (uint32_t)z * 64u + lane] = (uint16_t)v[z];
  if (lane == 0) sweeps[r] = (uint32_t)sweep;
}

template <bool FACE>
__global__ __launch_bounds__(512) void k_lds(const uint32_t *__restrict__ keys, uint32_t n, uint16_t *__restrict__ out) {
  __shared__ uint32_t s_k[512], s_v[512];
  const uint32_t r = blockIdx.x, c = threadIdx.x;
  const uint32_t k = keys[(size_t)r * 512u + c];
  uint32_t v = k != NO_KEY ? c : NO_LABEL;
  s_k[c] = k, s_v[c] = v;
  __syncthreads();
  const int x = (int)(c & 7u), y = (int)((c >> 3) & 7u), z = (int)(c >> 6);
  uint32_t eq = 0u;
#pragma unroll
  for (int b = 0; b < 27; ++b) {
    const int dx = b % 3 - 1, dy = (b / 3) % 3 - 1, dz = b / 9 - 1;
    if (b == 13 || (FACE && (dx != 0) + (dy != 0) + (dz != 0) != 1)) continue;
    const bool inside = x + dx >= 0 && x + dx <= 7 && y + dy >= 0 && y + dy <= 7 && z + dz >= 0 && z + dz <= 7;
    const uint32_t nk = inside ? s_k[(int)c + dx + 8 * dy + 64 * dz] : NO_KEY;
    eq |= (k != NO_KEY && nk == k ? 1u : 0u) << b;
  }
  for (int sweep = 0; sweep < 512; ++sweep) {
    uint32_t a = v;
#pragma unroll
    for (int b = 0; b < 27; ++b) {
      const int dx = b % 3 - 1, dy = (b / 3) % 3 - 1, dz = b / 9 - 1;
      if (b == 13 || (FACE && (dx != 0) + (dy != 0) + (dz != 0) != 1)) continue;
      if ((eq >> b) & 1u) a = min(a, s_v[(int)c + dx + 8 * dy + 64 * dz]);
    }
    const int changed = __syncthreads_or(a != v);  // (every read of this sweep is done)
    if (!changed) break;
    s_v[c] = v = a;
    __syncthreads();
  }
  out[(size_t)r * 512u + c] = (uint16_t)v;
}

static void fill(std::vector<uint32_t> &keys, uint32_t n, int kind) {
  keys.assign((size_t)n * 512, NO_KEY);
  uint32_t s = 12345u;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t c = 0; c < 512; ++c) {
      uint32_t &k = keys[(size_t)r * 512 + c];
      if (kind == 0) {
        s = s * 1664525u + 1013904223u;
        const uint32_t u = (s >> 8) % 100u;
        k = u < 10 ? 1u : u < 20 ? 2u : u < 30 ? 3u : NO_KEY;
      } else if (kind == 1) {
        k = 1u;
      } else {  // the serpentine: rows along x at even y on even layers, joined at alternating ends
        const uint32_t x = c & 7u, y = (c >> 3) & 7u, z = c >> 6;
        bool on = false;
        if (z % 2 == 0) {
          const bool up = (z / 2) % 2 == 0;  // the layer runs from y = 0 to 6, or back
          if (y % 2 == 0) on = true;
          else if (y < 7) {
            const uint32_t row = up ? (y - 1) / 2 : (5 - y) / 2;  // the connector behind row `row` of this layer's order
            on = x == (row % 2 == 0 ? 7u : 0u);
          }
        } else {
          on = x == 0u && y == ((z / 2) % 2 == 0 ? 6u : 0u);
        }
        k = on ? 1u : 2u;
      }
    }
}

template <class F>
static float median_ms(F launch) {
  hipEvent_t a, b;
  hipEventCreate(&a), hipEventCreate(&b);
  std::vector<float> t;
  launch();
  for (int i = 0; i < 5; ++i) {
    hipEventRecord(a, nullptr);
    launch();
    hipEventRecord(b, nullptr);
    hipEventSynchronize(b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, a, b);
    t.push_back(ms);
  }
  std::sort(t.begin(), t.end());
  hipEventDestroy(a), hipEventDestroy(b);
  return t[2];
}

int main(int argc, char **argv) {
  const uint32_t n = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 8192u;
  uint32_t *d_keys, *d_sweeps;
  uint16_t *d_a, *d_b;
  if (hipMalloc(&d_keys, (size_t)n * 512 * 4) != hipSuccess || hipMalloc(&d_a, (size_t)n * 512 * 2) != hipSuccess ||
      hipMalloc(&d_b, (size_t)n * 512 * 2) != hipSuccess || hipMalloc(&d_sweeps, (size_t)n * 4) != hipSuccess)
    return 2;
  std::vector<uint32_t> keys, sweeps(n);
  std::vector<uint16_t> a((size_t)n * 512), b((size_t)n * 512);
  const char *names[3] = {"random 30 %", "full brick", "serpentine"};
  for (int kind = 0; kind < 3; ++kind) {
    fill(keys, n, kind);
    hipMemcpy(d_keys, keys.data(), keys.size() * 4, hipMemcpyHostToDevice);
    for (int face = 0; face < 2; ++face) {
      const float reg = median_ms([&] {
        if (face) hipLaunchKernelGGL(k_reg<true>, dim3((n + 3) / 4), dim3(256), 0, nullptr, d_keys, n, d_a, d_sweeps);
        else hipLaunchKernelGGL(k_reg<false>, dim3((n + 3) / 4), dim3(256), 0, nullptr, d_keys, n, d_a, d_sweeps);
      });
      const float lds = median_ms([&] {
        if (face) hipLaunchKernelGGL(k_lds<true>, dim3(n), dim3(512), 0, nullptr, d_keys, n, d_b);
        else hipLaunchKernelGGL(k_lds<false>, dim3(n), dim3(512), 0, nullptr, d_keys, n, d_b);
      });
      if (hipDeviceSynchronize() != hipSuccess) return 3;
      hipMemcpy(a.data(), d_a, a.size() * 2, hipMemcpyDeviceToHost);
      hipMemcpy(b.data(), d_b, b.size() * 2, hipMemcpyDeviceToHost);
      hipMemcpy(sweeps.data(), d_sweeps, (size_t)n * 4, hipMemcpyDeviceToHost);
      std::printf("{\"fill\": \"%s\", \"connectivity\": %d, \"bricks\": %u, \"sweeps\": %u, \"reg_us\": %.1f, \"lds_us\": %.1f, \"lds_over_reg\": %.2f, \"same\": %s}\n",
                  names[kind], face ? 6 : 26, n, *std::max_element(sweeps.begin(), sweeps.end()), reg * 1e3f, lds * 1e3f, lds / reg,
                  a == b ? "true" : "false");
    }
  }
  hipFree(d_keys), hipFree(d_a), hipFree(d_b), hipFree(d_sweeps);
  return 0;
}
