// bloom_down.hip - the level-1 kernel of the HDR display chain (csrc/post.hip k_post_down<true>: the prefilter fused into the 4 x 4-tap
// down filter) two ways, at 1920 x 1080 on noise with a tenth of the texels above the threshold: (A) every lane reads its 16 source
// texels through the caches and prefilters each - the product kernel; (B) the block stages its 130 x 10 source tile, prefiltered once
// per texel, in LDS (20.8 KB) and filters from there. Both must produce the same bits; the times are hipEvent medians of 20 launches.
// build: hipcc -O3 --offload-arch=gfx950 -ffp-contract=off tools/microbench/bloom_down.hip -o tools/microbench/bloom_down.bin ; run on the GPU box
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 1; } } while (0)

constexpr uint32_t kRow = 64, kRows = 4, kTileW = 2 * kRow + 2, kTileH = 2 * kRows + 2;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ float4 prefilter(float4 s, float E, float threshold) {
   float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   const float lim = 281474976710656.0f;
   if (!(fabsf(s.x) <= lim && fabsf(s.y) <= lim && fabsf(s.z) <= lim)) return o;
   const float r = s.x * E, g = s.y * E, b = s.z * E;
   const float rg = r > g ? r : g, m = rg > b ? rg : b;
   if (!(m > threshold)) return o;
   const float f = (m - threshold) / m;
   o.x = r * f, o.y = g * f, o.z = b * f;
   return o;
}

__global__ __launch_bounds__(256) void k_down_caches(const float4* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ dst, uint32_t dw, uint32_t dh,
                                                     const float* __restrict__ exposure, float threshold) {
   const uint32_t X = blockIdx.x * kRow + threadIdx.x, Y = blockIdx.y * kRows + threadIdx.y;
   if (X >= dw || Y >= dh) return;
   const float E = *exposure;
   float r = 0.0f, g = 0.0f, b = 0.0f;
   for (int j = 0; j < 4; j++) {
      const size_t row = (size_t)clampi(2 * (int)Y - 1 + j, (int)sh - 1) * sw;
      const int wy = (j == 0 || j == 3) ? 1 : 3;
      for (int i = 0; i < 4; i++) {
         const int sx = clampi(2 * (int)X - 1 + i, (int)sw - 1);
         const float w = (float)(((i == 0 || i == 3) ? 1 : 3) * wy) * 0.015625f;
         const float4 t = prefilter(src[row + sx], E, threshold);
         r = r + w * t.x, g = g + w * t.y, b = b + w * t.z;
      }
   }
   dst[(size_t)Y * dw + X] = make_float4(r, g, b, 0.0f);
}

__global__ __launch_bounds__(256) void k_down_lds(const float4* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ dst, uint32_t dw, uint32_t dh,
                                                  const float* __restrict__ exposure, float threshold) {
   __shared__ float4 tile[kTileH][kTileW];
   const float E = *exposure;
   const int sx0 = 2 * (int)(blockIdx.x * kRow) - 1, sy0 = 2 * (int)(blockIdx.y * kRows) - 1;
   for (uint32_t idx = threadIdx.y * kRow + threadIdx.x; idx < kTileW * kTileH; idx += 256) {
      const uint32_t ty = idx / kTileW, tx = idx % kTileW;
      const int sx = clampi(sx0 + (int)tx, (int)sw - 1), sy = clampi(sy0 + (int)ty, (int)sh - 1);
      tile[ty][tx] = prefilter(src[(size_t)sy * sw + sx], E, threshold);
   }
   __syncthreads();
   const uint32_t X = blockIdx.x * kRow + threadIdx.x, Y = blockIdx.y * kRows + threadIdx.y;
   if (X >= dw || Y >= dh) return;
   float r = 0.0f, g = 0.0f, b = 0.0f;
   for (int j = 0; j < 4; j++) {
      const int wy = (j == 0 || j == 3) ? 1 : 3;
      for (int i = 0; i < 4; i++) {
         const float w = (float)(((i == 0 || i == 3) ? 1 : 3) * wy) * 0.015625f;
         const float4 t = tile[2 * threadIdx.y + j][2 * threadIdx.x + i];
         r = r + w * t.x, g = g + w * t.y, b = b + w * t.z;
      }
   }
   dst[(size_t)Y * dw + X] = make_float4(r, g, b, 0.0f);
}

int main() {
   const uint32_t W = 1920, H = 1080, dw = (W + 1) / 2, dh = (H + 1) / 2;
   std::vector<float4> host((size_t)W * H);
   uint32_t s = 12345u;
   for (float4& t : host) {
      float v[4];
      for (float& c : v) {
         s = s * 1664525u + 1013904223u;
         const float u = (float)(s >> 8) * (1.0f / 16777216.0f);
         c = u < 0.9f ? u : (u - 0.9f) * 200.0f;  // a tenth of the channels above 1
      }
      t = make_float4(v[0], v[1], v[2], 1.0f);
   }
   host[5].x = __builtin_nanf("");
   float4 *src = nullptr, *a = nullptr, *b = nullptr;
   float* exposure = nullptr;
   const float one = 1.0f;
   CK(hipMalloc(&src, host.size() * sizeof(float4)));
   CK(hipMalloc(&a, (size_t)dw * dh * sizeof(float4)));
   CK(hipMalloc(&b, (size_t)dw * dh * sizeof(float4)));
   CK(hipMalloc(&exposure, sizeof(float)));
   CK(hipMemcpy(src, host.data(), host.size() * sizeof(float4), hipMemcpyHostToDevice));
   CK(hipMemcpy(exposure, &one, sizeof(float), hipMemcpyHostToDevice));
   const dim3 grid((dw + kRow - 1) / kRow, (dh + kRows - 1) / kRows), block(kRow, kRows);
   hipEvent_t e0, e1;
   CK(hipEventCreate(&e0));
   CK(hipEventCreate(&e1));
   for (int variant = 0; variant < 2; variant++) {
      std::vector<float> ms;
      for (int it = 0; it < 25; it++) {
         CK(hipEventRecord(e0, nullptr));
         if (variant == 0)
            k_down_caches<<<grid, block>>>(src, W, H, a, dw, dh, exposure, 1.0f);
         else
            k_down_lds<<<grid, block>>>(src, W, H, b, dw, dh, exposure, 1.0f);
         CK(hipEventRecord(e1, nullptr));
         CK(hipEventSynchronize(e1));
         CK(hipGetLastError());
         float t = 0.0f;
         CK(hipEventElapsedTime(&t, e0, e1));
         if (it >= 5) ms.push_back(t);
      }
      std::sort(ms.begin(), ms.end());
      const double bytes = 16.0 * ((double)W * H + (double)dw * dh);
      printf("%s: median %.4f ms (min %.4f, max %.4f), %.0f GB/s of compulsory traffic\n", variant == 0 ? "caches" : "lds tile", ms[ms.size() / 2], ms.front(), ms.back(),
             bytes / (ms[ms.size() / 2] * 1e-3) / 1e9);
   }
   std::vector<float4> ha((size_t)dw * dh), hb((size_t)dw * dh);
   CK(hipMemcpy(ha.data(), a, ha.size() * sizeof(float4), hipMemcpyDeviceToHost));
   CK(hipMemcpy(hb.data(), b, hb.size() * sizeof(float4), hipMemcpyDeviceToHost));
   const bool same = std::memcmp(ha.data(), hb.data(), ha.size() * sizeof(float4)) == 0;
   printf("outputs %s\n", same ? "bit-identical" : "DIFFER");
   (void)hipFree(src), (void)hipFree(a), (void)hipFree(b), (void)hipFree(exposure);
   return same ? 0 : 1;
}
