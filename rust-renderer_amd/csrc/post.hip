// post.hip - the HDR display chain of the hybrid frame (UH_HYBRID_POST and uh_post_image; utopian_hip.h): metering (a 256-bin luminance
// histogram and the exposure it gives), bloom (a thresholded down-sampling pyramid and an up-sampling chain) and the composite with its
// tone-mapping operator into post_output. An extension: the reference's present.frag stops at a commented-out Reinhard line.
// Arithmetic: DESIGN.md section 2, "HDR display chain: the arithmetic contract of UH_HYBRID_POST"; tests/post_reference.py restates it.
// Everything is + - * /, compares and integer operations in float32 (-ffp-contract=off): the result is defined to the bit. Every count
// is an integer: no float atomic anywhere, so the order in which waves arrive changes nothing.
// Layout: the image kernels are TAA's - a block is 4 rows of 64 texels, one row per wave; overlapping reads of neighbouring texels are
// served by the caches, except in the level-1 kernel, which stages its prefiltered source tile in LDS ("HDR
// display chain": measured both ways).
#include <hip/hip_runtime.h>

#include "denoise_device.h"
#include "device_types.h"
#include "kernel_common.h"

namespace uh {

constexpr uint32_t kPostRow = 64, kPostRows = kBlock / kPostRow;

// the contract's max and min: the first operand when the compare holds, else the second (so max(-0, 0) is +0 on every path)
__device__ __forceinline__ float post_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float post_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ int post_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- metering ----
// The histogram: a grid sized to the device that strides over the frame, a wave taking 64 consecutive texels (one 16-byte load per
// lane) per step. Each wave counts into a histogram of its own in LDS (LDS integer atomics), the block adds its four up, and each
// non-empty bin goes to the global counts with one integer atomic per block.
__global__ __launch_bounds__(kBlock) void k_post_histogram(PostDev p) {
   __shared__ uint32_t bins[kWavesPerBlock][kPostBins];
   const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
   for (uint32_t w = 0; w < (uint32_t)kWavesPerBlock; w++) bins[w][t] = 0;
   __syncthreads();
   const size_t n = (size_t)p.W * p.H, step = (size_t)gridDim.x * kBlock;
   for (size_t base = ((size_t)blockIdx.x * kWavesPerBlock + wave) * 64; base < n; base += step) {
      const size_t i = base + lane;
      if (i >= n) continue;
      const float4 c = p.src[i];
      const float L = dn_luminance(c.x, c.y, c.z);
      int bin = 0;
      if (temporal_sample_ok(c.x, c.y, c.z) && L > 0.0f) bin = post_clampi((int)(__float_as_uint(L) >> 20) - 888, (int)kPostBins - 1);
      atomicAdd(&bins[wave][bin], 1u);
   }
   __syncthreads();
   uint32_t s = 0;
   for (uint32_t w = 0; w < (uint32_t)kWavesPerBlock; w++) s += bins[w][t];
   if (s) atomicAdd(&p.hist[t], s);
}

// The exposure: one block, thread b owns bin b. Prefix of the counts of bins 1..255, each bin's rank range clipped against [lo, hi),
// the two 64-bit sums reduced, and thread 0 writes the record. The counts move to hist_copy and hist is zero again for the next pass.
__global__ __launch_bounds__(kPostBins) void k_post_exposure(PostDev p) {
   __shared__ unsigned long long scan[kPostBins], sum_b[kPostBins], sum_n[kPostBins];
   const uint32_t b = threadIdx.x;
   uint32_t count = 0;
   if (p.auto_exposure) {
      count = p.hist[b];
      p.hist_copy[b] = count;
      p.hist[b] = 0;
   }
   const unsigned long long m = b ? count : 0;  // bin 0 is not metered
   scan[b] = m;
   __syncthreads();
   for (uint32_t d = 1; d < kPostBins; d <<= 1) {
      const unsigned long long add = b >= d ? scan[b - d] : 0;
      __syncthreads();
      scan[b] += add;
      __syncthreads();
   }
   const unsigned long long end = scan[b], begin = end - m, n = scan[kPostBins - 1];
   const unsigned long long lo = (unsigned long long)((double)p.low_percentile * (double)n), hi = (unsigned long long)((double)p.high_percentile * (double)n);
   unsigned long long kept = m;
   if (hi > lo) {
      const unsigned long long from = begin > lo ? begin : lo, to = end < hi ? end : hi;
      kept = to > from ? to - from : 0;
   }
   sum_b[b] = kept * b;
   sum_n[b] = kept;
   __syncthreads();
   for (uint32_t d = kPostBins / 2; d; d >>= 1) {
      if (b < d) sum_b[b] += sum_b[b + d], sum_n[b] += sum_n[b + d];
      __syncthreads();
   }
   if (b == 0) {
      const unsigned long long Sb = sum_b[0], N = sum_n[0];
      const float prev = p.rec->exposure;
      float E, target, lavg = 0.0f;
      if (!p.auto_exposure) {
         E = target = p.manual_exposure;
      } else if (N == 0) {
         E = target = p.have_prev ? prev : p.manual_exposure;
      } else {
         const uint32_t q = (888u << 20) + (uint32_t)((Sb << 20) / N) + (1u << 19);
         lavg = __uint_as_float(q);
         target = post_min(post_max(p.key / lavg, p.min_exposure), p.max_exposure);
         E = p.have_prev ? prev + (target - prev) * p.adaptation : target;
      }
      PostRecord r;
      r.exposure = E, r.target = target, r.lavg = lavg;
      r.metered = (uint32_t)n, r.bad = 0;
      r.pad[0] = r.pad[1] = r.pad[2] = 0;
      *p.rec = r;
   }
}

// ---- bloom ----
// the prefilter of a frame texel: 0 for a bad pixel and below the threshold, else the exposed colour scaled by (m - threshold) / m
__device__ __forceinline__ float4 post_prefilter(float4 s, float E, float threshold) {
   float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   if (!temporal_sample_ok(s.x, s.y, s.z)) return o;
   const float r = s.x * E, g = s.y * E, b = s.z * E;
   const float m = post_max(post_max(r, g), b);
   if (!(m > threshold)) return o;
   const float f = (m - threshold) / m;
   o.x = r * f, o.y = g * f, o.z = b * f;
   return o;
}

// the weight of tap (i, j) of the down filter: (1, 3, 3, 1) / 8 per axis, the product as (float)(wx * wy) / 64
__device__ __forceinline__ float post_down_weight(int i, int j) { return (float)(((i == 0 || i == 3) ? 1 : 3) * ((j == 0 || j == 3) ? 1 : 3)) * 0.015625f; }

// down[1], one lane per destination texel: the 4 x 4 taps around source (2X + 0.5, 2Y + 0.5) of the PREFILTERED frame, indices clamped,
// rows outer and columns inner. A block's 64 x 4 destinations read a 130 x 10 source tile: it is staged in LDS (20.8 KB), prefiltered
// once per texel instead of once per tap, the clamp applied where the tile is loaded (tap and tile index clamp to the same texel).
constexpr uint32_t kPostTileW = 2 * kPostRow + 2, kPostTileH = 2 * kPostRows + 2;
__global__ __launch_bounds__(kBlock) void k_post_down_first(const float4* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ dst, uint32_t dw, uint32_t dh,
                                                            const PostRecord* __restrict__ rec, float threshold) {
   __shared__ float4 tile[kPostTileH][kPostTileW];
   const float E = rec->exposure;
   const int sx0 = 2 * (int)(blockIdx.x * kPostRow) - 1, sy0 = 2 * (int)(blockIdx.y * kPostRows) - 1;
   for (uint32_t idx = threadIdx.y * kPostRow + threadIdx.x; idx < kPostTileW * kPostTileH; idx += kBlock) {
      const uint32_t ty = idx / kPostTileW, tx = idx - ty * kPostTileW;
      const int sx = post_clampi(sx0 + (int)tx, (int)sw - 1), sy = post_clampi(sy0 + (int)ty, (int)sh - 1);
      tile[ty][tx] = post_prefilter(src[(size_t)sy * sw + sx], E, threshold);
   }
   __syncthreads();
   const uint32_t X = blockIdx.x * kPostRow + threadIdx.x, Y = blockIdx.y * kPostRows + threadIdx.y;
   if (X >= dw || Y >= dh) return;
   float r = 0.0f, g = 0.0f, b = 0.0f;
   for (int j = 0; j < 4; j++) {
      for (int i = 0; i < 4; i++) {
         const float w = post_down_weight(i, j);
         const float4 t = tile[2 * threadIdx.y + j][2 * threadIdx.x + i];
         r = r + w * t.x, g = g + w * t.y, b = b + w * t.z;
      }
   }
   dst[(size_t)Y * dw + X] = make_float4(r, g, b, 0.0f);
}

// down[k], k >= 2, one lane per destination texel: the same taps of down[k - 1], read through the caches (these levels are small)
__global__ __launch_bounds__(kBlock) void k_post_down(const float4* __restrict__ src, uint32_t sw, uint32_t sh, float4* __restrict__ dst, uint32_t dw, uint32_t dh) {
   const uint32_t X = blockIdx.x * kPostRow + threadIdx.x, Y = blockIdx.y * kPostRows + threadIdx.y;
   if (X >= dw || Y >= dh) return;
   float r = 0.0f, g = 0.0f, b = 0.0f;
   for (int j = 0; j < 4; j++) {
      const size_t row = (size_t)post_clampi(2 * (int)Y - 1 + j, (int)sh - 1) * sw;
      for (int i = 0; i < 4; i++) {
         const int sx = post_clampi(2 * (int)X - 1 + i, (int)sw - 1);
         const float w = post_down_weight(i, j);
         const float4 t = src[row + sx];
         r = r + w * t.x, g = g + w * t.y, b = b + w * t.z;
      }
   }
   dst[(size_t)Y * dw + X] = make_float4(r, g, b, 0.0f);
}

// U(img) at destination (x, y): the two nearest source texels per axis at 0.75 and 0.25, indices clamped, the four taps in the order
// (first x, first y), (second x, first y), (first x, second y), (second x, second y)
__device__ __forceinline__ float4 post_upsample(const float4* __restrict__ img, uint32_t sw, uint32_t sh, uint32_t x, uint32_t y) {
   const bool ox = x & 1u, oy = y & 1u;
   const int x0 = post_clampi(ox ? (int)((x - 1) / 2) : (int)(x / 2) - 1, (int)sw - 1), x1 = post_clampi(ox ? (int)((x + 1) / 2) : (int)(x / 2), (int)sw - 1);
   const int y0 = post_clampi(oy ? (int)((y - 1) / 2) : (int)(y / 2) - 1, (int)sh - 1), y1 = post_clampi(oy ? (int)((y + 1) / 2) : (int)(y / 2), (int)sh - 1);
   const float wx0 = ox ? 0.75f : 0.25f, wx1 = ox ? 0.25f : 0.75f, wy0 = oy ? 0.75f : 0.25f, wy1 = oy ? 0.25f : 0.75f;
   const float4 a = img[(size_t)y0 * sw + x0], b = img[(size_t)y0 * sw + x1], c = img[(size_t)y1 * sw + x0], d = img[(size_t)y1 * sw + x1];
   const float w00 = wx0 * wy0, w10 = wx1 * wy0, w01 = wx0 * wy1, w11 = wx1 * wy1;
   float4 o;
   o.x = (((0.0f + w00 * a.x) + w10 * b.x) + w01 * c.x) + w11 * d.x;
   o.y = (((0.0f + w00 * a.y) + w10 * b.y) + w01 * c.y) + w11 * d.y;
   o.z = (((0.0f + w00 * a.z) + w10 * b.z) + w01 * c.z) + w11 * d.z;
   o.w = 0.0f;
   return o;
}

// up[k] = (down[k] + U(up[k + 1])) * 0.5, one lane per texel of level k
__global__ __launch_bounds__(kBlock) void k_post_up(const float4* __restrict__ down, const float4* __restrict__ next, uint32_t nw, uint32_t nh, float4* __restrict__ dst,
                                                    uint32_t w, uint32_t h) {
   const uint32_t x = blockIdx.x * kPostRow + threadIdx.x, y = blockIdx.y * kPostRows + threadIdx.y;
   if (x >= w || y >= h) return;
   const size_t i = (size_t)y * w + x;
   const float4 d = down[i], u = post_upsample(next, nw, nh, x, y);
   dst[i] = make_float4((d.x + u.x) * 0.5f, (d.y + u.y) * 0.5f, (d.z + u.z) * 0.5f, 0.0f);
}

// ---- composite and tone map ----
template <int kOp> __device__ __forceinline__ float post_tonemap(float x) {
   if (kOp == UH_TONEMAP_NONE) return x;
   const float xc = post_min(post_max(x, 0.0f), 1048576.0f);
   if (kOp == UH_TONEMAP_REINHARD) return xc / (xc + 1.0f);
   const float a = xc * (2.51f * xc + 0.03f), b = xc * (2.43f * xc + 0.59f) + 0.14f;
   return post_min(post_max(a / b, 0.0f), 1.0f);
}

// one lane per pixel: x = S.rgb * E + bloom_intensity * U(up[1]) through the operator; a bad pixel passes through, bits unchanged, and
// is counted (a ballot and at most one integer atomic per wave: bad pixels are rare)
template <int kOp, bool kBloom>
__global__ __launch_bounds__(kBlock) void k_post_composite(PostDev p) {
   const uint32_t x = blockIdx.x * kPostRow + threadIdx.x, y = blockIdx.y * kPostRows + threadIdx.y;
   bool bad = false;
   if (x < p.W && y < p.H) {
      const size_t i = (size_t)y * p.W + x;
      const float4 s = p.src[i];
      bad = !temporal_sample_ok(s.x, s.y, s.z);
      float4 o = s;
      if (!bad) {
         const float E = p.rec->exposure;
         float r = s.x * E, g = s.y * E, b = s.z * E;
         if (kBloom) {
            const float4 u = post_upsample(p.up[1], p.lw[1], p.lh[1], x, y);
            r = r + p.bloom_intensity * u.x, g = g + p.bloom_intensity * u.y, b = b + p.bloom_intensity * u.z;
         }
         o.x = post_tonemap<kOp>(r), o.y = post_tonemap<kOp>(g), o.z = post_tonemap<kOp>(b);
      }
      p.out[i] = o;
   }
   const unsigned long long bb = __ballot(bad);
   if (threadIdx.x == 0 && bb) atomicAdd(&p.rec->bad, (uint32_t)__popcll(bb));
}

// ---- launchers ----
static dim3 post_grid(uint32_t w, uint32_t h) { return dim3((w + kPostRow - 1) / kPostRow, (h + kPostRows - 1) / kPostRows); }

void launch_post_meter(const LaunchCfg& c, const PostDev& p) {
   if (p.auto_exposure) {
      const size_t blocks = ((size_t)p.W * p.H + kBlock - 1) / kBlock, cap = (size_t)c.num_cus * 4;
      k_post_histogram<<<dim3((uint32_t)(blocks < cap ? blocks : cap)), dim3(kBlock), 0, c.stream>>>(p);
   }
   k_post_exposure<<<dim3(1), dim3(kPostBins), 0, c.stream>>>(p);
}

void launch_post_bloom(const LaunchCfg& c, const PostDev& p) {
   const dim3 block(kPostRow, kPostRows);
   for (uint32_t k = 1; k <= p.levels; k++) {
      if (k == 1)
         k_post_down_first<<<post_grid(p.lw[1], p.lh[1]), block, 0, c.stream>>>(p.src, p.W, p.H, p.down[1], p.lw[1], p.lh[1], p.rec, p.bloom_threshold);
      else
         k_post_down<<<post_grid(p.lw[k], p.lh[k]), block, 0, c.stream>>>(p.down[k - 1], p.lw[k - 1], p.lh[k - 1], p.down[k], p.lw[k], p.lh[k]);
   }
   for (uint32_t k = p.levels; k-- > 1;)
      k_post_up<<<post_grid(p.lw[k], p.lh[k]), block, 0, c.stream>>>(p.down[k], p.up[k + 1], p.lw[k + 1], p.lh[k + 1], p.up[k], p.lw[k], p.lh[k]);
}

template <int kOp> static void launch_composite_op(const LaunchCfg& c, const PostDev& p) {
   const dim3 grid = post_grid(p.W, p.H), block(kPostRow, kPostRows);
   if (p.levels)
      k_post_composite<kOp, true><<<grid, block, 0, c.stream>>>(p);
   else
      k_post_composite<kOp, false><<<grid, block, 0, c.stream>>>(p);
}

void launch_post_composite(const LaunchCfg& c, const PostDev& p) {
   if (p.tonemap == UH_TONEMAP_NONE)
      launch_composite_op<UH_TONEMAP_NONE>(c, p);
   else if (p.tonemap == UH_TONEMAP_REINHARD)
      launch_composite_op<UH_TONEMAP_REINHARD>(c, p);
   else
      launch_composite_op<UH_TONEMAP_ACES>(c, p);
}

}  // namespace uh
