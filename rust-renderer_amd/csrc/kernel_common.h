// kernel_common.h — what the kernel files (kernels.hip, path_fused.hip, restir.hip, tiles.hip, hybrid_kernels.hip, rtao.hip, rtgi.hip, glossy.hip, fog.hip, glass.hip, area_lights.hip) share
// besides the device arithmetic: the block size, the launch-grid helpers of their launchers, and four small device functions that kernels
// of more than one file call (resolve_color: the path tracer's resolve and the tile composition; gbuffer_fetch: the ReSTIR passes and the
// hybrid passes; rtao_normal: rtao.hip, rtgi.hip and area_lights.hip; queue_pixels: every classify kernel of the hybrid frame). The hybrid frame's ray
// passes share more: their persistent walk is item_walk.h, the tile filter of rtao.hip and rtgi.hip is edge_filter.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_math.h"
#include "device_types.h"

namespace uh {

constexpr int kBlock = 256;                 // 4 waves
constexpr int kWavesPerBlock = kBlock / 64;

// reference.rgen:140-144: the accumulated radiance of a pixel as its B8G8R8A8 output texel
__device__ __forceinline__ uchar4 resolve_color(float4 acc, uint32_t total_samples, uint32_t limit) {
   float denom = (float)min(total_samples, limit);
   V3 c = v3(acc.x / denom, acc.y / denom, acc.z / denom);                               // rgen:140
   c = v3(linear_to_srgb(c.x), linear_to_srgb(c.y), linear_to_srgb(c.z));               // rgen:141
   return make_uchar4((unsigned char)unorm8(c.z), (unsigned char)unorm8(c.y), (unsigned char)unorm8(c.x), 0);  // B8G8R8A8, alpha 0
}

// texture(in_gbuffer_position, vec2(px) / vec2(size)) through the LINEAR + MIRRORED_REPEAT sampler
// (restir/initial_ris.rgen:22-23): the texel corner, i.e. the mean of the 2x2 texels up-left
__device__ __forceinline__ V3 gbuffer_fetch(const float4* __restrict__ g, uint32_t W, uint32_t px, uint32_t py) {
   uint32_t x0 = px == 0 ? 0 : px - 1, y0 = py == 0 ? 0 : py - 1;
   float4 a = g[(size_t)y0 * W + x0], b = g[(size_t)y0 * W + px], c = g[(size_t)py * W + x0], d = g[(size_t)py * W + px];
   return ((xyz(a) + xyz(b)) + (xyz(c) + xyz(d))) * 0.25f;
}

// Nn of a G-buffer pixel and whether it casts hemisphere rays (the rtao and rtgi passes): normalize3 of the normal texel, finite in every
// component
__device__ __forceinline__ bool rtao_normal(float4 N4, V3& nn) {
   nn = normalize3(v3(N4.x, N4.y, N4.z));
   return fabsf(nn.x) < INFINITY && fabsf(nn.y) < INFINITY && fabsf(nn.z) < INFINITY;  // NaN: false
}

// The classify of the hybrid frame's passes: one lane per pixel of the n, the pixels that satisfy pred(pix) are appended to a dense queue
// (one atomic per wave: wave group g holds pixels g * 64 + lane). pred is called once for every pixel: a kernel clears its texels there.
template <typename Pred>
__device__ __forceinline__ void queue_pixels(uint32_t n, uint32_t* counter, uint32_t* queue, Pred&& pred) {
   const uint32_t groups = (n + 63) / 64, lane = lane_id();
   for (uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += gridDim.x * kWavesPerBlock) {
      const uint32_t pix = g * 64u + lane;
      const bool queued = pix < n && pred(pix);
      const uint32_t slot = wave_append(counter, queued);
      if (queued) queue[slot] = pix;
   }
}

// ---- launch grids
static inline dim3 stream_grid(const LaunchCfg& c, uint32_t n) {
   uint32_t blocks = (n + kBlock - 1) / kBlock;
   uint32_t cap = c.num_cus * 8;
   return dim3(blocks < cap ? (blocks ? blocks : 1) : cap);
}
// persistent waves that take their work in chunks: at most one lane per item, at most `full` blocks
static inline dim3 persistent_grid(uint64_t items, uint32_t full) {
   const uint64_t need = (items + kBlock - 1) / kBlock;
   return dim3((uint32_t)(need < full ? (need ? need : 1) : full));
}
// grids of sharded kernels are whole multiples of kShards (blockIdx % kShards = shard)
static inline dim3 sharded_grid(uint32_t blocks) {
   uint32_t g = (blocks / kShards) * kShards;
   return dim3(g < kShards ? kShards : g);
}
static inline dim3 closest_grid(const LaunchCfg& c) { return sharded_grid(c.num_cus * c.closest_blocks_per_cu); }
static inline dim3 shadow_grid(const LaunchCfg& c) { return sharded_grid(c.num_cus * c.shadow_blocks_per_cu); }
static inline dim3 shade_grid(const LaunchCfg& c, uint32_t n) {
   uint32_t blocks = (n + kBlock - 1) / kBlock, cap = c.num_cus * 8;
   return sharded_grid(blocks < cap ? blocks : cap);
}

// a run-time bool as a template argument: f(std::true_type{}) or f(std::false_type{}) - the launchers pick a kernel's instantiation with it
template <typename F>
static inline void as_constant(bool b, F&& f) {
   if (b) f(std::true_type{});
   else f(std::false_type{});
}

// the primary-ray cast both G-buffers start from (kernels.hip): ray j = the ray through the centre of pixel spans.pixel_of(j), walked
// through the camera grid when there is one and through the tree otherwise; the hit records are left in rr.hit
void launch_gbuffer_cast(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const RawRays& rr, const RowSpans& spans, DeviceStats* stats,
                         const SunGridDev* camera_grid);

}  // namespace uh
