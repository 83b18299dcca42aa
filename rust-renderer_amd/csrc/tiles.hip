// tiles.hip — multi-GPU tiles of the RGBA32F accumulation image: pack, unpack and the root's composition, with their launchers.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"
#include "tile_partition.h"

namespace uh {

template <bool PACK>
__global__ __launch_bounds__(kBlock) void k_tiles(float4* acc, float4* packed, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile) {
   const uint32_t tiles_x = tiles_across(W, tile);
   const uint64_t total = pack_pixels(W, H, tile, rank, world);
   for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
      const PackedPixel p = packed_pixel(i, W, H, tile, tiles_x, rank, world);
      if (PACK)
         packed[i] = p.inside ? acc[(size_t)p.y * W + p.x] : make_float4(0, 0, 0, 0);
      else if (p.inside)
         acc[(size_t)p.y * W + p.x] = packed[i];
   }
}

// the root's composition in one pass over the frame: a pixel of another rank's tile comes out of that rank's packed buffer
// (`all` holds world buffers of `stride` pixels each, rank r's at r * stride, laid out as k_tiles<true> packs them), the
// root's own pixels stay, and pt_output_image is recomputed for every pixel (rgen:140-144)
__global__ __launch_bounds__(kBlock) void k_compose_tiles(Images im, const float4* __restrict__ all, uint64_t stride, uint32_t W, uint32_t H, uint32_t rank, uint32_t world,
                                                           uint32_t tile, uint32_t total_samples, uint32_t limit) {
   const uint32_t tiles_x = tiles_across(W, tile), n = W * H;
   for (uint32_t pix = blockIdx.x * kBlock + threadIdx.x; pix < n; pix += gridDim.x * kBlock) {
      const uint32_t x = pix % W, y = pix / W;
      const uint32_t t = tile_of_pixel(x, y, tile, tiles_x), owner = tile_owner(t, world);
      float4 acc;
      if (owner == rank)
         acc = im.accumulation[pix];
      else {
         acc = all[owner * stride + packed_position(t, x, y, tile, world)];
         im.accumulation[pix] = acc;
      }
      im.output[pix] = resolve_color(acc, total_samples, limit);
   }
}
void launch_compose_tiles(const LaunchCfg& c, const Images& im, const float4* all, uint64_t stride, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile,
                          uint32_t total_samples, uint32_t limit) {
   k_compose_tiles<<<stream_grid(c, W * H), kBlock, 0, c.stream>>>(im, all, stride, W, H, rank, world, tile, total_samples, limit);
}

void launch_pack_tiles(const LaunchCfg& c, const float4* acc, float4* out, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile) {
   k_tiles<true><<<stream_grid(c, W * H), kBlock, 0, c.stream>>>(const_cast<float4*>(acc), out, W, H, rank, world, tile);
}
void launch_unpack_tiles(const LaunchCfg& c, float4* acc, const float4* in, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile) {
   k_tiles<false><<<stream_grid(c, W * H), kBlock, 0, c.stream>>>(acc, const_cast<float4*>(in), W, H, rank, world, tile);
}

}  // namespace uh
