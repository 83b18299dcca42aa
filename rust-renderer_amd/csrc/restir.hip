// restir.hip — the ReSTIR reservoir passes (reference, utopian/shaders/restir/{reset_reservoirs.comp,initial_ris.rgen,temporal_reuse.rgen,
// spatial_reuse.rgen}) and their launchers.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"

namespace uh {

// ------------------------------------------------------------------------------------------
// ReSTIR passes. The light table (pos + intensity, 32 B/light, <= 32 KiB) is staged in LDS.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kMaxLdsLights = UH_MAX_GPU_LIGHTS;

__device__ __forceinline__ void stage_lights(float4* s_lights, const SceneDev& sc) {
   for (uint32_t i = threadIdx.x; i < 2 * sc.num_lights; i += blockDim.x) s_lights[i] = sc.lights[i];
   __syncthreads();
}

// restir/reset_reservoirs.comp:24-45
__global__ __launch_bounds__(kBlock) void k_reset_reservoirs(Images im, RowSpans spans) {
   const uint32_t n = spans.total();
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
      const uint32_t id = spans.pixel_of(j);
      UhReservoir z = {-1, 0.0f, 0.0f, 0};
      im.reservoirs[0][id] = z;
      im.reservoirs[1][id] = z;
   }
}

// restir/initial_ris.rgen:19-39 + restir_sampling.glsl:96-131 (resample, 32 candidates)
__global__ __launch_bounds__(kBlock) void k_initial_ris(FrameParams fp, SceneDev sc, Images im, RowSpans spans) {
   __shared__ float4 s_lights[2 * kMaxLdsLights];
   stage_lights(s_lights, sc);
   const uint32_t work = spans.total();
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < work; j += gridDim.x * kBlock) {
      const uint32_t id = spans.pixel_of(j);
      uint32_t px = id % fp.W, py = id / fp.W;
      uint32_t rng = init_rng(px, py, fp.W, fp.frame_number);
      V3 hit_position = gbuffer_fetch(im.gbuffer_pos, fp.W, px, py);
      UhReservoir r = {-1, 0.0f, 0.0f, 0};
      for (int i = 0; i < 32; i++) {
         int cand;
         float p;
         sample_light_uniform(fp.num_lights_used, rng, cand, p);
         float m_i = 1.0f / 32.0f;
         float p_hat = target_function(s_lights, sc.num_lights, cand, hit_position);
         float W_Xi = 1.0f / p;
         float w_i = m_i * p_hat * W_Xi;
         update_reservoir(rng, r, cand, w_i, 1);
      }
      r.M = 1;
      if (r.Y != -1) finalize_resampling(r, target_function(s_lights, sc.num_lights, r.Y, hit_position));
      UhReservoir nr = {-1, 0.0f, 0.0f, 0};
      update_reservoir(rng, nr, r.Y, r.W_sum * (float)r.M, r.M);
      finalize_resampling(nr, target_function(s_lights, sc.num_lights, nr.Y, hit_position));
      im.reservoirs[0][id] = nr;
   }
}

// restir/temporal_reuse.rgen:35-119
__global__ __launch_bounds__(kBlock) void k_temporal_reuse(FrameParams fp, SceneDev sc, Images im, RowSpans spans) {
   __shared__ float4 s_lights[2 * kMaxLdsLights];
   stage_lights(s_lights, sc);
   const uint32_t n = fp.W * fp.H, work = spans.total();
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < work; j += gridDim.x * kBlock) {
      const uint32_t id = spans.pixel_of(j);
      if (fp.temporal_enabled == 0) {
         im.reservoirs[1][id] = im.reservoirs[0][id];
         continue;
      }
      uint32_t px = id % fp.W, py = id / fp.W;
      uint32_t rng = init_rng(px, py, fp.W, fp.frame_number);
      V3 hit_position = gbuffer_fetch(im.gbuffer_pos, fp.W, px, py);
      UhReservoir nr = {-1, 0.0f, 0.0f, 0};
      UhReservoir ir = im.reservoirs[0][id];
      float p_hat = target_function(s_lights, sc.num_lights, ir.Y, hit_position);
      update_reservoir(rng, nr, ir.Y, p_hat * ir.W_X * (float)ir.M, ir.M);
      UhReservoir pr = {-1, 0.0f, 0.0f, 0};
      float4 puv = mat4_mul(fp.prev_pv, hit_position.x, hit_position.y, hit_position.z, 1.0f);
      float ux = puv.x / puv.w, uy = puv.y / puv.w;
      ux = ux * 0.5f + 0.5f;
      uy = uy * 0.5f + 0.5f;
      uy = 1.0f - uy;
      if (ux >= 0.0f && ux <= 1.0f && uy >= 0.0f && uy <= 1.0f) {
         int ix = (int)(ux * (float)fp.W + 0.5f), iy = (int)(uy * (float)fp.H + 0.5f);
         uint32_t ti = (uint32_t)iy * fp.W + (uint32_t)ix;  // may be one past the end in the reference (y == H)
         if (ti > n - 1) ti = n - 1;
         pr = im.prev_spatial[ti];  // last frame's spatial_reuse_reservoirs (renderers/mod.rs:294)
      }
      p_hat = pr.Y == -1 ? 0.0f : target_function(s_lights, sc.num_lights, pr.Y, hit_position);
      pr.M = min(20 * ir.M, pr.M);
      update_reservoir(rng, nr, pr.Y, p_hat * pr.W_X * (float)pr.M, pr.M);
      if (nr.Y != -1) finalize_resampling(nr, target_function(s_lights, sc.num_lights, nr.Y, hit_position));
      im.reservoirs[1][id] = nr;
   }
}

// restir/spatial_reuse.rgen:23-73
__global__ __launch_bounds__(kBlock) void k_spatial_reuse(FrameParams fp, SceneDev sc, Images im, RowSpans spans) {
   __shared__ float4 s_lights[2 * kMaxLdsLights];
   stage_lights(s_lights, sc);
   const uint32_t work = spans.total();
   const UhReservoir* __restrict__ temporal = im.reservoirs[1];
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < work; j += gridDim.x * kBlock) {
      const uint32_t id = spans.pixel_of(j);
      if (fp.spatial_enabled == 0) {
         im.reservoirs[2][id] = temporal[id];
         continue;
      }
      uint32_t px = id % fp.W, py = id / fp.W;
      uint32_t rng = init_rng(px, py, fp.W, fp.frame_number);
      V3 hit_position = gbuffer_fetch(im.gbuffer_pos, fp.W, px, py);
      UhReservoir nr = {-1, 0.0f, 0.0f, 0};
      UhReservoir tr = temporal[id];
      float p_hat = target_function(s_lights, sc.num_lights, tr.Y, hit_position);
      update_reservoir(rng, nr, tr.Y, p_hat * tr.W_X * (float)tr.M, tr.M);
      for (int i = 0; i < 5; i++) {
         float ox = random_float(rng) * 2.0f - 1.0f, oy = random_float(rng) * 2.0f - 1.0f;
         ox *= 30.0f;
         oy *= 30.0f;
         // uvec2(offset) of a negative float: pinned as (uint)(int)trunc(x); clamp(uvec2) then
         // sends a wrapped-negative coordinate to size-1
         uint32_t nx = px + (uint32_t)(int)ox, ny = py + (uint32_t)(int)oy;
         nx = min(nx, fp.W - 1);
         ny = min(ny, fp.H - 1);
         UhReservoir nb = temporal[(size_t)ny * fp.W + nx];
         float ph = target_function(s_lights, sc.num_lights, nb.Y, hit_position);
         update_reservoir(rng, nr, nb.Y, ph * nb.W_X * (float)nb.M, nb.M);
      }
      if (nr.Y != -1) finalize_resampling(nr, target_function(s_lights, sc.num_lights, nr.Y, hit_position));
      im.reservoirs[2][id] = nr;
   }
}

// the reservoir kernels stage the light table per block: no more blocks than the rows at hand can feed
static inline dim3 reservoir_grid(const LaunchCfg& c, const RowSpans& spans) {
   return persistent_grid(spans.total(), c.num_cus * 4);
}
void launch_reset_reservoirs(const LaunchCfg& c, const FrameParams& fp, const Images& im, const RowSpans& spans) {
   if (spans.total()) k_reset_reservoirs<<<stream_grid(c, spans.total()), kBlock, 0, c.stream>>>(im, spans);
}
void launch_initial_ris(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const Images& im, const RowSpans& spans) {
   if (spans.total()) k_initial_ris<<<reservoir_grid(c, spans), kBlock, 0, c.stream>>>(fp, sc, im, spans);
}
void launch_temporal_reuse(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const Images& im, const RowSpans& spans) {
   if (spans.total()) k_temporal_reuse<<<reservoir_grid(c, spans), kBlock, 0, c.stream>>>(fp, sc, im, spans);
}
void launch_spatial_reuse(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const Images& im, const RowSpans& spans) {
   if (spans.total()) k_spatial_reuse<<<reservoir_grid(c, spans), kBlock, 0, c.stream>>>(fp, sc, im, spans);
}

}  // namespace uh
