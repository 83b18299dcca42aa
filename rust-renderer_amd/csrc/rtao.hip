// rtao.hip — ray-traced ambient occlusion in the SSAO slot of the hybrid frame (UH_HYBRID_RTAO; utopian_hip.h): which pixels cast, their
// short cosine-weighted hemisphere rays through the any-hit walk, and the resolve / filter that writes ssao_output; with their launchers.
// An extension: the reference's ambient occlusion is ssao.frag. Arithmetic: DESIGN.md section 2 "Ray-traced ambient occlusion".
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"
#include "traversal.h"

namespace uh {

// One lane per pixel: its count is zeroed, and the geometry pixels (position w != 0) with a finite Nn are appended to a dense queue (one
// atomic per wave, as k_hybrid_restir_classify).
__global__ __launch_bounds__(kBlock) void k_rtao_classify(HybridDev hd, RtaoDev ao) {
   const uint32_t n = hd.W * hd.H, groups = (n + 63) / 64, lane = lane_id();
   for (uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += gridDim.x * kWavesPerBlock) {
      const uint32_t pix = g * 64u + lane;
      bool cast = false;
      if (pix < n) {
         ao.counts[pix] = 0;
         V3 nn;
         cast = hd.pos[pix].w != 0.0f && rtao_normal(hd.nrm[pix], nn);
      }
      const uint32_t slot = wave_append(ao.counters, cast);
      if (cast) ao.queue[slot] = pix;
   }
}

// The rays. Persistent waves with the LDS refill of k_hybrid_restir_trace; the pool carries item numbers alone (the lane that takes one
// makes its ray from the G-buffer and the RNG there). kOrder lays the items out (measured: DESIGN.md section 4 "Ray-traced ambient
// occlusion"):
//   0  item i = ray (queue[i / samples], i % samples): the samples of a pixel are neighbours in a wave
//   1  item i = ray (queue[i % pixels], i / pixels): a wave holds one sample of 64 consecutive queued pixels
//   2  item i = pixel queue[i]: its lane walks the samples one after the other and stores the count once, no atomic
// Orders 0 and 1 add an occluded ray into its pixel's byte with a 32-bit atomic on the word that holds it (a count is at most 64, so no
// byte carries into the next). Integers only: the counts do not depend on the schedule. kCount (option "count_visits"): the walks' node
// visits and triangle tests go to the pass's own counters, one atomic each per wave.
template <int kOrder, bool kCount>
__global__ __launch_bounds__(kBlock, 5) void k_rtao_trace(SceneDev sc, HybridDev hd, RtaoDev ao) {
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   __shared__ RayPool<0> s_pool[kWavesPerBlock];
   const uint32_t lane = lane_id();
   const uint32_t wave = threadIdx.x >> 6;
   uint32_t* lds_col = &s_stack[wave][0][lane];
   RayPool<0>& pool = s_pool[wave];
   const uint32_t pixels = ao.counters[0];
   RaySource src;
   src.queue = nullptr;
   src.count = kOrder == 2 ? pixels : pixels * ao.samples;
   src.cursor = nullptr;
   src.wave_index = blockIdx.x * kWavesPerBlock + wave;
   src.num_waves = gridDim.x * kWavesPerBlock;
   auto source_of = [](int, uint32_t) { return (const float4*)nullptr; };
   Feeder<0> f;
   Trav t;
   t.cur = kEmptyRef;
   t.sp = 0;
   uint32_t pix = 0, s = 0, count = 0, n_nodes = 0, n_tris = 0, n_occluded = 0;
   uint32_t spill[kSpillStack];
   // ray s of pixel pix, from the pixel's own texels
   auto start_ray = [&]() {
      const float4 P4 = hd.pos[pix];
      V3 nn;
      rtao_normal(hd.nrm[pix], nn);
      const V3 o = offset_ray(v3(P4.x, P4.y, P4.z), nn);
      uint32_t rng = init_rng(pix % hd.W, pix / hd.W, hd.W, ao.frame_base + s);
      const V3 u = normalize3(random_point_in_unit_sphere(rng));
      const V3 w = nn + u;
      const V3 d = !(dot3(w, w) >= 1e-12f) ? nn : normalize3(w);
      trav_init(t, make_float4(o.x, o.y, o.z, 0.001f), make_float4(d.x, d.y, d.z, 10000.0f), 0.001f, 10000.0f, ao.radius);
   };
   auto take = [&](uint32_t slot) {
      const uint32_t item = pool.id[slot];
      if (kOrder == 0) {
         pix = ao.queue[item / ao.samples];
         s = item % ao.samples;
      } else if (kOrder == 1) {
         pix = ao.queue[item % pixels];
         s = item / pixels;
      } else {
         pix = ao.queue[item];
         s = 0;
         count = 0;
      }
      start_ray();
   };
   while (refill_lanes<0>(f, src, pool, t.cur == kEmptyRef, source_of, take)) {
      if (t.cur != kEmptyRef) {
         bool occluded = false;
         if (trav_step<true, kCount>(sc.nodes, sc.tris, t, lds_col, spill, occluded, n_nodes, n_tris)) {
            if (occluded) n_occluded++;
            if (kOrder == 2) {
               if (occluded) count++;
               if (++s < ao.samples)
                  start_ray();  // the lane stays busy: its pixel's next sample
               else
                  ao.counts[pix] = (uint8_t)count;
            } else if (occluded) {
               atomicAdd((uint32_t*)ao.counts + (pix >> 2), 1u << (8u * (pix & 3u)));
            }
         }
      }
   }
   for (int off = 32; off > 0; off >>= 1) n_occluded += __shfl_down(n_occluded, off);  // one atomic per wave
   if (lane == 0 && n_occluded) atomicAdd(&ao.counters[1], n_occluded);
   if (kCount) {
      for (int off = 32; off > 0; off >>= 1) n_nodes += __shfl_down(n_nodes, off), n_tris += __shfl_down(n_tris, off);
      if (lane == 0) {
         atomicAdd((unsigned long long*)(ao.counters + 2), (unsigned long long)n_nodes);
         atomicAdd((unsigned long long*)(ao.counters + 4), (unsigned long long)n_tris);
      }
   }
}

// ao of a pixel that cast: 1 - strength * (count / samples)
__device__ __forceinline__ float rtao_raw(const RtaoDev& ao, uint32_t count) { return 1.0f - ao.strength * ((float)count / (float)ao.samples); }

// The resolve / filter: a block is a kAoTileW x kAoTileH tile of G-buffer pixels, one lane per pixel, which writes texel (x, H - 1 - y)
// of ssao_output. kBlur: the tile and its halo (blur_radius <= kAoMaxBlur on every side) of (P, Nn, ao) are staged in LDS once per
// block; s_valid says which records can be taps (inside the frame, a pixel that cast). Tiles are numbered along x first.
constexpr int kAoTileW = 32, kAoTileH = kBlock / kAoTileW, kAoMaxBlur = 4;
constexpr int kAoHaloW = kAoTileW + 2 * kAoMaxBlur, kAoHaloH = kAoTileH + 2 * kAoMaxBlur;
template <bool kBlur>
__global__ __launch_bounds__(kBlock) void k_rtao_resolve(HybridDev hd, RtaoDev ao, uint16_t* __restrict__ ssao) {
   // seven planes of the staged records: P, Nn, ao; s_valid: the record is a tap candidate
   __shared__ float s_rec[kBlur ? 7 : 1][kBlur ? kAoHaloW * kAoHaloH : 1];
   __shared__ uint8_t s_valid[kBlur ? kAoHaloW * kAoHaloH : 1];
   const int W = (int)hd.W, H = (int)hd.H, r = (int)ao.blur_radius;  // r <= kAoMaxBlur (uh_set_rtao_params)
   const int tx = (int)threadIdx.x % kAoTileW, ty = (int)threadIdx.x / kAoTileW;
   const int tiles_x = (W + kAoTileW - 1) / kAoTileW;
   const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * kAoTileW, y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * kAoTileH;
   const int px = x0 + tx, py = y0 + ty;
   if (kBlur) {
      const int hw = kAoTileW + 2 * r, hh = kAoTileH + 2 * r;  // the halo this radius needs, rows of hw records
      for (int i = (int)threadIdx.x; i < hw * hh; i += kBlock) {
         const int gx = x0 - r + i % hw, gy = y0 - r + i / hw;
         bool valid = false;
         if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            const float4 P4 = hd.pos[g];
            V3 nn;
            valid = P4.w != 0.0f && rtao_normal(hd.nrm[g], nn);
            if (valid) {
               s_rec[0][i] = P4.x, s_rec[1][i] = P4.y, s_rec[2][i] = P4.z;
               s_rec[3][i] = nn.x, s_rec[4][i] = nn.y, s_rec[5][i] = nn.z;
               s_rec[6][i] = rtao_raw(ao, ao.counts[g]);
            }
         }
         s_valid[i] = valid ? 1 : 0;
      }
      __syncthreads();
   }
   if (px >= W || py >= H) return;
   const size_t out = (size_t)(H - 1 - py) * W + px;
   if (!kBlur) {
      const size_t g = (size_t)py * W + px;
      V3 nn;
      const bool cast = hd.pos[g].w != 0.0f && rtao_normal(hd.nrm[g], nn);
      ssao[out] = (uint16_t)(cast ? unorm16(rtao_raw(ao, ao.counts[g])) : 65535u);
      return;
   }
   const int hw = kAoTileW + 2 * r;
   const int centre = (ty + r) * hw + (tx + r);
   if (!s_valid[centre]) {
      ssao[out] = 65535;
      return;
   }
   const V3 P = v3(s_rec[0][centre], s_rec[1][centre], s_rec[2][centre]), nn = v3(s_rec[3][centre], s_rec[4][centre], s_rec[5][centre]);
   float sum = 0.0f;
   uint32_t taps = 0;
   for (int dy = -r; dy < r; dy++) {
      for (int dx = -r; dx < r; dx++) {
         const int i = centre + dy * hw + dx;
         bool counts = dx == 0 && dy == 0;
         if (!counts && s_valid[i]) {
            const V3 Pt = v3(s_rec[0][i], s_rec[1][i], s_rec[2][i]), nt = v3(s_rec[3][i], s_rec[4][i], s_rec[5][i]);
            counts = dot3(nt, nn) >= ao.blur_normal_cos && fabsf(dot3(Pt - P, nn)) <= ao.blur_plane;
         }
         if (counts) {
            sum = sum + s_rec[6][i];
            taps++;
         }
      }
   }
   ssao[out] = (uint16_t)unorm16(sum / (float)taps);
}

void launch_rtao_trace(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const RtaoDev& ao, uint32_t order) {
   const uint32_t n = hd.W * hd.H;
   k_rtao_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(hd, ao);
   // at most one lane per item the whole frame could queue, at most the persistent grid of the other any-hit passes
   const uint64_t items = (uint64_t)n * (order == 2 ? 1u : ao.samples);
   const uint64_t need = (items + kBlock - 1) / kBlock;
   const uint32_t full = c.num_cus * c.shadow_blocks_per_cu;
   const dim3 grid((uint32_t)(need < full ? need : full));
   as_constant(c.count_visits, [&](auto count) {
      constexpr bool kCount = decltype(count)::value;
      if (order == 0)
         k_rtao_trace<0, kCount><<<grid, kBlock, 0, c.stream>>>(sc, hd, ao);
      else if (order == 1)
         k_rtao_trace<1, kCount><<<grid, kBlock, 0, c.stream>>>(sc, hd, ao);
      else
         k_rtao_trace<2, kCount><<<grid, kBlock, 0, c.stream>>>(sc, hd, ao);
   });
}

void launch_rtao_resolve(const LaunchCfg& c, const HybridDev& hd, const RtaoDev& ao, uint16_t* ssao) {
   const dim3 grid(((hd.W + kAoTileW - 1) / kAoTileW) * ((hd.H + kAoTileH - 1) / kAoTileH));
   if (ao.blur_radius)
      k_rtao_resolve<true><<<grid, kBlock, 0, c.stream>>>(hd, ao, ssao);
   else
      k_rtao_resolve<false><<<grid, kBlock, 0, c.stream>>>(hd, ao, ssao);
}

}  // namespace uh
