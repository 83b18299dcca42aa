// rtao.hip — ray-traced ambient occlusion in the SSAO slot of the hybrid frame (UH_HYBRID_RTAO; utopian_hip.h): which pixels cast, their
// short cosine-weighted hemisphere rays through the any-hit walk, and the resolve / filter that writes ssao_output; with their launchers.
// An extension: the reference's ambient occlusion is ssao.frag. Arithmetic: DESIGN.md section 2 "Ray-traced ambient occlusion".
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "edge_filter.h"
#include "item_walk.h"
#include "kernel_common.h"
#include "traversal.h"

namespace uh {

// Every pixel's count is zeroed; the geometry pixels (position w != 0) with a finite Nn are queued (queue_pixels, kernel_common.h).
__global__ __launch_bounds__(kBlock) void k_rtao_classify(HybridDev hd, RtaoDev ao) {
   queue_pixels(hd.W * hd.H, ao.counters, ao.queue, [&](uint32_t pix) {
      ao.counts[pix] = 0;
      V3 nn;
      return hd.pos[pix].w != 0.0f && rtao_normal(hd.nrm[pix], nn);
   });
}

// The rays, an item walk (item_walk.h): the lane that takes an item makes its ray from the G-buffer and the RNG there. kOrder lays the
// items out (measured: DESIGN.md section 4 "Ray-traced ambient occlusion"):
//   0  item i = ray (queue[i / samples], i % samples): the samples of a pixel are neighbours in a wave
//   1  item i = ray (queue[i % pixels], i / pixels): a wave holds one sample of 64 consecutive queued pixels
//   2  item i = pixel queue[i]: its lane walks the samples one after the other and stores the count once, no atomic
// Orders 0 and 1 add an occluded ray into its pixel's byte with a 32-bit atomic on the word that holds it (a count is at most 64, so no
// byte carries into the next). Integers only: the counts do not depend on the schedule. kCount (option "count_visits"): the walks' node
// visits and triangle tests go to the pass's own counters, one atomic each per wave.
template <int kOrder, bool kCount>
__global__ __launch_bounds__(kBlock, 5) void k_rtao_trace(SceneDev sc, HybridDev hd, RtaoDev ao) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   const uint32_t pixels = ao.counters[0];
   ItemWalk w(s_walk, t, spill, nullptr, kOrder == 2 ? pixels : pixels * ao.samples);
   uint32_t pix = 0, s = 0, count = 0, n_occluded = 0;
   // ray s of pixel pix, from the pixel's own texels
   auto start_ray = [&]() {
      const float4 P4 = hd.pos[pix];
      V3 nn;
      rtao_normal(hd.nrm[pix], nn);
      const V3 o = offset_ray(v3(P4.x, P4.y, P4.z), nn);
      uint32_t rng = init_rng(pix % hd.W, pix / hd.W, hd.W, ao.frame_base + s);
      const V3 u = normalize3(random_point_in_unit_sphere(rng));
      const V3 v = nn + u;
      const V3 d = !(dot3(v, v) >= 1e-12f) ? nn : normalize3(v);
      trav_init(t, make_float4(o.x, o.y, o.z, 0.001f), make_float4(d.x, d.y, d.z, 10000.0f), 0.001f, 10000.0f, ao.radius);
   };
   auto start = [&](uint32_t item) {
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
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<true, kCount>(w, sc, occluded)) {
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
   wave_add(&ao.counters[1], n_occluded);
   if (kCount) {
      wave_add((unsigned long long*)(ao.counters + 2), w.n_nodes);
      wave_add((unsigned long long*)(ao.counters + 4), w.n_tris);
   }
}

// ao of a pixel that cast: 1 - strength * (count / samples)
__device__ __forceinline__ float rtao_raw(const RtaoDev& ao, uint32_t count) { return 1.0f - ao.strength * ((float)count / (float)ao.samples); }

// The resolve / filter over the tiles of edge_filter.h: a lane writes texel (x, H - 1 - y) of ssao_output. kBlur: the mean of the ao over
// the filter's taps (dx, dy) in [-r, r)^2, blur_radius <= kAoMaxBlur (uh_set_rtao_params).
constexpr int kAoMaxBlur = 4;
template <bool kBlur>
__global__ __launch_bounds__(kBlock) void k_rtao_resolve(HybridDev hd, RtaoDev ao, uint16_t* __restrict__ ssao) {
   const int W = (int)hd.W, H = (int)hd.H, r = (int)ao.blur_radius;
   if constexpr (kBlur) {
      using Tile = FilterTile<kAoMaxBlur, 1>;
      __shared__ Tile::Rec s_rec;
      __shared__ Tile::Valid s_valid;
      Tile s_tile{s_rec, s_valid};
      const FilterLane me = s_tile.stage(hd, r, [&](size_t g, int i) { s_tile.rec[6][i] = rtao_raw(ao, ao.counts[g]); });
      if (me.px >= W || me.py >= H) return;
      const size_t out = (size_t)(H - 1 - me.py) * W + me.px;
      if (!s_tile.valid[me.centre]) {
         ssao[out] = 65535;
         return;
      }
      float sum = 0.0f;
      const uint32_t taps = s_tile.taps<false>(me.centre, r, ao.blur_normal_cos, ao.blur_plane, [&](int i) { sum = sum + s_tile.rec[6][i]; });
      ssao[out] = (uint16_t)unorm16(sum / (float)taps);
   } else {
      const FilterLane me = filter_lane(hd, 0);
      if (me.px >= W || me.py >= H) return;
      const size_t g = (size_t)me.py * W + me.px;
      V3 nn;
      const bool cast = hd.pos[g].w != 0.0f && rtao_normal(hd.nrm[g], nn);
      ssao[(size_t)(H - 1 - me.py) * W + me.px] = (uint16_t)(cast ? unorm16(rtao_raw(ao, ao.counts[g])) : 65535u);
   }
}

void launch_rtao_trace(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const RtaoDev& ao, uint32_t order) {
   const uint32_t n = hd.W * hd.H;
   k_rtao_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(hd, ao);
   const dim3 grid = persistent_grid((uint64_t)n * (order == 2 ? 1u : ao.samples), c.num_cus * c.shadow_blocks_per_cu);
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
   if (ao.blur_radius)
      k_rtao_resolve<true><<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, ao, ssao);
   else
      k_rtao_resolve<false><<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, ao, ssao);
}

}  // namespace uh
