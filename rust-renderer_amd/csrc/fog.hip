// fog.hip — volumetric fog with ray-traced sun shafts behind the sky pass of the hybrid frame (UH_HYBRID_FOG; utopian_hip.h): which pixels
// march, the any-hit walk of their samples' sun rays into per-pixel bit masks, the resolve / filter that turns a mask into (a, Ttot, F,
// Ff), and the composite into deferred_output; with their launchers. An extension: the reference has no participating medium.
// Arithmetic: DESIGN.md section 2 "Volumetric fog". The walk answers with integers only, so nothing here depends on the schedule.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "edge_filter.h"
#include "hybrid_shading.h"
#include "item_walk.h"
#include "kernel_common.h"
#include "traversal.h"

namespace uh {

// The march of pixel pix: the sky pass's view ray (o, d). A sky pixel (position w == 0) marches along d over max_distance; a geometry
// pixel toward its position P over min(|P - o|, max_distance), when |P - o| is finite and > 0. False: the pixel does not march.
__device__ __forceinline__ bool fog_ray(const FrameParams& fp, const HybridDev& hd, const FogDev& fg, uint32_t pix, V3& o, V3& dir, float& D) {
   V3 d;
   primary_ray(fp, pix % hd.W, pix / hd.W, 0.5f, 0.5f, o, d);
   const float4 P4 = hd.pos[pix];
   if (P4.w == 0.0f) {
      dir = d;
      D = fg.max_distance;
      return true;
   }
   const V3 V = v3(P4.x, P4.y, P4.z) - o;
   const float D0 = sqrtf(dot3(V, V));
   if (!(D0 > 0.0f && D0 < INFINITY)) return false;  // NaN: false
   dir = v3(V.x / D0, V.y / D0, V.z / D0);
   D = fminf(D0, fg.max_distance);
   return true;
}

// Every pixel's mask is zeroed and its march length written (0: it does not march); the pixels that march are queued.
__global__ __launch_bounds__(kBlock) void k_fog_classify(FrameParams fp, HybridDev hd, FogDev fg) {
   queue_pixels(hd.W * hd.H, fg.counters, fg.queue, [&](uint32_t pix) {
      fg.mask[pix] = 0;
      V3 o, dir;
      float D;
      const bool marches = fog_ray(fp, hd, fg, pix, o, dir, D);
      fg.dist[pix] = marches ? D : 0.0f;
      return marches;
   });
}

// The sun rays of the samples, an item walk (item_walk.h): the lane that takes an item makes the pixel's view ray and jitter there, and
// sample k's ray from X_k = o + dir * ((k + xi) * dt) toward the sun (no offset_ray: X_k lies on no surface). kOrder lays the items out
// (measured: DESIGN.md section 4 "Volumetric fog"):
//   0  item i = sample (queue[i / steps], i % steps): the samples of a pixel are neighbours in a wave
//   1  item i = sample (queue[i % pixels], i / pixels): a wave holds one sample index of 64 consecutive queued pixels
//   2  item i = pixel queue[i]: its lane walks the samples one after the other and stores the mask once, no atomic
// Orders 0 and 1 set the bit of a ray that reached the sun with atomicOr on the pixel's word. Integers only. kCount (option
// "count_visits"): the walks' node visits and triangle tests go to the pass's own counters, one atomic each per wave.
template <int kOrder, bool kCount>
__global__ __launch_bounds__(kBlock, 5) void k_fog_trace(FrameParams fp, SceneDev sc, HybridDev hd, FogDev fg) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   const uint32_t pixels = fg.counters[0];
   ItemWalk w(s_walk, t, spill, nullptr, kOrder == 2 ? pixels : pixels * fg.steps);
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   uint32_t pix = 0, k = 0, bits = 0, n_lit = 0;
   V3 o = v3(0.0f, 0.0f, 0.0f), dir = o;
   float dt = 0.0f, xi = 0.0f;
   // sample k of the lane's pixel
   auto start_ray = [&]() {
      const V3 X = o + dir * (((float)k + xi) * dt);
      trav_init(t, make_float4(X.x, X.y, X.z, 0.001f), make_float4(sun.x, sun.y, sun.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   auto start = [&](uint32_t item) {
      if (kOrder == 0) {
         pix = fg.queue[item / fg.steps];
         k = item % fg.steps;
      } else if (kOrder == 1) {
         pix = fg.queue[item % pixels];
         k = item / pixels;
      } else {
         pix = fg.queue[item];
         k = 0;
         bits = 0;
      }
      float D;
      fog_ray(fp, hd, fg, pix, o, dir, D);  // a queued pixel marches
      dt = D / (float)fg.steps;
      uint32_t rng = init_rng(pix % hd.W, pix / hd.W, hd.W, fg.frame_seed);
      xi = random_float(rng);
      start_ray();
   };
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<true, kCount>(w, sc, occluded)) {
         if (!occluded) n_lit++;
         if (kOrder == 2) {
            if (!occluded) bits |= 1u << k;
            if (++k < fg.steps)
               start_ray();  // the lane stays busy: its pixel's next sample
            else
               fg.mask[pix] = bits;
         } else if (!occluded) {
            atomicOr(&fg.mask[pix], 1u << k);
         }
      }
   }
   wave_add(&fg.counters[1], n_lit);
   if (kCount) {
      wave_add((unsigned long long*)(fg.counters + 2), w.n_nodes);
      wave_add((unsigned long long*)(fg.counters + 4), w.n_tris);
   }
}

// (a, Ttot, F) of a pixel that marched over D and whose samples left the mask m: one transcendental, then the samples front to back
__device__ __forceinline__ void fog_terms(const FogDev& fg, float D, uint32_t m, float& a, float& Ttot, float& F) {
   const float dt = D / (float)fg.steps;
   a = expf(-(fg.density * dt));
   float p = 1.0f, sum = 0.0f;
   for (uint32_t k = 0; k < fg.steps; k++) {
      if ((m >> k) & 1u) sum = sum + p;
      p = p * a;
   }
   Ttot = p;
   F = (1.0f - a) * sum;
}

// The resolve / filter over the tiles of edge_filter.h: a lane writes its pixel's terms. kBlur: Ff is the mean of F over the taps
// (dx, dy) in [-r, r]^2 that marched and lie within blur_depth * D of the centre's march length; blur_radius <= kFogMaxBlur
// (uh_set_fog_params). The value planes of a staged record: D, F.
constexpr int kFogMaxBlur = 4;
template <bool kBlur>
__global__ __launch_bounds__(kBlock) void k_fog_resolve(HybridDev hd, FogDev fg) {
   const int W = (int)hd.W, H = (int)hd.H, r = (int)fg.blur_radius;
   float a, Ttot, F, Ff;
   if constexpr (kBlur) {
      using Tile = FilterTile<kFogMaxBlur, 2>;
      __shared__ Tile::Rec s_rec;
      __shared__ Tile::Valid s_valid;
      Tile s_tile{s_rec, s_valid};
      const FilterLane me = s_tile.stage(
         hd, r, [&](size_t g) { return fg.dist[g] > 0.0f; },
         [&](size_t g, int i) {
            const float D = fg.dist[g];
            float ta, tT, tF;
            fog_terms(fg, D, fg.mask[g], ta, tT, tF);
            s_tile.rec[6][i] = D, s_tile.rec[7][i] = tF;
         });
      if (me.px >= W || me.py >= H) return;
      const size_t g = (size_t)me.py * W + me.px;
      if (!s_tile.valid[me.centre]) {
         fg.terms[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         return;
      }
      fog_terms(fg, fg.dist[g], fg.mask[g], a, Ttot, F);
      float sum = 0.0f;
      const uint32_t taps = s_tile.taps_depth(me.centre, r, s_tile.rec[6], fg.blur_depth, [&](int i) { sum = sum + s_tile.rec[7][i]; });
      Ff = sum / (float)taps;
      fg.terms[g] = make_float4(a, Ttot, F, Ff);
   } else {
      const FilterLane me = filter_lane(hd, 0);
      if (me.px >= W || me.py >= H) return;
      const size_t g = (size_t)me.py * W + me.px;
      const float D = fg.dist[g];
      if (!(D > 0.0f)) {
         fg.terms[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         return;
      }
      fog_terms(fg, D, fg.mask[g], a, Ttot, F);
      fg.terms[g] = make_float4(a, Ttot, F, F);
   }
}

// out = (C Ttot + S Ff) + ambient (1 - Ttot) on every pixel that marched: S the sun's radiance through the Henyey-Greenstein phase
// function of the angle between the sun and the view ray; alpha untouched
__global__ __launch_bounds__(kBlock) void k_fog_composite(FrameParams fp, HybridDev hd, HybridFrameDev fd, FogDev fg) {
   const uint32_t n = hd.W * hd.H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   V3 o, dir;
   float D;
   if (!(fg.dist[i] > 0.0f) || !fog_ray(fp, hd, fg, i, o, dir, D)) return;  // the pixel did not march
   const float4 T = fg.terms[i];
   const float Ttot = T.y, Ff = T.w;
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   const float c = dot3(sun, dir), g = fg.anisotropy;
   const float q = (1.0f + g * g) - (2.0f * g) * c;
   const float ph = (1.0f - g * g) / ((4.0f * kPiBrdf) * (q * sqrtf(q)));
   const V3 rad_sun = v3(1.0f * 1.0f, 1.0f * 1.0f, 1.0f * 1.0f);  // light record 0: color (1, 1, 1) times attenuation 1, as the rtgi pass takes it
   const V3 S = ((v3(fg.albedo[0], fg.albedo[1], fg.albedo[2]) * rad_sun) * ph) * fg.intensity;
   const float4 C4 = fd.deferred[i];
   const V3 out = (v3(C4.x, C4.y, C4.z) * Ttot + S * Ff) + v3(fg.ambient[0], fg.ambient[1], fg.ambient[2]) * (1.0f - Ttot);
   fd.deferred[i] = make_float4(out.x, out.y, out.z, C4.w);
}

void launch_fog_trace(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const HybridDev& hd, const FogDev& fg, uint32_t order) {
   const uint32_t n = hd.W * hd.H;
   k_fog_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(fp, hd, fg);
   const dim3 grid = persistent_grid((uint64_t)n * (order == 2 ? 1u : fg.steps), c.num_cus * c.shadow_blocks_per_cu);
   as_constant(c.count_visits, [&](auto count) {
      constexpr bool kCount = decltype(count)::value;
      if (order == 0)
         k_fog_trace<0, kCount><<<grid, kBlock, 0, c.stream>>>(fp, sc, hd, fg);
      else if (order == 1)
         k_fog_trace<1, kCount><<<grid, kBlock, 0, c.stream>>>(fp, sc, hd, fg);
      else
         k_fog_trace<2, kCount><<<grid, kBlock, 0, c.stream>>>(fp, sc, hd, fg);
   });
}

void launch_fog_resolve(const LaunchCfg& c, const HybridDev& hd, const FogDev& fg) {
   if (fg.blur_radius)
      k_fog_resolve<true><<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, fg);
   else
      k_fog_resolve<false><<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, fg);
}

void launch_fog_composite(const LaunchCfg& c, const FrameParams& fp, const HybridDev& hd, const HybridFrameDev& fd, const FogDev& fg) {
   k_fog_composite<<<dim3((hd.W * hd.H + kBlock - 1) / kBlock), kBlock, 0, c.stream>>>(fp, hd, fd, fg);
}

}  // namespace uh
