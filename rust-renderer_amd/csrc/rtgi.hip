// rtgi.hip — one-bounce ray-traced diffuse GI of the hybrid frame (UH_HYBRID_RTGI; utopian_hip.h): which pixels cast, their cosine-weighted
// hemisphere rays through the closest-hit walk with the hit shaded where the walk ends, the sun rays of the lit candidates through the
// any-hit walk, the per-pixel mean in sample order, the tile filter and the composite into deferred_output; with their launchers.
// An extension: the reference has no GI. Arithmetic: DESIGN.md section 2 "Ray-traced diffuse GI"; tests/rtgi_reference.py restates it.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "edge_filter.h"
#include "hybrid_shading.h"
#include "item_walk.h"
#include "kernel_common.h"
#include "path_shading.h"
#include "traversal.h"

namespace uh {

// the bytes of a pixel's count word
constexpr uint32_t kGiSunlit = 1u, kGiDark = 1u << 8, kGiEmitter = 1u << 16, kGiMissed = 1u << 24;

// L as it is stored: NaN, negatives and -0 become +0, then the cap (max_radiance is finite and > 0): always finite
__device__ __forceinline__ float rtgi_clamp(float x, float cap) { return fminf(x > 0.0f ? x : 0.0f, cap); }
__device__ __forceinline__ float4 rtgi_record(V3 L, float cap) { return make_float4(rtgi_clamp(L.x, cap), rtgi_clamp(L.y, cap), rtgi_clamp(L.z, cap), 0.0f); }

// Every pixel's counts and radiance are zeroed; the pixels that cast (RTAO's rule: position w != 0, Nn finite) are queued (queue_pixels,
// kernel_common.h).
__global__ __launch_bounds__(kBlock) void k_rtgi_classify(HybridDev hd, RtgiDev gi) {
   queue_pixels(hd.W * hd.H, gi.counters, gi.queue, [&](uint32_t pix) {
      gi.counts[pix] = 0;
      gi.radiance[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      V3 nn;
      return hd.pos[pix].w != 0.0f && rtao_normal(hd.nrm[pix], nn);
   });
}

// The hemisphere rays: closest hit, an item walk (item_walk.h): the lane that takes an item makes its ray from the G-buffer and the RNG
// there. kOrder lays the items out (measured: DESIGN.md section 4 "Ray-traced diffuse GI"):
//   0  item i = ray (queue[i / samples], i % samples): the samples of a pixel are neighbours in a wave
//   1  item i = ray (queue[i % pixels], i / pixels): a wave holds one sample of 64 consecutive queued pixels
// A lane whose walk ends shades its own ray - not at once: it waits, out of the walk and not yet idle, until kGiShadeBatch lanes of its
// wave wait with it or no lane walks any more, and they shade together (shading is three dependent round trips to memory - the shading
// packet, the mesh and texture records, the texels - or the sky integral; a lane at a time the wave paid them once per ray). Measured at
// 1, 16, 32 and 64 lanes: the whole wave is fastest, so a wave walks its rays, shades them together and refills.
// A miss, an emitter and a dark hit are final: the ray's record and its byte of the pixel's count word (a 32-bit atomic on the word: a
// byte never exceeds 16, so none carries; integers only, so the counts do not depend on the schedule). A hit the sun may light stores
// the radiance it would have and appends its sun ray to gi.sun_rays, one atomic per wave and batch; k_rtgi_shadow decides.
// A miss takes the sky integral with exact heights (sky::integrate_scattering_exact_heights, device_math.h): one ray is a third or all
// of a pixel's value here, and with the hardware square root a ray next to the sun was 1.1e-4 off the oracle's.
constexpr uint32_t kGiShadeBatch = 64;  // lanes that wait before the wave shades: 64 = when none of its lanes walks any more
template <int kOrder>
__global__ __launch_bounds__(kBlock, 5) void k_rtgi_trace(SceneDev sc, HybridDev hd, RtgiDev gi) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   const uint32_t pixels = gi.counters[0];
   ItemWalk w(s_walk, t, spill, nullptr, pixels * gi.samples);
   uint32_t pix = 0, ray = 0, n_missed = 0;
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   auto start = [&](uint32_t item) {
      uint32_t q, s;
      if (kOrder == 0) {
         q = item / gi.samples;
         s = item % gi.samples;
      } else {
         q = item % pixels;
         s = item / pixels;
      }
      pix = gi.queue[q];
      ray = q * gi.samples + s;
      const float4 P4 = hd.pos[pix];
      V3 nn;
      rtao_normal(hd.nrm[pix], nn);
      const V3 o = offset_ray(v3(P4.x, P4.y, P4.z), nn);
      uint32_t rng = init_rng(pix % hd.W, pix / hd.W, hd.W, (gi.frame_base + s) ^ kRtgiSeedXor);
      const V3 u = normalize3(random_point_in_unit_sphere(rng));
      const V3 v = nn + u;
      const V3 d = !(dot3(v, v) >= 1e-12f) ? nn : normalize3(v);
      trav_init(t, make_float4(o.x, o.y, o.z, 0.001f), make_float4(d.x, d.y, d.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   bool pending = false;  // the lane's walk has ended and its ray is not shaded yet
   while (w.next(pending, start)) {
      bool occluded;
      if (walk_step<false, false>(w, sc, occluded)) pending = true;
      const uint32_t n_pending = (uint32_t)__popcll(__ballot(pending));
      if (n_pending != 0 && (n_pending >= kGiShadeBatch || __ballot(w.walking()) == 0ull)) {
         bool want_sun = false;
         V3 sun_origin = v3(0.0f, 0.0f, 0.0f);
         if (pending) {
            pending = false;
            V3 L = v3(0.0f, 0.0f, 0.0f);
            uint32_t kind = kGiDark;
            if (t.best.idx == kEmptyRef) {
               kind = kGiMissed;
               n_missed++;
               L = hd.furnace ? v3(1.0f, 1.0f, 1.0f) : sky::integrate_scattering_exact_heights(t.o, t.d, 999999999.0f, sun);  // rmiss:12 / :16-19, unclamped
            } else {
               const float4* sp = sc.shade + 4 * (size_t)t.best.idx;
               const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
               const MeshShade ms = sc.meshes[__float_as_uint(s3.w)];
               if (ms.type == 3.0f) {
                  kind = kGiEmitter;
                  L = v3(1.0f, 1.0f, 1.0f);                                                      // rchit:85-89: the path ends with color = vec3(1.0)
               } else if (!hd.furnace) {
                  V3 normal;
                  float uu, vv;
                  surface_normal_uv(s0, s1, s2, s3, t.best.u, t.best.v, normal, uu, vv);         // rchit:30,39
                  V3 albedo = sample_texture(sc, sc.unorm_lut, ms.diffuse_map, uu, vv);          // rchit:41
                  albedo = albedo * v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);    // rchit:42
                  const V3 Nh = world_normal_of(ms, normal, t.d);                                // rchit:32-37
                  const V3 X = t.o + t.best.t * t.d;
                  const float NdotL = fmaxf(dot3(Nh, sun), 0.0f);
                  if (NdotL > 0.0f) {                                                            // 0 or NaN: dark, no sun ray
                     const V3 rad_sun = v3(1.0f * 1.0f, 1.0f * 1.0f, 1.0f * 1.0f);               // light record 0: color (1, 1, 1) times attenuation 1
                     L = ((v3(albedo.x / kPiBrdf, albedo.y / kPiBrdf, albedo.z / kPiBrdf)) * rad_sun) * NdotL;
                     want_sun = true;
                     sun_origin = offset_ray(X, Nh);
                  }
               }
            }
            gi.rays[ray] = rtgi_record(L, gi.max_radiance);
            if (!want_sun) atomicAdd(gi.counts + pix, kind);
         }
         const uint32_t slot = wave_append(gi.counters + 1, want_sun);
         if (want_sun) gi.sun_rays[slot] = make_float4(sun_origin.x, sun_origin.y, sun_origin.z, __uint_as_float(ray));
      }
   }
   wave_add(&gi.counters[2], n_missed);
}

// One any-hit ray toward the sun per queued record, an item walk over the record numbers. An occluded ray zeroes its radiance record and
// counts as dark, an unoccluded one keeps it and counts as sunlit.
__global__ __launch_bounds__(kBlock, 5) void k_rtgi_shadow(SceneDev sc, HybridDev hd, RtgiDev gi) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   ItemWalk w(s_walk, t, spill, nullptr, gi.counters[1]);
   uint32_t ray = 0;
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   auto start = [&](uint32_t item) {
      const float4 r = ld_stream(gi.sun_rays + item);
      ray = __float_as_uint(r.w);
      trav_init(t, make_float4(r.x, r.y, r.z, 0.001f), make_float4(sun.x, sun.y, sun.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<true, false>(w, sc, occluded)) {
         if (occluded) gi.rays[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         atomicAdd(gi.counts + gi.queue[ray / gi.samples], occluded ? kGiDark : kGiSunlit);
      }
   }
}

// E of the pixel in queue slot q: (L_0 + L_1 + ... + L_{samples - 1}) / (float)samples, one lane walking the samples in order
__global__ __launch_bounds__(kBlock) void k_rtgi_mean(RtgiDev gi, float4* __restrict__ out) {
   const uint32_t pixels = gi.counters[0];
   for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < pixels; q += gridDim.x * kBlock) {
      const float4* L = gi.rays + (size_t)q * gi.samples;
      V3 sum = xyz(L[0]);
      for (uint32_t s = 1; s < gi.samples; s++) sum = sum + xyz(L[s]);
      const float n = (float)gi.samples;
      out[gi.queue[q]] = make_float4(sum.x / n, sum.y / n, sum.z / n, 1.0f);
   }
}

// The filter over the tiles of edge_filter.h: the mean of E over the filter's taps (dx, dy) in [-r, r]^2, 1 <= blur_radius <= kGiMaxBlur
// (uh_set_rtgi_params, launch_rtgi_filter).
constexpr int kGiMaxBlur = 6;
__global__ __launch_bounds__(kBlock) void k_rtgi_filter(HybridDev hd, RtgiDev gi) {
   using Tile = FilterTile<kGiMaxBlur, 3>;
   __shared__ Tile::Rec s_rec;
   __shared__ Tile::Valid s_valid;
   Tile s_tile{s_rec, s_valid};
   const int r = (int)gi.blur_radius;
   const FilterLane me = s_tile.stage(hd, r, [&](size_t g, int i) {
      const float4 E = gi.mean[g];
      s_tile.rec[6][i] = E.x, s_tile.rec[7][i] = E.y, s_tile.rec[8][i] = E.z;
   });
   if (me.px >= (int)hd.W || me.py >= (int)hd.H || !s_tile.valid[me.centre]) return;  // not a pixel that cast: (0, 0, 0, 0) from the classify
   V3 sum = v3(0.0f, 0.0f, 0.0f);
   const float n = (float)s_tile.taps<true>(me.centre, r, gi.blur_normal_cos, gi.blur_plane,
                                            [&](int i) { sum = sum + v3(s_tile.rec[6][i], s_tile.rec[7][i], s_tile.rec[8][i]); });
   gi.radiance[(size_t)me.py * hd.W + me.px] = make_float4(sum.x / n, sum.y / n, sum.z / n, 1.0f);
}

// The composite, one lane per pixel that cast: deferred_output.rgb += ((base (1 - metallic)) Ef) intensity, times the occlusion and (with
// ssao_enabled) the pixel's ssao texel - base, metallic and the texel's index as k_hybrid_deferred forms them (frag:52-65, :113-115). A
// metal pixel with raytracing_supported = 1 holds its reflection and is left as it is. The gamma table as k_hybrid_deferred has it.
__global__ __launch_bounds__(kBlock) void k_rtgi_composite(SceneDev sc, HybridDev hd, HybridFrameDev fd, RtgiDev gi) {
   __shared__ float s_gamma[256];  // pow(c / 255, 2.2) of every UNORM8 value: pow in double, rounded to float
   s_gamma[threadIdx.x] = (float)pow((double)((float)threadIdx.x / 255.0f), (double)2.2f);
   __syncthreads();
   const uint32_t n = hd.W * hd.H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   const float4 Ef = gi.radiance[i];
   if (Ef.w == 0.0f) return;  // the pixel did not cast
   const float4 R4 = hd.pbr[i];
   const uchar4 A = hd.alb[i];
   const uint32_t material = (uint32_t)R4.w;                                                    // frag:46
   float mf = 1.0f, type = 0.0f;
   V3 bc = v3(1.0f, 1.0f, 1.0f);
   if (material < sc.num_meshes) {
      const MeshShade& ms = sc.meshes[material];
      mf = ms.metallic;
      type = ms.type;
      bc = v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);
   }
   if (fd.rt_on && type == 1.0f) return;                                                        // frag:92-95 replaced the colour
   const float metallic = R4.x * mf, occlusion = R4.z;                                          // frag:52-58
   const V3 base = v3(s_gamma[A.x], s_gamma[A.y], s_gamma[A.z]) * bc;                           // frag:61-65
   V3 add = ((base * (1.0f - metallic)) * v3(Ef.x, Ef.y, Ef.z)) * gi.intensity;
   add = add * occlusion;
   if (fd.ssao_on) add = add * ((float)fd.ssao[(size_t)(hd.H - 1 - i / hd.W) * hd.W + i % hd.W] / 65535.0f);
   const float4 d = fd.deferred[i];
   fd.deferred[i] = make_float4(d.x + add.x, d.y + add.y, d.z + add.z, d.w);
}

void launch_rtgi_trace(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const RtgiDev& gi, uint32_t order) {
   const uint32_t n = hd.W * hd.H;
   k_rtgi_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(hd, gi);
   const dim3 grid = persistent_grid((uint64_t)n * gi.samples, c.num_cus * c.closest_blocks_per_cu);
   if (order == 0)
      k_rtgi_trace<0><<<grid, kBlock, 0, c.stream>>>(sc, hd, gi);
   else
      k_rtgi_trace<1><<<grid, kBlock, 0, c.stream>>>(sc, hd, gi);
}

void launch_rtgi_shadow(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const RtgiDev& gi) {
   const dim3 grid = persistent_grid((uint64_t)hd.W * hd.H * gi.samples, c.num_cus * c.shadow_blocks_per_cu);
   k_rtgi_shadow<<<grid, kBlock, 0, c.stream>>>(sc, hd, gi);
}

void launch_rtgi_filter(const LaunchCfg& c, const HybridDev& hd, const RtgiDev& gi) {
   k_rtgi_mean<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(gi, gi.blur_radius ? gi.mean : gi.radiance);
   if (!gi.blur_radius) return;  // Ef = E
   k_rtgi_filter<<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, gi);
}

void launch_rtgi_composite(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const HybridFrameDev& fd, const RtgiDev& gi) {
   k_rtgi_composite<<<dim3((hd.W * hd.H + kBlock - 1) / kBlock), kBlock, 0, c.stream>>>(sc, hd, fd, gi);
}

}  // namespace uh
