// glass.hip — ray-traced glass of the hybrid frame (UH_HYBRID_GLASS; utopian_hip.h): which pixels cast (material type 2), the first event
// at the G-buffer's surface, which starts a reflected and a transmitted chain per pixel, then rounds of a closest-hit walk and a bend
// kernel: a segment that ends on glass produces the chain's next segment, any other end settles the chain. The rounds' ray lists are two
// queues that swap, each round's count is a device counter of its own, and the host enqueues max_events rounds without reading anything
// back. Then the sun rays of the lit ends through k_rtgi_shadow (rtgi.hip) and the composite, which replaces deferred_output.rgb.
// The walk is glossy.hip's k_glossy_trace, unchanged, on this pass's buffers (glass_walk_view): it writes hit records and nothing else.
// The event at an interface is reference.rchit:61-83 as material_scatter (path_shading.h) states it, without the draw. The hit normal
// has already been turned toward the ray (rchit:35-37), so dot(nd, N) <= 0 and the ratio is 1 / ior on the way out of the glass as well
// as on the way in: that is the reference's behaviour, k_shade_hit reproduces it, and this pass shows the glass the path tracer shows.
// Arithmetic: DESIGN.md section 2 "Ray-traced glass"; tests/glass_reference.py restates it.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "hybrid_shading.h"
#include "kernel_common.h"
#include "path_shading.h"

namespace uh {

// the bytes of a pixel's count word above the lowest (sunlit: k_rtgi_shadow adds the sun rays' verdicts), as the rtgi pass has them
constexpr uint32_t kGsDark = 1u << 8, kGsEmitter = 1u << 16, kGsMissed = 1u << 24;

// L as it is stored, and C: rtgi_clamp (rtgi.hip) with this pass's cap
__device__ __forceinline__ float gs_clamp(float x, float cap) { return fminf(x > 0.0f ? x : 0.0f, cap); }
__device__ __forceinline__ bool gs_finite(V3 a) { return fabsf(a.x) < INFINITY && fabsf(a.y) < INFINITY && fabsf(a.z) < INFINITY; }

// rchit:62-79 as material_scatter has them (path_shading.h:187-199), both outcomes and no draw. nd: the normalised ray direction
struct GlassEvent {
   V3 R, T;
   float Fr;
   bool cannot;
};
__device__ __forceinline__ GlassEvent glass_event(V3 nd, V3 N, float ior) {
   GlassEvent e;
   const float dnd = dot3(nd, N);
   const V3 outward = dnd > 0 ? vneg(N) : N;
   float ratio = ior;
   ratio = dnd > 0 ? ratio : 1.0f / ratio;
   const float cos_theta = fminf(dot3(-1.0f * nd, outward), 1.0f);
   const float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
   e.cannot = ratio * sin_theta > 1.0f;
   e.Fr = schlick_reflectance(cos_theta, ratio);
   e.R = reflect3(nd, outward);
   e.T = refract3(nd, outward, ratio);
   return e;
}

// What a pixel that casts hands its two chains: RTGI's rule, then a material in range and of type 2, then I = normalize(P - eye) finite
struct GlassPixel {
   V3 P, Nf, I;
   float ior;
};
__device__ __forceinline__ bool glass_pixel(const SceneDev& sc, const HybridDev& hd, uint32_t pix, GlassPixel& g) {
   const float4 P4 = hd.pos[pix];
   V3 Nn;
   if (!(P4.w != 0.0f && rtao_normal(hd.nrm[pix], Nn))) return false;
   const uint32_t material = (uint32_t)hd.pbr[pix].w;  // frag:46
   if (material >= sc.num_meshes) return false;        // out of range counts as type 0
   const MeshShade& ms = sc.meshes[material];
   if (ms.type != 2.0f) return false;
   g.ior = ms.property;
   g.P = v3(P4.x, P4.y, P4.z);
   g.I = normalize3(g.P - v3(hd.eye[0], hd.eye[1], hd.eye[2]));
   if (!gs_finite(g.I)) return false;
   g.Nf = dot3(Nn, g.I) > 0.0f ? vneg(Nn) : Nn;
   return true;
}

// Every pixel's three images are zeroed; the pixels that cast are queued (queue_pixels).
__global__ __launch_bounds__(kBlock) void k_glass_classify(SceneDev sc, HybridDev hd, GlassDev gs) {
   queue_pixels(hd.W * hd.H, gs.counters, gs.queue, [&](uint32_t pix) {
      gs.counts[pix] = 0;
      gs.events[pix] = 0;
      gs.radiance[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      GlassPixel g;
      return glass_pixel(sc, hd, pix, g);
   });
}

// The streaming kernels batch their appends as glossy.hip's do: a wave takes kGlBatch rounds of 64 items, keeps each round's ballot and
// reserves the slots of all of them with one atomic (wave_reserve, device_math.h). Items are numbered in 64 bits.
constexpr int kGlBatch = 4;

// Ray generation, two lanes per queued pixel (item i = chain i % 2 of queue slot i / 2): the first event, Event(I, Nf, ior). Chain 0 takes
// R with the weight cannot ? 1 : Fr, chain 1 takes T with 1 - Fr; with `cannot` chain 1 is not cast and is settled here - an all-zero
// record, a dark count, flag bit 0 - and never reaches the walk. Both start at offset_ray(P, Nf) with events = 1.
__global__ __launch_bounds__(kBlock) void k_glass_raygen(SceneDev sc, HybridDev hd, GlassDev gs) {
   const uint32_t n = gs.counters[0] * 2u, groups = (uint32_t)(((uint64_t)n + 64u * kGlBatch - 1) / (64u * kGlBatch)), lane = lane_id();
   uint32_t n_tir = 0;
   for (uint32_t grp = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); grp < groups; grp += gridDim.x * kWavesPerBlock) {
      unsigned long long masks[kGlBatch];
      uint32_t total = 0;
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         const uint64_t item = ((uint64_t)grp * kGlBatch + j) * 64u + lane;
         const uint32_t ray = (uint32_t)item;
         bool queued = false;
         if (item < n) {
            const uint32_t pix = gs.queue[ray >> 1];
            GlassPixel g;
            glass_pixel(sc, hd, pix, g);
            const GlassEvent e = glass_event(g.I, g.Nf, g.ior);
            const bool transmitted = (ray & 1u) != 0;
            if (transmitted && e.cannot) {
               gs.rays[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
               atomicAdd(gs.counts + pix, kGsDark);
               atomicAdd(gs.events + pix, kGlassTir);
               n_tir++;
            } else {
               const V3 o = offset_ray(g.P, g.Nf), d = transmitted ? e.T : e.R;
               const float w = transmitted ? 1.0f - e.Fr : (e.cannot ? 1.0f : e.Fr);
               gs.orig[ray] = make_float4(o.x, o.y, o.z, w);
               gs.dirs[ray] = make_float4(d.x, d.y, d.z, __uint_as_float(1u));
               queued = true;
            }
         }
         masks[j] = __ballot(queued);
         total += (uint32_t)__popcll(masks[j]);
      }
      uint32_t slot = wave_reserve(gs.counters + kGlassRound0, total);
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         if ((masks[j] >> lane) & 1ull) gs.ray_queue[0][slot + ballot_prefix(masks[j])] = (uint32_t)(((uint64_t)grp * kGlBatch + j) * 64u + lane);
         slot += (uint32_t)__popcll(masks[j]);
      }
   }
   wave_add(&gs.counters[4], n_tir);
}

// The bend of round `round`, one lane per ray of the round's queue (whole waves: both appends are batched). The segment's end:
//   a miss       L the sky as the rtgi pass takes it ((1, 1, 1) under furnace), counted missed
//   type 3       L = (1, 1, 1), counted emitter
//   type 2       with events == max_events the chain is cut: L = 0, counted dark, its cut flag set. Else Event(normalize(d), Nh, the
//                mesh's ior) and d' = cannot ? R : T, unnormalised (rgen:61); d' not finite or of length 0 cuts the chain as well. Else
//                the next segment (offset_ray(o + t d, Nh), d') replaces this one, events + 1, and the ray is listed for the next round
//   other types  the rtgi pass's Lambert lines, one any-hit sun ray from offset_ray(X, Nh); dark under furnace
// A chain that ends stores w clamp(L), adds its events and flags to the pixel's events word and - unless a sun ray decides - its count.
__global__ __launch_bounds__(kBlock) void k_glass_bend(SceneDev sc, HybridDev hd, GlassDev gs, uint32_t round) {
   const uint32_t n = gs.counters[kGlassRound0 + round], groups = (uint32_t)(((uint64_t)n + 64u * kGlBatch - 1) / (64u * kGlBatch)), lane = lane_id();
   const uint32_t* const in = gs.ray_queue[round & 1u];
   uint32_t* const out = gs.ray_queue[(round + 1u) & 1u];
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   uint32_t n_missed = 0, n_tir = 0, n_cut = 0;
   for (uint32_t grp = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); grp < groups; grp += gridDim.x * kWavesPerBlock) {
      unsigned long long sun_masks[kGlBatch], next_masks[kGlBatch];
      float4 sun_ray[kGlBatch];  // a round's sun ray: origin.xyz, ray number (bits)
      uint32_t next_ray[kGlBatch];
      uint32_t sun_total = 0, next_total = 0;
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         const uint64_t item = ((uint64_t)grp * kGlBatch + j) * 64u + lane;
         bool want_sun = false, goes_on = false;
         sun_ray[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         next_ray[j] = 0;
         if (item < n) {
            const uint32_t ray = ld_stream(in + item);
            const float4 hit = gs.rays[ray], o4 = ld_stream(gs.orig + ray), d4 = ld_stream(gs.dirs + ray);
            const V3 o = xyz(o4), d = xyz(d4);
            const float w = o4.w;
            const uint32_t events = __float_as_uint(d4.w), idx = __float_as_uint(hit.w), pix = gs.queue[ray >> 1];
            V3 L = v3(0.0f, 0.0f, 0.0f);
            uint32_t kind = kGsDark, flags = 0;
            if (idx == kEmptyRef) {
               kind = kGsMissed;
               n_missed++;
               L = hd.furnace ? v3(1.0f, 1.0f, 1.0f) : sky::integrate_scattering_exact_heights(o, d, 999999999.0f, sun);  // rmiss:12 / :16-19, unclamped
            } else {
               const float4* sp = sc.shade + 4 * (size_t)idx;
               const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
               const MeshShade ms = sc.meshes[__float_as_uint(s3.w)];
               if (ms.type == 3.0f) {
                  kind = kGsEmitter;
                  L = v3(1.0f, 1.0f, 1.0f);                                                      // rchit:85-89
               } else if (ms.type == 2.0f) {
                  bool cut = events == gs.max_events;
                  if (!cut) {
                     V3 normal;
                     float uu, vv;
                     surface_normal_uv(s0, s1, s2, s3, hit.y, hit.z, normal, uu, vv);            // rchit:30
                     const V3 Nh = world_normal_of(ms, normal, d);                               // rchit:32-37
                     const GlassEvent e = glass_event(normalize3(d), Nh, ms.property);           // rchit:62-79
                     if (e.cannot) n_tir++;
                     const V3 dn = e.cannot ? e.R : e.T;
                     cut = !gs_finite(dn) || dot3(dn, dn) == 0.0f;
                     if (!cut) {
                        const V3 X = o + hit.x * d;
                        const V3 on = offset_ray(X, Nh);                                         // rgen:59-60
                        gs.orig[ray] = make_float4(on.x, on.y, on.z, w);
                        gs.dirs[ray] = make_float4(dn.x, dn.y, dn.z, __uint_as_float(events + 1u));  // rgen:61: unnormalised
                        goes_on = true;
                        next_ray[j] = ray;
                     }
                  }
                  if (cut) {
                     flags = kGlassCut0 << (ray & 1u);
                     n_cut++;
                  }
               } else if (!hd.furnace) {
                  V3 normal;
                  float uu, vv;
                  surface_normal_uv(s0, s1, s2, s3, hit.y, hit.z, normal, uu, vv);               // rchit:30,39
                  V3 albedo = sample_texture(sc, sc.unorm_lut, ms.diffuse_map, uu, vv);          // rchit:41
                  albedo = albedo * v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);    // rchit:42
                  const V3 Nh = world_normal_of(ms, normal, d);                                  // rchit:32-37
                  const V3 X = o + hit.x * d;
                  const float NdotL = fmaxf(dot3(Nh, sun), 0.0f);
                  if (NdotL > 0.0f) {                                                            // 0 or NaN: dark, no sun ray
                     const V3 rad_sun = v3(1.0f * 1.0f, 1.0f * 1.0f, 1.0f * 1.0f);               // light record 0: color (1, 1, 1) times attenuation 1
                     L = ((v3(albedo.x / kPiBrdf, albedo.y / kPiBrdf, albedo.z / kPiBrdf)) * rad_sun) * NdotL;
                     want_sun = true;
                     const V3 so = offset_ray(X, Nh);
                     sun_ray[j] = make_float4(so.x, so.y, so.z, __uint_as_float(ray));
                  }
               }
            }
            if (!goes_on) {
               gs.rays[ray] = make_float4(w * gs_clamp(L.x, gs.max_radiance), w * gs_clamp(L.y, gs.max_radiance), w * gs_clamp(L.z, gs.max_radiance), 0.0f);
               if (!want_sun) atomicAdd(gs.counts + pix, kind);
               atomicAdd(gs.events + pix, (events << (8u * (ray & 1u))) | flags);
            }
         }
         sun_masks[j] = __ballot(want_sun);
         next_masks[j] = __ballot(goes_on);
         sun_total += (uint32_t)__popcll(sun_masks[j]);
         next_total += (uint32_t)__popcll(next_masks[j]);
      }
      uint32_t sun_slot = wave_reserve(gs.counters + 1, sun_total);
      uint32_t next_slot = wave_reserve(gs.counters + kGlassRound0 + round + 1u, next_total);
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         if ((sun_masks[j] >> lane) & 1ull) gs.sun_rays[sun_slot + ballot_prefix(sun_masks[j])] = sun_ray[j];
         if ((next_masks[j] >> lane) & 1ull) out[next_slot + ballot_prefix(next_masks[j])] = next_ray[j];
         sun_slot += (uint32_t)__popcll(sun_masks[j]);
         next_slot += (uint32_t)__popcll(next_masks[j]);
      }
   }
   wave_add(&gs.counters[2], n_missed);
   wave_add(&gs.counters[4], n_tir);
   wave_add(&gs.counters[5], n_cut);
}

// The composite, one lane per queued pixel: C = clamp(R_0 + R_1) per channel into the radiance image, and C * intensity REPLACES
// deferred_output.rgb (whatever the deferred, reservoir-light, rtgi and glossy passes wrote there); alpha untouched
__global__ __launch_bounds__(kBlock) void k_glass_composite(HybridFrameDev fd, GlassDev gs) {
   const uint32_t pixels = gs.counters[0];
   for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < pixels; q += gridDim.x * kBlock) {
      const float4 r0 = gs.rays[2 * (size_t)q], r1 = gs.rays[2 * (size_t)q + 1];
      const V3 C = v3(gs_clamp(r0.x + r1.x, gs.max_radiance), gs_clamp(r0.y + r1.y, gs.max_radiance), gs_clamp(r0.z + r1.z, gs.max_radiance));
      const uint32_t pix = gs.queue[q];
      gs.radiance[pix] = make_float4(C.x, C.y, C.z, 1.0f);
      fd.deferred[pix] = make_float4(C.x * gs.intensity, C.y * gs.intensity, C.z * gs.intensity, fd.deferred[pix].w);
   }
}

void launch_glass_raygen(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const GlassDev& gs) {
   const uint32_t n = hd.W * hd.H;
   k_glass_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(sc, hd, gs);
   k_glass_raygen<<<stream_grid(c, n * 2u), kBlock, 0, c.stream>>>(sc, hd, gs);
}

void launch_glass_bend(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const GlassDev& gs, uint32_t round) {
   k_glass_bend<<<stream_grid(c, hd.W * hd.H * 2u), kBlock, 0, c.stream>>>(sc, hd, gs, round);
}

void launch_glass_composite(const LaunchCfg& c, const HybridDev& hd, const HybridFrameDev& fd, const GlassDev& gs) {
   k_glass_composite<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(fd, gs);
}

}  // namespace uh
