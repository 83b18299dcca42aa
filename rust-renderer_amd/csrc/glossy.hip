// glossy.hip — ray-traced glossy reflections of the hybrid frame (UH_HYBRID_GLOSSY; utopian_hip.h): which pixels cast, their rays drawn from
// the GGX distribution of visible normals, a closest-hit walk that shades nothing and writes hit records, a streaming kernel that shades
// them with every lane busy, the sun rays of the lit candidates through k_rtgi_shadow (rtgi.hip), the per-pixel split sums in sample
// order, the roughness-aware tile filter and the composite into deferred_output; with their launchers.
// An extension: the reference has no glossy reflection. Arithmetic: DESIGN.md section 2 "Ray-traced glossy reflections";
// tests/glossy_reference.py restates it.
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

// the bytes of a pixel's count word above the lowest (sunlit: k_rtgi_shadow adds the sun rays' verdicts), as the rtgi pass has them
constexpr uint32_t kGlDark = 1u << 8, kGlEmitter = 1u << 16, kGlMissed = 1u << 24;
constexpr uint8_t kGlNoCast = 255;  // GlossyDev::re of a pixel that did not cast

// x > 0 ? x : 0: a NaN, a negative and -0 become +0
__device__ __forceinline__ float gl_pos(float x) { return x > 0.0f ? x : 0.0f; }
// L as it is stored: rtgi_clamp (rtgi.hip) with this pass's cap
__device__ __forceinline__ float gl_clamp(float x, float cap) { return fminf(gl_pos(x), cap); }
__device__ __forceinline__ V3 gl_cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ bool gl_finite(V3 a) { return fabsf(a.x) < INFINITY && fabsf(a.y) < INFINITY && fabsf(a.z) < INFINITY; }

// What a pixel that casts hands its samples. False: the pixel does not cast (RTGI's rule, then the material's type,
// the roughness window, V finite and NoV > 0).
struct GlossyPixel {
   V3 P, Nn, V;
   float NoV, r;
};
__device__ __forceinline__ bool glossy_pixel(const SceneDev& sc, const HybridDev& hd, const GlossyDev& gl, uint32_t pix, GlossyPixel& g) {
   const float4 P4 = hd.pos[pix];
   if (!(P4.w != 0.0f && rtao_normal(hd.nrm[pix], g.Nn))) return false;
   const float4 R4 = hd.pbr[pix];
   const uint32_t material = (uint32_t)R4.w;  // frag:46
   float rf = 1.0f, type = 0.0f;
   if (material < sc.num_meshes) {
      const MeshShade& ms = sc.meshes[material];
      rf = ms.roughness;
      type = ms.type;
   }
   if (gl.rt_on && type == 1.0f) return false;  // the pixel holds its mirror (frag:92-95)
   g.r = R4.y * rf;                             // frag:52-58
   if (!(g.r >= 0.0f && g.r <= gl.max_roughness)) return false;
   g.P = v3(P4.x, P4.y, P4.z);
   g.V = normalize3(v3(hd.eye[0], hd.eye[1], hd.eye[2]) - g.P);
   if (!gl_finite(g.V)) return false;
   g.NoV = dot3(g.Nn, g.V);
   return g.NoV > 0.0f;
}
__device__ __forceinline__ uint8_t glossy_radius(const GlossyDev& gl, float r) {
   return (uint8_t)(int)(fminf(r / gl.blur_roughness, 1.0f) * (float)gl.blur_radius);
}

// Sample s of a pixel that casts: the direction d, the weight Gw and x5 = (1 - VoH)^5. False: the sample is below (NoL > 0 does not hold).
__device__ __forceinline__ bool glossy_sample(const HybridDev& hd, const GlossyDev& gl, uint32_t pix, uint32_t s, const GlossyPixel& g, V3& d, float& Gw, float& x5) {
   const V3 n = g.Nn, V = g.V;
   const float alpha = g.r * g.r, a2 = alpha * alpha;
   // Duff et al. 2017, "Building an orthonormal basis, revisited"
   const float sign = copysignf(1.0f, n.z);
   const float a = -1.0f / (sign + n.z);
   const float b = (n.x * n.y) * a;
   const V3 T = v3(1.0f + ((sign * n.x) * n.x) * a, sign * b, -(sign * n.x));
   const V3 B = v3(b, sign + (n.y * n.y) * a, -n.y);
   const V3 Ve = v3(dot3(V, T), dot3(V, B), g.NoV);
   // Heitz 2018, "Sampling the GGX distribution of visible normals"
   const V3 Vh = normalize3(v3(alpha * Ve.x, alpha * Ve.y, Ve.z));
   const float lensq = Vh.x * Vh.x + Vh.y * Vh.y;
   V3 T1 = v3(1.0f, 0.0f, 0.0f);
   if (lensq > 0.0f) {
      const float len = sqrtf(lensq);
      T1 = v3(-Vh.y / len, Vh.x / len, 0.0f);
   }
   const V3 T2 = gl_cross(Vh, T1);
   uint32_t rng = init_rng(pix % hd.W, pix / hd.W, hd.W, (gl.frame_base + s) ^ kGlossySeedXor);
   float t1, t2;
   random_point_in_unit_disk(rng, t1, t2);
   const float sh = 0.5f * (1.0f + Vh.z);
   t2 = (1.0f - sh) * sqrtf(1.0f - t1 * t1) + sh * t2;
   const float c = sqrtf(gl_pos((1.0f - t1 * t1) - t2 * t2));
   const V3 Nh = (t1 * T1 + t2 * T2) + c * Vh;
   const V3 Ne = normalize3(v3(alpha * Nh.x, alpha * Nh.y, gl_pos(Nh.z)));
   const V3 Hw = (Ne.x * T + Ne.y * B) + Ne.z * n;
   const float VoH = dot3(V, Hw);
   d = normalize3((2.0f * VoH) * Hw - V);
   const float NoL = dot3(n, d), NoV = g.NoV;
   if (!(NoL > 0.0f)) return false;
   const float sv = sqrtf((NoV * NoV) * (1.0f - a2) + a2);
   const float sl = sqrtf((NoL * NoL) * (1.0f - a2) + a2);
   Gw = (NoL * (NoV + sv)) / (NoL * sv + NoV * sl);
   const float x = 1.0f - VoH;
   x5 = ((x * x) * (x * x)) * x;
   return true;
}

// Every pixel's counts and both images are zeroed and its radius byte is set; the pixels that cast are queued (queue_pixels).
__global__ __launch_bounds__(kBlock) void k_glossy_classify(SceneDev sc, HybridDev hd, GlossyDev gl) {
   queue_pixels(hd.W * hd.H, gl.counters, gl.queue, [&](uint32_t pix) {
      gl.counts[pix] = 0;
      gl.scale[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      gl.bias[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      GlossyPixel g;
      const bool casts = glossy_pixel(sc, hd, gl, pix, g);
      gl.re[pix] = casts ? glossy_radius(gl, g.r) : kGlNoCast;
      return casts;
   });
}

// The streaming kernels' appends. One same-address atomic per wave and 64 items costs 11 ns each on the MI355X whatever the kernel does
// beside it (k_rtgi_classify and k_glossy_classify: 0.375 ms for 32,400 of them), and a streaming kernel has no walk
// to hide them behind. So a wave takes kGlBatch rounds of 64 items, keeps each round's ballot, and reserves the slots of all of them
// with one atomic (wave_reserve, device_math.h): the lane's slot in round j is the base, plus the entries of the rounds before, plus its
// prefix in round j's ballot. Items are numbered in 64 bits: the last group of a count near 2^32 does not wrap onto the first rays.
constexpr int kGlBatch = 4;

// Ray generation, one lane per sample of a queued pixel (item i = sample i % samples of queue slot i / samples): a below sample is settled
// here - an all-zero record and a dark count - and never reaches the walk; the others store origin, direction and weights and are queued
// by ray number (in batches: above).
__global__ __launch_bounds__(kBlock) void k_glossy_raygen(SceneDev sc, HybridDev hd, GlossyDev gl) {
   const uint32_t n = gl.counters[0] * gl.samples, groups = (uint32_t)(((uint64_t)n + 64u * kGlBatch - 1) / (64u * kGlBatch)), lane = lane_id();
   uint32_t n_below = 0;
   for (uint32_t grp = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); grp < groups; grp += gridDim.x * kWavesPerBlock) {
      unsigned long long masks[kGlBatch];
      uint32_t total = 0;
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         const uint64_t item = ((uint64_t)grp * kGlBatch + j) * 64u + lane;
         const uint32_t ray = (uint32_t)item;
         bool queued = false;
         if (item < n) {
            const uint32_t pix = gl.queue[ray / gl.samples];
            GlossyPixel g;
            glossy_pixel(sc, hd, gl, pix, g);
            V3 d;
            float Gw, x5;
            queued = glossy_sample(hd, gl, pix, ray % gl.samples, g, d, Gw, x5);
            if (queued) {
               const V3 o = offset_ray(g.P, g.Nn);
               gl.orig[ray] = make_float4(o.x, o.y, o.z, Gw);
               gl.dirs[ray] = make_float4(d.x, d.y, d.z, x5);
            } else {
               gl.rays[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
               atomicAdd(gl.counts + pix, kGlDark);
               n_below++;
            }
         }
         masks[j] = __ballot(queued);
         total += (uint32_t)__popcll(masks[j]);
      }
      uint32_t slot = wave_reserve(gl.counters + 3, total);
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         if ((masks[j] >> lane) & 1ull) gl.ray_queue[slot + ballot_prefix(masks[j])] = (uint32_t)(((uint64_t)grp * kGlBatch + j) * 64u + lane);
         slot += (uint32_t)__popcll(masks[j]);
      }
   }
   wave_add(&gl.counters[4], n_below);
}

// The closest-hit walk over the queued rays, an item walk (item_walk.h) that shades nothing: the lane that takes a ray loads its origin
// and direction, and when its walk ends it writes the hit record (t, u, v, idx; idx = kEmptyRef for a miss) and is idle for the next
// refill at once. No lane waits for another and nothing of the shader is live here.
// The glass pass runs its rounds through this kernel on a view of its own buffers (glass_walk_view, graphs_internal.h) whose `counters`
// is valid at index 3 ALONE: the kernel must read nothing of gl but ray_queue, counters[3], orig, dirs and rays.
__global__ __launch_bounds__(kBlock, 5) void k_glossy_trace(SceneDev sc, GlossyDev gl) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   ItemWalk w(s_walk, t, spill, gl.ray_queue, gl.counters[3]);
   uint32_t ray = 0;
   auto start = [&](uint32_t item) {
      ray = item;
      const float4 o = ld_stream(gl.orig + item), d = ld_stream(gl.dirs + item);
      trav_init(t, make_float4(o.x, o.y, o.z, 0.001f), make_float4(d.x, d.y, d.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<false, false>(w, sc, occluded)) gl.rays[ray] = make_float4(t.best.t, t.best.u, t.best.v, __uint_as_float(t.best.idx));
   }
}

// The hit shading, one lane per queued ray (whole waves: the sun rays are appended with one atomic per wave and kGlBatch rounds). L is the rtgi pass's
// (k_rtgi_trace's shading, copied: a shared body once rescheduled that kernel's sky integral): a miss the sky with
// exact heights, unclamped ((1, 1, 1) under furnace), a type-3 hit (1, 1, 1), any other hit dark or sun-lit Lambert with one any-hit sun
// ray from offset_ray(X, Nh); then the clamp. The record (Gw L, x5) is stored and - unless a sun ray decides - the ray's count byte added.
__global__ __launch_bounds__(kBlock) void k_glossy_shade(SceneDev sc, HybridDev hd, GlossyDev gl) {
   const uint32_t n = gl.counters[3], groups = (uint32_t)(((uint64_t)n + 64u * kGlBatch - 1) / (64u * kGlBatch)), lane = lane_id();
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   uint32_t n_missed = 0;
   for (uint32_t grp = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); grp < groups; grp += gridDim.x * kWavesPerBlock) {
      unsigned long long masks[kGlBatch];
      float4 sun_ray[kGlBatch];  // a round's sun ray: origin.xyz, ray number (bits)
      uint32_t total = 0;
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         const uint64_t item = ((uint64_t)grp * kGlBatch + j) * 64u + lane;
         bool want_sun = false;
         sun_ray[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         if (item < n) {
            const uint32_t ray = ld_stream(gl.ray_queue + item);
            const float4 hit = gl.rays[ray], o4 = ld_stream(gl.orig + ray), d4 = ld_stream(gl.dirs + ray);
            const V3 o = xyz(o4), d = xyz(d4);
            const float Gw = o4.w, x5 = d4.w;
            const uint32_t idx = __float_as_uint(hit.w), pix = gl.queue[ray / gl.samples];
            V3 L = v3(0.0f, 0.0f, 0.0f);
            uint32_t kind = kGlDark;
            if (idx == kEmptyRef) {
               kind = kGlMissed;
               n_missed++;
               L = hd.furnace ? v3(1.0f, 1.0f, 1.0f) : sky::integrate_scattering_exact_heights(o, d, 999999999.0f, sun);  // rmiss:12 / :16-19, unclamped
            } else {
               const float4* sp = sc.shade + 4 * (size_t)idx;
               const float4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
               const MeshShade ms = sc.meshes[__float_as_uint(s3.w)];
               if (ms.type == 3.0f) {
                  kind = kGlEmitter;
                  L = v3(1.0f, 1.0f, 1.0f);                                                      // rchit:85-89
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
            gl.rays[ray] = make_float4(Gw * gl_clamp(L.x, gl.max_radiance), Gw * gl_clamp(L.y, gl.max_radiance), Gw * gl_clamp(L.z, gl.max_radiance), x5);
            if (!want_sun) atomicAdd(gl.counts + pix, kind);
         }
         masks[j] = __ballot(want_sun);
         total += (uint32_t)__popcll(masks[j]);
      }
      uint32_t slot = wave_reserve(gl.counters + 1, total);
#pragma unroll
      for (int j = 0; j < kGlBatch; j++) {
         if ((masks[j] >> lane) & 1ull) gl.sun_rays[slot + ballot_prefix(masks[j])] = sun_ray[j];
         slot += (uint32_t)__popcll(masks[j]);
      }
   }
   wave_add(&gl.counters[2], n_missed);
}

// S and Bi of the pixel in queue slot q, one lane walking the samples in order, each sum from its s = 0 term:
// S = (sum R_s (1 - x5_s)) / (float)samples, Bi = (sum R_s x5_s) / (float)samples
__global__ __launch_bounds__(kBlock) void k_glossy_mean(GlossyDev gl, float4* __restrict__ out_s, float4* __restrict__ out_b) {
   const uint32_t pixels = gl.counters[0];
   for (uint32_t q = blockIdx.x * kBlock + threadIdx.x; q < pixels; q += gridDim.x * kBlock) {
      const float4* R = gl.rays + (size_t)q * gl.samples;
      float4 r0 = R[0];
      float om = 1.0f - r0.w;
      V3 S = v3(r0.x * om, r0.y * om, r0.z * om), Bi = v3(r0.x * r0.w, r0.y * r0.w, r0.z * r0.w);
      for (uint32_t s = 1; s < gl.samples; s++) {
         r0 = R[s];
         om = 1.0f - r0.w;
         S = S + v3(r0.x * om, r0.y * om, r0.z * om);
         Bi = Bi + v3(r0.x * r0.w, r0.y * r0.w, r0.z * r0.w);
      }
      const float n = (float)gl.samples;
      const uint32_t pix = gl.queue[q];
      out_s[pix] = make_float4(S.x / n, S.y / n, S.z / n, 1.0f);
      out_b[pix] = make_float4(Bi.x / n, Bi.y / n, Bi.z / n, 1.0f);
   }
}

// The filter over the tiles of edge_filter.h, staged for blur_radius: a lane's own radius is its pixel's re (0: Sf = S, Bf = Bi), and a
// tap also needs max(|dx|, |dy|) <= its own re, which keeps the reuse symmetric. The means are float32 sums from 0 over the counting taps
// in their order, divided by their number.
constexpr int kGlMaxBlur = 6;
__global__ __launch_bounds__(kBlock) void k_glossy_filter(HybridDev hd, GlossyDev gl) {
   using Tile = FilterTile<kGlMaxBlur, 7>;
   __shared__ Tile::Rec s_rec;
   __shared__ Tile::Valid s_valid;
   Tile s_tile{s_rec, s_valid};
   const int r = (int)gl.blur_radius;
   const FilterLane me = s_tile.stage(
      hd, r, [&](size_t g) { return gl.re[g] != kGlNoCast; },
      [&](size_t g, int i) {
         const float4 S = gl.mean_s[g], Bi = gl.mean_b[g];
         s_tile.rec[6][i] = S.x, s_tile.rec[7][i] = S.y, s_tile.rec[8][i] = S.z;
         s_tile.rec[9][i] = Bi.x, s_tile.rec[10][i] = Bi.y, s_tile.rec[11][i] = Bi.z;
         s_tile.rec[12][i] = (float)gl.re[g];
      });
   if (me.px >= (int)hd.W || me.py >= (int)hd.H || !s_tile.valid[me.centre]) return;  // not a pixel that cast: (0, 0, 0, 0) from the classify
   const int c = me.centre, re = (int)s_tile.rec[12][c];
   const size_t pix = (size_t)me.py * hd.W + me.px;
   if (re == 0) {
      gl.scale[pix] = make_float4(s_tile.rec[6][c], s_tile.rec[7][c], s_tile.rec[8][c], 1.0f);
      gl.bias[pix] = make_float4(s_tile.rec[9][c], s_tile.rec[10][c], s_tile.rec[11][c], 1.0f);
      return;
   }
   V3 S = v3(0.0f, 0.0f, 0.0f), Bi = v3(0.0f, 0.0f, 0.0f);
   const float n = (float)s_tile.taps(
      c, r, re, gl.blur_normal_cos, gl.blur_plane, [&](int i, int reach) { return reach <= (int)s_tile.rec[12][i]; },
      [&](int i) {
         S = S + v3(s_tile.rec[6][i], s_tile.rec[7][i], s_tile.rec[8][i]);
         Bi = Bi + v3(s_tile.rec[9][i], s_tile.rec[10][i], s_tile.rec[11][i]);
      });
   gl.scale[pix] = make_float4(S.x / n, S.y / n, S.z / n, 1.0f);
   gl.bias[pix] = make_float4(Bi.x / n, Bi.y / n, Bi.z / n, 1.0f);
}

// The composite, one lane per pixel that cast: F0 = 0.04 (1 - metallic) + base metallic in the deferred pass's order (lighting:29-30),
// add = ((F0 Sf + Bf) intensity) occlusion, times (with ssao_enabled) the pixel's ssao texel; base, metallic and the texel's index as
// k_hybrid_deferred forms them. The gamma table as k_hybrid_deferred has it. (A metal pixel under raytracing_supported = 1 never cast.)
__global__ __launch_bounds__(kBlock) void k_glossy_composite(SceneDev sc, HybridDev hd, HybridFrameDev fd, GlossyDev gl) {
   __shared__ float s_gamma[256];  // pow(c / 255, 2.2) of every UNORM8 value: pow in double, rounded to float
   s_gamma[threadIdx.x] = (float)pow((double)((float)threadIdx.x / 255.0f), (double)2.2f);
   __syncthreads();
   const uint32_t n = hd.W * hd.H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   const float4 Sf = gl.scale[i];
   if (Sf.w == 0.0f) return;  // the pixel did not cast
   const float4 Bf = gl.bias[i];
   const float4 R4 = hd.pbr[i];
   const uchar4 A = hd.alb[i];
   const uint32_t material = (uint32_t)R4.w;                                                    // frag:46
   float mf = 1.0f;
   V3 bc = v3(1.0f, 1.0f, 1.0f);
   if (material < sc.num_meshes) {
      const MeshShade& ms = sc.meshes[material];
      mf = ms.metallic;
      bc = v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);
   }
   const float metallic = R4.x * mf, occlusion = R4.z;                                          // frag:52-58
   const V3 base = v3(s_gamma[A.x], s_gamma[A.y], s_gamma[A.z]) * bc;                           // frag:61-65
   const V3 F0 = v3(0.04f, 0.04f, 0.04f) * (1.0f - metallic) + base * metallic;                 // lighting:29-30
   V3 add = (F0 * v3(Sf.x, Sf.y, Sf.z) + v3(Bf.x, Bf.y, Bf.z)) * gl.intensity;
   add = add * occlusion;
   if (fd.ssao_on) add = add * ((float)fd.ssao[(size_t)(hd.H - 1 - i / hd.W) * hd.W + i % hd.W] / 65535.0f);
   const float4 d = fd.deferred[i];
   fd.deferred[i] = make_float4(d.x + add.x, d.y + add.y, d.z + add.z, d.w);
}

// the walk alone, over at most `most` queued rays: gl.ray_queue, gl.counters[3], gl.orig and gl.dirs in, gl.rays out (the glass pass runs
// its rounds through it: glass_walk_view, graphs_internal.h)
void launch_glossy_walk(const LaunchCfg& c, const SceneDev& sc, const GlossyDev& gl, uint64_t most) {
   const dim3 grid = persistent_grid(most, c.num_cus * c.closest_blocks_per_cu);
   k_glossy_trace<<<grid, kBlock, 0, c.stream>>>(sc, gl);
}

void launch_glossy_trace(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const GlossyDev& gl) {
   const uint32_t n = hd.W * hd.H;
   k_glossy_classify<<<stream_grid(c, n), kBlock, 0, c.stream>>>(sc, hd, gl);
   k_glossy_raygen<<<stream_grid(c, n * gl.samples), kBlock, 0, c.stream>>>(sc, hd, gl);
   launch_glossy_walk(c, sc, gl, (uint64_t)n * gl.samples);
}

void launch_glossy_shade(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const GlossyDev& gl) {
   k_glossy_shade<<<stream_grid(c, hd.W * hd.H * gl.samples), kBlock, 0, c.stream>>>(sc, hd, gl);
}

void launch_glossy_filter(const LaunchCfg& c, const HybridDev& hd, const GlossyDev& gl) {
   const bool blur = gl.blur_radius != 0;
   k_glossy_mean<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(gl, blur ? gl.mean_s : gl.scale, blur ? gl.mean_b : gl.bias);
   if (!blur) return;  // Sf = S, Bf = Bi
   k_glossy_filter<<<filter_grid(hd), kBlock, 0, c.stream>>>(hd, gl);
}

void launch_glossy_composite(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const HybridFrameDev& fd, const GlossyDev& gl) {
   k_glossy_composite<<<dim3((hd.W * hd.H + kBlock - 1) / kBlock), kBlock, 0, c.stream>>>(sc, hd, fd, gl);
}

}  // namespace uh
