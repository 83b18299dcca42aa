// rtgi.hip — one-bounce ray-traced diffuse GI of the hybrid frame (UH_HYBRID_RTGI; utopian_hip.h): which pixels cast, their cosine-weighted
// hemisphere rays through the closest-hit walk with the hit shaded where the walk ends, the sun rays of the lit candidates through the
// any-hit walk, the per-pixel mean in sample order, the tile filter and the composite into deferred_output; with their launchers.
// An extension: the reference has no GI. Arithmetic: DESIGN.md section 2 "Ray-traced diffuse GI"; tests/rtgi_reference.py restates it.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "hybrid_shading.h"
#include "kernel_common.h"
#include "path_shading.h"
#include "traversal.h"

namespace uh {

// the bytes of a pixel's count word
constexpr uint32_t kGiSunlit = 1u, kGiDark = 1u << 8, kGiEmitter = 1u << 16, kGiMissed = 1u << 24;

// L as it is stored: NaN, negatives and -0 become +0, then the cap (max_radiance is finite and > 0): always finite
__device__ __forceinline__ float rtgi_clamp(float x, float cap) { return fminf(x > 0.0f ? x : 0.0f, cap); }
__device__ __forceinline__ float4 rtgi_record(V3 L, float cap) { return make_float4(rtgi_clamp(L.x, cap), rtgi_clamp(L.y, cap), rtgi_clamp(L.z, cap), 0.0f); }

// One lane per pixel: its counts and radiance are zeroed, and the pixels that cast (RTAO's rule: position w != 0, Nn finite) are appended
// to a dense queue (one atomic per wave, as k_rtao_classify).
__global__ __launch_bounds__(kBlock) void k_rtgi_classify(HybridDev hd, RtgiDev gi) {
   const uint32_t n = hd.W * hd.H, groups = (n + 63) / 64, lane = lane_id();
   for (uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += gridDim.x * kWavesPerBlock) {
      const uint32_t pix = g * 64u + lane;
      bool cast = false;
      if (pix < n) {
         gi.counts[pix] = 0;
         gi.radiance[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
         V3 nn;
         cast = hd.pos[pix].w != 0.0f && rtao_normal(hd.nrm[pix], nn);
      }
      const uint32_t slot = wave_append(gi.counters, cast);
      if (cast) gi.queue[slot] = pix;
   }
}

// The hemisphere rays: closest hit. Persistent waves with the LDS refill of k_rtao_trace; the pool carries item numbers alone (the lane that
// takes one makes its ray from the G-buffer and the RNG there). kOrder lays the items out (measured: DESIGN.md section 4 "Ray-traced
// diffuse GI"):
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
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   __shared__ RayPool<0> s_pool[kWavesPerBlock];
   const uint32_t lane = lane_id();
   const uint32_t wave = threadIdx.x >> 6;
   uint32_t* lds_col = &s_stack[wave][0][lane];
   RayPool<0>& pool = s_pool[wave];
   const uint32_t pixels = gi.counters[0];
   RaySource src;
   src.queue = nullptr;
   src.count = pixels * gi.samples;
   src.cursor = nullptr;
   src.wave_index = blockIdx.x * kWavesPerBlock + wave;
   src.num_waves = gridDim.x * kWavesPerBlock;
   auto source_of = [](int, uint32_t) { return (const float4*)nullptr; };
   Feeder<0> f;
   Trav t;
   t.cur = kEmptyRef;
   t.sp = 0;
   uint32_t pix = 0, ray = 0, n_nodes = 0, n_tris = 0, n_missed = 0;
   uint32_t spill[kSpillStack];
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   auto take = [&](uint32_t slot) {
      const uint32_t item = pool.id[slot];
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
      const V3 w = nn + u;
      const V3 d = !(dot3(w, w) >= 1e-12f) ? nn : normalize3(w);
      trav_init(t, make_float4(o.x, o.y, o.z, 0.001f), make_float4(d.x, d.y, d.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   bool pending = false;  // the lane's walk has ended and its ray is not shaded yet
   while (refill_lanes<0>(f, src, pool, t.cur == kEmptyRef && !pending, source_of, take)) {
      if (t.cur != kEmptyRef) {
         bool occluded = false;
         pending = trav_step<false, false>(sc.nodes, sc.tris, t, lds_col, spill, occluded, n_nodes, n_tris);
      }
      const uint32_t n_pending = (uint32_t)__popcll(__ballot(pending));
      if (n_pending != 0 && (n_pending >= kGiShadeBatch || __ballot(t.cur != kEmptyRef) == 0ull)) {
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
   for (int off = 32; off > 0; off >>= 1) n_missed += __shfl_down(n_missed, off);  // one atomic per wave
   if (lane == 0 && n_missed) atomicAdd(&gi.counters[2], n_missed);
}

// One any-hit ray toward the sun per queued record, in the shape of k_hybrid_restir_trace: persistent waves with the LDS refill, the pool
// carries the record numbers alone. An occluded ray zeroes its radiance record and counts as dark, an unoccluded one keeps it and counts as
// sunlit.
__global__ __launch_bounds__(kBlock, 5) void k_rtgi_shadow(SceneDev sc, HybridDev hd, RtgiDev gi) {
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   __shared__ RayPool<0> s_pool[kWavesPerBlock];
   const uint32_t lane = lane_id();
   const uint32_t wave = threadIdx.x >> 6;
   uint32_t* lds_col = &s_stack[wave][0][lane];
   RayPool<0>& pool = s_pool[wave];
   RaySource src;
   src.queue = nullptr;
   src.count = gi.counters[1];
   src.cursor = nullptr;
   src.wave_index = blockIdx.x * kWavesPerBlock + wave;
   src.num_waves = gridDim.x * kWavesPerBlock;
   auto source_of = [](int, uint32_t) { return (const float4*)nullptr; };
   Feeder<0> f;
   Trav t;
   t.cur = kEmptyRef;
   t.sp = 0;
   uint32_t ray = 0, n_nodes = 0, n_tris = 0;
   uint32_t spill[kSpillStack];
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   auto take = [&](uint32_t slot) {
      const float4 r = ld_stream(gi.sun_rays + pool.id[slot]);
      ray = __float_as_uint(r.w);
      trav_init(t, make_float4(r.x, r.y, r.z, 0.001f), make_float4(sun.x, sun.y, sun.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   while (refill_lanes<0>(f, src, pool, t.cur == kEmptyRef, source_of, take)) {
      if (t.cur != kEmptyRef) {
         bool occluded = false;
         if (trav_step<true, false>(sc.nodes, sc.tris, t, lds_col, spill, occluded, n_nodes, n_tris)) {
            if (occluded) gi.rays[ray] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            atomicAdd(gi.counts + gi.queue[ray / gi.samples], occluded ? kGiDark : kGiSunlit);
         }
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

// The filter: a block is a kGiTileW x kGiTileH tile of pixels, one lane per pixel. The tile and its halo (blur_radius <= kGiMaxBlur on
// every side) of (P, Nn, E) are staged in LDS once per block, as k_rtao_resolve<true> does; s_valid says which records can be taps (inside
// the frame, a pixel that cast). Taps (dx, dy) in [-r, r]^2, dy outer. Tiles are numbered along x first.
constexpr int kGiTileW = 32, kGiTileH = kBlock / kGiTileW, kGiMaxBlur = 6;
constexpr int kGiHaloW = kGiTileW + 2 * kGiMaxBlur, kGiHaloH = kGiTileH + 2 * kGiMaxBlur;
__global__ __launch_bounds__(kBlock) void k_rtgi_filter(HybridDev hd, RtgiDev gi) {
   __shared__ float s_rec[9][kGiHaloW * kGiHaloH];  // nine planes of the staged records: P, Nn, E
   __shared__ uint8_t s_valid[kGiHaloW * kGiHaloH];
   const int W = (int)hd.W, H = (int)hd.H, r = (int)gi.blur_radius;  // 1 <= r <= kGiMaxBlur (uh_set_rtgi_params, launch_rtgi_filter)
   const int tx = (int)threadIdx.x % kGiTileW, ty = (int)threadIdx.x / kGiTileW;
   const int tiles_x = (W + kGiTileW - 1) / kGiTileW;
   const int x0 = (int)(blockIdx.x % (uint32_t)tiles_x) * kGiTileW, y0 = (int)(blockIdx.x / (uint32_t)tiles_x) * kGiTileH;
   const int px = x0 + tx, py = y0 + ty;
   const int hw = kGiTileW + 2 * r, hh = kGiTileH + 2 * r;  // the halo this radius needs, rows of hw records
   for (int i = (int)threadIdx.x; i < hw * hh; i += kBlock) {
      const int gx = x0 - r + i % hw, gy = y0 - r + i / hw;
      bool valid = false;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
         const size_t g = (size_t)gy * W + gx;
         const float4 P4 = hd.pos[g];
         V3 nn;
         valid = P4.w != 0.0f && rtao_normal(hd.nrm[g], nn);
         if (valid) {
            const float4 E = gi.mean[g];
            s_rec[0][i] = P4.x, s_rec[1][i] = P4.y, s_rec[2][i] = P4.z;
            s_rec[3][i] = nn.x, s_rec[4][i] = nn.y, s_rec[5][i] = nn.z;
            s_rec[6][i] = E.x, s_rec[7][i] = E.y, s_rec[8][i] = E.z;
         }
      }
      s_valid[i] = valid ? 1 : 0;
   }
   __syncthreads();
   if (px >= W || py >= H) return;
   const int centre = (ty + r) * hw + (tx + r);
   if (!s_valid[centre]) return;  // (0, 0, 0, 0) from the classify
   const V3 P = v3(s_rec[0][centre], s_rec[1][centre], s_rec[2][centre]), nn = v3(s_rec[3][centre], s_rec[4][centre], s_rec[5][centre]);
   V3 sum = v3(0.0f, 0.0f, 0.0f);
   uint32_t taps = 0;
   for (int dy = -r; dy <= r; dy++) {
      for (int dx = -r; dx <= r; dx++) {
         const int i = centre + dy * hw + dx;
         bool counts = dx == 0 && dy == 0;
         if (!counts && s_valid[i]) {
            const V3 Pt = v3(s_rec[0][i], s_rec[1][i], s_rec[2][i]), nt = v3(s_rec[3][i], s_rec[4][i], s_rec[5][i]);
            counts = dot3(nt, nn) >= gi.blur_normal_cos && fabsf(dot3(Pt - P, nn)) <= gi.blur_plane;
         }
         if (counts) {
            sum = sum + v3(s_rec[6][i], s_rec[7][i], s_rec[8][i]);
            taps++;
         }
      }
   }
   const float n = (float)taps;
   gi.radiance[(size_t)py * W + px] = make_float4(sum.x / n, sum.y / n, sum.z / n, 1.0f);
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

// at most one lane per item, at most the persistent grid of the kernel's kind
static inline dim3 persistent_grid(uint64_t items, uint32_t full) {
   const uint64_t need = (items + kBlock - 1) / kBlock;
   return dim3((uint32_t)(need < full ? (need ? need : 1) : full));
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
   const dim3 grid(((hd.W + kGiTileW - 1) / kGiTileW) * ((hd.H + kGiTileH - 1) / kGiTileH));
   k_rtgi_filter<<<grid, kBlock, 0, c.stream>>>(hd, gi);
}

void launch_rtgi_composite(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const HybridFrameDev& fd, const RtgiDev& gi) {
   k_rtgi_composite<<<dim3((hd.W * hd.H + kBlock - 1) / kBlock), kBlock, 0, c.stream>>>(sc, hd, fd, gi);
}

}  // namespace uh
