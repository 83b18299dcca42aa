// hybrid_kernels.hip — the hybrid graph's passes that are not rasterised (build_render_graph, renderers/mod.rs:61-186): the G-buffer
// resolve behind the primary-ray cast, rt_shadows and rt_reflections, then SSAO, deferred lighting, sky and present; with their launchers.
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "hybrid_shading.h"
#include "ibl_device.h"
#include "item_walk.h"
#include "kernel_common.h"
#include "path_shading.h"
#include "traversal.h"

namespace uh {

// ------------------------------------------------------------------------------------------
// The hybrid graph's ray-traced passes (build_render_graph, renderers/mod.rs:61-186): a G-buffer of four targets (gbuffer.vert /
// gbuffer.frag as a primary-ray cast), rt_shadows (rt_shadows.rgen) and rt_reflections (rt_reflections.{rgen,rchit,rmiss}, the
// IBL-off branch). Arithmetic: DESIGN.md section 2 "Hybrid passes".
// ------------------------------------------------------------------------------------------
// the clear value of every target (pass.rs:210-214): (1, 1, 1, 0); the two RT images hold the same until their pass first runs
__global__ __launch_bounds__(kBlock) void k_hybrid_clear(HybridDev hd, uint32_t n) {
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
      const float4 one = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      hd.pos[i] = one;
      hd.nrm[i] = one;
      hd.pbr[i] = one;
      hd.alb[i] = make_uchar4(255, 255, 255, 0);
      hd.shadow[i] = 255;
      hd.refl[i] = make_uchar4(255, 255, 255, 0);
   }
}

// gbuffer.vert:29-46 per vertex + the rasteriser's interpolation + gbuffer.frag:27-51, at the cast's hit. The cast left its records in the
// targets: ray origin in the normal target, direction in the pbr target, hit record (t, u, v, packet) in the position target; a lane
// reads the three of its pixel before it writes the four.
__global__ __launch_bounds__(kBlock) void k_hybrid_gbuffer_resolve(SceneDev sc, HybridDev hd, uint32_t n) {
   for (uint32_t j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
      const float4 h = hd.pos[j], ro = hd.nrm[j], rd = hd.pbr[j];
      const uint32_t packet = __float_as_uint(h.w);
      const float4 clear = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      float4 pos = clear, nrm = clear, pbr = clear;
      uchar4 alb = make_uchar4(255, 255, 255, 0);
      if (packet != kEmptyRef) {
         const V3 p = v3(ro.x, ro.y, ro.z) + h.x * v3(rd.x, rd.y, rd.z);  // k_gbuffer_resolve's expression: the same words
         pos = make_float4(p.x, p.y, p.z, 1.0f);
         const uint32_t key = __float_as_uint(sc.tris[kTriStride16 * (size_t)packet + 2].y);
         const uint32_t mesh = key >> kPrimBits, prim = key & kPrimMask;
         const HybridMesh m = hd.meshes[mesh];
         const uint32_t* tri = hd.indices + m.index_base + 3 * (size_t)prim;
         const UhVertex* vb = hd.vertices + m.vertex_base;
         const UhVertex& v0 = vb[tri[0]];
         const UhVertex& v1 = vb[tri[1]];
         const UhVertex& v2 = vb[tri[2]];
         const float b0 = 1.0f - h.y - h.z, b1 = h.y, b2 = h.z;
         V3 nn;
         float uu, vv;
         surface_attributes(sc, m, v0, v1, v2, b0, b1, b2, nn, uu, vv);
         gbuffer_targets(sc, m, mesh, nn, uu, vv, nrm, alb, pbr);
      }
      hd.pos[j] = pos;
      hd.nrm[j] = nrm;
      hd.alb[j] = alb;
      hd.pbr[j] = pbr;
   }
}

// rt_shadows.rgen:17-38: one any-hit ray per pixel toward the sun from the G-buffer's texel corner, an item walk (item_walk.h) over the
// pixels: the lane that takes pixel p makes its ray from the G-buffer there.
__global__ __launch_bounds__(kBlock, 5) void k_hybrid_shadow(SceneDev sc, HybridDev hd) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   ItemWalk w(s_walk, t, spill, nullptr, hd.W * hd.H);
   uint32_t pix = 0;
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);  // rgen:28
   auto start = [&](uint32_t item) {
      pix = item;
      const uint32_t px = pix % hd.W, py = pix / hd.W;
      const V3 p = gbuffer_fetch(hd.pos, hd.W, px, py), nn = gbuffer_fetch(hd.nrm, hd.W, px, py);  // rgen:22-24 (not renormalised)
      const V3 o = offset_ray(p, nn);                                                                // rgen:25
      trav_init(t, make_float4(o.x, o.y, o.z, 0.001f), make_float4(sun.x, sun.y, sun.z, 10000.0f), 0.001f, 10000.0f, INFINITY);
   };
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<true, false>(w, sc, occluded)) hd.shadow[pix] = occluded ? 0 : 255;  // rgen:34-37
   }
}

// the texel-corner fetch of gbuffer_fetch, alpha only
__device__ __forceinline__ float gbuffer_fetch_w(const float4* __restrict__ g, uint32_t W, uint32_t px, uint32_t py) {
   uint32_t x0 = px == 0 ? 0 : px - 1, y0 = py == 0 ? 0 : py - 1;
   return ((g[(size_t)y0 * W + x0].w + g[(size_t)y0 * W + px].w) + (g[(size_t)py * W + x0].w + g[(size_t)py * W + px].w)) * 0.25f;
}

// rt_reflections.rgen:34-47, the test: the material of uint(filtered pbr.a) is metal. Metal pixels are queued (queue_pixels,
// kernel_common.h), every other pixel gets (0, 0, 0, 0) here.
__global__ __launch_bounds__(kBlock) void k_hybrid_reflect_classify(SceneDev sc, HybridDev hd) {
   queue_pixels(hd.W * hd.H, hd.counter, hd.queue, [&](uint32_t pix) {
      const uint32_t material = (uint32_t)gbuffer_fetch_w(hd.pbr, hd.W, pix % hd.W, pix / hd.W);  // rgen:34: the filtered index, truncated
      const bool metal = material < sc.num_meshes && sc.meshes[material].type == 1.0f;            // rgen:38
      if (!metal) hd.refl[pix] = make_uchar4(0, 0, 0, 0);                                         // rgen:46
      return metal;
   });
}

// rt_reflections.rgen:22-44 + .rchit:22-64 + .rmiss:9-24 for the queued metal pixels: closest hit, then a lane shades its own ray. kIbl: the
// hit shader's ibl_enabled branch (rchit:50-61) on the IBL maps
template <bool kIbl>
__global__ __launch_bounds__(kBlock) void k_hybrid_reflect(SceneDev sc, HybridDev hd, IblMaps ibl) {
   __shared__ uint32_t s_stack[kWavesPerBlock][kLdsStack][64];
   uint32_t* lds_col = &s_stack[threadIdx.x >> 6][0][lane_id()];
   const uint32_t count = *hd.counter;
   const V3 eye = v3(hd.eye[0], hd.eye[1], hd.eye[2]), sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   uint32_t n_nodes = 0, n_tris = 0;
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
      const uint32_t pix = hd.queue[i], px = pix % hd.W, py = pix / hd.W;
      const V3 p = gbuffer_fetch(hd.pos, hd.W, px, py), nn = gbuffer_fetch(hd.nrm, hd.W, px, py);  // rgen:28-30
      const V3 o = offset_ray(p, nn);                                                                // rgen:31
      const V3 to_eye = normalize3(eye - o);                                                         // rgen:33
      const V3 dir = reflect3(vneg(to_eye), nn);                                                     // rgen:34: I - (2 dot(N, I)) N, N not normalised
      Hit h;
      V3 c;
      if (traverse<false, false>(sc, o, dir, 0.001f, 10000.0f, INFINITY, h, lds_col, n_nodes, n_tris)) {
         const float4* s = sc.shade + 4 * (size_t)h.idx;
         const float4 s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
         V3 normal;
         float uu, vv;
         surface_normal_uv(s0, s1, s2, s3, h.u, h.v, normal, uu, vv);                                // rchit:30,39
         const MeshShade ms = sc.meshes[__float_as_uint(s3.w)];
         V3 color = sample_texture(sc, sc.unorm_lut, ms.diffuse_map, uu, vv);                        // rchit:41
         color = color * v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);                   // rchit:42
         if (kIbl) {
            const HybridMesh& hm = hd.meshes[__float_as_uint(s3.w)];
            const V3 mr = sample_texture(sc, sc.unorm_lut, hm.metallic_roughness_map, uu, vv);        // rchit:56-57
            const V3 oc = sample_texture(sc, sc.unorm_lut, hm.occlusion_map, uu, vv);                 // rchit:58
            const V3 wn = world_normal_of(ms, normal, dir);                                          // rchit:32-37
            const V3 pos = o + h.t * dir;                                                            // the hit point of the ray
            c = ibl::image_based_lighting(ibl, pos, color, wn, mr.z, mr.y, oc.x, eye);               // rchit:60
         } else {
            c = 0.1f * color;                                                                        // rchit:62
         }
      } else if (hd.furnace) {
         c = v3(1.0f, 1.0f, 1.0f);                                                                   // rmiss:12 (FURNACE_TEST)
      } else {
         const V3 sk = sky::integrate_scattering(o, dir, 999999999.0f, sun);                         // rmiss:16-19
         c = v3(fminf(sk.x, 1.0f), fminf(sk.y, 1.0f), fminf(sk.z, 1.0f));                            // rmiss:22
      }
      hd.refl[pix] = make_uchar4((unsigned char)unorm8(c.x), (unsigned char)unorm8(c.y), (unsigned char)unorm8(c.z), 0);  // rgen:42
   }
}

// The reservoir lights (UH_HYBRID_RESTIR_LIGHTS; DESIGN.md section 2, "Reservoir lights"): which pixels cast a ray toward the light of
// their spatial reservoir. Every texel of the visibility image is written 0 here, the pixels that cast are queued (queue_pixels,
// kernel_common.h). The cull is direct_lighting's own NdotL (light_term): a culled pixel's term would be exactly zero.
__global__ __launch_bounds__(kBlock) void k_hybrid_restir_classify(HybridDev hd, HybridRestirDev rl) {
   queue_pixels(hd.W * hd.H, rl.counters, rl.queue, [&](uint32_t pix) {
      rl.vis[pix] = 0;
      const float4 P4 = hd.pos[pix];
      const UhReservoir r = rl.reservoirs[pix];
      if (!(P4.w != 0.0f && r.Y >= 0 && (uint32_t)r.Y < rl.num_lights && r.W_X > 0.0f && r.W_X < INFINITY)) return false;
      const UhGpuLight& l = rl.raw_lights[r.Y];
      if (!(l.light_type == 1.0f || l.light_type == 2.0f)) return false;                      // HybridLight::mode 1 or 2
      const float4 N4 = hd.nrm[pix];
      const V3 ptl = v3(l.position[0], l.position[1], l.position[2]) - v3(P4.x, P4.y, P4.z);
      const float d = sqrtf(dot3(ptl, ptl));
      const V3 L = ptl * (1.0f / d);
      return fmaxf(dot3(v3(N4.x, N4.y, N4.z), L), 0.0f) != 0.0f;                               // NaN: culled
   });
}

// One any-hit ray per queued pixel toward its reservoir's light: reference.rgen:113-119 as the path tracer pins it (make_shadow_ray<true>),
// from offset_ray of the pixel's own G-buffer texels, an item walk (item_walk.h) over the queued pixel ids: the lane that takes one makes
// its ray from the G-buffer, the reservoir and the light table there. No shading here: the deferred pass, which holds the surface terms
// anyway, adds the light where this kernel stores 255.
__global__ __launch_bounds__(kBlock, 5) void k_hybrid_restir_trace(SceneDev sc, FrameParams fp, HybridDev hd, HybridRestirDev rl) {
   __shared__ ItemWalkLds s_walk;
   Trav t;
   uint32_t spill[kSpillStack];
   ItemWalk w(s_walk, t, spill, rl.queue, rl.counters[0]);
   uint32_t pix = 0, n_occluded = 0;
   auto start = [&](uint32_t item) {
      pix = item;
      const float4 P4 = hd.pos[pix], N4 = hd.nrm[pix];
      const V3 o = offset_ray(v3(P4.x, P4.y, P4.z), v3(N4.x, N4.y, N4.z));
      const ShadowRay s = make_shadow_ray<true>(sc, fp, make_float4(o.x, o.y, o.z, 0.0f), (uint32_t)rl.reservoirs[pix].Y);
      trav_init(t, s.ro, s.rd, s.ro.w, s.rd.w, s.tlimit);
   };
   while (w.next(false, start)) {
      bool occluded;
      if (walk_step<true, false>(w, sc, occluded)) {
         if (occluded)
            n_occluded++;
         else
            rl.vis[pix] = 255;
      }
   }
   wave_add(&rl.counters[1], n_occluded);
}

void launch_hybrid_clear(const LaunchCfg& c, const HybridDev& hd) {
   k_hybrid_clear<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(hd, hd.W * hd.H);
}
void launch_hybrid_gbuffer_cast(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const HybridDev& hd, const SunGridDev* camera_grid) {
   const RawRays rr{hd.nrm, hd.pbr, hd.pos};
   launch_gbuffer_cast(c, fp, sc, rr, whole_frame(hd.W, hd.H), nullptr, camera_grid);
}
void launch_hybrid_gbuffer_resolve(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd) {
   const uint32_t n = hd.W * hd.H;
   k_hybrid_gbuffer_resolve<<<stream_grid(c, n), kBlock, 0, c.stream>>>(sc, hd, n);
}
void launch_hybrid_gbuffer(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const HybridDev& hd, const SunGridDev* camera_grid) {
   launch_hybrid_gbuffer_cast(c, fp, sc, hd, camera_grid);
   launch_hybrid_gbuffer_resolve(c, sc, hd);
}
void launch_hybrid_shadows(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd) {
   k_hybrid_shadow<<<persistent_grid(hd.W * hd.H, c.num_cus * c.shadow_blocks_per_cu), kBlock, 0, c.stream>>>(sc, hd);
}
void launch_hybrid_restir_lights(const LaunchCfg& c, const FrameParams& fp, const SceneDev& sc, const HybridDev& hd, const HybridRestirDev& rl) {
   k_hybrid_restir_classify<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(hd, rl);
   k_hybrid_restir_trace<<<persistent_grid(hd.W * hd.H, c.num_cus * c.shadow_blocks_per_cu), kBlock, 0, c.stream>>>(sc, fp, hd, rl);
}
void launch_hybrid_reflections(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const IblMaps* ibl) {
   k_hybrid_reflect_classify<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(sc, hd);
   if (!ibl)
      k_hybrid_reflect<false><<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(sc, hd, IblMaps{});
   else
      k_hybrid_reflect<true><<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(sc, hd, *ibl);
}

// ------------------------------------------------------------------------------------------
// The hybrid graph's final frame (build_render_graph, renderers/mod.rs:136-186): ssao_pass (ssao.frag), deferred_pass
// (deferred.frag + pbr_lighting.glsl / brdf.glsl), atmosphere_pass (atmosphere.frag, cubemap off) and present_pass (present.frag +
// fxaa.glsl). Arithmetic and orientation: DESIGN.md section 2 "Hybrid frame passes".
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_hybrid_frame_clear(HybridFrameDev fd, uint32_t n) {
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
      fd.ssao[i] = 65535;
      fd.deferred[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      fd.present[i] = make_uchar4(255, 255, 255, 0);
   }
}

// texture(image, uv) of an RGBA32F image through LINEAR + MIRRORED_REPEAT at texel coordinates (x, y) = uv * size - 0.5 (texture.rs's
// sampler, level 0): sample_texture's filter - weights x - floor(x), (t00 (1 - ax) + t10 ax) (1 - ay) + (t01 (1 - ax) + t11 ax) ay.
// Coordinates beyond 1e9 texels read 0, as there.
__device__ __forceinline__ V3 bilinear_rgb(const float4* __restrict__ img, uint32_t W, uint32_t H, float x, float y) {
   if (!(fabsf(x) < 1e9f) || !(fabsf(y) < 1e9f)) return v3(0.0f, 0.0f, 0.0f);
   const float fx = floorf(x), fy = floorf(y);
   const float ax = x - fx, ay = y - fy;
   const int x0 = mirror_index((int)fx, (int)W), x1 = mirror_index((int)fx + 1, (int)W);
   const int y0 = mirror_index((int)fy, (int)H), y1 = mirror_index((int)fy + 1, (int)H);
   const V3 t00 = xyz(img[(size_t)y0 * W + x0]), t10 = xyz(img[(size_t)y0 * W + x1]);
   const V3 t01 = xyz(img[(size_t)y1 * W + x0]), t11 = xyz(img[(size_t)y1 * W + x1]);
   const V3 a = t00 * (1.0f - ax) + t10 * ax;
   const V3 b = t01 * (1.0f - ax) + t11 * ax;
   return a * (1.0f - ay) + b * ay;
}

// ssao.frag:31-64, the fixed kernel (kernelSamples[i].xyz)
__device__ __forceinline__ V3 ssao_sample(int i) {
   constexpr float k[32][3] = {
      {-0.68217f, 0.23565f, 0.48243f}, {-0.14448f, 0.01628f, 0.22807f}, {0.00604f, 0.01909f, 0.0127f},   {0.09733f, 0.39072f, 0.7324f},
      {0.06055f, 0.87847f, 0.33303f},  {0.00734f, 0.19034f, 0.13091f},  {-0.01377f, 0.01745f, 0.00399f}, {0.01468f, 0.16627f, 0.09108f},
      {-0.10093f, -0.08015f, 0.06625f}, {-0.27125f, -0.39937f, 0.0601f}, {-0.06181f, -0.03065f, 0.01213f}, {-0.40189f, -0.48095f, 0.21808f},
      {0.04027f, -0.05818f, 0.26542f}, {-0.33535f, -0.07516f, 0.24997f}, {0.32748f, -0.18112f, 0.27292f}, {0.53962f, -0.03361f, 0.58926f},
      {-0.09598f, -0.25424f, 0.35754f}, {-0.17368f, 0.01261f, 0.23964f}, {0.1283f, 0.12573f, 0.16467f},  {-0.34418f, 0.19403f, 0.70285f},
      {-0.09686f, -0.0928f, 0.11447f}, {0.32727f, -0.49713f, 0.17518f}, {0.12345f, 0.13862f, 0.23822f},  {-0.39258f, -0.31128f, 0.67374f},
      {0.03308f, 0.07616f, 0.03422f},  {-0.31777f, 0.1885f, 0.40808f},  {-0.17464f, 0.28096f, 0.11686f}, {-0.50199f, -0.49002f, 0.2709f},
      {0.38629f, 0.15627f, 0.56716f},  {0.06649f, -0.05762f, 0.0857f},  {-0.1065f, -0.11726f, 0.10818f}, {0.53236f, -0.5286f, 0.45444f}};
   return v3(k[i][0], k[i][1], k[i][2]);
}

// ssao.frag:66-118 (radius 0.1, randomVec (1, 1, 0), strength 1.6: ssao.rs:11). Texel (x, y) of ssao_output samples the G-buffer at the
// UNFLIPPED in_uv, i.e. at texel (x, H-1-y), exactly; the projected samples go through FLIP_UV_Y and read bilinearly.
__global__ __launch_bounds__(kBlock) void k_hybrid_ssao(HybridDev hd, HybridFrameDev fd) {
   const uint32_t n = hd.W * hd.H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   const uint32_t x = i % hd.W, y = i / hd.W;
   const size_t src = (size_t)(hd.H - 1 - y) * hd.W + x;
   const float4 p4 = hd.pos[src];
   float occ = 1.0f;                                                                             // frag:76-79: the sky
   if (!(p4.x == 1.0f && p4.y == 1.0f && p4.z == 1.0f)) {
      const float4 f4 = mat4_mul(fd.view, p4.x, p4.y, p4.z, 1.0f);                               // frag:73
      const V3 frag = v3(f4.x, f4.y, f4.z);
      const float4 n4 = hd.nrm[src];
      const float* m = fd.inv_view;  // transpose(inverse(view)) * vec4(n, 0): row i of the transpose = column i of inverse_view
      const V3 nv = normalize3(v3(((m[0] * n4.x + m[1] * n4.y) + m[2] * n4.z) + m[3] * 0.0f, ((m[4] * n4.x + m[5] * n4.y) + m[6] * n4.z) + m[7] * 0.0f,
                                  ((m[8] * n4.x + m[9] * n4.y) + m[10] * n4.z) + m[11] * 0.0f));  // frag:81-83
      const V3 rnd = v3(1.0f, 1.0f, 0.0f);
      const V3 tangent = normalize3(rnd - nv * dot3(rnd, nv));                                  // frag:90
      const V3 bitangent = cross3(tangent, nv);                                                 // frag:91
      float o = 0.0f;
#pragma unroll 4
      for (int k = 0; k < 32; k++) {
         const V3 kk = ssao_sample(k);
         const V3 sp = frag + ((tangent * kk.x + bitangent * kk.y) + nv * kk.z) * 0.1f;         // frag:98-99
         const float4 c = mat4_mul(fd.proj, sp.x, sp.y, sp.z, 1.0f);                            // frag:102-103
         const float u = (c.x / c.w) * 0.5f + 0.5f, v = 1.0f - ((c.y / c.w) * 0.5f + 0.5f);   // frag:104-106
         const V3 q = bilinear_rgb(hd.pos, hd.W, hd.H, u * (float)hd.W - 0.5f, v * (float)hd.H - 0.5f);
         const float depth = mat4_mul(fd.view, q.x, q.y, q.z, 1.0f).z;                          // frag:108
         float t = 0.1f / fabsf(frag.z - depth);                                                // frag:110: smoothstep(0, 1, .)
         t = fminf(fmaxf(t, 0.0f), 1.0f);
         const float range = (t * t) * (3.0f - 2.0f * t);
         o = o + (depth >= sp.z ? 1.0f : 0.0f) * range;                                         // frag:111
      }
      occ = 1.0f - (o / 32.0f) * 1.6f;                                                          // frag:114-115
   }
   fd.ssao[i] = (uint16_t)unorm16(occ);
}

// the light-only terms of surfaceShading (pbr_lighting.glsl:36-53), once per light: record 0 is deferred.frag:74's sun, record k the
// light k - 1 of the uh_add_light table
__global__ void k_hybrid_light_prep(HybridFrameDev fd) {
   for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= fd.num_lights; i += gridDim.x * blockDim.x) {
      float type, spot;
      V3 pos, dir, att;
      float4 color;
      if (i == 0) {
         type = 0.0f;
         spot = 0.0f;
         pos = v3(0.0f, 0.0f, 0.0f);
         dir = v3(fd.sun_raw[0] * -1.0f, fd.sun_raw[1] * 1.0f, fd.sun_raw[2] * -1.0f);
         att = v3(1.0f, 1.0f, 1.0f);
         color = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
      } else {
         const UhGpuLight& l = fd.raw_lights[i - 1];
         type = l.light_type;
         spot = l.spot;
         pos = v3(l.position[0], l.position[1], l.position[2]);
         dir = v3(l.direction[0], l.direction[1], l.direction[2]);
         att = v3(l.attenuation[0], l.attenuation[1], l.attenuation[2]);
         color = make_float4(l.color[0], l.color[1], l.color[2], l.color[3]);
      }
      HybridLight h;
      h.mode = type == 0.0f ? 0.0f : type == 1.0f ? 1.0f : type == 2.0f ? 2.0f : 3.0f;
      V3 d = v3(0.0f, 0.0f, 0.0f);
      if (type == 0.0f) d = normalize3(dir * v3(-1.0f, 1.0f, -1.0f));  // :38
      if (type == 2.0f) d = normalize3(dir);                           // :51
      h.pos[0] = pos.x, h.pos[1] = pos.y, h.pos[2] = pos.z;
      h.color[0] = color.x, h.color[1] = color.y, h.color[2] = color.z;
      h.spot = spot;
      h.att[0] = att.x, h.att[1] = att.y, h.att[2] = att.z;
      h.dir[0] = d.x, h.dir[1] = d.y, h.dir[2] = d.z;
      h.pad0 = h.pad1 = 0.0f;
      fd.lights[i] = h;
   }
}

// deferred.frag:43-118 with surfaceShading (pbr_lighting.glsl:20-79) and brdf.glsl. One lane per pixel, no grid-stride loop (so the
// light records, read at wave-uniform addresses from a table nothing in the kernel writes, become scalar loads), the light loop
// wave-uniform with a scalar branch on the light's mode. The light-independent terms (V, F0, NdotV, GeometrySchlickGGX(NdotV), a2,
// k, 1 - metallic, 4 NdotV) are hoisted: the same operations on the same operands, so the same bits.
// kIbl: the ambient term is imageBasedLighting on the IBL maps (frag:85-88) instead of 0.03 * diffuse * occlusion.
// kShadow (shadows_enabled = 1): calculateShadow on the cascaded shadow maps (frag:98-106) instead of the rt_shadows factor.
// kRestir (UH_HYBRID_RESTIR_LIGHTS): count is 1 (the sun); a pixel whose light-visibility texel is 255 adds the term of its reservoir's
// light, record Y + 1, times the reservoir's W_X ("Reservoir lights"): a per-lane record, so vector loads.

template <bool kIbl, bool kShadow, bool kRestir>
__global__ __launch_bounds__(kBlock) void k_hybrid_deferred(SceneDev sc, HybridDev hd, HybridFrameDev fd, const HybridLight* __restrict__ lights, uint32_t count,
                                                            IblMaps ibl, ShadowLookup sl, HybridRestirDev rl) {
   __shared__ float s_gamma[256];  // pow(c / 255, 2.2) of every UNORM8 value: pow in double, rounded to float
   s_gamma[threadIdx.x] = (float)pow((double)((float)threadIdx.x / 255.0f), (double)2.2f);
   __syncthreads();
   const uint32_t n = hd.W * hd.H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   const float4 P4 = hd.pos[i], N4 = hd.nrm[i], R4 = hd.pbr[i];
   const uchar4 A = hd.alb[i];
   const uint32_t material = (uint32_t)R4.w;                                                    // frag:46
   float mf = 1.0f, rf = 1.0f, type = 0.0f;
   V3 bc = v3(1.0f, 1.0f, 1.0f);
   if (material < sc.num_meshes) {
      const MeshShade& ms = sc.meshes[material];
      mf = ms.metallic;
      rf = ms.roughness;
      type = ms.type;
      bc = v3(ms.base_color[0], ms.base_color[1], ms.base_color[2]);
   }
   const V3 P = v3(P4.x, P4.y, P4.z), N = v3(N4.x, N4.y, N4.z);
   const float roughness = R4.y * rf, metallic = R4.x * mf, occlusion = R4.z;                   // frag:52-58
   const V3 diffuse = v3(s_gamma[A.x], s_gamma[A.y], s_gamma[A.z]);                            // frag:61
   const V3 base = diffuse * bc;                                                                // frag:65
   const V3 V = normalize3(v3(hd.eye[0], hd.eye[1], hd.eye[2]) - P);                            // lighting:26
   V3 Lo = direct_lighting(lights, count, P, N, V, base, metallic, roughness);
   if (kRestir && rl.vis[i] == 255) {
      const UhReservoir r = rl.reservoirs[i];
      const LightTerm t = light_term(lights[r.Y + 1], surface_terms(N, V, base, metallic, roughness), P, N, V, base);
      Lo = Lo + (((t.c * t.rad) * t.NdotL) * r.W_X);
   }
   V3 ambient = (0.03f * diffuse) * occlusion;                                                  // frag:83
   if (kIbl) ambient = ibl::image_based_lighting(ibl, P, base, N, metallic, roughness, occlusion, v3(hd.eye[0], hd.eye[1], hd.eye[2]));  // frag:85-88
   V3 color = ambient + Lo;                                                                     // frag:90
   if (fd.rt_on && type == 1.0f) {                                                              // frag:92-95: mix(c, r, 1.0)
      const uchar4 r = hd.refl[i];
      const V3 refl = v3(sc.unorm_lut[r.x], sc.unorm_lut[r.y], sc.unorm_lut[r.z]);
      color = color * (1.0f - 1.0f) + refl * 1.0f;
   }
   if (kShadow)
      color = color * calculate_shadow(sl, fd.view, P);                                         // frag:98-106
   else if (fd.rt_on)
      color = color * fmaxf(sc.unorm_lut[hd.shadow[i]], 0.3f);                                  // frag:108-111
   if (fd.ssao_on) color = color * ((float)fd.ssao[(size_t)(hd.H - 1 - i / hd.W) * hd.W + i % hd.W] / 65535.0f);  // frag:55,113-115
   fd.deferred[i] = make_float4(color.x, color.y, color.z, 1.0f);
}

// atmosphere.frag (cubemap_enabled = 0) on the pixels the G-buffer cast missed: compacted first (one atomic per wave), so that
// geometry pixels cost nothing; skip (nullable): the marching-cubes pass's visibility, whose covered pixels fail the atmosphere pass's
// depth test
__global__ __launch_bounds__(kBlock) void k_hybrid_sky_classify(HybridDev hd, HybridFrameDev fd, const uint32_t* __restrict__ skip) {
   queue_pixels(hd.W * hd.H, fd.sky_counter, hd.queue, [&](uint32_t pix) { return hd.pos[pix].w == 0.0f && (!skip || skip[pix] == 0xFFFFFFFFu); });
}
// kCube (cubemap_enabled = 1): textureLod(environment, dir * (1, -1, 1), 2) (frag:27-29) instead of IntegrateScattering
template <bool kCube>
__global__ __launch_bounds__(kBlock) void k_hybrid_sky(FrameParams fp, HybridDev hd, HybridFrameDev fd, IblMaps ibl) {
   const uint32_t count = *fd.sky_counter;
   const V3 sun = v3(hd.sun_dir[0], hd.sun_dir[1], hd.sun_dir[2]);
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
      const uint32_t pix = hd.queue[i];
      V3 o, d;
      primary_ray(fp, pix % hd.W, pix / hd.W, 0.5f, 0.5f, o, d);  // origin: inverse_view's translation (extract_camera_position)
      const V3 c = kCube ? ibl::cube_lod(ibl.env, v3(d.x, -d.y, d.z), 2.0f)                     // frag:27-29
                         : sky::integrate_scattering(o, d, 999999999.0f, sun);                  // frag:19-32
      fd.deferred[pix] = make_float4(c.x, c.y, c.z, 1.0f);                                      // frag:35
   }
}

// present.frag + fxaa.glsl (enabled 1, debug 0, threshold 0.45: present.rs:10-23; SCREEN_WIDTH / HEIGHT 2000 x 1260 at every size)
__device__ __forceinline__ float rgb2luma(V3 c) { return sqrtf(dot3(c, v3(0.299f, 0.587f, 0.114f))); }  // fxaa:12-15
__device__ __forceinline__ float srgb_pow(float c) {                                            // view.glsl:53-61, pow in double
   if (c < 0.0031308f) return c * 12.92f;
   return 1.055f * (float)pow((double)c, (double)(1.0f / 2.4f)) - 0.055f;
}
__global__ __launch_bounds__(kBlock) void k_hybrid_present(HybridDev hd, HybridFrameDev fd) {
   const uint32_t W = hd.W, H = hd.H, n = W * H, i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= n) return;
   const float fW = (float)W, fH = (float)H;
   const float u = ((float)(i % W) + 0.5f) / fW, v = ((float)(i / W) + 0.5f) / fH;             // present.frag:24 FLIP_UV_Y(in_uv)
   const float4* img = fd.deferred;
   auto tex = [&](float uu, float vv) { return bilinear_rgb(img, W, H, uu * fW - 0.5f, vv * fH - 0.5f); };
   auto off = [&](int ox, int oy) { return rgb2luma(bilinear_rgb(img, W, H, (u * fW + (float)ox) - 0.5f, (v * fH + (float)oy) - 0.5f)); };
   const V3 center = tex(u, v);
   V3 color = center;
   if (fd.fxaa_on) {
      const float lC = rgb2luma(center);
      const float lD = off(0, -1), lU = off(0, 1), lL = off(-1, 0), lR = off(1, 0);
      const float lMin = fminf(lC, fminf(fminf(lD, lU), fminf(lL, lR)));
      const float lMax = fmaxf(lC, fmaxf(fmaxf(lD, lU), fmaxf(lL, lR)));
      const float range = lMax - lMin;
      if (!(range < fmaxf(0.0312f, lMax * 0.45f))) {                                            // fxaa:49
         const float lDL = off(-1, -1), lUR = off(1, 1), lUL = off(-1, 1), lDR = off(1, -1);
         const float lDU = lD + lU, lLR = lL + lR;
         const float lLC = lDL + lUL, lDC = lDL + lDR, lRC = lDR + lUR, lUC = lUR + lUL;
         const float eH = (fabsf(-2.0f * lL + lLC) + fabsf(-2.0f * lC + lDU) * 2.0f) + fabsf(-2.0f * lR + lRC);
         const float eV = (fabsf(-2.0f * lU + lUC) + fabsf(-2.0f * lC + lLR) * 2.0f) + fabsf(-2.0f * lD + lDC);
         const bool horiz = eH >= eV;
         const float l1 = horiz ? lD : lL, l2 = horiz ? lU : lR;
         const float g1 = l1 - lC, g2 = l2 - lC;
         const bool steep1 = fabsf(g1) >= fabsf(g2);
         const float gs = 0.25f * fmaxf(fabsf(g1), fabsf(g2));
         const float isx = 1.0f / 2000.0f, isy = 1.0f / 1260.0f;
         float step = horiz ? isy : isx;
         float avg;
         if (steep1) {
            step = -step;
            avg = 0.5f * (l1 + lC);
         } else {
            avg = 0.5f * (l2 + lC);
         }
         float cu = u, cv = v;
         if (horiz)
            cv = cv + step * 0.5f;
         else
            cu = cu + step * 0.5f;
         const float ox = horiz ? isx : 0.0f, oy = horiz ? 0.0f : isy;
         float u1 = cu - ox, v1 = cv - oy, u2 = cu + ox, v2 = cv + oy;
         float e1 = rgb2luma(tex(u1, v1)), e2 = rgb2luma(tex(u2, v2));
         e1 = e1 - avg;
         e2 = e2 - avg;
         bool r1 = fabsf(e1) >= gs, r2 = fabsf(e2) >= gs;
         if (!r1) u1 = u1 - ox, v1 = v1 - oy;
         if (!r2) u2 = u2 + ox, v2 = v2 + oy;
         if (!(r1 && r2)) {
            const float quality[7] = {1.5f, 2.0f, 2.0f, 2.0f, 2.0f, 4.0f, 8.0f};
            for (int it = 2; it < 7; it++) {
               if (!r1) e1 = rgb2luma(tex(u1, v1)) - avg;
               if (!r2) e2 = rgb2luma(tex(u2, v2)) - avg;
               r1 = fabsf(e1) >= gs;
               r2 = fabsf(e2) >= gs;
               if (!r1) u1 = u1 - ox * quality[it], v1 = v1 - oy * quality[it];
               if (!r2) u2 = u2 + ox * quality[it], v2 = v2 + oy * quality[it];
               if (r1 && r2) break;
            }
         }
         const float d1 = horiz ? (u - u1) : (v - v1), d2 = horiz ? (u2 - u) : (v2 - v);
         const bool dir1 = d1 < d2;
         const float dmin = fminf(d1, d2), thick = d1 + d2;
         const float pix_off = -dmin / thick + 0.5f;
         const bool smaller = lC < avg;
         const bool correct = ((dir1 ? e1 : e2) < 0.0f) != smaller;
         float fo = correct ? pix_off : 0.0f;
         const float lAvg = (1.0f / 12.0f) * (((2.0f * (lDU + lLR)) + lLC) + lRC);
         const float s1 = fminf(fmaxf(fabsf(lAvg - lC) / range, 0.0f), 1.0f);
         const float s2 = ((-2.0f * s1 + 3.0f) * s1) * s1;
         fo = fmaxf(fo, (s2 * s2) * 0.75f);
         float fu = u, fv = v;
         if (horiz)
            fv = fv + fo * step;
         else
            fu = fu + fo * step;
         color = tex(fu, fv);
      }
   }
   const V3 s = v3(srgb_pow(color.x), srgb_pow(color.y), srgb_pow(color.z));                  // present.frag:37
   fd.present[i] = make_uchar4((unsigned char)unorm8(s.z), (unsigned char)unorm8(s.y), (unsigned char)unorm8(s.x), 255);  // B8G8R8A8, alpha 1.0
}

void launch_hybrid_frame_clear(const LaunchCfg& c, const HybridDev& hd, const HybridFrameDev& fd) {
   k_hybrid_frame_clear<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(fd, hd.W * hd.H);
}
static inline dim3 one_lane_per_pixel(const HybridDev& hd) { return dim3((hd.W * hd.H + kBlock - 1) / kBlock); }
void launch_hybrid_ssao(const LaunchCfg& c, const HybridDev& hd, const HybridFrameDev& fd) {
   k_hybrid_ssao<<<one_lane_per_pixel(hd), kBlock, 0, c.stream>>>(hd, fd);
}
void launch_hybrid_light_prep(const LaunchCfg& c, const HybridFrameDev& fd) {
   k_hybrid_light_prep<<<(fd.num_lights + 1 + 255) / 256, 256, 0, c.stream>>>(fd);
}
void launch_hybrid_deferred(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const HybridFrameDev& fd, const IblMaps* ibl,
                            const ShadowLookup* shadow, const HybridRestirDev* restir) {
   launch_hybrid_light_prep(c, fd);
   const IblMaps im = ibl ? *ibl : IblMaps{};
   const ShadowLookup sl = shadow ? *shadow : ShadowLookup{};
   const HybridRestirDev rl = restir ? *restir : HybridRestirDev{};
   const dim3 grid = one_lane_per_pixel(hd);
   const uint32_t n = restir ? 1 : fd.num_lights + 1;
   as_constant(ibl != nullptr, [&](auto kIbl) {
      as_constant(shadow != nullptr, [&](auto kShadow) {
         as_constant(restir != nullptr, [&](auto kRestir) {
            k_hybrid_deferred<decltype(kIbl)::value, decltype(kShadow)::value, decltype(kRestir)::value><<<grid, kBlock, 0, c.stream>>>(sc, hd, fd, fd.lights, n, im, sl, rl);
         });
      });
   });
}
void launch_hybrid_sky(const LaunchCfg& c, const FrameParams& fp, const HybridDev& hd, const HybridFrameDev& fd, const IblMaps* cube, const uint32_t* skip) {
   k_hybrid_sky_classify<<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(hd, fd, skip);
   if (!cube)
      k_hybrid_sky<false><<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(fp, hd, fd, IblMaps{});
   else
      k_hybrid_sky<true><<<stream_grid(c, hd.W * hd.H), kBlock, 0, c.stream>>>(fp, hd, fd, *cube);
}
void launch_hybrid_present(const LaunchCfg& c, const HybridDev& hd, const HybridFrameDev& fd) {
   k_hybrid_present<<<one_lane_per_pixel(hd), kBlock, 0, c.stream>>>(hd, fd);
}

}  // namespace uh
