// path_shading.h — the per-path arithmetic of the reference's closest-hit, miss and raygen shaders that more than one kernel runs: the
// wavefront's k_shade_hit / k_shade_miss / k_trace_shadow (kernels.hip) and k_path_fused (path_fused.hip) give a path the same words
// because they call the same functions here; the hybrid reflections (hybrid_kernels.hip) use the surface part.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"

namespace uh {

// ---- shadow rays (reference.rgen:63-79 sun, :81-122 light)
struct ShadowRay {
   float4 ro, rd;  // origin / direction (tmin, tmax in w)
   float tlimit;
};
// light_bits: the path's light index (radiance.w), read by a light ray only
template <bool LIGHT>
__device__ __forceinline__ ShadowRay make_shadow_ray(const SceneDev& sc, const FrameParams& fp, float4 ro, uint32_t light_bits) {
   ShadowRay s;
   s.ro = make_float4(ro.x, ro.y, ro.z, 0.001f);
   s.tlimit = INFINITY;
   if (LIGHT) {
      const int light_index = (int)light_bits;
      V3 lpos = v3(0, 0, 0);
      if (light_index >= 0 && (uint32_t)light_index < sc.num_lights) lpos = xyz(sc.lights[2 * light_index]);
      const V3 o = v3(ro.x, ro.y, ro.z);
      const V3 dir = normalize3(lpos - o);  // rgen:113
      s.tlimit = length3(lpos - o);         // rgen:114
      s.rd = make_float4(dir.x, dir.y, dir.z, 10000.0f);
   } else {
      s.rd = make_float4(fp.sun_dir[0], fp.sun_dir[1], fp.sun_dir[2], 10000.0f);  // rgen:64
   }
   return s;
}
// the radiance record the path gets if its shadow ray is unoccluded (rgen:69-78 / :118-122)
template <bool LIGHT>
__device__ __forceinline__ float4 shadow_lit(float4 thr, float4 rad) {
   if (LIGHT) {
      const float f = thr.w;
      return make_float4(rad.x + thr.x * f, rad.y + thr.y * f, rad.z + thr.z * f, rad.w);
   }
   return make_float4(rad.x + thr.x, rad.y + thr.y, rad.z + thr.z, rad.w);
}
// The sun rays' verdicts (PathState::sun_lit, FrameParams::sun_verdicts). A sun ray is a predicate: with verdicts its kernels leave one
// bit per ray and touch the path state through the origin plane alone; k_shade_hit(b + 1), the miss shading and k_flush_survivors -
// which read the path's throughput and radiance next anyway - add the throughput where they hold both, with shadow_lit's expression.
__device__ __forceinline__ unsigned long long* sun_lit_word(const PathState& ps, uint32_t pos) { return ps.sun_lit + (pos >> 6); }
// Is the radiance of the paths of bounce b's queue materialised? Never for bounce 0 (it is zero). With verdicts not for bounce 1
// either: nothing adds to a path's radiance before k_shade_hit(1) (or the miss shading, or the flush) reads it - they start from
// 0.0f and add the lit paths' throughput, the very words the stored zero would have given.
__device__ __forceinline__ bool rad_stored(const FrameParams& fp, uint32_t b) { return b > fp.sun_verdicts; }
constexpr uint32_t kSunLitBit = 0x80000000u;  // the verdict beside a queue position (k_shade_hit's lists, Q_MISS): positions stay below 2^31
// A stored radiance as (r, g, b, 0 or the light index). SLIM (FrameParams::slim_state): r came with the throughput quad `thr` the caller
// holds, (g, b) is the pair of plane 3; otherwise plane 3's quad. pos: the queue position with its shard segment.
typedef float v2f_t __attribute__((ext_vector_type(2)));
template <bool SLIM>
__device__ __forceinline__ float4 ld_rad(const PathRecs& rec, uint32_t pos, float4 thr) {
   if constexpr (SLIM) {
      const v2f_t gb = __builtin_nontemporal_load(reinterpret_cast<const v2f_t*>(rec_pair(rec, pos)));
      return make_float4(thr.w, gb.x, gb.y, 0.0f);
   } else
      return ld_rec(rec_quad(rec, pos, REC_RAD));
}
__device__ __forceinline__ void st_rad_pair(const PathRecs& rec, uint32_t pos, float g, float b) {
   const v2f_t gb = {g, b};
   __builtin_nontemporal_store(gb, reinterpret_cast<v2f_t*>(rec_pair(rec, pos)));
}

// pos: the path's position in the bounce's ray queue (shard segment included), id: its path id. The path ends here: its radiance
// goes to the per-id array, with the raygen's RNG word (the frame's next sample starts from it, rgen:28-31).
// sun_lit: the verdict of the sun ray the path cast when it scattered, not yet added to its radiance (FrameParams::sun_verdicts)
// SLIM (FrameParams::slim_state): behind bounce 0 the id is the origin quad's w, not `id`; throughput | radiance.r and the (g, b) pair;
// the per-id record's w (the raygen RNG word, which only a second sample of the frame would read) is zero
template <bool SLIM = false>
__device__ __forceinline__ void shade_miss_path(const FrameParams& fp, const PathState& ps, uint32_t pos, uint32_t id, uint32_t bounce, bool sun_lit) {
   const PathRecs rec = ps.set[bounce & 1];
   const bool implicit = bounce == 0 && fp.primary_implicit;  // origin and throughput of a primary ray: not stored (FrameParams)
   float4 ro, rd_implicit = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   if (implicit)
      primary_state(fp, id, ro, rd_implicit);
   else
      ro = ld_rec(rec_quad(rec, pos, REC_ORIGIN));
   if constexpr (SLIM) {
      if (bounce != 0) id = __float_as_uint(ro.w);
      ro.w = 0.0f;
   }
   V3 sky_color = v3(0.0f, 0.0f, 0.0f);
   if (fp.furnace) {
      sky_color = v3(1.0f, 1.0f, 1.0f);  // rmiss:12 with FURNACE_TEST defined: the #ifndef block (rmiss:14-28) is compiled out
   } else if (fp.sky_enabled == 1) {
      const float4 rd = implicit ? rd_implicit : ld_rec(rec_quad(rec, pos, REC_DIR));
      V3 c = sky::integrate_scattering(v3(ro.x, ro.y, ro.z), v3(rd.x, rd.y, rd.z), 999999999.0f, v3(fp.sun_dir[0], fp.sun_dir[1], fp.sun_dir[2]));
      sky_color = v3(fminf(c.x, 1.0f), fminf(c.y, 1.0f), fminf(c.z, 1.0f));  // rmiss:22
   }
   float4 thr = make_float4(1.0f, 1.0f, 1.0f, 0.0f);  // rgen:39
   if (!implicit) thr = ld_rec(rec_quad(rec, pos, REC_THR));
   float4 rad = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   if (rad_stored(fp, bounce)) rad = ld_rad<SLIM>(rec, pos, thr);
   if (sun_lit) rad = shadow_lit<false>(thr, rad);                           // rgen:69-78, of the bounce before
   V3 t = v3(thr.x, thr.y, thr.z) * sky_color;                               // rgen:48
   st_stream(ps.radf + id, make_float4(rad.x + t.x, rad.y + t.y, rad.z + t.z, ro.w));   // rgen:55
}

// Material type 4 - an EXTENSION that no reference scene uses: the Cook-Torrance BRDF of
// include/pbr_lighting.glsl:20-79 / include/brdf.glsl:3-36,82-85 (GGX D, Smith-Schlick G with k = (r+1)^2/8, Schlick F,
// kD = (1-F)(1-metallic), +0.0001 in the denominator) evaluated for the Lambertian-style scatter direction
// L = normalize(n + randomPointInUnitSphere) and returned as BRDF * cos / pdf with pdf = cos/pi, i.e.
// kD * baseColor + specular * pi. Same operations in the same order as oracle.cpp::pbr_weight (bit-identical).
__device__ __forceinline__ V3 pbr_weight(V3 N, V3 V, V3 L, V3 base, float metallic, float roughness) {
   const float PI = 3.14159265359f;
   const V3 H = normalize3(V + L);
   const float a = roughness * roughness, a2 = a * a;
   const float NdotH = fmaxf(dot3(N, H), 0.0f), NdotH2 = NdotH * NdotH;
   float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
   denom = (PI * denom) * denom;
   const float NDF = a2 / denom;
   const float NdotV = fmaxf(dot3(N, V), 0.0f), NdotL = fmaxf(dot3(N, L), 0.0f);
   const float r = roughness + 1.0f, k = (r * r) / 8.0f;
   const float gV = NdotV / (NdotV * (1.0f - k) + k), gL = NdotL / (NdotL * (1.0f - k) + k);
   const float G = gL * gV;
   const float c = fminf(fmaxf(1.0f - fmaxf(dot3(H, V), 0.0f), 0.0f), 1.0f);
   const float c5 = ((c * c) * (c * c)) * c;
   const float om = 1.0f - metallic;
   const V3 F0 = v3(0.04f * om + base.x * metallic, 0.04f * om + base.y * metallic, 0.04f * om + base.z * metallic);
   const V3 F = v3(F0.x + (1.0f - F0.x) * c5, F0.y + (1.0f - F0.y) * c5, F0.z + (1.0f - F0.z) * c5);
   const V3 kD = v3((1.0f - F.x) * om, (1.0f - F.y) * om, (1.0f - F.z) * om);
   const float den = (4.0f * NdotV) * NdotL + 0.0001f;
   const float dg = NDF * G;
   const V3 spec = v3((dg * F.x) / den, (dg * F.y) / den, (dg * F.z) / den);
   return v3(kD.x * base.x + spec.x * PI, kD.y * base.y + spec.y * PI, kD.z * base.z + spec.z * PI);
}

__device__ __forceinline__ float schlick_reflectance(float cosine, float ref_idx) {  // rchit:12-18
   float r0 = (1.0f - ref_idx) / (1.0f + ref_idx);
   r0 = r0 * r0;
   float x = 1.0f - cosine;
   float x5 = ((x * x) * (x * x)) * x;  // pow(x, 5.0)
   return r0 + (1.0f - r0) * x5;
}
__device__ __forceinline__ V3 reflect3(V3 I, V3 N) { return I - N * (2.0f * dot3(N, I)); }
__device__ __forceinline__ V3 refract3(V3 I, V3 N, float eta) {
   float dn = dot3(N, I);
   float k = 1.0f - eta * eta * (1.0f - dn * dn);
   if (k < 0.0f) return v3(0, 0, 0);
   return I * eta - N * (eta * dn + sqrtf(k));
}

// ---- the closest-hit shader's arithmetic, shared by k_shade_hit (one bounce of a wavefront) and k_path_fused (a lone frame's later
// bounces inside one persistent kernel): the same expressions in the same order, so both give the path the same words
struct SurfaceHit {
   V3 world_normal, origin;  // rchit:32-37; where the path goes on from (and its shadow rays start): rgen:59-60
   float uu, vv;             // rchit:39
   uint32_t mesh_index;
};
// s0..s3: the hit's shading packet (SceneDev::shade); the mesh record comes second because its index is in the packet
__device__ __forceinline__ void surface_normal_uv(const float4 s0, const float4 s1, const float4 s2, const float4 s3, float bu, float bv, V3& normal, float& uu, float& vv) {
   const V3 n0 = v3(s0.x, s0.y, s0.z), n1 = v3(s0.w, s1.x, s1.y), n2 = v3(s1.z, s1.w, s2.x);
   const float uv0x = s2.y, uv0y = s2.z, uv1x = s2.w, uv1y = s3.x, uv2x = s3.y, uv2y = s3.z;
   const float bx = 1.0f - bu - bv, by = bu, bz = bv;                            // rchit:30
   normal = (n0 * bx + n1 * by) + n2 * bz;                                       // rchit:31
   uu = (uv0x * bx + uv1x * by) + uv2x * bz;                                     // rchit:39
   vv = (uv0y * bx + uv1y * by) + uv2y * bz;
}
__device__ __forceinline__ V3 world_normal_of(const MeshShade& ms, V3 normal, V3 ray_dir) {
   V3 wn = v3((normal.x * ms.w2o[0] + normal.y * ms.w2o[3]) + normal.z * ms.w2o[6],
              (normal.x * ms.w2o[1] + normal.y * ms.w2o[4]) + normal.z * ms.w2o[7],
              (normal.x * ms.w2o[2] + normal.y * ms.w2o[5]) + normal.z * ms.w2o[8]);  // rchit:32
   V3 world_normal = normalize3(wn);
   if (dot3(world_normal, ray_dir) > 0.0f) world_normal = vneg(world_normal);   // rchit:35-37
   return world_normal;
}
// Does the path go on? Decided by the material type and the side the ray came from (rchit:47-89) - nothing the texels bring
__device__ __forceinline__ bool path_scatters(const MeshShade& ms, V3 ray_dir, V3 world_normal) {
   return (ms.type == 0.0f || ms.type == 4.0f) ? dot3(ray_dir, world_normal) < 0.0f : (ms.type == 1.0f || ms.type == 2.0f);
}
// rchit:47-89: the scatter direction; `color` in: texel x base colour (rchit:40-41), out: what the throughput is multiplied by
__device__ __forceinline__ V3 material_scatter(const MeshShade& ms, V3 ray_dir, V3 world_normal, V3& color, uint32_t& seed) {
   V3 scatter = v3(0, 0, 0);
   if (ms.type == 0.0f) {                                                        // rchit:47-50
      scatter = world_normal + random_point_in_unit_sphere(seed);            // scattered = dot(ray, normal) < 0: path_scatters
   } else if (ms.type == 1.0f) {                                                 // rchit:52-59
      scatter = reflect3(normalize3(ray_dir), world_normal);
      scatter = scatter + ms.property * random_point_in_unit_sphere(seed);
      color = v3(1, 1, 1);
   } else if (ms.type == 2.0f) {                                                 // rchit:61-83
      V3 nd = normalize3(ray_dir);
      float dnd = dot3(nd, world_normal);
      V3 outward = dnd > 0 ? vneg(world_normal) : world_normal;
      float ratio = ms.property;
      ratio = dnd > 0 ? ratio : 1.0f / ratio;
      float cos_theta = fminf(dot3(-1.0f * nd, outward), 1.0f);
      float sin_theta = sqrtf(1.0f - cos_theta * cos_theta);
      bool cannot_refract = ratio * sin_theta > 1.0f;
      float reflectance = schlick_reflectance(cos_theta, ratio);
      if (cannot_refract || reflectance > random_float(seed))
         scatter = reflect3(nd, outward);
      else
         scatter = refract3(nd, outward, ratio);
      color = v3(1, 1, 1);
   } else if (ms.type == 4.0f) {
      // EXTENSION (never produced by the reference's scenes): Cook-Torrance, see pbr_weight()
      scatter = world_normal + random_point_in_unit_sphere(seed);
      color = pbr_weight(world_normal, -1.0f * normalize3(ray_dir), normalize3(scatter), color, ms.metallic, ms.roughness);
   } else {                                                                      // rchit:85-89: the path ends
      color = v3(1, 1, 1);
   }
   return scatter;
}
// rgen:81-121: which light the scattered path asks, and the weight f its throughput gets if the light is visible from `origin`
__device__ __forceinline__ bool select_light(const FrameParams& fp, const SceneDev& sc, uint32_t id, uint32_t& rng_x, V3 origin, float& f, int& light_index) {
   float light_sample_weight = 0.0f, total_weights = 1.0f;
   const uint32_t k = id % fp.n_owned;
   const uint32_t pix = fp.owned_pixels ? fp.owned_pixels[k] : k;
   uint32_t px = pix % fp.W;
   bool use_reservoir = (px > fp.W / 2 || fp.full_frame_restir) && fp.use_ris == 1;  // rgen:87
   if (use_reservoir) {
      UhReservoir rs = fp.spatial_of[id / fp.n_owned][pix];                // rgen:98 (the path's own frame of the batch)
      light_sample_weight = rs.W_X;
      total_weights = rs.W_sum;
      light_index = rs.Y;
   } else {
      sample_light_uniform(fp.num_lights_used, rng_x, light_index, light_sample_weight);  // rgen:107
      light_sample_weight = 1.0f / light_sample_weight;                    // rgen:108
   }
   if (total_weights != 0.0f) {                                            // rgen:112
      f = target_function(sc.lights, sc.num_lights, light_index, origin) * light_sample_weight;  // rgen:121
      return true;
   }
   return false;
}

}  // namespace uh
