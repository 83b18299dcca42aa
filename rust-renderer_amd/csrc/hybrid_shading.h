// hybrid_shading.h — the shading the hybrid graph's G-buffer and deferred passes (hybrid_kernels.hip) share with the forward pass
// (forward.hip): gbuffer.vert / forward.vert's per-vertex TBN and normal plus the fragment shaders' normal-map block, surfaceShading's
// light loop (pbr_lighting.glsl / brdf.glsl) and shadow_mapping.glsl's calculateShadow. Arithmetic: DESIGN.md section 2, "Hybrid
// passes", "Hybrid frame passes" and "Shadow maps".
#pragma once

#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"

namespace uh {

__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// mat3(world) * a: ((col0 * x + col1 * y) + col2 * z), world row-major
__device__ __forceinline__ V3 mat3_mul(const float* m, V3 a) {
   return v3((m[0] * a.x + m[1] * a.y) + m[2] * a.z, (m[3] * a.x + m[4] * a.y) + m[5] * a.z, (m[6] * a.x + m[7] * a.y) + m[8] * a.z);
}
// mat3(transpose(inverse(world))) * n with the row-major inverse: the same expression as world_normal_of (rchit:32)
__device__ __forceinline__ V3 inverse_transpose_mul(const float* w2o, V3 n) {
   return v3((n.x * w2o[0] + n.y * w2o[3]) + n.z * w2o[6], (n.x * w2o[1] + n.y * w2o[4]) + n.z * w2o[7], (n.x * w2o[2] + n.y * w2o[5]) + n.z * w2o[8]);
}

// gbuffer.vert:29-46 / forward.vert:44-55 per vertex, interpolated with the barycentrics (b0, b1, b2) of triangle (v0, v1, v2) of mesh m,
// then gbuffer.frag:27-51 / forward.frag:44-53: the shading normal nn and the uv
__device__ __forceinline__ void surface_attributes(const SceneDev& sc, const HybridMesh& m, const UhVertex& v0, const UhVertex& v1, const UhVertex& v2,
                                                   float b0, float b1, float b2, V3& nn, float& uu, float& vv) {
   auto lerp3 = [&](V3 a, V3 b, V3 c) { return (a * b0 + b * b1) + c * b2; };
   auto vec = [](const float* f) { return v3(f[0], f[1], f[2]); };
   uu = (v0.uv[0] * b0 + v1.uv[0] * b1) + v2.uv[0] * b2;
   vv = (v0.uv[1] * b0 + v1.uv[1] * b1) + v2.uv[1] * b2;
   const V3 n0 = vec(v0.normal), n1 = vec(v1.normal), n2 = vec(v2.normal);
   const V3 t0 = vec(v0.tangent), t1 = vec(v1.tangent), t2 = vec(v2.tangent);
   const V3 tangent = lerp3(t0, t1, t2);                                            // in_tangent.xyz
   if (tangent.x != 0.0f || tangent.y != 0.0f || tangent.z != 0.0f) {             // frag:41
      auto tbn = [&](V3 nk, V3 tk, V3& T, V3& B, V3& N) {                            // vert:31-35
         T = normalize3(mat3_mul(m.o2w, tk));
         B = normalize3(mat3_mul(m.o2w, cross3(nk, tk)));
         N = normalize3(mat3_mul(m.o2w, nk));
      };
      V3 T0, B0, N0, T1, B1, N1, T2, B2, N2;
      tbn(n0, t0, T0, B0, N0);
      tbn(n1, t1, T1, B1, N1);
      tbn(n2, t2, T2, B2, N2);
      const V3 T = lerp3(T0, T1, T2), B = lerp3(B0, B1, B2), N = lerp3(N0, N1, N2);
      const V3 nm = sample_texture(sc, sc.unorm_lut, m.normal_map, uu, vv);
      const V3 x = normalize3(v3(nm.x * 2.0f - 1.0f, nm.y * 2.0f - 1.0f, nm.z * 2.0f - 1.0f));  // frag:43
      nn = normalize3((T * x.x + B * x.y) + N * x.z);                                  // frag:44
   } else {
      nn = normalize3(lerp3(inverse_transpose_mul(m.w2o, n0), inverse_transpose_mul(m.w2o, n1), inverse_transpose_mul(m.w2o, n2)));  // vert:41, frag:39
   }
}

// gbuffer.frag:47-56's other three targets at a surface point of mesh `mesh` (shading normal nn, uv): normal (nn, 1), albedo the diffuse
// texel quantised (no base_color_factor, alpha 255), pbr (metallic = the metallic-roughness map's b, roughness = its g, occlusion = the
// occlusion map's r, the material index: mesh i has material i). The G-buffer cast (k_hybrid_gbuffer_resolve) and the rasterised
// G-buffer (k_gbuffer_raster_shade) share it.
__device__ __forceinline__ void gbuffer_targets(const SceneDev& sc, const HybridMesh& m, uint32_t mesh, V3 nn, float uu, float vv, float4& nrm,
                                                uchar4& alb, float4& pbr) {
   nrm = make_float4(nn.x, nn.y, nn.z, 1.0f);
   const V3 d = sample_texture(sc, sc.unorm_lut, m.diffuse_map, uu, vv);
   alb = make_uchar4((unsigned char)unorm8(d.x), (unsigned char)unorm8(d.y), (unsigned char)unorm8(d.z), 255);
   const V3 mr = sample_texture(sc, sc.unorm_lut, m.metallic_roughness_map, uu, vv);
   const V3 oc = sample_texture(sc, sc.unorm_lut, m.occlusion_map, uu, vv);
   pbr = make_float4(mr.z, mr.y, oc.x, (float)mesh);
}

constexpr float kPiBrdf = 3.14159265359f;  // brdf.glsl:1

// surfaceShading (pbr_lighting.glsl:20-79) with brdf.glsl, in two pieces: the light-independent terms (F0, NdotV,
// GeometrySchlickGGX(NdotV), a2, k, 1 - metallic, 4 NdotV), hoisted out of the light loop - the same operations on the same operands, so
// the same bits -, and one light's term from a record of k_hybrid_light_prep. direct_lighting sums the term over the records (the sun
// first); the deferred pass's reservoir term ("Reservoir lights") is the same function on one record.
struct SurfaceTerms {
   V3 F0;
   float om, a2, a2m1, k, omk, ggxV, nv4;
};
__device__ __forceinline__ SurfaceTerms surface_terms(V3 N, V3 V, V3 base, float metallic, float roughness) {
   SurfaceTerms s;
   s.om = 1.0f - metallic;
   s.F0 = v3(0.04f, 0.04f, 0.04f) * s.om + base * metallic;                                     // lighting:29-30
   const float NdotV = fmaxf(dot3(N, V), 0.0f);
   const float a = roughness * roughness;                                                       // brdf:5-6
   s.a2 = a * a;
   s.a2m1 = s.a2 - 1.0f;
   const float r1 = roughness + 1.0f;                                                           // brdf:19-20
   s.k = (r1 * r1) / 8.0f;
   s.omk = 1.0f - s.k;
   s.ggxV = NdotV / (NdotV * s.omk + s.k);                                                      // brdf:31
   s.nv4 = 4.0f * NdotV;                                                                        // lighting:71
   return s;
}
// one light: Lo += (c * rad) * NdotL. The branch on the light's mode is scalar where the record's address is wave-uniform.
struct LightTerm {
   V3 c, rad;
   float NdotL;
};
__device__ __forceinline__ LightTerm light_term(const HybridLight& hl, const SurfaceTerms& s, V3 P, V3 N, V3 V, V3 base) {
   const float mode = hl.mode;
   V3 L;
   float att;
   if (mode == 0.0f) {                                                                          // lighting:36-40
      L = v3(hl.dir[0], hl.dir[1], hl.dir[2]);
      att = 1.0f;
   } else if (mode == 3.0f) {
      L = v3(0.0f, 0.0f, 0.0f);
      att = 1.0f;
   } else {                                                                                     // lighting:41-53
      const V3 ptl = v3(hl.pos[0], hl.pos[1], hl.pos[2]) - P;
      const float d = sqrtf(dot3(ptl, ptl));
      L = ptl * (1.0f / d);
      const float den = (hl.att[0] * 1.0f + hl.att[1] * d) + hl.att[2] * (d * d);
      if (mode == 2.0f)
         att = powf(fmaxf(dot3(L, v3(hl.dir[0], hl.dir[1], hl.dir[2])), 0.0f), hl.spot) / den;
      else
         att = 1.0f / den;
   }
   LightTerm t;
   const V3 Hv = normalize3(V + L);                                                             // lighting:58
   t.rad = v3(hl.color[0] * att, hl.color[1] * att, hl.color[2] * att);                         // lighting:59
   const float NdotH = fmaxf(dot3(N, Hv), 0.0f);                                                // brdf:7-14
   float dn = (NdotH * NdotH) * s.a2m1 + 1.0f;
   dn = (kPiBrdf * dn) * dn;
   const float NDF = s.a2 / dn;
   t.NdotL = fmaxf(dot3(N, L), 0.0f);                                                           // brdf:28-36
   const float G = (t.NdotL / (t.NdotL * s.omk + s.k)) * s.ggxV;
   const float x = fminf(fmaxf(1.0f - fmaxf(dot3(Hv, V), 0.0f), 0.0f), 1.0f);                 // brdf:82-85
   const float p5 = ((x * x) * (x * x)) * x;
   const V3 F = s.F0 + (v3(1.0f, 1.0f, 1.0f) - s.F0) * p5;
   const V3 kD = (v3(1.0f, 1.0f, 1.0f) - F) * s.om;                                             // lighting:66-68
   const float NG = NDF * G, den2 = s.nv4 * t.NdotL + 0.0001f;                                  // lighting:70-72
   const V3 spec = v3((NG * F.x) / den2, (NG * F.y) / den2, (NG * F.z) / den2);
   const V3 kb = kD * base;                                                                     // lighting:76
   t.c = v3(kb.x / kPiBrdf + spec.x, kb.y / kPiBrdf + spec.y, kb.z / kPiBrdf + spec.z);
   return t;
}
// The same term for a light that is a direction L and a radiance Li and no record (the area-light pass, area_lights.hip), its two halves
// kept apart: d = kD * (Li * NdotL), without base / PI - the pass filters d and applies the base colour behind the filter -, and s =
// specular * (Li * NdotL); NdotL = dot(N, L) as the caller formed it, > 0. The operations of light_term in its order (DESIGN.md
// section 2, "Area lights").
struct LightHalves {
   V3 d, s;
};
__device__ __forceinline__ LightHalves light_halves(const SurfaceTerms& s, V3 N, V3 V, V3 L, float NdotL, V3 Li) {
   const V3 Hv = normalize3(V + L);                                                             // lighting:58
   const float NdotH = fmaxf(dot3(N, Hv), 0.0f);                                                // brdf:7-14
   float dn = (NdotH * NdotH) * s.a2m1 + 1.0f;
   dn = (kPiBrdf * dn) * dn;
   const float NDF = s.a2 / dn;
   const float G = (NdotL / (NdotL * s.omk + s.k)) * s.ggxV;                                    // brdf:28-36
   const float x = fminf(fmaxf(1.0f - fmaxf(dot3(Hv, V), 0.0f), 0.0f), 1.0f);                 // brdf:82-85
   const float p5 = ((x * x) * (x * x)) * x;
   const V3 F = s.F0 + (v3(1.0f, 1.0f, 1.0f) - s.F0) * p5;
   const V3 kD = (v3(1.0f, 1.0f, 1.0f) - F) * s.om;                                             // lighting:66-68
   const float NG = NDF * G, den2 = s.nv4 * NdotL + 0.0001f;                                    // lighting:70-72
   const V3 spec = v3((NG * F.x) / den2, (NG * F.y) / den2, (NG * F.z) / den2);
   const V3 rad = Li * NdotL;                                                                   // lighting:78's radiance * NdotL
   return LightHalves{kD * rad, spec * rad};
}
// summed over the light records of k_hybrid_light_prep (the sun first); the loop is wave-uniform
__device__ __forceinline__ V3 direct_lighting(const HybridLight* __restrict__ lights, uint32_t count, V3 P, V3 N, V3 V, V3 base, float metallic,
                                              float roughness) {
   const SurfaceTerms s = surface_terms(N, V, base, metallic, roughness);
   V3 Lo = v3(0.0f, 0.0f, 0.0f);
   for (uint32_t l = 0; l < count; l++) {
      const LightTerm t = light_term(lights[l], s, P, N, V, base);
      Lo = Lo + (t.c * t.rad) * t.NdotL;
   }
   return Lo;
}

// shadow_mapping.glsl calculateShadow: the cascade from the view-space depth, the light-space position divided by w, xy * 0.5 + 0.5,
// FLIP_UV_Y, then 3 x 3 PCF (x outer, y inner) of texture() reads of layer c - LINEAR + MIRRORED_REPEAT (texture.rs:85-94): the bilinear
// blend of bilinear_rgb at uv * size - 0.5 - each tap 0.3 when z - 0.0005 > depth, else 1.0 (1.0 when z is outside (-1, 1]); sum / 9
__device__ __forceinline__ float shadow_depth(const float* __restrict__ map, int S, float x, float y) {
   if (!(fabsf(x) < 1e9f) || !(fabsf(y) < 1e9f)) return 0.0f;
   const float fx = floorf(x), fy = floorf(y);
   const float ax = x - fx, ay = y - fy;
   const int x0 = mirror_index((int)fx, S), x1 = mirror_index((int)fx + 1, S);
   const int y0 = mirror_index((int)fy, S), y1 = mirror_index((int)fy + 1, S);
   const float t00 = map[(size_t)y0 * S + x0], t10 = map[(size_t)y0 * S + x1];
   const float t01 = map[(size_t)y1 * S + x0], t11 = map[(size_t)y1 * S + x1];
   const float a = t00 * (1.0f - ax) + t10 * ax;
   const float b = t01 * (1.0f - ax) + t11 * ax;
   return a * (1.0f - ay) + b * ay;
}
__device__ __forceinline__ float calculate_shadow(const ShadowLookup& sl, const float* view, V3 P) {
   const float vz = ((view[2] * P.x + view[6] * P.y) + view[10] * P.z) + view[14] * 1.0f;
   uint32_t c = 0;
   for (uint32_t i = 0; i < 3; i++)
      if (vz < -sl.params->cascade_splits[i]) c = i + 1;
   const float* m = sl.params->view_projection_matrices[c];
   const float lx = ((m[0] * P.x + m[4] * P.y) + m[8] * P.z) + m[12] * 1.0f;
   const float ly = ((m[1] * P.x + m[5] * P.y) + m[9] * P.z) + m[13] * 1.0f;
   const float lz = ((m[2] * P.x + m[6] * P.y) + m[10] * P.z) + m[14] * 1.0f;
   const float lw = ((m[3] * P.x + m[7] * P.y) + m[11] * P.z) + m[15] * 1.0f;
   const float px = lx / lw, py = ly / lw, pz = lz / lw;
   const float u = px * 0.5f + 0.5f, v = 1.0f - (py * 0.5f + 0.5f);
   const int S = (int)sl.size;
   const float fS = (float)S, ts = 1.0f / fS;
   const float* map = sl.maps + (size_t)c * sl.size * sl.size;
   const bool inside = pz <= 1.0f && pz > -1.0f;
   float shadow = 0.0f;
   for (int x = -1; x <= 1; x++) {
      for (int y = -1; y <= 1; y++) {
         if (inside) {
            const float uu = u + (float)x * ts, vv = v + (float)y * ts;
            const float d = shadow_depth(map, S, uu * fS - 0.5f, vv * fS - 0.5f);
            shadow += (pz - 0.0005f) > d ? 0.3f : 1.0f;
         } else {
            shadow += 1.0f;
         }
      }
   }
   return shadow / 9.0f;
}

}  // namespace uh
