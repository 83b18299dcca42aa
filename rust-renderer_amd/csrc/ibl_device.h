// ibl_device.h — device arithmetic of the IBL maps (ibl.rs and its shaders) shared by their build (ibl.hip) and their consumers
// (hybrid_kernels.hip): cube addressing with seamless edges, the LINEAR / trilinear filters, the brdf.glsl helpers and imageBasedLighting.
// Every line is pinned in DESIGN.md section 2 "Environment and IBL maps"; tests/ibl_reference.py restates it in numpy.
#pragma once
#include <hip/hip_fp16.h>

#include "device_math.h"
#include "device_types.h"

namespace uh {
namespace ibl {

constexpr float kPi = 3.14159265359f;  // brdf.glsl:1 and the shaders' #define PI: the same float

// the face table of the Vulkan cube-map face selection: major axis, and the axes (with signs) of sc and tc. Faces in layer order
// +X, -X, +Y, -Y, +Z, -Z; axes 0 = x, 1 = y, 2 = z.
struct FaceAxes {
   int ma, sc, tc;
   int ma_sign, sc_sign, tc_sign;
};
__host__ __device__ inline FaceAxes face_axes(int f) {
   switch (f) {
   case 0: return {0, 2, 1, +1, -1, -1};   // +X: sc = -z, tc = -y
   case 1: return {0, 2, 1, -1, +1, -1};   // -X: sc = +z, tc = -y
   case 2: return {1, 0, 2, +1, +1, +1};   // +Y: sc = +x, tc = +z
   case 3: return {1, 0, 2, -1, +1, -1};   // -Y: sc = +x, tc = -z
   case 4: return {2, 0, 1, +1, +1, -1};   // +Z: sc = +x, tc = -y
   default: return {2, 0, 1, -1, -1, -1};  // -Z: sc = -x, tc = -y
   }
}

// face and (s, t) of direction d. Ties on the major axis go to x, then y; a zero major component counts as positive.
// s = (sc * (1 / |ma|)) * 0.5 + 0.5: one correctly rounded reciprocal, then products.
__device__ __forceinline__ void cube_coords(V3 d, int& face, float& s, float& t) {
   const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
   float sc, tc, ma;
   if (ax >= ay && ax >= az) {
      const bool pos = !(d.x < 0.0f);
      face = pos ? 0 : 1;
      ma = ax;
      sc = pos ? -d.z : d.z;
      tc = -d.y;
   } else if (ay >= az) {
      const bool pos = !(d.y < 0.0f);
      face = pos ? 2 : 3;
      ma = ay;
      sc = d.x;
      tc = pos ? d.z : -d.z;
   } else {
      const bool pos = !(d.z < 0.0f);
      face = pos ? 4 : 5;
      ma = az;
      sc = pos ? d.x : -d.x;
      tc = -d.y;
   }
   const float inv = 1.0f / ma;
   s = (sc * inv) * 0.5f + 0.5f;
   t = (tc * inv) * 0.5f + 0.5f;
}

// texel (i, j) of face f of a level of size S, i and j in [-1, S]: inside the face, or across one edge folded onto the neighbouring
// face's texel that touches the same edge at the same place along it. Integer coordinates: a = 2i + 1 - S is the texel centre in
// units of half a texel from the face centre; the face plane is at S.
__device__ __forceinline__ uint32_t folded_texel(int f, int i, int j, int S) {
   const FaceAxes A = face_axes(f);
   int P[3];
   const int a = 2 * i + 1 - S, b = 2 * j + 1 - S;
   P[A.ma] = A.ma_sign * S;
   P[A.sc] = A.sc_sign * a;
   P[A.tc] = A.tc_sign * b;
   int axis = A.ma;
   if (a < -S || a > S) {  // across the sc edge: onto the face whose major axis is sc's
      P[A.ma] = A.ma_sign * (S - 1);
      P[A.sc] = A.sc_sign * (a < 0 ? -S : S);
      axis = A.sc;
   } else if (b < -S || b > S) {
      P[A.ma] = A.ma_sign * (S - 1);
      P[A.tc] = A.tc_sign * (b < 0 ? -S : S);
      axis = A.tc;
   }
   const int nf = 2 * axis + (P[axis] < 0 ? 1 : 0);
   const FaceAxes B = face_axes(nf);
   const int na = B.sc_sign * P[B.sc], nb = B.tc_sign * P[B.tc];
   const int ni = (na + S - 1) / 2, nj = (nb + S - 1) / 2;
   return (uint32_t)nf * (uint32_t)(S * S) + (uint32_t)(nj * S + ni);
}

// one texel of level `lvl` (face-major, row-major) at (i, j) in [-1, S]^2; a corner outside both ranges is the mean of the three texels
// that meet there: (own corner + across i + across j) * (1 / 3)
__device__ __forceinline__ V3 edge_texel(const float4* __restrict__ lvl, int f, int i, int j, int S) {
   const bool oi = i < 0 || i >= S, oj = j < 0 || j >= S;
   if (oi && oj) {
      const int ci = i < 0 ? 0 : S - 1, cj = j < 0 ? 0 : S - 1;
      const V3 own = xyz(lvl[(uint32_t)f * (uint32_t)(S * S) + (uint32_t)(cj * S + ci)]);
      const V3 across_i = xyz(lvl[folded_texel(f, i, cj, S)]);
      const V3 across_j = xyz(lvl[folded_texel(f, ci, j, S)]);
      return ((own + across_i) + across_j) * (1.0f / 3.0f);
   }
   return xyz(lvl[folded_texel(f, i, j, S)]);
}

// texture(cube, d) at one level of size S through LINEAR, seamless: x = s S - 0.5, y = t S - 0.5, weights x - floor(x), the filter of
// sample_texture. A direction with no face (zero, NaN) reads 0.
__device__ __forceinline__ V3 cube_bilinear(const float4* __restrict__ lvl, int S, V3 d) {
   int f;
   float s, t;
   cube_coords(d, f, s, t);
   const float x = s * (float)S - 0.5f, y = t * (float)S - 0.5f;
   if (!(x >= -1.0f && x < (float)S && y >= -1.0f && y < (float)S)) return v3(0.0f, 0.0f, 0.0f);  // [-0.5, S - 0.5] up to rounding
   const float fx = floorf(x), fy = floorf(y);
   const float ax = x - fx, ay = y - fy;
   const int i0 = (int)fx, j0 = (int)fy;
   V3 t00, t10, t01, t11;
   if (i0 >= 0 && j0 >= 0 && i0 + 1 < S && j0 + 1 < S) {
      const float4* p = lvl + (uint32_t)f * (uint32_t)(S * S) + (uint32_t)(j0 * S + i0);
      t00 = xyz(p[0]);
      t10 = xyz(p[1]);
      t01 = xyz(p[S]);
      t11 = xyz(p[S + 1]);
   } else {
      t00 = edge_texel(lvl, f, i0, j0, S);
      t10 = edge_texel(lvl, f, i0 + 1, j0, S);
      t01 = edge_texel(lvl, f, i0, j0 + 1, S);
      t11 = edge_texel(lvl, f, i0 + 1, j0 + 1, S);
   }
   const V3 a = t00 * (1.0f - ax) + t10 * ax;
   const V3 b = t01 * (1.0f - ax) + t11 * ax;
   return a * (1.0f - ay) + b * ay;
}

// textureLod(cube, d, lod) with mipmapMode LINEAR: lod clamped to [0, kEnvMips - 1], levels floor(lod) and min(floor(lod) + 1, last),
// c0 (1 - f) + c1 f with f = lod - floor(lod) (c1 not read when f = 0: c0 * 1 + c0 * 0 = c0)
__device__ __forceinline__ V3 cube_lod(const float4* __restrict__ cube, V3 d, float lod) {
   lod = fminf(fmaxf(lod, 0.0f), (float)(kEnvMips - 1));
   const float fl = floorf(lod);
   const uint32_t m0 = (uint32_t)fl, m1 = m0 + 1 < kEnvMips ? m0 + 1 : m0;
   const float fr = lod - fl;
   const V3 c0 = cube_bilinear(cube + env_mip_offset(m0), (int)(kEnvSize >> m0), d);
   const V3 c1 = fr == 0.0f ? c0 : cube_bilinear(cube + env_mip_offset(m1), (int)(kEnvSize >> m1), d);
   return c0 * (1.0f - fr) + c1 * fr;
}

// the BRDF LUT through LINEAR + MIRRORED_REPEAT (texture.rs's sampler): (R, G) at uv
__device__ __forceinline__ float2 lut_bilinear(const uint32_t* __restrict__ lut, float u, float v) {
   const float x = u * (float)kLutSize - 0.5f, y = v * (float)kLutSize - 0.5f;
   if (!(fabsf(x) < 1e9f) || !(fabsf(y) < 1e9f)) return make_float2(0.0f, 0.0f);
   const float fx = floorf(x), fy = floorf(y);
   const float ax = x - fx, ay = y - fy;
   const int n = (int)kLutSize;
   const int x0 = mirror_index((int)fx, n), x1 = mirror_index((int)fx + 1, n);
   const int y0 = mirror_index((int)fy, n), y1 = mirror_index((int)fy + 1, n);
   auto rg = [&](int xx, int yy) {
      const uint32_t w = lut[(uint32_t)yy * kLutSize + (uint32_t)xx];
      return make_float2(__half2float(__ushort_as_half((unsigned short)(w & 0xffffu))), __half2float(__ushort_as_half((unsigned short)(w >> 16))));
   };
   const float2 t00 = rg(x0, y0), t10 = rg(x1, y0), t01 = rg(x0, y1), t11 = rg(x1, y1);
   const float ar = t00.x * (1.0f - ax) + t10.x * ax, ag = t00.y * (1.0f - ax) + t10.y * ax;
   const float br = t01.x * (1.0f - ax) + t11.x * ax, bg = t01.y * (1.0f - ax) + t11.y * ax;
   return make_float2(ar * (1.0f - ay) + br * ay, ag * (1.0f - ay) + bg * ay);
}

// ---- brdf.glsl ------------------------------------------------------------------------------------------------------------------
// random(co): mod(x, y) = x - y * floor(x / y), device sinf, fract(x) = x - floor(x)
__device__ __forceinline__ float random2(float cx, float cy) {
   const float dt = cx * 12.9898f + cy * 78.233f;
   const float sn = dt - 3.14f * floorf(dt / 3.14f);
   const float r = sinf(sn) * 43758.5453f;
   return r - floorf(r);
}
__device__ __forceinline__ float2 hammersley2d(uint32_t i, uint32_t N) {
   uint32_t bits = (i << 16u) | (i >> 16u);
   bits = ((bits & 0x55555555u) << 1u) | ((bits & 0xAAAAAAAAu) >> 1u);
   bits = ((bits & 0x33333333u) << 2u) | ((bits & 0xCCCCCCCCu) >> 2u);
   bits = ((bits & 0x0F0F0F0Fu) << 4u) | ((bits & 0xF0F0F0F0u) >> 4u);
   bits = ((bits & 0x00FF00FFu) << 8u) | ((bits & 0xFF00FF00u) >> 8u);
   const float rdi = (float)bits * 2.3283064365386963e-10f;
   return make_float2((float)i / (float)N, rdi);
}
// importanceSample_GGX with the normal's random(normal.xz) passed in (it does not depend on the sample)
__device__ __forceinline__ V3 importance_sample_ggx(float2 Xi, float roughness, V3 N, float rnd) {
   const float alpha = roughness * roughness;
   const float phi = (2.0f * kPi) * Xi.x + rnd * 0.1f;
   const float cos_t = sqrtf((1.0f - Xi.y) / (1.0f + (alpha * alpha - 1.0f) * Xi.y));
   const float sin_t = sqrtf(1.0f - cos_t * cos_t);
   const V3 H = v3(sin_t * cosf(phi), sin_t * sinf(phi), cos_t);
   const V3 up = fabsf(N.z) < 0.999f ? v3(0.0f, 0.0f, 1.0f) : v3(1.0f, 0.0f, 0.0f);
   const V3 tx = normalize3(v3(up.y * N.z - up.z * N.y, up.z * N.x - up.x * N.z, up.x * N.y - up.y * N.x));
   const V3 ty = normalize3(v3(N.y * tx.z - N.z * tx.y, N.z * tx.x - N.x * tx.z, N.x * tx.y - N.y * tx.x));
   return normalize3((tx * H.x + ty * H.y) + N * H.z);
}

// pbr_lighting.glsl:81-108 imageBasedLighting: V = normalize(eye - P), R = -reflect(V, N), the LUT at (max(N.V, 0), 1 - roughness)
__device__ __forceinline__ V3 image_based_lighting(const IblMaps& m, V3 P, V3 base, V3 N, float metallic, float roughness, float occlusion, V3 eye) {
   const V3 V = normalize3(eye - P);
   const V3 R = vneg(V - N * (2.0f * dot3(N, V)));
   const float om = 1.0f - metallic;
   const V3 F0 = v3(0.04f, 0.04f, 0.04f) * om + base * metallic;                    // mix(0.04, base, metallic)
   const float NdotV = fmaxf(dot3(N, V), 0.0f);
   const float x = fminf(fmaxf(1.0f - NdotV, 0.0f), 1.0f);
   const float p5 = ((x * x) * (x * x)) * x;
   const float omr = 1.0f - roughness;
   const V3 Fr = F0 + (v3(fmaxf(omr, F0.x), fmaxf(omr, F0.y), fmaxf(omr, F0.z)) - F0) * p5;  // fresnelSchlickRoughness
   const V3 kD = (v3(1.0f, 1.0f, 1.0f) - Fr) * om;
   const V3 irradiance = cube_bilinear(m.irr, (int)kEnvSize, N);
   const V3 diffuse = irradiance * base;
   const V3 pre = cube_lod(m.spec, R, roughness * 7.0f);
   const float2 brdf = lut_bilinear(m.lut, NdotV, 1.0f - roughness);
   const V3 specular = pre * (Fr * brdf.x + v3(brdf.y, brdf.y, brdf.y));
   return (kD * diffuse + specular) * occlusion;
}

}  // namespace ibl
}  // namespace uh
