// ibl.hip — setup_cubemap_pass (utopian/src/renderers/ibl.rs) on gfx950: the environment cube (cubemap.frag), the irradiance cube
// (irradiance_filter.frag), the prefiltered specular cube (specular_filter.frag) and the BRDF LUT (brdf_lut.frag), each a compute
// kernel over the texels the reference's fragment passes shade. Arithmetic: DESIGN.md section 2 "Environment and IBL maps".
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "device_math.h"
#include "device_types.h"
#include "ibl_device.h"

namespace uh {

namespace {
constexpr int kIblBlock = 256;

inline dim3 grid_for(const LaunchCfg& c, uint32_t n) {
   const uint32_t blocks = (n + kIblBlock - 1) / kIblBlock, cap = c.num_cus * 8;
   return dim3(blocks < cap ? (blocks ? blocks : 1) : cap);
}

// world_dir_from_uv(in_uv, view_matrices[f], projection) at texel (i, j) of a face of size S: in_uv = ((i + 0.5) / S, 1 - (j + 0.5) / S)
// (render_utils::viewport flips Y), ndc = in_uv * 2 - 1. inverse(perspective_rh(90 deg, 1, 0.01, 20000)) * (x, y, -1, 1) with w set to 0
// is (x, y, -1) (glam's h = cos / sin of 45 deg is 1.0f), and inverse(look_at_rh(0, f, up)) is the transpose of a signed permutation:
// world = x s + y u + f, exact, before the normalize.
__device__ __forceinline__ V3 texel_dir(uint32_t f, uint32_t i, uint32_t j, uint32_t S) {
   const float fs = (float)S;
   const float u = ((float)i + 0.5f) / fs, v = 1.0f - ((float)j + 0.5f) / fs;
   const float x = u * 2.0f - 1.0f, y = v * 2.0f - 1.0f;
   V3 w;
   switch (f) {
   case 0: w = v3(1.0f, -y, -x); break;   // look_at_rh(0, +X, -Y)
   case 1: w = v3(-1.0f, -y, x); break;   // (0, -X, -Y)
   case 2: w = v3(x, -1.0f, -y); break;   // (0, -Y, -Z)
   case 3: w = v3(x, 1.0f, y); break;     // (0, +Y, +Z)
   case 4: w = v3(x, -y, 1.0f); break;    // (0, +Z, -Y)
   default: w = v3(-x, -y, -1.0f); break; // (0, -Z, -Y)
   }
   return normalize3(w);
}

// linear texel index over all mips of a cube -> (mip, face, i, j)
__device__ __forceinline__ void cube_texel(uint32_t t, uint32_t& m, uint32_t& f, uint32_t& i, uint32_t& j) {
   m = 0;
   uint32_t S = kEnvSize;
   while (m + 1 < kEnvMips && t >= 6u * S * S) {
      t -= 6u * S * S;
      m++;
      S >>= 1;
   }
   f = t / (S * S);
   t -= f * S * S;
   j = t / S;
   i = t - j * S;
}
}  // namespace

// cubemap.frag: IntegrateScattering(rayStart, worldDir, 999999999, view.sun_dir) at every texel of every mip, each at its own size
__global__ __launch_bounds__(kIblBlock) void k_env_cube(EnvDev e, uint32_t n) {
   const V3 eye = v3(e.eye[0], e.eye[1], e.eye[2]), sun = v3(e.sun[0], e.sun[1], e.sun[2]);
   for (uint32_t t = blockIdx.x * kIblBlock + threadIdx.x; t < n; t += gridDim.x * kIblBlock) {
      uint32_t m, f, i, j;
      cube_texel(t, m, f, i, j);
      const V3 d = texel_dir(f, i, j, kEnvSize >> m);
      const V3 c = sky::integrate_scattering(eye, d, 999999999.0f, sun);
      e.env[t] = make_float4(c.x, c.y, c.z, 1.0f);
   }
}

// irradiance_filter.frag: one lane per texel of the 6 x 512^2 face set, the taps in the shader's order (phi outer, theta inner), so the
// float sum is the shader's. The tap table is read at a wave-uniform index (scalar loads); what is left per tap is the basis transform,
// the face select and four 16-byte texel loads from environment mip 0 (25 MB: L2 / Infinity Cache resident).
__global__ __launch_bounds__(kIblBlock) void k_env_irradiance(EnvDev e) {
   const uint32_t n = 6u * kEnvSize * kEnvSize, t = blockIdx.x * kIblBlock + threadIdx.x;
   if (t >= n) return;
   const uint32_t f = t / (kEnvSize * kEnvSize), r = t - f * kEnvSize * kEnvSize, j = r / kEnvSize, i = r - j * kEnvSize;
   const V3 N = texel_dir(f, i, j, kEnvSize);
   V3 up = v3(0.0f, 1.0f, 0.0f);
   const V3 right = normalize3(v3(up.y * N.z - up.z * N.y, up.z * N.x - up.x * N.z, up.x * N.y - up.y * N.x));  // frag:31
   up = normalize3(v3(N.y * right.z - N.z * right.y, N.z * right.x - N.x * right.z, N.x * right.y - N.y * right.x));  // frag:32
   const float4* __restrict__ taps = e.taps;
   const float4* __restrict__ env0 = e.env;
   V3 acc = v3(0.0f, 0.0f, 0.0f);
   for (uint32_t k = 0; k < kIrrPhi * kIrrTheta; k++) {
      const float4 tp = taps[k];
      const V3 sv = (right * tp.x + up * tp.y) + N * tp.z;                                  // frag:45
      acc = acc + (ibl::cube_bilinear(env0, (int)kEnvSize, sv) * tp.z) * tp.w;             // frag:47
   }
   const float inv_n = 1.0f / (float)(kIrrPhi * kIrrTheta);
   const V3 irr = (ibl::kPi * acc) * inv_n;                                                 // frag:51
   e.irr[t] = make_float4(irr.x, irr.y, irr.z, 1.0f);
}

// specular_filter.frag: prefilterEnvMap(N, mip / 7) at every texel of every mip of a 512^2 cube (envMapDim = 512)
__global__ __launch_bounds__(kIblBlock) void k_env_specular(EnvDev e, uint32_t n) {
   const float dim = (float)kEnvSize;
   const float omega_p = (4.0f * ibl::kPi) / ((6.0f * dim) * dim);
   for (uint32_t t = blockIdx.x * kIblBlock + threadIdx.x; t < n; t += gridDim.x * kIblBlock) {
      uint32_t m, f, i, j;
      cube_texel(t, m, f, i, j);
      const float rough = (float)m / (float)(kEnvMips - 1);
      const V3 N = texel_dir(f, i, j, kEnvSize >> m), V = N;
      const float rnd = ibl::random2(N.x, N.z);
      const float alpha = rough * rough, alpha2 = alpha * alpha;
      V3 color = v3(0.0f, 0.0f, 0.0f);
      float total = 0.0f;
      for (uint32_t s = 0; s < 32; s++) {
         const V3 H = ibl::importance_sample_ggx(ibl::hammersley2d(s, 32), rough, N, rnd);
         const V3 L = H * (2.0f * dot3(V, H)) - V;
         const float nl = fminf(fmaxf(dot3(N, L), 0.0f), 1.0f);
         if (nl > 0.0f) {
            const float nh = fminf(fmaxf(dot3(N, H), 0.0f), 1.0f), vh = fminf(fmaxf(dot3(V, H), 0.0f), 1.0f);
            const float den = (nh * nh) * (alpha2 - 1.0f) + 1.0f;
            const float D = alpha2 / ((ibl::kPi * den) * den);
            const float pdf = (D * nh) / (4.0f * vh) + 0.0001f;
            const float omega_s = 1.0f / (32.0f * pdf);
            const float lod = rough == 0.0f ? 0.0f : fmaxf(0.5f * log2f(omega_s / omega_p) + 1.0f, 0.0f);
            color = color + ibl::cube_lod(e.env, L, lod) * nl;
            total = total + nl;
         }
      }
      e.spec[t] = make_float4(color.x / total, color.y / total, color.z / total, 1.0f);
   }
}

// brdf_lut.frag: texel (x, y) integrates at NoV = in_uv.x = (x + 0.5) / 512, roughness = in_uv.y = 1 - (y + 0.5) / 512 (the flipped
// viewport). H depends on the row only: a block takes half a row and makes its 1024 half vectors in LDS first.
__global__ __launch_bounds__(kIblBlock) void k_env_brdf_lut(EnvDev e) {
   __shared__ float s_h[1024][3];
   const uint32_t y = blockIdx.x >> 1, x = (blockIdx.x & 1) * kIblBlock + threadIdx.x;
   const float rough = 1.0f - ((float)y + 0.5f) / (float)kLutSize;
   const V3 N = v3(0.0f, 0.0f, 1.0f);
   const float rnd = ibl::random2(N.x, N.z);
   for (uint32_t k = threadIdx.x; k < 1024; k += kIblBlock) {
      const V3 H = ibl::importance_sample_ggx(ibl::hammersley2d(k, 1024), rough, N, rnd);
      s_h[k][0] = H.x;
      s_h[k][1] = H.y;
      s_h[k][2] = H.z;
   }
   __syncthreads();
   const float NoV = ((float)x + 0.5f) / (float)kLutSize;
   const V3 V = v3(sqrtf(1.0f - NoV * NoV), 0.0f, NoV);
   const float a2 = powf(rough, 4.0f), oma2 = 1.0f - a2;
   const float ggxl_v = (NoV * NoV) * oma2 + a2;
   float A = 0.0f, B = 0.0f;
   for (uint32_t k = 0; k < 1024; k++) {
      const V3 H = v3(s_h[k][0], s_h[k][1], s_h[k][2]);
      const float vdh = dot3(V, H);
      const V3 L = H * (2.0f * vdh) - V;
      const float NoL = fminf(fmaxf(dot3(N, L), 0.0f), 1.0f);
      const float NoH = fminf(fmaxf(dot3(N, H), 0.0f), 1.0f);
      const float VoH = fminf(fmaxf(vdh, 0.0f), 1.0f);
      if (NoL > 0.0f) {
         const float ggxv = NoL * sqrtf(ggxl_v);
         const float ggxl = NoV * sqrtf((NoL * NoL) * oma2 + a2);
         const float vis = 0.5f / (ggxv + ggxl);
         const float v_pdf = ((vis * VoH) * NoL) / NoH;
         const float fc = powf(1.0f - VoH, 5.0f);
         A = A + (1.0f - fc) * v_pdf;
         B = B + fc * v_pdf;
      }
   }
   const float r = (4.0f * A) / 1024.0f, g = (4.0f * B) / 1024.0f;
   e.lut[y * kLutSize + x] = (uint32_t)__half_as_ushort(__float2half_rn(r)) | ((uint32_t)__half_as_ushort(__float2half_rn(g)) << 16);
}

void launch_env_cube(const LaunchCfg& c, const EnvDev& e) {
   const uint32_t n = env_mip_offset(kEnvMips);
   k_env_cube<<<grid_for(c, n), kIblBlock, 0, c.stream>>>(e, n);
}
void launch_env_irradiance(const LaunchCfg& c, const EnvDev& e) {
   k_env_irradiance<<<dim3(6u * kEnvSize * kEnvSize / kIblBlock), kIblBlock, 0, c.stream>>>(e);
}
void launch_env_specular(const LaunchCfg& c, const EnvDev& e) {
   const uint32_t n = env_mip_offset(kEnvMips);
   k_env_specular<<<grid_for(c, n), kIblBlock, 0, c.stream>>>(e, n);
}
void launch_env_brdf_lut(const LaunchCfg& c, const EnvDev& e) {
   static_assert(kLutSize == 2 * kIblBlock, "a block takes half a row");
   k_env_brdf_lut<<<dim3(2 * kLutSize), kIblBlock, 0, c.stream>>>(e);
}

}  // namespace uh
