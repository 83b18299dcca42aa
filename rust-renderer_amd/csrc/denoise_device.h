// denoise_device.h - what the stages of the denoiser (denoise.hip) share: the luminance, the view depth, the guide weights of the
// variance estimate and the a-trous filter. Every function is the float32 arithmetic of DESIGN.md section 2, "Denoiser: the arithmetic
// contract of uh_denoise", in the order written there (the library is compiled with -ffp-contract=off); expf is the only transcendental.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"

namespace uh {

// Rec. 601 luma of a colour
__device__ __forceinline__ float dn_luminance(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

// A sample the temporal filters take in: every channel finite and at most 2^48 in magnitude (a NaN fails the compare). The bound is what
// keeps every later product finite - the squared luminance of a colour demodulated by 0.01, 49 taps of 4 x its second moment, nine
// squares of TAA's box - and what keeps r - prev finite for values of opposite sign ("Non-finite input")
constexpr float kTemporalMaxSample = 281474976710656.0f;
__device__ __forceinline__ bool temporal_sample_ok(float r, float g, float b) {
   return fabsf(r) <= kTemporalMaxSample && fabsf(g) <= kTemporalMaxSample && fabsf(b) <= kTemporalMaxSample;
}

// z of view * (P, 1): the third row of the column-major view matrix
__device__ __forceinline__ float dn_view_z(const float* m, V3 p) { return ((m[2] * p.x + m[6] * p.y) + m[10] * p.z) + m[14] * 1.0f; }

// max(dot(n_p, n_q), 0)^128 as seven squarings
__device__ __forceinline__ float dn_normal_weight(V3 np, V3 nq) {
   float t = fmaxf(dot3(np, nq), 0.0f);
   for (int k = 0; k < 7; k++) t = t * t;
   return t;
}

// |dot(P_q - P_p, n_p)| / plane_den, plane_den = sigma_plane * |z_p| + 1e-6
__device__ __forceinline__ float dn_plane_term(V3 pp, V3 np, V3 pq, float plane_den) { return fabsf(dot3(pq - pp, np)) / plane_den; }

// the a-trous kernel's row (1/16, 1/4, 3/8, 1/4, 1/16) at offset d = -2 .. 2
__device__ __forceinline__ float dn_kernel(int d) {
   const int a = d < 0 ? -d : d;
   return a == 0 ? 0.375f : (a == 1 ? 0.25f : 0.0625f);
}

// pixel (x, y) is in the image and was written as geometry
__device__ __forceinline__ bool dn_geometry(const float4* __restrict__ pos, uint32_t W, uint32_t H, int x, int y, float4& out) {
   if (x < 0 || y < 0 || x >= (int)W || y >= (int)H) return false;
   out = pos[(size_t)y * W + x];
   return out.w != 0.0f;
}

}  // namespace uh
