// box_reduce.h - a box of floats reduced over a grid with integer atomics: what k_iso_scatter (iso_update.hip) and k_deform_box
// (deform.hip) share. Minima and maxima are exact whatever the order, so the figures are those of a host loop over the same values.
#pragma once
#include <hip/hip_runtime.h>

// floats as unsigned integers of the same order (for atomicMin / atomicMax)
__device__ __forceinline__ uint32_t ordered(float f) {
   const uint32_t u = __float_as_uint(f);
   return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float wave_min(float v) {
   for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s));
   return v;
}
__device__ __forceinline__ float wave_max(float v) {
   for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s));
   return v;
}
