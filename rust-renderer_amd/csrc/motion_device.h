// motion_device.h - the motion texel of one G-buffer pixel (UH_HYBRID_MOTION; utopian_hip.h "motion vectors"), shared by the cast form's
// kernel (motion.hip k_hybrid_motion) and the rasterised form's (forward.hip k_gbuffer_raster_motion). The float32 arithmetic of DESIGN.md
// section 2, "Motion vectors", in the order written there (the library is compiled with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"

namespace uh {

// pos: the position texel the G-buffer pass writes for this pixel (w = 1). i0..i2: the triangle's vertices, local to the mesh;
// b0..b2: the barycentrics as the pass formed them. static: pos verbatim; none: pos with w = 0; rigid: the current corners, deformed:
// the previous ones (three 16-byte rows), through the previous object-to-world. A deformed triangle with a vertex outside the
// snapshot's rows has no correspondence.
__device__ __forceinline__ float4 motion_texel(const HybridDev& hd, const MotionDev& md, uint32_t mesh, uint32_t vertex_base, uint32_t i0, uint32_t i1,
                                               uint32_t i2, float b0, float b1, float b2, float4 pos) {
   const MotionMesh* mm = md.meshes + mesh;
   const uint32_t state = mm->state;
   if (state == kMotionStatic) return make_float4(pos.x, pos.y, pos.z, 1.0f);
   V3 q0, q1, q2;
   if (state == kMotionDeformed) {
      const uint32_t count = mm->prev_count;
      if (i0 >= count || i1 >= count || i2 >= count) return make_float4(pos.x, pos.y, pos.z, 0.0f);
      const float4* rows = md.prev_pos + mm->prev_base;
      q0 = xyz(rows[i0]), q1 = xyz(rows[i1]), q2 = xyz(rows[i2]);
   } else if (state == kMotionRigid) {
      const UhVertex* vb = hd.vertices + vertex_base;
      q0 = v3(vb[i0].pos[0], vb[i0].pos[1], vb[i0].pos[2]);
      q1 = v3(vb[i1].pos[0], vb[i1].pos[1], vb[i1].pos[2]);
      q2 = v3(vb[i2].pos[0], vb[i2].pos[1], vb[i2].pos[2]);
   } else {
      return make_float4(pos.x, pos.y, pos.z, 0.0f);
   }
   const V3 o = (q0 * b0 + q1 * b1) + q2 * b2;
   const float* m = mm->prev_o2w;
   return make_float4(((m[0] * o.x + m[1] * o.y) + m[2] * o.z) + m[3] * 1.0f, ((m[4] * o.x + m[5] * o.y) + m[6] * o.z) + m[7] * 1.0f,
                      ((m[8] * o.x + m[9] * o.y) + m[10] * o.z) + m[11] * 1.0f, 1.0f);
}

// The pass's two counts without an atomic. Both kernels run kMotionBlock lanes per block over a grid of at most motion_blocks(...) blocks,
// block-stride over the pixels (every lane of a wave runs the same number of rounds); a wave adds its ballots up in a scalar, and at the
// end a block stores the sum of its four waves to its own pair of words: counters[2 b] with, counters[2 b + 1] without a correspondence.
// The host adds the pairs up when the stats are asked for. (One atomic per wave on one word - 32,400 of them at 1080p - cost 0.37 ms,
// measured: more than the G-buffer pass itself.)
constexpr int kMotionBlock = 256;
static inline uint32_t motion_blocks(uint32_t pixels, uint32_t num_cus) {
   const uint32_t blocks = (pixels + kMotionBlock - 1) / kMotionBlock, cap = num_cus * 8;
   return blocks < cap ? (blocks ? blocks : 1) : cap;
}
struct MotionCount {
   uint32_t with = 0, without = 0;  // wave-uniform
   __device__ __forceinline__ void add(bool geometry, float w) {
      with += (uint32_t)__popcll(__ballot(geometry && w != 0.0f));
      without += (uint32_t)__popcll(__ballot(geometry && w == 0.0f));
   }
   __device__ __forceinline__ void store(const MotionDev& md) const {
      __shared__ uint32_t s_count[kMotionBlock / 64][2];
      if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6][0] = with, s_count[threadIdx.x >> 6][1] = without;
      __syncthreads();
      if (threadIdx.x < 2) {
         uint32_t sum = 0;
         for (int k = 0; k < kMotionBlock / 64; k++) sum += s_count[k][threadIdx.x];
         md.counters[2 * blockIdx.x + threadIdx.x] = sum;
      }
   }
};

}  // namespace uh
