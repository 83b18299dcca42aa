// motion.hip - motion vectors for moving geometry (UH_HYBRID_MOTION; utopian_hip.h "motion vectors"): the cast form's motion kernel and
// the snapshot of the vertex positions behind a motion pass, with their launchers. The rasterised form's kernel is forward.hip's
// k_gbuffer_raster_motion (it needs fragment_at); both call motion_device.h's motion_texel. Arithmetic: DESIGN.md section 2, "Motion
// vectors"; what the kernels read and write per pixel: section 4, "Motion vectors".
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "device_types.h"
#include "kernel_common.h"
#include "motion_device.h"
#include "traversal.h"

namespace uh {

// Between the cast and k_hybrid_gbuffer_resolve: the cast's records are still in the targets (ray origin in the normal target, direction
// in the pbr target, hit record (t, u, v, packet) in the position target). One lane per pixel: three coalesced 16-byte loads, the
// packet's key (one gathered word), the mesh's row, three gathered indices, then - only for a mesh that moved - three gathered corners
// (16-byte rows when deformed, the 12 position bytes of the 80-byte vertices when rigid), and one coalesced 16-byte store. p is the
// resolve's expression: the same words, so a static pixel's xyz has the position texel's bits. The two counts: motion_device.h.
__global__ __launch_bounds__(kMotionBlock) void k_hybrid_motion(SceneDev sc, HybridDev hd, MotionDev md, uint32_t n) {
   MotionCount count;
   for (uint32_t base = blockIdx.x * kMotionBlock; base < n; base += gridDim.x * kMotionBlock) {
      const uint32_t j = base + threadIdx.x;
      float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      bool geo = false;
      if (j < n) {
         const float4 h = hd.pos[j];
         const uint32_t packet = __float_as_uint(h.w);
         if (packet != kEmptyRef) {
            geo = true;
            const float4 ro = hd.nrm[j], rd = hd.pbr[j];
            const V3 p = v3(ro.x, ro.y, ro.z) + h.x * v3(rd.x, rd.y, rd.z);
            const uint32_t key = __float_as_uint(sc.tris[kTriStride16 * (size_t)packet + 2].y);
            const uint32_t mesh = key >> kPrimBits, prim = key & kPrimMask;
            const HybridMesh* m = hd.meshes + mesh;
            const uint32_t* tri = hd.indices + m->index_base + 3 * (size_t)prim;
            out = motion_texel(hd, md, mesh, m->vertex_base, tri[0], tri[1], tri[2], 1.0f - h.y - h.z, h.y, h.z, make_float4(p.x, p.y, p.z, 1.0f));
         }
         md.image[j] = out;
      }
      count.add(geo, out.w);
   }
   count.store(md);
}

// Behind a motion pass: the 12 position bytes of vertex i (80-byte records) to 16-byte row i, one lane per vertex - a strided gather
// (three dwords out of every 80 bytes: the lines are fetched whole) and a coalesced 16-byte store.
__global__ __launch_bounds__(kBlock) void k_motion_snapshot(const UhVertex* __restrict__ src, float4* __restrict__ dst, uint32_t n) {
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
      const float* p = src[i].pos;
      dst[i] = make_float4(p[0], p[1], p[2], 1.0f);
   }
}

void launch_hybrid_motion(const LaunchCfg& c, const SceneDev& sc, const HybridDev& hd, const MotionDev& md) {
   const uint32_t n = hd.W * hd.H;
   k_hybrid_motion<<<dim3(motion_blocks(n, c.num_cus)), kMotionBlock, 0, c.stream>>>(sc, hd, md, n);
}
void launch_motion_snapshot(const LaunchCfg& c, const UhVertex* src, float4* dst, uint32_t n) {
   if (n) k_motion_snapshot<<<stream_grid(c, n), kBlock, 0, c.stream>>>(src, dst, n);
}

}  // namespace uh
