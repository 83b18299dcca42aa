// deform.hip — the kernels behind uh_update_mesh_vertices (scene_build.hip): a mesh whose vertices moved while its index list stayed
// keeps the tree's topology, so a refit serves it once the packets of its triangles hold the new vertices. k_deform_gather writes
// them in LEAF order - packet i's key says which mesh and primitive it is - before refit.hip bakes the corners and recomputes the
// boxes; k_deform_scatter writes the same records in MESH order for the on-device builders (the indexed form of k_iso_scatter),
// k_deform_box reduces the mesh's object-space box, k_deform_check looks at a caller's device buffer before it is taken.
//
// Gather and scatter are one thread per triangle: 12 bytes of indices, then 48 of each vertex's 80 bytes as three 16-byte loads (pos
// at 0, normal at 16, uv at 32), 36 bytes of corners and the 64-byte shade packet as four 16-byte stores. The vertex loads are a
// gather by nature (neighbouring triangles share vertices: they hit in L2); the stores of a wave are contiguous in both orders.
#include <hip/hip_runtime.h>

#include "box_reduce.h"
#include "bvh.h"
#include "device_types.h"

namespace uh {

namespace {

constexpr uint32_t kBlock = 256;
static_assert(sizeof(UhVertex) == 80 && sizeof(ShadePacket) == 64, "the record arithmetic below");

// triangle `prim` of (verts, indices): its nine object-space corners verbatim and its shade packet, the layout of fill_shade_packet
__device__ __forceinline__ void write_triangle(const UhVertex* __restrict__ verts, const uint32_t* __restrict__ indices, uint32_t prim, uint32_t mesh,
                                               float* __restrict__ oc, float4* __restrict__ sp) {
   const uint32_t* ix = indices + 3 * (size_t)prim;
   const float4* v0 = reinterpret_cast<const float4*>(verts + ix[0]);
   const float4* v1 = reinterpret_cast<const float4*>(verts + ix[1]);
   const float4* v2 = reinterpret_cast<const float4*>(verts + ix[2]);
   const float4 p0 = v0[0], n0 = v0[1], t0 = v0[2];
   const float4 p1 = v1[0], n1 = v1[1], t1 = v1[2];
   const float4 p2 = v2[0], n2 = v2[1], t2 = v2[2];
   oc[0] = p0.x, oc[1] = p0.y, oc[2] = p0.z;
   oc[3] = p1.x, oc[4] = p1.y, oc[5] = p1.z;
   oc[6] = p2.x, oc[7] = p2.y, oc[8] = p2.z;
   // n0 n1 n2 (3 each), uv0 uv1 uv2 (2 each), the mesh index
   sp[0] = make_float4(n0.x, n0.y, n0.z, n1.x);
   sp[1] = make_float4(n1.y, n1.z, n2.x, n2.y);
   sp[2] = make_float4(n2.z, t0.x, t0.y, t1.x);
   sp[3] = make_float4(t1.y, t2.x, t2.y, __uint_as_float(mesh));
}

// one thread per triangle packet (leaf order); packets of meshes that did not move leave at once
__global__ __launch_bounds__(kBlock) void k_deform_gather(const DeformMesh* __restrict__ table, uint32_t num_meshes, const float4* __restrict__ tris,
                                                          float* __restrict__ obj_corners, float4* __restrict__ shade, uint32_t count) {
   const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= count) return;
   const uint32_t key = __float_as_uint(tris[kTriStride16 * (size_t)i + 2].y);  // TriPacket: e2z key pad pad
   const uint32_t mesh = key >> kPrimBits;
   if (mesh >= num_meshes) return;
   const DeformMesh m = table[mesh];
   if (!m.moved) return;
   write_triangle(m.verts, m.indices, key & kPrimMask, mesh, obj_corners + 9 * (size_t)i, shade + 4 * (size_t)i);
}

// one thread per triangle of one mesh (mesh order): the on-device build's sources
__global__ __launch_bounds__(kBlock) void k_deform_scatter(const UhVertex* __restrict__ verts, const uint32_t* __restrict__ indices, uint32_t num_tris, uint32_t mesh,
                                                           float* __restrict__ corners, uint32_t* __restrict__ keys, float4* __restrict__ shade) {
   const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
   if (p >= num_tris) return;
   write_triangle(verts, indices, p, mesh, corners + 9 * (size_t)p, shade + 4 * (size_t)p);
   keys[p] = (mesh << kPrimBits) | p;
}

// every vertex of the mesh, referenced by a triangle or not: the values build_on_device's host loop folds
__global__ __launch_bounds__(kBlock) void k_deform_box(const UhVertex* __restrict__ verts, uint32_t num_vertices, uint32_t* __restrict__ box) {
   float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
   for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < num_vertices; i += gridDim.x * kBlock) {
      const float4 p = *reinterpret_cast<const float4*>(verts + i);
      lo[0] = fminf(lo[0], p.x), lo[1] = fminf(lo[1], p.y), lo[2] = fminf(lo[2], p.z);
      hi[0] = fmaxf(hi[0], p.x), hi[1] = fmaxf(hi[1], p.y), hi[2] = fmaxf(hi[2], p.z);
   }
   for (int a = 0; a < 3; a++) {
      const float l = wave_min(lo[a]), h = wave_max(hi[a]);
      if ((threadIdx.x & 63) == 0) {
         if (l != INFINITY) atomicMin(&box[a], ordered(l));
         if (h != -INFINITY) atomicMax(&box[3 + a], ordered(h));
      }
   }
}

// a caller's buffer: scalar loads, since nothing says it is aligned to more than a float
__global__ __launch_bounds__(kBlock) void k_deform_check(const UhVertex* __restrict__ verts, uint32_t num_vertices, uint32_t* __restrict__ flag) {
   const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
   if (i >= num_vertices) return;
   const float* p = verts[i].pos;
   if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) atomicOr(flag, 1u);
}

inline uint32_t blocks_for(uint32_t n) { return (n + kBlock - 1) / kBlock; }

}  // namespace

void launch_deform_gather(hipStream_t stream, const DeformMesh* table, uint32_t num_meshes, const float4* tris, float* obj_corners, float4* shade, uint32_t num_tris) {
   if (num_tris) k_deform_gather<<<blocks_for(num_tris), kBlock, 0, stream>>>(table, num_meshes, tris, obj_corners, shade, num_tris);
}
void launch_deform_scatter(hipStream_t stream, const UhVertex* verts, const uint32_t* indices, uint32_t num_tris, uint32_t mesh, float* corners, uint32_t* keys,
                           float4* shade) {
   if (num_tris) k_deform_scatter<<<blocks_for(num_tris), kBlock, 0, stream>>>(verts, indices, num_tris, mesh, corners, keys, shade);
}
void launch_deform_box(hipStream_t stream, const UhVertex* verts, uint32_t num_vertices, uint32_t* box) {
   if (num_vertices) k_deform_box<<<blocks_for(num_vertices) < 1024u ? blocks_for(num_vertices) : 1024u, kBlock, 0, stream>>>(verts, num_vertices, box);
}
void launch_deform_check(hipStream_t stream, const UhVertex* verts, uint32_t num_vertices, uint32_t* flag) {
   if (num_vertices) k_deform_check<<<blocks_for(num_vertices), kBlock, 0, stream>>>(verts, num_vertices, flag);
}

}  // namespace uh
