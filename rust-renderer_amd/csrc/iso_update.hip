// iso_update.hip — the kernels behind uh_update_isosurface_mesh (context.hip) that feed the consumers of a device-resident
// mesh from its device vertices: the on-device build's per-triangle sources (object-space corners, key, shade packet: the
// arithmetic of build_on_device's host loop), the mesh's object-space box, and the raster tables' iota index list.
//
// k_iso_scatter is a streaming kernel: 240 bytes in and 36 + 4 + 64 bytes out per triangle, no reuse. A tile of 128 triangles
// (30,720 bytes of vertices) is read into LDS with 16-byte loads, consecutive lanes on consecutive addresses, and the three
// outputs leave the same way: output element e of the tile by thread e % 128, so that a wave writes whole lines whatever the
// 36- and 240-byte record sizes are. A mesh has one index list (iota), so triangle p's vertices are 3 p .. 3 p + 2.
#include <hip/hip_runtime.h>

#include "box_reduce.h"
#include "bvh.h"
#include "context_internal.h"

namespace {

constexpr uint32_t kTile = 128;                   // triangles per tile = threads per block
constexpr uint32_t kVertexFloats = sizeof(UhVertex) / 4;  // 20
constexpr uint32_t kTileQuads = kTile * 3 * sizeof(UhVertex) / 16;  // 1,920 16-byte loads per tile
static_assert(sizeof(UhVertex) == 80 && sizeof(uh::ShadePacket) == 64, "k_iso_scatter's record arithmetic");

__global__ __launch_bounds__(kTile) void k_iso_scatter(const float4* __restrict__ verts, uint32_t num_tris, uint32_t mesh, float* __restrict__ corners,
                                                       uint32_t* __restrict__ keys, float4* __restrict__ shade, uint32_t* __restrict__ box) {
   __shared__ float4 s_quads[kTileQuads];
   __shared__ float s_box[2][6];
   const float* s_f = reinterpret_cast<const float*>(s_quads);
   float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
   const uint32_t tiles = (num_tris + kTile - 1) / kTile;
   for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
      const uint32_t t0 = tile * kTile, n = min(kTile, num_tris - t0);
      const uint32_t quads = n * 15;  // 3 vertices of five 16-byte quads
      const float4* src = verts + (size_t)t0 * 15;
      __syncthreads();  // the last tile's readers are done
      for (uint32_t q = threadIdx.x; q < quads; q += kTile) s_quads[q] = src[q];
      __syncthreads();
      // corners: 9 floats per triangle, pos.xyz of vertices 0, 1, 2
      float* oc = corners + 9 * (size_t)t0;
      for (uint32_t e = threadIdx.x; e < 9 * n; e += kTile) {
         const uint32_t t = e / 9, w = e - 9 * t;
         oc[e] = s_f[(3 * t + w / 3) * kVertexFloats + w % 3];
      }
      // shade packets: n0 n1 n2 (3 each), uv0 uv1 uv2 (2 each), the mesh index
      // as 16-byte stores, four per packet (the array is float4 and a mesh's range starts on a packet)
      float4* os = shade + 4 * (size_t)t0;
      for (uint32_t e = threadIdx.x; e < 4 * n; e += kTile) {
         const float* v = s_f + 3 * (e >> 2) * kVertexFloats;  // the triangle's three vertices: normal at +4, uv at +8
         const float *v0 = v, *v1 = v + kVertexFloats, *v2 = v + 2 * kVertexFloats;
         float4 q;
         switch (e & 3) {
            case 0: q = make_float4(v0[4], v0[5], v0[6], v1[4]); break;
            case 1: q = make_float4(v1[5], v1[6], v2[4], v2[5]); break;
            case 2: q = make_float4(v2[6], v0[8], v0[9], v1[8]); break;
            default: q = make_float4(v1[9], v2[8], v2[9], __uint_as_float(mesh)); break;
         }
         os[e] = q;
      }
      if (threadIdx.x < n) {
         keys[t0 + threadIdx.x] = (mesh << uh::kPrimBits) | (t0 + threadIdx.x);
         for (uint32_t k = 0; k < 3; k++)
            for (uint32_t a = 0; a < 3; a++) {
               const float p = s_f[(3 * threadIdx.x + k) * kVertexFloats + a];
               lo[a] = fminf(lo[a], p);
               hi[a] = fmaxf(hi[a], p);
            }
      }
   }
   // the mesh's object-space box: min and max are exact whatever the order, so the figures are the host loop's
   const uint32_t wave = threadIdx.x / 64;
   for (int a = 0; a < 3; a++) {
      const float l = wave_min(lo[a]), h = wave_max(hi[a]);
      if ((threadIdx.x & 63) == 0) {
         s_box[wave][a] = l;
         s_box[wave][3 + a] = h;
      }
   }
   __syncthreads();
   if (threadIdx.x < 3) {
      const float l = fminf(s_box[0][threadIdx.x], s_box[1][threadIdx.x]);
      if (l != INFINITY) atomicMin(&box[threadIdx.x], ordered(l));
   } else if (threadIdx.x < 6) {
      const float h = fmaxf(s_box[0][threadIdx.x], s_box[1][threadIdx.x]);
      if (h != -INFINITY) atomicMax(&box[threadIdx.x], ordered(h));
   }
}

__global__ __launch_bounds__(256) void k_iota(uint32_t* __restrict__ out, uint32_t n) {
   const uint32_t i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) out[i] = i;
}
__global__ __launch_bounds__(256) void k_fill_u32(uint32_t* __restrict__ out, uint32_t n, uint32_t value) {
   const uint32_t i = blockIdx.x * 256 + threadIdx.x;
   if (i < n) out[i] = value;
}

}  // namespace

void uhi_iso_scatter(void* stream, const UhVertex* verts, uint32_t num_tris, uint32_t mesh, float* corners, uint32_t* keys, float4* shade, uint32_t* box) {
   if (!num_tris) return;
   const uint32_t tiles = (num_tris + kTile - 1) / kTile;
   k_iso_scatter<<<tiles < 2048u ? tiles : 2048u, kTile, 0, (hipStream_t)stream>>>(reinterpret_cast<const float4*>(verts), num_tris, mesh, corners, keys, shade, box);
}
void uhi_iota(void* stream, uint32_t* out, uint32_t n) {
   if (n) k_iota<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(out, n);
}
void uhi_fill_u32(void* stream, uint32_t* out, uint32_t n, uint32_t value) {
   if (n) k_fill_u32<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(out, n, value);
}
float uhi_box_decode(uint32_t u) {
   const uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
   float f;
   __builtin_memcpy(&f, &b, 4);
   return f;
}
