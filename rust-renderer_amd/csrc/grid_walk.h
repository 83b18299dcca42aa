// grid_walk.h — the sun grid's look-up (sun_grid.h) as the kernels walk it: a ray's cell, the coarse cover, and one sun ray through its
// cell's list. Shared by k_trace_sun_grid (kernels.hip) and k_path_fused (path_fused.hip); static_for also unrolls the sun-grid kernel's
// K-rays-per-lane stages.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_math.h"
#include "device_types.h"
#include "traversal.h"

namespace uh {

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop the compiler cannot leave rolled (arrays indexed by its
// counter stay in registers whatever the body holds)
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f) {
   if constexpr (I < N) {
      f(std::integral_constant<int, I>{});
      static_for<N, I + 1>(f);
   }
}

// The ray's cell: (pu, pv) = its origin in the grid's frame; outside the grid (or NaN) it is a border cell.
__device__ __forceinline__ void sun_cell_of(const SunGridDev& g, float pu, float pv, uint32_t& cx, uint32_t& cy) {
   float fx = (pu - g.u0) * g.inv_cell, fy = (pv - g.v0) * g.inv_cell;
   fx = !(fx >= 0.0f) ? 0.0f : fx;
   fy = !(fy >= 0.0f) ? 0.0f : fy;
   const float max_x = (float)(g.nx - 1), max_y = (float)(g.ny - 1);
   fx = fx > max_x ? max_x : fx;
   fy = fy > max_y ? max_y : fy;
   cx = (uint32_t)fx;
   cy = (uint32_t)fy;
}
// The coarse cover (SunGridDev::coarse, sun_grid.h): one depth per block of cells, below every cell's own cover depth - a ray that
// starts below it is below its own cell's cover too. 0.7 MB on the config-1 scene: it stays in an XCD's L2, where the cell
// records (23 MB) are a request to the memory side per ray.
__device__ __forceinline__ bool sun_coarse_covered(float coarse, float pw) { return pw < coarse && coarse - pw < kSunCoarseReach; }

// one sun ray through the grid (k_trace_sun_grid's walk for one ray): 0 = lit, 1 = occluded, 2 = the grid does not answer (border cell,
// long list): the tree's
template <bool COUNT, bool INLINE>
__device__ __forceinline__ int sun_grid_query(const SunGridDev& g, const float4* __restrict__ packets, V3 o, V3 d, uint32_t& n_tris, uint32_t& n_covered) {
   typedef float f4_t __attribute__((ext_vector_type(4)));
   const f4_t* __restrict__ recs = reinterpret_cast<const f4_t*>(g.recs);
   const f4_t* __restrict__ tris = reinterpret_cast<const f4_t*>(packets);
   const uint2* __restrict__ entries = reinterpret_cast<const uint2*>(g.entries);
   const uint4* __restrict__ cells = reinterpret_cast<const uint4*>(g.cell_start);
   const float pu = dot_fma(v3(g.U[0], g.U[1], g.U[2]), o), pv = dot_fma(v3(g.V[0], g.V[1], g.V[2]), o), pw = dot_fma(v3(g.W[0], g.W[1], g.W[2]), o);
   uint32_t cx, cy;
   sun_cell_of(g, pu, pv, cx, cy);
   if (g.coarse) {
      const float cw = g.coarse[(cy >> g.coarse_shift) * g.coarse_nx + (cx >> g.coarse_shift)];
      if (sun_coarse_covered(cw, pw)) {
         if (COUNT) n_covered++;
         return 1;
      }
   }
   const uint32_t cell = cy * g.nx + cx;
   const uint4 cs = cells[cell];
   const uint32_t end = cells[cell + 1].x;
   const float cover = __uint_as_float(cs.y);
   if (pw < cover && cover - pw < kSunCoverReach) {
      if (COUNT) n_covered++;
      return 1;
   }
   if (cx == 0 || cy == 0 || cx + 1 == g.nx || cy + 1 == g.ny || end - cs.x > g.max_walk) return 2;
   if (cs.x >= end) return 0;
   Hit best;
   best.t = 10000.0f;  // tmax (rgen:66)
   best.u = best.v = 0.0f;
   best.idx = kEmptyRef;
   best.key = 0xffffffffu;
   uint32_t e = cs.x;
   if constexpr (INLINE) {
      const f4_t* r = recs + 4 * (size_t)e;
      for (;;) {
         const f4_t na = r[0], nb = r[1], nc = r[2];
         if (nc.z < pw) return 0;  // from here on every packet ends behind the origin
         if (COUNT) n_tris++;
         if (tri_compute<true>(make_float4(na.x, na.y, na.z, na.w), make_float4(nb.x, nb.y, nb.z, nb.w), make_float4(nc.x, nc.y, nc.z, nc.w), 0u, o, d, 0.001f, INFINITY, best)) return 1;
         e++;
         if (e >= end || nc.w < pw) return 0;
         r += 4;
      }
   } else {
      uint2 cur = make_uint2(cs.z, cs.w);  // the list's first entry came with the cell record
      for (;;) {
         if (__uint_as_float(cur.y) < pw) return 0;  // sorted by far depth, descending
         const f4_t* r = tris + kTriStride16 * (size_t)cur.x;
         const f4_t na = r[0], nb = r[1], nc = r[2];
         e++;
         const uint2 nx = e < end ? entries[e] : make_uint2(0u, 0u);  // in flight with the packet
         if (COUNT) n_tris++;
         if (tri_compute<true>(make_float4(na.x, na.y, na.z, na.w), make_float4(nb.x, nb.y, nb.z, nb.w), make_float4(nc.x, nc.y, nc.z, nc.w), cur.x, o, d, 0.001f, INFINITY, best)) return 1;
         if (e >= end) return 0;
         cur = nx;
      }
   }
}

}  // namespace uh
