// node_slab.h - the float arithmetic of the BVH4 node test (traversal.h node_compute), as host + device functions, so that the
// traversal kernels and the host check of that arithmetic (tests/cpp/bvh_check.cpp) compile the same text.
//
// A child plane is origin + step * q (bvh.h Node4C, node_quant.h), so along one axis
//     t(q) = q * (step * idir) + (origin - o) * idir = q * a + b.
// Two roundings have to be allowed for (DESIGN.md "Arithmetic contract"):
//   the test's own: t(q) carries a few 2^-24 of |b| + q |a|, and idir one ulp of the hardware reciprocal;
//   the triangle test's: Moeller-Trumbore works on o - v0, which it knows to 2^-24 of its length, so it accepts rays that pass
//   a triangle - and the triangle's box - at a distance of a few 2^-24 |o - v0|, in any direction.
// Both grow with the distance between the ray's origin and the geometry; the builders' box padding (1e-4 + 1e-5 |coord|) does
// not. So the children's boxes of a node are grown, on every side, by kSlabMargin times the node's REACH: the largest distance
// along any axis between the ray's origin and the far end of the node's frame, in which the children's planes lie (bounded by
// the largest |origin - o| plus 255 of the largest step). It enters the test per axis, as the parameter margin
// m = kSlabMargin * reach * |idir|, subtracted from the near planes' b and added to the far planes'. A ray parallel to an axis
// (|idir| = 1e30) keeps its huge parameters beside that margin and still misses the boxes it passes by. Where the margin
// overflows (coordinates beyond 1e13 under such a ray) a parameter becomes inf or NaN, and fmax / fmin drop a NaN: that axis
// stops culling, it never culls more. The margin can open the inverted box of an empty slot: node_compute counts its slots.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define UH_HD __host__ __device__
#else
#ifndef UH_HD
#define UH_HD
#endif
#endif

namespace uh {

// 4 x the smallest power of two at which tests/cpp/bvh_check.cpp finds no (ray, triangle) pair that the triangle test accepts and a
// slot on the way to the triangle culls: measured 2^-18 (DESIGN.md "Arithmetic contract" has the series and what sets it)
#ifndef UH_SLAB_MARGIN
#define UH_SLAB_MARGIN 0x1p-16f
#endif
constexpr float kSlabMargin = UH_SLAB_MARGIN;

// per node: the growth of its children's boxes. d = origin - o per axis; 255 steps span the frame, so the far end of the frame
// is within max |d| + 255 max step of the ray's origin on every axis
UH_HD inline float slab_node_growth(float dx, float sx, float dy, float sy, float dz, float sz) {
   const float reach = fmaf(255.0f, fmaxf(fmaxf(sx, sy), sz), fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz)));
   return kSlabMargin * reach;
}

// per node and axis: t(q) = q * a + b_near for the planes the ray enters through, q * a + b_far for those it leaves through
UH_HD inline void slab_axis(float d, float step, float idir, float growth, float& a, float& b_near, float& b_far) {
   const float m = growth * fabsf(idir);
   a = step * idir;
   b_near = fmaf(d, idir, -m);
   b_far = fmaf(d, idir, m);
}

UH_HD inline float slab_t(uint32_t q, float a, float b) { return fmaf((float)q, a, b); }

}  // namespace uh
