// raster_device.h — the fixed-function stages the two rasterisers share (shadow_map.hip's depth-only cascades, forward.hip's
// perspective forward pass): the guard-band clip, the 8-bit snap, orientation and box, and the integer edge functions with the
// top-left rule. Every step is exact and pinned: DESIGN.md section 2, "Shadow maps" (the forward pass adds its own steps in front,
// "Forward pass").
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace uh {
namespace raster {

constexpr float kGuard = 524288.0f;  // 2^19 pixels: the guard band every vertex is clipped to; snapped coordinates stay below 2^27

// One screen-space triangle after the snap: vertex k at (X[k], Y[k]) / 256 with depth z[k]; `swapped` says vertices 1 and 2 of the
// input were exchanged to make the winding positive (no culling), so a caller carrying more per-vertex data swaps it alike.
struct SubTri {
   int X[3], Y[3];
   float z[3];
   int x0, x1, y0, y1;  // the pixels whose centres the snapped box holds, inclusive, inside [0, W) x [0, H)
   bool swapped;
};

__device__ __forceinline__ int ceil_shift8(int a) { return -((-a) >> 8); }
__device__ __forceinline__ bool top_left(int dx, int dy) { return dy < 0 || (dy == 0 && dx > 0); }

// snap, orient, box and reject one triangle of screen-space vertices (all inside the guard band); false when it emits nothing
template <class V>
__device__ __forceinline__ bool finish(const V& a, const V& b, const V& c, int W, int H, SubTri& t) {
   if (a.z < 0.0f && b.z < 0.0f && c.z < 0.0f) return false;
   if (a.z > 1.0f && b.z > 1.0f && c.z > 1.0f) return false;
   int X[3] = {(int)rintf(a.x * 256.0f), (int)rintf(b.x * 256.0f), (int)rintf(c.x * 256.0f)};
   int Y[3] = {(int)rintf(a.y * 256.0f), (int)rintf(b.y * 256.0f), (int)rintf(c.y * 256.0f)};
   float z[3] = {a.z, b.z, c.z};
   const long long area = (long long)(X[1] - X[0]) * (Y[2] - Y[0]) - (long long)(Y[1] - Y[0]) * (X[2] - X[0]);
   if (area == 0) return false;
   t.swapped = area < 0;
   if (t.swapped) {  // no culling: the other winding is swapped into this one
      int tx = X[1], ty = Y[1];
      float tz = z[1];
      X[1] = X[2], Y[1] = Y[2], z[1] = z[2];
      X[2] = tx, Y[2] = ty, z[2] = tz;
   }
   const int xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
   const int ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
   t.x0 = max(ceil_shift8(xmin - 128), 0);
   t.x1 = min((xmax - 128) >> 8, W - 1);
   t.y0 = max(ceil_shift8(ymin - 128), 0);
   t.y1 = min((ymax - 128) >> 8, H - 1);
   if (t.x0 > t.x1 || t.y0 > t.y1) return false;
   for (int k = 0; k < 3; k++) t.X[k] = X[k], t.Y[k] = Y[k], t.z[k] = z[k];
   return true;
}

// Sutherland-Hodgman against x >= -G, x <= G, y >= -G, y <= G, in that order; a crossing edge's point is computed from its inside
// end a towards its outside end b (so the two triangles of a shared edge compute the same point): t = (B - a.c) / (b.c - a.c),
// the clipped coordinate B, the other a.o + t (b.o - a.o); V::lerp(r, a, b, t) fills the rest (z: a.z + t (b.z - a.z)). Returns the
// vertex count (0 or 3..7) in v.
template <class V>
__device__ __noinline__ int clip_guard(V* v, int n) {
   V tmp[8];
   for (int p = 0; p < 4; p++) {
      const int axis = p >> 1;
      const float B = (p & 1) ? kGuard : -kGuard;
      auto coord = [&](const V& q) { return axis ? q.y : q.x; };
      auto inside = [&](const V& q) { return (p & 1) ? coord(q) <= B : coord(q) >= B; };
      int m = 0;
      for (int i = 0; i < n; i++) {
         const V cur = v[i], nxt = v[(i + 1) % n];
         const bool ci = inside(cur), ni = inside(nxt);
         if (ci) tmp[m++] = cur;
         if (ci != ni) {
            const V a = ci ? cur : nxt, b = ci ? nxt : cur;
            const float t = (B - coord(a)) / (coord(b) - coord(a));
            V r;
            if (axis) {
               r.y = B;
               r.x = a.x + t * (b.x - a.x);
            } else {
               r.x = B;
               r.y = a.y + t * (b.y - a.y);
            }
            V::lerp(r, a, b, t);
            tmp[m++] = r;
         }
      }
      n = m;
      for (int i = 0; i < n; i++) v[i] = tmp[i];
      if (n < 3) return 0;
   }
   for (int i = 0; i < n; i++)
      if (!(fabsf(v[i].x) <= kGuard) || !(fabsf(v[i].y) <= kGuard) || !(v[i].z == v[i].z)) return 0;
   return n;
}

// one screen-space triangle (a, b, c) of a W x H target through the rejects, the guard-band clip and the snap: emit(k, SubTri, piece)
// for each piece k that reaches the rasteriser, piece[0..2] the three (clipped) vertices it was made of, in input order
template <class V, class Emit>
__device__ __forceinline__ void screen_triangle(const V& a, const V& b, const V& c, int W, int H, Emit&& emit) {
   const V* in[3] = {&a, &b, &c};
   bool guard = false, finite = true;
   for (int k = 0; k < 3; k++) {
      finite = finite && isfinite(in[k]->x) && isfinite(in[k]->y) && isfinite(in[k]->z);
      guard = guard || !(fabsf(in[k]->x) <= kGuard) || !(fabsf(in[k]->y) <= kGuard);
   }
   if (!finite) return;
   if (a.z < 0.0f && b.z < 0.0f && c.z < 0.0f) return;
   if (a.z > 1.0f && b.z > 1.0f && c.z > 1.0f) return;
   // every vertex on the far side of one viewport edge: no pixel centre can be covered (snapping moves a vertex by 1/512 pixel)
   const float fW = (float)W, fH = (float)H;
   if ((a.x < 0.0f && b.x < 0.0f && c.x < 0.0f) || (a.y < 0.0f && b.y < 0.0f && c.y < 0.0f)) return;
   if ((a.x > fW && b.x > fW && c.x > fW) || (a.y > fH && b.y > fH && c.y > fH)) return;
   SubTri st;
   if (!guard) {
      const V* piece[3] = {&a, &b, &c};
      if (finish(a, b, c, W, H, st)) emit(0, st, piece);
      return;
   }
   V v[8] = {a, b, c};
   const int n = clip_guard(v, 3);
   int k = 0;
   for (int j = 1; j + 1 < n; j++) {  // the fan (v0, vj, vj+1)
      const V* piece[3] = {&v[0], &v[j], &v[j + 1]};
      if (finish(v[0], v[j], v[j + 1], W, H, st)) emit(k++, st, piece);
   }
}

// the three integer edge functions of a snapped triangle at pixel (px, py)'s centre and whether it covers it: every edge function
// > 0, or = 0 on a top-left edge (edges v1 -> v2, v2 -> v0, v0 -> v1)
struct Edges {
   int X0, Y0, X1, Y1, X2, Y2;
   bool tl0, tl1, tl2;
   float fa;  // the doubled area, as a float
};
__device__ __forceinline__ Edges make_edges(int X0, int Y0, int X1, int Y1, int X2, int Y2) {
   Edges q;
   q.X0 = X0, q.Y0 = Y0, q.X1 = X1, q.Y1 = Y1, q.X2 = X2, q.Y2 = Y2;
   const long long area = (long long)(X1 - X0) * (Y2 - Y0) - (long long)(Y1 - Y0) * (X2 - X0);
   q.fa = (float)area;
   q.tl0 = top_left(X2 - X1, Y2 - Y1);
   q.tl1 = top_left(X0 - X2, Y0 - Y2);
   q.tl2 = top_left(X1 - X0, Y1 - Y0);
   return q;
}
__device__ __forceinline__ bool cover(const Edges& q, int px, int py, long long& e0, long long& e1, long long& e2) {
   const long long Px = (long long)px * 256 + 128, Py = (long long)py * 256 + 128;
   e0 = (long long)(q.X2 - q.X1) * (Py - q.Y1) - (long long)(q.Y2 - q.Y1) * (Px - q.X1);
   e1 = (long long)(q.X0 - q.X2) * (Py - q.Y2) - (long long)(q.Y0 - q.Y2) * (Px - q.X2);
   e2 = (long long)(q.X1 - q.X0) * (Py - q.Y0) - (long long)(q.Y1 - q.Y0) * (Px - q.X0);
   return (e0 > 0 || (e0 == 0 && q.tl0)) && (e1 > 0 || (e1 == 0 && q.tl1)) && (e2 > 0 || (e2 == 0 && q.tl2));
}
// depth affine in screen space from the integer barycentrics: z0 + l1 (z1 - z0) + l2 (z2 - z0), l_k = e_k / area
__device__ __forceinline__ float depth_at(const Edges& q, float z0, float z1, float z2, long long e1, long long e2) {
   const float l1 = (float)e1 / q.fa, l2 = (float)e2 / q.fa;
   return (z0 + l1 * (z1 - z0)) + l2 * (z2 - z0);
}

}  // namespace raster
}  // namespace uh
