// forward.hip — the forward pass of build_minimal_forward_render_graph (utopian/src/renderers/forward.rs, shaders/forward/forward.vert /
// forward.frag) on gfx950: a perspective triangle rasteriser with a depth test and perspective-correct interpolation, then forward.frag
// once per pixel (a visibility buffer: under LESS_OR_EQUAL only the surviving fragment's colour remains). Four kernels, and a fifth
// for the hybrid graph's rasterised G-buffer:
//   k_forward_count    one lane per triangle (= draw index): forward.vert's gl_Position, clip to 0 <= z <= w, divide, viewport, then
//                      raster_device.h's guard-band clip, snap and rejects; counts its records and, per tile its box touches, one entry
//   (device_scan.h)    record offsets (in draw order) and the tiles' first entries
//   k_forward_emit     the same setup again: writes the records and scatters their ids into the tiles' lists
//   k_forward_resolve  one block per tile: the 64-bit min of depth_bits << 32 | (0xFFFFFFFE - record) per pixel in LDS (ds_min_u64) -
//                      the last record in draw order among those of minimum depth - then depth, draw index and record written out once
//   k_forward_shade    one lane per pixel: the surviving record's perspective-correct barycentrics, forward.vert's attributes and
//                      forward.frag (surfaceShading over the sun and the lights, ambient, calculateShadow)
//   k_gbuffer_raster_shade  one lane per pixel: the same prologue (fragment_at), then gbuffer.frag's four targets
// The kernels are templates on the triangle source and the depth seed. The forward pass draws the scene's meshes (kFlat = false) into
// a depth buffer cleared to 1.0; the hybrid graph's marching-cubes pass draws a flat list of world-space triangles (vertex 3 t + k of
// triangle t, one mesh of its own) against a depth buffer seeded from the G-buffer (kSeed), shading only the pixels it covers.
// The rasterised G-buffer draws the scene's meshes as the forward pass does, into a depth buffer of its own.
// Every step is exact and pinned: DESIGN.md section 2, "Forward pass", "Marching-cubes pass" and "Rasterised G-buffer".
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_math.h"
#include "device_types.h"
#include "hybrid_shading.h"
#include "motion_device.h"
#include "raster_device.h"
#include "utopian_hip.h"

namespace uh {

namespace {
using raster::SubTri;
constexpr int kSetupBlock = 256, kResolveBlock = 256, kShadeBlock = 256;
constexpr int kSmallPixels = 16;                   // a piece whose box in the tile has at most this many pixels is drawn by one lane
constexpr unsigned long long kEmptyKey = ~0ull;    // no fragment: depth 1.0, no visibility
constexpr uint32_t kNone = 0xFFFFFFFFu;
// a key's low word: 0xFFFFFFFE - record (records stay below 0xFFFFFFFF), so the last record in draw order has the smallest, and
// 0xFFFFFFFF is left for no fragment - a seeded depth loses every tie with a fragment
__device__ __forceinline__ uint32_t key_low(uint32_t r) { return 0xFFFFFFFEu - r; }
__device__ __forceinline__ uint32_t key_record(unsigned long long key) {
   const uint32_t lo = (uint32_t)key;
   return lo == kNone ? kNone : 0xFFFFFFFEu - lo;
}

// a clip-space vertex and its barycentrics with respect to the original triangle
struct HVert {
   float x, y, z, w, b[3];
};
// a screen-space vertex: x, y in pixels, z the depth, w the clip w, b the original triangle's barycentrics. A guard-band crossing
// interpolates 1/w and b/w (affine in screen space) and divides back, so the new vertex stays on the triangle.
struct FVert {
   float x, y, z, w, b[3];
   __device__ static void lerp(FVert& r, const FVert& a, const FVert& b, float t) {
      r.z = a.z + t * (b.z - a.z);
      const float ia = 1.0f / a.w, ib = 1.0f / b.w, iw = ia + t * (ib - ia);
      r.w = 1.0f / iw;
      for (int j = 0; j < 3; j++) {
         const float pa = a.b[j] * ia, pb = b.b[j] * ib;
         r.b[j] = (pa + t * (pb - pa)) / iw;
      }
   }
};

// Sutherland-Hodgman in homogeneous space against z >= 0, then z <= w (d = z, then d = w - z): a crossing is computed from its
// inside end a towards its outside end b, t = d_a / (d_a - d_b), every component a + t (b - a). Returns the count (0 or 3..5).
__device__ __forceinline__ int clip_depth(HVert* v, int n) {
   HVert tmp[5];
   for (int p = 0; p < 2; p++) {
      auto dist = [&](const HVert& q) { return p ? q.w - q.z : q.z; };
      int m = 0;
      for (int i = 0; i < n; i++) {
         const HVert cur = v[i], nxt = v[(i + 1) % n];
         const float dc = dist(cur), dn = dist(nxt);
         const bool ci = dc >= 0.0f, ni = dn >= 0.0f;
         if (ci) tmp[m++] = cur;
         if (ci != ni) {
            const HVert a = ci ? cur : nxt, b = ci ? nxt : cur;
            const float da = ci ? dc : dn, db = ci ? dn : dc;
            const float t = da / (da - db);
            HVert r;
            r.x = a.x + t * (b.x - a.x);
            r.y = a.y + t * (b.y - a.y);
            r.z = a.z + t * (b.z - a.z);
            r.w = a.w + t * (b.w - a.w);
            for (int j = 0; j < 3; j++) r.b[j] = a.b[j] + t * (b.b[j] - a.b[j]);
            tmp[m++] = r;
         }
      }
      n = m;
      for (int i = 0; i < n; i++) v[i] = tmp[i];
      if (n < 3) return 0;
   }
   return n;
}

// triangle t through forward.vert's gl_Position and the fixed-function stages: emit(k, SubTri, piece) for each piece that reaches the
// rasteriser, piece[0..2] its three screen-space vertices in SubTri order before the winding swap
// the vertex k of triangle t and its mesh: the scene's tables, or (kFlat) vertex 3 t + k of mesh 0
template <bool kFlat>
__device__ __forceinline__ uint32_t mesh_of(const ForwardDev& fd, uint32_t t) { return kFlat ? 0u : fd.tri_mesh[t]; }
template <bool kFlat>
__device__ __forceinline__ const UhVertex& vertex_of(const ForwardDev& fd, uint32_t vertex_base, uint32_t t, int k) {
   return kFlat ? fd.vertices[3 * (size_t)t + k] : fd.vertices[vertex_base + fd.indices[3 * (size_t)t + k]];
}

template <bool kFlat, class Emit>
__device__ __forceinline__ void setup(const ForwardDev& fd, uint32_t t, Emit&& emit) {
   const uint32_t mesh = mesh_of<kFlat>(fd, t);
   const float* M = fd.mats + (size_t)mesh * 28;
   const uint32_t vb = kFlat ? 0u : fd.meshes[mesh].vertex_base;
   HVert v[5];
   bool finite = true;
   for (int k = 0; k < 3; k++) {
      const UhVertex& vx = vertex_of<kFlat>(fd, vb, t, k);
      const float px = vx.pos[0], py = vx.pos[1], pz = vx.pos[2];
      // gl_Position = ((P V) W) (p, 1), mat4_mul's column order
      v[k].x = ((M[0] * px + M[4] * py) + M[8] * pz) + M[12] * 1.0f;
      v[k].y = ((M[1] * px + M[5] * py) + M[9] * pz) + M[13] * 1.0f;
      v[k].z = ((M[2] * px + M[6] * py) + M[10] * pz) + M[14] * 1.0f;
      v[k].w = ((M[3] * px + M[7] * py) + M[11] * pz) + M[15] * 1.0f;
      for (int j = 0; j < 3; j++) v[k].b[j] = j == k ? 1.0f : 0.0f;
      finite = finite && isfinite(v[k].x) && isfinite(v[k].y) && isfinite(v[k].z) && isfinite(v[k].w);
   }
   if (!finite) return;
   const int n = clip_depth(v, 3);
   const float fW = (float)fd.W, fH = (float)fd.H, hw = fW * 0.5f, hh = fH * 0.5f, nhh = -hh;
   FVert s[5];
   for (int i = 0; i < n; i++) {  // divide by w, then the viewport (0, H, W, -H): x = W/2 + xn W/2, y = H/2 - yn H/2
      const float xn = v[i].x / v[i].w, yn = v[i].y / v[i].w, zn = v[i].z / v[i].w;
      s[i].x = xn * hw + hw;
      s[i].y = yn * nhh + hh;
      s[i].z = zn;
      s[i].w = v[i].w;
      for (int j = 0; j < 3; j++) s[i].b[j] = v[i].b[j];
   }
   int k = 0;
   for (int j = 1; j + 1 < n; j++)  // the fan (s0, sj, sj+1)
      raster::screen_triangle(s[0], s[j], s[j + 1], (int)fd.W, (int)fd.H, [&](int, const SubTri& st, const FVert* const* piece) { emit(k++, st, piece); });
}

template <class F>
__device__ __forceinline__ void for_tiles(const SubTri& st, uint32_t tiles_x, F&& f) {
   for (int ty = st.y0 / (int)kForwardTile; ty <= st.y1 / (int)kForwardTile; ty++)
      for (int tx = st.x0 / (int)kForwardTile; tx <= st.x1 / (int)kForwardTile; tx++) f((uint32_t)ty * tiles_x + (uint32_t)tx);
}

template <bool kFlat>
__global__ __launch_bounds__(kSetupBlock) void k_forward_count(ForwardDev fd) {
   for (uint32_t t = blockIdx.x * kSetupBlock + threadIdx.x; t < fd.num_tris; t += gridDim.x * kSetupBlock) {
      uint32_t count = 0;
      setup<kFlat>(fd, t, [&](int, const SubTri& st, const FVert* const*) {
         count++;
         for_tiles(st, fd.tiles_x, [&](uint32_t tile) { atomicAdd(&fd.tile_count[tile], 1u); });
      });
      fd.rec_count[t] = count;
   }
}

// record r, 6 uint4: (X0, Y0, X1, Y1) (X2, Y2, z0, z1) (z2, x0 | x1 << 16, y0 | y1 << 16, draw) (w0, w1, w2, b00) (b01, b02, b10, b11)
// (b12, b20, b21, b22), vertex order after the winding swap; the first three are the shadow maps' record with the draw index added
template <bool kFlat>
__global__ __launch_bounds__(kSetupBlock) void k_forward_emit(ForwardDev fd) {
   for (uint32_t t = blockIdx.x * kSetupBlock + threadIdx.x; t < fd.num_tris; t += gridDim.x * kSetupBlock) {
      const uint32_t first = fd.rec_count[t];
      setup<kFlat>(fd, t, [&](int k, const SubTri& st, const FVert* const* piece) {
         const uint32_t r = first + (uint32_t)k;
         const FVert* p[3] = {piece[0], st.swapped ? piece[2] : piece[1], st.swapped ? piece[1] : piece[2]};
         uint4* q = fd.records + 6 * (size_t)r;
         auto u = [](float f) { return __float_as_uint(f); };
         q[0] = make_uint4((uint32_t)st.X[0], (uint32_t)st.Y[0], (uint32_t)st.X[1], (uint32_t)st.Y[1]);
         q[1] = make_uint4((uint32_t)st.X[2], (uint32_t)st.Y[2], u(st.z[0]), u(st.z[1]));
         q[2] = make_uint4(u(st.z[2]), (uint32_t)st.x0 | ((uint32_t)st.x1 << 16), (uint32_t)st.y0 | ((uint32_t)st.y1 << 16), t);
         q[3] = make_uint4(u(p[0]->w), u(p[1]->w), u(p[2]->w), u(p[0]->b[0]));
         q[4] = make_uint4(u(p[0]->b[1]), u(p[0]->b[2]), u(p[1]->b[0]), u(p[1]->b[1]));
         q[5] = make_uint4(u(p[1]->b[2]), u(p[2]->b[0]), u(p[2]->b[1]), u(p[2]->b[2]));
         for_tiles(st, fd.tiles_x, [&](uint32_t tile) { fd.entries[atomicAdd(&fd.tile_cursor[tile], 1u)] = r; });
      });
   }
}

struct Rec {
   raster::Edges e;
   float z0, z1, z2;
   int x0, x1, y0, y1;
};
__device__ __forceinline__ Rec load_rec(const uint4* __restrict__ records, uint32_t r) {
   const uint4 a = records[6 * (size_t)r], b = records[6 * (size_t)r + 1], c = records[6 * (size_t)r + 2];
   Rec q;
   q.e = raster::make_edges((int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y);
   q.z0 = __uint_as_float(b.z), q.z1 = __uint_as_float(b.w), q.z2 = __uint_as_float(c.x);
   q.x0 = (int)(c.y & 0xffffu), q.x1 = (int)(c.y >> 16), q.y0 = (int)(c.z & 0xffffu), q.y1 = (int)(c.z >> 16);
   return q;
}
// pixel (px, py) of record r: covered, then z kept when 0 <= z <= 1 (-0 as +0), then the unsigned min of the key
__device__ __forceinline__ void raster_pixel(const Rec& q, uint32_t r, int px, int py, unsigned long long* keys, int ox, int oy) {
   long long e0, e1, e2;
   if (!raster::cover(q.e, px, py, e0, e1, e2)) return;
   const float z = raster::depth_at(q.e, q.z0, q.z1, q.z2, e1, e2);
   if (!(z >= 0.0f && z <= 1.0f)) return;
   const uint32_t bits = z == 0.0f ? 0u : __float_as_uint(z);
   atomicMin(&keys[(py - oy) * (int)kForwardTile + (px - ox)], ((unsigned long long)bits << 32) | (unsigned long long)key_low(r));
}

// kSeed: every pixel's key starts at seed_bits << 32 | 0xFFFFFFFF (fd.depth holds the seed and receives the result), so a fragment
// survives when its depth is at most the seed's (LESS_OR_EQUAL against the seeded depth buffer)
template <bool kSeed>
__global__ __launch_bounds__(kResolveBlock) void k_forward_resolve(ForwardDev fd) {
   __shared__ unsigned long long s_key[kForwardTile * kForwardTile];  // 32 KiB
   __shared__ uint32_t s_big[kResolveBlock];
   __shared__ uint32_t s_nbig, s_covered;
   const uint32_t tile = blockIdx.x;
   const int ox = (int)((tile % fd.tiles_x) * kForwardTile), oy = (int)((tile / fd.tiles_x) * kForwardTile);
   const int W = (int)fd.W, tw = min((int)kForwardTile, W - ox), th = min((int)kForwardTile, (int)fd.H - oy);
   for (uint32_t i = threadIdx.x; i < kForwardTile * kForwardTile; i += kResolveBlock) {
      unsigned long long key = kEmptyKey;
      if (kSeed) {
         const int ly = (int)(i / kForwardTile), lx = (int)(i % kForwardTile);
         if (lx < tw && ly < th) key = ((unsigned long long)__float_as_uint(fd.depth[(size_t)(oy + ly) * W + ox + lx]) << 32) | kNone;
      }
      s_key[i] = key;
   }
   if (threadIdx.x == 0) s_nbig = 0, s_covered = 0;
   __syncthreads();
   const uint32_t begin = fd.tile_count[tile], end = fd.tile_cursor[tile];
   for (uint32_t base = begin; base < end; base += kResolveBlock) {
      const uint32_t i = base + threadIdx.x;
      if (i < end) {
         const uint32_t r = fd.entries[i];
         const Rec q = load_rec(fd.records, r);
         const int x0 = max(q.x0, ox), x1 = min(q.x1, ox + tw - 1), y0 = max(q.y0, oy), y1 = min(q.y1, oy + th - 1);
         if ((x1 - x0 + 1) * (y1 - y0 + 1) <= kSmallPixels) {
            for (int py = y0; py <= y1; py++)
               for (int px = x0; px <= x1; px++) raster_pixel(q, r, px, py, s_key, ox, oy);
         } else {
            s_big[atomicAdd(&s_nbig, 1u)] = r;
         }
      }
      __syncthreads();
      const uint32_t nbig = s_nbig;
      for (uint32_t k = 0; k < nbig; k++) {  // the large boxes: the whole block strides over the box's pixels in the tile
         const uint32_t r = s_big[k];
         const Rec q = load_rec(fd.records, r);
         const int x0 = max(q.x0, ox), x1 = min(q.x1, ox + tw - 1), y0 = max(q.y0, oy), y1 = min(q.y1, oy + th - 1);
         const int w = x1 - x0 + 1, npx = w * (y1 - y0 + 1);
         for (int p = (int)threadIdx.x; p < npx; p += kResolveBlock) raster_pixel(q, r, x0 + p % w, y0 + p / w, s_key, ox, oy);
      }
      __syncthreads();
      if (threadIdx.x == 0) s_nbig = 0;
      __syncthreads();
   }
   for (int i = (int)threadIdx.x; i < tw * th; i += kResolveBlock) {
      const int ly = i / tw, lx = i - ly * tw;
      const unsigned long long key = s_key[ly * (int)kForwardTile + lx];
      const size_t pix = (size_t)(oy + ly) * W + ox + lx;
      const uint32_t r = key_record(key);
      fd.depth[pix] = !kSeed && r == kNone ? 1.0f : __uint_as_float((uint32_t)(key >> 32));
      fd.rec_of[pix] = r;
      fd.vis[pix] = r == kNone ? kNone : fd.records[6 * (size_t)r + 2].w;
      if (r != kNone) atomicAdd(&s_covered, 1u);
   }
   __syncthreads();
   if (threadIdx.x == 0 && s_covered) atomicAdd(fd.covered, s_covered);
}

// the fragment stage's prologue at pixel i of surviving record r: the record's integer edge functions give the screen weights
// l_k = e_k / area; q_k = l_k / w_k and b = (q0 B0 + q1 B1 + q2 B2) / (q0 + q1 + q2) are the original triangle's barycentrics; every
// attribute is (a0 b0 + a1 b1) + a2 b2: out_pos = (world (p, 1)).xyz (world row-major 3x4), then surface_attributes. forward.frag and
// gbuffer.frag share it (k_forward_shade, k_gbuffer_raster_shade).
struct Fragment {
   uint32_t mesh;
   HybridMesh m;
   V3 P, N;
   float uu, vv;
   uint32_t tri;       // the draw index
   float b0, b1, b2;   // the original triangle's barycentrics
};
template <bool kFlat>
__device__ __forceinline__ Fragment fragment_at(const SceneDev& sc, const ForwardDev& fd, uint32_t i, uint32_t r) {
   const uint4* q = fd.records + 6 * (size_t)r;
   const uint4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
   const raster::Edges ed = raster::make_edges((int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y);
   long long e0, e1, e2;
   raster::cover(ed, (int)(i % fd.W), (int)(i / fd.W), e0, e1, e2);
   const float l0 = (float)e0 / ed.fa, l1 = (float)e1 / ed.fa, l2 = (float)e2 / ed.fa;
   const float q0 = l0 / __uint_as_float(d.x), q1 = l1 / __uint_as_float(d.y), q2 = l2 / __uint_as_float(d.z);
   const float B[3][3] = {{__uint_as_float(d.w), __uint_as_float(e.x), __uint_as_float(e.y)},
                          {__uint_as_float(e.z), __uint_as_float(e.w), __uint_as_float(f.x)},
                          {__uint_as_float(f.y), __uint_as_float(f.z), __uint_as_float(f.w)}};
   const float s = (q0 + q1) + q2;
   const float b0 = ((q0 * B[0][0] + q1 * B[1][0]) + q2 * B[2][0]) / s;
   const float b1 = ((q0 * B[0][1] + q1 * B[1][1]) + q2 * B[2][1]) / s;
   const float b2 = ((q0 * B[0][2] + q1 * B[1][2]) + q2 * B[2][2]) / s;
   Fragment fr;
   const uint32_t t = c.w;
   fr.mesh = mesh_of<kFlat>(fd, t);
   fr.m = fd.meshes[fr.mesh];
   const UhVertex& v0 = vertex_of<kFlat>(fd, fr.m.vertex_base, t, 0);
   const UhVertex& v1 = vertex_of<kFlat>(fd, fr.m.vertex_base, t, 1);
   const UhVertex& v2 = vertex_of<kFlat>(fd, fr.m.vertex_base, t, 2);
   const float* o = fd.mats + (size_t)fr.mesh * 28 + 16;
   auto world = [&](const UhVertex& v) {
      return v3(((o[0] * v.pos[0] + o[1] * v.pos[1]) + o[2] * v.pos[2]) + o[3] * 1.0f, ((o[4] * v.pos[0] + o[5] * v.pos[1]) + o[6] * v.pos[2]) + o[7] * 1.0f,
                ((o[8] * v.pos[0] + o[9] * v.pos[1]) + o[10] * v.pos[2]) + o[11] * 1.0f);
   };
   fr.P = (world(v0) * b0 + world(v1) * b1) + world(v2) * b2;
   surface_attributes(sc, fr.m, v0, v1, v2, b0, b1, b2, fr.N, fr.uu, fr.vv);                  // vert, frag:44-53
   fr.tri = t;
   fr.b0 = b0, fr.b1 = b1, fr.b2 = b2;
   return fr;
}

// forward.frag at pixel i on the surviving record's fragment_at. One lane per pixel, no grid-stride loop (the light records become
// scalar loads, as in k_hybrid_deferred). kFlat (the marching-cubes pass): the material is fd.meshes[0]'s and the base colour scene
// mesh 0's (mesh_index = 0), and an uncovered pixel keeps its colour.
template <bool kFlat, bool kShadow>
__global__ __launch_bounds__(kShadeBlock) void k_forward_shade(SceneDev sc, ForwardDev fd, ForwardShade fs, ShadowLookup sl) {
   const uint32_t n = fd.W * fd.H, i = blockIdx.x * kShadeBlock + threadIdx.x;
   if (i >= n) return;
   const uint32_t r = fd.rec_of[i];
   if (r == kNone) {  // the clear colour (pass.rs: (1, 1, 1, 0)); load_write: untouched
      if (!kFlat) fd.color[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      return;
   }
   const Fragment fr = fragment_at<kFlat>(sc, fd, i, r);
   const HybridMesh& m = fr.m;
   const uint32_t mesh = fr.mesh;
   const V3 P = fr.P, N = fr.N;
   const float uu = fr.uu, vv = fr.vv;
   const V3 dt = sample_texture(sc, sc.unorm_lut, m.diffuse_map, uu, vv);                      // frag:39
   const V3 mr = sample_texture(sc, sc.unorm_lut, m.metallic_roughness_map, uu, vv);           // frag:41-42
   const V3 oc = sample_texture(sc, sc.unorm_lut, m.occlusion_map, uu, vv);                    // frag:43
   auto gamma = [](float x) { return (float)pow((double)x, (double)2.2f); };                   // frag:46, pow in double
   const V3 diffuse = v3(gamma(dt.x), gamma(dt.y), gamma(dt.z));
   V3 bc = v3(1.0f, 1.0f, 1.0f);
   if (mesh < sc.num_meshes) bc = v3(sc.meshes[mesh].base_color[0], sc.meshes[mesh].base_color[1], sc.meshes[mesh].base_color[2]);
   const V3 base = diffuse * bc;                                                                // frag:57
   const float metallic = mr.z, roughness = mr.y, occlusion = oc.x;                             // frag:41-43, no factors
   const V3 V = normalize3(v3(fs.eye[0], fs.eye[1], fs.eye[2]) - P);                            // lighting:26
   const V3 Lo = direct_lighting(fs.lights, fs.count, P, N, V, base, metallic, roughness);      // frag:66-74
   V3 color = (0.03f * diffuse) * occlusion + Lo;                                               // frag:77-78
   if (kShadow) color = color * calculate_shadow(sl, fs.view, P);                               // frag:81-85
   fd.color[i] = make_float4(color.x, color.y, color.z, 1.0f);                                  // frag:93
}

// gbuffer.frag at pixel i on the surviving record's fragment_at (the hybrid graph's rasterised G-buffer): the four targets as
// gbuffer_targets writes them for the cast, the clear values (1, 1, 1, 0) / albedo (255, 255, 255, 0) where no fragment survived. One
// lane per pixel; depth and visibility are the resolve's.
__global__ __launch_bounds__(kShadeBlock) void k_gbuffer_raster_shade(SceneDev sc, ForwardDev fd, HybridDev hd) {
   const uint32_t n = fd.W * fd.H, i = blockIdx.x * kShadeBlock + threadIdx.x;
   if (i >= n) return;
   const uint32_t r = fd.rec_of[i];
   const float4 clear = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
   float4 pos = clear, nrm = clear, pbr = clear;
   uchar4 alb = make_uchar4(255, 255, 255, 0);
   if (r != kNone) {
      const Fragment fr = fragment_at<false>(sc, fd, i, r);
      pos = make_float4(fr.P.x, fr.P.y, fr.P.z, 1.0f);                                         // frag:47, out_pos with w = 1
      gbuffer_targets(sc, fr.m, fr.mesh, fr.N, fr.uu, fr.vv, nrm, alb, pbr);
   }
   hd.pos[i] = pos;
   hd.nrm[i] = nrm;
   hd.alb[i] = alb;
   hd.pbr[i] = pbr;
}

// the motion texel (UH_HYBRID_MOTION) of pixel i on the same surviving record, behind k_gbuffer_raster_shade: the position texel it
// wrote, the record's triangle and fragment_at's barycentrics into motion_device.h's motion_texel. One lane per pixel and round, one coalesced
// 16-byte store; the normal and the texture coordinates of the prologue are not used and fall away.
__global__ __launch_bounds__(kMotionBlock) void k_gbuffer_raster_motion(SceneDev sc, ForwardDev fd, HybridDev hd, MotionDev md) {
   const uint32_t n = fd.W * fd.H;
   MotionCount count;
   for (uint32_t base = blockIdx.x * kMotionBlock; base < n; base += gridDim.x * kMotionBlock) {
      const uint32_t i = base + threadIdx.x;
      float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      bool geo = false;
      if (i < n) {
         const uint32_t r = fd.rec_of[i];
         if (r != kNone) {
            geo = true;
            const Fragment fr = fragment_at<false>(sc, fd, i, r);
            const uint32_t* tri = fd.indices + 3 * (size_t)fr.tri;
            out = motion_texel(hd, md, fr.mesh, fr.m.vertex_base, tri[0], tri[1], tri[2], fr.b0, fr.b1, fr.b2, hd.pos[i]);
         }
         md.image[i] = out;
      }
      count.add(geo, out.w);
   }
   count.store(md);
}

// the images as the first call finds them: forward_output (1, 1, 1, 0), depth 1.0, no visibility, present (255, 255, 255, 0)
__global__ __launch_bounds__(kShadeBlock) void k_forward_clear(ForwardDev fd, uchar4* present) {
   const uint32_t n = fd.W * fd.H;
   for (uint32_t i = blockIdx.x * kShadeBlock + threadIdx.x; i < n; i += gridDim.x * kShadeBlock) {
      fd.color[i] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      fd.depth[i] = 1.0f;
      fd.vis[i] = kNone;
      fd.rec_of[i] = kNone;
      present[i] = make_uchar4(255, 255, 255, 0);
   }
}

inline dim3 setup_grid(const LaunchCfg& c, uint32_t n) {
   const uint32_t blocks = (n + kSetupBlock - 1) / kSetupBlock, cap = c.num_cus * 8;
   return dim3(blocks < cap ? (blocks ? blocks : 1) : cap);
}
// the marching-cubes pass's depth seed ("Marching-cubes pass"): one lane per pixel, c = (P V) (p, 1) of the
// G-buffer position, d = c.z / c.w kept when c.w > 0 and 0 <= d <= 1 (-0 as +0), 1.0 otherwise and where the cast missed
__global__ __launch_bounds__(kShadeBlock) void k_mc_depth_seed(const float4* __restrict__ pos, ForwardDev fd) {
   const uint32_t n = fd.W * fd.H, i = blockIdx.x * kShadeBlock + threadIdx.x;
   if (i >= n) return;
   const float4 p = pos[i];
   const float* M = fd.mats + 28;  // P V, column-major
   float d = 1.0f;
   if (p.w != 0.0f) {
      const float cz = ((M[2] * p.x + M[6] * p.y) + M[10] * p.z) + M[14];
      const float cw = ((M[3] * p.x + M[7] * p.y) + M[11] * p.z) + M[15];
      const float q = cz / cw;
      if (cw > 0.0f && q >= 0.0f && q <= 1.0f) d = q == 0.0f ? 0.0f : q;
   }
   fd.depth[i] = d;
}
}  // namespace

void launch_forward_clear(const LaunchCfg& c, const ForwardDev& fd, uchar4* present) {
   k_forward_clear<<<setup_grid(c, fd.W * fd.H), kShadeBlock, 0, c.stream>>>(fd, present);
}
void launch_forward_count(const LaunchCfg& c, const ForwardDev& fd, bool flat) {
   if (!fd.num_tris) return;
   if (flat)
      k_forward_count<true><<<setup_grid(c, fd.num_tris), kSetupBlock, 0, c.stream>>>(fd);
   else
      k_forward_count<false><<<setup_grid(c, fd.num_tris), kSetupBlock, 0, c.stream>>>(fd);
}
void launch_forward_emit(const LaunchCfg& c, const ForwardDev& fd, bool flat) {
   if (!fd.num_tris) return;
   if (flat)
      k_forward_emit<true><<<setup_grid(c, fd.num_tris), kSetupBlock, 0, c.stream>>>(fd);
   else
      k_forward_emit<false><<<setup_grid(c, fd.num_tris), kSetupBlock, 0, c.stream>>>(fd);
}
void launch_forward_resolve(const LaunchCfg& c, const ForwardDev& fd, bool seeded) {
   if (seeded)
      k_forward_resolve<true><<<dim3(fd.tiles_x * fd.tiles_y), kResolveBlock, 0, c.stream>>>(fd);
   else
      k_forward_resolve<false><<<dim3(fd.tiles_x * fd.tiles_y), kResolveBlock, 0, c.stream>>>(fd);
}
void launch_forward_shade(const LaunchCfg& c, const SceneDev& sc, const ForwardDev& fd, const ForwardShade& fs, const ShadowLookup* shadow, bool flat) {
   const dim3 grid((fd.W * fd.H + kShadeBlock - 1) / kShadeBlock);
   const ShadowLookup sl = shadow ? *shadow : ShadowLookup{};
   if (flat) {
      if (shadow)
         k_forward_shade<true, true><<<grid, kShadeBlock, 0, c.stream>>>(sc, fd, fs, sl);
      else
         k_forward_shade<true, false><<<grid, kShadeBlock, 0, c.stream>>>(sc, fd, fs, sl);
   } else {
      if (shadow)
         k_forward_shade<false, true><<<grid, kShadeBlock, 0, c.stream>>>(sc, fd, fs, sl);
      else
         k_forward_shade<false, false><<<grid, kShadeBlock, 0, c.stream>>>(sc, fd, fs, sl);
   }
}
void launch_gbuffer_raster_shade(const LaunchCfg& c, const SceneDev& sc, const ForwardDev& fd, const HybridDev& hd) {
   k_gbuffer_raster_shade<<<dim3((fd.W * fd.H + kShadeBlock - 1) / kShadeBlock), kShadeBlock, 0, c.stream>>>(sc, fd, hd);
}
void launch_gbuffer_raster_motion(const LaunchCfg& c, const SceneDev& sc, const ForwardDev& fd, const HybridDev& hd, const MotionDev& md) {
   k_gbuffer_raster_motion<<<dim3(motion_blocks(fd.W * fd.H, c.num_cus)), kMotionBlock, 0, c.stream>>>(sc, fd, hd, md);
}
void launch_mc_depth_seed(const LaunchCfg& c, const float4* gbuffer_pos, const ForwardDev& fd) {
   k_mc_depth_seed<<<dim3((fd.W * fd.H + kShadeBlock - 1) / kShadeBlock), kShadeBlock, 0, c.stream>>>(gbuffer_pos, fd);
}

}  // namespace uh
