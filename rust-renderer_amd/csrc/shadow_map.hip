// shadow_map.hip — the cascaded shadow maps of setup_shadow_pass (utopian/src/renderers/shadow.rs) on gfx950: the host arithmetic of
// the cascades (uh_shadow_cascades) and a depth-only rasteriser for shadow.vert's four passes. The rasteriser bins, then resolves:
//   k_shadow_count    one lane per (triangle, cascade): transform, guard-band clip, snap, reject; counts its records and, per tile
//                     its bounding box touches, one tile entry
//   (device_scan.h)   record offsets and the tiles' first entries
//   k_shadow_emit     the same setup again: writes the records and scatters their ids into the tiles' lists
//   k_shadow_resolve  one block per (tile, cascade): the tile's depth in LDS (ds_min_u32 on the bits of non-negative floats), small
//                     bounding boxes one lane per triangle, large ones by the whole block, then the tile written out once (empty tiles
//                     write 1.0: there is no separate clear)
// Every step is exact and pinned: DESIGN.md section 2, "Shadow maps".
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "device_scan.h"
#include "device_types.h"
#include "raster_device.h"
#include "utopian_hip.h"

namespace uh {

namespace {
using raster::SubTri;
constexpr int kSetupBlock = 256, kResolveBlock = 256;
constexpr int kSmallPixels = 16;        // a triangle whose box in the tile has at most this many texels is drawn by one lane
constexpr uint32_t kOne = 0x3f800000u;  // 1.0f, the cleared depth

struct ClipVert {
   float x, y, z;
   __device__ static void lerp(ClipVert& r, const ClipVert& a, const ClipVert& b, float t) { r.z = a.z + t * (b.z - a.z); }
};

// triangle t of cascade c through shadow.vert and the fixed-function stages (raster_device.h): emit(k, SubTri) for each piece that
// reaches the rasteriser
template <class Emit>
__device__ __forceinline__ void setup(const ShadowDev& sd, uint32_t t, uint32_t c, Emit&& emit) {
   const uint32_t mesh = sd.tri_mesh[t];
   const float* M = sd.mats + ((size_t)c * sd.num_meshes + mesh) * 16;
   const uint32_t vb = sd.meshes[mesh].vertex_base;
   const float S = (float)sd.size, half = S * 0.5f, nhalf = -half;
   ClipVert v[3];
   for (int k = 0; k < 3; k++) {
      const UhVertex& vx = sd.vertices[vb + sd.indices[3 * (size_t)t + k]];
      const float px = vx.pos[0], py = vx.pos[1], pz = vx.pos[2];
      // gl_Position = M (p, 1), mat4_mul's column order; M's last row is (0, 0, 0, 1), so w = 1 exactly and the division is skipped
      const float xd = ((M[0] * px + M[4] * py) + M[8] * pz) + M[12] * 1.0f;
      const float yd = ((M[1] * px + M[5] * py) + M[9] * pz) + M[13] * 1.0f;
      const float zd = ((M[2] * px + M[6] * py) + M[10] * pz) + M[14] * 1.0f;
      v[k].x = xd * half + half;   // viewport (0, S, S, -S): x = S/2 + xd S/2, y = S/2 - yd S/2, depth 0..1
      v[k].y = yd * nhalf + half;
      v[k].z = zd;
   }
   raster::screen_triangle(v[0], v[1], v[2], (int)sd.size, (int)sd.size, [&](int k, const SubTri& st, const ClipVert* const*) { emit(k, st); });
}

template <class F>
__device__ __forceinline__ void for_tiles(const SubTri& st, uint32_t tiles_x, F&& f) {
   for (int ty = st.y0 / (int)kShadowTile; ty <= st.y1 / (int)kShadowTile; ty++)
      for (int tx = st.x0 / (int)kShadowTile; tx <= st.x1 / (int)kShadowTile; tx++) f((uint32_t)ty * tiles_x + (uint32_t)tx);
}

__global__ __launch_bounds__(kSetupBlock) void k_shadow_count(ShadowDev sd) {
   const uint32_t n = 4u * sd.num_tris, tiles = sd.tiles_x * sd.tiles_x;
   for (uint32_t i = blockIdx.x * kSetupBlock + threadIdx.x; i < n; i += gridDim.x * kSetupBlock) {
      const uint32_t c = i / sd.num_tris, t = i - c * sd.num_tris;
      uint32_t count = 0;
      setup(sd, t, c, [&](int, const SubTri& st) {
         count++;
         for_tiles(st, sd.tiles_x, [&](uint32_t tile) { atomicAdd(&sd.tile_count[c * tiles + tile], 1u); });
      });
      sd.rec_count[i] = count;
   }
}

__global__ __launch_bounds__(kSetupBlock) void k_shadow_emit(ShadowDev sd) {
   const uint32_t n = 4u * sd.num_tris, tiles = sd.tiles_x * sd.tiles_x;
   for (uint32_t i = blockIdx.x * kSetupBlock + threadIdx.x; i < n; i += gridDim.x * kSetupBlock) {
      const uint32_t c = i / sd.num_tris, t = i - c * sd.num_tris, first = sd.rec_count[i];
      setup(sd, t, c, [&](int k, const SubTri& st) {
         const uint32_t r = first + (uint32_t)k;
         uint4* q = sd.records + 3 * (size_t)r;
         q[0] = make_uint4((uint32_t)st.X[0], (uint32_t)st.Y[0], (uint32_t)st.X[1], (uint32_t)st.Y[1]);
         q[1] = make_uint4((uint32_t)st.X[2], (uint32_t)st.Y[2], __float_as_uint(st.z[0]), __float_as_uint(st.z[1]));
         q[2] = make_uint4(__float_as_uint(st.z[2]), (uint32_t)st.x0 | ((uint32_t)st.x1 << 16), (uint32_t)st.y0 | ((uint32_t)st.y1 << 16), 0u);
         for_tiles(st, sd.tiles_x, [&](uint32_t tile) { sd.entries[atomicAdd(&sd.tile_cursor[c * tiles + tile], 1u)] = r; });
      });
   }
}

struct Rec {
   raster::Edges e;
   float z0, z1, z2;
   int x0, x1, y0, y1;
};
__device__ __forceinline__ Rec load_rec(const uint4* __restrict__ records, uint32_t r) {
   const uint4 a = records[3 * (size_t)r], b = records[3 * (size_t)r + 1], c = records[3 * (size_t)r + 2];
   Rec q;
   q.e = raster::make_edges((int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y);
   q.z0 = __uint_as_float(b.z), q.z1 = __uint_as_float(b.w), q.z2 = __uint_as_float(c.x);
   q.x0 = (int)(c.y & 0xffffu), q.x1 = (int)(c.y >> 16), q.y0 = (int)(c.z & 0xffffu), q.y1 = (int)(c.z >> 16);
   return q;
}
// texel (px, py): covered (raster::cover), then z from the integer barycentrics, kept when 0 <= z <= 1, -0 stored as +0
__device__ __forceinline__ void raster_texel(const Rec& q, int px, int py, uint32_t* tile_depth, int ox, int oy) {
   long long e0, e1, e2;
   if (!raster::cover(q.e, px, py, e0, e1, e2)) return;
   const float z = raster::depth_at(q.e, q.z0, q.z1, q.z2, e1, e2);
   if (!(z >= 0.0f && z <= 1.0f)) return;
   const uint32_t bits = z == 0.0f ? 0u : __float_as_uint(z);
   atomicMin(&tile_depth[(py - oy) * (int)kShadowTile + (px - ox)], bits);
}

__global__ __launch_bounds__(kResolveBlock) void k_shadow_resolve(ShadowDev sd) {
   __shared__ uint32_t s_depth[kShadowTile * kShadowTile];  // 64 KiB: two blocks per CU
   __shared__ uint32_t s_big[kResolveBlock];
   __shared__ uint32_t s_nbig;
   const uint32_t tile = blockIdx.x, c = blockIdx.y, tiles = sd.tiles_x * sd.tiles_x;
   const int ox = (int)((tile % sd.tiles_x) * kShadowTile), oy = (int)((tile / sd.tiles_x) * kShadowTile);
   const int S = (int)sd.size, tw = min((int)kShadowTile, S - ox), th = min((int)kShadowTile, S - oy);
   for (uint32_t i = threadIdx.x; i < kShadowTile * kShadowTile; i += kResolveBlock) s_depth[i] = kOne;
   if (threadIdx.x == 0) s_nbig = 0;
   __syncthreads();
   const uint32_t begin = sd.tile_count[c * tiles + tile], end = sd.tile_cursor[c * tiles + tile];
   for (uint32_t base = begin; base < end; base += kResolveBlock) {
      const uint32_t i = base + threadIdx.x;
      if (i < end) {
         const uint32_t r = sd.entries[i];
         const Rec q = load_rec(sd.records, r);
         const int x0 = max(q.x0, ox), x1 = min(q.x1, ox + tw - 1), y0 = max(q.y0, oy), y1 = min(q.y1, oy + th - 1);
         if ((x1 - x0 + 1) * (y1 - y0 + 1) <= kSmallPixels) {
            for (int py = y0; py <= y1; py++)
               for (int px = x0; px <= x1; px++) raster_texel(q, px, py, s_depth, ox, oy);
         } else {
            s_big[atomicAdd(&s_nbig, 1u)] = r;
         }
      }
      __syncthreads();
      const uint32_t nbig = s_nbig;
      for (uint32_t k = 0; k < nbig; k++) {  // the large boxes: the whole block strides over the box's texels in the tile
         const Rec q = load_rec(sd.records, s_big[k]);
         const int x0 = max(q.x0, ox), x1 = min(q.x1, ox + tw - 1), y0 = max(q.y0, oy), y1 = min(q.y1, oy + th - 1);
         const int w = x1 - x0 + 1, npx = w * (y1 - y0 + 1);
         for (int p = (int)threadIdx.x; p < npx; p += kResolveBlock) raster_texel(q, x0 + p % w, y0 + p / w, s_depth, ox, oy);
      }
      __syncthreads();
      if (threadIdx.x == 0) s_nbig = 0;
      __syncthreads();
   }
   float* out = sd.maps + (size_t)c * sd.size * sd.size;
   if ((S & 3) == 0) {  // every tile row starts and ends on a multiple of 4: 16-byte stores
      const int qw = tw >> 2;
      for (int i = (int)threadIdx.x; i < qw * th; i += kResolveBlock) {
         const int ly = i / qw, lx = (i - ly * qw) * 4;
         const uint32_t* s = s_depth + ly * (int)kShadowTile + lx;
         *reinterpret_cast<uint4*>(out + (size_t)(oy + ly) * S + ox + lx) = make_uint4(s[0], s[1], s[2], s[3]);
      }
   } else {
      for (int i = (int)threadIdx.x; i < tw * th; i += kResolveBlock) {
         const int ly = i / tw, lx = i - ly * tw;
         reinterpret_cast<uint32_t*>(out)[(size_t)(oy + ly) * S + ox + lx] = s_depth[ly * (int)kShadowTile + lx];
      }
   }
}

inline dim3 setup_grid(const LaunchCfg& c, uint32_t n) {
   const uint32_t blocks = (n + kSetupBlock - 1) / kSetupBlock, cap = c.num_cus * 8;
   return dim3(blocks < cap ? (blocks ? blocks : 1) : cap);
}
}  // namespace

void launch_shadow_count(const LaunchCfg& c, const ShadowDev& sd) {
   if (sd.num_tris) k_shadow_count<<<setup_grid(c, 4 * sd.num_tris), kSetupBlock, 0, c.stream>>>(sd);
}
void launch_shadow_emit(const LaunchCfg& c, const ShadowDev& sd) {
   if (sd.num_tris) k_shadow_emit<<<setup_grid(c, 4 * sd.num_tris), kSetupBlock, 0, c.stream>>>(sd);
}
void launch_shadow_resolve(const LaunchCfg& c, const ShadowDev& sd) {
   k_shadow_resolve<<<dim3(sd.tiles_x * sd.tiles_x, 4), kResolveBlock, 0, c.stream>>>(sd);
}

}  // namespace uh

// ---- setup_shadow_pass's host arithmetic (float32, no contraction; the order is DESIGN.md section 2's) ----
namespace {
struct M4 {
   float m[16];  // column-major: m[4 c + r]
};
struct V3f {
   float x, y, z;
};
V3f sub(V3f a, V3f b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3f add(V3f a, V3f b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3f mul(V3f a, float s) { return {a.x * s, a.y * s, a.z * s}; }
float dot(V3f a, V3f b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
V3f cross(V3f a, V3f b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
V3f normalize(V3f a) { return mul(a, 1.0f / std::sqrt(dot(a, a))); }
// a b: element (r, c) = ((a(r,0) b(0,c) + a(r,1) b(1,c)) + a(r,2) b(2,c)) + a(r,3) b(3,c)
M4 mat_mul(const M4& a, const M4& b) {
   M4 o;
   for (int c = 0; c < 4; c++)
      for (int r = 0; r < 4; r++)
         o.m[4 * c + r] = ((a.m[r] * b.m[4 * c] + a.m[4 + r] * b.m[4 * c + 1]) + a.m[8 + r] * b.m[4 * c + 2]) + a.m[12 + r] * b.m[4 * c + 3];
   return o;
}
// the GLM / glam scalar cofactor inverse; false when the determinant is 0
bool inverse(const M4& a, M4& out) {
   const float* m = a.m;
   auto e = [&](int c, int r) { return m[4 * c + r]; };
   const float m00 = e(0, 0), m01 = e(0, 1), m02 = e(0, 2), m03 = e(0, 3);
   const float m10 = e(1, 0), m11 = e(1, 1), m12 = e(1, 2), m13 = e(1, 3);
   const float m20 = e(2, 0), m21 = e(2, 1), m22 = e(2, 2), m23 = e(2, 3);
   const float m30 = e(3, 0), m31 = e(3, 1), m32 = e(3, 2), m33 = e(3, 3);
   const float c00 = m22 * m33 - m32 * m23, c02 = m12 * m33 - m32 * m13, c03 = m12 * m23 - m22 * m13;
   const float c04 = m21 * m33 - m31 * m23, c06 = m11 * m33 - m31 * m13, c07 = m11 * m23 - m21 * m13;
   const float c08 = m21 * m32 - m31 * m22, c10 = m11 * m32 - m31 * m12, c11 = m11 * m22 - m21 * m12;
   const float c12 = m20 * m33 - m30 * m23, c14 = m10 * m33 - m30 * m13, c15 = m10 * m23 - m20 * m13;
   const float c16 = m20 * m32 - m30 * m22, c18 = m10 * m32 - m30 * m12, c19 = m10 * m22 - m20 * m12;
   const float c20 = m20 * m31 - m30 * m21, c22 = m10 * m31 - m30 * m11, c23 = m10 * m21 - m20 * m11;
   const float f0[4] = {c00, c00, c02, c03}, f1[4] = {c04, c04, c06, c07}, f2[4] = {c08, c08, c10, c11};
   const float f3[4] = {c12, c12, c14, c15}, f4[4] = {c16, c16, c18, c19}, f5[4] = {c20, c20, c22, c23};
   const float v0[4] = {m10, m00, m00, m00}, v1[4] = {m11, m01, m01, m01}, v2[4] = {m12, m02, m02, m02}, v3[4] = {m13, m03, m03, m03};
   const float sa[4] = {1.0f, -1.0f, 1.0f, -1.0f}, sb[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
   M4 inv;
   for (int i = 0; i < 4; i++) {
      inv.m[i] = ((v1[i] * f0[i] - v2[i] * f1[i]) + v3[i] * f2[i]) * sa[i];
      inv.m[4 + i] = ((v0[i] * f0[i] - v2[i] * f3[i]) + v3[i] * f4[i]) * sb[i];
      inv.m[8 + i] = ((v0[i] * f1[i] - v1[i] * f3[i]) + v3[i] * f5[i]) * sa[i];
      inv.m[12 + i] = ((v0[i] * f2[i] - v1[i] * f4[i]) + v2[i] * f5[i]) * sb[i];
   }
   // det = dot(column 0 of a, row 0 of inv)
   const float det = ((m00 * inv.m[0] + m01 * inv.m[4]) + m02 * inv.m[8]) + m03 * inv.m[12];
   if (det == 0.0f || !std::isfinite(det)) return false;
   const float rcp = 1.0f / det;
   for (int i = 0; i < 16; i++) out.m[i] = inv.m[i] * rcp;
   return true;
}
}  // namespace

extern "C" int uh_shadow_cascades(const float view[16], const float projection[16], float z_near, float z_far, const float sun_dir[3],
                                  UhShadowmapParams* out) {
   if (!view || !projection || !sun_dir || !out) return UH_ERR_INVALID_ARGUMENT;
   for (int i = 0; i < 16; i++)
      if (!std::isfinite(view[i]) || !std::isfinite(projection[i])) return UH_ERR_INVALID_ARGUMENT;
   if (!std::isfinite(z_near) || !std::isfinite(z_far) || !(z_near > 0.0f) || !(z_far > z_near)) return UH_ERR_INVALID_ARGUMENT;
   const V3f sun = {sun_dir[0], sun_dir[1], sun_dir[2]};
   if (!std::isfinite(sun.x) || !std::isfinite(sun.y) || !std::isfinite(sun.z)) return UH_ERR_INVALID_ARGUMENT;
   if (sun.x == 0.0f && sun.z == 0.0f) return UH_ERR_INVALID_ARGUMENT;  // zero, or parallel to +Y: look_at_rh's side vector is 0
   const float near_clip = z_near, far_clip = z_far, clip_range = far_clip - near_clip;
   const float min_z = near_clip, max_z = near_clip + clip_range, range = max_z - min_z, ratio = max_z / min_z;
   const float lambda = 0.927f;
   float splits[4];
   for (int i = 0; i < 4; i++) {
      const float p = (float)(i + 1) / 4.0f;
      const float lg = min_z * (float)std::pow((double)ratio, (double)p);
      const float uniform = min_z + range * p;
      const float d = lambda * (lg - uniform) + uniform;
      splits[i] = (d - near_clip) / clip_range;
   }
   M4 V, P, inv_cam;
   std::memcpy(V.m, view, sizeof(V.m));
   std::memcpy(P.m, projection, sizeof(P.m));
   if (!inverse(mat_mul(P, V), inv_cam)) return UH_ERR_INVALID_ARGUMENT;
   UhShadowmapParams r;
   float last = 0.0f;
   for (int i = 0; i < 4; i++) {
      const float split = splits[i];
      const float cc[8][3] = {{-1, 1, 0}, {1, 1, 0}, {1, -1, 0}, {-1, -1, 0}, {-1, 1, 1}, {1, 1, 1}, {1, -1, 1}, {-1, -1, 1}};
      V3f corner[8];
      for (int k = 0; k < 8; k++) {
         float h[4];
         for (int row = 0; row < 4; row++)
            h[row] = ((inv_cam.m[row] * cc[k][0] + inv_cam.m[4 + row] * cc[k][1]) + inv_cam.m[8 + row] * cc[k][2]) + inv_cam.m[12 + row] * 1.0f;
         corner[k] = {h[0] / h[3], h[1] / h[3], h[2] / h[3]};
      }
      for (int k = 0; k < 4; k++) {
         const V3f dist = sub(corner[k + 4], corner[k]);
         corner[k + 4] = add(corner[k], mul(dist, split));
         corner[k] = add(corner[k], mul(dist, last));
      }
      V3f center = {0.0f, 0.0f, 0.0f};
      for (int k = 0; k < 8; k++) center = add(center, corner[k]);
      center = {center.x / 8.0f, center.y / 8.0f, center.z / 8.0f};
      float radius = 0.0f;
      for (int k = 0; k < 8; k++) radius = std::fmax(radius, std::sqrt(dot(sub(corner[k], center), sub(corner[k], center))));
      radius = std::ceil(radius * 16.0f) / 16.0f;
      // look_at_rh(center - sun * (-radius), center, +Y): f = normalize(eye - center), s = normalize(cross(up, f)), u = cross(f, s)
      const V3f eye = sub(center, mul(sun, -radius));
      const V3f f = normalize(sub(eye, center));
      const V3f s = normalize(cross(V3f{0.0f, 1.0f, 0.0f}, f));
      const V3f u = cross(f, s);
      M4 lv = {{s.x, u.x, f.x, 0.0f, s.y, u.y, f.y, 0.0f, s.z, u.z, f.z, 0.0f, -dot(s, eye), -dot(u, eye), -dot(f, eye), 1.0f}};
      // orthographic_rh(-r, r, -r, r, -2r, 2r)
      const float left = -radius, right = radius, bottom = -radius, top = radius, zn = -(radius - -radius), zf = radius - -radius;
      const float rw = 1.0f / (right - left), rh = 1.0f / (top - bottom), rz = 1.0f / (zn - zf);
      M4 ortho = {{rw + rw, 0.0f, 0.0f, 0.0f, 0.0f, rh + rh, 0.0f, 0.0f, 0.0f, 0.0f, rz, 0.0f, -(left + right) * rw, -(top + bottom) * rh, rz * zn, 1.0f}};
      const M4 vp = mat_mul(ortho, lv);
      std::memcpy(r.view_projection_matrices[i], vp.m, sizeof(vp.m));
      r.cascade_splits[i] = near_clip + split * clip_range;
      last = split;
   }
   for (int i = 0; i < 4; i++) {
      if (!std::isfinite(r.cascade_splits[i])) return UH_ERR_INVALID_ARGUMENT;
      for (int k = 0; k < 16; k++)
         if (!std::isfinite(r.view_projection_matrices[i][k])) return UH_ERR_INVALID_ARGUMENT;
   }
   *out = r;
   return UH_OK;
}
