// camera_grid_check.cpp - CPU proof of the camera grid (the structure behind every primary ray and the G-buffer cast of a camera at
// rest: reference.rgen:31-47, renderers/gbuffer.rs:11-52), run under ASan + UBSan. VERDICT r4 missing 4: the device builder had
// only ever been held against the tree walk on the GPU.
//
// The builder's arithmetic lives in csrc/camera_grid.h as host + device functions (pg_make_cam, pg_project_packet, sg_packet_edges,
// sg_cell_touches, sg_cell_of): the kernels of csrc/sun_grid_build.hip call them per packet / per cell, and this file calls THE
// SAME FUNCTIONS on the host, bins the packets the way k_sg_bin / k_sg_sort do, and then replays k_trace_camera_grid for rays in
// the kernels' float arithmetic (primary_ray of device_math.h, tri_compute<false> of traversal.h, restated with std::fmaf) against
// brute force over ALL packets. Three properties, each for every ray:
//   (1) listing     every packet whose float test accepts the ray (and whose padded box the ray meets: what a padded-box tree asks)
//                   is listed in the ray's pixel;
//   (2) bound       such a packet's sort key is a lower bound of the t the float test computes (-key <= t), so the walk's early exit
//                   ("the next bound exceeds the best hit") can neither skip the closest hit nor a tie with it;
//   (3) the walk    the hit record of the grid walk (t, u, v, packet; ties by key) equals brute force's, bit for bit.
// Rays: through every pixel's four corners (jitter 0 and 1: random_float can return exactly 1.0), edge midpoints and centre, plus
// random jitter. Cameras: inside the scene, the reference's Sponza-style view, from above, two centimetres above a floor, IN the
// plane of the floor, far outside, with packets behind and across the camera plane, a narrow and a wide field of view.
// Build: g++ -std=c++17 -O1 -ffp-contract=off -mfma -fsanitize=address,undefined -I rust-renderer_amd/csrc -I include tests/cpp/camera_grid_check.cpp
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "camera_grid.h"
#include "sun_grid.h"

using namespace uh;

static uint32_t rng_state = 0x2468aceu;
static float rnd() {
   rng_state = rng_state * 747796405u + 2891336453u;
   uint32_t w = ((rng_state >> ((rng_state >> 28) + 4u)) ^ rng_state) * 277803737u;
   w = (w >> 22) ^ w;
   return (float)w * 2.3283064365386963e-10f;
}

struct F3 {
   float x, y, z;
};
static float dot_fma(F3 a, F3 b) { return std::fmaf(a.z, b.z, std::fmaf(a.y, b.y, a.x * b.x)); }
static F3 cross_fma(F3 a, F3 b) { return F3{std::fmaf(a.y, b.z, -(a.z * b.y)), std::fmaf(a.z, b.x, -(a.x * b.z)), std::fmaf(a.x, b.y, -(a.y * b.x))}; }

struct Hit {
   float t, u, v;
   uint32_t idx, key;
};
static Hit no_hit() { return Hit{10000.0f, 0.0f, 0.0f, 0xffffffffu, 0xffffffffu}; }  // rgen:45: tmax

// tri_compute<ANY = false> of traversal.h (tmin 0.001): true when the packet ACCEPTS the ray (barycentrics and t > tmin); the best
// hit is updated as the kernel does (nearer t, ties by the smaller key)
static bool tri_compute(const float* q, uint32_t i, uint32_t key, F3 o, F3 d, Hit& best, float* t_out) {
   F3 v0{q[0], q[1], q[2]}, e1{q[3], q[4], q[5]}, e2{q[6], q[7], q[8]};
   F3 p = cross_fma(d, e2);
   float det = dot_fma(e1, p);
   if (det == 0.0f) return false;
   float inv = 1.0f / det;
   F3 tv{o.x - v0.x, o.y - v0.y, o.z - v0.z};
   float u = dot_fma(tv, p) * inv;
   if (!(u >= 0.0f && u <= 1.0f)) return false;
   F3 qq = cross_fma(tv, e1);
   float v = dot_fma(d, qq) * inv;
   if (!(v >= 0.0f && u + v <= 1.0f)) return false;
   float t = dot_fma(e2, qq) * inv;
   if (!(t > 0.001f)) return false;
   if (t_out) *t_out = t;
   if (t < best.t || (t == best.t && key < best.key)) best = Hit{t, u, v, i, key};
   return true;
}

// does the ray meet the packet's own padded box within (tmin, tmax)? What a padded-box tree asks before it tests a packet (padding
// and slab arithmetic of bvh_build.cpp / oracle.cpp): a ray lying IN the plane of an edge-on packet is accepted or rejected by
// rounding noise, and no tree - hence no reference - asks such a packet unless the ray meets its box.
static bool meets_box(const float* q, F3 o, F3 d) {
   float lo[3], hi[3];
   for (int a = 0; a < 3; a++) {
      const float c0 = q[a], c1 = q[a] + q[3 + a], c2 = q[a] + q[6 + a];
      float l = std::fmin(c0, std::fmin(c1, c2)), h = std::fmax(c0, std::fmax(c1, c2));
      const float pad = 1e-4f + 1e-5f * std::fmax(std::fabs(l), std::fabs(h));
      lo[a] = l - pad;
      hi[a] = h + pad;
   }
   const float id[3] = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z}, oo[3] = {o.x, o.y, o.z};
   float tn = 0.001f, tf = 10000.0f;
   for (int a = 0; a < 3; a++) {
      const float t0 = (lo[a] - oo[a]) * id[a], t1 = (hi[a] - oo[a]) * id[a];
      tn = std::fmax(tn, std::fmin(t0, t1));
      tf = std::fmin(tf, std::fmax(t0, t1));
   }
   return tn <= tf * 1.0000005f + 1e-30f;
}

// ---- the camera: matrices as the host mirrors hand them over (glam look_at_rh / perspective_rh 0..1, inverted; column-major
// floats), and primary_ray of device_math.h
struct Camera {
   float inv_view[16], inv_proj[16];
   uint32_t W, H;
};
static Camera make_camera(F3 eye, F3 target, F3 up, float fov_deg, uint32_t W, uint32_t H, float near = 0.01f, float far = 1000.0f) {
   Camera c{};
   c.W = W;
   c.H = H;
   auto nrm = [](double* v) {
      const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      for (int k = 0; k < 3; k++) v[k] /= l;
   };
   double f[3] = {(double)target.x - eye.x, (double)target.y - eye.y, (double)target.z - eye.z};
   nrm(f);
   double s[3] = {f[1] * up.z - f[2] * up.y, f[2] * up.x - f[0] * up.z, f[0] * up.y - f[1] * up.x};
   nrm(s);
   const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
   // inverse of look_at_rh: columns = right, up, -forward, eye
   const double cols[4][3] = {{s[0], s[1], s[2]}, {u[0], u[1], u[2]}, {-f[0], -f[1], -f[2]}, {eye.x, eye.y, eye.z}};
   for (int col = 0; col < 4; col++) {
      for (int r = 0; r < 3; r++) c.inv_view[4 * col + r] = (float)cols[col][r];
      c.inv_view[4 * col + 3] = col == 3 ? 1.0f : 0.0f;
   }
   // perspective_rh (depth 0..1): x' = x f / aspect, y' = y f, z' = A z + B, w' = -z with A = far / (near - far), B = near far / (near - far)
   const double ff = 1.0 / std::tan(0.5 * fov_deg * 3.14159265358979323846 / 180.0), aspect = (double)W / H;
   const double A = (double)far / ((double)near - far), B = (double)near * far / ((double)near - far);
   // its inverse: x = x' aspect / f, y = y' / f, z = -w', w = (z' + A w') / B
   c.inv_proj[0] = (float)(aspect / ff);
   c.inv_proj[5] = (float)(1.0 / ff);
   c.inv_proj[11] = (float)(1.0 / B);
   c.inv_proj[14] = -1.0f;
   c.inv_proj[15] = (float)(A / B);
   return c;
}
static void mat4_mul(const float* m, float x, float y, float z, float w, float out[4]) {
   out[0] = ((m[0] * x + m[4] * y) + m[8] * z) + m[12] * w;
   out[1] = ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * w;
   out[2] = ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w;
   out[3] = ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w;
}
static void primary_ray(const Camera& c, uint32_t px, uint32_t py, float jx, float jy, F3& org, F3& dir) {
   float cx = (float)px + jx, cy = (float)py + jy;
   float u = cx / (float)c.W, v = cy / (float)c.H;
   v = 1.0f - v;
   float dx = u * 2.0f - 1.0f, dy = v * 2.0f - 1.0f;
   float o4[4], tg[4], d4[4];
   mat4_mul(c.inv_view, 0.0f, 0.0f, 0.0f, 1.0f, o4);
   mat4_mul(c.inv_proj, dx, dy, 1.0f, 1.0f, tg);
   const float inv = 1.0f / std::sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2]);
   mat4_mul(c.inv_view, tg[0] * inv, tg[1] * inv, tg[2] * inv, 0.0f, d4);
   org = F3{o4[0], o4[1], o4[2]};
   dir = F3{d4[0], d4[1], d4[2]};
}

// ---- the grid, built on the host with the builder's own functions (build_grid_impl's camera branch: raster = the frame plus a
// border ring, u0 = v0 = -1, one cell per pixel; count, fill, sort of the lists a ray may walk with the early exit)
struct Grid {
   uint32_t nx = 0, ny = 0, max_walk = 48;
   std::vector<uint32_t> start;
   std::vector<SunGridEntry> entries;
   uint64_t used = 0, behind = 0;
};
static bool build_grid(const std::vector<float>& pk, const Camera& c, Grid& g, const char** why) {
   PgCam cam;
   if (!pg_make_cam(c.inv_view, c.inv_proj, c.W, c.H, cam, why)) return false;
   const uint32_t n = (uint32_t)(pk.size() / 12);
   std::vector<SgProj> pr(n);
   for (uint32_t i = 0; i < n; i++) pg_project_packet(&pk[12 * (size_t)i], cam, pr[i]);
   SgGrid sg{-1.0, -1.0, 1.0, c.W + 2, c.H + 2};
   g.nx = sg.nx;
   g.ny = sg.ny;
   const size_t ncell = (size_t)g.nx * g.ny;
   std::vector<std::vector<SunGridEntry>> lists(ncell);
   for (uint32_t i = 0; i < n; i++) {
      const SgProj& p = pr[i];
      if (!(p.flags & 1u)) {
         g.behind++;
         continue;
      }
      g.used++;
      const uint32_t ix0 = sg_cell_of(p.x0, sg.u0, sg.inv, sg.nx), ix1 = sg_cell_of(p.x1, sg.u0, sg.inv, sg.nx), iy0 = sg_cell_of(p.y0, sg.v0, sg.inv, sg.ny),
                     iy1 = sg_cell_of(p.y1, sg.v0, sg.inv, sg.ny);
      double nxe[3], nye[3], off[3], epad[3];
      const int ne = sg_packet_edges(p, nxe, nye, off, epad);
      const double cs = 1.0 / sg.inv;
      for (uint32_t iy = iy0; iy <= iy1; iy++)
         for (uint32_t ix = ix0; ix <= ix1; ix++) {
            const bool border = iy == 0 || iy == sg.ny - 1 || ix == 0 || ix == sg.nx - 1;
            bool in = true;
            if (!border) {
               const double cy0 = sg.v0 + iy * cs, cy1 = cy0 + cs, cx0 = sg.u0 + ix * cs, cx1 = cx0 + cs;
               bool inside = false;
               in = sg_cell_touches(ne, nxe, nye, off, epad, cx0, cx1, cy0, cy1, inside);
            }
            if (in) lists[(size_t)iy * g.nx + ix].push_back(SunGridEntry{i, p.wmax});
         }
   }
   g.start.assign(ncell + 1, 0);
   for (size_t cidx = 0; cidx < ncell; cidx++) {
      std::vector<SunGridEntry>& l = lists[cidx];
      const uint32_t ix = (uint32_t)(cidx % g.nx), iy = (uint32_t)(cidx / g.nx);
      const bool border = ix == 0 || iy == 0 || ix == g.nx - 1 || iy == g.ny - 1;
      if (!border && l.size() >= 2 && l.size() <= g.max_walk)  // k_sg_sort: by key descending (= distance bound ascending), ties by packet index
         std::sort(l.begin(), l.end(), [](const SunGridEntry& a, const SunGridEntry& b) { return a.wmax > b.wmax || (a.wmax == b.wmax && a.packet < b.packet); });
      g.start[cidx + 1] = g.start[cidx] + (uint32_t)l.size();
      g.entries.insert(g.entries.end(), l.begin(), l.end());
   }
   return true;
}

// k_trace_camera_grid for one ray (a list too long for the sorted walk is walked whole: the kernel's walk_whole / the G-buffer cast)
static Hit grid_walk(const Grid& g, const std::vector<float>& pk, uint32_t px, uint32_t py, F3 o, F3 d, uint64_t* tests) {
   const uint32_t cell = (py + 1) * g.nx + (px + 1);
   uint32_t e = g.start[cell];
   const uint32_t end = g.start[cell + 1];
   const bool sorted = end - e <= g.max_walk;
   Hit best = no_hit();
   for (; e < end; e++) {
      if (sorted && -g.entries[e].wmax > best.t) break;
      const uint32_t i = g.entries[e].packet;
      uint32_t key;
      std::memcpy(&key, &pk[12 * (size_t)i + 9], 4);
      (*tests)++;
      tri_compute(&pk[12 * (size_t)i], i, key, o, d, best, nullptr);
   }
   return best;
}

static void add_tri(std::vector<float>& pk, F3 a, F3 b, F3 c) {
   const uint32_t key = (uint32_t)(pk.size() / 12);
   float kf;
   std::memcpy(&kf, &key, 4);
   const float q[12] = {a.x, a.y, a.z, b.x - a.x, b.y - a.y, b.z - a.z, c.x - a.x, c.y - a.y, c.z - a.z, kf, 0, 0};
   pk.insert(pk.end(), q, q + 12);
}
static void add_quad(std::vector<float>& pk, F3 o, F3 ex, F3 ey, int nx, int ny) {
   for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
         auto at = [&](int a, int b) { return F3{o.x + ex.x * a / nx + ey.x * b / ny, o.y + ex.y * a / nx + ey.y * b / ny, o.z + ex.z * a / nx + ey.z * b / ny}; };
         add_tri(pk, at(i, j), at(i + 1, j), at(i + 1, j + 1));
         add_tri(pk, at(i, j), at(i + 1, j + 1), at(i, j + 1));
      }
}

// a small atrium: floor at y = 0 (exactly: a camera can stand IN its plane), walls, a ceiling with a hole, pillars, random clutter,
// slivers, a few huge and a few tiny triangles, coincident duplicates (exact ties in t)
static std::vector<float> make_scene(uint32_t seed, int clutter) {
   rng_state = seed;
   std::vector<float> pk;
   add_quad(pk, F3{-8, 0, -5}, F3{16, 0, 0}, F3{0, 0, 10}, 8, 6);           // floor
   add_quad(pk, F3{-8, 0, -5}, F3{16, 0, 0}, F3{0, 6, 0}, 8, 4);            // back wall
   add_quad(pk, F3{-8, 0, 5}, F3{0, 0, -10}, F3{0, 6, 0}, 6, 4);            // left wall
   add_quad(pk, F3{8, 0, -5}, F3{0, 0, 10}, F3{0, 6, 0}, 6, 4);             // right wall
   add_quad(pk, F3{-8, 6, -5}, F3{7, 0, 0}, F3{0, 0, 10}, 4, 4);            // ceiling, two parts with a gap
   add_quad(pk, F3{1, 6, -5}, F3{7, 0, 0}, F3{0, 0, 10}, 4, 4);
   for (int p = 0; p < 4; p++) {                                            // pillars
      const float x = -5.0f + 3.3f * p, z = -2.0f + (p & 1) * 3.0f;
      add_quad(pk, F3{x, 0, z}, F3{0.4f, 0, 0}, F3{0, 5.5f, 0}, 1, 5);
      add_quad(pk, F3{x + 0.4f, 0, z}, F3{0, 0, 0.4f}, F3{0, 5.5f, 0}, 1, 5);
      add_quad(pk, F3{x, 0, z + 0.4f}, F3{0.4f, 0, 0}, F3{0, 5.5f, 0}, 1, 5);
      add_quad(pk, F3{x, 0, z}, F3{0, 0, 0.4f}, F3{0, 5.5f, 0}, 1, 5);
   }
   for (int k = 0; k < clutter; k++) {
      const F3 c{rnd() * 14 - 7, rnd() * 5 + 0.2f, rnd() * 8 - 4};
      const float s = k % 17 == 0 ? 2.5f : (k % 5 == 0 ? 0.02f : 0.35f);
      F3 v[3];
      for (auto& p : v) p = F3{c.x + (rnd() - 0.5f) * s, c.y + (rnd() - 0.5f) * s, c.z + (rnd() - 0.5f) * s};
      if (k % 11 == 0) v[2] = F3{v[0].x + (v[1].x - v[0].x) * 0.5f + 1e-5f, v[0].y + (v[1].y - v[0].y) * 0.5f, v[0].z + (v[1].z - v[0].z) * 0.5f};  // sliver
      add_tri(pk, v[0], v[1], v[2]);
      if (k % 23 == 0) add_tri(pk, v[0], v[1], v[2]);  // coincident duplicate: a tie in t, decided by the key
   }
   add_tri(pk, F3{-300, -0.5f, -300}, F3{300, -0.5f, -300}, F3{0, -0.5f, 400});  // a huge ground triangle below the floor
   add_tri(pk, F3{0.1f, 1.0f, 0.1f}, F3{0.1f + 1e-4f, 1.0f, 0.1f}, F3{0.1f, 1.0f + 1e-4f, 0.1f});  // tiny
   add_tri(pk, F3{1, 1, 1}, F3{1, 1, 1}, F3{2, 1, 1});                      // degenerate (a line)
   add_tri(pk, F3{NAN, 0, 0}, F3{1, 0, 0}, F3{0, 1, 0});                    // non-finite
   return pk;
}

struct Totals {
   uint64_t rays = 0, hits = 0, accepted_pairs = 0, grid_tests = 0, brute_tests = 0;
   uint64_t not_listed = 0, bound_broken = 0, hit_differs = 0;
};

static int check_camera(const char* name, const std::vector<float>& pk, const Camera& c, Totals& tot, bool expect_refusal = false) {
   Grid g;
   const char* why = "";
   if (!build_grid(pk, c, g, &why)) {
      std::printf("%-34s refused: %s%s\n", name, why, expect_refusal ? " (expected)" : "");
      return expect_refusal ? 0 : 1;
   }
   if (expect_refusal) {
      std::printf("%-34s built, but a refusal was expected\n", name);
      return 1;
   }
   const uint32_t n = (uint32_t)(pk.size() / 12);
   Totals t;
   const float js[9][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {0.5f, 0}, {0, 0.5f}, {1, 0.5f}, {0.5f, 1}, {0.5f, 0.5f}};
   std::vector<uint8_t> listed(n);
   for (uint32_t py = 0; py < c.H; py++)
      for (uint32_t px = 0; px < c.W; px++) {
         const uint32_t cell = (py + 1) * g.nx + (px + 1);
         std::fill(listed.begin(), listed.end(), 0);
         for (uint32_t e = g.start[cell]; e < g.start[cell + 1]; e++) listed[g.entries[e].packet] = 1;
         for (int s = 0; s < 11; s++) {
            const float jx = s < 9 ? js[s][0] : rnd(), jy = s < 9 ? js[s][1] : rnd();
            F3 o, d;
            primary_ray(c, px, py, jx, jy, o, d);
            Hit want = no_hit();
            for (uint32_t i = 0; i < n; i++) {
               const float* q = &pk[12 * (size_t)i];
               uint32_t key;
               std::memcpy(&key, &q[9], 4);
               Hit scratch = no_hit();
               float tt = 0.0f;
               t.brute_tests++;
               if (!tri_compute(q, i, key, o, d, scratch, &tt)) continue;
               if (!meets_box(q, o, d)) continue;  // (an edge-on packet accepting a ray by rounding noise: no tree asks it)
               t.accepted_pairs++;
               if (tt < 10000.0f) tri_compute(q, i, key, o, d, want, nullptr);
               if (!listed[i]) {
                  if (t.not_listed++ < 5) std::printf("   NOT LISTED: packet %u accepts the ray of pixel (%u, %u) jitter (%g, %g) at t = %g\n", i, px, py, jx, jy, tt);
                  continue;
               }
               for (uint32_t e = g.start[cell]; e < g.start[cell + 1]; e++)
                  if (g.entries[e].packet == i && -g.entries[e].wmax > tt) {
                     if (t.bound_broken++ < 5) std::printf("   BOUND: packet %u pixel (%u, %u): bound %g above the float t %g\n", i, px, py, -g.entries[e].wmax, tt);
                  }
            }
            const Hit got = grid_walk(g, pk, px, py, o, d, &t.grid_tests);
            t.rays++;
            t.hits += want.idx != 0xffffffffu;
            if (std::memcmp(&got, &want, sizeof(Hit)) != 0) {
               if (t.hit_differs++ < 5)
                  std::printf("   HIT DIFFERS: pixel (%u, %u) jitter (%g, %g): grid t %g packet %u, brute force t %g packet %u\n", px, py, jx, jy, got.t, got.idx, want.t, want.idx);
            }
         }
      }
   const bool bad = t.not_listed || t.bound_broken || t.hit_differs;
   std::printf("%-34s %ux%u, %u packets (%llu listed, %llu behind): %llu rays, %llu hit, %llu accepted pairs, %.2f grid tests per ray (brute force %u), %zu entries  %s\n", name, c.W, c.H, n,
               (unsigned long long)g.used, (unsigned long long)g.behind, (unsigned long long)t.rays, (unsigned long long)t.hits, (unsigned long long)t.accepted_pairs,
               (double)t.grid_tests / (double)t.rays, n, g.entries.size(), bad ? "FAILED" : "ok");
   tot.rays += t.rays;
   tot.hits += t.hits;
   tot.accepted_pairs += t.accepted_pairs;
   tot.not_listed += t.not_listed;
   tot.bound_broken += t.bound_broken;
   tot.hit_differs += t.hit_differs;
   return bad ? 1 : 0;
}

int main(int argc, char** argv) {
   const int clutter = argc > 1 ? std::atoi(argv[1]) : 700;
   const uint32_t W = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 40, H = argc > 3 ? (uint32_t)std::atoi(argv[3]) : 26;
   int errors = 0;
   Totals tot;
   const std::vector<float> scene = make_scene(99, clutter);
   const F3 up{0, 1, 0};
   errors += check_camera("inside, towards the back wall", scene, make_camera(F3{0.3f, 2.1f, 3.6f}, F3{0, 1.5f, -5}, up, 60, W, H), tot);
   errors += check_camera("the reference's Sponza-style view", scene, make_camera(F3{-7.2f, 2.1f, -0.18f}, F3{0, 0.5f, 0}, up, 60, W, H), tot);
   errors += check_camera("from above, looking down", scene, make_camera(F3{0.1f, 5.5f, 0.2f}, F3{0.3f, 0, 0.1f}, F3{0, 0, -1}, 75, W, H), tot);
   errors += check_camera("two centimetres above the floor", scene, make_camera(F3{-6, 0.02f, 4}, F3{6, 0.5f, -4}, up, 60, W, H), tot);
   errors += check_camera("IN the plane of the floor", scene, make_camera(F3{-6, 0.0f, 4}, F3{6, 0.0f, -4}, up, 60, W, H), tot);
   errors += check_camera("far outside (packets in a few pixels)", scene, make_camera(F3{60, 25, 80}, F3{0, 2, 0}, up, 35, W, H), tot);
   errors += check_camera("narrow field of view, odd frame", scene, make_camera(F3{2, 3, 4.5f}, F3{-3, 1, -4}, up, 20, W + 3, H - 5), tot);
   errors += check_camera("wide field of view, scene behind too", scene, make_camera(F3{0, 2.5f, 0}, F3{5, 2.0f, 1}, up, 120, W, H), tot);
   errors += check_camera("on round coordinates, axis-aligned", scene, make_camera(F3{0, 3, 0}, F3{0, 3, -5}, up, 90, W, H), tot);
   {  // a second, smaller scene: other random clutter, a camera touching a pillar
      const std::vector<float> s2 = make_scene(7, clutter / 2);
      errors += check_camera("second scene, against a pillar", s2, make_camera(F3{-4.6f, 1.0f, -1.79f}, F3{-4.0f, 1.5f, 3}, up, 70, W, H), tot);
   }
   {  // matrices the grid must refuse instead of dividing by nothing
      Camera bad = make_camera(F3{0, 1, 0}, F3{0, 1, -1}, up, 60, W, H);
      bad.inv_view[5] = NAN;
      errors += check_camera("non-finite matrices", scene, bad, tot, true);
      Camera flat = make_camera(F3{0, 1, 0}, F3{0, 1, -1}, up, 60, W, H);
      for (int k = 0; k < 16; k++) flat.inv_proj[k] = 0.0f;
      errors += check_camera("a projection of rank 0", scene, flat, tot, true);
   }
   std::printf("camera grid against brute force: %llu rays, %llu hit, %llu accepted (ray, packet) pairs: %llu not listed, %llu bounds above t, %llu hit records differ: %s\n",
               (unsigned long long)tot.rays, (unsigned long long)tot.hits, (unsigned long long)tot.accepted_pairs, (unsigned long long)tot.not_listed, (unsigned long long)tot.bound_broken,
               (unsigned long long)tot.hit_differs, errors ? "FAILED" : "ok");
   return errors ? 1 : 0;
}
