// utopian_host.hpp — C++ host-side mirror of the reference's plugin surface for the path-tracing
// + ReSTIR path, layered on the C ABI of utopian_hip.h (header-only, C++17).
//
// The reference's host code is Rust; there is no Rust toolchain in the build image, so the host
// layer a Rust caller would write is provided in C++ with the same names and
// argument meaning:
//   utopian::Camera                    utopian/src/camera.rs:90-107 (look_at_rh / perspective_rh)
//   utopian::Material / Mesh / Model   utopian/src/gltf_loader.rs:11-45, primitive.rs:9-24
//   utopian::Renderer                  utopian/src/renderer.rs:123-412 (new, initialize, add_model,
//                                      add_light, get_num_lights) + Raytracing::initialize
//                                      (raytracing.rs:89) + rebuild_tlas (raytracing.rs:400)
//   utopian::Graph / build_path_tracing_render_graph
//                                      utopian/src/renderers/mod.rs:189-375: the same named passes in
//                                      the same order; each pass's render closure is one
//                                      uh_render_frame call with that pass's bit
//   utopian::Application               the per-frame protocol of prototype/src/main.rs:460-471,545-546
// Error behaviour: the reference panics on every failure (graph.rs:253, raytracing.rs:178); here a
// non-zero status throws utopian::Error carrying uh_last_error().
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "utopian_hip.h"

namespace utopian {

struct Error : std::runtime_error {
   int status;
   Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};

// ---- glam-like math (column-major Mat4, f32) ---------------------------------------------
struct Vec3 {
   float x = 0, y = 0, z = 0;
};
inline Vec3 operator-(Vec3 a, Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline Vec3 operator+(Vec3 a, Vec3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline float dot(Vec3 a, Vec3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline Vec3 cross(Vec3 a, Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline Vec3 normalize(Vec3 a) {
   float l = std::sqrt(dot(a, a));
   return {a.x / l, a.y / l, a.z / l};
}

struct Mat4 {
   float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // m[c*4 + r]
   float& at(int r, int c) { return m[c * 4 + r]; }
   float at(int r, int c) const { return m[c * 4 + r]; }
   static Mat4 identity() { return Mat4(); }
   static Mat4 from_diagonal(float a, float b, float c, float d) {
      Mat4 r;
      r.at(0, 0) = a;
      r.at(1, 1) = b;
      r.at(2, 2) = c;
      r.at(3, 3) = d;
      return r;
   }
   static Mat4 from_scale_translation(Vec3 s, Vec3 t) {
      Mat4 r;
      r.at(0, 0) = s.x;
      r.at(1, 1) = s.y;
      r.at(2, 2) = s.z;
      r.at(0, 3) = t.x;
      r.at(1, 3) = t.y;
      r.at(2, 3) = t.z;
      return r;
   }
   static Mat4 from_translation(Vec3 t) { return from_scale_translation({1, 1, 1}, t); }
   // glam Mat4::look_at_rh
   static Mat4 look_at_rh(Vec3 eye, Vec3 center, Vec3 up) {
      Vec3 f = normalize(center - eye), s = normalize(cross(f, up)), u = cross(s, f);
      Mat4 r;
      r.at(0, 0) = s.x;
      r.at(0, 1) = s.y;
      r.at(0, 2) = s.z;
      r.at(1, 0) = u.x;
      r.at(1, 1) = u.y;
      r.at(1, 2) = u.z;
      r.at(2, 0) = -f.x;
      r.at(2, 1) = -f.y;
      r.at(2, 2) = -f.z;
      r.at(0, 3) = -dot(s, eye);
      r.at(1, 3) = -dot(u, eye);
      r.at(2, 3) = dot(f, eye);
      return r;
   }
   // glam Mat4::perspective_rh (depth 0..1)
   static Mat4 perspective_rh(float fov_y_radians, float aspect, float z_near, float z_far) {
      float h = std::cos(0.5f * fov_y_radians) / std::sin(0.5f * fov_y_radians);
      float w = h / aspect, r = z_far / (z_near - z_far);
      Mat4 p;
      std::memset(p.m, 0, sizeof(p.m));
      p.at(0, 0) = w;
      p.at(1, 1) = h;
      p.at(2, 2) = r;
      p.at(3, 2) = -1.0f;
      p.at(2, 3) = r * z_near;
      return p;
   }
   Mat4 operator*(const Mat4& b) const {
      Mat4 r;
      for (int c = 0; c < 4; c++)
         for (int rr = 0; rr < 4; rr++) {
            float s = 0;
            for (int k = 0; k < 4; k++) s += at(rr, k) * b.at(k, c);
            r.at(rr, c) = s;
         }
      return r;
   }
   Mat4 inverse() const {  // Gauss-Jordan in double
      double a[4][8];
      for (int r = 0; r < 4; r++)
         for (int c = 0; c < 4; c++) {
            a[r][c] = at(r, c);
            a[r][4 + c] = r == c ? 1.0 : 0.0;
         }
      for (int col = 0; col < 4; col++) {
         int piv = col;
         for (int r = col + 1; r < 4; r++)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
         for (int c = 0; c < 8; c++) std::swap(a[col][c], a[piv][c]);
         double d = a[col][col];
         for (int c = 0; c < 8; c++) a[col][c] /= d;
         for (int r = 0; r < 4; r++)
            if (r != col) {
               double f = a[r][col];
               for (int c = 0; c < 8; c++) a[r][c] -= f * a[col][c];
            }
      }
      Mat4 out;
      for (int r = 0; r < 4; r++)
         for (int c = 0; c < 4; c++) out.at(r, c) = (float)a[r][4 + c];
      return out;
   }
   // row-major 3x4 (VkTransformMatrixKHR layout) of the affine part
   std::array<float, 12> to_3x4() const {
      std::array<float, 12> r{};
      for (int rr = 0; rr < 3; rr++)
         for (int c = 0; c < 4; c++) r[rr * 4 + c] = at(rr, c);
      return r;
   }
};

// ---- camera.rs ----------------------------------------------------------------------------
class Camera {
  public:
   Camera(Vec3 pos, Vec3 target, float fov_degrees, float aspect_ratio, float z_near, float z_far)
       : pos_(pos), target_(target), fov_(fov_degrees), aspect_(aspect_ratio), near_(z_near), far_(z_far) {}
   void set_position_target(Vec3 pos, Vec3 target) {
      pos_ = pos;
      target_ = target;
   }
   Mat4 get_view() const { return Mat4::look_at_rh(pos_, target_, {0, 1, 0}); }
   Mat4 get_projection() const { return Mat4::perspective_rh(fov_ * 3.14159265358979323846f / 180.0f, aspect_, near_, far_); }
   Vec3 get_position() const { return pos_; }
   float get_near_plane() const { return near_; }
   float get_far_plane() const { return far_; }

  private:
   Vec3 pos_, target_;
   float fov_, aspect_, near_, far_;
};

// ---- gltf_loader.rs / primitive.rs --------------------------------------------------------
using Vertex = UhVertex;
using ViewUniformData = UhViewUniformData;
using Reservoir = UhReservoir;
constexpr uint32_t DEFAULT_TEXTURE_MAP = 0xffffffffu;  // gltf_loader.rs:9
enum class MaterialType : uint32_t { Lambertian = 0, Metal = 1, Dielectric = 2, DiffuseLight = 3, CookTorrance = 4 /* extension, utopian_hip.h */ };

struct Texture {
   uint32_t width = 0, height = 0;
   std::vector<uint8_t> rgba;
};
struct Material {
   uint32_t diffuse_map = DEFAULT_TEXTURE_MAP;
   float base_color_factor[4] = {1, 1, 1, 1};
   float metallic_factor = 1.0f, roughness_factor = 1.0f;
   MaterialType material_type = MaterialType::Lambertian;
   float material_property = 0.0f;  // metal -> fuzz, dielectric -> index of refraction
};
struct Primitive {
   std::vector<Vertex> vertices;
   std::vector<uint32_t> indices;
};
struct Mesh {
   Primitive primitive;
   Material material;
   uint32_t gpu_mesh = 0;
};
struct Model {
   std::vector<Mesh> meshes;
   std::vector<Mat4> transforms;  // one per mesh (node transforms flattened, gltf_loader.rs:47-63)
   std::vector<Texture> textures;
};
struct ModelInstance {
   Model model;
   Mat4 transform;
};

// ---- renderer.rs + raytracing.rs ------------------------------------------------------------
// UH_HYBRID_TAA's sub-pixel jitter: `view` moved by (jx, jy) pixels of a width x height frame in G-buffer pixel coordinates (x right, y
// down). Its perspective projection gets -2 jx / width on element 8 and +2 jy / height on element 9 (ndc = clip.xy / -z), and
// inverse_projection the inverse of that; prev_frame_projection_view - which the caller has set to the previous frame's UN-jittered
// projection * view - gets the same offset in clip space (rows 0 and 1 less the offset times row 3), so that a camera at rest reprojects
// every pixel onto its own texel. The caller keeps the un-jittered projection * view of `view` for the next frame.
inline UhViewUniformData jitter_view(const UhViewUniformData& view, float jx, float jy, uint32_t width, uint32_t height) {
   UhViewUniformData v = view;
   const float dx = -2.0f * jx / (float)width, dy = 2.0f * jy / (float)height;
   v.projection[8] = v.projection[8] + dx;
   v.projection[9] = v.projection[9] + dy;
   Mat4 p;
   std::memcpy(p.m, v.projection, sizeof(p.m));
   const Mat4 inv = p.inverse();
   std::memcpy(v.inverse_projection, inv.m, sizeof(inv.m));
   for (int c = 0; c < 4; c++) {
      float* col = v.prev_frame_projection_view + 4 * c;
      col[0] = col[0] - dx * col[3];
      col[1] = col[1] - dy * col[3];
   }
   return v;
}

class Renderer {
  public:
   Renderer(int device_ordinal, uint32_t width, uint32_t height) : width_(width), height_(height) {
      int st = uh_create(device_ordinal, width, height, &ctx_);
      if (st != UH_OK) throw Error(st, std::string("Renderer::new: ") + uh_last_error(nullptr));
   }
   ~Renderer() { uh_destroy(ctx_); }
   Renderer(const Renderer&) = delete;
   Renderer& operator=(const Renderer&) = delete;

   // Renderer::initialize (renderer.rs:202-220): default 1x1 maps
   void initialize() {
      const uint8_t white[4] = {255, 255, 255, 255};
      check(uh_add_texture_rgba8(ctx_, white, 1, 1, &default_diffuse_map_index_), "initialize");
   }
   uint32_t add_bindless_texture(const Texture& t) {
      uint32_t idx = 0;
      check(uh_add_texture_rgba8(ctx_, t.rgba.data(), t.width, t.height, &idx), "add_bindless_texture");
      return idx;
   }
   // Renderer::add_model (renderer.rs:222-299): bindless remap of the diffuse map, one GpuMesh per mesh
   void add_model(Model model, const Mat4& transform) {
      std::vector<uint32_t> remap(model.textures.size(), DEFAULT_TEXTURE_MAP);
      for (size_t i = 0; i < model.meshes.size(); i++) {
         Mesh& mesh = model.meshes[i];
         UhGpuMaterial gm;
         std::memset(&gm, 0, sizeof(gm));
         if (mesh.material.diffuse_map == DEFAULT_TEXTURE_MAP) {
            gm.diffuse_map = default_diffuse_map_index_;
         } else {
            uint32_t& slot = remap.at(mesh.material.diffuse_map);
            if (slot == DEFAULT_TEXTURE_MAP) slot = add_bindless_texture(model.textures[mesh.material.diffuse_map]);
            gm.diffuse_map = slot;
         }
         std::memcpy(gm.base_color_factor, mesh.material.base_color_factor, sizeof(gm.base_color_factor));
         gm.metallic_factor = mesh.material.metallic_factor;
         gm.roughness_factor = mesh.material.roughness_factor;
         gm.raytrace_properties[0] = (float)(uint32_t)mesh.material.material_type;
         gm.raytrace_properties[1] = mesh.material.material_property;
         Mat4 world = transform * (i < model.transforms.size() ? model.transforms[i] : Mat4::identity());
         auto w = world.to_3x4();
         check(uh_add_mesh(ctx_, mesh.primitive.vertices.data(), (uint32_t)mesh.primitive.vertices.size(), mesh.primitive.indices.data(),
                           (uint32_t)mesh.primitive.indices.size(), &gm, w.data(), &mesh.gpu_mesh),
               "add_model");
      }
      instances.push_back(ModelInstance{std::move(model), transform});
   }
   // Renderer::add_light (renderer.rs:391-410)
   uint32_t add_light(Vec3 position, Vec3 color, float range) {
      UhGpuLight l;
      std::memset(&l, 0, sizeof(l));
      l.color[0] = color.x;
      l.color[1] = color.y;
      l.color[2] = color.z;
      l.position[0] = position.x;
      l.position[1] = position.y;
      l.position[2] = position.z;
      l.range = range;
      l.attenuation[2] = 0.1f;
      l.light_type = 1.0f;
      l.intensity[0] = l.intensity[1] = l.intensity[2] = 1.0f;
      uint32_t idx = 0;
      check(uh_add_light(ctx_, &l, &idx), "add_light");
      return idx;
   }
   uint32_t get_num_lights() const {
      uint32_t n = 0;
      uh_get_num_lights(ctx_, &n);
      return n;
   }
   // Raytracing::initialize (raytracing.rs:89-111)
   void initialize_raytracing() { check(uh_build_acceleration(ctx_), "Raytracing::initialize"); }
   // gizmo edit + Raytracing::rebuild_tlas (raytracing.rs:400-459)
   void set_instance_transform(uint32_t gpu_mesh, const Mat4& world) {
      auto w = world.to_3x4();
      check(uh_set_instance_transform(ctx_, gpu_mesh, w.data()), "set_instance_transform");
   }
   void rebuild_tlas() { check(uh_refit_acceleration(ctx_), "Raytracing::rebuild_tlas"); }

   std::vector<float> read_accumulation() {
      std::vector<float> out((size_t)width_ * height_ * 4);
      check(uh_read_accumulation(ctx_, out.data()), "read_accumulation");
      return out;
   }
   std::vector<uint8_t> read_output_bgra8() {
      std::vector<uint8_t> out((size_t)width_ * height_ * 4);
      check(uh_read_output_bgra8(ctx_, out.data()), "read_output_bgra8");
      return out;
   }
   UhStats get_stats() {
      UhStats s;
      check(uh_get_stats(ctx_, &s), "get_stats");
      return s;
   }
   // the hybrid graph's ray-traced passes (build_render_graph, renderers/mod.rs:61-186): rt_shadows on the previous G-buffer, the
   // G-buffer pass, rt_reflections on the new one, then SSAO, deferred, sky and present - for the bits of `mask` (utopian_hip.h
   // "uh_render_hybrid")
   void render_hybrid(const UhViewUniformData& view, uint32_t mask = UH_HYBRID_ALL) { check(uh_render_hybrid(ctx_, &view, mask), "render_hybrid"); }
   // one image as bytes: W*H texels of 16 (position, normal, pbr, deferred output, the motion image of UH_HYBRID_MOTION), 4 (albedo, reflections, present output, the
   // marching-cubes and rasterised G-buffer depth floats and draw indices uint32), 2 (SSAO) or 1 (shadows, light visibility, the
   // occluded-ray counts of UH_HYBRID_RTAO) bytes; taa_output of UH_HYBRID_TAA 16, its history length 4; the radiance of UH_HYBRID_RTGI
   // 16, its four ray counts 4; the scale and bias images of UH_HYBRID_GLOSSY 16 each, its four ray counts 4; the mask of UH_HYBRID_FOG 4, its
   // terms 16
   std::vector<uint8_t> read_hybrid(int which) {
      const size_t texel = (which == UH_HYBRID_AO_COUNTS) ? 1
                           : (which == UH_HYBRID_SHADOWS || which == UH_HYBRID_LIGHT_VISIBILITY) ? 1
                           : (which == UH_HYBRID_SSAO_IMAGE) ? 2
                           : (which == UH_HYBRID_ALBEDO || which == UH_HYBRID_REFLECTIONS || which == UH_HYBRID_PRESENT_OUTPUT ||
                              which == UH_HYBRID_DEPTH || which == UH_HYBRID_MARCHING_CUBES_VISIBILITY || which == UH_HYBRID_GBUFFER_DEPTH ||
                              which == UH_HYBRID_GBUFFER_VISIBILITY || which == UH_HYBRID_TAA_HISTORY || which == UH_HYBRID_GI_COUNTS ||
                              which == UH_HYBRID_GLOSSY_COUNTS || which == UH_HYBRID_FOG_MASK || which == UH_HYBRID_GLASS_COUNTS ||
                              which == UH_HYBRID_GLASS_EVENTS || which == UH_HYBRID_AREA_COUNTS) ? 4
                                                                     : 16;  // (UH_HYBRID_MOTION_IMAGE and UH_HYBRID_TAA_OUTPUT among them)
      static_assert(UH_HYBRID_MOTION_IMAGE == 15, "read_hybrid sizes image 15 as 16-byte texels");
      std::vector<uint8_t> out((size_t)width_ * height_ * texel);
      check(uh_read_hybrid(ctx_, which, out.data()), "read_hybrid");
      return out;
   }
   UhHybridStats hybrid_stats() {
      UhHybridStats s;
      check(uh_get_hybrid_stats(ctx_, &s), "hybrid_stats");
      return s;
   }
   // pass_ms of all seven passes of the last render_hybrid (bit order), with UH_HYBRID_FRAME = 0x7f the whole final frame
   UhHybridFrameStats hybrid_frame_stats() {
      UhHybridFrameStats s;
      check(uh_get_hybrid_frame_stats(ctx_, &s), "hybrid_frame_stats");
      return s;
   }
   // the last marching-cubes pass (UH_HYBRID_MARCHING_CUBES with view.marching_cubes_enabled == 1; utopian_hip.h)
   UhMarchingCubesStats marching_cubes_stats() {
      UhMarchingCubesStats s;
      check(uh_get_marching_cubes_stats(ctx_, &s), "marching_cubes_stats");
      return s;
   }
   // the last rasterised G-buffer pass (UH_HYBRID_GBUFFER | UH_HYBRID_GBUFFER_RASTER; utopian_hip.h)
   UhGbufferRasterStats gbuffer_raster_stats() {
      UhGbufferRasterStats s;
      check(uh_get_gbuffer_raster_stats(ctx_, &s), "gbuffer_raster_stats");
      return s;
   }
   // the last call with UH_HYBRID_RESTIR_LIGHTS: rays cast toward the reservoirs' lights, the occluded ones, the pass's time (utopian_hip.h)
   UhHybridRestirStats hybrid_restir_stats() {
      UhHybridRestirStats s;
      check(uh_get_hybrid_restir_stats(ctx_, &s), "hybrid_restir_stats");
      return s;
   }
   // ray-traced ambient occlusion in the SSAO slot of render_hybrid (UH_HYBRID_RTAO; utopian_hip.h): the params of the calls that
   // follow, and the last pass's pixels, rays, occluded rays and times
   static UhRtaoParams default_rtao_params() {
      UhRtaoParams p;
      if (uh_rtao_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_rtao_default_params");
      return p;
   }
   void set_rtao_params(const UhRtaoParams& params) { check(uh_set_rtao_params(ctx_, &params), "set_rtao_params"); }
   UhRtaoStats rtao_stats() {
      UhRtaoStats s;
      check(uh_get_rtao_stats(ctx_, &s), "rtao_stats");
      return s;
   }
   // one-bounce ray-traced diffuse GI behind the deferred pass of render_hybrid (UH_HYBRID_RTGI; utopian_hip.h): the params of the calls
   // that follow, and the last pass's pixels, rays, sun rays, misses and times
   static UhRtgiParams default_rtgi_params() {
      UhRtgiParams p;
      if (uh_rtgi_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_rtgi_default_params");
      return p;
   }
   void set_rtgi_params(const UhRtgiParams& params) { check(uh_set_rtgi_params(ctx_, &params), "set_rtgi_params"); }
   UhRtgiStats rtgi_stats() {
      UhRtgiStats s;
      check(uh_get_rtgi_stats(ctx_, &s), "rtgi_stats");
      return s;
   }
   // ray-traced glossy reflections behind the rtgi pass of render_hybrid (UH_HYBRID_GLOSSY; utopian_hip.h): the params of the calls that
   // follow, and the last pass's pixels, rays, below samples, sun rays, misses and times
   static UhGlossyParams default_glossy_params() {
      UhGlossyParams p;
      if (uh_glossy_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_glossy_default_params");
      return p;
   }
   void set_glossy_params(const UhGlossyParams& params) { check(uh_set_glossy_params(ctx_, &params), "set_glossy_params"); }
   UhGlossyStats glossy_stats() {
      UhGlossyStats s;
      check(uh_get_glossy_stats(ctx_, &s), "glossy_stats");
      return s;
   }
   // ray-traced glass behind the glossy pass of render_hybrid (UH_HYBRID_GLASS; utopian_hip.h): the params of the calls that follow, and the
   // last pass's pixels, chains, segments, events, TIR events, cut chains, sun rays, misses and times; its images through read_hybrid: the
   // radiance 16 bytes a texel, the counts and the events 4 each
   static UhGlassParams default_glass_params() {
      UhGlassParams p;
      if (uh_glass_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_glass_default_params");
      return p;
   }
   void set_glass_params(const UhGlassParams& params) { check(uh_set_glass_params(ctx_, &params), "set_glass_params"); }
   UhGlassStats glass_stats() {
      UhGlassStats s;
      check(uh_get_glass_stats(ctx_, &s), "glass_stats");
      return s;
   }
   // emissive meshes as area lights directly behind the deferred pass of render_hybrid (UH_HYBRID_AREA_LIGHTS; utopian_hip.h): the params of
   // the calls that follow, and the last pass's pixels, samples, shadow rays, emitter table figures and times; its images through
   // read_hybrid: the two means 16 bytes a texel, the counts 4
   static UhAreaLightParams default_area_light_params() {
      UhAreaLightParams p;
      if (uh_area_light_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_area_light_default_params");
      return p;
   }
   void set_area_light_params(const UhAreaLightParams& params) { check(uh_set_area_light_params(ctx_, &params), "set_area_light_params"); }
   UhAreaLightStats area_light_stats() {
      UhAreaLightStats s;
      check(uh_get_area_light_stats(ctx_, &s), "area_light_stats");
      return s;
   }
   // the emitter table of the last area-light pass in slot order: keys (mesh << 22 | prim), areas and integer weights
   struct AreaEmitters {
      std::vector<uint32_t> keys;
      std::vector<float> areas;
      std::vector<uint32_t> weights;
   };
   AreaEmitters read_area_emitters() {
      uint32_t n = 0;
      check(uh_read_area_emitters(ctx_, 0, nullptr, nullptr, nullptr, &n), "read_area_emitters");
      AreaEmitters e{std::vector<uint32_t>(n), std::vector<float>(n), std::vector<uint32_t>(n)};
      if (n) check(uh_read_area_emitters(ctx_, n, e.keys.data(), e.areas.data(), e.weights.data(), &n), "read_area_emitters");
      return e;
   }
   // volumetric fog behind the sky pass of render_hybrid (UH_HYBRID_FOG; utopian_hip.h): the params of the calls that follow, the last
   // pass's pixels, rays, lit rays and times, and with option "count_visits" its walks' node visits and triangle tests
   static UhFogParams default_fog_params() {
      UhFogParams p;
      if (uh_fog_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_fog_default_params");
      return p;
   }
   void set_fog_params(const UhFogParams& params) { check(uh_set_fog_params(ctx_, &params), "set_fog_params"); }
   UhFogStats fog_stats() {
      UhFogStats s;
      check(uh_get_fog_stats(ctx_, &s), "fog_stats");
      return s;
   }
   std::pair<uint64_t, uint64_t> fog_visits() {
      uint64_t nodes = 0, tris = 0;
      check(uh_get_fog_visits(ctx_, &nodes, &tris), "fog_visits");
      return {nodes, tris};
   }
   // motion vectors (UH_HYBRID_GBUFFER | UH_HYBRID_MOTION; utopian_hip.h "motion vectors"): the last motion pass's pixels with and
   // without a correspondence, its meshes per state, and the times of the motion kernel and of the snapshot behind it
   UhMotionStats motion_stats() {
      UhMotionStats s;
      check(uh_get_motion_stats(ctx_, &s), "motion_stats");
      return s;
   }
   // temporal anti-aliasing between the sky pass and present of render_hybrid (UH_HYBRID_TAA; utopian_hip.h "temporal anti-aliasing"):
   // the params of the calls that follow, a camera cut, the last pass's pixels and time, and the jitter of frame `index` in pixels
   static UhTaaParams default_taa_params() {
      UhTaaParams p;
      if (uh_taa_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_taa_default_params");
      return p;
   }
   void set_taa_params(const UhTaaParams& params) { check(uh_set_taa_params(ctx_, &params), "set_taa_params"); }
   void reset_taa_history() { check(uh_reset_taa_history(ctx_), "reset_taa_history"); }
   UhTaaStats taa_stats() {
      UhTaaStats s;
      check(uh_get_taa_stats(ctx_, &s), "taa_stats");
      return s;
   }
   // the HDR display chain between the taa pass and present of render_hybrid (UH_HYBRID_POST; utopian_hip.h "HDR display chain"): the
   // params of the passes that follow, a camera cut, the last pass's record and times, its images (post_output and the bloom levels
   // as float RGBA, the histogram as 256 uint32 - all as bytes), a level's size, and the chain on a caller's W*H*4 float image
   static UhPostParams default_post_params() {
      UhPostParams p;
      if (uh_post_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_post_default_params");
      return p;
   }
   void set_post_params(const UhPostParams& params) { check(uh_set_post_params(ctx_, &params), "set_post_params"); }
   void reset_post_exposure() { check(uh_reset_post_exposure(ctx_), "reset_post_exposure"); }
   UhPostStats post_stats() {
      UhPostStats s;
      check(uh_get_post_stats(ctx_, &s), "post_stats");
      return s;
   }
   std::pair<uint32_t, uint32_t> post_level_size(uint32_t level) const {
      uint32_t w = 0, h = 0;
      if (uh_post_level_size(width_, height_, level, &w, &h) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_post_level_size: no such level");
      return {w, h};
   }
   void post_image(const float* rgba32f) { check(uh_post_image(ctx_, rgba32f), "post_image"); }
   std::vector<uint8_t> read_post(int which, int level = 0) {
      size_t bytes = 256 * sizeof(uint32_t);
      if (which != UH_POST_HISTOGRAM) {
         const auto wh = post_level_size(which == UH_POST_OUTPUT ? 0u : (uint32_t)level);
         bytes = (size_t)wh.first * wh.second * 16;
      }
      std::vector<uint8_t> out(bytes);
      check(uh_read_post(ctx_, which, level, out.data()), "read_post");
      return out;
   }
   // `view` jittered by uh_taa_jitter(index) pixels of this renderer's frame (jitter_view, above): set its prev_frame_projection_view to
   // the previous frame's UN-jittered projection * view first, and keep this frame's un-jittered product for the next
   UhViewUniformData jittered(const UhViewUniformData& view, uint32_t index) const {
      float j[2];
      if (uh_taa_jitter(index, j) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_taa_jitter");
      return jitter_view(view, j[0], j[1], width_, height_);
   }
   // the denoiser (utopian_hip.h "the denoiser"): the accumulation of the last render_frame over the G-buffer of the last render_hybrid,
   // both rendered with view's camera by the caller; view.prev_frame_projection_view is projection * view of the previous call
   static UhDenoiseParams default_denoise_params() {
      UhDenoiseParams p;
      if (uh_denoise_default_params(&p) != UH_OK) throw Error(UH_ERR_INVALID_ARGUMENT, "uh_denoise_default_params");
      return p;
   }
   void denoise(const UhViewUniformData& view, const UhDenoiseParams& params) { check(uh_denoise(ctx_, &view, &params), "denoise"); }
   void denoise(const UhViewUniformData& view) { denoise(view, default_denoise_params()); }
   // one image of the last denoise as bytes: W*H texels of 16 (colour, input, temporal colour) or 4 (the 8-bit output, history, variance) bytes
   std::vector<uint8_t> read_denoised(int which) {
      const size_t texel = (which == UH_DENOISE_OUTPUT || which == UH_DENOISE_HISTORY || which == UH_DENOISE_VARIANCE) ? 4 : 16;
      std::vector<uint8_t> out((size_t)width_ * height_ * texel);
      check(uh_read_denoised(ctx_, which, out.data()), "read_denoised");
      return out;
   }
   void reset_denoise_history() { check(uh_reset_denoise_history(ctx_), "reset_denoise_history"); }
   UhDenoiseStats denoise_stats() {
      UhDenoiseStats s;
      check(uh_get_denoise_stats(ctx_, &s), "denoise_stats");
      return s;
   }
   // one face and mip of an IBL map built with UH_HYBRID_ENVIRONMENT (utopian_hip.h "uh_read_environment"): (512 >> mip)^2 texels of
   // 4 floats for the cubes, 512^2 pairs of IEEE half floats (as uint16_t bits) for the BRDF LUT
   std::vector<float> read_environment(int which, int face = 0, int mip = 0) {
      const size_t s = (size_t)UH_ENV_SIZE >> mip;
      std::vector<float> out(which == UH_ENV_BRDF_LUT ? (size_t)UH_BRDF_LUT_SIZE * UH_BRDF_LUT_SIZE : s * s * 4);
      check(uh_read_environment(ctx_, which, face, mip, out.data()), "read_environment");
      return out;
   }
   // pass_ms of the last build's four sub-passes (environment, irradiance, specular, BRDF LUT), the builds so far, its sun and eye
   UhEnvironmentStats environment_stats() {
      UhEnvironmentStats s;
      check(uh_get_environment_stats(ctx_, &s), "environment_stats");
      return s;
   }
   // the cascaded shadow maps (utopian_hip.h "UH_HYBRID_SHADOW_MAPS"): the params the next render uses, one layer (size^2 depths,
   // row 0 at NDC y = +1) and the last render's stats
   void set_shadowmap_params(const UhShadowmapParams& params) { check(uh_set_shadowmap_params(ctx_, &params), "set_shadowmap_params"); }
   std::vector<float> read_shadow_map(int cascade) {
      const UhShadowMapStats s = shadow_map_stats();
      std::vector<float> out((size_t)s.size * s.size);
      check(uh_read_shadow_map(ctx_, cascade, out.data()), "read_shadow_map");
      return out;
   }
   UhShadowMapStats shadow_map_stats() {
      UhShadowMapStats s;
      check(uh_get_shadow_map_stats(ctx_, &s), "shadow_map_stats");
      return s;
   }
   // the forward graph (build_minimal_forward_render_graph, the reference's render mode 3; utopian_hip.h "uh_render_forward"): shadow
   // maps, forward pass and present for the bits of `mask`; one image as bytes, W*H texels of 16 (output), 4 (depth float, draw index
   // uint32, present B G R A) bytes, row 0 at NDC y = +1; the last call's stats
   void render_forward(const UhViewUniformData& view, uint32_t mask = UH_FORWARD_GRAPH) { check(uh_render_forward(ctx_, &view, mask), "render_forward"); }
   std::vector<uint8_t> read_forward(int which) {
      std::vector<uint8_t> out((size_t)width_ * height_ * (which == UH_FORWARD_OUTPUT ? 16 : 4));
      check(uh_read_forward(ctx_, which, out.data()), "read_forward");
      return out;
   }
   UhForwardStats forward_stats() {
      UhForwardStats s;
      check(uh_get_forward_stats(ctx_, &s), "forward_stats");
      return s;
   }
   // uh_set_option: "device_build", "frames_in_flight", ... (DESIGN.md "Options")
   void set_option(const char* name, int value) { check(uh_set_option(ctx_, name, value), name); }
   // marching_cubes.rs:17-83 / marching_cubes.comp: the density field's iso-surface, extracted on the GPU and added
   // as a mesh of the scene; returns the triangle count (0: nothing crosses the iso value, no mesh added)
   uint32_t add_isosurface_mesh(uint32_t resolution, float lo, float hi, float time, const Material& material, const Mat4& world = Mat4::identity()) {
      UhGpuMaterial m;
      std::memset(&m, 0, sizeof(m));
      m.diffuse_map = default_diffuse_map_index_;
      std::memcpy(m.base_color_factor, material.base_color_factor, sizeof(m.base_color_factor));
      m.metallic_factor = material.metallic_factor;
      m.roughness_factor = material.roughness_factor;
      m.raytrace_properties[0] = (float)(uint32_t)material.material_type;
      m.raytrace_properties[1] = material.material_property;
      auto w = world.to_3x4();
      uint32_t mesh = 0, tris = 0;
      check(uh_add_isosurface_mesh(ctx_, resolution, lo, hi, time, &m, w.data(), &mesh, &tris), "add_isosurface_mesh");
      return tris;
   }
   // uh_update_isosurface_mesh: the field at another time as mesh `mesh`'s geometry, on the device; returns the triangle count.
   // build_acceleration() has to follow
   uint32_t update_isosurface_mesh(uint32_t mesh, float time) {
      uint32_t tris = 0;
      check(uh_update_isosurface_mesh(ctx_, mesh, time, &tris), "update_isosurface_mesh");
      return tris;
   }
   UhIsosurfaceUpdateStats isosurface_update_stats() {
      UhIsosurfaceUpdateStats s;
      check(uh_get_isosurface_update_stats(ctx_, &s), "isosurface_update_stats");
      return s;
   }
   // uh_update_mesh_vertices: new vertices for a mesh of add_mesh (its count of them; the index list stays), from the host or from
   // device memory the caller has finished writing (where = UH_VERTICES_DEVICE). rebuild_tlas(), a frame with
   // view.rebuild_tlas = 1 or initialize_raytracing() has to follow
   void update_mesh_vertices(uint32_t mesh, const UhVertex* vertices, uint32_t num_vertices, int where = UH_VERTICES_HOST) {
      check(uh_update_mesh_vertices(ctx_, mesh, vertices, num_vertices, where), "update_mesh_vertices");
   }
   UhMeshUpdateStats mesh_update_stats() {
      UhMeshUpdateStats s;
      check(uh_get_mesh_update_stats(ctx_, &s), "mesh_update_stats");
      return s;
   }
   // posed meshes: a skin (four joints and weights per vertex) and / or morph targets (deltas target-major) on a mesh of add_mesh, its
   // current vertices the bind pose; pose_mesh then writes the mesh's vertices on the device from the call's joint matrices (3x4 row-major,
   // 12 floats each) and morph weights - null / 0 for a part the mesh does not have - and leaves the state of
   // update_mesh_vertices(UH_VERTICES_DEVICE): rebuild_tlas() or a frame with view.rebuild_tlas = 1 follows
   void set_mesh_skin(uint32_t mesh, const uint16_t* joints, const float* weights, uint32_t num_vertices, uint32_t num_joints) {
      check(uh_set_mesh_skin(ctx_, mesh, joints, weights, num_vertices, num_joints), "set_mesh_skin");
   }
   void set_mesh_morph_targets(uint32_t mesh, const float* position_deltas, const float* normal_deltas, uint32_t num_vertices, uint32_t num_targets) {
      check(uh_set_mesh_morph_targets(ctx_, mesh, position_deltas, normal_deltas, num_vertices, num_targets), "set_mesh_morph_targets");
   }
   void pose_mesh(uint32_t mesh, const float* joint_matrices3x4, uint32_t num_joints, const float* morph_weights = nullptr, uint32_t num_targets = 0) {
      check(uh_pose_mesh(ctx_, mesh, joint_matrices3x4, num_joints, morph_weights, num_targets), "pose_mesh");
   }
   UhPoseStats pose_stats() {
      UhPoseStats s;
      check(uh_get_pose_stats(ctx_, &s), "pose_stats");
      return s;
   }
   // ---- one process per GPU (the reference is single-device: utopian/src/device.rs:45) ----
   // path tracing: tiles t % world == rank; reservoir passes: this rank's band of rows, exchanged over RCCL inside the library
   // (rank 0 makes the id, the launcher hands the 128 bytes to every rank); composition on the root: compose_tiles
   void set_tile_partition(uint32_t rank, uint32_t world, uint32_t tile_size = 64) { check(uh_set_tile_partition(ctx_, rank, world, tile_size), "set_tile_partition"); }
   static std::array<uint8_t, 128> rccl_unique_id() {
      std::array<uint8_t, 128> id{};
      if (uh_rccl_unique_id(id.data()) != UH_OK) throw Error(UH_ERR_HIP, "uh_rccl_unique_id: librccl is not loadable");
      return id;
   }
   void rccl_attach(uint32_t rank, uint32_t world, const std::array<uint8_t, 128>& id) { check(uh_rccl_attach(ctx_, rank, world, id.data()), "rccl_attach"); }
   void set_restir_partition(uint32_t rank, uint32_t world, UhRestirExchangeFn exchange = nullptr, void* user = nullptr) {
      check(uh_set_restir_partition(ctx_, rank, world, exchange, user), "set_restir_partition");
   }
   void pack_tiles(void* device_out, uint64_t capacity_pixels) { check(uh_pack_tiles(ctx_, device_out, capacity_pixels), "pack_tiles"); }
   void compose_tiles(const void* device_all, uint64_t stride_pixels, uint32_t total_samples, uint32_t accumulation_limit = 999999) {
      check(uh_compose_tiles(ctx_, device_all, stride_pixels, total_samples, accumulation_limit), "compose_tiles");
   }
   uh_ctx* handle() { return ctx_; }
   uint32_t width() const { return width_; }
   uint32_t height() const { return height_; }
   void check(int st, const char* where) {
      if (st != UH_OK) throw Error(st, std::string(where) + ": " + uh_last_error(ctx_));
   }

   std::vector<ModelInstance> instances;

  private:
   uh_ctx* ctx_ = nullptr;
   uint32_t width_, height_;
   uint32_t default_diffuse_map_index_ = 0;
};

// ---- graph.rs (only what the path-tracing recipe needs) -------------------------------------
struct RenderPass {
   std::string name;
   std::function<void(Renderer&, const ViewUniformData&)> render_func;  // graph.rs:126-127
};
class Graph {
  public:
   void clear() { passes.clear(); }
   void add_pass(std::string name, std::function<void(Renderer&, const ViewUniformData&)> f) { passes.push_back({std::move(name), std::move(f)}); }
   // Graph::render (graph.rs:703-1065): passes in submission order on the single render thread
   void render(Renderer& renderer, const ViewUniformData& view) {
      for (auto& p : passes) p.render_func(renderer, view);
   }
   std::vector<RenderPass> passes;
};

// renderers::build_path_tracing_render_graph (renderers/mod.rs:189-375): same pass names, same order
inline void build_path_tracing_render_graph(Graph& graph) {
   auto node = [](uint32_t mask) {
      return [mask](Renderer& r, const ViewUniformData& v) { r.check(uh_render_frame(r.handle(), &v, mask), "render_func"); };
   };
   graph.add_pass("gbuffer_pass", node(UH_PASS_GBUFFER));
   graph.add_pass("reset_reservoirs_pass", node(UH_PASS_RESET_RESERVOIRS));
   graph.add_pass("initial_ris_pass", node(UH_PASS_INITIAL_RIS));
   graph.add_pass("temporal_reuse_pass", node(UH_PASS_TEMPORAL_REUSE));
   graph.add_pass("spatial_reuse_pass", node(UH_PASS_SPATIAL_REUSE));
   graph.add_pass("reference_pt_pass", node(UH_PASS_REFERENCE_PT));
}

// ---- prototype/src/main.rs: view defaults (:55-86) and the frame protocol (:460-471, :545-546) ----
// setup_shadow_pass (shadow.rs) for the camera's own near / far planes: uh_shadow_cascades, host arithmetic only
inline UhShadowmapParams shadow_cascades(const Camera& camera, Vec3 sun_dir) {
   UhShadowmapParams p;
   const float sun[3] = {sun_dir.x, sun_dir.y, sun_dir.z};
   const int st = uh_shadow_cascades(camera.get_view().m, camera.get_projection().m, camera.get_near_plane(), camera.get_far_plane(), sun, &p);
   if (st != UH_OK) throw Error(st, "shadow_cascades: degenerate camera or sun direction");
   return p;
}

inline ViewUniformData default_view_data(const Camera& camera, uint32_t width, uint32_t height) {
   ViewUniformData v;
   std::memset(&v, 0, sizeof(v));
   Mat4 view = camera.get_view(), proj = camera.get_projection(), iv = view.inverse(), ip = proj.inverse();
   Mat4 prev = Mat4::from_diagonal(-1, -1, -1, -1);
   std::memcpy(v.view, view.m, 64);
   std::memcpy(v.projection, proj.m, 64);
   std::memcpy(v.inverse_view, iv.m, 64);
   std::memcpy(v.inverse_projection, ip.m, 64);
   std::memcpy(v.prev_frame_projection_view, prev.m, 64);
   Vec3 e = camera.get_position();
   v.eye_pos[0] = e.x;
   v.eye_pos[1] = e.y;
   v.eye_pos[2] = e.z;
   v.samples_per_frame = 1;
   v.total_samples = 0;
   v.num_bounces = 5;
   v.viewport_width = width;
   v.viewport_height = height;
   Vec3 sun = normalize({0.0f, 0.9f, 0.15f});
   v.sun_dir[0] = sun.x;
   v.sun_dir[1] = sun.y;
   v.sun_dir[2] = sun.z;
   v.shadows_enabled = v.ssao_enabled = v.fxaa_enabled = v.cubemap_enabled = v.ibl_enabled = 1;
   v.sky_enabled = v.sun_shadow_enabled = v.lights_enabled = 1;
   v.max_num_lights_used = 10000;
   v.temporal_reuse_enabled = v.spatial_reuse_enabled = 1;
   v.rebuild_tlas = 0;
   v.accumulation_limit = 999999;
   v.use_ris_light_sampling = 1;
   v.raytracing_supported = 1;
   return v;
}

class Application {
  public:
   Application(Renderer& renderer, const Camera& camera) : renderer_(renderer), view_data(default_view_data(camera, renderer.width(), renderer.height())) {
      build_path_tracing_render_graph(graph);
   }
   void frame() {
      view_data.total_samples += view_data.samples_per_frame;  // main.rs:467-469, BEFORE the frame
      view_data.num_lights = renderer_.get_num_lights();        // main.rs:471
      graph.render(renderer_, view_data);
      Mat4 proj, view;
      std::memcpy(proj.m, view_data.projection, 64);
      std::memcpy(view.m, view_data.view, 64);
      Mat4 pv = proj * view;                                    // main.rs:545-546, AFTER the frame
      std::memcpy(view_data.prev_frame_projection_view, pv.m, 64);
   }
   // `count` frames of a static camera, handed to the library in one call (uh_render_frames batches frames into shared
   // wavefronts and keeps several in flight). With the reservoir passes the first frame goes through the graph alone: it is
   // the one that may still see another prev_frame_projection_view (main.rs:545-546 sets it AFTER a frame).
   void frames(uint32_t count, bool path_tracing_only) {
      if (!path_tracing_only && count > 0) {
         frame();
         count--;
      }
      if (count < 2) {
         for (uint32_t i = 0; i < count; i++) frame();
         return;
      }
      view_data.num_lights = renderer_.get_num_lights();
      view_data.total_samples += view_data.samples_per_frame;
      renderer_.check(uh_render_frames(renderer_.handle(), &view_data, path_tracing_only ? UH_PASS_REFERENCE_PT : UH_PASS_ALL, count), "render_frames");
      view_data.total_samples += (count - 1) * view_data.samples_per_frame;
   }
   Graph graph;

  private:
   Renderer& renderer_;

  public:
   ViewUniformData view_data;
};

}  // namespace utopian
