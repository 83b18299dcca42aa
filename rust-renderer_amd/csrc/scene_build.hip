// scene_build.hip — the scene's geometry and the trees over it: uh_add_mesh and the instance transforms, the host builder
// (uh_build_acceleration; bvh_build.cpp), the on-device builders (option "device_build"; lbvh.hip) with their per-triangle sources,
// the refit (uh_refit_acceleration; refit.hip), and the device-resident meshes of uh_update_isosurface_mesh and uh_update_mesh_vertices
// (deform.hip) with the mesh read-backs.
// Host-side counterpart of Renderer::add_model (utopian/src/renderer.rs) and utopian::Raytracing (utopian/src/raytracing.rs).
// Host code only; struct uh_ctx is context_state.h, the rest of the C ABI is context.hip and the graphs (*_graph.hip).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "bvh.h"
#include "bvh_invariants.h"
#include "context_internal.h"
#include "context_state.h"
#include "device_scan.h"
#include "device_types.h"
#include "utopian_hip.h"

using namespace uh;

namespace {

bool is_identity3x4(const float* m) {
   static const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
   return std::memcmp(m, I, sizeof(I)) == 0;
}

// inverse of the upper 3x3 of a row-major 3x4 by cofactors (arithmetic contract: cofactor * (1/det))
void invert3x3(const float* m, float* inv) {
   float a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
   float A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
   float det = (a * A + b * B) + c * C;
   float id = 1.0f / det;
   inv[0] = A * id;
   inv[1] = -(b * i - c * h) * id;
   inv[2] = (b * f - c * e) * id;
   inv[3] = B * id;
   inv[4] = (a * i - c * g) * id;
   inv[5] = -(a * f - c * d) * id;
   inv[6] = C * id;
   inv[7] = -(a * h - b * g) * id;
   inv[8] = (a * e - b * d) * id;
}

void set_transform(HostMesh& m, const float* w) {
   std::memcpy(m.o2w, w, sizeof(m.o2w));
   if (is_identity3x4(w)) {
      static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      std::memcpy(m.w2o, I, sizeof(I));
   } else {
      invert3x3(w, m.w2o);
   }
}

}  // namespace

extern "C" {

int uh_add_mesh(uh_ctx* c, const UhVertex* vertices, uint32_t num_vertices, const uint32_t* indices, uint32_t num_indices,
                const UhGpuMaterial* material, const float world3x4[12], uint32_t* out_mesh_index) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!vertices || !indices || !material || !world3x4 || num_indices % 3 != 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_add_mesh: null argument or index count not a multiple of 3");
   if (c->meshes.size() >= UH_MAX_GPU_MESHES) return fail(c, UH_ERR_CAPACITY, "uh_add_mesh: more than 1024 meshes (MAX_NUM_GPU_MESHES)");
   if (num_indices / 3 > (1u << kPrimBits)) return fail(c, UH_ERR_CAPACITY, "uh_add_mesh: more than 4 Mi triangles in one mesh");
   for (uint32_t i = 0; i < num_indices; i++)
      if (indices[i] >= num_vertices) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_add_mesh: index out of range");
   for (uint32_t i = 0; i < num_vertices; i++)
      if (!std::isfinite(vertices[i].pos[0]) || !std::isfinite(vertices[i].pos[1]) || !std::isfinite(vertices[i].pos[2]))
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_add_mesh: vertex position is not finite");
   for (int i = 0; i < 12; i++)
      if (!std::isfinite(world3x4[i])) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_add_mesh: transform is not finite");
   HostMesh m;
   m.vertices.assign(vertices, vertices + num_vertices);
   m.indices.assign(indices, indices + num_indices);
   m.material = *material;
   set_transform(m, world3x4);
   c->meshes.push_back(std::move(m));
   c->built = false;
   c->topology_valid = false;
   c->src_valid = false;
   if (out_mesh_index) *out_mesh_index = (uint32_t)c->meshes.size() - 1;
   return UH_OK;
}

int uh_set_instance_transform(uh_ctx* c, uint32_t mesh_index, const float world3x4[12]) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (mesh_index >= c->meshes.size() || !world3x4) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_instance_transform: bad mesh index");
   for (int i = 0; i < 12; i++)
      if (!std::isfinite(world3x4[i])) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_instance_transform: transform is not finite");
   set_transform(c->meshes[mesh_index], world3x4);
   c->built = false;
   return UH_OK;
}

// per-mesh shading records, light table, texture descriptors: everything of the scene except the geometry
static int upload_scene_tables(uh_ctx* c) {
   std::vector<MeshShade> ms(c->meshes.size());
   for (size_t i = 0; i < c->meshes.size(); i++) {
      const HostMesh& m = c->meshes[i];
      std::memcpy(ms[i].w2o, m.w2o, sizeof(m.w2o));
      ms[i].diffuse_map = m.material.diffuse_map;
      for (int a = 0; a < 3; a++) ms[i].base_color[a] = m.material.base_color_factor[a];
      ms[i].type = m.material.raytrace_properties[0];
      ms[i].property = m.material.raytrace_properties[1];
      ms[i].pad = 0;
      ms[i].metallic = m.material.metallic_factor;
      ms[i].roughness = m.material.roughness_factor;
      ms[i].pad2[0] = ms[i].pad2[1] = 0.0f;
   }
   std::vector<float4> lights(2 * c->lights.size());
   for (size_t i = 0; i < c->lights.size(); i++) {
      const UhGpuLight& l = c->lights[i];
      lights[2 * i] = make_float4(l.position[0], l.position[1], l.position[2], 0.0f);
      lights[2 * i + 1] = make_float4(l.intensity[0], l.intensity[1], l.intensity[2], 0.0f);
   }
   std::vector<TexInfo> tex(c->textures.size());
   for (size_t i = 0; i < tex.size(); i++) tex[i] = TexInfo{c->textures[i].dev, c->textures[i].w, c->textures[i].h, c->textures[i].tiles_x, c->textures[i].blocks_x};

   HIP_TRY(c, c->d_meshes.alloc(ms.size()));
   HIP_TRY(c, c->d_lights.alloc(lights.size()));
   HIP_TRY(c, c->d_tex.alloc(tex.size()));
   if (!ms.empty()) HIP_TRY(c, hipMemcpy(c->d_meshes.p, ms.data(), ms.size() * sizeof(MeshShade), hipMemcpyHostToDevice));
   if (!lights.empty()) HIP_TRY(c, hipMemcpy(c->d_lights.p, lights.data(), lights.size() * sizeof(float4), hipMemcpyHostToDevice));
   if (!tex.empty()) HIP_TRY(c, hipMemcpy(c->d_tex.p, tex.data(), tex.size() * sizeof(TexInfo), hipMemcpyHostToDevice));
   c->scene.meshes = c->d_meshes.p;
   c->scene.textures = c->d_tex.p;
   c->scene.lights = c->d_lights.p;
   c->scene.unorm_lut = c->d_lut.p;
   c->scene.num_meshes = (uint32_t)ms.size();
   c->scene.num_textures = (uint32_t)tex.size();
   c->scene.num_lights = (uint32_t)c->lights.size();
   return UH_OK;
}

static int build_on_device(uh_ctx* c);

// the host builder and the host refit read HostMesh::vertices / indices: a device-resident mesh is copied back (once per update)
static int ensure_host_mirrors(uh_ctx* c) {
   for (HostMesh& m : c->meshes) {
      if (!m.dev || m.host_valid) continue;
      m.vertices.resize(3 * (size_t)m.dev_tris);
      m.indices.resize(m.vertices.size());
      if (m.dev_tris) {
         HIP_TRY(c, hipMemcpy(m.vertices.data(), m.d_verts, m.vertices.size() * sizeof(UhVertex), hipMemcpyDeviceToHost));  // blocking
         c->iso.st.host_geometry_bytes += m.vertices.size() * sizeof(UhVertex);
      }
      for (size_t i = 0; i < m.indices.size(); i++) m.indices[i] = (uint32_t)i;
      m.host_valid = true;
   }
   for (HostMesh& m : c->meshes) {
      if (!m.upd || m.host_valid) continue;  // (its last update took a device pointer: the index list is still the host's)
      HIP_TRY(c, hipMemcpy(m.vertices.data(), m.d_verts, m.vertices.size() * sizeof(UhVertex), hipMemcpyDeviceToHost));  // blocking
      c->mupd.st.host_geometry_bytes += m.vertices.size() * sizeof(UhVertex);
      m.host_valid = true;
   }
   return UH_OK;
}
// bytes per triangle of the device-resident meshes that a host-side assembly uploads (from their mirrors: a mesh without one is not in it)
static void count_host_upload(uh_ctx* c, size_t bytes_per_triangle) {
   for (const HostMesh& m : c->meshes) {
      if (m.dev) c->iso.st.host_geometry_bytes += bytes_per_triangle * m.dev_tris;
      if (m.upd && m.host_valid) c->mupd.st.host_geometry_bytes += bytes_per_triangle * m.tris();
   }
}

// triangle p of a host-resident mesh: its three vertices through the index list, its nine object-space corners, its shading packet
struct TriVerts { const UhVertex* v[3]; };
static TriVerts tri_verts(const HostMesh& m, uint32_t p) {
   const uint32_t* ix = &m.indices[3 * (size_t)p];
   return TriVerts{{&m.vertices[ix[0]], &m.vertices[ix[1]], &m.vertices[ix[2]]}};
}
static void write_obj_corners(const TriVerts& t, float* o) {
   for (int k = 0; k < 3; k++)
      for (int a = 0; a < 3; a++) o[3 * k + a] = t.v[k]->pos[a];
}
static void fill_shade_packet(const TriVerts& t, uint32_t mesh, ShadePacket& s) {
   for (int a = 0; a < 3; a++) {
      s.n0[a] = t.v[0]->normal[a];
      s.n1[a] = t.v[1]->normal[a];
      s.n2[a] = t.v[2]->normal[a];
   }
   for (int a = 0; a < 2; a++) {
      s.uv0[a] = t.v[0]->uv[a];
      s.uv1[a] = t.v[1]->uv[a];
      s.uv2[a] = t.v[2]->uv[a];
   }
   s.mesh = mesh;
}

// the scene's triangles; more than the keys and the traversal can address is refused
static int scene_triangles(uh_ctx* c, size_t* total) {
   *total = 0;
   for (const HostMesh& m : c->meshes) *total += m.tris();
   if (*total > kMaxTriangles) return fail(c, UH_ERR_CAPACITY, "scene has more than 2^31 - 2 triangles");
   return UH_OK;
}

// what refit.hip reads: a row per mesh, and the arrays of the tree in place
static std::vector<RefitMesh> refit_mesh_rows(uh_ctx* c) {
   std::vector<RefitMesh> rm(c->meshes.size());
   for (size_t i = 0; i < rm.size(); i++) {
      std::memset(&rm[i], 0, sizeof(RefitMesh));
      std::memcpy(rm[i].o2w, c->meshes[i].o2w, sizeof(rm[i].o2w));
      rm[i].identity = is_identity3x4(c->meshes[i].o2w) ? 1u : 0u;
   }
   return rm;
}
static RefitArgs refit_args(uh_ctx* c, size_t total) {
   RefitArgs a;
   a.obj_corners = c->d_obj_corners.p;
   a.meshes = c->d_refit_meshes.p;
   a.tris = c->d_tris.p;
   a.world_corners = c->d_world_corners.p;
   a.nodes = reinterpret_cast<uint4*>(c->d_nodes.p);
   a.node_box = c->d_node_box.p;
   a.level_start = c->level_start.data();
   a.num_levels = (uint32_t)c->level_start.size() - 1;
   a.num_tris = (uint32_t)total;
   return a;
}

// the common tail of the builders: the tree in d_nodes / d_tris / d_shade becomes the scene's
static void publish_tree(uh_ctx* c, uint32_t num_nodes, size_t total, std::chrono::steady_clock::time_point t0) {
   c->scene.nodes = reinterpret_cast<const uint4*>(c->d_nodes.p);
   c->scene.tris = c->d_tris.p;
   c->scene.shade = c->d_shade.p;
   c->scene.num_nodes = num_nodes;
   c->scene.num_tris = (uint32_t)total;
   c->bvh_nodes = c->scene.num_nodes;
   c->bvh_tris = c->scene.num_tris;
   c->geom_version++;
   c->topology_valid = true;
   c->built = true;
   c->packet_serial.resize(c->meshes.size());
   for (size_t i = 0; i < c->meshes.size(); i++) c->packet_serial[i] = c->meshes[i].serial;
   c->build_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int uh_build_acceleration(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   if (c->device_build) return build_on_device(c);
   auto t0 = std::chrono::steady_clock::now();
   if (int st = ensure_host_mirrors(c)) return st;
   // bake instance transforms: world = ((m0*x + m1*y) + m2*z) + m3 per row (identity: verbatim)
   size_t total = 0;
   if (int st = scene_triangles(c, &total)) return st;
   std::vector<float> corners(9 * total);
   std::vector<uint32_t> keys(total);
   size_t t = 0;
   for (uint32_t mi = 0; mi < c->meshes.size(); mi++) {
      const HostMesh& m = c->meshes[mi];
      const bool ident = is_identity3x4(m.o2w);
      const float* w = m.o2w;
      const uint32_t nt = (uint32_t)m.tris();
      for (uint32_t p = 0; p < nt; p++, t++) {
         float* o = &corners[9 * t];
         write_obj_corners(tri_verts(m, p), o);
         if (!ident)
            for (int k = 0; k < 3; k++, o += 3) {
               float x = o[0], y = o[1], z = o[2];
               o[0] = ((w[0] * x + w[1] * y) + w[2] * z) + w[3];
               o[1] = ((w[4] * x + w[5] * y) + w[6] * z) + w[7];
               o[2] = ((w[8] * x + w[9] * y) + w[10] * z) + w[11];
            }
         keys[t] = (mi << kPrimBits) | p;
      }
   }
   BuildInput in{corners.data(), keys.data(), (uint32_t)total};
   BuildOutput bo;
   int threads = (int)std::thread::hardware_concurrency();
   if (threads < 1) threads = 1;
   if (threads > 32) threads = 32;
   build_bvh4(in, bo, threads);
   if (bo.level_start.size() - 1 > kMaxTreeLevels) {
      // a tree deeper than the traversal stack holds (clustered / exponentially scaled geometry) would drop subtrees
      // silently: rebuild it balanced (median splits, depth ceil(log2 n) / 1..2 per 4-wide level)
      build_bvh4(in, bo, threads, true);
      if (bo.level_start.size() - 1 > kMaxTreeLevels) return fail(c, UH_ERR_CAPACITY, "internal: balanced BVH deeper than the traversal stack");
   }

   // packets in leaf order
   std::vector<TriPacket> tp(total);
   std::vector<ShadePacket> sp(total);
   for (size_t i = 0; i < total; i++) {
      uint32_t src = bo.tri_order[i];
      const float* cr = &corners[9 * (size_t)src];
      TriPacket& q = tp[i];
      q.v0[0] = cr[0];
      q.v0[1] = cr[1];
      q.v0[2] = cr[2];
      q.e1x = cr[3] - cr[0];
      q.e1yz[0] = cr[4] - cr[1];
      q.e1yz[1] = cr[5] - cr[2];
      q.e2[0] = cr[6] - cr[0];
      q.e2[1] = cr[7] - cr[1];
      q.e2z = cr[8] - cr[2];
      q.key = keys[src];
      q.pad[0] = q.pad[1] = 0;
      uint32_t mi = keys[src] >> kPrimBits, p = keys[src] & kPrimMask;
      fill_shade_packet(tri_verts(c->meshes[mi], p), mi, sp[i]);
   }
   if (bo.cnodes.empty()) return fail(c, UH_ERR_INVALID_ARGUMENT, "internal: BVH builder produced no root node");
   if (int st = sync_all(c)) return st;
   if (int st = upload_scene_tables(c)) return st;
   HIP_TRY(c, c->d_nodes.alloc(bo.cnodes.size() * kNodeStride16));
   HIP_TRY(c, c->d_tris.alloc(total * kTriStride16));
   HIP_TRY(c, c->d_shade.alloc(total * 4));
   // 48-byte records into arrays of stride kNodeStride16 / kTriStride16 x 16 bytes
   HIP_TRY(c, hipMemcpy2D(c->d_nodes.p, 16 * kNodeStride16, bo.cnodes.data(), sizeof(Node4C), sizeof(Node4C), bo.cnodes.size(), hipMemcpyHostToDevice));
   if (total) {
      HIP_TRY(c, hipMemcpy2D(c->d_tris.p, 16 * kTriStride16, tp.data(), sizeof(TriPacket), sizeof(TriPacket), total, hipMemcpyHostToDevice));
      HIP_TRY(c, hipMemcpy(c->d_shade.p, sp.data(), total * sizeof(ShadePacket), hipMemcpyHostToDevice));
      count_host_upload(c, sizeof(TriPacket) + sizeof(ShadePacket));
   }
   c->packet_keys.resize(total);
   for (size_t i = 0; i < total; i++) c->packet_keys[i] = tp[i].key;
   c->level_start = bo.level_start;
   c->d_obj_corners.release();  // leaf order changed: the next refit re-creates its inputs
   publish_tree(c, (uint32_t)bo.nodes.size(), total, t0);
   return UH_OK;
}

// Raytracing::rebuild_tlas (raytracing.rs:400-459) for a flattened tree: see refit.hip
int uh_refit_acceleration(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!c->topology_valid)
      return fail(c, UH_ERR_NOT_BUILT, "uh_refit_acceleration: meshes or lights were added since the last uh_build_acceleration (or it never ran)");
   HIP_TRY(c, hipSetDevice(c->device));
   auto t0 = std::chrono::steady_clock::now();
   if (int st = sync_all(c)) return st;  // frames in flight still traverse the old boxes
   const size_t total = c->packet_keys.size();
   // meshes whose vertices moved since the tree's packets were written (uh_update_mesh_vertices): k_deform_gather writes their
   // object-space corners and shade packets again, in leaf order, and the refit below bakes them like any other
   const bool fresh_corners = total && !c->d_obj_corners.p;
   std::vector<DeformMesh> dm(c->meshes.size());
   uint32_t moved_tris = 0;
   bool any_moved = false;
   for (size_t i = 0; i < dm.size(); i++) {
      const HostMesh& m = c->meshes[i];
      const bool moved = m.upd && m.tris() && (i >= c->packet_serial.size() || c->packet_serial[i] != m.serial || (fresh_corners && !m.host_valid));
      dm[i] = DeformMesh{moved ? m.d_verts : nullptr, moved ? m.d_indices : nullptr, moved ? 1u : 0u, 0u};
      if (moved) moved_tris += (uint32_t)m.tris();
      any_moved = any_moved || moved;
   }
   if (fresh_corners) {
      // (only the host builder leaves no d_obj_corners, and it has made the mirrors; a mesh updated from a device pointer since then
      // has none: its slots are the gather's)
      count_host_upload(c, 9 * sizeof(float));
      std::vector<float> oc(9 * total);
      for (size_t i = 0; i < total; i++) {
         const HostMesh& m = c->meshes[c->packet_keys[i] >> kPrimBits];
         if (!m.upd || m.host_valid) write_obj_corners(tri_verts(m, c->packet_keys[i] & kPrimMask), &oc[9 * i]);
      }
      HIP_TRY(c, c->d_obj_corners.alloc(9 * total));
      HIP_TRY(c, c->d_world_corners.alloc(9 * total));
      HIP_TRY(c, c->d_node_box.alloc(6 * (size_t)c->scene.num_nodes));
      HIP_TRY(c, c->d_refit_meshes.alloc(c->meshes.size()));
      HIP_TRY(c, hipMemcpy(c->d_obj_corners.p, oc.data(), oc.size() * sizeof(float), hipMemcpyHostToDevice));
   }
   const std::vector<RefitMesh> rm = refit_mesh_rows(c);
   std::vector<MeshShade> ms(c->meshes.size());
   HIP_TRY(c, hipMemcpy(ms.data(), c->d_meshes.p, ms.size() * sizeof(MeshShade), hipMemcpyDeviceToHost));
   for (size_t i = 0; i < c->meshes.size(); i++) std::memcpy(ms[i].w2o, c->meshes[i].w2o, sizeof(ms[i].w2o));
   if (!ms.empty()) HIP_TRY(c, hipMemcpy(c->d_meshes.p, ms.data(), ms.size() * sizeof(MeshShade), hipMemcpyHostToDevice));
   uh_ctx::MeshUpdate& u = c->mupd;
   if (total) {
      HIP_TRY(c, hipMemcpy(c->d_refit_meshes.p, rm.data(), rm.size() * sizeof(RefitMesh), hipMemcpyHostToDevice));
      if (any_moved) {
         if (u.table.n < dm.size()) HIP_TRY(c, u.table.alloc(dm.size()));
         HIP_TRY(c, hipMemcpy(u.table.p, dm.data(), dm.size() * sizeof(DeformMesh), hipMemcpyHostToDevice));
         HIP_TRY(c, hipEventRecord(u.ev[0], c->stream));
         launch_deform_gather(c->stream, u.table.p, (uint32_t)dm.size(), c->d_tris.p, c->d_obj_corners.p, c->d_shade.p, (uint32_t)total);
         HIP_TRY(c, hipEventRecord(u.ev[1], c->stream));
      }
      launch_refit(cfg(c), refit_args(c, total));
      if (any_moved) HIP_TRY(c, hipEventRecord(u.ev[2], c->stream));
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (any_moved) {
         HIP_TRY(c, hipEventElapsedTime(&u.st.gather_ms, u.ev[0], u.ev[1]));
         HIP_TRY(c, hipEventElapsedTime(&u.st.refit_ms, u.ev[1], u.ev[2]));
         u.st.triangles = moved_tris;
      }
   }
   c->packet_serial.resize(c->meshes.size());
   for (size_t i = 0; i < c->meshes.size(); i++) c->packet_serial[i] = c->meshes[i].serial;
   c->built = true;
   c->geom_version++;
   c->build_ms = c->refit_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
   return UH_OK;
}

// brackets of UhIsosurfaceUpdateStats::scatter_ms on the context's stream (the events exist once an update has run)
extern "C++" void iso_scatter_begin(uh_ctx* c) {
   if (c->iso.begin) (void)hipEventRecord(c->iso.begin, c->stream);
}
extern "C++" int iso_scatter_end(uh_ctx* c, bool add) {
   if (!c->iso.begin) return UH_OK;
   HIP_TRY(c, hipEventRecord(c->iso.end, c->stream));
   HIP_TRY(c, hipEventSynchronize(c->iso.end));
   float ms = 0.0f;
   HIP_TRY(c, hipEventElapsedTime(&ms, c->iso.begin, c->iso.end));
   c->iso.st.scatter_ms = add ? c->iso.st.scatter_ms + ms : ms;
   return UH_OK;
}

// ---- d_src (BuildSources): the on-device build's per-triangle sources in mesh order. Host-resident meshes are assembled on the
// host and uploaded when the mesh list has changed (src_valid); a device-resident mesh's range is written by k_iso_scatter from its
// device vertices whenever its serial has moved, and the ranges of the meshes that did not change are then copied on the device.
// `at`: the first triangle of each mesh's range in the layout being made, the total behind the last ----

static int sources_fail(uh_ctx* c, hipError_t e, const char* what) {
   return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string("build sources: ") + what + ": " + hipGetErrorString(e));
}

// f(i, j) for every maximal run [i, j) of mesh indices on which pred holds, until one fails
static hipError_t for_each_run(size_t nm, const std::function<bool(size_t)>& pred, const std::function<hipError_t(size_t, size_t)>& f) {
   for (size_t i = 0, j = 0; i < nm; i = j > i ? j : i + 1) {
      for (j = i; j < nm && pred(j);) j++;
      const hipError_t e = j > i ? f(i, j) : hipSuccess;  // (j == i: mesh i is outside every run)
      if (e != hipSuccess) return e;
   }
   return hipSuccess;
}

// new arrays; the host-resident meshes assembled on the host, one upload per run of them (the whole array when no mesh is
// device-resident)
static int upload_host_sources(uh_ctx* c, const std::vector<size_t>& at) {
   const size_t nm = c->meshes.size(), total = at[nm];
   std::vector<float> corners(9 * total);
   std::vector<uint32_t> keys(total);
   std::vector<ShadePacket> sp(total);
   for (uint32_t mi = 0; mi < nm; mi++) {
      const HostMesh& m = c->meshes[mi];
      if (m.resident()) continue;
      size_t t = at[mi];
      const uint32_t nt = (uint32_t)m.tris();
      for (uint32_t p = 0; p < nt; p++, t++) {
         const TriVerts tv = tri_verts(m, p);
         write_obj_corners(tv, &corners[9 * t]);
         fill_shade_packet(tv, mi, sp[t]);
         keys[t] = (mi << kPrimBits) | p;
      }
   }
   hipError_t e = c->d_src.alloc(total);
   if (e != hipSuccess) return sources_fail(c, e, "allocation");
   const BuildSources::View host{corners.data(), keys.data(), reinterpret_cast<const float4*>(sp.data())};
   e = for_each_run(nm, [&](size_t i) { return !c->meshes[i].resident(); }, [&](size_t i, size_t j) {
      return c->d_src.copy_range(at[i], host, at[i], at[j] - at[i], hipMemcpyHostToDevice, nullptr);
   });
   return e == hipSuccess ? UH_OK : sources_fail(c, e, "upload");
}

// the ranges move: a second set of arrays, the unchanged runs copied across on the device
static int move_unchanged_sources(uh_ctx* c, const std::vector<size_t>& at) {
   const size_t nm = c->meshes.size();
   BuildSources moved;
   const auto give_up = [&](hipError_t e, const char* what) {
      moved.release();
      return sources_fail(c, e, what);
   };
   hipError_t e = moved.alloc(at[nm]);
   if (e != hipSuccess) return give_up(e, "allocation");
   std::vector<size_t> old_at(nm + 1, 0);
   for (size_t i = 0; i < nm; i++) old_at[i + 1] = old_at[i] + c->src_tris[i];
   e = for_each_run(nm, [&](size_t i) { return c->src_serial[i] == c->meshes[i].serial; }, [&](size_t i, size_t j) {
      return moved.copy_range(at[i], c->d_src.view(), old_at[i], at[j] - at[i], hipMemcpyDeviceToDevice, c->stream);
   });
   const hipError_t waited = hipStreamSynchronize(c->stream);
   if (e != hipSuccess || (e = waited) != hipSuccess) return give_up(e, "device copy");
   c->d_src.swap(moved);
   moved.release();
   c->src_valid = false;  // src_tris / src_serial describe the old layout until the end of this call: a failure below starts over
   return UH_OK;
}

// every device-resident mesh in `todo` through k_iso_scatter, or through k_deform_scatter and k_deform_box when it is indexed
// (uh_update_mesh_vertices); its box words come back with the build's own wait
static int scatter_device_sources(uh_ctx* c, const std::vector<size_t>& at, const std::vector<uint32_t>& todo) {
   std::vector<uint32_t> box(6 * todo.size());
   for (size_t k = 0; k < todo.size(); k++)
      for (int a = 0; a < 6; a++) box[6 * k + a] = a < 3 ? 0xffffffffu : 0u;
   if (c->iso.box.n < box.size()) HIP_TRY(c, c->iso.box.alloc(box.size()));
   HIP_TRY(c, hipMemcpy(c->iso.box.p, box.data(), box.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
   for (size_t k = 0; k < todo.size(); k++) {
      const HostMesh& m = c->meshes[todo[k]];
      const size_t first = at[todo[k]];
      if (m.upd) {
         launch_deform_scatter(c->stream, m.d_verts, m.d_indices, (uint32_t)m.tris(), todo[k], c->d_src.corners.p + 9 * first, c->d_src.keys.p + first,
                               c->d_src.shade.p + 4 * first);
         launch_deform_box(c->stream, m.d_verts, (uint32_t)m.num_vertices(), c->iso.box.p + 6 * k);
         continue;
      }
      uhi_iso_scatter(c->stream, m.d_verts, m.dev_tris, todo[k], c->d_src.corners.p + 9 * first, c->d_src.keys.p + first,
                      c->d_src.shade.p + 4 * first, c->iso.box.p + 6 * k);
   }
   HIP_TRY(c, hipGetLastError());
   if (int st = iso_scatter_end(c, false)) return st;
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   HIP_TRY(c, hipMemcpy(box.data(), c->iso.box.p, box.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   for (size_t k = 0; k < todo.size(); k++) {
      HostMesh& m = c->meshes[todo[k]];
      for (int a = 0; a < 3; a++) {
         m.olo[a] = uhi_box_decode(box[6 * k + a]);
         m.ohi[a] = uhi_box_decode(box[6 * k + 3 + a]);
      }
      m.box_serial = m.serial;
   }
   return UH_OK;
}

static int refresh_build_sources(uh_ctx* c) {
   const size_t nm = c->meshes.size();
   std::vector<uint32_t> tris(nm);
   std::vector<size_t> at(nm + 1, 0);
   bool any_dev = false;
   for (size_t i = 0; i < nm; i++) {
      tris[i] = (uint32_t)c->meshes[i].tris();
      at[i + 1] = at[i] + tris[i];
      any_dev = any_dev || c->meshes[i].resident();
   }
   std::vector<uint32_t> todo;  // meshes whose range is written from their device vertices
   if (!c->src_valid) {
      for (size_t i = 0; i < nm; i++)
         if (c->meshes[i].resident()) todo.push_back((uint32_t)i);
      if (int st = upload_host_sources(c, at)) return st;
      iso_scatter_begin(c);
   } else {
      if (!any_dev) return UH_OK;  // (uh_add_mesh invalidates: the layout is that of the mesh list)
      bool same_counts = true;
      for (size_t i = 0; i < nm; i++) {
         if (c->src_serial[i] != c->meshes[i].serial) todo.push_back((uint32_t)i);
         same_counts = same_counts && c->src_tris[i] == tris[i];
      }
      if (todo.empty()) return UH_OK;
      iso_scatter_begin(c);
      if (!same_counts)
         if (int st = move_unchanged_sources(c, at)) return st;
   }
   if (!todo.empty())
      if (int st = scatter_device_sources(c, at, todo)) return st;
   c->src_tris = tris;
   c->src_serial.resize(nm);
   for (size_t i = 0; i < nm; i++) c->src_serial[i] = c->meshes[i].serial;
   c->src_valid = true;
   return UH_OK;
}

// uh_build_acceleration with option "device_build": Morton-order tree built by lbvh.hip, boxes by refit.hip
static int build_on_device(uh_ctx* c) {
   auto t0 = std::chrono::steady_clock::now();
   size_t total = 0;
   if (int st = scene_triangles(c, &total)) return st;
   if (int st = sync_all(c)) return st;
   if (int st = upload_scene_tables(c)) return st;
   if (int st = refresh_build_sources(c)) return st;
   // per-mesh rows + a box that holds every centroid: the 8 corners of each mesh's object-space box, transformed
   const std::vector<RefitMesh> rm = refit_mesh_rows(c);
   float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
   for (const HostMesh& m : c->meshes) {
      float olo[3] = {INFINITY, INFINITY, INFINITY}, ohi[3] = {-INFINITY, -INFINITY, -INFINITY};
      if (m.resident()) {
         // the same minima and maxima, reduced on the device by k_iso_scatter / k_deform_box (refresh_build_sources)
         if (m.dev ? !m.dev_tris : m.vertices.empty()) continue;
         if (m.box_serial != m.serial) return fail(c, UH_ERR_HIP, "internal: a device-resident mesh has no box");
         for (int a = 0; a < 3; a++) olo[a] = m.olo[a], ohi[a] = m.ohi[a];
      } else {
         for (const UhVertex& v : m.vertices)
            for (int a = 0; a < 3; a++) {
               olo[a] = std::fmin(olo[a], v.pos[a]);
               ohi[a] = std::fmax(ohi[a], v.pos[a]);
            }
         if (m.vertices.empty()) continue;
      }
      for (int k = 0; k < 8; k++) {
         const float x = (k & 1) ? ohi[0] : olo[0], y = (k & 2) ? ohi[1] : olo[1], z = (k & 4) ? ohi[2] : olo[2];
         for (int a = 0; a < 3; a++) {
            const float w = m.o2w[4 * a] * x + m.o2w[4 * a + 1] * y + m.o2w[4 * a + 2] * z + m.o2w[4 * a + 3];
            lo[a] = std::fmin(lo[a], w);
            hi[a] = std::fmax(hi[a], w);
         }
      }
   }
   for (int a = 0; a < 3; a++)
      if (!(lo[a] <= hi[a]) || !std::isfinite(lo[a]) || !std::isfinite(hi[a])) lo[a] = hi[a] = 0.0f;
   const size_t node_cap = total > 1 ? total : 1;
   HIP_TRY(c, c->d_nodes.alloc(node_cap * kNodeStride16));
   HIP_TRY(c, c->d_tris.alloc(total * kTriStride16));
   HIP_TRY(c, c->d_shade.alloc(total * 4));
   HIP_TRY(c, c->d_obj_corners.alloc(9 * total));
   HIP_TRY(c, c->d_world_corners.alloc(9 * total));
   HIP_TRY(c, c->d_node_box.alloc(6 * node_cap));
   HIP_TRY(c, c->d_refit_meshes.alloc(rm.size()));
   if (!rm.empty()) HIP_TRY(c, hipMemcpy(c->d_refit_meshes.p, rm.data(), rm.size() * sizeof(RefitMesh), hipMemcpyHostToDevice));
   LbvhArgs la;
   la.src_corners = c->d_src.corners.p;
   la.src_keys = c->d_src.keys.p;
   la.src_shade = c->d_src.shade.p;
   la.meshes = c->d_refit_meshes.p;
   for (int a = 0; a < 3; a++) {
      la.bounds_lo[a] = lo[a];
      la.bounds_hi[a] = hi[a];
   }
   la.num_tris = (uint32_t)total;
   la.kind = c->device_build_kind;
   la.ploc_radius = uh_ctx::kPlocRadius;
   la.sah_top = c->ploc_sah_top;
   la.nodes = reinterpret_cast<uint4*>(c->d_nodes.p);
   la.node_capacity = (uint32_t)node_cap;
   la.tris = c->d_tris.p;
   la.shade = c->d_shade.p;
   la.obj_corners = c->d_obj_corners.p;
   uint32_t num_nodes = 1;
   hipError_t e = lbvh_build(la, c->stream, c->level_start, &num_nodes);
   // the builder gave up on this geometry (a PLOC round that merges nothing: every union area inf / NaN, e.g. coordinates
   // around 1e19 whose area products overflow): like a tree that came out too deep, such a scene gets the host builder
   const bool gave_up = e == hipErrorUnknown;
   if (gave_up)
      (void)hipGetLastError();
   else if (e != hipSuccess)
      return fail(c, UH_ERR_HIP, std::string("device BVH build: ") + hipGetErrorString(e));
   if (gave_up || c->level_start.size() - 1 > kMaxTreeLevels) {
      // a Morton tree over clustered geometry can be a long chain; deeper than the traversal stack it would drop
      // subtrees silently: this scene gets the host builder (which has a balanced fallback of its own)
      c->device_build = false;
      const int st = uh_build_acceleration(c);
      c->device_build = true;
      return st;
   }
   if (total) {
      launch_refit(cfg(c), refit_args(c, total));
      HIP_TRY(c, hipGetLastError());
   }
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   c->packet_keys.assign(total, 0u);  // only its size is used once d_obj_corners exists (uh_refit_acceleration)
   publish_tree(c, num_nodes, total, t0);
   return UH_OK;
}

// diagnostics: the tree in use, read back and held to bvh_invariants.h - see utopian_hip.h
int uh_check_acceleration(uh_ctx* c, uint64_t out[16]) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   for (int k = 0; k < 16; k++) out[k] = 0;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (!c->built || !c->topology_valid || !c->d_nodes.p || c->level_start.size() < 2)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_check_acceleration: no tree has been built for the scene as it is (uh_build_acceleration or uh_refit_acceleration first)");
   const uint32_t nn = c->scene.num_nodes, nt = c->scene.num_tris;
   std::vector<Node4C> nodes(nn);
   std::vector<TriPacket> packets(nt);
   std::vector<ShadePacket> shade(nt);
   std::vector<float> corners(9 * (size_t)nt);
   HIP_TRY(c, hipMemcpy2D(nodes.data(), sizeof(Node4C), c->d_nodes.p, 16 * kNodeStride16, sizeof(Node4C), nn, hipMemcpyDeviceToHost));
   if (nt) {
      HIP_TRY(c, hipMemcpy2D(packets.data(), sizeof(TriPacket), c->d_tris.p, 16 * kTriStride16, sizeof(TriPacket), nt, hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy(shade.data(), c->d_shade.p, (size_t)nt * sizeof(ShadePacket), hipMemcpyDeviceToHost));
   }
   if (nt && c->d_obj_corners.p) {
      // a device build or a refit has baked them (k_refit_triangles): the corners the boxes on the device were made from
      HIP_TRY(c, hipMemcpy(corners.data(), c->d_world_corners.p, corners.size() * sizeof(float), hipMemcpyDeviceToHost));
   } else {
      // the host builder's tree, never refitted: no corners on the device. Its bake (uh_build_acceleration) again, by the packets' keys
      for (uint32_t i = 0; i < nt; i++) {
         const uint32_t mi = packets[i].key >> kPrimBits, p = packets[i].key & kPrimMask;
         float* o = &corners[9 * (size_t)i];
         if (mi >= c->meshes.size() || c->meshes[mi].vertices.empty() || p >= c->meshes[mi].indices.size() / 3) {
            for (int k = 0; k < 9; k++) o[k] = 0.0f;  // (a key the scene does not have: the report's `keys`)
            continue;
         }
         const HostMesh& m = c->meshes[mi];
         write_obj_corners(tri_verts(m, p), o);
         if (is_identity3x4(m.o2w)) continue;
         const float* w = m.o2w;
         for (int k = 0; k < 3; k++, o += 3) {
            const float x = o[0], y = o[1], z = o[2];
            o[0] = ((w[0] * x + w[1] * y) + w[2] * z) + w[3];
            o[1] = ((w[4] * x + w[5] * y) + w[6] * z) + w[7];
            o[2] = ((w[8] * x + w[9] * y) + w[10] * z) + w[11];
         }
      }
   }
   std::vector<uint32_t> keys;  // mesh order, primitive order: ascending
   for (uint32_t mi = 0; mi < c->meshes.size(); mi++)
      for (uint32_t p = 0, np = (uint32_t)c->meshes[mi].tris(); p < np; p++) keys.push_back((mi << kPrimBits) | p);
   TreeView v;
   v.nodes = nodes.data(), v.num_nodes = nn;
   v.packets = packets.data(), v.num_tris = nt;
   v.corners = corners.data();
   v.shade_mesh = nt ? &shade[0].mesh : nullptr;
   v.level_start = c->level_start.data(), v.level_entries = (uint32_t)c->level_start.size();
   v.keys = keys.data(), v.num_keys = (uint32_t)keys.size();
   const TreeReport rep = check_tree(v);
   out[0] = nn;
   out[1] = nt;
   out[2] = rep.levels;
   for (int k = 0; k < kTreeClasses; k++) out[3 + k] = rep.violations[k];
   std::memcpy(&out[10], &rep.sah, sizeof(double));
   out[11] = rep.geometry ? 1 : 0;
   c->err = rep.total() ? "uh_check_acceleration: " + rep.text() : std::string();  // violations are the result, not an error
   return UH_OK;
}

int uh_mesh_info(uh_ctx* c, uint32_t mesh_index, uint32_t* num_vertices, uint32_t* num_indices) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (mesh_index >= c->meshes.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_mesh_info: bad mesh index");
   if (num_vertices) *num_vertices = (uint32_t)c->meshes[mesh_index].num_vertices();
   if (num_indices) *num_indices = (uint32_t)c->meshes[mesh_index].num_indices();
   return UH_OK;
}

int uh_read_mesh(uh_ctx* c, uint32_t mesh_index, UhVertex* vertices, uint32_t* indices) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (mesh_index >= c->meshes.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_mesh: bad mesh index");
   const HostMesh& m = c->meshes[mesh_index];
   if (m.dev && !m.host_valid) {
      // a device-resident mesh without a host mirror: the vertices come from the device (a blocking copy; they are idle since the
      // update returned)
      if (!m.dev_tris) return UH_OK;
      HIP_TRY(c, hipSetDevice(c->device));
      const size_t n = 3 * (size_t)m.dev_tris;
      if (vertices) {
         HIP_TRY(c, hipMemcpy(vertices, m.d_verts, n * sizeof(UhVertex), hipMemcpyDeviceToHost));
         c->iso.st.host_geometry_bytes += n * sizeof(UhVertex);
      }
      if (indices) {
         for (size_t i = 0; i < n; i++) indices[i] = (uint32_t)i;  // the index list of a device-resident mesh is never stored
         c->iso.st.host_geometry_bytes += n * sizeof(uint32_t);    // counted as handed to the host, like the vertices
      }
      return UH_OK;
   }
   if (m.upd && !m.host_valid) {
      // updated from a device pointer: the vertices come from the device the same way, the index list is the host's
      if (vertices) {
         HIP_TRY(c, hipSetDevice(c->device));
         HIP_TRY(c, hipMemcpy(vertices, m.d_verts, m.vertices.size() * sizeof(UhVertex), hipMemcpyDeviceToHost));
         c->mupd.st.host_geometry_bytes += m.vertices.size() * sizeof(UhVertex);
      }
      if (indices) std::memcpy(indices, m.indices.data(), m.indices.size() * sizeof(uint32_t));
      return UH_OK;
   }
   if (vertices && !m.vertices.empty()) std::memcpy(vertices, m.vertices.data(), m.vertices.size() * sizeof(UhVertex));
   if (indices && !m.indices.empty()) std::memcpy(indices, m.indices.data(), m.indices.size() * sizeof(uint32_t));
   return UH_OK;
}

int uhi_mark_isosurface(uh_ctx* c, uint32_t mesh_index, uint32_t resolution, float lo, float hi, int reference) {
   if (!c || mesh_index >= c->meshes.size()) return UH_ERR_INVALID_ARGUMENT;
   HostMesh& m = c->meshes[mesh_index];
   m.iso = true;
   m.iso_reference = reference != 0;
   m.iso_res = resolution;
   m.iso_lo = lo;
   m.iso_hi = hi;
   return UH_OK;
}

int uh_update_isosurface_mesh(uh_ctx* c, uint32_t mesh_index, float time, uint32_t* out_triangles) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (mesh_index >= c->meshes.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_isosurface_mesh: bad mesh index");
   if (!c->meshes[mesh_index].iso) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_isosurface_mesh: the mesh was not created by uh_add_isosurface_mesh");
   if (!std::isfinite(time)) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_isosurface_mesh: time is not finite");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   HostMesh& m = c->meshes[mesh_index];
   uh_ctx::IsoUpdate& u = c->iso;
   for (hipEvent_t* ev : {&u.begin, &u.end})
      if (!*ev) HIP_TRY(c, hipEventCreate(ev));
   const uint32_t blocks = uhi_iso_blocks(m.iso_res), n_chunks = scan_chunk_count(blocks);
   if (u.counts.n < blocks) HIP_TRY(c, u.counts.alloc(blocks));
   if (u.chunks.n < n_chunks) HIP_TRY(c, u.chunks.alloc(n_chunks));
   if (!u.total.p) HIP_TRY(c, u.total.alloc(1));
   HIP_TRY(c, hipEventRecord(u.begin, c->stream));
   unsigned long long total = 0;  // the 8 bytes that size the buffers
   if (!uhi_iso_count_triangles(c->stream, m.iso_res, m.iso_lo, m.iso_hi, time, m.iso_reference, u.counts.p, u.chunks.p, u.total.p, &total))
      return fail(c, UH_ERR_HIP, std::string("uh_update_isosurface_mesh: count pass: ") + hipGetErrorString(hipGetLastError()));
   if (total > (1ull << kPrimBits)) return fail(c, UH_ERR_CAPACITY, "uh_update_isosurface_mesh: more than 4 Mi triangles");
   if (3 * total > m.d_capacity) {
      // the new buffer first: a refusal leaves the mesh as it was
      UhVertex* grown = nullptr;
      HIP_TRY(c, hipMalloc((void**)&grown, 3 * total * sizeof(UhVertex)));
      if (m.d_verts) (void)hipFree(m.d_verts);
      m.d_verts = grown;
      m.d_capacity = 3 * total;
   }
   // from here on the mesh's geometry is the new one (the vertex buffer is being overwritten): whatever happens, the context is not built
   m.dev = true;
   m.host_valid = false;
   m.dev_tris = (uint32_t)total;
   m.serial++;
   std::vector<UhVertex>().swap(m.vertices);
   std::vector<uint32_t>().swap(m.indices);
   c->built = false;
   c->topology_valid = false;
   if (total && !uhi_iso_extract_emit(c->stream, m.iso_res, m.iso_lo, m.iso_hi, time, m.iso_reference, u.counts.p, m.d_verts))
      return fail(c, UH_ERR_HIP, "uh_update_isosurface_mesh: the case tables could not be loaded");
   HIP_TRY(c, hipGetLastError());
   HIP_TRY(c, hipEventRecord(u.end, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   HIP_TRY(c, hipEventElapsedTime(&u.st.extract_ms, u.begin, u.end));
   u.st.scatter_ms = 0.0f;
   u.st.updates++;
   u.st.triangles = (uint32_t)total;
   if (out_triangles) *out_triangles = (uint32_t)total;
   return UH_OK;
}

int uh_get_isosurface_update_stats(uh_ctx* c, UhIsosurfaceUpdateStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_isosurface_update_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (!c->iso.st.updates) return UH_OK;
   *out = c->iso.st;
   const uh_ctx::IsoUpdate& u = c->iso;
   out->device_bytes = u.counts.n * sizeof(uint32_t) + u.chunks.n * sizeof(uint32_t) + u.box.n * sizeof(uint32_t) + u.total.n * sizeof(unsigned long long);
   for (const HostMesh& m : c->meshes)
      if (!m.upd) out->device_bytes += m.d_capacity * sizeof(UhVertex);
   return UH_OK;
}

}  // extern "C"

int replace_mesh_vertices(uh_ctx* c, HostMesh& m, const char* verb, bool host_valid, const std::function<int()>& write) {
   const size_t num_vertices = m.vertices.size();
   for (hipEvent_t& ev : c->mupd.ev)  // the refit behind this update times its gather with them
      if (!ev) HIP_TRY(c, hipEventCreate(&ev));
   if (!m.upd) {
      // the mesh's own buffers, and its index list to the device this once; a refusal leaves the mesh as it was
      UhVertex* dv = nullptr;
      uint32_t* di = nullptr;
      const size_t index_bytes = m.indices.size() * sizeof(uint32_t);
      hipError_t e = hipMalloc((void**)&dv, num_vertices * sizeof(UhVertex));
      if (e == hipSuccess && index_bytes) e = hipMalloc((void**)&di, index_bytes);
      if (e == hipSuccess && index_bytes) e = hipMemcpy(di, m.indices.data(), index_bytes, hipMemcpyHostToDevice);
      if (e != hipSuccess) {
         if (dv) (void)hipFree(dv);
         if (di) (void)hipFree(di);
         return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string(verb) + ": the mesh's device buffers: " + hipGetErrorString(e));
      }
      m.d_verts = dv;
      m.d_indices = di;
      m.d_capacity = num_vertices;
      m.upd = true;
   }
   // from here on the mesh's geometry is the new one: whatever happens, the context is not built
   m.serial++;
   c->built = false;
   m.host_valid = host_valid;
   if (int st = write()) return st;
   c->mupd.st.updates++;
   return UH_OK;
}

extern "C" {

int uh_update_mesh_vertices(uh_ctx* c, uint32_t mesh_index, const UhVertex* vertices, uint32_t num_vertices, int where) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (mesh_index >= c->meshes.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: bad mesh index");
   if (where != UH_VERTICES_HOST && where != UH_VERTICES_DEVICE) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: `where` is neither UH_VERTICES_HOST nor UH_VERTICES_DEVICE");
   HostMesh& m = c->meshes[mesh_index];
   if (m.iso) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: the mesh was created by uh_add_isosurface_mesh (uh_update_isosurface_mesh updates it)");
   if (num_vertices != m.vertices.size()) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: the vertex count differs from the mesh's");
   if (num_vertices && !vertices) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: null vertices");
   if (where == UH_VERTICES_HOST)
      for (uint32_t i = 0; i < num_vertices; i++)
         if (!std::isfinite(vertices[i].pos[0]) || !std::isfinite(vertices[i].pos[1]) || !std::isfinite(vertices[i].pos[2]))
            return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: vertex position is not finite");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   uh_ctx::MeshUpdate& u = c->mupd;
   if (!num_vertices) {  // nothing to move: the mesh stays where it is
      u.st.updates++;
      return UH_OK;
   }
   if (where == UH_VERTICES_DEVICE) {
      // the caller's buffer is looked at before anything of the mesh is overwritten
      if (!u.flag.p) HIP_TRY(c, u.flag.alloc(1));
      uint32_t flag = 0;
      HIP_TRY(c, hipMemsetAsync(u.flag.p, 0, sizeof(uint32_t), c->stream));
      launch_deform_check(c->stream, vertices, num_vertices, u.flag.p);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(&flag, u.flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (flag) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_update_mesh_vertices: vertex position is not finite");
   }
   const size_t bytes = num_vertices * sizeof(UhVertex);
   return replace_mesh_vertices(c, m, "uh_update_mesh_vertices", where == UH_VERTICES_HOST, [&]() -> int {
      if (where == UH_VERTICES_HOST) {
         std::memcpy(m.vertices.data(), vertices, bytes);
         HIP_TRY(c, hipMemcpy(m.d_verts, vertices, bytes, hipMemcpyHostToDevice));
         u.st.host_geometry_bytes += bytes;
      } else {
         HIP_TRY(c, hipMemcpyAsync(m.d_verts, vertices, bytes, hipMemcpyDeviceToDevice, c->stream));
         HIP_TRY(c, hipStreamSynchronize(c->stream));
      }
      return UH_OK;
   });
}

int uh_get_mesh_update_stats(uh_ctx* c, UhMeshUpdateStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_mesh_update_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (!c->mupd.st.updates) return UH_OK;
   *out = c->mupd.st;
   for (const HostMesh& m : c->meshes)
      if (m.upd) out->device_bytes += m.d_capacity * sizeof(UhVertex) + m.indices.size() * sizeof(uint32_t);
   return UH_OK;
}

}  // extern "C"
