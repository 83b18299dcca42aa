// hybrid_graph.hip - the hybrid graph of include/utopian_hip.h (uh_render_hybrid: the ray-traced passes, the final frame, the IBL
// maps, the marching-cubes pass, the rasterised G-buffer, the reservoir lights, ray-traced ambient occlusion, motion vectors, temporal
// anti-aliasing, the HDR display chain, one-bounce ray-traced diffuse GI) with its
// read and stats verbs, and what the forward graph and the denoiser share with it: the mesh and light tables, the wait behind the
// frames in flight and destroy_graphs. Host code over uh_ctx::Hybrid (context_state.h); the rasterised passes go through
// raster_driver.hip. Host-side counterpart of build_render_graph (utopian/src/renderers/mod.rs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "device_scan.h"
#include "graphs_internal.h"
#include "motion_device.h"

// ---- first use, the tables and what the other graphs share ----
// the events of the hybrid stages and of the waits behind the frames in flight (first hybrid or forward call)
int hybrid_events(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   for (hipEvent_t& ev : h.waits)
      if (!ev) HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
   return stage_create(c, h.stage, kHybridStages);
}
// the ray-traced images and the events (first call)
static int hybrid_alloc(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   if (h.counter.p) return UH_OK;
   if (int st = hybrid_events(c)) return st;
   return alloc_group(c, [&](auto f) { h.rt_images((size_t)c->W * c->H, f); });
}

// everything the graphs own (uh_destroy)
void destroy_graphs(uh_ctx* c) {
   c->hy.destroy();
   c->fw.destroy();
   if (c->dn.acc_read && c->last_acc == c->dn.acc_read) c->last_acc = nullptr;
   c->dn.destroy();
}

// the meshes as the vertex and fragment shaders read them: vertices, indices, the instance's world matrix and the material's maps
int hybrid_tables(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   if (h.geom == c->geom_version && h.meshes.p) return UH_OK;
   std::vector<HybridMesh> ms(c->meshes.size());
   size_t nv = 0, ni = 0;
   for (size_t i = 0; i < c->meshes.size(); i++) {
      const HostMesh& m = c->meshes[i];
      HybridMesh& d = ms[i];
      for (int r = 0; r < 3; r++)
         for (int k = 0; k < 3; k++) d.o2w[3 * r + k] = m.o2w[4 * r + k];
      std::memcpy(d.w2o, m.w2o, sizeof(d.w2o));
      d.vertex_base = (uint32_t)nv;
      d.index_base = (uint32_t)ni;
      d.diffuse_map = m.material.diffuse_map;
      d.normal_map = m.material.normal_map;
      d.metallic_roughness_map = m.material.metallic_roughness_map;
      d.occlusion_map = m.material.occlusion_map;
      nv += m.num_vertices();
      ni += m.num_indices();
   }
   if (nv >= (1ull << 32) || ni >= (1ull << 32)) return fail(c, UH_ERR_CAPACITY, "uh_render_hybrid: more than 2^32 vertices or indices");
   bool any_dev = false;
   for (const HostMesh& m : c->meshes) any_dev = any_dev || m.resident();
   if (any_dev) {
      // a second pair of arrays; per mesh: a range the old pair holds for the same serial is copied across on the device, a
      // device-resident mesh is copied from its vertex buffer with an iota index list (uh_update_mesh_vertices: with its own index
      // list, which is on the device too), a host-resident one is uploaded
      DevBuf<UhVertex> vb;
      DevBuf<uint32_t> ib;
      const auto give_up = [&](hipError_t e) {
         (void)hipStreamSynchronize(c->stream);
         vb.release(), ib.release();
         return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string("mesh tables: ") + hipGetErrorString(e));
      };
      hipError_t e;
      bool in_place = h.meshes.p && h.layout.size() == c->meshes.size();
      for (size_t i = 0; in_place && i < c->meshes.size(); i++)
         in_place = h.layout[i].nv == c->meshes[i].num_vertices() && h.layout[i].ni == c->meshes[i].num_indices();
      if (in_place) {
         // no count changed: the updated meshes' vertices over their old ones (their index range stays), the bases as they are
         iso_scatter_begin(c);
         for (size_t i = 0; i < c->meshes.size(); i++) {
            const HostMesh& m = c->meshes[i];
            if (h.layout[i].serial == m.serial) continue;
            if (h.layout[i].nv) HIP_TRY(c, hipMemcpyAsync(h.vertices.p + h.layout[i].vb, m.d_verts, h.layout[i].nv * sizeof(UhVertex), hipMemcpyDeviceToDevice, c->stream));
            h.layout[i].serial = ~0ull;  // (until the copy is known to have completed)
         }
         HIP_TRY(c, hipMemcpyAsync(h.meshes.p, ms.data(), ms.size() * sizeof(HybridMesh), hipMemcpyHostToDevice, c->stream));
         if (int st = iso_scatter_end(c, true)) return st;
         HIP_TRY(c, hipStreamSynchronize(c->stream));
         for (size_t i = 0; i < c->meshes.size(); i++) h.layout[i].serial = c->meshes[i].serial;
         h.geom = c->geom_version;
         return UH_OK;
      }
      if ((e = vb.alloc(nv)) != hipSuccess || (e = ib.alloc(ni)) != hipSuccess) return give_up(e);
      std::vector<uh_ctx::Hybrid::Range> layout(c->meshes.size());
      iso_scatter_begin(c);
      for (size_t i = 0; i < c->meshes.size(); i++) {
         const HostMesh& m = c->meshes[i];
         uh_ctx::Hybrid::Range& r = layout[i];
         r = uh_ctx::Hybrid::Range{ms[i].vertex_base, ms[i].index_base, (uint32_t)m.num_vertices(), (uint32_t)m.num_indices(), m.serial};
         const uh_ctx::Hybrid::Range* old = h.meshes.p && i < h.layout.size() ? &h.layout[i] : nullptr;
         e = hipSuccess;
         if (old && old->serial == r.serial && old->nv == r.nv && old->ni == r.ni) {
            if (r.nv) e = hipMemcpyAsync(vb.p + r.vb, h.vertices.p + old->vb, r.nv * sizeof(UhVertex), hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess && r.ni) e = hipMemcpyAsync(ib.p + r.ib, h.indices.p + old->ib, r.ni * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
         } else if (m.dev) {
            if (r.nv) e = hipMemcpyAsync(vb.p + r.vb, m.d_verts, r.nv * sizeof(UhVertex), hipMemcpyDeviceToDevice, c->stream);
            uhi_iota(c->stream, ib.p + r.ib, r.ni);
            if (e == hipSuccess) e = hipGetLastError();
         } else if (m.upd) {
            if (r.nv) e = hipMemcpyAsync(vb.p + r.vb, m.d_verts, r.nv * sizeof(UhVertex), hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess && r.ni) e = hipMemcpyAsync(ib.p + r.ib, m.d_indices, r.ni * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
         } else {
            if (r.nv) e = hipMemcpy(vb.p + r.vb, m.vertices.data(), r.nv * sizeof(UhVertex), hipMemcpyHostToDevice);
            if (e == hipSuccess && r.ni) e = hipMemcpy(ib.p + r.ib, m.indices.data(), r.ni * sizeof(uint32_t), hipMemcpyHostToDevice);
         }
         if (e != hipSuccess) return give_up(e);
      }
      if ((e = h.meshes.n == ms.size() && h.meshes.p ? hipSuccess : h.meshes.alloc(ms.size())) != hipSuccess) return give_up(e);
      if ((e = hipMemcpyAsync(h.meshes.p, ms.data(), ms.size() * sizeof(HybridMesh), hipMemcpyHostToDevice, c->stream)) != hipSuccess) return give_up(e);
      if (int st = iso_scatter_end(c, true)) {
         vb.release(), ib.release();
         return st;
      }
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return give_up(e);
      std::swap(h.vertices, vb);
      std::swap(h.indices, ib);
      vb.release(), ib.release();
      h.layout = std::move(layout);
      h.geom = c->geom_version;
      return UH_OK;
   }
   std::vector<UhVertex> verts;
   std::vector<uint32_t> idx;
   verts.reserve(nv);
   idx.reserve(ni);
   for (const HostMesh& m : c->meshes) {
      verts.insert(verts.end(), m.vertices.begin(), m.vertices.end());
      idx.insert(idx.end(), m.indices.begin(), m.indices.end());
   }
   HIP_TRY(c, h.meshes.alloc(ms.size()));
   HIP_TRY(c, h.vertices.alloc(verts.size()));
   HIP_TRY(c, h.indices.alloc(idx.size()));
   if (!ms.empty()) HIP_TRY(c, hipMemcpyAsync(h.meshes.p, ms.data(), ms.size() * sizeof(HybridMesh), hipMemcpyHostToDevice, c->stream));
   if (!verts.empty()) HIP_TRY(c, hipMemcpyAsync(h.vertices.p, verts.data(), verts.size() * sizeof(UhVertex), hipMemcpyHostToDevice, c->stream));
   if (!idx.empty()) HIP_TRY(c, hipMemcpyAsync(h.indices.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
   h.layout.resize(ms.size());
   for (size_t i = 0; i < ms.size(); i++)
      h.layout[i] = uh_ctx::Hybrid::Range{ms[i].vertex_base, ms[i].index_base, (uint32_t)c->meshes[i].num_vertices(), (uint32_t)c->meshes[i].num_indices(), c->meshes[i].serial};
   h.geom = c->geom_version;
   return UH_OK;
}

// the final frame's images and light table (first call with one of its bits); the metal-pixel queue of rt_reflections is reused
// for the sky pixels, which are queued after rt_reflections has run
static int hybrid_frame_alloc(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   if (h.sky_counter.p) return UH_OK;
   return alloc_group(c, [&](auto f) { h.frame_images((size_t)c->W * c->H, f); });
}

// the uh_add_light table as the deferred pass reads it (lights are only ever appended: the count says whether it changed)
int hybrid_light_table(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   if (h.lights_uploaded == c->lights.size()) return UH_OK;
   HIP_TRY(c, h.raw_lights.alloc(c->lights.size()));
   if (!c->lights.empty())
      HIP_TRY(c, hipMemcpyAsync(h.raw_lights.p, c->lights.data(), c->lights.size() * sizeof(UhGpuLight), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   h.lights_uploaded = c->lights.size();
   return UH_OK;
}

// the IBL maps (first call with UH_HYBRID_ENVIRONMENT) and the irradiance filter's tap table: irradiance_filter.frag:38-46's phi and
// theta are float accumulators stepped by 0.025 while below 2 PI and PI / 2 (float); sin and cos in double, rounded to float, and the
// products tangentSample.x = sin(theta) cos(phi), .y = sin(theta) sin(phi) in float
static int env_alloc(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   if (h.env.lut.p) return UH_OK;
   std::vector<float4> taps;
   taps.reserve(kIrrPhi * kIrrTheta);
   const float pi = 3.14159265358979323846f, delta = 0.025f;
   for (float phi = 0.0f; phi < 2.0f * pi; phi += delta) {
      for (float theta = 0.0f; theta < 0.5f * pi; theta += delta) {
         const float st = (float)std::sin((double)theta), ct = (float)std::cos((double)theta);
         const float cp = (float)std::cos((double)phi), sp = (float)std::sin((double)phi);
         taps.push_back(make_float4(st * cp, st * sp, ct, st));
      }
   }
   if (taps.size() != (size_t)kIrrPhi * kIrrTheta) return fail(c, UH_ERR_HIP, "irradiance tap count");
   HIP_TRY(c, h.env.taps.alloc(taps.size()));
   HIP_TRY(c, hipMemcpyAsync(h.env.taps.p, taps.data(), taps.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return alloc_group(c, [&](auto f) { h.env.images(f); });
}

// behind every frame in flight: the context's first stream (slot 0's, where hybrid and forward calls run) waits for the others
int wait_frames_in_flight(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   int w = 0;
   for (uint32_t i = 1; i < kMaxSlots; i++) {
      const Slot& s = c->slots[i];
      if (!s.ready) continue;
      for (hipStream_t st : {s.stream, s.side}) {
         HIP_TRY(c, hipEventRecord(h.waits[w], st));
         HIP_TRY(c, hipStreamWaitEvent(c->stream, h.waits[w++], 0));
      }
   }
   if (c->restir_stream) {
      HIP_TRY(c, hipEventRecord(h.waits[w], c->restir_stream));
      HIP_TRY(c, hipStreamWaitEvent(c->stream, h.waits[w++], 0));
   }
   if (c->slots[0].ready) {
      HIP_TRY(c, hipEventRecord(h.waits[w], c->slots[0].side));
      HIP_TRY(c, hipStreamWaitEvent(c->stream, h.waits[w++], 0));
   }
   return UH_OK;
}

// ---- the marching-cubes pass (utopian_hip.h "UH_HYBRID_MARCHING_CUBES"; isosurface.hip, forward.hip) ----
// extraction (count, scan, emit), depth seed, bin_and_resolve (flat triangles, seeded resolve), then forward.frag into deferred_output:
// the triangle count comes back to the host before the binning (the buffers grow to it)
static int render_mc_pass(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view) {
   uh_ctx::Hybrid& h = c->hy;
   RasterBins& b = h.mc.bins;
   ForwardDev fd{};
   const uint32_t tiles = forward_frame(c, h.mc.target, fd);
   const char* const who = "uh_render_hybrid: marching cubes";
   for (int st : {grow(c, b.tile_count, tiles, who), grow(c, b.tile_cursor, tiles, who),
                  grow(c, b.chunks, scan_chunk_count(std::max<uint32_t>(kMcBlocks, tiles)), who)})
      if (st) return st;
   // the material of mesh_index 0 under world = identity, and the matrices: (P V) I as forward_mesh_matrices makes it, then P V
   static const float identity3x4[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
   HybridMesh mm{};
   for (int k = 0; k < 9; k++) mm.o2w[k] = mm.w2o[k] = k % 4 == 0 ? 1.0f : 0.0f;
   const UhGpuMaterial& m0 = c->meshes[0].material;
   mm.diffuse_map = m0.diffuse_map;
   mm.normal_map = m0.normal_map;
   mm.metallic_roughness_map = m0.metallic_roughness_map;
   mm.occlusion_map = m0.occlusion_map;
   float mats[44], pv[16], ident[16];
   mat4_from_3x4(identity3x4, ident);
   mat4_mul(view.projection, view.view, pv);
   mat4_mul(pv, ident, mats);
   std::memcpy(mats + 16, identity3x4, sizeof(identity3x4));
   std::memcpy(mats + 28, pv, sizeof(pv));
   HIP_TRY(c, hipMemcpyAsync(h.mc.mesh.p, &mm, sizeof(mm), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(b.mats.p, mats, sizeof(mats), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemsetAsync(b.tile_count.p, 0, tiles * sizeof(uint32_t), c->stream));
   HIP_TRY(c, hipMemsetAsync(h.mc.target.covered.p, 0, sizeof(uint32_t), c->stream));
   // marching_cubes.comp at view.time: per-block counts, their scan, then (with the total known) the triangles
   if (!uhi_mc_extract_count(c->stream, view.time, h.mc.block_counts.p)) return fail(c, UH_ERR_HIP, "uh_render_hybrid: marching-cubes tables");
   device_exclusive_scan_u32(h.mc.block_counts.p, kMcBlocks, b.chunks.p, h.mc.total.p, c->stream);
   fd.meshes = h.mc.mesh.p;
   fd.mats = b.mats.p;
   fd.tile_count = b.tile_count.p;
   fd.tile_cursor = b.tile_cursor.p;
   fd.color = h.deferred.p;
   // the G-buffer's depth attachment (marching_cubes.rs:97, LOAD): the rasterised pass's own, or the cast's reconstruction
   if (h.gbuffer_rasterised)
      HIP_TRY(c, hipMemcpyAsync(h.mc.target.depth.p, h.gr.target.depth.p, (size_t)c->W * c->H * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
   else
      launch_mc_depth_seed(lc, h.pos.p, fd);
   unsigned long long ntri = 0;
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   HIP_TRY(c, hipMemcpy(&ntri, h.mc.total.p, sizeof(ntri), hipMemcpyDeviceToHost));
   if (ntri > 5ull * kMcRes * kMcRes * kMcRes) return fail(c, UH_ERR_HIP, "uh_render_hybrid: marching-cubes triangle count out of range");
   for (int st : {grow(c, h.mc.verts, std::max<size_t>(3, 3 * (size_t)ntri), who), grow(c, b.rec_count, std::max<size_t>(1, (size_t)ntri), who),
                  grow(c, b.chunks, scan_chunk_count(std::max<uint32_t>((uint32_t)ntri, tiles)), who)})
      if (st) return st;
   if (ntri && !uhi_mc_extract_emit(c->stream, view.time, h.mc.block_counts.p, h.mc.verts.p)) return fail(c, UH_ERR_HIP, "uh_render_hybrid: marching-cubes tables");
   fd.vertices = h.mc.verts.p;
   fd.num_tris = (uint32_t)ntri;
   fd.rec_count = b.rec_count.p;
   uint32_t pieces = 0;
   if (int st = bin_forward(c, lc, b, fd, tiles, who, true, &pieces)) return st;
   light_and_shade(c, lc, view, fd, h.mc.lights.p, true);
   h.mc.tris = (uint32_t)ntri;
   h.mc.pieces = pieces;
   h.mc.lights_used = view.num_lights + 1;
   h.mc.time = view.time;
   h.mc.renders++;
   return UH_OK;
}

// ---- motion vectors (utopian_hip.h "motion vectors"; motion.hip) ----
// before a motion pass: the pass's buffers (first call with the bit) and the per-mesh table - every mesh's state against the snapshot the
// previous motion pass left, with that snapshot's transform and rows
static int motion_prepare(uh_ctx* c, MotionDev& md) {
   uh_ctx::Hybrid& h = c->hy;
   const char* const who = "uh_render_hybrid: motion vectors";
   if (!h.mv.counters.p) {
      if (int st = stage_create(c, h.mv.stage, 2)) return st;
      if (int st = alloc_group(c, [&](auto f) { h.mv.images((size_t)c->W * c->H, f); })) return st;
   }
   const size_t nm = c->meshes.size();
   if (int st = grow(c, h.mv.table, std::max<size_t>(1, nm), who)) return st;
   h.mv.rows.assign(nm, MotionMesh{});
   uint32_t states[4] = {0, 0, 0, 0};
   for (size_t i = 0; i < nm; i++) {
      const HostMesh& m = c->meshes[i];
      MotionMesh& row = h.mv.rows[i];
      std::memcpy(row.prev_o2w, m.o2w, sizeof(row.prev_o2w));
      if (h.mv.renders == 0) {
         row.state = kMotionStatic;  // the first pass ever: what uh_denoise assumes without the flag
      } else if (i >= h.mv.snap.size()) {
         row.state = kMotionNone;    // added since
      } else {
         const uh_ctx::Hybrid::Motion::Snap& s = h.mv.snap[i];
         std::memcpy(row.prev_o2w, s.o2w, sizeof(row.prev_o2w));
         row.prev_base = s.base;
         row.prev_count = s.count;
         if (s.serial != m.serial)   // uh_update_isosurface_mesh re-extracts: no correspondence; uh_update_mesh_vertices keeps the topology
            row.state = m.iso ? kMotionNone : kMotionDeformed;
         else
            row.state = std::memcmp(s.o2w, m.o2w, sizeof(s.o2w)) == 0 ? kMotionStatic : kMotionRigid;
      }
      states[row.state]++;
   }
   if (nm) HIP_TRY(c, hipMemcpyAsync(h.mv.table.p, h.mv.rows.data(), nm * sizeof(MotionMesh), hipMemcpyHostToDevice, c->stream));
   std::memcpy(h.mv.states, states, sizeof(states));
   h.mv.blocks = motion_blocks(c->W * c->H, c->num_cus);
   if (h.mv.blocks > uh_ctx::Hybrid::Motion::kMaxBlocks) return fail(c, UH_ERR_CAPACITY, std::string(who) + ": a device of more than 1024 compute units");
   md = MotionDev{h.mv.image.p, h.mv.table.p, h.mv.prev.p, h.mv.counters.p};
   return UH_OK;
}

// behind a motion pass, on its stream: the positions of the meshes whose vertices changed since the last snapshot (all of them the
// first time and when a mesh was added: the rows are laid out again), and every mesh's transform and serial
static int motion_snapshot(uh_ctx* c, const LaunchCfg& lc) {
   uh_ctx::Hybrid& h = c->hy;
   const size_t nm = c->meshes.size();
   std::vector<uh_ctx::Hybrid::Motion::Snap> snap(nm);
   size_t rows = 0;
   for (size_t i = 0; i < nm; i++) {
      const HostMesh& m = c->meshes[i];
      std::memcpy(snap[i].o2w, m.o2w, sizeof(snap[i].o2w));
      snap[i].serial = m.serial;
      snap[i].base = (uint32_t)rows;
      snap[i].count = m.iso ? 0u : (uint32_t)m.num_vertices();  // an isosurface mesh is never `deformed`: no rows
      rows += snap[i].count;
   }
   const bool relayout = h.mv.snap.size() != nm || !h.mv.prev.p;
   if (relayout && h.mv.prev.n < std::max<size_t>(1, rows)) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // the pass read the old rows
      if (int st = grow(c, h.mv.prev, std::max<size_t>(1, rows), "uh_render_hybrid: motion vectors")) return st;
   }
   // one launch per run of meshes to copy whose vertices and rows both follow one another (a whole-scene update: one launch)
   size_t from = 0, to = 0, count = 0;
   const auto flush = [&] {
      if (count) launch_motion_snapshot(lc, h.vertices.p + from, h.mv.prev.p + to, (uint32_t)count);
      count = 0;
   };
   for (size_t i = 0; i < nm; i++) {
      if (!snap[i].count || (!relayout && h.mv.snap[i].serial == snap[i].serial)) continue;
      if (count && (h.layout[i].vb != from + count || snap[i].base != to + count)) flush();
      if (!count) from = h.layout[i].vb, to = snap[i].base;
      count += snap[i].count;
   }
   flush();
   HIP_TRY(c, hipGetLastError());
   h.mv.snap = std::move(snap);
   return UH_OK;
}

// ---- the rasterised G-buffer (utopian_hip.h "UH_HYBRID_GBUFFER_RASTER"; forward.hip) ----
// raster_scene into the pass's own depth, visibility and records, then gbuffer.frag into the four targets; with `motion` the motion
// pass on the same records behind it
static int render_gbuffer_raster(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, const HybridDev& hd, const MotionDev* motion) {
   uh_ctx::Hybrid& h = c->hy;
   ForwardDev fd{};
   uint32_t pieces = 0;
   if (int st = raster_scene(c, lc, view, h.gr.bins, h.gr.target, fd, "uh_render_hybrid: rasterised G-buffer", &pieces)) return st;
   launch_gbuffer_raster_shade(lc, c->scene, fd, hd);
   if (motion)
      if (int st = timed(c, h.mv.stage[0], [&] { launch_gbuffer_raster_motion(lc, c->scene, fd, hd, *motion); })) return st;
   h.gr.pieces = pieces;
   h.gr.renders++;
   return UH_OK;
}

// ---- uh_render_hybrid in four steps: plan, prepare, arguments, passes ----
// What a call does, decided from the context, the view and the mask alone - no HIP call, no state changed: `code` other than UH_OK
// with the message of the first rule the request breaks (the rules in the order utopian_hip.h gives them), or the passes that run
// and the first-use groups they need
struct HybridPlan {
   int code;
   const char* refusal;
   bool raster, maps, render_maps, restir, rtao, rtgi, mc, motion, rt, taa, post;  // maps: the IBL maps exist for this call's consumers
   bool deferred, frame, env;  // the deferred pass runs; the final frame's images and the IBL maps are needed
   bool first, frame_first;    // the ray-traced images, the final frame's images are allocated by this call (and cleared)
};
static HybridPlan hybrid_plan(const uh_ctx& c, const UhViewUniformData& view, uint32_t mask) {
   const uh_ctx::Hybrid& h = c.hy;
   HybridPlan p{};
   const auto refuse = [&p](int code, const char* why) {
      p.code = code, p.refusal = why;
      return p;
   };
   p.raster = (mask & UH_HYBRID_GBUFFER_RASTER) != 0;
   if (p.raster && !(mask & UH_HYBRID_GBUFFER))
      return refuse(UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: UH_HYBRID_GBUFFER_RASTER without UH_HYBRID_GBUFFER (the bit chooses how the G-buffer pass runs); set both, "
                  "or neither");
   // the IBL maps exist for this call's consumers when an earlier call built them or this one does, before rt_reflections
   p.maps = h.env.builds > 0 || (mask & UH_HYBRID_ENVIRONMENT);
   if ((mask & UH_HYBRID_RT_REFLECTIONS) && view.ibl_enabled == 1 && !p.maps)
      return refuse(UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: rt_reflections with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), "
                  "which are not part of this library until a call with UH_HYBRID_ENVIRONMENT builds them; set that bit, or ibl_enabled = 0 "
                  "for the reflection pass's non-IBL branch");
   p.render_maps = (mask & UH_HYBRID_SHADOW_MAPS) && view.shadows_enabled == 1;
   if (p.render_maps && !h.sm.params_set)
      return refuse(UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: UH_HYBRID_SHADOW_MAPS before uh_set_shadowmap_params (the cascades of uh_shadow_cascades or the caller's own)");
   if (mask & UH_HYBRID_DEFERRED) {
      if (view.shadows_enabled == 1 && !h.sm.size && !p.render_maps)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the deferred pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call "
                     "with UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0 for the rt_shadows branch");
      if (view.ibl_enabled == 1 && !p.maps)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the deferred pass with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), "
                     "which a call with UH_HYBRID_ENVIRONMENT builds; set that bit, or ibl_enabled = 0 for the ambient term 0.03 * diffuse * occlusion");
      if (view.num_lights > c.lights.size())
         return refuse(UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: view.num_lights exceeds the lights added with uh_add_light");
   }
   if ((mask & UH_HYBRID_SKY) && view.cubemap_enabled == 1 && !p.maps)
      return refuse(UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: the sky pass with view.cubemap_enabled = 1 needs the environment cube (ibl.rs), which a call with "
                  "UH_HYBRID_ENVIRONMENT builds; set that bit, or cubemap_enabled = 0 for the IntegrateScattering branch");
   // the reservoir lights: one shadow ray per pixel toward the light of its spatial reservoir, which the deferred pass then adds
   p.restir = (mask & UH_HYBRID_RESTIR_LIGHTS) != 0;
   if (p.restir) {
      if (view.raytracing_supported != 1)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts shadow rays and view.raytracing_supported is not 1; set it, or clear the bit");
      if (!(mask & UH_HYBRID_GBUFFER) && !h.gbuffer_done)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts its rays from the G-buffer, and no G-buffer has been rendered; set "
                     "UH_HYBRID_GBUFFER");
      if (!c.restir_recorded)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS reads the spatial reservoirs, and no reservoir pass has run on this context; "
                     "render a frame with UH_PASS_RESTIR (same camera) first");
      if (c.bands.world > 1)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS needs the whole frame's reservoirs, and a row partition with world > 1 is set "
                     "(uh_set_restir_partition)");
   }
   // ray-traced ambient occlusion takes the SSAO slot: short hemisphere rays from the G-buffer instead of ssao.frag
   p.rtao = (mask & UH_HYBRID_RTAO) && view.ssao_enabled == 1;
   if (p.rtao) {
      if (view.raytracing_supported != 1)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTAO casts occlusion rays and view.raytracing_supported is not 1; set it, or clear the bit");
      if (!(mask & UH_HYBRID_GBUFFER) && !h.gbuffer_done)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTAO casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER");
      if ((uint64_t)c.W * c.H * 64u >= (1ull << 32))
         return refuse(UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_RTAO: a frame of 2^26 pixels or more (its rays are numbered in 32 bits)");
   }
   // setup_marching_cubes_pass (mod.rs:164): only with the checkbox on
   p.mc = (mask & UH_HYBRID_MARCHING_CUBES) && view.marching_cubes_enabled == 1;
   if (p.mc) {
      if (!(mask & UH_HYBRID_GBUFFER) && !h.gbuffer_done)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the marching-cubes pass depth-tests against the G-buffer's depth, and no G-buffer has been rendered; "
                     "set UH_HYBRID_GBUFFER, or marching_cubes_enabled = 0");
      if (c.meshes.empty())
         return refuse(UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: the marching-cubes pass shades with the first mesh's material (mesh_index 0), and the scene has no mesh");
      if (view.shadows_enabled == 1 && !h.sm.size && !p.render_maps)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the marching-cubes pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a "
                     "call with UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0");
      if (view.num_lights > c.lights.size())
         return refuse(UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: the marching-cubes pass: view.num_lights exceeds the lights added with uh_add_light");
   }
   // motion vectors: a modifier of the G-buffer pass, ignored without it
   p.motion = (mask & UH_HYBRID_MOTION) && (mask & UH_HYBRID_GBUFFER);
   // temporal anti-aliasing: the resolve between the sky pass and present, over the G-buffer the call leaves
   p.taa = (mask & UH_HYBRID_TAA) != 0;
   if (p.taa) {
      if (!(mask & UH_HYBRID_GBUFFER) && !h.gbuffer_done)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_TAA reprojects the G-buffer's positions, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER");
      if ((h.taa.params.flags & UH_TAA_MOTION) && !((mask & UH_HYBRID_GBUFFER) ? p.motion : h.mv.last))
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_TAA with UH_TAA_MOTION reads the motion image, and the last G-buffer pass had no UH_HYBRID_MOTION; "
                     "set UH_HYBRID_GBUFFER | UH_HYBRID_MOTION, or clear the flag (uh_set_taa_params)");
   }
   // the HDR display chain: between the taa pass and present, over whatever the call leaves in its source; it refuses nothing
   p.post = (mask & UH_HYBRID_POST) != 0;
   // one-bounce diffuse GI: hemisphere rays from the G-buffer, shaded at their hits, added to what the deferred pass of this call wrote
   p.rtgi = (mask & UH_HYBRID_RTGI) != 0;
   if (p.rtgi) {
      if (view.raytracing_supported != 1)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTGI casts rays and view.raytracing_supported is not 1; set it, or clear the bit");
      if (!(mask & UH_HYBRID_GBUFFER) && !h.gbuffer_done)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTGI casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER");
      if (view.ibl_enabled == 1)
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTGI with view.ibl_enabled = 1: the IBL ambient term and this pass would both count the sky; "
                     "set ibl_enabled = 0, or clear the bit");
      if (!(mask & UH_HYBRID_DEFERRED))
         return refuse(UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTGI without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass "
                     "writes and has nothing to add to; set UH_HYBRID_DEFERRED");
      if ((uint64_t)c.W * c.H * 16u >= (1ull << 32))
         return refuse(UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_RTGI: a frame of 2^28 pixels or more (its rays are numbered in 32 bits)");
   }
   p.rt = view.raytracing_supported != 0;
   p.deferred = (mask & UH_HYBRID_DEFERRED) != 0;
   p.frame = (mask & (UH_HYBRID_SSAO | UH_HYBRID_DEFERRED | UH_HYBRID_SKY | UH_HYBRID_PRESENT)) || p.mc || p.rtao || p.taa || p.post;
   p.env = (mask & UH_HYBRID_ENVIRONMENT) != 0;
   p.first = !h.counter.p;
   p.frame_first = p.frame && !h.sky_counter.p;
   return p;
}

// ---- the HDR display chain (utopian_hip.h "HDR display chain"; post.hip) ----
// the pass's images, counts and record (first pass): the counts zero, as every pass leaves them
static int post_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::Post& t = c->hy.post;
   if (t.rec.p) return UH_OK;
   if (int st = stage_create(c, t.stage, 3)) return st;
   if (int st = alloc_group(c, [&](auto f) { t.images(c->W, c->H, f); })) return st;
   HIP_TRY(c, hipMemsetAsync(t.hist.p, 0, kPostBins * sizeof(uint32_t), c->stream));
   HIP_TRY(c, hipMemsetAsync(t.rec.p, 0, sizeof(PostRecord), c->stream));
   return UH_OK;
}

// the three stages over `src` on c->stream, each between its two events: uh_render_hybrid's post pass and uh_post_image
static int post_run(uh_ctx* c, const LaunchCfg& lc, const float4* src) {
   uh_ctx::Hybrid::Post& t = c->hy.post;
   const UhPostParams& p = t.params;
   PostDev pd{};
   pd.src = src;
   pd.out = t.out.p;
   pd.hist = t.hist.p, pd.hist_copy = t.hist_copy.p, pd.rec = t.rec.p;
   pd.levels = (p.flags & UH_POST_BLOOM) ? post_level_count(c->W, c->H, p.bloom_levels) : 0;
   for (uint32_t k = 0; k <= kPostMaxLevels; k++) {
      if (!post_level_dims(c->W, c->H, k, &pd.lw[k], &pd.lh[k])) pd.lw[k] = pd.lh[k] = 0;
      pd.down[k] = t.down[k].p;
      pd.up[k] = k == pd.levels ? t.down[k].p : t.up[k].p;  // up[last] = down[last]
   }
   pd.W = c->W, pd.H = c->H;
   pd.auto_exposure = (p.flags & UH_POST_AUTO_EXPOSURE) ? 1u : 0u;
   pd.have_prev = t.have_exposure ? 1u : 0u;
   pd.tonemap = p.tonemap;
   pd.manual_exposure = p.manual_exposure, pd.key = p.key, pd.min_exposure = p.min_exposure, pd.max_exposure = p.max_exposure;
   pd.adaptation = p.adaptation, pd.low_percentile = p.low_percentile, pd.high_percentile = p.high_percentile;
   pd.bloom_threshold = p.bloom_threshold, pd.bloom_intensity = p.bloom_intensity;
   for (Stage& s : t.stage) s.ran = false;
   if (int st = timed(c, t.stage[0], [&] { launch_post_meter(lc, pd); })) return st;
   t.have_exposure = true;  // from here on the record holds this pass's exposure, whatever fails below
   if (pd.levels)
      if (int st = timed(c, t.stage[1], [&] { launch_post_bloom(lc, pd); })) return st;
   if (int st = timed(c, t.stage[2], [&] { launch_post_composite(lc, pd); })) return st;
   HIP_TRY(c, hipGetLastError());
   t.metered = pd.auto_exposure != 0;
   t.levels = pd.levels;
   t.renders++;
   return UH_OK;
}

// First use: the groups the plan asks for, each allocated once (its last buffer says so), and the mesh and light tables
static int hybrid_prepare(uh_ctx* c, const HybridPlan& p) {
   uh_ctx::Hybrid& h = c->hy;
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = hybrid_alloc(c)) return st;
   if (int st = hybrid_tables(c)) return st;
   if (p.raster && !h.gr.target.covered.p)
      if (int st = alloc_group(c, [&](auto f) { h.gr.images(pixels, f); })) return st;
   if (p.frame) {
      if (int st = hybrid_frame_alloc(c)) return st;
      if (p.deferred || p.mc)
         if (int st = hybrid_light_table(c)) return st;
   }
   if (p.mc && !h.mc.target.covered.p)
      if (int st = alloc_group(c, [&](auto f) { h.mc.images(pixels, f); })) return st;
   if (p.restir) {
      if (int st = hybrid_light_table(c)) return st;
      if (!h.rl.read) HIP_TRY(c, hipEventCreateWithFlags(&h.rl.read, hipEventDisableTiming));
      if (!h.rl.counters.p) {
         if (int st = alloc_group(c, [&](auto f) { h.rl.images(pixels, f); })) return st;
         HIP_TRY(c, hipMemsetAsync(h.rl.vis.p, 0, pixels, c->stream));
         HIP_TRY(c, hipMemsetAsync(h.rl.counters.p, 0, 2 * sizeof(uint32_t), c->stream));
      }
   }
   if (p.rtao && !h.ao.counters.p) {
      if (int st = alloc_group(c, [&](auto f) { h.ao.images(pixels, f); })) return st;
      HIP_TRY(c, hipMemsetAsync(h.ao.counts.p, 0, h.ao.counts.n, c->stream));
   }
   if (p.rtgi) {
      uh_ctx::Hybrid::Rtgi& gi = h.gi;
      if (!gi.counters.p) {
         if (int st = stage_create(c, gi.stage, 4)) return st;
         if (int st = alloc_group(c, [&](auto f) { gi.images(pixels, f); })) return st;
      }
      // a record per ray: kept while they hold this pass's rays, else allocated again (the stream is waited for first: a pass in flight
      // may still use the old ones)
      const size_t rays = pixels * gi.params.samples;
      if (gi.rays.n < rays || gi.sun_rays.n < rays) {
         HIP_TRY(c, hipStreamSynchronize(c->stream));
         for (int st : {grow(c, gi.rays, rays, "uh_render_hybrid: UH_HYBRID_RTGI"), grow(c, gi.sun_rays, rays, "uh_render_hybrid: UH_HYBRID_RTGI")})
            if (st) return st;
      }
   }
   if (p.env)
      if (int st = env_alloc(c)) return st;
   if (p.taa && !h.taa.counters.p) {
      if (int st = stage_create(c, &h.taa.stage, 1)) return st;
      if (int st = alloc_group(c, [&](auto f) { h.taa.images(pixels, f); })) return st;
   }
   if (p.post)
      if (int st = post_alloc(c)) return st;
   return UH_OK;
}

HybridDev hybrid_dev(const uh_ctx* c, const UhViewUniformData& view, const float* sun) {
   const uh_ctx::Hybrid& h = c->hy;
   HybridDev hd{};
   hd.pos = h.pos.p;
   hd.nrm = h.nrm.p;
   hd.alb = h.alb.p;
   hd.pbr = h.pbr.p;
   hd.shadow = h.shadow.p;
   hd.refl = h.refl.p;
   hd.queue = h.queue.p;
   hd.counter = h.counter.p;
   hd.meshes = h.meshes.p;
   hd.vertices = h.vertices.p;
   hd.indices = h.indices.p;
   for (int a = 0; a < 3; a++) {
      hd.sun_dir[a] = sun ? sun[a] : 0.0f;
      hd.eye[a] = view.eye_pos[a];
   }
   hd.W = c->W;
   hd.H = c->H;
   hd.furnace = c->furnace ? 1u : 0u;
   return hd;
}

HybridFrameDev hybrid_frame_dev(const uh_ctx* c, const UhViewUniformData& view) {
   const uh_ctx::Hybrid& h = c->hy;
   HybridFrameDev fd{};
   fd.ssao = h.ssao.p;
   fd.deferred = h.deferred.p;
   fd.present = h.present.p;
   fd.sky_counter = h.sky_counter.p;
   fd.lights = h.lights.p;
   fd.raw_lights = h.raw_lights.p;
   std::memcpy(fd.view, view.view, sizeof(fd.view));
   std::memcpy(fd.proj, view.projection, sizeof(fd.proj));
   std::memcpy(fd.inv_view, view.inverse_view, sizeof(fd.inv_view));
   fd.num_lights = view.num_lights;
   fd.ssao_on = view.ssao_enabled == 1;
   fd.rt_on = view.raytracing_supported == 1;
   fd.fxaa_on = view.fxaa_enabled == 1;
   for (int a = 0; a < 3; a++) fd.sun_raw[a] = view.sun_dir[a];
   return fd;
}

// every stage this call runs between its two events; the passes that do not run report 0, the environment's last build stays
// (a call that only renders shadow maps leaves the passes' records as they are)
static void reset_stage_records(uh_ctx::Hybrid& h, const HybridPlan& p, uint32_t mask) {
   if ((mask & (UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT | UH_HYBRID_SHADOW_MAPS)) != UH_HYBRID_SHADOW_MAPS)
      for (int k = 0; k < kHybridPasses; k++) h.stage[k].ran = false;
   if (mask & UH_HYBRID_SHADOW_MAPS) h.stage[kStShadowMaps].ran = false;
   if (mask & UH_HYBRID_MARCHING_CUBES) h.stage[kStMarchingCubes].ran = false;
   if (p.restir) h.stage[kStRestirLights].ran = false;
   if (p.rtao) h.stage[kStRtaoTrace].ran = h.stage[kStRtaoFilter].ran = false;
   if (p.rtgi)
      for (Stage& s : h.gi.stage) s.ran = false;
}

// what the passes of one call share
struct HybridCall {
   const HybridPlan& plan;
   const UhViewUniformData& view;
   const FrameParams& fp;
   const LaunchCfg& lc;
   const HybridDev& hd;
   const HybridFrameDev& fd;
};

// the G-buffer pass: cast or rasterised, with the motion pass (`plan.motion`) on its hit records and the snapshot behind it
static int gbuffer_pass(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid& h = c->hy;
   const bool motion = k.plan.motion, raster = k.plan.raster;
   MotionDev md{};
   if (motion) {
      h.mv.last = false;  // until this pass and its snapshot are enqueued
      h.mv.stage[0].ran = h.mv.stage[1].ran = false;
      if (int st = motion_prepare(c, md)) return st;
   }
   // the camera grid when the path tracer's is built for this camera and geometry (read only: the grid's state is the path tracer's)
   float mats[32];
   std::memcpy(mats, k.fp.inv_view, sizeof(float) * 16);
   std::memcpy(mats + 16, k.fp.inv_proj, sizeof(float) * 16);
   const SunGridDev* grid = c->cam_grid_enabled && c->cam.holds(c->geom_version, mats) ? &c->cam.dev : nullptr;
   const int st = timed(c, h.stage[kStGbuffer], [&]() -> int {
      if (raster) return render_gbuffer_raster(c, k.lc, k.view, k.hd, motion ? &md : nullptr);
      if (!motion) {
         launch_hybrid_gbuffer(k.lc, k.fp, c->scene, k.hd, grid);
         return UH_OK;
      }
      // k_hybrid_motion between the cast and the resolve: it reads the hit records the cast left in the targets
      launch_hybrid_gbuffer_cast(k.lc, k.fp, c->scene, k.hd, grid);
      if (int st = timed(c, h.mv.stage[0], [&] { launch_hybrid_motion(k.lc, c->scene, k.hd, md); })) return st;
      launch_hybrid_gbuffer_resolve(k.lc, c->scene, k.hd);
      return UH_OK;
   });
   if (st) return st;
   h.gbuffer_done = true;
   h.gbuffer_rasterised = raster;
   h.mv.last = false;
   if (!motion) return UH_OK;
   if (int st = timed(c, h.mv.stage[1], [&] { return motion_snapshot(c, k.lc); })) return st;
   h.mv.renders++;
   h.mv.last = true;
   return UH_OK;
}

// setup_cubemap_pass: the cube, its irradiance and specular filters and the BRDF LUT, a stage each; the maps persist until the next build
static int environment_pass(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid& h = c->hy;
   EnvDev e{h.env.cube.p, h.env.irr.p, h.env.spec.p, h.env.lut.p, h.env.taps.p, {}, {}};
   for (int a = 0; a < 3; a++) {
      e.eye[a] = k.view.inverse_view[12 + a];  // extract_camera_position(view.view): inverse(view)[3]
      e.sun[a] = k.view.sun_dir[a];
      h.env.eye[a] = e.eye[a];
      h.env.sun[a] = e.sun[a];
   }
   void (*const build[4])(const LaunchCfg&, const EnvDev&) = {launch_env_cube, launch_env_irradiance, launch_env_specular, launch_env_brdf_lut};
   for (int s = 0; s < 4; s++)
      if (int st = timed(c, h.stage[kStEnvCube + s], [&] { build[s](k.lc, e); })) return st;
   h.env.builds++;
   return UH_OK;
}

// the rtao pass in ssao_pass's place: classify + trace into the counts, then the resolve / filter into ssao_output
static int rtao_pass(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid& h = c->hy;
   const UhRtaoParams& p = h.ao.params;
   const RtaoDev ao{h.ao.counts.p, h.ao.queue.p, h.ao.counters.p, p.samples, k.fp.frame_number * 64u, p.blur_radius, p.radius, p.strength, p.blur_normal_cos, p.blur_plane};
   int st = timed(c, h.stage[kStRtaoTrace], [&] {
      HIP_TRY(c, hipMemsetAsync(h.ao.counters.p, 0, 6 * sizeof(uint32_t), c->stream));
      LaunchCfg ac = k.lc;
      ac.count_visits = c->count_visits;  // into the pass's own counters (uh_get_rtao_visits), never UhStats
      launch_rtao_trace(ac, c->scene, k.hd, ao, h.ao.order);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, h.stage[kStRtaoFilter], [&] { launch_rtao_resolve(k.lc, k.hd, ao, h.ssao.p); }))) return st;
   h.ao.samples = p.samples;
   h.ao.renders++;
   return UH_OK;
}

// the rtgi pass behind deferred_pass: classify + closest-hit walk (which shades the rays and queues the sun rays), the sun rays' any-hit
// walk, the per-pixel mean + filter into the radiance image, then the composite into deferred_output; a stage each
static int rtgi_pass(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid::Rtgi& g = c->hy.gi;
   const UhRtgiParams& p = g.params;
   const RtgiDev gi{g.counts.p, g.radiance.p, g.mean.p, g.rays.p, g.sun_rays.p, g.queue.p, g.counters.p, p.samples, k.fp.frame_number * 64u,
                    p.blur_radius, p.max_radiance, p.intensity, p.blur_normal_cos, p.blur_plane};
   int st = timed(c, g.stage[0], [&] {
      HIP_TRY(c, hipMemsetAsync(g.counters.p, 0, g.counters.n * sizeof(uint32_t), c->stream));
      launch_rtgi_trace(k.lc, c->scene, k.hd, gi, g.order);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, g.stage[1], [&] { launch_rtgi_shadow(k.lc, c->scene, k.hd, gi); }))) return st;
   if ((st = timed(c, g.stage[2], [&] { launch_rtgi_filter(k.lc, k.hd, gi); }))) return st;
   if ((st = timed(c, g.stage[3], [&] { launch_rtgi_composite(k.lc, c->scene, k.hd, k.fd, gi); }))) return st;
   g.samples = p.samples;
   g.renders++;
   return UH_OK;
}

// the taa pass between atmosphere_pass and present_pass: deferred_output into the set that is not the history, which then becomes the
// current one (the ping-pong is the host's: the kernel is enqueued with both pointers)
static int taa_pass(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid& h = c->hy;
   uh_ctx::Hybrid::Taa& t = h.taa;
   const UhTaaParams& p = t.params;
   const int write = t.cur ^ 1;
   TaaDev td{};
   td.deferred = h.deferred.p;
   td.pos = h.pos.p;
   td.motion = (p.flags & UH_TAA_MOTION) ? h.mv.image.p : nullptr;
   td.prev_col = t.valid ? t.col[t.cur].p : nullptr;
   td.prev_n = t.valid ? t.n[t.cur].p : nullptr;
   td.col = t.col[write].p;
   td.n = t.n[write].p;
   td.counters = t.counters.p;
   td.clamp = (p.flags & UH_TAA_CLAMP) ? 1u : 0u;
   td.max_history = (float)p.max_history;
   td.alpha_min = p.alpha_min;
   td.clamp_gamma = p.clamp_gamma;
   const int st = timed(c, t.stage, [&] {
      HIP_TRY(c, hipMemsetAsync(t.counters.p, 0, t.counters.n * sizeof(uint32_t), c->stream));
      launch_hybrid_taa(k.lc, k.fp, td);
      return (int)UH_OK;
   });
   if (st) return st;
   t.cur = write;
   t.valid = true;
   t.renders++;
   return UH_OK;
}

// The passes in the order of build_render_graph (mod.rs:91-186, graph.rs:743), each between its stage's two events: setup_shadow_pass's
// four cascades first, rt_shadows, gbuffer, setup_cubemap_pass, rt_reflections, then the final frame - ssao_pass (not with
// ssao_enabled != 1, ssao.rs:27; the rtao pass takes its place), deferred_pass, the rtgi pass (an extension), setup_marching_cubes_pass, atmosphere_pass, the taa pass
// (an extension; present then reads its output), the post pass (an extension; it reads the taa pass's output or deferred_output, and
// present then reads its own), present_pass
static int hybrid_passes(uh_ctx* c, const HybridCall& k, uint32_t mask) {
   uh_ctx::Hybrid& h = c->hy;
   const HybridPlan& p = k.plan;
   const UhViewUniformData& view = k.view;
   const LaunchCfg& lc = k.lc;
   const HybridDev& hd = k.hd;
   const HybridFrameDev& fd = k.fd;
   int st = UH_OK;
   if (p.render_maps && (st = timed(c, h.stage[kStShadowMaps], [&] { return render_shadow_maps(c, lc, "uh_render_hybrid"); }))) return st;
   if (p.rt && (mask & UH_HYBRID_RT_SHADOWS) && (st = timed(c, h.stage[kStShadows], [&] { launch_hybrid_shadows(lc, c->scene, hd); }))) return st;
   if ((mask & UH_HYBRID_GBUFFER) && (st = gbuffer_pass(c, k))) return st;
   const IblMaps ibl{h.env.cube.p, h.env.irr.p, h.env.spec.p, h.env.lut.p};
   if (p.env && (st = environment_pass(c, k))) return st;
   if (p.rt && (mask & UH_HYBRID_RT_REFLECTIONS)) {
      st = timed(c, h.stage[kStReflections], [&] {
         HIP_TRY(c, hipMemsetAsync(h.counter.p, 0, sizeof(uint32_t), c->stream));
         launch_hybrid_reflections(lc, c->scene, hd, view.ibl_enabled == 1 ? &ibl : nullptr);
         return (int)UH_OK;
      });
      if (st) return st;
   }
   // restir_lights: the pixels' reservoirs (whatever the last reservoir pass left: read only) and this call's light count
   const HybridRestirDev rl{h.rl.vis.p, h.rl.queue.p, h.rl.counters.p, c->im.reservoirs[2], h.raw_lights.p,
                            (uint32_t)std::min<size_t>(view.num_lights, c->lights.size())};
   if (p.restir) {
      st = timed(c, h.stage[kStRestirLights], [&] {
         HIP_TRY(c, hipMemsetAsync(h.rl.counters.p, 0, 2 * sizeof(uint32_t), c->stream));
         launch_hybrid_restir_lights(lc, k.fp, c->scene, hd, rl);
         return (int)UH_OK;
      });
      if (st) return st;
      h.rl.renders++;
   }
   if (p.rtao) {
      if ((st = rtao_pass(c, k))) return st;
   } else if ((mask & UH_HYBRID_SSAO) && view.ssao_enabled == 1) {
      if ((st = timed(c, h.stage[kStSsao], [&] { launch_hybrid_ssao(lc, hd, fd); }))) return st;
   }
   if (p.deferred) {
      st = timed(c, h.stage[kStDeferred], [&] {
         const ShadowLookup sl{h.sm.maps.p, h.sm.dev_params.p, h.sm.size};
         launch_hybrid_deferred(lc, c->scene, hd, fd, view.ibl_enabled == 1 ? &ibl : nullptr, view.shadows_enabled == 1 ? &sl : nullptr, p.restir ? &rl : nullptr);
      });
      if (st) return st;
   }
   if (p.rtgi && (st = rtgi_pass(c, k))) return st;
   h.frame_lights = h.stage[kStDeferred].ran ? (p.restir ? 2 : view.num_lights + 1) : 0;  // with the reservoir lights: the sun and the reservoir's
   if (p.restir) {
      // a reservoir pass enqueued after this call starts behind the call's reads (the spatial ring comes round to the slot read here)
      HIP_TRY(c, hipEventRecord(h.rl.read, c->stream));
      HIP_TRY(c, hipStreamWaitEvent(c->restir_stream, h.rl.read, 0));
   }
   if (p.mc && (st = timed(c, h.stage[kStMarchingCubes], [&] { return render_mc_pass(c, lc, view); }))) return st;
   if (mask & UH_HYBRID_SKY) {
      st = timed(c, h.stage[kStSky], [&] {
         HIP_TRY(c, hipMemsetAsync(h.sky_counter.p, 0, sizeof(uint32_t), c->stream));
         launch_hybrid_sky(lc, k.fp, hd, fd, view.cubemap_enabled == 1 ? &ibl : nullptr, p.mc ? h.mc.target.vis.p : nullptr);
         return (int)UH_OK;
      });
      if (st) return st;
   }
   if (p.taa && (st = taa_pass(c, k))) return st;
   HybridFrameDev pd = fd;  // present's source: taa_output when the taa pass ran in this call
   if (p.taa) pd.deferred = h.taa.col[h.taa.cur].p;
   if (p.post) {
      if ((st = post_run(c, lc, pd.deferred))) return st;
      pd.deferred = h.post.out.p;
   }
   if ((mask & UH_HYBRID_PRESENT) && (st = timed(c, h.stage[kStPresent], [&] { launch_hybrid_present(lc, hd, pd); }))) return st;
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

int uh_render_hybrid(uh_ctx* c, const UhViewUniformData* view, uint32_t mask) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: null view");
   const HybridPlan plan = hybrid_plan(*c, *view, mask);
   if (plan.code != UH_OK) return fail(c, plan.code, plan.refusal);
   if (!c->built && c->topology_valid && view->rebuild_tlas == 1)
      if (int st = uh_refit_acceleration(c)) return st;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_render_hybrid before uh_build_acceleration");
   if (plan.raster && (c->W > 65535 || c->H > 65535))
      return fail(c, UH_ERR_CAPACITY, "uh_render_hybrid: rasterised G-buffer: a frame wider or taller than 65535 pixels");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = hybrid_prepare(c, plan)) return st;
   const FrameParams fp = make_params(c, *view);
   const HybridDev hd = hybrid_dev(c, *view, fp.sun_dir);
   if (int st = wait_frames_in_flight(c)) return st;
   LaunchCfg lc = cfg(c);
   lc.count_visits = false;  // nothing of this call goes to UhStats
   if (plan.first) launch_hybrid_clear(lc, hd);
   const HybridFrameDev fd = hybrid_frame_dev(c, *view);
   if (plan.frame_first) launch_hybrid_frame_clear(lc, hd, fd);
   reset_stage_records(c->hy, plan, mask);
   return hybrid_passes(c, HybridCall{plan, *view, fp, lc, hd, fd}, mask);
}

int uh_read_hybrid(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (!h.counter.p) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid before the first uh_render_hybrid");
   if (which < 0 || which > UH_HYBRID_GI_COUNTS) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image index must be 0..19");
   if (which >= UH_HYBRID_SSAO_IMAGE && which <= UH_HYBRID_PRESENT_OUTPUT && !h.sky_counter.p)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 6..8 before the first call with an SSAO, deferred, sky or present bit");
   if ((which == UH_HYBRID_DEPTH || which == UH_HYBRID_MARCHING_CUBES_VISIBILITY) && h.mc.renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 9..10 before the first marching-cubes pass");
   if ((which == UH_HYBRID_GBUFFER_DEPTH || which == UH_HYBRID_GBUFFER_VISIBILITY) && h.gr.renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 11..12 before the first rasterised G-buffer pass");
   if (which == UH_HYBRID_LIGHT_VISIBILITY && !h.rl.counters.p)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image 13 before the first call with UH_HYBRID_RESTIR_LIGHTS");
   if (which == UH_HYBRID_AO_COUNTS && h.ao.renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image 14 before the first rtao pass (UH_HYBRID_RTAO with view.ssao_enabled = 1)");
   if (which == UH_HYBRID_MOTION_IMAGE && h.mv.renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image 15 before the first motion pass (UH_HYBRID_GBUFFER | UH_HYBRID_MOTION)");
   if ((which == UH_HYBRID_TAA_OUTPUT || which == UH_HYBRID_TAA_HISTORY) && h.taa.renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 16..17 before the first taa pass (UH_HYBRID_TAA)");
   if ((which == UH_HYBRID_GI_RADIANCE || which == UH_HYBRID_GI_COUNTS) && h.gi.renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_read_hybrid: images 18..19 before the first rtgi pass (UH_HYBRID_RTGI); until then the image index must be 0..17");
   // image k's pixels and its bytes per pixel, in UH_HYBRID_* image order
   const std::pair<const void*, size_t> img[] = {
      {h.pos.p, sizeof(float4)}, {h.nrm.p, sizeof(float4)}, {h.alb.p, sizeof(uchar4)}, {h.pbr.p, sizeof(float4)}, {h.shadow.p, 1},
      {h.refl.p, sizeof(uchar4)}, {h.ssao.p, sizeof(uint16_t)}, {h.deferred.p, sizeof(float4)}, {h.present.p, sizeof(uchar4)},
      {h.mc.target.depth.p, sizeof(float)}, {h.mc.target.vis.p, sizeof(uint32_t)}, {h.gr.target.depth.p, sizeof(float)}, {h.gr.target.vis.p, sizeof(uint32_t)},
      {h.rl.vis.p, 1}, {h.ao.counts.p, 1}, {h.mv.image.p, sizeof(float4)},
      {h.taa.col[h.taa.cur].p, sizeof(float4)}, {h.taa.n[h.taa.cur].p, sizeof(float)},
      {h.gi.radiance.p, sizeof(float4)}, {h.gi.counts.p, sizeof(uint32_t)}};
   return read_back(c, out, img[which].first, (size_t)c->W * c->H * img[which].second);
}

int uh_get_hybrid_frame_stats(uh_ctx* c, UhHybridFrameStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_hybrid_frame_stats: null destination", c && c->hy.counter.p, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   for (int k = 0; k < kHybridPasses; k++)
      if ((st = stage_ms(c, c->hy.stage[k], &out->pass_ms[k]))) return st;
   if (h.stage[kStSky].ran) HIP_TRY(c, hipMemcpy(&out->sky_pixels, h.sky_counter.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   out->lights = h.frame_lights;
   return UH_OK;
}

int uh_get_hybrid_restir_stats(uh_ctx* c, UhHybridRestirStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_hybrid_restir_stats: null destination", c && c->hy.rl.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, c->hy.stage[kStRestirLights], &out->pass_ms))) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, h.rl.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->rays = counters[0];
   out->occluded = counters[1];
   return UH_OK;
}

// ---- ray-traced ambient occlusion (utopian_hip.h "UH_HYBRID_RTAO"; rtao.hip) ----
int uh_rtao_default_params(UhRtaoParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhRtaoParams{4, 1.0f, 1.0f, 2, 0.9f, 0.05f};
   return UH_OK;
}

static const char* rtao_params_refusal(const UhRtaoParams& p) {
   if (p.samples < 1 || p.samples > 64) return "samples must be 1..64";
   if (!(p.radius > 0.0f && p.radius <= 10000.0f)) return "radius must be finite, > 0 and <= 10000";
   if (!(p.strength >= 0.0f && p.strength < INFINITY)) return "strength must be finite and >= 0";
   if (p.blur_radius > 4) return "blur_radius must be 0..4";
   if (std::isnan(p.blur_normal_cos) || std::isnan(p.blur_plane)) return "blur_normal_cos and blur_plane must not be NaN";
   return nullptr;
}

int uh_set_rtao_params(uh_ctx* c, const UhRtaoParams* params) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!params) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_rtao_params: null params");
   if (const char* why = rtao_params_refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string("uh_set_rtao_params: ") + why);
   c->hy.ao.params = *params;
   return UH_OK;
}

int uh_get_rtao_stats(uh_ctx* c, UhRtaoStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_rtao_stats: null destination", c && c->hy.ao.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, c->hy.stage[kStRtaoTrace], &out->trace_ms))) return st;
   if ((st = stage_ms(c, c->hy.stage[kStRtaoFilter], &out->filter_ms))) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, h.ao.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->rays = (uint64_t)counters[0] * h.ao.samples;
   out->occluded = counters[1];
   return UH_OK;
}

int uh_get_rtao_visits(uh_ctx* c, uint64_t* nodes, uint64_t* triangles) {
   int st;
   if (c && nodes && triangles) *triangles = 0;  // (*nodes: by stats_begin)
   if (!stats_begin(c, nodes && triangles ? nodes : nullptr, sizeof(*nodes), "uh_get_rtao_visits: null destination", c && c->hy.ao.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   uint64_t visits[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(visits, h.ao.counters.p + 2, sizeof(visits), hipMemcpyDeviceToHost));
   *nodes = visits[0];
   *triangles = visits[1];
   return UH_OK;
}

// ---- one-bounce ray-traced diffuse GI (utopian_hip.h "UH_HYBRID_RTGI"; rtgi.hip) ----
int uh_rtgi_default_params(UhRtgiParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhRtgiParams{2, 3, 16.0f, 1.0f, 0.9f, 0.05f};
   return UH_OK;
}

static const char* rtgi_params_refusal(const UhRtgiParams& p) {
   if (p.samples < 1 || p.samples > 16) return "samples must be 1..16";
   if (p.blur_radius > 6) return "blur_radius must be 0..6";
   if (!(p.max_radiance > 0.0f && p.max_radiance < INFINITY)) return "max_radiance must be finite and > 0";
   if (!(p.intensity >= 0.0f && p.intensity < INFINITY)) return "intensity must be finite and >= 0";
   if (std::isnan(p.blur_normal_cos) || std::isnan(p.blur_plane)) return "blur_normal_cos and blur_plane must not be NaN";
   return nullptr;
}

int uh_set_rtgi_params(uh_ctx* c, const UhRtgiParams* params) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!params) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_rtgi_params: null params");
   if (const char* why = rtgi_params_refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string("uh_set_rtgi_params: ") + why);
   c->hy.gi.params = *params;
   return UH_OK;
}

int uh_get_rtgi_stats(uh_ctx* c, UhRtgiStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_rtgi_stats: null destination", c && c->hy.gi.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Rtgi& g = c->hy.gi;
   float* const ms[4] = {&out->trace_ms, &out->shadow_ms, &out->filter_ms, &out->composite_ms};
   for (int k = 0; k < 4; k++)
      if ((st = stage_ms(c, g.stage[k], ms[k]))) return st;
   uint32_t counters[3] = {0, 0, 0};
   HIP_TRY(c, hipMemcpy(counters, g.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->rays = (uint64_t)counters[0] * g.samples;
   out->shadow_rays = counters[1];
   out->misses = counters[2];
   return UH_OK;
}

int uh_get_motion_stats(uh_ctx* c, UhMotionStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_motion_stats: null destination", c && c->hy.mv.renders != 0, &st)) return st;
   uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, h.mv.stage[0], &out->motion_ms))) return st;
   if ((st = stage_ms(c, h.mv.stage[1], &out->snapshot_ms))) return st;
   std::vector<uint32_t> counts(2 * (size_t)h.mv.blocks);  // a pair per block of the kernel's grid
   HIP_TRY(c, hipMemcpy(counts.data(), h.mv.counters.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   for (uint32_t b = 0; b < h.mv.blocks; b++) out->pixels_with += counts[2 * b], out->pixels_without += counts[2 * b + 1];
   out->meshes_static = h.mv.states[kMotionStatic];
   out->meshes_rigid = h.mv.states[kMotionRigid];
   out->meshes_deformed = h.mv.states[kMotionDeformed];
   out->meshes_none = h.mv.states[kMotionNone];
   return UH_OK;
}

// ---- temporal anti-aliasing (utopian_hip.h "temporal anti-aliasing"; taa.hip) ----
int uh_taa_default_params(UhTaaParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhTaaParams{UH_TAA_CLAMP, 16, 0.1f, 1.0f};
   return UH_OK;
}

static const char* taa_params_refusal(const UhTaaParams& p) {
   if (p.flags & ~(uint32_t)(UH_TAA_CLAMP | UH_TAA_MOTION)) return "unknown flag bits (UH_TAA_CLAMP, UH_TAA_MOTION)";
   if (p.max_history < 1) return "max_history must be >= 1";
   if (!(p.alpha_min >= 0.0f && p.alpha_min <= 1.0f)) return "alpha_min must be in [0, 1]";
   if (!(p.clamp_gamma >= 0.0f && p.clamp_gamma < INFINITY)) return "clamp_gamma must be finite and >= 0";
   return nullptr;
}

int uh_set_taa_params(uh_ctx* c, const UhTaaParams* params) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!params) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_taa_params: null params");
   if (const char* why = taa_params_refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string("uh_set_taa_params: ") + why);
   c->hy.taa.params = *params;
   return UH_OK;
}

int uh_reset_taa_history(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (c->hy.taa.counters.p) {
      HIP_TRY(c, hipSetDevice(c->device));
      if (int st = sync_all(c)) return st;
   }
   c->hy.taa.valid = false;
   return UH_OK;
}

int uh_get_taa_stats(uh_ctx* c, UhTaaStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_taa_stats: null destination", c && c->hy.taa.renders != 0, &st)) return st;
   uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, h.taa.stage, &out->taa_ms))) return st;
   std::vector<uint32_t> counters(h.taa.counters.n);  // a pair per slot, a line apart
   HIP_TRY(c, hipMemcpy(counters.data(), h.taa.counters.p, counters.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   for (uint32_t s = 0; s < kTaaCounterSlots; s++)
      out->history_pixels += counters[(size_t)s * kTaaCounterStride], out->reset_pixels += counters[(size_t)s * kTaaCounterStride + 1];
   return UH_OK;
}

// ---- the HDR display chain (utopian_hip.h "HDR display chain"; post.hip) ----
int uh_post_default_params(UhPostParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhPostParams{UH_POST_AUTO_EXPOSURE | UH_POST_BLOOM, UH_TONEMAP_ACES, 6, 1.0f, 0.18f, 0.015625f, 64.0f, 0.1f, 0.5f, 0.95f, 1.0f, 0.04f};
   return UH_OK;
}

static const char* post_params_refusal(const UhPostParams& p) {
   const auto exposure_ok = [](float v) { return v > 0.0f && v <= 65536.0f; };  // (a NaN fails both compares)
   if (p.flags & ~(uint32_t)(UH_POST_AUTO_EXPOSURE | UH_POST_BLOOM)) return "unknown flag bits (UH_POST_AUTO_EXPOSURE, UH_POST_BLOOM)";
   if (p.tonemap > UH_TONEMAP_ACES) return "tonemap must be 0..2 (UH_TONEMAP_NONE, UH_TONEMAP_REINHARD, UH_TONEMAP_ACES)";
   if (p.bloom_levels < 1 || p.bloom_levels > kPostMaxLevels) return "bloom_levels must be 1..8";
   if (!exposure_ok(p.manual_exposure) || !exposure_ok(p.key) || !exposure_ok(p.min_exposure) || !exposure_ok(p.max_exposure))
      return "manual_exposure, key, min_exposure and max_exposure must be finite and in (0, 65536]";
   if (p.min_exposure > p.max_exposure) return "min_exposure must not exceed max_exposure";
   if (!(p.adaptation > 0.0f && p.adaptation <= 1.0f)) return "adaptation must be in (0, 1]";
   if (!(p.low_percentile >= 0.0f && p.low_percentile < p.high_percentile && p.high_percentile <= 1.0f))
      return "percentiles must be 0 <= low_percentile < high_percentile <= 1";
   if (!(p.bloom_threshold >= 0.0f && p.bloom_threshold <= 65536.0f) || !(p.bloom_intensity >= 0.0f && p.bloom_intensity <= 65536.0f))
      return "bloom_threshold and bloom_intensity must be finite and in [0, 65536]";
   return nullptr;
}

int uh_set_post_params(uh_ctx* c, const UhPostParams* params) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!params) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_post_params: null params");
   if (const char* why = post_params_refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string("uh_set_post_params: ") + why);
   c->hy.post.params = *params;
   return UH_OK;
}

int uh_reset_post_exposure(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   c->hy.post.have_exposure = false;  // a pass already enqueued took the flag with it
   return UH_OK;
}

int uh_post_image(uh_ctx* c, const float* rgba32f) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!rgba32f) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_post_image: null image");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Hybrid::Post& t = c->hy.post;
   if (int st = hybrid_events(c)) return st;
   if (int st = post_alloc(c)) return st;
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = grow(c, t.input, pixels, "uh_post_image")) return st;
   if (int st = sync_all(c)) return st;  // an earlier pass may still read the upload buffer
   HIP_TRY(c, hipMemcpy(t.input.p, rgba32f, pixels * sizeof(float4), hipMemcpyHostToDevice));
   if (int st = post_run(c, cfg(c), t.input.p)) return st;
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return UH_OK;
}

int uh_post_level_size(uint32_t W, uint32_t H, uint32_t level, uint32_t* w, uint32_t* h) {
   if (!w || !h) return UH_ERR_INVALID_ARGUMENT;
   return post_level_dims(W, H, level, w, h) ? UH_OK : UH_ERR_INVALID_ARGUMENT;
}

int uh_read_post(uh_ctx* c, int which, int level, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid::Post& t = c->hy.post;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: null destination");
   if (t.renders == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post before the first post pass (UH_HYBRID_POST or uh_post_image)");
   if (which < UH_POST_OUTPUT || which > UH_POST_HISTOGRAM) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: image must be 0..3");
   if (which == UH_POST_OUTPUT || which == UH_POST_HISTOGRAM) {
      if (level != 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: post_output and the histogram have level 0 only");
      if (which == UH_POST_OUTPUT) return read_back(c, out, t.out.p, (size_t)c->W * c->H * sizeof(float4));
      if (!t.metered) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: the last pass took no histogram (UH_POST_AUTO_EXPOSURE was not set)");
      return read_back(c, out, t.hist_copy.p, kPostBins * sizeof(uint32_t));
   }
   if (level < 1 || (uint32_t)level > t.levels)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: a bloom level the last pass did not build (1..UhPostStats::levels)");
   const float4* img = which == UH_POST_BLOOM_DOWN || (uint32_t)level == t.levels ? t.down[level].p : t.up[level].p;
   return read_back(c, out, img, post_level_texels(c->W, c->H, (uint32_t)level) * sizeof(float4));
}

int uh_get_post_stats(uh_ctx* c, UhPostStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_post_stats: null destination", c && c->hy.post.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Post& t = c->hy.post;
   PostRecord r;
   HIP_TRY(c, hipMemcpy(&r, t.rec.p, sizeof(r), hipMemcpyDeviceToHost));
   out->exposure = r.exposure, out->target_exposure = r.target, out->average_luminance = r.lavg;
   out->metered_pixels = r.metered, out->bad_pixels = r.bad, out->levels = t.levels;
   if ((st = stage_ms(c, t.stage[0], &out->meter_ms))) return st;
   if ((st = stage_ms(c, t.stage[1], &out->bloom_ms))) return st;
   if ((st = stage_ms(c, t.stage[2], &out->tonemap_ms))) return st;
   out->renders = t.renders;
   return UH_OK;
}

// element i (from 1) of the Halton sequence in base b, less 0.5: the radical inverse in double, rounded to float once and kept below 0.5
static float halton_centred(uint64_t i, uint32_t b) {
   double f = 1.0, r = 0.0;
   for (; i; i /= b) {
      f /= (double)b;
      r += f * (double)(i % b);
   }
   return std::fmin((float)(r - 0.5), 0.49999997f);
}

int uh_taa_jitter(uint32_t index, float out[2]) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   out[0] = halton_centred((uint64_t)index + 1, 2);
   out[1] = halton_centred((uint64_t)index + 1, 3);
   return UH_OK;
}

int uh_get_marching_cubes_stats(uh_ctx* c, UhMarchingCubesStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_marching_cubes_stats: null destination", c && c->hy.mc.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, c->hy.stage[kStMarchingCubes], &out->pass_ms))) return st;
   out->renders = h.mc.renders;
   out->triangles = h.mc.tris;
   out->pieces = h.mc.pieces;
   HIP_TRY(c, hipMemcpy(&out->covered_pixels, h.mc.target.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   out->lights = h.mc.lights_used;
   out->time = h.mc.time;
   return UH_OK;
}

int uh_get_gbuffer_raster_stats(uh_ctx* c, UhGbufferRasterStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_gbuffer_raster_stats: null destination", c && c->hy.gr.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if (h.gbuffer_rasterised)  // the G-buffer stage's record is the last rasterised pass's
      if ((st = stage_ms(c, c->hy.stage[kStGbuffer], &out->pass_ms))) return st;
   out->renders = h.gr.renders;
   out->pieces = h.gr.pieces;
   HIP_TRY(c, hipMemcpy(&out->covered_pixels, h.gr.target.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   return UH_OK;
}

int uh_read_environment(uh_ctx* c, int which, int face, int mip, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (h.env.builds == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment before the first call with UH_HYBRID_ENVIRONMENT");
   if (which == UH_ENV_BRDF_LUT) {
      if (face != 0 || mip != 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: the BRDF LUT has face 0 and mip 0 only");
      return read_back(c, out, h.env.lut.p, (size_t)kLutSize * kLutSize * sizeof(uint32_t));
   }
   if (which < UH_ENV_ENVIRONMENT || which > UH_ENV_SPECULAR) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: map must be 0..3");
   const int mips = which == UH_ENV_IRRADIANCE ? 1 : (int)kEnvMips;
   if (face < 0 || face > 5 || mip < 0 || mip >= mips) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: face 0..5, mip 0..7 (irradiance: 0)");
   const size_t S = kEnvSize >> mip;
   const float4* base = which == UH_ENV_ENVIRONMENT ? h.env.cube.p : which == UH_ENV_IRRADIANCE ? h.env.irr.p : h.env.spec.p;
   return read_back(c, out, base + env_mip_offset((uint32_t)mip) + (size_t)face * S * S, S * S * sizeof(float4));
}

int uh_get_environment_stats(uh_ctx* c, UhEnvironmentStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_environment_stats: null destination", c && c->hy.env.builds != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   for (int k = 0; k < 4; k++)
      if ((st = stage_ms(c, c->hy.stage[kStEnvCube + k], &out->pass_ms[k]))) return st;
   out->builds = h.env.builds;
   std::memcpy(out->sun_dir, h.env.sun, sizeof(out->sun_dir));
   std::memcpy(out->eye, h.env.eye, sizeof(out->eye));
   return UH_OK;
}

int uh_get_hybrid_stats(uh_ctx* c, UhHybridStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_hybrid_stats: null destination", c && c->hy.counter.p, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   uint32_t metal = 0;
   if (h.stage[kStReflections].ran) HIP_TRY(c, hipMemcpy(&metal, h.counter.p, sizeof(metal), hipMemcpyDeviceToHost));
   const uint64_t n = (uint64_t)c->W * c->H;
   out->rays[0] = h.stage[kStGbuffer].ran && !h.gbuffer_rasterised ? n : 0;  // a rasterised pass casts no ray
   out->rays[1] = h.stage[kStShadows].ran ? n : 0;
   out->rays[2] = metal;
   out->reflection_pixels = metal;
   const int stages[3] = {kStGbuffer, kStShadows, kStReflections};  // the header's order
   for (int k = 0; k < 3; k++)
      if ((st = stage_ms(c, c->hy.stage[stages[k]], &out->pass_ms[k]))) return st;
   return UH_OK;
}

