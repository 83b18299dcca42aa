// hybrid_graph.hip - uh_render_hybrid of include/utopian_hip.h: the context's facts for the plan of a call (hybrid_plan.h: which passes
// run, or why it is refused), first use of what they need as a list of calls and the passes in their order; and what the forward graph
// and the denoiser share with it: the mesh and light tables, the wait behind the frames in flight and destroy_graphs. The passes that
// cast rays from the G-buffer - first use, run and verbs - are hybrid_ray_passes.hip, the other read, stats and params verbs
// hybrid_verbs.hip, the HDR display chain post_graph.hip. Host code over uh_ctx::Hybrid (context_state.h); the rasterised passes go through raster_driver.hip.
// Host-side counterpart of build_render_graph (utopian/src/renderers/mod.rs).
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
   if (int st = first_use(c, h.mv, h.mv.counters.p, [&](auto f) { h.mv.images((size_t)c->W * c->H, f); })) return st;
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
// What hybrid_plan (hybrid_plan.h) decides a call from: the context's facts, read and nothing else
static HybridFacts hybrid_facts(const uh_ctx& c) {
   const uh_ctx::Hybrid& h = c.hy;
   HybridFacts f{};
   f.W = c.W, f.H = c.H, f.world = c.bands.world;
   f.lights = c.lights.size();
   f.has_mesh = !c.meshes.empty(), f.restir_recorded = c.restir_recorded;
   f.maps_built = h.env.builds > 0;
   f.cascades_set = h.sm.params_set, f.cascades_rendered = h.sm.size != 0;
   f.gbuffer_done = h.gbuffer_done, f.motion_last = h.mv.last;
   f.taa_flags = h.taa.params.flags;
   f.rt_images = h.counter.p != nullptr, f.frame_images = h.sky_counter.p != nullptr;
   return f;
}

// First use: the groups the plan asks for, each allocated once (its last buffer says so), and the mesh and light tables
static int hybrid_prepare(uh_ctx* c, const HybridPlan& p) {
   uh_ctx::Hybrid& h = c->hy;
   const size_t pixels = (size_t)c->W * c->H;
   int st = UH_OK;
   if ((st = hybrid_alloc(c)) || (st = hybrid_tables(c))) return st;
   if (p.raster && !h.gr.target.covered.p && (st = alloc_group(c, [&](auto f) { h.gr.images(pixels, f); }))) return st;
   if (p.frame && (st = hybrid_frame_alloc(c))) return st;
   if (p.frame && (p.deferred || p.mc) && (st = hybrid_light_table(c))) return st;
   if (p.mc && !h.mc.target.covered.p && (st = alloc_group(c, [&](auto f) { h.mc.images(pixels, f); }))) return st;
   if (p.restir && (st = restir_lights_alloc(c))) return st;
   if (p.rtao && (st = rtao_alloc(c))) return st;
   if (p.rtgi && (st = rtgi_alloc(c))) return st;
   if (p.glossy && (st = glossy_alloc(c))) return st;
   if (p.glass && (st = glass_alloc(c))) return st;
   if (p.fog && (st = fog_alloc(c))) return st;
   if (p.area && (st = area_lights_alloc(c))) return st;
   if (p.env && (st = env_alloc(c))) return st;
   if (p.taa && (st = first_use(c, h.taa, h.taa.counters.p, [&](auto f) { h.taa.images(pixels, f); }))) return st;
   if (p.post && (st = post_alloc(c))) return st;
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
   const auto not_run = [](Stage& s) { s.ran = false; };
   if (p.restir) h.stage[kStRestirLights].ran = false;
   if (p.rtao) h.stage[kStRtaoTrace].ran = h.stage[kStRtaoFilter].ran = false;
   if (p.rtgi) h.gi.stages(not_run);
   if (p.glossy) h.gl.stages(not_run);
   if (p.glass) h.glass.stages(not_run);
   if (p.fog) h.fog.stages(not_run);
   if (p.area)
      for (Stage& s : h.area.stage) not_run(s);  // (its table stage keeps the last build's time)
}

// the G-buffer pass: cast or rasterised, with the motion pass (`plan.motion`) on its hit records and the snapshot behind it
static int gbuffer_pass(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid& h = c->hy;
   const bool motion = k.plan.motion, raster = k.plan.raster;
   MotionDev md{};
   if (motion) {
      h.mv.last = false;  // until this pass and its snapshot are enqueued
      h.mv.stages([](Stage& s) { s.ran = false; });
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
// ssao_enabled != 1, ssao.rs:27; the rtao pass takes its place), deferred_pass, the area-light, rtgi, glossy and glass passes (extensions), setup_marching_cubes_pass, atmosphere_pass, the fog pass (an
// extension; it attenuates and in-scatters into what the deferred and sky passes wrote), the taa pass
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
   const HybridRestirDev rl = restir_lights_dev(c, view);
   if (p.restir && (st = restir_lights_run(c, k, rl))) return st;
   if (p.rtao) {
      if ((st = rtao_run(c, k))) return st;
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
   if (p.area && (st = area_lights_run(c, k))) return st;
   if (p.rtgi && (st = rtgi_run(c, k))) return st;
   if (p.glossy && (st = glossy_run(c, k))) return st;
   if (p.glass && (st = glass_run(c, k))) return st;
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
   if (p.fog && (st = fog_run(c, k))) return st;
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
   const HybridPlan plan = hybrid_plan(hybrid_facts(*c), *view, mask);
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
