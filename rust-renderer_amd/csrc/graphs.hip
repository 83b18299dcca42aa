// graphs.hip - the hybrid graph (uh_render_hybrid: the ray-traced passes, the final frame, the IBL maps, the cascaded shadow maps, the
// marching-cubes pass, the rasterised G-buffer), the forward graph (uh_render_forward) and the denoiser (uh_denoise) of
// include/utopian_hip.h: host code over uh_ctx::Hybrid, uh_ctx::Forward and uh_ctx::Denoise (context_state.h). Host-side counterpart of build_render_graph and
// build_minimal_forward_render_graph (utopian/src/renderers/mod.rs).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "context_state.h"
#include "device_scan.h"
#include "motion_device.h"

// ---- the timed stages of both graphs (context_state.h Stage) ----
// a stage runs between its two events on the graph's stream; stage_ms: its time in the last call that ran it, 0 when that did not
static int stage_create(uh_ctx* c, Stage* s, int n) {
   for (int k = 0; k < n; k++)
      for (hipEvent_t* ev : {&s[k].begin, &s[k].end})
         if (!*ev) HIP_TRY(c, hipEventCreate(ev));
   return UH_OK;
}
static void stage_destroy(Stage* s, int n) {
   for (int k = 0; k < n; k++)
      for (hipEvent_t ev : {s[k].begin, s[k].end})
         if (ev) (void)hipEventDestroy(ev);
}
static hipError_t stage_begin(Stage& s, hipStream_t stream) {
   const hipError_t e = hipEventRecord(s.begin, stream);
   s.ran = e == hipSuccess;  // no time for a stage that did not begin
   s.timed = false;
   return e;
}
static hipError_t stage_end(Stage& s, hipStream_t stream) { return hipEventRecord(s.end, stream); }
static int stage_ms(uh_ctx* c, Stage& s, float* out) {
   *out = 0.0f;
   if (!s.ran) return UH_OK;
   if (!s.timed) {
      HIP_TRY(c, hipEventElapsedTime(&s.ms, s.begin, s.end));
      s.timed = true;
   }
   *out = s.ms;
   return UH_OK;
}

// ---- the hybrid graph's ray-traced passes (utopian_hip.h "uh_render_hybrid") ----
// allocates one of uh_ctx::Hybrid's groups, visit(f) naming its buffers; stops at the first error, before the group's last buffer
template <class Visit> static int alloc_group(uh_ctx* c, Visit visit) {
   hipError_t e = hipSuccess;
   visit([&e](auto& b, size_t n) {
      if (e == hipSuccess) e = b.alloc(n);
   });
   if (e != hipSuccess)
      return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string("uh_render_hybrid: allocation: ") + hipGetErrorString(e));
   return UH_OK;
}

// the events of the hybrid stages and of the waits behind the frames in flight (first hybrid or forward call)
static int hybrid_events(uh_ctx* c) {
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

// everything the two graphs own (uh_destroy)
void destroy_graphs(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   const auto release = [](auto& b, size_t) { b.release(); };
   h.rt_images(0, release);
   h.frame_images(0, release);
   h.env_maps(release);
   h.shadow_maps(release);
   h.mc_images(0, release);
   h.restir_images(0, release);
   h.rtao_images(0, release);
   h.motion_images(0, release);
   stage_destroy(h.mv_stage, 2);
   if (h.rl_read) (void)hipEventDestroy(h.rl_read);
   h.mc_bins.each(release);
   h.gr.each(0, release);
   h.gr_bins.each(release);
   h.meshes.release();
   h.vertices.release();
   h.indices.release();
   h.raw_lights.release();
   h.taps.release();
   for (hipEvent_t ev : h.waits)
      if (ev) (void)hipEventDestroy(ev);
   stage_destroy(h.stage, kHybridStages);
   uh_ctx::Forward& f = c->fw;
   f.images(0, release);
   f.bins.each(release);
   stage_destroy(f.stage, 3);
   uh_ctx::Denoise& d = c->dn;
   d.images(0, release);
   stage_destroy(d.stage, 4);
   if (d.acc_read) {
      if (c->last_acc == d.acc_read) c->last_acc = nullptr;
      (void)hipEventDestroy(d.acc_read);
   }
}

// the meshes as the vertex and fragment shaders read them: vertices, indices, the instance's world matrix and the material's maps
static int hybrid_tables(uh_ctx* c) {
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
static int hybrid_light_table(uh_ctx* c) {
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
   if (h.lut.p) return UH_OK;
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
   HIP_TRY(c, h.taps.alloc(taps.size()));
   HIP_TRY(c, hipMemcpyAsync(h.taps.p, taps.data(), taps.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return alloc_group(c, [&](auto f) { h.env_maps(f); });
}

// ---- what the rasterised passes share ----
// b holds n elements or more: kept when it does, allocated again (its contents lost) when not
template <class Buf> static int grow(uh_ctx* c, Buf& b, size_t n, const char* prefix) {
   if (b.p && b.n >= n) return UH_OK;
   const hipError_t e = b.alloc(n);
   if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string(prefix) + ": allocation: " + hipGetErrorString(e));
   return UH_OK;
}

// One rasterised pass's binning, from its count kernel to its resolve kernel; the records' and tile entries' totals come back to the
// host in between (the buffers grow to them). The caller has sized and zeroed b.tile_count and sized tile_cursor, totals, chunks
// (for the longer of the two scans) and rec_count.
struct BinPass {
   size_t units;                   // count units in b.rec_count: triangles (the cascades: 4 x triangles)
   uint32_t tiles;
   size_t record_quads;            // uint4s per record
   unsigned long long max_pieces;  // exclusive: 2^32 less the record ids the pass's resolve key reserves
   const char* prefix;             // of every message
   const char* too_many;           // the rest of the capacity message
};
static const char* const kForwardTooMany = ": 2^32 - 1 or more triangle pieces, or 2^32 or more tile entries";
// count(): the pass's count kernel; after_wait(): the caller's own reads once the scans have completed (an int status);
// emit_resolve(): its emit and resolve kernels, b.records and b.entries sized. totals: records, tile entries.
template <class Count, class AfterWait, class EmitResolve>
static int bin_and_resolve(uh_ctx* c, RasterBins& b, const BinPass& p, unsigned long long totals[2], Count count, AfterWait after_wait, EmitResolve emit_resolve) {
   count();
   totals[0] = totals[1] = 0;
   if (p.units) device_exclusive_scan_u32(b.rec_count.p, (uint32_t)p.units, b.chunks.p, b.totals.p, c->stream);
   device_exclusive_scan_u32(b.tile_count.p, p.tiles, b.chunks.p, b.totals.p + 1, c->stream);
   HIP_TRY(c, hipMemcpyAsync(b.tile_cursor.p, b.tile_count.p, p.tiles * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   HIP_TRY(c, hipMemcpy(totals + 1, b.totals.p + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost));
   if (p.units) HIP_TRY(c, hipMemcpy(totals, b.totals.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
   if (int st = after_wait()) return st;
   if (totals[0] >= p.max_pieces || totals[1] >= (1ull << 32)) return fail(c, UH_ERR_CAPACITY, std::string(p.prefix) + p.too_many);
   for (int st : {grow(c, b.records, std::max<size_t>(1, p.record_quads * (size_t)totals[0]), p.prefix), grow(c, b.entries, std::max<size_t>(1, (size_t)totals[1]), p.prefix)})
      if (st) return st;
   emit_resolve();
   return UH_OK;
}

// the column-major product a b, element (r, c) summed ((a(r,0) b(0,c) + a(r,1) b(1,c)) + a(r,2) b(2,c)) + a(r,3) b(3,c)
static void mat4_mul(const float* a, const float* b, float* o) {
   for (int col = 0; col < 4; col++)
      for (int r = 0; r < 4; r++) o[4 * col + r] = ((a[r] * b[4 * col] + a[4 + r] * b[4 * col + 1]) + a[8 + r] * b[4 * col + 2]) + a[12 + r] * b[4 * col + 3];
}
// an instance's 3x4 (HostMesh::o2w, row-major) with row (0, 0, 0, 1), column-major
static void mat4_from_3x4(const float* o, float* w) {
   for (int col = 0; col < 4; col++) {
      for (int r = 0; r < 3; r++) w[4 * col + r] = o[4 * r + col];
      w[4 * col + 3] = col == 3 ? 1.0f : 0.0f;
   }
}

// the frame and its tile grid into fd, with t as what it resolves into; returns the tiles
static uint32_t forward_frame(const uh_ctx* c, const RasterTarget& t, ForwardDev& fd) {
   fd.W = c->W;
   fd.H = c->H;
   fd.tiles_x = (c->W + kForwardTile - 1) / kForwardTile;
   fd.tiles_y = (c->H + kForwardTile - 1) / kForwardTile;
   fd.depth = t.depth.p;
   fd.vis = t.vis.p;
   fd.rec_of = t.rec_of.p;
   fd.covered = t.covered.p;
   return fd.tiles_x * fd.tiles_y;
}

// k_hybrid_light_prep into the pass's own records (the sun first), then forward.frag over fd's surviving records
static void light_and_shade(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, const ForwardDev& fd, HybridLight* lights, bool flat) {
   const uh_ctx::Hybrid& h = c->hy;
   HybridFrameDev lp{};
   lp.lights = lights;
   lp.raw_lights = h.raw_lights.p;
   lp.num_lights = view.num_lights;
   for (int a = 0; a < 3; a++) lp.sun_raw[a] = view.sun_dir[a];
   launch_hybrid_light_prep(lc, lp);
   ForwardShade fs{};
   fs.lights = lights;
   fs.count = view.num_lights + 1;
   for (int a = 0; a < 3; a++) fs.eye[a] = view.eye_pos[a];
   std::memcpy(fs.view, view.view, sizeof(fs.view));
   const ShadowLookup sl{h.smaps.p, h.s_params.p, h.smap_size};
   launch_forward_shade(lc, c->scene, fd, fs, view.shadows_enabled == 1 ? &sl : nullptr, flat);
}

// ---- the cascaded shadow maps (utopian_hip.h "UH_HYBRID_SHADOW_MAPS"; shadow_map.hip) ----
// vp * W for every cascade and mesh: W the instance's 3x4 from the last build or refit
static void cascade_mesh_matrices(const uh_ctx* c, const UhShadowmapParams& p, std::vector<float>& out) {
   const size_t nm = c->meshes.size();
   out.assign(4 * nm * 16, 0.0f);
   for (int k = 0; k < 4; k++) {
      for (size_t m = 0; m < nm; m++) {
         float w[16];
         mat4_from_3x4(c->meshes[m].o2w, w);
         mat4_mul(p.view_projection_matrices[k], w, &out[((size_t)k * nm + m) * 16]);
      }
   }
}

// the rasterisers' per-triangle mesh ids: made on the host and uploaded, or - once a mesh is device-resident, whose count changes with
// every update - written on the device, one fill per mesh range, on the stream the rasterisers run on
static int fill_tri_mesh(uh_ctx* c, uint32_t* dst) {
   bool any_dev = false;
   for (const HostMesh& m : c->meshes) any_dev = any_dev || m.dev;
   if (!any_dev) {
      std::vector<uint32_t> tm;
      for (size_t m = 0; m < c->meshes.size(); m++) tm.insert(tm.end(), c->meshes[m].tris(), (uint32_t)m);
      if (!tm.empty()) HIP_TRY(c, hipMemcpy(dst, tm.data(), tm.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      return UH_OK;
   }
   size_t at = 0;
   for (size_t i = 0; i < c->meshes.size(); at += c->meshes[i].tris(), i++) uhi_fill_u32(c->stream, dst + at, (uint32_t)c->meshes[i].tris(), (uint32_t)i);
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

// the four cascades through bin_and_resolve; the first record of each cascade is read with the totals
static int render_shadow_maps(uh_ctx* c, const LaunchCfg& lc, const char* verb) {
   uh_ctx::Hybrid& h = c->hy;
   RasterBins& b = h.s_bins;
   const uint32_t S = c->shadow_map_size, tiles_x = (S + kShadowTile - 1) / kShadowTile, tiles = 4 * tiles_x * tiles_x;
   size_t ntri = 0;
   for (const HostMesh& m : c->meshes) ntri += m.tris();
   if (4 * ntri >= (1ull << 32)) return fail(c, UH_ERR_CAPACITY, std::string(verb) + ": shadow maps of more than 2^30 triangles");
   for (int st : {grow(c, h.smaps, 4 * (size_t)S * S, verb), grow(c, b.tile_count, tiles, verb), grow(c, b.tile_cursor, tiles, verb), grow(c, b.totals, 2, verb),
                  grow(c, h.s_params, 1, verb), grow(c, b.mats, std::max<size_t>(1, 64 * c->meshes.size()), verb),
                  grow(c, b.chunks, std::max<size_t>(1, scan_chunk_count((uint32_t)std::max<size_t>(4 * ntri, tiles))), verb)})
      if (st) return st;
   if (b.geom != c->geom_version || !b.rec_count.p) {
      HIP_TRY(c, b.tri_mesh.alloc(std::max<size_t>(1, ntri)));
      HIP_TRY(c, b.rec_count.alloc(std::max<size_t>(1, 4 * ntri)));
      if (int st = fill_tri_mesh(c, b.tri_mesh.p)) return st;
      b.geom = c->geom_version;
   }
   // until this render completes the maps and their params are invalid: a failure below leaves the deferred pass refused
   h.smap_size = 0;
   h.pending = h.params;
   cascade_mesh_matrices(c, h.pending, b.mats_host);
   if (!b.mats_host.empty())
      HIP_TRY(c, hipMemcpyAsync(b.mats.p, b.mats_host.data(), b.mats_host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(h.s_params.p, &h.pending, sizeof(UhShadowmapParams), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemsetAsync(b.tile_count.p, 0, tiles * sizeof(uint32_t), c->stream));
   ShadowDev sd{};
   sd.vertices = h.vertices.p;
   sd.indices = h.indices.p;
   sd.meshes = h.meshes.p;
   sd.tri_mesh = b.tri_mesh.p;
   sd.mats = b.mats.p;
   sd.num_tris = (uint32_t)ntri;
   sd.num_meshes = (uint32_t)c->meshes.size();
   sd.size = S;
   sd.tiles_x = tiles_x;
   sd.rec_count = b.rec_count.p;
   sd.tile_count = b.tile_count.p;
   sd.tile_cursor = b.tile_cursor.p;
   sd.maps = h.smaps.p;
   unsigned long long totals[2];
   uint32_t first[4] = {0, 0, 0, 0};  // the first record of each cascade
   const BinPass pass{4 * ntri, tiles, 3, 1ull << 32, verb, ": shadow maps with 2^32 or more triangle pieces or tile entries"};
   const int st = bin_and_resolve(
      c, b, pass, totals, [&] { launch_shadow_count(lc, sd); },
      [&] {
         for (int k = 1; ntri && k < 4; k++) HIP_TRY(c, hipMemcpy(first + k, b.rec_count.p + k * ntri, sizeof(uint32_t), hipMemcpyDeviceToHost));
         return (int)UH_OK;
      },
      [&] {
         sd.records = b.records.p;
         sd.entries = b.entries.p;
         launch_shadow_emit(lc, sd);
         launch_shadow_resolve(lc, sd);
      });
   if (st) return st;
   for (int k = 0; k < 4; k++) h.s_tris[k] = (k < 3 ? first[k + 1] : (uint32_t)totals[0]) - first[k];
   h.snapshot = h.pending;
   h.smap_size = S;
   h.s_renders++;
   return UH_OK;
}

// behind every frame in flight: the context's first stream (slot 0's, where hybrid and forward calls run) waits for the others
static int wait_frames_in_flight(uh_ctx* c) {
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
   RasterBins& b = h.mc_bins;
   ForwardDev fd{};
   const uint32_t tiles = forward_frame(c, h.mc, fd);
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
   HIP_TRY(c, hipMemcpyAsync(h.mc_mesh.p, &mm, sizeof(mm), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(b.mats.p, mats, sizeof(mats), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemsetAsync(b.tile_count.p, 0, tiles * sizeof(uint32_t), c->stream));
   HIP_TRY(c, hipMemsetAsync(h.mc.covered.p, 0, sizeof(uint32_t), c->stream));
   // marching_cubes.comp at view.time: per-block counts, their scan, then (with the total known) the triangles
   if (!uhi_mc_extract_count(c->stream, view.time, h.mc_block_counts.p)) return fail(c, UH_ERR_HIP, "uh_render_hybrid: marching-cubes tables");
   device_exclusive_scan_u32(h.mc_block_counts.p, kMcBlocks, b.chunks.p, h.mc_total.p, c->stream);
   fd.meshes = h.mc_mesh.p;
   fd.mats = b.mats.p;
   fd.tile_count = b.tile_count.p;
   fd.tile_cursor = b.tile_cursor.p;
   fd.color = h.deferred.p;
   // the G-buffer's depth attachment (marching_cubes.rs:97, LOAD): the rasterised pass's own, or the cast's reconstruction
   if (h.gbuffer_rasterised)
      HIP_TRY(c, hipMemcpyAsync(h.mc.depth.p, h.gr.depth.p, (size_t)c->W * c->H * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
   else
      launch_mc_depth_seed(lc, h.pos.p, fd);
   unsigned long long ntri = 0;
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   HIP_TRY(c, hipMemcpy(&ntri, h.mc_total.p, sizeof(ntri), hipMemcpyDeviceToHost));
   if (ntri > 5ull * kMcRes * kMcRes * kMcRes) return fail(c, UH_ERR_HIP, "uh_render_hybrid: marching-cubes triangle count out of range");
   for (int st : {grow(c, h.mc_verts, std::max<size_t>(3, 3 * (size_t)ntri), who), grow(c, b.rec_count, std::max<size_t>(1, (size_t)ntri), who),
                  grow(c, b.chunks, scan_chunk_count(std::max<uint32_t>((uint32_t)ntri, tiles)), who)})
      if (st) return st;
   if (ntri && !uhi_mc_extract_emit(c->stream, view.time, h.mc_block_counts.p, h.mc_verts.p)) return fail(c, UH_ERR_HIP, "uh_render_hybrid: marching-cubes tables");
   fd.vertices = h.mc_verts.p;
   fd.num_tris = (uint32_t)ntri;
   fd.rec_count = b.rec_count.p;
   unsigned long long totals[2];
   const BinPass pass{(size_t)ntri, tiles, 6, (1ull << 32) - 1, who, kForwardTooMany};
   const int st = bin_and_resolve(
      c, b, pass, totals, [&] { launch_forward_count(lc, fd, true); }, [] { return (int)UH_OK; },
      [&] {
         fd.records = b.records.p;
         fd.entries = b.entries.p;
         launch_forward_emit(lc, fd, true);
         launch_forward_resolve(lc, fd, true);
      });
   if (st) return st;
   light_and_shade(c, lc, view, fd, h.mc_lights.p, true);
   h.mc_tris = (uint32_t)ntri;
   h.mc_pieces = (uint32_t)totals[0];
   h.mc_lights_used = view.num_lights + 1;
   h.mc_time = view.time;
   h.mc_renders++;
   return UH_OK;
}

// ---- the rasterised G-buffer (utopian_hip.h "UH_HYBRID_GBUFFER_RASTER"; forward.hip) ----
static int raster_scene(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, RasterBins& b, const RasterTarget& t, ForwardDev& fd, const char* who, uint32_t* pieces);

// ---- motion vectors (utopian_hip.h "motion vectors"; motion.hip) ----
// before a motion pass: the pass's buffers (first call with the bit) and the per-mesh table - every mesh's state against the snapshot the
// previous motion pass left, with that snapshot's transform and rows
static int motion_prepare(uh_ctx* c, MotionDev& md) {
   uh_ctx::Hybrid& h = c->hy;
   const char* const who = "uh_render_hybrid: motion vectors";
   if (!h.mv_counters.p) {
      if (int st = stage_create(c, h.mv_stage, 2)) return st;
      if (int st = alloc_group(c, [&](auto f) { h.motion_images((size_t)c->W * c->H, f); })) return st;
   }
   const size_t nm = c->meshes.size();
   if (int st = grow(c, h.mv_table, std::max<size_t>(1, nm), who)) return st;
   h.mv_rows.assign(nm, MotionMesh{});
   uint32_t states[4] = {0, 0, 0, 0};
   for (size_t i = 0; i < nm; i++) {
      const HostMesh& m = c->meshes[i];
      MotionMesh& row = h.mv_rows[i];
      std::memcpy(row.prev_o2w, m.o2w, sizeof(row.prev_o2w));
      if (h.mv_renders == 0) {
         row.state = kMotionStatic;  // the first pass ever: what uh_denoise assumes without the flag
      } else if (i >= h.mv_snap.size()) {
         row.state = kMotionNone;    // added since
      } else {
         const uh_ctx::Hybrid::MotionSnap& s = h.mv_snap[i];
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
   if (nm) HIP_TRY(c, hipMemcpyAsync(h.mv_table.p, h.mv_rows.data(), nm * sizeof(MotionMesh), hipMemcpyHostToDevice, c->stream));
   std::memcpy(h.mv_states, states, sizeof(states));
   h.mv_blocks = motion_blocks(c->W * c->H, c->num_cus);
   if (h.mv_blocks > uh_ctx::Hybrid::kMotionMaxBlocks) return fail(c, UH_ERR_CAPACITY, std::string(who) + ": a device of more than 1024 compute units");
   md = MotionDev{h.mv_image.p, h.mv_table.p, h.mv_prev.p, h.mv_counters.p};
   return UH_OK;
}

// behind a motion pass, on its stream: the positions of the meshes whose vertices changed since the last snapshot (all of them the
// first time and when a mesh was added: the rows are laid out again), and every mesh's transform and serial
static int motion_snapshot(uh_ctx* c, const LaunchCfg& lc) {
   uh_ctx::Hybrid& h = c->hy;
   const size_t nm = c->meshes.size();
   std::vector<uh_ctx::Hybrid::MotionSnap> snap(nm);
   size_t rows = 0;
   for (size_t i = 0; i < nm; i++) {
      const HostMesh& m = c->meshes[i];
      std::memcpy(snap[i].o2w, m.o2w, sizeof(snap[i].o2w));
      snap[i].serial = m.serial;
      snap[i].base = (uint32_t)rows;
      snap[i].count = m.iso ? 0u : (uint32_t)m.num_vertices();  // an isosurface mesh is never `deformed`: no rows
      rows += snap[i].count;
   }
   const bool relayout = h.mv_snap.size() != nm || !h.mv_prev.p;
   if (relayout && h.mv_prev.n < std::max<size_t>(1, rows)) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // the pass read the old rows
      if (int st = grow(c, h.mv_prev, std::max<size_t>(1, rows), "uh_render_hybrid: motion vectors")) return st;
   }
   // one launch per run of meshes to copy whose vertices and rows both follow one another (a whole-scene update: one launch)
   size_t from = 0, to = 0, count = 0;
   const auto flush = [&] {
      if (count) launch_motion_snapshot(lc, h.vertices.p + from, h.mv_prev.p + to, (uint32_t)count);
      count = 0;
   };
   for (size_t i = 0; i < nm; i++) {
      if (!snap[i].count || (!relayout && h.mv_snap[i].serial == snap[i].serial)) continue;
      if (count && (h.layout[i].vb != from + count || snap[i].base != to + count)) flush();
      if (!count) from = h.layout[i].vb, to = snap[i].base;
      count += snap[i].count;
   }
   flush();
   HIP_TRY(c, hipGetLastError());
   h.mv_snap = std::move(snap);
   return UH_OK;
}

// raster_scene into the pass's own depth, visibility and records, then gbuffer.frag into the four targets; with `motion` the motion
// pass on the same records behind it
static int render_gbuffer_raster(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, const HybridDev& hd, const MotionDev* motion) {
   uh_ctx::Hybrid& h = c->hy;
   ForwardDev fd{};
   uint32_t pieces = 0;
   if (int st = raster_scene(c, lc, view, h.gr_bins, h.gr, fd, "uh_render_hybrid: rasterised G-buffer", &pieces)) return st;
   launch_gbuffer_raster_shade(lc, c->scene, fd, hd);
   if (motion) {
      HIP_TRY(c, stage_begin(h.mv_stage[0], c->stream));
      launch_gbuffer_raster_motion(lc, c->scene, fd, hd, *motion);
      HIP_TRY(c, stage_end(h.mv_stage[0], c->stream));
   }
   h.gr_pieces = pieces;
   h.gr_renders++;
   return UH_OK;
}

int uh_render_hybrid(uh_ctx* c, const UhViewUniformData* view, uint32_t mask) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: null view");
   const bool raster = (mask & UH_HYBRID_GBUFFER_RASTER) != 0;
   if (raster && !(mask & UH_HYBRID_GBUFFER))
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: UH_HYBRID_GBUFFER_RASTER without UH_HYBRID_GBUFFER (the bit chooses how the G-buffer pass runs); set both, "
                  "or neither");
   // the IBL maps exist for this call's consumers when an earlier call built them or this one does, before rt_reflections
   const bool maps = c->hy.env_builds > 0 || (mask & UH_HYBRID_ENVIRONMENT);
   if ((mask & UH_HYBRID_RT_REFLECTIONS) && view->ibl_enabled == 1 && !maps)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: rt_reflections with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), "
                  "which are not part of this library until a call with UH_HYBRID_ENVIRONMENT builds them; set that bit, or ibl_enabled = 0 "
                  "for the reflection pass's non-IBL branch");
   const bool render_maps = (mask & UH_HYBRID_SHADOW_MAPS) && view->shadows_enabled == 1;
   if (render_maps && !c->hy.params_set)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: UH_HYBRID_SHADOW_MAPS before uh_set_shadowmap_params (the cascades of uh_shadow_cascades or the caller's own)");
   if (mask & UH_HYBRID_DEFERRED) {
      if (view->shadows_enabled == 1 && !c->hy.smap_size && !render_maps)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the deferred pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call "
                     "with UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0 for the rt_shadows branch");
      if (view->ibl_enabled == 1 && !maps)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the deferred pass with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), "
                     "which a call with UH_HYBRID_ENVIRONMENT builds; set that bit, or ibl_enabled = 0 for the ambient term 0.03 * diffuse * occlusion");
      if (view->num_lights > c->lights.size())
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: view.num_lights exceeds the lights added with uh_add_light");
   }
   if ((mask & UH_HYBRID_SKY) && view->cubemap_enabled == 1 && !maps)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_render_hybrid: the sky pass with view.cubemap_enabled = 1 needs the environment cube (ibl.rs), which a call with "
                  "UH_HYBRID_ENVIRONMENT builds; set that bit, or cubemap_enabled = 0 for the IntegrateScattering branch");
   // the reservoir lights: one shadow ray per pixel toward the light of its spatial reservoir, which the deferred pass then adds
   const bool restir = (mask & UH_HYBRID_RESTIR_LIGHTS) != 0;
   if (restir) {
      if (view->raytracing_supported != 1)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts shadow rays and view.raytracing_supported is not 1; set it, or clear the bit");
      if (!(mask & UH_HYBRID_GBUFFER) && !c->hy.gbuffer_done)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts its rays from the G-buffer, and no G-buffer has been rendered; set "
                     "UH_HYBRID_GBUFFER");
      if (!c->restir_recorded)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS reads the spatial reservoirs, and no reservoir pass has run on this context; "
                     "render a frame with UH_PASS_RESTIR (same camera) first");
      if (c->rp_world > 1)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS needs the whole frame's reservoirs, and a row partition with world > 1 is set "
                     "(uh_set_restir_partition)");
   }
   // ray-traced ambient occlusion takes the SSAO slot: short hemisphere rays from the G-buffer instead of ssao.frag
   const bool rtao = (mask & UH_HYBRID_RTAO) && view->ssao_enabled == 1;
   if (rtao) {
      if (view->raytracing_supported != 1)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTAO casts occlusion rays and view.raytracing_supported is not 1; set it, or clear the bit");
      if (!(mask & UH_HYBRID_GBUFFER) && !c->hy.gbuffer_done)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: UH_HYBRID_RTAO casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER");
      if ((uint64_t)c->W * c->H * 64u >= (1ull << 32))
         return fail(c, UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_RTAO: a frame of 2^26 pixels or more (its rays are numbered in 32 bits)");
   }
   // setup_marching_cubes_pass (mod.rs:164): only with the checkbox on
   const bool mc = (mask & UH_HYBRID_MARCHING_CUBES) && view->marching_cubes_enabled == 1;
   if (mc) {
      if (!(mask & UH_HYBRID_GBUFFER) && !c->hy.gbuffer_done)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the marching-cubes pass depth-tests against the G-buffer's depth, and no G-buffer has been rendered; "
                     "set UH_HYBRID_GBUFFER, or marching_cubes_enabled = 0");
      if (c->meshes.empty())
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: the marching-cubes pass shades with the first mesh's material (mesh_index 0), and the scene has no mesh");
      if (view->shadows_enabled == 1 && !c->hy.smap_size && !render_maps)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_hybrid: the marching-cubes pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a "
                     "call with UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0");
      if (view->num_lights > c->lights.size())
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: the marching-cubes pass: view.num_lights exceeds the lights added with uh_add_light");
   }
   if (!c->built && c->topology_valid && view->rebuild_tlas == 1)
      if (int st = uh_refit_acceleration(c)) return st;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_render_hybrid before uh_build_acceleration");
   if (raster && (c->W > 65535 || c->H > 65535))
      return fail(c, UH_ERR_CAPACITY, "uh_render_hybrid: rasterised G-buffer: a frame wider or taller than 65535 pixels");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Hybrid& h = c->hy;
   const bool first = !h.counter.p;
   if (int st = hybrid_alloc(c)) return st;
   if (int st = hybrid_tables(c)) return st;
   if (raster && !h.gr.covered.p)
      if (int st = alloc_group(c, [&](auto f) { h.gr.each((size_t)c->W * c->H, f); })) return st;
   const uint32_t frame_bits = UH_HYBRID_SSAO | UH_HYBRID_DEFERRED | UH_HYBRID_SKY | UH_HYBRID_PRESENT;
   const bool frame_first = ((mask & frame_bits) || mc || rtao) && !h.sky_counter.p;
   if ((mask & frame_bits) || mc || rtao) {
      if (int st = hybrid_frame_alloc(c)) return st;
      if ((mask & UH_HYBRID_DEFERRED) || mc)
         if (int st = hybrid_light_table(c)) return st;
   }
   if (mc && !h.mc.covered.p)
      if (int st = alloc_group(c, [&](auto f) { h.mc_images((size_t)c->W * c->H, f); })) return st;
   if (restir) {
      if (int st = hybrid_light_table(c)) return st;
      if (!h.rl_read) HIP_TRY(c, hipEventCreateWithFlags(&h.rl_read, hipEventDisableTiming));
      if (!h.rl_counters.p) {
         if (int st = alloc_group(c, [&](auto f) { h.restir_images((size_t)c->W * c->H, f); })) return st;
         HIP_TRY(c, hipMemsetAsync(h.rl_vis.p, 0, (size_t)c->W * c->H, c->stream));
         HIP_TRY(c, hipMemsetAsync(h.rl_counters.p, 0, 2 * sizeof(uint32_t), c->stream));
      }
   }
   if (rtao && !h.ao_counters.p) {
      if (int st = alloc_group(c, [&](auto f) { h.rtao_images((size_t)c->W * c->H, f); })) return st;
      HIP_TRY(c, hipMemsetAsync(h.ao_counts.p, 0, h.ao_counts.n, c->stream));
   }
   if (mask & UH_HYBRID_ENVIRONMENT)
      if (int st = env_alloc(c)) return st;
   // motion vectors: a modifier of the G-buffer pass, ignored without it
   const bool motion = (mask & UH_HYBRID_MOTION) && (mask & UH_HYBRID_GBUFFER);
   const FrameParams fp = make_params(c, *view);
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
      hd.sun_dir[a] = fp.sun_dir[a];
      hd.eye[a] = view->eye_pos[a];
   }
   hd.W = c->W;
   hd.H = c->H;
   hd.furnace = c->furnace ? 1u : 0u;
   if (int st = wait_frames_in_flight(c)) return st;
   LaunchCfg lc = cfg(c);
   lc.count_visits = false;  // nothing of this call goes to UhStats
   if (first) launch_hybrid_clear(lc, hd);
   HybridFrameDev fd{};
   fd.ssao = h.ssao.p;
   fd.deferred = h.deferred.p;
   fd.present = h.present.p;
   fd.sky_counter = h.sky_counter.p;
   fd.lights = h.lights.p;
   fd.raw_lights = h.raw_lights.p;
   std::memcpy(fd.view, view->view, sizeof(fd.view));
   std::memcpy(fd.proj, view->projection, sizeof(fd.proj));
   std::memcpy(fd.inv_view, view->inverse_view, sizeof(fd.inv_view));
   fd.num_lights = view->num_lights;
   fd.ssao_on = view->ssao_enabled == 1;
   fd.rt_on = view->raytracing_supported == 1;
   fd.fxaa_on = view->fxaa_enabled == 1;
   for (int a = 0; a < 3; a++) fd.sun_raw[a] = view->sun_dir[a];
   if (frame_first) launch_hybrid_frame_clear(lc, hd, fd);
   // the camera grid when the path tracer's is built for this camera and geometry (read only: the grid's state is the path tracer's)
   float mats[32];
   std::memcpy(mats, fp.inv_view, sizeof(float) * 16);
   std::memcpy(mats + 16, fp.inv_proj, sizeof(float) * 16);
   const bool grid = c->cam_grid_enabled && c->cam_valid && c->cam_geom == c->geom_version && std::memcmp(mats, c->cam_mats, sizeof(mats)) == 0;
   const bool rt = view->raytracing_supported != 0;
   // every stage this call runs between its two events; the passes that do not run report 0, the environment's last build stays
   // (a call that only renders shadow maps leaves the passes' records as they are)
   if ((mask & (UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT | UH_HYBRID_SHADOW_MAPS)) != UH_HYBRID_SHADOW_MAPS)
      for (int k = 0; k < kHybridPasses; k++) h.stage[k].ran = false;
   if (mask & UH_HYBRID_SHADOW_MAPS) h.stage[kStShadowMaps].ran = false;
   if (mask & UH_HYBRID_MARCHING_CUBES) h.stage[kStMarchingCubes].ran = false;
   if (restir) h.stage[kStRestirLights].ran = false;
   if (rtao) h.stage[kStRtaoTrace].ran = h.stage[kStRtaoFilter].ran = false;
   // setup_shadow_pass's four passes are added first (mod.rs:91-98)
   if (render_maps) {
      HIP_TRY(c, stage_begin(h.stage[kStShadowMaps], c->stream));
      int st = render_shadow_maps(c, lc, "uh_render_hybrid");
      const hipError_t e = st ? hipSuccess : stage_end(h.stage[kStShadowMaps], c->stream);
      if (st || e != hipSuccess) h.stage[kStShadowMaps].ran = false;  // no time for a render that did not complete
      if (st) return st;
      HIP_TRY(c, e);
   }
   // pass order of build_render_graph (mod.rs:100-134, graph.rs:743): rt_shadows, gbuffer, rt_reflections
   if (rt && (mask & UH_HYBRID_RT_SHADOWS)) {
      HIP_TRY(c, stage_begin(h.stage[kStShadows], c->stream));
      launch_hybrid_shadows(lc, c->scene, hd);
      HIP_TRY(c, stage_end(h.stage[kStShadows], c->stream));
   }
   if (mask & UH_HYBRID_GBUFFER) {
      MotionDev md{};
      if (motion) {
         h.mv_last = false;  // until this pass and its snapshot are enqueued
         h.mv_stage[0].ran = h.mv_stage[1].ran = false;
         if (int st = motion_prepare(c, md)) return st;
      }
      HIP_TRY(c, stage_begin(h.stage[kStGbuffer], c->stream));
      if (raster) {
         if (int st = render_gbuffer_raster(c, lc, *view, hd, motion ? &md : nullptr)) {
            h.stage[kStGbuffer].ran = false;  // no time for a pass that did not complete
            return st;
         }
      } else if (motion) {
         // k_hybrid_motion between the cast and the resolve: it reads the hit records the cast left in the targets
         launch_hybrid_gbuffer_cast(lc, fp, c->scene, hd, grid ? &c->cam_dev : nullptr);
         HIP_TRY(c, stage_begin(h.mv_stage[0], c->stream));
         launch_hybrid_motion(lc, c->scene, hd, md);
         HIP_TRY(c, stage_end(h.mv_stage[0], c->stream));
         launch_hybrid_gbuffer_resolve(lc, c->scene, hd);
      } else {
         launch_hybrid_gbuffer(lc, fp, c->scene, hd, grid ? &c->cam_dev : nullptr);
      }
      HIP_TRY(c, stage_end(h.stage[kStGbuffer], c->stream));
      h.gbuffer_done = true;
      h.gbuffer_rasterised = raster;
      h.mv_last = false;
      if (motion) {
         HIP_TRY(c, stage_begin(h.mv_stage[1], c->stream));
         const int st = motion_snapshot(c, lc);
         if (st) {
            h.mv_stage[1].ran = false;
            return st;
         }
         HIP_TRY(c, stage_end(h.mv_stage[1], c->stream));
         h.mv_renders++;
         h.mv_last = true;
      }
   }
   // setup_cubemap_pass (mod.rs:121): after the G-buffer, before rt_reflections; the maps persist until the next build
   const IblMaps ibl{h.env.p, h.irr.p, h.spec.p, h.lut.p};
   if (mask & UH_HYBRID_ENVIRONMENT) {
      EnvDev e{h.env.p, h.irr.p, h.spec.p, h.lut.p, h.taps.p, {}, {}};
      for (int a = 0; a < 3; a++) {
         e.eye[a] = view->inverse_view[12 + a];  // extract_camera_position(view.view): inverse(view)[3]
         e.sun[a] = view->sun_dir[a];
         h.env_eye[a] = e.eye[a];
         h.env_sun[a] = e.sun[a];
      }
      void (*const build[4])(const LaunchCfg&, const EnvDev&) = {launch_env_cube, launch_env_irradiance, launch_env_specular, launch_env_brdf_lut};
      for (int k = 0; k < 4; k++) {
         HIP_TRY(c, stage_begin(h.stage[kStEnvCube + k], c->stream));
         build[k](lc, e);
         HIP_TRY(c, stage_end(h.stage[kStEnvCube + k], c->stream));
      }
      h.env_builds++;
   }
   if (rt && (mask & UH_HYBRID_RT_REFLECTIONS)) {
      HIP_TRY(c, stage_begin(h.stage[kStReflections], c->stream));
      HIP_TRY(c, hipMemsetAsync(h.counter.p, 0, sizeof(uint32_t), c->stream));
      launch_hybrid_reflections(lc, c->scene, hd, view->ibl_enabled == 1 ? &ibl : nullptr);
      HIP_TRY(c, stage_end(h.stage[kStReflections], c->stream));
   }
   // restir_lights: the pixels' reservoirs (whatever the last reservoir pass left: read only) and this call's light count
   const HybridRestirDev rl{h.rl_vis.p, h.rl_queue.p, h.rl_counters.p, c->im.reservoirs[2], h.raw_lights.p,
                            (uint32_t)std::min<size_t>(view->num_lights, c->lights.size())};
   if (restir) {
      HIP_TRY(c, stage_begin(h.stage[kStRestirLights], c->stream));
      HIP_TRY(c, hipMemsetAsync(h.rl_counters.p, 0, 2 * sizeof(uint32_t), c->stream));
      launch_hybrid_restir_lights(lc, fp, c->scene, hd, rl);
      HIP_TRY(c, stage_end(h.stage[kStRestirLights], c->stream));
      h.rl_renders++;
   }
   // the final frame (mod.rs:136-186): ssao_pass (not with ssao_enabled != 1, ssao.rs:27), deferred_pass, atmosphere_pass, present_pass
   if (rtao) {
      // the rtao pass in ssao_pass's place: classify + trace into the counts, then the resolve / filter into ssao_output
      const UhRtaoParams& p = h.ao_params;
      const RtaoDev ao{h.ao_counts.p, h.ao_queue.p, h.ao_counters.p, p.samples, fp.frame_number * 64u, p.blur_radius, p.radius, p.strength, p.blur_normal_cos, p.blur_plane};
      HIP_TRY(c, stage_begin(h.stage[kStRtaoTrace], c->stream));
      HIP_TRY(c, hipMemsetAsync(h.ao_counters.p, 0, 6 * sizeof(uint32_t), c->stream));
      LaunchCfg ac = lc;
      ac.count_visits = c->count_visits;  // into the pass's own counters (uh_get_rtao_visits), never UhStats
      launch_rtao_trace(ac, c->scene, hd, ao, h.ao_order);
      HIP_TRY(c, stage_end(h.stage[kStRtaoTrace], c->stream));
      HIP_TRY(c, stage_begin(h.stage[kStRtaoFilter], c->stream));
      launch_rtao_resolve(lc, hd, ao, h.ssao.p);
      HIP_TRY(c, stage_end(h.stage[kStRtaoFilter], c->stream));
      h.ao_samples = p.samples;
      h.ao_renders++;
   } else if ((mask & UH_HYBRID_SSAO) && view->ssao_enabled == 1) {
      HIP_TRY(c, stage_begin(h.stage[kStSsao], c->stream));
      launch_hybrid_ssao(lc, hd, fd);
      HIP_TRY(c, stage_end(h.stage[kStSsao], c->stream));
   }
   if (mask & UH_HYBRID_DEFERRED) {
      HIP_TRY(c, stage_begin(h.stage[kStDeferred], c->stream));
      const ShadowLookup sl{h.smaps.p, h.s_params.p, h.smap_size};
      launch_hybrid_deferred(lc, c->scene, hd, fd, view->ibl_enabled == 1 ? &ibl : nullptr, view->shadows_enabled == 1 ? &sl : nullptr, restir ? &rl : nullptr);
      HIP_TRY(c, stage_end(h.stage[kStDeferred], c->stream));
   }
   h.frame_lights = h.stage[kStDeferred].ran ? (restir ? 2 : view->num_lights + 1) : 0;  // with the reservoir lights: the sun and the reservoir's
   if (restir) {
      // a reservoir pass enqueued after this call starts behind the call's reads (the spatial ring comes round to the slot read here)
      HIP_TRY(c, hipEventRecord(h.rl_read, c->stream));
      HIP_TRY(c, hipStreamWaitEvent(c->restir_stream, h.rl_read, 0));
   }
   // setup_marching_cubes_pass (mod.rs:164-174): after the deferred pass, before the atmosphere pass
   if (mc) {
      HIP_TRY(c, stage_begin(h.stage[kStMarchingCubes], c->stream));
      if (int st = render_mc_pass(c, lc, *view)) {
         h.stage[kStMarchingCubes].ran = false;  // no time for a pass that did not complete
         return st;
      }
      HIP_TRY(c, stage_end(h.stage[kStMarchingCubes], c->stream));
   }
   if (mask & UH_HYBRID_SKY) {
      HIP_TRY(c, stage_begin(h.stage[kStSky], c->stream));
      HIP_TRY(c, hipMemsetAsync(h.sky_counter.p, 0, sizeof(uint32_t), c->stream));
      launch_hybrid_sky(lc, fp, hd, fd, view->cubemap_enabled == 1 ? &ibl : nullptr, mc ? h.mc.vis.p : nullptr);
      HIP_TRY(c, stage_end(h.stage[kStSky], c->stream));
   }
   if (mask & UH_HYBRID_PRESENT) {
      HIP_TRY(c, stage_begin(h.stage[kStPresent], c->stream));
      launch_hybrid_present(lc, hd, fd);
      HIP_TRY(c, stage_end(h.stage[kStPresent], c->stream));
   }
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

int uh_read_hybrid(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (!h.counter.p) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid before the first uh_render_hybrid");
   if (which < 0 || which > UH_HYBRID_MOTION_IMAGE) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image index must be 0..15");
   if (which >= UH_HYBRID_SSAO_IMAGE && which <= UH_HYBRID_PRESENT_OUTPUT && !h.sky_counter.p)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 6..8 before the first call with an SSAO, deferred, sky or present bit");
   if ((which == UH_HYBRID_DEPTH || which == UH_HYBRID_MARCHING_CUBES_VISIBILITY) && h.mc_renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 9..10 before the first marching-cubes pass");
   if ((which == UH_HYBRID_GBUFFER_DEPTH || which == UH_HYBRID_GBUFFER_VISIBILITY) && h.gr_renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: images 11..12 before the first rasterised G-buffer pass");
   if (which == UH_HYBRID_LIGHT_VISIBILITY && !h.rl_counters.p)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image 13 before the first call with UH_HYBRID_RESTIR_LIGHTS");
   if (which == UH_HYBRID_AO_COUNTS && h.ao_renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image 14 before the first rtao pass (UH_HYBRID_RTAO with view.ssao_enabled = 1)");
   if (which == UH_HYBRID_MOTION_IMAGE && h.mv_renders == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image 15 before the first motion pass (UH_HYBRID_GBUFFER | UH_HYBRID_MOTION)");
   // image k's pixels and its bytes per pixel, in UH_HYBRID_* image order
   const std::pair<const void*, size_t> img[] = {
      {h.pos.p, sizeof(float4)}, {h.nrm.p, sizeof(float4)}, {h.alb.p, sizeof(uchar4)}, {h.pbr.p, sizeof(float4)}, {h.shadow.p, 1},
      {h.refl.p, sizeof(uchar4)}, {h.ssao.p, sizeof(uint16_t)}, {h.deferred.p, sizeof(float4)}, {h.present.p, sizeof(uchar4)},
      {h.mc.depth.p, sizeof(float)}, {h.mc.vis.p, sizeof(uint32_t)}, {h.gr.depth.p, sizeof(float)}, {h.gr.vis.p, sizeof(uint32_t)},
      {h.rl_vis.p, 1}, {h.ao_counts.p, 1}, {h.mv_image.p, sizeof(float4)}};
   return read_back(c, out, img[which].first, (size_t)c->W * c->H * img[which].second);
}

int uh_get_hybrid_frame_stats(uh_ctx* c, UhHybridFrameStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_hybrid_frame_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (!h.counter.p) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   for (int k = 0; k < kHybridPasses; k++)
      if (int st = stage_ms(c, c->hy.stage[k], &out->pass_ms[k])) return st;
   if (h.stage[kStSky].ran) HIP_TRY(c, hipMemcpy(&out->sky_pixels, h.sky_counter.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   out->lights = h.frame_lights;
   return UH_OK;
}

int uh_get_hybrid_restir_stats(uh_ctx* c, UhHybridRestirStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_hybrid_restir_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (h.rl_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (int st = stage_ms(c, c->hy.stage[kStRestirLights], &out->pass_ms)) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, h.rl_counters.p, sizeof(counters), hipMemcpyDeviceToHost));
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
   c->hy.ao_params = *params;
   return UH_OK;
}

int uh_get_rtao_stats(uh_ctx* c, UhRtaoStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_rtao_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (h.ao_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (int st = stage_ms(c, c->hy.stage[kStRtaoTrace], &out->trace_ms)) return st;
   if (int st = stage_ms(c, c->hy.stage[kStRtaoFilter], &out->filter_ms)) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, h.ao_counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->rays = (uint64_t)counters[0] * h.ao_samples;
   out->occluded = counters[1];
   return UH_OK;
}

int uh_get_rtao_visits(uh_ctx* c, uint64_t* nodes, uint64_t* triangles) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!nodes || !triangles) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_rtao_visits: null destination");
   *nodes = *triangles = 0;
   const uh_ctx::Hybrid& h = c->hy;
   if (h.ao_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   uint64_t visits[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(visits, h.ao_counters.p + 2, sizeof(visits), hipMemcpyDeviceToHost));
   *nodes = visits[0];
   *triangles = visits[1];
   return UH_OK;
}

int uh_get_motion_stats(uh_ctx* c, UhMotionStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_motion_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   uh_ctx::Hybrid& h = c->hy;
   if (h.mv_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (int st = stage_ms(c, h.mv_stage[0], &out->motion_ms)) return st;
   if (int st = stage_ms(c, h.mv_stage[1], &out->snapshot_ms)) return st;
   std::vector<uint32_t> counts(2 * (size_t)h.mv_blocks);  // a pair per block of the kernel's grid
   HIP_TRY(c, hipMemcpy(counts.data(), h.mv_counters.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   for (uint32_t b = 0; b < h.mv_blocks; b++) out->pixels_with += counts[2 * b], out->pixels_without += counts[2 * b + 1];
   out->meshes_static = h.mv_states[kMotionStatic];
   out->meshes_rigid = h.mv_states[kMotionRigid];
   out->meshes_deformed = h.mv_states[kMotionDeformed];
   out->meshes_none = h.mv_states[kMotionNone];
   return UH_OK;
}

int uh_get_marching_cubes_stats(uh_ctx* c, UhMarchingCubesStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_marching_cubes_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (h.mc_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (int st = stage_ms(c, c->hy.stage[kStMarchingCubes], &out->pass_ms)) return st;
   out->renders = h.mc_renders;
   out->triangles = h.mc_tris;
   out->pieces = h.mc_pieces;
   HIP_TRY(c, hipMemcpy(&out->covered_pixels, h.mc.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   out->lights = h.mc_lights_used;
   out->time = h.mc_time;
   return UH_OK;
}

int uh_get_gbuffer_raster_stats(uh_ctx* c, UhGbufferRasterStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_gbuffer_raster_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (h.gr_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (h.gbuffer_rasterised)  // the G-buffer stage's record is the last rasterised pass's
      if (int st = stage_ms(c, c->hy.stage[kStGbuffer], &out->pass_ms)) return st;
   out->renders = h.gr_renders;
   out->pieces = h.gr_pieces;
   HIP_TRY(c, hipMemcpy(&out->covered_pixels, h.gr.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   return UH_OK;
}

int uh_read_environment(uh_ctx* c, int which, int face, int mip, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (h.env_builds == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment before the first call with UH_HYBRID_ENVIRONMENT");
   if (which == UH_ENV_BRDF_LUT) {
      if (face != 0 || mip != 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: the BRDF LUT has face 0 and mip 0 only");
      return read_back(c, out, h.lut.p, (size_t)kLutSize * kLutSize * sizeof(uint32_t));
   }
   if (which < UH_ENV_ENVIRONMENT || which > UH_ENV_SPECULAR) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: map must be 0..3");
   const int mips = which == UH_ENV_IRRADIANCE ? 1 : (int)kEnvMips;
   if (face < 0 || face > 5 || mip < 0 || mip >= mips) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: face 0..5, mip 0..7 (irradiance: 0)");
   const size_t S = kEnvSize >> mip;
   const float4* base = which == UH_ENV_ENVIRONMENT ? h.env.p : which == UH_ENV_IRRADIANCE ? h.irr.p : h.spec.p;
   return read_back(c, out, base + env_mip_offset((uint32_t)mip) + (size_t)face * S * S, S * S * sizeof(float4));
}

int uh_get_environment_stats(uh_ctx* c, UhEnvironmentStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_environment_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (h.env_builds == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   for (int k = 0; k < 4; k++)
      if (int st = stage_ms(c, c->hy.stage[kStEnvCube + k], &out->pass_ms[k])) return st;
   out->builds = h.env_builds;
   std::memcpy(out->sun_dir, h.env_sun, sizeof(out->sun_dir));
   std::memcpy(out->eye, h.env_eye, sizeof(out->eye));
   return UH_OK;
}

int uh_get_hybrid_stats(uh_ctx* c, UhHybridStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_hybrid_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (!h.counter.p) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   uint32_t metal = 0;
   if (h.stage[kStReflections].ran) HIP_TRY(c, hipMemcpy(&metal, h.counter.p, sizeof(metal), hipMemcpyDeviceToHost));
   const uint64_t n = (uint64_t)c->W * c->H;
   out->rays[0] = h.stage[kStGbuffer].ran && !h.gbuffer_rasterised ? n : 0;  // a rasterised pass casts no ray
   out->rays[1] = h.stage[kStShadows].ran ? n : 0;
   out->rays[2] = metal;
   out->reflection_pixels = metal;
   const int stages[3] = {kStGbuffer, kStShadows, kStReflections};  // the header's order
   for (int k = 0; k < 3; k++)
      if (int st = stage_ms(c, c->hy.stage[stages[k]], &out->pass_ms[k])) return st;
   return UH_OK;
}

int uh_set_shadowmap_params(uh_ctx* c, const UhShadowmapParams* p) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!p) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_shadowmap_params: null params");
   for (int k = 0; k < 4; k++) {
      const float* m = p->view_projection_matrices[k];
      for (int i = 0; i < 16; i++)
         if (!std::isfinite(m[i])) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_shadowmap_params: a non-finite matrix element");
      if (!std::isfinite(p->cascade_splits[k])) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_shadowmap_params: a non-finite split");
      if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f)
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_shadowmap_params: a matrix whose last row is not (0, 0, 0, 1) (not orthographic)");
   }
   c->hy.params = *p;
   c->hy.params_set = true;
   return UH_OK;
}

int uh_read_shadow_map(uh_ctx* c, int cascade, float* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (!h.smaps.p || !h.smap_size) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_shadow_map before the maps were rendered (UH_HYBRID_SHADOW_MAPS)");
   if (cascade < 0 || cascade > 3) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_shadow_map: cascade must be 0..3");
   const size_t n = (size_t)h.smap_size * h.smap_size;
   return read_back(c, out, h.smaps.p + (size_t)cascade * n, n * sizeof(float));
}

int uh_get_shadow_map_stats(uh_ctx* c, UhShadowMapStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_shadow_map_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   const uh_ctx::Hybrid& h = c->hy;
   if (h.s_renders == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   if (int st = stage_ms(c, c->hy.stage[kStShadowMaps], &out->pass_ms)) return st;
   out->renders = h.s_renders;
   out->size = h.smap_size;
   std::memcpy(out->triangles, h.s_tris, sizeof(out->triangles));
   out->params = h.snapshot;
   return UH_OK;
}

// ---- the forward graph (utopian_hip.h "uh_render_forward"; forward.hip) ----
// per mesh: (P V) W column-major - P V first, then times the instance's 3x4 with row (0, 0, 0, 1) - followed by the instance's 3x4
// row-major
static void forward_mesh_matrices(const uh_ctx* c, const UhViewUniformData& v, std::vector<float>& out) {
   float pv[16];
   mat4_mul(v.projection, v.view, pv);
   const size_t nm = c->meshes.size();
   out.assign(nm * 28, 0.0f);
   for (size_t m = 0; m < nm; m++) {
      const float* o = c->meshes[m].o2w;
      float w[16];
      mat4_from_3x4(o, w);
      mat4_mul(pv, w, &out[m * 28]);
      std::memcpy(&out[m * 28 + 16], o, 12 * sizeof(float));
   }
}

// the scene's meshes through the forward rasteriser (bin_and_resolve) into the target t: depth (cleared to 1.0), vis and rec_of; fd
// receives everything but its colour target. *pieces receives the records. `who` names the entry point in messages.
static int raster_scene(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, RasterBins& b, const RasterTarget& t, ForwardDev& fd, const char* who, uint32_t* pieces) {
   uh_ctx::Hybrid& h = c->hy;
   const uint32_t tiles = forward_frame(c, t, fd);
   size_t ntri = 0;
   for (const HostMesh& m : c->meshes) ntri += m.tris();
   if (ntri >= (1ull << 32) - 1) return fail(c, UH_ERR_CAPACITY, std::string(who) + ": 2^32 - 1 or more triangles");
   for (int st : {grow(c, b.tile_count, tiles, who), grow(c, b.tile_cursor, tiles, who), grow(c, b.totals, 2, who),
                  grow(c, b.mats, std::max<size_t>(1, 28 * c->meshes.size()), who),
                  grow(c, b.chunks, std::max<size_t>(1, scan_chunk_count((uint32_t)std::max<size_t>(ntri, tiles))), who)})
      if (st) return st;
   if (b.geom != c->geom_version || !b.rec_count.p) {
      for (int st : {grow(c, b.tri_mesh, std::max<size_t>(1, ntri), who), grow(c, b.rec_count, std::max<size_t>(1, ntri), who)})
         if (st) return st;
      if (int st = fill_tri_mesh(c, b.tri_mesh.p)) return st;
      b.geom = c->geom_version;
   }
   forward_mesh_matrices(c, view, b.mats_host);
   if (!b.mats_host.empty())
      HIP_TRY(c, hipMemcpyAsync(b.mats.p, b.mats_host.data(), b.mats_host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemsetAsync(b.tile_count.p, 0, tiles * sizeof(uint32_t), c->stream));
   HIP_TRY(c, hipMemsetAsync(t.covered.p, 0, sizeof(uint32_t), c->stream));
   fd.vertices = h.vertices.p;
   fd.indices = h.indices.p;
   fd.meshes = h.meshes.p;
   fd.tri_mesh = b.tri_mesh.p;
   fd.mats = b.mats.p;
   fd.num_tris = (uint32_t)ntri;
   fd.rec_count = b.rec_count.p;
   fd.tile_count = b.tile_count.p;
   fd.tile_cursor = b.tile_cursor.p;
   unsigned long long totals[2];
   // record ids below 2^32 - 1: the resolve's key holds 0xFFFFFFFE - record, and 0xFFFFFFFF stands for none
   const BinPass pass{ntri, tiles, 6, (1ull << 32) - 1, who, kForwardTooMany};
   const int st = bin_and_resolve(
      c, b, pass, totals, [&] { launch_forward_count(lc, fd); }, [] { return (int)UH_OK; },
      [&] {
         fd.records = b.records.p;
         fd.entries = b.entries.p;
         launch_forward_emit(lc, fd);
         launch_forward_resolve(lc, fd);
      });
   if (st) return st;
   *pieces = (uint32_t)totals[0];
   return UH_OK;
}

// raster_scene, then forward.frag into forward_output
static int render_forward_pass(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view) {
   uh_ctx::Forward& f = c->fw;
   ForwardDev fd{};
   fd.color = f.color.p;
   uint32_t pieces = 0;
   if (int st = raster_scene(c, lc, view, f.bins, f.target, fd, "uh_render_forward", &pieces)) return st;
   light_and_shade(c, lc, view, fd, f.lights.p, false);
   f.pieces = pieces;
   f.lights_used = view.num_lights + 1;
   f.renders++;
   return UH_OK;
}

int uh_render_forward(uh_ctx* c, const UhViewUniformData* view, uint32_t mask) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_forward: null view");
   const bool render_maps = (mask & UH_FORWARD_SHADOW_MAPS) && view->shadows_enabled == 1;
   if (render_maps && !c->hy.params_set)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_render_forward: UH_FORWARD_SHADOW_MAPS before uh_set_shadowmap_params (the cascades of uh_shadow_cascades or the caller's own)");
   if (mask & UH_FORWARD_PASS) {
      if (view->shadows_enabled == 1 && !c->hy.smap_size && !render_maps)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_forward: the forward pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call "
                     "with UH_FORWARD_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0");
      if (view->num_lights > c->lights.size())
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_forward: view.num_lights exceeds the lights added with uh_add_light");
   }
   if (!c->built && c->topology_valid && view->rebuild_tlas == 1)
      if (int st = uh_refit_acceleration(c)) return st;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_render_forward before uh_build_acceleration");
   if (c->W > 65535 || c->H > 65535) return fail(c, UH_ERR_CAPACITY, "uh_render_forward: a frame wider or taller than 65535 pixels");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Hybrid& h = c->hy;
   uh_ctx::Forward& f = c->fw;
   if (int st = hybrid_events(c)) return st;
   if (int st = hybrid_tables(c)) return st;
   const bool first = !f.color.p;
   if (first) {
      if (int st = stage_create(c, f.stage, 3)) return st;
      if (int st = alloc_group(c, [&](auto fn) { f.images((size_t)c->W * c->H, fn); })) return st;
   }
   if (mask & UH_FORWARD_PASS)
      if (int st = hybrid_light_table(c)) return st;
   if (int st = wait_frames_in_flight(c)) return st;
   LaunchCfg lc = cfg(c);
   lc.count_visits = false;  // nothing of this call goes to UhStats
   ForwardDev cd{};
   cd.W = c->W;
   cd.H = c->H;
   cd.depth = f.target.depth.p;
   cd.vis = f.target.vis.p;
   cd.rec_of = f.target.rec_of.p;
   cd.color = f.color.p;
   if (first) launch_forward_clear(lc, cd, f.present.p);
   for (auto& st : f.stage) st.ran = false;
   // setup_shadow_pass, setup_forward_pass, setup_present_pass (build_minimal_forward_render_graph): the maps are the hybrid graph's,
   // and their own record (uh_get_shadow_map_stats) is kept as a hybrid call with UH_HYBRID_SHADOW_MAPS keeps it
   if (render_maps) {
      Stage& hs = h.stage[kStShadowMaps];
      hs.ran = false;
      HIP_TRY(c, stage_begin(f.stage[0], c->stream));
      HIP_TRY(c, stage_begin(hs, c->stream));
      int st = render_shadow_maps(c, lc, "uh_render_forward");
      hipError_t e = st ? hipSuccess : stage_end(f.stage[0], c->stream);
      if (e == hipSuccess && !st) e = stage_end(hs, c->stream);
      if (st || e != hipSuccess) f.stage[0].ran = hs.ran = false;  // no time for a render that did not complete
      if (st) return st;
      HIP_TRY(c, e);
   }
   if (mask & UH_FORWARD_PASS) {
      HIP_TRY(c, stage_begin(f.stage[1], c->stream));
      int st = render_forward_pass(c, lc, *view);
      if (st) {
         f.stage[1].ran = false;
         return st;
      }
      HIP_TRY(c, stage_end(f.stage[1], c->stream));
   }
   if (mask & UH_FORWARD_PRESENT) {  // present.frag + FXAA on forward_output, into the forward graph's own image
      HIP_TRY(c, stage_begin(f.stage[2], c->stream));
      HybridDev hd{};
      hd.W = c->W;
      hd.H = c->H;
      HybridFrameDev pd{};
      pd.deferred = f.color.p;
      pd.present = f.present.p;
      pd.fxaa_on = view->fxaa_enabled == 1;
      launch_hybrid_present(lc, hd, pd);
      HIP_TRY(c, stage_end(f.stage[2], c->stream));
   }
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

int uh_read_forward(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Forward& f = c->fw;
   if (!f.color.p) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_forward before the first uh_render_forward");
   if (which < UH_FORWARD_OUTPUT || which > UH_FORWARD_PRESENT_OUTPUT) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_forward: image index must be 0..3");
   // image k's pixels and its bytes per pixel, in UH_FORWARD_* image order
   const std::pair<const void*, size_t> img[] = {{f.color.p, sizeof(float4)}, {f.target.depth.p, sizeof(float)}, {f.target.vis.p, sizeof(uint32_t)}, {f.present.p, sizeof(uchar4)}};
   return read_back(c, out, img[which].first, (size_t)c->W * c->H * img[which].second);
}

int uh_get_forward_stats(uh_ctx* c, UhForwardStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_forward_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   uh_ctx::Forward& f = c->fw;
   if (!f.color.p) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   for (int k = 0; k < 3; k++)
      if (int st = stage_ms(c, f.stage[k], &out->pass_ms[k])) return st;
   out->renders = f.renders;
   if (f.stage[1].ran) {
      out->pieces = f.pieces;
      out->lights = f.lights_used;
      HIP_TRY(c, hipMemcpy(&out->covered_pixels, f.target.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   }
   return UH_OK;
}

// ---- the denoiser (utopian_hip.h "the denoiser"; denoise.hip) ----
int uh_denoise_default_params(UhDenoiseParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   std::memset(out, 0, sizeof(*out));
   out->flags = UH_DENOISE_TEMPORAL | UH_DENOISE_DEMODULATE;
   out->iterations = 5;
   out->max_history = 32;
   out->alpha_min = 0.2f;
   out->sigma_luminance = 4.0f;
   out->sigma_plane = 0.005f;  // DESIGN.md section 2, "Denoiser": how the two plane fractions were chosen
   out->reproject_normal_cos = 0.9f;
   out->reproject_plane = 0.005f;
   return UH_OK;
}

// the first refusal of `p` by its own values, or nullptr
static const char* denoise_params_refusal(const UhDenoiseParams& p) {
   if (p.flags & ~(uint32_t)(UH_DENOISE_TEMPORAL | UH_DENOISE_DEMODULATE | UH_DENOISE_MOTION)) return "unknown flag bits";
   if (p.iterations > 5) return "iterations above 5";
   if (p.max_history < 1) return "max_history below 1";
   for (uint32_t r : p.reserved)
      if (r) return "a reserved word is not 0";
   if (!(p.alpha_min >= 0.0f && p.alpha_min <= 1.0f)) return "alpha_min outside [0, 1]";
   if (!(p.sigma_luminance > 0.0f) || !std::isfinite(p.sigma_luminance)) return "sigma_luminance not a finite value above 0";
   if (!(p.sigma_plane > 0.0f) || !std::isfinite(p.sigma_plane)) return "sigma_plane not a finite value above 0";
   if (!(p.reproject_normal_cos >= -1.0f && p.reproject_normal_cos <= 1.0f)) return "reproject_normal_cos outside [-1, 1]";
   if (!(p.reproject_plane > 0.0f) || !std::isfinite(p.reproject_plane)) return "reproject_plane not a finite value above 0";
   return nullptr;
}

int uh_denoise(uh_ctx* c, const UhViewUniformData* view, const UhDenoiseParams* params) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view || !params) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_denoise: null view or params");
   if (const char* why = denoise_params_refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string("uh_denoise: params: ") + why);
   const uint32_t n = std::min(view->total_samples, view->accumulation_limit);
   if (n == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_denoise: min(view.total_samples, view.accumulation_limit) is 0: the accumulation image holds no sample to divide by");
   if (c->tp_world > 1)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_denoise: a tile partition with world > 1 is set (uh_set_tile_partition): this context's accumulation image is partial");
   if (!c->hy.gbuffer_done)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_denoise reads the hybrid G-buffer (position, normal, albedo, mesh index), and none has been rendered; call "
                  "uh_render_hybrid with UH_HYBRID_GBUFFER (same camera) first");
   if ((params->flags & UH_DENOISE_MOTION) && !c->hy.mv_last)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_denoise: UH_DENOISE_MOTION reads the motion image of the last G-buffer pass, and that pass had no UH_HYBRID_MOTION; render "
                  "it with UH_HYBRID_GBUFFER | UH_HYBRID_MOTION, or clear the flag");
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_denoise before uh_build_acceleration");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Denoise& dn = c->dn;
   const uh_ctx::Hybrid& h = c->hy;
   const size_t pixels = (size_t)c->W * c->H;
   if (!dn.counters.p) {
      if (int st = stage_create(c, dn.stage, 4)) return st;
      if (!dn.acc_read) HIP_TRY(c, hipEventCreateWithFlags(&dn.acc_read, hipEventDisableTiming));
      hipError_t e = hipSuccess;
      dn.images(pixels, [&e](auto& b, size_t count) {
         if (e == hipSuccess) e = b.alloc(count);
      });
      if (e != hipSuccess) {
         dn.images(0, [](auto& b, size_t) { b.release(); });
         return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string("uh_denoise: allocation: ") + hipGetErrorString(e));
      }
      dn.have_history = false;
   }
   DenoiseDev d{};
   d.acc = c->accumulation.p;
   d.g_pos = h.pos.p, d.g_nrm = h.nrm.p, d.g_pbr = h.pbr.p, d.g_alb = h.alb.p;
   d.unorm_lut = c->d_lut.p;
   const int cur = dn.cur, prev = cur ^ 1;
   d.prev = DenoiseHistory{dn.h_pos[prev].p, dn.h_nrm[prev].p, dn.h_col[prev].p, dn.h_mom[prev].p};
   d.cur = DenoiseHistory{dn.h_pos[cur].p, dn.h_nrm[cur].p, dn.h_col[cur].p, dn.h_mom[cur].p};
   d.input = dn.input.p, d.cv[0] = dn.cv[0].p, d.cv[1] = dn.cv[1].p, d.temporal = dn.temporal.p, d.color = dn.color.p;
   d.output = dn.output.p, d.history = dn.history.p, d.variance = dn.variance.p, d.counters = dn.counters.p;
   d.W = c->W, d.H = c->H;
   d.n = (float)n;
   std::memcpy(d.view, view->view, sizeof(d.view));
   std::memcpy(d.prev_pv, view->prev_frame_projection_view, sizeof(d.prev_pv));
   d.temporal_on = ((params->flags & UH_DENOISE_TEMPORAL) && dn.have_history) ? 1u : 0u;
   d.demodulate = (params->flags & UH_DENOISE_DEMODULATE) ? 1u : 0u;
   d.motion = ((params->flags & UH_DENOISE_MOTION) && d.temporal_on) ? h.mv_image.p : nullptr;  // (without a temporal stage: no effect)
   d.max_history = (float)params->max_history;
   d.alpha_min = params->alpha_min, d.sigma_luminance = params->sigma_luminance, d.sigma_plane = params->sigma_plane;
   d.reproject_normal_cos = params->reproject_normal_cos, d.reproject_plane = params->reproject_plane;
   if (int st = wait_frames_in_flight(c)) return st;
   LaunchCfg lc = cfg(c);
   for (Stage& s : dn.stage) s.ran = false;
   HIP_TRY(c, stage_begin(dn.stage[0], c->stream));
   HIP_TRY(c, hipMemsetAsync(dn.counters.p, 0, 2 * sizeof(uint32_t), c->stream));
   launch_denoise_temporal(lc, d);
   HIP_TRY(c, stage_end(dn.stage[0], c->stream));
   // the accumulation image and the hybrid targets have been read (the output stage reads the albedo again: hybrid calls run on this
   // stream): a frame enqueued from here on applies its accumulate tail behind this point, like behind a frame's
   HIP_TRY(c, hipEventRecord(dn.acc_read, c->stream));
   c->last_acc = dn.acc_read;
   // from here on this call's set is the history, whatever fails below
   dn.cur = prev;
   dn.have_history = true;
   dn.calls++;
   HIP_TRY(c, stage_begin(dn.stage[1], c->stream));
   launch_denoise_variance(lc, d);
   HIP_TRY(c, stage_end(dn.stage[1], c->stream));
   HIP_TRY(c, stage_begin(dn.stage[2], c->stream));
   for (uint32_t level = 0; level < params->iterations; level++) launch_denoise_atrous(lc, d, level);
   HIP_TRY(c, stage_end(dn.stage[2], c->stream));
   HIP_TRY(c, stage_begin(dn.stage[3], c->stream));
   launch_denoise_output(lc, d, params->iterations & 1);
   HIP_TRY(c, stage_end(dn.stage[3], c->stream));
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

int uh_reset_denoise_history(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (c->dn.counters.p) {
      HIP_TRY(c, hipSetDevice(c->device));
      if (int st = sync_all(c)) return st;
   }
   c->dn.have_history = false;
   return UH_OK;
}

int uh_read_denoised(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Denoise& dn = c->dn;
   if (dn.calls == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_denoised before the first uh_denoise");
   if (which < UH_DENOISE_COLOR || which > UH_DENOISE_VARIANCE) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_denoised: image index must be 0..5");
   // image k's pixels and its bytes per pixel, in UH_DENOISE_* image order
   const std::pair<const void*, size_t> img[] = {{dn.color.p, sizeof(float4)}, {dn.output.p, sizeof(uchar4)}, {dn.input.p, sizeof(float4)},
                                                 {dn.temporal.p, sizeof(float4)}, {dn.history.p, sizeof(float)}, {dn.variance.p, sizeof(float)}};
   return read_back(c, out, img[which].first, (size_t)c->W * c->H * img[which].second);
}

int uh_get_denoise_stats(uh_ctx* c, UhDenoiseStats* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_get_denoise_stats: null destination");
   std::memset(out, 0, sizeof(*out));
   uh_ctx::Denoise& dn = c->dn;
   if (dn.calls == 0) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   for (int k = 0; k < 4; k++)
      if (int st = stage_ms(c, dn.stage[k], &out->pass_ms[k])) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, dn.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->geometry_pixels = counters[0];
   out->history_pixels = counters[1];
   return UH_OK;
}
