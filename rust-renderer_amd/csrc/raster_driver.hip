// raster_driver.hip - the host driver the rasterised passes share (the binning of one pass from its count kernel to its resolve
// kernel, the scene through the forward rasteriser, the light records and forward.frag) and the cascaded shadow maps, which the hybrid
// and the forward graph both render: uh_set_shadowmap_params, uh_read_shadow_map, uh_get_shadow_map_stats of include/utopian_hip.h.
// Host code over uh_ctx::Hybrid::sm and the RasterBins / RasterTarget of each pass (context_state.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "device_scan.h"
#include "graphs_internal.h"

// ---- what the rasterised passes share ----
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
void mat4_mul(const float* a, const float* b, float* o) {
   for (int col = 0; col < 4; col++)
      for (int r = 0; r < 4; r++) o[4 * col + r] = ((a[r] * b[4 * col] + a[4 + r] * b[4 * col + 1]) + a[8 + r] * b[4 * col + 2]) + a[12 + r] * b[4 * col + 3];
}
// an instance's 3x4 (HostMesh::o2w, row-major) with row (0, 0, 0, 1), column-major
void mat4_from_3x4(const float* o, float* w) {
   for (int col = 0; col < 4; col++) {
      for (int r = 0; r < 3; r++) w[4 * col + r] = o[4 * r + col];
      w[4 * col + 3] = col == 3 ? 1.0f : 0.0f;
   }
}

uint32_t forward_frame(const uh_ctx* c, const RasterTarget& t, ForwardDev& fd) {
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

void light_and_shade(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, const ForwardDev& fd, HybridLight* lights, bool flat) {
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
   const ShadowLookup sl{h.sm.maps.p, h.sm.dev_params.p, h.sm.size};
   launch_forward_shade(lc, c->scene, fd, fs, view.shadows_enabled == 1 ? &sl : nullptr, flat);
}

int bin_forward(uh_ctx* c, const LaunchCfg& lc, RasterBins& b, ForwardDev& fd, uint32_t tiles, const char* who, bool flat, uint32_t* pieces) {
   unsigned long long totals[2];
   // record ids below 2^32 - 1: the resolve's key holds 0xFFFFFFFE - record, and 0xFFFFFFFF stands for none
   const BinPass pass{fd.num_tris, tiles, 6, (1ull << 32) - 1, who, ": 2^32 - 1 or more triangle pieces, or 2^32 or more tile entries"};
   const int st = bin_and_resolve(
      c, b, pass, totals, [&] { launch_forward_count(lc, fd, flat); }, [] { return (int)UH_OK; },
      [&] {
         fd.records = b.records.p;
         fd.entries = b.entries.p;
         launch_forward_emit(lc, fd, flat);
         launch_forward_resolve(lc, fd, flat);
      });
   if (st) return st;
   *pieces = (uint32_t)totals[0];
   return UH_OK;
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

int raster_scene(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, RasterBins& b, const RasterTarget& t, ForwardDev& fd, const char* who, uint32_t* pieces) {
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
   return bin_forward(c, lc, b, fd, tiles, who, false, pieces);
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

// the four cascades through bin_and_resolve; the first record of each cascade is read with the totals
int render_shadow_maps(uh_ctx* c, const LaunchCfg& lc, const char* verb) {
   uh_ctx::Hybrid& h = c->hy;
   uh_ctx::Hybrid::ShadowMaps& sm = h.sm;
   RasterBins& b = sm.bins;
   const uint32_t S = c->shadow_map_size, tiles_x = (S + kShadowTile - 1) / kShadowTile, tiles = 4 * tiles_x * tiles_x;
   size_t ntri = 0;
   for (const HostMesh& m : c->meshes) ntri += m.tris();
   if (4 * ntri >= (1ull << 32)) return fail(c, UH_ERR_CAPACITY, std::string(verb) + ": shadow maps of more than 2^30 triangles");
   for (int st : {grow(c, sm.maps, 4 * (size_t)S * S, verb), grow(c, b.tile_count, tiles, verb), grow(c, b.tile_cursor, tiles, verb), grow(c, b.totals, 2, verb),
                  grow(c, sm.dev_params, 1, verb), grow(c, b.mats, std::max<size_t>(1, 64 * c->meshes.size()), verb),
                  grow(c, b.chunks, std::max<size_t>(1, scan_chunk_count((uint32_t)std::max<size_t>(4 * ntri, tiles))), verb)})
      if (st) return st;
   if (b.geom != c->geom_version || !b.rec_count.p) {
      HIP_TRY(c, b.tri_mesh.alloc(std::max<size_t>(1, ntri)));
      HIP_TRY(c, b.rec_count.alloc(std::max<size_t>(1, 4 * ntri)));
      if (int st = fill_tri_mesh(c, b.tri_mesh.p)) return st;
      b.geom = c->geom_version;
   }
   // until this render completes the maps and their params are invalid: a failure below leaves the deferred pass refused
   sm.size = 0;
   sm.pending = sm.params;
   cascade_mesh_matrices(c, sm.pending, b.mats_host);
   if (!b.mats_host.empty())
      HIP_TRY(c, hipMemcpyAsync(b.mats.p, b.mats_host.data(), b.mats_host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(sm.dev_params.p, &sm.pending, sizeof(UhShadowmapParams), hipMemcpyHostToDevice, c->stream));
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
   sd.maps = sm.maps.p;
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
   for (int k = 0; k < 4; k++) sm.tris[k] = (k < 3 ? first[k + 1] : (uint32_t)totals[0]) - first[k];
   sm.snapshot = sm.pending;
   sm.size = S;
   sm.renders++;
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
   c->hy.sm.params = *p;
   c->hy.sm.params_set = true;
   return UH_OK;
}

int uh_read_shadow_map(uh_ctx* c, int cascade, float* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid::ShadowMaps& sm = c->hy.sm;
   if (!sm.maps.p || !sm.size) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_shadow_map before the maps were rendered (UH_HYBRID_SHADOW_MAPS)");
   if (cascade < 0 || cascade > 3) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_shadow_map: cascade must be 0..3");
   const size_t n = (size_t)sm.size * sm.size;
   return read_back(c, out, sm.maps.p + (size_t)cascade * n, n * sizeof(float));
}

int uh_get_shadow_map_stats(uh_ctx* c, UhShadowMapStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_shadow_map_stats: null destination", c && c->hy.sm.renders != 0, &st)) return st;
   const uh_ctx::Hybrid::ShadowMaps& sm = c->hy.sm;
   if ((st = stage_ms(c, c->hy.stage[kStShadowMaps], &out->pass_ms))) return st;
   out->renders = sm.renders;
   out->size = sm.size;
   std::memcpy(out->triangles, sm.tris, sizeof(out->triangles));
   out->params = sm.snapshot;
   return UH_OK;
}
