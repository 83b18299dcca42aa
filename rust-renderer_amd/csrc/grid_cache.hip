// grid_cache.hip - upkeep of the context's two visibility grids (sun_grid.h; uh_ctx::sun and uh_ctx::cam, context_state.h
// CachedGrid): when one is built (the policy itself: grid_cache.h), the builders' results becoming the context's grid, the sun
// grid's inline records and coarse cover, the grids' figures in UhStats and the builder-against-builder diagnostic. Host code only:
// the builders' kernels are sun_grid_build.hip, the host builder sun_grid.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "context_state.h"

// the grid's frame and raster from one of SunGridHost, SunGridParams (what a builder chose) and SunGridDev (what the kernels are
// told) into another of them
template <class From, class To> static void copy_frame_and_raster(const From& f, To& t) {
   std::memcpy(t.U, f.U, sizeof(t.U));
   std::memcpy(t.V, f.V, sizeof(t.V));
   std::memcpy(t.W, f.W, sizeof(t.W));
   t.u0 = f.u0, t.v0 = f.v0, t.inv_cell = f.inv_cell;
   t.nx = f.nx, t.ny = f.ny;
}

static int host_builder_threads() {
   const int threads = (int)std::thread::hardware_concurrency();
   return threads < 1 ? 1 : (threads > 32 ? 32 : threads);
}

// the packets as the device holds them (leaf order; host build, device build and refit all end there), 12 floats each
static int read_packets(uh_ctx* c, std::vector<float>& packets) {
   packets.resize(12 * (size_t)c->scene.num_tris);
   HIP_TRY(c, hipMemcpy2D(packets.data(), sizeof(TriPacket), c->d_tris.p, 16 * kTriStride16, sizeof(TriPacket), c->scene.num_tris, hipMemcpyDeviceToHost));
   return UH_OK;
}

template <int N>
void CachedGrid<N>::adopt(SunGridDevice& g, bool ok, uint64_t geom, const float* key, uint32_t cell_words) {
   cache.built_for(geom, key);
   valid = ok;
   why = g.why_not;
   mean_list = (float)g.mean_list;
   max_list_interior = g.max_list_interior;
   cells = entries = 0;
   dev = SunGridDev{};  // (the sun grid's recs and coarse cover: attach_sun_inline_records)
   release();
   if (ok) {
      d_cells.take(g.cells, cell_words * ((size_t)g.params.nx * g.params.ny + 1));
      d_entries.take(g.entries, (size_t)g.num_entries);
      copy_frame_and_raster(g.params, dev);
      dev.max_walk = limits.max_walk;
      dev.cell_start = d_cells.p;
      dev.entries = d_entries.p;
      cells = g.params.nx * g.params.ny;
      entries = (uint32_t)g.num_entries;
   }
   g.release();
}

// the host builder's grid `h` (or its refusal) as the device builder leaves its own: `g` owns two device allocations
static hipError_t upload_sun_grid(const SunGridHost& h, bool ok, SunGridDevice& g) {
   g = SunGridDevice();
   g.why_not = h.why_not;
   g.mean_list = h.mean_list;
   if (!ok) return hipSuccess;
   copy_frame_and_raster(h, g.params);
   g.num_entries = h.entries.size();
   // per cell four words: offset into the entries | cover depth | the first entry (packet, far depth) (sun_grid.h kSunCellWords)
   std::vector<uint32_t> cells(kSunCellWords * h.cell_start.size());
   for (size_t k = 0; k < h.cell_start.size(); k++) {
      const float cover = k < h.cell_cover.size() ? h.cell_cover[k] : -INFINITY;
      cells[kSunCellWords * k] = h.cell_start[k];
      std::memcpy(&cells[kSunCellWords * k + 1], &cover, 4);
      SunGridEntry first{kEmptyRef, 0.0f};
      if (k + 1 < h.cell_start.size() && h.cell_start[k + 1] > h.cell_start[k]) first = h.entries[h.cell_start[k]];
      cells[kSunCellWords * k + 2] = first.packet;
      std::memcpy(&cells[kSunCellWords * k + 3], &first.wmax, 4);
   }
   const size_t cell_bytes = cells.size() * sizeof(uint32_t), entry_bytes = h.entries.size() * sizeof(SunGridEntry);
   hipError_t e;
   if ((e = hipMalloc((void**)&g.cells, cell_bytes)) != hipSuccess || (e = hipMalloc((void**)&g.entries, entry_bytes ? entry_bytes : sizeof(SunGridEntry))) != hipSuccess ||
       (e = hipMemcpy(g.cells, cells.data(), cell_bytes, hipMemcpyHostToDevice)) != hipSuccess)
      return e;
   return entry_bytes ? hipMemcpy(g.entries, h.entries.data(), entry_bytes, hipMemcpyHostToDevice) : hipSuccess;
}

// behind every adoption of a sun grid: the coarse cover of its cells, and its lists once more with the packets inline (sun_grid.h
// SunGridDev::recs): 64 bytes per entry
static int attach_sun_inline_records(uh_ctx* c) {
   CachedGrid<3>& s = c->sun;
   SunGridExtras& x = c->sun_x;
   x.release();
   if (s.valid && x.coarse_shift) {  // the coarse cover (sun_grid.h)
      const uint32_t sh = x.coarse_shift, b = 1u << sh, cnx = (s.dev.nx + b - 1) / b, cny = (s.dev.ny + b - 1) / b;
      HIP_TRY(c, x.d_coarse.alloc((size_t)cnx * cny));
      HIP_TRY(c, (hipError_t)build_sun_coarse_cover((void*)c->stream, s.d_cells.p, s.dev.nx, s.dev.ny, sh, x.d_coarse.p));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      s.dev.coarse = x.d_coarse.p;
      s.dev.coarse_shift = sh;
      s.dev.coarse_nx = cnx;
   }
   const uint64_t n = s.entries;
   const uint64_t budget = x.inline_max_mb < 0 ? 4ull * 16 * kTriStride16 * c->scene.num_tris : (uint64_t)x.inline_max_mb << 20;
   if (!s.valid || n == 0 || n * 64ull > budget) return UH_OK;
   if (x.d_recs.alloc((size_t)n * 4) != hipSuccess) {  // no room: the plain lists serve
      (void)hipGetLastError();
      return UH_OK;
   }
   HIP_TRY(c, (hipError_t)build_sun_inline_records((void*)c->stream, c->d_tris.p, s.d_entries.p, n, x.d_recs.p));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   s.dev.recs = reinterpret_cast<const float*>(x.d_recs.p);
   return UH_OK;
}

static float ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int ensure_sun_grid(uh_ctx* c, const float dir[3]) {
   CachedGrid<3>& s = c->sun;
   s.this_frame = false;
   if (!c->sun_grid_enabled || c->scene.num_tris == 0) return UH_OK;
   // another direction or other geometry than the grid's (a sun dragged in the UI, instances moved with rebuild_tlas every frame)
   // walks the tree until it has settled; the first request of all builds at once
   const GridDecision what = s.cache.decide(c->geom_version, dir, true);
   if (what == GridDecision::Use) s.this_frame = s.valid;
   if (what != GridDecision::Build) return UH_OK;
   // inside this frame call; the frames in flight may still read the grid this one replaces
   if (int st = sync_all(c)) return st;
   const auto t0 = std::chrono::steady_clock::now();
   SunGridDevice g;
   bool ok;
   if (c->sun_x.device_build) {  // from the packets where they lie: a few milliseconds
      ok = build_sun_grid_device((void*)c->stream, c->d_tris.p, c->scene.num_tris, dir, s.limits, nullptr, g);
      if (!ok && g.why_not.rfind("device build:", 0) == 0) return fail(c, UH_ERR_HIP, "sun grid: " + g.why_not);
   } else {
      std::vector<float> packets;
      if (int st = read_packets(c, packets)) return st;
      SunGridHost h;
      ok = build_sun_grid(packets.data(), c->scene.num_tris, dir, s.limits, host_builder_threads(), h);
      const hipError_t e = upload_sun_grid(h, ok, g);
      if (e != hipSuccess) g.release();
      HIP_TRY(c, e);
   }
   s.adopt(g, ok, c->geom_version, dir, kSunCellWords);
   if (int st = attach_sun_inline_records(c)) return st;
   s.build_ms = ms_since(t0);
   s.this_frame = s.valid;
   return UH_OK;
}

int ensure_camera_grid(uh_ctx* c, const FrameParams& fp, uint32_t batch) {
   CachedGrid<32>& k = c->cam;
   k.this_frame = false;
   if (!c->cam_grid_enabled || c->scene.num_tris == 0) return UH_OK;
   float mats[32];
   std::memcpy(mats, fp.inv_view, sizeof(float) * 16);
   std::memcpy(mats + 16, fp.inv_proj, sizeof(float) * 16);
   // another camera or other geometry than the grid's - a first request too - waits until it has settled, or builds at once when
   // this call alone carries enough frames of it to repay the build
   const GridDecision what = k.cache.decide(c->geom_version, mats, false, batch >= 8);
   if (what == GridDecision::Use) k.this_frame = k.valid;
   if (what != GridDecision::Build) return UH_OK;
   if (int st = sync_all(c)) return st;
   const auto t0 = std::chrono::steady_clock::now();
   SunGridDevice g;
   const bool ok = build_camera_grid_device((void*)c->stream, c->d_tris.p, c->scene.num_tris, fp.inv_view, fp.inv_proj, c->W, c->H, k.limits, g);
   if (!ok && g.why_not.rfind("device build:", 0) == 0) return fail(c, UH_ERR_HIP, "camera grid: " + g.why_not);
   k.adopt(g, ok, c->geom_version, mats, 1);  // plain offsets: one word per cell
   if (k.valid) {
      k.dev.walk_whole = c->cam_walk_whole;
      k.cells = c->W * c->H;  // one per pixel: the border ring is not counted
   }
   k.build_ms = ms_since(t0);
   k.this_frame = k.valid;
   return UH_OK;
}

void grid_stats(const uh_ctx* c, UhStats* out) {
   const CachedGrid<3>& s = c->sun;
   out->sun_grid_cells = s.cells;  // (a refused grid: no cells, no entries, no buffers)
   out->sun_grid_entries = s.entries;
   out->sun_grid_bytes = s.bytes() + c->sun_x.bytes();
   out->sun_grid_build_ms = s.build_ms;
   out->sun_grid_mean_list = s.mean_list;
   const CachedGrid<32>& k = c->cam;
   out->camera_grid_build_ms = k.build_ms;
   out->camera_grid_mean_list = k.mean_list;
   if (!k.this_frame) return;  // cells, entries and bytes: of the grid in use by the last frame call
   out->camera_grid_cells = k.cells;
   out->camera_grid_entries = k.entries;
   out->camera_grid_bytes = k.bytes();
}

// diagnostics: the grid in use (built on the device) against the host builder on the same raster - see utopian_hip.h
extern "C" int uh_sun_grid_compare_builders(uh_ctx* c, uint64_t out[8]) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   for (int k = 0; k < 8; k++) out[k] = 0;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   const CachedGrid<3>& s = c->sun;
   if (!s.valid) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_sun_grid_compare_builders: no sun grid in use (" + s.why + ")");
   const size_t ncell = (size_t)s.dev.nx * s.dev.ny;
   std::vector<float> packets;
   if (int st = read_packets(c, packets)) return st;
   std::vector<uint32_t> cells(kSunCellWords * (ncell + 1));
   std::vector<SunGridEntry> entries(s.entries);
   HIP_TRY(c, hipMemcpy(cells.data(), s.d_cells.p, cells.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   if (!entries.empty()) HIP_TRY(c, hipMemcpy(entries.data(), s.d_entries.p, entries.size() * sizeof(SunGridEntry), hipMemcpyDeviceToHost));
   SunGridParams prm;
   copy_frame_and_raster(s.dev, prm);
   SunGridLimits lim = s.limits;
   lim.max_mean_list = 1e30;  // the comparison wants the host grid whatever the host builder thinks of its worth
   lim.max_fallback_area = 2.0;
   SunGridHost h;
   if (!build_sun_grid(packets.data(), c->scene.num_tris, s.cache.key, lim, host_builder_threads(), h, &prm)) return fail(c, UH_ERR_INVALID_ARGUMENT, "host builder refused: " + h.why_not);
   out[0] = ncell;
   out[1] = entries.size();
   out[2] = h.entries.size();
   if (h.cell_start.size() != ncell + 1) return fail(c, UH_ERR_INVALID_ARGUMENT, "host grid has another raster");
   std::vector<uint32_t> a, b;
   for (size_t k = 0; k < ncell; k++) {
      const uint32_t d0 = cells[kSunCellWords * k], d1 = cells[kSunCellWords * (k + 1)], h0 = h.cell_start[k], h1 = h.cell_start[k + 1];
      uint32_t hc;
      std::memcpy(&hc, &h.cell_cover[k], 4);
      if (cells[kSunCellWords * k + 1] != hc) out[5]++;  // cover depth: bit for bit
      if (d1 - d0 != h1 - h0 || d0 != h0) {
         out[3]++;  // another list length (or offset)
         continue;
      }
      const uint32_t ix = (uint32_t)(k % prm.nx), iy = (uint32_t)(k / prm.nx), len = d1 - d0;
      const bool walkable = !(ix == 0 || iy == 0 || ix == prm.nx - 1 || iy == prm.ny - 1) && len <= lim.max_walk;
      bool same = true;
      if (walkable) {
         out[6]++;
         for (uint32_t e = 0; e < len && same; e++) same = entries[d0 + e].packet == h.entries[h0 + e].packet && std::memcmp(&entries[d0 + e].wmax, &h.entries[h0 + e].wmax, 4) == 0;
      } else {
         // lists no ray walks are left in arrival order on the device: the same packets, as a set
         a.clear();
         b.clear();
         for (uint32_t e = 0; e < len; e++) {
            a.push_back(entries[d0 + e].packet);
            b.push_back(h.entries[h0 + e].packet);
         }
         std::sort(a.begin(), a.end());
         std::sort(b.begin(), b.end());
         same = a == b;
      }
      if (!same) out[4]++;
   }
   out[7] = (uint64_t)(h.build_ms * 1000.0);  // the host builder's time on this box, microseconds
   return UH_OK;
}
