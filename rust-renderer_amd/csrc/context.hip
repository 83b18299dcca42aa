// context.hip — the C ABI of include/utopian_hip.h: context lifetime, textures and lights, the per-frame pass chain and
// read-backs. Host-side counterpart of utopian::Renderer (utopian/src/renderer.rs), utopian::Raytracing (utopian/src/raytracing.rs) and
// build_path_tracing_render_graph (utopian/src/renderers/mod.rs:189-375) for this path only.
// struct uh_ctx is context_state.h; meshes, the tree builders and the refit are scene_build.hip; the hybrid and the forward graph
// (uh_render_hybrid, uh_render_forward) are hybrid_graph.hip (its verbs hybrid_verbs.hip, its display chain post_graph.hip) and forward_graph.hip over raster_driver.hip, the denoiser denoise_graph.hip;
// the sun and camera grids' upkeep is grid_cache.hip; uh_set_option is options.hip; a frame split over several GPUs - the tile and band
// partitions, the tile composition - is partition.hip, the RCCL link rccl_link.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bvh.h"
#include "context_internal.h"
#include "context_state.h"
#include "device_scan.h"
#include "device_types.h"
#include "texture_layout.h"
#include "tile_partition.h"
#include "utopian_hip.h"

using namespace uh;

namespace {
std::string g_create_error;
}

int fail(uh_ctx* c, int code, const std::string& msg) {
   if (c)
      c->err = msg;
   else
      g_create_error = msg;
   return code;
}

namespace {

void begin_timed(uh_ctx* c, int kind, hipStream_t stream = nullptr) {
   if (!stream) stream = c->stream;
   if (!c->time_kernels) return;
   EventPair ep;
   if (!c->free_events.empty()) {
      ep = c->free_events.back();
      c->free_events.pop_back();
   } else {
      (void)hipEventCreate(&ep.start);
      (void)hipEventCreate(&ep.stop);
   }
   ep.kind = kind;
   (void)hipEventRecord(ep.start, stream);
   c->pending.push_back(ep);
}
void end_timed(uh_ctx* c, hipStream_t stream = nullptr) {
   if (!c->time_kernels) return;
   (void)hipEventRecord(c->pending.back().stop, stream ? stream : c->stream);
}

}  // namespace

void drain_timed(uh_ctx* c) {
   for (EventPair& ep : c->pending) {
      float ms = 0.0f;
      if (hipEventSynchronize(ep.stop) == hipSuccess && hipEventElapsedTime(&ms, ep.start, ep.stop) == hipSuccess) {
         c->ms_by_kind[ep.kind] += ms;
         if (ep.kind == 0) c->trace_closest_launches++;
         if (ep.kind == 4) c->trace_light_launches++;
      }
      c->free_events.push_back(ep);
   }
   c->pending.clear();
}

LaunchCfg cfg(uh_ctx* c) {
   return LaunchCfg{c->stream, c->num_cus, c->closest_blocks_per_cu, c->shadow_blocks_per_cu, c->count_visits, c->fused_blocks_per_cu};
}

namespace {
std::string hip_version_string(int v) { return std::to_string(v / 10000000) + "." + std::to_string(v / 100000 % 100) + "." + std::to_string(v % 100000); }
// "" when the runtime's major.minor is the one this library was built with
std::string hip_skew_warning() {
   int built = 0, rt = 0;
   if (uh_hip_versions(&built, &rt) != UH_OK || rt / 100000 == built / 100000) return "";
   return "warning: libutopian_hip.so was built with HIP " + hip_version_string(built) + " but this process runs it on HIP runtime " + hip_version_string(rt) +
          " (another libamdhip64.so.7 was loaded first - e.g. the copy bundled with a PyTorch wheel); link or preload the ROCm release the library was built with";
}
}  // namespace

extern "C" {

// The HIP release this library was compiled by (the hipcc whose headers and code objects are in it) and the one it RUNS on (whichever
// libamdhip64.so.7 the process bound first). They can differ: the soname covers every 7.x, and a host that has another copy loaded -
// the PyTorch wheel bundles ROCm 7.0's - hands that copy to this library too. Both go on record, and a differing major.minor is
// said out loud (round 4's heap corruption under context churn showed with a 7.2-built library on the wheel's 7.0 runtime only).
int uh_hip_versions(int* built, int* runtime) {
   if (built) *built = HIP_VERSION;
   int rt = 0;
   const hipError_t e = hipRuntimeGetVersion(&rt);
   if (runtime) *runtime = e == hipSuccess ? rt : 0;
   return e == hipSuccess ? UH_OK : UH_ERR_HIP;
}

const char* uh_version(void) {
   static const std::string s = [] {
      int built = 0, rt = 0;
      (void)uh_hip_versions(&built, &rt);
      return "utopian-hip 0.5 (gfx950; built with HIP " + hip_version_string(built) + "; HIP runtime " + (rt ? hip_version_string(rt) : std::string("unknown")) + ")";
   }();
   return s.c_str();
}

const char* uh_last_error(uh_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int uh_create(int device_ordinal, uint32_t width, uint32_t height, uh_ctx** out) {
   if (!out || width == 0 || height == 0 || (uint64_t)width * height > (1ull << 26)) return fail(nullptr, UH_ERR_INVALID_ARGUMENT, "bad size");
   int ndev = 0;
   hipError_t e = hipGetDeviceCount(&ndev);
   if (e != hipSuccess || ndev == 0)
      return fail(nullptr, UH_ERR_NO_DEVICE, std::string("no HIP device visible (") + hipGetErrorString(e) + "); this library has no CPU fallback");
   if (device_ordinal < 0 || device_ordinal >= ndev) return fail(nullptr, UH_ERR_INVALID_ARGUMENT, "device ordinal out of range");
   uh_ctx* c = new uh_ctx();
   c->device = device_ordinal;
   c->W = width;
   c->H = height;
   auto bail = [&](int code) {
      g_create_error = c->err;
      uh_destroy(c);
      return code;
   };
#define CREATE_TRY(expr)                                                                      \
   do {                                                                                       \
      hipError_t e_ = (expr);                                                                 \
      if (e_ != hipSuccess) {                                                                 \
         c->err = std::string(#expr) + ": " + hipGetErrorString(e_);                          \
         return bail(e_ == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP);          \
      }                                                                                       \
   } while (0)
   CREATE_TRY(hipSetDevice(device_ordinal));
   hipDeviceProp_t prop;
   CREATE_TRY(hipGetDeviceProperties(&prop, device_ordinal));
   c->num_cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256;
   {
      uint32_t occ = query_trace_occupancy();  // blocks/CU the traversal kernels can keep resident
      if (c->closest_blocks_per_cu > occ) c->closest_blocks_per_cu = occ;
      if (c->shadow_blocks_per_cu > occ) c->shadow_blocks_per_cu = occ;
   }
   const size_t n = (size_t)width * height;
   CREATE_TRY(c->slots[0].create(n));
   CREATE_TRY(c->accumulation.alloc(n));
   CREATE_TRY(c->gbuffer.alloc(n));
   CREATE_TRY(c->output.alloc(n));
   for (auto& r : c->reservoirs) CREATE_TRY(r.alloc(n));
   CREATE_TRY(c->dstats.alloc(1));
   CREATE_TRY(hipMemsetAsync(c->accumulation.p, 0, n * sizeof(float4), c->stream));
   CREATE_TRY(hipMemsetAsync(c->output.p, 0, n * sizeof(uchar4), c->stream));
   CREATE_TRY(hipMemsetAsync(c->gbuffer.p, 0, n * sizeof(float4), c->stream));
   for (auto& r : c->reservoirs) CREATE_TRY(hipMemsetAsync(r.p, 0, n * sizeof(UhReservoir), c->stream));
   CREATE_TRY(hipMemsetAsync(c->dstats.p, 0, sizeof(DeviceStats), c->stream));
   // c / 255.0f table (exact host division; replaces 12 IEEE divides per bilinear fetch)
   float lut[256];
   for (int i = 0; i < 256; i++) lut[i] = (float)i / 255.0f;
   CREATE_TRY(c->d_lut.alloc(256));
   CREATE_TRY(hipMemcpy(c->d_lut.p, lut, sizeof(lut), hipMemcpyHostToDevice));
   CREATE_TRY(hipStreamSynchronize(c->stream));
#undef CREATE_TRY
   c->im.accumulation = c->accumulation.p;
   c->im.output = c->output.p;
   c->im.gbuffer_pos = c->gbuffer.p;
   for (int i = 0; i < 3; i++) c->im.reservoirs[i] = c->reservoirs[i].p;
   c->im.prev_spatial = c->reservoirs[2].p;
   c->res_stride = n;
   c->bands.rows = height;
   c->cam.limits.max_walk = 48;          // a pixel listing more packets than this hands its ray to the tree walk
   c->cam.limits.max_mean_list = 24.0;   // entries per occupied pixel beyond which the grid is refused (the tree walk costs about 20 records per ray)
   c->cam.limits.max_fallback_area = 2.0;
   // a runtime of another release than the one the library was built with: uh_last_error(NULL) says so after a SUCCESSFUL create too,
   // and stderr once per process
   g_create_error = hip_skew_warning();
   if (!g_create_error.empty()) {
      static bool said = false;
      if (!said) std::fprintf(stderr, "[libutopian_hip] %s\n", g_create_error.c_str());
      said = true;
   }
   *out = c;
   return UH_OK;
}

void uh_destroy(uh_ctx* c) {
   if (!c) return;
   (void)hipSetDevice(c->device);
   // the communicator's collectives were enqueued on the reservoir stream: it goes (and every stream is drained) while that
   // stream still exists
   if (c->bands.link) (void)sync_all(c);
   c->bands.destroy();
   // every stream idle before anything goes; the streams themselves go LAST, after every event that was recorded on or waited for by
   // one of them (slot streams wait for the reservoir stream's event and the other way round)
   (void)hipDeviceSynchronize();
   c->spatial_ring.release();
   c->gb_ray_o.release();
   c->gb_ray_d.release();
   c->gb_hit.release();
   for (auto& s : c->slots) {
      if (s.stream) (void)hipStreamSynchronize(s.stream);
      if (s.side) (void)hipStreamSynchronize(s.side);
   }
   for (auto& t : c->textures)
      if (t.dev) (void)hipFree(t.dev);
   for (auto& ep : c->pending) {
      (void)hipEventDestroy(ep.start);
      (void)hipEventDestroy(ep.stop);
   }
   for (auto& ep : c->free_events) {
      (void)hipEventDestroy(ep.start);
      (void)hipEventDestroy(ep.stop);
   }
   c->d_nodes.release();
   c->d_tris.release();
   c->d_shade.release();
   c->d_lights.release();
   c->d_meshes.release();
   c->d_obj_corners.release();
   c->d_world_corners.release();
   c->d_node_box.release();
   c->d_refit_meshes.release();
   c->d_src.release();
   c->d_tex.release();
   c->d_lut.release();
   c->sun.release();
   c->sun_x.release();
   c->cam.release();
   c->accumulation.release();
   c->gbuffer.release();
   c->output.release();
   for (auto& r : c->reservoirs) r.release();
   c->dstats.release();
   for (HostMesh& m : c->meshes) {
      if (m.d_verts) (void)hipFree(m.d_verts);
      if (m.d_indices) (void)hipFree(m.d_indices);
   }
   for (hipEvent_t ev : c->mupd.ev)
      if (ev) (void)hipEventDestroy(ev);
   c->mupd.table.release();
   c->mupd.flag.release();
   for (hipEvent_t ev : {c->iso.begin, c->iso.end})
      if (ev) (void)hipEventDestroy(ev);
   c->iso.counts.release();
   c->iso.chunks.release();
   c->iso.box.release();
   c->iso.total.release();
   destroy_graphs(c);  // (their events were recorded on the slots' streams: they go first)
   for (auto& s : c->slots) s.destroy();
   for (hipEvent_t ev : c->ev_band)
      if (ev) (void)hipEventDestroy(ev);
   if (c->restir_stream) {
      for (hipEvent_t ev : {c->ev_restir, c->rs_start, c->rs_stop})
         if (ev) (void)hipEventDestroy(ev);
      (void)hipStreamDestroy(c->restir_stream);
      c->restir_stream = nullptr;
   }
   c->tiles.destroy();
   delete c;
}

int uh_add_texture_rgba8(uh_ctx* c, const uint8_t* pixels, uint32_t w, uint32_t h, uint32_t* out_index) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!pixels || !w || !h) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_add_texture_rgba8: null or empty texture");
   // Overlapped blocks, one per cache line (texture_layout.h), whatever the size; with option "texture_blocks" 0: 8x8-texel tiles
   // when both sides are multiples of 8, rows otherwise (device_types.h TexInfo)
   size_t texels = (size_t)w * h;
   uint32_t tiles_x = 0, blocks_x = 0;
   std::vector<uint8_t> packed;
   const uint8_t* src = pixels;
   if (c->texture_blocks) {
      if (TexLayout::texel_count(w, h, &texels) != UH_OK)
         return fail(c, UH_ERR_CAPACITY, "uh_add_texture_rgba8: the blocked texture would hold more than 2^32 texels (option texture_blocks = 0 stores it as it is)");
      blocks_x = (uint32_t)TexLayout::blocks_x(w);
      packed.resize(texels * 4);
      TexLayout::repack(pixels, w, h, packed.data());
      src = packed.data();
   } else if (w % 8 == 0 && h % 8 == 0) {
      tiles_x = w / 8;
      packed.resize(texels * 4);
      for (uint32_t y = 0; y < h; y++)
         for (uint32_t x = 0; x < w; x++) {
            size_t at = ((size_t)((y >> 3) * tiles_x + (x >> 3)) << 6) + ((y & 7) << 3) + (x & 7);
            std::memcpy(&packed[at * 4], &pixels[((size_t)y * w + x) * 4], 4);
         }
      src = packed.data();
   }
   HIP_TRY(c, hipSetDevice(c->device));
   uchar4* dev = nullptr;
   HIP_TRY(c, hipMalloc((void**)&dev, texels * 4));
   hipError_t e = hipMemcpy(dev, src, texels * 4, hipMemcpyHostToDevice);
   if (e != hipSuccess) {
      (void)hipFree(dev);
      return fail(c, UH_ERR_HIP, std::string("texture upload: ") + hipGetErrorString(e));
   }
   c->textures.push_back(uh_ctx::HostTex{w, h, dev, tiles_x, blocks_x});
   c->built = false;
   if (out_index) *out_index = (uint32_t)c->textures.size() - 1;
   return UH_OK;
}

int uh_add_light(uh_ctx* c, const UhGpuLight* light, uint32_t* out_index) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!light) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_add_light: null light");
   if (c->lights.size() >= UH_MAX_GPU_LIGHTS) return fail(c, UH_ERR_CAPACITY, "uh_add_light: more than 1024 lights (MAX_NUM_GPU_LIGHTS)");
   c->lights.push_back(*light);
   c->built = false;
   c->topology_valid = false;
   if (out_index) *out_index = (uint32_t)c->lights.size() - 1;
   return UH_OK;
}

int uh_get_num_lights(uh_ctx* c, uint32_t* out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   *out = (uint32_t)c->lights.size();
   return UH_OK;
}

extern "C++" FrameParams make_params(uh_ctx* c, const UhViewUniformData& v) {
   FrameParams fp;
   std::memset(&fp, 0, sizeof(fp));
   std::memcpy(fp.inv_view, v.inverse_view, sizeof(fp.inv_view));
   std::memcpy(fp.inv_proj, v.inverse_projection, sizeof(fp.inv_proj));
   std::memcpy(fp.prev_pv, v.prev_frame_projection_view, sizeof(fp.prev_pv));
   // normalize(view.sun_dir) (reference.rgen:64, reference.rmiss:18): v * (1 / sqrt(dot))
   float d = (v.sun_dir[0] * v.sun_dir[0] + v.sun_dir[1] * v.sun_dir[1]) + v.sun_dir[2] * v.sun_dir[2];
   float inv = 1.0f / std::sqrt(d);
   for (int a = 0; a < 3; a++) fp.sun_dir[a] = v.sun_dir[a] * inv;
   fp.W = c->W;
   fp.H = c->H;
   // reference.rgen:24: int(float(total_samples) + time * 10000.0)
   fp.frame_number = (uint32_t)(int32_t)((float)v.total_samples + v.time * 10000.0f);
   fp.batch_frames = 1;
   fp.frame_numbers[0] = fp.frame_number;
   fp.total_samples_of[0] = v.total_samples;
   fp.samples_per_frame = v.samples_per_frame;
   fp.total_samples = v.total_samples;
   fp.num_bounces = v.num_bounces;
   fp.accumulation_limit = v.accumulation_limit;
   fp.sky_enabled = v.sky_enabled;
   fp.sun_shadow_enabled = v.sun_shadow_enabled;
   fp.lights_enabled = v.lights_enabled;
   fp.use_ris = v.use_ris_light_sampling;
   fp.full_frame_restir = c->full_frame_restir ? 1u : 0u;
   fp.furnace = c->furnace ? 1u : 0u;
   fp.num_lights_used = v.num_lights < v.max_num_lights_used ? v.num_lights : v.max_num_lights_used;
   fp.temporal_enabled = v.temporal_reuse_enabled;
   fp.spatial_enabled = v.spatial_reuse_enabled;
   fp.tp_rank = c->tiles.rank;
   fp.tp_world = c->tiles.world;
   fp.tp_tile = c->tiles.tile;
   fp.tiles_x = tiles_across(c->W, c->tiles.tile);
   fp.owned_pixels = c->tiles.world > 1 ? c->tiles.owned_pixels.p : nullptr;
   fp.n_owned = traced_pixels(c);
   return fp;
}

// every stream of every slot idle (read-backs, scene rebuilds, stats)
extern "C++" int sync_all(uh_ctx* c) {
   if (c->restir_stream) HIP_TRY(c, hipStreamSynchronize(c->restir_stream));
   for (auto& s : c->slots) {
      if (!s.ready) continue;
      HIP_TRY(c, hipStreamSynchronize(s.stream));
      HIP_TRY(c, hipStreamSynchronize(s.side));
   }
   return UH_OK;
}

// slot i exists and can hold `batch` frames worth of paths
static int ensure_slot(uh_ctx* c, uint32_t i, uint32_t batch = 1) {
   size_t need = (size_t)traced_pixels(c) * batch;  // path ids are dense over the rank's owned pixels
   if (need < 64) need = 64;  // a rank that owns no pixel (more ranks than tiles) still gets a well-formed, empty slot
   Slot& s = c->slots[i];
   if (s.ready && s.capacity >= need) return UH_OK;
   if (s.ready) {
      HIP_TRY(c, hipStreamSynchronize(s.stream));
      HIP_TRY(c, hipStreamSynchronize(s.side));
      if (c->last_acc == s.ev_acc) c->last_acc = nullptr;
      for (hipEvent_t& r : c->spatial_reader)
         if (r == s.ev_acc) r = nullptr;
      if (c->t_start == s.frame_start) c->t_start = nullptr;
      if (c->t_stop == s.frame_stop) c->t_stop = nullptr;
      if (c->last_slot == &s) c->last_slot = nullptr;
      s.destroy();
   }
   HIP_TRY(c, s.create(need));
   return UH_OK;
}

// reference_pt_pass of one frame on one slot (reference.rgen:22-145 as a kernel chain)
static int enqueue_path_trace(uh_ctx* c, Slot& s, const FrameParams& frame) {
   FrameParams fp = frame;  // + sun_verdicts, which follows the launches chosen below
   LaunchCfg lc = cfg(c);
   lc.stream = s.stream;
   if (fp.batch_frames == 1) {  // a lone frame's launches are small: fewer persistent waves reach the end of their tails sooner
      lc.closest_blocks_per_cu = std::min(lc.closest_blocks_per_cu, uh_ctx::kSingleFrameBlocksPerCu);
      lc.shadow_blocks_per_cu = std::min(lc.shadow_blocks_per_cu, uh_ctx::kSingleFrameBlocksPerCu);
   }
   Control* ctl = s.control.p;
   DeviceStats* st = c->dstats.p;
   // reference.rgen:28: samples of one frame run back to back (the raygen RNG state carries over)
   for (uint32_t smp = 0; smp < fp.samples_per_frame; smp++) {
      uint32_t slot = 0;
      // a lone frame: bounce 0 as a wavefront (its rays are coherent, the camera grid serves them), the others inside k_path_fused
      // ... when the caller waits for its frames (the frame before this one has left the GPU): the fused kernel fills the chip by
      // itself, so with frames in flight - a caller that does not wait - the wavefront's small launches interleave better (2.2 against
      // 2.5 ms per frame). Both give the same image.
      // ... and when the frame is not so large that its launches are wavefronts of a batch's size already (a 4K frame: 8.3 M paths -
      // the fused kernel 2.5 % behind on config 1, 12 % on config 3; at 1080p 12 % ahead, at 960 x 540 37 %, profiles/README.md)
      const bool gpu_idle = !c->last_acc || hipEventQuery(c->last_acc) == hipSuccess;
      const bool fused = c->fused_bounces && fp.batch_frames == 1 && fp.num_bounces >= 2 && fp.num_bounces <= 64 && s.ps.shard_cap < (1u << 23) &&
                         ((gpu_idle && fp.n_owned <= uh_ctx::kFusedMaxPaths) || c->fused_always);
      const bool fused_sun0 = fused && fp.sun_shadow_enabled == 1 && fp.lights_enabled != 1;  // bounce 0's sun rays inside the fused kernel too
      // The sun rays leave verdicts, and the kernels that read a path's radiance next add its throughput (option "sun_verdicts") - when
      // the grid serves them (the tree walk of every sun ray keeps the read-modify-write: a plane to clear and an atomic per lit ray
      // otherwise), when no light ray adds to the same radiance behind them (the reference adds the sun's term first, rgen:63-122, and
      // float addition does not commute bit for bit) and when the wavefront runs every bounce (the fused kernel adds its own terms)
      fp.sun_verdicts = (c->sun_x.verdicts && c->sun.this_frame && fp.sun_shadow_enabled == 1 && fp.lights_enabled != 1 && !fused) ? 1u : 0u;
      // The slim path state (option "slim_state", device_types.h PathState): where the verdicts hold no light sample rides with the path,
      // and with one sample per frame nothing reads the raygen RNG word behind bounce 0 - its place carries the path id
      fp.slim_state = (c->slim_state && fp.sun_verdicts == 1 && fp.samples_per_frame == 1) ? 1u : 0u;
      HIP_TRY(c, hipMemsetAsync(ctl, 0, sizeof(Control), s.stream));
      launch_generate(lc, fp, s.ps, ctl, smp);  // (behind the choice of the state: the origin quads it stores carry the id or the RNG word)
      for (uint32_t b = 0; b < (fused ? 1u : fp.num_bounces); b++) {
         begin_timed(c, (b == 0 && c->cam.this_frame) ? 3 : 0, s.stream);
         if (b == 0 && c->cam.this_frame) {
            // no tree walk for the primary rays of a camera at rest (and no launch for one when no pixel's list is too long for the grid kernel)
            launch_trace_camera_grid(lc, fp, c->scene, s.ps, ctl, st, slot, slot + 1, c->cam.dev, c->cam.max_list_interior > std::max(c->cam.dev.walk_whole, c->cam.dev.max_walk));
            slot += 2;
         } else
            launch_trace_closest(lc, c->scene, s.ps, ctl, st, b, slot++, b == 0 ? UH_RAY_PRIMARY : UH_RAY_BOUNCE);
         end_timed(c, s.stream);
         const bool side_shadow = c->overlap_shadow && (fp.sun_shadow_enabled == 1 || fp.lights_enabled == 1);
         const bool side_used = side_shadow || c->overlap_miss;
         // shade_hit(b) rewrites ray_o / thr / rad of the paths shadow(b-1) still reads on the side stream, and refills the
         // miss queue shade_miss(b-1) reads there
         if (side_used && b > 0) HIP_TRY(c, hipStreamWaitEvent(s.stream, s.ev_shadowed, 0));
         begin_timed(c, 2, s.stream);
         launch_shade_hit(lc, fp, c->scene, s.ps, c->im, ctl, st, b);  // also hands the bounce's misses to shade_miss (Q_MISS)
         if (!c->overlap_miss) launch_shade_miss(lc, fp, s.ps, ctl, st, b);
         end_timed(c, s.stream);
         // shade_miss(b) and the shadow queries of bounce b are independent of trace_closest(b+1) (they only read what
         // shade_hit(b) wrote): on the side stream their blocks fill the tail of the other kernel
         LaunchCfg lsh = lc;
         hipStream_t sh_stream = s.stream;
         if (side_used) {
            HIP_TRY(c, hipEventRecord(s.ev_shaded, s.stream));
            HIP_TRY(c, hipStreamWaitEvent(s.side, s.ev_shaded, 0));
         }
         if (c->overlap_miss) {
            LaunchCfg ls = lc;
            ls.stream = s.side;
            begin_timed(c, 2, s.side);
            launch_shade_miss(ls, fp, s.ps, ctl, st, b);
            end_timed(c, s.side);
         }
         if (side_shadow) {
            lsh.stream = s.side;
            sh_stream = s.side;
         }
         if (fp.sun_shadow_enabled == 1 && !fused_sun0) {
            begin_timed(c, 1, sh_stream);
            if (c->sun.this_frame) {
               launch_trace_sun_grid(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, c->sun.dev);
               launch_trace_shadow(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, false, true);  // the rays the grid handed over (border cells, long lists)
            } else
               launch_trace_shadow(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, false);
            end_timed(c, sh_stream);
         }
         if (fp.lights_enabled == 1) {
            begin_timed(c, 4, sh_stream);
            launch_trace_shadow(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, true);
            end_timed(c, sh_stream);
         }
         if (side_used) HIP_TRY(c, hipEventRecord(s.ev_shadowed, s.side));
      }
      const bool join_side = (c->overlap_miss || c->overlap_shadow) && fp.num_bounces > 0;
      // the side stream's work: the sky integrals, and - unless the fused kernel asks them itself - bounce 0's sun and light rays, whose
      // results the fused kernel starts from
      if (join_side && !fused_sun0) {
         HIP_TRY(c, hipEventRecord(s.ev_side_done, s.side));
         HIP_TRY(c, hipStreamWaitEvent(s.stream, s.ev_side_done, 0));
      }
      if (fused) {
         begin_timed(c, 0, s.stream);
         launch_path_fused(lc, fp, c->scene, s.ps, ctl, st, c->sun.dev, c->sun.this_frame, fused_sun0);
         end_timed(c, s.stream);
      }
      if (join_side && fused_sun0) {  // (bounce 0's sky integrals ran beside the fused kernel)
         HIP_TRY(c, hipEventRecord(s.ev_side_done, s.side));
         HIP_TRY(c, hipStreamWaitEvent(s.stream, s.ev_side_done, 0));
      }
      // the paths still alive after the last bounce: their radiance (with what the last bounce's shadow rays added) goes to the
      // per-id array the tail reads
      // (slim state: the last bounce's sun kernels stood at those positions with the verdict in hand and stored it themselves)
      if (fp.num_bounces > 0 && !fused && !fp.slim_state) launch_flush_survivors(lc, fp, s.ps, ctl);
      const bool last = smp + 1 == fp.samples_per_frame;
      // the accumulate / store tail (rgen:130-144) is a read-modify-write on the accumulation image:
      // frames must apply it in order, everything before it may overlap with other frames in flight
      if (last && c->last_acc && c->last_acc != s.ev_acc) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->last_acc, 0));
      launch_finish_sample(lc, fp, s.ps, c->im, smp, last);
   }
   if (fp.samples_per_frame == 0) {
      // zero samples: the raygen still runs its accumulate / store tail
      if (c->last_acc && c->last_acc != s.ev_acc) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->last_acc, 0));
      launch_resolve(lc, c->im, c->W, c->H, fp.total_samples, fp.accumulation_limit);
   }
   HIP_TRY(c, hipEventRecord(s.ev_acc, s.stream));
   c->last_acc = s.ev_acc;
   return UH_OK;
}

// ---- one batch of frames, in phases: begin | per frame: reservoir chain, exchange | end (the path-tracing wavefront).
// uh_render_frame(s) runs the phases back to back; an in-process group (mgpu.hip) interleaves them over its contexts,
// because frame f + 1's temporal pass of one GPU reads the bands every other GPU wrote in frame f.
struct uh_batch {
   FrameParams fp;
   uint32_t pass_mask = 0, batch = 0;
   bool restir_frame = false, reads_reservoirs = false;
   int read_slot[kMaxBatchFrames];
   LaunchCfg rc;
};

static UhReservoir* spatial_buf(uh_ctx* c, int slot) { return slot ? c->spatial_ring.p + (size_t)(slot - 1) * c->res_stride : c->reservoirs[2].p; }

static RowSpans spans_of(const uh_ctx* c, uint32_t row0, uint32_t rows, uint32_t extra0, uint32_t extra_rows) { return RowSpans{{row0, extra0}, {rows, extra_rows}, c->W}; }

static int batch_begin(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t batch, uh_batch& bs) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frame: null view");
   if (!c->built && c->topology_valid && view->rebuild_tlas == 1) {
      // the application moved instances and asks for the per-frame rebuild (main.rs:392,526; graph.rs:715-741)
      if (int st = uh_refit_acceleration(c)) return st;
   }
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_render_frame before uh_build_acceleration");
   if (view->num_bounces > kMaxBounces) return fail(c, UH_ERR_INVALID_ARGUMENT, "num_bounces > 64");
   if (view->samples_per_frame > 4096) return fail(c, UH_ERR_INVALID_ARGUMENT, "samples_per_frame > 4096 (the reference UI stops at 10)");
   if (view->num_lights > c->lights.size() && (view->lights_enabled == 1 || (pass_mask & UH_PASS_RESTIR)))
      return fail(c, UH_ERR_INVALID_ARGUMENT, "view.num_lights exceeds the lights added with uh_add_light");
   HIP_TRY(c, hipSetDevice(c->device));
   FrameParams& fp = bs.fp;
   fp = make_params(c, *view);
   fp.batch_frames = batch;
   for (uint32_t f = 0; f < batch; f++) {
      // frame f of the batch: total_samples advanced by the application once per frame (main.rs:467-469)
      const uint32_t total = view->total_samples + f * view->samples_per_frame;
      fp.total_samples_of[f] = total;
      fp.frame_numbers[f] = (uint32_t)(int32_t)((float)total + view->time * 10000.0f);
   }
   // the per-camera grid serves the primary rays of the path tracer and the G-buffer cast of this call
   c->cam.this_frame = false;
   const bool primary_rays = ((pass_mask & UH_PASS_REFERENCE_PT) && fp.num_bounces > 0 && fp.samples_per_frame > 0) || (pass_mask & UH_PASS_GBUFFER);
   if (primary_rays)
      if (int st = ensure_camera_grid(c, fp, batch)) return st;
   // with the camera grid nothing but bounce 0's own kernels reads a primary ray's state: it is not stored
   fp.primary_implicit = (c->primary_implicit && c->cam.this_frame && fp.samples_per_frame == 1) ? 1u : 0u;
   bs.pass_mask = pass_mask;
   bs.batch = batch;
   bs.restir_frame = (pass_mask & UH_PASS_RESTIR) != 0;
   // the path tracer reads spatial_reuse_reservoirs when it samples lights from them (rgen:98)
   bs.reads_reservoirs = (pass_mask & UH_PASS_REFERENCE_PT) && fp.lights_enabled == 1 && fp.use_ris == 1;

   if (batch > 1 && !(pass_mask & UH_PASS_REFERENCE_PT)) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frames: a batch needs the path-tracing pass");
   if (batch > kRestirBatch && bs.restir_frame) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frames: more reservoir-pass frames in one batch than the spatial ring holds");
   c->t_start = c->t_stop = nullptr;
   // the slot each frame of the batch samples lights from (rgen:98): without reservoir passes in this call, the current one
   for (uint32_t f = 0; f < kMaxBatchFrames; f++) bs.read_slot[f] = c->spatial_cur;

   if (bs.restir_frame) {
      if (!c->restir_stream) {
         HIP_TRY(c, hipStreamCreateWithFlags(&c->restir_stream, hipStreamNonBlocking));
         HIP_TRY(c, hipEventCreateWithFlags(&c->ev_restir, hipEventDisableTiming));
         HIP_TRY(c, hipEventCreate(&c->rs_start));
         HIP_TRY(c, hipEventCreate(&c->rs_stop));
      }
      if (!c->spatial_ring.p) {
         HIP_TRY(c, c->spatial_ring.alloc((size_t)(kSpatialRing - 1) * c->res_stride));
         // every slot is written before it is read - by this context's passes; under a row partition other ranks' bands arrive by
         // the exchange, and a caller that times one rank without one (exchange == NULL) must still read defined reservoirs
         if (c->bands.world > 1) HIP_TRY(c, hipMemsetAsync(c->spatial_ring.p, 0, c->spatial_ring.n * sizeof(UhReservoir), c->restir_stream));
         HIP_TRY(c, hipStreamSynchronize(c->stream));  // slot 0 (zeroed at creation or uh_write_reservoirs) is the history
      }
      bs.rc = cfg(c);
      bs.rc.stream = c->restir_stream;
      HIP_TRY(c, hipEventRecord(c->rs_start, c->restir_stream));
      c->t_start = c->rs_start;
   }
   return UH_OK;
}

// G-buffer cast and reservoir chain of frame f of the batch, on the reservoir stream
static int batch_restir_frame(uh_ctx* c, uh_batch& bs, uint32_t f) {
   if (!bs.restir_frame) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   const uint32_t pass_mask = bs.pass_mask;
   const size_t npix = (size_t)c->W * c->H;
   FrameParams ff = bs.fp;  // frame f of the batch: its own RNG frame number (the reservoir kernels read nothing else per frame)
   ff.frame_number = bs.fp.frame_numbers[f];
   ff.total_samples = bs.fp.total_samples_of[f];
   UhRestirRows rows;
   restir_rows(c, rows);
   const RowSpans band = spans_of(c, rows.band_row0, rows.band_rows, 0, 0);
   const RowSpans reuse = spans_of(c, rows.reuse_row0, rows.reuse_rows, rows.reuse_extra_row0, rows.reuse_extra_rows);
   const RowSpans cast = spans_of(c, rows.cast_row0, rows.cast_rows, rows.cast_extra_row0, rows.cast_extra_rows);
   Images im = c->im;
   im.prev_spatial = spatial_buf(c, c->spatial_cur);
   im.reservoirs[2] = spatial_buf(c, c->spatial_cur);
   if (pass_mask & UH_PASS_GBUFFER) {
      if (!c->gb_hit.p) {
         HIP_TRY(c, c->gb_ray_o.alloc(npix));
         HIP_TRY(c, c->gb_ray_d.alloc(npix));
         HIP_TRY(c, c->gb_hit.alloc(npix));
      }
      const RawRays gps{c->gb_ray_o.p, c->gb_ray_d.p, c->gb_hit.p};
      launch_gbuffer(bs.rc, ff, c->scene, gps, im, c->dstats.p, cast, band.total(), c->cam.this_frame ? &c->cam.dev : nullptr);
   }
   if (pass_mask & UH_PASS_RESET_RESERVOIRS) launch_reset_reservoirs(bs.rc, ff, im, reuse);
   if (pass_mask & UH_PASS_INITIAL_RIS) launch_initial_ris(bs.rc, ff, c->scene, im, reuse);
   if (pass_mask & UH_PASS_TEMPORAL_REUSE) launch_temporal_reuse(bs.rc, ff, c->scene, im, reuse);
   if (pass_mask & UH_PASS_SPATIAL_REUSE) {
      // writes the NEXT slot of the ring: the path-tracing wavefronts that still read the current one keep going
      const int nxt = (c->spatial_cur + 1) % kSpatialRing;
      if (c->spatial_reader[nxt]) HIP_TRY(c, hipStreamWaitEvent(c->restir_stream, c->spatial_reader[nxt], 0));
      im.reservoirs[2] = spatial_buf(c, nxt);
      launch_spatial_reuse(bs.rc, ff, c->scene, im, band);
      c->spatial_cur = nxt;
      c->im.reservoirs[2] = spatial_buf(c, nxt);
      if (c->bands.world > 1) {
         if (!c->ev_band[nxt]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_band[nxt], hipEventDisableTiming));
         HIP_TRY(c, hipEventRecord(c->ev_band[nxt], c->restir_stream));
      }
   }
   bs.read_slot[f] = c->spatial_cur;
   return UH_OK;
}

// the other ranks' bands of the buffer frame f's spatial pass wrote (uh_set_restir_partition)
static int batch_exchange(uh_ctx* c, uh_batch& bs, uint32_t f) {
   (void)f;
   if (!bs.restir_frame || !c->bands.exchange || !(bs.pass_mask & UH_PASS_SPATIAL_REUSE)) return UH_OK;  // world 1 with an exchange: a one-rank all-gather (rehearsals)
   HIP_TRY(c, hipSetDevice(c->device));
   const uint64_t band_bytes = (uint64_t)c->bands.rows * c->W * sizeof(UhReservoir);
   if (int st = c->bands.exchange(c->bands.user, (void*)c->restir_stream, (void*)c->im.reservoirs[2], band_bytes, c->bands.rank, c->bands.world))
      return fail(c, UH_ERR_HIP, std::string("the reservoir exchange reported error ") + std::to_string(st));
   return UH_OK;
}

static int batch_end(uh_ctx* c, uh_batch& bs) {
   HIP_TRY(c, hipSetDevice(c->device));
   FrameParams& fp = bs.fp;
   const uint32_t batch = bs.batch;
   if (bs.restir_frame) {
      HIP_TRY(c, hipEventRecord(c->ev_restir, c->restir_stream));
      c->restir_recorded = true;
      HIP_TRY(c, hipEventRecord(c->rs_stop, c->restir_stream));
      c->t_stop = c->rs_stop;
   }
   for (uint32_t f = 0; f < kMaxBatchFrames; f++) fp.spatial_of[f] = spatial_buf(c, bs.read_slot[f < batch ? f : 0]);

   if (bs.pass_mask & UH_PASS_REFERENCE_PT) {
      c->sun.this_frame = false;
      if (fp.sun_shadow_enabled == 1 && fp.num_bounces > 0 && fp.samples_per_frame > 0)
         if (int st = ensure_sun_grid(c, fp.sun_dir)) return st;
      const uint32_t in_flight = c->frames_in_flight ? c->frames_in_flight : 1;
      {
         const uint32_t si = c->next_slot;
         c->next_slot = (c->next_slot + 1) % in_flight;
         int st = ensure_slot(c, si, batch);
         if (st != UH_OK) return st;
         Slot& s = c->slots[si];
         const FrameParams& fk = fp;
         // rgen:98 reads this frame's spatial_reuse_reservoirs
         if (bs.reads_reservoirs && c->restir_recorded) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->ev_restir, 0));
         HIP_TRY(c, hipEventRecord(s.frame_start, s.stream));
         if (!c->t_start) c->t_start = s.frame_start;
         st = enqueue_path_trace(c, s, fk);
         if (st != UH_OK) return st;
         if (bs.reads_reservoirs)
            for (uint32_t f = 0; f < batch; f++) c->spatial_reader[bs.read_slot[f]] = s.ev_acc;
         HIP_TRY(c, hipEventRecord(s.frame_stop, s.stream));
         c->t_stop = s.frame_stop;
         c->last_slot = &s;
      }
   }
   c->frame_timed = true;
   c->frames += batch;
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

static int render_batch(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t batch) {
   uh_batch bs;
   if (int st = batch_begin(c, view, pass_mask, batch, bs)) return st;
   for (uint32_t f = 0; f < batch; f++) {
      if (int st = batch_restir_frame(c, bs, f)) return st;
      if (int st = batch_exchange(c, bs, f)) return st;
   }
   return batch_end(c, bs);
}

// frames one wavefront carries for this pass mask (option "batch_frames", 0 = auto), and the slots it will rotate through
static int plan_batch(uh_ctx* c, uint32_t pass_mask, uint32_t* out_batch) {
   uint32_t batch = c->batch_frames;
   if (!batch) {
      // auto: about 32 M paths per wavefront (1080p: 16 frames, 4K: 4, a rank's eighth of 1080p: 32, 256 x 256: 32) - what
      // the launches need to fill the chip and amortise their tails; 1080p 4 / 8 / 12 / 16 frames = 6,271 / 6,341 / 6,388 /
      // 6,398 Mrays/s, the short paths of the iso-surface scene 4,974 / 5,393 / - / 6,223 (tools/sweep_batch.sh,
      // profiles/README.md) - within 33 M path-state records per slot (3.7 GB; path ids are dense over the pixels a rank
      // owns, so its wavefronts carry more frames than a whole frame's would)
      const uint64_t pixels = (uint64_t)c->W * c->H, owned = c->tiles.n_owned ? c->tiles.n_owned : pixels;
      uint64_t b = (32u << 20) / (owned ? owned : 1), cap = (33u << 20) / (owned ? owned : 1);
      if (b > cap) b = cap;
      batch = (uint32_t)(b < 1 ? 1 : b);
   }
   if (batch > kMaxBatchFrames) batch = kMaxBatchFrames;
   if ((pass_mask & UH_PASS_RESTIR) && batch > kRestirBatch) batch = kRestirBatch;
   if (!(pass_mask & UH_PASS_REFERENCE_PT)) batch = 1;  // reservoir passes alone: frame by frame
   // create every frames-in-flight slot now: the first call (an application's first frames, a benchmark's
   // warm-up) pays for the allocations and stream creation, not whichever later wavefront first reaches a slot
   if (pass_mask & UH_PASS_REFERENCE_PT)
      for (uint32_t i = 0; i < (c->frames_in_flight ? c->frames_in_flight : 1); i++)
         if (int st = ensure_slot(c, i, batch)) return st;
   *out_batch = batch;
   return UH_OK;
}

// ---- the phases for an in-process group (csrc/context_internal.h; mgpu.hip) ----
int uhi_plan_batch(uh_ctx* c, uint32_t pass_mask, uint32_t* out_batch) {
   if (!c || !out_batch) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   return plan_batch(c, pass_mask, out_batch);
}
int uhi_batch_begin(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t batch, uh_batch** out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   uh_batch* bs = new uh_batch();
   int st = batch_begin(c, view, pass_mask, batch, *bs);
   if (st != UH_OK) {
      delete bs;
      bs = nullptr;
   }
   *out = bs;
   return st;
}
int uhi_batch_restir_frame(uh_ctx* c, uh_batch* bs, uint32_t f) { return (c && bs) ? batch_restir_frame(c, *bs, f) : UH_ERR_INVALID_ARGUMENT; }
int uhi_batch_end(uh_ctx* c, uh_batch* bs) {
   if (!c || !bs) return UH_ERR_INVALID_ARGUMENT;
   int st = batch_end(c, *bs);
   delete bs;
   return st;
}
void uhi_batch_abandon(uh_batch* bs) { delete bs; }
// what a peer pulls a band from / into: the buffer the last spatial pass wrote, the event recorded behind that pass, the
// stream the passes run on
int uhi_exchange_endpoints(uh_ctx* c, void** spatial_base, void** band_event, void** stream, uint64_t* band_bytes) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (spatial_base) *spatial_base = (void*)c->im.reservoirs[2];
   if (band_event) *band_event = (void*)c->ev_band[c->spatial_cur];
   if (stream) *stream = (void*)c->restir_stream;
   if (band_bytes) *band_bytes = (uint64_t)c->bands.rows * c->W * sizeof(UhReservoir);
   return UH_OK;
}

int uhi_iso_reference_triangulation(uh_ctx* c) { return c && c->iso_reference ? 1 : 0; }

int uh_render_frame(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask) { return render_batch(c, view, pass_mask, 1); }

int uh_render_frames(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t count) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view || count == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frames: null view or zero frames");
   UhViewUniformData v = *view;
   uint32_t done = 0, batch = 1;
   if (int st = plan_batch(c, pass_mask, &batch)) return st;
   // wavefronts of equal size: 20 frames at 16 per wavefront go as 10 + 10, not 16 + 4 (a short wavefront's launches are mostly tail)
   const uint32_t n_batches = (count + batch - 1) / batch, even = (count + n_batches - 1) / n_batches;
   while (done < count) {
      uint32_t b = count - done < even ? count - done : even;
      int st = render_batch(c, &v, pass_mask, b);
      if (st != UH_OK) return st;
      done += b;
      v.total_samples += b * v.samples_per_frame;
   }
   return UH_OK;
}

int uh_reset_accumulation(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   HIP_TRY(c, hipMemsetAsync(c->accumulation.p, 0, c->accumulation.n * sizeof(float4), c->stream));
   HIP_TRY(c, hipMemsetAsync(c->output.p, 0, c->output.n * sizeof(uchar4), c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));  // the next frame may run on another slot's stream, which does not wait for this one
   return UH_OK;
}

int uh_synchronize(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   return sync_all(c);
}

// Device -> host, BLOCKING, behind a wait for the context's stream: every read-back of the library goes through here or is a
// plain hipMemcpy. (The round-4 soaks' heap corruption - profiles/README.md "the soak crash" - sits inside the HIP runtime copy
// bundled with the PyTorch wheel and does not show against /opt/rocm's; under the bundled one, asynchronous copies into locals
// followed by a wait for their stream made it twenty times as frequent, and a pinned staging buffer - per context or one for the
// process - made it worse again. This form is the one that ran cleanest under both.)
static int staged_read(uh_ctx* c, void* dst, const void* src, size_t bytes) {
   if (bytes == 0) return UH_OK;
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
   return UH_OK;
}

extern "C++" int read_back(uh_ctx* c, void* dst, const void* src, size_t bytes) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!dst) return fail(c, UH_ERR_INVALID_ARGUMENT, "null destination");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   return staged_read(c, dst, src, bytes);
}

int uh_read_accumulation(uh_ctx* c, float* out) { return read_back(c, out, c ? c->accumulation.p : nullptr, c ? c->accumulation.n * sizeof(float4) : 0); }
int uh_read_output_bgra8(uh_ctx* c, uint8_t* out) { return read_back(c, out, c ? c->output.p : nullptr, c ? c->output.n * sizeof(uchar4) : 0); }
int uh_read_gbuffer_position(uh_ctx* c, float* out) { return read_back(c, out, c ? c->gbuffer.p : nullptr, c ? c->gbuffer.n * sizeof(float4) : 0); }
int uh_read_reservoirs(uh_ctx* c, int which, UhReservoir* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (which < 0 || which > 2) return fail(c, UH_ERR_INVALID_ARGUMENT, "reservoir buffer index must be 0..2");
   // spatial_reuse_reservoirs is double-buffered (render_batch): the current one is what the reference's single buffer holds
   const UhReservoir* src = which == 2 ? c->im.reservoirs[2] : c->reservoirs[which].p;
   return read_back(c, out, src, (size_t)c->W * c->H * sizeof(UhReservoir));
}
int uh_write_reservoirs(uh_ctx* c, int which, const UhReservoir* in) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (which < 0 || which > 2 || !in) return fail(c, UH_ERR_INVALID_ARGUMENT, "reservoir buffer index must be 0..2");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   UhReservoir* dst = which == 2 ? c->im.reservoirs[2] : c->reservoirs[which].p;
   HIP_TRY(c, hipMemcpyAsync(dst, in, (size_t)c->W * c->H * sizeof(UhReservoir), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return UH_OK;
}

int uh_write_gbuffer_position(uh_ctx* c, const float* in) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!in) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_write_gbuffer_position: null source");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   HIP_TRY(c, hipMemcpyAsync(c->gbuffer.p, in, c->gbuffer.n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return UH_OK;
}

int uh_trace_closest(uh_ctx* c, const float* rays, uint32_t n, float* out_tuv, uint32_t* out_mesh, uint32_t* out_prim) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_trace_closest before uh_build_acceleration");
   if (n == 0) return UH_OK;
   if (!rays || !out_tuv || !out_mesh || !out_prim) return fail(c, UH_ERR_INVALID_ARGUMENT, "null argument");
   HIP_TRY(c, hipSetDevice(c->device));
   std::vector<float4> o(n), d(n);
   for (uint32_t i = 0; i < n; i++) {
      const float* r = rays + 8 * (size_t)i;
      o[i] = make_float4(r[0], r[1], r[2], r[3]);
      d[i] = make_float4(r[4], r[5], r[6], r[7]);
   }
   DevBuf<float4> d_o, dd, dh;
   HIP_TRY(c, d_o.alloc(n));
   HIP_TRY(c, dd.alloc(n));
   HIP_TRY(c, dh.alloc(n));
   HIP_TRY(c, hipMemcpyAsync(d_o.p, o.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(dd.p, d.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   begin_timed(c, 0);
   launch_trace_closest_raw(cfg(c), c->scene, d_o.p, dd.p, dh.p, n);
   end_timed(c);
   std::vector<float4> h(n);
   if (int st = staged_read(c, h.data(), dh.p, n * sizeof(float4))) return st;
   // packet index -> key needs the packet table: read keys back once
   std::vector<TriPacket> tp(c->scene.num_tris);
   if (!tp.empty()) HIP_TRY(c, hipMemcpy2D(tp.data(), sizeof(TriPacket), c->d_tris.p, 16 * kTriStride16, sizeof(TriPacket), tp.size(), hipMemcpyDeviceToHost));
   for (uint32_t i = 0; i < n; i++) {
      uint32_t idx;
      std::memcpy(&idx, &h[i].w, 4);
      if (idx == kEmptyRef || idx >= tp.size()) {
         out_tuv[3 * i] = -1.0f;
         out_tuv[3 * i + 1] = out_tuv[3 * i + 2] = 0.0f;
         out_mesh[i] = out_prim[i] = 0xffffffffu;
      } else {
         out_tuv[3 * i] = h[i].x;
         out_tuv[3 * i + 1] = h[i].y;
         out_tuv[3 * i + 2] = h[i].z;
         out_mesh[i] = tp[idx].key >> kPrimBits;
         out_prim[i] = tp[idx].key & kPrimMask;
      }
   }
   d_o.release();
   dd.release();
   dh.release();
   return UH_OK;
}

int uh_trace_any(uh_ctx* c, const float* rays, uint32_t n, uint8_t* out_occluded) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_trace_any before uh_build_acceleration");
   if (n == 0) return UH_OK;
   if (!rays || !out_occluded) return fail(c, UH_ERR_INVALID_ARGUMENT, "null argument");
   HIP_TRY(c, hipSetDevice(c->device));
   std::vector<float4> o(n), d(n);
   for (uint32_t i = 0; i < n; i++) {
      const float* r = rays + 8 * (size_t)i;
      o[i] = make_float4(r[0], r[1], r[2], r[3]);
      d[i] = make_float4(r[4], r[5], r[6], r[7]);
   }
   DevBuf<float4> d_o, dd;
   DevBuf<uint32_t> occ;
   HIP_TRY(c, d_o.alloc(n));
   HIP_TRY(c, dd.alloc(n));
   HIP_TRY(c, occ.alloc(n));
   HIP_TRY(c, hipMemcpyAsync(d_o.p, o.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(dd.p, d.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   begin_timed(c, 1);
   launch_trace_any_raw(cfg(c), c->scene, d_o.p, dd.p, occ.p, n);
   end_timed(c);
   std::vector<uint32_t> h(n);
   if (int st = staged_read(c, h.data(), occ.p, n * sizeof(uint32_t))) return st;
   for (uint32_t i = 0; i < n; i++) out_occluded[i] = h[i] ? 1 : 0;
   d_o.release();
   dd.release();
   occ.release();
   return UH_OK;
}

int uh_get_stats(uh_ctx* c, UhStats* out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   DeviceStats ds;
   if (int st = staged_read(c, &ds, c->dstats.p, sizeof(ds))) return st;
   drain_timed(c);
   if (c->frame_timed) {
      float ms = 0.0f;
      if (c->t_start && c->t_stop && hipEventElapsedTime(&ms, c->t_start, c->t_stop) == hipSuccess) c->last_frame_ms = ms;
   }
   std::memset(out, 0, sizeof(*out));
   for (int i = 0; i < UH_RAY_KINDS; i++) out->rays[i] = ds.rays[i];
   out->nodes_visited = ds.nodes_visited;
   out->tris_tested = ds.tris_tested;
   out->shadow_nodes_visited = ds.shadow_nodes_visited;
   out->shadow_tris_tested = ds.shadow_tris_tested;
   out->closest_hits = ds.closest_hits;
   out->misses = ds.misses;
   out->frames = c->frames;
   out->bvh_nodes = c->bvh_nodes;
   out->bvh_triangles = c->bvh_tris;
   out->build_ms = c->build_ms;
   out->last_frame_ms = c->last_frame_ms;
   out->trace_closest_ms = c->ms_by_kind[0];
   out->trace_shadow_ms = c->ms_by_kind[1];
   out->shade_ms = c->ms_by_kind[2];
   out->camera_grid_ms = c->ms_by_kind[3];
   out->trace_light_ms = c->ms_by_kind[4];
   out->trace_light_launches = c->trace_light_launches;
   out->light_nodes_visited = ds.light_nodes_visited;
   out->light_tris_tested = ds.light_tris_tested;
   out->trace_closest_launches = c->trace_closest_launches;
   out->sun_tree_rays = ds.sun_tree_rays;
   out->camera_tree_rays = ds.cam_tree_rays;
   out->camera_grid_tris_tested = ds.cam_tris_tested;
   out->sun_covered_rays = ds.sun_covered_rays;
   grid_stats(c, out);
   return UH_OK;
}

int uh_reset_stats(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   drain_timed(c);
   // on the context's stream and waited for: a hipMemset on the null stream may still be in flight when the call returns, and
   // the frames' non-blocking streams do not wait for it - the next frame's first counters could be wiped
   HIP_TRY(c, hipMemsetAsync(c->dstats.p, 0, sizeof(DeviceStats), c->stream));
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   c->frames = 0;
   for (float& ms : c->ms_by_kind) ms = 0.0f;
   c->trace_closest_launches = c->trace_light_launches = 0;
   return UH_OK;
}

int uh_device_pointer(uh_ctx* c, int which, void** out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   if (which == 0)
      *out = c->accumulation.p;
   else if (which == 1)
      *out = c->output.p;
   else
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_device_pointer: which must be 0 or 1");
   return UH_OK;
}

int uh_stream(uh_ctx* c, void** out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));  // the caller is about to enqueue on it
   *out = (void*)c->stream;
   return UH_OK;
}

}  // extern "C"
