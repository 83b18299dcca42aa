// context.hip — the C ABI of include/utopian_hip.h: context lifetime, textures and lights, reset and synchronise, the read-backs and
// writes, the two raw trace verbs and the stats, with the timed-event pool behind option "time_kernels". Host-side counterpart of
// utopian::Renderer (utopian/src/renderer.rs) and utopian::Raytracing (utopian/src/raytracing.rs) for this path only.
// struct uh_ctx is context_state.h; the path tracer's frames (uh_render_frame, uh_render_frames) are frame_loop.hip over the plan of
// frame_plan.h; meshes, the tree builders and the refit are scene_build.hip; the hybrid and the forward graph
// (uh_render_hybrid, uh_render_forward) are hybrid_graph.hip over the plan of hybrid_plan.h (its ray passes hybrid_ray_passes.hip, its
// other verbs hybrid_verbs.hip, its display chain post_graph.hip) and forward_graph.hip over raster_driver.hip, the denoiser denoise_graph.hip;
// the sun and camera grids' upkeep is grid_cache.hip; uh_set_option is options.hip; a frame split over several GPUs - the tile and band
// partitions, the tile composition - is partition.hip, the RCCL link rccl_link.hip.
#include <hip/hip_runtime.h>

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

void begin_timed(uh_ctx* c, int kind, hipStream_t stream) {
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
void end_timed(uh_ctx* c, hipStream_t stream) {
   if (!c->time_kernels) return;
   (void)hipEventRecord(c->pending.back().stop, stream ? stream : c->stream);
}

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
      if (m.pose) {
         m.pose->release();
         delete m.pose;
      }
   }
   for (hipEvent_t ev : c->pose.ev)
      if (ev) (void)hipEventDestroy(ev);
   c->pose.params.release();
   c->pose.flag.release();
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

int uhi_iso_reference_triangulation(uh_ctx* c) { return c && c->iso_reference ? 1 : 0; }

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

// the n rays of a raw trace verb (8 floats each: origin, tmin, direction, tmax) as the raw kernels read them: unpacked into o / d (n
// elements each), which the caller keeps until it has waited for the context's stream, and uploaded on that stream into d_o / dd
static int upload_rays(uh_ctx* c, const float* rays, uint32_t n, std::vector<float4>& o, std::vector<float4>& d, DevBuf<float4>& d_o, DevBuf<float4>& dd) {
   for (uint32_t i = 0; i < n; i++) {
      const float* r = rays + 8 * (size_t)i;
      o[i] = make_float4(r[0], r[1], r[2], r[3]);
      d[i] = make_float4(r[4], r[5], r[6], r[7]);
   }
   HIP_TRY(c, d_o.alloc(n));
   HIP_TRY(c, dd.alloc(n));
   HIP_TRY(c, hipMemcpyAsync(d_o.p, o.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   HIP_TRY(c, hipMemcpyAsync(dd.p, d.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
   return UH_OK;
}

int uh_trace_closest(uh_ctx* c, const float* rays, uint32_t n, float* out_tuv, uint32_t* out_mesh, uint32_t* out_prim) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_trace_closest before uh_build_acceleration");
   if (n == 0) return UH_OK;
   if (!rays || !out_tuv || !out_mesh || !out_prim) return fail(c, UH_ERR_INVALID_ARGUMENT, "null argument");
   HIP_TRY(c, hipSetDevice(c->device));
   std::vector<float4> o(n), d(n);
   DevBuf<float4> d_o, dd, dh;
   HIP_TRY(c, dh.alloc(n));
   if (int st = upload_rays(c, rays, n, o, d, d_o, dd)) return st;
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
   DevBuf<float4> d_o, dd;
   DevBuf<uint32_t> occ;
   HIP_TRY(c, occ.alloc(n));
   if (int st = upload_rays(c, rays, n, o, d, d_o, dd)) return st;
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

// (the kernel times by kind: a pass whose bounce 0 is k_primary_shade - SamplePlan::fused_primary - books it under kind 2, shading, and
// nothing under kind 3: camera_grid_ms reads 0 for such frames)
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
