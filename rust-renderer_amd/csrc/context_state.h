// context_state.h - struct uh_ctx and the types it is made of, for the files that implement the context: context.hip (lifetime,
// read-backs, stats), frame_loop.hip (the path tracer's frames), options.hip (uh_set_option), partition.hip (the tile and band partitions of a multi-GPU frame, the
// tile composition), rccl_link.hip (the RCCL link), scene_build.hip (meshes, builders, refit) and the graphs (raster_driver.hip,
// hybrid_graph.hip, hybrid_ray_passes.hip, hybrid_verbs.hip, post_graph.hip, forward_graph.hip, denoise_graph.hip; what they share: graphs_internal.h; what a
// uh_render_hybrid call reads of the context before it runs: hybrid_plan.h). Private: not installed, not part of
// the C ABI (include/utopian_hip.h), where uh_ctx stays opaque. The upkeep of the sun and camera grids is grid_cache.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "bvh.h"
#include "context_internal.h"
#include "device_types.h"
#include "grid_cache.h"
#include "utopian_hip.h"

using namespace uh;  // (the including files are written inside it)

// what uh_pose_mesh reads of a mesh (pose.hip), all on the device: the bind pose (the mesh's vertices when a set verb was last called),
// the skin's four joints and weights per vertex, the morph targets' deltas target-major, and the second vertex buffer a pose writes
// before it changes places with HostMesh::d_verts (made by the first pose)
struct MeshPose {
   UhVertex* bind = nullptr;
   UhVertex* back = nullptr;
   uint16_t* joints = nullptr;
   float* weights = nullptr;
   uint32_t num_joints = 0;   // 0: no skin
   float* dpos = nullptr;
   float* dnrm = nullptr;     // null: the targets carry no normal deltas
   uint32_t num_targets = 0;  // 0: no morph targets
   void release() {
      for (void* p : {(void*)bind, (void*)back, (void*)joints, (void*)weights, (void*)dpos, (void*)dnrm})
         if (p) (void)hipFree(p);
      *this = MeshPose{};
   }
};

struct HostMesh {
   std::vector<UhVertex> vertices;
   std::vector<uint32_t> indices;
   UhGpuMaterial material;
   float o2w[12];
   float w2o[9];
   // a mesh of uh_add_isosurface_mesh: what uh_update_isosurface_mesh re-extracts with
   bool iso = false, iso_reference = true;
   uint32_t iso_res = 0;
   float iso_lo = 0.0f, iso_hi = 0.0f;
   // device-resident (after uh_update_isosurface_mesh): d_verts holds 3 * dev_tris vertices, the index list is their iota.
   // vertices / indices above are then a mirror that exists only while host_valid (the host builder asks for it)
   bool dev = false, host_valid = true;
   UhVertex* d_verts = nullptr;
   size_t d_capacity = 0;        // vertices d_verts can hold
   uint32_t dev_tris = 0;
   uint64_t serial = 0;          // bumped by every update: what the build sources and the raster tables key this mesh's range on
   float olo[3] = {0, 0, 0}, ohi[3] = {0, 0, 0};  // object-space box of the device vertices (k_iso_scatter), for `box_serial`
   uint64_t box_serial = ~0ull;
   // indexed and device-resident (after uh_update_mesh_vertices): d_verts holds vertices.size() records and d_indices the index list,
   // uploaded by the first update. `indices` stays; `vertices` is stale while !host_valid (the last update took a device pointer)
   bool upd = false;
   uint32_t* d_indices = nullptr;
   // posed (uh_set_mesh_skin / uh_set_mesh_morph_targets; pose.hip): null until one of them is called, owned by the context
   struct MeshPose* pose = nullptr;
   bool resident() const { return dev || upd; }
   size_t tris() const { return dev ? dev_tris : indices.size() / 3; }
   size_t num_vertices() const { return dev ? 3 * (size_t)dev_tris : vertices.size(); }
   size_t num_indices() const { return dev ? 3 * (size_t)dev_tris : indices.size(); }
};

struct EventPair {
   hipEvent_t start, stop;
   int kind;  // 0 trace_closest, 1 trace_shadow, 2 shade
};

template <typename T>
struct DevBuf {
   T* p = nullptr;
   void* base = nullptr;
   size_t n = 0;
   // stagger_bytes shifts the array inside its allocation: the per-pixel SoA arrays are all the same
   // size, and kernels touch the same index of several of them at once; without a stagger those
   // accesses are an exact multiple of the array size apart
   hipError_t alloc(size_t count, size_t stagger_bytes = 0) {
      release();
      n = count;
      if (count == 0) return hipSuccess;
      hipError_t e = hipMalloc(&base, count * sizeof(T) + stagger_bytes);
      if (e == hipSuccess) p = reinterpret_cast<T*>(static_cast<char*>(base) + stagger_bytes);
      return e;
   }
   void release() {
      if (base) (void)hipFree(base);
      p = nullptr;
      base = nullptr;
      n = 0;
   }
   // a hipMalloc'ed array of `count` elements changes owner: what this buffer held is freed, `ptr` is cleared
   void take(T*& ptr, size_t count) {
      release();
      p = ptr, base = ptr, n = count;
      ptr = nullptr;
   }
};
// for a group's visitor (f(buffer, length)): frees every buffer it names (hidden, like every destroy() below: the library's dynamic
// symbols stay the C ABI's)
struct __attribute__((visibility("hidden"))) ReleaseBuf {
   template <class Buf> void operator()(Buf& b, size_t) const { b.release(); }
};

// the on-device build's per-triangle sources in mesh order: 9 floats of object-space corners, the key mesh << 22 | primitive and a
// ShadePacket (4 float4: normals and uvs of the three vertices, the mesh index) per triangle
struct __attribute__((visibility("hidden"))) BuildSources {
   DevBuf<float> corners;
   DevBuf<uint32_t> keys;
   DevBuf<float4> shade;
   struct View { const float* corners; const uint32_t* keys; const float4* shade; };
   View view() const { return View{corners.p, keys.p, shade.p}; }
   hipError_t alloc(size_t total) {
      hipError_t e;
      if ((e = corners.alloc(9 * total)) != hipSuccess || (e = keys.alloc(total)) != hipSuccess) return e;
      return shade.alloc(4 * total);
   }
   void release() { corners.release(), keys.release(), shade.release(); }
   void swap(BuildSources& o) { std::swap(corners, o.corners), std::swap(keys, o.keys), std::swap(shade, o.shade); }
   // triangles [src_first, src_first + n) of src to [dst_first, dst_first + n) of these arrays, if any: enqueued on `stream`, or,
   // without one, three blocking copies
   hipError_t copy_range(size_t dst_first, const View& src, size_t src_first, size_t n, hipMemcpyKind kind, hipStream_t stream) {
      const auto copy = [&](void* dst, const void* from, size_t bytes) { return stream ? hipMemcpyAsync(dst, from, bytes, kind, stream) : hipMemcpy(dst, from, bytes, kind); };
      if (!n) return hipSuccess;
      hipError_t e;
      if ((e = copy(corners.p + 9 * dst_first, src.corners + 9 * src_first, 9 * n * sizeof(float))) != hipSuccess ||
          (e = copy(keys.p + dst_first, src.keys + src_first, n * sizeof(uint32_t))) != hipSuccess)
         return e;
      return copy(shade.p + 4 * dst_first, src.shade + 4 * src_first, 4 * n * sizeof(float4));
   }
};

// a rasteriser's binning buffers (raster_driver.hip bin_and_resolve): the shadow maps, the marching-cubes pass, the rasterised
// G-buffer and the forward pass have a set each; they grow with what is drawn
struct RasterBins {
   DevBuf<uint32_t> tile_count, tile_cursor, rec_count, tri_mesh, chunks, entries;
   DevBuf<unsigned long long> totals;       // the grand totals of the two scans: records, tile entries
   DevBuf<uint4> records;
   DevBuf<float> mats;                      // per mesh (shadow maps: per cascade and mesh) what the pass's vertex stage multiplies by
   std::vector<float> mats_host;
   uint64_t geom = 0;                       // geom_version of tri_mesh / rec_count
   template <class F> void each(F&& f) {
      f(tile_count, 0), f(tile_cursor, 0), f(rec_count, 0), f(tri_mesh, 0), f(chunks, 0), f(entries, 0), f(totals, 0), f(records, 0), f(mats, 0);
   }
};

// what a perspective rasteriser resolves into, n pixels: depth, draw index and surviving record per pixel; covered[0] the covered
// pixels of the last pass. covered is allocated last: its pointer says "allocated"
struct RasterTarget {
   DevBuf<float> depth;
   DevBuf<uint32_t> vis, rec_of, covered;
   template <class F> void each(size_t n, F&& f) { f(depth, n), f(vis, n), f(rec_of, n), f(covered, 1); }
};

// one timed stage of a graph, between its two events (graphs_internal.h timed). ms: the elapsed time, resolved from the events by the
// first stats read after the stage ran and kept (a later read returns the same bits)
struct Stage {
   hipEvent_t begin = nullptr, end = nullptr;
   bool ran = false, timed = false;
   float ms = 0.0f;
   void destroy() {
      for (hipEvent_t ev : {begin, end})
         if (ev) (void)hipEventDestroy(ev);
   }
};

// the hybrid graph's stages (uh_ctx::Hybrid::stage): its seven passes in the order of their UH_HYBRID_* bits, then the environment's,
// then the shadow maps, then the marching-cubes pass, then the reservoir lights, then ray-traced ambient occlusion (classify + trace, resolve)
enum HybridStage : int {
   kStShadows, kStGbuffer, kStReflections, kStSsao, kStDeferred, kStSky, kStPresent, kHybridPasses,
   kStEnvCube = kHybridPasses, kStEnvIrradiance, kStEnvSpecular, kStEnvLut, kStShadowMaps, kStMarchingCubes, kStRestirLights,
   kStRtaoTrace, kStRtaoFilter, kHybridStages
};

// One frame in flight: its own stream pair, hazard events, path state and queue control block.
// Frames of the path-tracing pass are independent except for the order of the accumulation
// read-modify-write (reference.rgen:131-143), so up to `frames_in_flight` of them overlap on the
// GPU: one frame's memory-bound shading and kernel tails are filled by another frame's traversal,
// and a rank that owns only 1/N of the pixels still keeps the chip busy.
constexpr uint32_t kMaxSlots = 8;
struct Slot {
   hipStream_t stream = nullptr;
   // second stream: shade_miss (pure VALU, touches only paths that left the scene) and the shadow
   // traversals overlap the main stream's shade_hit / next closest-hit traversal
   hipStream_t side = nullptr;
   hipEvent_t ev_shaded = nullptr, ev_shadowed = nullptr, ev_side_done = nullptr;
   hipEvent_t ev_acc = nullptr;  // recorded after the frame's accumulate / store tail
   hipEvent_t frame_start = nullptr, frame_stop = nullptr;
   DevBuf<float4> rec, radf, pixcol;  // rec: two sets of four path-state planes + the hit plane (device_types.h PathState)
   DevBuf<uint32_t> queues[5];
   DevBuf<unsigned long long> sun_lit;  // the sun rays' verdicts: one bit per queue position (PathState::sun_lit)
   DevBuf<Control> control;
   PathState ps{};
   bool ready = false;
   size_t capacity = 0;  // path ids this slot can hold (pixels x frames per batch)

   hipError_t create(size_t n) {
      capacity = n;
      const uint32_t shard_cap = layout_shard_cap(n);  // exact: the largest number of 64-path runs one shard receives (shard_of_run)
      if (shard_cap >= (1u << 31)) return hipErrorInvalidValue;  // a queue position's top bit carries the path's sun verdict (path_shading.h kSunLitBit)
      hipError_t e;
#define SLOT_TRY(expr)                 \
   if ((e = (expr)) != hipSuccess) return e
      SLOT_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
      SLOT_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
      for (hipEvent_t* ev : {&ev_shaded, &ev_shadowed, &ev_side_done, &ev_acc}) SLOT_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
      SLOT_TRY(hipEventCreate(&frame_start));
      SLOT_TRY(hipEventCreate(&frame_stop));
      const size_t stagger = kPlaneStaggerBytes;  // 4 KiB + 256 B per array slot
      // planes staggered like the arrays: the same index of two planes must not alias. The hit plane is indexed by queue position
      // (shard segment + position in the shard's queue), which runs to kShards * shard_cap >= n
      const size_t plane = layout_plane_quads(n, shard_cap);
      SLOT_TRY(rec.alloc(plane * (2 * kRecQuads + 1), 0 * stagger));
      SLOT_TRY(radf.alloc(n, 1 * stagger));
      SLOT_TRY(pixcol.alloc(n, 2 * stagger));
      // sharded queues: capacity per shard = the pixels (64-pixel runs) a shard can own
      // (the miss queue holds (position, id) pairs: twice the words)
      for (int qi = 0; qi < 5; qi++) SLOT_TRY(queues[qi].alloc((size_t)shard_cap * kShards * (qi == 4 ? 2 : 1)));
      // shard_cap is a multiple of 64: a shard's segment is whole words. The sun kernels store every word the next kernels read
      SLOT_TRY(sun_lit.alloc((size_t)shard_cap * kShards / 64));
      SLOT_TRY(hipMemsetAsync(sun_lit.p, 0, sun_lit.n * sizeof(unsigned long long), stream));
      SLOT_TRY(control.alloc(1));
      SLOT_TRY(hipMemsetAsync(control.p, 0, sizeof(Control), stream));
      SLOT_TRY(hipStreamSynchronize(stream));
#undef SLOT_TRY
      ps.set[0] = PathRecs{rec.p, plane};
      ps.set[1] = PathRecs{rec.p + plane * kRecQuads, plane};
      ps.hit = rec.p + plane * 2 * kRecQuads;
      ps.radf = radf.p;
      ps.pixcol = pixcol.p;
      for (int i = 0; i < 5; i++) ps.queue[i] = queues[i].p;
      ps.sun_lit = sun_lit.p;
      ps.shard_cap = shard_cap;
      ready = true;
      return hipSuccess;
   }
   void destroy() {
      if (stream) (void)hipStreamSynchronize(stream);
      if (side) (void)hipStreamSynchronize(side);
      rec.release();
      radf.release();
      pixcol.release();
      for (auto& q : queues) q.release();
      sun_lit.release();
      control.release();
      for (hipEvent_t* ev : {&ev_shaded, &ev_shadowed, &ev_side_done, &ev_acc, &frame_start, &frame_stop}) {
         if (*ev) (void)hipEventDestroy(*ev);
         *ev = nullptr;  // (a create() that fails half-way must not leave handles for the next destroy())
      }
      if (side) (void)hipStreamDestroy(side);
      if (stream) (void)hipStreamDestroy(stream);
      stream = side = nullptr;
      ready = false;
   }
};

// A visibility grid the context keeps (sun_grid.h): the sun grid of one (geometry, direction), the camera grid of one (geometry,
// camera). `cache` says which pair that is and when another one is built (grid_cache.h); the rest is the last build's outcome.
template <int N>
struct __attribute__((visibility("hidden"))) CachedGrid {
   GridCache<N> cache;
   bool valid = false;              // d_cells / d_entries / dev hold a usable grid for (cache.geom, cache.key); false: refused, see why
   bool this_frame = false;         // the frame call being enqueued uses it (set by ensure_*_grid, read by the stats)
   DevBuf<uint32_t> d_cells;
   DevBuf<SunGridEntry> d_entries;
   SunGridDev dev{};
   SunGridLimits limits;
   std::string why;
   float build_ms = 0.0f, mean_list = 0.0f;
   uint32_t cells = 0, entries = 0, max_list_interior = 0;  // cells: as the stats report them

   bool holds(uint64_t geom, const float* key) const { return valid && cache.matches(geom, key); }
   size_t bytes() const { return d_cells.n * sizeof(uint32_t) + d_entries.n * sizeof(SunGridEntry); }
   void release() { d_cells.release(), d_entries.release(); }
   // a builder's result, or its refusal (!ok), becomes the grid for (geom, key): its two allocations change owner, the old ones are
   // freed - the caller has waited for the frames that may read them. cell_words: words per cell record. (grid_cache.hip)
   void adopt(SunGridDevice& g, bool ok, uint64_t geom, const float* key, uint32_t cell_words);
};

// what only the sun grid has: its lists a second time as 64-byte records that carry their packet (SunGridDev::recs), the coarse
// cover (SunGridDev::coarse), both made by attach_sun_inline_records behind every adoption, and the options of its build and use
struct SunGridExtras {
   DevBuf<float4> d_recs;
   DevBuf<float> d_coarse;
   uint32_t coarse_shift = 2;       // option "sun_grid_coarse": blocks of 4 x 4 cells; 0: no coarse cover
   // the records only while they stay within four times the packet array (a grid of 96 entries per triangle repeats every packet 96
   // times: 1.4 GB for the 17 MB of the config-1 scene); option "sun_grid_inline_max_mb" raises the budget (0: never)
   int64_t inline_max_mb = -1;      // -1: auto = 4 x the packet array
   bool device_build = true;        // option "sun_grid_build": 1 = on the device (sun_grid_build.hip: a few ms), 0 = the host builder (sun_grid.cpp)
   bool verdicts = true;            // option "sun_verdicts" (FrameParams::sun_verdicts)
   size_t bytes() const { return d_recs.n * sizeof(float4) + d_coarse.n * sizeof(float); }
   void release() { d_recs.release(), d_coarse.release(); }
};

// the ring of spatial buffers that lets the next batch's reservoir chains (at most kRestirBatch frames, frame_plan.h) run beside
// the current wavefront (two batches + the history slot)
constexpr int kSpatialRing = 2 * (int)kRestirBatch + 1;

struct RcclLink;  // rccl_link.hip

struct uh_ctx {
   int device = 0;
   Slot slots[kMaxSlots];
   uint32_t frames_in_flight = 4;     // slots used round-robin by path-tracing frames (swept: profiles/README.md)
   uint32_t batch_frames = 0;         // frames one uh_render_frames launch chain carries (option "batch_frames"); 0 = auto
   uint32_t next_slot = 0;
   hipEvent_t last_acc = nullptr;     // ev_acc of the most recent frame (accumulation order)
   // G-buffer cast + reservoir passes run in call order on their own stream, beside path-tracing frames in flight.
   // spatial_reuse_reservoirs is a RING of kSpatialRing buffers: the path tracer of frame f reads slot `spatial_cur` while
   // frame f+1's passes already run - its temporal pass reads the same slot and its spatial pass writes the next one, after
   // the last path-tracing wavefront that read THAT one has finished (spatial_reader[]). A batch of B static-camera frames
   // runs its B reservoir chains back to back (slots cur+1 .. cur+B) and then ONE path-tracing wavefront in which the
   // paths of frame f sample from slot cur+1+f (FrameParams::spatial_of): the ring holds two batches and the history.
   hipStream_t restir_stream = nullptr;
   hipEvent_t ev_restir = nullptr, rs_start = nullptr, rs_stop = nullptr;
   bool restir_recorded = false;
   int spatial_cur = 0;
   hipEvent_t spatial_reader[kSpatialRing] = {};
   // the reservoir passes by bands of rows over the ranks of a job (uh_set_restir_partition, partition.hip):
   // this rank's band, what hands the other ranks' bands over behind each spatial pass, and the RCCL link when that is what does
   // (uh_rccl_attach, rccl_link.hip)
   struct __attribute__((visibility("hidden"))) Bands {
      uint32_t rank = 0, world = 1, rows = 0;  // rows per band (the frame's height without a partition)
      UhRestirExchangeFn exchange = nullptr;
      void* user = nullptr;
      RcclLink* link = nullptr;
      void destroy();  // the link and its exchange go (rccl_link.hip); the caller has drained the streams its collectives run on
   } bands;
   size_t res_stride = 0;  // reservoirs per spatial_reuse buffer: the frame, padded to bands.world equal bands
   hipEvent_t ev_band[kSpatialRing] = {};  // "this context's band of ring slot k is written" (in-process groups pull on it)
   hipEvent_t t_start = nullptr, t_stop = nullptr;  // bracket of the last uh_render_frame call (last_frame_ms)
   hipStream_t& stream = slots[0].stream;  // slot 0 also serves every non-frame operation
   bool overlap_miss = true, overlap_shadow = true;
   uint32_t W = 0, H = 0;
   uint32_t num_cus = 256;
   // persistent grids of the traversal kernels, blocks per CU (the refill kernels' LDS - stacks + ray pool - admits 6 / 5). Round 4,
   // closest / shadow = 6/5, 5/5, 5/4, 4/4, 4/3, 3/4: a 16-frame wavefront 1.774 / 1.777 / 1.764 / 1.780 / 1.773 / 1.799 ms per frame,
   // one frame per call with a wait after it 2.95 / 2.88 / 2.88 / 2.84 / 2.85 / 2.89 ms: fewer waves finish a small launch's tail sooner
   uint32_t closest_blocks_per_cu = 5, shadow_blocks_per_cu = 5;  // (config 2, whose light shadow rays are a third of the frame: 6/5, 5/5, 5/4, 6/4 = 8,230 / 8,266 / 7,997 / 7,950 Mrays/s)
   uint32_t cam_walk_whole = 512;     // option "camera_grid_walk_whole" (sun_grid.h SunGridDev::walk_whole)
   // one frame per call: bounces 1 .. of a lone frame inside one persistent kernel (k_path_fused) instead of four launches per bounce
   // (when: frame_plan.h plan_sample, with kFusedMaxPaths and the lone frame's kSingleFrameBlocksPerCu)
   bool fused_bounces = true;  // option "fused_bounces"
   bool fused_always = false;  // fused_bounces = -1: also with frames in flight and for frames of any size (tests)
   uint32_t fused_blocks_per_cu = 4;
   bool texture_blocks = true;  // option "texture_blocks": how uh_add_texture_rgba8 lays the next textures out
   std::string err;

   // host scene
   std::vector<HostMesh> meshes;
   std::vector<UhGpuLight> lights;
   struct HostTex {
      uint32_t w, h;
      uchar4* dev;
      uint32_t tiles_x;   // 8x8 tiles per row; 0 = not tiled
      uint32_t blocks_x;  // overlapped blocks per row (texture_layout.h); 0 = not blocked: tiles, or rows when tiles_x is 0 too
   };
   std::vector<HostTex> textures;
   bool built = false;

   // device scene
   DevBuf<float4> d_nodes, d_tris, d_shade, d_lights;
   DevBuf<MeshShade> d_meshes;
   // on-device refit (refit.hip), allocated by the first uh_refit_acceleration
   DevBuf<float> d_obj_corners, d_world_corners, d_node_box;
   DevBuf<RefitMesh> d_refit_meshes;
   std::vector<uint32_t> packet_keys;  // key of triangle packet i (leaf order)
   std::vector<uint32_t> level_start;  // BFS levels of the node array
   bool topology_valid = false;        // the device tree matches the mesh list (transforms may differ)
   // on-device build (lbvh.hip, option "device_build"): per-triangle sources in mesh order, kept on the device
   // until a mesh is added, so that a rebuild after moved instances or changed parameters uploads nothing
   bool device_build = false, src_valid = false;
   uint32_t device_build_kind = 1;  // 1 = PLOC, 2 = radix tree (lbvh.hip)
   // PLOC rounds stop at this many clusters; a host SAH tree over them is the top (option "ploc_sah_top", 0 = PLOC to the root).
   // Config-1 scene: 0 / 1,024 / 8,192 / 131,072 clusters = 21.7 / 20.3 / 20.1 / 19.0 nodes per ray, rebuild 7.7 / 6.0 / 9.4 / 66 ms (host tree: 18.8)
   uint32_t ploc_sah_top = 1024;
   static constexpr uint32_t kPlocRadius = 8;  // swept 4..64 in round 3: tree quality flat (21.7-23.0 nodes/ray), build time grows with it (profiles/README.md)
   BuildSources d_src;
   // the layout of d_src: triangles and HostMesh::serial of each mesh's range (a mesh whose serial moved is rewritten from its
   // device vertices, the ranges behind it are moved on the device)
   std::vector<uint32_t> src_tris;
   std::vector<uint64_t> src_serial;
   // uh_update_isosurface_mesh: extraction scratch, the box words of k_iso_scatter, two events and the figures of
   // uh_get_isosurface_update_stats; nothing of it exists before the first update
   struct IsoUpdate {
      DevBuf<uint32_t> counts, chunks, box;
      DevBuf<unsigned long long> total;
      hipEvent_t begin = nullptr, end = nullptr;
      UhIsosurfaceUpdateStats st{};
   } iso;
   // uh_update_mesh_vertices: HostMesh::serial of every mesh when the tree's packets (d_obj_corners, d_shade) were last written - by
   // a build or by k_deform_gather -, that kernel's per-mesh table, the device pass's flag word, the events around the gather and
   // around the refit behind it, and the figures of uh_get_mesh_update_stats; nothing but packet_serial exists before the first update
   std::vector<uint64_t> packet_serial;
   struct MeshUpdate {
      DevBuf<DeformMesh> table;
      DevBuf<uint32_t> flag;
      hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // before the gather, between it and the refit, behind the refit
      UhMeshUpdateStats st{};
   } mupd;
   // uh_pose_mesh (pose.hip): a call's joint matrices and active targets on the device (and the host vector they are copied from), the
   // flag word of the finite-position check, the events around the kernel and the figures of uh_get_pose_stats; nothing of it exists
   // before the first pose
   struct Pose {
      DevBuf<float> params;
      std::vector<float> host_params;
      DevBuf<uint32_t> flag;
      hipEvent_t ev[2] = {nullptr, nullptr};
      UhPoseStats st{};
   } pose;
   float refit_ms = 0.0f;
   DevBuf<TexInfo> d_tex;
   DevBuf<float> d_lut;
   SceneDev scene{};

   // frame-persistent per-pixel images (graph resources of renderers/mod.rs:199-244)
   DevBuf<float4> accumulation, gbuffer;
   DevBuf<uchar4> output;
   DevBuf<UhReservoir> reservoirs[3], spatial_ring;  // ring slot 0 = reservoirs[2], slots 1.. = spatial_ring (allocated by the first reservoir pass)
   DevBuf<float4> gb_ray_o, gb_ray_d, gb_hit;  // scratch of the G-buffer cast (allocated by the first G-buffer pass)
   DevBuf<DeviceStats> dstats;
   Images im{};

   // options / stats
   bool count_visits = false, time_kernels = false, full_frame_restir = false;
   bool iso_reference = true;  // option "iso_reference_triangulation": uh_add_isosurface_mesh emits the reference's triangles (isosurface.hip)
   uint32_t shadow_map_size = 4096;  // option "shadow_map_size": the cascaded shadow maps' size (shadow.rs: 4096)
   bool furnace = false;  // option "furnace": reference.rmiss compiled with FURNACE_TEST (a miss returns white whatever view.sky_enabled says)
   uint64_t frames = 0;
   float build_ms = 0.0f, last_frame_ms = 0.0f;
   float ms_by_kind[5] = {0, 0, 0, 0, 0};  // trace_closest, sun shadow rays (grid + tree), shade, camera grid (bounce 0 through the grid + its leftovers), light shadow rays
   uint32_t trace_closest_launches = 0, trace_light_launches = 0;
   bool frame_timed = false;
   std::vector<EventPair> pending, free_events;
   uint32_t bvh_nodes = 0, bvh_tris = 0;

   // sun shadow rays through a per-direction grid instead of the tree (sun_grid.h; option "sun_grid"), built on the first frame that
   // traces sun rays and again once a new direction or geometry has stayed put for two frames (grid_cache.h; grid_cache.hip ensure_sun_grid)
   bool sun_grid_enabled = true;
   uint64_t geom_version = 1;
   CachedGrid<3> sun;               // key: the frame's sun direction
   SunGridExtras sun_x;
   bool primary_implicit = true;    // option "primary_implicit" (FrameParams::primary_implicit)
   bool slim_state = true;          // option "slim_state" (FrameParams::slim_state)
   bool fused_primary = true;       // option "fused_primary" (frame_plan.h SamplePlan::fused_primary)

   // the primary rays through a per-camera grid instead of the tree (sun_grid.h "camera grid"; option "camera_grid"), built once the same
   // camera has been asked for in two consecutive frame calls, or at once by a call that carries 8 frames of it (grid_cache.hip ensure_camera_grid)
   bool cam_grid_enabled = true;
   CachedGrid<32> cam;              // key: inverse_view, inverse_projection

   // the tile partition of the path-traced frame (uh_set_tile_partition, partition.hip; the owner rule: tile_partition.h), and its
   // composition without a host wait (uh_rccl_gather_tiles; the in-process group's uh_mgpu_compose): this rank's packed tiles, on the
   // root every rank's, and the event behind the last pack / composition - the next frame's accumulate tail waits for it like for a
   // frame's (last_acc)
   struct __attribute__((visibility("hidden"))) Tiles {
      uint32_t rank = 0, world = 1, tile = 64;
      DevBuf<uint32_t> owned_pixels;  // ascending pixel ids this rank owns (empty = the whole frame)
      uint32_t n_owned = 0;
      DevBuf<float4> send, recv;
      hipEvent_t ev_compose = nullptr;
      void destroy() {
         owned_pixels.release(), send.release(), recv.release();
         if (ev_compose) (void)hipEventDestroy(ev_compose);
      }
   } tiles;

   // the hybrid graph's passes (uh_render_hybrid): images, the metal-pixel queue and a copy of the scene's meshes as gbuffer.vert
   // reads them, all allocated by the first call. Every feature below names its buffers once, in a visitor f(buffer, length) over
   // n pixels that serves its first-use allocation and its destroy(): a group's last buffer is allocated last, its pointer says
   // "allocated"; length 0: grown by the pass. A feature with timed stages of its own names them likewise, in a visitor stages(f) that
   // serves their creation (graphs_internal.h first_use), the reset of their records and destroy()
   struct Hybrid {
      DevBuf<float4> pos, nrm, pbr;
      DevBuf<uchar4> alb, refl;
      DevBuf<uint8_t> shadow;
      DevBuf<uint32_t> queue, counter;
      DevBuf<HybridMesh> meshes;
      DevBuf<UhVertex> vertices;
      DevBuf<uint32_t> indices;
      uint64_t geom = 0;                       // geom_version the mesh tables were made for
      // with device-resident meshes: each mesh's range in vertices / indices and the HostMesh::serial it holds (unchanged ranges
      // are moved on the device instead of uploaded again)
      struct Range { uint32_t vb, ib, nv, ni; uint64_t serial; };
      std::vector<Range> layout;
      hipEvent_t waits[2 * kMaxSlots + 1] = {};  // behind the frames in flight
      // one record per stage: stage k < kHybridPasses is bit k of UH_HYBRID_* (rt_shadows, G-buffer, rt_reflections, SSAO, deferred,
      // sky, present: the last call's), the environment's sub-passes follow (cube, irradiance, specular, BRDF LUT: the last build's)
      Stage stage[kHybridStages];
      // the final frame's passes (SSAO, deferred, sky, present), allocated by the first call that asks for one of them
      DevBuf<uint16_t> ssao;
      DevBuf<float4> deferred;
      DevBuf<uchar4> present;
      DevBuf<uint32_t> sky_counter;
      DevBuf<UhGpuLight> raw_lights;           // the uh_add_light table as added
      DevBuf<HybridLight> lights;              // its records as the deferred pass reads them, the sun first
      size_t lights_uploaded = SIZE_MAX;       // c->lights.size() when raw_lights was uploaded
      uint32_t frame_lights = 0;               // lights the deferred pass of the last call evaluated (the sun included)
      bool gbuffer_done = false;               // a G-buffer pass has been enqueued (the marching-cubes pass's depth seed reads it)
      bool gbuffer_rasterised = false;         // the last G-buffer pass enqueued was rasterised: its depth is the marching-cubes seed
      template <class F> void rt_images(size_t n, F&& f) {
         f(pos, n), f(nrm, n), f(pbr, n), f(alb, n), f(refl, n), f(shadow, n), f(queue, n), f(counter, 1);
      }
      template <class F> void frame_images(size_t n, F&& f) {
         f(ssao, n), f(deferred, n), f(present, n), f(lights, UH_MAX_GPU_LIGHTS + 1), f(sky_counter, 1);
      }

      // the IBL maps of setup_cubemap_pass (UH_HYBRID_ENVIRONMENT), allocated by the first call that builds them
      struct __attribute__((visibility("hidden"))) Environment {
         DevBuf<float4> cube, irr, spec;
         DevBuf<uint32_t> lut;
         DevBuf<float4> taps;                  // the irradiance filter's tap table (uploaded before the maps are allocated)
         uint32_t builds = 0;
         float sun[3] = {0, 0, 0}, eye[3] = {0, 0, 0};  // what the last build was made with
         template <class F> void images(F&& f) {
            const size_t mips = env_mip_offset(kEnvMips);
            f(cube, mips), f(irr, 6 * (size_t)kEnvSize * kEnvSize), f(spec, mips), f(lut, (size_t)kLutSize * kLutSize);
         }
         void destroy() { images(ReleaseBuf{}), taps.release(); }
      } env;

      // the cascaded shadow maps (UH_HYBRID_SHADOW_MAPS), all grown by the first call that renders them; freed by a size change
      struct __attribute__((visibility("hidden"))) ShadowMaps {
         DevBuf<float> maps;                   // 4 layers of size^2
         DevBuf<UhShadowmapParams> dev_params; // the snapshot the deferred pass reads
         RasterBins bins;                      // rec_count: [cascade][triangle]; mats: [cascade][mesh][16]
         bool params_set = false;
         UhShadowmapParams params{}, snapshot{}, pending{};  // the last uh_set_shadowmap_params; what the maps were rendered with;
                                                             // what the render in progress uses
         uint32_t renders = 0, size = 0, tris[4] = {0, 0, 0, 0};
         template <class F> void images(F&& f) { f(maps, 0), f(dev_params, 0), bins.each(f); }
         void destroy() { images(ReleaseBuf{}); }
      } sm;

      // the rasterised G-buffer (UH_HYBRID_GBUFFER_RASTER), allocated by the first rasterised pass: its depth buffer, visibility,
      // surviving records and binning buffers ([mesh][28] matrices)
      struct __attribute__((visibility("hidden"))) GbufferRaster {
         RasterTarget target;
         RasterBins bins;
         uint32_t renders = 0, pieces = 0;
         template <class F> void images(size_t n, F&& f) { target.each(n, f); }  // (bins: grown by the pass)
         void destroy() { images(0, ReleaseBuf{}), bins.each(ReleaseBuf{}); }
      } gr;

      // the marching-cubes pass (UH_HYBRID_MARCHING_CUBES), allocated by the first pass: its depth buffer, visibility, surviving
      // records, light records, extracted triangles and binning buffers, whose chunks also serve the extraction's scan and whose
      // matrices are (P V) I column-major, the identity 3x4, then P V (44 floats)
      struct __attribute__((visibility("hidden"))) MarchingCubes {
         RasterTarget target;
         RasterBins bins;
         DevBuf<HybridLight> lights;
         DevBuf<UhVertex> verts;               // 3 per triangle, extraction order
         DevBuf<uint32_t> block_counts;
         DevBuf<unsigned long long> total;     // the extraction scan's grand total: triangles
         DevBuf<HybridMesh> mesh;              // mesh_index 0's maps with world = identity
         uint32_t renders = 0, tris = 0, pieces = 0, lights_used = 0;
         float time = 0.0f;
         template <class F> void images(size_t n, F&& f) {
            f(lights, UH_MAX_GPU_LIGHTS + 1), f(block_counts, kMcBlocks), f(bins.mats, 44), f(mesh, 1), f(total, 1), f(bins.totals, 2), f(verts, 0);
            target.each(n, f);  // (verts and the rest of bins are grown by the pass)
         }
         void destroy() { images(0, ReleaseBuf{}), bins.each(ReleaseBuf{}); }
      } mc;

      // the reservoir lights (UH_HYBRID_RESTIR_LIGHTS), allocated by the first call with the bit: the light-visibility image, the queue
      // of the pixels that cast a ray and the pass's counters (rays, occluded); read: behind the call's last read of the reservoirs
      struct __attribute__((visibility("hidden"))) RestirLights {
         DevBuf<uint8_t> vis;
         DevBuf<uint32_t> queue, counters;
         hipEvent_t read = nullptr;
         uint32_t renders = 0;
         template <class F> void images(size_t n, F&& f) { f(vis, n), f(queue, n), f(counters, 2); }
         void destroy() {
            images(0, ReleaseBuf{});
            if (read) (void)hipEventDestroy(read);
         }
      } rl;

      // ray-traced ambient occlusion (UH_HYBRID_RTAO), allocated by the first pass: the occluded-ray counts (a byte per pixel, rounded
      // up to whole words: the trace kernel adds into them by words), the queue of the pixels that cast and the pass's counters
      // (pixels, occluded, and with option "count_visits" the walks' node visits and triangle tests); params: the last
      // uh_set_rtao_params (the defaults before); samples: the last pass's
      struct __attribute__((visibility("hidden"))) Rtao {
         DevBuf<uint8_t> counts;
         DevBuf<uint32_t> queue, counters;
         UhRtaoParams params{4, 1.0f, 1.0f, 2, 0.9f, 0.05f};
         uint32_t renders = 0, samples = 0;
         uint32_t order = 0;                   // option "rtao_order" (rtao.hip: how the trace kernel's work items are laid out; 0 measured fastest)
         template <class F> void images(size_t n, F&& f) { f(counts, (n + 3) & ~(size_t)3), f(queue, n), f(counters, 6); }
         void destroy() { images(0, ReleaseBuf{}); }
      } ao;

      // one-bounce ray-traced diffuse GI (UH_HYBRID_RTGI), allocated by the first pass: the count words, the radiance image, the
      // unfiltered means, the queue of the pixels that cast and the pass's counters (pixels, sun rays, misses); rays and sun_rays (a
      // record per ray each) are grown to the largest `samples` a pass has run with. params: the last uh_set_rtgi_params (the defaults
      // before); samples: the last pass's. stage: trace, shadow, filter, composite of the last pass.
      struct __attribute__((visibility("hidden"))) Rtgi {
         DevBuf<uint32_t> counts, queue, counters;
         DevBuf<float4> radiance, mean, rays, sun_rays;
         UhRtgiParams params{2, 3, 16.0f, 1.0f, 0.9f, 0.05f};
         Stage stage[4];
         uint32_t renders = 0, samples = 0;
         uint32_t order = 0;                   // option "rtgi_order" (rtgi.hip: how the trace kernel's work items are laid out)
         template <class F> void images(size_t n, F&& f) { f(counts, n), f(radiance, n), f(mean, n), f(queue, n), f(counters, 4); }
         template <class F> void stages(F&& f) {
            for (Stage& s : stage) f(s);
         }
         void destroy() {
            images(0, ReleaseBuf{});
            rays.release(), sun_rays.release();
            stages([](Stage& s) { s.destroy(); });
         }
      } gi;

      // ray-traced glossy reflections (UH_HYBRID_GLOSSY), allocated by the first pass: the count words, the two images, the unfiltered
      // sums, the radius bytes, the queue of the pixels that cast and the pass's counters (GlossyDev::counters); rays, orig, dirs, sun_rays
      // (a record per ray each) and ray_queue (a word per ray) are grown to the largest `samples` a pass has run with. params: the last
      // uh_set_glossy_params (the defaults before). stage: trace, shade, shadow, filter, composite of the last pass.
      struct __attribute__((visibility("hidden"))) Glossy {
         DevBuf<uint32_t> counts, queue, counters, ray_queue;
         DevBuf<uint8_t> re;
         DevBuf<float4> scale, bias, mean_s, mean_b, rays, orig, dirs, sun_rays;
         UhGlossyParams params{1, 3, 0.6f, 16.0f, 1.0f, 0.5f, 0.95f, 0.05f};
         Stage stage[5];
         uint32_t renders = 0;
         template <class F> void images(size_t n, F&& f) { f(counts, n), f(scale, n), f(bias, n), f(mean_s, n), f(mean_b, n), f(re, n), f(queue, n), f(counters, 8); }
         template <class F> void stages(F&& f) {
            for (Stage& s : stage) f(s);
         }
         void destroy() {
            images(0, ReleaseBuf{});
            rays.release(), orig.release(), dirs.release(), sun_rays.release(), ray_queue.release();
            stages([](Stage& s) { s.destroy(); });
         }
      } gl;

      // volumetric fog (UH_HYBRID_FOG), allocated by the first pass: the mask words, the terms image, the march lengths, the queue of
      // the pixels that march and the pass's counters (FogDev::counters). params: the last uh_set_fog_params (the defaults before);
      // steps: the last pass's. stage: trace, resolve, composite of the last pass.
      struct __attribute__((visibility("hidden"))) Fog {
         DevBuf<uint32_t> mask, queue, counters;
         DevBuf<float4> terms;
         DevBuf<float> dist;
         UhFogParams params{16, 2, 0.02f, 200.0f, 0.6f, 1.0f, 0.1f, 0, {1.0f, 1.0f, 1.0f}, {0.05f, 0.06f, 0.08f}};
         Stage stage[3];
         uint32_t renders = 0, steps = 0;
         uint32_t order = 2;                   // option "fog_order" (fog.hip: how the trace kernel's work items are laid out; 2 measured fastest)
         template <class F> void images(size_t n, F&& f) { f(mask, n), f(terms, n), f(dist, n), f(queue, n), f(counters, 6); }
         template <class F> void stages(F&& f) {
            for (Stage& s : stage) f(s);
         }
         void destroy() {
            images(0, ReleaseBuf{});
            stages([](Stage& s) { s.destroy(); });
         }
      } fog;

      // ray-traced glass (UH_HYBRID_GLASS), allocated by the first pass: per pixel the count words, the radiance image, the events words and
      // the queue of the pixels that cast; per ray (two a pixel) the hit / radiance record, origin, direction, sun-ray record and a word in
      // each of the two round queues; and the pass's counters (GlassDev::counters). params: the last uh_set_glass_params (the defaults
      // before). trace, bend: a stage per round of the last pass (its first `rounds`; the raygen is in trace[0]); then shadow, composite.
      struct __attribute__((visibility("hidden"))) Glass {
         DevBuf<uint32_t> counts, events, queue, counters, ray_queue[2];
         DevBuf<float4> radiance, rays, orig, dirs, sun_rays;
         UhGlassParams params{8, 16.0f, 1.0f};
         Stage trace[kGlassMaxEvents], bend[kGlassMaxEvents], shadow, composite;
         uint32_t renders = 0, rounds = 0;
         template <class F> void images(size_t n, F&& f) {
            f(counts, n), f(events, n), f(radiance, n), f(queue, n), f(rays, 2 * n), f(orig, 2 * n), f(dirs, 2 * n), f(sun_rays, 2 * n), f(ray_queue[0], 2 * n),
               f(ray_queue[1], 2 * n), f(counters, kGlassCounters);
         }
         template <class F> void stages(F&& f) {
            for (Stage& s : trace) f(s);
            for (Stage& s : bend) f(s);
            f(shadow), f(composite);
         }
         void destroy() {
            images(0, ReleaseBuf{});
            stages([](Stage& s) { s.destroy(); });
         }
      } glass;

      // emissive meshes as area lights (UH_HYBRID_AREA_LIGHTS), allocated by the first pass: per pixel the count words, the two images,
      // their unfiltered means and the queue of the pixels that cast; the pass's counters (AreaDev::counters) and the table's two scalars.
      // rec_d, rec_s (a record per sample each) and rays (two records per sample) are grown to the largest `samples` a pass has run with.
      // The emitter table (AreaTableDev) is grown to the scene's emitter triangles and filled again when geom != the context's
      // geom_version - a build or a refit has written the packets since; host_base: the per-mesh first slots as uploaded. params: the
      // last uh_set_area_light_params (the defaults before); samples: the last pass's. stage: classify + sample, shadow, filter,
      // composite of the last pass; table: the last table build.
      struct __attribute__((visibility("hidden"))) AreaLights {
         DevBuf<uint32_t> counts, queue, counters, amax;
         DevBuf<unsigned long long> total;
         DevBuf<float4> diffuse, specular, mean_d, mean_s, rec_d, rec_s, rays;
         DevBuf<float4> tri;
         DevBuf<uint32_t> keys, weights, cum, base, chunks;
         DevBuf<float> areas;
         std::vector<uint32_t> host_base;
         UhAreaLightParams params{2, 3, 1, 64.0f, 16.0f, 1.0f, 0.9f, 0.05f};
         Stage stage[4], table;
         uint64_t geom = 0;                    // geom_version the table was filled for (0: never)
         uint32_t emitters = 0, table_builds = 0, renders = 0, samples = 0;
         uint32_t order = 0;                   // option "area_light_order" (area_lights.hip: how the sample kernel's work items are laid out)
         template <class F> void images(size_t n, F&& f) {
            f(counts, n), f(diffuse, n), f(specular, n), f(mean_d, n), f(mean_s, n), f(queue, n), f(amax, 1), f(total, 1), f(counters, 4);
         }
         template <class F> void stages(F&& f) {
            for (Stage& s : stage) f(s);
            f(table);
         }
         void destroy() {
            images(0, ReleaseBuf{});
            rec_d.release(), rec_s.release(), rays.release(), tri.release(), keys.release(), weights.release(), cum.release(), base.release(),
               chunks.release(), areas.release();
            stages([](Stage& s) { s.destroy(); });
         }
      } area;

      // motion vectors (UH_HYBRID_MOTION), allocated by the first call with the bit: the motion image, the pass's counts (pixels with /
      // without a correspondence, a pair per block of the kernel's grid, added up by uh_get_motion_stats), the per-mesh table the
      // kernels read, and the previous-position table (16-byte rows with bases of their own: isosurface meshes, which are never
      // `deformed`, hold none). snap: the meshes as the last motion pass left them - the transform and HostMesh::serial then, and the
      // mesh's rows
      struct __attribute__((visibility("hidden"))) Motion {
         struct Snap { float o2w[12]; uint64_t serial; uint32_t base, count; };
         DevBuf<float4> image, prev;
         DevBuf<MotionMesh> table;
         DevBuf<uint32_t> counters;
         std::vector<Snap> snap;
         std::vector<MotionMesh> rows;         // table's host copy
         Stage stage[2];                       // the motion kernel, the snapshot behind it (the last pass's)
         uint32_t renders = 0, states[4] = {0, 0, 0, 0};  // meshes per MotionState at the last pass
         static constexpr uint32_t kMaxBlocks = 8 * 1024;  // the grid's cap (8 blocks per CU) for any device this runs on
         uint32_t blocks = 0;                  // blocks of the last pass's grid
         bool last = false;                    // the last G-buffer pass enqueued had the bit (uh_denoise with UH_DENOISE_MOTION asks)
         template <class F> void images(size_t n, F&& f) { f(prev, 0), f(table, 0), f(image, n), f(counters, 2 * (size_t)kMaxBlocks); }
         template <class F> void stages(F&& f) {
            for (Stage& s : stage) f(s);
         }
         void destroy() {
            images(0, ReleaseBuf{});
            stages([](Stage& s) { s.destroy(); });
         }
      } mv;

      // temporal anti-aliasing (UH_HYBRID_TAA), allocated by the first call with the bit: two sets of taa_output and the history length N,
      // ping-ponged - set `cur` is the one the last pass wrote (what uh_read_hybrid and present read), the other the one the next pass
      // writes - and the pass's counters (pixels that blended a history, pixels that started one: TaaDev's pairs); params: the last uh_set_taa_params
      // (the defaults before); valid: set `cur` is a history the next pass may read (false before the first pass and after
      // uh_reset_taa_history)
      struct __attribute__((visibility("hidden"))) Taa {
         DevBuf<float4> col[2];
         DevBuf<float> n[2];
         DevBuf<uint32_t> counters;
         UhTaaParams params{UH_TAA_CLAMP, 16, 0.1f, 1.0f};
         Stage stage;                          // the last pass's
         int cur = 0;
         bool valid = false;
         uint32_t renders = 0;
         template <class F> void images(size_t n_, F&& f) { f(col[0], n_), f(col[1], n_), f(n[0], n_), f(n[1], n_), f(counters, (size_t)kTaaCounterSlots * kTaaCounterStride); }
         template <class F> void stages(F&& f) { f(stage); }
         void destroy() {
            images(0, ReleaseBuf{});
            stages([](Stage& s) { s.destroy(); });
         }
      } taa;

      // the HDR display chain (UH_HYBRID_POST, uh_post_image), allocated by the first pass: post_output, the bloom pyramid (every level
      // of the frame that exists, up to kPostMaxLevels; the last level a pass builds has no `up` of its own - it is its `down`), the
      // histogram with the copy uh_read_post reads, and the exposure record, which stays on the device from pass to pass. input:
      // uh_post_image's upload (its first call). params: the last uh_set_post_params (the defaults before). have_exposure: the record
      // holds a previous pass's exposure (false before the first pass and after uh_reset_post_exposure); levels, metered: what the last
      // pass built. stage: meter, bloom, composite of the last pass.
      struct __attribute__((visibility("hidden"))) Post {
         DevBuf<float4> out, input;
         DevBuf<float4> down[kPostMaxLevels + 1], up[kPostMaxLevels + 1];  // [0] unused
         DevBuf<uint32_t> hist, hist_copy;
         DevBuf<PostRecord> rec;
         UhPostParams params{UH_POST_AUTO_EXPOSURE | UH_POST_BLOOM, UH_TONEMAP_ACES, 6, 1.0f, 0.18f, 0.015625f, 64.0f, 0.1f, 0.5f, 0.95f, 1.0f, 0.04f};
         Stage stage[3];
         bool have_exposure = false, metered = false;
         uint32_t levels = 0, renders = 0;
         template <class F> void images(uint32_t W, uint32_t H, F&& f) {
            f(out, (size_t)W * H);
            for (uint32_t k = 1; k <= kPostMaxLevels; k++) f(down[k], post_level_texels(W, H, k)), f(up[k], post_level_texels(W, H, k));
            f(hist, (size_t)kPostBins), f(hist_copy, (size_t)kPostBins), f(rec, (size_t)1);
         }
         template <class F> void stages(F&& f) {
            for (Stage& s : stage) f(s);
         }
         void destroy() {
            images(0, 0, ReleaseBuf{});
            input.release();
            stages([](Stage& s) { s.destroy(); });
         }
      } post;

      __attribute__((visibility("hidden"))) void destroy() {
         rt_images(0, ReleaseBuf{}), frame_images(0, ReleaseBuf{});
         env.destroy(), sm.destroy(), gr.destroy(), mc.destroy(), rl.destroy(), ao.destroy(), gi.destroy(), gl.destroy(), glass.destroy(), area.destroy(), fog.destroy(), mv.destroy(), taa.destroy(), post.destroy();
         meshes.release(), vertices.release(), indices.release(), raw_lights.release();
         for (hipEvent_t ev : waits)
            if (ev) (void)hipEventDestroy(ev);
         for (Stage& s : stage) s.destroy();
      }
   } hy;

   // the forward graph (uh_render_forward): its images, light records and binning buffers, allocated by the first call; it shares the
   // hybrid graph's mesh tables, uploaded light table and shadow maps
   struct Forward {
      DevBuf<float4> color;                    // forward_output RGBA32F
      RasterTarget target;
      DevBuf<uchar4> present;                  // the forward graph's present image, B8G8R8A8
      DevBuf<HybridLight> lights;              // forward.frag's light records, the sun first
      RasterBins bins;                         // [mesh][28] matrices
      Stage stage[3];                          // pass k: 0 shadow maps, 1 forward, 2 present (the last call's)
      uint32_t renders = 0, pieces = 0, lights_used = 0;
      template <class F> void images(size_t n, F&& f) { target.each(n, f), f(present, n), f(lights, UH_MAX_GPU_LIGHTS + 1), f(color, n); }
      __attribute__((visibility("hidden"))) void destroy() {
         images(0, ReleaseBuf{}), bins.each(ReleaseBuf{});
         for (Stage& s : stage) s.destroy();
      }
   } fw;

   // the denoiser (uh_denoise): two history sets (the previous call's, read, and this call's, written), the filter's two images and the
   // images uh_read_denoised copies out, all allocated by the first call; counters: geometry pixels, pixels that kept a history
   struct Denoise {
      DevBuf<float4> h_pos[2], h_nrm[2], h_col[2], cv[2], input, temporal, color;
      DevBuf<float2> h_mom[2];
      DevBuf<float> history, variance;
      DevBuf<uchar4> output;
      DevBuf<uint32_t> counters;
      Stage stage[4];                          // input + temporal, variance estimate, the a-trous levels, output (the last call's)
      hipEvent_t acc_read = nullptr;           // behind the call's read of the accumulation image (the next frame's tail waits for it)
      int cur = 0;                             // the set the next call writes
      bool have_history = false;
      uint32_t calls = 0;
      template <class F> void images(size_t n, F&& f) {
         for (int k = 0; k < 2; k++) f(h_pos[k], n), f(h_nrm[k], n), f(h_col[k], n), f(h_mom[k], n), f(cv[k], n);
         f(input, n), f(temporal, n), f(color, n), f(history, n), f(variance, n), f(output, n), f(counters, 2);
      }
      __attribute__((visibility("hidden"))) void destroy() {  // (uh_ctx::last_acc may still name acc_read: destroy_graphs clears it first)
         images(0, ReleaseBuf{});
         for (Stage& s : stage) s.destroy();
         if (acc_read) (void)hipEventDestroy(acc_read);
      }
   } dn;
};

// ---- context.hip, for the other files of the context (not exported: the library's dynamic symbols stay the C ABI's) ----
#pragma GCC visibility push(hidden)
int fail(uh_ctx* c, int code, const std::string& msg);  // sets uh_last_error (c null: uh_create's); returns code
#define HIP_TRY(ctx, expr)                                                                                   \
   do {                                                                                                      \
      hipError_t e_ = (expr);                                                                                \
      if (e_ != hipSuccess) return fail(ctx, e_ == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, \
                                        std::string(#expr) + ": " + hipGetErrorString(e_));                 \
   } while (0)
LaunchCfg cfg(uh_ctx* c);
// option "time_kernels": the launches between the two are timed as `kind` (EventPair::kind) on `stream` (null: the context's)
void begin_timed(uh_ctx* c, int kind, hipStream_t stream = nullptr);
void end_timed(uh_ctx* c, hipStream_t stream = nullptr);
void drain_timed(uh_ctx* c);  // the pending kernel timings (option "time_kernels") into ms_by_kind; waits for their events
int read_back(uh_ctx* c, void* dst, const void* src, size_t bytes);
// paths this rank traces per frame: path ids are dense over the pixels it owns
inline uint32_t traced_pixels(const uh_ctx* c) { return c->tiles.world > 1 ? c->tiles.n_owned : c->W * c->H; }
// ---- frame_loop.hip ----
FrameParams make_params(uh_ctx* c, const UhViewUniformData& v);
int sync_all(uh_ctx* c);  // every stream of every slot idle (read-backs, scene rebuilds, stats)
// ---- partition.hip, for frame_loop.hip and rccl_link.hip ----
void restir_rows(const uh_ctx* c, UhRestirRows& r);  // rows of this context's reservoir passes (uh_get_restir_rows)
uint64_t max_pack_pixels(uh_ctx* c);                 // the largest uh_tile_pack_count over the ranks: rank 0's
int mark_composed(uh_ctx* c);                        // records tiles.ev_compose on the context's stream; it becomes last_acc
// ---- grid_cache.hip, for frame_loop.hip and uh_get_stats ----
// the sun grid for this frame's direction / the camera grid for this call's camera, if there is (or now should be) one: this_frame
int ensure_sun_grid(uh_ctx* c, const float dir[3]);
int ensure_camera_grid(uh_ctx* c, const FrameParams& fp, uint32_t batch);
void grid_stats(const uh_ctx* c, UhStats* out);  // the sun_grid_* and camera_grid_* figures
// ---- scene_build.hip, for hybrid_graph.hip ----
// brackets of UhIsosurfaceUpdateStats::scatter_ms on the context's stream (the mesh tables of device-resident meshes count into it)
void iso_scatter_begin(uh_ctx* c);
int iso_scatter_end(uh_ctx* c, bool add);
// ---- scene_build.hip, for pose.hip ----
// The tail of every verb that replaces all vertices of a mesh of uh_add_mesh on the device: the mesh's own vertex buffer and its index
// list on the device (made by the first such call; a refusal leaves the mesh as it was), then serial bumped and the context not built,
// then write() - it fills m.d_verts or exchanges it for a buffer of the same size that is already filled -, then the host copy marked
// valid or stale and the update counted (UhMeshUpdateStats::updates). `verb` names the caller in uh_last_error
int replace_mesh_vertices(uh_ctx* c, HostMesh& m, const char* verb, bool host_valid, const std::function<int()>& write);
// ---- hybrid_graph.hip, for uh_destroy ----
void destroy_graphs(uh_ctx* c);  // everything uh_ctx::Hybrid, uh_ctx::Forward and uh_ctx::Denoise own; before the slots' streams go
#pragma GCC visibility pop
