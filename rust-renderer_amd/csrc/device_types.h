// device_types.h — structs passed between the host context (context.hip, frame_loop.hip) and the kernels
// (kernels.hip and the other kernel files). Device pointers only; everything here is plain data.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "bvh.h"
#include "frame_plan.h"
#include "path_layout.h"
#include "post_levels.h"
#include "sun_grid.h"
#include "utopian_hip.h"

namespace uh {

constexpr uint32_t kMaxBounces = 64;
// per bounce: RAY (paths whose ray the bounce traces; the shading kernels tell hits from misses by the hit
// record, so no hit / miss queues exist) and LIGHT (scattered paths that carry a light sample)
constexpr uint32_t kQueueKinds = 5;
// Q_SUN_TREE: sun rays the grid kernel hands to the tree walk (border cells, long lists). Q_MISS: the paths of a bounce whose ray
// left the scene - k_shade_hit meets them while it classifies the bounce's RAY queue and hands their ids to k_shade_miss
// Q_CAM_TREE (bounce 0 only): primary rays the camera grid hands to the tree walk (pixels with long lists); shares queue 3 with
// Q_SUN_TREE, which the same bounce's sun rays fill only after the shading kernel
enum { Q_RAY = 0, Q_LIGHT = 1, Q_SUN_TREE = 2, Q_MISS = 3, Q_CAM_TREE = 4 };
constexpr uint32_t kLaunchSlots = kMaxBounces * 4 + 8;  // per bounce: closest, sun (grid), sun leftovers (tree), light; bounce 0: + camera grid, its leftovers

// Queues are sharded: path p lives in shard shard_of_run(p / 64) for its whole life, every queue
// has one segment (capacity PathState::shard_cap) and one counter per shard, and the blocks of a
// launch are bound to shards by blockIdx % kShards. A single device-wide counter saturates at
// ~88 atomics/us on MI355X (MI355X_MICROARCH.md "dequeue"), which capped every queue-building
// kernel of the unsharded first version (profiles/r01a_*): 32 shards lift that ceiling 32x - provided
// the 32 counters live in 32 different 128-byte lines (see Control below).
// Blocks b and b + 8 share an XCD under the observed round-robin dispatch, so shard s is served by
// XCD s % 8 and its queue segments stay in that XCD's L2 between producer and consumer launches.
constexpr uint32_t kShards = 32;
constexpr uint32_t kShardBits = 5;
static_assert((1u << kShardBits) == kShards, "kShards is a power of two");
static_assert(kLayoutShards == kShards && kLayoutShardBits == kShardBits, "path_layout.h states the same shards");
// Fibonacci hash of the 64-path run index (top 5 bits). A plain `run % 32` aliases with the tile
// partition: with 64-pixel-wide tiles every run a rank owns is even, which left half of the shards
// (and half of the traversal blocks) empty on every rank of a multi-GPU job.
__host__ __device__ inline uint32_t shard_of_run(uint32_t run) { return (run * 0x9E3779B1u) >> (32 - kShardBits); }

// Zeroed once per sample pass by one hipMemsetAsync.
// Counter layout: the words that one launch hammers concurrently (the same bounce and queue kind, or
// the same launch slot, of all 32 shards) must not share a 128-byte line - atomics to one LINE
// serialise in its L2 channel just like atomics to one word. So the shard (and queue kind) select
// the line and the bounce / launch slot the word inside it.
constexpr uint32_t kBounceStride = ((kMaxBounces + 1 + 31) / 32) * 32;  // words, whole lines
constexpr uint32_t kSlotStride = ((kLaunchSlots + 31) / 32) * 32;
struct Control {
   uint32_t q_count[kShards * kQueueKinds * kBounceStride];
   uint32_t cursor[kShards * kSlotStride];  // persistent-thread work cursors, one per (shard, launch of the pass)
};
__host__ __device__ inline uint32_t qc_index(uint32_t bounce, uint32_t kind, uint32_t shard) { return (shard * kQueueKinds + kind) * kBounceStride + bounce; }
__host__ __device__ inline uint32_t cursor_index(uint32_t slot, uint32_t shard) { return shard * kSlotStride + slot; }

// Persistent across frames; read back by uh_get_stats.
struct DeviceStats {
   unsigned long long rays[UH_RAY_KINDS];
   unsigned long long nodes_visited, tris_tested, shadow_nodes_visited, shadow_tris_tested;
   unsigned long long closest_hits, misses;
   unsigned long long sun_tree_rays;  // sun rays k_trace_sun_grid handed to the tree walk
   unsigned long long cam_tree_rays;  // primary rays k_trace_camera_grid handed to the tree walk
   unsigned long long cam_tris_tested;  // triangle packets k_trace_camera_grid tested (count_visits)
   unsigned long long sun_covered_rays; // sun rays k_trace_sun_grid answered from the cell's cover depth alone (count_visits)
   unsigned long long light_nodes_visited, light_tris_tested;  // the light shadow rays' walks (count_visits)
};

// per-mesh shading record (80 B): inverse instance rotation/scale + the material fields the
// closest-hit shader reads (reference.rchit:22-23,32,40-41,47-89)
struct alignas(16) MeshShade {
   float w2o[9];  // row-major inverse of the object-to-world upper 3x3
   uint32_t diffuse_map;
   float base_color[3];
   float type;      // raytrace_properties.x
   float property;  // raytrace_properties.y
   uint32_t pad;
   float metallic, roughness;  // metallic_factor / roughness_factor: read by material type 4 only (Cook-Torrance extension)
   float pad2[2];
};
static_assert(sizeof(MeshShade) == 80, "mesh shading record");

struct TexInfo {
   const uchar4* texels;
   uint32_t w, h;
   // blocks_x > 0 (every texture unless option "texture_blocks" was 0 when it was added): overlapped blocks of kTexBlockW x
   // kTexBlockH texels, one block per cache line, blocks_x of them per row of blocks (texture_layout.h): a bilinear footprint
   // lies in one line. Otherwise tiles_x > 0: 8x8-texel tiles (256 B, row-major inside the tile, tiles row-major), a footprint
   // in 1.4 lines; both 0: plain row-major (with blocks off, sizes that are not multiples of 8).
   uint32_t tiles_x;
   uint32_t blocks_x;
};

struct SceneDev {
   const uint4* nodes;    // 3 uint4 per Node4C (quantised BVH4 node with implicit child addresses, 48 B)
   const float4* tris;    // 3 float4 per TriPacket
   const float4* shade;   // 4 float4 per ShadePacket
   const MeshShade* meshes;
   const TexInfo* textures;
   const float4* lights;  // 2 float4 per light: (pos, 0), (intensity, 0)
   const float* unorm_lut;  // 256 entries: c / 255.0f (host-computed, exact)
   uint32_t num_nodes, num_tris, num_meshes, num_textures, num_lights;
};

struct FrameParams {
   // A launch chain may carry `batch_frames` consecutive frames of the path-tracing pass as one
   // wavefront: path id = f * (W*H) + pixel. Frames differ only in their RNG frame number and in
   // total_samples (prototype/src/main.rs:467-469 adds samples_per_frame per frame); the
   // accumulate / store tail applies them in frame order, so results equal one-by-one rendering.
   uint32_t batch_frames;
   uint32_t frame_numbers[kMaxBatchFrames];
   uint32_t total_samples_of[kMaxBatchFrames];
   // spatial_reuse_reservoirs of each frame of the batch (rgen:98; a ring in the context: frame_loop.hip render_batch)
   const UhReservoir* spatial_of[kMaxBatchFrames];
   float inv_view[16], inv_proj[16], prev_pv[16];
   float sun_dir[3];  // normalize(view.sun_dir), computed on the host with the contract's normalize
   uint32_t W, H, frame_number;
   uint32_t samples_per_frame, total_samples, num_bounces, accumulation_limit;
   uint32_t sky_enabled, sun_shadow_enabled, lights_enabled, use_ris, full_frame_restir;
   // option "primary_implicit" (camera grid in use, one sample per frame): the state planes of bounce 0 are not materialised -
   // k_generate only fills the ray queue with path ids, and every kernel of bounce 0 computes a path's origin, direction,
   // throughput (1) and RNG words from its id (device_math.h primary_state): 48 bytes less written and 96 less read per path
   uint32_t primary_implicit;
   // option "sun_verdicts" (set per sample pass where the launches are chosen, frame_plan.h plan_sample): 1 = the sun kernels of
   // this pass leave one verdict bit per ray in PathState::sun_lit and the kernels that read a path's radiance next add its throughput
   // there; 0 = the sun kernels add it themselves (lights enabled, no grid for the bounce, the fused kernel's frames, the option off)
   uint32_t sun_verdicts;
   // option "slim_state" (set per sample pass beside sun_verdicts, frame_plan.h plan_sample: sun_verdicts == 1 and one sample per
   // frame): 1 = the pass carries the slim path state (PathState below) - the path id rides with the origin, no id queue is written
   // or read behind bounce 0, throughput and radiance are 24 bytes in 24, and the sun kernels of the last bounce store every surviving
   // path's final radiance (radf[id]) themselves, so k_flush_survivors is not launched; 0 = the four-quad state, the id queues, the flush
   uint32_t slim_state;
   uint32_t furnace;  // option "furnace": the reference's FURNACE_TEST build of the miss shader (reference.rmiss:14-28): a miss returns white
   uint32_t num_lights_used;  // min(view.num_lights, view.max_num_lights_used)
   uint32_t temporal_enabled, spatial_enabled;
   uint32_t tp_rank, tp_world, tp_tile, tiles_x;
   // pixels this rank owns under the tile partition, ascending; nullptr = all W*H pixels. The
   // per-pixel kernels (generate, finish_sample) walk this list, so their cost shrinks with 1/world.
   const uint32_t* owned_pixels;
   uint32_t n_owned;
};

// Path state: four 16-byte quads per path, each quad in a PLANE of its own (SoA), and - round 4 - indexed by the path's POSITION
// IN ITS BOUNCE'S RAY QUEUE (shard segment + position), not by path id. Two SETS of planes ping-pong: set b & 1 holds the paths of
// bounce b's queue; k_shade_hit(b) reads a path's state at its position in queue b and writes the scattered path's new state at
// the position it gets in queue b + 1 (in set (b + 1) & 1). Why: every kernel of the path walks a queue, so state by position is
// read and written as contiguous streams (a wave's scattered paths get consecutive positions from one wave-level append), where
// state by path id was one 64-byte sector per 16-byte record once the first bounce had thinned the ids out (rounds 1-3: the
// shading and sun-ray kernels ran at the memory system's random-sector rate, profiles/r03_counters.json). The price: the
// radiance travels with the path (plane 3: k_shade_hit copies it forward, +32 dense bytes per scattered hit) instead of resting
// in a per-id array, and a path's final radiance is written where the path ends - miss, absorption, or the flush of the paths
// still alive after the last bounce - into `radf`, by path id, once.
// The RNG words ride in the w components the constant ray range (rgen:45-47: 0.001, 10000) does not need:
//   plane 0  ray origin.xyz            | raygen rngState (bits)            reference.rgen:24,31
//   plane 1  ray direction.xyz         | rayPayload.randomSeed (bits)      un-normalised direction (rgen:61); seed: rgen:30, rchit:91
//   plane 2  throughput.rgb            | light weight f                    radiance += throughput * f when the light is visible (rgen:121)
//   plane 3  radiance.rgb              | light index (bits)                rgen:69-78, :118-122 add to it; not materialised for bounce 0 (it is zero), nor - with sun verdicts - for bounce 1
// The hit record of a bounce's ray (t, u, v | packet index, 0xffffffff = miss) lies in a plane of its own at the same position.
// SLIM state (FrameParams::slim_state: no lights, one sample per frame, sun verdicts): the light weight and the light index are never
// read, and the raygen RNG word is consumed by select_light and the next sample's k_generate alone - three dead words. The same
// planes, same stride, then hold 56 bytes per path:
//   plane 0  ray origin.xyz            | path id                           in every set, also what k_generate writes when primary_implicit is off
//   plane 1  ray direction.xyz         | rayPayload.randomSeed (bits)      as above
//   plane 2  throughput.rgb            | radiance.r
//   plane 3  radiance.g, radiance.b                                        8-byte PAIRS by the same position (rec_pair), in the plane's first half
// Where the radiance is not materialised (rad_stored), plane 2's w is a zero nobody reads and plane 3 is not touched. With the id
// beside the origin no kernel behind bounce 0 needs queue[0 / 1]: k_shade_hit neither appends ids nor, at b >= 1, reads them, and a path
// still knows its id where it ends. (Keeping queue[0] and its counts from pass to pass - they depend on the number of ids alone - was
// measured level with rebuilding them and is not done: profiles/README.md "Slim path state".)
constexpr uint32_t kRecQuads = 4;
enum { REC_ORIGIN = 0, REC_DIR = 1, REC_THR = 2, REC_RAD = 3 };
struct PathRecs {
   float4* base;
   size_t plane;  // float4 between two planes (the queue capacity plus a stagger: the planes must not alias in the caches)
};
struct PathState {
   PathRecs set[2];  // set b & 1: state of the paths of bounce b's RAY queue, by queue position
   float4* hit;      // hit record of the bounce being traced, by queue position
   float4* radf;     // by path id: a finished path's radiance.rgb | its raygen rngState (the frame's next sample starts from it, rgen:28-31)
   float4* pixcol;   // by path id: sum over the frame's samples
   // 0,1 = ray ping-pong: path ids; 2 = light, 3 = sun rays for the tree walk: positions in the NEXT bounce's ray queue; 4 = misses:
   // (position in the CURRENT one, id) pairs; each kShards * shard_cap entries
   uint32_t* queue[5];
   // the sun rays' verdicts (FrameParams::sun_verdicts): bit p & 63 of word p >> 6 = the sun ray that left position p of the NEXT bounce's
   // ray queue was not occluded. Shard segments start at multiples of 64, so the 64 positions a wave reads in one piece are one word.
   // One plane: the verdicts of bounce b are read by k_shade_hit(b + 1) (or the flush), which the sun kernels of bounce b + 1 wait for
   unsigned long long* sun_lit;
   uint32_t shard_cap;  // entries per shard segment = pixels a shard can own (multiple of 64)
};
// the address arithmetic of both layouts is path_layout.h rec_offset (checked on the host: tests/cpp/path_layout_check.cpp)
__host__ __device__ inline float4* rec_quad(const PathRecs& rec, uint32_t pos, int quad) {
   return reinterpret_cast<float4*>(reinterpret_cast<char*>(rec.base) + rec_offset(rec.plane, pos, quad));
}
__host__ __device__ inline float2* rec_pair(const PathRecs& rec, uint32_t pos) {  // slim state: plane 3's (radiance.g, radiance.b)
   return reinterpret_cast<float2*>(reinterpret_cast<char*>(rec.base) + rec_offset(rec.plane, pos, REC_RAD, true));
}

// rays of the stand-alone queries (uh_trace_closest, the G-buffer cast): record i = ray i, tmin / tmax in the w components
struct RawRays {
   float4* ray_o;   // origin.xyz, tmin
   float4* ray_d;   // direction.xyz, tmax
   float4* hit;     // t, u, v, packet index (bits)
};

struct Images {
   float4* accumulation;  // pt_accumulation_image RGBA32F
   uchar4* output;        // pt_output_image B8G8R8A8_UNORM
   float4* gbuffer_pos;   // gbuffer_position RGBA32F, un-filtered texels
   UhReservoir* reservoirs[3];          // initial, temporal, spatial (the buffer this frame's spatial pass writes / the path tracer reads)
   const UhReservoir* prev_spatial;     // last frame's spatial_reuse_reservoirs, read by the temporal pass (renderers/mod.rs:294)
};

// Rows of the frame a reservoir-pass launch covers: the whole frame on one GPU; on a rank of an N-rank job (DESIGN.md
// section 5, "band partition") the rank's band of rows plus what its spatial pass gathers from - at most two row intervals
// (spatial_reuse.rgen:54's uvec2 wrap sends the first 30 rows to row H - 1). Work item j of a launch is pixel pixel_of(j).
struct RowSpans {
   uint32_t row0[2], rows[2];  // interval k covers rows [row0[k], row0[k] + rows[k]); rows[1] == 0: one interval
   uint32_t W;
   __host__ __device__ uint32_t total() const { return (rows[0] + rows[1]) * W; }
   __host__ __device__ uint32_t pixel_of(uint32_t j) const {
      const uint32_t first = rows[0] * W;
      return j < first ? row0[0] * W + j : row0[1] * W + (j - first);
   }
};
inline RowSpans whole_frame(uint32_t W, uint32_t H) { return RowSpans{{0, 0}, {H, 0}, W}; }

// The hybrid (rasterized) graph's ray-traced passes (uh_render_hybrid; renderers/mod.rs:61-186): its own G-buffer of four targets
// and the two images rt_shadows / rt_reflections write. Full-frame, pixel = y * W + x everywhere.
struct HybridMesh {           // what gbuffer.vert / gbuffer.frag read per mesh (push constants + Material)
   float o2w[9];              // mat3(world): row-major upper 3x3 of the object-to-world 3x4
   float w2o[9];              // its inverse (= MeshShade::w2o): mat3(transpose(inverse(world))) * n reads it by columns
   uint32_t vertex_base, index_base;  // the mesh's first vertex / index in HybridDev::vertices / indices
   uint32_t diffuse_map, normal_map, metallic_roughness_map, occlusion_map;
};
struct HybridDev {
   float4* pos;       // gbuffer_position RGBA32F
   float4* nrm;       // gbuffer_normal RGBA32F
   uchar4* alb;       // gbuffer_albedo RGBA8
   float4* pbr;       // gbuffer_pbr RGBA32F (metallic, roughness, occlusion, material index)
   uint8_t* shadow;   // rt_shadows output R8
   uchar4* refl;      // rt_reflections output RGBA8
   uint32_t* queue;   // metal pixels, compacted (rt_reflections)
   uint32_t* counter; // [0]: entries of `queue`
   const HybridMesh* meshes;
   const UhVertex* vertices;
   const uint32_t* indices;
   float sun_dir[3];  // normalize(view.sun_dir), as FrameParams::sun_dir
   float eye[3];      // view.eye_pos
   uint32_t W, H, furnace;
};
// the final frame's passes (ssao_pass, deferred_pass, atmosphere_pass, present_pass): their images and what they read of the view
struct HybridLight {  // one light as the deferred pass's loop reads it (k_hybrid_light_prep): 64 B, the light-only terms made once
   float pos[3];      // light.pos
   float mode;        // 0 directional, 1 point, 2 spot, 3 any other type (L = 0, attenuation 1)
   float color[3];    // light.color.rgb
   float spot;        // light.spot
   float att[3];      // light.att
   float pad0;
   float dir[3];      // directional: normalize(light.dir * (-1, 1, -1)) = L; spot: normalize(light.dir)
   float pad1;
};
struct HybridFrameDev {
   uint16_t* ssao;            // ssao_output R16 UNORM
   float4* deferred;          // deferred_output RGBA32F
   uchar4* present;           // present output B8G8R8A8
   uint32_t* sky_counter;     // [0]: sky pixels queued in HybridDev::queue
   HybridLight* lights;       // [0] the sun, [1 .. num_lights] the uh_add_light table in order
   const UhGpuLight* raw_lights;
   float view[16], proj[16], inv_view[16];  // column-major, as UhViewUniformData
   uint32_t num_lights;       // view.num_lights (the sun not counted)
   uint32_t ssao_on, rt_on, fxaa_on;  // view.ssao_enabled == 1, view.raytracing_supported == 1, view.fxaa_enabled == 1
   float sun_raw[3];          // view.sun_dir as given (the sun light's dir = sun_raw * (-1, 1, -1))
};

// the reservoir lights of the hybrid frame (UH_HYBRID_RESTIR_LIGHTS): what the restir_lights pass writes and the deferred pass reads
struct HybridRestirDev {
   uint8_t* vis;                   // light visibility R8: 255 where a ray was cast and found the light, else 0
   uint32_t* queue;                // the pixels that cast a ray, compacted
   uint32_t* counters;             // [0]: entries of `queue` = rays cast, [1]: occluded rays
   const UhReservoir* reservoirs;  // spatial_reuse_reservoirs as the last reservoir pass left them (read only)
   const UhGpuLight* raw_lights;   // the uh_add_light table as added
   uint32_t num_lights;            // view.num_lights, at most the table's length
};

// ray-traced ambient occlusion of the hybrid frame (UH_HYBRID_RTAO; rtao.hip): what its three kernels read and write
struct RtaoDev {
   uint8_t* counts;                // UH_HYBRID_AO_COUNTS: a pixel's occluded rays, G-buffer orientation; whole words (the trace adds by words)
   uint32_t* queue;                // the pixels that cast, compacted
   uint32_t* counters;             // [0]: entries of `queue`, [1]: occluded rays; with count_visits [2..3]: node visits, [4..5]: triangle tests (64 bits each)
   uint32_t samples;               // UhRtaoParams::samples
   uint32_t frame_base;            // frameNumber(view) * 64: ray s seeds its state with frame_base + s
   uint32_t blur_radius;
   float radius, strength, blur_normal_cos, blur_plane;
};

// one-bounce ray-traced diffuse GI of the hybrid frame (UH_HYBRID_RTGI; rtgi.hip): what its kernels read and write. Ray s of the pixel in
// queue slot q is ray q * samples + s in `rays` and in the words of `sun_rays`
struct RtgiDev {
   uint32_t* counts;               // UH_HYBRID_GI_COUNTS: a word per pixel, bytes (low first) sunlit, dark, emitter, missed; added to by words
   float4* radiance;               // UH_HYBRID_GI_RADIANCE: Ef.rgb, w = 1 where the pixel cast, else (0, 0, 0, 0)
   float4* mean;                   // E.rgb of the pixels that cast (the filter's input; not written when blur_radius is 0)
   float4* rays;                   // L.rgb of every ray, by ray number
   float4* sun_rays;               // the sun rays queued by the closest-hit kernel: origin.xyz, ray number (bits)
   uint32_t* queue;                // the pixels that cast, compacted
   uint32_t* counters;             // [0]: entries of `queue`, [1]: entries of `sun_rays`, [2]: rays that missed
   uint32_t samples;               // UhRtgiParams::samples
   uint32_t frame_base;            // frameNumber(view) * 64: ray s seeds its state with (frame_base + s) ^ kRtgiSeedXor
   uint32_t blur_radius;
   float max_radiance, intensity, blur_normal_cos, blur_plane;
};
constexpr uint32_t kRtgiSeedXor = 0x52544749u;  // keeps the rays from being the rtao pass's own

// ray-traced glossy reflections of the hybrid frame (UH_HYBRID_GLOSSY; glossy.hip): what its kernels read and write. Sample s of the pixel
// in queue slot q is ray q * samples + s in `rays`, `orig` and `dirs`; the rays that are cast (not below) are listed in `ray_queue`.
// counts, rays, sun_rays, queue and counters[0..2] are laid out as RtgiDev's: the sun rays go through k_rtgi_shadow (glossy_sun_view)
struct GlossyDev {
   uint32_t* counts;               // UH_HYBRID_GLOSSY_COUNTS: a word per pixel, bytes (low first) sunlit, dark, emitter, missed; added to by words
   float4* scale;                  // UH_HYBRID_GLOSSY_SCALE: Sf.rgb, w = 1 where the pixel cast, else (0, 0, 0, 0)
   float4* bias;                   // UH_HYBRID_GLOSSY_BIAS: Bf.rgb, w likewise
   float4* mean_s;                 // S.rgb and Bi.rgb of the pixels that cast (the filter's input; not written when blur_radius is 0)
   float4* mean_b;
   uint8_t* re;                    // the pixel's filter radius, 255 where it did not cast
   float4* rays;                   // by ray number: the hit record (t, u, v, idx) behind the walk, (Gw L.rgb, x5) behind the shading
   float4* orig;                   // by ray number: origin.xyz, Gw
   float4* dirs;                   // by ray number: direction.xyz, x5
   float4* sun_rays;               // the sun rays queued by the shading: origin.xyz, ray number (bits)
   uint32_t* ray_queue;            // the numbers of the rays that are cast, compacted
   uint32_t* queue;                // the pixels that cast, compacted
   uint32_t* counters;             // [0]: entries of `queue`, [1]: entries of `sun_rays`, [2]: rays that missed, [3]: entries of `ray_queue`, [4]: below samples
   uint32_t samples;               // UhGlossyParams::samples
   uint32_t frame_base;            // frameNumber(view) * 64: sample s seeds its state with (frame_base + s) ^ kGlossySeedXor
   uint32_t blur_radius;
   uint32_t rt_on;                 // view.raytracing_supported == 1: type-1 pixels hold their mirror
   float max_roughness, max_radiance, intensity, blur_roughness, blur_normal_cos, blur_plane;
};
// emissive meshes as area lights of the hybrid frame (UH_HYBRID_AREA_LIGHTS; area_lights.hip). The emitter table, n slots in canonical
// order (slot = base[mesh] + prim), filled from the tree's triangle packets; and what the pass's kernels read and write. Sample s of the
// pixel in queue slot q is number q * samples + s in rec_d and rec_s; the samples that cast a ray are listed in `rays`
struct AreaTableDev {
   float4* tri;                    // 3 per slot: (v0, area), (e1, weight bits), (e2, 0)
   uint32_t* keys;                 // the packet's key, mesh << kPrimBits | prim
   float* areas;                   // 0.5 |cross(e1, e2)|, 0 when that is not finite
   uint32_t* weights;              // q
   uint32_t* cum;                  // the inclusive prefix of q
   const uint32_t* base;           // per mesh: its first slot, kNoEmitter for a mesh that is no emitter
   uint32_t* amax;                 // the bits of the largest area
   unsigned long long* total;      // cum[n - 1]; 0 without emitters
   uint32_t n, num_meshes;
};
constexpr uint32_t kNoEmitter = 0xffffffffu;
struct AreaDev {
   AreaTableDev tab;
   uint32_t* counts;               // UH_HYBRID_AREA_COUNTS: a word per pixel, bytes (low first) lit, occluded, away, 0; added to by words
   float4* diffuse;                // UH_HYBRID_AREA_DIFFUSE: Df.rgb, w = 1 where the pixel cast, else (0, 0, 0, 0)
   float4* specular;               // UH_HYBRID_AREA_SPECULAR: Spf.rgb, w likewise
   float4* mean_d;                 // D and Sp of the pixels that cast (the filter's input; not written when blur_radius is 0)
   float4* mean_s;
   float4* rec_d;                  // d_s and s_s of every sample, by sample number; zero for an AWAY or OCCLUDED one
   float4* rec_s;
   float4* rays;                   // 2 per queued shadow ray: (o, sample number bits), (Y, 0)
   uint32_t* queue;                // the pixels that cast, compacted
   uint32_t* counters;             // [0]: entries of `queue`, [1]: entries of `rays`, [2]: occluded rays, [3]: emitter pixels
   uint32_t samples;               // UhAreaLightParams::samples
   uint32_t frame_base;            // frameNumber(view) * 64: sample s seeds its state with (frame_base + s) ^ kAreaSeedXor
   uint32_t blur_radius, show_emitters;
   uint32_t rt_on;                 // view.raytracing_supported == 1: type-1 pixels hold their mirror
   float max_weight, max_radiance, intensity, blur_normal_cos, blur_plane;
};
constexpr uint32_t kAreaSeedXor = 0x41524541u;  // keeps the samples from being another pass's own
constexpr uint32_t kAreaMaxEmitters = 1u << 20;

constexpr uint32_t kGlossySeedXor = 0x474C4F53u;  // keeps the samples from being the rtao or rtgi pass's own

// volumetric fog of the hybrid frame (UH_HYBRID_FOG; fog.hip): what its kernels read and write
struct FogDev {
   uint32_t* mask;                 // UH_HYBRID_FOG_MASK: a word per pixel, bit k = sample k saw the sun; 0 where the pixel did not march
   float4* terms;                  // UH_HYBRID_FOG_TERMS: (a, Ttot, F, Ff), all 0 where the pixel did not march
   float* dist;                    // the march length D of a pixel that marched (classify writes it); 0 where it did not
   uint32_t* queue;                // the pixels that march, compacted
   uint32_t* counters;             // [0]: entries of `queue`, [1]: lit rays; with count_visits [2..3]: node visits, [4..5]: triangle tests (64 bits each)
   uint32_t steps;                 // UhFogParams::steps
   uint32_t frame_seed;            // (frameNumber(view) * 64) ^ kFogSeedXor: the state of a pixel's one jitter xi
   uint32_t blur_radius;
   float density, max_distance, anisotropy, intensity, blur_depth;
   float albedo[3], ambient[3];
};
constexpr uint32_t kFogSeedXor = 0x464F4721u;  // keeps the jitter from being another pass's sample

// ray-traced glass of the hybrid frame (UH_HYBRID_GLASS; glass.hip): what its kernels read and write. Chain c (0 reflected, 1 transmitted)
// of the pixel in queue slot q is ray q * 2 + c in `rays`, `orig` and `dirs`. Round r walks the rays listed in ray_queue[r & 1], whose
// count is counters[kGlassRound0 + r], and its bend kernel lists the chains that go on in ray_queue[(r + 1) & 1], counted in
// counters[kGlassRound0 + r + 1]: no host read-back between rounds. counts, rays, sun_rays, queue and counters[0..2] are laid out as
// RtgiDev's with samples = 2: the sun rays go through k_rtgi_shadow (glass_sun_view)
constexpr uint32_t kGlassMaxEvents = 16, kGlassRound0 = 8, kGlassCounters = kGlassRound0 + kGlassMaxEvents + 1;
static_assert(kGlassRound0 >= 3, "glass_walk_view points GlossyDev::counters three words before a round's counter");
struct GlassDev {
   uint32_t* counts;               // UH_HYBRID_GLASS_COUNTS: a word per pixel, bytes (low first) sunlit, dark, emitter, missed; added to by words
   float4* radiance;               // UH_HYBRID_GLASS_RADIANCE: (C, 1) where the pixel cast, else (0, 0, 0, 0)
   uint32_t* events;               // UH_HYBRID_GLASS_EVENTS: a word per pixel, byte 0 / 1 the events of chain 0 / 1, byte 2 the flags; added to by words
   float4* rays;                   // by ray number: the hit record (t, u, v, idx) behind a round's walk, (w L.rgb, 0) once the chain has ended
   float4* orig;                   // by ray number: the segment's origin.xyz, the chain's weight w
   float4* dirs;                   // by ray number: the segment's direction.xyz (unnormalised), the chain's events so far (bits)
   float4* sun_rays;               // the sun rays queued by the bend kernels: origin.xyz, ray number (bits)
   uint32_t* ray_queue[2];         // the numbers of the rays of a round, compacted; ping-pong
   uint32_t* queue;                // the pixels that cast, compacted
   uint32_t* counters;             // [0]: entries of `queue`, [1]: entries of `sun_rays`, [2]: chains that missed,
                                   // [4]: events at which `cannot` held, [5]: chains cut, [kGlassRound0 + r]: the rays of round r
   uint32_t max_events;            // UhGlassParams::max_events
   float max_radiance, intensity;
};
constexpr uint32_t kGlassTir = 1u << 16, kGlassCut0 = 1u << 17;  // the flag bits of an events word (chain c cut: kGlassCut0 << c)

// the denoiser (uh_denoise; denoise.hip): one frame's guides and moments as the next call's history reads them
struct DenoiseHistory {
   float4* pos;                    // the position texel (w != 0: geometry)
   float4* nrm;                    // the normal texel's xyz, w = the mesh index (pbr.a)
   float4* col;                    // temporal colour (demodulated), w = history length N
   float2* mom;                    // temporal first and second luminance moments
};
struct DenoiseDev {
   const float4* acc;              // the path tracer's accumulation image (read only)
   const float4 *g_pos, *g_nrm, *g_pbr;  // the hybrid G-buffer (read only)
   const uchar4* g_alb;
   const float* unorm_lut;         // c / 255
   DenoiseHistory prev, cur;       // the previous call's set (read) and this call's (written by the temporal stage)
   float4* input;                  // UH_DENOISE_INPUT
   float4* cv[2];                  // the filter's images: colour and variance, ping-pong; the temporal stage writes cv[0]
   float4* temporal;               // UH_DENOISE_TEMPORAL_COLOR
   float4* color;                  // UH_DENOISE_COLOR
   uchar4* output;                 // UH_DENOISE_OUTPUT
   float* history;                 // UH_DENOISE_HISTORY
   float* variance;                // UH_DENOISE_VARIANCE
   uint32_t* counters;             // [0] geometry pixels, [1] pixels that kept a history
   uint32_t W, H;
   float n;                        // min(total_samples, accumulation_limit)
   float view[16], prev_pv[16];    // column-major
   uint32_t temporal_on;           // UH_DENOISE_TEMPORAL and a history exists
   uint32_t demodulate;
   float max_history, alpha_min, sigma_luminance, sigma_plane, reproject_normal_cos, reproject_plane;
   const float4* motion;           // UH_HYBRID_MOTION_IMAGE with UH_DENOISE_MOTION, else null (the launcher picks the instantiation)
};

// motion vectors (UH_HYBRID_MOTION; motion.hip, motion_device.h): one row per mesh of the scene, written by the host before a motion pass
enum MotionState : uint32_t { kMotionStatic = 0, kMotionRigid = 1, kMotionDeformed = 2, kMotionNone = 3 };
struct MotionMesh {                // 64 B
   float prev_o2w[12];             // the object-to-world 3x4 (row-major) the tree was baked with at the previous motion pass
   uint32_t prev_base, prev_count; // the mesh's rows in MotionDev::prev_pos at the previous pass (read when state is deformed)
   uint32_t state;                 // MotionState
   uint32_t pad;
};
struct MotionDev {
   float4* image;                  // UH_HYBRID_MOTION_IMAGE
   const MotionMesh* meshes;
   const float4* prev_pos;         // object-space positions at the previous pass, w unused
   uint32_t* counters;             // per block of the motion kernel's grid: [2 b] its geometry pixels with a correspondence, [2 b + 1] without
};

// temporal anti-aliasing of the hybrid frame (UH_HYBRID_TAA; taa.hip): what its kernel reads and writes
constexpr uint32_t kTaaCounterSlots = 256, kTaaCounterStride = 16;  // a 64-byte line per pair: 16 KiB
struct TaaDev {
   const float4* deferred;         // deferred_output as the call's passes left it
   const float4* pos;              // the G-buffer's position image (w != 0: geometry)
   const float4* motion;           // UH_HYBRID_MOTION_IMAGE with UH_TAA_MOTION, else null (the launcher picks the instantiation)
   const float4* prev_col;         // the previous pass's taa_output and N; null: no history (the first pass, or after a reset)
   const float* prev_n;
   float4* col;                    // UH_HYBRID_TAA_OUTPUT
   float* n;                       // UH_HYBRID_TAA_HISTORY
   uint32_t* counters;             // kTaaCounterSlots pairs, kTaaCounterStride words apart: [0] pixels that blended a history, [1] pixels
                                   // that started one; a wave adds into the pair of its number modulo the slots, the host adds the pairs up
   uint32_t clamp;                 // UH_TAA_CLAMP
   float max_history, alpha_min, clamp_gamma;
};

// the HDR display chain of the hybrid frame (UH_HYBRID_POST; post.hip): what its kernels read and write
constexpr uint32_t kPostBins = 256;
// the exposure record, on the device from one pass to the next: the exposure E the later kernels of a pass read, its target and the
// metered average (0 where there was none), the metered pixels (bins 1..255) and the bad pixels the composite kernel counted
struct PostRecord {
   float exposure, target, lavg;
   uint32_t metered, bad, pad[3];
};
struct PostDev {
   const float4* src;              // S: taa_output of this call, deferred_output, or uh_post_image's upload
   float4* out;                    // post_output
   uint32_t* hist;                 // kPostBins counts, zero between passes (the exposure kernel takes them and zeroes them again)
   uint32_t* hist_copy;            // the last metered pass's counts, for uh_read_post
   PostRecord* rec;
   float4* down[kPostMaxLevels + 1];  // [k]: level k, 1..levels ([0] unused); up[levels] is down[levels]
   float4* up[kPostMaxLevels + 1];
   uint32_t lw[kPostMaxLevels + 1], lh[kPostMaxLevels + 1];  // level sizes, [0] the frame's
   uint32_t levels;                // the levels this pass builds: 0 without UH_POST_BLOOM or for a 1 x 1 frame
   uint32_t W, H;
   uint32_t auto_exposure;         // UH_POST_AUTO_EXPOSURE
   uint32_t have_prev;             // rec->exposure is a previous pass's (not the first pass, not after uh_reset_post_exposure)
   uint32_t tonemap;               // UH_TONEMAP_*
   float manual_exposure, key, min_exposure, max_exposure, adaptation, low_percentile, high_percentile, bloom_threshold, bloom_intensity;
};

// launch wrappers implemented in kernels.hip, path_fused.hip, restir.hip, tiles.hip and hybrid_kernels.hip --------------------------------------------------
struct LaunchCfg {
   hipStream_t stream;
   uint32_t num_cus;
   uint32_t closest_blocks_per_cu, shadow_blocks_per_cu;
   bool count_visits;
   uint32_t fused_blocks_per_cu = 4;  // k_path_fused's grid (option "fused_bounces" 2..8); its registers and LDS are sized for path_fused.hip kFusedBlocks
};

void launch_generate(const LaunchCfg&, const FrameParams&, const PathState&, Control*, uint32_t sample);
void launch_trace_closest(const LaunchCfg&, const SceneDev&, const PathState&, Control*, DeviceStats*, uint32_t bounce, uint32_t cursor_slot,
                          int ray_kind);
void launch_trace_camera_grid(const LaunchCfg&, const FrameParams&, const SceneDev&, const PathState&, Control*, DeviceStats*, uint32_t cursor_slot_grid, uint32_t cursor_slot_tree,
                              const SunGridDev&, bool leftovers_possible = true);  // false: the grid's longest list is one its kernel walks itself - no tree-walk launch behind it
void launch_shade_miss(const LaunchCfg&, const FrameParams&, const PathState&, Control*, DeviceStats*, uint32_t bounce);
void launch_shade_hit(const LaunchCfg&, const FrameParams&, const SceneDev&, const PathState&, const Images&, Control*, DeviceStats*, uint32_t bounce);
// bounce 0 in one kernel (frame_plan.h SamplePlan::fused_primary): stands in for launch_generate, launch_trace_camera_grid and launch_shade_hit(0)
void launch_primary_shade(const LaunchCfg&, const FrameParams&, const SceneDev&, const PathState&, Control*, DeviceStats*, const SunGridDev&);
// the paths still alive after the last bounce hand their radiance to the per-id array k_finish_sample reads
// (not launched for a pass with FrameParams::slim_state: its last sun kernels store the radiance themselves)
void launch_flush_survivors(const LaunchCfg&, const FrameParams&, const PathState&, Control*);
void launch_path_fused(const LaunchCfg&, const FrameParams&, const SceneDev&, const PathState&, Control*, DeviceStats*, const SunGridDev& g, bool use_grid, bool sun_of_bounce0);
void launch_trace_shadow(const LaunchCfg&, const FrameParams&, const SceneDev&, const PathState&, Control*, DeviceStats*, uint32_t bounce,
                         uint32_t cursor_slot, bool light, bool sun_leftovers = false);
// sun shadow rays through the per-direction grid (sun_grid.h) instead of the tree
void launch_trace_sun_grid(const LaunchCfg&, const FrameParams&, const SceneDev&, const PathState&, Control*, DeviceStats*, uint32_t bounce,
                           uint32_t cursor_slot, const SunGridDev&);
void launch_finish_sample(const LaunchCfg&, const FrameParams&, const PathState&, const Images&, uint32_t sample, bool last);
void launch_resolve(const LaunchCfg&, const Images&, uint32_t W, uint32_t H, uint32_t total_samples, uint32_t limit);
// G-buffer + ReSTIR
// the reservoir passes and the G-buffer cast over the rows of `spans`; `counted` = the G-buffer rays this launch adds to the
// statistics (a rank counts its own band, not the halo it casts again)
void launch_gbuffer(const LaunchCfg&, const FrameParams&, const SceneDev&, const RawRays&, const Images&, DeviceStats*, const RowSpans& spans, uint32_t counted,
                    const SunGridDev* camera_grid = nullptr);  // camera_grid: the cast walks the per-camera grid instead of the tree
void launch_reset_reservoirs(const LaunchCfg&, const FrameParams&, const Images&, const RowSpans& spans);
void launch_initial_ris(const LaunchCfg&, const FrameParams&, const SceneDev&, const Images&, const RowSpans& spans);
void launch_temporal_reuse(const LaunchCfg&, const FrameParams&, const SceneDev&, const Images&, const RowSpans& spans);
void launch_spatial_reuse(const LaunchCfg&, const FrameParams&, const SceneDev&, const Images&, const RowSpans& spans);
// stand-alone queries (n rays in ray_o/ray_d[0..n), identity queue)
void launch_trace_closest_raw(const LaunchCfg&, const SceneDev&, const float4* ray_o, const float4* ray_d, float4* hit, uint32_t n);
void launch_trace_any_raw(const LaunchCfg&, const SceneDev&, const float4* ray_o, const float4* ray_d, uint32_t* occluded, uint32_t n);
// the hybrid graph's passes (uh_render_hybrid): every pixel of the frame
void launch_hybrid_clear(const LaunchCfg&, const HybridDev&);
// the G-buffer cast of launch_gbuffer (same rays, same traversal choice) and the resolve of all four targets; the cast's ray and hit
// records live in the targets themselves until the resolve (ray_o = normal, ray_d = pbr, hit = position target)
void launch_hybrid_gbuffer(const LaunchCfg&, const FrameParams&, const SceneDev&, const HybridDev&, const SunGridDev* camera_grid);
// its two halves, for a pass that runs k_hybrid_motion between them
void launch_hybrid_gbuffer_cast(const LaunchCfg&, const FrameParams&, const SceneDev&, const HybridDev&, const SunGridDev* camera_grid);
void launch_hybrid_gbuffer_resolve(const LaunchCfg&, const SceneDev&, const HybridDev&);
// the motion pass (motion.hip): the cast form's kernel over the pixels' hit records, between the cast and the resolve; the snapshot of
// n vertices' positions, vertex i of `src` to row i of `dst`
void launch_hybrid_motion(const LaunchCfg&, const SceneDev&, const HybridDev&, const MotionDev&);
void launch_motion_snapshot(const LaunchCfg&, const UhVertex* src, float4* dst, uint32_t n);
void launch_hybrid_shadows(const LaunchCfg&, const SceneDev&, const HybridDev&);
void launch_hybrid_frame_clear(const LaunchCfg&, const HybridDev&, const HybridFrameDev&);
void launch_hybrid_ssao(const LaunchCfg&, const HybridDev&, const HybridFrameDev&);
void launch_hybrid_present(const LaunchCfg&, const HybridDev&, const HybridFrameDev&);
// image-based lighting (setup_cubemap_pass, ibl.rs; ibl.hip): the four maps and their consumers
constexpr uint32_t kEnvSize = 512, kEnvMips = 8, kLutSize = 512;
// the irradiance filter's float-stepped loops (irradiance_filter.frag:38-41): phi 0, 0.025, ... < 2 PI; theta 0, 0.025, ... < PI / 2
constexpr uint32_t kIrrPhi = 252, kIrrTheta = 63;
// a cube of kEnvSize: mip m (size kEnvSize >> m) starts at texel env_mip_offset(m); face f of it at + f * size^2; row-major inside
__host__ __device__ inline uint32_t env_mip_offset(uint32_t m) {
   uint32_t o = 0;
   for (uint32_t k = 0; k < m; k++) o += 6u * (kEnvSize >> k) * (kEnvSize >> k);
   return o;
}
struct IblMaps {                // what the consumers read
   const float4* env;           // environment cube, kEnvMips mips
   const float4* irr;           // irradiance cube, mip 0
   const float4* spec;          // prefiltered specular cube, kEnvMips mips
   const uint32_t* lut;         // BRDF LUT, kLutSize^2 half pairs (R in the low 16 bits)
};
struct EnvDev {                 // what the build writes
   float4* env;
   float4* irr;
   float4* spec;
   uint32_t* lut;
   const float4* taps;          // kIrrPhi * kIrrTheta: (sin t cos p, sin t sin p, cos t, sin t), phi-major, rounded from double
   float eye[3];                // rayStart: the translation of view.inverse_view
   float sun[3];                // view.sun_dir as given
};
void launch_env_cube(const LaunchCfg&, const EnvDev&);
void launch_env_irradiance(const LaunchCfg&, const EnvDev&);
void launch_env_specular(const LaunchCfg&, const EnvDev&);
void launch_env_brdf_lut(const LaunchCfg&, const EnvDev&);
// the passes with an IBL branch: nullptr for the non-IBL one (the sky's: the environment cube, or IntegrateScattering)
void launch_hybrid_reflections(const LaunchCfg&, const SceneDev&, const HybridDev&, const IblMaps* ibl);
// the deferred pass's calculateShadow (shadow_mapping.glsl) reads the cascaded shadow maps with the params they were rendered with
struct ShadowLookup {
   const float* maps;           // 4 layers of size^2 D32, row 0 at NDC y = +1
   const UhShadowmapParams* params;  // the snapshot the maps were rendered with (device copy)
   uint32_t size;
};
// restir: when not null, the light loop evaluates the sun alone and the pixels whose visibility texel is 255 add their reservoir's light
void launch_hybrid_deferred(const LaunchCfg&, const SceneDev&, const HybridDev&, const HybridFrameDev&, const IblMaps* ibl,
                            const ShadowLookup* shadow, const HybridRestirDev* restir = nullptr);
// the restir_lights pass: classify (which pixels cast a ray toward their reservoir's light), then the rays; rl.counters zeroed by the caller
void launch_hybrid_restir_lights(const LaunchCfg&, const FrameParams&, const SceneDev&, const HybridDev&, const HybridRestirDev&);
// the rtao pass (rtao.hip): classify (which pixels cast; their counts zeroed) and the rays; ao.counters zeroed by the caller;
// LaunchCfg::count_visits: the walks' visits are counted there too. order: 0 an
// item is one ray, a pixel's samples consecutive; 1 an item is one ray, one sample of consecutive queued pixels; 2 an item is a pixel,
// whose lane walks its samples one after the other and stores the count once
void launch_rtao_trace(const LaunchCfg&, const SceneDev&, const HybridDev&, const RtaoDev&, uint32_t order);
// ao (and its filter, blur_radius > 0) from the counts into ssao_output, texel (x, y) = G-buffer pixel (x, H - 1 - y)
void launch_rtao_resolve(const LaunchCfg&, const HybridDev&, const RtaoDev&, uint16_t* ssao);
// the rtgi pass (rtgi.hip), a launcher per timed stage; gi.counters zeroed by the caller. trace: classify (which pixels cast; counts and
// radiance zeroed) and the closest-hit walk that shades its rays and queues the sun rays (order: 0 a pixel's samples are consecutive
// items, 1 one sample of consecutive queued pixels); shadow: the any-hit walk over the queued sun rays; filter: E from the rays in sample
// order, then (blur_radius > 0) the tile filter; composite: deferred_output.rgb += the pixel's share of Ef
void launch_rtgi_trace(const LaunchCfg&, const SceneDev&, const HybridDev&, const RtgiDev&, uint32_t order);
void launch_rtgi_shadow(const LaunchCfg&, const SceneDev&, const HybridDev&, const RtgiDev&);
void launch_rtgi_filter(const LaunchCfg&, const HybridDev&, const RtgiDev&);
void launch_rtgi_composite(const LaunchCfg&, const SceneDev&, const HybridDev&, const HybridFrameDev&, const RtgiDev&);
// the fog pass (fog.hip), a launcher per timed stage; fg.counters zeroed by the caller. trace: classify (which pixels march; their march
// length written, their mask zeroed) and the any-hit walk of their samples' sun rays into the masks (order: 0 a pixel's samples are
// consecutive items, 1 one sample of consecutive queued pixels, 2 an item is a pixel whose lane walks its samples one after the other);
// LaunchCfg::count_visits: the walks' visits go to fg.counters too. resolve: (a, Ttot, F, Ff) from the masks, Ff through the tile filter
// when blur_radius > 0; composite: deferred_output.rgb of every pixel that marched
void launch_fog_trace(const LaunchCfg&, const FrameParams&, const SceneDev&, const HybridDev&, const FogDev&, uint32_t order);
void launch_fog_resolve(const LaunchCfg&, const HybridDev&, const FogDev&);
void launch_fog_composite(const LaunchCfg&, const FrameParams&, const HybridDev&, const HybridFrameDev&, const FogDev&);
// the taa pass (taa.hip): one lane per pixel; fp gives the frame, the matrices of primary_ray and prev_pv; t.counters zeroed by the caller
void launch_hybrid_taa(const LaunchCfg&, const FrameParams&, const TaaDev&);
// the three stages of the post pass (post.hip). meter: the histogram (with auto_exposure) and the exposure record; bloom: down[1..levels]
// and up[levels - 1..1] (levels >= 1); composite: post_output, and the bad pixels into the record
void launch_post_meter(const LaunchCfg&, const PostDev&);
void launch_post_bloom(const LaunchCfg&, const PostDev&);
void launch_post_composite(const LaunchCfg&, const PostDev&);
// the shadow-map rasteriser (shadow_map.hip): setup per (triangle, cascade), binning into kShadowTile^2 tiles, resolve per tile in LDS
constexpr uint32_t kShadowTile = 128;
struct ShadowDev {
   const UhVertex* vertices;    // HybridDev's tables: vertex vertex_base + indices[3 t + k] of triangle t (mesh tri_mesh[t])
   const uint32_t* indices;
   const HybridMesh* meshes;
   const uint32_t* tri_mesh;
   const float* mats;           // [cascade][mesh][16]: vp[cascade] * world, column-major, last row (0, 0, 0, 1)
   uint32_t num_tris, num_meshes, size, tiles_x;
   uint32_t* rec_count;         // [cascade * num_tris + t]: the records of (t, cascade); scanned in place into record offsets
   uint32_t* tile_count;        // [cascade * tiles_x^2 + tile]: entries per tile; scanned in place into the tiles' first entries
   uint32_t* tile_cursor;       // a copy of the tiles' first entries, advanced by the scatter to their ends
   uint4* records;              // 3 per record
   uint32_t* entries;           // record ids, grouped by tile
   float* maps;
};
void launch_shadow_count(const LaunchCfg&, const ShadowDev&);
void launch_shadow_emit(const LaunchCfg&, const ShadowDev&);
void launch_shadow_resolve(const LaunchCfg&, const ShadowDev&);
// skip: when not null, a pixel p with skip[p] != 0xFFFFFFFF is not sky (the marching-cubes pass's visibility: the atmosphere pass's
// depth test against the fragments it drew)
void launch_hybrid_sky(const LaunchCfg&, const FrameParams&, const HybridDev&, const HybridFrameDev&, const IblMaps* cube, const uint32_t* skip = nullptr);
// the forward pass's rasteriser (forward.hip): setup per triangle, binning into kForwardTile^2 tiles, a visibility buffer resolved per
// tile in LDS (the 64-bit min of depth bits << 32 | ~record), then one shading lane per pixel
constexpr uint32_t kForwardTile = 64;
struct ForwardDev {
   const UhVertex* vertices;    // HybridDev's tables: vertex vertex_base + indices[3 t + k] of triangle t (mesh tri_mesh[t]); t is the draw index
   const uint32_t* indices;
   const HybridMesh* meshes;
   const uint32_t* tri_mesh;
   const float* mats;           // [mesh][28]: (P V) W column-major (16), then the instance's 3x4 row-major (12); the marching-cubes
                                // pass: mesh 0 with W the identity, then P V (16) for its depth seed
   uint32_t num_tris, W, H, tiles_x, tiles_y;
   uint32_t* rec_count;         // [t]: the records of triangle t; scanned in place into record offsets (so records follow draw order)
   uint32_t* tile_count;        // [tile]: entries per tile; scanned in place into the tiles' first entries
   uint32_t* tile_cursor;       // a copy of the tiles' first entries, advanced by the scatter to their ends
   uint4* records;              // 6 per record
   uint32_t* entries;           // record ids, grouped by tile
   float* depth;                // W * H, row 0 at NDC y = +1
   uint32_t* vis;               // W * H draw indices, 0xFFFFFFFF none
   uint32_t* rec_of;            // W * H: the surviving record, 0xFFFFFFFF none
   float4* color;               // forward_output, W * H
   uint32_t* covered;           // [0]: pixels the resolve left covered
};
struct ForwardShade {           // what forward.frag reads besides the scene and the fragment
   const HybridLight* lights;   // k_hybrid_light_prep's records, the sun first
   uint32_t count;              // view.num_lights + 1
   float eye[3];                // view.eye_pos
   float view[16];              // view.view (calculateShadow's cascade choice)
};
void launch_forward_clear(const LaunchCfg&, const ForwardDev&, uchar4* present);
// flat: the marching-cubes pass's triangle source (vertex 3 t + k of triangle t, mesh 0 of `meshes` and `mats`; shading leaves the
// pixels it does not cover untouched); seeded: the resolve starts from the depths in `depth` and loses ties
void launch_forward_count(const LaunchCfg&, const ForwardDev&, bool flat = false);
void launch_forward_emit(const LaunchCfg&, const ForwardDev&, bool flat = false);
void launch_forward_resolve(const LaunchCfg&, const ForwardDev&, bool seeded = false);
void launch_forward_shade(const LaunchCfg&, const SceneDev&, const ForwardDev&, const ForwardShade&, const ShadowLookup* shadow, bool flat = false);
// the hybrid graph's rasterised G-buffer: gbuffer.frag on the surviving records of a resolve of the scene's meshes into hd's four targets
void launch_gbuffer_raster_shade(const LaunchCfg&, const SceneDev&, const ForwardDev&, const HybridDev&);
// the rasterised form's motion pass, on the same surviving records, behind launch_gbuffer_raster_shade (it reads the position target)
void launch_gbuffer_raster_motion(const LaunchCfg&, const SceneDev&, const ForwardDev&, const HybridDev&, const MotionDev&);
// the marching-cubes pass's depth buffer from the G-buffer positions, into fd.depth; P V column-major at fd.mats + 28
void launch_mc_depth_seed(const LaunchCfg&, const float4* gbuffer_pos, const ForwardDev&);
void launch_hybrid_light_prep(const LaunchCfg&, const HybridFrameDev&);
// the denoiser's stages (denoise.hip): input + temporal (counters zeroed by the caller), the short-history variance estimate, one
// a-trous level of step 1 << level from cv[level & 1] into cv[~level & 1], and the output from cv[from]
void launch_denoise_temporal(const LaunchCfg&, const DenoiseDev&);
void launch_denoise_variance(const LaunchCfg&, const DenoiseDev&);
void launch_denoise_atrous(const LaunchCfg&, const DenoiseDev&, uint32_t level);
void launch_denoise_output(const LaunchCfg&, const DenoiseDev&, uint32_t from);
// tiles
// on-device refit (refit.hip): per-mesh object->world rows, and what one refit pass touches
struct RefitMesh {
   float o2w[12];
   uint32_t identity;
   uint32_t pad[3];
};
struct RefitArgs {
   const float* obj_corners;   // 9 floats per triangle packet, object space, leaf order
   const RefitMesh* meshes;
   float4* tris;               // TriPacket array, rewritten
   float* world_corners;       // scratch, 9 floats per packet
   uint4* nodes;               // Node4C array: origin, step exponents and planes rewritten; counts and bases kept
   float* node_box;            // scratch, 6 floats per node (unpadded)
   const uint32_t* level_start;  // HOST array: BFS level l = nodes [level_start[l], level_start[l+1])
   uint32_t num_levels;
   uint32_t num_tris;
};
void launch_refit(const LaunchCfg&, const RefitArgs&);

// uh_update_mesh_vertices (deform.hip): a mesh that keeps its vertices on the device behind its index list, as k_deform_gather reads
// it - one row per mesh of the scene; a row with moved == 0 is never dereferenced
struct DeformMesh {
   const UhVertex* verts;
   const uint32_t* indices;
   uint32_t moved;
   uint32_t pad;
};
// every triangle packet i (leaf order) of a moved mesh: obj_corners[9 i ..] and shade[4 i ..] again from the mesh's vertices
void launch_deform_gather(hipStream_t, const DeformMesh* table, uint32_t num_meshes, const float4* tris, float* obj_corners, float4* shade, uint32_t num_tris);
// the on-device build's sources of one such mesh (k_iso_scatter's outputs, through the index list), already offset to its range
void launch_deform_scatter(hipStream_t, const UhVertex* verts, const uint32_t* indices, uint32_t num_tris, uint32_t mesh, float* corners, uint32_t* keys, float4* shade);
// the box of ALL its vertices, as build_on_device's host loop takes it: box[0..2] minima, box[3..5] maxima as ordered integers
// (initialise to 0xffffffff / 0, read with uhi_box_decode)
void launch_deform_box(hipStream_t, const UhVertex* verts, uint32_t num_vertices, uint32_t* box);
// *flag |= 1 when a position among `verts` (any alignment a UhVertex may have) is not finite
void launch_deform_check(hipStream_t, const UhVertex* verts, uint32_t num_vertices, uint32_t* flag);

// on-device LBVH build (lbvh.hip): topology + packets in Morton order; boxes come from launch_refit afterwards
struct LbvhArgs {
   const float* src_corners;     // 9 floats per triangle, object space, mesh order
   const uint32_t* src_keys;     // mesh << 22 | primitive, mesh order
   const float4* src_shade;      // ShadePacket (4 float4) per triangle, mesh order
   const RefitMesh* meshes;
   float bounds_lo[3], bounds_hi[3];  // world-space box containing every centroid (Morton normalisation)
   uint32_t num_tris;
   uint32_t kind;                // binary tree under the 4-wide collapse: 1 = PLOC (default), 2 = radix tree (Karras)
   uint32_t ploc_radius;         // PLOC: places searched to either side for the nearest neighbour (1..64)
   uint32_t sah_top;             // PLOC: the rounds stop at this many clusters and a binned-SAH tree over them (host, bvh_build.cpp) is the top; <= 1: PLOC to the root
   uint4* nodes;                 // out: Node4C array (child counts and bases valid, boxes to be refitted)
   uint32_t node_capacity;       // nodes the array can hold
   float4* tris;                 // out: TriPacket array in leaf order (keys; refit writes the geometry)
   float4* shade;                // out: ShadePacket array in leaf order
   float* obj_corners;           // out: object-space corners in leaf order (the refit input)
};
hipError_t lbvh_build(const LbvhArgs&, hipStream_t, std::vector<uint32_t>& level_start, uint32_t* out_nodes);

void launch_pack_tiles(const LaunchCfg&, const float4* acc, float4* out, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile);
void launch_unpack_tiles(const LaunchCfg&, float4* acc, const float4* in, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile);
void launch_compose_tiles(const LaunchCfg&, const Images&, const float4* all, uint64_t stride, uint32_t W, uint32_t H, uint32_t rank, uint32_t world, uint32_t tile,
                          uint32_t total_samples, uint32_t limit);
uint32_t query_trace_occupancy();

}  // namespace uh
