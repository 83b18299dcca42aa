// frame_plan.h - what the frame loop (frame_loop.hip) decides before it enqueues: which launches one sample pass of the path tracer
// is made of (plan_sample), how many frames one wavefront carries (plan_batch_size) and how a call's frames are split over its
// wavefronts (even_piece). Decided from plain values alone - the options, the frame's facts, whether the GPU is idle - no HIP call,
// no state changed: host code without HIP, which tests/cpp/frame_plan_check.cpp holds to its rules on the CPU.
#pragma once
#include <cstdint>

#include "utopian_hip.h"

namespace uh {

constexpr uint32_t kMaxBatchFrames = 32;  // frames one wavefront carries at most (FrameParams' per-frame arrays)
// frames of the reservoir passes one uh_render_frames wavefront carries at most (the ring of spatial buffers holds two such batches
// and the history slot: context_state.h kSpatialRing)
constexpr uint32_t kRestirBatch = 16;
constexpr uint32_t kFusedMaxPaths = 4u << 20;  // a lone frame of more paths than this is not fused (below)
// the cap on both traversal kernels' blocks per CU for a wavefront of one frame (fewer persistent waves reach the end of a small
// launch's tail sooner: round 4's sweep)
constexpr uint32_t kSingleFrameBlocksPerCu = 4;

struct SampleOptions {  // uh_set_option's, as the context holds them
   bool fused_bounces, fused_always, sun_verdicts, slim_state, overlap_miss, overlap_shadow;
   uint32_t closest_blocks_per_cu, shadow_blocks_per_cu;
   bool fused_primary = true;  // option "fused_primary"
};
struct SampleFacts {  // the frame's
   uint32_t batch_frames, num_bounces, samples_per_frame, n_owned, shard_cap;
   bool sun_shadow_enabled, lights_enabled;  // the view's flags == 1
   bool sun_grid, camera_grid;               // the sun grid / the camera grid serves this frame (CachedGrid::this_frame)
   bool primary_implicit = false;            // FrameParams::primary_implicit: bounce 0's state is not stored
   bool camera_lists_walked = false;         // no pixel's list is longer than the camera-grid kernel walks itself: none of its rays goes to the tree
   bool count_visits = false;                // option "count_visits": the walks count their node and triangle tests
   bool tile_partition = false;              // the rank traces the pixels of its tiles only (FrameParams::owned_pixels): path ids are not pixels
};
struct SamplePlan {
   bool fused;            // bounces 1.. run inside k_path_fused
   bool fused_sun0;       // bounce 0's sun rays inside the fused kernel too
   bool sun_verdicts;     // FrameParams::sun_verdicts
   bool slim_state;       // FrameParams::slim_state
   uint32_t closest_blocks_per_cu, shadow_blocks_per_cu;  // the options' figures under the lone frame's cap
   bool grid_primary;     // bounce 0's rays go through the camera grid (timed as kind 3), not the tree walk (kind 0)
   bool side_shadow;      // the shadow rays run on the side stream
   bool side_used;        // something runs on the side stream in every bounce
   bool join_side;        // the main stream waits for the side stream's work: before the fused kernel, or with fused_sun0 behind it
   uint32_t wave_bounces; // bounces the wavefront of launches runs
   bool flush;            // launch_flush_survivors runs
   bool fused_primary;    // bounce 0 is k_primary_shade: no k_generate, no camera-grid launch, no k_shade_hit(0)
};

// gpu_idle: the frame before this one has left the GPU (the caller asks per sample)
inline SamplePlan plan_sample(const SampleOptions& o, const SampleFacts& f, bool gpu_idle) {
   SamplePlan p;
   // a lone frame's launches are small: fewer persistent waves reach the end of their tails sooner
   const bool lone = f.batch_frames == 1;
   p.closest_blocks_per_cu = lone && o.closest_blocks_per_cu > kSingleFrameBlocksPerCu ? kSingleFrameBlocksPerCu : o.closest_blocks_per_cu;
   p.shadow_blocks_per_cu = lone && o.shadow_blocks_per_cu > kSingleFrameBlocksPerCu ? kSingleFrameBlocksPerCu : o.shadow_blocks_per_cu;
   // a lone frame: bounce 0 as a wavefront (its rays are coherent, the camera grid serves them), the others inside k_path_fused
   // ... when the caller waits for its frames (the frame before this one has left the GPU): the fused kernel fills the chip by
   // itself, so with frames in flight - a caller that does not wait - the wavefront's small launches interleave better (2.2 against
   // 2.5 ms per frame). Both give the same image.
   // ... and when the frame is not so large that its launches are wavefronts of a batch's size already (a 4K frame: 8.3 M paths -
   // the fused kernel 2.5 % behind on config 1, 12 % on config 3; at 1080p 12 % ahead, at 960 x 540 37 %, profiles/README.md)
   // (shard_cap < 2^23: the fused kernel's list entries keep a queue position in 23 bits, path_fused.hip)
   p.fused = o.fused_bounces && f.batch_frames == 1 && f.num_bounces >= 2 && f.num_bounces <= 64 && f.shard_cap < (1u << 23) &&
             ((gpu_idle && f.n_owned <= kFusedMaxPaths) || o.fused_always);
   p.fused_sun0 = p.fused && f.sun_shadow_enabled && !f.lights_enabled;
   // The sun rays leave verdicts, and the kernels that read a path's radiance next add its throughput (option "sun_verdicts") - when
   // the grid serves them (the tree walk of every sun ray keeps the read-modify-write: a plane to clear and an atomic per lit ray
   // otherwise), when no light ray adds to the same radiance behind them (the reference adds the sun's term first, rgen:63-122, and
   // float addition does not commute bit for bit) and when the wavefront runs every bounce (the fused kernel adds its own terms)
   p.sun_verdicts = o.sun_verdicts && f.sun_grid && f.sun_shadow_enabled && !f.lights_enabled && !p.fused;
   // The slim path state (option "slim_state", device_types.h PathState): where the verdicts hold no light sample rides with the path,
   // and with one sample per frame nothing reads the raygen RNG word behind bounce 0 - its place carries the path id
   p.slim_state = o.slim_state && p.sun_verdicts && f.samples_per_frame == 1;
   p.grid_primary = f.camera_grid;
   p.side_shadow = o.overlap_shadow && (f.sun_shadow_enabled || f.lights_enabled);
   p.side_used = p.side_shadow || o.overlap_miss;
   p.join_side = (o.overlap_miss || o.overlap_shadow) && f.num_bounces > 0;
   p.wave_bounces = p.fused ? 1u : f.num_bounces;
   // the paths still alive after the last bounce: their radiance (with what the last bounce's shadow rays added) goes to the
   // per-id array the tail reads
   // (slim state: the last bounce's sun kernels stood at those positions with the verdict in hand and stored it themselves)
   p.flush = f.num_bounces > 0 && !p.fused && !p.slim_state;
   // Bounce 0 in one kernel (option "fused_primary", kernels.hip k_primary_shade): where the three kernels of bounce 0 hand each other
   // nothing a lane at the pixel cannot compute - the camera grid serves the primary rays and none of them goes to the tree, their
   // state is implicit, and the slim state wants no id queue behind bounce 0 - and nobody counts the walk's tests. A rank of a tile
   // partition keeps the three kernels: its runs of 64 ids are not 64 neighbouring pixels, which the one kernel has not been measured
   // on. The slim state implies sun verdicts, which imply !fused: a lone frame that runs k_path_fused keeps the three kernels in front of it.
   p.fused_primary = o.fused_primary && p.grid_primary && f.primary_implicit && p.slim_state && f.camera_lists_walked && !f.count_visits && !f.tile_partition;
   return p;
}

// frames one wavefront carries for this pass mask: option "batch_frames" (0 = auto) over `owned` paths per frame (the pixels this
// rank traces; 0: a rank that owns none)
inline uint32_t plan_batch_size(uint32_t option, uint64_t owned, uint32_t pass_mask) {
   uint32_t batch = option;
   if (!batch) {
      // auto: about 32 M paths per wavefront (1080p: 16 frames, 4K: 4, a rank's eighth of 1080p: 32, 256 x 256: 32) - what
      // the launches need to fill the chip and amortise their tails; 1080p 4 / 8 / 12 / 16 frames = 6,271 / 6,341 / 6,388 /
      // 6,398 Mrays/s, the short paths of the iso-surface scene 4,974 / 5,393 / - / 6,223 (tools/sweep_batch.sh,
      // profiles/README.md) - within 33 M path-state records per slot (3.7 GB; path ids are dense over the pixels a rank
      // owns, so its wavefronts carry more frames than a whole frame's would)
      uint64_t b = (32u << 20) / (owned ? owned : 1), cap = (33u << 20) / (owned ? owned : 1);
      if (b > cap) b = cap;
      batch = (uint32_t)(b < 1 ? 1 : b);
   }
   if (batch > kMaxBatchFrames) batch = kMaxBatchFrames;
   if ((pass_mask & UH_PASS_RESTIR) && batch > kRestirBatch) batch = kRestirBatch;
   if (!(pass_mask & UH_PASS_REFERENCE_PT)) batch = 1;  // reservoir passes alone: frame by frame
   return batch;
}

// wavefronts of equal size: 20 frames at 16 per wavefront go as 10 + 10, not 16 + 4 (a short wavefront's launches are mostly tail).
// The frames of every piece but a shorter last one, for count >= 1 frames at batch >= 1 per wavefront.
inline uint32_t even_piece(uint32_t count, uint32_t batch) {
   const uint32_t n_batches = (count + batch - 1) / batch;
   return (count + n_batches - 1) / n_batches;
}

}  // namespace uh
