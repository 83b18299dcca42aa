// frame_plan_check.cpp - the frame loop's decisions (csrc/frame_plan.h, product code: what csrc/frame_loop.hip enqueues follows them)
// on the host, under ASan + UBSan (tests/test_sanitizers.py): the plan of a sample pass over the cross product of its inputs, every
// output against its rule written a second way - a truth table over the values enumerated here, or implications -, the batch size
// against the figures in the comment of plan_batch_size, and the even split of a call's frames.
#include <cstdio>
#include <string>
#include <vector>

#include "frame_plan.h"

using namespace uh;

static int g_failures = 0;

static void expect(bool ok, const std::string& what) {
   if (!ok) {
      if (g_failures < 40) std::printf("FAIL: %s\n", what.c_str());
      g_failures++;
   }
}

static std::string show(const SampleOptions& o, const SampleFacts& f, bool idle) {
   char buf[256];
   std::snprintf(buf, sizeof(buf), " [opt fused %d always %d verdicts %d slim %d miss %d shadow %d blocks %u/%u | batch %u bounces %u spp %u owned %u cap %u sun %d lights %d sun_grid %d cam_grid %d | idle %d]",
                 o.fused_bounces, o.fused_always, o.sun_verdicts, o.slim_state, o.overlap_miss, o.overlap_shadow, o.closest_blocks_per_cu, o.shadow_blocks_per_cu, f.batch_frames,
                 f.num_bounces, f.samples_per_frame, f.n_owned, f.shard_cap, f.sun_shadow_enabled, f.lights_enabled, f.sun_grid, f.camera_grid, idle);
   return buf;
}

// the bounces enumerated below: which of them the fused kernel takes
static bool fusable_bounces(uint32_t b) {
   switch (b) {
      case 2: case 64: return true;
      default: return false;  // 0, 1: nothing to fuse; 65: more than a list entry's bounce field counts
   }
}

static bool same(const SamplePlan& a, const SamplePlan& b) {
   return a.fused == b.fused && a.fused_sun0 == b.fused_sun0 && a.sun_verdicts == b.sun_verdicts && a.slim_state == b.slim_state &&
          a.closest_blocks_per_cu == b.closest_blocks_per_cu && a.shadow_blocks_per_cu == b.shadow_blocks_per_cu && a.grid_primary == b.grid_primary &&
          a.side_shadow == b.side_shadow && a.side_used == b.side_used && a.join_side == b.join_side && a.wave_bounces == b.wave_bounces && a.flush == b.flush;
}

static void check_sample(const SampleOptions& o, const SampleFacts& f, bool idle) {
   const SamplePlan p = plan_sample(o, f, idle);
   const auto expect = [&](bool ok, const char* what) {
      if (!ok) ::expect(false, what + show(o, f, idle));
   };

   // fused: the table, condition by condition
   bool fused = true;
   if (!o.fused_bounces) fused = false;
   if (f.batch_frames == 2) fused = false;
   if (!fusable_bounces(f.num_bounces)) fused = false;
   if (f.shard_cap == (1u << 23)) fused = false;
   if (!o.fused_always) {
      if (!idle) fused = false;
      if (f.n_owned == kFusedMaxPaths + 1) fused = false;
   }
   expect(p.fused == fused, "fused");
   // fused implies one frame per batch and 2..64 bounces
   if (p.fused) expect(f.batch_frames == 1 && f.num_bounces >= 2 && f.num_bounces <= 64, "fused implies a lone frame of 2..64 bounces");

   // fused_sun0 implies fused; within fused it is "sun rays and no light rays"
   if (p.fused_sun0) expect(p.fused, "fused_sun0 implies fused");
   if (p.fused) expect(p.fused_sun0 == (f.sun_shadow_enabled ? !f.lights_enabled : false), "fused_sun0 of a fused frame");

   // sun_verdicts: all five of its conditions and nothing less
   const int held = (o.sun_verdicts ? 1 : 0) + (f.sun_grid ? 1 : 0) + (f.sun_shadow_enabled ? 1 : 0) + (f.lights_enabled ? 0 : 1) + (p.fused ? 0 : 1);
   expect(p.sun_verdicts == (held == 5), "sun_verdicts");
   if (p.sun_verdicts) expect(!p.fused && f.sun_grid, "sun_verdicts implies not fused and the sun grid");

   // slim_state implies sun_verdicts and one sample per frame; with the option on, those two suffice
   if (p.slim_state) expect(p.sun_verdicts && f.samples_per_frame == 1 && o.slim_state, "slim_state implies sun_verdicts, one sample, the option");
   if (o.slim_state && p.sun_verdicts && f.samples_per_frame == 1) expect(p.slim_state, "slim_state where nothing forbids it");

   // the wavefront's bounces and the flush
   expect(p.wave_bounces == (p.fused ? 1u : f.num_bounces), "wave_bounces");
   bool flush = true;
   if (f.num_bounces == 0 || p.fused || p.slim_state) flush = false;
   expect(p.flush == flush, "flush iff bounces > 0, not fused, not slim");

   // the block caps: a lone frame only, never a raise
   const uint32_t given[2] = {o.closest_blocks_per_cu, o.shadow_blocks_per_cu}, got[2] = {p.closest_blocks_per_cu, p.shadow_blocks_per_cu};
   for (int k = 0; k < 2; k++) {
      expect(got[k] <= given[k], "a cap never raises a figure");
      if (f.batch_frames != 1) expect(got[k] == given[k], "no cap on a batch");
      if (f.batch_frames == 1) expect(got[k] == (given[k] >= 5 ? kSingleFrameBlocksPerCu : given[k]), "a lone frame's cap");  // (given: 3..6, the cap 4)
   }

   // the side stream
   expect(p.grid_primary == f.camera_grid, "grid_primary");
   bool side_shadow = false;
   if (o.overlap_shadow && f.sun_shadow_enabled) side_shadow = true;
   if (o.overlap_shadow && f.lights_enabled) side_shadow = true;
   expect(p.side_shadow == side_shadow, "side_shadow");
   expect(p.side_used == !(!p.side_shadow && !o.overlap_miss), "side_used");
   bool join = true;
   if (f.num_bounces == 0) join = false;
   if (!o.overlap_miss && !o.overlap_shadow) join = false;
   expect(p.join_side == join, "join_side");
   if (p.side_used && f.num_bounces > 0) expect(p.join_side, "a side stream that was used is joined");

   // with fused_always neither gpu_idle nor n_owned matters
   if (o.fused_always) {
      SampleFacts g = f;
      g.n_owned = f.n_owned == kFusedMaxPaths ? kFusedMaxPaths + 1 : kFusedMaxPaths;
      expect(same(p, plan_sample(o, f, !idle)) && same(p, plan_sample(o, g, idle)) && same(p, plan_sample(o, g, !idle)), "fused_always: gpu_idle and n_owned do not matter");
   }
}

static uint64_t check_samples() {
   static_assert(kSingleFrameBlocksPerCu == 4, "the blocks enumerated below straddle the cap");
   const uint32_t blocks[4][2] = {{5, 5}, {6, 3}, {3, 6}, {4, 4}};
   const uint32_t bounces[5] = {0, 1, 2, 64, 65};
   uint64_t n = 0;
   for (uint32_t bits = 0; bits < (1u << 11); bits++) {
      const auto bit = [&](int k) { return ((bits >> k) & 1u) != 0; };
      for (const auto& bl : blocks)
         for (uint32_t batch = 1; batch <= 2; batch++)
            for (uint32_t nb : bounces)
               for (uint32_t spp = 1; spp <= 2; spp++)
                  for (uint32_t owned : {kFusedMaxPaths, kFusedMaxPaths + 1})
                     for (uint32_t cap : {(1u << 23) - 64, 1u << 23}) {
                        const SampleOptions o{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bl[0], bl[1]};
                        const SampleFacts f{batch, nb, spp, owned, cap, bit(6), bit(7), bit(8), bit(9)};
                        check_sample(o, f, bit(10));
                        n++;
                     }
   }
   return n;
}

static void check_batch_size() {
   const uint32_t pt = UH_PASS_REFERENCE_PT, all = UH_PASS_ALL;
   expect(plan_batch_size(0, 1920ull * 1080, pt) == 16, "auto: 1920 x 1080 carries 16 frames");
   expect(plan_batch_size(0, 3840ull * 2160, pt) == 4, "auto: 3840 x 2160 carries 4");
   expect(plan_batch_size(0, 256ull * 256, pt) == kMaxBatchFrames, "auto: 256 x 256 lands on kMaxBatchFrames");
   expect(plan_batch_size(0, 1920ull * 1080 / 8, pt) == kMaxBatchFrames, "auto: a rank's eighth of 1080p lands on kMaxBatchFrames");
   expect(plan_batch_size(0, 8192ull * 8192, pt) == 1, "auto: a frame of more paths than a wavefront's share still goes, alone");
   expect(plan_batch_size(0, 0, pt) == kMaxBatchFrames, "owned = 0 does not divide by zero");
   // a mask with UH_PASS_RESTIR never exceeds kRestirBatch; without UH_PASS_REFERENCE_PT it is 1; an explicit value is kept up to the caps
   for (uint32_t option = 0; option <= 2 * kMaxBatchFrames; option++)
      for (uint64_t owned : {0ull, 64ull, 256ull * 256, 1920ull * 1080, 3840ull * 2160})
         for (uint32_t mask = 0; mask <= all; mask++) {
            const uint32_t b = plan_batch_size(option, owned, mask);
            const auto expect = [&](bool ok, const char* what) {
               if (!ok) ::expect(false, what + (" [option " + std::to_string(option) + " owned " + std::to_string(owned) + " mask " + std::to_string(mask) + "]"));
            };
            expect(b >= 1 && b <= kMaxBatchFrames, "1 <= batch <= kMaxBatchFrames");
            if (mask & UH_PASS_RESTIR) expect(b <= kRestirBatch, "reservoir passes: at most kRestirBatch");
            if (!(mask & pt)) expect(b == 1, "reservoir passes alone: frame by frame");
            if (option && mask == pt) expect(b == (option > kMaxBatchFrames ? kMaxBatchFrames : option), "an explicit value is kept up to kMaxBatchFrames");
            if (option && mask == all) expect(b == (option > kRestirBatch ? kRestirBatch : option), "an explicit value is kept up to kRestirBatch");
         }
}

// the pieces uh_render_frames renders: `even` frames each until fewer are left
static std::vector<uint32_t> pieces_of(uint32_t count, uint32_t batch) {
   std::vector<uint32_t> out;
   const uint32_t even = even_piece(count, batch);
   for (uint32_t done = 0; done < count; done += out.back()) out.push_back(count - done < even ? count - done : even);
   return out;
}

static void check_split() {
   expect(pieces_of(20, 16) == std::vector<uint32_t>({10, 10}), "20 frames at 16 go as 10 + 10");
   for (uint32_t count = 1; count <= 100; count++)
      for (uint32_t batch = 1; batch <= 32; batch++) {
         const std::vector<uint32_t> p = pieces_of(count, batch);
         const auto expect = [&](bool ok, const char* what) {
            if (!ok) ::expect(false, what + (" [count " + std::to_string(count) + " batch " + std::to_string(batch) + "]"));
         };
         uint32_t sum = 0;
         bool sized = true, even = true;
         for (size_t k = 0; k < p.size(); k++) {
            sum += p[k];
            sized = sized && p[k] >= 1 && p[k] <= batch;
            if (k + 1 < p.size()) even = even && p[k] == p[0];  // all but the last are equal ...
         }
         even = even && p.back() <= p[0];                       // ... and the last is no longer
         expect(sum == count, "the pieces sum to count");
         expect(sized, "no piece is empty or exceeds the batch");
         expect(even, "the pieces differ by at most one, except a shorter last piece");
         expect(p.size() == (count + batch - 1) / batch, "as few wavefronts as the batch allows");
      }
}

int main() {
   const uint64_t plans = check_samples();
   check_batch_size();
   check_split();
   if (g_failures) {
      std::printf("FRAME PLAN CHECK FAILED: %d\n", g_failures);
      return 1;
   }
   std::printf("FRAME PLAN CHECK OK (%llu sample plans)\n", (unsigned long long)plans);
   return 0;
}
