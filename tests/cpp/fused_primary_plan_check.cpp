// fused_primary_plan_check.cpp - SamplePlan::fused_primary (csrc/frame_plan.h, product code: csrc/frame_loop.hip launches k_primary_shade
// in place of k_generate, the camera-grid kernel and k_shade_hit(0) where it holds) on the host: from a pass that has it, each of its
// conditions taken away alone must take it away, and over the cross product of its inputs it holds where all of them do and nowhere
// else. The rule for a lone frame: fused_primary implies !fused - the slim state needs sun verdicts, which a pass with k_path_fused
// does not leave -, so a lone frame that runs k_path_fused keeps the three kernels of bounce 0 in front of it.
#include <cstdio>
#include <initializer_list>

#include "frame_plan.h"

using namespace uh;

static int g_failures = 0;

static void expect(bool ok, const char* what) {
   if (!ok) {
      if (g_failures < 40) std::printf("FAIL: %s\n", what);
      g_failures++;
   }
}

// the pass the benchmark times: 16 frames of 1080p, 5 bounces, one sample, sun on, lights off, both grids, every option at its default
static SampleOptions bench_options() { return SampleOptions{true, false, true, true, true, true, 6, 5, true}; }
static SampleFacts bench_facts() { return SampleFacts{16, 5, 1, 1920u * 1080u, 65536, true, false, true, true, true, true, false, false}; }

int main() {
   const SampleOptions o = bench_options();
   const SampleFacts f = bench_facts();
   expect(plan_sample(o, f, true).fused_primary && plan_sample(o, f, false).fused_primary, "the benchmark's pass has it");
   expect(plan_sample(o, f, true).slim_state && !plan_sample(o, f, true).fused, "... with the slim state, not fused");
   // one assertion per condition: taken away alone, it takes the plan away
   {
      SampleFacts g = f;
      g.camera_grid = false;
      expect(!plan_sample(o, g, true).fused_primary, "no camera grid (grid_primary): the three kernels");
   }
   {
      SampleFacts g = f;
      g.primary_implicit = false;
      expect(!plan_sample(o, g, true).fused_primary, "primary_implicit off: the three kernels");
   }
   {
      SampleOptions q = o;
      q.slim_state = false;
      expect(!plan_sample(q, f, true).fused_primary, "option slim_state off: the three kernels");
      SampleFacts g = f;
      g.samples_per_frame = 2;
      expect(!plan_sample(o, g, true).fused_primary, "two samples per frame (no slim state): the three kernels");
      g = f;
      g.lights_enabled = true;
      expect(!plan_sample(o, g, true).fused_primary, "lights enabled (no verdicts, no slim state): the three kernels");
      g = f;
      g.sun_grid = false;
      expect(!plan_sample(o, g, true).fused_primary, "no sun grid (no verdicts, no slim state): the three kernels");
   }
   {
      SampleFacts g = f;
      g.camera_lists_walked = false;
      expect(!plan_sample(o, g, true).fused_primary, "a pixel's list goes to the tree: the three kernels");
   }
   {
      SampleFacts g = f;
      g.count_visits = true;
      expect(!plan_sample(o, g, true).fused_primary, "count_visits on: the three kernels");
   }
   {
      SampleOptions q = o;
      q.fused_primary = false;
      expect(!plan_sample(q, f, true).fused_primary, "option fused_primary off: the three kernels");
   }
   {
      SampleFacts g = f;
      g.tile_partition = true;
      expect(!plan_sample(o, g, true).fused_primary, "a tile partition: the three kernels");
   }
   // a lone frame: k_path_fused when the GPU is idle (no fused_primary), the wavefront with frames in flight (fused_primary)
   {
      SampleFacts g = f;
      g.batch_frames = 1;
      expect(plan_sample(o, g, true).fused && !plan_sample(o, g, true).fused_primary, "a lone frame on an idle GPU: k_path_fused behind the three kernels");
      expect(!plan_sample(o, g, false).fused && plan_sample(o, g, false).fused_primary, "a lone frame with frames in flight: the wavefront, bounce 0 in one kernel");
   }
   // members left out of an initialiser list (code written before the plan had the field) never ask for it
   expect(!plan_sample(o, SampleFacts{16, 5, 1, 1920u * 1080u, 65536, true, false, true, true}, true).fused_primary, "facts without the new members: the three kernels");

   // the cross product: it holds exactly where every condition does, and never with fused
   unsigned long long plans = 0, held = 0;
   for (uint32_t bits = 0; bits < (1u << 14); bits++) {
      const auto bit = [&](int k) { return ((bits >> k) & 1u) != 0; };
      for (uint32_t batch = 1; batch <= 2; batch++)
         for (uint32_t nb : {0u, 1u, 2u, 5u})
            for (uint32_t spp = 1; spp <= 2; spp++) {
               const SampleOptions q{bit(0), bit(1), bit(2), bit(3), true, true, 6, 5, bit(4)};
               const SampleFacts g{batch, nb, spp, 64u * 48u, 4096, bit(5), bit(6), bit(7), bit(8), bit(9), bit(10), bit(11), bit(12)};
               const SamplePlan p = plan_sample(q, g, bit(13));
               const bool all = q.fused_primary && p.grid_primary && g.camera_grid && g.primary_implicit && p.slim_state && g.camera_lists_walked && !g.count_visits && !g.tile_partition;
               expect(p.fused_primary == all, "fused_primary iff all of its conditions");
               if (p.fused_primary) expect(!p.fused && !p.fused_sun0 && p.sun_verdicts && !p.flush && g.samples_per_frame == 1 && !g.lights_enabled, "fused_primary implies a slim pass without k_path_fused");
               plans++;
               held += p.fused_primary ? 1 : 0;
            }
   }
   expect(held > 0 && held < plans, "the cross product has passes of both kinds");
   if (g_failures) {
      std::printf("FUSED PRIMARY PLAN CHECK FAILED: %d\n", g_failures);
      return 1;
   }
   std::printf("FUSED PRIMARY PLAN CHECK OK (%llu plans, %llu with fused_primary)\n", plans, held);
   return 0;
}
