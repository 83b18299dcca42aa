// options.hip — uh_set_option: the run-time switches of a context. Host code only; struct uh_ctx is context_state.h.
#include <hip/hip_runtime.h>

#include <string>

#include "context_state.h"
#include "utopian_hip.h"

using namespace uh;

extern "C" {

// The options (33): DESIGN.md section 7 has the table with defaults and what was measured. Variants that two rounds of measurements
// left behind (batch traversal kernels, wave-per-tile primary rays, sub-frame interleave, the fused coarse-cover look-up, spatial
// splits, insertion-based tree optimisation, the host-thread grid build) were removed in round 5 together with their options.
int uh_set_option(uh_ctx* c, const char* name, int value) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!name) return fail(c, UH_ERR_INVALID_ARGUMENT, "null option name");
   const std::string n(name);
   auto range = [&](int lo, int hi) { return value >= lo && value <= hi; };
   auto bad = [&](const char* what) { return fail(c, UH_ERR_INVALID_ARGUMENT, n + " " + what); };
   // ---- diagnostics
   if (n == "count_visits")
      c->count_visits = value != 0;
   else if (n == "time_kernels") {
      if (c->time_kernels && !value) {
         (void)sync_all(c);
         drain_timed(c);
      }
      c->time_kernels = value != 0;
   }
   // ---- the tree
   else if (n == "device_build") {
      // 0 = host SAH builder; 1 = device build, PLOC under a host SAH top; 2 = device build, radix tree
      if (!range(0, 2)) return bad("must be 0, 1 (PLOC) or 2 (radix tree)");
      if (c->device_build != (value != 0) || (value && c->device_build_kind != (uint32_t)value)) c->built = c->topology_valid = false;
      c->device_build = value != 0;
      if (value) c->device_build_kind = (uint32_t)value;
   } else if (n == "ploc_sah_top") {
      if (!range(0, 1 << 20)) return bad("must be 0..1048576");
      if (c->ploc_sah_top != (uint32_t)value && c->device_build) c->built = c->topology_valid = false;
      c->ploc_sah_top = (uint32_t)value;
   }
   // ---- the sun grid (sun_grid.h): every change takes effect with the next grid that is built
   else if (n == "sun_grid")
      c->sun_grid_enabled = value != 0;  // 0: the sun shadow rays always walk the tree
   else if (n == "sun_grid_build") {
      c->sun_x.device_build = value != 0;  // 1: built on the device (sun_grid_build.hip); 0: by the host builder (sun_grid.cpp, the reference implementation)
      c->sun.cache.invalidate();
   } else if (n == "sun_grid_density") {
      if (!range(1, 4096)) return bad("(entries per triangle) must be 1..4096");
      c->sun.limits.entries_per_triangle = (double)value;
      c->sun.cache.invalidate();
   } else if (n == "sun_grid_max_walk") {
      if (!range(1, 4096)) return bad("(longest list a ray tests itself) must be 1..4096");
      c->sun.limits.max_walk = (uint32_t)value;
      c->sun.cache.invalidate();
   } else if (n == "sun_grid_max_mb") {
      if (!range(1, 65536)) return bad("must be 1..65536");
      c->sun.limits.max_entries = ((uint64_t)value << 20) / sizeof(SunGridEntry);
      c->sun.cache.invalidate();
   } else if (n == "sun_grid_force") {
      // 1: the grid is never refused for what it would be worth (more than 12 entries per occupied cell, more than a fifth of the scene's
      // surface handed to the tree): tests and studies of scenes the defaults would refuse; 0: the defaults
      const SunGridLimits defaults;
      c->sun.limits.max_mean_list = value ? 1e30 : defaults.max_mean_list;
      c->sun.limits.max_fallback_area = value ? 2.0 : defaults.max_fallback_area;
      c->sun.cache.invalidate();
   } else if (n == "sun_grid_inline_max_mb") {
      // the lists a second time as 64-byte records that carry their packet (one round trip per triangle test instead of two): memory budget
      // in MB; -1 (default) = four times the packet array; 0 = never
      if (!range(-1, 1 << 20)) return bad("must be -1 (auto: 4 x the packet array), 0 (off) .. 1048576");
      c->sun_x.inline_max_mb = value;
      c->sun.cache.invalidate();
   } else if (n == "sun_verdicts")
      // 1: the grid's sun kernels leave one bit per ray and the next shading kernel (or the flush) adds the lit paths' throughput to
      // their radiance; 0: the sun kernels add it themselves. Same images; frames with lights enabled always take the second form
      c->sun_x.verdicts = value != 0;
   else if (n == "slim_state")
      // 1: a pass with sun verdicts and one sample per frame carries the slim path state (device_types.h PathState); 0: never
      c->slim_state = value != 0;
   else if (n == "sun_grid_coarse") {
      // the coarse cover (sun_grid.h): one depth per block of 2^value x 2^value cells, asked before the cell's own record; 0: none
      if (!range(0, 6)) return bad("(log2 of the block edge in cells) must be 0..6");
      c->sun_x.coarse_shift = (uint32_t)value;
      c->sun.cache.invalidate();
   }
   // ---- the camera grid
   else if (n == "camera_grid")
      c->cam_grid_enabled = value != 0;  // 0: the primary rays always walk the tree
   else if (n == "camera_grid_max_walk") {
      if (!range(1, 4096)) return bad("must be 1..4096");
      c->cam.limits.max_walk = (uint32_t)value;
      c->cam.cache.invalidate();
   } else if (n == "camera_grid_walk_whole") {
      // lists of up to this many packets are walked whole by the grid kernel (those beyond camera_grid_max_walk are not sorted: no early
      // exit) instead of handing the ray to the tree; 0: every list beyond camera_grid_max_walk goes to the tree
      if (!range(0, 65536)) return bad("must be 0..65536");
      c->cam_walk_whole = (uint32_t)value;
      c->cam.cache.invalidate();
   } else if (n == "camera_grid_max_mean_list_x10") {
      if (!range(1, 100000)) return bad("must be 1..100000");
      c->cam.limits.max_mean_list = value / 10.0;
      c->cam.cache.invalidate();
   } else if (n == "primary_implicit")
      c->primary_implicit = value != 0;  // 0: bounce 0's state planes are stored by k_generate even when the camera grid is in use
   else if (n == "fused_primary")
      // 1: where the plan allows it (frame_plan.h SamplePlan::fused_primary) bounce 0 is one kernel, k_primary_shade; 0: always k_generate,
      // the camera-grid kernel and k_shade_hit(0). Same images
      c->fused_primary = value != 0;
   // ---- what the frames compute
   else if (n == "full_frame_restir")
      c->full_frame_restir = value != 0;
   else if (n == "iso_reference_triangulation")
      c->iso_reference = value != 0;
   else if (n == "furnace")
      c->furnace = value != 0;  // applies to the frames enqueued from now on
   else if (n == "rtao_order") {
      // how the rtao trace kernel lays out its work (rtao.hip; same counts whichever): 0 (default) one ray per item, a pixel's samples
      // together; 1 one ray per item, one sample of consecutive pixels together; 2 one pixel per item, its lane walks the samples
      if (!range(0, 2)) return bad("must be 0..2");
      c->hy.ao.order = (uint32_t)value;
   }
   else if (n == "rtgi_order") {
      // how the rtgi closest-hit kernel lays out its work (rtgi.hip; same images whichever): 0 (default) a pixel's samples together;
      // 1 one sample of consecutive pixels together
      if (!range(0, 1)) return bad("must be 0 or 1");
      c->hy.gi.order = (uint32_t)value;
   }
   else if (n == "area_light_order") {
      // how the area-light sample kernel lays out its work (area_lights.hip; same images whichever): 0 (default) a pixel's samples
      // together; 1 one sample of consecutive pixels together
      if (!range(0, 1)) return bad("must be 0 or 1");
      c->hy.area.order = (uint32_t)value;
   }
   else if (n == "fog_order") {
      // how the fog trace kernel lays out its work (fog.hip; same masks whichever): 0 one sample per item, a pixel's samples together;
      // 1 one sample per item, one sample index of consecutive pixels together; 2 (default, measured fastest) one pixel per item, its
      // lane walks the samples
      if (!range(0, 2)) return bad("must be 0..2");
      c->hy.fog.order = (uint32_t)value;
   }
   else if (n == "texture_blocks")
      // 1: the textures added from now on are stored as overlapped blocks, a bilinear footprint in one cache line (texture_layout.h);
      // 0: as 8x8 tiles, or rows. Same images bit for bit: the same four texel words enter the filter
      c->texture_blocks = value != 0;
   else if (n == "shadow_map_size") {
      if (!range(16, 8192)) return bad("must be 16..8192");
      if ((uint32_t)value != c->shadow_map_size) {  // the maps go: the deferred pass with shadows is refused until they are rendered again
         if (int st = sync_all(c)) return st;
         c->hy.sm.destroy();
         c->hy.sm.bins.geom = 0;
         c->hy.sm.size = 0;
      }
      c->shadow_map_size = (uint32_t)value;
   }
   // ---- how the frames are scheduled
   else if (n == "overlap")
      c->overlap_miss = c->overlap_shadow = value != 0;  // k_shade_miss and the shadow traversals on the slot's side stream
   else if (n == "batch_frames") {
      if (!range(0, (int)kMaxBatchFrames)) return bad("must be 0 (auto) .. 32");
      c->batch_frames = (uint32_t)value;
   } else if (n == "frames_in_flight") {
      if (!range(1, (int)kMaxSlots)) return bad("must be 1..8");
      (void)sync_all(c);
      c->frames_in_flight = (uint32_t)value;
      c->next_slot = 0;
   } else if (n == "fused_bounces") {
      // 0: a lone frame runs the wavefront of a batch (four launches per bounce); 1: its bounces 1 .. in one persistent kernel; 2..8: that
      // kernel's blocks per CU
      if (!range(-1, 8)) return bad("must be 0 (off), 1 (on when no frame is in flight), -1 (always on) or 2..8 (as 1, and blocks per CU of its grid)");
      c->fused_bounces = value != 0;
      c->fused_always = value == -1;
      if (value >= 2) c->fused_blocks_per_cu = (uint32_t)value;
   } else if (n == "trace_blocks_per_cu") {
      if (!range(1, 8)) return bad("must be 1..8");
      c->closest_blocks_per_cu = c->shadow_blocks_per_cu = (uint32_t)value;  // persistent grids of the traversal kernels
   } else
      return fail(c, UH_ERR_INVALID_ARGUMENT, "unknown option: " + n);
   return UH_OK;
}

}  // extern "C"
