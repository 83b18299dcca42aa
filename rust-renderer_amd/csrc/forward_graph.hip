// forward_graph.hip - the forward graph of include/utopian_hip.h (uh_render_forward, uh_read_forward, uh_get_forward_stats): shadow
// maps, forward pass, present. Host code over uh_ctx::Forward (context_state.h); it shares the hybrid graph's mesh tables, light table
// and shadow maps (hybrid_graph.hip, raster_driver.hip). Host-side counterpart of build_minimal_forward_render_graph
// (utopian/src/renderers/mod.rs).
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>

#include "graphs_internal.h"

// raster_scene, then forward.frag into forward_output
static int render_forward_pass(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view) {
   uh_ctx::Forward& f = c->fw;
   ForwardDev fd{};
   fd.color = f.color.p;
   uint32_t pieces = 0;
   if (int st = raster_scene(c, lc, view, f.bins, f.target, fd, "uh_render_forward", &pieces)) return st;
   light_and_shade(c, lc, view, fd, f.lights.p, false);
   f.pieces = pieces;
   f.lights_used = view.num_lights + 1;
   f.renders++;
   return UH_OK;
}

int uh_render_forward(uh_ctx* c, const UhViewUniformData* view, uint32_t mask) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_forward: null view");
   const bool render_maps = (mask & UH_FORWARD_SHADOW_MAPS) && view->shadows_enabled == 1;
   if (render_maps && !c->hy.sm.params_set)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_render_forward: UH_FORWARD_SHADOW_MAPS before uh_set_shadowmap_params (the cascades of uh_shadow_cascades or the caller's own)");
   if (mask & UH_FORWARD_PASS) {
      if (view->shadows_enabled == 1 && !c->hy.sm.size && !render_maps)
         return fail(c, UH_ERR_INVALID_ARGUMENT,
                     "uh_render_forward: the forward pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call "
                     "with UH_FORWARD_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0");
      if (view->num_lights > c->lights.size())
         return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_forward: view.num_lights exceeds the lights added with uh_add_light");
   }
   if (!c->built && c->topology_valid && view->rebuild_tlas == 1)
      if (int st = uh_refit_acceleration(c)) return st;
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_render_forward before uh_build_acceleration");
   if (c->W > 65535 || c->H > 65535) return fail(c, UH_ERR_CAPACITY, "uh_render_forward: a frame wider or taller than 65535 pixels");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Forward& f = c->fw;
   if (int st = hybrid_events(c)) return st;
   if (int st = hybrid_tables(c)) return st;
   const bool first = !f.color.p;
   if (first) {
      if (int st = stage_create(c, f.stage, 3)) return st;
      if (int st = alloc_group(c, [&](auto fn) { f.images((size_t)c->W * c->H, fn); })) return st;
   }
   if (mask & UH_FORWARD_PASS)
      if (int st = hybrid_light_table(c)) return st;
   if (int st = wait_frames_in_flight(c)) return st;
   LaunchCfg lc = cfg(c);
   lc.count_visits = false;  // nothing of this call goes to UhStats
   if (first) {
      ForwardDev cd{};
      forward_frame(c, f.target, cd);
      cd.color = f.color.p;
      launch_forward_clear(lc, cd, f.present.p);
   }
   for (auto& st : f.stage) st.ran = false;
   // setup_shadow_pass, setup_forward_pass, setup_present_pass (build_minimal_forward_render_graph): the maps are the hybrid graph's,
   // and their own record (uh_get_shadow_map_stats) is kept as a hybrid call with UH_HYBRID_SHADOW_MAPS keeps it
   if (render_maps) {
      Stage& hs = c->hy.stage[kStShadowMaps];
      hs.ran = false;
      if (int st = timed(c, {&f.stage[0], &hs}, [&] { return render_shadow_maps(c, lc, "uh_render_forward"); })) return st;
   }
   if (mask & UH_FORWARD_PASS)
      if (int st = timed(c, f.stage[1], [&] { return render_forward_pass(c, lc, *view); })) return st;
   if (mask & UH_FORWARD_PRESENT) {  // present.frag + FXAA on forward_output, into the forward graph's own image
      const HybridDev hd = hybrid_dev(c, *view, nullptr);
      HybridFrameDev pd = hybrid_frame_dev(c, *view);
      pd.deferred = f.color.p;
      pd.present = f.present.p;
      if (int st = timed(c, f.stage[2], [&] { launch_hybrid_present(lc, hd, pd); })) return st;
   }
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

int uh_read_forward(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Forward& f = c->fw;
   if (!f.color.p) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_forward before the first uh_render_forward");
   if (which < UH_FORWARD_OUTPUT || which > UH_FORWARD_PRESENT_OUTPUT) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_forward: image index must be 0..3");
   // image k's pixels and its bytes per pixel, in UH_FORWARD_* image order
   const std::pair<const void*, size_t> img[] = {{f.color.p, sizeof(float4)}, {f.target.depth.p, sizeof(float)}, {f.target.vis.p, sizeof(uint32_t)}, {f.present.p, sizeof(uchar4)}};
   return read_back(c, out, img[which].first, (size_t)c->W * c->H * img[which].second);
}

int uh_get_forward_stats(uh_ctx* c, UhForwardStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_forward_stats: null destination", c && c->fw.color.p, &st)) return st;
   uh_ctx::Forward& f = c->fw;
   for (int k = 0; k < 3; k++)
      if ((st = stage_ms(c, f.stage[k], &out->pass_ms[k]))) return st;
   out->renders = f.renders;
   if (f.stage[1].ran) {
      out->pieces = f.pieces;
      out->lights = f.lights_used;
      HIP_TRY(c, hipMemcpy(&out->covered_pixels, f.target.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   }
   return UH_OK;
}
