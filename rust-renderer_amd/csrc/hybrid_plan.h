// hybrid_plan.h - what uh_render_hybrid (hybrid_graph.hip) decides before it touches the device: the passes a call runs and the
// first-use groups they need, or the message of the first rule the request breaks, the rules in the order utopian_hip.h gives them.
// Decided from plain values alone - the context's facts, the view and the mask - no HIP call, no state changed: host code without
// HIP, which tests/cpp/hybrid_plan_check.cpp holds to its rules and their order on the CPU.
#pragma once
#include <cstdint>

#include "utopian_hip.h"

namespace uh {

struct HybridFacts {  // the context's, as hybrid_facts (hybrid_graph.hip) reads them
   uint32_t W, H, world;                  // the frame; the row partition's world (uh_set_restir_partition)
   uint64_t lights;                       // uh_add_light calls
   bool has_mesh, restir_recorded;        // the scene has a mesh; a reservoir pass has run
   bool maps_built;                       // a call with UH_HYBRID_ENVIRONMENT has built the IBL maps
   bool cascades_set, cascades_rendered;  // uh_set_shadowmap_params has been called; the cascaded shadow maps exist
   bool gbuffer_done, motion_last;        // a G-buffer pass has been enqueued; the last one had UH_HYBRID_MOTION
   uint32_t taa_flags;                    // UhTaaParams::flags as set
   bool rt_images, frame_images;          // the ray-traced images, the final frame's images exist
};

struct HybridPlan {
   int code;             // UH_OK, or what the call returns with `refusal`
   const char* refusal;
   bool raster, maps, render_maps, restir, rtao, rtgi, glossy, glass, fog, mc, motion, rt, taa, post;  // maps: the IBL maps exist for this call's consumers
   bool deferred, frame, env;  // the deferred pass runs; the final frame's images and the IBL maps are needed
   bool first, frame_first;    // the ray-traced images, the final frame's images are allocated by this call (and cleared)
   bool area;                  // the area-light pass (UH_HYBRID_AREA_LIGHTS) runs, behind the deferred pass
};

// What a pass that casts rays from the G-buffer asks of a call, in the order it is asked (a null message: not asked): the view's
// raytracing_supported = 1; a G-buffer, this call's or an earlier one's; ibl_enabled other than 1; the bits of `with` all in the same
// call; none of `never`; fewer than 2^32 rays at rays_per_pixel (UH_ERR_CAPACITY; every other refusal is UH_ERR_INVALID_ARGUMENT).
// Every message is one literal: a text search for it finds its row.
struct RayPassRules {
   uint32_t bit;
   const char *raytracing, *gbuffer, *ibl;
   uint32_t with;
   const char* without;
   uint32_t never;
   const char* together;
   uint32_t rays_per_pixel;
   const char* capacity;
};
constexpr RayPassRules kRestirLightsRules = {
   UH_HYBRID_RESTIR_LIGHTS,
   "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts shadow rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   nullptr, 0, nullptr, 0, nullptr, 0, nullptr};
constexpr RayPassRules kRtaoRules = {
   UH_HYBRID_RTAO,
   "uh_render_hybrid: UH_HYBRID_RTAO casts occlusion rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_RTAO casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   nullptr, 0, nullptr, 0, nullptr, 64, "uh_render_hybrid: UH_HYBRID_RTAO: a frame of 2^26 pixels or more (its rays are numbered in 32 bits)"};
constexpr RayPassRules kRtgiRules = {
   UH_HYBRID_RTGI,
   "uh_render_hybrid: UH_HYBRID_RTGI casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_RTGI casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   "uh_render_hybrid: UH_HYBRID_RTGI with view.ibl_enabled = 1: the IBL ambient term and this pass would both count the sky; set ibl_enabled = 0, or clear the bit",
   UH_HYBRID_DEFERRED,
   "uh_render_hybrid: UH_HYBRID_RTGI without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass writes and has nothing to add to; set UH_HYBRID_DEFERRED",
   0, nullptr, 16, "uh_render_hybrid: UH_HYBRID_RTGI: a frame of 2^28 pixels or more (its rays are numbered in 32 bits)"};
constexpr RayPassRules kGlossyRules = {
   UH_HYBRID_GLOSSY,
   "uh_render_hybrid: UH_HYBRID_GLOSSY casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_GLOSSY casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   "uh_render_hybrid: UH_HYBRID_GLOSSY with view.ibl_enabled = 1: the IBL specular term and this pass would both count the sky; set ibl_enabled = 0, or clear the bit",
   UH_HYBRID_DEFERRED,
   "uh_render_hybrid: UH_HYBRID_GLOSSY without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass writes and has nothing to add to; set UH_HYBRID_DEFERRED",
   0, nullptr, 16, "uh_render_hybrid: UH_HYBRID_GLOSSY: a frame of 2^28 pixels or more (its rays are numbered in 32 bits)"};
constexpr RayPassRules kFogRules = {
   UH_HYBRID_FOG,
   "uh_render_hybrid: UH_HYBRID_FOG casts sun rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_FOG marches to the G-buffer's positions, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   nullptr, UH_HYBRID_DEFERRED | UH_HYBRID_SKY,
   "uh_render_hybrid: UH_HYBRID_FOG without UH_HYBRID_DEFERRED and UH_HYBRID_SKY in the same call: the pass attenuates what those two write and has nothing to attenuate; set both",
   UH_HYBRID_MARCHING_CUBES,
   "uh_render_hybrid: UH_HYBRID_FOG with UH_HYBRID_MARCHING_CUBES in the same call: the marching-cubes pass's pixels are not in the G-buffer the fog marches to; clear one of the two bits",
   64, "uh_render_hybrid: UH_HYBRID_FOG: a frame of 2^26 pixels or more (its rays are numbered in 32 bits)"};
constexpr RayPassRules kGlassRules = {
   UH_HYBRID_GLASS,
   "uh_render_hybrid: UH_HYBRID_GLASS casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_GLASS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   nullptr, UH_HYBRID_DEFERRED,
   "uh_render_hybrid: UH_HYBRID_GLASS without UH_HYBRID_DEFERRED in the same call: the pass replaces what the deferred pass writes on dielectric pixels and has nothing to write into; set UH_HYBRID_DEFERRED",
   0, nullptr, 32, "uh_render_hybrid: UH_HYBRID_GLASS: a frame of 2^27 pixels or more (its rays are numbered in 32 bits)"};
constexpr RayPassRules kAreaLightRules = {
   UH_HYBRID_AREA_LIGHTS,
   "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS casts shadow rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   nullptr, UH_HYBRID_DEFERRED,
   "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass writes and has nothing to add to; set UH_HYBRID_DEFERRED",
   0, nullptr, 16, "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS: a frame of 2^28 pixels or more (its samples are numbered in 32 bits)"};

// true when the request breaks one of r's rules: the first of them, in the order above, into p
inline bool ray_pass_refused(const RayPassRules& r, const HybridFacts& f, const UhViewUniformData& view, uint32_t mask, HybridPlan& p) {
   p.refusal = view.raytracing_supported != 1                                           ? r.raytracing
               : !(mask & UH_HYBRID_GBUFFER) && !f.gbuffer_done                         ? r.gbuffer
               : r.ibl && view.ibl_enabled == 1                                         ? r.ibl
               : (mask & r.with) != r.with                                              ? r.without
               : (mask & r.never)                                                       ? r.together
               : r.capacity && (uint64_t)f.W * f.H * r.rays_per_pixel >= (1ull << 32)   ? r.capacity
                                                                                        : nullptr;
   p.code = !p.refusal ? UH_OK : p.refusal == r.capacity ? UH_ERR_CAPACITY : UH_ERR_INVALID_ARGUMENT;
   return p.refusal != nullptr;
}

inline HybridPlan hybrid_plan(const HybridFacts& f, const UhViewUniformData& view, uint32_t mask) {
   HybridPlan p{};
   const auto refuse = [&p](const char* why) {  // (but for a pass's capacity, every refusal is UH_ERR_INVALID_ARGUMENT)
      p.code = UH_ERR_INVALID_ARGUMENT, p.refusal = why;
      return p;
   };
   p.raster = (mask & UH_HYBRID_GBUFFER_RASTER) != 0;
   if (p.raster && !(mask & UH_HYBRID_GBUFFER))
      return refuse("uh_render_hybrid: UH_HYBRID_GBUFFER_RASTER without UH_HYBRID_GBUFFER (the bit chooses how the G-buffer pass runs); set both, or neither");
   // the IBL maps exist for this call's consumers when an earlier call built them or this one does, before rt_reflections
   p.maps = f.maps_built || (mask & UH_HYBRID_ENVIRONMENT);
   if ((mask & UH_HYBRID_RT_REFLECTIONS) && view.ibl_enabled == 1 && !p.maps)
      return refuse("uh_render_hybrid: rt_reflections with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), which are not part of this library until a call with UH_HYBRID_ENVIRONMENT builds them; set that bit, or ibl_enabled = 0 for the reflection pass's non-IBL branch");
   p.render_maps = (mask & UH_HYBRID_SHADOW_MAPS) && view.shadows_enabled == 1;
   if (p.render_maps && !f.cascades_set)
      return refuse("uh_render_hybrid: UH_HYBRID_SHADOW_MAPS before uh_set_shadowmap_params (the cascades of uh_shadow_cascades or the caller's own)");
   if (mask & UH_HYBRID_DEFERRED) {
      if (view.shadows_enabled == 1 && !f.cascades_rendered && !p.render_maps)
         return refuse("uh_render_hybrid: the deferred pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call with UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0 for the rt_shadows branch");
      if (view.ibl_enabled == 1 && !p.maps)
         return refuse("uh_render_hybrid: the deferred pass with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), which a call with UH_HYBRID_ENVIRONMENT builds; set that bit, or ibl_enabled = 0 for the ambient term 0.03 * diffuse * occlusion");
      if (view.num_lights > f.lights)
         return refuse("uh_render_hybrid: view.num_lights exceeds the lights added with uh_add_light");
   }
   if ((mask & UH_HYBRID_SKY) && view.cubemap_enabled == 1 && !p.maps)
      return refuse("uh_render_hybrid: the sky pass with view.cubemap_enabled = 1 needs the environment cube (ibl.rs), which a call with UH_HYBRID_ENVIRONMENT builds; set that bit, or cubemap_enabled = 0 for the IntegrateScattering branch");
   // the reservoir lights: one shadow ray per pixel toward the light of its spatial reservoir, which the deferred pass then adds
   p.restir = (mask & UH_HYBRID_RESTIR_LIGHTS) != 0;
   if (p.restir) {
      if (ray_pass_refused(kRestirLightsRules, f, view, mask, p)) return p;
      if (!f.restir_recorded)
         return refuse("uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS reads the spatial reservoirs, and no reservoir pass has run on this context; render a frame with UH_PASS_RESTIR (same camera) first");
      if (f.world > 1)
         return refuse("uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS needs the whole frame's reservoirs, and a row partition with world > 1 is set (uh_set_restir_partition)");
   }
   // ray-traced ambient occlusion takes the SSAO slot: short hemisphere rays from the G-buffer instead of ssao.frag
   p.rtao = (mask & UH_HYBRID_RTAO) && view.ssao_enabled == 1;
   if (p.rtao && ray_pass_refused(kRtaoRules, f, view, mask, p)) return p;
   // setup_marching_cubes_pass (mod.rs:164): only with the checkbox on
   p.mc = (mask & UH_HYBRID_MARCHING_CUBES) && view.marching_cubes_enabled == 1;
   if (p.mc) {
      if (!(mask & UH_HYBRID_GBUFFER) && !f.gbuffer_done)
         return refuse("uh_render_hybrid: the marching-cubes pass depth-tests against the G-buffer's depth, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER, or marching_cubes_enabled = 0");
      if (!f.has_mesh)
         return refuse("uh_render_hybrid: the marching-cubes pass shades with the first mesh's material (mesh_index 0), and the scene has no mesh");
      if (view.shadows_enabled == 1 && !f.cascades_rendered && !p.render_maps)
         return refuse("uh_render_hybrid: the marching-cubes pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call with UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0");
      if (view.num_lights > f.lights)
         return refuse("uh_render_hybrid: the marching-cubes pass: view.num_lights exceeds the lights added with uh_add_light");
   }
   // motion vectors: a modifier of the G-buffer pass, ignored without it
   p.motion = (mask & UH_HYBRID_MOTION) && (mask & UH_HYBRID_GBUFFER);
   // temporal anti-aliasing: the resolve between the sky pass and present, over the G-buffer the call leaves
   p.taa = (mask & UH_HYBRID_TAA) != 0;
   if (p.taa) {
      if (!(mask & UH_HYBRID_GBUFFER) && !f.gbuffer_done)
         return refuse("uh_render_hybrid: UH_HYBRID_TAA reprojects the G-buffer's positions, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER");
      if ((f.taa_flags & UH_TAA_MOTION) && !((mask & UH_HYBRID_GBUFFER) ? p.motion : f.motion_last))
         return refuse("uh_render_hybrid: UH_HYBRID_TAA with UH_TAA_MOTION reads the motion image, and the last G-buffer pass had no UH_HYBRID_MOTION; set UH_HYBRID_GBUFFER | UH_HYBRID_MOTION, or clear the flag (uh_set_taa_params)");
   }
   // the HDR display chain: between the taa pass and present, over whatever the call leaves in its source; it refuses nothing
   p.post = (mask & UH_HYBRID_POST) != 0;
   // one-bounce diffuse GI: hemisphere rays from the G-buffer, shaded at their hits, added to what the deferred pass of this call wrote
   p.rtgi = (mask & UH_HYBRID_RTGI) != 0;
   if (p.rtgi && ray_pass_refused(kRtgiRules, f, view, mask, p)) return p;
   // glossy reflections: rays drawn around the mirror direction by the pixel's roughness, shaded at their hits, added behind the rtgi pass
   p.glossy = (mask & UH_HYBRID_GLOSSY) != 0;
   if (p.glossy && ray_pass_refused(kGlossyRules, f, view, mask, p)) return p;
   // volumetric fog: sun rays from samples along every pixel's view ray, composited behind the sky pass
   p.fog = (mask & UH_HYBRID_FOG) != 0;
   if (p.fog && ray_pass_refused(kFogRules, f, view, mask, p)) return p;
   // ray-traced glass: two chains of rays per dielectric pixel, which replace what the passes before wrote there
   p.glass = (mask & UH_HYBRID_GLASS) != 0;
   if (p.glass && ray_pass_refused(kGlassRules, f, view, mask, p)) return p;
   // emissive meshes as area lights: sampled points on the emitters, shadowed by any-hit rays, added directly behind the deferred pass
   p.area = (mask & UH_HYBRID_AREA_LIGHTS) != 0;
   if (p.area && ray_pass_refused(kAreaLightRules, f, view, mask, p)) return p;
   p.rt = view.raytracing_supported != 0;
   p.deferred = (mask & UH_HYBRID_DEFERRED) != 0;
   p.frame = (mask & (UH_HYBRID_SSAO | UH_HYBRID_DEFERRED | UH_HYBRID_SKY | UH_HYBRID_PRESENT)) || p.mc || p.rtao || p.taa || p.post;
   p.env = (mask & UH_HYBRID_ENVIRONMENT) != 0;
   p.first = !f.rt_images;
   p.frame_first = p.frame && !f.frame_images;
   return p;
}

}  // namespace uh
