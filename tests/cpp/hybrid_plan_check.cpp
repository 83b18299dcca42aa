// hybrid_plan_check.cpp - the plan of a uh_render_hybrid call (csrc/hybrid_plan.h, product code: what csrc/hybrid_graph.hip refuses and
// runs follows it) on the host, under ASan + UBSan (tests/test_hybrid_plan_cpp.py). The 39 rules in the order utopian_hip.h states them,
// each with its code, its whole message and a "breaker" - an edit of the facts, the view and the mask that breaks this rule and, at
// most, later ones, and that forces the rule's own preconditions whatever a later rule's breaker left. Over a baseline in which
// everything exists: every breaker alone answers with its rule; of two breakers the earlier rule answers, all 741 pairs; the five
// capacity rules at their last accepted and first refused sizes; and every field of an accepted plan against its one-line definition.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "hybrid_plan.h"

using namespace uh;

static int g_failures = 0;

static void expect(bool ok, const std::string& what) {
   if (!ok) {
      if (g_failures < 40) std::printf("FAIL: %s\n", what.c_str());
      g_failures++;
   }
}

struct Request {
   HybridFacts f;
   UhViewUniformData v;
   uint32_t mask;
};

// everything exists: the G-buffer rendered, the maps built, the cascades set and rendered, reservoirs recorded, world = 1, two lights,
// one mesh; raytracing_supported = 1, ssao_enabled = 1, every other switch 0; 24 x 16
static Request baseline() {
   Request r{};
   r.f.W = 24, r.f.H = 16;
   r.f.lights = 2;
   r.f.has_mesh = true;
   r.f.restir_recorded = true;
   r.f.world = 1;
   r.f.maps_built = true;
   r.f.cascades_set = true;
   r.f.cascades_rendered = true;
   r.f.gbuffer_done = true;
   r.f.motion_last = true;
   r.f.taa_flags = UH_TAA_CLAMP;
   r.f.rt_images = r.f.frame_images = true;
   r.v.raytracing_supported = 1;
   r.v.ssao_enabled = 1;
   r.mask = UH_HYBRID_FRAME;
   return r;
}

static void no_gbuffer(Request& r) { r.mask &= ~(uint32_t)UH_HYBRID_GBUFFER, r.f.gbuffer_done = false; }
// a pass that casts rays: its bit, whether it minds ibl_enabled = 1, the bits it wants in the same call (`drop`: the one a breaker takes
// away), the bit it does not, its rays per pixel (0: not numbered)
struct Pass { uint32_t bit; bool ibl; uint32_t with, drop, never, rays_per_pixel; };
constexpr Pass kRestir{UH_HYBRID_RESTIR_LIGHTS, false, 0, 0, 0, 0}, kRtao{UH_HYBRID_RTAO, false, 0, 0, 0, 64},
   kRtgi{UH_HYBRID_RTGI, true, UH_HYBRID_DEFERRED, UH_HYBRID_DEFERRED, 0, 16}, kGlossy{UH_HYBRID_GLOSSY, true, UH_HYBRID_DEFERRED, UH_HYBRID_DEFERRED, 0, 16},
   kFog{UH_HYBRID_FOG, false, UH_HYBRID_DEFERRED | UH_HYBRID_SKY, UH_HYBRID_SKY, UH_HYBRID_MARCHING_CUBES, 64},
   kGlass{UH_HYBRID_GLASS, false, UH_HYBRID_DEFERRED, UH_HYBRID_DEFERRED, 0, 32};
// the pass requested with its rule `broken` broken and the rules before that one kept (kPast: all of them kept)
enum RayRule { kRaytracing, kGbuffer, kIbl, kWith, kNever, kCapacity, kPast };
static void ray_pass(Request& r, const Pass& p, RayRule broken) {
   r.mask |= p.bit;
   if (p.bit == UH_HYBRID_RTAO) r.v.ssao_enabled = 1;
   r.v.raytracing_supported = broken == kRaytracing ? 0 : 1;
   if (broken == kRaytracing) return;
   if (broken == kGbuffer) return no_gbuffer(r);
   r.mask |= UH_HYBRID_GBUFFER;
   if (broken == kIbl) r.f.maps_built = true;  // (the reflection and deferred passes' own rules of ibl_enabled = 1 come first)
   if (p.ibl) r.v.ibl_enabled = broken == kIbl ? 1 : 0;
   if (broken == kIbl) return;
   r.mask |= p.with;
   if (broken == kWith) r.mask &= ~p.drop;
   if (broken == kWith) return;
   r.mask &= ~p.never;
   if (broken == kNever) r.mask |= p.never;
   if (broken == kCapacity) r.f.W = (uint32_t)((1ull << 32) / p.rays_per_pixel), r.f.H = 1;
}
static void mc_pass(Request& r) { r.mask |= UH_HYBRID_MARCHING_CUBES, r.v.marching_cubes_enabled = 1; }

struct Rule {
   const char* name;
   int code;
   const char* message;
   void (*breaker)(Request&);
};

static const Rule kRules[] = {
   {"raster_without_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_GBUFFER_RASTER without UH_HYBRID_GBUFFER (the bit chooses how the G-buffer pass runs); set both, or neither",
    [](Request& r) { r.mask |= UH_HYBRID_GBUFFER_RASTER, r.mask &= ~(uint32_t)UH_HYBRID_GBUFFER; }},
   {"reflections_ibl", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: rt_reflections with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), which are not part of this "
    "library until a call with UH_HYBRID_ENVIRONMENT builds them; set that bit, or ibl_enabled = 0 for the reflection pass's non-IBL branch",
    [](Request& r) { r.mask |= UH_HYBRID_RT_REFLECTIONS, r.mask &= ~(uint32_t)UH_HYBRID_ENVIRONMENT, r.v.ibl_enabled = 1, r.f.maps_built = false; }},
   {"maps_before_params", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_SHADOW_MAPS before uh_set_shadowmap_params (the cascades of uh_shadow_cascades or the caller's own)",
    [](Request& r) { r.mask |= UH_HYBRID_SHADOW_MAPS, r.v.shadows_enabled = 1, r.f.cascades_set = false; }},
   {"deferred_maps", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: the deferred pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call with "
    "UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0 for the rt_shadows branch",
    [](Request& r) { r.mask |= UH_HYBRID_DEFERRED, r.mask &= ~(uint32_t)UH_HYBRID_SHADOW_MAPS, r.v.shadows_enabled = 1, r.f.cascades_rendered = false; }},
   {"deferred_ibl", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: the deferred pass with view.ibl_enabled = 1 needs the IBL maps (irradiance, specular, BRDF LUT of ibl.rs), which a call with "
    "UH_HYBRID_ENVIRONMENT builds; set that bit, or ibl_enabled = 0 for the ambient term 0.03 * diffuse * occlusion",
    [](Request& r) {
       r.mask |= UH_HYBRID_DEFERRED, r.mask &= ~(uint32_t)(UH_HYBRID_RT_REFLECTIONS | UH_HYBRID_ENVIRONMENT);
       r.v.shadows_enabled = 0, r.v.ibl_enabled = 1, r.f.maps_built = false;
    }},
   {"deferred_lights", UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: view.num_lights exceeds the lights added with uh_add_light",
    [](Request& r) { r.mask |= UH_HYBRID_DEFERRED, r.v.shadows_enabled = 0, r.v.num_lights = 3; }},
   {"sky_cube", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: the sky pass with view.cubemap_enabled = 1 needs the environment cube (ibl.rs), which a call with UH_HYBRID_ENVIRONMENT builds; "
    "set that bit, or cubemap_enabled = 0 for the IntegrateScattering branch",
    [](Request& r) {  // (no reflection and no deferred pass: a later breaker's ibl_enabled = 1 stays)
       r.mask |= UH_HYBRID_SKY, r.mask &= ~(uint32_t)(UH_HYBRID_RT_REFLECTIONS | UH_HYBRID_DEFERRED | UH_HYBRID_ENVIRONMENT);
       r.v.cubemap_enabled = 1, r.f.maps_built = false;
    }},
   {"restir_raytracing", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts shadow rays and view.raytracing_supported is not 1; set it, or clear the bit",
    [](Request& r) { ray_pass(r, kRestir, kRaytracing); }},
   {"restir_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { ray_pass(r, kRestir, kGbuffer); }},
   {"restir_no_reservoirs", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS reads the spatial reservoirs, and no reservoir pass has run on this context; render a frame with "
    "UH_PASS_RESTIR (same camera) first",
    [](Request& r) { ray_pass(r, kRestir, kPast), r.f.restir_recorded = false; }},
   {"restir_partition", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RESTIR_LIGHTS needs the whole frame's reservoirs, and a row partition with world > 1 is set (uh_set_restir_partition)",
    [](Request& r) { ray_pass(r, kRestir, kPast), r.f.restir_recorded = true, r.f.world = 2; }},
   {"rtao_raytracing", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RTAO casts occlusion rays and view.raytracing_supported is not 1; set it, or clear the bit",
    [](Request& r) { ray_pass(r, kRtao, kRaytracing); }},
   {"rtao_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RTAO casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { ray_pass(r, kRtao, kGbuffer); }},
   {"rtao_capacity", UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_RTAO: a frame of 2^26 pixels or more (its rays are numbered in 32 bits)",
    [](Request& r) { ray_pass(r, kRtao, kCapacity); }},
   {"mc_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: the marching-cubes pass depth-tests against the G-buffer's depth, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER, or "
    "marching_cubes_enabled = 0",
    [](Request& r) { mc_pass(r), no_gbuffer(r); }},
   {"mc_no_mesh", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: the marching-cubes pass shades with the first mesh's material (mesh_index 0), and the scene has no mesh",
    [](Request& r) { mc_pass(r), r.mask |= UH_HYBRID_GBUFFER, r.f.has_mesh = false; }},
   {"mc_maps", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: the marching-cubes pass with view.shadows_enabled = 1 needs the cascaded shadow maps (shadow.rs), which a call with "
    "UH_HYBRID_SHADOW_MAPS renders; set that bit, or shadows_enabled = 0",
    [](Request& r) {  // (no deferred pass: its own rule of the maps comes first)
       mc_pass(r), r.mask |= UH_HYBRID_GBUFFER, r.mask &= ~(uint32_t)(UH_HYBRID_SHADOW_MAPS | UH_HYBRID_DEFERRED);
       r.f.has_mesh = true, r.v.shadows_enabled = 1, r.f.cascades_rendered = false;
    }},
   {"mc_lights", UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: the marching-cubes pass: view.num_lights exceeds the lights added with uh_add_light",
    [](Request& r) {  // (no deferred pass: its own rule of the lights comes first)
       mc_pass(r), r.mask |= UH_HYBRID_GBUFFER, r.mask &= ~(uint32_t)UH_HYBRID_DEFERRED;
       r.f.has_mesh = true, r.v.shadows_enabled = 0, r.v.num_lights = 3;
    }},
   {"taa_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_TAA reprojects the G-buffer's positions, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { r.mask |= UH_HYBRID_TAA, no_gbuffer(r); }},
   {"taa_motion", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_TAA with UH_TAA_MOTION reads the motion image, and the last G-buffer pass had no UH_HYBRID_MOTION; set "
    "UH_HYBRID_GBUFFER | UH_HYBRID_MOTION, or clear the flag (uh_set_taa_params)",
    [](Request& r) { r.mask |= UH_HYBRID_TAA | UH_HYBRID_GBUFFER, r.mask &= ~(uint32_t)UH_HYBRID_MOTION, r.f.taa_flags = UH_TAA_CLAMP | UH_TAA_MOTION; }},
   {"rtgi_raytracing", UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: UH_HYBRID_RTGI casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
    [](Request& r) { ray_pass(r, kRtgi, kRaytracing); }},
   {"rtgi_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RTGI casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { ray_pass(r, kRtgi, kGbuffer); }},
   {"rtgi_ibl", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RTGI with view.ibl_enabled = 1: the IBL ambient term and this pass would both count the sky; set ibl_enabled = 0, or "
    "clear the bit",
    [](Request& r) { ray_pass(r, kRtgi, kIbl); }},
   {"rtgi_deferred", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_RTGI without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass writes and has nothing to add "
    "to; set UH_HYBRID_DEFERRED",
    [](Request& r) { ray_pass(r, kRtgi, kWith); }},
   {"rtgi_capacity", UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_RTGI: a frame of 2^28 pixels or more (its rays are numbered in 32 bits)",
    [](Request& r) { ray_pass(r, kRtgi, kCapacity); }},
   {"glossy_raytracing", UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: UH_HYBRID_GLOSSY casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
    [](Request& r) { ray_pass(r, kGlossy, kRaytracing); }},
   {"glossy_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_GLOSSY casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { ray_pass(r, kGlossy, kGbuffer); }},
   {"glossy_ibl", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_GLOSSY with view.ibl_enabled = 1: the IBL specular term and this pass would both count the sky; set ibl_enabled = 0, or "
    "clear the bit",
    [](Request& r) { ray_pass(r, kGlossy, kIbl); }},
   {"glossy_deferred", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_GLOSSY without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass writes and has nothing to "
    "add to; set UH_HYBRID_DEFERRED",
    [](Request& r) { ray_pass(r, kGlossy, kWith); }},
   {"glossy_capacity", UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_GLOSSY: a frame of 2^28 pixels or more (its rays are numbered in 32 bits)",
    [](Request& r) { ray_pass(r, kGlossy, kCapacity); }},
   {"fog_raytracing", UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: UH_HYBRID_FOG casts sun rays and view.raytracing_supported is not 1; set it, or clear the bit",
    [](Request& r) { ray_pass(r, kFog, kRaytracing); }},
   {"fog_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_FOG marches to the G-buffer's positions, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { ray_pass(r, kFog, kGbuffer); }},
   {"fog_deferred_and_sky", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_FOG without UH_HYBRID_DEFERRED and UH_HYBRID_SKY in the same call: the pass attenuates what those two write and has "
    "nothing to attenuate; set both",
    [](Request& r) { ray_pass(r, kFog, kWith); }},
   {"fog_marching_cubes", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_FOG with UH_HYBRID_MARCHING_CUBES in the same call: the marching-cubes pass's pixels are not in the G-buffer the fog "
    "marches to; clear one of the two bits",
    [](Request& r) { ray_pass(r, kFog, kNever); }},
   {"fog_capacity", UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_FOG: a frame of 2^26 pixels or more (its rays are numbered in 32 bits)",
    [](Request& r) { ray_pass(r, kFog, kCapacity); }},
   {"glass_raytracing", UH_ERR_INVALID_ARGUMENT, "uh_render_hybrid: UH_HYBRID_GLASS casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
    [](Request& r) { ray_pass(r, kGlass, kRaytracing); }},
   {"glass_gbuffer", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_GLASS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
    [](Request& r) { ray_pass(r, kGlass, kGbuffer); }},
   {"glass_deferred", UH_ERR_INVALID_ARGUMENT,
    "uh_render_hybrid: UH_HYBRID_GLASS without UH_HYBRID_DEFERRED in the same call: the pass replaces what the deferred pass writes on dielectric "
    "pixels and has nothing to write into; set UH_HYBRID_DEFERRED",
    [](Request& r) { ray_pass(r, kGlass, kWith); }},
   {"glass_capacity", UH_ERR_CAPACITY, "uh_render_hybrid: UH_HYBRID_GLASS: a frame of 2^27 pixels or more (its rays are numbered in 32 bits)",
    [](Request& r) { ray_pass(r, kGlass, kCapacity); }},
};
constexpr int kRuleCount = (int)(sizeof(kRules) / sizeof(kRules[0]));
static_assert(kRuleCount == 39, "the rules utopian_hip.h states for uh_render_hybrid");

static HybridPlan plan(const Request& r) { return hybrid_plan(r.f, r.v, r.mask); }

static void expect_rule(const HybridPlan& p, const Rule& rule, const std::string& where) {
   const bool ok = p.code == rule.code && p.refusal && std::strcmp(p.refusal, rule.message) == 0;
   expect(ok, where + ": expected " + rule.name + ", got code " + std::to_string(p.code) + " \"" + (p.refusal ? p.refusal : "(accepted)") + "\"");
}

// every extension bit the rules allow together: all of them but one of fog and marching cubes
constexpr uint32_t kEveryBit = UH_HYBRID_FRAME | UH_HYBRID_ENVIRONMENT | UH_HYBRID_SHADOW_MAPS | UH_HYBRID_MARCHING_CUBES | UH_HYBRID_GBUFFER_RASTER |
                               UH_HYBRID_RESTIR_LIGHTS | UH_HYBRID_RTAO | UH_HYBRID_MOTION | UH_HYBRID_TAA | UH_HYBRID_POST | UH_HYBRID_RTGI | UH_HYBRID_GLOSSY |
                               UH_HYBRID_FOG | UH_HYBRID_GLASS;
constexpr uint32_t kUnions[2] = {kEveryBit & ~(uint32_t)UH_HYBRID_MARCHING_CUBES, kEveryBit & ~(uint32_t)UH_HYBRID_FOG};

static void check_baseline() {
   Request r = baseline();
   HybridPlan p = plan(r);
   expect(p.code == UH_OK && !p.refusal, std::string("the baseline with UH_HYBRID_FRAME is accepted: ") + (p.refusal ? p.refusal : ""));
   for (uint32_t mask : kUnions)
      for (int mc = 0; mc < 2; mc++) {
         r = baseline();
         r.mask = mask, r.v.marching_cubes_enabled = mc;
         p = plan(r);
         expect(p.code == UH_OK && !p.refusal, "the baseline with mask " + std::to_string(mask) + " is accepted: " + (p.refusal ? p.refusal : ""));
      }
}

static void check_rules_alone_and_in_pairs() {
   for (int i = 0; i < kRuleCount; i++) {
      Request r = baseline();
      kRules[i].breaker(r);
      expect_rule(plan(r), kRules[i], std::string("breaker ") + kRules[i].name + " alone");
   }
   int pairs = 0;
   for (int i = 0; i < kRuleCount; i++)
      for (int j = i + 1; j < kRuleCount; j++, pairs++) {
         Request r = baseline();
         kRules[j].breaker(r);
         kRules[i].breaker(r);
         expect_rule(plan(r), kRules[i], std::string("breaker ") + kRules[j].name + " then " + kRules[i].name);
      }
   expect(pairs == 741, "741 pairs");
}

// the capacity rule of the five passes that number their rays: rule `at` of kRules, the pass's first rule `first`
static void check_capacity(int first, int at, uint32_t rays_per_pixel) {
   const Rule& rule = kRules[at];
   Request r = baseline();
   rule.breaker(r);
   const uint32_t refused = (uint32_t)((1ull << 32) / rays_per_pixel);
   expect(r.f.W == refused && r.f.H == 1, std::string(rule.name) + ": the breaker's frame is the first refused one");
   expect_rule(plan(r), rule, std::string(rule.name) + " at W = 2^32 / k");
   Request ok = r;
   ok.f.W = refused - 1;
   const HybridPlan p = plan(ok);
   expect(p.code == UH_OK && !p.refusal, std::string(rule.name) + " at W = 2^32 / k - 1 is accepted: " + (p.refusal ? p.refusal : ""));
   ok = r;
   ok.f.W = 1, ok.f.H = refused;  // (the product is taken in 64 bits)
   expect_rule(plan(ok), rule, std::string(rule.name) + " at H = 2^32 / k");
   // the order inside the pass holds at a refused size
   for (int k = first; k < at; k++) {
      Request q = r;
      kRules[k].breaker(q);
      q.f.W = refused, q.f.H = 1;
      expect_rule(plan(q), kRules[k], std::string(rule.name) + "'s size with " + kRules[k].name);
   }
}

// every field of an accepted plan against its definition
static int g_accepted = 0;
static uint32_t g_seen_true = 0, g_seen_false = 0;
static void check_fields(const Request& r) {
   const HybridPlan p = plan(r);
   if (p.code != UH_OK) {
      expect(p.refusal != nullptr, "a refused request has a message");
      return;
   }
   g_accepted++;
   const uint32_t m = r.mask;
   const UhViewUniformData& v = r.v;
   const bool mc = (m & UH_HYBRID_MARCHING_CUBES) && v.marching_cubes_enabled == 1;
   const bool rtao = (m & UH_HYBRID_RTAO) && v.ssao_enabled == 1;
   const bool taa = (m & UH_HYBRID_TAA) != 0, post = (m & UH_HYBRID_POST) != 0;
   const bool frame = (m & (UH_HYBRID_SSAO | UH_HYBRID_DEFERRED | UH_HYBRID_SKY | UH_HYBRID_PRESENT)) || mc || rtao || taa || post;
   const struct { const char* name; bool got, want; } fields[] = {
      {"raster", p.raster, (m & UH_HYBRID_GBUFFER_RASTER) != 0},
      {"maps", p.maps, r.f.maps_built || (m & UH_HYBRID_ENVIRONMENT)},
      {"render_maps", p.render_maps, (m & UH_HYBRID_SHADOW_MAPS) && v.shadows_enabled == 1},
      {"restir", p.restir, (m & UH_HYBRID_RESTIR_LIGHTS) != 0},
      {"rtao", p.rtao, rtao},
      {"rtgi", p.rtgi, (m & UH_HYBRID_RTGI) != 0},
      {"glossy", p.glossy, (m & UH_HYBRID_GLOSSY) != 0},
      {"glass", p.glass, (m & UH_HYBRID_GLASS) != 0},
      {"fog", p.fog, (m & UH_HYBRID_FOG) != 0},
      {"mc", p.mc, mc},
      {"motion", p.motion, (m & UH_HYBRID_MOTION) && (m & UH_HYBRID_GBUFFER)},
      {"rt", p.rt, v.raytracing_supported != 0},
      {"taa", p.taa, taa},
      {"post", p.post, post},
      {"deferred", p.deferred, (m & UH_HYBRID_DEFERRED) != 0},
      {"frame", p.frame, frame},
      {"env", p.env, (m & UH_HYBRID_ENVIRONMENT) != 0},
      {"first", p.first, !r.f.rt_images},
      {"frame_first", p.frame_first, frame && !r.f.frame_images},
   };
   expect(!p.refusal, "an accepted request has no message");
   int k = 0;
   for (const auto& f : fields) {
      if (f.got != f.want) expect(false, std::string("field ") + f.name + " with mask " + std::to_string(m));
      (f.got ? g_seen_true : g_seen_false) |= 1u << k++;
   }
}

static void check_accepted_plans() {
   uint32_t masks[2 * 21 + 3];
   int n = 0;
   for (int b = 0; b <= 20; b++) masks[n++] = 1u << b, masks[n++] = (1u << b) | UH_HYBRID_FRAME;  // (bit 9 is no pass's: ignored)
   masks[n++] = kUnions[0], masks[n++] = kUnions[1], masks[n++] = kEveryBit;
   for (int k = 0; k < n; k++)
      for (int sw = 0; sw < 8; sw++)
         for (uint32_t rt = 0; rt <= 2; rt++)
            for (int have = 0; have < 4; have++)
               for (int maps = 0; maps < 2; maps++) {
                  Request r = baseline();
                  r.mask = masks[k];
                  r.v.ssao_enabled = sw & 1, r.v.marching_cubes_enabled = (sw >> 1) & 1, r.v.shadows_enabled = (sw >> 2) & 1;
                  r.v.raytracing_supported = rt;
                  r.f.rt_images = have & 1, r.f.frame_images = (have >> 1) & 1;
                  r.f.maps_built = maps != 0;
                  check_fields(r);
               }
   expect(g_accepted >= 2000, "accepted requests among those enumerated: " + std::to_string(g_accepted));
   expect(g_seen_true == (1u << 19) - 1 && g_seen_false == (1u << 19) - 1, "every field is seen true and false in an accepted plan");
}

int main() {
   check_baseline();
   check_rules_alone_and_in_pairs();
   check_capacity(11, 13, 64);  // rtao
   check_capacity(20, 24, 16);  // rtgi
   check_capacity(25, 29, 16);  // glossy
   check_capacity(30, 34, 64);  // fog
   check_capacity(35, 38, 32);  // glass
   check_accepted_plans();
   if (g_failures) {
      std::printf("FAIL: %d checks\n", g_failures);
      return 1;
   }
   std::printf("HYBRID PLAN CHECK OK\n");
   return 0;
}
