// area_light_plan_check.cpp - the area-light pass's row of the plan of a uh_render_hybrid call (csrc/hybrid_plan.h, product code) on the
// host, under ASan + UBSan (tests/test_area_light_plan_cpp.py): its four rules, each with its code and its whole message, in their own
// order; their place behind the glass pass's rules (of a glass rule and an area-light rule broken together the glass rule answers, all
// sixteen pairs); no rule on ibl_enabled; the capacity rule at its last accepted and first refused size; and the baseline requests of
// tests/cpp/hybrid_plan_check.cpp, without the bit, accepted as before with `area` false.
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

// hybrid_plan_check.cpp's baseline: everything exists; raytracing_supported = 1, ssao_enabled = 1, every other switch 0; 24 x 16
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

static const char* const kRaytracing = "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS casts shadow rays and view.raytracing_supported is not 1; set it, or clear the bit";
static const char* const kGbuffer =
   "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER";
static const char* const kWithout =
   "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS without UH_HYBRID_DEFERRED in the same call: the pass adds to what the deferred pass writes and has nothing to "
   "add to; set UH_HYBRID_DEFERRED";
static const char* const kCapacity = "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS: a frame of 2^28 pixels or more (its samples are numbered in 32 bits)";
static const char* const kGlass[4] = {
   "uh_render_hybrid: UH_HYBRID_GLASS casts rays and view.raytracing_supported is not 1; set it, or clear the bit",
   "uh_render_hybrid: UH_HYBRID_GLASS casts its rays from the G-buffer, and no G-buffer has been rendered; set UH_HYBRID_GBUFFER",
   "uh_render_hybrid: UH_HYBRID_GLASS without UH_HYBRID_DEFERRED in the same call: the pass replaces what the deferred pass writes on dielectric pixels and "
   "has nothing to write into; set UH_HYBRID_DEFERRED",
   "uh_render_hybrid: UH_HYBRID_GLASS: a frame of 2^27 pixels or more (its rays are numbered in 32 bits)"};

// the four ways to break a pass of this shape, in rule order; `bit` is requested. A later breaker keeps the earlier rules
static void break_rule(Request& r, uint32_t bit, int rule, uint32_t rays_per_pixel) {
   r.mask |= bit;
   if (rule == 0) r.v.raytracing_supported = 0;
   if (rule == 1) r.mask &= ~(uint32_t)UH_HYBRID_GBUFFER, r.f.gbuffer_done = false;
   if (rule == 2) r.mask &= ~(uint32_t)UH_HYBRID_DEFERRED;
   if (rule == 3) r.f.W = (uint32_t)((1ull << 32) / rays_per_pixel), r.f.H = 1;
}

static HybridPlan plan_of(const Request& r) { return hybrid_plan(r.f, r.v, r.mask); }

static void expect_refusal(const Request& r, int code, const char* message, const std::string& what) {
   const HybridPlan p = plan_of(r);
   expect(p.code == code, what + ": code " + std::to_string(p.code));
   expect(p.refusal && std::strcmp(p.refusal, message) == 0, what + ": message " + (p.refusal ? p.refusal : "(none)"));
}

int main() {
   const char* const area[4] = {kRaytracing, kGbuffer, kWithout, kCapacity};
   const int codes[4] = {UH_ERR_INVALID_ARGUMENT, UH_ERR_INVALID_ARGUMENT, UH_ERR_INVALID_ARGUMENT, UH_ERR_CAPACITY};
   // the row itself
   expect(kAreaLightRules.bit == UH_HYBRID_AREA_LIGHTS && UH_HYBRID_AREA_LIGHTS == (1u << 21), "the bit");
   expect(kAreaLightRules.ibl == nullptr, "no ibl rule");
   expect(kAreaLightRules.with == UH_HYBRID_DEFERRED && kAreaLightRules.never == 0 && kAreaLightRules.rays_per_pixel == 16, "the row's bits");
   // accepted
   {
      Request r = baseline();
      r.mask |= UH_HYBRID_AREA_LIGHTS;
      const HybridPlan p = plan_of(r);
      expect(p.code == UH_OK && !p.refusal && p.area && p.deferred && p.frame, "the bit beside UH_HYBRID_FRAME is accepted");
      r.v.ibl_enabled = 1;  // (the maps are built: the deferred pass accepts it) - direct light has no quarrel with the IBL ambient term
      const HybridPlan q = plan_of(r);
      expect(q.code == UH_OK && q.area, "ibl_enabled = 1 is no refusal");
      r.mask |= UH_HYBRID_RTAO | UH_HYBRID_RTGI | UH_HYBRID_GLOSSY | UH_HYBRID_GLASS | UH_HYBRID_TAA | UH_HYBRID_POST;
      r.v.ibl_enabled = 0;
      const HybridPlan all = plan_of(r);
      expect(all.code == UH_OK && all.area && all.rtgi && all.glossy && all.glass && all.rtao && all.taa && all.post, "beside every neighbour");
   }
   // each rule alone, and of two of its own the earlier
   for (int a = 0; a < 4; a++) {
      Request r = baseline();
      break_rule(r, UH_HYBRID_AREA_LIGHTS, a, 16);
      expect_refusal(r, codes[a], area[a], "rule " + std::to_string(a));
      const HybridPlan p = plan_of(r);
      expect(std::strcmp(p.refusal ? p.refusal : "", a == 0   ? kAreaLightRules.raytracing
                                                   : a == 1 ? kAreaLightRules.gbuffer
                                                   : a == 2 ? kAreaLightRules.without
                                                            : kAreaLightRules.capacity) == 0,
             "the message is the row's");
      for (int b = a + 1; b < 4; b++) {
         Request two = baseline();
         break_rule(two, UH_HYBRID_AREA_LIGHTS, b, 16);
         break_rule(two, UH_HYBRID_AREA_LIGHTS, a, 16);
         expect_refusal(two, codes[a], area[a], "rules " + std::to_string(a) + " and " + std::to_string(b));
      }
   }
   // behind the glass pass's rules: of one of each broken together the glass rule answers
   for (int gl = 0; gl < 4; gl++)
      for (int a = 0; a < 4; a++) {
         Request r = baseline();
         break_rule(r, UH_HYBRID_AREA_LIGHTS, a, 16);
         break_rule(r, UH_HYBRID_GLASS, gl, 32);
         // (a capacity breaker of either pass is a frame the other's may accept: 2^27 pixels break the glass rule alone, 2^28 both)
         const bool glass_broken = gl != 3 || (uint64_t)r.f.W * r.f.H >= (1ull << 27);
         expect(glass_broken, "the glass rule is broken");
         // the earlier rules of the glass row that the area breaker broke as well answer first
         int first = gl;
         if (a < gl && a != 3) first = a;
         expect_refusal(r, first == 3 ? UH_ERR_CAPACITY : UH_ERR_INVALID_ARGUMENT, kGlass[first], "glass " + std::to_string(gl) + " before area " + std::to_string(a));
      }
   // the capacity rule at its edge
   {
      Request r = baseline();
      r.mask |= UH_HYBRID_AREA_LIGHTS;
      r.f.W = (1u << 28) - 1, r.f.H = 1;
      expect(plan_of(r).code == UH_OK, "2^28 - 1 pixels are accepted");
      r.f.W = 1u << 14, r.f.H = 1u << 14;
      expect_refusal(r, UH_ERR_CAPACITY, kCapacity, "2^28 pixels");
   }
   // without the bit: the baseline requests as they were
   {
      const uint32_t masks[] = {UH_HYBRID_FRAME, UH_HYBRID_FRAME | UH_HYBRID_RTGI | UH_HYBRID_GLOSSY, UH_HYBRID_GBUFFER, UH_HYBRID_FRAME | UH_HYBRID_GLASS,
                                UH_HYBRID_FRAME | UH_HYBRID_RTAO | UH_HYBRID_TAA | UH_HYBRID_POST, UH_HYBRID_FRAME | UH_HYBRID_FOG};
      for (uint32_t m : masks) {
         Request r = baseline();
         r.mask = m;
         const HybridPlan p = plan_of(r);
         expect(p.code == UH_OK && !p.refusal && !p.area, "mask " + std::to_string(m) + " is accepted without the pass");
      }
      // and a request that breaks every rule of the pass without asking for it is not refused by it
      Request r = baseline();
      r.v.raytracing_supported = 0;
      r.mask = UH_HYBRID_SSAO | UH_HYBRID_SKY | UH_HYBRID_PRESENT;
      r.f.gbuffer_done = false;
      const HybridPlan p = plan_of(r);
      expect(p.code == UH_OK && !p.area, "the rules are consulted with the bit alone");
   }
   if (g_failures) {
      std::printf("%d failure(s)\n", g_failures);
      return 1;
   }
   std::printf("AREA LIGHT PLAN CHECK OK\n");
   return 0;
}
