// hybrid_verbs.hip - what a caller reads from and sets on the hybrid graph between uh_render_hybrid calls (include/utopian_hip.h): the
// images and IBL maps (uh_read_hybrid, uh_read_environment), every pass's stats, the params of the rtao, rtgi, glossy, glass, fog and taa passes, the
// taa history reset and jitter. Host code over uh_ctx::Hybrid (context_state.h); nothing here touches the pass order
// (hybrid_graph.hip). The HDR display chain's verbs are in post_graph.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "graphs_internal.h"

int uh_read_hybrid(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (!h.counter.p) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid before the first uh_render_hybrid");
   if (which < 0 || which > UH_HYBRID_GLASS_EVENTS) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image index must be 0..27");
   const char* const no_frame = "uh_read_hybrid: images 6..8 before the first call with an SSAO, deferred, sky or present bit";
   const char* const no_mc = "uh_read_hybrid: images 9..10 before the first marching-cubes pass";
   const char* const no_gr = "uh_read_hybrid: images 11..12 before the first rasterised G-buffer pass";
   const char* const no_taa = "uh_read_hybrid: images 16..17 before the first taa pass (UH_HYBRID_TAA)";
   const char* const no_gi = "uh_read_hybrid: images 18..19 before the first rtgi pass (UH_HYBRID_RTGI); until then the image index must be 0..17";
   const char* const no_gl = "uh_read_hybrid: images 20..22 before the first glossy pass (UH_HYBRID_GLOSSY); until then the image index must be 0..19";
   const char* const no_fog = "uh_read_hybrid: images 23..24 before the first fog pass (UH_HYBRID_FOG); until then the image index must be 0..22";
   const char* const no_glass = "uh_read_hybrid: images 25..27 before the first glass pass (UH_HYBRID_GLASS); until then the image index must be 0..24";
   // image k in UH_HYBRID_* image order: its pixels, its bytes per pixel, whether it exists yet and what a read before that is told
   const struct { const void* pixels; size_t bpp; bool ready; const char* refusal; } img[] = {
      {h.pos.p, sizeof(float4), true, nullptr},
      {h.nrm.p, sizeof(float4), true, nullptr},
      {h.alb.p, sizeof(uchar4), true, nullptr},
      {h.pbr.p, sizeof(float4), true, nullptr},
      {h.shadow.p, 1, true, nullptr},
      {h.refl.p, sizeof(uchar4), true, nullptr},
      {h.ssao.p, sizeof(uint16_t), h.sky_counter.p != nullptr, no_frame},
      {h.deferred.p, sizeof(float4), h.sky_counter.p != nullptr, no_frame},
      {h.present.p, sizeof(uchar4), h.sky_counter.p != nullptr, no_frame},
      {h.mc.target.depth.p, sizeof(float), h.mc.renders != 0, no_mc},
      {h.mc.target.vis.p, sizeof(uint32_t), h.mc.renders != 0, no_mc},
      {h.gr.target.depth.p, sizeof(float), h.gr.renders != 0, no_gr},
      {h.gr.target.vis.p, sizeof(uint32_t), h.gr.renders != 0, no_gr},
      {h.rl.vis.p, 1, h.rl.counters.p != nullptr, "uh_read_hybrid: image 13 before the first call with UH_HYBRID_RESTIR_LIGHTS"},
      {h.ao.counts.p, 1, h.ao.renders != 0, "uh_read_hybrid: image 14 before the first rtao pass (UH_HYBRID_RTAO with view.ssao_enabled = 1)"},
      {h.mv.image.p, sizeof(float4), h.mv.renders != 0, "uh_read_hybrid: image 15 before the first motion pass (UH_HYBRID_GBUFFER | UH_HYBRID_MOTION)"},
      {h.taa.col[h.taa.cur].p, sizeof(float4), h.taa.renders != 0, no_taa},
      {h.taa.n[h.taa.cur].p, sizeof(float), h.taa.renders != 0, no_taa},
      {h.gi.radiance.p, sizeof(float4), h.gi.renders != 0, no_gi},
      {h.gi.counts.p, sizeof(uint32_t), h.gi.renders != 0, no_gi},
      {h.gl.scale.p, sizeof(float4), h.gl.renders != 0, no_gl},
      {h.gl.bias.p, sizeof(float4), h.gl.renders != 0, no_gl},
      {h.gl.counts.p, sizeof(uint32_t), h.gl.renders != 0, no_gl},
      {h.fog.mask.p, sizeof(uint32_t), h.fog.renders != 0, no_fog},
      {h.fog.terms.p, sizeof(float4), h.fog.renders != 0, no_fog},
      {h.glass.radiance.p, sizeof(float4), h.glass.renders != 0, no_glass},
      {h.glass.counts.p, sizeof(uint32_t), h.glass.renders != 0, no_glass},
      {h.glass.events.p, sizeof(uint32_t), h.glass.renders != 0, no_glass}};
   static_assert(sizeof(img) / sizeof(img[0]) == UH_HYBRID_GLASS_EVENTS + 1, "one row per UH_HYBRID_* image");
   if (!img[which].ready) return fail(c, UH_ERR_INVALID_ARGUMENT, img[which].refusal);
   return read_back(c, out, img[which].pixels, (size_t)c->W * c->H * img[which].bpp);
}

int uh_get_hybrid_frame_stats(uh_ctx* c, UhHybridFrameStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_hybrid_frame_stats: null destination", c && c->hy.counter.p, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   for (int k = 0; k < kHybridPasses; k++)
      if ((st = stage_ms(c, c->hy.stage[k], &out->pass_ms[k]))) return st;
   if (h.stage[kStSky].ran) HIP_TRY(c, hipMemcpy(&out->sky_pixels, h.sky_counter.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   out->lights = h.frame_lights;
   return UH_OK;
}

int uh_get_hybrid_restir_stats(uh_ctx* c, UhHybridRestirStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_hybrid_restir_stats: null destination", c && c->hy.rl.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, c->hy.stage[kStRestirLights], &out->pass_ms))) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, h.rl.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->rays = counters[0];
   out->occluded = counters[1];
   return UH_OK;
}

// ---- ray-traced ambient occlusion (utopian_hip.h "UH_HYBRID_RTAO"; rtao.hip) ----
int uh_rtao_default_params(UhRtaoParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhRtaoParams{4, 1.0f, 1.0f, 2, 0.9f, 0.05f};
   return UH_OK;
}

static const char* rtao_params_refusal(const UhRtaoParams& p) {
   if (p.samples < 1 || p.samples > 64) return "samples must be 1..64";
   if (!(p.radius > 0.0f && p.radius <= 10000.0f)) return "radius must be finite, > 0 and <= 10000";
   if (!(p.strength >= 0.0f && p.strength < INFINITY)) return "strength must be finite and >= 0";
   if (p.blur_radius > 4) return "blur_radius must be 0..4";
   if (std::isnan(p.blur_normal_cos) || std::isnan(p.blur_plane)) return "blur_normal_cos and blur_plane must not be NaN";
   return nullptr;
}

int uh_set_rtao_params(uh_ctx* c, const UhRtaoParams* params) {
   return set_params(c, params, "uh_set_rtao_params", rtao_params_refusal, &uh_ctx::Hybrid::ao);
}

int uh_get_rtao_stats(uh_ctx* c, UhRtaoStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_rtao_stats: null destination", c && c->hy.ao.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, c->hy.stage[kStRtaoTrace], &out->trace_ms))) return st;
   if ((st = stage_ms(c, c->hy.stage[kStRtaoFilter], &out->filter_ms))) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, h.ao.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->rays = (uint64_t)counters[0] * h.ao.samples;
   out->occluded = counters[1];
   return UH_OK;
}

int uh_get_rtao_visits(uh_ctx* c, uint64_t* nodes, uint64_t* triangles) {
   int st;
   if (c && nodes && triangles) *triangles = 0;  // (*nodes: by stats_begin)
   if (!stats_begin(c, nodes && triangles ? nodes : nullptr, sizeof(*nodes), "uh_get_rtao_visits: null destination", c && c->hy.ao.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   uint64_t visits[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(visits, h.ao.counters.p + 2, sizeof(visits), hipMemcpyDeviceToHost));
   *nodes = visits[0];
   *triangles = visits[1];
   return UH_OK;
}

// ---- one-bounce ray-traced diffuse GI (utopian_hip.h "UH_HYBRID_RTGI"; rtgi.hip) ----
int uh_rtgi_default_params(UhRtgiParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhRtgiParams{2, 3, 16.0f, 1.0f, 0.9f, 0.05f};
   return UH_OK;
}

static const char* rtgi_params_refusal(const UhRtgiParams& p) {
   if (p.samples < 1 || p.samples > 16) return "samples must be 1..16";
   if (p.blur_radius > 6) return "blur_radius must be 0..6";
   if (!(p.max_radiance > 0.0f && p.max_radiance < INFINITY)) return "max_radiance must be finite and > 0";
   if (!(p.intensity >= 0.0f && p.intensity < INFINITY)) return "intensity must be finite and >= 0";
   if (std::isnan(p.blur_normal_cos) || std::isnan(p.blur_plane)) return "blur_normal_cos and blur_plane must not be NaN";
   return nullptr;
}

int uh_set_rtgi_params(uh_ctx* c, const UhRtgiParams* params) {
   return set_params(c, params, "uh_set_rtgi_params", rtgi_params_refusal, &uh_ctx::Hybrid::gi);
}

int uh_get_rtgi_stats(uh_ctx* c, UhRtgiStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_rtgi_stats: null destination", c && c->hy.gi.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Rtgi& g = c->hy.gi;
   float* const ms[4] = {&out->trace_ms, &out->shadow_ms, &out->filter_ms, &out->composite_ms};
   for (int k = 0; k < 4; k++)
      if ((st = stage_ms(c, g.stage[k], ms[k]))) return st;
   uint32_t counters[3] = {0, 0, 0};
   HIP_TRY(c, hipMemcpy(counters, g.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->rays = (uint64_t)counters[0] * g.samples;
   out->shadow_rays = counters[1];
   out->misses = counters[2];
   return UH_OK;
}

// ---- ray-traced glossy reflections (utopian_hip.h "UH_HYBRID_GLOSSY"; glossy.hip) ----
int uh_glossy_default_params(UhGlossyParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhGlossyParams{1, 3, 0.6f, 16.0f, 1.0f, 0.5f, 0.95f, 0.05f};
   return UH_OK;
}

static const char* glossy_params_refusal(const UhGlossyParams& p) {
   if (p.samples < 1 || p.samples > 16) return "samples must be 1..16";
   if (p.blur_radius > 6) return "blur_radius must be 0..6";
   if (!(p.max_roughness >= 0.0f && p.max_roughness < INFINITY)) return "max_roughness must be finite and >= 0";
   if (!(p.max_radiance > 0.0f && p.max_radiance < INFINITY)) return "max_radiance must be finite and > 0";
   if (!(p.intensity >= 0.0f && p.intensity < INFINITY)) return "intensity must be finite and >= 0";
   if (!(p.blur_roughness > 0.0f && p.blur_roughness < INFINITY)) return "blur_roughness must be finite and > 0";
   if (std::isnan(p.blur_normal_cos) || std::isnan(p.blur_plane)) return "blur_normal_cos and blur_plane must not be NaN";
   return nullptr;
}

int uh_set_glossy_params(uh_ctx* c, const UhGlossyParams* params) {
   return set_params(c, params, "uh_set_glossy_params", glossy_params_refusal, &uh_ctx::Hybrid::gl);
}

int uh_get_glossy_stats(uh_ctx* c, UhGlossyStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_glossy_stats: null destination", c && c->hy.gl.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Glossy& g = c->hy.gl;
   float* const ms[5] = {&out->trace_ms, &out->shade_ms, &out->shadow_ms, &out->filter_ms, &out->composite_ms};
   for (int k = 0; k < 5; k++)
      if ((st = stage_ms(c, g.stage[k], ms[k]))) return st;
   uint32_t counters[5] = {0, 0, 0, 0, 0};
   HIP_TRY(c, hipMemcpy(counters, g.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->shadow_rays = counters[1];
   out->misses = counters[2];
   out->rays = counters[3];
   out->below = counters[4];
   return UH_OK;
}

// ---- ray-traced glass (utopian_hip.h "UH_HYBRID_GLASS"; glass.hip) ----
int uh_glass_default_params(UhGlassParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhGlassParams{8, 16.0f, 1.0f};
   return UH_OK;
}

static const char* glass_params_refusal(const UhGlassParams& p) {
   if (p.max_events < 1 || p.max_events > kGlassMaxEvents) return "max_events must be 1..16";
   if (!(p.max_radiance > 0.0f && p.max_radiance < INFINITY)) return "max_radiance must be finite and > 0";
   if (!(p.intensity >= 0.0f && p.intensity < INFINITY)) return "intensity must be finite and >= 0";
   return nullptr;
}

int uh_set_glass_params(uh_ctx* c, const UhGlassParams* params) {
   return set_params(c, params, "uh_set_glass_params", glass_params_refusal, &uh_ctx::Hybrid::glass);
}

// chains: the rays of round 0; events: the rays of the rounds behind it (a chain enters round r + 1 by the event at the end of its
// segment r); segments: the rays of every round
int uh_get_glass_stats(uh_ctx* c, UhGlassStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_glass_stats: null destination", c && c->hy.glass.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Glass& g = c->hy.glass;
   for (uint32_t r = 0; r < g.rounds; r++) {
      float t = 0.0f, b = 0.0f;
      if ((st = stage_ms(c, g.trace[r], &t)) || (st = stage_ms(c, g.bend[r], &b))) return st;
      out->trace_ms += t;
      out->bend_ms += b;
   }
   if ((st = stage_ms(c, g.shadow, &out->shadow_ms)) || (st = stage_ms(c, g.composite, &out->composite_ms))) return st;
   uint32_t counters[kGlassCounters] = {};
   HIP_TRY(c, hipMemcpy(counters, g.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->shadow_rays = counters[1];
   out->misses = counters[2];
   out->tir = counters[4];
   out->cut = counters[5];
   out->chains = counters[kGlassRound0];
   for (uint32_t r = 1; r <= kGlassMaxEvents; r++) out->events += counters[kGlassRound0 + r];
   out->segments = out->chains + out->events;
   return UH_OK;
}

// ---- volumetric fog (utopian_hip.h "UH_HYBRID_FOG"; fog.hip) ----
int uh_fog_default_params(UhFogParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhFogParams{16, 2, 0.02f, 200.0f, 0.6f, 1.0f, 0.1f, 0, {1.0f, 1.0f, 1.0f}, {0.05f, 0.06f, 0.08f}};
   return UH_OK;
}

static const char* fog_params_refusal(const UhFogParams& p) {
   if (p.steps < 1 || p.steps > 32) return "steps must be 1..32";
   if (p.blur_radius > 4) return "blur_radius must be 0..4";
   if (!(p.density >= 0.0f && p.density < INFINITY)) return "density must be finite and >= 0";
   if (!(p.max_distance > 0.0f && p.max_distance < INFINITY)) return "max_distance must be finite and > 0";
   if (!(p.anisotropy >= -0.95f && p.anisotropy <= 0.95f)) return "anisotropy must be -0.95..0.95";
   if (!(p.intensity >= 0.0f && p.intensity < INFINITY)) return "intensity must be finite and >= 0";
   if (!(p.blur_depth >= 0.0f && p.blur_depth < INFINITY)) return "blur_depth must be finite and >= 0";
   if (p.reserved != 0) return "reserved must be 0";
   for (float a : p.albedo)
      if (!(a >= 0.0f && a <= 1.0f)) return "albedo must be 0..1 in every channel";
   for (float a : p.ambient)
      if (!(a >= 0.0f && a < INFINITY)) return "ambient must be finite and >= 0 in every channel";
   return nullptr;
}

int uh_set_fog_params(uh_ctx* c, const UhFogParams* params) {
   return set_params(c, params, "uh_set_fog_params", fog_params_refusal, &uh_ctx::Hybrid::fog);
}

int uh_get_fog_stats(uh_ctx* c, UhFogStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_fog_stats: null destination", c && c->hy.fog.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Fog& g = c->hy.fog;
   float* const ms[3] = {&out->trace_ms, &out->filter_ms, &out->composite_ms};
   for (int k = 0; k < 3; k++)
      if ((st = stage_ms(c, g.stage[k], ms[k]))) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, g.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->rays = (uint64_t)counters[0] * g.steps;
   out->lit = counters[1];
   return UH_OK;
}

int uh_get_fog_visits(uh_ctx* c, uint64_t* nodes, uint64_t* triangles) {
   int st;
   if (c && nodes && triangles) *triangles = 0;  // (*nodes: by stats_begin)
   if (!stats_begin(c, nodes && triangles ? nodes : nullptr, sizeof(*nodes), "uh_get_fog_visits: null destination", c && c->hy.fog.renders != 0, &st)) return st;
   uint64_t visits[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(visits, c->hy.fog.counters.p + 2, sizeof(visits), hipMemcpyDeviceToHost));
   *nodes = visits[0];
   *triangles = visits[1];
   return UH_OK;
}

int uh_get_motion_stats(uh_ctx* c, UhMotionStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_motion_stats: null destination", c && c->hy.mv.renders != 0, &st)) return st;
   uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, h.mv.stage[0], &out->motion_ms))) return st;
   if ((st = stage_ms(c, h.mv.stage[1], &out->snapshot_ms))) return st;
   std::vector<uint32_t> counts(2 * (size_t)h.mv.blocks);  // a pair per block of the kernel's grid
   HIP_TRY(c, hipMemcpy(counts.data(), h.mv.counters.p, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   for (uint32_t b = 0; b < h.mv.blocks; b++) out->pixels_with += counts[2 * b], out->pixels_without += counts[2 * b + 1];
   out->meshes_static = h.mv.states[kMotionStatic];
   out->meshes_rigid = h.mv.states[kMotionRigid];
   out->meshes_deformed = h.mv.states[kMotionDeformed];
   out->meshes_none = h.mv.states[kMotionNone];
   return UH_OK;
}

// ---- temporal anti-aliasing (utopian_hip.h "temporal anti-aliasing"; taa.hip) ----
int uh_taa_default_params(UhTaaParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhTaaParams{UH_TAA_CLAMP, 16, 0.1f, 1.0f};
   return UH_OK;
}

static const char* taa_params_refusal(const UhTaaParams& p) {
   if (p.flags & ~(uint32_t)(UH_TAA_CLAMP | UH_TAA_MOTION)) return "unknown flag bits (UH_TAA_CLAMP, UH_TAA_MOTION)";
   if (p.max_history < 1) return "max_history must be >= 1";
   if (!(p.alpha_min >= 0.0f && p.alpha_min <= 1.0f)) return "alpha_min must be in [0, 1]";
   if (!(p.clamp_gamma >= 0.0f && p.clamp_gamma < INFINITY)) return "clamp_gamma must be finite and >= 0";
   return nullptr;
}

int uh_set_taa_params(uh_ctx* c, const UhTaaParams* params) {
   return set_params(c, params, "uh_set_taa_params", taa_params_refusal, &uh_ctx::Hybrid::taa);
}

int uh_reset_taa_history(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (c->hy.taa.counters.p) {
      HIP_TRY(c, hipSetDevice(c->device));
      if (int st = sync_all(c)) return st;
   }
   c->hy.taa.valid = false;
   return UH_OK;
}

int uh_get_taa_stats(uh_ctx* c, UhTaaStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_taa_stats: null destination", c && c->hy.taa.renders != 0, &st)) return st;
   uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, h.taa.stage, &out->taa_ms))) return st;
   std::vector<uint32_t> counters(h.taa.counters.n);  // a pair per slot, a line apart
   HIP_TRY(c, hipMemcpy(counters.data(), h.taa.counters.p, counters.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
   for (uint32_t s = 0; s < kTaaCounterSlots; s++)
      out->history_pixels += counters[(size_t)s * kTaaCounterStride], out->reset_pixels += counters[(size_t)s * kTaaCounterStride + 1];
   return UH_OK;
}

// element i (from 1) of the Halton sequence in base b, less 0.5: the radical inverse in double, rounded to float once and kept below 0.5
static float halton_centred(uint64_t i, uint32_t b) {
   double f = 1.0, r = 0.0;
   for (; i; i /= b) {
      f /= (double)b;
      r += f * (double)(i % b);
   }
   return std::fmin((float)(r - 0.5), 0.49999997f);
}

int uh_taa_jitter(uint32_t index, float out[2]) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   out[0] = halton_centred((uint64_t)index + 1, 2);
   out[1] = halton_centred((uint64_t)index + 1, 3);
   return UH_OK;
}

int uh_get_marching_cubes_stats(uh_ctx* c, UhMarchingCubesStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_marching_cubes_stats: null destination", c && c->hy.mc.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if ((st = stage_ms(c, c->hy.stage[kStMarchingCubes], &out->pass_ms))) return st;
   out->renders = h.mc.renders;
   out->triangles = h.mc.tris;
   out->pieces = h.mc.pieces;
   HIP_TRY(c, hipMemcpy(&out->covered_pixels, h.mc.target.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   out->lights = h.mc.lights_used;
   out->time = h.mc.time;
   return UH_OK;
}

int uh_get_gbuffer_raster_stats(uh_ctx* c, UhGbufferRasterStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_gbuffer_raster_stats: null destination", c && c->hy.gr.renders != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   if (h.gbuffer_rasterised)  // the G-buffer stage's record is the last rasterised pass's
      if ((st = stage_ms(c, c->hy.stage[kStGbuffer], &out->pass_ms))) return st;
   out->renders = h.gr.renders;
   out->pieces = h.gr.pieces;
   HIP_TRY(c, hipMemcpy(&out->covered_pixels, h.gr.target.covered.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
   return UH_OK;
}

int uh_read_environment(uh_ctx* c, int which, int face, int mip, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid& h = c->hy;
   if (h.env.builds == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment before the first call with UH_HYBRID_ENVIRONMENT");
   if (which == UH_ENV_BRDF_LUT) {
      if (face != 0 || mip != 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: the BRDF LUT has face 0 and mip 0 only");
      return read_back(c, out, h.env.lut.p, (size_t)kLutSize * kLutSize * sizeof(uint32_t));
   }
   if (which < UH_ENV_ENVIRONMENT || which > UH_ENV_SPECULAR) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: map must be 0..3");
   const int mips = which == UH_ENV_IRRADIANCE ? 1 : (int)kEnvMips;
   if (face < 0 || face > 5 || mip < 0 || mip >= mips) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_environment: face 0..5, mip 0..7 (irradiance: 0)");
   const size_t S = kEnvSize >> mip;
   const float4* base = which == UH_ENV_ENVIRONMENT ? h.env.cube.p : which == UH_ENV_IRRADIANCE ? h.env.irr.p : h.env.spec.p;
   return read_back(c, out, base + env_mip_offset((uint32_t)mip) + (size_t)face * S * S, S * S * sizeof(float4));
}

int uh_get_environment_stats(uh_ctx* c, UhEnvironmentStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_environment_stats: null destination", c && c->hy.env.builds != 0, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   for (int k = 0; k < 4; k++)
      if ((st = stage_ms(c, c->hy.stage[kStEnvCube + k], &out->pass_ms[k]))) return st;
   out->builds = h.env.builds;
   std::memcpy(out->sun_dir, h.env.sun, sizeof(out->sun_dir));
   std::memcpy(out->eye, h.env.eye, sizeof(out->eye));
   return UH_OK;
}

int uh_get_hybrid_stats(uh_ctx* c, UhHybridStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_hybrid_stats: null destination", c && c->hy.counter.p, &st)) return st;
   const uh_ctx::Hybrid& h = c->hy;
   uint32_t metal = 0;
   if (h.stage[kStReflections].ran) HIP_TRY(c, hipMemcpy(&metal, h.counter.p, sizeof(metal), hipMemcpyDeviceToHost));
   const uint64_t n = (uint64_t)c->W * c->H;
   out->rays[0] = h.stage[kStGbuffer].ran && !h.gbuffer_rasterised ? n : 0;  // a rasterised pass casts no ray
   out->rays[1] = h.stage[kStShadows].ran ? n : 0;
   out->rays[2] = metal;
   out->reflection_pixels = metal;
   const int stages[3] = {kStGbuffer, kStShadows, kStReflections};  // the header's order
   for (int k = 0; k < 3; k++)
      if ((st = stage_ms(c, c->hy.stage[stages[k]], &out->pass_ms[k]))) return st;
   return UH_OK;
}
