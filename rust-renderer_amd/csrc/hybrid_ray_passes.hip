// hybrid_ray_passes.hip - the host side of uh_render_hybrid's passes that cast rays from the G-buffer (include/utopian_hip.h): the
// reservoir lights, rtao, rtgi, glossy, glass, area lights and fog. Per pass its first use (what hybrid_prepare of hybrid_graph.hip calls when the
// plan has the pass), its run between its stages' events (what hybrid_passes calls, in the graph's order) and its verbs - default
// params, set params, stats, visits. Host code over uh_ctx::Hybrid (context_state.h) that emits no kernel: those are
// hybrid_kernels.hip, rtao.hip, rtgi.hip, glossy.hip, glass.hip, area_lights.hip and fog.hip. What a call asks of a pass before it runs is a row of
// hybrid_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "graphs_internal.h"

// uh_get_*_visits of the pass `pass`: the walks' node visits and triangle tests, which option "count_visits" has the trace kernel add up
// behind the pass's first two counters
template <class Pass> static int pass_visits(uh_ctx* c, uint64_t* nodes, uint64_t* triangles, const char* null_message, Pass uh_ctx::Hybrid::*pass) {
   int st;
   if (c && nodes && triangles) *triangles = 0;  // (*nodes: by stats_begin)
   if (!stats_begin(c, nodes && triangles ? nodes : nullptr, sizeof(*nodes), null_message, c && (c->hy.*pass).renders != 0, &st)) return st;
   uint64_t visits[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(visits, (c->hy.*pass).counters.p + 2, sizeof(visits), hipMemcpyDeviceToHost));
   *nodes = visits[0];
   *triangles = visits[1];
   return UH_OK;
}

// ---- the reservoir lights (utopian_hip.h "UH_HYBRID_RESTIR_LIGHTS"; hybrid_kernels.hip) ----
int restir_lights_alloc(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = hybrid_light_table(c)) return st;
   if (!h.rl.read) HIP_TRY(c, hipEventCreateWithFlags(&h.rl.read, hipEventDisableTiming));
   if (h.rl.counters.p) return UH_OK;
   if (int st = alloc_group(c, [&](auto f) { h.rl.images(pixels, f); })) return st;
   HIP_TRY(c, hipMemsetAsync(h.rl.vis.p, 0, pixels, c->stream));
   HIP_TRY(c, hipMemsetAsync(h.rl.counters.p, 0, 2 * sizeof(uint32_t), c->stream));
   return UH_OK;
}

// the pixels' reservoirs (whatever the last reservoir pass left: read only) and this call's light count
HybridRestirDev restir_lights_dev(const uh_ctx* c, const UhViewUniformData& view) {
   const uh_ctx::Hybrid& h = c->hy;
   return HybridRestirDev{h.rl.vis.p, h.rl.queue.p, h.rl.counters.p, c->im.reservoirs[2], h.raw_lights.p, (uint32_t)std::min<size_t>(view.num_lights, c->lights.size())};
}

int restir_lights_run(uh_ctx* c, const HybridCall& k, const HybridRestirDev& rl) {
   uh_ctx::Hybrid& h = c->hy;
   const int st = timed(c, h.stage[kStRestirLights], [&] {
      HIP_TRY(c, hipMemsetAsync(h.rl.counters.p, 0, 2 * sizeof(uint32_t), c->stream));
      launch_hybrid_restir_lights(k.lc, k.fp, c->scene, k.hd, rl);
      return (int)UH_OK;
   });
   if (st) return st;
   h.rl.renders++;
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
int rtao_alloc(uh_ctx* c) {
   uh_ctx::Hybrid& h = c->hy;
   if (h.ao.counters.p) return UH_OK;
   if (int st = alloc_group(c, [&](auto f) { h.ao.images((size_t)c->W * c->H, f); })) return st;
   HIP_TRY(c, hipMemsetAsync(h.ao.counts.p, 0, h.ao.counts.n, c->stream));
   return UH_OK;
}

// the rtao pass in ssao_pass's place: classify + trace into the counts, then the resolve / filter into ssao_output
int rtao_run(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid& h = c->hy;
   const UhRtaoParams& p = h.ao.params;
   const RtaoDev ao{h.ao.counts.p, h.ao.queue.p, h.ao.counters.p, p.samples, k.fp.frame_number * 64u, p.blur_radius, p.radius, p.strength, p.blur_normal_cos, p.blur_plane};
   int st = timed(c, h.stage[kStRtaoTrace], [&] {
      HIP_TRY(c, hipMemsetAsync(h.ao.counters.p, 0, 6 * sizeof(uint32_t), c->stream));
      LaunchCfg ac = k.lc;
      ac.count_visits = c->count_visits;  // into the pass's own counters (uh_get_rtao_visits), never UhStats
      launch_rtao_trace(ac, c->scene, k.hd, ao, h.ao.order);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, h.stage[kStRtaoFilter], [&] { launch_rtao_resolve(k.lc, k.hd, ao, h.ssao.p); }))) return st;
   h.ao.samples = p.samples;
   h.ao.renders++;
   return UH_OK;
}

int uh_rtao_default_params(UhRtaoParams* out) { return default_params<uh_ctx::Hybrid::Rtao>(out); }

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
   return pass_visits(c, nodes, triangles, "uh_get_rtao_visits: null destination", &uh_ctx::Hybrid::ao);
}

// ---- one-bounce ray-traced diffuse GI (utopian_hip.h "UH_HYBRID_RTGI"; rtgi.hip) ----
int rtgi_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::Rtgi& gi = c->hy.gi;
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = first_use(c, gi, gi.counters.p, [&](auto f) { gi.images(pixels, f); })) return st;
   // a record per ray: kept while they hold this pass's rays, else allocated again (the stream is waited for first: a pass in flight
   // may still use the old ones)
   const size_t rays = pixels * gi.params.samples;
   if (gi.rays.n < rays || gi.sun_rays.n < rays) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (int st : {grow(c, gi.rays, rays, "uh_render_hybrid: UH_HYBRID_RTGI"), grow(c, gi.sun_rays, rays, "uh_render_hybrid: UH_HYBRID_RTGI")})
         if (st) return st;
   }
   return UH_OK;
}

// the rtgi pass behind deferred_pass: classify + closest-hit walk (which shades the rays and queues the sun rays), the sun rays' any-hit
// walk, the per-pixel mean + filter into the radiance image, then the composite into deferred_output; a stage each
int rtgi_run(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid::Rtgi& g = c->hy.gi;
   const UhRtgiParams& p = g.params;
   const RtgiDev gi{g.counts.p, g.radiance.p, g.mean.p, g.rays.p, g.sun_rays.p, g.queue.p, g.counters.p, p.samples, k.fp.frame_number * 64u,
                    p.blur_radius, p.max_radiance, p.intensity, p.blur_normal_cos, p.blur_plane};
   int st = timed(c, g.stage[0], [&] {
      HIP_TRY(c, hipMemsetAsync(g.counters.p, 0, g.counters.n * sizeof(uint32_t), c->stream));
      launch_rtgi_trace(k.lc, c->scene, k.hd, gi, g.order);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, g.stage[1], [&] { launch_rtgi_shadow(k.lc, c->scene, k.hd, gi); }))) return st;
   if ((st = timed(c, g.stage[2], [&] { launch_rtgi_filter(k.lc, k.hd, gi); }))) return st;
   if ((st = timed(c, g.stage[3], [&] { launch_rtgi_composite(k.lc, c->scene, k.hd, k.fd, gi); }))) return st;
   g.samples = p.samples;
   g.renders++;
   return UH_OK;
}

int uh_rtgi_default_params(UhRtgiParams* out) { return default_params<uh_ctx::Hybrid::Rtgi>(out); }

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
int glossy_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::Glossy& gl = c->hy.gl;
   const char* const who = "uh_render_hybrid: UH_HYBRID_GLOSSY";
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = first_use(c, gl, gl.counters.p, [&](auto f) { gl.images(pixels, f); })) return st;
   // the per-ray buffers, as the rtgi pass keeps its own
   const size_t rays = pixels * gl.params.samples;
   if (gl.rays.n < rays || gl.orig.n < rays || gl.dirs.n < rays || gl.sun_rays.n < rays || gl.ray_queue.n < rays) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (int st : {grow(c, gl.rays, rays, who), grow(c, gl.orig, rays, who), grow(c, gl.dirs, rays, who), grow(c, gl.sun_rays, rays, who),
                     grow(c, gl.ray_queue, rays, who)})
         if (st) return st;
   }
   return UH_OK;
}

// the glossy pass behind the rtgi pass (behind deferred_pass without it): classify + ray generation + the closest-hit walk into hit
// records, the streaming shade (which queues the sun rays), the sun rays' any-hit walk (k_rtgi_shadow on this pass's buffers), the
// per-pixel sums + filter into the two images, then the composite into deferred_output; a stage each
int glossy_run(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid::Glossy& g = c->hy.gl;
   const UhGlossyParams& p = g.params;
   const GlossyDev gl{g.counts.p, g.scale.p, g.bias.p, g.mean_s.p, g.mean_b.p, g.re.p, g.rays.p, g.orig.p, g.dirs.p, g.sun_rays.p, g.ray_queue.p, g.queue.p,
                      g.counters.p, p.samples, k.fp.frame_number * 64u, p.blur_radius, k.fd.rt_on, p.max_roughness, p.max_radiance, p.intensity,
                      p.blur_roughness, p.blur_normal_cos, p.blur_plane};
   int st = timed(c, g.stage[0], [&] {
      HIP_TRY(c, hipMemsetAsync(g.counters.p, 0, g.counters.n * sizeof(uint32_t), c->stream));
      launch_glossy_trace(k.lc, c->scene, k.hd, gl);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, g.stage[1], [&] { launch_glossy_shade(k.lc, c->scene, k.hd, gl); }))) return st;
   if ((st = timed(c, g.stage[2], [&] { launch_rtgi_shadow(k.lc, c->scene, k.hd, glossy_sun_view(gl)); }))) return st;
   if ((st = timed(c, g.stage[3], [&] { launch_glossy_filter(k.lc, k.hd, gl); }))) return st;
   if ((st = timed(c, g.stage[4], [&] { launch_glossy_composite(k.lc, c->scene, k.hd, k.fd, gl); }))) return st;
   g.renders++;
   return UH_OK;
}

int uh_glossy_default_params(UhGlossyParams* out) { return default_params<uh_ctx::Hybrid::Glossy>(out); }

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
int glass_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::Glass& gs = c->hy.glass;
   return first_use(c, gs, gs.counters.p, [&](auto f) { gs.images((size_t)c->W * c->H, f); });
}

// the glass pass behind the glossy pass (behind the rtgi pass or deferred_pass without it): classify + the first event, then max_events
// rounds of the closest-hit walk and the bend kernel - every kernel takes its count from that round's device counter, the two ray queues
// swap, nothing is read back and nothing is waited for -, the sun rays' any-hit walk (k_rtgi_shadow on this pass's buffers) and the
// composite, which replaces deferred_output.rgb on the pixels that cast. A stage per round's walk and bend (trace[0] holds the raygen).
int glass_run(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid::Glass& g = c->hy.glass;
   const UhGlassParams& p = g.params;
   const GlassDev gs{g.counts.p, g.radiance.p, g.events.p, g.rays.p, g.orig.p, g.dirs.p, g.sun_rays.p, {g.ray_queue[0].p, g.ray_queue[1].p}, g.queue.p,
                     g.counters.p, p.max_events, p.max_radiance, p.intensity};
   const uint64_t most = (uint64_t)k.hd.W * k.hd.H * 2u;
   int st = UH_OK;
   for (uint32_t round = 0; round < p.max_events; round++) {
      st = timed(c, g.trace[round], [&] {
         if (round == 0) {
            HIP_TRY(c, hipMemsetAsync(g.counters.p, 0, g.counters.n * sizeof(uint32_t), c->stream));
            launch_glass_raygen(k.lc, c->scene, k.hd, gs);
         }
         launch_glossy_walk(k.lc, c->scene, glass_walk_view(gs, round), most);
         return (int)UH_OK;
      });
      if (st) return st;
      if ((st = timed(c, g.bend[round], [&] { launch_glass_bend(k.lc, c->scene, k.hd, gs, round); }))) return st;
   }
   if ((st = timed(c, g.shadow, [&] { launch_rtgi_shadow(k.lc, c->scene, k.hd, glass_sun_view(gs)); }))) return st;
   if ((st = timed(c, g.composite, [&] { launch_glass_composite(k.lc, k.hd, k.fd, gs); }))) return st;
   g.rounds = p.max_events;
   g.renders++;
   return UH_OK;
}

int uh_glass_default_params(UhGlassParams* out) { return default_params<uh_ctx::Hybrid::Glass>(out); }

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

// ---- emissive meshes as area lights (utopian_hip.h "UH_HYBRID_AREA_LIGHTS"; area_lights.hip) ----
static AreaTableDev area_table_dev(const uh_ctx* c) {
   const uh_ctx::Hybrid::AreaLights& a = c->hy.area;
   return AreaTableDev{a.tri.p, a.keys.p, a.areas.p, a.weights.p, a.cum.p, a.base.p, a.amax.p, a.total.p, a.emitters, (uint32_t)a.host_base.size()};
}

// The emitter table for the tree as it stands: nothing when it was filled for this geom_version (every build and refit bumps it, and a
// mesh's material type changes with uh_add_mesh alone, which asks for a build). Else the emitter meshes' first slots - a host prefix over
// their triangle counts, in uh_add_mesh order - are uploaded and the table is filled, weighted and scanned on the context's stream.
static int area_table(uh_ctx* c) {
   uh_ctx::Hybrid::AreaLights& a = c->hy.area;
   if (a.geom == c->geom_version) return UH_OK;
   const char* const who = "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS";
   std::vector<uint32_t> base(c->meshes.size(), kNoEmitter);
   uint64_t n = 0;
   for (size_t i = 0; i < c->meshes.size(); i++) {
      if (c->meshes[i].material.raytrace_properties[0] != 3.0f) continue;
      base[i] = (uint32_t)n;
      n += c->meshes[i].tris();
      if (n > kAreaMaxEmitters) return fail(c, UH_ERR_CAPACITY, std::string(who) + ": more than 2^20 emitter triangles (the triangles of the meshes of material type 3)");
   }
   const size_t slots = std::max<uint64_t>(1, n), nm = std::max<size_t>(1, base.size());
   if (a.tri.n < 3 * slots || a.base.n < nm) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // a pass in flight may still read the old table
      for (int st : {grow(c, a.tri, 3 * slots, who), grow(c, a.keys, slots, who), grow(c, a.areas, slots, who), grow(c, a.weights, slots, who),
                     grow(c, a.cum, slots, who), grow(c, a.chunks, std::max<uint32_t>(1, area_table_chunks((uint32_t)slots)), who), grow(c, a.base, nm, who)})
         if (st) return st;
   }
   a.host_base = std::move(base);
   a.emitters = (uint32_t)n;
   const int st = timed(c, a.table, [&] {
      HIP_TRY(c, hipMemsetAsync(a.amax.p, 0, sizeof(uint32_t), c->stream));
      HIP_TRY(c, hipMemsetAsync(a.total.p, 0, sizeof(unsigned long long), c->stream));
      if (n) {
         // a slot no packet writes (there is none: every triangle has a packet) would be a degenerate emitter
         HIP_TRY(c, hipMemsetAsync(a.tri.p, 0, 3 * slots * sizeof(float4), c->stream));
         HIP_TRY(c, hipMemsetAsync(a.keys.p, 0, slots * sizeof(uint32_t), c->stream));
         HIP_TRY(c, hipMemsetAsync(a.areas.p, 0, slots * sizeof(float), c->stream));
         HIP_TRY(c, hipMemcpyAsync(a.base.p, a.host_base.data(), a.host_base.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
         launch_area_table(cfg(c), c->scene, area_table_dev(c), a.chunks.p);
      }
      return (int)UH_OK;
   });
   if (st) return st;
   a.geom = c->geom_version;
   a.table_builds++;
   return UH_OK;
}

int area_lights_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::AreaLights& a = c->hy.area;
   const char* const who = "uh_render_hybrid: UH_HYBRID_AREA_LIGHTS";
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = first_use(c, a, a.counters.p, [&](auto f) { a.images(pixels, f); })) return st;
   // the per-sample buffers, as the rtgi pass keeps its own
   const size_t samples = pixels * a.params.samples;
   if (a.rec_d.n < samples || a.rec_s.n < samples || a.rays.n < 2 * samples) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (int st : {grow(c, a.rec_d, samples, who), grow(c, a.rec_s, samples, who), grow(c, a.rays, 2 * samples, who)})
         if (st) return st;
   }
   return area_table(c);
}

// the area-light pass directly behind deferred_pass: classify (which writes the emitters' own pixels) + the samples, whose shadow rays are
// queued, those rays' any-hit walk, the per-pixel means + filter into the two images, then the composite into deferred_output; a stage each
int area_lights_run(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid::AreaLights& a = c->hy.area;
   const UhAreaLightParams& p = a.params;
   const AreaDev al{area_table_dev(c), a.counts.p, a.diffuse.p, a.specular.p, a.mean_d.p, a.mean_s.p, a.rec_d.p, a.rec_s.p, a.rays.p, a.queue.p, a.counters.p,
                    p.samples, k.fp.frame_number * 64u, p.blur_radius, p.show_emitters, k.fd.rt_on, p.max_weight, p.max_radiance, p.intensity,
                    p.blur_normal_cos, p.blur_plane};
   int st = timed(c, a.stage[0], [&] {
      HIP_TRY(c, hipMemsetAsync(a.counters.p, 0, a.counters.n * sizeof(uint32_t), c->stream));
      launch_area_sample(k.lc, c->scene, k.hd, k.fd, al, a.order);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, a.stage[1], [&] { launch_area_shadow(k.lc, c->scene, k.hd, al); }))) return st;
   if ((st = timed(c, a.stage[2], [&] { launch_area_filter(k.lc, k.hd, al); }))) return st;
   if ((st = timed(c, a.stage[3], [&] { launch_area_composite(k.lc, c->scene, k.hd, k.fd, al); }))) return st;
   a.samples = p.samples;
   a.renders++;
   return UH_OK;
}

int uh_area_light_default_params(UhAreaLightParams* out) { return default_params<uh_ctx::Hybrid::AreaLights>(out); }

static const char* area_light_params_refusal(const UhAreaLightParams& p) {
   if (p.samples < 1 || p.samples > 16) return "samples must be 1..16";
   if (p.blur_radius > 6) return "blur_radius must be 0..6";
   if (p.show_emitters > 1) return "show_emitters must be 0 or 1";
   if (!(p.max_weight > 0.0f && p.max_weight < INFINITY)) return "max_weight must be finite and > 0";
   if (!(p.max_radiance > 0.0f && p.max_radiance < INFINITY)) return "max_radiance must be finite and > 0";
   if (!(p.intensity >= 0.0f && p.intensity < INFINITY)) return "intensity must be finite and >= 0";
   if (std::isnan(p.blur_normal_cos) || std::isnan(p.blur_plane)) return "blur_normal_cos and blur_plane must not be NaN";
   return nullptr;
}

int uh_set_area_light_params(uh_ctx* c, const UhAreaLightParams* params) {
   return set_params(c, params, "uh_set_area_light_params", area_light_params_refusal, &uh_ctx::Hybrid::area);
}

int uh_get_area_light_stats(uh_ctx* c, UhAreaLightStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_area_light_stats: null destination", c && c->hy.area.renders != 0, &st)) return st;
   uh_ctx::Hybrid::AreaLights& a = c->hy.area;
   float* const ms[4] = {&out->sample_ms, &out->shadow_ms, &out->filter_ms, &out->composite_ms};
   for (int k = 0; k < 4; k++)
      if ((st = stage_ms(c, a.stage[k], ms[k]))) return st;
   if ((st = stage_ms(c, a.table, &out->table_ms))) return st;
   uint32_t counters[4] = {0, 0, 0, 0};
   unsigned long long total = 0;
   HIP_TRY(c, hipMemcpy(counters, a.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   HIP_TRY(c, hipMemcpy(&total, a.total.p, sizeof(total), hipMemcpyDeviceToHost));
   out->pixels = counters[0];
   out->samples = (uint64_t)counters[0] * a.samples;
   out->shadow_rays = counters[1];
   out->occluded = counters[2];
   out->emitter_pixels = counters[3];
   out->emitters = a.emitters;
   out->total_weight = total;
   out->table_builds = a.table_builds;
   return UH_OK;
}

int uh_read_area_emitters(uh_ctx* c, uint32_t capacity, uint32_t* keys, float* areas, uint32_t* weights, uint32_t* count) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!count) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_area_emitters: null count");
   const uh_ctx::Hybrid::AreaLights& a = c->hy.area;
   if (!a.renders) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_area_emitters before the first area-light pass (UH_HYBRID_AREA_LIGHTS)");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   *count = a.emitters;
   const size_t n = std::min(capacity, a.emitters);
   if (!n) return UH_OK;
   if (keys) HIP_TRY(c, hipMemcpy(keys, a.keys.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
   if (areas) HIP_TRY(c, hipMemcpy(areas, a.areas.p, n * sizeof(float), hipMemcpyDeviceToHost));
   if (weights) HIP_TRY(c, hipMemcpy(weights, a.weights.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
   return UH_OK;
}

// ---- volumetric fog (utopian_hip.h "UH_HYBRID_FOG"; fog.hip) ----
int fog_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::Fog& fog = c->hy.fog;
   return first_use(c, fog, fog.counters.p, [&](auto f) { fog.images((size_t)c->W * c->H, f); });
}

// the fog pass behind atmosphere_pass: classify + the any-hit walk of the samples' sun rays into the bit masks, the resolve / filter into
// the terms image, then the composite into deferred_output; a stage each
int fog_run(uh_ctx* c, const HybridCall& k) {
   uh_ctx::Hybrid::Fog& g = c->hy.fog;
   const UhFogParams& p = g.params;
   const FogDev fg{g.mask.p, g.terms.p, g.dist.p, g.queue.p, g.counters.p, p.steps, (k.fp.frame_number * 64u) ^ kFogSeedXor, p.blur_radius,
                   p.density, p.max_distance, p.anisotropy, p.intensity, p.blur_depth, {p.albedo[0], p.albedo[1], p.albedo[2]},
                   {p.ambient[0], p.ambient[1], p.ambient[2]}};
   int st = timed(c, g.stage[0], [&] {
      HIP_TRY(c, hipMemsetAsync(g.counters.p, 0, g.counters.n * sizeof(uint32_t), c->stream));
      LaunchCfg fc = k.lc;
      fc.count_visits = c->count_visits;  // into the pass's own counters, never UhStats
      launch_fog_trace(fc, k.fp, c->scene, k.hd, fg, g.order);
      return (int)UH_OK;
   });
   if (st) return st;
   if ((st = timed(c, g.stage[1], [&] { launch_fog_resolve(k.lc, k.hd, fg); }))) return st;
   if ((st = timed(c, g.stage[2], [&] { launch_fog_composite(k.lc, k.fp, k.hd, k.fd, fg); }))) return st;
   g.steps = p.steps;
   g.renders++;
   return UH_OK;
}

int uh_fog_default_params(UhFogParams* out) { return default_params<uh_ctx::Hybrid::Fog>(out); }

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
   return pass_visits(c, nodes, triangles, "uh_get_fog_visits: null destination", &uh_ctx::Hybrid::fog);
}
