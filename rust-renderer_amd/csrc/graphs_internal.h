// graphs_internal.h - what the host files of the graphs share (raster_driver.hip, hybrid_graph.hip, hybrid_ray_passes.hip, hybrid_verbs.hip,
// post_graph.hip, forward_graph.hip, denoise_graph.hip): the timed stages, first-use allocation, the preamble of the stats verbs, the
// params setter, what the passes of one uh_render_hybrid call share (HybridCall, over hybrid_plan.h's plan) and the entry points of one
// file that another calls. Private, like context_state.h; nothing here is exported.
#pragma once
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "context_state.h"
#include "hybrid_plan.h"

#pragma GCC visibility push(hidden)
// ---- the timed stages of the graphs (context_state.h Stage) ----
// a stage runs between its two events on the graph's stream; stage_ms: its time in the last call that ran it, 0 when that did not
static int stage_create(uh_ctx* c, Stage* s, int n) {
   for (int k = 0; k < n; k++)
      for (hipEvent_t* ev : {&s[k].begin, &s[k].end})
         if (!*ev) HIP_TRY(c, hipEventCreate(ev));
   return UH_OK;
}
static hipError_t stage_begin(Stage& s, hipStream_t stream) {
   const hipError_t e = hipEventRecord(s.begin, stream);
   s.ran = e == hipSuccess;  // no time for a stage that did not begin
   s.timed = false;
   return e;
}
static hipError_t stage_end(Stage& s, hipStream_t stream) { return hipEventRecord(s.end, stream); }
static int stage_ms(uh_ctx* c, Stage& s, float* out) {
   *out = 0.0f;
   if (!s.ran) return UH_OK;
   if (!s.timed) {
      HIP_TRY(c, hipEventElapsedTime(&s.ms, s.begin, s.end));
      s.timed = true;
   }
   *out = s.ms;
   return UH_OK;
}
// One timed pass: body() between the two events of every stage of `stages` on c->stream, begun in order and ended in order. body
// returns nothing or an int status; a status other than UH_OK, or an end that fails, leaves every stage with ran = false (no time
// for a pass that did not complete) and is what comes back.
template <class Body> static int timed(uh_ctx* c, std::initializer_list<Stage*> stages, Body body) {
   for (Stage* s : stages) HIP_TRY(c, stage_begin(*s, c->stream));
   int st = UH_OK;
   if constexpr (std::is_void_v<decltype(body())>)
      body();
   else
      st = body();
   hipError_t e = hipSuccess;
   for (Stage* s : stages)
      if (!st && e == hipSuccess) e = stage_end(*s, c->stream);
   if (st || e != hipSuccess)
      for (Stage* s : stages) s->ran = false;
   if (st) return st;
   HIP_TRY(c, e);
   return UH_OK;
}
template <class Body> static int timed(uh_ctx* c, Stage& s, Body body) { return timed(c, {&s}, body); }

// ---- first-use allocation ----
// allocates one of the graphs' groups, visit(f) naming its buffers; stops at the first error, before the group's last buffer
template <class Visit> static int alloc_group(uh_ctx* c, Visit visit) {
   hipError_t e = hipSuccess;
   visit([&e](auto& b, size_t n) {
      if (e == hipSuccess) e = b.alloc(n);
   });
   if (e != hipSuccess)
      return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string("uh_render_hybrid: allocation: ") + hipGetErrorString(e));
   return UH_OK;
}
// A pass's first use, when `last` - its group's last buffer - is not there yet: the events of its stages (Pass::stages), then the
// buffers `images` names (alloc_group)
template <class Pass, class Images> static int first_use(uh_ctx* c, Pass& pass, const void* last, Images images) {
   if (last) return UH_OK;
   int st = UH_OK;
   pass.stages([&](Stage& s) {
      if (!st) st = stage_create(c, &s, 1);
   });
   return st ? st : alloc_group(c, images);
}
// b holds n elements or more: kept when it does, allocated again (its contents lost) when not
template <class Buf> static int grow(uh_ctx* c, Buf& b, size_t n, const char* prefix) {
   if (b.p && b.n >= n) return UH_OK;
   const hipError_t e = b.alloc(n);
   if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string(prefix) + ": allocation: " + hipGetErrorString(e));
   return UH_OK;
}

// ---- the stats verbs ----
// What every uh_get_*_stats begins with: a null context is UH_ERR_INVALID_ARGUMENT, a null destination that with `null_message`; the
// destination's `bytes` are zeroed, and they are the answer (UH_OK) while nothing has `rendered`; else every stream is waited for.
// false: *st is what the verb returns; true: the verb fills in its own.
static bool stats_begin(uh_ctx* c, void* out, size_t bytes, const char* null_message, bool rendered, int* st) {
   const auto run = [&]() -> int {
      if (!c) return UH_ERR_INVALID_ARGUMENT;
      if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, null_message);
      std::memset(out, 0, bytes);
      if (!rendered) return UH_OK;
      HIP_TRY(c, hipSetDevice(c->device));
      return sync_all(c);
   };
   *st = run();
   return *st == UH_OK && c && out && rendered;
}

// ---- the params verbs of the hybrid passes ----
// uh_*_default_params of the pass type `Pass`: the params a context holds before the first uh_set_*_params (context_state.h states them once)
template <class Pass, class P> static int default_params(P* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = Pass{}.params;
   return UH_OK;
}
// uh_set_*_params of the pass `pass` (the member of uh_ctx::Hybrid that holds its `params`): a null context is UH_ERR_INVALID_ARGUMENT; null
// params, or params in which `refusal` names a fault, that with "<verb>: null params" or "<verb>: <the fault>", the old ones staying.
template <class P, class Pass> static int set_params(uh_ctx* c, const P* params, const char* verb, const char* (*refusal)(const P&), Pass uh_ctx::Hybrid::*pass) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!params) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string(verb) + ": null params");
   if (const char* why = refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string(verb) + ": " + why);
   (c->hy.*pass).params = *params;
   return UH_OK;
}

// ---- glossy.hip ----
// the glossy pass (UH_HYBRID_GLOSSY), a launcher per timed stage; gl.counters zeroed by the caller. trace: classify (which pixels cast;
// their images zeroed), ray generation (the below samples are settled, the others queued) and the closest-hit walk into the hit records;
// shade: the hit records into radiance records, the sun rays queued (k_rtgi_shadow walks them: launch_rtgi_shadow on glossy_sun_view);
// filter: the per-pixel sums, then the filter when blur_radius is not 0; composite: into deferred_output
namespace uh {
void launch_glossy_trace(const LaunchCfg&, const SceneDev&, const HybridDev&, const GlossyDev&);
void launch_glossy_shade(const LaunchCfg&, const SceneDev&, const HybridDev&, const GlossyDev&);
void launch_glossy_filter(const LaunchCfg&, const HybridDev&, const GlossyDev&);
void launch_glossy_composite(const LaunchCfg&, const SceneDev&, const HybridDev&, const HybridFrameDev&, const GlossyDev&);
// this pass's buffers as k_rtgi_shadow reads them: the sun-ray records, the ray records they zero, the count words, the pixel queue
inline RtgiDev glossy_sun_view(const GlossyDev& gl) {
   RtgiDev gi{};
   gi.counts = gl.counts, gi.rays = gl.rays, gi.sun_rays = gl.sun_rays, gi.queue = gl.queue, gi.counters = gl.counters, gi.samples = gl.samples;
   return gi;
}
void launch_glossy_walk(const LaunchCfg&, const SceneDev&, const GlossyDev&, uint64_t most);  // k_glossy_trace alone, over at most `most` rays
}  // namespace uh

// ---- glass.hip ----
// the glass pass (UH_HYBRID_GLASS); gs.counters zeroed by the caller. raygen: classify (which pixels cast; their images zeroed) and the
// first event, which queues round 0's rays. A round is launch_glossy_walk on glass_walk_view(gs, round) - k_glossy_trace, unchanged,
// writing the hit records of the round's queue - and launch_glass_bend(round), which settles the chains that end and lists those that go
// on for round + 1. Then launch_rtgi_shadow on glass_sun_view and the composite, which replaces deferred_output.rgb.
namespace uh {
void launch_glass_raygen(const LaunchCfg&, const SceneDev&, const HybridDev&, const GlassDev&);
void launch_glass_bend(const LaunchCfg&, const SceneDev&, const HybridDev&, const GlassDev&, uint32_t round);
void launch_glass_composite(const LaunchCfg&, const HybridDev&, const HybridFrameDev&, const GlassDev&);
// round `round` of this pass as k_glossy_trace reads it: the round's queue and its count (GlossyDev::counters[3]), origins, directions
// (their w words are the chain's weight and events: the walk sets its own tmin and tmax), and the hit records out. The view's `counters`
// is valid at index 3 alone (kGlassRound0 >= 3 keeps the pointer inside the buffer): k_glossy_trace reads no other slot, and says so
inline GlossyDev glass_walk_view(const GlassDev& gs, uint32_t round) {
   GlossyDev gl{};
   gl.rays = gs.rays, gl.orig = gs.orig, gl.dirs = gs.dirs, gl.ray_queue = gs.ray_queue[round & 1u], gl.counters = gs.counters + (kGlassRound0 + round - 3u);
   return gl;
}
// this pass's buffers as k_rtgi_shadow reads them: two chains per queued pixel
inline RtgiDev glass_sun_view(const GlassDev& gs) {
   RtgiDev gi{};
   gi.counts = gs.counts, gi.rays = gs.rays, gi.sun_rays = gs.sun_rays, gi.queue = gs.queue, gi.counters = gs.counters, gi.samples = 2;
   return gi;
}
}  // namespace uh

// ---- area_lights.hip ----
// the area-light pass (UH_HYBRID_AREA_LIGHTS). table: the emitter table from the tree's packets (tab.amax zeroed and tab.base uploaded by
// the caller; chunks: scan_chunk_count(tab.n) words). Then a launcher per timed stage, al.counters zeroed by the caller - sample: classify
// (which pixels cast; the images zeroed; the emitters' own pixels written) and the samples, whose shadow rays are queued; shadow: their
// any-hit walk; filter: the per-pixel means, then the filter when blur_radius is not 0; composite: into deferred_output
namespace uh {
uint32_t area_table_chunks(uint32_t n);  // the scan's scratch words for a table of n slots
void launch_area_table(const LaunchCfg&, const SceneDev&, const AreaTableDev&, uint32_t* chunks);
void launch_area_sample(const LaunchCfg&, const SceneDev&, const HybridDev&, const HybridFrameDev&, const AreaDev&, uint32_t order);
void launch_area_shadow(const LaunchCfg&, const SceneDev&, const HybridDev&, const AreaDev&);
void launch_area_filter(const LaunchCfg&, const HybridDev&, const AreaDev&);
void launch_area_composite(const LaunchCfg&, const SceneDev&, const HybridDev&, const HybridFrameDev&, const AreaDev&);
}  // namespace uh

// ---- what the passes of one uh_render_hybrid call share ----
struct HybridCall {
   const HybridPlan& plan;
   const UhViewUniformData& view;
   const FrameParams& fp;
   const LaunchCfg& lc;
   const HybridDev& hd;
   const HybridFrameDev& fd;
};

// ---- hybrid_graph.hip ----
int hybrid_events(uh_ctx* c);          // the events of the hybrid stages and of wait_frames_in_flight (first hybrid or forward call)
int wait_frames_in_flight(uh_ctx* c);  // c->stream (where the graphs run) waits for every other stream of the context
int hybrid_tables(uh_ctx* c);          // the meshes as the vertex and fragment shaders read them (uh_ctx::Hybrid meshes, vertices, indices)
int hybrid_light_table(uh_ctx* c);     // the uh_add_light table as the lit passes read it (uh_ctx::Hybrid::raw_lights)
// the kernels' arguments from the context and the view: the targets, tables and frame of every hybrid kernel (sun: make_params'
// normalised direction, or null for a pass that reads none), and those of the final frame's passes
HybridDev hybrid_dev(const uh_ctx* c, const UhViewUniformData& view, const float* sun);
HybridFrameDev hybrid_frame_dev(const uh_ctx* c, const UhViewUniformData& view);

// ---- hybrid_ray_passes.hip ----
// the passes that cast rays from the G-buffer. *_alloc: the pass's first use (hybrid_prepare, when the plan has the pass); *_run: the pass
// on c->stream, every stage between its two events (hybrid_passes, in the graph's order)
int restir_lights_alloc(uh_ctx* c);  // and the light table, and the event behind the call's reads of the reservoirs
HybridRestirDev restir_lights_dev(const uh_ctx* c, const UhViewUniformData& view);  // what the pass and the deferred pass behind it read
int restir_lights_run(uh_ctx* c, const HybridCall& k, const HybridRestirDev& rl);
int rtao_alloc(uh_ctx* c);
int rtao_run(uh_ctx* c, const HybridCall& k);
int rtgi_alloc(uh_ctx* c);  // and a record per ray of the params' samples
int rtgi_run(uh_ctx* c, const HybridCall& k);
int glossy_alloc(uh_ctx* c);  // and the per-ray buffers of the params' samples
int glossy_run(uh_ctx* c, const HybridCall& k);
int glass_alloc(uh_ctx* c);
int glass_run(uh_ctx* c, const HybridCall& k);
int fog_alloc(uh_ctx* c);
int fog_run(uh_ctx* c, const HybridCall& k);
int area_lights_alloc(uh_ctx* c);  // and the per-sample buffers of the params' samples, and the emitter table when the packets have changed
int area_lights_run(uh_ctx* c, const HybridCall& k);

// ---- post_graph.hip ----
int post_alloc(uh_ctx* c);                                               // the display chain's images, counts and record (first post pass)
int post_run(uh_ctx* c, const LaunchCfg& lc, const float4* src);  // its three timed stages over `src` on c->stream, into post_output

// ---- raster_driver.hip ----
// the column-major product a b, and an instance's row-major 3x4 with row (0, 0, 0, 1), column-major
void mat4_mul(const float* a, const float* b, float* o);
void mat4_from_3x4(const float* o, float* w);
// the frame and its tile grid into fd, with t as what it resolves into; returns the tiles
uint32_t forward_frame(const uh_ctx* c, const RasterTarget& t, ForwardDev& fd);
// k_hybrid_light_prep into the pass's own records (the sun first), then forward.frag over fd's surviving records
void light_and_shade(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, const ForwardDev& fd, HybridLight* lights, bool flat);
// fd.num_tris triangles (flat: bare vertex triples without indices or meshes) from forward.hip's count kernel to its resolve kernel
// over `tiles` tiles: the caller has filled fd but its records and entries, and sized and zeroed b as bin_and_resolve asks
int bin_forward(uh_ctx* c, const LaunchCfg& lc, RasterBins& b, ForwardDev& fd, uint32_t tiles, const char* who, bool flat, uint32_t* pieces);
// the scene's meshes through the forward rasteriser into the target t: depth (cleared to 1.0), vis and rec_of; fd receives everything
// but its colour target. *pieces receives the records. `who` names the entry point in messages.
int raster_scene(uh_ctx* c, const LaunchCfg& lc, const UhViewUniformData& view, RasterBins& b, const RasterTarget& t, ForwardDev& fd, const char* who, uint32_t* pieces);
// the four cascades of uh_ctx::Hybrid::sm; `verb` names the entry point in messages
int render_shadow_maps(uh_ctx* c, const LaunchCfg& lc, const char* verb);
#pragma GCC visibility pop
