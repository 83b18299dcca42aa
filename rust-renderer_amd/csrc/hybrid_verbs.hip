// hybrid_verbs.hip - what a caller reads from and sets on the hybrid graph between uh_render_hybrid calls (include/utopian_hip.h): the
// images and IBL maps (uh_read_hybrid, uh_read_environment), the frame, hybrid, motion, taa, marching-cubes, raster and environment
// stats, the taa params, history reset and jitter. Host code over uh_ctx::Hybrid (context_state.h); nothing here touches the pass order
// (hybrid_graph.hip). The verbs of the passes that cast rays are in hybrid_ray_passes.hip, the HDR display chain's in post_graph.hip.
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
   if (which < 0 || which > UH_HYBRID_AREA_COUNTS) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_hybrid: image index must be 0..30");
   const char* const no_frame = "uh_read_hybrid: images 6..8 before the first call with an SSAO, deferred, sky or present bit";
   const char* const no_mc = "uh_read_hybrid: images 9..10 before the first marching-cubes pass";
   const char* const no_gr = "uh_read_hybrid: images 11..12 before the first rasterised G-buffer pass";
   const char* const no_taa = "uh_read_hybrid: images 16..17 before the first taa pass (UH_HYBRID_TAA)";
   const char* const no_gi = "uh_read_hybrid: images 18..19 before the first rtgi pass (UH_HYBRID_RTGI); until then the image index must be 0..17";
   const char* const no_gl = "uh_read_hybrid: images 20..22 before the first glossy pass (UH_HYBRID_GLOSSY); until then the image index must be 0..19";
   const char* const no_fog = "uh_read_hybrid: images 23..24 before the first fog pass (UH_HYBRID_FOG); until then the image index must be 0..22";
   const char* const no_glass = "uh_read_hybrid: images 25..27 before the first glass pass (UH_HYBRID_GLASS); until then the image index must be 0..24";
   const char* const no_area = "uh_read_hybrid: images 28..30 before the first area-light pass (UH_HYBRID_AREA_LIGHTS); until then the image index must be 0..27";
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
      {h.glass.events.p, sizeof(uint32_t), h.glass.renders != 0, no_glass},
      {h.area.diffuse.p, sizeof(float4), h.area.renders != 0, no_area},
      {h.area.specular.p, sizeof(float4), h.area.renders != 0, no_area},
      {h.area.counts.p, sizeof(uint32_t), h.area.renders != 0, no_area}};
   static_assert(sizeof(img) / sizeof(img[0]) == UH_HYBRID_AREA_COUNTS + 1, "one row per UH_HYBRID_* image");
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
int uh_taa_default_params(UhTaaParams* out) { return default_params<uh_ctx::Hybrid::Taa>(out); }

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
