// post_graph.hip - the HDR display chain's host side (utopian_hip.h "HDR display chain"; kernels in post.hip): first use and the three
// timed stages, which uh_render_hybrid's post pass (hybrid_graph.hip) and uh_post_image both run, and the chain's own verbs - params,
// exposure reset, uh_post_image, level sizes, read-back and stats. Host code over uh_ctx::Hybrid::Post (context_state.h).
#include <hip/hip_runtime.h>

#include <string>

#include "graphs_internal.h"

// the pass's images, counts and record (first pass): the counts zero, as every pass leaves them
int post_alloc(uh_ctx* c) {
   uh_ctx::Hybrid::Post& t = c->hy.post;
   if (t.rec.p) return UH_OK;
   if (int st = first_use(c, t, t.rec.p, [&](auto f) { t.images(c->W, c->H, f); })) return st;
   HIP_TRY(c, hipMemsetAsync(t.hist.p, 0, kPostBins * sizeof(uint32_t), c->stream));
   HIP_TRY(c, hipMemsetAsync(t.rec.p, 0, sizeof(PostRecord), c->stream));
   return UH_OK;
}

// the three stages over `src` on c->stream, each between its two events: uh_render_hybrid's post pass and uh_post_image
int post_run(uh_ctx* c, const LaunchCfg& lc, const float4* src) {
   uh_ctx::Hybrid::Post& t = c->hy.post;
   const UhPostParams& p = t.params;
   PostDev pd{};
   pd.src = src;
   pd.out = t.out.p;
   pd.hist = t.hist.p, pd.hist_copy = t.hist_copy.p, pd.rec = t.rec.p;
   pd.levels = (p.flags & UH_POST_BLOOM) ? post_level_count(c->W, c->H, p.bloom_levels) : 0;
   for (uint32_t k = 0; k <= kPostMaxLevels; k++) {
      if (!post_level_dims(c->W, c->H, k, &pd.lw[k], &pd.lh[k])) pd.lw[k] = pd.lh[k] = 0;
      pd.down[k] = t.down[k].p;
      pd.up[k] = k == pd.levels ? t.down[k].p : t.up[k].p;  // up[last] = down[last]
   }
   pd.W = c->W, pd.H = c->H;
   pd.auto_exposure = (p.flags & UH_POST_AUTO_EXPOSURE) ? 1u : 0u;
   pd.have_prev = t.have_exposure ? 1u : 0u;
   pd.tonemap = p.tonemap;
   pd.manual_exposure = p.manual_exposure, pd.key = p.key, pd.min_exposure = p.min_exposure, pd.max_exposure = p.max_exposure;
   pd.adaptation = p.adaptation, pd.low_percentile = p.low_percentile, pd.high_percentile = p.high_percentile;
   pd.bloom_threshold = p.bloom_threshold, pd.bloom_intensity = p.bloom_intensity;
   t.stages([](Stage& s) { s.ran = false; });
   if (int st = timed(c, t.stage[0], [&] { launch_post_meter(lc, pd); })) return st;
   t.have_exposure = true;  // from here on the record holds this pass's exposure, whatever fails below
   if (pd.levels)
      if (int st = timed(c, t.stage[1], [&] { launch_post_bloom(lc, pd); })) return st;
   if (int st = timed(c, t.stage[2], [&] { launch_post_composite(lc, pd); })) return st;
   HIP_TRY(c, hipGetLastError());
   t.metered = pd.auto_exposure != 0;
   t.levels = pd.levels;
   t.renders++;
   return UH_OK;
}

int uh_post_default_params(UhPostParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   *out = UhPostParams{UH_POST_AUTO_EXPOSURE | UH_POST_BLOOM, UH_TONEMAP_ACES, 6, 1.0f, 0.18f, 0.015625f, 64.0f, 0.1f, 0.5f, 0.95f, 1.0f, 0.04f};
   return UH_OK;
}

static const char* post_params_refusal(const UhPostParams& p) {
   const auto exposure_ok = [](float v) { return v > 0.0f && v <= 65536.0f; };  // (a NaN fails both compares)
   if (p.flags & ~(uint32_t)(UH_POST_AUTO_EXPOSURE | UH_POST_BLOOM)) return "unknown flag bits (UH_POST_AUTO_EXPOSURE, UH_POST_BLOOM)";
   if (p.tonemap > UH_TONEMAP_ACES) return "tonemap must be 0..2 (UH_TONEMAP_NONE, UH_TONEMAP_REINHARD, UH_TONEMAP_ACES)";
   if (p.bloom_levels < 1 || p.bloom_levels > kPostMaxLevels) return "bloom_levels must be 1..8";
   if (!exposure_ok(p.manual_exposure) || !exposure_ok(p.key) || !exposure_ok(p.min_exposure) || !exposure_ok(p.max_exposure))
      return "manual_exposure, key, min_exposure and max_exposure must be finite and in (0, 65536]";
   if (p.min_exposure > p.max_exposure) return "min_exposure must not exceed max_exposure";
   if (!(p.adaptation > 0.0f && p.adaptation <= 1.0f)) return "adaptation must be in (0, 1]";
   if (!(p.low_percentile >= 0.0f && p.low_percentile < p.high_percentile && p.high_percentile <= 1.0f))
      return "percentiles must be 0 <= low_percentile < high_percentile <= 1";
   if (!(p.bloom_threshold >= 0.0f && p.bloom_threshold <= 65536.0f) || !(p.bloom_intensity >= 0.0f && p.bloom_intensity <= 65536.0f))
      return "bloom_threshold and bloom_intensity must be finite and in [0, 65536]";
   return nullptr;
}

int uh_set_post_params(uh_ctx* c, const UhPostParams* params) {
   return set_params(c, params, "uh_set_post_params", post_params_refusal, &uh_ctx::Hybrid::post);
}

int uh_reset_post_exposure(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   c->hy.post.have_exposure = false;  // a pass already enqueued took the flag with it
   return UH_OK;
}

int uh_post_image(uh_ctx* c, const float* rgba32f) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!rgba32f) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_post_image: null image");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Hybrid::Post& t = c->hy.post;
   if (int st = hybrid_events(c)) return st;
   if (int st = post_alloc(c)) return st;
   const size_t pixels = (size_t)c->W * c->H;
   if (int st = grow(c, t.input, pixels, "uh_post_image")) return st;
   if (int st = sync_all(c)) return st;  // an earlier pass may still read the upload buffer
   HIP_TRY(c, hipMemcpy(t.input.p, rgba32f, pixels * sizeof(float4), hipMemcpyHostToDevice));
   if (int st = post_run(c, cfg(c), t.input.p)) return st;
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return UH_OK;
}

int uh_post_level_size(uint32_t W, uint32_t H, uint32_t level, uint32_t* w, uint32_t* h) {
   if (!w || !h) return UH_ERR_INVALID_ARGUMENT;
   return post_level_dims(W, H, level, w, h) ? UH_OK : UH_ERR_INVALID_ARGUMENT;
}

int uh_read_post(uh_ctx* c, int which, int level, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Hybrid::Post& t = c->hy.post;
   if (!out) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: null destination");
   if (t.renders == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post before the first post pass (UH_HYBRID_POST or uh_post_image)");
   if (which < UH_POST_OUTPUT || which > UH_POST_HISTOGRAM) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: image must be 0..3");
   if (which == UH_POST_OUTPUT || which == UH_POST_HISTOGRAM) {
      if (level != 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: post_output and the histogram have level 0 only");
      if (which == UH_POST_OUTPUT) return read_back(c, out, t.out.p, (size_t)c->W * c->H * sizeof(float4));
      if (!t.metered) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: the last pass took no histogram (UH_POST_AUTO_EXPOSURE was not set)");
      return read_back(c, out, t.hist_copy.p, kPostBins * sizeof(uint32_t));
   }
   if (level < 1 || (uint32_t)level > t.levels)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_post: a bloom level the last pass did not build (1..UhPostStats::levels)");
   const float4* img = which == UH_POST_BLOOM_DOWN || (uint32_t)level == t.levels ? t.down[level].p : t.up[level].p;
   return read_back(c, out, img, post_level_texels(c->W, c->H, (uint32_t)level) * sizeof(float4));
}

int uh_get_post_stats(uh_ctx* c, UhPostStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_post_stats: null destination", c && c->hy.post.renders != 0, &st)) return st;
   uh_ctx::Hybrid::Post& t = c->hy.post;
   PostRecord r;
   HIP_TRY(c, hipMemcpy(&r, t.rec.p, sizeof(r), hipMemcpyDeviceToHost));
   out->exposure = r.exposure, out->target_exposure = r.target, out->average_luminance = r.lavg;
   out->metered_pixels = r.metered, out->bad_pixels = r.bad, out->levels = t.levels;
   if ((st = stage_ms(c, t.stage[0], &out->meter_ms))) return st;
   if ((st = stage_ms(c, t.stage[1], &out->bloom_ms))) return st;
   if ((st = stage_ms(c, t.stage[2], &out->tonemap_ms))) return st;
   out->renders = t.renders;
   return UH_OK;
}
