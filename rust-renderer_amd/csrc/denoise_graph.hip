// denoise_graph.hip - the denoiser's host side (uh_denoise, uh_denoise_default_params, uh_reset_denoise_history, uh_read_denoised,
// uh_get_denoise_stats of include/utopian_hip.h; the kernels: denoise.hip). Host code over uh_ctx::Denoise (context_state.h); it reads
// the hybrid graph's G-buffer and motion image and runs on the stream the graphs run on.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "graphs_internal.h"

// ---- the denoiser (utopian_hip.h "the denoiser"; denoise.hip) ----
int uh_denoise_default_params(UhDenoiseParams* out) {
   if (!out) return UH_ERR_INVALID_ARGUMENT;
   std::memset(out, 0, sizeof(*out));
   out->flags = UH_DENOISE_TEMPORAL | UH_DENOISE_DEMODULATE;
   out->iterations = 5;
   out->max_history = 32;
   out->alpha_min = 0.2f;
   out->sigma_luminance = 4.0f;
   out->sigma_plane = 0.005f;  // DESIGN.md section 2, "Denoiser": how the two plane fractions were chosen
   out->reproject_normal_cos = 0.9f;
   out->reproject_plane = 0.005f;
   return UH_OK;
}

// the first refusal of `p` by its own values, or nullptr
static const char* denoise_params_refusal(const UhDenoiseParams& p) {
   if (p.flags & ~(uint32_t)(UH_DENOISE_TEMPORAL | UH_DENOISE_DEMODULATE | UH_DENOISE_MOTION)) return "unknown flag bits";
   if (p.iterations > 5) return "iterations above 5";
   if (p.max_history < 1) return "max_history below 1";
   for (uint32_t r : p.reserved)
      if (r) return "a reserved word is not 0";
   if (!(p.alpha_min >= 0.0f && p.alpha_min <= 1.0f)) return "alpha_min outside [0, 1]";
   if (!(p.sigma_luminance > 0.0f) || !std::isfinite(p.sigma_luminance)) return "sigma_luminance not a finite value above 0";
   if (!(p.sigma_plane > 0.0f) || !std::isfinite(p.sigma_plane)) return "sigma_plane not a finite value above 0";
   if (!(p.reproject_normal_cos >= -1.0f && p.reproject_normal_cos <= 1.0f)) return "reproject_normal_cos outside [-1, 1]";
   if (!(p.reproject_plane > 0.0f) || !std::isfinite(p.reproject_plane)) return "reproject_plane not a finite value above 0";
   return nullptr;
}

int uh_denoise(uh_ctx* c, const UhViewUniformData* view, const UhDenoiseParams* params) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view || !params) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_denoise: null view or params");
   if (const char* why = denoise_params_refusal(*params)) return fail(c, UH_ERR_INVALID_ARGUMENT, std::string("uh_denoise: params: ") + why);
   const uint32_t n = std::min(view->total_samples, view->accumulation_limit);
   if (n == 0)
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_denoise: min(view.total_samples, view.accumulation_limit) is 0: the accumulation image holds no sample to divide by");
   if (c->tiles.world > 1)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_denoise: a tile partition with world > 1 is set (uh_set_tile_partition): this context's accumulation image is partial");
   if (!c->hy.gbuffer_done)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_denoise reads the hybrid G-buffer (position, normal, albedo, mesh index), and none has been rendered; call "
                  "uh_render_hybrid with UH_HYBRID_GBUFFER (same camera) first");
   if ((params->flags & UH_DENOISE_MOTION) && !c->hy.mv.last)
      return fail(c, UH_ERR_INVALID_ARGUMENT,
                  "uh_denoise: UH_DENOISE_MOTION reads the motion image of the last G-buffer pass, and that pass had no UH_HYBRID_MOTION; render "
                  "it with UH_HYBRID_GBUFFER | UH_HYBRID_MOTION, or clear the flag");
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_denoise before uh_build_acceleration");
   HIP_TRY(c, hipSetDevice(c->device));
   uh_ctx::Denoise& dn = c->dn;
   const uh_ctx::Hybrid& h = c->hy;
   const size_t pixels = (size_t)c->W * c->H;
   if (!dn.counters.p) {
      if (int st = stage_create(c, dn.stage, 4)) return st;
      if (!dn.acc_read) HIP_TRY(c, hipEventCreateWithFlags(&dn.acc_read, hipEventDisableTiming));
      hipError_t e = hipSuccess;
      dn.images(pixels, [&e](auto& b, size_t count) {
         if (e == hipSuccess) e = b.alloc(count);
      });
      if (e != hipSuccess) {
         dn.images(0, ReleaseBuf{});
         return fail(c, e == hipErrorOutOfMemory ? UH_ERR_OUT_OF_MEMORY : UH_ERR_HIP, std::string("uh_denoise: allocation: ") + hipGetErrorString(e));
      }
      dn.have_history = false;
   }
   DenoiseDev d{};
   d.acc = c->accumulation.p;
   d.g_pos = h.pos.p, d.g_nrm = h.nrm.p, d.g_pbr = h.pbr.p, d.g_alb = h.alb.p;
   d.unorm_lut = c->d_lut.p;
   const int cur = dn.cur, prev = cur ^ 1;
   d.prev = DenoiseHistory{dn.h_pos[prev].p, dn.h_nrm[prev].p, dn.h_col[prev].p, dn.h_mom[prev].p};
   d.cur = DenoiseHistory{dn.h_pos[cur].p, dn.h_nrm[cur].p, dn.h_col[cur].p, dn.h_mom[cur].p};
   d.input = dn.input.p, d.cv[0] = dn.cv[0].p, d.cv[1] = dn.cv[1].p, d.temporal = dn.temporal.p, d.color = dn.color.p;
   d.output = dn.output.p, d.history = dn.history.p, d.variance = dn.variance.p, d.counters = dn.counters.p;
   d.W = c->W, d.H = c->H;
   d.n = (float)n;
   std::memcpy(d.view, view->view, sizeof(d.view));
   std::memcpy(d.prev_pv, view->prev_frame_projection_view, sizeof(d.prev_pv));
   d.temporal_on = ((params->flags & UH_DENOISE_TEMPORAL) && dn.have_history) ? 1u : 0u;
   d.demodulate = (params->flags & UH_DENOISE_DEMODULATE) ? 1u : 0u;
   d.motion = ((params->flags & UH_DENOISE_MOTION) && d.temporal_on) ? h.mv.image.p : nullptr;  // (without a temporal stage: no effect)
   d.max_history = (float)params->max_history;
   d.alpha_min = params->alpha_min, d.sigma_luminance = params->sigma_luminance, d.sigma_plane = params->sigma_plane;
   d.reproject_normal_cos = params->reproject_normal_cos, d.reproject_plane = params->reproject_plane;
   if (int st = wait_frames_in_flight(c)) return st;
   LaunchCfg lc = cfg(c);
   for (Stage& s : dn.stage) s.ran = false;
   const int temporal = timed(c, dn.stage[0], [&] {
      HIP_TRY(c, hipMemsetAsync(dn.counters.p, 0, 2 * sizeof(uint32_t), c->stream));
      launch_denoise_temporal(lc, d);
      return (int)UH_OK;
   });
   if (temporal) return temporal;
   // the accumulation image and the hybrid targets have been read (the output stage reads the albedo again: hybrid calls run on this
   // stream): a frame enqueued from here on applies its accumulate tail behind this point, like behind a frame's
   HIP_TRY(c, hipEventRecord(dn.acc_read, c->stream));
   c->last_acc = dn.acc_read;
   // from here on this call's set is the history, whatever fails below
   dn.cur = prev;
   dn.have_history = true;
   dn.calls++;
   if (int st = timed(c, dn.stage[1], [&] { launch_denoise_variance(lc, d); })) return st;
   const auto atrous = [&] {
      for (uint32_t level = 0; level < params->iterations; level++) launch_denoise_atrous(lc, d, level);
   };
   if (int st = timed(c, dn.stage[2], atrous)) return st;
   if (int st = timed(c, dn.stage[3], [&] { launch_denoise_output(lc, d, params->iterations & 1); })) return st;
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

int uh_reset_denoise_history(uh_ctx* c) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (c->dn.counters.p) {
      HIP_TRY(c, hipSetDevice(c->device));
      if (int st = sync_all(c)) return st;
   }
   c->dn.have_history = false;
   return UH_OK;
}

int uh_read_denoised(uh_ctx* c, int which, void* out) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   const uh_ctx::Denoise& dn = c->dn;
   if (dn.calls == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_denoised before the first uh_denoise");
   if (which < UH_DENOISE_COLOR || which > UH_DENOISE_VARIANCE) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_read_denoised: image index must be 0..5");
   // image k's pixels and its bytes per pixel, in UH_DENOISE_* image order
   const std::pair<const void*, size_t> img[] = {{dn.color.p, sizeof(float4)}, {dn.output.p, sizeof(uchar4)}, {dn.input.p, sizeof(float4)},
                                                 {dn.temporal.p, sizeof(float4)}, {dn.history.p, sizeof(float)}, {dn.variance.p, sizeof(float)}};
   return read_back(c, out, img[which].first, (size_t)c->W * c->H * img[which].second);
}

int uh_get_denoise_stats(uh_ctx* c, UhDenoiseStats* out) {
   int st;
   if (!stats_begin(c, out, sizeof(*out), "uh_get_denoise_stats: null destination", c && c->dn.calls != 0, &st)) return st;
   uh_ctx::Denoise& dn = c->dn;
   for (int k = 0; k < 4; k++)
      if ((st = stage_ms(c, dn.stage[k], &out->pass_ms[k]))) return st;
   uint32_t counters[2] = {0, 0};
   HIP_TRY(c, hipMemcpy(counters, dn.counters.p, sizeof(counters), hipMemcpyDeviceToHost));
   out->geometry_pixels = counters[0];
   out->history_pixels = counters[1];
   return UH_OK;
}
