// frame_loop.hip — the frame loop of the path tracer: uh_render_frame and uh_render_frames, and the phases of one batch of frames
// they run back to back (begin | per frame: reservoir chain, exchange | end: the path-tracing wavefront), which an in-process group
// (mgpu.hip) interleaves over its contexts through the uhi_* entry points of context_internal.h. Host-side counterpart of
// build_path_tracing_render_graph (utopian/src/renderers/mod.rs:189-375). What a sample pass is made of, how many frames a wavefront
// carries and how a call's frames are split is decided in frame_plan.h, without HIP; here the plan is taken and enqueued.
// struct uh_ctx is context_state.h; the context's lifetime, read-backs and stats are context.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "context_internal.h"
#include "context_state.h"
#include "device_types.h"
#include "frame_plan.h"
#include "tile_partition.h"
#include "utopian_hip.h"

using namespace uh;

FrameParams make_params(uh_ctx* c, const UhViewUniformData& v) {
   FrameParams fp;
   std::memset(&fp, 0, sizeof(fp));
   std::memcpy(fp.inv_view, v.inverse_view, sizeof(fp.inv_view));
   std::memcpy(fp.inv_proj, v.inverse_projection, sizeof(fp.inv_proj));
   std::memcpy(fp.prev_pv, v.prev_frame_projection_view, sizeof(fp.prev_pv));
   // normalize(view.sun_dir) (reference.rgen:64, reference.rmiss:18): v * (1 / sqrt(dot))
   float d = (v.sun_dir[0] * v.sun_dir[0] + v.sun_dir[1] * v.sun_dir[1]) + v.sun_dir[2] * v.sun_dir[2];
   float inv = 1.0f / std::sqrt(d);
   for (int a = 0; a < 3; a++) fp.sun_dir[a] = v.sun_dir[a] * inv;
   fp.W = c->W;
   fp.H = c->H;
   // reference.rgen:24: int(float(total_samples) + time * 10000.0)
   fp.frame_number = (uint32_t)(int32_t)((float)v.total_samples + v.time * 10000.0f);
   fp.batch_frames = 1;
   fp.frame_numbers[0] = fp.frame_number;
   fp.total_samples_of[0] = v.total_samples;
   fp.samples_per_frame = v.samples_per_frame;
   fp.total_samples = v.total_samples;
   fp.num_bounces = v.num_bounces;
   fp.accumulation_limit = v.accumulation_limit;
   fp.sky_enabled = v.sky_enabled;
   fp.sun_shadow_enabled = v.sun_shadow_enabled;
   fp.lights_enabled = v.lights_enabled;
   fp.use_ris = v.use_ris_light_sampling;
   fp.full_frame_restir = c->full_frame_restir ? 1u : 0u;
   fp.furnace = c->furnace ? 1u : 0u;
   fp.num_lights_used = v.num_lights < v.max_num_lights_used ? v.num_lights : v.max_num_lights_used;
   fp.temporal_enabled = v.temporal_reuse_enabled;
   fp.spatial_enabled = v.spatial_reuse_enabled;
   fp.tp_rank = c->tiles.rank;
   fp.tp_world = c->tiles.world;
   fp.tp_tile = c->tiles.tile;
   fp.tiles_x = tiles_across(c->W, c->tiles.tile);
   fp.owned_pixels = c->tiles.world > 1 ? c->tiles.owned_pixels.p : nullptr;
   fp.n_owned = traced_pixels(c);
   return fp;
}

int sync_all(uh_ctx* c) {
   if (c->restir_stream) HIP_TRY(c, hipStreamSynchronize(c->restir_stream));
   for (auto& s : c->slots) {
      if (!s.ready) continue;
      HIP_TRY(c, hipStreamSynchronize(s.stream));
      HIP_TRY(c, hipStreamSynchronize(s.side));
   }
   return UH_OK;
}

// slot i exists and can hold `batch` frames worth of paths
static int ensure_slot(uh_ctx* c, uint32_t i, uint32_t batch = 1) {
   size_t need = (size_t)traced_pixels(c) * batch;  // path ids are dense over the rank's owned pixels
   if (need < 64) need = 64;  // a rank that owns no pixel (more ranks than tiles) still gets a well-formed, empty slot
   Slot& s = c->slots[i];
   if (s.ready && s.capacity >= need) return UH_OK;
   if (s.ready) {
      HIP_TRY(c, hipStreamSynchronize(s.stream));
      HIP_TRY(c, hipStreamSynchronize(s.side));
      if (c->last_acc == s.ev_acc) c->last_acc = nullptr;
      for (hipEvent_t& r : c->spatial_reader)
         if (r == s.ev_acc) r = nullptr;
      if (c->t_start == s.frame_start) c->t_start = nullptr;
      if (c->t_stop == s.frame_stop) c->t_stop = nullptr;
      s.destroy();
   }
   HIP_TRY(c, s.create(need));
   return UH_OK;
}

// reference_pt_pass of one frame on one slot (reference.rgen:22-145 as a kernel chain): per sample the plan (frame_plan.h), then
// its launches
static int enqueue_path_trace(uh_ctx* c, Slot& s, const FrameParams& frame) {
   FrameParams fp = frame;  // + sun_verdicts and slim_state, which follow the launches chosen per sample
   LaunchCfg lc = cfg(c);
   lc.stream = s.stream;
   const SampleOptions opt{c->fused_bounces, c->fused_always, c->sun_x.verdicts, c->slim_state, c->overlap_miss, c->overlap_shadow, lc.closest_blocks_per_cu, lc.shadow_blocks_per_cu,
                           c->fused_primary};
   // (a pixel whose list is longer than the grid kernel walks hands its ray to the tree walk behind it)
   const bool cam_leftovers = c->cam.max_list_interior > std::max(c->cam.dev.walk_whole, c->cam.dev.max_walk);
   const SampleFacts facts{fp.batch_frames, fp.num_bounces, fp.samples_per_frame, fp.n_owned, s.ps.shard_cap, fp.sun_shadow_enabled == 1, fp.lights_enabled == 1,
                           c->sun.this_frame, c->cam.this_frame, fp.primary_implicit != 0, c->cam.this_frame && !cam_leftovers, lc.count_visits, fp.owned_pixels != nullptr};
   Control* ctl = s.control.p;
   DeviceStats* st = c->dstats.p;
   // reference.rgen:28: samples of one frame run back to back (the raygen RNG state carries over)
   for (uint32_t smp = 0; smp < fp.samples_per_frame; smp++) {
      uint32_t slot = 0;
      const bool gpu_idle = !c->last_acc || hipEventQuery(c->last_acc) == hipSuccess;
      const SamplePlan plan = plan_sample(opt, facts, gpu_idle);
      lc.closest_blocks_per_cu = plan.closest_blocks_per_cu;
      lc.shadow_blocks_per_cu = plan.shadow_blocks_per_cu;
      fp.sun_verdicts = plan.sun_verdicts ? 1u : 0u;
      fp.slim_state = plan.slim_state ? 1u : 0u;
      HIP_TRY(c, hipMemsetAsync(ctl, 0, sizeof(Control), s.stream));
      // (behind the choice of the state: the origin quads it stores carry the id or the RNG word; fused_primary: bounce 0's kernel stands at the pixels itself)
      if (!plan.fused_primary) launch_generate(lc, fp, s.ps, ctl, smp);
      for (uint32_t b = 0; b < plan.wave_bounces; b++) {
         const bool primary_shade = b == 0 && plan.fused_primary;  // bounce 0's walk and shading are one launch, timed as shading (kind 2)
         if (primary_shade)
            slot += 2;  // (the cursor slots of the two launches it stands for stay theirs: the later launches keep their numbers)
         else {
            begin_timed(c, (b == 0 && plan.grid_primary) ? 3 : 0, s.stream);
            if (b == 0 && plan.grid_primary) {
               // no tree walk for the primary rays of a camera at rest (and no launch for one when no pixel's list is too long for the grid kernel)
               launch_trace_camera_grid(lc, fp, c->scene, s.ps, ctl, st, slot, slot + 1, c->cam.dev, cam_leftovers);
               slot += 2;
            } else
               launch_trace_closest(lc, c->scene, s.ps, ctl, st, b, slot++, b == 0 ? UH_RAY_PRIMARY : UH_RAY_BOUNCE);
            end_timed(c, s.stream);
         }
         // shade_hit(b) rewrites ray_o / thr / rad of the paths shadow(b-1) still reads on the side stream, and refills the
         // miss queue shade_miss(b-1) reads there
         if (plan.side_used && b > 0) HIP_TRY(c, hipStreamWaitEvent(s.stream, s.ev_shadowed, 0));
         begin_timed(c, 2, s.stream);
         if (primary_shade) launch_primary_shade(lc, fp, c->scene, s.ps, ctl, st, c->cam.dev);
         else launch_shade_hit(lc, fp, c->scene, s.ps, c->im, ctl, st, b);  // either also hands the bounce's misses to shade_miss (Q_MISS)
         if (!c->overlap_miss) launch_shade_miss(lc, fp, s.ps, ctl, st, b);
         end_timed(c, s.stream);
         // shade_miss(b) and the shadow queries of bounce b are independent of trace_closest(b+1) (they only read what
         // shade_hit(b) wrote): on the side stream their blocks fill the tail of the other kernel
         LaunchCfg lsh = lc;
         hipStream_t sh_stream = s.stream;
         if (plan.side_used) {
            HIP_TRY(c, hipEventRecord(s.ev_shaded, s.stream));
            HIP_TRY(c, hipStreamWaitEvent(s.side, s.ev_shaded, 0));
         }
         if (c->overlap_miss) {
            LaunchCfg ls = lc;
            ls.stream = s.side;
            begin_timed(c, 2, s.side);
            launch_shade_miss(ls, fp, s.ps, ctl, st, b);
            end_timed(c, s.side);
         }
         if (plan.side_shadow) {
            lsh.stream = s.side;
            sh_stream = s.side;
         }
         if (fp.sun_shadow_enabled == 1 && !plan.fused_sun0) {
            begin_timed(c, 1, sh_stream);
            if (c->sun.this_frame) {
               launch_trace_sun_grid(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, c->sun.dev);
               launch_trace_shadow(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, false, true);  // the rays the grid handed over (border cells, long lists)
            } else
               launch_trace_shadow(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, false);
            end_timed(c, sh_stream);
         }
         if (fp.lights_enabled == 1) {
            begin_timed(c, 4, sh_stream);
            launch_trace_shadow(lsh, fp, c->scene, s.ps, ctl, st, b, slot++, true);
            end_timed(c, sh_stream);
         }
         if (plan.side_used) HIP_TRY(c, hipEventRecord(s.ev_shadowed, s.side));
      }
      // the side stream's work: the sky integrals, and - unless the fused kernel asks them itself - bounce 0's sun and light rays, whose
      // results the fused kernel starts from
      if (plan.join_side && !plan.fused_sun0) {
         HIP_TRY(c, hipEventRecord(s.ev_side_done, s.side));
         HIP_TRY(c, hipStreamWaitEvent(s.stream, s.ev_side_done, 0));
      }
      if (plan.fused) {
         begin_timed(c, 0, s.stream);
         launch_path_fused(lc, fp, c->scene, s.ps, ctl, st, c->sun.dev, c->sun.this_frame, plan.fused_sun0);
         end_timed(c, s.stream);
      }
      if (plan.join_side && plan.fused_sun0) {  // (bounce 0's sky integrals ran beside the fused kernel)
         HIP_TRY(c, hipEventRecord(s.ev_side_done, s.side));
         HIP_TRY(c, hipStreamWaitEvent(s.stream, s.ev_side_done, 0));
      }
      if (plan.flush) launch_flush_survivors(lc, fp, s.ps, ctl);
      const bool last = smp + 1 == fp.samples_per_frame;
      // the accumulate / store tail (rgen:130-144) is a read-modify-write on the accumulation image:
      // frames must apply it in order, everything before it may overlap with other frames in flight
      if (last && c->last_acc && c->last_acc != s.ev_acc) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->last_acc, 0));
      launch_finish_sample(lc, fp, s.ps, c->im, smp, last);
   }
   if (fp.samples_per_frame == 0) {
      // zero samples: the raygen still runs its accumulate / store tail
      if (c->last_acc && c->last_acc != s.ev_acc) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->last_acc, 0));
      launch_resolve(lc, c->im, c->W, c->H, fp.total_samples, fp.accumulation_limit);
   }
   HIP_TRY(c, hipEventRecord(s.ev_acc, s.stream));
   c->last_acc = s.ev_acc;
   return UH_OK;
}

// ---- one batch of frames, in phases: begin | per frame: reservoir chain, exchange | end (the path-tracing wavefront).
// uh_render_frame(s) runs the phases back to back; an in-process group (mgpu.hip) interleaves them over its contexts,
// because frame f + 1's temporal pass of one GPU reads the bands every other GPU wrote in frame f.
struct uh_batch {
   FrameParams fp;
   uint32_t pass_mask = 0, batch = 0;
   bool restir_frame = false, reads_reservoirs = false;
   int read_slot[kMaxBatchFrames];
   LaunchCfg rc;
};

static UhReservoir* spatial_buf(uh_ctx* c, int slot) { return slot ? c->spatial_ring.p + (size_t)(slot - 1) * c->res_stride : c->reservoirs[2].p; }

static RowSpans spans_of(const uh_ctx* c, uint32_t row0, uint32_t rows, uint32_t extra0, uint32_t extra_rows) { return RowSpans{{row0, extra0}, {rows, extra_rows}, c->W}; }

static int batch_begin(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t batch, uh_batch& bs) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frame: null view");
   if (!c->built && c->topology_valid && view->rebuild_tlas == 1) {
      // the application moved instances and asks for the per-frame rebuild (main.rs:392,526; graph.rs:715-741)
      if (int st = uh_refit_acceleration(c)) return st;
   }
   if (!c->built) return fail(c, UH_ERR_NOT_BUILT, "uh_render_frame before uh_build_acceleration");
   if (view->num_bounces > kMaxBounces) return fail(c, UH_ERR_INVALID_ARGUMENT, "num_bounces > 64");
   if (view->samples_per_frame > 4096) return fail(c, UH_ERR_INVALID_ARGUMENT, "samples_per_frame > 4096 (the reference UI stops at 10)");
   if (view->num_lights > c->lights.size() && (view->lights_enabled == 1 || (pass_mask & UH_PASS_RESTIR)))
      return fail(c, UH_ERR_INVALID_ARGUMENT, "view.num_lights exceeds the lights added with uh_add_light");
   HIP_TRY(c, hipSetDevice(c->device));
   FrameParams& fp = bs.fp;
   fp = make_params(c, *view);
   fp.batch_frames = batch;
   for (uint32_t f = 0; f < batch; f++) {
      // frame f of the batch: total_samples advanced by the application once per frame (main.rs:467-469)
      const uint32_t total = view->total_samples + f * view->samples_per_frame;
      fp.total_samples_of[f] = total;
      fp.frame_numbers[f] = (uint32_t)(int32_t)((float)total + view->time * 10000.0f);
   }
   // the per-camera grid serves the primary rays of the path tracer and the G-buffer cast of this call
   c->cam.this_frame = false;
   const bool primary_rays = ((pass_mask & UH_PASS_REFERENCE_PT) && fp.num_bounces > 0 && fp.samples_per_frame > 0) || (pass_mask & UH_PASS_GBUFFER);
   if (primary_rays)
      if (int st = ensure_camera_grid(c, fp, batch)) return st;
   // with the camera grid nothing but bounce 0's own kernels reads a primary ray's state: it is not stored
   fp.primary_implicit = (c->primary_implicit && c->cam.this_frame && fp.samples_per_frame == 1) ? 1u : 0u;
   bs.pass_mask = pass_mask;
   bs.batch = batch;
   bs.restir_frame = (pass_mask & UH_PASS_RESTIR) != 0;
   // the path tracer reads spatial_reuse_reservoirs when it samples lights from them (rgen:98)
   bs.reads_reservoirs = (pass_mask & UH_PASS_REFERENCE_PT) && fp.lights_enabled == 1 && fp.use_ris == 1;

   if (batch > 1 && !(pass_mask & UH_PASS_REFERENCE_PT)) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frames: a batch needs the path-tracing pass");
   if (batch > kRestirBatch && bs.restir_frame) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frames: more reservoir-pass frames in one batch than the spatial ring holds");
   c->t_start = c->t_stop = nullptr;
   // the slot each frame of the batch samples lights from (rgen:98): without reservoir passes in this call, the current one
   for (uint32_t f = 0; f < kMaxBatchFrames; f++) bs.read_slot[f] = c->spatial_cur;

   if (bs.restir_frame) {
      if (!c->restir_stream) {
         HIP_TRY(c, hipStreamCreateWithFlags(&c->restir_stream, hipStreamNonBlocking));
         HIP_TRY(c, hipEventCreateWithFlags(&c->ev_restir, hipEventDisableTiming));
         HIP_TRY(c, hipEventCreate(&c->rs_start));
         HIP_TRY(c, hipEventCreate(&c->rs_stop));
      }
      if (!c->spatial_ring.p) {
         HIP_TRY(c, c->spatial_ring.alloc((size_t)(kSpatialRing - 1) * c->res_stride));
         // every slot is written before it is read - by this context's passes; under a row partition other ranks' bands arrive by
         // the exchange, and a caller that times one rank without one (exchange == NULL) must still read defined reservoirs
         if (c->bands.world > 1) HIP_TRY(c, hipMemsetAsync(c->spatial_ring.p, 0, c->spatial_ring.n * sizeof(UhReservoir), c->restir_stream));
         HIP_TRY(c, hipStreamSynchronize(c->stream));  // slot 0 (zeroed at creation or uh_write_reservoirs) is the history
      }
      bs.rc = cfg(c);
      bs.rc.stream = c->restir_stream;
      HIP_TRY(c, hipEventRecord(c->rs_start, c->restir_stream));
      c->t_start = c->rs_start;
   }
   return UH_OK;
}

// G-buffer cast and reservoir chain of frame f of the batch, on the reservoir stream
static int batch_restir_frame(uh_ctx* c, uh_batch& bs, uint32_t f) {
   if (!bs.restir_frame) return UH_OK;
   HIP_TRY(c, hipSetDevice(c->device));
   const uint32_t pass_mask = bs.pass_mask;
   const size_t npix = (size_t)c->W * c->H;
   FrameParams ff = bs.fp;  // frame f of the batch: its own RNG frame number (the reservoir kernels read nothing else per frame)
   ff.frame_number = bs.fp.frame_numbers[f];
   ff.total_samples = bs.fp.total_samples_of[f];
   UhRestirRows rows;
   restir_rows(c, rows);
   const RowSpans band = spans_of(c, rows.band_row0, rows.band_rows, 0, 0);
   const RowSpans reuse = spans_of(c, rows.reuse_row0, rows.reuse_rows, rows.reuse_extra_row0, rows.reuse_extra_rows);
   const RowSpans cast = spans_of(c, rows.cast_row0, rows.cast_rows, rows.cast_extra_row0, rows.cast_extra_rows);
   Images im = c->im;
   im.prev_spatial = spatial_buf(c, c->spatial_cur);
   im.reservoirs[2] = spatial_buf(c, c->spatial_cur);
   if (pass_mask & UH_PASS_GBUFFER) {
      if (!c->gb_hit.p) {
         HIP_TRY(c, c->gb_ray_o.alloc(npix));
         HIP_TRY(c, c->gb_ray_d.alloc(npix));
         HIP_TRY(c, c->gb_hit.alloc(npix));
      }
      const RawRays gps{c->gb_ray_o.p, c->gb_ray_d.p, c->gb_hit.p};
      launch_gbuffer(bs.rc, ff, c->scene, gps, im, c->dstats.p, cast, band.total(), c->cam.this_frame ? &c->cam.dev : nullptr);
   }
   if (pass_mask & UH_PASS_RESET_RESERVOIRS) launch_reset_reservoirs(bs.rc, ff, im, reuse);
   if (pass_mask & UH_PASS_INITIAL_RIS) launch_initial_ris(bs.rc, ff, c->scene, im, reuse);
   if (pass_mask & UH_PASS_TEMPORAL_REUSE) launch_temporal_reuse(bs.rc, ff, c->scene, im, reuse);
   if (pass_mask & UH_PASS_SPATIAL_REUSE) {
      // writes the NEXT slot of the ring: the path-tracing wavefronts that still read the current one keep going
      const int nxt = (c->spatial_cur + 1) % kSpatialRing;
      if (c->spatial_reader[nxt]) HIP_TRY(c, hipStreamWaitEvent(c->restir_stream, c->spatial_reader[nxt], 0));
      im.reservoirs[2] = spatial_buf(c, nxt);
      launch_spatial_reuse(bs.rc, ff, c->scene, im, band);
      c->spatial_cur = nxt;
      c->im.reservoirs[2] = spatial_buf(c, nxt);
      if (c->bands.world > 1) {
         if (!c->ev_band[nxt]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_band[nxt], hipEventDisableTiming));
         HIP_TRY(c, hipEventRecord(c->ev_band[nxt], c->restir_stream));
      }
   }
   bs.read_slot[f] = c->spatial_cur;
   return UH_OK;
}

// the other ranks' bands of the buffer frame f's spatial pass wrote (uh_set_restir_partition)
static int batch_exchange(uh_ctx* c, uh_batch& bs, uint32_t f) {
   (void)f;
   if (!bs.restir_frame || !c->bands.exchange || !(bs.pass_mask & UH_PASS_SPATIAL_REUSE)) return UH_OK;  // world 1 with an exchange: a one-rank all-gather (rehearsals)
   HIP_TRY(c, hipSetDevice(c->device));
   const uint64_t band_bytes = (uint64_t)c->bands.rows * c->W * sizeof(UhReservoir);
   if (int st = c->bands.exchange(c->bands.user, (void*)c->restir_stream, (void*)c->im.reservoirs[2], band_bytes, c->bands.rank, c->bands.world))
      return fail(c, UH_ERR_HIP, std::string("the reservoir exchange reported error ") + std::to_string(st));
   return UH_OK;
}

static int batch_end(uh_ctx* c, uh_batch& bs) {
   HIP_TRY(c, hipSetDevice(c->device));
   FrameParams& fp = bs.fp;
   const uint32_t batch = bs.batch;
   if (bs.restir_frame) {
      HIP_TRY(c, hipEventRecord(c->ev_restir, c->restir_stream));
      c->restir_recorded = true;
      HIP_TRY(c, hipEventRecord(c->rs_stop, c->restir_stream));
      c->t_stop = c->rs_stop;
   }
   for (uint32_t f = 0; f < kMaxBatchFrames; f++) fp.spatial_of[f] = spatial_buf(c, bs.read_slot[f < batch ? f : 0]);

   if (bs.pass_mask & UH_PASS_REFERENCE_PT) {
      c->sun.this_frame = false;
      if (fp.sun_shadow_enabled == 1 && fp.num_bounces > 0 && fp.samples_per_frame > 0)
         if (int st = ensure_sun_grid(c, fp.sun_dir)) return st;
      const uint32_t in_flight = c->frames_in_flight ? c->frames_in_flight : 1;
      const uint32_t si = c->next_slot;
      c->next_slot = (c->next_slot + 1) % in_flight;
      int st = ensure_slot(c, si, batch);
      if (st != UH_OK) return st;
      Slot& s = c->slots[si];
      // rgen:98 reads this frame's spatial_reuse_reservoirs
      if (bs.reads_reservoirs && c->restir_recorded) HIP_TRY(c, hipStreamWaitEvent(s.stream, c->ev_restir, 0));
      HIP_TRY(c, hipEventRecord(s.frame_start, s.stream));
      if (!c->t_start) c->t_start = s.frame_start;
      st = enqueue_path_trace(c, s, fp);
      if (st != UH_OK) return st;
      if (bs.reads_reservoirs)
         for (uint32_t f = 0; f < batch; f++) c->spatial_reader[bs.read_slot[f]] = s.ev_acc;
      HIP_TRY(c, hipEventRecord(s.frame_stop, s.stream));
      c->t_stop = s.frame_stop;
   }
   c->frame_timed = true;
   c->frames += batch;
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

static int render_batch(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t batch) {
   uh_batch bs;
   if (int st = batch_begin(c, view, pass_mask, batch, bs)) return st;
   for (uint32_t f = 0; f < batch; f++) {
      if (int st = batch_restir_frame(c, bs, f)) return st;
      if (int st = batch_exchange(c, bs, f)) return st;
   }
   return batch_end(c, bs);
}

// frames one wavefront carries for this pass mask (frame_plan.h plan_batch_size), and the slots it will rotate through
static int plan_batch(uh_ctx* c, uint32_t pass_mask, uint32_t* out_batch) {
   const uint32_t batch = plan_batch_size(c->batch_frames, c->tiles.n_owned ? c->tiles.n_owned : (uint64_t)c->W * c->H, pass_mask);
   // create every frames-in-flight slot now: the first call (an application's first frames, a benchmark's
   // warm-up) pays for the allocations and stream creation, not whichever later wavefront first reaches a slot
   if (pass_mask & UH_PASS_REFERENCE_PT)
      for (uint32_t i = 0; i < (c->frames_in_flight ? c->frames_in_flight : 1); i++)
         if (int st = ensure_slot(c, i, batch)) return st;
   *out_batch = batch;
   return UH_OK;
}

extern "C" {

// ---- the phases for an in-process group (csrc/context_internal.h; mgpu.hip) ----
int uhi_plan_batch(uh_ctx* c, uint32_t pass_mask, uint32_t* out_batch) {
   if (!c || !out_batch) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   return plan_batch(c, pass_mask, out_batch);
}
int uhi_batch_begin(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t batch, uh_batch** out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   uh_batch* bs = new uh_batch();
   int st = batch_begin(c, view, pass_mask, batch, *bs);
   if (st != UH_OK) {
      delete bs;
      bs = nullptr;
   }
   *out = bs;
   return st;
}
int uhi_batch_restir_frame(uh_ctx* c, uh_batch* bs, uint32_t f) { return (c && bs) ? batch_restir_frame(c, *bs, f) : UH_ERR_INVALID_ARGUMENT; }
int uhi_batch_end(uh_ctx* c, uh_batch* bs) {
   if (!c || !bs) return UH_ERR_INVALID_ARGUMENT;
   int st = batch_end(c, *bs);
   delete bs;
   return st;
}
void uhi_batch_abandon(uh_batch* bs) { delete bs; }
// what a peer pulls a band from / into: the buffer the last spatial pass wrote, the event recorded behind that pass, the
// stream the passes run on
int uhi_exchange_endpoints(uh_ctx* c, void** spatial_base, void** band_event, void** stream, uint64_t* band_bytes) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (spatial_base) *spatial_base = (void*)c->im.reservoirs[2];
   if (band_event) *band_event = (void*)c->ev_band[c->spatial_cur];
   if (stream) *stream = (void*)c->restir_stream;
   if (band_bytes) *band_bytes = (uint64_t)c->bands.rows * c->W * sizeof(UhReservoir);
   return UH_OK;
}

int uh_render_frame(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask) { return render_batch(c, view, pass_mask, 1); }

int uh_render_frames(uh_ctx* c, const UhViewUniformData* view, uint32_t pass_mask, uint32_t count) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!view || count == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_render_frames: null view or zero frames");
   UhViewUniformData v = *view;
   uint32_t done = 0, batch = 1;
   if (int st = plan_batch(c, pass_mask, &batch)) return st;
   const uint32_t even = even_piece(count, batch);
   while (done < count) {
      uint32_t b = count - done < even ? count - done : even;
      int st = render_batch(c, &v, pass_mask, b);
      if (st != UH_OK) return st;
      done += b;
      v.total_samples += b * v.samples_per_frame;
   }
   return UH_OK;
}

}  // extern "C"
