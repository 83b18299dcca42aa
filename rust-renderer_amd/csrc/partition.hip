// partition.hip — a frame split over several GPUs, on the host: the tile partition of the path-traced frame (uh_set_tile_partition; the
// owner rule is tile_partition.h, the kernels tiles.hip), the composition of its tiles - blocking (uh_pack_tiles, uh_unpack_tiles,
// uh_compose_tiles) and enqueued (uhi_enqueue_*, for mgpu.hip and rccl_link.hip) -, and the band partition of the reservoir passes
// (uh_set_restir_partition). Host code only; struct uh_ctx (its members `tiles` and `bands`) is context_state.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "context_internal.h"
#include "context_state.h"
#include "device_types.h"
#include "tile_partition.h"
#include "utopian_hip.h"

using namespace uh;

// rows of this context's reservoir passes (uh_set_restir_partition): its band, the band's 30-row neighbourhood (plus the last
// row for the first band: spatial_reuse.rgen:54's wrapped offset is clamped to size - 1), and for the G-buffer cast the row
// above each of those (the 2 x 2 corner filter)
void restir_rows(const uh_ctx* c, UhRestirRows& r) {
   const uint32_t H = c->H, B = c->bands.world > 1 ? c->bands.rows : H;
   r = UhRestirRows{};
   r.rows_per_band = B;
   const uint32_t b0 = std::min<uint64_t>((uint64_t)c->bands.rank * B, H), b1 = std::min<uint64_t>((uint64_t)b0 + B, H);
   r.band_row0 = b0;
   r.band_rows = b1 - b0;
   if (b1 == b0) return;  // more ranks than bands: nothing to do here
   const uint32_t halo = 30;
   const uint32_t t0 = b0 > halo ? b0 - halo : 0, t1 = std::min<uint64_t>((uint64_t)b1 + halo, H);
   r.reuse_row0 = t0;
   r.reuse_rows = t1 - t0;
   if (b0 < halo && t1 < H) {
      r.reuse_extra_row0 = H - 1;
      r.reuse_extra_rows = 1;
   }
   const uint32_t g0 = t0 > 0 ? t0 - 1 : 0;
   r.cast_row0 = g0;
   r.cast_rows = t1 - g0;
   if (r.reuse_extra_rows) {
      const uint32_t e0 = std::max(H >= 2 ? H - 2 : 0u, t1);  // rows H - 2 and H - 1, without what the first interval already holds
      r.cast_extra_row0 = e0;
      r.cast_extra_rows = H - e0;
   }
}

uint64_t max_pack_pixels(uh_ctx* c) { return pack_pixels(c->W, c->H, c->tiles.tile, 0, c->tiles.world); }  // (no rank owns more tiles than rank 0)
// what was just enqueued on the context's stream read or wrote the accumulation image: the next frame's accumulate tail
// (enqueue_path_trace) and the next composition wait for it
int mark_composed(uh_ctx* c) {
   uh_ctx::Tiles& t = c->tiles;
   if (!t.ev_compose) HIP_TRY(c, hipEventCreateWithFlags(&t.ev_compose, hipEventDisableTiming));
   HIP_TRY(c, hipEventRecord(t.ev_compose, c->stream));
   c->last_acc = t.ev_compose;
   return UH_OK;
}

namespace {

// ---- the launches that a blocking verb and its enqueued twin share, on the context's stream, and the two ways a verb runs one ----
void launch_pack(uh_ctx* c, void* device_out) {
   launch_pack_tiles(cfg(c), c->accumulation.p, (float4*)device_out, c->W, c->H, c->tiles.rank, c->tiles.world, c->tiles.tile);
}
void launch_compose(uh_ctx* c, const void* device_all, uint64_t stride_pixels, uint32_t total_samples, uint32_t accumulation_limit) {
   launch_compose_tiles(cfg(c), c->im, (const float4*)device_all, stride_pixels, c->W, c->H, c->tiles.rank, c->tiles.world, c->tiles.tile, total_samples, accumulation_limit);
}
// `device_all` can be composed from: world buffers of stride_pixels, each long enough for any rank's packed tiles
bool composable(uh_ctx* c, const void* device_all, uint64_t stride_pixels) { return device_all && stride_pixels >= max_pack_pixels(c); }

// BLOCKING: behind everything the context has in flight, and waited for. Touches neither last_acc nor the compose event
template <class Launch>
int run_blocking(uh_ctx* c, Launch&& launch) {
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   launch();
   HIP_TRY(c, hipStreamSynchronize(c->stream));
   return UH_OK;
}
// ENQUEUED: behind the accumulate tail of every frame in flight and behind the `n_waits` events; nothing waits on the host, and the
// next frame's tail waits for this (mark_composed)
template <class Launch>
int run_enqueued(uh_ctx* c, void* const* wait_events, int n_waits, Launch&& launch) {
   HIP_TRY(c, hipSetDevice(c->device));
   if (c->last_acc) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->last_acc, 0));
   for (int k = 0; k < n_waits; k++)
      if (wait_events[k]) HIP_TRY(c, hipStreamWaitEvent(c->stream, (hipEvent_t)wait_events[k], 0));
   launch();
   HIP_TRY(c, hipGetLastError());
   return mark_composed(c);
}

}  // namespace

extern "C" {

int uh_set_tile_partition(uh_ctx* c, uint32_t rank, uint32_t world, uint32_t tile_size) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (world == 0 || rank >= world || tile_size == 0) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_tile_partition: need rank < world, tile_size > 0");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   uh_ctx::Tiles& t = c->tiles;
   t.rank = rank;
   t.world = world;
   t.tile = tile_size;
   t.n_owned = c->W * c->H;
   t.owned_pixels.release();
   if (world > 1) {
      const uint32_t tiles_x = tiles_across(c->W, tile_size);
      std::vector<uint32_t> own;
      own.reserve((size_t)c->W * c->H / world + 1);
      for (uint32_t y = 0; y < c->H; y++)
         for (uint32_t x = 0; x < c->W; x++)
            if (pixel_owner(x, y, tile_size, tiles_x, world) == rank) own.push_back(y * c->W + x);
      t.n_owned = (uint32_t)own.size();
      HIP_TRY(c, t.owned_pixels.alloc(own.size() ? own.size() : 1));
      if (!own.empty()) HIP_TRY(c, hipMemcpy(t.owned_pixels.p, own.data(), own.size() * 4, hipMemcpyHostToDevice));
   }
   return UH_OK;
}

int uh_tile_pack_count(uh_ctx* c, uint32_t rank, uint64_t* out_pixels) {
   if (!c || !out_pixels) return UH_ERR_INVALID_ARGUMENT;
   if (rank >= c->tiles.world) return fail(c, UH_ERR_INVALID_ARGUMENT, "rank >= world");
   *out_pixels = pack_pixels(c->W, c->H, c->tiles.tile, rank, c->tiles.world);
   return UH_OK;
}

int uh_pack_tiles(uh_ctx* c, void* device_out, uint64_t capacity_pixels) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!device_out || capacity_pixels < pack_pixels(c->W, c->H, c->tiles.tile, c->tiles.rank, c->tiles.world))
      return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_pack_tiles: buffer too small");
   return run_blocking(c, [&] { launch_pack(c, device_out); });
}

int uh_unpack_tiles(uh_ctx* c, uint32_t from_rank, const void* device_in, uint64_t num_pixels) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   uint64_t need = 0;
   if (uh_tile_pack_count(c, from_rank, &need) != UH_OK) return UH_ERR_INVALID_ARGUMENT;
   if (!device_in || num_pixels < need) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_unpack_tiles: buffer too small");
   return run_blocking(c, [&] { launch_unpack_tiles(cfg(c), c->accumulation.p, (const float4*)device_in, c->W, c->H, from_rank, c->tiles.world, c->tiles.tile); });
}

int uh_compose_tiles(uh_ctx* c, const void* device_all, uint64_t stride_pixels, uint32_t total_samples, uint32_t accumulation_limit) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (!composable(c, device_all, stride_pixels)) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_compose_tiles: stride smaller than a rank's packed tiles");
   return run_blocking(c, [&] { launch_compose(c, device_all, stride_pixels, total_samples, accumulation_limit); });
}

int uh_resolve_output(uh_ctx* c, uint32_t total_samples, uint32_t accumulation_limit) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   launch_resolve(cfg(c), c->im, c->W, c->H, total_samples, accumulation_limit);
   HIP_TRY(c, hipGetLastError());
   return UH_OK;
}

// ---- composition of a tile-partitioned frame, ENQUEUED (context_internal.h) ----
// this context's owned tiles, packed into `device_out` (>= uh_tile_pack_count pixels), on the context's stream behind the accumulate
// tail of every frame in flight
int uhi_enqueue_pack_tiles(uh_ctx* c, void* device_out, void** out_stream) {
   if (!c || !device_out) return UH_ERR_INVALID_ARGUMENT;
   if (out_stream) *out_stream = (void*)c->stream;
   return run_enqueued(c, nullptr, 0, [&] { launch_pack(c, device_out); });
}
// the root's composition (k_compose_tiles over `device_all`: world buffers of stride_pixels, uh_compose_tiles' layout) on the context's
// stream, behind its own frames in flight and behind the `n_waits` events (hipEvent_t) that say the other ranks' tiles have landed
int uhi_enqueue_compose_tiles(uh_ctx* c, const void* device_all, uint64_t stride_pixels, uint32_t total_samples, uint32_t accumulation_limit, void* const* wait_events,
                              int n_waits) {
   if (!c || !composable(c, device_all, stride_pixels)) return UH_ERR_INVALID_ARGUMENT;
   return run_enqueued(c, wait_events, n_waits, [&] { launch_compose(c, device_all, stride_pixels, total_samples, accumulation_limit); });
}
// the event behind this context's last pack / composition (hipEvent_t; null before the first)
void* uhi_composed_event(uh_ctx* c) { return c ? (void*)c->tiles.ev_compose : nullptr; }

int uh_set_restir_partition(uh_ctx* c, uint32_t rank, uint32_t world, UhRestirExchangeFn exchange, void* user) {
   if (!c) return UH_ERR_INVALID_ARGUMENT;
   if (world == 0 || rank >= world) return fail(c, UH_ERR_INVALID_ARGUMENT, "uh_set_restir_partition: need rank < world");
   HIP_TRY(c, hipSetDevice(c->device));
   if (int st = sync_all(c)) return st;
   const size_t npix = (size_t)c->W * c->H;
   const uint32_t band_rows = (c->H + world - 1) / world;
   const size_t stride = std::max(npix, (size_t)band_rows * world * c->W);
   if (stride != c->res_stride) {
      // the history (the current slot of the ring) moves into a buffer of the new length, which becomes slot 0
      DevBuf<UhReservoir> fresh;
      HIP_TRY(c, fresh.alloc(stride));
      HIP_TRY(c, hipMemsetAsync(fresh.p, 0, stride * sizeof(UhReservoir), c->stream));
      HIP_TRY(c, hipMemcpyAsync(fresh.p, c->im.reservoirs[2], npix * sizeof(UhReservoir), hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      std::swap(c->reservoirs[2], fresh);
      fresh.release();
      c->spatial_ring.release();
      c->res_stride = stride;
   } else if (c->spatial_cur != 0) {
      HIP_TRY(c, hipMemcpyAsync(c->reservoirs[2].p, c->im.reservoirs[2], npix * sizeof(UhReservoir), hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
   }
   c->spatial_cur = 0;
   for (auto& r : c->spatial_reader) r = nullptr;
   c->im.reservoirs[2] = c->reservoirs[2].p;
   c->im.prev_spatial = c->reservoirs[2].p;
   c->bands.rank = rank;
   c->bands.world = world;
   c->bands.rows = world > 1 ? band_rows : c->H;
   c->bands.exchange = exchange;
   c->bands.user = user;
   return UH_OK;
}

int uh_get_restir_rows(uh_ctx* c, UhRestirRows* out) {
   if (!c || !out) return UH_ERR_INVALID_ARGUMENT;
   restir_rows(c, *out);
   return UH_OK;
}

}  // extern "C"
