// context_internal.h — the phases of one batch of frames, for the in-process group (mgpu.hip). Not part of the C ABI
// (include/utopian_hip.h): uh_render_frame(s) runs these back to back on one context; a group interleaves them over its
// contexts because, with the reservoir passes partitioned by rows (uh_set_restir_partition), frame f + 1's temporal pass on
// one GPU reads the bands every other GPU wrote in frame f. The batch phases are frame_loop.hip's, the enqueued tile composition
// partition.hip's, the extraction entry points isosurface.hip's, uhi_mark_isosurface scene_build.hip's, the rest iso_update.hip's.
#pragma once
#include <cstdint>

#include "utopian_hip.h"

struct uh_batch;
extern "C" {
// ---- frame_loop.hip ----
int uhi_plan_batch(uh_ctx*, uint32_t pass_mask, uint32_t* out_batch);  // frames per wavefront for this pass mask; creates the slots
int uhi_batch_begin(uh_ctx*, const UhViewUniformData*, uint32_t pass_mask, uint32_t batch, uh_batch** out);
int uhi_batch_restir_frame(uh_ctx*, uh_batch*, uint32_t f);  // G-buffer cast + reservoir chain of frame f (this context's rows)
int uhi_batch_end(uh_ctx*, uh_batch*);                       // the path-tracing wavefront; frees the batch
void uhi_batch_abandon(uh_batch*);
// what a peer pulls a band from / into after uhi_batch_restir_frame: the buffer the spatial pass wrote, the event recorded
// behind it (hipEvent_t), the stream the passes run on (hipStream_t), bytes per band
int uhi_exchange_endpoints(uh_ctx*, void** spatial_base, void** band_event, void** stream, uint64_t* band_bytes);
// ---- context.hip ----
int uhi_iso_reference_triangulation(uh_ctx*);  // option "iso_reference_triangulation" (isosurface.hip)
// ---- partition.hip: composition of a tile-partitioned frame without a host wait (uh_rccl_gather_tiles, uh_mgpu_compose):
// pack this context's tiles into device_out on the context's stream (returned as hipStream_t), behind its frames in flight
int uhi_enqueue_pack_tiles(uh_ctx*, void* device_out, void** out_stream);
// the root: k_compose_tiles over device_all (world buffers of stride_pixels) on the context's stream, behind its frames in flight
// and behind the n_waits events (hipEvent_t) that say the other ranks' tiles have landed
int uhi_enqueue_compose_tiles(uh_ctx*, const void* device_all, uint64_t stride_pixels, uint32_t total_samples, uint32_t accumulation_limit, void* const* wait_events, int n_waits);
void* uhi_composed_event(uh_ctx*);  // hipEvent_t behind the context's last pack / composition (null before the first)
}
// the hybrid graph's marching-cubes pass (isosurface.hip): the reference's grid (marching_cubes.rs:17-45, kMcRes^3 cells of size 1 from
// the origin) at `time`, reference triangulation, enqueued on `stream` (hipStream_t). Count writes the triangles of each block of 256
// cells, x fastest (kMcBlocks of them); emit writes vertex 3 t + k of triangle t at block_offsets[block] (their exclusive scan) plus
// the block's prefix: pos and normal those of uh_add_isosurface_mesh(ctx, kMcRes, 0, kMcRes, time, ...), uv, colour and tangent zero.
// false when the case tables could not be loaded.
constexpr uint32_t kMcRes = 32, kMcBlocks = kMcRes * kMcRes * kMcRes / 256;
bool uhi_mc_extract_count(void* stream, float time, uint32_t* block_counts);
bool uhi_mc_extract_emit(void* stream, float time, const uint32_t* block_offsets, UhVertex* verts);
// the extraction of uh_add_isosurface_mesh / uh_update_isosurface_mesh (isosurface.hip) in its two halves, on `stream` (hipStream_t).
// uhi_iso_count_triangles: the triangles of each block of 256 cells, x fastest (uhi_iso_blocks(resolution) of them), scanned in place
// into block_counts (chunks: scan_chunk_count(blocks) words of scratch, d_total: one device word), waits and reads the 64-bit total
// back; false on a HIP error or when the case tables could not be loaded. uhi_iso_extract_emit (enqueued): vertex 3 t + k of
// triangle t at block_offsets[block] (that scan) plus the block's prefix.
uint32_t uhi_iso_blocks(uint32_t resolution);
bool uhi_iso_count_triangles(void* stream, uint32_t resolution, float lo, float hi, float time, bool reference, uint32_t* block_counts, uint32_t* chunks,
                             unsigned long long* d_total, unsigned long long* total);
bool uhi_iso_extract_emit(void* stream, uint32_t resolution, float lo, float hi, float time, bool reference, const uint32_t* block_offsets, UhVertex* verts);
// scene_build.hip: mesh `mesh_index` was made by uh_add_isosurface_mesh with these parameters (uh_update_isosurface_mesh re-extracts with them)
extern "C" int uhi_mark_isosurface(uh_ctx*, uint32_t mesh_index, uint32_t resolution, float lo, float hi, int reference);
// iso_update.hip: what feeds a device-resident mesh's consumers from its device vertices, enqueued on `stream`.
// uhi_iso_scatter: per triangle p of the mesh (vertices 3 p .. 3 p + 2) the on-device build's sources - 9 corner floats, key = mesh << 22 | p,
// the 64-byte shade packet - at corners / keys / shade (already offset to the mesh's range), and the mesh's object-space box folded into
// box[0..2] (minima) / box[3..5] (maxima) as ordered integers: initialise them to 0xffffffff / 0 and read them with uhi_box_decode.
void uhi_iso_scatter(void* stream, const UhVertex* verts, uint32_t num_tris, uint32_t mesh, float* corners, uint32_t* keys, float4* shade, uint32_t* box);
void uhi_iota(void* stream, uint32_t* out, uint32_t n);
void uhi_fill_u32(void* stream, uint32_t* out, uint32_t n, uint32_t value);
float uhi_box_decode(uint32_t ordered);
