/*
 * utopian_hip.h — C ABI of libutopian_hip.so: the MI355X (gfx950) replacement for the
 * reference's path-tracing + ReSTIR render-graph nodes.
 *
 * Every entry point below replaces one verb of the reference's Rust/Vulkan surface for this
 * path (citations are relative to the reference checkout):
 *
 *   uh_create                 Renderer::new + Raytracing::new + the graph resources of
 *                             build_path_tracing_render_graph   (utopian/src/renderer.rs:123,
 *                             utopian/src/raytracing.rs:36, utopian/src/renderers/mod.rs:199-244)
 *   uh_add_texture_rgba8      Renderer::add_bindless_texture    (utopian/src/renderer.rs:301)
 *   uh_add_mesh               Renderer::add_model, per mesh     (utopian/src/renderer.rs:222-299)
 *                             + one row of fill_instance_array  (utopian/src/raytracing.rs:218-277)
 *   uh_add_light              Renderer::add_light               (utopian/src/renderer.rs:391-410)
 *   uh_set_instance_transform gizmo edit + rebuild_tlas         (utopian/src/raytracing.rs:400-459)
 *   uh_build_acceleration     Raytracing::initialize            (utopian/src/raytracing.rs:89-111)
 *   uh_render_frame           the 6 graph passes gbuffer→reset→initial_ris→temporal→spatial→pt
 *                             (utopian/src/renderers/mod.rs:246-358), one ViewUniformData memcpy
 *                             per frame (prototype/src/main.rs:477-478)
 *   uh_render_frames          the same node for N consecutive frames of a static camera (batched)
 *   uh_reset_accumulation     total_samples = 0 semantics       (prototype/src/main.rs:400-413)
 *   uh_read_*                 pt_accumulation_image / pt_output_image / reservoir SSBO read-back
 *   uh_set_tile_partition,
 *   uh_pack_tiles, uh_unpack_tiles, uh_resolve_output
 *                             multi-GPU framebuffer tile partition; no reference counterpart
 *                             (the reference is single-device, utopian/src/device.rs:45)
 *   uh_set_restir_partition, uh_rccl_attach
 *                             multi-GPU partition of the reservoir passes by bands of rows with one
 *                             all-gather of spatial_reuse_reservoirs per frame (temporal_reuse.rgen:90-99,
 *                             spatial_reuse.rgen:40-60 read across any pixel partition)
 *
 * Contract: plain C, POD in / status out, no exceptions cross the boundary. One context per
 * GPU; all calls on one context are serialised by the caller (the reference has a single render
 * thread, utopian/src/graph.rs:1004-1007). The library fails loudly (UH_ERR_NO_DEVICE) when no
 * HIP device is present: there is no CPU fallback.
 */
#ifndef UTOPIAN_HIP_H
#define UTOPIAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- POD structs, byte-identical to the reference's GPU structs ------------------------ */

/* utopian/src/primitive.rs:9-17 == shaders/include/bindless.glsl:4-11 (std430, 80 B) */
typedef struct UhVertex {
   float pos[4];     /* @0  */
   float normal[4];  /* @16 */
   float uv[2];      /* @32 */
   float _pad[2];    /* @40 */
   float color[4];   /* @48 */
   float tangent[4]; /* @64 */
} UhVertex;

/* utopian/src/renderer.rs:20-36 == bindless.glsl:13-28 (scalar layout, 64 B) */
typedef struct UhGpuMaterial {
   uint32_t diffuse_map;
   uint32_t normal_map;
   uint32_t metallic_roughness_map;
   uint32_t occlusion_map;
   float base_color_factor[4];   /* @16 */
   float metallic_factor;        /* @32 */
   float roughness_factor;       /* @36 */
   float padding[2];             /* @40 */
   float raytrace_properties[4]; /* @48: x = 0 lambertian,1 metal,2 dielectric,3 diffuse light (reference.rchit:47-89), 4 = Cook-Torrance from
                                  * metallic_factor / roughness_factor (extension, SURVEY 8f N2: no reference scene uses it); y = fuzz | ior */
} UhGpuMaterial;

/* utopian/src/renderer.rs:38-44 (12 B) */
typedef struct UhGpuMesh {
   uint32_t vertex_buffer;
   uint32_t index_buffer;
   uint32_t material;
} UhGpuMesh;

/* utopian/src/renderer.rs:46-59 == bindless.glsl:37-49 (scalar layout, 96 B) */
typedef struct UhGpuLight {
   float color[4];       /* @0  */
   float position[3];    /* @16 */
   float range;          /* @28 */
   float direction[3];   /* @32 */
   float spot;           /* @44 */
   float attenuation[3]; /* @48 */
   float light_type;     /* @60 */
   float intensity[3];   /* @64 */
   float id;             /* @76 */
   float padding[4];     /* @80 */
} UhGpuLight;

/* utopian/src/renderer.rs:84-120 == shaders/include/view.glsl:1-35 (std140, 448 B).
 * Matrices are column-major (glam::Mat4): m[c*4 + r]. */
typedef struct UhViewUniformData {
   float view[16];                       /* @0   */
   float projection[16];                 /* @64  */
   float inverse_view[16];               /* @128 */
   float inverse_projection[16];         /* @192 */
   float prev_frame_projection_view[16]; /* @256 */
   float eye_pos[3];                     /* @320 */
   uint32_t samples_per_frame;           /* @332 */
   float sun_dir[3];                     /* @336 */
   uint32_t total_samples;               /* @348 */
   uint32_t num_bounces;                 /* @352 */
   uint32_t viewport_width;              /* @356 */
   uint32_t viewport_height;             /* @360 */
   float time;                           /* @364 */
   uint32_t num_lights;                  /* @368 */
   uint32_t shadows_enabled;             /* @372 */
   uint32_t ssao_enabled;                /* @376 */
   uint32_t fxaa_enabled;                /* @380 */
   uint32_t cubemap_enabled;             /* @384 */
   uint32_t ibl_enabled;                 /* @388 */
   uint32_t sky_enabled;                 /* @392 */
   uint32_t sun_shadow_enabled;          /* @396 */
   uint32_t lights_enabled;              /* @400 */
   uint32_t max_num_lights_used;         /* @404 */
   uint32_t marching_cubes_enabled;      /* @408 */
   uint32_t temporal_reuse_enabled;      /* @412 */
   uint32_t spatial_reuse_enabled;       /* @416 */
   uint32_t rebuild_tlas;                /* @420 */
   uint32_t accumulation_limit;          /* @424 */
   uint32_t use_ris_light_sampling;      /* @428 */
   uint32_t raytracing_supported;        /* @432 */
   uint32_t _tail_pad[3];                /* @436 → 448 */
} UhViewUniformData;

/* shaders/include/restir_sampling.glsl:51-57 (16 B) */
typedef struct UhReservoir {
   int32_t Y;
   float W_sum;
   float W_X;
   int32_t M;
} UhReservoir;

/* ---- compile-time layout guard: a C11 / C++11 consumer (or a bindgen run over this header)
 * learns of a packing mismatch when it compiles, not at run time. Sizes and offsets are the reference's. */
#include <stddef.h>
#if defined(__cplusplus)
#define UH_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define UH_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#else
#define UH_LAYOUT_ASSERT(cond, msg) typedef char uh_layout_assert_[(cond) ? 1 : -1]
#endif
UH_LAYOUT_ASSERT(sizeof(UhVertex) == 80 && offsetof(UhVertex, normal) == 16 && offsetof(UhVertex, uv) == 32 && offsetof(UhVertex, color) == 48 &&
                    offsetof(UhVertex, tangent) == 64, "UhVertex: std430 Vertex of bindless.glsl:4-11 (80 B)");
UH_LAYOUT_ASSERT(sizeof(UhGpuMaterial) == 64 && offsetof(UhGpuMaterial, base_color_factor) == 16 && offsetof(UhGpuMaterial, metallic_factor) == 32 &&
                    offsetof(UhGpuMaterial, roughness_factor) == 36 && offsetof(UhGpuMaterial, raytrace_properties) == 48, "UhGpuMaterial: renderer.rs:20-36 (64 B)");
UH_LAYOUT_ASSERT(sizeof(UhGpuMesh) == 12, "UhGpuMesh: renderer.rs:38-44 (12 B)");
UH_LAYOUT_ASSERT(sizeof(UhGpuLight) == 96 && offsetof(UhGpuLight, position) == 16 && offsetof(UhGpuLight, range) == 28 && offsetof(UhGpuLight, direction) == 32 &&
                    offsetof(UhGpuLight, attenuation) == 48 && offsetof(UhGpuLight, light_type) == 60 && offsetof(UhGpuLight, intensity) == 64 &&
                    offsetof(UhGpuLight, id) == 76, "UhGpuLight: renderer.rs:46-59 (96 B)");
UH_LAYOUT_ASSERT(sizeof(UhViewUniformData) == 448 && offsetof(UhViewUniformData, inverse_view) == 128 && offsetof(UhViewUniformData, prev_frame_projection_view) == 256 &&
                    offsetof(UhViewUniformData, eye_pos) == 320 && offsetof(UhViewUniformData, samples_per_frame) == 332 && offsetof(UhViewUniformData, sun_dir) == 336 &&
                    offsetof(UhViewUniformData, total_samples) == 348 && offsetof(UhViewUniformData, num_bounces) == 352 && offsetof(UhViewUniformData, time) == 364 &&
                    offsetof(UhViewUniformData, sky_enabled) == 392 && offsetof(UhViewUniformData, sun_shadow_enabled) == 396 &&
                    offsetof(UhViewUniformData, lights_enabled) == 400 && offsetof(UhViewUniformData, max_num_lights_used) == 404 &&
                    offsetof(UhViewUniformData, temporal_reuse_enabled) == 412 && offsetof(UhViewUniformData, spatial_reuse_enabled) == 416 &&
                    offsetof(UhViewUniformData, accumulation_limit) == 424 && offsetof(UhViewUniformData, use_ris_light_sampling) == 428 &&
                    offsetof(UhViewUniformData, raytracing_supported) == 432, "UhViewUniformData: std140 UBO_view of view.glsl:1-35 (448 B)");
UH_LAYOUT_ASSERT(sizeof(UhReservoir) == 16 && offsetof(UhReservoir, W_sum) == 4 && offsetof(UhReservoir, W_X) == 8 && offsetof(UhReservoir, M) == 12,
                 "UhReservoir: restir_sampling.glsl:51-57 (16 B)");

/* ---- pass mask for uh_render_frame (pass order of renderers/mod.rs:246-358) -------------- */
enum {
   UH_PASS_GBUFFER = 1u << 0,        /* gbuffer_pass (position only; produced by primary-ray cast) */
   UH_PASS_RESET_RESERVOIRS = 1u << 1,
   UH_PASS_INITIAL_RIS = 1u << 2,
   UH_PASS_TEMPORAL_REUSE = 1u << 3,
   UH_PASS_SPATIAL_REUSE = 1u << 4,
   UH_PASS_REFERENCE_PT = 1u << 5,
   UH_PASS_RESTIR = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 3) | (1u << 4),
   UH_PASS_ALL = 0x3f
};

/* ---- status codes ---------------------------------------------------------------------- */
enum {
   UH_OK = 0,
   UH_ERR_INVALID_ARGUMENT = 1,
   UH_ERR_NO_DEVICE = 2,
   UH_ERR_HIP = 3,
   UH_ERR_CAPACITY = 4,   /* > 1024 materials/meshes/lights (utopian/src/renderer.rs:5-7) */
   UH_ERR_NOT_BUILT = 5,  /* render before uh_build_acceleration */
   UH_ERR_OUT_OF_MEMORY = 6
};

enum { UH_MAX_GPU_MATERIALS = 1024, UH_MAX_GPU_MESHES = 1024, UH_MAX_GPU_LIGHTS = 1024 };

/* ray kinds counted in UhStats.rays[] ("ray" = one traceRayEXT-equivalent query) */
enum { UH_RAY_PRIMARY = 0, UH_RAY_BOUNCE = 1, UH_RAY_SUN_SHADOW = 2, UH_RAY_LIGHT_SHADOW = 3, UH_RAY_GBUFFER = 4, UH_RAY_KINDS = 5 };

typedef struct UhStats {
   uint64_t rays[UH_RAY_KINDS]; /* since the last uh_reset_stats */
   uint64_t nodes_visited;      /* BVH4 nodes fetched by closest-hit traversals (only with uh_set_option("count_visits",1)) */
   uint64_t tris_tested;        /* triangle packets tested by closest-hit traversals (same option) */
   uint64_t shadow_nodes_visited;
   uint64_t shadow_tris_tested;
   uint64_t closest_hits;       /* closest-hit shader invocations for path rays */
   uint64_t misses;             /* miss (sky) evaluations for path rays */
   uint64_t frames;
   uint32_t bvh_nodes;          /* BVH4 node count */
   uint32_t bvh_triangles;
   float build_ms;              /* last uh_build_acceleration / uh_refit_acceleration, host wall time */
   float last_frame_ms;         /* hipEvent time of the last uh_render_frame (all passes) */
   float trace_closest_ms;      /* summed hipEvent time of closest-hit traversal launches since reset (option "time_kernels") */
   float trace_shadow_ms;       /* the sun shadow rays: grid kernel + the tree walk of what it hands over */
   float shade_ms;
   uint32_t trace_closest_launches;
   uint32_t sun_grid_cells;     /* the sun-direction visibility grid in use (0 = none: the sun shadow rays walk the tree) */
   uint32_t sun_grid_entries;   /* (triangle, cell) pairs it holds */
   float sun_grid_build_ms;     /* host time of its last build (once per sun direction and geometry) */
   float sun_grid_mean_list;    /* entries per occupied cell */
   uint64_t sun_tree_rays;      /* sun shadow rays the grid handed to the tree walk (border cells, long lists); part of rays[UH_RAY_SUN_SHADOW] */
   uint32_t camera_grid_cells;  /* the per-camera grid the primary rays go through (pixels; 0 = none: they walk the tree) */
   uint32_t camera_grid_entries;
   float camera_grid_build_ms;  /* host wall time of its last build (on the device; once per camera at rest and geometry) */
   float camera_grid_mean_list; /* entries per occupied pixel */
   uint64_t camera_tree_rays;   /* primary rays the grid handed to the tree walk (pixels with long lists); part of rays[UH_RAY_PRIMARY] */
   uint64_t camera_grid_tris_tested; /* triangle packets tested by the grid walk of the primary rays (option "count_visits") */
   float camera_grid_ms;        /* summed hipEvent time of the primary rays' launches when they go through the grid (option "time_kernels");
                                   0 for the passes whose first bounce is one kernel (option "fused_primary"): that kernel's time is part of shade_ms */
   float trace_light_ms;        /* summed hipEvent time of the light shadow rays' traversal launches (reference.rgen:106-124; option "time_kernels"); not part of trace_shadow_ms */
   uint64_t sun_covered_rays;   /* sun shadow rays answered by their cell's cover depth alone (option "count_visits") */
   uint64_t sun_grid_bytes;     /* device memory of the sun grid in use: cell records + entry lists + coarse cover + the lists as 64-byte records (when within "sun_grid_inline_max_mb") */
   uint64_t camera_grid_bytes;  /* device memory of the camera grid in use: cell offsets + entry lists */
   uint64_t light_nodes_visited; /* BVH4 nodes fetched / triangle packets tested by the light shadow rays' walks (option "count_visits"); */
   uint64_t light_tris_tested;   /* not part of shadow_nodes_visited / shadow_tris_tested, which count the sun rays */
   uint32_t trace_light_launches;
   uint32_t reserved1;
} UhStats;

typedef struct uh_ctx uh_ctx;

/* ---- Stream ordering (what a caller may rely on; tests/test_gpu_stream_order.py holds the library to it) ----------------
 * uh_render_frame / uh_render_frames ENQUEUE and return; up to "frames_in_flight" frames run on streams of their own, the
 * reservoir passes on another. Every other verb that reads or writes device state WAITS for all frames in flight first and
 * is COMPLETE when it returns (its own copies and clears are waited for: the next frame may run on any of the library's
 * streams, none of which is ordered against the null stream):
 *   waits + complete on return:  uh_reset_stats, uh_get_stats, uh_reset_accumulation, uh_synchronize, every uh_read_*,
 *        uh_write_reservoirs, uh_write_gbuffer_position, uh_build_acceleration, uh_refit_acceleration (also when uh_render_frame calls it for
 *        view->rebuild_tlas), uh_set_tile_partition, uh_set_restir_partition, uh_rccl_attach / uh_rccl_detach, uh_pack_tiles,
 *        uh_unpack_tiles, uh_compose_tiles, uh_resolve_output, uh_add_isosurface_mesh, uh_update_isosurface_mesh (it reads the
 *        triangle total, 8 bytes, back to size its buffers), uh_get_isosurface_update_stats, uh_update_mesh_vertices (device input:
 *        it reads a 4-byte verdict on the caller's buffer back before it takes it), uh_get_mesh_update_stats, uh_set_mesh_skin,
 *        uh_set_mesh_morph_targets (both upload into fresh buffers and take the bind pose), uh_pose_mesh (it reads a 4-byte verdict on the
 *        posed positions back before the mesh takes them), uh_get_pose_stats, uh_read_denoised,
 *        uh_get_denoise_stats, uh_reset_denoise_history, uh_get_rtao_stats, uh_get_rtao_visits, uh_get_motion_stats, uh_reset_taa_history,
 *        uh_get_taa_stats, uh_post_image, uh_read_post, uh_get_post_stats, uh_get_rtgi_stats, uh_get_glossy_stats, uh_get_fog_stats,
 *        uh_get_fog_visits, uh_get_glass_stats, uh_get_area_light_stats, uh_read_area_emitters, uh_destroy;
 *   enqueues like a frame, ordered behind the frames in flight and before those that follow:  uh_rccl_gather_tiles, uh_mgpu_compose;
 *        uh_set_option for "frames_in_flight" and for "time_kernels" 1 -> 0 (the others only change what the NEXT enqueued
 *        frame does: "furnace", "sun_grid*", "camera_grid*", "overlap", "batch_frames", "trace_blocks_per_cu", "count_visits",
 *        "full_frame_restir", "primary_implicit", "rtao_order", "rtgi_order", "fog_order", "area_light_order"; "device_build", "ploc_sah_top" invalidate the tree: the next frame
 *        needs uh_build_acceleration, which waits);
 *   host state only (no device access, nothing to wait for):  uh_add_mesh, uh_add_light, uh_set_instance_transform,
 *        uh_get_num_lights, uh_mesh_info, uh_read_mesh, uh_get_restir_rows, uh_tile_pack_count, uh_set_rtao_params, uh_set_taa_params,
 *        uh_set_post_params, uh_reset_post_exposure, uh_set_rtgi_params, uh_set_glossy_params, uh_set_fog_params, uh_set_glass_params, uh_set_area_light_params (read by the next uh_render_hybrid; the post
 *        pair also by the next uh_post_image), uh_taa_default_params, uh_taa_jitter, uh_post_default_params, uh_post_level_size,
 *        uh_rtgi_default_params, uh_glossy_default_params, uh_fog_default_params, uh_glass_default_params, uh_area_light_default_params,
 *        uh_last_error
 *        (uh_read_mesh of a mesh that uh_update_isosurface_mesh has made device-resident, or that uh_update_mesh_vertices last updated
 *        from a device pointer, copies it from the device: a blocking copy);
 *   uh_add_texture_rgba8 uploads into a fresh allocation no frame in flight can reference (textures enter a frame's tables at the
 *        next uh_build_acceleration) and is complete on return;
 *   uh_trace_closest / uh_trace_any run on the context's first stream, in order with the frames of that stream, read the scene
 *        only, and are complete on return;
 *   uh_render_hybrid enqueues like a frame, ordered behind the frames in flight and before those that follow (on the context's first
 *        stream, after a wait for the others); uh_read_hybrid and uh_get_hybrid_stats wait and are complete on return.
 *   uh_denoise enqueues like uh_render_hybrid; a frame enqueued after it accumulates behind its read of the accumulation image.
 * The sun-direction grid and the camera grid are (re)built inside the first frame call that wants them, after a wait for the frames in flight. */

/* ---- lifetime -------------------------------------------------------------------------- */
int uh_create(int device_ordinal, uint32_t width, uint32_t height, uh_ctx** out);
void uh_destroy(uh_ctx* ctx);
const char* uh_last_error(uh_ctx* ctx); /* ctx may be NULL: the last creation error - or, after a SUCCESSFUL uh_create, "" or a
                                         * "warning: ..." when the HIP runtime of the process is of another release (major.minor)
                                         * than the one the library was built with (also printed to stderr once per process) */
const char* uh_version(void);           /* "utopian-hip <v> (gfx950; built with HIP a.b.c; HIP runtime x.y.z)"; needs no GPU */
/* the same two releases as numbers, HIP_VERSION style (major * 10000000 + minor * 100000 + patch): the hipcc that compiled the
 * library, and hipRuntimeGetVersion() of the libamdhip64.so.7 this process bound (the soname covers every 7.x: a host that loaded
 * another copy first - the PyTorch wheel bundles one - hands it to this library as well). Either pointer may be NULL. */
int uh_hip_versions(int* built_with, int* runtime);

/* ---- scene ----------------------------------------------------------------------------- */
int uh_add_texture_rgba8(uh_ctx* ctx, const uint8_t* pixels, uint32_t w, uint32_t h, uint32_t* out_index);
/* material->diffuse_map must be an index returned by uh_add_texture_rgba8.
 * world3x4: row-major 3x4 object-to-world (VkTransformMatrixKHR layout, raytracing.rs:233-248). */
int uh_add_mesh(uh_ctx* ctx, const UhVertex* vertices, uint32_t num_vertices, const uint32_t* indices,
                uint32_t num_indices, const UhGpuMaterial* material, const float world3x4[12],
                uint32_t* out_mesh_index);
int uh_add_light(uh_ctx* ctx, const UhGpuLight* light, uint32_t* out_index);
int uh_get_num_lights(uh_ctx* ctx, uint32_t* out); /* Renderer::get_num_lights (renderer.rs:412) */
int uh_set_instance_transform(uh_ctx* ctx, uint32_t mesh_index, const float world3x4[12]);
int uh_build_acceleration(uh_ctx* ctx);
/* Raytracing::rebuild_tlas (raytracing.rs:400-459): after uh_set_instance_transform calls, re-bakes the
 * triangles and recomputes every box of the existing tree ON THE DEVICE (no host rebuild; topology kept).
 * Results equal a full uh_build_acceleration bit for bit - hits do not depend on the boxes - only the
 * traversal cost grows while instances drift from where the tree was built. UH_ERR_NOT_BUILT when meshes
 * or lights were added since the last build. uh_render_frame calls it by itself when transforms are
 * pending and view->rebuild_tlas == 1 (the flag the application sets, main.rs:392,526). */
int uh_refit_acceleration(uh_ctx* ctx);

/* ---- per frame ------------------------------------------------------------------------- */
/* UH_ERR_INVALID_ARGUMENT for view->num_bounces > 64, view->samples_per_frame > 4096, view->num_lights beyond the
 * lights added; UH_ERR_NOT_BUILT before uh_build_acceleration (or after moved instances without view->rebuild_tlas). */
int uh_render_frame(uh_ctx* ctx, const UhViewUniformData* view, uint32_t pass_mask);
/* `count` consecutive frames of the reference_pt pass with an unchanged camera: frame i is rendered
 * with total_samples = view->total_samples + i * samples_per_frame, exactly what `count` calls of
 * uh_render_frame under the application's frame protocol (prototype/src/main.rs:467-469) produce,
 * bit for bit; internally up to option "batch_frames" frames share one wavefront (path id =
 * frame * W*H + pixel) so that a rank owning few pixels still launches full-size kernels.
 * Only UH_PASS_REFERENCE_PT without reservoir light sampling can be batched (each ReSTIR frame
 * depends on the previous one); otherwise UH_ERR_INVALID_ARGUMENT. */
int uh_render_frames(uh_ctx* ctx, const UhViewUniformData* view, uint32_t pass_mask, uint32_t count);
int uh_reset_accumulation(uh_ctx* ctx);
int uh_synchronize(uh_ctx* ctx);

/* ---- read-back (host pointers; each call synchronises the context's stream) ------------ */
int uh_read_accumulation(uh_ctx* ctx, float* rgba32f /* W*H*4 */);
int uh_read_output_bgra8(uh_ctx* ctx, uint8_t* bgra /* W*H*4 */);
int uh_read_reservoirs(uh_ctx* ctx, int which /* 0 initial, 1 temporal, 2 spatial */, UhReservoir* out /* W*H */);
int uh_read_gbuffer_position(uh_ctx* ctx, float* rgba32f /* W*H*4, un-filtered texels */);
/* upload a reservoir buffer (tests seed the temporal history with it) */
int uh_write_reservoirs(uh_ctx* ctx, int which, const UhReservoir* in /* W*H */);
/* upload gbuffer_position (tests run the reservoir passes on given positions: frames without UH_PASS_GBUFFER read what is there) */
int uh_write_gbuffer_position(uh_ctx* ctx, const float* rgba32f /* W*H*4 */);

/* ---- stand-alone ray queries through the same traversal kernels (parity tests) ---------- */
/* rays: n * 8 floats (ox,oy,oz,tmin,dx,dy,dz,tmax); hits: n * 4 words (t,u,v as f32, then
 * (mesh_index << 22 | primitive) as u32, 0xffffffff on miss... see DESIGN.md "hit record") */
int uh_trace_closest(uh_ctx* ctx, const float* rays, uint32_t n, float* out_tuv /* n*3 */,
                     uint32_t* out_mesh /* n */, uint32_t* out_prim /* n */);
int uh_trace_any(uh_ctx* ctx, const float* rays, uint32_t n, uint8_t* out_occluded /* n */);

/* ---- stats / options ------------------------------------------------------------------- */
int uh_get_stats(uh_ctx* ctx, UhStats* out);
int uh_reset_stats(uh_ctx* ctx);
/* The 33 options (DESIGN.md section 7 has the defaults and what was measured); unknown names return UH_ERR_INVALID_ARGUMENT.
 *  diagnostics   "count_visits" (0/1: UhStats' node / triangle / cover counters), "time_kernels" (0/1: hipEvent time per kernel kind)
 *  results       "full_frame_restir" (0/1; 1 = documented divergence: the reservoir for every pixel instead of the reference's
 *                x > W/2 split), "furnace" (0/1: the reference's FURNACE_TEST build of the miss shader, reference.rmiss:14-28 - a path
 *                ray that leaves the scene returns white whatever view->sky_enabled says), "iso_reference_triangulation" (0/1,
 *                default 1: see uh_add_isosurface_mesh)
 *  textures      "texture_blocks" (0/1, default 1: uh_add_texture_rgba8 stores the textures added from now on as overlapped blocks of
 *                texels, one block per cache line, so that a bilinear footprint lies in one line - about 1.5 times the texels'
 *                memory; 0: as 8x8-texel tiles, or as rows when a side is no multiple of 8. Same images bit for bit. With 1 a texture
 *                whose blocks would hold more than 2^32 texels is refused with UH_ERR_CAPACITY)
 *  the tree      "device_build" (0/1/2; 1 or 2 = uh_build_acceleration builds the tree ON THE DEVICE in a few ms instead of the host
 *                SAH tree in tens to hundreds: same hits bit for bit, about 10 % (1: clusters under a SAH top) or 30 % (2: radix tree)
 *                more traversal work per ray - for geometry that changes every few frames), "ploc_sah_top" (clusters the PLOC rounds
 *                stop at; 0 = PLOC to the root)
 *  sun grid      "sun_grid" (0/1, default 1: sun shadow rays through a per-direction visibility grid once the direction has settled;
 *                same images), "sun_grid_build" (0/1, default 1: built on the device in a few milliseconds; 0: by the host builder,
 *                the reference implementation, in 130-550 ms), "sun_grid_density" (entries per triangle the cell size aims at),
 *                "sun_grid_max_mb" (budget of the entry lists), "sun_grid_max_walk" (longest list a ray tests itself),
 *                "sun_grid_force" (0/1: 1 = never refused for its worth - long lists, much of the surface handed to the tree), "sun_grid_inline_max_mb" (the lists a
 *                second time as 64-byte records that carry their triangle packet - one round trip per triangle test instead of two:
 *                budget in MB, -1 = default = four times the packet array, 0 = never), "sun_grid_coarse" (0..6, default 2: a cover
 *                depth per block of 4 x 4 cells, small enough to stay in the L2, asked before the cell's own record; 0: none),
 *                "sun_verdicts" (0/1, default 1: with the grid in use and lights disabled the sun-ray kernels leave one verdict bit per
 *                ray, and the kernels that read the path's radiance next add its throughput there - no read-modify-write of the
 *                radiance in the sun kernels; 0: they add it themselves; same images),
 *                "slim_state" (0/1, default 1: a pass with sun verdicts and one sample per frame carries 56 bytes of state per path
 *                instead of 64 - the path id rides with the origin, so no id queue is written or read behind bounce 0 - and the sun
 *                kernels of its last bounce store the surviving paths' radiance themselves, no flush launch; every other pass keeps
 *                the four-quad state; same images)
 *  camera grid   "camera_grid" (0/1, default 1: the primary rays of a camera that has been the same for two consecutive frame calls -
 *                or for a call of 8 or more frames - go through a per-camera grid of packet lists, one cell per pixel, instead of
 *                the tree; same hit records bit for bit), "camera_grid_max_walk", "camera_grid_walk_whole",
 *                "camera_grid_max_mean_list_x10", "primary_implicit" (0/1, default 1: with that grid in use and one sample per frame,
 *                the primary rays' state is not stored - the kernels of the first bounce compute it from the path id; same images),
 *                "fused_primary" (0/1, default 1: in a pass with that grid, "primary_implicit" and the slim state in effect, none of
 *                whose pixels hands its ray to the tree, and "count_visits" off, the first bounce is ONE kernel that stands at the
 *                pixel - primary ray, list walk and hit shading - instead of three that pass ids and hit records through memory;
 *                0: always the three kernels; same images)
 *  scheduling    "frames_in_flight" (1..8, default 4), "batch_frames" (0 = auto), "overlap" (0/1, default 1: the miss shader and the
 *                shadow traversals on a second stream beside the next bounce's traversal), "trace_blocks_per_cu" (1..8: persistent
 *                grid of the traversal kernels), "fused_bounces" (default 1: a frame that goes alone - uh_render_frame, or a call
 *                of one frame - and finds the GPU idle, i.e. a caller that waits for its frames, runs its bounces 1 .. inside one
 *                persistent kernel, a wavefront per block, instead of four launches per bounce: same images, 2.5 ms against 2.85
 *                for a 1080p frame, 0.99 against 1.57 at 960 x 540; with frames in flight the launches interleave better and are
 *                kept, and so they are for frames of more than 4 M paths, whose launches are large already. 0: never; -1: always;
 *                2..8: as 1, and the kernel's blocks per CU)
 * Removed in round 5 with the measured-negative variants they selected: "closest_variant" / "shadow_variant" / "trace_variant" (batch
 * traversal kernels), "primary_tiles", "interleave", "sun_grid_fused", "sun_leftover_batch", "sun_grid_async", "sun_grid_inline",
 * "spatial_splits", "bvh_optimise", "raw_visit_counts", "ploc_radius", "overlap_miss" / "overlap_shadow" (now "overlap"),
 * "sun_grid_max_mean_list_x10" / "sun_grid_max_fallback_pct" (now "sun_grid_force"),
 * "closest_blocks_per_cu" / "shadow_blocks_per_cu" (now "trace_blocks_per_cu"), "single_frame_blocks_per_cu", "miss_blocks_per_cu". */
int uh_set_option(uh_ctx* ctx, const char* name, int value);

/* diagnostics: the sun-direction grid in use (built on the device, option "sun_grid_build" = 1) read back and held against the host
 * builder - the reference implementation whose margins tests/cpp/sun_grid_check.cpp checks against brute force - run on the same
 * packets and the same raster. out[0] cells, out[1] / out[2] entries of the device / host grid, out[3] cells whose list length
 * differs, out[4] cells whose list differs (element by element where a ray may walk it - interior cells of at most
 * "sun_grid_max_walk" entries -, as a set elsewhere), out[5] cells whose cover depth differs in any bit, out[6] walkable cells
 * compared, out[7] the host builder's time in microseconds. UH_ERR_INVALID_ARGUMENT when no grid is in use. */
int uh_sun_grid_compare_builders(uh_ctx* ctx, uint64_t out[8]);

/* diagnostics: the tree in use - whichever builder or refit wrote it - read back (nodes, packets, world corners, shade packets) and
 * held on the host, in double, to the invariants the traversal relies on (csrc/bvh_invariants.h; the host builder's trees are their
 * reference, tests/cpp/bvh_check.cpp). Waits for the frames in flight. out[0] nodes, out[1] triangles, out[2] levels, then one
 * violation count per class: out[3] levels (level_start well formed, at most as many as the traversal stack holds, every child in a
 * later level than its parent), out[4] counts (n_tri <= n_child <= 4, child_base's copy of n_tri, step exponents), out[5] refs (every
 * node but the root and every packet referenced exactly once), out[6] keys (the packets' keys are the scene's, each once; the shade
 * packet's mesh), out[7] packets (the packet is the bake of its world corners bit for bit), out[8] empty slots (inverted boxes),
 * out[9] containment (a slot's planes contain the padded box of its subtree; not checked when out[11] = 0: non-finite corners);
 * out[10] the bits of a double: the sum of the slots' box areas over the root's (reported, not judged). Violations are the result,
 * not an error: UH_OK, and uh_last_error names the first offender of each class (empty when there is none).
 * UH_ERR_INVALID_ARGUMENT when no tree has been built for the scene as it is. There is no raw read-back of the tree. */
int uh_check_acceleration(uh_ctx* ctx, uint64_t out[16]);

/* ---- multi-GPU framebuffer tile partition (one process per GPU) ------------------------ */
/* After this call uh_render_frame path-traces only pixels of tiles t with t % world == rank
 * (tile_size x tile_size tiles, row-major tile ids). ReSTIR passes stay full-frame unless uh_set_restir_partition says otherwise. */
int uh_set_tile_partition(uh_ctx* ctx, uint32_t rank, uint32_t world, uint32_t tile_size);
/* number of float4 pixels uh_pack_tiles writes for `rank` (padded: whole tiles) */
int uh_tile_pack_count(uh_ctx* ctx, uint32_t rank, uint64_t* out_pixels);
/* pack this rank's owned tiles of the RGBA32F accumulation into a contiguous DEVICE buffer */
int uh_pack_tiles(uh_ctx* ctx, void* device_out, uint64_t capacity_pixels);
/* scatter `from_rank`'s packed tiles (DEVICE buffer) into this context's accumulation image */
int uh_unpack_tiles(uh_ctx* ctx, uint32_t from_rank, const void* device_in, uint64_t num_pixels);
/* the root's whole composition in one launch: `device_all` holds `world` packed buffers (rank r's at r * stride_pixels
 * float4 pixels, as uh_pack_tiles wrote them; the root's own slot is not read); scatters every other rank's tiles into the
 * accumulation image and recomputes pt_output_image (= uh_unpack_tiles for every rank + uh_resolve_output) */
int uh_compose_tiles(uh_ctx* ctx, const void* device_all, uint64_t stride_pixels, uint32_t total_samples, uint32_t accumulation_limit);
/* recompute pt_output_image from the accumulation image (after uh_unpack_tiles on the root) */
int uh_resolve_output(uh_ctx* ctx, uint32_t total_samples, uint32_t accumulation_limit);
/* ---- multi-GPU, the reservoir passes: a band of rows per rank + one exchange per frame ------ */
/* The path tracer needs spatial_reuse_reservoirs only at its own pixels, but temporal_reuse reads last frame's buffer at a
 * reprojected pixel (restir/temporal_reuse.rgen:90-99) and spatial_reuse gathers from a 30-pixel neighbourhood
 * (restir/spatial_reuse.rgen:40-60), so run full-frame on every rank these passes do not scale (alternative).
 * After uh_set_restir_partition(rank, world) the G-buffer cast and the reservoir passes of this context cover
 *   spatial_reuse      rows [rank * B, min(H, (rank + 1) * B)),  B = ceil(H / world)        (the band)
 *   reset / initial / temporal   the band +- 30 rows, plus row H - 1 for the first band (spatial_reuse.rgen:54: a row
 *                      offset below zero wraps and is clamped to the last row)
 *   G-buffer cast      those rows and the row above each (the 2 x 2 corner filter of initial_ris.rgen:22-23)
 * and every spatial pass is followed by ONE call of `exchange`, which must enqueue on `hip_stream` whatever makes
 * spatial_base[k * band_bytes, (k + 1) * band_bytes) hold rank k's band for every k (an in-place all-gather: this rank's band
 * is already where it belongs). It is called while the frame is ENQUEUED, not when it runs: it must not wait for the GPU.
 * Each spatial_reuse buffer is world * B rows long (the frame, padded to equal bands). With the exchange in place every
 * rank holds the whole spatial_reuse_reservoirs of every frame - bit for bit the single-GPU buffer - while buffers 0 and 1
 * (uh_read_reservoirs) are valid on the rank's own rows only. world = 1 (the default) restores full-frame passes (an
 * exchange given with world = 1 is still called: a one-rank all-gather, for rehearsals). exchange == NULL with world > 1
 * leaves the other bands stale: for timing one rank's share only. The call waits for the frames in flight and keeps the
 * temporal history. */
typedef int (*UhRestirExchangeFn)(void* user, void* hip_stream, void* spatial_base, uint64_t band_bytes, uint32_t rank, uint32_t world);
int uh_set_restir_partition(uh_ctx* ctx, uint32_t rank, uint32_t world, UhRestirExchangeFn exchange, void* user);
/* the rows of this context's band and of its reservoir / G-buffer passes (counts of rows; *_extra_row0 is the first row of the second interval or 0 with *_extra_rows 0) */
typedef struct UhRestirRows {
   uint32_t band_row0, band_rows;        /* spatial_reuse */
   uint32_t reuse_row0, reuse_rows, reuse_extra_row0, reuse_extra_rows;   /* reset, initial_ris, temporal_reuse */
   uint32_t cast_row0, cast_rows, cast_extra_row0, cast_extra_rows;       /* G-buffer cast */
   uint32_t rows_per_band;               /* B */
} UhRestirRows;
int uh_get_restir_rows(uh_ctx* ctx, UhRestirRows* out);
/* RCCL, built in (one process per GPU): librccl is opened at run time (the library does not link it). Rank 0 makes an id, the
 * job's launcher hands the 128 bytes to every rank (rust-renderer_amd/launch.py: a TCP socket on 127.0.0.1 - no torch in a GPU
 * process), every rank attaches: ncclCommInitRank + uh_set_restir_partition(rank, world, <ncclAllGather on the reservoir stream>);
 * a job that wants full-frame reservoir passes calls uh_set_restir_partition(ctx, 0, 1, NULL, NULL) afterwards (the communicator
 * stays for uh_rccl_gather_tiles). */
int uh_rccl_unique_id(uint8_t out_id[128]);
int uh_rccl_attach(uh_ctx* ctx, uint32_t rank, uint32_t world, const uint8_t id[128]);
int uh_rccl_detach(uh_ctx* ctx);
/* ranks of the communicator uh_rccl_attach made, as RCCL itself counts them (ncclCommCount); 0 when none is attached */
int uh_rccl_comm_count(uh_ctx* ctx, uint32_t* out_ranks);
/* The composition of a tile-partitioned frame over that communicator (ONE gather per composed image): every rank packs
 * its tiles of pt_accumulation_image (uh_pack_tiles' layout) and sends them to `root` - grouped ncclSend / ncclRecv, the peers' tiles
 * arrive on distinct xGMI links at once -, the root scatters them into its accumulation image and recomputes pt_output_image with
 * (total_samples, accumulation_limit) in one launch (the two images of renderers/mod.rs:199-214,354-358, which the reference's
 * single device holds whole). Collective: every rank of the communicator calls it, with the same root, after
 * uh_set_tile_partition(rank, world, tile) with the communicator's rank and size. ENQUEUED on the context's stream behind the frames
 * in flight - no host wait, no staging through the host; the root's uh_read_* (or uh_synchronize) waits for it, and frames enqueued
 * after it accumulate behind it. */
int uh_rccl_gather_tiles(uh_ctx* ctx, uint32_t root, uint32_t total_samples, uint32_t accumulation_limit);
/* raw device pointers (zero-copy wrap by the caller, e.g. for RCCL): 0 accumulation RGBA32F,
 * 1 output BGRA8 */
int uh_device_pointer(uh_ctx* ctx, int which, void** out);
/* the HIP stream all work of this context is enqueued on (hipStream_t as void*); also makes the context's device
 * the calling thread's current device */
int uh_stream(uh_ctx* ctx, void** out);

/* ---- GPU extraction of the reference's marching-cubes density field (BASELINE configs[4]) --------
 * Adds the iso-surface {density = 0} of utopian/shaders/marching_cubes/marching_cubes.comp:83-103 (torus over a box,
 * plus the sphere of radius 8 |sin(0.3 time)|; shapes placed in a 32-unit domain) sampled on a resolution^3 grid over
 * [lo, hi]^3 as one mesh with uh_add_mesh semantics. Extraction runs on the device: marching cubes on the reference's case table,
 * cell by cell the triangles marching_cubes.comp:231-251 emits - same vertices (vertexInterp in the shader's corner order), same
 * order within a cell, zero-area triangles included; cells in x-fastest order (the reference's order is whatever its atomics
 * give). Option "iso_reference_triangulation" = 0 selects this repository's own tables (other interior diagonals, slivers
 * dropped). Vertex normals come from the density gradient (generateNormal), uv = position.xz / (hi - lo). *out_triangles receives the triangle count; when nothing
 * crosses the iso value no mesh is added and *out_mesh_index is 0xffffffff. UH_ERR_CAPACITY above 4 Mi triangles. */
int uh_add_isosurface_mesh(uh_ctx* ctx, uint32_t resolution, float lo, float hi, float time, const UhGpuMaterial* material,
                           const float world3x4[12], uint32_t* out_mesh_index, uint32_t* out_triangles);
/* diagnostics of the extraction: per cell (x fastest, resolution^3 of them) the marching-cubes case index (bit i set when corner i
 * is outside, marching_cubes.comp:185-190) and the number of triangles the cell contributes (zero-area ones dropped); either
 * pointer may be NULL. The oracle's restatement of the shader is compared with these cell by cell. */
int uh_isosurface_cells(uh_ctx* ctx, uint32_t resolution, float lo, float hi, float time, uint8_t* out_cube_index, uint8_t* out_triangle_count);
/* the context's host copy of a mesh (Model keeps CPU copies, primitive.rs:19-24): sizes, then the data */
int uh_mesh_info(uh_ctx* ctx, uint32_t mesh_index, uint32_t* num_vertices, uint32_t* num_indices);
int uh_read_mesh(uh_ctx* ctx, uint32_t mesh_index, UhVertex* vertices, uint32_t* indices);

/* ---- the density field at another time, without leaving the GPU -------------------------------------------------------
 * Re-extracts the field at `time` with the resolution, lo, hi and triangulation mesh `mesh_index` was created with by
 * uh_add_isosurface_mesh in this context, and makes the result that mesh's geometry. Material, transform and the mesh's index stay;
 * the triangle count may grow, shrink or become zero (the mesh keeps its index with no vertices and comes back with a later update).
 * *out_triangles (may be NULL) receives the new count.
 * Equivalence: after the update and a uh_build_acceleration every observable of the context - traces, the hybrid and forward
 * graphs' images, the shadow maps, uh_read_mesh, and frames rendered from cleared temporal state - equals, bit for bit, that of a
 * fresh context whose same scene was made with uh_add_isosurface_mesh(..., time, ...) in the first place. Temporal state is the
 * accumulation (uh_reset_accumulation) and the reservoirs' history, which an update does not touch and uh_reset_accumulation does not
 * clear (uh_write_reservoirs does): a frame's temporal pass reads what the frames before the update left, as it does after any
 * other change of the scene.
 * State: that of uh_add_mesh - the context is not built. Every render and trace verb and uh_refit_acceleration return
 * UH_ERR_NOT_BUILT until uh_build_acceleration has run (the topology changed: view->rebuild_tlas does not rebuild by itself).
 * Errors: UH_ERR_INVALID_ARGUMENT for a null context, an index out of range, a mesh that uh_add_isosurface_mesh did not create, or a
 * non-finite time; UH_ERR_CAPACITY above 4 Mi triangles; UH_ERR_OUT_OF_MEMORY when the vertex buffer cannot grow: all of these leave
 * everything as it was (a built context stays built and renders as before). UH_ERR_HIP from the emit pass itself, behind that
 * point, leaves the mesh with its new size and undefined vertices and the context not built: update again.
 * Stream order: waits for the frames in flight and is complete on return.
 * Memory: the mesh's vertices then live on the device, 240 bytes per triangle (the buffer grows when needed and is reused
 * otherwise), and the host copy is dropped. Every consumer is fed from there: with option "device_build" 1 or 2 the build's
 * per-triangle sources (104 bytes per triangle of the scene, as before; while a changed count is being applied a second set exists)
 * are written by a kernel and the other meshes' ranges are moved on the device; the hybrid / forward graphs' mesh tables are
 * refreshed by device copies. With "device_build" 0 the host builder needs the host copy: the mesh is read back once per update
 * (80 bytes per vertex) and its packets uploaded as before (112 bytes per triangle) - the slow route, same results.
 * uh_mesh_info answers from the recorded counts; uh_read_mesh of such a mesh copies from the device (a blocking copy the call does
 * not make for other meshes). */
int uh_update_isosurface_mesh(uh_ctx* ctx, uint32_t mesh_index, float time, uint32_t* out_triangles);
typedef struct UhIsosurfaceUpdateStats {
   float extract_ms;             /* hipEvent: count + scan + emit of the last update */
   float scatter_ms;             /* hipEvent: the refreshes from device vertices since the last update: the build sources of the last
                                    uh_build_acceleration plus the raster tables of the hybrid / forward call after it */
   uint32_t updates;             /* so far */
   uint32_t triangles;           /* of the last update */
   uint64_t host_geometry_bytes; /* cumulative: vertex, index, corner and shade-packet bytes of updated isosurface meshes that this
                                    context moved between host and device, either way, in any verb (uh_read_mesh's index list, which
                                    is written on the host, counts as handed over: 4 bytes per index) */
   uint64_t device_bytes;        /* device memory held for device-resident meshes: their vertex buffers and the extraction's scratch */
} UhIsosurfaceUpdateStats;
UH_LAYOUT_ASSERT(sizeof(UhIsosurfaceUpdateStats) == 32 && offsetof(UhIsosurfaceUpdateStats, updates) == 8 && offsetof(UhIsosurfaceUpdateStats, triangles) == 12 &&
                    offsetof(UhIsosurfaceUpdateStats, host_geometry_bytes) == 16 && offsetof(UhIsosurfaceUpdateStats, device_bytes) == 24,
                 "UhIsosurfaceUpdateStats (32 B)");
/* all zero before the first update; waits for the frames in flight like the other stats calls */
int uh_get_isosurface_update_stats(uh_ctx* ctx, UhIsosurfaceUpdateStats* out);

/* ---- deforming meshes: new vertices for a mesh of uh_add_mesh, refitted on the device ----------------------------------
 * Replaces ALL vertices of mesh `mesh_index` - positions, normals, uvs and the rest of the 80-byte record - with the `num_vertices`
 * records at `vertices`; num_vertices must equal the mesh's count. The index list, material, transform and mesh index stay. `where`
 * says what `vertices` is: UH_VERTICES_HOST a host pointer, UH_VERTICES_DEVICE a device pointer on the context's device, whose buffer
 * the caller has finished writing; the library copies it into the mesh's own buffer and the caller may reuse it after return.
 * State: that of uh_set_instance_transform, not that of uh_add_mesh - the context is not built, the topology is as valid as it was.
 * uh_refit_acceleration is accepted, and uh_render_frame / uh_render_hybrid / uh_render_forward refit by themselves when
 * view->rebuild_tlas == 1 (UH_ERR_NOT_BUILT without it); the per-frame protocol is update, rebuild_tlas = 1, render. The refit writes
 * the moved meshes' triangle packets again in the tree's leaf order (k_deform_gather) and then recomputes every box; instances moved
 * in the same interval are served by the same refit. uh_build_acceleration is the other way out, for a surface that has drifted far
 * from where the tree was built (the refitted tree answers the same, at more node visits). If meshes were added since the last
 * build only a build will do, as ever.
 * Equivalence: after the update and either a refit or a build every observable of the context - uh_read_mesh, uh_trace_closest /
 * uh_trace_any, frames path traced from cleared temporal state (see uh_update_isosurface_mesh) with both grids, the cast and the
 * rasterised G-buffer, the shadow maps, the forward graph - equals, bit for bit, that of a fresh context whose same scene was made
 * with uh_add_mesh from the new vertices and then built. Node-visit counters are not observables.
 * Errors: UH_ERR_INVALID_ARGUMENT for a null context, a null pointer with num_vertices > 0, an index out of range, a count that
 * differs from the mesh's, a `where` other than the two values, a mesh created by uh_add_isosurface_mesh (it has its own verb) or a
 * non-finite position - host input is checked on the host as uh_add_mesh checks it, device input by a pass over the caller's buffer
 * before anything of the mesh is overwritten; UH_ERR_OUT_OF_MEMORY when the mesh's device buffers cannot be made. All of these leave
 * everything as it was (a built context stays built and renders as before). A mesh with zero vertices accepts num_vertices == 0,
 * which changes nothing but the stats.
 * Stream order: waits for the frames in flight and is complete on return.
 * Memory: an updated mesh keeps its vertices in a device buffer of its own (80 bytes per vertex) behind its index list, which goes to
 * the device once, with the first update. Host input also overwrites the host copy; after device input the host copy is stale, and
 * the host builder ("device_build" 0) and uh_read_mesh fetch it with a blocking copy (the index list never: the host still has it).
 * With "device_build" 1 or 2 a UH_VERTICES_DEVICE update followed by a refit or a build moves no geometry between host and device. */
#define UH_VERTICES_HOST   0
#define UH_VERTICES_DEVICE 1
int uh_update_mesh_vertices(uh_ctx* ctx, uint32_t mesh_index, const UhVertex* vertices, uint32_t num_vertices, int where);
typedef struct UhMeshUpdateStats {
   float gather_ms;              /* hipEvent: k_deform_gather of the last refit that had moved vertices to gather */
   float refit_ms;               /* hipEvent: the passes of that refit behind it (the bake and the boxes) */
   uint32_t updates;             /* so far */
   uint32_t triangles;           /* rewritten by that refit: the triangles of the meshes whose vertices had moved */
   uint64_t host_geometry_bytes; /* cumulative: vertex, corner and packet bytes of updated meshes that this context moved between host
                                    and device, either way, in any verb. The index list's one upload, 4 bytes per index with a mesh's
                                    first update, is not in it: it is the same list the host keeps */
   uint64_t device_bytes;        /* the vertex and index buffers held for updated meshes */
} UhMeshUpdateStats;
UH_LAYOUT_ASSERT(sizeof(UhMeshUpdateStats) == 32 && offsetof(UhMeshUpdateStats, updates) == 8 && offsetof(UhMeshUpdateStats, triangles) == 12 &&
                    offsetof(UhMeshUpdateStats, host_geometry_bytes) == 16 && offsetof(UhMeshUpdateStats, device_bytes) == 24,
                 "UhMeshUpdateStats (32 B)");
/* all zero before the first update; waits for the frames in flight like the other stats calls */
int uh_get_mesh_update_stats(uh_ctx* ctx, UhMeshUpdateStats* out);

/* ---- posed meshes: a skin and / or morph targets on a mesh of uh_add_mesh, posed on the device ------------------------------
 * An EXTENSION: the reference draws its glTF assets in their bind pose. uh_set_mesh_skin gives mesh `mesh_index` four joint indices
 * and four weights per vertex (linear blend skinning over `num_joints` joints), uh_set_mesh_morph_targets gives it `num_targets`
 * morph targets: position deltas, 3 floats per vertex, target-major (target t's deltas are position_deltas[3 * (t * num_vertices + i)
 * ..]), and optionally normal deltas of the same shape. A mesh may have either or both. Each set verb takes the mesh's CURRENT
 * vertices as the bind pose (from the device when the host copy is stale after a device update or a pose), keeps its input in device
 * buffers of the mesh, and replaces what an earlier call of the same verb set; the bind pose is taken anew by every call of either.
 * Neither changes the geometry: a built context stays built and renders as before.
 * uh_pose_mesh then writes ALL vertices of the mesh from the bind pose: one kernel (k_pose, pose.hip), its only host input the call's
 * joint matrices - row-major 3x4, 12 floats each, the layout of uh_set_instance_transform, object space to object space - and morph
 * weights. num_joints / num_targets must equal what was set, or be 0 with a null pointer for a part the mesh does not have. The
 * arithmetic is DESIGN.md section 2, "Posed meshes": targets with a weight of exactly zero are skipped, the others added in ascending
 * order; the blend of the four joint matrices transforms the position, and its upper 3x3 - not the inverse transpose: exact in
 * direction for rigid and uniformly scaled joints, as in common glTF viewers - the normal and the tangent; the normal is normalised
 * unless it is zero, the tangent too when a skin transformed it; every other field is the bind record's, bit for bit.
 * State after a pose: that of uh_update_mesh_vertices(UH_VERTICES_DEVICE) - the context is not built, the host copy is stale,
 * UhMeshUpdateStats::updates counts it, motion vectors classify the mesh `deformed`; the per-frame protocol is pose,
 * view->rebuild_tlas = 1, render. A later uh_update_mesh_vertices on the mesh is allowed; the bind pose stays what it was when set.
 * No vertex data moves between host and device in a pose.
 * Errors, each UH_ERR_INVALID_ARGUMENT and each leaving everything as it was: a null context, an index out of range, a mesh of
 * uh_add_isosurface_mesh or one without vertices, num_vertices differing from the mesh's count, num_joints == 0 (or more than 65,536)
 * or num_targets == 0 in a set verb, a null pointer (normal_deltas may be null), a joint index >= num_joints, a weight that is
 * negative or not finite, a vertex whose four weights are all zero, a delta that is not finite; in uh_pose_mesh a mesh with neither
 * part, counts that differ from what was set, a matrix entry or morph weight that is not finite - all checked on the host before
 * anything is stored -, and a posed position that is not finite: the kernel raises a flag, and the call is refused with the mesh,
 * the tree and the build state exactly as before (the pose is written into a second vertex buffer that changes places with the
 * mesh's own only on success). UH_ERR_OUT_OF_MEMORY when a buffer cannot be made.
 * STREAM ORDER: the four verbs wait for the frames in flight and are complete on return.
 * RESOURCES: per posed mesh 80 bytes per vertex of bind pose, 24 per vertex of skin, 12 (24 with normals) per vertex and target,
 * allocated by the set verbs; with the first pose the second vertex buffer (80 per vertex) and the buffers of an updated mesh; per
 * context the call's parameters (48 bytes per joint, 8 per active target) and two events. All freed by uh_destroy. A context that never
 * calls these verbs allocates nothing and launches no new kernel.
 * ISOLATION: no other verb's result changes; uh_update_mesh_vertices runs the code it ran (its tail is now a helper pose shares).
 * No uh_mgpu_ twin. */
int uh_set_mesh_skin(uh_ctx* ctx, uint32_t mesh_index, const uint16_t* joints, const float* weights, uint32_t num_vertices, uint32_t num_joints);
int uh_set_mesh_morph_targets(uh_ctx* ctx, uint32_t mesh_index, const float* position_deltas, const float* normal_deltas, uint32_t num_vertices,
                              uint32_t num_targets);
int uh_pose_mesh(uh_ctx* ctx, uint32_t mesh_index, const float* joint_matrices3x4, uint32_t num_joints, const float* morph_weights,
                 uint32_t num_targets);
typedef struct UhPoseStats {
   float pose_ms;               /* hipEvent: k_pose of the last pose */
   uint32_t poses;              /* so far (refused ones are not counted) */
   uint32_t vertices;           /* of the last pose */
   uint32_t joints;             /* of the last pose */
   uint32_t active_targets;     /* of the last pose: the targets whose weight was not zero */
   uint32_t staged_joint_limit; /* the largest joint count k_pose keeps in LDS; 0: it never stages - the case: staging measured no
                                   faster at 64 joints and slower at 1,024 (DESIGN.md section 4 "Posed meshes") */
   uint64_t device_bytes;       /* bind poses, skins, deltas, second vertex buffers and the call parameters held for posed meshes */
} UhPoseStats;
UH_LAYOUT_ASSERT(sizeof(UhPoseStats) == 32 && offsetof(UhPoseStats, poses) == 4 && offsetof(UhPoseStats, vertices) == 8 &&
                    offsetof(UhPoseStats, joints) == 12 && offsetof(UhPoseStats, active_targets) == 16 &&
                    offsetof(UhPoseStats, staged_joint_limit) == 20 && offsetof(UhPoseStats, device_bytes) == 24,
                 "UhPoseStats (32 B)");
/* all zero before the first pose; waits for the frames in flight like the other stats calls */
int uh_get_pose_stats(uh_ctx* ctx, UhPoseStats* out);

/* ---- several GPUs behind ONE application process (SURVEY.md section 8b "multi-GPU", 8e) ------------
 * The reference application is a single process with one render thread (prototype/src/main.rs:86-570);
 * a maintainer who wants N GPUs behind it binds this group instead of one uh_ctx. Every verb above has a
 * uh_mgpu_ twin with the same meaning: scene verbs replicate the scene on every GPU, frame verbs make GPU i
 * path-trace the tiles t % N == i (tile_size x tile_size, row-major ids; ReSTIR / G-buffer passes run
 * full-frame on every GPU, identical results), nothing is exchanged per frame, and the read-backs (or
 * uh_mgpu_compose) gather the packed RGBA32F tiles onto GPU 0 with peer copies over xGMI and recompute
 * pt_output_image there. Pixels are bit-identical to a single-GPU render (RNG keyed on absolute pixel
 * coordinates, random.glsl:14-18). device_ordinals == NULL means GPUs 0..ngpus-1; the same ordinal may
 * appear several times (how the 1-GPU tests exercise this layer). */
typedef struct uh_mgpu uh_mgpu;
int uh_mgpu_create(int ngpus, const int* device_ordinals, uint32_t width, uint32_t height, uint32_t tile_size, uh_mgpu** out);
void uh_mgpu_destroy(uh_mgpu* group);
const char* uh_mgpu_last_error(uh_mgpu* group); /* NULL: the last creation error */
int uh_mgpu_num_devices(uh_mgpu* group);
uh_ctx* uh_mgpu_context(uh_mgpu* group, int index); /* GPU i's context (options, stats, queries); owned by the group */
int uh_mgpu_add_texture_rgba8(uh_mgpu* group, const uint8_t* pixels, uint32_t w, uint32_t h, uint32_t* out_index);
int uh_mgpu_add_mesh(uh_mgpu* group, const UhVertex* vertices, uint32_t num_vertices, const uint32_t* indices, uint32_t num_indices,
                     const UhGpuMaterial* material, const float world3x4[12], uint32_t* out_mesh_index);
int uh_mgpu_add_light(uh_mgpu* group, const UhGpuLight* light, uint32_t* out_index);
int uh_mgpu_get_num_lights(uh_mgpu* group, uint32_t* out);
int uh_mgpu_set_instance_transform(uh_mgpu* group, uint32_t mesh_index, const float world3x4[12]);
int uh_mgpu_build_acceleration(uh_mgpu* group);  /* the N host builds run concurrently */
int uh_mgpu_refit_acceleration(uh_mgpu* group);
int uh_mgpu_render_frame(uh_mgpu* group, const UhViewUniformData* view, uint32_t pass_mask);   /* enqueues on every GPU, does not wait */
int uh_mgpu_render_frames(uh_mgpu* group, const UhViewUniformData* view, uint32_t pass_mask, uint32_t count);
int uh_mgpu_reset_accumulation(uh_mgpu* group);
int uh_mgpu_synchronize(uh_mgpu* group);
int uh_mgpu_compose(uh_mgpu* group);             /* gather tiles to GPU 0 + resolve; a no-op until the next frame */
int uh_mgpu_read_accumulation(uh_mgpu* group, float* rgba32f /* W*H*4 */);  /* compose, then read GPU 0 */
int uh_mgpu_read_output_bgra8(uh_mgpu* group, uint8_t* bgra /* W*H*4 */);
/* reservoir buffers of the whole frame (0 initial, 1 temporal: each GPU's band of rows; 2 spatial: complete on every GPU) */
int uh_mgpu_read_reservoirs(uh_mgpu* group, int which, UhReservoir* out /* W*H */);
int uh_mgpu_get_stats(uh_mgpu* group, UhStats* out); /* counters summed over GPUs, times = slowest GPU */
int uh_mgpu_reset_stats(uh_mgpu* group);
/* every context's options, plus "restir_partition" (default 1 for more than one GPU): the G-buffer cast and the reservoir
 * passes by bands of rows, one band per GPU (uh_set_restir_partition), the bands exchanged by peer copies after every
 * spatial pass; 0 = every GPU runs them for the whole frame */
int uh_mgpu_set_option(uh_mgpu* group, const char* name, int value);

/* ---- the hybrid graph's ray-traced passes (build_render_graph, utopian/src/renderers/mod.rs:61-186) -------------------------
 * Per-context verbs: they have no uh_mgpu_ twin. The rasterized graph of the reference (key 2 of the prototype) traces rays in
 * two passes over a G-buffer of four targets (create_gbuffer_textures, mod.rs:17-45):
 *   UH_HYBRID_GBUFFER         gbuffer_pass (gbuffer.vert / gbuffer.frag) as a cast of the un-jittered primary rays - the same rays and
 *                             the same traversal as UH_PASS_GBUFFER, so the position target equals gbuffer_position bit for bit - and
 *                             a resolve of position RGBA32F, normal RGBA32F (normal-mapped where the tangent is not zero), albedo RGBA8
 *                             (the diffuse map without base_color_factor, alpha 255) and pbr RGBA32F (metallic = the metallic-roughness
 *                             map's b, roughness = its g, occlusion = the occlusion map's r, the material index: mesh i has material i)
 *   UH_HYBRID_RT_SHADOWS      rt_shadows (rt_shadows.rgen): one any-hit ray per pixel toward normalize(view.sun_dir) from the G-buffer's
 *                             texel corner; R8: 0 occluded, 255 not (sun_shadow_enabled / shadows_enabled are not read, as there)
 *   UH_HYBRID_RT_REFLECTIONS  rt_reflections (rt_reflections.rgen/.rchit/.rmiss, IBL off): one closest-hit ray per pixel whose material
 *                             is metal (raytrace_properties.x == 1), RGBA8 = 0.1 * diffuse texel * base colour on a hit, the sky
 *                             (white under option "furnace") on a miss, alpha 0; every other pixel (0, 0, 0, 0)
 * PASS ORDER is the reference's (rt_shadows is added to the graph before gbuffer_pass, mod.rs:100-119, and the graph runs passes in the
 * order they were added, graph.rs:743): with UH_HYBRID_ALL, rt_shadows reads the G-buffer of the PREVIOUS hybrid call, then the G-buffer
 * pass runs, then rt_reflections on the new G-buffer. A caller that wants this frame's shadows calls with UH_HYBRID_GBUFFER, then with
 * UH_HYBRID_RT_SHADOWS.
 * RESOURCES of its own, separate from the path-tracing graph's gbuffer_position (each graph of the reference creates its own): allocated by
 * the first uh_render_hybrid (61 bytes per pixel with the reflection queue; UH_ERR_OUT_OF_MEMORY when that fails), cleared to
 * (1, 1, 1, 0) - albedo (255, 255, 255, 0), rt_shadows 255, rt_reflections (255, 255, 255, 0) - and freed by uh_destroy. A context
 * that never calls uh_render_hybrid allocates nothing for it.
 * ISOLATION: a hybrid call changes nothing a path-traced frame reads or reports (accumulation, gbuffer_position, reservoirs, UhStats,
 * the camera / sun grids' state); its rays and times go to UhHybridStats only. The passes are always full-frame:
 * uh_set_tile_partition and uh_set_restir_partition do not apply to them.
 * GATES: view->raytracing_supported == 0 skips both ray-traced passes and leaves their images as they are (mod.rs:107,134);
 * UH_HYBRID_RT_REFLECTIONS with view->ibl_enabled == 1 is UH_ERR_INVALID_ARGUMENT - and nothing runs - until the IBL maps (irradiance,
 * specular, BRDF LUT of ibl.rs) have been built with UH_HYBRID_ENVIRONMENT, below; mask bits, UH_ERR_NOT_BUILT and moved instances with
 * view->rebuild_tlas as for uh_render_frame (bits above UH_HYBRID_SHADOW_MAPS, below, are ignored, except UH_HYBRID_MARCHING_CUBES,
 * UH_HYBRID_GBUFFER_RASTER, UH_HYBRID_RESTIR_LIGHTS, UH_HYBRID_RTAO, UH_HYBRID_MOTION, UH_HYBRID_TAA, UH_HYBRID_POST, UH_HYBRID_RTGI, UH_HYBRID_GLOSSY, UH_HYBRID_FOG and UH_HYBRID_GLASS); UH_HYBRID_AREA_LIGHTS is not ignored either.
 * STREAM ORDER: uh_render_hybrid enqueues like a frame (behind the frames in flight, ahead of those that follow); uh_read_hybrid and
 * uh_get_hybrid_stats wait for all work of the context and are complete on return. The exception is UH_HYBRID_SHADOW_MAPS, below: a
 * call that renders shadow maps BLOCKS the host until the frames in flight and the pass's binning have finished (it reads the
 * binning's totals back to size its buffers); the passes after it are enqueued as usual. So does a G-buffer pass rasterised with
 * UH_HYBRID_GBUFFER_RASTER, below, for the same reason.
 * Arithmetic: DESIGN.md section 2, "Hybrid passes". */
enum { UH_HYBRID_RT_SHADOWS = 1u << 0, UH_HYBRID_GBUFFER = 1u << 1, UH_HYBRID_RT_REFLECTIONS = 1u << 2, UH_HYBRID_ALL = 7 };
/* which image uh_read_hybrid copies out (W*H texels each) */
enum {
   UH_HYBRID_POSITION = 0,   /* RGBA32F */
   UH_HYBRID_NORMAL = 1,     /* RGBA32F */
   UH_HYBRID_ALBEDO = 2,     /* RGBA8 */
   UH_HYBRID_PBR = 3,        /* RGBA32F */
   UH_HYBRID_SHADOWS = 4,    /* R8 */
   UH_HYBRID_REFLECTIONS = 5 /* RGBA8 */
};
/* the last uh_render_hybrid call: rays[0] G-buffer cast (0 for a rasterised G-buffer), rays[1] rt_shadows, rays[2] rt_reflections (= metal pixels); pass_ms the
 * hipEvent time of each pass in the same order (0 for a pass that did not run) */
typedef struct UhHybridStats {
   uint64_t rays[3];
   float pass_ms[3];
   uint32_t reflection_pixels;
   uint32_t reserved[2];
} UhHybridStats;
UH_LAYOUT_ASSERT(sizeof(UhHybridStats) == 48 && offsetof(UhHybridStats, pass_ms) == 24 && offsetof(UhHybridStats, reflection_pixels) == 36,
                 "UhHybridStats (48 B)");
int uh_render_hybrid(uh_ctx* ctx, const UhViewUniformData* view, uint32_t hybrid_mask);
int uh_read_hybrid(uh_ctx* ctx, int which, void* out); /* UH_ERR_INVALID_ARGUMENT before the first uh_render_hybrid */
int uh_get_hybrid_stats(uh_ctx* ctx, UhHybridStats* out);

/* ---- the hybrid graph's final frame: ssao_pass, deferred_pass, atmosphere_pass, present_pass (mod.rs:136-186) -------------
 * Four more bits of uh_render_hybrid, run after the three above in the reference's order:
 *   UH_HYBRID_SSAO      ssao.frag (radius 0.1, the 32 fixed kernel samples, randomVec (1, 1, 0), strength 1.6, no blur: ssao.rs) into
 *                       the R16 UNORM ssao_output; it does not run with view->ssao_enabled != 1 (ssao.rs:27)
 *   UH_HYBRID_DEFERRED  deferred.frag + pbr_lighting.glsl / brdf.glsl into the RGBA32F deferred_output: the sun as a directional light
 *                       of colour 1, then view->num_lights lights of the uh_add_light table (all 96 bytes of each: point, spot and
 *                       directional), ambient 0.03 * diffuse * occlusion, rt_reflections on metal pixels and rt_shadows (max(s, 0.3))
 *                       when view->raytracing_supported == 1, ssao_output when view->ssao_enabled == 1
 *   UH_HYBRID_SKY       atmosphere.frag, cubemap_enabled = 0 branch: IntegrateScattering along the un-jittered primary ray of every pixel
 *                       the G-buffer cast missed (a deviation: the reference draws the first mesh scaled by 1000 with a depth test)
 *   UH_HYBRID_PRESENT   present.frag + fxaa.glsl (threshold 0.45: present.rs; FXAA when view->fxaa_enabled == 1) + linearToSrgb into an
 *                       8-bit image of the layout and channel order of uh_read_output_bgra8 (B, G, R, A = 255), row 0 at the top
 * UH_HYBRID_FRAME runs all seven: rt_shadows (previous G-buffer), G-buffer, rt_reflections, SSAO, deferred, sky, present.
 * THE REFERENCE'S DEFAULTS (prototype/src/main.rs) SET shadows_enabled, ibl_enabled AND cubemap_enabled TO 1: a caller of these passes
 * must clear them, or build the maps they read: shadows_enabled with UH_HYBRID_SHADOW_MAPS, ibl_enabled and cubemap_enabled with
 * UH_HYBRID_ENVIRONMENT, below. UH_ERR_INVALID_ARGUMENT with a
 * message, and nothing runs, for UH_HYBRID_DEFERRED with view->shadows_enabled == 1 before the first shadow-map render (the cascaded
 * shadow maps of shadow.rs) or, before the first build, view->ibl_enabled == 1 (the IBL maps of ibl.rs), for UH_HYBRID_SKY with
 * view->cubemap_enabled == 1 before the first build (the environment cube of ibl.rs), and for UH_HYBRID_DEFERRED with view->num_lights
 * above the lights added with uh_add_light. view->marching_cubes_enabled is read by UH_HYBRID_MARCHING_CUBES, below; meshes of
 * uh_add_isosurface_mesh are scene geometry and go through the G-buffer like any other.
 * ORIENTATION (the reference draws under a Y-flipped viewport, pass.rs:260-267): deferred pixel (x, y) and present pixel (x, y) read the
 * G-buffer and deferred texel (x, y); ssao_output texel (x, y) is the occlusion of G-buffer texel (x, H-1-y) (ssao.frag samples at the
 * unflipped in_uv), and deferred pixel (x, y) reads ssao_output texel (x, H-1-y), so it is lit by its own texel's occlusion.
 * RESOURCES: the three images (22 bytes per pixel) are allocated by the first call whose mask holds one of these four bits, cleared to
 * (1, 1, 1, 0) (ssao 65535, present (255, 255, 255, 0)), and freed by uh_destroy; the light table goes with them. The passes change
 * nothing the path tracer or the three passes above read or report. Arithmetic: DESIGN.md section 2, "Hybrid frame passes". */
enum { UH_HYBRID_SSAO = 1u << 3, UH_HYBRID_DEFERRED = 1u << 4, UH_HYBRID_SKY = 1u << 5, UH_HYBRID_PRESENT = 1u << 6, UH_HYBRID_FRAME = 0x7f };
/* more images of uh_read_hybrid (W*H texels each) */
enum {
   UH_HYBRID_SSAO_IMAGE = 6,        /* uint16 (R16 UNORM) */
   UH_HYBRID_DEFERRED_OUTPUT = 7,   /* RGBA32F */
   UH_HYBRID_PRESENT_OUTPUT = 8     /* 8 bits x 4 channels, B G R A */
};
/* the last uh_render_hybrid call: pass_ms[k] the hipEvent time of the pass of bit k (rt_shadows, G-buffer, rt_reflections, SSAO, deferred,
 * sky, present; 0 for a pass that did not run; pass_ms[1] times the G-buffer pass cast or rasterised); sky_pixels the pixels the sky pass wrote; lights the lights the deferred pass evaluated
 * per pixel (the sun included; 0 when it did not run) */
typedef struct UhHybridFrameStats {
   float pass_ms[7];
   uint32_t sky_pixels;
   uint32_t lights;
   uint32_t reserved[3];
} UhHybridFrameStats;
UH_LAYOUT_ASSERT(sizeof(UhHybridFrameStats) == 48 && offsetof(UhHybridFrameStats, sky_pixels) == 28 && offsetof(UhHybridFrameStats, lights) == 32,
                 "UhHybridFrameStats (48 B)");
int uh_get_hybrid_frame_stats(uh_ctx* ctx, UhHybridFrameStats* out); /* waits; all zero before the first uh_render_hybrid */

/* ---- image-based lighting: setup_cubemap_pass (ibl.rs) and its consumers ---------------------------------------------------
 * One more bit of uh_render_hybrid, run where the reference adds the pass (mod.rs:121): after the G-buffer pass, before rt_reflections.
 *   UH_HYBRID_ENVIRONMENT  builds the four maps of ibl.rs at the reference's sizes, in its order:
 *     environment cube  cubemap.frag: RGBA32F, 512^2, 8 mips, every mip integrated from the atmosphere at its own size (not
 *                       downsampled); rayStart = the translation of view->inverse_view (extract_camera_position), view->sun_dir as
 *                       given (not normalised)
 *     irradiance cube   irradiance_filter.frag: RGBA32F, 512^2, 1 mip; the shader's 252 x 63 float-stepped taps in its order, on
 *                       environment mip 0
 *     specular cube     specular_filter.frag: RGBA32F, 512^2, 8 mips; 32 GGX taps at roughness mip / 7, trilinear environment lookups
 *     BRDF LUT          brdf_lut.frag: 512^2 R16G16_SFLOAT (fp16 pairs, rounded to nearest even), 1024 taps per texel
 * The reference rebuilds them when renderer.need_environment_map_update is set (the first frame, or on request); here the caller asks
 * by setting the bit. The maps persist in the context until the next call with the bit: moving the sun without it leaves them
 * stale, as there. UH_HYBRID_FRAME stays 0x7f: it does not build them.
 * CONSUMERS, once the maps exist (built by an earlier call or earlier in the same call):
 *   UH_HYBRID_DEFERRED with view->ibl_enabled == 1      ambient = imageBasedLighting (pbr_lighting.glsl:81-108) instead of 0.03 * diffuse * occlusion
 *   UH_HYBRID_SKY with view->cubemap_enabled == 1       textureLod(environment, dir * (1, -1, 1), 2) (atmosphere.frag:27-29), dir the
 *                                                       pixel's un-jittered primary-ray direction
 *   UH_HYBRID_RT_REFLECTIONS with view->ibl_enabled == 1  the hit shader's IBL branch (rt_reflections.rchit:50-61): imageBasedLighting of
 *                                                       the hit, stored like the non-IBL payload; the miss branch is unchanged
 * On a context whose maps were never built, these three are refused as before (UH_ERR_INVALID_ARGUMENT, nothing runs); the message
 * names UH_HYBRID_ENVIRONMENT. view->shadows_enabled == 1 needs the shadow maps of UH_HYBRID_SHADOW_MAPS, below.
 * RESOURCES: the four maps (about 93 MB) are allocated by the first call whose mask holds UH_HYBRID_ENVIRONMENT (UH_ERR_OUT_OF_MEMORY
 * when that fails) and freed by uh_destroy; a context that never sets the bit allocates nothing for them. A build changes no other
 * image of the hybrid graph and nothing in UhStats or UhHybridStats.
 * READ-BACK: uh_read_environment copies face `face` (0..5: +X, -X, +Y, -Y, +Z, -Z layers of the reference's cube) of mip `mip` of map
 * `which`: (512 >> mip)^2 texels, row 0 first. RGBA32F for the cubes; the LUT (face 0, mip 0) is 512^2 pairs of IEEE half floats
 * (R, G), row 0 first. UH_ERR_INVALID_ARGUMENT before the first build, and for an unknown map, face or mip. Waits like uh_read_hybrid.
 * Arithmetic (texel directions, cube addressing and seamless filtering, the deviations): DESIGN.md section 2, "Environment and IBL maps". */
enum { UH_HYBRID_ENVIRONMENT = 1u << 7 };
enum { UH_ENV_SIZE = 512, UH_ENV_MIPS = 8, UH_BRDF_LUT_SIZE = 512 };
enum {
   UH_ENV_ENVIRONMENT = 0, /* RGBA32F, 6 faces, 8 mips */
   UH_ENV_IRRADIANCE = 1,  /* RGBA32F, 6 faces, mip 0 */
   UH_ENV_SPECULAR = 2,    /* RGBA32F, 6 faces, 8 mips */
   UH_ENV_BRDF_LUT = 3     /* 2 x fp16, face 0, mip 0 */
};
int uh_read_environment(uh_ctx* ctx, int which, int face, int mip, void* out);
/* the last build: pass_ms the hipEvent time of its four sub-passes (environment, irradiance, specular, BRDF LUT); builds the number
 * of builds so far; sun_dir (as given) and eye (the translation of view->inverse_view) the maps were built with. All zero before the
 * first build. Waits for all work of the context. */
typedef struct UhEnvironmentStats {
   float pass_ms[4];
   uint32_t builds;
   float sun_dir[3];
   float eye[3];
   uint32_t reserved[5];
} UhEnvironmentStats;
UH_LAYOUT_ASSERT(sizeof(UhEnvironmentStats) == 64 && offsetof(UhEnvironmentStats, builds) == 16 && offsetof(UhEnvironmentStats, sun_dir) == 20 &&
                    offsetof(UhEnvironmentStats, eye) == 32,
                 "UhEnvironmentStats (64 B)");
int uh_get_environment_stats(uh_ctx* ctx, UhEnvironmentStats* out);

/* ---- cascaded shadow maps: setup_shadow_pass (shadow.rs) and the deferred pass's calculateShadow ---------------------------
 * uh_shadow_cascades is setup_shadow_pass's host arithmetic: four cascades, split lambda 0.927 between z_near and z_far, each an
 * orthographic light view of the sphere around its slice of the view frustum (corners from inverse(projection * view)). It takes no
 * context, needs no device, and fills the UBO_shadowmapParams of deferred.frag:28-32 byte for byte (column-major matrices,
 * split_depth = z_near + split * (z_far - z_near)). UH_ERR_INVALID_ARGUMENT, and *out untouched, for z_near <= 0, z_far <= z_near,
 * a non-finite input, a singular projection * view, a zero sun_dir or one parallel to +Y (look_at_rh degenerates), or any
 * non-finite result. The order of its float32 operations: DESIGN.md section 2, "Shadow maps".
 * uh_set_shadowmap_params copies params into the context (host state only: it waits for nothing). Every value must be finite and
 * every matrix's last row (0, 0, 0, 1), as the orthographic matrices of setup_shadow_pass are; UH_ERR_INVALID_ARGUMENT otherwise.
 * A caller that runs its own setup_shadow_pass passes its output here.
 * UH_HYBRID_SHADOW_MAPS (bit 8) of uh_render_hybrid renders all four cascades of the params last set into four D32 layers of
 * shadow_map_size^2 (option, default 4096): every triangle of every mesh, no culling, depth test LESS_OR_EQUAL cleared to 1.0, under
 * the Y-flipped viewport (pass.rs:260-267). It waits on the host: see STREAM ORDER above. It runs first in the call, before
 * rt_shadows (mod.rs:91-98), and only with
 * view->shadows_enabled == 1: otherwise the bit is a no-op and its pass_ms is 0 (setup_shadow_pass's early return). Without params
 * set, the call is UH_ERR_INVALID_ARGUMENT and nothing runs. UH_HYBRID_FRAME stays 0x7f: the reference's default view is
 * UH_HYBRID_FRAME | UH_HYBRID_SHADOW_MAPS (| UH_HYBRID_ENVIRONMENT).
 * CONSUMER: UH_HYBRID_DEFERRED with view->shadows_enabled == 1 multiplies by calculateShadow (shadow_mapping.glsl: cascade choice,
 * 3 x 3 PCF of bilinear depth reads, 0.3 / 1.0 per tap) instead of the rt_shadows factor, once maps exist (rendered earlier in the
 * same call or by an earlier one), with the params snapshot the maps were rendered with. Before that it is refused as before.
 * READ-BACK: uh_read_shadow_map copies layer `cascade` (0..3): size^2 floats, row 0 the texel row at NDC y = +1 (the first row of the
 * flipped viewport). UH_ERR_INVALID_ARGUMENT before the first render. Waits like uh_read_hybrid.
 * RESOURCES: the maps (16 bytes per texel of one layer) and the binning buffers are allocated by the first call that renders them
 * (UH_ERR_OUT_OF_MEMORY when that fails) and freed by uh_destroy; changing shadow_map_size frees them. A render that fails part way
 * (UH_ERR_OUT_OF_MEMORY, UH_ERR_CAPACITY) leaves no maps: the deferred pass with shadows is refused until a render completes. The pass changes no other
 * image, nothing in UhStats, UhHybridStats or UhHybridFrameStats. Arithmetic: DESIGN.md section 2, "Shadow maps". */
typedef struct UhShadowmapParams {
   float view_projection_matrices[4][16]; /* column-major, cascade c at [c] */
   float cascade_splits[4];               /* split depths (view-space distances) */
} UhShadowmapParams;
UH_LAYOUT_ASSERT(sizeof(UhShadowmapParams) == 272 && offsetof(UhShadowmapParams, cascade_splits) == 256, "UhShadowmapParams (272 B)");
enum { UH_HYBRID_SHADOW_MAPS = 1u << 8, UH_SHADOW_CASCADES = 4 };
int uh_shadow_cascades(const float view[16], const float projection[16], float z_near, float z_far, const float sun_dir[3], UhShadowmapParams* out);
int uh_set_shadowmap_params(uh_ctx* ctx, const UhShadowmapParams* params);
int uh_read_shadow_map(uh_ctx* ctx, int cascade, float* out);
/* the last shadow-map render: pass_ms its hipEvent time, renders the number so far, size the maps' size, triangles[c] the triangles
 * of cascade c that reached the rasteriser (after the setup's rejects; a triangle clipped to the guard band counts once per piece),
 * params the snapshot the deferred pass reads. All zero before the first render. Waits for all work of the context. */
typedef struct UhShadowMapStats {
   float pass_ms;
   uint32_t renders;
   uint32_t size;
   uint32_t triangles[4];
   uint32_t reserved;
   UhShadowmapParams params;
} UhShadowMapStats;
UH_LAYOUT_ASSERT(sizeof(UhShadowMapStats) == 304 && offsetof(UhShadowMapStats, triangles) == 12 && offsetof(UhShadowMapStats, params) == 32,
                 "UhShadowMapStats (304 B)");
int uh_get_shadow_map_stats(uh_ctx* ctx, UhShadowMapStats* out);

/* ---- the forward graph: build_minimal_forward_render_graph (utopian/src/renderers/mod.rs; the reference's render mode 3) ----------
 * uh_render_forward runs the three passes of the reference's Minimal mode, in its order, for the bits of `mask`:
 *   UH_FORWARD_SHADOW_MAPS  setup_shadow_pass: the same pass and the same four maps as UH_HYBRID_SHADOW_MAPS (above), rendered from the
 *                           params last set, only with view->shadows_enabled == 1 (otherwise a no-op), first in the call
 *   UH_FORWARD_PASS         setup_forward_pass (forward.vert / forward.frag): every triangle of every mesh in order (the draw index of a
 *                           triangle is its mesh's first triangle plus its primitive, meshes in the order added) through a perspective
 *                           rasteriser - clip to 0 <= z <= w, the viewport (0, H, W, -H), the shadow maps' guard band, 8-bit snap and
 *                           top-left rule, no culling, one sample per pixel at its centre, depth LESS_OR_EQUAL with writes, cleared to
 *                           1.0 - then forward.frag once per pixel on the surviving fragment (the last in draw order among those of
 *                           minimum depth), with perspective-correct attributes: the unquantised diffuse texel ^ 2.2 times the
 *                           material's base_color_factor, metallic and roughness from the texture without the factors, the sun plus
 *                           view->num_lights lights through surfaceShading, ambient 0.03 * diffuse * occlusion, calculateShadow when
 *                           view->shadows_enabled == 1; no IBL, SSAO, reflections or rt_shadows. Colour cleared to (1, 1, 1, 0).
 *   UH_FORWARD_PRESENT      setup_present_pass: present.frag + FXAA (view->fxaa_enabled == 1) as UH_HYBRID_PRESENT, reading forward_output
 *                           and writing the forward graph's own 8-bit image (the hybrid graph's present image is untouched)
 * UH_FORWARD_GRAPH runs all three. view->raytracing_supported is not read: the graph needs no ray tracing.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, for a null view, UH_FORWARD_SHADOW_MAPS (with shadows_enabled == 1) before
 * uh_set_shadowmap_params, and UH_FORWARD_PASS with view->shadows_enabled == 1 before any shadow-map render (by either graph) or with
 * view->num_lights above the lights added; UH_ERR_NOT_BUILT before the first build (moved instances with view->rebuild_tlas as for
 * uh_render_frame); UH_ERR_CAPACITY for a frame wider or taller than 65535 pixels or 2^32 - 1 or more triangle pieces.
 * ORIENTATION: every forward image is W*H texels, row-major, row 0 the pixel row at NDC y = +1 (the first row of the flipped viewport,
 * as uh_read_shadow_map) - the layout of the hybrid graph's images: forward pixel (x, y) and G-buffer texel (x, y) see the same point.
 * STREAM ORDER: a call enqueues like uh_render_hybrid (behind the frames in flight, on the context's first stream), but UH_FORWARD_PASS
 * BLOCKS the host until the frames in flight and the pass's binning have finished: it reads the number of triangle pieces and tile
 * entries back to size its buffers, as UH_FORWARD_SHADOW_MAPS does. uh_read_forward and uh_get_forward_stats wait and are complete on
 * return.
 * RESOURCES: the images (37 bytes per pixel with the visibility buffer's record ids) are allocated by the first call, cleared, and
 * freed by uh_destroy; the binning buffers grow with the scene. A context that never calls uh_render_forward allocates nothing for it.
 * The graph shares the hybrid graph's mesh tables, light table and shadow maps.
 * ISOLATION: a call changes no path-traced or hybrid image and nothing in UhStats, UhHybridStats or UhHybridFrameStats; the one
 * exception is the shadow maps (and UhShadowMapStats) when its mask renders them.
 * Arithmetic: DESIGN.md section 2, "Forward pass". */
enum { UH_FORWARD_PASS = 1u << 0, UH_FORWARD_PRESENT = 1u << 1, UH_FORWARD_SHADOW_MAPS = UH_HYBRID_SHADOW_MAPS, UH_FORWARD_GRAPH = UH_HYBRID_SHADOW_MAPS | 3u };
/* which image uh_read_forward copies out (W*H texels each) */
enum {
   UH_FORWARD_OUTPUT = 0,         /* RGBA32F forward_output */
   UH_FORWARD_DEPTH = 1,          /* float32 depth, 1.0 where nothing was drawn */
   UH_FORWARD_VISIBILITY = 2,     /* uint32 draw index of the surviving fragment, 0xFFFFFFFF for none */
   UH_FORWARD_PRESENT_OUTPUT = 3  /* 8 bits x 4 channels, B G R A (as uh_read_output_bgra8) */
};
/* the last uh_render_forward call: pass_ms the hipEvent time of (shadow maps, forward, present), 0 for a pass that did not run;
 * renders the calls that ran the forward pass so far; pieces the triangle pieces that reached the rasteriser (after clipping and the
 * setup's rejects), covered_pixels the pixels with a surviving fragment and lights the lights forward.frag evaluated (the sun
 * included), all three of the last forward pass. All zero before the first call. Waits for all work of the context. */
typedef struct UhForwardStats {
   float pass_ms[3];
   uint32_t renders;
   uint32_t pieces;
   uint32_t covered_pixels;
   uint32_t lights;
   uint32_t reserved;
} UhForwardStats;
UH_LAYOUT_ASSERT(sizeof(UhForwardStats) == 32 && offsetof(UhForwardStats, renders) == 12 && offsetof(UhForwardStats, pieces) == 16 &&
                    offsetof(UhForwardStats, covered_pixels) == 20 && offsetof(UhForwardStats, lights) == 24,
                 "UhForwardStats (32 B)");
int uh_render_forward(uh_ctx* ctx, const UhViewUniformData* view, uint32_t mask);
int uh_read_forward(uh_ctx* ctx, int which, void* out); /* UH_ERR_INVALID_ARGUMENT before the first uh_render_forward */
int uh_get_forward_stats(uh_ctx* ctx, UhForwardStats* out);

/* ---- the hybrid graph's marching-cubes pass: setup_marching_cubes_pass (mod.rs:164-174, renderers/marching_cubes.rs) ------------
 * UH_HYBRID_MARCHING_CUBES (bit 10; bit 9 stays unused and ignored) of uh_render_hybrid runs after UH_HYBRID_DEFERRED and before
 * UH_HYBRID_SKY, the reference's order, and only with view->marching_cubes_enabled == 1: otherwise the bit is a no-op and its pass_ms
 * is 0. UH_HYBRID_FRAME stays 0x7f: the reference's default hybrid view with the checkbox on is
 * UH_HYBRID_FRAME | UH_HYBRID_SHADOW_MAPS | UH_HYBRID_MARCHING_CUBES. Every call that runs it:
 *   extraction      marching_cubes.comp on the device at view->time: the reference's 32^3 grid of voxel size 1 from the origin, the
 *                   reference's triangulation (whatever the option iso_reference_triangulation says). pos and normal equal, bit for
 *                   bit, those of uh_add_isosurface_mesh(ctx, 32, 0.0f, 32.0f, view->time, ...) with that triangulation; uv, colour
 *                   and tangent are zero. The draw index of a triangle is its place in extraction order (cells x fastest, then the
 *                   case list). The triangles are a transient buffer, not scene geometry: no mesh is added, and they are in no tree,
 *                   shadow map, rt_shadows or rt_reflections ray.
 *   depth buffer    the reference rasterises it in the G-buffer pass; here it comes from the G-buffer last rendered: per pixel
 *                   d = c.z / c.w with c = (P V) (position, 1), kept when c.w > 0 and 0 <= d <= 1, else 1.0; 1.0 where the cast missed
 *   draw            forward.vert / forward.frag (world = identity, mesh_index = 0) through the forward pass's rasteriser, depth test
 *                   LESS_OR_EQUAL with writes against that buffer (a fragment at exactly the G-buffer's depth is drawn), shaded
 *                   with the material of the FIRST MESH ADDED (its maps and base_color_factor: the reference's quirk) at uv (0, 0),
 *                   the sun plus view->num_lights lights, ambient 0.03 * diffuse * occlusion, calculateShadow when
 *                   view->shadows_enabled == 1; (colour, 1) into deferred_output at covered pixels, every other pixel untouched
 *   sky             UH_HYBRID_SKY in the same call skips the pixels a marching-cubes fragment covers (the atmosphere pass's
 *                   depth test): sky_pixels drops by as many
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, when the bit is set with view->marching_cubes_enabled == 1 and no
 * G-buffer was rendered (by this call or an earlier one), the scene has no mesh, view->shadows_enabled == 1 and no shadow-map render
 * has completed (by this call or an earlier one), or view->num_lights is above the lights added. UH_ERR_NOT_BUILT and moved
 * instances as for the other bits.
 * STREAM ORDER: the pass BLOCKS the host until the frames in flight, the passes before it in the call and its extraction and binning
 * have finished: it reads the triangle count and the binning totals back to size its buffers, as UH_FORWARD_PASS does.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first pass): UH_HYBRID_DEPTH, the float32 depth buffer after the last
 * pass, and UH_HYBRID_MARCHING_CUBES_VISIBILITY, the uint32 draw index of the surviving marching-cubes fragment or 0xFFFFFFFF;
 * W*H texels, row 0 at NDC y = +1 as the other hybrid images.
 * RESOURCES: the depth, visibility and triangle buffers (and the binning buffers, which grow with the mesh) are allocated by the first
 * pass (and the final frame's images, if no earlier call allocated them) and freed by uh_destroy.
 * ISOLATION: with the bit absent or the flag 0 nothing changes. The pass writes deferred_output and its own buffers only: no
 * path-traced image, G-buffer, rt_shadows, rt_reflections, forward or shadow-map image, and nothing in UhStats, UhHybridStats,
 * UhShadowMapStats or UhHybridFrameStats beyond the sky pass's sky_pixels.
 * Arithmetic: DESIGN.md section 2, "Marching-cubes pass". */
enum { UH_HYBRID_MARCHING_CUBES = 1u << 10 };
enum {
   UH_HYBRID_DEPTH = 9,                     /* float32 */
   UH_HYBRID_MARCHING_CUBES_VISIBILITY = 10 /* uint32 draw index, 0xFFFFFFFF for none */
};
/* the last pass: pass_ms its hipEvent time (0 when the last call with the bit did not run it); renders the passes so far; triangles
 * extracted (zero-area ones included), pieces that reached the rasteriser, covered_pixels with a surviving fragment, lights evaluated
 * (the sun included) and the view->time used, all of the last pass that ran. All zero before the first pass. Waits for all work of
 * the context. */
typedef struct UhMarchingCubesStats {
   float pass_ms;
   uint32_t renders;
   uint32_t triangles;
   uint32_t pieces;
   uint32_t covered_pixels;
   uint32_t lights;
   float time;
   uint32_t reserved;
} UhMarchingCubesStats;
UH_LAYOUT_ASSERT(sizeof(UhMarchingCubesStats) == 32 && offsetof(UhMarchingCubesStats, triangles) == 8 && offsetof(UhMarchingCubesStats, pieces) == 12 &&
                    offsetof(UhMarchingCubesStats, covered_pixels) == 16 && offsetof(UhMarchingCubesStats, lights) == 20 &&
                    offsetof(UhMarchingCubesStats, time) == 24,
                 "UhMarchingCubesStats (32 B)");
int uh_get_marching_cubes_stats(uh_ctx* ctx, UhMarchingCubesStats* out);

/* ---- the hybrid graph's G-buffer pass rasterised: gbuffer_pass (renderers/gbuffer.rs, gbuffer.vert / gbuffer.frag) ---------------------
 * UH_HYBRID_GBUFFER_RASTER (bit 11; bit 9 stays unused and ignored) is a modifier of UH_HYBRID_GBUFFER: with both bits set, the
 * G-buffer pass of that call is drawn through the forward pass's rasteriser instead of cast, as the reference draws it. UH_HYBRID_FRAME
 * stays 0x7f and the cast stays the default: the reference's default frame is
 * UH_HYBRID_FRAME | UH_HYBRID_GBUFFER_RASTER | UH_HYBRID_SHADOW_MAPS. The pass runs at the G-buffer's slot (rt_shadows of the same call
 * still reads the PREVIOUS G-buffer, whichever kind it was):
 *   raster      UH_FORWARD_PASS's stages unchanged - every triangle of every mesh in draw order, clip to 0 <= z <= w, the viewport
 *               (0, H, W, -H), guard band, snap, top-left rule, no culling, one sample at the pixel centre, LESS_OR_EQUAL with writes
 *               against a depth buffer cleared to 1.0 - so its depth and visibility equal uh_render_forward's UH_FORWARD_DEPTH and
 *               UH_FORWARD_VISIBILITY for the same view, bit for bit
 *   fragment    gbuffer.frag once per covered pixel on the surviving fragment with perspective-correct attributes: position the
 *               interpolated (world (p, 1), 1), and normal, albedo and pbr as the cast's resolve writes them (above)
 *   uncovered   the clear values of the cast's miss: (1, 1, 1, 0), albedo (255, 255, 255, 0)
 *   depth       the marching-cubes pass after a rasterised G-buffer depth-tests against this depth buffer, bit for bit (the reference's
 *               shared attachment); after a cast it reconstructs the depth from the positions, as described above. The choice follows
 *               the G-buffer pass that ran last, in this call or an earlier one.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, for the bit without UH_HYBRID_GBUFFER. UH_ERR_NOT_BUILT and moved
 * instances with view->rebuild_tlas as for UH_HYBRID_GBUFFER; UH_ERR_CAPACITY, as in uh_render_forward, for a frame wider or taller
 * than 65535 pixels or 2^32 - 1 or more triangle pieces.
 * STREAM ORDER: the pass BLOCKS the host until the frames in flight, the passes before it in the call and its binning have finished: it
 * reads the binning totals back to size its buffers, as UH_FORWARD_PASS does. The passes after it are enqueued as usual.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first rasterised pass): UH_HYBRID_GBUFFER_DEPTH, the float32 depth
 * buffer, and UH_HYBRID_GBUFFER_VISIBILITY, the uint32 draw index of the surviving fragment or 0xFFFFFFFF; both after the last
 * rasterised pass, W*H texels, row 0 at NDC y = +1 as the other hybrid images. UH_HYBRID_DEPTH stays the marching-cubes pass's buffer.
 * RESOURCES: about 12 bytes per pixel (depth, visibility, surviving record) and binning buffers that grow with the scene, allocated by
 * the first rasterised pass and freed by uh_destroy. A context that never sets the bit allocates nothing for it.
 * ISOLATION: the pass writes the four G-buffer targets and its own depth and visibility: no forward-graph image, path-traced image,
 * reservoir or shadow map, and nothing in UhStats or UhForwardStats. In UhHybridFrameStats pass_ms[1] times the G-buffer pass
 * whichever way it ran; in UhHybridStats rays[0] is 0 for a rasterised pass. The path-tracing graph's UH_PASS_GBUFFER stays a cast.
 * Arithmetic: DESIGN.md section 2, "Rasterised G-buffer". */
enum { UH_HYBRID_GBUFFER_RASTER = 1u << 11 };
enum {
   UH_HYBRID_GBUFFER_DEPTH = 11,     /* float32, 1.0 where nothing was drawn */
   UH_HYBRID_GBUFFER_VISIBILITY = 12 /* uint32 draw index, 0xFFFFFFFF for none */
};
/* the last rasterised G-buffer pass: pass_ms its hipEvent time (0 when the last call that ran a G-buffer pass cast it, or when the
 * last call ran none); renders the rasterised passes so far; pieces the triangle pieces that reached the rasteriser (after clipping
 * and the setup's rejects) and covered_pixels the pixels with a surviving fragment, both of the last rasterised pass. All zero before
 * the first one. Waits for all work of the context. */
typedef struct UhGbufferRasterStats {
   float pass_ms;
   uint32_t renders;
   uint32_t pieces;
   uint32_t covered_pixels;
} UhGbufferRasterStats;
UH_LAYOUT_ASSERT(sizeof(UhGbufferRasterStats) == 16 && offsetof(UhGbufferRasterStats, renders) == 4 && offsetof(UhGbufferRasterStats, pieces) == 8 &&
                    offsetof(UhGbufferRasterStats, covered_pixels) == 12,
                 "UhGbufferRasterStats (16 B)");
int uh_get_gbuffer_raster_stats(uh_ctx* ctx, UhGbufferRasterStats* out);

/* ---- the hybrid frame's local lights from the ReSTIR reservoirs: one light and one shadow ray per pixel ---------------------------------
 * An EXTENSION: the reference's hybrid graph with reservoirs (build_hybrid_render_graph, renderers/mod.rs:377-391) is an empty "Todo".
 * UH_HYBRID_RESTIR_LIGHTS (bit 12; bit 9 stays unused and ignored) does two things in one uh_render_hybrid call:
 *   restir_lights   a pass of its own after rt_reflections and before SSAO. A pixel casts a ray exactly when its position texel is geometry
 *                   (w != 0), its spatial reservoir r has 0 <= r.Y < view->num_lights, light r.Y is a point or spot light (light_type 1
 *                   or 2), r.W_X is finite and > 0, and the light is above the pixel's horizon (the deferred pass's own NdotL of that light
 *                   is not 0; NaN counts as 0). The ray is the path tracer's light shadow ray (reference.rgen:113-119) from offsetRay of the
 *                   pixel's own position and normal texels toward the light's position: tmin 0.001, tmax 10000, occluded when a triangle
 *                   has tmin < t < tmax and t <= the distance. The pass writes the light-visibility image: 255 where a ray was cast and
 *                   found the light, 0 where it was occluded or none was cast.
 *   deferred        UH_HYBRID_DEFERRED of the same call evaluates the sun with its light loop and then, where the visibility texel is 255,
 *                   adds the one light of the pixel's reservoir - one iteration of the same loop on that light's record - times r.W_X,
 *                   instead of looping over all view->num_lights lights unshadowed. Everything after the loop is unchanged.
 *                   UhHybridFrameStats.lights reports 2.
 * RESERVOIRS: the ones uh_read_reservoirs(ctx, 2) reads - whatever the last uh_render_frame with UH_PASS_RESTIR or more left. Rendering
 * them with the SAME CAMERA (and lights) as this call's view is the caller's job: nothing checks it. The pass only reads them. A light
 * the reservoir passes never sample lights nothing in this mode: lights beyond view->max_num_lights_used, lights of another type, and
 * lights whose `intensity` has zero luminance.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs: the bit with view->raytracing_supported != 1; no G-buffer rendered in this
 * call or an earlier one; no reservoir pass has ever run on the context; a reservoir row partition with world > 1 is set
 * (uh_set_restir_partition); and, as without the bit, UH_HYBRID_DEFERRED with view->num_lights above the lights added.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first call with the bit): UH_HYBRID_LIGHT_VISIBILITY, R8, W*H texels.
 * RESOURCES: 5 bytes per pixel (the image and a queue of the pixels that cast), allocated by the first call with the bit, the image
 * cleared to 0; freed by uh_destroy. A context that never sets the bit allocates nothing for it.
 * STREAM ORDER: as uh_render_hybrid; a reservoir pass enqueued later starts behind this call's reads.
 * ISOLATION: the bit changes no reservoir, accumulation, gbuffer_position, grid or UhStats, and no hybrid image but the two named; its
 * rays are counted in UhHybridRestirStats only. Without the bit every pass is what it was. No uh_mgpu_ twin.
 * Arithmetic: DESIGN.md section 2, "Reservoir lights". */
enum { UH_HYBRID_RESTIR_LIGHTS = 1u << 12 };
enum { UH_HYBRID_LIGHT_VISIBILITY = 13 /* R8: 255 lit, 0 occluded or no ray */ };
/* the last call with the bit: rays cast, how many of them were occluded, and the pass's hipEvent time. All zero before the first call
 * with the bit. Waits for all work of the context. */
typedef struct UhHybridRestirStats {
   uint64_t rays;
   uint64_t occluded;
   float pass_ms;
   uint32_t reserved[3];
} UhHybridRestirStats;
UH_LAYOUT_ASSERT(sizeof(UhHybridRestirStats) == 32 && offsetof(UhHybridRestirStats, occluded) == 8 && offsetof(UhHybridRestirStats, pass_ms) == 16 &&
                    offsetof(UhHybridRestirStats, reserved) == 20,
                 "UhHybridRestirStats (32 B)");
int uh_get_hybrid_restir_stats(uh_ctx* ctx, UhHybridRestirStats* out);

/* ---- the denoiser: reprojected history and a variance-guided a-trous filter over a path-traced frame ------------------------------------
 * An EXTENSION: the reference has no denoiser. uh_denoise is SVGF (Schied et al. 2017) cut short: temporal accumulation of colour and
 * luminance moments through view->prev_frame_projection_view, a spatial variance estimate where the history is shorter than 4 frames,
 * and `iterations` levels of an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by normals, plane distance and
 * luminance over that variance. Per-context verbs: no uh_mgpu_ twin.
 * INPUTS, all already on the device: the accumulation image as the last uh_render_frame left it, divided by
 * n = min(view->total_samples, view->accumulation_limit) (reference.rgen:140), and the hybrid G-buffer (position, normal, albedo, and the
 * mesh index in pbr.a) of the last uh_render_hybrid(..., UH_HYBRID_GBUFFER ...). Rendering both with the SAME CAMERA as `view` is the
 * caller's job: nothing checks it. A caller that wants one frame's samples renders each frame with total_samples = samples_per_frame
 * (the reference's own protocol after a camera move); the filter takes the accumulation for what it is. A pixel is geometry when its
 * position texel has w != 0; every other pixel passes through unchanged, is never a tap, and has history 0 and variance 0.
 * view->prev_frame_projection_view is projection * view of the previous uh_denoise call; view->view gives the depth the plane
 * tolerances scale with.
 * NON-FINITE INPUT: a geometry pixel is BAD when a channel of its accumulation / n is NaN, infinite or above 2^48 (281474976710656) in
 * magnitude - the bound keeps every later product and difference finite ("Non-finite input"). A bad pixel is
 * treated exactly as a pixel that is not geometry, in this call and in the history it leaves: its colour, not demodulated, passes
 * through to every colour image unchanged, it is never a tap, its history is 0 and its variance 0, and the next call fetches no
 * history from it. Every other pixel of every image is finite, whatever the bad ones hold, and stays so in the calls that follow.
 * So UH_DENOISE_HISTORY == 0 means "took no part": not geometry, or bad. geometry_pixels still counts position w != 0, the bad
 * pixels included; history_pixels never counts one.
 * HISTORY: the call keeps its own copies of this frame's position, normal with the mesh index beside it, temporal colour, history
 * length and moments for the next call (the hybrid targets are overwritten by then). Without UH_DENOISE_MOTION the scene is assumed
 * static between calls: after uh_update_isosurface_mesh / uh_update_mesh_vertices / uh_set_instance_transform with a refit, render the
 * G-buffer with UH_HYBRID_MOTION and set UH_DENOISE_MOTION (below, "motion vectors") and the history follows the moved mesh; without
 * the flag, call uh_reset_denoise_history, or accept ghosting on the moved mesh. Without UH_DENOISE_TEMPORAL every call starts from no
 * history (and still leaves one).
 * UH_DENOISE_MOTION (bit 3; bit 2 stays an unknown flag): with UH_DENOISE_TEMPORAL, a geometry pixel whose motion texel
 * (UH_HYBRID_MOTION_IMAGE) has w == 1 reprojects that texel's xyz - where its surface point was at the previous motion pass - instead of
 * its position: through prev_frame_projection_view, and in the plane test |dot(q - p_prev, n)| <= tol. The normal n, the mesh-index test,
 * tol (from the CURRENT view depth) and the bilinear weights are as without the flag. A pixel whose motion texel has w == 0 keeps no
 * history: N = 1, this frame's colour and moments, not counted in history_pixels. The history normal is still compared with the current
 * normal: a mesh that turns by more than acos(reproject_normal_cos) in one frame loses its history (noise, not ghosting). Without
 * UH_DENOISE_TEMPORAL the flag is accepted and has no effect. On a static scene the flag changes no bit of any image.
 * UH_ERR_INVALID_ARGUMENT with a message - nothing runs, the history is untouched: a null view or params; no hybrid G-buffer rendered
 * yet; n == 0; iterations > 5; a non-zero reserved word; unknown flag bits; a parameter outside its range (below) or not finite; a
 * tile partition with world > 1 is set (uh_set_tile_partition: the accumulation is then partial); UH_DENOISE_MOTION when the last
 * G-buffer pass had no UH_HYBRID_MOTION. UH_ERR_NOT_BUILT before
 * uh_build_acceleration, as for a frame.
 * ISOLATION: the call changes no accumulation, reservoir, gbuffer_position, hybrid image, grid or UhStats.
 * RESOURCES: 204 bytes per pixel (two history sets of 56, two filter images of 16, the input, temporal and colour images of 16, the
 * 8-bit image, history length and variance of 4 each), allocated by the first uh_denoise (UH_ERR_OUT_OF_MEMORY when that fails) and
 * freed by uh_destroy. A context that never calls uh_denoise allocates nothing for it.
 * STREAM ORDER: uh_denoise enqueues like uh_render_hybrid (behind the frames in flight, on the context's first stream; a frame enqueued
 * later accumulates behind the call's read of the accumulation). uh_read_denoised, uh_get_denoise_stats and uh_reset_denoise_history
 * wait and are complete on return.
 * Arithmetic: DESIGN.md section 2, "Denoiser: the arithmetic contract of uh_denoise". */
enum { UH_DENOISE_TEMPORAL = 1u << 0, UH_DENOISE_DEMODULATE = 1u << 1 };
enum { UH_DENOISE_MOTION = 1u << 3 /* bit 2 stays an unknown flag */ };
typedef struct UhDenoiseParams {
   uint32_t flags;             /* UH_DENOISE_* */
   uint32_t iterations;        /* a-trous levels, 0..5; level i has step 2^i */
   uint32_t max_history;       /* >= 1; default 32 */
   float alpha_min;            /* [0, 1]; default 0.2 (SVGF) */
   float sigma_luminance;      /* > 0; default 4 (SVGF) */
   float sigma_plane;          /* > 0; plane distance tolerated, as a fraction of view depth; default 0.005 */
   float reproject_normal_cos; /* [-1, 1]; default 0.9 */
   float reproject_plane;      /* > 0; the same fraction, for history taps; default 0.005 */
   uint32_t reserved[4];       /* must be 0 */
} UhDenoiseParams;
UH_LAYOUT_ASSERT(sizeof(UhDenoiseParams) == 48 && offsetof(UhDenoiseParams, iterations) == 4 && offsetof(UhDenoiseParams, max_history) == 8 &&
                    offsetof(UhDenoiseParams, alpha_min) == 12 && offsetof(UhDenoiseParams, sigma_luminance) == 16 &&
                    offsetof(UhDenoiseParams, sigma_plane) == 20 && offsetof(UhDenoiseParams, reproject_normal_cos) == 24 &&
                    offsetof(UhDenoiseParams, reproject_plane) == 28 && offsetof(UhDenoiseParams, reserved) == 32,
                 "UhDenoiseParams (48 B)");
/* which image uh_read_denoised copies out (W*H texels each), all of the last uh_denoise call */
enum {
   UH_DENOISE_COLOR = 0,          /* RGBA32F: the filtered colour, linear, alpha 0 like the accumulation */
   UH_DENOISE_OUTPUT = 1,         /* 8 bits x 4 channels, B G R A: the filtered colour through the path tracer's linearToSrgb and packing */
   UH_DENOISE_INPUT = 2,          /* RGBA32F: what the filter read (accumulation / n, demodulated on geometry with UH_DENOISE_DEMODULATE) */
   UH_DENOISE_TEMPORAL_COLOR = 3, /* RGBA32F: the colour after the temporal stage, remodulated */
   UH_DENOISE_HISTORY = 4,        /* float32: history length N (0 where not geometry, and at a bad pixel: "NON-FINITE INPUT" above) */
   UH_DENOISE_VARIANCE = 5        /* float32: the variance level 0 of the filter read */
};
/* the last uh_denoise call: pass_ms the hipEvent time of its stages (input + temporal, variance estimate, all a-trous levels, output),
 * geometry_pixels the pixels whose position texel has w != 0, history_pixels those of them that kept a history (a valid reprojection).
 * All zero before the first call. Waits for all work of the context. */
typedef struct UhDenoiseStats {
   float pass_ms[4];
   uint32_t geometry_pixels;
   uint32_t history_pixels;
   uint32_t reserved[2];
} UhDenoiseStats;
UH_LAYOUT_ASSERT(sizeof(UhDenoiseStats) == 32 && offsetof(UhDenoiseStats, geometry_pixels) == 16 && offsetof(UhDenoiseStats, history_pixels) == 20 &&
                    offsetof(UhDenoiseStats, reserved) == 24,
                 "UhDenoiseStats (32 B)");
int uh_denoise_default_params(UhDenoiseParams* out); /* needs no GPU; UH_ERR_INVALID_ARGUMENT for NULL */
int uh_denoise(uh_ctx* ctx, const UhViewUniformData* view, const UhDenoiseParams* params);
int uh_reset_denoise_history(uh_ctx* ctx);           /* the next uh_denoise starts from no history */
int uh_read_denoised(uh_ctx* ctx, int which, void* out); /* UH_ERR_INVALID_ARGUMENT before the first uh_denoise */
int uh_get_denoise_stats(uh_ctx* ctx, UhDenoiseStats* out);

/* ---- ray-traced ambient occlusion for the hybrid frame: short hemisphere rays instead of ssao.frag ---------------------------------------
 * An EXTENSION: the reference's ambient occlusion is ssao.frag alone (32 fixed kernel samples, a constant "random" vector, what is on
 * screen, no blur). UH_HYBRID_RTAO (bit 13; bit 9 stays unused and ignored) takes the SSAO slot of uh_render_hybrid: with the bit set and
 * view->ssao_enabled == 1 the rtao pass writes ssao_output (UH_HYBRID_SSAO_IMAGE, R16 UNORM) and ssao.frag's kernel is not launched,
 * whether or not UH_HYBRID_SSAO is set - UH_HYBRID_FRAME | UH_HYBRID_RTAO is the natural call. With ssao_enabled != 1 the pass does not
 * run and the image keeps what it held, as for SSAO. The deferred pass is untouched: it reads ssao_output as it always has.
 *   rays      a G-buffer pixel (px, py) whose position texel has w != 0 and whose normal texel N normalises to a finite Nn casts
 *             `samples` rays from offsetRay(P, Nn) of its OWN texels. Ray s has direction normalize(Nn + normalize(u)), u =
 *             randomPointInUnitSphere of the state initRNG(px, py, W, frameNumber(view) * 64 + s) (random.glsl) - the closest-hit
 *             shader's Lambertian scatter, cosine-weighted; Nn itself where |Nn + normalize(u)|^2 < 1e-12. It is occluded when a triangle
 *             has 0.001 < t < 10000 and t <= radius. count = the pixel's occluded rays; every other pixel casts nothing, count 0.
 *   image     ao = 1 - strength * ((float)count / (float)samples), 1 where no ray was cast. blur_radius 0: ssao_output = unorm16(ao).
 *             blur_radius r: a geometry pixel gets the mean of ao over the taps (dx, dy) in [-r, r)^2 (blur.frag's window) that lie in
 *             the frame, cast rays themselves, and pass dot(Nn_tap, Nn) >= blur_normal_cos and |dot(P_tap - P, Nn)| <= blur_plane; the
 *             centre always counts. Texel (x, y) of ssao_output belongs to G-buffer pixel (x, H - 1 - y), as ssao.frag writes it.
 * PARAMS: uh_set_rtao_params validates and keeps them for the calls that follow (a refused call leaves the old ones); before the
 * first call the defaults of uh_rtao_default_params hold: 4 samples, radius 1.0, strength 1.0, blur_radius 2, 0.9, 0.05.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs: the bit (with ssao_enabled == 1) and view->raytracing_supported != 1; no
 * G-buffer rendered in this call or an earlier one. UH_ERR_NOT_BUILT before uh_build_acceleration, as without the bit.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first rtao pass): UH_HYBRID_AO_COUNTS, one byte per pixel in G-buffer
 * orientation: the pixel's occluded rays, 0 where none were cast.
 * RESOURCES: 5 bytes per pixel (the counts and a queue of the pixels that cast), allocated by the first pass; freed by uh_destroy. A
 * context that never sets the bit allocates nothing for it.
 * STREAM ORDER: as uh_render_hybrid. uh_set_rtao_params is host state, read by the next uh_render_hybrid; uh_get_rtao_stats waits.
 * ISOLATION: the bit changes no reservoir, accumulation, gbuffer_position, grid or UhStats, and no hybrid image but ssao_output and the
 * counts; its rays are counted in UhRtaoStats only. Without the bit every pass is what it was. No uh_mgpu_ twin.
 * Arithmetic: DESIGN.md section 2, "Ray-traced ambient occlusion". */
enum { UH_HYBRID_RTAO = 1u << 13 };
enum { UH_HYBRID_AO_COUNTS = 14 /* uint8 per pixel, G-buffer orientation: occluded rays of the pixel, 0 where none were cast */ };
typedef struct UhRtaoParams {
   uint32_t samples;      /* rays per geometry pixel, 1..64 */
   float radius;          /* world units; finite, > 0, <= 10000 */
   float strength;        /* ao = 1 - strength * occluded / samples; finite, >= 0 */
   uint32_t blur_radius;  /* 0 = no filter; else 1..4: taps dx, dy in [-r, r) as blur.frag */
   float blur_normal_cos; /* a tap counts when dot(Nn_tap, Nn) >= this; not NaN */
   float blur_plane;      /* and |dot(P_tap - P, Nn)| <= this (world units); not NaN */
} UhRtaoParams;
UH_LAYOUT_ASSERT(sizeof(UhRtaoParams) == 24 && offsetof(UhRtaoParams, radius) == 4 && offsetof(UhRtaoParams, strength) == 8 &&
                    offsetof(UhRtaoParams, blur_radius) == 12 && offsetof(UhRtaoParams, blur_normal_cos) == 16 &&
                    offsetof(UhRtaoParams, blur_plane) == 20,
                 "UhRtaoParams (24 B)");
/* the last rtao pass: the pixels that cast, their rays (pixels * samples), the occluded ones, and the hipEvent times of classify + trace
 * and of the resolve / filter. All zero before the first pass. Waits for all work of the context. */
typedef struct UhRtaoStats {
   uint64_t pixels, rays, occluded;
   float trace_ms, filter_ms;
} UhRtaoStats;
UH_LAYOUT_ASSERT(sizeof(UhRtaoStats) == 32 && offsetof(UhRtaoStats, rays) == 8 && offsetof(UhRtaoStats, occluded) == 16 &&
                    offsetof(UhRtaoStats, trace_ms) == 24 && offsetof(UhRtaoStats, filter_ms) == 28,
                 "UhRtaoStats (32 B)");
int uh_rtao_default_params(UhRtaoParams* out); /* needs no GPU: 4, 1.0, 1.0, 2, 0.9, 0.05; UH_ERR_INVALID_ARGUMENT for NULL */
int uh_set_rtao_params(uh_ctx* ctx, const UhRtaoParams* params); /* validated here; a refused call leaves the old ones */
int uh_get_rtao_stats(uh_ctx* ctx, UhRtaoStats* out);            /* waits; all zero before the first pass */
/* measurement: the node visits and triangle tests of the last pass's walks, counted while option "count_visits" is 1 (the kernel is
 * then another instantiation, a little slower); 0 otherwise. Waits. */
int uh_get_rtao_visits(uh_ctx* ctx, uint64_t* nodes, uint64_t* triangles);

/* ---- motion vectors: where each G-buffer pixel's surface point was one motion pass ago ----------------------------------------------------
 * An EXTENSION: the reference's G-buffer has no velocity target. UH_HYBRID_MOTION (bit 14; bit 9 stays unused and ignored) is a modifier
 * of UH_HYBRID_GBUFFER, as UH_HYBRID_GBUFFER_RASTER is: without the G-buffer bit in the same call it is ignored. With it the G-buffer pass,
 * cast or rasterised, also writes UH_HYBRID_MOTION_IMAGE (RGBA32F, G-buffer orientation): xyz the PREVIOUS world position of the pixel's
 * surface point, w 1 where there is a correspondence and 0 where there is none. "Previous" is the previous uh_render_hybrid call that had
 * the bit: the context keeps, per mesh, the object-to-world 3x4 the tree was baked with then and (16 bytes per vertex) the object-space
 * positions then, both snapshotted on the stream behind each motion pass; only meshes whose vertices changed are copied again.
 *   state of a mesh at a pass   static    its transform is bit-identical to the snapshot's, its vertices not updated since
 *                               rigid     the transform differs, the vertices were not updated
 *                               deformed  uh_update_mesh_vertices since the snapshot (the transform may differ too)
 *                               none      not in the snapshot (added since), or uh_update_isosurface_mesh since
 *                               At the first pass ever every mesh is static.
 *   texel     not geometry (position w == 0): (0, 0, 0, 0). static: the position texel's xyz, the same bits, w 1. none: the position
 *             texel's xyz, w 0. rigid / deformed: o = (q0 b0 + q1 b1) + q2 b2 with b0 = 1 - u - v, b1 = u, b2 = v of the pixel's triangle
 *             as the G-buffer pass forms them, q the triangle's object-space corners - the previous ones when deformed, the current ones
 *             when rigid -, xyz = prev_o2w (o, 1), w 1.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first motion pass): UH_HYBRID_MOTION_IMAGE.
 * The denoiser follows the image with UH_DENOISE_MOTION (above). Per frame of a moving scene: the updates, view.rebuild_tlas = 1,
 * uh_render_frame, uh_render_hybrid(UH_HYBRID_GBUFFER | UH_HYBRID_MOTION), uh_denoise(UH_DENOISE_TEMPORAL | UH_DENOISE_MOTION); no reset.
 * RESOURCES: 16 bytes per pixel, 16 bytes per vertex of the meshes uh_update_mesh_vertices can deform (isosurface meshes hold no row: they
 * are never `deformed`), 64 bytes per mesh and 64 KiB of per-block counts, allocated by the first call with the bit; freed by
 * uh_destroy. A context that never sets the bit allocates nothing and runs no new code.
 * STREAM ORDER: as uh_render_hybrid. uh_get_motion_stats waits.
 * ISOLATION: the bit changes no other hybrid image, reservoir, accumulation, grid or UhStats; UhHybridStats is untouched. Without the bit
 * every pass is what it was. No uh_mgpu_ twin.
 * Arithmetic: DESIGN.md section 2, "Motion vectors". */
enum { UH_HYBRID_MOTION = 1u << 14 };
enum { UH_HYBRID_MOTION_IMAGE = 15 /* RGBA32F, G-buffer orientation: previous world position, w = 1 with a correspondence, else 0 */ };
/* the last motion pass: the geometry pixels with (w == 1) and without (w == 0) a correspondence, the meshes per state, and the hipEvent
 * times of the motion kernel and of the snapshot behind it. All zero before the first pass. Waits for all work of the context. */
typedef struct UhMotionStats {
   uint32_t pixels_with, pixels_without;
   uint32_t meshes_static, meshes_rigid, meshes_deformed, meshes_none;
   float motion_ms, snapshot_ms;
} UhMotionStats;
UH_LAYOUT_ASSERT(sizeof(UhMotionStats) == 32 && offsetof(UhMotionStats, pixels_without) == 4 && offsetof(UhMotionStats, meshes_static) == 8 &&
                    offsetof(UhMotionStats, meshes_rigid) == 12 && offsetof(UhMotionStats, meshes_deformed) == 16 &&
                    offsetof(UhMotionStats, meshes_none) == 20 && offsetof(UhMotionStats, motion_ms) == 24 && offsetof(UhMotionStats, snapshot_ms) == 28,
                 "UhMotionStats (32 B)");
int uh_get_motion_stats(uh_ctx* ctx, UhMotionStats* out); /* waits; all zero before the first pass */

/* ---- temporal anti-aliasing for the hybrid frame: a jittered camera resolved over time between the sky pass and present ------------------
 * An EXTENSION: the reference's only anti-aliasing is present's FXAA. UH_HYBRID_TAA (bit 15; bit 9 stays unused and ignored) adds a
 * temporal resolve to uh_render_hybrid AFTER the sky pass and BEFORE present: it reads deferred_output as that call's passes left it (or
 * as it stands when none of them ran in the call), the G-buffer's position image, view->prev_frame_projection_view and, with
 * UH_TAA_MOTION, the motion image, and writes taa_output (UH_HYBRID_TAA_OUTPUT, RGBA32F, G-buffer orientation as deferred_output) and the
 * history length N (UH_HYBRID_TAA_HISTORY, float32). Per pixel, with c its deferred_output texel:
 *   box       with UH_TAA_CLAMP: mean m1 and deviation sg per channel of deferred_output over the 3 x 3 pixels around it that lie in the
 *             frame; lo = m1 - clamp_gamma * sg, hi = m1 + clamp_gamma * sg.
 *   history   a geometry pixel (position w != 0) reprojects its position - with UH_TAA_MOTION the motion texel's xyz where that has
 *             w == 1, and nothing (no history) where it has w == 0 - as a point; every other pixel (the sky, the marching-cubes pass's
 *             pixels) reprojects the direction of its primary ray as a point at infinity. Through prev_frame_projection_view to a
 *             bilinear fetch of the previous taa_output and N, exactly as the denoiser's temporal stage forms it (8-bit fractions, the
 *             taps inside the image). There is NO mesh, normal or plane test.
 *   blend     with a history: hc = the fetched colour (clamped to [lo, hi] with UH_TAA_CLAMP), N' = min(N + 1, max_history), a =
 *             max(1 / N', alpha_min), out = hc + (c - hc) * a. Without: out = c, N' = 1. taa_output = (out.rgb, c.a).
 * When the pass ran in a call that also has UH_HYBRID_PRESENT, present reads taa_output instead of deferred_output (FXAA and the
 * conversion as ever); in every other call present is what it was. The first pass ever and the first after uh_reset_taa_history have no
 * history anywhere.
 * NON-FINITE INPUT: a pixel is BAD when a colour channel of its deferred_output texel is NaN, infinite or above 2^48 in magnitude (the
 * denoiser's bound and rule: DESIGN.md section 2, "Non-finite input"). A bad pixel passes through and takes part in nothing: its
 * taa_output is its input, bits unchanged; its N is 0, which no other pixel has (N' >= 1), so UH_HYBRID_TAA_HISTORY == 0 means "no
 * history here" and a later call's history tap on such a texel is skipped like a tap outside the frame; the boxes of its neighbours
 * leave it out of their mean and deviation; it counts in reset_pixels. Every other pixel of taa_output is finite, whatever the bad
 * ones hold, and stays so in the calls that follow.
 * JITTER IS THE CALLER'S: the library never jitters anything. Per frame k the caller offsets view->projection / inverse_projection by
 * uh_taa_jitter(k) pixels (for this perspective matrix elements 8 and 9 get -2 jx / W and +2 jy / H) and passes in
 * prev_frame_projection_view the previous frame's UN-jittered projection * view moved by the SAME offset in clip space (rows 0 and 1
 * less the offset times row 3): the pixel's sample lies j off its centre, and so does its reprojection, so a camera at rest reprojects
 * every pixel onto its own texel and the history stays registered to the un-jittered pixel grid. utopian::jitter_view of
 * utopian_host.hpp does all three to a view that holds the un-jittered matrices; the caller keeps the un-jittered product for the next
 * frame. (With the un-jittered product passed as it is the fetch lands j off the texel and every frame resamples the history: measured
 * on the slanted edge of tests/test_taa_cpu.py, 0.112 mean error against 0.035.) The bit counts as a final-frame pass: the final
 * frame's images are allocated by the first call with it.
 * LIMITS: nothing but the clamp rejects history - a disoccluded pixel keeps what the clamp lets through; the marching-cubes pass's
 * pixels are reprojected as if at infinity and ghost within the clamp box under camera translation; a camera cut is the caller's
 * uh_reset_taa_history.
 * PARAMS: uh_set_taa_params validates and keeps them for the calls that follow (a refused call leaves the old ones): unknown flag bits,
 * max_history < 1, alpha_min outside [0, 1] or clamp_gamma not finite and >= 0 are refused. Before the first call the defaults of
 * uh_taa_default_params hold: UH_TAA_CLAMP, 16, 0.1, 1.0.
 * UH_ERR_INVALID_ARGUMENT with a message, nothing runs and the history is untouched: no G-buffer rendered in this call or an earlier
 * one; UH_TAA_MOTION in the params while the last G-buffer pass had no UH_HYBRID_MOTION.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first pass): UH_HYBRID_TAA_OUTPUT, UH_HYBRID_TAA_HISTORY - the set the
 * last pass wrote.
 * RESOURCES: 40 bytes per pixel (two sets of RGBA32F colour and float N, ping-ponged) and 16 KiB of counters, allocated by the first call
 * with the bit; freed by uh_destroy. A context that never sets the bit allocates nothing and runs no new code.
 * STREAM ORDER: as uh_render_hybrid. uh_set_taa_params is host state, read by the next uh_render_hybrid; uh_reset_taa_history and
 * uh_get_taa_stats wait.
 * ISOLATION: the bit changes no other hybrid image, reservoir, accumulation, grid or UhStats, and not UhHybridFrameStats: its time goes
 * to UhTaaStats only. Without the bit every pass, image and stat is what it was. No uh_mgpu_ twin.
 * Arithmetic: DESIGN.md section 2, "Temporal anti-aliasing". */
enum { UH_HYBRID_TAA = 1u << 15 };
enum { UH_HYBRID_TAA_OUTPUT = 16 /* RGBA32F */, UH_HYBRID_TAA_HISTORY = 17 /* float32: N */ };
enum { UH_TAA_CLAMP = 1u << 0, UH_TAA_MOTION = 1u << 1 };
typedef struct UhTaaParams { uint32_t flags; uint32_t max_history; float alpha_min; float clamp_gamma; } UhTaaParams;   /* 16 B */
UH_LAYOUT_ASSERT(sizeof(UhTaaParams) == 16 && offsetof(UhTaaParams, max_history) == 4 && offsetof(UhTaaParams, alpha_min) == 8 &&
                    offsetof(UhTaaParams, clamp_gamma) == 12,
                 "UhTaaParams (16 B)");
/* the last pass: the pixels that blended a history and those that started one (their sum is the frame), and its hipEvent time */
typedef struct UhTaaStats  { uint32_t history_pixels, reset_pixels; float taa_ms; uint32_t reserved; } UhTaaStats;       /* 16 B */
UH_LAYOUT_ASSERT(sizeof(UhTaaStats) == 16 && offsetof(UhTaaStats, reset_pixels) == 4 && offsetof(UhTaaStats, taa_ms) == 8 &&
                    offsetof(UhTaaStats, reserved) == 12,
                 "UhTaaStats (16 B)");
int uh_taa_default_params(UhTaaParams* out);        /* needs no GPU: UH_TAA_CLAMP, 16, 0.1, 1.0 */
int uh_set_taa_params(uh_ctx*, const UhTaaParams*); /* validated here; a refused call leaves the old ones */
int uh_reset_taa_history(uh_ctx*);                  /* the next pass starts from no history (camera cut) */
int uh_get_taa_stats(uh_ctx*, UhTaaStats*);         /* waits; all zero before the first pass */
int uh_taa_jitter(uint32_t index, float out[2]);    /* needs no GPU: (halton(index+1, 2) - 0.5, halton(index+1, 3) - 0.5), in pixels */

/* ---- HDR display chain for the hybrid frame: exposure, bloom and tone mapping between the taa pass and present ---------------------------
 * An EXTENSION: the reference's present.frag converts the unbounded scene-linear frame straight to 8-bit sRGB (its Reinhard line,
 * present.frag:35-36, is commented out). UH_HYBRID_POST (bit 16; bit 9 stays unused and ignored) adds one pass to uh_render_hybrid AFTER
 * the taa pass (after the sky pass when that did not run in the call) and BEFORE present. Its source S is the taa_output this call wrote
 * when UH_HYBRID_TAA ran in it, else deferred_output as it stands. Three stages, max(a, b) = a > b ? a : b and min likewise throughout:
 *   meter     with UH_POST_AUTO_EXPOSURE: a histogram of L = 0.299 r + 0.587 g + 0.114 b over 256 bins, bin = clamp((bits(L) >> 20) - 888,
 *             0, 255) - eight bins per octave from 2^-16 up; L <= 0 and bad pixels go to bin 0, which is not metered. Of the n metered
 *             samples those ranked [(uint64)(low_percentile n), (uint64)(high_percentile n)) in bin order are kept (all when that range
 *             is empty); Lavg = the float with bits (888 << 20) + ((sum kept_b b) << 20) / (sum kept_b) + (1 << 19), E_target =
 *             min(max(key / Lavg, min_exposure), max_exposure), E = E_prev + (E_target - E_prev) adaptation - or E_target on the first
 *             pass and the first after uh_reset_post_exposure. Nothing metered: E = E_prev (manual_exposure without one). Without the
 *             flag: E = manual_exposure and no histogram. E stays on the device; every pass leaves an E_prev to the next.
 *   bloom     with UH_POST_BLOOM: level k is (ceil(w / 2), ceil(h / 2)) of level k - 1 for k = 1..bloom_levels while level k - 1 is
 *             larger than 1 x 1. Level 1 filters the prefiltered frame (0 for a bad pixel; c = S.rgb E, m = its largest channel: 0
 *             unless m > bloom_threshold, else c ((m - bloom_threshold) / m)), deeper levels the level above: 4 x 4 taps (1, 3, 3, 1) / 8
 *             per axis at source 2X - 1 .. 2X + 2, clamped. Up: U(img) takes the two nearest texels per axis at 0.75 and 0.25, clamped;
 *             up[last] = down[last], up[k] = (down[k] + U(up[k + 1])) 0.5. Bloom images are RGBA32F with alpha 0.
 *   composite x = S.rgb E + bloom_intensity U(up[1]) (no second term without the flag or without a level), then the operator:
 *             UH_TONEMAP_NONE y = x; UH_TONEMAP_REINHARD xc = min(max(x, 0), 2^20), y = xc / (xc + 1); UH_TONEMAP_ACES a = xc (2.51 xc +
 *             0.03), b = xc (2.43 xc + 0.59) + 0.14, y = min(max(a / b, 0), 1). post_output = (y, S.a), RGBA32F, oriented as S.
 * When the pass ran in a call that also has UH_HYBRID_PRESENT, present reads post_output (FXAA and linearToSrgb as ever, now on display-range
 * values); in every other call present is what it was. The bit counts as a final-frame pass: the final frame's images are allocated by
 * the first call with it. It adds no refusal to uh_render_hybrid.
 * NON-FINITE INPUT: a pixel is BAD by TAA's rule (a channel NaN, infinite or above 2^48 in magnitude). Its post_output texel is its S
 * texel, bits unchanged; it is not metered and contributes 0 to bloom. Every other post_output texel is finite.
 * uh_post_image runs the same three stages on a caller's W x H RGBA32F host image (the context's frame size) with the same params and
 * exposure state, writes post_output and runs no present: for a path-traced or denoised frame. It needs no scene.
 * PARAMS: uh_set_post_params validates and keeps them for the passes that follow (a refused call leaves the old ones): unknown flag
 * bits; tonemap > 2; bloom_levels outside 1..8; manual_exposure, key, min_exposure or max_exposure not finite or outside (0, 65536], or
 * min_exposure > max_exposure; adaptation outside (0, 1]; percentiles that are not 0 <= low < high <= 1; bloom_threshold or
 * bloom_intensity not finite, < 0 or > 65536. Before the first call the defaults of uh_post_default_params hold: both flags, ACES, 6
 * levels, manual_exposure 1, key 0.18, exposure in [1 / 64, 64], adaptation 0.1, percentiles 0.5 and 0.95, threshold 1, intensity 0.04.
 * READ-BACK is uh_read_post (uh_read_hybrid keeps its images 0..17): UH_POST_OUTPUT (level 0), UH_POST_BLOOM_DOWN and UH_POST_BLOOM_UP
 * (level 1..UhPostStats::levels, W x H as uh_post_level_size gives them), UH_POST_HISTOGRAM (level 0, 256 uint32). UH_ERR_INVALID_ARGUMENT
 * before the first pass, for a level the last pass did not build, and for the histogram when the last pass did not meter.
 * RESOURCES: 16 bytes per pixel of post_output, about 11 more of pyramid (two images per level that exists, up to 8 levels), 2 KiB of
 * counts and a 32-byte record, allocated by the first pass; uh_post_image's upload another 16 bytes per pixel at its first call; freed by
 * uh_destroy. A context that never sets the bit allocates nothing and runs no new code.
 * STREAM ORDER: the pass as uh_render_hybrid. uh_post_image, uh_read_post and uh_get_post_stats wait and are complete on return.
 * uh_set_post_params and uh_reset_post_exposure are host state, read by the next pass.
 * ISOLATION: the bit changes no other hybrid image but present_output, no reservoir, accumulation, grid or UhStats, and not
 * UhHybridFrameStats: its time goes to UhPostStats only. Without the bit every pass, image and stat is what it was. No uh_mgpu_ twin.
 * LIMITS: no firefly suppression in the prefilter (one bright texel blooms); no lens effects or grading; the display output stays the
 * 8-bit sRGB of present; uh_denoise and uh_render_forward reach the chain through uh_post_image and the host.
 * Arithmetic: DESIGN.md section 2, "HDR display chain". */
enum { UH_HYBRID_POST = 1u << 16 };
enum { UH_POST_AUTO_EXPOSURE = 1u << 0, UH_POST_BLOOM = 1u << 1 };
enum { UH_TONEMAP_NONE = 0, UH_TONEMAP_REINHARD = 1, UH_TONEMAP_ACES = 2 };
enum { UH_POST_OUTPUT = 0 /* RGBA32F */, UH_POST_BLOOM_DOWN = 1, UH_POST_BLOOM_UP = 2 /* RGBA32F, level 1.. */, UH_POST_HISTOGRAM = 3 /* 256 x uint32 */ };
typedef struct UhPostParams {
   uint32_t flags, tonemap, bloom_levels;
   float manual_exposure, key, min_exposure, max_exposure, adaptation, low_percentile, high_percentile, bloom_threshold, bloom_intensity;
} UhPostParams;   /* 48 B */
UH_LAYOUT_ASSERT(sizeof(UhPostParams) == 48 && offsetof(UhPostParams, tonemap) == 4 && offsetof(UhPostParams, bloom_levels) == 8 &&
                    offsetof(UhPostParams, manual_exposure) == 12 && offsetof(UhPostParams, key) == 16 && offsetof(UhPostParams, min_exposure) == 20 &&
                    offsetof(UhPostParams, max_exposure) == 24 && offsetof(UhPostParams, adaptation) == 28 &&
                    offsetof(UhPostParams, low_percentile) == 32 && offsetof(UhPostParams, high_percentile) == 36 &&
                    offsetof(UhPostParams, bloom_threshold) == 40 && offsetof(UhPostParams, bloom_intensity) == 44,
                 "UhPostParams (48 B)");
/* the last pass: its exposure E, E_target (E where nothing was metered) and Lavg (0 where nothing was), the pixels in bins 1..255 (0
 * without UH_POST_AUTO_EXPOSURE), the bad pixels, the bloom levels built, the hipEvent times of the three stages, the passes so far */
typedef struct UhPostStats {
   float exposure, target_exposure, average_luminance;
   uint32_t metered_pixels, bad_pixels, levels;
   float meter_ms, bloom_ms, tonemap_ms;
   uint32_t renders, reserved[2];
} UhPostStats;    /* 48 B */
UH_LAYOUT_ASSERT(sizeof(UhPostStats) == 48 && offsetof(UhPostStats, target_exposure) == 4 && offsetof(UhPostStats, average_luminance) == 8 &&
                    offsetof(UhPostStats, metered_pixels) == 12 && offsetof(UhPostStats, bad_pixels) == 16 && offsetof(UhPostStats, levels) == 20 &&
                    offsetof(UhPostStats, meter_ms) == 24 && offsetof(UhPostStats, bloom_ms) == 28 && offsetof(UhPostStats, tonemap_ms) == 32 &&
                    offsetof(UhPostStats, renders) == 36 && offsetof(UhPostStats, reserved) == 40,
                 "UhPostStats (48 B)");
int uh_post_default_params(UhPostParams* out);          /* needs no GPU */
int uh_set_post_params(uh_ctx*, const UhPostParams*);   /* validated here; a refused call leaves the old ones */
int uh_reset_post_exposure(uh_ctx*);                    /* the next pass snaps to its target (camera cut) */
int uh_get_post_stats(uh_ctx*, UhPostStats*);           /* waits; all zero before the first pass */
int uh_post_image(uh_ctx*, const float* rgba32f);       /* W*H*4 floats on the host; the three stages into post_output; waits */
int uh_read_post(uh_ctx*, int which, int level, void* out);   /* waits */
/* needs no GPU: the size of bloom level `level` (0: the frame) of a W x H frame; UH_ERR_INVALID_ARGUMENT for one that does not exist */
int uh_post_level_size(uint32_t W, uint32_t H, uint32_t level, uint32_t* w, uint32_t* h);

/* ---- one-bounce ray-traced diffuse GI for the hybrid frame: the light that arrives by way of another surface ---------------------------
 * An EXTENSION: the reference has no GI at all; the hybrid frame's whole indirect term is deferred.frag's 0.03 * diffuse * occlusion (or
 * the IBL lookup), which knows nothing of the scene's own geometry. UH_HYBRID_RTGI (bit 17; bit 9 stays unused and ignored) adds one pass
 * to uh_render_hybrid directly AFTER the deferred pass and BEFORE the marching-cubes, sky, taa and post passes, so TAA - which integrates
 * the per-frame ray noise over time - and the display chain see it. UH_HYBRID_FRAME | UH_HYBRID_RTGI is the natural call. The deferred
 * pass itself is untouched and the reference's 0.03 ambient STAYS in it: this pass adds to deferred_output, it replaces nothing.
 *   rays      RTAO's rule says which pixels cast: position texel w != 0 and a normal texel N that normalises to a finite Nn. Such a pixel
 *             (px, py) casts `samples` rays from offsetRay(P, Nn) of its OWN texels. Ray s has direction normalize(Nn + normalize(u)), u =
 *             randomPointInUnitSphere of the state initRNG(px, py, W, (frameNumber(view) * 64 + s) ^ 0x52544749) - the XOR keeps the rays
 *             from being RTAO's own; Nn itself where |Nn + normalize(u)|^2 is not >= 1e-12. tmin 0.001, tmax 10000, closest hit.
 *   radiance  L of a ray. A miss: IntegrateScattering(o, d, 999999999, sun) as rt_reflections.rmiss forms it, unclamped; (1, 1, 1) under
 *             option "furnace". A hit on material type 3: the emission the path tracer's closest-hit shader gives it, (1, 1, 1)
 *             (reference.rchit:85-89); no sun ray. Any other hit: albedo = texture(diffuse_map, uv) * base_color (rchit:41-42), Nh the
 *             hit's world normal turned toward the ray (rchit:32-37), X = o + t d, NdotL = max(dot(Nh, sun), 0). NdotL == 0 (or NaN):
 *             the hit is DARK, L = 0, no sun ray. Otherwise one any-hit ray from offsetRay(X, Nh) toward sun (0.001, 10000): occluded
 *             DARK, L = 0; else SUNLIT, L = ((albedo / PI) * rad_sun) * NdotL with PI of brdf.glsl and rad_sun the radiance of the
 *             deferred pass's light record 0 (the sun: colour (1, 1, 1), attenuation 1). Under "furnace" a non-emitter hit is dark and
 *             casts no sun ray. Then per channel L = min(L > 0 ? L : 0, max_radiance): a NaN is 0, L is always finite.
 *   pixel     E = (L_0 + L_1 + ... + L_{samples-1}) / (float)samples, summed in sample order: it does not depend on the schedule.
 *   filter    blur_radius 0: Ef = E. r > 0: the mean of E over the taps (dx, dy) in [-r, r]^2 (dy outer) that lie in the frame, cast
 *             themselves and pass dot(Nn_tap, Nn) >= blur_normal_cos and |dot(P_tap - P, Nn)| <= blur_plane; the centre always counts.
 *   composite for every pixel that cast, with base = pow(albedo, 2.2) * base_color and metallic = pbr.r * material.metallic as
 *             deferred.frag:52-65 forms them: add = ((base * (1 - metallic)) * Ef) * intensity, times the occlusion pbr.b, times (with
 *             view->ssao_enabled == 1) the pixel's ssao_output texel / 65535; deferred_output.rgb += add, alpha untouched. A pixel whose
 *             material is metal (type 1) with raytracing_supported == 1 is left as it is: the deferred pass replaced its colour with the
 *             reflection. The shadow factor is NOT applied: indirect light is not sun-shadowed.
 * PARAMS: uh_set_rtgi_params validates and keeps them for the calls that follow (a refused call leaves the old ones); before the
 * first call the defaults of uh_rtgi_default_params hold: 2 samples, blur_radius 3, max_radiance 16.0, intensity 1.0, 0.9, 0.05.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, in this order after the rules above: the bit and
 * view->raytracing_supported != 1; no G-buffer rendered in this call or an earlier one; the bit and view->ibl_enabled == 1 (the IBL
 * ambient term and this pass would both count the sky); the bit without UH_HYBRID_DEFERRED in the same call (the pass has nothing to add
 * to). UH_ERR_CAPACITY for a frame of 2^28 pixels or more (its rays are numbered in 32 bits). UH_ERR_NOT_BUILT before
 * uh_build_acceleration, as without the bit.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first rtgi pass; both in G-buffer orientation): UH_HYBRID_GI_RADIANCE,
 * RGBA32F: Ef, w = 1 where the pixel cast, (0, 0, 0, 0) elsewhere. UH_HYBRID_GI_COUNTS, 4 bytes per pixel: the rays that hit a sunlit
 * surface, a dark one, an emitter, and those that missed; they sum to `samples` where the pixel cast and are all 0 elsewhere.
 * RESOURCES: 40 bytes per pixel (counts, radiance, the unfiltered means, the queue of the pixels that cast) and 32 bytes per ray (its
 * radiance and its sun-ray record) at the largest `samples` a pass has run with, allocated by the first pass; freed by uh_destroy. A
 * context that never sets the bit allocates nothing for it.
 * STREAM ORDER: as uh_render_hybrid. uh_set_rtgi_params is host state, read by the next uh_render_hybrid; uh_get_rtgi_stats waits.
 * ISOLATION: the bit changes no reservoir, accumulation, gbuffer_position, grid, UhStats or RTAO state, and no hybrid image but
 * deferred_output (and what later passes of the call make of it) and its own two; its rays are counted in UhRtgiStats only, and
 * UhHybridFrameStats keeps its layout and its times. Without the bit every pass, image, statistic and allocation is what it was.
 * No uh_mgpu_ twin.
 * OUT OF SCOPE: point, spot and reservoir lights at the hit; more than one bounce; specular GI (a pass of its own: UH_HYBRID_GLOSSY,
 * below); a history of its own (UH_HYBRID_TAA serves); the forward graph.
 * Arithmetic: DESIGN.md section 2, "Ray-traced diffuse GI". */
enum { UH_HYBRID_RTGI = 1u << 17 };
enum { UH_HYBRID_GI_RADIANCE = 18 /* RGBA32F: Ef, w = 1 where the pixel cast */, UH_HYBRID_GI_COUNTS = 19 /* 4 x uint8: sunlit, dark, emitter, missed */ };
typedef struct UhRtgiParams {
   uint32_t samples;      /* rays per pixel that casts, 1..16 */
   uint32_t blur_radius;  /* 0 = no filter; else 1..6: taps dx, dy in [-r, r] */
   float max_radiance;    /* the cap of a ray's L per channel; finite, > 0 */
   float intensity;       /* scales what the composite adds; finite, >= 0 */
   float blur_normal_cos; /* a tap counts when dot(Nn_tap, Nn) >= this; not NaN */
   float blur_plane;      /* and |dot(P_tap - P, Nn)| <= this (world units); not NaN */
} UhRtgiParams;
UH_LAYOUT_ASSERT(sizeof(UhRtgiParams) == 24 && offsetof(UhRtgiParams, blur_radius) == 4 && offsetof(UhRtgiParams, max_radiance) == 8 &&
                    offsetof(UhRtgiParams, intensity) == 12 && offsetof(UhRtgiParams, blur_normal_cos) == 16 &&
                    offsetof(UhRtgiParams, blur_plane) == 20,
                 "UhRtgiParams (24 B)");
/* the last rtgi pass: the pixels that cast, their rays (pixels * samples), the sun rays cast from the hits and the rays that missed, and
 * the hipEvent times of classify + closest-hit walk, of the sun rays' any-hit walk, of the mean + filter and of the composite. All zero
 * before the first pass. Waits for all work of the context. */
typedef struct UhRtgiStats {
   uint64_t pixels, rays, shadow_rays, misses;
   float trace_ms, shadow_ms, filter_ms, composite_ms;
} UhRtgiStats;
UH_LAYOUT_ASSERT(sizeof(UhRtgiStats) == 48 && offsetof(UhRtgiStats, rays) == 8 && offsetof(UhRtgiStats, shadow_rays) == 16 &&
                    offsetof(UhRtgiStats, misses) == 24 && offsetof(UhRtgiStats, trace_ms) == 32 && offsetof(UhRtgiStats, shadow_ms) == 36 &&
                    offsetof(UhRtgiStats, filter_ms) == 40 && offsetof(UhRtgiStats, composite_ms) == 44,
                 "UhRtgiStats (48 B)");
int uh_rtgi_default_params(UhRtgiParams* out); /* needs no GPU: 2, 3, 16.0, 1.0, 0.9, 0.05; UH_ERR_INVALID_ARGUMENT for NULL */
int uh_set_rtgi_params(uh_ctx* ctx, const UhRtgiParams* params); /* validated here; a refused call leaves the old ones */
int uh_get_rtgi_stats(uh_ctx* ctx, UhRtgiStats* out);            /* waits; all zero before the first pass */

/* ---- ray-traced glossy reflections for the hybrid frame: the specular half of the indirect light ---------------------------------------
 * An EXTENSION: the reference's only reflection of the scene is rt_reflections' perfect mirror on material type 1. UH_HYBRID_GLOSSY
 * (bit 18) adds one pass to uh_render_hybrid directly AFTER the rtgi pass (after the deferred pass when that bit is clear) and BEFORE the
 * marching-cubes, sky, taa and post passes. It adds roughness-aware specular reflection of the scene's own geometry to deferred_output;
 * the deferred pass and rt_reflections are untouched. UH_HYBRID_FRAME | UH_HYBRID_RTGI | UH_HYBRID_GLOSSY is the natural call.
 *   pixels    RTGI's rule first: position texel w != 0 and Nn = normalize(N) finite. Then the material record as deferred.frag forms it
 *             (index uint(pbr.a); out of range: factors 1, type 0). The pixel casts when it is not (raytracing_supported == 1 and type 1:
 *             it holds its mirror), r = pbr.g * roughness_factor has r >= 0 && r <= max_roughness (a NaN fails), V = normalize(eye - P)
 *             is finite and NoV = dot(Nn, V) > 0.
 *   rays      `samples` per pixel that casts. alpha = r r, a2 = alpha alpha. T, B from Nn by the branch-free frame of Duff et al. 2017.
 *             The half vector Hw is drawn from the GGX distribution of visible normals (Heitz 2018) with randomPointInUnitDisk of the
 *             state initRNG(px, py, W, (frameNumber(view) * 64 + s) ^ 0x474C4F53); d = normalize((2 dot(V, Hw)) Hw - V). A sample whose
 *             NoL = dot(Nn, d) is not > 0 is BELOW: no ray, an all-zero record, counted dark. Else a closest-hit ray from
 *             offsetRay(P, Nn), tmin 0.001, tmax 10000.
 *   radiance  L of a cast ray is UH_HYBRID_RTGI's (sky unclamped with exact heights, (1, 1, 1) for type 3 and under "furnace" for a miss,
 *             shadowed-sun-lit Lambert or dark elsewhere), clamped per channel with this pass's max_radiance.
 *   weight    the unbiased visible-normal estimator, height-correlated Smith term, Fresnel split off: sv = sqrt((NoV NoV)(1 - a2) + a2),
 *             sl likewise of NoL, Gw = (NoL (NoV + sv)) / (NoL sv + NoV sl); x = 1 - dot(V, Hw), x5 = ((x x)(x x)) x. The ray's record
 *             is (Gw L, x5).
 *   pixel     S = (sum R_s (1 - x5_s)) / samples and Bi = (sum R_s x5_s) / samples, in sample order from the s = 0 term.
 *   filter    per pixel radius re = (int)(min(r / blur_roughness, 1) * blur_radius); re == 0: Sf = S, Bf = Bi. Else the mean over the
 *             taps (dx, dy) in [-re, re]^2, dy outer: the centre, and every tap in the frame that cast, has max(|dx|, |dy|) <= its own
 *             re, dot(Nn_tap, Nn) >= blur_normal_cos and |dot(P_tap - P, Nn)| <= blur_plane.
 *   composite for every pixel that cast, base, metallic and occlusion as deferred.frag:52-65 forms them: F0 = 0.04 (1 - metallic) +
 *             base metallic; add = ((F0 Sf + Bf) intensity) occlusion, times (view->ssao_enabled == 1) the ssao texel / 65535;
 *             deferred_output.rgb += add, alpha untouched, no shadow factor.
 * PARAMS: uh_set_glossy_params validates and keeps them (a refused call leaves the old ones); the defaults of uh_glossy_default_params:
 * 1 sample, blur_radius 3, max_roughness 0.6, max_radiance 16.0, intensity 1.0, blur_roughness 0.5, 0.95, 0.05.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, in this order after every rule above (UH_HYBRID_RTGI's included): the bit
 * and view->raytracing_supported != 1; no G-buffer rendered in this call or an earlier one; the bit and view->ibl_enabled == 1 (the IBL
 * specular term and this pass would both count the sky); the bit without UH_HYBRID_DEFERRED in the same call. UH_ERR_CAPACITY for a
 * frame of 2^28 pixels or more. UH_ERR_NOT_BUILT before uh_build_acceleration, as without the bit.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first glossy pass; all three in G-buffer orientation):
 * UH_HYBRID_GLOSSY_SCALE and UH_HYBRID_GLOSSY_BIAS, RGBA32F: Sf and Bf, w = 1 where the pixel cast, (0, 0, 0, 0) elsewhere.
 * UH_HYBRID_GLOSSY_COUNTS, 4 bytes per pixel: sunlit, dark (below samples among them), emitter, missed; they sum to `samples` where the
 * pixel cast and are 0 elsewhere.
 * RESOURCES: 73 bytes per pixel (counts, the two images, the two unfiltered means, the pixel queue, the radius byte) and 68 bytes per ray
 * (its hit record, which becomes its radiance record, its origin and direction, its sun-ray record, its queue word) at the largest
 * `samples` a pass has run with, allocated by the first pass; freed by uh_destroy. A context that never sets the bit allocates nothing.
 * STREAM ORDER: as uh_render_hybrid. uh_set_glossy_params is host state, read by the next uh_render_hybrid; uh_get_glossy_stats waits.
 * ISOLATION: the bit changes no reservoir, accumulation, gbuffer_position, grid, UhStats, RTAO or RTGI state, and no hybrid image but
 * deferred_output (and what later passes of the call make of it) and its own three. Without the bit every pass, image, statistic and
 * allocation is what it was.
 * No uh_mgpu_ twin.
 * OUT OF SCOPE: replacing rt_reflections or lighting metal pixels; point, spot and reservoir lights at the hit; a second bounce; a
 * history of its own (UH_HYBRID_TAA serves); the forward graph; moving UH_HYBRID_RTGI onto this pass's kernels.
 * Arithmetic: DESIGN.md section 2, "Ray-traced glossy reflections". */
enum { UH_HYBRID_GLOSSY = 1u << 18 };
enum { UH_HYBRID_GLOSSY_SCALE = 20 /* RGBA32F: Sf, w = 1 where the pixel cast */, UH_HYBRID_GLOSSY_BIAS = 21 /* RGBA32F: Bf, w likewise */,
       UH_HYBRID_GLOSSY_COUNTS = 22 /* 4 x uint8: sunlit, dark, emitter, missed */ };
typedef struct UhGlossyParams {
   uint32_t samples;      /* rays per pixel that casts, 1..16 */
   uint32_t blur_radius;  /* the filter's largest radius, 0..6; 0 = no filter */
   float max_roughness;   /* a pixel casts when 0 <= pbr.g * roughness_factor <= this; finite, >= 0 */
   float max_radiance;    /* the cap of a ray's L per channel; finite, > 0 */
   float intensity;       /* scales what the composite adds; finite, >= 0 */
   float blur_roughness;  /* the roughness at which a pixel's radius reaches blur_radius; finite, > 0 */
   float blur_normal_cos; /* a tap counts when dot(Nn_tap, Nn) >= this; not NaN */
   float blur_plane;      /* and |dot(P_tap - P, Nn)| <= this (world units); not NaN */
} UhGlossyParams;
UH_LAYOUT_ASSERT(sizeof(UhGlossyParams) == 32 && offsetof(UhGlossyParams, blur_radius) == 4 && offsetof(UhGlossyParams, max_roughness) == 8 &&
                    offsetof(UhGlossyParams, max_radiance) == 12 && offsetof(UhGlossyParams, intensity) == 16 &&
                    offsetof(UhGlossyParams, blur_roughness) == 20 && offsetof(UhGlossyParams, blur_normal_cos) == 24 &&
                    offsetof(UhGlossyParams, blur_plane) == 28,
                 "UhGlossyParams (32 B)");
/* the last glossy pass: the pixels that cast, the rays cast and the below samples (rays + below == pixels * samples), the sun rays cast
 * from the hits, the rays that missed, and the hipEvent times of classify + ray generation + closest-hit walk, of the hit shading, of
 * the sun rays' any-hit walk, of the mean + filter and of the composite. All zero before the first pass. Waits. */
typedef struct UhGlossyStats {
   uint64_t pixels, rays, below, shadow_rays, misses;
   float trace_ms, shade_ms, shadow_ms, filter_ms, composite_ms; /* then 4 bytes of tail padding */
} UhGlossyStats;
UH_LAYOUT_ASSERT(sizeof(UhGlossyStats) == 64 && offsetof(UhGlossyStats, rays) == 8 && offsetof(UhGlossyStats, below) == 16 &&
                    offsetof(UhGlossyStats, shadow_rays) == 24 && offsetof(UhGlossyStats, misses) == 32 &&
                    offsetof(UhGlossyStats, trace_ms) == 40 && offsetof(UhGlossyStats, shade_ms) == 44 &&
                    offsetof(UhGlossyStats, shadow_ms) == 48 && offsetof(UhGlossyStats, filter_ms) == 52 &&
                    offsetof(UhGlossyStats, composite_ms) == 56,
                 "UhGlossyStats (64 B)");
int uh_glossy_default_params(UhGlossyParams* out); /* needs no GPU: 1, 3, 0.6, 16.0, 1.0, 0.5, 0.95, 0.05; UH_ERR_INVALID_ARGUMENT for NULL */
int uh_set_glossy_params(uh_ctx* ctx, const UhGlossyParams* params); /* validated here; a refused call leaves the old ones */
int uh_get_glossy_stats(uh_ctx* ctx, UhGlossyStats* out);            /* waits; all zero before the first pass */

/* ---- volumetric fog for the hybrid frame: a homogeneous medium with ray-traced sun shafts --------------------------------------------
 * An EXTENSION: the reference has no participating medium. UH_HYBRID_FOG (bit 19) adds one pass to uh_render_hybrid directly AFTER the
 * sky pass and BEFORE the taa, post and present passes, so the taa pass integrates the march jitter and the display chain sees the
 * fogged frame. UH_HYBRID_FRAME | UH_HYBRID_FOG is the natural call. Everything float32 in the order written, nothing fused.
 *   ray       (o, d) = the sky pass's view ray through the pixel centre. Geometry pixel (position texel w != 0): V = P - o, D0 =
 *             sqrt(dot(V, V)); it marches when D0 is finite and > 0, with dir = V / D0 and D = min(D0, max_distance); one that does not
 *             is left exactly as it is, its mask 0 and its terms 0. Sky pixel (w == 0): dir = d, D = max_distance; it always marches.
 *   samples   dt = D / (float)steps; xi = randomFloat of the state initRNG(px, py, W, (frameNumber(view) * 64) ^ 0x464F4721): one jitter
 *             per pixel per frame. Sample k is X_k = o + dir * (((float)k + xi) * dt); its ray is an any-hit ray from X_k toward the sun,
 *             tmin 0.001, tmax 10000, no offsetRay (there is no surface). Bit k of the pixel's mask is set when the ray is not occluded.
 *   resolve   a = expf(-(density * dt)); p = 1, sum = 0; for k = 0 .. steps - 1: if bit k: sum += p; then p = p * a. Ttot = p and
 *             F = (1 - a) * sum: the fraction of the sun's scattered light that survives to the eye.
 *   filter    blur_radius r == 0: Ff = F. Else the mean of F (float32 sum in tap order over the float tap count) over the taps (dx, dy)
 *             in [-r, r]^2, dy outer: the centre, and every tap in the frame that marched with |D_tap - D| <= blur_depth * D.
 *   phase     c = dot(sun, dir), g = anisotropy, q = (1 + g g) - (2 g) c, ph = (1 - g g) / ((4 PI) * (q * sqrt(q))), PI of brdf.glsl.
 *   composite for every pixel that marched: C = deferred_output.rgb, S = ((albedo * rad_sun) * ph) * intensity with the sun radiance
 *             UH_HYBRID_RTGI takes from the deferred pass's light record 0; out = (C * Ttot + S * Ff) + ambient * (1 - Ttot); alpha
 *             untouched. Option "furnace" does not change this pass.
 * PARAMS: uh_set_fog_params validates and keeps them (a refused call leaves the old ones); the defaults of uh_fog_default_params:
 * 16 steps, blur_radius 2, density 0.02, max_distance 200.0, anisotropy 0.6, intensity 1.0, blur_depth 0.1, albedo (1, 1, 1), ambient
 * (0.05, 0.06, 0.08).
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, in this order after every rule above (UH_HYBRID_GLOSSY's included): the bit
 * and view->raytracing_supported != 1; no G-buffer rendered in this call or an earlier one; the bit without both UH_HYBRID_DEFERRED and
 * UH_HYBRID_SKY in the same call; the bit together with UH_HYBRID_MARCHING_CUBES in the same call. UH_ERR_CAPACITY for a frame of 2^26
 * pixels or more (items are numbered in 32 bits at up to 32 per pixel). UH_ERR_NOT_BUILT before uh_build_acceleration, as without the bit.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first fog pass; both in G-buffer orientation): UH_HYBRID_FOG_MASK, one
 * uint32 per pixel; UH_HYBRID_FOG_TERMS, RGBA32F (a, Ttot, F, Ff), all 0 where the pixel did not march.
 * RESOURCES: 28 bytes per pixel (the mask, the terms, the march length, the pixel queue), allocated by the first pass; freed by
 * uh_destroy. A context that never sets the bit allocates nothing.
 * STREAM ORDER: as uh_render_hybrid. uh_set_fog_params is host state, read by the next uh_render_hybrid; uh_get_fog_stats waits.
 * OPTIONS: "fog_order" 0..2 (default 2) lays the trace kernel's work out (same masks whichever; DESIGN.md section 4 "Volumetric fog"); with
 * "count_visits" the walks' node visits and triangle tests go to the pass's own counters (uh_get_fog_visits), never to UhStats.
 * ISOLATION: the bit changes no reservoir, accumulation, grid, UhStats, RTAO, RTGI, GLOSSY, TAA-history or post state beyond what those
 * passes make of a fogged deferred_output, and no hybrid image but deferred_output and its own two. Without the bit every pass, image,
 * statistic and allocation is what it was.
 * No uh_mgpu_ twin.
 * OUT OF SCOPE: height-dependent or heterogeneous density; point, spot and reservoir lights in the medium; multiple scattering; fog in
 * rt_reflections, RTGI or GLOSSY rays, or in uh_render_forward; the marching-cubes pass's pixels (hence the refusal); answering these
 * rays from the path tracer's sun grid (its reach rule is stated for surface points: a follow-up with its own proof); a uh_mgpu_ twin;
 * a history of its own (UH_HYBRID_TAA serves).
 * Arithmetic: DESIGN.md section 2, "Volumetric fog". */
enum { UH_HYBRID_FOG = 1u << 19 };
enum { UH_HYBRID_FOG_MASK = 23 /* uint32 per pixel, G-buffer orientation: bit k = sample k saw the sun */,
       UH_HYBRID_FOG_TERMS = 24 /* RGBA32F, G-buffer orientation: (a, Ttot, F, Ff), all 0 where the pixel did not march */ };
typedef struct UhFogParams {
   uint32_t steps;        /* samples along a pixel's view ray, 1..32 */
   uint32_t blur_radius;  /* 0 = no filter; else 1..4: taps dx, dy in [-r, r] */
   float density;         /* extinction per world unit; finite, >= 0 */
   float max_distance;    /* march length of a sky pixel and the cap of a geometry pixel's; finite, > 0 */
   float anisotropy;      /* Henyey-Greenstein g; -0.95..0.95, not NaN */
   float intensity;       /* scales the sun's in-scattering; finite, >= 0 */
   float blur_depth;      /* a tap counts when |D_tap - D| <= blur_depth * D; finite, >= 0 */
   uint32_t reserved;     /* must be 0 */
   float albedo[3];       /* single-scattering albedo per channel; each finite, 0..1 */
   float ambient[3];      /* unshadowed fog radiance (sky light in the medium); each finite, >= 0 */
} UhFogParams;
UH_LAYOUT_ASSERT(sizeof(UhFogParams) == 56 && offsetof(UhFogParams, blur_radius) == 4 && offsetof(UhFogParams, density) == 8 &&
                    offsetof(UhFogParams, max_distance) == 12 && offsetof(UhFogParams, anisotropy) == 16 &&
                    offsetof(UhFogParams, intensity) == 20 && offsetof(UhFogParams, blur_depth) == 24 &&
                    offsetof(UhFogParams, reserved) == 28 && offsetof(UhFogParams, albedo) == 32 && offsetof(UhFogParams, ambient) == 44,
                 "UhFogParams (56 B)");
/* the last fog pass: the pixels that marched, their rays (pixels * steps), the rays that reached the sun, and the hipEvent times of
 * classify + walk, of resolve + filter and of the composite. All zero before the first pass. Waits. */
typedef struct UhFogStats {
   uint64_t pixels, rays, lit;
   float trace_ms, filter_ms, composite_ms;
   uint32_t reserved;
} UhFogStats;
UH_LAYOUT_ASSERT(sizeof(UhFogStats) == 40 && offsetof(UhFogStats, rays) == 8 && offsetof(UhFogStats, lit) == 16 &&
                    offsetof(UhFogStats, trace_ms) == 24 && offsetof(UhFogStats, filter_ms) == 28 &&
                    offsetof(UhFogStats, composite_ms) == 32 && offsetof(UhFogStats, reserved) == 36,
                 "UhFogStats (40 B)");
int uh_fog_default_params(UhFogParams* out); /* needs no GPU: 16, 2, 0.02, 200.0, 0.6, 1.0, 0.1, 0, (1, 1, 1), (0.05, 0.06, 0.08); UH_ERR_INVALID_ARGUMENT for NULL */
int uh_set_fog_params(uh_ctx* ctx, const UhFogParams* params); /* validated here; a refused call leaves the old ones */
int uh_get_fog_stats(uh_ctx* ctx, UhFogStats* out);            /* waits; all zero before the first pass */
/* the last fog pass's node visits and triangle tests, counted while option "count_visits" is 1; else 0, 0. Waits. */
int uh_get_fog_visits(uh_ctx* ctx, uint64_t* nodes, uint64_t* triangles);

/* ---- ray-traced glass for the hybrid frame: dielectric pixels show what lies behind and before them -----------------------------------
 * The reference's path tracer renders material type 2 (dielectric) as glass; its hybrid frame shades it as an opaque Cook-Torrance solid.
 * UH_HYBRID_GLASS (bit 20) adds one pass to uh_render_hybrid directly AFTER the glossy pass (after the rtgi pass, or the deferred pass,
 * when those bits are clear) and BEFORE the marching-cubes, sky, fog, taa and post passes. For every G-buffer pixel whose material is of
 * type 2 it follows two deterministic chains of rays - one reflected, one transmitted at the visible surface - and REPLACES
 * deferred_output.rgb: whatever the deferred, reservoir-light, rtgi and glossy passes wrote on that pixel is overwritten; alpha is
 * untouched. The pass draws no random numbers. Everything float32 in the order written, nothing fused.
 *   event     Event(nd, N, ior) is reference.rchit:62-79 without the draw: dnd = dot(nd, N); outward = dnd > 0 ? -N : N; ratio =
 *             dnd > 0 ? ior : 1 / ior; cos = min(dot(-nd, outward), 1); sin = sqrt(1 - cos cos); cannot = ratio sin > 1; Fr =
 *             schlick(cos, ratio); R = reflect(nd, outward); T = refract(nd, outward, ratio). N has already been turned toward the ray
 *             (rchit:35-37), so dnd <= 0 and the ratio is 1 / ior on the way OUT of the glass as well as on the way in. That is the
 *             reference's behaviour, the path tracer reproduces it, and this pass shows the glass the path tracer shows - not textbook Snell.
 *   pixels    RTGI's rule first: position texel w != 0 and Nn = normalize(N) finite. The material index uint(pbr.a) is in range and its
 *             type is 2 (out of range counts as type 0). I = normalize(P - eye) is finite.
 *   first     Nf = dot(Nn, I) > 0 ? -Nn : Nn; Event(I, Nf, raytrace_properties.y). Chain 0 (reflected): direction R, weight w0 =
 *             cannot ? 1 : Fr. Chain 1 (transmitted): direction T, weight w1 = 1 - Fr; with `cannot` it is NOT cast: an all-zero record,
 *             counted dark, flag bit 0. Both start at offsetRay(P, Nf), tmin 0.001, tmax 10000, closest hit; events = 1.
 *   segment   its end: a miss takes the sky as UH_HYBRID_RTGI does ((1, 1, 1) under "furnace"), counted missed. Type 3: (1, 1, 1), counted
 *             emitter. Type 2 with events == max_events: the chain is CUT, L = 0, counted dark, its cut flag set; else Nh = the hit's
 *             world normal turned toward the ray, Event(normalize(d), Nh, the mesh's ior), d' = cannot ? R : T (unnormalised, rgen:61);
 *             d' not finite or of length 0 cuts the chain as well; else the next segment starts at offsetRay(o + t d, Nh) with
 *             events + 1. Any other type: UH_HYBRID_RTGI's shadowed-sun-lit Lambert (dark under "furnace"), one any-hit sun ray.
 *             L is clamped per channel with this pass's max_radiance; the chain's record is w L; an occluded sun ray zeroes it.
 *   pixel     C = clamp(R_0 + R_1) per channel (NaN, negative and -0 become +0, then the cap); deferred_output.rgb = C * intensity.
 * PARAMS: uh_set_glass_params validates and keeps them (a refused call leaves the old ones); the defaults of uh_glass_default_params:
 * max_events 8, max_radiance 16.0, intensity 1.0.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, in this order after every rule above: the bit and
 * view->raytracing_supported != 1; no G-buffer rendered in this call or an earlier one; the bit without UH_HYBRID_DEFERRED in the same
 * call. UH_ERR_CAPACITY for a frame of 2^27 pixels or more. UH_ERR_NOT_BUILT before uh_build_acceleration, as without the bit.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first glass pass; all three in G-buffer orientation):
 * UH_HYBRID_GLASS_RADIANCE, RGBA32F: (C, 1) where the pixel cast, (0, 0, 0, 0) elsewhere. UH_HYBRID_GLASS_COUNTS, 4 bytes per pixel:
 * sunlit, dark, emitter, missed; they sum to 2 where the pixel cast. UH_HYBRID_GLASS_EVENTS, 4 bytes per pixel: the events of chain 0,
 * the events of chain 1 (0 when it was not cast), the flags (bit 0: first-event TIR, bit 1: chain 0 cut, bit 2: chain 1 cut), 0.
 * RESOURCES: 28 bytes per pixel (counts, the radiance image, the events words, the pixel queue) and 72 bytes per ray (its hit record,
 * which becomes its radiance record, its origin and direction, its sun-ray record, a word in each of the two round queues), two rays per
 * pixel: 172 bytes per pixel of the frame, allocated by the first pass; freed by uh_destroy. A context that never sets the bit
 * allocates nothing. The pass enqueues max_events rounds of walk and bend whose counts stay on the device: no read-back, no wait.
 * STREAM ORDER: as uh_render_hybrid. uh_set_glass_params is host state, read by the next uh_render_hybrid; uh_get_glass_stats waits.
 * ISOLATION: the bit changes no reservoir, accumulation, gbuffer_position, grid, UhStats, RTAO, RTGI, glossy or fog state, and no hybrid
 * image but deferred_output (and what later passes of the call make of it) and its own three. Without the bit every pass, image,
 * statistic and allocation is what it was.
 * No uh_mgpu_ twin.
 * OUT OF SCOPE: a Fresnel split behind the first event; absorption or tint (the reference's glass is vec3(1)); rough transmission; point,
 * spot and reservoir lights at the hit; fog inside chains; the marching-cubes mesh in chains; the forward graph; teaching the rtgi or
 * glossy pass to skip glass pixels.
 * Arithmetic: DESIGN.md section 2, "Ray-traced glass". */
enum { UH_HYBRID_GLASS = 1u << 20 };
enum { UH_HYBRID_GLASS_RADIANCE = 25 /* RGBA32F: (C, 1) where the pixel cast */, UH_HYBRID_GLASS_COUNTS = 26 /* 4 x uint8: sunlit, dark, emitter, missed */,
       UH_HYBRID_GLASS_EVENTS = 27 /* 4 x uint8: events of chain 0, of chain 1, flags, 0 */ };
typedef struct UhGlassParams {
   uint32_t max_events; /* the events of a chain, the first included, 1..16: a chain that meets glass with this many behind it is cut */
   float max_radiance;  /* the cap of a chain's L, and of C, per channel; finite, > 0 */
   float intensity;     /* scales what the composite writes; finite, >= 0 */
} UhGlassParams;
UH_LAYOUT_ASSERT(sizeof(UhGlassParams) == 12 && offsetof(UhGlassParams, max_radiance) == 4 && offsetof(UhGlassParams, intensity) == 8, "UhGlassParams (12 B)");
/* the last glass pass: the pixels that cast; the chains cast (chains + the first-event TIR pixels == 2 * pixels); the segments walked
 * (segments == chains + events); the events behind the first; every event, the first included, at which `cannot` held; the chains cut;
 * the sun rays cast from the ends; the chains that missed; and the hipEvent times of classify + first event + the rounds' closest-hit
 * walks, of the rounds' bend kernels, of the sun rays' any-hit walk and of the composite. All zero before the first pass. Waits. */
typedef struct UhGlassStats {
   uint64_t pixels, chains, segments, events, tir, cut, shadow_rays, misses;
   float trace_ms, bend_ms, shadow_ms, composite_ms;
} UhGlassStats;
UH_LAYOUT_ASSERT(sizeof(UhGlassStats) == 80 && offsetof(UhGlassStats, chains) == 8 && offsetof(UhGlassStats, segments) == 16 &&
                    offsetof(UhGlassStats, events) == 24 && offsetof(UhGlassStats, tir) == 32 && offsetof(UhGlassStats, cut) == 40 &&
                    offsetof(UhGlassStats, shadow_rays) == 48 && offsetof(UhGlassStats, misses) == 56 && offsetof(UhGlassStats, trace_ms) == 64 &&
                    offsetof(UhGlassStats, bend_ms) == 68 && offsetof(UhGlassStats, shadow_ms) == 72 && offsetof(UhGlassStats, composite_ms) == 76,
                 "UhGlassStats (80 B)");
int uh_glass_default_params(UhGlassParams* out); /* needs no GPU: 8, 16.0, 1.0; UH_ERR_INVALID_ARGUMENT for NULL */
int uh_set_glass_params(uh_ctx* ctx, const UhGlassParams* params); /* validated here; a refused call leaves the old ones */
int uh_get_glass_stats(uh_ctx* ctx, UhGlassStats* out);            /* waits; all zero before the first pass */

/* ---- emissive meshes as area lights for the hybrid frame: direct light from the scene's own lamps, with soft shadows --------------------
 * An EXTENSION: the reference's closest-hit shader leaves its fourth material, the diffuse light, a "Todo" (reference.rchit:84-89: the path
 * ends with white), and its hybrid frame shades such a mesh as an ordinary surface. UH_HYBRID_AREA_LIGHTS (bit 21) adds one pass to
 * uh_render_hybrid directly AFTER the deferred pass and BEFORE the rtgi pass - and so before the glossy, glass, marching-cubes, sky, fog,
 * taa, post and present passes: TAA and the display chain see it. UH_HYBRID_FRAME | UH_HYBRID_AREA_LIGHTS is the natural call. The
 * deferred pass itself is untouched: this pass adds to deferred_output on the pixels that cast and writes the emitters' own pixels.
 *   emitters  the triangles of every mesh whose raytrace_properties.x == 3, in a table whose order does not depend on the tree: meshes
 *             in uh_add_mesh order, primitives in index order, slot = base[mesh] + prim. The table is filled on the device from the
 *             tree's own triangle packets (world-space v0, e1, e2), so it follows uh_set_instance_transform, uh_update_mesh_vertices,
 *             uh_pose_mesh, uh_update_isosurface_mesh, a refit and a rebuild, host- or device-built, with the same bytes. Ng =
 *             cross(e1, e2), area = 0.5 * sqrt(dot(Ng, Ng)), a non-finite area counts as 0. Integer weights: with N emitters, b = 31 -
 *             bit_length(N - 1) and amax = m * 2^x (frexpf) the largest area, q = max(1, trunc(ldexpf(area, b - x))) for area > 0, else
 *             0; cum the inclusive prefix of q, total = cum[N - 1] <= 2^31. Rebuilt, on the context's stream, by the first pass after a
 *             build or refit; never otherwise.
 *   pixels    RTAO's rule first: position texel w != 0 and Nn = normalize(N) finite. Then the material record as deferred.frag forms it
 *             (index uint(pbr.a), in range): a pixel of type 3, or of type 1 with view->raytracing_supported == 1 (it holds its
 *             reflection), does not cast. With total == 0 no pixel casts.
 *   samples   a pixel (px, py) that casts takes `samples` of them; sample s draws from the state initRNG(px, py, W, (frameNumber(view) *
 *             64 + s) ^ 0x41524541) the 32-bit word r that randomFloat would convert, then u1 and u2 = randomFloat. The emitter i is the
 *             first slot with cum[i] > ((uint64_t)r * total) >> 32; its point Y = (v0 + u1 e1) + u2 e2 after u1 + u2 > 1 folds both to
 *             1 - u. With w = Y - P, d2 = dot(w, w), l = w / sqrt(d2), cosL = |dot(Ng, l)| / sqrt(dot(Ng, Ng)) (emitters shine from both
 *             faces), NdotL = dot(N, l) and G = min((cosL / d2) * ((area * total) / q), max_weight): the sample is AWAY - it adds nothing and
 *             casts no ray - when d2, NdotL or cosL is not > 0 or G is NaN. Otherwise one any-hit ray from o = offsetRay(P, Nn) toward Y,
 *             tmin 0.001, tmax 0.999 |Y - o|: a hit makes it OCCLUDED, none (or an empty interval) LIT. A LIT sample brings the two halves
 *             of deferred.frag's surfaceShading for direction l and radiance Li = (1, 1, 1) * G - the emission every other pass gives type
 *             3 -: d = kD * (Li * NdotL), without base / PI, and s = specular * (Li * NdotL).
 *   pixel     D = (d_0 + ... + d_{samples-1}) / (float)samples and Sp likewise, summed in sample order (AWAY and OCCLUDED add +0), then per
 *             channel min(x > 0 ? x : 0, max_radiance): a NaN is 0, the value is finite and does not depend on the schedule.
 *   filter    UH_HYBRID_RTGI's, on D and on Sp alike: blur_radius 0 is the identity; r > 0: the mean over the taps (dx, dy) in [-r, r]^2
 *             (dy outer) that lie in the frame, cast themselves and pass dot(Nn_tap, Nn) >= blur_normal_cos and |dot(P_tap - P, Nn)| <=
 *             blur_plane; the centre always counts. The base colour is applied after the filter and stays sharp.
 *   composite for every pixel that cast, with base = pow(albedo, 2.2) * base_color as deferred.frag:61-65 forms it: add = (((base / PI) *
 *             Df) + Spf) * intensity; deferred_output.rgb += add, alpha untouched. No occlusion, ssao or shadow factor: direct light,
 *             shadowed by its own rays. A pixel whose position texel has w != 0 and whose material is type 3 gets deferred_output.rgb =
 *             (1, 1, 1) * intensity when show_emitters == 1 and is left alone when it is 0. Under option "furnace" the pass runs unchanged.
 * PARAMS: uh_set_area_light_params validates and keeps them for the calls that follow (a refused call leaves the old ones); before the
 * first call the defaults of uh_area_light_default_params hold: 2 samples, blur_radius 3, show_emitters 1, max_weight 64.0, max_radiance
 * 16.0, intensity 1.0, 0.9, 0.05.
 * UH_ERR_INVALID_ARGUMENT with a message, and nothing runs, in this order after every rule above (UH_HYBRID_GLASS's included): the bit and
 * view->raytracing_supported != 1; no G-buffer rendered in this call or an earlier one; the bit without UH_HYBRID_DEFERRED in the same
 * call. UH_ERR_CAPACITY for a frame of 2^28 pixels or more, and for more than 2^20 emitter triangles, at the call that sets the bit.
 * There is no ibl_enabled rule: this is direct light. UH_ERR_NOT_BUILT before uh_build_acceleration, as without the bit. A scene without
 * emitters, or with degenerate ones alone, is no refusal: no pixel casts, the images are zero and deferred_output stays what it was.
 * READ-BACK (uh_read_hybrid, UH_ERR_INVALID_ARGUMENT before the first area-light pass; all three in G-buffer orientation):
 * UH_HYBRID_AREA_DIFFUSE, RGBA32F: Df, w = 1 where the pixel cast, (0, 0, 0, 0) elsewhere. UH_HYBRID_AREA_SPECULAR, RGBA32F: Spf, w
 * likewise. UH_HYBRID_AREA_COUNTS, 4 bytes per pixel: the samples that were lit, occluded and away, and 0; they sum to `samples` where the
 * pixel cast and are all 0 elsewhere. uh_read_area_emitters reads the table back.
 * RESOURCES: 72 bytes per pixel (counts, the two images, their unfiltered means, the queue of the pixels that cast), 64 bytes per sample
 * (its two records and its ray) at the largest `samples` a pass has run with, and 64 bytes per emitter triangle, allocated by the first
 * pass; freed by uh_destroy. A context that never sets the bit allocates nothing for it.
 * STREAM ORDER: as uh_render_hybrid. uh_set_area_light_params is host state, read by the next uh_render_hybrid; uh_get_area_light_stats
 * and uh_read_area_emitters wait.
 * ISOLATION: the bit changes no reservoir, accumulation, gbuffer_position, grid, UhStats, RTAO, RTGI, glossy, glass or fog state, and no
 * hybrid image but deferred_output (and what later passes of the call make of it) and its own three. Without the bit every pass, image,
 * statistic and allocation is what it was.
 * No uh_mgpu_ twin.
 * OPTIONS: "area_light_order" 0 (default) or 1 lays the sample kernel's work out (same images whichever; DESIGN.md section 4 "Area lights").
 * OUT OF SCOPE: emission other than (1, 1, 1) (textures, strengths); emitters in the path tracer, ReSTIR, the forward graph, or at the
 * hits of RTGI, GLOSSY, GLASS or FOG rays; mapping glTF emissiveFactor in the loaders; light hierarchies or reservoir resampling of the
 * picks; a history of its own (UH_HYBRID_TAA serves).
 * Arithmetic: DESIGN.md section 2, "Area lights". */
enum { UH_HYBRID_AREA_LIGHTS = 1u << 21 };
enum { UH_HYBRID_AREA_DIFFUSE = 28 /* RGBA32F: Df, w = 1 where the pixel cast */, UH_HYBRID_AREA_SPECULAR = 29 /* RGBA32F: Spf, w likewise */,
       UH_HYBRID_AREA_COUNTS = 30 /* 4 x uint8: lit, occluded, away, 0 */ };
typedef struct UhAreaLightParams {
   uint32_t samples;       /* samples per pixel that casts, 1..16 */
   uint32_t blur_radius;   /* 0 = no filter; else 1..6: taps dx, dy in [-r, r] */
   uint32_t show_emitters; /* 1: a type-3 pixel is written (1, 1, 1) * intensity; 0: it is left alone */
   float max_weight;       /* the cap of a sample's G = (cosL / d2) / pdf; finite, > 0 */
   float max_radiance;     /* the cap of D and Sp per channel; finite, > 0 */
   float intensity;        /* scales what the composite adds and the emitter pixels; finite, >= 0 */
   float blur_normal_cos;  /* a tap counts when dot(Nn_tap, Nn) >= this; not NaN */
   float blur_plane;       /* and |dot(P_tap - P, Nn)| <= this (world units); not NaN */
} UhAreaLightParams;
UH_LAYOUT_ASSERT(sizeof(UhAreaLightParams) == 32 && offsetof(UhAreaLightParams, blur_radius) == 4 && offsetof(UhAreaLightParams, show_emitters) == 8 &&
                    offsetof(UhAreaLightParams, max_weight) == 12 && offsetof(UhAreaLightParams, max_radiance) == 16 &&
                    offsetof(UhAreaLightParams, intensity) == 20 && offsetof(UhAreaLightParams, blur_normal_cos) == 24 &&
                    offsetof(UhAreaLightParams, blur_plane) == 28,
                 "UhAreaLightParams (32 B)");
/* the last area-light pass: the pixels that cast, their samples (pixels * samples), the shadow rays cast (the samples that were not away),
 * those that were occluded, the emitter pixels; the table's emitter triangles N, its total weight and how often it has been built; and
 * the hipEvent times of the last table build, of classify + sampling, of the shadow rays' any-hit walk, of the means + filter and of the
 * composite. All zero before the first pass. Waits for all work of the context. */
typedef struct UhAreaLightStats {
   uint64_t pixels, samples, shadow_rays, occluded, emitter_pixels, emitters, total_weight, table_builds;
   float table_ms, sample_ms, shadow_ms, filter_ms, composite_ms;
   uint32_t reserved;
} UhAreaLightStats;
UH_LAYOUT_ASSERT(sizeof(UhAreaLightStats) == 88 && offsetof(UhAreaLightStats, samples) == 8 && offsetof(UhAreaLightStats, shadow_rays) == 16 &&
                    offsetof(UhAreaLightStats, occluded) == 24 && offsetof(UhAreaLightStats, emitter_pixels) == 32 &&
                    offsetof(UhAreaLightStats, emitters) == 40 && offsetof(UhAreaLightStats, total_weight) == 48 &&
                    offsetof(UhAreaLightStats, table_builds) == 56 && offsetof(UhAreaLightStats, table_ms) == 64 &&
                    offsetof(UhAreaLightStats, sample_ms) == 68 && offsetof(UhAreaLightStats, shadow_ms) == 72 &&
                    offsetof(UhAreaLightStats, filter_ms) == 76 && offsetof(UhAreaLightStats, composite_ms) == 80 &&
                    offsetof(UhAreaLightStats, reserved) == 84,
                 "UhAreaLightStats (88 B)");
int uh_area_light_default_params(UhAreaLightParams* out); /* needs no GPU: 2, 3, 1, 64.0, 16.0, 1.0, 0.9, 0.05; UH_ERR_INVALID_ARGUMENT for NULL */
int uh_set_area_light_params(uh_ctx* ctx, const UhAreaLightParams* params); /* validated here; a refused call leaves the old ones */
int uh_get_area_light_stats(uh_ctx* ctx, UhAreaLightStats* out);            /* waits; all zero before the first pass */
/* The emitter table of the last area-light pass, in slot order: the packet keys (mesh << 22 | prim), the areas and the integer weights of
 * its first min(capacity, N) slots into whichever of the three arrays is not NULL, and N into *count. capacity == 0 returns the count
 * alone. Waits. UH_ERR_INVALID_ARGUMENT for a NULL count, and before the first pass. */
int uh_read_area_emitters(uh_ctx* ctx, uint32_t capacity, uint32_t* keys, float* areas, uint32_t* weights, uint32_t* count);

#ifdef __cplusplus
}
#endif

#endif /* UTOPIAN_HIP_H */
