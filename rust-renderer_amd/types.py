"""ctypes / numpy mirrors of the POD structs in include/utopian_hip.h.

Each struct is byte-identical to the reference's GPU-side struct it replaces:
Vertex (utopian/src/primitive.rs:9-17), GpuMaterial / GpuMesh / GpuLight
(utopian/src/renderer.rs:20-59), ViewUniformData (utopian/src/renderer.rs:84-120),
Reservoir (utopian/shaders/include/restir_sampling.glsl:51-57).
"""
import ctypes as C

import numpy as np

VERTEX_DTYPE = np.dtype(
    [("pos", "<f4", 4), ("normal", "<f4", 4), ("uv", "<f4", 2), ("_pad", "<f4", 2), ("color", "<f4", 4), ("tangent", "<f4", 4)]
)
assert VERTEX_DTYPE.itemsize == 80

RESERVOIR_DTYPE = np.dtype([("Y", "<i4"), ("W_sum", "<f4"), ("W_X", "<f4"), ("M", "<i4")])
assert RESERVOIR_DTYPE.itemsize == 16

# MaterialType (utopian/src/gltf_loader.rs:11-17)
LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT = 0, 1, 2, 3
PBR = 4  # extension: Cook-Torrance from metallic_factor / roughness_factor; no reference scene uses it


class GpuMaterial(C.Structure):
    _fields_ = [
        ("diffuse_map", C.c_uint32),
        ("normal_map", C.c_uint32),
        ("metallic_roughness_map", C.c_uint32),
        ("occlusion_map", C.c_uint32),
        ("base_color_factor", C.c_float * 4),
        ("metallic_factor", C.c_float),
        ("roughness_factor", C.c_float),
        ("padding", C.c_float * 2),
        ("raytrace_properties", C.c_float * 4),
    ]


class GpuLight(C.Structure):
    _fields_ = [
        ("color", C.c_float * 4),
        ("position", C.c_float * 3),
        ("range", C.c_float),
        ("direction", C.c_float * 3),
        ("spot", C.c_float),
        ("attenuation", C.c_float * 3),
        ("light_type", C.c_float),
        ("intensity", C.c_float * 3),
        ("id", C.c_float),
        ("padding", C.c_float * 4),
    ]


class ViewUniformData(C.Structure):
    _fields_ = [
        ("view", C.c_float * 16),
        ("projection", C.c_float * 16),
        ("inverse_view", C.c_float * 16),
        ("inverse_projection", C.c_float * 16),
        ("prev_frame_projection_view", C.c_float * 16),
        ("eye_pos", C.c_float * 3),
        ("samples_per_frame", C.c_uint32),
        ("sun_dir", C.c_float * 3),
        ("total_samples", C.c_uint32),
        ("num_bounces", C.c_uint32),
        ("viewport_width", C.c_uint32),
        ("viewport_height", C.c_uint32),
        ("time", C.c_float),
        ("num_lights", C.c_uint32),
        ("shadows_enabled", C.c_uint32),
        ("ssao_enabled", C.c_uint32),
        ("fxaa_enabled", C.c_uint32),
        ("cubemap_enabled", C.c_uint32),
        ("ibl_enabled", C.c_uint32),
        ("sky_enabled", C.c_uint32),
        ("sun_shadow_enabled", C.c_uint32),
        ("lights_enabled", C.c_uint32),
        ("max_num_lights_used", C.c_uint32),
        ("marching_cubes_enabled", C.c_uint32),
        ("temporal_reuse_enabled", C.c_uint32),
        ("spatial_reuse_enabled", C.c_uint32),
        ("rebuild_tlas", C.c_uint32),
        ("accumulation_limit", C.c_uint32),
        ("use_ris_light_sampling", C.c_uint32),
        ("raytracing_supported", C.c_uint32),
        ("_tail_pad", C.c_uint32 * 3),
    ]


class Reservoir(C.Structure):
    _fields_ = [("Y", C.c_int32), ("W_sum", C.c_float), ("W_X", C.c_float), ("M", C.c_int32)]


RAY_KINDS = 5
RAY_PRIMARY, RAY_BOUNCE, RAY_SUN_SHADOW, RAY_LIGHT_SHADOW, RAY_GBUFFER = range(5)


class RestirRows(C.Structure):
    """UhRestirRows: the rows a context's reservoir passes cover under uh_set_restir_partition"""
    _fields_ = [(n, C.c_uint32) for n in ("band_row0", "band_rows", "reuse_row0", "reuse_rows", "reuse_extra_row0", "reuse_extra_rows",
                                          "cast_row0", "cast_rows", "cast_extra_row0", "cast_extra_rows", "rows_per_band")]


# int exchange(void* user, void* hip_stream, void* spatial_base, uint64_t band_bytes, uint32_t rank, uint32_t world)
RESTIR_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32)


class Stats(C.Structure):
    _fields_ = [
        ("rays", C.c_uint64 * RAY_KINDS),
        ("nodes_visited", C.c_uint64),
        ("tris_tested", C.c_uint64),
        ("shadow_nodes_visited", C.c_uint64),
        ("shadow_tris_tested", C.c_uint64),
        ("closest_hits", C.c_uint64),
        ("misses", C.c_uint64),
        ("frames", C.c_uint64),
        ("bvh_nodes", C.c_uint32),
        ("bvh_triangles", C.c_uint32),
        ("build_ms", C.c_float),
        ("last_frame_ms", C.c_float),
        ("trace_closest_ms", C.c_float),
        ("trace_shadow_ms", C.c_float),
        ("shade_ms", C.c_float),
        ("trace_closest_launches", C.c_uint32),
        ("sun_grid_cells", C.c_uint32),
        ("sun_grid_entries", C.c_uint32),
        ("sun_grid_build_ms", C.c_float),
        ("sun_grid_mean_list", C.c_float),
        ("sun_tree_rays", C.c_uint64),
        ("camera_grid_cells", C.c_uint32),
        ("camera_grid_entries", C.c_uint32),
        ("camera_grid_build_ms", C.c_float),
        ("camera_grid_mean_list", C.c_float),
        ("camera_tree_rays", C.c_uint64),
        ("camera_grid_tris_tested", C.c_uint64),
        ("camera_grid_ms", C.c_float),
        ("trace_light_ms", C.c_float),
        ("sun_covered_rays", C.c_uint64),
        ("sun_grid_bytes", C.c_uint64),
        ("camera_grid_bytes", C.c_uint64),
        ("light_nodes_visited", C.c_uint64),
        ("light_tris_tested", C.c_uint64),
        ("trace_light_launches", C.c_uint32),
        ("reserved1", C.c_uint32),
    ]

    @property
    def path_rays(self):
        """rays the metric counts: primary + bounce + sun-shadow + light-shadow (not G-buffer)."""
        return sum(self.rays[i] for i in range(4))


assert C.sizeof(GpuMaterial) == 64
assert C.sizeof(GpuLight) == 96
assert C.sizeof(ViewUniformData) == 448
assert C.sizeof(Reservoir) == 16
assert ViewUniformData.eye_pos.offset == 320 and ViewUniformData.samples_per_frame.offset == 332
assert ViewUniformData.sun_dir.offset == 336 and ViewUniformData.total_samples.offset == 348
assert ViewUniformData.num_bounces.offset == 352 and ViewUniformData.sky_enabled.offset == 392
assert ViewUniformData.accumulation_limit.offset == 424 and ViewUniformData.raytracing_supported.offset == 432

PASS_GBUFFER, PASS_RESET_RESERVOIRS, PASS_INITIAL_RIS, PASS_TEMPORAL_REUSE, PASS_SPATIAL_REUSE, PASS_REFERENCE_PT = (1 << i for i in range(6))
PASS_RESTIR = 0x1F
PASS_ALL = 0x3F

UH_OK = 0
ERR_NAMES = {1: "INVALID_ARGUMENT", 2: "NO_DEVICE", 3: "HIP", 4: "CAPACITY", 5: "NOT_BUILT", 6: "OUT_OF_MEMORY"}

# the hybrid graph's ray-traced passes (uh_render_hybrid; utopian/src/renderers/mod.rs:61-186)
HYBRID_RT_SHADOWS, HYBRID_GBUFFER, HYBRID_RT_REFLECTIONS = 1 << 0, 1 << 1, 1 << 2
HYBRID_ALL = 7
HYBRID_POSITION, HYBRID_NORMAL, HYBRID_ALBEDO, HYBRID_PBR, HYBRID_SHADOWS, HYBRID_REFLECTIONS = range(6)


class HybridStats(C.Structure):
    """UhHybridStats: the last uh_render_hybrid call - rays and hipEvent ms of (G-buffer, rt_shadows, rt_reflections)"""

    _fields_ = [("rays", C.c_uint64 * 3), ("pass_ms", C.c_float * 3), ("reflection_pixels", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(HybridStats) == 48 and HybridStats.pass_ms.offset == 24 and HybridStats.reflection_pixels.offset == 36


# the hybrid graph's final frame (ssao_pass, deferred_pass, atmosphere_pass, present_pass; mod.rs:136-186)
HYBRID_SSAO, HYBRID_DEFERRED, HYBRID_SKY, HYBRID_PRESENT = 1 << 3, 1 << 4, 1 << 5, 1 << 6
HYBRID_FRAME = 0x7F
HYBRID_SSAO_IMAGE, HYBRID_DEFERRED_OUTPUT, HYBRID_PRESENT_OUTPUT = 6, 7, 8


class HybridFrameStats(C.Structure):
    """UhHybridFrameStats: the last uh_render_hybrid call - hipEvent ms of the pass of each bit (rt_shadows, G-buffer, rt_reflections,
    SSAO, deferred, sky, present), the sky pixels written and the lights evaluated per pixel (the sun included)"""

    _fields_ = [("pass_ms", C.c_float * 7), ("sky_pixels", C.c_uint32), ("lights", C.c_uint32), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(HybridFrameStats) == 48 and HybridFrameStats.sky_pixels.offset == 28 and HybridFrameStats.lights.offset == 32


# image-based lighting: setup_cubemap_pass (ibl.rs) - the environment, irradiance and specular cubes and the BRDF LUT
HYBRID_ENVIRONMENT = 1 << 7
ENV_SIZE, ENV_MIPS, BRDF_LUT_SIZE = 512, 8, 512
ENV_ENVIRONMENT, ENV_IRRADIANCE, ENV_SPECULAR, ENV_BRDF_LUT = range(4)


class EnvironmentStats(C.Structure):
    """UhEnvironmentStats: the last UH_HYBRID_ENVIRONMENT build - hipEvent ms of its sub-passes (environment, irradiance, specular,
    BRDF LUT), the builds so far, and the sun direction (as given) and eye the maps were built with"""

    _fields_ = [("pass_ms", C.c_float * 4), ("builds", C.c_uint32), ("sun_dir", C.c_float * 3), ("eye", C.c_float * 3), ("reserved", C.c_uint32 * 5)]


assert C.sizeof(EnvironmentStats) == 64 and EnvironmentStats.builds.offset == 16 and EnvironmentStats.sun_dir.offset == 20 and EnvironmentStats.eye.offset == 32


# cascaded shadow maps: setup_shadow_pass (shadow.rs) and the deferred pass's calculateShadow
HYBRID_SHADOW_MAPS = 1 << 8
SHADOW_CASCADES = 4


class ShadowmapParams(C.Structure):
    """UhShadowmapParams: deferred.frag's UBO_shadowmapParams - four column-major view-projection matrices and the split depths"""

    _fields_ = [("view_projection_matrices", (C.c_float * 16) * 4), ("cascade_splits", C.c_float * 4)]


assert C.sizeof(ShadowmapParams) == 272 and ShadowmapParams.cascade_splits.offset == 256


class ShadowMapStats(C.Structure):
    """UhShadowMapStats: the last shadow-map render - hipEvent ms, renders so far, map size, triangles per cascade that reached the
    rasteriser, and the params snapshot the deferred pass reads"""

    _fields_ = [("pass_ms", C.c_float), ("renders", C.c_uint32), ("size", C.c_uint32), ("triangles", C.c_uint32 * 4), ("reserved", C.c_uint32),
                ("params", ShadowmapParams)]


assert C.sizeof(ShadowMapStats) == 304 and ShadowMapStats.triangles.offset == 12 and ShadowMapStats.params.offset == 32


# the forward graph: build_minimal_forward_render_graph (utopian/src/renderers/mod.rs; the reference's render mode 3)
FORWARD_PASS, FORWARD_PRESENT = 1 << 0, 1 << 1
FORWARD_SHADOW_MAPS = HYBRID_SHADOW_MAPS
FORWARD_GRAPH = FORWARD_SHADOW_MAPS | FORWARD_PASS | FORWARD_PRESENT
FORWARD_OUTPUT, FORWARD_DEPTH, FORWARD_VISIBILITY, FORWARD_PRESENT_OUTPUT = range(4)
FORWARD_NONE = 0xFFFFFFFF  # FORWARD_VISIBILITY of a pixel nothing was drawn on


class ForwardStats(C.Structure):
    """UhForwardStats: the last uh_render_forward call - hipEvent ms of (shadow maps, forward, present), the forward renders so far, and
    of the last forward pass the triangle pieces that reached the rasteriser, the covered pixels and the lights evaluated (the sun
    included)"""

    _fields_ = [("pass_ms", C.c_float * 3), ("renders", C.c_uint32), ("pieces", C.c_uint32), ("covered_pixels", C.c_uint32), ("lights", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(ForwardStats) == 32 and ForwardStats.renders.offset == 12 and ForwardStats.pieces.offset == 16 and \
    ForwardStats.covered_pixels.offset == 20 and ForwardStats.lights.offset == 24


# the hybrid graph's marching-cubes pass: setup_marching_cubes_pass (mod.rs:164-174, renderers/marching_cubes.rs); bit 9 stays unused
HYBRID_MARCHING_CUBES = 1 << 10
HYBRID_DEPTH, HYBRID_MARCHING_CUBES_VISIBILITY = 9, 10
MARCHING_CUBES_NONE = 0xFFFFFFFF  # HYBRID_MARCHING_CUBES_VISIBILITY of a pixel no marching-cubes fragment survived on


class MarchingCubesStats(C.Structure):
    """UhMarchingCubesStats: the last marching-cubes pass - hipEvent ms, the passes so far, triangles extracted (zero-area ones included),
    pieces that reached the rasteriser, covered pixels, lights evaluated (the sun included) and the view.time used"""

    _fields_ = [("pass_ms", C.c_float), ("renders", C.c_uint32), ("triangles", C.c_uint32), ("pieces", C.c_uint32), ("covered_pixels", C.c_uint32),
                ("lights", C.c_uint32), ("time", C.c_float), ("reserved", C.c_uint32)]


assert C.sizeof(MarchingCubesStats) == 32 and MarchingCubesStats.triangles.offset == 8 and MarchingCubesStats.pieces.offset == 12 and \
    MarchingCubesStats.covered_pixels.offset == 16 and MarchingCubesStats.lights.offset == 20 and MarchingCubesStats.time.offset == 24


class IsosurfaceUpdateStats(C.Structure):
    """UhIsosurfaceUpdateStats: uh_update_isosurface_mesh so far - hipEvent ms of the last extraction and of the refreshes from device
    vertices since, the updates, the last one's triangles, geometry bytes of updated meshes moved between host and device (cumulative)
    and the device memory held for device-resident meshes"""

    _fields_ = [("extract_ms", C.c_float), ("scatter_ms", C.c_float), ("updates", C.c_uint32), ("triangles", C.c_uint32),
                ("host_geometry_bytes", C.c_uint64), ("device_bytes", C.c_uint64)]


assert C.sizeof(IsosurfaceUpdateStats) == 32 and IsosurfaceUpdateStats.updates.offset == 8 and IsosurfaceUpdateStats.triangles.offset == 12 and \
    IsosurfaceUpdateStats.host_geometry_bytes.offset == 16 and IsosurfaceUpdateStats.device_bytes.offset == 24


VERTICES_HOST, VERTICES_DEVICE = 0, 1  # uh_update_mesh_vertices' `where`


class MeshUpdateStats(C.Structure):
    """UhMeshUpdateStats: uh_update_mesh_vertices so far - hipEvent ms of k_deform_gather and of the refit behind it in the last refit
    that gathered, the updates, the triangles that refit rewrote, vertex and packet bytes of updated meshes moved between host and
    device (cumulative) and the vertex and index buffers held for updated meshes"""

    _fields_ = [("gather_ms", C.c_float), ("refit_ms", C.c_float), ("updates", C.c_uint32), ("triangles", C.c_uint32),
                ("host_geometry_bytes", C.c_uint64), ("device_bytes", C.c_uint64)]


assert C.sizeof(MeshUpdateStats) == 32 and MeshUpdateStats.updates.offset == 8 and MeshUpdateStats.triangles.offset == 12 and \
    MeshUpdateStats.host_geometry_bytes.offset == 16 and MeshUpdateStats.device_bytes.offset == 24


class PoseStats(C.Structure):
    """UhPoseStats: uh_pose_mesh so far - hipEvent ms of the last k_pose, the poses, the last one's vertices, joints and active (non-zero)
    targets, the largest joint count the kernel stages in LDS, and the device memory held for posed meshes"""

    _fields_ = [("pose_ms", C.c_float), ("poses", C.c_uint32), ("vertices", C.c_uint32), ("joints", C.c_uint32), ("active_targets", C.c_uint32),
                ("staged_joint_limit", C.c_uint32), ("device_bytes", C.c_uint64)]


assert C.sizeof(PoseStats) == 32 and PoseStats.poses.offset == 4 and PoseStats.staged_joint_limit.offset == 20 and PoseStats.device_bytes.offset == 24


# the hybrid graph's G-buffer pass rasterised (gbuffer.rs, gbuffer.vert / gbuffer.frag): a modifier of HYBRID_GBUFFER
HYBRID_GBUFFER_RASTER = 1 << 11
HYBRID_GBUFFER_DEPTH, HYBRID_GBUFFER_VISIBILITY = 11, 12
GBUFFER_NONE = 0xFFFFFFFF  # HYBRID_GBUFFER_VISIBILITY of a pixel no fragment survived on


class GbufferRasterStats(C.Structure):
    """UhGbufferRasterStats: the last rasterised G-buffer pass - hipEvent ms, the rasterised passes so far, pieces that reached the
    rasteriser and covered pixels"""

    _fields_ = [("pass_ms", C.c_float), ("renders", C.c_uint32), ("pieces", C.c_uint32), ("covered_pixels", C.c_uint32)]


assert C.sizeof(GbufferRasterStats) == 16 and GbufferRasterStats.renders.offset == 4 and GbufferRasterStats.pieces.offset == 8 and \
    GbufferRasterStats.covered_pixels.offset == 12


# the hybrid frame's local lights from the ReSTIR reservoirs (an extension; utopian_hip.h "UH_HYBRID_RESTIR_LIGHTS"); bit 9 stays unused
HYBRID_RESTIR_LIGHTS = 1 << 12
HYBRID_LIGHT_VISIBILITY = 13


class HybridRestirStats(C.Structure):
    """UhHybridRestirStats: the last render_hybrid call with HYBRID_RESTIR_LIGHTS - rays cast, the occluded ones, hipEvent ms of the pass"""

    _fields_ = [("rays", C.c_uint64), ("occluded", C.c_uint64), ("pass_ms", C.c_float), ("reserved", C.c_uint32 * 3)]


assert C.sizeof(HybridRestirStats) == 32 and HybridRestirStats.occluded.offset == 8 and HybridRestirStats.pass_ms.offset == 16 and \
    HybridRestirStats.reserved.offset == 20


# the denoiser (an extension; utopian_hip.h "the denoiser"): uh_denoise's flags, the images of uh_read_denoised, params and stats
DENOISE_TEMPORAL, DENOISE_DEMODULATE = 1 << 0, 1 << 1
DENOISE_MOTION = 1 << 3  # reproject through the motion image of HYBRID_MOTION; bit 2 stays an unknown flag
DENOISE_COLOR, DENOISE_OUTPUT, DENOISE_INPUT, DENOISE_TEMPORAL_COLOR, DENOISE_HISTORY, DENOISE_VARIANCE = range(6)


class DenoiseParams(C.Structure):
    """UhDenoiseParams: flags (DENOISE_*), a-trous levels (0..5), the history cap, the smallest blend factor, the luminance and plane
    tolerances of the filter, and the normal and plane tolerances of a history tap; uh_denoise_default_params fills the defaults"""

    _fields_ = [("flags", C.c_uint32), ("iterations", C.c_uint32), ("max_history", C.c_uint32), ("alpha_min", C.c_float),
                ("sigma_luminance", C.c_float), ("sigma_plane", C.c_float), ("reproject_normal_cos", C.c_float), ("reproject_plane", C.c_float),
                ("reserved", C.c_uint32 * 4)]


assert C.sizeof(DenoiseParams) == 48 and DenoiseParams.alpha_min.offset == 12 and DenoiseParams.reproject_plane.offset == 28 and \
    DenoiseParams.reserved.offset == 32


class DenoiseStats(C.Structure):
    """UhDenoiseStats: the last uh_denoise call - hipEvent ms of (input + temporal, variance estimate, a-trous levels, output), the
    geometry pixels and those of them that kept a history"""

    _fields_ = [("pass_ms", C.c_float * 4), ("geometry_pixels", C.c_uint32), ("history_pixels", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(DenoiseStats) == 32 and DenoiseStats.geometry_pixels.offset == 16 and DenoiseStats.history_pixels.offset == 20 and \
    DenoiseStats.reserved.offset == 24


# ray-traced ambient occlusion in the hybrid frame's SSAO slot (an extension; utopian_hip.h "UH_HYBRID_RTAO"); bit 9 stays unused
HYBRID_RTAO = 1 << 13
HYBRID_AO_COUNTS = 14


class RtaoParams(C.Structure):
    """UhRtaoParams: rays per geometry pixel (1..64), their reach in world units, the strength of ao = 1 - strength * occluded / samples,
    the filter's radius (0 none, else 1..4: taps in [-r, r)^2) and a tap's normal and plane thresholds; uh_rtao_default_params fills
    the defaults"""

    _fields_ = [("samples", C.c_uint32), ("radius", C.c_float), ("strength", C.c_float), ("blur_radius", C.c_uint32),
                ("blur_normal_cos", C.c_float), ("blur_plane", C.c_float)]


assert C.sizeof(RtaoParams) == 24 and RtaoParams.radius.offset == 4 and RtaoParams.strength.offset == 8 and RtaoParams.blur_radius.offset == 12 and \
    RtaoParams.blur_normal_cos.offset == 16 and RtaoParams.blur_plane.offset == 20


class RtaoStats(C.Structure):
    """UhRtaoStats: the last rtao pass - the pixels that cast, their rays, the occluded ones, hipEvent ms of classify + trace and of the
    resolve / filter"""

    _fields_ = [("pixels", C.c_uint64), ("rays", C.c_uint64), ("occluded", C.c_uint64), ("trace_ms", C.c_float), ("filter_ms", C.c_float)]


assert C.sizeof(RtaoStats) == 32 and RtaoStats.rays.offset == 8 and RtaoStats.occluded.offset == 16 and RtaoStats.trace_ms.offset == 24 and \
    RtaoStats.filter_ms.offset == 28


# one-bounce ray-traced diffuse GI of the hybrid frame (an extension; utopian_hip.h "UH_HYBRID_RTGI"): the pass behind the deferred pass and
# its two images; bit 9 stays unused
HYBRID_RTGI = 1 << 17
HYBRID_GI_RADIANCE, HYBRID_GI_COUNTS = 18, 19


class RtgiParams(C.Structure):
    """UhRtgiParams: rays per pixel that casts (1..16), the filter's radius (0 none, else 1..6: taps in [-r, r]^2), the cap of a ray's
    radiance, the scale of what the composite adds, and a tap's normal and plane thresholds; uh_rtgi_default_params fills the defaults"""

    _fields_ = [("samples", C.c_uint32), ("blur_radius", C.c_uint32), ("max_radiance", C.c_float), ("intensity", C.c_float),
                ("blur_normal_cos", C.c_float), ("blur_plane", C.c_float)]


assert C.sizeof(RtgiParams) == 24 and [getattr(RtgiParams, n).offset for n, _ in RtgiParams._fields_] == list(range(0, 24, 4))


class RtgiStats(C.Structure):
    """UhRtgiStats: the last rtgi pass - the pixels that cast, their rays, the sun rays cast from the hits, the rays that missed, hipEvent
    ms of classify + closest-hit walk, of the sun rays' walk, of the mean + filter and of the composite"""

    _fields_ = [("pixels", C.c_uint64), ("rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("misses", C.c_uint64), ("trace_ms", C.c_float),
                ("shadow_ms", C.c_float), ("filter_ms", C.c_float), ("composite_ms", C.c_float)]


assert C.sizeof(RtgiStats) == 48 and RtgiStats.misses.offset == 24 and RtgiStats.trace_ms.offset == 32 and RtgiStats.composite_ms.offset == 44


# ray-traced glossy reflections of the hybrid frame (an extension; utopian_hip.h "UH_HYBRID_GLOSSY"): the pass behind the rtgi pass and its
# three images
HYBRID_GLOSSY = 1 << 18
HYBRID_GLOSSY_SCALE, HYBRID_GLOSSY_BIAS, HYBRID_GLOSSY_COUNTS = 20, 21, 22


class GlossyParams(C.Structure):
    """UhGlossyParams: rays per pixel that casts (1..16), the filter's largest radius (0..6), the roughness up to which a pixel casts, the
    cap of a ray's radiance, the scale of what the composite adds, the roughness at which a pixel's radius reaches blur_radius, and a
    tap's normal and plane thresholds; uh_glossy_default_params fills the defaults"""

    _fields_ = [("samples", C.c_uint32), ("blur_radius", C.c_uint32), ("max_roughness", C.c_float), ("max_radiance", C.c_float),
                ("intensity", C.c_float), ("blur_roughness", C.c_float), ("blur_normal_cos", C.c_float), ("blur_plane", C.c_float)]


assert C.sizeof(GlossyParams) == 32 and [getattr(GlossyParams, n).offset for n, _ in GlossyParams._fields_] == list(range(0, 32, 4))


class GlossyStats(C.Structure):
    """UhGlossyStats: the last glossy pass - the pixels that cast, the rays cast, the below samples, the sun rays cast from the hits, the
    rays that missed, hipEvent ms of classify + ray generation + closest-hit walk, of the hit shading, of the sun rays' walk, of the
    sums + filter and of the composite"""

    _fields_ = [("pixels", C.c_uint64), ("rays", C.c_uint64), ("below", C.c_uint64), ("shadow_rays", C.c_uint64), ("misses", C.c_uint64),
                ("trace_ms", C.c_float), ("shade_ms", C.c_float), ("shadow_ms", C.c_float), ("filter_ms", C.c_float), ("composite_ms", C.c_float)]


assert C.sizeof(GlossyStats) == 64 and GlossyStats.misses.offset == 32 and GlossyStats.trace_ms.offset == 40 and GlossyStats.composite_ms.offset == 56


# volumetric fog of the hybrid frame (an extension; utopian_hip.h "UH_HYBRID_FOG"): the pass behind the sky pass and its two images
HYBRID_FOG = 1 << 19
HYBRID_FOG_MASK, HYBRID_FOG_TERMS = 23, 24


class FogParams(C.Structure):
    """UhFogParams: samples along a pixel's view ray (1..32), the filter's radius (0..4), the extinction per world unit, the march length
    of a sky pixel and cap of a geometry pixel's, the Henyey-Greenstein g, the scale of the sun's in-scattering, the filter's relative
    depth threshold, a reserved word (0), the single-scattering albedo and the unshadowed fog radiance; uh_fog_default_params fills the
    defaults"""

    _fields_ = [("steps", C.c_uint32), ("blur_radius", C.c_uint32), ("density", C.c_float), ("max_distance", C.c_float),
                ("anisotropy", C.c_float), ("intensity", C.c_float), ("blur_depth", C.c_float), ("reserved", C.c_uint32),
                ("albedo", C.c_float * 3), ("ambient", C.c_float * 3)]


assert C.sizeof(FogParams) == 56 and [getattr(FogParams, n).offset for n, _ in FogParams._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 44]


class FogStats(C.Structure):
    """UhFogStats: the last fog pass - the pixels that marched, their rays (pixels * steps), the rays that reached the sun, hipEvent ms of
    classify + walk, of resolve + filter and of the composite"""

    _fields_ = [("pixels", C.c_uint64), ("rays", C.c_uint64), ("lit", C.c_uint64),
                ("trace_ms", C.c_float), ("filter_ms", C.c_float), ("composite_ms", C.c_float), ("reserved", C.c_uint32)]


assert C.sizeof(FogStats) == 40 and FogStats.lit.offset == 16 and FogStats.trace_ms.offset == 24 and FogStats.reserved.offset == 36


# ray-traced glass of the hybrid frame (utopian_hip.h "UH_HYBRID_GLASS"): the pass behind the glossy pass and its three images
HYBRID_GLASS = 1 << 20
HYBRID_GLASS_RADIANCE, HYBRID_GLASS_COUNTS, HYBRID_GLASS_EVENTS = 25, 26, 27


class GlassParams(C.Structure):
    """UhGlassParams: the events of a chain, the first included (1..16), the cap of a chain's radiance and of the pixel's sum, and the
    scale of what the composite writes; uh_glass_default_params fills the defaults"""

    _fields_ = [("max_events", C.c_uint32), ("max_radiance", C.c_float), ("intensity", C.c_float)]


assert C.sizeof(GlassParams) == 12 and [getattr(GlassParams, n).offset for n, _ in GlassParams._fields_] == [0, 4, 8]


class GlassStats(C.Structure):
    """UhGlassStats: the last glass pass - the pixels that cast, the chains cast, the segments walked (chains + events), the events behind
    the first, the events at which refraction was impossible (the first included), the chains cut, the sun rays cast from the ends, the
    chains that missed, hipEvent ms of classify + first event + the rounds' walks, of the rounds' bend kernels, of the sun rays' walk
    and of the composite"""

    _fields_ = [("pixels", C.c_uint64), ("chains", C.c_uint64), ("segments", C.c_uint64), ("events", C.c_uint64), ("tir", C.c_uint64),
                ("cut", C.c_uint64), ("shadow_rays", C.c_uint64), ("misses", C.c_uint64),
                ("trace_ms", C.c_float), ("bend_ms", C.c_float), ("shadow_ms", C.c_float), ("composite_ms", C.c_float)]


assert C.sizeof(GlassStats) == 80 and GlassStats.misses.offset == 56 and GlassStats.trace_ms.offset == 64 and GlassStats.composite_ms.offset == 76


# emissive meshes as area lights of the hybrid frame (an extension; utopian_hip.h "UH_HYBRID_AREA_LIGHTS"): the pass directly behind the
# deferred pass and its three images
HYBRID_AREA_LIGHTS = 1 << 21
HYBRID_AREA_DIFFUSE, HYBRID_AREA_SPECULAR, HYBRID_AREA_COUNTS = 28, 29, 30


class AreaLightParams(C.Structure):
    """UhAreaLightParams: samples per pixel that casts (1..16), the filter's radius (0 none, else 1..6), whether the emitters' own pixels
    are written (0 or 1), the cap of a sample's geometry term over its pdf, the cap of a pixel's two means per channel, the scale of what
    the composite adds, and a tap's normal and plane thresholds; uh_area_light_default_params fills the defaults"""

    _fields_ = [("samples", C.c_uint32), ("blur_radius", C.c_uint32), ("show_emitters", C.c_uint32), ("max_weight", C.c_float),
                ("max_radiance", C.c_float), ("intensity", C.c_float), ("blur_normal_cos", C.c_float), ("blur_plane", C.c_float)]


assert C.sizeof(AreaLightParams) == 32 and [getattr(AreaLightParams, n).offset for n, _ in AreaLightParams._fields_] == list(range(0, 32, 4))


class AreaLightStats(C.Structure):
    """UhAreaLightStats: the last area-light pass - the pixels that cast, their samples, the shadow rays cast, those occluded, the emitter
    pixels, the table's emitter triangles, its total weight and its builds so far, hipEvent ms of the last table build, of classify +
    sampling, of the shadow rays' walk, of the means + filter and of the composite"""

    _fields_ = [("pixels", C.c_uint64), ("samples", C.c_uint64), ("shadow_rays", C.c_uint64), ("occluded", C.c_uint64),
                ("emitter_pixels", C.c_uint64), ("emitters", C.c_uint64), ("total_weight", C.c_uint64), ("table_builds", C.c_uint64),
                ("table_ms", C.c_float), ("sample_ms", C.c_float), ("shadow_ms", C.c_float), ("filter_ms", C.c_float), ("composite_ms", C.c_float),
                ("reserved", C.c_uint32)]


assert C.sizeof(AreaLightStats) == 88 and AreaLightStats.table_builds.offset == 56 and AreaLightStats.table_ms.offset == 64 and \
    AreaLightStats.composite_ms.offset == 80


# motion vectors for moving geometry (an extension; utopian_hip.h "motion vectors"): a modifier of HYBRID_GBUFFER; bit 9 stays unused
HYBRID_MOTION = 1 << 14
HYBRID_MOTION_IMAGE = 15


class MotionStats(C.Structure):
    """UhMotionStats: the last motion pass - geometry pixels with and without a correspondence, the meshes per state, hipEvent ms of the
    motion kernel and of the snapshot behind it"""

    _fields_ = [("pixels_with", C.c_uint32), ("pixels_without", C.c_uint32), ("meshes_static", C.c_uint32), ("meshes_rigid", C.c_uint32),
                ("meshes_deformed", C.c_uint32), ("meshes_none", C.c_uint32), ("motion_ms", C.c_float), ("snapshot_ms", C.c_float)]


assert C.sizeof(MotionStats) == 32 and MotionStats.meshes_static.offset == 8 and MotionStats.meshes_none.offset == 20 and \
    MotionStats.motion_ms.offset == 24 and MotionStats.snapshot_ms.offset == 28


# temporal anti-aliasing of the hybrid frame (an extension; utopian_hip.h "temporal anti-aliasing"): the resolve between the sky pass and
# present, its two images, and the flags of TaaParams; bit 9 stays unused
HYBRID_TAA = 1 << 15
HYBRID_TAA_OUTPUT, HYBRID_TAA_HISTORY = 16, 17
TAA_CLAMP, TAA_MOTION = 1 << 0, 1 << 1


class TaaParams(C.Structure):
    """UhTaaParams: flags (TAA_*), the history cap, the smallest blend factor and the width of the neighbourhood clamp in standard
    deviations; uh_taa_default_params fills the defaults"""

    _fields_ = [("flags", C.c_uint32), ("max_history", C.c_uint32), ("alpha_min", C.c_float), ("clamp_gamma", C.c_float)]


assert C.sizeof(TaaParams) == 16 and TaaParams.max_history.offset == 4 and TaaParams.alpha_min.offset == 8 and TaaParams.clamp_gamma.offset == 12


class TaaStats(C.Structure):
    """UhTaaStats: the last taa pass - the pixels that blended a history, those that started one, hipEvent ms of the pass"""

    _fields_ = [("history_pixels", C.c_uint32), ("reset_pixels", C.c_uint32), ("taa_ms", C.c_float), ("reserved", C.c_uint32)]


assert C.sizeof(TaaStats) == 16 and TaaStats.reset_pixels.offset == 4 and TaaStats.taa_ms.offset == 8 and TaaStats.reserved.offset == 12


# the HDR display chain of the hybrid frame (an extension; utopian_hip.h "HDR display chain"): the pass between the taa pass and present,
# the flags and operators of PostParams and the images of Renderer.read_post; bit 9 stays unused
HYBRID_POST = 1 << 16
POST_AUTO_EXPOSURE, POST_BLOOM = 1 << 0, 1 << 1
TONEMAP_NONE, TONEMAP_REINHARD, TONEMAP_ACES = 0, 1, 2
POST_OUTPUT, POST_BLOOM_DOWN, POST_BLOOM_UP, POST_HISTOGRAM = 0, 1, 2, 3


class PostParams(C.Structure):
    """UhPostParams: flags (POST_*), the operator (TONEMAP_*), the bloom levels asked for, the exposure without metering, the key the
    metered average is mapped to, the exposure clamps, the adaptation rate, the percentiles kept by the meter, the bloom threshold and
    intensity; uh_post_default_params fills the defaults"""

    _fields_ = [("flags", C.c_uint32), ("tonemap", C.c_uint32), ("bloom_levels", C.c_uint32), ("manual_exposure", C.c_float),
                ("key", C.c_float), ("min_exposure", C.c_float), ("max_exposure", C.c_float), ("adaptation", C.c_float),
                ("low_percentile", C.c_float), ("high_percentile", C.c_float), ("bloom_threshold", C.c_float), ("bloom_intensity", C.c_float)]


assert C.sizeof(PostParams) == 48 and [getattr(PostParams, n).offset for n, _ in PostParams._fields_] == list(range(0, 48, 4))


class PostStats(C.Structure):
    """UhPostStats: the last post pass - its exposure, target and metered average luminance, the metered and the bad pixels, the bloom
    levels built, hipEvent ms of the three stages, the passes so far"""

    _fields_ = [("exposure", C.c_float), ("target_exposure", C.c_float), ("average_luminance", C.c_float), ("metered_pixels", C.c_uint32),
                ("bad_pixels", C.c_uint32), ("levels", C.c_uint32), ("meter_ms", C.c_float), ("bloom_ms", C.c_float), ("tonemap_ms", C.c_float),
                ("renders", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(PostStats) == 48 and PostStats.renders.offset == 36 and PostStats.reserved.offset == 40
