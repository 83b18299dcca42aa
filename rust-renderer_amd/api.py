"""Host-side mirror of the reference's plugin surface for the path-tracing + ReSTIR path, over
the C ABI of include/utopian_hip.h (ctypes; no torch types cross the boundary).

Reference verbs mirrored (same names / argument meaning):
  Renderer.add_model / add_light / get_num_lights      utopian/src/renderer.rs:222,391,412
  Renderer.initialize_raytracing                       Raytracing::initialize, utopian/src/raytracing.rs:89
  build_path_tracing_render_graph pass order           utopian/src/renderers/mod.rs:246-358
  FrameLoop (total_samples / prev_frame_projection_view protocol)   prototype/src/main.rs:460-471,545-546
Errors: the reference panics on every failure (graph.rs:253, raytracing.rs:178); here every
non-zero status raises UtopianError carrying uh_last_error().
"""
import ctypes as C
import os

import numpy as np

from . import camera as cam
from .types import (
    ERR_NAMES,
    PASS_ALL,
    RESERVOIR_DTYPE,
    RESTIR_EXCHANGE_FN,
    VERTEX_DTYPE,
    BRDF_LUT_SIZE,
    DENOISE_COLOR,
    DENOISE_HISTORY,
    DENOISE_INPUT,
    DENOISE_OUTPUT,
    DENOISE_TEMPORAL_COLOR,
    DENOISE_VARIANCE,
    DenoiseParams,
    DenoiseStats,
    ENV_BRDF_LUT,
    ENV_ENVIRONMENT,
    ENV_IRRADIANCE,
    ENV_MIPS,
    ENV_SIZE,
    ENV_SPECULAR,
    AreaLightParams,
    AreaLightStats,
    HYBRID_ALBEDO,
    HYBRID_ALL,
    HYBRID_AREA_COUNTS,
    HYBRID_AREA_DIFFUSE,
    HYBRID_AREA_LIGHTS,
    HYBRID_AREA_SPECULAR,
    HYBRID_AO_COUNTS,
    HYBRID_GI_COUNTS,
    HYBRID_GI_RADIANCE,
    HYBRID_FOG_MASK,
    HYBRID_GLASS,
    HYBRID_GLASS_COUNTS,
    HYBRID_GLASS_EVENTS,
    HYBRID_GLASS_RADIANCE,
    HYBRID_FOG_TERMS,
    HYBRID_GLOSSY_BIAS,
    HYBRID_GLOSSY_COUNTS,
    HYBRID_GLOSSY_SCALE,
    HYBRID_DEFERRED_OUTPUT,
    HYBRID_DEPTH,
    HYBRID_GBUFFER_DEPTH,
    HYBRID_GBUFFER_VISIBILITY,
    HYBRID_LIGHT_VISIBILITY,
    HYBRID_MARCHING_CUBES_VISIBILITY,
    HYBRID_MOTION_IMAGE,
    HYBRID_NORMAL,
    HYBRID_POSITION,
    HYBRID_PBR,
    HYBRID_PRESENT_OUTPUT,
    HYBRID_REFLECTIONS,
    HYBRID_SHADOWS,
    HYBRID_SSAO_IMAGE,
    HYBRID_POST,
    HYBRID_TAA,
    HYBRID_TAA_HISTORY,
    HYBRID_TAA_OUTPUT,
    GpuLight,
    GpuMaterial,
    EnvironmentStats,
    HybridFrameStats,
    HybridRestirStats,
    HybridStats,
    GbufferRasterStats,
    IsosurfaceUpdateStats,
    MeshUpdateStats,
    PoseStats,
    MotionStats,
    MarchingCubesStats,
    ShadowmapParams,
    ShadowMapStats,
    FORWARD_DEPTH,
    FORWARD_GRAPH,
    FORWARD_OUTPUT,
    FORWARD_PRESENT_OUTPUT,
    FORWARD_VISIBILITY,
    ForwardStats,
    Reservoir,
    POST_BLOOM_DOWN,
    POST_BLOOM_UP,
    POST_HISTOGRAM,
    POST_OUTPUT,
    PostParams,
    PostStats,
    RestirRows,
    RtaoParams,
    RtaoStats,
    RtgiParams,
    RtgiStats,
    FogParams,
    FogStats,
    GlassParams,
    GlassStats,
    GlossyParams,
    GlossyStats,
    Stats,
    TaaParams,
    TaaStats,
    ViewUniformData,
)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UTOPIAN_HIP_LIB") or os.path.join(_HERE, "libutopian_hip.so")  # UTOPIAN_HIP_LIB: an alternative build of the same library (experiments)


class UtopianError(RuntimeError):
    pass


_p, _int, _u32, _u64, _f32, _vp = C.POINTER, C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p
_fp, _view = _p(_f32), _p(ViewUniformData)
# One row per C entry point this module calls: its name without "uh_", then its argtypes - the restype is c_int - or (argtypes, restype).
# ctypes never compares a row with the C declaration: tests/test_api_signatures.py holds every row to include/utopian_hip.h.
# What every backend exports under a prefix of its own (uh_, uh_mgpu_, the oracle's orc_): CApi binds these
_CONTEXT_VERBS = {
    "destroy": ([_vp], None),
    "add_texture_rgba8": [_vp, _vp, _u32, _u32, _p(_u32)],
    "add_mesh": [_vp, _vp, _u32, _vp, _u32, _p(GpuMaterial), _fp, _p(_u32)],
    "add_light": [_vp, _p(GpuLight), _p(_u32)],
    "set_instance_transform": [_vp, _u32, _fp],
    "build_acceleration": [_vp],
    "refit_acceleration": [_vp],
    "render_frame": [_vp, _view, _u32],
    "render_frames": [_vp, _view, _u32, _u32],
    "reset_accumulation": [_vp],
    "read_accumulation": [_vp, _vp],
    "read_output_bgra8": [_vp, _vp],
    "read_reservoirs": [_vp, _int, _vp],
    "write_reservoirs": [_vp, _int, _vp],
    "write_gbuffer_position": [_vp, _vp],
    "read_gbuffer_position": [_vp, _vp],
    "trace_closest": [_vp, _vp, _u32, _vp, _vp, _vp],
    "trace_any": [_vp, _vp, _u32, _vp],
    "get_stats": [_vp, _p(Stats)],
    "reset_stats": [_vp],
    "set_option": [_vp, C.c_char_p, _int],
    "set_tile_partition": [_vp, _u32, _u32, _u32],
    "set_restir_partition": [_vp, _u32, _u32, _vp, _vp],
    "get_restir_rows": [_vp, _p(RestirRows)],
    "resolve_output": [_vp, _u32, _u32],
    "render_hybrid": [_vp, _view, _u32],
    "read_hybrid": [_vp, _int, _vp],
    "get_hybrid_stats": [_vp, _p(HybridStats)],
    "get_hybrid_frame_stats": [_vp, _p(HybridFrameStats)],
    "read_environment": [_vp, _int, _int, _int, _vp],
    "get_environment_stats": [_vp, _p(EnvironmentStats)],
}
_HYBRID_VERBS = ("render_hybrid", "read_hybrid", "get_hybrid_stats", "get_hybrid_frame_stats", "read_environment", "get_environment_stats")
# The HIP library's alone, under uh_: bound where they are called (_bind)
_LIBRARY_VERBS = {
    "create": [_int, _u32, _u32, _p(_vp)],
    "last_error": ([_vp], C.c_char_p),
    "version": ([], C.c_char_p),
    "hip_versions": [_p(_int), _p(_int)],
    "get_num_lights": [_vp, _p(_u32)],
    "synchronize": [_vp],
    "tile_pack_count": [_vp, _u32, _p(_u64)],
    "pack_tiles": [_vp, _vp, _u64],
    "unpack_tiles": [_vp, _u32, _vp, _u64],
    "compose_tiles": [_vp, _vp, _u64, _u32, _u32],
    "device_pointer": [_vp, _int, _p(_vp)],
    "stream": [_vp, _p(_vp)],
    "add_isosurface_mesh": [_vp, _u32, _f32, _f32, _f32, _p(GpuMaterial), _fp, _p(_u32), _p(_u32)],
    "update_isosurface_mesh": [_vp, _u32, _f32, _p(_u32)],
    "get_isosurface_update_stats": [_vp, _p(IsosurfaceUpdateStats)],
    "update_mesh_vertices": [_vp, _u32, _vp, _u32, _int],
    "get_mesh_update_stats": [_vp, _p(MeshUpdateStats)],
    "set_mesh_skin": [_vp, _u32, _vp, _vp, _u32, _u32],
    "set_mesh_morph_targets": [_vp, _u32, _vp, _vp, _u32, _u32],
    "pose_mesh": [_vp, _u32, _vp, _u32, _vp, _u32],
    "get_pose_stats": [_vp, _p(PoseStats)],
    "isosurface_cells": [_vp, _u32, _f32, _f32, _f32, _vp, _vp],
    "mesh_info": [_vp, _u32, _p(_u32), _p(_u32)],
    "read_mesh": [_vp, _u32, _vp, _vp],
    "get_marching_cubes_stats": [_vp, _p(MarchingCubesStats)],
    "get_gbuffer_raster_stats": [_vp, _p(GbufferRasterStats)],
    "get_hybrid_restir_stats": [_vp, _p(HybridRestirStats)],
    "rtao_default_params": [_p(RtaoParams)],
    "set_rtao_params": [_vp, _p(RtaoParams)],
    "get_rtao_stats": [_vp, _p(RtaoStats)],
    "get_rtao_visits": [_vp, _p(_u64), _p(_u64)],
    "rtgi_default_params": [_p(RtgiParams)],
    "set_rtgi_params": [_vp, _p(RtgiParams)],
    "get_rtgi_stats": [_vp, _p(RtgiStats)],
    "glossy_default_params": [_p(GlossyParams)],
    "set_glossy_params": [_vp, _p(GlossyParams)],
    "get_glossy_stats": [_vp, _p(GlossyStats)],
    "fog_default_params": [_p(FogParams)],
    "set_fog_params": [_vp, _p(FogParams)],
    "get_fog_stats": [_vp, _p(FogStats)],
    "get_fog_visits": [_vp, _p(_u64), _p(_u64)],
    "glass_default_params": [_p(GlassParams)],
    "set_glass_params": [_vp, _p(GlassParams)],
    "get_glass_stats": [_vp, _p(GlassStats)],
    "area_light_default_params": [_p(AreaLightParams)],
    "set_area_light_params": [_vp, _p(AreaLightParams)],
    "get_area_light_stats": [_vp, _p(AreaLightStats)],
    "read_area_emitters": [_vp, _u32, _vp, _vp, _vp, _p(_u32)],
    "get_motion_stats": [_vp, _p(MotionStats)],
    "taa_default_params": [_p(TaaParams)],
    "set_taa_params": [_vp, _p(TaaParams)],
    "reset_taa_history": [_vp],
    "get_taa_stats": [_vp, _p(TaaStats)],
    "taa_jitter": [_u32, _p(_f32 * 2)],
    "post_default_params": [_p(PostParams)],
    "set_post_params": [_vp, _p(PostParams)],
    "reset_post_exposure": [_vp],
    "get_post_stats": [_vp, _p(PostStats)],
    "post_level_size": [_u32, _u32, _u32, _p(_u32), _p(_u32)],
    "post_image": [_vp, _vp],
    "read_post": [_vp, _int, _int, _vp],
    "denoise_default_params": [_p(DenoiseParams)],
    "denoise": [_vp, _view, _p(DenoiseParams)],
    "read_denoised": [_vp, _int, _vp],
    "reset_denoise_history": [_vp],
    "get_denoise_stats": [_vp, _p(DenoiseStats)],
    "shadow_cascades": [_fp, _fp, _f32, _f32, _fp, _p(ShadowmapParams)],
    "set_shadowmap_params": [_vp, _p(ShadowmapParams)],
    "read_shadow_map": [_vp, _int, _vp],
    "get_shadow_map_stats": [_vp, _p(ShadowMapStats)],
    "render_forward": [_vp, _view, _u32],
    "read_forward": [_vp, _int, _vp],
    "get_forward_stats": [_vp, _p(ForwardStats)],
    "rccl_unique_id": [_vp],  # (no context: the id's 128 bytes)
    "rccl_attach": [_vp, _u32, _u32, _vp],
    "rccl_comm_count": [_vp, _p(_u32)],
    "rccl_gather_tiles": [_vp, _u32, _u32, _u32],
    "rccl_detach": [_vp],
    "sun_grid_compare_builders": [_vp, _p(_u64)],
    "check_acceleration": [_vp, _p(_u64)],
    "mgpu_create": [_int, _p(_int), _u32, _u32, _u32, _p(_vp)],
    "mgpu_last_error": ([_vp], C.c_char_p),
    "mgpu_context": ([_vp, _int], _vp),
    "mgpu_num_devices": [_vp],
    "mgpu_get_num_lights": [_vp, _p(_u32)],
    "mgpu_synchronize": [_vp],
    "mgpu_compose": [_vp],
}
_SIGNATURES = {**_CONTEXT_VERBS, **_LIBRARY_VERBS}


def _bind(lib, prefix, name):
    """`prefix + name` of `lib` with the signature of its row: the one place argtypes and restype are set"""
    row = _SIGNATURES[name]
    fn = getattr(lib, prefix + name)
    fn.argtypes, fn.restype = row if isinstance(row, tuple) else (row, _int)
    return fn


class CApi:
    """Typed ctypes view of a library exporting the utopian_hip.h entry points under `prefix`."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        for name in _CONTEXT_VERBS:
            if not hasattr(lib, prefix + name) and (name == "render_frames" or name in _HYBRID_VERBS or prefix == "uh_mgpu_"):
                continue  # the oracle renders frame by frame and has no hybrid passes; the GPU group has no per-context queries
            setattr(self, name, _bind(lib, prefix, name))


_lib_cache = {}


def _preload_hip_runtime():
    """One HIP runtime per process, and by default the one the library was BUILT with: libutopian_hip.so carries a RUNPATH to
    /opt/rocm's lib directory and binds libamdhip64.so.7 there - what a C / C++ / Rust host links. Nothing in a GPU
    process of this package needs torch (the multi-GPU composition is RCCL inside the library, the launcher's rendezvous a TCP socket).
    UH_HIP_RUNTIME=torch is the opt-in for a process that must share the GPU with PyTorch: the wheel bundles its own libamdhip64.so
    (same soname, ROCm 7.0) and, loaded second, would see no devices - so its copy is loaded first, by path, without importing
    torch, and the library binds to it by soname. That is a 7.2-built library on a 7.0 runtime: uh_version() / uh_last_error(NULL)
    say so, and round 4's context-churn soaks corrupted the host heap in that configuration only (profiles/README.md)."""
    import importlib.util

    if os.environ.get("UH_HIP_RUNTIME", "system") != "torch":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library(path=LIB_PATH):
    """Load libutopian_hip.so. Fails loudly if it has not been built: there is no fallback."""
    if path in _lib_cache:
        return _lib_cache[path]
    if not os.path.exists(path):
        raise UtopianError(f"{path} not built - run `python -c 'import __graft_entry__ as g; g.build()'`")
    _preload_hip_runtime()
    lib = C.CDLL(path)
    _lib_cache[path] = lib
    for name in ("create", "last_error", "version", "hip_versions", "get_num_lights", "synchronize", "tile_pack_count", "pack_tiles", "unpack_tiles",
                 "compose_tiles", "device_pointer", "stream"):
        _bind(lib, "uh_", name)
    return lib


def hip_versions():
    """(built_with, runtime) as 'major.minor.patch' strings: the HIP release that compiled libutopian_hip.so and the one this
    process runs it on (uh_hip_versions); they differ when another libamdhip64.so.7 was loaded first (UH_HIP_RUNTIME=torch)"""
    lib = load_library()
    b, r = C.c_int(0), C.c_int(0)
    lib.uh_hip_versions(C.byref(b), C.byref(r))
    fmt = lambda v: f"{v // 10000000}.{v // 100000 % 100}.{v % 100000}"
    return fmt(b.value), fmt(r.value)


def identity3x4():
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)


def transform3x4(scale=(1, 1, 1), translation=(0, 0, 0), rotation=None):
    """row-major 3x4 from scale / rotation(3x3) / translation: the recomposed
    VkTransformMatrixKHR of Raytracing::fill_instance_array (raytracing.rs:229-248)."""
    r = np.eye(3, dtype=np.float32) if rotation is None else np.asarray(rotation, dtype=np.float32)
    m = np.zeros((3, 4), dtype=np.float32)
    m[:, :3] = r * np.asarray(scale, dtype=np.float32)[None, :]
    m[:, 3] = np.asarray(translation, dtype=np.float32)
    return m.reshape(12)


def make_material(material_type=0, material_property=0.0, base_color=(1, 1, 1, 1), diffuse_map=0, metallic=1.0, roughness=1.0):
    """GpuMaterial as Renderer::add_model fills it (renderer.rs:266-281)."""
    m = GpuMaterial()
    m.diffuse_map = diffuse_map
    m.base_color_factor[:] = [float(x) for x in base_color]
    m.metallic_factor, m.roughness_factor = metallic, roughness
    m.raytrace_properties[:] = [float(material_type), float(material_property), 0.0, 0.0]
    return m


def make_light(position, color=(1, 1, 1), range_=1.0, intensity=(1, 1, 1)):
    """GpuLight as Renderer::add_light fills it (renderer.rs:391-404)."""
    l = GpuLight()
    l.color[:] = [color[0], color[1], color[2], 0.0]
    l.position[:] = [float(x) for x in position]
    l.range = range_
    l.attenuation[:] = [0.0, 0.0, 0.1]
    l.light_type = 1.0
    l.intensity[:] = [float(x) for x in intensity]
    return l


class Renderer:
    """utopian::Renderer + Raytracing + the path-tracing graph resources, on one GPU.

    `_api`/`_ctx_factory` let the test-only oracle binding reuse this class over liboracle.so
    (oracle/oracle_api.py); the product never passes them.
    """

    backend = "hip"

    def __init__(self, width, height, device=0, _api=None, _ctx_factory=None):
        self.width, self.height = int(width), int(height)
        if _api is None:
            lib = load_library()
            self._lib = lib
            ctx = C.c_void_p()
            st = lib.uh_create(int(device), self.width, self.height, C.byref(ctx))
            if st != 0:
                msg = lib.uh_last_error(None)
                raise UtopianError(f"uh_create failed: {ERR_NAMES.get(st, st)}: {msg.decode() if msg else ''}")
            self._ctx, self._api = ctx, CApi(lib, "uh_")
        else:
            self._lib, self._api, self._ctx = _api.lib, _api, _ctx_factory(self.width, self.height)
        self._keep = []

    # -- helpers --------------------------------------------------------------------------
    def _check(self, st):
        if st != 0:
            msg = b""
            if self.backend == "hip":
                msg = self._lib.uh_last_error(self._ctx) or b""
            raise UtopianError(f"{ERR_NAMES.get(st, st)}: {msg.decode()}")

    def _uh(self, name):
        """uh_<name> of the HIP library, bound from the table"""
        return _bind(self._lib, "uh_", name)

    def _hip_only(self, what, name=None, present=True):
        """The guard of the verbs that only the HIP library has: NotImplementedError naming `what` ("<a pass> is a per-context verb") on
        another backend, or where such a verb is not `present`; else uh_<name>, bound."""
        if self.backend != "hip" or not present:
            raise NotImplementedError(f"{what} of the HIP library; backend {self.backend!r} has none")
        return name and self._uh(name)

    def _stats(self, Struct, fn):
        """a `Struct` as the stats verb `fn` fills it"""
        s = Struct()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    def _set_params(self, Struct, fn, defaults, params, fields):
        """the params verb `fn` on a copy of `params` (of `defaults()` when None) with `fields` set; returns the copy"""
        p = Struct.from_buffer_copy(defaults() if params is None else params)
        for k, v in fields.items():
            if not hasattr(p, k):
                raise TypeError(f"{Struct.__name__} has no field {k!r}")
            setattr(p, k, v)
        self._check(fn(self._ctx, C.byref(p)))
        return p

    def _read_image(self, images, fn, which, refusal):
        """image `which` of `images` ({index: (dtype, channels)}) by the read verb `fn`; ValueError(refusal) for an index not in it"""
        if which not in images:
            raise ValueError(refusal)
        dtype, ch = images[which]
        out = np.empty((self.height, self.width, ch) if ch > 1 else (self.height, self.width), dtype=dtype)
        self._check(fn(self._ctx, int(which), out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_ctx", None):
            self._api.destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- scene (Renderer::add_model / add_light) ------------------------------------------
    def add_texture(self, rgba):
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        assert rgba.ndim == 3 and rgba.shape[2] == 4
        out = C.c_uint32()
        self._check(self._api.add_texture_rgba8(self._ctx, rgba.ctypes.data, rgba.shape[1], rgba.shape[0], C.byref(out)))
        return out.value

    def add_mesh(self, vertices, indices, material, world3x4=None):
        vertices = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        w = identity3x4() if world3x4 is None else np.ascontiguousarray(world3x4, dtype=np.float32).reshape(12)
        out = C.c_uint32()
        self._check(
            self._api.add_mesh(
                self._ctx, vertices.ctypes.data, len(vertices), indices.ctypes.data, len(indices), C.byref(material),
                w.ctypes.data_as(C.POINTER(C.c_float)), C.byref(out),
            )
        )
        return out.value

    def initialize(self, default_textures=None):
        """Renderer::initialize (renderer.rs:202-220): the four default maps get bindless indices 0..3 - diffuse (white),
        normal (flat), occlusion (white), metallic-roughness - before any model texture. `default_textures`: four
        (H, W, 4) uint8 arrays (the files of utopian/data/textures/defaults/); without them 1x1 texels of the same
        values are used (the files are constant images except for +-2 LSB dither in the normal map)."""
        if hasattr(self, "_defaults"):
            return self._defaults
        if default_textures is None:
            texel = lambda *rgba: np.array(rgba, dtype=np.uint8).reshape(1, 1, 4)
            default_textures = [texel(255, 255, 255, 255), texel(127, 127, 255, 255), texel(255, 255, 255, 255), texel(0, 255, 0, 255)]
        diffuse, normal, occlusion, mr = (self.add_texture(t) for t in default_textures)
        self._defaults = dict(diffuse=diffuse, normal=normal, occlusion=occlusion, metallic_roughness=mr)
        self._default_diffuse = diffuse
        return self._defaults

    def add_model(self, model, transform=None):
        """model: scenes.Model (textures + meshes). Texture indices are remapped to bindless indices exactly like
        Renderer::add_model does (renderer.rs:222-262): a map that is DEFAULT_TEXTURE_MAP (None here) takes the
        renderer's default of its kind, every other one is a fresh bindless texture."""
        tex_map = {}
        mesh_ids = []
        defaults = getattr(self, "_defaults", None)
        for mesh in model.meshes:
            mat = mesh.material_struct()
            if defaults:  # the reference assigns all four maps; the path tracer reads diffuse_map only (rchit:40)
                mat.normal_map, mat.metallic_roughness_map, mat.occlusion_map = defaults["normal"], defaults["metallic_roughness"], defaults["occlusion"]
            if mesh.texture is not None:
                if mesh.texture not in tex_map:
                    tex_map[mesh.texture] = self.add_texture(model.textures[mesh.texture])
                mat.diffuse_map = tex_map[mesh.texture]
            else:
                mat.diffuse_map = self.default_diffuse_map()
            w = mesh.transform if transform is None else compose3x4(transform, mesh.transform)
            mesh_ids.append(self.add_mesh(mesh.vertices, mesh.indices, mat, w))
            if self.backend == "hip":  # a rigged primitive of a glTF (gltf.Animator poses it): the other backends draw the bind pose
                if getattr(mesh, "skin", None) is not None:
                    self.set_mesh_skin(mesh_ids[-1], mesh.joints, mesh.weights, len(model.skins[mesh.skin].joints))
                if getattr(mesh, "morph_positions", None) is not None:
                    self.set_mesh_morph_targets(mesh_ids[-1], mesh.morph_positions, mesh.morph_normals)
        return mesh_ids

    def add_isosurface_mesh(self, resolution, lo, hi, time=0.0, material=None, world3x4=None):
        """uh_add_isosurface_mesh: the reference's marching-cubes density field, extracted on the GPU.
        Returns (mesh index or None, triangle count)."""
        if material is None:
            material = make_material(base_color=(0.8, 0.8, 0.8, 1.0), diffuse_map=self.default_diffuse_map())
        w = identity3x4() if world3x4 is None else np.ascontiguousarray(world3x4, dtype=np.float32).reshape(12)
        mesh, tris = C.c_uint32(), C.c_uint32()
        self._check(self._uh("add_isosurface_mesh")(self._ctx, int(resolution), float(lo), float(hi), float(time), C.byref(material), w.ctypes.data_as(C.POINTER(C.c_float)), C.byref(mesh), C.byref(tris)))
        return (None if mesh.value == 0xFFFFFFFF else mesh.value), tris.value

    def update_isosurface_mesh(self, mesh, time):
        """uh_update_isosurface_mesh: re-extracts the field at `time` with the parameters mesh `mesh` was created with by
        add_isosurface_mesh and makes the result its geometry, on the device. Returns the triangle count; the context needs
        build_acceleration afterwards."""
        tris = C.c_uint32()
        self._check(self._uh("update_isosurface_mesh")(self._ctx, int(mesh), float(time), C.byref(tris)))
        return tris.value

    def isosurface_update_stats(self):
        """UhIsosurfaceUpdateStats (all zero before the first update_isosurface_mesh)"""
        return self._stats(IsosurfaceUpdateStats, self._uh("get_isosurface_update_stats"))

    def update_mesh_vertices(self, mesh, vertices=None, *, device_ptr=None, count=None):
        """uh_update_mesh_vertices: new vertices for a mesh of add_mesh, its index list kept. Host input: `vertices`, a VERTEX_DTYPE
        array of the mesh's length. Device input: `device_ptr`, the address of `count` vertex records on the renderer's device, which
        the caller has finished writing. refit_acceleration (or a frame with view.rebuild_tlas = 1) or build_acceleration follows."""
        fn = self._uh("update_mesh_vertices")
        if device_ptr is not None:
            assert vertices is None and count is not None, "device input: device_ptr= with count="
            self._check(fn(self._ctx, int(mesh), C.c_void_p(int(device_ptr)), int(count), 1))
            return
        vertices = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        self._check(fn(self._ctx, int(mesh), C.c_void_p(vertices.ctypes.data if len(vertices) else None), len(vertices), 0))

    def mesh_update_stats(self):
        """UhMeshUpdateStats (all zero before the first update_mesh_vertices)"""
        return self._stats(MeshUpdateStats, self._uh("get_mesh_update_stats"))

    def set_mesh_skin(self, mesh, joints, weights, num_joints):
        """uh_set_mesh_skin: `joints` (N, 4) uint16 and `weights` (N, 4) float32 for the N vertices of a mesh of add_mesh, over
        `num_joints` joints; the mesh's current vertices become the bind pose. The geometry does not change."""
        joints = np.ascontiguousarray(joints, dtype=np.uint16)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if joints.ndim != 2 or joints.shape[1] != 4 or weights.shape != joints.shape:
            raise ValueError("joints and weights are (N, 4) arrays")
        self._check(self._uh("set_mesh_skin")(self._ctx, int(mesh), joints.ctypes.data, weights.ctypes.data, len(joints), int(num_joints)))

    def set_mesh_morph_targets(self, mesh, position_deltas, normal_deltas=None):
        """uh_set_mesh_morph_targets: `position_deltas` (T, N, 3) float32 and, optionally, `normal_deltas` of the same shape for the N
        vertices of a mesh of add_mesh; the mesh's current vertices become the bind pose. The geometry does not change."""
        dp = np.ascontiguousarray(position_deltas, dtype=np.float32)
        dn = None if normal_deltas is None else np.ascontiguousarray(normal_deltas, dtype=np.float32)
        if dp.ndim != 3 or dp.shape[2] != 3 or (dn is not None and dn.shape != dp.shape):
            raise ValueError("deltas are (T, N, 3) arrays of one shape")
        self._check(self._uh("set_mesh_morph_targets")(self._ctx, int(mesh), dp.ctypes.data, None if dn is None else dn.ctypes.data, dp.shape[1], dp.shape[0]))

    def pose_mesh(self, mesh, joint_matrices=None, morph_weights=None):
        """uh_pose_mesh: the mesh's vertices from its bind pose, on the device. `joint_matrices`: (J, 12) or (J, 3, 4) float32, row-major
        3x4 per joint of the skin; `morph_weights`: (T,) float32; None for a part the mesh does not have. refit_acceleration (or a frame
        with view.rebuild_tlas = 1) or build_acceleration follows, as after update_mesh_vertices."""
        jm = None if joint_matrices is None else np.ascontiguousarray(joint_matrices, dtype=np.float32).reshape(-1, 12)
        mw = None if morph_weights is None else np.ascontiguousarray(morph_weights, dtype=np.float32).reshape(-1)
        self._check(self._uh("pose_mesh")(self._ctx, int(mesh), None if jm is None else jm.ctypes.data, 0 if jm is None else len(jm),
                                          None if mw is None else mw.ctypes.data, 0 if mw is None else len(mw)))

    def pose_stats(self):
        """UhPoseStats (all zero before the first pose_mesh)"""
        return self._stats(PoseStats, self._uh("get_pose_stats"))

    def isosurface_cells(self, resolution, lo, hi, time=0.0):
        """uh_isosurface_cells: per cell of the extraction grid (x fastest) its marching-cubes case index and the triangles it keeps"""
        n = int(resolution) ** 3
        cube, kept = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self._uh("isosurface_cells")(self._ctx, int(resolution), float(lo), float(hi), float(time), cube.ctypes.data, kept.ctypes.data))
        return cube, kept

    def read_mesh(self, mesh_index):
        """the context's host copy of a mesh: (vertices as VERTEX_DTYPE, indices)"""
        nv, ni = C.c_uint32(), C.c_uint32()
        self._check(self._uh("mesh_info")(self._ctx, mesh_index, C.byref(nv), C.byref(ni)))
        v = np.zeros(nv.value, dtype=VERTEX_DTYPE)
        idx = np.zeros(ni.value, dtype=np.uint32)
        self._check(self._uh("read_mesh")(self._ctx, mesh_index, v.ctypes.data, idx.ctypes.data))
        return v, idx

    def default_diffuse_map(self):
        """Renderer::initialize's default_diffuse_map (renderer.rs:202-220): a white texel."""
        if not hasattr(self, "_default_diffuse"):
            self._default_diffuse = self.add_texture(np.full((1, 1, 4), 255, dtype=np.uint8))
        return self._default_diffuse

    def add_light(self, position, color=(1, 1, 1), range_=1.0):
        out = C.c_uint32()
        l = make_light(position, color, range_)
        self._check(self._api.add_light(self._ctx, C.byref(l), C.byref(out)))
        return out.value

    def add_gpu_light(self, light):
        out = C.c_uint32()
        self._check(self._api.add_light(self._ctx, C.byref(light), C.byref(out)))
        return out.value

    def get_num_lights(self):
        if self.backend == "hip":
            out = C.c_uint32()
            self._check(self._lib.uh_get_num_lights(self._ctx, C.byref(out)))
            return out.value
        return self._num_lights

    def set_instance_transform(self, mesh_index, world3x4):
        w = np.ascontiguousarray(world3x4, dtype=np.float32).reshape(12)
        self._check(self._api.set_instance_transform(self._ctx, mesh_index, w.ctypes.data_as(C.POINTER(C.c_float))))

    def initialize_raytracing(self):
        """Raytracing::initialize (raytracing.rs:89): build the acceleration structure."""
        self._check(self._api.build_acceleration(self._ctx))

    build_acceleration = initialize_raytracing

    def rebuild_tlas(self):
        """Raytracing::rebuild_tlas (raytracing.rs:400): on-device refit after set_instance_transform."""
        self._check(self._api.refit_acceleration(self._ctx))

    refit_acceleration = rebuild_tlas

    # -- per frame ------------------------------------------------------------------------
    def render_frame(self, view, pass_mask=PASS_ALL):
        self._check(self._api.render_frame(self._ctx, C.byref(view), pass_mask))

    def render_frames(self, view, pass_mask, count):
        """`count` consecutive path-tracing frames of a static camera (uh_render_frames)."""
        self._check(self._api.render_frames(self._ctx, C.byref(view), pass_mask, count))

    def reset_accumulation(self):
        self._check(self._api.reset_accumulation(self._ctx))

    def synchronize(self):
        if self.backend == "hip":
            self._check(self._lib.uh_synchronize(self._ctx))

    # -- read-back ------------------------------------------------------------------------
    def read_accumulation(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._api.read_accumulation(self._ctx, out.ctypes.data))
        return out

    def read_output_bgra8(self):
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        self._check(self._api.read_output_bgra8(self._ctx, out.ctypes.data))
        return out

    def read_reservoirs(self, which):
        out = np.empty((self.height, self.width), dtype=RESERVOIR_DTYPE)
        self._check(self._api.read_reservoirs(self._ctx, which, out.ctypes.data))
        return out

    def write_reservoirs(self, which, data):
        data = np.ascontiguousarray(data, dtype=RESERVOIR_DTYPE)
        assert data.size == self.width * self.height
        self._check(self._api.write_reservoirs(self._ctx, which, data.ctypes.data))

    def write_gbuffer_position(self, rgba32f):
        """uh_write_gbuffer_position: frames rendered without PASS_GBUFFER read these positions (known-answer tests)"""
        data = np.ascontiguousarray(rgba32f, dtype=np.float32)
        assert data.size == self.width * self.height * 4
        self._check(self._api.write_gbuffer_position(self._ctx, data.ctypes.data))

    def read_gbuffer_position(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._api.read_gbuffer_position(self._ctx, out.ctypes.data))
        return out

    # -- the hybrid graph's ray-traced passes (uh_render_hybrid; include/utopian_hip.h) ----
    def _hybrid_api(self):
        self._hip_only("the hybrid passes (rt_shadows / rt_reflections / the final frame) are per-context verbs", present=hasattr(self._api, "render_hybrid"))
        return self._api

    def _hybrid_verb(self, name):
        """uh_<name>, a verb of the hybrid graph that CApi does not carry"""
        self._hybrid_api()
        return self._uh(name)

    def render_hybrid(self, view, mask=HYBRID_ALL):
        """rt_shadows (previous G-buffer), gbuffer, rt_reflections (this one), ssao, deferred, sky, present - the reference's pass order -
        for the bits of `mask` (HYBRID_FRAME: all seven)"""
        api = self._hybrid_api()
        self._check(api.render_hybrid(self._ctx, C.byref(view), int(mask)))
        if int(mask) & HYBRID_TAA:
            self._taa_rendered = True
        if int(mask) & HYBRID_GLASS:
            self._glass_rendered = True
        if int(mask) & HYBRID_AREA_LIGHTS:
            self._area_rendered = True

    _HYBRID_IMAGES = {
        HYBRID_POSITION: (np.float32, 4),
        HYBRID_NORMAL: (np.float32, 4),
        HYBRID_ALBEDO: (np.uint8, 4),
        HYBRID_PBR: (np.float32, 4),
        HYBRID_SHADOWS: (np.uint8, 1),
        HYBRID_REFLECTIONS: (np.uint8, 4),
        HYBRID_SSAO_IMAGE: (np.uint16, 1),
        HYBRID_DEFERRED_OUTPUT: (np.float32, 4),
        HYBRID_PRESENT_OUTPUT: (np.uint8, 4),
        HYBRID_DEPTH: (np.float32, 1),
        HYBRID_MARCHING_CUBES_VISIBILITY: (np.uint32, 1),
        HYBRID_GBUFFER_DEPTH: (np.float32, 1),
        HYBRID_GBUFFER_VISIBILITY: (np.uint32, 1),
        HYBRID_LIGHT_VISIBILITY: (np.uint8, 1),
        HYBRID_AO_COUNTS: (np.uint8, 1),
        HYBRID_MOTION_IMAGE: (np.float32, 4),
    }
    # the two images of HYBRID_TAA, which exist once a render_hybrid call with the bit has succeeded on this renderer (_taa_rendered)
    _TAA_IMAGES = {HYBRID_TAA_OUTPUT: (np.float32, 4), HYBRID_TAA_HISTORY: (np.float32, 1)}
    _taa_rendered = False
    # the two images of HYBRID_RTGI: the library refuses them before the first rtgi pass
    _GI_IMAGES = {HYBRID_GI_RADIANCE: (np.float32, 4), HYBRID_GI_COUNTS: (np.uint8, 4)}
    # the three images of HYBRID_GLOSSY: the library refuses them before the first glossy pass
    _GLOSSY_IMAGES = {HYBRID_GLOSSY_SCALE: (np.float32, 4), HYBRID_GLOSSY_BIAS: (np.float32, 4), HYBRID_GLOSSY_COUNTS: (np.uint8, 4)}
    # the two images of HYBRID_FOG: the library refuses them before the first fog pass
    _FOG_IMAGES = {HYBRID_FOG_MASK: (np.uint32, 1), HYBRID_FOG_TERMS: (np.float32, 4)}
    # the three images of HYBRID_GLASS, which exist once a render_hybrid call with the bit has succeeded on this renderer (_glass_rendered)
    _GLASS_IMAGES = {HYBRID_GLASS_RADIANCE: (np.float32, 4), HYBRID_GLASS_COUNTS: (np.uint8, 4), HYBRID_GLASS_EVENTS: (np.uint8, 4)}
    _glass_rendered = False
    # the three images of HYBRID_AREA_LIGHTS, which exist once a render_hybrid call with the bit has succeeded on this renderer (_area_rendered)
    _AREA_IMAGES = {HYBRID_AREA_DIFFUSE: (np.float32, 4), HYBRID_AREA_SPECULAR: (np.float32, 4), HYBRID_AREA_COUNTS: (np.uint8, 4)}
    _area_rendered = False

    def read_hybrid(self, which):
        """one image of the hybrid graph: (H, W, 4) float32 position / normal / pbr / deferred output, (H, W, 4) uint8 albedo / reflections /
        present output (B, G, R, A), (H, W) uint8 shadows, (H, W) uint16 SSAO, (H, W) float32 marching-cubes depth buffer, (H, W) uint32
        marching-cubes draw index (MARCHING_CUBES_NONE where none survived), (H, W) float32 rasterised G-buffer depth, (H, W) uint32
        rasterised G-buffer draw index (GBUFFER_NONE where none survived), (H, W) uint8 light visibility of HYBRID_RESTIR_LIGHTS,
        (H, W) uint8 occluded-ray counts of HYBRID_RTAO, (H, W, 4) float32 motion image of HYBRID_MOTION (previous world position, w = 1
        with a correspondence), once a call with HYBRID_TAA has run (H, W, 4) float32 taa_output and (H, W) float32 history length, and of
        HYBRID_RTGI (H, W, 4) float32 filtered incoming radiance (w = 1 where the pixel cast) and (H, W, 4) uint8 ray counts (sunlit, dark,
        emitter, missed), and of HYBRID_GLOSSY (H, W, 4) float32 filtered scale and bias sums (w = 1 where the pixel cast) and (H, W, 4) uint8
        ray counts (sunlit, dark, emitter, missed), and of HYBRID_FOG (H, W) uint32 masks (bit k: sample k saw the sun) and (H, W, 4) float32
        terms (a, Ttot, F, Ff; all 0 where the pixel did not march), and once a call with HYBRID_GLASS has run (H, W, 4) float32 glass
        radiance (C, 1 where the pixel cast), (H, W, 4) uint8 chain counts (sunlit, dark, emitter, missed) and (H, W, 4) uint8 events (chain 0,
        chain 1, flags, 0), and once a call with HYBRID_AREA_LIGHTS has run (H, W, 4) float32 filtered diffuse and specular means of the
        area lights (w = 1 where the pixel cast) and (H, W, 4) uint8 sample counts (lit, occluded, away, 0)"""
        images = {**self._HYBRID_IMAGES, **(self._TAA_IMAGES if self._taa_rendered else {}), **self._GI_IMAGES, **self._GLOSSY_IMAGES,
                  **self._FOG_IMAGES, **(self._GLASS_IMAGES if self._glass_rendered else {}), **(self._AREA_IMAGES if self._area_rendered else {})}
        return self._read_image(images, self._hybrid_api().read_hybrid, which,
                                f"hybrid image index {which} (0..15, 18..24, 16..17 once a render_hybrid call with HYBRID_TAA has run, "
                                f"25..27 once one with HYBRID_GLASS has and 28..30 once one with HYBRID_AREA_LIGHTS has)")

    def hybrid_stats(self):
        return self._stats(HybridStats, self._hybrid_api().get_hybrid_stats)

    def read_environment(self, which, face=0, mip=0):
        """one face and mip of an IBL map (ENV_ENVIRONMENT / ENV_IRRADIANCE / ENV_SPECULAR: (S, S, 4) float32, S = 512 >> mip, row 0
        first) or the BRDF LUT (ENV_BRDF_LUT, face 0, mip 0: (512, 512, 2) float16, R and G)"""
        api = self._hybrid_api()
        if which == ENV_BRDF_LUT:
            out = np.empty((BRDF_LUT_SIZE, BRDF_LUT_SIZE, 2), dtype=np.float16)
        elif which in (ENV_ENVIRONMENT, ENV_IRRADIANCE, ENV_SPECULAR) and 0 <= mip < ENV_MIPS:
            s = ENV_SIZE >> mip
            out = np.empty((s, s, 4), dtype=np.float32)
        else:
            raise ValueError(f"environment map {which} (0..3), mip {mip} (0..7)")
        self._check(api.read_environment(self._ctx, int(which), int(face), int(mip), out.ctypes.data))
        return out

    def environment_stats(self):
        """UhEnvironmentStats of the last HYBRID_ENVIRONMENT build: pass_ms of its four sub-passes, builds, sun_dir and eye"""
        return self._stats(EnvironmentStats, self._hybrid_api().get_environment_stats)

    def hybrid_frame_stats(self):
        """UhHybridFrameStats of the last render_hybrid call: pass_ms of all seven passes in bit order"""
        return self._stats(HybridFrameStats, self._hybrid_api().get_hybrid_frame_stats)

    def marching_cubes_stats(self):
        """UhMarchingCubesStats of the last HYBRID_MARCHING_CUBES pass"""
        return self._stats(MarchingCubesStats, self._hybrid_verb("get_marching_cubes_stats"))

    def gbuffer_raster_stats(self):
        """UhGbufferRasterStats of the last rasterised G-buffer pass (HYBRID_GBUFFER | HYBRID_GBUFFER_RASTER)"""
        return self._stats(GbufferRasterStats, self._hybrid_verb("get_gbuffer_raster_stats"))

    def hybrid_restir_stats(self):
        """UhHybridRestirStats of the last render_hybrid call with HYBRID_RESTIR_LIGHTS: rays, occluded, pass_ms"""
        return self._stats(HybridRestirStats, self._hybrid_verb("get_hybrid_restir_stats"))

    # -- ray-traced ambient occlusion (HYBRID_RTAO; include/utopian_hip.h "UH_HYBRID_RTAO") ---
    _RTAO = "ray-traced ambient occlusion is a per-context verb"

    def set_rtao_params(self, params=None, **fields):
        """uh_set_rtao_params: `params` (an RtaoParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_RTAO that follow. A refused call raises and leaves the old ones."""
        return self._set_params(RtaoParams, self._hip_only(self._RTAO, "set_rtao_params"), rtao_default_params, params, fields)

    def rtao_stats(self):
        """UhRtaoStats of the last rtao pass: pixels, rays, occluded, trace_ms, filter_ms"""
        return self._stats(RtaoStats, self._hip_only(self._RTAO, "get_rtao_stats"))

    # -- one-bounce ray-traced diffuse GI (HYBRID_RTGI; include/utopian_hip.h "UH_HYBRID_RTGI") ---
    _RTGI = "ray-traced diffuse GI is a per-context verb"

    def set_rtgi_params(self, params=None, **fields):
        """uh_set_rtgi_params: `params` (an RtgiParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_RTGI that follow. A refused call raises and leaves the old ones."""
        return self._set_params(RtgiParams, self._hip_only(self._RTGI, "set_rtgi_params"), rtgi_default_params, params, fields)

    def rtgi_stats(self):
        """UhRtgiStats of the last rtgi pass: pixels, rays, shadow_rays, misses, trace_ms, shadow_ms, filter_ms, composite_ms"""
        return self._stats(RtgiStats, self._hip_only(self._RTGI, "get_rtgi_stats"))

    # -- ray-traced glossy reflections (HYBRID_GLOSSY; include/utopian_hip.h "UH_HYBRID_GLOSSY") ---
    _GLOSSY = "ray-traced glossy reflections are a per-context verb"

    def set_glossy_params(self, params=None, **fields):
        """uh_set_glossy_params: `params` (a GlossyParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_GLOSSY that follow. A refused call raises and leaves the old ones."""
        return self._set_params(GlossyParams, self._hip_only(self._GLOSSY, "set_glossy_params"), glossy_default_params, params, fields)

    def glossy_stats(self):
        """UhGlossyStats of the last glossy pass: pixels, rays, below, shadow_rays, misses, trace_ms, shade_ms, shadow_ms, filter_ms, composite_ms"""
        return self._stats(GlossyStats, self._hip_only(self._GLOSSY, "get_glossy_stats"))

    # -- ray-traced glass (HYBRID_GLASS; include/utopian_hip.h "UH_HYBRID_GLASS") ---
    _GLASS = "ray-traced glass is a per-context verb"

    def set_glass_params(self, params=None, **fields):
        """uh_set_glass_params: `params` (a GlassParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_GLASS that follow. A refused call raises and leaves the old ones."""
        return self._set_params(GlassParams, self._hip_only(self._GLASS, "set_glass_params"), glass_default_params, params, fields)

    def glass_stats(self):
        """UhGlassStats of the last glass pass: pixels, chains, segments, events, tir, cut, shadow_rays, misses, trace_ms, bend_ms, shadow_ms,
        composite_ms"""
        return self._stats(GlassStats, self._hip_only(self._GLASS, "get_glass_stats"))

    # -- emissive meshes as area lights (HYBRID_AREA_LIGHTS; include/utopian_hip.h "UH_HYBRID_AREA_LIGHTS") ---
    _AREA = "area lights are a per-context verb"

    def set_area_light_params(self, params=None, **fields):
        """uh_set_area_light_params: `params` (an AreaLightParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_AREA_LIGHTS that follow. A refused call raises and leaves the old ones."""
        return self._set_params(AreaLightParams, self._hip_only(self._AREA, "set_area_light_params"), area_light_default_params, params, fields)

    def area_light_stats(self):
        """UhAreaLightStats of the last area-light pass: pixels, samples, shadow_rays, occluded, emitter_pixels, emitters, total_weight,
        table_builds, table_ms, sample_ms, shadow_ms, filter_ms, composite_ms"""
        return self._stats(AreaLightStats, self._hip_only(self._AREA, "get_area_light_stats"))

    def read_area_emitters(self):
        """uh_read_area_emitters: the emitter table of the last area-light pass in slot order - keys (N,) uint32 (mesh << 22 | prim),
        areas (N,) float32 and weights (N,) uint32"""
        read = self._hip_only(self._AREA, "read_area_emitters")
        n = C.c_uint32()
        self._check(read(self._ctx, 0, None, None, None, C.byref(n)))
        keys, areas, weights = np.zeros(n.value, np.uint32), np.zeros(n.value, np.float32), np.zeros(n.value, np.uint32)
        if n.value:
            self._check(read(self._ctx, n.value, keys.ctypes.data, areas.ctypes.data, weights.ctypes.data, C.byref(n)))
        return keys, areas, weights

    # -- volumetric fog (HYBRID_FOG; include/utopian_hip.h "UH_HYBRID_FOG") ---
    _FOG = "volumetric fog is a per-context verb"

    def set_fog_params(self, params=None, **fields):
        """uh_set_fog_params: `params` (a FogParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_FOG that follow. A refused call raises and leaves the old ones."""
        return self._set_params(FogParams, self._hip_only(self._FOG, "set_fog_params"), fog_default_params, params, fields)

    def fog_stats(self):
        """UhFogStats of the last fog pass: pixels, rays, lit, trace_ms, filter_ms, composite_ms"""
        return self._stats(FogStats, self._hip_only(self._FOG, "get_fog_stats"))

    def fog_visits(self):
        """(node visits, triangle tests) of the last fog pass's walks, counted while option "count_visits" is 1; else (0, 0)"""
        fn = self._hip_only(self._FOG, "get_fog_visits")
        nodes, tris = C.c_uint64(), C.c_uint64()
        self._check(fn(self._ctx, C.byref(nodes), C.byref(tris)))
        return nodes.value, tris.value

    def rtao_visits(self):
        """(node visits, triangle tests) of the last rtao pass's walks, counted while option "count_visits" is 1; else (0, 0)"""
        fn = self._hip_only(self._RTAO, "get_rtao_visits")
        nodes, tris = C.c_uint64(), C.c_uint64()
        self._check(fn(self._ctx, C.byref(nodes), C.byref(tris)))
        return nodes.value, tris.value

    # -- motion vectors (HYBRID_GBUFFER | HYBRID_MOTION; include/utopian_hip.h "motion vectors") ---
    def motion_stats(self):
        """UhMotionStats of the last motion pass: pixels_with / pixels_without a correspondence, meshes_static / _rigid / _deformed /
        _none, motion_ms, snapshot_ms; all zero before the first pass"""
        return self._stats(MotionStats, self._hip_only("motion vectors are a per-context verb", "get_motion_stats"))

    # -- temporal anti-aliasing (HYBRID_TAA; include/utopian_hip.h "temporal anti-aliasing") ---
    _TAA = "temporal anti-aliasing is a per-context verb"

    @staticmethod
    def taa_default_params():
        """UhTaaParams as uh_taa_default_params fills it: TAA_CLAMP, 16, 0.1, 1.0"""
        return taa_default_params()

    def set_taa_params(self, params=None, **fields):
        """uh_set_taa_params: `params` (a TaaParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_TAA that follow. A refused call raises and leaves the old ones."""
        return self._set_params(TaaParams, self._hip_only(self._TAA, "set_taa_params"), taa_default_params, params, fields)

    def reset_taa_history(self):
        """uh_reset_taa_history: the next taa pass starts from no history (a camera cut)"""
        self._check(self._hip_only(self._TAA, "reset_taa_history")(self._ctx))

    def taa_stats(self):
        """UhTaaStats of the last taa pass: history_pixels, reset_pixels, taa_ms; all zero before the first pass"""
        return self._stats(TaaStats, self._hip_only(self._TAA, "get_taa_stats"))

    # -- the HDR display chain (HYBRID_POST; include/utopian_hip.h "HDR display chain") ---
    _POST = "the HDR display chain is a per-context verb"

    @staticmethod
    def post_default_params():
        """UhPostParams as uh_post_default_params fills it: both flags, ACES, 6 levels, 1.0, 0.18, [1/64, 64], 0.1, 0.5, 0.95, 1.0, 0.04"""
        return post_default_params()

    def set_post_params(self, params=None, **fields):
        """uh_set_post_params: `params` (a PostParams; the defaults when None) with `fields` set on a copy - the params of the post
        passes that follow (render_hybrid with HYBRID_POST, post_image). A refused call raises and leaves the old ones."""
        return self._set_params(PostParams, self._hip_only(self._POST, "set_post_params"), post_default_params, params, fields)

    def reset_post_exposure(self):
        """uh_reset_post_exposure: the next post pass snaps to its target exposure (a camera cut)"""
        self._check(self._hip_only(self._POST, "reset_post_exposure")(self._ctx))

    def post_stats(self):
        """UhPostStats of the last post pass; all zero before the first"""
        return self._stats(PostStats, self._hip_only(self._POST, "get_post_stats"))

    def post_level_size(self, level):
        """(w, h) of bloom level `level` of this renderer's frame (0: the frame); raises ValueError for one that does not exist"""
        return post_level_size(self.width, self.height, level)

    def post_image(self, image):
        """uh_post_image: the three stages of the chain on `image`, (H, W, 4) float32, into post_output (read_post(POST_OUTPUT))"""
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.shape != (self.height, self.width, 4):
            raise ValueError(f"post_image: the image must be ({self.height}, {self.width}, 4), not {img.shape}")
        self._check(self._hip_only(self._POST, "post_image")(self._ctx, img.ctypes.data))

    def read_post(self, which, level=0):
        """uh_read_post: POST_OUTPUT (H, W, 4) float32; POST_BLOOM_DOWN / POST_BLOOM_UP level 1..post_stats().levels, (h, w, 4) float32 at
        the level's size; POST_HISTOGRAM 256 uint32 of the last metered pass"""
        if which == POST_HISTOGRAM:
            out = np.empty(256, np.uint32)
        elif which in (POST_BLOOM_DOWN, POST_BLOOM_UP):
            w, h = self.post_level_size(level)
            out = np.empty((h, w, 4), np.float32)
        elif which == POST_OUTPUT:
            out = np.empty((self.height, self.width, 4), np.float32)
        else:
            raise ValueError(f"post image index {which} (0..3)")
        self._check(self._hip_only(self._POST, "read_post")(self._ctx, int(which), int(level), out.ctypes.data))
        return out

    @staticmethod
    def jitter_view(view, index, width=None, height=None):
        """a copy of `view` jittered by taa_jitter(index) pixels: projection and inverse_projection through camera.jitter_projection, and
        prev_frame_projection_view - which the caller has set to the previous frame's UN-jittered projection * view - through
        camera.jitter_clip with the same offset, so that a camera at rest reprojects every pixel onto its own texel. The caller keeps the
        un-jittered projection * view of `view` for the next frame. width, height: the frame's, view.viewport_width / viewport_height
        when None."""
        v = ViewUniformData.from_buffer_copy(view)
        w = int(view.viewport_width) if width is None else width
        h = int(view.viewport_height) if height is None else height
        jx, jy = taa_jitter(index)
        proj, inv = cam.jitter_projection(np.array(view.projection[:], np.float32), jx, jy, w, h)
        v.projection[:] = proj.tolist()
        v.inverse_projection[:] = inv.tolist()
        v.prev_frame_projection_view[:] = cam.jitter_clip(np.array(view.prev_frame_projection_view[:], np.float32), jx, jy, w, h).tolist()
        return v

    # -- the denoiser (uh_denoise; include/utopian_hip.h "the denoiser") --------------------
    _DENOISE = "the denoiser is a per-context verb"

    def denoise(self, view, params=None):
        """uh_denoise on the accumulation of the last render_frame and the G-buffer of the last render_hybrid (same camera as `view`:
        the caller's job); view.prev_frame_projection_view is projection * view of the previous call. params None: the defaults"""
        params = default_denoise_params() if params is None else params
        self._check(self._hip_only(self._DENOISE, "denoise")(self._ctx, C.byref(view), C.byref(params)))

    _DENOISE_IMAGES = {
        DENOISE_COLOR: (np.float32, 4),
        DENOISE_OUTPUT: (np.uint8, 4),
        DENOISE_INPUT: (np.float32, 4),
        DENOISE_TEMPORAL_COLOR: (np.float32, 4),
        DENOISE_HISTORY: (np.float32, 1),
        DENOISE_VARIANCE: (np.float32, 1),
    }

    def read_denoised(self, which):
        """one image of the last denoise call: (H, W, 4) float32 colour / input / temporal colour, (H, W, 4) uint8 output (B, G, R, A),
        (H, W) float32 history length / variance"""
        return self._read_image(self._DENOISE_IMAGES, self._hip_only(self._DENOISE, "read_denoised"), which, f"denoiser image index {which} (0..5)")

    def reset_denoise_history(self):
        self._check(self._hip_only(self._DENOISE, "reset_denoise_history")(self._ctx))

    def denoise_stats(self):
        """UhDenoiseStats of the last denoise call: pass_ms of its four stages, geometry pixels, pixels that kept a history"""
        return self._stats(DenoiseStats, self._hip_only(self._DENOISE, "get_denoise_stats"))

    # -- cascaded shadow maps (UH_HYBRID_SHADOW_MAPS; include/utopian_hip.h) ---------------
    def set_shadowmap_params(self, params):
        """the cascades the next HYBRID_SHADOW_MAPS render uses: a ShadowmapParams (shadow_cascades, or the caller's own)"""
        self._check(self._hybrid_verb("set_shadowmap_params")(self._ctx, C.byref(params)))

    def read_shadow_map(self, cascade):
        """layer `cascade` of the shadow maps: (S, S) float32, row 0 at NDC y = +1"""
        s = self.shadow_map_stats().size
        if not s:
            s = 16  # the library refuses the read before the first render
        out = np.empty((s, s), dtype=np.float32)
        self._check(self._hybrid_verb("read_shadow_map")(self._ctx, int(cascade), out.ctypes.data))
        return out

    def shadow_map_stats(self):
        """UhShadowMapStats of the last shadow-map render"""
        return self._stats(ShadowMapStats, self._hybrid_verb("get_shadow_map_stats"))

    # -- the forward graph (uh_render_forward; include/utopian_hip.h) ------------------------
    def _forward_verb(self, name):
        return self._hip_only("the forward graph (shadow maps, forward pass, present) is a per-context verb", name, hasattr(self._lib, "uh_" + name))

    def render_forward(self, view, mask=FORWARD_GRAPH):
        """shadow maps, forward pass, present - the reference's Minimal mode in its pass order - for the bits of `mask`"""
        self._check(self._forward_verb("render_forward")(self._ctx, C.byref(view), int(mask)))

    _FORWARD_IMAGES = {
        FORWARD_OUTPUT: (np.float32, 4),
        FORWARD_DEPTH: (np.float32, 1),
        FORWARD_VISIBILITY: (np.uint32, 1),
        FORWARD_PRESENT_OUTPUT: (np.uint8, 4),
    }

    def read_forward(self, which):
        """one image of the forward graph, row 0 at NDC y = +1: (H, W, 4) float32 output, (H, W) float32 depth, (H, W) uint32 draw index
        (FORWARD_NONE where nothing was drawn), (H, W, 4) uint8 present output (B, G, R, A)"""
        return self._read_image(self._FORWARD_IMAGES, self._forward_verb("read_forward"), which, f"forward image index {which} (0..3)")

    def forward_stats(self):
        """UhForwardStats of the last render_forward call"""
        return self._stats(ForwardStats, self._forward_verb("get_forward_stats"))

    # -- stand-alone ray queries ----------------------------------------------------------
    def trace_closest(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        tuv = np.empty((n, 3), dtype=np.float32)
        mesh = np.empty(n, dtype=np.uint32)
        prim = np.empty(n, dtype=np.uint32)
        self._check(self._api.trace_closest(self._ctx, rays.ctypes.data, n, tuv.ctypes.data, mesh.ctypes.data, prim.ctypes.data))
        return tuv, mesh, prim

    def trace_any(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        occ = np.empty(len(rays), dtype=np.uint8)
        self._check(self._api.trace_any(self._ctx, rays.ctypes.data, len(rays), occ.ctypes.data))
        return occ

    # -- stats / options ------------------------------------------------------------------
    def get_stats(self):
        s = Stats()
        self._check(self._api.get_stats(self._ctx, C.byref(s)))
        return s

    def reset_stats(self):
        self._check(self._api.reset_stats(self._ctx))

    def set_option(self, name, value):
        self._check(self._api.set_option(self._ctx, name.encode(), int(value)))

    # -- multi-GPU tile partition ---------------------------------------------------------
    def set_tile_partition(self, rank, world, tile_size=64):
        self._check(self._api.set_tile_partition(self._ctx, rank, world, tile_size))

    def resolve_output(self, total_samples, accumulation_limit=999999):
        self._check(self._api.resolve_output(self._ctx, total_samples, accumulation_limit))

    # -- multi-GPU, the reservoir passes by bands of rows (uh_set_restir_partition) --------
    def set_restir_partition(self, rank, world, exchange=None):
        """`exchange(stream, spatial_base, band_bytes, rank, world) -> int`: called after every spatial pass, while the frame is
        enqueued; it must enqueue on `stream` (a hipStream_t as int; None on the CPU oracle, which calls it synchronously)
        whatever fills the other ranks' bands of the buffer at `spatial_base`. None with world > 1: the other bands stay stale."""
        fn = None
        if exchange is not None:
            fn = RESTIR_EXCHANGE_FN(lambda user, stream, base, band_bytes, r, w: int(exchange(stream, base, band_bytes, r, w) or 0))
        self._check(self._api.set_restir_partition(self._ctx, rank, world, C.cast(fn, C.c_void_p) if fn else None, None))
        self._restir_exchange = fn  # the library keeps the pointer: the trampoline must live as long as the partition

    def restir_rows(self):
        out = RestirRows()
        self._check(self._api.get_restir_rows(self._ctx, C.byref(out)))
        return out

    @staticmethod
    def rccl_unique_id():
        buf = (C.c_uint8 * 128)()
        st = _bind(load_library(), "uh_", "rccl_unique_id")(buf)
        if st != 0:
            raise UtopianError(f"uh_rccl_unique_id failed: {ERR_NAMES.get(st, st)} (is librccl loadable?)")
        return bytes(buf)

    def rccl_attach(self, rank, world, unique_id):
        """ncclCommInitRank on this context's device + the band partition with ncclAllGather as its exchange (collective:
        every rank of the job calls it with the id rank 0 made)"""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self._uh("rccl_attach")(self._ctx, rank, world, buf))

    def sun_grid_compare_builders(self):
        """uh_sun_grid_compare_builders: the device-built grid in use against the host builder on the same raster"""
        out = (C.c_uint64 * 8)()
        self._check(self._uh("sun_grid_compare_builders")(self._ctx, out))
        keys = ("cells", "entries_device", "entries_host", "cells_length_differs", "cells_list_differs", "cells_cover_differs", "walkable_cells", "host_build_us")
        return dict(zip(keys, (int(x) for x in out)))

    def check_acceleration(self):
        """uh_check_acceleration: the tree in use read back and held to the builders' invariants (csrc/bvh_invariants.h). One
        violation count per class under "violations" (all zero for a sound tree), the first offenders as text under "first"."""
        out = (C.c_uint64 * 16)()
        self._check(self._uh("check_acceleration")(self._ctx, out))
        classes = ("levels", "counts", "refs", "keys", "packets", "empty_slots", "containment")
        return {
            "nodes": int(out[0]), "triangles": int(out[1]), "levels": int(out[2]),
            "violations": {k: int(out[3 + i]) for i, k in enumerate(classes)},
            "sah": float(np.array([out[10]], dtype=np.uint64).view(np.float64)[0]),
            "geometry_checked": bool(out[11]),
            "first": (self._lib.uh_last_error(self._ctx) or b"").decode(),
        }

    def rccl_comm_count(self):
        """ranks of the attached RCCL communicator as ncclCommCount reports them (0: none attached)"""
        n = C.c_uint32(0)
        self._check(self._uh("rccl_comm_count")(self._ctx, C.byref(n)))
        return n.value

    def rccl_gather_tiles(self, root, total_samples, accumulation_limit=999999):
        """uh_rccl_gather_tiles: every rank's tiles to `root` over the attached communicator, composed there; enqueued (no host wait)"""
        self._check(self._uh("rccl_gather_tiles")(self._ctx, root, total_samples, accumulation_limit))

    def rccl_detach(self):
        self._check(self._uh("rccl_detach")(self._ctx))

    def tile_pack_count(self, rank):
        out = C.c_uint64()
        self._check(self._lib.uh_tile_pack_count(self._ctx, rank, C.byref(out)))
        return out.value

    def pack_tiles(self, device_ptr, capacity_pixels):
        self._check(self._lib.uh_pack_tiles(self._ctx, C.c_void_p(device_ptr), capacity_pixels))

    def unpack_tiles(self, from_rank, device_ptr, num_pixels):
        self._check(self._lib.uh_unpack_tiles(self._ctx, from_rank, C.c_void_p(device_ptr), num_pixels))

    def compose_tiles(self, device_ptr_all, stride_pixels, total_samples, accumulation_limit=999999):
        """every other rank's packed tiles (world buffers of stride_pixels each) into the accumulation image + the output resolve, one launch"""
        self._check(self._lib.uh_compose_tiles(self._ctx, C.c_void_p(device_ptr_all), stride_pixels, total_samples, accumulation_limit))

    def device_pointer(self, which):
        out = C.c_void_p()
        self._check(self._lib.uh_device_pointer(self._ctx, which, C.byref(out)))
        return out.value

    def stream(self):
        out = C.c_void_p()
        self._check(self._lib.uh_stream(self._ctx, C.byref(out)))
        return out.value


class MultiGpuRenderer(Renderer):
    """uh_mgpu_*: the same host interface over several GPUs driven by ONE process (tiles t % N == i
    per GPU, composition on GPU 0 at read-back). `devices` may repeat an ordinal."""

    backend = "hip-group"

    def __init__(self, width, height, devices, tile_size=64):
        lib = load_library()
        for name in ("mgpu_create", "mgpu_last_error", "mgpu_context", "mgpu_num_devices", "mgpu_get_num_lights", "mgpu_synchronize", "mgpu_compose"):
            _bind(lib, "uh_", name)  # (the group's twins of the context verbs, refit_acceleration among them: CApi below)
        devices = [int(d) for d in devices]
        arr = (C.c_int * len(devices))(*devices)

        def factory(w, h):
            ctx = C.c_void_p()
            st = lib.uh_mgpu_create(len(devices), arr, w, h, int(tile_size), C.byref(ctx))
            if st != 0:
                raise UtopianError(f"uh_mgpu_create failed: {ERR_NAMES.get(st, st)}: {(lib.uh_mgpu_last_error(None) or b'').decode()}")
            return ctx

        super().__init__(width, height, _api=CApi(lib, "uh_mgpu_"), _ctx_factory=factory)
        self.devices = devices

    def _check(self, st):
        if st != 0:
            raise UtopianError(f"{ERR_NAMES.get(st, st)}: {(self._lib.uh_mgpu_last_error(self._ctx) or b'').decode()}")

    def get_num_lights(self):
        out = C.c_uint32()
        self._check(self._lib.uh_mgpu_get_num_lights(self._ctx, C.byref(out)))
        return out.value

    def synchronize(self):
        self._check(self._lib.uh_mgpu_synchronize(self._ctx))

    def compose(self):
        self._check(self._lib.uh_mgpu_compose(self._ctx))


def _default_params(Struct, name):
    """a `Struct` as uh_<name> fills it"""
    p = Struct()
    if _bind(load_library(), "uh_", name)(C.byref(p)) != 0:
        raise UtopianError(f"uh_{name} failed")
    return p


def area_light_default_params():
    """UhAreaLightParams as uh_area_light_default_params fills it (needs no GPU)"""
    return _default_params(AreaLightParams, "area_light_default_params")


def glass_default_params():
    """UhGlassParams as uh_glass_default_params fills it (needs no GPU)"""
    return _default_params(GlassParams, "glass_default_params")


def fog_default_params():
    """UhFogParams as uh_fog_default_params fills it (needs no GPU)"""
    return _default_params(FogParams, "fog_default_params")


def glossy_default_params():
    """UhGlossyParams as uh_glossy_default_params fills it (needs no GPU)"""
    return _default_params(GlossyParams, "glossy_default_params")


def rtgi_default_params():
    """UhRtgiParams as uh_rtgi_default_params fills it (needs no GPU)"""
    return _default_params(RtgiParams, "rtgi_default_params")


def rtao_default_params():
    """UhRtaoParams as uh_rtao_default_params fills it (needs no GPU)"""
    return _default_params(RtaoParams, "rtao_default_params")


def default_denoise_params():
    """UhDenoiseParams as uh_denoise_default_params fills it (needs no GPU)"""
    return _default_params(DenoiseParams, "denoise_default_params")


def compose3x4(a, b):
    """a * b for row-major 3x4 affine matrices (instance.transform * model.transforms[i])."""
    A = np.vstack([np.asarray(a, dtype=np.float32).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)
    B = np.vstack([np.asarray(b, dtype=np.float32).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)
    return (A @ B)[:3].astype(np.float32).reshape(12)


def taa_default_params():
    """UhTaaParams as uh_taa_default_params fills it (needs no GPU)"""
    return _default_params(TaaParams, "taa_default_params")


def post_default_params():
    """UhPostParams as uh_post_default_params fills it (needs no GPU)"""
    return _default_params(PostParams, "post_default_params")


def post_level_size(width, height, level):
    """uh_post_level_size: (w, h) of bloom level `level` of a width x height frame (needs no GPU); ValueError for one that does not exist"""
    w, h = C.c_uint32(), C.c_uint32()
    if _bind(load_library(), "uh_", "post_level_size")(int(width), int(height), int(level), C.byref(w), C.byref(h)) != 0:
        raise ValueError(f"a {width} x {height} frame has no bloom level {level}")
    return int(w.value), int(h.value)


def taa_jitter(index):
    """uh_taa_jitter: the sub-pixel offset (jx, jy) of frame `index`, Halton(2, 3) - 0.5 in pixels (needs no GPU)"""
    out = (C.c_float * 2)()
    if _bind(load_library(), "uh_", "taa_jitter")(int(index), C.byref(out)) != 0:
        raise UtopianError("uh_taa_jitter failed")
    return float(out[0]), float(out[1])


def default_view(camera, width, height, num_lights=0):
    """ViewUniformData with the reference's defaults (prototype/src/main.rs:55-86), time = 0."""
    v = ViewUniformData()
    view, proj = camera.get_view(), camera.get_projection()
    v.view[:] = cam.to_glam(view).tolist()
    v.projection[:] = cam.to_glam(proj).tolist()
    v.inverse_view[:] = cam.to_glam(cam.inverse(view)).tolist()
    v.inverse_projection[:] = cam.to_glam(cam.inverse(proj)).tolist()
    v.prev_frame_projection_view[:] = cam.to_glam(np.diag(np.float32([-1, -1, -1, -1]))).tolist()
    v.eye_pos[:] = camera.get_position().tolist()
    v.samples_per_frame, v.total_samples, v.num_bounces = 1, 0, 5
    v.viewport_width, v.viewport_height = width, height
    v.time = 0.0
    v.num_lights = num_lights
    sun = np.float32([0.0, 0.9, 0.15])
    sun = sun / np.sqrt(np.dot(sun, sun), dtype=np.float32)
    v.sun_dir[:] = sun.tolist()
    v.shadows_enabled = v.ssao_enabled = v.fxaa_enabled = v.cubemap_enabled = v.ibl_enabled = 1
    v.sky_enabled = v.sun_shadow_enabled = v.lights_enabled = 1
    v.max_num_lights_used = 10000
    v.marching_cubes_enabled = 0
    v.temporal_reuse_enabled = v.spatial_reuse_enabled = 1
    v.rebuild_tlas = 0
    v.accumulation_limit = 999999
    v.use_ris_light_sampling = 1
    v.raytracing_supported = 1
    return v


class FrameLoop:
    """The per-frame protocol of Application::run (prototype/src/main.rs:460-471, 545-546):
    total_samples += samples_per_frame BEFORE the frame is rendered; prev_frame_projection_view =
    projection * view AFTER it was recorded."""

    def __init__(self, renderer, view):
        self.renderer, self.view = renderer, view

    def frame(self, pass_mask=PASS_ALL):
        v = self.view
        v.total_samples += v.samples_per_frame
        v.num_lights = self.renderer.get_num_lights()
        self.renderer.render_frame(v, pass_mask)
        self.end_frame()

    def end_frame(self):
        """main.rs:545-546: prev_frame_projection_view = projection * view, after the frame."""
        v = self.view
        proj = np.array(v.projection[:], dtype=np.float32).reshape(4, 4).T
        view = np.array(v.view[:], dtype=np.float32).reshape(4, 4).T
        v.prev_frame_projection_view[:] = cam.to_glam((proj @ view).astype(np.float32)).tolist()

    def frames(self, count, pass_mask=PASS_ALL):
        """`count` frames of the loop with the camera at rest. Everything that includes the path-tracing pass is handed to
        uh_render_frames in one call (the library batches frames into shared wavefronts of about 32 M paths: 16 frames at
        1080p, at most 16 when the reservoir passes run too). The first frame of a run that includes the temporal pass goes alone:
        it is the one that may still see another prev_frame_projection_view."""
        from .types import PASS_REFERENCE_PT, PASS_TEMPORAL_REUSE

        v = self.view
        batchable = self.renderer.backend.startswith("hip") and count > 1 and (pass_mask & PASS_REFERENCE_PT)
        if batchable and (pass_mask & PASS_TEMPORAL_REUSE):
            self.frame(pass_mask)
            count -= 1
            batchable = count > 1
        if not batchable:
            for _ in range(count):
                self.frame(pass_mask)
            return
        v.num_lights = self.renderer.get_num_lights()
        v.total_samples += v.samples_per_frame  # first frame of the run
        self.renderer.render_frames(v, pass_mask, count)
        v.total_samples += (count - 1) * v.samples_per_frame
        proj = np.array(v.projection[:], dtype=np.float32).reshape(4, 4).T
        view = np.array(v.view[:], dtype=np.float32).reshape(4, 4).T
        v.prev_frame_projection_view[:] = cam.to_glam((proj @ view).astype(np.float32)).tolist()

    def reset(self):
        """camera / setting change: total_samples = 0 (main.rs:400-413)."""
        self.view.total_samples = 0
        self.renderer.reset_accumulation()


def shadow_cascades(camera, sun_dir):
    """setup_shadow_pass (shadow.rs) for `camera` (its own z_near / z_far) and `sun_dir`: a ShadowmapParams, by uh_shadow_cascades
    (host arithmetic: no device needed)"""
    view = (C.c_float * 16)(*cam.to_glam(camera.get_view()).tolist())
    proj = (C.c_float * 16)(*cam.to_glam(camera.get_projection()).tolist())
    sun = (C.c_float * 3)(*[float(x) for x in sun_dir])
    out = ShadowmapParams()
    st = _bind(load_library(), "uh_", "shadow_cascades")(view, proj, float(camera.z_near), float(camera.z_far), sun, C.byref(out))
    if st != 0:
        raise UtopianError(f"uh_shadow_cascades: {ERR_NAMES.get(st, st)}")
    return out
