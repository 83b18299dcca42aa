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
    HYBRID_ALBEDO,
    HYBRID_ALL,
    HYBRID_AO_COUNTS,
    HYBRID_GI_COUNTS,
    HYBRID_GI_RADIANCE,
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
    Stats,
    TaaParams,
    TaaStats,
    ViewUniformData,
)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UTOPIAN_HIP_LIB") or os.path.join(_HERE, "libutopian_hip.so")  # UTOPIAN_HIP_LIB: an alternative build of the same library (experiments)


class UtopianError(RuntimeError):
    pass


class CApi:
    """Typed ctypes view of a library exporting the utopian_hip.h entry points under `prefix`."""

    def __init__(self, lib, prefix):
        self.lib, self.prefix = lib, prefix
        p, u32, vp = C.POINTER, C.c_uint32, C.c_void_p
        sig = {
            "add_texture_rgba8": [vp, vp, u32, u32, p(u32)],
            "add_mesh": [vp, vp, u32, vp, u32, p(GpuMaterial), p(C.c_float), p(u32)],
            "add_light": [vp, p(GpuLight), p(u32)],
            "set_instance_transform": [vp, u32, p(C.c_float)],
            "build_acceleration": [vp],
            "refit_acceleration": [vp],
            "render_frame": [vp, p(ViewUniformData), u32],
            "render_frames": [vp, p(ViewUniformData), u32, u32],
            "reset_accumulation": [vp],
            "read_accumulation": [vp, vp],
            "read_output_bgra8": [vp, vp],
            "read_reservoirs": [vp, C.c_int, vp],
            "write_reservoirs": [vp, C.c_int, vp],
            "write_gbuffer_position": [vp, vp],
            "read_gbuffer_position": [vp, vp],
            "trace_closest": [vp, vp, u32, vp, vp, vp],
            "trace_any": [vp, vp, u32, vp],
            "get_stats": [vp, p(Stats)],
            "reset_stats": [vp],
            "set_option": [vp, C.c_char_p, C.c_int],
            "set_tile_partition": [vp, u32, u32, u32],
            "set_restir_partition": [vp, u32, u32, vp, vp],
            "get_restir_rows": [vp, p(RestirRows)],
            "resolve_output": [vp, u32, u32],
            "render_hybrid": [vp, p(ViewUniformData), u32],
            "read_hybrid": [vp, C.c_int, vp],
            "get_hybrid_stats": [vp, p(HybridStats)],
            "get_hybrid_frame_stats": [vp, p(HybridFrameStats)],
            "read_environment": [vp, C.c_int, C.c_int, C.c_int, vp],
            "get_environment_stats": [vp, p(EnvironmentStats)],
        }
        hybrid = ("render_hybrid", "read_hybrid", "get_hybrid_stats", "get_hybrid_frame_stats", "read_environment", "get_environment_stats")
        for name, argtypes in sig.items():
            if not hasattr(lib, prefix + name) and (name == "render_frames" or name in hybrid or prefix == "uh_mgpu_"):
                continue  # the oracle renders frame by frame and has no hybrid passes; the GPU group has no per-context queries
            fn = getattr(lib, prefix + name)
            fn.argtypes, fn.restype = argtypes, C.c_int
            setattr(self, name, fn)
        self.destroy = getattr(lib, prefix + "destroy")
        self.destroy.argtypes, self.destroy.restype = [vp], None


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
    lib.uh_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.uh_create.restype = C.c_int
    lib.uh_last_error.argtypes, lib.uh_last_error.restype = [C.c_void_p], C.c_char_p
    lib.uh_version.restype = C.c_char_p
    lib.uh_hip_versions.argtypes, lib.uh_hip_versions.restype = [C.POINTER(C.c_int), C.POINTER(C.c_int)], C.c_int
    for name, extra in (
        ("uh_get_num_lights", [C.POINTER(C.c_uint32)]),
        ("uh_synchronize", []),
        ("uh_tile_pack_count", [C.c_uint32, C.POINTER(C.c_uint64)]),
        ("uh_pack_tiles", [C.c_void_p, C.c_uint64]),
        ("uh_unpack_tiles", [C.c_uint32, C.c_void_p, C.c_uint64]),
        ("uh_compose_tiles", [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
        ("uh_device_pointer", [C.c_int, C.POINTER(C.c_void_p)]),
        ("uh_stream", [C.POINTER(C.c_void_p)]),
    ):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [C.c_void_p] + extra, C.c_int
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
        return mesh_ids

    def add_isosurface_mesh(self, resolution, lo, hi, time=0.0, material=None, world3x4=None):
        """uh_add_isosurface_mesh: the reference's marching-cubes density field, extracted on the GPU.
        Returns (mesh index or None, triangle count)."""
        if material is None:
            material = make_material(base_color=(0.8, 0.8, 0.8, 1.0), diffuse_map=self.default_diffuse_map())
        w = identity3x4() if world3x4 is None else np.ascontiguousarray(world3x4, dtype=np.float32).reshape(12)
        fn = self._lib.uh_add_isosurface_mesh
        fn.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.POINTER(GpuMaterial), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        fn.restype = C.c_int
        mesh, tris = C.c_uint32(), C.c_uint32()
        self._check(fn(self._ctx, int(resolution), float(lo), float(hi), float(time), C.byref(material), w.ctypes.data_as(C.POINTER(C.c_float)), C.byref(mesh), C.byref(tris)))
        return (None if mesh.value == 0xFFFFFFFF else mesh.value), tris.value

    def update_isosurface_mesh(self, mesh, time):
        """uh_update_isosurface_mesh: re-extracts the field at `time` with the parameters mesh `mesh` was created with by
        add_isosurface_mesh and makes the result its geometry, on the device. Returns the triangle count; the context needs
        build_acceleration afterwards."""
        fn = self._lib.uh_update_isosurface_mesh
        fn.argtypes, fn.restype = [C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_uint32)], C.c_int
        tris = C.c_uint32()
        self._check(fn(self._ctx, int(mesh), float(time), C.byref(tris)))
        return tris.value

    def isosurface_update_stats(self):
        """UhIsosurfaceUpdateStats (all zero before the first update_isosurface_mesh)"""
        fn = self._lib.uh_get_isosurface_update_stats
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(IsosurfaceUpdateStats)], C.c_int
        s = IsosurfaceUpdateStats()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    def update_mesh_vertices(self, mesh, vertices=None, *, device_ptr=None, count=None):
        """uh_update_mesh_vertices: new vertices for a mesh of add_mesh, its index list kept. Host input: `vertices`, a VERTEX_DTYPE
        array of the mesh's length. Device input: `device_ptr`, the address of `count` vertex records on the renderer's device, which
        the caller has finished writing. refit_acceleration (or a frame with view.rebuild_tlas = 1) or build_acceleration follows."""
        fn = self._lib.uh_update_mesh_vertices
        fn.argtypes, fn.restype = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int], C.c_int
        if device_ptr is not None:
            assert vertices is None and count is not None, "device input: device_ptr= with count="
            self._check(fn(self._ctx, int(mesh), C.c_void_p(int(device_ptr)), int(count), 1))
            return
        vertices = np.ascontiguousarray(vertices, dtype=VERTEX_DTYPE)
        self._check(fn(self._ctx, int(mesh), C.c_void_p(vertices.ctypes.data if len(vertices) else None), len(vertices), 0))

    def mesh_update_stats(self):
        """UhMeshUpdateStats (all zero before the first update_mesh_vertices)"""
        fn = self._lib.uh_get_mesh_update_stats
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(MeshUpdateStats)], C.c_int
        s = MeshUpdateStats()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    def isosurface_cells(self, resolution, lo, hi, time=0.0):
        """uh_isosurface_cells: per cell of the extraction grid (x fastest) its marching-cubes case index and the triangles it keeps"""
        n = int(resolution) ** 3
        cube, kept = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        fn = self._lib.uh_isosurface_cells
        fn.argtypes, fn.restype = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p], C.c_int
        self._check(fn(self._ctx, int(resolution), float(lo), float(hi), float(time), cube.ctypes.data, kept.ctypes.data))
        return cube, kept

    def read_mesh(self, mesh_index):
        """the context's host copy of a mesh: (vertices as VERTEX_DTYPE, indices)"""
        lib = self._lib
        lib.uh_mesh_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.uh_read_mesh.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.uh_mesh_info.restype = lib.uh_read_mesh.restype = C.c_int
        nv, ni = C.c_uint32(), C.c_uint32()
        self._check(lib.uh_mesh_info(self._ctx, mesh_index, C.byref(nv), C.byref(ni)))
        v = np.zeros(nv.value, dtype=VERTEX_DTYPE)
        idx = np.zeros(ni.value, dtype=np.uint32)
        self._check(lib.uh_read_mesh(self._ctx, mesh_index, v.ctypes.data, idx.ctypes.data))
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
        if self.backend != "hip" or not hasattr(self._api, "render_hybrid"):
            raise NotImplementedError(f"the hybrid passes (rt_shadows / rt_reflections / the final frame) are per-context verbs of the HIP library; backend {self.backend!r} has none")
        return self._api

    def render_hybrid(self, view, mask=HYBRID_ALL):
        """rt_shadows (previous G-buffer), gbuffer, rt_reflections (this one), ssao, deferred, sky, present - the reference's pass order -
        for the bits of `mask` (HYBRID_FRAME: all seven)"""
        api = self._hybrid_api()
        self._check(api.render_hybrid(self._ctx, C.byref(view), int(mask)))
        if int(mask) & HYBRID_TAA:
            self._taa_rendered = True

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

    def read_hybrid(self, which):
        """one image of the hybrid graph: (H, W, 4) float32 position / normal / pbr / deferred output, (H, W, 4) uint8 albedo / reflections /
        present output (B, G, R, A), (H, W) uint8 shadows, (H, W) uint16 SSAO, (H, W) float32 marching-cubes depth buffer, (H, W) uint32
        marching-cubes draw index (MARCHING_CUBES_NONE where none survived), (H, W) float32 rasterised G-buffer depth, (H, W) uint32
        rasterised G-buffer draw index (GBUFFER_NONE where none survived), (H, W) uint8 light visibility of HYBRID_RESTIR_LIGHTS,
        (H, W) uint8 occluded-ray counts of HYBRID_RTAO, (H, W, 4) float32 motion image of HYBRID_MOTION (previous world position, w = 1
        with a correspondence), once a call with HYBRID_TAA has run (H, W, 4) float32 taa_output and (H, W) float32 history length, and of
        HYBRID_RTGI (H, W, 4) float32 filtered incoming radiance (w = 1 where the pixel cast) and (H, W, 4) uint8 ray counts (sunlit, dark,
        emitter, missed)"""
        api = self._hybrid_api()
        images = {**self._HYBRID_IMAGES, **(self._TAA_IMAGES if self._taa_rendered else {}), **self._GI_IMAGES}
        if which not in images:
            raise ValueError(f"hybrid image index {which} (0..15, 18..19, and 16..17 once a render_hybrid call with HYBRID_TAA has run)")
        dtype, ch = images[which]
        out = np.empty((self.height, self.width, ch) if ch > 1 else (self.height, self.width), dtype=dtype)
        self._check(api.read_hybrid(self._ctx, int(which), out.ctypes.data))
        return out

    def hybrid_stats(self):
        api = self._hybrid_api()
        s = HybridStats()
        self._check(api.get_hybrid_stats(self._ctx, C.byref(s)))
        return s

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
        api = self._hybrid_api()
        s = EnvironmentStats()
        self._check(api.get_environment_stats(self._ctx, C.byref(s)))
        return s

    def hybrid_frame_stats(self):
        """UhHybridFrameStats of the last render_hybrid call: pass_ms of all seven passes in bit order"""
        api = self._hybrid_api()
        s = HybridFrameStats()
        self._check(api.get_hybrid_frame_stats(self._ctx, C.byref(s)))
        return s

    def marching_cubes_stats(self):
        """UhMarchingCubesStats of the last HYBRID_MARCHING_CUBES pass"""
        self._hybrid_api()
        fn = getattr(self._lib, "uh_get_marching_cubes_stats")
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(MarchingCubesStats)], C.c_int
        s = MarchingCubesStats()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    def gbuffer_raster_stats(self):
        """UhGbufferRasterStats of the last rasterised G-buffer pass (HYBRID_GBUFFER | HYBRID_GBUFFER_RASTER)"""
        self._hybrid_api()
        fn = getattr(self._lib, "uh_get_gbuffer_raster_stats")
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(GbufferRasterStats)], C.c_int
        s = GbufferRasterStats()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    def hybrid_restir_stats(self):
        """UhHybridRestirStats of the last render_hybrid call with HYBRID_RESTIR_LIGHTS: rays, occluded, pass_ms"""
        self._hybrid_api()
        fn = getattr(self._lib, "uh_get_hybrid_restir_stats")
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(HybridRestirStats)], C.c_int
        s = HybridRestirStats()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    # -- ray-traced ambient occlusion (HYBRID_RTAO; include/utopian_hip.h "UH_HYBRID_RTAO") ---
    def _rtao_fn(self, name, arg):
        if self.backend != "hip":
            raise NotImplementedError(f"ray-traced ambient occlusion is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(arg)], C.c_int
        return fn

    def set_rtao_params(self, params=None, **fields):
        """uh_set_rtao_params: `params` (an RtaoParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_RTAO that follow. A refused call raises and leaves the old ones."""
        p = RtaoParams.from_buffer_copy(rtao_default_params() if params is None else params)
        for k, v in fields.items():
            if not hasattr(p, k):
                raise TypeError(f"RtaoParams has no field {k!r}")
            setattr(p, k, v)
        self._check(self._rtao_fn("set_rtao_params", RtaoParams)(self._ctx, C.byref(p)))
        return p

    def rtao_stats(self):
        """UhRtaoStats of the last rtao pass: pixels, rays, occluded, trace_ms, filter_ms"""
        s = RtaoStats()
        self._check(self._rtao_fn("get_rtao_stats", RtaoStats)(self._ctx, C.byref(s)))
        return s

    # -- one-bounce ray-traced diffuse GI (HYBRID_RTGI; include/utopian_hip.h "UH_HYBRID_RTGI") ---
    def _rtgi_fn(self, name, arg):
        if self.backend != "hip":
            raise NotImplementedError(f"ray-traced diffuse GI is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(arg)], C.c_int
        return fn

    def set_rtgi_params(self, params=None, **fields):
        """uh_set_rtgi_params: `params` (an RtgiParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_RTGI that follow. A refused call raises and leaves the old ones."""
        p = RtgiParams.from_buffer_copy(rtgi_default_params() if params is None else params)
        for k, v in fields.items():
            if not hasattr(p, k):
                raise TypeError(f"RtgiParams has no field {k!r}")
            setattr(p, k, v)
        self._check(self._rtgi_fn("set_rtgi_params", RtgiParams)(self._ctx, C.byref(p)))
        return p

    def rtgi_stats(self):
        """UhRtgiStats of the last rtgi pass: pixels, rays, shadow_rays, misses, trace_ms, shadow_ms, filter_ms, composite_ms"""
        s = RtgiStats()
        self._check(self._rtgi_fn("get_rtgi_stats", RtgiStats)(self._ctx, C.byref(s)))
        return s

    def rtao_visits(self):
        """(node visits, triangle tests) of the last rtao pass's walks, counted while option "count_visits" is 1; else (0, 0)"""
        if self.backend != "hip":
            raise NotImplementedError(f"ray-traced ambient occlusion is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = self._lib.uh_get_rtao_visits
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int
        nodes, tris = C.c_uint64(), C.c_uint64()
        self._check(fn(self._ctx, C.byref(nodes), C.byref(tris)))
        return nodes.value, tris.value

    # -- motion vectors (HYBRID_GBUFFER | HYBRID_MOTION; include/utopian_hip.h "motion vectors") ---
    def motion_stats(self):
        """UhMotionStats of the last motion pass: pixels_with / pixels_without a correspondence, meshes_static / _rigid / _deformed /
        _none, motion_ms, snapshot_ms; all zero before the first pass"""
        if self.backend != "hip":
            raise NotImplementedError(f"motion vectors are a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = self._lib.uh_get_motion_stats
        fn.argtypes, fn.restype = [C.c_void_p, C.POINTER(MotionStats)], C.c_int
        s = MotionStats()
        self._check(fn(self._ctx, C.byref(s)))
        return s

    # -- temporal anti-aliasing (HYBRID_TAA; include/utopian_hip.h "temporal anti-aliasing") ---
    def _taa_fn(self, name, *argtypes):
        if self.backend != "hip":
            raise NotImplementedError(f"temporal anti-aliasing is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p] + [C.POINTER(a) for a in argtypes], C.c_int
        return fn

    @staticmethod
    def taa_default_params():
        """UhTaaParams as uh_taa_default_params fills it: TAA_CLAMP, 16, 0.1, 1.0"""
        return taa_default_params()

    def set_taa_params(self, params=None, **fields):
        """uh_set_taa_params: `params` (a TaaParams; the defaults when None) with `fields` set on a copy - the params of the
        render_hybrid calls with HYBRID_TAA that follow. A refused call raises and leaves the old ones."""
        p = TaaParams.from_buffer_copy(taa_default_params() if params is None else params)
        for k, v in fields.items():
            if not hasattr(p, k):
                raise TypeError(f"TaaParams has no field {k!r}")
            setattr(p, k, v)
        self._check(self._taa_fn("set_taa_params", TaaParams)(self._ctx, C.byref(p)))
        return p

    def reset_taa_history(self):
        """uh_reset_taa_history: the next taa pass starts from no history (a camera cut)"""
        self._check(self._taa_fn("reset_taa_history")(self._ctx))

    def taa_stats(self):
        """UhTaaStats of the last taa pass: history_pixels, reset_pixels, taa_ms; all zero before the first pass"""
        s = TaaStats()
        self._check(self._taa_fn("get_taa_stats", TaaStats)(self._ctx, C.byref(s)))
        return s

    # -- the HDR display chain (HYBRID_POST; include/utopian_hip.h "HDR display chain") ---
    def _post_fn(self, name, *argtypes):
        if self.backend != "hip":
            raise NotImplementedError(f"the HDR display chain is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p] + list(argtypes), C.c_int
        return fn

    @staticmethod
    def post_default_params():
        """UhPostParams as uh_post_default_params fills it: both flags, ACES, 6 levels, 1.0, 0.18, [1/64, 64], 0.1, 0.5, 0.95, 1.0, 0.04"""
        return post_default_params()

    def set_post_params(self, params=None, **fields):
        """uh_set_post_params: `params` (a PostParams; the defaults when None) with `fields` set on a copy - the params of the post
        passes that follow (render_hybrid with HYBRID_POST, post_image). A refused call raises and leaves the old ones."""
        p = PostParams.from_buffer_copy(post_default_params() if params is None else params)
        for k, v in fields.items():
            if not hasattr(p, k):
                raise TypeError(f"PostParams has no field {k!r}")
            setattr(p, k, v)
        self._check(self._post_fn("set_post_params", C.POINTER(PostParams))(self._ctx, C.byref(p)))
        return p

    def reset_post_exposure(self):
        """uh_reset_post_exposure: the next post pass snaps to its target exposure (a camera cut)"""
        self._check(self._post_fn("reset_post_exposure")(self._ctx))

    def post_stats(self):
        """UhPostStats of the last post pass; all zero before the first"""
        s = PostStats()
        self._check(self._post_fn("get_post_stats", C.POINTER(PostStats))(self._ctx, C.byref(s)))
        return s

    def post_level_size(self, level):
        """(w, h) of bloom level `level` of this renderer's frame (0: the frame); raises ValueError for one that does not exist"""
        return post_level_size(self.width, self.height, level)

    def post_image(self, image):
        """uh_post_image: the three stages of the chain on `image`, (H, W, 4) float32, into post_output (read_post(POST_OUTPUT))"""
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.shape != (self.height, self.width, 4):
            raise ValueError(f"post_image: the image must be ({self.height}, {self.width}, 4), not {img.shape}")
        self._check(self._post_fn("post_image", C.c_void_p)(self._ctx, img.ctypes.data))

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
        self._check(self._post_fn("read_post", C.c_int, C.c_int, C.c_void_p)(self._ctx, int(which), int(level), out.ctypes.data))
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
    def _denoise_fn(self, name, argtypes):
        if self.backend != "hip":
            raise NotImplementedError(f"the denoiser is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p] + argtypes, C.c_int
        return fn

    def denoise(self, view, params=None):
        """uh_denoise on the accumulation of the last render_frame and the G-buffer of the last render_hybrid (same camera as `view`:
        the caller's job); view.prev_frame_projection_view is projection * view of the previous call. params None: the defaults"""
        params = default_denoise_params() if params is None else params
        self._check(self._denoise_fn("denoise", [C.POINTER(ViewUniformData), C.POINTER(DenoiseParams)])(self._ctx, C.byref(view), C.byref(params)))

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
        fn = self._denoise_fn("read_denoised", [C.c_int, C.c_void_p])
        if which not in self._DENOISE_IMAGES:
            raise ValueError(f"denoiser image index {which} (0..5)")
        dtype, ch = self._DENOISE_IMAGES[which]
        out = np.empty((self.height, self.width, ch) if ch > 1 else (self.height, self.width), dtype=dtype)
        self._check(fn(self._ctx, int(which), out.ctypes.data))
        return out

    def reset_denoise_history(self):
        self._check(self._denoise_fn("reset_denoise_history", [])(self._ctx))

    def denoise_stats(self):
        """UhDenoiseStats of the last denoise call: pass_ms of its four stages, geometry pixels, pixels that kept a history"""
        s = DenoiseStats()
        self._check(self._denoise_fn("get_denoise_stats", [C.POINTER(DenoiseStats)])(self._ctx, C.byref(s)))
        return s

    # -- cascaded shadow maps (UH_HYBRID_SHADOW_MAPS; include/utopian_hip.h) ---------------
    def _shadow_fn(self, name, argtypes):
        self._hybrid_api()
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p] + argtypes, C.c_int
        return fn

    def set_shadowmap_params(self, params):
        """the cascades the next HYBRID_SHADOW_MAPS render uses: a ShadowmapParams (shadow_cascades, or the caller's own)"""
        self._check(self._shadow_fn("set_shadowmap_params", [C.POINTER(ShadowmapParams)])(self._ctx, C.byref(params)))

    def read_shadow_map(self, cascade):
        """layer `cascade` of the shadow maps: (S, S) float32, row 0 at NDC y = +1"""
        s = self.shadow_map_stats().size
        if not s:
            s = 16  # the library refuses the read before the first render
        out = np.empty((s, s), dtype=np.float32)
        self._check(self._shadow_fn("read_shadow_map", [C.c_int, C.c_void_p])(self._ctx, int(cascade), out.ctypes.data))
        return out

    def shadow_map_stats(self):
        """UhShadowMapStats of the last shadow-map render"""
        s = ShadowMapStats()
        self._check(self._shadow_fn("get_shadow_map_stats", [C.POINTER(ShadowMapStats)])(self._ctx, C.byref(s)))
        return s

    # -- the forward graph (uh_render_forward; include/utopian_hip.h) ------------------------
    def _forward_fn(self, name, argtypes):
        if self.backend != "hip" or not hasattr(self._lib, "uh_" + name):
            raise NotImplementedError(f"the forward graph (shadow maps, forward pass, present) is a per-context verb of the HIP library; backend {self.backend!r} has none")
        fn = getattr(self._lib, "uh_" + name)
        fn.argtypes, fn.restype = [C.c_void_p] + argtypes, C.c_int
        return fn

    def render_forward(self, view, mask=FORWARD_GRAPH):
        """shadow maps, forward pass, present - the reference's Minimal mode in its pass order - for the bits of `mask`"""
        fn = self._forward_fn("render_forward", [C.POINTER(ViewUniformData), C.c_uint32])
        self._check(fn(self._ctx, C.byref(view), int(mask)))

    _FORWARD_IMAGES = {
        FORWARD_OUTPUT: (np.float32, 4),
        FORWARD_DEPTH: (np.float32, 1),
        FORWARD_VISIBILITY: (np.uint32, 1),
        FORWARD_PRESENT_OUTPUT: (np.uint8, 4),
    }

    def read_forward(self, which):
        """one image of the forward graph, row 0 at NDC y = +1: (H, W, 4) float32 output, (H, W) float32 depth, (H, W) uint32 draw index
        (FORWARD_NONE where nothing was drawn), (H, W, 4) uint8 present output (B, G, R, A)"""
        fn = self._forward_fn("read_forward", [C.c_int, C.c_void_p])
        if which not in self._FORWARD_IMAGES:
            raise ValueError(f"forward image index {which} (0..3)")
        dtype, ch = self._FORWARD_IMAGES[which]
        out = np.empty((self.height, self.width, ch) if ch > 1 else (self.height, self.width), dtype=dtype)
        self._check(fn(self._ctx, int(which), out.ctypes.data))
        return out

    def forward_stats(self):
        """UhForwardStats of the last render_forward call"""
        s = ForwardStats()
        self._check(self._forward_fn("get_forward_stats", [C.POINTER(ForwardStats)])(self._ctx, C.byref(s)))
        return s

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
        lib = load_library()
        lib.uh_rccl_unique_id.argtypes, lib.uh_rccl_unique_id.restype = [C.c_void_p], C.c_int
        buf = (C.c_uint8 * 128)()
        st = lib.uh_rccl_unique_id(buf)
        if st != 0:
            raise UtopianError(f"uh_rccl_unique_id failed: {ERR_NAMES.get(st, st)} (is librccl loadable?)")
        return bytes(buf)

    def rccl_attach(self, rank, world, unique_id):
        """ncclCommInitRank on this context's device + the band partition with ncclAllGather as its exchange (collective:
        every rank of the job calls it with the id rank 0 made)"""
        self._lib.uh_rccl_attach.argtypes, self._lib.uh_rccl_attach.restype = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p], C.c_int
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self._lib.uh_rccl_attach(self._ctx, rank, world, buf))

    def sun_grid_compare_builders(self):
        """uh_sun_grid_compare_builders: the device-built grid in use against the host builder on the same raster"""
        out = (C.c_uint64 * 8)()
        self._lib.uh_sun_grid_compare_builders.argtypes, self._lib.uh_sun_grid_compare_builders.restype = [C.c_void_p, C.POINTER(C.c_uint64)], C.c_int
        self._check(self._lib.uh_sun_grid_compare_builders(self._ctx, out))
        keys = ("cells", "entries_device", "entries_host", "cells_length_differs", "cells_list_differs", "cells_cover_differs", "walkable_cells", "host_build_us")
        return dict(zip(keys, (int(x) for x in out)))

    def check_acceleration(self):
        """uh_check_acceleration: the tree in use read back and held to the builders' invariants (csrc/bvh_invariants.h). One
        violation count per class under "violations" (all zero for a sound tree), the first offenders as text under "first"."""
        out = (C.c_uint64 * 16)()
        self._lib.uh_check_acceleration.argtypes, self._lib.uh_check_acceleration.restype = [C.c_void_p, C.POINTER(C.c_uint64)], C.c_int
        self._check(self._lib.uh_check_acceleration(self._ctx, out))
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
        self._lib.uh_rccl_comm_count.argtypes, self._lib.uh_rccl_comm_count.restype = [C.c_void_p, C.POINTER(C.c_uint32)], C.c_int
        self._check(self._lib.uh_rccl_comm_count(self._ctx, C.byref(n)))
        return n.value

    def rccl_gather_tiles(self, root, total_samples, accumulation_limit=999999):
        """uh_rccl_gather_tiles: every rank's tiles to `root` over the attached communicator, composed there; enqueued (no host wait)"""
        fn = self._lib.uh_rccl_gather_tiles
        fn.argtypes, fn.restype = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32], C.c_int
        self._check(fn(self._ctx, root, total_samples, accumulation_limit))

    def rccl_detach(self):
        self._lib.uh_rccl_detach.argtypes, self._lib.uh_rccl_detach.restype = [C.c_void_p], C.c_int
        self._check(self._lib.uh_rccl_detach(self._ctx))

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
        lib.uh_mgpu_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        lib.uh_mgpu_create.restype = C.c_int
        lib.uh_mgpu_last_error.argtypes, lib.uh_mgpu_last_error.restype = [C.c_void_p], C.c_char_p
        lib.uh_mgpu_context.argtypes, lib.uh_mgpu_context.restype = [C.c_void_p, C.c_int], C.c_void_p
        lib.uh_mgpu_num_devices.argtypes, lib.uh_mgpu_num_devices.restype = [C.c_void_p], C.c_int
        for name, extra in (("get_num_lights", [C.POINTER(C.c_uint32)]), ("synchronize", []), ("compose", []), ("refit_acceleration", [])):
            fn = getattr(lib, "uh_mgpu_" + name)
            fn.argtypes, fn.restype = [C.c_void_p] + extra, C.c_int
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


def rtgi_default_params():
    """UhRtgiParams as uh_rtgi_default_params fills it (needs no GPU)"""
    fn = load_library().uh_rtgi_default_params
    fn.argtypes, fn.restype = [C.POINTER(RtgiParams)], C.c_int
    p = RtgiParams()
    if fn(C.byref(p)) != 0:
        raise UtopianError("uh_rtgi_default_params failed")
    return p


def rtao_default_params():
    """UhRtaoParams as uh_rtao_default_params fills it (needs no GPU)"""
    fn = load_library().uh_rtao_default_params
    fn.argtypes, fn.restype = [C.POINTER(RtaoParams)], C.c_int
    p = RtaoParams()
    if fn(C.byref(p)) != 0:
        raise UtopianError("uh_rtao_default_params failed")
    return p


def default_denoise_params():
    """UhDenoiseParams as uh_denoise_default_params fills it (needs no GPU)"""
    fn = load_library().uh_denoise_default_params
    fn.argtypes, fn.restype = [C.POINTER(DenoiseParams)], C.c_int
    p = DenoiseParams()
    if fn(C.byref(p)) != 0:
        raise UtopianError("uh_denoise_default_params failed")
    return p


def compose3x4(a, b):
    """a * b for row-major 3x4 affine matrices (instance.transform * model.transforms[i])."""
    A = np.vstack([np.asarray(a, dtype=np.float32).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)
    B = np.vstack([np.asarray(b, dtype=np.float32).reshape(3, 4), [0, 0, 0, 1]]).astype(np.float32)
    return (A @ B)[:3].astype(np.float32).reshape(12)


def taa_default_params():
    """UhTaaParams as uh_taa_default_params fills it (needs no GPU)"""
    fn = load_library().uh_taa_default_params
    fn.argtypes, fn.restype = [C.POINTER(TaaParams)], C.c_int
    p = TaaParams()
    if fn(C.byref(p)) != 0:
        raise UtopianError("uh_taa_default_params failed")
    return p


def post_default_params():
    """UhPostParams as uh_post_default_params fills it (needs no GPU)"""
    fn = load_library().uh_post_default_params
    fn.argtypes, fn.restype = [C.POINTER(PostParams)], C.c_int
    p = PostParams()
    if fn(C.byref(p)) != 0:
        raise UtopianError("uh_post_default_params failed")
    return p


def post_level_size(width, height, level):
    """uh_post_level_size: (w, h) of bloom level `level` of a width x height frame (needs no GPU); ValueError for one that does not exist"""
    fn = load_library().uh_post_level_size
    fn.argtypes, fn.restype = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], C.c_int
    w, h = C.c_uint32(), C.c_uint32()
    if fn(int(width), int(height), int(level), C.byref(w), C.byref(h)) != 0:
        raise ValueError(f"a {width} x {height} frame has no bloom level {level}")
    return int(w.value), int(h.value)


def taa_jitter(index):
    """uh_taa_jitter: the sub-pixel offset (jx, jy) of frame `index`, Halton(2, 3) - 0.5 in pixels (needs no GPU)"""
    fn = load_library().uh_taa_jitter
    fn.argtypes, fn.restype = [C.c_uint32, C.POINTER(C.c_float * 2)], C.c_int
    out = (C.c_float * 2)()
    if fn(int(index), C.byref(out)) != 0:
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
    lib = load_library()
    fn = lib.uh_shadow_cascades
    fp = C.POINTER(C.c_float)
    fn.argtypes, fn.restype = [fp, fp, C.c_float, C.c_float, fp, C.POINTER(ShadowmapParams)], C.c_int
    view = (C.c_float * 16)(*cam.to_glam(camera.get_view()).tolist())
    proj = (C.c_float * 16)(*cam.to_glam(camera.get_projection()).tolist())
    sun = (C.c_float * 3)(*[float(x) for x in sun_dir])
    out = ShadowmapParams()
    st = fn(view, proj, float(camera.z_near), float(camera.z_far), sun, C.byref(out))
    if st != 0:
        raise UtopianError(f"uh_shadow_cascades: {ERR_NAMES.get(st, st)}")
    return out
