"""Shared helpers of the hybrid graph's tests (uh_render_hybrid: test_gpu_hybrid*.py, test_gpu_ibl.py, test_hybrid_cpp.py and the CPU
tests of its passes): the scenes, a GPU renderer next to the oracle, the views, image reads and distances, the tolerances, the lights,
one frame checked pass by pass, the C++ host program and the log of measured values. Not a conftest: test modules import it."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hybrid_frame_reference as fr
import hybrid_reference as hr
import ibl_reference as ir
import oracle_api as oa
import rust_renderer_amd as rr
from rust_renderer_amd.scenes import Scene, icosphere, procedural_texture, quad
from util import reference_cornell_scene, reference_spheres_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 120
OUT = os.environ.get("HYBRID_FRAME_RECORD")  # a directory: the measured errors and pass times are appended there (record)
# deferred output against the reference: device powf (spot lights) is not correctly rounded; measured 0 ulp at up to 12 lights,
# 3 ulp at 1,024 lights (512 spot lights)
DEFERRED_ULP = 4
# the IBL consumers read the device's maps with the same arithmetic as the restatement
CONSUMER_ULP = DEFERRED_ULP


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def assets():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_assets.npz"))


def _normal_map(size=32):
    """a bumpy tangent-space normal map (z dominant), RGBA8"""
    y, x = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
    nx, ny = 0.45 * np.sin(x * 0.7), 0.45 * np.cos(y * 0.5)
    nz = np.sqrt(np.maximum(1.0 - nx * nx - ny * ny, 0.0))
    rgba = np.stack([(nx * 0.5 + 0.5) * 255, (ny * 0.5 + 0.5) * 255, (nz * 0.5 + 0.5) * 255, np.full_like(nx, 255)], axis=-1)
    return np.ascontiguousarray(np.rint(rgba).astype(np.uint8))


class SyntheticScene(Scene):
    """mesh 0: a metal, normal-mapped floor (tangent (1, 0, 0)) - material 0 is metal, so the sky pixels trace too; mesh 1: a
    Lambertian sphere under a rotated, non-uniformly scaled instance, tangent zero; mesh 2: a normal-mapped box-side quad under another
    rotation and scale, textured maps everywhere; mesh 3: a metal sphere. The upper rows see the sky."""

    def upload(self, renderer):
        renderer.default_diffuse_map()
        tex = [renderer.add_texture(procedural_texture(11, k, 32)) for k in range(4)]
        nmap = renderer.add_texture(_normal_map())

        def mat(kind, diffuse, normal, base=(1.0, 1.0, 1.0, 1.0)):
            m = rr.make_material(kind, 0.0, base, diffuse_map=diffuse)
            m.normal_map, m.metallic_roughness_map, m.occlusion_map = normal, tex[2], tex[3]
            return m

        fv, fi = quad((-6.0, 0.0, 6.0), (12.0, 0.0, 0.0), (0.0, 0.0, -12.0), nu=6, nv=6, uv_scale=(3.0, 3.0))
        fv["tangent"][:, :3] = (1.0, 0.0, 0.0)
        renderer.add_mesh(fv, fi, mat(rr.METAL, tex[0], nmap, (0.9, 0.8, 0.7, 1.0)))
        sv, si = icosphere(2)
        rot = np.array([[0.8, -0.6, 0.0], [0.6, 0.8, 0.0], [0.0, 0.0, 1.0]], np.float32)
        renderer.add_mesh(sv, si, mat(rr.LAMBERTIAN, tex[1], nmap, (0.5, 0.9, 0.4, 1.0)), rr.transform3x4((1.4, 0.6, 0.9), (-1.5, 0.8, 0.0), rot))
        qv, qi = quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), nu=3, nv=3, uv_scale=(2.0, 2.0))
        qv["tangent"][:, :3] = (1.0, 0.0, 0.0)
        rot2 = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]], np.float32) @ np.array([[0.96, 0.0, -0.28], [0.0, 1.0, 0.0], [0.28, 0.0, 0.96]], np.float32)
        renderer.add_mesh(qv, qi, mat(rr.LAMBERTIAN, tex[2], nmap), rr.transform3x4((1.0, 0.7, 1.6), (2.2, 1.0, -1.0), rot2))
        renderer.add_mesh(sv, si, mat(rr.METAL, tex[3], nmap), rr.transform3x4((0.7, 0.7, 0.7), (0.6, 0.7, 1.4)))
        renderer.initialize_raytracing()
        return renderer


def synthetic_scene():
    cam = rr.camera.Camera((0.0, 2.2, 6.5), (0.0, 0.9, 0.0), 60.0, W / H, 0.01, 1000.0)
    return SyntheticScene("hybrid_synthetic", [], [], cam, dict(sky_enabled=1))


def scene_named(name, assets):
    return {"cornell": lambda: reference_cornell_scene(assets), "spheres": lambda: reference_spheres_scene(assets), "synthetic": synthetic_scene}[name]()


def pair(scene, width=W, height=H):
    """the scene on a GPU renderer and on the oracle (Renderer.initialize's default maps first, except for the synthetic scene), and
    the meshes as the GPU's add_mesh received them"""
    defaults = not isinstance(scene, SyntheticScene)
    gpu = rr.Renderer(width, height)
    meshes = hr.upload_recorded(scene, gpu, defaults)
    cpu = oa.OracleRenderer(width, height)
    hr.upload_recorded(scene, cpu, defaults)
    return gpu, cpu, meshes


# ---- views: the reference's flags that this library refuses cleared (see utopian_hip.h) ------------------------------------------
def hybrid_view(scene, width=W, height=H, **kw):
    v = scene.make_view(width, height, **kw)
    v.ibl_enabled = 0  # the reflection pass's non-IBL branch
    return v


def frame_view(scene, width=W, height=H, **kw):
    v = scene.make_view(width, height, **kw)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    return v


def unit_sun(view):
    s = np.array(view.sun_dir[:], np.float64)
    view.sun_dir[:] = tuple(np.float32(s / np.linalg.norm(s)))
    return view


def ibl_view(scene, width=W, height=H, **kw):
    v = scene.make_view(width, height, **kw)
    v.shadows_enabled = 0
    v.ibl_enabled = v.cubemap_enabled = 1
    return unit_sun(v)


# ---- images -------------------------------------------------------------------------------------------------------------------------
def read_all(r):
    return {i: r.read_hybrid(i) for i in range(9)}


def gbuf(r):
    return dict(position=r.read_hybrid(rr.HYBRID_POSITION), normal=r.read_hybrid(rr.HYBRID_NORMAL), albedo=r.read_hybrid(rr.HYBRID_ALBEDO),
                pbr=r.read_hybrid(rr.HYBRID_PBR))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulps(a, b):
    """distance in float32 units in the last place (same-sign values; either sign of zero is 0)"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def record(log, name, **values):
    """appends one line of measured values to OUT/<log>_measured.txt (log: "hybrid_frame" or "ibl"), when OUT is set"""
    if not OUT:
        return
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"{log}_measured.txt"), "a") as f:
        f.write(f"{name} " + " ".join(f"{k}={v}" for k, v in values.items()) + "\n")


# ---- the passes against the references ----------------------------------------------------------------------------------------------
def add_lights(gpu, n, seed, kinds=(1, 2)):
    """n GpuLight records (point, spot, directional or an unknown type, by `kinds`) above the synthetic scene; the renderer's tree is rebuilt"""
    rng = np.random.default_rng(seed)
    lights = []
    for k in range(n):
        l = rr.make_light(rng.uniform((-4.0, 0.5, -4.0), (4.0, 4.0, 3.0)), color=tuple(rng.uniform(0.2, 1.0, 3)))
        l.light_type = float(kinds[k % len(kinds)])
        l.attenuation[:] = (float(rng.uniform(0.5, 1.0)), float(rng.uniform(0.0, 0.3)), float(rng.uniform(0.05, 0.4)))
        l.direction[:] = tuple(rng.uniform(-1.0, 1.0, 3) + np.array([0.0, -1.5, 0.0]))
        l.spot = float(rng.uniform(1.0, 16.0))
        gpu.add_gpu_light(l)
        lights.append(l)
    gpu.initialize_raytracing()
    return lights


def assert_reflections(got, ref, kind):
    assert np.array_equal(got[kind == 0], ref[kind == 0]) and not got[kind == 0].any(), "non-metal pixels are exactly 0"
    assert np.array_equal(got[kind == 1], ref[kind == 1]), "pixels whose ray hits are byte-identical"
    d = np.abs(got[kind == 2].astype(np.int16) - ref[kind == 2].astype(np.int16))
    assert d.size == 0 or d.max() <= 1, "sky pixels within 1 LSB"
    assert (got[..., 3] == 0).all()


def check_frame(gpu, cpu, meshes, view, lights, name):
    """one UH_HYBRID_FRAME call, then each pass against the reference on the device's own inputs"""
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    g = gbuf(gpu)
    sh, refl = gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS)
    ss, d, p = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
    # SSAO: exact
    assert np.array_equal(ss, fr.ssao(g["position"], g["normal"], view)), "ssao"
    # deferred: the geometry pixels (the sky pass overwrites the others)
    ref = fr.deferred(g, sh, refl, ss, view, meshes, lights)
    geo = g["position"][..., 3] == 1.0
    u = ulps(d[geo], ref[geo])
    assert geo.any() and np.isfinite(d[geo]).all()
    record("hybrid_frame", name, deferred_max_ulp=int(u.max()), deferred_exact=float((u == 0).mean()))
    assert u.max() <= DEFERRED_ULP, f"deferred: {u.max()} ulp"
    # sky: within 1 LSB after present's conversion
    sky = fr.sky(g["position"], view)
    if sky:
        ys, xs = np.array(list(sky)).T
        want = np.array(list(sky.values()), np.float32)
        got = d[ys, xs, :3]
        assert (d[ys, xs, 3] == 1.0).all()
        assert np.abs(hr.unorm8(fr.linear_to_srgb(got)).astype(int) - hr.unorm8(fr.linear_to_srgb(want)).astype(int)).max() <= 1
        assert np.allclose(got, want, rtol=1e-4, atol=1e-6)
    # present: exact given the device's deferred output
    assert np.array_equal(p, fr.present(d, view.fxaa_enabled == 1)), "present"
    s = gpu.hybrid_frame_stats()
    assert all(ms > 0 for ms in s.pass_ms) and s.sky_pixels == len(sky) and s.lights == view.num_lights + 1
    return g, d, p


def check_ibl_frame(gpu, cpu, meshes, view, maps, name):
    """one UH_HYBRID_FRAME call with the IBL maps `maps` built, then its IBL consumers against the restatement on the device's inputs"""
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    g = gbuf(gpu)
    sh, refl = gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS)
    ss, d = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    # rt_reflections with IBL: hits shaded by imageBasedLighting, misses the sky as before
    want_refl, kind = ir.reflections_ibl(cpu, meshes, g["position"], g["normal"], g["pbr"], view, maps)
    diff = np.abs(refl.astype(int) - want_refl.astype(int))
    assert diff.max() <= 1, (name, diff.max())
    # deferred with IBL on the geometry pixels
    ref = ir.deferred_ibl(g, sh, refl, ss, view, meshes, [], maps)
    geo = g["position"][..., 3] == 1.0
    u = ulps(d[geo], ref[geo])
    assert geo.any() and np.isfinite(d[geo]).all()
    assert u.max() <= CONSUMER_ULP, (name, u.max())
    # the sky from the cube
    sky = ir.sky_cube(g["position"], view, maps["env"])
    if sky:
        ys, xs = np.array(list(sky)).T
        want = np.array(list(sky.values()), np.float32)
        assert np.allclose(d[ys, xs, :3], want, rtol=1e-5, atol=1e-7), name
    record("ibl", name, deferred_max_ulp=int(u.max()), reflection_hits=int((kind == 1).sum()), sky=len(sky), refl_max_lsb=int(diff.max()))
    return g, d


# ---- small frames of infinite planes, cast on the host (the CPU tests of the passes) ------------------------------------------------
def plane_view(eye, target, width, height):
    cam = rr.camera.Camera(eye, target, 60.0, width / height, 0.01, 1000.0)
    v = rr.default_view(cam, width, height)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 0
    return v


def cast_planes(view, planes, width, height):
    """position and normal targets of a scene of infinite planes (point, normal): the nearest along each primary ray"""
    pos = np.tile(np.array([1, 1, 1, 0], np.float32), (height, width, 1))
    nrm = pos.copy()
    for y in range(height):
        for x in range(width):
            r = oa.primary_ray(view, width, height, x, y, 0.5, 0.5).astype(np.float64)
            best = None
            for p0, n in planes:
                den = np.dot(r[3:], n)
                if abs(den) < 1e-9:
                    continue
                t = np.dot(np.asarray(p0) - r[:3], n) / den
                if t > 0 and (best is None or t < best[0]):
                    best = (t, n)
            if best:
                pos[y, x, :3], pos[y, x, 3] = r[:3] + best[0] * r[3:], 1.0
                nrm[y, x, :3], nrm[y, x, 3] = best[1], 1.0
    return pos, nrm


# ---- the C++ host mirror (include/utopian_host.hpp, tests/cpp/hybrid_host.cpp) ------------------------------------------------------
CPP_W, CPP_H = 96, 64


def build_cpp(tmp_path):
    exe = str(tmp_path / "hybrid_host")
    libdir = os.path.dirname(rr.api.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "hybrid_host.cpp"),
                    "-o", exe, "-L", libdir, "-lutopian_hip", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def cpp_scene():
    """(vertices, indices, material type, base colour) per mesh, identity transforms: a metal floor, a Lambertian sphere, a metal sphere"""
    fv, fi = quad((-5.0, 0.0, 5.0), (10.0, 0.0, 0.0), (0.0, 0.0, -10.0), nu=4, nv=4)
    sv, si = icosphere(2)
    sv2 = sv.copy()
    sv["pos"][:, :3] = sv["pos"][:, :3] * 0.8 + np.array([-1.0, 0.8, 0.0], np.float32)
    sv2["pos"][:, :3] = sv2["pos"][:, :3] * 0.6 + np.array([1.0, 0.6, 0.5], np.float32)
    return [(fv, fi, rr.METAL, (0.9, 0.9, 0.9, 1.0)), (sv, si, rr.LAMBERTIAN, (0.8, 0.3, 0.2, 1.0)), (sv2, si, rr.METAL, (1.0, 1.0, 1.0, 1.0))]


def cpp_view():
    cam = rr.camera.Camera((0.0, 2.0, 5.0), (0.0, 0.7, 0.0), 60.0, CPP_W / CPP_H, 0.01, 1000.0)
    v = rr.default_view(cam, CPP_W, CPP_H)
    v.ibl_enabled = 0
    return v


def write_blob(path, meshes, v):
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x44594855, CPP_W, CPP_H))
        f.write(bytes(v))
        f.write(struct.pack("<I", len(meshes)))
        for vert, idx, kind, base in meshes:
            f.write(struct.pack("<III4f", len(vert), len(idx), kind, *base))
            f.write(np.ascontiguousarray(vert).tobytes())
            f.write(np.ascontiguousarray(idx, dtype=np.uint32).tobytes())


def run_cpp(tmp_path, mode, meshes, view, timeout=120):
    """the host program in `mode` on the blob of (meshes, view): its completed process and the bytes it wrote; then the same meshes
    on a ctypes renderer, for the caller to render and compare"""
    exe = build_cpp(tmp_path)
    blob, out = tmp_path / "scene.blob", tmp_path / "out.bin"
    write_blob(blob, meshes, view)
    res = subprocess.run([exe, mode, str(blob), str(out)], capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr
    r = rr.Renderer(CPP_W, CPP_H)
    white = r.default_diffuse_map()
    for vert, idx, kind, base in meshes:
        r.add_mesh(vert, idx, rr.make_material(kind, 0.0, base, diffuse_map=white))
    r.initialize_raytracing()
    return res, np.fromfile(out, dtype=np.uint8), r
