"""GPU: the forward graph (uh_render_forward) against the numpy restatement of tests/forward_reference.py - depth and visibility bit
for bit, forward_output within DEFERRED_ULP, the present image exactly - on the synthetic (normal-mapped) scene and the reference's
assets, at awkward sizes and 1080p, with 0 / 16 / 1,024 lights, with shadows, after a moved instance and under a floor beyond the guard
band; the visibility against the tracer's primary hits; the C++ mirror; refusals and isolation."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forward_reference as fw
import oracle_api as oa
import rust_renderer_amd as rr
from hybrid_util import DEFERRED_ULP, CPP_H, CPP_W, ROOT, SyntheticScene, add_lights, assets, cpp_scene, cpp_view, frame_view, read_all, scene_named, \
    synthetic_scene, ulps, write_blob
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import Scene, quad

pytestmark = pytest.mark.gpu
W, H = 160, 120


def _setup(scene, width=W, height=H, lights=0, seed=5):
    gpu = rr.Renderer(width, height)
    meshes, textures = fw.upload_recorded(scene, gpu, defaults=not isinstance(scene, SyntheticScene))
    ls = add_lights(gpu, lights, seed) if lights else []
    view = frame_view(scene, width, height)
    view.num_lights = lights
    return gpu, meshes, textures, ls, view


def _check(gpu, meshes, textures, lights, view, shadow=None):
    """the device's four images against the restatement; returns the restatement"""
    Wd, Hd = gpu.width, gpu.height
    ref = fw.forward(meshes, textures, view, lights, Wd, Hd, shadow)
    depth, vis = gpu.read_forward(rr.FORWARD_DEPTH), gpu.read_forward(rr.FORWARD_VISIBILITY)
    assert np.array_equal(vis, ref["visibility"]), f"visibility: {(vis != ref['visibility']).sum()} pixels differ"
    assert np.array_equal(depth.view(np.uint32), ref["depth"].view(np.uint32)), "depth bits"
    out = gpu.read_forward(rr.FORWARD_OUTPUT)
    covered = vis != fw.NONE
    assert np.array_equal(out[~covered], ref["output"][~covered]), "the clear colour where nothing was drawn"
    if covered.any():
        assert np.isfinite(out[covered]).all()
        assert ulps(out[covered], ref["output"][covered]).max() <= DEFERRED_ULP
    present = gpu.read_forward(rr.FORWARD_PRESENT_OUTPUT)
    assert np.array_equal(present, fw.present(out, view)), "the present pass on the device's forward_output"
    restated = fw.present(ref["output"], view)
    assert (np.abs(present.astype(int) - restated.astype(int)) <= 1).all() and (present != restated).mean() < 1e-3
    s = gpu.forward_stats()
    assert s.pieces == len(ref["records"]) and s.covered_pixels == int(covered.sum()) and s.lights == view.num_lights + 1
    return ref


def _shadow_input(gpu):
    return gpu.shadow_map_stats().params, np.stack([gpu.read_shadow_map(c) for c in range(4)])


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (257, 129), (W, H)])
def test_synthetic_scene_at_awkward_sizes(size):
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene, *size)
    gpu.render_forward(view, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    _check(gpu, meshes, textures, lights, view)


def test_synthetic_scene_at_1080p():
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene, 1920, 1080, lights=16)
    gpu.render_forward(view, rr.FORWARD_GRAPH)
    ref = _check(gpu, meshes, textures, lights, view)
    assert (ref["visibility"] != fw.NONE).mean() > 0.4


@pytest.mark.parametrize("n", [16, 1024])
def test_lights(n):
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene, lights=n, seed=n)
    gpu.render_forward(view)
    _check(gpu, meshes, textures, lights, view)


def test_shadows_enabled():
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene, lights=4)
    view.shadows_enabled = 1
    gpu.set_option("shadow_map_size", 512)
    gpu.set_shadowmap_params(rr.shadow_cascades(scene.camera, view.sun_dir[:]))
    gpu.render_forward(view, rr.FORWARD_GRAPH)
    assert gpu.shadow_map_stats().renders == 1 and gpu.forward_stats().pass_ms[0] > 0
    _check(gpu, meshes, textures, lights, view, _shadow_input(gpu))
    gpu.render_forward(view, rr.FORWARD_PASS)  # the maps of the earlier call
    assert gpu.shadow_map_stats().renders == 1 and gpu.forward_stats().pass_ms[0] == 0
    _check(gpu, meshes, textures, lights, view, _shadow_input(gpu))


@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_reference_assets(name, assets):
    scene = scene_named(name, assets)
    gpu, meshes, textures, lights, view = _setup(scene)
    gpu.render_forward(view)
    _check(gpu, meshes, textures, lights, view)


def test_moved_instance_after_refit():
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene)
    gpu.render_forward(view)
    w = rr.transform3x4((1.2, 0.6, 0.9), (-0.7, 1.1, 0.4), np.array([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], np.float32))
    gpu.set_instance_transform(1, w)
    meshes[1]["world"] = w.copy()
    view.rebuild_tlas = 1
    gpu.render_forward(view)
    _check(gpu, meshes, textures, lights, view)


class _HugeFloor(Scene):
    def upload(self, renderer):
        renderer.default_diffuse_map()
        fv, fi = quad((-30000.0, 0.0, 30000.0), (60000.0, 0.0, 0.0), (0.0, 0.0, -60000.0))
        renderer.add_mesh(fv, fi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.8, 0.8, 1.0)))
        bv, bi = quad((-0.5, 0.8, 0.5), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0))
        renderer.add_mesh(bv, bi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.3, 0.3, 1.0)))
        renderer.initialize_raytracing()
        return renderer


def test_floor_beyond_the_guard_band():
    cam = rr.camera.Camera((0.0, 2.0, 3.0), (0.0, 0.5, 0.0), 60.0, W / H, 0.3, 100000.0)
    scene = _HugeFloor("huge_floor", [], [], cam, dict(sky_enabled=1))
    gpu, meshes, textures, lights, view = _setup(scene)
    gpu.render_forward(view)
    ref = _check(gpu, meshes, textures, lights, view)
    assert len(ref["records"]) > 2, "the floor was clipped into pieces"
    assert (ref["visibility"] == 0).mean() > 0.3


class _Behind(Scene):
    def upload(self, renderer):
        renderer.default_diffuse_map()
        v, i = quad((-1.0, -1.0, 5.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0))
        renderer.add_mesh(v, i, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.8, 0.8, 1.0)))
        renderer.initialize_raytracing()
        return renderer


def test_nothing_in_view_leaves_the_clear_values():
    cam = rr.camera.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 60.0, W / H, 0.1, 100.0)
    scene = _Behind("behind", [], [], cam, dict(sky_enabled=1))
    gpu, meshes, textures, lights, view = _setup(scene)
    gpu.render_forward(view)
    assert (gpu.read_forward(rr.FORWARD_OUTPUT) == np.array([1, 1, 1, 0], np.float32)).all()
    assert (gpu.read_forward(rr.FORWARD_DEPTH) == 1.0).all()
    assert (gpu.read_forward(rr.FORWARD_VISIBILITY) == fw.NONE).all()
    s = gpu.forward_stats()
    assert s.pieces == 0 and s.covered_pixels == 0 and s.renders == 1
    _check(gpu, meshes, textures, lights, view)


def test_visibility_agrees_with_the_tracers_primary_hits():
    Wd, Hd = 257, 129
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene, Wd, Hd)
    gpu.render_forward(view, rr.FORWARD_PASS)
    ref = fw.forward(meshes, textures, view, lights, Wd, Hd)
    vis = gpu.read_forward(rr.FORWARD_VISIBILITY)
    rays = np.zeros((Wd * Hd, 8), np.float32)
    for pix in range(Wd * Hd):
        rays[pix, :3], rays[pix, 4:7] = np.split(np.asarray(oa.primary_ray(view, Wd, Hd, pix % Wd, pix // Wd, 0.5, 0.5), np.float32), 2)
    rays[:, 3], rays[:, 7] = 0.001, 10000.0
    _, mesh, prim = gpu.trace_closest(rays)
    tmesh, tprim = fw.triangle_of(meshes)
    v = vis.reshape(-1)
    cov = v != fw.NONE
    fm = np.where(cov, tmesh[np.where(cov, v, 0)], -1)
    fp = np.where(cov, tprim[np.where(cov, v, 0)], -1)
    tm = np.where(mesh == 0xFFFFFFFF, -1, mesh.astype(np.int64))
    same = (fm == tm) & ((fp == prim.astype(np.int64)) | ~cov)
    assert same[cov].mean() >= 0.995
    # a mismatch lies within one pixel of a triangle edge: a neighbour in the 3 x 3 window shows another draw index
    pad = np.pad(vis.astype(np.int64), 1, mode="edge")
    edge = np.zeros((Hd, Wd), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            edge |= pad[1 + dy:1 + dy + Hd, 1 + dx:1 + dx + Wd] != vis
    assert edge.reshape(-1)[~same].all()
    # world positions away from edges against the G-buffer cast's
    gpu.render_hybrid(view, rr.HYBRID_GBUFFER)
    gp = gpu.read_hybrid(rr.HYBRID_POSITION).reshape(-1, 4)[:, :3]
    pix = ref["pixels"]
    keep = ~edge.reshape(-1)[pix] & same[pix]
    # within 1e-5 of the scene's extent plus what the 8-bit snap may move a pixel's point by: a vertex moves by up to 1/512 pixel, so
    # the point by up to that share of the pixel's world footprint (its G-buffer neighbours' distance; doubled for the two axes)
    extent = 12.0  # the synthetic scene's floor
    g = gp.reshape(Hd, Wd, 3)
    step = np.zeros((Hd, Wd))
    step[:, :-1] = np.maximum(step[:, :-1], np.linalg.norm(g[:, 1:] - g[:, :-1], axis=-1))
    step[:-1] = np.maximum(step[:-1], np.linalg.norm(g[1:] - g[:-1], axis=-1))
    err = np.abs(ref["position"][keep] - gp[pix[keep]]).max(-1)
    bound = 1e-5 * extent + step.reshape(-1)[pix[keep]] / 256.0
    assert (err <= bound).all(), (err - bound).max()
    assert np.median(err) <= 1e-5 * extent


def test_refusals_leave_every_image_unchanged():
    scene = synthetic_scene()
    gpu, meshes, textures, lights, view = _setup(scene)
    with pytest.raises(UtopianError):
        gpu.read_forward(rr.FORWARD_OUTPUT)  # before the first render
    assert gpu.forward_stats().renders == 0
    gpu.render_forward(view)
    before = [gpu.read_forward(k).copy() for k in range(4)]
    bad = []
    v = frame_view(scene, W, H)
    v.shadows_enabled = 1  # no shadow map was ever rendered
    bad.append(v)
    v = frame_view(scene, W, H)
    v.num_lights = 3  # no light was added
    bad.append(v)
    for v in bad:
        with pytest.raises(UtopianError):
            gpu.render_forward(v, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    v = frame_view(scene, W, H)
    v.shadows_enabled = 1
    with pytest.raises(UtopianError):
        gpu.render_forward(v, rr.FORWARD_GRAPH)  # shadow maps before any params
    lib = rr.load_library()
    lib.uh_render_forward.argtypes, lib.uh_render_forward.restype = [C.c_void_p, C.c_void_p, C.c_uint32], C.c_int
    assert lib.uh_render_forward(gpu._ctx, None, rr.FORWARD_GRAPH) == 1
    for k in range(4):
        assert np.array_equal(gpu.read_forward(k), before[k])
    assert gpu.forward_stats().renders == 1
    fresh = rr.Renderer(W, H)
    fresh.default_diffuse_map()
    with pytest.raises(UtopianError, match="uh_build_acceleration"):
        fresh.render_forward(frame_view(scene, W, H))


def test_forward_call_changes_no_hybrid_frame():
    frames = []
    for between in (False, True):
        scene = synthetic_scene()
        gpu, meshes, textures, lights, view = _setup(scene, lights=3)
        gpu.render_hybrid(view, rr.HYBRID_FRAME)
        stats = (bytes(gpu.hybrid_stats())[:24], gpu.hybrid_frame_stats().lights, gpu.hybrid_frame_stats().sky_pixels)
        if between:
            gpu.render_forward(view)
        assert (bytes(gpu.hybrid_stats())[:24], gpu.hybrid_frame_stats().lights, gpu.hybrid_frame_stats().sky_pixels) == stats
        gpu.render_hybrid(view, rr.HYBRID_FRAME)
        frames.append(read_all(gpu))
    for k in frames[0]:
        assert np.array_equal(frames[0][k], frames[1][k]), k


def test_cpp_mirror_renders_what_the_python_layer_renders(tmp_path):
    exe = str(tmp_path / "forward_host")
    libdir = os.path.dirname(rr.api.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "forward_host.cpp"),
                    "-o", exe, "-L", libdir, "-lutopian_hip", f"-Wl,-rpath,{libdir}"], check=True)
    meshes, view = cpp_scene(), cpp_view()
    view.shadows_enabled = 0
    blob, out = tmp_path / "scene.blob", tmp_path / "out.bin"
    write_blob(blob, meshes, view)
    res = subprocess.run([exe, str(blob), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    r = rr.Renderer(CPP_W, CPP_H)
    white = r.default_diffuse_map()
    for vert, idx, kind, base in meshes:
        r.add_mesh(vert, idx, rr.make_material(kind, 0.0, base, diffuse_map=white))
    r.initialize_raytracing()
    r.render_forward(view, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    want = b"".join(r.read_forward(k).tobytes() for k in range(4))
    assert np.fromfile(out, np.uint8).tobytes() == want
    assert f"covered {r.forward_stats().covered_pixels}" in res.stdout
