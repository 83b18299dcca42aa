"""GPU: the hybrid graph's marching-cubes pass (uh_render_hybrid with UH_HYBRID_MARCHING_CUBES) against the numpy restatement of
tests/marching_cubes_pass_reference.py - depth and visibility bit for bit, deferred_output within DEFERRED_ULP where it draws and
untouched elsewhere, present and sky_pixels - at t = 0 and 5, with shadows and 16 lights, at an awkward size and 1080p; the extraction
against uh_add_isosurface_mesh; the flag, bit 9, the refusals and isolation."""
import os
import re
import subprocess

import numpy as np
import pytest

import forward_reference as fw
import marching_cubes_pass_reference as mr
import rust_renderer_amd as rr
from hybrid_util import CPP_H, CPP_W, DEFERRED_ULP, ROOT, SyntheticScene, add_lights, cpp_scene, frame_view, ulps, write_blob
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import Scene, quad

pytestmark = pytest.mark.gpu
W, H = 160, 120
MC = rr.HYBRID_MARCHING_CUBES


class MarchingCubesScene(SyntheticScene):
    """the synthetic scene, a floor under the marching-cubes domain [0, 32]^3, and a quad between the camera and the domain that hides
    part of it; the camera looks at (10, 15, 10) from above the floor's far corner, so the upper rows see only sky"""

    def upload(self, renderer):
        renderer.initialize_raytracing = lambda: None  # once, after the two meshes below
        try:
            r = super().upload(renderer)
        finally:
            del renderer.initialize_raytracing
        m = rr.make_material(rr.LAMBERTIAN, 0.0, (0.7, 0.7, 0.7, 1.0), diffuse_map=renderer.default_diffuse_map())
        fv, fi = quad((-12.0, -0.5, 44.0), (56.0, 0.0, 0.0), (0.0, 0.0, -56.0), nu=4, nv=4)
        renderer.add_mesh(fv, fi, m)
        qv, qi = quad((-8.0, 6.0, 2.0), (8.0, 0.0, -8.0), (0.0, 14.0, 0.0), nu=2, nv=2)
        renderer.add_mesh(qv, qi, m)
        renderer.initialize_raytracing()
        return r


def mc_scene(width, height):
    cam = rr.camera.Camera((-30.0, 28.0, -22.0), (10.0, 15.0, 10.0), 60.0, width / height, 0.1, 1000.0)
    return MarchingCubesScene("marching_cubes", [], [], cam, dict(sky_enabled=1))


def _setup(width=W, height=H, lights=0, t=0.0, seed=3):
    scene = mc_scene(width, height)
    gpu = rr.Renderer(width, height)
    meshes, textures = fw.upload_recorded(scene, gpu, defaults=False)
    ls = add_lights(gpu, lights, seed) if lights else []
    view = frame_view(scene, width, height)
    view.num_lights = lights
    view.time = t
    view.marching_cubes_enabled = 1
    return gpu, meshes, textures, ls, view


def _extracted(t):
    """positions and normals of uh_add_isosurface_mesh(32, 0, 32, t) on a context of its own"""
    other = rr.Renderer(8, 8)
    index, tris = other.add_isosurface_mesh(32, 0.0, 32.0, t)
    vtx, idx = other.read_mesh(index)
    v = vtx[idx]
    assert len(v) == 3 * tris
    return v["pos"][:, :3].reshape(-1, 3, 3).copy(), v["normal"][:, :3].reshape(-1, 3, 3).copy()


def _images(gpu):
    return {i: gpu.read_hybrid(i) for i in range(9)}


def _frame_stats(gpu):
    s = gpu.hybrid_frame_stats()
    return s.sky_pixels, s.lights


def _shadow_input(gpu):
    return gpu.shadow_map_stats().params, np.stack([gpu.read_shadow_map(c) for c in range(4)])


def _run(gpu, meshes, textures, lights, view, base_mask=rr.HYBRID_FRAME):
    """a steady frame without the pass, then the same frame with it: checks the pass against the restatement and returns it"""
    view.marching_cubes_enabled = 1
    gpu.render_hybrid(view, base_mask)
    gpu.render_hybrid(view, base_mask)  # rt_shadows reads the previous G-buffer: the second call is the steady state
    before = _images(gpu)
    sky_before = gpu.hybrid_frame_stats().sky_pixels
    gpu.render_hybrid(view, base_mask | MC)
    after = _images(gpu)
    pos, nrm = _extracted(view.time)
    shadow = _shadow_input(gpu) if view.shadows_enabled == 1 else None
    mesh = mr.pass_mesh(pos, nrm, meshes[0])
    ref = mr.marching_cubes_pass(mesh, textures, view, lights, before[rr.HYBRID_POSITION], before[rr.HYBRID_DEFERRED_OUTPUT], shadow)
    depth, vis = gpu.read_hybrid(rr.HYBRID_DEPTH), gpu.read_hybrid(rr.HYBRID_MARCHING_CUBES_VISIBILITY)
    assert np.array_equal(vis, ref["visibility"]), f"visibility: {(vis != ref['visibility']).sum()} pixels differ"
    assert np.array_equal(depth.view(np.uint32), ref["depth"].view(np.uint32)), "depth bits"
    covered = vis != mr.NONE
    out = after[rr.HYBRID_DEFERRED_OUTPUT]
    assert np.array_equal(out[~covered], before[rr.HYBRID_DEFERRED_OUTPUT][~covered]), "untouched where the pass did not draw"
    if covered.any():
        assert np.isfinite(out[covered]).all() and (out[covered, 3] == 1.0).all()
        assert ulps(out[covered], ref["output"][covered]).max() <= DEFERRED_ULP
    assert np.array_equal(after[rr.HYBRID_PRESENT_OUTPUT], fw.present(out, view)), "the present pass on the device's deferred_output"
    miss = before[rr.HYBRID_POSITION][..., 3] == 0
    assert gpu.hybrid_frame_stats().sky_pixels == sky_before - int((miss & covered).sum()) == int((miss & ~covered).sum())
    for i in range(rr.HYBRID_SSAO_IMAGE + 1):  # the G-buffer, rt_shadows, rt_reflections and SSAO images
        assert np.array_equal(after[i], before[i]), f"hybrid image {i} changed"
    s = gpu.marching_cubes_stats()
    assert s.renders == 1 and s.triangles == len(pos) and s.pieces == len(ref["records"]) and s.covered_pixels == int(covered.sum())
    assert s.lights == view.num_lights + 1 and s.time == np.float32(view.time) and s.pass_ms > 0
    return ref, covered, before


@pytest.mark.parametrize("t,reference_triangulation", [(0.0, 1), (5.0, 1), (5.0, 0)])
def test_pass_against_the_restatement(t, reference_triangulation):
    gpu, meshes, textures, lights, view = _setup(t=t)
    # the option shapes uh_add_isosurface_mesh only: the pass extracts the reference's triangles either way
    gpu.set_option("iso_reference_triangulation", reference_triangulation)
    ref, covered, before = _run(gpu, meshes, textures, lights, view)
    assert covered.mean() > 0.02, "the isosurface is in view"
    miss = before[rr.HYBRID_POSITION][..., 3] == 0
    assert (miss & ~covered).any() and (miss & covered).any(), "sky-only pixels, and the isosurface in front of the sky"
    unseeded = fw.resolve(ref["records"], W, H)[1] != mr.NONE
    assert (unseeded & ~covered).sum() > 20, "the quad and the floor hide part of the isosurface"


def test_shadows_and_lights_at_an_awkward_size():
    gpu, meshes, textures, lights, view = _setup(97, 61, lights=16, t=5.0)
    view.shadows_enabled = 1
    gpu.set_shadowmap_params(rr.shadow_cascades(mc_scene(97, 61).camera, view.sun_dir[:]))
    gpu.render_hybrid(view, rr.HYBRID_SHADOW_MAPS)
    maps = [gpu.read_shadow_map(c) for c in range(4)]
    sm = gpu.shadow_map_stats()
    _run(gpu, meshes, textures, lights, view)
    assert all(np.array_equal(a, gpu.read_shadow_map(c)) for c, a in enumerate(maps)), "the pass renders no shadow map"
    assert gpu.shadow_map_stats().renders == sm.renders


def test_1080p():
    gpu, meshes, textures, lights, view = _setup(1920, 1080, lights=16, t=5.0)
    _, covered, _ = _run(gpu, meshes, textures, lights, view)
    assert covered.sum() > 10000


def test_flag_off_and_bit_9_are_no_ops():
    gpu, meshes, textures, lights, view = _setup()
    view.marching_cubes_enabled = 0
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    ref, stats = _images(gpu), _frame_stats(gpu)
    for mask in (rr.HYBRID_FRAME | MC, rr.HYBRID_FRAME | (1 << 9)):
        gpu.render_hybrid(view, mask)
        got = _images(gpu)
        assert all(np.array_equal(got[i], ref[i]) for i in range(9)) and _frame_stats(gpu) == stats
    view.marching_cubes_enabled = 1
    gpu.render_hybrid(view, rr.HYBRID_FRAME | (1 << 9))
    got = _images(gpu)
    assert all(np.array_equal(got[i], ref[i]) for i in range(9))
    s = gpu.marching_cubes_stats()
    assert (s.renders, s.triangles, s.pass_ms) == (0, 0, 0.0), "the pass never ran"
    with pytest.raises(UtopianError):
        gpu.read_hybrid(rr.HYBRID_DEPTH)


def _refused(gpu, view, mask, what):
    """the call is UH_ERR_INVALID_ARGUMENT with the marching-cubes pass's message naming `what`"""
    with pytest.raises(UtopianError) as e:
        gpu.render_hybrid(view, mask)
    assert re.match(r"INVALID_ARGUMENT: uh_render_hybrid: the marching-cubes pass", str(e.value)), str(e.value)
    assert what in str(e.value), str(e.value)


def test_refusals_change_nothing():
    # no mesh: refused before the build check (forward.frag reads meshes[0])
    empty = rr.Renderer(W, H)
    v = frame_view(mc_scene(W, H), W, H)
    v.marching_cubes_enabled, v.num_lights = 1, 0
    _refused(empty, v, rr.HYBRID_GBUFFER | MC, "no mesh")
    gpu, meshes, textures, lights, view = _setup(lights=2)
    _refused(gpu, view, MC | rr.HYBRID_SKY, "no G-buffer")
    with pytest.raises(UtopianError):
        gpu.read_hybrid(rr.HYBRID_POSITION)  # nothing ran: not even the first call's allocation
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    ref = _images(gpu)
    v = frame_view(mc_scene(W, H), W, H)
    v.marching_cubes_enabled, v.shadows_enabled, v.num_lights = 1, 1, 0  # no shadow map rendered
    bad = [(v, "shadow maps")]
    v = frame_view(mc_scene(W, H), W, H)
    v.marching_cubes_enabled, v.num_lights = 1, 3  # two lights added
    bad.append((v, "num_lights"))
    # masks without UH_HYBRID_DEFERRED, whose own checks would refuse the same views first
    for v, what in bad:
        for mask in (MC, MC | rr.HYBRID_SKY):
            _refused(gpu, v, mask, what)
            got = _images(gpu)
            assert all(np.array_equal(got[i], ref[i]) for i in range(9))
    assert gpu.marching_cubes_stats().renders == 0
    with pytest.raises(UtopianError):
        gpu.read_hybrid(rr.HYBRID_DEPTH)


class TieScene(Scene):
    """one quad in the plane z = 11, inside the front face of the density field's box (x in [11, 21], y in [5, 15]): the isosurface's
    triangles there lie in the same plane (their corners have density -0, so every edge point is a grid corner)"""

    def upload(self, renderer):
        m = rr.make_material(rr.LAMBERTIAN, 0.0, (0.6, 0.7, 0.8, 1.0), diffuse_map=renderer.default_diffuse_map())
        qv, qi = quad((12.0, 6.0, 11.0), (8.0, 0.0, 0.0), (0.0, 8.0, 0.0), nu=2, nv=2)
        renderer.add_mesh(qv, qi, m)
        renderer.initialize_raytracing()
        return renderer


def test_a_fragment_at_the_g_buffers_depth_is_drawn():
    # looking along +z with an axis-aligned view, depth depends on z alone: where the cast's hit lands exactly on z = 11, the seed
    # equals the isosurface fragment's depth, and LESS_OR_EQUAL draws the fragment
    w, h = 96, 64
    cam = rr.camera.Camera((16.0, 10.0, -20.0), (16.0, 10.0, 16.0), 40.0, w / h, 0.1, 1000.0)
    scene = TieScene("tie", [], [], cam, dict(sky_enabled=1))
    gpu = rr.Renderer(w, h)
    meshes, textures = fw.upload_recorded(scene, gpu, defaults=True)
    view = frame_view(scene, w, h)
    view.num_lights, view.time, view.marching_cubes_enabled = 0, 0.0, 1
    ref, covered, before = _run(gpu, meshes, textures, [], view)
    depth0, vis0, _ = fw.resolve(ref["records"], w, h)
    ties = (vis0 != mr.NONE) & (ref["seed"].view(np.uint32) == depth0.view(np.uint32))
    assert ties.sum() > 10, "some hits land exactly on the plane"
    vis = gpu.read_hybrid(rr.HYBRID_MARCHING_CUBES_VISIBILITY)
    assert np.array_equal(vis[ties], vis0[ties]), "the seed loses ties"


def test_cpp_mirror_renders_what_the_python_layer_renders(tmp_path):
    exe = str(tmp_path / "marching_cubes_host")
    libdir = os.path.dirname(rr.api.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "marching_cubes_host.cpp"), "-o", exe, "-L", libdir, "-lutopian_hip",
                    f"-Wl,-rpath,{libdir}"], check=True)
    meshes = cpp_scene()
    cam = rr.camera.Camera((-30.0, 28.0, -22.0), (10.0, 15.0, 10.0), 60.0, CPP_W / CPP_H, 0.1, 1000.0)
    view = rr.default_view(cam, CPP_W, CPP_H)
    view.shadows_enabled = view.ibl_enabled = view.cubemap_enabled = 0
    view.marching_cubes_enabled, view.time = 1, 5.0
    blob, out = tmp_path / "scene.blob", tmp_path / "out.bin"
    write_blob(blob, meshes, view)
    res = subprocess.run([exe, str(blob), str(out)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    r = rr.Renderer(CPP_W, CPP_H)
    white = r.default_diffuse_map()
    for vert, idx, kind, base in meshes:
        r.add_mesh(vert, idx, rr.make_material(kind, 0.0, base, diffuse_map=white))
    r.initialize_raytracing()
    r.render_hybrid(view, rr.HYBRID_FRAME | MC)
    want = b"".join(r.read_hybrid(k).tobytes() for k in (rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_DEPTH, rr.HYBRID_MARCHING_CUBES_VISIBILITY))
    assert np.fromfile(out, np.uint8).tobytes() == want
    s = r.marching_cubes_stats()
    assert s.covered_pixels > 0
    assert f"renders {s.renders} triangles {s.triangles} pieces {s.pieces} covered {s.covered_pixels} lights {s.lights}" in res.stdout


def test_isolation_from_the_other_graphs():
    gpu, meshes, textures, lights, view = _setup(t=5.0)
    loop = rr.FrameLoop(gpu, view)
    loop.frame(rr.PASS_ALL)
    acc, stats = gpu.read_accumulation(), gpu.get_stats()
    gpu.render_forward(view, rr.FORWARD_PASS | rr.FORWARD_PRESENT)
    fwd = [gpu.read_forward(i) for i in range(4)]
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    hs = gpu.hybrid_stats()
    gpu.render_hybrid(view, rr.HYBRID_FRAME | MC)
    assert gpu.marching_cubes_stats().covered_pixels > 0
    assert np.array_equal(gpu.read_accumulation(), acc) and gpu.get_stats().path_rays == stats.path_rays
    assert all(np.array_equal(gpu.read_forward(i), a) for i, a in enumerate(fwd))
    h2 = gpu.hybrid_stats()
    assert list(h2.rays) == list(hs.rays) and h2.reflection_pixels == hs.reflection_pixels
    assert gpu.shadow_map_stats().renders == 0
