"""GPU: the hybrid graph's final frame (uh_render_hybrid's SSAO, deferred, sky and present passes) against the CPU reference of
tests/hybrid_frame_reference.py, one pass at a time on the device's own input images; the image orientation, the refusals and gates,
UH_HYBRID_FRAME against the passes one by one, isolation from the path tracer and the ray-traced passes, 1080p and 1,024 lights, and
the C++ mirror."""
import numpy as np
import pytest

import hybrid_frame_reference as fr
import hybrid_reference as hr
import rust_renderer_amd as rr
from hybrid_util import (DEFERRED_ULP, W, H, add_lights, assets, check_frame, cpp_scene, cpp_view, frame_view, gbuf, pair, read_all,  # noqa: F401
                         record, run_cpp, scene_named, synthetic_scene, ulps)
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import Mesh, Model, Scene, quad
from util import reference_spheres_scene

pytestmark = pytest.mark.gpu


# ---- 1. every pass against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "spheres", "synthetic"])
def test_each_pass_equals_the_reference(assets, name):
    scene = scene_named(name, assets)
    gpu, cpu, meshes = pair(scene)
    view = frame_view(scene)
    view.num_lights = 0
    check_frame(gpu, cpu, meshes, view, [], name)
    gpu.render_hybrid(view, rr.HYBRID_FRAME)  # again, now rt_shadows reads this camera's G-buffer
    check_frame(gpu, cpu, meshes, view, [], name + "-second")


@pytest.mark.parametrize("kinds", [(1, 2), (0, 1, 2, 5)])
def test_point_spot_directional_and_unknown_lights_equal_the_reference(kinds):
    scene = synthetic_scene()
    gpu, cpu, meshes = pair(scene)
    lights = add_lights(gpu, 12, 3, kinds)
    view = frame_view(scene)
    view.num_lights = len(lights)
    check_frame(gpu, cpu, meshes, view, lights, f"lights{kinds}")
    view.num_lights = 5  # fewer than added: the first five, in order
    check_frame(gpu, cpu, meshes, view, lights, f"lights{kinds}-5")


# ---- 2. orientation -------------------------------------------------------------------------------------------------------
def _crease_scene(top):
    """a back wall facing the camera and a slab meeting it at the top (or the bottom) of the view: one inside corner"""
    # one cell each, off-centre: no primary ray meets a shared triangle edge exactly (such a ray misses both triangles, a sky texel)
    wv, wi = quad((-23.0, -19.0, -3.0), (41.0, 0.0, 0.0), (0.0, 43.0, 0.0))
    wv["normal"][:, :3] = (0.0, 0.0, 1.0)
    y = 1.0 if top else -1.0
    sv, si = quad((-21.3, y, 0.1), (43.0, 0.0, 0.0), (0.0, 0.0, -3.3))
    sv["normal"][:, :3] = (0.0, -1.0 if top else 1.0, 0.0)
    cam = rr.camera.Camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 60.0, W / H, 0.01, 1000.0)
    return Scene("crease", [(Model([Mesh(wv, wi, rr.LAMBERTIAN), Mesh(sv, si, rr.LAMBERTIAN)], []), None)], [], cam)


@pytest.mark.parametrize("top", [True, False])
def test_a_crease_at_the_top_darkens_only_the_top_of_the_present_image(top):
    scene = _crease_scene(top)
    gpu, cpu, meshes = pair(scene)
    on, off = frame_view(scene, raytracing_supported=0, fxaa_enabled=0), frame_view(scene, raytracing_supported=0, fxaa_enabled=0, ssao_enabled=0)
    gpu.render_hybrid(off, rr.HYBRID_FRAME)
    bright = gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
    gpu.render_hybrid(on, rr.HYBRID_FRAME)
    dark = gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
    rows = np.nonzero((dark[..., :3].astype(int) < bright[..., :3].astype(int)).any(axis=(1, 2)))[0]
    assert rows.size > 0
    assert (rows < H // 2).all() if top else (rows >= H // 2).all(), rows
    # and the path tracer's orientation: its G-buffer position has the slab in the same rows
    gpu.render_frame(on, rr.PASS_GBUFFER)
    slab = np.abs(gpu.read_gbuffer_position()[..., 1] - (1.0 if top else -1.0)) < 1e-4
    assert slab.any() and ((np.nonzero(slab)[0] < H // 2).all() if top else (np.nonzero(slab)[0] >= H // 2).all())


# ---- 3. refusals and gates ------------------------------------------------------------------------------------------------
def test_refusals_run_nothing():
    scene = synthetic_scene()
    gpu, cpu, meshes = pair(scene)
    v = frame_view(scene)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    before = read_all(gpu)
    cases = [("shadows_enabled", rr.HYBRID_DEFERRED, "shadow maps"), ("ibl_enabled", rr.HYBRID_DEFERRED, "IBL"),
             ("cubemap_enabled", rr.HYBRID_SKY, "environment cube"), ("num_lights", rr.HYBRID_DEFERRED, "num_lights")]
    for field, bit, msg in cases:
        bad = frame_view(scene)
        setattr(bad, field, 5 if field == "num_lights" else 1)
        with pytest.raises(UtopianError, match=msg) as e:
            gpu.render_hybrid(bad, rr.HYBRID_FRAME)
        assert "INVALID_ARGUMENT" in str(e.value)
        with pytest.raises(UtopianError):
            gpu.render_hybrid(bad, bit)
        after = read_all(gpu)
        for i in range(9):
            assert np.array_equal(before[i], after[i]), (field, i)
    # the same flags without the pass that needs them are fine
    ok = frame_view(scene, cubemap_enabled=1)
    gpu.render_hybrid(ok, rr.HYBRID_FRAME & ~rr.HYBRID_SKY)


def test_ssao_and_raytracing_gates():
    scene = synthetic_scene()
    gpu, cpu, meshes = pair(scene)
    v = frame_view(scene)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    ssao_before = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE)
    scene.camera = rr.camera.Camera((1.0, 1.5, 5.0), (0.0, 0.5, 0.0), 60.0, W / H, 0.01, 1000.0)
    for kw in (dict(ssao_enabled=0), dict(raytracing_supported=0), dict(ssao_enabled=0, raytracing_supported=0)):
        v2 = frame_view(scene, **kw)
        gpu.render_hybrid(v2, rr.HYBRID_FRAME)
        s = gpu.hybrid_frame_stats()
        ss = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE)
        if v2.ssao_enabled == 0:
            assert np.array_equal(ss, ssao_before) and s.pass_ms[3] == 0.0, "the SSAO pass does not run"
        g = gbuf(gpu)
        ref = fr.deferred(g, gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), ss, v2, meshes, [])
        geo = g["position"][..., 3] == 1.0
        d = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
        assert ulps(d[geo], ref[geo]).max() <= DEFERRED_ULP, kw
        ssao_before = ss


def test_frame_equals_the_passes_one_by_one():
    scene = synthetic_scene()
    a, _, _ = pair(scene)
    b, _, _ = pair(scene)
    v = frame_view(scene)
    a.render_hybrid(v, rr.HYBRID_FRAME)
    for bit in range(7):
        b.render_hybrid(v, 1 << bit)
    ia, ib = read_all(a), read_all(b)
    for i in range(9):
        assert np.array_equal(ia[i].view(np.uint8), ib[i].view(np.uint8)), i
    # bits outside UH_HYBRID_FRAME are ignored
    a.render_hybrid(v, rr.HYBRID_FRAME | (1 << 9))
    b.render_hybrid(v, rr.HYBRID_FRAME)
    for i in range(9):
        assert np.array_equal(a.read_hybrid(i).view(np.uint8), b.read_hybrid(i).view(np.uint8)), i


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_flight", [4, 1])
def test_frame_calls_change_nothing_the_path_tracer_or_the_ray_traced_passes_read(assets, in_flight):
    scene = reference_spheres_scene(assets)

    def run(with_frame):
        r = scene.upload(rr.Renderer(W, H))
        r.set_option("frames_in_flight", in_flight)
        loop = rr.FrameLoop(r, scene.make_view(W, H))
        hv = frame_view(scene)
        for i in range(5):
            loop.frame(rr.PASS_ALL)
            r.render_hybrid(hv, rr.HYBRID_ALL)
            if with_frame:
                r.render_hybrid(hv, rr.HYBRID_FRAME if i % 2 else rr.HYBRID_SSAO | rr.HYBRID_PRESENT)
        loop.frames(3, rr.PASS_ALL)
        r.render_hybrid(hv, rr.HYBRID_ALL)
        s, hs = r.get_stats(), r.hybrid_stats()
        out = dict(acc=r.read_accumulation().view(np.uint32), out=r.read_output_bgra8(), pos=r.read_gbuffer_position().view(np.uint32),
                   stats=(list(s.rays), s.frames, s.camera_grid_cells, s.sun_grid_cells, s.closest_hits, s.misses, list(hs.rays), hs.reflection_pixels))
        for k in range(3):
            out[f"res{k}"] = r.read_reservoirs(k).view(np.uint8)
        for k in range(6):
            out[f"hy{k}"] = r.read_hybrid(k).view(np.uint8)
        return out

    a, b = run(False), run(True)
    assert a.pop("stats") == b.pop("stats")
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 5. full size ---------------------------------------------------------------------------------------------------------
def _sampled_deferred(g, sh, refl, ss, view, meshes, lights, rows):
    sub = {k: v[rows] for k, v in g.items()}
    return fr.deferred(sub, sh[rows], refl[rows], ss[::-1][rows][::-1], view, meshes, lights)


def test_1080p_frame_on_the_config1_scene():
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    Wf, Hf = 1920, 1080
    gpu = rr.Renderer(Wf, Hf)
    meshes = hr.upload_recorded(scene, gpu, defaults=False)
    view = frame_view(scene, Wf, Hf)
    view.num_lights = 0
    gpu.render_hybrid(view, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    g = gbuf(gpu)
    sh, refl = gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS)
    ss, d, p = gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
    assert np.array_equal(ss, fr.ssao(g["position"], g["normal"], view))
    assert ss.min() < 65535, "Sponza-class geometry has creases"
    rows = np.arange(5, Hf, 97)
    ref = _sampled_deferred(g, sh, refl, ss, view, meshes, [], rows)
    geo = g["position"][rows][..., 3] == 1.0
    assert ulps(d[rows][geo], ref[geo]).max() <= DEFERRED_ULP
    assert np.array_equal(p, fr.present(d))
    s = gpu.hybrid_frame_stats()
    record("hybrid_frame", "config1-1080p", **{f"ms{k}": round(s.pass_ms[k], 4) for k in range(7)}, sky=s.sky_pixels)
    assert all(ms > 0 for ms in s.pass_ms)


def test_1024_lights_at_1080p_on_sampled_rows():
    scene = rr.scenes.scene_for_config(1, with_spheres=True)
    Wf, Hf = 1920, 1080
    gpu = rr.Renderer(Wf, Hf)
    meshes = hr.upload_recorded(scene, gpu, defaults=False)
    lights = add_lights(gpu, 1024, 11, (1, 2))
    view = frame_view(scene, Wf, Hf)
    view.num_lights = 1024
    gpu.render_hybrid(view, rr.HYBRID_GBUFFER)
    gpu.render_hybrid(view, rr.HYBRID_FRAME)
    g = gbuf(gpu)
    sh, refl, ss = gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE)
    d = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    rows = np.array([0, 217, 540, 811, 1079])
    ref = _sampled_deferred(g, sh, refl, ss, view, meshes, lights, rows)
    geo = g["position"][rows][..., 3] == 1.0
    u = ulps(d[rows][geo], ref[geo])
    record("hybrid_frame", "1024-lights", deferred_max_ulp=int(u.max()), deferred_exact=float((u == 0).mean()), ms=round(gpu.hybrid_frame_stats().pass_ms[4], 4))
    assert u.max() <= DEFERRED_ULP
    assert gpu.hybrid_frame_stats().lights == 1025


# ---- 6. the C++ mirror ----------------------------------------------------------------------------------------------------
def test_cpp_frame_images_equal_the_ctypes_images(tmp_path):
    meshes, v = cpp_scene(), cpp_view()
    v.shadows_enabled = v.cubemap_enabled = 0
    res, blob_out, r = run_cpp(tmp_path, "frame", meshes, v)
    r.render_hybrid(v, rr.HYBRID_FRAME)
    at = 0
    for which in (rr.HYBRID_SSAO_IMAGE, rr.HYBRID_DEFERRED_OUTPUT, rr.HYBRID_PRESENT_OUTPUT):
        mine = r.read_hybrid(which).view(np.uint8).reshape(-1)
        assert np.array_equal(blob_out[at : at + mine.size], mine), which
        at += mine.size
    assert at == blob_out.size
    s = r.hybrid_frame_stats()
    assert f"sky {s.sky_pixels} lights {s.lights}" in res.stdout and s.lights == 1
