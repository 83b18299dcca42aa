"""GPU: the whole hybrid graph at frame sizes that are not whole numbers of 64-lane waves or 256-lane blocks - the i >= n tails of the
one-lane-per-pixel passes, the partial last wave of the reflection and sky compactions, the last partial chunk of rt_shadows' feeder,
and frames one pixel wide or tall (a mirrored repeat of period 2, a texel-corner fetch of one column or row) - against the CPU
references pass by pass, with lights of all four kinds; at two sizes also the IBL maps and their consumers."""
import numpy as np
import pytest

import hybrid_reference as hr
import ibl_reference as ir
import rust_renderer_amd as rr
from hybrid_util import add_lights, assert_reflections, bits, check_frame, check_ibl_frame, frame_view, gbuf, ibl_view, pair, read_all, synthetic_scene

pytestmark = pytest.mark.gpu

# (W, H): n = W H and n mod 64 / n mod 256 - 1/1, 45/45, 3/67, 3/195, 3/3, 29/29, 47/239, 0/192
SIZES = [(1, 1), (1, 45), (67, 1), (65, 3), (257, 3), (97, 61), (255, 17), (320, 7)]


def sized_scene(w, h):
    """the synthetic scene of hybrid_util.py with a camera of this aspect, so that the frame holds sky, metal and non-metal pixels.
    A one-pixel column looks down through the Lambertian sphere: sky above, the metal floor below, the sphere between. A one-pixel
    row looks at that sphere from close by, so that it covers more than one pixel (the texel-corner fetch averages the material index
    of neighbours); a frame of two or three rows from further away. Their wide views end in the floor and the sky. Other frames keep
    the usual camera"""
    scene = synthetic_scene()
    if w == 1:
        eye, target = (-1.5, 2.2, 6.5), (-1.5, 0.9, 0.0)
    elif h == 1:
        eye, target = (-1.5, 1.5, 1.8), (-1.5, 0.8, 0.0)
    elif h <= 3:
        eye, target = (0.0, 2.2, 6.5), (-1.5, 0.8, 0.0)
    else:
        eye, target = (0.0, 2.2, 6.5), (0.0, 0.9, 0.0)
    scene.camera = rr.camera.Camera(eye, target, 60.0, w / h, 0.01, 1000.0)
    return scene


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_pass_at_an_awkward_size(w, h):
    n = w * h
    scene = sized_scene(w, h)
    gpu, cpu, meshes = pair(scene, w, h)
    lights = add_lights(gpu, 8, 5, (0, 1, 2, 5))
    view = frame_view(scene, w, h)
    view.num_lights = len(lights)
    # G-buffer: bit-exact, with the camera grid on and off; the position target is the path tracer's
    ref = None
    for grid in (1, 0):
        gpu.set_option("camera_grid", grid)
        for _ in range(2):
            gpu.render_frame(view, rr.PASS_GBUFFER)
        gpu.render_hybrid(view, rr.HYBRID_GBUFFER)
        g = gbuf(gpu)
        assert np.array_equal(bits(g["position"]), bits(gpu.read_gbuffer_position())), grid
        ref = ref or hr.gbuffer(cpu, meshes, view, w, h)
        for k in ("position", "normal", "pbr"):
            assert np.array_equal(bits(g[k]), bits(ref[k])), (grid, k)
        assert np.array_equal(g["albedo"], ref["albedo"]), grid
    # rt_shadows (exact) and rt_reflections (exact, 1 LSB where the ray meets the sky) of this G-buffer
    gpu.render_hybrid(view, rr.HYBRID_RT_SHADOWS | rr.HYBRID_RT_REFLECTIONS)
    assert np.array_equal(gpu.read_hybrid(rr.HYBRID_SHADOWS), hr.shadows(cpu, g["position"], g["normal"], view))
    want_refl, kind = hr.reflections(cpu, meshes, g["position"], g["normal"], g["pbr"], view)
    assert_reflections(gpu.read_hybrid(rr.HYBRID_REFLECTIONS), want_refl, kind)
    s = gpu.hybrid_stats()
    assert s.reflection_pixels == np.count_nonzero(kind) and list(s.rays) == [0, n, np.count_nonzero(kind)]
    sky = g["position"][..., 3] == 0
    if n > 1:  # both compaction queues end in a partial wave, and each holds some but not all pixels
        assert sky.any() and (~sky).any(), "sky and geometry"
        assert (kind != 0).any() and (kind == 0).any(), "metal and non-metal"
    # the final frame, pass by pass on the device's inputs, with FXAA on and off (check_frame: SSAO exact, deferred DEFERRED_ULP, sky
    # within 1 LSB after present, present exact, sky_pixels)
    for fxaa in (1, 0):
        view.fxaa_enabled = fxaa
        check_frame(gpu, cpu, meshes, view, lights, f"size{w}x{h}-fxaa{fxaa}")
        assert gpu.hybrid_frame_stats().sky_pixels == np.count_nonzero(sky)
        s = gpu.hybrid_stats()
        assert list(s.rays) == [n, n, np.count_nonzero(kind)] and s.reflection_pixels == np.count_nonzero(kind)
    # UH_HYBRID_FRAME gives the bytes of the seven passes one at a time (two fresh contexts)
    one, _, _ = pair(scene, w, h)
    seven, _, _ = pair(scene, w, h)
    for r in (one, seven):
        add_lights(r, 8, 5, (0, 1, 2, 5))
    one.render_hybrid(view, rr.HYBRID_FRAME)
    for bit in range(7):
        seven.render_hybrid(view, 1 << bit)
    ia, ib = read_all(one), read_all(seven)
    for i in range(9):
        assert np.array_equal(ia[i].view(np.uint8), ib[i].view(np.uint8)), i


@pytest.mark.parametrize("w,h", [(97, 61), (1, 45)], ids=["97x61", "1x45"])
def test_ibl_consumers_at_an_awkward_size(w, h):
    scene = sized_scene(w, h)
    gpu, cpu, meshes = pair(scene, w, h)
    v = ibl_view(scene, w, h)
    v.num_lights = 0
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_ENVIRONMENT)
    maps = ir.read_maps(gpu)
    g, d = check_ibl_frame(gpu, cpu, meshes, v, maps, f"ibl-size{w}x{h}")
    assert (g["position"][..., 3] == 0).any() and (g["position"][..., 3] == 1).any()
