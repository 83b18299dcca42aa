"""CPU: the composed restatement of the deferred pass (tests/hybrid_compose_reference.py) equals each restatement of one feature, on that
restatement's own domain, bit for bit: hybrid_frame_reference.deferred, ibl_reference.deferred_ibl, hybrid_restir_reference.deferred and
shadow_map_reference.deferred_with_shadow_maps. The G-buffer and the reservoirs are the oracle's, the shadow maps the numpy
rasteriser's at size 256; the IBL maps are seeded random arrays of the device's layout (the functions only read them). With the features
together nothing is left to compare it with on the CPU: that is what the device tests use it for."""
import numpy as np
import pytest

import hybrid_compose_reference as cr
import hybrid_frame_reference as fr
import hybrid_reference as hr
import hybrid_restir_reference as rl
import ibl_reference as ir
import oracle_api as oa
import rust_renderer_amd as rr
import shadow_map_reference as sr
from hybrid_util import frame_view, synthetic_scene

W, H = 48, 36
S = 256
VIEWS = (dict(), dict(ssao_enabled=0), dict(raytracing_supported=0), dict(ssao_enabled=0, raytracing_supported=0))


def tight(scene, near=3.0, far=12.0):
    """the scene's camera with near / far tight around it, so that geometry falls into all four cascades"""
    c = scene.camera
    scene.camera = rr.camera.Camera(c.position, c.target, c.fov_degrees, c.aspect_ratio, near, far)
    return scene


def random_maps(seed):
    """arrays of the layout of ibl_reference.read_maps: values in [0, 2), the LUT in [0, 1)"""
    rng = np.random.default_rng(seed)
    cube = lambda size: (2.0 * rng.random((6, size, size, 4), np.float32))
    return dict(irr=cube(ir.SIZE), spec=[cube(ir.SIZE >> m) for m in range(ir.MIPS)], lut=rng.random((ir.LUT, ir.LUT, 2), np.float32).astype(np.float16))


def build_world():
    """the tightened synthetic scene with 8 partly occluded lights on the oracle: its G-buffer, the spatial reservoirs after three
    frames with their visibility image, the numpy shadow maps, random IBL maps and random rt_shadows / rt_reflections / SSAO images"""
    scene = tight(synthetic_scene())
    cpu = oa.OracleRenderer(W, H)
    meshes = hr.upload_recorded(scene, cpu, defaults=False)
    lights = rl.occluded_lights(8)
    for l in lights:
        cpu.add_gpu_light(l)
    cpu.initialize_raytracing()
    view = frame_view(scene, W, H)
    view.num_lights = len(lights)
    g = hr.gbuffer(cpu, meshes, view, W, H)
    for k in range(3):
        v = frame_view(scene, W, H)
        v.num_lights, v.total_samples = len(lights), k + 1
        cpu.render_frame(v, rr.PASS_RESTIR)
    res = cpu.read_reservoirs(2)
    vis, rays, occluded = rl.visibility(cpu, g, res, view, lights)
    assert 0 < occluded < rays
    params = rr.shadow_cascades(scene.camera, view.sun_dir[:])
    rng = np.random.default_rng(5)
    return dict(scene=scene, meshes=meshes, lights=lights, g=g, res=res, vis=vis, shadow=(params, sr.shadow_maps(meshes, params, S)), maps=random_maps(3),
                sh=rng.integers(0, 256, (H, W)).astype(np.uint8), refl=rng.integers(0, 256, (H, W, 4)).astype(np.uint8),
                ss=rng.integers(0, 65536, (H, W)).astype(np.uint16))


@pytest.fixture(scope="module")
def world():
    return build_world()


def views(world, num_lights):
    for kw in VIEWS:
        v = frame_view(world["scene"], W, H, **kw)
        v.num_lights = num_lights
        yield kw, v


def same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_plain_equals_the_frame_restatement(world):
    g, sh, refl, ss, meshes, lights = (world[k] for k in ("g", "sh", "refl", "ss", "meshes", "lights"))
    for n in (0, len(lights)):
        for kw, v in views(world, n):
            assert same(cr.deferred(g, sh, refl, ss, v, meshes, lights), fr.deferred(g, sh, refl, ss, v, meshes, lights)), (n, kw)


def test_with_ibl_maps_equals_the_ibl_restatement(world):
    g, sh, refl, ss, meshes, lights, maps = (world[k] for k in ("g", "sh", "refl", "ss", "meshes", "lights", "maps"))
    for kw, v in views(world, len(lights)):
        v.ibl_enabled = 1
        a, b = cr.deferred(g, sh, refl, ss, v, meshes, lights, maps=maps), ir.deferred_ibl(g, sh, refl, ss, v, meshes, lights, maps)
        assert same(a, b), kw
        assert not same(a, fr.deferred(g, sh, refl, ss, v, meshes, lights)), "the maps are read"


def test_with_reservoirs_equals_the_reservoir_restatement(world):
    g, sh, refl, ss, meshes, lights, res, vis = (world[k] for k in ("g", "sh", "refl", "ss", "meshes", "lights", "res", "vis"))
    for kw, v in views(world, len(lights)):
        a, b = cr.deferred(g, sh, refl, ss, v, meshes, lights, res=res, vis=vis), rl.deferred(g, sh, refl, ss, v, meshes, lights, res, vis)
        assert same(a, b), kw
        assert not same(a, fr.deferred(g, sh, refl, ss, v, meshes, lights))


def test_with_shadow_maps_equals_the_shadow_map_construction(world):
    g, sh, refl, ss, meshes, lights, shadow = (world[k] for k in ("g", "sh", "refl", "ss", "meshes", "lights", "shadow"))
    geo = (g["position"][..., 3] != 0).reshape(-1)
    factor, cascade = cr.shadow_factor(g, frame_view(world["scene"], W, H), shadow)
    assert set(np.unique(cascade[geo])) == {0, 1, 2, 3} and (factor[geo] < 1).any() and (factor[geo] == 1).any()
    for n in (0, len(lights)):
        for kw, v in views(world, n):
            v.shadows_enabled = 1
            a = cr.deferred(g, sh, refl, ss, v, meshes, lights, shadow=shadow)
            b, _ = sr.deferred_with_shadow_maps(g, refl, ss, v, meshes, *shadow, lights=lights)
            assert same(a, b), (n, kw)
            if v.raytracing_supported == 1:
                assert not same(a, fr.deferred(g, sh, refl, ss, v, meshes, lights)), "rt_shadows is not read"
