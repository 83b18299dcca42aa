"""GPU: the cascaded shadow maps (UH_HYBRID_SHADOW_MAPS) bit for bit against the numpy rasteriser of tests/shadow_map_reference.py at
awkward sizes, after a moved instance and under a floor far beyond the guard band; the deferred pass with shadows_enabled = 1 against
the restatement; the reference's default view end to end; the refusals, gates and isolation of the pass."""
import copy

import numpy as np
import pytest

import hybrid_compose_reference as cr
import hybrid_frame_reference as fr
import ibl_reference as ir
import rust_renderer_amd as rr
import shadow_map_reference as sr
from hybrid_util import CONSUMER_ULP, DEFERRED_ULP, W, H, assets, frame_view, gbuf, pair, read_all, scene_named, synthetic_scene, ulps
from rust_renderer_amd.api import UtopianError
from rust_renderer_amd.scenes import Scene, quad

pytestmark = pytest.mark.gpu


def _tight(scene, near=3.0, far=12.0):
    """the scene's camera with near / far tight around it, so that geometry falls into all four cascades"""
    c = scene.camera
    scene.camera = rr.camera.Camera(c.position, c.target, c.fov_degrees, c.aspect_ratio, near, far)
    return scene


def _shadow_view(scene, **kw):
    v = frame_view(scene, **kw)
    v.shadows_enabled = 1
    return v


def _params(scene, view):
    return rr.shadow_cascades(scene.camera, view.sun_dir[:])


def _render_maps(gpu, scene, view, size):
    gpu.set_option("shadow_map_size", size)
    p = _params(scene, view)
    gpu.set_shadowmap_params(p)
    gpu.render_hybrid(view, rr.HYBRID_SHADOW_MAPS)
    return p


def _check_maps(gpu, meshes, p, size):
    ref = sr.shadow_maps(meshes, p, size)
    s = gpu.shadow_map_stats()
    assert s.size == size
    for c in range(4):
        got = gpu.read_shadow_map(c)
        assert got.shape == (size, size)
        bad = np.count_nonzero(got.view(np.uint32) != ref[c].view(np.uint32))
        assert bad == 0, f"cascade {c}: {bad} texels differ from the numpy rasteriser at size {size}"
        vp, _ = sr.params_arrays(p)
        assert s.triangles[c] == len(sr.records_for(meshes, vp[c], size))
    return ref


@pytest.mark.parametrize("size", [64, 257, 1000])
def test_maps_bit_for_bit_at_awkward_sizes(size):
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene)
    p = _render_maps(gpu, scene, v, size)
    ref = _check_maps(gpu, meshes, p, size)
    assert all((ref[c] < 1.0).any() for c in range(4)), "every cascade sees geometry"


def test_maps_bit_for_bit_at_the_reference_size():
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene)
    p = _render_maps(gpu, scene, v, 4096)
    _check_maps(gpu, meshes, p, 4096)
    s = gpu.shadow_map_stats()
    assert s.renders == 1 and s.pass_ms > 0.0
    assert np.array_equal(np.frombuffer(bytes(s.params), np.uint8), np.frombuffer(bytes(p), np.uint8))


@pytest.mark.parametrize("name", ["cornell", "spheres"])
def test_maps_bit_for_bit_on_the_reference_assets(name, assets):
    scene = scene_named(name, assets)
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene)
    p = _render_maps(gpu, scene, v, 509)
    _check_maps(gpu, meshes, p, 509)


def test_moved_instance_after_rebuild_tlas():
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene)
    _render_maps(gpu, scene, v, 300)
    w = rr.transform3x4((1.2, 0.6, 0.9), (-0.7, 1.1, 0.4), np.array([[0.8, 0.0, -0.6], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]], np.float32))
    gpu.set_instance_transform(1, w)
    meshes[1]["world"] = w.copy()
    v.rebuild_tlas = 1
    p = _render_maps(gpu, scene, v, 300)
    _check_maps(gpu, meshes, p, 300)


class _HugeFloor(Scene):
    def upload(self, renderer):
        renderer.default_diffuse_map()
        fv, fi = quad((-30000.0, 0.0, 30000.0), (60000.0, 0.0, 0.0), (0.0, 0.0, -60000.0))
        renderer.add_mesh(fv, fi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.8, 0.8, 1.0)))
        bv, bi = quad((-0.5, 0.8, 0.5), (1.0, 0.0, 0.0), (0.0, 0.0, -1.0))
        renderer.add_mesh(bv, bi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.3, 0.3, 1.0)))
        renderer.initialize_raytracing()
        return renderer


def _floor_scene(near=0.3, far=30.0):
    cam = rr.camera.Camera((0.0, 2.0, 3.0), (0.0, 0.5, 0.0), 60.0, W / H, near, far)
    return _HugeFloor("huge_floor", [], [], cam, dict(sky_enabled=1))


def test_ground_plane_far_beyond_the_guard_band():
    scene = _floor_scene()
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene)
    p = _render_maps(gpu, scene, v, 512)
    ref = _check_maps(gpu, meshes, p, 512)
    vp, _ = sr.params_arrays(p)
    M = sr.mesh_matrix(vp[0], meshes[0]["world"])
    corner = meshes[0]["vertices"]["pos"][0, :3]
    x = ((M[0] * corner[0] + M[4] * corner[1]) + M[8] * corner[2]) + M[12]
    assert abs(x * 256.0 + 256.0) > sr.GUARD, "the floor's corners lie beyond the guard band of cascade 0: it is clipped"
    assert (ref[0] < 1.0).mean() > 0.2, "the clipped floor covers cascade 0"


def _deferred_restated(gpu, view, meshes, p, maps):
    """deferred.frag with shadows_enabled = 1 from the device's own inputs: the rt_shadows branch neutralised (all 255 multiplies by
    exactly 1.0) and SSAO off, then calculateShadow's factor and the SSAO factor in the reference's order"""
    g = gbuf(gpu)
    out, cascade = sr.deferred_with_shadow_maps(g, gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), view, meshes, p, maps)
    return out, cascade, g


@pytest.mark.parametrize("ssao", [0, 1])
def test_deferred_with_shadow_maps_matches_the_restatement(ssao):
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene, ssao_enabled=ssao)
    p = _render_maps(gpu, scene, v, 1000)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    maps = np.stack([gpu.read_shadow_map(c) for c in range(4)])
    ref, cascade, g = _deferred_restated(gpu, v, meshes, p, maps)
    got = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    geo = g["position"][..., 3] == 1.0
    for c in range(4):
        assert (geo & (cascade == c)).any(), f"no geometry pixel in cascade {c}"
    d = ulps(got[geo][:, :3], ref[geo][:, :3])
    assert d.max() <= DEFERRED_ULP, d.max()
    factor, _ = sr.calculate_shadow(g["position"][..., :3].reshape(-1, 3).astype(np.float32), v, p, maps)
    assert (factor < 1.0).any() and (factor == 1.0).any()


def test_reference_default_view_end_to_end():
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v = frame_view(scene)
    v.shadows_enabled = v.ibl_enabled = v.cubemap_enabled = 1
    gpu.set_option("shadow_map_size", 256)
    gpu.set_shadowmap_params(_params(scene, v))
    gpu.render_hybrid(v, rr.HYBRID_FRAME | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS)
    deferred = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    present = gpu.read_hybrid(rr.HYBRID_PRESENT_OUTPUT)
    assert np.isfinite(deferred).all()
    # k_hybrid_deferred<1, 1, 0>: IBL ambient and calculateShadow together, on the device's own inputs
    g = gbuf(gpu)
    p, shadow_maps = gpu.shadow_map_stats().params, np.stack([gpu.read_shadow_map(c) for c in range(4)])
    ref = cr.deferred(g, gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), v, meshes, [],
                      maps=ir.read_maps(gpu), shadow=(p, shadow_maps))
    geo = g["position"][..., 3] == 1.0
    factor, cascade = cr.shadow_factor(g, v, (p, shadow_maps))
    assert geo.any() and (factor[geo.reshape(-1)] < 1.0).any() and (factor[geo.reshape(-1)] == 1.0).any()
    d = ulps(deferred[geo][:, :3], ref[geo][:, :3])
    assert d.max() <= CONSUMER_ULP, d.max()
    assert np.array_equal(present, fr.present(deferred, v.fxaa_enabled == 1))
    s = gpu.hybrid_frame_stats()
    assert all(s.pass_ms[k] > 0.0 for k in range(7)) and gpu.shadow_map_stats().renders == 1


def test_refusals_and_gates_leave_the_images_unchanged():
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v0 = frame_view(scene)
    gpu.render_hybrid(v0, rr.HYBRID_FRAME)
    before = read_all(gpu)
    v = _shadow_view(scene)
    # the bit without params
    with pytest.raises(UtopianError, match="uh_set_shadowmap_params") as e:
        gpu.render_hybrid(v, rr.HYBRID_SHADOW_MAPS | rr.HYBRID_FRAME)
    assert "INVALID_ARGUMENT" in str(e.value)
    # deferred with shadows before any render
    with pytest.raises(UtopianError, match="UH_HYBRID_SHADOW_MAPS"):
        gpu.render_hybrid(v, rr.HYBRID_FRAME)
    with pytest.raises(UtopianError):
        gpu.read_shadow_map(0)
    after = read_all(gpu)
    for i in range(9):
        assert np.array_equal(before[i], after[i]), i
    assert gpu.shadow_map_stats().renders == 0
    # the bit with shadows_enabled = 0 runs nothing, and the frame is byte-identical with and without it
    gpu.set_shadowmap_params(_params(scene, v))
    gpu.render_hybrid(v0, rr.HYBRID_FRAME | rr.HYBRID_SHADOW_MAPS)
    assert gpu.shadow_map_stats().renders == 0
    with_bit = read_all(gpu)
    gpu.render_hybrid(v0, rr.HYBRID_FRAME)
    for i in range(9):
        assert np.array_equal(with_bit[i], read_all(gpu)[i]), i
    # after a size change the maps are gone: deferred with shadows is refused again
    gpu.set_option("shadow_map_size", 64)
    gpu.render_hybrid(v, rr.HYBRID_SHADOW_MAPS)
    gpu.render_hybrid(v, rr.HYBRID_FRAME)
    done = read_all(gpu)
    gpu.set_option("shadow_map_size", 65)
    with pytest.raises(UtopianError, match="shadow maps"):
        gpu.render_hybrid(v, rr.HYBRID_DEFERRED)
    with pytest.raises(UtopianError):
        gpu.read_shadow_map(0)
    for i in range(9):
        assert np.array_equal(done[i], read_all(gpu)[i]), i
    with pytest.raises(UtopianError, match="16..8192"):
        gpu.set_option("shadow_map_size", 8193)


def test_shadow_map_pass_is_isolated():
    scene = _tight(synthetic_scene())
    gpu, _, meshes = pair(scene)
    v = _shadow_view(scene)
    gpu.set_shadowmap_params(_params(scene, v))
    gpu.set_option("shadow_map_size", 128)
    gpu.render_hybrid(v, rr.HYBRID_FRAME | rr.HYBRID_SHADOW_MAPS)
    imgs, st, hs, fs = read_all(gpu), bytes(gpu.get_stats()), bytes(gpu.hybrid_stats()), bytes(gpu.hybrid_frame_stats())
    gpu.render_hybrid(v, rr.HYBRID_SHADOW_MAPS)
    assert gpu.shadow_map_stats().renders == 2
    after = read_all(gpu)
    for i in range(9):
        assert np.array_equal(imgs[i], after[i]), i
    assert bytes(gpu.get_stats()) == st and bytes(gpu.hybrid_stats()) == hs and bytes(gpu.hybrid_frame_stats()) == fs
    # the deferred pass reads the snapshot the maps were rendered with, not params set since
    other = copy.deepcopy(_params(scene, v))
    other.cascade_splits[0] = 0.5
    gpu.set_shadowmap_params(other)
    gpu.render_hybrid(v, rr.HYBRID_DEFERRED | rr.HYBRID_SKY)
    assert np.array_equal(gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT), imgs[rr.HYBRID_DEFERRED_OUTPUT])


def test_set_params_rejects_non_orthographic_and_non_finite():
    scene = synthetic_scene()
    gpu, _, _ = pair(scene)
    p = _params(scene, frame_view(scene))
    for mutate in (lambda q: q.view_projection_matrices[1].__setitem__(3, 0.5), lambda q: q.view_projection_matrices[0].__setitem__(15, 2.0),
                   lambda q: q.cascade_splits.__setitem__(2, float("nan")), lambda q: q.view_projection_matrices[3].__setitem__(0, float("inf"))):
        q = copy.deepcopy(p)
        mutate(q)
        with pytest.raises(UtopianError, match="INVALID_ARGUMENT"):
            gpu.set_shadowmap_params(q)


# ---- independent of the restatement: quads over a floor, against analytic shadows and this frame's rt_shadows --------------------
SUN = np.array([0.2, 0.95, 0.15]) / np.linalg.norm([0.2, 0.95, 0.15])
# one horizontal square per cascade, (centre x, centre z, height above the floor, side), its shadow on the floor in that cascade's slice
OCCLUDERS = [(0.0, 5.0, 0.1, 0.3), (0.0, 4.0, 0.2, 0.7), (0.0, 1.0, 0.4, 1.6), (0.0, -11.5, 1.0, 5.0)]


class _QuadsOverFloor(Scene):
    def upload(self, renderer):
        renderer.default_diffuse_map()
        fv, fi = quad((-30.0, 0.0, 30.0), (60.0, 0.0, 0.0), (0.0, 0.0, -60.0))
        renderer.add_mesh(fv, fi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.8, 0.8, 0.8, 1.0)))
        for x, z, h, side in OCCLUDERS:
            # the square whose shadow (along -SUN) is centred on (x, 0, z)
            cx, cz = x + SUN[0] * h / SUN[1], z + SUN[2] * h / SUN[1]
            qv, qi = quad((cx - side / 2, h, cz + side / 2), (side, 0.0, 0.0), (0.0, 0.0, -side))
            renderer.add_mesh(qv, qi, rr.make_material(rr.LAMBERTIAN, 0.0, (0.3, 0.5, 0.8, 1.0)))
        renderer.initialize_raytracing()
        return renderer


def test_quads_over_floor_shadow_analytic_and_rt_shadows():
    """floor pixels more than 3 texels (of their cascade) inside a square's analytic shadow get 0.3, those more than 3 texels outside
    every shadow get 1.0 and are lit in this frame's rt_shadows, in every cascade; the factor is the device's own output divided by
    the same frame without shadows, so nothing here goes through shadow_map_reference"""
    Wq, Hq, S = 320, 240, 1024
    cam = rr.camera.Camera((0.0, 1.0, 6.0), (0.0, 0.0, 3.0), 60.0, Wq / Hq, 0.3, 25.0)
    scene = _QuadsOverFloor("quads_over_floor", [], [], cam, dict(sky_enabled=1))
    gpu, _, _ = pair(scene, Wq, Hq)
    v = _shadow_view(scene, width=Wq, height=Hq, ssao_enabled=0, raytracing_supported=1)
    v.sun_dir[:] = tuple(np.float32(SUN))
    gpu.set_option("shadow_map_size", S)
    p = rr.shadow_cascades(cam, v.sun_dir[:])
    gpu.set_shadowmap_params(p)
    for _ in range(2):  # rt_shadows reads the previous call's G-buffer: the second call's is this camera's
        gpu.render_hybrid(v, rr.HYBRID_FRAME | rr.HYBRID_SHADOW_MAPS)
    lit = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)[..., :3].astype(np.float64)
    rt = gpu.read_hybrid(rr.HYBRID_SHADOWS)
    g = gbuf(gpu)
    plain = frame_view(scene, Wq, Hq, ssao_enabled=0, raytracing_supported=0)
    plain.sun_dir[:] = v.sun_dir[:]
    gpu.render_hybrid(plain, rr.HYBRID_FRAME)
    base = gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)[..., :3].astype(np.float64)

    P = g["position"][..., :3].astype(np.float64)
    V = np.array(v.view[:], np.float64).reshape(4, 4).T
    vz = P @ V[2, :3] + V[2, 3]
    # floor pixels inside the view frustum's depth range: the G-buffer cast has no far plane, but the cascades cover only the frustum
    # (and the reference's rasterised G-buffer clips there), so a floor point beyond z_far falls outside every cascade's map
    floor = (g["position"][..., 3] == 1.0) & (g["pbr"][..., 3] == 0.0) & (-vz < 0.98 * cam.z_far)
    splits = np.array(p.cascade_splits[:], np.float64)
    cascade = (vz < -splits[0]).astype(int) + (vz < -splits[1]) + (vz < -splits[2])
    near_split = np.zeros_like(floor)
    for s in splits[:3]:
        near_split |= np.abs(-vz - s) < 0.02 * s
    vp = np.array([list(p.view_projection_matrices[k]) for k in range(4)], np.float64).reshape(4, 4, 4).transpose(0, 2, 1)
    texel = np.array([2.0 / np.linalg.norm(vp[k, 0, :3]) / S for k in range(4)])  # 2 r / S, r = 1 / |row 0|
    # signed distance, in the squares' planes, of q = P + (h / sun.y) sun to each square's edge (> 0 inside); a horizontal distance
    # shrinks by at most |sun.y| on the light's image plane
    inside_m = np.full(P.shape[:2], -np.inf)
    outside_m = np.full(P.shape[:2], np.inf)
    for x, z, h, side in OCCLUDERS:
        cx, cz = x + SUN[0] * h / SUN[1], z + SUN[2] * h / SUN[1]
        qx, qz = P[..., 0] + SUN[0] * h / SUN[1] - cx, P[..., 2] + SUN[2] * h / SUN[1] - cz
        dx, dz = np.abs(qx) - side / 2, np.abs(qz) - side / 2
        inside_m = np.maximum(inside_m, np.minimum(-dx, -dz))
        outside_m = np.minimum(outside_m, np.hypot(np.maximum(dx, 0), np.maximum(dz, 0)) + np.minimum(np.maximum(dx, dz), 0))
    tex = texel[np.clip(cascade, 0, 3)]
    well_in = floor & ~near_split & (inside_m * SUN[1] > 3 * tex)
    well_out = floor & ~near_split & (outside_m * SUN[1] > 3 * tex)
    ch = np.argmax(base, axis=-1)
    b = np.take_along_axis(base, ch[..., None], -1)[..., 0]
    a = np.take_along_axis(lit, ch[..., None], -1)[..., 0]
    ok = b > 1e-4
    factor = np.where(ok, a / np.where(ok, b, 1.0), np.nan)
    # rt_shadows traces from the mean of the 2 x 2 texels up and to the left (rt_shadows.rgen's texture() at the pixel corner): it
    # is compared where that whole block is floor and classified alike
    def block(m):
        y0, x0 = np.maximum(np.arange(m.shape[0]) - 1, 0), np.maximum(np.arange(m.shape[1]) - 1, 0)
        return m & m[y0] & m[:, x0] & m[y0][:, x0]

    rt_in, rt_out = block(well_in), block(well_out)
    for c in range(4):
        i, o = well_in & ok & (cascade == c), well_out & ok & (cascade == c)
        assert i.sum() >= 20 and o.sum() >= 20, f"cascade {c}: {i.sum()} pixels well inside a shadow, {o.sum()} well outside"
        assert np.allclose(factor[i], 0.3, rtol=1e-5, atol=0), (c, np.unique(np.round(factor[i], 5)))
        bad = o & ~np.isclose(factor, 1.0, rtol=1e-5, atol=0)
        assert not bad.any(), (c, np.count_nonzero(bad), o.sum(), P[bad][:4], vz[bad][:4], outside_m[bad][:4], tex[bad][:1], np.argwhere(bad)[:4])
        ri, ro = rt_in & (cascade == c), rt_out & (cascade == c)
        assert ri.sum() >= 10 and ro.sum() >= 10, (c, ri.sum(), ro.sum())
        assert np.all(rt[ro] == 255), f"cascade {c}: {np.count_nonzero(rt[ro] != 255)} lit pixels the ray-traced shadows call occluded"
        assert np.all(rt[ri] == 0), f"cascade {c}: {np.count_nonzero(rt[ri] != 0)} shadowed pixels the ray-traced shadows call lit"
