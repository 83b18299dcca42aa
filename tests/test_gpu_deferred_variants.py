"""GPU: all eight instantiations of k_hybrid_deferred<kIbl, kShadow, kRestir>, each with SSAO off and on, against the composed
restatement of tests/hybrid_compose_reference.py on the device's own inputs. One world at 97 x 61 (W H mod 64 = 29: the last wave is
partial and the image ends inside a block): the synthetic scene with its camera tight enough for all four cascades, 8 partly occluded
point and spot lights, three reservoir frames, shadow maps of size 256 and the IBL maps, all built once. Each case also asserts that its
frame reaches what it is meant to: every cascade, shadowed and lit pixels, arrived and occluded reservoir rays, metal and matte.

Those lights stand behind the scene's occluders, and with raytracing_supported = 1 the metal floor shows its reflection alone: the
reservoir light's term reaches the image on a handful of matte pixels only (6 of 1,068 lit ones on the oracle). So the four kRestir
variants run once more in a second world whose 8 lights stand on the camera's side, where over a hundred matte pixels carry the term."""
import numpy as np
import pytest

import hybrid_compose_reference as cr
import hybrid_restir_reference as rl
import ibl_reference as ir
import rust_renderer_amd as rr
from hybrid_util import CONSUMER_ULP, DEFERRED_ULP, bits, gbuf, synthetic_scene, ulps
from test_gpu_hybrid_restir import World
from test_gpu_shadow_map import _tight

pytestmark = pytest.mark.gpu

W, H = 97, 61
SIZE = 256


class Variants(World):
    def view(self, ibl=0, shadows=0, **kw):
        v = super().view(**kw)
        v.ibl_enabled = v.cubemap_enabled = ibl
        v.shadows_enabled = shadows
        return v


def front_lights(n=8):
    """n point and spot lights between the camera and the meshes, a little above the floor: they light the matte ellipsoid's near side,
    and the metal sphere hides part of it from some of them"""
    out = []
    for k in range(n):
        l = rr.make_light((-3.5 + 7.0 * k / (n - 1), 0.9 + 0.3 * (k % 3), 2.6 + 0.4 * (k % 2)),
                          color=(0.3 + 0.7 * ((k * 5) % 7) / 6.0, 0.9 - 0.6 * ((k * 3) % 5) / 4.0, 0.4 + 0.5 * (k % 3) / 2.0))
        l.light_type = float(1 + k % 2)
        l.direction[:] = (0.0, -0.2, -1.0)
        l.spot = 1.0 + (k % 2)
        out.append(l)
    return out


def build_variants(lights=None):
    w = Variants(_tight(synthetic_scene()), rl.occluded_lights(8) if lights is None else lights, W, H)
    gpu = w.gpu
    v = w.view(ibl=1, shadows=1)
    gpu.set_option("shadow_map_size", SIZE)
    gpu.set_shadowmap_params(rr.shadow_cascades(w.scene.camera, v.sun_dir[:]))
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER | rr.HYBRID_ENVIRONMENT | rr.HYBRID_SHADOW_MAPS)
    w.maps = ir.read_maps(gpu)
    w.shadow = (gpu.shadow_map_stats().params, np.stack([gpu.read_shadow_map(c) for c in range(4)]))
    assert gpu.shadow_map_stats().size == SIZE and gpu.shadow_map_stats().renders == 1
    return w


@pytest.fixture(scope="module")
def world():
    return build_variants()


@pytest.fixture(scope="module")
def front():
    return build_variants(front_lights())


@pytest.mark.parametrize("ssao", [0, 1])
@pytest.mark.parametrize("ibl, shadows, restir", [(i, s, r) for i in (0, 1) for s in (0, 1) for r in (0, 1)])
def test_deferred_variant_equals_the_composed_restatement(world, ibl, shadows, restir, ssao):
    check_variant(world, ibl, shadows, restir, ssao)


@pytest.mark.parametrize("ibl, shadows", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_reservoir_variants_where_the_term_shows_on_matte_pixels(front, ibl, shadows):
    matte_lit, matte_occluded = check_variant(front, ibl, shadows, 1, 1)
    assert matte_lit >= 100 and matte_occluded > 0, (matte_lit, matte_occluded)


def check_variant(world, ibl, shadows, restir, ssao):
    """one steady UH_HYBRID_FRAME call with the variant's bits and flags against the composed restatement on the device's inputs, and
    the coverage conditions; returns the matte pixels whose reservoir ray arrived and those whose ray was occluded"""
    gpu, meshes, lights = world.gpu, world.meshes, world.all_lights()
    v = world.view(ibl=ibl, shadows=shadows, ssao_enabled=ssao)
    assert v.raytracing_supported == 1 and v.num_lights == 8
    gpu.render_hybrid(v, rr.HYBRID_GBUFFER)  # rt_shadows reads the previous call's G-buffer: a steady frame
    gpu.render_hybrid(v, rr.HYBRID_FRAME | (rr.HYBRID_RESTIR_LIGHTS if restir else 0))
    g, d = gbuf(gpu), gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    res = vis = None
    if restir:
        res, vis = gpu.read_reservoirs(2), gpu.read_hybrid(rr.HYBRID_LIGHT_VISIBILITY)
    ref = cr.deferred(g, gpu.read_hybrid(rr.HYBRID_SHADOWS), gpu.read_hybrid(rr.HYBRID_REFLECTIONS), gpu.read_hybrid(rr.HYBRID_SSAO_IMAGE), v, meshes, lights,
                      maps=world.maps if ibl else None, shadow=world.shadow if shadows else None, res=res, vis=vis)
    geo = g["position"][..., 3] != 0
    assert geo.any() and not geo.all() and np.isfinite(d[geo]).all()
    u = ulps(d[geo][:, :3], ref[geo][:, :3])
    print(f"ibl {ibl} shadows {shadows} restir {restir} ssao {ssao}: max {u.max()} ulp, exact on {(u == 0).mean():.4f} of the geometry pixels' channels")
    assert u.max() <= (CONSUMER_ULP if ibl else DEFERRED_ULP), u.max()
    # the frame reaches what the variant is there for
    typ = np.array([m["type"] for m in meshes] + [0.0], np.float32)[np.minimum(g["pbr"][..., 3].astype(np.uint32), len(meshes))]
    assert (geo & (typ == 1.0)).any() and (geo & (typ != 1.0)).any(), "metal and matte pixels"
    assert gpu.hybrid_frame_stats().lights == (2 if restir else v.num_lights + 1)
    if shadows:
        factor, cascade = (a.reshape(H, W) for a in cr.shadow_factor(g, v, world.shadow))
        for c in range(4):
            assert (geo & (cascade == c)).any(), f"no geometry pixel in cascade {c}"
        assert (factor[geo] < 1.0).any() and (factor[geo] == 1.0).any()
    else:
        assert (gpu.read_hybrid(rr.HYBRID_SHADOWS)[geo] == 0).any(), "rt_shadows darkens some pixel"
    if restir:
        cast = rl.cast_mask(g, res, v, lights)
        assert set(np.unique(vis[cast])) == {0, 255} and not vis[~cast].any()
        if not ibl:  # the sun's term, the constant ambient and the factors are exact: bit for bit where no reservoir light is added
            quiet = geo & ~cast
            assert quiet.any() and np.array_equal(bits(d[quiet]), bits(ref[quiet]))
        matte = geo & (typ != 1.0)
        assert (matte & (vis == 255)).any(), "the reservoir's term reaches the image on some matte pixel"
        return int((matte & (vis == 255)).sum()), int((matte & cast & (vis == 0)).sum())
    return 0, 0
