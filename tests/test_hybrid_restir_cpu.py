"""CPU: the restatement of the hybrid frame's reservoir lights (tests/hybrid_restir_reference.py) on the oracle. Its split of the deferred
pass's light loop equals hybrid_frame_reference.deferred bit for bit; the cast rule and the rays have known answers; and the estimator the
frame computes - one light per pixel from the spatial reservoir, weighted by W_X, times the ray's verdict - is unbiased for the shadowed
sum over all lights, while the same sum without shadows lies far outside its error (the negative control)."""
import numpy as np
import pytest

import hybrid_frame_reference as fr
import hybrid_reference as hr
import hybrid_restir_reference as rl
import oracle_api as oa
import rust_renderer_amd as rr
from hybrid_util import frame_view, synthetic_scene

W, H = 48, 36
K = 64  # independent frames
F = np.float32


@pytest.fixture(scope="module")
def world():
    """the synthetic scene with the lights on the oracle, its hybrid G-buffer and deferred surface terms, and the truth: every light's
    visibility from every pixel that faces it"""
    scene = synthetic_scene()
    cpu = oa.OracleRenderer(W, H)
    meshes = hr.upload_recorded(scene, cpu, defaults=False)
    lights = rl.occluded_lights()
    for l in lights:
        cpu.add_gpu_light(l)
    cpu.initialize_raytracing()
    view = frame_view(scene, W, H)
    view.num_lights = len(lights)
    g = hr.gbuffer(cpu, meshes, view, W, H)
    s = rl.surface_terms(g, view, meshes)
    pairs = rl.all_lights_visibility(cpu, g, view, lights)
    return dict(scene=scene, cpu=cpu, meshes=meshes, lights=lights, view=view, g=g, s=s, pairs=pairs)


def test_the_split_light_loop_equals_the_deferred_reference_bit_for_bit(world):
    g, view, meshes, lights = world["g"], world["view"], world["meshes"], world["lights"]
    rng = np.random.default_rng(5)
    sh = rng.integers(0, 256, (H, W)).astype(np.uint8)
    refl = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    ss = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    for kw in (dict(), dict(ssao_enabled=0), dict(raytracing_supported=0)):
        v = frame_view(world["scene"], W, H, **kw)
        v.num_lights = len(lights)
        a = rl.deferred_all_lights(g, sh, refl, ss, v, meshes, lights)
        b = fr.deferred(g, sh, refl, ss, v, meshes, lights)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kw


def _reservoirs(Y, WX):
    r = np.zeros((H, W), rr.RESERVOIR_DTYPE)
    r["Y"], r["W_X"], r["W_sum"], r["M"] = Y, WX, 1.0, 1
    return r


def test_the_cast_rule(world):
    g, view, lights = world["g"], world["view"], world["lights"]
    geo = g["position"][..., 3] != 0
    assert geo.any() and not geo.all(), "the upper rows see the sky"
    base = rl.cast_mask(g, _reservoirs(3, 1.0), view, lights)
    assert base.any() and not base[~geo].any(), "sky pixels cast nothing"
    facing = rl.light_geometry(fr.light_records(view, lights)[4], g["position"][..., :3].reshape(-1, 3))[0]
    ndl = hr.dot(g["normal"][..., :3].reshape(-1, 3), facing).reshape(H, W)
    assert np.array_equal(base, geo & (ndl > 0)), "exactly the geometry pixels that face light 3"
    for Y, WX in ((-1, 1.0), (len(lights), 1.0), (3, 0.0), (3, -1.0), (3, np.inf), (3, np.nan)):
        assert not rl.cast_mask(g, _reservoirs(Y, WX), view, lights).any(), (Y, WX)
    fewer = frame_view(world["scene"], W, H)
    fewer.num_lights = 3
    assert not rl.cast_mask(g, _reservoirs(3, 1.0), fewer, lights).any(), "light 3 is beyond this call's num_lights"
    directional = rl.occluded_lights()
    directional[3].light_type = 0.0
    assert not rl.cast_mask(g, _reservoirs(3, 1.0), view, directional).any(), "only point and spot lights"


def test_a_ray_is_occluded_exactly_by_what_lies_before_the_light(world):
    """a floor point under the rim of the metal sphere (radius 0.7 about (0.6, 0.7, 1.4): above the point it spans y 0.21 .. 1.19), the
    light straight above: occluded with the light above the sphere, visible with the light below it"""
    cpu = world["cpu"]
    g = dict(position=np.zeros((1, 1, 4), np.float32), normal=np.zeros((1, 1, 4), np.float32))
    g["position"][0, 0] = (0.6, 0.0, 1.9, 1.0)
    g["normal"][0, 0] = (0.0, 1.0, 0.0, 1.0)
    for height, want in ((3.0, True), (0.7, True), (0.15, False)):
        o, d, dist = rl.shadow_rays(g, np.array([0]), np.array([[0.6, height, 1.9]], np.float32))
        assert np.allclose(d, (0, 1, 0)) and abs(dist[0] - height) < 1e-4
        assert rl.occluded(cpu, o, d, dist)[0] == want, height


def _frame_sums(world, spatial):
    """S_k of K independent frames: the image sum, per channel, of the restatement's reservoir term"""
    cpu, g, s, lights = world["cpu"], world["g"], world["s"], world["lights"]
    sums = np.zeros((K, 3), np.float64)
    for k in range(K):
        v = frame_view(world["scene"], W, H, temporal_reuse_enabled=0, spatial_reuse_enabled=spatial)
        v.num_lights = len(lights)
        v.total_samples = k + 1
        cpu.render_frame(v, rr.PASS_RESTIR)
        res = cpu.read_reservoirs(2)
        vis, rays, occluded = rl.visibility(cpu, g, res, v, lights)
        term, lit = rl.reservoir_term(s, v, lights, res, vis)
        assert rays > 0 and 0 < occluded < rays and lit.sum() == rays - occluded
        sums[k] = term.astype(np.float64).sum(axis=0)
    return sums


def test_the_estimator_is_unbiased_and_the_unshadowed_sum_is_not_what_it_estimates(world):
    """|mean_k S_k - S_truth| <= 5 std_k(S_k) / sqrt(K) per channel, with spatial reuse on; and the same sum with visibility dropped lies
    outside that bound (the lights are placed so that at least 10 % of the facing (pixel, light) pairs are occluded)"""
    s, view, lights, pairs = world["s"], world["view"], world["lights"], world["pairs"]
    facing = sum(len(rows) for rows, _ in pairs)
    hidden = sum(int((~visible).sum()) for _, visible in pairs)
    print(f"facing pairs {facing}, occluded {hidden} ({hidden / facing:.3f})")
    assert hidden >= 0.10 * facing
    truth = rl.brute_force_sum(s, view, lights, pairs)
    unshadowed = rl.brute_force_sum(s, view, lights, pairs, shadowed=False)
    sums = _frame_sums(world, spatial=1)
    mean, sigma = sums.mean(axis=0), sums.std(axis=0, ddof=1) / np.sqrt(K)
    z, z_control = (mean - truth) / sigma, (mean - unshadowed) / sigma
    print(f"truth {truth}, mean {mean}, sigma of the mean {sigma}, per-frame relative std {sums.std(axis=0, ddof=1) / mean}")
    print(f"z {z}, z of the unshadowed sum {z_control}")
    assert (np.abs(z) <= 5.0).all(), z
    assert (np.abs(z_control) > 5.0).all(), z_control
