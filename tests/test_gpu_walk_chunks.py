"""GPU: the hybrid frame's persistent walking kernels (k_rtgi_trace<0|1>, k_rtgi_shadow, k_rtao_trace<0|1|2> and the per-pixel walks of
rt_shadows and the reservoir lights) at frames where a wave comes back for a second and a third chunk of 64 items: the
static chunk stride (traversal.h Feeder::advance: chunk k of wave w = (k * num_waves + w) * 64), the three-stage refill pipeline across
more than one advance, the partial last chunk in a wave that already did a full one, and k_rtgi_trace's idle predicate, which keeps a
lane that waits to be shaded from taking another ray. Option "trace_blocks_per_cu" = 1 makes the grids small enough for that at frames
the restatements (tests/rtgi_reference.py, tests/rtao_reference.py) still compute in seconds; the per-pixel walks, which have no
restatement at this size, are held to the same device at 8 blocks per CU, where no wave refills (the small-frame tests hold that case
to the restatements). tests/test_rtgi_cpu.py proves on the oracle's G-buffer that the frames chosen here are adequate."""
import numpy as np
import pytest

import rtao_reference as ao
import rtgi_reference as gi
import rust_renderer_amd as rr
from hybrid_util import bits
from test_gpu_hybrid_restir import World as LitWorld
from test_gpu_rtao import World as AoWorld
from test_gpu_rtgi import RTGI, World, integers, plain_deferred

pytestmark = pytest.mark.gpu

# The header does not report the CU count. With trace_blocks_per_cu = 1 the persistent grids hold at most 256 CUs x 1 block x 256 lanes
# (fewer where the occupancy clamp of uh_create bites or the device has fewer CUs, which only makes a wave refill sooner).
LANES = 65536
assert LANES == gi.WALK_LANES


def one_block_per_cu(world):
    world.gpu.set_option("trace_blocks_per_cu", 1)
    return world


# ---- A1: the closed box -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    return one_block_per_cu(World(gi.inward_box_scene(), *gi.WALK_BOX_SIZE))


@pytest.mark.parametrize("blur_radius", [0, 6])
@pytest.mark.parametrize("order", [0, 1])
def test_a_box_of_three_grids_of_rays_equals_the_restatement(box, order, blur_radius):
    """131 x 97 at 16 samples: every pixel casts and no ray misses, 203,312 items, 3.1 x LANES: every wave of k_rtgi_trace takes a third
    chunk and some a fourth, and k_rtgi_shadow's 49,529 sun rays (all occluded) stay within one grid"""
    Ww, Hh = box.size
    samples = 16
    assert samples * Ww * Hh >= 3 * LANES
    v = box.view()
    box.gpu.set_option("rtgi_order", order)
    try:
        box.render(v, rr.HYBRID_FRAME, samples=samples, blur_radius=blur_radius)
        plain = box.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
        box.render(v, samples=samples, blur_radius=blur_radius)
        got = box.check(v, plain)
    finally:
        box.gpu.set_option("rtgi_order", 0)
    assert got["cast"].all() and got["exact"].all() and (got["counts"] == (0, samples, 0, 0)).all()
    s = box.gpu.rtgi_stats()
    assert s.pixels == Ww * Hh and s.rays == samples * Ww * Hh and s.misses == 0 and 0 < s.shadow_rays < s.rays
    assert np.array_equal(bits(got["deferred"]), bits(plain)), "nothing arrives inside a closed box"


# ---- A2: the emissive box, three samples ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emissive():
    return one_block_per_cu(World(gi.emissive_box_scene(), *gi.WALK_EMISSIVE_SIZE)), World(gi.emissive_box_scene(), *gi.WALK_EMISSIVE_SIZE)


@pytest.mark.parametrize("order", [0, 1])
def test_three_samples_split_no_chunk_evenly_and_the_last_chunk_is_partial(emissive, order):
    """263 x 167 at 3 samples: 131,763 items, 2.01 x LANES; a chunk of 64 items holds 21 pixels and a third of another (order 0), and the
    last chunk has 51 items and lands in a wave that already walked two full ones. No ray misses, so every pixel is bit for bit"""
    w, t = emissive
    Ww, Hh = w.size
    samples = 3
    assert samples * Ww * Hh >= 2 * LANES and (samples * Ww * Hh) % 64 != 0
    v = w.view()
    w.gpu.set_option("rtgi_order", order)
    try:
        w.render(v, samples=samples, blur_radius=0, max_radiance=0.5)
        got = w.check(v, plain_deferred(t, v))
    finally:
        w.gpu.set_option("rtgi_order", 0)
    assert got["cast"].all() and got["exact"].all(), "no ray misses: every pixel is held bit for bit"
    lit_ = got["counts"][..., gi.EMITTER] > 0
    assert 0.25 < lit_.mean() < 1 and (got["radiance"][lit_][:, :3] > 0).all() and (got["radiance"][..., :3] <= 0.5).all()
    assert not got["counts"][..., gi.SUNLIT].any() and not got["counts"][..., gi.MISSED].any()
    # a ray that meets the emitter brings min(emission, max_radiance) = 0.5 on every channel, every other ray of this box nothing: sums of
    # halves are exact, so the mean is one rounding
    want = (got["counts"][..., gi.EMITTER].astype(np.float32) * np.float32(0.5)) / np.float32(samples)
    assert np.array_equal(got["radiance"][..., :3], np.repeat(want[..., None], 3, axis=-1))
    assert (got["counts"].sum(axis=-1) == samples).all() and w.gpu.rtgi_stats().rays == samples * Ww * Hh


# ---- A3: the courtyard, where the sun rays refill too ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_yard():
    return one_block_per_cu(World(gi.courtyard_scene(), *gi.WALK_YARD_SIZE)), World(gi.courtyard_scene(), *gi.WALK_YARD_SIZE)


@pytest.mark.parametrize("order", [0, 1])
def test_the_sun_rays_of_a_lit_yard_refill_too(big_yard, order):
    """the courtyard at 183 x 113 and 16 samples: the smallest frame of its family (odd widths at the 67 : 41 shape of the small frame)
    at which the restatement on the oracle's G-buffer casts at least 2 x LANES sun rays: 20,001 pixels cast 320,016 rays (4.9 x LANES),
    134,390 sun rays (2.05 x LANES), 25,479 rays miss; the restatement takes 3.1 s of CPU, shared by both orders (test_rtgi_cpu.py
    asserts the counts). Sunlit, shadowed, dark and missed rays all occur, so k_rtgi_trace's waves shade mixed batches between refills
    and k_rtgi_shadow walks its third chunk."""
    w, t = big_yard
    samples = 16
    v = w.view()
    w.gpu.set_option("rtgi_order", order)
    try:
        w.render(v, samples=samples, blur_radius=3)
        got = w.check(v, plain_deferred(t, v))
    finally:
        w.gpu.set_option("rtgi_order", 0)
    s = w.gpu.rtgi_stats()
    assert s.rays >= 3 * LANES and s.shadow_rays >= 2 * LANES and s.misses > 0
    assert got["counts"][..., gi.SUNLIT].any() and got["counts"][..., gi.DARK].any() and (got["exact"] & got["cast"]).any() and (~got["exact"]).any()
    assert int(got["counts"][..., gi.SUNLIT].sum()) < s.shadow_rays, "some sun rays were occluded"


# ---- RTAO ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ao_box():
    return one_block_per_cu(AoWorld(ao.inward_box_scene(), *gi.WALK_AO_SIZE))


@pytest.mark.parametrize("order", [0, 1, 2])
def test_rtao_at_three_grids_of_rays_equals_the_restatement(ao_box, order):
    """the closed box at 71 x 45 and 64 samples, the cap: 204,480 rays, 3.1 x LANES, for orders 0 and 1. Order 2 is one item per pixel:
    3,195 items, still one chunk per wave at this size (a frame of 2 x LANES pixels at any sample count is beyond the restatement); its
    refill is held by test_the_per_pixel_walks_do_not_depend_on_the_grid below, device against device"""
    Ww, Hh = ao_box.size
    samples = ao.MAX_SAMPLES
    assert Ww * Hh * samples >= 3 * LANES
    v = ao_box.view()
    ao_box.gpu.set_option("rtao_order", order)
    try:
        ao_box.render(v, samples=samples, radius=ao.BOX_RADIUS, blur_radius=2)
        g, count, img = ao_box.check(v)
    finally:
        ao_box.gpu.set_option("rtao_order", 0)
    assert (g["position"][..., 3] != 0).all() and (count == samples).all() and (img == 0).all()
    s = ao_box.gpu.rtao_stats()
    assert s.pixels == Ww * Hh and s.occluded == s.rays == samples * Ww * Hh


# ---- the per-pixel walks, device against device -----------------------------------------------------------------------------------
DIFF_W, DIFF_H = 461, 289
DIFF_CAMERA = ((0.0, 3.0, 4.5), (0.0, 0.0, 0.5))  # eye, target: looking down at the floor, the sky above its far edge
DIFF_MASK = rr.HYBRID_FRAME | rr.HYBRID_RTAO | rr.HYBRID_RESTIR_LIGHTS | RTGI
# what read_hybrid gives after a call with DIFF_MASK: the frame's nine, the light visibility, the AO counts and the rtgi pass's two (the
# marching-cubes, rasterised G-buffer, motion and taa images belong to passes that do not run here)
DIFF_IMAGES = list(range(9)) + [rr.HYBRID_LIGHT_VISIBILITY, rr.HYBRID_AO_COUNTS, rr.HYBRID_GI_RADIANCE, rr.HYBRID_GI_COUNTS]


def every_counter(r):
    h, l, a, g = r.hybrid_stats(), r.hybrid_restir_stats(), r.rtao_stats(), r.rtgi_stats()
    return dict(hybrid=tuple(h.rays) + (h.reflection_pixels,), restir=(l.rays, l.occluded), rtao=(a.pixels, a.rays, a.occluded), rtgi=integers(g))


@pytest.fixture(scope="module")
def two_grids():
    """the reservoir-lights fixture scene (the synthetic scene, 8 occluded lights, three reservoir frames) at 461 x 289 from a camera that
    looks down at the floor, on two contexts fed identically; then one walks with 1 block per CU and one with 8"""
    import hybrid_restir_reference as rl
    from hybrid_util import synthetic_scene

    worlds = []
    for blocks in (1, 8):
        scene = synthetic_scene()
        scene.camera = rr.camera.Camera(*DIFF_CAMERA, 60.0, DIFF_W / DIFF_H, 0.01, 1000.0)
        w = LitWorld(scene, rl.occluded_lights(8), DIFF_W, DIFF_H)
        w.gpu.set_option("trace_blocks_per_cu", blocks)
        worlds.append(w)
    return worlds


@pytest.mark.parametrize("rtao_order, rtgi_order", [(0, 0), (2, 1)])
def test_the_per_pixel_walks_do_not_depend_on_the_grid(two_grids, rtao_order, rtgi_order):
    """the walks that are fed one item per pixel, at 1 block per CU against 8. What refills is what has more than LANES items, and each
    count is asserted: k_hybrid_shadow (rt_shadows) walks all W x H = 133,229 pixels; k_rtao_trace<2> the queued geometry pixels (0.80 of
    the frame on the oracle's G-buffer at a quarter of the size, about 107,000); k_hybrid_restir_trace the queued pixels whose reservoir
    holds a light that faces them (0.62 of the frame there, about 82,000); the per-ray kernels k_rtao_trace<0> (4 samples) and k_rtgi_trace
    (3 samples) more; k_rtgi_shadow's few sun rays here stay within one grid (the courtyard above refills it). At 8 blocks per CU the grid holds 524,288 lanes, more than any of these counts: no wave
    refills, the case the small-frame tests hold to the restatements. rt_reflections is a grid-stride loop the option does not touch:
    it runs the same in both contexts and nothing is held about it here. Every image and every counter is the same."""
    images, counters = [], []
    for w in two_grids:
        v = w.view()
        w.gpu.set_option("rtao_order", rtao_order)
        w.gpu.set_option("rtgi_order", rtgi_order)
        try:
            w.gpu.set_rtao_params(samples=4)
            w.gpu.set_rtgi_params(samples=3, blur_radius=1)
            w.gpu.render_hybrid(v, rr.HYBRID_GBUFFER)  # rt_shadows reads the previous call's G-buffer: this camera's
            w.gpu.render_hybrid(v, DIFF_MASK)
        finally:
            w.gpu.set_option("rtao_order", 0)
            w.gpu.set_option("rtgi_order", 0)
        images.append({i: w.gpu.read_hybrid(i).view(np.uint8) for i in DIFF_IMAGES})
        counters.append(every_counter(w.gpu))
    c = counters[0]
    print(c)
    # every walk's own item count against the two grids: it refills at 1 block per CU and does not at 8
    items = dict(rt_shadows=c["hybrid"][1], rtao_pixels=c["rtao"][0], rtao_rays=c["rtao"][1], restir=c["restir"][0], rtgi=c["rtgi"][1])
    assert items["rt_shadows"] == DIFF_W * DIFF_H
    for name, n in items.items():
        assert LANES < n < 8 * LANES, (name, n)
    assert counters[0] == counters[1]
    a, b = images
    for i in DIFF_IMAGES:
        assert np.array_equal(a[i], b[i]), i
    # the frame is not trivial
    gpu = two_grids[0].gpu
    sky = gpu.read_hybrid(rr.HYBRID_POSITION)[..., 3] == 0
    vis = gpu.read_hybrid(rr.HYBRID_LIGHT_VISIBILITY)
    assert sky.any() and not sky.all()
    assert (vis == 255).any() and 0 < c["restir"][1] < c["restir"][0], "lit and occluded reservoir pixels"
    assert len(np.unique(gpu.read_hybrid(rr.HYBRID_AO_COUNTS))) > 2
    assert c["rtgi"][0] == c["rtao"][0] and c["rtgi"][1] == 3 * c["rtgi"][0] and c["rtgi"][3] > 0 and c["rtao"][1] == 4 * c["rtao"][0]
    assert c["hybrid"][2] > 0 and a[rr.HYBRID_GI_RADIANCE].any()
