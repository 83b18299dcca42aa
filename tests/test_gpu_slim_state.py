"""-m gpu: option "slim_state". A pass with sun verdicts and one sample per frame carries the slim path state (device_types.h PathState:
the path id beside the origin, throughput | radiance.r and a (g, b) pair, no id queues behind bounce 0), and the sun kernels of its
last bounce store the surviving paths' radiance themselves instead of k_flush_survivors. Every other pass keeps the four-quad state. Both settings must give the same
words everywhere: accumulation image, output image, ray counts, hit and miss counts - and the same as the oracle."""
import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from test_gpu_sun_verdicts import SUN, WAVEFRONT, batches, one_by_one, same_everywhere
from util import L2_TOL, per_pixel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def atrium():
    return rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=0, sphere_subdivisions=2)


@pytest.fixture(scope="module")
def cornell():
    return rr.scenes.cornell_scene(subdivisions=2, tex_size=16)


@pytest.fixture(scope="module")
def lit_atrium():
    return rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=48, sphere_subdivisions=2)


def make(scene, W, H, slim, options=(), prepare=None, **flags):
    """a renderer with the scene and its frame loop; slim: the option's value"""
    r = scene.upload(rr.Renderer(W, H))
    r.set_option("slim_state", slim)
    for k, v in dict(options).items():
        r.set_option(k, v)
    if prepare:
        prepare(r)
    view = dict(sun_shadow_enabled=1, sky_enabled=1, lights_enabled=0)
    view.update(flags)
    loop = rr.FrameLoop(r, scene.make_view(W, H, **view))
    loop.view.sun_dir[:] = list(SUN)
    return r, loop


def render(scene, W, H, slim, drive, mask=rr.PASS_REFERENCE_PT, **kw):
    r, loop = make(scene, W, H, slim, **kw)
    drive(loop, mask)
    return r


def pair(scene, W, H, drive, **kw):
    on, off = (render(scene, W, H, v, drive, **kw) for v in (1, 0))
    sa, _ = same_everywhere(on, off, str(kw))
    return on, off, sa


def acc_bits(r):
    return r.read_accumulation().view(np.uint32)


# ---- frame forms at 128 x 72
@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
def test_one_frame_per_call(request, scene_name):
    scene = request.getfixturevalue(scene_name)
    on, _, s = pair(scene, 128, 72, one_by_one(3), options=WAVEFRONT)
    assert s.sun_grid_cells > 0 and s.rays[rr.RAY_SUN_SHADOW] > 0
    assert (on.read_accumulation()[..., :3] > 0).any()


@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
def test_batches_of_sixteen_frames(request, scene_name):
    scene = request.getfixturevalue(scene_name)
    _, _, s = pair(scene, 128, 72, batches(16))
    assert s.sun_grid_cells > 0
    # and the slim batch equals the frames one by one in the classic form
    a = render(scene, 128, 72, 1, batches(16))
    b = render(scene, 128, 72, 0, one_by_one(16), options=WAVEFRONT)
    assert np.array_equal(acc_bits(a), acc_bits(b))


@pytest.mark.parametrize("size", [(67, 41), (33, 5), (130, 73)])
def test_queue_counts_that_are_not_multiples_of_64(atrium, size):
    W, H = size
    for drive in (one_by_one(2), batches(5)):
        pair(atrium, W, H, drive, options=WAVEFRONT)


@pytest.mark.parametrize("bounces", [1, 2, 5])
@pytest.mark.parametrize("drive", [one_by_one(2), batches(4)], ids=["one_by_one", "batch"])
def test_number_of_bounces(atrium, cornell, bounces, drive):
    """one bounce: the final form runs straight behind k_shade_hit(0), with no stored radiance"""
    for scene in (atrium, cornell):
        _, _, s = pair(scene, 96, 54, drive, options=WAVEFRONT, num_bounces=bounces)
        assert s.rays[rr.RAY_SUN_SHADOW] > 0


def test_zero_bounces(atrium):
    for drive in (one_by_one(2), batches(4)):
        _, _, s = pair(atrium, 96, 54, drive, options=WAVEFRONT, num_bounces=0)
        assert s.path_rays == 0


def test_tile_partition(atrium):
    """ids are then not pixels"""
    for drive in (one_by_one(2), batches(4)):
        _, _, s = pair(atrium, 200, 120, drive, options=WAVEFRONT, prepare=lambda r: r.set_tile_partition(1, 3, 64))
        assert s.rays[rr.RAY_SUN_SHADOW] > 0


def test_leftovers_store_the_radiance(atrium):
    """a grid whose kernel walks lists of two entries at most: many rays go to the tree walk behind it, whose final form stores the
    radiance of every ray it ends, lit or not"""
    options = {"sun_grid_max_walk": 2, "sun_grid_force": 1, **WAVEFRONT}
    for drive in (one_by_one(2), batches(4)):
        on, _, s = pair(atrium, 128, 72, drive, options=options)
        assert s.sun_tree_rays > 0 and s.sun_grid_cells > 0
        assert s.sun_tree_rays * 20 > s.rays[rr.RAY_SUN_SHADOW], "only a handful of rays went to the tree: the test does not test its kernel"
        tree = render(atrium, 128, 72, 1, drive, options={"sun_grid": 0, **WAVEFRONT})
        assert np.array_equal(acc_bits(on), acc_bits(tree))


# ---- passes that keep the four-quad state: either option value gives the classic words
@pytest.mark.parametrize("drive", [one_by_one(2), batches(4)], ids=["one_by_one", "batch"])
def test_fallback_three_samples_per_frame(atrium, drive):
    pair(atrium, 96, 54, drive, options=WAVEFRONT, samples_per_frame=3)


def test_fallback_lights_enabled(lit_atrium):
    for drive in (one_by_one(2), batches(6)):
        for options in ({}, WAVEFRONT):
            _, _, s = pair(lit_atrium, 128, 72, drive, options=options, mask=rr.PASS_ALL, lights_enabled=1)
            assert s.rays[rr.RAY_LIGHT_SHADOW] > 0 and s.sun_grid_cells > 0


def test_fallback_sun_shadows_disabled(atrium):
    for drive in (one_by_one(2), batches(4)):
        _, _, s = pair(atrium, 96, 54, drive, options=WAVEFRONT, sun_shadow_enabled=0)
        assert s.rays[rr.RAY_SUN_SHADOW] == 0


def test_fallback_tree_walk_of_the_sun_rays(atrium):
    for drive in (one_by_one(2), batches(4)):
        _, _, s = pair(atrium, 128, 72, drive, options={"sun_grid": 0, **WAVEFRONT})
        assert s.sun_grid_cells == 0


def test_fallback_fused_frames(atrium, cornell):
    """a frame per call with the defaults: bounces 1.. inside k_path_fused"""
    for scene in (atrium, cornell):
        pair(scene, 128, 72, one_by_one(3))


@pytest.mark.parametrize("options", [{"camera_grid": 0}, {"primary_implicit": 0}], ids=["camera_grid_0", "primary_implicit_0"])
def test_generated_state_carries_the_id(atrium, cornell, options):
    """k_generate then writes the state of bounce 0, with the id in the origin's word"""
    for scene in (atrium, cornell):
        for drive, more in ((one_by_one(2), WAVEFRONT), (batches(5), {})):
            pair(scene, 128, 72, drive, options={**options, **more})
            pair(scene, 67, 41, drive, options={**options, **more}, num_bounces=1)


# ---- slim and classic passes in turn on the same slots: what one leaves in the planes and queues must not reach the other
@pytest.mark.parametrize("in_flight", [1, 4])
def test_call_sequence_on_one_renderer(lit_atrium, in_flight):
    """one renderer through slim passes of several sizes, a fused frame, a lights-on frame (classic wavefronts, which write the id
    queues and the four-quad planes) and new tile partitions, step by step against one that never runs the slim state"""
    W, H = 128, 72
    options = {"frames_in_flight": in_flight}
    both = [make(lit_atrium, W, H, slim, options=options) for slim in (1, 0)]

    def step(what, fn):
        for r, loop in both:
            fn(r, loop)
        same_everywhere(both[0][0], both[1][0], what)

    def lights_on_frame(r, loop):
        loop.view.lights_enabled = 1
        loop.frame(rr.PASS_ALL)
        loop.view.lights_enabled = 0

    pt = rr.PASS_REFERENCE_PT
    step("frames(16)", lambda r, loop: loop.frames(16, pt))
    step("frames(16) again", lambda r, loop: loop.frames(16, pt))
    step("frames(4): another n", lambda r, loop: loop.frames(4, pt))
    step("frames(4) again", lambda r, loop: loop.frames(4, pt))
    step("frame(): the fused kernel's lists", lambda r, loop: loop.frame(pt))
    step("frames(4) behind the fused frame", lambda r, loop: loop.frames(4, pt))
    step("a lights-on frame: a classic wavefront", lights_on_frame)
    for k in range(in_flight + 1):  # every slot again
        step(f"frames(4) behind the lights-on frame, {k}", lambda r, loop: loop.frames(4, pt))
    step("a new tile partition", lambda r, loop: r.set_tile_partition(1, 3, 64))
    for k in range(in_flight + 1):
        step(f"frames(4) under the partition, {k}", lambda r, loop: loop.frames(4, pt))
    step("the partition of rank 0 of 2", lambda r, loop: r.set_tile_partition(0, 2, 64))
    step("frames(4) under the second partition", lambda r, loop: loop.frames(4, pt))
    step("frames(4) again", lambda r, loop: loop.frames(4, pt))
    step("rank 1 of 2: as many ids, other pixels", lambda r, loop: r.set_tile_partition(1, 2, 64))
    for k in range(in_flight + 1):
        step(f"frames(4) under the third partition, {k}", lambda r, loop: loop.frames(4, pt))


# ---- against the oracle
@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
def test_against_the_oracle(request, scene_name):
    scene = request.getfixturevalue(scene_name)
    W, H, n = 128, 72, 4
    for sky in (0, 1):
        cpu = scene.upload(oa.OracleRenderer(W, H))
        loop = rr.FrameLoop(cpu, scene.make_view(W, H, sun_shadow_enabled=1, sky_enabled=sky, lights_enabled=0))
        loop.view.sun_dir[:] = list(SUN)
        one_by_one(n)(loop, rr.PASS_REFERENCE_PT)
        want = cpu.read_accumulation()
        for drive in (one_by_one(n), batches(n)):
            gpu = render(scene, W, H, 1, drive, options=WAVEFRONT, sky_enabled=sky)
            got = gpu.read_accumulation()
            if sky == 0:
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            else:
                assert per_pixel_l2(got / n, want / n) <= L2_TOL
            assert list(gpu.get_stats().rays)[:4] == list(cpu.get_stats().rays)[:4]
