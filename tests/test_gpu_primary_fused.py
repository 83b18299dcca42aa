"""-m gpu: option "fused_primary". Where the plan allows it (csrc/frame_plan.h SamplePlan::fused_primary: camera grid, primary_implicit,
slim state, no pixel handed to the tree, count_visits off, no tile partition) bounce 0 of a pass is one kernel, k_primary_shade, in place
of k_generate, k_trace_camera_grid and k_shade_hit(0). Both settings must give the same words everywhere - accumulation image, output
image, every ray count, hit and miss counts -, option 1 must hold against the oracle, and every pass the plan does not allow it for must
run the three kernels (their time is booked as camera_grid_ms; the one kernel's as shade_ms) and give the same words too."""
import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from test_gpu_sun_verdicts import SUN, WAVEFRONT, batches, one_by_one, same_everywhere
from util import L2_TOL, per_pixel_l2

pytestmark = pytest.mark.gpu

PT = rr.PASS_REFERENCE_PT
# (W, H, the call, the options it needs to run as a wavefront): one frame per call; three frames in one call - 97 * 61 * 3 is no multiple
# of 64, so the last run is partial, and 97 * 61 is none either, so runs hold ids of two frames
SHAPES = {"64x48_one_frame": (64, 48, one_by_one(1), WAVEFRONT), "97x61_three_frames": (97, 61, batches(3), {})}


@pytest.fixture(scope="module")
def atrium():
    return rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=0, sphere_subdivisions=2)


@pytest.fixture(scope="module")
def cornell():
    return rr.scenes.cornell_scene(subdivisions=2, tex_size=16)


@pytest.fixture(scope="module")
def one_light_atrium():
    return rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=1, sphere_subdivisions=2)


def render(scene, W, H, fused, drive, options=(), mask=PT, prepare=None, **flags):
    """the call twice: the first settles the camera (and the sun) so that the second goes through the grids; the kernel times and the
    counts are the second call's"""
    r = scene.upload(rr.Renderer(W, H))
    r.set_option("fused_primary", fused)
    r.set_option("time_kernels", 1)
    r.set_option("camera_grid_max_mean_list_x10", 100000)  # never refused for its worth: these frames are small, their pixels large
    for k, v in dict(options).items():
        r.set_option(k, v)
    if prepare:
        prepare(r)
    view = dict(sun_shadow_enabled=1, sky_enabled=1, lights_enabled=0)
    view.update(flags)
    loop = rr.FrameLoop(r, scene.make_view(W, H, **view))
    loop.view.sun_dir[:] = list(SUN)
    drive(loop, mask)
    r.reset_stats()
    drive(loop, mask)
    return r


def pair(scene, W, H, drive, **kw):
    on, off = (render(scene, W, H, v, drive, **kw) for v in (1, 0))
    s_on, s_off = same_everywhere(on, off, str(kw))
    assert s_on.camera_grid_cells == W * H and s_off.camera_grid_cells == W * H, "the second call did not go through the camera grid"
    assert s_off.camera_grid_ms > 0.0, "option 0: the camera-grid kernel did not run"
    assert s_on.shade_ms > 0.0
    return on, s_on


def ran_fused(s):
    return s.camera_grid_ms == 0.0 and s.camera_tree_rays == 0


# ---- the passes the plan allows it for
@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(request, scene_name, shape):
    scene = request.getfixturevalue(scene_name)
    W, H, drive, options = SHAPES[shape]
    on, s = pair(scene, W, H, drive, options=options)
    assert ran_fused(s), "option 1: the three kernels ran"
    assert s.rays[rr.RAY_PRIMARY] > 0 and s.closest_hits > 0 and s.misses > 0 and s.rays[rr.RAY_SUN_SHADOW] > 0
    assert (on.read_accumulation()[..., :3] > 0).any()


@pytest.mark.parametrize("bounces", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bounce_0_is_the_last_or_the_one_before(atrium, cornell, shape, bounces):
    W, H, drive, options = SHAPES[shape]
    for scene in (atrium, cornell):
        _, s = pair(scene, W, H, drive, options=options, num_bounces=bounces)
        assert ran_fused(s)
        assert (s.rays[rr.RAY_BOUNCE] > 0) == (bounces == 2)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_sky_off(atrium, shape):
    W, H, drive, options = SHAPES[shape]
    _, s = pair(atrium, W, H, drive, options=options, sky_enabled=0)
    assert ran_fused(s) and s.misses > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_furnace(atrium, shape):
    W, H, drive, options = SHAPES[shape]
    _, s = pair(atrium, W, H, drive, options={"furnace": 1, **options})
    assert ran_fused(s) and s.misses > 0


# ---- the passes it is not for: the three kernels run under either setting
def test_fallback_pixels_handed_to_the_tree(atrium):
    """lists of more than one packet are not walked by the grid kernel: their rays go to the tree walk behind it (Q_CAM_TREE)"""
    W, H, drive, options = SHAPES["97x61_three_frames"]
    _, s = pair(atrium, W, H, drive, options={"camera_grid_max_walk": 1, "camera_grid_walk_whole": 0, **options})
    assert s.camera_grid_ms > 0.0 and 0 < s.camera_tree_rays <= s.rays[rr.RAY_PRIMARY]


def test_long_lists_walked_whole_are_fused(atrium):
    """... and with walk_whole raised instead, the unsorted lists are walked whole by the one kernel as by the grid kernel"""
    W, H, drive, options = SHAPES["97x61_three_frames"]
    _, s = pair(atrium, W, H, drive, options={"camera_grid_max_walk": 1, "camera_grid_walk_whole": 512, **options})
    assert ran_fused(s)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fallback_count_visits(atrium, shape):
    W, H, drive, options = SHAPES[shape]
    on, s = pair(atrium, W, H, drive, options={"count_visits": 1, **options})
    assert s.camera_grid_ms > 0.0 and s.camera_grid_tris_tested > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fallback_two_samples_per_frame(atrium, shape):
    W, H, drive, options = SHAPES[shape]
    _, s = pair(atrium, W, H, drive, options=options, samples_per_frame=2)
    assert s.camera_grid_ms > 0.0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fallback_one_light(one_light_atrium, shape):
    W, H, drive, options = SHAPES[shape]
    _, s = pair(one_light_atrium, W, H, drive, options=options, mask=rr.PASS_ALL, lights_enabled=1)
    assert s.camera_grid_ms > 0.0 and s.rays[rr.RAY_LIGHT_SHADOW] > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fallback_tile_partition(atrium, shape):
    """ids are then not pixels: the owned-pixel list stands between them"""
    W, H, drive, options = SHAPES[shape]
    _, s = pair(atrium, W, H, drive, options=options, prepare=lambda r: r.set_tile_partition(1, 3, 16))
    assert s.camera_grid_ms > 0.0 and 0 < s.rays[rr.RAY_PRIMARY] < 3 * W * H


def test_fallback_lone_frame_in_the_fused_kernel(atrium):
    """a frame per call with the defaults: bounces 1.. inside k_path_fused, which wants the classic state in front of it"""
    W, H, drive, _ = SHAPES["64x48_one_frame"]
    _, s = pair(atrium, W, H, drive)
    assert s.camera_grid_ms > 0.0


# ---- against the oracle
@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_oracle(request, scene_name, shape):
    scene = request.getfixturevalue(scene_name)
    W, H, drive, options = SHAPES[shape]
    for sky in (0, 1):
        gpu = render(scene, W, H, 1, drive, options=options, sky_enabled=sky)
        assert ran_fused(gpu.get_stats())
        n = 2 * (3 if shape == "97x61_three_frames" else 1)  # both calls' frames
        cpu = scene.upload(oa.OracleRenderer(W, H))
        loop = rr.FrameLoop(cpu, scene.make_view(W, H, sun_shadow_enabled=1, sky_enabled=sky, lights_enabled=0))
        loop.view.sun_dir[:] = list(SUN)
        one_by_one(n // 2)(loop, PT)
        first_call = list(cpu.get_stats().rays)[:4]
        one_by_one(n // 2)(loop, PT)
        got, want = gpu.read_accumulation(), cpu.read_accumulation()
        if sky == 0:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        else:
            assert per_pixel_l2(got / n, want / n) <= L2_TOL
        assert list(gpu.get_stats().rays)[:4] == [a - b for a, b in zip(list(cpu.get_stats().rays)[:4], first_call)]
