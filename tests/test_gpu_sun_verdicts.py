"""-m gpu: option "sun_verdicts". With it (the default) the grid's sun-ray kernels leave one verdict bit per ray and the kernels that
read a path's radiance next - k_shade_hit of the next bounce, the miss shading, k_flush_survivors - add the lit paths' throughput;
without it the sun kernels add it themselves (reference.rgen:69-78). Both forms must give the same words everywhere: accumulation
image, output image, ray counts, hit and miss counts - and the same as the oracle."""
import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from util import L2_TOL, per_pixel_l2

pytestmark = pytest.mark.gpu

SUN = (0.3, 0.8, 0.2)


@pytest.fixture(scope="module")
def atrium():
    return rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=0, sphere_subdivisions=2)


@pytest.fixture(scope="module")
def cornell():
    return rr.scenes.cornell_scene(subdivisions=2, tex_size=16)


def one_by_one(n):
    def drive(loop, mask):
        for _ in range(n):
            loop.frame(mask)
    return drive


def batches(n):
    return lambda loop, mask: loop.frames(n, mask)


def render(scene, W, H, verdicts, drive, options=(), mask=rr.PASS_REFERENCE_PT, prepare=None, **flags):
    r = scene.upload(rr.Renderer(W, H))
    r.set_option("sun_verdicts", verdicts)
    for k, v in dict(options).items():
        r.set_option(k, v)
    if prepare:
        prepare(r)
    view = dict(sun_shadow_enabled=1, sky_enabled=1, lights_enabled=0)
    view.update(flags)
    loop = rr.FrameLoop(r, scene.make_view(W, H, **view))
    loop.view.sun_dir[:] = list(SUN)
    drive(loop, mask)
    return r


def same_everywhere(a, b, what=""):
    sa, sb = a.get_stats(), b.get_stats()
    assert np.array_equal(a.read_accumulation().view(np.uint32), b.read_accumulation().view(np.uint32)), what
    assert np.array_equal(a.read_output_bgra8(), b.read_output_bgra8()), what
    assert sa.path_rays == sb.path_rays and list(sa.rays) == list(sb.rays), what
    assert (sa.closest_hits, sa.misses) == (sb.closest_hits, sb.misses), what
    return sa, sb


def pair(scene, W, H, drive, **kw):
    on, off = (render(scene, W, H, v, drive, **kw) for v in (1, 0))
    sa, _ = same_everywhere(on, off, str(kw))
    return on, off, sa


# the wavefront of a lone frame: the fused kernel (the default for a frame per call) adds its sun terms itself under either setting
WAVEFRONT = {"fused_bounces": 0}


@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
@pytest.mark.parametrize("options", [{}, WAVEFRONT])
def test_one_frame_per_call(request, scene_name, options):
    scene = request.getfixturevalue(scene_name)
    on, _, s = pair(scene, 128, 72, one_by_one(3), options=options)
    assert s.sun_grid_cells > 0 and s.rays[rr.RAY_SUN_SHADOW] > 0
    assert (on.read_accumulation()[..., :3] > 0).any()


@pytest.mark.parametrize("scene_name", ["atrium", "cornell"])
def test_batches_of_sixteen_frames(request, scene_name):
    scene = request.getfixturevalue(scene_name)
    _, _, s = pair(scene, 128, 72, batches(16))
    assert s.sun_grid_cells > 0
    # and the batch equals the frames one by one in the other form
    a = render(scene, 128, 72, 1, batches(16))
    b = render(scene, 128, 72, 0, one_by_one(16), options=WAVEFRONT)
    assert np.array_equal(a.read_accumulation().view(np.uint32), b.read_accumulation().view(np.uint32))


@pytest.mark.parametrize("drive", [one_by_one(2), batches(4)], ids=["one_by_one", "batch"])
def test_three_samples_per_frame(atrium, drive):
    pair(atrium, 96, 54, drive, options=WAVEFRONT, samples_per_frame=3)


@pytest.mark.parametrize("bounces", [1, 2, 5])
@pytest.mark.parametrize("drive", [one_by_one(2), batches(4)], ids=["one_by_one", "batch"])
def test_number_of_bounces(atrium, cornell, bounces, drive):
    """one bounce: the flush is the only reader of the verdicts"""
    for scene in (atrium, cornell):
        _, _, s = pair(scene, 96, 54, drive, options=WAVEFRONT, num_bounces=bounces)
        assert s.rays[rr.RAY_SUN_SHADOW] > 0


@pytest.mark.parametrize("size", [(67, 41), (33, 5), (130, 73)])
def test_queue_counts_that_are_not_multiples_of_64(atrium, size):
    W, H = size
    for drive in (one_by_one(2), batches(5)):
        pair(atrium, W, H, drive, options=WAVEFRONT)


def test_tile_partition(atrium):
    for drive in (one_by_one(2), batches(4)):
        on, _, s = pair(atrium, 200, 120, drive, options=WAVEFRONT, prepare=lambda r: r.set_tile_partition(1, 3, 64))
        assert s.rays[rr.RAY_SUN_SHADOW] > 0


def test_tree_walk_form(atrium):
    """sun_grid = 0: every sun ray walks the tree and adds its term itself under either setting"""
    for drive in (one_by_one(2), batches(4)):
        _, _, s = pair(atrium, 128, 72, drive, options={"sun_grid": 0, **WAVEFRONT})
        assert s.sun_grid_cells == 0
    grid = render(atrium, 128, 72, 1, batches(4))
    tree = render(atrium, 128, 72, 1, batches(4), options={"sun_grid": 0})
    assert np.array_equal(grid.read_accumulation().view(np.uint32), tree.read_accumulation().view(np.uint32))


def test_leftovers_set_their_bits(atrium):
    """a grid whose kernel walks lists of two entries at most: many rays go to the tree walk behind it, which sets the bits of those it
    finds lit in the words the grid kernel stored"""
    options = {"sun_grid_max_walk": 2, "sun_grid_force": 1, **WAVEFRONT}
    for drive in (one_by_one(2), batches(4)):
        on, _, s = pair(atrium, 128, 72, drive, options=options)
        assert s.sun_tree_rays > 0 and s.sun_grid_cells > 0
        assert s.sun_tree_rays * 20 > s.rays[rr.RAY_SUN_SHADOW], "only a handful of rays went to the tree: the test does not test its kernel"
        tree = render(atrium, 128, 72, 1, drive, options={"sun_grid": 0, **WAVEFRONT})
        assert np.array_equal(on.read_accumulation().view(np.uint32), tree.read_accumulation().view(np.uint32))


def test_sun_shadows_disabled(atrium):
    for drive in (one_by_one(2), batches(4)):
        _, _, s = pair(atrium, 96, 54, drive, options=WAVEFRONT, sun_shadow_enabled=0)
        assert s.rays[rr.RAY_SUN_SHADOW] == 0


def test_lights_enabled_takes_the_same_kernels():
    """with lights the light rays add to the same radiance behind the sun rays (rgen:63-122, in that order): both settings run the
    sun kernels that add their term themselves"""
    scene = rr.scenes.sponza_class_scene(detail=0.12, tex_size=32, with_spheres=True, num_lights=48, sphere_subdivisions=2)
    for drive in (one_by_one(2), batches(6)):
        for options in ({}, WAVEFRONT):
            _, _, s = pair(scene, 128, 72, drive, options=options, mask=rr.PASS_ALL, lights_enabled=1)
            assert s.rays[rr.RAY_LIGHT_SHADOW] > 0 and s.sun_grid_cells > 0


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
