"""GPU: the glossy pass's persistent walks at frames where their waves refill. With option "trace_blocks_per_cu" = 1 a persistent grid
holds at most 65,536 lanes, so a queue of more rays than that is walked in several chunks per wave: k_glossy_trace takes the next ray
the moment a lane's walk ends and writes its hit record, and the sun rays go through k_rtgi_shadow on this pass's buffers. As
tests/test_gpu_walk_chunks.py does for the other walks, against the restatement (tests/glossy_reference.py)."""
import numpy as np
import pytest

import glossy_reference as gl
import rust_renderer_amd as rr
from test_gpu_glossy import World, integers, plain_deferred

pytestmark = pytest.mark.gpu

LANES = gl.WALK_LANES


def one_block_per_cu(world):
    world.gpu.set_option("trace_blocks_per_cu", 1)
    return world


def test_a_closed_box_of_three_grids_of_rays():
    """131 x 97 at 16 samples: every pixel casts, 203,312 samples of which the below ones never reach the walk; no ray misses, every sun
    ray is occluded, so every count is (0, 16, 0, 0)"""
    Ww, Hh = gl.WALK_BOX_SIZE
    w = one_block_per_cu(World(gl.inward_box_scene(), Ww, Hh))
    v = w.view()
    w.render(v, rr.HYBRID_FRAME, samples=16, blur_radius=1)
    plain = w.gpu.read_hybrid(rr.HYBRID_DEFERRED_OUTPUT)
    w.render(v, samples=16, blur_radius=1)
    got = w.check(v, plain)
    s = w.gpu.glossy_stats()
    print(integers(s))
    assert s.pixels == Ww * Hh and s.rays + s.below == 16 * Ww * Hh and s.misses == 0
    assert LANES < s.rays <= 8 * LANES, "k_glossy_trace's waves take more than one chunk"
    assert (got["counts"] == (0, 16, 0, 0)).all()
    assert np.array_equal(got["deferred"].view(np.uint32), plain.view(np.uint32))


def test_an_emissive_box_at_three_samples():
    """263 x 167 at 3 samples: 131,763 samples, a chunk of 64 rays holds 21 pixels and a third of another; no ray misses, so every pixel
    is held bit for bit"""
    Ww, Hh = gl.WALK_EMISSIVE_SIZE
    w, t = one_block_per_cu(World(gl.emissive_box_scene(), Ww, Hh)), one_block_per_cu(World(gl.emissive_box_scene(), Ww, Hh))
    v = w.view()
    w.render(v, samples=3, blur_radius=3)
    got = w.check(v, plain_deferred(t, v))
    s = w.gpu.glossy_stats()
    print(integers(s))
    assert got["exact"].all() and s.misses == 0 and s.rays + s.below == 3 * s.pixels
    assert LANES < s.rays <= 8 * LANES
    assert got["counts"][..., gl.EMITTER].any() and 0 < s.shadow_rays


def test_the_sun_rays_of_the_gallery_refill_too():
    """the gallery at 163 x 101 and 16 samples: on the oracle's G-buffer 207,684 rays (3.2 grids) and 96,510 sun rays (1.5 grids), so
    k_rtgi_shadow's waves on this pass's buffers take a second chunk; sunlit, shadowed, dark, emitter and missed rays all occur
    (tests/test_glossy_cpu.py asserts the counts)"""
    Ww, Hh = gl.WALK_GALLERY_SIZE
    w, t = one_block_per_cu(World(gl.gallery_scene(), Ww, Hh)), one_block_per_cu(World(gl.gallery_scene(), Ww, Hh))
    v = w.view()
    w.render(v, samples=16, blur_radius=3, blur_roughness=gl.GALLERY_BLUR_ROUGHNESS)
    got = w.check(v, plain_deferred(t, v))
    s = w.gpu.glossy_stats()
    print(integers(s))
    assert LANES < s.rays <= 8 * LANES and LANES < s.shadow_rays <= 8 * LANES, "both walks refill"
    assert all((got["want"]["kind"] == k).any() for k in range(4)) and s.below > 0
