"""-m gpu: rays that start far from small geometry lying in a coordinate plane (a floor at z = 0 seen from thousands of units away).
The builders pad a box by 1e-4 + 1e-5 |coord| - an absolute amount near a coordinate plane - while the rounding of the node test
and of the triangle test grows with the distance to the ray's origin; from a few thousand units on a node test that does not
allow for it culls triangles the triangle test accepts, the floor gets pin-holes, and what shows through depends on the tree
(DESIGN.md "Arithmetic contract"). The reference is the oracle's brute force over all triangles - no tree, no boxes - and every
comparison is bit for bit."""
import functools

import numpy as np
import pytest

import oracle_api as oa
import rust_renderer_amd as rr
from util import FAR_DISTANCES, FAR_SCENES, far_rays, far_scene, run_frames

pytestmark = pytest.mark.gpu

N_RAYS = 40_000
MISS = 0xFFFFFFFF
TREES = [0, 1, 2, "refit"]  # option device_build 0 / 1 / 2, and the host tree refitted after the wall (mesh 1) was moved into place


@functools.lru_cache(maxsize=None)
def _brute(kind):
    return far_scene(kind).upload(oa.OracleRenderer(8, 8, brute_force=True))


@functools.lru_cache(maxsize=None)
def _reference(kind, distance, normalised):
    """the rays of one (scene, distance) case and what brute force answers: computed once, shared by the four trees, never written to"""
    rays = far_rays(kind, distance, N_RAYS, 3000 + 1000 * normalised + 16 * FAR_SCENES.index(kind) + FAR_DISTANCES.index(distance), normalised)
    tuv, mesh, prim = _brute(kind).trace_closest(rays)
    for a in (rays, tuv, mesh, prim):
        a.setflags(write=False)
    return rays, tuv, mesh, prim


@functools.lru_cache(maxsize=None)
def _gpu(kind, tree):
    r = rr.Renderer(8, 8, device=0)
    if tree == "refit":
        far_scene(kind, wall_moved=True).upload(r)
        r.set_instance_transform(1, rr.identity3x4())
        r.rebuild_tlas()
    else:
        r.set_option("device_build", tree)
        far_scene(kind).upload(r)
    return r


def _compare(kind, distance, tree, normalised):
    rays, tuv, mesh, prim = _reference(kind, distance, normalised)
    front = int((mesh == 0).sum())
    gpu = _gpu(kind, tree)
    tg, mg, pg = gpu.trace_closest(rays)
    differ = (tg.view(np.uint32) != tuv.view(np.uint32)).any(axis=1) | (mg != mesh) | (pg != prim)
    print(f"{kind} D={distance:g} tree={tree} normalised={normalised}: brute force hits mesh 0 with {front} of {N_RAYS} rays; the GPU differs on {int(differ.sum())}, "
          f"misses {int(((mg == MISS) & (mesh != MISS)).sum())} outright")
    assert front >= 0.3 * N_RAYS, "the rays must hit the surface they are aimed at, or the comparison is vacuous"
    assert np.array_equal(mg, mesh) and np.array_equal(pg, prim)
    assert np.array_equal(tg.view(np.uint32), tuv.view(np.uint32)), "t / u / v must equal brute force bit for bit"
    assert np.array_equal(gpu.trace_any(rays).astype(bool), mesh != MISS)


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("distance", FAR_DISTANCES)
@pytest.mark.parametrize("kind", FAR_SCENES)
def test_far_rays_keep_every_hit(kind, distance, tree):
    _compare(kind, distance, tree, False)


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("distance", [d for d in FAR_DISTANCES if d <= 3e3])
@pytest.mark.parametrize("kind", FAR_SCENES)
def test_far_rays_with_unit_directions_keep_every_hit(kind, distance, tree):
    """t is about the distance here, not about 1, and tmax = 10000 is a bound that could cut"""
    _compare(kind, distance, tree, True)


def _far_view_scene():
    """the grid floor with its wall one unit behind, from 5,000 units above its centre; the vertical field of view just frames the
    unit square (2 atan(0.5 / 5000)), so at 4:3 the wall shows beside it"""
    from rust_renderer_amd.camera import Camera
    scene = far_scene("grid")
    scene.camera = Camera((0.5, 0.5, 5000.0), (0.5, 0.5, 0.0), float(np.degrees(2.0 * np.arctan(0.5 / 5000.0))), 64 / 48, 1.0, 10000.0)
    scene.view_flags = dict(lights_enabled=0, sky_enabled=0)
    return scene


@functools.lru_cache(maxsize=None)
def _far_view_reference():
    W, H = 64, 48
    scene = _far_view_scene()
    cpu = scene.upload(oa.OracleRenderer(W, H, brute_force=True))
    run_frames(cpu, scene, W, H, 2, rr.PASS_ALL)
    pos, acc = cpu.read_gbuffer_position(), cpu.read_accumulation()
    for a in (pos, acc):
        a.setflags(write=False)
    return pos, acc, list(cpu.get_stats().rays)


@pytest.mark.parametrize("grids", [True, False])
def test_frames_of_a_floor_seen_from_far_away(grids):
    """two frames of every pass: G-buffer positions, accumulation and ray counts of the brute-force oracle, bit for bit - through the
    camera grid and the sun grid (default options), which have conservativeness assumptions of their own, and through the tree walk
    alone"""
    W, H = 64, 48
    pos, acc, rays = _far_view_reference()
    scene = _far_view_scene()
    gpu = rr.Renderer(W, H, device=0)
    if not grids:
        gpu.set_option("sun_grid", 0)
        gpu.set_option("camera_grid", 0)
    scene.upload(gpu)
    run_frames(gpu, scene, W, H, 2, rr.PASS_ALL)
    on_floor = int((np.abs(pos[..., 2]) < 0.5).sum())  # the wall is at z = -1
    gp = gpu.read_gbuffer_position()
    print(f"grids={grids}: G-buffer positions differ in {int((gp.view(np.uint32) != pos.view(np.uint32)).any(axis=-1).sum())} of {W * H} pixels; "
          f"rays {list(gpu.get_stats().rays)} against {rays}")
    assert on_floor >= 0.3 * W * H, "the view must show the floor"
    assert np.array_equal(gp.view(np.uint32), pos.view(np.uint32)), "G-buffer positions must equal the brute-force oracle's bit for bit"
    assert np.array_equal(gpu.read_accumulation().view(np.uint32), acc.view(np.uint32))
    assert list(gpu.get_stats().rays) == rays
